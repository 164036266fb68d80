"""The evidence tools that turn rocprofv3 databases into the tables under profiles/ (tools/summarize_rocprof.py,
tools/timeline_rocprof.py), run on a small hand-made rocpd-shaped database: grouping by (kernel, grid), the demangling of names
rocprofv3 leaves mangled, and the per-stream time line of the last step.

The shell tools (tools/*.sh) without a GPU: `step` (tools/gpu_step.sh) ends the calling script at the first command that fails or
runs into its time limit, tools/gpu_ab.sh does not start a variant after one that failed, and every script starts what opens the
GPU through `step`."""
import csv
import glob
import os
import re
import sqlite3
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOLS = os.path.join(ROOT, "tools")


def _db(path):
    c = sqlite3.connect(path)
    c.execute("create table kernels (name text, start integer, end integer, duration integer, grid_x integer, grid_y integer, "
              "grid_z integer, workgroup_x integer, lds_size integer, vgpr_count integer, accum_vgpr_count integer, stream_id integer)")
    rows, t = [], 1000
    for step in range(3):
        for name, dur, gx, stream in [("void umx::conv_f16x3<9, 4, 1>(umx::HConvParams)", 700, 256 * 32, 1),
                                      ("_ZN3umx16split_dyn_kernelEPKfmiiPKjPfPDF16_S5_PiPj", 40, 256 * 4096, 1),
                                      ("void umx::wgrad_f16x3<true>(umx::WgradParams)", 250, 256 * 171, 2),
                                      ("void at::native::elementwise_kernel<128>(int)", 5, 256, 1),
                                      ("void umx::softmax_loss_kernel(float const*)", 11, 256 * 1024, 1)]:
            rows.append((name, t, t + dur, dur, gx, 1, 1, 256, 80000, 128, 0, stream))
            t += dur + (7 if stream == 1 else 0)
    c.executemany("insert into kernels values (?,?,?,?,?,?,?,?,?,?,?,?)", rows)
    c.commit()
    c.close()


def test_summary_groups_by_kernel_and_grid_and_demangles(tmp_path):
    db = str(tmp_path / "run_results.db")
    _db(db)
    out = str(tmp_path / "by_kernel.csv")
    subprocess.run([sys.executable, os.path.join(ROOT, "tools", "summarize_rocprof.py"), db, "-o", out], check=True)
    rows = list(csv.DictReader(open(out)))
    names = {r["kernel"] for r in rows}
    assert "umx::split_dyn_kernel" in names                       # (left mangled by rocprofv3: _Float16 parameters)
    assert not any("elementwise" in n for n in names)             # only umx:: kernels unless --all
    conv = next(r for r in rows if r["kernel"].startswith("umx::conv_f16x3"))
    assert conv["calls"] == "3" and conv["workgroups_x"] == "32" and float(conv["avg_us"]) == 0.7


def test_time_line_of_the_last_step_with_streams(tmp_path):
    db = str(tmp_path / "run_results.db")
    _db(db)
    out = str(tmp_path / "tl.txt")
    subprocess.run([sys.executable, os.path.join(ROOT, "tools", "timeline_rocprof.py"), db, "-o", out], check=True)
    text = open(out).read().splitlines()
    body = [l for l in text if l and not l.startswith("#") and not l.lstrip().startswith("start_us")]
    assert len(body) == 5                                          # the dispatches between the last two loss kernels
    assert body[-1].split()[4].startswith("umx::softmax_loss_kernel")
    streams = {l.split()[3] for l in body}
    assert streams == {"1", "2"}
    busy = [l for l in text if l.startswith("# stream")]
    assert len(busy) == 2 and busy[0].startswith("# stream 1")     # sorted by busy time


def run_script(tmp_path, body):
    """a script that sources gpu_step.sh, runs `body` and then echoes `after` -> (status, stdout, stderr)"""
    script = tmp_path / "s.sh"
    script.write_text(". %s\necho before\n%s\necho after\n" % (os.path.join(TOOLS, "gpu_step.sh"), body))
    r = subprocess.run(["bash", str(script)], capture_output=True, text=True, timeout=60)
    return r.returncode, r.stdout.split(), r.stderr


def test_step_lets_the_script_continue_after_a_command_that_passes(tmp_path):
    status, out, err = run_script(tmp_path, "step 5 true")
    assert status == 0 and out == ["before", "after"] and err == ""


def test_step_ends_the_script_with_the_status_of_a_command_that_fails(tmp_path):
    marker = tmp_path / "ran"
    status, out, err = run_script(tmp_path, "step 5 false\ntouch %s" % marker)
    assert status == 1 and out == ["before"] and not marker.exists()
    assert "status 1" in err and "false" in err
    status, out, err = run_script(tmp_path, "step 5 sh -c 'exit 7'\ntouch %s" % marker)
    assert status == 7 and out == ["before"] and not marker.exists()


def test_step_ends_the_script_with_124_at_the_time_limit(tmp_path):
    marker = tmp_path / "ran"
    status, out, err = run_script(tmp_path, "step 1 sleep 5\ntouch %s" % marker)
    assert status == 124 and out == ["before"] and not marker.exists()
    assert "status 124" in err and "sleep 5" in err


def test_step_leaves_redirections_to_the_caller(tmp_path):
    log = tmp_path / "x.log"
    status, out, err = run_script(tmp_path, "step 5 echo hello > %s 2>&1" % log)
    assert status == 0 and out == ["before", "after"] and log.read_text() == "hello\n"


def test_gpu_ab_does_not_start_a_variant_after_one_that_failed(tmp_path):
    variants = tmp_path / "v.txt"
    variants.write_text("first | UMX_X=1 | --steps 1\nsecond | | --steps 1\n")
    env = dict(os.environ, PYTHON="/bin/false")
    # (the script works from the directory above its own: a stand-in root that links to the tools and holds nothing else, so that
    # the logs land in tmp_path)
    os.symlink(TOOLS, tmp_path / "tools")
    r = subprocess.run(["bash", str(tmp_path / "tools" / "gpu_ab.sh"), "ab", str(variants)], capture_output=True, text=True, env=env, timeout=60)
    assert r.returncode != 0
    assert len(list(tmp_path.rglob("ab/first.log"))) == 1
    assert not list(tmp_path.rglob("second.log"))
    assert "first" in r.stderr and "second" not in r.stdout + r.stderr


def tool_scripts():
    return sorted(glob.glob(os.path.join(TOOLS, "*.sh")))


def test_every_gpu_command_of_the_tool_scripts_goes_through_step():
    gpu = re.compile(r"bench\.py|rocprofv3|pytest|tools/probes/")
    checked = 0
    for path in tool_scripts():
        if os.path.basename(path) in ("asan.sh", "gpu_step.sh"):
            continue
        text = open(path).read()
        assert re.search(r"^\. tools/gpu_step\.sh$", text, re.M), path
        for n, line in enumerate(text.split("\n"), 1):
            code = line.split("#", 1)[0] if line.lstrip().startswith("#") else line
            if not gpu.search(code):
                continue
            assert re.match(r"\s*step \d+ ", code), "%s:%d starts a GPU command outside step: %s" % (path, n, line)
            checked += 1
    assert checked >= 4   # (the four scripts each start at least one)


def test_no_tool_script_is_numbered_by_round_session_or_call():
    assert len(tool_scripts()) >= 5
    for path in tool_scripts():
        name = os.path.basename(path)
        assert not re.search(r"\d", name), name
        assert not re.search(r"(^|_)(r|round|session|call|visit)\d*(_|\.)", name), name
