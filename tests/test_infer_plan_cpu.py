"""The split-precision plan of the inference engine (plan_model, umx_plan.hip) through umx_test_infer_plan: no device needed.  Every
launch of the shipped hyper-parameter sets with and without the F6 form, of the switches test's graph under each planner switch, of
the depth-to-space shapes, of the workgroup-order graph and of the fuzz sets of tests/test_plan_check_cpu.py, against
tests/golden/infer_plan_lines.json: the lines recorded from plan_model and run_launch_f16 as they stood while the planner still read its
switches from the environment and the launch path formed the kernel name and the workgroup order (a copy of that commit with a
recording entry added -- it sets the corresponding environment variables, runs that commit's plan_model, formats the "[umx plan]"
text, the kernel name and the order rule with that commit's statements copied verbatim and hashes with the same serialisation -- run on
a CPU).

A line is the launch's UMX_DEBUG_PLAN text (a dense-K first layer: both lines, joined by " | "), then " || " and the kernel
instantiation as a profile names it, the destination buffer's layout, the N-tiles per workgroup, the weight shift, a 64-bit FNV-1a
digest of everything the upload sends (infer_digest) and, for every batch n of BATCHES, "n:<workgroup order>/<tiles per XCD>" as a
launch on n tiles chooses them (launch_shape).  A model the planner refuses is recorded as the refusal's text."""
import json
import os
import re

import pytest

from test_gpu_switches import D2S_SHAPES, HP, SWITCHES
from test_plan_check_cpu import _random_hps
from unmicst_amd import model, umx

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "infer_plan_lines.json")
BATCHES = (5, 64, 70, 255, 278, 320)
# tests/test_gpu_switches.py::test_workgroup_order_2_is_chosen_by_rule: 160 / 320 output channels, layers of 2 and 3 N-blocks
ORDER2_HP = model.HParams(model.GRAPH_V2, 32, 2, 3, 40, 3, 3, 0, 2)
ORDER2_SEED = 2
PLANNER_VARS = {"UMX_PLAN_NT": "nt", "UMX_PLAN_OVERRIDE": "override", "UMX_DEBUG_STAMPS": "stamps"}


def cases():
    """id -> (hp, f6, act_shift, blob seed, switches as keyword arguments of umx.infer_plan)"""
    out = {}
    for key, hp in model.KNOWN_HP.items():
        for f6 in (False, True):
            out["%s f6=%d" % (key, f6)] = (hp, f6, 0, 21, {})
    for env in SWITCHES:   # (as the default engine of that test plans it: the F6 form allowed, its blob)
        kw = {PLANNER_VARS[k]: v for k, v in env.items() if k in PLANNER_VARS}
        if env and not kw and "UMX_ACT_SHIFT" not in env:
            continue
        name = ",".join("%s=%s" % kv for kv in env.items()) or "default"
        out["switches " + name] = (HP, True, int(env.get("UMX_ACT_SHIFT", 0)), 9, kw)
    out["switches UMX_DEBUG_STAMPS=lu0.conv"] = (HP, True, 0, 9, {"stamps": "lu0.conv"})
    for n0, C, ks, S in D2S_SHAPES:
        out["d2s n%d_c%d_k%d_s%d" % (n0, C, ks, S)] = (model.HParams(model.GRAPH_V2, S, C, 3, n0, 2, ks, 0, 2), False, 0, 40 + n0, {})
    out["order2"] = (ORDER2_HP, True, 0, ORDER2_SEED, {})
    for i, hp in enumerate(_random_hps(14, 2026)):
        out["fuzz %d" % i] = (hp, True, 0, 21, {})
    return out


def plan_of(case, plan=None, **more):
    """the lines of one case, or the refusal's text"""
    hp, f6, act_shift, seed, kw = case
    try:
        return (plan or umx.infer_plan)(hp, f6, act_shift, model.random_blob(hp, seed=seed), batches=BATCHES, **kw, **more)
    except umx.UmxError as e:
        return str(e)


@pytest.fixture(scope="module")
def lines():
    return {name: plan_of(c) for name, c in cases().items()}


_LINE = re.compile(r"^\[umx plan\] (\S+) +((?:fused-phase |packed |fp6-cross )*)NT (\d+) x (\d+) blocks, OC \d+ x \d halo slot\(s\), S \d+, LDS \d+ B, "
                   r"k-steps \d+, wshift -?\d+( \| \[umx plan\] \S+ +dense-K first layer: [^|]*)? \|\| (conv_\w+<[^>]*>), dst f32 (\d) planar (\d) "
                   r"Cs (\d+), nt16 (\d+), wshift (-?\d+), digest ([0-9a-f]{16}),((?: \d+:\d/\d+)+)$")


def _parsed(plan):
    for ln in plan:
        m = _LINE.match(ln)
        assert m, ln
        name, form, nt, nblocks, first, kernel, f32, planar, Cs, nt16, wshift, digest, shapes = m.groups()
        yield dict(name=name, form=form, nblocks=int(nblocks), first=bool(first), kernel=kernel, targs=kernel[kernel.index("<") + 1:-1].split(", "),
                   digest=digest, shapes={int(n): (int(o), int(t)) for n, o, t in re.findall(r"(\d+):(\d)/(\d+)", shapes)})


def test_plans_are_the_recorded_ones(lines):
    with open(GOLDEN) as f:
        want = json.load(f)
    assert sorted(lines) == sorted(want)
    wrong = {k: (lines[k], want[k]) for k in want if lines[k] != want[k]}
    assert not wrong, list(wrong.items())[:3]


def test_the_threaded_weight_fill_writes_the_same_images(lines):
    """nucleiDAPILAMIN's weight images are large enough to take the threaded fill: one thread and the default count, equal digests"""
    one = plan_of(cases()["nucleiDAPILAMIN f6=1"], threads=1)
    assert [p["digest"] for p in _parsed(one)] == [p["digest"] for p in _parsed(lines["nucleiDAPILAMIN f6=1"])]


def test_workgroup_order_2_from_the_host_alone(lines):
    """What tests/test_gpu_switches.py::test_workgroup_order_2_is_chosen_by_rule and tests/test_gpu_infer_guard.py's twin establish on the
    device: at 278 and 320 images at least two launches of the graph take order 2, at 5 and 70 none does (70 images are 18 workgroup
    tiles of the 8 x 8-pixel layers, not 70); and no launch in the F6 form takes order 2 at any batch."""
    plan = list(_parsed(lines["order2"]))
    for n in (278, 320):
        assert sum(1 for p in plan if p["shapes"][n][0] == 2) >= 2, n
    for n in (5, 70):
        assert all(p["shapes"][n][0] == 1 for p in plan), n
    f6 = [p for plan in lines.values() if not isinstance(plan, str) for p in _parsed(plan) if p["form"] == "fp6-cross "]
    assert f6 and all(order == 1 for p in f6 for order, _ in p["shapes"].values())


def test_the_cases_reach_every_form(lines):
    reached = set()
    for name, plan in lines.items():
        if isinstance(plan, str):
            reached.add("refused")
            continue
        folded = any(p["first"] for p in _parsed(plan))   # (the graph keeps the raw-skip fold only with a dense-K first layer)
        for p in _parsed(plan):
            a = p["targs"]
            if p["first"]:
                reached.add("dense-K first")
                continue
            fold = " with the fold" if folded else " without the fold"
            reached.add("fold" if folded else "no fold")
            if "packed " in p["form"]:
                reached.add("packed")
            if "fused-phase " in p["form"]:
                reached.add("fused-phase" + fold)
            if a[6] == "true":
                reached.add("depth-to-space" + fold)
            if "convT" in p["name"] and a[2] == "1" and a[6] == "false":
                reached.add("per-phase" + fold)
            if p["form"] == "fp6-cross ":
                reached.add("fp6-cross")
            for order, _ in p["shapes"].values():
                reached.add("order %d" % order)
    need = ["dense-K first", "fold", "no fold", "packed", "fused-phase with the fold", "fused-phase without the fold", "depth-to-space with the fold",
            "depth-to-space without the fold", "per-phase with the fold", "per-phase without the fold", "fp6-cross", "order 1", "order 2", "refused"]
    assert [f for f in need if f not in reached] == []
    # 278 images on the order-2 graph's 8 x 8-pixel layers (4 images a workgroup tile): 70 tiles over 8 XCDs, 9 a piece -- not a divisor
    assert any(p["shapes"][278] == (2, 9) for p in _parsed(lines["order2"]))


def test_the_trainers_plan_does_not_follow_the_environment(monkeypatch):
    """tconv_plan reaches plan_f16 with the switches its caller hands it; umx_test_train_plan hands it none.  (CytoplasmIncell's ld0 has
    two N-tiles per workgroup: while plan_f16 read the variable itself, these lines changed with it.)"""
    hp = model.KNOWN_HP["CytoplasmIncell"]
    blob = model.random_blob(hp, seed=21)
    base = umx.train_plan(hp, 8, blob)
    monkeypatch.setenv("UMX_PLAN_NT", "ld0:1")
    assert umx.train_plan(hp, 8, blob) == base
