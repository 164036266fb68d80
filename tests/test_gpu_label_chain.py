"""GPU tests of the label mask's stages TOGETHER (include/umx.h and DESIGN.md section 8.1): sessions of many calls on one umx_labeler --
whose buffers the stages share, reuse and move -- against tests/label_chain_ref.py, the interpreter that composes the stages' own
restatements and keeps the resident state in numpy.  Every operation is compared as it happens.  Everything is an integer and
compared for equality: there is no tolerance anywhere in this file.  The sessions themselves are held to what they are for by
tests/test_label_chain_cpu.py."""
import os
import subprocess
import sys

import numpy as np
import pytest

import helpers
import label_chain_ref as ref
from unmicst_amd import driver, model, tiffio, umx

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = (ref.TALL, ref.ODD, ref.LITTLE)
IDS = ["%dx%d" % s for s in SHAPES]


def brief(v):
    if isinstance(v, np.ndarray):
        return "%s%s %s" % (v.dtype.names or v.dtype, v.shape, v.ravel()[:6].tolist())
    if isinstance(v, (tuple, list)):
        return [brief(x) for x in v]
    return v


def same_bytes(a, b):
    if isinstance(a, (tuple, list)):
        return isinstance(b, (tuple, list)) and len(a) == len(b) and all(same_bytes(x, y) for x, y in zip(a, b))
    if isinstance(a, np.ndarray):
        return isinstance(b, np.ndarray) and a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()
    return a == b


def walk(lb, session, named=None, what=""):
    """the session on the labeler, every operation against the interpreter as it happens; the counts of the last producer stand through
    everything that follows it (the informative `launches` / `recon_launches` are not among them) -> the results"""
    got, ctx, counts = [], {}, {}
    for i, (op, (args, want)) in enumerate(zip(session, ref.interpret(session, named=named))):
        g = ref.perform(lb, op, args, ctx)
        assert ref.equal(g, want), (what, i, op, brief(g), brief(want))
        if op[0] in ("run", "run_ptr"):
            counts = want[2]
        assert ref.counts_of(lb) == counts, (what, i, op, ref.counts_of(lb), counts)
        got.append(g)
    return got


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_the_commands_order_after_every_producer(shape):
    """(a) plain, grow, split, split + flood, hmax, hmax + flood + grow on one labeler, each followed by
    run -> shape -> contacts(0) -> relabel(pairs) -> shape -> hull -> measure -> relabel(keep) -> measure -> shape -> contacts(reach) -> hull
    and objects(), with one *_ptr consumer on a foreign plane of another shape after the first relabel"""
    umx.require_torch_runtime("test_gpu_label_chain")
    session = ref.chain_session(shape)
    assert {op[3] for op in session if op[0] == "run"} == set(ref.VARIANTS) and len(session) == 6 * (2 + len(ref.CHAIN))
    with umx.Labeler() as lb:
        walk(lb, session, what=shape)


@pytest.mark.parametrize("shape,variant", ref.PAIRS, ids=[v for _, v in ref.PAIRS])
def test_every_ordered_pair_of_consumers(shape, variant):
    """(b) measure, shape, contacts, hull, relabel(pairs), relabel(keep), objects: all 49 ordered pairs (A, B) after a run of the
    producer on one labeler, a *_ptr consumer on a foreign plane before each"""
    umx.require_torch_runtime("test_gpu_label_chain")
    session = ref.pair_session(shape, variant)
    assert len(session) == 4 * 49
    with umx.Labeler() as lb:
        walk(lb, session, what=variant)


@pytest.mark.parametrize("seed", ref.SEEDS)
def test_random_walk_and_its_replay(seed):
    """(c) a seeded walk over producers in all three forms, consumers, *_ptr consumers and refusals; the last producer and what follows
    it give the same bytes on a fresh labeler"""
    umx.require_torch_runtime("test_gpu_label_chain")
    session = ref.random_session(seed, ref.LENGTH)
    with umx.Labeler() as lb:
        got = walk(lb, session, what=seed)
    last, rest = ref.tail(session)
    with umx.Labeler() as fresh:
        again = walk(fresh, rest, what=(seed, "replay"))
    assert len(again) == len(got[last:]) and all(same_bytes(a, b) for a, b in zip(again, got[last:]))


def test_regrowth_session():
    """(d) the seven events that move the labeler's memory (tests/test_label_chain_cpu.py holds the session to them), a consumer before
    and after each"""
    umx.require_torch_runtime("test_gpu_label_chain")
    with umx.Labeler() as lb:
        walk(lb, ref.regrowth_session(), what="regrowth")


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_device_forms_equal_the_host_forms(shape):
    """(e) run_ptr on torch tensors and the *_ptr consumers on the plane it wrote give what run and the resident consumers give; the
    resident consumers are refused after a run_ptr"""
    umx.require_torch_runtime("test_gpu_label_chain")
    with umx.Labeler() as lb:
        for variant in ref.VARIANTS:
            session = ref.dev_session(shape, variant)
            got = walk(lb, session, what=(shape, variant))
            host = [want for _, want in ref.interpret([("run", "discs", shape, variant, True)] + ref.CHAIN)]
            assert len(session) == len(host) + 2 and [op[0] for op in session[-3:]] == ["shape", "relabel", "objects"]
            for op, g, h in zip(session[:len(host) - 1], got, host):
                if op[0] == "relabel_ptr":
                    assert (h[0] is None or np.array_equal(g[0], h[0])) and np.array_equal(g[1], h[2]) and g[2] == len(h[1]), (shape, variant, op)
                else:
                    assert ref.equal(g, h), (shape, variant, op)
            assert got[-3] is ref.REFUSED and got[-2] is ref.REFUSED and ref.equal(got[-1], host[0][1])   # objects(): still the run's table


def test_a_refused_run_keeps_the_counts_of_the_run_before():
    """a run that is refused (a class the planes do not have) has touched nothing: the resident labels serve, and split_counts(),
    flood_counts() and hmax_counts() are still those of the run before (the wrapper used to forget them before it made the call)"""
    sc = ref.scene("discs", ref.LITTLE)
    labels, table, counts = ref.produce("discs", ref.LITTLE, "hmax_flood_grow")
    with umx.Labeler() as lb:
        lb.run(sc.planes, **ref.run_kwargs(sc, "hmax_flood_grow"))
        assert ref.counts_of(lb) == counts and lb.split_counts() is not None and lb.flood_counts() is not None
        for variant in ("plain", "split", "split_flood", "hmax"):
            with pytest.raises(umx.UmxError) as e:
                lb.run(sc.planes, **dict(ref.run_kwargs(sc, variant), cls=4))
            assert e.value.code == umx.ERR_INVALID
            assert ref.counts_of(lb) == counts and lb.split_counts() is not None and lb.flood_counts() is not None
        assert ref.equal(lb.objects(), table) and len(lb.shape()) == len(table)
        lb.run(sc.planes, **ref.run_kwargs(sc, "plain"))
        assert lb.split_counts() is None and lb.flood_counts() is None and lb.hmax_counts() is None


_GUARD_CHILD = """
import sys
sys.path.insert(0, %r); sys.path.insert(0, %r)
import label_chain_ref as ref
import test_gpu_label_chain as t
from unmicst_amd import umx
umx.require_torch_runtime("test_gpu_label_chain")
with umx.Labeler() as lb:                                  # (an operation raises UmxError 7 when a red zone was written)
    t.walk(lb, ref.chain_session(ref.ODD), what="chain")
with umx.Labeler() as lb:
    t.walk(lb, ref.regrowth_session(), what="regrowth")
print("guard-ok")
"""


def test_guard_mode_finds_no_write_outside_the_buffers():
    """(f) UMX_DEBUG_GUARD=0xa5 in a child process: red zones round every buffer of the labeler, checked at the end of every call.  The
    commands' order after all six producers at the odd width and the regrowth session: every call returns UMX_OK (or the expected
    refusal) and the right answer."""
    env = dict(os.environ, UMX_DEBUG_GUARD="0xa5")
    r = subprocess.run([sys.executable, "-c", _GUARD_CHILD % (ROOT, os.path.join(ROOT, "tests"))], env=env, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0 and "guard-ok" in r.stdout, r.stderr[-2000:]


MERGE = 0.3
KEEP = ("area>=40", "eccentricity<=0.85", "solidity>=0.8", "pm2_mean>=90")
SEEDS_FLAGS = {"hmax_flood_grow": ["--labelHmax", str(ref.HMAX)], "split_flood_grow": ["--labelSplit", "2"]}


@pytest.mark.parametrize("variant", sorted(SEEDS_FLAGS))
def test_command_with_every_label_flag(tmp_path, variant):
    """(g) UnMicst.py --stackOutput --labelMask on the 150 x 171 crop of sample 105 with every label flag at once: --labelHmax (or
    --labelSplit) / --labelFlood / --labelGrow, --labelMerge, --labelKeep with a rule on the area, on a Shapes column, on a Hulls column
    and on a pm intensity, --labelMeasure, --labelShape, --labelNeighbors with a reach, --labelHull with its vertices.  The Labels,
    Objects, Intensities, Shapes, Neighbors, Hulls and HullVertices files are, byte for byte, what the driver's writers make of the
    interpreter's results on the probability pages the same run wrote, and the relabel line has the restated numbers.  MERGE and KEEP
    were chosen on the restatement of this crop's pages: the merge joins some objects and not all, every rule has objects on both of
    its sides, the keep drops some and not all (asserted below before any file is compared; no condition had to be relaxed)."""
    hp, blob, mean, std = helpers.load_nuclei_dapi()
    models = tmp_path / "models"
    model.save_converted(model.ModelArtefacts(hp, blob, mean, std), str(models / "nucleiDAPI"))
    raw = np.ascontiguousarray(helpers.load_sample_105()[0][300:450, 200:371])
    reg = tmp_path / "x" / "registration"
    os.makedirs(reg)
    img = str(reg / "crop.tif")
    tiffio.imsave(img, raw)
    env = {k: v for k, v in os.environ.items() if k != "UMX_HIP_RUNTIME"}
    env["UMX_MODELS_DIR"] = str(models)
    out = str(tmp_path / "out")
    flags = (["--labelMask"] + SEEDS_FLAGS[variant] + ["--labelFlood", "1", "--labelFloodStep", str(ref.STEP), "--labelGrow", str(ref.GROW),
             "--labelMerge", str(MERGE), "--labelKeep"] + list(KEEP) + ["--labelMeasure", "--labelShape", "--labelNeighbors",
             "--labelNeighborsReach", str(ref.REACH), "--labelHull", "--labelHullVertices"])
    r = subprocess.run([sys.executable, os.path.join(ROOT, "UnMicst.py"), img, "--model", "nucleiDAPI", "--stackOutput", "--outputPath", out] + flags,
                       env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    pages = tiffio.imread_all(os.path.join(out, "crop_Probabilities_1.tif"))
    assert pages.shape == (3, 150, 171) and pages.dtype == np.uint8 and raw.dtype == np.uint16
    name = "crop " + variant
    ref.EXTRA_SCENES[name] = ref.Scene(np.ascontiguousarray(pages[::-1]), 2, 1, (1,), 2, 1, 2)     # the pages are in reversed class order
    try:
        chain = ref.chain(("driver", MERGE), ("rules", KEEP))
        session = [("run", name, (150, 171), variant, True)] + chain[:8] + [("measure", ("named", "ch0"))] + chain[8:11]
        want = [w for _, w in ref.interpret(session, named={"ch0": raw[None]})]
    finally:
        del ref.EXTRA_SCENES[name]
        ref.scene.cache_clear()
        ref.produce.cache_clear()
    N0, N1, (labels, table, keep_map) = len(want[0][1]), len(want[3][1]), want[7]
    N2 = len(table)
    print("command %s: %d objects, %d merged away, %d dropped, %d left" % (variant, N0, N0 - N1, N1 - N2, N2))
    assert 0 < N0 - N1 < N0 - 1 and 0 < N2 < N1                      # the merge joins some and not all, the keep drops some and not all
    assert "Label relabel: %d objects from %d (%d dropped, %d merged away)" % (N2, N0, N1 - N2, N0 - N1) in r.stdout, r.stdout[-2000:]
    pm, ch0, shapes, contacts, (hulls, vertices) = want[8], want[9], want[10], want[11], want[12]
    mine = tmp_path / "mine"
    os.makedirs(mine)
    tiffio.imsave(str(mine / "crop_Labels_1.tif"), labels, append=False)
    driver.write_objects_csv(str(mine / "crop_Objects_1.csv"), table)
    driver.write_intensities_csv(str(mine / "crop_Intensities_1.csv"), table, [("pm%d" % k, pm[k]) for k in range(len(pm))] + [("ch0", ch0[0])])
    driver.write_shapes_csv(str(mine / "crop_Shapes_1.csv"), table, shapes)
    driver.write_neighbors_csv(str(mine / "crop_Neighbors_1.csv"), contacts)
    driver.write_hulls_csv(str(mine / "crop_Hulls_1.csv"), table, hulls, vertices)
    driver.write_hull_vertices_csv(str(mine / "crop_HullVertices_1.csv"), hulls, vertices)
    assert len(os.listdir(mine)) == 7 and len(contacts) > 0 and len(vertices) > 3 * N2
    for f in sorted(os.listdir(mine)):
        assert open(os.path.join(out, f), "rb").read() == open(mine / f, "rb").read(), f
