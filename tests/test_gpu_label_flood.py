"""GPU tests of the label mask's level flood (unmicst_amd/csrc/umx_label.hip; include/umx.h and DESIGN.md section 8.1, steps 19 to 21):
the labels, every field of the table and the counts of umx_labeler_run_flood / _run_flood_dev against tests/label_flood_ref.py, compared
for equality.  Everything is an integer: there is no tolerance anywhere in this file.  `launches` is informative and is only held
to bounds that follow from the definition of the host loop, never to a figure."""
import ctypes
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
from scipy import ndimage

import helpers
import label_flood_ref as ref
import label_measure_ref
import label_ref
import label_shape_ref
import label_split_ref
from unmicst_amd import model, tiffio, umx

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

T, HALO = umx.LABEL_GROW_TILE, umx.LABEL_GROW_HALO
TALL, WIDE = (2 * T + 2, 2 * T + 22), (T + 6, 3 * T + 8)      # 130 x 150 and 70 x 200: the seams at 64 and 128 fall inside necks
LITTLE = (40, 50)                                            # smaller than a tile
# (column of the ridge, its offset in the bar): on the seam's two sides, in the first and the last column of a halo ring, inside one
RIDGES = {TALL: [(T - HALO, 0), (T - 4, 1), (T - 1, 2), (T, 3), (T + 1, 4), (T + HALO - 1, 5), (T + HALO, 6),
                 (2 * T - 1, 7), (2 * T, 8), (2 * T, 4), (2 * T - 1, 3)],
          WIDE: [(T - 1, 2), (T, 3), (T + 1, 4), (T - HALO, 0), (2 * T - 1, 3), (2 * T, 4), (2 * T + 1, 5), (2 * T - HALO, 8)],
          LITTLE: [(25, 3)]}


@functools.lru_cache(maxsize=None)
def scene(shape, name):
    """-> (planes, D, C, P, invert, R).  A name ending in "^T" is the scene of the transposed shape, transposed: its necks run down
    the image and cross the seams between tile rows."""
    if name.endswith("^T"):
        planes, D, C, P, invert, R = scene(shape[::-1], name[:-2])
        planes = np.ascontiguousarray(planes.transpose(0, 2, 1))
        planes.setflags(write=False)
        return planes, D, C, P, invert, R
    H, W = shape
    D, C, P, invert, R, rim, inverted = ref.DEPTH, 1, 1, False, 0, None, False
    if name == "ridges":
        mask, relief, _ = ref.ridge_scene(H, W, RIDGES[shape])
    elif name == "two_values":
        mask, relief, _ = ref.ridge_scene(H, W, RIDGES[shape], low=3)
        relief = np.where(relief > 3, 200, relief)
    elif name == "corridor":
        mask, relief, _ = ref.corridor_scene(H, W)
    elif name.startswith("trap"):
        mask, relief = ref.trap_scene(H, W, int(name[5:7]), int(name[8:10]))
    elif name == "blobs":
        (mask, relief), C = ref.blob_scene(H, W), 5
    elif name == "inverted":
        (mask, relief), C, P, invert, inverted = ref.blob_scene(H, W), 5, 2, True, True
    elif name.startswith("rim"):
        mask, relief, _ = ref.ridge_scene(H, W, RIDGES[shape])
        rim, R = ndimage.binary_dilation(mask, iterations=3), int(name[3:])
    elif name == "full":
        mask, relief = np.ones((H, W), bool), np.random.default_rng(8).integers(0, 255, (H, W))
    elif name == "empty":
        mask, relief = np.zeros((H, W), bool), np.zeros((H, W), np.int64)
    else:
        raise KeyError(name)
    planes = ref.planes_of(mask, relief, rim, inverted)
    planes.setflags(write=False)
    return planes, D, C, P, invert, R


@functools.lru_cache(maxsize=None)
def want(shape, name, q):
    """(labels, table, counts): the restatement, computed once per case and never changed"""
    planes, D, C, P, invert, R = scene(shape, name)
    labels, table, counts = ref.split_flood(planes, 2, 1, D, C, P, q, invert, R, (1,) if R else None)
    labels.setflags(write=False)
    table.setflags(write=False)
    return labels, table, counts


@pytest.fixture(scope="module")
def lab():
    with umx.Labeler() as lb:
        yield lb


def kwargs_of(shape, name, q):
    planes, D, C, P, invert, R = scene(shape, name)
    return dict(grow=R, grow_classes=(1,) if R else None, split=D, split_core=C, flood=P, flood_step=q, flood_invert=invert)


def same(got_labels, got_table, lab, wanted, what):
    labels, table, counts = wanted
    if got_labels is not None:
        assert got_labels.dtype == np.int32 and got_labels.shape == labels.shape
        assert np.array_equal(got_labels, labels), (what, int((got_labels != labels).sum()))
    assert len(got_table) == len(table), (what, len(got_table), len(table))
    for f in label_ref.FIELDS:
        assert np.array_equal(got_table[f], table[f]), (what, f)
    got = dict(lab.flood_counts())
    launches = got.pop("launches")
    assert got == counts, (what, got, counts)
    assert lab.split_counts() == {k: counts[k] for k in label_split_ref.COUNTS}
    # every launch but the last of a level claims a pixel, and a level is entered only when a pixel waits for it or it is the first:
    # at most one launch per pixel claimed, one more per level that claimed and one for the first level; a level that claims has a launch
    assert counts["levels_claimed"] <= launches <= counts["claimed"] + counts["levels_claimed"] + 1, (what, launches)
    return launches


def check(lab, shape, name, q):
    planes = scene(shape, name)[0]
    kw = kwargs_of(shape, name, q)
    a = lab.run(planes, 2, 1, **kw)
    launches = same(a[0], a[1], lab, want(shape, name, q), (shape, name, q))
    counts = lab.flood_counts()
    b = lab.run(planes, 2, 1, **kw)                           # twice: the same bytes
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and lab.flood_counts() == counts
    return launches


def test_the_inputs_are_what_they_are_for():
    """asserted on the restatement alone: every pair is cut on its ridge; the ridges stand on the seams and in the halo rings; the
    corridor is long; the trap's chamber goes to the lower gate"""
    assert TALL == (130, 150) and WIDE == (70, 200)
    for shape in (TALL, WIDE, LITTLE):
        mask, relief, placed = ref.ridge_scene(*shape, RIDGES[shape])
        labels, table, counts = want(shape, "ridges", 16)
        assert counts["n_objects"] == 2 * counts["n_before"] == 2 * len(RIDGES[shape]) and counts["unreached"] == 0
        for top, bx, off, value in placed:
            a, b = labels[top, bx - 1], labels[top, bx + ref.LENGTH]
            assert 0 < a < b and (labels[top:top + 4, bx:bx + off + 1] == a).all() and (labels[top:top + 4, bx + off + 1:bx + ref.LENGTH] == b).all()
        assert want(shape, "two_values", 1)[2]["levels_claimed"] == 2
    cols = {c for c, _ in RIDGES[TALL]}
    assert {T - HALO, T - 1, T, T + HALO - 1, T + HALO, 2 * T - 1, 2 * T} <= cols
    for shape in (TALL, WIDE):
        path = ref.corridor_scene(*shape)[2]
        assert len(path) >= 200 and want(shape, "corridor", 1)[2]["levels_claimed"] == 2
        assert want(shape, "trap_50_45", 1)[0][14, 80] == 2 and want(shape, "trap_45_50", 1)[0][14, 80] == 1
    assert want(TALL, "blobs", 1)[2]["levels_claimed"] > 100 > want(TALL, "blobs", 16)[2]["levels_claimed"] > 1


@pytest.mark.parametrize("shape", [TALL, WIDE], ids=["130x150", "70x200"])
@pytest.mark.parametrize("name", ["ridges", "ridges^T"])
def test_bridged_pairs_are_cut_on_their_ridges(lab, shape, name):
    shape = shape[::-1] if name.endswith("^T") else shape
    for q in (1, 4, 16, 64):
        check(lab, shape, name, q)


@pytest.mark.parametrize("shape", [TALL, WIDE, TALL[::-1], WIDE[::-1]], ids=["130x150", "70x200", "150x130", "200x70"])
def test_a_long_corridor_at_one_level(lab, shape):
    name = "corridor^T" if shape[0] > shape[1] else "corridor"
    path = ref.corridor_scene(*sorted(shape))[2]
    for q in (1, 16):
        launches = check(lab, shape, name, q)
        assert launches >= (3 * len(path) // 4) // HALO          # 8 steps a launch at the most: the corridor alone needs as many


@pytest.mark.parametrize("shape", [TALL, WIDE], ids=["130x150", "70x200"])
def test_two_relief_values_skipping_jumps(lab, shape):
    for name in ("two_values", "two_values^T"):
        s = shape[::-1] if name.endswith("^T") else shape
        launches = check(lab, s, name, 1)
        assert launches < 200                                 # a visit to every level 0 .. 200 would take a launch each at the least
        check(lab, s, name, 2)


@pytest.mark.parametrize("name", ["trap_50_45", "trap_45_50"])
def test_no_jump_past_a_level_that_opens_late(lab, name):
    """the gate beside the seam is reachable only when level 40 has finished across it; the other gate waits from the start"""
    for shape in (TALL, WIDE):
        for q in (1, 2, 4):
            check(lab, shape, name, q)
        check(lab, shape[::-1], name + "^T", 1)


def test_one_level_is_the_split_on_the_splits_inputs(lab):
    for shape, name, D, C in (((150, 203), "mixture2", 2, 1), ((150, 203), "blobs", 2, 5), ((2 * T + HALO - 3, 3 * T + 5), "mixture3", 3, 5),
                              ((150, 203), "salt", 1, 1)):
        if name.startswith("mixture"):
            planes, cls, min_area = label_ref.planes_of(label_split_ref.mixture(*shape, int(name[7:])), 3, 2, seed=11), 2, 1
        else:
            planes, cls, min_area = label_ref.case(*shape, name)
        labels, table, counts = label_split_ref.split(planes, cls, min_area, D, C)
        assert counts["unreached"] == 0
        cut = lab.run(planes, cls, min_area, split=D, split_core=C)
        assert lab.split_counts() == counts and lab.flood_counts() is None
        for P, invert in ((1, False), (cls, True)):
            got = lab.run(planes, cls, min_area, split=D, split_core=C, flood=P, flood_step=256, flood_invert=invert)
            assert got[0].tobytes() == cut[0].tobytes() == labels.tobytes() and got[1].tobytes() == cut[1].tobytes() == table.tobytes()
            c = lab.flood_counts()
            assert lab.split_counts() == counts and c["levels_claimed"] == 1 and c["claimed"] == int((labels > 0).sum()) - int(
                (label_split_ref.seeds_of(label_ref.label(planes, cls, min_area)[0], D, C)[0] > 0).sum())


def test_inverted_class_plane(lab):
    for q in (1, 16):
        check(lab, TALL, "inverted", q)
    assert want(TALL, "inverted", 16)[0].tobytes() == want(TALL, "blobs", 16)[0].tobytes()    # the same relief, read from another plane


@pytest.mark.parametrize("q", [1, 16, 256])
def test_random_blobs_with_random_relief(lab, q):
    check(lab, TALL, "blobs", q)
    check(lab, WIDE[::-1], "blobs^T", q)


def test_with_a_rim_growth_after_the_flood(lab):
    inner, grown = want(TALL, "ridges", 16), want(TALL, "rim3", 16)
    assert grown[2] == inner[2] and (grown[0] > 0).sum() > (inner[0] > 0).sum()
    for name in ("rim1", "rim3", "rim%d" % (HALO + 1)):
        check(lab, TALL, name, 16)
    check(lab, WIDE, "rim3", 1)


@pytest.mark.parametrize("shape", [(1, 1), (1, 130), (130, 1), (2, 2), LITTLE, (T, T), (T + 1, T + 1)])
def test_small_shapes(lab, shape):
    for name in ("full", "empty") + (("ridges", "corridor") if shape == LITTLE else ("blobs",)):
        for q in (1, 256):
            check(lab, shape, name, q)


def test_without_a_label_plane(lab):
    planes = scene(TALL, "ridges")[0]
    got_labels, got_table = lab.run(planes, 2, 1, want_labels=False, **kwargs_of(TALL, "ridges", 4))
    assert got_labels is None
    same(None, got_table, lab, want(TALL, "ridges", 4), "no plane")


def test_run_flood_dev_on_torch_tensors_equals_the_host_entry(lab):
    import torch
    umx.require_torch_runtime("test_gpu_label_flood")
    for shape, name, q in ((TALL, "ridges", 4), (WIDE, "corridor", 1), (TALL, "rim3", 16)):
        planes = scene(shape, name)[0]
        wanted = want(shape, name, q)
        K, H, W = planes.shape
        kw = kwargs_of(shape, name, q)
        d_planes = torch.from_numpy(np.array(planes)).cuda()
        d_labels = torch.full((H, W), -7, dtype=torch.int32, device="cuda")     # a sentinel: every word must be written
        torch.cuda.synchronize()
        tables = []
        for _ in range(2):                                                      # twice: the same bytes
            d_labels.fill_(-7)
            torch.cuda.synchronize()
            tables.append(lab.run_ptr(d_planes.data_ptr(), K, H, W, d_labels.data_ptr(), 2, 1, **kw))
            same(d_labels.cpu().numpy(), tables[-1], lab, wanted, (name, "dev"))
        assert tables[0].tobytes() == tables[1].tobytes()
        host_labels, host_table = lab.run(planes, 2, 1, **kw)
        assert host_labels.tobytes() == d_labels.cpu().numpy().tobytes() and host_table.tobytes() == tables[0].tobytes()
        none = lab.run_ptr(d_planes.data_ptr(), K, H, W, 0, 2, 1, **kw)
        same(None, none, lab, wanted, (name, "dev, no plane"))
        assert np.array_equal(d_planes.cpu().numpy(), planes)                   # the planes are only read


def test_plain_and_split_runs_after_flood_runs_on_one_labeler():
    """the planes hold the leftovers of a flood when the older entries start: their bytes are a fresh labeler's"""
    with umx.Labeler() as lb, umx.Labeler() as fresh:
        planes = scene(TALL, "blobs")[0]
        check(lb, TALL, "blobs", 16)
        for kw in (dict(), dict(split=2, split_core=5), dict(split=2, split_regrow=3)):
            a, b = lb.run(planes, 2, 1, **kw), fresh.run(planes, 2, 1, **kw)
            assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
            assert lb.flood_counts() is None and lb.split_counts() == fresh.split_counts()
            check(lb, LITTLE, "ridges", 1)                    # (a smaller shape in between)
        wanted = label_split_ref.split(planes, 2, 1, 2, 5)
        got = lb.run(planes, 2, 1, split=2, split_core=5)
        assert np.array_equal(got[0], wanted[0]) and got[1].tobytes() == wanted[1].tobytes()


def test_measure_and_shape_take_the_flooded_labels(lab):
    planes = scene(TALL, "blobs")[0]
    labels, table, counts = want(TALL, "blobs", 16)
    N = counts["n_objects"]
    px = label_measure_ref.pixels(TALL, np.uint16, 2, seed=5)
    got_labels, got_table = lab.run(planes, 2, 1, **kwargs_of(TALL, "blobs", 16))
    rec = lab.measure(px)
    wanted = label_measure_ref.measure(labels, px, N)
    assert rec.shape == wanted.shape == (2, N) and rec.tobytes() == wanted.tobytes() and np.array_equal(rec["count"][0], got_table["area"])
    shapes = lab.shape()
    assert shapes.tobytes() == label_shape_ref.records(labels, N).tobytes()
    assert not np.array_equal(labels, label_split_ref.split(planes, 2, 1, 2, 5)[0])       # they are not the split's labels
    lab.run(planes, 2, 1, want_labels=False, **kwargs_of(TALL, "blobs", 16))
    with pytest.raises(umx.UmxError) as e:
        lab.measure(px)
    assert e.value.code == umx.ERR_INVALID and "no label plane" in str(e.value)


def test_a_refused_flood_touches_nothing_and_keeps_the_resident_labels(lab):
    planes = scene(TALL, "ridges")[0]
    labels, table, counts = want(TALL, "ridges", 4)
    px = label_measure_ref.pixels(TALL, np.uint8, 1, seed=6)
    good = kwargs_of(TALL, "ridges", 4)
    lab.run(planes, 2, 1, **good)
    before, shapes = lab.measure(px), lab.shape()
    out = np.full(TALL, -7, np.int32)
    for kw, word in ((dict(flood=3), "relief_plane"), (dict(flood=-1), "relief_plane"), (dict(flood_step=3), "level_step"),
                     (dict(flood_step=0), "level_step"), (dict(flood_step=512), "level_step"), (dict(flood_invert=2), "invert"),
                     (dict(split_regrow=8), "regrow"), (dict(split=0), "depth"), (dict(split=9), "depth"), (dict(split_core=0), "core_min_area"),
                     (dict(min_area=0), "min_area"), (dict(grow=256, grow_classes=(1,)), "grow_radius")):
        kw = dict(dict(good, min_area=1), **kw)
        with pytest.raises(umx.UmxError) as e:
            lab.run(planes, 2, **kw)
        assert e.value.code == umx.ERR_INVALID and word in str(e.value), kw
        o = umx._label_flood_options(umx._label_split_options(umx._label_options(3, 2, kw["min_area"], kw["grow"], kw["grow_classes"]), kw["split"],
                                                              kw["split_core"], kw.get("split_regrow", 255)), kw["flood"], kw["flood_step"],
                                     kw["flood_invert"])
        rc = lab._L.umx_labeler_run_flood(lab._lb, planes.ctypes.data, 3, TALL[0], TALL[1], ctypes.byref(o), out.ctypes.data, None)
        assert rc == umx.ERR_INVALID and (out == -7).all()    # the caller's plane is not written
        assert lab.measure(px).tobytes() == before.tobytes() and lab.shape().tobytes() == shapes.tobytes()
    assert lab._L.umx_labeler_run_flood(lab._lb, planes.ctypes.data, 3, TALL[0], TALL[1], None, out.ctypes.data, None) == umx.ERR_INVALID
    assert (out == -7).all() and lab.measure(px).tobytes() == before.tobytes()
    assert before.tobytes() == label_measure_ref.measure(labels, px, counts["n_objects"]).tobytes()
    check(lab, TALL, "ridges", 4)


_GUARD_CHILD = """
import sys
sys.path.insert(0, %r); sys.path.insert(0, %r)
import numpy as np
import label_flood_ref as ref
import test_gpu_label_flood as t
from unmicst_amd import umx
with umx.Labeler() as lb:
    for shape, names in (((1, 1), ("full",)), ((1, 130), ("full",)), ((130, 1), ("full",)), (t.LITTLE, ("ridges", "corridor")),
                         (t.WIDE, ("ridges", "corridor", "trap_50_45")), (t.TALL, ("ridges", "blobs", "rim3", "inverted")),
                         (t.TALL[::-1], ("ridges^T",))):   # (no shape smaller than one before it)
        for name in names:
            for q in (1, 16):
                t.check(lb, shape, name, q)                # (raises UmxError 7 when a red zone was written)
print("guard-ok")
"""


def test_guard_mode_finds_no_write_outside_the_buffers():
    """UMX_DEBUG_GUARD=0xa5 in a child process (the variable is read at umx_labeler_create): red zones round the three planes, the
    flags and the flood's two words, the planes exactly H * W words at a shape's first run, checked at the end of every run"""
    env = dict(os.environ, UMX_DEBUG_GUARD="0xa5")
    r = subprocess.run([sys.executable, "-c", _GUARD_CHILD % (ROOT, os.path.join(ROOT, "tests"))], env=env, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0 and "guard-ok" in r.stdout, r.stderr[-2000:]


def test_command_floods_the_label_mask(tmp_path, lab):
    """UnMicst.py --stackOutput --labelMask --labelSplit 2 --labelSplitCore 5 --labelFlood 1 --labelFloodStep 4 --labelMeasure
    --labelShape on the 150 x 171 crop of sample 105: the label page and the tables are the restatement applied to the probability pages
    the same run wrote, the contour plane as the relief.  Without --labelFlood the files are those of the split of before."""
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
    outs = {}
    for sub, flags in (("flood", ["--labelFlood", "1", "--labelFloodStep", "4"]), ("split", [])):
        out = outs[sub] = str(tmp_path / sub)
        r = subprocess.run([sys.executable, os.path.join(ROOT, "UnMicst.py"), img, "--model", "nucleiDAPI", "--stackOutput", "--outputPath", out,
                            "--labelMask", "--labelMinArea", "4", "--labelSplit", "2", "--labelSplitCore", "5", "--labelMeasure", "--labelShape"]
                           + flags, env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        pages = tiffio.imread_all(os.path.join(out, "crop_Probabilities_1.tif"))
        assert pages.shape == (3, 150, 171) and pages.dtype == np.uint8
        planes = np.ascontiguousarray(pages[::-1])                # the pages are in reversed class order
        if sub == "flood":
            labels, table, counts = ref.split_flood(planes, 2, 4, 2, 5, 1, 4)
            cut = label_split_ref.split(planes, 2, 4, 2, 5)
            assert counts["n_objects"] > counts["n_before"] > 1 and counts["levels_claimed"] > 1 and not np.array_equal(labels, cut[0])
            line = [l for l in r.stdout.splitlines() if l.startswith("Label flood: ")]
            assert len(line) == 1 and line[0].startswith("Label flood: %d pixels claimed at %d levels in " % (counts["claimed"], counts["levels_claimed"]))
            assert line[0].endswith(" launches, %d pixels unreached" % counts["unreached"])
        else:
            labels, table, counts = label_split_ref.split(planes, 2, 4, 2, 5)
            assert "Label flood" not in r.stdout
            got_labels, got_table = lab.run(planes, 2, 4, split=2, split_core=5)      # the entry of before, on the same planes
            assert np.array_equal(got_labels, labels) and got_table.tobytes() == table.tobytes()
        assert "Label split: %d objects from %d (%d with a core), %d pixels unreached" % tuple(counts[k] for k in label_split_ref.COUNTS) in r.stdout
        got = tiffio.imread_all(os.path.join(out, "crop_Labels_1.tif"))
        assert got.dtype == np.int32 and got.shape == (1, 150, 171) and np.array_equal(got[0], labels), sub
        lines = open(os.path.join(out, "crop_Objects_1.csv")).read().splitlines()
        cy, cx = label_ref.centroids(table)
        assert lines[0] == "label,area,y0,x0,y1,x1,centroid_y,centroid_x"
        assert lines[1:] == ["%d,%d,%d,%d,%d,%d,%.6f,%.6f" % (j + 1, t["area"], t["y0"], t["x0"], t["y1"], t["x1"], cy[j], cx[j])
                             for j, t in enumerate(table)], sub
        N = len(table)
        measured = [("pm%d" % k, label_measure_ref.measure(labels, planes[k], N)[0]) for k in range(3)]
        measured.append(("ch0", label_measure_ref.measure(labels, raw, N)[0]))
        assert open(os.path.join(out, "crop_Intensities_1.csv")).read().splitlines() == label_measure_ref.csv_lines(list(table["area"]), measured), sub
        assert len(open(os.path.join(out, "crop_Shapes_1.csv")).read().splitlines()) == N + 1
    # the flood changes nothing but the label files
    assert open(os.path.join(outs["flood"], "crop_Probabilities_1.tif"), "rb").read() == open(os.path.join(outs["split"], "crop_Probabilities_1.tif"), "rb").read()
