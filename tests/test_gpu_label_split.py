"""GPU tests of the label mask's split at the necks (unmicst_amd/csrc/umx_label.hip; include/umx.h and DESIGN.md section 8.1, steps 10 to
15): the labels, every field of the table and the four counts of umx_labeler_run_split / _run_split_dev against tests/label_split_ref.py,
compared for equality.  Everything is an integer: there is no tolerance anywhere in this file."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import helpers
import label_grow_ref
import label_measure_ref
import label_ref
import label_split_ref as ref
from unmicst_amd import model, tiffio, umx

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

T, HALO = umx.LABEL_GROW_TILE, umx.LABEL_GROW_HALO
MAIN = (150, 203)                              # 3 x 4 tiles with ragged last ones, five strips of 32 rows, 15 scan blocks of 2048 pixels
RAGGED = (2 * T + HALO - 3, 3 * T + 5)         # the last tiles HALO - 3 rows and 5 columns: inside a neighbour's halo
SMALL = [(1, 1), (1, 130), (130, 1), (2, 2), (17, 17), (64, 64), (65, 65)]
NAMES = ("blobs", "blobs_min40", "cls0", "k16_cls7", "salt", "serpentine", "comb", "checker", "full", "empty")
DEPTHS, CORES = (1, 2, 3, 8), (1, 5)


@functools.lru_cache(maxsize=None)
def case_of(shape, name):
    """(planes, cls, min_area): label_ref's cases by name; "mixture<D>", "bridges<D>" and "pairs" are this file's own"""
    H, W = shape
    if name.startswith("mixture"):
        planes, cls, min_area = label_ref.planes_of(ref.mixture(H, W, int(name[7:])), 3, 2, seed=11), 2, 1
    elif name.startswith("bridges"):
        D = int(name[7:])
        # across the tile corner (64, 64), the strip seam at row 32, the end of a 64-pixel chunk of a row, and the seam at row 96
        mask = ref.bridges_at(H, W, D, [(T, T), (umx.LABEL_STRIP_ROWS, 100), (100, 2 * T), (3 * umx.LABEL_STRIP_ROWS, 40), (130, 150)])
        planes, cls, min_area = label_ref.planes_of(mask, 3, 2, seed=12), 2, 1
    elif name == "pairs":
        planes, cls, min_area = label_grow_ref.planes_of_pred(ref.rimmed_pairs(H, W), 3, seed=13), 2, 1
    else:
        planes, cls, min_area = label_ref.case(H, W, name)
    planes.setflags(write=False)
    return planes, cls, min_area


@functools.lru_cache(maxsize=None)
def want(shape, name, D, C=1, L=255, R=0):
    """(labels, table, counts): the restatement, computed once per case and never changed"""
    planes, cls, min_area = case_of(shape, name)
    labels, table, counts = ref.split(planes, cls, min_area, D, C, L, R, (1,) if R else None)
    labels.setflags(write=False)
    table.setflags(write=False)
    return labels, table, counts


@pytest.fixture(scope="module")
def lab():
    with umx.Labeler() as lb:
        yield lb


def same(got_labels, got_table, got_counts, wanted, what):
    labels, table, counts = wanted
    if got_labels is not None:
        assert got_labels.dtype == np.int32 and got_labels.shape == labels.shape
        assert np.array_equal(got_labels, labels), (what, int((got_labels != labels).sum()))
    assert len(got_table) == len(table), (what, len(got_table), len(table))
    for f in label_ref.FIELDS:
        assert np.array_equal(got_table[f], table[f]), (what, f)
    assert got_counts == counts, (what, got_counts, counts)


def check(lab, shape, name, D, C=1, L=255, R=0):
    planes, cls, min_area = case_of(shape, name)
    got_labels, got_table = lab.run(planes, cls, min_area, grow=R, grow_classes=(1,) if R else None, split=D, split_core=C, split_regrow=L)
    same(got_labels, got_table, lab.split_counts(), want(shape, name, D, C, L, R), (shape, name, D, C, L, R))


def test_the_inputs_are_what_they_are_for():
    """asserted on the restatement alone: the inputs hold objects that split, objects that stay whole for want of a core and cored single
    ones; the figures of the CPU prototype; the thin inputs are wholly uncored"""
    H, W = RAGGED
    assert H > 2 * T and W > 2 * T and 0 < H - 2 * T <= HALO and 0 < W - 3 * T <= HALO
    labels, table, c = want(MAIN, "blobs", 2, 5)
    assert (c["n_before"], c["n_objects"], c["n_cored"], c["unreached"]) == (111, 141, 52, 0) and want(MAIN, "blobs", 2, 1)[2]["n_objects"] == 218
    for shape, name, D, C in ((MAIN, "blobs", 2, 5), (MAIN, "mixture2", 2, 1), (RAGGED, "mixture3", 3, 5), (MAIN, "bridges2", 2, 1)):
        planes, cls, min_area = case_of(shape, name)
        labels0 = label_ref.label(planes, cls, min_area)[0]
        labels, table, c = want(shape, name, D, C)
        assert c["n_objects"] > c["n_before"] > c["n_cored"] > 0 or name.startswith("bridges"), (name, c)
        per_object = [len(np.unique(labels[labels0 == o])) for o in range(1, c["n_before"] + 1)]
        assert max(per_object) >= 2, name                                                   # one splits
        if not name.startswith("bridges"):
            seeds = ref.seeds_of(labels0, D, C)[0]
            whole = [o for o in range(1, c["n_before"] + 1) if (seeds[labels0 == o] > 0).all()]
            assert len(whole) == c["n_before"] - c["n_cored"] > 0, name                        # one stays whole for want of a core
            assert sum(1 for o, k in enumerate(per_object, 1) if k == 1 and o not in whole) > 0, name   # one is cored but single
    for D in (1, 2, 3):
        c = want(MAIN, "bridges%d" % D, D)[2]
        assert c["n_before"] >= 4 and c["n_objects"] == 2 * c["n_before"] == 2 * c["n_cored"], (D, c)   # every dumbbell fits and is cut
    for name in ("checker", "comb", "serpentine"):
        for D in DEPTHS:
            c = want(MAIN, name, D)[2]
            assert c["n_objects"] == c["n_before"] > 0 and c["n_cored"] == 0 and c["unreached"] == 0


@pytest.mark.parametrize("name", NAMES)
def test_main_shape(lab, name):
    for D in DEPTHS:
        for C in CORES:
            check(lab, MAIN, name, D, C)


@pytest.mark.parametrize("D", [1, 2, 3])
def test_bridges_across_the_kernels_boundaries(lab, D):
    check(lab, MAIN, "bridges%d" % D, D)
    check(lab, MAIN, "mixture%d" % D, D)
    check(lab, MAIN, "mixture%d" % D, D, 5)


@pytest.mark.parametrize("name", ["mixture2", "mixture3", "blobs", "salt", "full"])
def test_ragged_shape_from_the_kernels_constants(lab, name):
    for D in DEPTHS:
        for C in CORES:
            check(lab, RAGGED, name, D, C)
    check(lab, RAGGED[::-1], name, 2, 1)


@pytest.mark.parametrize("shape", SMALL)
def test_small_shapes(lab, shape):
    for name in ("full", "blobs", "salt", "checker", "empty"):
        for D in (1, 2, 8) if shape != (17, 17) else (8,):
            check(lab, shape, name, D)
    if shape == (17, 17):
        assert want(shape, "full", 8)[2] == dict(n_objects=1, n_before=1, n_cored=1, unreached=0)    # the one-pixel core of 2 D + 1
    if shape == (65, 65):
        assert want(shape, "full", 8)[2]["n_cored"] == 1


def test_short_regrow_leaves_pixels_unreached(lab):
    assert want(MAIN, "blobs", 3, 1, 2)[2]["unreached"] > 0
    check(lab, MAIN, "blobs", 3, 1, 2)
    for L in (1, 3, HALO - 1):
        check(lab, MAIN, "full", 8, 1, L)                     # one core, `L` levels of one launch
    for L in (HALO, HALO + 1, 2 * HALO + 1):
        check(lab, RAGGED, "full", 8, 1, L)                   # one, two and three launches, all of which claim pixels
    assert want(RAGGED, "full", 8, 1, 2 * HALO)[2]["unreached"] == 0 < want(RAGGED, "full", 8, 1, 2 * HALO - 1)[2]["unreached"]


def test_early_stop_gives_the_bytes_of_all_levels(lab):
    """the necks of bridges2 are full after 4 levels: the second launch of L = 9 and of L = 255 claims nothing and the launches stop"""
    assert want(MAIN, "bridges2", 2, 1, HALO)[2]["unreached"] == 0 < want(MAIN, "bridges2", 2, 1, 3)[2]["unreached"]
    planes, cls, min_area = case_of(MAIN, "bridges2")
    runs = []
    for L in (HALO, HALO + 1, 255):
        check(lab, MAIN, "bridges2", 2, 1, L)
        runs.append(lab.run(planes, cls, min_area, split=2, split_regrow=L))
    assert all(r[0].tobytes() == runs[0][0].tobytes() and r[1].tobytes() == runs[0][1].tobytes() for r in runs)
    # an object whose regrow needs more than one launch, with a bound that ends in the middle of the second
    for L in (HALO, HALO + 3, 255):
        check(lab, MAIN, "full", 8, 1, L)


def test_with_a_rim_growth(lab):
    c = want(MAIN, "pairs", 2, 5, 255, 3)[2]
    inner = want(MAIN, "pairs", 2, 5)
    assert c == inner[2] and c["n_objects"] > c["n_before"] > 4 and (want(MAIN, "pairs", 2, 5, 255, 3)[0] > 0).sum() > (inner[0] > 0).sum()
    for R in (1, 3, HALO + 1):
        check(lab, MAIN, "pairs", 2, 5, 255, R)
    check(lab, RAGGED, "pairs", 2, 1, 255, 3)


def test_without_a_label_plane(lab):
    for name, D, C in (("blobs", 2, 5), ("mixture2", 2, 1), ("empty", 2, 1)):
        planes, cls, min_area = case_of(MAIN, name)
        got_labels, got_table = lab.run(planes, cls, min_area, want_labels=False, split=D, split_core=C)
        assert got_labels is None
        same(None, got_table, lab.split_counts(), want(MAIN, name, D, C), (name, D, C))


def test_run_split_dev_on_torch_tensors_equals_the_host_entry(lab):
    import torch
    umx.require_torch_runtime("test_gpu_label_split")
    for shape, name, D, C, R in ((RAGGED, "mixture2", 2, 1, 0), (MAIN, "blobs", 3, 5, 0), (MAIN, "pairs", 2, 5, 3)):
        planes, cls, min_area = case_of(shape, name)
        wanted = want(shape, name, D, C, 255, R)
        K, H, W = planes.shape
        kw = dict(grow=R, grow_classes=(1,) if R else None, split=D, split_core=C)
        d_planes = torch.from_numpy(np.array(planes)).cuda()
        d_labels = torch.full((H, W), -7, dtype=torch.int32, device="cuda")     # a sentinel: every word must be written
        torch.cuda.synchronize()
        got_table = lab.run_ptr(d_planes.data_ptr(), K, H, W, d_labels.data_ptr(), cls, min_area, **kw)
        same(d_labels.cpu().numpy(), got_table, lab.split_counts(), wanted, (name, "dev"))
        host_labels, host_table = lab.run(planes, cls, min_area, **kw)
        assert host_labels.tobytes() == d_labels.cpu().numpy().tobytes() and host_table.tobytes() == got_table.tobytes()
        none = lab.run_ptr(d_planes.data_ptr(), K, H, W, 0, cls, min_area, **kw)
        same(None, none, lab.split_counts(), wanted, (name, "dev, no plane"))
        assert np.array_equal(d_planes.cpu().numpy(), planes)                   # the planes are only read


def test_two_runs_give_the_same_bytes(lab):
    planes, cls, min_area = case_of(MAIN, "mixture2")
    a = lab.run(planes, cls, min_area, split=2, split_core=5) + (lab.split_counts(),)
    b = lab.run(planes, cls, min_area, split=2, split_core=5) + (lab.split_counts(),)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and a[2] == b[2]


def test_plain_runs_after_split_runs_on_one_labeler():
    """every plane holds the leftovers of a split when the plain run starts; a smaller shape after a larger one; split=0 through the
    binding is the plain entry: the bytes of a fresh labeler"""
    with umx.Labeler() as lb, umx.Labeler() as fresh:
        for shape, name, D in ((MAIN, "mixture2", 2), (MAIN, "mixture2", 0), (RAGGED, "blobs", 8), (RAGGED, "blobs", 0), ((17, 17), "full", 8),
                               ((17, 17), "full", 0), (MAIN, "salt", 1), (MAIN, "pairs", 0)):
            planes, cls, min_area = case_of(shape, name)
            if D:
                got_labels, got_table = lb.run(planes, cls, min_area, split=D)
                same(got_labels, got_table, lb.split_counts(), want(shape, name, D), (shape, name, D))
            else:
                R = 3 if name == "pairs" else 0
                got_labels, got_table = lb.run(planes, cls, min_area, grow=R, split=0)
                assert lb.split_counts() is None
                labels, table = label_grow_ref.label_grow(planes, cls, min_area, R)
                assert np.array_equal(got_labels, labels) and got_table.tobytes() == table.tobytes()
                f_labels, f_table = fresh.run(planes, cls, min_area, grow=R)
                assert f_labels.tobytes() == got_labels.tobytes() and f_table.tobytes() == got_table.tobytes()


def test_measure_measures_the_split_labels(lab):
    planes, cls, min_area = case_of(MAIN, "mixture2")
    labels, table, counts = want(MAIN, "mixture2", 2, 5)
    px = label_measure_ref.pixels(MAIN, np.uint16, 2, seed=5)
    got_labels, got_table = lab.run(planes, cls, min_area, split=2, split_core=5)
    rec = lab.measure(px)
    wanted = label_measure_ref.measure(labels, px, counts["n_objects"])
    assert rec.shape == wanted.shape == (2, counts["n_objects"]) and rec.tobytes() == wanted.tobytes()
    assert np.array_equal(rec["count"][0], got_table["area"]) and counts["n_objects"] > counts["n_before"]
    # a split run without a label plane leaves nothing to measure, as a plain one
    lab.run(planes, cls, min_area, want_labels=False, split=2)
    with pytest.raises(umx.UmxError) as e:
        lab.measure(px)
    assert e.value.code == umx.ERR_INVALID and "no label plane" in str(e.value)


def test_a_refused_split_leaves_the_labeler_usable_and_its_labels_resident(lab):
    planes, cls, min_area = case_of(MAIN, "mixture2")
    labels, table, counts = want(MAIN, "mixture2", 2)
    px = label_measure_ref.pixels(MAIN, np.uint8, 1, seed=6)
    lab.run(planes, cls, min_area, split=2)
    before = lab.measure(px)
    for kw, word in ((dict(split=9), "depth"), (dict(split=-1), "depth"), (dict(split=2, split_core=0), "core_min_area"),
                     (dict(split=2, split_core=65537), "core_min_area"), (dict(split=2, split_regrow=0), "regrow"),
                     (dict(split=2, split_regrow=256), "regrow"), (dict(split=2, grow=256, grow_classes=(1,)), "grow_radius"),
                     (dict(split=2, min_area=0), "min_area")):
        kw = dict(dict(min_area=min_area), **kw)
        with pytest.raises(umx.UmxError) as e:
            lab.run(planes, cls, **kw)
        assert e.value.code == umx.ERR_INVALID and word in str(e.value)
        after = lab.measure(px)                               # the labels of the last good run are still there
        assert after.tobytes() == before.tobytes()
    assert before.tobytes() == label_measure_ref.measure(labels, px, counts["n_objects"]).tobytes()
    check(lab, MAIN, "mixture2", 2)


_GUARD_CHILD = """
import sys
sys.path.insert(0, %r); sys.path.insert(0, %r)
import numpy as np
import label_ref
import label_grow_ref
import label_split_ref as ref
from unmicst_amd import umx
T, HALO = umx.LABEL_GROW_TILE, umx.LABEL_GROW_HALO
with umx.Labeler() as lb:
    for shape in ((1, 1), (1, 130), (130, 1), (17, 17), (65, 65), (2 * T + HALO - 3, 3 * T + 5), (3 * T + 5, 2 * T + HALO - 3)):   # (no shape smaller than one before it)
        for name in ("mixture", "full", "salt"):
            mask = ref.mixture(shape[0], shape[1], 2) if name == "mixture" else label_ref._CASES[name][0](shape[0], shape[1])
            planes = label_ref.planes_of(mask, 3, 2, seed=3)
            for D, C, L, R in ((1, 1, 255, 0), (2, 5, 255, 0), (8, 1, 255, 0), (3, 1, 2, 0), (2, 1, HALO + 1, 3)):
                labels, table, counts = ref.split(planes, 2, 1, D, C, L, R)
                got_labels, got_table = lb.run(planes, 2, 1, grow=R, split=D, split_core=C, split_regrow=L)   # (raises UmxError 7 when a red zone was written)
                assert np.array_equal(got_labels, labels) and got_table.tobytes() == table.tobytes() and lb.split_counts() == counts, (shape, name, D, C, L, R)
print("guard-ok")
"""


def test_guard_mode_finds_no_write_outside_the_buffers():
    """UMX_DEBUG_GUARD=0xa5 in a child process (the variable is read at umx_labeler_create): red zones round the three planes and the
    flags, which are exactly H * W words (bytes, rounded up to a word) at a shape's first run, checked at the end of every run"""
    env = dict(os.environ, UMX_DEBUG_GUARD="0xa5")
    r = subprocess.run([sys.executable, "-c", _GUARD_CHILD % (ROOT, os.path.join(ROOT, "tests"))], env=env, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0 and "guard-ok" in r.stdout, r.stderr[-2000:]


def test_command_splits_the_label_mask(tmp_path, lab):
    """UnMicst.py --stackOutput --labelMask --labelSplit 2 --labelSplitCore 5 --labelMeasure on the 150 x 171 crop of sample 105: the label
    page and both tables are the restatement applied to the probability pages the same run wrote.  Without --labelSplit the files are
    those of the plain entry."""
    hp, blob, mean, std = helpers.load_nuclei_dapi()
    models = tmp_path / "models"
    model.save_converted(model.ModelArtefacts(hp, blob, mean, std), str(models / "nucleiDAPI"))
    raw = np.ascontiguousarray(helpers.load_sample_105()[0][300:450, 200:371])
    assert raw.dtype in (np.uint8, np.uint16)
    reg = tmp_path / "x" / "registration"
    os.makedirs(reg)
    img = str(reg / "crop.tif")
    tiffio.imsave(img, raw)
    env = {k: v for k, v in os.environ.items() if k != "UMX_HIP_RUNTIME"}
    env["UMX_MODELS_DIR"] = str(models)
    outs = {}
    for sub, flags in (("split", ["--labelSplit", "2", "--labelSplitCore", "5"]), ("plain", [])):
        out = outs[sub] = str(tmp_path / sub)
        r = subprocess.run([sys.executable, os.path.join(ROOT, "UnMicst.py"), img, "--model", "nucleiDAPI", "--stackOutput", "--outputPath", out,
                            "--labelMask", "--labelMinArea", "4", "--labelMeasure"] + flags, env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        pages = tiffio.imread_all(os.path.join(out, "crop_Probabilities_1.tif"))
        assert pages.shape == (3, 150, 171) and pages.dtype == np.uint8
        planes = np.ascontiguousarray(pages[::-1])                # the pages are in reversed class order
        if sub == "split":
            labels, table, counts = ref.split(planes, 2, 4, 2, 5)
            assert counts["n_objects"] > counts["n_before"] > 1   # the case is not empty: nuclei were split
            assert "Label split: %d objects from %d (%d with a core), %d pixels unreached" % tuple(counts[k] for k in ref.COUNTS) in r.stdout
        else:
            labels, table = label_ref.label(planes, 2, 4)
            assert "Label split" not in r.stdout
            got_labels, got_table = lab.run(planes, 2, 4)         # the entry of before, on the same planes
            assert np.array_equal(got_labels, labels) and got_table.tobytes() == table.tobytes()
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
    for n in ("crop_Probabilities_1.tif",):                      # the split changes nothing but the label files
        assert open(os.path.join(outs["split"], n), "rb").read() == open(os.path.join(outs["plain"], n), "rb").read()
