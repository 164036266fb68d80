"""GPU tests of the label mask's growth (unmicst_amd/csrc/umx_label.hip; include/umx.h and DESIGN.md section 8.1, steps 6 and 7): the
labels, the count and every field of the table of umx_labeler_run / _run_dev with grow_radius > 0 against tests/label_grow_ref.py,
compared for equality.  Everything is an integer: there is no tolerance anywhere in this file."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import helpers
import label_grow_ref as ref
import label_ref
from unmicst_amd import model, tiffio, umx

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

T, HALO = umx.LABEL_GROW_TILE, umx.LABEL_GROW_HALO
MAIN = (150, 203)                              # 3 x 4 tiles, the last ones 22 rows and 11 columns
SMALL = [(1, 1), (1, 130), (130, 1)]
RAGGED = (2 * T + HALO - 3, 3 * T + 5)         # more than two tiles each way; the last ones HALO - 3 rows and 5 columns: inside a neighbour's halo
RADII = (1, 2, HALO - 1, HALO, HALO + 1, 2 * HALO, 2 * HALO + 1)   # one launch, its last level, the first of the next, two launches, a third


@functools.lru_cache(maxsize=None)
def case_of(shape, name):
    planes, cls, min_area, classes = ref.case(shape[0], shape[1], name, T, HALO)
    planes.setflags(write=False)
    return planes, cls, min_area, classes


@functools.lru_cache(maxsize=None)
def want(shape, name, R):
    """(labels, table): the restatement, computed once per shape, case and radius and never changed"""
    planes, cls, min_area, classes = case_of(shape, name)
    labels, table = ref.label_grow(planes, cls, min_area, R, classes)
    labels.setflags(write=False)
    table.setflags(write=False)
    return labels, table


@pytest.fixture(scope="module")
def lab():
    with umx.Labeler() as lb:
        yield lb


def same(got_labels, got_table, labels, table, what):
    if got_labels is not None:
        assert got_labels.dtype == np.int32 and got_labels.shape == labels.shape
        assert np.array_equal(got_labels, labels), (what, int((got_labels != labels).sum()))
    assert len(got_table) == len(table), (what, len(got_table), len(table))
    for f in label_ref.FIELDS:
        assert np.array_equal(got_table[f], table[f]), (what, f)


def check(lab, shape, name, R):
    planes, cls, min_area, classes = case_of(shape, name)
    labels, table = want(shape, name, R)
    got_labels, got_table = lab.run(planes, cls, min_area, grow=R, grow_classes=classes)
    same(got_labels, got_table, labels, table, (shape, name, R))


def test_shapes_are_what_they_are_for():
    H, W = RAGGED
    assert H > 2 * T and W > 2 * T and 0 < H - 2 * T <= HALO and 0 < W - 3 * T <= HALO
    assert len(want(MAIN, "rings", 1)[1]) == 154 and len(want(RAGGED, "rings", 1)[1]) > 100
    a, b = want(RAGGED, "rings", HALO)[0], want(RAGGED, "rings", HALO + 1)[0]
    assert (a > 0).sum() < (b > 0).sum()                      # the second launch has work to do


@pytest.mark.parametrize("name", ref.NAMES)
def test_main_shape(lab, name):
    for R in RADII:
        check(lab, MAIN, name, R)


@pytest.mark.parametrize("name", ref.NAMES)
def test_ragged_shape_from_the_kernels_constants(lab, name):
    for R in RADII:
        check(lab, RAGGED, name, R)


@pytest.mark.parametrize("shape", SMALL)
def test_small_shapes(lab, shape):
    for name in ref.NAMES:
        for R in RADII:
            check(lab, shape, name, R)


@pytest.mark.parametrize("shape", [MAIN, RAGGED, (1, 130), (130, 1)])
def test_longest_radius_on_the_corridor(lab, shape):
    """32 launches; on the two larger shapes every one of them claims pixels: the path is longer than 255"""
    labels = want(shape, "corridor", umx.LABEL_MAX_GROW)[0]
    assert (labels > 0).sum() == 1 + min(umx.LABEL_MAX_GROW, len(ref.path(shape[0], shape[1], T)) - 1)
    check(lab, shape, "corridor", umx.LABEL_MAX_GROW)


def test_default_classes_are_all_but_the_background_and_the_label_class(lab):
    planes, cls, min_area, classes = case_of(MAIN, "rings")
    assert classes == (1,) and cls == planes.shape[0] - 1
    labels, table = want(MAIN, "rings", 3)
    got_labels, got_table = lab.run(planes, grow=3)
    same(got_labels, got_table, labels, table, "default classes")


def test_without_a_label_plane(lab):
    for name, R in (("rings", 3), ("rings", HALO + 1), ("corridor", 2 * HALO), ("empty", 2)):
        planes, cls, min_area, classes = case_of(MAIN, name)
        labels, table = want(MAIN, name, R)
        got_labels, got_table = lab.run(planes, cls, min_area, want_labels=False, grow=R, grow_classes=classes)
        assert got_labels is None
        same(None, got_table, labels, table, (name, R))


def test_run_dev_on_torch_tensors_equals_run(lab):
    import torch
    umx.require_torch_runtime("test_gpu_label_grow")
    for name, R in (("rings", 3), ("rings", HALO + 1), ("duel_odd", 2 * HALO), ("cls_in_G", 2 * HALO + 1)):   # 1, 2, 2 and 3 launches
        planes, cls, min_area, classes = case_of(RAGGED, name)
        labels, table = want(RAGGED, name, R)
        K, H, W = planes.shape
        d_planes = torch.from_numpy(np.array(planes)).cuda()
        d_labels = torch.full((H, W), -7, dtype=torch.int32, device="cuda")     # a sentinel: every word must be written
        torch.cuda.synchronize()
        got_table = lab.run_ptr(d_planes.data_ptr(), K, H, W, d_labels.data_ptr(), cls, min_area, grow=R, grow_classes=classes)
        same(d_labels.cpu().numpy(), got_table, labels, table, (name, R))
        host_labels, host_table = lab.run(planes, cls, min_area, grow=R, grow_classes=classes)
        assert host_labels.tobytes() == d_labels.cpu().numpy().tobytes() and host_table.tobytes() == got_table.tobytes()
        none = lab.run_ptr(d_planes.data_ptr(), K, H, W, 0, cls, min_area, grow=R, grow_classes=classes)
        same(None, none, labels, table, (name, R, "no plane"))
        assert np.array_equal(d_planes.cpu().numpy(), planes)                   # the planes are only read


def test_two_runs_give_the_same_bytes(lab):
    planes, cls, min_area, classes = case_of(MAIN, "rings")
    a = lab.run(planes, cls, min_area, grow=HALO + 1, grow_classes=classes)
    b = lab.run(planes, cls, min_area, grow=HALO + 1, grow_classes=classes)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()


def test_a_plain_run_after_a_growth_on_one_labeler():
    """both planes hold grown labels when the plain run starts; and a growth after a larger growth"""
    with umx.Labeler() as lb:
        for shape, name, R in ((MAIN, "rings", 2 * HALO + 1), (MAIN, "rings", 0), (RAGGED, "cls_in_G", HALO), (RAGGED, "cls_in_G", 0),
                               ((1, 130), "duel_even", HALO + 1), (MAIN, "far", 3), (MAIN, "rings", 1)):
            planes, cls, min_area, classes = case_of(shape, name)
            got_labels, got_table = lb.run(planes, cls, min_area, grow=R, grow_classes=classes if R else None)
            labels, table = want(shape, name, R) if R else label_ref.label(planes, cls, min_area)
            same(got_labels, got_table, labels, table, (shape, name, R))


def test_refused_growth_leaves_the_labeler_usable(lab):
    planes, cls, min_area, classes = case_of(MAIN, "rings")
    for kw, word in ((dict(grow=256, grow_classes=classes), "grow_radius"), (dict(grow=-1, grow_classes=classes), "grow_radius"),
                     (dict(grow=2, grow_classes=()), "grow_classes"), (dict(grow=2, grow_classes=(1, 3)), "grow_classes"),
                     (dict(grow=0, grow_classes=(1,)), "grow_classes")):
        with pytest.raises(umx.UmxError) as e:
            lab.run(planes, cls, min_area, **kw)
        assert e.value.code == umx.ERR_INVALID and word in str(e.value)
    check(lab, MAIN, "rings", 3)


_GUARD_CHILD = """
import sys
sys.path.insert(0, %r); sys.path.insert(0, %r)
import numpy as np
import label_grow_ref as ref
from unmicst_amd import umx
T, HALO = umx.LABEL_GROW_TILE, umx.LABEL_GROW_HALO
with umx.Labeler() as lb:
    for shape in ((1, 130), (130, 1), (2 * T + HALO - 3, 3 * T + 5), (3 * T + 5, 2 * T + HALO - 3)):   # (no shape smaller than one before it)
        for name in ("rings", "corridor", "duel_odd"):
            planes, cls, min_area, classes = ref.case(shape[0], shape[1], name, T, HALO)
            for R in (1, HALO, HALO + 1, 2 * HALO + 1):
                labels, table = ref.label_grow(planes, cls, min_area, R, classes)
                got_labels, got_table = lb.run(planes, cls, min_area, grow=R, grow_classes=classes)   # (raises UmxError 7 when a red zone was written)
                assert np.array_equal(got_labels, labels) and got_table.tobytes() == table.tobytes(), (shape, name, R)
print("guard-ok")
"""


def test_guard_mode_finds_no_write_outside_the_buffers():
    """UMX_DEBUG_GUARD=0xa5 in a child process (the variable is read at umx_labeler_create): red zones round both planes, which are
    exactly H * W words at a shape's first run, checked at the end of every run; the ragged shapes return UMX_OK and the right answer."""
    env = dict(os.environ, UMX_DEBUG_GUARD="0xa5")
    r = subprocess.run([sys.executable, "-c", _GUARD_CHILD % (ROOT, os.path.join(ROOT, "tests"))], env=env, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0 and "guard-ok" in r.stdout, r.stderr[-2000:]


def test_command_grows_the_label_mask(tmp_path):
    """UnMicst.py --stackOutput --labelMask --labelMinArea 4 --labelGrow 3 on the 150 x 171 crop of sample 105: the label page and the
    table are the restatement applied to the probability pages the same run wrote, on the raw fast path and on the host-side one."""
    hp, blob, mean, std = helpers.load_nuclei_dapi()
    models = tmp_path / "models"
    model.save_converted(model.ModelArtefacts(hp, blob, mean, std), str(models / "nucleiDAPI"))
    raw = helpers.load_sample_105()[0][300:450, 200:371]
    reg = tmp_path / "x" / "registration"
    os.makedirs(reg)
    img = str(reg / "crop.tif")
    tiffio.imsave(img, np.ascontiguousarray(raw))
    env = {k: v for k, v in os.environ.items() if k != "UMX_HIP_RUNTIME"}
    env["UMX_MODELS_DIR"] = str(models)
    for sub, extra in (("out_raw", {}), ("out_host", {"UMX_NO_RAW_PATH": "1"})):
        out = str(tmp_path / sub)
        r = subprocess.run([sys.executable, os.path.join(ROOT, "UnMicst.py"), img, "--model", "nucleiDAPI", "--stackOutput", "--outputPath", out,
                            "--labelMask", "--labelMinArea", "4", "--labelGrow", "3"], env=dict(env, **extra), capture_output=True, text=True,
                           timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        pages = tiffio.imread_all(os.path.join(out, "crop_Probabilities_1.tif"))
        assert pages.shape == (3, 150, 171) and pages.dtype == np.uint8
        planes = np.ascontiguousarray(pages[::-1])                # the pages are in reversed class order
        seeds, seed_table = label_ref.label(planes, 2, 4)
        labels, table = ref.label_grow(planes, 2, 4, 3, (1,))     # the default set of a three-class model: the contours
        assert len(table) == len(seed_table) > 1 and (table["area"] >= seed_table["area"]).all()
        assert table["area"].sum() > seed_table["area"].sum()     # the case is not empty: the nuclei did grow
        got = tiffio.imread_all(os.path.join(out, "crop_Labels_1.tif"))
        assert got.dtype == np.int32 and got.shape == (1, 150, 171) and np.array_equal(got[0], labels), sub
        lines = open(os.path.join(out, "crop_Objects_1.csv")).read().splitlines()
        cy, cx = label_ref.centroids(table)
        assert lines[0] == "label,area,y0,x0,y1,x1,centroid_y,centroid_x"
        assert lines[1:] == ["%d,%d,%d,%d,%d,%d,%.6f,%.6f" % (j + 1, t["area"], t["y0"], t["x0"], t["y1"], t["x1"], cy[j], cx[j])
                             for j, t in enumerate(table)], sub
