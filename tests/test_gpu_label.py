"""GPU tests of the label mask (unmicst_amd/csrc/umx_label.hip; include/umx.h and DESIGN.md section 8.1): the labels, the count and
every field of the table of umx_labeler_run / _run_dev against tests/label_ref.py (numpy + scipy.ndimage.label), compared for equality.
Everything is an integer: there is no tolerance anywhere in this file."""
import ctypes
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import helpers
import label_ref
from unmicst_amd import model, tiffio, umx

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

MAIN = (150, 203)      # rows cross three 64-lane chunks with a ragged last one; 4 strips of 32 rows + 22; 4 x 4 scan-block waves and more
SMALL = [(1, 1), (1, 130), (130, 1), (64, 64)]


def big_shape():
    """From the kernels' own constants: more than LABEL_THREADS columns (two rounds along a seam and in every strip), more than
    LABEL_THREADS scan blocks (two rounds of the one-workgroup scan), more than four strips (two seam levels and more)."""
    W = umx.LABEL_THREADS + 37
    H = max(4 * umx.LABEL_STRIP_ROWS + 3, (umx.LABEL_THREADS * umx.LABEL_SCAN_BLOCK) // W + 2)
    assert H <= 2048 and W <= 2048
    assert W > umx.LABEL_THREADS and -(-H * W // umx.LABEL_SCAN_BLOCK) > umx.LABEL_THREADS and H > 4 * umx.LABEL_STRIP_ROWS
    return H, W


@functools.lru_cache(maxsize=None)
def case_of(shape, name):
    """(planes, cls, min_area, labels, table): the restatement, computed once per shape and case and never changed"""
    planes, cls, min_area = label_ref.case(shape[0], shape[1], name)
    labels, table = label_ref.label(planes, cls, min_area)
    for a in (planes, labels, table):
        a.setflags(write=False)
    return planes, cls, min_area, labels, table


def cases_of(shape):
    return {name: case_of(shape, name) for name in label_ref.NAMES}


@pytest.fixture(scope="module")
def lab():
    with umx.Labeler() as lb:
        yield lb


def same(got_labels, got_table, labels, table, what):
    if got_labels is not None:
        assert got_labels.dtype == np.int32 and got_labels.shape == labels.shape
        assert np.array_equal(got_labels, labels), what
    assert len(got_table) == len(table), (what, len(got_table), len(table))
    for f in label_ref.FIELDS:
        assert np.array_equal(got_table[f], table[f]), (what, f)


def test_the_cases_have_the_properties_they_are_named_for():
    """asserted on the restatement, so that a change of the builders cannot empty a case"""
    c = cases_of(MAIN)
    n = {k: len(v[4]) for k, v in c.items()}
    assert n["empty"] == 0 and n["full"] == 1
    assert n["checker"] == 15225 and (c["checker"][4]["area"] == 1).all() and n["checker_min5"] == 0
    assert n["serpentine"] == 1 and c["serpentine"][4]["y1"][0] // umx.LABEL_STRIP_ROWS == (MAIN[0] - 1) // umx.LABEL_STRIP_ROWS   # one object, first strip to last
    assert n["comb"] == 1 and c["comb"][4]["area"][0] == 149 * 68 + 203             # teeth across every seam, joined at the bottom
    assert n["salt"] > 0 and n["salt_min5"] > 0 and n["salt"] != n["salt_min5"]
    assert n["blobs"] > n["blobs_min40"] > 0                                        # the filter drops some and keeps some
    assert c["cls0"][1] == 0 and n["cls0"] > 1 and c["k2"][0].shape[0] == 2 and n["k2"] > 1
    assert c["k16_cls7"][0].shape[0] == 16 and n["k16_cls7"] > 1
    H, W = big_shape()
    assert len(case_of((H, W), "serpentine")[4]) == 1 and len(case_of((H, W), "salt")[4]) > umx.LABEL_THREADS   # more objects than one round of any loop numbers


@pytest.mark.parametrize("name", label_ref.NAMES)
def test_main_shape(lab, name):
    planes, cls, min_area, labels, table = case_of(MAIN, name)
    got_labels, got_table = lab.run(planes, cls, min_area)
    same(got_labels, got_table, labels, table, name)


@pytest.mark.parametrize("shape", SMALL)
def test_small_shapes(lab, shape):
    for name, (planes, cls, min_area, labels, table) in cases_of(shape).items():
        got_labels, got_table = lab.run(planes, cls, min_area)
        same(got_labels, got_table, labels, table, (shape, name))


@pytest.mark.parametrize("name", ["serpentine", "comb", "salt", "salt_min5", "blobs", "checker"])
def test_shape_from_the_kernels_constants(lab, name):
    planes, cls, min_area, labels, table = case_of(big_shape(), name)
    got_labels, got_table = lab.run(planes, cls, min_area)
    same(got_labels, got_table, labels, table, name)


def test_default_class_is_the_last(lab):
    planes, cls, min_area, labels, table = case_of(MAIN, "blobs")
    assert cls == planes.shape[0] - 1
    got_labels, got_table = lab.run(planes)
    same(got_labels, got_table, labels, table, "default class")


def test_two_runs_give_the_same_bytes(lab):
    planes, cls, min_area, _, _ = case_of(MAIN, "salt_min5")
    a = lab.run(planes, cls, min_area)
    b = lab.run(planes, cls, min_area)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()


def test_a_smaller_run_after_a_larger_one():
    """the kept buffers hold the larger run's parents, areas, block counts and table"""
    with umx.Labeler() as lb:
        for shape, name in ((big_shape(), "salt"), (MAIN, "blobs"), ((1, 130), "salt"), (MAIN, "checker"), ((64, 64), "empty"), (MAIN, "comb")):
            planes, cls, min_area, labels, table = case_of(shape, name)
            got_labels, got_table = lb.run(planes, cls, min_area)
            same(got_labels, got_table, labels, table, (shape, name))


def test_without_a_label_plane(lab):
    for name in ("salt_min5", "blobs", "empty"):
        planes, cls, min_area, labels, table = case_of(MAIN, name)
        got_labels, got_table = lab.run(planes, cls, min_area, want_labels=False)
        assert got_labels is None
        same(None, got_table, labels, table, name)


def test_run_dev_on_torch_tensors_equals_run(lab):
    import torch
    umx.require_torch_runtime("test_gpu_label")
    for name in ("salt_min5", "serpentine", "k2"):
        planes, cls, min_area, labels, table = case_of(MAIN, name)
        K, H, W = planes.shape
        d_planes = torch.from_numpy(np.array(planes)).cuda()
        d_labels = torch.full((H, W), -7, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        got_table = lab.run_ptr(d_planes.data_ptr(), K, H, W, d_labels.data_ptr(), cls, min_area)
        same(d_labels.cpu().numpy(), got_table, labels, table, name)
        host_labels, host_table = lab.run(planes, cls, min_area)
        assert host_labels.tobytes() == d_labels.cpu().numpy().tobytes() and host_table.tobytes() == got_table.tobytes()
        same(None, lab.run_ptr(d_planes.data_ptr(), K, H, W, 0, cls, min_area), labels, table, name + ", no plane")


def test_refused_calls_leave_the_labeler_usable(lab):
    planes, cls, min_area, labels, table = case_of(MAIN, "blobs")
    for kw, word in ((dict(cls=3), "cls"), (dict(cls=-1), "cls"), (dict(min_area=0), "min_area"), (dict(min_area=65537), "min_area")):
        with pytest.raises(umx.UmxError) as e:
            lab.run(planes, **kw)
        assert e.value.code == umx.ERR_INVALID and word in str(e.value)
    with pytest.raises(umx.UmxError) as e:
        lab.run(np.zeros((17, 4, 4), np.uint8), 0)
    assert e.value.code == umx.ERR_INVALID and "classes" in str(e.value)
    o = umx._LabelOptions(2, 1)
    o.reserved[5] = 1
    n = ctypes.c_int64(-1)
    out = np.full(planes.shape[1:], -3, np.int32)
    rc = lab._L.umx_labeler_run(lab._lb, planes.ctypes.data, 3, MAIN[0], MAIN[1], ctypes.byref(o), out.ctypes.data, ctypes.byref(n))
    assert rc == umx.ERR_INVALID and b"reserved" in lab._L.umx_labeler_last_error(lab._lb) and n.value == -1 and (out == -3).all()
    assert lab._L.umx_labeler_run(lab._lb, None, 3, 4, 4, ctypes.byref(umx._LabelOptions(2, 1)), None, ctypes.byref(n)) == umx.ERR_INVALID
    got_labels, got_table = lab.run(planes, cls, min_area)
    same(got_labels, got_table, labels, table, "after the refusals")


_GUARD_CHILD = """
import sys
sys.path.insert(0, %r); sys.path.insert(0, %r)
import numpy as np
import label_ref
from unmicst_amd import umx
with umx.Labeler() as lb:
    for shape in ((150, 203), (1, 130), (130, 1), (203, 150)):
        for name in ("salt", "salt_min5", "comb", "checker"):
            planes, cls, min_area = label_ref.case(shape[0], shape[1], name)
            labels, table = label_ref.label(planes, cls, min_area)
            got_labels, got_table = lb.run(planes, cls, min_area)      # (raises UmxError 7 when a red zone was written)
            assert np.array_equal(got_labels, labels) and got_table.tobytes() == table.tobytes(), (shape, name)
print("guard-ok")
"""


def test_guard_mode_finds_no_write_outside_the_buffers():
    """UMX_DEBUG_GUARD=0xa5 in a child process (the variable is read at umx_labeler_create): red zones round every buffer of the
    labeler, checked at the end of every run; the ragged shapes return UMX_OK and the right answer."""
    env = dict(os.environ, UMX_DEBUG_GUARD="0xa5")
    r = subprocess.run([sys.executable, "-c", _GUARD_CHILD % (ROOT, os.path.join(ROOT, "tests"))], env=env, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0 and "guard-ok" in r.stdout, r.stderr[-2000:]


def test_command_writes_the_label_mask_and_changes_nothing_else(tmp_path):
    """UnMicst.py --stackOutput --labelMask --labelMinArea 4 on a synthetic uint16 TIFF of 2 x 2 tiles with a ragged edge: the label
    page and the table are the restatement of the probability pages the same run wrote; without the flag every file is the same bytes
    and neither label file exists."""
    hp, blob, mean, std = helpers.load_nuclei_dapi()
    models = tmp_path / "models"
    model.save_converted(model.ModelArtefacts(hp, blob, mean, std), str(models / "nucleiDAPI"))
    raw = helpers.load_sample_105()[0][300:450, 200:371]          # 150 x 171: two tiles of 128 (margin 16) either way, ragged
    reg = tmp_path / "x" / "registration"
    os.makedirs(reg)
    img = str(reg / "crop.tif")
    tiffio.imsave(img, np.ascontiguousarray(raw))
    env = {k: v for k, v in os.environ.items() if k != "UMX_HIP_RUNTIME"}
    env["UMX_MODELS_DIR"] = str(models)
    outs = []
    for flags in (["--labelMask", "--labelMinArea", "4"], []):
        out = str(tmp_path / ("out%d" % len(outs)))
        r = subprocess.run([sys.executable, os.path.join(ROOT, "UnMicst.py"), img, "--model", "nucleiDAPI", "--stackOutput",
                            "--outputPath", out] + flags, env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        outs.append(out)
    pages = tiffio.imread_all(os.path.join(outs[0], "crop_Probabilities_1.tif"))
    assert pages.shape == (3, 150, 171) and pages.dtype == np.uint8
    planes = np.ascontiguousarray(pages[::-1])                    # the pages are in reversed class order
    labels, table = label_ref.label(planes, 2, 4)
    assert len(table) > 1 and len(label_ref.label(planes, 2, 1)[1]) > len(table)   # nuclei were found, and the filter dropped some
    got = tiffio.imread_all(os.path.join(outs[0], "crop_Labels_1.tif"))
    assert got.dtype == np.int32 and got.shape == (1, 150, 171) and np.array_equal(got[0], labels)
    lines = open(os.path.join(outs[0], "crop_Objects_1.csv")).read().splitlines()
    assert lines[0] == "label,area,y0,x0,y1,x1,centroid_y,centroid_x" and len(lines) == 1 + len(table)
    rows = np.array([[float(v) for v in l.split(",")] for l in lines[1:]])
    assert np.array_equal(rows[:, 0], np.arange(1, len(table) + 1))
    for j, f in enumerate(("area", "y0", "x0", "y1", "x1")):
        assert np.array_equal(rows[:, 1 + j], table[f]), f
    cy, cx = label_ref.centroids(table)
    assert lines[1:] == ["%d,%d,%d,%d,%d,%d,%.6f,%.6f" % (j + 1, t["area"], t["y0"], t["x0"], t["y1"], t["x1"], cy[j], cx[j])
                         for j, t in enumerate(table)]

    # the host-side path (no raw fast path: the planes come from singleImageInference and the uint8 recipe) labels its own pages
    out = str(tmp_path / "out_host")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "UnMicst.py"), img, "--model", "nucleiDAPI", "--stackOutput", "--outputPath", out,
                        "--labelMask", "--labelMinArea", "4"], env=dict(env, UMX_NO_RAW_PATH="1"), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    host_planes = np.ascontiguousarray(tiffio.imread_all(os.path.join(out, "crop_Probabilities_1.tif"))[::-1])
    host_labels, host_table = label_ref.label(host_planes, 2, 4)
    assert np.array_equal(tiffio.imread_all(os.path.join(out, "crop_Labels_1.tif"))[0], host_labels)
    assert len(open(os.path.join(out, "crop_Objects_1.csv")).read().splitlines()) == 1 + len(host_table) > 1

    def files(d):
        return sorted(os.path.relpath(os.path.join(r, f), d) for r, _, fs in os.walk(d) for f in fs)
    label_files = ["crop_Labels_1.tif", "crop_Objects_1.csv"]
    assert files(outs[1]) == [f for f in files(outs[0]) if f not in label_files] and set(label_files) <= set(files(outs[0]))
    for f in files(outs[1]):
        assert open(os.path.join(outs[0], f), "rb").read() == open(os.path.join(outs[1], f), "rb").read(), f
