"""GPU tests of the label mask's measurement (unmicst_amd/csrc/umx_label.hip; include/umx.h and DESIGN.md section 8.1, steps 8 and 9):
the records of umx_labeler_measure / _measure_dev against tests/label_measure_ref.py, compared for equality.  Everything is an integer:
there is no tolerance anywhere in this file."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import helpers
import label_grow_ref as grow_ref
import label_measure_ref as ref
from unmicst_amd import model, tiffio, umx

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

T, HALO = umx.LABEL_GROW_TILE, umx.LABEL_GROW_HALO
MAIN = (150, 203)                              # as tests/test_gpu_label_grow.py: 38 workgroups of 4 row waves, 4 chunks a row, the last 11 pixels
RAGGED = (2 * T + HALO - 3, 3 * T + 5)
DTYPES = (np.uint8, np.uint16)
GROUPS = (1, umx.LABEL_MEASURE_GROUP, umx.LABEL_MEASURE_GROUP + 1)   # one plane, a full group, a full group and a remainder
FIELDS = ("sum", "sum_sq", "min", "max", "count", "reserved")


@functools.lru_cache(maxsize=None)
def case_of(shape, name):
    planes, cls, min_area, classes = grow_ref.case(shape[0], shape[1], name, T, HALO)
    planes.setflags(write=False)
    return planes, cls, min_area, classes


@functools.lru_cache(maxsize=None)
def pixels(shape, dtype, C):
    p = ref.pixels(shape, dtype, C, seed=shape[1])
    p.setflags(write=False)
    return p


@pytest.fixture(scope="module")
def lab():
    with umx.Labeler() as lb:
        yield lb


def same(got, want, what):
    assert got.dtype == umx.LABEL_MEASURE_DTYPE and got.shape == want.shape, (what, got.shape, want.shape)
    for f in FIELDS:
        assert np.array_equal(got[f], want[f]), (what, f)


def dev(a):
    """a numpy array as a device tensor of the same bytes (uint16 goes as int16: the kernel is given the address and the type code)"""
    import torch
    a = np.array(a)                                               # (a copy: the shared inputs are read-only)
    return torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).cuda()


def measure_ptr(lab, labels, N, planes):
    import torch
    d_labels, d_planes = dev(labels), dev(planes)
    torch.cuda.synchronize()
    C, H, W = planes.shape
    got = lab.measure_ptr(d_labels.data_ptr(), N, d_planes.data_ptr(), planes.dtype, C, H, W)
    assert np.array_equal(d_labels.cpu().numpy(), labels)         # both are only read
    assert d_planes.cpu().numpy().tobytes() == planes.tobytes()
    return got


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", [MAIN, RAGGED])
def test_cases_of_the_growth(lab, shape, dtype):
    """every case of tests/label_grow_ref.py, plain and grown: the records of the labels the run returned, by the restatement; the
    count is the table's area"""
    measured = 0
    for name in grow_ref.NAMES:
        planes, cls, min_area, classes = case_of(shape, name)
        for R in (0, 3):
            labels, table = lab.run(planes, cls, min_area, grow=R, grow_classes=classes if R else None)
            N = len(table)
            for C in GROUPS:
                px = pixels(shape, dtype, GROUPS[-1])[:C]
                got = lab.measure(px)
                same(got, ref.measure(labels, px, N), (shape, name, R, C))
                assert got.shape == (C, N) and (got["count"] == table["area"][None, :]).all()
            measured += N
    assert measured > 200                                         # the cases are not empty


@pytest.mark.parametrize("dtype", DTYPES)
def test_probability_planes_of_the_run_itself(lab, dtype):
    """what the command's pm columns are: the uint8 planes the labeler just used, here also widened to uint16"""
    planes, cls, min_area, classes = case_of(MAIN, "rings")
    labels, table = lab.run(planes, cls, min_area, grow=3, grow_classes=classes)
    px = planes.astype(dtype)
    same(lab.measure(px), ref.measure(labels, px, len(table)), "pm")
    one = lab.measure(px[1])                                      # [H, W]: one plane
    same(one, ref.measure(labels, px[1:2], len(table)), "one plane")


def boundary_labels(H, W):
    """one object covering everything (a run carried across every chunk), vertical stripes one pixel wide (every pixel a run of its
    own), a checkerboard of the stripes' labels"""
    stripes = np.tile(np.arange(1, W + 1, dtype=np.int32), (H, 1))
    yy, xx = np.mgrid[0:H, 0:W]
    return (("one", np.ones((H, W), np.int32), 1), ("stripes", stripes, W),
            ("checkerboard", np.where((yy + xx) % 2 == 0, stripes, 0).astype(np.int32), W))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("H", [1, 3, 4, 5])
def test_chunk_and_row_wave_boundaries(lab, H, dtype):
    """W round the 64-pixel chunk, H round the 4 rows of a workgroup"""
    umx.require_torch_runtime("test_gpu_label_measure")
    for W in (1, 63, 64, 65, 127, 128, 129):
        px = pixels((H, W), dtype, 2)
        for name, labels, N in boundary_labels(H, W):
            same(measure_ptr(lab, labels, N, px), ref.measure(labels, px, N), (H, W, name))


@pytest.mark.parametrize("dtype", DTYPES)
def test_sums_past_32_bits(lab, dtype):
    """H = 2, W = 70 001, one object, every pixel the type's maximum: at uint16 one row run sums to 4 587 515 535 > 2^32, the object's
    sum_sq to 6.0e14"""
    H, W = 2, 70001
    planes = case_of((H, W), "full")[0]                           # "full": every pixel is of class 1
    top = int(np.iinfo(dtype).max)
    labels, table = lab.run(planes, 1, 1)
    assert len(table) == 1 and table["area"][0] == H * W and (labels == 1).all()
    got = lab.measure(np.full((1, H, W), top, dtype))
    assert got.shape == (1, 1)
    r = got[0, 0]
    assert (int(r["count"]), int(r["sum"]), int(r["sum_sq"]), int(r["min"]), int(r["max"])) == (H * W, H * W * top, H * W * top * top, top, top)
    if dtype == np.uint16:
        assert W * top > 2 ** 32 and int(r["sum"]) > 2 ** 32 and 5.9e14 < int(r["sum_sq"]) < 6.1e14
    px = pixels((H, W), dtype, 2)
    same(lab.measure(px), ref.measure(labels, px, 1), "random pixels on the long run")


def test_a_plane_of_ones(lab):
    planes, cls, min_area, classes = case_of(RAGGED, "rings")
    labels, table = lab.run(planes, cls, min_area, grow=2, grow_classes=classes)
    for dtype in DTYPES:
        got = lab.measure(np.ones((3,) + RAGGED, dtype))
        assert got.shape == (3, len(table)) and len(table) > 100
        for f in ("sum", "sum_sq", "count"):
            assert np.array_equal(got[f], np.broadcast_to(table["area"], got.shape)), f
        assert (got["min"] == 1).all() and (got["max"] == 1).all()


def sprinkled(labels, N, seed=7):
    """the labels with -5, N + 1 and 2^31 - 1 sprinkled in, and label `gone` (in 1..N) taken from every pixel that carried it"""
    rng = np.random.default_rng(seed)
    out = labels.copy()
    gone = N // 2 + 1
    out[out == gone] = 0
    hit = rng.random(out.shape)
    out[hit < 0.03] = -5
    out[(hit >= 0.03) & (hit < 0.06)] = N + 1
    out[(hit >= 0.06) & (hit < 0.09)] = 2 ** 31 - 1
    assert (out == -5).any() and (out == N + 1).any() and (out == 2 ** 31 - 1).any() and not (out == gone).any()
    return out, gone


@pytest.mark.parametrize("dtype", DTYPES)
def test_measure_ptr_on_torch_tensors_equals_the_host_entry(lab, dtype):
    umx.require_torch_runtime("test_gpu_label_measure")
    planes, cls, min_area, classes = case_of(RAGGED, "rings")
    labels, table = lab.run(planes, cls, min_area, grow=3, grow_classes=classes)
    N = len(table)
    px = pixels(RAGGED, dtype, GROUPS[-1])
    host = lab.measure(px)
    got = measure_ptr(lab, labels, N, px)
    assert got.tobytes() == host.tobytes()
    assert lab.measure(px).tobytes() == host.tobytes()            # the device entry left the resident labels alone
    bad, gone = sprinkled(labels, N)
    got = measure_ptr(lab, bad, N, px)
    same(got, ref.measure(bad, px, N), "labels outside 0..N")
    for c in range(px.shape[0]):
        e = got[c, gone - 1]
        assert (int(e["count"]), int(e["sum"]), int(e["sum_sq"]), int(e["min"]), int(e["max"])) == (0, 0, 0, 2 ** 32 - 1, 0)
    none = measure_ptr(lab, labels, 0, px)                        # no object asked for: no record
    assert none.shape == (px.shape[0], 0)


_GUARD_CHILD = """
import sys
sys.path.insert(0, %r); sys.path.insert(0, %r)
import numpy as np
import torch
import label_grow_ref as grow_ref
import label_measure_ref as ref
from unmicst_amd import umx
umx.require_torch_runtime("test_gpu_label_measure")
T, HALO = umx.LABEL_GROW_TILE, umx.LABEL_GROW_HALO
shape = (2 * T + HALO - 3, 3 * T + 5)
planes, cls, min_area, classes = grow_ref.case(shape[0], shape[1], "rings", T, HALO)
with umx.Labeler() as lb:
    labels, table = lb.run(planes, cls, min_area, grow=3, grow_classes=classes)
    N = len(table)
    bad = labels.copy()
    hit = np.random.default_rng(7).random(bad.shape)
    bad[bad == N // 2 + 1] = 0
    bad[hit < 0.03] = -5; bad[(hit >= 0.03) & (hit < 0.06)] = N + 1; bad[(hit >= 0.06) & (hit < 0.09)] = 2 ** 31 - 1
    d_labels = torch.from_numpy(bad).cuda()
    for dtype in (np.uint8, np.uint16):
        for C in (1, 4, 5):
            px = ref.pixels(shape, dtype, C, seed=C)
            got = lb.measure(px)                                  # (raises UmxError 7 when a red zone was written)
            assert got.tobytes() == ref.measure(labels, px, N).tobytes(), (dtype, C, "host")
            d_px = torch.from_numpy(px.view(np.int16) if dtype == np.uint16 else px).cuda()
            torch.cuda.synchronize()
            got = lb.measure_ptr(d_labels.data_ptr(), N, d_px.data_ptr(), dtype, C, shape[0], shape[1])
            assert got.tobytes() == ref.measure(bad, px, N).tobytes(), (dtype, C, "device")
    again, _ = lb.run(planes, cls, min_area, grow=3, grow_classes=classes)
    assert np.array_equal(again, labels)
print("guard-ok")
"""


def test_guard_mode_finds_no_write_outside_the_buffers():
    """UMX_DEBUG_GUARD in a child process: red zones round the planes, the staging and the records, which are exactly one group's
    size at a shape's first measurement; both entries end with UMX_OK and the right records, labels outside 0..N included."""
    env = dict(os.environ, UMX_DEBUG_GUARD="1")
    r = subprocess.run([sys.executable, "-c", _GUARD_CHILD % (ROOT, os.path.join(ROOT, "tests"))], env=env, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0 and "guard-ok" in r.stdout, r.stderr[-2000:]


def refused(lab, planes, word):
    with pytest.raises(umx.UmxError) as e:
        lab.measure(planes)
    assert e.value.code == umx.ERR_INVALID and word in str(e.value), str(e.value)


def test_resident_labels():
    umx.require_torch_runtime("test_gpu_label_measure")
    import torch
    planes, cls, min_area, classes = case_of(MAIN, "rings")
    px = pixels(MAIN, np.uint16, 2)
    with umx.Labeler() as lb:
        refused(lb, px, "no labels to measure")                   # before any run
        labels, table = lb.run(planes, cls, min_area)
        want = ref.measure(labels, px, len(table))
        a = lb.measure(px)
        same(a, want, "after a run")
        assert lb.measure(px).tobytes() == a.tobytes()            # twice: the same bytes
        refused(lb, pixels(RAGGED, np.uint16, 2), "150 x 203")    # another shape
        with pytest.raises(TypeError):
            lb.measure(px.astype(np.float32))
        with pytest.raises(umx.UmxError):
            lb.run(planes, cls, 0)                                # a refused run (min_area 0) ...
        same(lb.measure(px), want, "after a refused run")         # ... leaves the resident labels as they were
        n = umx.ctypes.c_int64(-1)
        out = np.zeros((2, len(table)), umx.LABEL_MEASURE_DTYPE)
        code = umx.MEASURE_U16
        assert lb._L.umx_labeler_measure(lb._lb, None, code, 2, 150, 203, None, 0, umx.ctypes.byref(n)) == 0 and n.value == len(table)
        rc = lb._L.umx_labeler_measure(lb._lb, px.ctypes.data, code, 2, 150, 203, out.ctypes.data, out.size - 1, None)   # cap < C * N
        assert rc == umx.ERR_INVALID and "records" in lb._L.umx_labeler_last_error(lb._lb).decode()
        assert not out.view(np.uint8).any()                       # nothing was touched
        same(lb.measure(px), want, "after refused measurements")
        _, t2 = lb.run(planes, cls, min_area, want_labels=False)
        assert len(t2) == len(table)
        refused(lb, px, "no label plane")                         # a later run without a label plane
        lb.run(planes, cls, min_area)
        same(lb.measure(px), want, "after a run with labels again")
        d_planes = torch.from_numpy(np.array(planes)).cuda()
        d_labels = torch.zeros(MAIN, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        lb.run_ptr(d_planes.data_ptr(), 3, MAIN[0], MAIN[1], d_labels.data_ptr(), cls, min_area)
        refused(lb, px, "umx_labeler_run_dev")                    # the device run leaves its labels with the caller
        labels2, table2 = lb.run(planes, cls, min_area, grow=2, grow_classes=classes)
        same(lb.measure(px), ref.measure(labels2, px, len(table2)), "usable after every refusal")


def test_staging_larger_than_the_labelers_planes_keeps_the_labels():
    """a run on a K = 1 stack, then five uint16 planes: the staging of one group (4 x 2 bytes a pixel) is larger than the labeler's
    plane buffer (1 byte a pixel), and growing it must not empty the arena that holds the labels"""
    planes = np.ascontiguousarray(case_of(MAIN, "rings")[0][2:3])
    mask_planes = np.where(planes > 100, 255, 0).astype(np.uint8)  # K = 1: every pixel is of class 0; one object, the whole image
    px = pixels(MAIN, np.uint16, 5)
    three, cls, min_area, classes = case_of(MAIN, "rings")
    with umx.Labeler() as fresh:
        labels3, table3 = fresh.run(three, cls, min_area)
        want = fresh.measure(px)
    same(want, ref.measure(labels3, px, len(table3)), "a fresh labeler")
    with umx.Labeler() as lb:
        labels, table = lb.run(mask_planes, 0, 1)
        assert len(table) == 1 and (labels == 1).all()
        got = lb.measure(px)
        same(got, ref.measure(labels, px, 1), "K = 1, then C = 5")
        again, _ = lb.run(mask_planes, 0, 1)
        assert np.array_equal(again, labels)
    # the same with labels worth keeping: three planes, but measured planes that still outgrow them (5 uint16 > 3 uint8 a pixel)
    with umx.Labeler() as lb:
        labels, table = lb.run(three, cls, min_area)
        assert np.array_equal(labels, labels3)
        got = lb.measure(px)
        assert got.tobytes() == want.tobytes()
        assert lb.measure(px[:1]).tobytes() == want[:1].tobytes()
        again, _ = lb.run(three, cls, min_area)
        assert np.array_equal(again, labels3)


def run_command(tmp_path, img, sub, flags, env):
    out = str(tmp_path / sub)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "UnMicst.py"), img, "--model", "nucleiDAPI", "--stackOutput", "--outputPath", out,
                        "--labelMask", "--labelGrow", "2"] + flags, env=env, capture_output=True, text=True, timeout=600)
    return out, r


def test_command_measures_the_label_mask(tmp_path):
    """UnMicst.py --stackOutput --labelMask --labelGrow 2 --labelMeasure on a 3-page uint16 TIFF of 96 x 130 (a crop of sample 105, the
    crop turned upside down, random pixels): the Intensities file is the restatement applied to the Labels page and the Probabilities
    pages the same run wrote and to the input's pages; without the flag every other file has the same bytes and there is no such file;
    a float32 page is refused and leaves none."""
    hp, blob, mean, std = helpers.load_nuclei_dapi()
    models = tmp_path / "models"
    model.save_converted(model.ModelArtefacts(hp, blob, mean, std), str(models / "nucleiDAPI"))
    raw = np.ascontiguousarray(helpers.load_sample_105()[0][300:396, 200:330]).astype(np.uint16)
    pages = [raw, np.ascontiguousarray(raw[::-1]), ref.pixels(raw.shape, np.uint16, 1, seed=11)[0]]
    reg = tmp_path / "x" / "registration"
    os.makedirs(reg)
    img = str(reg / "crop.tif")
    for i, page in enumerate(pages):
        tiffio.imsave(img, page, append=i > 0)
    env = {k: v for k, v in os.environ.items() if k != "UMX_HIP_RUNTIME"}
    env["UMX_MODELS_DIR"] = str(models)
    env["UMX_SYNTHETIC_WEIGHTS"] = "1"
    plain, r = run_command(tmp_path, img, "plain", [], env)
    assert r.returncode == 0, r.stderr[-2000:]
    names = sorted(os.listdir(plain))
    assert "crop_Labels_1.tif" in names and not [n for n in names if "Intensities" in n]
    for sub, flags, measured in (("all", ["--labelMeasure"], [0, 1, 2]), ("some", ["--labelMeasure", "2", "0"], [2, 0])):
        out, r = run_command(tmp_path, img, sub, flags, env)
        assert r.returncode == 0, r.stderr[-2000:]
        assert sorted(os.listdir(out)) == sorted(names + ["crop_Intensities_1.csv"])
        for n in names:                                           # every other file: the bytes of the run without the flag
            a, b = os.path.join(plain, n), os.path.join(out, n)
            if os.path.isdir(a):
                assert sorted(os.listdir(a)) == sorted(os.listdir(b))
                for q in os.listdir(a):
                    assert open(os.path.join(a, q), "rb").read() == open(os.path.join(b, q), "rb").read(), (sub, n, q)
            else:
                assert open(a, "rb").read() == open(b, "rb").read(), (sub, n)
        labels = tiffio.imread_all(os.path.join(out, "crop_Labels_1.tif"))[0]
        pm = np.ascontiguousarray(tiffio.imread_all(os.path.join(out, "crop_Probabilities_1.tif"))[::-1])   # pages: reversed class order
        area = [int(line.split(",")[1]) for line in open(os.path.join(out, "crop_Objects_1.csv")).read().splitlines()[1:]]
        N = len(area)
        assert N > 1 and labels.max() == N and pm.shape == (3, 96, 130) and pm.dtype == np.uint8
        planes = [("pm%d" % k, ref.measure(labels, pm[k], N)[0]) for k in range(3)]
        planes += [("ch%d" % p, ref.measure(labels, pages[p], N)[0]) for p in measured]
        for _, rec in planes:
            assert np.array_equal(rec["count"], area)
        assert open(os.path.join(out, "crop_Intensities_1.csv")).read().splitlines() == ref.csv_lines(area, planes), sub
    bad = str(reg / "withfloat.tif")
    tiffio.imsave(bad, raw)
    tiffio.imsave(bad, raw.astype(np.float32), append=True)
    out, r = run_command(tmp_path, bad, "float", ["--labelMeasure"], env)
    assert r.returncode != 0 and "page 1" in r.stderr and "float32" in r.stderr, r.stderr[-2000:]
    assert not [n for n in os.listdir(out) if "Intensities" in n]
