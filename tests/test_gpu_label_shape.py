"""GPU tests of the label mask's shapes (unmicst_amd/csrc/umx_label.hip; include/umx.h and DESIGN.md section 8.1, steps 16 to 18): the
records of umx_labeler_shape / _shape_dev against tests/label_shape_ref.py, compared for equality.  Everything is an integer: there
is no tolerance anywhere in this file."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import helpers
import label_grow_ref as grow_ref
import label_ref
import label_shape_ref as ref
from unmicst_amd import driver, model, tiffio, umx

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

T, HALO = umx.LABEL_GROW_TILE, umx.LABEL_GROW_HALO
BLOBS = (200, 264)                             # 50 workgroups of 4 row waves, 5 chunks a row, the last 8 pixels
FIELDS = ref.MOMENTS + ref.QUADS + ("reserved",)
WIDTHS, HEIGHTS = (1, 63, 64, 65, 129, 200), (1, 3, 4, 5, 9)


@pytest.fixture(scope="module")
def lab():
    with umx.Labeler() as lb:
        yield lb


@functools.lru_cache(maxsize=None)
def rings():
    planes, cls, min_area, classes = grow_ref.case(BLOBS[0], BLOBS[1], "rings", T, HALO)
    planes.setflags(write=False)
    return planes, cls, min_area, classes


@functools.lru_cache(maxsize=None)
def blobs():
    planes, cls, min_area = label_ref.case(BLOBS[0], BLOBS[1], "blobs")
    planes.setflags(write=False)
    return planes, cls, min_area


@functools.lru_cache(maxsize=None)
def want(H, W):
    """the seeded pattern of a size and its restatement, computed once"""
    labels, N = ref.seeded_labels(H, W)
    rec = ref.records(labels, N)
    labels.setflags(write=False)
    rec.setflags(write=False)
    return labels, N, rec


def same(got, wanted, what):
    assert got.dtype == umx.LABEL_SHAPE_DTYPE and got.shape == wanted.shape, (what, got.shape, wanted.shape)
    for f in FIELDS:
        assert np.array_equal(got[f], wanted[f]), (what, f, got[f][:8], wanted[f][:8])


def shape_ptr(lab, labels, N):
    import torch
    d_labels = torch.from_numpy(np.array(labels, np.int32)).cuda()   # (a copy: the shared inputs are read-only)
    torch.cuda.synchronize()
    got = lab.shape_ptr(d_labels.data_ptr(), N, labels.shape[0], labels.shape[1])
    assert np.array_equal(d_labels.cpu().numpy(), labels)            # only read
    return got


@pytest.mark.parametrize("H", HEIGHTS)
def test_chunk_and_row_group_boundaries(lab, H):
    """W round the 64-pixel chunk and its multiples, H round the 4 rows of a workgroup; runs that end on, before and after lanes 63 /
    64, one run longer than 128 pixels, rows of one-pixel runs"""
    umx.require_torch_runtime("test_gpu_label_shape")
    for W in WIDTHS:
        labels, N, rec = want(H, W)
        same(shape_ptr(lab, labels, N), rec, (H, W))
    assert any((want(h, 200)[0][1::4, 3:136] > 0).all() for h in HEIGHTS if h > 1)   # the long run is there


def test_hand_made_planes(lab):
    """borders and corners, one and two holes, holes that touch diagonally, labels meeting at a corner and along an edge, a label in
    pieces, a checkerboard, values outside 1..N, N = 0"""
    umx.require_torch_runtime("test_gpu_label_shape")
    for name, labels, N, euler_known in ref.hand_made():
        got = shape_ptr(lab, labels, N)
        rec, edges, holes, area = ref.shapes(labels, N)
        same(got, rec, name)
        d = umx.shape_descriptors(got)
        assert np.array_equal(d["area"], area) and np.array_equal(d["perimeter_edges"], edges), name
        for j, e in euler_known.items():
            assert d["euler"][j - 1] == e, (name, j)
        if name in ("ring", "frame", "diagonal holes"):
            assert np.array_equal(d["holes"], holes), name
        if name == "checkerboard":
            assert got["q2"][0] == 0 and got["q3"][0] == 0 and got["q4"][0] == 0 and got["q1"][0] > 0 and got["qd"][0] > 0
        if name == "N = 0":
            assert got.shape == (0,)


@pytest.mark.parametrize("shape", [(65536, 8), (4, 65536)])
def test_sums_past_32_bits(lab, shape):
    """a full-height column object on 65536 x 8 and a full-width row object on 4 x 65536: sum_yy (sum_xx) is 65535 * 65536 * 131071 / 6
    = 9.4e13 a column (row), far past 2^32, and a row run of 65536 pixels is carried across 1024 chunks"""
    umx.require_torch_runtime("test_gpu_label_shape")
    H, W = shape
    labels = np.zeros(shape, np.int32)
    n = max(H, W)
    if H > W:
        labels[:, 2:5] = 1                                           # three columns, every row a run of 3
        labels[::2, 6] = 2                                           # one-pixel runs in every second row
        first, second = ("sum_yy", 3 * ((n - 1) * n * (2 * n - 1) // 6)), ("sum_xy", (n - 1) * n // 2 * 9)
    else:
        labels[1:3, :] = 1                                           # two full rows
        labels[3, 5:W - 7:2] = 2
        first, second = ("sum_xx", 2 * ((n - 1) * n * (2 * n - 1) // 6)), ("sum_xy", (n - 1) * n // 2 * 3)
    got = shape_ptr(lab, labels, 2)
    assert int(got[first[0]][0]) == first[1] > 2 ** 32 and int(got[second[0]][0]) == second[1] > 2 ** 32
    same(got, ref.records(labels, 2), shape)
    d = umx.shape_descriptors(got)
    assert d["area"][0] == (3 if H > W else 2) * n and d["holes"][0] == 0


def run_cases():
    planes, cls, min_area, classes = rings()
    bplanes, bcls, bmin = blobs()
    return (("plain", planes, dict(cls=cls, min_area=min_area)),
            ("grow", planes, dict(cls=cls, min_area=min_area, grow=3, grow_classes=classes)),
            ("split", bplanes, dict(cls=bcls, min_area=bmin, split=2)))


def test_labels_of_the_run_itself(lab):
    """Labeler.run then shape(), plain, grown and split: the restatement on the labels the run returned; the area the window counts
    give and the first moments are the object table's; holes is scipy's count (the run's objects are 4-connected)"""
    seen = 0
    for name, planes, kw in run_cases():
        labels, table = lab.run(planes, **kw)
        N = len(table)
        got = lab.shape()
        rec, edges, holes, area = ref.shapes(labels, N)
        same(got, rec, name)
        d = umx.shape_descriptors(got)
        assert np.array_equal(d["area"], table["area"]), name
        assert np.array_equal(got["sum_y"], table["sum_y"]) and np.array_equal(got["sum_x"], table["sum_x"]), name
        assert np.array_equal(d["holes"], holes) and np.array_equal(d["perimeter_edges"], edges), name
        assert lab.shape().tobytes() == got.tobytes()                # twice: the same bytes
        k, dl = lab.shape_last_ms()
        assert k > 0.0 and dl > 0.0
        seen += N
    assert seen > 100


def test_shape_ptr_on_torch_tensors_equals_the_host_entry(lab):
    umx.require_torch_runtime("test_gpu_label_shape")
    planes, cls, min_area, classes = rings()
    labels, table = lab.run(planes, cls, min_area, grow=3, grow_classes=classes)
    host = lab.shape()
    assert shape_ptr(lab, labels, len(table)).tobytes() == host.tobytes()
    assert lab.shape().tobytes() == host.tobytes()                   # the device entry left the resident labels alone
    fewer = shape_ptr(lab, labels, len(table) - 3)                   # the last three labels are now outside 1..N
    assert fewer.tobytes() == host[:-3].tobytes()


def refused(call, word):
    with pytest.raises(umx.UmxError) as e:
        call()
    assert e.value.code == umx.ERR_INVALID and word in str(e.value), str(e.value)


def test_refusals_leave_the_resident_labels():
    umx.require_torch_runtime("test_gpu_label_shape")
    import torch
    planes, cls, min_area, classes = rings()
    H, W = BLOBS
    with umx.Labeler() as lb:
        refused(lb.shape, "no labels")                               # before any run
        labels, table = lb.run(planes, cls, min_area)
        N = len(table)
        wanted = ref.records(labels, N)
        same(lb.shape(), wanted, "after a run")
        refused(lambda: lb.shape(W, H), "200 x 264")                 # another shape
        refused(lambda: lb.shape(0, W), "at least 1")
        refused(lambda: lb.shape(65537, W), "65536")
        with pytest.raises(umx.UmxError):
            lb.run(planes, cls, 0)                                   # a refused run (min_area 0) ...
        same(lb.shape(), wanted, "after a refused run")              # ... leaves the resident labels as they were
        n = umx.ctypes.c_int64(-1)
        out = np.zeros(N, umx.LABEL_SHAPE_DTYPE)
        assert lb._L.umx_labeler_shape(lb._lb, H, W, None, 0, umx.ctypes.byref(n)) == 0 and n.value == N
        rc = lb._L.umx_labeler_shape(lb._lb, H, W, out.ctypes.data, N - 1, None)   # cap < N
        assert rc == umx.ERR_INVALID and "records" in lb._L.umx_labeler_last_error(lb._lb).decode()
        assert not out.view(np.uint8).any()                          # nothing was touched
        d_labels = torch.from_numpy(np.array(labels)).cuda()
        torch.cuda.synchronize()
        rc = lb._L.umx_labeler_shape_dev(lb._lb, umx.ctypes.c_void_p(d_labels.data_ptr()), N, H, W, out.ctypes.data, N - 1)
        assert rc == umx.ERR_INVALID and not out.view(np.uint8).any()
        refused(lambda: lb.shape_ptr(d_labels.data_ptr(), -1, H, W), "n_objects")
        refused(lambda: lb.shape_ptr(0, N, H, W), "null")
        same(lb.shape(), wanted, "after refused shape calls")
        _, t2 = lb.run(planes, cls, min_area, want_labels=False)
        assert len(t2) == N
        refused(lb.shape, "no label plane")                          # a later run without a label plane
        lb.run(planes, cls, min_area)
        same(lb.shape(), wanted, "after a run with labels again")
        d_planes = torch.from_numpy(np.array(planes)).cuda()
        d_out = torch.zeros(BLOBS, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        lb.run_ptr(d_planes.data_ptr(), 3, H, W, d_out.data_ptr(), cls, min_area)
        refused(lb.shape, "umx_labeler_run_dev")                     # the device run leaves its labels with the caller
        same(lb.shape_ptr(d_out.data_ptr(), N, H, W), wanted, "the device run's own labels")
        labels2, table2 = lb.run(planes, cls, min_area, grow=2, grow_classes=classes)
        same(lb.shape(), ref.records(labels2, len(table2)), "usable after every refusal")
        px = np.ones((1,) + BLOBS, np.uint8)
        assert np.array_equal(lb.measure(px)["count"][0], table2["area"])   # the measurement and the shapes share the arena
        same(lb.shape(), ref.records(labels2, len(table2)), "after a measurement")


_GUARD_CHILD = """
import sys
sys.path.insert(0, %r); sys.path.insert(0, %r)
import numpy as np
import torch
import label_grow_ref as grow_ref
import label_shape_ref as ref
from unmicst_amd import umx
umx.require_torch_runtime("test_gpu_label_shape")
T, HALO = umx.LABEL_GROW_TILE, umx.LABEL_GROW_HALO
shape = (2 * T + HALO - 3, 3 * T + 5)
planes, cls, min_area, classes = grow_ref.case(shape[0], shape[1], "rings", T, HALO)
with umx.Labeler() as lb:
    labels, table = lb.run(planes, cls, min_area, grow=3, grow_classes=classes)
    N = len(table)
    got = lb.shape()                                              # (raises UmxError 7 when a red zone was written)
    assert got.tobytes() == ref.records(labels, N).tobytes(), "host"
    bad = labels.copy()
    hit = np.random.default_rng(7).random(bad.shape)
    bad[hit < 0.03] = -5; bad[(hit >= 0.03) & (hit < 0.06)] = N + 1; bad[(hit >= 0.06) & (hit < 0.09)] = 2 ** 31 - 1
    d_labels = torch.from_numpy(bad).cuda()
    torch.cuda.synchronize()
    got = lb.shape_ptr(d_labels.data_ptr(), N, shape[0], shape[1])
    assert got.tobytes() == ref.records(bad, N).tobytes(), "device"
    again, _ = lb.run(planes, cls, min_area, grow=3, grow_classes=classes)
    assert np.array_equal(again, labels)
print("guard-ok")
"""


def test_guard_mode_finds_no_write_outside_the_buffers():
    """UMX_DEBUG_GUARD in a child process: red zones round the planes and the records, which are exactly N records at a labeler's
    first shape call; both entries end with UMX_OK and the right records on a ragged plane, labels outside 0..N included."""
    env = dict(os.environ, UMX_DEBUG_GUARD="1")
    r = subprocess.run([sys.executable, "-c", _GUARD_CHILD % (ROOT, os.path.join(ROOT, "tests"))], env=env, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0 and "guard-ok" in r.stdout, r.stderr[-2000:]


def test_command_writes_the_shapes_and_changes_nothing_else(tmp_path):
    """UnMicst.py --stackOutput --labelMask --labelGrow 2 [--labelShape] on a 96 x 130 crop of sample 105: the Shapes file's integer
    columns are the restatement on the Labels page the same run wrote, its float columns shape_descriptors of them digit for digit;
    every other file has the bytes of the run without the flag, which writes no Shapes file; without --labelMask the flag is the
    parser's error."""
    hp, blob, mean, std = helpers.load_nuclei_dapi()
    models = tmp_path / "models"
    model.save_converted(model.ModelArtefacts(hp, blob, mean, std), str(models / "nucleiDAPI"))
    raw = np.ascontiguousarray(helpers.load_sample_105()[0][300:396, 200:330]).astype(np.uint16)
    reg = tmp_path / "x" / "registration"
    os.makedirs(reg)
    img = str(reg / "crop.tif")
    tiffio.imsave(img, raw)
    env = {k: v for k, v in os.environ.items() if k != "UMX_HIP_RUNTIME"}
    env["UMX_MODELS_DIR"] = str(models)
    env["UMX_SYNTHETIC_WEIGHTS"] = "1"

    def command(sub, flags):
        out = str(tmp_path / sub)
        r = subprocess.run([sys.executable, os.path.join(ROOT, "UnMicst.py"), img, "--model", "nucleiDAPI", "--stackOutput", "--outputPath",
                            out] + flags, env=env, capture_output=True, text=True, timeout=600)
        return out, r

    def files(d):
        return sorted(os.path.relpath(os.path.join(r, f), d) for r, _, fs in os.walk(d) for f in fs)
    plain, r = command("plain", ["--labelMask", "--labelGrow", "2"])
    assert r.returncode == 0, r.stderr[-2000:]
    out, r = command("shape", ["--labelMask", "--labelGrow", "2", "--labelShape"])
    assert r.returncode == 0, r.stderr[-2000:]
    assert "crop_Labels_1.tif" in files(plain) and not [f for f in files(plain) if "Shapes" in f]
    assert files(out) == sorted(files(plain) + ["crop_Shapes_1.csv"])
    for f in files(plain):
        assert open(os.path.join(plain, f), "rb").read() == open(os.path.join(out, f), "rb").read(), f
    labels = tiffio.imread_all(os.path.join(out, "crop_Labels_1.tif"))[0]
    table = [[int(v) for v in line.split(",")[:6]] for line in open(os.path.join(out, "crop_Objects_1.csv")).read().splitlines()[1:]]
    N = len(table)
    assert N > 1 and labels.max() == N
    rec, edges, holes, area = ref.shapes(labels, N)
    d = umx.shape_descriptors(rec)
    lines = open(os.path.join(out, "crop_Shapes_1.csv")).read().splitlines()
    assert lines[0] == ",".join(driver.SHAPE_COLUMNS) and len(lines) == N + 1
    for j, line in enumerate(lines[1:]):
        f = line.split(",")
        _, a, y0, x0, y1, x1 = table[j]
        assert [int(f[k]) for k in (0, 1, 2, 4, 5)] == [j + 1, a, edges[j], 1 - holes[j], holes[j]] and a == area[j], j
        want_floats = [d[n][j] for n in ("perimeter", "major_axis_length", "minor_axis_length", "eccentricity", "orientation")]
        want_floats.append(a / ((y1 - y0 + 1) * (x1 - x0 + 1)))
        assert [f[k] for k in (3, 6, 7, 8, 9, 10)] == [repr(float(v)) for v in want_floats], j
        assert [float(f[k]) for k in (3, 6, 7, 8, 9, 10)] == [float(v) for v in want_floats], j
    out, r = command("nomask", ["--labelShape"])
    assert r.returncode == 2 and "--labelShape needs --labelMask" in r.stderr, r.stderr[-2000:]
    assert not os.path.exists(out) or not [f for f in files(out) if "Shapes" in f]
