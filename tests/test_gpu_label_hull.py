"""GPU tests of the label mask's hulls (unmicst_amd/csrc/umx_label_hull.hip; include/umx.h and DESIGN.md section 8.1, steps 25 to 28):
the records and the vertex list of umx_labeler_hull / _hull_dev against tests/label_hull_ref.py, compared for equality.  Everything
is an integer: there is no tolerance anywhere in this file."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import helpers
import label_grow_ref as grow_ref
import label_hull_ref as ref
import label_ref
from unmicst_amd import driver, model, tiffio, umx

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

T, HALO = umx.LABEL_GROW_TILE, umx.LABEL_GROW_HALO
BLOBS = (200, 264)                             # 50 workgroups of 4 row waves, 5 chunks a row, the last 8 pixels
WIDTHS, HEIGHTS = (1, 63, 64, 65, 129, 200), (1, 3, 4, 5, 9)
ERR_OOM = 5                                    # UMX_ERR_OOM


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
    rec, verts = ref.hulls(labels, N)
    for a in (labels, rec, verts):
        a.setflags(write=False)
    return labels, N, rec, verts


def same(got, wanted, what):
    """(records, vertices) twice: every field equal, and so the bytes"""
    assert got[0].dtype == umx.LABEL_HULL_DTYPE and got[1].dtype == umx.LABEL_HULL_VERTEX_DTYPE, what
    assert got[0].shape == wanted[0].shape, (what, got[0].shape, wanted[0].shape)
    for f in umx.LABEL_HULL_DTYPE.names:
        assert np.array_equal(got[0][f], wanted[0][f]), (what, f, got[0][f][:8], wanted[0][f][:8])
    assert got[1].shape == wanted[1].shape, (what, got[1].shape, wanted[1].shape)
    for f in ("y", "x"):
        assert np.array_equal(got[1][f], wanted[1][f]), (what, f, got[1][f][:12], wanted[1][f][:12])
    assert got[0].tobytes() == wanted[0].tobytes() and got[1].tobytes() == wanted[1].tobytes(), what


def hull_ptr(lab, labels, N):
    import torch
    d_labels = torch.from_numpy(np.array(labels, np.int32)).cuda()   # (a copy: the shared inputs are read-only)
    torch.cuda.synchronize()
    got = lab.hull_ptr(d_labels.data_ptr(), N, labels.shape[0], labels.shape[1])
    assert np.array_equal(d_labels.cpu().numpy(), labels)            # only read
    return got


@pytest.mark.parametrize("H", HEIGHTS)
def test_chunk_and_row_group_boundaries(lab, H):
    """W round the 64-pixel chunk and its multiples, H round the 4 rows of a workgroup; runs that end on, before and after lanes 63 /
    64, one run longer than 128 pixels, rows of one-pixel runs; labels in several pieces"""
    umx.require_torch_runtime("test_gpu_label_hull")
    for W in WIDTHS:
        labels, N, rec, verts = want(H, W)
        same(hull_ptr(lab, labels, N), (rec, verts), (H, W))
    assert any((want(h, 200)[0][1::4, 3:136] > 0).all() for h in HEIGHTS if h > 1)   # the long run is there


def test_hand_made_planes(lab):
    """one pixel, the full plane as one object, staircases and lenses (every level a vertex, the bound of 2 rows + 2 attained), an L
    and a ring, two combs whose hulls overlap, a label in far-apart pieces, a label no pixel carries, values outside 1..N, N = 0"""
    umx.require_torch_runtime("test_gpu_label_hull")
    seen = set()
    for name, labels, N in ref.hand_made():
        got = hull_ptr(lab, labels, N)
        same(got, ref.hulls(labels, N), name)
        seen.add(name)
        rec, verts = got
        if name in ("one pixel", "full plane"):
            assert rec["n_vertices"][0] == 4 and rec["area2"][0] == 2 * int((labels == 1).sum())    # solidity 1
        if name in ("staircase of two", "lens", "tall lens"):
            assert rec["n_vertices"][0] == 2 * rec["rows"][0] + 2
        if name == "far-apart pieces":
            assert rec["rows"][0] == 9 < 36                          # rows of the box without a pixel
        if name == "a label without pixels":
            assert rec[1].tolist() == (0, 0, 4, 0, 0)
        if name == "N = 0":
            assert rec.shape == (0,) and verts.shape == (0,)
    assert {"L", "ring", "combs", "outside 1..N"} <= seen


@pytest.mark.parametrize("r", [100, 1000])
def test_discs_past_the_waves_64_in_levels_and_vertices(lab, r):
    """a disc of radius 100 on 201 x 201: more than 64 levels, 72 vertices; of radius 1000 on 2001 x 2001: 408 vertices"""
    umx.require_torch_runtime("test_gpu_label_hull")
    labels = ref.disc(r)
    got = hull_ptr(lab, labels, 1)
    same(got, ref.hulls(labels, 1), r)
    known = {100: (72, 63462, 40562), 1000: (408, 6290346, 4005602)}[r]
    assert (int(got[0]["n_vertices"][0]), int(got[0]["area2"][0]), int(got[0]["feret_max_sq"][0])) == known
    assert got[0]["rows"][0] == 2 * r + 1 and len(got[1]) == known[0]


def test_several_hundred_small_objects(lab):
    """500 objects of three rows in one plane: many objects per workgroup, whatever the assignment"""
    umx.require_torch_runtime("test_gpu_label_hull")
    labels, N = ref.many_small()
    assert N == 500
    got = hull_ptr(lab, labels, N)
    same(got, ref.hulls(labels, N), "many small")
    assert (got[0]["rows"] == 3).all() and len(set(got[0]["n_vertices"].tolist())) > 3


@pytest.mark.parametrize("shape", [(65536, 8), (4, 65536)])
def test_distances_past_32_bits(lab, shape):
    """a full-height column object on 65536 x 8 and a full-width row object on 4 x 65536: feret_max_sq = 65536^2 + 3^2 (2^2) is past
    2^32, E is 65536 for one object (one row of 65536 pixels carried across 1024 chunks)"""
    umx.require_torch_runtime("test_gpu_label_hull")
    H, W = shape
    labels = np.zeros(shape, np.int32)
    if H > W:
        labels[:, 2:5] = 1                                           # three columns, every row a run of 3
        labels[::2, 6] = 2                                           # one-pixel runs in every second row
        first = (2 * 3 * 65536, 2 ** 32 + 9, 0, 4, 65536)
    else:
        labels[1:3, :] = 1                                           # two full rows
        labels[3, 5:W - 7:2] = 2
        first = (2 * 2 * 65536, 2 ** 32 + 4, 0, 4, 2)
    got = hull_ptr(lab, labels, 2)
    assert got[0][0].tolist() == first and first[1] > 2 ** 32
    same(got, ref.hulls(labels, 2), shape)


def run_cases():
    planes, cls, min_area, classes = rings()
    bplanes, bcls, bmin = blobs()
    return (("plain", planes, dict(cls=cls, min_area=min_area)),
            ("grow", planes, dict(cls=cls, min_area=min_area, grow=3, grow_classes=classes)),
            ("split", bplanes, dict(cls=bcls, min_area=bmin, split=2)))


def test_labels_of_the_run_itself(lab):
    """Labeler.run then hull(), plain, grown and split: the restatement on the labels the run returned, the same from hull_ptr on a
    torch tensor, the same bytes from a second call; the object table, the shapes and the contacts are afterwards what they were"""
    umx.require_torch_runtime("test_gpu_label_hull")
    seen = 0
    for name, planes, kw in run_cases():
        labels, table = lab.run(planes, **kw)
        N = len(table)
        before = (lab.objects().tobytes(), lab.shape().tobytes(), lab.contacts().tobytes())
        got = lab.hull()
        same(got, ref.hulls(labels, N), name)
        assert np.array_equal(got[0]["rows"], table["y1"].astype(np.int64) - table["y0"] + 1), name     # 4-connected: no row of the box is empty
        assert (2 * table["area"].astype(np.int64) <= got[0]["area2"]).all(), name
        same(lab.hull(), got, name + ", twice")
        same(hull_ptr(lab, labels, N), got, name + ", on a device pointer")
        same(lab.hull(), got, name + ", after the device entry")     # it left the resident labels alone
        k, dl = lab.hull_last_ms()
        assert k > 0.0 and dl > 0.0
        assert (lab.objects().tobytes(), lab.shape().tobytes(), lab.contacts().tobytes()) == before, name
        d = umx.hull_descriptors(got[0], got[1], table["area"])
        assert (d["solidity"] <= 1.0).all() and (d["solidity"] > 0.0).all() and (d["feret_min"] <= d["feret_max"]).all(), name
        seen += N
    assert seen > 100


def refused(call, word, code=umx.ERR_INVALID):
    with pytest.raises(umx.UmxError) as e:
        call()
    assert e.value.code == code and word in str(e.value), str(e.value)


def test_refusals_leave_the_resident_labels():
    umx.require_torch_runtime("test_gpu_label_hull")
    import torch
    planes, cls, min_area, classes = rings()
    H, W = BLOBS
    with umx.Labeler() as lb:
        refused(lb.hull, "no labels")                                # before any run
        labels, table = lb.run(planes, cls, min_area)
        N = len(table)
        wanted = ref.hulls(labels, N)
        V = len(wanted[1])
        same(lb.hull(), wanted, "after a run")
        refused(lambda: lb.hull(W, H), "200 x 264")                  # another shape
        refused(lambda: lb.hull(0, W), "at least 1")
        refused(lambda: lb.hull(65537, W), "65536")
        n, v = umx.ctypes.c_int64(-1), umx.ctypes.c_int64(-1)
        call = lb._L.umx_labeler_hull
        assert call(lb._lb, H, W, None, 0, umx.ctypes.byref(n), None, 0, umx.ctypes.byref(v)) == 0 and (n.value, v.value) == (N, V)   # only N and V
        rec, verts = np.zeros(N, umx.LABEL_HULL_DTYPE), np.zeros(V, umx.LABEL_HULL_VERTEX_DTYPE)
        rc = call(lb._lb, H, W, rec.ctypes.data, N - 1, None, verts.ctypes.data, V, None)          # cap < N
        assert rc == umx.ERR_INVALID and "records" in lb._L.umx_labeler_last_error(lb._lb).decode()
        v.value = -1
        rc = call(lb._lb, H, W, rec.ctypes.data, N, None, verts.ctypes.data, V - 1, umx.ctypes.byref(v))   # vcap < V: V is stored
        assert rc == umx.ERR_INVALID and v.value == V and "vertices" in lb._L.umx_labeler_last_error(lb._lb).decode()
        assert not rec.view(np.uint8).any() and not verts.view(np.uint8).any()                   # nothing was touched
        assert call(lb._lb, H, W, rec.ctypes.data, N, None, verts.ctypes.data, V, None) == 0
        same((rec, verts), wanted, "the C entry with room for exactly N and V")
        d_labels = torch.from_numpy(np.array(labels)).cuda()
        torch.cuda.synchronize()
        rec[:] = 0
        rc = lb._L.umx_labeler_hull_dev(lb._lb, umx.ctypes.c_void_p(d_labels.data_ptr()), N, H, W, rec.ctypes.data, N - 1, verts.ctypes.data, V, None)
        assert rc == umx.ERR_INVALID and not rec.view(np.uint8).any()
        refused(lambda: lb.hull_ptr(d_labels.data_ptr(), -1, H, W), "n_objects")
        refused(lambda: lb.hull_ptr(0, N, H, W), "null")
        lb._hull_room = (1, 1)                                       # the binding's own retry: too little room for either list
        same(lb.hull(), wanted, "after refused hull calls, through the retry")
        # E past the limit: labels 1..16384 in the first and the last row of 16385 x 16384, nothing between -- every box is the plane's
        # height, E = 16385 * 16384 > 2^28.  The plane is 1 GiB, made on the device, with no host copy.
        big_h, big_w = 16385, 16384
        assert big_h * big_w > umx.HULL_MAX_ROWS and umx.label_hull_check(big_h, big_w, big_w) == ""
        d_big = torch.zeros((big_h, big_w), dtype=torch.int32, device="cuda")
        d_big[0] = torch.arange(1, big_w + 1, dtype=torch.int32, device="cuda")
        d_big[-1] = d_big[0]
        torch.cuda.synchronize()
        refused(lambda: lb.hull_ptr(d_big.data_ptr(), big_w, big_h, big_w), "UMX_HULL_MAX_ROWS", ERR_OOM)
        del d_big
        same(lb.hull(), wanted, "after the refusal of E")
        _, t2 = lb.run(planes, cls, min_area, want_labels=False)
        assert len(t2) == N
        refused(lb.hull, "no label plane")                           # a later run without a label plane
        labels2, table2 = lb.run(planes, cls, min_area, grow=2, grow_classes=classes)
        same(lb.hull(), ref.hulls(labels2, len(table2)), "usable after every refusal")
        px = np.ones((1,) + BLOBS, np.uint8)
        assert np.array_equal(lb.measure(px)["count"][0], table2["area"])   # the measurement and the hulls share the arena
        same(lb.hull(), ref.hulls(labels2, len(table2)), "after a measurement")


_GUARD_CHILD = """
import sys
sys.path.insert(0, %r); sys.path.insert(0, %r)
import numpy as np
import torch
import label_grow_ref as grow_ref
import label_hull_ref as ref
from unmicst_amd import umx
umx.require_torch_runtime("test_gpu_label_hull")
T, HALO = umx.LABEL_GROW_TILE, umx.LABEL_GROW_HALO
# every label present and every hull at its bound of 2 rows + 2 vertices (lenses, single pixels, a staircase of two): at a labeler's
# first hull call the records, the row entries and the scratch vertices are allocated at exactly N, 2 E and 2 (E + N), and all filled
full = np.zeros((40, 200), np.int32)
parts = [ref.lens(3), np.ones((1, 1), np.int32), ref.lens(6), ref.staircase(2), np.ones((1, 1), np.int32)]
x = 1
for j, m in enumerate(parts, start=1):
    full[2 + j:2 + j + m.shape[0], x:x + m.shape[1]][m > 0] = j
    x += m.shape[1] + 1
N = len(parts)
with umx.Labeler() as lb:
    d_full = torch.from_numpy(full).cuda()
    torch.cuda.synchronize()
    rec, verts = lb.hull_ptr(d_full.data_ptr(), N, full.shape[0], full.shape[1])   # (raises UmxError 7 when a red zone was written)
    want = ref.hulls(full, N)
    assert rec.tobytes() == want[0].tobytes() and verts.tobytes() == want[1].tobytes(), "filled"
    E = int(rec["rows"].sum())
    assert E == sum(m.shape[0] for m in parts) and len(verts) == 2 * (E + N), "every place of the scratch area is used"
shape = (2 * T + HALO - 3, 3 * T + 5)
planes, cls, min_area, classes = grow_ref.case(shape[0], shape[1], "rings", T, HALO)
with umx.Labeler() as lb:
    labels, table = lb.run(planes, cls, min_area, grow=3, grow_classes=classes)
    N = len(table)
    rec, verts = lb.hull()
    want = ref.hulls(labels, N)
    assert rec.tobytes() == want[0].tobytes() and verts.tobytes() == want[1].tobytes(), "host"
    bad = labels.copy()
    hit = np.random.default_rng(7).random(bad.shape)
    bad[hit < 0.03] = -5; bad[(hit >= 0.03) & (hit < 0.06)] = N + 1; bad[(hit >= 0.06) & (hit < 0.09)] = 2 ** 31 - 1
    d_labels = torch.from_numpy(bad).cuda()
    torch.cuda.synchronize()
    rec, verts = lb.hull_ptr(d_labels.data_ptr(), N, shape[0], shape[1])
    want = ref.hulls(bad, N)
    assert rec.tobytes() == want[0].tobytes() and verts.tobytes() == want[1].tobytes(), "device"
    again, _ = lb.run(planes, cls, min_area, grow=3, grow_classes=classes)
    assert np.array_equal(again, labels)
print("guard-ok")
"""


def test_guard_mode_finds_no_write_outside_the_buffers():
    """UMX_DEBUG_GUARD in a child process: red zones round every buffer of the hulls.  A plane on which the records, the row entries
    and the scratch vertices are exactly filled, then both entries on a ragged plane, labels outside 0..N included: all end with
    UMX_OK and the right lists."""
    env = dict(os.environ, UMX_DEBUG_GUARD="1")
    r = subprocess.run([sys.executable, "-c", _GUARD_CHILD % (ROOT, os.path.join(ROOT, "tests"))], env=env, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0 and "guard-ok" in r.stdout, r.stderr[-2000:]


def test_command_writes_the_hulls_and_changes_nothing_else(tmp_path):
    """UnMicst.py --stackOutput --labelMask --labelGrow 2 [--labelHull [--labelHullVertices]] on a 96 x 130 crop of sample 105: the
    Hulls file's integer columns and repr floats are hull_descriptors of the restatement on the Labels page the same run wrote, the
    HullVertices file its vertex list; every other file has the bytes of the run without the flags, which writes neither; without
    --labelMask the flags are the parser's error."""
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
    hull, r = command("hull", ["--labelMask", "--labelGrow", "2", "--labelHull"])
    assert r.returncode == 0, r.stderr[-2000:]
    out, r = command("vertices", ["--labelMask", "--labelGrow", "2", "--labelHull", "--labelHullVertices"])
    assert r.returncode == 0, r.stderr[-2000:]
    assert "crop_Labels_1.tif" in files(plain) and not [f for f in files(plain) if "Hull" in f]
    assert files(hull) == sorted(files(plain) + ["crop_Hulls_1.csv"])
    assert files(out) == sorted(files(plain) + ["crop_Hulls_1.csv", "crop_HullVertices_1.csv"])
    for f in files(plain):
        assert open(os.path.join(plain, f), "rb").read() == open(os.path.join(hull, f), "rb").read() == open(os.path.join(out, f), "rb").read(), f
    assert open(os.path.join(hull, "crop_Hulls_1.csv"), "rb").read() == open(os.path.join(out, "crop_Hulls_1.csv"), "rb").read()
    labels = tiffio.imread_all(os.path.join(out, "crop_Labels_1.tif"))[0]
    table = [[int(v) for v in line.split(",")[:6]] for line in open(os.path.join(out, "crop_Objects_1.csv")).read().splitlines()[1:]]
    N = len(table)
    assert N > 1 and labels.max() == N
    rec, verts = ref.hulls(labels, N)
    area = np.array([t[1] for t in table])
    assert np.array_equal(area, np.bincount(labels.ravel(), minlength=N + 1)[1:])
    d = umx.hull_descriptors(rec, verts, area)
    lines = open(os.path.join(out, "crop_Hulls_1.csv")).read().splitlines()
    assert lines[0] == ",".join(driver.HULL_COLUMNS) and len(lines) == N + 1
    for j, line in enumerate(lines[1:]):
        f = line.split(",")
        assert [int(f[0]), int(f[6])] == [j + 1, rec["n_vertices"][j]], j
        want_floats = [d[n][j] for n in driver.HULL_COLUMNS[1:6]]
        assert f[1:6] == [repr(float(v)) for v in want_floats], j
        assert [float(v) for v in f[1:6]] == [float(v) for v in want_floats], j
        assert float(f[1]) == rec["area2"][j] / 2 and float(f[2]) == area[j] / (rec["area2"][j] / 2) <= 1.0, j
    lines = open(os.path.join(out, "crop_HullVertices_1.csv")).read().splitlines()
    assert lines[0] == ",".join(driver.HULL_VERTEX_COLUMNS) and len(lines) == len(verts) + 1
    want_rows = [(j + 1, i, int(verts["y"][rec["first"][j] + i]), int(verts["x"][rec["first"][j] + i]))
                 for j in range(N) for i in range(rec["n_vertices"][j])]
    assert [tuple(int(v) for v in line.split(",")) for line in lines[1:]] == want_rows
    for flags, word in ((["--labelHull"], "--labelHull needs --labelMask"), (["--labelMask", "--labelHullVertices"], "--labelHullVertices needs --labelHull")):
        bad, r = command("refused", flags)
        assert r.returncode == 2 and word in r.stderr, r.stderr[-2000:]
        assert not os.path.exists(bad) or not [f for f in files(bad) if "Hull" in f]
