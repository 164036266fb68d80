"""GPU tests of the label mask's relabel (unmicst_amd/csrc/umx_label_relabel.hip; include/umx.h and DESIGN.md section 8.1, steps 29 to
32): the plane, the object table and the map of umx_labeler_relabel / _relabel_dev against tests/label_relabel_ref.py, and the tables
of the later calls against their own restatements on the restated plane.  Everything is an integer and compared for equality: there is
no tolerance anywhere in this file."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import helpers
import label_contact_ref
import label_grow_ref as grow_ref
import label_hull_ref
import label_measure_ref
import label_ref
import label_relabel_ref as ref
import label_shape_ref
from unmicst_amd import driver, model, tiffio, umx

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

T, HALO = umx.LABEL_GROW_TILE, umx.LABEL_GROW_HALO
BLOBS = (120, 200)                             # 30 workgroups of 4 row waves, 4 chunks a row, the last 8 pixels
WIDTHS, HEIGHTS = (1, 63, 64, 65, 130), (1, 3, 4, 5)
LATTICE = (2047, 2048, 2049, 4097)


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
def pixels():
    px = label_measure_ref.pixels(BLOBS, np.uint16, 2, seed=3)
    px.setflags(write=False)
    return px


def same_table(got, want, what):
    assert got.dtype == umx.LABEL_OBJECT_DTYPE and got.shape == want.shape, (what, got.shape, want.shape)
    for f in umx.LABEL_OBJECT_DTYPE.names:
        assert np.array_equal(got[f], want[f]), (what, f, got[f][:8], want[f][:8])


def same(got, want, what):
    """(labels, objects, map) of Labeler.relabel against the restatement's"""
    assert got[0].dtype == np.int32 and np.array_equal(got[0], want[0]), what
    same_table(got[1], want[1], what)
    assert got[2].dtype == np.int32 and np.array_equal(got[2], want[2]), (what, got[2][:10], want[2][:10])


def relabel_ptr(lab, labels, N, keep=None, pairs=None, in_place=True):
    """the device entry on a copy of `labels` -> (labels', map, N'); out of place the input must be as it was"""
    import torch
    d_in = torch.from_numpy(np.array(labels, np.int32)).cuda()
    d_out = d_in if in_place else torch.full(labels.shape, -77, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    m, n_new = lab.relabel_ptr(d_in.data_ptr(), N, labels.shape[0], labels.shape[1], keep, pairs, None if in_place else d_out.data_ptr())
    if not in_place:
        assert np.array_equal(d_in.cpu().numpy(), labels)            # only read
    return d_out.cpu().numpy(), m, n_new


@pytest.mark.parametrize("H", HEIGHTS)
def test_chunk_and_row_group_boundaries(lab, H):
    """W round the 64-pixel chunk, H round the 4 rows of a workgroup; runs that end on, before and after a chunk's end, one run through
    every chunk of a 130-pixel row, values -5 and N + 3 in the caller's plane; in place and out of place"""
    umx.require_torch_runtime("test_gpu_label_relabel")
    for W in WIDTHS:
        labels, N = ref.geometry(H, W)
        if W >= 130:
            assert (labels[H // 2, 1:W - 1] == labels[H // 2, 1]).all() and W - 2 >= 128         # the run that spans three chunks
        keep = ref.keeps(N, seed=H * 1000 + W)["seeded"]
        pairs = ref.seeded_pairs(N, max(1, N // 4), seed=W, among=np.flatnonzero(keep) + 1)
        for k, p in ((None, None), (keep, None), (keep, pairs), (None, ref.chain(N))):
            want, _, want_map = ref.relabel(labels, N, k, p)
            for in_place in (True, False):
                got, m, n_new = relabel_ptr(lab, labels, N, k, p, in_place)
                assert np.array_equal(m, want_map) and n_new == want_map.max(initial=0), (H, W, in_place)
                assert np.array_equal(got, want), (H, W, in_place, got, want)
        if W >= 3:
            assert labels[H - 1, W - 1] == -5 and labels[0, 0] == N + 3 and want[H - 1, W - 1] == 0 and want[0, 0] == 0


@pytest.mark.parametrize("N", LATTICE)
def test_numbering_across_the_blocks_of_2048_labels(N):
    """single pixels on the even coordinates of 130 x 130, the first N of them: the run numbers them in raster order, the relabel drops
    every third one and merges seeded pairs of the rest"""
    lattice = ref.lattice(N)
    with umx.Labeler() as lb:
        labels, table = lb.run(label_ref.planes_of(lattice > 0))
        assert len(table) == N and np.array_equal(labels, lattice)
        keep = np.arange(N) % 3 != 1
        pairs = ref.seeded_pairs(N, N // 5, seed=N, among=np.flatnonzero(keep) + 1)
        want = ref.relabel(lattice, N, keep, pairs)
        got = lb.relabel(keep, pairs)
        same(got, want, N)
        assert got[2].max() == len(got[1]) < N - N // 3 and np.array_equal(lb.objects(), got[1])
        up, k, dl = lb.relabel_last_ms()
        assert up > 0.0 and k > 0.0 and dl > 0.0
        ident = lb.relabel()                                         # then the identity on what is left
        same(ident, (want[0], want[1], np.arange(len(want[1]) + 1, dtype=np.int32)), (N, "identity"))


def tables_after(lb, labels, N, what):
    """every later call of the labeler against its own restatement on the (restated) plane"""
    same_table(lb.objects(), ref.table_of(labels, N), what)
    px = pixels()
    got = lb.measure(px)
    want = label_measure_ref.measure(labels, px, N)
    assert got.shape == want.shape and all(np.array_equal(got[f], want[f]) for f in want.dtype.names), (what, "measure")
    got = lb.shape()
    want = label_shape_ref.records(labels, N)
    assert got.shape == want.shape and all(np.array_equal(got[f], want[f]) for f in want.dtype.names), (what, "shape")
    got = lb.contacts()
    assert got.tobytes() == label_contact_ref.contacts(labels, N).tobytes(), (what, "contacts")
    rec, verts = lb.hull()
    want = label_hull_ref.hulls(labels, N)
    assert rec.tobytes() == want[0].tobytes() and verts.tobytes() == want[1].tobytes(), (what, "hull")


def test_keep_variations(lab):
    """keep none (an empty plane and empty tables from every later call), keep all (the identity, byte for byte), alternating, seeded"""
    planes, cls, min_area = blobs()
    labels, table = lab.run(planes, cls, min_area)
    N = len(table)
    assert N > 20
    got = lab.relabel(np.ones(N, np.uint8))
    assert got[0].tobytes() == labels.tobytes() and got[1].tobytes() == table.tobytes() and got[2].tobytes() == np.arange(N + 1, dtype=np.int32).tobytes()
    got = lab.relabel()
    assert got[0].tobytes() == labels.tobytes() and got[1].tobytes() == table.tobytes() and lab.objects().tobytes() == table.tobytes()
    for name in ("alternating", "seeded", "first only", "last only"):
        lab.run(planes, cls, min_area)
        keep = ref.keeps(N, seed=4)[name]
        got = lab.relabel(keep)
        same(got, ref.relabel(labels, N, keep), name)
        assert len(got[1]) == int(keep.sum())
    tables_after(lab, got[0], 1, "last only")
    lab.run(planes, cls, min_area)
    got = lab.relabel(np.zeros(N, np.uint8))
    assert not got[0].any() and len(got[1]) == 0 and not got[2].any() and len(lab.objects()) == 0
    assert lab.shape().shape == (0,) and lab.measure(pixels()).shape == (2, 0) and lab.contacts().shape == (0,)
    rec, verts = lab.hull()
    assert rec.shape == (0,) and verts.shape == (0,)
    assert len(lab.relabel()[1]) == 0                                # and a relabel of no object


def test_pair_variations(lab):
    """the chain (one object remains), a star, shuffled and doubled pairs (the same bytes), pairs of objects that do not touch"""
    planes, cls, min_area = blobs()
    labels, table = lab.run(planes, cls, min_area)
    N = len(table)
    assert len(lab.contacts()) == 0                                  # a plain run: no two objects touch, every pair is a far one
    far = np.array([[1, N], [2, N - 1], [N, 3]])
    seeded = ref.seeded_pairs(N, N // 2, seed=9)
    rng = np.random.default_rng(1)
    shuffled = np.concatenate([seeded, seeded[:, ::-1]])[rng.permutation(2 * len(seeded))]
    first = None
    for name, pairs in (("chain", ref.chain(N)), ("star", ref.star(N, N // 2)), ("far", far), ("seeded", seeded), ("shuffled", shuffled)):
        lab.run(planes, cls, min_area)
        got = lab.relabel(pairs=pairs)
        same(got, ref.relabel(labels, N, None, pairs), name)
        if name in ("chain", "star"):
            assert len(got[1]) == 1 and got[1]["area"][0] == table["area"].sum() and set(np.unique(got[0])) == {0, 1}
        if name == "far":
            assert len(got[1]) == N - 3
        if name == "seeded":
            first = got
        if name == "shuffled":
            assert all(a.tobytes() == b.tobytes() for a, b in zip(got, first))
    tables_after(lab, got[0], len(got[1]), "merged, disconnected objects")


def run_cases():
    planes, cls, min_area, classes = rings()
    bplanes, bcls, bmin = blobs()
    return (("grow", planes, dict(cls=cls, min_area=min_area, grow=3, grow_classes=classes)),
            ("split", bplanes, dict(cls=bcls, min_area=bmin, split=2)))


def test_later_tables_see_the_new_labels(lab):
    """after a relabel on the labels of a grown run and of a split run -- objects that touch are merged by their contacts, a seeded
    half of the rest dropped -- objects(), measure(), shape(), contacts() and hull() are the restatements on the restated plane; two
    calls equal one; two identical calls give identical bytes; the counts of the split stay"""
    seen = 0
    for name, planes, kw in run_cases():
        labels, table = lab.run(planes, **kw)
        N = len(table)
        counts = lab.split_counts()
        touching = lab.contacts()
        pairs = np.stack([touching["a"], touching["b"]], 1)[::2]
        l1, t1, m1 = lab.relabel(pairs=pairs)
        same((l1, t1, m1), ref.relabel(labels, N, None, pairs), name + ", merged")
        N1 = len(t1)
        tables_after(lab, l1, N1, name + ", merged")
        keep = ref.keeps(N1, seed=6)["seeded"]
        l2, t2, m2 = lab.relabel(keep)
        same((l2, t2, m2), ref.relabel(l1, N1, keep), name + ", then dropped")
        tables_after(lab, l2, len(t2), name + ", then dropped")
        assert lab.split_counts() == counts
        # the two calls as one: the pairs of the first with the second's keep taken back through its map
        keep0 = np.concatenate([[False], keep])[m1[1:]]
        lab.run(planes, **kw)
        once = lab.relabel(keep0, pairs[keep0[pairs[:, 0] - 1]] if len(pairs) else pairs)
        assert np.array_equal(once[0], l2) and once[1].tobytes() == t2.tobytes() and np.array_equal(once[2], m2[m1]), name
        lab.run(planes, **kw)
        again = lab.relabel(keep0, pairs[keep0[pairs[:, 0] - 1]] if len(pairs) else pairs)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(once, again)), name
        seen += len(pairs)
    assert seen > 0                                                  # something was merged


def test_device_entry_and_the_callers_table(lab):
    """in place and out of place on a caller's plane with values outside 0..N; relabel_objects on the caller's table is step 4 on the
    new plane; the resident labels are left alone"""
    umx.require_torch_runtime("test_gpu_label_relabel")
    planes, cls, min_area, classes = rings()
    labels, table = lab.run(planes, cls, min_area, grow=2, grow_classes=classes)
    N = len(table)
    before = (lab.objects().tobytes(), lab.shape().tobytes())
    bad = labels.copy()
    hit = np.random.default_rng(7).random(bad.shape)
    bad[hit < 0.03] = -5
    bad[(hit >= 0.03) & (hit < 0.06)] = N + 3
    bad[(hit >= 0.06) & (hit < 0.08)] = 2 ** 31 - 1
    keep = ref.keeps(N, seed=8)["seeded"]
    pairs = ref.seeded_pairs(N, N // 4, seed=2, among=np.flatnonzero(keep) + 1)
    want, want_table, want_map = ref.relabel(bad, N, keep, pairs)
    assert not want[(bad < 0) | (bad > N)].any()
    for in_place in (True, False):
        got, m, n_new = relabel_ptr(lab, bad, N, keep, pairs, in_place)
        assert np.array_equal(got, want) and np.array_equal(m, want_map) and n_new == len(want_table), in_place
    same_table(umx.relabel_objects(ref.table_of(ref.clean(bad, N), N), m), want_table, "the caller's table")
    got, m, n_new = relabel_ptr(lab, bad, 0)                          # N = 0: every value counts as 0
    assert not got.any() and m.tolist() == [0] and n_new == 0
    assert (lab.objects().tobytes(), lab.shape().tobytes()) == before


def refused(call, *words):
    with pytest.raises(umx.UmxError) as e:
        call()
    assert e.value.code == umx.ERR_INVALID and all(w in str(e.value) for w in words), str(e.value)


def test_refusals_leave_the_resident_labels():
    umx.require_torch_runtime("test_gpu_label_relabel")
    import torch
    planes, cls, min_area, classes = rings()
    H, W = BLOBS
    with umx.Labeler() as lb:
        refused(lambda: lb.relabel(H=H, W=W), "no labels")           # before any run
        lb.run(planes, cls, min_area, want_labels=False)
        refused(lambda: lb.relabel(H=H, W=W), "no label plane")      # a run without a label plane
        labels, table = lb.run(planes, cls, min_area, grow=2, grow_classes=classes)
        N = len(table)
        shapes = lb.shape().tobytes()
        keep = np.ones(N, np.uint8)
        keep[4] = 0
        for call, words in ((lambda: lb.relabel(H=W, W=H), ("%d x %d" % (H, W),)),
                            (lambda: lb.relabel(H=0, W=W), ("at least 1",)),
                            (lambda: lb.relabel(keep[:-1]), ("n_keep is %d" % (N - 1),)),
                            (lambda: lb.relabel(np.ones(N + 1, np.uint8)), ("n_keep is %d" % (N + 1),)),
                            (lambda: lb.relabel(pairs=[[1, 2], [1, N + 1]]), ("pair 1 is (1, %d)" % (N + 1),)),
                            (lambda: lb.relabel(pairs=[[0, 2]]), ("pair 0 is (0, 2)",)),
                            (lambda: lb.relabel(keep, [[1, 2], [2, 3], [3, 5]]), ("pair 2 is (3, 5)", "keep drops label 5"))):
            refused(call, *words)
            assert lb.shape().tobytes() == shapes and lb.objects().tobytes() == table.tobytes()      # as they were
        n = umx.ctypes.c_int64(-1)
        rc = lb._L.umx_labeler_relabel(lb._lb, H, W, None, 3, None, 0, None, None, umx.ctypes.byref(n))   # keep null with a count
        assert rc == umx.ERR_INVALID and n.value == -1 and "n_keep is 3" in lb._L.umx_labeler_last_error(lb._lb).decode()
        d_labels = torch.from_numpy(np.array(labels)).cuda()
        torch.cuda.synchronize()
        refused(lambda: lb.relabel_ptr(d_labels.data_ptr(), -1, H, W), "n_objects")
        refused(lambda: lb.relabel_ptr(0, N, H, W), "null")
        refused(lambda: lb.relabel_ptr(d_labels.data_ptr(), N, H, W, pairs=[[1, N + 1]]), "pair 0")
        assert np.array_equal(d_labels.cpu().numpy(), labels)
        assert lb.shape().tobytes() == shapes
        got = lb.relabel(keep, want_labels=False)                    # usable after every refusal
        assert got[0] is None
        same_table(got[1], ref.relabel(labels, N, keep)[1], "after the refusals")
        assert len(lb.shape()) == N - 1


_GUARD_CHILD = """
import sys
sys.path.insert(0, %r); sys.path.insert(0, %r)
import numpy as np
import torch
import label_grow_ref as grow_ref
import label_relabel_ref as ref
from unmicst_amd import umx
umx.require_torch_runtime("test_gpu_label_relabel")
T, HALO = umx.LABEL_GROW_TILE, umx.LABEL_GROW_HALO
shape = (2 * T + HALO - 3, 3 * T + 5)
planes, cls, min_area, classes = grow_ref.case(shape[0], shape[1], "rings", T, HALO)
with umx.Labeler() as lb:
    labels, table = lb.run(planes, cls, min_area, grow=3, grow_classes=classes)
    N = len(table)
    keep = ref.keeps(N, seed=1)["seeded"]
    got = lb.relabel(keep)                                 # (raises UmxError 7 when a red zone was written)
    want = ref.relabel(labels, N, keep)
    assert all(np.array_equal(a, b) for a, b in zip(got, want)), "resident"
    got = lb.relabel()                                     # the tables have changed places: once more, and back
    assert np.array_equal(got[0], want[0]) and got[1].tobytes() == want[1].tobytes(), "identity"
    # a map larger than any buffer the run made: 4 * (big + 1) bytes against two planes of 4 * H * W; only its first words are read
    big = 4 * shape[0] * shape[1]
    bad = want[0].copy()
    hit = np.random.default_rng(7).random(bad.shape)
    bad[hit < 0.03] = -5; bad[(hit >= 0.03) & (hit < 0.06)] = big + 1; bad[(hit >= 0.06) & (hit < 0.07)] = big
    d_labels = torch.from_numpy(bad).cuda()
    torch.cuda.synchronize()
    keep = np.arange(big) %% 2 == 0
    m, n_new = lb.relabel_ptr(d_labels.data_ptr(), big, shape[0], shape[1], keep, [[1, big - 1]])
    want2, _, want_map = ref.relabel(bad, big, keep, [[1, big - 1]])
    assert np.array_equal(m, want_map) and np.array_equal(d_labels.cpu().numpy(), want2), "device"
    again, table2 = lb.run(planes, cls, min_area, grow=3, grow_classes=classes)
    assert np.array_equal(again, labels) and table2.tobytes() == table.tobytes()
    got = lb.relabel(pairs=ref.chain(N))
    assert len(got[1]) == 1 and got[1]["area"][0] == table["area"].sum(), "after a second run"
print("guard-ok")
"""


def test_guard_mode_finds_no_write_outside_the_buffers():
    """UMX_DEBUG_GUARD in a child process: red zones round the map, both tables and the planes.  Both entries, the tables changing
    places twice, a map upload larger than any buffer the run made, labels outside 0..N, a run afterwards: all end with UMX_OK and
    the right planes."""
    env = dict(os.environ, UMX_DEBUG_GUARD="1")
    r = subprocess.run([sys.executable, "-c", _GUARD_CHILD % (ROOT, os.path.join(ROOT, "tests"))], env=env, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0 and "guard-ok" in r.stdout, r.stderr[-2000:]


def test_command_merges_drops_and_writes_consistent_files(tmp_path):
    """UnMicst.py --stackOutput --labelMask --labelGrow 2 --labelShape --labelMeasure on a 96 x 130 crop of sample 105, without and with
    --labelKeep area>=30 border==0 --labelMerge 0.5: the second run's Labels, Objects, Shapes and Intensities are the restatement --
    merge by the contacts and perimeter edges of the first run's labels, then the two rules on the merged table -- applied to the first
    run's files, and agree with one another; the first run prints no relabel line and its Shapes file is the writer's on its labels."""
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
    base = ["--labelMask", "--labelGrow", "2", "--labelShape", "--labelMeasure"]

    def command(sub, flags):
        out = str(tmp_path / sub)
        r = subprocess.run([sys.executable, os.path.join(ROOT, "UnMicst.py"), img, "--model", "nucleiDAPI", "--stackOutput", "--outputPath",
                            out] + flags, env=env, capture_output=True, text=True, timeout=600)
        return out, r

    def files(d):
        return sorted(os.path.relpath(os.path.join(r, f), d) for r, _, fs in os.walk(d) for f in fs)

    def read(d):
        labels = tiffio.imread_all(os.path.join(d, "crop_Labels_1.tif"))[0]
        objects = [[int(v) for v in line.split(",")[:6]] for line in open(os.path.join(d, "crop_Objects_1.csv")).read().splitlines()[1:]]
        return labels, np.array(objects, np.int64).reshape(-1, 6)

    plain, r = command("plain", base)
    assert r.returncode == 0 and "Label relabel" not in r.stdout, r.stderr[-2000:]
    out, r = command("relabel", base + ["--labelKeep", "area>=30", "border==0", "--labelMerge", "0.5"])
    assert r.returncode == 0, r.stderr[-2000:]
    assert files(out) == files(plain) and "crop_Shapes_1.csv" in files(out) and "crop_Intensities_1.csv" in files(out)
    for f in files(plain):
        if not any(w in f for w in ("Labels", "Objects", "Shapes", "Intensities")):
            assert open(os.path.join(plain, f), "rb").read() == open(os.path.join(out, f), "rb").read(), f
    labels0, objects0 = read(plain)
    N0 = len(objects0)
    assert N0 > 3 and labels0.max() == N0
    table0 = ref.table_of(labels0, N0)
    driver.write_shapes_csv(str(tmp_path / "shapes0.csv"), table0, label_shape_ref.records(labels0, N0))
    assert open(tmp_path / "shapes0.csv").read() == open(os.path.join(plain, "crop_Shapes_1.csv")).read()
    # the restatement: merge, then keep
    perimeter_edges = umx.shape_descriptors(label_shape_ref.records(labels0, N0))["perimeter_edges"]
    pairs = driver.merge_pairs(label_contact_ref.contacts(labels0, N0), perimeter_edges, 0.5)
    labels1, table1, _ = ref.relabel(labels0, N0, None, pairs)
    H, W = labels0.shape
    keep = (table1["area"] >= 30) & (table1["y0"] > 0) & (table1["x0"] > 0) & (table1["y1"] < H - 1) & (table1["x1"] < W - 1)
    labels2, table2, _ = ref.relabel(labels1, len(table1), keep)
    N2 = len(table2)
    merged, dropped = N0 - len(table1), len(table1) - N2
    print("command: %d objects, %d merged away, %d dropped, %d left" % (N0, merged, dropped, N2))
    assert 0 < N2 < N0 and dropped > 0
    assert "Label relabel: %d objects from %d (%d dropped, %d merged away)" % (N2, N0, dropped, merged) in r.stdout
    labels, objects = read(out)
    assert np.array_equal(labels, labels2) and labels.dtype == np.int32
    assert np.array_equal(objects, np.stack([np.arange(1, N2 + 1)] + [table2[f] for f in ("area", "y0", "x0", "y1", "x1")], 1))
    driver.write_objects_csv(str(tmp_path / "objects2.csv"), table2)
    assert open(tmp_path / "objects2.csv").read() == open(os.path.join(out, "crop_Objects_1.csv")).read()
    driver.write_shapes_csv(str(tmp_path / "shapes2.csv"), table2, label_shape_ref.records(labels2, N2))
    assert open(tmp_path / "shapes2.csv").read() == open(os.path.join(out, "crop_Shapes_1.csv")).read()
    pm = np.ascontiguousarray(tiffio.imread_all(os.path.join(out, "crop_Probabilities_1.tif"))[::-1])   # pages: reversed class order
    measured = [("pm%d" % k, label_measure_ref.measure(labels2, pm[k], N2)[0]) for k in range(len(pm))]
    measured += [("ch0", label_measure_ref.measure(labels2, raw, N2)[0])]
    assert open(os.path.join(out, "crop_Intensities_1.csv")).read().splitlines() == label_measure_ref.csv_lines(table2["area"].tolist(), measured)
    for flags, word in ((["--labelKeep", "area>=30"], "--labelKeep needs --labelMask"), (["--labelMask", "--labelKeep", "volume>1"], "'volume'"),
                        (["--labelMask", "--labelMerge", "2"], "--labelMerge 2.0")):
        bad, r = command("refused", flags)
        assert r.returncode == 2 and word in r.stderr, r.stderr[-2000:]
        assert not os.path.exists(bad) or not files(bad)
