"""GPU tests of the label mask's contacts (unmicst_amd/csrc/umx_label_contact.hip; include/umx.h and DESIGN.md section 8.1, steps 22 to
24): the lists of umx_labeler_contacts / _contacts_dev against tests/label_contact_ref.py, compared for equality.  Everything is an
integer: there is no tolerance anywhere in this file.  The list is ordered on the device when no label has more than
UMX_CONTACT_DEVICE_SORT_MAX contacts and on the host otherwise; contacts_stats() says which, and the hub test holds both to the same
restatement."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import helpers
import label_contact_ref as ref
import label_grow_ref as grow_ref
import label_ref
from unmicst_amd import driver, model, tiffio, umx

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

T, HALO = umx.LABEL_GROW_TILE, umx.LABEL_GROW_HALO
BLOBS = (200, 264)                             # 50 workgroups of 4 row waves, 5 chunks a row; 4 x 5 growth tiles
WIDTHS, HEIGHTS = (1, 63, 64, 65, 129, 200), (1, 2, 3, 4, 5, 9)


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
    """the mosaic of a size and its restatement, computed once"""
    labels, N = ref.mosaic(H, W)
    rec = ref.contacts(labels, N)
    labels.setflags(write=False)
    rec.setflags(write=False)
    return labels, N, rec


def same(got, wanted, what):
    assert got.dtype == umx.LABEL_CONTACT_DTYPE and got.shape == wanted.shape, (what, got.shape, wanted.shape)
    assert got.tobytes() == wanted.tobytes(), (what, ref.as_tuples(got)[:6], ref.as_tuples(wanted)[:6])


def contacts_ptr(lab, labels, N, reach=0):
    import torch
    d_labels = torch.from_numpy(np.array(labels, np.int32)).cuda()   # (a copy: the shared inputs are read-only)
    torch.cuda.synchronize()
    got = lab.contacts_ptr(d_labels.data_ptr(), N, labels.shape[0], labels.shape[1], reach)
    assert np.array_equal(d_labels.cpu().numpy(), labels)            # only read
    return got


@pytest.mark.parametrize("H", HEIGHTS)
def test_chunk_and_row_group_boundaries(lab, H):
    """W round the 64-pixel chunk and its multiples, H round the 4 rows of a workgroup; long shared borders, one of them past two
    chunk ends, rows of one-pixel labels, values outside 1..N"""
    umx.require_torch_runtime("test_gpu_label_contacts")
    for W in WIDTHS:
        labels, N, rec = want(H, W)
        same(contacts_ptr(lab, labels, N), rec, (H, W))
        assert lab.contacts_stats()["ordered_by"] == ("device" if len(rec) else "none")
    if H > 1:
        labels, N, rec = want(H, 200)
        assert ref.has_long_border(labels) and ref.LONG > 128 and (1, 2) in [t[:2] for t in ref.as_tuples(rec)]   # the long border is there
    if H >= 4:
        assert len(want(H, 200)[2]) > 150                            # the one-pixel labels' pairs


def test_hand_made_planes(lab):
    """an edge, a corner (no contact), a checkerboard, a label in pieces, a label enclosed in another, values outside 1..N, N = 0, a
    plane of one label"""
    umx.require_torch_runtime("test_gpu_label_contacts")
    for name, labels, N, known in ref.hand_made():
        got = contacts_ptr(lab, labels, N)
        same(got, ref.contacts(labels, N), name)
        assert ref.as_tuples(got) == known, name
        if name == "checkerboard":
            H, W = labels.shape
            assert len(got) == 1 and int(got["edges"][0]) == H * (W - 1) + W * (H - 1)


def test_table_growth(lab):
    """256 x 256, every pixel its own label: 2 * 255 * 256 = 130 560 contacts in a first table of 65 536 entries (N = 65 536 is not
    above UMX_CONTACT_TABLE_MIN), so the pass overflows and runs again with the table doubled; a small plane afterwards is right with
    the grown table kept"""
    umx.require_torch_runtime("test_gpu_label_contacts")
    n = 256
    labels = np.arange(1, n * n + 1, dtype=np.int32).reshape(n, n)
    with umx.Labeler() as lb:                                        # a labeler of its own: its table starts at the least size
        got = contacts_ptr(lb, labels, n * n)
        st = lb.contacts_stats()
        assert len(got) == 2 * n * (n - 1) > umx.CONTACT_TABLE_MIN
        same(got, ref.contacts(labels, n * n), "every pixel a label")
        assert st["reruns"] >= 1 and st["table_capacity"] >= 2 * umx.CONTACT_TABLE_MIN and st["longest_row"] == 2, st
        assert st["ordered_by"] == "device"
        again = contacts_ptr(lb, labels, n * n)
        assert again.tobytes() == got.tobytes() and lb.contacts_stats()["reruns"] == 0   # the table is kept
        small, N, rec = want(5, 65)
        same(contacts_ptr(lb, small, N), rec, "a small plane in the grown table")
        assert lb.contacts_stats()["table_capacity"] == st["table_capacity"]


def hub(n):
    """2 x 2 n: row 0 all label 1, row 1 one-pixel labels 2 .. n + 1 at every second column -- n contacts (1, b)"""
    labels = np.zeros((2, 2 * n), np.int32)
    labels[0] = 1
    labels[1, ::2] = np.arange(2, n + 2)
    return labels, n + 1


def test_hub(lab):
    """label 1 touches 10 001 others: its row is longer than UMX_CONTACT_DEVICE_SORT_MAX and the host orders the list; with exactly
    UMX_CONTACT_DEVICE_SORT_MAX others the device does"""
    umx.require_torch_runtime("test_gpu_label_contacts")
    labels, N = hub(10001)
    assert labels.shape == (2, 20002)
    got = contacts_ptr(lab, labels, N)
    same(got, ref.contacts(labels, N), "hub")
    st = lab.contacts_stats()
    assert len(got) == 10001 > umx.CONTACT_DEVICE_SORT_MAX and st["longest_row"] == 10001 and st["ordered_by"] == "host", st
    labels, N = hub(umx.CONTACT_DEVICE_SORT_MAX)
    got = contacts_ptr(lab, labels, N)
    same(got, ref.contacts(labels, N), "under the cap")
    st = lab.contacts_stats()
    assert st["longest_row"] == umx.CONTACT_DEVICE_SORT_MAX and st["ordered_by"] == "device", st
    mixed = np.zeros((6, 2 * 1100), np.int32)                        # the hub and, below it, short rows: still the same bytes
    mixed[:2], n = hub(1100)
    mixed[3, :] = 2000 + np.arange(2200) // 5
    mixed[4, :] = 3000 + np.arange(2200) // 7
    got = contacts_ptr(lab, mixed, 4000)
    same(got, ref.contacts(mixed, 4000), "hub and short rows")
    assert lab.contacts_stats()["ordered_by"] == "host"


def run_cases():
    planes, cls, min_area, classes = rings()
    bplanes, bcls, bmin = blobs()
    return (("plain", planes, dict(cls=cls, min_area=min_area)),
            ("grow", planes, dict(cls=cls, min_area=min_area, grow=3, grow_classes=classes)),
            ("split", bplanes, dict(cls=bcls, min_area=bmin, split=2)),
            ("flood", bplanes, dict(cls=bcls, min_area=bmin, split=2, flood=bcls, flood_step=16, flood_invert=True)))


def test_labels_of_the_run_itself(lab):
    """Labeler.run then contacts(): nothing after a plain run (4-connected components of one class never touch); after a growth, a
    split and a flood the restatement on the labels the run returned, which is not empty: the cut lines.  shape() and measure()
    give afterwards what they gave before."""
    for name, planes, kw in run_cases():
        labels, table = lab.run(planes, **kw)
        N = len(table)
        shape_before, measure_before = lab.shape(), lab.measure(planes)
        got = lab.contacts()
        same(got, ref.contacts(labels, N), name)
        assert (len(got) == 0) == (name == "plain"), (name, len(got))
        assert lab.contacts().tobytes() == got.tobytes()             # twice: the same bytes
        k, dl = lab.contacts_last_ms()
        assert k > 0.0 and dl >= 0.0
        assert lab.shape().tobytes() == shape_before.tobytes() and lab.measure(planes).tobytes() == measure_before.tobytes(), name
        degree, shared = umx.contact_degrees(got, N)
        assert degree.sum() == 2 * len(got) and (shared <= umx.shape_descriptors(shape_before)["perimeter_edges"]).all(), name


@pytest.mark.parametrize("R", (1, 8, 9, 17))
def test_reach(lab, R):
    """the blobs labels grown 1, 8, 9 and 17 levels on a scratch plane -- one, one, two and three growth launches, fronts across the
    64-pixel tile seams: the restatement, and the resident labels as they were"""
    planes, cls, min_area = blobs()
    labels, table = lab.run(planes, cls, min_area)
    N = len(table)
    shape_before = lab.shape()
    assert len(lab.contacts()) == 0
    got = lab.contacts(reach=R)
    wanted = ref.contacts(labels, N, R)
    same(got, wanted, R)
    assert len(got) > 0
    assert lab.shape().tobytes() == shape_before.tobytes()           # the resident labels: every moment and window count as before
    same(lab.contacts(reach=0), ref.contacts(labels, N), "R = 0")
    assert lab.contacts(reach=0).tobytes() == lab.contacts().tobytes()


def test_reach_on_a_device_pointer_needs_no_run():
    """_contacts_dev with a reach on a labeler that never ran: the scratch planes are the contacts' own; values outside 1..N are
    domain like any 0"""
    umx.require_torch_runtime("test_gpu_label_contacts")
    planes, cls, min_area = blobs()
    labels = label_ref.label(planes, cls, min_area)[0].astype(np.int32)
    N = int(labels.max())
    hit = np.random.default_rng(3).random(labels.shape)
    labels[(labels == 0) & (hit < 0.02)] = -7
    labels[(labels == 0) & (hit > 0.98)] = N + 5
    with umx.Labeler() as lb:
        for R in (9, 3):
            same(contacts_ptr(lb, labels, N, R), ref.contacts(labels, N, R), R)


def refused(call, word):
    with pytest.raises(umx.UmxError) as e:
        call()
    assert e.value.code == umx.ERR_INVALID and word in str(e.value), str(e.value)


def test_refusals_leave_the_resident_labels():
    umx.require_torch_runtime("test_gpu_label_contacts")
    import torch
    planes, cls, min_area, classes = rings()
    H, W = BLOBS
    with umx.Labeler() as lb:
        refused(lb.contacts, "no labels")                            # before any run
        labels, table = lb.run(planes, cls, min_area, grow=3, grow_classes=classes)
        N = len(table)
        wanted = ref.contacts(labels, N)
        M = len(wanted)
        same(lb.contacts(), wanted, "after a run")
        refused(lambda: lb.contacts(0, W, H), "200 x 264")           # another shape
        refused(lambda: lb.contacts(0, 0, W), "at least 1")
        refused(lambda: lb.contacts(256), "reach")
        refused(lambda: lb.contacts(-1), "reach")
        with pytest.raises(umx.UmxError):
            lb.run(planes, cls, 0)                                   # a refused run (min_area 0) ...
        same(lb.contacts(), wanted, "after a refused run")           # ... leaves the resident labels as they were
        m = umx.ctypes.c_int64(-1)
        out = np.zeros(M, umx.LABEL_CONTACT_DTYPE)
        assert lb._L.umx_labeler_contacts(lb._lb, H, W, 0, None, 0, umx.ctypes.byref(m)) == 0 and m.value == M > 1
        m = umx.ctypes.c_int64(-1)
        rc = lb._L.umx_labeler_contacts(lb._lb, H, W, 0, out.ctypes.data, M - 1, umx.ctypes.byref(m))   # cap < M: M is reported
        assert rc == umx.ERR_INVALID and m.value == M and "records" in lb._L.umx_labeler_last_error(lb._lb).decode()
        assert not out.view(np.uint8).any()                          # nothing was written
        d_labels = torch.from_numpy(np.array(labels)).cuda()
        torch.cuda.synchronize()
        m = umx.ctypes.c_int64(-1)
        rc = lb._L.umx_labeler_contacts_dev(lb._lb, umx.ctypes.c_void_p(d_labels.data_ptr()), N, H, W, 0, out.ctypes.data, M - 1,
                                            umx.ctypes.byref(m))
        assert rc == umx.ERR_INVALID and m.value == M and not out.view(np.uint8).any()
        refused(lambda: lb.contacts_ptr(d_labels.data_ptr(), -1, H, W), "n_objects")
        refused(lambda: lb.contacts_ptr(0, N, H, W), "null")
        refused(lambda: lb.contacts_ptr(d_labels.data_ptr(), N, H, W, 256), "reach")
        same(lb.contacts(), wanted, "after refused contacts calls")
        _, t2 = lb.run(planes, cls, min_area, want_labels=False)
        refused(lb.contacts, "no label plane")                       # a later run without a label plane
        lb.run(planes, cls, min_area, grow=3, grow_classes=classes)
        same(lb.contacts(), wanted, "after a run with labels again")
        d_planes = torch.from_numpy(np.array(planes)).cuda()
        d_out = torch.zeros(BLOBS, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        lb.run_ptr(d_planes.data_ptr(), 3, H, W, d_out.data_ptr(), cls, min_area, grow=3, grow_classes=classes)
        refused(lb.contacts, "umx_labeler_run_dev")                  # the device run leaves its labels with the caller
        same(lb.contacts_ptr(d_out.data_ptr(), N, H, W), wanted, "the device run's own labels")
        labels2, table2 = lb.run(planes, cls, min_area, grow=2, grow_classes=classes)
        same(lb.contacts(), ref.contacts(labels2, len(table2)), "usable after every refusal")


@pytest.mark.parametrize("fill", ("0x00", "0xff"))
def test_guard_mode(fill, monkeypatch):
    """UMX_DEBUG_GUARD: red zones round every buffer of the contacts, which are exactly as large as asked for at a labeler's first
    call, and every buffer filled with the byte unless the call clears or writes it: the hand-made planes and one reach across two
    growth launches end with UMX_OK (no red zone touched) and the bytes of the unguarded run"""
    umx.require_torch_runtime("test_gpu_label_contacts")
    planes, cls, min_area = blobs()
    outs = []
    for mode in (None, fill):
        if mode is None:
            monkeypatch.delenv("UMX_DEBUG_GUARD", raising=False)
        else:
            monkeypatch.setenv("UMX_DEBUG_GUARD", mode)
        try:
            with umx.Labeler() as lb:
                got = [contacts_ptr(lb, labels, N) for _, labels, N, _ in ref.hand_made()]
                labels, table = lb.run(planes, cls, min_area)
                got.append(lb.contacts(reach=9))
                got.append(lb.contacts())
                got.append(contacts_ptr(lb, *want(9, 200)[:2]))
                outs.append([g.tobytes() for g in got])
        finally:
            monkeypatch.delenv("UMX_DEBUG_GUARD", raising=False)
    assert outs[0] == outs[1]
    assert outs[0][-3] == ref.contacts(labels, len(table), 9).tobytes() and outs[0][-1] == want(9, 200)[2].tobytes()


def test_command_writes_the_neighbors_and_changes_nothing_else(tmp_path):
    """UnMicst.py --stackOutput --labelMask --labelGrow 2 [--labelNeighbors [--labelNeighborsReach 3]] on a 96 x 130 crop of sample
    105: the Neighbors file's rows are the restatement on the Labels page the same run wrote; every other file has the bytes of the
    run without the flag, which writes no Neighbors file; with a reach of 3 the file is the restatement at that reach, which on this
    crop contains every contact of reach 0 (asked of the restatement first)."""
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

    def rows(path):
        lines = open(path).read().splitlines()
        assert lines[0] == ",".join(driver.NEIGHBOR_COLUMNS) == "label_a,label_b,shared_edges"
        return [tuple(int(v) for v in line.split(",")) for line in lines[1:]]
    plain, r = command("plain", ["--labelMask", "--labelGrow", "2"])
    assert r.returncode == 0, r.stderr[-2000:]
    out, r = command("neighbors", ["--labelMask", "--labelGrow", "2", "--labelNeighbors"])
    assert r.returncode == 0, r.stderr[-2000:]
    assert "crop_Labels_1.tif" in files(plain) and not [f for f in files(plain) if "Neighbors" in f]
    assert files(out) == sorted(files(plain) + ["crop_Neighbors_1.csv"])
    for f in files(plain):
        assert open(os.path.join(plain, f), "rb").read() == open(os.path.join(out, f), "rb").read(), f
    labels = tiffio.imread_all(os.path.join(out, "crop_Labels_1.tif"))[0]
    N = len(open(os.path.join(out, "crop_Objects_1.csv")).read().splitlines()) - 1
    assert N > 1 and labels.max() == N
    near = ref.as_tuples(ref.contacts(labels, N))
    got = rows(os.path.join(out, "crop_Neighbors_1.csv"))
    assert got == near
    degree = umx.contact_degrees(ref.contacts(labels, N), N)[0]
    assert "Label neighbors: %d contacts, largest degree %d" % (len(near), degree.max()) in r.stdout, r.stdout[-2000:]
    far = ref.as_tuples(ref.contacts(labels, N, 3))
    out3, r = command("reach", ["--labelMask", "--labelGrow", "2", "--labelNeighbors", "--labelNeighborsReach", "3"])
    assert r.returncode == 0, r.stderr[-2000:]
    assert rows(os.path.join(out3, "crop_Neighbors_1.csv")) == far
    assert open(os.path.join(out3, "crop_Labels_1.tif"), "rb").read() == open(os.path.join(plain, "crop_Labels_1.tif"), "rb").read()
    if {t[:2] for t in near} <= {t[:2] for t in far}:                # (what the restatement says of this crop decides)
        assert {t[:2] for t in near} <= {t[:2] for t in rows(os.path.join(out3, "crop_Neighbors_1.csv"))} and len(far) >= len(near)
    out, r = command("nomask", ["--labelNeighbors"])
    assert r.returncode == 2 and "--labelNeighbors needs --labelMask" in r.stderr, r.stderr[-2000:]
    out, r = command("noflag", ["--labelMask", "--labelNeighborsReach", "3"])
    assert r.returncode == 2 and "--labelNeighborsReach needs --labelNeighbors" in r.stderr, r.stderr[-2000:]
