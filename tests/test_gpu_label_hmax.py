"""GPU tests of the label mask's h-maxima seeds (unmicst_amd/csrc/umx_label_hmax.hip; include/umx.h and DESIGN.md section 8.1, steps 33
to 36): the labels, every field of the table and the counts of umx_labeler_run_hmax / _run_hmax_dev against tests/label_hmax_ref.py,
compared for equality.  Everything is an integer: there is no tolerance anywhere in this file.  `launches` and `recon_launches` are
informative; the latter is held to 1 <= n <= UMX_HMAX_MAX_LAUNCHES and to nothing else."""
import ctypes
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
from scipy import ndimage

import helpers
import label_contact_ref
import label_hmax_ref as ref
import label_measure_ref
import label_ref
import label_shape_ref
import label_split_ref
from unmicst_amd import model, tiffio, umx

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

T, HALO = umx.LABEL_GROW_TILE, umx.LABEL_GROW_HALO
TALL, WIDE = (2 * T + 2, 2 * T + 22), (T + 6, 3 * T + 8)      # 130 x 150 and 70 x 200: seams at 64 and 128
ODD = (97, 131)                                              # a width that is no multiple of 4: the byte planes' rows are unaligned
LITTLE = (40, 50)                                            # smaller than a tile
SHAPES = [TALL, WIDE, TALL[::-1], WIDE[::-1], ODD]
IDS = ["%dx%d" % s for s in SHAPES]
S, P = 3, 1                                                  # the seed plane and the flood's relief plane of ref.planes_of


@functools.lru_cache(maxsize=None)
def scene(shape, name):
    """-> planes uint8 [4][H][W].  A name ending in "^T" is the scene of the transposed shape, transposed."""
    if name.endswith("^T"):
        planes = np.ascontiguousarray(scene(shape[::-1], name[:-2]).transpose(0, 2, 1))
        planes.setflags(write=False)
        return planes
    H, W = shape
    rim, flood_relief = None, None
    if name == "peaks":
        mask, relief, _ = ref.peak_scene(H, W)
    elif name == "plateau":
        mask, relief = ref.plateau_scene(H, W)
    elif name == "serpentine":
        mask, relief, _ = ref.serpentine_scene(H, W)
    elif name == "domes":
        mask, relief = ref.dome_scene(H, W)
        flood_relief = np.where(mask, 254 - relief, 0)
    elif name == "noise":
        mask, relief = ref.noise_scene(H, W)
        flood_relief = np.where(mask, np.random.default_rng(9).integers(0, 255, (H, W)), 0)
    elif name == "rimmed":
        mask, relief, _ = ref.overlapping_discs(H, W)
        rim = ndimage.binary_dilation(mask, iterations=3)
    elif name == "specks":
        mask, relief = ref.speck_scene(H, W)
    elif name == "full":
        mask, relief = np.ones((H, W), bool), np.random.default_rng(8).integers(0, 255, (H, W))
    elif name == "empty":
        mask, relief = np.zeros((H, W), bool), np.zeros((H, W), np.int64)
    else:
        raise KeyError(name)
    planes = ref.planes_of(mask, relief, flood_relief, rim)
    planes.setflags(write=False)
    return planes


@functools.lru_cache(maxsize=None)
def want(shape, name, h, C=1, q=None, invert=False, R=0, plane=S):
    """(labels, table, counts): the restatement, computed once per case and never changed"""
    labels, table, counts = ref.hmax(scene(shape, name), 2, 1, h, plane, invert, C, None if q is None else P, q or 256, False, R,
                                     (1,) if R else None)
    labels.setflags(write=False)
    table.setflags(write=False)
    return labels, table, counts


def kwargs_of(h, C=1, q=None, invert=False, R=0, plane=S):
    kw = dict(grow=R, grow_classes=(1,) if R else None, hmax=h, hmax_plane=plane, hmax_invert=invert, hmax_core=C)
    if q is not None:
        kw.update(flood=P, flood_step=q)
    return kw


@pytest.fixture(scope="module")
def lab():
    with umx.Labeler() as lb:
        yield lb


def same(got_labels, got_table, lab, wanted, what):
    labels, table, counts = wanted
    if got_labels is not None:
        assert got_labels.dtype == np.int32 and got_labels.shape == labels.shape
        assert np.array_equal(got_labels, labels), (what, int((got_labels != labels).sum()))
    assert len(got_table) == len(table), (what, len(got_table), len(table))
    for f in label_ref.FIELDS:
        assert np.array_equal(got_table[f], table[f]), (what, f)
    got = dict(lab.hmax_counts())
    got.pop("launches")
    recon = got.pop("recon_launches")
    assert got == counts, (what, got, counts)
    assert len(recon) == 2 and all(1 <= n <= umx.HMAX_MAX_LAUNCHES for n in recon), (what, recon)
    assert lab.split_counts() == {k: counts[k] for k in label_split_ref.COUNTS}
    assert {k: v for k, v in lab.flood_counts().items() if k != "launches"} == {k: counts[k] for k in ref.COUNTS if k != "seed_pixels"}
    return recon


def check(lab, shape, name, h, **kw):
    planes = scene(shape, name)
    a = lab.run(planes, 2, 1, **kwargs_of(h, **kw))
    recon = same(a[0], a[1], lab, want(shape, name, h, **kw), (shape, name, h, kw))
    counts = dict(lab.hmax_counts(), recon_launches=None)
    b = lab.run(planes, 2, 1, **kwargs_of(h, **kw))               # twice: the same bytes
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and dict(lab.hmax_counts(), recon_launches=None) == counts
    return recon


def test_the_inputs_are_what_they_are_for():
    """asserted on the restatement alone"""
    assert TALL == (130, 150) and WIDE == (70, 200) and ODD[1] % 4
    for shape in (TALL, WIDE, ODD):
        _, _, peaks = ref.peak_scene(*shape)
        labels, table, counts = want(shape, "peaks", 40)
        assert counts["n_before"] == counts["n_cored"] == 1 and counts["n_objects"] == counts["seed_pixels"] == len(peaks) > 20
        assert sorted(labels[y, x] for y, x, _ in peaks) == list(range(1, len(peaks) + 1)) and counts["unreached"] == 0
        assert want(shape, "peaks", 1)[2]["n_objects"] > 4 * len(peaks)          # the noise
        assert want(shape, "peaks", 255)[2]["n_objects"] == 1
    ys, xs = ref.peak_places(*TALL)
    assert {0, T - HALO, T - 1, T, T + HALO - 1, 2 * T - 1, 2 * T, TALL[0] - 1} <= set(ys) and {T - 1, T, 2 * T - 1, 2 * T, TALL[1] - 1} <= set(xs)
    for shape in (TALL, WIDE):
        mask, relief = ref.plateau_scene(*shape)
        g = ref.hmaxima(relief, 10)
        E = ref.extended_maxima(g)
        assert E[4, T + HALO + 4] and E[4].sum() == (shape[1] - 1) // T and not E[4, T - 14:T + HALO + 4].any()    # the 140 alone: its plateau is none
        assert E[10, T - 14:T + HALO + 4].all() and (g[4, T - 14:T + HALO + 4] == 100).all()      # raised from 90 from beyond the halo
        mask, relief, path = ref.serpentine_scene(*shape)
        assert 3000 < len(path) < 10000 and int(ref.seed_set(relief, 40).sum()) >= len(path) // 6
        assert set((y // T, x // T) for y, x in path) == set((y, x) for y in range((shape[0] - 1) // T + 1) for x in range((shape[1] - 1) // T + 1))
    pairs = ref.overlapping_discs(*TALL)[2]
    c = want(TALL, "rimmed", 40, R=3)[2]
    assert c["n_before"] == pairs and c["n_objects"] == 2 * pairs                # cut where no erosion of depth <= 8 cuts
    assert label_split_ref.split(scene(TALL, "rimmed"), 2, 1, 8)[2]["n_objects"] == pairs


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_peaks_on_the_seams_and_in_the_halo_rings(lab, shape):
    name = "peaks^T" if shape[0] > shape[1] and shape != ODD else "peaks"
    for h in (1, 40, 255):
        for C in (1, 5):
            check(lab, shape, name, h, C=C)


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_a_plateau_whose_fate_is_decided_in_another_tile(lab, shape):
    name = "plateau^T" if shape[0] > shape[1] and shape != ODD else "plateau"
    for h in (10, 40):
        check(lab, shape, name, h)
    check(lab, shape, name, 10, q=16)


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_a_value_travels_along_a_serpentine_through_every_tile(lab, shape):
    name = "serpentine^T" if shape[0] > shape[1] and shape != ODD else "serpentine"
    check(lab, shape, name, 40)
    check(lab, shape, name, 1, C=5)


@pytest.mark.parametrize("q", [None, 1, 16, 256])
def test_blobs_with_domes_and_with_noise(lab, q):
    for invert in (False, True):
        check(lab, TALL, "domes", 40, q=q, invert=invert)
        check(lab, WIDE[::-1], "noise^T", 1, q=q, invert=invert, C=5 if invert else 1)
    check(lab, ODD, "domes", 1, q=q, C=5)
    check(lab, ODD, "noise", 40, q=q)


def test_wide_necks_are_cut_and_the_rim_grows_afterwards(lab):
    for shape in (TALL, ODD):
        check(lab, shape, "rimmed", 40, R=3)
        check(lab, shape, "rimmed", 40, R=3, q=16, C=5)
    check(lab, TALL, "rimmed", 255, R=3)


@pytest.mark.parametrize("shape", [(1, 1), (1, 130), (130, 1), (2, 2), LITTLE, (T, T), (T + 1, T + 1)])
def test_small_shapes(lab, shape):
    for name in ("full", "empty", "specks", "noise"):
        for h in (1, 40, 255):
            check(lab, shape, name, h)
        check(lab, shape, name, 1, q=1, C=5, invert=True)


def test_no_core_and_one_plateau_are_the_plain_labelling(lab):
    """consequences (b) and (c): h = 255, and a relief that is constant and above h on M (the class plane itself: 255 there)"""
    for shape, name in ((TALL, "domes"), (ODD, "noise"), (WIDE, "rimmed"), (LITTLE, "specks")):
        planes = scene(shape, name)
        for R in (0, 3):
            plain = lab.run(planes, 2, 1, grow=R, grow_classes=(1,) if R else None)
            assert lab.hmax_counts() is None
            for h, plane, seeds in ((255, S, 0), (255, 2, 0), (40, 2, int((plain[0] > 0).sum()) if R == 0 else None)):
                got = lab.run(planes, 2, 1, **kwargs_of(h, R=R, plane=plane))
                assert got[0].tobytes() == plain[0].tobytes() and got[1].tobytes() == plain[1].tobytes(), (shape, name, R, h, plane)
                c = lab.hmax_counts()
                assert c["n_objects"] == c["n_before"] == len(plain[1]) and c["claimed"] == c["unreached"] == 0
                assert seeds is None or c["seed_pixels"] == seeds
                assert c["n_cored"] == (0 if h == 255 else c["n_before"])
            same(got[0], got[1], lab, want(shape, name, 40, R=R, plane=2), (shape, name, "class plane"))


def test_hmax_with_split_is_refused_by_the_binding(lab):
    with pytest.raises(ValueError):
        lab.run(scene(LITTLE, "noise"), 2, 1, split=2, hmax=40)


def test_without_a_label_plane(lab):
    got_labels, got_table = lab.run(scene(TALL, "domes"), 2, 1, want_labels=False, **kwargs_of(40, q=16))
    assert got_labels is None
    same(None, got_table, lab, want(TALL, "domes", 40, q=16), "no plane")


def test_run_hmax_dev_on_torch_tensors_equals_the_host_entry(lab):
    import torch
    umx.require_torch_runtime("test_gpu_label_hmax")
    for shape, name, h, kw in ((TALL, "peaks", 40, {}), (ODD, "domes", 40, dict(q=16)), (WIDE, "plateau", 10, {}), (TALL, "rimmed", 40, dict(R=3))):
        planes = scene(shape, name)
        wanted = want(shape, name, h, **kw)
        K, H, W = planes.shape
        d_planes = torch.from_numpy(np.array(planes)).cuda()
        d_labels = torch.full((H, W), -7, dtype=torch.int32, device="cuda")     # a sentinel: every word must be written
        torch.cuda.synchronize()
        tables = []
        for _ in range(2):                                                      # twice: the same bytes
            d_labels.fill_(-7)
            torch.cuda.synchronize()
            tables.append(lab.run_ptr(d_planes.data_ptr(), K, H, W, d_labels.data_ptr(), 2, 1, **kwargs_of(h, **kw)))
            same(d_labels.cpu().numpy(), tables[-1], lab, wanted, (name, "dev"))
        assert tables[0].tobytes() == tables[1].tobytes()
        host_labels, host_table = lab.run(planes, 2, 1, **kwargs_of(h, **kw))
        assert host_labels.tobytes() == d_labels.cpu().numpy().tobytes() and host_table.tobytes() == tables[0].tobytes()
        none = lab.run_ptr(d_planes.data_ptr(), K, H, W, 0, 2, 1, **kwargs_of(h, **kw))
        same(None, none, lab, wanted, (name, "dev, no plane"))
        assert np.array_equal(d_planes.cpu().numpy(), planes)                   # the planes are only read


def test_a_large_then_a_small_then_the_large_shape_on_one_labeler():
    """the third plane holds the bytes of the run before, of another shape, when the relief kernel starts: nothing of them shows; and
    the older entries after an h-maxima run give a fresh labeler's bytes"""
    with umx.Labeler() as lb, umx.Labeler() as fresh:
        for shape, name, h, kw in ((TALL, "noise", 1, dict(q=16)), (LITTLE, "noise", 40, {}), (TALL, "noise", 1, dict(q=16)), (ODD, "domes", 40, {}),
                                   ((1, 130), "full", 1, {}), (TALL, "peaks", 40, {}), (LITTLE, "specks", 1, {}), (TALL, "serpentine", 40, {})):
            check(lb, shape, name, h, **kw)
        planes = scene(TALL, "noise")
        for kw in (dict(), dict(split=2, split_core=5), dict(split=2, flood=P, flood_step=16)):
            a, b = lb.run(planes, 2, 1, **kw), fresh.run(planes, 2, 1, **kw)
            assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
            assert lb.hmax_counts() is None and lb.split_counts() == fresh.split_counts() and lb.flood_counts() == fresh.flood_counts()
            check(lb, LITTLE, "noise", 40)


def test_measure_shape_and_contacts_take_the_new_labels(lab):
    planes = scene(TALL, "rimmed")
    labels, table, counts = want(TALL, "rimmed", 40, q=16)
    N = counts["n_objects"]
    px = label_measure_ref.pixels(TALL, np.uint16, 2, seed=5)
    got_labels, got_table = lab.run(planes, 2, 1, **kwargs_of(40, q=16))
    rec = lab.measure(px)
    wanted = label_measure_ref.measure(labels, px, N)
    assert rec.shape == wanted.shape == (2, N) and rec.tobytes() == wanted.tobytes() and np.array_equal(rec["count"][0], got_table["area"])
    assert lab.shape().tobytes() == label_shape_ref.records(labels, N).tobytes()
    contacts = lab.contacts()
    assert contacts.tobytes() == label_contact_ref.contacts(labels, N).tobytes() and len(contacts) == counts["n_before"]   # one cut per pair
    assert not np.array_equal(labels, label_ref.label(planes, 2, 1)[0])
    lab.run(planes, 2, 1, want_labels=False, **kwargs_of(40, q=16))
    with pytest.raises(umx.UmxError) as e:
        lab.measure(px)
    assert e.value.code == umx.ERR_INVALID and "no label plane" in str(e.value)


def test_a_refused_call_touches_nothing_and_keeps_the_resident_labels(lab):
    planes = scene(TALL, "domes")
    labels, table, counts = want(TALL, "domes", 40, q=16)
    px = label_measure_ref.pixels(TALL, np.uint8, 1, seed=6)
    good = kwargs_of(40, q=16)
    lab.run(planes, 2, 1, **good)
    before, shapes = lab.measure(px), lab.shape()
    out = np.full(TALL, -7, np.int32)
    H, W = TALL
    for kw, word in ((dict(hmax=0), "height"), (dict(hmax=256), "height"), (dict(hmax_plane=4), "seed_plane"), (dict(hmax_plane=-1), "seed_plane"),
                     (dict(hmax_invert=2), "seed_invert"), (dict(hmax_core=0), "core_min_area"), (dict(flood=4), "relief_plane"),
                     (dict(flood_step=3), "level_step"), (dict(min_area=0), "min_area"), (dict(grow=256, grow_classes=(1,)), "grow_radius")):
        kw = dict(dict(good, min_area=1), **kw)
        with pytest.raises(umx.UmxError) as e:
            lab.run(planes, 2, **kw)
        assert e.value.code == umx.ERR_INVALID and word in str(e.value), kw
        o = umx._label_hmax_options(umx._label_options(4, 2, kw["min_area"], kw["grow"], kw["grow_classes"]), kw["hmax"], kw["hmax_plane"],
                                    kw["hmax_invert"], kw["hmax_core"], kw["flood"], kw["flood_step"], False)
        for fn in (lab._L.umx_labeler_run_hmax,):
            assert fn(lab._lb, planes.ctypes.data, 4, H, W, ctypes.byref(o), out.ctypes.data, None) == umx.ERR_INVALID
        assert (out == -7).all()                                  # the caller's plane is not written
        assert lab.measure(px).tobytes() == before.tobytes() and lab.shape().tobytes() == shapes.tobytes()
    o = umx._label_hmax_options(umx._label_options(4, 2, 1, 0, None), 40, S, False, 1, None, 16, False)
    o.flood.split.depth = 0                                       # not used, and still the split's check must pass
    assert lab._L.umx_labeler_run_hmax(lab._lb, planes.ctypes.data, 4, H, W, ctypes.byref(o), out.ctypes.data, None) == umx.ERR_INVALID
    assert "depth" in lab._L.umx_labeler_last_error(lab._lb).decode()
    assert lab._L.umx_labeler_run_hmax(lab._lb, planes.ctypes.data, 4, H, W, None, out.ctypes.data, None) == umx.ERR_INVALID
    assert (out == -7).all() and lab.measure(px).tobytes() == before.tobytes()
    assert before.tobytes() == label_measure_ref.measure(labels, px, counts["n_objects"]).tobytes()
    check(lab, TALL, "domes", 40, q=16)


def test_the_depth_is_not_looked_at(lab):
    planes = scene(TALL, "domes")
    H, W = TALL
    outs = []
    for depth in (1, 8):
        o = umx._label_hmax_options(umx._label_options(4, 2, 1, 0, None), 40, S, False, 1, None, 16, False)
        o.flood.split.depth = depth
        out, hc = np.full(TALL, -7, np.int32), umx._LabelHmaxCounts()
        assert lab._L.umx_labeler_run_hmax(lab._lb, planes.ctypes.data, 4, H, W, ctypes.byref(o), out.ctypes.data, ctypes.byref(hc)) == 0
        outs.append(out)
    assert outs[0].tobytes() == outs[1].tobytes() == want(TALL, "domes", 40)[0].tobytes()


_GUARD_CHILD = """
import sys
sys.path.insert(0, %r); sys.path.insert(0, %r)
import test_gpu_label_hmax as t
from unmicst_amd import umx
with umx.Labeler() as lb:
    for shape, cases in (((1, 1), (("full", 1, {}),)), ((1, 130), (("full", 1, {}),)), ((130, 1), (("noise", 40, {}),)),
                         (t.LITTLE, (("specks", 1, {}), ("noise", 40, dict(q=1)))),
                         (t.ODD, (("peaks", 40, {}), ("domes", 1, dict(q=16, C=5)), ("plateau", 10, {}))),
                         (t.WIDE, (("plateau", 10, {}), ("serpentine", 40, {}), ("peaks", 1, dict(C=5)))),
                         (t.TALL, (("peaks", 40, {}), ("domes", 40, dict(q=16, invert=True)), ("rimmed", 40, dict(R=3)), ("noise", 255, {}))),
                         (t.TALL[::-1], (("peaks^T", 40, {}), ("serpentine^T", 40, {})))):   # (no shape smaller than one before it)
        for name, h, kw in cases:
            t.check(lb, shape, name, h, **kw)                  # (raises UmxError 7 when a red zone was written)
print("guard-ok")
"""


def test_guard_mode_finds_no_write_outside_the_buffers():
    """UMX_DEBUG_GUARD=0xa5 in a child process (the variable is read at umx_labeler_create): red zones round the three planes -- the
    third one exactly 4 * H * W bytes at a shape's first run, which the four byte planes fill to the last byte --, the flags and the
    h-maxima's words, checked at the end of every run"""
    env = dict(os.environ, UMX_DEBUG_GUARD="0xa5")
    r = subprocess.run([sys.executable, "-c", _GUARD_CHILD % (ROOT, os.path.join(ROOT, "tests"))], env=env, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0 and "guard-ok" in r.stdout, r.stderr[-2000:]


def test_command_seeds_the_label_mask_by_h_maxima(tmp_path, lab):
    """UnMicst.py --stackOutput --labelMask --labelHmax 40 --labelHmaxCore 3 --labelFlood 1 --labelFloodStep 4 --labelMeasure
    --labelShape on the 150 x 171 crop of sample 105: the label page and the tables are the restatement applied to the probability pages
    the same run wrote -- the nuclei plane as the seed relief, the contour plane as the flood's.  Without --labelHmax the files are those
    of the plain labelling of before."""
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
    for sub, flags in (("hmax", ["--labelHmax", "40", "--labelHmaxCore", "3", "--labelFlood", "1", "--labelFloodStep", "4"]), ("plain", [])):
        out = outs[sub] = str(tmp_path / sub)
        r = subprocess.run([sys.executable, os.path.join(ROOT, "UnMicst.py"), img, "--model", "nucleiDAPI", "--stackOutput", "--outputPath", out,
                            "--labelMask", "--labelMinArea", "4", "--labelMeasure", "--labelShape"] + flags, env=env, capture_output=True,
                           text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        pages = tiffio.imread_all(os.path.join(out, "crop_Probabilities_1.tif"))
        assert pages.shape == (3, 150, 171) and pages.dtype == np.uint8
        planes = np.ascontiguousarray(pages[::-1])                # the pages are in reversed class order
        if sub == "hmax":
            labels, table, counts = ref.hmax(planes, 2, 4, 40, 2, False, 3, 1, 4)
            assert counts["n_objects"] >= counts["n_before"] > 1 and counts["n_cored"] >= 1 and counts["seed_pixels"] >= 1
            line = [l for l in r.stdout.splitlines() if l.startswith("Label hmax: ")]
            assert len(line) == 1 and line[0].startswith("Label hmax: %d seed pixels, %d objects from %d (%d with a core), reconstructions in "
                                                         % (counts["seed_pixels"], counts["n_objects"], counts["n_before"], counts["n_cored"]))
            assert "Label flood: %d pixels claimed at %d levels in " % (counts["claimed"], counts["levels_claimed"]) in r.stdout
        else:
            labels, table = label_ref.label(planes, 2, 4)
            assert "Label hmax" not in r.stdout and "Label flood" not in r.stdout and "Label split" not in r.stdout
            got_labels, got_table = lab.run(planes, 2, 4)             # the entry of before, on the same planes
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
        assert len(open(os.path.join(out, "crop_Shapes_1.csv")).read().splitlines()) == N + 1
    # the seeds change nothing but the label files
    assert open(os.path.join(outs["hmax"], "crop_Probabilities_1.tif"), "rb").read() == open(os.path.join(outs["plain"], "crop_Probabilities_1.tif"), "rb").read()
