"""CPU checks of the label mask's split at the necks (include/umx.h and DESIGN.md section 8.1, steps 10 to 15): the restatement
tests/label_split_ref.py against a second statement of steps 11 to 13 and against the properties the definition promises, with counts
derived on paper; umx_label_split_check; the header against the binding; the drivers' refusals.  No GPU."""
import ctypes
import os
import re

import numpy as np
import pytest
from scipy import ndimage

import helpers
import label_grow_ref
import label_ref
import label_split_ref as ref
from unmicst_amd import build, driver, model, umx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAIN = (150, 203)


@pytest.fixture(scope="module")
def lib():
    build.build()
    return umx.load()


def pred_of_mask(mask):
    """class 2 on the mask, class 1 off it"""
    return np.where(mask, 2, 1)


def split_mask(mask, D, C=1, L=255, min_area=1):
    return ref.split_pred(pred_of_mask(mask), 2, min_area, D, C, L)


# ---- 1. a second statement of steps 11 to 13 ----
def ball_erode(M, D):
    """E by the definition's sentence: the city-block ball of radius D round the pixel lies wholly in M; outside the image is not in M"""
    H, W = M.shape
    p = np.pad(M, D, constant_values=False)
    E = np.ones_like(M)
    for dy in range(-D, D + 1):
        for dx in range(-(D - abs(dy)), D - abs(dy) + 1):
            E &= p[D + dy:D + dy + H, D + dx:D + dx + W]
    return E


def seeds_by_the_sentence(labels0, D, C):
    """cores and seeds object by object, with scipy's labelling directly: -> (S, n_cored)"""
    M = labels0 > 0
    comp, n = ndimage.label(ball_erode(M, D))
    S = np.zeros_like(M)
    n_cored = 0
    for obj in range(1, int(labels0.max()) + 1):
        inside = labels0 == obj
        cores = [k for k in np.unique(comp[inside]) if k > 0 and (comp == k).sum() >= C]
        assert all((labels0[comp == k] == obj).all() for k in cores)          # a component of E lies in one object
        if cores:
            n_cored += 1
            S |= np.isin(comp, cores)
        else:
            S |= inside
    return S, n_cored


@pytest.mark.parametrize("name", ["blobs", "blobs_min40", "salt", "comb", "cls0"])
def test_restatement_equals_the_second_statement(name):
    H, W = 60, 75
    planes, cls, min_area = label_ref.case(H, W, name)
    labels0 = label_ref.label(planes, cls, min_area)[0]
    for D, C in ((1, 1), (1, 3), (2, 1), (2, 5), (3, 1), (8, 1)):
        assert np.array_equal(ref.erode(labels0 > 0, D), ball_erode(labels0 > 0, D)), (D,)
        seeds, N, n_cored = ref.seeds_of(labels0, D, C)
        S, n_cored2 = seeds_by_the_sentence(labels0, D, C)
        assert np.array_equal(seeds > 0, S) and n_cored == n_cored2, (D, C)
        assert np.array_equal(seeds, ndimage.label(S)[0]) and N == seeds.max() >= labels0.max()
        labels, table, counts = ref.split(planes, cls, min_area, D, C)
        assert counts == dict(n_objects=N, n_before=int(labels0.max()), n_cored=n_cored, unreached=int(((labels0 > 0) & (labels == 0)).sum()))
        assert len(table) == N and np.array_equal(table["area"], np.bincount(labels.ravel(), minlength=N + 1)[1:])


# ---- 2. properties, with counts derived on paper ----
@pytest.mark.parametrize("D", [1, 2, 3, 5])
def test_a_bar_is_cut_iff_it_is_at_most_2D_wide(D):
    """A pixel of a bar of w rows survives the erosion iff D rows above and D below it are in the bar: iff w >= 2 D + 1.  The squares'
    cores (15 - 2 D >= 5 pixels wide) are then one component or two."""
    for w, N in ((2 * D - 1, 2), (2 * D, 2), (2 * D + 1, 1)):
        m = ref.bridge(w)
        labels, table, counts = split_mask(m, D)
        assert counts == dict(n_objects=N, n_before=1, n_cored=1, unreached=0), (D, w)
        assert np.array_equal(labels > 0, m)                                 # every pixel comes back
        if N == 2:
            # the cut lies in the bar: each square belongs to one object whole, and the bar's columns are shared half and half
            # (equal distances; the middle column of the odd length goes to the smaller label)
            assert (labels[2:17, 2:17] == 1).all() and (labels[2:17, 22:37] == 2).all()
            bar = labels[:, 17:22]
            assert ((bar[:, :3] == 1) | (bar[:, :3] == 0)).all() and ((bar[:, 3:] == 2) | (bar[:, 3:] == 0)).all()


def test_a_single_core_object_keeps_exactly_its_pixels():
    planes, cls, min_area = label_ref.case(*MAIN, "blobs")
    labels0, table0 = label_ref.label(planes, cls, min_area)
    labels, table, counts = ref.split(planes, cls, min_area, 2, 5)
    seeds, N, n_cored = ref.seeds_of(labels0, 2, 5)
    single = [o for o in range(1, len(table0) + 1) if len(np.unique(seeds[(labels0 == o) & (seeds > 0)])) == 1]
    assert len(single) > 20 and counts["unreached"] == 0
    for o in single:
        inside = labels0 == o
        assert len(np.unique(labels[inside])) == 1 and (labels == labels[inside][0]).sum() == inside.sum()
    assert np.array_equal(labels > 0, labels0 > 0)


@pytest.mark.parametrize("D,C", [(1, 1), (2, 5), (3, 1)])
def test_every_object_is_connected_and_contains_its_seed(D, C):
    planes, cls, min_area = label_ref.case(*MAIN, "blobs")
    labels0 = label_ref.label(planes, cls, min_area)[0]
    labels, table, counts = ref.split(planes, cls, min_area, D, C)
    seeds, N, _ = ref.seeds_of(labels0, D, C)
    assert counts["n_objects"] == N > counts["n_before"]
    assert np.array_equal(labels[seeds > 0], seeds[seeds > 0]) and label_grow_ref.connected(labels, N)
    assert ((labels > 0) <= (labels0 > 0)).all()                              # no front leaves an object
    again = ref.split(planes, cls, min_area, D, C)
    assert again[0].tobytes() == labels.tobytes() and again[1].tobytes() == table.tobytes() and again[2] == counts


def test_prototype_counts_on_blobs():
    """the figures the issue records for blobs at 150 x 203"""
    planes, cls, min_area = label_ref.case(*MAIN, "blobs")
    c = ref.split(planes, cls, min_area, 2, 5)[2]
    assert (c["n_before"], c["n_objects"], c["n_cored"]) == (111, 141, 52)
    assert ref.split(planes, cls, min_area, 2, 1)[2]["n_objects"] == 218


@pytest.mark.parametrize("D", [1, 2, 3, 8])
def test_the_smallest_square_with_a_core(D):
    """(2 D + 1) x (2 D + 1): the centre is the only pixel at distance >= D from all four edges.  At C = 2 the square has no core and
    stays whole as it is."""
    n = 2 * D + 1
    m = np.zeros((n + 4, n + 6), bool)
    m[2:2 + n, 3:3 + n] = True
    E = ref.erode(m, D)
    assert E.sum() == 1 and E[2 + D, 3 + D]
    labels, table, counts = split_mask(m, D, 1)
    assert counts == dict(n_objects=1, n_before=1, n_cored=1, unreached=0) and np.array_equal(labels > 0, m)
    labels, table, counts = split_mask(m, D, 2)
    assert counts == dict(n_objects=1, n_before=1, n_cored=0, unreached=0) and np.array_equal(labels > 0, m)
    labels, table, counts = split_mask(m, D, 1, L=D - 1 if D > 1 else 1)      # the far corner is 2 D steps from the centre
    assert counts["unreached"] == (n * n - (2 * (D - 1) * (D - 1) + 2 * (D - 1) + 1) if D > 1 else n * n - 5)


def test_an_object_cut_by_the_image_edge_erodes_from_that_edge():
    D = 2
    for edge in ("top", "bottom", "left", "right"):
        m = np.zeros((12, 12), bool)
        m[3:9, 3:9] = True
        if edge == "top": m[0:3, 3:9] = True
        if edge == "bottom": m[9:12, 3:9] = True
        if edge == "left": m[3:9, 0:3] = True
        if edge == "right": m[3:9, 9:12] = True
        E = ref.erode(m, D)
        want = np.zeros_like(m)                                              # 9 x 6 or 6 x 9 less two pixels on every side, the image's too
        if edge == "top": want[2:7, 5:7] = True
        if edge == "bottom": want[5:10, 5:7] = True
        if edge == "left": want[5:7, 2:7] = True
        if edge == "right": want[5:7, 5:10] = True
        assert np.array_equal(E, want), edge
    full = np.ones((7, 9), bool)
    assert np.array_equal(ref.erode(full, 3), ball_erode(full, 3)) and ref.erode(full, 3).sum() == 1 * 3


def test_a_short_regrow_leaves_exactly_the_far_pixels():
    """one 15 x 15 square, D = 3: the core is the 9 x 9 square; after L levels a pixel is reached iff its city-block distance to the
    core is <= L.  The corner is 6 away."""
    m = np.zeros((19, 19), bool)
    m[2:17, 2:17] = True
    core = ref.erode(m, 3)
    assert core.sum() == 81
    dist = ndimage.distance_transform_cdt(~core, metric="taxicab")
    for L in (1, 2, 5, 6):
        labels, table, counts = split_mask(m, 3, 1, L)
        assert np.array_equal(labels > 0, m & (dist <= L)) and counts["unreached"] == int((m & (dist > L)).sum())
        assert (counts["unreached"] > 0) == (L < 6)
    planes, cls, min_area = label_ref.case(*MAIN, "blobs")
    assert ref.split(planes, cls, min_area, 3, 1, 2)[2]["unreached"] > 0      # the GPU test's short case is not vacuous


def test_split_then_grow_is_the_composition():
    pred = ref.rimmed_pairs(*MAIN)
    labels, table, counts = ref.split_pred(pred, 2, 1, 2, 5, 255, 3, (1,))
    inner = ref.split_pred(pred, 2, 1, 2, 5, 255)
    assert counts == inner[2] and counts["n_objects"] > counts["n_before"] > 4
    assert np.array_equal(labels, label_grow_ref.grow(inner[0], pred, (1,), 3)) and (labels > 0).sum() > (inner[0] > 0).sum()
    assert np.array_equal(labels[inner[0] > 0], inner[0][inner[0] > 0]) and label_grow_ref.connected(labels, counts["n_objects"])
    assert np.array_equal(table["area"], np.bincount(labels.ravel(), minlength=len(table) + 1)[1:])
    # every second dumbbell has a bar of 2 D + 1 rows and stays one object
    assert counts["n_objects"] - counts["n_before"] == (counts["n_before"] + 1) // 2


@pytest.mark.parametrize("name", ["checker", "comb", "serpentine"])
def test_objects_too_thin_for_a_core_come_back_whole(name):
    planes, cls, min_area = label_ref.case(*MAIN, name)
    labels0, table0 = label_ref.label(planes, cls, min_area)
    for D in (1, 2, 8):
        labels, table, counts = ref.split(planes, cls, min_area, D, 1)
        assert counts == dict(n_objects=len(table0), n_before=len(table0), n_cored=0, unreached=0)
        assert np.array_equal(labels, labels0) and table.tobytes() == table0.tobytes()


# ---- 3. umx_label_split_check ----
def test_split_check(lib):
    ok = umx.label_split_check
    assert ok(3, 150, 203, 2) == "" and ok(3, 5, 5, 2, split=8, split_core=65536, split_regrow=1) == ""
    assert ok(3, 5, 5, 2, grow=3, grow_classes=(1,), split=2, split_core=5) == ""
    # the base's refusals, word for word
    for kw in (dict(cls=3), dict(min_area=0), dict(grow=256, grow_classes=(1,)), dict(grow=2, grow_classes=()), dict(grow=0, grow_classes=(1,)),
               dict(grow=2, grow_classes=(1, 3))):
        a = dict(cls=2, min_area=1, grow=0, grow_classes=None)
        a.update(kw)
        base = umx.label_options_check(3, 5, 5, a["cls"], a["min_area"], grow=a["grow"], grow_classes=a["grow_classes"])
        assert base != "" and ok(3, 5, 5, a["cls"], a["min_area"], grow=a["grow"], grow_classes=a["grow_classes"], split=2) == base
    for K, H, W in ((3, 0, 5), (3, 5, -1), (3, 65536, 65536), (0, 5, 5), (17, 5, 5)):
        base = umx.label_options_check(K, H, W, 0, 1)
        assert base != "" and ok(K, H, W, 0, 1) == base
    for j in range(2, 6):
        assert ok(3, 5, 5, 2, base_reserved=[0] * j + [1]) == "reserved must be zero"
    # the base is checked first
    assert "cls" in ok(3, 5, 5, 3, split=0)
    for d in (0, -1, 9, 2 ** 31 - 1, -2 ** 31):
        assert "depth" in ok(3, 5, 5, 2, split=d), d
    for c in (0, -1, 65537, -2 ** 31):
        assert "core_min_area" in ok(3, 5, 5, 2, split_core=c), c
    for l in (0, -1, 256, 2 ** 31 - 1):
        assert "regrow" in ok(3, 5, 5, 2, split_regrow=l), l
    for j in range(5):
        assert "reserved" in ok(3, 5, 5, 2, reserved=[0] * j + [1]), j
        assert "reserved" in ok(3, 5, 5, 2, reserved=[0] * j + [-1]), j
    assert "null" in ok(3, 5, 5, 2, null=True)
    # a short message buffer is filled and terminated; none at all is allowed
    o = umx._label_split_options(umx._label_options(3, 2, 1, 0, None), 9, 1, 255)
    buf = ctypes.create_string_buffer(b"\x7f" * 16, 16)
    assert lib.umx_label_split_check(ctypes.byref(o), 3, 5, 5, buf, 8) == umx.ERR_INVALID
    assert buf.raw[:8] == b"depth i\x00" and buf.raw[8:] == b"\x7f" * 8
    assert lib.umx_label_split_check(ctypes.byref(o), 3, 5, 5, None, 0) == umx.ERR_INVALID
    o.depth = 2
    assert lib.umx_label_split_check(ctypes.byref(o), 3, 5, 5, None, 0) == 0


# ---- 4. header and binding ----
def test_binding_mirrors_the_header(lib):
    header = open(os.path.join(ROOT, "include", "umx.h")).read()
    enum = {k: int(v) for k, v in re.findall(r"(UMX_SPLIT_\w+) = (\d+)", header)}
    assert enum == {"UMX_SPLIT_MAX_DEPTH": umx.SPLIT_MAX_DEPTH, "UMX_SPLIT_MAX_CORE_AREA": umx.SPLIT_MAX_CORE_AREA,
                    "UMX_SPLIT_MAX_REGROW": umx.SPLIT_MAX_REGROW}
    assert umx.SPLIT_MAX_DEPTH == 8 <= umx.LABEL_GROW_HALO and umx.SPLIT_MAX_REGROW == 255 and umx.SPLIT_MAX_CORE_AREA == umx.LABEL_MAX_MIN_AREA
    body = re.search(r"typedef struct umx_label_split_options \{(.*?)\} umx_label_split_options;", header, re.S).group(1)
    assert re.findall(r"^\s*(\w+) (\w+)(?:\[(\d)\])?;", body, re.M) == [("umx_label_options", "base", ""), ("int32_t", "depth", ""),
                                                                        ("int32_t", "core_min_area", ""), ("int32_t", "regrow", ""),
                                                                        ("int32_t", "reserved", "5")]
    body = re.search(r"typedef struct umx_label_split_counts \{(.*?)\} umx_label_split_counts;", header, re.S).group(1)
    assert tuple(re.findall(r"int64_t (\w+);", body)) == ref.COUNTS == tuple(n for n, _ in umx._LabelSplitCounts._fields_)
    S, C = umx._LabelSplitOptions, umx._LabelSplitCounts
    assert ctypes.sizeof(S) == 64 and ctypes.sizeof(C) == 32
    assert (S.base.offset, S.depth.offset, S.core_min_area.offset, S.regrow.offset, S.reserved.offset) == (0, 32, 36, 40, 44)
    assert [getattr(C, n).offset for n in ref.COUNTS] == [0, 8, 16, 24]
    base = umx._label_options(3, 2, 4, 3, (1,))
    o = umx._label_split_options(base, 2, 5, 255)
    assert bytes(o)[:32] == bytes(base) and bytes(o)[32:] == bytes(np.array([2, 5, 255, 0, 0, 0, 0, 0], "<i4"))
    assert not re.findall(r"#define (UMX_SPLIT_\w+)", header)
    for name in ("umx_label_split_check", "umx_labeler_run_split", "umx_labeler_run_split_dev"):
        assert name in umx.EXPORTS and hasattr(ctypes.CDLL(build.lib_path()), name)


# ---- 5. the drivers ----
def test_driver_refuses_bad_split_flags_before_any_engine(tmp_path, monkeypatch, capsys):
    hp, blob, mean, std = helpers.load_nuclei_dapi()
    models = tmp_path / "models"
    model.save_converted(model.ModelArtefacts(hp, blob, mean, std), str(models / "nucleiDAPI"))
    monkeypatch.setenv("UMX_MODELS_DIR", str(models))

    def no_engine(*a, **k):
        raise AssertionError("the engine was set up before the label flags were checked")
    monkeypatch.setattr(umx, "Engine", no_engine)
    img = str(tmp_path / "x" / "registration" / "missing.tif")   # never read: the refusal comes first
    lm = ["--labelMask"]
    for tool in driver.TOOLS:
        for flags, word in ((["--labelSplit", "2"], "--labelSplit needs --labelMask"),
                            (["--labelSplitCore", "2"], "--labelSplitCore needs --labelMask"),
                            (["--labelSplitRegrow", "2"], "--labelSplitRegrow needs --labelMask"),
                            (lm + ["--labelSplitCore", "2"], "--labelSplitCore needs --labelSplit"),
                            (lm + ["--labelSplitRegrow", "2"], "--labelSplitRegrow needs --labelSplit"),
                            (lm + ["--labelSplit", "0"], "1..8"), (lm + ["--labelSplit", "9"], "1..8"), (lm + ["--labelSplit", "-1"], "1..8"),
                            (lm + ["--labelSplit", "2", "--labelSplitCore", "0"], "1..65536"),
                            (lm + ["--labelSplit", "2", "--labelSplitCore", "65537"], "1..65536"),
                            (lm + ["--labelSplit", "2", "--labelSplitRegrow", "0"], "1..255"),
                            (lm + ["--labelSplit", "2", "--labelSplitRegrow", "256"], "1..255"),
                            (lm + ["--labelSplit"], "expected one argument")):
            with pytest.raises(SystemExit) as e:
                driver.run(tool, [img, "--model", "nucleiDAPI"] + flags)
            assert e.value.code == 2
            assert word in capsys.readouterr().err, (tool, flags)


def test_bench_tool_bridges():
    """tools/bench_label.py --split D: bodies joined in pairs by bridges of width <= 2 D, so every pair is cut"""
    import importlib.util
    spec = importlib.util.spec_from_file_location("bench_label", os.path.join(ROOT, "tools", "bench_label.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    for D in (2, 3):
        mask = m.bridged_mask(10 * m.PAIR_H, 7 * m.PAIR_W, D)                # (whole cells: no pair is cut by the image's edge)
        planes = m.planes_of(mask)
        assert np.array_equal(label_grow_ref.pred_of(planes) == 2, mask)
        labels, table, counts = ref.split(planes, 2, 1, D, 1)
        assert counts["n_before"] > 10 and counts["n_objects"] == 2 * counts["n_before"] and counts["unreached"] == 0
