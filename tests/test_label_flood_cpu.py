"""CPU checks of the label mask's level flood (include/umx.h and DESIGN.md section 8.1, steps 19 to 21): the consequences the definition
promises, on the restatement tests/label_flood_ref.py; umx_label_flood_check; the header against the binding; the drivers' refusals; the
outputs without the flag.  No GPU."""
import ctypes
import os
import re

import numpy as np
import pytest

import helpers
import label_flood_ref as ref
import label_grow_ref
import label_ref
import label_split_ref
from unmicst_amd import build, driver, model, umx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAIN = (150, 203)
STEPS = (1, 2, 4, 8, 16, 32, 64, 128, 256)


@pytest.fixture(scope="module")
def lib():
    build.build()
    return umx.load()


def test_levels():
    assert ref.levels(256) == [255] and ref.levels(16) == list(range(15, 256, 16)) and ref.levels(1) == list(range(256))
    for q in STEPS:
        lv = ref.levels(q)
        assert len(lv) == 256 // q and lv[-1] == 255 and lv == sorted(set(lv))


# ---- (a) one level is the split ----
@pytest.mark.parametrize("name,D,C", [("blobs", 2, 5), ("blobs", 3, 1), ("mixture2", 2, 1), ("salt", 1, 1), ("comb", 2, 1)])
def test_one_level_equals_the_split_with_the_longest_regrow(name, D, C):
    if name.startswith("mixture"):
        planes, cls, min_area = label_ref.planes_of(label_split_ref.mixture(*MAIN, 2), 3, 2, seed=11), 2, 1
    else:
        planes, cls, min_area = label_ref.case(*MAIN, name)
    labels, table, counts = label_split_ref.split(planes, cls, min_area, D, C, 255)
    assert counts["unreached"] == 0
    for P, invert in ((0, False), (1, True), (cls, False)):
        got = ref.split_flood(planes, cls, min_area, D, C, P, 256, invert)
        assert got[0].tobytes() == labels.tobytes() and got[1].tobytes() == table.tobytes()
        assert {k: got[2][k] for k in label_split_ref.COUNTS} == counts
        assert got[2]["levels_claimed"] == (1 if got[2]["claimed"] else 0)
        assert got[2]["claimed"] == int((labels > 0).sum() - (label_split_ref.seeds_of(label_ref.label(planes, cls, min_area)[0], D, C)[0] > 0).sum())


# ---- (b), (c), (e) ----
@pytest.mark.parametrize("q", [1, 16, 256])
def test_seeds_numbering_and_connectivity_are_the_splits(q):
    mask, relief = ref.blob_scene(*MAIN)
    planes = ref.planes_of(mask, relief)
    labels0 = label_ref.label(planes, 2, 1)[0]
    seeds, N, n_cored = label_split_ref.seeds_of(labels0, 2, 5)
    labels, table, counts = ref.split_flood(planes, 2, 1, 2, 5, 1, q)
    split = label_split_ref.split(planes, 2, 1, 2, 5)
    assert {k: counts[k] for k in label_split_ref.COUNTS} == split[2] and counts["n_objects"] == N > counts["n_before"]
    assert counts["unreached"] == 0 and np.array_equal(labels > 0, labels0 > 0) and counts["claimed"] == int((labels0 > 0).sum() - (seeds > 0).sum())
    assert np.array_equal(labels[seeds > 0], seeds[seeds > 0]) and label_grow_ref.connected(labels, N)
    assert len(table) == N and np.array_equal(table["area"], np.bincount(labels.ravel(), minlength=N + 1)[1:])
    # (c) an object with one core or none keeps exactly its pixels
    single = [o for o in range(1, counts["n_before"] + 1) if len(np.unique(seeds[(labels0 == o) & (seeds > 0)])) == 1]
    assert len(single) > 20
    for o in single:
        inside = labels0 == o
        assert len(np.unique(labels[inside])) == 1 and (labels == labels[inside][0]).sum() == inside.sum()
    # (e) a function of the planes and the options only
    again = ref.split_flood(planes, 2, 1, 2, 5, 1, q)
    assert again[0].tobytes() == labels.tobytes() and again[1].tobytes() == table.tobytes() and again[2] == counts
    if q == 1:
        assert not np.array_equal(labels, split[0])          # the relief moves the cuts
        assert 1 < counts["levels_claimed"] <= 255


def test_levels_claimed_counts_levels_not_pixels():
    """{3, 200} at q = 1: two levels claim; at q = 256 one; at q = 4 the levels 3 and 203"""
    mask, relief, placed = ref.ridge_scene(60, 100, [(40, 0), (60, 1)], low=3)
    relief = np.where(relief > 3, 200, relief)
    planes = ref.planes_of(mask, relief)
    ridge = int((relief == 200).sum())
    assert ridge == 2 * 2 * ref.DEPTH
    for q, n in ((1, 2), (4, 2), (256, 1)):
        c = ref.split_flood(planes, 2, 1, ref.DEPTH, 1, 1, q)[2]
        assert c["levels_claimed"] == n and c["unreached"] == 0 and c["n_objects"] == 4 and c["n_before"] == 2


# ---- (d) the cut lies on the ridge ----
@pytest.mark.parametrize("q", [1, 4, 16])
def test_a_neck_is_cut_on_its_ridge_wherever_it_stands(q):
    """every offset of the ridge in a bar of 9 columns: the columns before the ridge and the ridge itself (both neighbours labelled when
    its level comes: the smaller label) belong to the first body, the columns after it to the second.  The split's regrow cuts all of
    them after the middle column."""
    H, W = 130, 150
    ridges = [((24 if k % 2 == 0 else 88) + k % ref.LENGTH, k % ref.LENGTH) for k in range(12)]      # bars at columns 24 and 88, side by side
    mask, relief, placed = ref.ridge_scene(H, W, ridges)
    planes = ref.planes_of(mask, relief)
    labels, table, counts = ref.split_flood(planes, 2, 1, ref.DEPTH, 1, 1, q)
    by_distance = label_split_ref.split(planes, 2, 1, ref.DEPTH, 1)[0]
    assert counts["n_objects"] == 2 * counts["n_before"] == 2 * len(placed) == 24 and counts["unreached"] == 0
    assert np.array_equal(labels > 0, mask)
    moved = 0
    for top, bx, off, value in placed:
        rows = slice(top, top + 2 * ref.DEPTH)
        a, b = labels[top, bx - 1], labels[top, bx + ref.LENGTH]
        assert 0 < a < b and (labels[rows, bx - ref.SIZE:bx] == a).all() and (labels[rows, bx + ref.LENGTH:bx + ref.LENGTH + ref.SIZE] == b).all()
        assert (labels[rows, bx:bx + off + 1] == a).all() and (labels[rows, bx + off + 1:bx + ref.LENGTH] == b).all(), (off, q)
        assert (relief[rows, bx + off] == value).all()
        mid = (by_distance[rows, bx:bx + ref.LENGTH] == a).sum(axis=1)
        assert (mid == ref.LENGTH // 2 + 1).all()
        moved += off != ref.LENGTH // 2
    assert moved == 11                                     # offsets 0 .. 8, 0, 1, 2: the middle one once


def test_the_lower_gate_takes_the_chamber():
    """the trap of the GPU tests on the restatement: the chamber between the gates belongs to the label whose gate is lower"""
    for late, early, owner in ((50, 45, 2), (45, 50, 1)):
        mask, relief = ref.trap_scene(40, 130, late, early)
        for q in (1, 2, 4):
            labels, table, counts = ref.split_flood(ref.planes_of(mask, relief), 2, 1, 2, 1, 1, q)
            assert counts["n_objects"] == 2 and counts["n_before"] == 1 and counts["unreached"] == 0
            assert (labels[14, 48:64] == 1).all() and (labels[13:16, 71:91] == owner).all() and (labels[14, 65:96] == owner).all(), (late, q)
            assert labels[14, 64] == 1 and labels[14, 96] == (2 if owner == 2 else 1)
        # one level for both gates: the chamber is shared by distance
        shared = ref.split_flood(ref.planes_of(mask, relief), 2, 1, 2, 1, 1, 64)[0]
        assert len(np.unique(shared[13:16, 71:91])) == 2


def test_the_corridor_is_one_level_and_many_steps():
    mask, relief, path = ref.corridor_scene(130, 150)
    assert len(path) > 200
    labels, table, counts = ref.split_flood(ref.planes_of(mask, relief), 2, 1, 2, 1, 1, 1)
    cut = 3 * len(path) // 4
    assert counts["n_objects"] == 2 and counts["levels_claimed"] == 2 and counts["unreached"] == 0
    assert all(labels[y, x] == 1 for y, x in path[:cut + 1]) and all(labels[y, x] == 2 for y, x in path[cut + 1:])


def test_the_inverted_class_plane_is_the_same_relief():
    mask, relief = ref.blob_scene(70, 90)
    a = ref.split_flood(ref.planes_of(mask, relief), 2, 1, 2, 1, 1, 4)
    b = ref.split_flood(ref.planes_of(mask, relief, inverted=True), 2, 1, 2, 1, 2, 4, invert=True)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and a[2] == b[2]


# ---- umx_label_flood_check ----
def test_flood_check(lib):
    ok = umx.label_flood_check
    assert ok(3, 150, 203, 2) == "" and ok(3, 5, 5, 2, split=8, split_core=65536, flood=2, flood_step=256, flood_invert=True) == ""
    for q in STEPS:
        assert ok(3, 5, 5, 2, flood_step=q) == ""
    # the base's and the split's refusals, word for word
    for kw in (dict(cls=3), dict(min_area=0), dict(grow=256, grow_classes=(1,)), dict(split=0), dict(split=9), dict(split_core=0),
               dict(split_regrow=0), dict(split_regrow=256)):
        a = dict(cls=2)
        a.update(kw)
        below = umx.label_split_check(3, 5, 5, **a)
        assert below != "" and ok(3, 5, 5, **a) == below
    for K, H, W in ((3, 0, 5), (3, 65536, 65536), (0, 5, 5), (17, 5, 5)):
        below = umx.label_split_check(K, H, W, 0)
        assert below != "" and ok(K, H, W, 0) == below
    for j in range(2, 6):
        assert ok(3, 5, 5, 2, base_reserved=[0] * j + [1]) == "reserved must be zero"
    for j in range(5):
        assert ok(3, 5, 5, 2, split_reserved=[0] * j + [1]) == umx.label_split_check(3, 5, 5, 2, reserved=[0] * j + [1]) != ""
    # the split is checked first
    assert "depth" in ok(3, 5, 5, 2, split=0, flood=7)
    for L in (1, 8, 254):
        msg = ok(3, 5, 5, 2, split_regrow=L)
        assert "regrow is %d" % L in msg and "255" in msg
    for P in (-1, 3, 16, 2 ** 31 - 1, -2 ** 31):
        assert "relief_plane is %d" % P in ok(3, 5, 5, 2, flood=P), P
    assert ok(16, 5, 5, 2, flood=15) == ""
    for q in (0, -1, 3, 5, 6, 12, 255, 257, 512, 2 ** 30, -2 ** 31, 2 ** 31 - 1):
        assert "level_step is %d" % q in ok(3, 5, 5, 2, flood_step=q), q
    for v in (2, -1, 256):
        assert "invert is %d" % v in ok(3, 5, 5, 2, flood_invert=v), v
    for j in range(5):
        assert "reserved" in ok(3, 5, 5, 2, reserved=[0] * j + [1]) and "word %d" % j in ok(3, 5, 5, 2, reserved=[0] * j + [-1]), j
    assert "null" in ok(3, 5, 5, 2, null=True)
    # a short message buffer is filled and terminated; none at all is allowed
    o = umx._label_flood_options(umx._label_split_options(umx._label_options(3, 2, 1, 0, None), 2, 1, 255), 1, 3, False)
    buf = ctypes.create_string_buffer(b"\x7f" * 16, 16)
    assert lib.umx_label_flood_check(ctypes.byref(o), 3, 5, 5, buf, 8) == umx.ERR_INVALID
    assert buf.raw[:8] == b"level_s\x00" and buf.raw[8:] == b"\x7f" * 8
    assert lib.umx_label_flood_check(ctypes.byref(o), 3, 5, 5, None, 0) == umx.ERR_INVALID
    o.level_step = 4
    assert lib.umx_label_flood_check(ctypes.byref(o), 3, 5, 5, None, 0) == 0


# ---- header and binding ----
def test_binding_mirrors_the_header(lib):
    header = open(os.path.join(ROOT, "include", "umx.h")).read()
    enum = {k: int(v) for k, v in re.findall(r"(UMX_FLOOD_\w+) = (\d+)", header)}
    assert enum == {"UMX_FLOOD_MAX_STEP": umx.FLOOD_MAX_STEP, "UMX_FLOOD_DEFAULT_STEP": umx.FLOOD_DEFAULT_STEP,
                    "UMX_FLOOD_LAUNCH_STEPS": umx.FLOOD_LAUNCH_STEPS}
    assert set(re.findall(r"UMX_FLOOD_\w+", header)) == set(enum) and not re.findall(r"#define (UMX_FLOOD_\w+)", header)
    assert umx.FLOOD_MAX_STEP == 256 and umx.FLOOD_DEFAULT_STEP == 16 and umx.FLOOD_LAUNCH_STEPS == umx.LABEL_GROW_HALO
    body = re.search(r"typedef struct umx_label_flood_options \{(.*?)\} umx_label_flood_options;", header, re.S).group(1)
    assert re.findall(r"^\s*(\w+) (\w+)(?:\[(\d)\])?;", body, re.M) == [("umx_label_split_options", "split", ""), ("int32_t", "relief_plane", ""),
                                                                        ("int32_t", "invert", ""), ("int32_t", "level_step", ""),
                                                                        ("int32_t", "reserved", "5")]
    body = re.search(r"typedef struct umx_label_flood_counts \{(.*?)\} umx_label_flood_counts;", header, re.S).group(1)
    names = tuple(n for line in re.findall(r"int64_t ([\w, ]+);", body) for n in line.split(", "))
    assert names == ref.COUNTS + ("launches", "reserved") == tuple(n for n, _ in umx._LabelFloodCounts._fields_)
    assert names[:4] == tuple(n for n, _ in umx._LabelSplitCounts._fields_)
    F, C = umx._LabelFloodOptions, umx._LabelFloodCounts
    assert ctypes.sizeof(F) == 96 and ctypes.sizeof(C) == 64 and ctypes.sizeof(umx._LabelSplitOptions) == 64
    assert (F.split.offset, F.relief_plane.offset, F.invert.offset, F.level_step.offset, F.reserved.offset) == (0, 64, 68, 72, 76)
    assert [getattr(C, n).offset for n in names] == list(range(0, 64, 8))
    so = umx._label_split_options(umx._label_options(3, 2, 4, 3, (1,)), 2, 5, 255)
    o = umx._label_flood_options(so, 1, 16, True)
    assert bytes(o)[:64] == bytes(so) and bytes(o)[64:] == bytes(np.array([1, 1, 16, 0, 0, 0, 0, 0], "<i4"))
    for name in ("umx_label_flood_check", "umx_labeler_run_flood", "umx_labeler_run_flood_dev"):
        assert name in umx.EXPORTS and hasattr(ctypes.CDLL(build.lib_path()), name)
    # the older records are what they were
    assert ctypes.sizeof(umx._LabelOptions) == 32 and ctypes.sizeof(umx._LabelSplitCounts) == 32


# ---- the drivers ----
def _models(tmp_path, monkeypatch):
    hp, blob, mean, std = helpers.load_nuclei_dapi()
    models = tmp_path / "models"
    model.save_converted(model.ModelArtefacts(hp, blob, mean, std), str(models / "nucleiDAPI"))
    monkeypatch.setenv("UMX_MODELS_DIR", str(models))


def test_driver_refuses_bad_flood_flags_before_any_engine(tmp_path, monkeypatch, capsys):
    _models(tmp_path, monkeypatch)

    def no_engine(*a, **k):
        raise AssertionError("the engine was set up before the label flags were checked")
    monkeypatch.setattr(umx, "Engine", no_engine)
    img = str(tmp_path / "x" / "registration" / "missing.tif")   # never read: the refusal comes first
    lm, ls = ["--labelMask"], ["--labelMask", "--labelSplit", "2"]
    for tool in driver.TOOLS:
        for flags, word in ((["--labelFlood", "1"], "--labelFlood needs --labelMask"),
                            (["--labelFloodStep", "4"], "--labelFloodStep needs --labelMask"),
                            (["--labelFloodInvert"], "--labelFloodInvert needs --labelMask"),
                            (lm + ["--labelFlood", "1"], "--labelFlood needs --labelSplit"),
                            (ls + ["--labelFloodStep", "4"], "--labelFloodStep needs --labelFlood"),
                            (ls + ["--labelFloodInvert"], "--labelFloodInvert needs --labelFlood"),
                            (ls + ["--labelFlood", "-1"], "0..15"), (ls + ["--labelFlood", "16"], "0..15"),
                            (ls + ["--labelFlood", "3"], "the model has planes 0..2"),
                            (ls + ["--labelFlood", "1", "--labelFloodStep", "0"], "power of two"),
                            (ls + ["--labelFlood", "1", "--labelFloodStep", "3"], "power of two"),
                            (ls + ["--labelFlood", "1", "--labelFloodStep", "512"], "power of two"),
                            (ls + ["--labelFlood", "1", "--labelSplitRegrow", "8"], "it must be 255"),
                            (ls + ["--labelFlood"], "expected one argument")):
            with pytest.raises(SystemExit) as e:
                driver.run(tool, [img, "--model", "nucleiDAPI"] + flags)
            assert e.value.code == 2
            assert word in capsys.readouterr().err, (tool, flags)


class _Recorder:
    """stands in for the loaded library behind a Labeler: records the entry a run goes through and the bytes of its option record"""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def entry(lb, planes, K, H, W, options, labels, out):
            self.calls.append((name, bytes(options._obj)))
            return 0
        if name in ("umx_labeler_run", "umx_labeler_run_dev", "umx_labeler_run_split", "umx_labeler_run_split_dev", "umx_labeler_run_flood",
                    "umx_labeler_run_flood_dev"):
            return entry
        raise AttributeError(name)


def test_without_the_flag_every_call_reaches_the_library_as_before():
    """Byte identity on the path that needs no device.  The drivers' parsers leave the three flood arguments at None / None / False
    when the flag is absent, for every tool and beside every older label flag; and a Labeler that is not given a flood plane goes through
    the entry of before -- umx_labeler_run, or umx_labeler_run_split with the 64-byte record of before -- and never through the
    flood's.  What the label stage writes is a function of that call alone."""
    older = ["--labelMask", "--labelClass", "2", "--labelMinArea", "4", "--labelGrow", "3", "--labelGrowClasses", "1", "--labelSplit", "2",
             "--labelSplitCore", "5", "--labelSplitRegrow", "9", "--labelMeasure", "--labelShape"]
    for tool, spec in driver.TOOLS.items():
        parser = driver.build_parser(spec)
        for flags in ([], ["--labelMask"], older):
            a = parser.parse_args(["x.tif"] + flags)
            driver.check_label_args(parser, a)
            assert (a.labelFlood, a.labelFloodStep, a.labelFloodInvert) == (None, None, False), (tool, flags)
        a = parser.parse_args(["x.tif", "--labelMask", "--labelSplit", "2", "--labelFlood", "1", "--labelSplitRegrow", "255", "--labelFloodInvert"])
        driver.check_label_args(parser, a)
        assert (a.labelFlood, a.labelFloodStep, a.labelFloodInvert) == (1, None, True)
    lb = umx.Labeler.__new__(umx.Labeler)
    lb._L, lb._lb = _Recorder(), ctypes.c_void_p()
    base = umx._label_options(3, 2, 4, 3, (1,))
    for dev in (False, True):
        tail = "_dev" if dev else ""
        lb._L.calls.clear()
        lb._run_any(0, dev, 3, 5, 5, base, 0, 0, 1, 255)
        lb._run_any(0, dev, 3, 5, 5, base, 0, 2, 5, 9)
        lb._run_any(0, dev, 3, 5, 5, base, 0, 2, 5, 9, None, 4, True)          # a step and an inversion without a plane: still no flood
        assert lb.flood_counts() is None and lb.split_counts() is not None
        lb._run_any(0, dev, 3, 5, 5, base, 0, 2, 5, 255, 1, 4, True)
        assert set(lb.flood_counts()) == set(ref.COUNTS + ("launches",)) and set(lb.split_counts()) == set(label_split_ref.COUNTS)
        split_record = bytes(umx._label_split_options(base, 2, 5, 9))
        assert len(split_record) == 64
        assert lb._L.calls[:3] == [("umx_labeler_run" + tail, bytes(base)), ("umx_labeler_run_split" + tail, split_record),
                                   ("umx_labeler_run_split" + tail, split_record)]
        name, record = lb._L.calls[3]
        assert name == "umx_labeler_run_flood" + tail and len(record) == 96
        assert record == bytes(umx._label_split_options(base, 2, 5, 255)) + bytes(np.array([1, 1, 4, 0, 0, 0, 0, 0], "<i4"))
    lb._lb = ctypes.c_void_p()                                                 # (nothing to destroy)


def test_bench_tool_ridges():
    """tools/bench_label.py --flood: every bridge holds a ridge two columns into it, and the flood cuts there, not in the middle"""
    import importlib.util
    spec = importlib.util.spec_from_file_location("bench_label", os.path.join(ROOT, "tools", "bench_label.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    D = 3
    H, W = 6 * m.PAIR_H, 5 * m.PAIR_W
    planes = m.ridged_planes(H, W, D, 1)
    mask = m.bridged_mask(H, W, D)
    assert np.array_equal(label_grow_ref.pred_of(planes) == 2, mask) and np.array_equal(planes[2], m.planes_of(mask)[2])
    assert (planes[1] == m.RIDGE).sum() == 2 * D * (label_ref.label_mask(mask, 1)[1].size) > 0
    labels, table, counts = ref.split_flood(planes, 2, 1, D, 1, 1, 16)
    cut = label_split_ref.split(planes, 2, 1, D, 1)
    assert counts["n_objects"] == 2 * counts["n_before"] == cut[2]["n_objects"] and counts["unreached"] == 0 and counts["levels_claimed"] == 2
    bridge = 2 * D * (m.PAIR_W - 8 - 2 * m.SQUARE)
    areas = np.sort(table["area"])
    assert areas[0] == m.SQUARE ** 2 + 2 * D * 3 and areas[-1] == m.SQUARE ** 2 + bridge - 2 * D * 3      # three columns and five
    assert np.sort(cut[1]["area"])[0] == m.SQUARE ** 2 + bridge // 2
