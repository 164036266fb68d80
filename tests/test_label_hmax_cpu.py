"""CPU checks of the label mask's h-maxima seeds (include/umx.h and DESIGN.md section 8.1, steps 33 to 36): the two forms of step 35 and
the consequences (a) to (f) the definition promises, on the restatement tests/label_hmax_ref.py; umx_label_hmax_check; the header against
the binding; the drivers' refusals; the calls without the flag.  No GPU."""
import ctypes
import os
import re

import numpy as np
import pytest
from scipy import ndimage

import helpers
import label_flood_ref
import label_grow_ref
import label_hmax_ref as ref
import label_ref
import label_split_ref
from unmicst_amd import build, driver, model, umx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAIN = (90, 110)


@pytest.fixture(scope="module")
def lib():
    build.build()
    return umx.load()


def row(values):
    """a one-row image whose object is the pixels of relief > 0 -> (planes, relief)"""
    relief = np.array([values])
    return ref.planes_of(relief > 0, relief), relief


def seeds_in_row(values, h):
    E = ref.seed_set(np.array([values]), h)
    return ndimage.label(E, ref.CROSS)[1], E[0]


# ---- step 35: the reconstruction form is the plateau form ----
def test_extended_maxima_are_the_plateaus_without_a_higher_neighbour():
    rng = np.random.default_rng(12)
    for k in range(120):
        H, W = rng.integers(1, 41, 2)
        mask = ndimage.binary_opening(rng.random((H, W)) < 0.7, iterations=int(rng.integers(0, 2))) if k % 3 else rng.random((H, W)) < 0.8
        top = int(rng.choice([3, 20, 255]))                      # few values: wide plateaus; many: none
        f = np.where(mask, rng.integers(0, top + 1, (H, W)), 0)
        for h in (1, int(rng.integers(1, top + 1)), 255):
            g = ref.hmaxima(f, h)
            assert (g <= f).all() and (g >= np.maximum(f - h, 0)).all()
            E = ref.extended_maxima(g)
            assert np.array_equal(E, ref.plateau_maxima(g)), (k, h)
            assert not (E & ~mask).any() and E.any() == (f.max() > h)
            # g is a fixed point, and the least one: lowering any of its plateaus that holds no marker pixel at its own value leaves one
            c = np.pad(g, 1)
            up = np.maximum(np.maximum(c[:-2, 1:-1], c[2:, 1:-1]), np.maximum(c[1:-1, :-2], c[1:-1, 2:]))
            assert np.array_equal(g, np.minimum(f, np.maximum(g, up)))


# ---- (d): the three rows, literally ----
def test_two_peaks_over_a_saddle():
    assert seeds_in_row([0, 200, 60, 100, 0], 39)[0] == 2 and seeds_in_row([0, 200, 60, 100, 0], 40)[0] == 1
    n, E = seeds_in_row([0, 100, 60, 100, 0], 39)
    assert n == 2 and list(E) == [False, True, False, True, False]
    n, E = seeds_in_row([0, 100, 60, 100, 0], 40)
    assert n == 1 and list(E) == [False, True, True, True, False]      # one plateau, the saddle in it
    for a, b, s in ((100, 200, 60), (90, 90, 10), (255, 255, 254), (50, 250, 49), (3, 9, 1)):
        for h in range(1, 256, 1 if b < 20 else 13):
            n = seeds_in_row([b, s, a], h)[0]
            assert n == (2 if a - s > h else 1 if b > h else 0), (a, b, s, h)
    labels, table, counts = ref.hmax(row([0, 200, 60, 100, 0])[0], 2, 1, 39, 3)
    assert labels.tolist() == [[0, 1, 1, 2, 0]] and counts["n_objects"] == 2 and counts["seed_pixels"] == 2   # the saddle goes to the smaller label
    assert ref.hmax(row([0, 200, 60, 100, 0])[0], 2, 1, 40, 3)[0].tolist() == [[0, 1, 1, 1, 0]]


# ---- (a), (b), (c), (e), (f) ----
def scenes():
    for name, (mask, relief) in (("domes", ref.dome_scene(*MAIN)), ("noise", ref.noise_scene(*MAIN)), ("specks", ref.speck_scene(*MAIN)),
                                 ("plateau", ref.plateau_scene(*MAIN)), ("discs", ref.overlapping_discs(*MAIN)[:2])):
        flood_relief = np.where(mask, np.random.default_rng(2).integers(0, 255, MAIN), 0)
        yield name, ref.planes_of(mask, relief, flood_relief, ndimage.binary_dilation(mask, iterations=2)), relief


def test_cored_objects_are_those_whose_peak_exceeds_h():
    """(a)"""
    for name, planes, relief in scenes():
        labels0, table0 = label_ref.label(planes, 2, 3)
        tops = ndimage.maximum(relief, labels0, np.arange(1, len(table0) + 1)) if len(table0) else np.zeros(0)
        for h in (1, 40, 119, 120, 254, 255):
            c = ref.hmax(planes, 2, 3, h, 3)[2]
            assert c["n_before"] == len(table0) and c["n_cored"] == int((tops > h).sum()), (name, h)
            inv = ref.hmax(planes, 2, 3, h, 3, True)[2]
            assert inv["n_cored"] == int((255 - ndimage.minimum(relief, labels0, np.arange(1, len(table0) + 1)) > h).sum()), (name, h)


def test_no_core_and_one_plateau_are_the_plain_labelling():
    """(b) and (c)"""
    for name, planes, relief in scenes():
        for R in (0, 2):
            plain = label_grow_ref.label_grow(planes, 2, 3, R, (1,) if R else None)
            for h, S, q in ((255, 3, None), (255, 2, 16), (40, 2, None), (254, 2, 1)):      # plane 2 is 255 on every object
                got = ref.hmax(planes, 2, 3, h, S, False, 1, None if q is None else 1, q or 256, False, R, (1,) if R else None)
                assert got[0].tobytes() == plain[0].tobytes() and got[1].tobytes() == plain[1].tobytes(), (name, R, h, S)
                assert got[2]["n_objects"] == got[2]["n_before"] == len(plain[1]) and got[2]["claimed"] == 0
                assert got[2]["n_cored"] == (0 if h == 255 else len(plain[1]))


@pytest.mark.parametrize("q", [None, 1, 16])
def test_objects_contain_their_seeds_and_are_connected(q):
    """(e) and (f)"""
    for name, planes, relief in scenes():
        for h, C in ((1, 1), (40, 1), (40, 5), (1, 5)):
            args = (planes, 2, 3, h, 3, False, C, None if q is None else 1, q or 256)
            labels, table, counts = ref.hmax(*args)
            labels0 = label_ref.label(planes, 2, 3)[0]
            E = ref.seed_set(ref.seed_relief(planes, labels0, 3), h)
            seeds, N, n_cored = ref.seeds_of(labels0, E, C)
            assert N == counts["n_objects"] >= counts["n_before"] and counts["unreached"] == 0 and counts["seed_pixels"] == int(E.sum())
            assert np.array_equal(labels[seeds > 0], seeds[seeds > 0]) and np.array_equal(labels > 0, labels0 > 0)
            assert label_grow_ref.connected(labels, N)
            again = ref.hmax(*args)
            assert again[0].tobytes() == labels.tobytes() and again[1].tobytes() == table.tobytes() and again[2] == counts
            if C == 1:
                assert N - counts["n_before"] == ndimage.label(E, ref.CROSS)[1] - counts["n_cored"]


def test_wide_necks_are_cut_where_no_erosion_cuts():
    mask, relief, pairs = ref.overlapping_discs(*MAIN)
    planes = ref.planes_of(mask, relief)
    assert pairs >= 2 and all(label_split_ref.split(planes, 2, 1, D)[2]["n_objects"] == pairs for D in (4, 8))
    labels, table, counts = ref.hmax(planes, 2, 1, 40, 3)
    assert counts["n_objects"] == 2 * pairs and counts["n_cored"] == counts["n_before"] == pairs
    assert abs(int(table["area"].max()) - int(table["area"].min())) <= 40          # the cut runs down the middle of every pair


# ---- umx_label_hmax_check ----
def test_hmax_check(lib):
    ok = umx.label_hmax_check
    assert ok(3, 150, 203, 2) == "" and ok(3, 5, 5, 2, hmax=255, hmax_plane=0, hmax_invert=True, hmax_core=65536, flood=2, flood_step=1) == ""
    assert ok(16, 5, 5, 2, hmax_plane=15) == "" and ok(3, 5, 5, 2, depth=8) == ""
    # the inner records' refusals, word for word: the base's and the split's through the flood's
    for kw in (dict(cls=3), dict(min_area=0), dict(grow=256, grow_classes=(1,)), dict(flood=3), dict(flood=-1), dict(flood=1, flood_step=3),
               dict(flood=1, flood_step=512), dict(flood=1, flood_invert=2)):
        a = dict(cls=2)
        a.update(kw)
        below = umx.label_flood_check(3, 5, 5, **a)
        assert below != "" and ok(3, 5, 5, **a) == below, kw
    for K, H, W in ((3, 0, 5), (3, 65536, 65536), (0, 5, 5), (17, 5, 5)):
        below = umx.label_flood_check(K, H, W, 0)
        assert below != "" and ok(K, H, W, 0) == below
    for depth in (0, 9, -1):
        assert ok(3, 5, 5, 2, depth=depth) == umx.label_split_check(3, 5, 5, 2, split=depth) != ""
    for C in (0, 65537):
        assert ok(3, 5, 5, 2, hmax_core=C) == umx.label_split_check(3, 5, 5, 2, split_core=C) != ""
    for j in range(2, 6):
        assert ok(3, 5, 5, 2, base_reserved=[0] * j + [1]) == "reserved must be zero"
    for j in range(5):
        assert ok(3, 5, 5, 2, split_reserved=[0] * j + [1]) == umx.label_split_check(3, 5, 5, 2, reserved=[0] * j + [1]) != ""
        assert ok(3, 5, 5, 2, flood_reserved=[0] * j + [1]) == umx.label_flood_check(3, 5, 5, 2, reserved=[0] * j + [1]) != ""
    # the flood is checked first
    assert "level_step" in ok(3, 5, 5, 2, flood=1, flood_step=3, hmax=0)
    # its own bounds, on both sides
    for h in (1, 2, 254, 255):
        assert ok(3, 5, 5, 2, hmax=h) == ""
    for h in (0, -1, 256, 2 ** 31 - 1, -2 ** 31):
        assert "height is %d" % h in ok(3, 5, 5, 2, hmax=h), h
    for S in (0, 1, 2):
        assert ok(3, 5, 5, 2, hmax_plane=S) == ""
    for S in (-1, 3, 16, 2 ** 31 - 1, -2 ** 31):
        assert "seed_plane is %d" % S in ok(3, 5, 5, 2, hmax_plane=S), S
    assert ok(3, 5, 5, 2, hmax_invert=0) == ok(3, 5, 5, 2, hmax_invert=1) == ""
    for v in (2, -1, 256):
        assert "seed_invert is %d" % v in ok(3, 5, 5, 2, hmax_invert=v), v
    for j in range(5):
        assert "reserved" in ok(3, 5, 5, 2, reserved=[0] * j + [1]) and "word %d" % j in ok(3, 5, 5, 2, reserved=[0] * j + [-1]), j
    assert "null" in ok(3, 5, 5, 2, null=True)
    # a short message buffer is filled and terminated; none at all is allowed
    o = umx._label_hmax_options(umx._label_options(3, 2, 1, 0, None), 0, None, False, 1, None, 16, False)
    buf = ctypes.create_string_buffer(b"\x7f" * 16, 16)
    assert lib.umx_label_hmax_check(ctypes.byref(o), 3, 5, 5, buf, 8) == umx.ERR_INVALID
    assert buf.raw[:8] == b"height \x00" and buf.raw[8:] == b"\x7f" * 8
    assert lib.umx_label_hmax_check(ctypes.byref(o), 3, 5, 5, None, 0) == umx.ERR_INVALID
    o.height = 4
    assert lib.umx_label_hmax_check(ctypes.byref(o), 3, 5, 5, None, 0) == 0


# ---- header and binding ----
def test_binding_mirrors_the_header(lib):
    header = open(os.path.join(ROOT, "include", "umx.h")).read()
    enum = {k: int(v) for k, v in re.findall(r"(UMX_HMAX_\w+) = (\d+)", header)}
    assert enum == {"UMX_HMAX_MAX_HEIGHT": umx.HMAX_MAX_HEIGHT, "UMX_HMAX_LAUNCH_STEPS": umx.HMAX_LAUNCH_STEPS,
                    "UMX_HMAX_MAX_LAUNCHES": umx.HMAX_MAX_LAUNCHES}
    assert set(re.findall(r"UMX_HMAX_\w+", header)) == set(enum) and not re.findall(r"#define (UMX_HMAX_\w+)", header)
    # a launch carries a value a halo's width along any path at the least: a path of 10 000 pixels converges
    assert umx.HMAX_LAUNCH_STEPS >= umx.LABEL_GROW_HALO and umx.HMAX_MAX_LAUNCHES * umx.LABEL_GROW_HALO > 10000 and umx.HMAX_MAX_HEIGHT == 255
    body = re.search(r"typedef struct umx_label_hmax_options \{(.*?)\} umx_label_hmax_options;", header, re.S).group(1)
    assert re.findall(r"^\s*(\w+) (\w+)(?:\[(\d)\])?;", body, re.M) == [("umx_label_flood_options", "flood", ""), ("int32_t", "seed_plane", ""),
                                                                        ("int32_t", "seed_invert", ""), ("int32_t", "height", ""),
                                                                        ("int32_t", "reserved", "5")]
    body = re.search(r"typedef struct umx_label_hmax_counts \{(.*?)\} umx_label_hmax_counts;", header, re.S).group(1)
    assert re.findall(r"^\s*(\w+) (\w+)(?:\[(\d)\])?;", body, re.M) == [("umx_label_flood_counts", "flood", ""), ("int64_t", "seed_pixels", ""),
                                                                        ("int64_t", "recon_launches", "2"), ("int64_t", "reserved", "")]
    O, C = umx._LabelHmaxOptions, umx._LabelHmaxCounts
    assert ctypes.sizeof(O) == 128 and ctypes.sizeof(C) == 96
    assert (O.flood.offset, O.seed_plane.offset, O.seed_invert.offset, O.height.offset, O.reserved.offset) == (0, 96, 100, 104, 108)
    assert (C.flood.offset, C.seed_pixels.offset, C.recon_launches.offset, C.reserved.offset) == (0, 64, 72, 88)
    base = umx._label_options(3, 2, 4, 3, (1,))
    fo = umx._label_flood_options(umx._label_split_options(base, 1, 5, 255), 1, 4, True)
    o = umx._label_hmax_options(base, 40, 0, True, 5, 1, 4, True)
    assert bytes(o)[:96] == bytes(fo) and bytes(o)[96:] == bytes(np.array([0, 1, 40, 0, 0, 0, 0, 0], "<i4"))
    # without a flood: one level on the class plane; without a seed plane: the class plane
    o = umx._label_hmax_options(base, 7, None, False, 1, None, 4, True)
    assert bytes(o)[:96] == bytes(umx._label_flood_options(umx._label_split_options(base, 1, 1, 255), 2, 256, False))
    assert bytes(o)[96:] == bytes(np.array([2, 0, 7, 0, 0, 0, 0, 0], "<i4"))
    for name in ("umx_label_hmax_check", "umx_labeler_run_hmax", "umx_labeler_run_hmax_dev"):
        assert name in umx.EXPORTS and hasattr(ctypes.CDLL(build.lib_path()), name)
    # the older records are what they were, and their reserved words are still refused
    assert ctypes.sizeof(umx._LabelOptions) == 32 and ctypes.sizeof(umx._LabelSplitOptions) == 64 and ctypes.sizeof(umx._LabelSplitCounts) == 32
    assert ctypes.sizeof(umx._LabelFloodOptions) == 96 and ctypes.sizeof(umx._LabelFloodCounts) == 64
    for j in range(5):
        assert umx.label_split_check(3, 5, 5, 2, reserved=[0] * j + [1]) != "" and umx.label_flood_check(3, 5, 5, 2, reserved=[0] * j + [1]) != ""
    for j in range(2, 6):
        assert umx.label_options_check(3, 5, 5, 2, reserved=[0] * j + [1]) != ""
    # the header no longer says that h-maxima are missing
    assert "Not here: h-maxima" not in header


# ---- the drivers ----
def _models(tmp_path, monkeypatch):
    hp, blob, mean, std = helpers.load_nuclei_dapi()
    models = tmp_path / "models"
    model.save_converted(model.ModelArtefacts(hp, blob, mean, std), str(models / "nucleiDAPI"))
    monkeypatch.setenv("UMX_MODELS_DIR", str(models))


def test_driver_refuses_bad_hmax_flags_before_any_engine(tmp_path, monkeypatch, capsys):
    _models(tmp_path, monkeypatch)

    def no_engine(*a, **k):
        raise AssertionError("the engine was set up before the label flags were checked")
    monkeypatch.setattr(umx, "Engine", no_engine)
    img = str(tmp_path / "x" / "registration" / "missing.tif")   # never read: the refusal comes first
    lm, lh = ["--labelMask"], ["--labelMask", "--labelHmax", "40"]
    for tool in driver.TOOLS:
        for flags, word in ((["--labelHmax", "40"], "--labelHmax needs --labelMask"),
                            (["--labelHmaxPlane", "1"], "--labelHmaxPlane needs --labelMask"),
                            (["--labelHmaxInvert"], "--labelHmaxInvert needs --labelMask"),
                            (["--labelHmaxCore", "3"], "--labelHmaxCore needs --labelMask"),
                            (lm + ["--labelHmaxPlane", "1"], "--labelHmaxPlane needs --labelHmax"),
                            (lm + ["--labelHmaxInvert"], "--labelHmaxInvert needs --labelHmax"),
                            (lm + ["--labelHmaxCore", "3"], "--labelHmaxCore needs --labelHmax"),
                            (lh + ["--labelSplit", "2"], "it excludes --labelSplit"),
                            (lh + ["--labelSplit", "2", "--labelSplitCore", "3"], "it excludes --labelSplit"),
                            (lh + ["--labelSplit", "2", "--labelFlood", "1"], "it excludes --labelSplit"),
                            (lh + ["--labelSplitCore", "3"], "--labelSplitCore needs --labelSplit"),        # (today's words)
                            (lm + ["--labelHmax", "0"], "1..255"), (lm + ["--labelHmax", "256"], "1..255"), (lm + ["--labelHmax", "-3"], "1..255"),
                            (lh + ["--labelHmaxPlane", "-1"], "0..15"), (lh + ["--labelHmaxPlane", "16"], "0..15"),
                            (lh + ["--labelHmaxPlane", "3"], "the model has planes 0..2"),
                            (lh + ["--labelHmaxCore", "0"], "1..65536"), (lh + ["--labelHmaxCore", "65537"], "1..65536"),
                            (lh + ["--labelFlood", "3"], "the model has planes 0..2"),
                            (lh + ["--labelFlood", "1", "--labelFloodStep", "3"], "power of two"),
                            (lh + ["--labelFloodStep", "4"], "--labelFloodStep needs --labelFlood"),
                            (lm + ["--labelFlood", "1"], "--labelFlood needs --labelSplit"),                # (today's words)
                            (lm + ["--labelHmax"], "expected one argument")):
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
        if name.startswith("umx_labeler_run"):
            return entry
        raise AttributeError(name)


def test_the_flags_reach_the_library_and_without_them_every_call_is_the_one_of_before():
    older = ["--labelMask", "--labelClass", "2", "--labelMinArea", "4", "--labelGrow", "3", "--labelGrowClasses", "1", "--labelSplit", "2",
             "--labelSplitCore", "5", "--labelFlood", "1", "--labelFloodStep", "4", "--labelMeasure", "--labelShape"]
    for tool, spec in driver.TOOLS.items():
        parser = driver.build_parser(spec)
        for flags in ([], ["--labelMask"], older):
            a = parser.parse_args(["x.tif"] + flags)
            driver.check_label_args(parser, a)
            assert (a.labelHmax, a.labelHmaxPlane, a.labelHmaxInvert, a.labelHmaxCore) == (None, None, False, None), (tool, flags)
        a = parser.parse_args(["x.tif", "--labelMask", "--labelHmax", "40", "--labelHmaxPlane", "1", "--labelHmaxInvert", "--labelHmaxCore", "3",
                               "--labelFlood", "1", "--labelFloodStep", "4", "--labelFloodInvert"])
        driver.check_label_args(parser, a)
        assert (a.labelHmax, a.labelHmaxPlane, a.labelHmaxInvert, a.labelHmaxCore, a.labelFlood, a.labelFloodStep) == (40, 1, True, 3, 1, 4)
        a = parser.parse_args(["x.tif", "--labelMask", "--labelHmax", "255"])
        driver.check_label_args(parser, a)
    lb = umx.Labeler.__new__(umx.Labeler)
    lb._L, lb._lb = _Recorder(), ctypes.c_void_p()
    base = umx._label_options(3, 2, 4, 3, (1,))
    for dev in (False, True):
        tail = "_dev" if dev else ""
        lb._L.calls.clear()
        lb._run_any(0, dev, 3, 5, 5, base, 0, 0, 1, 255)
        lb._run_any(0, dev, 3, 5, 5, base, 0, 2, 5, 9, None, 4, True, None, 1, True, 7)     # a plane, an inversion and a core without a height
        assert lb.hmax_counts() is None and lb.flood_counts() is None
        lb._run_any(0, dev, 3, 5, 5, base, 0, 2, 5, 255, 1, 4, True)
        assert lb.hmax_counts() is None and lb.flood_counts() is not None
        lb._run_any(0, dev, 3, 5, 5, base, 0, 0, 1, 255, 1, 4, True, 40, 0, True, 5)
        assert set(lb.hmax_counts()) == set(ref.COUNTS + ("launches", "recon_launches"))
        assert set(lb.flood_counts()) == set(label_flood_ref.COUNTS + ("launches",)) and set(lb.split_counts()) == set(label_split_ref.COUNTS)
        with pytest.raises(ValueError):
            lb._run_any(0, dev, 3, 5, 5, base, 0, 2, 1, 255, None, 16, False, 40)
        assert [n for n, _ in lb._L.calls] == ["umx_labeler_run" + tail, "umx_labeler_run_split" + tail, "umx_labeler_run_flood" + tail,
                                               "umx_labeler_run_hmax" + tail]
        assert lb._L.calls[0][1] == bytes(base) and lb._L.calls[1][1] == bytes(umx._label_split_options(base, 2, 5, 9))
        assert lb._L.calls[2][1] == bytes(umx._label_split_options(base, 2, 5, 255)) + bytes(np.array([1, 1, 4, 0, 0, 0, 0, 0], "<i4"))
        record = lb._L.calls[3][1]
        assert len(record) == 128 and record == bytes(umx._label_split_options(base, 1, 5, 255)) + bytes(
            np.array([1, 1, 4, 0, 0, 0, 0, 0, 0, 1, 40, 0, 0, 0, 0, 0], "<i4"))
    lb._lb = ctypes.c_void_p()                                                 # (nothing to destroy)


def test_bench_tool_overlapping_discs():
    """tools/bench_label.py --hmax: pairs of discs over a neck that no --split can cut, one dome per disc in the seed plane; the
    h-maxima seeds cut every pair"""
    import importlib.util
    spec = importlib.util.spec_from_file_location("bench_label", os.path.join(ROOT, "tools", "bench_label.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    H, W = 3 * m.DISC_PITCH, 4 * m.DISC_PITCH
    planes = m.disc_planes(H, W)
    assert planes.shape == (3, H, W) and planes.dtype == np.uint8
    n0 = len(label_ref.label(planes, 2, 1)[1])
    assert n0 == 12 and label_split_ref.split(planes, 2, 1, 8)[2]["n_objects"] == n0      # the neck is wider than 2 * 8
    labels, table, counts = ref.hmax(planes, 2, 1, m.DISC_H, 1)
    assert counts["n_objects"] == 2 * n0 and counts["n_cored"] == n0 and counts["unreached"] == 0
