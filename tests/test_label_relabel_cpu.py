"""CPU checks of the label mask's relabel: umx.relabel_map -- the exported host function, a
union-find in C++ -- against the restatement by scipy's connected components at every N round the 2048-label blocks, its three
identities on maps and on numpy planes, umx.relabel_objects against step 4 on the relabelled plane, the limits and every refusal with
the pair's index, the binding against the header, the drivers' rule parser, merge selection and refusals, the host part as a
stand-alone program under the host sanitizers, and the host route of tools/bench_label.py --relabel.  No kernel runs here:
tests/test_gpu_label_relabel.py holds the device to the restatement."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import helpers
import label_relabel_ref as ref
from unmicst_amd import build, driver, model, umx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = (0, 1, 2047, 2048, 2049, 4097)


@pytest.fixture(scope="module")
def lib():
    build.build()
    return umx.load()


def pair_sets(N, keep, seed):
    """name -> pairs that the keep accepts (they name kept labels only): refused inputs are excluded by construction"""
    kept = np.arange(1, N + 1) if keep is None else np.flatnonzero(keep) + 1
    sets = {"none": None, "empty": np.zeros((0, 2), np.int64)}
    if len(kept) >= 1:
        k = kept.astype(np.int64)
        sets["chain of the kept"] = np.stack([k[:-1], k[1:]], 1).reshape(-1, 2)
        sets["star round the last kept"] = np.stack([np.full(len(k), k[-1]), k], 1)          # (its own (a, a) included)
        sets["seeded with (a, a), (b, a) and repeats"] = ref.seeded_pairs(N, max(1, len(k) // 3), seed, among=k)
    return sets


@pytest.mark.parametrize("N", SIZES)
def test_relabel_map_against_the_restatement(lib, N):
    """every N, every keep, every pair set the keep accepts; the pairs shuffled and doubled give the same bytes"""
    seen = 0
    for kname, keep in ref.keeps(N, seed=N).items():
        for pname, pairs in pair_sets(N, keep, seed=N + 1).items():
            want, want_n = ref.relabel_map(N, keep, pairs)
            got, got_n = umx.relabel_map(N, keep, pairs)
            assert got.dtype == np.int32 and got.shape == (N + 1,), (kname, pname)
            assert got_n == want_n and np.array_equal(got, want), (kname, pname, got[:10], want[:10])
            assert got[0] == 0 and got.max(initial=0) == got_n
            firsts = np.unique(got[got > 0], return_index=True)[1]                    # numbered in order of the least member
            assert np.array_equal(firsts, np.sort(firsts)), (kname, pname)
            if pairs is not None and len(pairs):
                rng = np.random.default_rng(3)
                shuffled = np.concatenate([pairs, pairs[::-1, ::-1]])[rng.permutation(2 * len(pairs))]
                again, again_n = umx.relabel_map(N, keep, shuffled)
                assert again_n == got_n and again.tobytes() == got.tobytes(), (kname, pname)
            seen += 1
    assert seen >= (7 * 2 if N == 0 else 20)


def test_the_chain_and_the_star_of_all_labels():
    for N in SIZES[1:]:
        for pairs in (ref.chain(N), ref.chain(N)[::-1], ref.star(N, 1), ref.star(N, N), ref.star(N, (N + 1) // 2)):
            m, n = umx.relabel_map(N, None, pairs)
            assert n == 1 and m[0] == 0 and (m[1:] == 1).all(), N
            assert np.array_equal(m, ref.relabel_map(N, None, pairs)[0])


def seeded_plane(N, seed, shape=(37, 91)):
    return np.random.default_rng(seed).integers(0, N + 1, shape).astype(np.int32)


def test_identities_on_maps_and_planes():
    for N in (1, 5, 2049):
        labels = seeded_plane(N, N)
        ident, n = umx.relabel_map(N, np.ones(N, np.uint8), None)                     # keep all, no pair: the identity
        assert n == N and np.array_equal(ident, np.arange(N + 1)) and np.array_equal(ref.apply(labels, N, ident), labels)
        table = ref.table_of(labels, N)
        assert umx.relabel_objects(table, ident).tobytes() == table.tobytes()
        rng = np.random.default_rng(N)
        for _ in range(4):                                                            # relabel(k2) o relabel(k1) = relabel(k1 & k2[map1])
            k1 = rng.random(N) < 0.7
            m1, n1 = umx.relabel_map(N, k1)
            k2 = rng.random(n1) < 0.5
            m2, n2 = umx.relabel_map(n1, k2)
            through = np.concatenate([[False], k2])[m1[1:]]                           # k2[map1], False where map1 is 0
            m12, n12 = umx.relabel_map(N, k1 & through)
            assert n12 == n2 and np.array_equal(m2[m1], m12)
            assert np.array_equal(ref.apply(ref.apply(labels, N, m1), n1, m2), ref.apply(labels, N, m12))
            assert umx.relabel_objects(umx.relabel_objects(table, m1), m2).tobytes() == umx.relabel_objects(table, m12).tobytes()


def test_relabel_objects_is_step_4_on_the_new_plane():
    seen = 0
    for N in (1, 7, 300):
        labels = seeded_plane(N, 10 + N)
        if N == 300:
            labels[labels == 17] = 0                                                  # a label no pixel carries, merged and alone
            labels[labels == 250] = 0
        table = ref.table_of(labels, N)
        for kname, keep in ref.keeps(N, seed=2).items():
            for pname, pairs in pair_sets(N, keep, seed=4).items():
                new, want, m = ref.relabel(labels, N, keep, pairs)
                got = umx.relabel_objects(table, umx.relabel_map(N, keep, pairs)[0])
                assert got.dtype == umx.LABEL_OBJECT_DTYPE and got.shape == want.shape, (N, kname, pname)
                for f in umx.LABEL_OBJECT_DTYPE.names:
                    assert np.array_equal(got[f], want[f]), (N, kname, pname, f)
                seen += 1
    assert seen > 50
    empty = umx.relabel_objects(ref.table_of(np.zeros((3, 3), np.int32), 2), np.array([0, 1, 1], np.int32))
    assert empty.tolist() == [(0, ref.INT_MAX, ref.INT_MAX, -1, -1, 0, 0, 0)]
    with pytest.raises(ValueError):
        umx.relabel_objects(table, np.zeros(3, np.int32))
    bad = labels.copy()
    bad[0, 0], bad[1, 1], bad[2, 2] = -5, N + 1, 2 ** 31 - 1                          # outside 0..N: they count as 0
    assert np.array_equal(ref.apply(bad, N, np.arange(N + 1)), np.where((bad < 0) | (bad > N), 0, bad))


def refused(call, *words):
    with pytest.raises(umx.UmxError) as e:
        call()
    assert e.value.code == umx.ERR_INVALID and all(w in str(e.value) for w in words), str(e.value)


def test_limits_and_refusals(lib):
    ok = umx.label_relabel_check
    assert ok(1, 1) == "" and ok(32767, 65536, 2 ** 31 - 2, umx.RELABEL_MAX_PAIRS) == "" and ok(1, 2 ** 31 - 1) == "" and ok(46340, 46340) == ""
    assert "at least 1" in ok(0, 5) and "at least 1" in ok(5, 0) and "at least 1" in ok(-1, 5)
    assert "flat pixel index" in ok(32768, 65536) and "flat pixel index" in ok(46341, 46341)
    assert "n_objects" in ok(4, 4, -1) and "n_objects" in ok(4, 4, 2 ** 31 - 1) and ok(4, 4, 2 ** 31 - 2) == ""
    assert "n_pairs" in ok(4, 4, 0, -1) and "n_pairs" in ok(4, 4, 0, umx.RELABEL_MAX_PAIRS + 1)
    assert lib.umx_label_relabel_check(0, 0, 0, 0, None, 0) == umx.ERR_INVALID and lib.umx_label_relabel_check(1, 1, 0, 0, None, 0) == 0
    buf = ctypes.create_string_buffer(8)
    assert lib.umx_label_relabel_check(0, 0, 0, 0, buf, 8) == umx.ERR_INVALID and len(buf.value) == 7
    # the pairs: outside 1..N, and naming a dropped label, at every position of the list
    N = 40
    keep = np.ones(N, np.uint8)
    keep[9] = 0
    good = ref.chain(N)[20:30]
    for bad in ((0, 5), (5, 0), (-1, 5), (5, N + 1), (2 ** 31 - 1, 5), (10, 5), (5, 10), (10, 10)):
        for at in range(len(good) + 1):
            pairs = np.concatenate([good[:at], [bad], good[at:]])
            refused(lambda: umx.relabel_map(N, keep, pairs), "pair %d is (%d, %d)" % (at, bad[0], bad[1]))
            with pytest.raises(ValueError):
                ref.relabel_map(N, keep, pairs)
    refused(lambda: umx.relabel_map(N, keep, [[5, 10]]), "keep drops label 10")
    assert umx.relabel_map(N, None, [[5, 10]])[1] == N - 1                            # without the keep the same pair is fine
    refused(lambda: umx.relabel_map(N, keep[:-1]), "keep has 39 entries")
    refused(lambda: umx.relabel_map(N, None, [[1, 2, 3]]), "[M, 2]")
    refused(lambda: umx.relabel_map(N, None, [[1, 2 ** 40]]), "int32")
    refused(lambda: umx.relabel_map(N, None, [[1.5, 2.0]]), "integers")
    refused(lambda: umx.relabel_map(-1), "n_objects")
    refused(lambda: umx.relabel_map(2 ** 31 - 1), "n_objects")
    # the C entry itself: validation only with a null map, at the largest N; null pairs with a count; the message cut to its buffer
    p = np.array([[1, 2 ** 31 - 2], [2 ** 31 - 2, 7]], np.int32)
    n = ctypes.c_int64(-5)
    msg = ctypes.create_string_buffer(256)
    call = lib.umx_label_relabel_map
    assert call(2 ** 31 - 2, None, p.ctypes.data, 2, None, ctypes.byref(n), msg, 256) == 0 and n.value == -5 and msg.value == b""
    p[1, 0] = 2 ** 31 - 1
    assert call(2 ** 31 - 2, None, p.ctypes.data, 2, None, None, msg, 256) == umx.ERR_INVALID and b"pair 1 is" in msg.value
    assert call(5, None, None, 2, None, None, msg, 256) == umx.ERR_INVALID and b"null" in msg.value
    assert call(5, None, p.ctypes.data, 1, None, None, None, 0) == umx.ERR_INVALID
    assert call(5, None, p.ctypes.data, 1, None, None, buf, 8) == umx.ERR_INVALID and len(buf.value) == 7


def test_binding_mirrors_the_header(lib):
    header = open(os.path.join(ROOT, "include", "umx.h")).read()
    macros = {k: int(v) for k, v in re.findall(r"#define (UMX_RELABEL_\w+) (\d+)", header)}
    assert macros == {"UMX_RELABEL_MAX_PAIRS": umx.RELABEL_MAX_PAIRS}
    assert set(re.findall(r"UMX_RELABEL_\w+", header)) == set(macros)                  # no enumerator, no stray name
    assert umx.RELABEL_MAX_PAIRS == umx.CONTACT_TABLE_MAX == 2 ** 28
    raw = ctypes.CDLL(build.lib_path())
    names = ("umx_label_relabel_check", "umx_label_relabel_map", "umx_labeler_relabel", "umx_labeler_relabel_dev", "umx_labeler_relabel_last_ms")
    for name in names:
        assert hasattr(raw, name) and name in umx.EXPORTS
        decl = re.search(r"UMX_API int %s\((.*?)\);" % name, header, re.S).group(1)
        params = [p for p in re.sub(r"/\*.*?\*/", "", decl, flags=re.S).split(",") if p.strip()]
        assert len(params) == len(getattr(lib, name).argtypes), name                   # the binding passes as many arguments
    host = open(os.path.join(ROOT, "unmicst_amd", "csrc", "umx_relabel_host.h")).read()
    assert "hip/" not in host and "__global__" not in host and "__device__" not in host   # plain C++: no HIP in the host part


def test_keep_rules_on_a_hand_made_table():
    parse = driver.parse_keep_rule
    assert parse("area>=30") == ("area", ">=", 30.0, "objects") and parse("border==0") == ("border", "==", 0.0, "objects")
    assert parse("solidity<0.9") == ("solidity", "<", 0.9, "hull") and parse("eccentricity<=1e-1") == ("eccentricity", "<=", 0.1, "shape")
    assert parse("pm2_mean>=128") == ("pm2_mean", ">=", 128.0, ("pm", 2)) and parse("ch11_max!=-3.5") == ("ch11_max", "!=", -3.5, ("ch", 11))
    assert parse("n_vertices>4")[3] == "hull" and parse("perimeter_edges>4")[3] == "shape" and parse("extent>.5")[3] == "shape"
    for bad in ("", "area", "area>", ">=3", "area=>3", "area>=x", "area >= 3", "area>=3 ", "area>=nan", "area>=inf", "label>=3", "pm_mean>1",
                "pm2_median>1", "ch-1_mean>1", "volume>=3", "area>==3", "area>=3>=4"):
        with pytest.raises(ValueError):
            parse(bad)
    assert driver.keep_rule_refusal([parse("pm2_mean>1"), parse("ch0_min>1")], 3, 1) == ""
    assert "planes 0..2" in driver.keep_rule_refusal([parse("pm3_mean>1")], 3, 1)
    assert "pages 0..0" in driver.keep_rule_refusal([parse("area>1"), parse("ch1_min>1")], 3, 1)
    assert "TIFF" in driver.keep_rule_refusal([parse("ch0_min>1")], 3, None)
    # a table of five objects on 20 x 30: the second touches the top, the fourth the right border
    objects = np.zeros(5, umx.LABEL_OBJECT_DTYPE)
    objects["area"] = [10, 30, 29, 500, 31]
    objects["y0"], objects["x0"], objects["y1"], objects["x1"] = [3, 0, 5, 2, 9], [3, 8, 1, 20, 5], [4, 2, 7, 18, 12], [6, 12, 9, 29, 9]
    cols = driver.object_columns(objects, (20, 30))
    assert cols["border"].tolist() == [0, 1, 0, 1, 0]
    cols["pm2_mean"] = np.array([127.999999, 128.0, np.nan, 200.0, 128.000001])
    mask = lambda *rules: driver.keep_mask([parse(r) for r in rules], cols).tolist()   # noqa: E731
    assert mask("area>=30") == [0, 1, 0, 1, 1] and mask("area>30") == [0, 0, 0, 1, 1] and mask("area<=30", "area!=29") == [1, 1, 0, 0, 0]
    assert mask("area>=30", "border==0") == [0, 0, 0, 0, 1] and mask("border!=0") == [0, 1, 0, 1, 0]
    assert mask("pm2_mean>=128") == [0, 1, 0, 1, 1] and mask("pm2_mean<128") == [1, 0, 0, 0, 0] and mask("pm2_mean!=128") == [1, 0, 1, 1, 1]
    assert mask("area<5000", "area>=30", "border==0", "pm2_mean>=128") == [0, 0, 0, 0, 1]
    assert driver.keep_mask([parse("area>=30")], cols).dtype == np.uint8
    # the columns the writers print from are the ones the rules read
    planes = [("pm0", np.zeros(5, umx.LABEL_MEASURE_DTYPE))]
    planes[0][1]["count"], planes[0][1]["sum"], planes[0][1]["sum_sq"] = objects["area"], 2 * objects["area"], 4 * objects["area"]
    ic = driver.intensity_columns(objects, planes)
    assert sorted(ic) == ["pm0_max", "pm0_mean", "pm0_min", "pm0_std"] and ic["pm0_mean"].tolist() == [2.0] * 5 and ic["pm0_std"].tolist() == [0.0] * 5
    planes[0][1]["count"][2] += 1
    with pytest.raises(AssertionError):
        driver.intensity_columns(objects, planes)


def test_merge_selection_on_a_hand_made_table():
    contacts = np.zeros(4, umx.LABEL_CONTACT_DTYPE)
    contacts["a"], contacts["b"], contacts["edges"] = [1, 1, 2, 4], [2, 3, 3, 5], [5, 4, 10, 1]
    perimeter_edges = np.array([10, 20, 40, 3, 2])
    pairs = driver.merge_pairs(contacts, perimeter_edges, 0.5)
    assert pairs.dtype == np.int32 and pairs.tolist() == [[1, 2], [2, 3], [4, 5]]      # 5 >= 5, 4 < 5, 10 >= 10, 1 >= 1
    assert driver.merge_pairs(contacts, perimeter_edges, 0.51).tolist() == []
    assert driver.merge_pairs(contacts, perimeter_edges, 0.4).tolist() == [[1, 2], [1, 3], [2, 3], [4, 5]]
    assert driver.merge_pairs(contacts, perimeter_edges, 1.0).tolist() == []
    assert driver.merge_pairs(contacts[:0], perimeter_edges, 0.5).shape == (0, 2)
    m, n = umx.relabel_map(5, None, pairs)                                             # the closure of the qualifying pairs
    assert n == 2 and m.tolist() == [0, 1, 1, 1, 2, 2]


def test_driver_refusals_before_any_file(tmp_path, monkeypatch, capsys):
    hp, blob, mean, std = helpers.load_nuclei_dapi()
    models = tmp_path / "models"
    model.save_converted(model.ModelArtefacts(hp, blob, mean, std), str(models / "nucleiDAPI"))
    monkeypatch.setenv("UMX_MODELS_DIR", str(models))

    def no_engine(*a, **k):
        raise AssertionError("the engine was set up before the label flags were checked")
    monkeypatch.setattr(umx, "Engine", no_engine)
    from unmicst_amd import tiffio
    os.makedirs(tmp_path / "x" / "registration")
    img = str(tmp_path / "x" / "registration" / "one.tif")
    tiffio.imsave(img, np.zeros((5, 7), np.uint16))
    before = sorted(os.path.join(r, f) for r, _, fs in os.walk(tmp_path / "x") for f in fs)
    K = hp.nClasses
    cases = ((["--labelKeep", "area>=30"], "--labelKeep needs --labelMask"),
             (["--labelMerge", "0.5"], "--labelMerge needs --labelMask"),
             (["--labelMask", "--labelMerge", "0"], "--labelMerge 0.0"),
             (["--labelMask", "--labelMerge", "1.5"], "--labelMerge 1.5"),
             (["--labelMask", "--labelMerge", "nan"], "--labelMerge nan"),
             (["--labelMask", "--labelKeep", "area>=30", "volume>3"], "'volume'"),
             (["--labelMask", "--labelKeep", "area=30"], "NAME OP VALUE"),
             (["--labelMask", "--labelKeep", "area>=thirty"], "is no number"),
             (["--labelMask", "--labelKeep", "pm%d_mean>=1" % K], "the model has planes 0..%d" % (K - 1)),
             (["--labelMask", "--labelKeep", "ch1_mean>=1"], "the file has pages 0..0"),
             (["--labelMask", "--labelMeasure", "0", "--labelKeep", "ch0_mean>=1", "ch7_max<3"], "ch7_max"))
    for tool in driver.TOOLS:
        for flags, word in cases:
            with pytest.raises(SystemExit) as e:
                driver.run(tool, [img, "--model", "nucleiDAPI"] + flags)
            assert e.value.code == 2
            assert word in capsys.readouterr().err, (tool, flags)
    assert sorted(os.path.join(r, f) for r, _, fs in os.walk(tmp_path / "x") for f in fs) == before   # no file was created


def test_host_part_under_the_sanitizers(tmp_path):
    """tools/relabel_host_check.cpp -- the limits, the validation and the union-find of unmicst_amd/csrc/umx_relabel_host.h -- built as
    a stand-alone program with ASan and UBSan on the host compiler, and run"""
    cxx = shutil.which("g++") or shutil.which("clang++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "relabel_host_check")
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        os.path.join(ROOT, "tools", "relabel_host_check.cpp"), "-o", exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "relabel-host-ok" in r.stdout, (r.stdout[-1000:], r.stderr[-2000:])


def test_bench_tool_host_route():
    """tools/bench_label.py --relabel: its host route gives the restatement's plane, map and count on its own blobs"""
    import importlib.util
    from scipy import ndimage
    spec = importlib.util.spec_from_file_location("bench_label", os.path.join(ROOT, "tools", "bench_label.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    labels, N = ndimage.label(bench.blob_mask(96, 160))
    labels = labels.astype(np.int32)
    assert N > 5
    keep = bench.relabel_keep(N)
    assert 0 < keep.sum() < N and np.array_equal(keep, bench.relabel_keep(N))          # seeded, and it drops some
    got, m, n_new, map_s, numpy_s = bench.host_relabel(labels, N, keep)
    want, _, want_m = ref.relabel(labels, N, keep)
    assert n_new == int(keep.sum()) and np.array_equal(m, want_m) and np.array_equal(got, want) and map_s >= 0.0 and numpy_s >= 0.0
