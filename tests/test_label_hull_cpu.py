"""CPU checks of the label mask's hulls: the Python restatement against Qhull
(scipy.spatial.ConvexHull over all pixel corners) and against its own hull of all corners, the identities of the record,
umx.hull_descriptors against values known on paper and against an exact-rational least width, the records' sizes, the host-only limits
of umx_label_hull_check, the UMX_HULL_ macros, the two CSV writers, the drivers' refusals, and the host arithmetic of the library
(limits, the limit on E, buffer sizes) as a stand-alone program under the host sanitizers.  No kernel runs here:
tests/test_gpu_label_hull.py holds the device to the restatement."""
import ctypes
import math
import os
import re
import shutil
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import helpers
import label_hull_ref as ref
from unmicst_amd import build, driver, model, umx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    build.build()
    return umx.load()


def seeded_masks(count, seed=11):
    """bool masks with sides 1..40 at seeded densities, none empty"""
    rng = np.random.default_rng(seed)
    for _ in range(count):
        H, W = (int(v) for v in rng.integers(1, 41, 2))
        m = rng.random((H, W)) < rng.random() ** 2
        m[int(rng.integers(0, H)), int(rng.integers(0, W))] = True
        yield m


def test_restatement_against_qhull_and_the_all_corners_hull():
    """Qhull on every corner of every pixel: the area within a relative 1e-9 -- four orders above float64 rounding of a few hundred
    terms, two below the 1e-7 one wrong lattice step makes on a plane of side up to 2048 -- and the same vertex count; the hull of
    the boundary pixels' corners is the hull of all corners, vertex for vertex."""
    from scipy.spatial import ConvexHull
    seen = 0
    for m in seeded_masks(300):
        hull = ref.hull_of_mask(m)
        assert hull == ref.hull_of_mask(m, corners=ref.all_corners)
        q = ConvexHull(np.array(ref.all_corners(m), np.float64))
        assert abs(q.volume - ref.area2_of(hull) / 2) <= 1e-9 * q.volume, m.shape     # (in two dimensions Qhull's volume is the area)
        assert len(q.vertices) == len(hull), m.shape
        assert sorted(map(tuple, q.points[q.vertices].astype(int).tolist())) == sorted(hull)
        seen += len(hull)
    assert seen > 1500


def test_identities_of_the_records():
    for name, labels, N in ref.hand_made():
        rec, verts = ref.hulls(labels, N)
        assert rec.dtype == ref.RECORD and verts.dtype == ref.VERTEX and len(rec) == N, name
        n = rec["n_vertices"].astype(np.int64)
        assert np.array_equal(rec["first"], np.cumsum(n) - n) and n.sum() == len(verts), name        # first: the running sum
        area = np.bincount(ref.clean(labels, N).ravel(), minlength=N + 1)[1:]
        assert (2 * area <= rec["area2"]).all() and ((n == 0) == (area == 0)).all(), name
        assert (n <= 2 * rec["rows"] + 2).all() and (n[area > 0] >= 4).all(), name
        for j in np.flatnonzero(n):
            v = verts[rec["first"][j]:rec["first"][j] + n[j]]
            pts = list(zip(v["y"].tolist(), v["x"].tolist()))
            assert pts[0] == min(pts) and pts[1][0] == pts[0][0] and pts[1][1] > pts[0][1], name     # the canonical start, the top edge
            assert ref.area2_of(pts) == rec["area2"][j] > 0, name                                  # ... and direction
            assert all(ref.cross(pts[i - 1], pts[i], pts[(i + 1) % len(pts)]) > 0 for i in range(len(pts))), name   # strictly convex
    by_name = {name: (labels, N) for name, labels, N in ref.hand_made()}
    for name in ("full plane", "one pixel"):                        # solidity 1 exactly for rectangles
        labels, N = by_name[name]
        rec, verts = ref.hulls(labels, N)
        assert rec["area2"][0] == 2 * int((labels == 1).sum()) and rec["n_vertices"][0] == 4
    for name in ("staircase of two", "lens", "tall lens"):          # the bound on the vertices, attained
        rec, _ = ref.hulls(*by_name[name])
        assert rec["n_vertices"][0] == 2 * rec["rows"][0] + 2, name
    rec, _ = ref.hulls(*by_name["staircase"])                       # collinear corners are dropped: a hexagon
    assert rec["n_vertices"][0] == 6 and rec["rows"][0] == 9 and rec["area2"][0] == 2 * 9 + 2 * 8
    rec, _ = ref.hulls(*by_name["a label without pixels"])
    assert rec[1].tolist() == (0, 0, 4, 0, 0)
    rec, _ = ref.hulls(*by_name["far-apart pieces"])
    assert rec["rows"][0] == 9 and rec["n_vertices"][0] == 6


def exact_feret_min_sq(pts):
    """the least width squared as a Fraction: every edge against every vertex, no numpy"""
    n = len(pts)
    best = None
    for i in range(n):
        a, b = pts[i], pts[(i + 1) % n]
        widest = max(abs(ref.cross(a, b, p)) for p in pts)
        w = Fraction(widest * widest, (b[0] - a[0]) ** 2 + (b[1] - a[1]) ** 2)
        best = w if best is None or w < best else best
    return best


def descriptors_of(labels, N):
    rec, verts = ref.hulls(labels, N)
    area = np.bincount(ref.clean(labels, N).ravel(), minlength=N + 1)[1:]
    return rec, verts, umx.hull_descriptors(rec, verts, area)


def test_hull_descriptors_against_values_known_on_paper():
    assert umx.HULL_DESCRIPTORS == ("hull_area", "solidity", "feret_max", "feret_min", "hull_perimeter", "n_vertices")
    _, _, d = descriptors_of(np.ones((1, 1), np.int32), 1)          # the unit square
    assert tuple(d) == umx.HULL_DESCRIPTORS
    assert [d[n][0] for n in umx.HULL_DESCRIPTORS] == [1.0, 1.0, math.sqrt(2.0), 1.0, 4.0, 4]
    a, b = 3, 7                                                     # an a x b rectangle, off the origin
    lab = np.zeros((6, 12), np.int32)
    lab[2:2 + a, 4:4 + b] = 1
    _, _, d = descriptors_of(lab, 1)
    assert [d[n][0] for n in umx.HULL_DESCRIPTORS] == [21.0, 1.0, math.sqrt(58.0), 3.0, 20.0, 4]
    n = 6                                                           # a right-triangle staircase: row k holds pixels 0..k
    lab = np.tril(np.ones((n, n), np.int32))
    rec, verts, d = descriptors_of(lab, 1)
    # its hull: (0,0) (0,1) (n-1,n) (n,n) (n,0): the triangle of legs n, area n^2 / 2, and along its hypotenuse a strip with the
    # corners (0,0) (0,1) (n-1,n) (n,n), area n - 1/2
    assert list(zip(verts["y"].tolist(), verts["x"].tolist())) == [(0, 0), (0, 1), (n - 1, n), (n, n), (n, 0)]
    assert d["hull_area"][0] == n * n / 2 + n - 0.5 and d["solidity"][0] == (n * (n + 1) / 2) / d["hull_area"][0] < 1.0
    assert d["feret_max"][0] == math.sqrt(2.0 * n * n) and d["n_vertices"][0] == 5
    assert d["hull_perimeter"][0] == ((1.0 + math.hypot(n - 1, n - 1)) + 1.0 + n) + n
    # the least width: from the long diagonal edge (0,1) - (n-1,n) the corner (n,0) is (n - 1) (n + 1) / sqrt(2 (n - 1)^2) away,
    # less than the n of the four axis-parallel edges
    assert d["feret_min"][0] == math.sqrt((n + 1) ** 2 / 2)
    _, _, d = descriptors_of(*[c[1:] for c in ref.hand_made() if c[0] == "a label without pixels"][0])
    assert [d[n][1] for n in umx.HULL_DESCRIPTORS] == [0.0, 0.0, 0.0, 0.0, 0.0, 0]
    assert d["n_vertices"].dtype == np.int64 and all(d[n].dtype == np.float64 for n in umx.HULL_DESCRIPTORS[:-1])
    with pytest.raises(ValueError):
        umx.hull_descriptors(rec, verts[:-1], [21])
    with pytest.raises(ValueError):
        umx.hull_descriptors(rec, verts, [21, 3])


def test_feret_min_is_the_exact_rational_rounded_once():
    seen = 0
    cases = [(labels, N) for _, labels, N in ref.hand_made()] + [(m.astype(np.int32), 1) for m in seeded_masks(40, seed=5)] + [(ref.disc(11), 1)]
    for labels, N in cases:
        rec, verts, d = descriptors_of(labels, N)
        for j in np.flatnonzero(rec["n_vertices"]):
            v = verts[rec["first"][j]:rec["first"][j] + rec["n_vertices"][j]]
            pts = list(zip(v["y"].tolist(), v["x"].tolist()))
            w = exact_feret_min_sq(pts)
            assert Fraction(*umx.hull_feret_min_sq(v["y"], v["x"])) == w
            assert d["feret_min"][j] == math.sqrt(w.numerator / w.denominator)
            assert d["feret_min"][j] <= d["feret_max"][j] and d["solidity"][j] <= 1.0
            assert d["hull_perimeter"][j] == pytest.approx(sum(math.dist(pts[i], pts[(i + 1) % len(pts)]) for i in range(len(pts))), rel=1e-12)
            seen += 1
    assert seen > 50
    big = np.array([(0, 0), (0, 65536), (65536, 65536), (65536, 0)], umx.LABEL_HULL_VERTEX_DTYPE)   # cross products of 2^32, squared 2^64
    assert umx.hull_feret_min_sq(big["y"], big["x"]) == (2 ** 64, 2 ** 32)


def test_discs_read_lower_than_a_pixel_centre_hull():
    """the figures DESIGN.md quotes for the pixel-square convention"""
    for r, vertices, solidity in ((5, 16, 0.853), (11, 24, 0.926), (100, 72, 0.990)):
        rec, verts, d = descriptors_of(ref.disc(r), 1)
        assert rec["n_vertices"][0] == vertices and round(float(d["solidity"][0]), 3) == solidity, r


def test_limits(lib):
    ok = umx.label_hull_check
    assert ok(1, 1) == "" and ok(65536, 8, 2 ** 31 - 1) == "" and ok(4, 65536) == "" and ok(46340, 46340) == "" and ok(32767, 65536) == ""
    assert "at least 1" in ok(0, 5) and "at least 1" in ok(5, 0) and "at least 1" in ok(-1, 5)
    assert "65536" in ok(65537, 1) and "65536" in ok(1, 65537) and "at most 65536" in ok(1, 70000)
    assert "flat pixel index" in ok(32768, 65536) and "flat pixel index" in ok(46341, 46341) and "flat pixel index" in ok(65536, 65536)
    assert "n_objects" in ok(4, 4, -1) and "n_objects" in ok(4, 4, 2 ** 31) and ok(4, 4, 2 ** 31 - 1) == ""
    assert lib.umx_label_hull_check(0, 0, 0, None, 0) == umx.ERR_INVALID and lib.umx_label_hull_check(1, 1, 0, None, 0) == 0
    buf = ctypes.create_string_buffer(8)
    assert lib.umx_label_hull_check(0, 0, 0, buf, 8) == umx.ERR_INVALID and len(buf.value) == 7


def test_binding_mirrors_the_header(lib):
    header = open(os.path.join(ROOT, "include", "umx.h")).read()
    ctype = {"int32_t": ctypes.c_int32, "uint32_t": ctypes.c_uint32, "int64_t": ctypes.c_int64}
    for struct, size, dtype, binding, restated in (("umx_label_hull", 32, umx.LABEL_HULL_DTYPE, umx.LabelHull, ref.RECORD),
                                                   ("umx_label_hull_vertex", 8, umx.LABEL_HULL_VERTEX_DTYPE, umx.LabelHullVertex, ref.VERTEX)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;\s*/\* %d bytes \*/" % (struct, struct, size), header, re.S).group(1)
        fields = [(t, n.strip()) for t, decl in re.findall(r"(u?int\d+_t) ([\w, ]+);", body) for n in decl.split(",")]
        assert dtype == restated and dtype.itemsize == size == ctypes.sizeof(binding), struct
        assert tuple(n for _, n in fields) == dtype.names == tuple(n for n, _ in binding._fields_), struct

        class Record(ctypes.Structure):                              # the header's record, field by field
            _fields_ = [(n, ctype[t]) for t, n in fields]
        assert ctypes.sizeof(Record) == size
        for name, _ in Record._fields_:
            assert getattr(Record, name).offset == dtype.fields[name][1] == getattr(binding, name).offset, (struct, name)
    macros = {k: int(v) for k, v in re.findall(r"#define (UMX_HULL_\w+) (\d+)", header)}
    assert macros == {"UMX_HULL_MAX_SIDE": umx.HULL_MAX_SIDE, "UMX_HULL_MAX_ROWS": umx.HULL_MAX_ROWS}
    assert set(re.findall(r"UMX_HULL_\w+", header)) == set(macros)                    # no enumerator, no stray name
    assert umx.HULL_MAX_ROWS == 2 ** 28 and umx.HULL_MAX_SIDE == 65536 == umx.SHAPE_MAX_SIDE
    raw = ctypes.CDLL(build.lib_path())
    for name in ("umx_label_hull_check", "umx_labeler_hull", "umx_labeler_hull_dev", "umx_labeler_hull_last_ms"):
        assert hasattr(raw, name) and name in umx.EXPORTS


def test_hull_csv_writers(tmp_path):
    labels, N = ref.many_small(4, 5)
    labels[0:3, 0:5] = 1                                             # a full rectangle among them
    rec, verts, d = descriptors_of(labels, N)
    objects = np.zeros(N, [("area", "<i4")])
    objects["area"] = np.bincount(labels.ravel(), minlength=N + 1)[1:]
    p = str(tmp_path / "h.csv")
    driver.write_hulls_csv(p, objects, rec, verts)
    lines = open(p).read().splitlines()
    assert lines[0] == "label,hull_area,solidity,feret_max,feret_min,hull_perimeter,n_vertices" == ",".join(driver.HULL_COLUMNS)
    assert len(lines) == N + 1 == 21
    for j, line in enumerate(lines[1:]):
        f = line.split(",")
        assert int(f[0]) == j + 1 and int(f[6]) == rec["n_vertices"][j]
        assert f[1:6] == [repr(float(d[n][j])) for n in driver.HULL_COLUMNS[1:6]]
        assert [float(v) for v in f[1:6]] == [float(d[n][j]) for n in driver.HULL_COLUMNS[1:6]]     # repr reads back to the same float64
    assert lines[1] == "1,15.0,1.0,%r,3.0,16.0,4" % math.sqrt(34.0)
    p = str(tmp_path / "v.csv")
    driver.write_hull_vertices_csv(p, rec, verts)
    lines = open(p).read().splitlines()
    assert lines[0] == "label,index,y,x" == ",".join(driver.HULL_VERTEX_COLUMNS) and len(lines) == len(verts) + 1
    rows = [tuple(int(v) for v in line.split(",")) for line in lines[1:]]
    assert rows[:4] == [(1, 0, 0, 0), (1, 1, 0, 5), (1, 2, 3, 5), (1, 3, 3, 0)]
    want = [(j + 1, i, int(verts["y"][rec["first"][j] + i]), int(verts["x"][rec["first"][j] + i])) for j in range(N) for i in range(rec["n_vertices"][j])]
    assert rows == want
    with pytest.raises(AssertionError):                              # a table of other objects than the hulls'
        driver.write_hulls_csv(p, objects[:-1], rec, verts)
    objects["area"][3] += 40
    with pytest.raises(AssertionError):
        driver.write_hulls_csv(p, objects, rec, verts)
    driver.write_hulls_csv(p, objects[:0], rec[:0], verts[:0])
    assert open(p).read() == ",".join(driver.HULL_COLUMNS) + "\n"
    driver.write_hull_vertices_csv(p, rec[:0], verts[:0])
    assert open(p).read() == "label,index,y,x\n"


def test_driver_refusals(tmp_path, monkeypatch, capsys):
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
    for tool in driver.TOOLS:
        for flags, word in ((["--labelHull"], "--labelHull needs --labelMask"),
                            (["--labelHullVertices"], "--labelHullVertices needs --labelMask"),
                            (["--labelHull", "--labelHullVertices"], "--labelHull needs --labelMask"),
                            (["--labelMask", "--labelHullVertices"], "--labelHullVertices needs --labelHull")):
            with pytest.raises(SystemExit) as e:
                driver.run(tool, [img, "--model", "nucleiDAPI"] + flags)
            assert e.value.code == 2
            assert word in capsys.readouterr().err, (tool, flags)


def test_host_arithmetic_under_the_sanitizers(tmp_path):
    """tools/hull_host_check.cpp -- the limits, the limit on E and the buffer sizes, all of unmicst_amd/csrc/umx_hull_host.h -- built
    as a stand-alone program with ASan and UBSan on the host compiler, and run"""
    cxx = shutil.which("g++") or shutil.which("clang++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "hull_host_check")
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        os.path.join(ROOT, "tools", "hull_host_check.cpp"), "-o", exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "hull-host-ok" in r.stdout, (r.stdout[-1000:], r.stderr[-2000:])


def test_bench_tool_host_route():
    """tools/bench_label.py --hull: its numpy / scipy yardstick gives the restatement's areas and vertex counts on its own blobs"""
    import importlib.util
    from scipy import ndimage
    spec = importlib.util.spec_from_file_location("bench_label", os.path.join(ROOT, "tools", "bench_label.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    labels, N = ndimage.label(bench.blob_mask(96, 160))
    labels = labels.astype(np.int32)
    assert N > 5
    area, count = bench.host_hulls(labels, N)
    rec, _ = ref.hulls(labels, N)
    assert np.array_equal(count, rec["n_vertices"]) and np.allclose(area, rec["area2"] / 2.0, rtol=1e-9, atol=0.0)
