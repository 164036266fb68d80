"""CPU checks of the label mask's shapes: the integer identities of step 17 on the numpy /
scipy restatement, umx.shape_descriptors on closed forms and against a float64 np.cov route, the Shapes file, the host-only limits of
umx_label_shape_check, the record's size and the drivers' flag refusal.  No kernel runs here: tests/test_gpu_label_shape.py holds the
device to the restatement."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

import helpers
import label_shape_ref as ref
from unmicst_amd import build, driver, model, umx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    build.build()
    return umx.load()


def identities(labels, N, what, connected=False):
    """step 17 on the restatement: three counts made in three different ways agree"""
    rec, edges, holes, area = ref.shapes(labels, N)
    q1, q2, qd, q3, q4 = (rec[n].astype(np.int64) for n in ref.QUADS)
    assert np.array_equal(q1 + 2 * q2 + 2 * qd + 3 * q3 + 4 * q4, 4 * area), what
    assert np.array_equal(q1 + q2 + 2 * qd + q3, edges), what
    assert not ((q1 - q3 + 2 * qd) % 4).any(), what
    euler = (q1 - q3 + 2 * qd) // 4
    if connected:
        assert np.array_equal((1 - euler)[area > 0], holes[area > 0]), what
    return rec, euler, holes, area


@pytest.mark.parametrize("density", [0.1, 0.35, 0.6, 0.85])
def test_identities_on_random_masks(density):
    """random masks, each 4-connected component an object (scipy's labelling): area, edges and holes from the window counts"""
    from scipy import ndimage
    rng = np.random.default_rng(int(density * 100))
    seen = 0
    for H, W in ((17, 23), (40, 31), (1, 50), (33, 1)):
        labels, N = ndimage.label(rng.random((H, W)) < density)
        identities(labels.astype(np.int32), N, (density, H, W), connected=True)
        seen += N
        several = rng.integers(-1, 6, (H, W)).astype(np.int32)       # labels that are not connected, next to each other
        identities(several, 4, (density, H, W, "several"))
    assert seen > 8                                                   # (a dense mask has few, large objects with many holes)


def test_identities_and_euler_numbers_of_the_hand_made_cases():
    for name, labels, N, euler_known in ref.hand_made():
        rec, euler, holes, area = identities(labels, N, name)
        assert len(rec) == N
        for j, e in euler_known.items():
            assert euler[j - 1] == e, (name, j)
    lab, N = ref.seeded_labels(9, 200)
    identities(lab, N, "seeded")
    assert (np.bincount(lab.ravel(), minlength=N + 1)[1:] > 0).all()


def test_python_integer_moments_equal_the_bincount_route():
    lab, N = ref.seeded_labels(5, 129)
    assert ref.shapes(lab, N, exact=True)[0].tobytes() == ref.shapes(lab, N, exact=False)[0].tobytes()


def one_object(mask):
    mask = np.asarray(mask)
    return ref.records(mask.astype(np.int32), 1)


def test_descriptors_of_closed_forms():
    for h, w, y0, x0 in ((1, 1, 0, 0), (3, 7, 2, 5), (12, 5, 0, 0), (9, 9, 40, 3), (1, 30, 7, 7)):
        m = np.zeros((y0 + h + 2, x0 + w + 3), bool)
        m[y0:y0 + h, x0:x0 + w] = True
        d = umx.shape_descriptors(one_object(m))
        assert d["area"][0] == h * w and d["euler"][0] == 1 and d["holes"][0] == 0 and d["perimeter_edges"][0] == 2 * (h + w)
        assert d["mu_yy"][0] == (h * h - 1) / 12 and d["mu_xx"][0] == (w * w - 1) / 12 and d["mu_yx"][0] == 0.0
        big, small = max(h, w), min(h, w)
        # l1 and l2 come from half +- root, each rounded: l2 = half - root is off by a few 2^-53 of l1, so the minor axis by that times
        # l1 / l2 <= 143 / 2 here and the eccentricity by less; 1e-13 relative holds all three with room.  A zero is exact.
        close = lambda got, want: got == want if want == 0.0 else abs(got - want) <= 1e-13 * want
        assert close(d["major_axis_length"][0], 4.0 * math.sqrt((big * big - 1) / 12))
        assert close(d["minor_axis_length"][0], 4.0 * math.sqrt((small * small - 1) / 12))
        assert close(d["eccentricity"][0], 0.0 if big == 1 else math.sqrt(1.0 - (small * small - 1) / (big * big - 1)))
        assert d["orientation"][0] == (0.0 if h >= w else math.pi / 2)   # along the rows' axis, along the columns'; 0 for a square
    d = umx.shape_descriptors(one_object(np.ones((1, 1), bool)))     # a single pixel
    assert (d["major_axis_length"][0], d["minor_axis_length"][0], d["eccentricity"][0], d["orientation"][0]) == (0.0, 0.0, 0.0, 0.0)
    assert d["perimeter"][0] == 4 / math.sqrt(2.0) and d["perimeter_edges"][0] == 4
    stairs = np.eye(11, dtype=bool)                                  # y = x: the major axis at +45 degrees from the row axis
    assert umx.shape_descriptors(one_object(stairs))["orientation"][0] == math.pi / 4
    assert umx.shape_descriptors(one_object(stairs[::-1]))["orientation"][0] == -math.pi / 4
    d = umx.shape_descriptors(one_object(stairs))
    assert d["minor_axis_length"][0] == 0.0 and d["eccentricity"][0] == 1.0 and d["euler"][0] == 11   # 11 pieces under 4-connectivity
    empty = umx.shape_descriptors(np.zeros(2, umx.LABEL_SHAPE_DTYPE))   # labels no pixel carries
    assert (empty["area"] == 0).all() and (empty["holes"] == 1).all() and np.isnan(empty["major_axis_length"]).all()
    with pytest.raises(ValueError):
        bad = np.zeros(1, umx.LABEL_SHAPE_DTYPE)
        bad["q1"] = 3
        umx.shape_descriptors(bad)


def ellipse(H, W, cy, cx, a, b, theta):
    """pixels inside an ellipse of half axes a >= b whose major axis makes the angle theta with the row (y) axis"""
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    u = (yy - cy) * math.cos(theta) + (xx - cx) * math.sin(theta)
    v = -(yy - cy) * math.sin(theta) + (xx - cx) * math.cos(theta)
    return (u / a) ** 2 + (v / b) ** 2 <= 1.0


def test_descriptors_against_a_float64_covariance_route():
    """The same formulas on np.cov of the pixel coordinates: the two routes differ only in rounding (the integer route is the
    definition), so they agree to a relative 1e-12 on objects whose axes differ by a factor of two -- neither the difference l1 - l2
    nor mu_yy - mu_xx and mu_yx cancels."""
    for k, theta in enumerate((0.3, 1.1, -0.7, 0.5 * math.pi - 0.2, -1.3)):
        m = ellipse(90, 110, 41.3 + k, 52.7 - k, 30.0 + k, 14.0, theta)
        d = umx.shape_descriptors(one_object(m))
        ys, xs = np.nonzero(m)
        cov = np.cov(np.stack([ys, xs]).astype(np.float64), bias=True)
        myy, mxx, myx = cov[0, 0], cov[1, 1], cov[0, 1]
        half, root = (myy + mxx) / 2, math.sqrt(((myy - mxx) / 2) ** 2 + myx * myx)
        want = {"mu_yy": myy, "mu_xx": mxx, "mu_yx": myx, "major_axis_length": 4 * math.sqrt(half + root),
                "minor_axis_length": 4 * math.sqrt(half - root), "eccentricity": math.sqrt(1 - (half - root) / (half + root)),
                "orientation": 0.5 * math.atan2(2 * myx, myy - mxx)}
        for name, w in want.items():
            assert abs(d[name][0] - w) <= 1e-12 * abs(w), (theta, name, d[name][0], w)
        fold = lambda a: (a + math.pi / 2) % math.pi - math.pi / 2   # an axis has no direction
        assert abs(fold(d["orientation"][0] - theta)) < 0.02          # the angle is the one the ellipse was drawn with
        assert abs(d["major_axis_length"][0] - 2 * (30.0 + k)) < 0.5 and abs(d["minor_axis_length"][0] - 28.0) < 0.5


def test_numerators_past_64_bits_are_formed_exactly():
    """one full-width row of 65536 pixels at y = 65535: A * sum_yy is 2^16 * 2^16 * (2^16 - 1)^2 > 2^63; the variance along y is 0
    exactly, which a rounded numerator would not give"""
    W, y = 65536, 65535
    rec = np.zeros(1, umx.LABEL_SHAPE_DTYPE)
    rec["sum_y"], rec["sum_x"] = y * W, W * (W - 1) // 2
    rec["sum_yy"], rec["sum_xy"], rec["sum_xx"] = y * y * W, y * (W * (W - 1) // 2), (W - 1) * W * (2 * W - 1) // 6
    rec["q1"], rec["q2"] = 4, 2 * (W - 1)
    assert W * int(rec["sum_yy"][0]) > 2 ** 63
    d = umx.shape_descriptors(rec)
    assert d["area"][0] == W and d["mu_yy"][0] == 0.0 and d["mu_yx"][0] == 0.0 and d["mu_xx"][0] == (W * W - 1) / 12
    assert d["orientation"][0] == math.pi / 2 and d["eccentricity"][0] == 1.0


def test_shape_check_accepts_and_refuses_each_limit(lib):
    ok = umx.label_shape_check
    assert ok(1, 1, 0) == "" and ok(150, 203, 7) == ""
    assert ok(65536, 8, 1) == "" and ok(8, 65536, 1) == ""
    assert "65536" in ok(65537, 8, 1) and "65536" in ok(8, 65537, 1)
    assert ok(65536, 32767, 1) == "" and ok(32767, 65536, 1) == ""   # H * W = 2^31 - 2^16
    assert "int32" in ok(65536, 32768, 1) and "int32" in ok(46341, 46341, 1)   # H * W = 2^31 and just above it
    assert ok(46340, 46340, 1) == ""
    assert "at least 1" in ok(0, 5, 1) and "at least 1" in ok(5, -1, 1)
    assert "n_objects" in ok(5, 5, -1) and ok(5, 5, 2 ** 31 - 1) == "" and "n_objects" in ok(5, 5, 2 ** 31)
    buf = ctypes.create_string_buffer(10)
    assert lib.umx_label_shape_check(0, 5, 1, buf, 10) == umx.ERR_INVALID and buf.value == b"the image"
    assert lib.umx_label_shape_check(5, 5, 1, None, 0) == 0
    assert lib.umx_label_shape_check(0, 5, 1, None, 0) == umx.ERR_INVALID


def test_limit_of_h_times_w_at_2_31_minus_1(lib):
    """H * W = 2^31 - 1 exactly is prime, so only 1 x (2^31 - 1) has it, and that side is past 65536: the largest product the two limits
    allow together is 65536 x 32767; the product rule alone is held at 2^31 - 1 / 2^31 by the labelling's and the measurement's checks"""
    assert "65536" in umx.label_shape_check(1, 2 ** 31 - 1, 1)
    assert umx.label_measure_check(umx.MEASURE_U8, 1, 1, 2 ** 31 - 1, 1) == ""


def test_binding_mirrors_the_header(lib):
    header = open(os.path.join(ROOT, "include", "umx.h")).read()
    assert umx.LABEL_SHAPE_DTYPE == ref.RECORD and umx.LABEL_SHAPE_DTYPE.itemsize == 64 and ctypes.sizeof(umx.LabelShape) == 64
    body = re.search(r"typedef struct umx_label_shape \{(.*?)\} umx_label_shape;\s*/\* 64 bytes \*/", header, re.S).group(1)
    fields = [(t, n.strip()) for t, decl in re.findall(r"(u?int\d+_t) ([\w, ]+);", body) for n in decl.split(",")]
    assert tuple(n for _, n in fields) == umx.LABEL_SHAPE_DTYPE.names == tuple(n for n, _ in umx.LabelShape._fields_)
    ctype = {"int64_t": ctypes.c_int64, "uint32_t": ctypes.c_uint32}

    class Record(ctypes.Structure):                              # the header's record, field by field
        _fields_ = [(n, ctype[t]) for t, n in fields]
    assert ctypes.sizeof(Record) == 64
    for name, _ in Record._fields_:
        assert getattr(Record, name).offset == umx.LABEL_SHAPE_DTYPE.fields[name][1] == getattr(umx.LabelShape, name).offset, name
    macros = {k: int(v) for k, v in re.findall(r"#define (UMX_SHAPE_\w+) (\d+)", header)}
    assert macros == {"UMX_SHAPE_MAX_SIDE": umx.SHAPE_MAX_SIDE} and umx.SHAPE_MAX_SIDE == 65536
    raw = ctypes.CDLL(build.lib_path())
    for name in ("umx_label_shape_check", "umx_labeler_shape", "umx_labeler_shape_dev", "umx_labeler_shape_last_ms"):
        assert hasattr(raw, name) and name in umx.EXPORTS


def test_shapes_csv(tmp_path):
    """the file is shape_descriptors of the records and the extent of the table's box, the floats written so that they read back bit
    for bit"""
    cases = [c for c in ref.hand_made() if c[0] in ("borders", "edge")]
    for name, labels, N, _ in cases:
        rec, edges, holes, area = ref.shapes(labels, N)
        objects = np.zeros(N, umx.LABEL_OBJECT_DTYPE)
        for j in range(N):
            ys, xs = np.nonzero(labels == j + 1)
            objects[j] = (len(ys), ys.min(), xs.min(), ys.max(), xs.max(), 0, ys.sum(), xs.sum())
        p = str(tmp_path / "s.csv")
        driver.write_shapes_csv(p, objects, rec)
        lines = open(p).read().splitlines()
        assert lines[0] == "label,area,perimeter_edges,perimeter,euler,holes,major_axis_length,minor_axis_length,eccentricity,orientation,extent"
        assert lines[0].split(",") == list(driver.SHAPE_COLUMNS) and len(lines) == N + 1
        d = umx.shape_descriptors(rec)
        for j, line in enumerate(lines[1:]):
            f = line.split(",")
            assert [int(f[k]) for k in (0, 1, 2, 4, 5)] == [j + 1, area[j], edges[j], 1 - holes[j], holes[j]]
            got = [float(f[k]) for k in (3, 6, 7, 8, 9)]
            want = [d[n][j] for n in ("perimeter", "major_axis_length", "minor_axis_length", "eccentricity", "orientation")]
            assert got == want, (name, j)
            box = (objects["y1"][j] - objects["y0"][j] + 1) * (objects["x1"][j] - objects["x0"][j] + 1)
            assert float(f[10]) == area[j] / box
        bad = objects.copy()
        bad["area"][0] += 1
        os.remove(p)
        with pytest.raises(AssertionError):
            driver.write_shapes_csv(p, bad, rec)                  # the window counts give another area than the table
        assert not os.path.exists(p)
    driver.write_shapes_csv(p, objects[:0], rec[:0])
    assert open(p).read() == ",".join(driver.SHAPE_COLUMNS) + "\n"


def test_driver_refuses_label_shape_without_label_mask(tmp_path, monkeypatch, capsys):
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
        with pytest.raises(SystemExit) as e:
            driver.run(tool, [img, "--model", "nucleiDAPI", "--labelShape"])
        assert e.value.code == 2
        assert "--labelShape needs --labelMask" in capsys.readouterr().err, tool
