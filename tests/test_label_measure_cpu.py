"""CPU checks of the label mask's measurement: the numpy restatement against scipy.ndimage, the
Intensities file against exact rational arithmetic, the host-only limits of umx_label_measure_check, the record's size and the drivers'
flag refusals.  No kernel runs here: tests/test_gpu_label_measure.py holds the device to the restatement."""
import ctypes
import math
import os
import re
from fractions import Fraction

import numpy as np
import pytest
from scipy import ndimage

import helpers
import label_measure_ref as ref
from unmicst_amd import build, driver, model, umx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    build.build()
    return umx.load()


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16])
def test_restatement_equals_scipy_where_float64_is_exact(dtype):
    """37 x 53 pixels of at most 65535: every sum is below 2^53, so scipy's float64 sums are exact"""
    rng = np.random.default_rng(3)
    N = 9
    labels = rng.integers(-2, N + 3, (37, 53)).astype(np.int32)      # -2, -1, N + 1 and N + 2 count as 0
    labels[labels == 4] = 0                                          # a label no pixel carries
    planes = ref.pixels((37, 53), dtype, 3, seed=5)
    got = ref.measure(labels, planes, N)
    index = np.arange(1, N + 1)
    for c in range(3):
        v = planes[c].astype(np.float64)
        assert np.array_equal(got["sum"][c], ndimage.sum_labels(v, labels, index).astype(np.uint64))
        assert np.array_equal(got["sum_sq"][c], ndimage.sum_labels(v * v, labels, index).astype(np.uint64))
        assert np.array_equal(got["count"][c], ndimage.sum_labels(np.ones_like(v), labels, index).astype(np.uint32))
        present = got["count"][c] > 0
        assert present.sum() == N - 1 and not present[3]
        assert np.array_equal(got["min"][c][present], ndimage.minimum(v, labels, index)[present].astype(np.uint32))
        assert np.array_equal(got["max"][c][present], ndimage.maximum(v, labels, index)[present].astype(np.uint32))
        empty = got[c][3]
        assert (empty["count"], empty["sum"], empty["sum_sq"], empty["min"], empty["max"]) == (0, 0, 0, 2 ** 32 - 1, 0)
    assert (got["reserved"] == 0).all()


def test_binding_mirrors_the_header(lib):
    header = open(os.path.join(ROOT, "include", "umx.h")).read()
    assert umx.LABEL_MEASURE_DTYPE == ref.RECORD and umx.LABEL_MEASURE_DTYPE.itemsize == 32
    body = re.search(r"typedef struct umx_label_measure \{(.*?)\} umx_label_measure;", header, re.S).group(1)
    fields = [n.strip() for decl in re.findall(r"uint\d+_t ([\w, ]+);", body) for n in decl.split(",")]
    assert tuple(fields) == umx.LABEL_MEASURE_DTYPE.names
    assert int(re.search(r"#define UMX_MEASURE_U8 (\d+)", header).group(1)) == umx.MEASURE_U8
    assert int(re.search(r"#define UMX_MEASURE_U16 (\d+)", header).group(1)) == umx.MEASURE_U16
    macros = {k: int(v) for k, v in re.findall(r"#define (UMX_MEASURE_\w+) (\d+)", header)}
    assert macros == {"UMX_MEASURE_U8": umx.MEASURE_U8, "UMX_MEASURE_U16": umx.MEASURE_U16,
                      "UMX_MEASURE_GROUP_PLANES": umx.LABEL_MEASURE_GROUP, "UMX_MEASURE_MAX_PLANES": umx.LABEL_MAX_MEASURE_PLANES}
    assert "enum { UMX_LABEL_MEASURE_GROUP = UMX_MEASURE_GROUP_PLANES, UMX_LABEL_MAX_MEASURE_PLANES = UMX_MEASURE_MAX_PLANES };" in header
    assert (umx.LABEL_MEASURE_GROUP, umx.LABEL_MAX_MEASURE_PLANES) == (4, 1024)

    class Record(ctypes.Structure):                              # the header's record, field by field
        _fields_ = [("sum", ctypes.c_uint64), ("sum_sq", ctypes.c_uint64), ("min", ctypes.c_uint32), ("max", ctypes.c_uint32),
                    ("count", ctypes.c_uint32), ("reserved", ctypes.c_uint32)]
    assert ctypes.sizeof(Record) == 32
    for name, _ in Record._fields_:
        assert getattr(Record, name).offset == umx.LABEL_MEASURE_DTYPE.fields[name][1], name


def test_measure_check_accepts_and_refuses_each_limit(lib):
    ok = umx.label_measure_check
    assert ok(umx.MEASURE_U8, 1, 1, 1, 0) == "" and ok(umx.MEASURE_U16, 1024, 150, 203, 7) == ""
    assert "dtype" in ok(0, 1, 5, 5, 1) and "dtype" in ok(3, 1, 5, 5, 1)
    assert "planes" in ok(1, 0, 5, 5, 1) and "planes" in ok(1, 1025, 5, 5, 1)
    assert ok(2, 3, 46340, 46340, 1) == "" and ok(2, 3, 1, 2 ** 31 - 1, 1) == ""
    assert "int32" in ok(2, 3, 2 ** 16, 2 ** 15, 1) and "int32" in ok(2, 3, 46341, 46341, 1)      # H * W > 2^31 - 1
    assert "at least 1" in ok(2, 3, 0, 5, 1) and "at least 1" in ok(2, 3, 5, -1, 1)
    assert "n_objects" in ok(2, 3, 5, 5, -1) and ok(2, 3, 5, 5, 2 ** 31 - 1) == "" and "n_objects" in ok(2, 3, 5, 5, 2 ** 31)
    buf = ctypes.create_string_buffer(6)
    assert lib.umx_label_measure_check(0, 1, 5, 5, 1, buf, 6) == umx.ERR_INVALID and buf.value == b"dtype"
    assert lib.umx_label_measure_check(1, 1, 5, 5, 1, None, 0) == 0


def records_of(rows):
    r = np.zeros(len(rows), ref.RECORD)
    for j, pix in enumerate(rows):
        r[j] = (sum(pix), sum(p * p for p in pix), min(pix), max(pix), len(pix), 0)
    return r


def test_intensities_csv_against_exact_rationals(tmp_path):
    """The mean is one correctly rounded division of two exact integers.  The std is the stated formula, a difference of two numbers
    near sum_sq / count, each rounded to 2^-53 relative: its variance is off by about 3 * 2^-53 * sum_sq / count, so the std holds
    1e-9 relative where variance / (sum_sq / count) is above 2e-7 -- every record here is above 1e-3 or constant (DESIGN.md section
    8.1 states the limit for nearly constant objects)."""
    rows = [[7], [65535] * 1000, [0, 65535], [1, 2, 4], [65535] * 35000 + [60000] * 35001, [3, 3, 3, 3, 3, 3, 3], [0, 0, 1]]
    ch = records_of(rows)
    pm = records_of([[min(p, 255) for p in pix] for pix in rows])
    area = np.array([len(pix) for pix in rows], np.int32)
    objects = np.zeros(len(rows), umx.LABEL_OBJECT_DTYPE)
    objects["area"] = area
    mean, std = umx.measure_mean_std(ch)
    for j, pix in enumerate(rows):
        m, var = ref.exact_mean_var(ch[j])
        assert m == Fraction(sum(pix), len(pix)) and var >= 0
        assert mean[j] == float(m)                                # the mean to the last bit: one correctly rounded division
        want = math.sqrt(float(var)) if var else 0.0
        if len(set(pix)) == 1:
            assert std[j] == 0.0                                  # exactly 0 for a constant object
        else:
            assert var / Fraction(int(ch[j]["sum_sq"]), len(pix)) > Fraction(1, 1000)
            assert abs(std[j] - want) <= 1e-9 * want, (j, std[j], want)
    p = str(tmp_path / "i.csv")
    driver.write_intensities_csv(p, objects, [("pm0", pm), ("ch2", ch)])
    lines = open(p).read().splitlines()
    assert lines == ref.csv_lines(area, [("pm0", pm), ("ch2", ch)])
    assert lines[0] == "label,area,pm0_mean,pm0_std,pm0_min,pm0_max,ch2_mean,ch2_std,ch2_min,ch2_max"
    assert lines[1] == "1,1,7.000000,0.000000,7,7,7.000000,0.000000,7,7"
    assert lines[3] == "3,2,127.500000,127.500000,0,255,32767.500000,32767.500000,0,65535"
    assert lines[4] == "4,3,2.333333,1.247219,1,4,2.333333,1.247219,1,4"
    driver.write_intensities_csv(p, objects[:0], [("ch0", ch[:0])])
    assert open(p).read() == "label,area,ch0_mean,ch0_std,ch0_min,ch0_max\n"
    bad = ch.copy()
    bad["count"][2] += 1
    os.remove(p)
    with pytest.raises(AssertionError):
        driver.write_intensities_csv(p, objects, [("ch0", bad)])  # count != area
    assert not os.path.exists(p)


def test_driver_refuses_bad_measure_flags_before_any_engine(tmp_path, monkeypatch, capsys):
    hp, blob, mean, std = helpers.load_nuclei_dapi()
    models = tmp_path / "models"
    model.save_converted(model.ModelArtefacts(hp, blob, mean, std), str(models / "nucleiDAPI"))
    monkeypatch.setenv("UMX_MODELS_DIR", str(models))

    def no_engine(*a, **k):
        raise AssertionError("the engine was set up before the label flags were checked")
    monkeypatch.setattr(umx, "Engine", no_engine)
    from unmicst_amd import tiffio
    os.makedirs(tmp_path / "x" / "registration")
    img = str(tmp_path / "x" / "registration" / "two.tif")
    tiffio.imsave(img, np.zeros((5, 7), np.uint16))
    tiffio.imsave(img, np.zeros((5, 7), np.uint16), append=True)
    for tool in driver.TOOLS:
        for flags, word in ((["--labelMeasure"], "--labelMeasure needs --labelMask"), (["--labelMeasure", "0"], "--labelMeasure needs --labelMask"),
                            (["--labelMask", "--labelMeasure", "-1"], "from 0"), (["--labelMask", "--labelMeasure", "0", "2"], "pages 0..1")):
            with pytest.raises(SystemExit) as e:
                driver.run(tool, [img, "--model", "nucleiDAPI"] + flags)
            assert e.value.code == 2
            assert word in capsys.readouterr().err, (tool, flags)
