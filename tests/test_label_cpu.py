"""CPU checks of the label mask: the numpy / scipy restatement against a flood fill of its own, the class rule's
ties, the host-only limits of umx_label_options_check, the drivers' flag refusals, the int32 TIFF page, and the loud failure without a
GPU.  No kernel runs here: tests/test_gpu_label.py holds the device to the restatement."""
import ctypes
import os
import re

import numpy as np
import pytest

import helpers
import label_ref
from unmicst_amd import build, driver, model, tiffio, umx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    build.build()
    return umx.load()


def flood_fill(planes, cls, min_area):
    """The definition, literally, sharing no code with label_ref: first maximum by a loop, components by a stack, in raster order."""
    K, H, W = planes.shape
    obj = np.zeros((H, W), bool)
    for y in range(H):
        for x in range(W):
            best, arg = -1, -1
            for k in range(K):
                if int(planes[k, y, x]) > best:
                    best, arg = int(planes[k, y, x]), k
            obj[y, x] = arg == cls
    seen = np.zeros((H, W), bool)
    labels = np.zeros((H, W), np.int32)
    rows = []
    for y in range(H):
        for x in range(W):
            if not obj[y, x] or seen[y, x]:
                continue
            seen[y, x] = True
            todo, px = [(y, x)], []
            while todo:
                cy, cx = todo.pop()
                px.append((cy, cx))
                for ny, nx in ((cy - 1, cx), (cy + 1, cx), (cy, cx - 1), (cy, cx + 1)):
                    if 0 <= ny < H and 0 <= nx < W and obj[ny, nx] and not seen[ny, nx]:
                        seen[ny, nx] = True
                        todo.append((ny, nx))
            if len(px) < min_area:
                continue
            ys, xs = [p[0] for p in px], [p[1] for p in px]
            rows.append((len(px), min(ys), min(xs), max(ys), max(xs), 0, sum(ys), sum(xs)))
            for cy, cx in px:
                labels[cy, cx] = len(rows)
    return labels, np.array(rows, label_ref.OBJECT) if rows else np.zeros(0, label_ref.OBJECT)


@pytest.mark.parametrize("H,W", [(9, 13), (17, 5)])
def test_restatement_equals_a_flood_fill(H, W):
    rng = np.random.default_rng(H * 100 + W)
    for K, cls, min_area, levels in ((3, 2, 1, 256), (3, 2, 3, 4), (3, 0, 1, 3), (2, 1, 2, 2), (5, 3, 1, 2)):
        planes = rng.integers(0, levels, (K, H, W)).astype(np.uint8)     # few levels: many ties
        labels, table = label_ref.label(planes, cls, min_area)
        want_labels, want_table = flood_fill(planes, cls, min_area)
        assert labels.dtype == np.int32 and np.array_equal(labels, want_labels), (K, cls, min_area)
        assert len(table) == len(want_table) == labels.max()
        for f in label_ref.FIELDS:
            assert np.array_equal(table[f], want_table[f]), f


def test_a_tie_goes_to_the_lower_class():
    planes = np.full((3, 6, 7), 85, np.uint8)
    assert len(label_ref.label(planes, 2)[1]) == 0
    labels, table = label_ref.label(planes, 0)
    assert len(table) == 1 and table["area"][0] == 42 and (labels == 1).all()
    assert len(label_ref.label(planes)[1]) == 0              # the default class is the last one


def test_binding_mirrors_the_header(lib):
    header = open(os.path.join(ROOT, "include", "umx.h")).read()
    macros = {k: int(v) for k, v in re.findall(r"#define (UMX_LABEL_\w+) (\d+)", header)}
    assert macros == {"UMX_LABEL_MAX_CLASSES": umx.LABEL_MAX_CLASSES, "UMX_LABEL_MAX_MIN_AREA": umx.LABEL_MAX_MIN_AREA,
                      "UMX_LABEL_STRIP_ROWS": umx.LABEL_STRIP_ROWS, "UMX_LABEL_THREADS": umx.LABEL_THREADS,
                      "UMX_LABEL_SCAN_BLOCK": umx.LABEL_SCAN_BLOCK}
    assert ctypes.sizeof(umx._LabelOptions) == 32 and ctypes.sizeof(umx.LabelObject) == 40 == umx.LABEL_OBJECT_DTYPE.itemsize
    assert umx.LABEL_OBJECT_DTYPE == label_ref.OBJECT
    for name, _ in umx.LabelObject._fields_:
        assert getattr(umx.LabelObject, name).offset == umx.LABEL_OBJECT_DTYPE.fields[name][1], name


def test_options_check_accepts_and_refuses_each_limit(lib):
    ok = umx.label_options_check
    assert ok(3, 150, 203, 2, 1) == ""
    assert ok(1, 1, 1, 0, 1) == "" and ok(16, 1, 1, 15, 65536) == ""
    assert "at least 1" in ok(3, 0, 5, 2) and "at least 1" in ok(3, 5, 0, 2) and "at least 1" in ok(3, -1, 5, 2)
    assert ok(3, 46340, 46340, 2) == ""                       # 2 147 395 600 pixels
    assert ok(3, 1, 2 ** 31 - 1, 2) == "" and ok(3, 2 ** 31 - 1, 1, 2) == ""
    assert "int32" in ok(3, 2 ** 16, 2 ** 15, 2)              # H * W = 2^31
    assert "int32" in ok(3, 46341, 46341, 2)
    assert "classes" in ok(0, 5, 5, 0) and "classes" in ok(17, 5, 5, 0)
    assert "cls" in ok(3, 5, 5, 3) and "cls" in ok(3, 5, 5, -1) and ok(3, 5, 5, 0) == ""
    assert "min_area" in ok(3, 5, 5, 2, 0) and "min_area" in ok(3, 5, 5, 2, 65537) and "min_area" in ok(3, 5, 5, 2, -4)
    for j in range(6):
        assert "reserved" in ok(3, 5, 5, 2, 1, reserved=[0] * j + [1])
    buf = ctypes.create_string_buffer(8)
    assert lib.umx_label_options_check(None, 3, 5, 5, buf, 8) == umx.ERR_INVALID and buf.value == b"null la"
    o = umx._LabelOptions(2, 1)
    assert lib.umx_label_options_check(ctypes.byref(o), 3, 5, 5, None, 0) == 0


def test_driver_refuses_bad_label_flags_before_any_engine(tmp_path, monkeypatch, capsys):
    hp, blob, mean, std = helpers.load_nuclei_dapi()
    models = tmp_path / "models"
    model.save_converted(model.ModelArtefacts(hp, blob, mean, std), str(models / "nucleiDAPI"))
    monkeypatch.setenv("UMX_MODELS_DIR", str(models))

    def no_engine(*a, **k):
        raise AssertionError("the engine was set up before the label flags were checked")
    monkeypatch.setattr(umx, "Engine", no_engine)
    img = str(tmp_path / "x" / "registration" / "missing.tif")   # never read: the refusal comes first
    for tool in driver.TOOLS:
        for flags, word in ((["--labelClass", "1"], "needs --labelMask"), (["--labelMinArea", "4"], "needs --labelMask"),
                            (["--labelMask", "--labelClass", "3"], "classes 0..2"), (["--labelMask", "--labelClass", "-1"], "from 0"),
                            (["--labelMask", "--labelMinArea", "0"], "1..65536"), (["--labelMask", "--labelMinArea", "65537"], "1..65536")):
            with pytest.raises(SystemExit) as e:
                driver.run(tool, [img, "--model", "nucleiDAPI"] + flags)
            assert e.value.code == 2
            assert word in capsys.readouterr().err, (tool, flags)


def test_objects_csv(tmp_path):
    table = np.zeros(2, label_ref.OBJECT)
    table[0] = (3, 0, 1, 1, 2, 0, 1, 4)
    table[1] = (7, 5, 0, 6, 9, 0, 38, 31)
    p = str(tmp_path / "o.csv")
    driver.write_objects_csv(p, table)
    assert open(p).read() == ("label,area,y0,x0,y1,x1,centroid_y,centroid_x\n1,3,0,1,1,2,0.333333,1.333333\n"
                              "2,7,5,0,6,9,5.428571,4.428571\n")
    driver.write_objects_csv(p, table[:0])
    assert open(p).read() == "label,area,y0,x0,y1,x1,centroid_y,centroid_x\n"


def test_int32_page_round_trips_through_tiffio(tmp_path):
    rng = np.random.default_rng(2)
    page = rng.integers(0, 2 ** 31 - 1, (37, 53)).astype(np.int32)
    page[0, 0], page[0, 1] = 0, 2 ** 31 - 1
    p = str(tmp_path / "l.tif")
    tiffio.imsave(p, page)
    back = tiffio.imread(p)
    assert back.dtype == np.int32 and np.array_equal(back, page)


def test_labeler_fails_loudly_without_a_gpu(lib):
    if umx.device_count() > 0:
        pytest.skip("a GPU is present")
    with pytest.raises(umx.UmxError) as e:
        umx.Labeler()
    assert e.value.code == 3


def test_bench_tool_generators():
    """tools/bench_label.py states its two inputs: seeded, of the asked shape, discs inside their cells, salt near its density"""
    import importlib.util
    spec = importlib.util.spec_from_file_location("bench_label", os.path.join(ROOT, "tools", "bench_label.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    a, b = m.blob_mask(150, 203), m.blob_mask(150, 203)
    assert a.shape == (150, 203) and a.dtype == bool and np.array_equal(a, b) and 0.05 < a.mean() < 0.4
    n = len(label_ref.label_mask(a)[1])
    assert 5 < n <= 5 * 7                                     # at most one disc per 32 x 32 cell, some fused
    s = m.salt_mask(300, 300)
    assert abs(s.mean() - 0.6) < 0.01
    planes = m.planes_of(a)
    assert planes.dtype == np.uint8 and np.array_equal(label_ref.object_pixels(planes), a)
