"""Host checks of the object score (include/umx_train.h umx_object_options, DESIGN.md section 9.2, "Object score"): the numpy / scipy
restatement (tests/trainset_objects_ref.py) on hand-made planes whose counts are written out by hand, the plane rule, the host
validation of the options, ObjectOptions, the command's flags and its selection rule."""
import argparse
import ctypes
import math

import numpy as np
import pytest

import trainset_objects_ref as oref
from unmicst_amd import finetune, model, trainer, trainset, umx

OBJ = oref.OBJ


@pytest.mark.parametrize("name", sorted(oref.hand_made()))
def test_restatement_on_hand_made_planes(name):
    truth, pred, min_area, want = oref.hand_made()[name]
    counts, tl, pl = oref.object_counts(truth, pred, OBJ, min_area)
    assert counts.dtype == np.int64 and counts.shape == (8,) and tuple(counts[6:]) == (0, 0)
    assert dict(zip(oref.NAMES, counts[:6].tolist())) == want, name
    assert tl.dtype == np.int32 and pl.dtype == np.int32
    assert len(np.unique(tl)) - 1 == want["truth"]


def test_the_thresholds_are_strict():
    c = oref.hand_made()
    t, p, _, _ = c["iou_exactly_one_half"]
    assert oref.object_counts(t, t, OBJ)[0][2] == 1                       # the same object predicted whole is matched
    t, p, _, _ = c["iou_exactly_three_quarters"]
    assert oref.object_counts(t, t, OBJ)[0][3] == 1
    # one pixel more on either side of the 3/4 pair: 4 of 4 is above, 2 of 4 (IoU 1/2) is not even matched
    p2 = p.copy()
    p2[8, 9] = oref.BG
    assert tuple(oref.object_counts(t, p2, OBJ)[0][2:4]) == (0, 0)


def test_labels_are_one_plus_the_first_pixel_and_four_connected():
    t = oref.hand_made()["diagonal_touch"][0]
    P = t.shape[0]
    tl = oref.labels_of(t, OBJ)
    assert sorted(np.unique(tl)) == [0, 1 + 6 * P + 6, 1 + 10 * P + 10]     # a shared corner does not join them
    assert np.array_equal(tl, oref.bref.labels_of(t, OBJ))                  # the border maps label the same way
    t, p = oref.stripes(32)
    counts, tl, pl = oref.object_counts(t, p, OBJ)
    assert tuple(counts[:6]) == (16, 16, 0, 0, 0, 0)                        # 256 pairs of one shared pixel: nothing is mostly inside anything
    assert sorted(np.unique(pl)) == [0] + [1 + 64 * k for k in range(16)]


def test_unlabelled_pixels_are_outside_the_evaluation():
    truth, pred, _, _ = oref.hand_made()["unlabelled_block"]
    ruled = oref.plane_rule(truth, pred)
    assert (ruled[truth == 0] == 0).all() and np.array_equal(ruled[truth != 0], pred[truth != 0])
    assert (pred[truth == 0] == OBJ).sum() == 6 * 4 + 16                  # half of one object and the whole of another
    # planes_of: first maximum, first label
    probs = np.zeros((1, 2, 2, 3), np.float32)
    labels = np.zeros((1, 2, 2, 3), np.float32)
    probs[0, 0, 0] = (0.2, 0.4, 0.4)
    probs[0, 0, 1] = (0.1, 0.2, 0.7)
    probs[0, 1, 0] = (0.5, 0.5, 0.0)
    probs[0, 1, 1] = (0.0, 0.0, 1.0)
    labels[0, 0, 0, 2] = labels[0, 0, 1, 2] = labels[0, 1, 0, 0] = 1
    truth, pred = oref.planes_of(probs, labels)
    assert truth.tolist() == [[[3, 3], [1, 0]]] and pred.tolist() == [[[2, 3], [1, 0]]]


def test_f1_of_the_totals():
    assert oref.f1(np.array([4, 4, 3, 0, 0, 0, 0, 0])) == 0.75 and trainer.object_f1(3, 4, 4) == 0.75
    assert math.isnan(oref.f1(np.zeros(8, np.int64))) and math.isnan(trainer.object_f1(0, 0, 0))
    assert trainer.object_f1(0, 2, 0) == 0.0


def _check(code, min_area, n_classes, reserved=None):
    L = trainer._bind(umx.load())
    o = trainer.ObjectOptionsC()
    o.object_code, o.min_area = code, min_area
    if reserved is not None:
        o.reserved[reserved] = 1
    msg = ctypes.create_string_buffer(160)
    rc = L.umx_object_options_check(ctypes.byref(o), n_classes, msg, 160)
    return rc, msg.value.decode()


def test_umx_object_options_check():
    assert ctypes.sizeof(trainer.ObjectOptionsC) == 32
    assert _check(3, 1, 3) == (0, "") and _check(1, 65536, 2) == (0, "") and _check(2, 5, 3) == (0, "")
    for (code, area, K, res), word in (((0, 1, 3, None), "object_code is 0"), ((4, 1, 3, None), "1..3"), ((-1, 1, 3, None), "object_code"),
                                       ((3, 0, 3, None), "min_area is 0"), ((3, 65537, 3, None), "1..65536"), ((3, -4, 3, None), "min_area"),
                                       ((3, 1, 3, 0), "reserved must be zero"), ((3, 1, 3, 5), "reserved must be zero")):
        rc, msg = _check(code, area, K, res)
        assert rc == 1 and word in msg, (code, area, K, res, msg)
    L = trainer._bind(umx.load())
    msg = ctypes.create_string_buffer(160)
    assert L.umx_object_options_check(None, 3, msg, 160) == 1 and b"null" in msg.value
    o = trainer.ObjectOptionsC()
    o.object_code, o.min_area = 0, 1
    assert L.umx_object_options_check(ctypes.byref(o), 3, None, 0) == 1   # msg may be NULL
    for name in ("umx_object_options_check", "umx_trainer_evaluate_objects", "umx_trainer_object_counts"):
        assert name in trainer.EXPORTS


def test_object_options_defaults_and_refusals():
    o = trainset.ObjectOptions()
    assert o.object_class is None and o.min_area == 1 and o.object_code(3) == 3 and o.object_code(2) == 2
    c = trainset.ObjectOptions(1, 7).c_struct(3)
    assert (c.object_code, c.min_area, list(c.reserved)) == (2, 7, [0] * 6)
    for bad in (0, -1, 65537, 1.5, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            trainset.ObjectOptions(None, bad)
    for bad in (-1, 1.5):
        with pytest.raises(ValueError):
            trainset.ObjectOptions(bad)
    with pytest.raises(ValueError):
        trainset.ObjectOptions(3).c_struct(3)


def _args(*flags):
    return finetune.build_parser().parse_args(["--model", "m", "--train", "t", "--valid", "v", "--out", "o"] + list(flags))


V2 = model.HParams(model.GRAPH_V2, 32, 1, 3, 8, 2, 3, 0)
LEGACY = model.HParams(model.GRAPH_LEGACY, 32, 1, 2, 8, 2, 3, 0)


def test_object_settings_of_the_command():
    assert finetune.object_settings(_args()) is None and finetune.object_settings(_args(), V2) is None
    assert finetune.object_settings(_args("--select", "pixel")) is None
    assert finetune.object_settings(argparse.Namespace()) is None         # (callers that build their own namespace)
    assert finetune.object_settings(_args("--object-score")) == {"class": None, "min_area": 1, "select": "pixel"}
    assert finetune.object_settings(_args("--object-score"), V2) == {"class": 2, "min_area": 1, "select": "pixel"}
    assert finetune.object_settings(_args("--object-score"), LEGACY) == {"class": 1, "min_area": 1, "select": "pixel"}
    assert finetune.object_settings(_args("--object-score", "--object-class", "1", "--object-min-area", "9", "--select", "object"), V2) == {
        "class": 1, "min_area": 9, "select": "object"}
    for flags, hp, word in ((("--object-class", "2"), None, "--object-class needs --object-score"),
                            (("--object-min-area", "3"), V2, "--object-min-area needs --object-score"),
                            (("--select", "object"), None, "--select object needs --object-score"),
                            (("--object-score", "--object-class", "-1"), None, "--object-class"),
                            (("--object-score", "--object-class", "3"), V2, "the model has classes 0..2"),
                            (("--object-score", "--object-class", "2"), LEGACY, "the model has classes 0..1"),
                            (("--object-score", "--object-min-area", "0"), None, "--object-min-area"),
                            (("--object-score", "--object-min-area", "65537"), None, "--object-min-area")):
        with pytest.raises(finetune.Refusal) as e:
            finetune.object_settings(_args(*flags), hp)
        assert word in str(e.value), flags


def test_prepare_refuses_the_flags_before_anything_is_read(tmp_path):
    with pytest.raises(finetune.Refusal) as e:
        finetune.prepare(_args("--select", "object"))
    assert "--select object needs --object-score" in str(e.value)


def test_selection_by_f1():
    nan = float("nan")
    assert finetune.better_f1(nan, None) and finetune.better_f1(0.0, None)      # the first evaluation is kept whatever it is
    assert not finetune.better_f1(nan, 0.0) and not finetune.better_f1(nan, nan)
    assert finetune.better_f1(0.0, nan) and finetune.better_f1(0.5, 0.25)
    assert not finetune.better_f1(0.5, 0.5) and not finetune.better_f1(0.25, 0.5)   # a tie keeps the earlier step
