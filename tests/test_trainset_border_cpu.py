"""Host checks of the border weight maps (include/umx_train.h umx_border_options): the numpy / scipy restatement
(tests/trainset_border_ref.py) against a literal brute force of the definition, the tie rule, BorderOptions and the command's flags,
the host validation of the options, and the shape of the log's "border" object."""
import argparse
import ctypes
import json

import numpy as np
import pytest

import trainset_border_ref as bref
from unmicst_amd import finetune, model, trainer, trainset, umx

OBJ = bref.OBJ


@pytest.mark.parametrize("sigma", [1.0, 1.5])
@pytest.mark.parametrize("which", ["blobs", "edges", "checker"])
def test_restatement_is_the_brute_force_of_the_definition(which, sigma):
    S = 20
    A = {"blobs": bref.blobs(S, 5, 1.2, 0.7), "edges": bref.edges_and_corners(S), "checker": bref.checkerboard(S)}[which]
    got, want = bref.border_planes(A, OBJ, sigma), bref.brute_force(A, OBJ, sigma)
    assert len(np.unique(want[0])) - 1 >= 5
    for g, w, name in zip(got, want, ("labels", "d1sq", "d2sq", "W")):
        assert g.dtype == w.dtype and np.array_equal(g, w), (which, sigma, name)
    R = bref.radius(sigma)
    assert R == int(np.ceil(4 * sigma)) and got[1].max() <= R * R and got[2].max() <= R * R
    assert (got[3] > 0).any() and ((got[3] > 0) == (got[2] >= 0)).all()


def test_labels_are_one_plus_the_first_pixel_and_four_connected():
    A = bref.diagonal_touch(24)
    labels, d1, d2, W = bref.border_planes(A, OBJ, 1.0)
    assert sorted(np.unique(labels)) == [0, 1 + 6 * 24 + 6, 1 + 10 * 24 + 10]     # a shared corner does not join them
    assert d2[9, 9] == 2 and d2[10, 10] == 2 and d1[9, 9] == 0
    assert (bref.labels_of(bref.serpentine(64), OBJ)[::2] == 1).all()
    assert sorted(np.unique(bref.labels_of(bref.double_serpentine(64), OBJ))) == [0, 1 + 2, 1 + 2 * 64]
    assert len(np.unique(bref.labels_of(bref.checkerboard(48), OBJ))) - 1 == 48 * 48 // 2


def test_a_pixel_equidistant_from_two_components_has_equal_distances():
    A = np.full((21, 21), bref.BG, np.uint8)
    A[10, 4], A[10, 16], A[2, 10] = OBJ, OBJ, OBJ         # (10, 10) is 6 from the first two and 8 from the third
    for B in (A, A.T):                                    # the scan meets the left one first, resp. the upper one
        labels, d1, d2, W = bref.border_planes(B, OBJ, 2.0)
        assert d1[10, 10] == 36 and d2[10, 10] == 36
        assert W[10, 10] == np.float32(np.exp(-(12.0 ** 2) / 8.0))
    labels, d1, d2, W = bref.border_planes(A, OBJ, 2.0)
    assert d1[10, 5] == 1 and d2[10, 5] == -1 and W[10, 5] == 0           # the others are 11 and sqrt(89) > R = 8 away
    one = np.full((21, 21), bref.BG, np.uint8)
    one[5:9, 5:9] = OBJ
    labels, d1, d2, W = bref.border_planes(one, OBJ, 2.0)
    assert (d2 == -1).all() and (W == 0).all() and (d1[5:9, 5:9] == 0).all() and d1[20, 20] == -1


def test_border_options_defaults_and_refusals():
    o = trainset.BorderOptions()
    assert o.sigma == 5.0 and o.object_class is None and o.radius == 20
    assert o.object_code(3) == 3 and o.object_code(2) == 2               # the last class
    assert trainset.BorderOptions(2.5, 0).object_code(3) == 1
    assert trainset.BorderOptions(8.0).radius == 32 and trainset.BorderOptions(0.1).radius == 1
    c = trainset.BorderOptions(1.5, 1).c_struct(3)
    assert (c.object_code, c.sigma, list(c.reserved)) == (2, 1.5, [0] * 6)
    assert ctypes.sizeof(trainer.BorderOptionsC) == 32
    for bad in (0.0, -1.0, 8.5, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            trainset.BorderOptions(bad)
    for bad in (-1, 1.5):
        with pytest.raises(ValueError):
            trainset.BorderOptions(5.0, bad)
    with pytest.raises(ValueError):
        trainset.BorderOptions(5.0, 3).c_struct(3)
    assert "umx_trainset_border_weights" in trainer.EXPORTS and "umx_trainset_border_planes" in trainer.EXPORTS


def _args(*flags):
    return finetune.build_parser().parse_args(["--model", "m", "--train", "t", "--valid", "v", "--out", "o"] + list(flags))


V2 = model.HParams(model.GRAPH_V2, 32, 1, 3, 8, 2, 3, 0)
LEGACY = model.HParams(model.GRAPH_LEGACY, 32, 1, 2, 8, 2, 3, 0)


def test_border_settings_of_the_command():
    assert finetune.border_settings(_args()) is None and finetune.border_settings(_args(), V2) is None
    assert finetune.border_settings(argparse.Namespace()) is None         # (callers that build their own namespace)
    assert finetune.border_settings(_args("--border-sigma", "5")) == {"sigma": 5.0, "class": None, "radius": 20}
    assert finetune.border_settings(_args("--border-sigma", "5"), V2) == {"sigma": 5.0, "class": 2, "radius": 20}
    assert finetune.border_settings(_args("--border-sigma", "1.3", "--border-class", "1"), V2) == {"sigma": 1.3, "class": 1, "radius": 6}
    for flags, hp, word in ((("--border-sigma", "0"), None, "--border-sigma"), (("--border-sigma", "8.5"), None, "--border-sigma"),
                            (("--border-sigma", "nan"), None, "--border-sigma"), (("--border-sigma", "-2"), None, "--border-sigma"),
                            (("--border-class", "2"), None, "needs --border-sigma"), (("--border-class", "2"), V2, "needs --border-sigma"),
                            (("--border-sigma", "5", "--border-class", "-1"), None, "--border-class"),
                            (("--border-sigma", "5", "--border-class", "3"), V2, "--border-class"),
                            (("--border-sigma", "5"), LEGACY, "the legacy loss takes no weights")):
        with pytest.raises(finetune.Refusal) as e:
            finetune.border_settings(_args(*flags), hp)
        assert word in str(e.value), flags


def test_the_log_object_has_the_documented_shape():
    b = finetune.border_settings(_args("--border-sigma", "2.5"), V2)
    b["computed"] = [6, 2]
    line = json.loads(json.dumps({"elastic": {"prob": 0.5, "sigma": 1.0, "grid": 2}, "border": b}))
    assert list(line) == ["elastic", "border"]
    assert line["border"] == {"sigma": 2.5, "class": 2, "radius": 10, "computed": [6, 2]}


def test_upload_refuses_a_border_for_an_unweighted_set():
    class FakeTrainer:
        hp = LEGACY
    ds = trainset.Dataset(np.zeros((1, 1, 1, 32, 32), np.float32), np.ones((1, 32, 32), np.uint8), [None])
    with pytest.raises(ValueError) as e:
        trainset.upload(FakeTrainer(), ds, trainset.UNWEIGHTED, border=trainset.BorderOptions())
    assert "the legacy loss takes no weights" in str(e.value)


def _check(code, sigma, n_classes, reserved=None):
    L = trainer._bind(umx.load())
    o = trainer.BorderOptionsC()
    o.object_code, o.sigma = code, sigma
    if reserved is not None:
        o.reserved[reserved] = 1
    msg = ctypes.create_string_buffer(160)
    rc = L.umx_border_options_check(ctypes.byref(o), n_classes, msg, 160)
    return rc, msg.value.decode()


def test_umx_border_options_check_messages():
    assert _check(3, 5.0, 3) == (0, "") and _check(1, 8.0, 2) == (0, "") and _check(2, 1e-3, 3) == (0, "")
    for (code, sigma, K, res), word in (((0, 5.0, 3, None), "object_code is 0"), ((4, 5.0, 3, None), "1..3"),
                                        ((3, 0.0, 3, None), "sigma is 0"), ((3, 8.5, 3, None), "at most 8"),
                                        ((3, float("nan"), 3, None), "sigma is nan"), ((3, -1.0, 3, None), "sigma is -1"),
                                        ((3, 5.0, 3, 0), "reserved must be zero"), ((3, 5.0, 3, 5), "reserved must be zero")):
        rc, msg = _check(code, sigma, K, res)
        assert rc == 1 and word in msg, (code, sigma, K, res, msg)
    L = trainer._bind(umx.load())
    msg = ctypes.create_string_buffer(160)
    assert L.umx_border_options_check(None, 3, msg, 160) == 1 and b"null" in msg.value
    o = trainer.BorderOptionsC()
    o.object_code, o.sigma = 0, 5.0
    assert L.umx_border_options_check(ctypes.byref(o), 3, None, 0) == 1   # msg may be NULL
