"""GPU tests of the border weight maps (include/umx_train.h: umx_trainset_border_weights, umx_trainset_border_planes; DESIGN.md section
9.2, "Border weight maps") against tests/trainset_border_ref.py: labels and both squared distances bit-equal, the map within one float32
ulp (sqrt in float64 is correctly rounded on both sides, the device's float64 exp may differ from the host's by an ulp of float64, which
moves the float32 rounding by at most one ulp; W >= exp(-32) is a normal number) and exactly 0 where the restatement has 0.  Then: one
sample's map is replaced and nothing else, two runs give the same bits, the kernels stay inside their buffers under UMX_DEBUG_GUARD,
refused calls change nothing, the map reaches the assembled weights, and the fine-tuning command computes it for sets without _wt.tif."""
import ctypes
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import helpers
import trainset_border_ref as bref
import trainset_ref as ref
from unmicst_amd import finetune, model, trainer, trainset, umx

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_INVALID = 1
OBJ, RING = bref.OBJ, bref.RING

HP = helpers.small_hps()["v2_duo_like"]                  # 32-pixel tile, 2 channels, 3 classes
LW = trainset.LABEL_WEIGHTS["duo"]                       # class (1, 2, 5), intersect (0, 10, 0)
B = 2
R2 = bref.radius(2.0)                                    # 8


def _empty(S):
    return np.full((S, S), bref.BG, np.uint8)


def _single(S):
    A = _empty(S)
    A[7:19, 5:30] = OBJ
    return A


# name -> (annotation, sigma)
CASES = {
    "blobs_S45_s1": (lambda: bref.blobs(45, 1), 1.0),
    "blobs_S70_s2.5": (lambda: bref.blobs(70, 2), 2.5),
    "blobs_S64_s5": (lambda: bref.blobs(64, 3), 5.0),
    "blobs_S96_s8": (lambda: bref.blobs(96, 4), 8.0),
    "serpentine": (lambda: bref.serpentine(64), 2.0),
    "double_serpentine": (lambda: bref.double_serpentine(64), 2.0),
    "u_shapes": (lambda: bref.u_shapes(64), 1.5),
    "checkerboard": (lambda: bref.checkerboard(48), 1.0),
    "diagonal_touch": (lambda: bref.diagonal_touch(33), 1.0),
    "edges_and_corners": (lambda: bref.edges_and_corners(45), 3.0),
    "cut_row": (lambda: bref.two_pixels(40, 20, 10, 0, R2), 2.0),
    "cut_row_beyond": (lambda: bref.two_pixels(40, 20, 10, 0, R2 + 1), 2.0),
    "cut_diagonal_beyond": (lambda: bref.two_pixels(40, 20, 10, 4, 7), 2.0),     # 16 + 49 = 65 > 64
    "no_object": (lambda: _empty(37), 2.0),
    "one_component": (lambda: _single(37), 2.0),
}


@functools.lru_cache(maxsize=None)
def _case(name):
    """(annotation, sigma, reference planes): computed once, shared, never written to."""
    make, sigma = CASES[name]
    A = make()
    want = bref.border_planes(A, OBJ, sigma)
    for a in (A,) + want:
        a.setflags(write=False)
    return A, sigma, want


def _trainer():
    return trainer.Trainer(HP, model.random_blob(HP, seed=3), trainer.duo_options(), batch=B)


def _set_of(tr, anns, wmaps=None, seed=0):
    rng = np.random.default_rng(seed)
    S = anns[0].shape[0]
    planes = rng.normal(0, 1, (len(anns), HP.nChannels, 1, S, S)).astype(np.float32)
    return planes, trainset.TrainSet.from_arrays(tr, planes, anns, wmaps, LW)


def _assert_planes(got, want, what):
    for g, w, name in zip(got[:3], want[:3], ("labels", "d1sq", "d2sq")):
        assert g.dtype == np.int32 and g.shape == w.shape, (what, name)
        ne = g != w
        assert not ne.any(), (what, name, int(ne.sum()), np.argwhere(ne)[:4].tolist())
    g, w = got[3], want[3]
    assert g.dtype == np.float32 and g.shape == w.shape, what
    ulp = bref.ulp_distance(g, w)
    print(what, "W: max ulp", int(ulp.max()), "pixels off", int((ulp > 0).sum()), "of", int((w > 0).sum()))
    assert ((g == 0) == (w == 0)).all(), (what, "zeros")
    assert ulp.max() <= 1, (what, int(ulp.max()), np.argwhere(ulp > 1)[:4].tolist())


def _identity_descs(idx):
    d = np.zeros(len(idx), trainer.SAMPLE_DESC)
    for j, i in enumerate(idx):
        d[j] = (i, 0, 0, 0, 0, 0.0, 1.0, 0)
    return d


def _assemble_all(tr, ts):
    """(data, labels, weights) of every sample of a set with size == imSize, at identity descriptors."""
    parts = [tr.assemble(ts, _identity_descs(list(range(b0, min(b0 + B, ts.n_samples))))) for b0 in range(0, ts.n_samples, B)]
    return tuple(np.concatenate([p[k] for p in parts]) for k in range(3))


def _weights_of(W, k=1):
    return (np.float64(np.float32(LW.intersect_weight[k])) * W.astype(np.float64) + np.float64(np.float32(LW.class_weight[k]))).astype(np.float32)


@pytest.mark.parametrize("name", sorted(CASES))
def test_planes_against_the_restatement(name):
    A, sigma, want = _case(name)
    labels, d1, d2, W = want
    S, R = A.shape[0], bref.radius(sigma)
    n_comp = len(np.unique(labels)) - 1
    # what the input must exercise, asserted on the restatement
    if name.startswith("blobs"):
        assert n_comp >= 5
        if sigma >= 2.5:
            assert (W > 0).sum() >= 500 and ((W > 0) & (A == RING)).any()
    elif name == "serpentine":
        assert n_comp == 1 and (labels[A == OBJ] == 1).all() and (A == OBJ).sum() > S * S // 2
    elif name == "double_serpentine":
        assert sorted(np.unique(labels)) == [0, 3, 1 + 2 * S] and (W > 0).mean() > 0.9
    elif name == "u_shapes":
        assert n_comp >= 5
    elif name == "checkerboard":
        assert n_comp == 1152 and len(np.unique(W)) == 2 and (W > 0).all()
    elif name == "diagonal_touch":
        assert n_comp == 2 and d2[9, 9] == 2 and d2[10, 10] == 2
    elif name == "edges_and_corners":
        assert all(labels[y, x] != 0 for y in (0, S - 1) for x in (0, S - 1)) and n_comp >= 8
    elif name == "cut_row":
        assert d1[20, 10] == 0 and d2[20, 10] == R * R and W[20, 10] == np.float32(np.exp(-R * R / 8.0)) and W[20, 10] > 0
        assert d1[20, 9] == 1 and d2[20, 9] == -1 and W[20, 9] == 0                      # (R + 1)^2 would be its d2sq
    elif name in ("cut_row_beyond", "cut_diagonal_beyond"):
        assert n_comp == 2 and d2[20, 10] == -1 and W[20, 10] == 0 and (W > 0).any()
    elif name == "no_object":
        assert n_comp == 0 and (d1 == -1).all()
    elif name == "one_component":
        assert n_comp == 1 and (d1 >= 0).any()
    if name in ("no_object", "one_component"):
        assert (W == 0).all() and (d2 == -1).all()
    # the sample sits between two samples that are one object each: nothing may be read from a neighbouring sample or from row padding
    full = np.full((S, S), OBJ, np.uint8)
    tr = _trainer()
    try:
        _, ts = _set_of(tr, [full, A, full])
        opts = trainset.BorderOptions(sigma)
        _assert_planes(ts.border_planes(1, opts), want, name)
        got = ts.border_planes(0, opts)
        assert (got[0] == 1).all() and (got[1] == 0).all() and (got[2] == -1).all() and (got[3] == 0).all()
    finally:
        tr.close()


def _three_samples(S=32):
    return [bref.blobs(S, 20 + i, 1.3, 0.7) for i in range(3)]


def test_one_sample_is_replaced_and_nothing_else():
    anns = _three_samples()
    rng = np.random.default_rng(5)
    wmaps = [rng.random((32, 32)).astype(np.float32) for _ in range(3)]
    opts = trainset.BorderOptions(2.0)
    want = [bref.border_planes(a, OBJ, 2.0)[3] for a in anns]
    assert all((w > 0).sum() > 50 for w in want)
    tr = _trainer()
    try:
        _, ts = _set_of(tr, anns, wmaps)
        before = _assemble_all(tr, ts)
        ts.border_weights(opts, 1)
        after = _assemble_all(tr, ts)
        assert after[0].tobytes() == before[0].tobytes() and after[1].tobytes() == before[1].tobytes()
        for i in (0, 2):
            assert after[2][i].tobytes() == before[2][i].tobytes(), i
        assert (after[2][1][..., 0] == 1.0).all() and (after[2][1][..., 2] == 5.0).all()
        assert bref.ulp_distance(after[2][1][..., 1], _weights_of(want[1])).max() <= 1
        assert after[2][1].tobytes() != before[2][1].tobytes()
        # every sample at once is three single calls
        ts.border_weights(opts)
        every = _assemble_all(tr, ts)
        _, ts2 = _set_of(tr, anns, wmaps)
        for i in (2, 0, 1):
            ts2.border_weights(opts, i)
        single = _assemble_all(tr, ts2)
        assert all(e.tobytes() == s.tobytes() for e, s in zip(every, single))
        for i in range(3):
            assert bref.ulp_distance(every[2][i][..., 1], _weights_of(want[i])).max() <= 1, i
        # a later upload of the sample overwrites the map as ever
        ts.set(1, np.zeros((HP.nChannels, 1, 32, 32), np.float32), anns[1], wmaps[1])
        assert tr.assemble(ts, _identity_descs([1]))[2].tobytes() == before[2][1:2].tobytes()
    finally:
        tr.close()


def test_two_runs_give_the_same_bits():
    tr = _trainer()
    try:
        for name in ("blobs_S96_s8", "serpentine", "checkerboard"):
            A, sigma, _ = _case(name)
            _, ts = _set_of(tr, [A, A])
            opts = trainset.BorderOptions(sigma)
            first = ts.border_planes(0, opts)
            for again in (ts.border_planes(0, opts), ts.border_planes(1, opts), ts.border_planes(0, opts)):
                assert all(a.tobytes() == b.tobytes() for a, b in zip(first, again)), name
            ts.close()
    finally:
        tr.close()


_GUARD_CHILD = """
import sys
import numpy as np
import trainset_border_ref as bref
import test_gpu_trainset_border as t
from unmicst_amd import trainset
A = bref.blobs(70, 2)
tr = t._trainer()
_, ts = t._set_of(tr, [A, bref.blobs(70, 9)])
opts = trainset.BorderOptions(2.5)
planes = ts.border_planes(0, opts)
ts.border_weights(opts)
ts.border_weights(opts, 1)
again = ts.border_planes(0, opts)
np.savez(sys.argv[1], *planes, *again)
tr.close()
"""


def test_blobs_under_the_debug_guard(tmp_path):
    """Every red zone of the set -- the workspace's and the diagnostic planes' included -- is checked at the end of both calls."""
    A, sigma, want = _case("blobs_S70_s2.5")
    out = str(tmp_path / "planes.npz")
    env = dict(os.environ, UMX_DEBUG_GUARD="0xff", PYTHONPATH=os.pathsep.join([ROOT, os.path.join(ROOT, "tests")]))
    r = subprocess.run([sys.executable, "-c", _GUARD_CHILD, out], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    assert "UMX_DEBUG_GUARD=0xff" in r.stderr
    z = np.load(out)
    got = [z["arr_%d" % k] for k in range(8)]
    _assert_planes(got[:4], want, "guarded")
    _assert_planes(got[4:], want, "guarded, second call")


def _raw(ts, index, code, sigma, reserved=None, planes=False):
    o = trainer.BorderOptionsC()
    o.object_code, o.sigma = code, sigma
    if reserved is not None:
        o.reserved[reserved] = 7
    if planes:
        return ts._lib.umx_trainset_border_planes(ts._handle(), index, ctypes.byref(o), None, None, None, None)
    return ts._lib.umx_trainset_border_weights(ts._handle(), index, ctypes.byref(o))


def test_refusals_leave_the_stored_map():
    anns = _three_samples()
    rng = np.random.default_rng(6)
    wmaps = [rng.random((32, 32)).astype(np.float32) for _ in range(3)]
    tr = _trainer()
    leg_hp = helpers.small_hps()["legacy_k3_x0"]
    leg = trainer.Trainer(leg_hp, model.random_blob(leg_hp), trainer.legacy_options(), batch=B)
    try:
        _, ts = _set_of(tr, anns, wmaps)
        before = _assemble_all(tr, ts)
        nan = float("nan")
        for planes in (False, True):
            for index, code, sigma, res in ((3, 3, 5.0, None), (-2, 3, 5.0, None), (0, 0, 5.0, None), (0, HP.nClasses + 1, 5.0, None),
                                            (0, 3, 0.0, None), (0, 3, 8.5, None), (0, 3, nan, None), (-1, 3, -1.0, None),
                                            (0, 3, 5.0, 0), (1, 3, 5.0, 5)):
                assert _raw(ts, index, code, sigma, res, planes) == ERR_INVALID, (planes, index, code, sigma, res)
        assert _raw(ts, -1, 3, 5.0, planes=True) == ERR_INVALID          # the diagnostics take one sample
        assert ts._lib.umx_trainset_border_weights(ts._handle(), 0, None) == ERR_INVALID
        assert ts._lib.umx_trainset_border_weights(None, 0, None) == ERR_INVALID
        with pytest.raises(umx.UmxError) as e:
            ts.border_weights(trainset.BorderOptions(5.0), 3)
        assert e.value.code == ERR_INVALID and "sample 3" in str(e.value)
        after = _assemble_all(tr, ts)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(after, before))
        # an unweighted set has no map
        S = leg_hp.imSize
        planes = np.zeros((1, leg_hp.nChannels, 1, S, S), np.float32)
        us = trainset.TrainSet.from_arrays(leg, planes, [np.ones((S, S), np.uint8)], None, trainset.UNWEIGHTED)
        for call in (lambda: us.border_weights(trainset.BorderOptions(2.0, 1)), lambda: us.border_planes(0, trainset.BorderOptions(2.0, 1))):
            with pytest.raises(umx.UmxError) as e:
                call()
            assert e.value.code == ERR_INVALID and "unweighted" in str(e.value)
    finally:
        tr.close()
        leg.close()


def test_upload_computes_the_missing_maps_only():
    anns = _three_samples()
    rng = np.random.default_rng(7)
    own = rng.random((32, 32)).astype(np.float32) * 2
    planes = rng.normal(0, 1, (3, HP.nChannels, 1, 32, 32)).astype(np.float32)
    ds = trainset.Dataset(planes, np.stack(anns), [None, own, None])
    want = [bref.border_planes(a, OBJ, 5.0)[3] for a in anns]
    assert all((w > 0).sum() >= 100 for w in want)
    tr = _trainer()
    try:
        plain = trainset.upload(tr, ds, LW)
        assert plain.border_computed == 0
        w0 = _assemble_all(tr, plain)[2]
        assert (w0[0][..., 1] == 2.0).all()               # without the option a missing map counts as 0
        ts = trainset.upload(tr, ds, LW, border=trainset.BorderOptions(5.0))
        assert ts.border_computed == 2
        data, labels, weights = _assemble_all(tr, ts)
        assert data.tobytes() == planes[:, :, 0].transpose(0, 2, 3, 1).tobytes()
        assert (weights[..., 0] == 1.0).all() and (weights[..., 2] == 5.0).all()
        for i in (0, 2):
            assert bref.ulp_distance(weights[i][..., 1], _weights_of(want[i])).max() <= 1, i
            assert (weights[i][..., 1] > 2.0).sum() == (want[i] > 0).sum()
        assert weights[1][..., 1].tobytes() == _weights_of(own).tobytes()
        all_own = trainset.upload(tr, trainset.Dataset(planes, np.stack(anns), [own, own, own]), LW, border=trainset.BorderOptions(5.0))
        assert all_own.border_computed == 0
    finally:
        tr.close()


def _write_sets(tmp_path, hp, S):
    rng = np.random.default_rng(6)
    for name, n in (("train", 5), ("valid", 2)):
        raws = (rng.random((n, hp.nChannels, 1, S, S)) ** 3 * 40000).astype(np.uint16)
        codes = [bref.blobs(S, 40 + i, 1.5, 0.7) for i in range(n)]
        ref.write_dataset(str(tmp_path / name), raws, codes, None)


def _finetune(tmp_path, mdir, out, *flags):
    return finetune.main(["--model", mdir, "--train", str(tmp_path / "train"), "--valid", str(tmp_path / "valid"), "--out", out,
                          "--steps", "4", "--eval-every", "2", "--batch", "2", "--seed", "3"] + list(flags))


def test_finetune_computes_the_maps_of_a_set_without_wt_files(tmp_path, capfd):
    hp = model.HParams(model.GRAPH_V2, 32, 1, 3, 8, 2, 3, 0, batchSize=2)            # a solo stand-in: hyper-parameters only
    mdir = str(tmp_path / "solo_like")
    os.makedirs(mdir)
    np.savez(os.path.join(mdir, model.HP_ONLY_NAME), hp=model._hp_vector(hp), mean=np.float64(0.1), std=np.float64(0.2))
    _write_sets(tmp_path, hp, 40)
    out = str(tmp_path / "out_border")
    assert _finetune(tmp_path, mdir, out, "--from-scratch", "--border-sigma", "5") == 0
    recs = [json.loads(l) for l in open(os.path.join(out, finetune.LOG_NAME))]
    assert list(recs[0]) == ["init", "border"]
    assert recs[0]["border"] == {"sigma": 5.0, "class": 2, "radius": 20, "computed": [5, 2]}
    assert [r["step"] for r in recs[1:]] == [0, 2, 4] and all(np.isfinite(r["loss"]) for r in recs[1:])
    assert np.isfinite(recs[-1]["train_loss"])
    plain = str(tmp_path / "out_plain")
    assert _finetune(tmp_path, mdir, plain, "--from-scratch") == 0
    recs0 = [json.loads(l) for l in open(os.path.join(plain, finetune.LOG_NAME))]
    assert list(recs0[0]) == ["init"] and all("border" not in r for r in recs0)
    assert recs0[-1]["train_loss"] != recs[-1]["train_loss"]             # the contour term is on
    capfd.readouterr()
    # the legacy loss takes no weights
    assert _finetune(tmp_path, "nucleiDAPI", str(tmp_path / "out_legacy"), "--border-sigma", "5") == 2
    assert "the legacy loss takes no weights" in capfd.readouterr().err
    assert not os.path.exists(str(tmp_path / "out_legacy"))
