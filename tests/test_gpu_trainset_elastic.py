"""GPU tests of the elastic deformation (include/umx_train.h: umx_elastic_desc, umx_train_step_elastic, umx_trainer_assemble_elastic;
DESIGN.md section 9.2): the assembled batch is bit-equal to tests/trainset_elastic_ref.py, a row without a lattice is what the existing
entries make of it, a zero lattice is the warp, a deformed step is the host-fed step on the same arrays, bad descriptors are refused
before anything is enqueued, the kernels stay inside their buffers under UMX_DEBUG_GUARD, and a fine-tuning run with the new flags is
reproducible.  Sources far outside the sample are folded back into it: nothing here reads outside a buffer."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import helpers
import trainset_elastic_ref as eref
import trainset_ref as ref
import trainset_warp_ref as wref
from trainset_cases import MEAN, STD, _augs, _descs, _elastics, _random_set, _same_bits, _state, _warps
from unmicst_amd import finetune, model, trainer, trainset, umx

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_INVALID = 1

V2_C2K3 = helpers.small_hps()["v2_duo_like"]            # 32-pixel tile
LW3 = trainset.LabelWeights(True, (1.0, 2.0, 7.0), (0.0, 15.0, 0.25))
SIGMAS = (0.75, 1.5, 4.0)                               # radii 2, 5 and 12 (the largest the kernel takes)
GAINS = (1.0, 1.5, 4.0)
IDENTITY = (1.0, 0.0, 0.0, 1.0)
WARPS = ((30.0, 1.25), (0.0, 1.0), (133.7, 0.5), (-171.0, 2.0), (7.0, 1.0), (0.0, 0.8), (90.0, 1.0), (261.0, 1.7))


def _lattice(rng, n, sigma):
    return n, trainset.elastic_lattice(rng.standard_normal(2 * n * n), sigma, n)


def _ref(planes, ann, wmaps, d, a, w, e, table, hp, lw):
    cw, iw = (lw.class_weight, lw.intersect_weight) if lw.weighted else (None, None)
    return eref.assemble_elastic(planes, ann, wmaps, d, a, w, e, table, hp.imSize, hp.nClasses, cw, iw)


def _cases(S, P, N, pages):
    """32 (descriptor, augmentation, warp, lattice) rows: all 8 transforms; n = 0, 4, 5, 6; lattices at the descriptor's bound of +-32
    pixels on a few images (sources far outside the sample); crops at the corners and edges of the sample and inside it; no blur,
    R = 12 and a smaller radius; every gain; every third warp the identity."""
    far, mid = S - P, (S - P) // 2
    origins = [(0, 0), (0, far), (far, 0), (far, far), (mid, mid), (0, mid), (far, mid)]
    rng = np.random.default_rng(99)
    rows, augs, warps, lats = [], [], [], []
    for i in range(32):
        t = i % 8
        y0, x0 = origins[i % len(origins)]
        rows.append((i % N, i % pages, y0, x0, t, 0.25 - 0.0625 * t, 1.0 + 0.03 * (i // 8)))
        augs.append(((0, 3, 3, 1 + i % 2)[i // 8], GAINS[(i // 3) % 3]))
        angle, zoom = WARPS[(i + i // 8) % 8]
        warps.append(IDENTITY if i % 3 == 2 else trainset.warp_matrix(angle, zoom))
        n = (4, 0, 5, 6, 5)[i % 5]
        if n == 0:
            lats.append(None)
        elif i % 7 == 3:                                 # every lattice value at +-32
            d = np.zeros((2, 6, 6), np.float32)
            d[:, :n, :n] = np.where(rng.random((2, n, n)) < 0.5, -32.0, 32.0)
            lats.append((n, d))
        else:
            lats.append(_lattice(rng, n, (1.0, 2.5, 6.0)[i % 3]))
    deformed = [(r[4], a, l[0], wref.is_identity(w)) for r, a, w, l in zip(rows, augs, warps, lats) if l is not None]
    assert {t for t, _, _, _ in deformed} == set(range(8)) and {n for _, _, n, _ in deformed} == {4, 5, 6}
    assert {a[0] for _, a, _, _ in deformed} == {0, 1, 2, 3} and {a[1] for _, a, _, _ in deformed} == set(GAINS)
    assert {i for _, _, _, i in deformed} == {True, False} and sum(l is None for l in lats) >= 6
    assert sum(l is not None and abs(l[1]).max() == 32.0 for l in lats) >= 3
    return rows, augs, warps, lats


CONFIGS = {
    "v2_C2_P32_weighted": (V2_C2K3, "duo", LW3),
    "v2_C1_P64_weighted": (model.HParams(model.GRAPH_V2, 64, 1, 3, 8, 3, 3, 0), "solo", LW3),
    "legacy_C1_P128_unweighted": (model.HParams(model.GRAPH_LEGACY, 128, 1, 2, 4, 2, 3, 0), "legacy", trainset.UNWEIGHTED),
}
OPTS = {"duo": trainer.duo_options, "solo": trainer.solo_options, "legacy": trainer.legacy_options}


@pytest.mark.parametrize("wider", [0, 17], ids=["S_eq_P", "S_gt_P"])
@pytest.mark.parametrize("which", sorted(CONFIGS))
def test_assemble_elastic_is_bit_equal_to_the_restatement(which, wider):
    hp, regime, lw = CONFIGS[which]
    B, N, pages, S = 8, 3, 2, hp.imSize + wider
    planes, ann, wmaps = _random_set(hp, N, pages, S, 7)
    table = trainset.AugmentTable.from_sigmas(SIGMAS, MEAN, STD)
    tr = trainer.Trainer(hp, model.random_blob(hp, seed=3), OPTS[regime](), batch=B)
    ts = trainset.TrainSet.from_arrays(tr, planes, ann, wmaps, lw)
    rows, augs, warps, lats = _cases(S, hp.imSize, N, pages)
    batches = [slice(b0, b0 + B) for b0 in range(0, len(rows), B)] + [slice(13, 16)]          # the last one: n < B
    for sl in batches:                                   # aug == NULL: the set has no table yet
        d, w, e = _descs(rows[sl]), _warps(warps[sl]), _elastics(lats[sl])
        plain = [j for j in range(len(d)) if e["n"][j] == 0]
        got = tr.assemble_elastic(ts, d, None, None, e)
        assert got[0].shape == (len(d), hp.imSize, hp.imSize, hp.nChannels)
        _same_bits(got, _ref(planes, ann, wmaps, d, None, None, e, None, hp, lw), (which, S, "aug NULL, warp NULL", sl))
        _same_bits(got, tr.assemble(ts, d), (which, S, "n == 0 rows against umx_trainer_assemble"), plain)
        got = tr.assemble_elastic(ts, d, None, w, e)
        _same_bits(got, _ref(planes, ann, wmaps, d, None, w, e, None, hp, lw), (which, S, "aug NULL", sl))
        _same_bits(got, tr.assemble_warped(ts, d, None, w), (which, S, "n == 0 rows against umx_trainer_assemble_warped"), plain)
    ts.set_augment(table)
    for sl in batches:
        d, a, w, e = _descs(rows[sl]), _augs(augs[sl]), _warps(warps[sl]), _elastics(lats[sl])
        plain = [j for j in range(len(d)) if e["n"][j] == 0]
        assert len(plain) < len(d) and (plain or len(d) < B)
        got = tr.assemble_elastic(ts, d, a, w, e)
        _same_bits(got, _ref(planes, ann, wmaps, d, a, w, e, table, hp, lw), (which, S, "blur, gain and warp", sl))
        _same_bits(got, tr.assemble_warped(ts, d, a, w), (which, S, "n == 0 rows against umx_trainer_assemble_warped"), plain)
        got = tr.assemble_elastic(ts, d, a, None, e)
        _same_bits(got, _ref(planes, ann, wmaps, d, a, None, e, table, hp, lw), (which, S, "warp NULL", sl))
        _same_bits(got, tr.assemble_augmented(ts, d, a), (which, S, "n == 0 rows against umx_trainer_assemble_augmented"), plain)
    # a zero lattice is the warp: with matrices other than the identity under every blur and gain, and with the identity where there is
    # no blur (an unwarped blur replicates the sample's edge, the lattice code mirrors it as the warp code does)
    zero = _elastics([(4, np.zeros((2, 6, 6), np.float32))] * B)
    d, a = _descs(rows[8:16]), _augs(augs[8:16])
    turned = _warps([trainset.warp_matrix(*WARPS[(j % 7) + (j % 7 >= 1)]) for j in range(B)])
    assert not any(wref.is_identity(m) for m in turned["m"])
    _same_bits(tr.assemble_elastic(ts, d, a, turned, zero), tr.assemble_warped(ts, d, a, turned), (which, S, "zero lattice"))
    w = _warps(warps[8:16])
    _same_bits(tr.assemble_elastic(ts, d, None, w, zero), tr.assemble_warped(ts, d, None, w), (which, S, "zero lattice, no blur"))
    _same_bits(tr.assemble_elastic(ts, d, None, None, zero), tr.assemble(ts, d), (which, S, "zero lattice, nothing else"))
    # a real deformation changes the image and some of its labels
    rng = np.random.default_rng(4)
    bent = _elastics([_lattice(rng, 5, 3.0) for _ in range(B)])
    plain, got = tr.assemble(ts, d), tr.assemble_elastic(ts, d, None, None, bent)
    for j in range(B):
        assert (got[0][j] != plain[0][j]).mean() > 0.5 and (got[1][j] != plain[1][j]).any()
    tr.close()


@pytest.mark.parametrize("with_aug", [True, False])
def test_step_elastic_is_the_host_fed_step_v2_duo(with_aug):
    hp, B = V2_C2K3, 4
    planes, ann, wmaps = _random_set(hp, 4, 2, 40, 11)
    table = trainset.AugmentTable.from_sigmas(SIGMAS, MEAN, STD)
    kw = dict(blur_levels=4, blur_prob=0.6, saturate_prob=0.5, max_gain=3.0) if with_aug else {}
    s = trainset.Sampler(2, 4, B, 40, hp.imSize, 2, 0.25, 0.025, transforms=True, rotate_prob=0.7, zoom_prob=0.5, zoom_range=(0.8, 1.25),
                         elastic_prob=0.7, elastic_sigma=1.5, elastic_grid=2, **kw)
    batches = [s.next_elastic() for _ in range(3)]
    ns = [int(n) for _, _, _, e in batches for n in e["n"]]
    assert 0 in ns and 5 in ns
    blob, opts = model.random_blob(hp, seed=5), trainer.duo_options()
    a, b = trainer.Trainer(hp, blob, opts, batch=B), trainer.Trainer(hp, blob, opts, batch=B)
    ts = trainset.TrainSet.from_arrays(a, planes, ann, wmaps, LW3)
    if with_aug:
        ts.set_augment(table)
    for k, (d, g, w, e) in enumerate(batches):
        g = g if with_aug else None
        w = None if k == 2 else w                         # once without the warp descriptors
        a.step_elastic(ts, d, g, w, e)
        la = a.loss()
        data, labels, weights = _ref(planes, ann, wmaps, d, g, w, e, table, hp, LW3)
        lb = b.step(data, labels, weights)
        assert la == lb
        assert a.grads().tobytes() == b.grads().tobytes()
    assert a.blob().tobytes() == b.blob().tobytes()
    assert a.step_count == b.step_count == len(batches)
    a.close()
    b.close()


def test_refusals_enqueue_nothing():
    hp = helpers.small_hps()["legacy_k3_x0"]
    B, S = 4, 40
    planes, ann, wmaps = _random_set(hp, 3, 2, S, 1)
    blob = model.random_blob(hp)
    table = trainset.AugmentTable.from_sigmas(SIGMAS, MEAN, STD)
    rows = [(j % 3, j % 2, 2 * j, 8 - 2 * j, j, 0.0, 1.0) for j in range(B)]
    rng = np.random.default_rng(8)
    good_d = _descs(rows)
    good_a = _augs([(j % 4, GAINS[j % 3]) for j in range(B)])
    good_w = _warps([trainset.warp_matrix(*WARPS[j]) for j in range(B)])
    good_e = _elastics([_lattice(rng, 4, 2.0), None, _lattice(rng, 6, 4.0), _lattice(rng, 5, 1.0)])

    def fresh():
        t = trainer.Trainer(hp, blob, trainer.legacy_options(), batch=B)
        return t, trainset.TrainSet.from_arrays(t, planes, ann, wmaps, trainset.UNWEIGHTED)

    ref_tr, ref_ts = fresh()                              # what a run without any refused call gives
    want_plain = ref_tr.assemble_elastic(ref_ts, good_d, None, None, good_e)
    ref_ts.set_augment(table)
    want_batch = ref_tr.assemble_elastic(ref_ts, good_d, good_a, good_w, good_e)
    ref_tr.step_elastic(ref_ts, good_d, good_a, good_w, good_e)
    want_loss, want_state = ref_tr.loss(), _state(ref_tr)

    tr, ts = fresh()
    other, _ = fresh()
    calls = (lambda a, w, e: tr.step_elastic(ts, good_d, a, w, e), lambda a, w, e: tr.assemble_elastic(ts, good_d, a, w, e))
    for call in calls:                                    # aug != NULL on a set without a table
        with pytest.raises(umx.UmxError) as err:
            call(good_a, good_w, good_e)
        assert err.value.code == ERR_INVALID and "table" in str(err.value)
    _same_bits(tr.assemble_elastic(ts, good_d, None, None, good_e), want_plain, "aug NULL needs no table")
    ts.set_augment(table)
    nan, inf = float("nan"), float("inf")

    def broken(at, kw):
        e = good_e.copy()
        for k, v in kw.items():
            if k == "n":
                e["n"][at] = v
            elif k == "reserved":
                e["reserved"][at][v] = 1
            else:
                e["d"][at][k] = v
        return e

    # every rule of umx_elastic_desc_check, on the last descriptor or on the one without a lattice
    for at, kw in ((3, dict(n=3)), (3, dict(n=7)), (1, dict(n=-1)), (3, dict(reserved=0)), (1, dict(reserved=2)), (3, {(0, 1, 1): nan}),
                   (3, {(1, 5, 5): inf}), (3, {(0, 0, 0): 32.5}), (3, {(1, 2, 2): -33.0}), (3, {(0, 5, 0): 1.0}), (3, {(1, 0, 5): -1.0}),
                   (1, {(0, 0, 0): 1.0})):
        bad = broken(at, kw)
        for call in calls:
            for a, w in ((good_a, good_w), (None, None), (None, good_w)):
                with pytest.raises(umx.UmxError) as err:
                    call(a, w, bad)
                assert err.value.code == ERR_INVALID and "elastic %d " % at in str(err.value), kw
        assert tr.step_count == 0
    for m in ((nan, 0, 0, 1), (4.5, 0, 0, 1), (0, 0, 0, 0)):              # a bad warp is still refused on this entry
        bad = good_w.copy()
        bad["m"][B - 1] = m
        for call in calls:
            with pytest.raises(umx.UmxError) as err:
                call(good_a, bad, good_e)
            assert err.value.code == ERR_INVALID and "warp %d" % (B - 1) in str(err.value), m
    for level, gain in ((4, 1.0), (-1, 1.0), (1, 0.5), (1, nan)):         # and a bad augmentation
        bad = good_a.copy()
        bad[B - 1] = (level, gain)
        for call in calls:
            with pytest.raises(umx.UmxError) as err:
                call(bad, good_w, good_e)
            assert err.value.code == ERR_INVALID, (level, gain)
    with pytest.raises(umx.UmxError) as err:             # and a bad sample descriptor
        tr.step_elastic(ts, _descs(rows[:-1] + [(3, 0, 0, 0, 0, 0.0, 1.0)]), good_a, good_w, good_e)
    assert err.value.code == ERR_INVALID
    for call in (lambda: other.step_elastic(ts, good_d, good_a, good_w, good_e),
                 lambda: other.assemble_elastic(ts, good_d, good_a, good_w, good_e)):
        with pytest.raises(umx.UmxError) as err:         # a set of another trainer
            call()
        assert err.value.code == ERR_INVALID and other.step_count == 0
    L = tr._lib                                           # a NULL elastic array
    assert L.umx_train_step_elastic(tr._h, ts._handle(), good_d.ctypes.data, good_a.ctypes.data, good_w.ctypes.data, None, 1) == ERR_INVALID
    out = [np.zeros((B, hp.imSize, hp.imSize, c), np.float32) for c in (hp.nChannels, hp.nClasses)]
    assert L.umx_trainer_assemble_elastic(tr._h, ts._handle(), good_d.ctypes.data, None, None, None, B, out[0].ctypes.data,
                                          out[1].ctypes.data, None) == ERR_INVALID
    with pytest.raises(ValueError):                       # the arrays are parallel
        tr.step_elastic(ts, good_d, good_a, good_w, good_e[:-1])
    assert tr.step_count == 0
    # nothing was enqueued by any refused call: the good calls give the bytes of the run that never saw one
    _same_bits(tr.assemble_elastic(ts, good_d, good_a, good_w, good_e), want_batch, "after refusals")
    tr.step_elastic(ts, good_d, good_a, good_w, good_e)
    assert tr.loss() == want_loss and tr.step_count == 1 and _state(tr) == want_state
    for t in (tr, other, ref_tr):
        t.close()


def _run_guarded(hp, regime, lw, monkeypatch, fill):
    """assemble_elastic and step_elastic on a 45-pixel set and on one whose samples are exactly one tile: every level and gain, lattices
    that reach far outside the sample, with and without augmentation and warp descriptors."""
    if fill is None:
        monkeypatch.delenv("UMX_DEBUG_GUARD", raising=False)
    else:
        monkeypatch.setenv("UMX_DEBUG_GUARD", fill)
    B, pages, P = 4, 3, hp.imSize
    table = trainset.AugmentTable.from_sigmas(SIGMAS, MEAN, STD)
    tr = trainer.Trainer(hp, model.random_blob(hp, seed=9), OPTS[regime](), batch=B)
    out = {}
    try:
        for S in (45, P):
            planes, ann, wmaps = _random_set(hp, 3, pages, S, S)
            ts = trainset.TrainSet.from_arrays(tr, planes, ann, wmaps, lw)
            far = S - P
            rng = np.random.default_rng(S)
            rows = [(t % 3, (pages - 1, t % pages)[t % 2], (far, 0, far, min(1, far))[t % 4], (far, far, 0, 0)[t % 4], t,
                     0.25 - 0.125 * t, 1.0 + 0.05 * t) for t in range(8)]
            augs = [((t + 1) % 4, GAINS[t % 3]) for t in range(8)]
            warps = [trainset.warp_matrix(*WARPS[t]) for t in range(8)]
            lats = [None if t == 5 else _lattice(rng, 4 + t % 3, (2.0, 16.0)[t % 2]) for t in range(8)]
            for with_aug in (False, True):
                if with_aug:
                    ts.set_augment(table)
                for j, sl in enumerate((slice(0, B), slice(B, 8), slice(B - 1, B), slice(1, B))):        # n = B, B, 1, B - 1
                    a = _augs(augs[sl]) if with_aug else None
                    w = _warps(warps[sl]) if j % 2 == 0 else None
                    for k, v in enumerate(tr.assemble_elastic(ts, _descs(rows[sl]), a, w, _elastics(lats[sl]))):
                        out["S%d.aug%d.assemble%d.%d" % (S, with_aug, j, k)] = np.zeros(0) if v is None else v
            for s in range(2):
                pick = [(s * 3 + b) % 8 for b in range(B)]
                tr.step_elastic(ts, _descs([rows[i] for i in pick]), _augs([augs[i] for i in pick]), _warps([warps[i] for i in pick]),
                                _elastics([lats[i] for i in pick]))
                out["S%d.step%d.loss" % (S, s)] = np.array(tr.loss())
            out["S%d.grads" % S], out["S%d.blob" % S], out["S%d.probs" % S] = tr.grads(), tr.blob(), tr.probs()
            ts.close()
    finally:
        tr.close()
    monkeypatch.delenv("UMX_DEBUG_GUARD", raising=False)
    return out


@pytest.mark.parametrize("graph", ["legacy_unweighted", "v2"])
def test_elastic_training_set_under_guards(graph, monkeypatch):
    """Every call checks every red zone (UMX_ERR_GUARD otherwise); the results do not depend on the fill byte and equal the
    unguarded run's."""
    if graph == "v2":
        hp, regime, lw = V2_C2K3, "duo", LW3
    else:
        hp, regime, lw = model.HParams(model.GRAPH_LEGACY, 32, 1, 2, 8, 2, 3, 0), "legacy", trainset.UNWEIGHTED
    got = {fill: _run_guarded(hp, regime, lw, monkeypatch, fill) for fill in ("0x00", "0xff")}
    plain = _run_guarded(hp, regime, lw, monkeypatch, None)
    assert all(np.isfinite(v).all() for v in plain.values())
    for fill, out in got.items():
        assert out.keys() == plain.keys()
        for k in out:
            x, y = np.asarray(out[k]), np.asarray(plain[k])
            assert x.shape == y.shape and x.tobytes() == y.tobytes(), (graph, fill, k)


def test_finetune_with_elastic_deformation_end_to_end(tmp_path):
    hp, blob, mean, std = helpers.load_nuclei_dapi()
    mdir = str(tmp_path / "models" / "nucleiDAPI")
    model.save_converted(model.ModelArtefacts(hp, blob, mean, std), mdir)
    rng = np.random.default_rng(6)                        # a small synthetic set: 6 + 2 samples of exactly one tile
    S = hp.imSize
    for name, n in (("train", 6), ("valid", 2)):
        raws = (rng.random((n, S, S)) ** 3 * 40000).astype(np.uint16)
        codes = rng.integers(1, hp.nClasses + 1, (n, S, S)).astype(np.uint8)
        ref.write_dataset(str(tmp_path / name), raws, codes, None)
    outs = []
    for k in range(2):
        out = str(tmp_path / ("out%d" % k))
        r = subprocess.run([sys.executable, "-m", "unmicst_amd.finetune", "--model", mdir, "--train", str(tmp_path / "train"), "--valid",
                            str(tmp_path / "valid"), "--out", out, "--steps", "10", "--eval-every", "5", "--seed", "9", "--batch", "4",
                            "--transforms", "--elastic-sigma", "3", "--elastic-grid", "2", "--elastic-prob", "1"],
                           cwd=ROOT, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-3000:]
        outs.append(out)
    logs = [open(os.path.join(o, finetune.LOG_NAME)).read() for o in outs]
    assert logs[0] == logs[1]
    recs = [json.loads(l) for l in logs[0].splitlines()]
    assert recs[0] == {"elastic": {"prob": 1.0, "sigma": 3.0, "grid": 2}}
    assert [r["step"] for r in recs[1:]] == [0, 5, 10] and all(np.isfinite(r["loss"]) for r in recs[1:])
    assert recs[2]["train_loss"] is not None and np.isfinite(recs[2]["train_loss"])
    z = [np.load(os.path.join(o, model.CONVERTED_NAME)) for o in outs]
    assert sorted(z[0].files) == sorted(z[1].files) and all(z[0][k].tobytes() == z[1][k].tobytes() for k in z[0].files)
    arts = [model.load_model_dir(o) for o in outs]
    assert arts[0].hp == hp and np.array_equal(arts[0].blob, arts[1].blob)
