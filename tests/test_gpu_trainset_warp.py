"""GPU tests of the rotation / zoom augmentation (include/umx_train.h: umx_warp_desc, umx_train_step_warped,
umx_trainer_assemble_warped): the assembled batch is bit-equal to tests/trainset_warp_ref.py, a row whose warp
is the identity is what the existing entries make of it, the two quarter-turn matrices are dihedral transforms of the plain entry, a
warped step is the host-fed step on the same arrays, bad descriptors are refused before anything is enqueued, the kernels stay inside
their buffers under UMX_DEBUG_GUARD, and a fine-tuning run with the new flags is reproducible."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import helpers
import trainset_ref as ref
import trainset_warp_ref as wref
from trainset_cases import MEAN, STD, _augs, _descs, _random_set, _same_bits, _state, _warps
from unmicst_amd import finetune, model, trainer, trainset, umx

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_INVALID = 1

V2_C2K3 = helpers.small_hps()["v2_duo_like"]            # 32-pixel tile
LW3 = trainset.LabelWeights(True, (1.0, 2.0, 7.0), (0.0, 15.0, 0.25))
SIGMAS = (0.75, 1.5, 4.0)                               # radii 2, 5 and 12 (the largest the kernel takes)
GAINS = (1.0, 1.5, 4.0)
IDENTITY = (1.0, 0.0, 0.0, 1.0)
QUARTER_TURNS = (((0.0, -1.0, 1.0, 0.0), 5), ((-1.0, 0.0, 0.0, -1.0), 3))   # (matrix, the transform code it equals)
# (angle, zoom) per image: every quadrant, both ends of the zoom range the sampler may draw and beyond the crop's own sample
WARPS = ((30.0, 1.25), (0.0, 1.0), (133.7, 0.5), (-171.0, 2.0), (7.0, 1.0), (0.0, 0.8), (90.0, 1.0), (261.0, 1.7))


def _ref(planes, ann, wmaps, d, a, w, table, hp, lw):
    cw, iw = (lw.class_weight, lw.intersect_weight) if lw.weighted else (None, None)
    return wref.assemble_warped(planes, ann, wmaps, d, a, w, table, hp.imSize, hp.nClasses, cw, iw)


def _cases(S, P, N, pages):
    """32 (descriptor, augmentation, warp) rows: all 8 transforms without a blur, at R = 12 (twice) and at R = 2 or 5, every gain,
    crops at the corners and edges of the sample and inside it, every page, jitter; every third image keeps the identity."""
    far, mid = S - P, (S - P) // 2
    origins = [(0, 0), (0, far), (far, 0), (far, far), (mid, mid), (0, mid), (far, mid)]
    rows, augs, warps = [], [], []
    for i in range(32):
        t = i % 8
        y0, x0 = origins[i % len(origins)]
        rows.append((i % N, i % pages, y0, x0, t, 0.25 - 0.0625 * t, 1.0 + 0.03 * (i // 8)))
        augs.append(((0, 3, 3, 1 + i % 2)[i // 8], GAINS[(i // 3) % 3]))
        angle, zoom = WARPS[(i + i // 8) % 8]
        warps.append(IDENTITY if i % 3 == 2 else trainset.warp_matrix(angle, zoom))
    moved = [(r[4], a) for r, a, w in zip(rows, augs, warps) if not wref.is_identity(w)]
    assert {t for t, a in moved if a[0] == 3} == {t for t, a in moved} == set(range(8))       # (the aug == NULL pass: all without a blur)
    assert {a for _, a in moved} >= {(l, g) for l in (0, 3) for g in GAINS}
    return rows, augs, warps


CONFIGS = {
    "v2_C2_P64_weighted": (helpers.small_hps()["v2_deep"], "duo", LW3),
    "v2_C1_P64_weighted": (model.HParams(model.GRAPH_V2, 64, 1, 3, 8, 3, 3, 0), "solo", LW3),
    "legacy_C2_P128_weighted": (model.HParams(model.GRAPH_LEGACY, 128, 2, 3, 4, 2, 3, 0), "legacy", LW3),
    "legacy_C1_P128_unweighted": (model.HParams(model.GRAPH_LEGACY, 128, 1, 2, 4, 2, 3, 0), "legacy", trainset.UNWEIGHTED),
}
OPTS = {"duo": trainer.duo_options, "solo": trainer.solo_options, "legacy": trainer.legacy_options}


@pytest.mark.parametrize("wider", [0, 17], ids=["S_eq_P", "S_gt_P"])
@pytest.mark.parametrize("which", sorted(CONFIGS))
def test_assemble_warped_is_bit_equal_to_the_restatement(which, wider):
    hp, regime, lw = CONFIGS[which]
    B, N, pages, S = 8, 3, 2, hp.imSize + wider
    planes, ann, wmaps = _random_set(hp, N, pages, S, 7)
    table = trainset.AugmentTable.from_sigmas(SIGMAS, MEAN, STD)
    tr = trainer.Trainer(hp, model.random_blob(hp, seed=3), OPTS[regime](), batch=B)
    ts = trainset.TrainSet.from_arrays(tr, planes, ann, wmaps, lw)
    rows, augs, warps = _cases(S, hp.imSize, N, pages)
    batches = [slice(b0, b0 + B) for b0 in range(0, len(rows), B)] + [slice(13, 16)]          # the last one: n < B
    for sl in batches:                                   # aug == NULL: the set has no table yet
        d, w = _descs(rows[sl]), _warps(warps[sl])
        got = tr.assemble_warped(ts, d, None, w)
        assert got[0].shape == (len(d), hp.imSize, hp.imSize, hp.nChannels)
        _same_bits(got, _ref(planes, ann, wmaps, d, None, w, None, hp, lw), (which, S, "aug NULL", sl))
        ident = [j for j in range(len(d)) if wref.is_identity(w["m"][j])]
        _same_bits(got, tr.assemble(ts, d), (which, S, "identity rows against umx_trainer_assemble"), ident)
    ts.set_augment(table)
    for sl in batches:
        d, a, w = _descs(rows[sl]), _augs(augs[sl]), _warps(warps[sl])
        got = tr.assemble_warped(ts, d, a, w)
        _same_bits(got, _ref(planes, ann, wmaps, d, a, w, table, hp, lw), (which, S, "blur and gain", sl))
        ident = [j for j in range(len(d)) if wref.is_identity(w["m"][j])]
        assert ident and len(ident) < len(d)
        _same_bits(got, tr.assemble_augmented(ts, d, a), (which, S, "identity rows against umx_trainer_assemble_augmented"), ident)
        # aug == NULL on a set with a table is still "no blur, gain 1"
        _same_bits(tr.assemble_warped(ts, d, None, w), _ref(planes, ann, wmaps, d, None, w, None, hp, lw), (which, S, "aug NULL, table", sl))
    # the warp did something: a rotated image differs from the plain one in data and in labels
    d, w = _descs(rows[:B]), _warps(warps[:B])
    plain = tr.assemble(ts, d)
    got = tr.assemble_warped(ts, d, None, w)
    assert (got[0][0] != plain[0][0]).mean() > 0.5 and (got[1][0] != plain[1][0]).mean() > 0.1
    tr.close()


@pytest.mark.parametrize("wider", [0, 9])
def test_quarter_turns_equal_the_plain_entry_with_the_matching_transform(wider):
    hp, B = V2_C2K3, 8
    P, S = hp.imSize, hp.imSize + wider
    planes, ann, wmaps = _random_set(hp, 3, 2, S, 21)
    tr = trainer.Trainer(hp, model.random_blob(hp, seed=3), trainer.duo_options(), batch=B)
    ts = trainset.TrainSet.from_arrays(tr, planes, ann, wmaps, LW3)
    far = S - P
    rows = [(j % 3, j % 2, (0, far, far // 2)[j % 3], (far, 0, far // 3)[j % 3], 0, 0.25 - 0.0625 * j, 1.0 + 0.03 * j) for j in range(B)]
    for m, code in QUARTER_TURNS:
        got = tr.assemble_warped(ts, _descs(rows), None, _warps([m] * B))
        _same_bits(got, tr.assemble(ts, _descs([r[:4] + (code,) + r[5:] for r in rows])), (m, code, S))
    tr.close()


def _step_pair(hp, blob, opts, B, planes, ann, wmaps, lw, table, batches, with_aug):
    a, b = trainer.Trainer(hp, blob, opts, batch=B), trainer.Trainer(hp, blob, opts, batch=B)
    ts = trainset.TrainSet.from_arrays(a, planes, ann, wmaps, lw)
    if with_aug:
        ts.set_augment(table)
    for d, g, w in batches:
        g = g if with_aug else None
        a.step_warped(ts, d, g, w)
        la = a.loss()
        data, labels, weights = _ref(planes, ann, wmaps, d, g, w, table, hp, lw)
        lb = b.step(data, labels, weights)
        assert la == lb
        assert a.grads().tobytes() == b.grads().tobytes()
    assert a.blob().tobytes() == b.blob().tobytes()
    assert a.step_count == b.step_count == len(batches)
    a.close()
    b.close()


@pytest.mark.parametrize("with_aug", [True, False])
def test_step_warped_is_the_host_fed_step_v2_duo(with_aug):
    hp = V2_C2K3
    planes, ann, wmaps = _random_set(hp, 4, 2, 40, 11)
    table = trainset.AugmentTable.from_sigmas(SIGMAS, MEAN, STD)
    kw = dict(blur_levels=4, blur_prob=0.6, saturate_prob=0.5, max_gain=3.0) if with_aug else {}
    s = trainset.Sampler(2, 4, 4, 40, hp.imSize, 2, 0.25, 0.025, transforms=True, rotate_prob=0.7, zoom_prob=0.5, zoom_range=(0.8, 1.25), **kw)
    batches = [s.next_warped() for _ in range(3)]
    ident = [wref.is_identity(m) for _, _, w in batches for m in w["m"]]
    assert any(ident) and not all(ident)
    _step_pair(hp, model.random_blob(hp, seed=5), trainer.duo_options(), 4, planes, ann, wmaps, LW3, table, batches, with_aug)


def test_step_warped_is_the_host_fed_step_nucleidapi():
    hp, blob, mean, std = helpers.load_nuclei_dapi()
    raws, codes, wts = ref.sample_105_crops(ref.TRAIN_ORIGINS, S=256)
    planes = ref.normalise(raws, mean, std)[:, None, None]
    table = trainset.AugmentTable.from_sigmas((1.0, 2.0, 4.0), mean, std)
    s = trainset.Sampler(3, len(raws), 16, 256, hp.imSize, 1, 0.0, 0.0, transforms=True, blur_levels=4, blur_prob=0.5,
                         saturate_prob=0.25, max_gain=2.0, rotate_prob=0.75, zoom_prob=0.5, zoom_range=(0.5, 2.0))
    batches = [s.next_warped() for _ in range(2)]
    _step_pair(hp, blob, trainer.legacy_options(), 16, planes, codes, list(wts), trainset.UNWEIGHTED, table, batches, True)


def test_refusals_enqueue_nothing():
    hp = helpers.small_hps()["legacy_k3_x0"]
    B, S = 4, 40
    planes, ann, wmaps = _random_set(hp, 3, 2, S, 1)
    blob = model.random_blob(hp)
    table = trainset.AugmentTable.from_sigmas(SIGMAS, MEAN, STD)
    rows = [(j % 3, j % 2, 2 * j, 8 - 2 * j, j, 0.0, 1.0) for j in range(B)]
    good_d = _descs(rows)
    good_a = _augs([(j % 4, GAINS[j % 3]) for j in range(B)])
    good_w = _warps([trainset.warp_matrix(*WARPS[j]) for j in range(B)])

    def fresh():
        t = trainer.Trainer(hp, blob, trainer.legacy_options(), batch=B)
        return t, trainset.TrainSet.from_arrays(t, planes, ann, wmaps, trainset.UNWEIGHTED)

    ref_tr, ref_ts = fresh()                              # what a run without any refused call gives
    want_plain = ref_tr.assemble_warped(ref_ts, good_d, None, good_w)
    ref_ts.set_augment(table)
    want_batch = ref_tr.assemble_warped(ref_ts, good_d, good_a, good_w)
    ref_tr.step_warped(ref_ts, good_d, good_a, good_w)
    want_loss, want_state = ref_tr.loss(), _state(ref_tr)

    tr, ts = fresh()
    other, _ = fresh()
    calls = (lambda a, w: tr.step_warped(ts, good_d, a, w), lambda a, w: tr.assemble_warped(ts, good_d, a, w))
    for call in calls:                                    # aug != NULL on a set without a table
        with pytest.raises(umx.UmxError) as e:
            call(good_a, good_w)
        assert e.value.code == ERR_INVALID and "table" in str(e.value)
    _same_bits(tr.assemble_warped(ts, good_d, None, good_w), want_plain, "aug NULL needs no table")
    ts.set_augment(table)
    nan, inf = float("nan"), float("inf")
    for m in ((nan, 0, 0, 1), (1, 0, inf, 1), (1, -inf, 0, 1), (4.5, 0, 0, 1), (1, 0, 0, -4.0000005), (0, 0, 0, 0), (1, 2, 2, 4), (0, 0, 1, 0)):
        bad = good_w.copy()
        bad["m"][B - 1] = m
        for call in calls:
            for a in (good_a, None):
                with pytest.raises(umx.UmxError) as e:
                    call(a, bad)
                assert e.value.code == ERR_INVALID and "warp %d" % (B - 1) in str(e.value), m
        assert tr.step_count == 0
    for level, gain in ((4, 1.0), (-1, 1.0), (1, 0.5), (1, nan)):         # a level outside the table, a bad gain
        bad = good_a.copy()
        bad[B - 1] = (level, gain)
        for call in calls:
            with pytest.raises(umx.UmxError) as e:
                call(bad, good_w)
            assert e.value.code == ERR_INVALID, (level, gain)
    with pytest.raises(umx.UmxError) as e:               # a bad sample descriptor is still refused on this entry
        tr.step_warped(ts, _descs(rows[:-1] + [(3, 0, 0, 0, 0, 0.0, 1.0)]), good_a, good_w)
    assert e.value.code == ERR_INVALID
    for call in (lambda: other.step_warped(ts, good_d, good_a, good_w), lambda: other.assemble_warped(ts, good_d, good_a, good_w)):
        with pytest.raises(umx.UmxError) as e:           # a set of another trainer
            call()
        assert e.value.code == ERR_INVALID and other.step_count == 0
    assert tr._lib.umx_train_step_warped(tr._h, ts._handle(), good_d.ctypes.data, good_a.ctypes.data, None, 1) == ERR_INVALID
    with pytest.raises(ValueError):                       # the arrays are parallel
        tr.step_warped(ts, good_d, good_a, good_w[:-1])
    assert tr.step_count == 0
    # nothing was enqueued by any refused call: the good calls give the bytes of the run that never saw one
    _same_bits(tr.assemble_warped(ts, good_d, good_a, good_w), want_batch, "after refusals")
    tr.step_warped(ts, good_d, good_a, good_w)
    assert tr.loss() == want_loss and tr.step_count == 1 and _state(tr) == want_state
    for t in (tr, other, ref_tr):
        t.close()


def _run_guarded(hp, regime, lw, monkeypatch, fill):
    """assemble_warped and step_warped on a 45-pixel set and on one whose samples are exactly one tile: every level and gain, warps
    that reach far outside the sample, with and without augmentation descriptors."""
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
            rows = [(t % 3, (pages - 1, t % pages)[t % 2], (far, 0, far, min(1, far))[t % 4], (far, far, 0, 0)[t % 4], t,
                     0.25 - 0.125 * t, 1.0 + 0.05 * t) for t in range(8)]
            augs = [((t + 1) % 4, GAINS[t % 3]) for t in range(8)]
            warps = [trainset.warp_matrix(*WARPS[t]) for t in range(8)]
            for with_aug in (False, True):
                if with_aug:
                    ts.set_augment(table)
                for j, sl in enumerate((slice(0, B), slice(B, 8), slice(B - 1, B), slice(1, B))):        # n = B, B, 1, B - 1
                    a = _augs(augs[sl]) if with_aug else None
                    for k, v in enumerate(tr.assemble_warped(ts, _descs(rows[sl]), a, _warps(warps[sl]))):
                        out["S%d.aug%d.assemble%d.%d" % (S, with_aug, j, k)] = np.zeros(0) if v is None else v
            for s in range(2):
                pick = [(s * 3 + b) % 8 for b in range(B)]
                tr.step_warped(ts, _descs([rows[i] for i in pick]), _augs([augs[i] for i in pick]), _warps([warps[i] for i in pick]))
                out["S%d.step%d.loss" % (S, s)] = np.array(tr.loss())
            out["S%d.grads" % S], out["S%d.blob" % S], out["S%d.probs" % S] = tr.grads(), tr.blob(), tr.probs()
            ts.close()
    finally:
        tr.close()
    monkeypatch.delenv("UMX_DEBUG_GUARD", raising=False)
    return out


@pytest.mark.parametrize("graph", ["legacy_unweighted", "v2"])
def test_warped_training_set_under_guards(graph, monkeypatch):
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


def test_finetune_with_rotation_and_zoom_end_to_end(tmp_path):
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
                            "--transforms", "--rotate-prob", "1", "--zoom-range", "0.8,1.25"],
                           cwd=ROOT, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-3000:]
        outs.append(out)
    logs = [open(os.path.join(o, finetune.LOG_NAME)).read() for o in outs]
    assert logs[0] == logs[1]
    recs = [json.loads(l) for l in logs[0].splitlines()]
    assert recs[0] == {"warp": {"rotate_prob": 1.0, "zoom_prob": 0.5, "zoom_range": [0.8, 1.25]}}
    assert [r["step"] for r in recs[1:]] == [0, 5, 10] and all(np.isfinite(r["loss"]) for r in recs[1:])
    assert recs[2]["train_loss"] is not None and np.isfinite(recs[2]["train_loss"])
    z = [np.load(os.path.join(o, model.CONVERTED_NAME)) for o in outs]
    assert sorted(z[0].files) == sorted(z[1].files) and all(z[0][k].tobytes() == z[1][k].tobytes() for k in z[0].files)
    arts = [model.load_model_dir(o) for o in outs]
    assert arts[0].hp == hp and np.array_equal(arts[0].blob, arts[1].blob)
