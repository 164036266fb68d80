"""GPU tests of the computed defocus / saturation augmentation (include/umx_train.h: umx_trainset_set_augment,
umx_train_step_augmented, umx_trainer_assemble_augmented): the assembled batch is bit-equal to
tests/trainset_augment_ref.py, an image with (level 0, gain 1) is what the plain entries make of it, an augmented step is the
host-fed step on the same arrays, bad augmentation descriptors are refused before anything is enqueued, the kernel stays inside
its buffers under UMX_DEBUG_GUARD, and a fine-tuning run with the new flags is reproducible and saves a model that loads."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import helpers
import trainset_augment_ref as aref
import trainset_ref as ref
from trainset_cases import MEAN, STD, _augs, _descs, _random_set, _same_bits, _state
from unmicst_amd import finetune, model, tiffio, trainer, trainset, umx

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_INVALID = 1

V2_C2K3 = helpers.small_hps()["v2_duo_like"]            # 32-pixel tile: one workgroup tile per image
LEG_P16 = helpers.small_hps()["legacy_k3_x2"]           # 16-pixel tile, 2 channels: smaller than the kernel's tile
LW3 = trainset.LabelWeights(True, (1.0, 2.0, 7.0), (0.0, 15.0, 0.25))
SIGMAS = (0.75, 1.5, 4.0)                               # radii 2, 5 and 12 (the largest the kernel takes)
GAINS = (1.0, 1.5, 4.0)


def _ref(planes, ann, wmaps, d, a, table, hp, lw):
    cw, iw = (lw.class_weight, lw.intersect_weight) if lw.weighted else (None, None)
    return aref.assemble_augmented(planes, ann, wmaps, d, a, table, hp.imSize, hp.nClasses, cw, iw)


def _cases(S, P, N, pages):
    """40 (descriptor, augmentation) rows: every level with every transform, every gain with every level, crops at the four corners
    and edges of the sample (the clamp) and inside it (real neighbours), every page."""
    far, mid = S - P, (S - P) // 2
    origins = [(0, 0), (0, far), (far, 0), (far, far), (0, mid), (mid, 0), (far, mid), (mid, far), (mid, mid), (1, far - 1)]
    rows, augs = [], []
    for i in range(32):
        level, t = i // 8, i % 8
        y0, x0 = origins[i % len(origins)]
        rows.append((i % N, i % pages, y0, x0, t, 0.25 - 0.0625 * t, 1.0 + 0.03 * level))
        augs.append((level, GAINS[(level + t) % 3]))
    for i, (y0, x0) in enumerate(origins[:4] + origins[8:9] + origins[4:7]):   # the largest radius at every corner, inside, on edges
        rows.append(((i + 1) % N, (i + 1) % pages, y0, x0, (3 * i + 4) % 8, -0.125, 0.9))
        augs.append((3, GAINS[i % 3]))
    assert {(a[0], r[4]) for r, a in zip(rows, augs)} >= {(l, t) for l in range(4) for t in range(8)}
    assert {a for a in augs} >= {(l, g) for l in range(4) for g in GAINS}
    assert {(r[2], r[3]) for r, a in zip(rows, augs) if a[0] == 3} >= set(origins[:9])
    return rows, augs


@pytest.mark.parametrize("which", ["v2_C2K3_weighted_S130", "nucleiDAPI_unweighted_S257", "legacy_P16_C2_S45"])
def test_assemble_augmented_is_bit_equal_to_the_restatement(which):
    if which.startswith("v2"):
        hp, blob, opts, lw, B, S = V2_C2K3, model.random_blob(V2_C2K3, seed=3), trainer.duo_options(), LW3, 8, 130
    elif which.startswith("nuclei"):
        hp, blob, _, _ = helpers.load_nuclei_dapi()
        opts, lw, B, S = trainer.legacy_options(), trainset.UNWEIGHTED, 16, 257
    else:
        hp, blob, opts, lw, B, S = LEG_P16, model.random_blob(LEG_P16, seed=3), trainer.legacy_options(), trainset.UNWEIGHTED, 8, 45
    N, pages = 3, 2
    planes, ann, wmaps = _random_set(hp, N, pages, S, 7)
    table = trainset.AugmentTable.from_sigmas(SIGMAS, MEAN, STD)
    assert table.radius == (0, 2, 5, 12)
    tr = trainer.Trainer(hp, blob, opts, batch=B)
    ts = trainset.TrainSet.from_arrays(tr, planes, ann, wmaps, lw)
    ts.set_augment(table)
    rows, augs = _cases(S, hp.imSize, N, pages)
    batches = [(rows[b0:b0 + B], augs[b0:b0 + B]) for b0 in range(0, len(rows), B)] + [(rows[29:32], augs[29:32])]
    assert any(len(r) < B for r, _ in batches)           # a short batch
    for r, a in batches:
        d, g = _descs(r), _augs(a)
        got = tr.assemble_augmented(ts, d, g)
        want = _ref(planes, ann, wmaps, d, g, table, hp, lw)
        assert got[0].shape == (len(d), hp.imSize, hp.imSize, hp.nChannels)
        _same_bits(got, want, which)
    # the clip did something and left something: some pixels sit on the ceiling, others do not
    s = tr.assemble_augmented(ts, _descs([r[:5] + (0.0, 1.0) for r in rows[:B]]), _augs([(0, 4.0)] * B))[0]
    ceiling = np.float32((1.0 - np.float64(np.float32(MEAN))) / np.float64(np.float32(STD)))
    assert 0.05 < float((s == ceiling).mean()) < 0.95
    tr.close()


@pytest.mark.parametrize("which", ["v2", "legacy"])
def test_level_0_gain_1_is_the_plain_path(which):
    hp = V2_C2K3 if which == "v2" else helpers.small_hps()["legacy_k3_x0"]
    opts, lw = (trainer.duo_options(), LW3) if which == "v2" else (trainer.legacy_options(), trainset.UNWEIGHTED)
    B, S, N, pages = 4, 50, 4, 2
    planes, ann, wmaps = _random_set(hp, N, pages, S, 11)
    blob = model.random_blob(hp, seed=5)
    table = trainset.AugmentTable.from_sigmas(SIGMAS, MEAN, STD)
    a, b = trainer.Trainer(hp, blob, opts, batch=B), trainer.Trainer(hp, blob, opts, batch=B)
    tsa, tsb = (trainset.TrainSet.from_arrays(t, planes, ann, wmaps, lw) for t in (a, b))
    tsa.set_augment(table)
    none = _augs([(0, 1.0)] * B)
    s = trainset.Sampler(2, N, B, S, hp.imSize, pages, 0.25, 0.025, transforms=True)
    descs = [s.next() for _ in range(3)]
    for d in descs:
        _same_bits(a.assemble_augmented(tsa, d, none), b.assemble(tsb, d), which)
    _same_bits(a.assemble_augmented(tsa, descs[0][:2], none[:2]), b.assemble(tsb, descs[0][:2]), which)
    for d in descs:
        a.step_augmented(tsa, d, none)
        b.step_sampled(tsb, d)
        assert a.loss() == b.loss()
    assert a.step_count == b.step_count == 3
    assert _state(a) == _state(b)
    a.close()
    b.close()


def _step_pair(hp, blob, opts, B, planes, ann, wmaps, lw, table, batches):
    a, b = trainer.Trainer(hp, blob, opts, batch=B), trainer.Trainer(hp, blob, opts, batch=B)
    ts = trainset.TrainSet.from_arrays(a, planes, ann, wmaps, lw)
    ts.set_augment(table)
    for d, g in batches:
        a.step_augmented(ts, d, g)
        la = a.loss()
        data, labels, weights = _ref(planes, ann, wmaps, d, g, table, hp, lw)
        lb = b.step(data, labels, weights)
        assert la == lb
        assert a.grads().tobytes() == b.grads().tobytes()
    assert a.blob().tobytes() == b.blob().tobytes()
    assert a.step_count == b.step_count == len(batches)
    a.close()
    b.close()


def test_step_augmented_is_the_host_fed_step_v2_duo():
    hp = V2_C2K3
    planes, ann, wmaps = _random_set(hp, 4, 2, 40, 11)
    table = trainset.AugmentTable.from_sigmas(SIGMAS, MEAN, STD)
    s = trainset.Sampler(2, 4, 4, 40, hp.imSize, 2, 0.25, 0.025, transforms=True, blur_levels=4, blur_prob=0.6, saturate_prob=0.5,
                         max_gain=3.0)
    batches = [s.next_augmented() for _ in range(3)]
    assert any((g["blur_level"] != 0).any() for _, g in batches) and any((g["gain"] != 1).any() for _, g in batches)
    _step_pair(hp, model.random_blob(hp, seed=5), trainer.duo_options(), 4, planes, ann, wmaps, LW3, table, batches)


def test_step_augmented_is_the_host_fed_step_nucleidapi():
    hp, blob, mean, std = helpers.load_nuclei_dapi()
    raws, codes, wts = ref.sample_105_crops(ref.TRAIN_ORIGINS, S=256)
    planes = ref.normalise(raws, mean, std)[:, None, None]
    table = trainset.AugmentTable.from_sigmas((1.0, 2.0, 4.0), mean, std)
    s = trainset.Sampler(3, len(raws), 16, 256, hp.imSize, 1, 0.0, 0.0, transforms=True, blur_levels=4, blur_prob=0.5,
                         saturate_prob=0.25, max_gain=2.0)
    batches = [s.next_augmented() for _ in range(3)]
    _step_pair(hp, blob, trainer.legacy_options(), 16, planes, codes, list(wts), trainset.UNWEIGHTED, table, batches)


def test_refusals_enqueue_nothing():
    hp = helpers.small_hps()["legacy_k3_x0"]
    B, S = 4, 40
    planes, ann, wmaps = _random_set(hp, 3, 2, S, 1)
    blob = model.random_blob(hp)
    table = trainset.AugmentTable.from_sigmas(SIGMAS, MEAN, STD)
    rows = [(j % 3, j % 2, 2 * j, 8 - 2 * j, j, 0.0, 1.0) for j in range(B)]
    good_a = _augs([(j % 4, GAINS[j % 3]) for j in range(B)])
    good_d = _descs(rows)

    def fresh():
        t = trainer.Trainer(hp, blob, trainer.legacy_options(), batch=B)
        return t, trainset.TrainSet.from_arrays(t, planes, ann, wmaps, trainset.UNWEIGHTED)

    ref_tr, ref_ts = fresh()                              # what a run without any refused call gives
    ref_ts.set_augment(table)
    want_batch = ref_tr.assemble_augmented(ref_ts, good_d, good_a)
    ref_tr.step_augmented(ref_ts, good_d, good_a)
    want_loss, want_state = ref_tr.loss(), _state(ref_tr)

    tr, ts = fresh()
    other, _ = fresh()
    calls = (lambda a: tr.step_augmented(ts, good_d, a), lambda a: tr.assemble_augmented(ts, good_d, a))
    for call in calls:                                    # no table attached
        with pytest.raises(umx.UmxError) as e:
            call(good_a)
        assert e.value.code == ERR_INVALID and "table" in str(e.value)
    ts.set_augment(table)
    for level, gain in ((4, 1.0), (-1, 1.0), (16, 2.0), (1, 0.5), (0, 0.5), (1, float("nan")), (0, float("inf")), (2, -1.0)):
        bad = good_a.copy()
        bad[B - 1] = (level, gain)
        for call in calls:
            with pytest.raises(umx.UmxError) as e:
                call(bad)
            assert e.value.code == ERR_INVALID, (level, gain)
        assert tr.step_count == 0
    with pytest.raises(umx.UmxError) as e:               # a bad sample descriptor is still refused on this entry
        tr.step_augmented(ts, _descs(rows[:-1] + [(3, 0, 0, 0, 0, 0.0, 1.0)]), good_a)
    assert e.value.code == ERR_INVALID
    for call in (lambda: other.step_augmented(ts, good_d, good_a), lambda: other.assemble_augmented(ts, good_d, good_a)):
        with pytest.raises(umx.UmxError) as e:           # a set of another trainer
            call()
        assert e.value.code == ERR_INVALID and other.step_count == 0
    with pytest.raises(ValueError):                       # the arrays are parallel
        tr.step_augmented(ts, good_d, good_a[:-1])
    bad_table = table.c_struct()
    bad_table.radius[1] = 13
    assert tr._lib.umx_trainset_set_augment(ts._handle(), ctypes.byref(bad_table)) == ERR_INVALID      # (the table attached before stays)
    # nothing was enqueued by any refused call: the good calls give the bytes of the run that never saw one
    _same_bits(tr.assemble_augmented(ts, good_d, good_a), want_batch, "after refusals")
    tr.step_augmented(ts, good_d, good_a)
    assert tr.loss() == want_loss and tr.step_count == 1 and _state(tr) == want_state
    for t in (tr, other, ref_tr):
        t.close()


def _run_guarded(hp, regime, lw, monkeypatch, fill):
    """assemble_augmented and step_augmented on a 45-pixel set and on one whose samples are exactly one tile, every level and gain."""
    if fill is None:
        monkeypatch.delenv("UMX_DEBUG_GUARD", raising=False)
    else:
        monkeypatch.setenv("UMX_DEBUG_GUARD", fill)
    B, pages, P = 4, 3, hp.imSize
    opts = trainer.duo_options() if regime == "duo" else trainer.legacy_options()
    table = trainset.AugmentTable.from_sigmas(SIGMAS, MEAN, STD)
    tr = trainer.Trainer(hp, model.random_blob(hp, seed=9), opts, batch=B)
    out = {}
    try:
        for S in (45, P):
            planes, ann, wmaps = _random_set(hp, 3, pages, S, S)
            ts = trainset.TrainSet.from_arrays(tr, planes, ann, wmaps, lw)
            ts.set_augment(table)
            far = S - P
            rows = [(t % 3, (pages - 1, t % pages)[t % 2], (far, 0, far, min(1, far))[t % 4], (far, far, 0, 0)[t % 4], t,
                     0.25 - 0.125 * t, 1.0 + 0.05 * t) for t in range(8)]
            augs = [((t + 1) % 4, GAINS[t % 3]) for t in range(8)]
            for j, sl in enumerate((slice(0, B), slice(B, 8), slice(B - 1, B), slice(1, B))):        # n = B, B, 1, B - 1
                for k, a in enumerate(tr.assemble_augmented(ts, _descs(rows[sl]), _augs(augs[sl]))):
                    out["S%d.assemble%d.%d" % (S, j, k)] = np.zeros(0) if a is None else a
            for s in range(2):
                pick = [(s * 3 + b) % 8 for b in range(B)]
                tr.step_augmented(ts, _descs([rows[i] for i in pick]), _augs([augs[i] for i in pick]))
                out["S%d.step%d.loss" % (S, s)] = np.array(tr.loss())
            out["S%d.grads" % S], out["S%d.blob" % S], out["S%d.probs" % S] = tr.grads(), tr.blob(), tr.probs()
            ts.close()
    finally:
        tr.close()
    monkeypatch.delenv("UMX_DEBUG_GUARD", raising=False)
    return out


@pytest.mark.parametrize("graph", ["legacy_unweighted", "v2"])
def test_augmented_training_set_under_guards(graph, monkeypatch):
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


def test_finetune_with_blur_and_saturation_end_to_end(tmp_path):
    hp, blob, mean, std = helpers.load_nuclei_dapi()
    mdir = str(tmp_path / "models" / "nucleiDAPI")
    model.save_converted(model.ModelArtefacts(hp, blob, mean, std), mdir)
    raws, codes, wts = ref.sample_105_crops(ref.TRAIN_ORIGINS, S=256)
    ref.write_dataset(str(tmp_path / "train"), raws, codes, wts)
    raws, codes, wts = ref.sample_105_crops(ref.VALID_ORIGINS, S=256)
    ref.write_dataset(str(tmp_path / "valid"), raws, codes, wts)
    outs = []
    for k in range(2):
        out = str(tmp_path / ("out%d" % k))
        r = subprocess.run([sys.executable, "-m", "unmicst_amd.finetune", "--model", mdir, "--train", str(tmp_path / "train"), "--valid",
                            str(tmp_path / "valid"), "--out", out, "--steps", "20", "--eval-every", "10", "--seed", "9", "--transforms",
                            "--blur-sigmas", "1,2", "--blur-prob", "0.5", "--saturate-prob", "0.25", "--max-gain", "2"],
                           cwd=ROOT, capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, r.stderr[-3000:]
        outs.append(out)
    logs = [open(os.path.join(o, finetune.LOG_NAME)).read() for o in outs]
    assert logs[0] == logs[1]
    recs = [json.loads(l) for l in logs[0].splitlines()]
    assert recs[0] == {"augment": {"blur_sigmas": [1.0, 2.0], "blur_prob": 0.5, "saturate_prob": 0.25, "max_gain": 2.0}}
    assert [r["step"] for r in recs[1:]] == [0, 10, 20] and all(np.isfinite(r["loss"]) for r in recs[1:])
    arts = [model.load_model_dir(o) for o in outs]
    assert arts[0].hp == hp and arts[0].mean == mean and arts[0].std == std
    assert np.array_equal(arts[0].blob, arts[1].blob)
    z = [np.load(os.path.join(o, model.CONVERTED_NAME)) for o in outs]
    assert sorted(z[0].files) == sorted(z[1].files) and all(z[0][k].tobytes() == z[1][k].tobytes() for k in z[0].files)
    # UnMicst.py --model <out> on a small TIFF cut from 105
    img = str(tmp_path / "cut.tif")
    tiffio.imsave(img, np.ascontiguousarray(helpers.load_sample_105()[0][:200, :300]))
    res = str(tmp_path / "res")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "UnMicst.py"), img, "--model", outs[0], "--stackOutput", "--outputPath", res],
                       cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    names = [f for f in os.listdir(res) if f.startswith("cut_Probabilities_")]
    assert len(names) == 1, os.listdir(res)
    stack = tiffio.imread_all(os.path.join(res, names[0]))
    assert stack.shape[1:] == (200, 300) and stack.max() > 0
