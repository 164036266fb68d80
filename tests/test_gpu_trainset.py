"""GPU tests of the device-resident training set (include/umx_train.h: umx_trainset_*, umx_train_step_sampled, umx_trainer_assemble,
umx_trainer_evaluate) and of the finetune command: the assembled batch is bit-equal to tests/trainset_ref.py, a sampled step is
bit-equal to the host-fed step on the same arrays, the device counts equal numpy's, bad descriptors are refused, and a fine-tuning
run saves a model the inference paths load."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import helpers
import trainset_ref as ref
from trainset_cases import _descs
from unmicst_amd import finetune, model, tiffio, trainer, trainset, umx

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_INVALID, ERR_OOM = 1, 5    # UMX_ERR_INVALID, UMX_ERR_OOM (include/umx.h)

LEG_C1K2 = model.HParams(model.GRAPH_LEGACY, 32, 1, 2, 8, 2, 3, 0)
V2_C2K3 = helpers.small_hps()["v2_duo_like"]
LW3 = trainset.LabelWeights(True, (1.0, 2.0, 7.0), (0.0, 15.0, 0.25))
LW2 = trainset.LabelWeights(True, (0.5, 3.0), (1.5, 0.0))


def _random_set(hp, N, pages, S, seed):
    rng = np.random.default_rng(seed)
    planes = rng.normal(0, 1, (N, hp.nChannels, pages, S, S)).astype(np.float32)
    ann = rng.integers(0, hp.nClasses + 2, (N, S, S)).astype(np.uint8)       # codes 0 and > K included
    wmaps = [rng.random((S, S)).astype(np.float32) * 2 for _ in range(N)]
    wmaps[1] = None                                                          # a missing map counts as 0
    return planes, ann, wmaps


def _ref(planes, ann, wmaps, d, hp, lw):
    if lw.weighted:
        return ref.assemble(planes, ann, wmaps, d, hp.imSize, hp.nClasses, lw.class_weight, lw.intersect_weight)
    return ref.assemble(planes, ann, wmaps, d, hp.imSize, hp.nClasses)


@pytest.mark.parametrize("hp,lw", [(LEG_C1K2, trainset.UNWEIGHTED), (LEG_C1K2, LW2), (V2_C2K3, LW3)],
                         ids=["legacy_C1K2_unweighted", "legacy_C1K2_weighted", "v2_C2K3_weighted"])
def test_assemble_is_bit_equal_to_the_restatement(hp, lw):
    S, P, pages, B = 45, hp.imSize, 2, 8
    planes, ann, wmaps = _random_set(hp, 3, pages, S, 7)
    opts = trainer.legacy_options() if hp.graph == model.GRAPH_LEGACY else trainer.duo_options()
    tr = trainer.Trainer(hp, model.random_blob(hp, seed=3), opts, batch=B)
    ts = trainset.TrainSet.from_arrays(tr, planes, ann, wmaps, lw)
    far = S - P
    rows = [(t % 3, t % 2, (0, far, 5, 0)[t % 4], (far, 0, 0, 7)[t % 4], t, 0.5 - 0.25 * t, 1.0 + 0.03 * t) for t in range(8)]
    rows_b = [(2, 1, far, far, t, -0.125, 0.9) for t in range(8)]
    for d in (_descs(rows), _descs(rows_b), _descs(rows[:3])):      # every transform, crops at 0 and S - P, n < B
        got = tr.assemble(ts, d)
        want = _ref(planes, ann, wmaps, d, hp, lw)
        assert got[0].shape == (len(d), P, P, hp.nChannels)
        assert got[0].tobytes() == want[0].tobytes()
        assert got[1].tobytes() == want[1].tobytes()
        if lw.weighted:
            assert got[2].tobytes() == want[2].tobytes()
        else:
            assert got[2] is None
    tr.close()


def _step_pair(hp, blob, opts, B, planes, ann, wmaps, lw, descs):
    a = trainer.Trainer(hp, blob, opts, batch=B)
    b = trainer.Trainer(hp, blob, opts, batch=B)
    ts = trainset.TrainSet.from_arrays(a, planes, ann, wmaps, lw)
    for d in descs:
        a.step_sampled(ts, d)
        la = a.loss()
        data, labels, weights = _ref(planes, ann, wmaps, d, hp, lw)
        lb = b.step(data, labels, weights)
        assert la == lb
        assert a.grads().tobytes() == b.grads().tobytes()
    assert a.blob().tobytes() == b.blob().tobytes()
    assert a.step_count == b.step_count == len(descs)
    a.close()
    b.close()


def test_step_sampled_is_the_host_fed_step_v2_duo():
    hp = V2_C2K3
    planes, ann, wmaps = _random_set(hp, 4, 2, 40, 11)
    s = trainset.Sampler(2, 4, 4, 40, hp.imSize, 2, 0.25, 0.025, transforms=True)
    _step_pair(hp, model.random_blob(hp, seed=5), trainer.duo_options(), 4, planes, ann, wmaps, LW3, [s.next() for _ in range(3)])


def test_step_sampled_is_the_host_fed_step_nucleidapi():
    hp, blob, mean, std = helpers.load_nuclei_dapi()
    raws, codes, wts = ref.sample_105_crops(ref.TRAIN_ORIGINS, S=256)
    planes = ref.normalise(raws, mean, std)[:, None, None]
    s = trainset.Sampler(3, len(raws), 16, 256, hp.imSize, 1, 0.0, 0.0, transforms=True)
    descs = [s.next() for _ in range(3)]
    _step_pair(hp, blob, trainer.legacy_options(), 16, planes, codes, list(wts), trainset.UNWEIGHTED, descs)
    # the legacy step takes weights as well: a weighted set is step(data, labels, weights)
    _step_pair(hp, blob, trainer.legacy_options(), 16, planes, codes, list(wts), trainset.LABEL_WEIGHTS["solo"], descs[:2])


def test_evaluate_counts_are_numpys():
    hp, blob, mean, std = helpers.load_nuclei_dapi()
    raws, codes, wts = ref.sample_105_crops(ref.VALID_ORIGINS, S=256)
    planes = ref.normalise(raws, mean, std)[:, None, None]
    B = 8
    tr = trainer.Trainer(hp, blob, trainer.legacy_options(), batch=B)
    ts = trainset.TrainSet.from_arrays(tr, planes, codes, None, trainset.UNWEIGHTED)
    vd = trainset.validation_descriptors(len(raws), 256, hp.imSize)      # 12 crops: one full batch, one of 4
    total = np.zeros((2, hp.nClasses), np.int64)
    total_loss = 0.0
    for n0 in range(0, len(vd), B):
        d = vd[n0:n0 + B]
        ev = tr.evaluate(ts, d)
        data, labels, _ = tr.assemble(ts, d)
        pad = np.zeros((B,) + data.shape[1:], np.float32)
        pad[:len(d)] = data
        probs = tr.eval(pad)[:len(d)]                                     # rows len(d)..B-1 are not counted
        want_c, want_l = ref.class_counts(probs, labels)
        assert np.array_equal(ev["counts"], want_c)
        assert abs(ev["loss_sum"] - want_l) <= 1e-9 * abs(want_l)
        total += want_c
        total_loss += want_l
    ev = tr.evaluate(ts, vd)
    assert np.array_equal(ev["counts"], total) and ev["counts"][1].sum() > 0
    assert abs(ev["loss_sum"] - total_loss) <= 1e-9 * abs(total_loss)
    assert np.allclose(ev["per_class_error"], 1 - total[0] / total[1])
    tr.close()


def test_refusals():
    hp = LEG_C1K2
    B, S = 4, 40
    planes, ann, wmaps = _random_set(hp, 3, 2, S, 1)
    tr = trainer.Trainer(hp, model.random_blob(hp), trainer.legacy_options(), batch=B)
    other = trainer.Trainer(hp, model.random_blob(hp), trainer.legacy_options(), batch=B)
    ts = trainset.TrainSet.from_arrays(tr, planes, ann, wmaps, trainset.UNWEIGHTED)
    good = [(0, 0, 0, 0, 0, 0.0, 1.0)] * B
    tr.step_sampled(ts, _descs(good))
    tr.loss()
    assert tr.step_count == 1
    bad = [(3, 0, 0, 0, 0, 0.0, 1.0), (-1, 0, 0, 0, 0, 0.0, 1.0), (0, 2, 0, 0, 0, 0.0, 1.0), (0, 0, S - hp.imSize + 1, 0, 0, 0.0, 1.0),
           (0, 0, 0, -1, 0, 0.0, 1.0), (0, 0, 0, 0, 8, 0.0, 1.0), (0, 0, 0, 0, 0, float("nan"), 1.0), (0, 0, 0, 0, 0, 0.0, float("inf"))]
    for row in bad:
        d = _descs(good[:-1] + [row])
        for call in (lambda: tr.step_sampled(ts, d), lambda: tr.assemble(ts, d), lambda: tr.evaluate(ts, d)):
            with pytest.raises(umx.UmxError) as e:
                call()
            assert e.value.code == ERR_INVALID, row
        assert tr.step_count == 1
    d = _descs(good)
    d["reserved"][2] = 1
    with pytest.raises(umx.UmxError) as e:
        tr.step_sampled(ts, d)
    assert e.value.code == ERR_INVALID and tr.step_count == 1
    with pytest.raises(umx.UmxError) as e:   # a set of another trainer
        other.step_sampled(ts, _descs(good))
    assert e.value.code == ERR_INVALID and other.step_count == 0
    with pytest.raises(umx.UmxError) as e:   # samples smaller than the tile
        trainset.TrainSet(tr, 2, 1, hp.imSize - 1, trainset.UNWEIGHTED)
    assert e.value.code == ERR_INVALID
    with pytest.raises(umx.UmxError) as e:   # more than fits in device memory
        trainset.TrainSet(tr, 1 << 20, 64, 1024, trainset.UNWEIGHTED)
    assert e.value.code == ERR_OOM
    v2 = trainer.Trainer(V2_C2K3, model.random_blob(V2_C2K3), trainer.duo_options(), batch=2)
    with pytest.raises(umx.UmxError) as e:   # the v2 graph has no unweighted loss
        trainset.TrainSet(v2, 2, 1, 40, trainset.UNWEIGHTED)
    assert e.value.code == ERR_INVALID
    tr.step_sampled(ts, _descs(good))
    tr.loss()
    assert tr.step_count == 2
    for t in (tr, other, v2):
        t.close()


def _run_finetune(args, timeout=900):
    return subprocess.run([sys.executable, "-m", "unmicst_amd.finetune"] + args, cwd=ROOT, capture_output=True, text=True,
                          timeout=timeout)


def test_finetune_nucleidapi_end_to_end(tmp_path):
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
        r = _run_finetune(["--model", mdir, "--train", str(tmp_path / "train"), "--valid", str(tmp_path / "valid"), "--out", out,
                           "--steps", "40", "--eval-every", "20", "--seed", "9", "--transforms"])
        assert r.returncode == 0, r.stderr[-3000:]
        outs.append(out)
    logs = [open(os.path.join(o, finetune.LOG_NAME)).read() for o in outs]
    assert logs[0] == logs[1]
    recs = [json.loads(l) for l in logs[0].splitlines()]
    assert [r["step"] for r in recs] == [0, 20, 40]
    arts = [model.load_model_dir(o) for o in outs]
    assert arts[0].hp == hp and arts[0].mean == mean and arts[0].std == std
    assert np.array_equal(arts[0].blob, arts[1].blob)
    # the saved blob runs on the inference engine as on the trainer's eval
    x = ref.normalise(raws[:, :hp.imSize, :hp.imSize], mean, std)[..., None]
    x = np.concatenate([x] * (16 // len(x) + 1))[:16]
    tr = trainer.Trainer(hp, arts[0].blob, trainer.legacy_options(), batch=16)
    want = tr.eval(x)
    tr.close()
    with umx.Engine(hp, arts[0].blob, max_batch=16, precision="f32") as eng:
        got = eng.forward_tiles(x)
    assert np.abs(got - want).max() <= 1e-4
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


def test_finetune_learns_a_synthetic_set(tmp_path):
    """A random legacy model on a set whose classes a small network can tell apart: the validation error falls."""
    hp = model.HParams(model.GRAPH_LEGACY, 32, 1, 2, 8, 2, 3, 0, batchSize=8)
    mdir = str(tmp_path / "m")
    model.save_converted(model.ModelArtefacts(hp, model.random_blob(hp, seed=4), 0.5, 0.25), mdir)
    rng = np.random.default_rng(12)

    def make(path, n):
        raws, codes = [], []
        for _ in range(n):
            yy, xx = np.mgrid[:48, :48]
            m = np.zeros((48, 48), bool)
            for _ in range(5):
                cy, cx, r = rng.integers(0, 48, 2).tolist() + [int(rng.integers(4, 9))]
                m |= (yy - cy) ** 2 + (xx - cx) ** 2 < r * r
            img = np.where(m, 0.75, 0.25) + rng.normal(0, 0.05, (48, 48))
            raws.append(np.clip(img * 255, 0, 255).astype(np.uint8))
            codes.append((1 + m).astype(np.uint8))
        ref.write_dataset(path, raws, codes)

    make(str(tmp_path / "train"), 12)
    make(str(tmp_path / "valid"), 4)
    out = str(tmp_path / "out")
    rc = finetune.main(["--model", mdir, "--train", str(tmp_path / "train"), "--valid", str(tmp_path / "valid"), "--out", out,
                        "--steps", "60", "--eval-every", "30", "--seed", "1", "--lr0", "0.05"])
    assert rc == 0
    recs = [json.loads(l) for l in open(os.path.join(out, finetune.LOG_NAME))]
    assert recs[-1]["mean_error"] < recs[0]["mean_error"], recs
