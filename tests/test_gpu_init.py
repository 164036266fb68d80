"""GPU tests of the trainer's initial state (include/umx_train.h: umx_trainer_init) and of
``python -m unmicst_amd.finetune --from-scratch``: the kernel against its numpy restatement (tests/init_ref.py), re-initialisation,
no stale derived copy of the old variables, refused input, the debug guard, and one run from the initial state per regime."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import helpers
import init_ref
import trainset_ref as ref
from unmicst_amd import finetune, model, tiffio, trainer, umx

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_INVALID = 1    # UMX_ERR_INVALID (include/umx.h)

SMALL = {   # name -> (hp, options, batch)
    "solo_small": (helpers.small_hps()["v2_solo_like"], trainer.solo_options, 4),
    "duo_small": (helpers.small_hps()["v2_duo_like"], trainer.duo_options, 4),
    "legacy_small": (helpers.small_hps()["legacy_k3_x2"], trainer.legacy_options, 4),
    "legacy_k5": (helpers.small_hps()["legacy_k5"], trainer.legacy_options, 3),
}
CASES = dict(SMALL, duo_full=(model.KNOWN_HP["nucleiDAPILAMIN"], trainer.duo_options, 1))


def _ordered(a):
    """float32 -> int64 that counts representable values: neighbours differ by 1, -0.0 and +0.0 coincide."""
    i = np.ascontiguousarray(a, np.float32).view(np.int32).astype(np.int64)
    return np.where(i < 0, -(i & 0x7FFFFFFF), i)


def _batch(hp, B, seed):
    rng = np.random.default_rng(seed)
    data = rng.normal(0, 1, (B, hp.imSize, hp.imSize, hp.nChannels)).astype(np.float32)
    labels = np.eye(hp.nClasses, dtype=np.float32)[rng.integers(0, hp.nClasses, (B, hp.imSize, hp.imSize))]
    weights = rng.uniform(0.5, 3.0, labels.shape).astype(np.float32)
    return data, labels, weights


@pytest.mark.parametrize("case", sorted(CASES))
def test_kernel_against_the_restatement(case):
    """BN values bit-equal; every filter value within 1 float32 ulp, and at most 1e-5 of them different at all: device and host
    float64 log / cos / sqrt agree to a few float64 ulp, so a difference survives the rounding to float32 only next to a rounding
    boundary (odds about 2^-28 per value) -- a larger share means the streams differ, not the libm."""
    hp, options, B = CASES[case]
    seed, sd0 = 20261017 + len(case), 0.03
    tr = trainer.Trainer.from_scratch(hp, options(), seed, sd0, batch=B)
    try:
        got = tr.blob()
        assert tr.step_count == 0
    finally:
        tr.close()
    want = init_ref.initial_blob(hp, seed, sd0)
    assert got.shape == want.shape
    g, w = model.tensors_from_blob(hp, got), model.tensors_from_blob(hp, want)
    n_filter = n_diff = 0
    for name, _ in model.tensor_specs(hp):
        if ".bn." in name:
            assert np.array_equal(g[name].view(np.uint32), w[name].view(np.uint32)), name
            continue
        d = np.abs(_ordered(g[name]) - _ordered(w[name]))
        print("%s %s: %d of %d values differ, max %d ulp" % (case, name, int((d != 0).sum()), d.size, int(d.max())))
        assert d.max() <= 1, (name, int(d.max()))
        n_filter += d.size
        n_diff += int((d != 0).sum())
    print("%s: %d of %d filter values differ from the restatement" % (case, n_diff, n_filter))
    assert n_diff <= 1e-5 * n_filter, (n_diff, n_filter)


@pytest.mark.parametrize("case", sorted(SMALL))
def test_reinitialisation_equals_a_fresh_start(case):
    """Three real steps from weights of another scale, then init: the blob of a fresh from_scratch, step 0, zero slots and gradients --
    and the next step is bit-equal to the fresh trainer's first step (no weight scale of the old variables survives)."""
    hp, options, B = SMALL[case]
    seed, sd0 = 77, 0.02
    old = model.random_blob(hp, seed=5)                # N(0, 1 / fan_in) filters, several times the initial state's: other weight scales
    tr = trainer.Trainer(hp, old, options(seed=3), batch=B)
    fresh = trainer.Trainer.from_scratch(hp, options(seed=3), seed, sd0, batch=B)
    try:
        for s in range(3):
            tr.step(*_batch(hp, B, 10 + s))
        assert tr.step_count == 3
        tr.init(seed, sd0)
        assert tr.step_count == 0
        assert np.array_equal(tr.blob().view(np.uint32), fresh.blob().view(np.uint32))
        m, v = tr.slots()
        assert not m.any() and not v.any() and not tr.grads().any()
        batch = _batch(hp, B, 20)
        la, lb = tr.step(*batch), fresh.step(*batch)
        assert la == lb
        assert np.array_equal(tr.grads().view(np.uint32), fresh.grads().view(np.uint32))
        assert np.array_equal(tr.blob().view(np.uint32), fresh.blob().view(np.uint32))
        assert tr.step_count == fresh.step_count == 1
    finally:
        tr.close()
        fresh.close()


@pytest.mark.parametrize("case", sorted(CASES))
def test_no_stale_copies_after_from_scratch(case):
    """One step after from_scratch == one step of a trainer created from the blob read back: parameters, gradients and loss."""
    hp, options, B = CASES[case]
    a = trainer.Trainer.from_scratch(hp, options(seed=8), 123, 0.03, batch=B)
    try:
        blob = a.blob()
        b = trainer.Trainer(hp, blob, options(seed=8), batch=B)
        try:
            batch = _batch(hp, B, 31)
            la, lb = a.step(*batch), b.step(*batch)
            assert la == lb, (la, lb)
            assert np.array_equal(a.grads().view(np.uint32), b.grads().view(np.uint32))
            assert np.array_equal(a.blob().view(np.uint32), b.blob().view(np.uint32))
            assert not np.array_equal(a.blob(), blob)          # (a real step: the variables moved)
        finally:
            b.close()
    finally:
        a.close()


def test_invalid_input_leaves_the_variables():
    hp, options, B = SMALL["duo_small"]
    tr = trainer.Trainer(hp, model.random_blob(hp, seed=2), options(), batch=B)
    try:
        tr.step(*_batch(hp, B, 1))
        before, step = tr.blob(), tr.step_count
        for bad in (0.0, -0.01, float("nan"), float("inf"), -float("inf")):
            with pytest.raises(umx.UmxError) as e:
                tr.init(1, bad)
            assert e.value.code == ERR_INVALID, bad
            assert "std_dev0" in str(e.value)
        for slot in range(5):
            o = trainer._InitOptions()
            o.seed, o.std_dev0 = 1, 0.03
            o.reserved[slot] = 1
            assert tr._lib.umx_trainer_init(tr._h, ctypes.byref(o)) == ERR_INVALID
            assert b"reserved" in tr._lib.umx_trainer_last_error(tr._h)
        assert tr._lib.umx_trainer_init(tr._h, None) == ERR_INVALID
        assert np.array_equal(tr.blob().view(np.uint32), before.view(np.uint32)) and tr.step_count == step
        m, _ = tr.slots()
        assert m.any()                                          # (the optimiser state of the step is still there)
    finally:
        tr.close()


@pytest.mark.parametrize("case", sorted(SMALL))
def test_guard_mode_create_init_step(case, monkeypatch):
    """Under UMX_DEBUG_GUARD every entry checks every red zone: a write of the init kernel outside the parameter vector (or of its
    table) would be UMX_ERR_GUARD here.  The result is the unguarded one."""
    hp, options, B = SMALL[case]
    outs = []
    for fill in (None, "0xff"):
        if fill is None:
            monkeypatch.delenv("UMX_DEBUG_GUARD", raising=False)
        else:
            monkeypatch.setenv("UMX_DEBUG_GUARD", fill)
        tr = trainer.Trainer.from_scratch(hp, options(), 9, 0.03, batch=B)
        try:
            blob0 = tr.blob()
            loss = tr.step(*_batch(hp, B, 3))
            tr.init(10, 0.03)                                  # a second call reuses the table
            outs.append((blob0, loss, tr.blob()))
        finally:
            tr.close()
        monkeypatch.delenv("UMX_DEBUG_GUARD", raising=False)
    for x, y in zip(outs[0], outs[1]):
        assert np.array_equal(np.asarray(x), np.asarray(y))


# ---- one run from the initial state per regime ---------------------------------------------------------------------------------
def make_separable_set(path, n, S, C, K, seed):
    """Discs on a dark background, as tests/test_gpu_trainset.py::test_finetune_learns_a_synthetic_set builds them; K == 3 adds the
    discs' 2-pixel rim as the middle class (codes 1 background, 2 rim, 3 interior), at an intensity of its own.  C planes per sample,
    each with its own noise.  -> the class codes [n][S][S]."""
    rng = np.random.default_rng(seed)
    raws, codes = [], []
    yy, xx = np.mgrid[:S, :S]
    for _ in range(n):
        inner = np.zeros((S, S), bool)
        outer = np.zeros((S, S), bool)
        for _ in range(max(5, 5 * S * S // (48 * 48))):
            cy, cx = rng.integers(0, S, 2).tolist()
            r = int(rng.integers(5, 10))
            d2 = (yy - cy) ** 2 + (xx - cx) ** 2
            outer |= d2 < r * r
            inner |= d2 < (r - 2) * (r - 2)
        if K == 2:
            level, code = np.where(outer, 0.75, 0.25), (1 + outer).astype(np.uint8)
        else:
            rim = outer & ~inner
            level = np.where(inner, 0.8, np.where(rim, 0.5, 0.2))
            code = np.where(inner, 3, np.where(rim, 2, 1)).astype(np.uint8)
        planes = [np.clip((level + rng.normal(0, 0.05, (S, S))) * 255, 0, 255).astype(np.uint8) for _ in range(C)]
        raws.append(np.stack(planes)[:, None])                  # [C][1 page][S][S]
        codes.append(code)
    ref.write_dataset(path, raws, codes)
    return np.stack(codes)


def majority_class_error(codes, K):
    """The mean per-class error (the log's mean_error) of answering the most frequent class everywhere: 0 for that class, 1 for
    every other class that has a pixel."""
    counts = np.array([(codes == k + 1).sum() for k in range(K)])
    present = counts > 0
    err = np.where(np.arange(K) == counts.argmax(), 0.0, 1.0)
    return float(err[present].mean())


def legacy_reference_dir(dst):
    """A small legacy model directory in the reference's layout, without weights: hp.data (with stdDev0), the two normalisation
    pickles, and the checkpoint index of the shipped nucleiDAPI (the graph kind is read from its variable names)."""
    import pickle
    import shutil
    os.makedirs(dst)
    hp = {"imSize": 32, "nClasses": 2, "nChannels": 1, "nExtraConvs": 1, "nLayers": 2, "featMapsFact": 2, "downSampFact": 2, "ks": 3,
          "nOut0": 8, "stdDev0": 0.03, "batchSize": 8}
    for name, v in (("hp.data", hp), ("datasetMean.data", 0.4), ("datasetStDev.data", 0.25)):
        with open(os.path.join(dst, name), "wb") as f:
            pickle.dump(v, f)
    shutil.copy(os.path.join(helpers.REFERENCE_MODELS, "nucleiDAPI", "model.ckpt.index"), dst)
    return dst


# kind -> (model, sample size, tool, tool arguments, flags of the run).  Steps and learning rates were picked on an MI355X
# (DESIGN.md section 9.3 records the losses and errors they give)
RUNS = {
    "solo": ("nucleiDAPI1-5", 96, "UnMicst1-5.py", [],
             ["--batch", "8", "--steps", "300", "--eval-every", "100"]),
    "duo": ("nucleiDAPILAMIN", 160, "UnMicst2.py", ["--channel", "0", "1"],
            ["--batch", "4", "--steps", "300", "--eval-every", "100"]),
    "legacy": (None, 48, "UnMicst.py", [],
               ["--batch", "8", "--steps", "300", "--eval-every", "100"]),
}


def run_from_scratch(kind, tmp, extra=()):
    """Write the sets, run the command twice with equal arguments -> (model directory, K, C, validation codes, out dirs, results)."""
    name, S, _, _, flags = RUNS[kind]
    mdir = os.path.join(ROOT, "models", name) if name else legacy_reference_dir(os.path.join(tmp, "legacy_model"))
    hp = model.load_hparams_dir(mdir)[0]
    make_separable_set(os.path.join(tmp, "train"), 12, S, hp.nChannels, hp.nClasses, 12)
    vcodes = make_separable_set(os.path.join(tmp, "valid"), 4, S, hp.nChannels, hp.nClasses, 13)
    outs, results = [], []
    for k in range(2):
        out = os.path.join(tmp, "out%d" % k)
        r = subprocess.run([sys.executable, "-m", "unmicst_amd.finetune", "--model", mdir, "--train", os.path.join(tmp, "train"),
                            "--valid", os.path.join(tmp, "valid"), "--out", out, "--from-scratch", "--seed", "4", "--init-seed", "21",
                            "--mean", "0.45", "--std", "0.3"] + flags + list(extra),
                           cwd=ROOT, capture_output=True, text=True, timeout=600)
        outs.append(out)
        results.append(r)
    return mdir, hp, vcodes, outs, results


@pytest.mark.parametrize("kind", sorted(RUNS))
def test_from_scratch_end_to_end(kind, tmp_path):
    mdir, hp, vcodes, outs, results = run_from_scratch(kind, str(tmp_path))
    for r in results:
        assert r.returncode == 0, r.stderr[-3000:]
    logs = [open(os.path.join(o, finetune.LOG_NAME)).read() for o in outs]
    assert logs[0] == logs[1]
    arts = [model.load_model_dir(o) for o in outs]
    assert np.array_equal(arts[0].blob.view(np.uint32), arts[1].blob.view(np.uint32))
    assert arts[0].hp == hp and (arts[0].mean, arts[0].std) == (0.45, 0.3)
    recs = [json.loads(l) for l in logs[0].splitlines()]
    sd0 = 0.03 if kind == "legacy" else trainer.DEFAULT_STD_DEV0        # hp.data of the legacy directory; no hp.data in the stand-ins
    assert recs[0] == {"init": {"seed": 21, "std_dev0": sd0, "mean": 0.45, "std": 0.3}}
    evals = recs[1:]
    print(kind, json.dumps(evals))
    losses = [e["train_loss"] for e in evals if e["train_loss"] is not None]
    assert losses[-1] < losses[0], losses
    best = min(e["mean_error"] for e in evals)
    floor = majority_class_error(vcodes, hp.nClasses)
    print("%s: train loss %.6g -> %.6g, best mean error %.4f, majority-class error %.4f" % (kind, losses[0], losses[-1], best, floor))
    assert best < floor, (best, floor)
    # the saved directory runs through the regime's command-line tool
    _, S, tool, tool_args, _ = RUNS[kind]
    rng = np.random.default_rng(5)
    img = str(tmp_path / "cut.tif")
    for c in range(hp.nChannels):
        tiffio.imsave(img, rng.integers(0, 60000, (150, 200)).astype(np.uint16), append=c > 0)
    res = str(tmp_path / "res")
    r = subprocess.run([sys.executable, os.path.join(ROOT, tool), img, "--model", outs[0], "--stackOutput", "--outputPath", res] + tool_args,
                       cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    names = [f for f in os.listdir(res) if f.startswith("cut_Probabilities_")]
    assert len(names) == 1, os.listdir(res)
    stack = tiffio.imread_all(os.path.join(res, names[0]))
    assert stack.shape[1:] == (150, 200) and stack.max() > 0


def test_from_scratch_ignores_the_weights_of_the_model_directory(tmp_path):
    """A directory that has weights supplies its hyper-parameters only: the log says so, and the start is the hyper-parameter-only
    directory's."""
    hp = model.HParams(model.GRAPH_LEGACY, 32, 1, 2, 8, 2, 3, 0, batchSize=8)
    with_w, hp_only = str(tmp_path / "with_w"), str(tmp_path / "hp_only")
    model.save_converted(model.ModelArtefacts(hp, model.random_blob(hp, seed=4), 0.5, 0.25), with_w)
    os.makedirs(hp_only)
    np.savez(os.path.join(hp_only, model.HP_ONLY_NAME), hp=model._hp_vector(hp), mean=np.float64(0.5), std=np.float64(0.25))
    make_separable_set(str(tmp_path / "set"), 4, 48, 1, 2, 3)
    blobs = []
    for mdir, out in ((with_w, str(tmp_path / "o1")), (hp_only, str(tmp_path / "o2"))):
        rc = finetune.main(["--model", mdir, "--train", str(tmp_path / "set"), "--valid", str(tmp_path / "set"), "--out", out,
                            "--from-scratch", "--steps", "4", "--eval-every", "4", "--seed", "2"])
        assert rc == 0
        first = json.loads(open(os.path.join(out, finetune.LOG_NAME)).readline())
        assert first["init"]["seed"] == 2 and first["init"]["std_dev0"] == trainer.DEFAULT_STD_DEV0
        assert first["init"].get("weights_not_read", False) == (mdir == with_w)
        blobs.append(model.load_model_dir(out).blob)
    assert np.array_equal(blobs[0], blobs[1])
