"""Host checks of the trainer's initial state (include/umx_train.h umx_trainer_init) on its numpy restatement
tests/init_ref.py -- the bound, the BN constants, the statistics and the sigma of every tensor, the independence of a value from
where its tensor sits in the blob, the separation of the streams -- and of the finetune command's from-scratch flags: every refusal
comes before any device work."""
import ctypes
import math
import os

import numpy as np
import pytest

import init_ref
import trainset_ref
from unmicst_amd import finetune, model, trainer

KINDS = {"solo": "nucleiDAPI1-5", "duo": "nucleiDAPILAMIN", "legacy": "nucleiDAPI"}
STD_DEV0 = 0.03      # hp.data of four of the five shipped models
SEED = 20261017


@pytest.fixture(scope="module", params=sorted(KINDS))
def state(request):
    hp = model.KNOWN_HP[KINDS[request.param]]
    return hp, init_ref.initial_tensors(hp, SEED, STD_DEV0)


def _sigma(hp, name, shape):
    """The sigma table of the header, recomputed here from the shape alone."""
    sd0 = float(np.float32(STD_DEV0))
    if hp.graph == model.GRAPH_LEGACY:
        return sd0
    if name.startswith("ld") and name.endswith(".w1"):
        return sd0                                   # kernelD<i>: tf.truncated_normal(stddev=stdDev0)
    kh, kw, d2, _ = shape                            # VarianceScaling(scale=1, mode='fan_in'): every dimension but the last
    return math.sqrt(1.0 / (kh * kw * d2)) / 0.87962566103423978


def _filters(hp, tensors):
    return [(n, s, tensors[n]) for n, s in model.tensor_specs(hp) if ".bn." not in n]


def test_every_filter_value_is_within_two_sigma(state):
    hp, tensors = state
    for name, shape, v in _filters(hp, tensors):
        assert v.dtype == np.float32 and v.shape == tuple(shape)
        bound = np.float32(2.0 * _sigma(hp, name, shape))
        assert np.abs(v).max() <= bound, name
        assert np.isfinite(v).all(), name


def test_every_bn_tensor_holds_its_constant(state):
    hp, tensors = state
    seen = 0
    for name, shape in model.tensor_specs(hp):
        if ".bn." not in name:
            continue
        want = 1.0 if name.endswith((".bn.gamma", ".bn.var")) else 0.0
        assert np.array_equal(tensors[name], np.full(shape, want, np.float32)), name
        seen += 1
    assert seen == 4 * (hp.nLayers if hp.graph == model.GRAPH_LEGACY else 2 * hp.nLayers + 2)


def test_tensor_statistics(state):
    """For z a standard normal truncated at +-a (a = 2), with phi the normal density and Z = 2 Phi(a) - 1 its mass on [-a, a]:
        v  = E z^2 = 1 - 2 a phi(a) / Z                 (integrate z * z phi by parts)            = 0.77374, sqrt(v) = 0.87962566
        m4 = E z^4 = 3 v - 2 a^3 phi(a) / Z             (integrate z^3 * z phi by parts)
    A tensor of n independent values sigma * z has sample mean with standard error sigma sqrt(v / n).  Its sample variance s^2 has
    variance (m4 - v^2) sigma^4 / n up to O(1/n^2), so by the delta method s = sqrt(s^2) has standard error
        sigma sqrt(m4 - v^2) / (2 sqrt(v) sqrt(n)).
    (The float32 rounding of a value moves it by 2^-24 relative: nothing next to 1 / sqrt(n) for n <= 1e8.)"""
    hp, tensors = state
    a = 2.0
    phi = math.exp(-a * a / 2) / math.sqrt(2 * math.pi)
    Z = math.erf(a / math.sqrt(2))
    v = 1 - 2 * a * phi / Z
    m4 = 3 * v - 2 * a ** 3 * phi / Z
    assert abs(math.sqrt(v) - 0.87962566) < 1e-8
    checked = 0
    for name, shape, t in _filters(hp, tensors):
        n = t.size
        if n < 10000:
            continue
        sigma = _sigma(hp, name, shape)
        x = t.astype(np.float64).ravel()
        se_mean = sigma * math.sqrt(v / n)
        se_std = sigma * math.sqrt(m4 - v * v) / (2 * math.sqrt(v) * math.sqrt(n))
        assert abs(x.mean()) <= 5 * se_mean, (name, x.mean(), se_mean)
        assert abs(x.std() - 0.87962566 * sigma) <= 5 * se_std, (name, x.std(), 0.87962566 * sigma, se_std)
        checked += 1
    assert checked >= 4


def test_sigma_per_tensor(state):
    """init_ref's table against the shapes: stdDev0 on every legacy filter and on ld<i>.w1 of v2; everywhere else in v2 the
    shape-based fan_in -- for lu<i>.wt [ks, ks, Cout, Cin] that is ks^2 Cout, half the convolution's true fan-in ks^2 Cin."""
    hp, tensors = state
    n = hp.nOutX
    for name, shape, t in _filters(hp, tensors):
        want = _sigma(hp, name, shape)
        assert init_ref.sigma_of(hp, name, shape, STD_DEV0) == pytest.approx(want, rel=1e-15), name
        if hp.graph == model.GRAPH_V2 and name.endswith(".wt"):
            idx = int(name[2:name.index(".")])
            assert shape == (hp.ks, hp.ks, n[idx + 1], n[idx + 2])
            assert want == pytest.approx(math.sqrt(1.0 / (hp.ks * hp.ks * n[idx + 1])) / 0.87962566103423978, rel=1e-15)
            true_fan_in = hp.ks * hp.ks * n[idx + 2]           # what model.random_blob uses: sqrt(2) smaller
            assert want == pytest.approx(math.sqrt(2.0) * math.sqrt(1.0 / true_fan_in) / 0.87962566103423978, rel=1e-12)
        if t.size >= 10000:     # and the values follow it: the largest of n draws comes close to the 2 sigma bound
            assert np.abs(t).max() >= 1.9 * want, name
    if hp.graph == model.GRAPH_V2:
        sd0 = float(np.float32(STD_DEV0))
        for i in range(hp.nLayers):
            assert init_ref.sigma_of(hp, "ld%d.w1" % i, (3, 3, n[i], n[i + 1]), STD_DEV0) == sd0
            assert init_ref.sigma_of(hp, "ld%d.wshort" % i, (3, 3, n[i], n[i + 1]), STD_DEV0) != sd0


def test_values_do_not_depend_on_the_tensors_offset():
    # the issue's example: ld0.w1 (tensor 0) under two depths
    a = model.HParams(model.GRAPH_V2, 32, 1, 3, 12, 2, 3, 0)
    b = model.HParams(model.GRAPH_V2, 32, 1, 3, 12, 3, 3, 0)
    ta, tb = init_ref.initial_tensors(a, 7, 0.01), init_ref.initial_tensors(b, 7, 0.01)
    assert np.array_equal(ta["ld0.w1"], tb["ld0.w1"])
    # ld1.w1 is tensor 6 of both graphs and has one shape, but sits behind a ld0 of another size: another offset in the blob
    c = model.HParams(model.GRAPH_V2, 32, 2, 3, 12, 2, 3, 0)
    ba, bc = init_ref.initial_blob(a, 7, 0.01), init_ref.initial_blob(c, 7, 0.01)
    specs_a, specs_c = model.tensor_specs(a), model.tensor_specs(c)
    assert specs_a[6] == specs_c[6] == ("ld1.w1", (3, 3, 12, 24))
    off_a = sum(int(np.prod(s)) for _, s in specs_a[:6])
    off_c = sum(int(np.prod(s)) for _, s in specs_c[:6])
    cnt = 3 * 3 * 12 * 24
    assert off_a != off_c
    assert np.array_equal(ba[off_a:off_a + cnt], bc[off_c:off_c + cnt])
    assert np.array_equal(ba[off_a:off_a + cnt], init_ref.initial_tensor(7, 6, (cnt,), float(np.float32(0.01))))
    # a prefix of a tensor is the prefix of a longer one with the same (seed, tensor index)
    assert np.array_equal(init_ref.truncated_normal(7, 3, 1000), init_ref.truncated_normal(7, 3, 5000)[:1000])


def test_streams_are_separate():
    hp = model.HParams(model.GRAPH_LEGACY, 16, 2, 3, 4, 1, 3, 2)
    t1, t2 = init_ref.initial_tensors(hp, 1, 0.03), init_ref.initial_tensors(hp, 2, 0.03)
    for name, shape in model.tensor_specs(hp):
        if ".bn." not in name:
            assert not np.array_equal(t1[name], t2[name]), name            # two seeds
            assert (t1[name] == t2[name]).mean() < 0.01, name
    x0, x1 = t1["ld0.wextra0"], t1["ld0.wextra1"]                          # one shape, one sigma, one seed, two tensors
    assert x0.shape == x1.shape and (x0 == x1).mean() < 0.01
    assert abs(np.corrcoef(x0.ravel(), x1.ravel())[0, 1]) < 5 / math.sqrt(x0.size)
    # the stream is not the dropout stream's key schedule: the domain constant separates equal seeds
    assert init_ref.tensor_key(5, 0) != init_ref.mix64(np.uint64(5) + init_ref.GOLDEN)


def test_c_layout_of_init_options():
    assert ctypes.sizeof(trainer._InitOptions) == 8 + 4 + 5 * 4
    assert trainer._InitOptions.std_dev0.offset == 8 and trainer._InitOptions.reserved.offset == 12
    assert trainer.DEFAULT_STD_DEV0 == 0.007


def test_init_entry_checks_its_arguments_without_a_device():
    from unmicst_amd import build, umx
    build.build()
    L = trainer._bind(umx.load())
    assert L.umx_trainer_init(None, None) == 1                       # UMX_ERR_INVALID
    o = trainer._InitOptions()
    o.seed, o.std_dev0 = 1, 0.03
    assert L.umx_trainer_init(None, ctypes.byref(o)) == 1
    assert b"null" in L.umx_trainer_last_error(None)


# ---- the command ---------------------------------------------------------------------------------------------------------------
@pytest.fixture()
def dirs(tmp_path):
    hp = model.HParams(model.GRAPH_V2, 32, 1, 3, 8, 2, 3, 0, batchSize=4)
    hp_only = tmp_path / "hp_only"
    hp_only.mkdir()
    np.savez(str(hp_only / model.HP_ONLY_NAME), hp=model._hp_vector(hp), mean=np.float64(0.34), std=np.float64(0.25))
    rng = np.random.default_rng(0)
    raws = [rng.integers(0, 255, (40, 40)).astype(np.uint8) for _ in range(2)]      # (raws[0]: the generator's first draw)
    codes = [rng.integers(1, 4, (40, 40)).astype(np.uint8) for _ in range(2)]
    data = str(tmp_path / "data")
    trainset_ref.write_dataset(data, raws, codes)
    return hp, str(hp_only), data, str(tmp_path / "out")


def _argv(dirs, *extra):
    _, hp_only, data, out = dirs
    return ["--model", hp_only, "--train", data, "--valid", data, "--out", out] + list(extra)


@pytest.mark.parametrize("extra,flag", [
    (["--init-seed", "3"], "--init-seed"),
    (["--std-dev0", "0.01"], "--std-dev0"),
    (["--mean", "0.3", "--std", "0.2"], "--mean"),
    (["--std", "0.2"], "--std"),
    (["--from-scratch", "--std-dev0", "0"], "--std-dev0"),
    (["--from-scratch", "--std-dev0", "-0.01"], "--std-dev0"),
    (["--from-scratch", "--std-dev0", "inf"], "--std-dev0"),
    (["--from-scratch", "--std-dev0", "nan"], "--std-dev0"),
    (["--from-scratch", "--mean", "0.3", "--std", "0"], "--std"),
    (["--from-scratch", "--mean", "0.3", "--std", "-1"], "--std"),
    (["--from-scratch", "--mean", "0.3", "--std", "inf"], "--std"),
    (["--from-scratch", "--mean", "0.3", "--std", "nan"], "--std"),
    (["--from-scratch", "--mean", "0.3"], "--mean"),
    (["--from-scratch", "--std", "0.2"], "--std"),
], ids=lambda v: " ".join(v) if isinstance(v, list) else None)
def test_finetune_refuses_bad_from_scratch_flags(dirs, capsys, extra, flag):
    rc = finetune.main(_argv(dirs, *extra))
    err = capsys.readouterr().err
    assert rc == 2, err
    assert flag in err, err
    assert "no HIP device" not in err              # (before any device work: not the missing-device error)
    assert not os.path.exists(dirs[3])


def test_from_scratch_accepts_a_hyper_parameter_only_directory(dirs, capsys):
    hp, hp_only, data, out = dirs
    ns = finetune.build_parser().parse_args(_argv(dirs, "--from-scratch", "--seed", "11"))
    art, tr_ds, va_ds = finetune.prepare(ns)
    assert art.hp == hp and art.blob is None and (art.mean, art.std) == (0.34, 0.25)
    assert tr_ds.planes.shape == (2, 1, 1, 40, 40)
    assert finetune.init_settings(ns, hp_only) == {"seed": 11, "std_dev0": 0.007, "mean": 0.34, "std": 0.25}
    ns = finetune.build_parser().parse_args(_argv(dirs, "--from-scratch", "--init-seed", "5", "--std-dev0", "0.02", "--mean", "0.1",
                                                  "--std", "0.2"))
    art, tr_ds, _ = finetune.prepare(ns)
    assert (art.mean, art.std) == (0.1, 0.2)
    raw1 = np.random.default_rng(0).integers(0, 255, (40, 40)).astype(np.uint8)      # the fixture's first image
    assert np.array_equal(tr_ds.planes[0, 0, 0], trainset_ref.normalise(raw1, 0.1, 0.2))   # normalised with the chosen scalars
    assert finetune.init_settings(ns, hp_only) == {"seed": 5, "std_dev0": 0.02, "mean": 0.1, "std": 0.2}
    # the same directory without the flag is still refused, with the text the fine-tuning tests pin
    rc = finetune.main(_argv(dirs))
    assert rc == 2 and "no weights to fine-tune" in capsys.readouterr().err


def test_load_hparams_dir_reads_every_kind_of_directory(tmp_path):
    import helpers
    # the reference's layout: hp.data names stdDev0; no weight shard is needed
    for name in ("nucleiDAPI", "nucleiDAPI1-5", "nucleiDAPILAMIN"):
        hp, mean, std, sd0 = model.load_hparams_dir(os.path.join(helpers.REFERENCE_MODELS, name))
        assert hp == model.KNOWN_HP[name]
        assert sd0 == (1e-6 if name == "nucleiDAPILAMIN" else 0.03)
    assert (mean, std) == (0.18, 0.17)
    # the shipped stand-ins: hyper-parameters and scalars, no stdDev0
    hp, mean, std, sd0 = model.load_hparams_dir(os.path.join(helpers.ROOT, "models", "nucleiDAPI1-5"))
    assert hp == model.KNOWN_HP["nucleiDAPI1-5"] and (mean, std, sd0) == (0.34, 0.25, None)
    # a converted directory: its weights are not needed (a blob of the wrong length would fail load_model_dir)
    conv = tmp_path / "conv"
    model.save_converted(model.ModelArtefacts(hp, np.zeros(3, np.float32), 0.5, 0.125), str(conv))
    assert model.load_hparams_dir(str(conv)) == (hp, 0.5, 0.125, None)
    with pytest.raises(FileNotFoundError):
        model.load_hparams_dir(str(tmp_path))
