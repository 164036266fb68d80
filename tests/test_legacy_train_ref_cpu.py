"""Host checks of tests/legacy_train_ref.py (the float64 yardstick of the legacy training step) and of the legacy preset:
its inference-mode forward is the C oracle's (which the 105 goldens pin), its gradients are the loss's (central differences),
its constants are the reference's, and libumx fills umx_train_options_legacy with the same values."""
import numpy as np
import pytest
import torch

import helpers
import legacy_train_ref as ref
from unmicst_amd import build, model, trainer

LEGACY = ["legacy_k5", "legacy_k3_x0", "legacy_k3_x2"]


def _tiles(hp, mean, std, n):
    """n tiles of 'UNet sample data' 105.tif as the legacy driver feeds them: preprocessed, then (x - mean) / std."""
    raw = helpers.load_sample_105()[0]
    I = (helpers.legacy_preprocess(raw) - mean) / std
    P = hp.imSize
    out = [I[y:y + P, x:x + P] for y, x in [(0, 0), (300, 417), (832 - P, 960 - P), (200, 600)][:n]]
    return np.stack(out)[..., None].repeat(hp.nChannels, axis=-1).astype(np.float32)


@pytest.mark.parametrize("name", ["nucleiDAPI", "mousenucleiDAPI", "CytoplasmIncell"])
def test_inference_forward_is_the_c_oracle_on_shipped_models(name):
    from oracle import oracle
    hp, blob, mean, std = helpers.load_nuclei_dapi(name)
    assert hp.graph == model.GRAPH_LEGACY
    x = _tiles(hp, mean, std, 2)
    got = ref.inference_probs(hp, blob, x)
    want = oracle.forward(hp, blob, x)
    # (the C oracle returns float32 probabilities: the bound is that rounding plus the float32 tensors it keeps between ops; a wrong op
    # order -- BN before the ReLU, the pool before BN, a missing shortcut -- moves them by 1e-2 .. 1)
    assert np.abs(got - want).max() <= 1e-6


def _batch(hp, B, seed):
    rng = np.random.default_rng(seed)
    data = rng.normal(0, 1, (B, hp.imSize, hp.imSize, hp.nChannels))
    labels = np.eye(hp.nClasses)[rng.integers(0, hp.nClasses, (B, hp.imSize, hp.imSize))]
    return data, labels


@pytest.mark.parametrize("name", LEGACY)
def test_gradients_are_central_differences(name):
    hp = helpers.small_hps()[name]
    blob = model.random_blob(hp, seed=5).astype(np.float64)
    data, labels = _batch(hp, 2, 9)
    _, g, _, _ = ref.loss_and_grads(hp, blob, data, labels)

    def loss_at(b):
        T = ref.split_blob(hp, b)
        P = {k: torch.tensor(v) for k, v in T.items()}
        with torch.no_grad():
            p, _ = ref.forward(hp, P, torch.tensor(data), True)
        return float((-(torch.tensor(labels) * torch.log(p)).sum(dim=3)).mean())

    rng = np.random.default_rng(1)
    pos = 0
    for nm, shape in model.tensor_specs(hp):
        n = int(np.prod(shape))
        if ref.trainable(nm):
            for j in rng.choice(n, size=min(n, 3), replace=False):
                k = pos + int(j)
                h = 1e-6
                bp, bm = blob.copy(), blob.copy()
                bp[k] += h
                bm[k] -= h
                fd = (loss_at(bp) - loss_at(bm)) / (2 * h)
                assert abs(fd - g[k]) <= 1e-6 * max(1.0, abs(g[k])) + 1e-8, (nm, int(j), fd, g[k])
        else:
            assert not g[pos:pos + n].any(), nm
        pos += n


def test_reference_constants_are_legacy_options():
    o, want = ref.LegacyOptions(), trainer.legacy_options()
    for k in ("lr0", "decay_steps", "decay_rate", "momentum", "bn_momentum"):
        assert getattr(want, k) == getattr(o, k), k
    assert want.optimizer == trainer.OPT_MOMENTUM and want.reg_kind == trainer.REG_NONE and want.clip_eps == 0.0
    for k in ("reg_down", "reg_bottom", "reg_up", "reg_top", "drop_down_step", "drop_bottom", "drop_up0", "drop_up_step"):
        assert getattr(want, k) == 0.0, k


def test_native_legacy_options_match_the_dataclass():
    build.build()
    assert "umx_train_options_legacy" in trainer.EXPORTS
    nat, py = trainer.native_options("legacy"), trainer.legacy_options()
    for k, v in vars(py).items():
        assert getattr(nat, k) == pytest.approx(v, rel=1e-6), k


def test_legacy_trainer_refusals_are_raised_before_the_library():
    hp = helpers.small_hps()["legacy_k5"]
    blob = model.random_blob(hp)
    for bad in (trainer.legacy_options(drop_bottom=0.3), trainer.legacy_options(reg_kind=trainer.REG_L2, reg_down=1e-3), None):
        with pytest.raises(ValueError, match="legacy_options"):
            trainer.Trainer(hp, blob, bad)
