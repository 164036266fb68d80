"""The on-decisions check of tests/train_parity.py, proven without a GPU: a float32 run of oracle/train_oracle.py stands in for the HIP
step (train_parity.StandIn), float64 on the stand-in's own decisions is the reference -- the code path tests/test_gpu_train_tight.py
runs, with the kernels swapped out.  For every case, seed and step of that file:

  * the stand-in's worst gradient tensor is within TIGHT / 2 (measured 1.0e-6 .. 4.1e-6: a correct fp32 implementation sits 4.8 x
    inside TIGHT) and the flip cap holds (three cases have 1 .. 3 decisions within rounding distance of zero, the rest none);
  * the decisions rebuilt from the stand-in's z / stat / us tensors equal the branches the float32 run took, element for element;
  * planted flaws of the size a kernel bug has pass the bounds the suite used before (LOOSE, or 0.1 on the odd shapes) and fail the
    new check, which names the tensor; a wrong BRANCH, which an on-decisions comparison follows, fails the flip cap.

The planted weight-gradient flaws are rebuilt from the traced activations (dW = sum over pixels of input patch x dz).  A whole 8-channel
chunk of one filter zeroed moves a tensor by 0.3 .. 0.6 of its scale, which the old bounds reject too; what they let through is a PART
of a reduction: one image row of it (1 / sqrt(rows) of a noise-like sum), one tap off by a percent."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import train_parity as tp
from oracle import train_oracle as to
from unmicst_amd import model

CASES = tp.tight_cases()


@functools.lru_cache(maxsize=None)
def _run(cid, step=0):
    """One case on the stand-in and the float64 reference on the stand-in's decisions (computed once, shared, never modified)."""
    hp, B, regime, blob_seed, batch_seed = CASES[cid]
    oo = tp._oracle_opts(tp.trainer_options(regime))
    blob = model.random_blob(hp, seed=blob_seed)
    if step:   # the parameters one applied update leaves (the GPU test reads them back from the trainer)
        st = to.TrainState(blob)
        for s in range(step):
            to.train_step(hp, st, *tp._batch(hp, B, batch_seed + s), oo)
        blob = st.blob.astype(np.float32)
    batch = tp._batch(hp, B, batch_seed + step)
    si = tp.StandIn(hp, blob, *batch, oo, step=step)
    dec = tp._hip_decisions(si.read_tensor, hp, oo, step, B)
    trace = {}
    want = to.loss_and_grads(hp, blob, *batch, oo, step=step, decisions=dec, trace=trace)
    return dict(hp=hp, B=B, oo=oo, blob=blob, batch=batch, si=si, dec=dec, trace=trace, want=want)


STEPS = [(cid, 0) for cid in CASES] + [(cid, 1) for cid in tp.STEP1_CASES]


@pytest.mark.parametrize("cid,step", STEPS, ids=["%s-step%d" % cs for cs in STEPS])
def test_stand_in_is_within_half_the_bound_and_the_flip_cap(cid, step):
    r = _run(cid, step)
    res = tp.check_on_decisions(r["hp"], r["si"].got, r["want"], r["dec"], r["trace"], cid)      # (asserts the flip cap)
    print("%s step %d: worst %.2e (%s), flips %s of %d" % (cid, step, res["worst"], res["tensor"], res["flips"] or "none", res["sites"]))
    assert res["worst"] <= tp.TIGHT / 2, res


@pytest.mark.parametrize("cid,step", STEPS, ids=["%s-step%d" % cs for cs in STEPS])
def test_reconstruction_equals_the_branches_the_stand_in_took(cid, step):
    r = _run(cid, step)
    took = r["si"].branches()
    assert set(took) == set(r["dec"])
    for site, d in r["dec"].items():
        if site.startswith("pool"):
            assert torch.equal(d, took[site]), site
        else:
            assert torch.equal(d > 0.5, took[site]), site
            assert set(np.unique(d.numpy())) <= {to.LEAK, 1.0}, site


def test_a_reconstruction_off_by_a_layer_id_a_step_or_a_window_order_is_noticed():
    """What the exactness test is for: the dropout stream of another layer or step, or windows read x-major, give other pool choices
    (duo regime: down layer 1 drops 5 %)."""
    r = _run("v2_duo_like-duo")
    took = r["si"].branches()
    other_step = tp._hip_decisions(r["si"].read_tensor, r["hp"], r["oo"], 1, r["B"])
    assert not torch.equal(other_step["pool1"], took["pool1"])
    assert torch.equal(other_step["pool0"], took["pool0"])          # (layer 0 has no dropout)
    saved = to.LAYER_DOWN
    try:
        to.LAYER_DOWN = saved + 1
        other_id = tp._hip_decisions(r["si"].read_tensor, r["hp"], r["oo"], 0, r["B"])
    finally:
        to.LAYER_DOWN = saved
    assert not torch.equal(other_id["pool1"], took["pool1"])
    d = r["dec"]["pool0"]
    x_major = (d % 2) * 2 + d // 2
    assert not torch.equal(x_major, took["pool0"])


# ---- planted flaws ------------------------------------------------------------------------------------------------------------------

def _conv_input(r, layer):
    """Input of the ld<i> / lb convolution in the stand-in's run, NCHW float32."""
    i = r["hp"].nLayers if layer == "lb" else int(layer[2:])
    if i == 0:
        return torch.from_numpy(r["batch"][0]).permute(0, 3, 1, 2)
    return F.max_pool2d(r["si"].trace["pool%d" % (i - 1)], 2)


def _wgrad_part(r, layer, mask):
    """The share of a filter gradient [ky, kx, ci, co] that the output pixels selected by `mask` (shaped like dz, NCHW) contribute."""
    x, ks = _conv_input(r, layer), r["hp"].ks
    dz = r["si"].trace[layer + ".dz"] * mask
    w = torch.nn.grad.conv2d_weight(x, (dz.shape[1], x.shape[1], ks, ks), dz, padding=ks // 2)
    return w.permute(2, 3, 1, 0).numpy().astype(np.float64)


def _flaw_tap(r, G):
    """One filter tap of a down layer scaled by 0.99 (a wrong scale in one slab's epilogue): at most 1e-2 of the tensor's scale."""
    G["ld1.w1"][0, 0] *= 0.99
    return "ld1.w1"


def _flaw_chunk(r, G):
    """A deep filter (lb.w): for one output channel, the first 8-channel chunk of input channels misses the last row of the last image
    in its reduction over pixels (one k-step of one accumulator never issued)."""
    dz = r["si"].trace["lb.dz"]
    mask = torch.zeros_like(dz)
    mask[-1, 0, -1, :] = 1
    G["lb.w"][:, :, :8, 0] -= _wgrad_part(r, "lb", mask)[:, :, :8, 0]
    return "lb.w"


def _flaw_border(r, G, layer):
    """One filter's gradient without what the first row of every image contributes (a border row clipped with the halo)."""
    dz = r["si"].trace[layer + ".dz"]
    mask = torch.zeros_like(dz)
    mask[:, 0, 0, :] = 1
    G[layer + ".w1"][..., 0] -= _wgrad_part(r, layer, mask)[..., 0]
    return layer + ".w1"


# (flaw, case, the bound the suite held this case to before).  The border row is planted where it is smallest against the tensor, on the
# largest layers (one row of 64: the 64-pixel ld0 of v2_wide and the 64-pixel ld1 of the 128-pixel shape).
FLAWS = [
    ("tap", _flaw_tap, "v2_wide-duo", tp.LOOSE), ("tap", _flaw_tap, "odd_l5_2x2", 0.1),
    ("chunk", _flaw_chunk, "v2_wide-duo", tp.LOOSE), ("chunk", _flaw_chunk, "odd_128", 0.1),
    ("border", lambda r, G: _flaw_border(r, G, "ld0"), "v2_wide-duo", tp.LOOSE),
    ("border", lambda r, G: _flaw_border(r, G, "ld1"), "odd_128", 0.1),
]


def test_the_recomputed_weight_gradient_is_the_stand_ins():
    """_wgrad_part over every pixel is the stand-in's own gradient (ld*.w1 carries no regulariser), so a flaw is exactly a missing part."""
    r = _run("v2_wide-duo")
    G = to.split_blob(r["hp"], r["si"].got["grads"])
    for layer in ("ld0", "ld1", "ld2"):
        full = _wgrad_part(r, layer, torch.ones_like(r["si"].trace[layer + ".dz"]))
        assert np.abs(full - G[layer + ".w1"]).max() <= 1e-6 * np.abs(full).max(), layer


@pytest.mark.parametrize("flaw,plant,cid,old", FLAWS, ids=["%s-%s" % (f[0], f[2]) for f in FLAWS])
def test_a_planted_flaw_passes_the_old_bound_and_fails_the_new_check(flaw, plant, cid, old):
    r = _run(cid)
    hp = r["hp"]
    G = {k: np.array(v, dtype=np.float64) for k, v in to.split_blob(hp, r["si"].got["grads"]).items()}
    name = plant(r, G)
    flawed = to.join_blob(hp, G)
    W = to.split_blob(hp, r["want"][3])
    moved = np.abs(G[name] - to.split_blob(hp, r["si"].got["grads"])[name]).max() / np.abs(W[name]).max()
    print("%s on %s: %s moved by %.2e of its scale" % (flaw, cid, name, moved))
    assert name not in tp.TOP and moved > 0
    # the bound in force before, against the free float64 run as the existing tests make it (every tensor at 0.1 on the odd shapes)
    free = to.loss_and_grads(hp, r["blob"], *r["batch"], r["oo"], step=0)[3]
    tp._per_tensor(hp, flawed, free, "old bound", rel=old, top=old if old == 0.1 else tp.TIGHT)
    got = dict(r["si"].got, grads=flawed)
    with pytest.raises(AssertionError) as e:
        tp.check_on_decisions(hp, got, r["want"], r["dec"], r["trace"], cid)
    assert "'%s'" % name in str(e.value), str(e.value)


def test_a_wrong_branch_is_rejected_by_the_flip_cap_alone(monkeypatch):
    """LeakyReLU slopes of one site inverted on 1 % of its elements: the step and the reference then follow the same wrong branches, so
    loss, probabilities and every gradient agree -- only the count against the float64 run's own branches sees it."""
    r = _run("v2_duo_like-duo")
    hp, oo, site = r["hp"], r["oo"], "lu1"
    dec = dict(r["dec"])
    d = dec[site].clone()
    pick = torch.from_numpy(np.random.default_rng(0).random(tuple(d.shape)) < 0.01)
    d[pick] = torch.where(d[pick] > 0.5, to.LEAK, 1.0).to(d.dtype)
    dec[site] = d
    out = to.loss_and_grads(hp, r["blob"], *r["batch"], oo, step=0, dtype=torch.float32, decisions=dec, fused_bn=True)
    got = {"loss": out[0], "reg": out[2], "probs": out[4], "grads": np.asarray(out[3], np.float64)}
    trace = {}
    want = to.loss_and_grads(hp, r["blob"], *r["batch"], oo, step=0, decisions=dec, trace=trace)
    with pytest.raises(AssertionError) as e:
        tp.check_on_decisions(hp, got, want, dec, trace, "wrong branch")
    assert "decisions of %s" % site in str(e.value), str(e.value)
    monkeypatch.setattr(tp, "FLIP_RATE", 1.0)          # without the cap the check passes: everything else agrees
    res = tp.check_on_decisions(hp, got, want, dec, trace, "wrong branch, no cap")
    assert res["worst"] <= tp.TIGHT / 2 and res["flips"][site] >= 0.005 * d.numel()
