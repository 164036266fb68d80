"""GPU parity tests of the training step (BASELINE.json configs[4]): the HIP path through the C ABI of
include/umx_train.h against oracle/train_oracle.py (float64 autograd restatement of the reference's graph, loss and
optimisers).

Tolerances, fp32 arithmetic against a float64 oracle: loss 1e-5 relative; training-mode probabilities 2e-5 max-abs;
gradients per tensor as max-abs error over that tensor's max-abs value:
  TIGHT 2e-5  where no LeakyReLU / max-pool decision differs between fp32 and fp64 (measured 1e-7 .. 4e-6, the same
              as the oracle itself evaluated in float32 by torch -- profiles/r01/train_parity_report.log);
  LOOSE 5e-2  otherwise: the loss is continuous but its gradient is not -- an activation within rounding distance of 0
              (or two pool candidates within rounding distance of each other) takes the other branch in fp32, and every
              gradient below that point moves by 1e-4 .. 1e-2 of its scale (the oracle in float32 does the same, at
              other elements; a float64 run with 1e-7 input noise does too).  A wrong kernel moves a tensor by O(1).
The top of the graph (lt.*, lu0.bn.*, lu0.w2) must always be TIGHT; the small graphs must be TIGHT everywhere for at
least one of three batches.  BN moving statistics 1e-5; optimiser slots like the gradients; the update itself is
checked exactly against the kernel's own gradient (Adam divides by sqrt(v): where |g| is at rounding level the
*direction* of a step is not determined by the maths, so parameters after Adam steps are compared with nsteps * lr)."""
import os

import numpy as np
import pytest

import helpers
import train_parity
from train_parity import LOOSE, TIGHT, _batch, _count_flips, _hip_decisions, _oracle_opts, _per_tensor
from unmicst_amd import model, trainer, umx

pytestmark = pytest.mark.gpu


CASES = [("v2_solo_like", 4, "solo"), ("v2_duo_like", 4, "duo"), ("v2_deep", 3, "duo"), ("v2_wide", 2, "solo"),
         ("v2_wide", 2, "duo"), ("v2_k5", 3, "duo")]


def _hp(name):
    extra = {
        # 5x5 filters: 25 weight-gradient slabs in groups of 9/9/7, transposed conv with pad_before 1 (space-to-depth taps
        # -1..1, parity groups 9/6/6/4)
        "v2_k5": model.HParams(model.GRAPH_V2, 32, 2, 3, 8, 2, 5, 0),
    }
    return extra[name] if name in extra else helpers.small_hps()[name]


# the forward / input-gradient convolutions run on conv_f16x3 (split precision, round 4); the switches the trainer keeps select
# ARITHMETIC, not schedules: UMX_TRAIN_CONV_F32=1 the exact-fp32 MFMA kernel for them, UMX_TRAIN_WGRAD_F32=1 the fp32 weight-gradient
# kernel, UMX_TRAIN_NO_KSPLIT=1 every convolution as one pass over K (no partial sums: another summation order).  Round 5 retired the
# fourteen A/B switches of round 4 whose answer is settled (stream counts, slice targets, staging forms: VERDICT r4 item 8).
ROUTES = [{}, {"UMX_TRAIN_CONV_F32": "1"}, {"UMX_TRAIN_NO_KSPLIT": "1"}, {"UMX_TRAIN_WGRAD_F32": "1"},
          {"UMX_TRAIN_CONV_F32": "1", "UMX_TRAIN_WGRAD_F32": "1"}]


@pytest.mark.parametrize("route", ROUTES, ids=lambda r: ",".join("%s=%s" % kv for kv in r.items()) or "f16x3")
@pytest.mark.parametrize("name,B,regime", CASES)
def test_loss_gradients_and_probabilities_match_oracle(name, B, regime, route, monkeypatch):
    from oracle import train_oracle as to
    for k, v in route.items():
        monkeypatch.setenv(k, v)
    hp = _hp(name)
    opts = trainer.solo_options() if regime == "solo" else trainer.duo_options()
    blob = model.random_blob(hp, seed=21)
    data, labels, weights = _batch(hp, B, 3)
    want_loss, want_data, want_reg, want_g, want_p, _ = to.loss_and_grads(hp, blob, data, labels, weights,
                                                                         _oracle_opts(opts), step=0)
    tr = trainer.Trainer(hp, blob, opts, batch=B)
    loss, data_term, reg = tr.step(data, labels, weights, apply_update=False)
    assert tr.step_count == 0
    assert loss == pytest.approx(want_loss, rel=1e-5)
    assert data_term == pytest.approx(want_data, rel=1e-5)
    assert reg == pytest.approx(want_reg, rel=1e-5)
    assert np.abs(tr.probs() - want_p).max() <= 2e-5
    worst = _per_tensor(hp, tr.grads(), want_g, "grads")
    assert np.array_equal(tr.blob(), blob)           # nothing moved, moving statistics included
    if hp.imSize * hp.nOut0 <= 32 * 20:              # small graphs: few decisions, a flip-free batch exists
        for seed in (4, 5):
            if worst <= TIGHT:
                break
            data, labels, weights = _batch(hp, B, seed)
            want_g = to.loss_and_grads(hp, blob, data, labels, weights, _oracle_opts(opts), step=0)[3]
            tr.step(data, labels, weights, apply_update=False)
            worst = _per_tensor(hp, tr.grads(), want_g, "grads seed %d" % seed)
        assert worst <= TIGHT, worst
    tr.close()


@pytest.mark.parametrize("name,B,regime", [("v2_duo_like", 4, "duo"), ("v2_solo_like", 4, "solo")])
def test_adam_steps_track_the_oracle(name, B, regime):
    from oracle import train_oracle as to
    hp = helpers.small_hps()[name]
    opts = trainer.solo_options(decay_steps=2) if regime == "solo" else trainer.duo_options(decay_steps=2)
    oo = _oracle_opts(opts)
    blob = model.random_blob(hp, seed=8)
    st = to.TrainState(blob)
    tr = trainer.Trainer(hp, blob, opts, batch=B)
    nsteps = 3
    for s in range(nsteps):
        data, labels, weights = _batch(hp, B, 40 + s)
        before = tr.blob()
        m0, v0 = tr.slots()
        want = to.train_step(hp, st, data, labels, weights, oo)
        got = tr.step(data, labels, weights)[0]
        assert got == pytest.approx(want, rel=2e-4), s       # later steps inherit the Adam direction ambiguity
        g = tr.grads().astype(np.float64)
        # the update, exactly, from the kernel's own gradient (fp32 arithmetic restated in float64: 1e-6 relative)
        lr = opts.lr0 * opts.decay_rate ** (s // opts.decay_steps)
        t = s + 1
        b1, b2 = np.float32(opts.beta1), np.float32(opts.beta2)      # the kernel forms 1 - beta in fp32, like TF's
        m1 = float(b1) * m0 + float(np.float32(1) - b1) * g           # ApplyAdam does on float32 variables
        v1 = float(b2) * v0 + float(np.float32(1) - b2) * g * g
        w1 = before - lr * np.sqrt(1 - opts.beta2 ** t) / (1 - opts.beta1 ** t) * m1 / (np.sqrt(v1) + opts.adam_eps)
        m_got, v_got = tr.slots()
        after = tr.blob()
        assert np.allclose(m_got, m1, rtol=1e-5, atol=2e-6 * np.abs(m1).max())     # fp32 fma with cancellation
        assert np.allclose(v_got, v1, rtol=1e-5, atol=2e-6 * np.abs(v1).max())
        T_after, T_w1 = to.split_blob(hp, after), to.split_blob(hp, w1)
        for nm in T_after:
            if to.trainable(nm):
                assert np.abs(T_after[nm] - T_w1[nm]).max() <= 1e-6 * max(1.0, np.abs(T_w1[nm]).max()), nm
        if s == 0:
            _per_tensor(hp, tr.grads(), st.last["grads"], "grads step 0")
            _per_tensor(hp, m_got, st.m, "slot m")
        # BN moving statistics (UPDATE_OPS)
        T_or = to.split_blob(hp, st.blob)
        for nm in T_after:
            if not to.trainable(nm):
                assert np.allclose(T_after[nm], T_or[nm], rtol=1e-5, atol=1e-6), nm
    assert tr.step_count == nsteps
    assert np.abs(tr.blob() - st.blob).max() <= nsteps * opts.lr0 * 1.01 + 1e-6
    tr.close()


def test_momentum_steps_match_oracle_tightly():
    """MomentumOptimizer (reference UnMicst.py:270-279) is linear in the gradient: parameters are comparable directly."""
    from oracle import train_oracle as to
    hp = helpers.small_hps()["v2_duo_like"]
    opts = trainer.TrainOptions(optimizer=trainer.OPT_MOMENTUM, lr0=0.01, decay_steps=1000, decay_rate=0.95,
                                reg_kind=trainer.REG_L2, reg_down=1e-3, reg_bottom=1e-3, reg_up=1e-3, reg_top=1e-3,
                                clip_eps=0.0, drop_down_step=0.05, drop_bottom=0.3, drop_up0=0.25, drop_up_step=0.05)
    blob = model.random_blob(hp, seed=4)
    st = to.TrainState(blob)
    tr = trainer.Trainer(hp, blob, opts, batch=4)
    for s in range(3):
        data, labels, weights = _batch(hp, 4, 70 + s)
        want = to.train_step(hp, st, data, labels, weights, _oracle_opts(opts))
        got = tr.step(data, labels, weights)[0]
        assert got == pytest.approx(want, rel=5e-5), s
    got_blob = tr.blob()
    T_g, T_w = to.split_blob(hp, got_blob), to.split_blob(hp, st.blob)
    for nm in T_w:
        assert np.abs(T_g[nm] - T_w[nm]).max() <= LOOSE * np.abs(T_w[nm] - to.split_blob(hp, blob)[nm]).max() + 2e-6, nm
    tr.close()


def test_step_is_bit_reproducible_and_trained_blob_serves_inference():
    from oracle import oracle
    hp = helpers.small_hps()["v2_wide"]
    blob = model.random_blob(hp, seed=2)
    data, labels, weights = _batch(hp, 2, 6)
    outs = []
    for _ in range(2):
        tr = trainer.Trainer(hp, blob, trainer.duo_options(), batch=2)
        losses = [tr.step(data, labels, weights)[0] for _ in range(2)]
        outs.append((losses, tr.grads(), tr.blob()))
        tr.close()
    assert outs[0][0] == outs[1][0]
    assert np.array_equal(outs[0][1], outs[1][1]) and np.array_equal(outs[0][2], outs[1][2])
    assert outs[0][0][1] < outs[0][0][0]            # same batch twice: the loss goes down
    trained = outs[0][2]
    ref = oracle.forward(hp, trained, data)
    with umx.Engine(hp, trained, max_batch=2, precision="f32") as eng:
        got = eng.forward_tiles(data)
    assert np.abs(got - ref).max() <= 1e-4


def _smallest_v2(L):
    """the v2 shape of L layers (2 channels, 3 classes, 8 features) at the smallest imSize check_create and the planner accept"""
    for sh in range(L, 10):
        hp = model.HParams(model.GRAPH_V2, 1 << sh, 2, 3, 8, L, 3, 0)
        try:
            umx.step_plan(hp, 3, model.random_blob(hp, seed=17))   # (the host pass alone)
        except umx.UmxError:
            continue
        return hp
    raise AssertionError("no imSize accepted for %d layers" % L)


def _two_steps(hp, blob, batches, serial):
    tr = trainer.Trainer(hp, blob, trainer.duo_options(), batch=3)   # (regulariser on, dropout everywhere)
    try:
        tr.test_serial(serial)
        losses = [tuple(tr.step(*b)) for b in batches]
        return losses, tr.probs().tobytes(), tr.grads().tobytes(), tr.blob().tobytes()
    finally:
        tr.close()


# The overlapped step (four streams, the plan's events) against the serial walk of the same plan (every step on the main stream in plan
# order, no events: umx_test_trainer_serial).  Every kernel has a fixed summation order and the two loss words are separate, so a step
# whose events order every hazard equals the serial walk byte for byte: losses, probabilities, the whole gradient vector and the
# parameters after the second step.  (tests/test_step_plan_cpu.py checks the same plans for hazards on the host.)
@pytest.mark.parametrize("L,route", [(3, r) for r in ROUTES] + [(1, {}), (2, {})],
                         ids=lambda v: (",".join("%s=%s" % kv for kv in v.items()) or "f16x3") if isinstance(v, dict) else "L%d" % v)
def test_overlapped_step_equals_the_serial_walk(L, route, monkeypatch):
    for k, v in route.items():
        monkeypatch.setenv(k, v)
    hp = _smallest_v2(L)
    blob = model.random_blob(hp, seed=17)
    batches = [_batch(hp, 3, 23), _batch(hp, 3, 24)]
    overlapped = _two_steps(hp, blob, batches, False)
    serial = _two_steps(hp, blob, batches, True)
    assert overlapped[0] == serial[0]
    for what, a, b in zip(("probabilities", "gradients", "parameters"), overlapped[1:], serial[1:]):
        assert a == b, what
    assert overlapped[3] != blob.tobytes()


def test_device_pointer_step_matches_host_step(torch_cuda=None):
    import torch
    hp = helpers.small_hps()["v2_duo_like"]
    blob = model.random_blob(hp, seed=12)
    data, labels, weights = _batch(hp, 4, 9)
    a = trainer.Trainer(hp, blob, trainer.duo_options(), batch=4)
    want = a.step(data, labels, weights)
    b = trainer.Trainer(hp, blob, trainer.duo_options(), batch=4)
    d, y, w = (torch.from_numpy(v).cuda() for v in (data, labels, weights))
    torch.cuda.synchronize()
    b.step_dev(d.data_ptr(), y.data_ptr(), w.data_ptr())
    assert b.loss() == want
    assert np.array_equal(a.blob(), b.blob())
    a.close()
    b.close()


def test_errors():
    hp = helpers.small_hps()["v2_duo_like"]
    blob = model.random_blob(hp)
    with pytest.raises(umx.UmxError) as e:
        trainer.Trainer(hp, blob[:-1], batch=2)
    assert e.value.code == 2
    with pytest.raises(ValueError):
        trainer.Trainer(helpers.small_hps()["legacy_k5"], model.random_blob(helpers.small_hps()["legacy_k5"]))
    tr = trainer.Trainer(hp, blob, batch=2)
    with pytest.raises(ValueError):
        tr.step(np.zeros((3, 32, 32, 2)), np.zeros((3, 32, 32, 3)), np.zeros((3, 32, 32, 3)))
    tr.close()


def test_eval_is_the_inference_mode_forward():
    """umx_trainer_eval == Session.run(UNet2D.nn, {tfTraining: 0}) with the current variables (moving statistics)."""
    from oracle import oracle
    hp = helpers.small_hps()["v2_duo_like"]
    blob = model.random_blob(hp, seed=31)
    tr = trainer.Trainer(hp, blob, trainer.duo_options(), batch=4)
    data, labels, weights = _batch(hp, 4, 2)
    assert np.abs(tr.eval(data) - oracle.forward(hp, blob, data)).max() <= 1e-5
    for s in range(2):
        tr.step(*_batch(hp, 4, 50 + s))
    now = tr.blob()
    assert not np.array_equal(now, blob)
    assert np.abs(tr.eval(data) - oracle.forward(hp, now, data)).max() <= 1e-5
    tr.close()


def test_steps_over_resident_batches_learn_and_the_result_serves_the_engine(tmp_path):
    """Row f-1 is the STEP: a plain loop over a few fixed batches calling Trainer.step (the shape of bench.py's train leg) brings the
    loss down, and the parameters it leaves are a blob the inference engine loads as they are (train -> infer without conversion)."""
    hp = model.HParams(model.GRAPH_V2, 32, 1, 3, 8, 2, 3, 0)
    blob = model.random_blob(hp, seed=11)
    rng = np.random.default_rng(5)
    batches = []
    for _ in range(3):   # a learnable rule: the class is a threshold of the (smoothed) input
        x = rng.normal(size=(4, 32, 32, 1)).astype(np.float32)
        cls = (x[..., 0] > 0.4).astype(int) + (x[..., 0] > -0.4).astype(int)
        batches.append((x, np.eye(3, dtype=np.float32)[cls], np.ones((4, 32, 32, 3), np.float32)))
    tr = trainer.Trainer(hp, blob, trainer.solo_options(), batch=4)
    losses = [tr.step(*batches[i % 3])[0] for i in range(60)]
    assert np.mean(losses[-10:]) < np.mean(losses[:10])
    model.save_converted(model.ModelArtefacts(hp, tr.blob(), 0.0, 1.0), str(tmp_path / "model"))
    tr.close()
    art = model.load_model_dir(str(tmp_path / "model"))
    with umx.Engine(art.hp, art.blob, max_batch=2) as eng:
        p = eng.forward_tiles(np.zeros((1, 32, 32, 1), np.float32))
    assert np.allclose(p.sum(-1), 1.0, atol=1e-5)


def test_the_loops_around_the_step_are_refused():
    from unmicst_amd.unet2d import UNet2D
    with pytest.raises(NotImplementedError):
        UNet2D.train()
    with pytest.raises(NotImplementedError):
        UNet2D.deploy()


def test_weight_scale_refresh_does_not_change_a_result(monkeypatch):
    """UMX_TRAIN_WSCALE_EVERY: the power-of-two scale of each layer's repacked weights is re-derived from the parameters every N steps
    (default 256: a long run cannot grow a filter out of the 32 x headroom the scale of step 0 left it).  Refreshing before every
    step must give bit-identical losses to never refreshing: a scale is a power of two and is undone exactly in the epilogue."""
    hp = helpers.small_hps()["v2_wide"]
    blob = model.random_blob(hp, seed=5)
    data, labels, weights = _batch(hp, 2, 9)
    losses = []
    for every in ("0", "1"):
        monkeypatch.setenv("UMX_TRAIN_WSCALE_EVERY", every)
        tr = trainer.Trainer(hp, blob, trainer.duo_options(), batch=2)
        losses.append([tr.step(data, labels, weights)[0] for _ in range(4)])
        tr.close()
        monkeypatch.delenv("UMX_TRAIN_WSCALE_EVERY")
    assert losses[0] == losses[1], losses


def test_the_two_convolution_routes_agree_step_for_step(monkeypatch):
    """Three Adam steps of the duo regime (dropout on) on the split-precision route and on the exact-fp32 route: same losses to
    1e-6 relative, same parameters to 1e-5 of each tensor's scale (2^-22 per product against fp32 rounding -- and the routes must take
    every LeakyReLU / pool / dropout decision alike on this batch for that to hold)."""
    from oracle import train_oracle as to
    hp = helpers.small_hps()["v2_wide"]
    blob = model.random_blob(hp, seed=5)
    data, labels, weights = _batch(hp, 2, 9)
    out = []
    for env in ({}, {"UMX_TRAIN_CONV_F32": "1"}):
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        tr = trainer.Trainer(hp, blob, trainer.duo_options(), batch=2)
        losses = [tr.step(data, labels, weights)[0] for _ in range(3)]
        out.append((losses, tr.blob()))
        tr.close()
        for k in env:
            monkeypatch.delenv(k)
    (la, ba), (lb, bb) = out
    assert np.allclose(la, lb, rtol=1e-6, atol=0), (la, lb)
    A, Bv = to.split_blob(hp, ba), to.split_blob(hp, bb)
    for name in A:
        assert np.abs(A[name] - Bv[name]).max() <= 1e-5 * np.abs(Bv[name]).max() + 1e-7, name


def test_baseline_config_256x256x2_batch8_against_the_oracle():
    """BASELINE.json configs[4] at full size: synthetic-256 hyper-parameters (duo widths 36..1152, 5 levels), batch 8 of
    256 x 256 x 2, duo regime -- loss and EVERY gradient tensor against the float64 oracle at TIGHT (about a minute of CPU).

    4.7 M LeakyReLU decisions per full-resolution tensor: some sit within rounding distance of zero and fall the other way in
    float64, and every gradient below such a flip moves by 1e-4 .. 3e-2 of its scale (rounds 1-4 therefore held this size to 0.1 --
    a band that would also hide a wrong weight gradient in a deep layer).  Here the oracle differentiates the loss ON THE KERNELS'
    OWN DECISIONS (_hip_decisions): the same smooth piece of the function, so nothing is excused -- and the flips are counted."""
    import torch
    from oracle import train_oracle as to
    hp = model.KNOWN_HP["synthetic-256"]
    opts = trainer.duo_options()
    blob = model.random_blob(hp, seed=20260101)
    data, labels, weights = _batch(hp, 8, 11)
    tr = trainer.Trainer(hp, blob, opts, batch=8)
    loss, data_term, reg = tr.step(data, labels, weights, apply_update=False)
    g = tr.grads()
    dec = _hip_decisions(tr.read_tensor, hp, opts, 0, 8)
    tr.close()
    torch.set_num_threads(max(1, torch.get_num_threads()))
    trace = {}
    want = to.loss_and_grads(hp, blob, data, labels, weights, _oracle_opts(opts), step=0, decisions=dec, trace=trace)
    assert loss == pytest.approx(want[0], rel=1e-5)
    assert reg == pytest.approx(want[2], rel=1e-5)
    flips = _count_flips(dec, trace)
    total = sum(f for f, _ in flips.values())
    for site, (f, n) in flips.items():
        assert f <= 1e-4 * n + 2, (site, f, n)      # rounding-distance events only: a broken reconstruction flips percents
    worst = _per_tensor(hp, g, want[3], "grads at 256x256x2, batch 8, on the kernels' decisions", rel=TIGHT, top=TIGHT)
    print("worst relative gradient error %.2e with %d of %d decisions differing from the float64 run's (%s)" % (
        worst, total, sum(n for _, n in flips.values()), ", ".join("%s %d" % (k, f) for k, (f, _) in flips.items() if f)))


def test_weight_gradient_of_a_deep_layer_against_finite_differences_of_the_kernels_own_loss():
    """Independent of any oracle: the bottom layer's filter gradient (lb.w, 576 -> 1152 channels at 8 x 8: wgrad_f16x3 on a deep
    layer, K split and all) at the BASELINE size against a central finite difference of the HIP step's OWN loss along the
    gradient's direction: (L(w + h d) - L(w - h d)) / 2h = <g, d> = |g| for d = g / |g|.  The loss comes back as float64 sums of a
    float32-equivalent forward pass (1e-7 relative noise); h moves it by 2e-3 of itself, so the difference quotient is good to
    ~1e-4 plus curvature; a wrong scale, a dropped tap or a mis-reduced K slice moves it by O(1)."""
    from oracle import train_oracle as to
    hp = model.KNOWN_HP["synthetic-256"]
    opts = trainer.duo_options()
    blob = model.random_blob(hp, seed=20260101).astype(np.float32)
    data, labels, weights = _batch(hp, 8, 11)
    tr = trainer.Trainer(hp, blob, opts, batch=8)
    loss0 = tr.step(data, labels, weights, apply_update=False)[0]
    g = tr.grads()
    tr.close()
    off = {}
    pos = 0
    for name, shape in to.tensor_specs(hp):
        off[name] = (pos, int(np.prod(shape)))
        pos += int(np.prod(shape))
    for name in ("lb.w", "lu4.w2"):
        a, n = off[name]
        G = g[a:a + n].astype(np.float64)
        norm = float(np.sqrt((G * G).sum()))
        d = G / norm
        h = 2e-3 * abs(loss0) / norm
        L = []
        for sgn in (+1.0, -1.0):
            b2 = blob.astype(np.float64).copy()
            b2[a:a + n] += sgn * h * d
            t2 = trainer.Trainer(hp, b2.astype(np.float32), opts, batch=8)
            L.append(t2.step(data, labels, weights, apply_update=False)[0])
            t2.close()
        # (the perturbed blobs are rounded to float32: the realised step is what the two blobs actually differ by)
        bp = (blob.astype(np.float64)[a:a + n] + h * d).astype(np.float32).astype(np.float64)
        bm = (blob.astype(np.float64)[a:a + n] - h * d).astype(np.float32).astype(np.float64)
        realised = float(((bp - bm) * d).sum())          # = 2h up to the rounding of the blobs
        fd = (L[0] - L[1]) / realised
        assert fd == pytest.approx(norm, rel=5e-3), (name, fd, norm, loss0, h)
        print("%s: finite difference %.6e, |gradient| %.6e (%.2e relative)" % (name, fd, norm, abs(fd / norm - 1)))


@pytest.mark.parametrize("hp_args,B", [
    ((16, 1, 2, 4, 1, 3, 0), 1),      # one level, one image, two classes, 8x8 bottom
    ((16, 3, 4, 5, 2, 3, 0), 5),      # three input channels, four classes, odd widths and batch, 4x4 bottom
    ((64, 2, 3, 6, 5, 3, 0), 2),      # five levels down to a 2x2 bottom
    ((16, 1, 3, 8, 2, 5, 0), 3),      # 5x5 filters on 4x4 layers (fp32 weight-gradient path, big halos)
    ((128, 1, 3, 4, 2, 3, 0), 1),     # one large image
])
def test_odd_shapes_match_oracle(hp_args, B):
    """Shapes off the beaten path: every launch geometry (image groups, partial channel tiles, tiny layers) must still be
    right -- loss 1e-5, gradients within the discontinuity bound against the free float64 run and within TIGHT on the kernels' own
    decisions (train_parity.check_on_decisions), nothing out of range."""
    from oracle import train_oracle as to
    hp = model.HParams(model.GRAPH_V2, *hp_args)
    opts = trainer.duo_options()
    blob = model.random_blob(hp, seed=17)
    data, labels, weights = _batch(hp, B, 23)
    want = to.loss_and_grads(hp, blob, data, labels, weights, _oracle_opts(opts), step=0)
    tr = trainer.Trainer(hp, blob, opts, batch=B)
    loss, _, reg = tr.step(data, labels, weights, apply_update=False)
    assert loss == pytest.approx(want[0], rel=1e-5)
    _per_tensor(hp, tr.grads(), want[3], "odd shape grads", rel=0.1, top=0.1)
    assert np.abs(tr.probs() - want[4]).max() <= 2e-5
    # ... and, on the kernels' own decisions, every gradient tensor within TIGHT (and the decisions within the flip cap)
    dec = _hip_decisions(tr.read_tensor, hp, opts, 0, B)
    trace = {}
    on_dec = to.loss_and_grads(hp, blob, data, labels, weights, _oracle_opts(opts), step=0, decisions=dec, trace=trace)
    train_parity.check_on_decisions(hp, {"loss": loss, "reg": reg, "probs": tr.probs(), "grads": tr.grads()}, on_dec, dec, trace,
                                    "odd shape %r" % (hp_args,))
    l2 = tr.step(data, labels, weights)[0]
    assert l2 == pytest.approx(want[0], rel=1e-5) and tr.step_count == 1
    tr.close()
