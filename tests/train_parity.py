"""Shared parity code of the v2 training tests: one step of the HIP trainer against oracle/train_oracle.py ON THE DECISIONS THE
STEP UNDER TEST TOOK (every LeakyReLU branch, every max-pool choice), so that both differentiate the same smooth piece of the loss
and every gradient tensor can be held to TIGHT -- plus the count of decisions that differ from the float64 run's own, which is what
catches a WRONG branch (an on-decisions check follows whatever branch it is given).

Nothing here needs a GPU: `_hip_decisions` reads its tensors through any callable name -> array.  tests/test_train_parity_cpu.py
feeds it from a float32 run of the oracle (`StandIn`), tests/test_gpu_train*.py from umx_trainer_read_tensor."""
import numpy as np

TIGHT, LOOSE = 2e-5, 5e-2
TOP = ("lt.w", "lt.bn.gamma", "lt.bn.beta", "lu0.bn.gamma", "lu0.bn.beta", "lu0.w2")
FLIP_RATE, FLIP_SLACK = 1e-4, 2       # per site: flips <= FLIP_RATE * n + FLIP_SLACK (rounding-distance events only)


def _batch(hp, B, seed):
    rng = np.random.default_rng(seed)
    data = rng.normal(0, 1, (B, hp.imSize, hp.imSize, hp.nChannels)).astype(np.float32)
    cls = rng.integers(0, hp.nClasses, (B, hp.imSize, hp.imSize))
    labels = np.eye(hp.nClasses, dtype=np.float32)[cls]
    weights = rng.uniform(0.5, 3.0, labels.shape).astype(np.float32)
    return data, labels, weights


def _oracle_opts(o):
    """trainer.TrainOptions -> the oracle's."""
    from oracle import train_oracle as to
    from unmicst_amd import trainer
    kw = {k: getattr(o, k) for k in ("lr0", "decay_steps", "decay_rate", "momentum", "beta1", "beta2", "adam_eps",
                                      "reg_kind", "reg_down", "reg_bottom", "reg_up", "reg_top", "clip_eps",
                                      "drop_down_step", "drop_bottom", "drop_up0", "drop_up_step", "bn_momentum", "seed")}
    kw["optimizer"] = "adam" if o.optimizer == trainer.OPT_ADAM else "momentum"
    return to.TrainOptions(**kw)


def _per_tensor(hp, got, want, what, rel=LOOSE, top=TIGHT):
    """-> worst relative error over the tensors; asserts rel on every tensor and `top` on the top of the graph."""
    from oracle import train_oracle as to
    G, W = to.split_blob(hp, got), to.split_blob(hp, want)
    worst = 0.0
    for name in W:
        scale = np.abs(W[name]).max()
        err = np.abs(G[name] - W[name]).max()
        assert err <= (top if name in TOP else rel) * scale + 1e-7, (what, name, err, scale)
        worst = max(worst, err / (scale + 1e-30))
    return worst


def _hip_decisions(read, hp, opts, step, B):
    """The LeakyReLU branches and max-pool choices a step took in its last forward pass, rebuilt from the tensors they were taken on
    (`read`: tensor name -> flat array, e.g. Trainer.read_tensor): BN output = z * scale + shift evaluated exactly (float64 product
    of two float32 + one rounding: the sign of the kernels' fused multiply-add), the pooled element = first maximum of
    act(v) * dropout in float32 like act_fwd_kernel.  Given to the oracle (train_oracle.forward(decisions=...)) the two
    implementations differentiate the SAME smooth piece of the loss, so every gradient tensor can be held to TIGHT -- at any size,
    however many activations sit within rounding distance of zero."""
    import torch
    from oracle import train_oracle as to
    n, L, S = hp.nOutX, hp.nLayers, hp.imSize
    dec = {}

    def nchw(a):
        return torch.from_numpy(np.ascontiguousarray(a.transpose(0, 3, 1, 2)))

    def bn_value(layer, S, C):
        z = np.asarray(read(layer + ".z")).reshape(B, S, S, C).astype(np.float64)
        st = np.asarray(read(layer + ".stat")).reshape(4, C).astype(np.float64)
        return z * st[2] + st[3]

    for i in range(L):
        C = n[i + 1]
        v = bn_value("ld%d" % i, S, C)
        dec["ld%d" % i] = nchw(np.where(v > 0, 1.0, to.LEAK))
        v32 = v.astype(np.float32)
        y = np.where(v32 > 0, v32, np.float32(0.2) * v32).astype(np.float32)
        m = to.dropout_mask(opts.seed, step, to.LAYER_DOWN + i, (B, S, S, C), opts.drop_down_step * i).astype(np.float32)
        y = y * m
        win = y.reshape(B, S // 2, 2, S // 2, 2, C).transpose(0, 1, 3, 5, 2, 4).reshape(B, S // 2, S // 2, C, 4)   # element 2 dy + dx
        dec["pool%d" % i] = torch.from_numpy(np.ascontiguousarray(win.argmax(-1).transpose(0, 3, 1, 2))).long()
        S //= 2
    dec["lb"] = nchw(np.where(bn_value("lb", S, n[L + 1]) > 0, 1.0, to.LEAK))
    for idx in range(L - 1, -1, -1):
        S *= 2
        C = n[idx + 1]
        us = np.asarray(read("lu%d.us" % idx)).reshape(B, S, S, C)
        dec["us%d" % idx] = nchw(np.where(us > 0, 1.0, to.LEAK))
        dec["lu%d" % idx] = nchw(np.where(bn_value("lu%d" % idx, S, C) > 0, 1.0, to.LEAK))
    return dec


def _count_flips(dec, trace):
    """Per site: decisions of `dec` (the kernels') that differ from what the oracle's own values (trace) would take."""
    flips = {}
    for site, d in dec.items():
        a = trace[site]
        if site.startswith("pool"):
            B, C, H, W = a.shape
            win = a.reshape(B, C, H // 2, 2, W // 2, 2).permute(0, 1, 2, 4, 3, 5).reshape(B, C, H // 2, W // 2, 4)
            own = win.argmax(-1)
            flips[site] = (int((own != d).sum()), int(d.numel()))
        else:   # (slopes: 1 on the positive branch, 0.2 on the other)
            flips[site] = (int(((a > 0) != (d > 0.5)).sum()), int(d.numel()))
    return flips


def check_on_decisions(hp, got, want, dec, trace, what):
    """The whole on-decisions check of one step.  got: {"loss", "reg", "probs", "grads"} of the step under test; want: what
    train_oracle.loss_and_grads(..., decisions=dec, trace=trace) returned (float64); dec: the decisions of the step under test.

    Asserts loss and regulariser 1e-5 relative, probabilities 2e-5 max-abs, per site flips <= 1e-4 * n + 2 against the float64 run's
    own branches, and every trainable tensor's gradient within TIGHT of that tensor's max-abs value (+ 1e-7); every message names what
    failed (the site, the tensor).  -> {"worst": worst relative gradient error, "tensor": its name, "flips": {site: count} of the
    sites with any, "sites": number of decisions}."""
    import pytest
    from oracle import train_oracle as to
    assert got["loss"] == pytest.approx(want[0], rel=1e-5), (what, "loss", got["loss"], want[0])
    assert got["reg"] == pytest.approx(want[2], rel=1e-5), (what, "reg", got["reg"], want[2])
    perr = float(np.abs(np.asarray(got["probs"], np.float64) - want[4]).max())
    assert perr <= 2e-5, (what, "probs", perr)
    flips = _count_flips(dec, trace)
    for site, (f, n) in flips.items():
        assert f <= FLIP_RATE * n + FLIP_SLACK, (what, "decisions of %s" % site, f, n)
    G, W = to.split_blob(hp, got["grads"]), to.split_blob(hp, want[3])
    worst, worst_name = 0.0, None
    for name in W:
        if not to.trainable(name):
            continue
        scale = np.abs(W[name]).max()
        err = np.abs(G[name] - W[name]).max()
        assert err <= TIGHT * scale + 1e-7, (what, name, err, scale)
        if err / (scale + 1e-30) > worst:
            worst, worst_name = err / (scale + 1e-30), name
    return {"worst": worst, "tensor": worst_name, "flips": {s: f for s, (f, _) in flips.items() if f},
            "sites": sum(n for _, n in flips.values())}


class StandIn:
    """A float32 run of the oracle standing in for the HIP step: the same outputs (`got` of check_on_decisions) and, through
    read_tensor, the tensors umx_trainer_read_tensor serves for _hip_decisions -- <layer>.z (NHWC), <layer>.stat ([mean, 1/sqrt(var +
    eps), scale, shift]) and lu<i>.us -- taken from the oracle's trace.  The run evaluates batch normalisation as the kernels do
    (fused_bn: z * scale + shift with one rounding), so the branches it took are a function of exactly those tensors."""

    def __init__(self, hp, blob, data, labels, weights, oopts, step=0):
        import torch
        from oracle import train_oracle as to
        self.trace = {}
        out = to.loss_and_grads(hp, blob, data, labels, weights, oopts, step=step, dtype=torch.float32, trace=self.trace, fused_bn=True)
        self.got = {"loss": out[0], "reg": out[2], "probs": out[4], "grads": np.asarray(out[3], np.float64)}

    def read_tensor(self, name):
        t = self.trace["us" + name[2:-3] if name.endswith(".us") else name]          # lu<i>.us: the tensor in front of site us<i>
        a = t.numpy()
        return np.ascontiguousarray(a.transpose(0, 2, 3, 1) if a.ndim == 4 else a).ravel()

    def branches(self):
        """The decisions the float32 run actually took, from the tensors in front of them: {site: bool NCHW (positive branch) |
        int64 window element 2 dy + dx of max_pool2d's own choice}."""
        import torch.nn.functional as F
        out = {}
        for site, a in self.trace.items():
            if site.startswith("pool"):
                W = a.shape[3]
                idx = F.max_pool2d(a, 2, return_indices=True)[1]          # flat y * W + x of the chosen element
                out[site] = 2 * ((idx // W) % 2) + (idx % W) % 2
            elif "." not in site:
                out[site] = a > 0
        return out


# ---- the cases of tests/test_gpu_train_tight.py, each proven on the stand-in by tests/test_train_parity_cpu.py ---------------------
ROUTES = [{}, {"UMX_TRAIN_CONV_F32": "1"}, {"UMX_TRAIN_NO_KSPLIT": "1"}, {"UMX_TRAIN_WGRAD_F32": "1"},
          {"UMX_TRAIN_CONV_F32": "1", "UMX_TRAIN_WGRAD_F32": "1"}]          # tests/test_gpu_train.py::ROUTES
ROUTE_IDS = [",".join("%s=%s" % kv for kv in r.items()) or "f16x3" for r in ROUTES]


def trainer_options(regime):
    from unmicst_amd import trainer
    if regime == "momentum":   # the configuration of tests/test_gpu_train.py::test_momentum_steps_match_oracle_tightly
        return trainer.TrainOptions(optimizer=trainer.OPT_MOMENTUM, lr0=0.01, decay_steps=1000, decay_rate=0.95,
                                    reg_kind=trainer.REG_L2, reg_down=1e-3, reg_bottom=1e-3, reg_up=1e-3, reg_top=1e-3,
                                    clip_eps=0.0, drop_down_step=0.05, drop_bottom=0.3, drop_up0=0.25, drop_up_step=0.05)
    return {"solo": trainer.solo_options, "duo": trainer.duo_options}[regime]()


def tight_cases():
    """id -> (hp, batch, regime, blob seed, batch seed).  HParams(GRAPH_V2, imSize, nChannels, nClasses, nOut0, nLayers, ks, nExtraConvs);
    the convolutions put 256 / (H * W) images of a layer smaller than 16 x 16 into one tile (4 at 8 x 8, 16 at 4 x 4, 64 at 2 x 2)."""
    import helpers
    from unmicst_amd import model
    small = helpers.small_hps()

    def v2(*a):
        return model.HParams(model.GRAPH_V2, *a)

    cases = {
        # tests/test_gpu_train.py::CASES (blob seed 21, batch seed 3)
        "v2_solo_like-solo": (small["v2_solo_like"], 4, "solo", 21, 3),
        "v2_duo_like-duo": (small["v2_duo_like"], 4, "duo", 21, 3),
        "v2_deep-duo": (small["v2_deep"], 3, "duo", 21, 3),
        "v2_wide-solo": (small["v2_wide"], 2, "solo", 21, 3),
        "v2_wide-duo": (small["v2_wide"], 2, "duo", 21, 3),
        "v2_k5-duo": (v2(32, 2, 3, 8, 2, 5, 0), 3, "duo", 21, 3),
        # tests/test_gpu_train.py::test_odd_shapes_match_oracle (blob seed 17, batch seed 23)
        "odd_b1_l1": (v2(16, 1, 2, 4, 1, 3, 0), 1, "duo", 17, 23),
        "odd_c3k4": (v2(16, 3, 4, 5, 2, 3, 0), 5, "duo", 17, 23),
        "odd_l5_2x2": (v2(64, 2, 3, 6, 5, 3, 0), 2, "duo", 17, 23),
        "odd_k5_4x4": (v2(16, 1, 3, 8, 2, 5, 0), 3, "duo", 17, 23),
        "odd_128": (v2(128, 1, 3, 4, 2, 3, 0), 1, "duo", 17, 23),
        # partial image groups: 7 images = one full tile of four 8 x 8 images + three, and 7 of the 16 a tile of 4 x 4 images holds;
        # 3 of the 64 a tile of 2 x 2 images holds (and 3 of 16, 3 of 4 on the layers above)
        "group_b7_l3": (v2(32, 1, 3, 8, 3, 3, 0), 7, "solo", 17, 23),
        "group_b3_l5": (v2(64, 2, 3, 4, 5, 3, 0), 3, "duo", 17, 23),
        # scalar channel paths: channel counts and concat offsets that are no multiples of 4 (vecx / vecg off)
        "scalar_n6": (v2(32, 1, 3, 6, 2, 3, 0), 2, "solo", 17, 23),
        "scalar_n5": (v2(32, 2, 3, 5, 2, 3, 0), 3, "duo", 17, 23),
        # a first layer that is not thin: more than 4 input channels
        "first_c5": (v2(32, 5, 3, 8, 2, 3, 0), 2, "duo", 17, 23),
        "first_c9": (v2(32, 9, 3, 8, 2, 3, 0), 2, "solo", 17, 23),
        # the wide first layer: more than 128 filters on one input channel
        "first_wide": (v2(16, 1, 3, 132, 1, 3, 0), 2, "duo", 17, 23),
        # class counts: the head kernels loop over K
        "classes_2": (v2(32, 1, 2, 8, 2, 3, 0), 3, "solo", 17, 23),
        "classes_5": (v2(32, 2, 5, 8, 2, 3, 0), 3, "duo", 17, 23),
        # the MomentumOptimizer configuration on v2 (L2 1e-3, dropout everywhere)
        "momentum": (small["v2_duo_like"], 4, "momentum", 17, 23),
    }
    return cases


STEP1_CASES = ("v2_duo_like-duo", "scalar_n5", "momentum")      # a second step after one applied update (dropout stream of step 1)
