#!/usr/bin/env python3
"""The reference side of the inference arithmetic gate (checked by tests/test_inference_arith_cpu.py) -- CPU only.  The GPU side is
tests/test_gpu_arith.py: every precision of the engine held to `tol` / `tol_f6` of tests/arith_cases.json against forward64.

Three things live here:

* ``forward64``: a plain float64 forward of both graphs in inference mode, written from oracle/unet_oracle.c and the launch list of
  umx_describe_graph (moving-statistics BatchNorm, (Leaky)ReLU, max-pool, stride-2 transposed convolutions, concat order, the 1 x 1
  head, softmax).  It never touches the engine.
* the emulation of the engine's split-precision arithmetic (``split16``, the MX block quantisers, ``gemm``, ``conv_same``,
  ``conv_transpose_s2``, ``forward``), moved here from tests/fp8_cross_term_report.py, with two fault plans added to ``gemm``:
  ``f16x3-xlo`` (x_lo * w_hi omitted) and ``f16x3-wlo`` (x_hi * w_lo omitted).
* ``ARITH_CASES`` and the table tests/arith_cases.json derived from them (``python tests/inference_ref.py --write``): per case
  E_ref  = max(max |oracle.forward - p64|, max |emulated f16x3 - p64|)      what two CPU restatements of the correct arithmetic give
  E_drop = min over layers and both fault plans of max |emulated - p64|     one product lost on ONE layer, the others on f16x3
  E_f6   = max |emulated - p64| with fp6x on the launches the planner gives the F6 form (cases that have one)
  tol    = E_drop / 4,  tol_f6 = 4 * E_f6
  The conditions a case must meet (``case_conditions``) are stated on these reference-side numbers only.
"""
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
if os.path.join(ROOT, "tests") not in sys.path:
    sys.path.insert(0, os.path.join(ROOT, "tests"))

import helpers  # noqa: E402
from unmicst_amd import model  # noqa: E402

BN_EPS = 1e-3
LEAK = 0.2
TABLE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "arith_cases.json")


# ------------------------------------------------------------------------------------------------ number formats
def f16(x):
    return x.to(torch.float16).to(torch.float32)


def split16(x):
    hi = f16(x)
    return hi, f16(x - hi)


def q_e4m3(v):
    """Round-to-nearest-even onto OCP e4m3 (bias 7, 3 mantissa bits, subnormals at 2^-9, max 448, saturating)."""
    a = v.abs().clamp(max=448.0)
    e = torch.floor(torch.log2(torch.where(a > 0, a, torch.ones_like(a)))).clamp(min=-6.0)   # exponent of the binade (subnormal: -6)
    ulp = torch.exp2(e - 3.0)
    q = torch.round(a / ulp) * ulp            # torch.round = half to even
    return torch.sign(v) * q.clamp(max=448.0)


def q_e2m3(v):
    """Round-to-nearest-even onto OCP fp6 e2m3 (bias 1, 3 mantissa bits, subnormals in steps of 1/8 below 1, max 7.5, saturating)."""
    a = v.abs().clamp(max=7.5)
    e = torch.floor(torch.log2(torch.where(a > 0, a, torch.ones_like(a)))).clamp(min=0.0)
    ulp = torch.exp2(e - 3.0)
    return torch.sign(v) * (torch.round(a / ulp) * ulp).clamp(max=7.5)


def mx_block(m, axis, q, emax):
    """MX block format along `axis` (K): blocks of 32, shared e8m0 scale 2^(floor(log2(max|block|)) - emax), elements quantised by q."""
    m = m.movedim(axis, -1)
    K = m.shape[-1]
    pad = (-K) % 32
    mp = F.pad(m, (0, pad))
    blk = mp.reshape(*mp.shape[:-1], -1, 32)
    amax = blk.abs().amax(dim=-1, keepdim=True)
    scale = torch.exp2(torch.floor(torch.log2(torch.where(amax > 0, amax, torch.ones_like(amax)))) - emax)
    deq = q(blk / scale) * scale
    return deq.reshape(*mp.shape)[..., :K].movedim(-1, axis)


def mx_e2m3(m, axis):
    return mx_block(m, axis, q_e2m3, 2.0)


def mx_e4m3(m, axis):
    """MX block format along `axis` (K): blocks of 32, shared scale 2^(floor(log2(max|block|)) - 8), elements e4m3."""
    m = m.movedim(axis, -1)
    K = m.shape[-1]
    pad = (-K) % 32
    mp = F.pad(m, (0, pad))
    blk = mp.reshape(*mp.shape[:-1], -1, 32)
    amax = blk.abs().amax(dim=-1, keepdim=True)
    scale = torch.exp2(torch.floor(torch.log2(torch.where(amax > 0, amax, torch.ones_like(amax)))) - 8.0)
    deq = q_e4m3(blk / scale) * scale
    return deq.reshape(*mp.shape)[..., :K].movedim(-1, axis)


# ------------------------------------------------------------------------------------------------ the emulated GEMM
FAULT_PLANS = ("f16x3-xlo", "f16x3-wlo")


def gemm(A, Wm, plan):
    """A [M, K] activations (fp32 values as the previous layer produced them), Wm [K, N] weights -> [M, N].
    plan: 'exact' (float64), 'f16x3', 'f16x2' (x_lo*w_hi dropped: the input rounded to binary16), 'fp8x' / 'fp6x' (cross terms in MX e4m3 / MX e2m3);
    the fault plans 'f16x3-xlo' (x_lo*w_hi omitted: 'f16x2' under the name the gate uses) and 'f16x3-wlo' (x_hi*w_lo omitted)."""
    if plan == "exact":
        return (A.double() @ Wm.double()).float()
    wmax = float(Wm.abs().max())
    sh = 0.0 if wmax == 0 else 14 - (np.frexp(wmax)[1])          # largest |w| lands in [2^13, 2^14): the planner's weight shift
    Ws = Wm * (2.0 ** sh)
    wh, wl = split16(Ws)
    xh, xl = split16(A)
    acc = (xh.double() @ wh.double())
    if plan == "f16x3":
        acc = acc + xh.double() @ wl.double() + xl.double() @ wh.double()
    elif plan in ("f16x2", "f16x3-xlo"):
        acc = acc + xh.double() @ wl.double()
    elif plan == "f16x3-wlo":
        acc = acc + xl.double() @ wh.double()
    elif plan == "fp8x":
        acc = acc + mx_e4m3(xh, 1).double() @ mx_e4m3(wl, 0).double() + mx_e4m3(xl, 1).double() @ mx_e4m3(wh, 0).double()
    elif plan == "fp6x":
        acc = acc + mx_e2m3(xh, 1).double() @ mx_e2m3(wl, 0).double() + mx_e2m3(xl, 1).double() @ mx_e2m3(wh, 0).double()
    else:
        raise ValueError(plan)
    return (acc * (2.0 ** -sh)).float()


def conv_same(x, w_tf, plan):
    """x NCHW fp32, w_tf [kh, kw, Cin, Cout]; K ordered (tap, channel) like the engine's (tap, octet) pairs."""
    kh, kw, Ci, Co = w_tf.shape
    B, _, H, W = x.shape
    cols = F.unfold(x, (kh, kw), padding=(kh // 2, kw // 2))                 # [B, Ci*kh*kw, H*W], K order (channel, tap)
    cols = cols.reshape(B, Ci, kh * kw, H * W).permute(0, 3, 2, 1).reshape(B * H * W, kh * kw * Ci)
    out = gemm(cols, w_tf.reshape(kh * kw * Ci, Co), plan)
    return out.reshape(B, H, W, Co).permute(0, 3, 1, 2)


def conv_transpose_s2(x, wt_tf, plan):
    """tf.nn.conv2d_transpose, stride 2, SAME (crop (k-2)//2 before): per output phase a GEMM over that phase's taps."""
    kh, kw, Co, Ci = wt_tf.shape
    B, _, H, W = x.shape
    pb = max(kh - 2, 0) // 2
    out = torch.zeros(B, Co, 2 * H, 2 * W)
    xp = F.pad(x, (2, 2, 2, 2))
    for oy in range(2):
        for ox in range(2):
            # output (2i+oy, 2j+ox) = sum over taps a with (2i + oy + pb - a) even: input row (2i + oy + pb - a) / 2
            cols, ws = [], []
            for a in range(kh):
                if (oy + pb - a) % 2:
                    continue
                dy = (oy + pb - a) // 2
                for b in range(kw):
                    if (ox + pb - b) % 2:
                        continue
                    dx = (ox + pb - b) // 2
                    cols.append(xp[:, :, 2 + dy:2 + dy + H, 2 + dx:2 + dx + W])
                    ws.append(wt_tf[a, b].t())                                   # [Ci, Co]
            A = torch.stack(cols, 1).permute(0, 3, 4, 1, 2).reshape(B * H * W, len(cols) * Ci)
            o = gemm(A, torch.cat(ws, 0), plan).reshape(B, H, W, Co).permute(0, 3, 1, 2)
            out[:, :, oy::2, ox::2] = o
    return out


def bn(x, T, p):
    g, b, mu, va = (T[p + ".bn." + t] for t in ("gamma", "beta", "mean", "var"))
    s = g / torch.sqrt(va + BN_EPS)
    return x * s[None, :, None, None] + (b - mu * s)[None, :, None, None]


def forward(hp, T, x_nhwc, plan_of):
    """plan_of(layer name) -> plan; graph order follows oracle/unet_oracle.c (reference UnMicst1-5.py:83-237 / UnMicst.py:51-187).
    plan_of may also return {launch suffix: plan} for a layer whose launches differ (the engine's names: "conv" / "conv1" /
    "extraN" / "convT" / "head"; a shortcut belongs to the launch that adds it); suffixes it leaves out run 'f16x3'."""
    v2 = hp.graph == model.GRAPH_V2
    act = (lambda t: F.leaky_relu(t, LEAK)) if v2 else F.relu
    L = hp.nLayers
    nx = hp.nExtraConvs

    def pl(n, part):
        p = plan_of(n)
        return p if isinstance(p, str) else p.get(part, "f16x3")

    x = x_nhwc.permute(0, 3, 1, 2)
    ds = [x]
    for i in range(L):
        n = "ld%d" % i
        c = conv_same(ds[i], T[n + ".w1"], pl(n, "conv1" if nx else "conv"))
        for e in range(nx):
            c = conv_same(act(c), T["%s.wextra%d" % (n, e)], pl(n, "extra%d" % e))
        c = c + conv_same(ds[i], T[n + ".wshort"], pl(n, "extra%d" % (nx - 1) if nx else "conv"))
        c = act(bn(c, T, n)) if v2 else bn(act(c), T, n)
        ds.append(F.max_pool2d(c, 2))
    cur = conv_same(ds[L], T["lb.w"], pl("lb", "conv"))
    cur = act(bn(cur, T, "lb")) if v2 else act(cur)
    for idx in range(L - 1, -1, -1):
        n = "lu%d" % idx
        us = act(conv_transpose_s2(cur, T[n + ".wt"], pl(n, "convT")))
        cv = conv_same(torch.cat([ds[idx], us], 1), T[n + ".w2"], pl(n, "conv"))
        cv = act(bn(cv, T, n)) if v2 else act(cv)
        for e in range(nx):
            cv = act(conv_same(cv, T["%s.wextra%d" % (n, e)], pl(n, "extra%d" % e)))
        cur = cv
    t = conv_same(cur, T["lt.w"], pl("lt", "head"))
    if v2:
        t = bn(t, T, "lt")
    return torch.softmax(t, 1).permute(0, 2, 3, 1)


def layer_names(hp):
    """The layers a plan is chosen for, in execution order."""
    L = hp.nLayers
    return ["ld%d" % i for i in range(L)] + ["lb"] + ["lu%d" % i for i in range(L - 1, -1, -1)] + ["lt"]


def torch_tensors(hp, blob, dtype=torch.float32):
    return {k: torch.from_numpy(np.ascontiguousarray(v)).to(dtype) for k, v in model.tensors_from_blob(hp, blob).items()}


def emulate(hp, blob, x, plan_of):
    """The emulated engine on a float32 NHWC batch -> probabilities (numpy float32)."""
    with torch.no_grad():
        return forward(hp, torch_tensors(hp, blob), torch.from_numpy(np.array(x, np.float32)), plan_of).numpy()   # (a copy: x may be read-only)


# ------------------------------------------------------------------------------------------------ the float64 forward
def _conv64(x, w_tf):
    """SAME convolution, stride 1: x NCHW, w_tf [kh, kw, Cin, Cout] (TensorFlow's layout; odd kernels pad (k - 1) / 2 on both sides)."""
    return F.conv2d(x, w_tf.permute(3, 2, 0, 1), padding=(w_tf.shape[0] // 2, w_tf.shape[1] // 2))


def _convT64(x, wt_tf):
    """tf.nn.conv2d_transpose(stride 2, SAME) to twice the size: the gradient of a stride-2 SAME convolution whose padding of
    k - 2 puts (k - 2) // 2 before -- the full transposed convolution (out[2i + a] += x[i] w[a]) cropped by that many."""
    kh, kw = wt_tf.shape[:2]
    H, W = x.shape[2:]
    full = F.conv_transpose2d(x, wt_tf.permute(3, 2, 0, 1), stride=2)
    pbh, pbw = max(kh - 2, 0) // 2, max(kw - 2, 0) // 2
    out = full[:, :, pbh:pbh + 2 * H, pbw:pbw + 2 * W]
    return F.pad(out, (0, 2 * W - out.shape[3], 0, 2 * H - out.shape[2]))


def _bn64(x, T, p):
    g, b, mu, va = (T[p + ".bn." + t] for t in ("gamma", "beta", "mean", "var"))
    return (x - mu[None, :, None, None]) / torch.sqrt(va + BN_EPS)[None, :, None, None] * g[None, :, None, None] + b[None, :, None, None]


def forward64(hp, blob, x_nhwc, bn_hook=None):
    """Both graphs in inference mode, float64 end to end, on an NHWC batch -> probabilities [B, P, P, K] (numpy float64).
    v2 (UnMicst1-5.py / UnMicst2.py): block = conv + ks x ks shortcut, leaky(BN(.)), pool; bottom conv with BN; up = leaky(convT),
    concat [skip, up], leaky(BN(conv)); head 1 x 1 + BN + softmax.  legacy (UnMicst.py): 1 x 1 shortcut, BN(relu(.)) in the
    down blocks and no BatchNorm anywhere else.  Extra convolutions read the activated tensor before them.
    bn_hook(prefix, input NCHW, T), if given, runs before every BatchNorm in graph order and may rewrite that BatchNorm's entries of
    T (tests/trained_like.py sets moving statistics this way); `blob` may then also be the dict of float64 tensors itself."""
    v2 = hp.graph == model.GRAPH_V2
    T = blob if isinstance(blob, dict) else torch_tensors(hp, blob, torch.float64)
    act = (lambda t: torch.where(t >= 0, t, t * LEAK)) if v2 else (lambda t: t.clamp(min=0))
    L = hp.nLayers

    def bn(t, p):
        if bn_hook is not None:
            bn_hook(p, t, T)
        return _bn64(t, T, p)

    with torch.no_grad():
        x = torch.from_numpy(np.ascontiguousarray(x_nhwc, np.float64)).permute(0, 3, 1, 2)
        skips = [x]
        for i in range(L):
            n = "ld%d" % i
            c = _conv64(skips[i], T[n + ".w1"])
            for e in range(hp.nExtraConvs):
                c = _conv64(act(c), T["%s.wextra%d" % (n, e)])
            c = c + _conv64(skips[i], T[n + ".wshort"])
            c = act(bn(c, n)) if v2 else bn(act(c), n)
            skips.append(F.max_pool2d(c, 2))
        cur = _conv64(skips[L], T["lb.w"])
        cur = act(bn(cur, "lb")) if v2 else act(cur)
        for idx in range(L - 1, -1, -1):
            n = "lu%d" % idx
            up = act(_convT64(cur, T[n + ".wt"]))
            cur = _conv64(torch.cat([skips[idx], up], 1), T[n + ".w2"])
            cur = act(bn(cur, n)) if v2 else act(cur)
            for e in range(hp.nExtraConvs):
                cur = act(_conv64(cur, T["%s.wextra%d" % (n, e)]))
        t = _conv64(cur, T["lt.w"])
        if v2:
            t = bn(t, "lt")
        return torch.softmax(t, 1).permute(0, 2, 3, 1).contiguous().numpy()


# ------------------------------------------------------------------------------------------------ weights that make the deep path count
def deep_path_blob(hp, seed, damp=None):
    """model.random_blob with one change (damp None: none): in every lu*.w2 the filter slice that reads the skip tensor (the first
    half of the concatenated input channels: concat [skip, up]) is scaled by `damp`, the slice that reads the up-sampled tensor by
    sqrt(2).  With damp < 1 the output depends on the deep path, so a fault in lb or a low ld* / lu* layer is not diluted by the skips."""
    blob = model.random_blob(hp, seed=seed)
    if damp is None:
        return blob
    T = {k: np.array(v, dtype=np.float32) for k, v in model.tensors_from_blob(hp, blob).items()}
    n = hp.nOutX
    for idx in range(hp.nLayers):
        w2 = T["lu%d.w2" % idx]
        w2[:, :, :n[idx], :] *= np.float32(damp)
        w2[:, :, n[idx]:, :] *= np.float32(np.sqrt(2.0))
    return model.blob_from_tensors(hp, T)


# ------------------------------------------------------------------------------------------------ which launches take the F6 form
def f6_launches(hp):
    """The launches conv_f16x3's F6 form takes under precision f16f6 (the rule of choose_form in umx_plan.hip, restated): plain
    convolutions at <= 1/4 of the tile and >= 16 x 16 pixels whose output is nine N-tiles per workgroup in >= 2 N-blocks.
    The rule also asks for a tile of one image (here: >= 16 x 16 pixels) and no packed last N-tile (a single N-block only), and the
    planner's debug overrides are taken as unset.  tests/test_gpu_arith.py holds this set to the kernel names the engine's profile
    reports (eighth template argument of conv_f16x3), on every case."""
    L, nx, n = hp.nLayers, hp.nExtraConvs, hp.nOutX
    convs = []                                    # (launch name, size, output channels) of every plain convolution
    S = hp.imSize
    for i in range(L):
        for nm in (["conv1"] + ["extra%d" % e for e in range(nx)] if nx else ["conv"]):
            convs.append(("ld%d.%s" % (i, nm), S, n[i + 1]))
        S //= 2
    convs.append(("lb.conv", S, n[L + 1]))
    for idx in range(L - 1, -1, -1):
        S *= 2
        for nm in ["conv"] + ["extra%d" % e for e in range(nx)]:
            convs.append(("lu%d.%s" % (idx, nm), S, n[idx + 1]))
    out = set()
    for name, size, cout in convs:
        t16 = (cout + 15) // 16
        pads = {c: -(-t16 // c) * c for c in range(1, 10)}
        best = min(pads.values())
        nt16 = max(c for c, p in pads.items() if p == best)       # least padding, widest workgroup
        if nt16 == 9 and best // 9 >= 2 and size * 4 <= hp.imSize and size >= 16:
            out.add(name)
    return out


def f6_plan_of(hp):
    """plan_of for forward(): 'fp6x' on the launches of f6_launches(hp), 'f16x3' elsewhere."""
    per_layer = {}
    for name in f6_launches(hp):
        layer, part = name.split(".")
        per_layer.setdefault(layer, {})[part] = "fp6x"
    return lambda n: per_layer.get(n, "f16x3")


# ------------------------------------------------------------------------------------------------ the cases of the gate
HP_F6 = model.HParams(model.GRAPH_V2, 64, 2, 3, 72, 2, 3, 0)          # tests/test_gpu_f6.py: lb takes the F6 form
HP_SWITCHES = model.HParams(model.GRAPH_V2, 64, 2, 3, 28, 3, 3, 0, 2)  # tests/test_gpu_switches.py


def _d2s(n0, C, ks, S):
    return model.HParams(model.GRAPH_V2, S, C, 3, n0, 2, ks, 0, 2)


# name -> (hp, seed, damp, n_tiles).  seed: of the weights (deep_path_blob) and of the input tiles (case_inputs); n_tiles = 5 is meant to run
# through max_batch = 3 on the GPU: a ragged last batch, and a half-empty two-tile workgroup for the F6 form.
_S = helpers.small_hps()
ARITH_CASES = {
    "v2_duo_like": (_S["v2_duo_like"], 11, None, 5),
    "v2_wide": (_S["v2_wide"], 11, None, 5),
    "legacy_k5": (_S["legacy_k5"], 11, None, 5),
    "legacy_k3_x2": (_S["legacy_k3_x2"], 11, None, 5),
    "v2_extra": (_S["v2_extra"], 12, None, 5),                # (seed 11: tol 7.5e-7 < 1e-6)
    "v2_deep_damp": (_S["v2_deep"], 12, 1.0 / 16, 5),       # (plain random_blob: tol < 8 x E_ref; seed 11 with damp: tol 7.5e-7)
    "v2_72_f6": (HP_F6, 11, None, 5),
    "v2_72_f6_damp": (HP_F6, 12, 1.0 / 16, 5),
    "v2_28_switches": (HP_SWITCHES, 9, None, 5),
    "d2s_n22_c3": (_d2s(22, 3, 3, 32), 62, None, 5),      # D2S_SHAPES: two blocks of 6 with a two-phase remainder tile
    "d2s_n40_c1": (_d2s(40, 1, 3, 32), 80, None, 5),      # D2S_SHAPES: two blocks of 5, no remainder tile
    "v2_k5": (_d2s(12, 1, 5, 32), 52, None, 5),           # 5 x 5 filters on the v2 graph
    # the solo model's widths on half its tile: the kernel forms of model.KNOWN_HP that none of the above launches (dense-K first layer
    # of 5 N-tiles on one channel, fused-phase transposed convolution of 5 N-tiles, plain convolution of 8 N-tiles per workgroup;
    # exact fp32: 5 N-tiles on the 4 x 4-pixel layer) -- tests/test_gpu_arith.py checks that coverage
    "v2_solo_like": (model.HParams(model.GRAPH_V2, 32, 1, 3, 80, 3, 3, 0), 11, None, 5),
}


def case_inputs(name):
    hp, seed, damp, n = ARITH_CASES[name]
    blob = deep_path_blob(hp, seed, damp)
    x = np.random.default_rng(seed).normal(size=(n, hp.imSize, hp.imSize, hp.nChannels)).astype(np.float32)
    return hp, blob, x


def case_numbers(name, per_layer=None):
    """E_ref, E_drop, E_f6 (None where no launch takes the form), tol, tol_f6 of one case; per_layer (a dict) receives
    {fault plan: {layer: error}}."""
    from oracle import oracle
    hp, blob, x = case_inputs(name)
    p64 = forward64(hp, blob, x)

    def err(p):
        return float(np.abs(p.astype(np.float64) - p64).max())

    e_ref = max(err(oracle.forward(hp, blob, x)), err(emulate(hp, blob, x, lambda n: "f16x3")))
    e_drop = np.inf
    for fault in FAULT_PLANS:
        for layer in layer_names(hp):
            e = err(emulate(hp, blob, x, lambda n: fault if n == layer else "f16x3"))
            e_drop = min(e_drop, e)
            if per_layer is not None:
                per_layer.setdefault(fault, {})[layer] = e
    e_f6 = err(emulate(hp, blob, x, f6_plan_of(hp))) if f6_launches(hp) else None
    return {"E_ref": e_ref, "E_drop": e_drop, "E_f6": e_f6, "tol": e_drop / 4, "tol_f6": None if e_f6 is None else 4 * e_f6}


def case_conditions(c):
    """The conditions of the gate on one case's numbers -> list of the violated ones (empty: the case stands)."""
    bad = []
    if not c["tol"] == c["E_drop"] / 4:
        bad.append("tol != E_drop / 4")
    if not c["tol"] >= 8 * c["E_ref"]:
        bad.append("tol %.3g < 8 x E_ref %.3g: the correct arithmetic is not 8 x under the bound" % (c["tol"], c["E_ref"]))
    if not c["tol"] >= 1e-6:
        bad.append("tol %.3g < 1e-6: no room for the engine's fp32 accumulation order (4.2e-7 measured)" % c["tol"])
    if not c["tol"] <= 2e-5:
        bad.append("tol %.3g > 2e-5: not 5 x tighter than the 1e-4 gate" % c["tol"])
    if c["E_f6"] is not None:
        if not c["tol_f6"] == 4 * c["E_f6"]:
            bad.append("tol_f6 != 4 x E_f6")
        if not c["E_drop"] >= 2 * c["tol_f6"]:
            bad.append("E_drop %.3g < 2 x tol_f6 %.3g" % (c["E_drop"], c["tol_f6"]))
    return bad


def load_table():
    with open(TABLE) as f:
        return json.load(f)


def main(argv):
    torch.set_num_threads(max(1, min(16, (os.cpu_count() or 2) - 1)))
    names = [a for a in argv if not a.startswith("--")] or list(ARITH_CASES)
    table = {}
    for name in names:
        per_layer = {}
        c = case_numbers(name, per_layer)
        table[name] = c
        print("%-16s E_ref %.3g  E_drop %.3g  E_f6 %s  tol %.3g  tol_f6 %s  %s" % (
            name, c["E_ref"], c["E_drop"], "-" if c["E_f6"] is None else "%.3g" % c["E_f6"], c["tol"],
            "-" if c["tol_f6"] is None else "%.3g" % c["tol_f6"], "; ".join(case_conditions(c)) or "ok"), flush=True)
        for fault, row in per_layer.items():
            print("    %-10s" % fault + " ".join("%s %.2g" % kv for kv in row.items()), flush=True)
    if "--write" in argv:
        if names != list(ARITH_CASES):
            raise SystemExit("--write takes every case")
        with open(TABLE, "w") as f:
            json.dump(table, f, indent=1, sort_keys=True)
            f.write("\n")
        print("wrote", TABLE)


if __name__ == "__main__":
    main(sys.argv[1:])
