#!/usr/bin/env python3
"""The reference side of the inference arithmetic gate (checked by tests/test_inference_arith_cpu.py) -- CPU only.  The GPU side is
tests/test_gpu_arith.py: every precision of the engine held to `tol` / `tol_f6` of tests/arith_cases.json against forward64.

Four things live here:

* ``forward64``: a plain float64 forward of both graphs in inference mode, written from oracle/unet_oracle.c and the launch list of
  umx_describe_graph (moving-statistics BatchNorm, (Leaky)ReLU, max-pool, stride-2 transposed convolutions, concat order, the 1 x 1
  head, softmax).  It never touches the engine.
* the emulation of the engine's split-precision arithmetic (``split16``, the MX block quantisers, ``gemm``, ``conv_same``,
  ``conv_transpose_s2``, ``forward``), moved here from tests/fp8_cross_term_report.py, with two fault plans added to ``gemm``:
  ``f16x3-xlo`` (x_lo * w_hi omitted) and ``f16x3-wlo`` (x_hi * w_lo omitted).
* the fault cells (``cells``): either fault plan confined to one launch of a layer that has several, to the shortcut's K segment, to
  one output phase of a transposed convolution, or to one N-block of a launch -- the block boundaries from ``n_blocks``, the planner's
  rule restated here (this file never touches the engine; the CPU test holds the restatement to the host plan).
* ``ARITH_CASES`` and the table tests/arith_cases.json derived from them (``python tests/inference_ref.py --write``; ``--cells``
  prints every cell): per case
  E_ref  = max(max |oracle.forward - p64|, max |emulated f16x3 - p64|)      what two CPU restatements of the correct arithmetic give
  E_drop = min over layers and both fault plans of max |emulated - p64|     one product lost on ONE layer, the others on f16x3
  E_cell = min over cells and both fault plans of max |emulated - p64|      one product lost in ONE cell; worst_cell names it
           (and of 0.999 x D_w_lo = max |forward64(w_lo_cell's filter rounded to binary16 precision) - p64|: numbers_of)
  E_f6   = max |emulated - p64| with fp6x on the launches the planner gives the F6 form (cases that have one)
  tol    = min(E_drop, E_cell) / 4,  tol_f6 = 4 * E_f6
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
PHASES = ((0, 0), (0, 1), (1, 0), (1, 1))      # output phases (oy, ox) of a stride-2 transposed convolution


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


def gemm_cell(A, Wm, plan):
    """gemm under a plan that may be a fault cell (fault plan, "nblk", (c0, c1)): the output channels [c0, c1) -- one N-block of the
    launch -- come from the fault plan, all others from 'f16x3' (both on the whole filter: the weight shift is the launch's)."""
    if isinstance(plan, str):
        return gemm(A, Wm, plan)
    fault, kind, (c0, c1) = plan
    assert kind == "nblk" and fault in FAULT_PLANS and 0 <= c0 < c1 <= Wm.shape[1], plan
    out = gemm(A, Wm, "f16x3")
    out[:, c0:c1] = gemm(A, Wm, fault)[:, c0:c1]
    return out


def conv_same(x, w_tf, plan):
    """x NCHW fp32, w_tf [kh, kw, Cin, Cout]; K ordered (tap, channel) like the engine's (tap, octet) pairs.
    plan: a plan of gemm, or an N-block cell (gemm_cell)."""
    kh, kw, Ci, Co = w_tf.shape
    B, _, H, W = x.shape
    cols = F.unfold(x, (kh, kw), padding=(kh // 2, kw // 2))                 # [B, Ci*kh*kw, H*W], K order (channel, tap)
    cols = cols.reshape(B, Ci, kh * kw, H * W).permute(0, 3, 2, 1).reshape(B * H * W, kh * kw * Ci)
    out = gemm_cell(cols, w_tf.reshape(kh * kw * Ci, Co), plan)
    return out.reshape(B, H, W, Co).permute(0, 3, 1, 2)


def conv_transpose_s2(x, wt_tf, plan):
    """tf.nn.conv2d_transpose, stride 2, SAME (crop (k-2)//2 before): per output phase a GEMM over that phase's taps.
    plan: a plan of gemm, an N-block cell (gemm_cell: the same channels of every phase), or a phase cell (fault plan, "phase", (oy, ox)):
    the GEMM of output phase (oy, ox) runs the fault plan, the three others 'f16x3'."""
    kh, kw, Co, Ci = wt_tf.shape
    phase_cell = None
    if not isinstance(plan, str) and plan[1] == "phase":
        assert plan[0] in FAULT_PLANS and plan[2] in PHASES, plan
        phase_cell, plan = plan, "f16x3"
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
            p = phase_cell[0] if phase_cell is not None and phase_cell[2] == (oy, ox) else plan
            o = gemm_cell(A, torch.cat(ws, 0), p).reshape(B, H, W, Co).permute(0, 3, 1, 2)
            out[:, :, oy::2, ox::2] = o
    return out


def bn(x, T, p):
    g, b, mu, va = (T[p + ".bn." + t] for t in ("gamma", "beta", "mean", "var"))
    s = g / torch.sqrt(va + BN_EPS)
    return x * s[None, :, None, None] + (b - mu * s)[None, :, None, None]


def forward(hp, T, x_nhwc, plan_of):
    """plan_of(layer name) -> plan; graph order follows oracle/unet_oracle.c (reference UnMicst1-5.py:83-237 / UnMicst.py:51-187).
    plan_of may also return {launch suffix: plan} for a layer whose launches differ (the engine's names: "conv" / "conv1" /
    "extraN" / "convT" / "head"; a shortcut belongs to the launch that adds it, unless the dict names "short": then the shortcut's
    product alone takes that plan -- a cell only where the engine keeps the shortcut a K segment of its own, which is with extra
    convolutions); suffixes it leaves out run 'f16x3'.  A launch's plan may be a fault cell (conv_same, conv_transpose_s2)."""
    v2 = hp.graph == model.GRAPH_V2
    act = (lambda t: F.leaky_relu(t, LEAK)) if v2 else F.relu
    L = hp.nLayers
    nx = hp.nExtraConvs

    def pl(n, part, own=None):
        p = plan_of(n)
        if not isinstance(p, dict):
            return p
        return p[own] if own in p else p.get(part, "f16x3")

    x = x_nhwc.permute(0, 3, 1, 2)
    ds = [x]
    for i in range(L):
        n = "ld%d" % i
        c = conv_same(ds[i], T[n + ".w1"], pl(n, "conv1" if nx else "conv"))
        for e in range(nx):
            c = conv_same(act(c), T["%s.wextra%d" % (n, e)], pl(n, "extra%d" % e))
        c = c + conv_same(ds[i], T[n + ".wshort"], pl(n, "extra%d" % (nx - 1) if nx else "conv", "short" if nx else None))
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
def deep_path_blob(hp, seed, damp=None, phase_eq=None):
    """model.random_blob with two changes (each None: not made).
    damp: in every lu*.w2 the filter slice that reads the skip tensor (the first half of the concatenated input channels: concat
    [skip, up]) is scaled by `damp`, the slice that reads the up-sampled tensor by sqrt(2).  With damp < 1 the output depends on the
    deep path, so a fault in lb or a low ld* / lu* layer is not diluted by the skips.
    phase_eq: in every lu*.wt the taps of an output phase that has t of them are scaled by (t_max / t) ** (phase_eq / 2), t_max the
    taps of the fullest phase (3 x 3: the centre tap, alone in phase (1, 1), by 4 ** (phase_eq / 2), the two-tap phases by
    2 ** (phase_eq / 2)).  A random filter gives a phase signal in proportion to its taps, so a product lost in the one-tap phase is the
    cheapest fault of the graph; with phase_eq = 1 every phase carries the variance of the fullest one."""
    blob = model.random_blob(hp, seed=seed)
    if damp is None and phase_eq is None:
        return blob
    T = {k: np.array(v, dtype=np.float32) for k, v in model.tensors_from_blob(hp, blob).items()}
    n = hp.nOutX
    for idx in range(hp.nLayers):
        if damp is not None:
            w2 = T["lu%d.w2" % idx]
            w2[:, :, :n[idx], :] *= np.float32(damp)
            w2[:, :, n[idx]:, :] *= np.float32(np.sqrt(2.0))
        if phase_eq is not None:
            wt = T["lu%d.wt" % idx]
            taps = {ph: phase_taps(wt.shape[0], ph) for ph in PHASES}
            tmax = max(len(t) for t in taps.values())
            for t in taps.values():
                for a, b in t:
                    wt[a, b] *= np.float32((tmax / len(t)) ** (phase_eq / 2.0))
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


# ------------------------------------------------------------------------------------------------ N-blocks and fault cells
def n_blocks(hp):
    """{launch name: (NT, number of N-blocks)} of every convolution launch: the N-tiles of 16 output channels a workgroup computes and
    the blocks of 16 * NT channels the launch's N axis is cut into (choose_form and make_d2s in umx_plan.hip, restated): the NT of
    1 ... 9 that pads the ceil(Cout / 16) N-tiles least, the widest of those.  A stride-2 transposed convolution of F = Cout // 8
    octets and R = Cout % 8 <= 4 left-over channels takes the depth-to-space form where the four phases (2 F + (R > 0) N-tiles) or the
    two phases of an output row (F + (R > 0)) make 5 ... 9 N-tiles: then its N axis is [phase][channel] in ONE block, and its cells are
    its phases.  Otherwise, with <= 5 N-tiles on >= 8 x 16 input pixels it runs the four phases fused in one workgroup (NT <= 5).
    Taken as not happening: the planner's overrides, the narrower NT a per-phase transposed convolution of tiny images may get from
    the LDS search (the same padded width, so only the block boundaries would move), and a raw-skip fold that keeps a layer off the
    depth-to-space form.  tests/test_inference_arith_cpu.py holds every entry to the engine's host plan on every case."""
    L, nx, n = hp.nLayers, hp.nExtraConvs, hp.nOutX

    def rule(cout, cmax=9):
        t16 = (cout + 15) // 16
        pads = {c: -(-t16 // c) * c for c in range(1, cmax + 1)}
        best = min(pads.values())
        nt = max(c for c, p in pads.items() if p == best)
        return nt, best // nt

    out = {}
    S = hp.imSize
    for i in range(L):
        for nm in (["conv1"] + ["extra%d" % e for e in range(nx)] if nx else ["conv"]):
            out["ld%d.%s" % (i, nm)] = rule(n[i + 1])
        S //= 2
    out["lb.conv"] = rule(n[L + 1])
    for idx in range(L - 1, -1, -1):
        cout = n[idx + 1]
        Fo, R = cout // 8, cout % 8
        rem = 1 if R else 0
        if Fo >= 1 and R <= 4 and S >= 2 and (5 <= 2 * Fo + rem <= 9 or 5 <= Fo + rem <= 9):
            out["lu%d.convT" % idx] = (2 * Fo + rem if 5 <= 2 * Fo + rem <= 9 else Fo + rem, 1)
        else:
            out["lu%d.convT" % idx] = rule(cout, 5 if (cout + 15) // 16 <= 5 and S >= 16 else 9)
        S *= 2
        for nm in ["conv"] + ["extra%d" % e for e in range(nx)]:
            out["lu%d.%s" % (idx, nm)] = rule(cout)
    return out


def launch_couts(hp):
    """{launch name: output channels} of the launches of n_blocks(hp)."""
    n = hp.nOutX
    return {name: n[hp.nLayers + 1] if name.startswith("lb") else n[int(name[2:name.index(".")]) + 1] for name in n_blocks(hp)}


def phase_taps(ks, phase):
    """The taps (a, b) of a ks x ks stride-2 transposed filter that output phase (oy, ox) uses (conv_transpose_s2's rule)."""
    pb = max(ks - 2, 0) // 2
    return [(a, b) for a in range(ks) if (phase[0] + pb - a) % 2 == 0 for b in range(ks) if (phase[1] + pb - b) % 2 == 0]


def cells(hp):
    """The fault cells of a graph, finer than a layer: [(cell name, layer, fault plan -> what plan_of returns for that layer)].
    * "<launch>": the launch alone, where its layer has several (the last extra convolution of a down block with its shortcut);
    * "ld<i>.short": the shortcut's product alone -- only with extra convolutions: there the engine runs the shortcut as a second K
      segment of the last extra convolution's launch (umx_graph.hip: add_conv_group(Le, ds[i], wsc, ...)).  Without them the shortcut
      filter is summed into the convolution's at plan time (summed_shortcut) and there is no such cell;
    * "<launch>@p<oy><ox>": one output phase of a transposed convolution, on the mathematics, whichever kernel form runs it;
    * "<launch>@n<c0>:<c1>": one N-block of a launch that has >= 2 (n_blocks), output channels [c0, c1)."""
    nx = hp.nExtraConvs
    out = []
    couts = launch_couts(hp)
    for name, (nt, nb) in n_blocks(hp).items():
        layer, part = name.split(".")
        several = layer.startswith("lu") or (layer.startswith("ld") and nx > 0)
        if several:
            out.append((name, layer, lambda f, part=part: {part: f}))
        if layer.startswith("ld") and nx and part == "extra%d" % (nx - 1):
            out.append((layer + ".short", layer, lambda f: {"short": f}))
        if part == "convT":
            for ph in PHASES:
                out.append(("%s@p%d%d" % (name, ph[0], ph[1]), layer, lambda f, ph=ph: {"convT": (f, "phase", ph)}))
        if nb >= 2:
            for b in range(nb):
                c0, c1 = b * 16 * nt, min((b + 1) * 16 * nt, couts[name])
                out.append(("%s@n%d:%d" % (name, c0, c1), layer, lambda f, part=part, c=(c0, c1): {part: (f, "nblk", c)}))
    return out


def round11(w):
    """Round to an 11-bit significand (binary16's precision at any exponent), half to even: invariant under a power-of-two scale, so
    the lo half of the planner's binary16 split of such a weight is exactly 0."""
    m, e = np.frexp(np.asarray(w, np.float64))
    return np.ldexp(np.round(m * 2048.0) / 2048.0, e).astype(np.float32)


def cell_filter_view(hp, T, cell):
    """The entries of the filter (in T, model.tensors_from_blob's dict of arrays) that a phase or N-block cell of lb.conv / lu*.convT /
    lu*.conv multiplies -> (tensor key, index): T[key][index] is a view of exactly those entries."""
    launch, sel = cell.split("@")
    layer, part = launch.split(".")
    key = layer + {"convT": ".wt", "conv": ".w" if layer == "lb" else ".w2"}[part]
    if sel[0] == "p":
        assert part == "convT"
        taps = phase_taps(T[key].shape[0], (int(sel[1]), int(sel[2])))
        a, b = sorted({t[0] for t in taps}), sorted({t[1] for t in taps})
        return key, np.ix_(a, b)
    c0, c1 = (int(v) for v in sel[1:].split(":"))
    return key, (slice(None), slice(None), slice(c0, c1)) if part == "convT" else (Ellipsis, slice(c0, c1))


def blob_with_cell_rounded(hp, blob, cell):
    """`blob` with the filter entries of one cell rounded to binary16 precision (round11): the engine's w_lo is 0 there."""
    T = {k: np.array(v, dtype=np.float32) for k, v in model.tensors_from_blob(hp, blob).items()}
    key, idx = cell_filter_view(hp, T, cell)
    T[key][idx] = round11(T[key][idx])
    return model.blob_from_tensors(hp, T)


def qualifies_for_w_lo_test(cell):
    """A phase or an N-block of a launch whose filter the engine splits as stored (lb.conv, lu*.convT, lu*.conv) -- not a launch
    alone, not a down block's convolution (its filter is summed with the shortcut's at plan time, or it is not a stored split)."""
    launch = cell.split("@")[0]
    return "@" in cell and (launch == "lb.conv" or (launch.startswith("lu") and launch.split(".")[1] in ("convT", "conv")))


# ------------------------------------------------------------------------------------------------ the cases of the gate
HP_F6 = model.HParams(model.GRAPH_V2, 64, 2, 3, 72, 2, 3, 0)          # tests/test_gpu_f6.py: lb takes the F6 form
HP_F6_HALF = model.HParams(model.GRAPH_V2, 32, 2, 3, 72, 2, 3, 0)      # the same launches and cells; lb at 8 x 8 pixels: no F6 form
HP_SWITCHES = model.HParams(model.GRAPH_V2, 64, 2, 3, 28, 3, 3, 0, 2)  # tests/test_gpu_switches.py


def _d2s(n0, C, ks, S):
    return model.HParams(model.GRAPH_V2, S, C, 3, n0, 2, ks, 0, 2)


# name -> (hp, seed, damp, n_tiles, phase_eq).  seed: of the weights (deep_path_blob) and of the input tiles (case_inputs); damp, phase_eq:
# deep_path_blob's knobs; n_tiles = 5 is meant to run through max_batch = 3 on the GPU: a ragged last batch, and a half-empty two-tile
# workgroup for the F6 form.  Seeds and knobs were chosen on case_conditions alone -- on the numbers this file computes -- and so that no
# case's tol is above what it was while only whole layers were faulted (in brackets: what the first choice gave once cells were swept).
_S = helpers.small_hps()
ARITH_CASES = {
    "v2_duo_like": (_S["v2_duo_like"], 12, None, 5, 1),        # (seed 11, no phase_eq: tol 1.04e-6 < 8 x E_ref; seed 11 with it: tol above the former)
    "v2_wide": (_S["v2_wide"], 11, None, 5, None),
    "legacy_k5": (_S["legacy_k5"], 11, 0.25, 5, 1),             # (no knob: tol 7.5e-7 < 1e-6, lu1.convT's phases; phase_eq alone: 8.5e-7)
    "legacy_k3_x2": (_S["legacy_k3_x2"], 11, None, 5, None),
    "v2_extra": (_S["v2_extra"], 12, None, 5, None),                # (seed 11: tol 7.5e-7 < 1e-6)
    "v2_deep_damp": (_S["v2_deep"], 12, 1.0 / 16, 5, None),       # (plain random_blob: tol < 8 x E_ref; seed 11 with damp: tol 7.5e-7)
    "v2_72_f6": (HP_F6, 11, None, 5, None),
    "v2_72_f6_damp": (HP_F6, 12, 1.0 / 16, 5, None),
    "v2_28_switches": (HP_SWITCHES, 9, None, 5, None),
    "d2s_n22_c3": (_d2s(22, 3, 3, 32), 62, None, 5, None),      # D2S_SHAPES: two blocks of 6 with a two-phase remainder tile
    "d2s_n40_c1": (_d2s(40, 1, 3, 32), 80, None, 5, None),      # D2S_SHAPES: two blocks of 5, no remainder tile
    "v2_k5": (_d2s(12, 1, 5, 32), 52, None, 5, None),           # 5 x 5 filters on the v2 graph
    # the solo model's widths on half its tile: the kernel forms of model.KNOWN_HP that none of the above launches (dense-K first layer
    # of 5 N-tiles on one channel, fused-phase transposed convolution of 5 N-tiles, plain convolution of 8 N-tiles per workgroup;
    # exact fp32: 5 N-tiles on the 4 x 4-pixel layer) -- tests/test_gpu_arith.py checks that coverage
    # (seed 11, no phase_eq: tol 1.01e-6, 0.7 % over 1e-6 -- inside the 2 % the table reproduces to; seed 11 with it: tol above the former)
    "v2_solo_like": (model.HParams(model.GRAPH_V2, 32, 1, 3, 80, 3, 3, 0), 12, None, 5, 1),
    # the companion of the two F6 cases (HELD_ELSEWHERE): their widths on half their tile, where lb is 8 x 8 pixels and takes no F6 form
    "v2_72_phase": (HP_F6_HALF, 11, None, 5, None),
}

# Cells a case leaves to a companion: {case: (companion, what the names of those cells contain)}.  A case's E_cell is taken over the cells
# it keeps; every cell it leaves out must stand at >= 4 x tol in the companion (tests/test_inference_arith_cpu.py).
# The two F6 cases: one phase of a transposed convolution is a quarter of the launch behind the F6 layer, and a product lost there costs
# 6 - 8 x E_f6 whatever the seed, damp or phase_eq (1.0 ... 2.0 x tol_f6 on seeds 11 - 14, damp 1/16 and 1/4, phase_eq 1 ... 2),
# where min(E_drop, E_cell) >= 2 x tol_f6 = 8 x E_f6 is required.  The same widths without an F6 launch are not bound by tol_f6.
HELD_ELSEWHERE = {"v2_72_f6": ("v2_72_phase", "convT@p"), "v2_72_f6_damp": ("v2_72_phase", "convT@p")}


def kept(name, cell):
    """Whether the case's own tol is taken over this cell (else its companion holds it)."""
    return name not in HELD_ELSEWHERE or HELD_ELSEWHERE[name][1] not in cell


def case_inputs(name):
    hp, seed, damp, n, phase_eq = ARITH_CASES[name]
    blob = deep_path_blob(hp, seed, damp, phase_eq)
    x = np.random.default_rng(seed).normal(size=(n, hp.imSize, hp.imSize, hp.nChannels)).astype(np.float32)
    return hp, blob, x


def case_numbers(name, per_layer=None, per_cell=None, only_cells=None):
    """numbers_of on the inputs of a case, E_cell over the cells the case keeps."""
    return numbers_of(*case_inputs(name), per_layer=per_layer, per_cell=per_cell, only_cells=only_cells, keep=lambda cell: kept(name, cell))


def numbers_of(hp, blob, x, per_layer=None, per_cell=None, only_cells=None, keep=lambda cell: True):
    """E_ref, E_drop, E_cell, worst_cell ("<cell> xlo" / "<cell> wlo": the cell and the product lost), w_lo_cell (worst_cell's cell if
    it qualifies_for_w_lo_test, else the weakest cell that does: what tests/test_gpu_arith.py rounds the filter of), D_w_lo, E_f6 (None where
    no launch takes the form), tol, tol_f6 of one case; per_layer (a dict) receives {fault plan: {layer: error}}, per_cell (a dict)
    {cell name: {fault plan: error}}.  only_cells: the cell names to emulate (None: all of cells(hp)); E_cell, worst_cell and
    w_lo_cell are then taken over those alone -- and over the cells keep(cell name) accepts only (the others are emulated for per_cell)."""
    from oracle import oracle
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
    e_cell, worst, e_q, w_lo_cell = np.inf, None, np.inf, None
    for cell, layer, plan in cells(hp):
        if only_cells is not None and cell not in only_cells:
            continue
        for fault in FAULT_PLANS:
            e = err(emulate(hp, blob, x, lambda n: plan(fault) if n == layer else "f16x3"))
            if e < e_cell and keep(cell):
                e_cell, worst = e, "%s %s" % (cell, fault[-3:])
            if e < e_q and keep(cell) and qualifies_for_w_lo_test(cell):
                e_q, w_lo_cell = e, cell
            if per_cell is not None:
                per_cell.setdefault(cell, {})[fault] = e
    # the w_lo product of w_lo_cell has a second reference-side measure, with no emulation in it: D_w_lo, what the float64 forward
    # itself moves by when that cell's filter loses its lo halves.  It is x * w_lo where the fault plan omits x_hi * w_lo, and it carries
    # none of the emulation's own rounding (E_ref), so the two differ by a per cent or so either way; E_cell takes the smaller (D_w_lo less
    # 0.1 % for the float64 summation order of another machine), so that D_w_lo >= 4 x tol holds wherever the table is recomputed.
    d_w_lo = None
    if w_lo_cell is not None:
        d_w_lo = float(np.abs(forward64(hp, blob_with_cell_rounded(hp, blob, w_lo_cell), x) - p64).max())
        if 0.999 * d_w_lo < e_cell:
            e_cell, worst = 0.999 * d_w_lo, w_lo_cell + " wlo"
    e_f6 = err(emulate(hp, blob, x, f6_plan_of(hp))) if f6_launches(hp) else None
    return {"E_ref": e_ref, "E_drop": e_drop, "E_cell": e_cell, "worst_cell": worst, "w_lo_cell": w_lo_cell, "D_w_lo": d_w_lo, "E_f6": e_f6,
            "tol": min(e_drop, e_cell) / 4, "tol_f6": None if e_f6 is None else 4 * e_f6}


def w_lo_sensitivity(name, cell):
    """(blob B' = the case's blob with `cell`'s filter entries rounded to binary16 precision, D = max |forward64(B') - forward64(B)|
    over the case's tiles): what the exact function moves by when that cell's w_lo is taken away."""
    hp, blob, x = case_inputs(name)
    blob2 = blob_with_cell_rounded(hp, blob, cell)
    return blob2, float(np.abs(forward64(hp, blob2, x) - forward64(hp, blob, x)).max())


def case_conditions(c):
    """The conditions of the gate on one case's numbers -> list of the violated ones (empty: the case stands)."""
    bad = []
    e_min = min(c["E_drop"], c["E_cell"])           # the cheapest single lost product: on a whole layer, or on one cell of a launch
    if not c["tol"] == e_min / 4:
        bad.append("tol != min(E_drop, E_cell) / 4")
    if not c["tol"] >= 8 * c["E_ref"]:
        bad.append("tol %.3g < 8 x E_ref %.3g: the correct arithmetic is not 8 x under the bound" % (c["tol"], c["E_ref"]))
    if not c["tol"] >= 1e-6:
        bad.append("tol %.3g < 1e-6: no room for the engine's fp32 accumulation order (4.2e-7 measured)" % c["tol"])
    if not c["tol"] <= 2e-5:
        bad.append("tol %.3g > 2e-5: not 5 x tighter than the 1e-4 gate" % c["tol"])
    if c["E_f6"] is not None:
        if not c["tol_f6"] == 4 * c["E_f6"]:
            bad.append("tol_f6 != 4 x E_f6")
        if not e_min >= 2 * c["tol_f6"]:
            bad.append("min(E_drop, E_cell) %.3g < 2 x tol_f6 %.3g" % (e_min, c["tol_f6"]))
    return bad


def load_table():
    with open(TABLE) as f:
        return json.load(f)


def main(argv):
    torch.set_num_threads(max(1, min(16, (os.cpu_count() or 2) - 1)))
    names = [a for a in argv if not a.startswith("--")] or list(ARITH_CASES)
    table = {}
    for name in names:
        per_layer, per_cell = {}, {}
        c = case_numbers(name, per_layer, per_cell)
        table[name] = c
        print("%-16s E_ref %.3g  E_drop %.3g  E_cell %.3g (%s)  E_f6 %s  tol %.3g  tol_f6 %s  w_lo cell %s  %s" % (
            name, c["E_ref"], c["E_drop"], c["E_cell"], c["worst_cell"], "-" if c["E_f6"] is None else "%.3g" % c["E_f6"], c["tol"],
            "-" if c["tol_f6"] is None else "%.3g" % c["tol_f6"], c["w_lo_cell"], "; ".join(case_conditions(c)) or "ok"), flush=True)
        for fault, row in per_layer.items():
            print("    %-10s" % fault + " ".join("%s %.2g" % kv for kv in row.items()), flush=True)
        if "--cells" in argv:
            for cell, row in sorted(per_cell.items(), key=lambda kv: min(kv[1].values())):
                print("    %-22s" % cell + " ".join("%s %.3g = %.1f x tol" % (f[-3:], e, e / c["tol"]) for f, e in row.items()), flush=True)
    if "--write" in argv:
        if names != list(ARITH_CASES):
            raise SystemExit("--write takes every case")
        with open(TABLE, "w") as f:
            json.dump(table, f, indent=1, sort_keys=True)
            f.write("\n")
        print("wrote", TABLE)


if __name__ == "__main__":
    main(sys.argv[1:])
