"""Float64 autograd restatement of one training step of the LEGACY graph -- the yardstick of tests/test_gpu_train_legacy.py.

The graph is reference UnMicst.py:80-186, the loss and optimiser :270-279 (train() with restoreVariables, :330-331):
  down i   c = conv(x, w1); c = conv(relu(c), wextra_e) per extra conv; z = c + conv1x1(x, wshort);
           y = BN(relu(z)) with batch statistics (training) or the moving ones; ds_{i+1} = maxpool2(y)
  bottom   relu(conv(ds_L, lb.w))                          (no BN)
  up idx   us = relu(convT_s2(x, wt)); cv = relu(conv([ds_idx, us], w2)); cv = relu(conv(cv, wextra_e)) per extra conv
  top      softmax(conv1x1(cv, lt.w))                      (no BN)
  loss     mean_{b,y,x}(-sum_k labels * log p)             (no weights, no clip, no regulariser; `weights` multiplies in)
  update   MomentumOptimizer(0.01 * 0.95^floor(step / 1000), 0.9); BN moving averages with momentum 0.99 every step
BN epsilon 1e-3 (tests/golden/meta_graph_nucleiDAPI.json).  oracle/ is frozen: this file only imports its convolution helpers.

`decisions` (as oracle/train_oracle.forward's): {site: 0/1 mask shaped like the tensor in front of that ReLU, "pool<i>": window
element 2 dy + dx} -- the branches another evaluation of the same step (the HIP kernels') took, so both differentiate the same
smooth piece of the loss.  ReLU sites are named after the trainer's tensors (umx_trainer_read_tensor): "ld<i>.x<e>", "ld<i>.z",
"lb.z", "lu<i>.us", "lu<i>.x<e>", "lu<i>.z"."""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np
import torch

from oracle.train_oracle import _conv_same, _conv_transpose_s2
from unmicst_amd import model

BN_EPS = 1e-3


@dataclass
class LegacyOptions:
    """The constants of UnMicst.py:270-279 plus the BN moving-average momentum of tf.layers.batch_normalization."""
    lr0: float = 0.01
    decay_steps: int = 1000
    decay_rate: float = 0.95
    momentum: float = 0.9
    bn_momentum: float = 0.99


def split_blob(hp, blob):
    return {k: np.array(v, dtype=np.float64) for k, v in model.tensors_from_blob(hp, np.asarray(blob, np.float64)).items()}


def join_blob(hp, tensors):
    return np.concatenate([np.asarray(tensors[n], np.float64).ravel() for n, _ in model.tensor_specs(hp)])


def trainable(name: str) -> bool:
    return not (name.endswith(".bn.mean") or name.endswith(".bn.var"))


def _relu(a, site, decisions, trace):
    if trace is not None:
        trace[site] = a.detach()
    if decisions is not None and site in decisions:
        return a * decisions[site]
    return torch.relu(a)


def _pool(a, site, decisions, trace):
    if trace is not None:
        trace[site] = a.detach()
    B, C, H, W = a.shape
    win = a.reshape(B, C, H // 2, 2, W // 2, 2).permute(0, 1, 2, 4, 3, 5).reshape(B, C, H // 2, W // 2, 4)
    if decisions is not None and site in decisions:
        return torch.gather(win, 4, decisions[site].unsqueeze(-1)).squeeze(-1)
    return win.max(-1).values


def _bn(x, P, prefix, training, stats):
    g, b = P[prefix + ".bn.gamma"], P[prefix + ".bn.beta"]
    if training:
        mean = x.mean(dim=(0, 2, 3))
        var = x.var(dim=(0, 2, 3), unbiased=False)
        stats[prefix] = (mean.detach(), var.detach(), x.numel() // x.shape[1])
    else:
        mean, var = P[prefix + ".bn.mean"], P[prefix + ".bn.var"]
    xh = (x - mean[None, :, None, None]) * torch.rsqrt(var[None, :, None, None] + BN_EPS)
    return xh * g[None, :, None, None] + b[None, :, None, None]


def forward(hp, P, data_nhwc, training, decisions=None, trace=None):
    """-> (softmax probabilities NHWC, {"ld<i>": (batch mean, batch variance, count) of relu(z)})."""
    L, E = hp.nLayers, hp.nExtraConvs
    stats = {}
    ds = [data_nhwc.permute(0, 3, 1, 2)]
    for i in range(L):
        x = ds[i]
        c = _conv_same(x, P["ld%d.w1" % i])
        for e in range(E):
            c = _conv_same(_relu(c, "ld%d.x%d" % (i, e), decisions, trace), P["ld%d.wextra%d" % (i, e)])
        z = c + _conv_same(x, P["ld%d.wshort" % i])
        y = _bn(_relu(z, "ld%d.z" % i, decisions, trace), P, "ld%d" % i, training, stats)
        ds.append(_pool(y, "pool%d" % i, decisions, trace))
    cur = _relu(_conv_same(ds[L], P["lb.w"]), "lb.z", decisions, trace)
    for idx in range(L - 1, -1, -1):
        us = _relu(_conv_transpose_s2(cur, P["lu%d.wt" % idx]), "lu%d.us" % idx, decisions, trace)
        c = _conv_same(torch.cat([ds[idx], us], dim=1), P["lu%d.w2" % idx])
        for e in range(E):
            c = _conv_same(_relu(c, "lu%d.x%d" % (idx, e), decisions, trace), P["lu%d.wextra%d" % (idx, e)])
        cur = _relu(c, "lu%d.z" % idx, decisions, trace)
    t = _conv_same(cur, P["lt.w"])
    return torch.softmax(t, dim=1).permute(0, 2, 3, 1), stats


def loss_and_grads(hp, blob, data, labels, weights=None, decisions=None, trace=None):
    """-> (loss, gradient as a blob-shaped float64 vector (0 on the moving statistics), probabilities, batch statistics)."""
    T = split_blob(hp, blob)
    P = {k: torch.tensor(v, requires_grad=trainable(k)) for k, v in T.items()}
    d = torch.tensor(np.asarray(data, np.float64))
    y = torch.tensor(np.asarray(labels, np.float64))
    probs, stats = forward(hp, P, d, True, decisions, trace)
    wy = y if weights is None else y * torch.tensor(np.asarray(weights, np.float64))
    loss = (-(wy * torch.log(probs)).sum(dim=3)).mean()
    loss.backward()
    g = {k: (P[k].grad.numpy() if trainable(k) and P[k].grad is not None else np.zeros(T[k].shape)) for k in T}
    return loss.item(), join_blob(hp, g), probs.detach().numpy(), {k: (m.numpy(), v.numpy(), n) for k, (m, v, n) in stats.items()}


def learning_rate(o: LegacyOptions, step: int) -> float:
    return o.lr0 * o.decay_rate ** (step // o.decay_steps)   # tf.train.exponential_decay(staircase=True)


@dataclass
class TrainState:
    blob: np.ndarray
    m: np.ndarray = None
    step: int = 0
    last: dict = field(default_factory=dict)

    def __post_init__(self):
        self.blob = np.asarray(self.blob, np.float64).copy()
        if self.m is None:
            self.m = np.zeros_like(self.blob)


def train_step(hp, st: TrainState, data, labels, o: LegacyOptions, weights=None, decisions=None) -> float:
    """One optimOp in place: Momentum on every trainable variable (accum = mom accum + g; w -= lr accum), then the BN moving
    averages (UPDATE_OPS; the unbiased batch variance feeds the moving variance, as TF's fused kernel)."""
    loss, g, probs, stats = loss_and_grads(hp, st.blob, data, labels, weights, decisions)
    lr = learning_rate(o, st.step)
    mask = np.concatenate([np.full(int(np.prod(s)), 1.0 if trainable(n) else 0.0) for n, s in model.tensor_specs(hp)])
    st.m = o.momentum * st.m + g
    st.blob = st.blob - mask * lr * st.m
    T = split_blob(hp, st.blob)
    for prefix, (mean, var, n) in stats.items():
        T[prefix + ".bn.mean"] = T[prefix + ".bn.mean"] * o.bn_momentum + mean * (1.0 - o.bn_momentum)
        T[prefix + ".bn.var"] = T[prefix + ".bn.var"] * o.bn_momentum + var * (n / max(n - 1.0, 1.0)) * (1.0 - o.bn_momentum)
    st.blob = join_blob(hp, T)
    st.step += 1
    st.last = {"loss": loss, "grads": g, "probs": probs, "stats": stats, "lr": lr}
    return loss


def inference_probs(hp, blob, data) -> np.ndarray:
    """tfTraining: 0 -- moving statistics (tied to oracle.forward by tests/test_legacy_train_ref_cpu.py)."""
    P = {k: torch.tensor(v) for k, v in split_blob(hp, blob).items()}
    with torch.no_grad():
        return forward(hp, P, torch.tensor(np.asarray(data, np.float64)), False)[0].numpy()
