"""What the GPU tests of the training set's assembly share (tests/test_gpu_trainset*.py): a random set whose gains clip, the descriptor
arrays from plain rows, the bit-for-bit comparison and a trainer's state as bytes."""
import numpy as np

from unmicst_amd import trainer

MEAN, STD = 0.2, 0.15


def _random_set(hp, N, pages, S, seed):
    """Normalised planes whose im2double values lie in 0..1, so that gains of 1.5 and 4 clip some pixels and leave others; codes 0 and
    > K included; sample 1 has no weight map (a missing map counts as 0)."""
    rng = np.random.default_rng(seed)
    raw = rng.random((N, hp.nChannels, pages, S, S)) ** 2
    planes = ((raw - MEAN) / STD).astype(np.float32)
    ann = rng.integers(0, hp.nClasses + 2, (N, S, S)).astype(np.uint8)
    wmaps = [rng.random((S, S)).astype(np.float32) * 2 for _ in range(N)]
    wmaps[1] = None
    return planes, ann, wmaps


def _descs(rows):
    d = np.zeros(len(rows), trainer.SAMPLE_DESC)
    for j, r in enumerate(rows):
        d[j] = tuple(r) + (0,)
    return d


def _augs(rows):
    a = np.zeros(len(rows), trainer.AUGMENT_DESC)
    for j, r in enumerate(rows):
        a[j] = tuple(r)
    return a


def _warps(ms):
    w = np.zeros(len(ms), trainer.WARP_DESC)
    for j, m in enumerate(ms):
        w["m"][j] = m
    return w


def _elastics(lats):
    """lats: per image None (n = 0) or (n, d [2][6][6])."""
    e = np.zeros(len(lats), trainer.ELASTIC_DESC)
    for j, l in enumerate(lats):
        if l is not None:
            e["n"][j], e["d"][j] = l
    return e


def _same_bits(got, want, what, rows=slice(None)):
    for k, (g, w) in enumerate(zip(got, want)):
        if w is None:
            assert g is None, what
            continue
        g, w = g[rows], w[rows]
        assert g.dtype == np.float32 and g.shape == w.shape, (what, k)
        ne = g.view(np.uint32) != w.view(np.uint32)
        assert not ne.any(), (what, ("data", "labels", "weights")[k], int(ne.sum()), np.argwhere(ne)[:4].tolist())


def _state(tr):
    m, v = tr.slots()
    return tr.blob().tobytes(), m.tobytes(), v.tobytes()
