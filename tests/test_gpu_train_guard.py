"""GPU tests of the training kernels' memory discipline, in the trainer's debug guard mode (UMX_DEBUG_GUARD, include/umx_train.h).

Every device buffer of a trainer / training set then sits between two red zones filled with one byte, and so does the content of every
buffer the library neither zeroes nor uploads.  Two properties are checked on the same runs:
  no stray writes  every public call checks every zone and fails with UMX_ERR_GUARD (naming the buffer) if one changed;
  no stray reads   the same case under the fills 0x00, 0xFF (a NaN that propagates through products) and 0x7F (a huge finite value
                   that max-reductions and fmaxf cannot drop) gives bit-identical losses, gradients, parameters, probabilities and
                   decision-site tensors -- and the same bits as a run without guards.  Reduction orders are fixed, so this is exact.
Shapes: the small v2 / legacy hyper-parameters of the numerics tests plus odd ones (batch 1, 3 channels, odd widths, a 2x2
bottom, 5x5 filters on 4x4 layers, a 128-pixel image), every convolution route, and one full-size run per graph."""
import numpy as np
import pytest

import helpers
from unmicst_amd import model, trainer, trainset, umx

pytestmark = pytest.mark.gpu

FILLS = ("0x00", "0xff", "0x7f")
# the convolution routes of tests/test_gpu_train.py::ROUTES (arithmetic switches of the trainer)
ROUTES = [{}, {"UMX_TRAIN_CONV_F32": "1"}, {"UMX_TRAIN_NO_KSPLIT": "1"}, {"UMX_TRAIN_WGRAD_F32": "1"},
          {"UMX_TRAIN_CONV_F32": "1", "UMX_TRAIN_WGRAD_F32": "1"}]
ROUTE_IDS = [",".join("%s=%s" % kv for kv in r.items()) or "f16x3" for r in ROUTES]

V2, LEG = model.GRAPH_V2, model.GRAPH_LEGACY
SHAPES = {   # name -> (hp, batch, regime)
    **{nm: (helpers.small_hps()[nm], B, rg) for nm, B, rg in [("v2_solo_like", 4, "solo"), ("v2_duo_like", 4, "duo"),
                                                             ("v2_deep", 3, "duo"), ("v2_wide", 2, "duo")]},
    "v2_k5": (model.HParams(V2, 32, 2, 3, 8, 2, 5, 0), 3, "duo"),
    "v2_b1_l1": (model.HParams(V2, 16, 1, 2, 4, 1, 3, 0), 1, "duo"),
    "v2_c3k4_odd": (model.HParams(V2, 16, 3, 4, 5, 2, 3, 0), 5, "duo"),
    "v2_l5_2x2": (model.HParams(V2, 64, 2, 3, 6, 5, 3, 0), 2, "duo"),
    "v2_k5_4x4": (model.HParams(V2, 16, 1, 3, 8, 2, 5, 0), 3, "duo"),
    "v2_128": (model.HParams(V2, 128, 1, 3, 4, 2, 3, 0), 1, "duo"),
    **{nm: (helpers.small_hps()[nm], B, "legacy") for nm, B in [("legacy_k5", 3), ("legacy_k3_x0", 4), ("legacy_k3_x2", 4)]},
    # the odd legacy shapes of tests/test_gpu_train_legacy.py::ODD
    "legacy_b1_l1": (model.HParams(LEG, 16, 1, 2, 4, 1, 3, 0), 1, "legacy"),
    "legacy_c3k4_odd": (model.HParams(LEG, 16, 3, 4, 5, 2, 3, 1), 3, "legacy"),
    "legacy_l5_2x2": (model.HParams(LEG, 64, 1, 3, 4, 5, 3, 0), 2, "legacy"),
    "legacy_k5_x2_4x4": (model.HParams(LEG, 16, 1, 3, 4, 2, 5, 2), 2, "legacy"),
    "legacy_128": (model.HParams(LEG, 128, 1, 3, 4, 2, 3, 1), 1, "legacy"),
}


def _options(regime):
    return {"solo": trainer.solo_options, "duo": trainer.duo_options, "legacy": trainer.legacy_options}[regime]()


def _batch(hp, B, seed):
    rng = np.random.default_rng(seed)
    data = rng.normal(0, 1, (B, hp.imSize, hp.imSize, hp.nChannels)).astype(np.float32)
    labels = np.eye(hp.nClasses, dtype=np.float32)[rng.integers(0, hp.nClasses, (B, hp.imSize, hp.imSize))]
    weights = rng.uniform(0.5, 3.0, labels.shape).astype(np.float32)
    return data, labels, weights


def site_names(hp):
    """Every decision-site tensor umx_trainer_read_tensor serves for this graph."""
    L, E = hp.nLayers, hp.nExtraConvs
    names = ["ds%d" % i for i in range(L + 1)] + ["lu%d.us" % i for i in range(L)]
    if hp.graph == LEG:
        names += ["lb.z", "lt.z"] + ["ld%d.stat" % i for i in range(L)]
        names += ["%s%d.%s" % (p, i, w) for p in ("ld", "lu") for i in range(L) for w in ["z"] + ["x%d" % e for e in range(E)]]
    else:
        names += ["%s.%s" % (s, w) for s in ["lb", "lt"] + ["ld%d" % i for i in range(L)] + ["lu%d" % i for i in range(L)]
                  for w in ("z", "stat")]
    return names


def _set_env(monkeypatch, route, fill):
    for k, v in route.items():
        monkeypatch.setenv(k, v)
    if fill is None:
        monkeypatch.delenv("UMX_DEBUG_GUARD", raising=False)
    else:
        monkeypatch.setenv("UMX_DEBUG_GUARD", fill)


def run_case(hp, B, regime, blob, monkeypatch, route, fill):
    """Two steps with the update applied (the optimiser slots live), one device-pointer step, then an eval pass; every output as
    bytes.  Under guards each call also checks every red zone (UmxError ERR_GUARD otherwise)."""
    import torch
    _set_env(monkeypatch, route, fill)
    legacy = hp.graph == LEG
    tr = trainer.Trainer(hp, blob, _options(regime), batch=B)
    out = {}
    try:
        for s in range(2):
            data, labels, weights = _batch(hp, B, 40 + s)
            if legacy and s == 0:
                weights = None                               # the unweighted loss (all-ones weights buffer)
            out["step%d.loss" % s] = np.array(tr.step(data, labels, weights))
        out["step1.grads"], out["step1.blob"] = tr.grads(), tr.blob()
        out["step1.m"], out["step1.v"] = tr.slots()
        data, labels, weights = _batch(hp, B, 42)
        dev = torch.device("cuda")
        td, tl, tw = (torch.from_numpy(a).to(dev) for a in (data, labels, weights))
        tr.step_dev(td.data_ptr(), tl.data_ptr(), tw.data_ptr())
        out["dev.loss"] = np.array(tr.loss())
        out["dev.grads"], out["dev.blob"], out["dev.probs"] = tr.grads(), tr.blob(), tr.probs()
        for name in site_names(hp):
            out["dev." + name] = tr.read_tensor(name)
        out["eval"] = tr.eval(data)
    finally:
        tr.close()
    monkeypatch.delenv("UMX_DEBUG_GUARD", raising=False)
    return out


def assert_same(a, b, what):
    assert a.keys() == b.keys()
    for k in a:
        x, y = np.asarray(a[k]), np.asarray(b[k])
        assert x.shape == y.shape and x.tobytes() == y.tobytes(), (what, k, float(np.nanmax(np.abs(x.astype(np.float64) - y))))


@pytest.mark.parametrize("route", ROUTES, ids=ROUTE_IDS)
@pytest.mark.parametrize("name", list(SHAPES))
def test_no_stray_writes_and_no_reads_of_unwritten_memory(name, route, monkeypatch):
    hp, B, regime = SHAPES[name]
    blob = model.random_blob(hp, seed=11)
    # the guarded runs first: a stray write is named there before a run without red zones could land it in a live buffer
    got = {fill: run_case(hp, B, regime, blob, monkeypatch, route, fill) for fill in FILLS}
    plain = run_case(hp, B, regime, blob, monkeypatch, route, None)
    assert all(np.isfinite(v).all() for v in plain.values()), name
    for fill, out in got.items():
        assert_same(out, plain, "%s under UMX_DEBUG_GUARD=%s" % (name, fill))


@pytest.mark.parametrize("which", ["synthetic-256_b8", "nucleiDAPI_b16"])
def test_full_size_under_guards(which, monkeypatch):
    if which.startswith("synthetic"):
        hp, B, regime = model.KNOWN_HP["synthetic-256"], 8, "duo"
        blob = model.random_blob(hp, seed=5)
    else:
        hp, blob, _, _ = helpers.load_nuclei_dapi("nucleiDAPI")
        B, regime = 16, "legacy"
    got = {fill: run_case(hp, B, regime, blob, monkeypatch, {}, fill) for fill in ("0x00", "0xff")}
    plain = run_case(hp, B, regime, blob, monkeypatch, {}, None)
    for fill, out in got.items():
        assert_same(out, plain, "%s under UMX_DEBUG_GUARD=%s" % (which, fill))


@pytest.mark.parametrize("graph", [V2, LEG], ids=["v2", "legacy"])
@pytest.mark.parametrize("fill", [None, "0xff"])
def test_a_1x1_bottom_is_refused(graph, fill, monkeypatch):
    """A 1x1 bottom layer: a 16 x 16 output tile of the convolution kernels then holds 256 images, whose 3x3 halos (2304 pixels)
    overflow the staging registers -- the same limit the inference engine's graph builder applies.  The trainer refuses the model
    cleanly (UMX_ERR_INVALID, every buffer allocated so far freed), with and without red zones."""
    _set_env(monkeypatch, {}, fill)
    hp = model.HParams(graph, 16, 1, 2, 4, 4, 3, 0)
    with pytest.raises(umx.UmxError) as e:
        trainer.Trainer(hp, model.random_blob(hp), _options("legacy" if graph == LEG else "duo"), batch=2)
    assert e.value.code == umx.ERR_INVALID and "halo too large" in str(e.value)


@pytest.mark.parametrize("graph", ["v2", "legacy"])
def test_guard_mode_covers_every_buffer(graph, monkeypatch, capfd):
    """The mode is on when asked (and only then): the trainer and its training set report how many buffers sit between red zones."""
    hp = helpers.small_hps()["v2_duo_like" if graph == "v2" else "legacy_k3_x0"]
    lw = trainset.LabelWeights(True, (1.0,) * hp.nClasses, (0.0,) * hp.nClasses)
    for fill in (None, "0x7f"):
        _set_env(monkeypatch, {}, fill)
        capfd.readouterr()
        tr = trainer.Trainer(hp, model.random_blob(hp), _options("duo" if graph == "v2" else "legacy"), batch=2)
        ts = trainset.TrainSet(tr, 2, 1, hp.imSize, lw)
        err = capfd.readouterr().err
        ts.close()
        tr.close()
        lines = [ln for ln in err.splitlines() if "UMX_DEBUG_GUARD" in ln]
        if fill is None:
            assert lines == []
        else:
            assert len(lines) == 2, err
            assert "UMX_DEBUG_GUARD=0x7f" in lines[0] and "trainer buffers" in lines[0]
            assert int(lines[0].split(": ")[1].split()[0]) >= 40, lines[0]          # every activation, gradient and plane buffer
            assert lines[1].endswith("6 training-set buffers between red zones"), lines[1]
    monkeypatch.delenv("UMX_DEBUG_GUARD", raising=False)


def test_a_bad_fill_is_refused(monkeypatch):
    hp = helpers.small_hps()["legacy_k3_x0"]
    monkeypatch.setenv("UMX_DEBUG_GUARD", "0x100")
    with pytest.raises(umx.UmxError) as e:
        trainer.Trainer(hp, model.random_blob(hp), trainer.legacy_options(), batch=2)
    assert e.value.code == umx.ERR_INVALID and "UMX_DEBUG_GUARD" in str(e.value)


# ---- the training set ----------------------------------------------------------------------------------------------------

def _descs(rows):
    d = np.zeros(len(rows), trainer.SAMPLE_DESC)
    for j, r in enumerate(rows):
        d[j] = tuple(r) + (0,)
    return d


def _set_data(hp, N, pages, S, seed):
    rng = np.random.default_rng(seed)
    planes = rng.normal(0, 1, (N, hp.nChannels, pages, S, S)).astype(np.float32)
    ann = rng.integers(0, hp.nClasses + 2, (N, S, S)).astype(np.uint8)          # codes 0 and > K: unlabelled pixels
    wmaps = [rng.random((S, S)).astype(np.float32) * 2 for _ in range(N)]
    wmaps[1] = None                                                             # a missing weight map
    return planes, ann, wmaps


def run_trainset(hp, B, regime, lw, monkeypatch, fill):
    """assemble / step_sampled / evaluate on a set of 45-pixel samples and on one whose samples are exactly one tile (S == P)."""
    _set_env(monkeypatch, {}, fill)
    P, pages = hp.imSize, 3
    tr = trainer.Trainer(hp, model.random_blob(hp, seed=9), _options(regime), batch=B)
    out = {}
    try:
        for S in (45, P):
            planes, ann, wmaps = _set_data(hp, 3, pages, S, S)
            ts = trainset.TrainSet.from_arrays(tr, planes, ann, wmaps, lw)
            far = S - P
            # every transform, crops at 0 and S - P on both axes, the last page, the sample without a weight map
            rows = [(t % 3, (pages - 1, t % pages)[t % 2], (far, 0, far, min(1, far))[t % 4], (far, far, 0, 0)[t % 4], t,
                     0.25 - 0.125 * t, 1.0 + 0.05 * t) for t in range(8)]
            for j, d in enumerate((_descs(rows[:B]), _descs(rows[B:]), _descs(rows[B - 1:B]), _descs(rows[1:B]))):   # n = B, 1, < B
                for k, a in enumerate(tr.assemble(ts, d)):
                    out["S%d.assemble%d.%d" % (S, j, k)] = np.zeros(0) if a is None else a
            for s in range(2):
                tr.step_sampled(ts, _descs([rows[(s * 3 + b) % 8] for b in range(B)]))
                out["S%d.sampled%d.loss" % (S, s)] = np.array(tr.loss())
            out["S%d.grads" % S], out["S%d.blob" % S], out["S%d.probs" % S] = tr.grads(), tr.blob(), tr.probs()
            ev = tr.evaluate(ts, _descs(rows + rows[:B + 1]))                       # 9 + B descriptors: not a multiple of B
            out["S%d.counts" % S], out["S%d.loss_sum" % S] = ev["counts"], np.array(ev["loss_sum"])
            ts.close()
    finally:
        tr.close()
    monkeypatch.delenv("UMX_DEBUG_GUARD", raising=False)
    return out


@pytest.mark.parametrize("graph", ["legacy_weighted", "legacy_unweighted", "v2"])
def test_training_set_under_guards(graph, monkeypatch):
    if graph == "v2":
        hp, regime, lw = helpers.small_hps()["v2_duo_like"], "duo", trainset.LabelWeights(True, (1.0, 2.0, 7.0), (0.0, 15.0, 0.25))
    else:
        hp, regime = model.HParams(LEG, 32, 1, 2, 8, 2, 3, 0), "legacy"
        lw = trainset.LabelWeights(True, (0.5, 3.0), (1.5, 0.0)) if graph == "legacy_weighted" else trainset.UNWEIGHTED
    B = 4
    got = {fill: run_trainset(hp, B, regime, lw, monkeypatch, fill) for fill in FILLS}
    plain = run_trainset(hp, B, regime, lw, monkeypatch, None)
    for fill, out in got.items():
        assert_same(out, plain, "%s set under UMX_DEBUG_GUARD=%s" % (graph, fill))
