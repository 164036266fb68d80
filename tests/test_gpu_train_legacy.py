"""GPU tests of the legacy graph's training step (reference UnMicst.py:80-186 graph, :270-279 loss and optimiser) through the
C ABI of include/umx_train.h, against tests/legacy_train_ref.py (float64 autograd).

The gradients are compared on the kernels' own decisions (every ReLU branch and pool choice rebuilt from umx_trainer_read_tensor,
as tests/train_parity.py::_hip_decisions does for v2), so every tensor is held to TIGHT: max-abs error <= 2e-5 of its max-abs."""
import numpy as np
import pytest
import torch

import helpers
import legacy_train_ref as ref
from unmicst_amd import model, trainer, umx

pytestmark = pytest.mark.gpu

TIGHT = 2e-5
SMALL = [("legacy_k5", 3), ("legacy_k3_x0", 4), ("legacy_k3_x2", 4)]
# every convolution route of tests/test_gpu_train.py::ROUTES (UMX_TRAIN_* arithmetic switches)
ROUTES = [{}, {"UMX_TRAIN_CONV_F32": "1"}, {"UMX_TRAIN_NO_KSPLIT": "1"}, {"UMX_TRAIN_WGRAD_F32": "1"},
          {"UMX_TRAIN_CONV_F32": "1", "UMX_TRAIN_WGRAD_F32": "1"}]


def _batch(hp, B, seed):
    rng = np.random.default_rng(seed)
    data = rng.normal(0, 1, (B, hp.imSize, hp.imSize, hp.nChannels)).astype(np.float32)
    labels = np.eye(hp.nClasses, dtype=np.float32)[rng.integers(0, hp.nClasses, (B, hp.imSize, hp.imSize))]
    return data, labels


def _sample_batches(hp, mean, std, B, nbatch):
    """Crops of 'UNet sample data' 105.tif (legacy preprocessing, then the model's normalisation) and labels from the fixture's
    reference probability maps in the model's class order: 0 background, 1 contours, 2 nuclei."""
    raw, cont, _, nuc = helpers.load_sample_105()
    I = (helpers.legacy_preprocess(raw) - mean) / std
    c, n = cont.astype(np.float64) / 255, nuc.astype(np.float64) / 255
    lab = np.stack([np.clip(1 - c - n, 0, 1), c, n], -1)
    lab /= lab.sum(-1, keepdims=True)
    P, rng, out = hp.imSize, np.random.default_rng(7), []
    for _ in range(nbatch):
        ys, xs = rng.integers(0, I.shape[0] - P, B), rng.integers(0, I.shape[1] - P, B)
        d = np.stack([I[y:y + P, x:x + P] for y, x in zip(ys, xs)])[..., None].astype(np.float32)
        y = np.stack([lab[y:y + P, x:x + P] for y, x in zip(ys, xs)]).astype(np.float32)
        out.append((d, y))
    return out


def _decisions(tr, hp, B):
    """The ReLU branches and pool choices of the kernels' last forward pass: a ReLU's branch is the sign of the tensor in front
    of it; a pool takes the first maximum of relu(z) * scale + shift, formed as the kernel's fused multiply-add (float64 product
    of two float32, one rounding to float32)."""
    n, L, E, S = hp.nOutX, hp.nLayers, hp.nExtraConvs, hp.imSize
    dec = {}

    def t(name, S, C):
        return tr.read_tensor(name).reshape(B, S, S, C)

    def mask(a):
        return torch.from_numpy(np.ascontiguousarray((a > 0).astype(np.float64).transpose(0, 3, 1, 2)))

    for i in range(L):
        C = n[i + 1]
        for e in range(E):
            dec["ld%d.x%d" % (i, e)] = mask(t("ld%d.x%d" % (i, e), S, C))
        z = t("ld%d.z" % i, S, C)
        dec["ld%d.z" % i] = mask(z)
        st = tr.read_tensor("ld%d.stat" % i).reshape(4, C).astype(np.float64)
        v = (np.maximum(z, 0).astype(np.float64) * st[2] + st[3]).astype(np.float32)
        win = v.reshape(B, S // 2, 2, S // 2, 2, C).transpose(0, 1, 3, 5, 2, 4).reshape(B, S // 2, S // 2, C, 4)
        dec["pool%d" % i] = torch.from_numpy(np.ascontiguousarray(win.argmax(-1).transpose(0, 3, 1, 2))).long()
        S //= 2
    dec["lb.z"] = mask(t("lb.z", S, n[L + 1]))
    for idx in range(L - 1, -1, -1):
        S *= 2
        C = n[idx + 1]
        dec["lu%d.us" % idx] = mask(t("lu%d.us" % idx, S, C))
        for e in range(E):
            dec["lu%d.x%d" % (idx, e)] = mask(t("lu%d.x%d" % (idx, e), S, C))
        dec["lu%d.z" % idx] = mask(t("lu%d.z" % idx, S, C))
    return dec


def _check_tight(hp, got, want, what):
    G, W = ref.split_blob(hp, got), ref.split_blob(hp, want)
    for name in W:
        if not ref.trainable(name):
            continue
        scale = np.abs(W[name]).max()
        err = np.abs(G[name] - W[name]).max()
        assert err <= TIGHT * scale + 1e-9, (what, name, err, scale)


@pytest.mark.parametrize("route", ROUTES, ids=lambda r: ",".join("%s=%s" % kv for kv in r.items()) or "f16x3")
@pytest.mark.parametrize("name,B", SMALL)
def test_loss_probabilities_and_gradients_match_reference(name, B, route, monkeypatch):
    for k, v in route.items():
        monkeypatch.setenv(k, v)
    hp = helpers.small_hps()[name]
    blob = model.random_blob(hp, seed=21)
    data, labels = _batch(hp, B, 3)
    tr = trainer.Trainer(hp, blob, trainer.legacy_options(), batch=B)
    loss, data_term, reg = tr.step(data, labels, None, apply_update=False)
    assert tr.step_count == 0 and reg == 0.0 and loss == data_term
    want_loss, want_g, want_p, stats = ref.loss_and_grads(hp, blob, data, labels, decisions=_decisions(tr, hp, B))
    assert loss == pytest.approx(want_loss, rel=1e-5)
    assert np.abs(tr.probs() - want_p).max() <= 2e-5
    _check_tight(hp, tr.grads(), want_g, name)
    for i in range(hp.nLayers):
        st = tr.read_tensor("ld%d.stat" % i).reshape(4, -1)
        mean, var, _ = stats["ld%d" % i]
        assert np.abs(st[0] - mean).max() <= 1e-5 * max(1.0, np.abs(mean).max())
        assert np.abs(st[1] - 1 / np.sqrt(var + ref.BN_EPS)).max() <= 1e-5 * np.abs(st[1]).max()
    assert np.array_equal(tr.blob(), blob)
    tr.close()


def _check_step(hp, B, blob, data, labels, weights, what):
    """One step without update against the float64 reference on the kernels' own decisions: loss, probabilities, every gradient."""
    tr = trainer.Trainer(hp, blob, trainer.legacy_options(), batch=B)
    loss, data_term, reg = tr.step(data, labels, weights, apply_update=False)
    assert reg == 0.0 and loss == data_term
    want_loss, want_g, want_p, _ = ref.loss_and_grads(hp, blob, data, labels, weights, decisions=_decisions(tr, hp, B))
    assert loss == pytest.approx(want_loss, rel=1e-5), what
    assert np.abs(tr.probs() - want_p).max() <= 2e-5, what
    _check_tight(hp, tr.grads(), want_g, what)
    assert np.array_equal(tr.blob(), blob)
    tr.close()


# legacy shapes off the beaten path (HParams(GRAPH_LEGACY, imSize, nChannels, nClasses, nOut0, nLayers, ks, nExtraConvs), batch);
# a 1x1 bottom is refused (tests/test_gpu_train_guard.py::test_a_1x1_bottom_is_refused)
ODD = [
    ((16, 1, 2, 4, 1, 3, 0), 1),      # one level, one image, two classes
    ((16, 3, 4, 5, 2, 3, 1), 3),      # three input channels, four classes, odd widths and batch
    ((64, 1, 3, 4, 5, 3, 0), 2),      # five levels down to a 2x2 bottom
    ((16, 1, 3, 4, 2, 5, 2), 2),      # 5x5 filters, two extra convolutions, 4x4 bottom
    ((128, 1, 3, 4, 2, 3, 1), 1),     # one large image
]


@pytest.mark.parametrize("hp_args,B", ODD, ids=["b1_l1", "c3k4_odd", "l5_2x2", "k5_x2_4x4", "im128"])
def test_odd_shapes_match_reference(hp_args, B):
    hp = model.HParams(model.GRAPH_LEGACY, *hp_args)
    blob = model.random_blob(hp, seed=17)
    data, labels = _batch(hp, B, 23)
    _check_step(hp, B, blob, data, labels, None, "odd shape %r" % (hp_args,))


@pytest.mark.parametrize("name,B", SMALL)
def test_weighted_loss_matches_reference(name, B):
    """The weighted form step_sampled uses with class / intersect weights: non-uniform per-pixel, per-class weights."""
    hp = helpers.small_hps()[name]
    blob = model.random_blob(hp, seed=8)
    data, labels = _batch(hp, B, 12)
    weights = np.random.default_rng(13).uniform(0.25, 4.0, labels.shape).astype(np.float32)
    _check_step(hp, B, blob, data, labels, weights, "weighted " + name)


@pytest.mark.parametrize("graph", [model.GRAPH_LEGACY, model.GRAPH_V2], ids=["legacy", "v2"])
def test_one_class_is_refused(graph):
    """nClasses == 1: the softmax of a single class is 1 everywhere, so the cross-entropy and all its gradients vanish -- the
    trainer refuses the model instead of running a step that cannot learn."""
    hp = model.HParams(graph, 16, 1, 1, 4, 2, 3, 0)
    opts = trainer.legacy_options() if graph == model.GRAPH_LEGACY else trainer.duo_options()
    with pytest.raises(umx.UmxError) as e:
        trainer.Trainer(hp, model.random_blob(hp), opts, batch=2)
    assert e.value.code == umx.ERR_INVALID and "nClasses" in str(e.value)


def test_nucleidapi_gradients_at_real_size():
    hp, blob, mean, std = helpers.load_nuclei_dapi("nucleiDAPI")
    B = 4
    (data, labels), = _sample_batches(hp, mean, std, B, 1)
    tr = trainer.Trainer(hp, blob, trainer.legacy_options(), batch=B)
    loss = tr.step(data, labels, None, apply_update=False)[0]
    want_loss, want_g, _, _ = ref.loss_and_grads(hp, blob, data, labels, decisions=_decisions(tr, hp, B))
    assert loss == pytest.approx(want_loss, rel=1e-5)
    g = tr.grads()
    _check_tight(hp, g, want_g, "nucleiDAPI")
    # the kernel's own loss, differenced in the parameters: agrees with the kernel's gradient
    T = model.tensors_from_blob(hp, blob)
    offs, pos = {}, 0
    for nm, shape in model.tensor_specs(hp):
        offs[nm] = pos
        pos += int(np.prod(shape))
    for nm in ("ld0.wshort", "lb.w"):
        k = offs[nm] + int(np.argmax(np.abs(g[offs[nm]:offs[nm] + T[nm].size])))
        h = 2e-3 * max(abs(float(blob[k])), 1e-2)
        ls = []
        for sgn in (1, -1):
            b = blob.copy()
            b[k] += sgn * h
            t2 = trainer.Trainer(hp, b, trainer.legacy_options(), batch=B)
            ls.append(t2.step(data, labels, None, apply_update=False)[0])
            t2.close()
        fd = (ls[0] - ls[1]) / (2 * h)
        assert fd == pytest.approx(float(g[k]), rel=5e-2, abs=1e-6), (nm, fd, g[k])
    tr.close()


def test_momentum_steps_match_reference():
    hp = helpers.small_hps()["legacy_k5"]
    opts = trainer.legacy_options(decay_steps=2)
    ro = ref.LegacyOptions(decay_steps=2)
    blob = model.random_blob(hp, seed=4)
    st = ref.TrainState(blob)
    tr = trainer.Trainer(hp, blob, opts, batch=4)
    for s in range(4):
        data, labels = _batch(hp, 4, 70 + s)
        got = tr.step(data, labels, None)[0]
        want = ref.train_step(hp, st, data, labels, ro)
        assert got == pytest.approx(want, rel=5e-5), s
    T_g, T_w, T_0 = ref.split_blob(hp, tr.blob()), ref.split_blob(hp, st.blob), ref.split_blob(hp, blob)
    for nm in T_w:   # (the bound of tests/test_gpu_train.py::test_momentum_steps_match_oracle_tightly)
        assert np.abs(T_g[nm] - T_w[nm]).max() <= 5e-2 * np.abs(T_w[nm] - T_0[nm]).max() + 2e-6, nm
    M_g, M_w = ref.split_blob(hp, tr.slots()[0]), ref.split_blob(hp, st.m)
    for nm in M_w:
        assert np.abs(M_g[nm] - M_w[nm]).max() <= 5e-2 * np.abs(M_w[nm]).max() + 2e-6, nm
    tr.close()


def test_eval_inference_and_conversion(tmp_path):
    from oracle import oracle
    hp = helpers.small_hps()["legacy_k3_x2"]
    blob = model.random_blob(hp, seed=31)
    tr = trainer.Trainer(hp, blob, trainer.legacy_options(lr0=0.05), batch=4)
    data, labels = _batch(hp, 4, 2)
    assert np.abs(tr.eval(data) - oracle.forward(hp, blob, data)).max() <= 1e-5
    for s in range(3):
        tr.step(*_batch(hp, 4, 10 + s))
    trained = tr.blob()
    assert not np.array_equal(trained, blob)
    assert np.abs(tr.eval(data) - oracle.forward(hp, trained, data)).max() <= 1e-5
    with umx.Engine(hp, trained, max_batch=4, precision="f32") as eng:
        assert np.abs(eng.forward_tiles(data) - oracle.forward(hp, trained, data)).max() <= 1e-4
    d = str(tmp_path / "m")
    model.save_converted(model.ModelArtefacts(hp, trained, 0.0, 1.0), d)
    art = model.load_model_dir(d)
    assert art.hp.graph == model.GRAPH_LEGACY and art.hp == hp and np.array_equal(art.blob, trained)
    tr.close()


def test_determinism_step_dev_and_unweighted():
    hp = helpers.small_hps()["legacy_k3_x0"]
    blob = model.random_blob(hp, seed=2)
    data, labels = _batch(hp, 4, 6)
    outs = []
    for _ in range(2):
        tr = trainer.Trainer(hp, blob, trainer.legacy_options(), batch=4)
        losses = [tr.step(data, labels)[0] for _ in range(2)]
        outs.append((losses, tr.grads(), tr.blob()))
        tr.close()
    assert outs[0][0] == outs[1][0]
    assert np.array_equal(outs[0][1], outs[1][1]) and np.array_equal(outs[0][2], outs[1][2])
    # all-ones weights == weights None, bit for bit
    tr = trainer.Trainer(hp, blob, trainer.legacy_options(), batch=4)
    l1 = tr.step(data, labels, np.ones_like(labels))[0]
    g1, b1 = tr.grads(), tr.blob()
    tr.close()
    tr = trainer.Trainer(hp, blob, trainer.legacy_options(), batch=4)
    l0 = tr.step(data, labels, None)[0]
    assert l0 == l1 and np.array_equal(tr.grads(), g1) and np.array_equal(tr.blob(), b1)
    tr.close()
    # step_dev == step
    dev = torch.device("cuda")
    td, tl = torch.from_numpy(data).to(dev), torch.from_numpy(labels).to(dev)
    tr = trainer.Trainer(hp, blob, trainer.legacy_options(), batch=4)
    tr.step_dev(td.data_ptr(), tl.data_ptr(), None)
    assert tr.loss()[0] == l0 and np.array_equal(tr.grads(), g1) and np.array_equal(tr.blob(), b1)
    tr.close()


def test_fine_tuning_nucleidapi_learns():
    hp, blob, mean, std = helpers.load_nuclei_dapi("nucleiDAPI")
    batches = _sample_batches(hp, mean, std, 4, 3)
    tr = trainer.Trainer(hp, blob, trainer.legacy_options(), batch=4)
    losses = [tr.step(*batches[s % 3])[0] for s in range(30)]
    tr.close()
    assert np.isfinite(losses).all()
    assert np.mean(losses[-5:]) < np.mean(losses[:5]), losses


def test_refusals():
    hp = helpers.small_hps()["legacy_k5"]
    blob = model.random_blob(hp)
    with pytest.raises(ValueError):
        trainer.Trainer(hp, blob, trainer.legacy_options(drop_bottom=0.3))
    with pytest.raises(ValueError):
        trainer.Trainer(hp, blob, trainer.legacy_options(reg_kind=trainer.REG_L1, reg_down=1e-4))
    # the same through the C call: UMX_ERR_INVALID
    import ctypes
    L = trainer._bind(umx.load())
    for kw in ({"drop_bottom": 0.3}, {"drop_up0": 0.1}, {"reg_kind": trainer.REG_L2}):
        o = trainer._TrainOptions()
        L.umx_train_options_legacy(ctypes.byref(o))
        for k, v in kw.items():
            setattr(o, k, v)
        b = np.ascontiguousarray(blob, np.float32)
        h = ctypes.c_void_p()
        hps = umx._hp_struct(hp)
        assert L.umx_trainer_create(ctypes.byref(hps), b.ctypes.data, b.size, ctypes.byref(o), ctypes.byref(h)) == umx.ERR_INVALID, kw
    v2 = helpers.small_hps()["v2_duo_like"]
    tr = trainer.Trainer(v2, model.random_blob(v2), trainer.duo_options(), batch=2)
    d, y = _batch(v2, 2, 1)
    with pytest.raises(ValueError):
        tr.step(d, y, None)
    tr.close()
