"""GPU tests of the object score (include/umx_train.h: umx_trainer_object_counts, umx_trainer_evaluate_objects; DESIGN.md section 9.2,
"Object score") against tests/trainset_objects_ref.py.  Everything is an integer, so everything is compared for equality: per-image
counts and both label planes at two tile sizes -- P = 32 (a row is half a 64-lane ballot chunk) and P = 128 (a row crosses one; a batch
of 3 with 2 images given leaves n < B) -- then isolation of the images of a batch, two calls giving the same bytes, the kernels staying
inside their buffers under UMX_DEBUG_GUARD, refused calls, the entry behind Trainer.evaluate against the plain one, and the command."""
import ctypes
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import helpers
import trainset_border_ref as bref
import trainset_objects_ref as oref
import trainset_ref as ref
from unmicst_amd import finetune, model, trainer, trainset, umx

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_INVALID = 1
OBJ = oref.OBJ

# tile -> (hyper-parameters, batch, options, label weights)
SETUPS = {
    32: (helpers.small_hps()["v2_duo_like"], 2, trainer.duo_options, trainset.LABEL_WEIGHTS["duo"]),
    128: (model.HParams(model.GRAPH_V2, 128, 1, 3, 4, 2, 3, 0), 3, trainer.solo_options, trainset.LABEL_WEIGHTS["solo"]),
}


def _trainer_and_set(P, S=None):
    """A trainer of tile P and a one-sample set of S x S (default P x P) blobs in its memory."""
    hp, B, opts, lw = SETUPS[P]
    S = P if S is None else S
    tr = trainer.Trainer(hp, model.random_blob(hp, seed=3), opts(), batch=B)
    rng = np.random.default_rng(1)
    planes = rng.normal(0, 1, (1, hp.nChannels, 1, S, S)).astype(np.float32)
    ann = [bref.blobs(S, 7, 1.5, 0.7)]
    return tr, trainset.TrainSet.from_arrays(tr, planes, ann, None, lw), planes, ann


@pytest.fixture(scope="module", params=sorted(SETUPS))
def rig(request):
    tr, ts, _, _ = _trainer_and_set(request.param)
    yield request.param, tr, ts
    tr.close()


@functools.lru_cache(maxsize=None)
def _cases(P):
    """name -> (truth, pred, min_area, per-image counts, truth labels, predicted labels): the restatement, computed once, read-only."""
    out = {}
    every = {k: v[:3] for k, v in oref.hand_made(P).items()}
    every.update(oref.large_cases(P))
    for name, (t, p, min_area) in every.items():
        c, tl, pl = oref.object_counts(t, p, OBJ, min_area)
        for a in (t, p, c, tl, pl):
            a.setflags(write=False)
        out[name] = (t, p, min_area, c, tl, pl)
    return out


CASE_NAMES = sorted(_cases(32))


def _assert_image(got, want, what):
    for g, w, name in zip(got, want, ("counts", "truth labels", "predicted labels")):
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.dtype, g.shape)
        ne = g != w
        assert not ne.any(), (what, name, g[ne][:6].tolist(), w[ne][:6].tolist(), np.argwhere(ne)[:4].tolist())


@pytest.mark.parametrize("name", CASE_NAMES)
def test_counts_and_labels_against_the_restatement(rig, name):
    P, tr, ts = rig
    t, p, min_area, c, tl, pl = _cases(P)[name]
    # what the input must exercise, asserted on the restatement
    if name == "stripes":
        assert tuple(c[:2]) == (P // 2, P // 2) and ((tl > 0) & (pl > 0)).sum() == (P // 2) ** 2
    elif name == "identical_blobs":
        assert c[0] >= 4 and c[0] == c[1] == c[2] == c[3]
    elif name == "blobs_shifted":
        assert c[2] >= 2 and c[3] < c[0]
    elif name == "blobs_eroded":
        assert c[1] > c[0] and c[5] >= 1 and c[3] == 0    # necks break: more predicted objects than annotated ones, and splits
    elif name == "blobs_eroded_min_area_5":
        assert c[1] < _cases(P)["blobs_eroded"][3][1]
    elif name == "checkerboard":
        assert c[0] == P * P // 2 == c[2]
    elif name == "serpentine":
        assert c[0] == 1 and (tl[t == OBJ] == 1).all()
    # the case sits next to an image that is one object against background stripes: nothing may come from a neighbour
    full = np.full((P, P), OBJ, np.uint8)
    other = oref.stripes(P)[1]
    opts = trainset.ObjectOptions(None, min_area)
    per, gtl, gpl = tr.object_counts(ts, np.stack([t, full]), np.stack([p, other]), opts, labels=True)
    print(name, P, dict(zip(oref.NAMES, per[0].tolist())))
    _assert_image((per[0], gtl[0], gpl[0]), (c, tl, pl), (name, P))
    _assert_image((per[1], gtl[1], gpl[1]), oref.object_counts(full, other, OBJ, min_area), (name, P, "neighbour"))
    # alone in the batch (n = 1 < B), without the label planes
    alone = tr.object_counts(ts, t[None], p[None], opts)
    assert alone.shape == (1, 8) and np.array_equal(alone[0], c)


def test_the_plane_rule_is_applied_to_uploaded_planes(rig):
    P, tr, ts = rig
    t, p, _, c, tl, pl = _cases(P)["unlabelled_block"]
    assert (p[t == 0] == OBJ).any()
    ruled = oref.plane_rule(t, p)
    a = tr.object_counts(ts, t[None], p[None], trainset.ObjectOptions(), labels=True)
    b = tr.object_counts(ts, t[None], ruled[None], trainset.ObjectOptions(), labels=True)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
    assert (a[2][0][t == 0] == 0).all()


def test_another_class_and_codes_above_the_classes(rig):
    P, tr, ts = rig
    t, p, _, _, _, _ = _cases(P)["merge"]
    t2 = t.copy()
    t2[20:24, 20:24] = 200                                # a code no class has is labelled nothing, but it is not 0: the rule leaves pred
    opts = trainset.ObjectOptions(1)                      # the contour class
    per, gtl, gpl = tr.object_counts(ts, t2[None], p[None], opts, labels=True)
    _assert_image((per[0], gtl[0], gpl[0]), oref.object_counts(t2, p, oref.RING), "contour class")
    assert per[0][0] == 1 and per[0][1] == 0


def test_changing_one_image_leaves_the_other(rig):
    P, tr, ts = rig
    cases = _cases(P)
    t0, p0, _, c0, tl0, pl0 = cases["blobs_shifted"]
    opts = trainset.ObjectOptions()
    first = None
    for name in ("stripes", "checkerboard", "both_empty"):
        t1, p1 = cases[name][:2]
        per, gtl, gpl = tr.object_counts(ts, np.stack([t0, t1]), np.stack([p0, p1]), opts, labels=True)
        mine = (per[0].tobytes(), gtl[0].tobytes(), gpl[0].tobytes())
        first = first or mine
        assert mine == first, name
        assert np.array_equal(per[1], cases[name][3]), name
    assert np.array_equal(np.frombuffer(first[0], np.int64), c0)


def test_two_calls_give_the_same_bytes(rig):
    P, tr, ts = rig
    cases = _cases(P)
    for name in ("stripes", "blobs_eroded", "checkerboard"):
        t, p = cases[name][:2]
        n = min(2, tr.batch)
        args = (np.stack([t] * n), np.stack([p] * n), trainset.ObjectOptions())
        first = tr.object_counts(ts, *args, labels=True)
        tr.object_counts(ts, np.stack([p] * n), np.stack([t] * n), trainset.ObjectOptions(None, 3))      # something else in between
        again = tr.object_counts(ts, *args, labels=True)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(first, again)), name
        assert np.array_equal(first[0][0], first[0][-1])


_GUARD_CHILD = """
import sys
import numpy as np
import test_gpu_trainset_objects as t
from unmicst_amd import trainset
tr, ts, _, _ = t._trainer_and_set(32, 40)
out = {}
for name, (tp, pp, min_area, c, tl, pl) in t._cases(32).items():
    per, gtl, gpl = tr.object_counts(ts, np.stack([tp, pp]), np.stack([pp, tp]), trainset.ObjectOptions(None, min_area), labels=True)
    out[name + ".per"], out[name + ".tl"], out[name + ".pl"] = per[0], gtl[0], gpl[0]
d = trainset.validation_descriptors(1, 40, 32)
ev = tr.evaluate(ts, d, objects=trainset.ObjectOptions())
out["objects"] = np.array([ev["objects"][k] for k in ("truth", "predicted", "matched")])
np.savez(sys.argv[1], **out)
tr.close()
"""


def test_the_case_list_under_the_debug_guard(tmp_path):
    """Every red zone of the set -- those of the object workspace included -- is checked at the end of every call."""
    out = str(tmp_path / "guarded.npz")
    env = dict(os.environ, UMX_DEBUG_GUARD="0xff", PYTHONPATH=os.pathsep.join([ROOT, os.path.join(ROOT, "tests")]))
    r = subprocess.run([sys.executable, "-c", _GUARD_CHILD, out], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    assert "UMX_DEBUG_GUARD=0xff" in r.stderr
    z = np.load(out)
    for name, (_, _, _, c, tl, pl) in _cases(32).items():
        _assert_image((z[name + ".per"], z[name + ".tl"], z[name + ".pl"]), (c, tl, pl), ("guarded", name))
    assert z["objects"][0] > 0


def _raw_counts(tr, ts, truth, pred, n, code=3, min_area=1, reserved=None, per=True):
    o = trainer.ObjectOptionsC()
    o.object_code, o.min_area = code, min_area
    if reserved is not None:
        o.reserved[reserved] = 7
    out = np.full((max(n, 1), 8), -5, np.int64)
    rc = tr._lib.umx_trainer_object_counts(tr._h, ts._handle(), None if truth is None else truth.ctypes.data,
                                           None if pred is None else pred.ctypes.data, n, ctypes.byref(o), out.ctypes.data if per else None,
                                           None, None)
    return rc, out


def test_refused_calls_enqueue_nothing(rig):
    P, tr, ts = rig
    B = tr.batch
    t, p = _cases(P)["blobs_shifted"][:2]
    T, Q = np.stack([t] * B), np.stack([p] * B)
    d = trainset.validation_descriptors(1, P, P)
    before = tr.evaluate(ts, d)
    steps = tr.step_count
    for kw in (dict(n=0), dict(n=B + 1), dict(code=0), dict(code=4), dict(min_area=0), dict(min_area=65537), dict(reserved=0), dict(reserved=5),
               dict(per=False)):
        kw.setdefault("n", 1)
        rc, out = _raw_counts(tr, ts, T, Q, **kw)
        assert rc == ERR_INVALID and (out == -5).all(), kw
    assert _raw_counts(tr, ts, None, Q, 1)[0] == ERR_INVALID and _raw_counts(tr, ts, T, None, 1)[0] == ERR_INVALID
    o = trainer.ObjectOptionsC()
    o.object_code, o.min_area = 3, 1
    L = tr._lib
    assert L.umx_trainer_object_counts(tr._h, ts._handle(), T.ctypes.data, Q.ctypes.data, 1, None, T.ctypes.data, None, None) == ERR_INVALID
    assert L.umx_trainer_object_counts(tr._h, None, T.ctypes.data, Q.ctypes.data, 1, ctypes.byref(o), T.ctypes.data, None, None) == ERR_INVALID
    assert L.umx_trainer_object_counts(None, ts._handle(), T.ctypes.data, Q.ctypes.data, 1, ctypes.byref(o), T.ctypes.data, None, None) == ERR_INVALID
    # the evaluation entry: bad options, a bad descriptor, missing outputs
    i64p = ctypes.POINTER(ctypes.c_int64)
    counts, obj = np.full(6, -5, np.int64), np.full(8, -5, np.int64)
    ls = ctypes.c_double(-5.0)

    def ev(desc, n, opt, c=counts, o_=obj):
        return L.umx_trainer_evaluate_objects(tr._h, ts._handle(), desc.ctypes.data, n, opt, None if c is None else c.ctypes.data_as(i64p),
                                              ctypes.byref(ls), None if o_ is None else o_.ctypes.data_as(i64p), None, None)
    bad = trainer.ObjectOptionsC()
    bad.object_code, bad.min_area = 4, 1
    off = d.copy()
    off["y0"] = 1
    assert ev(d, 1, ctypes.byref(bad)) == ERR_INVALID and ev(d, 1, None) == ERR_INVALID
    assert ev(off, 1, ctypes.byref(o)) == ERR_INVALID and ev(d, 0, ctypes.byref(o)) == ERR_INVALID
    assert ev(d, 1, ctypes.byref(o), o_=None) == ERR_INVALID and ev(d, 1, ctypes.byref(o), c=None) == ERR_INVALID
    assert (counts == -5).all() and (obj == -5).all() and ls.value == -5.0
    with pytest.raises(umx.UmxError) as e:
        tr.object_counts(ts, T[:1], Q[:1], _Opt(4, 1))
    assert e.value.code == ERR_INVALID and "object_code is 4" in str(e.value)
    # nothing ran: the trainer and the set answer as before
    after = tr.evaluate(ts, d)
    assert after["counts"].tobytes() == before["counts"].tobytes() and after["loss_sum"] == before["loss_sum"] and tr.step_count == steps
    good = tr.object_counts(ts, T[:1], Q[:1], trainset.ObjectOptions())
    assert np.array_equal(good[0], _cases(P)["blobs_shifted"][3])


class _Opt:
    """Options the Python class would refuse, handed to the library as they are."""

    def __init__(self, code, min_area):
        self.code, self.min_area = code, min_area

    def c_struct(self, n_classes):
        o = trainer.ObjectOptionsC()
        o.object_code, o.min_area = self.code, self.min_area
        return o


def test_evaluate_objects_end_to_end():
    """A set larger than the tile (the last validation crop is flush with the far edge): counts and loss of the plain entry bit for bit,
    the planes against Trainer.eval and the assembled labels, the objects against the restatement on those planes."""
    P, S = 32, 40
    tr, ts, planes, ann = _trainer_and_set(P, S)
    try:
        ann[0][3:9, 30:38] = 0                            # an unlabelled block
        ts.set(0, planes[0], ann[0])
        d = trainset.validation_descriptors(1, S, P)
        assert len(d) == 4 and d["y0"].max() == S - P
        opts = trainset.ObjectOptions()
        total = np.zeros(8, np.int64)
        pred_objects = 0
        for b0 in (0, 2):
            chunk = d[b0:b0 + 2]
            plain = tr.evaluate(ts, chunk)
            counts, loss_sum, obj, truth, pred = tr.evaluate_objects(ts, chunk, opts)
            assert counts.tobytes() == plain["counts"].tobytes() and np.float64(loss_sum).tobytes() == np.float64(plain["loss_sum"]).tobytes()
            data, labels, _ = tr.assemble(ts, chunk)
            probs = tr.eval(data)
            want_t, want_p = oref.planes_of(probs, labels)
            assert truth.dtype == np.uint8 and np.array_equal(truth, want_t) and np.array_equal(pred, want_p)
            assert np.array_equal(want_t, np.stack([ann[0][y:y + P, x:x + P] for y, x in zip(chunk["y0"], chunk["x0"])]))
            want = oref.batch_counts(truth, pred, OBJ)[0].sum(axis=0)
            print("chunk", b0, dict(zip(oref.NAMES, obj.tolist())))
            assert obj.dtype == np.int64 and np.array_equal(obj, want)
            total += obj
            pred_objects += int(want[1])
        assert (ann[0][:P, S - P:] == 0).any() and total[0] >= 4
        ev = tr.evaluate(ts, d, objects=opts)
        plain = tr.evaluate(ts, d)
        assert {k: ev["objects"][k] for k in oref.NAMES} == dict(zip(oref.NAMES, total[:6].tolist()))
        assert ev["objects"]["f1"] == oref.f1(total) or (np.isnan(ev["objects"]["f1"]) and np.isnan(oref.f1(total)))
        assert ev["counts"].tobytes() == plain["counts"].tobytes() and ev["loss_sum"] == plain["loss_sum"] and "objects" not in plain
        # min_area reaches the device through this entry too
        big = tr.evaluate(ts, d, objects=trainset.ObjectOptions(None, 40))["objects"]
        assert big["truth"] == total[0] and big["predicted"] <= total[1]
    finally:
        tr.close()


def _disc_sets(tmp_path, hp, S):
    rng = np.random.default_rng(8)
    yy, xx = np.mgrid[:S, :S]
    for name, n in (("train", 6), ("valid", 2)):
        raws, codes = [], []
        for _ in range(n):
            inner, outer = np.zeros((S, S), bool), np.zeros((S, S), bool)
            for _ in range(6):
                cy, cx = rng.integers(0, S, 2).tolist()
                r = int(rng.integers(5, 9))
                d2 = (yy - cy) ** 2 + (xx - cx) ** 2
                outer |= d2 < r * r
                inner |= d2 < (r - 2) * (r - 2)
            rim = outer & ~inner
            level = np.where(inner, 0.8, np.where(rim, 0.5, 0.2))
            codes.append(np.where(inner, 3, np.where(rim, 2, 1)).astype(np.uint8))
            raws.append(np.clip((level + rng.normal(0, 0.05, (S, S))) * 255, 0, 255).astype(np.uint8)[None, None])
        ref.write_dataset(str(tmp_path / name), raws, codes)


def test_the_command_logs_and_selects_by_the_object_score(tmp_path, capfd):
    hp = model.HParams(model.GRAPH_V2, 32, 1, 3, 8, 2, 3, 0, batchSize=4)            # a solo stand-in: hyper-parameters only
    mdir = str(tmp_path / "solo_like")
    os.makedirs(mdir)
    np.savez(os.path.join(mdir, model.HP_ONLY_NAME), hp=model._hp_vector(hp), mean=np.float64(0.4), std=np.float64(0.25))
    _disc_sets(tmp_path, hp, 48)
    base = ["--model", mdir, "--train", str(tmp_path / "train"), "--valid", str(tmp_path / "valid"), "--steps", "60", "--eval-every", "15",
            "--seed", "5", "--from-scratch", "--lr0", "0.002"]
    plain, scored = str(tmp_path / "plain"), str(tmp_path / "scored")
    assert finetune.main(base + ["--out", plain]) == 0
    capfd.readouterr()
    assert finetune.main(base + ["--out", scored, "--object-score", "--select", "object", "--object-min-area", "2"]) == 0
    printed = capfd.readouterr().out
    old = [json.loads(l) for l in open(os.path.join(plain, finetune.LOG_NAME))]
    new = [json.loads(l) for l in open(os.path.join(scored, finetune.LOG_NAME))]
    assert list(old[0]) == ["init"] and all("objects" not in r for r in old)
    assert list(new[0]) == ["init", "objects"] and new[0]["objects"] == {"class": 2, "min_area": 2, "select": "object"}
    assert len(old) == len(new) == 6
    for a, b in zip(old, new):                            # the keys that existed before hold what they held
        assert {k: v for k, v in b.items() if k != "objects"} == a
    evals = new[1:]
    assert [r["step"] for r in evals] == [0, 15, 30, 45, 60]
    for r in evals:
        o = r["objects"]
        assert list(o) == list(oref.NAMES) + ["f1"] and o["truth"] == evals[0]["objects"]["truth"] > 0
        assert o["f1"] == (2.0 * o["matched"] / (o["truth"] + o["predicted"]))
    f1s = [r["objects"]["f1"] for r in evals]
    kept = evals[int(np.argmax(f1s))]["step"]             # (np.argmax: the first of equal maxima)
    assert "best object F1 %.6g at step %d " % (max(f1s), kept) in printed, printed[-400:]
    a, b = np.load(os.path.join(plain, model.CONVERTED_NAME)), np.load(os.path.join(scored, model.CONVERTED_NAME))
    assert sorted(a.files) == sorted(b.files)
    by_pixel = evals[int(np.argmin([r["mean_error"] for r in evals]))]["step"]
    for k in a.files:                                     # the same step kept by both scores is the same model, bit for bit
        if k != "blob" or kept == by_pixel:
            assert a[k].tobytes() == b[k].tobytes(), k
    # refusals come before any device work
    assert finetune.main(base + ["--out", str(tmp_path / "no"), "--select", "object"]) == 2
    assert "--select object needs --object-score" in capfd.readouterr().err
    assert finetune.main(base + ["--out", str(tmp_path / "no"), "--object-score", "--object-class", "3"]) == 2
    assert "the model has classes 0..2" in capfd.readouterr().err
    assert not os.path.exists(str(tmp_path / "no"))
    print("kept step %d (by pixel error: %d)" % (kept, by_pixel), json.dumps([r["objects"] for r in evals]))
