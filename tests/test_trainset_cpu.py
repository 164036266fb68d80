"""Host checks of the device-resident training set: the dataset reader (the reference's published layout), the numpy restatement
of the assembly kernel (tests/trainset_ref.py), the descriptor sampler, the finetune command's refusals (all before any device
work) and the C layout of umx_sample_desc / umx_label_weights."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import helpers
import trainset_ref as ref
from unmicst_amd import finetune, imtools, model, trainer, trainset

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _synthetic_dir(path, C=2, pages=3, S=20, seed=0, with_wt=(True, False, True)):
    """Three samples with uint8, uint16 and float32 pages; returns the raw pages [n][C][pages][S][S] as written."""
    rng = np.random.default_rng(seed)
    raws, codes, wts = [], [], []
    for i, dt in enumerate((np.uint8, np.uint16, np.float32)):
        if dt == np.float32:
            r = rng.random((C, pages, S, S)).astype(np.float32)
        else:
            r = rng.integers(0, np.iinfo(dt).max, (C, pages, S, S)).astype(dt)
        raws.append(r)
        codes.append(rng.integers(0, 5, (S, S)).astype(np.uint8))
        wts.append(rng.random((S, S)).astype(np.float32) * 3 if with_wt[i] else None)
    ref.write_dataset(path, raws, codes, wts)
    return raws, codes, wts


def test_reader_round_trip(tmp_path):
    mean, std = 0.34, 0.25
    raws, codes, wts = _synthetic_dir(str(tmp_path))
    ds = trainset.read_dataset_dir(str(tmp_path), 3, 2, mean, std)
    assert ds.planes.shape == (3, 2, 3, 20, 20) and ds.planes.dtype == np.float32
    for i, r in enumerate(raws):
        for c in range(2):
            for a in range(3):
                want = ((imtools.im2double(r[c, a]) - mean) / std).astype(np.float32)
                assert np.array_equal(ds.planes[i, c, a], want), (i, c, a)
        assert ds.annotations.dtype == np.uint8 and np.array_equal(ds.annotations[i], codes[i])
        if wts[i] is None:
            assert ds.weight_maps[i] is None
        else:
            assert np.array_equal(ds.weight_maps[i], wts[i])
    # the page order is aug + pages * channel: swapping the counts must fail or read other planes
    with pytest.raises(ValueError):
        trainset.read_dataset_dir(str(tmp_path), 2, 2, mean, std)


def test_eight_distinct_dihedral_transforms():
    g = np.arange(9).reshape(3, 3)
    imgs = [ref.transform(g, t) for t in range(8)]
    assert len({im.tobytes() for im in map(np.ascontiguousarray, imgs)}) == 8
    # the group of the square: every image is a rotation or a reflection of the grid
    group = [np.rot90(g, r) for r in range(4)] + [np.rot90(g.T, r) for r in range(4)]
    assert sorted(im.tobytes() for im in map(np.ascontiguousarray, imgs)) == sorted(im.tobytes() for im in map(np.ascontiguousarray, group))
    assert np.array_equal(imgs[4], g.T) and np.array_equal(imgs[2], g[::-1]) and np.array_equal(imgs[1], g[:, ::-1])


def test_restatement_labels_and_weights():
    S, P, K = 6, 4, 3
    planes = np.arange(S * S, dtype=np.float32).reshape(1, 1, 1, S, S)
    ann = np.zeros((1, S, S), np.uint8)
    ann[0, 0, 1], ann[0, 1, 0], ann[0, 2, 2], ann[0, 3, 3] = 1, 2, 3, 7   # 7 > K: no class
    wm = [np.full((S, S), 0.5, np.float32)]
    d = np.zeros(1, trainer.SAMPLE_DESC)
    d[0] = (0, 0, 0, 0, 0, 0.25, 2.0, 0)
    data, lab, w = ref.assemble(planes, ann, wm, d, P, K, (1, 2, 7), (0, 15, 0))
    assert data[0, 1, 1, 0] == np.float32(planes[0, 0, 0, 1, 1] * 2.0 + 0.25)
    assert lab[0, 0, 0].tolist() == [0, 0, 0]          # code 0
    assert lab[0, 3, 3].tolist() == [0, 0, 0]          # code above K
    assert lab[0, 0, 1].tolist() == [1, 0, 0] and lab[0, 1, 0].tolist() == [0, 1, 0] and lab[0, 2, 2].tolist() == [0, 0, 1]
    assert w[0, 0, 0].tolist() == [1.0, 2.0 + 15 * 0.5, 7.0]
    counts, loss = ref.class_counts(np.full((1, 2, 2, K), 1.0 / K, np.float32), lab[:, :2, :2])
    assert counts[1].tolist() == [1, 1, 0] and counts[0].tolist() == [1, 0, 0]   # first maximum: class 0
    assert loss == pytest.approx(2 * np.log(K))


def test_sampler_stream_epochs_bounds_and_legacy_defaults():
    kw = dict(n_samples=7, batch=3, size=40, P=16, n_pages=2, max_brightness=0.25, max_contrast=0.025, transforms=True)
    a, b = trainset.Sampler(5, **kw), trainset.Sampler(5, **kw)
    da = np.concatenate([a.next() for _ in range(14)])
    db = np.concatenate([b.next() for _ in range(14)])
    assert da.tobytes() == db.tobytes()
    assert trainset.Sampler(6, **kw).next().tobytes() != trainset.Sampler(5, **kw).next().tobytes()
    idx = da["index"]
    for e in range(len(idx) // 7):
        assert sorted(idx[7 * e:7 * e + 7]) == list(range(7))
    assert (da["y0"] >= 0).all() and (da["y0"] <= 24).all() and (da["x0"] >= 0).all() and (da["x0"] <= 24).all()
    assert set(da["transform"]) <= set(range(8)) and len(set(da["transform"])) > 1
    assert (da["page"] >= 0).all() and (da["page"] < 2).all() and (da["reserved"] == 0).all()
    assert (np.abs(da["brightness"]) <= 0.25).all() and (np.abs(da["contrast"] - 1) <= 0.025).all()
    assert (da["brightness"] < 0).any() and (da["brightness"] > 0).any()
    mb, mc = trainset.default_jitter("legacy", 0.25)
    leg = trainset.Sampler(1, 7, 4, 40, 16, 1, mb, mc)
    dl = np.concatenate([leg.next() for _ in range(5)])
    assert (dl["brightness"] == 0).all() and not np.signbit(dl["brightness"]).any() and (dl["contrast"] == 1).all()
    assert (dl["transform"] == 0).all()
    assert trainset.default_jitter("solo", 0.25) == (0.25, 0.025)
    v = leg.validation_descriptors()
    assert len(v) == 7 * 9 and set(v["y0"]) == {0, 16, 24} and (v["contrast"] == 1).all() and (v["brightness"] == 0).all()
    assert sorted(set(v["index"])) == list(range(7))


def test_graph_defaults():
    assert trainset.LABEL_WEIGHTS["solo"] == trainset.LabelWeights(True, (1, 2, 7), (0, 15, 0))
    assert trainset.LABEL_WEIGHTS["duo"] == trainset.LabelWeights(True, (1, 2, 5), (0, 10, 0))
    assert not trainset.LABEL_WEIGHTS["legacy"].weighted
    assert trainset.graph_kind(model.KNOWN_HP["nucleiDAPI"]) == "legacy"
    assert trainset.graph_kind(model.KNOWN_HP["nucleiDAPI1-5"]) == "solo"
    assert trainset.graph_kind(model.KNOWN_HP["nucleiDAPILAMIN"]) == "duo"


def test_c_layout_of_descriptor_and_label_weights(tmp_path):
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "umx_train.h"\nint main(void) {\n'
                   '  printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu\\n", sizeof(umx_sample_desc), offsetof(umx_sample_desc, transform),\n'
                   '         offsetof(umx_sample_desc, brightness), offsetof(umx_sample_desc, reserved), sizeof(umx_label_weights),\n'
                   '         offsetof(umx_label_weights, class_weight), offsetof(umx_label_weights, intersect_weight),\n'
                   '         offsetof(umx_label_weights, reserved), sizeof(umx_sample_desc));\n  return 0;\n}\n')
    exe = str(tmp_path / "layout")
    subprocess.check_call(["cc", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe])
    got = [int(v) for v in subprocess.check_output([exe]).split()]
    D, L = trainer.SAMPLE_DESC, trainer.LabelWeightsC
    assert got[0] == 32 == D.itemsize
    assert got[1:4] == [D.fields["transform"][1], D.fields["brightness"][1], D.fields["reserved"][1]]
    assert got[4] == ctypes.sizeof(L)
    assert got[5:8] == [L.class_weight.offset, L.intersect_weight.offset, L.reserved.offset]


def _cli(args, env_extra=None):
    env = dict(os.environ)
    env.update(env_extra or {})
    return subprocess.run([sys.executable, "-m", "unmicst_amd.finetune"] + args, cwd=ROOT, capture_output=True, text=True, timeout=300,
                          env=env)


def test_finetune_refuses_before_the_device(tmp_path):
    hp, blob, mean, std = helpers.load_nuclei_dapi()
    mdir = tmp_path / "m"
    model.save_converted(model.ModelArtefacts(hp, blob, mean, std), str(mdir))
    raws, codes, wts = ref.sample_105_crops(ref.VALID_ORIGINS[:2], S=128)
    good = str(tmp_path / "good")
    ref.write_dataset(good, raws, codes, wts)
    empty = tmp_path / "empty"
    empty.mkdir()
    small = str(tmp_path / "small")
    ref.write_dataset(small, raws[:, :64, :64], codes[:, :64, :64])
    two = str(tmp_path / "two")
    ref.write_dataset(two, [np.stack([r[None], r[None]]) for r in raws], codes)   # 2 channels, 1 page
    hp_only = tmp_path / "hp_only"
    hp_only.mkdir()
    h = model.KNOWN_HP["nucleiDAPILAMIN"]
    np.savez(str(hp_only / model.HP_ONLY_NAME), hp=model._hp_vector(h), mean=np.float64(0.1), std=np.float64(0.2))
    out = str(tmp_path / "out")
    cases = [
        (["--model", str(mdir), "--train", str(tmp_path / "missing"), "--valid", good], "no such directory"),
        (["--model", str(mdir), "--train", good, "--valid", str(empty)], "holds no"),
        (["--model", str(tmp_path / "nomodel"), "--train", good, "--valid", good], "no such directory"),
        (["--model", str(hp_only), "--train", good, "--valid", good], "no weights"),
        (["--model", str(mdir), "--train", small, "--valid", good], "smaller than"),
        (["--model", str(mdir), "--train", two, "--valid", good], "channel"),
    ]
    for args, msg in cases:
        # (every refusal comes before the trainer is created: none of them is the missing-device error)
        r = _cli(args + ["--out", out])
        assert r.returncode == 2, (args, r.stdout, r.stderr)
        assert msg in r.stderr, (args, r.stderr)
        assert not os.path.exists(out)
    ns = finetune.build_parser().parse_args(["--model", str(mdir), "--train", good, "--valid", good, "--out", out])
    art, tr_ds, va_ds = finetune.prepare(ns)
    assert art.hp == hp and tr_ds.planes.shape == (2, 1, 1, 128, 128)
    assert np.array_equal(tr_ds.planes[1, 0, 0], ref.normalise(raws[1], mean, std))
