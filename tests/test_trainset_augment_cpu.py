"""Host checks of the computed defocus / saturation augmentation: the Gaussian taps, the numpy restatement
of assemble_augmented_kernel (tests/trainset_augment_ref.py) against scipy, the saturation recipe, the sampler's extra draws, the
host validation of umx_augment_table and the finetune command's new flags."""
import ctypes
import math

import numpy as np
import pytest

import trainset_augment_ref as aref
from unmicst_amd import finetune, trainer, trainset

SIGMAS = (0.5, 0.75, 1.0, 1.5, 2.0, 3.0, 4.0)
ERR_INVALID = 1


def test_gaussian_taps_radius_symmetry_and_sum():
    for sigma in SIGMAS + (0.2, 0.3, 2.5, 3.99):
        w = trainset.gaussian_taps(sigma)
        R = int(3.0 * sigma + 0.5)
        assert w.dtype == np.float32 and w.shape == (R + 1,)
        t = np.arange(-R, R + 1, dtype=np.float64)
        full = np.exp(-0.5 * (t / sigma) ** 2)
        full /= full.sum()
        for k in range(R + 1):   # one-sided taps: both halves of the float64 kernel round to them
            assert w[k] == np.float32(full[R + k]) == np.float32(full[R - k])
        assert (np.diff(w) < 0).all() and (w > 0).all()
        total = float(w[0].astype(np.float64) + 2 * w[1:].astype(np.float64).sum())
        assert abs(total - 1.0) <= (2 * R + 1) * 2.0 ** -24, (sigma, total)
    assert len(trainset.gaussian_taps(4.0)) == 13
    for bad in (0.0, -1.0, float("nan"), float("inf"), 4.2):
        with pytest.raises(ValueError):
            trainset.gaussian_taps(bad)
    tab = trainset.AugmentTable.from_sigmas([0.75, 1.5, 3], 0.25, 0.125)
    assert tab.n_levels == 4 and tab.radius == (0, 2, 5, 9)
    c = tab.c_struct()
    assert c.n_levels == 4 and list(c.radius)[:5] == [0, 2, 5, 9, 0] and c.taps[3][9] == tab.taps[3][9] and c.taps[3][10] == 0
    with pytest.raises(ValueError):
        trainset.AugmentTable.from_sigmas([1.0] * 16, 0.0, 1.0)


@pytest.mark.parametrize("kind", ["image_like", "normal_0_5"])
def test_restatement_against_scipy(kind):
    """Bound: per pass one float32 rounding of each tap and one of the stored result, weights summing to 1 -> 2 units of 2^-24 max|p|
    per pass, 4 for both."""
    import scipy.ndimage as ndi
    rng = np.random.default_rng(3)
    S = 97
    if kind == "image_like":   # a normalised microscope-like plane: smooth blobs + noise, (x - mean) / std
        yy, xx = np.mgrid[:S, :S]
        img = sum(np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2.0 * r * r)) for cy, cx, r in rng.uniform(3, S - 3, (12, 3)) / (1, 1, 12))
        p = ((np.clip(0.1 + 0.5 * img + rng.normal(0, 0.02, (S, S)), 0, 1) - 0.2) / 0.15).astype(np.float32)
    else:
        p = rng.normal(0, 5, (S, S)).astype(np.float32)
    unit = 2.0 ** -24 * float(np.abs(p).max())
    for sigma in SIGMAS:
        got = aref.blur_plane(p, trainset.gaussian_taps(sigma))
        want = ndi.gaussian_filter(p.astype(np.float64), sigma, mode="nearest", truncate=3.0)
        err = float(np.abs(got.astype(np.float64) - want).max())
        print("%s sigma %g: max difference %.3f units of 2^-24 max|p|" % (kind, sigma, err / unit))
        assert got.dtype == np.float32 and err <= 4 * unit, (kind, sigma, err / unit)


def test_blur_replicates_the_edge_and_keeps_a_constant():
    w = trainset.gaussian_taps(1.0)
    p = np.zeros((9, 9), np.float32)
    p[:, 0] = 1.0                                        # the first column is replicated to the left
    h = aref._pass(p, w, 1)
    wf = np.concatenate([w[:0:-1], w]).astype(np.float64)
    assert h[4, 0] == np.float32(wf[:4].sum()) or abs(h[4, 0] - wf[:4].sum()) < 1e-6
    assert h[4, 3] == np.float32(w[3]) and h[4, 4] == 0
    c = np.full((7, 7), 3.0, np.float32)
    assert np.abs(aref.blur_plane(c, w) - 3.0).max() <= 4 * 2.0 ** -24 * 3.0


def test_saturation_recipe():
    mean, std = np.float32(0.2), np.float32(0.15)
    rng = np.random.default_rng(5)
    raw = rng.random(4000)
    b = ((raw - np.float64(mean)) / np.float64(std)).astype(np.float32)
    same = aref.saturate(b, 1.0, mean, std)
    assert same.tobytes() == b.tobytes()
    ceiling = np.float32((1.0 - np.float64(mean)) / np.float64(std))
    prev = None
    for g in (1.25, 1.5, 2.0, 4.0):
        s = aref.saturate(b, g, mean, std)
        r = b.astype(np.float64) * np.float64(std) + np.float64(mean)
        clipped = r * np.float64(np.float32(g)) >= 1.0
        assert clipped.any() and not clipped.all()
        assert (s[clipped] == ceiling).all() and (s[~clipped] <= ceiling).all()
        assert (s >= b - 1e-5).all()                    # a gain >= 1 never darkens (up to the rounding of the round trip)
        if prev is not None:
            assert (s >= prev).all()                    # monotone in the gain
        prev = s
    assert (aref.saturate(b, 1e6, mean, std)[raw > 1e-3] == ceiling).all()


def test_sampler_keeps_its_stream_and_draws_the_extras():
    kw = dict(n_samples=7, batch=4, size=40, P=16, n_pages=2, max_brightness=0.25, max_contrast=0.025, transforms=True)
    off = dict(blur_levels=4, blur_prob=0.0, saturate_prob=0.0, max_gain=3.0)
    steps = 3 * 7 // 4 + 2                               # more than 3 epochs
    a, b, c = trainset.Sampler(5, **kw), trainset.Sampler(5, **kw, **off), trainset.Sampler(5, **kw, **off)
    for _ in range(steps):
        da, db = a.next(), b.next()
        dc, ac = c.next_augmented()
        assert da.tobytes() == db.tobytes() == dc.tobytes()
        assert ac.dtype == trainer.AUGMENT_DESC and (ac["blur_level"] == 0).all() and (ac["gain"] == 1.0).all()
    assert a.epoch >= 3
    on = dict(blur_levels=4, blur_prob=0.4, saturate_prob=0.25, max_gain=3.0)
    s1, s2 = trainset.Sampler(9, **kw, **on), trainset.Sampler(9, **kw, **on)
    n = 2000
    descs, augs = [], []
    for _ in range(n // 4):
        d1, a1 = s1.next_augmented()
        d2, a2 = s2.next_augmented()
        assert d1.tobytes() == d2.tobytes() and a1.tobytes() == a2.tobytes()
        descs.append(d1)
        augs.append(a1)
    d, g = np.concatenate(descs), np.concatenate(augs)
    assert len(g) == n and (d["reserved"] == 0).all()
    assert set(g["blur_level"]) == {0, 1, 2, 3}
    assert (g["gain"] >= 1.0).all() and (g["gain"] < 3.0).all() and np.isfinite(g["gain"]).all()

    def near(count, p):
        sd = math.sqrt(n * p * (1 - p))
        assert abs(count - n * p) <= 4 * sd, (count, n * p, sd)
    near(int((g["blur_level"] != 0).sum()), 0.4)
    near(int((g["gain"] != 1.0).sum()), 0.25)
    for level in (1, 2, 3):
        near(int((g["blur_level"] == level).sum()), 0.4 / 3)
    sat = g["gain"][g["gain"] != 1.0]
    assert sat.min() < 1.2 and sat.max() > 2.8 and abs(sat.mean() - 2.0) < 0.1       # uniform over [1, 3)
    # the coins are independent of each other and of what the descriptor half drew
    both = int(((g["blur_level"] != 0) & (g["gain"] != 1.0)).sum())
    near(both, 0.4 * 0.25)
    for bad in (dict(blur_prob=1.5), dict(saturate_prob=-0.1), dict(max_gain=0.5), dict(max_gain=float("nan")),
                dict(blur_levels=1, blur_prob=0.5), dict(blur_levels=17)):
        with pytest.raises(ValueError):
            trainset.Sampler(1, **kw, **bad)


def _check(table):
    from unmicst_amd import build, umx
    build.build()
    L = trainer._bind(umx.load())
    msg = ctypes.create_string_buffer(256)
    rc = L.umx_augment_table_check(ctypes.byref(table), msg, len(msg))
    return rc, msg.value.decode()


def test_augment_table_check():
    good = trainset.AugmentTable.from_sigmas([0.75, 1.5, 4.0], 0.2, 0.15)
    assert ctypes.sizeof(trainer.AugmentTableC) == 12 + 64 + 16 * 13 * 4 + 20 and trainer.AUGMENT_DESC.itemsize == 8
    assert _check(good.c_struct()) == (0, "")
    assert _check(trainset.AugmentTable.from_sigmas([], 0.0, 1.0).c_struct()) == (0, "")

    def broken(edit):
        t = good.c_struct()
        edit(t)
        return t
    cases = [
        (lambda t: setattr(t, "n_levels", 0), "n_levels"),
        (lambda t: setattr(t, "n_levels", 17), "n_levels"),
        (lambda t: t.radius.__setitem__(0, 1), "level 0"),
        (lambda t: t.radius.__setitem__(2, 13), "radius of level 2"),
        (lambda t: t.radius.__setitem__(1, -1), "radius of level 1"),
        (lambda t: t.taps[3].__setitem__(5, float("nan")), "tap 5 of level 3"),
        (lambda t: t.taps[1].__setitem__(0, float("inf")), "tap 0 of level 1"),
        (lambda t: t.taps[2].__setitem__(1, -0.25), "tap 1 of level 2"),
        (lambda t: setattr(t, "std", 0.0), "std"),
        (lambda t: setattr(t, "std", float("nan")), "std"),
        (lambda t: setattr(t, "mean", float("inf")), "mean"),
        (lambda t: t.reserved.__setitem__(4, 1), "reserved"),
    ]
    for edit, rule in cases:
        rc, msg = _check(broken(edit))
        assert rc == ERR_INVALID and rule in msg, (rule, rc, msg)
    # a tap beyond a level's radius, or a level beyond n_levels, is not read
    assert _check(broken(lambda t: t.taps[1].__setitem__(12, float("nan")))) == (0, "")
    assert _check(broken(lambda t: t.radius.__setitem__(9, 99))) == (0, "")


def test_finetune_flags_parse_and_refuse():
    base = ["--model", "no-such-model", "--train", "t", "--valid", "v", "--out", "o"]
    parse = finetune.build_parser().parse_args
    assert finetune.augment_settings(parse(base)) is None
    ns = parse(base + ["--blur-sigmas", "0.75,1.5,3", "--blur-prob", "0.5", "--saturate-prob", "0.25", "--max-gain", "2"])
    assert finetune.augment_settings(ns) == {"blur_sigmas": [0.75, 1.5, 3.0], "blur_prob": 0.5, "saturate_prob": 0.25, "max_gain": 2.0}
    assert finetune.augment_settings(parse(base + ["--blur-sigmas", "1"])) == {"blur_sigmas": [1.0], "blur_prob": 0.5,
                                                                              "saturate_prob": 0.0, "max_gain": 1.0}
    assert finetune.augment_settings(parse(base + ["--saturate-prob", "1"]))["max_gain"] == 2.0
    bad = [["--blur-sigmas", "1,x"], ["--blur-sigmas", ""], ["--blur-sigmas", "0"], ["--blur-sigmas", "4.5"], ["--blur-sigmas", "nan"],
           ["--blur-sigmas", ",".join(["1"] * 16)], ["--blur-prob", "0.5"], ["--blur-sigmas", "1", "--blur-prob", "1.5"],
           ["--blur-sigmas", "1", "--blur-prob", "nan"], ["--saturate-prob", "-0.5"], ["--saturate-prob", "0.5", "--max-gain", "0.9"],
           ["--max-gain", "inf"], ["--max-gain", "nan"]]
    for extra in bad:
        with pytest.raises(finetune.Refusal):
            finetune.augment_settings(parse(base + extra))
        with pytest.raises(finetune.Refusal) as e:       # prepare refuses them before it looks at the model or the sets
            finetune.prepare(parse(base + extra))
        assert "no such directory" not in str(e.value), extra
    with pytest.raises(finetune.Refusal) as e:
        finetune.prepare(parse(base + ["--blur-sigmas", "1"]))
    assert "no such directory" in str(e.value)
