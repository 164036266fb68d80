"""Host checks of the rotation / zoom augmentation (include/umx_train.h umx_warp_desc): the numpy restatement
(tests/trainset_warp_ref.py) against scipy, the two matrices that are dihedral transforms, the mirror fold, the sampler's extra
draws, the host validation of umx_warp_desc and the finetune command's new flags."""
import ctypes

import numpy as np
import pytest

import trainset_ref as ref
import trainset_warp_ref as wref
from unmicst_amd import finetune, trainer, trainset

ERR_INVALID = 1
SIZES = ((64, 64), (96, 64), (40, 32))                   # (S, P)
ANGLES = (7.0, 30.0, 133.7, -171.0)
ZOOMS = (0.6, 0.8, 1.0, 1.25, 1.7)


def test_warp_matrix():
    assert trainer.WARP_DESC.itemsize == 16
    m = trainset.warp_matrix(0.0, 1.0)
    assert m.dtype == np.float32 and m.tobytes() == np.array([1, 0, 0, 1], np.float32).tobytes()      # (no -0.0 either)
    assert wref.is_identity(m) and not wref.is_identity(trainset.warp_matrix(0.0, 1.25))
    for angle, zoom in ((30.0, 1.0), (133.7, 1.7), (-171.0, 0.6)):
        m = trainset.warp_matrix(angle, zoom)
        t = np.deg2rad(angle)
        want = np.array([np.cos(t), -np.sin(t), np.sin(t), np.cos(t)]) / zoom
        assert m.tobytes() == want.astype(np.float32).tobytes()
        assert abs(float(m[0]) * m[3] - float(m[1]) * m[2] - 1.0 / zoom ** 2) < 1e-6
    for bad in ((float("nan"), 1.0), (0.0, 0.0), (0.0, -1.0), (0.0, float("inf"))):
        with pytest.raises(ValueError):
            trainset.warp_matrix(*bad)


def test_restatement_against_scipy():
    """Data: the restatement rounds once to float32 (2^-24 max|p|) on top of float64 noise; the bound leaves a factor 2 over that:
    2^-23 max|p|.  Labels: equal on every pixel -- these inputs have no source coordinate within 1e-9 of a rounding tie, asserted."""
    import scipy.ndimage as ndi
    rng = np.random.default_rng(17)
    pixels = 0
    for S, P in SIZES:
        p = rng.normal(0, 3, (S, S)).astype(np.float32)
        code = rng.integers(0, 5, (S, S)).astype(np.uint8)
        unit = 2.0 ** -24 * float(np.abs(p).max())
        y0 = x0 = (S - P) // 2                           # the centred crop
        c = (P - 1) / 2.0
        g = np.arange(P, dtype=np.float64) - c
        for angle in ANGLES:
            for zoom in ZOOMS:
                m = trainset.warp_matrix(angle, zoom)
                m64 = m.astype(np.float64)
                sy = m64[0] * g[:, None] + m64[1] * g[None, :] + (y0 + c)
                sx = m64[2] * g[:, None] + m64[3] * g[None, :] + (x0 + c)
                ty, tx = wref.source(m, np.arange(P), np.arange(P), P, y0, x0, S)
                for t in (ty, tx):
                    assert t.min() >= 0.0 and t.max() <= S - 1
                    assert np.abs((t - np.floor(t)) - 0.5).min() > 1e-9, (S, P, angle, zoom)
                got = wref.warp_plane(p, m, P, y0, x0)
                want = ndi.map_coordinates(p.astype(np.float64), [sy, sx], order=1, mode="mirror")
                err = float(np.abs(got.astype(np.float64) - want).max()) / unit
                print("S %d P %d angle %g zoom %g: data within %.3f units of 2^-24 max|p|" % (S, P, angle, zoom, err))
                assert got.dtype == np.float32 and err <= 2.0, (S, P, angle, zoom, err)
                lab = wref.warp_nearest(code, m, P, y0, x0)
                want_lab = ndi.map_coordinates(code, [sy, sx], order=0, mode="mirror")
                assert lab.dtype == np.uint8 and np.array_equal(lab, want_lab), (S, P, angle, zoom, int((lab != want_lab).sum()))
                pixels += lab.size
    assert pixels == 184320


def _set(S, N=2, C=2, pages=2, K=3, seed=4):
    rng = np.random.default_rng(seed)
    planes = rng.normal(0, 2, (N, C, pages, S, S)).astype(np.float32)
    ann = rng.integers(0, K + 2, (N, S, S)).astype(np.uint8)
    wmaps = [rng.random((S, S)).astype(np.float32) * 2 for _ in range(N)]
    return planes, ann, wmaps


def _descs(rows):
    d = np.zeros(len(rows), trainer.SAMPLE_DESC)
    for j, r in enumerate(rows):
        d[j] = tuple(r) + (0,)
    return d


def _warps(ms):
    w = np.zeros(len(ms), trainer.WARP_DESC)
    for j, m in enumerate(ms):
        w["m"][j] = m
    return w


def _same_bits(got, want, what):
    for k, (g, w) in enumerate(zip(got, want)):
        assert g.dtype == np.float32 and g.shape == w.shape and g.tobytes() == w.tobytes(), (what, ("data", "labels", "weights")[k])


# out[y][x] = crop[P-1-x][y] is "swap the axes, then flip the columns" (transform 5); out[y][x] = crop[P-1-y][P-1-x] is both flips (3)
QUARTER_TURNS = (((0.0, -1.0, 1.0, 0.0), 5), ((-1.0, 0.0, 0.0, -1.0), 3))


@pytest.mark.parametrize("S,P", [(40, 16), (32, 32), (21, 15)])
def test_quarter_turn_matrices_are_dihedral_transforms(S, P):
    """Coordinates are exact there and f = 0: data, labels and weights equal the plain crop under the matching transform bit for bit."""
    planes, ann, wmaps = _set(S)
    cw, iw = (1.0, 2.0, 7.0), (0.0, 15.0, 0.25)
    far = S - P
    for m, code in QUARTER_TURNS:
        rows = [(j % 2, j % 2, (0, far, far // 2)[j % 3], (far, 0, far // 3)[j % 3], 0, 0.25 - 0.125 * j, 1.0 + 0.03 * j) for j in range(4)]
        plain = _descs([r[:4] + (code,) + r[5:] for r in rows])
        got = wref.assemble_warped(planes, ann, wmaps, _descs(rows), None, _warps([m] * 4), None, P, 3, cw, iw)
        _same_bits(got, ref.assemble(planes, ann, wmaps, plain, P, 3, cw, iw), (m, S, P))
    # and an identity row is the plain row
    d = _descs(rows)
    _same_bits(wref.assemble_warped(planes, ann, wmaps, d, None, _warps([(1, 0, 0, 1)] * 4), None, P, 3, cw, iw),
               ref.assemble(planes, ann, wmaps, d, P, 3, cw, iw), "identity")


def test_mirror_fold():
    for S in (2, 5, 16):
        T = 2 * (S - 1)
        k = np.arange(-5 * T - 3, 5 * T + 4)             # several periods on both sides
        want = np.where((k % T) <= S - 1, k % T, T - (k % T))
        got = wref.fold(k.astype(np.float64), S)
        assert got.dtype == np.float64 and np.array_equal(got, want.astype(np.float64)), S
        frac = wref.fold(k + 0.25, S)                    # between the pixels: the same triangle wave
        tri = np.where(((k + 0.25) % T) <= S - 1, (k + 0.25) % T, T - ((k + 0.25) % T))
        assert np.array_equal(frac, tri) and frac.min() >= 0 and frac.max() <= S - 1
    assert wref.fold(np.float64(-1e-300), 9) == 0.0 and wref.fold(np.nextafter(16.0, 0.0), 9) >= 0.0
    # S = 2: a plane of two pixels per axis, read far outside; S = P: the whole sample is the crop, every halo pixel is mirrored
    p2 = np.array([[1.0, 2.0], [3.0, 5.0]], np.float32)
    ty, tx = wref.source((1, 0, 0, 1), np.arange(-9, 11), np.arange(-9, 11), 2, 0, 0, 2)
    v = wref.bilinear(p2, ty, tx)
    assert v.shape == (20, 20) and v.min() >= 1.0 and v.max() <= 5.0
    assert v[9, 9] == 1.0 and v[10, 9] == 3.0 and v[11, 9] == 1.0 and v[8, 9] == 3.0    # rows ... 3 1 | 1 3 | 1 3 ...: period 2
    S = P = 16
    p = np.random.default_rng(2).normal(size=(S, S)).astype(np.float32)
    halo = wref.warp_plane(p, (1.0, 0.0, 0.0, 1.0), P, 0, 0, halo=12)                     # the identity matrix through the warp code
    assert np.array_equal(halo, np.pad(p, 12, mode="reflect"))
    rot = wref.warp_plane(p, trainset.warp_matrix(45.0, 0.5), P, 0, 0, halo=12)           # corners reach 1.4 * 2 * 20 pixels out
    assert np.isfinite(rot).all() and rot.min() >= p.min() and rot.max() <= p.max()


def _today(seed, n_samples, batch, size, P, n_pages, mb, mc, transforms, aug=None, warp=None, batches=1):
    """The documented draw order, restated: per epoch a permutation; per image page, y0, x0, transform (when enabled), brightness sign
    and magnitude, contrast sign and magnitude; then (blur / saturation on) blur coin, level, saturation coin, gain; then (warp on)
    rotation coin, angle, zoom coin, zoom."""
    r = np.random.Generator(np.random.PCG64(seed))
    perm, pos = r.permutation(n_samples), 0
    out = []
    for _ in range(batches):
        d = np.zeros(batch, trainer.SAMPLE_DESC)
        a = np.zeros(batch, trainer.AUGMENT_DESC)
        a["gain"] = 1.0
        coins = []
        for j in range(batch):
            if pos == n_samples:
                perm, pos = r.permutation(n_samples), 0
            d["index"][j] = perm[pos]
            pos += 1
            d["page"][j] = r.integers(n_pages)
            d["y0"][j] = r.integers(size - P + 1)
            d["x0"][j] = r.integers(size - P + 1)
            d["transform"][j] = r.integers(8) if transforms else 0
            sb = -1.0 if r.random() < 0.5 else 1.0
            d["brightness"][j] = mb * sb * r.random() + 0.0
            sc = -1.0 if r.random() < 0.5 else 1.0
            d["contrast"][j] = 1.0 + mc * sc * r.random()
            if aug:
                levels, bp, sp, mg = aug
                blur, level, sat, gain = r.random() < bp, 1 + int(r.integers(max(levels - 1, 1))), r.random() < sp, 1.0 + (mg - 1.0) * r.random()
                a[j] = (level if blur else 0, gain if sat else 1.0)
            if warp:
                rp, zp, (lo, hi) = warp
                coins.append((r.random() < rp, 360.0 * r.random(), r.random() < zp, lo * (hi / lo) ** r.random()))
        out.append((d, a, coins))
    return out


def test_sampler_keeps_its_stream_and_draws_the_warp():
    kw = dict(n_samples=7, batch=4, size=40, P=16, n_pages=2, max_brightness=0.25, max_contrast=0.025, transforms=True)
    pos = (7, 4, 40, 16, 2, 0.25, 0.025, True)
    augkw = dict(blur_levels=4, blur_prob=0.4, saturate_prob=0.25, max_gain=3.0)
    steps = 8
    for seed in (0, 5, 123456789):
        # warp off: the streams of next_augmented() as they are without the feature, with and without blur / saturation
        for akw, atup in ((dict(), None), (augkw, (4, 0.4, 0.25, 3.0))):
            want = _today(seed, *pos, aug=atup, batches=steps)
            s1 = trainset.Sampler(seed, **kw, **akw)
            s2 = trainset.Sampler(seed, **kw, **akw, rotate_prob=0.0, zoom_prob=0.0, zoom_range=(0.8, 1.25))
            s3 = trainset.Sampler(seed, **kw, **akw)
            for d, a, _ in want:
                d1, a1 = s1.next_augmented()
                d2, a2, w2 = s2.next_warped()
                assert d1.tobytes() == d2.tobytes() == d.tobytes() == s3.next().tobytes()
                assert a1.tobytes() == a2.tobytes() == a.tobytes()
                assert w2.dtype == trainer.WARP_DESC and w2.tobytes() == np.array([[1, 0, 0, 1]] * 4, np.float32).tobytes()
        # warp on: the four draws follow the gain draw (blur / saturation on) or the contrast draw (off)
        for akw, atup in ((dict(), None), (augkw, (4, 0.4, 0.25, 3.0))):
            wkw = dict(rotate_prob=0.5, zoom_prob=0.5, zoom_range=(0.8, 1.25))
            want = _today(seed, *pos, aug=atup, warp=(0.5, 0.5, (0.8, 1.25)), batches=steps)
            s = trainset.Sampler(seed, **kw, **akw, **wkw)
            for d, a, coins in want:
                d1, a1, w1 = s.next_warped()
                assert d1.tobytes() == d.tobytes() and a1.tobytes() == a.tobytes()
                for j, (rot, angle, zoomed, zoom) in enumerate(coins):
                    assert 0.8 <= zoom < 1.25 and 0.0 <= angle < 360.0
                    assert w1["m"][j].tobytes() == trainset.warp_matrix(angle if rot else 0.0, zoom if zoomed else 1.0).tobytes()
    # one image's coins do not shift the next image's draws: with other probabilities the descriptors are the same, and wherever
    # the first run both rotates and zooms an image it uses the angle and the zoom of the run that always does both
    a, b = (trainset.Sampler(3, **kw, rotate_prob=pr, zoom_prob=pz, zoom_range=(0.5, 2.0)) for pr, pz in ((0.5, 0.6), (1.0, 1.0)))
    both = none = 0
    for _ in range(50):
        (da, _, wa), (db, _, wb) = a.next_warped(), b.next_warped()
        assert da.tobytes() == db.tobytes()
        for ma, mb in zip(wa["m"], wb["m"]):
            rotated, zoomed = ma[1] != 0, abs(float(ma[0]) * ma[3] - float(ma[1]) * ma[2] - 1.0) > 1e-4
            if rotated and zoomed:
                assert ma.tobytes() == mb.tobytes()
                both += 1
            none += wref.is_identity(ma)
    assert both > 30 and none > 15, (both, none)
    for bad in (dict(rotate_prob=1.5), dict(zoom_prob=-0.1), dict(zoom_range=(0.4, 1.0)), dict(zoom_range=(1.0, 2.5)),
                dict(zoom_range=(1.1, 1.2)), dict(zoom_range=(0.8, 0.9)), dict(zoom_range=(float("nan"), 1.0)), dict(rotate_prob=float("nan"))):
        with pytest.raises(ValueError):
            trainset.Sampler(1, **kw, **bad)


def _check(ms):
    from unmicst_amd import build, umx
    build.build()
    L = trainer._bind(umx.load())
    w = _warps(ms)
    msg = ctypes.create_string_buffer(256)
    rc = L.umx_warp_desc_check(w.ctypes.data, len(w), msg, len(msg))
    return rc, msg.value.decode()


def test_warp_desc_check():
    good = [(1, 0, 0, 1), tuple(trainset.warp_matrix(133.7, 0.5)), (0, -1, 1, 0), (-1, 0, 0, -1), (4, 0, 0, -4), (0.25, 0, 0, 0.25)]
    assert _check(good) == (0, "")
    assert np.abs(trainset.warp_matrix(45.0, 0.5)).max() <= 2.0      # what the sampler can draw stays far inside the bound
    nan, inf = float("nan"), float("inf")
    for k, (m, rule) in enumerate([((nan, 0, 0, 1), "finite"), ((1, 0, inf, 1), "finite"), ((1, 0, 0, -inf), "finite"),
                                   ((4.5, 0, 0, 1), "above 4"), ((1, -4.0000005, 0, 1), "above 4"), ((0, 0, 0, 0), "singular"),
                                   ((1, 2, 2, 4), "singular"), ((1, 0, 0, 0), "singular")]):
        at = k % len(good)
        rc, msg = _check(good[:at] + [m] + good[at:])
        assert rc == ERR_INVALID and rule in msg and ("warp %d " % at) in msg, (m, rc, msg)
    from unmicst_amd import umx
    L = trainer._bind(umx.load())
    assert L.umx_warp_desc_check(None, 1, None, 0) == ERR_INVALID
    bad = _warps([(nan, 0, 0, 1)])
    assert L.umx_warp_desc_check(bad.ctypes.data, 1, None, 0) == ERR_INVALID            # msg may be NULL


def test_finetune_warp_flags_parse_and_refuse():
    base = ["--model", "no-such-model", "--train", "t", "--valid", "v", "--out", "o"]
    parse = finetune.build_parser().parse_args
    assert finetune.warp_settings(parse(base)) is None
    assert finetune.warp_settings(parse(base + ["--blur-sigmas", "1"])) is None
    assert finetune.augment_settings(parse(base + ["--rotate-prob", "1"])) is None
    ns = parse(base + ["--rotate-prob", "1", "--zoom-range", "0.8,1.25"])
    assert finetune.warp_settings(ns) == {"rotate_prob": 1.0, "zoom_prob": 0.5, "zoom_range": [0.8, 1.25]}
    assert finetune.warp_settings(parse(base + ["--rotate-prob", "0.25"])) == {"rotate_prob": 0.25, "zoom_prob": 0.0, "zoom_range": [1.0, 1.0]}
    assert finetune.warp_settings(parse(base + ["--zoom-range", "0.5,2", "--zoom-prob", "1"])) == {"rotate_prob": 0.0, "zoom_prob": 1.0,
                                                                                                 "zoom_range": [0.5, 2.0]}
    bad = [["--rotate-prob", "1.5"], ["--rotate-prob", "nan"], ["--rotate-prob", "-0.1"], ["--zoom-prob", "0.5"],
           ["--zoom-range", "0.8"], ["--zoom-range", "0.8,1,1.25"], ["--zoom-range", "a,b"], ["--zoom-range", ""],
           ["--zoom-range", "0.4,1.25"], ["--zoom-range", "0.8,2.5"], ["--zoom-range", "1.1,1.25"], ["--zoom-range", "0.8,0.9"],
           ["--zoom-range", "nan,1.25"], ["--zoom-range", "0.8,1.25", "--zoom-prob", "2"]]
    for extra in bad:
        with pytest.raises(finetune.Refusal):
            finetune.warp_settings(parse(base + extra))
        with pytest.raises(finetune.Refusal) as e:       # prepare refuses them before it looks at the model or the sets
            finetune.prepare(parse(base + extra))
        assert "no such directory" not in str(e.value), extra
    with pytest.raises(finetune.Refusal) as e:
        finetune.prepare(parse(base + ["--rotate-prob", "1"]))
    assert "no such directory" in str(e.value)
