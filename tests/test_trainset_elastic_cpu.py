"""Host checks of the elastic deformation (include/umx_train.h umx_elastic_desc): the numpy restatement
(tests/trainset_elastic_ref.py) against scipy's cubic spline and its linear / nearest resampling, the zero lattice, the host validation
of umx_elastic_desc, the sampler's extra draws and the finetune command's new flags."""
import ctypes

import numpy as np
import pytest

import trainset_elastic_ref as eref
import trainset_ref as ref
import trainset_warp_ref as wref
from unmicst_amd import finetune, trainer, trainset

ERR_INVALID = 1
CW, IW = (1.0, 2.0, 7.0), (0.0, 15.0, 0.25)


def _lattice(rng, n, sigma):
    return trainset.elastic_lattice(rng.standard_normal(2 * n * n), sigma, n)


def _scipy_displacement(d, n, ys, xs, P):
    """The same spline by scipy: the lattice is its own coefficient array (prefilter=False), lattice point 1 sits on pixel 0."""
    import scipy.ndimage as ndi
    scale = (n - 3) / (P - 1)
    uy = np.clip(np.asarray(ys, np.float64), 0, P - 1) * scale
    ux = np.clip(np.asarray(xs, np.float64), 0, P - 1) * scale
    co = [np.broadcast_to(uy[:, None] + 1.0, (len(ys), len(xs))), np.broadcast_to(ux[None, :] + 1.0, (len(ys), len(xs)))]
    return [ndi.map_coordinates(np.asarray(d[k], np.float64)[:n, :n], co, order=3, prefilter=False) for k in range(2)]


def test_displacement_against_scipy():
    """0a / 0b against scipy.ndimage.map_coordinates(order=3, prefilter=False) on the lattice: within 1e-13 max|D| (float64 noise of
    about 40 operations, with a few hundred times of room).  Seen here: 2.2e-16 max|D| at the worst of the 9 (n, P) pairs.  A zero
    lattice gives +0.0 everywhere, and |e| <= max|D|."""
    rng = np.random.default_rng(5)
    worst = 0.0
    for n in (4, 5, 6):
        for P in (32, 64, 128):
            d = _lattice(rng, n, 8.0)
            d[0, 0, 0], d[1, n - 1, n - 1] = 32.0, -32.0         # the bound of the descriptor
            g = np.arange(-12, P + 12)
            got = eref.displacement(d, n, g, g, P)
            want = _scipy_displacement(d, n, g, g, P)
            top = float(np.abs(d).max())
            for k in range(2):
                assert got[k].dtype == np.float64 and got[k].shape == (P + 24, P + 24)
                err = float(np.abs(got[k] - want[k]).max()) / top
                worst = max(worst, err)
                print("n %d P %d component %d: within %.3g max|D| of scipy" % (n, P, k, err))
                assert err <= 1e-13, (n, P, k, err)
                assert np.abs(got[k]).max() <= top
                # outside the crop: the displacement of the nearest crop-edge pixel
                assert np.array_equal(got[k][:12], np.broadcast_to(got[k][12], (12, P + 24)))
                assert np.array_equal(got[k][:, -12:], np.broadcast_to(got[k][:, -13:-12], (P + 24, 12)))
            W, i = eref.weights(g, P, n)
            assert i.min() == 0 and i.max() == n - 4 and W.min() >= 0.0 and np.abs(W.sum(axis=1) - 6.0).max() < 1e-14
            zero = eref.displacement(np.zeros((2, 6, 6), np.float32), n, g, g, P)
            for z in zero:
                assert not z.any() and not np.signbit(z).any()
    print("worst: %.3g max|D|" % worst)


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


def _elastics(lats):
    """lats: per image None (n = 0) or (n, d [2][6][6])."""
    e = np.zeros(len(lats), trainer.ELASTIC_DESC)
    for j, l in enumerate(lats):
        if l is not None:
            e["n"][j], e["d"][j] = l
    return e


def _same_bits(got, want, what):
    for k, (g, w) in enumerate(zip(got, want)):
        assert g.dtype == np.float32 and g.shape == w.shape and g.tobytes() == w.tobytes(), (what, ("data", "labels", "weights")[k])


@pytest.mark.parametrize("S,P", [(40, 16), (32, 32), (21, 15)])
def test_zero_lattice_is_the_warp_and_with_the_identity_the_plain_batch(S, P):
    planes, ann, wmaps = _set(S)
    table = trainset.AugmentTable.from_sigmas((0.75, 1.5), 0.2, 0.15)
    far = S - P
    rows = [(j % 2, j % 2, (0, far, far // 2)[j % 3], (far, 0, far // 3)[j % 3], j % 8, 0.25 - 0.125 * j, 1.0 + 0.03 * j) for j in range(6)]
    d = _descs(rows)
    a = np.zeros(6, trainer.AUGMENT_DESC)
    a["blur_level"], a["gain"] = (0, 1, 2, 0, 1, 2), (1.0, 1.0, 2.0, 3.0, 1.5, 1.0)
    w = _warps([trainset.warp_matrix(ang, z) for ang, z in ((30.0, 1.25), (0.0, 1.0), (133.7, 0.5), (-171.0, 2.0), (7.0, 1.0), (0.0, 0.8))])
    zero = np.zeros((2, 6, 6), np.float32)
    for n in (4, 5, 6):
        e = _elastics([(n, zero)] * 6)
        # an identity row of the warp entry is the unwarped path (the blur replicates the sample's edge there); through the lattice code
        # it is the warp code with the identity matrix (the blur's halo is mirrored): equal where there is no blur
        moved = [j for j in range(6) if not wref.is_identity(w["m"][j]) or a["blur_level"][j] == 0]
        got = eref.assemble_elastic(planes, ann, wmaps, d, a, w, e, table, P, 3, CW, IW)
        want = wref.assemble_warped(planes, ann, wmaps, d, a, w, table, P, 3, CW, IW)
        _same_bits([g[moved] for g in got], [v[moved] for v in want], ("warp", n, S, P))
        got = eref.assemble_elastic(planes, ann, wmaps, d, None, w, e, None, P, 3, CW, IW)
        _same_bits(got, wref.assemble_warped(planes, ann, wmaps, d, None, w, None, P, 3, CW, IW), ("warp, aug None", n, S, P))
        for wi in (None, _warps([(1, 0, 0, 1)] * 6)):
            got = eref.assemble_elastic(planes, ann, wmaps, d, None, wi, e, None, P, 3, CW, IW)
            _same_bits(got, ref.assemble(planes, ann, wmaps, d, P, 3, CW, IW), ("plain", n, S, P))
    # n == 0 rows are the warp reference's rows whatever the other rows carry
    rng = np.random.default_rng(1)
    mixed = _elastics([None if j % 2 else (5, _lattice(rng, 5, 2.0)) for j in range(6)])
    got = eref.assemble_elastic(planes, ann, wmaps, d, a, w, mixed, table, P, 3, CW, IW)
    want = wref.assemble_warped(planes, ann, wmaps, d, a, w, table, P, 3, CW, IW)
    _same_bits([g[1::2] for g in got], [v[1::2] for v in want], "n == 0 rows")
    assert all((g[0::2] != v[0::2]).any() for g, v in zip(got[:2], want[:2]))


# (S, P, seed): seeds for which no source coordinate lies within 1e-9 of a rounding tie (asserted below)
PIPELINE = ((64, 64, 11), (96, 64, 12), (40, 32, 13))


def test_restatement_against_scipy():
    """Data against map_coordinates(plane, displaced coordinates, order=1, mode="mirror"), the coordinates from scipy's own cubic spline
    on the lattice: the restatement rounds once to float32 (2^-24 max|p|) on top of float64 noise; the bound leaves a factor 2 over
    that, 2^-23 max|p|, as the warp's test does.  Labels equal order=0 on every pixel -- no source coordinate of these cases lies within
    1e-9 of a tie, asserted."""
    import scipy.ndimage as ndi
    pixels = 0
    for S, P, seed in PIPELINE:
        rng = np.random.default_rng(seed)
        p = rng.normal(0, 3, (S, S)).astype(np.float32)
        code = rng.integers(0, 5, (S, S)).astype(np.uint8)
        unit = 2.0 ** -24 * float(np.abs(p).max())
        y0 = x0 = (S - P) // 2
        c = (P - 1) / 2.0
        g = np.arange(P)
        for n in (4, 5, 6):
            for angle, zoom, sigma in ((0.0, 1.0, 2.0), (30.0, 1.25, 1.0), (133.7, 0.6, 3.0), (-171.0, 1.7, 0.5), (0.0, 1.0, 15.0)):
                m = trainset.warp_matrix(angle, zoom)
                m64 = m.astype(np.float64)
                d = _lattice(rng, n, sigma)
                ey, ex = _scipy_displacement(d, n, g, g, P)
                dy, dx = g[:, None] + ey - c, g[None, :] + ex - c
                sy = m64[0] * dy + m64[1] * dx + (y0 + c)
                sx = m64[2] * dy + m64[3] * dx + (x0 + c)
                ty, tx = eref.source(m, d, n, g, g, P, y0, x0, S)
                for t in (ty, tx):
                    assert t.min() >= 0.0 and t.max() <= S - 1
                    assert np.abs((t - np.floor(t)) - 0.5).min() > 1e-9, (S, P, n, angle, zoom, sigma)
                got = eref.deform_plane(p, m, d, n, P, y0, x0)
                want = ndi.map_coordinates(p.astype(np.float64), [sy, sx], order=1, mode="mirror")
                err = float(np.abs(got.astype(np.float64) - want).max()) / unit
                print("S %d P %d n %d angle %g zoom %g sigma %g: data within %.3f units of 2^-24 max|p|" % (S, P, n, angle, zoom, sigma, err))
                assert got.dtype == np.float32 and err <= 2.0, (S, P, n, angle, zoom, sigma, err)
                lab = eref.deform_nearest(code, m, d, n, P, y0, x0)
                want_lab = ndi.map_coordinates(code, [sy, sx], order=0, mode="mirror")
                assert lab.dtype == np.uint8 and np.array_equal(lab, want_lab), (S, P, n, angle, zoom, sigma, int((lab != want_lab).sum()))
                if sigma >= 2.0 and angle == 0.0:            # the deformation moved something
                    assert (lab != code[y0:y0 + P, x0:x0 + P]).mean() > 0.1
                pixels += lab.size
    assert pixels == 3 * 5 * (64 * 64 + 64 * 64 + 32 * 32)


def _check(e, n=None, msg_cap=256):
    from unmicst_amd import build, umx
    build.build()
    L = trainer._bind(umx.load())
    msg = ctypes.create_string_buffer(msg_cap)
    rc = L.umx_elastic_desc_check(e.ctypes.data, len(e) if n is None else n, msg, len(msg))
    return rc, msg.value.decode()


def test_elastic_desc_check():
    assert trainer.ELASTIC_DESC.itemsize == 304 and trainer.ELASTIC_DESC.fields["d"][1] == 16
    rng = np.random.default_rng(3)
    edge = np.zeros((2, 6, 6), np.float32)
    edge[:, :4, :4] = 32.0
    edge[1, 3, 3] = -32.0
    good = _elastics([None, (4, _lattice(rng, 4, 3.0)), (5, _lattice(rng, 5, 16.0)), (6, _lattice(rng, 6, 1.0)), (4, edge), None])
    assert _check(good) == (0, "")
    nan, inf = float("nan"), float("inf")

    def broken(at, kw):
        e = good.copy()
        for k, v in kw.items():
            if k == "n":
                e["n"][at] = v
            elif k == "reserved":
                e["reserved"][at][v] = 1
            else:
                e["d"][at][k] = v
        return e

    cases = [(0, dict(n=3), "n is not"), (1, dict(n=7), "n is not"), (2, dict(n=-4), "n is not"), (3, dict(n=1), "n is not"),
             (1, dict(reserved=0), "reserved"), (0, dict(reserved=2), "reserved"), (5, dict(reserved=1), "reserved"),
             (1, {(0, 1, 1): nan}, "finite"), (2, {(1, 4, 4): inf}, "finite"), (3, {(0, 5, 5): -inf}, "finite"),
             (0, {(1, 5, 5): nan}, "finite"),
             (1, {(0, 0, 0): 32.000004}, "above 32"), (3, {(1, 5, 0): -33.0}, "above 32"),
             (1, {(0, 4, 0): 0.5}, "outside"), (1, {(1, 0, 4): -1e-30}, "outside"), (2, {(0, 5, 5): 1.0}, "outside"),
             (2, {(1, 2, 5): 1.0}, "outside"), (0, {(0, 0, 0): 0.25}, "outside"), (5, {(1, 3, 3): 1.0}, "outside")]
    for at, kw, rule in cases:
        rc, msg = _check(broken(at, kw))
        assert rc == ERR_INVALID and rule in msg and ("elastic %d " % at) in msg, (at, kw, rc, msg)
    # the first broken one is named; the ones behind the checked range are not looked at
    two = broken(4, dict(n=9))
    two["n"][2] = 2
    assert "elastic 2 " in _check(two)[1]
    assert _check(two, n=2) == (0, "")
    # with n == 0 a block that would be fine for n == 4 is refused; -0.0 counts as zero
    e = _elastics([(4, edge)])
    e["n"][0] = 0
    assert _check(e)[0] == ERR_INVALID
    e = _elastics([None])
    e["d"][0][0, 0, 0] = -0.0
    assert _check(e) == (0, "")
    from unmicst_amd import umx
    L = trainer._bind(umx.load())
    assert L.umx_elastic_desc_check(None, 1, None, 0) == ERR_INVALID
    bad = broken(1, dict(n=7))
    assert L.umx_elastic_desc_check(bad.ctypes.data, len(bad), None, 0) == ERR_INVALID          # msg may be NULL
    assert L.umx_elastic_desc_check(good.ctypes.data, len(good), None, 0) == 0
    assert _check(bad, msg_cap=8)[1] == "elastic"                                               # truncated, NUL-terminated


def test_elastic_lattice():
    z = np.array([-3.0, -2.0, -0.5, 0.0, 0.5, 2.0, 2.5, 1.0] * 4, np.float64)
    d = trainset.elastic_lattice(z, 3.0, 4)
    assert d.dtype == np.float32 and d.shape == (2, 6, 6)
    assert d[:, :4, :4].tobytes() == (3.0 * np.clip(z, -2, 2)).astype(np.float32).tobytes()
    assert not d[:, 4:, :].any() and not d[:, :, 4:].any() and not (np.signbit(d) & (d == 0)).any()
    assert trainset.elastic_lattice(z.reshape(2, 4, 4), 3.0, 4).tobytes() == d.tobytes()
    assert np.abs(trainset.elastic_lattice(np.full(72, 9.0), 16.0, 6)).max() == 32.0
    for bad in ((z, 3.0, 5), (z, 3.0, 3), (z, 3.0, 7), (z, -1.0, 4), (z, float("nan"), 4), (z, 16.5, 4), (np.full(32, np.inf), 1.0, 4)):
        with pytest.raises(ValueError):
            trainset.elastic_lattice(*bad)


def _stream(seed, n_samples, batch, size, P, n_pages, mb, mc, aug, warp, elastic, batches):
    """The documented draw order, restated: per epoch a permutation; per image page, y0, x0, transform, brightness sign and magnitude,
    contrast sign and magnitude; then (blur / saturation on) 4 draws; then (warp on) 4 draws; then (elastic on) the coin and
    standard_normal(2 n n)."""
    r = np.random.Generator(np.random.PCG64(seed))
    perm, pos = r.permutation(n_samples), 0
    out = []
    for _ in range(batches):
        d = np.zeros(batch, trainer.SAMPLE_DESC)
        coins = []
        for j in range(batch):
            if pos == n_samples:
                perm, pos = r.permutation(n_samples), 0
            d["index"][j] = perm[pos]
            pos += 1
            d["page"][j] = r.integers(n_pages)
            d["y0"][j] = r.integers(size - P + 1)
            d["x0"][j] = r.integers(size - P + 1)
            d["transform"][j] = r.integers(8)
            sb = -1.0 if r.random() < 0.5 else 1.0
            d["brightness"][j] = mb * sb * r.random() + 0.0
            sc = -1.0 if r.random() < 0.5 else 1.0
            d["contrast"][j] = 1.0 + mc * sc * r.random()
            if aug:
                r.random(), r.integers(max(aug - 1, 1)), r.random(), r.random()
            if warp:
                r.random(), r.random(), r.random(), r.random()
            prob, n = elastic
            coins.append((r.random() < prob, r.standard_normal(2 * n * n)))
        out.append((d, coins))
    return out


def test_sampler_keeps_its_stream_and_draws_the_lattice():
    kw = dict(n_samples=7, batch=4, size=40, P=16, n_pages=2, max_brightness=0.25, max_contrast=0.025, transforms=True)
    augkw = dict(blur_levels=4, blur_prob=0.4, saturate_prob=0.25, max_gain=3.0)
    warpkw = dict(rotate_prob=0.5, zoom_prob=0.5, zoom_range=(0.8, 1.25))
    for seed in (0, 5, 123456789):
        for extra in (dict(), augkw, warpkw, dict(augkw, **warpkw)):
            # elastic off: the bytes of a sampler built without the new arguments, through every entry
            s0 = trainset.Sampler(seed, **kw, **extra)
            s1 = trainset.Sampler(seed, **kw, **extra, elastic_prob=0.0, elastic_sigma=3.0, elastic_grid=3)
            s2 = trainset.Sampler(seed, **kw, **extra, elastic_prob=0.0)
            for _ in range(8):
                want = s0.next_warped()
                got = s1.next_warped()
                d, a, w, e = s2.next_elastic()
                assert len(want) == len(got) == 3
                for x, y, z in zip(want, got, (d, a, w)):
                    assert x.dtype == y.dtype and x.tobytes() == y.tobytes() == z.tobytes()
                assert e.dtype == trainer.ELASTIC_DESC and e.shape == (4,) and not e.tobytes().strip(b"\0")
            # elastic on: the two draws follow the image's previous ones
            for grid in (1, 2, 3):
                n = grid + 3
                s = trainset.Sampler(seed, **kw, **extra, elastic_prob=0.5, elastic_sigma=2.5, elastic_grid=grid)
                want = _stream(seed, 7, 4, 40, 16, 2, 0.25, 0.025, 4 if "blur_prob" in extra else 0, "rotate_prob" in extra, (0.5, n), 6)
                for d0, coins in want:
                    d, a, w, e = s.next_elastic()
                    assert d.tobytes() == d0.tobytes()
                    for j, (coin, z) in enumerate(coins):
                        assert e["n"][j] == (n if coin else 0) and not e["reserved"][j].any()
                        lat = trainset.elastic_lattice(z, 2.5, n) if coin else np.zeros((2, 6, 6), np.float32)
                        assert e["d"][j].tobytes() == lat.tobytes()
                        assert np.abs(e["d"][j]).max() <= 5.0 and not e["d"][j][:, n:, :].any() and not e["d"][j][:, :, n:].any()
    # the coins shift nothing: d, a, w of consecutive batches are those of the run that deforms every image, and so are the lattices
    # of the images that are deformed
    full = dict(augkw, **warpkw)
    a_, b_ = (trainset.Sampler(3, **kw, **full, elastic_prob=p, elastic_sigma=4.0, elastic_grid=2) for p in (0.4, 1.0))
    c_ = trainset.Sampler(3, **kw, **full, elastic_prob=0.4, elastic_sigma=4.0, elastic_grid=2)
    hit = miss = 0
    for _ in range(40):
        (da, aa, wa, ea), (db, ab, wb, eb) = a_.next_elastic(), b_.next_elastic()
        assert da.tobytes() == db.tobytes() and aa.tobytes() == ab.tobytes() and wa.tobytes() == wb.tobytes()
        assert all(x.tobytes() == y.tobytes() for x, y in zip(c_.next_warped(), (da, aa, wa)))       # next_warped: the first three
        assert (eb["n"] == 5).all()
        for j in range(4):
            if ea["n"][j]:
                assert ea[j].tobytes() == eb[j].tobytes() and np.abs(ea["d"][j]).max() <= 8.0 and ea["d"][j].any()
                hit += 1
            else:
                assert not ea["d"][j].any()
                miss += 1
    assert hit > 40 and miss > 60, (hit, miss)
    for bad in (dict(elastic_prob=1.5), dict(elastic_prob=-0.1), dict(elastic_prob=float("nan")), dict(elastic_prob=0.5),
                dict(elastic_prob=0.5, elastic_sigma=0.0), dict(elastic_sigma=-1.0), dict(elastic_sigma=float("inf")),
                dict(elastic_sigma=16.5), dict(elastic_sigma=1.0, elastic_grid=0), dict(elastic_sigma=1.0, elastic_grid=4),
                dict(elastic_sigma=1.0, elastic_grid=1.5)):
        with pytest.raises(ValueError):
            trainset.Sampler(1, **kw, **bad)


def test_finetune_elastic_flags_parse_and_refuse():
    base = ["--model", "no-such-model", "--train", "t", "--valid", "v", "--out", "o"]
    parse = finetune.build_parser().parse_args
    assert finetune.elastic_settings(parse(base)) is None
    assert finetune.elastic_settings(parse(base + ["--rotate-prob", "1"])) is None
    assert finetune.warp_settings(parse(base + ["--elastic-sigma", "3"])) is None
    assert finetune.augment_settings(parse(base + ["--elastic-sigma", "3"])) is None
    assert finetune.elastic_settings(parse(base + ["--elastic-sigma", "3"])) == {"prob": 0.5, "sigma": 3.0, "grid": 2}
    ns = parse(base + ["--elastic-sigma", "3", "--elastic-grid", "2", "--elastic-prob", "1"])
    assert finetune.elastic_settings(ns) == {"prob": 1.0, "sigma": 3.0, "grid": 2}
    assert finetune.elastic_settings(ns, 128) == {"prob": 1.0, "sigma": 3.0, "grid": 2}
    assert finetune.elastic_settings(parse(base + ["--elastic-sigma", "1.5", "--elastic-grid", "3", "--elastic-prob", "0"]), 64) == {
        "prob": 0.0, "sigma": 1.5, "grid": 3}
    bad = [["--elastic-prob", "0.5"], ["--elastic-prob", "1.5", "--elastic-sigma", "2"], ["--elastic-prob", "nan", "--elastic-sigma", "2"],
           ["--elastic-prob", "-0.1", "--elastic-sigma", "2"], ["--elastic-sigma", "0"], ["--elastic-sigma", "-2"], ["--elastic-sigma", "nan"],
           ["--elastic-sigma", "inf"], ["--elastic-sigma", "2", "--elastic-grid", "0"], ["--elastic-sigma", "2", "--elastic-grid", "4"],
           ["--elastic-grid", "7"]]
    for extra in bad:
        with pytest.raises(finetune.Refusal):
            finetune.elastic_settings(parse(base + extra))
        with pytest.raises(finetune.Refusal) as e:       # prepare refuses them before it looks at the model or the sets
            finetune.prepare(parse(base + extra))
        assert "no such directory" not in str(e.value), extra
    with pytest.raises(finetune.Refusal) as e:
        finetune.prepare(parse(base + ["--elastic-sigma", "3"]))
    assert "no such directory" in str(e.value)
    # sigma < (imSize - 1) / (8 G): the deformation cannot fold the image over itself
    for P, G, ok, refused in ((128, 2, 7.9, 7.9375), (128, 1, 15.8, 15.875), (128, 3, 5.29, 5.3), (32, 2, 1.9, 1.9375), (64, 3, 2.6, 2.625),
                              (256, 1, 16.0, 31.875), (256, 2, 15.9, 15.9375)):
        args = ["--elastic-grid", str(G), "--elastic-sigma"]
        assert finetune.elastic_settings(parse(base + args + [repr(ok)]), P)["sigma"] == ok
        with pytest.raises(finetune.Refusal) as e:
            finetune.elastic_settings(parse(base + args + [repr(refused)]), P)
        assert "fold" in str(e.value), (P, G)
        assert finetune.elastic_settings(parse(base + args + [repr(refused)])) is not None          # without the tile: only the flags
    # a tile above 256: the clip at 2 sigma has to stay inside the descriptor's bound, whatever the fold bound allows
    assert finetune.elastic_settings(parse(base + ["--elastic-grid", "1", "--elastic-sigma", "16"]), 512)["sigma"] == 16.0
    with pytest.raises(finetune.Refusal) as e:
        finetune.elastic_settings(parse(base + ["--elastic-grid", "1", "--elastic-sigma", "16.5"]), 512)
    assert "32" in str(e.value) and "fold" not in str(e.value)
