"""The driver-side image kernels of umx_kernels.hip -- what --scalingFactor, --outlier and the device-side range search run --
plane by plane against scipy.ndimage / numpy, bit for bit, through the umx_test_*_dev entries (thin wrappers around the
production functions).  The end-to-end tests in test_gpu_cli.py see these kernels only through a whole network and a uint8 cast.

A mismatch in the resize is diagnosed with tests/resize_ref.py, the numpy restatement of the kernels' arithmetic that
tests/test_imagekernels_cpu.py holds to scipy without a GPU: the failure message says whether the device left the restatement."""
import numpy as np
import pytest

import resize_ref as R
from unmicst_amd import build, imtools, umx

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def lib():
    build.build()
    return umx.load()


def lib_weights(sigma):
    return None, umx.gauss_weights(sigma)


# ---- resize ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", R.CONTENTS)
@pytest.mark.parametrize("shape", R.SHAPES, ids=lambda s: "%dx%d-%dx%d" % s)
def test_resize_is_scipys(shape, kind):
    """Reference: scipy.ndimage.correlate1d(mode='mirror'), axis 0 then 1, with the library's own weights; scipy.ndimage.zoom
    (order 1, 'mirror', grid mode) as imtools.resize calls it; the clip to the filtered plane's range.  The plane after the
    Gaussian, the float64 plane and the uint8 plane are bit-equal, on and off the mirrored band (the output pixels whose source
    coordinate lies outside [0, n - 1]: the kernel evaluates the border the way scipy does, so no bound is needed there; the
    bound the band would otherwise get is asserted first, to tell an ulp from a wrong pixel)."""
    H, W, h, w = shape
    src = R.plane(kind, H, W)
    filt, want, want8 = R.scipy_resize(src, h, w, lib_weights)
    got, got8, got_filt = umx.resize_dev(src, h, w)
    band = R.band_mask(H, W, h, w)
    d = np.abs(got - want)
    print("%s %s: band pixels %d, differing on the band %d, off it %d, largest difference %.3g; uint8 differing %d; filtered differing %d"
          % (shape, kind, band.sum(), (d[band] != 0).sum(), (d[~band] != 0).sum(), d.max(), (got8 != want8).sum(),
             (got_filt != filt).sum()))

    def restated():
        mine, mine8 = R.resize(src, h, w, lib_weights)
        return "device == restatement: float64 %s, uint8 %s" % (np.array_equal(got, mine), np.array_equal(got8, mine8))

    assert np.array_equal(got_filt, filt), "after the Gaussian: %d pixels differ, at most %.3g" % (
        (got_filt != filt).sum(), np.abs(got_filt - filt).max())
    assert np.array_equal(got[~band], want[~band]) and np.array_equal(got8[~band], want8[~band]), restated()
    assert d.max() <= R.band_bound(H, W, filt), restated()
    assert np.array_equal(got, want), restated()
    assert np.array_equal(got8, want8), restated()


# ---- percentile and rescale --------------------------------------------------------------------------------------------------
SIZES = (1, 2, 3, 101, 255, 256, 257, 4097, 1200000)
QS = (0.0, 100.0, 50.0, 99.0, 99.9, 37.5, 25.0, 1e-9, 100 - 1e-9)
PLANES = ("uniform", "levels", "equal", "last_byte", "powers")


def value_plane(kind, n):
    rng = np.random.default_rng([n, PLANES.index(kind)])
    if kind == "uniform":
        return rng.random(n)
    if kind == "levels":        # 256 levels of u8 / 255: heavy ties
        return np.multiply(rng.integers(0, 256, n, dtype=np.uint8), 1.0 / 255, dtype=np.float64)
    if kind == "equal":         # takes the lo == hi branch of the rescale at every q
        return np.full(n, 0.37)
    if kind == "last_byte":     # 0.5 + i 2^-53: distinct doubles that differ only in the last byte(s) of the radix selection
        return rng.permutation(0.5 + np.arange(n) * 2.0 ** -53)
    # powers of two from 2^-1074 (the smallest subnormal) to 1 and exact zeros: they differ in the top bytes
    k = np.arange(n) % 1080
    return rng.permutation(np.where(k > 1074, 0.0, np.ldexp(1.0, -np.minimum(k, 1074))))


def test_percentile_cases_cover_the_interpolation_branches():
    """the (n, q) grid below holds an integral index (gamma 0: q = 25 at n = 101), a gamma >= 0.5 and a gamma in (0, 0.5)"""
    gam = {(n, q): (n - 1) * (q / 100) - np.floor((n - 1) * (q / 100)) for n in SIZES for q in QS}
    assert gam[(101, 25.0)] == 0.0
    assert gam[(256, 50.0)] == 0.5 and 0.5 < gam[(4097, 99.9)] < 1
    assert 0 < gam[(257, 99.0)] < 0.5


@pytest.mark.parametrize("kind", PLANES)
def test_percentile_and_rescale_are_numpys(kind):
    """The limit has the bits of np.percentile(plane, q); the rescaled plane the bits of imtools.rescale_intensity(plane,
    (plane.min(), limit), (0, 0.983)).  outlier < 0 rescales to (min, max)."""
    for n in SIZES:
        plane = value_plane(kind, n)
        lo = plane.min()
        for q in QS + (-1.0,):
            limit = np.percentile(plane, q) if q >= 0 else plane.max()
            got, rng = umx.rescale_dev(plane, q)
            assert rng[0].tobytes() == lo.tobytes() and rng[1].tobytes() == np.float64(limit).tobytes(), (
                n, q, float(rng[0]), float(lo), float(rng[1]).hex(), float(limit).hex())
            want = imtools.rescale_intensity(plane, (lo, limit), (0, 0.983))
            assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), (n, q, np.abs(got - want).max())


# ---- raw range ---------------------------------------------------------------------------------------------------------------
LEVELS = {np.uint8: (3, 100, 250), np.uint16: (0x00FF, 0x8080, 0xFF00)}   # (minimum, filling, maximum)


def check_ranges(planes, offsets):
    """the range of every plane at its offset, over one slab and over three slabs of odd length: always (min, max) exactly"""
    want = np.array([[p.min(), p.max()] for p in planes], np.uint32)
    for nslabs in (1, 3):
        got = umx.plane_range_dev(planes, offsets, [nslabs] * len(planes))
        bad = np.flatnonzero((got != want).any(axis=1))
        assert bad.size == 0, "nslabs %d: %d of %d wrong, first: n %d offset %d got %s want %s" % (
            nslabs, bad.size, len(planes), planes[bad[0]].size, offsets[bad[0]], got[bad[0]], want[bad[0]])


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16])
def test_raw_range_finds_an_extreme_at_every_position(dtype):
    """every start offset 0..16 elements from an aligned address, every n in 1..40, a filling value with one minimum at
    position i and one maximum at n - 1 - i for every i: a scalar head, 16-byte middle or scalar tail that skips an element
    loses the one extreme that sits there"""
    lo, mid, hi = LEVELS[dtype]
    planes = []
    for n in range(1, 41):
        m = np.full((n, n), mid, dtype)
        m[np.arange(n), np.arange(n)] = lo
        m[np.arange(n), n - 1 - np.arange(n)] = hi
        planes += list(m)
    for offset in range(17):
        check_ranges(planes, [offset] * len(planes))


def extreme_positions(n, offset, itemsize):
    """(position of the minimum, position of the maximum) pairs: the first 20 and the last 20 elements, and either side of the
    head | middle and middle | tail boundaries of the kernel for a plane that starts `offset` elements past an aligned address"""
    per = 16 // itemsize
    head = min(n, ((16 - offset * itemsize % 16) % 16) // itemsize)
    tail = head + (n - head) // per * per
    pairs = [(i, n - 1 - i) for i in range(min(20, n))] + [(n - 1 - i, i) for i in range(min(20, n))]
    for b in (head, tail):
        if 1 <= b < n:
            pairs += [(b - 1, b), (b, b - 1)]
    return pairs


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16])
@pytest.mark.parametrize("n", [255, 256, 257, 4099])
def test_raw_range_at_the_ends_and_the_vector_boundaries(n, dtype):
    lo, mid, hi = LEVELS[dtype]
    planes, offsets = [], []
    for offset in range(17):
        for i_lo, i_hi in extreme_positions(n, offset, np.dtype(dtype).itemsize):
            p = np.full(n, mid, dtype)
            p[i_lo], p[i_hi] = lo, hi
            planes.append(p)
            offsets.append(offset)
    check_ranges(planes, offsets)


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16])
def test_raw_range_of_a_large_plane(dtype):
    """2^21 + 3 elements (more than one block per wave of the grid), one plane per call"""
    n = 2 ** 21 + 3
    lo, mid, hi = LEVELS[dtype]
    p = np.full(n, mid, dtype)
    for offset in (0, 1, 13):
        for i_lo, i_hi in extreme_positions(n, offset, np.dtype(dtype).itemsize):
            p[i_lo], p[i_hi] = lo, hi
            check_ranges([p], [offset])
            p[i_lo] = p[i_hi] = mid


# ---- uint8 cast --------------------------------------------------------------------------------------------------------------
def test_uint8_cast_of_every_probability():
    """every float16 bit pattern from 0 to 1.0 against the numpy recipe of imtools.to_uint8_via_resize at the identity grid:
    np.uint8(255 * pm) in float16, times 1 / 255 in float64, np.uint8(255 * .)"""
    pm = np.arange(0x3C00 + 1, dtype=np.uint16).view(np.float16)
    got8, gotf = umx.half_to_u8_dev(pm)
    wantf = imtools.img_as_float(np.uint8(255 * pm))
    want8 = imtools.to_uint8_via_resize(pm.reshape(1, -1), (1, pm.size)).ravel()
    assert wantf.dtype == np.float64 and np.array_equal(gotf.view(np.uint64), wantf.view(np.uint64))
    assert np.array_equal(got8, want8)
    assert want8[-1] == 255 and want8[0] == 0
