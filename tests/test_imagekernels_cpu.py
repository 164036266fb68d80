"""The resize of the scaled path without a GPU: the library's host-side Gaussian weights against scipy's, and the numpy
restatement of the kernels' arithmetic (tests/resize_ref.py) against scipy.ndimage bit for bit -- the restatement is what
tests/test_gpu_imagekernels.py diagnoses a device mismatch with, so it has to be right on its own."""
import math

import numpy as np
import pytest
from scipy import ndimage as ndi

import resize_ref as R
from unmicst_amd import build, imtools, umx


@pytest.fixture(scope="module")
def lib():
    build.build()
    return umx.load()


def sigma_of(s):
    return (1 / s - 1) / 2


def libm_exp(x):
    return np.array([math.exp(v) for v in x])


@pytest.mark.parametrize("s", R.SCALINGS)
def test_gauss_weights_against_scipy(lib, s):
    """Radius as scipy's; every tap within 4 ulp of scipy's (one from exp -- numpy's and the C library's differ on a few taps --
    and the normalising sum of at most 2 r + 1 terms moves the quotient by the rest); the full kernel sums to 1 within 2 r + 1
    ulp of 1 (one rounding per quotient)."""
    sigma = sigma_of(s)
    r, want = R.scipy_weights(sigma)
    got = umx.gauss_weights(sigma)
    assert len(got) == r + 1
    ulps = np.abs(got - want) / np.spacing(want)
    print("scaling %.4g sigma %.4g radius %d: %d taps differ, at most %g ulp" % (s, sigma, r, (got != want).sum(), ulps.max()))
    assert ulps.max() <= 4
    assert abs(math.fsum(got) + math.fsum(got[1:]) - 1.0) <= (2 * r + 1) * 2.0 ** -52


@pytest.mark.parametrize("sigma", [sigma_of(s) for s in R.SCALINGS] + [0.875, 3.5, 16.25, 40.0])
def test_gauss_weights_operation_order(lib, sigma):
    """exp aside, the weights are scipy's operations in scipy's order: c * (x * x) and numpy's pairwise sum.  The restatement
    with numpy's exp IS scipy's kernel, bit for bit; the library is the same restatement with the C library's exp.  (sigma 16.25
    and 40: 131 and 321 taps, where numpy's sum recurses.)"""
    r, want = R.scipy_weights(sigma)
    r2, mine = R.gauss_weights(sigma)
    assert r2 == r and np.array_equal(mine, want)
    assert np.array_equal(umx.gauss_weights(sigma), R.gauss_weights(sigma, exp=libm_exp)[1])


def test_pairwise_sum_is_numpys():
    rng = np.random.default_rng(5)
    for n in list(range(1, 150)) + [255, 256, 257, 300, 641, 1000]:
        a = rng.random(n) * 10.0 ** rng.integers(-3, 4, n)
        assert R.pairwise_sum(a) == a.sum(), n


def test_gauss_weights_refuses_what_the_resize_cannot_take(lib):
    with pytest.raises(ValueError):
        umx.gauss_weights(0.0)
    with pytest.raises(ValueError):
        umx.gauss_weights(1024.0)      # radius 4096: one tap more than the kernels' weight buffer holds
    assert len(umx.gauss_weights(1023.8)) == 4096


@pytest.mark.parametrize("kind", R.CONTENTS)
@pytest.mark.parametrize("shape", R.SHAPES, ids=lambda s: "%dx%d-%dx%d" % s)
def test_restated_kernels_are_scipy_bit_for_bit(lib, shape, kind):
    """Gaussian (with the library's weights), zoom, clip and uint8 cast of the restatement against scipy.ndimage.correlate1d /
    zoom: every pixel, the mirrored band included."""
    H, W, h, w = shape
    src = R.plane(kind, H, W)
    weights = lambda sigma: (None, umx.gauss_weights(sigma))
    filt, want, want8 = R.scipy_resize(src, h, w, weights)
    assert np.array_equal(R.filtered(src, h, w, weights), filt)
    got, got8 = R.resize(src, h, w, weights)
    band = R.band_mask(H, W, h, w)
    assert np.array_equal(got[~band], want[~band])
    assert np.abs(got - want).max() <= R.band_bound(H, W, filt)
    assert np.array_equal(got, want) and np.array_equal(got8, want8)


@pytest.mark.parametrize("shape", [s for s in R.SHAPES if s[0] * s[1] < 65536], ids=lambda s: "%dx%d-%dx%d" % s)
def test_restatement_with_numpys_exp_is_the_host_recipe(shape):
    """with scipy's own weights the restatement is unmicst_amd.imtools.resize (gaussian_filter + zoom + clip) bit for bit"""
    H, W, h, w = shape
    src = R.plane("u16", H, W)
    assert np.array_equal(R.resize(src, h, w)[0], imtools.resize(src, (h, w)))


def test_band_is_where_the_coordinate_leaves_the_image():
    assert not R.band_mask(40, 52, 20, 26).any()                 # shrinking: the first coordinate is (z - 1) / 2 >= 0
    b = R.band_mask(2, 2, 5, 5)
    assert b.sum() == 16 and not b[1:4, 1:4].any()
    assert R.band_mask(20, 26, 32, 41)[0].all() and R.band_mask(20, 26, 32, 41)[:, -1].all()


def test_zoom_of_a_single_sample_axis():
    """1 -> n along an axis: scipy maps every coordinate to sample 0"""
    src = np.random.default_rng(2).random((1, 7))
    out = np.empty((3, 10))
    ndi.zoom(src, [3, 10 / 7], output=out, order=1, mode="mirror", cval=0, grid_mode=True)
    assert np.array_equal(R.zoom1(src, 3, 10), out)
