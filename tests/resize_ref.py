"""numpy restatement of the resize kernels' arithmetic (unmicst_amd/csrc/umx_kernels.hip: gauss1d_kernel, zoom1_kernel, the clip
and the uint8 cast of resize_plane) and of the host-side Gaussian weights (umx_host.hip: gauss_weights), one IEEE operation per
numpy operation in the kernels' order.  It runs without a GPU: tests/test_imagekernels_cpu.py holds it to scipy.ndimage, and a
device mismatch in tests/test_gpu_imagekernels.py is diagnosed by asking which of the two the device disagrees with."""
import numpy as np


def mirror_index(i, n):
    """scipy 'mirror' (d c b | a b c d | c b a) of integer indices, as the kernels' mirror_index"""
    i = np.asarray(i, np.int64)
    if n == 1:
        return np.zeros_like(i)
    period = 2 * n - 2
    i = np.mod(i, period)
    return np.where(i < n, i, period - i)


def pairwise_sum(a):
    """numpy's float64 add.reduce over a contiguous vector: sequential below 8 terms, eight accumulators up to 128, halves beyond"""
    n = len(a)
    if n < 8:
        res = np.float64(0.0)
        for v in a:
            res = res + v
        return res
    if n <= 128:
        r = [np.float64(v) for v in a[:8]]
        i = 8
        while i < n - n % 8:
            for j in range(8):
                r[j] = r[j] + a[i + j]
            i += 8
        res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]))
        for v in a[i:]:
            res = res + v
        return res
    n2 = n // 2
    n2 -= n2 % 8
    return pairwise_sum(a[:n2]) + pairwise_sum(a[n2:])


def gauss_weights(sigma, exp=np.exp):
    """(radius, w[0..radius]) with w[0] the centre tap: exp(c * (x * x)) / pairwise sum, c = -0.5 / (sigma * sigma)"""
    sigma = np.float64(sigma)
    radius = int(4.0 * sigma + 0.5)
    c = np.float64(-0.5) / (sigma * sigma)
    x = np.arange(-radius, radius + 1).astype(np.float64)
    full = exp(c * (x * x))
    return radius, full[radius:] / pairwise_sum(full)


def resize_sigmas(H, W, h, w):
    return [max(0.0, (np.float64(n) / np.float64(m) - 1.0) / 2.0) for n, m in ((H, h), (W, w))]


def gauss1d(src, axis, w):
    """one axis of the separable Gaussian: centre tap, then the symmetric pairs from the outside in (scipy's correlate1d)"""
    n = src.shape[axis]
    idx = np.arange(n)
    acc = src * w[0]
    for j in range(len(w) - 1, 0, -1):
        a = np.take(src, mirror_index(idx - j, n), axis=axis)
        b = np.take(src, mirror_index(idx + j, n), axis=axis)
        acc = acc + (a + b) * w[j]
    return acc


def zoom_axis(n_in, n_out):
    """per output index of one axis: (i0, i1, w0, w1, on_band).  The coordinate (o + 0.5) * (in / out) - 0.5 is reflected about
    sample 0 when it is negative, the way scipy maps the coordinate before it splits it; the second weight is 1 - (1 - t)."""
    z = np.float64(n_in) / np.float64(n_out)
    c = (np.arange(n_out).astype(np.float64) + 0.5) * z - 0.5
    band = (c < 0) | (c > n_in - 1)
    c = np.where(c < 0, -c, c) if n_in > 1 else np.zeros(n_out)   # (an axis of one sample: scipy maps every coordinate to 0)
    f = np.floor(c)
    w0 = 1.0 - (c - f)
    w1 = 1.0 - w0
    i0 = f.astype(np.int64)
    return mirror_index(i0, n_in), mirror_index(i0 + 1, n_in), w0, w1, band


def zoom1(src, h, w):
    """order-1 zoom (grid mode, mirror) [H, W] -> [h, w]: value * w_axis0 * w_axis1 over the 2 x 2 support in C order"""
    H, W = src.shape
    y0, y1, wy0, wy1, _ = zoom_axis(H, h)
    x0, x1, wx0, wx1, _ = zoom_axis(W, w)
    v = np.zeros((h, w))
    v = v + src[y0][:, x0] * wy0[:, None] * wx0[None, :]
    v = v + src[y0][:, x1] * wy0[:, None] * wx1[None, :]
    v = v + src[y1][:, x0] * wy1[:, None] * wx0[None, :]
    v = v + src[y1][:, x1] * wy1[:, None] * wx1[None, :]
    return v


def band_mask(H, W, h, w):
    """output pixels whose source coordinate lies outside [0, n - 1] on some axis"""
    return zoom_axis(H, h)[4][:, None] | zoom_axis(W, w)[4][None, :]


def filtered(src, h, w, weights=gauss_weights):
    """the anti-aliasing Gaussian of resize_plane: both axes when any axis shrinks, an axis with sigma <= 1e-15 skipped"""
    H, W = src.shape
    cur = src
    if h < H or w < W:
        for axis, sigma in enumerate(resize_sigmas(H, W, h, w)):
            if sigma > 1e-15:
                cur = gauss1d(cur, axis, weights(sigma)[1])
    return cur


def resize(src, h, w, weights=gauss_weights):
    """(float64 plane, uint8 plane) of resize_plane: filter, zoom, clip to the filtered plane's range, np.uint8(255 * .)"""
    cur = filtered(np.ascontiguousarray(src, np.float64), h, w, weights)
    v = np.minimum(np.maximum(zoom1(cur, h, w), cur.min()), cur.max())
    return v, (255.0 * v).astype(np.int64).astype(np.uint8)


# ---- the cases tests/test_imagekernels_cpu.py and tests/test_gpu_imagekernels.py share, and their scipy reference -------------
SCALINGS = (0.9, 0.8, 0.75, 2 / 3, 0.6, 0.5, 0.4, 4 / 11, 1 / 3, 0.3, 0.25, 0.125)

SHAPES = [(40, 52, 20, 26), (37, 53, 27, 39), (44, 33, 12, 9),   # the third has radius 5
          (3, 40, 1, 13),                                        # radius larger than the axis
          (9, 9, 3, 14),                                         # one axis shrinks, the other grows
          (1, 17, 1, 5),                                         # single row
          (20, 26, 32, 41), (13, 11, 52, 44), (2, 2, 5, 5)]      # upsampling
SHAPES += [(97, 131, int(97 * s), int(131 * s)) for s in (0.5, 0.75, 1.6, 0.3)]
SHAPES += [(1100, 1000, 550, 500), (550, 500, 1100, 1000)]       # > 1,048,576 elements: the grid-stride loops go round again
CONTENTS = ("uniform", "u16", "plateau8")


def plane(kind, H, W):
    rng = np.random.default_rng([H, W, CONTENTS.index(kind)])
    if kind == "uniform":
        return rng.random((H, W))
    if kind == "u16":
        return np.multiply(rng.integers(0, 65536, (H, W), dtype=np.uint16), 1.0 / 65535, dtype=np.float64)
    # piecewise-constant uint8 levels on a coarse grid of cells: plateaus touch all four borders and the corners, one corner is
    # saturated (255 * v sits on an integer there, so one ulp would decide a whole LSB of np.uint8(255 * v))
    ny, nx = min(H, 4), min(W, 5)
    cells = rng.integers(0, 256, (ny, nx), dtype=np.uint8)
    cells[0, 0], cells[-1, -1] = 255, 0
    img = cells[(np.arange(H) * ny) // H][:, (np.arange(W) * nx) // W]
    return np.multiply(img, 1.0 / 255, dtype=np.float64)


def scipy_weights(sigma):
    """scipy's own Gaussian weights [0] = centre .. [radius], through a public call: the response to a unit impulse"""
    from scipy import ndimage as ndi
    radius = int(4.0 * float(sigma) + 0.5)
    impulse = np.zeros(2 * radius + 1)
    impulse[radius] = 1.0
    return radius, ndi.gaussian_filter1d(impulse, sigma, mode="constant")[radius:]


def scipy_filtered(src, h, w, weights):
    """the anti-aliasing filter by scipy.ndimage.correlate1d (mode 'mirror', axis 0 then 1) with the given weights(sigma) ->
    (radius, w[0..radius]) mirrored to full length, which takes scipy's symmetric path"""
    from scipy import ndimage as ndi
    H, W = src.shape
    cur = src
    if h < H or w < W:
        for axis, sigma in enumerate(resize_sigmas(H, W, h, w)):
            if sigma > 1e-15:
                wt = np.asarray(weights(sigma)[1])
                cur = ndi.correlate1d(cur, np.concatenate([wt[:0:-1], wt]), axis=axis, mode="mirror")
    return cur


def scipy_resize(src, h, w, weights):
    """(filtered plane, float64 plane, uint8 plane): scipy.ndimage.zoom as unmicst_amd.imtools.resize calls it, clipped to the
    filtered plane's range, and the drivers' np.uint8(255 * .)"""
    from scipy import ndimage as ndi
    H, W = src.shape
    cur = scipy_filtered(src, h, w, weights)
    out = np.empty((h, w), np.float64)
    ndi.zoom(cur, [h / H, w / W], output=out, order=1, mode="mirror", cval=0, grid_mode=True)
    out = np.clip(out, cur.min(), cur.max())
    return cur, out, np.uint8(255 * out)


def band_bound(H, W, src):
    """the bound on the mirrored band, had the kernel kept its own order there: (8 + 4 max(H, W)) 2^-53 max|src| -- four
    non-negative terms with two roundings each and three additions, plus the rounding of the reflected coordinate in the weight"""
    return (8 + 4 * max(H, W)) * 2.0 ** -53 * float(np.abs(src).max())
