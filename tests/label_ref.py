"""numpy / scipy restatement of the label mask (unmicst_amd/csrc/umx_label.hip; include/umx.h and DESIGN.md section 8.1, "Label mask").
For a stack u8[K][H][W] of uint8 probability planes, a class c and a minimum area A:

  1. object pixels: np.argmax over the planes (the FIRST maximum: a tie goes to the lower class) == c.
  2. objects: their 4-connected components, scipy.ndimage.label with its default structure, which numbers them in raster order of
     their first pixel.
  3. kept objects: area >= A, renumbered 1..N in the same order; labels int32 [H][W], 0 elsewhere.
  4. one record per kept object: area, inclusive bounding box, int64 sums of y and of x.

Also the inputs of the tests: masks (serpentine, comb, salt, blobs, ...), planes whose class rule yields a given mask, and cases(H, W)."""
import numpy as np
from scipy import ndimage

OBJECT = np.dtype([(n, "<i4") for n in ("area", "y0", "x0", "y1", "x1", "reserved")] + [("sum_y", "<i8"), ("sum_x", "<i8")])
FIELDS = ("area", "y0", "x0", "y1", "x1", "reserved", "sum_y", "sum_x")


def object_pixels(planes, cls=None):
    planes = np.asarray(planes)
    cls = planes.shape[0] - 1 if cls is None else cls
    return np.argmax(planes, axis=0) == cls


def label_mask(mask, min_area=1):
    """-> (labels int32 [H][W], table OBJECT[N]) of a boolean mask."""
    lab, n = ndimage.label(mask)                          # the default structure: 4-connected
    area = np.bincount(lab.ravel(), minlength=n + 1)
    keep = area >= min_area
    keep[0] = False
    number = np.where(keep, np.cumsum(keep), 0).astype(np.int32)   # order-keeping renumbering
    labels = number[lab]
    N = int(keep.sum())
    table = np.zeros(N, OBJECT)
    ys, xs = np.nonzero(labels)                           # raster order
    l = labels[ys, xs] - 1
    table["area"] = np.bincount(l, minlength=N)
    table["sum_y"] = np.bincount(l, weights=ys, minlength=N).astype(np.int64)   # (exact: far below 2^53)
    table["sum_x"] = np.bincount(l, weights=xs, minlength=N).astype(np.int64)
    y0, y1, x0, x1 = (np.zeros(N, np.int32) for _ in range(4))
    y0[l[::-1]] = ys[::-1]                                # the last write is the first pixel in raster order
    y1[l] = ys
    o = np.argsort(xs, kind="stable")
    x0[l[o][::-1]] = xs[o][::-1]
    x1[l[o]] = xs[o]
    table["y0"], table["y1"], table["x0"], table["x1"] = y0, y1, x0, x1
    return labels.astype(np.int32), table


def label(planes, cls=None, min_area=1):
    return label_mask(object_pixels(planes, cls), min_area)


def centroids(table):
    return table["sum_y"] / table["area"], table["sum_x"] / table["area"]


# ---- inputs ----
def planes_of(mask, K=3, cls=None, seed=0):
    """Random uint8 planes whose class rule gives exactly `mask`: on the mask plane cls is one above every lower class and EQUAL to the
    largest higher one (the tie the rule gives to the lower class); off it plane cls is 0 and a neighbouring class at least 1."""
    mask = np.asarray(mask, bool)
    cls = K - 1 if cls is None else cls
    rng = np.random.default_rng(seed)
    p = rng.integers(0, 200, (K,) + mask.shape).astype(np.int64)
    lower = p[:cls].max(axis=0) + 1 if cls > 0 else np.zeros(mask.shape, np.int64)
    higher = p[cls + 1:].max(axis=0) if cls + 1 < K else np.zeros(mask.shape, np.int64)
    p[cls] = np.where(mask, np.maximum(lower, higher), 0)
    if K > 1:
        other = (cls + 1) % K
        p[other] = np.where(mask, p[other], np.maximum(p[other], 1))
    else:
        assert mask.all()
    out = p.astype(np.uint8)
    assert np.array_equal(object_pixels(out, cls), mask)
    return out


def checker(H, W):
    yy, xx = np.mgrid[0:H, 0:W]
    return (yy + xx) % 2 == 0


def serpentine(H, W):
    """Every second row full, joined alternately at the right and the left end: one object whose chain of unions runs through every
    row of the image."""
    m = np.zeros((H, W), bool)
    m[0::2, :] = True
    for k, r in enumerate(range(1, H - 1, 2)):
        m[r, W - 1 if k % 2 == 0 else 0] = True
    return m


def comb(H, W):
    """Vertical teeth from the top row down, three columns apart, joined by the bottom row only."""
    m = np.zeros((H, W), bool)
    m[:, 0::3] = True
    m[H - 1, :] = True
    return m


def salt(H, W, seed=5, density=0.6):
    return np.random.default_rng(seed).random((H, W)) < density


def blobs(H, W, seed=3, smooth=2.0, quantile=0.72):
    """Smoothed noise thresholded into nuclei-like blobs (the recipe of trainset_border_ref.blobs on a rectangle)."""
    f = ndimage.gaussian_filter(np.random.default_rng(seed).random((H, W)), smooth, mode="constant")
    return f > np.quantile(f, quantile)


# name -> (mask builder, K, cls, plane seed, min_area)
_CASES = {
    "empty": (lambda H, W: np.zeros((H, W), bool), 3, 2, 0, 1),
    "full": (lambda H, W: np.ones((H, W), bool), 3, 2, 0, 1),
    "checker": (checker, 3, 2, 0, 1),
    "checker_min5": (checker, 3, 2, 0, 5),
    "serpentine": (serpentine, 3, 2, 1, 1),
    "comb": (comb, 3, 2, 2, 1),
    "salt": (salt, 3, 2, 3, 1),
    "salt_min5": (salt, 3, 2, 3, 5),
    "blobs": (blobs, 3, 2, 4, 1),
    "blobs_min40": (blobs, 3, 2, 4, 40),
    "cls0": (lambda H, W: blobs(H, W, seed=6), 3, 0, 5, 1),
    "k2": (lambda H, W: salt(H, W, seed=8, density=0.5), 2, 1, 6, 2),
    "k16_cls7": (lambda H, W: blobs(H, W, seed=9), 16, 7, 7, 1),
}
NAMES = tuple(_CASES)


def case(H, W, name):
    """-> (planes uint8 [K][H][W], cls, min_area)"""
    mask, K, cls, seed, min_area = _CASES[name]
    return planes_of(mask(H, W), K, cls, seed), cls, min_area


def cases(H, W):
    """name -> (planes uint8 [K][H][W], cls, min_area)"""
    return {name: case(H, W, name) for name in NAMES}
