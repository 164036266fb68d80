"""numpy / scipy restatement of the label mask's h-maxima seeds (unmicst_amd/csrc/umx_label_hmax.hip; include/umx.h and DESIGN.md
section 8.1, steps 33 to 36), on top of tests/label_split_ref.py and tests/label_flood_ref.py.  With the kept objects of step 10 (M their
pixels), a seed plane S, an invert flag, a height h, a minimum core area C and the flood's relief plane P, invert flag and level step q:

  33. f = planes[S] on M, or 255 - planes[S] with invert; 0 off M and outside the image.
  34. g = the reconstruction by dilation of max(f - h, 0) under f, 4-connectivity.
  35. r = the reconstruction of max(g - 1, 0) under g; E = {g > r}.
  36. cores: the components of E with area >= C; seeds as step 13; the flood of steps 19 to 21 (q = 256 on any plane: the regrow by
      distance); the rim growth and the table of step 15.

A reconstruction is whole-plane dilation steps repeated to the fixed point: no tiles, no queue.  Also the inputs of the tests."""
import numpy as np
from scipy import ndimage

import label_flood_ref
import label_grow_ref
import label_ref
import label_split_ref

COUNTS = label_flood_ref.COUNTS + ("seed_pixels",)             # (`launches` and `recon_launches` are informative: no test compares them)
CROSS = ndimage.generate_binary_structure(2, 1)


def recon(marker, mask):
    """the limit of g <- min(mask, max(g, g of the four neighbours)) from the marker (outside the image counts as 0)"""
    g = np.minimum(np.asarray(marker).astype(np.int64), mask)
    while True:
        c = np.pad(g, 1, constant_values=0)
        n = np.minimum(mask, np.maximum(g, np.maximum(np.maximum(c[:-2, 1:-1], c[2:, 1:-1]), np.maximum(c[1:-1, :-2], c[1:-1, 2:]))))
        if np.array_equal(n, g):
            return g
        g = n


def hmaxima(f, h):
    """step 34"""
    f = np.asarray(f).astype(np.int64)
    return recon(np.maximum(f - h, 0), f)


def extended_maxima(g):
    """step 35, first form"""
    return g > recon(np.maximum(g - 1, 0), g)


def plateau_maxima(g):
    """step 35, second form: the 4-connected plateaus of g with value > 0 that have no 4-neighbour of greater g"""
    g = np.asarray(g).astype(np.int64)
    c = np.pad(g, 1, constant_values=0)
    higher = np.maximum(np.maximum(c[:-2, 1:-1], c[2:, 1:-1]), np.maximum(c[1:-1, :-2], c[1:-1, 2:])) > g
    E = np.zeros(g.shape, bool)
    for v in np.unique(g[g > 0]):
        lab, n = ndimage.label(g == v, CROSS)
        if n:
            bad = np.unique(lab[higher & (lab > 0)])
            E |= (lab > 0) & ~np.isin(lab, bad)
    return E


def seed_relief(planes, labels0, S, invert=False):
    """step 33"""
    v = np.asarray(planes)[S].astype(np.int64)
    return np.where(labels0 > 0, 255 - v if invert else v, 0)


def seed_set(f, h):
    """steps 34 and 35 -> E"""
    return extended_maxima(hmaxima(f, h))


def seeds_of(labels0, E, C):
    """steps 12 and 13 with a given E -> (seed labels int32 [H][W], N, n_cored); label_split_ref.seeds_of with the erosion taken out"""
    M = labels0 > 0
    cores = label_ref.label_mask(E, C)[0] > 0
    cored = np.unique(labels0[cores])
    S = cores | (M & ~np.isin(labels0, cored))
    seeds, table = label_ref.label_mask(S, 1)
    return seeds, len(table), len(cored)


def hmax(planes, cls=None, min_area=1, h=1, S=None, invert=False, C=1, P=None, q=256, flood_invert=False, R=0, classes=None):
    """-> (labels, table, counts) of uint8 planes [K][H][W]; S None: the class plane; P None: the regrow by distance"""
    planes = np.asarray(planes)
    cls = planes.shape[0] - 1 if cls is None else cls
    if R and classes is None:
        classes = label_grow_ref.default_classes(planes.shape[0], cls)
    pred = label_grow_ref.pred_of(planes)
    labels0, table0 = label_ref.label_mask(pred == cls, min_area)
    E = seed_set(seed_relief(planes, labels0, cls if S is None else S, invert), h)
    assert not (E & (labels0 == 0)).any()
    seeds, N, n_cored = seeds_of(labels0, E, C)
    if P is None:
        P, q, flood_invert = cls, 256, False
    lab, levels_claimed, claimed = label_flood_ref.flood(seeds, pred, cls, label_flood_ref.relief_of(planes, P, flood_invert), q)
    unreached = int(((labels0 > 0) & (lab == 0)).sum())
    if R:
        lab = label_grow_ref.grow(lab, pred, classes, R)
    counts = dict(n_objects=N, n_before=len(table0), n_cored=n_cored, unreached=unreached, levels_claimed=levels_claimed, claimed=claimed,
                  seed_pixels=int(E.sum()))
    return lab, label_grow_ref.table_of(lab, N), counts


# ---- inputs: K = 4; class 2 the nuclei, plane 1 the flood's relief (the rim's class), plane 3 the seed relief ----
def planes_of(mask, seed_relief_, flood_relief=None, rim=None, seed=0):
    """uint8 [4][H][W] whose first maximum is 2 on `mask`, 1 on `rim` and 0 elsewhere.  Plane 2 is 255 on the mask, plane 3 the seed
    relief there (0..254: it never wins or ties) and random 0..254 off the mask -- step 33 must not look at it there -- and plane 1
    the flood's relief on the mask."""
    mask = np.asarray(mask, bool)
    sr = np.asarray(seed_relief_)
    fr = np.zeros(mask.shape, np.int64) if flood_relief is None else np.asarray(flood_relief)
    assert sr.min() >= 0 and sr.max() <= 254 and fr.min() >= 0 and fr.max() <= 254
    p = np.zeros((4,) + mask.shape, np.uint8)
    p[0] = np.where(mask, 0, 255)
    p[1] = np.where(mask, fr, 0)
    p[2] = np.where(mask, 255, 0)
    p[3] = np.where(mask, sr, np.random.default_rng(seed).integers(0, 255, mask.shape))
    pred = np.where(mask, 2, 0)
    if rim is not None:
        rim = np.asarray(rim, bool) & ~mask
        p[0][rim], p[1][rim], p[2][rim] = 0, 255, 0
        pred = np.where(rim, 1, pred)
    assert np.array_equal(label_grow_ref.pred_of(p), pred)
    return p


def peak_places(H, W, tile=64, halo=8):
    """rows and columns on both sides of every tile seam and in the first and the last ring of a halo round it, the image's own first
    and last ones, where they fit"""
    def along(n):
        v = {0, n - 1}
        for s in range(tile, n, tile):
            v |= {s - halo, s - halo + 1, s - 1, s, s + halo - 2, s + halo - 1}
        return sorted(x for x in v if 0 <= x < n)
    return along(H), along(W)


def peak_scene(H, W, base=30, seed=4):
    """One object, the whole image (it lies on the border): a noisy relief 0..base and one-pixel peaks of heights 100..250 at every
    other crossing of peak_places' rows and columns (the i-th row with the j-th column when i + j is even: no two peaks are
    4-neighbours, and both sides of every seam carry some).  -> (mask, relief, [(y, x, height)])"""
    rng = np.random.default_rng(seed)
    relief = rng.integers(0, base + 1, (H, W))
    ys, xs = peak_places(H, W)
    peaks = []
    for i, y in enumerate(ys):
        for j, x in enumerate(xs):
            if (i + j) % 2 == 0:
                v = 100 + (7 * len(peaks)) % 151
                relief[y, x] = v
                peaks.append((y, x, v))
    return np.ones((H, W), bool), relief, peaks


def plateau_scene(H, W, tile=64, halo=8):
    """Bars three rows high over every vertical seam the image has (columns s - 20 .. s + 20 where they fit): relief 50, a flat plateau
    of 100 in the middle row from s - 14 to s + halo + 4, and at its far end, more than a halo beyond the seam, one pixel of 140.  With
    h < 40 the plateau is no maximum -- which the tile left of the seam learns only from a later launch.  A second bar below each has
    the plateau alone: that one is a maximum.  -> (mask, relief)"""
    mask = np.zeros((H, W), bool)
    relief = np.zeros((H, W), np.int64)
    for s in range(tile, W, tile):
        x0, x1 = max(s - 20, 1), min(s + 20, W - 1)
        for k, y in enumerate((3, 9)):
            if y + 3 > H or x1 - x0 < 12:
                continue
            mask[y:y + 3, x0:x1] = True
            relief[y:y + 3, x0:x1] = 50
            a, b = max(s - 14, x0 + 1), min(s + halo + 4, x1 - 2)
            relief[y + 1, a:b] = 100
            if k == 0:
                relief[y + 1, b] = 140
    return mask, relief


def serpentine_scene(H, W, gap=4, low=200, span=50):
    """A corridor one pixel wide along every `gap`-th row, joined at alternating ends: it passes through every tile.  Its relief
    rises from `low` to `low + span` along the path, so with h < span the value low + span - h has to travel back along
    (span - h) / span of the whole path.  -> (mask, relief, path)"""
    path = []
    rows = list(range(0, H, gap))
    for k, y in enumerate(rows):
        xs = range(W) if k % 2 == 0 else range(W - 1, -1, -1)
        path += [(y, x) for x in xs]
        if k + 1 < len(rows):
            x = path[-1][1]
            path += [(yy, x) for yy in range(y + 1, rows[k + 1])]
    mask = np.zeros((H, W), bool)
    relief = np.zeros((H, W), np.int64)
    n = len(path)
    for k, (y, x) in enumerate(path):
        mask[y, x] = True
        relief[y, x] = low + (k * span) // max(n - 1, 1)
    return mask, relief, path


def dome_scene(H, W, seed=3):
    """label_ref.blobs with one dome per bulge: the city-block distance to the background, scaled, plus a little noise"""
    mask = label_ref.blobs(H, W, seed=seed)
    d = ndimage.distance_transform_cdt(mask, "taxicab").astype(np.int64)
    noise = np.random.default_rng(seed).integers(0, 4, (H, W))
    return mask, np.where(mask, np.minimum(20 * d + noise, 254), 0)


def noise_scene(H, W, seed=3):
    """label_ref.blobs with a random relief 0..254 in every pixel"""
    mask = label_ref.blobs(H, W, seed=seed)
    return mask, np.where(mask, np.random.default_rng(seed + 1).integers(0, 255, (H, W)), 0)


def speck_scene(H, W):
    """one-pixel objects on a grid, every third with relief 0; a 3 x 3 object of relief 0 where it fits"""
    mask = np.zeros((H, W), bool)
    mask[::3, ::3] = True
    relief = np.where(mask, 120, 0)
    relief[::3, ::9] = 0
    if H >= 8 and W >= 8:
        mask[4:7, 4:7] = True
        relief[4:7, 4:7] = 0
    return mask, relief


def overlapping_discs(H, W, radius=14, shift=16, pitch=48):
    """pairs of discs whose centres are `shift` apart: the neck between them is far wider than 2 * 8, so no erosion of depth <= 8 cuts
    it; the seed relief is one dome per disc (the larger of the two discs' scaled distances to their own rims).
    -> (mask, relief, pairs)"""
    yy, xx = np.mgrid[:H, :W]
    mask = np.zeros((H, W), bool)
    relief = np.zeros((H, W), np.int64)
    pairs = 0
    for cy in range(radius + 2, H - radius - 2, pitch):
        for cx in range(radius + 2, W - radius - shift - 2, pitch + shift):
            for dx in (0, shift):
                d = np.sqrt((yy - cy) ** 2 + (xx - cx - dx) ** 2)
                mask |= d <= radius
                relief = np.maximum(relief, np.where(d <= radius, (250 * (radius - d) / radius).astype(np.int64), 0))
            pairs += 1
    return mask, np.where(mask, np.minimum(relief + 1, 254), 0), pairs
