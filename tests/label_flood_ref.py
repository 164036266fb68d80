"""numpy restatement of the label mask's level flood (unmicst_amd/csrc/umx_label.hip; include/umx.h and DESIGN.md section 8.1, steps 19 to
21), on top of tests/label_split_ref.py.  With the seed objects of a split run (steps 10 to 13), a relief plane P, an invert flag and a
level step q:

  19. r = planes[P], or 255 - planes[P] with invert; the levels t_j = min(255, (j + 1) q - 1), j = 0 .. 256 / q - 1, ascending.
  20. at level t the domain is label 0, pred == cls and r <= t; synchronous steps of the growth rule until one claims nothing; the next
      level starts from that state.
  21. R > 0: label_grow_ref.grow(that, pred, G, R); the table of the final labels.

Every level is visited and every step is a pass over the whole plane: no tiles and no skipping.  Also the inputs of the tests."""
import numpy as np

import label_grow_ref
import label_ref
import label_split_ref

COUNTS = label_split_ref.COUNTS + ("levels_claimed", "claimed")        # (`launches` is informative: no test compares it)
BIG = np.iinfo(np.int64).max


def levels(q):
    assert q in (1, 2, 4, 8, 16, 32, 64, 128, 256)
    return [min(255, (j + 1) * q - 1) for j in range(256 // q)]


def step(lab, domain):
    """one synchronous step of the rule of step 6 -> (labels, pixels claimed)"""
    c = np.pad(np.where(lab > 0, lab, BIG), 1, constant_values=BIG)
    least = np.minimum(np.minimum(c[:-2, 1:-1], c[2:, 1:-1]), np.minimum(c[1:-1, :-2], c[1:-1, 2:]))
    take = domain & (lab == 0) & (least < BIG)
    return np.where(take, least, lab), int(take.sum())


def flood(seeds, pred, cls, relief, q):
    """step 20 -> (labels int32 [H][W], levels_claimed, claimed)"""
    lab = np.asarray(seeds).astype(np.int64)
    of_class = np.asarray(pred) == cls
    levels_claimed = claimed = 0
    for t in levels(q):
        domain = of_class & (relief <= t)
        at_level = 0
        while True:
            lab, n = step(lab, domain)
            if n == 0:
                break
            at_level += n
        levels_claimed += at_level > 0
        claimed += at_level
    return lab.astype(np.int32), levels_claimed, claimed


def relief_of(planes, P, invert=False):
    r = np.asarray(planes)[P].astype(np.int64)
    return 255 - r if invert else r


def split_flood(planes, cls=None, min_area=1, D=1, C=1, P=0, q=16, invert=False, R=0, classes=None):
    """-> (labels, table, counts) of uint8 planes [K][H][W]"""
    planes = np.asarray(planes)
    cls = planes.shape[0] - 1 if cls is None else cls
    if R and classes is None:
        classes = label_grow_ref.default_classes(planes.shape[0], cls)
    pred = label_grow_ref.pred_of(planes)
    labels0, table0 = label_ref.label_mask(pred == cls, min_area)
    seeds, N, n_cored = label_split_ref.seeds_of(labels0, D, C)
    lab, levels_claimed, claimed = flood(seeds, pred, cls, relief_of(planes, P, invert), q)
    unreached = int(((labels0 > 0) & (lab == 0)).sum())
    if R:
        lab = label_grow_ref.grow(lab, pred, classes, R)
    counts = dict(n_objects=N, n_before=len(table0), n_cored=n_cored, unreached=unreached, levels_claimed=levels_claimed, claimed=claimed)
    return lab, label_grow_ref.table_of(lab, N), counts


# ---- inputs: K = 3, class 2 the nuclei, plane 1 (or 255 - plane 2) the relief ----
def planes_of(mask, relief, rim=None, inverted=False):
    """uint8 [3][H][W] whose first maximum is 2 on `mask`, 1 on `rim` and 0 elsewhere.  Plane 2 is 255 inside the objects and plane 1
    their relief, 0..254, so it never wins or ties the arg-max.  inverted: plane 2 is 255 - relief (>= 1) inside the objects and the
    other two are 0 there, so that P = 2 with invert reads the same relief."""
    mask = np.asarray(mask, bool)
    relief = np.asarray(relief)
    assert relief.min() >= 0 and relief.max() <= 254
    p = np.zeros((3,) + mask.shape, np.uint8)
    p[0] = np.where(mask, 0, 255)
    p[1] = 0 if inverted else relief
    p[2] = np.where(mask, 255 - relief if inverted else 255, 0)
    if rim is not None:
        rim = np.asarray(rim, bool) & ~mask
        p[0][rim], p[1][rim], p[2][rim] = 0, 255, 0
    pred = np.where(mask, 2, 0) if rim is None else np.where(mask, 2, np.where(rim, 1, 0))
    assert np.array_equal(label_grow_ref.pred_of(p), pred)
    return p


SIZE, LENGTH, DEPTH = 15, 9, 2                 # the bridged pairs: two 15 x 15 bodies, a bar of 2 DEPTH rows and 9 columns


def ridge_scene(H, W, ridges, low=None, seed=0):
    """Bridged pairs (label_split_ref.dumbbell, bar width 2 DEPTH: cut by a split of depth DEPTH) whose bars each hold a one-pixel-wide
    ridge: for the k-th (column, offset) of `ridges` a pair whose bar has its ridge in that image column, `offset` columns into the
    bar, with value 100 + 7 k; every other pixel of the objects has a relief in 0..30 (random; `low`: that constant).  -> (mask, relief,
    [(first row of the bar, first column of the bar, offset, value)]).  Pairs go into row bands from the top, side by side where they
    fit."""
    rng = np.random.default_rng(seed)
    mask = np.zeros((H, W), bool)
    relief = rng.integers(0, 31, (H, W)) if low is None else np.full((H, W), low)
    placed = []
    for k, (rx, off) in enumerate(ridges):
        assert 0 <= off < LENGTH
        bx = rx - off
        x0, x1 = bx - SIZE, bx + LENGTH + SIZE
        assert x0 >= 1 and x1 <= W - 1, (k, rx, off)
        for y in range(1, H - SIZE + 1, SIZE + 3):
            if not mask[y - 1:y + SIZE + 1, x0 - 1:x1 + 1].any():
                break
        else:
            raise AssertionError("no room for pair %d" % k)
        label_split_ref.dumbbell(mask, y, x0, 2 * DEPTH, SIZE, LENGTH)
        top = y + (SIZE - 2 * DEPTH) // 2
        relief[top:top + 2 * DEPTH, rx] = 100 + 7 * k
        placed.append((top, bx, off, 100 + 7 * k))
    return mask, np.where(mask, relief, 0), placed


def corridor_scene(H, W, level=5, ridge=90):
    """Two 7 x 7 bodies (a core of 3 x 3 at depth 2) joined by a corridor one pixel wide: along row 4 from the first body to column
    W - 5, then down that column to the second body.  Every pixel has the relief `level` but one ridge pixel at three quarters of the
    corridor: the first body's label floods three quarters of the corridor at one level, 8 steps a launch.  An image too small for
    that gets one body and a corridor along row 4 (or none at all).  -> (mask, relief, corridor pixels in order)"""
    mask = np.zeros((H, W), bool)
    path = []
    if H >= 9 and W >= 9:
        mask[1:8, 1:8] = True
        path = [(4, x) for x in range(8, W - 4)]
        if H >= 22 and W >= 16:
            path += [(y, W - 5) for y in range(5, H - 8)]
            mask[H - 8:H - 1, W - 8:W - 1] = True
        for y, x in path:
            mask[y, x] = True
    relief = np.where(mask, level, 0)
    if len(path) > 8:
        y, x = path[3 * len(path) // 4]
        relief[y, x] = ridge
    return mask, relief, path


def trap_scene(H, W, late, early, y=14):
    """Two 9 x 9 bodies A (label 1, columns 39..47) and B (label 2, columns 97..105) of one object, relief 10.  From A a corridor of
    16 pixels of relief 40 runs along row y to column 63 -- two launches of 8 steps at level 40, the last pixel claimed at the last
    step beside the tile seam -- then a gate of relief `late` at column 64, the first of the next tile, and a passage of relief 10 into
    a chamber three rows high (too thin for a core).  The chamber's other end reaches B through a gate of relief `early` that lies beside
    B's body from the start.  Whichever gate is lower opens at its own level and its label takes the whole chamber up to the other
    gate; a flood that jumps past the lower gate's level opens both at once and shares the chamber by distance.  q must be 1 .. 4."""
    assert H >= y + 6 and W >= 108 and y >= 5
    mask = np.zeros((H, W), bool)
    relief = np.full((H, W), 10)
    mask[y - 4:y + 5, 39:48] = True
    mask[y - 4:y + 5, 97:106] = True
    mask[y, 48:97] = True
    mask[y - 1:y + 2, 71:91] = True
    relief[y, 48:64] = 40
    relief[y, 64] = late
    relief[y, 96] = early
    return mask, np.where(mask, relief, 0)


def blob_scene(H, W, seed=3):
    """label_ref.blobs with a random relief 0..254 in every pixel"""
    mask = label_ref.blobs(H, W)
    return mask, np.where(mask, np.random.default_rng(seed).integers(0, 255, (H, W)), 0)
