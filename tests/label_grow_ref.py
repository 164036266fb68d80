"""numpy restatement of the label mask's growth (unmicst_amd/csrc/umx_label.hip; include/umx.h and DESIGN.md section 8.1, steps 6 and 7),
on top of tests/label_ref.py.  With pred = the first-maximum class of every pixel, labels0 = the label mask of class c with minimum area A
(label_ref.label: the seeds, numbered 1..N), a radius R >= 1 and a set G of classes:

  6. domain: labels0 == 0 and pred in G.  R synchronous levels: at each one every domain pixel that is still 0 and has a labelled
     4-neighbour takes the smallest label among them; all pixels decide on the state of the level before.  Outside the image is nothing.
  7. the table is that of the grown labels: N records, numbered as the seeds are.

Also the inputs of the tests.  Each is built as a map of classes (`pred`) and turned into uint8 planes whose first maximum is exactly
that map (planes_of_pred: label_ref.planes_of for every class at once)."""
import heapq

import numpy as np
from scipy import ndimage

import label_ref

BIG = np.iinfo(np.int64).max


def pred_of(planes):
    return np.argmax(np.asarray(planes), axis=0)


def grow(labels0, pred, classes, R):
    """-> int32 [H][W]: labels0 grown R levels over the pixels whose pred is in `classes`"""
    labels0 = np.asarray(labels0)
    domain = (labels0 == 0) & np.isin(pred, sorted(classes))
    lab = labels0.astype(np.int64)
    for _ in range(R):
        c = np.pad(np.where(lab > 0, lab, BIG), 1, constant_values=BIG)
        least = np.minimum(np.minimum(c[:-2, 1:-1], c[2:, 1:-1]), np.minimum(c[1:-1, :-2], c[1:-1, 2:]))
        take = domain & (lab == 0) & (least < BIG)
        if not take.any():
            break                                             # a level that claims nothing: no later one can
        lab = np.where(take, least, lab)
    return lab.astype(np.int32)


def table_of(labels, N):
    """-> OBJECT[N]: area, inclusive box and coordinate sums of labels 1..N of a label plane (every one of them present)"""
    table = np.zeros(N, label_ref.OBJECT)
    ys, xs = np.nonzero(labels)                               # raster order
    l = labels[ys, xs] - 1
    table["area"] = np.bincount(l, minlength=N)
    table["sum_y"] = np.bincount(l, weights=ys, minlength=N).astype(np.int64)   # (exact: far below 2^53)
    table["sum_x"] = np.bincount(l, weights=xs, minlength=N).astype(np.int64)
    y0, y1, x0, x1 = (np.zeros(N, np.int32) for _ in range(4))
    y0[l[::-1]] = ys[::-1]                                    # the last write is the first pixel in raster order
    y1[l] = ys
    o = np.argsort(xs, kind="stable")
    x0[l[o][::-1]] = xs[o][::-1]
    x1[l[o]] = xs[o]
    table["y0"], table["y1"], table["x0"], table["x1"] = y0, y1, x0, x1
    return table


def default_classes(K, cls):
    return tuple(k for k in range(1, K) if k != cls)


def label_grow(planes, cls=None, min_area=1, R=0, classes=None):
    """-> (labels int32 [H][W], table OBJECT[N]) of the planes: label_ref.label, then the growth when R > 0"""
    planes = np.asarray(planes)
    cls = planes.shape[0] - 1 if cls is None else cls
    labels0, table0 = label_ref.label(planes, cls, min_area)
    if R == 0:
        return labels0, table0
    classes = default_classes(planes.shape[0], cls) if classes is None else classes
    grown = grow(labels0, pred_of(planes), classes, R)
    return grown, table_of(grown, len(table0))


def nearest_seed(labels0, pred, classes, R):
    """The third consequence as a definition of its own, sharing no code with grow(): every pixel reached within R steps through the
    domain takes the label of a seed at the least distance, the smaller label on a tie -- one pass over a heap ordered by
    (distance, label)."""
    H, W = labels0.shape
    domain = (labels0 == 0) & np.isin(pred, sorted(classes))
    out = np.zeros((H, W), np.int32)
    heap = [(0, int(labels0[y, x]), int(y), int(x)) for y, x in zip(*np.nonzero(labels0))]
    heapq.heapify(heap)
    while heap:
        d, l, y, x = heapq.heappop(heap)
        if out[y, x]:
            continue
        out[y, x] = l
        if d == R:
            continue
        for ny, nx in ((y - 1, x), (y + 1, x), (y, x - 1), (y, x + 1)):
            if 0 <= ny < H and 0 <= nx < W and domain[ny, nx] and not out[ny, nx]:
                heapq.heappush(heap, (d + 1, l, ny, nx))
    return out


def connected(labels, N):
    """every label 1..N is one 4-connected component"""
    return all(ndimage.label(labels == l)[1] == 1 for l in range(1, N + 1))


# ---- inputs ----
def planes_of_pred(pred, K=3, seed=0):
    """Random uint8 planes whose first maximum is exactly `pred`: at each pixel the plane of its class is one above every lower class
    and EQUAL to the largest higher one (the tie the rule gives to the lower class)."""
    pred = np.asarray(pred)
    assert pred.min() >= 0 and pred.max() < K
    p = np.random.default_rng(seed).integers(0, 200, (K,) + pred.shape).astype(np.int64)
    out = p.copy()
    for c in range(K):
        lower = p[:c].max(axis=0) + 1 if c > 0 else np.zeros(pred.shape, np.int64)
        higher = p[c + 1:].max(axis=0) if c + 1 < K else np.zeros(pred.shape, np.int64)
        out[c] = np.where(pred == c, np.maximum(lower, higher), p[c])
    out = out.astype(np.uint8)
    assert np.array_equal(pred_of(out), pred)
    return out


def ring_bodies(H, W):
    """(bodies, nuclei): label_ref.blobs(seed=4, quantile=0.6), and the bodies eroded twice (4-connected, the image's edge erodes too)"""
    bodies = label_ref.blobs(H, W, seed=4, quantile=0.6)
    return bodies, ndimage.binary_erosion(bodies, iterations=2)


def rings(H, W):
    """nuclei (class 2) inside their contour rims (class 1): the erosion splits many a body into several nuclei"""
    bodies, nuclei = ring_bodies(H, W)
    return np.where(nuclei, 2, np.where(bodies, 1, 0))


def far(H, W):
    """rings whose every second body lost its nuclei to the background: its rim is a domain component with no seed at all"""
    bodies, nuclei = ring_bodies(H, W)
    body = ndimage.label(bodies)[0]
    return np.where(nuclei & (body % 2 == 1), 2, np.where(bodies, 1, 0))


def path(H, W, tile):
    """A simple 4-connected path of pixels, one pixel wide (no pixel of it touches a third one).  Where the image has the room it
    zigzags down the two columns on either side of the kernel's first tile boundary, x = tile - 1 and x = tile, crossing it at every
    third step -- as often as a simple path can -- then runs along the bottom row away from the zigzag and up the image's first or last
    column, across the tile boundaries there.  In an image too narrow
    for that it is the image's first column, or its first row when that is the longer one."""
    if W <= tile + 1 or H < 4:
        p = [(y, 0) for y in range(H)] if H >= W else [(0, x) for x in range(W)]
    else:
        p, side = [], 0
        for y in range(H):
            if y % 2 == 0:
                p += [(y, tile - 1 + side), (y, tile - side)]                 # across the boundary
                side = 1 - side
            else:
                p.append((y, tile - 1 + side))
        if p[-1][1] == tile - 1:                               # away from the zigzag: left and up the first column
            p += [(H - 1, x) for x in range(tile - 2, -1, -1)] + [(y, 0) for y in range(H - 2, -1, -1)]
        elif W - 1 >= tile + 3:                               # or right and up the last one
            p += [(H - 1, x) for x in range(tile + 1, W)] + [(y, W - 1) for y in range(H - 2, -1, -1)]
    s = set(p)
    assert len(s) == len(p)
    for i, (y, x) in enumerate(p):                            # neighbours in the set: the one before and the one after, nothing else
        near = {(y - 1, x), (y + 1, x), (y, x - 1), (y, x + 1)} & s
        assert near == set(p[max(0, i - 1):i] + p[i + 1:i + 2]), (i, y, x)
    return p


def _along(H, W, p, seeds):
    pred = np.zeros((H, W), np.int64)
    for y, x in p:
        pred[y, x] = 1
    for y, x in seeds:
        pred[y, x] = 2
    return pred


def corridor(H, W, tile, halo):
    """the path as domain with one seed, its first pixel: R levels claim exactly min(R, len(path) - 1) pixels"""
    p = path(H, W, tile)
    return _along(H, W, p, p[:1])


def duel(H, W, tile, halo, length):
    """the first `length` domain pixels of the path (fewer where the image has no room) between two seeds: the fronts meet at level
    ceil(length / 2), which is halo + 1 for length 2 halo + 1 and 2 halo + 2 -- in the second launch, on the tile boundary"""
    p = path(H, W, tile)[:length + 2]
    return _along(H, W, p, [p[0], p[-1]] if len(p) > 1 else p)


def tie(H, W):
    """Single domain pixels between two seeds, in the four arrangements: the smaller label above, below, left of and right of the
    pixel.  A seed's number is the raster rank of its FIRST pixel, so the seed below (right) gets the smaller label through an arm that
    reaches two rows higher than the other seed, away from the pixel.  Arrangements that do not fit into the image are left out."""
    pred = np.zeros((H, W), np.int64)
    blocks = {
        "above": ([(1, 1)], [(0, 1)], [(2, 1)]),
        "below": ([(3, 1)], [(2, 1)], [(4, 1), (4, 2), (4, 3), (3, 3), (2, 3), (1, 3), (0, 3)]),
        "left": ([(1, 2)], [(1, 1)], [(1, 3)]),
        "right": ([(2, 2)], [(2, 1)], [(2, 3), (1, 3), (0, 3)]),
    }
    where = {}
    x0 = 0
    for name, (mid, a, b) in blocks.items():
        h = 1 + max(y for y, _ in mid + a + b)
        w = 2 + max(x for _, x in mid + a + b)
        oy = 0 if name in ("above", "left") else 1            # (distinct first rows, so that no two first pixels share a raster rank by chance)
        if name == "left" and H == 1:
            mid, a, b, h = [(0, 2)], [(0, 1)], [(0, 3)], 1
        if oy + h <= H and x0 + w <= W:
            for y, x in mid:
                pred[oy + y, x0 + x] = 1
                where[name] = (oy + y, x0 + x)
            for y, x in a + b:
                pred[oy + y, x0 + x] = 2
            x0 += w + 1
    return pred, where


# name -> (H, W, tile, halo) -> (pred, cls, min_area, classes); K = 3 throughout, class 2 the nuclei
_CASES = {
    "rings": lambda H, W, T, h: (rings(H, W), 2, 1, (1,)),
    "corridor": lambda H, W, T, h: (corridor(H, W, T, h), 2, 1, (1,)),
    "duel_odd": lambda H, W, T, h: (duel(H, W, T, h, 2 * h + 1), 2, 1, (1,)),
    "duel_even": lambda H, W, T, h: (duel(H, W, T, h, 2 * h + 2), 2, 1, (1,)),
    "tie": lambda H, W, T, h: (tie(H, W)[0], 2, 1, (1,)),
    "cls_in_G": lambda H, W, T, h: (rings(H, W), 2, 12, (1, 2)),
    "far": lambda H, W, T, h: (far(H, W), 2, 1, (1,)),
    "empty": lambda H, W, T, h: (np.zeros((H, W), np.int64), 2, 1, (1,)),
    "full": lambda H, W, T, h: (np.ones((H, W), np.int64), 2, 1, (1,)),
}
NAMES = tuple(_CASES)


def case(H, W, name, tile, halo):
    """-> (planes uint8 [3][H][W], cls, min_area, classes)"""
    pred, cls, min_area, classes = _CASES[name](H, W, tile, halo)
    return planes_of_pred(pred, 3, seed=NAMES.index(name)), cls, min_area, classes
