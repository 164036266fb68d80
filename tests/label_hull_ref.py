"""Python restatement of the label mask's hulls (unmicst_amd/csrc/umx_label_hull.hip; include/umx.h and DESIGN.md section 8.1, steps
25 to 27).  From labels int32 [H][W] with objects 1..N (a value < 0 or > N counts as 0), for every label j:

  25. hull(j): the convex hull of the unit squares [y, y + 1] x [x, x + 1] of its pixels, on the corner lattice; strictly convex
      corners only, from the vertex with the smallest (y, x) in the direction in which sum (x_i y_{i+1} - x_{i+1} y_i) is positive.
  26. RECORD: area2 (that sum), feret_max_sq, first, n_vertices, rows.  A label no pixel carries: zeros but `first`.
  27. VERTEX: all hulls one after the other in label order.

Nothing here follows the kernels' method (row ranges, row extremes, one candidate per corner level, a gift wrap by waves): the points
are the four corners of every boundary pixel of the label -- a pixel with a 4-neighbour that is not the label's, or on the image
border --, the hull is Andrew's monotone chain over them, sorted, in Python integers, the area the shoelace sum and feret_max_sq a
brute-force maximum over all vertex pairs."""
import numpy as np
from scipy import ndimage

from label_shape_ref import clean, seeded_labels  # noqa: F401  (seeded_labels: the pattern for the chunk and row-group boundaries)

RECORD = np.dtype([("area2", "<i8"), ("feret_max_sq", "<i8"), ("first", "<i8"), ("n_vertices", "<i4"), ("rows", "<i4")])
VERTEX = np.dtype([("y", "<i4"), ("x", "<i4")])


def boundary_corners(m, y0=0, x0=0):
    """the corners (y, x) of the boundary pixels of a bool mask whose [0, 0] is image pixel (y0, x0) and which holds the whole label:
    a sorted list of distinct tuples of Python integers"""
    p = np.pad(m, 1)
    inner = p[1:-1, 1:-1] & p[:-2, 1:-1] & p[2:, 1:-1] & p[1:-1, :-2] & p[1:-1, 2:]
    ys, xs = np.nonzero(m & ~inner)
    pts = set()
    for y, x in zip((ys + y0).tolist(), (xs + x0).tolist()):
        pts.update(((y, x), (y, x + 1), (y + 1, x), (y + 1, x + 1)))
    return sorted(pts)


def all_corners(m, y0=0, x0=0):
    """the corners of every pixel of the mask: what the boundary corners must give the same hull as"""
    ys, xs = np.nonzero(m)
    pts = set()
    for y, x in zip((ys + y0).tolist(), (xs + x0).tolist()):
        pts.update(((y, x), (y, x + 1), (y + 1, x), (y + 1, x + 1)))
    return sorted(pts)


def cross(o, a, b):
    """(a - o) x (b - o) with x as the first axis and y as the second: positive when o -> a -> b turns in the list's direction"""
    return (a[1] - o[1]) * (b[0] - o[0]) - (a[0] - o[0]) * (b[1] - o[1])


def monotone_chain(pts):
    """sorted distinct (y, x) points, not all on one line -> the strictly convex hull vertices from the smallest (y, x), in the
    direction of a positive shoelace sum (Andrew's algorithm; exact: Python integers)"""
    lower, upper = [], []
    for p in pts:                                            # by (y, x) ascending: the chain on which x is largest comes first
        while len(lower) >= 2 and cross(lower[-2], lower[-1], p) <= 0:
            lower.pop()
        lower.append(p)
    for p in reversed(pts):
        while len(upper) >= 2 and cross(upper[-2], upper[-1], p) <= 0:
            upper.pop()
        upper.append(p)
    hull = lower[:-1] + upper[:-1]
    k = hull.index(min(hull))
    return hull[k:] + hull[:k]


def area2_of(hull):
    n = len(hull)
    return sum(hull[i][1] * hull[(i + 1) % n][0] - hull[(i + 1) % n][1] * hull[i][0] for i in range(n))


def feret_max_sq_of(hull):
    ys, xs = np.array([p[0] for p in hull], np.int64), np.array([p[1] for p in hull], np.int64)
    best = 0
    for i in range(len(hull)):                               # (every pair; int64 holds 2^33)
        d = (ys - ys[i]) ** 2 + (xs - xs[i]) ** 2
        best = max(best, int(d.max()))
    return best


def hull_of_mask(m, y0=0, x0=0, corners=boundary_corners):
    hull = monotone_chain(corners(m, y0, x0))
    if area2_of(hull) < 0:
        hull = [hull[0]] + hull[:0:-1]
    return hull


def hulls(labels, N, corners=boundary_corners):
    """-> (RECORD [N], VERTEX [V])"""
    lab = clean(labels, N)
    rec = np.zeros(N, RECORD)
    verts = []
    for j, box in enumerate(ndimage.find_objects(lab.astype(np.int32), max_label=N), start=1):
        rec["first"][j - 1] = len(verts)
        if box is None:
            continue
        m = lab[box] == j
        hull = hull_of_mask(m, box[0].start, box[1].start, corners)
        rec["area2"][j - 1] = area2_of(hull)
        rec["feret_max_sq"][j - 1] = feret_max_sq_of(hull)
        rec["n_vertices"][j - 1] = len(hull)
        rec["rows"][j - 1] = int(m.any(axis=1).sum())
        verts += hull
    return rec, np.array(verts, VERTEX).reshape(len(verts))


def disc(r):
    """the pixels whose centres lie within r of the centre of a (2 r + 1)^2 plane, as label 1"""
    yy, xx = np.mgrid[-r:r + 1, -r:r + 1]
    return (yy * yy + xx * xx <= r * r).astype(np.int32)


def staircase(n, step=1):
    """n pixels on a diagonal, `step` columns apart.  Two pixels attain the bound of 2 * rows + 2 vertices; from three on the inner
    corners are collinear and dropped, and the hull is a hexagon"""
    lab = np.zeros((n, step * (n - 1) + 1), np.int32)
    lab[np.arange(n), step * np.arange(n)] = 1
    return lab


def lens(m):
    """2 m + 1 rows whose left ends step in by m, m - 1, ..., 1 pixels towards the middle row and out again, the right ends
    likewise: a staircase down either diagonal on each side, convex, so that every corner level carries a vertex on both chains and
    the hull has 2 * rows + 2 of them -- the bound"""
    t = [i * (i + 1) // 2 for i in range(m + 1)]
    lab = np.zeros((2 * m + 1, 2 * t[m] + 2), np.int32)
    for k in range(2 * m + 1):
        a = t[abs(k - m)]
        lab[k, a:lab.shape[1] - a] = 1
    return lab


def hand_made():
    """[(name, labels int32, N)] -- the cases a hull by row extremes can get wrong"""
    cases = [("one pixel", np.array([[0, 0, 0], [0, 1, 0]], np.int32), 1),
             ("full plane", np.ones((5, 70), np.int32), 1),
             ("staircase of two", staircase(2), 1),
             ("staircase", staircase(9), 1),
             ("wide staircase", staircase(5, 33), 1),
             ("lens", lens(4), 1),
             ("tall lens", lens(12), 1)]                     # 25 rows, 52 vertices, 158 pixels wide
    ell = np.zeros((8, 9), np.int32)
    ell[1:7, 1:3] = 1; ell[5:7, 1:8] = 1
    cases.append(("L", ell, 1))
    ring = np.zeros((9, 70), np.int32)                       # the hull ignores the hole; its rows cross a chunk end
    ring[1:8, 2:68] = 1; ring[3:6, 4:66] = 0
    cases.append(("ring", ring, 1))
    combs = np.zeros((11, 12), np.int32)                     # two interdigitated combs: each hull covers most of the other's teeth
    combs[0, 1:11] = 1; combs[1:8, 1:11:4] = 1
    combs[10, 1:11] = 2; combs[3:10, 3:11:4] = 2
    cases.append(("combs", combs, 2))
    apart = np.zeros((40, 90), np.int32)                     # one label in two far-apart pieces: rows of its box without a pixel
    apart[1:3, 70:80] = 1; apart[30:37, 2:5] = 1; apart[12:20, 30:40] = 2
    cases.append(("far-apart pieces", apart, 2))
    gap = np.zeros((6, 8), np.int32)                         # label 2 of 3 is carried by no pixel
    gap[1:3, 1:4] = 1; gap[3:5, 4:7] = 3
    cases.append(("a label without pixels", gap, 3))
    odd = np.zeros((5, 7), np.int32)                         # values outside 1..N: counted as 0, no record addressed
    odd[1:4, 1:6] = 2; odd[2, 3] = -3; odd[0, 0] = 3; odd[4, 6] = -3; odd[0, 6] = 2 ** 31 - 1; odd[4, 0:3] = 1
    cases.append(("outside 1..N", odd, 2))
    cases.append(("N = 0", np.array([[0, 1, 2], [3, 0, -1]], np.int32), 0))
    return cases


def many_small(n_y=20, n_x=25, seed=3):
    """n_y * n_x objects of three rows each in cells of 4 x 6, every one a seeded 3 x 5 pattern with its middle row full (so that it
    is one object of three rows): several hundred objects, many to a workgroup whatever the assignment"""
    rng = np.random.default_rng(seed)
    lab = np.zeros((4 * n_y, 6 * n_x), np.int32)
    j = 0
    for cy in range(n_y):
        for cx in range(n_x):
            j += 1
            m = rng.random((3, 5)) < 0.5
            m[1, :] = True
            m[0, int(rng.integers(0, 5))] = True
            m[2, int(rng.integers(0, 5))] = True
            lab[4 * cy:4 * cy + 3, 6 * cx:6 * cx + 5][m] = j
    return lab, j
