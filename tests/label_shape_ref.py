"""numpy / scipy restatement of the label mask's shapes (unmicst_amd/csrc/umx_label.hip; include/umx.h and DESIGN.md section 8.1, steps
16 to 18).  From labels int32 [H][W] with objects 1..N (a value < 0 or > N counts as 0), for every label j with M_j = (labels == j)
padded with one ring of 0:

  16. the sums of y, x, y * y, y * x, x * x over M_j, and the numbers of 2x2 windows of the padded mask that hold one pixel of M_j
      (q1), two that share an edge (q2), two on a diagonal (qd), three (q3), four (q4).  A label no pixel carries: all zeros.
  17. 4 * area = q1 + 2 q2 + 2 qd + 3 q3 + 4 q4; edges = q1 + q2 + 2 qd + q3; euler = (q1 - q3 + 2 qd) / 4; holes = 1 - euler for a
      4-connected object.

Nothing here follows the kernel's method (row runs, closed forms, one owner pixel per window): the moments are np.bincount over int64
coordinate planes (or Python integers where a float64 weight sum could round), the windows are counted label by label by comparing
the four shifted views of the label's own padded mask, `edges` differences that mask along both axes, and `holes` is
scipy.ndimage.label on its complement with the 3x3 structure."""
import numpy as np
from scipy import ndimage

RECORD = np.dtype([(n, "<i8") for n in ("sum_y", "sum_x", "sum_yy", "sum_xy", "sum_xx")] +
                  [(n, "<u4") for n in ("q1", "q2", "qd", "q3", "q4", "reserved")])
MOMENTS = ("sum_y", "sum_x", "sum_yy", "sum_xy", "sum_xx")
QUADS = ("q1", "q2", "qd", "q3", "q4")


def clean(labels, N):
    """the labels as int64 with every value outside 1..N set to 0"""
    lab = np.asarray(labels).astype(np.int64)
    lab[(lab < 1) | (lab > N)] = 0
    return lab


def moments(lab, N, exact=None):
    """-> {name: int64 [N]}.  np.bincount sums its weights in float64, which is exact while every partial sum stays below 2^53: the
    bound used is pixels * (largest coordinate)^2.  Past it (or with exact=True) the sums are Python integers, pixel by pixel."""
    H, W = lab.shape
    yy, xx = np.mgrid[0:H, 0:W].astype(np.int64)
    planes = {"sum_y": yy, "sum_x": xx, "sum_yy": yy * yy, "sum_xy": yy * xx, "sum_xx": xx * xx}
    if exact is None:
        exact = H * W * max(H - 1, W - 1, 1) ** 2 >= 2 ** 53
    out = {}
    flat = lab.ravel()
    for name, plane in planes.items():
        if exact:
            acc = [0] * (N + 1)
            for j, v in zip(flat.tolist(), plane.ravel().tolist()):
                acc[j] += v
            out[name] = np.array(acc[1:], dtype=np.int64).reshape(N)
        else:
            s = np.bincount(flat, weights=plane.ravel().astype(np.float64), minlength=N + 1)[1:N + 1]
            out[name] = s.astype(np.int64)
    return out


def padded_masks(lab, N):
    """(j, M_j cut to the label's bounding box and padded with one ring of 0) for every label j in 1..N that a pixel carries: a
    window outside that box holds no pixel of M_j, so nothing is lost"""
    for j, box in enumerate(ndimage.find_objects(lab.astype(np.int32), max_label=N), start=1):
        if box is not None:
            yield j, np.pad(lab[box] == j, 1)


def window_counts(m):
    """q1, q2, qd, q3, q4 of one padded mask: its four shifted views are the four corners of every 2x2 window"""
    a, b, c, d = m[:-1, :-1], m[:-1, 1:], m[1:, :-1], m[1:, 1:]
    n = a.astype(np.int64) + b + c + d
    two = n == 2
    diagonal = two & (a == d)                                # a and d, or neither of them and so b and c
    return (int((n == 1).sum()), int(two.sum() - diagonal.sum()), int(diagonal.sum()), int((n == 3).sum()), int((n == 4).sum()))


def edge_count(m):
    """pixel edges between the mask and its complement (the ring of 0 makes the image border one)"""
    return int((m[1:, :] != m[:-1, :]).sum() + (m[:, 1:] != m[:, :-1]).sum())


def hole_count(m):
    """8-connected components of the padded complement, less the one that holds the ring"""
    return int(ndimage.label(~m, structure=np.ones((3, 3), int))[1]) - 1


def shapes(labels, N, exact=None):
    """-> (RECORD [N], edges int64 [N], holes int64 [N], area int64 [N]); a label no pixel carries has 0 everywhere (holes too)"""
    lab = clean(labels, N)
    rec = np.zeros(N, RECORD)
    for name, v in moments(lab, N, exact).items():
        rec[name] = v
    edges, holes = np.zeros(N, np.int64), np.zeros(N, np.int64)
    for j, m in padded_masks(lab, N):
        q = window_counts(m)
        for name, v in zip(QUADS, q):
            rec[name][j - 1] = v
        edges[j - 1], holes[j - 1] = edge_count(m), hole_count(m)
    area = np.bincount(lab.ravel(), minlength=N + 1)[1:N + 1].astype(np.int64)
    return rec, edges, holes, area


def records(labels, N):
    return shapes(labels, N)[0]


def seeded_labels(H, W, seed=0):
    """A pattern for the chunk and row-group boundaries: per row, runs whose ends fall on, before and after columns 63 / 64 (and 127 /
    128), runs of one pixel, one run longer than 128 pixels where the row has room, gaps; the labels 1..N are spread so that a label
    has pieces in several rows and neighbours of other labels above, below and diagonally.  -> (labels int32, N)"""
    rng = np.random.default_rng(1000 * H + W + seed)
    N = 7
    lab = np.zeros((H, W), np.int32)
    cuts = [0, 1, 2, 5, 31, 62, 63, 64, 65, 66, 100, 126, 127, 128, 129, 130, 160, 199, 200]
    for y in range(H):
        xs = sorted(set(c + (y % 3) - 1 for c in cuts if 0 <= c + (y % 3) - 1 < W) | {0})
        for i, x0 in enumerate(xs):
            x1 = xs[i + 1] if i + 1 < len(xs) else W
            lab[y, x0:x1] = int(rng.integers(0, N + 1))
        if y % 4 == 1 and W > 140:
            lab[y, 3:3 + 133] = 1 + y % N                    # one run longer than two chunks
        if y % 4 == 2:
            lab[y, ::2] = 0                                  # a row of one-pixel runs
    if lab.max() < N:
        lab.flat[0] = N                                      # (so that N is the largest label present whatever the size)
    return lab, N


def hand_made():
    """[(name, labels int32, N, {label: euler} known on paper)] -- the cases the window rule can get wrong"""
    cases = []
    b = np.zeros((12, 15), np.int32)                         # objects on every border and in every corner
    b[0, 0] = 1; b[0:2, 13:15] = 2; b[10:12, 0] = 3; b[11, 14] = 4
    b[0, 5:9] = 5; b[4:8, 0] = 6; b[3:9, 14] = 7; b[11, 3:11] = 8; b[10, 6] = 8
    cases.append(("borders", b, 8, {j: 1 for j in range(1, 9)}))
    ring = np.zeros((9, 70), np.int32)                       # one hole; its top and bottom rows cross a chunk end
    ring[1:8, 2:68] = 1; ring[3:6, 4:66] = 0
    cases.append(("ring", ring, 1, {1: 0}))
    frame = np.zeros((7, 11), np.int32)                      # two holes
    frame[:, :] = 1; frame[1:6, 1:5] = 0; frame[1:6, 6:10] = 0
    cases.append(("frame", frame, 1, {1: -1}))
    diag = np.ones((5, 5), np.int32)                         # two missing pixels that touch diagonally: one hole (8-connected background)
    diag[1, 1] = 0; diag[2, 2] = 0
    cases.append(("diagonal holes", diag, 1, {1: 0}))
    corner = np.zeros((6, 6), np.int32)                      # two labels meeting only at a corner
    corner[1:3, 1:3] = 1; corner[3:5, 3:5] = 2
    cases.append(("corner", corner, 2, {1: 1, 2: 1}))
    edge = np.zeros((4, 8), np.int32)                        # two labels along an edge, and one above the other
    edge[1:3, 1:4] = 1; edge[1:3, 4:7] = 2; edge[3, 1:7] = 3
    cases.append(("edge", edge, 3, {1: 1, 2: 1, 3: 1}))
    pieces = np.zeros((5, 9), np.int32)                      # one label in three 4-connected pieces, two of them touching diagonally: euler 3
    pieces[1:3, 1:3] = 1; pieces[3, 6] = 1; pieces[2, 7] = 1
    cases.append(("pieces", pieces, 1, {1: 3}))
    yy, xx = np.mgrid[0:6, 0:67]
    cases.append(("checkerboard", ((yy + xx) % 2 == 0).astype(np.int32), 1, {}))
    odd = np.zeros((5, 7), np.int32)                         # values outside 1..N: counted as 0, no record addressed
    odd[1:4, 1:6] = 2; odd[2, 3] = -3; odd[0, 0] = 3; odd[4, 6] = -3; odd[0, 6] = 2 ** 31 - 1; odd[4, 0:3] = 1
    cases.append(("outside 1..N", odd, 2, {1: 1, 2: 0}))
    cases.append(("N = 0", np.array([[0, 1, 2], [3, 0, -1]], np.int32), 0, {}))
    return cases
