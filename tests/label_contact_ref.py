"""numpy restatement of the label mask's contacts (unmicst_amd/csrc/umx_label_contact.hip; include/umx.h and DESIGN.md section 8.1,
steps 22 to 24).  From labels int32 [H][W] with objects 1..N (a value outside 1..N counts as 0):

  22. a pixel edge is a pair of horizontally or vertically adjacent pixels of the image; for a < b, edges(a, b) is the number of pixel
      edges whose two pixels carry a and b.  The list: one (a, b, edges) per pair with edges > 0, sorted by (a, b).
  23. with a reach R > 0 the same on S = the cleaned labels grown R levels (label_grow_ref.grow: the level rule of step 6) over the
      domain "label 0".

It shares nothing with the kernels' method: every horizontal and every vertical neighbour pair of the whole plane is stacked, those of
two different labels are kept, and np.unique counts them.  Also the inputs of the tests."""
import numpy as np

import label_grow_ref as grow_ref

RECORD = np.dtype([("a", "<i4"), ("b", "<i4"), ("edges", "<u4"), ("reserved", "<u4")])


def clean(labels, N):
    """the labels as int64 with every value outside 1..N set to 0"""
    lab = np.asarray(labels).astype(np.int64)
    lab[(lab < 1) | (lab > N)] = 0
    return lab


def reached(labels, N, R):
    """S of step 23: the cleaned labels grown R levels over every pixel that carries none (R = 0: the cleaned labels)"""
    lab = clean(labels, N)
    if R == 0:
        return lab
    return grow_ref.grow(lab, (lab == 0).astype(np.int64), (1,), R).astype(np.int64)


def contacts(labels, N, R=0):
    """-> RECORD [M], sorted by (a, b)"""
    lab = reached(labels, N, R)
    p = np.concatenate([lab[:, :-1].ravel(), lab[:-1, :].ravel()])
    q = np.concatenate([lab[:, 1:].ravel(), lab[1:, :].ravel()])
    keep = (p > 0) & (q > 0) & (p != q)
    p, q = p[keep], q[keep]
    key, count = np.unique((np.minimum(p, q) << 32) | np.maximum(p, q), return_counts=True)
    rec = np.zeros(len(key), RECORD)
    rec["a"], rec["b"], rec["edges"] = key >> 32, key & 0xFFFFFFFF, count
    return rec


def contacts_slow(labels, N):
    """step 22 edge by edge in Python: what contacts() is held to on small planes"""
    lab = clean(labels, N)
    H, W = lab.shape
    found = {}
    for y in range(H):
        for x in range(W):
            for yy, xx in ((y, x + 1), (y + 1, x)):
                if yy < H and xx < W:
                    a, b = int(lab[y, x]), int(lab[yy, xx])
                    if a > 0 and b > 0 and a != b:
                        k = (min(a, b), max(a, b))
                        found[k] = found.get(k, 0) + 1
    return [(a, b, n) for (a, b), n in sorted(found.items())]


def as_tuples(rec):
    return list(zip(rec["a"].tolist(), rec["b"].tolist(), rec["edges"].tolist()))


LONG = 133                                                    # the long border's pixels: past two chunk ends


def mosaic(H, W, seed=0):
    """A pattern for the chunk and row-group boundaries -> (labels int32, N): a seeded mosaic of few labels in large patches (long
    shared borders, some background, some values outside 1..N); where the plane has the room, rows 0 and 1 carry two labels side by
    side over columns 3 .. 3 + LONG - 1 -- one segment of one pair across the chunk ends at 64 and 128 -- and the last two rows hold
    one-pixel labels, every lane another pair."""
    rng = np.random.default_rng(1000 * H + W + seed)
    ph, pw = max(1, (H + 2) // 3), max(1, (W + 6) // 7)
    coarse = rng.integers(0, 6, (ph, pw))
    lab = np.kron(coarse, np.ones((3, 7), np.int64))[:H, :W]
    lab = np.roll(lab, int(rng.integers(0, 7)), axis=1)
    N = 5
    hit = rng.random((H, W))
    lab[hit < 0.02] = -3
    lab[(hit >= 0.02) & (hit < 0.04)] = N + 200               # (stays outside 1..N whatever N becomes below)
    if H >= 2 and W >= LONG + 3:
        lab[0, 3:3 + LONG] = 1
        lab[1, 3:3 + LONG] = 2
    if H >= 4:
        n1 = np.arange(W)
        lab[H - 2, :] = 6 + n1 % 97                           # one-pixel labels: 6 .. 102
        lab[H - 1, :] = 6 + (n1 * 7 + 3) % 97
        N = 102
    return lab.astype(np.int32), N


def has_long_border(labels):
    lab = np.asarray(labels)
    return lab.shape[0] >= 2 and lab.shape[1] >= LONG + 3 and (lab[0, 3:3 + LONG] == 1).all() and (lab[1, 3:3 + LONG] == 2).all()


def hand_made():
    """[(name, labels int32, N, the list known on paper or None)]"""
    cases = []
    e = np.zeros((6, 9), np.int32)
    e[1:5, 1:4] = 1
    e[1:5, 4:8] = 2
    cases.append(("edge", e, 2, [(1, 2, 4)]))
    c = np.zeros((6, 6), np.int32)
    c[0:3, 0:3] = 1
    c[3:6, 3:6] = 2
    cases.append(("corner", c, 2, []))
    H, W = 7, 70
    yy, xx = np.mgrid[0:H, 0:W]
    cases.append(("checkerboard", (1 + (yy + xx) % 2).astype(np.int32), 2, [(1, 2, H * (W - 1) + W * (H - 1))]))
    p = np.zeros((8, 12), np.int32)
    p[0:8, 5:7] = 2
    p[0:2, 2:5] = 1                                           # three pieces of label 1, each against label 2
    p[3:5, 7:10] = 1
    p[6:8, 3:5] = 1
    cases.append(("pieces", p, 2, [(1, 2, 6)]))
    r = np.zeros((9, 9), np.int32)
    r[1:8, 1:8] = 2
    r[3:6, 3:6] = 1
    cases.append(("enclosed", r, 2, [(1, 2, 12)]))
    o = np.zeros((5, 8), np.int32)
    o[1:4, 1:3] = 1
    o[1:4, 3:5] = 9                                           # outside 1..N between two real labels: no contact through it
    o[1:4, 5:7] = 2
    o[0, 1:7] = -4
    o[4, 1:3] = 2 ** 31 - 1
    o[4, 5:7] = 1
    cases.append(("outside 1..N", o, 2, [(1, 2, 2)]))
    cases.append(("N = 0", e.copy(), 0, []))
    cases.append(("one label", np.ones((5, 67), np.int32), 1, []))
    return cases
