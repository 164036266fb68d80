"""numpy / scipy restatement of the label mask's relabel (unmicst_amd/csrc/umx_label_relabel.hip and umx_relabel_host.h; include/umx.h and
DESIGN.md section 8.1, steps 29 to 32).  From a label plane with values 0..N, keep (N flags or None) and pairs (M pairs of labels):

 29. classes: the connected components of the graph on 1..N whose edges are the pairs (scipy.sparse.csgraph.connected_components:
     no loop and no union-find here, nothing shared with the C++).
 30. numbering: the kept classes 1..N' in order of their least member; map[0] = 0, map[j] = the number of j's class, 0 when dropped.
 31. labels' = map[labels], a value outside 0..N counting as 0.
 32. the table: label_grow_ref.table_of on labels' (step 4), a label no pixel carries having the empty record of the device.

Refused inputs (a pair outside 1..N, a pair naming a dropped label) raise ValueError here."""
import numpy as np
from scipy import sparse
from scipy.sparse import csgraph

import label_grow_ref
import label_ref

INT_MAX = 2 ** 31 - 1


def classes(N, pairs):
    """-> int64 [N + 1]: least[j] = the least member of j's class (least[0] = 0)"""
    p = np.asarray(pairs if pairs is not None else [], np.int64).reshape(-1, 2)
    if len(p) and (p.min() < 1 or p.max() > N):
        raise ValueError("a pair outside 1..%d" % N)
    graph = sparse.coo_matrix((np.ones(len(p), np.int64), (p[:, 0], p[:, 1])), shape=(N + 1, N + 1))   # (repeats add up: no int8)
    _, comp = csgraph.connected_components(graph, directed=False)
    least = np.full(comp.max() + 1, N + 1, np.int64)
    np.minimum.at(least, comp, np.arange(N + 1))
    return least[comp]


def relabel_map(N, keep=None, pairs=None):
    """-> (map int32 [N + 1], N')"""
    keep = np.ones(N, bool) if keep is None else np.asarray(keep) != 0
    assert keep.shape == (N,)
    p = np.asarray(pairs if pairs is not None else [], np.int64).reshape(-1, 2)
    least = classes(N, p)
    if len(p) and not keep[p - 1].all():
        raise ValueError("a pair names a dropped label")
    kept = np.concatenate([[False], keep])
    root = kept & (least == np.arange(N + 1))                 # the least member of every kept class, ascending
    number = np.where(root, np.cumsum(root), 0)
    m = np.where(kept, number[least], 0).astype(np.int32)
    return m, int(root.sum())


def clean(labels, N):
    labels = np.asarray(labels)
    return np.where((labels >= 0) & (labels <= N), labels, 0)


def apply(labels, N, m):
    return np.asarray(m, np.int32)[clean(labels, N)]


def table_of(labels, N):
    """step 4 on a plane with labels 1..N; a label no pixel carries: area 0, y0 = x0 = INT_MAX, y1 = x1 = -1"""
    table = label_grow_ref.table_of(labels, N)
    gone = table["area"] == 0
    table["y0"][gone] = table["x0"][gone] = INT_MAX
    table["y1"][gone] = table["x1"][gone] = -1
    return table


def relabel(labels, N, keep=None, pairs=None):
    """-> (labels' int32 [H][W], table OBJECT[N'], map int32 [N + 1])"""
    m, n_new = relabel_map(N, keep, pairs)
    out = apply(labels, N, m)
    return out, table_of(out, n_new), m


# ---- inputs ----
def chain(N):
    return np.stack([np.arange(1, N), np.arange(2, N + 1)], 1).reshape(-1, 2)


def star(N, centre):
    others = np.array([j for j in range(1, N + 1) if j != centre], np.int64)
    return np.stack([np.full(len(others), centre), others], 1).reshape(-1, 2)


def seeded_pairs(N, count, seed, among=None):
    """count pairs drawn among the labels `among` (default 1..N), with (a, a), (b, a) and repeats"""
    rng = np.random.default_rng(seed)
    pool = np.arange(1, N + 1) if among is None else np.asarray(among)
    if len(pool) == 0 or count == 0:
        return np.zeros((0, 2), np.int64)
    p = pool[rng.integers(0, len(pool), (count, 2))]
    p[::7, 1] = p[::7, 0]                                     # (a, a)
    return np.concatenate([p, p[::3, ::-1], p[::5]])          # (b, a) and repeats


def keeps(N, seed=0):
    """name -> keep, the variations every N is taken through"""
    alt = (np.arange(N) % 2 == 0)
    first, last = np.zeros(N, bool), np.zeros(N, bool)
    first[:1] = True
    last[N - 1:] = True
    return {"null": None, "none": np.zeros(N, bool), "all": np.ones(N, bool), "alternating": alt, "first only": first, "last only": last,
            "seeded": np.random.default_rng(seed).random(N) < 0.6}


def lattice(N, side=130):
    """single pixels on the even coordinates of side x side, the first N of them in raster order labelled 1..N"""
    per_row = (side + 1) // 2
    assert N <= per_row * per_row
    labels = np.zeros((side, side), np.int32)
    j = np.arange(N)
    labels[2 * (j // per_row), 2 * (j % per_row)] = j + 1
    return labels


def geometry(H, W):
    """-> (labels, N): runs that end on, before and after a chunk's end, one run that spans three chunks where W allows, a row of
    one-pixel runs, a label in two rows of two workgroups, values outside 0..N"""
    lab = np.zeros((H, W), np.int32)
    N = 0
    for y in range(H):
        x = 0
        width = 1 + y % 3
        while x < W:
            N += 1
            lab[y, x:x + width] = N
            x += width + (y + x) % 2
            width = width % 5 + 1
    if W >= 130:
        N += 1
        lab[H // 2, 1:W - 1] = N                             # one run through every chunk of the row
    if H >= 5:
        lab[4, :min(W, 3)] = lab[0, 0]                        # label 1 again, in the second workgroup
    if W >= 3:
        lab[H - 1, W - 1] = -5
        lab[0, 0] = N + 3
    return lab, N


OBJECT = label_ref.OBJECT
