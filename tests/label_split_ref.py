"""numpy / scipy restatement of the label mask's split at the necks (unmicst_amd/csrc/umx_label.hip; include/umx.h and DESIGN.md section
8.1, steps 10 to 15), on top of tests/label_ref.py and tests/label_grow_ref.py.  With pred = the first-maximum class of every pixel, a class
c, a minimum area A, a depth D, a minimum core area C, a regrow bound L and optionally a rim growth R over the classes G:

  10. objects: label_ref.label(planes, c, A): the kept objects, N0 of them; M = their pixels.
  11. erosion: E = scipy.ndimage.binary_erosion(M, cross, iterations=D, border_value=0).
  12. cores: the 4-connected components of E with area >= C; an object that contains one is cored.
  13. seeds: S = the cores' pixels and every pixel of the kept objects that are not cored; label_ref.label_mask(S, 1) numbers them 1..N.
  14. regrow: label_grow_ref.grow(seeds, pred, [c], L); unreached = the pixels of M still 0.
  15. R > 0: label_grow_ref.grow(that, pred, G, R); the table of the final labels.

Also the inputs of the tests."""
import numpy as np
from scipy import ndimage

import label_grow_ref
import label_ref

CROSS = ndimage.generate_binary_structure(2, 1)
COUNTS = ("n_objects", "n_before", "n_cored", "unreached")


def erode(M, D):
    return ndimage.binary_erosion(M, CROSS, iterations=D, border_value=0)


def seeds_of(labels0, D, C):
    """steps 11 to 13 -> (seed labels int32 [H][W], N, n_cored)"""
    M = labels0 > 0
    cores = label_ref.label_mask(erode(M, D), C)[0] > 0
    cored = np.unique(labels0[cores])                         # (no 0 among them: a core lies in M)
    S = cores | (M & ~np.isin(labels0, cored))
    seeds, table = label_ref.label_mask(S, 1)
    return seeds, len(table), len(cored)


def split_pred(pred, cls, min_area, D, C=1, L=255, R=0, classes=None):
    """-> (labels int32 [H][W], table OBJECT[N], counts dict) of a map of classes"""
    pred = np.asarray(pred)
    labels0, table0 = label_ref.label_mask(pred == cls, min_area)
    seeds, N, n_cored = seeds_of(labels0, D, C)
    lab = label_grow_ref.grow(seeds, pred, [cls], L)
    unreached = int(((labels0 > 0) & (lab == 0)).sum())
    if R:
        lab = label_grow_ref.grow(lab, pred, classes, R)
    counts = dict(n_objects=N, n_before=len(table0), n_cored=n_cored, unreached=unreached)
    return lab, label_grow_ref.table_of(lab, N), counts


def split(planes, cls=None, min_area=1, D=1, C=1, L=255, R=0, classes=None):
    """-> (labels, table, counts) of uint8 planes [K][H][W]"""
    planes = np.asarray(planes)
    cls = planes.shape[0] - 1 if cls is None else cls
    if R and classes is None:
        classes = label_grow_ref.default_classes(planes.shape[0], cls)
    return split_pred(label_grow_ref.pred_of(planes), cls, min_area, D, C, L, R, classes)


# ---- inputs ----
def dumbbell(mask, y, x, w, size=15, length=5):
    """Two size x size squares, the first with its corner at (y, x), joined by a bar of `w` rows and `length` columns whose rows are
    centred on the squares' (the extra row of an even w lies below).  Drawn into the boolean `mask`; -> the columns it spans."""
    top = y + (size - w) // 2
    mask[y:y + size, x:x + size] = True
    mask[y:y + size, x + size + length:x + 2 * size + length] = True
    mask[top:top + w, x + size:x + size + length] = True
    return 2 * size + length


def bridge(w, size=15, length=5, margin=2):
    """one dumbbell in an image of its own, `margin` pixels of background round it"""
    m = np.zeros((size + 2 * margin, 2 * size + length + 2 * margin), bool)
    dumbbell(m, margin, margin, w, size, length)
    return m


def bridges_at(H, W, D, places, size=15, length=5):
    """dumbbells of bar width 2 D (cut) with their bar's first pixel near each (y, x) of `places`, where they fit into the image"""
    m = np.zeros((H, W), bool)
    for y, x in places:
        y0, x0 = y - size // 2, x - size - length // 2
        if y0 >= 0 and x0 >= 0 and y0 + size <= H and x0 + 2 * size + length <= W and not m[max(y0 - 1, 0):y0 + size + 1, max(x0 - 1, 0):x0 + 2 * size + length + 1].any():
            dumbbell(m, y0, x0, 2 * D, size, length)
    return m


def mixture(H, W, D):
    """label_ref.blobs (objects that split, single-cored ones and ones too thin for a core) with dumbbells across the kernels'
    boundaries drawn over a cleared margin: the tile corner (64, 64), the strip seam at row 32 and the end of a 64-pixel chunk"""
    m = label_ref.blobs(H, W)
    extra = bridges_at(H, W, D, [(64, 64), (32, 100), (100, 128), (120, 40)])
    m &= ~ndimage.binary_dilation(extra, iterations=2)
    return m | extra


def rimmed_pairs(H, W, D=2):
    """a map of classes like label_grow_ref.rings, but with nuclei that touch: dumbbells (class 2) of bar width 2 D on a grid, every
    other one with a bar one row wider (not cut), inside a rim (class 1) two pixels wide; 0 elsewhere"""
    nuclei = np.zeros((H, W), bool)
    k = 0
    for y in range(3, H - 17, 22):
        for x in range(3 + (y % 3), W - 38, 42):
            dumbbell(nuclei, y, x, 2 * D + (k % 2), 15, 5)
            k += 1
    bodies = ndimage.binary_dilation(nuclei, CROSS, iterations=2)
    return np.where(nuclei, 2, np.where(bodies, 1, 0))
