"""numpy / scipy restatement of the object score of the validation pass (unmicst_amd/csrc/umx_trainset_objects.hip; include/umx_train.h
and DESIGN.md section 9.2, "Object score").  Per image, a P x P crop, with c the objects' class code and min_area >= 1:

  1. planes: truth = k + 1 where the one-hot label of class k is 1, else 0; pred = 1 + argmax of the probabilities (first maximum), and 0
     where truth is 0.
  2. objects: the 4-connected components (scipy.ndimage.label with its default structure) of truth == c, and those of pred == c with an
     area of at least min_area.  label = 1 + the least flat index y * P + x of the component; 0 off the objects.
  3. for a truth object t and a kept predicted object p with I shared pixels and areas a_t, a_p, in Python integers:
     matched 3 I > a_t + a_p; matched75 7 I > 3 (a_t + a_p); merged: kept p with at least two t of 2 I > a_t; split: t with at least two
     kept p of 2 I > a_p.
  4. counts = int64[8] = truth, predicted, matched, matched75, merged, split, 0, 0.

Also the hand-made planes of the tests, each with the counts it must give written out by hand, and the larger inputs of the GPU tests."""
import numpy as np
from scipy import ndimage

import trainset_border_ref as bref

OBJ, RING, BG = bref.OBJ, bref.RING, bref.BG
NAMES = ("truth", "predicted", "matched", "matched75", "merged", "split")


def planes_of(probs, labels):
    """probs, labels [n, P, P, K] -> (truth, pred) uint8 [n, P, P]."""
    labels = np.asarray(labels)
    truth = np.where((labels != 0).any(axis=-1), 1 + np.argmax(labels != 0, axis=-1), 0).astype(np.uint8)
    pred = (1 + np.argmax(np.asarray(probs), axis=-1)).astype(np.uint8)          # np.argmax: the first maximum
    return truth, plane_rule(truth, pred)


def plane_rule(truth, pred):
    """An unlabelled pixel is outside the evaluation: nothing is predicted there."""
    return np.where(np.asarray(truth) == 0, 0, pred).astype(np.uint8)


def labels_of(plane, code):
    """int32 [P][P]: 1 + the flat index of the first pixel of the 4-connected component of (plane == code); 0 off the objects."""
    plane = np.asarray(plane)
    P = plane.shape[0]
    lab, n = ndimage.label(plane == code)                 # the default structure: 4-connected
    out = np.zeros((P, P), np.int32)
    for k in range(1, n + 1):
        m = lab == k
        out[m] = 1 + int(np.flatnonzero(m)[0])
    return out


def object_counts(truth, pred, code, min_area=1):
    """One image -> (counts int64[8], truth labels, predicted labels).  The label plane of the prediction holds every component, also
    those below min_area."""
    truth = np.asarray(truth, np.uint8)
    pred = plane_rule(truth, np.asarray(pred, np.uint8))
    tl, pl = labels_of(truth, code), labels_of(pred, code)
    area_t = {int(k): int(v) for k, v in zip(*np.unique(tl[tl > 0], return_counts=True))}
    area_p = {int(k): int(v) for k, v in zip(*np.unique(pl[pl > 0], return_counts=True)) if int(v) >= int(min_area)}
    both = (tl > 0) & (pl > 0)
    pairs = {}
    for t, p in zip(tl[both].tolist(), pl[both].tolist()):
        if p in area_p:
            pairs[(t, p)] = pairs.get((t, p), 0) + 1
    matched = sum(1 for (t, p), I in pairs.items() if 3 * I > area_t[t] + area_p[p])
    matched75 = sum(1 for (t, p), I in pairs.items() if 7 * I > 3 * (area_t[t] + area_p[p]))
    inside_p, inside_t = {}, {}
    for (t, p), I in pairs.items():
        if 2 * I > area_t[t]:
            inside_p[p] = inside_p.get(p, 0) + 1
        if 2 * I > area_p[p]:
            inside_t[t] = inside_t.get(t, 0) + 1
    merged = sum(1 for v in inside_p.values() if v >= 2)
    split = sum(1 for v in inside_t.values() if v >= 2)
    return np.array([len(area_t), len(area_p), matched, matched75, merged, split, 0, 0], np.int64), tl, pl


def batch_counts(truth, pred, code, min_area=1):
    """[n, P, P] planes -> (per image int64 [n, 8], truth labels [n, P, P], predicted labels [n, P, P])."""
    out = [object_counts(t, p, code, min_area) for t, p in zip(truth, pred)]
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out]), np.stack([o[2] for o in out])


def f1(counts):
    t, p, m = (int(v) for v in counts[:3])
    return 2.0 * m / (t + p) if t + p else float("nan")


# ---- hand-made planes: name -> (truth, pred, min_area, the counts written out by hand) ----
def _bg(P):
    return np.full((P, P), BG, np.uint8)


def hand_made(P=32):
    """Every case fits a 32-pixel tile; a larger P leaves the rest background."""
    cases = {}
    # exactly IoU 1/2: a 2-pixel object, one of its pixels predicted.  I = 1, a_t = 2, a_p = 1: 3 I = 3 is not above 3.
    t, p = _bg(P), _bg(P)
    t[5, 5:7] = OBJ
    p[5, 5] = OBJ
    cases["iou_exactly_one_half"] = (t, p, 1, dict(truth=1, predicted=1, matched=0, matched75=0, merged=0, split=0))
    # exactly IoU 3/4: a 2 x 2 object, three of its pixels predicted.  I = 3, a_t = 4, a_p = 3: 9 > 7, and 21 is not above 21.
    t, p = _bg(P), _bg(P)
    t[8:10, 8:10] = OBJ
    p[8:10, 8:10] = OBJ
    p[9, 9] = BG
    cases["iou_exactly_three_quarters"] = (t, p, 1, dict(truth=1, predicted=1, matched=1, matched75=0, merged=0, split=0))
    # two nuclei divided by a one-pixel contour line, one predicted blob over both: each lies wholly inside it (2 * 48 > 48), and
    # neither is matched (3 * 48 = 144 is not above 48 + 104)
    t, p = _bg(P), _bg(P)
    t[4:12, 4:10] = OBJ
    t[4:12, 10] = RING
    t[4:12, 11:17] = OBJ
    p[4:12, 4:17] = OBJ
    cases["merge"] = (t, p, 1, dict(truth=2, predicted=1, matched=0, matched75=0, merged=1, split=0))
    cases["split"] = (p.copy(), t.copy(), 1, dict(truth=1, predicted=2, matched=0, matched75=0, merged=0, split=1))
    # two squares that share only a corner are two objects; predicted as they are
    t = bref.diagonal_touch(P)
    cases["diagonal_touch"] = (t, t.copy(), 1, dict(truth=2, predicted=2, matched=2, matched75=2, merged=0, split=0))
    # predicted components of 4 and of 5 pixels on annotated objects of 5 pixels each: 3 * 4 = 12 > 9, 7 * 4 = 28 > 27
    t, p = _bg(P), _bg(P)
    t[3, 3:8] = OBJ
    t[20, 3:8] = OBJ
    p[3, 3:7] = OBJ
    p[20, 3:8] = OBJ
    cases["min_area_1"] = (t, p, 1, dict(truth=2, predicted=2, matched=2, matched75=2, merged=0, split=0))
    cases["min_area_5"] = (t, p, 5, dict(truth=2, predicted=1, matched=1, matched75=1, merged=0, split=0))
    # a block of unlabelled pixels that holds a whole predicted object (it vanishes) and cuts another one in half: the annotated object
    # of 6 x 8 is cut to 6 x 4 on both sides
    t, p = _bg(P), _bg(P)
    t[2:8, 2:10] = OBJ
    p[2:8, 2:10] = OBJ
    p[14:18, 22:26] = OBJ
    t[0:10, 6:12] = 0
    t[12:20, 20:28] = 0
    cases["unlabelled_block"] = (t, p, 1, dict(truth=1, predicted=1, matched=1, matched75=1, merged=0, split=0))
    # nothing annotated, nothing predicted, neither
    t, p = _bg(P), _bg(P)
    p[4:9, 4:9] = OBJ
    p[20:22, 20:30] = OBJ
    cases["empty_truth"] = (t, p, 1, dict(truth=0, predicted=2, matched=0, matched75=0, merged=0, split=0))
    cases["empty_prediction"] = (p.copy(), t.copy(), 1, dict(truth=2, predicted=0, matched=0, matched75=0, merged=0, split=0))
    cases["both_empty"] = (_bg(P), _bg(P), 1, dict(truth=0, predicted=0, matched=0, matched75=0, merged=0, split=0))
    return cases


def stripes(P):
    """Vertical one-pixel stripes annotated, horizontal ones predicted: (P / 2)^2 pairs of one shared pixel each."""
    t, p = _bg(P), _bg(P)
    t[:, 0::2] = OBJ
    p[0::2, :] = OBJ
    return t, p


def shifted(A):
    """The annotation one pixel down, background moving in."""
    p = np.full(A.shape, BG, np.uint8)
    p[1:] = A[:-1]
    return p


def eroded(A):
    """The objects without their outermost pixels (4-neighbourhood), background in their place."""
    keep = ndimage.binary_erosion(A == OBJ)
    p = np.where(A == OBJ, BG, A).astype(np.uint8)
    p[keep] = OBJ
    return p


def large_cases(P):
    """name -> (truth, pred, min_area): the inputs of the GPU tests beyond the hand-made ones."""
    blobs = bref.blobs(P, 11, 1.5 if P <= 32 else 2.0, 0.7)
    cases = {"identical_blobs": (blobs, blobs.copy(), 1), "blobs_shifted": (blobs, shifted(blobs), 1), "blobs_eroded": (blobs, eroded(blobs), 1),
             "blobs_eroded_min_area_5": (blobs, eroded(blobs), 5), "stripes": stripes(P) + (1,)}
    for name, make in (("serpentine", bref.serpentine), ("checkerboard", bref.checkerboard), ("edges_and_corners", bref.edges_and_corners)):
        A = make(P)
        cases[name] = (A, A.copy(), 1)
    return cases
