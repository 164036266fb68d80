"""numpy restatement of the label mask's measurement (unmicst_amd/csrc/umx_label.hip; include/umx.h and DESIGN.md section 8.1, steps 8
and 9).  From labels int32 [H][W] with values in 0..N and planes [C][H][W] of uint8 or uint16:

  8. for every plane c and label j = 1..N, over the pixels with labels == j: count, sum, sum_sq, min, max -- record [c][j - 1].  A
     label no pixel carries: count 0, sum 0, sum_sq 0, min 2^32 - 1, max 0.  A label value < 0 or > N counts as 0.
  9. mean = sum / count, std = sqrt(max(sum_sq / count - mean * mean, 0)), in float64.

Every sum is accumulated in uint64 with np.add.at: no float weights (np.bincount with weights is inexact above 2^53)."""
from fractions import Fraction

import numpy as np

RECORD = np.dtype([("sum", "<u8"), ("sum_sq", "<u8"), ("min", "<u4"), ("max", "<u4"), ("count", "<u4"), ("reserved", "<u4")])
U32_MAX = 2 ** 32 - 1


def measure(labels, planes, N):
    """-> RECORD [C][N]"""
    labels = np.asarray(labels)
    planes = np.asarray(planes)
    if planes.ndim == 2:
        planes = planes[None]
    assert planes.dtype in (np.uint8, np.uint16) and planes.shape[1:] == labels.shape
    flat = labels.ravel().astype(np.int64)
    keep = (flat >= 1) & (flat <= N)
    idx = flat[keep] - 1
    out = np.zeros((planes.shape[0], N), RECORD)
    out["min"] = U32_MAX
    for c, plane in enumerate(planes):
        v = plane.ravel()[keep].astype(np.uint64)
        s, q, n = np.zeros(N, np.uint64), np.zeros(N, np.uint64), np.zeros(N, np.uint32)
        lo, hi = np.full(N, U32_MAX, np.uint32), np.zeros(N, np.uint32)
        np.add.at(s, idx, v)
        np.add.at(q, idx, v * v)
        np.add.at(n, idx, np.uint32(1))
        np.minimum.at(lo, idx, v.astype(np.uint32))
        np.maximum.at(hi, idx, v.astype(np.uint32))
        out["sum"][c], out["sum_sq"][c], out["count"][c], out["min"][c], out["max"][c] = s, q, n, lo, hi
    return out


def mean_std(records):
    """step 9, as stated: float64 throughout"""
    count = records["count"].astype(np.float64)
    mean = records["sum"].astype(np.float64) / count
    return mean, np.sqrt(np.maximum(records["sum_sq"].astype(np.float64) / count - mean * mean, 0.0))


def exact_mean_var(record):
    """(mean, variance) of one record as exact rationals"""
    n = int(record["count"])
    mean = Fraction(int(record["sum"]), n)
    return mean, Fraction(int(record["sum_sq"]), n) - mean * mean


def csv_lines(area, planes):
    """The Intensities file: planes = [(prefix, RECORD [N])] -> its lines, floats as write_objects_csv writes centroids"""
    head = "label,area" + "".join(",%s_mean,%s_std,%s_min,%s_max" % ((p,) * 4) for p, _ in planes)
    stats = [mean_std(r) for _, r in planes]
    lines = [head]
    for j in range(len(area)):
        line = "%d,%d" % (j + 1, area[j])
        for (_, r), (m, s) in zip(planes, stats):
            line += ",%.6f,%.6f,%d,%d" % (m[j], s[j], r["min"][j], r["max"][j])
        lines.append(line)
    return lines


def pixels(shape, dtype, C, seed):
    """Random planes [C][H][W] with 0 and the type's maximum forced in (at the first two pixels that exist, and at random places)"""
    rng = np.random.default_rng(seed)
    top = np.iinfo(dtype).max
    p = rng.integers(0, top + 1, (C,) + tuple(shape)).astype(dtype)
    hit = rng.random(p.shape)
    p[hit < 0.02] = 0
    p[hit > 0.98] = top
    flat = p.reshape(C, -1)
    flat[:, 0] = top
    flat[:, -1] = 0 if flat.shape[1] > 1 else top
    return p
