"""numpy restatement of the rotation / zoom path (assemble_augmented_kernel<true> and assemble_resampled_labels_kernel<AugChunk> of
unmicst_amd/csrc/umx_trainset_assemble.hip; include/umx_train.h and DESIGN.md section 9.2, "Rotation and zoom"): per image and channel
page plane -> warp -> blur -> saturation -> crop orientation + dihedral transform -> jitter, and labels / weights from the nearest
source pixel.  Every product, sum, division and floor is its own float64 rounding, in the kernel's order, so the device result must
equal this bit for bit.  Images whose warp is the identity come from tests/trainset_augment_ref.py (or trainset_ref.py) unchanged."""
import numpy as np

import trainset_augment_ref as aref
import trainset_ref as ref


def is_identity(m):
    m = np.asarray(m, np.float32)
    return bool(m[0] == 1 and m[1] == 0 and m[2] == 0 and m[3] == 1)


def fold(s, S):
    """Source coordinates (float64) mirrored into 0 .. S-1 about the centres of the edge pixels (d c b | a b c d | c b a)."""
    s = np.asarray(s, np.float64)
    T = np.float64(2.0 * (S - 1))
    q = np.floor(s / T)
    t = s - T * q
    t = np.where(t > np.float64(S - 1), T - t, t)
    return np.where(t < 0.0, 0.0, t)


def source(m, ys, xs, P, y0, x0, S):
    """-> (ty, tx) float64 [len(ys), len(xs)]: where the pixels (y, x) of the crop's grid (any integers) lie in the sample, folded."""
    m = np.asarray(m, np.float32).astype(np.float64)
    c = np.float64(0.5 * (P - 1))
    dy = (np.asarray(ys, np.float64) - c)[:, None]
    dx = (np.asarray(xs, np.float64) - c)[None, :]
    sy = (m[0] * dy + m[1] * dx) + (np.float64(y0) + c)
    sx = (m[2] * dy + m[3] * dx) + (np.float64(x0) + c)
    return fold(sy, S), fold(sx, S)


def bilinear(p, ty, tx):
    """float32 value of the plane p [S][S] at folded coordinates: along the row first, then between the two rows."""
    S = p.shape[0]
    p64 = np.asarray(p, np.float32).astype(np.float64)
    iy, ix = np.minimum(np.floor(ty).astype(np.int64), S - 1), np.minimum(np.floor(tx).astype(np.int64), S - 1)
    fy, fx = ty - iy.astype(np.float64), tx - ix.astype(np.float64)
    iy1, ix1 = np.minimum(iy + 1, S - 1), np.minimum(ix + 1, S - 1)
    gx = 1.0 - fx
    top = gx * p64[iy, ix] + fx * p64[iy, ix1]
    bot = gx * p64[iy1, ix] + fx * p64[iy1, ix1]
    return ((1.0 - fy) * top + fy * bot).astype(np.float32)


def nearest(t, S):
    return np.minimum(np.floor(t + 0.5).astype(np.int64), S - 1)


def warp_plane(p, m, P, y0, x0, halo=0):
    """The warped image on the crop's grid, rows and columns -halo .. P-1+halo: float32 [P + 2 halo][P + 2 halo]."""
    g = np.arange(-halo, P + halo)
    ty, tx = source(m, g, g, P, y0, x0, p.shape[0])
    return bilinear(p, ty, tx)


def warp_nearest(a, m, P, y0, x0):
    """The nearest-pixel resampling of a label or weight plane a [S][S] on the crop's grid 0 .. P-1."""
    g = np.arange(P)
    ty, tx = source(m, g, g, P, y0, x0, a.shape[0])
    S = a.shape[0]
    return a[nearest(ty, S), nearest(tx, S)]


def assemble_warped(planes, annotations, weight_maps, desc, aug, warp, table, P, K, class_weight=None, intersect_weight=None):
    """aref.assemble_augmented with a warp matrix per image (warp: a WARP_DESC array).  aug None: no blur, gain 1 (table unused)."""
    if aug is None:
        data, labels, weights = ref.assemble(planes, annotations, weight_maps, desc, P, K, class_weight, intersect_weight)
    else:
        data, labels, weights = aref.assemble_augmented(planes, annotations, weight_maps, desc, aug, table, P, K, class_weight,
                                                        intersect_weight)
    for b, d in enumerate(desc):
        m = np.asarray(warp[b]["m"], np.float32)
        if is_identity(m):
            continue
        level, gain = (0, np.float32(1.0)) if aug is None else (int(aug[b]["blur_level"]), np.float32(aug[b]["gain"]))
        i, pg, y0, x0, t = (int(d[f]) for f in ("index", "page", "y0", "x0", "transform"))
        cont, brig = np.float64(d["contrast"]), np.float64(d["brightness"])
        for c in range(planes.shape[1]):
            if level != 0:
                taps = table.taps[level]
                R = len(taps) - 1
                # the halo holds warped pixels, so the clamp of aref.blur_plane only reaches rows and columns that are cut away
                v = aref.blur_plane(warp_plane(planes[i, c, pg], m, P, y0, x0, R), taps)[R:R + P, R:R + P]
            else:
                v = warp_plane(planes[i, c, pg], m, P, y0, x0)
            if gain != np.float32(1.0):
                v = aref.saturate(v, gain, table.mean, table.std)
            data[b, :, :, c] = (ref.transform(v, t).astype(np.float64) * cont + brig).astype(np.float32)
        code = ref.transform(warp_nearest(annotations[i], m, P, y0, x0), t)
        for k in range(K):
            labels[b, :, :, k] = code == k + 1
        if weights is not None:
            wm = weight_maps[i] if weight_maps is not None and weight_maps[i] is not None else np.zeros(annotations.shape[1:], np.float32)
            w = ref.transform(warp_nearest(np.asarray(wm, np.float32), m, P, y0, x0), t).astype(np.float64)
            for k in range(K):
                weights[b, :, :, k] = (np.float64(np.float32(intersect_weight[k])) * w + np.float64(np.float32(class_weight[k]))).astype(np.float32)
    return data, labels, weights
