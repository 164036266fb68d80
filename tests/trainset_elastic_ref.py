"""numpy restatement of the elastic deformation path (assemble_augmented_kernel<true, true> and assemble_resampled_labels_kernel<ElasticChunk>
of unmicst_amd/csrc/umx_trainset_assemble.hip; include/umx_train.h and DESIGN.md section 9.2, "Elastic deformation"): per image and channel
page plane -> elastic + warp (one resampling) -> blur -> saturation -> crop orientation + dihedral transform -> jitter, and labels /
weights from the nearest source pixel.  Every product, sum, division and floor is its own float64 rounding, in the kernel's order, so
the device result must equal this bit for bit.  Images without a lattice (n == 0) come from tests/trainset_warp_ref.py unchanged."""
import numpy as np

import trainset_augment_ref as aref
import trainset_ref as ref
import trainset_warp_ref as wref

IDENTITY = np.array([1.0, 0.0, 0.0, 1.0], np.float32)


def weights(t, P, n):
    """Recipe 0a for integer coordinates t of one axis -> (W float64 [len(t), 4], six times the B-spline's weights; i int64 [len(t)],
    the first of the 4 lattice points)."""
    tc = np.minimum(np.maximum(np.asarray(t, np.int64), 0), P - 1).astype(np.float64)
    scale = np.float64(n - 3) / np.float64(P - 1)
    u = tc * scale
    i = np.minimum(np.floor(u).astype(np.int64), n - 4)
    f = u - i.astype(np.float64)
    g = 1.0 - f
    f2 = f * f
    f3 = f2 * f
    W = np.stack([(g * g) * g, (3.0 * f3 - 6.0 * f2) + 4.0, ((-3.0 * f3 + 3.0 * f2) + 3.0 * f) + 1.0, f3], axis=-1)
    return W, i


def displacement(d, n, ys, xs, P):
    """Recipe 0b -> (e_0, e_1) float64 [len(ys), len(xs)]: the row and column displacement of the pixels (y, x) of the crop's grid."""
    D = np.asarray(d, np.float32).astype(np.float64)
    Wy, iy = weights(ys, P, n)
    Wx, ix = weights(xs, P, n)
    out = []
    for k in range(2):
        rows = []
        for a in range(4):
            r = (iy + a)[:, None]
            c = ix[None, :]
            rows.append(((Wx[None, :, 0] * D[k][r, c] + Wx[None, :, 1] * D[k][r, c + 1]) + Wx[None, :, 2] * D[k][r, c + 2])
                        + Wx[None, :, 3] * D[k][r, c + 3])
        out.append((((Wy[:, None, 0] * rows[0] + Wy[:, None, 1] * rows[1]) + Wy[:, None, 2] * rows[2]) + Wy[:, None, 3] * rows[3]) / 36.0)
    return out[0], out[1]


def unfolded_source(m, d, n, ys, xs, P, y0, x0):
    """Recipe 1' in front of the fold -> (sy, sx) float64 [len(ys), len(xs)]."""
    m = np.asarray(m, np.float32).astype(np.float64)
    ey, ex = displacement(d, n, ys, xs, P)
    c = np.float64(0.5 * (P - 1))
    dy = (np.asarray(ys, np.float64)[:, None] + ey) - c
    dx = (np.asarray(xs, np.float64)[None, :] + ex) - c
    sy = (m[0] * dy + m[1] * dx) + (np.float64(y0) + c)
    sx = (m[2] * dy + m[3] * dx) + (np.float64(x0) + c)
    return sy, sx


def source(m, d, n, ys, xs, P, y0, x0, S):
    """-> (ty, tx) float64: where the displaced pixels lie in the sample, folded."""
    sy, sx = unfolded_source(m, d, n, ys, xs, P, y0, x0)
    return wref.fold(sy, S), wref.fold(sx, S)


def deform_plane(p, m, d, n, P, y0, x0, halo=0):
    """The deformed and warped image on the crop's grid, rows and columns -halo .. P-1+halo: float32."""
    g = np.arange(-halo, P + halo)
    ty, tx = source(m, d, n, g, g, P, y0, x0, p.shape[0])
    return wref.bilinear(p, ty, tx)


def deform_nearest(a, m, d, n, P, y0, x0):
    """The nearest-pixel resampling of a label or weight plane a [S][S] on the crop's grid 0 .. P-1."""
    g = np.arange(P)
    S = a.shape[0]
    ty, tx = source(m, d, n, g, g, P, y0, x0, S)
    return a[wref.nearest(ty, S), wref.nearest(tx, S)]


def assemble_elastic(planes, annotations, weight_maps, desc, aug, warp, elastic, table, P, K, class_weight=None, intersect_weight=None):
    """wref.assemble_warped with a lattice per image (elastic: an ELASTIC_DESC array).  aug None: no blur, gain 1; warp None: the
    identity for every image."""
    if warp is None:
        if aug is None:
            data, labels, weights_ = ref.assemble(planes, annotations, weight_maps, desc, P, K, class_weight, intersect_weight)
        else:
            data, labels, weights_ = aref.assemble_augmented(planes, annotations, weight_maps, desc, aug, table, P, K, class_weight,
                                                             intersect_weight)
    else:
        data, labels, weights_ = wref.assemble_warped(planes, annotations, weight_maps, desc, aug, warp, table, P, K, class_weight,
                                                      intersect_weight)
    for b, dsc in enumerate(desc):
        n = int(elastic[b]["n"])
        if n == 0:
            continue
        lat = np.asarray(elastic[b]["d"], np.float32)
        m = IDENTITY if warp is None else np.asarray(warp[b]["m"], np.float32)
        level, gain = (0, np.float32(1.0)) if aug is None else (int(aug[b]["blur_level"]), np.float32(aug[b]["gain"]))
        i, pg, y0, x0, t = (int(dsc[f]) for f in ("index", "page", "y0", "x0", "transform"))
        cont, brig = np.float64(dsc["contrast"]), np.float64(dsc["brightness"])
        for c in range(planes.shape[1]):
            if level != 0:
                taps = table.taps[level]
                R = len(taps) - 1
                v = aref.blur_plane(deform_plane(planes[i, c, pg], m, lat, n, P, y0, x0, R), taps)[R:R + P, R:R + P]
            else:
                v = deform_plane(planes[i, c, pg], m, lat, n, P, y0, x0)
            if gain != np.float32(1.0):
                v = aref.saturate(v, gain, table.mean, table.std)
            data[b, :, :, c] = (ref.transform(v, t).astype(np.float64) * cont + brig).astype(np.float32)
        code = ref.transform(deform_nearest(annotations[i], m, lat, n, P, y0, x0), t)
        for k in range(K):
            labels[b, :, :, k] = code == k + 1
        if weights_ is not None:
            wm = weight_maps[i] if weight_maps is not None and weight_maps[i] is not None else np.zeros(annotations.shape[1:], np.float32)
            w = ref.transform(deform_nearest(np.asarray(wm, np.float32), m, lat, n, P, y0, x0), t).astype(np.float64)
            for k in range(K):
                weights_[b, :, :, k] = (np.float64(np.float32(intersect_weight[k])) * w
                                        + np.float64(np.float32(class_weight[k]))).astype(np.float32)
    return data, labels, weights_
