"""numpy restatement of assemble_augmented_kernel (unmicst_amd/csrc/umx_trainset_assemble.hip): per image and
channel page plane -> separable Gaussian blur -> saturation -> crop + dihedral transform -> jitter.  Every product and every sum is its own
float64 rounding, in the kernel's order, so the device result must equal this bit for bit.  Labels, weights and every image with
(level 0, gain 1) come from tests/trainset_ref.py unchanged."""
import numpy as np

import trainset_ref as ref


def _pass(a, w, axis):
    """float32(sum over t = -R..R, ascending, of w[|t|] * a[clamp(i + t)]) along `axis`; the sum starts at 0.0."""
    R, S = len(w) - 1, a.shape[axis]
    a64 = a.astype(np.float64)
    acc = np.zeros(a.shape, np.float64)
    for t in range(-R, R + 1):
        idx = np.clip(np.arange(S) + t, 0, S - 1)
        acc = acc + np.float64(w[abs(t)]) * np.take(a64, idx, axis=axis)
    return acc.astype(np.float32)


def blur_plane(p, taps):
    """A whole S x S plane (float32) through the one-sided float32 taps w[0..R]: along the rows, rounded to float32, then down the
    columns.  The edges replicate."""
    w = np.asarray(taps, np.float32)
    return _pass(_pass(np.asarray(p, np.float32), w, 1), w, 0)


def saturate(b, gain, mean, std):
    """gain 1: the input bits.  Else back to the im2double scale, amplified, clipped at 1, normalised again (float64, one rounding per
    operation; mean / std / gain are the float32 values the table and the descriptor carry)."""
    b = np.asarray(b, np.float32)
    g = np.float32(gain)
    if g == np.float32(1.0):
        return b
    m, s = np.float64(np.float32(mean)), np.float64(np.float32(std))
    r = b.astype(np.float64) * s + m
    r2 = np.minimum(r * np.float64(g), 1.0)
    return ((r2 - m) / s).astype(np.float32)


def assemble_augmented(planes, annotations, weight_maps, desc, aug, table, P, K, class_weight=None, intersect_weight=None):
    """ref.assemble with a blur level and a gain per image (aug: an AUGMENT_DESC array; table: trainset.AugmentTable)."""
    data, labels, weights = ref.assemble(planes, annotations, weight_maps, desc, P, K, class_weight, intersect_weight)
    for b, (d, a) in enumerate(zip(desc, aug)):
        level, gain = int(a["blur_level"]), np.float32(a["gain"])
        if level == 0 and gain == np.float32(1.0):
            continue
        i, pg, y0, x0, t = (int(d[f]) for f in ("index", "page", "y0", "x0", "transform"))
        cont, brig = np.float64(d["contrast"]), np.float64(d["brightness"])
        for c in range(planes.shape[1]):
            p = planes[i, c, pg]
            if level != 0:
                p = blur_plane(p, table.taps[level])
            p = saturate(p, gain, table.mean, table.std)
            v = ref.transform(p[y0:y0 + P, x0:x0 + P], t).astype(np.float64)
            data[b, :, :, c] = (v * cont + brig).astype(np.float32)
    return data, labels, weights
