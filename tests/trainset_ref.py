"""numpy restatement of the two training-set kernels (assemble_batch_kernel of unmicst_amd/csrc/umx_trainset_assemble.hip and
class_counts_kernel of unmicst_amd/csrc/umx_trainset.hip).

``assemble`` is what assemble_batch_kernel writes for a list of descriptors; the device result must equal it bit for bit (float64
product and sum, one rounding -- numpy does not fuse them).  ``class_counts`` is class_counts_kernel on host arrays."""
import numpy as np


def transform(a, t):
    """The dihedral transform t (0..7) of a P x P crop: bit 2 swaps the axes, then bit 1 flips the rows, then bit 0 the columns."""
    if t & 4:
        a = a.T
    if t & 2:
        a = a[::-1, :]
    if t & 1:
        a = a[:, ::-1]
    return a


def assemble(planes, annotations, weight_maps, desc, P, K, class_weight=None, intersect_weight=None):
    """planes [N][C][pages][S][S] float32, annotations [N][S][S] uint8, weight_maps per sample ([S][S] or None); desc a SAMPLE_DESC
    array.  -> data [n,P,P,C], labels [n,P,P,K], weights [n,P,P,K] (None when class_weight is None: an unweighted set)."""
    n, C = len(desc), planes.shape[1]
    data = np.empty((n, P, P, C), np.float32)
    labels = np.empty((n, P, P, K), np.float32)
    weights = None if class_weight is None else np.empty((n, P, P, K), np.float32)
    for b, d in enumerate(desc):
        i, pg, y0, x0, t = (int(d[f]) for f in ("index", "page", "y0", "x0", "transform"))
        cont, brig = np.float64(d["contrast"]), np.float64(d["brightness"])
        for c in range(C):
            v = transform(planes[i, c, pg, y0:y0 + P, x0:x0 + P], t).astype(np.float64)
            data[b, :, :, c] = (v * cont + brig).astype(np.float32)
        code = transform(annotations[i, y0:y0 + P, x0:x0 + P], t)
        for k in range(K):
            labels[b, :, :, k] = code == k + 1
        if weights is not None:
            wm = weight_maps[i] if weight_maps is not None and weight_maps[i] is not None else np.zeros(annotations.shape[1:], np.float32)
            w = transform(np.asarray(wm, np.float32)[y0:y0 + P, x0:x0 + P], t).astype(np.float64)
            for k in range(K):
                weights[b, :, :, k] = (np.float64(np.float32(intersect_weight[k])) * w + np.float64(np.float32(class_weight[k]))).astype(np.float32)
    return data, labels, weights


def class_counts(probs, labels):
    """-> (counts int64 [2, K] = correct | labelled, loss_sum float64): per labelled pixel, argmax (first maximum) == label, and
    -log p[label]."""
    K = probs.shape[-1]
    p = probs.reshape(-1, K)
    lab = labels.reshape(-1, K)
    has = lab.any(axis=1)
    y = np.argmax(lab != 0, axis=1)
    am = np.argmax(p, axis=1)
    counts = np.zeros((2, K), np.int64)
    for k in range(K):
        sel = has & (y == k)
        counts[1, k] = int(sel.sum())
        counts[0, k] = int((sel & (am == k)).sum())
    py = p[np.arange(p.shape[0]), y].astype(np.float64)
    loss = float(-np.log(py[has]).sum())
    return counts, loss


# ---- fixtures cut from 'UNet sample data' 105 (tests/golden/unet_sample_105.npz: raw 832 x 960 + the reference's maps) ----
TRAIN_ORIGINS = [(y, x) for y in (0, 288, 576) for x in (0, 192, 384)]   # x < 640
VALID_ORIGINS = [(0, 704), (288, 704), (576, 704)]                         # x >= 704: disjoint from the training crops


def sample_105_codes():
    """Class codes 1..3 = 1 + argmax of (background, contours, nuclei) of the reference's probability maps (uint8), background =
    255 - contours - nuclei clipped at 0."""
    import helpers
    raw, cont, _, nuc = helpers.load_sample_105()
    c, n = cont.astype(np.int32), nuc.astype(np.int32)
    bg = np.clip(255 - c - n, 0, 255)
    return raw, (np.argmax(np.stack([bg, c, n]), axis=0) + 1).astype(np.uint8), (cont / 255.0).astype(np.float32)


def sample_105_crops(origins, S=256):
    """-> raw uint16 crops [n][S][S], codes [n][S][S] uint8, weight maps [n][S][S] float32."""
    raw, codes, wmap = sample_105_codes()
    return (np.stack([raw[y:y + S, x:x + S] for y, x in origins]), np.stack([codes[y:y + S, x:x + S] for y, x in origins]),
            np.stack([wmap[y:y + S, x:x + S] for y, x in origins]))


def normalise(raw, mean, std):
    """(im2double(raw) - mean) / std in float64, one rounding to float32 (what read_dataset_dir does)."""
    from unmicst_amd import imtools
    return ((imtools.im2double(raw) - float(mean)) / float(std)).astype(np.float32)


def write_dataset(path, raws, codes, wmaps=None, pages=1):
    """The published layout: I%05d_Img.tif (pages x channels pages, page aug + pages * channel), _Ant.tif, _wt.tif.  raws [n][S][S]
    (one channel: every page the same plane) or [n][C][pages][S][S]."""
    import os
    from unmicst_amd import tiffio
    os.makedirs(path, exist_ok=True)
    for i in range(len(raws)):
        r = np.asarray(raws[i])
        if r.ndim == 2:
            r = np.broadcast_to(r, (1, pages) + r.shape)
        C, A = r.shape[:2]
        img = os.path.join(path, "I%05d_Img.tif" % i)
        for c in range(C):
            for a in range(A):
                tiffio.imsave(img, np.ascontiguousarray(r[c, a]), append=(c, a) != (0, 0))
        tiffio.imsave(os.path.join(path, "I%05d_Ant.tif" % i), np.ascontiguousarray(codes[i]))
        if wmaps is not None and wmaps[i] is not None:
            tiffio.imsave(os.path.join(path, "I%05d_wt.tif" % i), np.ascontiguousarray(wmaps[i]))
