"""Images/s of a training step fed from the device-resident training set (Trainer.step_sampled) against the host-fed step
(numpy batch assembly -- crop, augmentation page, dihedral transform, jitter, one-hot labels, weight maps -- then Trainer.step),
in one process, alternating the two, on the same descriptor stream.  Every step reads its loss (one synchronisation per step on
both paths).  A third leg, "augmented", is Trainer.step_augmented with every image at the largest blur level of the sigmas
0.75, 1.5, 3 and gain 2 -- the worst case of the computed defocus / saturation -- alternated with the other two in the same process,
so that step_sampled of the same run is its yardstick.  A fourth leg, "warped", is Trainer.step_warped with the same blur and gain and
every image rotated by 30 degrees at zoom 1.25, alternated in the same way.  A fifth leg, "elastic", is Trainer.step_elastic with the
warped leg's settings plus a 5 x 5 lattice (2 spline cells, sigma 4 pixels) on every image.  Then the validation pass
(Trainer.evaluate) over the whole set.  One JSON line per (shape, path, repeat).  --paths picks the legs (for a profile of one of them).
--objects adds the object-score leg: the validation pass over a set of blob annotations (random codes have no objects worth the name),
alternating Trainer.evaluate without and with ObjectOptions in the same process, so that the plain pass of the same run is the yardstick;
one line per (shape, repeat) with the milliseconds per validation batch of both and the object counts.

    python tools/bench_trainset.py [--steps 30] [--warmup 5] [--repeats 3] [--shapes nucleiDAPI,v2-256]
                                   [--paths step_sampled,augmented,warped,elastic,host_fed,evaluate] [--objects]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from unmicst_amd import model, trainer, trainset  # noqa: E402


def host_batch(planes, ann, wmaps, d, P, K, lw):
    """What a host-fed loop builds per step (the reference's own loop does this in numpy, UnMicst1-5.py:466-481)."""
    n, C = len(d), planes.shape[1]
    data = np.empty((n, P, P, C), np.float32)
    labels = np.empty((n, P, P, K), np.float32)
    weights = np.empty((n, P, P, K), np.float32) if lw.weighted else None
    ks = np.arange(1, K + 1, dtype=np.uint8)
    for b in range(n):
        i, pg, y0, x0, t = (int(d[f][b]) for f in ("index", "page", "y0", "x0", "transform"))

        def tf(a):
            if t & 4:
                a = np.swapaxes(a, -1, -2)
            if t & 2:
                a = a[..., ::-1, :]
            if t & 1:
                a = a[..., ::-1]
            return a
        v = tf(planes[i, :, pg, y0:y0 + P, x0:x0 + P]).astype(np.float64)
        data[b] = np.moveaxis(v * np.float64(d["contrast"][b]) + np.float64(d["brightness"][b]), 0, -1)
        code = tf(ann[i, y0:y0 + P, x0:x0 + P])
        labels[b] = code[..., None] == ks
        if weights is not None:
            w = tf(wmaps[i, y0:y0 + P, x0:x0 + P]).astype(np.float64)[..., None]
            weights[b] = w * np.asarray(lw.intersect_weight[:K], np.float64) + np.asarray(lw.class_weight[:K], np.float64)
    return data, labels, weights


def blob_annotation(S, K, seed):
    """Smoothed noise thresholded into blobs of the last class with a one-pixel ring of the class before it, class 0 elsewhere: what a
    nuclei annotation looks like to the object pass.  numpy only (a 9-tap box filter, five times)."""
    rng = np.random.default_rng(seed)
    f = rng.random((S + 40, S + 40))
    for _ in range(5):                                    # each pass takes 8 pixels off either axis
        c = np.cumsum(np.cumsum(np.pad(f, ((1, 0), (1, 0))), axis=0), axis=1)
        f = c[9:, 9:] - c[:-9, 9:] - c[9:, :-9] + c[:-9, :-9]
    obj = f > np.quantile(f, 0.7)
    grown = obj.copy()
    grown[1:] |= obj[:-1]
    grown[:-1] |= obj[1:]
    grown[:, 1:] |= obj[:, :-1]
    grown[:, :-1] |= obj[:, 1:]
    A = np.ones((S, S), np.uint8)
    if K > 2:
        A[grown & ~obj] = K - 1
    A[obj] = K
    return A


def shapes(names):
    out = []
    for nm in names:
        if nm == "nucleiDAPI":
            out.append((nm, model.KNOWN_HP["nucleiDAPI"], 16, trainer.legacy_options(), trainset.UNWEIGHTED, 0.0, 0.0))
        elif nm == "v2-256":
            out.append((nm, model.KNOWN_HP["synthetic-256"], 8, trainer.duo_options(), trainset.LABEL_WEIGHTS["duo"], 0.17, 0.017))
        else:
            raise SystemExit("unknown shape %s" % nm)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--shapes", default="nucleiDAPI,v2-256")
    ap.add_argument("--samples", type=int, default=32)
    ap.add_argument("--paths", default="step_sampled,augmented,warped,elastic,host_fed,evaluate")
    ap.add_argument("--objects", action="store_true", help="add the object-score leg: evaluate with and without ObjectOptions, alternated")
    a = ap.parse_args()
    paths = a.paths.split(",")
    unknown = set(paths) - {"step_sampled", "augmented", "warped", "elastic", "host_fed", "evaluate"}
    if unknown:
        raise SystemExit("unknown path(s) %s" % sorted(unknown))
    for name, hp, B, opts, lw, mb, mc in shapes(a.shapes.split(",")):
        P, S, pages = hp.imSize, hp.imSize + hp.imSize // 4, 2
        rng = np.random.default_rng(0)
        planes = rng.normal(0, 1, (a.samples, hp.nChannels, pages, S, S)).astype(np.float32)
        ann = rng.integers(0, hp.nClasses + 1, (a.samples, S, S)).astype(np.uint8)
        wmaps = rng.random((a.samples, S, S)).astype(np.float32)
        blob = model.random_blob(hp, seed=1)
        tr = trainer.Trainer(hp, blob, opts, batch=B)
        ts = trainset.TrainSet.from_arrays(tr, planes, ann, list(wmaps), lw)
        ts.set_augment(trainset.AugmentTable.from_sigmas((0.75, 1.5, 3.0), 0.3, 0.2))
        worst = np.zeros(B, trainer.AUGMENT_DESC)
        worst["blur_level"], worst["gain"] = 3, 2.0
        turned = np.zeros(B, trainer.WARP_DESC)
        turned["m"] = trainset.warp_matrix(30.0, 1.25)
        bent = np.zeros(B, trainer.ELASTIC_DESC)
        bent["n"] = 5
        lrng = np.random.default_rng(2)
        for j in range(B):
            bent["d"][j] = trainset.elastic_lattice(lrng.standard_normal(50), 4.0, 5)
        sampler = trainset.Sampler(1, a.samples, B, S, P, pages, mb, mc, transforms=True)
        per_step = B * P * P * (hp.nChannels + (2 if lw.weighted else 1) * hp.nClasses) * 4

        def run_sampled(n):
            t0 = time.perf_counter()
            for _ in range(n):
                tr.step_sampled(ts, sampler.next())
                tr.loss()
            return time.perf_counter() - t0

        def run_augmented(n):
            t0 = time.perf_counter()
            for _ in range(n):
                tr.step_augmented(ts, sampler.next(), worst)
                tr.loss()
            return time.perf_counter() - t0

        def run_warped(n):
            t0 = time.perf_counter()
            for _ in range(n):
                tr.step_warped(ts, sampler.next(), worst, turned)
                tr.loss()
            return time.perf_counter() - t0

        def run_elastic(n):
            t0 = time.perf_counter()
            for _ in range(n):
                tr.step_elastic(ts, sampler.next(), worst, turned, bent)
                tr.loss()
            return time.perf_counter() - t0

        def run_host(n):
            t0 = time.perf_counter()
            for _ in range(n):
                tr.step(*host_batch(planes, ann, wmaps, sampler.next(), P, hp.nClasses, lw))
            return time.perf_counter() - t0

        legs = [(path, fn) for path, fn in (("step_sampled", run_sampled), ("augmented", run_augmented), ("warped", run_warped),
                                            ("elastic", run_elastic), ("host_fed", run_host)) if path in paths]
        for _, fn in legs:
            fn(a.warmup)
        for r in range(a.repeats):
            for path, fn in legs:
                dt = fn(a.steps)
                print(json.dumps({"shape": name, "batch": B, "path": path, "repeat": r, "steps": a.steps, "seconds": round(dt, 5),
                                  "images_per_s": round(a.steps * B / dt, 1), "step_ms": round(1e3 * dt / a.steps, 4),
                                  "host_fed_upload_bytes_per_step": per_step}), flush=True)
        vd = trainset.validation_descriptors(a.samples, S, P)
        if "evaluate" in paths:
            tr.evaluate(ts, vd)
        for r in range(a.repeats if "evaluate" in paths else 0):
            t0 = time.perf_counter()
            ev = tr.evaluate(ts, vd)
            dt = time.perf_counter() - t0
            print(json.dumps({"shape": name, "batch": B, "path": "evaluate", "repeat": r, "images": len(vd), "seconds": round(dt, 5),
                              "images_per_s": round(len(vd) / dt, 1), "labelled": int(ev["counts"][1].sum())}), flush=True)
        if a.objects:
            bann = np.stack([blob_annotation(S, hp.nClasses, 100 + i) for i in range(a.samples)])
            bs = trainset.TrainSet.from_arrays(tr, planes, bann, list(wmaps), lw)
            oopts = trainset.ObjectOptions()
            batches = -(-len(vd) // B)
            for _ in range(max(1, a.warmup // 3)):
                tr.evaluate(bs, vd)
                tr.evaluate(bs, vd, objects=oopts)
            for r in range(a.repeats):
                t0 = time.perf_counter()
                tr.evaluate(bs, vd)
                t1 = time.perf_counter()
                ev = tr.evaluate(bs, vd, objects=oopts)
                t2 = time.perf_counter()
                print(json.dumps({"shape": name, "batch": B, "path": "objects", "repeat": r, "images": len(vd), "batches": batches,
                                  "evaluate_ms_per_batch": round(1e3 * (t1 - t0) / batches, 4),
                                  "evaluate_objects_ms_per_batch": round(1e3 * (t2 - t1) / batches, 4),
                                  "objects": {k: v for k, v in ev["objects"].items() if k != "f1"}}), flush=True)
            bs.close()
        ts.close()
        tr.close()


if __name__ == "__main__":
    main()
