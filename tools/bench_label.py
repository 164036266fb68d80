#!/usr/bin/env python3
"""Time the label mask (umx_labeler_run) on synthetic H x W stacks of K = 3 uint8 planes (GPU box); one JSON
line.  usage: bench_label.py [H=16384] [W=H] [--reps 3]

Two inputs, both made here by pure-numpy recipes (no scipy in the generators, nothing from tests/):
  blobs  nuclei-like discs: the image is cut into 32 x 32 cells; a seeded draw keeps 60 % of them, and each kept cell gets one disc of
         radius 5..11 whose centre lies 12..19 pixels into the cell either way -- discs of neighbouring cells may touch and fuse, as
         nuclei do.  On the discs the last plane is 200 and the others 20 / 30, off them the first plane is 200.
  salt   every pixel an object pixel with probability 0.6 (seeded): the many-small-objects extreme, about one object per 40 pixels.
Per input: the upload, kernel and download milliseconds umx_labeler_last_ms reports (HIP events on the labeler's stream; the best
of --reps runs after one warm-up that also grows the buffers), the object count, and the seconds scipy.ndimage.label + np.bincount
take on the same object mask on this box's CPU share."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from unmicst_amd import umx  # noqa: E402

CELL = 32


def blob_mask(H, W, seed=1):
    rng = np.random.default_rng(seed)
    ny, nx = -(-H // CELL), -(-W // CELL)
    keep = rng.random((ny, nx)) < 0.6
    r = rng.integers(5, 12, (ny, nx))
    cy = rng.integers(12, 20, (ny, nx))
    cx = rng.integers(12, 20, (ny, nx))
    mask = np.zeros((ny * CELL, nx * CELL), bool)
    oy, ox = np.mgrid[0:CELL, 0:CELL]
    band = 32                                                # cell rows per step: bounds the temporaries
    for y0 in range(0, ny, band):
        s = slice(y0, min(ny, y0 + band))
        d2 = (oy[None, None] - cy[s, :, None, None]) ** 2 + (ox[None, None] - cx[s, :, None, None]) ** 2
        disc = (d2 <= (r[s, :, None, None] ** 2)) & keep[s, :, None, None]          # [cells y, cells x, 32, 32]
        n = disc.shape[0]
        mask[y0 * CELL:(y0 + n) * CELL] = disc.transpose(0, 2, 1, 3).reshape(n * CELL, nx * CELL)
    return mask[:H, :W]


def salt_mask(H, W, seed=2):
    return np.random.default_rng(seed).random((H, W), dtype=np.float32) < 0.6


def planes_of(mask):
    planes = np.empty((3,) + mask.shape, np.uint8)
    planes[0] = np.where(mask, 20, 200)
    planes[1] = 30
    planes[2] = np.where(mask, 200, 25)
    return planes


def scipy_seconds(mask):
    from scipy import ndimage
    t = time.perf_counter()
    lab, n = ndimage.label(mask)
    area = np.bincount(lab.ravel(), minlength=n + 1)
    return time.perf_counter() - t, n, int(area[1:].sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("H", type=int, nargs="?", default=16384)
    ap.add_argument("W", type=int, nargs="?", default=None)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args()
    H, W = a.H, a.W or a.H
    out = {"tool": "bench_label", "H": H, "W": W, "K": 3, "min_area": 1, "reps": a.reps}
    with umx.Labeler(a.device) as lb:
        for name, mask in (("blobs", blob_mask(H, W)), ("salt", salt_mask(H, W))):
            planes = planes_of(mask)
            labels, objects = lb.run(planes)                 # warm-up: grows the buffers
            best = None
            for _ in range(a.reps):
                t = time.perf_counter()
                labels, objects = lb.run(planes)
                wall = (time.perf_counter() - t) * 1e3
                ms = lb.last_ms()
                if best is None or ms[1] < best[1]:
                    best = ms + (wall,)
            cpu_s, n, pixels = scipy_seconds(mask)
            assert n == len(objects) and pixels == int(objects["area"].sum()) == int((labels > 0).sum())
            out[name] = {"objects": len(objects), "object_pixels": pixels, "upload_ms": round(best[0], 3), "kernel_ms": round(best[1], 3),
                         "download_ms": round(best[2], 3), "call_wall_ms": round(best[3], 3), "scipy_label_bincount_s": round(cpu_s, 3)}
            del planes, labels, objects
    print(json.dumps(out))


if __name__ == "__main__":
    main()
