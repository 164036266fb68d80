#!/usr/bin/env python3
"""Time the label mask (umx_labeler_run) on synthetic H x W stacks of K = 3 uint8 planes (GPU box); one JSON
line.  usage: bench_label.py [H=16384] [W=H] [--reps 3] [--grow R] [--measure C [--measure-dtype u8|u16]] [--split D [--split-core C]]
       [--flood P [--flood-step Q]] [--shape [--no-host]] [--contacts [--reach R] [--no-host]] [--hull [--no-host]]
       [--relabel [--no-host]] [--hmax H]

Two inputs, both made here by pure-numpy recipes (no scipy in the generators, nothing from tests/):
  blobs  nuclei-like discs: the image is cut into 32 x 32 cells; a seeded draw keeps 60 % of them, and each kept cell gets one disc of
         radius 5..11 whose centre lies 12..19 pixels into the cell either way -- discs of neighbouring cells may touch and fuse, as
         nuclei do.  On the discs the last plane is 200 and the others 20 / 30, off them the first plane is 200.
  salt   every pixel an object pixel with probability 0.6 (seeded): the many-small-objects extreme, about one object per 40 pixels.
Per input: the upload, kernel and download milliseconds umx_labeler_last_ms reports (HIP events on the labeler's stream; the best
of --reps runs after one warm-up that also grows the buffers), the object count, and the seconds scipy.ndimage.label + np.bincount
take on the same object mask on this box's CPU share.
--grow R: the blobs input alone, its discs as cores inside bodies whose radii are RIM = 3 pixels larger (the rim is the contour class,
plane 1, and the growth's default domain).  The same planes are labelled without and with the growth; the object count must agree,
and "grow_ms" is the difference of the two kernel times: what the growth adds to a call (its ceil(R / 8) launches and the pass that
writes the labels and the table from the grown plane, less the seed stage's last launch, which it replaces).
--measure C: the blobs input alone, labelled with its label plane kept on the device, then C seeded random planes of --measure-dtype
measured against it (umx_labeler_measure): the upload, kernel and download milliseconds
umx_labeler_measure_last_ms reports, summed over the groups of 4 planes (the best of --reps by kernel time, after one warm-up), the
same for the first plane alone (a group of 1), the bytes one full group moves, and the seconds np.bincount takes for the per-object
sums of the same planes over the same labels on this box's CPU share (one weighted pass per plane: the sum only).
--split D: an input of its own, bodies joined in pairs: the image is cut into cells of 32 x 64; a seeded draw keeps 60 % of them, and each
kept cell gets two squares of 24 x 24 joined by a bridge of 2 D rows -- the widest neck that depth D cuts, so every pair must come back
as two objects.  The same planes are labelled without and with the split; "split_ms" is the
difference of the two kernel times, and the four counts of the split are reported.
--flood P (with --split D): the same bridged pairs, with plane P given a ridge of RIDGE in the third column of every bridge -- off the
bridge's middle, where the split's regrow cuts -- over the plane's 30 elsewhere.  The planes are labelled with the split alone (the
yardstick) and with the flood on plane P in levels of --flood-step; "flood_ms" is the difference
of the two kernel times, and the flood's counts -- its launches among them -- are reported.
--hmax H: an input of its own, overlapping discs: the image is cut into cells of 48 x 48, each with two discs of radius 12 whose centres
are 14 apart -- their common neck is 19 pixels wide, more than 2 * 8, so no --split can cut it -- and plane 1 carries one dome per disc
(30 at the rim to 190 at the centre, 96 on the saddle between the two).  The same planes are labelled plainly, with --split 3 and with
the h-maxima seeds of height H on plane 1, in one process; "hmax_ms" is what the seeds and their
regrow add to the plain call, and the counts -- the launches of the two reconstructions among them -- are reported.
--shape: the blobs input alone, labelled with its label plane kept on the device, then the shapes of its objects (umx_labeler_shape,
DESIGN.md section 8.1 steps 16 to 18): the kernel and download milliseconds umx_labeler_shape_last_ms reports (the best of --reps by
kernel time, after one warm-up), beside them the one-plane uint16 measurement of the same labels (the yardstick: it reads the same
label plane once and 2 bytes a pixel more), the bytes the shape launch moves at most and at least, and the seconds numpy / scipy take
for the same table on this box's CPU share: five weighted np.bincount passes for the moments, band by band, and the window counts
object by object on scipy.ndimage.find_objects' boxes.
--hull: the blobs input alone, labelled with its label plane kept on the device, then the hulls of its objects (umx_labeler_hull,
DESIGN.md section 8.1 steps 25 to 28): the kernel and download milliseconds umx_labeler_hull_last_ms reports (the best of --reps by
kernel time, after one warm-up that also grows the buffers and learns V), beside them the shape call on the same labels in the same
process (the yardstick of DESIGN.md's expectation), E (the rows of all boxes, from the object table) and V, and the seconds numpy / scipy
take for the same hulls on this box's CPU share: scipy.spatial.ConvexHull over the corners of every object's boundary pixels, object by
object on scipy.ndimage.find_objects' boxes, its area held to area2 / 2 and its vertex count to n_vertices.
--relabel: the blobs input alone, labelled with its label plane kept on the device, then relabelled (umx_labeler_relabel, DESIGN.md
section 8.1 steps 29 to 32) with a seeded keep that drops about half the objects: the upload, kernel and download milliseconds
umx_labeler_relabel_last_ms reports (the best of --reps by kernel time; every repetition labels the planes again first, since the call
edits the resident labels), beside them the labelling call of the same process (the yardstick of DESIGN.md's expectation), the seconds
umx.relabel_map takes for the map on the host, and the seconds numpy takes for map[labels] on this box's CPU share, held to the device's
plane.  The host route (relabel_keep, host_relabel) needs no device."""
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
RIM = 3


def blob_mask(H, W, seed=1, rim=0):
    """rim > 0: the same discs with their radii larger by `rim` (the bodies whose cores the plain discs are)"""
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
        disc = (d2 <= ((r[s, :, None, None] + rim) ** 2)) & keep[s, :, None, None]          # [cells y, cells x, 32, 32]
        n = disc.shape[0]
        mask[y0 * CELL:(y0 + n) * CELL] = disc.transpose(0, 2, 1, 3).reshape(n * CELL, nx * CELL)
    return mask[:H, :W]


PAIR_H, PAIR_W, SQUARE = 32, 64, 24


def bridged_mask(H, W, D, seed=4):
    """pairs of squares joined by a bridge of 2 D rows (D <= 8), one pair per kept cell of 32 x 64; no two pairs touch"""
    rng = np.random.default_rng(seed)
    ny, nx = -(-H // PAIR_H), -(-W // PAIR_W)
    keep = rng.random((ny, nx)) < 0.6
    cell = np.zeros((PAIR_H, PAIR_W), bool)
    cell[4:4 + SQUARE, 4:4 + SQUARE] = True
    cell[4:4 + SQUARE, PAIR_W - 4 - SQUARE:PAIR_W - 4] = True
    cell[PAIR_H // 2 - D:PAIR_H // 2 + D, 4 + SQUARE:PAIR_W - 4 - SQUARE] = True
    mask = (keep[:, None, :, None] & cell[None, :, None, :]).reshape(ny * PAIR_H, nx * PAIR_W)
    return mask[:H, :W]


RIDGE, RIDGE_COLUMN = 180, 4 + SQUARE + 2                    # below the nuclei plane's 200; the third column of the bridge


def ridged_planes(H, W, D, P):
    """planes_of the bridged pairs with plane P raised to RIDGE on column RIDGE_COLUMN of every bridge"""
    mask = bridged_mask(H, W, D)
    planes = planes_of(mask)
    x = np.arange(W) % PAIR_W == RIDGE_COLUMN
    y = np.abs(np.arange(H) % PAIR_H - PAIR_H // 2 + 0.5) < D    # the bridge's 2 D rows
    planes[P][mask & y[:, None] & x[None, :]] = RIDGE
    return planes


def flood_bench(a, H, W):
    planes = ridged_planes(H, W, a.split, a.flood)
    with umx.Labeler(a.device) as lb:
        cut, with_split = best_kernel_ms(lb, planes, a.reps, split=a.split, split_core=a.split_core)
        flooded, with_flood = best_kernel_ms(lb, planes, a.reps, split=a.split, split_core=a.split_core, flood=a.flood, flood_step=a.flood_step)
        counts = lb.flood_counts()
    assert len(cut) == len(flooded) == counts["n_objects"] and int(cut["area"].sum()) == int(flooded["area"].sum()) and counts["unreached"] == 0
    assert not np.array_equal(cut["area"], flooded["area"])      # the cut has moved
    return dict({"split": a.split, "split_core": a.split_core, "flood": a.flood, "flood_step": a.flood_step,
                 "object_pixels": int(cut["area"].sum()), "kernel_ms_with_split": round(with_split[1], 3),
                 "kernel_ms_with_flood": round(with_flood[1], 3), "flood_ms": round(with_flood[1] - with_split[1], 3),
                 # what one flood launch moves at most, as a growth launch: the label word and, where it is 0, the K class bytes of
                 # every pixel of a tile and its halo (the relief byte is one of them); one label word written per pixel
                 "bytes_per_launch_upper": int(((1 + 2 * umx.LABEL_GROW_HALO / umx.LABEL_GROW_TILE) ** 2 * (4 + planes.shape[0]) + 4) * H * W)},
                **counts)


DISC_PITCH, DISC_RADIUS, DISC_SHIFT, DISC_H = 48, 12, 14, 40


def disc_planes(H, W):
    """planes_of pairs of overlapping discs, one pair per cell of 48 x 48, with plane 1 one dome per disc on them"""
    oy, ox = np.mgrid[0:DISC_PITCH, 0:DISC_PITCH]
    cy, cx = DISC_PITCH // 2, (DISC_PITCH - DISC_SHIFT) // 2
    d = np.minimum(np.hypot(oy - cy, ox - cx), np.hypot(oy - cy, ox - cx - DISC_SHIFT))
    ny, nx = -(-H // DISC_PITCH), -(-W // DISC_PITCH)
    dome = np.where(d <= DISC_RADIUS, 30 + (160 * (DISC_RADIUS - d) / DISC_RADIUS).astype(np.int64), 0).astype(np.uint8)
    mask = np.tile(d <= DISC_RADIUS, (ny, nx))[:H, :W]
    planes = planes_of(mask)
    planes[1] = np.where(mask, np.tile(dome, (ny, nx))[:H, :W], 30)
    return planes


def hmax_bench(a, H, W):
    planes = disc_planes(H, W)
    tile, halo = umx.LABEL_GROW_TILE, umx.LABEL_GROW_HALO
    with umx.Labeler(a.device) as lb:
        before, plain = best_kernel_ms(lb, planes, a.reps)
        cut, with_split = best_kernel_ms(lb, planes, a.reps, split=3)
        after, with_hmax = best_kernel_ms(lb, planes, a.reps, hmax=a.hmax, hmax_plane=1)
        counts = lb.hmax_counts()
    assert len(cut) == len(before) == counts["n_before"] and len(after) == counts["n_objects"] and counts["unreached"] == 0
    assert int(before["area"].sum()) == int(after["area"].sum())
    return dict({"hmax": a.hmax, "object_pixels": int(before["area"].sum()), "kernel_ms": round(plain[1], 3),
                 "kernel_ms_with_split3": round(with_split[1], 3), "kernel_ms_with_hmax": round(with_hmax[1], 3),
                 "hmax_ms": round(with_hmax[1] - plain[1], 3),
                 # what one reconstruction launch moves at most: the mask and the marker byte of every pixel of a tile and its halo,
                 # one marker byte written per pixel
                 "bytes_per_recon_launch_upper": int(((1 + 2 * halo / tile) ** 2 * 2 + 1) * H * W)}, **counts)


def split_bench(a, H, W):
    planes = planes_of(bridged_mask(H, W, a.split))
    with umx.Labeler(a.device) as lb:
        before, plain = best_kernel_ms(lb, planes, a.reps)
        after, with_split = best_kernel_ms(lb, planes, a.reps, split=a.split, split_core=a.split_core)
        counts = lb.split_counts()
    assert counts["n_before"] == len(before) and counts["n_objects"] == len(after) and int(before["area"].sum()) == int(after["area"].sum()) + counts["unreached"]
    return dict({"split": a.split, "split_core": a.split_core, "object_pixels": int(before["area"].sum()),
                 "kernel_ms": round(plain[1], 3), "kernel_ms_with_split": round(with_split[1], 3),
                 "split_ms": round(with_split[1] - plain[1], 3)}, **counts)


def salt_mask(H, W, seed=2):
    return np.random.default_rng(seed).random((H, W), dtype=np.float32) < 0.6


def planes_of(mask, bodies=None):
    """bodies (a superset of mask): their pixels off the mask are the contour class, plane 1 at 210 over 20 / 25"""
    planes = np.empty((3,) + mask.shape, np.uint8)
    planes[0] = np.where(mask if bodies is None else bodies, 20, 200)
    planes[1] = 30 if bodies is None else np.where(bodies & ~mask, 210, 30)
    planes[2] = np.where(mask, 200, 25)
    return planes


def scipy_seconds(mask):
    from scipy import ndimage
    t = time.perf_counter()
    lab, n = ndimage.label(mask)
    area = np.bincount(lab.ravel(), minlength=n + 1)
    return time.perf_counter() - t, n, int(area[1:].sum())


def best_kernel_ms(lb, planes, reps, **kw):
    """-> (objects, (upload, kernel, download) ms of the run with the least kernel time) after one warm-up that grows the buffers"""
    _, objects = lb.run(planes, want_labels=False, **kw)
    best = None
    for _ in range(reps):
        lb.run(planes, want_labels=False, **kw)
        ms = lb.last_ms()
        if best is None or ms[1] < best[1]:
            best = ms
    return objects, best


def grow_bench(a, H, W):
    core, bodies = blob_mask(H, W), blob_mask(H, W, rim=RIM)
    planes = planes_of(core, bodies)
    tile, halo = umx.LABEL_GROW_TILE, umx.LABEL_GROW_HALO
    launches = -(-a.grow // halo)
    with umx.Labeler(a.device) as lb:
        seeds, plain = best_kernel_ms(lb, planes, a.reps)
        grown, with_growth = best_kernel_ms(lb, planes, a.reps, grow=a.grow)
    assert len(seeds) == len(grown) and (grown["area"] >= seeds["area"]).all()
    # what one growth launch moves at most: the label word and, where it is 0, the K class bytes of every pixel of a tile and its halo;
    # one label word written per pixel
    read = (1 + 2 * halo / tile) ** 2 * (4 + planes.shape[0])
    return {"grow": a.grow, "rim": RIM, "objects": len(seeds), "seed_pixels": int(seeds["area"].sum()), "grown_pixels": int(grown["area"].sum()),
            "kernel_ms": round(plain[1], 3), "kernel_ms_with_growth": round(with_growth[1], 3),
            "grow_ms": round(with_growth[1] - plain[1], 3), "grow_launches": launches,
            "bytes_per_launch_upper": int((read + 4) * H * W)}


def best_measure_ms(lb, px, reps):
    """-> (records, (upload, kernel, download) ms of the measurement with the least kernel time) after one warm-up"""
    rec = lb.measure(px)
    best = None
    for _ in range(reps):
        lb.measure(px)
        ms = lb.measure_last_ms()
        if best is None or ms[1] < best[1]:
            best = ms
    return rec, best


def measure_bench(a, H, W):
    dtype = np.uint8 if a.measure_dtype == "u8" else np.uint16
    C, esz, npix = a.measure, np.dtype(dtype).itemsize, H * W
    group = min(C, umx.LABEL_MEASURE_GROUP)
    rng = np.random.default_rng(3)
    px = np.empty((C, H, W), dtype)
    for c in range(C):
        px[c] = rng.integers(0, np.iinfo(dtype).max + 1, (H, W), dtype=dtype)
    with umx.Labeler(a.device) as lb:
        planes = planes_of(blob_mask(H, W))
        labels, objects = lb.run(planes)
        label_ms = lb.last_ms()
        del planes
        N = len(objects)
        rec, ms = best_measure_ms(lb, px, a.reps)
        _, ms1 = best_measure_ms(lb, px[:1], a.reps)
    assert (rec["count"] == objects["area"][None, :]).all()
    t = time.perf_counter()
    sums = [np.bincount(labels.ravel(), weights=px[c].ravel(), minlength=N + 1)[1:] for c in range(C)]
    cpu_s = time.perf_counter() - t
    assert all(np.array_equal(rec["sum"][c], sums[c].astype(np.uint64)) for c in range(C))   # (exact: every sum is below 2^53)
    groups = -(-C // umx.LABEL_MEASURE_GROUP)
    return {"measure": C, "measure_dtype": a.measure_dtype, "objects": N, "object_pixels": int(objects["area"].sum()),
            "label_kernel_ms": round(label_ms[1], 3), "groups": groups, "upload_ms": round(ms[0], 3), "kernel_ms": round(ms[1], 3),
            "download_ms": round(ms[2], 3), "kernel_ms_per_plane": round(ms[1] / C, 3),
            "one_plane_upload_ms": round(ms1[0], 3), "one_plane_kernel_ms": round(ms1[1], 3),
            # a full group: every label word and every pixel of its planes read once at most, its records written once and added to
            "group_upload_bytes": group * esz * npix, "group_read_bytes_upper": (4 + group * esz) * npix, "group_record_bytes": 32 * group * N,
            "numpy_bincount_s": round(cpu_s, 3)}


def best_shape_ms(lb, reps):
    """-> (records, (kernel, download) ms of the shape call with the least kernel time) after one warm-up"""
    rec = lb.shape()
    best = None
    for _ in range(reps):
        lb.shape()
        ms = lb.shape_last_ms()
        if best is None or ms[0] < best[0]:
            best = ms
    return rec, best


def host_shapes(labels, N, band=1024):
    """the same table by numpy / scipy -> (sum_y, sum_x, sum_yy, sum_xy, sum_xx, q1, q2, qd, q3, q4), int64 [N] each"""
    from scipy import ndimage
    H, W = labels.shape
    mom = np.zeros((5, N + 1))
    xx = np.arange(W, dtype=np.float64)
    for y0 in range(0, H, band):                             # (every sum stays below 2^53: exact in float64)
        lab = labels[y0:y0 + band]
        yy = np.arange(y0, y0 + lab.shape[0], dtype=np.float64)[:, None]
        for k, w in enumerate((yy + 0 * xx, xx + 0 * yy, yy * yy + 0 * xx, yy * xx, xx * xx + 0 * yy)):
            mom[k] += np.bincount(lab.ravel(), weights=w.ravel(), minlength=N + 1)
    q = np.zeros((5, N), np.int64)
    for j, box in enumerate(ndimage.find_objects(labels, max_label=N)):
        if box is None:
            continue
        m = np.pad(labels[box] == j + 1, 1)
        a, b, c, d = m[:-1, :-1], m[:-1, 1:], m[1:, :-1], m[1:, 1:]
        n = a.astype(np.int8) + b + c + d
        two = n == 2
        diag = int((two & (a == d)).sum())
        q[:, j] = (int((n == 1).sum()), int(two.sum()) - diag, diag, int((n == 3).sum()), int((n == 4).sum()))
    return tuple(mom[:, 1:].astype(np.int64)) + tuple(q)


def shape_bench(a, H, W):
    npix = H * W
    px = np.random.default_rng(3).integers(0, 65536, (1, H, W), dtype=np.uint16)
    with umx.Labeler(a.device) as lb:
        planes = planes_of(blob_mask(H, W))
        labels, objects = lb.run(planes)
        label_ms = lb.last_ms()
        del planes
        N = len(objects)
        rec, ms = best_shape_ms(lb, a.reps)
        _, ms1 = best_measure_ms(lb, px, a.reps)
    d = umx.shape_descriptors(rec)
    assert np.array_equal(d["area"], objects["area"]) and np.array_equal(rec["sum_y"], objects["sum_y"])
    cpu_s = None
    if not a.no_host:
        t = time.perf_counter()
        host = host_shapes(labels, N)
        cpu_s = time.perf_counter() - t
        names = ("sum_y", "sum_x", "sum_yy", "sum_xy", "sum_xx", "q1", "q2", "qd", "q3", "q4")
        assert all(np.array_equal(rec[n].astype(np.int64), h) for n, h in zip(names, host))
    return {"shape": True, "objects": N, "object_pixels": int(objects["area"].sum()), "holes": int(d["holes"].sum()),
            "label_kernel_ms": round(label_ms[1], 3), "kernel_ms": round(ms[0], 3), "download_ms": round(ms[1], 3),
            "one_plane_u16_measure_kernel_ms": round(ms1[1], 3), "ratio_to_measure": round(ms[0] / ms1[1], 3),
            # every label word once from memory at least; three times (the rows above and below again) at most; the records written and added to
            "read_bytes_lower": 4 * npix, "read_bytes_upper": 12 * npix, "record_bytes": 64 * N,
            "numpy_scipy_s": None if cpu_s is None else round(cpu_s, 3)}


def host_hulls(labels, N):
    """the same hulls by numpy / scipy -> (area float64 [N], n_vertices int64 [N]): Qhull over the corners of the boundary pixels"""
    from scipy import ndimage
    from scipy.spatial import ConvexHull
    area, count = np.zeros(N), np.zeros(N, np.int64)
    for j, box in enumerate(ndimage.find_objects(labels, max_label=N)):
        if box is None:
            continue
        m = np.pad(labels[box] == j + 1, 1)
        inner = m[1:-1, 1:-1] & m[:-2, 1:-1] & m[2:, 1:-1] & m[1:-1, :-2] & m[1:-1, 2:]
        ys, xs = np.nonzero(m[1:-1, 1:-1] & ~inner)
        pts = np.unique(np.concatenate([np.stack([ys + dy, xs + dx], 1) for dy in (0, 1) for dx in (0, 1)]), axis=0)
        q = ConvexHull(pts)
        area[j], count[j] = q.volume, len(q.vertices)
    return area, count


def hull_bench(a, H, W):
    with umx.Labeler(a.device) as lb:
        planes = planes_of(blob_mask(H, W))
        labels, objects = lb.run(planes)
        label_ms = lb.last_ms()
        del planes
        N = len(objects)
        rec, verts = lb.hull()
        first_ms = lb.hull_last_ms()
        best = None
        for _ in range(a.reps):
            again = lb.hull()
            ms = lb.hull_last_ms()
            if best is None or ms[0] < best[0]:
                best = ms
        assert again[0].tobytes() == rec.tobytes() and again[1].tobytes() == verts.tobytes()
        _, shape_ms = best_shape_ms(lb, a.reps)
    E = int((objects["y1"].astype(np.int64) - objects["y0"] + 1).sum())
    assert int(rec["rows"].sum()) == E and (2 * objects["area"].astype(np.int64) <= rec["area2"]).all()
    cpu_s = None
    if not a.no_host:
        t = time.perf_counter()
        area, count = host_hulls(labels, N)
        cpu_s = time.perf_counter() - t
        assert np.array_equal(count, rec["n_vertices"]) and np.allclose(area, rec["area2"] / 2.0, rtol=1e-9, atol=0.0)
    solidity = objects["area"] / (rec["area2"] / 2.0)
    return {"hull": True, "objects": N, "object_pixels": int(objects["area"].sum()), "E": E, "V": len(verts),
            "most_vertices": int(rec["n_vertices"].max()) if N else 0, "mean_solidity": round(float(solidity.mean()), 4) if N else None,
            "label_kernel_ms": round(label_ms[1], 3), "kernel_ms": round(best[0], 3), "download_ms": round(best[1], 3),
            "first_call_kernel_ms": round(first_ms[0], 3), "shape_kernel_ms": round(shape_ms[0], 3),
            "ratio_to_shape": round(best[0] / shape_ms[0], 3),
            # every label word twice from memory (the two row passes); the row entries cleared, added to and read; the scratch vertices
            # written and read; the records and the list written
            "read_bytes_labels": 8 * H * W, "row_entry_bytes": 8 * E, "scratch_bytes": 16 * (E + N), "record_bytes": 32 * N, "vertex_bytes": 8 * len(verts),
            "numpy_scipy_s": None if cpu_s is None else round(cpu_s, 3)}


def relabel_keep(N, seed=5):
    """uint8 [N]: a seeded draw that keeps about half the objects"""
    return (np.random.default_rng(seed).random(N) < 0.5).astype(np.uint8)


def host_relabel(labels, N, keep):
    """the same relabel on the host -> (labels', map, N', seconds of umx.relabel_map, seconds of numpy's map[labels])"""
    t = time.perf_counter()
    m, n_new = umx.relabel_map(N, keep=keep)
    map_s = time.perf_counter() - t
    t = time.perf_counter()
    out = m[labels]
    return out, m, n_new, map_s, time.perf_counter() - t


def relabel_bench(a, H, W):
    with umx.Labeler(a.device) as lb:
        planes = planes_of(blob_mask(H, W))
        labels, objects = lb.run(planes)
        N = len(objects)
        keep = relabel_keep(N)
        first = lb.relabel(keep=keep)                         # warm-up: allocates the map and the second table
        first_ms = lb.relabel_last_ms()
        best = label_ms = None
        for _ in range(a.reps):
            lb.run(planes)
            run_ms = lb.last_ms()
            again = lb.relabel(keep=keep, want_labels=False)
            ms = lb.relabel_last_ms()
            assert again[1].tobytes() == first[1].tobytes() and again[2].tobytes() == first[2].tobytes()
            if best is None or ms[1] < best[1]:
                best = ms
            if label_ms is None or run_ms[1] < label_ms[1]:
                label_ms = run_ms
        shapes = lb.shape()                                    # the tables afterwards are those of the new labels
        assert len(shapes) == len(first[1]) and np.array_equal(umx.shape_descriptors(shapes)["area"], first[1]["area"])
    del planes
    new_labels, new_objects, m = first
    n_new = len(new_objects)
    assert n_new == int(keep.sum()) and np.array_equal(new_objects["area"], objects["area"][keep != 0])
    map_s = numpy_s = None
    if not a.no_host:
        want, hm, hn, map_s, numpy_s = host_relabel(labels, N, keep)
        assert hn == n_new and np.array_equal(hm, m) and np.array_equal(want, new_labels)
        assert umx.relabel_objects(objects, m).tobytes() == new_objects.tobytes()
    return {"relabel": True, "objects": N, "objects_after": n_new, "object_pixels": int(objects["area"].sum()),
            "object_pixels_after": int(new_objects["area"].sum()),
            "label_kernel_ms": round(label_ms[1], 3), "upload_ms": round(best[0], 3), "kernel_ms": round(best[1], 3),
            "first_call_kernel_ms": round(first_ms[1], 3), "first_call_download_ms": round(first_ms[2], 3),
            "ratio_to_label": round(best[1] / label_ms[1], 3),
            # every label word read once; at most every word written (in place only the words that change are); the map up and read;
            # both tables
            "read_bytes_labels": 4 * H * W, "write_bytes_upper": 4 * H * W, "map_bytes": 4 * (N + 1), "table_bytes": 40 * (N + n_new),
            "host_map_s": None if map_s is None else round(map_s, 4), "numpy_remap_s": None if numpy_s is None else round(numpy_s, 3)}


def host_contacts(labels, reach=0, band=1024):
    """the same list by numpy -> (a, b, edges), int64 [M] each: every horizontal and vertical neighbour pair of two different labels,
    counted by np.unique; a reach first grows the labels level by level over the unlabelled pixels (the least labelled 4-neighbour)"""
    lab = labels.astype(np.int64)
    big = np.iinfo(np.int64).max
    for _ in range(reach):
        c = np.pad(np.where(lab > 0, lab, big), 1, constant_values=big)
        least = np.minimum(np.minimum(c[:-2, 1:-1], c[2:, 1:-1]), np.minimum(c[1:-1, :-2], c[1:-1, 2:]))
        lab = np.where((lab == 0) & (least < big), least, lab)
    keys = []
    for y0 in range(0, lab.shape[0], band):                  # (band by band: the pairs of a whole slide at once are tens of GB)
        rows = lab[y0:y0 + band + 1]                         # the band and the row below it
        for p, q in ((rows[:band, :-1], rows[:band, 1:]), (rows[:-1], rows[1:])):
            keep = (p > 0) & (q > 0) & (p != q)
            p, q = p[keep], q[keep]
            keys.append((np.minimum(p, q) << 32) | np.maximum(p, q))
    key, count = np.unique(np.concatenate(keys), return_counts=True)
    return key >> 32, key & 0xFFFFFFFF, count


def contacts_bench(a, H, W):
    """the grown-blobs input of --grow (every shared rim is a contact): the labelling with the growth once, then the contacts of the
    resident labels; the first call grows the table (its reruns are reported), the timed ones find it large enough"""
    core, bodies = blob_mask(H, W), blob_mask(H, W, rim=RIM)
    planes = planes_of(core, bodies)
    grow = a.grow or RIM
    with umx.Labeler(a.device) as lb:
        labels, objects = lb.run(planes, grow=grow)
        label_ms = lb.last_ms()
        del planes
        N = len(objects)
        rec = lb.contacts(reach=a.reach)
        first_ms, first = lb.contacts_last_ms(), lb.contacts_stats()
        best = None
        for _ in range(a.reps):
            again = lb.contacts(reach=a.reach)
            ms = lb.contacts_last_ms()
            if best is None or ms[0] < best[0]:
                best = ms
        stats = lb.contacts_stats()
        assert again.tobytes() == rec.tobytes()
    degree, shared = umx.contact_degrees(rec, N)
    cpu_s = None
    if not a.no_host:
        t = time.perf_counter()
        ha, hb, hn = host_contacts(labels, a.reach)
        cpu_s = time.perf_counter() - t
        assert np.array_equal(rec["a"], ha) and np.array_equal(rec["b"], hb) and np.array_equal(rec["edges"], hn)
    return {"contacts": True, "grow": grow, "reach": a.reach, "objects": N, "M": len(rec), "largest_degree": int(degree.max()) if N else 0,
            "shared_edges": int(rec["edges"].sum()), "label_kernel_ms": round(label_ms[1], 3),
            "kernel_ms": round(best[0], 3), "download_ms": round(best[1], 3),
            "first_call_kernel_ms": round(first_ms[0], 3), "first_call_reruns": first["reruns"], "stats": stats,
            # every label word once from memory at least, twice (the row below again) at most; the table cleared and, per segment, a key read and a count added to
            "read_bytes_lower": 4 * H * W, "read_bytes_upper": 8 * H * W, "table_bytes": 12 * stats["table_capacity"], "record_bytes": 16 * len(rec),
            "numpy_unique_s": None if cpu_s is None else round(cpu_s, 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("H", type=int, nargs="?", default=16384)
    ap.add_argument("W", type=int, nargs="?", default=None)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--grow", type=int, default=0)
    ap.add_argument("--measure", type=int, default=0, metavar="C")
    ap.add_argument("--split", type=int, default=0, metavar="D")
    ap.add_argument("--split-core", dest="split_core", type=int, default=1, metavar="C")
    ap.add_argument("--flood", type=int, default=None, metavar="P", help="with --split: the relief plane of the level flood")
    ap.add_argument("--flood-step", dest="flood_step", type=int, default=umx.FLOOD_DEFAULT_STEP, metavar="Q")
    ap.add_argument("--measure-dtype", dest="measure_dtype", choices=("u8", "u16"), default="u16")
    ap.add_argument("--shape", action="store_true")
    ap.add_argument("--no-host", dest="no_host", action="store_true", help="with --shape / --contacts / --hull / --relabel: leave the numpy / scipy figure out (a traced run)")
    ap.add_argument("--contacts", action="store_true", help="the contacts of the grown-blobs input (--grow R, default the rim)")
    ap.add_argument("--reach", type=int, default=0, metavar="R", help="with --contacts: the reach")
    ap.add_argument("--hull", action="store_true", help="the hulls of the blobs input")
    ap.add_argument("--relabel", action="store_true", help="a relabel of the blobs input that drops about half its objects")
    ap.add_argument("--hmax", type=int, default=None, metavar="H", help="h-maxima seeds of this height on the overlapping-discs input")
    a = ap.parse_args()
    H, W = a.H, a.W or a.H
    out = {"tool": "bench_label", "H": H, "W": W, "K": 3, "min_area": 1, "reps": a.reps}
    if a.relabel:
        print(json.dumps(dict(out, **relabel_bench(a, H, W))))
        return
    if a.hmax is not None:
        print(json.dumps(dict(out, **hmax_bench(a, H, W))))
        return
    if a.hull:
        print(json.dumps(dict(out, **hull_bench(a, H, W))))
        return
    if a.contacts:
        print(json.dumps(dict(out, **contacts_bench(a, H, W))))
        return
    if a.grow:
        print(json.dumps(dict(out, **grow_bench(a, H, W))))
        return
    if a.flood is not None:
        if not a.split:
            ap.error("--flood needs --split")
        print(json.dumps(dict(out, **flood_bench(a, H, W))))
        return
    if a.split:
        print(json.dumps(dict(out, **split_bench(a, H, W))))
        return
    if a.measure:
        print(json.dumps(dict(out, **measure_bench(a, H, W))))
        return
    if a.shape:
        print(json.dumps(dict(out, **shape_bench(a, H, W))))
        return
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
