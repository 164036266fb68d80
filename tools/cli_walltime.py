#!/usr/bin/env python3
"""End-to-end wall time of the reference-compatible CLI on a synthetic slide (GPU box): UnMicst.py (legacy tool, the shipped
nucleiDAPI weights) on an N x N uint16 TIFF, with the per-stage breakdown the driver prints under UMX_CLI_TIMING=1
(interpreter start + imports, engine set-up, TIFF read, engine call, page writes, clean-up).
usage: cli_walltime.py [N=16384] [other-tree ...]   -- every further argument is another checkout of the repo (with its own built
libumx.so) whose UnMicst.py is timed on the same file, same box: how a round's change is compared with the round before.
       cli_walltime.py N --label   -- only this tree: twice without and twice with --labelMask (the `label` stage: stacking the
planes, the labelling call, the int32 page and the table).
       cli_walltime.py N --label --grow R   -- and twice with --labelMask --labelGrow R as well.
       cli_walltime.py N --label --split D  -- and twice with --labelMask --labelSplit D as well (the stage line then carries the
split's four counts as "label_split").
       cli_walltime.py N --label --split D --flood P  -- and twice with --labelFlood P beside the split as well (the stage line then
carries the flood's counts as "label_flood").
       cli_walltime.py N --label --measure  -- and twice with --labelMask --labelMeasure as well (the `measure` stage: the three
probability planes and the slide's one page against the labels left on the device, and the Intensities file)."""
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import helpers  # noqa: E402
from unmicst_amd import model, tiffio  # noqa: E402


def one(tree, path, out, env_extra, label, n, script="UnMicst.py", what="legacy nucleiDAPI", extra=()):
    e = dict(os.environ, UMX_CLI_TIMING="1", **env_extra)
    e["UMX_CLI_T0"] = repr(time.time())
    t = time.perf_counter()
    r = subprocess.run([sys.executable, os.path.join(tree, script), path, "--stackOutput", "--outputPath", out] + list(extra), env=e,
                       capture_output=True, text=True)
    dt = time.perf_counter() - t
    assert r.returncode == 0, r.stderr[-2000:]
    stages = [l[len("umx-cli-timing "):] for l in r.stderr.splitlines() if l.startswith("umx-cli-timing ")]
    print("%d x %d uint16, %s, --stackOutput: %-44s %.2f s wall (process start to exit)  %s" % (
        n, n, what, label, dt, stages[-1] if stages else ""), flush=True)
    return dt


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 16384
    rest = sys.argv[2:]
    label_only = "--label" in rest
    grow = None
    if "--grow" in rest:
        grow = str(int(rest[rest.index("--grow") + 1]))
        del rest[rest.index("--grow"):rest.index("--grow") + 2]
    split = None
    if "--split" in rest:
        split = str(int(rest[rest.index("--split") + 1]))
        del rest[rest.index("--split"):rest.index("--split") + 2]
    flood = None
    if "--flood" in rest:
        flood = str(int(rest[rest.index("--flood") + 1]))
        del rest[rest.index("--flood"):rest.index("--flood") + 2]
    measure = "--measure" in rest
    others = [a for a in rest if a not in ("--label", "--measure")]
    hp, blob, mean, std = helpers.load_nuclei_dapi()
    raw = helpers.load_sample_105()[0]
    reps = (-(-n // raw.shape[0]), -(-n // raw.shape[1]))
    img = np.tile(raw, reps)[:n, :n]
    with tempfile.TemporaryDirectory() as d:
        model.save_converted(model.ModelArtefacts(hp, blob, mean, std), os.path.join(d, "models", "nucleiDAPI"))
        os.makedirs(os.path.join(d, "x", "registration"))
        path = os.path.join(d, "x", "registration", "slide.tif")
        tiffio.imsave(path, img)
        env = {"UMX_MODELS_DIR": os.path.join(d, "models")}
        if label_only:
            for rep in range(2):
                one(ROOT, path, os.path.join(d, "out_plain%d" % rep), env, "this tree, run %d" % (rep + 1), n)
                one(ROOT, path, os.path.join(d, "out_label%d" % rep), env, "this tree, --labelMask, run %d" % (rep + 1), n,
                    extra=["--labelMask"])
                if grow:
                    one(ROOT, path, os.path.join(d, "out_grow%d" % rep), env, "this tree, --labelMask --labelGrow %s, run %d" % (grow, rep + 1), n,
                        extra=["--labelMask", "--labelGrow", grow])
                if split:
                    one(ROOT, path, os.path.join(d, "out_split%d" % rep), env, "this tree, --labelMask --labelSplit %s, run %d" % (split, rep + 1), n,
                        extra=["--labelMask", "--labelSplit", split])
                if split and flood:
                    one(ROOT, path, os.path.join(d, "out_flood%d" % rep), env,
                        "this tree, --labelMask --labelSplit %s --labelFlood %s, run %d" % (split, flood, rep + 1), n,
                        extra=["--labelMask", "--labelSplit", split, "--labelFlood", flood])
                if measure:
                    one(ROOT, path, os.path.join(d, "out_measure%d" % rep), env, "this tree, --labelMask --labelMeasure, run %d" % (rep + 1), n,
                        extra=["--labelMask", "--labelMeasure"])
            if measure:
                f = [f for f in os.listdir(os.path.join(d, "out_measure0")) if "_Intensities_" in f][0]
                print("  %-40s %d bytes" % (f, os.path.getsize(os.path.join(d, "out_measure0", f))))
            for f in sorted(os.listdir(os.path.join(d, "out_label0"))):
                if "_Labels_" in f or "_Objects_" in f:
                    print("  %-40s %d bytes" % (f, os.path.getsize(os.path.join(d, "out_label0", f))))
            return
        for rep in range(2):
            one(ROOT, path, os.path.join(d, "out_new%d" % rep), env, "this tree, run %d" % (rep + 1), n)
            for i, tree in enumerate(others):
                one(tree, path, os.path.join(d, "out_o%d_%d" % (i, rep)), env, "%s, run %d" % (os.path.basename(tree.rstrip("/")), rep + 1), n)
        one(ROOT, path, os.path.join(d, "out_host"), dict(env, UMX_NO_RAW_PATH="1"), "this tree, host pre/post (UMX_NO_RAW_PATH=1)", n)
        # the default tool (UnMicst1-5.py, solo hyper-parameters: 116 964 tiles of 64 x 64 on this slide; the reference downloads its
        # weights at image-build time, so seeded weights stand in -- timing only) from the repo's own models/ directory
        solo_env = {"UMX_SYNTHETIC_WEIGHTS": "1"}
        for rep in range(2):
            one(ROOT, path, os.path.join(d, "out_solo%d" % rep), solo_env, "this tree, run %d" % (rep + 1), n, "UnMicst1-5.py",
                "solo hp (seeded weights)")
        # the pages of the two trees must be the same bytes
        a = os.path.join(d, "out_new0")
        for i in range(len(others)):
            b = os.path.join(d, "out_o%d_0" % i)
            for root, _, files in os.walk(a):
                for f in files:
                    pa, pb = os.path.join(root, f), os.path.join(b, os.path.relpath(os.path.join(root, f), a))
                    same = open(pa, "rb").read() == open(pb, "rb").read()
                    print("  %-40s %s" % (os.path.relpath(pa, a), "identical to the other tree's" if same else "DIFFERS"))


if __name__ == "__main__":
    main()
