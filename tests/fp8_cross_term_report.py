#!/usr/bin/env python3
"""Accuracy gate of the FP8 / block-scaled cross-term plan, on the CPU -- no GPU needed.

The split-precision engine evaluates every fp32 product as  x_hi*w_hi + x_hi*w_lo + x_lo*w_hi  on the binary16 matrix pipe
(3 units of matrix work).  The plan priced here keeps x_hi*w_hi in binary16 and moves the two CROSS terms to
v_mfma_scale_f32_16x16x128_f8f6f4 (OCP e4m3 elements, one power-of-two e8m0 scale per 32 consecutive K elements of each operand,
twice the binary16 rate): 1 + 2 * 0.5 = 2 units instead of 3.  This script emulates that arithmetic layer by layer -- activations
re-split into (hi, lo) binary16 pairs after every layer exactly as the engine stores them, weights pre-scaled by the planner's power of
two -- and prints max |p - p_oracle| over the softmax outputs for: the exact 3-product plan (calibration: must reproduce the engine's
~1e-7 .. 3e-6), the 2-product plan of round 2 (calibration: profiles/r02/two_product_probe_report.log measured 5e-5 .. 2.2e-4 on the
random graphs and 6.6e-3 on the shipped nucleiDAPI weights ON THE GPU), and the FP8 cross-term plan on all layers / on layer subsets.

Lives in tests/ because it checks against the oracle (oracle/ is test infrastructure).  Usage: python tests/fp8_cross_term_report.py
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import helpers  # noqa: E402
from oracle import oracle, pi2d_oracle  # noqa: E402
from unmicst_amd import model  # noqa: E402

# the arithmetic emulation lives in tests/inference_ref.py (the inference arithmetic gate derives its tolerances from it)
from inference_ref import forward  # noqa: E402


def run_case(name, hp, blob, x, plans):
    T = {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in model.tensors_from_blob(hp, blob).items()}
    xt = torch.from_numpy(x)
    ref = oracle.forward(hp, blob, x)
    row = []
    for label, plan_of in plans:
        with torch.no_grad():
            p = forward(hp, T, xt, plan_of).numpy()
        row.append(float(np.abs(p - ref).max()))
    print("%-42s" % name + "".join(" %10.3g" % e for e in row), flush=True)
    return row


def main():
    torch.set_num_threads(max(1, (os.cpu_count() or 2) - 1))
    deep = {"ld2", "ld3", "ld4", "lb", "lu4", "lu3", "lu2"}
    plans = [
        ("exact", lambda n: "exact"),
        ("f16x3", lambda n: "f16x3"),
        ("f16x2 all", lambda n: "f16x2"),
        ("fp8x all", lambda n: "fp8x"),
        ("fp8x deep", lambda n: "fp8x" if n in deep else "f16x3"),
        ("fp8x lb only", lambda n: "fp8x" if n == "lb" else "f16x3"),
        ("fp8x top (lu0,lu1)", lambda n: "fp8x" if n in ("lu0", "lu1") else "f16x3"),
        ("fp6x all", lambda n: "fp6x"),
        ("fp6x deep", lambda n: "fp6x" if n in deep else "f16x3"),
    ]
    print("max |p - p_oracle| over the softmax outputs; plans: " + " | ".join(l for l, _ in plans))
    print("%-42s" % "case" + "".join(" %10s" % l.replace(" ", "-")[:10] for l, _ in plans))
    cases = dict(helpers.small_hps())
    cases["duo hp (128x128x2, widths 36..1152)"] = model.KNOWN_HP["nucleiDAPILAMIN"]
    worst = [0.0] * len(plans)
    for name, hp in cases.items():
        blob = model.random_blob(hp, seed=11)
        n = 1 if hp.imSize >= 128 else 3
        x = np.random.default_rng(5).normal(size=(n, hp.imSize, hp.imSize, hp.nChannels)).astype(np.float32)
        row = run_case(name, hp, blob, x, plans)
        worst = [max(a, b) for a, b in zip(worst, row)]
    print("%-42s" % "worst of the nine random graphs" + "".join(" %10.3g" % e for e in worst))
    # the three models the reference ships weights for, on real tiles of its sample image
    raw = helpers.load_sample_105()[0]
    I = helpers.legacy_preprocess(raw)
    for key in ("nucleiDAPI", "mousenucleiDAPI", "CytoplasmIncell"):
        art = model.load_model_dir(os.path.join(ROOT, "models", key))
        hp = art.hp
        pi = pi2d_oracle.PI2DOracle(I, hp.imSize, hp.margin, "accumulate")
        nt = 4 if hp.imSize <= 128 else 2
        x = pi2d_oracle.normalised_batch(pi, 5, nt, hp.nChannels, art.mean, art.std, False)
        run_case("%s real weights, 105.tif tiles" % key, hp, art.blob, x, plans)


if __name__ == "__main__":
    main()
