#!/usr/bin/env python3
"""Trained-like weights for the v2 graph, and the cases that pin the split-precision forms on them -- CPU only.

The only v2 model whose layers take the F6 form (fp6 cross terms) is the duo family, and its trained weights are not shipped; every
other GPU figure for the form is on model.random_blob (N(0, 1 / fan_in) filters, BN variance in [0.5, 1.5]).  This module builds a
v2 blob of any width whose tensors carry the statistics of the three legacy models that ARE shipped with weights
(models/{nucleiDAPI,mousenucleiDAPI,CytoplasmIncell}/umx_model.npz), calibrates it so that it is a working network (not a
saturated one), and states the cases (TRAINED_CASES) and test tiles.  tests/trained_cases.json holds the reference-side numbers
(``python tests/trained_like.py --write``); tests/test_trained_like_cpu.py checks them, tests/test_gpu_trained_like.py is the GPU side.

The weights are RESAMPLED from trained tensors; they are not a trained duo checkpoint.
"""
import functools
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
if os.path.join(ROOT, "tests") not in sys.path:
    sys.path.insert(0, os.path.join(ROOT, "tests"))

import helpers  # noqa: E402
import inference_ref as R  # noqa: E402
from unmicst_amd import model  # noqa: E402

DONORS = ("nucleiDAPI", "mousenucleiDAPI", "CytoplasmIncell")
NORM_DONOR = "nucleiDAPI"            # its mean / std normalise every tile (105.tif is this model's sample image)
TABLE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "trained_cases.json")
ROLES = ("w1", "wshort", "wt", "w2", "lb.w", "lt.w")
# a donor BN channel whose input variance on the sample tiles is below this share of its layer's median is dead (a ReLU output that
# is zero almost everywhere): its stored / seen variance ratio says nothing about a live channel, and it is left out of the pairs
DEAD_SHARE = 1e-3


# ------------------------------------------------------------------------------------------------ the donors
@functools.lru_cache(maxsize=None)
def donor(key):
    """(hp, {name: float64 array}, mean, std) of a shipped legacy model."""
    z = np.load(os.path.join(ROOT, "models", key, "umx_model.npz"))
    hp = model.hparams_from_vector(z["hp"])
    T = {k: np.array(v, dtype=np.float64) for k, v in model.tensors_from_blob(hp, z["blob"]).items()}
    return hp, T, float(z["mean"]), float(z["std"])


@functools.lru_cache(maxsize=None)
def sample_plane():
    """105.tif as the legacy drivers pre-process it: float64 in [0, 0.983]."""
    return helpers.legacy_preprocess(helpers.load_sample_105()[0])


def _crop(S, y, x, C, mean, std):
    p = (sample_plane()[y:y + S, x:x + S] - mean) / std
    return np.repeat(p[:, :, None], C, axis=2)              # the plane duplicated into every channel (UnMicst2.py:679-681 with one plane)


def _cal_positions(S, n):
    """n tile origins in the TOP half of the sample image (rows < 416): the calibration tiles."""
    H, W = sample_plane().shape
    rows = max(1, (H // 2) // S)
    per_row = -(-n // rows)
    xs = np.linspace(0, W - S, per_row).astype(int)
    return [(r * S, int(xs[k])) for r in range(rows) for k in range(per_row)][:n]


def _test_positions(S, n):
    """n tile origins in the BOTTOM half (rows >= 416): the real test tiles, disjoint from every calibration tile."""
    H, W = sample_plane().shape
    y0 = H // 2
    return [(y0 + (k * 37) % (H - y0 - S + 1), (k * 211 + 50) % (W - S + 1)) for k in range(n)]


def cal_tiles(hp, n=4):
    """Calibration tiles of 105.tif for trained_like_blob: float64 NHWC, normalised with NORM_DONOR's mean and std."""
    _, _, mean, std = donor(NORM_DONOR)
    return np.stack([_crop(hp.imSize, y, x, hp.nChannels, mean, std) for y, x in _cal_positions(hp.imSize, n)])


@functools.lru_cache(maxsize=None)
def donor_mismatch(key):
    """Per BN channel of a donor, how its stored moving statistics differ from the moments it actually sees on tiles of 105.tif
    (normalised with the donor's own mean / std, float64 forward): array [channels, 2] of
    (stored mean - seen mean) / seen sigma  and  stored variance / seen variance.  Dead channels (DEAD_SHARE) are left out.
    The comparison can be made for all three donors; 105.tif is nucleiDAPI's own kind of image and foreign to the other two, so
    their pairs are wider -- they are kept, as the duo model would also meet images its statistics were not collected on."""
    hp, T, mean, std = donor(key)
    S = hp.imSize
    x = np.stack([_crop(S, y, xx, hp.nChannels, mean, std) for y, xx in _cal_positions(S, 4) + _test_positions(S, 2)])
    pairs = []

    def hook(p, t, _T):
        m = t.mean(dim=(0, 2, 3)).numpy()
        v = t.var(dim=(0, 2, 3), unbiased=False).numpy()
        live = v > DEAD_SHARE * np.median(v)
        d = (T[p + ".bn.mean"] - m) / np.sqrt(np.where(live, v, 1.0))
        f = T[p + ".bn.var"] / np.where(live, v, 1.0)
        pairs.append(np.stack([d, f], 1)[live])

    R.forward64(hp, {k: torch.from_numpy(v) for k, v in T.items()}, x, bn_hook=hook)
    out = np.concatenate(pairs)
    out.setflags(write=False)
    return out


# ------------------------------------------------------------------------------------------------ the generator
def _depth(i, L, Ld):
    """Donor level at the same relative depth as level i of L."""
    return 0 if L <= 1 or Ld <= 1 else int(round(i / (L - 1) * (Ld - 1)))


def donor_name(name, hp, dhp):
    """The donor tensor (or BN prefix) of the same role and relative depth as `name` of a v2 graph `hp`, in a donor graph `dhp`.
    The legacy graph has BatchNorm in its down blocks only: lb takes the deepest one, lu<i> the one of ld<i>'s depth, lt the first."""
    layer, rest = name.split(".", 1)
    L, Ld = hp.nLayers, dhp.nLayers
    if layer == "lb":
        return "lb.w" if rest == "w" else "ld%d" % (Ld - 1)
    if layer == "lt":
        return "lt.w" if rest == "w" else "ld0"
    j = _depth(int(layer[2:]), L, Ld)
    if rest.startswith("bn"):
        return "ld%d" % j
    return "%s%d.%s" % (layer[:2], j, rest)


def fan_in(name, shape):
    kh, kw, a, b = shape
    return kh * kw * (b if name.endswith(".wt") else a)        # transposed-convolution filters are [kh, kw, Cout, Cin]


def filter_stats(name, w):
    """(excess kurtosis, per-input-channel RMS max / median, per-output-channel RMS max / median, rms * sqrt(fan_in)) of a filter."""
    w = np.asarray(w, np.float64)
    z = (w - w.mean()) / w.std()
    rms = np.sqrt((w * w).mean())
    ci = np.sqrt((w * w).mean(axis=(0, 1, 3)))
    co = np.sqrt((w * w).mean(axis=(0, 1, 2)))
    return float((z ** 4).mean() - 3.0), float(ci.max() / np.median(ci)), float(co.max() / np.median(co)), float(rms * np.sqrt(fan_in(name, w.shape)))


def _resampled_filter(rng, name, shape, dname, dw):
    rms = np.sqrt((dw * dw).mean())
    prof_in = np.sqrt((dw * dw).mean(axis=(0, 1, 3))) / rms
    prof_out = np.sqrt((dw * dw).mean(axis=(0, 1, 2))) / rms
    # standardised with the two channel profiles divided out first: they are multiplied back in below, and values that still
    # carried them would count the channel structure twice (measured: excess kurtosis up to 4 x the donor's)
    z = dw / (prof_in[None, None, :, None] * prof_out[None, None, None, :])
    z = ((z - z.mean()) / z.std()).ravel()
    w = rng.choice(z, size=shape)
    w = w * rng.choice(prof_in, size=shape[2])[None, None, :, None] * rng.choice(prof_out, size=shape[3])[None, None, None, :]
    target = rms * np.sqrt(fan_in(dname, dw.shape))            # the donor's rms * sqrt(fan_in), carried over
    return w * (target / (np.sqrt((w * w).mean()) * np.sqrt(fan_in(name, shape))))


def trained_like_blob(hp, seed, cal, report=None):
    """A v2 blob of hyper-parameters `hp` with the value statistics of the shipped legacy models; deterministic in (hp, seed, cal).

    Filters: per tensor a donor model is drawn, and in it the tensor of the same role (w1, wshort, wt, w2, lb.w, lt.w) and relative
    depth; the values are resampled with replacement from the donor's standardised values, multiplied by per-input-channel and
    per-output-channel RMS factors resampled from the donor's channel profiles, and scaled so that rms * sqrt(fan_in) is the donor's.
    BatchNorm: (gamma, beta) drawn jointly per channel from the donor's BN channels at that depth; moving mean and variance set by
    ONE float64 forward in graph order over `cal` (float64 NHWC tiles, see cal_tiles) -- each BN takes the per-channel moments of its
    own input with every BN above it already set -- times a per-channel mismatch (offset of the mean in sigma, factor on the
    variance) resampled from donor_mismatch of the same donor: what the donors' own stored statistics show against what they see.
    report (a dict) receives {tensor name: donor model}."""
    if hp.graph != model.GRAPH_V2 or hp.nExtraConvs:
        raise ValueError("trained_like_blob builds v2 graphs without extra convolutions")
    rng = np.random.default_rng(seed)
    T, bn_donor = {}, {}
    for name, shape in model.tensor_specs(hp):
        if ".bn." in name:
            prefix = name[:name.index(".bn.")]
            if name.endswith(".bn.gamma"):
                key = DONORS[rng.integers(len(DONORS))]
                dhp, dT, _, _ = donor(key)
                dp = donor_name(name, hp, dhp)
                idx = rng.integers(dT[dp + ".bn.gamma"].size, size=shape)
                T[name] = dT[dp + ".bn.gamma"][idx]
                T[prefix + ".bn.beta"] = dT[dp + ".bn.beta"][idx]
                mm = donor_mismatch(key)
                bn_donor[prefix] = mm[rng.integers(len(mm), size=shape)]
                if report is not None:
                    report[prefix + ".bn"] = key
            elif name.endswith(".bn.mean"):
                T[name] = np.zeros(shape)
            elif name.endswith(".bn.var"):
                T[name] = np.ones(shape)
            continue
        key = DONORS[rng.integers(len(DONORS))]
        dhp, dT, _, _ = donor(key)
        dname = donor_name(name, hp, dhp)
        T[name] = _resampled_filter(rng, name, shape, dname, dT[dname])
        if report is not None:
            report[name] = key

    Tt = {k: torch.from_numpy(np.ascontiguousarray(v, np.float64)) for k, v in T.items()}

    def hook(p, t, TT):
        m = t.mean(dim=(0, 2, 3))
        v = t.var(dim=(0, 2, 3), unbiased=False)
        mis = torch.from_numpy(bn_donor[p])
        TT[p + ".bn.mean"] = m + mis[:, 0] * torch.sqrt(v)
        TT[p + ".bn.var"] = v * mis[:, 1]

    R.forward64(hp, Tt, cal, bn_hook=hook)
    return model.blob_from_tensors(hp, {k: v.numpy() for k, v in Tt.items()})


# ------------------------------------------------------------------------------------------------ the test tiles
# the order the cases take their tiles in: every case has a real tile, the padding tile and noise of sigma 1 (the first three); the
# 12-tile sets hold every family.  The padding of the tile grid is zeros before normalisation, so "padding" and "const0" are the
# same values (-mean / std): both stay, as two slots of a batch.  Noise of sigma 4 (inputs to 16 sigma) is in the 12-tile sets only:
# on that tile the two CPU restatements of the correct arithmetic already stand 2 - 9e-6 from float64 (eight seeds of each graph), and
# on the three deeper graphs no seed tried leaves a bound <= 2e-5 that is 8 x above them.
TILE_ORDER = ("real0", "padding", "noise1", "real1", "blobs", "noise4", "ramp", "const0.983", "noise0.1", "const0", "real2", "real3")


def tiles_for(hp, seed, n):
    """The first n tiles of TILE_ORDER for a graph: float32 NHWC, each family normalised with NORM_DONOR's mean and std (the noise
    families are drawn in normalised units, independently per channel)."""
    _, _, mean, std = donor(NORM_DONOR)
    S, C = hp.imSize, hp.nChannels
    pos = _test_positions(S, 4)
    yy, xx = np.mgrid[0:S, 0:S]

    def plane(v):
        return np.repeat(((np.asarray(v, np.float64) - mean) / std)[:, :, None], C, axis=2)

    out = []
    for fam in TILE_ORDER[:n]:
        rng = np.random.default_rng([seed, 1000 + TILE_ORDER.index(fam)])      # a family's draw does not depend on the others
        if fam.startswith("real"):
            t = _crop(S, *pos[int(fam[4:])], C, mean, std)
        elif fam == "padding":
            t = plane(np.zeros((S, S)))
        elif fam.startswith("const"):
            t = plane(np.full((S, S), float(fam[5:])))
        elif fam == "ramp":
            t = plane(0.983 * (yy + xx) / (2.0 * (S - 1)))
        elif fam.startswith("noise"):
            t = rng.normal(0.0, float(fam[5:]), size=(S, S, C))
        elif fam == "blobs":                                   # a smooth field: white noise low-passed to a scale of S / 16 pixels
            f = np.fft.fftfreq(S)
            g = np.exp(-0.5 * ((f[:, None] ** 2 + f[None, :] ** 2) * (2 * np.pi * S / 16.0) ** 2))
            b = np.fft.ifft2(np.fft.fft2(rng.normal(size=(S, S))) * g).real
            t = plane(0.983 * (b - b.min()) / (b.max() - b.min()))
        else:
            raise KeyError(fam)
        out.append(t)
    return np.stack(out).astype(np.float32)


# ------------------------------------------------------------------------------------------------ the cases
# name -> (hp, seed, tiles, max_batch on the GPU).  The odd batches leave a half-empty two-tile workgroup of the F6 form.
# Seeds: the first from 11 upward for which the case stands on the reference side (case_conditions: tol >= 8 x E_ref and the
# saturation cap).  No GPU figure and no E_f6 entered the choice.  On the 12-tile sets it is the sigma-4 tile that rejects seeds
# (tl_72_lb: E_ref 4.3 / 3.3 / 3.4 / 2.9 / 3.4 / 3.0e-6 for seeds 11 - 16, 9.5e-7 for 17; tl_144_lb: 4.7e-6 for 11, 1.6e-6 for 12);
# on the duo graphs it is E_drop, which a fault on ld4 / lb sets there (the skips dilute the deep path): seeds 11 and 12 give
# tol = E_drop / 4 = 6.7e-6 / 3.6e-6 (128 pixels) and 7.7e-6 / 5.0e-6 (256) against 8 x E_ref = 7.5e-6 / 6.1e-6 and 1.0e-5 / 8.8e-6.
TRAINED_CASES = {
    "tl_72_lb": (R.HP_F6, 17, 12, 5),
    "tl_144_lb": (model.HParams(model.GRAPH_V2, 64, 2, 3, 144, 2, 3, 0), 12, 12, 5),
    "tl_72_l3": (model.HParams(model.GRAPH_V2, 128, 2, 3, 72, 3, 3, 0), 11, 5, 3),
    "tl_duo128": (model.KNOWN_HP["nucleiDAPILAMIN"], 13, 5, 3),
    "tl_duo256": (model.KNOWN_HP["synthetic-256"], 13, 3, 2),
}
# the launches that must take the F6 form (held to inference_ref.f6_launches on the CPU and to the profile's kernel names on the GPU)
F6_LAUNCHES = {
    "tl_72_lb": {"lb.conv"},
    "tl_144_lb": {"lb.conv"},
    "tl_72_l3": {"ld2.conv", "lb.conv", "lu2.conv"},
    "tl_duo128": {"ld3.conv", "lu3.conv"},
    "tl_duo256": {"ld3.conv", "ld4.conv", "lu4.conv", "lu3.conv"},
}
# the cases whose every figure -- all tiles, the full fault sweep (two faults x every layer) -- the CPU test recomputes; for the two duo
# graphs (the sweep takes 4 - 8 minutes there) it recomputes E_ref and E_f6 on the first tile and the saturated share of all tiles
SWEPT_IN_TEST = ("tl_72_lb", "tl_144_lb", "tl_72_l3")
# cap on the share of pixels whose largest class probability exceeds 0.999, over a case's test tiles (measured on the cases:
# 0.008 ... 0.062; rejected seeds reach 0.18, an uncalibrated blob 1)
SATURATION_CAP = 0.15


@functools.lru_cache(maxsize=None)
def case_inputs(name, seed=None):
    """(hp, blob, tiles) of a case -- or of its graph and tile count under another seed; computed once per process, not to be
    written to."""
    hp, case_seed, n, _ = TRAINED_CASES[name]
    seed = case_seed if seed is None else seed
    blob = trained_like_blob(hp, seed, cal_tiles(hp))
    x = tiles_for(hp, seed, n)
    x.setflags(write=False)
    return hp, blob, x


def saturated_share(p):
    return float((p.max(axis=-1) > 0.999).mean())


def case_numbers(name, tiles=None, sweep=True, per_layer=None, seed=None, per_tile=None):
    """E_ref, E_f6 and (sweep) E_drop, tol, tol_f6, the recorded condition E_drop >= 2 x tol_f6 -- on the first `tiles` tiles (None: all).
    seed: another seed than the case's; per_tile (a dict) receives the per-tile E_ref and E_f6."""
    from oracle import oracle
    hp, blob, x = case_inputs(name, seed)
    x = x if tiles is None else x[:tiles]
    p64 = R.forward64(hp, blob, x)

    def tile_errs(p):
        return np.abs(p.astype(np.float64) - p64).reshape(len(x), -1).max(axis=1)

    def err(p):
        return float(tile_errs(p).max())

    ref = np.maximum(tile_errs(oracle.forward(hp, blob, x)), tile_errs(R.emulate(hp, blob, x, lambda n: "f16x3")))
    f6 = tile_errs(R.emulate(hp, blob, x, R.f6_plan_of(hp)))
    out = {"E_ref": float(ref.max()), "E_f6": float(f6.max())}
    if per_tile is not None:
        per_tile.update(E_ref=ref, E_f6=f6, saturated=saturated_share(p64))
    if sweep:
        e_drop = np.inf
        for fault in R.FAULT_PLANS:
            for layer in R.layer_names(hp):
                e = err(R.emulate(hp, blob, x, lambda n: fault if n == layer else "f16x3"))
                e_drop = min(e_drop, e)
                if per_layer is not None:
                    per_layer.setdefault(fault, {})[layer] = e
        out["E_drop"] = e_drop
        out.update(tolerances(out))
        out["saturated"] = saturated_share(p64)
        out["E_ref_tile0"], out["E_f6_tile0"] = float(ref[0]), float(f6[0])     # what the CPU test repeats for the slow cases
    return out


def tolerances(c):
    tol, tol_f6 = min(c["E_drop"] / 4, 2e-5), min(4 * c["E_f6"], 1e-4)
    return {"tol": tol, "tol_f6": tol_f6, "drop_is_twice_tol_f6": bool(c["E_drop"] >= 2 * tol_f6)}


def case_conditions(c):
    """The conditions a case must meet, on the reference side's numbers alone -> the violated ones (empty: the case stands).
    E_drop >= 2 x tol_f6 (a condition of the random-weight gate) is recorded, not required: on these weights the fp6 cross terms come
    within a small factor of a dropped product."""
    bad = []
    t = tolerances(c)
    if not (c["tol"] == t["tol"] and c["tol_f6"] == t["tol_f6"]):
        bad.append("tol / tol_f6 are not min(E_drop / 4, 2e-5) / min(4 x E_f6, 1e-4)")
    if not c["tol"] >= 8 * c["E_ref"]:
        bad.append("tol %.3g < 8 x E_ref %.3g: the correct arithmetic is not 8 x under the bound" % (c["tol"], c["E_ref"]))
    if not c["saturated"] <= SATURATION_CAP:
        bad.append("saturated share %.3g > %.3g" % (c["saturated"], SATURATION_CAP))
    return bad


def load_table():
    with open(TABLE) as f:
        return json.load(f)


def gpu_rows(name, seed=None):
    """Prints, per tile, what the engine gives on a case's graph and tiles (under the case's seed or another one) in the three
    precisions against forward64, next to the emulated E_f6 -- needs an MI355X.  The figures DESIGN.md section 6 quotes for the seeds
    the reference side rejected come from here: ``python tests/trained_like.py tl_72_lb --seed=11 --gpu``."""
    from unmicst_amd import umx
    hp, blob, x = case_inputs(name, seed)
    p64 = R.forward64(hp, blob, x)
    per_tile = {}
    c = case_numbers(name, sweep=False, seed=seed, per_tile=per_tile)
    rows, outs = [("E_ref (CPU)", per_tile["E_ref"]), ("emulated f6", per_tile["E_f6"])], {}
    for prec in ("f32", "f16x3", "f16f6"):
        with umx.Engine(hp, blob, max_batch=TRAINED_CASES[name][3], precision=prec) as eng:
            outs[prec] = eng.forward_tiles(x)
        rows.append(("E_gpu " + prec, np.abs(outs[prec].astype(np.float64) - p64).reshape(len(x), -1).max(axis=1)))
    print("%s seed %s: E_ref %.3g (a case stands at <= 2.5e-6), saturated %.3g;  tiles: %s" % (
        name, TRAINED_CASES[name][1] if seed is None else seed, c["E_ref"], per_tile["saturated"], " ".join(TILE_ORDER[:len(x)])))
    for label, e in rows:
        print("    %-12s max %.3g   per tile %s" % (label, e.max(), " ".join("%.2g" % v for v in e)))
    print("    max |f16f6 - f16x3| %.3g" % np.abs(outs["f16f6"].astype(np.float64) - outs["f16x3"]).max(), flush=True)


def main(argv):
    """[case ...] [--seed=N] [--gpu] [--write | --update].  Without --gpu: the reference-side numbers of the cases (of their graphs
    under seed N, if given: how a seed is judged); --write / --update store them in tests/trained_cases.json (the cases' own seeds
    only).  With --gpu: gpu_rows of each named case."""
    torch.set_num_threads(max(1, min(16, (os.cpu_count() or 2) - 1)))
    names = [a for a in argv if not a.startswith("--")] or list(TRAINED_CASES)
    seed = ([int(a[7:]) for a in argv if a.startswith("--seed=")] or [None])[0]
    if seed is not None and ("--write" in argv or "--update" in argv):
        raise SystemExit("the table holds the cases' own seeds")
    if "--gpu" in argv:
        for name in names:
            gpu_rows(name, seed)
        return
    table = {}
    for name in names:
        per_layer = {}
        c = case_numbers(name, per_layer=per_layer, seed=seed)
        table[name] = c
        print("%-10s E_ref %.3g  E_drop %.3g  E_f6 %.3g  tol %.3g  tol_f6 %.3g  saturated %.3g  %s" % (
            name, c["E_ref"], c["E_drop"], c["E_f6"], c["tol"], c["tol_f6"], c["saturated"], "; ".join(case_conditions(c)) or "ok"), flush=True)
        for fault, row in per_layer.items():
            print("    %-10s" % fault + " ".join("%s %.2g" % kv for kv in row.items()), flush=True)
    if "--update" in argv and os.path.exists(TABLE):                 # the named cases replace their rows, the others stay
        table = dict(load_table(), **table)
    if "--write" in argv or "--update" in argv:
        if sorted(table) != sorted(TRAINED_CASES):
            raise SystemExit("--write takes every case")
        with open(TABLE, "w") as f:
            json.dump({k: table[k] for k in TRAINED_CASES}, f, indent=1, sort_keys=True)
            f.write("\n")
        print("wrote", TABLE)


if __name__ == "__main__":
    main(sys.argv[1:])
