"""conv_f16x3 through the C ABI on shapes where a workgroup's set-up and its epilogue can go wrong, every kernel form of the bench graph
included: against the oracle at the usual 1e-4 per tile, and bit for bit against the library as it was before the epilogues' range
tracking moved onto the stored binary16 words and the pooled epilogue's pair maximum became one DPP instruction
(tests/golden/conv_setup_crc.json: CRC-32 of each case's float32 probabilities, recorded from that library on an MI355X in the same
session as the first run of this file).  The range flag itself: a stored activation of +-5.8e4 passes, +-6.2e4 raises UMX_ERR_RANGE,
on the fused-head, the plain and the pooled epilogue.

Tile sizes: the engine takes powers of two only, so the shapes are 64 pixels (four levels: 8 x 8 and 4 x 4-pixel images share an
M-tile group at the bottom) and 128 pixels (five levels, the bench graph's kernels at half its tile).  Batches of 1, 3, 5 and 9 tiles:
images past the batch inside a workgroup, an odd tile count for the two-tile F6 workgroups, grids that are no multiple of 8."""
import json
import os
import zlib

import numpy as np
import pytest

import helpers
from unmicst_amd import model, umx

pytestmark = pytest.mark.gpu
TILE_TOL = 1e-4
CRC_FILE = os.path.join(helpers.GOLDEN, "conv_setup_crc.json")
MODELS = {
    "duo64": model.HParams(model.GRAPH_V2, 64, 2, 3, 36, 4, 3, 0),
    "duo128": model.KNOWN_HP["nucleiDAPILAMIN"],       # duo widths from 36, 128 x 128 x 2
}
BATCHES = (1, 3, 5, 9)
# kernel forms the bench uses (template arguments NT, KMT, NPH, DBG, MAXP, PK, D2S, F6, W2) and a launch of duo128 that must run each
FORMS = {
    "lu0.conv": "conv_f16x3<3, 4, 1, false, 4, true, false, false, false>",     # 3-tile packed kernel + fused head
    "lu1.conv": "conv_f16x3<5, 4, 1, false, 4, true, false, false, false>",     # 5-tile packed kernel
    "ld1.conv": "conv_f16x3<5, 4, 1, false, 4, true, false, false, false>",     # ... with the pooled epilogue
    "lu2.conv": "conv_f16x3<9, 4, 1, false, 4, false, false, false, false>",    # 9-tile kernel
    "lu2.convT": "conv_f16x3<9, 4, 1, false, 4, false, false, false, false>",   # per-phase transposed convolution
    "lu0.convT": "conv_f16x3<9, 4, 1, false, 4, false, true, false, false>",    # depth-to-space form
    "lu3.conv": "conv_f16x3<9, 4, 1, false, 4, false, false, true, true>",      # F6 pair kernel
}


def case_inputs(name):
    hp = MODELS[name]
    seed = 31 + hp.imSize
    blob = model.random_blob(hp, seed=seed)
    x = np.random.default_rng(seed).normal(size=(max(BATCHES), hp.imSize, hp.imSize, hp.nChannels)).astype(np.float32)
    return hp, blob, x


def run_model(name):
    """{batch: probabilities} of one model: the first n of the same nine tiles, one launch group each."""
    hp, blob, x = case_inputs(name)
    with umx.Engine(hp, blob, max_batch=16) as eng:
        return {n: eng.forward_tiles(x[:n]) for n in BATCHES}


def crc_of(a):
    return zlib.crc32(np.ascontiguousarray(a, dtype="<f4").tobytes()) & 0xFFFFFFFF


@pytest.fixture(scope="module")
def results():
    from oracle import oracle
    out = {}
    for name in MODELS:
        hp, blob, x = case_inputs(name)
        out[name] = (run_model(name), oracle.forward(hp, blob, x))   # (the oracle once, on all nine tiles: a tile's result is its own)
    return out


def test_the_shapes_reach_every_kernel_form_of_the_bench():
    hp, blob, _ = case_inputs("duo128")
    lines = umx.infer_plan(hp, True, 0, blob, batches=BATCHES)
    for layer, kernel in FORMS.items():
        line = [l for l in lines if l.startswith("[umx plan] %s " % layer)]
        assert len(line) == 1 and kernel in line[0], (layer, line)
    assert "packed NT 3" in [l for l in lines if "lu0.conv " in l][0]
    with umx.Engine(hp, blob, max_batch=2) as eng:
        assert eng.precision == "f16f6"


@pytest.mark.parametrize("name", list(MODELS))
@pytest.mark.parametrize("n", BATCHES)
def test_forward_tiles_match_the_oracle_and_the_recorded_bytes(results, name, n):
    got, ref = results[name]
    err = float(np.abs(got[n] - ref[:n]).max())
    crc = crc_of(got[n])
    print("%s n=%d: max |p - oracle| %.3g, crc32 %08x" % (name, n, err, crc))
    assert got[n].shape == ref[:n].shape and err <= TILE_TOL, (name, n, err)
    with open(CRC_FILE) as f:
        want = json.load(f)["%s/%d" % (name, n)]
    assert "%08x" % crc == want, "the probabilities differ from the bytes the library gave before the change"


# ---- the range flag on the stored words ---------------------------------------------------------------------------------
# A BatchNorm with gamma = 0 makes its layer's activation leaky(beta) on every pixel, whatever the convolution gave: beta = c for c > 0,
# beta = c / 0.2 for c < 0 (the graph's LeakyReLU; 5 c is exact in binary32 for these c up to the product's rounding, 2^-24 relative).
# The consumers' filter slices over that channel are zeroed, so nothing else in the graph sees the value.
HP_RANGE = helpers.small_hps()["v2_duo_like"]       # 32 x 32 x 2, widths 12 / 24 / 48, three levels


def range_blob(site, c):
    blob = model.random_blob(HP_RANGE, seed=6).copy()
    T = model.tensors_from_blob(HP_RANGE, blob)      # views into blob
    beta = c / 0.2 if c < 0 else c                   # (NaN and infinity as they are)
    if site == "head":            # lu0.conv, fused head: every channel (the head's logits stay finite in binary32)
        T["lu0.bn.gamma"][:] = 0.0
        T["lu0.bn.beta"][:] = beta
    elif site == "store":         # lu1.conv, the plain (hi, lo) epilogue: channel 0, read by lu0's transposed convolution [kh, kw, Cout, Cin]
        T["lu1.bn.gamma"][0] = 0.0
        T["lu1.bn.beta"][0] = beta
        T["lu0.wt"][:, :, :, 0] = 0.0
    else:                         # ld1.conv, the pooled epilogue: channel 0, read by ld2 and, as the skip, by lu2.conv [kh, kw, Cin, Cout]
        T["ld1.bn.gamma"][0] = 0.0
        T["ld1.bn.beta"][0] = beta
        T["ld2.w1"][:, :, 0, :] = 0.0
        T["ld2.wshort"][:, :, 0, :] = 0.0
        T["lu2.w2"][:, :, 0, :] = 0.0
    return blob


@pytest.mark.parametrize("site", ["head", "store", "pool"])
@pytest.mark.parametrize("sign", [1.0, -1.0])
def test_range_flag_follows_the_stored_words(site, sign):
    """|v| = 5.8e4 is inside the range (the flag may rise from 59 984 on: one binary16 ulp of 32 below 6e4, half of it by rounding),
    |v| = 6.2e4 is outside, whatever the sign -- the two signs are tracked by different instructions."""
    x = np.random.default_rng(3).normal(size=(3, 32, 32, 2)).astype(np.float32)
    with umx.Engine(HP_RANGE, range_blob(site, sign * 5.8e4), max_batch=4, precision="f16x3") as eng:
        p = eng.forward_tiles(x)
        assert np.isfinite(p).all()
    with umx.Engine(HP_RANGE, range_blob(site, sign * 6.2e4), max_batch=4, precision="f16x3") as eng:
        with pytest.raises(umx.UmxError) as e:
            eng.forward_tiles(x)
        assert e.value.code == umx.ERR_RANGE


@pytest.mark.parametrize("site", ["head", "store", "pool"])
def test_range_flag_rises_for_nan_and_infinity(site):
    x = np.random.default_rng(3).normal(size=(2, 32, 32, 2)).astype(np.float32)
    for c in (np.nan, np.inf, -np.inf):
        with umx.Engine(HP_RANGE, range_blob(site, c), max_batch=4, precision="f16x3") as eng:
            with pytest.raises(umx.UmxError) as e:
                eng.forward_tiles(x)
            assert e.value.code == umx.ERR_RANGE, (site, c)
