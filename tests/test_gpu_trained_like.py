"""The split-precision forms on trained-like weights and real tiles, on the GPU (reference side: tests/trained_like.py,
tests/trained_cases.json, tests/test_trained_like_cpu.py).

Every other GPU figure for precision f16f6 -- the form UMX_PREC_DEFAULT resolves to wherever a layer can take it -- is on
model.random_blob.  Here the weights are resampled from the three shipped legacy models and calibrated on tiles of 105.tif
(trained_like.trained_like_blob), the tiles are real 105.tif tiles, the all-padding tile, constants, a ramp, noise of sigma 0.1 / 1 / 4
and a smooth field, and the graphs run from one F6 launch (K 1 296) to the duo graph at 256 pixels (four, K up to 7 776).  Per case

    max |p - p64| <= tol                 f32 and f16x3, every tile      (tol = min(E_drop / 4, 2e-5))
    max |p - p64| <= tol_f6, <= 1e-4     f16f6, every tile              (tol_f6 = min(4 x emulated E_f6, 1e-4)), the F6 kernels on
                                         exactly the launches the emulation assumed
    no precision argument                the bytes of f16f6
    the first three tiles alone,         the bits they have inside the full run (f16f6 runs two tiles per workgroup; the second
    tiles 1 ... 3 alone                  run changes a tile's partner in every case)

Every test prints E_gpu of the three precisions and max |p_f16f6 - p_f16x3| of its case.  Measured on MI355X:
f32 7.6e-6 ... 1.3e-5 and f16x3 4.3e-6 ... 8.3e-6 against tol 2e-5; f16f6 3.8e-5 ... 6.4e-5 (0.88 ... 1.13 x its emulation) against
tol_f6 = 1e-4, and 3.8e-5 ... 6.3e-5 from f16x3.  A case over its bound is a finding about a kernel, the planner or the form, never a
reason to move a bound."""
import functools

import numpy as np
import pytest

import inference_ref as R
import trained_like as TL
from unmicst_amd import umx

pytestmark = pytest.mark.gpu

TABLE = TL.load_table()
NORTH_STAR = 1e-4


@pytest.fixture(scope="module", params=list(TL.TRAINED_CASES))
def case(request):
    """(name, hp, blob, tiles, float64 probabilities, max_batch): computed once per case, never written to."""
    name = request.param
    hp, blob, x = TL.case_inputs(name)
    p64 = R.forward64(hp, blob, x)
    p64.setflags(write=False)
    return name, hp, blob, x, p64, TL.TRAINED_CASES[name][3]


def _template_args(kernel):
    return kernel[kernel.index("<") + 1:-1].split(", ")


def _f6_sites(prof):
    """Launch names whose kernel is conv_f16x3<NT, KMT, NPH, DBG, MAXP, PK, D2S, F6, W2> with F6 (the eighth argument) set."""
    return {e["name"] for e in prof if e["kernel"].startswith("conv_f16x3<") and _template_args(e["kernel"])[7] == "true"}


@functools.lru_cache(maxsize=None)
def _run(name, prec):
    """(probabilities, eng.precision, F6 launch names) of a case's tiles through its max_batch; one engine per (case, precision)."""
    hp, blob, x = TL.case_inputs(name)
    with umx.Engine(hp, blob, max_batch=TL.TRAINED_CASES[name][3], precision=prec) as eng:
        got = eng.forward_tiles(x)
        eng.profile_enable(1)
        eng.forward_tiles(x[:1])
        sites = _f6_sites(eng.profile_read())
        eng.profile_enable(False)
        got.setflags(write=False)
        return got, eng.precision, sites


def _tile_errors(got, p64):
    return np.abs(got.astype(np.float64) - p64).reshape(got.shape[0], -1).max(axis=1)


def _summary(name, p64):
    """Prints and returns {precision: per-tile errors}."""
    errs = {prec: _tile_errors(_run(name, prec)[0], p64) for prec in ("f32", "f16x3", "f16f6")}
    d = float(np.abs(_run(name, "f16f6")[0].astype(np.float64) - _run(name, "f16x3")[0]).max())
    t = TABLE[name]
    print("%s: E_gpu f32 %.3g  f16x3 %.3g  (tol %.3g)   f16f6 %.3g  (tol_f6 %.3g, emulated %.3g)   max |f16f6 - f16x3| %.3g" % (
        name, errs["f32"].max(), errs["f16x3"].max(), t["tol"], errs["f16f6"].max(), t["tol_f6"], t["E_f6"], d))
    print("    f16f6 per tile (%s): %s" % (" ".join(TL.TILE_ORDER[:len(p64)]), " ".join("%.2g" % e for e in errs["f16f6"])))
    return errs


@pytest.mark.parametrize("prec", ["f32", "f16x3"])
def test_every_tile_within_tol(case, prec):
    name, hp, blob, x, p64, mb = case
    errs = _summary(name, p64)[prec]
    assert _run(name, prec)[1] == prec
    assert x.shape[0] == TL.TRAINED_CASES[name][2] and (mb % 2 == 1 or x.shape[0] % mb % 2 == 1)   # some batch ends in a half-empty tile pair
    assert np.all(errs <= TABLE[name]["tol"]), (name, prec, errs.tolist(), TABLE[name]["tol"])


def test_f16f6_takes_the_emulated_launches_and_stays_within_its_bounds(case):
    name, hp, blob, x, p64, mb = case
    errs = _summary(name, p64)["f16f6"]
    got, precision, sites = _run(name, "f16f6")
    assert precision == "f16f6"
    # E_f6 was emulated with fp6 cross terms on exactly these launches
    assert sites == R.f6_launches(hp) == TL.F6_LAUNCHES[name], (name, sites)
    assert _run(name, "f16x3")[2] == set()
    assert not np.array_equal(got, _run(name, "f16x3")[0]), "the fp6 form was not used on any layer"
    tol_f6 = TABLE[name]["tol_f6"]
    assert np.all(errs <= tol_f6), "%s: f16f6 is more than 4 x its emulation (or over 1e-4) from float64: per tile %s, tol_f6 %.3g" % (
        name, errs.tolist(), tol_f6)
    assert np.all(errs <= NORTH_STAR), "%s: f16f6 breaks the 1e-4 parity bound: per tile %s" % (name, errs.tolist())


def test_no_precision_argument_gives_the_bytes_of_f16f6(case):
    name, hp, blob, x, p64, mb = case
    _summary(name, p64)
    with umx.Engine(hp, blob, max_batch=mb) as eng:
        assert eng.precision == "f16f6"
        got = eng.forward_tiles(x)
    assert np.array_equal(got.view(np.uint32), _run(name, "f16f6")[0].view(np.uint32))


def test_f16f6_tile_bits_do_not_depend_on_the_batch_partners(case):
    """The first three tiles alone (one batch of three: pairs (0 1)(2 -)) against the same tiles inside the full run -- and tiles
    1 ... 3 alone (pairs (1 2)(3 -); with three tiles in all: (1 2)), which gives tile 1 and tile 2 another partner than the full run
    does in EVERY case: there the batches of 5, 3 and 2 pair them (0 1)(2 3), (0 1)(2 -) and (0 1) | (2 -)."""
    name, hp, blob, x, p64, mb = case
    _summary(name, p64)
    full = _run(name, "f16f6")[0]
    with umx.Engine(hp, blob, max_batch=3, precision="f16f6") as eng:
        alone = eng.forward_tiles(x[:3])
        shifted = eng.forward_tiles(x[1:4])
    assert np.array_equal(alone.view(np.uint32), full[:3].view(np.uint32))
    assert shifted.shape[0] == min(3, x.shape[0] - 1)
    assert np.array_equal(shifted.view(np.uint32), full[1:4].view(np.uint32))
