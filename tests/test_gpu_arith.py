"""The inference arithmetic gate on the GPU: every precision of the engine against a float64 forward, at a bound that a lost
split-precision product on ONE layer -- or in one launch, one output phase of a transposed convolution or one N-block of a layer --
cannot meet.

The 1e-4 gates of test_gpu_parity / _switches / _f6 / _shipped_models stay; this is a second, tighter one.  For each case of
inference_ref.ARITH_CASES (graphs of <= 64 pixels with seeded weights and tiles) tests/arith_cases.json holds, from the CPU side alone
(tests/test_inference_arith_cpu.py): tol = min(E_drop, E_cell) / 4, the smallest error the emulated arithmetic shows when x_lo * w_hi or
x_hi * w_lo is omitted on a single layer (E_drop) or in a single cell of one launch (E_cell: inference_ref.cells; the two F6 cases
leave the phases of their transposed convolutions to v2_72_phase, the same widths without an F6 launch), and tol >= 8 x the error of
the correct arithmetic; tol_f6 = 4 x the emulated error of the
F6 form (fp6 cross terms).  Here five tiles run through max_batch = 3 (a ragged last batch; for the eight-wave two-tile workgroups
of the F6 form a half-empty one), and every tile is held to

    max |p_gpu - p64| <= tol      for f32 and f16x3
    max |p_gpu - p64| <= tol_f6   for f16f6 (only where a launch takes the form; it must differ from f16x3 there, and the launches
                                  that take it must be the ones tol_f6 was derived for)

A case over its bound is a finding about a kernel or the planner, never a reason to scale tol.

That the engine's result does depend on the w_lo of a weak cell is shown on the device as well: with the filter entries of the case's
w_lo_cell rounded to binary16 precision -- their lo halves are then exactly 0, whatever the planner's power-of-two shift -- the float64
forward moves by D >= 4 x tol, and the engine's output must move by at least D - 2 x tol.
The coverage tests show that the cases reach the kernel forms the shipped hyper-parameter sets run."""
import functools

import numpy as np
import pytest

import inference_ref as R
from unmicst_amd import model, umx

pytestmark = pytest.mark.gpu

TABLE = R.load_table()
F6_CASES = [n for n in R.ARITH_CASES if TABLE[n]["tol_f6"] is not None]
HP_F6_CASES = [n for n in F6_CASES if R.ARITH_CASES[n][0] == R.HP_F6]


@functools.lru_cache(maxsize=None)
def _case(name):
    """(hp, blob, tiles, float64 probabilities) of a case: computed once, shared by the precisions, never written to."""
    hp, blob, x = R.case_inputs(name)
    p64 = R.forward64(hp, blob, x)
    for a in (blob, x, p64):
        a.setflags(write=False)
    return hp, blob, x, p64


@functools.lru_cache(maxsize=None)
def _case_without_w_lo(name):
    """(blob B' of the case with its w_lo_cell's filter rounded to binary16 precision, float64 probabilities of B', D): computed once"""
    hp, blob, x, p64 = _case(name)
    blob2 = R.blob_with_cell_rounded(hp, blob, TABLE[name]["w_lo_cell"])
    p64b = R.forward64(hp, blob2, x)
    for a in (blob2, p64b):
        a.setflags(write=False)
    return blob2, p64b, float(np.abs(p64b - p64).max())


@functools.lru_cache(maxsize=None)
def _engine_output(name, prec):
    """The five tiles of a case through max_batch = 3 in one precision: run once, shared, never written to."""
    hp, blob, x, _ = _case(name)
    assert x.shape[0] == 5
    with umx.Engine(hp, blob, max_batch=3, precision=prec) as eng:
        assert eng.precision == prec
        got = eng.forward_tiles(x)
    got.setflags(write=False)
    return got


def _tile_errors(got, p64):
    return np.abs(got.astype(np.float64) - p64).reshape(got.shape[0], -1).max(axis=1)


def _report(name, prec, errs, tol):
    print("%s %s: E_gpu %.3g = %.3f x tol %.3g   (per tile: %s)" % (name, prec, errs.max(), errs.max() / tol, tol,
                                                                 " ".join("%.2g" % e for e in errs)))


def _template_args(kernel):
    return kernel[kernel.index("<") + 1:-1].split(", ")


def _f6_sites(prof):
    """Launch names whose kernel is conv_f16x3<NT, KMT, NPH, DBG, MAXP, PK, D2S, F6, W2> with F6 (the eighth argument) set."""
    return {e["name"] for e in prof if e["kernel"].startswith("conv_f16x3<") and _template_args(e["kernel"])[7] == "true"}


def _profile_of(eng, x):
    eng.profile_enable(1)
    eng.forward_tiles(x)
    prof = eng.profile_read()
    eng.profile_enable(False)
    return prof


@pytest.mark.parametrize("prec", ["f32", "f16x3"])
@pytest.mark.parametrize("name", list(R.ARITH_CASES))
def test_five_tiles_within_a_quarter_of_one_lost_product(name, prec):
    hp, blob, x, p64 = _case(name)
    tol = TABLE[name]["tol"]
    got = _engine_output(name, prec)
    errs = _tile_errors(got, p64)
    _report(name, prec, errs, tol)
    assert np.all(errs <= tol), (name, prec, errs.tolist(), tol)


@pytest.mark.parametrize("prec", ["f32", "f16x3"])
@pytest.mark.parametrize("name", list(R.ARITH_CASES))
def test_the_output_moves_when_the_weak_cells_w_lo_is_taken_away(name, prec):
    """B' = the case's blob with the filter of its w_lo_cell (the weakest phase or N-block of lb.conv / lu*.convT / lu*.conv, whose
    filters the engine splits as stored) rounded to binary16 precision.  On the CPU D = max |forward64(B') - forward64(B)| >= 4 x tol;
    a correct engine is within tol of the float64 forward on either blob, so its two outputs differ by >= D - 2 x tol -- which an engine
    that never multiplied by that cell's w_lo (the same output for B and B', up to w_hi's last bit) cannot show."""
    hp, blob, x, p64 = _case(name)
    tol, cell = TABLE[name]["tol"], TABLE[name]["w_lo_cell"]
    blob2, p64b, D = _case_without_w_lo(name)
    assert R.qualifies_for_w_lo_test(cell) and R.kept(name, cell)
    assert D >= 4 * tol, (name, cell, D, tol)
    with umx.Engine(hp, blob2, max_batch=3, precision=prec) as eng:
        assert eng.precision == prec
        got2 = eng.forward_tiles(x)
    moved = float(np.abs(got2.astype(np.float64) - _engine_output(name, prec).astype(np.float64)).max())
    errs = _tile_errors(got2, p64b)
    print("%s %s %s: D %.3g = %.2f x tol, the engine moved by %.3g = %.3f x D (needed: %.3g); on B' E_gpu %.3g = %.3f x tol" % (
        name, prec, cell, D, D / tol, moved, moved / D, D - 2 * tol, errs.max(), errs.max() / tol))
    assert moved >= D - 2 * tol, (name, prec, cell, moved, D, tol)
    assert np.all(errs <= tol), (name, prec, errs.tolist(), tol)


@pytest.mark.parametrize("name", F6_CASES)
def test_five_tiles_f16f6_within_four_times_the_emulated_form(name):
    hp, blob, x, p64 = _case(name)
    tol_f6 = TABLE[name]["tol_f6"]
    with umx.Engine(hp, blob, max_batch=3, precision="f16f6") as eng:
        assert eng.precision == "f16f6"
        got = eng.forward_tiles(x)
        sites = _f6_sites(_profile_of(eng, x))
    errs = _tile_errors(got, p64)
    _report(name, "f16f6", errs, tol_f6)
    assert np.all(errs <= tol_f6), (name, errs.tolist(), tol_f6)
    # E_f6 was emulated with fp6 cross terms on exactly these launches
    assert sites == R.f6_launches(hp), (name, sites)
    with umx.Engine(hp, blob, max_batch=3, precision="f16x3") as eng:
        base = eng.forward_tiles(x)
    assert not np.array_equal(got, base), "the fp6 form was not used on any layer"


@pytest.mark.parametrize("name", HP_F6_CASES)
def test_f16f6_tile_partner_does_not_matter(name):
    """The F6 form runs two tiles per workgroup: a tile's bits must not depend on its partner.  max_batch = 4 against max_batch = 3
    (equal batches: both split five tiles 3 + 2), and one batch of five, which pairs the tiles (0 1)(2 3)(4 -) instead of
    (0 1)(2 -)(3 4)."""
    hp, blob, x, _ = _case(name)
    outs = []
    for mb in (3, 4, 5):
        with umx.Engine(hp, blob, max_batch=mb, precision="f16f6") as eng:
            outs.append(eng.forward_tiles(x))
    assert np.array_equal(outs[0].view(np.uint32), outs[1].view(np.uint32))
    assert np.array_equal(outs[0].view(np.uint32), outs[2].view(np.uint32))


# ------------------------------------------------------------------------------------------------ kernel-instantiation coverage
# instantiations of the shipped graphs that no graph of <= 64 pixels reaches: (precision, kernel, reason); at most two
UNREACHED = ()


def _instantiations(hp, blob, prec, n=1):
    x = np.random.default_rng(1).normal(size=(n, hp.imSize, hp.imSize, hp.nChannels)).astype(np.float32)
    with umx.Engine(hp, blob, max_batch=max(n, 1), precision=prec) as eng:
        prof = _profile_of(eng, x)
    return prof


@pytest.mark.parametrize("prec", ["f32", "f16x3", "f16f6"])
def test_the_cases_reach_every_kernel_instantiation_of_the_shipped_graphs(prec):
    """Union of the kernel names (umx_profile_read) launched over ARITH_CASES in this precision >= what the six model.KNOWN_HP
    graphs launch on one tile (random weights), but for UNREACHED.  Under f16f6 every case's F6 launches are also the set
    inference_ref.f6_launches states (empty where no launch takes the form)."""
    assert len(UNREACHED) <= 2
    reached = set()
    for name in R.ARITH_CASES:
        hp, blob, x, _ = _case(name)
        with umx.Engine(hp, blob, max_batch=3, precision=prec) as eng:
            prof = _profile_of(eng, x)
        reached |= {e["kernel"] for e in prof}
        if prec == "f16f6":
            assert _f6_sites(prof) == R.f6_launches(hp), (name, _f6_sites(prof))
    missing = {}
    for key, hp in model.KNOWN_HP.items():
        for e in _instantiations(hp, model.random_blob(hp, seed=1), prec):
            if e["kernel"] not in reached:
                missing.setdefault(e["kernel"], []).append("%s %s" % (key, e["name"]))
    print("%s: %d instantiations reached by the cases; of the shipped graphs' not among them: %s" % (prec, len(reached), missing or "none"))
    allowed = {k for p, k, _ in UNREACHED if p == prec}
    assert set(missing) <= allowed, (prec, missing)
    assert allowed <= set(missing), "an UNREACHED entry is reached (or never launched): remove it"
