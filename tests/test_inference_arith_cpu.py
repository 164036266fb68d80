"""The reference side of the inference arithmetic gate, checked on the CPU (tests/inference_ref.py).

* the float64 forward is pinned to oracle.forward -- the restatement the reference project's golden vectors pin -- within 1e-6
  (fp32 against float64 was measured at <= 4.2e-7 on all of these: profiles/r06/fp8_fp6_cross_term_accuracy_cpu.log, column `exact`);
* every number of tests/arith_cases.json reproduces from the emulation to 2 %, so the committed tolerances cannot drift from it;
* every case meets the conditions that make its tolerance mean something (inference_ref.case_conditions): a product lost on any
  single layer, or in any single cell of a launch (inference_ref.cells: a launch of a layer that has several, the shortcut's K
  segment, one output phase of a transposed convolution, one N-block), stands 4 x over the bound, the correct arithmetic sits 8 x
  under it, 1e-6 <= tol <= 2e-5, and for the F6 form tol_f6 = 4 x E_f6 with min(E_drop, E_cell) >= 2 x tol_f6.  These are conditions on
  the reference side alone: no GPU figure enters them.  Every cell of every case is emulated here, under both fault plans: nothing is
  sampled (the whole file: 25 s before the cells, about 90 s with them, on eight cores);
* the N-block boundaries the cells use (inference_ref.n_blocks, the planner's rule restated) are the host plan's, on every launch of
  every case (umx.infer_plan: host only);
* for the cell tests/test_gpu_arith.py takes away the w_lo of (w_lo_cell), the float64 forward itself moves by D >= 4 x tol."""
import functools
import re

import numpy as np
import pytest
import torch

import helpers
import inference_ref as R
from oracle import oracle, pi2d_oracle
from unmicst_amd import model, umx

F64_TOL = 1e-6


@pytest.mark.parametrize("name", sorted(helpers.small_hps()))
def test_float64_forward_matches_the_oracle_on_the_small_graphs(name):
    hp = helpers.small_hps()[name]
    blob = model.random_blob(hp, seed=11)
    x = np.random.default_rng(5).normal(size=(3, hp.imSize, hp.imSize, hp.nChannels)).astype(np.float32)
    p64 = R.forward64(hp, blob, x)
    assert p64.dtype == np.float64 and p64.shape == (3, hp.imSize, hp.imSize, hp.nClasses)
    err = float(np.abs(oracle.forward(hp, blob, x) - p64).max())
    print("%s: max |oracle - p64| = %.3g" % (name, err))
    assert err <= F64_TOL, (name, err)


@pytest.mark.parametrize("key", ["nucleiDAPI", "mousenucleiDAPI", "CytoplasmIncell"])
def test_float64_forward_matches_the_oracle_on_the_shipped_models(key):
    """Trained weights on real tiles of the reference's sample image (the legacy graph: 5 x 5 and 3 x 3 filters, 1 x 1 shortcuts,
    BatchNorm after the activation, extra convolutions, 2 and 3 classes)."""
    hp, blob, mean, std = helpers.load_nuclei_dapi(key)
    I = helpers.legacy_preprocess(helpers.load_sample_105()[0])
    pi = pi2d_oracle.PI2DOracle(I, hp.imSize, hp.margin, "accumulate")
    x = pi2d_oracle.normalised_batch(pi, 5, 2, hp.nChannels, mean, std, False)
    err = float(np.abs(oracle.forward(hp, blob, x) - R.forward64(hp, blob, x)).max())
    print("%s: max |oracle - p64| = %.3g" % (key, err))
    assert err <= F64_TOL, (key, err)


def test_fault_plans_drop_exactly_one_cross_term():
    g = torch.Generator().manual_seed(0)
    A, W = torch.randn(40, 70, generator=g), torch.randn(70, 9, generator=g) * 0.1
    exact = A.double() @ W.double()
    full, xlo, wlo = (R.gemm(A, W, p).double() for p in ("f16x3", "f16x3-xlo", "f16x3-wlo"))
    assert torch.equal(xlo, R.gemm(A, W, "f16x2").double())
    ah, al = R.split16(A)
    sh = 2.0 ** (14 - np.frexp(float(W.abs().max()))[1])
    wh, wl = R.split16(W * sh)
    # what each plan leaves out, to the rounding of the float32 results (|result| ~ 1: 6e-8)
    assert (full - exact).abs().max() < 1e-6
    assert ((full - xlo) - al.double() @ wh.double() / sh).abs().max() < 5e-7
    assert ((full - wlo) - ah.double() @ wl.double() / sh).abs().max() < 5e-7
    assert (full - xlo).abs().max() > 1e-5 and (full - wlo).abs().max() > 1e-5


def test_deep_path_blob_scales_only_the_two_halves_of_the_concat_filters():
    hp = helpers.small_hps()["v2_deep"]
    assert np.array_equal(R.deep_path_blob(hp, 7, None), model.random_blob(hp, seed=7))
    a, b = model.tensors_from_blob(hp, model.random_blob(hp, seed=7)), model.tensors_from_blob(hp, R.deep_path_blob(hp, 7, 0.125))
    n = hp.nOutX
    for k in a:
        if k.endswith(".w2"):
            c = n[int(k[2:k.index(".")])]            # the skip tensor's channels come first in concat [skip, up]
            assert a[k].shape[2] == c + b[k].shape[3]
            assert np.array_equal(b[k][:, :, :c], a[k][:, :, :c] * np.float32(0.125))
            assert np.array_equal(b[k][:, :, c:], a[k][:, :, c:] * np.float32(np.sqrt(2.0)))
        else:
            assert np.array_equal(a[k], b[k]), k


def test_phase_eq_scales_only_the_taps_of_the_thin_phases():
    for key, scale in (("v2_deep", {1: 2.0, 2: np.sqrt(2.0), 4: 1.0}), ("legacy_k5", {4: 1.5, 6: np.sqrt(1.5), 9: 1.0})):
        hp = helpers.small_hps()[key]
        a, b = model.tensors_from_blob(hp, model.random_blob(hp, seed=7)), model.tensors_from_blob(hp, R.deep_path_blob(hp, 7, None, 1))
        for k in a:
            if not k.endswith(".wt"):
                assert np.array_equal(a[k], b[k]), k
                continue
            seen = np.zeros(a[k].shape[:2], int)
            for ph in R.PHASES:
                taps = R.phase_taps(hp.ks, ph)
                for t in taps:
                    seen[t] += 1
                    assert np.array_equal(b[k][t], a[k][t] * np.float32(scale[len(taps)])), (k, ph, t)
            assert np.all(seen == 1)          # every tap belongs to exactly one phase


def test_a_cell_plan_faults_its_cell_and_nothing_else():
    g = torch.Generator().manual_seed(1)
    x = torch.randn(2, 24, 6, 5, generator=g)
    w, wt = torch.randn(3, 3, 24, 40, generator=g) * 0.1, torch.randn(3, 3, 40, 24, generator=g) * 0.1
    for fault in R.FAULT_PLANS:
        full, bad = R.conv_same(x, w, "f16x3"), R.conv_same(x, w, fault)
        got = R.conv_same(x, w, (fault, "nblk", (16, 32)))
        assert torch.equal(got[:, 16:32], bad[:, 16:32]) and torch.equal(got[:, :16], full[:, :16]) and torch.equal(got[:, 32:], full[:, 32:])
        assert not torch.equal(bad[:, 16:32], full[:, 16:32])
        full, bad = R.conv_transpose_s2(x, wt, "f16x3"), R.conv_transpose_s2(x, wt, fault)
        got = R.conv_transpose_s2(x, wt, (fault, "nblk", (32, 40)))
        assert torch.equal(got[:, 32:], bad[:, 32:]) and torch.equal(got[:, :32], full[:, :32])
        for oy, ox in R.PHASES:
            got = R.conv_transpose_s2(x, wt, (fault, "phase", (oy, ox)))
            rest = torch.ones(12, 10, dtype=torch.bool)
            rest[oy::2, ox::2] = False
            assert torch.equal(got[:, :, oy::2, ox::2], bad[:, :, oy::2, ox::2]) and torch.equal(got[:, :, rest], full[:, :, rest])
            assert not torch.equal(bad[:, :, oy::2, ox::2], full[:, :, oy::2, ox::2])
    # the float64 transposed convolution has the same phases: only phase (1, 1) reads the centre tap of a 3 x 3 filter
    wt2 = wt.clone()
    wt2[1, 1] *= 2
    d = (R._convT64(x.double(), wt2.double()) - R._convT64(x.double(), wt.double())) != 0
    assert d[:, :, 1::2, 1::2].all() and not d[:, :, 0::2, :].any() and not d[:, :, :, 0::2].any()
    assert R.phase_taps(3, (1, 1)) == [(1, 1)] and len(R.phase_taps(3, (0, 0))) == 4 and sorted(len(R.phase_taps(5, p)) for p in R.PHASES) == [4, 6, 6, 9]


def test_the_cells_of_a_graph():
    """Launch cells only where a layer has several launches; a shortcut cell only with extra convolutions (without them the engine
    sums the shortcut's filter into the convolution's at plan time); four phases per transposed convolution; N-blocks that tile the
    output channels of the launches that have two or more."""
    S = helpers.small_hps()
    names = lambda hp: [c for c, _, _ in R.cells(hp)]            # noqa: E731
    assert names(S["legacy_k3_x2"]) == ["ld0.conv1", "ld0.extra0", "ld0.extra1", "ld0.short"] + [   # (lb: one launch)
        "lu0.convT", "lu0.convT@p00", "lu0.convT@p01", "lu0.convT@p10", "lu0.convT@p11", "lu0.conv", "lu0.extra0", "lu0.extra1"]
    got = names(R.HP_F6)
    assert "lb.conv@n0:144" in got and "lb.conv@n144:288" in got and not [c for c in got if c.startswith("ld") or c == "lb.conv"]
    for name, (hp, _, _, _, _) in R.ARITH_CASES.items():
        got, couts = names(hp), R.launch_couts(hp)
        assert len(got) == len(set(got))
        assert ("ld0.short" in got) == (hp.nExtraConvs > 0), name
        for launch, (nt, nb) in R.n_blocks(hp).items():
            assert [c for c in got if c.startswith(launch + "@p")] == (["%s@p%d%d" % (launch, oy, ox) for oy, ox in R.PHASES] if launch.endswith("convT") else [])
            edges = [tuple(int(v) for v in c.split("@n")[1].split(":")) for c in got if c.startswith(launch + "@n")]
            if nb == 1:
                assert edges == []
                continue
            assert len(edges) == nb and edges[0][0] == 0 and edges[-1][1] == couts[launch], (name, launch)
            assert all(a[1] == b[0] for a, b in zip(edges, edges[1:])) and all(c1 - c0 == 16 * nt for c0, c1 in edges[:-1])


_PLAN_LINE = re.compile(r"^\[umx plan\] (\S+) +(?:fused-phase |packed |fp6-cross )*NT (\d+) x (\d+) blocks,")


@pytest.mark.parametrize("name", list(R.ARITH_CASES))
def test_the_n_block_restatement_is_the_host_plan(name):
    hp, blob, _ = R.case_inputs(name)
    for f6 in (False, True):
        plan = {}
        for ln in umx.infer_plan(hp, f6, 0, blob, batches=(5,)):
            m = _PLAN_LINE.match(ln)
            assert m, ln
            plan[m.group(1)] = (int(m.group(2)), int(m.group(3)))
        assert plan == R.n_blocks(hp), (name, f6)
    assert any(nb >= 2 for hp, *_ in R.ARITH_CASES.values() for _, nb in R.n_blocks(hp).values())


def test_round11_leaves_no_lo_half_under_any_power_of_two_shift():
    w = np.random.default_rng(3).normal(0, 0.05, size=4000).astype(np.float32)
    r = R.round11(w)
    assert np.all(np.abs(r - w) <= np.abs(w) * 2.0 ** -11) and np.any(r != w)
    assert np.array_equal(R.round11(r), r) and np.array_equal(R.round11(w * np.float32(2.0 ** 7)), r * np.float32(2.0 ** 7))
    for sh in (14, 16, 17):           # (where the planner's shift puts filters like these: every entry in binary16's normal range)
        hi, lo = R.split16(torch.from_numpy(r) * 2.0 ** sh)
        assert torch.equal(hi, torch.from_numpy(r) * 2.0 ** sh) and not lo.any(), sh
    assert R.split16(torch.from_numpy(w) * 2.0 ** 16)[1].any()


def test_the_table_lists_the_cases_and_the_f6_cases_are_the_ones_with_an_f6_launch():
    table = R.load_table()
    assert sorted(table) == sorted(R.ARITH_CASES)
    assert 8 <= len(R.ARITH_CASES) <= 14          # (twelve, the one the kernel-form coverage asked for, and the F6 cases' companion)
    for name, (hp, seed, damp, n, phase_eq) in R.ARITH_CASES.items():
        assert hp.imSize <= 64 and n == 5
        assert (table[name]["E_f6"] is not None) == bool(R.f6_launches(hp)) == (table[name]["tol_f6"] is not None), name
    assert R.f6_launches(R.HP_F6) == {"lb.conv"}
    assert sum(1 for hp, *_ in R.ARITH_CASES.values() if R.f6_launches(hp)) >= 2


# tol of every case while E_drop alone set it (whole layers faulted): the cells may only have tightened it
FORMER_TOL = {"d2s_n22_c3": 7.623e-06, "d2s_n40_c1": 6.555e-06, "legacy_k3_x2": 5.744e-06, "legacy_k5": 1.702e-06, "v2_28_switches": 4.398e-06,
              "v2_72_f6": 9.790e-06, "v2_72_f6_damp": 1.4488e-05, "v2_deep_damp": 1.967e-06, "v2_duo_like": 1.991e-06, "v2_extra": 7.203e-06,
              "v2_k5": 4.932e-06, "v2_solo_like": 2.170e-06, "v2_wide": 4.619e-06, "v2_72_phase": 2e-5}    # (the last: new, the cap)


@functools.lru_cache(maxsize=None)
def _sweep(name):
    """(numbers, {cell: {fault plan: error}}) of a case: every cell emulated under both fault plans, once"""
    per_cell = {}
    return R.case_numbers(name, per_cell=per_cell), per_cell


def test_cells_left_to_a_companion_exist_there():
    for name, (other, what) in R.HELD_ELSEWHERE.items():
        mine, theirs = ([c for c, _, _ in R.cells(R.ARITH_CASES[n][0])] for n in (name, other))
        assert mine == theirs and any(what in c for c in mine) and other not in R.HELD_ELSEWHERE
        assert R.n_blocks(R.ARITH_CASES[name][0]) == R.n_blocks(R.ARITH_CASES[other][0])      # the same N-tiles and blocks, launch by launch
        assert not R.f6_launches(R.ARITH_CASES[other][0])


@pytest.mark.parametrize("name", list(R.ARITH_CASES))
def test_committed_numbers_reproduce_and_meet_the_conditions(name):
    """... and every cell of the case, under either fault plan, stands at >= 4 x the committed tol (to the 2 % the table reproduces
    to; at 4 x the recomputed one exactly).  The recorded worst_cell and w_lo_cell are held by their figures, not by their names: two
    cells within a per cent of each other may change places with the CPU's summation order."""
    want = R.load_table()[name]
    got, per_cell = _sweep(name)
    print(name, got)
    assert sorted(got) == sorted(want)
    for k, v in got.items():
        if v is None:
            assert want[k] is None, (name, k)
        elif not isinstance(v, str):
            assert want[k] == pytest.approx(v, rel=0.02), (name, k, want[k], v)
    assert R.case_conditions(want) == [], name
    assert R.case_conditions(got) == [], name
    assert want["tol"] <= FORMER_TOL[name], name
    hp = R.ARITH_CASES[name][0]
    assert sorted(per_cell) == sorted(c for c, _, _ in R.cells(hp)) and all(sorted(v) == sorted(R.FAULT_PLANS) for v in per_cell.values())
    for cell, row in per_cell.items():
        # no cell is left without a case that holds it at 4 x: this one, or for the cells it hands over (HELD_ELSEWHERE) its companion
        holder = name if R.kept(name, cell) else R.HELD_ELSEWHERE[name][0]
        tol_got, tol_want, held = _sweep(holder)[0]["tol"], R.load_table()[holder]["tol"], _sweep(holder)[1][cell]
        assert R.kept(holder, cell)
        for fault, e in row.items():
            print("    %-22s %s %.3g = %.2f x tol; in %s %.3g = %.2f x its tol" % (cell, fault, e, e / want["tol"], holder, held[fault], held[fault] / tol_want))
            assert held[fault] >= 4 * tol_got and held[fault] >= 0.98 * 4 * tol_want, (name, cell, fault, holder, held[fault])
    cell, lost = want["worst_cell"].split()
    assert R.kept(name, cell) and per_cell[cell]["f16x3-" + lost] == pytest.approx(want["E_cell"], rel=0.02)
    q = {c: min(row.values()) for c, row in per_cell.items() if R.kept(name, c) and R.qualifies_for_w_lo_test(c)}
    assert want["w_lo_cell"] in q and q[want["w_lo_cell"]] <= 1.02 * min(q.values())
    if cell in q:
        assert q[want["w_lo_cell"]] == pytest.approx(want["E_cell"], rel=0.02)
    assert want["E_cell"] <= 0.999 * want["D_w_lo"] and want["D_w_lo"] == pytest.approx(got["D_w_lo"], rel=1e-6)


@pytest.mark.parametrize("name", list(R.ARITH_CASES))
def test_the_float64_forward_moves_by_four_tol_without_the_weak_cells_w_lo(name):
    """What tests/test_gpu_arith.py then asks of the engine: B' = the case's blob with w_lo_cell's filter entries rounded to binary16
    precision; only those entries change, and D = max |forward64(B') - forward64(B)| >= 4 x tol."""
    want = R.load_table()[name]
    hp, blob, _ = R.case_inputs(name)
    blob2, D = R.w_lo_sensitivity(name, want["w_lo_cell"])
    assert D == pytest.approx(want["D_w_lo"], rel=1e-6)
    a, b = model.tensors_from_blob(hp, blob), model.tensors_from_blob(hp, blob2)
    key, idx = R.cell_filter_view(hp, a, want["w_lo_cell"])
    for k in a:
        if k != key:
            assert np.array_equal(a[k], b[k]), k
    mask = np.zeros(a[key].shape, bool)
    mask[idx] = True
    assert np.array_equal(a[key][~mask], b[key][~mask]) and np.array_equal(b[key][mask], R.round11(a[key][mask]))
    assert 0 < mask.sum() < mask.size and np.mean(a[key][mask] != b[key][mask]) > 0.9
    print("%s %s: D %.3g = %.2f x tol" % (name, want["w_lo_cell"], D, D / want["tol"]))
    assert D >= 4 * want["tol"], (name, want["w_lo_cell"], D, want["tol"])
