"""The reference side of the inference arithmetic gate, checked on the CPU (tests/inference_ref.py).

* the float64 forward is pinned to oracle.forward -- the restatement the reference project's golden vectors pin -- within 1e-6
  (fp32 against float64 was measured at <= 4.2e-7 on all of these: profiles/r06/fp8_fp6_cross_term_accuracy_cpu.log, column `exact`);
* every number of tests/arith_cases.json reproduces from the emulation to 2 %, so the committed tolerances cannot drift from it;
* every case meets the conditions that make its tolerance mean something (inference_ref.case_conditions): a product lost on any
  single layer stands 4 x over the bound, the correct arithmetic sits 8 x under it, 1e-6 <= tol <= 2e-5, and for the F6 form
  tol_f6 = 4 x E_f6 with E_drop >= 2 x tol_f6.  These are conditions on the reference side alone: no GPU figure enters them."""
import numpy as np
import pytest
import torch

import helpers
import inference_ref as R
from oracle import oracle, pi2d_oracle
from unmicst_amd import model

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


def test_the_table_lists_the_cases_and_the_f6_cases_are_the_ones_with_an_f6_launch():
    table = R.load_table()
    assert sorted(table) == sorted(R.ARITH_CASES)
    assert 8 <= len(R.ARITH_CASES) <= 13          # (the issue's twelve and the one the kernel-form coverage asked for)
    for name, (hp, seed, damp, n) in R.ARITH_CASES.items():
        assert hp.imSize <= 64 and n == 5
        assert (table[name]["E_f6"] is not None) == bool(R.f6_launches(hp)) == (table[name]["tol_f6"] is not None), name
    assert R.f6_launches(R.HP_F6) == {"lb.conv"}
    assert sum(1 for hp, _, _, _ in R.ARITH_CASES.values() if R.f6_launches(hp)) >= 2


@pytest.mark.parametrize("name", list(R.ARITH_CASES))
def test_committed_numbers_reproduce_and_meet_the_conditions(name):
    want = R.load_table()[name]
    got = R.case_numbers(name)
    print(name, got)
    assert sorted(got) == sorted(want)
    for k, v in got.items():
        if v is None:
            assert want[k] is None, (name, k)
        else:
            assert want[k] == pytest.approx(v, rel=0.02), (name, k, want[k], v)
    assert R.case_conditions(want) == [], name
    assert R.case_conditions(got) == [], name
