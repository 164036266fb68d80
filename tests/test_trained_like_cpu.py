"""The trained-like blob generator, its tiles and the committed table tests/trained_cases.json, checked on the CPU
(tests/trained_like.py; the GPU side is tests/test_gpu_trained_like.py).

* the generator is deterministic and stays with its donors: per filter, the kurtosis, the per-channel RMS max / median (input and
  output channels) and rms * sqrt(fan_in) against the donor tensor it was resampled from.  Measured over three graphs:
  kurtosis 0.48 ... 1.74 x the donor's (the donors differ among themselves by 1.1 ... 5.0 x per role), channel RMS max / median
  0.94 ... 1.37 x (donors: 1.0 ... 4.3 x), rms * sqrt(fan_in) equal to float32 rounding.  Bounds: 2.5 x, 1.5 x, 1e-6;
* moving statistics are the calibration tiles' own moments times the donors' measured mismatch, and the calibrated networks are
  not saturated: at most SATURATION_CAP of a case's test pixels have a class probability above 0.999 (measured 0.008 ... 0.062, cap 0.15);
* the tile families are what the cases say, calibration and test tiles come from disjoint halves of 105.tif;
* the F6 launch sets of the cases are the ones inference_ref.f6_launches derives;
* the committed table reproduces from the emulation to 2 %: for tl_72_lb, tl_144_lb and tl_72_l3 (trained_like.SWEPT_IN_TEST) every
  figure of the row is recomputed -- all tiles, the full fault sweep, tol, tol_f6, the saturated share.  RESTRICTED are the two duo
  cases, tl_duo128 and tl_duo256, whose sweep takes 4 - 8 minutes: for them E_ref and E_f6 are recomputed on the first tile (the table
  records them as E_ref_tile0 / E_f6_tile0) and the saturated share on all tiles; their E_drop, all-tile E_ref and all-tile E_f6 are
  checked only by ``python tests/trained_like.py tl_duo128 tl_duo256``.  Every row meets case_conditions."""
import numpy as np
import pytest
import torch

import inference_ref as R
import trained_like as TL
from unmicst_amd import model

KURTOSIS_FACTOR = 2.5
CHANNEL_RMS_FACTOR = 1.5
SMALL = model.HParams(model.GRAPH_V2, 32, 2, 3, 12, 3, 3, 0)


def test_the_generator_is_deterministic_and_seeded():
    cal = TL.cal_tiles(SMALL)
    a, b, c = (TL.trained_like_blob(SMALL, s, cal) for s in (3, 3, 4))
    assert a.dtype == np.float32 and a.size == model.random_blob(SMALL).size
    assert np.array_equal(a, b) and not np.array_equal(a, c)
    assert np.isfinite(a).all()
    with pytest.raises(ValueError):
        TL.trained_like_blob(model.HParams(model.GRAPH_LEGACY, 32, 1, 3, 8, 2, 3, 0), 3, cal)


@pytest.mark.parametrize("name", ["tl_72_l3", "tl_duo128"])
def test_filters_keep_their_donors_statistics(name):
    hp, blob, _ = TL.case_inputs(name)
    rep = {}
    again = TL.trained_like_blob(hp, TL.TRAINED_CASES[name][1], TL.cal_tiles(hp), report=rep)
    assert np.array_equal(again, blob)
    seen = set()
    for n, w in model.tensors_from_blob(hp, blob).items():
        if ".bn." in n:
            continue
        dhp, dT, _, _ = TL.donor(rep[n])
        dn = TL.donor_name(n, hp, dhp)
        role = n if n in ("lb.w", "lt.w") else n.split(".")[1]
        assert (dn if dn in ("lb.w", "lt.w") else dn.split(".")[1]) == role
        seen.add(role)
        g, d = TL.filter_stats(n, w), TL.filter_stats(dn, dT[dn])
        assert 1 / KURTOSIS_FACTOR <= (g[0] + 3) / (d[0] + 3) <= KURTOSIS_FACTOR, (n, g, d)
        for k in (1, 2):
            assert 1 / CHANNEL_RMS_FACTOR <= g[k] / d[k] <= CHANNEL_RMS_FACTOR, (n, k, g, d)
        assert g[3] == pytest.approx(d[3], rel=1e-6), (n, g, d)
    assert seen == set(TL.ROLES)
    assert set(rep.values()) == set(TL.DONORS)            # every donor contributes


def test_donor_mismatch_is_measured_on_every_donor():
    for key in TL.DONORS:
        mm = TL.donor_mismatch(key)
        hp = TL.donor(key)[0]
        assert mm.ndim == 2 and mm.shape[1] == 2 and 0.8 * sum(hp.nOutX[1:hp.nLayers + 1]) <= len(mm) <= sum(hp.nOutX[1:hp.nLayers + 1])
        assert np.isfinite(mm).all() and (mm[:, 1] > 0).all()
        print(key, "mean offset / sigma: 5 %% %.2f median %.2f 95 %% %.2f;  variance factor: 5 %% %.2f median %.2f 95 %% %.2f" % (
            *np.percentile(mm[:, 0], [5, 50, 95]), *np.percentile(mm[:, 1], [5, 50, 95])))
    own = TL.donor_mismatch("nucleiDAPI")                  # its own kind of image: stored statistics near the seen ones
    assert np.abs(own[:, 0]).max() < 1 and 0.25 < own[:, 1].min() and own[:, 1].max() < 4


def test_moving_statistics_are_the_calibration_moments_times_a_mismatch():
    """Re-running the calibration tiles through the finished blob: every BatchNorm's stored mean lies within the mismatch's range of
    the moments it sees, so no layer is normalised with statistics from another network."""
    cal = TL.cal_tiles(SMALL)
    blob = TL.trained_like_blob(SMALL, 3, cal)
    lo = min(TL.donor_mismatch(k)[:, 1].min() for k in TL.DONORS)
    hi = max(TL.donor_mismatch(k)[:, 1].max() for k in TL.DONORS)
    dmax = max(np.abs(TL.donor_mismatch(k)[:, 0]).max() for k in TL.DONORS)
    seen = []

    def hook(p, t, T):
        m, v = t.mean(dim=(0, 2, 3)).numpy(), t.var(dim=(0, 2, 3), unbiased=False).numpy()
        f = T[p + ".bn.var"].numpy() / v
        d = (T[p + ".bn.mean"].numpy() - m) / np.sqrt(v)
        assert (f >= lo * (1 - 1e-5)).all() and (f <= hi * (1 + 1e-5)).all(), p
        assert (np.abs(d) <= dmax * (1 + 1e-5) + 1e-5).all(), p
        seen.append(p)

    R.forward64(SMALL, R.torch_tensors(SMALL, blob, torch.float64), cal, bn_hook=hook)
    assert seen == ["ld0", "ld1", "ld2", "lb", "lu2", "lu1", "lu0", "lt"]


def test_tile_families_and_disjoint_halves():
    _, _, mean, std = TL.donor(TL.NORM_DONOR)
    assert TL.TILE_ORDER[:3] == ("real0", "padding", "noise1")
    assert sorted(TL.TILE_ORDER) == sorted(["real0", "real1", "real2", "real3", "padding", "const0", "const0.983", "ramp", "noise0.1",
                                            "noise1", "noise4", "blobs"])
    for S in (64, 128, 256):
        assert all(y + S <= 416 for y, _ in TL._cal_positions(S, 4)) and all(x + S <= 960 for _, x in TL._cal_positions(S, 4))
        assert all(416 <= y and y + S <= 832 and x + S <= 960 for y, x in TL._test_positions(S, 4))
    hp = R.HP_F6
    x = TL.tiles_for(hp, 5, 12)
    assert x.shape == (12, 64, 64, 2) and x.dtype == np.float32
    fam = dict(zip(TL.TILE_ORDER, x))
    assert np.all(fam["padding"] == np.float32(-mean / std)) and np.array_equal(fam["padding"], fam["const0"])
    assert np.all(fam["const0.983"] == np.float32((0.983 - mean) / std))
    for s in ("0.1", "1", "4"):
        assert fam["noise" + s].std() == pytest.approx(float(s), rel=0.05)
        assert not np.array_equal(fam["noise" + s][..., 0], fam["noise" + s][..., 1])
    for k in ("real0", "real1", "real2", "real3", "ramp", "blobs"):
        assert np.array_equal(fam[k][..., 0], fam[k][..., 1])                   # one plane in both channels
        assert fam[k].min() >= np.float32(-mean / std) and fam[k].max() <= np.float32((0.983 - mean) / std)
        assert fam[k].std() > 0.05
    r = fam["ramp"][..., 0]
    assert r[0, 0] == np.float32(-mean / std) and r[-1, -1] == np.float32((0.983 - mean) / std) and np.all(np.diff(r, axis=0) > 0)
    assert np.array_equal(TL.tiles_for(hp, 5, 5), x[:5])


def test_the_cases_and_their_f6_launch_sets():
    table = TL.load_table()
    assert list(table) == sorted(TL.TRAINED_CASES) and len(TL.TRAINED_CASES) == 5
    assert TL.TRAINED_CASES["tl_72_lb"][0] == R.HP_F6
    assert TL.TRAINED_CASES["tl_duo128"][0] == model.KNOWN_HP["nucleiDAPILAMIN"]
    assert TL.TRAINED_CASES["tl_duo256"][0] == model.KNOWN_HP["synthetic-256"]
    assert [(c[2], c[3]) for c in TL.TRAINED_CASES.values()] == [(12, 5), (12, 5), (5, 3), (5, 3), (3, 2)]
    for name, (hp, seed, n, mb) in TL.TRAINED_CASES.items():
        assert R.f6_launches(hp) == TL.F6_LAUNCHES[name], name
        assert TL.case_conditions(table[name]) == [], (name, TL.case_conditions(table[name]))
    assert TL.F6_LAUNCHES["tl_duo256"] == {"ld3.conv", "ld4.conv", "lu4.conv", "lu3.conv"}
    assert TL.F6_LAUNCHES["tl_72_l3"] == {"ld2.conv", "lb.conv", "lu2.conv"}
    n = TL.TRAINED_CASES["tl_144_lb"][0].nOutX
    assert (n[2], n[3]) == (288, 576)                     # lb.conv: K = 9 x 288 = 2 592, 36 N-tiles = four blocks of nine


@pytest.mark.parametrize("name", list(TL.TRAINED_CASES))
def test_committed_numbers_reproduce(name):
    want = TL.load_table()[name]
    if name in TL.SWEPT_IN_TEST:
        got = TL.case_numbers(name)
        assert sorted(got) == sorted(want)
        assert TL.case_conditions(got) == [], name
    else:
        assert name in ("tl_duo128", "tl_duo256")
        one = TL.case_numbers(name, tiles=1, sweep=False)
        hp, blob, x = TL.case_inputs(name)
        got = {"E_ref_tile0": one["E_ref"], "E_f6_tile0": one["E_f6"], "saturated": TL.saturated_share(R.forward64(hp, blob, x))}
        assert got["saturated"] <= TL.SATURATION_CAP
    print(name, got)
    for k, v in got.items():
        if isinstance(v, bool):
            assert want[k] == v, (name, k)
        else:
            assert want[k] == pytest.approx(v, rel=0.02, abs=1e-9 if k == "saturated" else 0), (name, k, want[k], v)
    assert want["E_ref_tile0"] <= want["E_ref"] and want["E_f6_tile0"] <= want["E_f6"]
