"""GPU tests of the inference kernels' memory discipline, in the engine's debug guard mode (UMX_DEBUG_GUARD, include/umx.h).

Every device buffer of a context then sits between two red zones filled with one byte; the call-scoped buffers -- activations, tile
staging, the per-call scratch of the image entries and of the sharded entries -- are filled with that byte at allocation and again at
the start of every public entry that enqueues work.  Two properties are checked on the same runs:
  no stray writes  every entry checks every zone at its end (umx_infer_image_wait for a submitted call) and fails with UMX_ERR_GUARD,
                   naming the buffer, if one changed;
  no stray reads   the same sequence of calls under the fills 0x00, 0xFF (a binary16 / fp32 NaN) and 0x7F (a large value a max cannot
                   drop) gives bit-identical outputs -- and the bits of a run without the variable.  A padded channel, a pixel past
                   the last image of a ragged batch, the empty half of an F6 tile pair, the tail of the last XCD range or a halo slot
                   that is read and multiplied by zero shows here; so does a stitch or a download that runs ahead of its producer,
                   because a repeated call starts from poison and not from the previous call's results.
The guarded runs go first: a stray write is named there before a run without red zones could land it in a live buffer.  Launches and
reduction orders are fixed, so the equality needs no tolerance."""
import functools
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

import helpers
import inference_ref as R
from test_gpu_switches import SWITCHES, _kernels_run
from test_gpu_world8 import ThreadWorld, _run_ranks
from unmicst_amd import model, umx

pytestmark = pytest.mark.gpu

FILLS = ("0x00", "0xff", "0x7f")
TABLE = R.load_table()
MARGIN = 4096                      # sentinel bytes in front of and behind a device output handed to a *_dev entry
SENTINEL = 0xA5


def _under(monkeypatch, fills, body):
    """body() under every fill, then once without the variable -> ({fill: output}, plain output)."""
    got = {}
    for fill in fills:
        monkeypatch.setenv("UMX_DEBUG_GUARD", fill)
        try:
            got[fill] = body()               # (UmxError ERR_GUARD from any call fails the test)
        finally:
            monkeypatch.delenv("UMX_DEBUG_GUARD", raising=False)
    return got, body()


def _same(a, b, what):
    assert a.keys() == b.keys(), what
    for k in a:
        x, y = np.asarray(a[k]), np.asarray(b[k])
        assert x.shape == y.shape and x.dtype == y.dtype and x.tobytes() == y.tobytes(), (what, k, int((x != y).sum()))


def _all_same(got, plain, what):
    for fill, out in got.items():
        _same(out, plain, "%s under UMX_DEBUG_GUARD=%s against the plain run" % (what, fill))


class _Margined:
    """A device region of n bytes with MARGIN sentinel bytes on both sides (one torch allocation)."""

    def __init__(self, n):
        import torch
        self.n = n
        self.buf = torch.full((MARGIN + n + MARGIN,), SENTINEL, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        self.ptr = self.buf.data_ptr() + MARGIN

    def read(self, dtype, shape):
        """the region as a numpy array, after asserting that both margins still hold the sentinel"""
        import torch
        torch.cuda.synchronize()
        h = self.buf.cpu().numpy()
        assert (h[:MARGIN] == SENTINEL).all() and (h[MARGIN + self.n:] == SENTINEL).all(), "a sentinel byte next to the output changed"
        return h[MARGIN:MARGIN + self.n].view(dtype).reshape(shape).copy()


# ---- a. tiles, every kernel form ---------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _case(name):
    """(hp, blob, tiles, float64 probabilities) of an arithmetic case: computed once, shared, never written to."""
    hp, blob, x = R.case_inputs(name)
    p64 = R.forward64(hp, blob, x)
    for a in (blob, x, p64):
        a.setflags(write=False)
    return hp, blob, x, p64


def _precisions(name):
    return ["f32", "f16x3"] + (["f16f6"] if TABLE[name]["tol_f6"] is not None else [])


TILE_CASES = [(n, p) for n in R.ARITH_CASES for p in _precisions(n)]
HP_F6_CASES = [n for n in R.ARITH_CASES if R.ARITH_CASES[n][0] == R.HP_F6 and TABLE[n]["tol_f6"] is not None]
SW = "v2_28_switches"


def _tile_calls(hp, blob, x, prec, max_batch=3, lanes=0):
    """5 tiles, tiles [0:2], the 5 tiles again on one engine: a ragged last batch (for the F6 form a half-empty tile pair) and a
    smaller call after a larger one."""
    with umx.Engine(hp, blob, max_batch=max_batch, precision=prec, lanes=lanes) as eng:
        if prec != "default":
            assert eng.precision == prec
        return {"five": eng.forward_tiles(x), "two": eng.forward_tiles(x[:2]), "again": eng.forward_tiles(x)}


def _check_tiles(name, prec, got, plain, p64=None):
    for fill, out in list(got.items()) + [(None, plain)]:
        assert out["five"].tobytes() == out["again"].tobytes(), (name, prec, fill, "the repeated call differs from the first")
    _all_same(got, plain, "%s %s" % (name, prec))
    if p64 is None:
        return
    tol = TABLE[name]["tol_f6" if prec == "f16f6" else "tol"]
    for fill, out in got.items():      # the guarded result itself, held to the float64 forward as tests/test_gpu_arith.py holds the plain one
        errs = np.abs(out["five"].astype(np.float64) - p64).reshape(5, -1).max(axis=1)
        print("%s %s UMX_DEBUG_GUARD=%s: E_gpu %.3g = %.3f x tol %.3g" % (name, prec, fill, errs.max(), errs.max() / tol, tol))
        assert np.all(errs <= tol), (name, prec, fill, errs.tolist(), tol)


@pytest.mark.parametrize("name,prec", TILE_CASES, ids=["%s-%s" % c for c in TILE_CASES])
def test_tiles_do_not_depend_on_the_fill(name, prec, monkeypatch):
    hp, blob, x, p64 = _case(name)
    assert x.shape[0] == 5
    got, plain = _under(monkeypatch, FILLS, lambda: _tile_calls(hp, blob, x, prec))
    _check_tiles(name, prec, got, plain, p64)


@pytest.mark.parametrize("name", HP_F6_CASES)
def test_f6_tile_pairs_of_one_batch_of_five(name, monkeypatch):
    """max_batch = 5 pairs the tiles (0 1)(2 3)(4 -): the last workgroup's second tile does not exist."""
    hp, blob, x, p64 = _case(name)
    got, plain = _under(monkeypatch, FILLS, lambda: _tile_calls(hp, blob, x, "f16f6", max_batch=5))
    _check_tiles(name, "f16f6", got, plain, p64)


@pytest.mark.parametrize("prec", _precisions(SW))
def test_two_lanes_under_guards(prec, monkeypatch):
    """lanes = 2: the batches alternate between two activation sets on two streams, both between red zones"""
    hp, blob, x, p64 = _case(SW)
    got, plain = _under(monkeypatch, FILLS, lambda: _tile_calls(hp, blob, x, prec, lanes=2))
    _check_tiles(SW, prec, got, plain, p64)


@pytest.mark.parametrize("prec", _precisions(SW))
def test_forward_tiles_dev_stays_inside_the_callers_region(prec, monkeypatch):
    """umx_forward_tiles_dev into a torch tensor with sentinel bytes on both sides of the region handed in"""
    import torch
    hp, blob, x, _ = _case(SW)
    n, P, K = x.shape[0], hp.imSize, hp.nClasses

    def body():
        tiles = torch.from_numpy(np.array(x)).cuda()
        out = _Margined(n * P * P * K * 4)
        torch.cuda.synchronize()
        with umx.Engine(hp, blob, max_batch=3, precision=prec) as eng:
            eng.forward_tiles_dev(tiles.data_ptr(), n, out.ptr)
            eng.synchronize()
            dev = out.read(np.float32, (n, P, P, K))
            host = eng.forward_tiles(x)
        assert dev.tobytes() == host.tobytes(), "the device entry differs from the host entry"
        return {"dev": dev}

    got, plain = _under(monkeypatch, FILLS, body)
    _all_same(got, plain, "forward_tiles_dev %s" % prec)


@pytest.mark.parametrize("env", SWITCHES, ids=lambda e: ",".join("%s=%s" % kv for kv in e.items()) or "default")
def test_planner_switches_under_guards(env, monkeypatch):
    """every environment switch of tests/test_gpu_switches.py: a forced plan, forced N-tiles, the activation shift, the precision"""
    hp, blob, x, _ = _case(SW)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    got, plain = _under(monkeypatch, ("0xff",), lambda: _tile_calls(hp, blob, x, "default"))
    _check_tiles(SW, str(env), got, plain)


# ---- b. workgroup order 2 ----------------------------------------------------------------------------------------------------

ORDER2_IMAGES = 278                # one batch: ceil(278 / 4) = 70 workgroup tiles on the 8 x 8-pixel layers
ORDER2_IMGS_PER_TILE = 4           # images one 16 x 16 M-tile of an 8 x 8-pixel layer holds


def test_workgroup_order_2_under_guards(monkeypatch):
    """The graph of test_workgroup_order_2_is_chosen_by_rule at 70 workgroup tiles in one batch; the profile must show order 2 on at
    least two launches, in the guarded run and in the plain one.

    The rule of run_launch_f16 reads WORKGROUP tiles, ceil(images / images per M-tile) x tiles per image, and this graph's layers of
    more than one N-block (160 and 320 output channels) are 8 x 8 and 4 x 4 pixels, the 8 x 8 ones 4 images to an M-tile.  The figure 70 --
    at least 64, no multiple of 8 (tiles_per_xcd = ceil(70 / 8) = 9: the last XCD range holds 7 tiles and 2 empty slots) -- therefore
    belongs to the tile count of the 8 x 8 layers, and the batch that gives it without being a multiple of the 4 images per M-tile is
    278 images (a last M-tile with 2 of its 4).  Seventy IMAGES would be 18 and 5 tiles there: measured, no launch takes order 2
    then, so a batch of 70 images cannot test the order at all; it runs here too, for its ragged M-tile, without a claim about the
    order."""
    n = ORDER2_IMAGES
    ntiles = -(-n // ORDER2_IMGS_PER_TILE)
    assert ntiles == 70 and ntiles >= 64 and ntiles % 8 != 0 and n % ORDER2_IMGS_PER_TILE != 0
    hp = model.HParams(model.GRAPH_V2, 32, 2, 3, 40, 3, 3, 0, 2)
    blob = model.random_blob(hp, seed=2)
    x = np.random.default_rng(1).normal(size=(n, 32, 32, 2)).astype(np.float32)

    def body():
        out = {}
        for m in (n, 70):
            with umx.Engine(hp, blob, max_batch=m) as eng:
                out["probs%d" % m] = eng.forward_tiles(x[:m])
                orders = _kernels_run(eng, x[:m], "xcd_order")
                again = eng.forward_tiles(x[:m])
            assert out["probs%d" % m].tobytes() == again.tobytes()
            if m == n:
                seen.append(orders)
        return out

    seen = []
    got, plain = _under(monkeypatch, ("0xff",), body)
    assert all(np.isfinite(v).all() for v in plain.values())
    _all_same(got, plain, "order 2")
    assert len(seen) == 2
    for orders in seen:
        print("%d images: launches in order 2: %s" % (n, sorted(k for k, o in orders.items() if o == 2)))
        assert sum(1 for o in orders.values() if o == 2) >= 2, orders


# ---- c. whole-image entries --------------------------------------------------------------------------------------------------

IMAGE_MODELS = ("v2_duo_like", "v2_solo_like", "legacy_k5")     # patch 32, margin 4, sub 24
MEAN, STD = 0.2, 0.2


def _shapes(hp):
    """the images of one sequence, in call order: grow() grows, keeps a larger buffer, grows again; the last repeats the first"""
    C = hp.nChannels
    first = (C, 70, 45) if C > 1 else (70, 45)
    return [("first", first, 1), ("tiny", (5, 7), 1), ("wide", (31, 200), C), ("again", first, 1)]


def _images(hp, kind):
    """name -> array per _shapes(hp): float64 in [0, 0.5), or uint8 / uint16 samples; "wide" is one plane in every channel"""
    out = []
    for i, (nm, shape, dup) in enumerate(_shapes(hp)):
        rng = np.random.default_rng([17, 0 if nm == "again" else i])
        if kind == "f64":
            a = rng.random(shape) * 0.5
        else:
            a = rng.integers(0, np.iinfo(kind).max + 1, size=shape).astype(kind)
        if dup > 1:
            a = np.ascontiguousarray(np.repeat(a[None], dup, axis=0))
        out.append((nm, a))
    return out


def _range_of(raw):
    planes = raw if raw.ndim == 3 else raw[None]
    return [(int(p.min()), int(p.max())) for p in planes]


def _entry_image(eng, hp):
    out = {}
    for stitch in (umx.STITCH_FP16_COMPAT, umx.STITCH_FP32):
        for mode in (umx.MODE_ACCUMULATE, umx.MODE_REPLACE):
            for nm, img in _images(hp, "f64"):
                out["%s.s%d.m%d" % (nm, stitch, mode)] = eng.infer_image(img, MEAN, STD, mode=mode, stitch=stitch)
    return out


def _entry_raw(eng, hp):
    out = {}
    for dt in (np.uint8, np.uint16):
        for how in ("off", "on", "range"):
            for nm, raw in _images(hp, dt):
                out["%s.%s.%s" % (nm, np.dtype(dt).name, how)] = eng.infer_image_raw(
                    raw, how != "off", MEAN, STD, value_range=_range_of(raw) if how == "range" else None)
    return out


def _entry_scaled(eng, hp):
    """the resize, percentile and range kernels inside the image entries"""
    out = {}
    for nm, raw in _images(hp, np.uint16):
        out[nm + ".scaled"] = eng.infer_image_raw_scaled(raw, 0.5, True, MEAN, STD)
        out[nm + ".outlier"] = eng.infer_image_raw_outlier(raw, 0.5, 99.0, MEAN, STD)
    for nm, raw in _images(hp, np.uint8):
        out[nm + ".outlier1"] = eng.infer_image_raw_outlier(raw, 1.0, 97.5, MEAN, STD)      # scaling 1: the percentile alone
    return out


def _entry_flight(eng, hp):
    """two slides in flight on slots 0 and 1, then both waits; then the slots swapped and without the rescale; then the first pair"""
    imgs = dict(_images(hp, np.uint16))
    K = hp.nClasses
    out = {}
    for rnd, (names, rescale) in enumerate(((("first", "wide"), True), (("wide", "first"), False), (("again", "wide"), True))):
        raws = [imgs[n] if imgs[n].ndim == 3 else imgs[n][None] for n in names]
        outs = [np.zeros((K,) + r.shape[1:], np.uint8) for r in raws]
        for slot in (0, 1):
            r = raws[slot]
            eng.infer_image_raw_submit(slot, r.ctypes.data, 16, r.shape[0], r.shape[1], r.shape[2], rescale, MEAN, STD, outs[slot].ctypes.data)
        eng.infer_image_wait(0)
        eng.infer_image_wait(1)
        for slot in (0, 1):
            out["round%d.slot%d.%s" % (rnd, slot, names[slot])] = outs[slot]
    assert out["round0.slot0.first"].tobytes() == out["round2.slot0.again"].tobytes()
    assert out["round0.slot1.wide"].tobytes() == out["round2.slot1.wide"].tobytes()
    return out


def _entry_dev(eng, hp):
    """umx_infer_image_dev into a device region with sentinel bytes on both sides"""
    import torch
    K = hp.nClasses
    out = {}
    for stitch, dt in ((umx.STITCH_FP16_COMPAT, np.float16), (umx.STITCH_FP32, np.float32)):
        for nm, img in _images(hp, "f64"):
            img = img if img.ndim == 3 else img[None]
            C, H, W = img.shape
            d_img = torch.from_numpy(img).cuda()
            region = _Margined(K * H * W * np.dtype(dt).itemsize)
            torch.cuda.synchronize()
            eng.infer_image_dev(d_img.data_ptr(), C, H, W, MEAN, STD, umx.MODE_ACCUMULATE, stitch, region.ptr)
            eng.synchronize()
            out["%s.s%d" % (nm, stitch)] = region.read(dt, (K, H, W))
    return out


ENTRIES = {"image": _entry_image, "raw": _entry_raw, "scaled": _entry_scaled, "flight": _entry_flight, "dev": _entry_dev}


@pytest.mark.parametrize("entry", list(ENTRIES))
@pytest.mark.parametrize("max_batch", [2, 32], ids=["slabs", "one-stream"])
@pytest.mark.parametrize("name", IMAGE_MODELS)
def test_image_entries_do_not_depend_on_the_fill(name, max_batch, entry, monkeypatch):
    """max_batch = 2: several slabs, so the copy streams and their events; 32: one in-order stream.  Four images on one engine."""
    hp = helpers.small_hps()[name]
    blob = model.random_blob(hp, seed=4)

    def body():
        with umx.Engine(hp, blob, max_batch=max_batch) as eng:
            out = ENTRIES[entry](eng, hp)
        for k in [k for k in out if k.startswith("first.")]:
            assert out[k].tobytes() == out["again." + k[6:]].tobytes(), (k, "the repeated image differs from the first")
        return out

    got, plain = _under(monkeypatch, FILLS, body)
    _all_same(got, plain, "%s max_batch %d %s" % (name, max_batch, entry))


# ---- d. sharded entries ------------------------------------------------------------------------------------------------------

WORLD = 3
SH_H, SH_W = 24 * 5 - 7, 61                  # 5 patch rows over 3 ranks: bands of 2 / 2 / 1


@functools.lru_cache(maxsize=None)
def _sharded_reference():
    """the plain one-GPU results (call with UMX_DEBUG_GUARD unset)"""
    assert "UMX_DEBUG_GUARD" not in os.environ
    hp = helpers.small_hps()["v2_duo_like"]
    blob = model.random_blob(hp, seed=4)
    img = np.random.default_rng(8).random((2, SH_H, SH_W)) * 0.5
    raw = (np.random.default_rng(9).random((2, SH_H, SH_W)) * 50000).astype(np.uint16)
    raw2 = np.ascontiguousarray(raw[:, ::-1])
    rng = _range_of(raw)
    with umx.Engine(hp, blob, max_batch=8) as eng:
        want = {s: eng.infer_image(img, MEAN, STD, stitch=s) for s in (umx.STITCH_FP16_COMPAT, umx.STITCH_FP32)}
        want_raw = eng.infer_image_raw(raw, True, MEAN, STD, value_range=rng)
        want_raw2 = eng.infer_image_raw(raw2, True, MEAN, STD, value_range=rng)
        assert eng.tile_grid(SH_H, SH_W)[0] == 5
    return hp, blob, img, raw, raw2, rng, want, want_raw, want_raw2


@pytest.mark.parametrize("fill", ["0xff", "0x7f"])
@pytest.mark.parametrize("nslabs", [1, 2])
def test_sharded_entries_under_guards(nslabs, fill, monkeypatch):
    """A world of three on one GPU (tests/test_gpu_world8.py's thread transport), every rank's engine created under the guard: the
    device entry at both stitch types, the raw entry synchronously and with two slides in flight -- every rank's gathered stack and
    own rows equal the plain one-GPU result byte for byte."""
    import torch
    monkeypatch.delenv("UMX_DEBUG_GUARD", raising=False)
    hp, blob, img, raw, raw2, rng, want, want_raw, want_raw2 = _sharded_reference()
    K, H, W = hp.nClasses, SH_H, SH_W
    tw = ThreadWorld(WORLD)
    monkeypatch.setenv("UMX_DEBUG_GUARD", fill)

    def body(rank):
        torch.cuda.set_device(0)
        ok = {}
        with umx.Engine(hp, blob, max_batch=8) as eng:
            eng.shard_init_transport(rank=rank, world=WORLD, **tw.transport(rank))
            pl = eng.shard_plan(H, W, rank, WORLD, nslabs)
            r0, r1, o0, o1 = pl["need_row0"], pl["need_row1"], pl["own_row0"], pl["own_row1"]
            for stitch, tdt, bits in ((umx.STITCH_FP16_COMPAT, torch.float16, np.uint16), (umx.STITCH_FP32, torch.float32, np.uint32)):
                band = torch.from_numpy(np.ascontiguousarray(img[:, r0:max(r1, r0 + 1)])).cuda()
                full = torch.empty((K, H, W), dtype=tdt, device="cuda")
                torch.cuda.synchronize()
                eng.infer_image_sharded_dev(band.data_ptr(), 2, H, W, r0, band.shape[1], MEAN, STD, umx.MODE_ACCUMULATE, stitch, nslabs,
                                            full.data_ptr())
                eng.synchronize()
                torch.cuda.synchronize()
                ok["dev.s%d" % stitch] = np.array_equal(full.cpu().numpy().view(bits), want[stitch].view(bits))
            b1, b2 = np.ascontiguousarray(raw[:, r0:r1]), np.ascontiguousarray(raw2[:, r0:r1])
            full = torch.zeros((K, H, W), dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            own = eng.infer_image_sharded_raw(b1, H, W, r0, rng, MEAN, STD, nslabs=nslabs, own_rows=o1 - o0, out_full_ptr=full.data_ptr())
            torch.cuda.synchronize()
            ok["raw"] = np.array_equal(full.cpu().numpy(), want_raw) and np.array_equal(own, want_raw[:, o0:o1])
            fulls = [torch.zeros((K, H, W), dtype=torch.uint8, device="cuda") for _ in range(2)]
            owns = [np.zeros((K, o1 - o0, W), np.uint8) for _ in range(2)]
            torch.cuda.synchronize()
            for slot, b in ((0, b1), (1, b2)):                                               # two slides in flight
                eng.infer_image_sharded_raw_submit(slot, b.ctypes.data, 16, 2, H, W, r0, b.shape[1], rng, MEAN, STD, umx.MODE_ACCUMULATE,
                                                   nslabs, owns[slot].ctypes.data, fulls[slot].data_ptr())
            eng.infer_image_wait(0)
            eng.infer_image_wait(1)
            torch.cuda.synchronize()
            ok["flight"] = (np.array_equal(fulls[0].cpu().numpy(), want_raw) and np.array_equal(fulls[1].cpu().numpy(), want_raw2)
                            and np.array_equal(owns[0], want_raw[:, o0:o1]) and np.array_equal(owns[1], want_raw2[:, o0:o1]))
        return (pl["patch_row0"], pl["patch_row1"]), ok

    try:
        res = _run_ranks(WORLD, body)
    finally:
        monkeypatch.delenv("UMX_DEBUG_GUARD", raising=False)
    assert [b - a for (a, b), _ in res] == [2, 2, 1]
    assert all(all(ok.values()) for _, ok in res), res


# ---- e. the mode itself ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,prec", [("v2_duo_like", "default"), ("v2_duo_like", "f32"), ("legacy_k5", "default")])
def test_guard_mode_covers_every_buffer(name, prec, monkeypatch, capfd):
    """On when asked, and only then: one line per created context (the cascade of the default precision included), counting at
    least the plan's activation buffers and one uploaded tensor per launch."""
    hp = helpers.small_hps()[name]
    blob = model.random_blob(hp, seed=4)
    g = umx.describe_graph(hp)
    least = len(g["buffers"]) + len(g["launches"])
    for fill in (None, "0x7f"):
        if fill is None:
            monkeypatch.delenv("UMX_DEBUG_GUARD", raising=False)
        else:
            monkeypatch.setenv("UMX_DEBUG_GUARD", fill)
        capfd.readouterr()
        with umx.Engine(hp, blob, max_batch=2, precision=prec):
            pass
        with umx.Engine(hp, blob, max_batch=2, precision=prec, lanes=2):
            pass
        err = capfd.readouterr().err
        lines = [ln for ln in err.splitlines() if "UMX_DEBUG_GUARD" in ln]
        if fill is None:
            assert lines == []
            continue
        assert len(lines) == 2, err
        counts = []
        for ln in lines:
            assert ln.startswith("[umx] UMX_DEBUG_GUARD=0x7f: ") and ln.endswith(" engine buffers between red zones"), ln
            counts.append(int(ln.split(": ")[1].split()[0]))
        assert counts[0] >= least, (counts, least)
        assert counts[1] >= counts[0] + len(g["buffers"]), counts          # the second lane's activation set
    monkeypatch.delenv("UMX_DEBUG_GUARD", raising=False)


def test_a_bad_fill_is_refused(monkeypatch):
    hp = helpers.small_hps()["v2_duo_like"]
    monkeypatch.setenv("UMX_DEBUG_GUARD", "0x100")
    for prec in ("default", "f32", "f16x3"):
        with pytest.raises(umx.UmxError) as e:
            umx.Engine(hp, model.random_blob(hp), max_batch=2, precision=prec)
        assert e.value.code == umx.ERR_INVALID and "UMX_DEBUG_GUARD" in str(e.value)


def image_kernel_digest():
    """The smallest cases of tests/test_gpu_imagekernels.py through the umx_test_*_dev entries (their scratch is a call-local arena:
    red zones round it, poison inside, checked before it is freed) -> one digest of every output byte."""
    import resize_ref
    from test_gpu_imagekernels import value_plane
    h = hashlib.sha256()
    for shape in ((2, 2, 5, 5), (1, 17, 1, 5), (3, 40, 1, 13), (9, 9, 3, 14)):
        H, W, hh, ww = shape
        for a in umx.resize_dev(resize_ref.plane("uniform", H, W), hh, ww):
            h.update(np.ascontiguousarray(a).tobytes())
    for n in (1, 2, 3, 101, 257):
        for q in (-1.0, 0.0, 50.0, 99.9):
            for a in umx.rescale_dev(value_plane("levels", n), q):
                h.update(np.ascontiguousarray(a).tobytes())
    for dt in (np.uint8, np.uint16):
        planes = [np.random.default_rng(n).integers(1, 200, n).astype(dt) for n in (1, 2, 15, 16, 17, 40)]
        for off in (0, 1, 13):
            for nslabs in (1, 3):
                h.update(umx.plane_range_dev(planes, [off] * len(planes), [nslabs] * len(planes)).tobytes())
    for a in umx.half_to_u8_dev(np.arange(0x3C00 + 1, dtype=np.uint16).view(np.float16)):
        h.update(np.ascontiguousarray(a).tobytes())
    h.update(umx.double_to_half_dev(np.linspace(-2.0, 2.0, 1001)).tobytes())
    return h.hexdigest()


_CHILD = """
import sys
sys.path.insert(0, %r); sys.path.insert(0, %r)
import test_gpu_infer_guard as T
print("digest", T.image_kernel_digest())      # (UmxError 7 from an entry when a red zone was written)
"""


def test_image_kernel_entries_under_guards(monkeypatch):
    """UMX_DEBUG_GUARD=0xff in a child process, as the labeler's guard test runs: the bytes of the plain run in this process"""
    monkeypatch.delenv("UMX_DEBUG_GUARD", raising=False)
    want = image_kernel_digest()
    env = dict(os.environ, UMX_DEBUG_GUARD="0xff")
    r = subprocess.run([sys.executable, "-c", _CHILD % (helpers.ROOT, os.path.join(helpers.ROOT, "tests"))], env=env, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "digest " + want in r.stdout, (r.stdout[-500:], want)
