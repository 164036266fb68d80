"""CPU checks of the label mask's growth: the inputs of tests/label_grow_ref.py have the
properties they are named for, the consequences the definition promises hold on the restatement, umx_label_options_check accepts and
refuses the two growth words as the header says, and the drivers refuse the flag combinations.  No kernel runs here:
tests/test_gpu_label_grow.py holds the device to the restatement."""
import ctypes
import functools
import os
import re

import numpy as np
import pytest
from scipy import ndimage

import helpers
import label_grow_ref as ref
import label_ref
from unmicst_amd import build, driver, model, umx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAIN = (150, 203)
T, HALO = umx.LABEL_GROW_TILE, umx.LABEL_GROW_HALO
RADII = (1, 2, HALO - 1, HALO, HALO + 1, 2 * HALO, 2 * HALO + 1)


@pytest.fixture(scope="module")
def lib():
    build.build()
    return umx.load()


@functools.lru_cache(maxsize=None)
def seeds_of(name, shape=MAIN):
    """(planes, pred, labels0, N, cls, min_area, classes)"""
    planes, cls, min_area, classes = ref.case(shape[0], shape[1], name, T, HALO)
    labels0, table0 = label_ref.label(planes, cls, min_area)
    pred = ref.pred_of(planes)
    for a in (planes, pred, labels0):
        a.setflags(write=False)
    return planes, pred, labels0, len(table0), cls, min_area, classes


def grown(name, R, shape=MAIN):
    _, pred, labels0, _, _, _, classes = seeds_of(name, shape)
    return ref.grow(labels0, pred, classes, R)


def test_rings_hold_several_seeds_in_one_body():
    bodies, nuclei = ref.ring_bodies(*MAIN)
    body, n_bodies = ndimage.label(bodies)
    _, pred, labels0, N, _, _, _ = seeds_of("rings")
    assert np.array_equal(pred == 2, nuclei) and np.array_equal(pred == 1, bodies & ~nuclei)
    per_body = [len(np.unique(labels0[(body == b) & (labels0 > 0)])) for b in range(1, n_bodies + 1)]
    assert (N, n_bodies, sum(n > 1 for n in per_body)) == (154, 75, 29)      # some body holds two seeds: fronts meet inside a rim
    assert (grown("rings", 1) > 0).sum() > (labels0 > 0).sum()
    assert np.array_equal(grown("rings", 16), grown("rings", 40))             # saturated by 16: long radii need the corridor
    assert not np.array_equal(grown("rings", HALO), grown("rings", HALO + 1))   # but still growing past one launch's levels


def test_corridor_claims_one_pixel_per_level_across_the_tile_boundary():
    p = ref.path(MAIN[0], MAIN[1], T)
    length = len(p) - 1
    assert length > 255 > 2 * HALO + 3
    stretch = p[:3 * (2 * HALO + 3)]
    crossings = sum((a[1] < T) != (b[1] < T) for a, b in zip(stretch, stretch[1:]))
    assert crossings >= len(stretch) // 3                      # every third step of the stretch crosses x = T
    _, pred, labels0, N, _, _, _ = seeds_of("corridor")
    assert N == 1 and (labels0 > 0).sum() == 1 and labels0[p[0]] == 1 and ((pred == 1).sum(), (pred == 2).sum()) == (length, 1)
    for R in RADII + (255, 300, length, length + 5):
        g = grown("corridor", R)
        assert (g > 0).sum() == 1 + min(R, length)
        assert all(g[q] == 1 for q in p[:1 + min(R, length)])
    assert not np.array_equal(grown("corridor", HALO), grown("corridor", HALO + 1))      # the level after a launch's last one
    for shape, n in (((1, 130), 129), ((130, 1), 129), ((1, 1), 0)):
        assert len(ref.path(shape[0], shape[1], T)) - 1 == n
        assert (grown("corridor", 255, shape) > 0).sum() == 1 + n


@pytest.mark.parametrize("name,length", [("duel_odd", 2 * HALO + 1), ("duel_even", 2 * HALO + 2)])
def test_duel_fronts_meet_in_the_middle(name, length):
    p = ref.path(MAIN[0], MAIN[1], T)[:length + 2]
    _, pred, labels0, N, _, _, _ = seeds_of(name)
    assert N == 2 and labels0[p[0]] == 1 and labels0[p[-1]] == 2 and (pred == 1).sum() == length
    meet = -(-length // 2)
    assert meet == HALO + 1                                    # the level after the first launch's last
    assert (grown(name, meet - 1) == 0)[pred == 1].sum() == length - 2 * (meet - 1) > 0
    g = grown(name, meet)
    assert (g > 0).sum() == length + 2 and np.array_equal(g, grown(name, 2 * HALO + 1))
    got = [int(g[q]) for q in p]
    ones = 1 + (length + 1) // 2                               # with an odd length the middle pixel goes to the smaller label
    assert got == [1] * ones + [2] * (length + 2 - ones)


def test_tie_goes_to_the_smaller_label_wherever_it_lies():
    pred, where = ref.tie(*MAIN)
    _, _, labels0, N, _, _, _ = seeds_of("tie")
    assert sorted(where) == ["above", "below", "left", "right"] and N == 8 and (pred == 1).sum() == 4
    g = grown("tie", 1)
    assert np.array_equal(g, grown("tie", 5))
    step = {"above": (-1, 0), "below": (1, 0), "left": (0, -1), "right": (0, 1)}
    for name, (y, x) in where.items():
        dy, dx = step[name]
        small, large = labels0[y + dy, x + dx], labels0[y - dy, x - dx]
        assert 0 < small < large and g[y, x] == small, name
    assert len(ref.tie(1, 130)[1]) == 1 and len(ref.tie(130, 1)[1]) == 0


def test_dropped_nuclei_are_claimed_when_the_label_class_grows_too():
    planes, pred, labels0, N, cls, min_area, classes = seeds_of("cls_in_G")
    assert cls in classes and min_area > 1
    all_seeds = label_ref.label(planes, cls, 1)[0]
    dropped = (all_seeds > 0) & (labels0 == 0)
    assert 0 < N < all_seeds.max() and dropped.sum() > 0
    g = grown("cls_in_G", 2 * HALO + 1)
    assert (g[dropped] > 0).sum() > 0 and g.max() == N
    only_rims = ref.grow(labels0, pred, (1,), 2 * HALO + 1)
    assert (only_rims[dropped] == 0).all() and (only_rims > 0).sum() < (g > 0).sum()


def test_far_domain_stays_empty():
    _, pred, labels0, N, _, _, classes = seeds_of("far")
    domain, n_dom = ndimage.label((pred == 1) | (labels0 > 0))
    seedless = [c for c in range(1, n_dom + 1) if not (labels0[domain == c] > 0).any()]
    assert N > 0 and len(seedless) > 5
    g = grown("far", 255)
    assert all((g[domain == c] == 0).all() for c in seedless)
    beyond = tuple(np.array(ref.path(MAIN[0], MAIN[1], T)[2 * HALO + 2:]).T)        # the corridor past level 2 * HALO + 1: no seed within R
    assert len(beyond[0]) > 0 and (grown("corridor", 2 * HALO + 1)[beyond] == 0).all()


@pytest.mark.parametrize("name", ["empty", "full"])
def test_nothing_grows_without_a_seed(name):
    _, pred, labels0, N, _, _, classes = seeds_of(name)
    assert N == 0 and ((pred == 1).all() if name == "full" else (pred == 0).all())
    planes = seeds_of(name)[0]
    labels, table = ref.label_grow(planes, 2, 1, 2 * HALO + 1, classes)
    assert len(table) == 0 and not labels.any()


@pytest.mark.parametrize("name", ["rings", "corridor", "cls_in_G", "far"])
def test_consequences_of_the_definition(name):
    planes, pred, labels0, N, cls, min_area, classes = seeds_of(name)
    for R in (1, 2, 3, HALO, HALO + 1, 2 * HALO + 1, 40):
        g = grown(name, R)
        assert g.dtype == np.int32 and g.max() == N == len(np.unique(g[g > 0]))            # N does not change
        assert np.array_equal(g[labels0 > 0], labels0[labels0 > 0])                         # every object contains its seed, numbered as before
        assert ((g > 0) <= ((labels0 > 0) | np.isin(pred, classes))).all()                  # and grows nowhere but over the domain
        assert ref.connected(g, N)
        assert np.array_equal(g, ref.nearest_seed(labels0, pred, classes, R))               # nearest seed through the domain, ties to the smaller
        labels, table = ref.label_grow(planes, cls, min_area, R, classes)
        assert np.array_equal(labels, g)
        for l in range(1, N + 1, max(1, N // 7)):                                           # the table, against the plain definition
            ys, xs = np.nonzero(g == l)
            t = table[l - 1]
            assert (t["area"], t["y0"], t["x0"], t["y1"], t["x1"], t["reserved"], t["sum_y"], t["sum_x"]) == \
                (len(ys), ys.min(), xs.min(), ys.max(), xs.max(), 0, ys.sum(), xs.sum())
        assert len(table) == N
    for r1, r2 in ((1, 1), (1, 2), (2, 1), (HALO, 1), (HALO, HALO), (3, 13), (HALO + 1, HALO), (16, 24)):
        assert np.array_equal(ref.grow(grown(name, r1), pred, classes, r2), grown(name, r1 + r2)), (r1, r2)


def test_binding_mirrors_the_header(lib):
    header = open(os.path.join(ROOT, "include", "umx.h")).read()
    enum = dict(re.findall(r"(UMX_LABEL_\w+) = (\d+)", header))
    assert {k: int(v) for k, v in enum.items()} == {"UMX_LABEL_MAX_GROW": umx.LABEL_MAX_GROW, "UMX_LABEL_GROW_TILE": umx.LABEL_GROW_TILE,
                                                    "UMX_LABEL_GROW_HALO": umx.LABEL_GROW_HALO}
    assert umx.LABEL_MAX_GROW == 255 and 1 <= umx.LABEL_GROW_HALO <= umx.LABEL_GROW_TILE
    assert ctypes.sizeof(umx._LabelOptions) == 32
    o = umx._LabelOptions(2, 1)
    assert bytes(o) == bytes(np.array([2, 1, 0, 0, 0, 0, 0, 0], "<i4"))                    # no growth: the bytes of before
    o.grow_radius, o.grow_classes = 3, 0x80000002
    assert list(o.reserved) == [3, -0x7ffffffe, 0, 0, 0, 0]                                # the six words by index, as before
    o.reserved[5] = 7
    assert bytes(o) == bytes(np.array([2, 1, 3, -0x7ffffffe, 0, 0, 0, 7], "<i4"))
    assert (umx._LabelOptions.cls.offset, umx._LabelOptions.min_area.offset, umx._LabelOptions.grow_radius.offset,
            umx._LabelOptions.grow_classes.offset, umx._LabelOptions.reserved.offset) == (0, 4, 8, 12, 8)


def test_options_check_accepts_and_refuses_the_growth_words(lib):
    ok = umx.label_options_check
    assert ok(3, 150, 203, 2, 1) == "" and ok(3, 150, 203, 2, 1, grow=0, grow_classes=()) == ""
    assert ok(3, 5, 5, 2, 1, grow=1, grow_classes=(1,)) == "" and ok(3, 5, 5, 2, 1, grow=255, grow_classes=(0, 1, 2)) == ""
    assert ok(3, 5, 5, 2, 1, grow=3) == ""                                                 # the default set: class 1
    assert ok(16, 5, 5, 15, 1, grow=8, grow_classes=range(16)) == "" and ok(1, 5, 5, 0, 1, grow=8, grow_classes=(0,)) == ""
    for r in (-1, 256, 2 ** 31 - 1, -2 ** 31):
        assert "grow_radius" in ok(3, 5, 5, 2, 1, grow=r, grow_classes=(1,)), r
    assert "grow_classes" in ok(3, 5, 5, 2, 1, grow=2, grow_classes=()) and "empty" in ok(3, 5, 5, 2, 1, grow=2, grow_classes=())
    assert "grow_classes" in ok(2, 5, 5, 1, 1, grow=2)                                      # two classes: the default set is empty
    for k in (3, 4, 15, 31):
        assert "grow_classes" in ok(3, 5, 5, 2, 1, grow=2, grow_classes=(1, k)), k
    assert "grow_classes" in ok(16, 5, 5, 2, 1, grow=2, grow_classes=(16,))
    msg = ok(3, 5, 5, 2, 1, grow=0, grow_classes=(1,))
    assert "grow_classes" in msg and "grow_radius is 0" in msg
    with pytest.raises(ValueError):
        ok(3, 5, 5, 2, 1, grow=2, grow_classes=(32,))
    for j in range(6):                                                                      # the refusal of before, word by word
        assert "reserved" in ok(3, 5, 5, 2, 1, reserved=[0] * j + [1])
    for j in range(2, 6):                                                                   # the four words that remain reserved
        assert ok(3, 5, 5, 2, 1, reserved=[0] * j + [1], grow=2, grow_classes=(1,)) == "reserved must be zero"
    assert "cls" in ok(3, 5, 5, 3, 1, grow=2, grow_classes=(1,)) and "min_area" in ok(3, 5, 5, 2, 0, grow=2, grow_classes=(1,))


def test_driver_refuses_bad_growth_flags_before_any_engine(tmp_path, monkeypatch, capsys):
    hp, blob, mean, std = helpers.load_nuclei_dapi()
    models = tmp_path / "models"
    model.save_converted(model.ModelArtefacts(hp, blob, mean, std), str(models / "nucleiDAPI"))
    monkeypatch.setenv("UMX_MODELS_DIR", str(models))

    def no_engine(*a, **k):
        raise AssertionError("the engine was set up before the label flags were checked")
    monkeypatch.setattr(umx, "Engine", no_engine)
    img = str(tmp_path / "x" / "registration" / "missing.tif")   # never read: the refusal comes first
    lm = ["--labelMask"]
    for tool in driver.TOOLS:
        for flags, word in ((["--labelGrow", "3"], "--labelGrow needs --labelMask"),
                            (["--labelGrowClasses", "1"], "--labelGrowClasses needs --labelMask"),
                            (lm + ["--labelGrowClasses", "1"], "--labelGrowClasses needs --labelGrow"),
                            (lm + ["--labelGrow", "0"], "1..255"), (lm + ["--labelGrow", "256"], "1..255"), (lm + ["--labelGrow", "-2"], "1..255"),
                            (lm + ["--labelGrow", "3", "--labelGrowClasses", "1", "-1"], "from 0"),
                            (lm + ["--labelGrow", "3", "--labelGrowClasses", "1", "3"], "classes 0..2"),
                            (lm + ["--labelGrow", "3", "--labelGrowClasses"], "expected at least one argument")):
            with pytest.raises(SystemExit) as e:
                driver.run(tool, [img, "--model", "nucleiDAPI"] + flags)
            assert e.value.code == 2
            assert word in capsys.readouterr().err, (tool, flags)


def test_default_growth_classes_of_the_driver():
    import argparse
    parser = argparse.ArgumentParser()
    ns = argparse.Namespace
    f = driver.label_grow_classes
    assert f(parser, ns(labelGrow=None, labelGrowClasses=None, labelClass=None), 3) is None
    assert f(parser, ns(labelGrow=3, labelGrowClasses=None, labelClass=None), 3) == [1]
    assert f(parser, ns(labelGrow=3, labelGrowClasses=None, labelClass=1), 4) == [2, 3]
    assert f(parser, ns(labelGrow=3, labelGrowClasses=[2, 0, 2], labelClass=None), 3) == [0, 2]
    with pytest.raises(SystemExit) as e:                          # a two-class model: nothing is left
        f(parser, ns(labelGrow=3, labelGrowClasses=None, labelClass=None), 2)
    assert e.value.code == 2
    assert f(parser, ns(labelGrow=3, labelGrowClasses=[0], labelClass=None), 2) == [0]


def test_bench_tool_rims():
    """tools/bench_label.py --grow: the discs become cores with a rim of the contour class around them"""
    import importlib.util
    spec = importlib.util.spec_from_file_location("bench_label", os.path.join(ROOT, "tools", "bench_label.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    core, rim = m.blob_mask(150, 203), m.blob_mask(150, 203, rim=3)
    assert np.array_equal(core, m.blob_mask(150, 203, rim=0)) and (core <= rim).all() and rim.sum() > core.sum()
    planes = m.planes_of(core, rim)
    pred = ref.pred_of(planes)
    assert np.array_equal(pred == 2, core) and np.array_equal(pred == 1, rim & ~core) and np.array_equal(m.planes_of(core), m.planes_of(core, None))
