"""The host plan of the trainer's forward / input-gradient convolutions (tconv_plan, umx_tconv.hip) through umx_test_train_plan: no
device needed.  Every convolution of the shipped hyper-parameter sets and of synthetic-256 at batch 8 and 16, of the shapes of
tests/train_parity.py::tight_cases() at their own batch and of the legacy shapes of tests/test_gpu_train_legacy.py, each on the default
route, the UMX_TRAIN_CONV_F32 route and the UMX_TRAIN_NO_KSPLIT route, against tests/golden/tconv_plan_lines.json: the lines recorded
from setup_conv / setup_hconv as they stood before planning and upload were separated (a copy of that commit with a recording entry
added and its device allocator swapped for host memory, run on a CPU).

A line is the convolution's UMX_DEBUG_PLAN text, its groups (channels x taps per phase @ channel offset / master dims), the fused
activation, `direct`, the weight shift, the numbers of pack descriptors and weight references, the K-split scratch floats and a 64-bit
FNV-1a digest of everything the upload sends (tconv_digest).  The golden file holds one entry per convolution, keyed by what the build
says about it -- "b<batch> <name>: <shape>; groups <groups>, act <act>, wsh <shift on the first route>" -- with what the planner decided on the three routes, in the
order of ROUTES: the rest of the line, shortened to "NT <NT>x<blocks> k<k-steps> wg<workgroups> ks<K split>" (fp32 kernel: "fp32 NT <NT>
img <images a group> wg ks") and "d<direct> w<shift> p<packs> r<references> s<scratch> <digest>", and "="
where UMX_TRAIN_NO_KSPLIT changes nothing.  The digest covers no parameter offset, so the same convolution of two sets is one entry."""
import json
import os
import re

import pytest

import helpers
import train_parity
from unmicst_amd import model, umx

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tconv_plan_lines.json")
ROUTES = (("f16x3", False, False), ("conv_f32", True, False), ("no_ksplit", False, True))
# tests/test_gpu_train_legacy.py: SMALL and ODD (HParams(GRAPH_LEGACY, imSize, nChannels, nClasses, nOut0, nLayers, ks, nExtraConvs), batch)
LEGACY_SMALL = [("legacy_k5", 3), ("legacy_k3_x0", 4), ("legacy_k3_x2", 4)]
LEGACY_ODD = [((16, 1, 2, 4, 1, 3, 0), 1), ((16, 3, 4, 5, 2, 3, 1), 3), ((64, 1, 3, 4, 5, 3, 0), 2), ((16, 1, 3, 4, 2, 5, 2), 2),
              ((128, 1, 3, 4, 2, 3, 1), 1)]


def sets():
    """(hp, batch, blob seed) of every trainer whose plan is checked"""
    out = [(hp, B, 21) for hp in model.KNOWN_HP.values() for B in (8, 16)]
    out += [(c[0], c[1], c[3]) for c in train_parity.tight_cases().values()]
    small = helpers.small_hps()
    out += [(small[name], B, 17) for name, B in LEGACY_SMALL]
    out += [(model.HParams(model.GRAPH_LEGACY, *a), B, 17) for a, B in LEGACY_ODD]
    return out


_LINE = re.compile(r"^(.+?): (fp32 conv, )?(\d+ x \d+ -> \d+ ch, \d+ phase\(s\)), (.*); (groups \S+, act \d), "
                   r"direct (\d), wsh (-?\d+), packs (\d+), refs (\d+), scratch (\d+), digest ([0-9a-f]{16})$")


_F16 = re.compile(r"^NT (\d+) x (\d+) blocks, (\d+) k-steps, (\d+) workgroups, K split (\d+)$")
_F32 = re.compile(r"^NT (\d+), (\d+) img/group, (\d+) workgroups, K split (\d+)$")


def _short(f32, decided):
    """the middle of a line, shortened: NT, blocks, k-steps (fp32 kernel: NT, images a group), workgroups, K split"""
    if f32:
        return "fp32 NT %s img %s wg%s ks%s" % _F32.match(decided).groups()
    return "NT %sx%s k%s wg%s ks%s" % _F16.match(decided).groups()


def plan_lines():
    """key -> [decisions on each route of ROUTES]; two sets that share a key must share its decisions"""
    out = {}
    blobs = {}
    for hp, B, seed in sets():
        if (hp, seed) not in blobs:
            blobs[(hp, seed)] = model.random_blob(hp, seed=seed)
        plans = [umx.train_plan(hp, B, blobs[(hp, seed)], conv_f32=conv_f32, no_ksplit=no_ksplit) for _, conv_f32, no_ksplit in ROUTES]
        assert len(set(len(p) for p in plans)) == 1
        for per_route in zip(*plans):   # one convolution, in build order on every route
            keys, vals, wshs = set(), [], []
            for ln in per_route:
                name, f32, shape, decided, groups, direct, wsh, packs, refs, scratch, digest = _LINE.match(ln).groups()
                keys.add("b%d %s: %s; %s" % (B, name, shape, groups))
                wshs.append(wsh)
                vals.append("%s; d%s w%s p%s r%s s%s %s" % (_short(f32, decided), direct, wsh, packs, refs, scratch, digest))
            assert len(keys) == 1, per_route
            if vals[2] == vals[0]:
                vals[2] = "="
            key = "%s, wsh %s" % (keys.pop(), wshs[0])   # (the shift follows the set's weights)
            assert out.setdefault(key, vals) == vals, key
    return out


@pytest.fixture(scope="module")
def lines():
    return plan_lines()


def test_plans_are_the_recorded_ones(lines):
    with open(GOLDEN) as f:
        want = json.load(f)
    assert sorted(lines) == sorted(want)
    wrong = {k: (lines[k], want[k]) for k in want if lines[k] != want[k]}
    assert not wrong, list(wrong.items())[:5]


_HCONV = re.compile(r"^NT \d+x\d+ k\d+ wg\d+ ks(\d+); d(\d) ")
_FCONV = re.compile(r"^fp32 NT \d+ img (\d+) wg\d+ ks(\d+); d0 ")
_KEY = re.compile(r"^b(\d+) .+: \d+ x \d+ -> \d+ ch, (\d+) phase\(s\); groups (\S+), act \d, wsh -?\d+$")


def test_the_cases_reach_every_convolution_form(lines):
    """The forms tests/test_gpu_train_tight.py::test_the_cases_reach_the_launch_forms requires of the convolutions on the device, on
    the host: both kernels with and without a K split, image groups of 4, 16 and 64 left partial by the batch, both values of
    `direct` (0: a transposed convolution's input gradient whose parity blocks are no multiple of 8 channels wide), a four-phase
    transposed convolution and a two-group convolution.  As there, no accepted shape stays on the fp32 kernel beside conv_f16x3."""
    reached = set()
    for key, vals in lines.items():
        B, nphase, groups = _KEY.match(key).groups()
        for (route, _, _), val in zip(ROUTES, vals):
            val = vals[0] if val == "=" else val
            m = _HCONV.match(val)
            if m:
                reached.add("conv_f16x3, K split %s" % ("1" if m.group(1) == "1" else "> 1"))
                reached.add("direct %s" % m.group(2))
                continue
            m = _FCONV.match(val)
            assert m, (key, val)
            if route != "conv_f32":
                reached.add("a convolution that stays on the fp32 kernel")
            reached.add("fp32 conv, K split %s" % ("1" if m.group(2) == "1" else "> 1"))
            if int(m.group(1)) > 1 and int(B) % int(m.group(1)):
                reached.add("image group left partial by the batch (%s images a group)" % m.group(1))
        if nphase == "4":
            reached.add("four phases")
        if "+" in groups:
            reached.add("two groups")
    need = ["conv_f16x3, K split 1", "conv_f16x3, K split > 1", "fp32 conv, K split 1", "fp32 conv, K split > 1",
            "image group left partial by the batch (4 images a group)", "image group left partial by the batch (16 images a group)",
            "image group left partial by the batch (64 images a group)", "direct 0", "direct 1", "four phases", "two groups"]
    assert [f for f in need if f not in reached] == []
    assert "a convolution that stays on the fp32 kernel" not in reached, "reachable now: require it"
