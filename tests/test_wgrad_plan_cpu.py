"""The weight-gradient planner (wgrad_setup) and the kernel selection (wgrad_select) on the host, through umx_test_wgrad_plan: no device
needed.  Every weight-gradient layer of the shipped hyper-parameter sets and of synthetic-256 at batch 8 and 16, and of the odd shapes
of tests/train_parity.py::tight_cases() at their own batch, each on the split-precision route with and without operand planes and on
the UMX_TRAIN_WGRAD_F32 route, against lines recorded from the planner and launcher as they stood before the two were separated
(tests/golden/wgrad_plan_lines.json), and a check that the list reaches all 16 kernel instantiations."""
import json
import os

import pytest

from unmicst_amd import model, umx

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "wgrad_plan_lines.json")

INSTANTIATIONS = (["wgrad_mfma_f32<%s>" % a for a in ("1,false", "1,true", "2,false", "2,true", "3,false")]
                  + ["wgrad_thin_kernel<%d,%d>" % (cx, v) for cx in (1, 2, 3, 4) for v in (4, 1)]
                  + ["wgrad_f16x3<%s>" % a for a in ("false,false", "true,false", "true,true")])


def _same_taps(ks):
    """(dy, dx, master tap, channel offset) of a stride-1 SAME convolution: same_taps of the trainer"""
    ph = (ks - 1) // 2
    return [(a - ph, b - ph, a * ks + b, 0) for a in range(ks) for b in range(ks)]


def _transposed_slabs(ks, Cup):
    """The slabs of a stride-2 transposed convolution's weight gradient on the space-to-depth output gradient, grouped by parity block
    (setup_up_layer): tap a reads dY at q = a - pb = 2 * d + parity."""
    pb = (ks - 2) // 2

    def split(q):
        par = q % 2
        return (q - par) // 2, par
    out = []
    for par in range(4):
        for a in range(ks):
            for b in range(ks):
                (di, pa), (dj, pbb) = split(a - pb), split(b - pb)
                if pa * 2 + pbb == par:
                    out.append((di, dj, a * ks + b, par * Cup))
    return out


def layers(hp):
    """(H, Cxt, Cx, Cg, kind of slabs, slabs) of every setup_wgrad call of the trainer's build"""
    n, L, ks, P = hp.nOutX, hp.nLayers, hp.ks, hp.imSize
    E = hp.nExtraConvs if hp.graph == model.GRAPH_LEGACY else 0
    fwd, out, k = _same_taps(ks), [], "k%d" % ks
    for i in range(L):
        S = P >> i
        for e in range(1, E + 1):
            out.append((S, n[i + 1], n[i + 1], n[i + 1], k, fwd))
        out.append((S, n[i], n[i], n[i + 1], k, fwd))
        if hp.graph == model.GRAPH_LEGACY:
            out.append((S, n[i], n[i], n[i + 1], "k1", [(0, 0, 0, 0)]))
    out.append((P >> L, n[L], n[L], n[L + 1], k, fwd))
    for idx in range(L - 1, -1, -1):
        Cskip, Cup, Cin = n[idx], n[idx + 1], n[idx + 2]
        S = P >> (idx + 1)
        out.append((S, 4 * Cup, Cup, Cin, "T%d" % ks, _transposed_slabs(ks, Cup)))
        out.append((2 * S, Cskip, Cskip, Cup, k, fwd))
        out.append((2 * S, Cup, Cup, Cup, k, fwd))
        for e in range(1, E + 1):
            out.append((2 * S, Cup, Cup, Cup, k, fwd))
    return out


def cases():
    """key -> arguments of umx.wgrad_plan.  Planes, where present, store round_up(C, 8) channels (alloc_planes)."""
    import train_parity
    sets = [(hp, B) for hp in model.KNOWN_HP.values() for B in (8, 16)]
    sets += [(c[0], c[1]) for c in train_parity.tight_cases().values()]
    # two thin forms no set above has: a first layer of 3 channels with Cg % 4 == 0, and one of 4 channels with Cg % 4 != 0
    sets += [(model.HParams(model.GRAPH_V2, 32, 3, 3, 8, 2, 3, 0), 2), (model.HParams(model.GRAPH_V2, 32, 4, 3, 6, 2, 3, 0), 2)]
    out = {}
    for hp, B in sets:
        for H, Cxt, Cx, Cg, kind, slabs in layers(hp):
            for route, f32, planes in (("f16x3+planes", False, True), ("f16x3", False, False), ("fp32", True, False)):
                key = "b%d %dx%d X%d(of %d) G%d %s %s" % (B, H, H, Cx, Cxt, Cg, kind, route)
                out[key] = (B, H, Cxt, Cx, Cg, slabs, f32, planes, -(-Cxt // 8) * 8, -(-Cg // 8) * 8)
    return out


def line_of(args):
    try:
        return umx.wgrad_plan(*args)
    except umx.UmxError as e:
        return "refused: " + str(e)


@pytest.fixture(scope="module")
def lines():
    return {key: line_of(args) for key, args in cases().items()}


def test_plan_and_selection_are_the_recorded_ones(lines):
    with open(GOLDEN) as f:
        want = json.load(f)
    assert sorted(lines) == sorted(want)
    wrong = {k: (lines[k], want[k]) for k in want if lines[k] != want[k]}
    assert not wrong, list(wrong.items())[:5]


def test_the_list_reaches_every_instantiation(lines):
    reached = {ln.split(", ")[-4] for ln in lines.values() if not ln.startswith("refused")}
    assert reached == set(INSTANTIATIONS), sorted(set(INSTANTIATIONS) - reached)
