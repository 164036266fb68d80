"""The sessions of tests/label_chain_ref.py are what they are for: asserted on the composed restatement alone (no device), so that a change
of a scene, of a rule or of the generator cannot empty a case of tests/test_gpu_label_chain.py.  Conditions, not measurements."""
import functools

import numpy as np
import pytest

import label_chain_ref as ref
import label_contact_ref

SHAPES = (ref.TALL, ref.ODD, ref.LITTLE)
SERVED = {"measure": "measure", "shape": "shape", "contacts": "contacts", "hull": "hull", "objects": "objects"}


def consumer_of(op):
    """the name among ref.CONSUMERS of a resident consumer's operation, else None"""
    if op[0] == "relabel":
        return "relabel_pairs" if op[1] is not None else "relabel_keep"
    return SERVED.get(op[0])


@functools.lru_cache(maxsize=None)
def fixed_sessions():
    s = {("chain", shape): ref.chain_session(shape) for shape in SHAPES}
    s.update({("pairs", shape, variant): ref.pair_session(shape, variant) for shape, variant in ref.PAIRS})
    s[("regrowth",)] = ref.regrowth_session()
    return s


@functools.lru_cache(maxsize=None)
def expected(key):
    return ref.interpret(fixed_sessions()[key])


@pytest.mark.parametrize("shape", SHAPES + (ref.WIDE,))
def test_main_scene_is_crowded_touching_and_its_rules_bite(shape):
    for variant in ref.VARIANTS:
        session = [("run", "discs", shape, variant, True)] + ref.CHAIN
        out = ref.interpret(session)
        labels, table, counts = out[0][1]
        N = len(table)
        assert N >= 64, (shape, variant, N)
        if variant != "plain":                                        # a producer that grows or splits: objects touch
            assert len(label_contact_ref.contacts(labels, N, 0)) > 0, (shape, variant)
            assert len(out[2][1]) > 0 and ref.equal(out[2][1], label_contact_ref.contacts(labels, N, 0))
        if variant in ("split", "split_flood", "hmax", "hmax_flood_grow"):
            assert counts["n_objects"] == N > counts["n_before"] >= 64 and counts["n_cored"] > 0, (shape, variant, counts)
        m = out[3][1][2]                                              # the merge: one class of >= 3 members, one object left alone
        members = np.bincount(m[1:])[1:]
        assert members.max() >= 3 and (members == 1).any() and len(out[3][1][1]) < N, (shape, variant, members.max())
        m = out[7][1][2]                                              # the keep: drops some, keeps some
        assert 0 < (m[1:] > 0).sum() < len(m) - 1, (shape, variant)
        records, vertices = out[5][1]                                 # the hulls: polygons for most objects
        assert (records["n_vertices"] >= 3).sum() > len(records) // 2 and len(vertices) == records["n_vertices"].sum()
        assert all(want is not ref.REFUSED for _, want in out)


def test_the_driver_own_rules_are_used_and_bite():
    """pair_session merges by unmicst_amd.driver.merge_pairs at 0.2 (pairs of touching halves, as the commands find them) and CHAIN keeps
    by unmicst_amd.driver.keep_mask"""
    for shape, variant in ref.PAIRS:
        labels, table, _ = ref.produce("discs", shape, variant)
        pairs = ref.merge_pairs_of(("driver", 0.2), labels, len(table))
        assert 0 < len(pairs) < len(label_contact_ref.contacts(labels, len(table), 0)) or variant == "split_flood" and len(pairs) > 0
        assert ("relabel", ("driver", 0.2), None, True) in ref.pair_session(shape, variant)
    assert ("relabel", None, "median", True) in ref.CHAIN and ref.CHAIN[2] == ("relabel", "star", None, False)


def test_fixed_sessions_cover_the_matrix():
    for shape in SHAPES:
        session = ref.chain_session(shape)
        after = {}
        for op in session:
            if op[0] == "run":
                current = after.setdefault(op[3], set())
            elif consumer_of(op):
                current.add(consumer_of(op) + (str(op[1]) if op[0] == "contacts" else ""))
        assert set(after) == set(ref.VARIANTS)
        wanted = (set(ref.CONSUMERS) - {"contacts"}) | {"contacts0", "contacts%d" % ref.REACH}
        assert all(seen == wanted for seen in after.values()), after
        # the commands' own order, untouched but for the call on a foreign plane
        per_producer = len(session) // len(ref.VARIANTS)
        assert [op for op in session[1:per_producer] if not op[0].endswith("_ptr")] == ref.CHAIN
    for shape, variant in ref.PAIRS:
        session = ref.pair_session(shape, variant)
        pairs = set()
        for i, op in enumerate(session):
            if op[0] == "run":
                assert op[3] == variant and session[i + 1][0] in ref.PTR_CONSUMERS
                pairs.add((consumer_of(session[i + 2]), consumer_of(session[i + 3])))
        assert pairs == {(a, b) for a in ref.CONSUMERS for b in ref.CONSUMERS} and len(pairs) == 49
        assert all(want is not ref.REFUSED for _, want in expected(("pairs", shape, variant)))
    assert {v for _, v in ref.PAIRS} == {"hmax_flood_grow", "split_flood"}


def test_regrowth_session_moves_the_memory_seven_times_in_order():
    """the events of umx_label.hip's ensure_buffers / ensure_table and of the relabel's swap, from the sizes the code compares: pixels,
    bytes of the uploaded planes, whether the split's planes were asked for, and ref.TABLE0 records of a new table"""
    session = ref.regrowth_session()
    out = ref.interpret(session)
    runs = [i for i, op in enumerate(session) if op[0] in ("run", "run_ptr")]
    assert len(runs) == 9

    def size(i):
        planes = out[i][0]["planes"]
        return planes.shape[1] * planes.shape[2], planes.size if session[i][0] == "run" else 0, len(out[i][1][1])

    def split_family(i):
        return session[i][3] not in ("plain", "grow")

    def served_between(a, b):
        return [op for op, (_, want) in zip(session[a + 1:b], out[a + 1:b]) if want is not ref.REFUSED and op[0] != "objects"]

    r = runs
    assert size(r[1])[0] > size(r[0])[0]                                                              # 1. npix grows
    assert size(r[2])[0] == size(r[1])[0] and size(r[2])[1] > size(r[1])[1]                           # 2. K grows alone: 3 -> 4 planes
    assert out[r[1]][0]["planes"].shape[0] == 3 and out[r[2]][0]["planes"].shape[0] == 4
    assert not any(split_family(i) for i in r[:3]) and split_family(r[3]) and size(r[3])[:2] == size(r[2])[:2]   # 3. the first split-family run
    assert session[r[4]][0] == "run_ptr" and session[r[5]][0] == "run" and session[r[4]][1:4] == session[r[5]][1:4]   # 4. host after dev, same shape
    assert size(r[4])[0] > max(size(i)[0] for i in r[:4]) and size(r[5])[1] > max(size(i)[1] for i in r[:5])
    assert size(r[6])[2] > ref.TABLE0 and all(size(i)[2] <= ref.TABLE0 for i in r[:6])                 # 5. the table grows
    swaps = [i for i in range(r[6], r[7]) if session[i][0] == "relabel"]                              # 6. the tables change places ...
    assert len(swaps) == 1 and 0 < len(out[swaps[0]][1][1]) <= 5 and size(r[7])[2] > ref.TABLE0 > 5  # ... the small one must grow ...
    assert [op[0] for op in session[r[7]:r[8]]].count("relabel") == 2                                 # ... and changes places again, twice
    assert size(r[8])[0] < min(size(i)[0] for i in r[1:8])                                            # 7. a smaller shape after all of that
    for a, b in zip(r, r[1:] + [len(session)]):                                                       # a consumer before and after each
        if session[a][0] == "run_ptr":
            assert any(op[0].endswith("_ptr") and op[1] == "own" for op in session[a + 1:b])
        else:
            assert len(served_between(a, b)) >= 2, (a, b)
    assert session[swaps[0] + 1][0] == "shape" and out[swaps[0] + 1][1] is not ref.REFUSED
    assert sum(want is ref.REFUSED for _, want in out) == 0


@pytest.mark.parametrize("key", sorted(fixed_sessions(), key=str), ids=lambda k: "-".join(str(v) for v in k))
@pytest.mark.parametrize("stale", ref.STALE)
def test_a_stale_interpreter_expects_something_else(key, stale):
    """the sessions would notice a labeler that keeps the old N after a relabel, the old plane after a producer, or lets a *_ptr
    consumer replace the resident plane: an interpreter that is stale in that one way expects another result from a later operation"""
    session, right = fixed_sessions()[key], expected(key)
    wrong = ref.interpret(session, stale=stale)
    differ = [i for i, (a, b) in enumerate(zip(right, wrong)) if not ref.equal(a[1], b[1])]
    assert differ, (key, stale)
    first = {"old_N": lambda op: op[0] == "relabel", "old_plane": lambda op: op[0] == "run", "ptr_replaces": lambda op: op[0].endswith("_ptr")}[stale]
    assert min(i for i, op in enumerate(session) if first(op)) < differ[0]


def test_random_sessions_are_deterministic_and_cover_every_operation():
    seen = {}
    for seed in ref.SEEDS:
        session = ref.random_session(seed, ref.LENGTH)
        assert session == ref.random_session(seed, ref.LENGTH) and session != ref.random_session(seed + 100, ref.LENGTH)
        assert ref.LENGTH <= len(session) <= ref.LENGTH + 12
        out = ref.interpret(session)
        resident = False
        for op, (_, want) in zip(session, out):
            names = []
            if op[0] in ("run", "run_ptr"):
                names = [op[3], op[0] + ("" if op[4] else ", no plane"), "shape %d x %d" % op[2]]
                resident = op[0] == "run" and op[4]
            elif op[0].startswith("refuse"):
                assert want is ref.REFUSED
                names = [op[0]]
            elif op[0].endswith("_ptr"):
                assert want is not ref.REFUSED
                names = [op[0], op[0] + " " + op[1]]
            elif want is ref.REFUSED:
                assert not resident and op[0] != "objects"
                names = ["no_resident"]
            else:
                assert resident or op[0] == "objects"
                names = [consumer_of(op)]
            for n in names:
                seen[n] = seen.get(n, 0) + 1
        # the replay of the GPU test starts at a producer and has something to compare
        last, rest = ref.tail(session)
        assert len(rest) >= 3 and ref.equal([w for _, w in ref.interpret(rest)], [w for _, w in out[last:]])
    for name in ref.VARIANTS + ref.CONSUMERS + ref.PTR_CONSUMERS + ref.REFUSALS + ("run", "run_ptr", "run, no plane"):
        assert seen.get(name, 0) >= 3, (name, seen)
    for shape in SHAPES + (ref.WIDE,) + ref.THIN:
        assert seen.get("shape %d x %d" % shape, 0) >= 1, shape
    assert all(seen.get(p + " own", 0) >= 1 for p in ref.PTR_CONSUMERS), seen
