"""The composed restatement of the label mask: an interpreter of *sessions* -- lists of operations on ONE labeler, written as plain
tuples -- that keeps in numpy what a umx_labeler keeps on the device (include/umx.h, DESIGN.md section 8.1, "how the stages are tested
together"): the resident label plane with its H, W, N and object table, and, when there is no resident plane, why not:

  state        entered by                                                       resident consumers
  "never"      a new labeler                                                    refused
  None         a host run that was given a label plane; a relabel of it          served
  "no plane"   a host run without a label plane                                  refused
  "dev"        a run_ptr (its labels are the caller's: the *_ptr consumers)      refused
  (a refused call -- bad cls, another H or W, a pair that names a dropped label, no resident plane -- and every *_ptr consumer leave
  the state as it was; objects() is the table of the last run or relabel in every state.)

It states no stage a second time: every expected value is a call of the stages' own restatements (label_ref, label_grow_ref,
label_split_ref, label_flood_ref, label_hmax_ref, label_measure_ref, label_shape_ref, label_contact_ref, label_hull_ref,
label_relabel_ref), and the merge and keep rules of the driver are the driver's own merge_pairs and keep_mask.

Operations (`interpret` returns, for each, the concrete arguments and the expected result, or REFUSED):

  ("run" | "run_ptr", scene, shape, variant, want_labels)    variant in VARIANTS
  ("measure", source)         source: "scene" (the last producer's planes), ("px", "u8" | "u16", C) or ("named", key)
  ("shape",)  ("contacts", reach)  ("hull",)  ("objects",)
  ("relabel", merge rule | None, keep rule | None, want_labels)      rules: see merge_pairs_of and keep_of
  ("measure_ptr", on, source)  ("shape_ptr", on)  ("contacts_ptr", on, reach)  ("hull_ptr", on)  ("relabel_ptr", on, merge, keep)
                              on: "foreign" (a caller's plane of another shape) or "own" (the plane the last run_ptr wrote)
  ("refuse_cls", scene, shape, variant)  ("refuse_shape", consumer)  ("refuse_pair",)

`perform` is the one place where an operation becomes a call of umx.Labeler; the GPU tests and their guard-mode child share it.

A FUTURE STAGE extends three places, and the CPU test (tests/test_label_chain_cpu.py) fails until all three know it:
  1. the operation list: VARIANTS / CONSUMERS / PTR_CONSUMERS here, with its branch in `interpret` and in `perform`;
  2. the generator: the decks of `random_session`;
  3. the producer-by-consumer matrix: CHAIN and `chain_session` / `pair_session`."""
import functools

import numpy as np
from scipy import ndimage

import label_contact_ref
import label_flood_ref
import label_grow_ref
import label_hmax_ref
import label_hull_ref
import label_measure_ref
import label_ref
import label_relabel_ref
import label_shape_ref
import label_split_ref

TALL, WIDE, ODD, LITTLE = (130, 150), (70, 200), (97, 131), (40, 50)       # the stage tests' shapes (LABEL_GROW_TILE = 64, _HALO = 8)
THIN = ((1, 130), (130, 1))
HMAX, STEP, GROW, REACH = 10, 16, 2, 3
VARIANTS = ("plain", "grow", "split", "split_flood", "hmax", "hmax_flood_grow")
CONSUMERS = ("measure", "shape", "contacts", "hull", "relabel_pairs", "relabel_keep", "objects")
PTR_CONSUMERS = ("measure_ptr", "shape_ptr", "contacts_ptr", "hull_ptr", "relabel_ptr")
REFUSALS = ("refuse_cls", "refuse_shape", "refuse_pair", "no_resident")
REFUSED = "refused"                                                          # UmxError with ERR_INVALID, nothing changed
STALE = ("old_N", "old_plane", "ptr_replaces")
FOREIGN = WIDE                                                               # the caller's plane of the *_ptr consumers; (97, 70) when the resident one is WIDE

# the main scene per shape: (radius, shift, pitch, margin, split depth) of label_hmax_ref.overlapping_discs, chosen so that every
# producer leaves >= 64 objects and the erosion of the given depth cuts the pairs as the h-maxima do (asserted in the CPU test)
DISCS = {TALL: (5, 8, 12, 0, 4), WIDE: (3, 4, 8, 0, 3), ODD: (3, 4, 8, 0, 3), LITTLE: (1, 2, 4, 2, 1)}


class Scene:
    def __init__(self, planes, cls, min_area, classes, S, P, D):
        planes.setflags(write=False)
        self.planes, self.cls, self.min_area, self.classes, self.S, self.P, self.D = planes, cls, min_area, tuple(classes), S, P, D


EXTRA_SCENES = {}                                                            # name -> Scene, for planes a test reads from a file


@functools.lru_cache(maxsize=None)
def scene(name, shape):
    """"discs": pairs of overlapping discs (one dome each in plane 3, a random flood relief in plane 1, a rim of class 1 three pixels
    wide), cropped by its margin so that objects lie on the border; any name of label_ref.NAMES with K = 3: that case, the seed
    plane 1, the flood's plane 0"""
    if name in EXTRA_SCENES:
        return EXTRA_SCENES[name]
    H, W = shape
    if name == "discs":
        radius, shift, pitch, m, D = DISCS[shape]
        mask, relief, _ = label_hmax_ref.overlapping_discs(H + 2 * m, W + 2 * m, radius, shift, pitch)
        mask, relief = mask[m:m + H, m:m + W], relief[m:m + H, m:m + W]
        flood_relief = np.where(mask, np.random.default_rng(H * W).integers(0, 255, (H, W)), 0)
        planes = label_hmax_ref.planes_of(mask, relief, flood_relief, ndimage.binary_dilation(mask, iterations=3))
        return Scene(planes, 2, 1, (1,), 3, 1, D)
    planes, cls, min_area = label_ref.case(H, W, name)
    assert planes.shape[0] == 3 and cls == 2
    return Scene(planes, cls, min_area, (1,), 1, 0, 1)


def run_kwargs(sc, variant):
    """the keyword arguments of umx.Labeler.run / run_ptr for a producer variant"""
    kw = dict(cls=sc.cls, min_area=sc.min_area)
    if "grow" in variant:
        kw.update(grow=GROW, grow_classes=sc.classes)
    if variant.startswith("split"):
        kw.update(split=sc.D)
    if variant.startswith("hmax"):
        kw.update(hmax=HMAX, hmax_plane=sc.S)
    if "flood" in variant:
        kw.update(flood=sc.P, flood_step=STEP)
    return kw


@functools.lru_cache(maxsize=None)
def produce(name, shape, variant):
    """-> (labels, table, counts): the producer's own restatement; counts {} where the call has none"""
    sc = scene(name, shape)
    p, R = sc.planes, GROW if "grow" in variant else 0
    if variant in ("plain", "grow"):
        out = label_grow_ref.label_grow(p, sc.cls, sc.min_area, R, sc.classes) + ({},)
    elif variant == "split":
        out = label_split_ref.split(p, sc.cls, sc.min_area, sc.D)
    elif variant == "split_flood":
        out = label_flood_ref.split_flood(p, sc.cls, sc.min_area, sc.D, 1, sc.P, STEP)
    elif variant == "split_flood_grow":                                      # (not among VARIANTS: the commands' second run)
        out = label_flood_ref.split_flood(p, sc.cls, sc.min_area, sc.D, 1, sc.P, STEP, R=R, classes=sc.classes)
    elif variant == "hmax":
        out = label_hmax_ref.hmax(p, sc.cls, sc.min_area, HMAX, sc.S)
    elif variant == "hmax_flood_grow":
        out = label_hmax_ref.hmax(p, sc.cls, sc.min_area, HMAX, sc.S, P=sc.P, q=STEP, R=R, classes=sc.classes)
    else:
        raise KeyError(variant)
    labels, table = np.ascontiguousarray(out[0], np.int32), out[1]
    labels.setflags(write=False)
    table.setflags(write=False)
    return labels, table, dict(out[2])


@functools.lru_cache(maxsize=None)
def pixels(shape, dtype, C):
    px = label_measure_ref.pixels(shape, {"u8": np.uint8, "u16": np.uint16}[dtype], C, seed=7 + C)
    px.setflags(write=False)
    return px


@functools.lru_cache(maxsize=None)
def foreign(shape):
    """the caller's own label plane: pieces of 7 labels spread over the rows (label_shape_ref.seeded_labels) -> (labels, N)"""
    labels, N = label_shape_ref.seeded_labels(shape[0], shape[1], seed=2)
    labels.setflags(write=False)
    return labels, N


def foreign_shape(H, W):
    return FOREIGN if (H, W) != FOREIGN else (ODD[0], WIDE[0])


# ---- rules: pairs and keep masks derived from the plane they are applied to ----
def merge_pairs_of(rule, labels, N):
    """"star": the contacts (within REACH) of the object with the most neighbours and of its neighbours -- one class of >= 3 members
    where an object has two neighbours; "touch": every second contact at reach 0; ("driver", F): unmicst_amd.driver.merge_pairs on the
    contacts at reach 0 and the perimeter edges of the shapes, as the commands do.  -> int32 [M, 2]"""
    from unmicst_amd import driver, umx
    if rule is None:
        return None
    if N == 0:
        return np.zeros((0, 2), np.int32)
    if rule == "star":
        c = label_contact_ref.contacts(labels, N, REACH)
        degree = np.bincount(np.concatenate([c["a"], c["b"]]), minlength=N + 1)
        j = int(np.argmax(degree))
        near = {j} | set(c["b"][c["a"] == j].tolist()) | set(c["a"][c["b"] == j].tolist())
        take = np.isin(c["a"], sorted(near)) | np.isin(c["b"], sorted(near))
        return np.stack([c["a"][take], c["b"][take]], 1).astype(np.int32).reshape(-1, 2)
    if rule == "touch":
        c = label_contact_ref.contacts(labels, N, 0)
        return np.stack([c["a"], c["b"]], 1)[::2].astype(np.int32).reshape(-1, 2)
    if rule[0] == "driver":
        perimeter_edges = umx.shape_descriptors(label_shape_ref.records(labels, N))["perimeter_edges"]
        return driver.merge_pairs(label_contact_ref.contacts(labels, N, 0), perimeter_edges, rule[1])
    raise KeyError(rule)


def keep_of(rule, labels, N, table, planes=None):
    """"median": area >= the median area and the box's first row in the upper 0.6 of the plane (where every object has the same
    area the first rule alone drops nothing), by unmicst_amd.driver.keep_mask on driver.object_columns; "thirds": every third label
    dropped; "first_five": labels 1..5 alone; "but_least": all but the (first) smallest object; ("rules", texts): the commands' --labelKeep rules on the driver's own
    columns of the restated tables (pm<k> columns from `planes`).  -> uint8 [N]"""
    from unmicst_amd import driver
    if rule is None:
        return None
    if N == 0:
        return np.zeros(0, np.uint8)
    if rule == "median":
        columns = dict(driver.object_columns(table, labels.shape), y0=table["y0"])
        return driver.keep_mask([("area", ">=", float(np.median(table["area"]))), ("y0", "<", 0.6 * labels.shape[0])], columns)
    if rule == "thirds":
        return (np.arange(N) % 3 != 1).astype(np.uint8)
    if rule == "first_five":
        return (np.arange(N) < 5).astype(np.uint8)
    if rule == "but_least":
        keep = np.ones(N, np.uint8)
        keep[int(np.argmin(table["area"]))] = 0
        return keep
    if rule[0] == "rules":
        rules = [driver.parse_keep_rule(t) for t in rule[1]]
        columns = driver.object_columns(table, labels.shape)
        columns.update(driver.shape_columns(table, label_shape_ref.records(labels, N)))
        columns.update(driver.hull_columns(table, *label_hull_ref.hulls(labels, N)))
        pm = label_measure_ref.measure(labels, planes, N)
        columns.update(driver.intensity_columns(table, [("pm%d" % k, pm[k]) for k in range(len(pm))]))
        return driver.keep_mask(rules, columns)
    raise KeyError(rule)


# ---- the interpreter ----
class State:
    def __init__(self):
        self.plane, self.H, self.W, self.N = None, 0, 0, 0
        self.why = "never"
        self.table = np.zeros(0, label_ref.OBJECT)                           # what objects() returns
        self.planes = None                                                   # the last producer's planes ("scene" measurements)
        self.own = None                                                      # (plane, N) the last run_ptr left with the caller
        self.counts = {}


def _consume(kind, op, labels, N, planes, named):
    """a consumer's restatement on a plane -> (args, want)"""
    if kind == "measure":
        src = op[-1]
        px = planes if src == "scene" else named[src[1]] if src[0] == "named" else pixels(labels.shape, src[1], src[2])
        if px.shape[1:] != labels.shape:                                     # (only a stale interpreter comes here)
            px = pixels(labels.shape, "u8", 1)
        return dict(px=px), label_measure_ref.measure(labels, px, N)
    if kind == "shape":
        return {}, label_shape_ref.records(labels, N)
    if kind == "contacts":
        return dict(reach=op[-1]), label_contact_ref.contacts(labels, N, op[-1])
    if kind == "hull":
        return {}, label_hull_ref.hulls(labels, N)
    raise KeyError(kind)


def interpret(session, stale=None, named=None):
    """-> [(args, want)] per operation; want is REFUSED or the expected result:
      run / run_ptr: (labels | None, table, counts);  measure, shape, contacts: the records;  hull: (records, vertices);
      relabel: (labels | None, table, map);  relabel_ptr: (labels, map, N');  objects: the table.
    stale: one of STALE -- an interpreter that is wrong in that one way (for the sensitivity checks of the CPU test only)."""
    assert stale is None or stale in STALE
    st, out = State(), []

    def step(op):
            kind = op[0]
            if kind in ("run", "run_ptr"):
                _, name, shape, variant, want_labels = op
                sc = scene(name, shape)
                labels, table, counts = produce(name, shape, variant)
                args = dict(planes=sc.planes, kw=run_kwargs(sc, variant), want_labels=want_labels)
                result = (args, (labels if want_labels else None, table, counts))
                keep_old = stale == "old_plane" and st.why is None and st.plane.shape == labels.shape
                st.table, st.planes, st.counts, st.own = table, sc.planes, counts, None
                if kind == "run" and want_labels:
                    st.plane, st.H, st.W, st.N, st.why = (st.plane if keep_old else labels), shape[0], shape[1], len(table), None
                else:
                    st.plane, st.why = None, "no plane" if kind == "run" else "dev"
                    if kind == "run_ptr" and want_labels:
                        st.own = (labels, len(table))
            elif kind == "refuse_cls":
                sc = scene(op[1], op[2])
                result = (dict(planes=sc.planes, kw=dict(run_kwargs(sc, op[3]), cls=sc.planes.shape[0])), REFUSED)
            elif kind == "refuse_shape":
                H, W = (st.W, st.H) if st.H != st.W else (st.H + 1, st.W)
                result = (dict(H=max(H, 1), W=max(W, 1), consumer=op[1]), REFUSED)
            elif kind == "refuse_pair":
                keep = np.ones(max(st.N, 1), np.uint8)
                keep[0] = 0
                result = (dict(keep=keep, pairs=np.array([[1, 2]], np.int32)), REFUSED)
            elif kind == "objects":
                result = ({}, st.table)
            elif kind in ("measure", "shape", "contacts", "hull"):
                if st.why is not None:
                    result = (dict(px=np.zeros((1, 1, 1), np.uint8), reach=op[-1] if kind == "contacts" else 0), REFUSED)
                else:
                    result = _consume(kind, op, st.plane, st.N, st.planes, named)
            elif kind == "relabel":
                _, merge, keep_rule, want_labels = op
                if st.why is not None:
                    return dict(keep=None, pairs=None, want_labels=want_labels), REFUSED
                pairs = merge_pairs_of(merge, st.plane, st.N)
                keep = keep_of(keep_rule, st.plane, st.N, st.table, st.planes)
                labels, table, m = label_relabel_ref.relabel(st.plane, st.N, keep, pairs)
                labels = np.ascontiguousarray(labels, np.int32)
                result = (dict(keep=keep, pairs=pairs, want_labels=want_labels), (labels if want_labels else None, table, m))
                st.plane, st.table = labels, table
                if stale != "old_N":
                    st.N = len(table)
            elif kind in PTR_CONSUMERS:
                on = op[1]
                if on == "own":
                    assert st.own is not None, "an operation on the caller's own plane needs a run_ptr with a label plane before it"
                    labels, N = st.own
                else:
                    labels, N = foreign(foreign_shape(st.H, st.W))
                args = dict(labels=labels, N=N, on=on)
                if kind == "relabel_ptr":
                    table = label_relabel_ref.table_of(label_relabel_ref.clean(labels, N), N)
                    pairs = merge_pairs_of(op[2], labels, N)
                    keep = keep_of(op[3], labels, N, table, st.planes)
                    new, new_table, m = label_relabel_ref.relabel(labels, N, keep, pairs)
                    new = np.ascontiguousarray(new, np.int32)
                    result = (dict(args, keep=keep, pairs=pairs), (new, m, len(new_table)))
                    if on == "own":
                        st.own = (new, len(new_table))                           # in place: the caller's plane is the new one
                    labels, N = new, len(new_table)
                else:
                    a, want = _consume(kind[:-4], op, labels, N, st.planes if on == "own" else None, named)
                    result = (dict(args, **a), want)
                if stale == "ptr_replaces":
                    st.plane, st.H, st.W, st.N, st.why = labels, labels.shape[0], labels.shape[1], N, None
            else:
                raise KeyError(op)
            return result

    for op in session:
        try:
            out.append(step(op))
        except (ValueError, AssertionError, IndexError) as e:                # a stale interpreter's state need not make sense
            if stale is None:
                raise
            out.append(({}, ("undefined", type(e).__name__)))
    return out


def equal(got, want):
    """exact equality of two results: REFUSED, None, ints, dicts of ints, arrays (structured ones field by field of `want`), tuples"""
    if isinstance(want, (tuple, list)):
        return isinstance(got, (tuple, list)) and len(got) == len(want) and all(equal(g, w) for g, w in zip(got, want))
    if isinstance(want, np.ndarray):
        if not isinstance(got, np.ndarray) or got.shape != want.shape:
            return False
        if want.dtype.names:
            return got.dtype.names is not None and all(n in got.dtype.names and np.array_equal(got[n], want[n]) for n in want.dtype.names)
        return got.dtype.kind == want.dtype.kind and got.dtype.itemsize == want.dtype.itemsize and np.array_equal(got, want)
    return type(got) is type(want) and got == want


# ---- the fixed sessions ----
# the order in which the commands call one labeler (unmicst_amd/driver.py, run, the args.labelMask block), and objects() at its end
def chain(merge="star", keep="median", measure="scene"):
    return [("shape",), ("contacts", 0), ("relabel", merge, None, False), ("shape",), ("hull",), ("measure", measure),
            ("relabel", None, keep, True), ("measure", measure), ("shape",), ("contacts", REACH), ("hull",), ("objects",)]


CHAIN = chain()


def intruder(i):
    """the i-th *_ptr consumer on a foreign plane: it must serve that plane and leave the resident one alone"""
    return [("measure_ptr", "foreign", ("px", "u16", 5)), ("shape_ptr", "foreign"), ("contacts_ptr", "foreign", REACH), ("hull_ptr", "foreign"),
            ("relabel_ptr", "foreign", "touch", None), ("contacts_ptr", "foreign", 0)][i % 6]


def chain_session(shape, name="discs"):
    """(a): the six producers one after the other on one labeler, each followed by the commands' twelve calls -- with a *_ptr call on a
    foreign plane after the first relabel"""
    s = []
    for i, variant in enumerate(VARIANTS):
        s += [("run", name, shape, variant, True)] + CHAIN[:3] + [intruder(i)] + CHAIN[3:]
    return s


def consumer_op(c, reach=REACH, merge=("driver", 0.2)):
    return {"measure": ("measure", ("px", "u16", 5)), "shape": ("shape",), "contacts": ("contacts", reach), "hull": ("hull",),
            "relabel_pairs": ("relabel", merge, None, True), "relabel_keep": ("relabel", None, "thirds", False), "objects": ("objects",)}[c]


def pair_session(shape, variant, name="discs"):
    """(b): every ordered pair (A, B) of the seven consumers after a fresh run of the producer on the same labeler, a *_ptr call on a
    foreign plane before each pair"""
    s = []
    for i, a in enumerate(CONSUMERS):
        for j, b in enumerate(CONSUMERS):
            s += [("run", name, shape, variant, True), intruder(7 * i + j), consumer_op(a), consumer_op(b, 0 if a == "contacts" else REACH)]
    return s


def dev_session(shape, variant, name="discs"):
    """(e): the chain with the producer as run_ptr and the consumers as *_ptr on the plane it wrote"""
    s = [("run_ptr", name, shape, variant, True)]
    for op in CHAIN:
        if op[0] == "relabel":
            s.append(("relabel_ptr", "own", op[1], op[2]))
        elif op[0] != "objects":
            s.append((op[0] + "_ptr", "own") + op[1:])
    return s + [("shape",), ("relabel", None, "thirds", True), ("objects",)]      # the resident consumers are refused after it


def regrowth_session():
    """(d): every event that moves the labeler's memory, in the order of the list in the CPU test, a consumer before and after each"""
    BIG = (150, 203)
    few = [("shape",), ("contacts", REACH), ("hull",), ("measure", ("px", "u8", 1))]
    return ([("run", "blobs", LITTLE, "plain", True)] + few +
            [("run", "blobs", ODD, "plain", True)] + few +                                        # 1. npix grows
            [("run", "discs", ODD, "plain", True)] + few +                                        # 2. K grows, 3 -> 4 planes
            [("run", "discs", ODD, "hmax_flood_grow", True), intruder(2)] + few + [("relabel", "star", None, True), ("hull",)] +   # 3. the first split-family run
            [("run_ptr", "discs", TALL, "split_flood", True), ("shape_ptr", "own"), ("objects",),
             ("run", "discs", TALL, "split_flood", True)] + few +                                 # 4. a host run after a run_ptr of the same shape
            [("run", "checker", BIG, "plain", True), ("objects",), ("measure", ("px", "u16", 5)), ("contacts", 1)] +   # 5. > 1024 objects
            [("relabel", None, "first_five", True)] + few +                                       # 6. the tables change places ...
            [("run", "checker", BIG, "plain", True), ("contacts", 1), ("relabel", None, "thirds", True), ("objects",), ("measure", ("px", "u8", 1)),
             ("relabel", "touch", "but_least", False), ("contacts", 1)] +                         # ... and the swapped one must grow
            [("run", "discs", LITTLE, "hmax_flood_grow", True)] + CHAIN)                          # 7. a smaller shape after all of that


# ---- the generator ----
class Deck:
    """draws without replacement from a shuffled copy of `items`, shuffled again when it is empty: every item comes round"""

    def __init__(self, rng, items):
        self.rng, self.items, self.left = rng, list(items), []

    def draw(self):
        if not self.left:
            self.left = [self.items[i] for i in self.rng.permutation(len(self.items))]
        return self.left.pop()


def random_session(seed, length=40):
    """A walk of about `length` operations, the same for the same seed: a producer, then -- where it left resident labels -- a stretch
    of consumers, *_ptr calls on a foreign plane and refusals; where it did not, the refused consumers, objects() and the *_ptr calls
    on the plane a run_ptr wrote."""
    rng = np.random.default_rng(seed)
    variants, forms = Deck(rng, VARIANTS), Deck(rng, ["host", "host", "host", "host", "no plane", "dev", "dev"])
    places = Deck(rng, [("discs", TALL), ("discs", ODD), ("discs", LITTLE), ("discs", WIDE), ("discs", LITTLE), ("salt", THIN[0]), ("salt", THIN[1])])
    consumers, ptrs, refusals = Deck(rng, CONSUMERS + ("contacts0", "measure1")), Deck(rng, range(6)), Deck(rng, REFUSALS[:3])
    merges, keeps = Deck(rng, ["star", "touch", ("driver", 0.2)]), Deck(rng, ["median", "thirds", "but_least"])
    wrong_shape = Deck(rng, ["measure", "shape", "contacts", "hull", "relabel"])

    def consumer():
        c = consumers.draw()
        if c == "contacts0":
            return ("contacts", 0)
        if c == "measure1":
            return ("measure", ("px", "u8", 1))
        if c == "relabel_pairs":
            return ("relabel", merges.draw(), None, bool(rng.integers(2)))
        if c == "relabel_keep":
            return ("relabel", None, keeps.draw(), bool(rng.integers(2)))
        return consumer_op(c)

    def refusal(name, shape, variant):
        r = refusals.draw()
        return ("refuse_cls", name, shape, variant) if r == "refuse_cls" else ("refuse_shape", wrong_shape.draw()) if r == "refuse_shape" else ("refuse_pair",)

    s, devs = [consumer()], 0                                                 # before any run: refused
    while len(s) < length:
        (name, shape), variant, form = places.draw(), variants.draw(), forms.draw()
        if form == "host":
            s.append(("run", name, shape, variant, True))
            for _ in range(int(rng.integers(4, 8))):
                u = rng.random()
                s.append(consumer() if u < 0.65 else intruder(ptrs.draw()) if u < 0.85 else refusal(name, shape, variant))
        elif form == "no plane":
            s += [("run", name, shape, variant, False), consumer(), ("objects",), intruder(ptrs.draw()), refusal(name, shape, variant)]
        else:
            want = devs == 0 or bool(rng.integers(4))
            s += [("run_ptr", name, shape, variant, want), consumer(), ("objects",)]
            if want:
                own = intruder((seed + devs) % 5)                             # over the seeds: every *_ptr consumer on the plane a run_ptr wrote
                devs += 1
                s += [(own[0], "own") + own[2:], ("relabel_ptr", "own", None, keeps.draw()), ("shape_ptr", "own")]
            s.append(intruder(ptrs.draw()))
    return s


SEEDS, LENGTH = (1, 2, 3, 4, 5), 40                                         # the walks of the GPU test, held to their coverage by the CPU test
PAIRS = ((ODD, "hmax_flood_grow"), (TALL, "split_flood"))                    # the producers of the GPU test's consumer pairs
TABLE0 = 1024                                                                # records of a new labeler's object table (umx_label.hip, ensure_buffers)


def tail(session):
    """the last producer and what follows it"""
    last = max(i for i, op in enumerate(session) if op[0] in ("run", "run_ptr"))
    return last, session[last:]


# ---- the one place where an operation becomes a call of the labeler ----
def counts_of(lb):
    """the restated counts of the labeler's last run, by the most specific of its three records"""
    for counts, names in ((lb.hmax_counts(), label_hmax_ref.COUNTS), (lb.flood_counts(), label_flood_ref.COUNTS), (lb.split_counts(), label_split_ref.COUNTS)):
        if counts is not None:
            return {n: counts[n] for n in names}
    return {}


def perform(lb, op, args, ctx):
    """op on the umx.Labeler `lb` with the interpreter's `args` -> the result in the interpreter's form, REFUSED for an UmxError with
    ERR_INVALID.  ctx: a dict the caller keeps for one labeler (the device tensors of the caller's planes)."""
    from unmicst_amd import umx
    kind = op[0]
    try:
        if kind in ("run", "refuse_cls"):
            labels, table = lb.run(args["planes"], want_labels=args.get("want_labels", True), **args["kw"])
            return labels, table, counts_of(lb)
        if kind == "run_ptr":
            import torch
            K, H, W = args["planes"].shape
            d_planes = torch.from_numpy(np.array(args["planes"])).cuda()
            d_labels = torch.full((H, W), -7, dtype=torch.int32, device="cuda") if args["want_labels"] else None
            torch.cuda.synchronize()
            table = lb.run_ptr(d_planes.data_ptr(), K, H, W, d_labels.data_ptr() if args["want_labels"] else 0, **args["kw"])
            ctx["own"] = d_labels
            return (d_labels.cpu().numpy() if args["want_labels"] else None), table, counts_of(lb)
        if kind == "refuse_shape":
            H, W = args["H"], args["W"]
            return {"measure": lambda: lb.measure(np.zeros((1, H, W), np.uint8)), "shape": lambda: lb.shape(H, W), "contacts": lambda: lb.contacts(0, H, W),
                    "hull": lambda: lb.hull(H, W), "relabel": lambda: lb.relabel(H=H, W=W)}[args["consumer"]]()
        if kind == "refuse_pair":
            return lb.relabel(args["keep"], args["pairs"])
        if kind == "objects":
            return lb.objects()
        if kind == "measure":
            return lb.measure(args["px"])
        if kind == "shape":
            return lb.shape()
        if kind == "contacts":
            return lb.contacts(args["reach"])
        if kind == "hull":
            return lb.hull()
        if kind == "relabel":
            return lb.relabel(args["keep"], args["pairs"], want_labels=args["want_labels"])
        if kind in PTR_CONSUMERS:
            import torch
            labels, N = args["labels"], args["N"]
            H, W = labels.shape
            if args["on"] == "own":
                d = ctx["own"]
            else:
                d = torch.from_numpy(np.array(labels)).cuda()
            torch.cuda.synchronize()
            before = None if kind == "relabel_ptr" else d.cpu().numpy()
            if kind == "measure_ptr":
                px = args["px"]
                d_px = torch.from_numpy(np.array(px).view(np.int16 if px.dtype == np.uint16 else np.uint8)).cuda()
                torch.cuda.synchronize()
                got = lb.measure_ptr(d.data_ptr(), N, d_px.data_ptr(), px.dtype, px.shape[0], H, W)
            elif kind == "shape_ptr":
                got = lb.shape_ptr(d.data_ptr(), N, H, W)
            elif kind == "contacts_ptr":
                got = lb.contacts_ptr(d.data_ptr(), N, H, W, args["reach"])
            elif kind == "hull_ptr":
                got = lb.hull_ptr(d.data_ptr(), N, H, W)
            else:
                m, n_new = lb.relabel_ptr(d.data_ptr(), N, H, W, args["keep"], args["pairs"])
                return d.cpu().numpy(), m, n_new
            assert np.array_equal(d.cpu().numpy(), before), "a *_ptr consumer wrote to the caller's plane"
            return got
    except umx.UmxError as e:
        if e.code != umx.ERR_INVALID:
            raise
        return REFUSED
    raise KeyError(op)
