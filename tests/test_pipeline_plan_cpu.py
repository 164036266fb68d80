"""The schedules of the whole-slide entry points as data (slide_plan / band_plan, unmicst_amd/csrc/umx_pipeline.hip) through
umx_test_slide_plan / umx_test_band_plan: no device needed.

Recorded lines.  tests/golden/slide_plan_lines.json and tests/golden/band_plan_lines.json hold, for every case of slide_cases() /
band_cases(), the lines host_enqueue (umx_host.hip) and sharded_run (umx_shard.hip) enqueued before the schedule and the enqueueing
were separated.  They were made from a copy of that commit: the text of the two functions compiled on a CPU against stubs of
everything they call on the device (grow, tiles_range, stitch_rows, put_range, slot_finish, launch_minmax_init / launch_minmax /
launch_raw_convert, umx_plane_range, the transport, hipMemcpyAsync / hipEventRecord / hipStreamWaitEvent / hipEventCreateWithFlags) that
wrote down each call; rows, tiles and event indices were read back from the calls' addresses, byte counts and events, the buffer cuts
and the band's slab rows from the functions' own variables.  (The same stubs under the new executors give call for call the same
trace -- every address, byte count, stream and event -- except that sharded_run now sizes its gather buffers before its first
launch.)  A tile's FLOP figure is the graph builder's (umx_describe), as umx_test_slide_plan takes it.  The lines are kept in a short form
(pack_* below).  The slides' file: "calls", the calls of slide_calls() in order; "heads", the distinct header lines; "texts", the distinct
step texts; "cases", geometry -> the header and the text of every call, in that order (v*k: k times v).  The bands' file: "heads"; "lines", the distinct group and
slab lines; "bodies", the distinct texts as lists of lines and events (unpack_body); "cases", geometry -> "body.header.header" of
every call of band_cases() in order, one entry for its three variants.

Invariants.  Checked from the lines alone, whatever the golden files say: see the two tests at the end."""
import json
import os
import re

import pytest

import helpers
from unmicst_amd import model, sharding, umx

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
OUTS = (("f16", 0, False), ("f32", 1, False), ("u8", 0, True))   # (name, UMX_STITCH_*, out_u8)


def slide_geometries():
    """(name, hp, H, W, max_batch)"""
    small = helpers.small_hps()
    out = [(n, small[n], H, W, mb) for n in ("v2_duo_like", "v2_solo_like", "legacy_k5")
           for H, W in ((70, 45), (5, 7), (31, 200), (113, 61)) for mb in (2, 8, 32)]
    K = model.KNOWN_HP
    out += [("synthetic-256", K["synthetic-256"], 16384, 16384, 256), ("synthetic-256", K["synthetic-256"], 2048, 16384, 256),
            ("nucleiDAPI1-5", K["nucleiDAPI1-5"], 1024, 1024, 4096), ("nucleiDAPI1-5", K["nucleiDAPI1-5"], 16384, 16384, 4096),
            ("nucleiDAPI", K["nucleiDAPI"], 1024, 1024, 1024)]
    return out


def slide_calls():
    """call key -> keyword arguments of umx.slide_plan: source x range handling x host range allowed x raw gather x output"""
    out = {}
    for oname, stitch, u8 in OUTS:
        for sync in (1, 0):
            out["f64 sync%d %s" % (sync, oname)] = dict(src_bits=0, sync_call=sync, stitch=stitch, out_u8=u8)
        for bits in (8, 16):
            for rg in (1, 0):
                # rescale off | on without a range, synchronous | on without a range, submitted | on with a range (both: either way of calling)
                for rescale, has_range, sync in ((0, 0, 1), (0, 0, 0), (1, 0, 1), (1, 0, 0), (1, 1, 1), (1, 1, 0)):
                    for host_ok in (1, 0):
                        out["u%d r%d%d sync%d host%d gather%d %s" % (bits, rescale, has_range, sync, host_ok, rg, oname)] = dict(
                            src_bits=bits, rescale=rescale, has_range=has_range, sync_call=sync, host_range_ok=host_ok, raw_gather=rg,
                            stitch=stitch, out_u8=u8)
    return out


def slide_cases():
    """(geometry key, call key, hp, H, W, max_batch, keyword arguments)"""
    calls = slide_calls()
    for name, hp, H, W, mb in slide_geometries():
        for ck, kw in calls.items():
            yield "%s %dx%d b%d" % (name, H, W, mb), ck, hp, H, W, mb, kw


BAND_VARIANTS = (("device", dict(stitch=0, u8=False, staged=False, own_stream=False)),
                 ("staged own", dict(stitch=0, u8=True, staged=True, own_stream=True)),
                 ("staged same", dict(stitch=0, u8=True, staged=True, own_stream=False)))
BAND_W = 77


def band_cases():
    """(geometry key, call key, hp, H, world, rank, nslabs, max_batch, band_row0, band_rows, variant keywords): the sizes of
    tests/test_sharding_cpu.py::test_library_band_geometry_equals_the_python_schedule; a rank's band = the rows its tiles read"""
    hps = [("v2_duo_like", helpers.small_hps()["v2_duo_like"]), ("nucleiDAPI1-5", model.KNOWN_HP["nucleiDAPI1-5"]),
           ("synthetic-256", model.KNOWN_HP["synthetic-256"])]
    for name, hp in hps:
        m = hp.margin
        sub = hp.imSize - 2 * m
        for H in (5, sub, sub + 1, 3 * sub - 1, 7 * sub + 13, 2048, 16384):
            npr = -(-H // sub)
            for world in (1, 2, 3, 8):
                bands = sharding.band_partition(npr, world)
                for rank in range(world):
                    r0, r1 = sharding.needed_image_rows(bands[rank][0], bands[rank][1], sub, m, hp.imSize, H)
                    for nslabs in (1, 2, 4):
                        for mb in (8, 256):
                            for vname, kw in BAND_VARIANTS:
                                yield ("%s H%d" % (name, H), "w%d r%d n%d b%d %s" % (world, rank, nslabs, mb, vname), hp, H, world, rank,
                                       nslabs, mb, r0, r1 - r0, kw)


@pytest.fixture(scope="module")
def slide_lines():
    flops = {}
    out = []
    for gk, ck, hp, H, W, mb, kw in slide_cases():
        if hp not in flops:
            flops[hp] = umx.describe(hp)["flops_per_tile"]
        out.append((gk, ck, hp, H, W, mb, kw, umx.slide_plan(hp, H, W, mb, hp.nChannels, tile_flops=flops[hp], **kw)))
    return out


@pytest.fixture(scope="module")
def band_lines():
    return [c + (umx.band_plan(c[2], c[3], BAND_W, c[4], c[5], c[6], c[7], c[8], c[9], **c[10]),) for c in band_cases()]


# The golden files hold the lines in a short form, one to one with the text: a header as its numbers, a step as a letter and its
# numbers, a launch group as g<tiles, staged rows>, a slab as s<index, mx, event>;<rank:rows>...
_STEP = {"upload": "u", "wait_upload": "w", "minmax_init": "i", "put_range": "p", "host_range": "h", "minmax": "m", "convert": "c",
         "tiles": "t", "stitch": "s", "download_event": "e", "download": "d", "flag": "f"}


def pack_slide_head(line):
    return " ".join(_HEAD.match(line).groups())


def pack_step(line):
    w = line.split()
    return _STEP[w[0]] + ",".join(w[1:])


def pack_band(lines, rank):
    """(header, group / slab lines, events of the staged groups); a slab's own rows are its entry among the ranks' rows"""
    out, events = [], []
    for line in lines[1:]:
        g = _GROUP.match(line)
        if g:
            out.append("g" + ",".join(v for v in g.groups()[:4] if v is not None))
            if g.group(5) is not None:
                events.append(int(g.group(5)))
            continue
        i, s0, s1, mx, ev = _SLAB.match(line).groups()[:5]
        ranks = _SLAB.match(line).group(6).split()
        own = [r.split(":")[1:] for r in ranks if r.split(":")[0] == str(rank)]
        assert [s0, s1] == (own[0] if own else ["0", "0"]), line
        out.append("s" + ",".join((i, mx, ev)) + "".join(";" + r for r in ranks))
    return " ".join(_BAND.match(lines[0]).groups()), out, events


def unpack_body(want, body, variant):
    """the lines and events a body of the golden file stands for: it is the one the "staged own" call recorded, a token = a line
    (or i-j, the lines i..j) and, where the event differs from the staged group's before, @event; the call's two other variants recorded the same lines without
    the staged rows (device band) or with no event (same stream), which the packing checked against the recording case by case"""
    out, events = [], []
    for tok in body.split():
        i, _, e = tok.partition("@")
        i, _, j = i.partition("-")
        for k in range(int(i), int(j or i) + 1):   # (i-j: the lines i..j)
            line = want["lines"][k]
            if line[0] == "g" and line.count(",") == 3:
                events.append(int(e) if e else events[-1])
                if variant == "device":
                    line = ",".join(line.split(",")[:2])
            out.append(line)
    return out, [] if variant == "device" else [-1] * len(events) if variant == "staged same" else events


def test_slide_plans_are_the_recorded_ones(slide_lines):
    with open(os.path.join(GOLDEN, "slide_plan_lines.json")) as f:
        want = json.load(f)
    assert want["calls"] == list(slide_calls())
    def runs(text):   # "7*3 9" -> 7, 7, 7, 9
        for tok in text.split():
            v, _, k = tok.partition("*")
            for _ in range(int(k or 1)):
                yield int(v)
    at = {gk: zip(runs(v["heads"]), runs(v["texts"])) for gk, v in want["cases"].items()}
    for gk, ck, hp, H, W, mb, kw, lines in slide_lines:
        h, t = next(at[gk])
        assert pack_slide_head(lines[0]) == want["heads"][h], (gk, ck)
        assert [pack_step(ln) for ln in lines[1:]] == want["texts"][t].split(), (gk, ck)
    assert len(slide_lines) > 6000 and all(next(it, None) is None for it in at.values())


def test_band_plans_are_the_recorded_ones(band_lines):
    with open(os.path.join(GOLDEN, "band_plan_lines.json")) as f:
        want = json.load(f)
    at = {gk: iter(v.split()) for gk, v in want["cases"].items()}
    for c in band_lines:
        variant = [v for v, _ in BAND_VARIANTS if c[1].endswith(v)][0]
        if variant == BAND_VARIANTS[0][0]:   # one entry for the three variants of a call: body.header of the device band.header of the staged ones
            body, h_dev, h_staged = map(int, next(at[c[0]]).split("."))
        head, lines, events = pack_band(c[-1], c[5])
        assert head == want["heads"][h_dev if variant == "device" else h_staged], c[:2]
        assert (lines, events) == unpack_body(want, want["bodies"][body], variant), c[:2]
    assert len(band_lines) > 5000 and all(next(it, None) is None for it in at.values())


def test_the_flop_figure_may_come_from_the_graph():
    """tile_flops <= 0: the entry builds the graph itself -- the same schedule as with umx_describe's figure handed in"""
    hp = model.KNOWN_HP["nucleiDAPI"]
    kw = dict(src_bits=16, rescale=1, sync_call=0, out_u8=True, raw_gather=1)
    assert umx.slide_plan(hp, 1024, 1024, 1024, 1, **kw) == umx.slide_plan(hp, 1024, 1024, 1024, 1,
                                                                            tile_flops=umx.describe(hp)["flops_per_tile"], **kw)


_HEAD = re.compile(r"^slide S (\d+) single ([01]) events (\d+) pm_b (\d+) u8_b (\d+) raw_off (\d+) mm_off (\d+) image (\d+) out (\d+) probs (\d+)$")


def _covered(iv, lo, hi):
    """do the intervals `iv` cover [lo, hi)?"""
    at = lo
    for a, b in sorted(iv):
        if a > at:
            break
        at = max(at, b)
    return at >= hi or hi <= lo


def check_slide(hp, H, W, mb, kw, lines):
    P, margin, K, C = hp.imSize, hp.margin, hp.nClasses, hp.nChannels
    sub = P - 2 * margin
    npr, npc = -(-H // sub), -(-W // sub)
    T = npr * npc
    bits, rescale = kw["src_bits"], bool(kw["src_bits"] and kw.get("rescale"))
    converts = bool(bits and not kw.get("raw_gather"))
    S, single, nev, pm_b, u8_b, raw_off, mm_off, image_b, out_b, probs_b = map(int, _HEAD.match(lines[0]).groups())
    # the buffers: [stitched planes | uint8 planes | raw planes | (min, max) words] without overlap, the two cuts on 256 bytes
    plane = H * W
    assert pm_b >= K * plane * (4 if kw["stitch"] == 1 else 2) and u8_b >= (K * plane if kw["out_u8"] else 0)
    assert raw_off % 256 == 0 and mm_off % 256 == 0
    assert raw_off >= pm_b + u8_b and mm_off >= raw_off + (plane * C * bits // 8) and out_b >= mm_off + 64 * C
    assert image_b >= (0 if bits and kw.get("raw_gather") else plane * C * 8) and probs_b >= T * P * P * K * 4
    assert S == max(1, -(-T // mb))
    steps = [(ln.split()[0], [int(v) for v in ln.split()[1:]]) for ln in lines[1:]]
    up, waited, recorded, converted, reduced, tiles, stitched, down = [], set(), set(), [], [], [], [], []
    have_range = False
    up_event = {}           # event -> rows of its upload
    dn_event_after = None   # the download event behind the last stitch
    for i, (kind, a) in enumerate(steps):
        if kind == "upload":
            assert a[0] == (up[-1][1] if up else 0) and a[1] > a[0], "rows go up once, in order"
            up.append((a[0], a[1]))
            assert (a[2] == -1) == bool(single)
            if a[2] >= 0:
                assert a[2] < nev and a[2] not in recorded
                recorded.add(a[2])
                up_event[a[2]] = (a[0], a[1])
        elif kind == "wait_upload":
            assert not single and a[0] in up_event, "an event is recorded before it is waited for"
            waited.add(a[0])
        elif kind == "minmax_init":
            assert bits and not reduced and not have_range
        elif kind == "host_range":
            assert rescale and not kw.get("has_range") and kw["sync_call"] and kw.get("host_range_ok")
            assert _covered(up, 0, H), "the uploads are enqueued ahead of the host pass"
        elif kind == "put_range":
            assert rescale and (kw.get("has_range") or ("host_range", []) in steps[:i]) and ("minmax_init", []) in steps[:i]
            have_range = True
        elif kind in ("minmax", "convert"):
            assert bits and (rescale if kind == "minmax" else converts)
            assert ("minmax_init", []) in steps[:i]
            assert _covered(up, a[0], a[1]), "reduced / converted rows are up"
            assert single or all(e in waited for e, r in up_event.items() if r[0] < a[1] and r[1] > a[0]), "... and waited for"
            if kind == "convert":
                assert not rescale or have_range or _covered(reduced, 0, H), "a rescaling conversion has its range"
            (reduced if kind == "minmax" else converted).append((a[0], a[1]))
        elif kind == "tiles":
            assert a[0] == (tiles[-1][1] if tiles else 0) and 0 < a[1] - a[0] <= mb, "tiles run once, in groups of <= max_batch"
            tiles.append((a[0], a[1]))
            pr1 = (a[1] - 1) // npc + 1
            need = min(H, (pr1 - 1) * sub + P - margin)
            assert _covered(up, 0, need), "a tile's rows are up"
            assert single or all(e in waited for e, r in up_event.items() if r[0] < need), "... and waited for"
            assert not converts or _covered(converted, 0, need), "... and converted"
            if rescale:
                assert have_range or (sorted(reduced) == up and _covered(reduced, 0, H)), "a rescale has its range before the first tile"
        elif kind == "stitch":
            y0, y1, pr1 = a
            assert y0 == (stitched[-1][1] if stitched else 0) and y1 > y0, "output rows are stitched once, in order"
            assert y1 <= pr1 * sub - margin or pr1 == npr, "stitched rows are final"
            assert tiles and tiles[-1][1] >= min(T, pr1 * npc), "the patch rows a stitch reads have run"
            stitched.append((y0, y1))
            dn_event_after = None
        elif kind == "download_event":
            assert not single and steps[i - 1][0] == "stitch" and S <= a[0] < nev and a[0] not in recorded
            recorded.add(a[0])
            dn_event_after = a[0]
        elif kind == "download":
            assert stitched and (a[0], a[1]) == stitched[-1] and len(down) == len(stitched) - 1, "every stitched slab goes down once"
            assert single or dn_event_after is not None, "the download stream waits for the stitch"
            down.append((a[0], a[1]))
        elif kind == "flag":
            assert not single and i == len(steps) - 1 and a[0] < nev and a[0] not in recorded
        else:
            raise AssertionError(kind)
    assert up and up[-1][1] == H and tiles[-1][1] == T and len(tiles) == S
    assert stitched[-1][1] == H and down == stitched
    assert single or steps[-1][0] == "flag"
    assert not bits or ("minmax_init", []) in steps
    assert not converts or (sorted(converted) == up or converted == [(0, H)]), "every row is converted once"
    if single:
        assert S == 1 and not recorded


def test_slide_schedules_are_sound(slide_lines):
    for gk, ck, hp, H, W, mb, kw, lines in slide_lines:
        try:
            check_slide(hp, H, W, mb, kw, lines)
        except AssertionError as e:
            raise AssertionError("%s | %s: %s" % (gk, ck, e))
    # the 0.6 TFLOP rule: a submitted 1024 x 1024 slide of the legacy model runs as one in-order stream
    legacy = [ln for gk, ck, *_, ln in slide_lines if gk.startswith("nucleiDAPI 1024") and ck == "u16 r10 sync0 host1 gather1 u8"]
    assert len(legacy) == 1 and " single 1 " in legacy[0][0]
    big = [ln for gk, ck, *_, ln in slide_lines if gk.startswith("synthetic-256 16384") and ck == "u16 r10 sync0 host1 gather1 u8"]
    assert len(big) == 1 and " single 0 " in big[0][0]


_BAND = re.compile(r"^band n (\d+) lo (-?\d+) F (\d+) send (-?\d+) recv (-?\d+) mx_all (\d+) events (\d+) probs (\d+) gathered (\d+) send_buf (\d+)$")
_GROUP = re.compile(r"^group (\d+) (\d+)(?: stage (\d+) (\d+) event (-?\d+))?$")
_SLAB = re.compile(r"^slab (\d+) rows (\d+) (\d+) mx (\d+) event (\d+) ranks((?: \d+:\d+:\d+)*)$")


def check_band(hp, H, world, rank, nslabs, mb, row0, rows, kw, lines):
    P, margin, K = hp.imSize, hp.margin, hp.nClasses
    sub = P - 2 * margin
    npr, npc = -(-H // sub), -(-BAND_W // sub)
    bands = sharding.band_partition(npr, world)
    active = [q for q, (a, b) in enumerate(bands) if b > a]
    pa, pb = bands[rank]
    n, lo, F, send, recv, mx_all, nev, probs_b, gathered_b, send_b = map(int, _BAND.match(lines[0]).groups())
    assert n == max(1, min(nslabs, min(b - a for a, b in bands if b > a)))
    # halo peers: the neighbouring active ranks
    me = active.index(rank) if rank in active else None
    assert send == (active[me + 1] if me is not None and me + 1 < len(active) else -1)
    assert recv == (active[me - 1] if me else -1)
    assert lo == (-1 if pa >= pb else pa - 1 if recv >= 0 else pa)
    el = 1 if kw["u8"] else 4 if kw["stitch"] == 1 else 2
    assert send_b >= K * mx_all * BAND_W * el and gathered_b >= world * send_b and probs_b >= (pb - lo if pa < pb else 0) * npc * P * P * K * 4
    groups, staged, events, slabs = [], [], set(), []
    for ln in lines[1:]:
        g = _GROUP.match(ln)
        if g:
            t0, t1 = int(g.group(1)), int(g.group(2))
            assert t1 > t0
            if g.group(3) is not None:
                a, b, e = int(g.group(3)), int(g.group(4)), int(g.group(5))
                assert kw["staged"] and row0 <= a < b <= row0 + rows, "staged rows lie inside the band"
                assert all(b <= x or y <= a for x, y in staged), "... and go up once"
                staged.append((a, b))
                assert (e >= 0) == kw["own_stream"] and e < nev
                if e >= 0:
                    assert e >= 6 + 2 * n and (e not in events or e == nev - 1)
                    events.add(e)
            if kw["staged"]:   # what is up covers the rows the group reads
                r0, r1 = sharding.needed_image_rows(t0 // npc, (t1 - 1) // npc + 1, sub, margin, P, H)
                at = r0
                for a, b in sorted(staged):
                    if a <= at:
                        at = max(at, b)
                assert at >= r1, "a group's rows are staged before it"
            groups.append((t0, t1))
            continue
        s = _SLAB.match(ln)
        assert s, ln
        i, s0, s1, mx, ev = (int(v) for v in s.groups()[:5])
        ranks = {int(q): (int(a), int(b)) for q, a, b in (r.split(":") for r in s.group(6).split())}
        assert i == len(slabs) and ev == 6 + 2 * i < nev and 1 <= mx <= mx_all
        assert all(b - a <= mx for a, b in ranks.values())
        assert ranks.get(rank, (0, 0)) == (s0, s1)
        if s1 > s0:   # every tile of the patch rows that touch the slab's rows has been launched
            hi = min(pb, -(-(s1 + margin) // sub)) if s1 < H else pb
            done = sorted(groups)
            assert all(any(a <= t < b for a, b in done) for t in range(pa * npc, hi * npc, max(1, npc // 2))) and \
                any(a < hi * npc <= b for a, b in done), "a slab's tiles run before its stitch"
        slabs.append(ranks)
    # the launch groups: the band's tiles once; the first one the band's last F tiles, with the whole last patch row for a next rank
    assert sorted(groups) == groups[1:] + groups[:1] if F and len(groups) > 1 else sorted(groups) == groups
    flat = sorted(groups)
    if pa < pb:
        assert flat[0][0] == pa * npc and flat[-1][1] == pb * npc and all(flat[j][1] == flat[j + 1][0] for j in range(len(flat) - 1))
        if send >= 0:
            assert groups[0] == (pb * npc - F, pb * npc) and F >= min(npc, (pb - pa) * npc)
        else:
            assert F == 0
        assert all(b - a <= mb for a, b in groups[1:]) and (F == 0 or F < mb + npc)
    else:
        assert not groups and F == 0
    if not kw["staged"]:
        assert not staged
    # the slabs: every rank's owned rows, cut into n pieces in order
    assert len(slabs) == n
    for q, (a, b) in enumerate(bands):
        y0, y1 = sharding.owned_rows(a, b, npr, sub, margin, H)
        pieces = [s[q] for s in slabs if q in s]
        at = y0
        for r0, r1 in pieces:
            assert r0 == at and r1 > r0
            at = r1
        assert at == y1, "the slabs partition rank %d's rows" % q


def test_band_schedules_are_sound(band_lines):
    for c in band_lines:
        try:
            check_band(*c[2:])
        except AssertionError as e:
            raise AssertionError("%s | %s: %s" % (c[0], c[1], e))
