// The schedules of the whole-slide entry points, on the host: what umx_host.hip (host_enqueue: one GPU) and umx_shard.hip (sharded_run:
// one band of a sharded slide) enqueue, as data.  A plan says which rows go up before which tiles, which tiles form a launch group,
// which output rows are final after which patch row, which event orders what across the streams and how the call's buffers are
// cut; the executors in those two files turn its row and tile numbers into addresses and issue the copies, launches and events in
// the plan's order.  No HIP call, no context and no environment variable is read here, so a schedule can be printed, diffed and
// tested without a device (umx_test_slide_plan / umx_test_band_plan, tests/test_pipeline_plan_cpu.py, tools/pipeline_plan_main.hip).
#include "umx_internal.h"

using namespace umx;

// ---- band geometry (the C twin of unmicst_amd/sharding.py: band_partition / owned_rows / needed_image_rows / slab_rows;
// tests/test_abi.py compares the two over a grid of sizes)
namespace umx_geom {

void band(int npr, int world, int rank, int* pa, int* pb) {
    const int active = std::min(world, npr);
    const int base = active ? npr / active : 0, extra = active ? npr % active : 0;
    int start = 0;
    for (int r = 0; r <= rank; ++r) {
        const int n = r < active ? base + (r < extra ? 1 : 0) : 0;
        if (r == rank) { *pa = start; *pb = start + n; }
        start += n;
    }
}

void owned(int pa, int pb, int npr, int sub, int margin, int H, int* y0, int* y1) {
    if (pa >= pb) { *y0 = *y1 = 0; return; }
    *y0 = pa == 0 ? 0 : std::min(H, std::max(0, pa * sub - margin));
    *y1 = pb == npr ? H : std::min(H, std::max(0, pb * sub - margin));
}

void needed(int pa, int pb, int sub, int margin, int patch, int H, int* r0, int* r1) {
    if (pa >= pb) { *r0 = *r1 = 0; return; }
    *r0 = std::max(0, pa * sub - margin);
    *r1 = std::min(H, (pb - 1) * sub + patch - margin);
}

int cut(int pa, int pb, int n, int i) { return pa + (int)(((long long)(pb - pa) * i) / n); }

void slab(int pa, int pb, int npr, int sub, int margin, int H, int n, int i, int* s0, int* s1) {
    if (pa >= pb) { *s0 = *s1 = 0; return; }
    int y0, y1;
    owned(pa, pb, npr, sub, margin, H, &y0, &y1);
    const int a = i == 0 ? y0 : std::min(y1, std::max(y0, cut(pa, pb, n, i) * sub - margin));
    const int b = i == n - 1 ? y1 : std::min(y1, std::max(y0, cut(pa, pb, n, i + 1) * sub - margin));
    *s0 = a;
    *s1 = std::max(a, b);
}

}  // namespace umx_geom

namespace umx {

// the tile grid of an H x W slide (PI2D.setup)
TileGeom geom_of(const umx_hparams& hp, int H, int W) {
    TileGeom g;
    g.H = H; g.W = W;
    g.P = hp.imSize;
    g.margin = hp.imSize / 8;              // int(imSize/8), UnMicst1-5.py:694
    g.sub = g.P - 2 * g.margin;
    g.npr = (H + g.sub - 1) / g.sub;       // ceil, PartitionOfImage.py:49-50
    g.npc = (W + g.sub - 1) / g.sub;
    return g;
}

namespace {
size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }
}  // namespace

// ---- one slide on one GPU.  Slabs = the launch groups of the tile loop (equal groups of <= max_batch tiles, exactly what
// umx_infer_image_dev runs), so that pipelining the transfers does not change a single kernel launch: slab s = tiles
// [T s / S, T (s + 1) / S); its upload covers the image rows its tiles read that are not on the device yet, its download the image
// rows no later patch row touches.
SlidePlan slide_plan(const TileGeom& g, const SlideSpec& sp) {
    SlidePlan p;
    const int H = g.H, T = g.npr * g.npc;
    const size_t plane = (size_t)H * g.W, K = sp.K;
    const size_t in_b = sp.src_bits ? (size_t)(sp.src_bits / 8) : sizeof(double);
    p.pm_b = K * plane * sp.stitch_el;
    p.u8_b = sp.out_u8 ? K * plane : 0;
    p.raw_off = align256(p.pm_b + p.u8_b);
    p.mm_off = align256(p.raw_off + (sp.src_bits ? plane * sp.C_img * in_b : 0));
    p.out_b = p.mm_off + 64 * (size_t)sp.C_img;
    // raw planes into an engine that gathers from them: the float64 image is never made, and not allocated either
    p.image_b = sp.src_bits && sp.raw_gather ? 0 : plane * sp.C_img * sizeof(double);
    p.probs_b = (size_t)T * g.P * g.P * K * sizeof(float);
    const int S = p.S = std::max(1, (T + sp.max_batch - 1) / sp.max_batch);
    // A synchronous call on a slide of one launch group has nothing to overlap: its upload, kernels and download go down ONE
    // stream in order, without the copy streams and the events that hand slabs from one stream to the next (a 1024 x 1024
    // slide is a 1 - 3 ms call).  Submitted calls keep the copy streams: slide i+1's upload rides under slide i's kernels --
    // unless the slide is so small (< 0.6 TFLOP, about 2 ms of kernels: the legacy model's 1024 x 1024 slide is 1 ms) that the
    // cross-stream events cost more than the overlap returns: that call measured 1.03 ms on some boxes and 1.54 on others through
    // the copy streams, 1.02 as one in-order stream.
    const bool single = p.single = S == 1 && (sp.sync_call || sp.tile_flops * (double)T < 0.6e12);
    p.nev = 2 * S + 1;   // upload events [0, S), download events [S, 2 S), the flag's 2 S
    // tile cuts; cut(i) = patch rows COMPLETE after slab i-1 (cut(S) = npr); up(s + 1) = the image rows the tiles of slabs <= s read:
    // up to the last patch row slab s touches (nothing here allocates: a 1024 x 1024 slide is planned on every 1 ms call)
    auto tcut = [&](int i) { return (int)((long long)T * i / S); };
    auto cut = [&](int i) { return tcut(i) / g.npc; };
    auto up = [&](int s) { return s == 0 ? 0 : s == S ? H : std::min(H, ((tcut(s) - 1) / g.npc) * g.sub + g.P - g.margin); };
    const bool raw = sp.src_bits != 0, rescale = raw && sp.rescale;
    const bool convert = raw && !sp.raw_gather;   // raw rows -> float64 rows (im2double [+ rescale]) for an engine that gathers float64
    // A rescale needs the planes' (min, max) before the first tile.  Handed in: the slide goes up slab by slab under the tile
    // kernels like an un-rescaled one.  A synchronous call without one: every slab's upload is enqueued first (pinned pages: DMA),
    // the range found by host threads while the rows cross the bus, and the tiles start on the first slab as soon as that pass is
    // done.  Otherwise (submitted, or the host pass switched off): whole planes first, min / max reduced on the device as the
    // slabs arrive, and only the download is hidden.
    const bool host_range = rescale && !sp.has_range && sp.sync_call && sp.C_img <= 8 && sp.host_range_ok;
    const bool dev_range = rescale && !sp.has_range && !host_range;
    p.steps.reserve(8 * (size_t)S + 8);
    auto step = [&](int kind, int a = 0, int b = 0, int c = 0) { p.steps.push_back(Step{kind, a, b, c}); };
    // the new rows of slab s: uploaded (event s, unless the call is one stream), waited for by the compute stream, reduced or converted
    auto rows = [&](int s, bool upload, bool wait, int then) {
        const int r0 = up(s), r1 = up(s + 1);
        if (r1 <= r0) return;
        if (upload) step(kStepUpload, r0, r1, single ? -1 : s);
        if (wait && !single) step(kStepWaitUpload, s);
        if (then == kStepMinMax || (then == kStepConvert && convert)) step(then, r0, r1);
    };
    if (host_range) {
        for (int s = 0; s < S; ++s) rows(s, true, false, -1);
        step(kStepHostRange);
    }
    if (raw) step(kStepMinMaxInit);
    if (rescale && !dev_range) step(kStepPutRange);
    if (dev_range) {
        for (int s = 0; s < S; ++s) rows(s, true, true, kStepMinMax);
        if (convert) step(kStepConvert, 0, H);
    }
    int y_done = 0;
    for (int s = 0; s < S; ++s) {
        if (!dev_range) rows(s, !host_range, true, kStepConvert);
        if (tcut(s + 1) > tcut(s)) step(kStepTiles, tcut(s), tcut(s + 1));
        // image rows no later tile touches: below the first incomplete patch row
        const int y1 = s == S - 1 ? H : std::max(y_done, std::min(H, cut(s + 1) * g.sub - g.margin));
        if (y1 > y_done && cut(s + 1) > 0) {
            step(kStepStitch, y_done, y1, cut(s + 1));
            if (!single) step(kStepDownloadEvent, S + s);
            step(kStepDownload, y_done, y1);
            y_done = y1;
        }
    }
    // the range flag of the split-precision path rides down behind the last planes (every upload precedes a kernel that precedes a
    // download on the download stream)
    if (!single) step(kStepFlag, 2 * S);
    return p;
}

std::string slide_describe(const SlidePlan& p) {
    static const char* const names[] = {"upload", "wait_upload", "minmax_init", "put_range", "host_range", "minmax", "convert", "tiles",
                                        "stitch", "download_event", "download", "flag"};
    static const int nargs[] = {3, 1, 0, 0, 0, 2, 2, 2, 3, 1, 2, 1};
    char b[256];
    snprintf(b, sizeof b, "slide S %d single %d events %d pm_b %zu u8_b %zu raw_off %zu mm_off %zu image %zu out %zu probs %zu\n", p.S,
             p.single ? 1 : 0, p.nev, p.pm_b, p.u8_b, p.raw_off, p.mm_off, p.image_b, p.out_b, p.probs_b);
    std::string out = b;
    for (const Step& s : p.steps) {
        const int v[3] = {s.a, s.b, s.c};
        out += names[s.kind];
        for (int i = 0; i < nargs[s.kind]; ++i) out += " " + std::to_string(v[i]);
        out += "\n";
    }
    return out;
}

// ---- one band of a sharded slide (the schedule at the head of umx_shard.hip)
BandPlan band_plan(const TileGeom& g, const BandSpec& sp) {
    BandPlan p;
    const int npr = g.npr, npc = g.npc, H = g.H, world = sp.world, rank = sp.rank;
    p.A.resize(world);
    p.B.resize(world);
    int n = std::max(1, sp.nslabs);
    for (int q = 0; q < world; ++q) {
        umx_geom::band(npr, world, q, &p.A[q], &p.B[q]);
        if (p.B[q] > p.A[q]) { p.active.push_back(q); n = std::min(n, p.B[q] - p.A[q]); }
    }
    p.n = n = std::max(1, n);
    const int pa = p.pa = p.A[rank], pb = p.pb = p.B[rank];
    const bool has_prev = pa < pb && pa > 0, has_next = pa < pb && pb < npr;
    p.lo = has_prev ? pa - 1 : pa;   // the previous rank's last patch row sits in front of the band's own
    if (has_next || has_prev) {
        const int me = (int)(std::find(p.active.begin(), p.active.end(), rank) - p.active.begin());
        if (has_next) p.send_peer = p.active[me + 1];
        if (has_prev) p.recv_peer = p.active[me - 1];
    }
    umx_geom::owned(pa, pb, npr, g.sub, g.margin, H, &p.own0, &p.own1);
    p.nev = 6 + 4 * n;   // 0..4: in, last, halo, done, end; 6 + 2 i: slab i; 6 + 2 n + j: staged piece j
    p.probs_b = std::max<size_t>(1, (size_t)std::max(pb - p.lo, 0)) * npc * g.P * g.P * sp.K * sizeof(float);
    // Launch groups.  The next rank waits for this band's LAST patch row, so it is computed first -- but not as a launch group of
    // its own (86 tiles of the 16384-wide slide fill a third of the chip's workgroup slots on the deep layers and still cost every
    // layer a generation): the first group is the band's last F tiles, F = the remainder of the band's tile count over the launch
    // group size (raised by whole groups until it holds the last row), and every later group is a full one, whatever slab it
    // belongs to.  11 patch rows of 86 tiles at 256 per group: 178 + 3 x 256 instead of 86 + 4 x 215 -- the same number of
    // workgroup generations as an unsharded band.  The last band (nobody waits) runs in order.
    const int Bt = std::max(1, sp.max_batch), T0 = pa * npc, T1 = pb * npc;
    int F = 0;
    if (has_next) {
        F = (T1 - T0) % Bt;
        while (F < npc) F += Bt;
        F = std::min(F, T1 - T0);
    }
    p.F = F;
    // staged upload of a raw band: the rows of the band's LAST patch row go first (its tiles run first), then the rows of the slabs
    // from the top; what is up = [band_row0, head) and [tail, band end)
    const int band_end = sp.band_row0 + sp.band_rows;
    int head = sp.band_row0, tail = band_end, nup = 0;
    auto group = [&](int t0, int t1) {
        if (t1 <= t0) return;
        BandPlan::Group G{t0, t1, 0, 0, -1};
        const int pr0 = t0 / npc, pr1 = (t1 - 1) / npc + 1;
        int a = std::max(sp.band_row0, std::max(0, pr0 * g.sub - g.margin));
        int b = std::min(band_end, std::min(H, (pr1 - 1) * g.sub + g.P - g.margin));
        a = std::max(a, head);
        b = std::min(b, tail);
        if (sp.staged && b > a) {
            if (a > head && b < tail) a = head;          // (never with this schedule: keep the two intervals contiguous anyway)
            G.r0 = a;
            G.r1 = b;
            if (a == head) head = b; else tail = a;
            if (sp.own_stream) G.ev = 6 + 2 * n + std::min(nup++, 2 * n - 1);
        }
        p.groups.push_back(G);
    };
    group(T1 - F, T1);
    int done = T0;   // tiles [T0, done) and [T1 - F, T1) are planned
    // the gather buffers hold the largest slab of any rank ([K][mx][W], padded): sized once, so that nothing is reallocated between
    // enqueued collectives
    p.mx_all = 1;
    p.slabs.resize(n);
    for (int i = 0; i < n; ++i) {
        BandPlan::Slab& s = p.slabs[i];
        // the launch groups slab i still lacks: every tile of the patch rows below its last image row (full groups: one may run into the next slab)
        const int need = pa < pb ? std::min(umx_geom::cut(pa, pb, n, i + 1) * npc, T1 - F) : T0;
        s.g0 = (int)p.groups.size();
        while (done < need) {
            const int t1 = std::min(done + Bt, T1 - F);
            group(done, t1);
            done = t1;
        }
        s.g1 = (int)p.groups.size();
        umx_geom::slab(pa, pb, npr, g.sub, g.margin, H, n, i, &s.s0, &s.s1);
        s.ra.resize(world);
        s.rb.resize(world);
        s.mx = 1;
        for (int q = 0; q < world; ++q) {
            umx_geom::slab(p.A[q], p.B[q], npr, g.sub, g.margin, H, n, i, &s.ra[q], &s.rb[q]);
            s.mx = std::max(s.mx, s.rb[q] - s.ra[q]);
        }
        s.ev = 6 + 2 * i;
        p.mx_all = std::max(p.mx_all, s.mx);
    }
    p.send_b = (size_t)sp.K * p.mx_all * g.W * sp.gather_el;
    p.gathered_b = (size_t)world * p.send_b;
    return p;
}

std::string band_describe(const BandPlan& p) {
    char b[256];
    snprintf(b, sizeof b, "band n %d lo %d F %d send %d recv %d mx_all %d events %d probs %zu gathered %zu send_buf %zu\n", p.n,
             p.pb > p.pa ? p.lo : -1 /* (a rank without patch rows: no tile and no stitch reads it) */, p.F, p.send_peer, p.recv_peer, p.mx_all, p.nev, p.probs_b, p.gathered_b, p.send_b);
    std::string out = b;
    auto groups = [&](int g0, int g1) {
        for (int i = g0; i < g1; ++i) {
            const BandPlan::Group& G = p.groups[i];
            if (G.r1 > G.r0) snprintf(b, sizeof b, "group %d %d stage %d %d event %d\n", G.t0, G.t1, G.r0, G.r1, G.ev);
            else snprintf(b, sizeof b, "group %d %d\n", G.t0, G.t1);
            out += b;
        }
    };
    groups(0, p.slabs.empty() ? (int)p.groups.size() : p.slabs[0].g0);
    for (size_t i = 0; i < p.slabs.size(); ++i) {
        const BandPlan::Slab& s = p.slabs[i];
        groups(s.g0, s.g1);
        snprintf(b, sizeof b, "slab %zu rows %d %d mx %d event %d ranks", i, s.s1 > s.s0 ? s.s0 : 0, s.s1 > s.s0 ? s.s1 : 0, s.mx, s.ev);
        out += b;
        for (size_t q = 0; q < s.ra.size(); ++q)
            if (s.rb[q] > s.ra[q]) out += " " + std::to_string(q) + ":" + std::to_string(s.ra[q]) + ":" + std::to_string(s.rb[q]);
        out += "\n";
    }
    return out;
}

}  // namespace umx
