// Whole-slide inference sharded over the GPUs of one node INSIDE the library: one process per GPU, RCCL over xGMI.
// (SURVEY.md section 8(b) lists umx_infer_image_sharded in the C ABI; the reference itself is single-device,
// UnMicst1-5.py:769.)  The schedule is the one unmicst_amd/sharding.py runs through torch.distributed -- and which the
// gloo tests (tests/test_sharding_cpu.py, 2 and 3 ranks) and the 2/3-ranks-on-one-GPU test check bit for bit against a
// single process:
//   * patch rows are split into contiguous bands, one per rank; a rank holds only the image rows its tiles read;
//   * the LAST patch row of a band is computed first and sent to the next rank (ncclSend / ncclRecv on a communication
//     stream, hidden under the rest of the band's tiles): the 2*margin image rows below a band boundary are covered by
//     patch rows pb-1 and pb;
//   * the band is computed in slabs of patch rows; as soon as a slab's image rows are final they are stitched (tiles visited
//     in ascending global index: bit-identical to a one-GPU run) and all-gathered (ncclAllGather on equal-size padded slabs)
//     while the next slab's tiles run; the gathered rows are scattered into the [K, H, W] result every rank ends up with.
// RCCL is not linked: the few nccl* entry points are resolved with dlopen / dlsym when a context is given a communicator,
// from the librccl the process already holds (a Python caller has torch's) or from ROCm's.
#include <dlfcn.h>
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstring>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "umx_internal.h"

using namespace umx;

namespace {

struct Rccl {
    void* h = nullptr;
    decltype(&ncclGetUniqueId) GetUniqueId = nullptr;
    decltype(&ncclCommInitRank) CommInitRank = nullptr;
    decltype(&ncclCommDestroy) CommDestroy = nullptr;
    decltype(&ncclSend) Send = nullptr;
    decltype(&ncclRecv) Recv = nullptr;
    decltype(&ncclAllGather) AllGather = nullptr;
    decltype(&ncclGroupStart) GroupStart = nullptr;
    decltype(&ncclGroupEnd) GroupEnd = nullptr;
    decltype(&ncclGetErrorString) GetErrorString = nullptr;
    decltype(&ncclCommGetAsyncError) CommGetAsyncError = nullptr;   // (optional: failure detection)
    decltype(&ncclCommAbort) CommAbort = nullptr;
    std::string err;
};

Rccl* rccl() {
    static Rccl r;
    static std::once_flag once;
    std::call_once(once, [] {
        const char* names[] = {"librccl.so.1", "librccl.so"};
        for (const char* n : names)
            if (!r.h) r.h = dlopen(n, RTLD_NOW | RTLD_NOLOAD);          // the copy the process already uses (torch's)
        if (!r.h)
            if (const char* e = getenv("UMX_RCCL_PATH")) r.h = dlopen(e, RTLD_NOW | RTLD_GLOBAL);
        for (const char* n : names)
            if (!r.h) r.h = dlopen(n, RTLD_NOW | RTLD_GLOBAL);
        if (!r.h) r.h = dlopen("/opt/rocm/lib/librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
        if (!r.h) { r.err = std::string("cannot load librccl: ") + (dlerror() ? dlerror() : "?"); return; }
#define UMX_SYM(f) r.f = reinterpret_cast<decltype(r.f)>(dlsym(r.h, "nccl" #f)); if (!r.f) r.err = "librccl lacks nccl" #f;
        UMX_SYM(GetUniqueId) UMX_SYM(CommInitRank) UMX_SYM(CommDestroy) UMX_SYM(Send) UMX_SYM(Recv) UMX_SYM(AllGather)
        UMX_SYM(GroupStart) UMX_SYM(GroupEnd) UMX_SYM(GetErrorString)
#undef UMX_SYM
        r.CommGetAsyncError = reinterpret_cast<decltype(r.CommGetAsyncError)>(dlsym(r.h, "ncclCommGetAsyncError"));
        r.CommAbort = reinterpret_cast<decltype(r.CommAbort)>(dlsym(r.h, "ncclCommAbort"));
    });
    return &r;
}

}  // namespace

// The sharded state of one context (umx_ctx::shard): what umx_shard_init made, owned by the context until umx_shard_fini /
// umx_destroy.  Its buffers are read on the communication and download streams: a grow drains the whole device before it frees one.
struct umx::Shard {
    ncclComm_t comm = nullptr;
    // Every inter-rank byte of the schedule below goes through this table -- the umx_shard_transport of include/umx.h.  umx_shard_init
    // fills it with RCCL (stream-ordered ncclSend / ncclRecv / ncclAllGather on the context's communicator); umx_shard_init_transport
    // takes the caller's: how the band / halo / scatter code runs in worlds of 2 and 3 on ONE GPU in the test-suite (RCCL refuses two
    // ranks on a device), with the messages staged through host memory.
    umx_shard_transport tp = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    bool failed = false;          // a transport call failed, a peer's failure was seen or a wait timed out: the communicator (RCCL) is
                                  // aborted and every later call on this context is refused until umx_shard_fini + a new umx_shard_init
    std::string tp_err;           // message of the last failed transport call (RCCL: ncclGetErrorString)
    int rank = 0, world = 1;
    hipStream_t comm_stream = nullptr;
    std::vector<hipEvent_t> events[2];   // per call slot (the raw entry keeps two slides in flight; the device entry uses slot 0)
    // probs is written and read in the order of the context's stream only; per slot, the communication stream of slide i may still
    // read the others under slide i+1's tiles
    void* probs = nullptr;       size_t probs_cap = 0;
    void* gathered[2] = {};      size_t gathered_cap[2] = {};
    void* full_u8[2] = {};       size_t full_u8_cap[2] = {};
    std::vector<void*> send[2];  std::vector<size_t> send_cap[2];

    ~Shard() {
        if (comm && rccl()->CommDestroy) rccl()->CommDestroy(comm);
        if (comm_stream) hipStreamDestroy(comm_stream);
        for (auto& ev : events) for (auto e : ev) hipEventDestroy(e);
    }   // (the buffers live in the context's arena: shard_release)
};

namespace {

#define S_NCCL(ctx, expr)                                                                                   \
    do {                                                                                                    \
        ncclResult_t r__ = (expr);                                                                          \
        if (r__ != ncclSuccess) return fail(ctx, UMX_ERR_HIP, "%s failed: %s", #expr, rccl()->GetErrorString(r__)); \
    } while (0)

// After a failure the collectives already enqueued can wait for peers that will never arrive: ncclCommAbort makes them return, so that
// the streams drain and the peers' own waits see an error instead of blocking (they poll ncclCommGetAsyncError, shard_wait below).
void shard_abort(Shard& s) {
    s.failed = true;
    if (s.comm && rccl()->CommAbort) { rccl()->CommAbort(s.comm); s.comm = nullptr; }
}

int rccl_fail(Shard* s, ncclResult_t r, const char* what) {
    s->tp_err = std::string(what) + " failed: " + rccl()->GetErrorString(r);
    return 1;
}
int rccl_send(void* user, const void* dev, size_t bytes, int peer, void* stream) {
    Shard* s = static_cast<Shard*>(user);
    const ncclResult_t r = rccl()->Send(dev, bytes, ncclUint8, peer, s->comm, (hipStream_t)stream);
    return r == ncclSuccess ? 0 : rccl_fail(s, r, "ncclSend");
}
int rccl_recv(void* user, void* dev, size_t bytes, int peer, void* stream) {
    Shard* s = static_cast<Shard*>(user);
    const ncclResult_t r = rccl()->Recv(dev, bytes, ncclUint8, peer, s->comm, (hipStream_t)stream);
    return r == ncclSuccess ? 0 : rccl_fail(s, r, "ncclRecv");
}
int rccl_all_gather(void* user, const void* send_dev, void* recv_dev, size_t bytes_per_rank, void* stream) {
    Shard* s = static_cast<Shard*>(user);
    const ncclResult_t r = rccl()->AllGather(send_dev, recv_dev, bytes_per_rank, ncclUint8, s->comm, (hipStream_t)stream);
    return r == ncclSuccess ? 0 : rccl_fail(s, r, "ncclAllGather");
}
int rccl_group_start(void* user) {
    const ncclResult_t r = rccl()->GroupStart();
    return r == ncclSuccess ? 0 : rccl_fail(static_cast<Shard*>(user), r, "ncclGroupStart");
}
int rccl_group_end(void* user) {
    const ncclResult_t r = rccl()->GroupEnd();
    return r == ncclSuccess ? 0 : rccl_fail(static_cast<Shard*>(user), r, "ncclGroupEnd");
}

// the end of umx_shard_init / umx_shard_init_transport: the state goes to the context only when it is complete
int publish(umx_ctx* ctx, std::unique_ptr<Shard> s, int rank, int world) {
    s->rank = rank;
    s->world = world;
    HIP_TRY(ctx, hipStreamCreateWithFlags(&s->comm_stream, hipStreamNonBlocking));
    ctx->shard = s.release();
    return UMX_OK;
}

}  // namespace

void umx::shard_release(umx_ctx* ctx) {
    std::vector<void*> bufs;   // freed behind the communicator, its stream and events, as ever
    if (Shard* s = ctx->shard) {
        bufs = {s->probs, s->gathered[0], s->gathered[1], s->full_u8[0], s->full_u8[1]};
        for (auto& v : s->send) bufs.insert(bufs.end(), v.begin(), v.end());
    }
    delete ctx->shard;
    ctx->shard = nullptr;
    for (void* d : bufs) if (d) (void)arena_release(&ctx->mem, d);
}

hipStream_t umx::shard_stream(const umx_ctx* ctx) { return ctx->shard ? ctx->shard->comm_stream : nullptr; }

extern "C" {

int umx_shard_unique_id(umx_unique_id* out) {
    if (!out) return fail(nullptr, UMX_ERR_INVALID, "out is NULL");
    Rccl* r = rccl();
    if (!r->err.empty()) return fail(nullptr, UMX_ERR_HIP, "%s", r->err.c_str());
    static_assert(sizeof(umx_unique_id) == sizeof(ncclUniqueId), "umx_unique_id must be ncclUniqueId-sized");
    ncclUniqueId id;
    ncclResult_t rc = r->GetUniqueId(&id);
    if (rc != ncclSuccess) return fail(nullptr, UMX_ERR_HIP, "%s", r->GetErrorString(rc));
    memcpy(out, &id, sizeof id);
    return UMX_OK;
}

int umx_shard_init(umx_ctx* ctx, const umx_unique_id* id, int rank, int world) {
    if (!ctx || !id) return fail(ctx, UMX_ERR_INVALID, "ctx / id is NULL");
    if (world < 1 || rank < 0 || rank >= world) return fail(ctx, UMX_ERR_INVALID, "bad rank / world");
    Rccl* r = rccl();
    if (!r->err.empty()) return fail(ctx, UMX_ERR_HIP, "%s", r->err.c_str());
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    shard_release(ctx);
    auto s = std::make_unique<Shard>();
    ncclUniqueId nid;
    memcpy(&nid, id, sizeof nid);
    S_NCCL(ctx, r->CommInitRank(&s->comm, world, nid, rank));
    s->tp = umx_shard_transport{s.get(), rccl_send, rccl_recv, rccl_all_gather, rccl_group_start, rccl_group_end};
    return publish(ctx, std::move(s), rank, world);
}

int umx_shard_init_transport(umx_ctx* ctx, const umx_shard_transport* tp, int rank, int world) {
    if (!ctx || !tp) return fail(ctx, UMX_ERR_INVALID, "ctx / transport is NULL");
    if (!tp->send || !tp->recv || !tp->all_gather) return fail(ctx, UMX_ERR_INVALID, "the transport lacks send / recv / all_gather");
    if (world < 1 || rank < 0 || rank >= world) return fail(ctx, UMX_ERR_INVALID, "bad rank / world");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    shard_release(ctx);
    auto s = std::make_unique<Shard>();
    s->tp = *tp;
    return publish(ctx, std::move(s), rank, world);
}

int umx_shard_fini(umx_ctx* ctx) {
    if (ctx) shard_release(ctx);
    return UMX_OK;
}

int umx_shard_plan(const umx_hparams* hpp, int H, int W, int rank, int world, int nslabs, int slab, int* patch_row0,
                   int* patch_row1, int* need_row0, int* need_row1, int* own_row0, int* own_row1, int* slab_row0,
                   int* slab_row1, int* nslabs_used) {
    if (!hpp || hpp->imSize < 8 || H < 1 || W < 1 || world < 1 || rank < 0 || rank >= world)
        return fail(nullptr, UMX_ERR_INVALID, "bad hp / H / W / rank / world");
    const umx_hparams hp = *hpp;
    const int margin = hp.imSize / 8, sub = hp.imSize - 2 * margin;
    const int npr = (H + sub - 1) / sub;           // PI2D.setup, PartitionOfImage.py:49
    int pa, pb;
    umx_geom::band(npr, world, rank, &pa, &pb);
    int n = std::max(1, nslabs);
    for (int r = 0; r < world; ++r) {
        int a, b;
        umx_geom::band(npr, world, r, &a, &b);
        if (b > a) n = std::min(n, b - a);
    }
    n = std::max(1, n);
    if (slab < 0 || slab >= n) return fail(nullptr, UMX_ERR_INVALID, "slab index out of range");
    int v0, v1;
    if (patch_row0) *patch_row0 = pa;
    if (patch_row1) *patch_row1 = pb;
    umx_geom::needed(pa, pb, sub, margin, hp.imSize, H, &v0, &v1);
    if (need_row0) *need_row0 = v0;
    if (need_row1) *need_row1 = v1;
    umx_geom::owned(pa, pb, npr, sub, margin, H, &v0, &v1);
    if (own_row0) *own_row0 = v0;
    if (own_row1) *own_row1 = v1;
    umx_geom::slab(pa, pb, npr, sub, margin, H, n, slab, &v0, &v1);
    if (slab_row0) *slab_row0 = v0;
    if (slab_row1) *slab_row1 = v1;
    if (nslabs_used) *nslabs_used = n;
    return UMX_OK;
}

// The schedule of one rank's band on the host alone (no device, no communicator): band_describe of the plan sharded_run would
// execute -- stitch: UMX_STITCH_*; u8: the uint8 result is gathered; staged / own_stream: a host band goes up piece by piece, on a
// stream of its own.  *needed: bytes of the text with its terminator; UMX_ERR_INVALID where cap is smaller.
int umx_test_band_plan(const umx_hparams* hp, int H, int W, int world, int rank, int nslabs, int max_batch, int band_row0, int band_rows,
                       int stitch, int u8, int staged, int own_stream, char* text, size_t cap, size_t* needed) {
    if (!hp || !needed || (!text && cap)) return fail(nullptr, UMX_ERR_INVALID, "umx_test_band_plan: null argument");
    *needed = 0;
    std::string why;
    if (const int rc = check_hp(hp, &why)) return fail(nullptr, rc, "%s", why.c_str());
    if (H < 1 || W < 1 || world < 1 || rank < 0 || rank >= world || max_batch < 1 || band_row0 < 0 || band_rows < 0 || band_row0 + band_rows > H)
        return fail(nullptr, UMX_ERR_INVALID, "umx_test_band_plan: bad H / W / rank / world / max_batch / band");
    BandSpec sp;
    sp.world = world;
    sp.rank = rank;
    sp.nslabs = nslabs;
    sp.max_batch = max_batch;
    sp.band_row0 = band_row0;
    sp.band_rows = band_rows;
    sp.K = hp->nClasses;
    sp.gather_el = u8 ? 1 : stitch == UMX_STITCH_FP32 ? 4 : 2;
    sp.staged = staged != 0;
    sp.own_stream = own_stream != 0;
    const std::string out = band_describe(band_plan(geom_of(*hp, H, W), sp));
    *needed = out.size() + 1;
    if (cap < *needed) return fail(nullptr, UMX_ERR_INVALID, "umx_test_band_plan: the text takes %zu bytes", *needed);
    memcpy(text, out.c_str(), *needed);
    return UMX_OK;
}

}  // extern "C"

namespace {

// What one call of the schedule reads and writes.  Source: a float64 band on the device, or a raw integer band (the tile gather
// converts, umx_conv_f16.hip gather_split_kernel) that is still on its way up -- then `band_host` is staged piece by piece on
// `up_s` ahead of the tiles that read it.  Result: the stitched slabs as they are (fp16 / fp32), or cast to the drivers' uint8
// (UnMicst1-5.py:848-854 at the identity grid) before they are gathered; optionally this rank's own rows also go down to
// the host on `dn_s` as soon as their slab is final.
struct RunIO {
    const double* band_f64 = nullptr;
    const void* raw_dev = nullptr;
    int raw_bits = 0;
    const unsigned* mm = nullptr;          // raw source with intensity rescale: the planes' (min, max) words, 16 apart
    const void* band_host = nullptr;       // raw source: host rows to stage into raw_dev (NULL: raw_dev is complete)
    hipStream_t up_s = nullptr, dn_s = nullptr;
    int u8 = 0;
    void* out_full = nullptr;              // [K, H, W] on the device, every rank
    uint8_t* own_host = nullptr;           // u8 only: [K, own rows, W] on the host, this rank's rows
    int slot = 0;
    bool join = true;                      // the context's stream waits for the gathers at the end (device entry)
    hipEvent_t* ev_gathered = nullptr;     // out: recorded on the communication stream behind the last scatter copy
    hipEvent_t* ev_cs_end = nullptr;       // out: recorded on the context's stream behind the call's last kernel
};

// Every check of a sharded call, before anything is enqueued (the range kernels below index the band unchecked; the band plan is
// host geometry): the context must hold a world that has not failed, and the band must lie in the image, be there and cover the
// image rows its patch rows read.  The entries check the rest of their arguments with check_image first.
int shard_check(umx_ctx* ctx, const void* band, int H, int W, int band_row0, int band_rows) {
    const Shard* s = ctx->shard;
    if (!s) return fail(ctx, UMX_ERR_INVALID, "call umx_shard_init (or umx_shard_init_transport) on this context first");
    if (s->failed) return fail(ctx, UMX_ERR_INVALID, "the sharded world of this context failed earlier (its communicator was aborted): umx_shard_fini, then umx_shard_init in every rank");
    if (band_rows < 0 || band_row0 < 0 || band_row0 + band_rows > H) return fail(ctx, UMX_ERR_INVALID, "sharded entry: band outside the image");
    const TileGeom g = geom_of(ctx->hp, H, W);
    int pa, pb, need0, need1;
    umx_geom::band(g.npr, s->world, s->rank, &pa, &pb);
    if (pa >= pb) return UMX_OK;   // (a rank without patch rows reads no band)
    if (!band) return fail(ctx, UMX_ERR_INVALID, "sharded entry: NULL band");
    umx_geom::needed(pa, pb, g.sub, g.margin, g.P, H, &need0, &need1);
    if (band_row0 > need0 || band_row0 + band_rows < need1)
        return fail(ctx, UMX_ERR_INVALID, "sharded entry: the band does not cover the image rows its patch rows read (umx_shard_plan: need_row0 .. need_row1)");
    return UMX_OK;
}

// An error after shard_check: gathers and scatter copies into the caller's `out_full` may already sit on the communication stream --
// abort the world (peers must not wait for this rank's collectives, and ours must not wait for theirs) and drain that stream and the
// context's, whose kernels feed it, before the caller gets its buffers back; the message survives.
int shard_drain(umx_ctx* ctx, int rc) {
    if (!rc) return rc;
    const std::string msg = ctx->err;
    shard_abort(*ctx->shard);
    hipStreamSynchronize(ctx->stream);
    if (ctx->shard->comm_stream) hipStreamSynchronize(ctx->shard->comm_stream);
    ctx->err = msg;
    return rc;
}

// The executor of a band's schedule (band_plan, umx_pipeline.hip): the buffers sized from the plan, the events, then its launch groups
// and slabs in order on the context's stream `cs`, with the halo exchange, the gathers and the scatter copies on the communication
// stream `ms`.
int sharded_run(umx_ctx* ctx, const RunIO& io, int C_img, int H, int W, int band_row0, int band_rows, double mean, double stdv, int mode,
                int stitch, int nslabs) {
    Shard& s = *ctx->shard;
    const umx_shard_transport& tp = s.tp;
#define S_TP(ctx, expr)                                                                                       \
    do {                                                                                                      \
        s.tp_err.clear();                                                                                     \
        if ((expr) != 0) return fail(ctx, UMX_ERR_HIP, "%s", s.tp_err.empty() ? #expr " failed" : s.tp_err.c_str()); \
    } while (0)
    hipStream_t cs = ctx->stream, ms = s.comm_stream;
    const TileGeom g = geom_of(ctx->hp, H, W);
    const int K = ctx->hp.nClasses, world = s.world, slot = io.slot;
    BandSpec sp;
    sp.world = world;
    sp.rank = s.rank;
    sp.nslabs = nslabs;
    sp.max_batch = ctx->max_batch;
    sp.band_row0 = band_row0;
    sp.band_rows = band_rows;
    sp.K = K;
    const size_t el = sp.gather_el = io.u8 ? 1 : stitch == UMX_STITCH_FP32 ? 4 : 2;   // element that is gathered (uint8: cast in the stitch)
    sp.staged = io.band_host != nullptr;
    sp.own_stream = io.up_s != cs;
    const BandPlan p = band_plan(g, sp);
    const int n = p.n;
    int rc;
    // every buffer is sized before anything is enqueued (a grow() between enqueued collectives would synchronise the device and free
    // memory under them when a later slide is larger); the gather buffers hold the largest slab, [K][mx_all][W] per rank
    if ((rc = grow(ctx, &s.probs, &s.probs_cap, p.probs_b, "shard probs", true))) return rc;
    std::vector<void*>& send = s.send[slot];
    if ((int)send.size() < n) { send.resize(n); s.send_cap[slot].resize(n); }
    if ((rc = grow(ctx, &s.gathered[slot], &s.gathered_cap[slot], p.gathered_b, slot ? "shard gathered[1]" : "shard gathered[0]", true))) return rc;
    for (int i = 0; i < n; ++i) {
        const std::string label = "shard send[" + std::to_string(slot) + "][" + std::to_string(i) + "]";
        if ((rc = grow(ctx, &send[i], &s.send_cap[slot][i], p.send_b, label.c_str(), true))) return rc;
    }
    float* const probs = (float*)s.probs;
    std::vector<hipEvent_t>& evs = s.events[slot];
    while ((int)evs.size() < p.nev) {
        hipEvent_t e;
        HIP_TRY(ctx, hipEventCreateWithFlags(&e, hipEventDisableTiming));
        evs.push_back(e);
    }
    hipEvent_t ev_in = evs[0], ev_last = evs[1], ev_halo = evs[2], ev_done = evs[3], ev_end = evs[4];
    const size_t in_b = io.raw_bits ? (size_t)io.raw_bits / 8 : sizeof(double);
    const size_t tile_f = (size_t)g.P * g.P * K, row_f = tile_f * g.npc;
    // launch groups [g0, g1): each one's staged rows of the host band (if any), then its tiles -> their place in `probs` (patch row lo first)
    auto groups = [&](int g0, int g1) -> int {
        for (int i = g0; i < g1; ++i) {
            const BandPlan::Group& G = p.groups[i];
            for (int c = 0; c < C_img && G.r1 > G.r0; ++c) {
                const size_t off = ((size_t)c * band_rows + (G.r0 - band_row0)) * W * in_b;
                HIP_TRY(ctx, hipMemcpyAsync((unsigned char*)io.raw_dev + off, (const unsigned char*)io.band_host + off, (size_t)(G.r1 - G.r0) * W * in_b,
                                          hipMemcpyHostToDevice, io.up_s));
            }
            if (G.ev >= 0) {
                HIP_TRY(ctx, hipEventRecord(evs[G.ev], io.up_s));
                HIP_TRY(ctx, hipStreamWaitEvent(cs, evs[G.ev], 0));
            }
            if ((rc = tiles_range(ctx, io.raw_dev ? nullptr : io.band_f64, C_img, g, band_row0, band_rows, mean, stdv, G.t0, G.t1,
                                  probs + ((size_t)G.t0 - (size_t)p.lo * g.npc) * tile_f, io.raw_dev, io.raw_bits, io.mm)))
                return rc;
        }
        return UMX_OK;
    };
    // the communication stream starts behind whatever the caller queued on the context's stream
    HIP_TRY(ctx, hipEventRecord(ev_in, cs));
    HIP_TRY(ctx, hipStreamWaitEvent(ms, ev_in, 0));
    // the band's last tiles first: the next rank waits for their patch row
    if ((rc = groups(0, p.slabs[0].g0))) return rc;
    HIP_TRY(ctx, hipEventRecord(ev_last, cs));
    HIP_TRY(ctx, hipStreamWaitEvent(ms, ev_last, 0));
    if (p.send_peer >= 0 || p.recv_peer >= 0) {
        if (tp.group_start) S_TP(ctx, tp.group_start(tp.user));
        if (p.send_peer >= 0) S_TP(ctx, tp.send(tp.user, probs + (size_t)(p.pb - 1 - p.lo) * row_f, row_f * sizeof(float), p.send_peer, ms));
        if (p.recv_peer >= 0) S_TP(ctx, tp.recv(tp.user, probs, row_f * sizeof(float), p.recv_peer, ms));
        if (tp.group_end) S_TP(ctx, tp.group_end(tp.user));
    }
    HIP_TRY(ctx, hipEventRecord(ev_halo, ms));
    for (int i = 0; i < n; ++i) {
        const BandPlan::Slab& sl = p.slabs[i];
        if ((rc = groups(sl.g0, sl.g1))) return rc;
        if (i == 0) HIP_TRY(ctx, hipStreamWaitEvent(cs, ev_halo, 0));   // the previous rank's last patch row feeds this band's first rows
        const size_t plane_b = (size_t)sl.mx * W * el, send_b = (size_t)K * plane_b;
        // straight into the padded gather buffer [K][mx][W] (the padded tails stay uninitialised: the scatter never reads them)
        if (sl.s1 > sl.s0 && (rc = stitch_rows(ctx, probs, p.lo, p.pb, H, W, mode, io.u8 ? kStitchU8 : stitch, sl.s0, sl.s1, send[i], sl.mx))) return rc;
        hipEvent_t ev_s = evs[sl.ev];
        HIP_TRY(ctx, hipEventRecord(ev_s, cs));
        HIP_TRY(ctx, hipStreamWaitEvent(ms, ev_s, 0));
        if (io.own_host && sl.s1 > sl.s0) {   // this rank's rows of the slab: down to the host under the next slab's tiles
            if (io.dn_s != cs) HIP_TRY(ctx, hipStreamWaitEvent(io.dn_s, ev_s, 0));
            const size_t own_rows = (size_t)(p.own1 - p.own0);
            for (int k = 0; k < K; ++k)
                HIP_TRY(ctx, hipMemcpyAsync(io.own_host + ((size_t)k * own_rows + (size_t)(sl.s0 - p.own0)) * W, (char*)send[i] + k * plane_b,
                                          (size_t)(sl.s1 - sl.s0) * W, hipMemcpyDeviceToHost, io.dn_s));
        }
        // (one gather buffer per slot, reused slab after slab: gather i+1 is queued behind the scatter copies of gather i)
        S_TP(ctx, tp.all_gather(tp.user, send[i], s.gathered[slot], send_b, ms));
        for (int q = 0; q < world; ++q)
            for (int k = 0; k < K && sl.rb[q] > sl.ra[q]; ++k)
                HIP_TRY(ctx, hipMemcpyAsync((char*)io.out_full + ((size_t)k * H + sl.ra[q]) * W * el,
                                          (char*)s.gathered[slot] + (size_t)q * send_b + k * plane_b,
                                          (size_t)(sl.rb[q] - sl.ra[q]) * W * el, hipMemcpyDeviceToDevice, ms));
    }
    HIP_TRY(ctx, hipEventRecord(ev_done, ms));
    if (io.join) HIP_TRY(ctx, hipStreamWaitEvent(cs, ev_done, 0));   // the result is complete for whatever the caller queues next
    HIP_TRY(ctx, hipEventRecord(ev_end, cs));
    if (io.ev_gathered) *io.ev_gathered = ev_done;
    if (io.ev_cs_end) *io.ev_cs_end = ev_end;
#undef S_TP
    return UMX_OK;
}

}  // namespace

// How a submitted sharded call is waited for (umx_infer_image_wait): the completion event is polled, and between polls the
// communicator's asynchronous error state is read (ncclCommGetAsyncError: a peer died, a link failed) and a wall-clock bound is kept
// (UMX_SHARD_TIMEOUT_S, default 600 s; 0 = none) -- either ends the wait with UMX_ERR_HIP after ncclCommAbort, never with a hang.
int umx::shard_wait(umx_ctx* ctx, hipEvent_t ev) {
    Shard& s = *ctx->shard;
    double limit = 600.0;
    if (const char* e = getenv("UMX_SHARD_TIMEOUT_S")) limit = atof(e);
    const auto t0 = std::chrono::steady_clock::now();
    unsigned spins = 0;
    for (;;) {
        const hipError_t q = hipEventQuery(ev);
        if (q == hipSuccess) break;
        if (q != hipErrorNotReady) { shard_abort(s); return fail(ctx, UMX_ERR_HIP, "hipEventQuery failed: %s", hipGetErrorString(q)); }
        if ((++spins & 63u) == 0u) {
            if (s.comm && rccl()->CommGetAsyncError) {
                ncclResult_t ae = ncclSuccess;
                const ncclResult_t r = rccl()->CommGetAsyncError(s.comm, &ae);
                if (r != ncclSuccess || (ae != ncclSuccess && ae != ncclInProgress)) {
                    const char* why = rccl()->GetErrorString(r != ncclSuccess ? r : ae);
                    shard_abort(s);
                    hipStreamSynchronize(s.comm_stream);
                    return fail(ctx, UMX_ERR_HIP, "the sharded world failed while this rank waited (RCCL: %s); the communicator was aborted", why);
                }
            }
            const double waited = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
            if (limit > 0.0 && waited > limit) {
                shard_abort(s);
                return fail(ctx, UMX_ERR_HIP, "timed out after %d s waiting for a sharded call (UMX_SHARD_TIMEOUT_S): a peer is not taking part; "
                                              "the communicator was aborted", (int)waited);
            }
            std::this_thread::sleep_for(std::chrono::microseconds(50));
        }
    }
    return UMX_OK;
}

extern "C" {

int umx_infer_image_sharded_dev(umx_ctx* ctx, const double* band_dev, int C_img, int H, int W, int band_row0, int band_rows,
                                double mean, double stdv, int mode, int stitch, int nslabs, void* out_full_dev) {
    if (const int rc = check_image(ctx, out_full_dev != nullptr, C_img, H, W, false, 0, stdv, mode, stitch, nullptr)) return rc;
    if (const int rc = shard_check(ctx, band_dev, H, W, band_row0, band_rows)) return rc;
    if (ctx->hs[0].busy || ctx->hs[1].busy)   // (slot 0's gather buffers are this entry's too)
        return fail(ctx, UMX_ERR_INVALID, "a submitted call is still in flight on this context: wait for it first");
    return guarded(ctx, true, true, [&]() -> int {
        HIP_TRY(ctx, hipSetDevice(ctx->device));
        RunIO io;
        io.band_f64 = band_dev;
        io.out_full = out_full_dev;
        return shard_drain(ctx, sharded_run(ctx, io, C_img, H, W, band_row0, band_rows, mean, stdv, mode, stitch, nslabs));
    });
}

// The same schedule fed the way the one-GPU line is fed (umx_infer_image_raw_submit): this rank's raw uint8 / uint16 rows come up
// from the host piece by piece on the upload stream ahead of the tiles that read them, the tile gather converts (im2double, and
// with `range` the drivers' rescale_intensity to the whole planes' (min, max), which the caller's reader knows -- a rank sees only
// its band), stitched slabs are cast to the drivers' uint8 before they are gathered (a quarter of the fp32 bytes over xGMI), and
// the rank's own rows go down to the host on the download stream under the next slab's tiles.  Two slides may be in flight.
static int sharded_raw_enqueue(umx_ctx* ctx, int slot, const void* band_host, int bits, int C_img, int H, int W, int band_row0,
                               int band_rows, const uint32_t* range, double mean, double stdv, int mode, int nslabs,
                               uint8_t* own_out_host, uint8_t* out_full_dev) {
    Shard& s = *ctx->shard;
    umx_ctx::HostSlot& hs = ctx->hs[slot];
    const size_t in_b = (size_t)bits / 8, K = ctx->hp.nClasses;
    const size_t raw_b = (size_t)C_img * std::max(band_rows, 0) * W * in_b;
    const size_t mm_off = (raw_b + 255) & ~(size_t)255;
    int rc;
    if ((rc = grow(ctx, &hs.d_out, &hs.out_cap, mm_off + 64 * (size_t)std::max(C_img, 1) + 256, slot ? "slot 1 d_out" : "slot 0 d_out"))) return rc;
    unsigned char* const base = (unsigned char*)hs.d_out;
    unsigned* const mm = (unsigned*)(base + mm_off);
    if (!out_full_dev) {
        if ((rc = grow(ctx, &s.full_u8[slot], &s.full_u8_cap[slot], K * (size_t)H * W, slot ? "shard full_u8[1]" : "shard full_u8[0]", true))) return rc;
        out_full_dev = (uint8_t*)s.full_u8[slot];
    }
    RunIO io;
    io.slot = slot;
    io.u8 = 1;
    io.out_full = out_full_dev;
    io.own_host = own_out_host;
    io.up_s = ctx->up_stream;
    io.dn_s = ctx->dn_stream;
    io.join = false;
    hipEvent_t ev_gathered = nullptr, ev_end = nullptr;
    io.ev_gathered = &ev_gathered;
    io.ev_cs_end = &ev_end;
    if (range && (rc = put_range(ctx, mm, range, C_img))) return rc;
    if (gathers_raw(ctx)) {
        io.raw_dev = base;
        io.raw_bits = bits;
        io.mm = range ? mm : nullptr;
        io.band_host = band_host;
    } else {
        // an engine whose gather reads float64 (exact-fp32 precision): the band goes up whole and is converted first
        if ((rc = grow(ctx, (void**)&hs.d_image, &hs.image_cap, (size_t)C_img * std::max(band_rows, 1) * W * sizeof(double),
                       slot ? "slot 1 d_image" : "slot 0 d_image")))
            return rc;
        if (raw_b) HIP_TRY(ctx, hipMemcpyAsync(base, band_host, raw_b, hipMemcpyHostToDevice, ctx->stream));
        for (int c = 0; c < C_img && band_rows > 0; ++c)
            HIP_TRY(ctx, launch_raw_convert(base + (size_t)c * band_rows * W * in_b, bits, (size_t)band_rows * W, range ? 1 : 0, mm + 16 * c,
                                            hs.d_image + (size_t)c * band_rows * W, ctx->stream));
        io.band_f64 = hs.d_image;
    }
    if ((rc = sharded_run(ctx, io, C_img, H, W, band_row0, band_rows, mean, stdv, mode, UMX_STITCH_FP16_COMPAT, nslabs))) return rc;
    // `done`: the gathers and scatters (communication stream), this rank's downloads and the range flag behind the last kernel
    HIP_TRY(ctx, hipStreamWaitEvent(ctx->dn_stream, ev_gathered, 0));
    HIP_TRY(ctx, hipStreamWaitEvent(ctx->dn_stream, ev_end, 0));
    return slot_finish(ctx, slot, ctx->dn_stream);
}

int umx_infer_image_sharded_raw_submit(umx_ctx* ctx, int slot, const void* band_host, int bits, int C_img, int H, int W,
                                       int band_row0, int band_rows, const uint32_t* range, double mean, double stdv, int mode,
                                       int nslabs, uint8_t* own_out_host, uint8_t* out_full_dev) {
    if (const int rc = check_image(ctx, band_host || band_rows == 0, C_img, H, W, true, bits, stdv, mode, UMX_STITCH_FP16_COMPAT, range))
        return rc;
    if (const int rc = shard_check(ctx, band_host, H, W, band_row0, band_rows)) return rc;
    return guarded(ctx, true, false, [&]() -> int {   // (guard mode: umx_infer_image_wait checks the zones)
        return slot_submit(ctx, slot, [&] {
            return shard_drain(ctx, sharded_raw_enqueue(ctx, slot, band_host, bits, C_img, H, W, band_row0, band_rows, range, mean, stdv, mode,
                                                        nslabs, own_out_host, out_full_dev));
        });
    });
}

int umx_infer_image_sharded_raw(umx_ctx* ctx, const void* band_host, int bits, int C_img, int H, int W, int band_row0, int band_rows,
                                const uint32_t* range, double mean, double stdv, int mode, int nslabs, uint8_t* own_out_host,
                                uint8_t* out_full_dev) {
    return guarded(ctx, true, true, [&]() -> int {
        const int rc = umx_infer_image_sharded_raw_submit(ctx, 0, band_host, bits, C_img, H, W, band_row0, band_rows, range, mean, stdv, mode,
                                                          nslabs, own_out_host, out_full_dev);
        return rc ? rc : umx_infer_image_wait(ctx, 0);
    });
}

}  // extern "C"
