// Host side of libumx: graph construction from the reference's hyper-parameters, weight folding / packing,
// device memory plan, launch sequencing and the C ABI declared in include/umx.h.  gfx950 (MI355X) only.
#include "umx_internal.h"

using namespace umx;

namespace umx {

thread_local std::string g_err;

int fail(umx_ctx* ctx, int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    if (ctx) ctx->err = buf;
    g_err = buf;
    return code;
}

int dev_alloc(umx_ctx* ctx, void** out, size_t bytes, const std::string& label, bool scoped) {
    void* d = nullptr;
    HIP_TRY(ctx, arena_alloc(&ctx->mem, &d, bytes, false, label.c_str(), scoped));
    *out = d;
    return UMX_OK;
}


int grow(umx_ctx* ctx, void** buf, size_t* cap, size_t bytes, const char* label, bool device_wide) {
    if (*cap >= bytes) return UMX_OK;
    if (*buf) {
        if (device_wide) HIP_TRY(ctx, hipDeviceSynchronize());
        else HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        HIP_TRY(ctx, arena_release(&ctx->mem, *buf));
        *buf = nullptr;
        *cap = 0;
    }
    HIP_TRY(ctx, arena_alloc(&ctx->mem, buf, bytes, false, label, true));
    *cap = bytes;
    return UMX_OK;
}

// guard mode: every stream that touches the context's buffers -- the context's (or a caller's, umx_set_stream), the second lane's,
// the copy streams and a sharded context's communication stream
static int guard_drain(umx_ctx* ctx) {
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    for (hipStream_t s : {ctx->stream, ctx->own_stream, ctx->stream2, ctx->up_stream, ctx->dn_stream, shard_stream(ctx)})
        if (s) HIP_TRY(ctx, hipStreamSynchronize(s));
    return UMX_OK;
}

int guard_begin(umx_ctx* ctx, bool refill) {
    if (ctx->guard_depth == 0 && refill) {   // (an entry that only waits keeps its own, bounded, way of waiting)
        if (const int rc = guard_drain(ctx)) return rc;
        HIP_TRY(ctx, arena_refill(ctx->mem, ctx->stream));
    }
    ++ctx->guard_depth;
    return UMX_OK;
}

int guard_end(umx_ctx* ctx, int rc, bool check) {
    if (--ctx->guard_depth > 0 || rc != UMX_OK || !check) return rc;
    if ((rc = guard_drain(ctx))) return rc;
    std::string msg;
    rc = arena_check(ctx->mem, &msg);
    return rc == UMX_OK ? UMX_OK : fail(ctx, rc, "%s", msg.c_str());
}

int site_of(umx_ctx* ctx, const std::string& name, const std::string& kernel) {
    for (size_t i = 0; i < ctx->sites.size(); ++i)
        if (ctx->sites[i].name == name && ctx->sites[i].kernel == kernel) return (int)i;   // (a layer that runs on two kernels -- e.g. the persistent form for large launch groups only -- has two entries)
    ProfSite s;
    s.name = name;
    s.kernel = kernel;
    ctx->sites.push_back(s);
    return (int)ctx->sites.size() - 1;
}

int prof_fold(umx_ctx* ctx) {
    if (ctx->pending.empty()) return UMX_OK;
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if (ctx->stream2) HIP_TRY(ctx, hipStreamSynchronize(ctx->stream2));
    for (auto& pe : ctx->pending) {
        float ms = 0.f;
        HIP_TRY(ctx, hipEventElapsedTime(&ms, pe.a, pe.b));
        ctx->sites[pe.site].total_ms += ms;
        ctx->free_events.push_back(pe.a);
        ctx->free_events.push_back(pe.b);
    }
    ctx->pending.clear();
    return UMX_OK;
}

// ---- one launch group of n tiles on a lane: every tensor lives in the lane's full-batch buffer (hi plane of n tiles, then lo plane
// of n tiles -- lo_of(b, n) moves with n, so operands are bound per launch)

// fp32 tiles -> (hi, lo) input planes (2 -> 8 channels, scaled by 2^act_shift)
int run_input_split(umx_ctx* ctx, const Lane& lane, const float* tiles, int n) {
    if (!tiles) return UMX_OK;   // the gather kernel already wrote the (hi, lo) planes
    const Buffer& b0 = (*lane.bufs)[0];
    if (ctx->site_split < 0) ctx->site_split = site_of(ctx, "input.split", "split_f32");
    ProfScope ps(ctx, lane.stream, ctx->site_split, 0.0, (double)n * b0.S * b0.S * (4.0 * b0.C + 4.0 * b0.Cs));
    HIP_TRY(ctx, launch_split_f32(tiles, (size_t)n * b0.S * b0.S, b0.C, b0.Cs, std::ldexp(1.f, ctx->act_shift), hi_of(b0), lo_of(b0, n),
                                  ctx->in_cw, lane.stream));
    return UMX_OK;
}

// the operands of launch L on n tiles of the lane -> *p: sources, destination, the appended raw skip
int bind_f16(umx_ctx* ctx, const Lane& lane, const Launch& L, int n, float* probs, HConvParams* out) {
    const std::vector<Buffer>& bufs = *lane.bufs;
    HConvParams& p = *out;
    p = L.hcp;
    p.B = n;
    p.overflow_flag = ctx->d_flag + ctx->flag_word;
    for (int gi = 0; gi < L.ngroups; ++gi) {
        const Buffer& sb = bufs[L.g[gi].src];
        p.src_hi[gi] = hi_of(sb);
        p.src_lo[gi] = lo_of(sb, n);
        p.Cs[gi] = sb.Cs;
        p.srcA[gi] = sb.planar ? 16 : sb.Cs * 2;
        p.srcB[gi] = sb.planar ? sb.S * sb.S * 16 : 16;
    }
    if (L.ngroups < 2) { p.srcA[1] = p.srcA[0]; p.srcB[1] = p.srcB[0]; }
    const Buffer& db = bufs[L.dst];
    if (p.head_K > 0) p.probs = probs;   // fused softmax head
    else if (db.as_f32) p.dst_f32 = db.d;
    else { p.dst_hi = hi_of(db); p.dst_lo = lo_of(db, n); p.dst_planar = db.planar ? 1 : 0; }
    if (L.app_src >= 0) {   // the raw-input skip rides in the spare channels of this launch's output (Launch::app_src)
        const Buffer& ab = bufs[L.app_src];
        if (L.app_src != 0 || !ctx->in_cw) return fail(ctx, UMX_ERR_INVALID, "internal: the appended tensor is not in the compact form");
        p.app_c = reinterpret_cast<const unsigned char*>(ab.d);
        p.app_cw = ctx->in_cw;
        p.app_oct = L.app_c0 / 8;                 // the stored octet ...
        p.app_word = (L.app_c0 % 8) / 2;          // ... and its 32-bit word the two appended binary16 values fill
    }
    for (int gi = 0; gi < L.ngroups; ++gi)
        if (L.g[gi].src == 0 && ctx->in_cw && !L.use_first)
            return fail(ctx, UMX_ERR_INVALID, "internal: %s reads the compact input tiles through the generic kernel", L.name.c_str());
    return UMX_OK;
}

// diagnostic: UMX_DEBUG_STAMPS=<layer name> prints the mean s_memtime segments of that layer's workgroups
int run_stamps(umx_ctx* ctx, const Lane& lane, const Launch& L, HConvParams& p, int n) {
    size_t nwg = (size_t)((n + p.imgs - 1) / p.imgs) * p.tiles_y * p.tiles_x;
    if (p.f6) nwg = (nwg + 1) / 2;   // (two tiles per workgroup)
    nwg *= (size_t)p.nblocks * (p.fused_phases ? 1 : p.nphase);
    long long* d = nullptr;
    HIP_TRY(ctx, hipMalloc((void**)&d, nwg * 7 * sizeof(long long)));
    p.dbg = d;
    if (p.xcd_order == 2) p.xcd_order = 1;   // (the stamp records are indexed by the three-dimensional grid)
    HIP_TRY(ctx, launch_conv_f16(p, lane.stream));
    HIP_TRY(ctx, hipStreamSynchronize(lane.stream));
    std::vector<long long> hst(nwg * 7);
    HIP_TRY(ctx, hipMemcpy(hst.data(), d, hst.size() * sizeof(long long), hipMemcpyDeviceToHost));
    hipFree(d);
    double m[7] = {0, 0, 0, 0, 0, 0, 0};
    for (size_t w = 0; w < nwg; ++w)
        for (int k = 0; k < 7; ++k) m[k] += (double)hst[w * 7 + k] / nwg;
    fprintf(stderr, "[umx stamps] %s: %zu workgroups, LDS %d B, wbuf %d B | shader cycles: prologue %.0f, stage waits %.0f "
                    "(own loads %.0f, barrier %.0f), issuing the next stage's loads %.0f, MFMA blocks %.0f, epilogue %.0f, total %.0f\n",
            L.name.c_str(), nwg, p.lds_bytes, p.wbuf_bytes, m[0], m[1], m[5], m[1] - m[5], m[6], m[2] - m[6], m[3], m[4]);
    return UMX_OK;
}

// one launch of the split-precision plan
int run_launch_f16(umx_ctx* ctx, const Lane& lane, Launch& L, int n, float* probs) {
    if (L.head) {
        if (ctx->head_fused) return UMX_OK;   // computed in the epilogue of the last convolution
        const Buffer& sb = (*lane.bufs)[L.g[0].src];
        ProfScope ps(ctx, lane.stream, site_of(ctx, L.name, "head_softmax"), L.flops * n, L.bytes * n);
        HIP_TRY(ctx, launch_head_softmax(sb.d, (size_t)n * L.H * L.W, L.head_C, L.head_K, L.d_head_w, L.d_pre_s, L.d_pre_b, probs, lane.stream));
        return UMX_OK;
    }
    HConvParams p;
    if (const int rc = bind_f16(ctx, lane, L, n, probs, &p)) return rc;
    const LaunchShape sh = launch_shape(L, p, n);
    p.xcd_order = sh.xcd_order; p.ntiles_grid = sh.ntiles_grid; p.tiles_per_xcd = sh.tiles_per_xcd;
    if (!ctx->stamps.empty() && L.name == ctx->stamps) return run_stamps(ctx, lane, L, p, n);
    if (L.use_first) {   // dense-K kernel of the first down-sampling layer
        FirstParams f = L.first;
        const Buffer& sb = (*lane.bufs)[0];
        f.B = n;
        f.src_hi = hi_of(sb); f.src_lo = lo_of(sb, n);
        f.src_c = ctx->in_cw ? reinterpret_cast<const unsigned char*>(sb.d) : nullptr;
        f.dst_hi = p.dst_hi; f.dst_lo = p.dst_lo; f.dst_planar = p.dst_planar;
        f.overflow_flag = p.overflow_flag;
        ProfScope ps(ctx, lane.stream, site_of(ctx, L.name, L.kernel), L.flops * n, L.bytes * n, 2.0 * 3.0 * f.NKS * 32.0 * f.NT * 16.0 * L.H * L.W * n);
        HIP_TRY(ctx, launch_conv_first(f, lane.stream));
        return UMX_OK;
    }
    const int site = site_of(ctx, L.name, L.kernel);
    ctx->sites[site].xcd_order = p.xcd_order;
    ProfScope ps(ctx, lane.stream, site, L.flops * n, L.bytes * n, L.exec_flops * n);
    HIP_TRY(ctx, launch_conv_f16(p, lane.stream));
    return UMX_OK;
}

// The split-precision plan: input split (unless the gather kernel already wrote the planes), then every launch once
// over the whole batch.  (Running the full-resolution layers as chains over sub-batches, to keep producer -> consumer
// tensors in the 256 MiB Infinity Cache, was measured slower at every sub-batch size -- DESIGN.md section 4.)
int run_unet_f16(umx_ctx* ctx, const Lane& lane, const float* tiles, int n, float* probs) {
    int rc = run_input_split(ctx, lane, tiles, n);
    if (rc) return rc;
    for (auto& L : ctx->plan)
        if ((rc = run_launch_f16(ctx, lane, L, n, probs))) return rc;
    if (ctx->prof && ctx->pending.size() > 4096) return prof_fold(ctx);
    return UMX_OK;
}

int check_range_flag(umx_ctx* ctx) {   // call with the stream idle
    if (!ctx->d_flag) return UMX_OK;
    int f = 0;
    HIP_TRY(ctx, hipMemcpy(&f, ctx->d_flag, sizeof f, hipMemcpyDeviceToHost));
    if (!f) return UMX_OK;
    HIP_TRY(ctx, hipMemset(ctx->d_flag, 0, sizeof f));
    return fail(ctx, UMX_ERR_RANGE, "an activation left the binary16 range of the split-precision path; "
                                    "create the context with UMX_PREC_F32 (or UMX_PRECISION=f32)");
}

// run the UNet on n tiles already in bufs[0] layout at `tiles` -> probs, on a lane
int run_unet(umx_ctx* ctx, const Lane& lane, const float* tiles, int n, float* probs) {
    if (ctx->precision == UMX_PREC_F16X3) return run_unet_f16(ctx, lane, tiles, n, probs);
    const std::vector<Buffer>& bufs = *lane.bufs;
    for (auto& L : ctx->plan) {
        const float* src0 = L.g[0].src == 0 ? tiles : bufs[L.g[0].src].d;
        if (L.head) {
            const size_t npix = (size_t)n * L.H * L.W;
            ProfScope ps(ctx, lane.stream, site_of(ctx, L.name, "head_softmax"), L.flops * n, L.bytes * n);
            HIP_TRY(ctx, launch_head_softmax(src0, npix, L.head_C, L.head_K, L.d_head_w, L.d_pre_s, L.d_pre_b, probs, lane.stream));
            continue;
        }
        ConvParams p = L.cp;
        p.B = n;
        p.src[0] = src0;
        if (L.ngroups > 1) p.src[1] = L.g[1].src == 0 ? tiles : bufs[L.g[1].src].d;
        p.dst = bufs[L.dst].d;
        char kn[48];
        snprintf(kn, sizeof kn, "conv_mfma_f32<%d, %d>", L.nt, L.hpix <= 2 ? 2 : 4);
        ProfScope ps(ctx, lane.stream, site_of(ctx, L.name, kn), L.flops * n, L.bytes * n, L.exec_flops * n);
        HIP_TRY(ctx, launch_conv(p, L.nt, L.hpix, lane.stream));
    }
    if (ctx->prof && ctx->pending.size() > 4096) return prof_fold(ctx);
    return UMX_OK;
}

// Batching of `total` tiles over the lanes of a context: equal batches (<= max_batch), as many as a multiple of the lane
// count when there is more than one batch, consecutive batches on alternating lanes.  The second lane's stream is forked
// from the context's stream by an event at the first use and joined back in join(); with one lane (or one batch) every
// launch stays on the context's stream.  next() hands out the batch's size and the lane it runs on.
struct LaneLoop {
    umx_ctx* ctx;
    int batch, k = 0;
    bool forked = false;
    LaneLoop(umx_ctx* c, int total) : ctx(c) {
        int nbatch = (total + c->max_batch - 1) / c->max_batch;
        if (c->nlanes > 1 && nbatch > 1) nbatch = (nbatch + c->nlanes - 1) / c->nlanes * c->nlanes;
        batch = nbatch > 0 ? (total + nbatch - 1) / nbatch : 1;
    }
    int next(int left, Lane* lane) {
        int i = ctx->nlanes > 1 ? k % ctx->nlanes : 0;
        if (i == 1 && !forked) {
            forked = true;
            if (hipEventRecord(ctx->ev_fork, ctx->stream) != hipSuccess ||
                hipStreamWaitEvent(ctx->stream2, ctx->ev_fork, 0) != hipSuccess) i = 0;   // degrade to one lane
        }
        ++k;
        *lane = lane_of(ctx, i);
        return std::min(batch, left);
    }
    int join() {
        if (!forked) return UMX_OK;
        forked = false;
        HIP_TRY(ctx, hipEventRecord(ctx->ev_join, ctx->stream2));
        HIP_TRY(ctx, hipStreamWaitEvent(ctx->stream, ctx->ev_join, 0));
        return UMX_OK;
    }
    ~LaneLoop() { join(); }   // error paths: the side stream is still joined into the context's stream
};

// tiles [t0, t1) of the slide (row-major tile index) -> probs_dev (tile t0 first): gather + normalise + UNet, in launch
// groups of <= max_batch tiles
bool gathers_raw(const umx_ctx* ctx) {
    return ctx->precision == UMX_PREC_F16X3 && ctx->hp.nChannels <= 8 && ctx->bufs[0].Cs == 8;
}

int tiles_range(umx_ctx* ctx, const double* image_dev, int C_img, const TileGeom& g, int band_row0, int band_rows,
                       double mean, double stdv, int t0, int t1, float* probs_dev, const void* raw_dev, int raw_bits,
                       const unsigned* mm_dev) {
    const size_t prob_f = (size_t)g.P * g.P * ctx->hp.nClasses;
    if (ctx->site_gather < 0) ctx->site_gather = site_of(ctx, "pi2d.gather_normalise", "gather_normalise");
    const bool direct16 = gathers_raw(ctx);
    if (raw_dev && !direct16) return fail(ctx, UMX_ERR_INVALID, "internal: raw planes handed to an engine that does not gather from them");
    const void* const src = raw_dev ? raw_dev : (const void*)image_dev;
    const double src_b = raw_dev ? raw_bits / 8.0 : 8.0;
    LaneLoop ll(ctx, t1 - t0);
    Lane lane;
    for (int t = t0, nb; t < t1; t += nb) {
        nb = ll.next(t1 - t, &lane);
        const Buffer& b0 = (*lane.bufs)[0];
        float* const tiles32 = ctx->precision == UMX_PREC_F16X3 ? lane.tiles32 : b0.d;
        {
            ProfScope ps(ctx, lane.stream, ctx->site_gather, 0.0,
                         (double)nb * g.P * g.P * (src_b * C_img + (ctx->in_cw ? 4.0 * ctx->in_cw : direct16 ? 32.0 : 4.0 * ctx->hp.nChannels)));
            if (direct16) {   // gather + normalise + (hi, lo) split in one pass
                HIP_TRY(ctx, launch_gather_split(src, raw_dev ? raw_bits : 0, C_img, band_row0, band_rows, g, ctx->hp.nChannels, mean, stdv, t, nb,
                                                 std::ldexp(1.f, ctx->act_shift), hi_of(b0), lo_of(b0, nb), ctx->in_cw, lane.stream,
                                                 raw_dev ? mm_dev : nullptr));
            } else {
                HIP_TRY(ctx, launch_gather_normalise(image_dev, C_img, band_row0, band_rows, g, ctx->hp.nChannels, mean, stdv, t,
                                                     nb, tiles32, lane.stream));
            }
        }
        int rc = run_unet(ctx, lane, direct16 ? nullptr : tiles32, nb, probs_dev + (size_t)(t - t0) * prob_f);
        if (rc) return rc;
    }
    return ll.join();
}

// the planner's switches from the environment; called by umx_create_opts, umx_plan_check and the trainer's select_route, nowhere else
PlanSwitches plan_switches_from_env() {
    return plan_switches_parse(getenv("UMX_PLAN_NT"), getenv("UMX_PLAN_OVERRIDE"), getenv("UMX_PLAN_THREADS"), getenv("UMX_DEBUG_PLAN") != nullptr,
                               getenv("UMX_DEBUG_STAMPS"));
}

// a host plan on the device: its arrays in the context's allocations, the launch's parameters with their pointers set
int upload_plan(umx_ctx* ctx, Launch& L, const HostPlan& P) {
    int rc = UMX_OK;
    auto up = [&](const auto& v, const std::string& what) {   // (an empty array: null)
        typename std::decay_t<decltype(v)>::value_type* d = nullptr;
        if (!rc) rc = upload_raw(ctx, v, &d, L.name + " " + what);
        return d;
    };
    HConvParams& h = L.hcp;
    h = P.h;
    h.stages = up(P.stages, "stages");
    h.econst = reinterpret_cast<const uint4*>(up(P.econst, "econst"));
    for (int list = 0; list < 4; ++list) h.ph[list].w = reinterpret_cast<const uint4*>(up(P.wimg[list], "weights[" + std::to_string(list) + "]"));
    h.head_frag = reinterpret_cast<const uint4*>(up(P.head_frag, "head_frag"));
    h.zeros = ctx->d_zeros;
    h.overflow_flag = ctx->d_flag;
    adopt_plan(L, P);
    if (P.use_first) {
        L.first = P.first;
        L.first.w = reinterpret_cast<const uint4*>(up(P.first_w, "first weights"));
        L.first.econst = reinterpret_cast<const float*>(h.econst);
    }
    return rc;
}

}  // namespace umx

extern "C" {

const char* umx_version(void) { return "umx 0.4 (gfx950)"; }
int umx_prof_entry_size(void) { return (int)sizeof(umx_prof_entry); }

int umx_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int umx_device_mem_info(int device_ordinal, size_t* free_bytes, size_t* total_bytes) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1)
        return fail(nullptr, UMX_ERR_NO_DEVICE, "no HIP device available (libumx has no CPU fallback)");
    if (device_ordinal < 0 || device_ordinal >= ndev)
        return fail(nullptr, UMX_ERR_INVALID, "device ordinal %d out of range (%d devices)", device_ordinal, ndev);
    int prev = 0;
    HIP_TRY(nullptr, hipGetDevice(&prev));
    HIP_TRY(nullptr, hipSetDevice(device_ordinal));
    size_t f = 0, t = 0;
    hipError_t e = hipMemGetInfo(&f, &t);
    hipSetDevice(prev);
    if (e != hipSuccess) return fail(nullptr, UMX_ERR_HIP, "hipMemGetInfo failed: %s", hipGetErrorString(e));
    if (free_bytes) *free_bytes = f;
    if (total_bytes) *total_bytes = t;
    return UMX_OK;
}

const char* umx_last_error(const umx_ctx* ctx) { return ctx ? ctx->err.c_str() : g_err.c_str(); }

void umx_test_double_to_half(const double* in, uint16_t* out, size_t n) {
    for (size_t i = 0; i < n; ++i) out[i] = double_to_half_rne(in[i]);
}

// the planner's OCP MX fp6 packing of one block of 32 (what the F6 form's weight images are made of): 24 bytes + the e8m0 scale byte
int umx_test_mx_pack_e2m3(const double* v32, uint8_t* out24) {
    if (!v32 || !out24) return -1;
    double v[32], amax = 0.0;
    for (int i = 0; i < 32; ++i) { v[i] = v32[i]; amax = std::max(amax, std::fabs(v[i])); }
    unsigned char b[24];
    const int e8 = mx_pack_e2m3(v, amax, b);
    memcpy(out24, b, 24);
    return e8;
}

// the DEVICE routine the stitch kernel converts with (d2h_rne: round-to-odd binary32, then v_cvt_f16_f32) on the same vectors: the
// host routine above states the conversion, this one is what runs
int umx_test_double_to_half_dev(const double* in, uint16_t* out, size_t n) {
    if (!in || !out) return fail(nullptr, UMX_ERR_INVALID, "in / out is NULL");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) return fail(nullptr, UMX_ERR_NO_DEVICE, "no HIP device available");
    double* din = nullptr;
    uint16_t* dout = nullptr;
    DevArena mem;   // call-local (UMX_DEBUG_GUARD: red zones round both vectors, checked before they are freed)
    std::string msg;
    if (arena_init(&mem, &msg) != UMX_OK) return fail(nullptr, UMX_ERR_INVALID, "%s", msg.c_str());
    hipError_t e = arena_alloc(&mem, (void**)&din, n * sizeof(double) + 16, false, "double_to_half in", true);
    if (e == hipSuccess) e = arena_alloc(&mem, (void**)&dout, n * sizeof(uint16_t) + 16, false, "double_to_half out", true);
    if (e == hipSuccess) e = hipMemcpy(din, in, n * sizeof(double), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = launch_d2h_rne_test(din, dout, n, nullptr);
    if (e == hipSuccess) e = hipMemcpy(out, dout, n * sizeof(uint16_t), hipMemcpyDeviceToHost);
    const int grc = e == hipSuccess ? arena_check(mem, &msg) : UMX_OK;
    arena_free(&mem);
    if (e != hipSuccess)
        return fail(nullptr, e == hipErrorOutOfMemory ? UMX_ERR_OOM : UMX_ERR_HIP, "umx_test_double_to_half_dev: %s", hipGetErrorString(e));
    return grc == UMX_OK ? UMX_OK : fail(nullptr, grc, "%s", msg.c_str());
}

int umx_describe(const umx_hparams* hp, int* n_launches, double* flops_per_tile, double* executed_flops_per_tile) {
    std::string why;
    int rc = check_hp(hp, &why);
    if (rc) return fail(nullptr, rc, "%s", why.c_str());
    std::vector<Launch> plan;
    build_graph(*hp, nullptr, &plan, nullptr, nullptr, nullptr);
    double f = 0, e = 0;
    for (auto& L : plan) { f += L.flops; e += L.exec_flops; }
    if (n_launches) *n_launches = (int)plan.size();
    if (flops_per_tile) *flops_per_tile = f;
    if (executed_flops_per_tile) *executed_flops_per_tile = e;
    return UMX_OK;
}

// Would umx_create(UMX_PREC_F16X3) take this model?  Host only (no device): the graph is built with zero weights and planned as
// umx_create plans it, without the upload.  UMX_OK, or UMX_ERR_INVALID with the first refused layer and the planner's reason in
// umx_last_error(NULL).
int umx_plan_check(const umx_hparams* hp) {
    std::string why;
    int rc = check_hp(hp, &why);
    if (rc) return fail(nullptr, rc, "%s", why.c_str());
    std::vector<float> blob(blob_floats_needed(*hp), 0.f);
    ModelPlan m;
    if ((rc = plan_model(*hp, blob.data(), true, false, 0, plan_switches_from_env(), &m, &why))) return fail(nullptr, rc, "%s", why.c_str());
    return UMX_OK;
}

// The split-precision plan of a model as text, host only: plan_model under the given switches (strings as the variables would hold
// them, NULL or "": not set; threads 0: default), one line per launch but the head -- its UMX_DEBUG_PLAN text, the kernel, the
// destination's layout, nt16, wshift, infer_digest and, for every batch n, "n:<workgroup order>/<tiles per XCD>" (launch_shape)
int umx_test_infer_plan(const umx_hparams* hp, int f6, int act_shift, const float* blob, size_t blob_floats, const char* nt,
                        const char* override_list, const char* stamps, int threads, const int* batches, int nbatches, char* text, size_t cap,
                        size_t* needed) {
    if (!hp || !blob || !needed || (!text && cap) || (!batches && nbatches) || nbatches < 0 || act_shift < 0 || act_shift > 8 || threads < 0)
        return fail(nullptr, UMX_ERR_INVALID, "umx_test_infer_plan: bad arguments");
    *needed = 0;
    for (int k = 0; k < nbatches; ++k)
        if (batches[k] < 1 || batches[k] > 4096) return fail(nullptr, UMX_ERR_INVALID, "umx_test_infer_plan: batch %d outside [1, 4096]", batches[k]);
    std::string why;
    int rc = check_hp(hp, &why);
    if (rc) return fail(nullptr, rc, "%s", why.c_str());
    if (blob_floats != blob_floats_needed(*hp))
        return fail(nullptr, UMX_ERR_BLOB, "weight blob has %zu floats, the graph needs %zu", blob_floats, blob_floats_needed(*hp));
    auto set = [](const char* s) { return s && *s ? s : nullptr; };
    PlanSwitches sw = plan_switches_parse(set(nt), set(override_list), nullptr, false, set(stamps));
    sw.threads = threads;
    ModelPlan m;
    if ((rc = plan_model(*hp, blob, true, f6 != 0, act_shift, sw, &m, &why))) return fail(nullptr, rc, "%s", why.c_str());
    std::string out;
    for (size_t li = 0; li < m.plan.size(); ++li) {
        Launch& L = m.plan[li];
        if (L.head) continue;
        const HostPlan& P = m.hplans[li];
        adopt_plan(L, P);
        std::string line = plan_describe(L, P);
        line.pop_back();
        for (size_t at; (at = line.find('\n')) != std::string::npos;) line.replace(at, 1, " | ");
        const Buffer& db = m.bufs[L.dst];
        char b[256];
        snprintf(b, sizeof b, " || %s, dst f32 %d planar %d Cs %d, nt16 %d, wshift %d, digest %016llx,", L.kernel.c_str(), db.as_f32 ? 1 : 0,
                 db.planar ? 1 : 0, db.Cs, P.nt16, P.wshift, infer_digest(P));
        line += b;
        for (int k = 0; k < nbatches; ++k) {
            const LaunchShape sh = launch_shape(L, P.h, batches[k]);
            snprintf(b, sizeof b, " %d:%d/%d", batches[k], sh.xcd_order, sh.tiles_per_xcd);
            line += b;
        }
        out += line + "\n";
    }
    *needed = out.size() + 1;
    if (cap < *needed) return fail(nullptr, UMX_ERR_INVALID, "umx_test_infer_plan: the text takes %zu bytes", *needed);
    memcpy(text, out.c_str(), *needed);
    return UMX_OK;
}

// The trainer's weight-gradient planner and kernel selection on one layer (umx_wgrad.hip), host only: wgrad_setup, then wgrad_select on
// operands with or without planes, as the plan's UMX_DEBUG_PLAN text + the instantiation, its grid, its LDS bytes and the scale handling
int umx_test_wgrad_plan(int B, int H, int Cxt, int Cx, int Cg, int nslab, const int* dy, const int* dx, const int* mslab, const int* coff,
                        int f32_route, int planes, int XCs, int GCs, char* line, size_t cap) {
    if (!dy || !dx || !mslab || !coff || !line || nslab < 1 || nslab > kWgMaxSlabs)
        return fail(nullptr, UMX_ERR_INVALID, "umx_test_wgrad_plan: bad arguments");
    WgradPlan w;
    memset(&w, 0, sizeof w);
    w.B = B; w.H = H; w.W = H;
    w.Cxt = Cxt; w.Cx = Cx; w.Cg = Cg;
    w.nslab = nslab;
    for (int s = 0; s < nslab; ++s) {
        w.dy[s] = (short)dy[s]; w.dx[s] = (short)dx[s]; w.mslab[s] = (short)mslab[s];
        w.coff[s] = coff[s];
    }
    std::string why;
    if (!wgrad_setup(&w, f32_route != 0, &why)) return fail(nullptr, UMX_ERR_INVALID, "%s", why.c_str());
    WgradOperands o = {};
    o.planes = planes != 0 && w.f16 && Cxt <= XCs && Cg <= GCs;   // (as the trainer's run_wgrad decides it)
    o.XCs = XCs; o.GCs = GCs;
    const WgradLaunch l = wgrad_select(w, o);
    static const char* const scales[] = {"none", "max words", "plane inverse scales"};
    char b[256];
    snprintf(b, sizeof b, ", %s, launch %u x %u x %u, lds %zu, scales %s", l.name, l.grid.x, l.grid.y, l.grid.z, l.lds, scales[l.scales]);
    const std::string text = wgrad_describe(w, "test") + b;
    if (text.size() + 1 > cap) return fail(nullptr, UMX_ERR_INVALID, "umx_test_wgrad_plan: the line takes %zu bytes", text.size() + 1);
    memcpy(line, text.c_str(), text.size() + 1);
    return UMX_OK;
}

int umx_describe_graph(const umx_hparams* hp, char* json, size_t cap, size_t* needed) {
    std::string why;
    int rc = check_hp(hp, &why);
    if (rc) return fail(nullptr, rc, "%s", why.c_str());
    std::vector<Launch> plan;
    std::vector<std::pair<int, int>> geom;
    build_graph(*hp, nullptr, &plan, nullptr, &geom, nullptr);
    std::string o = "{";
    char b[256];
    snprintf(b, sizeof b, "\"bn_epsilon\": %.9g, \"leaky_slope\": %.9g, \"buffers\": [", kBnEpsilon, (double)kLeakySlope);
    o += b;
    for (size_t i = 0; i < geom.size(); ++i) {
        snprintf(b, sizeof b, "%s{\"id\": %zu, \"size\": %d, \"channels\": %d}", i ? ", " : "", i, geom[i].first, geom[i].second);
        o += b;
    }
    o += "], \"launches\": [";
    for (size_t li = 0; li < plan.size(); ++li) {
        const Launch& L = plan[li];
        static const char* acts[] = {"none", "relu", "leaky_relu"};
        static const char* bns[] = {"none", "before_activation", "after_activation"};
        snprintf(b, sizeof b, "%s{\"name\": \"%s\", \"kind\": \"%s\", \"size\": %d, \"out_channels\": %d, \"dst\": %d, "
                              "\"max_pool\": %d, \"activation\": \"%s\", \"batch_norm\": \"%s\", \"stride\": %d, "
                              "\"summed_shortcut_ks\": %d, \"groups\": [",
                 li ? ", " : "", L.name.c_str(), L.head ? "head_softmax" : L.o_mul == 2 ? "conv_transpose" : "conv", L.H,
                 L.head ? L.head_K : L.Cout, L.dst, L.pool ? 2 : 0, L.head ? "softmax" : acts[L.act], bns[L.bn], L.o_mul, L.summed_shortcut);
        o += b;
        for (int gi = 0; gi < L.ngroups; ++gi) {
            size_t ntaps = 0;
            for (int ph = 0; ph < (L.head ? 0 : L.nphase); ++ph) ntaps += L.g[gi].taps[ph].size();
            int ks = 1;
            while ((size_t)ks * ks < ntaps) ++ks;
            snprintf(b, sizeof b, "%s{\"src\": %d, \"channels\": %d, \"ks\": %d}", gi ? ", " : "", L.g[gi].src, L.g[gi].C, L.head ? 1 : ks);
            o += b;
        }
        o += "]}";
    }
    o += "]}";
    if (needed) *needed = o.size() + 1;
    if (!json || cap < o.size() + 1) return json ? fail(nullptr, UMX_ERR_INVALID, "umx_describe_graph: %zu bytes needed", o.size() + 1) : UMX_OK;
    memcpy(json, o.c_str(), o.size() + 1);
    return UMX_OK;
}

int umx_create(const umx_hparams* hp, const float* weight_blob, size_t blob_floats, int device_ordinal, int max_batch,
               umx_ctx** out) {
    umx_options o;
    memset(&o, 0, sizeof o);
    o.device_ordinal = device_ordinal;
    o.max_batch = max_batch;
    o.precision = UMX_PREC_DEFAULT;
    o.act_shift = -1;
    return umx_create_opts(hp, weight_blob, blob_floats, &o, out);
}

int umx_create_opts(const umx_hparams* hp, const float* weight_blob, size_t blob_floats, const umx_options* opts,
                    umx_ctx** out) {
    if (!out) return fail(nullptr, UMX_ERR_INVALID, "out is NULL");
    *out = nullptr;
    if (!opts) return fail(nullptr, UMX_ERR_INVALID, "opts is NULL");
    DevArena guard;   // UMX_DEBUG_GUARD, read by every attempt of the cascade below (each is a call of this function)
    {
        std::string bad;
        if (arena_init(&guard, &bad) != UMX_OK) return fail(nullptr, UMX_ERR_INVALID, "%s", bad.c_str());
    }
    if (opts->precision == UMX_PREC_DEFAULT && !getenv("UMX_PRECISION")) {
        // default = split precision where its planner covers every layer, else the exact-fp32 MFMA kernels (tiny layers
        // under big filters exceed the LDS image of conv_f16x3).  Both are HIP paths; there is no CPU fallback.
        umx_options o2 = *opts;
        o2.precision = UMX_PREC_F16X3_F6;   // (= UMX_PREC_F16X3 for every model without wide low-resolution layers)
        int rc = umx_create_opts(hp, weight_blob, blob_floats, &o2, out);
        if (rc != UMX_ERR_INVALID) return rc;
        o2.precision = UMX_PREC_F16X3;
        rc = umx_create_opts(hp, weight_blob, blob_floats, &o2, out);
        if (rc != UMX_ERR_INVALID) return rc;
        const std::string first = g_err;
        o2.precision = UMX_PREC_F32;
        rc = umx_create_opts(hp, weight_blob, blob_floats, &o2, out);
        if (rc) g_err = first + "; fp32 kernels: " + g_err;
        // not silently: the exact-fp32 engine is ~4.6 x slower.  The note is what umx_last_error(ctx) returns until an error replaces it
        else (*out)->err = "note: UMX_PREC_DEFAULT runs this model on the exact-fp32 engine, about 4.6 x slower than the split-precision "
                           "kernels, whose planner refused it (" + first + ")";
        return rc;
    }
    const int device_ordinal = opts->device_ordinal, max_batch = opts->max_batch;
    int precision = opts->precision;
    if (precision == UMX_PREC_DEFAULT) {
        const char* e = getenv("UMX_PRECISION");
        precision = (e && !strcmp(e, "f32")) ? UMX_PREC_F32 : (e && !strcmp(e, "f16x3")) ? UMX_PREC_F16X3 : UMX_PREC_F16X3_F6;
    }
    if (precision != UMX_PREC_F32 && precision != UMX_PREC_F16X3 && precision != UMX_PREC_F16X3_F6)
        return fail(nullptr, UMX_ERR_INVALID, "unknown precision %d", precision);
    const bool f6 = precision == UMX_PREC_F16X3_F6;   // (internally: the split-precision engine with a flag)
    if (f6) precision = UMX_PREC_F16X3;
    int act_shift = opts->act_shift;
    if (act_shift < 0) {
        const char* e = getenv("UMX_ACT_SHIFT");
        act_shift = e ? atoi(e) : 0;
    }
    if (act_shift < 0 || act_shift > 8) return fail(nullptr, UMX_ERR_INVALID, "act_shift must be in [0,8]");
    std::string why;
    int rc = check_hp(hp, &why);
    if (rc) return fail(nullptr, rc, "%s", why.c_str());
    if (!weight_blob) return fail(nullptr, UMX_ERR_INVALID, "weight_blob is NULL");
    if (max_batch < 1) return fail(nullptr, UMX_ERR_INVALID, "max_batch must be >= 1");
    const size_t need = blob_floats_needed(*hp);
    if (need != blob_floats)
        return fail(nullptr, UMX_ERR_BLOB, "weight blob has %zu floats, the graph needs %zu", blob_floats, need);
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1)
        return fail(nullptr, UMX_ERR_NO_DEVICE, "no HIP device available (libumx has no CPU fallback)");
    if (device_ordinal < 0 || device_ordinal >= ndev)
        return fail(nullptr, UMX_ERR_INVALID, "device ordinal %d out of range (%d devices)", device_ordinal, ndev);
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device_ordinal) != hipSuccess)
        return fail(nullptr, UMX_ERR_HIP, "hipGetDeviceProperties failed");
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(nullptr, UMX_ERR_NO_DEVICE, "device %d is %s; libumx is built for gfx950 only", device_ordinal,
                    prop.gcnArchName);

    const bool f16 = precision == UMX_PREC_F16X3;
    ModelPlan mp;
    const PlanSwitches sw = plan_switches_from_env();
    if ((rc = plan_model(*hp, weight_blob, f16, f6, act_shift, sw, &mp, &why))) return fail(nullptr, rc, "%s", why.c_str());
    if (mp.pos != blob_floats) return fail(nullptr, UMX_ERR_BLOB, "internal blob walk mismatch");

    std::unique_ptr<umx_ctx> ctx(new umx_ctx());
    ctx->ncu = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    ctx->hp = *hp;
    ctx->device = device_ordinal;
    ctx->max_batch = max_batch;
    ctx->precision = precision;
    ctx->f6 = f6;
    ctx->act_shift = act_shift;
    ctx->stamps = sw.stamps;
    ctx->mem.fill = guard.fill;
    ctx->plan = std::move(mp.plan);
    ctx->bufs = std::move(mp.bufs);
    umx_ctx* c = ctx.get();
    HIP_TRY(nullptr, hipSetDevice(device_ordinal));
    HIP_TRY(nullptr, hipStreamCreateWithFlags(&c->own_stream, hipStreamNonBlocking));
    c->stream = c->own_stream;
    auto bail = [&](int code) { std::string m = c->err; umx_destroy(ctx.release()); g_err = m; return code; };
    {
        int lanes = opts->lanes;
        if (lanes == 0) lanes = 1;   // two lanes measured neutral on MI355X: off by default
        if (lanes < 1 || lanes > 2) { c->err = "lanes must be 1 or 2"; return bail(UMX_ERR_INVALID); }
        c->nlanes = lanes;
    }
    if (c->nlanes == 2) {
        if (hipStreamCreateWithFlags(&c->stream2, hipStreamNonBlocking) != hipSuccess ||
            hipEventCreateWithFlags(&c->ev_fork, hipEventDisableTiming) != hipSuccess ||
            hipEventCreateWithFlags(&c->ev_join, hipEventDisableTiming) != hipSuccess) {
            c->err = "creating the second lane's stream/events failed";
            return bail(UMX_ERR_HIP);
        }
        c->bufs2 = c->bufs;
    }
    for (std::vector<Buffer>* set : {&c->bufs, &c->bufs2})
        for (Buffer& B : *set) {
            // (hi, lo) binary16 planes with Cs channels take 4*Cs bytes per pixel
            const size_t bytes_per_tile = B.as_f32 ? B.floats_per_tile * sizeof(float) : (size_t)B.S * B.S * B.Cs * 4;
            const int id = (int)(&B - set->data());
            std::string label = std::string(set == &c->bufs ? "bufs[" : "bufs2[") + std::to_string(id) + (id ? "]" : "] input tiles");
            for (const Launch& L : c->plan)
                if (L.dst == id) label += " <- " + L.name;
            void* d = nullptr;
            if ((rc = dev_alloc(c, &d, bytes_per_tile * (size_t)max_batch, label, true))) return bail(rc);
            B.d = (float*)d;
        }
    if (f16) {
        void* d = nullptr;
        if ((rc = dev_alloc(c, &d, c->bufs[0].floats_per_tile * sizeof(float) * (size_t)max_batch, "d_tiles32", true))) return bail(rc);
        c->d_tiles32 = (float*)d;
        if (c->nlanes == 2) {
            if ((rc = dev_alloc(c, &d, c->bufs[0].floats_per_tile * sizeof(float) * (size_t)max_batch, "d_tiles32_2", true))) return bail(rc);
            c->d_tiles32_2 = (float*)d;
        }
        if ((rc = dev_alloc(c, &d, 256, "d_zeros", false))) return bail(rc);
        c->d_zeros = (uint4*)d;
        if ((rc = dev_alloc(c, &d, 256, "d_flag", false))) return bail(rc);
        c->d_flag = (int*)d;
        if (hipMemset(c->d_zeros, 0, 256) != hipSuccess || hipMemset(c->d_flag, 0, 256) != hipSuccess) {
            c->err = "hipMemset failed";
            return bail(UMX_ERR_HIP);
        }
    }
    for (size_t li = 0; li < c->plan.size(); ++li) {
        Launch& L = c->plan[li];
        if (f16 && !L.head) {
            if ((rc = upload_plan(c, L, mp.hplans[li]))) return bail(rc);
            mp.hplans[li] = HostPlan();
            if (L.hcp.f6) c->f6_used = true;
            if (L.hcp.head_K > 0) {
                c->head_fused = true;
                const Launch& Hd = c->plan.back();
                L.flops += Hd.flops;
                L.bytes += 4.0 * Hd.H * Hd.W * Hd.head_K - 4.0 * L.outH * L.outW * L.Cout;   // probabilities out, no fp32 tensor
            }
            for (int ph = 0; ph < L.nphase; ++ph)
                for (int gi = 0; gi < L.ngroups; ++gi) std::vector<float>().swap(L.g[gi].packed[ph]);
            continue;
        }
        if ((rc = upload_raw(c, L.pre_s, &L.d_pre_s, L.name + " pre_s")) || (rc = upload_raw(c, L.pre_b, &L.d_pre_b, L.name + " pre_b")) ||
            (rc = upload_raw(c, L.post_s, &L.d_post_s, L.name + " post_s")) || (rc = upload_raw(c, L.post_b, &L.d_post_b, L.name + " post_b")))
            return bail(rc);
        if (L.head) {
            if ((rc = upload_raw(c, L.head_w, &L.d_head_w, L.name + " head_w"))) return bail(rc);
            continue;
        }
        for (int ph = 0; ph < L.nphase; ++ph)
            for (int gi = 0; gi < L.ngroups; ++gi) {
                float* d = nullptr;
                if ((rc = upload_raw(c, L.g[gi].packed[ph], &d, L.name + " weights[" + std::to_string(ph) + "][" + std::to_string(gi) + "]")))
                    return bail(rc);
                L.cp.ph[ph].w[gi] = d;
                std::vector<float>().swap(L.g[gi].packed[ph]);
            }
        L.cp.pre_s = L.d_pre_s; L.cp.pre_b = L.d_pre_b; L.cp.post_s = L.d_post_s; L.cp.post_b = L.d_post_b;
    }
    for (const Launch& L : c->plan)   // compact input tiles: the graph folded the raw skip (and so the first layer runs on the dense-K kernel)
        if (L.app_src == 0) c->in_cw = c->hp.nChannels == 1 ? 1 : c->hp.nChannels == 2 ? 2 : 4;
    if (c->mem.fill >= 0)
        fprintf(stderr, "[umx] UMX_DEBUG_GUARD=0x%02x: %zu engine buffers between red zones\n", c->mem.fill, c->mem.blocks.size());
    *out = ctx.release();
    return UMX_OK;
}

int umx_precision_of(const umx_ctx* ctx) { return !ctx ? UMX_PREC_DEFAULT : ctx->f6_used ? UMX_PREC_F16X3_F6 : ctx->precision; }

void umx_destroy(umx_ctx* ctx) {
    if (!ctx) return;
    hipSetDevice(ctx->device);
    // drain everything that may still touch the context's buffers (or a communicator's) before anything is released
    if (ctx->stream) hipStreamSynchronize(ctx->stream);
    if (ctx->stream2) hipStreamSynchronize(ctx->stream2);
    if (ctx->up_stream) hipStreamSynchronize(ctx->up_stream);
    if (ctx->dn_stream) hipStreamSynchronize(ctx->dn_stream);
    shard_release(ctx);   // a communicator / buffers umx_shard_init attached to this context
    for (auto& pe : ctx->pending) { hipEventDestroy(pe.a); hipEventDestroy(pe.b); }
    for (auto e : ctx->free_events) hipEventDestroy(e);
    arena_free(&ctx->mem);   // every device buffer: the create-time ones, the grown ones and the host slots'
    if (ctx->up_stream) { hipStreamSynchronize(ctx->up_stream); hipStreamDestroy(ctx->up_stream); }
    if (ctx->dn_stream) { hipStreamSynchronize(ctx->dn_stream); hipStreamDestroy(ctx->dn_stream); }
    for (auto& h : ctx->hs) {
        for (auto e : h.events) hipEventDestroy(e);
        if (h.done) hipEventDestroy(h.done);
        if (h.flag_host) hipHostFree(h.flag_host);
    }
    if (ctx->stream2) { hipStreamSynchronize(ctx->stream2); hipStreamDestroy(ctx->stream2); }
    if (ctx->ev_fork) hipEventDestroy(ctx->ev_fork);
    if (ctx->ev_join) hipEventDestroy(ctx->ev_join);
    if (ctx->own_stream) hipStreamDestroy(ctx->own_stream);
    delete ctx;
}

int umx_set_stream(umx_ctx* ctx, void* hip_stream) {
    if (!ctx) return fail(nullptr, UMX_ERR_INVALID, "ctx is NULL");
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    ctx->stream = hip_stream ? (hipStream_t)hip_stream : ctx->own_stream;
    return UMX_OK;
}

int umx_synchronize(umx_ctx* ctx) {
    if (!ctx) return fail(nullptr, UMX_ERR_INVALID, "ctx is NULL");
    return guarded(ctx, false, true, [&]() -> int {
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        return check_range_flag(ctx);
    });
}

int umx_forward_tiles_dev(umx_ctx* ctx, const float* tiles_dev, int n, float* probs_dev) {
    if (!ctx) return fail(nullptr, UMX_ERR_INVALID, "ctx is NULL");
    if (n < 0 || (n > 0 && (!tiles_dev || !probs_dev))) return fail(ctx, UMX_ERR_INVALID, "bad tiles/probs/n");
    return guarded(ctx, true, true, [&]() -> int {
        HIP_TRY(ctx, hipSetDevice(ctx->device));
        const size_t P = ctx->hp.imSize;
        const size_t tile_f = P * P * ctx->hp.nChannels, prob_f = P * P * ctx->hp.nClasses;
        LaneLoop ll(ctx, n);
        Lane lane;
        for (int i = 0, nb; i < n; i += nb) {
            nb = ll.next(n - i, &lane);
            int rc = run_unet(ctx, lane, tiles_dev + (size_t)i * tile_f, nb, probs_dev + (size_t)i * prob_f);
            if (rc) return rc;
        }
        return ll.join();
    });
}

int umx_forward_tiles(umx_ctx* ctx, const float* tiles_host, int n, float* probs_host) {
    if (!ctx) return fail(nullptr, UMX_ERR_INVALID, "ctx is NULL");
    if (n < 0 || (n > 0 && (!tiles_host || !probs_host))) return fail(ctx, UMX_ERR_INVALID, "bad tiles/probs/n");
    if (n == 0) return UMX_OK;
    return guarded(ctx, true, true, [&]() -> int {
        HIP_TRY(ctx, hipSetDevice(ctx->device));
        const size_t P = ctx->hp.imSize;
        const size_t tile_b = P * P * ctx->hp.nChannels * sizeof(float), prob_b = P * P * ctx->hp.nClasses * sizeof(float);
        int rc;
        if ((rc = grow(ctx, (void**)&ctx->d_io_tiles, &ctx->io_tiles_cap, tile_b * n, "d_io_tiles"))) return rc;
        if ((rc = grow(ctx, (void**)&ctx->d_io_probs, &ctx->io_probs_cap, prob_b * n, "d_io_probs"))) return rc;
        HIP_TRY(ctx, hipMemcpyAsync(ctx->d_io_tiles, tiles_host, tile_b * n, hipMemcpyHostToDevice, ctx->stream));
        if ((rc = umx_forward_tiles_dev(ctx, ctx->d_io_tiles, n, ctx->d_io_probs))) return rc;
        HIP_TRY(ctx, hipMemcpyAsync(probs_host, ctx->d_io_probs, prob_b * n, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        return check_range_flag(ctx);
    });
}

int umx_tile_grid(const umx_ctx* ctx, int H, int W, int* patch_rows, int* patch_cols, int* padded_rows,
                  int* padded_cols) {
    if (!ctx || H < 1 || W < 1) return fail(nullptr, UMX_ERR_INVALID, "bad ctx/H/W");
    const TileGeom g = geom_of(ctx->hp, H, W);
    if (patch_rows) *patch_rows = g.npr;
    if (patch_cols) *patch_cols = g.npc;
    if (padded_rows) *padded_rows = g.npr * g.sub + 2 * g.margin;
    if (padded_cols) *padded_cols = g.npc * g.sub + 2 * g.margin;
    return UMX_OK;
}

int umx_band_tiles_dev(umx_ctx* ctx, const double* image_dev, int C_img, int H, int W, int band_row0, int band_rows,
                       double mean, double stdv, int pr0, int pr1, float* probs_dev) {
    if (!ctx) return fail(nullptr, UMX_ERR_INVALID, "ctx is NULL");
    if (!image_dev || !probs_dev || H < 1 || W < 1) return fail(ctx, UMX_ERR_INVALID, "bad image/probs/H/W");
    if (C_img != 1 && C_img != ctx->hp.nChannels)
        return fail(ctx, UMX_ERR_INVALID, "image has %d channels, model wants 1 or %d", C_img, ctx->hp.nChannels);
    if (!(stdv != 0.0)) return fail(ctx, UMX_ERR_INVALID, "std must be non-zero");
    const TileGeom g = geom_of(ctx->hp, H, W);
    if (pr0 < 0 || pr1 > g.npr || pr0 > pr1) return fail(ctx, UMX_ERR_INVALID, "patch rows [%d,%d) outside [0,%d)", pr0, pr1, g.npr);
    if (pr0 == pr1) return UMX_OK;
    // image rows the patch rows touch: [pr0*sub - m, (pr1-1)*sub + P - m) clipped to the image
    const int need0 = std::max(0, pr0 * g.sub - g.margin), need1 = std::min(H, (pr1 - 1) * g.sub + g.P - g.margin);
    if (band_row0 < 0 || band_rows < 0 || (need1 > need0 && (band_row0 > need0 || band_row0 + band_rows < need1)))
        return fail(ctx, UMX_ERR_INVALID, "band rows [%d,%d) do not cover the rows [%d,%d) the patch rows need",
                    band_row0, band_row0 + band_rows, need0, need1);
    return guarded(ctx, true, true, [&]() -> int {
        HIP_TRY(ctx, hipSetDevice(ctx->device));
        return tiles_range(ctx, image_dev, C_img, g, band_row0, band_rows, mean, stdv, pr0 * g.npc, pr1 * g.npc, probs_dev);
    });
}

int umx_stitch_dev(umx_ctx* ctx, const float* probs_dev, int tpr0, int tpr1, int H, int W, int mode, int stitch, int y0,
                   int y1, void* out_dev) {
    if (!ctx) return fail(nullptr, UMX_ERR_INVALID, "ctx is NULL");
    if (stitch != UMX_STITCH_FP16_COMPAT && stitch != UMX_STITCH_FP32) return fail(ctx, UMX_ERR_INVALID, "bad stitch %d", stitch);
    return guarded(ctx, true, true, [&]() -> int { return umx::stitch_rows(ctx, probs_dev, tpr0, tpr1, H, W, mode, stitch, y0, y1, out_dev, 0); });
}

}  // extern "C"

namespace umx {
// (umx_stitch_dev + the internal forms: stitch = kStitchU8 writes the drivers' uint8 planes, plane_rows > 0 a padded destination)
int stitch_rows(umx_ctx* ctx, const float* probs_dev, int tpr0, int tpr1, int H, int W, int mode, int stitch, int y0, int y1,
                void* out_dev, int plane_rows) {
    if (!probs_dev || !out_dev || H < 1 || W < 1) return fail(ctx, UMX_ERR_INVALID, "bad probs/out/H/W");
    if (mode != UMX_MODE_ACCUMULATE && mode != UMX_MODE_REPLACE) return fail(ctx, UMX_ERR_INVALID, "bad mode %d", mode);
    const TileGeom g = geom_of(ctx->hp, H, W);
    if (y0 < 0 || y1 > H || y0 > y1) return fail(ctx, UMX_ERR_INVALID, "rows [%d,%d) outside the image", y0, y1);
    if (y0 == y1) return UMX_OK;
    // patch rows touching image rows [y0,y1): padded rows R = y + m; pr*sub <= R < pr*sub + P
    const int R0 = y0 + g.margin, R1 = y1 - 1 + g.margin;
    const int need_lo = (R0 - g.P + 1 <= 0) ? 0 : (R0 - g.P + g.sub) / g.sub;  // ceil((R0-P+1)/sub)
    const int need_hi = std::min(g.npr - 1, R1 / g.sub);
    if (tpr0 > need_lo || tpr1 <= need_hi || tpr0 < 0 || tpr1 > g.npr)
        return fail(ctx, UMX_ERR_INVALID, "tile rows [%d,%d) do not cover the patch rows [%d,%d] touching image rows [%d,%d)",
                    tpr0, tpr1, need_lo, need_hi, y0, y1);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (ctx->site_stitch < 0) ctx->site_stitch = site_of(ctx, "pi2d.stitch", "stitch");
    const int K = ctx->hp.nClasses;
    ProfScope ps(ctx, ctx->stream, ctx->site_stitch, 0.0,
                 (double)(y1 - y0) * W * K * (4.0 * ((double)g.P / g.sub) * ((double)g.P / g.sub) + (stitch == 0 ? 2.0 : stitch == kStitchU8 ? 1.0 : 4.0)));
    HIP_TRY(ctx, launch_stitch(probs_dev, tpr0, tpr1, g, K, mode, stitch, y0, y1, out_dev, ctx->stream, plane_rows));
    return UMX_OK;
}
}  // namespace umx

extern "C" {

int umx_infer_image_dev(umx_ctx* ctx, const double* image_dev, int C_img, int H, int W, double mean, double stdv,
                        int mode, int stitch, void* out_dev) {
    if (!ctx) return fail(nullptr, UMX_ERR_INVALID, "ctx is NULL");
    if (H < 1 || W < 1) return fail(ctx, UMX_ERR_INVALID, "bad H/W");
    const TileGeom g = geom_of(ctx->hp, H, W);
    const size_t prob_b = (size_t)g.npr * g.npc * g.P * g.P * ctx->hp.nClasses * sizeof(float);
    return guarded(ctx, true, true, [&]() -> int {
        int rc;
        HIP_TRY(ctx, hipSetDevice(ctx->device));
        if ((rc = grow(ctx, (void**)&ctx->d_probs, &ctx->probs_cap, prob_b, "d_probs"))) return rc;
        if ((rc = umx_band_tiles_dev(ctx, image_dev, C_img, H, W, 0, H, mean, stdv, 0, g.npr, ctx->d_probs))) return rc;
        return umx_stitch_dev(ctx, ctx->d_probs, 0, g.npr, H, W, mode, stitch, 0, H, out_dev);
    });
}

int umx_profile_enable(umx_ctx* ctx, int on) {
    if (!ctx) return fail(nullptr, UMX_ERR_INVALID, "ctx is NULL");
    int rc = prof_fold(ctx);
    if (rc) return rc;
    ctx->prof = on < 0 ? 0 : on;
    for (auto& s : ctx->sites) { s.launches = 0; s.seen = 0; s.total_ms = 0; s.flops = 0; s.bytes = 0; s.exec = 0; }
    return UMX_OK;
}

int umx_profile_read(umx_ctx* ctx, umx_prof_entry* entries, int max_entries, int* n_entries) {
    if (!ctx || !n_entries) return fail(ctx, UMX_ERR_INVALID, "bad arguments");
    int rc = prof_fold(ctx);
    if (rc) return rc;
    int n = 0;
    for (auto& s : ctx->sites) {
        if (s.launches == 0) continue;
        if (entries && n < max_entries) {
            umx_prof_entry& e = entries[n];
            memset(&e, 0, sizeof e);
            snprintf(e.name, sizeof e.name, "%s", s.name.c_str());
            snprintf(e.kernel, sizeof e.kernel, "%s", s.kernel.c_str());
            e.launches = s.launches;
            e.total_ms = s.total_ms;
            e.flops_per_launch_sum = s.flops;
            e.bytes_per_launch_sum = s.bytes;
            e.exec_flops_sum = s.exec;
            e.launches_seen = s.seen;
            e.xcd_order = s.xcd_order;
        }
        ++n;
    }
    *n_entries = n;
    return UMX_OK;
}

}  // extern "C"

