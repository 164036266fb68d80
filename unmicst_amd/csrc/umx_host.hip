// Host pipeline of libumx: the entry points that take host arrays (reference seam UnMicst1-5.py:687-710 and the drivers'
// pre/post-processing around it, :807-854), with uploads / downloads overlapped with the tile kernels.
#include "umx_internal.h"

#include <limits>
#include <thread>

using namespace umx;

// (min, max) of a host plane in one pass on a few threads -- what np.min / np.max over the page cost the reference's driver
// (UnMicst1-5.py:817-821) twice; the loops are plain enough for the host compiler to vectorise (AVX2 where the CPU has it)
namespace {
template <class T>
__attribute__((target("avx2"))) void range_avx2(const T* x, size_t n, uint32_t* lo, uint32_t* hi) {
    T a = std::numeric_limits<T>::max(), b = 0;
    for (size_t i = 0; i < n; ++i) { a = x[i] < a ? x[i] : a; b = x[i] > b ? x[i] : b; }
    *lo = a; *hi = b;
}
template <class T>
void range_plain(const T* x, size_t n, uint32_t* lo, uint32_t* hi) {
    T a = std::numeric_limits<T>::max(), b = 0;
    for (size_t i = 0; i < n; ++i) { a = x[i] < a ? x[i] : a; b = x[i] > b ? x[i] : b; }
    *lo = a; *hi = b;
}
template <class T>
void range_threads(const T* x, size_t n, uint32_t* out) {
    static const bool avx2 = __builtin_cpu_supports("avx2");
    unsigned nt = std::max(1u, std::min(16u, std::thread::hardware_concurrency()));
    if (const char* e = getenv("UMX_HOST_THREADS")) nt = (unsigned)std::max(1, atoi(e));
    nt = (unsigned)std::max<size_t>(1, std::min<size_t>(nt, n >> 20));   // >= 1 M samples per thread
    std::vector<uint32_t> lo(nt, 0xFFFFFFFFu), hi(nt, 0u);
    auto work = [&](unsigned t) {
        const size_t a = n * t / nt, b = n * (t + 1) / nt;
        if (avx2) range_avx2(x + a, b - a, &lo[t], &hi[t]);
        else range_plain(x + a, b - a, &lo[t], &hi[t]);
    };
    std::vector<std::thread> th;
    for (unsigned t = 1; t < nt; ++t) th.emplace_back(work, t);
    work(0);
    for (auto& t : th) t.join();
    out[0] = *std::min_element(lo.begin(), lo.end());
    out[1] = *std::max_element(hi.begin(), hi.end());
}
}  // namespace

namespace umx {

int check_image(umx_ctx* ctx, bool ptrs, int C_img, int H, int W, bool raw, int bits, double stdv, int mode, int stitch,
                const uint32_t* range) {
    if (!ctx) return fail(nullptr, UMX_ERR_INVALID, "ctx is NULL");
    if (!ptrs || H < 1 || W < 1 || C_img < 1) return fail(ctx, UMX_ERR_INVALID, "bad image/out/H/W");
    if (raw && bits != 8 && bits != 16) return fail(ctx, UMX_ERR_INVALID, "raw planes must be uint8 or uint16 (bits = %d)", bits);
    if (C_img != 1 && C_img != ctx->hp.nChannels)
        return fail(ctx, UMX_ERR_INVALID, "image has %d channels, model wants 1 or %d", C_img, ctx->hp.nChannels);
    if (!(stdv != 0.0)) return fail(ctx, UMX_ERR_INVALID, "std must be non-zero");
    if (mode != UMX_MODE_ACCUMULATE && mode != UMX_MODE_REPLACE) return fail(ctx, UMX_ERR_INVALID, "bad mode %d", mode);
    if (stitch != UMX_STITCH_FP16_COMPAT && stitch != UMX_STITCH_FP32) return fail(ctx, UMX_ERR_INVALID, "bad stitch %d", stitch);
    const uint32_t top = bits == 8 ? 255u : 65535u;
    for (int c = 0; range && c < C_img; ++c)
        if (range[2 * c] > range[2 * c + 1] || range[2 * c + 1] > top)
            return fail(ctx, UMX_ERR_INVALID, "plane %d: range (%u, %u) is not a (min, max) of %d-bit samples", c, range[2 * c],
                        range[2 * c + 1], bits);
    return UMX_OK;
}

int slot_submit(umx_ctx* ctx, int slot, const std::function<int()>& enqueue) {
    if (slot < 0 || slot > 1) return fail(ctx, UMX_ERR_INVALID, "slot must be 0 or 1");
    if (ctx->hs[slot].busy) return fail(ctx, UMX_ERR_INVALID, "slot %d still holds a submitted call: wait for it first", slot);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    umx_ctx::HostSlot& hs = ctx->hs[slot];
    auto begin = [&]() -> int {
        if (!hs.done) {
            HIP_TRY(ctx, hipEventCreateWithFlags(&hs.done, hipEventDisableTiming));
            HIP_TRY(ctx, hipHostMalloc((void**)&hs.flag_host, 64, hipHostMallocDefault));
        }
        if (!ctx->up_stream) {
            HIP_TRY(ctx, hipStreamCreateWithFlags(&ctx->up_stream, hipStreamNonBlocking));
            HIP_TRY(ctx, hipStreamCreateWithFlags(&ctx->dn_stream, hipStreamNonBlocking));
        }
        // this call's range flag: its own word, cleared in stream order in front of its kernels
        const int fw = 16 * (slot + 1);
        if (ctx->d_flag) HIP_TRY(ctx, hipMemsetAsync(ctx->d_flag + fw, 0, sizeof(int), ctx->stream));
        ctx->flag_word = fw;
        return enqueue();
    };
    const int rc = begin();
    ctx->flag_word = 0;
    if (rc) {
        // an error in the middle of enqueueing: transfers that reference the caller's buffers and this slot's device buffers may
        // be in flight -- drain them before the caller (or the next submit) frees or reuses anything
        const std::string msg = ctx->err;
        if (ctx->up_stream) hipStreamSynchronize(ctx->up_stream);
        hipStreamSynchronize(ctx->stream);
        if (ctx->dn_stream) hipStreamSynchronize(ctx->dn_stream);
        ctx->err = msg;
    }
    return rc;
}

int slot_finish(umx_ctx* ctx, int slot, hipStream_t dn_s) {
    umx_ctx::HostSlot& hs = ctx->hs[slot];
    if (ctx->d_flag)
        HIP_TRY(ctx, hipMemcpyAsync(hs.flag_host, ctx->d_flag + 16 * (slot + 1), sizeof(int), hipMemcpyDeviceToHost, dn_s));
    else
        *hs.flag_host = 0;
    HIP_TRY(ctx, hipEventRecord(hs.done, dn_s));
    hs.busy = true;
    return UMX_OK;
}

int put_range(umx_ctx* ctx, unsigned* mm, const uint32_t* range, int C_img) {
    for (int c = 0; c < C_img; ++c) {
        HIP_TRY(ctx, hipMemsetD32Async((hipDeviceptr_t)(mm + 16 * c), (int)range[2 * c], 1, ctx->stream));
        HIP_TRY(ctx, hipMemsetD32Async((hipDeviceptr_t)(mm + 16 * c + 1), (int)range[2 * c + 1], 1, ctx->stream));
    }
    return UMX_OK;
}

}  // namespace umx

extern "C" {

// ---- host entry points.  The reference hands host arrays across its seam (UnMicst1-5.py:687-710); here the slide goes up
// and the probability stack comes down in row slabs on two copy streams while the tile kernels of the neighbouring slabs
// run: slab s = patch rows [cut[s], cut[s+1]); its upload covers the image rows its tiles read that are not on the device
// yet, its download the image rows no later patch row touches.  With pinned host buffers the transfers are true DMA and
// all but the first upload and the last download ride under compute; with pageable buffers HIP stages them (still correct).
// src_bits: 0 = float64 planes (what singleImageInference receives), 8 / 16 = raw integer planes (the driver's file
// contents; im2double and, with `rescale`, rescale_intensity run on the device).  out_u8: the driver's uint8 planes
// instead of the stitch result.  A rescale needs the plane's (min, max) before the first tile: the upload then runs
// ahead of compute (min/max reduced slab by slab as the rows arrive) and only the download is hidden.
static int host_wait(umx_ctx* ctx, int slot) {
    if (slot < 0 || slot > 1) return fail(ctx, UMX_ERR_INVALID, "slot must be 0 or 1");
    umx_ctx::HostSlot& hs = ctx->hs[slot];
    if (!hs.busy) return UMX_OK;
    hs.busy = false;
    if (ctx->shard) {   // a sharded context polls its communicator while it waits
        if (const int rc = shard_wait(ctx, hs.done)) return rc;
    } else if (const hipError_t e = hipEventSynchronize(hs.done)) {
        return fail(ctx, UMX_ERR_HIP, "hipEventSynchronize failed: %s", hipGetErrorString(e));
    }
    if (*hs.flag_host)   // this slot's own flag word, cleared by the next submit on the slot in stream order
        return fail(ctx, UMX_ERR_RANGE, "an activation left the binary16 range of the split-precision path; "
                                        "create the context with UMX_PREC_F32 (or UMX_PRECISION=f32)");
    return UMX_OK;
}

// The executor of a slide's schedule (slide_plan, umx_pipeline.hip): the slot's buffers sized from the plan, its events, then the
// plan's steps in order -- their rows and tiles turned into addresses, each step one copy, launch or event per plane.
// range: the planes' (min, max) as the caller's reader found them, or NULL
static int host_enqueue(umx_ctx* ctx, int slot, bool sync_call, const void* src, int src_bits, int C_img, int H, int W, int rescale,
                        const uint32_t* range, double mean, double stdv, int mode, int stitch, int out_u8, void* out_host) {
    umx_ctx::HostSlot& hs = ctx->hs[slot];
    const TileGeom g = geom_of(ctx->hp, H, W);
    SlideSpec sp;
    sp.max_batch = ctx->max_batch;
    sp.K = ctx->hp.nClasses;
    sp.C_img = C_img;
    sp.src_bits = src_bits;
    sp.rescale = rescale;
    sp.has_range = range != nullptr;
    sp.sync_call = sync_call;
    // (read only where the plan can use it -- a synchronous call without a range: getenv walks the environment, and a submitted
    // 1024 x 1024 slide is a 1 ms call)
    sp.host_range_ok = sync_call && !range && !(getenv("UMX_HOST_RANGE") && atoi(getenv("UMX_HOST_RANGE")) == 0);
    sp.stitch_el = stitch == UMX_STITCH_FP32 ? 4 : 2;
    sp.out_u8 = out_u8;
    sp.raw_gather = src_bits != 0 && gathers_raw(ctx);
    for (const Launch& L : ctx->plan) sp.tile_flops += L.flops;
    const SlidePlan p = slide_plan(g, sp);
    int rc;
    if (p.image_b && (rc = grow(ctx, (void**)&hs.d_image, &hs.image_cap, p.image_b, slot ? "slot 1 d_image" : "slot 0 d_image"))) return rc;
    if ((rc = grow(ctx, &hs.d_out, &hs.out_cap, p.out_b, slot ? "slot 1 d_out" : "slot 0 d_out"))) return rc;
    if ((rc = grow(ctx, (void**)&hs.d_probs, &hs.probs_cap, p.probs_b, slot ? "slot 1 d_probs" : "slot 0 d_probs"))) return rc;
    while ((int)hs.events.size() < p.nev) {
        hipEvent_t ev;
        HIP_TRY(ctx, hipEventCreateWithFlags(&ev, hipEventDisableTiming));
        hs.events.push_back(ev);
    }
    const hipStream_t cs = ctx->stream, up_s = p.single ? cs : ctx->up_stream, dn_s = p.single ? cs : ctx->dn_stream;
    const size_t plane = (size_t)H * W, K = sp.K, in_b = src_bits ? (size_t)(src_bits / 8) : sizeof(double);
    const size_t el = out_u8 ? 1 : sp.stitch_el;   // element of what goes down
    unsigned char* const base = (unsigned char*)hs.d_out;
    unsigned char* const d_raw = base + p.raw_off;
    unsigned char* const d_up = src_bits ? d_raw : (unsigned char*)hs.d_image;         // where the caller's planes go up
    unsigned char* const d_res = out_u8 ? base + p.pm_b : base;                        // the result: compact slabs [K][rows][W], one after the other
    unsigned* const mm = (unsigned*)(base + p.mm_off);
    uint32_t own_range[2 * 8];
    for (const Step& st : p.steps) {
        const size_t e0 = (size_t)st.a * W, n = (size_t)(st.b - st.a) * W;             // first element and elements of rows [a, b) in a plane
        switch (st.kind) {
        case kStepUpload:
            for (int c = 0; c < C_img; ++c) {
                const size_t off = (c * plane + e0) * in_b;
                HIP_TRY(ctx, hipMemcpyAsync(d_up + off, (const unsigned char*)src + off, n * in_b, hipMemcpyHostToDevice, up_s));
            }
            if (st.c >= 0) HIP_TRY(ctx, hipEventRecord(hs.events[st.c], up_s));
            break;
        case kStepWaitUpload:
            HIP_TRY(ctx, hipStreamWaitEvent(cs, hs.events[st.a], 0));
            break;
        case kStepMinMaxInit:
            for (int c = 0; c < C_img; ++c) HIP_TRY(ctx, launch_minmax_init(mm + 16 * c, cs));
            break;
        case kStepHostRange:   // (3 ms per 537 MB plane, while the uploads enqueued so far cross the bus)
            for (int c = 0; c < C_img; ++c)
                if (umx_plane_range((const unsigned char*)src + c * plane * in_b, src_bits, plane, own_range + 2 * c) != UMX_OK)
                    return fail(ctx, UMX_ERR_INVALID, "plane range");
            range = own_range;
            break;
        case kStepPutRange:
            if ((rc = put_range(ctx, mm, range, C_img))) return rc;
            break;
        case kStepMinMax:
            for (int c = 0; c < C_img; ++c)
                HIP_TRY(ctx, launch_minmax(d_raw + (c * plane + e0) * in_b, src_bits, n, mm + 16 * c, cs));
            break;
        case kStepConvert:
            for (int c = 0; c < C_img; ++c)
                HIP_TRY(ctx, launch_raw_convert(d_raw + (c * plane + e0) * in_b, src_bits, n, rescale, mm + 16 * c, hs.d_image + c * plane + e0, cs));
            break;
        case kStepTiles:
            if ((rc = tiles_range(ctx, sp.raw_gather ? nullptr : hs.d_image, C_img, g, 0, H, mean, stdv, st.a, st.b,
                                  hs.d_probs + (size_t)st.a * g.P * g.P * K, sp.raw_gather ? d_raw : nullptr, sp.raw_gather ? src_bits : 0,
                                  sp.raw_gather && rescale ? mm : nullptr)))
                return rc;
            break;
        case kStepStitch:      // (uint8 out: the cast rides in the stitch -- no float16 slab is written and read back)
            if ((rc = stitch_rows(ctx, hs.d_probs, 0, st.c, H, W, mode, out_u8 ? kStitchU8 : stitch, st.a, st.b, d_res + K * e0 * el, 0))) return rc;
            break;
        case kStepDownloadEvent:
        case kStepFlag:
            if (st.kind == kStepFlag && !ctx->d_flag) break;
            HIP_TRY(ctx, hipEventRecord(hs.events[st.a], cs));
            HIP_TRY(ctx, hipStreamWaitEvent(dn_s, hs.events[st.a], 0));
            break;
        case kStepDownload:
            for (size_t k = 0; k < K; ++k)
                HIP_TRY(ctx, hipMemcpyAsync((unsigned char*)out_host + (k * plane + e0) * el, d_res + (K * e0 + k * n) * el, n * el,
                                            hipMemcpyDeviceToHost, dn_s));
            break;
        }
    }
    // `done` then says the call is complete (a slot's buffers are private to it and free again once host_wait has returned)
    return slot_finish(ctx, slot, dn_s);
}

// sync_call: a synchronous entry (slot 0), which also waits for the call
static int host_submit(umx_ctx* ctx, int slot, bool sync_call, const void* src, int src_bits, int C_img, int H, int W, int rescale,
                       const uint32_t* range, double mean, double stdv, int mode, int stitch, int out_u8, void* out_host) {
    return guarded(ctx, true, sync_call, [&]() -> int {   // (guard mode: a submitted call's zones are checked by its wait)
        const int rc = slot_submit(ctx, slot, [&] {
            return host_enqueue(ctx, slot, sync_call, src, src_bits, C_img, H, W, rescale, range, mean, stdv, mode, stitch, out_u8, out_host);
        });
        return rc || !sync_call ? rc : host_wait(ctx, slot);
    });
}

int umx_infer_image(umx_ctx* ctx, const double* image_host, int C_img, int H, int W, double mean, double stdv, int mode,
                    int stitch, void* out_host) {
    if (const int rc = check_image(ctx, image_host && out_host, C_img, H, W, false, 0, stdv, mode, stitch, nullptr)) return rc;
    return host_submit(ctx, 0, true, image_host, 0, C_img, H, W, 0, nullptr, mean, stdv, mode, stitch, 0, out_host);
}

int umx_infer_image_raw(umx_ctx* ctx, const void* raw_host, int bits, int C_img, int H, int W, int rescale, double mean,
                        double stdv, int mode, uint8_t* out_host) {
    if (const int rc = check_image(ctx, raw_host && out_host, C_img, H, W, true, bits, stdv, mode, UMX_STITCH_FP16_COMPAT, nullptr))
        return rc;
    return host_submit(ctx, 0, true, raw_host, bits, C_img, H, W, rescale, nullptr, mean, stdv, mode, UMX_STITCH_FP16_COMPAT, 1, out_host);
}

int umx_plane_range(const void* raw_host, int bits, size_t n, uint32_t* range) {
    if (!raw_host || !range || n == 0 || (bits != 8 && bits != 16)) return UMX_ERR_INVALID;
    if (bits == 16) range_threads(static_cast<const uint16_t*>(raw_host), n, range);
    else range_threads(static_cast<const uint8_t*>(raw_host), n, range);
    return UMX_OK;
}

int umx_infer_image_raw_range(umx_ctx* ctx, const void* raw_host, int bits, int C_img, int H, int W, const uint32_t* range,
                              double mean, double stdv, int mode, uint8_t* out_host) {
    if (const int rc = check_image(ctx, raw_host && out_host, C_img, H, W, true, bits, stdv, mode, UMX_STITCH_FP16_COMPAT, range))
        return rc;
    return host_submit(ctx, 0, true, raw_host, bits, C_img, H, W, 1, range, mean, stdv, mode, UMX_STITCH_FP16_COMPAT, 1, out_host);
}

// numpy's float64 add.reduce over a contiguous vector (what ndarray.sum() runs): sequential below 8 terms, eight accumulators
// combined pairwise up to 128 terms with the tail added in order, two halves (the first a multiple of 8) beyond
static double pairwise_sum(const double* a, size_t n) {
    if (n < 8) {
        double res = 0.0;
        for (size_t i = 0; i < n; ++i) res += a[i];
        return res;
    }
    if (n <= 128) {
        double r[8];
        for (int j = 0; j < 8; ++j) r[j] = a[j];
        size_t i = 8;
        for (; i < n - n % 8; i += 8)
            for (int j = 0; j < 8; ++j) r[j] += a[i + j];
        double res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
        for (; i < n; ++i) res += a[i];
        return res;
    }
    size_t n2 = n / 2;
    n2 -= n2 % 8;
    return pairwise_sum(a, n2) + pairwise_sum(a + n2, n - n2);
}

// The anti-aliasing weights of one axis in scipy.ndimage's operation order (_gaussian_kernel1d): radius = int(4 sigma + 0.5),
// phi = exp(c * (x * x)) with c = -0.5 / (sigma * sigma), divided by phi.sum().  wts[0] is the centre tap.  What is left to the
// platform is exp itself: numpy's and the C library's differ by an ulp on a few taps (DESIGN.md has the table).
static int gauss_weights(double sigma, std::vector<double>* wts) {
    const int radius = (int)(4.0 * sigma + 0.5);
    const double c = -0.5 / (sigma * sigma);
    std::vector<double> full(2 * (size_t)radius + 1);
    for (int x = -radius; x <= radius; ++x) full[x + radius] = std::exp(c * ((double)x * (double)x));
    const double sum = pairwise_sum(full.data(), full.size());
    wts->resize((size_t)radius + 1);
    for (int j = 0; j <= radius; ++j) (*wts)[j] = full[radius + j] / sum;
    return radius;
}

constexpr int kMaxGaussTaps = 4096;   // radius + 1 weights per axis in the device scratch

// ---- the drivers' whole recipe at --scalingFactor != 1 on the device (reference UnMicst1-5.py:807-821,845-854):
// raw planes -> im2double -> resize to (int(H*sf), int(W*sf)) -> [rescale_intensity((min, max) -> (0, 0.983))] -> inference
// -> np.uint8(255 * pm) -> resize back to (H, W) -> np.uint8(255 * .).  One resize = skimage.transform.resize's defaults
// (umx_kernels.hip).  Synchronous; the planes are small next to the tile work, so nothing is pipelined here.
// ctx only receives the error text (NULL from the test entries); *filtered: the plane the zoom read (src, tmpA or tmpB)
static int resize_plane(umx_ctx* ctx, hipStream_t stream, const double* src, int H, int W, int h, int w, double* tmpA, double* tmpB,
                        double* wdev, unsigned long long* mm64, double* dst, unsigned char* dst_u8, const double** filtered = nullptr) {
    const double* cur = src;
    const double fy = (double)H / h, fx = (double)W / w;
    const double sig[2] = {std::max(0.0, (fy - 1.0) / 2.0), std::max(0.0, (fx - 1.0) / 2.0)};
    if (h < H || w < W) {   // anti-aliasing Gaussian, axis by axis (scipy.ndimage.gaussian_filter: axis 0 first)
        double* bufs[2] = {tmpA, tmpB};
        int which = 0;
        for (int axis = 0; axis < 2; ++axis) {
            if (!(sig[axis] > 1e-15)) continue;   // scipy skips axes with sigma <= 1e-15
            if (4.0 * sig[axis] + 0.5 >= (double)kMaxGaussTaps) return fail(ctx, UMX_ERR_INVALID, "scaling factor too small for the resize kernel");
            std::vector<double> wts;
            const int radius = gauss_weights(sig[axis], &wts);
            HIP_TRY(ctx, hipMemcpyAsync(wdev + axis * kMaxGaussTaps, wts.data(), wts.size() * sizeof(double), hipMemcpyHostToDevice, stream));
            HIP_TRY(ctx, hipStreamSynchronize(stream));   // (wts is a stack-lifetime host buffer)
            HIP_TRY(ctx, launch_gauss1d(cur, bufs[which], H, W, axis, radius, wdev + axis * kMaxGaussTaps, stream));
            cur = bufs[which];
            which ^= 1;
        }
    }
    if (filtered) *filtered = cur;
    HIP_TRY(ctx, launch_minmax_f64(cur, (size_t)H * W, mm64, stream));   // resize clips to the (filtered) input's range
    HIP_TRY(ctx, launch_zoom1(cur, H, W, h, w, mm64, dst, dst_u8, stream));
    return UMX_OK;
}

// outlier < 0: rescale (if set) to the plane's (min, max); outlier in [0, 100]: to (min, np.percentile(plane, outlier))
static int infer_raw_scaled_impl(umx_ctx* ctx, const void* raw_host, int bits, int C_img, int H, int W, double scaling, int rescale,
                                 double outlier, double mean, double stdv, int mode, uint8_t* out_host) {
    if (const int rc = check_image(ctx, raw_host && out_host, C_img, H, W, true, bits, stdv, mode, UMX_STITCH_FP16_COMPAT, nullptr))
        return rc;
    if (!(scaling > 0.0)) return fail(ctx, UMX_ERR_INVALID, "scaling factor must be positive");
    const int h = (int)((double)H * scaling), w = (int)((double)W * scaling);   // int(float(I.shape[0]) * float(sf))
    if (h < 1 || w < 1) return fail(ctx, UMX_ERR_INVALID, "scaled image is empty");
    const bool same = h == H && w == W;   // resize(I, I.shape) leaves im2double(I): the pipelined path does all but the percentile
    if (same && outlier < 0) return umx_infer_image_raw(ctx, raw_host, bits, C_img, H, W, rescale, mean, stdv, mode, out_host);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t big = (size_t)std::max(H, h) * std::max(W, w), plane = (size_t)H * W, sp = (size_t)h * w, K = ctx->hp.nClasses;
    const size_t in_b = bits / 8;
    // scratch: [raw upload | 3 float64 work planes of the larger size | scaled input planes | fp16 result | u8 out | weights | mm]
    size_t off = 0;
    auto take = [&](size_t bytes) { const size_t o = off; off = (off + bytes + 255) & ~(size_t)255; return o; };
    const size_t o_raw = take(plane * C_img * in_b), o_a = take(big * 8), o_b = take(big * 8), o_c = take(big * 8);
    const size_t o_in = take(sp * C_img * 8), o_pm = take(K * sp * 2), o_u8 = take(K * plane), o_w = take(2 * kMaxGaussTaps * 8), o_mm = take(256);
    const size_t o_sel = take(64 + 512 * 4);   // radix-selection state + histograms of the percentile
    int rc;
    umx_ctx::HostSlot& hs = ctx->hs[0];
    if (hs.busy) return fail(ctx, UMX_ERR_INVALID, "slot 0 still holds a submitted call: wait for it first");
    if ((rc = grow(ctx, &hs.d_out, &hs.out_cap, off, "slot 0 d_out"))) return rc;
    unsigned char* const base = (unsigned char*)hs.d_out;
    double *A = (double*)(base + o_a), *B = (double*)(base + o_b), *Cw = (double*)(base + o_c), *din = (double*)(base + o_in);
    double* const wdev = (double*)(base + o_w);
    unsigned long long* const mm64 = (unsigned long long*)(base + o_mm);
    unsigned* const mm32 = (unsigned*)(base + o_mm + 64);
    HIP_TRY(ctx, hipMemcpyAsync(base + o_raw, raw_host, plane * C_img * in_b, hipMemcpyHostToDevice, ctx->stream));
    for (int c = 0; c < C_img; ++c) {
        HIP_TRY(ctx, launch_minmax_init(mm32, ctx->stream));
        HIP_TRY(ctx, launch_raw_convert(base + o_raw + (size_t)c * plane * in_b, bits, plane, 0, mm32, A, ctx->stream));   // im2double
        if (same) HIP_TRY(ctx, hipMemcpyAsync(din + (size_t)c * sp, A, sp * 8, hipMemcpyDeviceToDevice, ctx->stream));
        else if ((rc = resize_plane(ctx, ctx->stream, A, H, W, h, w, B, Cw, wdev, mm64, din + (size_t)c * sp, nullptr))) return rc;
        if (rescale) {   // rescale_intensity(I, (min, max | percentile), (0, 0.983)) of the RESIZED plane (UnMicst1-5.py:817-821)
            HIP_TRY(ctx, launch_minmax_f64(din + (size_t)c * sp, sp, mm64, ctx->stream));
            if (outlier >= 0)
                HIP_TRY(ctx, launch_percentile_f64(din + (size_t)c * sp, sp, outlier, (unsigned long long*)(base + o_sel),
                                                   (unsigned*)(base + o_sel + 64), mm64, ctx->stream));
            HIP_TRY(ctx, launch_rescale_f64(din + (size_t)c * sp, sp, mm64, ctx->stream));
        }
    }
    if ((rc = umx_infer_image_dev(ctx, din, C_img, h, w, mean, stdv, mode, UMX_STITCH_FP16_COMPAT, base + o_pm))) return rc;
    for (size_t k = 0; k < K; ++k) {
        if (same) {   // resize of a uint8 plane to its own shape and back through np.uint8(255 * .): the plane itself
            HIP_TRY(ctx, launch_half_to_u8(base + o_pm + k * sp * 2, sp, base + o_u8 + k * plane, ctx->stream));
            continue;
        }
        HIP_TRY(ctx, launch_half_to_u8_f64(base + o_pm + k * sp * 2, sp, A, ctx->stream));   // np.uint8(255 * pm) as float u8/255
        if ((rc = resize_plane(ctx, ctx->stream, A, h, w, H, W, B, Cw, wdev, mm64, nullptr, base + o_u8 + k * plane))) return rc;
    }
    HIP_TRY(ctx, hipMemcpyAsync(out_host, base + o_u8, K * plane, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return check_range_flag(ctx);
}

int umx_infer_image_raw_scaled(umx_ctx* ctx, const void* raw_host, int bits, int C_img, int H, int W, double scaling, int rescale,
                               double mean, double stdv, int mode, uint8_t* out_host) {
    return guarded(ctx, true, true, [&]() -> int {
        return infer_raw_scaled_impl(ctx, raw_host, bits, C_img, H, W, scaling, rescale, -1.0, mean, stdv, mode, out_host);
    });
}

int umx_infer_image_raw_outlier(umx_ctx* ctx, const void* raw_host, int bits, int C_img, int H, int W, double scaling, double outlier,
                                double mean, double stdv, int mode, uint8_t* out_host) {
    if (!(outlier >= 0.0 && outlier <= 100.0)) return fail(ctx, UMX_ERR_INVALID, "outlier percentile must be in [0, 100]");
    return guarded(ctx, true, true, [&]() -> int {
        return infer_raw_scaled_impl(ctx, raw_host, bits, C_img, H, W, scaling, 1, outlier, mean, stdv, mode, out_host);
    });
}

int umx_infer_image_raw_submit(umx_ctx* ctx, int slot, const void* raw_host, int bits, int C_img, int H, int W, int rescale,
                               double mean, double stdv, int mode, uint8_t* out_host) {
    if (const int rc = check_image(ctx, raw_host && out_host, C_img, H, W, true, bits, stdv, mode, UMX_STITCH_FP16_COMPAT, nullptr))
        return rc;
    return host_submit(ctx, slot, false, raw_host, bits, C_img, H, W, rescale, nullptr, mean, stdv, mode, UMX_STITCH_FP16_COMPAT, 1, out_host);
}

int umx_infer_image_wait(umx_ctx* ctx, int slot) {
    if (!ctx) return fail(nullptr, UMX_ERR_INVALID, "ctx is NULL");
    return guarded(ctx, false, true, [&]() -> int { return host_wait(ctx, slot); });
}

// The schedule of a whole-slide call on the host alone (no device): slide_describe of the plan host_enqueue would execute for this
// model, slide and call -- stitch: UMX_STITCH_*; tile_flops <= 0: the graph is built from the hyper-parameters for the figure.
// *needed: bytes of the text with its terminator; UMX_ERR_INVALID where cap is smaller.
int umx_test_slide_plan(const umx_hparams* hp, int H, int W, int max_batch, int C_img, int src_bits, int rescale, int has_range, int sync_call,
                        int host_range_ok, int raw_gather, int stitch, int out_u8, double tile_flops, char* text, size_t cap, size_t* needed) {
    if (!hp || !needed || (!text && cap)) return fail(nullptr, UMX_ERR_INVALID, "umx_test_slide_plan: null argument");
    *needed = 0;
    std::string why;
    if (const int rc = check_hp(hp, &why)) return fail(nullptr, rc, "%s", why.c_str());
    if (H < 1 || W < 1 || max_batch < 1 || C_img < 1 || (src_bits != 0 && src_bits != 8 && src_bits != 16))
        return fail(nullptr, UMX_ERR_INVALID, "umx_test_slide_plan: bad H / W / max_batch / C_img / src_bits");
    SlideSpec sp;
    sp.max_batch = max_batch;
    sp.K = hp->nClasses;
    sp.C_img = C_img;
    sp.src_bits = src_bits;
    sp.rescale = rescale;
    sp.has_range = has_range != 0;
    sp.sync_call = sync_call != 0;
    sp.host_range_ok = host_range_ok != 0;
    sp.stitch_el = stitch == UMX_STITCH_FP32 ? 4 : 2;
    sp.out_u8 = out_u8;
    sp.raw_gather = src_bits != 0 && raw_gather != 0;
    sp.tile_flops = tile_flops;
    if (!(tile_flops > 0.0)) {
        std::vector<Launch> plan;
        build_graph(*hp, nullptr, &plan, nullptr, nullptr, nullptr);
        sp.tile_flops = 0.0;
        for (const Launch& L : plan) sp.tile_flops += L.flops;
    }
    const std::string out = slide_describe(slide_plan(geom_of(*hp, H, W), sp));
    *needed = out.size() + 1;
    if (cap < *needed) return fail(nullptr, UMX_ERR_INVALID, "umx_test_slide_plan: the text takes %zu bytes", *needed);
    memcpy(text, out.c_str(), *needed);
    return UMX_OK;
}

// ---- test entries of the driver-side image kernels (tests/test_gpu_imagekernels.py, tests/test_imagekernels_cpu.py): thin wrappers
// around the production functions above on caller-given planes, on the default stream, with scratch of their own

namespace {
struct DevScratch {   // one allocation cut into 256-byte-aligned pieces, as infer_raw_scaled_impl cuts the slot's buffer
    unsigned char* base = nullptr;
    size_t off = 0;
    DevArena mem;         // call-local (UMX_DEBUG_GUARD: red zones round the allocation, its content poisoned)
    size_t take(size_t bytes) { const size_t o = off; off = (off + bytes + 255) & ~(size_t)255; return o; }
    int alloc(const char* who) {   // the `off` bytes taken so far
        std::string why;
        if (arena_init(&mem, &why) != UMX_OK) return fail(nullptr, UMX_ERR_INVALID, "%s", why.c_str());
        HIP_TRY(nullptr, arena_alloc(&mem, (void**)&base, off, false, who, true));
        return UMX_OK;
    }
    int check() {                  // at the end of the entry, before the destructor frees the allocation
        if (mem.fill < 0) return UMX_OK;
        HIP_TRY(nullptr, hipDeviceSynchronize());
        std::string msg;
        const int rc = arena_check(mem, &msg);
        return rc == UMX_OK ? UMX_OK : fail(nullptr, rc, "%s", msg.c_str());
    }
    ~DevScratch() { arena_free(&mem); }
};
int test_device(const char* who) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) return fail(nullptr, UMX_ERR_NO_DEVICE, "%s: no HIP device available", who);
    return UMX_OK;
}
}  // namespace

int umx_test_gauss_weights(double sigma, double* out, int cap) {
    if (!out || !(sigma > 1e-15) || !(4.0 * sigma + 0.5 < (double)kMaxGaussTaps)) return -1;
    std::vector<double> wts;
    const int radius = gauss_weights(sigma, &wts);
    if (radius + 1 > cap) return -1;
    memcpy(out, wts.data(), wts.size() * sizeof(double));
    return radius;
}

int umx_test_resize_dev(const double* src, int H, int W, int h, int w, double* out_f64, uint8_t* out_u8, double* out_filtered) {
    if (!src || (!out_f64 && !out_u8) || H < 1 || W < 1 || h < 1 || w < 1) return fail(nullptr, UMX_ERR_INVALID, "umx_test_resize_dev: bad arguments");
    if (const int rc = test_device("umx_test_resize_dev")) return rc;
    const size_t big = (size_t)std::max(H, h) * std::max(W, w), plane = (size_t)H * W, sp = (size_t)h * w;
    DevScratch d;
    const size_t o_a = d.take(big * 8), o_b = d.take(big * 8), o_c = d.take(big * 8), o_dst = d.take(sp * 8), o_u8 = d.take(sp);
    const size_t o_w = d.take(2 * kMaxGaussTaps * 8), o_mm = d.take(256);
    if (const int rc = d.alloc("umx_test_resize_dev scratch")) return rc;
    double *A = (double*)(d.base + o_a), *B = (double*)(d.base + o_b), *Cw = (double*)(d.base + o_c);
    HIP_TRY(nullptr, hipMemcpy(A, src, plane * 8, hipMemcpyHostToDevice));
    int rc;
    const double* filt = nullptr;
    if (out_f64) {
        if ((rc = resize_plane(nullptr, nullptr, A, H, W, h, w, B, Cw, (double*)(d.base + o_w), (unsigned long long*)(d.base + o_mm),
                               (double*)(d.base + o_dst), nullptr, &filt)))
            return rc;
        HIP_TRY(nullptr, hipMemcpy(out_f64, d.base + o_dst, sp * 8, hipMemcpyDeviceToHost));
    }
    if (out_u8) {
        if ((rc = resize_plane(nullptr, nullptr, A, H, W, h, w, B, Cw, (double*)(d.base + o_w), (unsigned long long*)(d.base + o_mm),
                               nullptr, d.base + o_u8, &filt)))
            return rc;
        HIP_TRY(nullptr, hipMemcpy(out_u8, d.base + o_u8, sp, hipMemcpyDeviceToHost));
    }
    if (out_filtered) HIP_TRY(nullptr, hipMemcpy(out_filtered, filt, plane * 8, hipMemcpyDeviceToHost));
    return d.check();
}

int umx_test_rescale_dev(const double* plane, size_t n, double outlier, double* out_plane, double* range2) {
    if (!plane || !out_plane || !range2 || n == 0 || !(outlier <= 100.0)) return fail(nullptr, UMX_ERR_INVALID, "umx_test_rescale_dev: bad arguments");
    if (const int rc = test_device("umx_test_rescale_dev")) return rc;
    DevScratch d;
    const size_t o_x = d.take(n * 8), o_mm = d.take(256), o_sel = d.take(64 + 512 * 4);
    if (const int rc = d.alloc("umx_test_rescale_dev scratch")) return rc;
    double* const x = (double*)(d.base + o_x);
    unsigned long long* const mm64 = (unsigned long long*)(d.base + o_mm);
    HIP_TRY(nullptr, hipMemcpy(x, plane, n * 8, hipMemcpyHostToDevice));
    HIP_TRY(nullptr, launch_minmax_f64(x, n, mm64, nullptr));
    if (outlier >= 0)
        HIP_TRY(nullptr, launch_percentile_f64(x, n, outlier, (unsigned long long*)(d.base + o_sel), (unsigned*)(d.base + o_sel + 64), mm64, nullptr));
    HIP_TRY(nullptr, launch_rescale_f64(x, n, mm64, nullptr));
    HIP_TRY(nullptr, hipMemcpy(range2, mm64, 16, hipMemcpyDeviceToHost));   // the (min, limit) doubles the rescale read
    HIP_TRY(nullptr, hipMemcpy(out_plane, x, n * 8, hipMemcpyDeviceToHost));
    return d.check();
}

int umx_test_plane_range_dev(const void* raw, int bits, const size_t* n, const size_t* offset_elems, const int* nslabs, int njobs,
                             uint32_t* range2) {
    if (!raw || !n || !offset_elems || !nslabs || !range2 || njobs < 1 || (bits != 8 && bits != 16))
        return fail(nullptr, UMX_ERR_INVALID, "umx_test_plane_range_dev: bad arguments");
    if (const int rc = test_device("umx_test_plane_range_dev")) return rc;
    const size_t el = bits / 8;
    size_t most = 0;
    for (int j = 0; j < njobs; ++j) {
        if (n[j] == 0 || nslabs[j] < 1) return fail(nullptr, UMX_ERR_INVALID, "umx_test_plane_range_dev: empty job %d", j);
        most = std::max(most, (n[j] + offset_elems[j]) * el);
    }
    DevScratch d;
    const size_t o_raw = d.take(most), o_mm = d.take((size_t)njobs * 8);
    if (const int rc = d.alloc("umx_test_plane_range_dev scratch")) return rc;   // (hipMalloc's addresses are 256-byte aligned, and so is every piece)
    unsigned* const mm = (unsigned*)(d.base + o_mm);
    const unsigned char* src = (const unsigned char*)raw;
    for (int j = 0; j < njobs; ++j) {   // the jobs share the plane buffer: the default stream orders copy j + 1 behind reduction j
        unsigned char* const plane = d.base + o_raw + offset_elems[j] * el;
        HIP_TRY(nullptr, hipMemcpyAsync(plane, src, n[j] * el, hipMemcpyHostToDevice, nullptr));
        HIP_TRY(nullptr, launch_minmax_init(mm + 2 * j, nullptr));
        // consecutive slabs as host_enqueue reduces the rows it uploads; with more than one slab their length is odd, so that
        // the second slab of a 16-bit plane starts at an odd element
        size_t len = (n[j] + nslabs[j] - 1) / nslabs[j];
        if (nslabs[j] > 1) len |= 1;
        for (size_t e0 = 0; e0 < n[j]; e0 += len)
            HIP_TRY(nullptr, launch_minmax(plane + e0 * el, bits, std::min(len, n[j] - e0), mm + 2 * j, nullptr));
        src += n[j] * el;
    }
    HIP_TRY(nullptr, hipMemcpy(range2, mm, (size_t)njobs * 8, hipMemcpyDeviceToHost));
    return d.check();
}

int umx_test_half_to_u8_dev(const uint16_t* half_bits, size_t n, uint8_t* out_u8, double* out_f64) {
    if (!half_bits || !out_u8 || !out_f64 || n == 0) return fail(nullptr, UMX_ERR_INVALID, "umx_test_half_to_u8_dev: bad arguments");
    if (const int rc = test_device("umx_test_half_to_u8_dev")) return rc;
    DevScratch d;
    const size_t o_pm = d.take(n * 2), o_u8 = d.take(n), o_f = d.take(n * 8);
    if (const int rc = d.alloc("umx_test_half_to_u8_dev scratch")) return rc;
    HIP_TRY(nullptr, hipMemcpy(d.base + o_pm, half_bits, n * 2, hipMemcpyHostToDevice));
    HIP_TRY(nullptr, launch_half_to_u8(d.base + o_pm, n, d.base + o_u8, nullptr));
    HIP_TRY(nullptr, launch_half_to_u8_f64(d.base + o_pm, n, (double*)(d.base + o_f), nullptr));
    HIP_TRY(nullptr, hipMemcpy(out_u8, d.base + o_u8, n, hipMemcpyDeviceToHost));
    HIP_TRY(nullptr, hipMemcpy(out_f64, d.base + o_f, n * 8, hipMemcpyDeviceToHost));
    return d.check();
}

}  // extern "C"
