// libumx device-resident training set: storage, the host checks, the chunking of a batch into launches, the validation counts and the
// C ABI of the umx_trainset_* / umx_train_step_sampled / _augmented / _warped / _elastic / umx_trainer_assemble / _augmented / _warped /
// _elastic / umx_trainer_evaluate / _evaluate_objects / umx_trainer_object_counts / umx_trainset_border_weights / _border_planes entries
// of include/umx_train.h (the assembly kernels and their launchers: umx_trainset_assemble.hip; the kernels of the border maps:
// umx_trainset_border.hip; of the object score: umx_trainset_objects.hip).
//
// The set is the reference's annotated layout (I%05d_Img.tif pages, _Ant.tif class codes, _wt.tif contour-intersection map;
// UnMicst1-5.py:295-312, UnMicst2.py:293-309, UnMicst.py:236-243) uploaded once, already normalised.  A step then costs 32 bytes
// of descriptors per image (passed as kernel arguments) and one small kernel that writes the step's own data / labels / weights
// buffers; the validation pass reduces the eval-mode softmax to exact per-class counts on the device.  DESIGN.md section 9.2.
//
//   class_counts_kernel    per block: correct / labelled per class (int64) and sum of -log p[label] (float64), fixed order;
//   class_counts_final     one block sums the block partials in a fixed order
#include "../../include/umx_train.h"
#include "umx_internal.h"
#include "umx_kernels.h"

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <vector>

using namespace umx;

static_assert(sizeof(umx_sample_desc) == 32, "umx_sample_desc is 32 bytes");
static_assert(sizeof(umx_label_weights) == 4 + 8 * 4 + 8 * 4 + 7 * 4, "umx_label_weights layout");
static_assert(sizeof(umx_augment_desc) == 8, "umx_augment_desc is 8 bytes");
static_assert(sizeof(umx_augment_table) == 12 + 16 * 4 + 16 * 13 * 4 + 5 * 4, "umx_augment_table layout");
static_assert(sizeof(umx_warp_desc) == 16, "umx_warp_desc is 16 bytes");
static_assert(sizeof(umx_elastic_desc) == 304, "umx_elastic_desc is 304 bytes");
static_assert(sizeof(umx_object_options) == 32, "umx_object_options is 32 bytes");

struct umx_trainset {
    umx_trainer* tr = nullptr;
    int N = 0, pages = 0, S = 0, C = 0, K = 0, row_f = 0, row_a = 0;
    bool weighted = false;
    umx_label_weights lw;
    bool has_aug = false;               // umx_trainset_set_augment was called
    umx_augment_table aug;              // (host copy: levels travel to the kernel as arguments)
    float* planes = nullptr;
    uint8_t* ann = nullptr;
    float* wmap = nullptr;
    double* part = nullptr;             // class_counts workspace (B P^2 pixels at most)
    long long* counts = nullptr;        // [2K]
    double* loss = nullptr;             // [1]
    int* border_ws = nullptr;           // [N][S][S] labelling workspace, allocated by the first umx_trainset_border_* call
    int* border_diag = nullptr;         // [4][S][S] labels | d1sq | d2sq | map of umx_trainset_border_planes, allocated by its first call
    ObjectWorkspace obj;                // the object score's planes, words and pair tables, allocated by the first call of an object entry
    DevArena mem;                       // every device buffer above (UMX_DEBUG_GUARD: with red zones)
};

namespace umx {

namespace {

constexpr int kCountThreads = 256;
constexpr int kMaxClasses = 8;       // umx_trainer_create: nClasses 2..8
constexpr int kMaxCountBlocks = 1024;

int count_blocks(size_t npix) {
    const size_t per = (size_t)kCountThreads * 8;
    return (int)std::min<size_t>(kMaxCountBlocks, std::max<size_t>(1, (npix + per - 1) / per));
}

// the block's values of 2K + 1 quantities summed over its threads by a tree in LDS (fixed order), thread 0 writes them
template <typename T>
__device__ T block_sum(T v, T* sm) {
    const int t = threadIdx.x;
    __syncthreads();
    sm[t] = v;
    __syncthreads();
    for (int s = kCountThreads / 2; s > 0; s >>= 1) {
        if (t < s) sm[t] += sm[t + s];
        __syncthreads();
    }
    return sm[0];
}

// part: [gridDim.x][2K + 1] doubles -- the int64 counts stored as their bit patterns, then the loss
__global__ void __launch_bounds__(kCountThreads) class_counts_kernel(const float* __restrict__ probs, const float* __restrict__ labels,
                                                                     size_t npix, int K, double* __restrict__ part) {
    __shared__ long long smi[kCountThreads];
    __shared__ double smd[kCountThreads];
    const size_t rpb = (npix + gridDim.x - 1) / gridDim.x;
    const size_t r0 = (size_t)blockIdx.x * rpb, r1 = std::min(npix, r0 + rpb);
    int correct[kMaxClasses], labelled[kMaxClasses];
#pragma unroll
    for (int k = 0; k < kMaxClasses; ++k) correct[k] = labelled[k] = 0;
    double loss = 0.0;
    for (size_t r = r0 + threadIdx.x; r < r1; r += kCountThreads) {
        const float* p = probs + r * K;
        const float* l = labels + r * K;
        int lab = -1, arg = 0;
        float best = p[0];
        for (int k = 0; k < K; ++k) {
            if (lab < 0 && l[k] != 0.f) lab = k;
            if (k > 0 && p[k] > best) { best = p[k]; arg = k; }   // first maximum (tf.argmax)
        }
        if (lab < 0) continue;   // code 0 / above K: an all-zero label row is no pixel of any class
#pragma unroll
        for (int k = 0; k < kMaxClasses; ++k)
            if (k == lab) { labelled[k] += 1; correct[k] += arg == k; }
        loss += -log((double)p[lab]);
    }
    double* out = part + (size_t)blockIdx.x * (2 * K + 1);
#pragma unroll
    for (int k = 0; k < kMaxClasses; ++k)
        if (k < K) {
            const long long c = block_sum<long long>(correct[k], smi);
            const long long n = block_sum<long long>(labelled[k], smi);
            if (threadIdx.x == 0) { out[k] = __longlong_as_double(c); out[K + k] = __longlong_as_double(n); }
        }
    const double ls = block_sum<double>(loss, smd);
    if (threadIdx.x == 0) out[2 * K] = ls;
}

__global__ void __launch_bounds__(kCountThreads) class_counts_final(const double* __restrict__ part, int nblk, int K,
                                                                    long long* __restrict__ counts, double* __restrict__ loss) {
    __shared__ long long smi[kCountThreads];
    __shared__ double smd[kCountThreads];
    for (int q = 0; q < 2 * K; ++q) {
        long long s = 0;
        for (int g = threadIdx.x; g < nblk; g += kCountThreads) s += __double_as_longlong(part[(size_t)g * (2 * K + 1) + q]);
        s = block_sum<long long>(s, smi);
        if (threadIdx.x == 0) counts[q] = s;
    }
    double s = 0.0;
    for (int g = threadIdx.x; g < nblk; g += kCountThreads) s += part[(size_t)g * (2 * K + 1) + 2 * K];
    s = block_sum<double>(s, smd);
    if (threadIdx.x == 0) *loss = s;
}

}  // namespace

size_t class_counts_parts(size_t npix, int K) { return (size_t)count_blocks(npix) * (2 * K + 1); }

hipError_t launch_class_counts(const float* probs, const float* labels, size_t npix, int K, double* part, long long* counts,
                               double* loss, hipStream_t stream) {
    if (K < 1 || K > kMaxClasses || npix == 0) return hipErrorInvalidValue;
    const int nblk = count_blocks(npix);
    hipLaunchKernelGGL(class_counts_kernel, dim3((unsigned)nblk), dim3(kCountThreads), 0, stream, probs, labels, npix, K, part);
    hipLaunchKernelGGL(class_counts_final, dim3(1), dim3(kCountThreads), 0, stream, part, nblk, K, counts, loss);
    return hipGetLastError();
}

}  // namespace umx

namespace {

int tsfail(umx_trainer* tr, int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    return trainer_fail(tr, code, buf);
}

#define TS_HIP(tr, call)                                                                                   \
    do {                                                                                                   \
        hipError_t e_ = (call);                                                                            \
        if (e_ != hipSuccess)                                                                              \
            return tsfail(tr, e_ == hipErrorOutOfMemory ? UMX_ERR_OOM : UMX_ERR_HIP, "%s failed: %s", #call, \
                          hipGetErrorString(e_));                                                          \
    } while (0)
#define TS_TRY(call)                   \
    do {                               \
        int rc_ = (call);              \
        if (rc_ != UMX_OK) return rc_; \
    } while (0)

template <typename T>
int ts_alloc_(umx_trainset* ts, T** out, size_t count, const char* label) {
    void* d = nullptr;
    TS_HIP(ts->tr, arena_alloc(&ts->mem, &d, count * sizeof(T), false, label));
    *out = reinterpret_cast<T*>(d);
    return UMX_OK;
}
#define ts_alloc(ts, out, count) ts_alloc_(ts, out, count, #out)

// guard mode: the trainer's zones (its streams idle afterwards), then the set's own
int guard_check(umx_trainer* tr, const umx_trainset* ts) {
    TS_TRY(trainer_guard_check(tr));
    std::string msg;
    const int rc = arena_check(ts->mem, &msg);
    return rc == UMX_OK ? UMX_OK : tsfail(tr, rc, "%s", msg.c_str());
}

TrainSetView view_of(const umx_trainset* ts) {
    TrainSetView v;
    v.planes = ts->planes; v.ann = ts->ann; v.wmap = ts->wmap;
    v.S = ts->S; v.pages = ts->pages; v.C = ts->C; v.row_f = ts->row_f; v.row_a = ts->row_a;
    for (int k = 0; k < 8; ++k) { v.cw[k] = ts->lw.class_weight[k]; v.iw[k] = ts->lw.intersect_weight[k]; }
    return v;
}

// every descriptor checked on the host before anything is enqueued (the kernel trusts them: its reads stay inside the sample)
int check_descs(umx_trainer* tr, const umx_trainset* ts, const umx_sample_desc* desc, int n, int n_max, const char* what) {
    if (!tr || !ts || !desc) return tsfail(tr, UMX_ERR_INVALID, "null argument");
    if (ts->tr != tr) return tsfail(tr, UMX_ERR_INVALID, "%s: the training set belongs to another trainer", what);
    const TrainerIO io = trainer_io(tr);
    if (n < 1 || n > n_max) return tsfail(tr, UMX_ERR_INVALID, "%s: %d descriptors, the batch holds 1..%d", what, n, n_max);
    for (int i = 0; i < n; ++i) {
        const umx_sample_desc& d = desc[i];
        const char* why = nullptr;
        if (d.index < 0 || d.index >= ts->N) why = "sample index out of range";
        else if (d.page < 0 || d.page >= ts->pages) why = "page out of range";
        else if (d.y0 < 0 || d.x0 < 0 || d.y0 > ts->S - io.P || d.x0 > ts->S - io.P) why = "crop outside the sample";
        else if (d.transform < 0 || d.transform > 7) why = "transform outside 0..7";
        else if (!std::isfinite(d.brightness) || !std::isfinite(d.contrast)) why = "brightness / contrast not finite";
        else if (d.reserved != 0) why = "reserved field not zero";
        if (why)
            return tsfail(tr, UMX_ERR_INVALID, "%s: descriptor %d (index %d, page %d, crop %d,%d, transform %d): %s", what, i, d.index, d.page,
                          d.y0, d.x0, d.transform, why);
    }
    return UMX_OK;
}

// rows 0..n-1 from desc, rows n..B-1 zero; weights written only when `weights`
int enqueue_assemble(umx_trainer* tr, const umx_trainset* ts, const umx_sample_desc* desc, int n, bool weights) {
    const TrainerIO io = trainer_io(tr);
    const TrainSetView v = view_of(ts);
    for (int b0 = 0; b0 < io.B; b0 += kDescChunk) {
        const int m = std::min(kDescChunk, io.B - b0);
        DescChunk dc;
        memset(&dc, 0, sizeof dc);
        for (int j = 0; j < m; ++j) {
            if (b0 + j < n) dc.d[j] = desc[b0 + j];
            else dc.d[j].index = -1;
        }
        TS_HIP(tr, launch_assemble_batch(v, dc, m, b0, io.P, io.K, io.data, io.labels, weights ? io.weights : nullptr, io.stream));
    }
    return UMX_OK;
}

// the parallel array of umx_augment_desc, checked like the descriptors: before anything is enqueued
int check_augs(umx_trainer* tr, const umx_trainset* ts, const umx_augment_desc* aug, int n, const char* what) {
    if (!aug) return tsfail(tr, UMX_ERR_INVALID, "null argument");
    if (!ts->has_aug) return tsfail(tr, UMX_ERR_INVALID, "%s: the training set has no augmentation table (umx_trainset_set_augment)", what);
    for (int i = 0; i < n; ++i) {
        const char* why = nullptr;
        if (aug[i].blur_level < 0 || aug[i].blur_level >= ts->aug.n_levels) why = "blur level outside the table";
        else if (!std::isfinite(aug[i].gain) || aug[i].gain < 1.f) why = "gain not finite or below 1";
        if (why)
            return tsfail(tr, UMX_ERR_INVALID, "%s: augmentation %d (blur level %d of %d, gain %g): %s", what, i, aug[i].blur_level,
                          ts->aug.n_levels, (double)aug[i].gain, why);
    }
    return UMX_OK;
}

bool warp_is_identity(const umx_warp_desc& w) { return w.m[0] == 1.f && w.m[1] == 0.f && w.m[2] == 0.f && w.m[3] == 1.f; }

// the parallel array of umx_warp_desc, likewise
int check_warps(umx_trainer* tr, const umx_trainset* ts, const umx_warp_desc* warp, int n, const char* what) {
    if (!warp) return tsfail(tr, UMX_ERR_INVALID, "null argument");
    if (ts->S < 2) return tsfail(tr, UMX_ERR_INVALID, "%s: a sample of one pixel cannot be warped", what);
    char why[160];
    if (umx_warp_desc_check(warp, n, why, sizeof why) != UMX_OK) return tsfail(tr, UMX_ERR_INVALID, "%s: %s", what, why);
    return UMX_OK;
}

// the parallel array of umx_elastic_desc, likewise
int check_elastics(umx_trainer* tr, const umx_trainset* ts, const umx_elastic_desc* elastic, int n, const char* what) {
    if (!elastic) return tsfail(tr, UMX_ERR_INVALID, "null argument");
    if (ts->S < 2) return tsfail(tr, UMX_ERR_INVALID, "%s: a sample of one pixel cannot be deformed", what);
    char why[160];
    if (umx_elastic_desc_check(elastic, n, why, sizeof why) != UMX_OK) return tsfail(tr, UMX_ERR_INVALID, "%s: %s", what, why);
    return UMX_OK;
}

// the parallel arrays an entry cannot do without: the one it is named for.  An array in front of that one may be null (aug: no blur,
// gain 1; warp: the identity), and an entry passes null for the arrays behind it.
enum : unsigned { kNeedsAug = 1, kNeedsWarp = 2, kNeedsElastic = 4 };

// the checks of an entry, in the order descriptors, augmentations, warps, lattices; nothing is enqueued before all of them pass
int check_batch(umx_trainer* tr, const umx_trainset* ts, const umx_sample_desc* desc, const umx_augment_desc* aug, const umx_warp_desc* warp,
                const umx_elastic_desc* elastic, unsigned needs, int n, int n_max, const char* what) {
    TS_TRY(check_descs(tr, ts, desc, n, n_max, what));
    if (aug || (needs & kNeedsAug)) TS_TRY(check_augs(tr, ts, aug, n, what));
    if (warp || (needs & kNeedsWarp)) TS_TRY(check_warps(tr, ts, warp, n, what));
    if (elastic || (needs & kNeedsElastic)) TS_TRY(check_elastics(tr, ts, elastic, n, what));
    return UMX_OK;
}

// launch(chunk, m) once the chunk's m images fill it, or at the batch's last image if it holds any; the chunk is empty afterwards
template <typename Chunk, typename Launch>
hipError_t flush_chunk(Chunk& ch, int& m, bool last, Launch launch) {
    if (m < (int)(sizeof ch.im / sizeof ch.im[0]) && !(m > 0 && last)) return hipSuccess;
    const hipError_t e = launch(ch, m);
    memset(&ch, 0, sizeof ch);
    m = 0;
    return e;
}

// enqueue_assemble for every image (labels, weights and the plain data: today's path), then, on the same stream, the images that ask
// for more written over it, 16 per launch: the data planes of those with a blur level or a gain (aug, may be null), and data, labels
// and weights of those with a warp other than the identity (warp, may be null).  An image with (level 0, gain 1, identity) is never
// touched again, and one with the identity never meets the warp code.  The images with a lattice (elastic, may be null; n != 0) go,
// 8 per launch, to the elastic instances instead -- with the identity matrix where they have no warp -- and the others never meet those.
int enqueue_batch(umx_trainer* tr, const umx_trainset* ts, const umx_sample_desc* desc, const umx_augment_desc* aug,
                  const umx_warp_desc* warp, const umx_elastic_desc* elastic, int n, bool weights) {
    TS_TRY(enqueue_assemble(tr, ts, desc, n, weights));
    if (!aug && !warp && !elastic) return UMX_OK;
    const TrainerIO io = trainer_io(tr);
    const TrainSetView v = view_of(ts);
    const float mean = ts->has_aug ? ts->aug.mean : 0.f, std = ts->has_aug ? ts->aug.std : 1.f;   // (read only when a gain != 1)
    float* const wts = weights ? io.weights : nullptr;
    const auto data_only = [&](const AugChunk& c, int m) { return launch_assemble_augmented(v, c, m, io.P, mean, std, io.data, io.stream); };
    const auto resampled = [&](const auto& c, int m) {
        return launch_assemble_resampled(v, c, m, io.P, io.K, mean, std, io.data, io.labels, wts, io.stream);
    };
    AugChunk chunk[2];   // [0] blur / gain only, [1] warped
    int m[2] = {0, 0};
    memset(chunk, 0, sizeof chunk);
    ElasticChunk ec;
    int me = 0;
    memset(&ec, 0, sizeof ec);
    for (int i = 0; i < n; ++i) {
        const bool deformed = elastic && elastic[i].n != 0;
        const bool warped = warp && !warp_is_identity(warp[i]);
        if (deformed || warped || (aug && (aug[i].blur_level != 0 || aug[i].gain != 1.f))) {
            if (deformed) {
                ec.im[me].n = elastic[i].n;
                memcpy(ec.im[me].d, elastic[i].d, sizeof ec.im[me].d);
            }
            AugImage& im = deformed ? ec.im[me++].a : chunk[warped].im[m[warped]++];
            im.d = desc[i];
            im.row = i;
            im.gain = aug ? aug[i].gain : 1.f;
            im.R = !aug || aug[i].blur_level == 0 ? -1 : ts->aug.radius[aug[i].blur_level];
            if (im.R >= 0) memcpy(im.taps, ts->aug.taps[aug[i].blur_level], sizeof im.taps);
            if (warped) memcpy(im.m, warp[i].m, sizeof im.m);
            else if (deformed) im.m[0] = im.m[3] = 1.f;
        }
        const bool last = i == n - 1;
        TS_HIP(tr, flush_chunk(ec, me, last, resampled));
        TS_HIP(tr, flush_chunk(chunk[0], m[0], last, data_only));
        TS_HIP(tr, flush_chunk(chunk[1], m[1], last, resampled));
    }
    return UMX_OK;
}

// umx_train_step_sampled / _augmented / _warped / _elastic
int step_from_set(umx_trainer* tr, const umx_trainset* ts, const umx_sample_desc* desc, const umx_augment_desc* aug,
                  const umx_warp_desc* warp, const umx_elastic_desc* elastic, unsigned needs, int apply_update, const char* what) {
    if (!tr) return tsfail(nullptr, UMX_ERR_INVALID, "null trainer");
    const TrainerIO io = trainer_io(tr);
    TS_TRY(check_batch(tr, ts, desc, aug, warp, elastic, needs, io.B, io.B, what));
    TS_HIP(tr, hipSetDevice(io.device));
    TS_TRY(enqueue_batch(tr, ts, desc, aug, warp, elastic, io.B, ts->weighted));
    TS_TRY(umx_train_step_dev(tr, io.data, io.labels, ts->weighted ? io.weights : nullptr, apply_update));   // (checks the trainer's zones)
    std::string msg;
    const int rc = arena_check(ts->mem, &msg);
    return rc == UMX_OK ? UMX_OK : tsfail(tr, rc, "%s", msg.c_str());
}

// umx_trainer_assemble / _augmented / _warped / _elastic
int assemble_to_host(umx_trainer* tr, const umx_trainset* ts, const umx_sample_desc* desc, const umx_augment_desc* aug,
                     const umx_warp_desc* warp, const umx_elastic_desc* elastic, unsigned needs, int n, float* data, float* labels,
                     float* weights, const char* what) {
    if (!tr) return tsfail(nullptr, UMX_ERR_INVALID, "null trainer");
    const TrainerIO io = trainer_io(tr);
    TS_TRY(check_batch(tr, ts, desc, aug, warp, elastic, needs, n, io.B, what));
    if (!data || !labels) return tsfail(tr, UMX_ERR_INVALID, "null argument");
    TS_HIP(tr, hipSetDevice(io.device));
    TS_TRY(enqueue_batch(tr, ts, desc, aug, warp, elastic, n, ts->weighted));
    const size_t npx = (size_t)n * io.P * io.P;
    TS_HIP(tr, hipMemcpyAsync(data, io.data, npx * io.C * sizeof(float), hipMemcpyDeviceToHost, io.stream));
    TS_HIP(tr, hipMemcpyAsync(labels, io.labels, npx * io.K * sizeof(float), hipMemcpyDeviceToHost, io.stream));
    if (weights && ts->weighted)
        TS_HIP(tr, hipMemcpyAsync(weights, io.weights, npx * io.K * sizeof(float), hipMemcpyDeviceToHost, io.stream));
    TS_HIP(tr, hipStreamSynchronize(io.stream));
    return guard_check(tr, ts);
}

// umx_trainset_border_weights / _border_planes: everything checked and the workspace there before anything is enqueued
int border_begin(umx_trainset* ts, int index, int index_min, const umx_border_options* o, bool diag, const char* what) {
    if (!ts) return tsfail(nullptr, UMX_ERR_INVALID, "null training set");
    umx_trainer* tr = ts->tr;
    if (!ts->weighted) return tsfail(tr, UMX_ERR_INVALID, "%s: an unweighted set has no weight map", what);
    if (index < index_min || index >= ts->N) return tsfail(tr, UMX_ERR_INVALID, "%s: sample %d of a set of %d", what, index, ts->N);
    char why[160];
    if (umx_border_options_check(o, ts->K, why, sizeof why) != UMX_OK) return tsfail(tr, UMX_ERR_INVALID, "%s: %s", what, why);
    if (ts->S > 46340) return tsfail(tr, UMX_ERR_INVALID, "%s: samples of %d pixels a side: a label (1 + y * size + x) is an int32", what, ts->S);
    const TrainerIO io = trainer_io(tr);
    TS_HIP(tr, hipSetDevice(io.device));
    const size_t plane = (size_t)ts->S * ts->S;
    const size_t need = (ts->border_ws ? 0 : plane * ts->N * sizeof(int)) + (diag && !ts->border_diag ? 4 * plane * sizeof(int) : 0);
    if (need) {
        size_t free_b = 0, total_b = 0;
        if (umx_device_mem_info(io.device, &free_b, &total_b) != UMX_OK) return tsfail(tr, UMX_ERR_HIP, "%s", umx_last_error(nullptr));
        if (need > free_b)
            return tsfail(tr, UMX_ERR_OOM, "%s: the labelling workspace of %d samples of %d x %d needs %.1f MB, %.1f MB are free", what,
                          ts->N, ts->S, ts->S, need / 1e6, free_b / 1e6);
        if (!ts->border_ws) TS_TRY(ts_alloc(ts, &ts->border_ws, plane * ts->N));
        if (diag && !ts->border_diag) TS_TRY(ts_alloc(ts, &ts->border_diag, 4 * plane));
    }
    return UMX_OK;
}

// umx_trainer_evaluate_objects / umx_trainer_object_counts: the options checked and the workspace there before anything is enqueued
int object_begin(umx_trainer* tr, umx_trainset* ts, const umx_object_options* o, const char* what) {
    char why[160];
    if (umx_object_options_check(o, ts->K, why, sizeof why) != UMX_OK) return tsfail(tr, UMX_ERR_INVALID, "%s: %s", what, why);
    const TrainerIO io = trainer_io(tr);
    if (io.P > kObjectMaxTile) return tsfail(tr, UMX_ERR_INVALID, "%s: a tile of %d pixels a side, the object pass takes up to %d", what, io.P, kObjectMaxTile);
    TS_HIP(tr, hipSetDevice(io.device));
    ObjectWorkspace& w = ts->obj;
    if (w.planes) return UMX_OK;
    const size_t part = (size_t)io.B * io.P * io.P, slots = object_table_slots(io.P);
    const size_t need = 2 * part + 6 * part * sizeof(int) + (size_t)io.B * slots * (sizeof(unsigned long long) + sizeof(int)) +
                        (size_t)io.B * UMX_OBJECT_COUNTS * sizeof(long long);
    size_t free_b = 0, total_b = 0;
    if (umx_device_mem_info(io.device, &free_b, &total_b) != UMX_OK) return tsfail(tr, UMX_ERR_HIP, "%s", umx_last_error(nullptr));
    if (need > free_b)
        return tsfail(tr, UMX_ERR_OOM, "%s: the object workspace of %d images of %d x %d needs %.1f MB, %.1f MB are free", what, io.B, io.P,
                      io.P, need / 1e6, free_b / 1e6);
    ObjectWorkspace n;
    n.B = io.B; n.P = io.P; n.slots = slots;
    TS_TRY(ts_alloc(ts, &n.planes, 2 * part));
    TS_TRY(ts_alloc(ts, &n.words, 6 * part));
    TS_TRY(ts_alloc(ts, &n.keys, (size_t)io.B * slots));
    TS_TRY(ts_alloc(ts, &n.overlap, (size_t)io.B * slots));
    TS_TRY(ts_alloc(ts, &n.counts, (size_t)io.B * UMX_OBJECT_COUNTS));
    w = n;
    return UMX_OK;
}

// umx_trainer_evaluate (o == nullptr: nothing below the class counts is enqueued or read) and umx_trainer_evaluate_objects
int evaluate_batch(umx_trainer* tr, umx_trainset* ts, const umx_sample_desc* desc, int n, const umx_object_options* o, int64_t* counts,
                   double* loss_sum, int64_t* objects, uint8_t* truth_codes, uint8_t* pred_codes, const char* what) {
    if (!tr) return tsfail(nullptr, UMX_ERR_INVALID, "null trainer");
    const TrainerIO io = trainer_io(tr);
    TS_TRY(check_descs(tr, ts, desc, n, io.B, what));
    if (!counts || !loss_sum || (o && !objects)) return tsfail(tr, UMX_ERR_INVALID, "null argument");
    if (o) TS_TRY(object_begin(tr, ts, o, what));
    TS_TRY(trainer_eval_begin(tr));
    TS_TRY(enqueue_assemble(tr, ts, desc, n, false));
    TS_TRY(trainer_eval_forward(tr));
    TS_HIP(tr, launch_class_counts(io.probs, io.labels, (size_t)n * io.P * io.P, io.K, ts->part, ts->counts, ts->loss, io.stream));
    long long c[2 * kMaxClasses];
    double l = 0.0;
    TS_HIP(tr, hipMemcpyAsync(c, ts->counts, 2 * io.K * sizeof(long long), hipMemcpyDeviceToHost, io.stream));
    TS_HIP(tr, hipMemcpyAsync(&l, ts->loss, sizeof l, hipMemcpyDeviceToHost, io.stream));
    std::vector<long long> per;
    if (o) {
        const ObjectWorkspace& w = ts->obj;
        const size_t npix = (size_t)n * io.P * io.P, part = (size_t)w.B * w.P * w.P;
        per.resize((size_t)n * UMX_OBJECT_COUNTS);
        TS_HIP(tr, launch_object_planes(io.probs, io.labels, n, io.P, io.K, w.planes, w.planes + part, io.stream));
        TS_HIP(tr, launch_object_counts(w, n, o->object_code, o->min_area, io.stream));
        TS_HIP(tr, hipMemcpyAsync(per.data(), w.counts, per.size() * sizeof(long long), hipMemcpyDeviceToHost, io.stream));
        if (truth_codes) TS_HIP(tr, hipMemcpyAsync(truth_codes, w.planes, npix, hipMemcpyDeviceToHost, io.stream));
        if (pred_codes) TS_HIP(tr, hipMemcpyAsync(pred_codes, w.planes + part, npix, hipMemcpyDeviceToHost, io.stream));
    }
    const int rc = trainer_eval_end(tr);
    TS_TRY(guard_check(tr, ts));   // (a damaged zone before a range report)
    TS_TRY(rc);
    for (int q = 0; q < 2 * io.K; ++q) counts[q] = c[q];
    *loss_sum = l;
    if (o)
        for (int q = 0; q < UMX_OBJECT_COUNTS; ++q) {
            objects[q] = 0;
            for (int i = 0; i < n; ++i) objects[q] += per[(size_t)i * UMX_OBJECT_COUNTS + q];
        }
    return UMX_OK;
}

}  // namespace

extern "C" {

int umx_trainset_border_weights(umx_trainset* ts, int index, const umx_border_options* o) {
    TS_TRY(border_begin(ts, index, -1, o, false, "umx_trainset_border_weights"));
    umx_trainer* tr = ts->tr;
    const TrainerIO io = trainer_io(tr);
    const int first = index < 0 ? 0 : index, n = index < 0 ? ts->N : 1;
    const size_t plane = (size_t)ts->S * ts->S, plane_w = (size_t)ts->S * ts->row_f;
    int* ws = ts->border_ws + first * plane;
    TS_HIP(tr, hipStreamSynchronize(io.stream));   // (a step in flight may still read the map)
    TS_HIP(tr, launch_border_label(ts->ann + (size_t)first * ts->S * ts->row_a, n, ts->S, ts->row_a, o->object_code, ws, io.stream));
    TS_HIP(tr, launch_border_map(ws, n, ts->S, border_radius(o->sigma), 2.0 * ((double)o->sigma * (double)o->sigma),
                                 ts->wmap + first * plane_w, ts->row_f, plane_w, nullptr, nullptr, nullptr, io.stream));
    TS_HIP(tr, hipStreamSynchronize(io.stream));
    return guard_check(tr, ts);
}

int umx_trainset_border_planes(umx_trainset* ts, int index, const umx_border_options* o, int32_t* labels, int32_t* d1sq, int32_t* d2sq,
                               float* wmap) {
    TS_TRY(border_begin(ts, index, 0, o, true, "umx_trainset_border_planes"));
    umx_trainer* tr = ts->tr;
    const TrainerIO io = trainer_io(tr);
    const size_t plane = (size_t)ts->S * ts->S;
    int* ws = ts->border_ws + index * plane;
    int* dg = ts->border_diag;
    TS_HIP(tr, hipStreamSynchronize(io.stream));
    TS_HIP(tr, launch_border_label(ts->ann + (size_t)index * ts->S * ts->row_a, 1, ts->S, ts->row_a, o->object_code, ws, io.stream));
    TS_HIP(tr, launch_border_map(ws, 1, ts->S, border_radius(o->sigma), 2.0 * ((double)o->sigma * (double)o->sigma),
                                 reinterpret_cast<float*>(dg + 3 * plane), ts->S, plane, dg, dg + plane, dg + 2 * plane, io.stream));
    void* host[4] = {labels, d1sq, d2sq, wmap};
    for (int k = 0; k < 4; ++k)
        if (host[k]) TS_HIP(tr, hipMemcpyAsync(host[k], dg + k * plane, plane * sizeof(int), hipMemcpyDeviceToHost, io.stream));
    TS_HIP(tr, hipStreamSynchronize(io.stream));
    return guard_check(tr, ts);
}

int umx_trainset_create(umx_trainer* tr, int n_samples, int n_pages, int size, const umx_label_weights* lw, umx_trainset** out) {
    if (!tr || !lw || !out) return tsfail(tr, UMX_ERR_INVALID, "null argument");
    *out = nullptr;
    const TrainerIO io = trainer_io(tr);
    if (n_samples < 1 || n_pages < 1) return tsfail(tr, UMX_ERR_INVALID, "a training set needs at least one sample and one page");
    if (size < io.P || size > 65536)
        return tsfail(tr, UMX_ERR_INVALID, "samples of %d pixels: the trainer's tile is %d (size must be imSize .. 65536)", size, io.P);
    for (int i = 0; i < 7; ++i)
        if (lw->reserved[i]) return tsfail(tr, UMX_ERR_INVALID, "umx_label_weights.reserved must be zero");
    if (lw->weighted != 0 && lw->weighted != 1) return tsfail(tr, UMX_ERR_INVALID, "umx_label_weights.weighted must be 0 or 1");
    if (!lw->weighted && !io.legacy)
        return tsfail(tr, UMX_ERR_INVALID, "the v2 graph has no unweighted loss: give the set class / intersect weights");
    for (int k = 0; k < 8; ++k)
        if (!std::isfinite(lw->class_weight[k]) || !std::isfinite(lw->intersect_weight[k]))
            return tsfail(tr, UMX_ERR_INVALID, "class / intersect weights must be finite");
    umx_trainset* ts = new umx_trainset();
    ts->tr = tr;
    ts->N = n_samples; ts->pages = n_pages; ts->S = size; ts->C = io.C; ts->K = io.K;
    ts->row_f = (size + 3) & ~3;        // 16-byte rows
    ts->row_a = (size + 15) & ~15;
    ts->weighted = lw->weighted != 0;
    ts->lw = *lw;
    const size_t px_f = (size_t)n_samples * size * ts->row_f, px_a = (size_t)n_samples * size * ts->row_a;
    const size_t bytes = px_f * 4 * io.C * n_pages + px_a + (ts->weighted ? px_f * 4 : 0);
    size_t free_b = 0, total_b = 0;
    std::string why;
    int rc = arena_init(&ts->mem, &why);
    if (rc != UMX_OK) rc = tsfail(tr, rc, "%s", why.c_str());
    if (rc == UMX_OK && (rc = umx_device_mem_info(io.device, &free_b, &total_b)) != UMX_OK) rc = tsfail(tr, rc, "%s", umx_last_error(nullptr));
    else if (rc == UMX_OK && bytes > free_b)
        rc = tsfail(tr, UMX_ERR_OOM, "a training set of %d samples of %d x %d (%d channels x %d pages) needs %.1f MB, %.1f MB are free", n_samples,
                    size, size, io.C, n_pages, bytes / 1e6, free_b / 1e6);
    if (rc == UMX_OK) rc = hipSetDevice(io.device) == hipSuccess ? UMX_OK : tsfail(tr, UMX_ERR_HIP, "hipSetDevice failed");
    if (rc == UMX_OK) rc = ts_alloc(ts, &ts->planes, px_f * io.C * n_pages);
    if (rc == UMX_OK) rc = ts_alloc(ts, &ts->ann, px_a);
    if (rc == UMX_OK && ts->weighted) rc = ts_alloc(ts, &ts->wmap, px_f);
    if (rc == UMX_OK) rc = ts_alloc(ts, &ts->part, class_counts_parts((size_t)io.B * io.P * io.P, io.K));
    if (rc == UMX_OK) rc = ts_alloc(ts, &ts->counts, 2 * (size_t)io.K);
    if (rc == UMX_OK) rc = ts_alloc(ts, &ts->loss, 1);
    if (rc != UMX_OK) {
        umx_trainset_destroy(ts);
        return rc;
    }
    if (ts->mem.fill >= 0)
        fprintf(stderr, "[umx train] UMX_DEBUG_GUARD=0x%02x: %zu training-set buffers between red zones\n", ts->mem.fill, ts->mem.blocks.size());
    *out = ts;
    return UMX_OK;
}

int umx_trainset_set(umx_trainset* ts, int index, const float* planes, const uint8_t* annotation, const float* weight_map) {
    if (!ts) return tsfail(nullptr, UMX_ERR_INVALID, "null training set");
    umx_trainer* tr = ts->tr;
    if (!planes || !annotation) return tsfail(tr, UMX_ERR_INVALID, "null argument");
    if (index < 0 || index >= ts->N) return tsfail(tr, UMX_ERR_INVALID, "sample %d of a set of %d", index, ts->N);
    const TrainerIO io = trainer_io(tr);
    const size_t S = ts->S, plane = S * ts->row_f;
    TS_HIP(tr, hipSetDevice(io.device));
    TS_HIP(tr, hipStreamSynchronize(io.stream));   // (a step in flight may still read the set)
    const int np = ts->C * ts->pages;
    TS_HIP(tr, hipMemcpy2DAsync(ts->planes + (size_t)index * np * plane, ts->row_f * sizeof(float), planes, S * sizeof(float),
                                S * sizeof(float), S * np, hipMemcpyHostToDevice, io.stream));
    TS_HIP(tr, hipMemcpy2DAsync(ts->ann + (size_t)index * S * ts->row_a, ts->row_a, annotation, S, S, S, hipMemcpyHostToDevice, io.stream));
    if (ts->weighted) {   // (an unweighted set has no map to keep)
        float* dst = ts->wmap + (size_t)index * plane;
        if (weight_map)
            TS_HIP(tr, hipMemcpy2DAsync(dst, ts->row_f * sizeof(float), weight_map, S * sizeof(float), S * sizeof(float), S,
                                        hipMemcpyHostToDevice, io.stream));
        else
            TS_HIP(tr, hipMemsetAsync(dst, 0, plane * sizeof(float), io.stream));   // a missing map counts as 0
    }
    TS_HIP(tr, hipStreamSynchronize(io.stream));
    return guard_check(tr, ts);
}

void umx_trainset_destroy(umx_trainset* ts) {
    if (!ts) return;
    if (!ts->mem.allocs.empty()) {
        const TrainerIO io = trainer_io(ts->tr);
        (void)hipSetDevice(io.device);
        (void)hipStreamSynchronize(io.stream);
        arena_free(&ts->mem);
    }
    delete ts;
}

int umx_train_step_sampled(umx_trainer* tr, const umx_trainset* ts, const umx_sample_desc* desc, int apply_update) {
    return step_from_set(tr, ts, desc, nullptr, nullptr, nullptr, 0, apply_update, "umx_train_step_sampled");
}

int umx_train_step_augmented(umx_trainer* tr, const umx_trainset* ts, const umx_sample_desc* desc, const umx_augment_desc* aug,
                             int apply_update) {
    return step_from_set(tr, ts, desc, aug, nullptr, nullptr, kNeedsAug, apply_update, "umx_train_step_augmented");
}

int umx_train_step_warped(umx_trainer* tr, const umx_trainset* ts, const umx_sample_desc* desc, const umx_augment_desc* aug,
                          const umx_warp_desc* warp, int apply_update) {
    return step_from_set(tr, ts, desc, aug, warp, nullptr, kNeedsWarp, apply_update, "umx_train_step_warped");
}

int umx_trainer_assemble(umx_trainer* tr, const umx_trainset* ts, const umx_sample_desc* desc, int n, float* data, float* labels,
                         float* weights) {
    return assemble_to_host(tr, ts, desc, nullptr, nullptr, nullptr, 0, n, data, labels, weights, "umx_trainer_assemble");
}

int umx_trainer_assemble_augmented(umx_trainer* tr, const umx_trainset* ts, const umx_sample_desc* desc, const umx_augment_desc* aug,
                                   int n, float* data, float* labels, float* weights) {
    return assemble_to_host(tr, ts, desc, aug, nullptr, nullptr, kNeedsAug, n, data, labels, weights, "umx_trainer_assemble_augmented");
}

int umx_trainer_assemble_warped(umx_trainer* tr, const umx_trainset* ts, const umx_sample_desc* desc, const umx_augment_desc* aug,
                                const umx_warp_desc* warp, int n, float* data, float* labels, float* weights) {
    return assemble_to_host(tr, ts, desc, aug, warp, nullptr, kNeedsWarp, n, data, labels, weights, "umx_trainer_assemble_warped");
}

int umx_train_step_elastic(umx_trainer* tr, const umx_trainset* ts, const umx_sample_desc* desc, const umx_augment_desc* aug,
                           const umx_warp_desc* warp, const umx_elastic_desc* elastic, int apply_update) {
    return step_from_set(tr, ts, desc, aug, warp, elastic, kNeedsElastic, apply_update, "umx_train_step_elastic");
}

int umx_trainer_assemble_elastic(umx_trainer* tr, const umx_trainset* ts, const umx_sample_desc* desc, const umx_augment_desc* aug,
                                 const umx_warp_desc* warp, const umx_elastic_desc* elastic, int n, float* data, float* labels,
                                 float* weights) {
    return assemble_to_host(tr, ts, desc, aug, warp, elastic, kNeedsElastic, n, data, labels, weights, "umx_trainer_assemble_elastic");
}

int umx_elastic_desc_check(const umx_elastic_desc* e, int n_desc, char* msg, size_t cap) {
    char buf[160] = "";
    if (!e) snprintf(buf, sizeof buf, "null elastic descriptors");
    for (int i = 0; !buf[0] && i < n_desc; ++i) {
        const int n = e[i].n;
        const char* why = nullptr;
        if (n != 0 && (n < 4 || n > UMX_ELASTIC_MAX_GRID)) why = "n is not 0 or 4..6";
        else if (e[i].reserved[0] || e[i].reserved[1] || e[i].reserved[2]) why = "reserved field not zero";
        for (int k = 0; k < 2 && !why; ++k)
            for (int a = 0; a < UMX_ELASTIC_MAX_GRID && !why; ++a)
                for (int b = 0; b < UMX_ELASTIC_MAX_GRID && !why; ++b) {
                    const float v = e[i].d[k][a][b];
                    if (!std::isfinite(v)) why = "an entry is not finite";
                    else if (std::fabs(v) > UMX_ELASTIC_MAX_DISP) why = "an entry is above 32 pixels in magnitude";
                    else if ((a >= n || b >= n) && v != 0.f) why = "a non-zero entry outside the n x n block";
                }
        if (why) snprintf(buf, sizeof buf, "elastic %d (n %d): %s", i, n, why);
    }
    if (msg && cap) snprintf(msg, cap, "%s", buf);
    return buf[0] ? UMX_ERR_INVALID : UMX_OK;
}

int umx_warp_desc_check(const umx_warp_desc* warp, int n, char* msg, size_t cap) {
    char buf[160] = "";
    if (!warp) snprintf(buf, sizeof buf, "null warp descriptors");
    for (int i = 0; !buf[0] && i < n; ++i) {
        const float* m = warp[i].m;
        const char* why = nullptr;
        for (int k = 0; k < 4 && !why; ++k)
            if (!std::isfinite(m[k])) why = "an entry is not finite";
            else if (std::fabs(m[k]) > 4.f) why = "an entry is above 4 in magnitude";
        if (!why && (double)m[0] * (double)m[3] - (double)m[1] * (double)m[2] == 0.0) why = "the matrix is singular";
        if (why)
            snprintf(buf, sizeof buf, "warp %d (%g, %g, %g, %g): %s", i, (double)m[0], (double)m[1], (double)m[2], (double)m[3], why);
    }
    if (msg && cap) snprintf(msg, cap, "%s", buf);
    return buf[0] ? UMX_ERR_INVALID : UMX_OK;
}

int umx_augment_table_check(const umx_augment_table* t, char* msg, size_t cap) {
    char buf[160] = "";
    if (!t) snprintf(buf, sizeof buf, "null table");
    else if (t->n_levels < 1 || t->n_levels > UMX_AUGMENT_MAX_LEVELS)
        snprintf(buf, sizeof buf, "n_levels is %d: a table holds 1..%d levels", t->n_levels, UMX_AUGMENT_MAX_LEVELS);
    else if (t->radius[0] != 0) snprintf(buf, sizeof buf, "level 0 is 'no blur': its radius must be 0, not %d", t->radius[0]);
    else if (!std::isfinite(t->mean)) snprintf(buf, sizeof buf, "mean is not finite");
    else if (!std::isfinite(t->std) || !(t->std > 0.f)) snprintf(buf, sizeof buf, "std must be finite and > 0");
    for (int l = 0; !buf[0] && l < t->n_levels; ++l) {
        if (t->radius[l] < 0 || t->radius[l] > UMX_AUGMENT_MAX_RADIUS)
            snprintf(buf, sizeof buf, "radius of level %d is %d, outside 0..%d", l, t->radius[l], UMX_AUGMENT_MAX_RADIUS);
        for (int k = 0; !buf[0] && k <= t->radius[l]; ++k)
            if (!std::isfinite(t->taps[l][k]) || t->taps[l][k] < 0.f)
                snprintf(buf, sizeof buf, "tap %d of level %d is not finite or negative", k, l);
    }
    for (int i = 0; !buf[0] && i < 5; ++i)
        if (t->reserved[i]) snprintf(buf, sizeof buf, "reserved must be zero");
    if (msg && cap) snprintf(msg, cap, "%s", buf);
    return buf[0] ? UMX_ERR_INVALID : UMX_OK;
}

int umx_trainset_set_augment(umx_trainset* ts, const umx_augment_table* table) {
    if (!ts) return tsfail(nullptr, UMX_ERR_INVALID, "null training set");
    umx_trainer* tr = ts->tr;
    char why[160];
    if (umx_augment_table_check(table, why, sizeof why) != UMX_OK) return tsfail(tr, UMX_ERR_INVALID, "umx_augment_table: %s", why);
    const TrainerIO io = trainer_io(tr);
    TS_HIP(tr, hipSetDevice(io.device));
    TS_HIP(tr, hipStreamSynchronize(io.stream));
    ts->aug = *table;
    ts->has_aug = true;
    return UMX_OK;
}

int umx_trainer_evaluate(umx_trainer* tr, const umx_trainset* ts, const umx_sample_desc* desc, int n, int64_t* counts, double* loss_sum) {
    // (without options the set is only read)
    return evaluate_batch(tr, const_cast<umx_trainset*>(ts), desc, n, nullptr, counts, loss_sum, nullptr, nullptr, nullptr, "umx_trainer_evaluate");
}

int umx_trainer_evaluate_objects(umx_trainer* tr, umx_trainset* ts, const umx_sample_desc* desc, int n, const umx_object_options* o,
                                 int64_t* counts, double* loss_sum, int64_t* objects, uint8_t* truth_codes, uint8_t* pred_codes) {
    if (!o) return tsfail(tr, UMX_ERR_INVALID, "umx_trainer_evaluate_objects: null object options");
    return evaluate_batch(tr, ts, desc, n, o, counts, loss_sum, objects, truth_codes, pred_codes, "umx_trainer_evaluate_objects");
}

int umx_trainer_object_counts(umx_trainer* tr, umx_trainset* ts, const uint8_t* truth_codes, const uint8_t* pred_codes, int n,
                              const umx_object_options* o, int64_t* per_image, int32_t* truth_labels, int32_t* pred_labels) {
    const char* what = "umx_trainer_object_counts";
    if (!tr) return tsfail(nullptr, UMX_ERR_INVALID, "null trainer");
    if (!ts || !truth_codes || !pred_codes || !per_image) return tsfail(tr, UMX_ERR_INVALID, "null argument");
    if (ts->tr != tr) return tsfail(tr, UMX_ERR_INVALID, "%s: the training set belongs to another trainer", what);
    const TrainerIO io = trainer_io(tr);
    if (n < 1 || n > io.B) return tsfail(tr, UMX_ERR_INVALID, "%s: %d images, the batch holds 1..%d", what, n, io.B);
    TS_TRY(object_begin(tr, ts, o, what));
    const ObjectWorkspace& w = ts->obj;
    const size_t plane = (size_t)w.P * w.P, npix = (size_t)n * plane, part = (size_t)w.B * plane;
    TS_HIP(tr, hipMemcpyAsync(w.planes, truth_codes, npix, hipMemcpyHostToDevice, io.stream));
    TS_HIP(tr, hipMemcpyAsync(w.planes + part, pred_codes, npix, hipMemcpyHostToDevice, io.stream));
    TS_HIP(tr, launch_object_rule(w.planes, w.planes + part, n, w.P, io.stream));
    TS_HIP(tr, launch_object_counts(w, n, o->object_code, o->min_area, io.stream));
    std::vector<long long> per((size_t)n * UMX_OBJECT_COUNTS);
    TS_HIP(tr, hipMemcpyAsync(per.data(), w.counts, per.size() * sizeof(long long), hipMemcpyDeviceToHost, io.stream));
    if (truth_labels) TS_HIP(tr, hipMemcpyAsync(truth_labels, w.words, npix * sizeof(int), hipMemcpyDeviceToHost, io.stream));
    if (pred_labels) TS_HIP(tr, hipMemcpyAsync(pred_labels, w.words + part, npix * sizeof(int), hipMemcpyDeviceToHost, io.stream));
    TS_HIP(tr, hipStreamSynchronize(io.stream));
    TS_TRY(guard_check(tr, ts));
    for (size_t q = 0; q < per.size(); ++q) per_image[q] = per[q];
    for (int32_t* lab : {truth_labels, pred_labels})       // the planes hold roots (-1 off the objects): a label is root + 1
        for (size_t q = 0; lab && q < npix; ++q) lab[q] += 1;
    return UMX_OK;
}

}  // extern "C"
