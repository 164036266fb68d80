// libumx object-level validation score: the kernels behind umx_trainer_evaluate_objects / umx_trainer_object_counts (include/umx_train.h,
// DESIGN.md section 9.2 "Object score") and the host check of their options.  The labelling itself is border_label_kernel
// (umx_trainset_border.hip), launched twice with S = row_a = P: one workgroup per image, canonical roots.
//
//   object_planes_kernel  one thread per pixel of the batch: truth code (k + 1 of the one-hot label, 0 unlabelled) and predicted code
//                         (1 + first maximum of the K probabilities, 0 where the truth is 0) into two uint8 planes [n][P][P]
//   object_rule_kernel    the same rule (pred = 0 where truth = 0) on planes that were uploaded (umx_trainer_object_counts)
//   object_pairs_kernel   one wave per row of an image: the row is cut into runs of equal (truth root, predicted root) with ballots; the
//                         head of a run adds the run's length to the area word of either root and to the overlap of the pair, which
//                         lives in an open-addressing table of the image (key t * P^2 + p + 1, 0 = empty; atomicCAS, then atomicAdd)
//   object_reduce_kernel  one workgroup per image: over the table's slots the two match rules and, per root, how many partners lie
//                         mostly inside it; then over the roots the object counts and the merge / split rules; eight int64 per image
//
// Every value is an integer sum, so no result depends on the order in which the atomics arrive; where a pair lands in its table does,
// and nothing reads that.  No workgroup waits for another one: a kernel reads only what the launches before it finished, except for
// the per-root partner counts, which one workgroup writes (atomicAdd), fences, and reads back itself.
#include "../../include/umx_train.h"
#include "umx_internal.h"

#include <climits>
#include <cstdio>

namespace umx {

namespace {

constexpr int kPlaneThreads = 256;
constexpr int kPairWaves = 4;                            // rows of an image per workgroup of the pair pass
constexpr int kReduceThreads = 1024;                     // one workgroup per image
constexpr int kMaxClasses = 8;                           // umx_trainer_create: nClasses 2..8

// The plane rule of the definition: an unlabelled pixel is outside the evaluation, so nothing is predicted there.  Both ways into the
// planes (the trainer's probabilities, uploaded codes) go through here.
__device__ inline uint8_t object_pred_code(uint8_t truth, uint8_t pred) { return truth == 0 ? (uint8_t)0 : pred; }

__global__ void __launch_bounds__(kPlaneThreads) object_planes_kernel(const float* __restrict__ probs, const float* __restrict__ labels,
                                                                      size_t npix, int K, uint8_t* __restrict__ truth,
                                                                      uint8_t* __restrict__ pred) {
    const size_t i = (size_t)blockIdx.x * kPlaneThreads + threadIdx.x;
    if (i >= npix) return;
    const float* p = probs + i * K;
    const float* l = labels + i * K;
    int lab = -1, arg = 0;
    float best = p[0];
    for (int k = 0; k < K; ++k) {
        if (lab < 0 && l[k] != 0.f) lab = k;
        if (k > 0 && p[k] > best) { best = p[k]; arg = k; }   // first maximum, as class_counts_kernel
    }
    const uint8_t t = (uint8_t)(lab + 1);
    truth[i] = t;
    pred[i] = object_pred_code(t, (uint8_t)(arg + 1));
}

__global__ void __launch_bounds__(kPlaneThreads) object_rule_kernel(const uint8_t* __restrict__ truth, uint8_t* __restrict__ pred,
                                                                    size_t npix) {
    const size_t i = (size_t)blockIdx.x * kPlaneThreads + threadIdx.x;
    if (i >= npix) return;
    pred[i] = object_pred_code(truth[i], pred[i]);
}

// where a key starts probing: the top bits of a Fibonacci hash (shift = 64 - log2(slots))
__device__ inline unsigned slot_of(unsigned long long key, int shift) { return (unsigned)((key * 0x9E3779B97F4A7C15ull) >> shift); }

// grid (ceil(P / 4), n).  T / Q: the image's root planes (flat index of the component's first pixel, -1 off the objects).  A lane past
// the row's end holds (-2, -2), which no pixel has: the first such lane heads a run of its own, so a run of pixels never reaches it.
// Loop bounds: ceil(P / 64) chunks; a probe sequence visits each of the `slots` slots at most once, and because an image has fewer than
// P^2 <= slots / 2 distinct pairs it meets its own key or an empty slot long before that.
__global__ void __launch_bounds__(64 * kPairWaves) object_pairs_kernel(const int* __restrict__ troot, const int* __restrict__ proot,
                                                                       int P, size_t stride, int* __restrict__ area_t,
                                                                       int* __restrict__ area_p, unsigned long long* __restrict__ keys,
                                                                       int* __restrict__ overlap, int slots, int shift) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int y = blockIdx.x * kPairWaves + wave;
    if (y >= P) return;                                   // (the whole wave: no barrier below)
    const size_t img = (size_t)blockIdx.y * stride;
    const int* T = troot + img + (size_t)y * P;
    const int* Q = proot + img + (size_t)y * P;
    int* At = area_t + img;
    int* Ap = area_p + img;
    unsigned long long* Kt = keys + (size_t)blockIdx.y * slots;
    int* Ov = overlap + (size_t)blockIdx.y * slots;
    const unsigned long long P2 = (unsigned long long)P * P;
    for (int x0 = 0; x0 < P; x0 += 64) {
        const int x = x0 + lane;
        const int t = x < P ? T[x] : -2, p = x < P ? Q[x] : -2;
        const int tl = __shfl_up(t, 1), pl = __shfl_up(p, 1);
        const bool head = lane == 0 || t != tl || p != pl;
        const unsigned long long heads = __ballot(head);
        const unsigned long long later = lane == 63 ? 0ull : heads >> (lane + 1);
        const int len = later ? __ffsll((long long)later) : 64 - lane;   // pixels up to the next head, or to the chunk's end
        if (head && t >= 0) atomicAdd(At + t, len);
        if (head && p >= 0) atomicAdd(Ap + p, len);
        if (head && t >= 0 && p >= 0) {
            const unsigned long long key = (unsigned long long)t * P2 + (unsigned long long)p + 1ull;
            unsigned h = slot_of(key, shift);
            for (int probe = 0; probe < slots; ++probe) {
                const unsigned long long old = atomicCAS(Kt + h, 0ull, key);
                if (old == 0ull || old == key) {
                    atomicAdd(Ov + h, len);
                    break;
                }
                h = (h + 1u) & (unsigned)(slots - 1);
            }
        }
    }
}

// the partner counts are changed with atomicAdd, which executes in L2: read them back through L2 too (relaxed, agent scope)
__device__ inline int count_load(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// out: int64[8] of image blockIdx.x = truth, predicted, matched, matched75, merged, split, 0, 0.  in_t[t] / in_p[p] (zero on entry):
// the kept predicted objects that lie mostly inside truth object t, resp. the truth objects that lie mostly inside predicted object p.
// Two loops of ceil(slots / 1024) and ceil(P^2 / 1024) rounds, a barrier between them.
__global__ void __launch_bounds__(kReduceThreads) object_reduce_kernel(const int* __restrict__ troot, const int* __restrict__ proot, int P,
                                                                       size_t stride, const int* __restrict__ area_t,
                                                                       const int* __restrict__ area_p, int* __restrict__ in_t,
                                                                       int* __restrict__ in_p, const unsigned long long* __restrict__ keys,
                                                                       const int* __restrict__ overlap, int slots, int min_area,
                                                                       long long* __restrict__ out) {
    __shared__ unsigned long long tot[UMX_OBJECT_COUNTS];
    const size_t img = (size_t)blockIdx.x * stride;
    const int* T = troot + img;
    const int* Q = proot + img;
    const int* At = area_t + img;
    const int* Ap = area_p + img;
    int* It = in_t + img;
    int* Ip = in_p + img;
    const unsigned long long* Kt = keys + (size_t)blockIdx.x * slots;
    const int* Ov = overlap + (size_t)blockIdx.x * slots;
    const unsigned long long P2 = (unsigned long long)P * P;
    const int npix = P * P;
    if (threadIdx.x < UMX_OBJECT_COUNTS) tot[threadIdx.x] = 0ull;
    __syncthreads();
    unsigned long long n_truth = 0, n_pred = 0, matched = 0, matched75 = 0, merged = 0, split = 0;
    for (int s = threadIdx.x; s < slots; s += kReduceThreads) {
        const unsigned long long key = Kt[s];
        if (key == 0ull) continue;
        const int t = (int)((key - 1ull) / P2), p = (int)((key - 1ull) % P2);
        const long long I = Ov[s], at = At[t], ap = Ap[p];
        if (ap < min_area) continue;                      // a predicted object below min_area does not exist
        matched += 3 * I > at + ap;                       // IoU > 1/2:  I / (at + ap - I) > 1/2
        matched75 += 7 * I > 3 * (at + ap);               // IoU > 3/4
        if (2 * I > at) atomicAdd(Ip + p, 1);
        if (2 * I > ap) atomicAdd(It + t, 1);
    }
    __threadfence();
    __syncthreads();
    for (int i = threadIdx.x; i < npix; i += kReduceThreads) {
        if (T[i] == i) {
            n_truth += 1;
            split += count_load(It + i) >= 2;
        }
        if (Q[i] == i && Ap[i] >= min_area) {
            n_pred += 1;
            merged += count_load(Ip + i) >= 2;
        }
    }
    const unsigned long long mine[6] = {n_truth, n_pred, matched, matched75, merged, split};
#pragma unroll
    for (int q = 0; q < 6; ++q)
        if (mine[q]) atomicAdd(&tot[q], mine[q]);
    __syncthreads();
    if (threadIdx.x < UMX_OBJECT_COUNTS) out[(size_t)blockIdx.x * UMX_OBJECT_COUNTS + threadIdx.x] = (long long)tot[threadIdx.x];
}

}  // namespace

size_t object_table_slots(int P) {
    size_t s = 64;
    while (s < 2 * (size_t)P * P) s <<= 1;
    return s;
}

hipError_t launch_object_planes(const float* probs, const float* labels, int n, int P, int K, uint8_t* truth, uint8_t* pred,
                                hipStream_t stream) {
    if (n < 1 || P < 1 || K < 1 || K > kMaxClasses) return hipErrorInvalidValue;
    const size_t npix = (size_t)n * P * P;
    hipLaunchKernelGGL(object_planes_kernel, dim3((unsigned)((npix + kPlaneThreads - 1) / kPlaneThreads)), dim3(kPlaneThreads), 0, stream,
                       probs, labels, npix, K, truth, pred);
    return hipGetLastError();
}

hipError_t launch_object_rule(const uint8_t* truth, uint8_t* pred, int n, int P, hipStream_t stream) {
    if (n < 1 || P < 1) return hipErrorInvalidValue;
    const size_t npix = (size_t)n * P * P;
    hipLaunchKernelGGL(object_rule_kernel, dim3((unsigned)((npix + kPlaneThreads - 1) / kPlaneThreads)), dim3(kPlaneThreads), 0, stream,
                       truth, pred, npix);
    return hipGetLastError();
}

hipError_t launch_object_counts(const ObjectWorkspace& w, int n, int code, int min_area, hipStream_t stream) {
    if (n < 1 || n > w.B || w.P < 1 || w.P > kObjectMaxTile || code < 1 || code > 255 || min_area < 1) return hipErrorInvalidValue;
    if (w.slots != object_table_slots(w.P)) return hipErrorInvalidValue;
    const size_t plane = (size_t)w.P * w.P, part = (size_t)w.B * plane;
    int* troot = w.words;                                 // [6][B][P^2]: roots of truth | of pred | areas | areas | partners | partners
    int* proot = w.words + part;
    hipError_t e;
    if ((e = hipMemsetAsync(w.words + 2 * part, 0, 4 * part * sizeof(int), stream)) != hipSuccess) return e;
    if ((e = hipMemsetAsync(w.keys, 0, (size_t)n * w.slots * sizeof(unsigned long long), stream)) != hipSuccess) return e;
    if ((e = hipMemsetAsync(w.overlap, 0, (size_t)n * w.slots * sizeof(int), stream)) != hipSuccess) return e;
    if ((e = launch_border_label(w.planes, n, w.P, w.P, code, troot, stream)) != hipSuccess) return e;
    if ((e = launch_border_label(w.planes + part, n, w.P, w.P, code, proot, stream)) != hipSuccess) return e;
    int shift = 64;
    for (size_t s = w.slots; s > 1; s >>= 1) --shift;     // 64 - log2(slots), slots >= 64
    hipLaunchKernelGGL(object_pairs_kernel, dim3((unsigned)((w.P + kPairWaves - 1) / kPairWaves), (unsigned)n), dim3(64 * kPairWaves), 0,
                       stream, troot, proot, w.P, plane, w.words + 2 * part, w.words + 3 * part, w.keys, w.overlap, (int)w.slots, shift);
    hipLaunchKernelGGL(object_reduce_kernel, dim3((unsigned)n), dim3(kReduceThreads), 0, stream, troot, proot, w.P, plane,
                       w.words + 2 * part, w.words + 3 * part, w.words + 4 * part, w.words + 5 * part, w.keys, w.overlap, (int)w.slots,
                       min_area, w.counts);
    return hipGetLastError();
}

}  // namespace umx

extern "C" {

int umx_object_options_check(const umx_object_options* o, int n_classes, char* msg, size_t cap) {
    char buf[160] = "";
    if (!o) snprintf(buf, sizeof buf, "null object options");
    else if (o->object_code < 1 || o->object_code > n_classes)
        snprintf(buf, sizeof buf, "object_code is %d: the objects' class code is 1..%d", o->object_code, n_classes);
    else if (o->min_area < 1 || o->min_area > UMX_OBJECT_MAX_MIN_AREA)
        snprintf(buf, sizeof buf, "min_area is %d: it must be 1..%d pixels", o->min_area, UMX_OBJECT_MAX_MIN_AREA);
    for (int i = 0; o && !buf[0] && i < 6; ++i)
        if (o->reserved[i]) snprintf(buf, sizeof buf, "reserved must be zero");
    if (msg && cap) snprintf(msg, cap, "%s", buf);
    return buf[0] ? UMX_ERR_INVALID : UMX_OK;
}

}  // extern "C"
