// libumx label mask, relabel: drop and merge objects and renumber the rest 1..N' -- the kernels and the C ABI behind
// umx_labeler_relabel / _relabel_dev (include/umx.h).  The classes and their numbering are host
// work (umx_relabel_host.h: `keep` and `pairs` come from tables the host has); the device gets the finished map of N + 1 words and
// one call is this sequence on the labeler's stream:
//
//   (the map goes up into an allocation of its own)
//   relabel_table_init_kernel    one thread per NEW record: the empty record                      } on the resident labels only
//   relabel_table_merge_kernel   one thread per OLD label j: its record into new[map[j] - 1]      }
//   relabel_plane_kernel         one wave per row: labels'(y, x) = map[labels(y, x)], in place over the resident plane or from the
//                                caller's plane into the caller's output plane (which may be the same)
//   (the plane and the new table come down; on the resident labels the two tables change places)
//
// The plane pass.  A row is walked in chunks of 64 pixels.  A chunk in which no pixel has a label in 1..N is not looked up: it is
// written as zeros where it is not zero already (out of place: everywhere).  In any other chunk the first lane of every run of equal
// labels loads the run's word of the map and the others take it from that lane by a shuffle, so a nucleus of w pixels in a row costs
// one load of the map, not w: the map of a whole slide (4.4 MB for 1.1 M objects) does not fit an XCD's L2, and the pass is to cost
// the plane's own traffic.  A run that crosses a chunk's end is looked up once per chunk.  A pixel whose new value is its old one is
// not written in place.
//
// Why no thread waits for another one: a workgroup reads and writes only words of its own rows, every pixel depends on its own word
// alone (so in place is safe), and nobody writes the map.  The merge takes the integer atomics of label_write_kernel (int32 add / min /
// max, int64 add) on records that nothing reads before the launch ends.  Why the result does not depend on any order: sums, minima
// and maxima of integers.
#include "../../include/umx.h"
#include "umx_internal.h"
#include "umx_label_state.h"
#include "umx_relabel_host.h"

#include <climits>
#include <new>

namespace umx {

namespace {

constexpr int kRowWaves = 4;                             // rows of the image per workgroup
constexpr int kPixThreads = 256;                         // one thread per record
static_assert(sizeof(umx_label_object) == 40, "the object record");
const char* const kMidway = "a umx_labeler_relabel failed after its first launch: the resident labels are partly renumbered";

// one thread per record, j < n
__global__ void __launch_bounds__(kPixThreads) relabel_table_init_kernel(umx_label_object* __restrict__ table, long long n) {
    const long long j = (long long)blockIdx.x * kPixThreads + threadIdx.x;
    if (j >= n) return;
    umx_label_object o;
    o.area = 0; o.y0 = INT_MAX; o.x0 = INT_MAX; o.y1 = -1; o.x1 = -1; o.reserved = 0; o.sum_y = 0; o.sum_x = 0;
    table[j] = o;
}

// one thread per old label j + 1, j < N.  old [N] and map [N + 1] are only read; fresh [n_new] takes integer atomics at record
// map[j + 1] - 1, which is inside 0 .. n_new (checked), and nothing reads it in this launch.  A record without pixels adds nothing.
__global__ void __launch_bounds__(kPixThreads) relabel_table_merge_kernel(const umx_label_object* __restrict__ old, const int* __restrict__ map,
                                                                          long long N, long long n_new, umx_label_object* __restrict__ fresh) {
    const long long j = (long long)blockIdx.x * kPixThreads + threadIdx.x;
    if (j >= N) return;
    const int m = map[j + 1];
    if (m < 1 || m > n_new) return;
    const umx_label_object o = old[j];
    if (o.area <= 0) return;
    umx_label_object* t = fresh + (m - 1);
    atomicAdd(&t->area, o.area);
    atomicMin(&t->y0, o.y0);
    atomicMax(&t->y1, o.y1);
    atomicMin(&t->x0, o.x0);
    atomicMax(&t->x1, o.x1);
    atomicAdd(reinterpret_cast<unsigned long long*>(&t->sum_y), (unsigned long long)o.sum_y);
    atomicAdd(reinterpret_cast<unsigned long long*>(&t->sum_x), (unsigned long long)o.sum_x);
}

// grid ceil(H / 4).  src [H][W] and dst [H][W] may be the same plane: a lane reads src at its own pixel before it writes dst there, and
// no other thread touches that word (row y < H by its wave; a pixel word is y * W + x < H * W <= INT_MAX).  map [N + 1] is only read,
// at a label in 1..N; any other value counts as 0 and is never an index.
__global__ void __launch_bounds__(64 * kRowWaves) relabel_plane_kernel(const int* src, int* dst, int H, int W, int N, const int* __restrict__ map) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if ((long long)blockIdx.x * kRowWaves + wave >= H) return;    // (the whole wave: no barrier below)
    const int y = blockIdx.x * kRowWaves + wave;
    const int* in = src + (size_t)y * W;
    int* out = dst + (size_t)y * W;
    const bool in_place = src == dst;
    const int nchunks = (W - 1) / 64 + 1;
    for (int c = 0; c < nchunks; ++c) {
        const int x0 = c * 64;
        const bool inside = lane < W - x0;
        const int x = x0 + lane;
        const int v = inside ? in[x] : 0;
        const int t = v >= 1 && v <= N ? v : 0;
        if (__ballot(t != 0) == 0ull) {                   // nothing labelled here (wave-uniform): no look-up
            if (inside && (!in_place || v != 0)) out[x] = 0;
            continue;
        }
        const int tl = __shfl_up(t, 1);
        const bool head = lane == 0 || t != tl;
        const unsigned long long heads = __ballot(head);  // (bit 0 is always set)
        int m = head && t ? map[t] : 0;                   // one load per run
        const int hl = 63 - __clzll((long long)(heads & (~0ull >> (63 - lane))));   // the head of this lane's run
        m = __shfl(m, hl);
        if (inside && (!in_place || m != v)) out[x] = m;
    }
}

inline unsigned row_grid(int H) { return (unsigned)((H - 1) / kRowWaves + 1); }
inline unsigned record_grid(long long n) { return (unsigned)((n + kPixThreads - 1) / kPixThreads); }

// The device part of a call whose arguments are checked and whose map (N + 1 words, n_new classes) is made.  resident: src == dst ==
// d_P and the object table follows; else the caller's planes and no table.  Returns with the stream idle.
int relabel_launches(umx_labeler* lb, const int* src, int* dst, long long N, int H, int W, const int32_t* map, long long n_new, bool resident,
                     int32_t* labels_host) {
    L_HIP(lb, hipSetDevice(lb->device));
    lb->rms[0] = lb->rms[1] = lb->rms[2] = 0.0;
    hipStream_t s = lb->stream;
    int rc = ensure_measure_buffer(lb, &lb->d_rmap, &lb->rmap_cap, (size_t)N + 1, sizeof(int), "relabel map");
    if (rc) return rc;
    std::vector<umx_label_object> fresh;
    if (resident) {
        if ((rc = ensure_measure_buffer(lb, &lb->d_rtable, &lb->rtable_cap, (size_t)n_new, sizeof(umx_label_object), "relabel table"))) return rc;
        try {
            fresh.resize((size_t)n_new);
        } catch (const std::bad_alloc&) {
            return lfail(lb, UMX_ERR_OOM, "no host memory for a table of %lld objects", n_new);
        }
    }
    const size_t npix = (size_t)H * W;
    L_HIP(lb, hipEventRecord(lb->ev[0], s));
    L_HIP(lb, hipMemcpyAsync(lb->d_rmap, map, ((size_t)N + 1) * sizeof(int), hipMemcpyHostToDevice, s));
    L_HIP(lb, hipEventRecord(lb->ev[1], s));
    if (resident) {
        lb->res_why = kMidway;                            // until the call has ended well
        if (n_new > 0) {
            hipLaunchKernelGGL(relabel_table_init_kernel, dim3(record_grid(n_new)), dim3(kPixThreads), 0, s, lb->d_rtable, n_new);
            hipLaunchKernelGGL(relabel_table_merge_kernel, dim3(record_grid(N)), dim3(kPixThreads), 0, s, lb->d_table, lb->d_rmap, N, n_new,
                               lb->d_rtable);
        }
    }
    hipLaunchKernelGGL(relabel_plane_kernel, dim3(row_grid(H)), dim3(64 * kRowWaves), 0, s, src, dst, H, W, (int)N, lb->d_rmap);
    L_HIP(lb, hipGetLastError());
    L_HIP(lb, hipEventRecord(lb->ev[2], s));
    if (labels_host) L_HIP(lb, hipMemcpyAsync(labels_host, dst, npix * sizeof(int), hipMemcpyDeviceToHost, s));
    if (resident && n_new > 0)
        L_HIP(lb, hipMemcpyAsync(fresh.data(), lb->d_rtable, (size_t)n_new * sizeof(umx_label_object), hipMemcpyDeviceToHost, s));
    L_HIP(lb, hipEventRecord(lb->ev[3], s));
    L_HIP(lb, hipStreamSynchronize(s));
    for (int k = 0; k < 3; ++k) {
        float f = 0.f;
        if (hipEventElapsedTime(&f, lb->ev[k], lb->ev[k + 1]) == hipSuccess) lb->rms[k] = f;
    }
    std::string gmsg;
    if ((rc = arena_check(lb->mem, &gmsg)) != UMX_OK) return lfail(lb, rc, "%s", gmsg.c_str());
    if (resident) {                                       // the two tables change places; the host copy follows
        std::swap(lb->d_table, lb->d_rtable);
        std::swap(lb->table_cap, lb->rtable_cap);
        lb->table.swap(fresh);
        lb->res_N = n_new;
        lb->res_why = nullptr;
    }
    return UMX_OK;
}

// the map of a call on the host: UMX_OK with map (N + 1 words) and *n_new, or the refusal
int relabel_host_map(umx_labeler* lb, long long N, const uint8_t* keep, const int32_t* pairs, long long M, std::vector<int32_t>* map, long long* n_new) {
    try {
        map->resize((size_t)N + 1);
    } catch (const std::bad_alloc&) {
        return lfail(lb, UMX_ERR_OOM, "no host memory for a map of %lld labels", N);
    }
    char msg[240] = "";
    if (relabel_map(N, keep, pairs, M, map->data(), n_new, msg, sizeof msg) != UMX_OK) return lfail(lb, UMX_ERR_INVALID, "%s", msg);
    return UMX_OK;
}

}  // namespace

}  // namespace umx

using namespace umx;

extern "C" {

int umx_label_relabel_check(int H, int W, int64_t n_objects, int64_t n_pairs, char* msg, size_t cap) {
    char buf[240] = "";
    relabel_check_message(H, W, (long long)n_objects, (long long)n_pairs, buf, sizeof buf);
    if (msg && cap) snprintf(msg, cap, "%s", buf);
    return buf[0] ? UMX_ERR_INVALID : UMX_OK;
}

int umx_label_relabel_map(int64_t n_objects, const uint8_t* keep, const int32_t* pairs, int64_t n_pairs, int32_t* map, int64_t* n_new, char* msg,
                          size_t cap) {
    char buf[240] = "";
    long long n = 0;
    const int rc = relabel_map((long long)n_objects, keep, pairs, (long long)n_pairs, map, &n, buf, sizeof buf);
    if (msg && cap) snprintf(msg, cap, "%s", buf);
    if (rc == UMX_OK && map && n_new) *n_new = n;
    return rc;
}

int umx_labeler_relabel(umx_labeler* lb, int H, int W, const uint8_t* keep, int64_t n_keep, const int32_t* pairs, int64_t n_pairs,
                        int32_t* labels_host, int32_t* map_host, int64_t* n_new) {
    if (!lb) return lfail(nullptr, UMX_ERR_INVALID, "null labeler");
    char msg[240];
    if (umx_label_relabel_check(H, W, 0, n_pairs, msg, sizeof msg) != UMX_OK) return lfail(lb, UMX_ERR_INVALID, "%s", msg);
    if (lb->res_why) return lfail(lb, UMX_ERR_INVALID, "umx_labeler_relabel has no labels to work on: %s", lb->res_why);
    if (H != lb->res_H || W != lb->res_W)
        return lfail(lb, UMX_ERR_INVALID, "the call names %d x %d and the labels of the last run are %d x %d", H, W, lb->res_H, lb->res_W);
    const long long N = lb->res_N;
    if (keep ? (long long)n_keep != N : n_keep != 0)
        return lfail(lb, UMX_ERR_INVALID, "keep is %s and n_keep is %lld: the resident labels have %lld objects (keep null goes with n_keep 0)",
                     keep ? "set" : "null", (long long)n_keep, N);
    std::vector<int32_t> map;
    long long n = 0;
    int rc = relabel_host_map(lb, N, keep, pairs, (long long)n_pairs, &map, &n);
    if (rc) return rc;
    if ((rc = relabel_launches(lb, lb->d_P, lb->d_P, N, H, W, map.data(), n, true, labels_host))) return rc;
    if (map_host) memcpy(map_host, map.data(), map.size() * sizeof(int32_t));
    if (n_new) *n_new = n;
    return UMX_OK;
}

int umx_labeler_relabel_dev(umx_labeler* lb, const int32_t* labels_dev, int64_t n_objects, int H, int W, const uint8_t* keep, const int32_t* pairs,
                            int64_t n_pairs, int32_t* labels_out_dev, int32_t* map_host, int64_t* n_new) {
    if (!lb) return lfail(nullptr, UMX_ERR_INVALID, "null labeler");
    char msg[240];
    if (umx_label_relabel_check(H, W, n_objects, n_pairs, msg, sizeof msg) != UMX_OK) return lfail(lb, UMX_ERR_INVALID, "%s", msg);
    if (!labels_dev || !labels_out_dev) return lfail(lb, UMX_ERR_INVALID, "null labels");
    std::vector<int32_t> map;
    long long n = 0;
    int rc = relabel_host_map(lb, (long long)n_objects, keep, pairs, (long long)n_pairs, &map, &n);
    if (rc) return rc;
    if ((rc = relabel_launches(lb, labels_dev, labels_out_dev, (long long)n_objects, H, W, map.data(), n, false, nullptr))) return rc;
    if (map_host) memcpy(map_host, map.data(), map.size() * sizeof(int32_t));
    if (n_new) *n_new = n;
    return UMX_OK;
}

int umx_labeler_relabel_last_ms(const umx_labeler* lb, double* upload_ms, double* kernel_ms, double* download_ms) {
    if (!lb) return lfail(nullptr, UMX_ERR_INVALID, "null labeler");
    if (upload_ms) *upload_ms = lb->rms[0];
    if (kernel_ms) *kernel_ms = lb->rms[1];
    if (download_ms) *download_ms = lb->rms[2];
    return UMX_OK;
}

}  // extern "C"
