// libumx label mask, hulls: the convex hull of every labelled object -- the kernels and the C ABI behind umx_labeler_hull / _hull_dev
// (include/umx.h).  One call is this sequence of launches on the labeler's stream, from a label
// plane that is only read:
//
//   (ymin is set to "none", ymax to -1, the words the host reads to 0)
//   hull_rowrange_kernel     one wave per row: per run of a label an atomicMin of y into ymin[label - 1] and an atomicMax into ymax
//   hull_blocksum_kernel     per block of 2048 labels the sum of their heights ymax - ymin + 1 (0 for a label no pixel carries), 64 bits
//   hull_scan_kernel         ONE workgroup: the block sums to their exclusive prefix sums, the total E to the host's word
//   hull_offsets_kernel      per block again: offset[label - 1] = the heights of all labels below it
//   (E comes back to the host: the first synchronisation.  Above UMX_HULL_MAX_ROWS the call ends here; else the row entries and the
//   scratch vertices are allocated, the least x of every entry set to "none" and the largest x + 1 to 0)
//   hull_extremes_kernel     one wave per row again: per run an atomicMin of its first x and an atomicMax of its last x + 1 at entry
//                            offset[label - 1] + y - ymin[label - 1]
//   hull_wrap_kernel         one wave per object: the gift wrap below; the vertices into the object's scratch places, the record
//   hull_blocksum_kernel, hull_scan_kernel, hull_offsets_kernel   the same prefix sum over n_vertices, into the records' `first`
//   (V comes back to the host: the second synchronisation)
//   hull_compact_kernel      one wave per object: its scratch vertices to first .. first + n_vertices of the list
//
// The hull of one object.  Its box has h rows and so h + 1 corner levels; level k lies at y = ymin + k between rows k - 1 and k.  The
// only points of the object's squares that can be hull vertices are, per level, the leftmost and the rightmost corner: the lesser of
// the least x of the two rows that meet at the level, and the greater of their largest x + 1 (a row of the box in which the label has
// no pixel keeps "none" and gives nothing; a level between two such rows has no candidate).  They are ordered by y as they lie, so
// there is no sort.  The list starts at the left candidate of level 0, goes to the right candidate of level 0 (the top edge), down
// the right chain to level h, to the left candidate of level h (the bottom edge) and up the left chain back to level 0.  On a chain
// the next vertex after P is the candidate Q beyond it for which (x_Q - x_P) / |y_Q - y_P| is largest to the chain's own side, the
// farthest one among equals, so that collinear points are passed over: two candidates are compared by the cross product of their
// differences to P, formed in 64 bits (each factor <= 2^16), every lane keeps the best of the levels it looks at (level by level in
// chunks of 64) and six xor-shuffles leave the wave's best in every lane.  The order used is total on distinct candidates, so every
// lane ends with the same one, whatever the order of the comparisons.  One step costs ceil(levels beyond P / 64) rounds; an object of
// h rows with v vertices costs about v * ceil(h / 128) rounds: one or two dozen for a nucleus, 408 * 16 for a disc of radius 1000,
// quadratic (2^15 * 2^8 rounds) for a staircase across a whole slide.  The largest squared distance is then taken over all vertex
// pairs, 64 a round.
//
// Why no thread waits for another one: no kernel reads a word that an atomic of its own launch writes; a wave of the wrap reads the
// vertices its own lane 0 wrote, behind a workgroup fence, and nothing of another wave's.  Why the result does not depend on any
// order: minima, maxima and integer sums are order-free, and the wrap of an object is a function of its row entries alone.
#include "../../include/umx.h"
#include "umx_hull_host.h"
#include "umx_internal.h"
#include "umx_label_state.h"

#include <climits>

namespace umx {

namespace {

constexpr int kRowWaves = 4;                             // rows of the image (objects of the table) per workgroup
constexpr int kPixThreads = 256;                         // one thread per 8 labels
constexpr int kScanBlock = UMX_LABEL_SCAN_BLOCK;
constexpr int kPerThread = kScanBlock / kPixThreads;     // labels per thread of the two per-label kernels
constexpr int kScanThreads = 1024;                       // of the one-workgroup scan
constexpr int kWordE = 0, kWordV = 1, kWords = 2;        // the 64-bit words the host reads
constexpr int kNoX = 0x7f7f7f7f;                         // "none" as hipMemset of 0x7f leaves it: above any coordinate (<= 2^16)
static_assert(kPerThread * kPixThreads == kScanBlock, "a block of labels is a whole number per thread");
static_assert(sizeof(umx_label_hull) == 32 && sizeof(umx_label_hull_vertex) == 8, "the hull records");
static_assert(UMX_HULL_MAX_SIDE == 65536, "a coordinate is at most 2^16: cross products of differences stay below 2^33");

// The runs of one row by one wave (for_each_run of umx_label.hip): key_at(x) once for every pixel of the row (>= 0: the pixel's
// object; < 0: none), flush(key, start, len) once for every maximal segment [start, start + len) of equal key >= 0, by one lane.  A
// segment that reaches the end of a 64-pixel chunk is carried into the next one.  ceil(W / 64) rounds; start + len <= W.
template <typename KeyAt, typename Flush>
__device__ inline void runs_of_row(int W, int lane, KeyAt key_at, Flush flush) {
    int ckey = -1, cstart = 0, clen = 0;                  // the carried segment; ckey < 0: none
    const int nchunks = (W - 1) / 64 + 1;
    for (int c = 0; c < nchunks; ++c) {
        const int x0 = c * 64;
        const bool in = lane < W - x0;
        const int x = in ? x0 + lane : x0;
        const int t = in ? key_at(x) : -2;                // past the row's end: a key no pixel has
        const int tl = __shfl_up(t, 1);
        const bool head = lane == 0 || t != tl;
        const unsigned long long heads = __ballot(head);  // (bit 0 is always set)
        const unsigned long long later = lane == 63 ? 0ull : heads >> (lane + 1);
        int len = later ? __ffsll((long long)later) : 64 - lane;   // pixels up to the next head, or to the chunk's end
        int start = x;
        const int t0 = __shfl(t, 0);
        if (lane == 0 && ckey >= 0) {
            if (t0 == ckey) { start = cstart; len += clen; }
            else flush(ckey, cstart, clen);
        }
        const bool last = c + 1 == nchunks;
        if (head && t >= 0 && (later || last)) flush(t, start, len);
        const int hl = 63 - __clzll((long long)heads);    // the head of the chunk's last segment
        const int lk = __shfl(t, hl), ls = __shfl(start, hl), ll = __shfl(len, hl);
        if (!last && lk >= 0) { ckey = lk; cstart = ls; clen = ll; }
        else ckey = -1;
    }
}

// grid ceil(H / 4).  labels [H][W] is only read (row y < H by its wave; a pixel word is y * W + x < H * W <= INT_MAX); a value outside
// 1..N forms no run, so the words addressed are ymin / ymax [0 .. N).  Both take integer atomics that nothing reads in this launch.
__global__ void __launch_bounds__(64 * kRowWaves) hull_rowrange_kernel(const int* __restrict__ labels, int H, int W, int N, int* __restrict__ ymin,
                                                                       int* __restrict__ ymax) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if ((long long)blockIdx.x * kRowWaves + wave >= H) return;    // (the whole wave: no barrier below)
    const int y = blockIdx.x * kRowWaves + wave;
    const int* row = labels + (size_t)y * W;
    runs_of_row(
        W, lane, [&](int x) { const int v = row[x]; return v >= 1 && v <= N ? v - 1 : -1; },
        [&](int key, int, int) {
            atomicMin(ymin + key, y);
            atomicMax(ymax + key, y);
        });
}

// what the two prefix sums add up, label by label (i < N), and where their results go
struct HeightOf {
    const int* ymin;
    const int* ymax;
    __device__ int operator()(long long i) const {
        const int lo = ymin[i], hi = ymax[i];
        return hi >= lo ? hi - lo + 1 : 0;                // (a label no pixel carries: ymin "none", ymax -1)
    }
};
struct CountOf {
    const umx_label_hull* rec;
    __device__ int operator()(long long i) const { return rec[i].n_vertices; }
};
struct ToOffsets {
    long long* off;
    __device__ void operator()(long long i, long long v) const { off[i] = v; }
};
struct ToFirst {
    umx_label_hull* rec;
    __device__ void operator()(long long i, long long v) const { rec[i].first = v; }
};

// grid ceil(N / 2048), 256 threads of 8 labels.  bsum[block] by thread 0.  A sum of heights is <= N * H < 2^47.
template <typename Value>
__global__ void __launch_bounds__(kPixThreads) hull_blocksum_kernel(Value value, long long N, long long* __restrict__ bsum) {
    __shared__ long long wsum[kPixThreads / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long base = (long long)blockIdx.x * kScanBlock + (long long)threadIdx.x * kPerThread;
    long long sum = 0;
    for (int j = 0; j < kPerThread; ++j)
        if (base + j < N) sum += value(base + j);
    for (int d = 32; d > 0; d >>= 1) sum += __shfl_down(sum, d);
    if (lane == 0) wsum[wave] = sum;
    __syncthreads();
    if (threadIdx.x == 0) {
        long long s = 0;
        for (int k = 0; k < kPixThreads / 64; ++k) s += wsum[k];
        bsum[blockIdx.x] = s;
    }
}

// ONE workgroup.  sums[0 .. nblocks) -> their exclusive prefix sums, in place (a thread reads and writes its own element of a round);
// *total = the sum.  ceil(nblocks / 1024) rounds, nblocks <= 2^20.  (label_scan_kernel of umx_label.hip in 64 bits: N * 65536 passes
// 2^31 long before the limit on E is checked.)
__global__ void __launch_bounds__(kScanThreads) hull_scan_kernel(long long* __restrict__ sums, int nblocks, long long* __restrict__ total) {
    __shared__ long long wsum[kScanThreads / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    long long carry = 0;
    for (int base = 0; base < nblocks; base += kScanThreads) {
        const int idx = base + threadIdx.x;
        const long long v = idx < nblocks ? sums[idx] : 0;
        long long s = v;
        for (int d = 1; d < 64; d <<= 1) {
            const long long t = __shfl_up(s, d);
            if (lane >= d) s += t;
        }
        if (lane == 63) wsum[wave] = s;
        __syncthreads();
        long long before = 0, all = 0;
        for (int k = 0; k < kScanThreads / 64; ++k) {
            if (k < wave) before += wsum[k];
            all += wsum[k];
        }
        if (idx < nblocks) sums[idx] = carry + before + s - v;
        carry += all;
        __syncthreads();
    }
    if (threadIdx.x == 0) *total = carry;
}

// grid ceil(N / 2048), 256 threads of 8 consecutive labels.  bsum: the exclusive prefix sums of the blocks, only read.  The result
// of label i goes to the place `store` gives it, by the thread of label i alone.
template <typename Value, typename Store>
__global__ void __launch_bounds__(kPixThreads) hull_offsets_kernel(Value value, long long N, const long long* __restrict__ bsum, Store store) {
    __shared__ long long wsum[kPixThreads / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long base = (long long)blockIdx.x * kScanBlock + (long long)threadIdx.x * kPerThread;
    int v[kPerThread];
    long long mine = 0;
#pragma unroll
    for (int j = 0; j < kPerThread; ++j) {
        v[j] = base + j < N ? value(base + j) : 0;
        mine += v[j];
    }
    long long s = mine;                                   // inclusive over the wave's threads
    for (int d = 1; d < 64; d <<= 1) {
        const long long u = __shfl_up(s, d);
        if (lane >= d) s += u;
    }
    if (lane == 63) wsum[wave] = s;
    __syncthreads();
    long long off = bsum[blockIdx.x] + s - mine;
    for (int k = 0; k < wave; ++k) off += wsum[k];
#pragma unroll
    for (int j = 0; j < kPerThread; ++j) {
        if (base + j < N) store(base + j, off);
        off += v[j];
    }
}

// grid ceil(H / 4).  labels as in hull_rowrange_kernel; ymin, ymax and off are only read.  A run of label j in row y addresses entry
// off[j - 1] + y - ymin[j - 1], which is below off[j - 1] + height <= E while ymin <= y <= ymax -- as the first pass left it; a row
// outside that range (the labels changed between the passes) and an entry outside 0 .. E are skipped, not written.
__global__ void __launch_bounds__(64 * kRowWaves) hull_extremes_kernel(const int* __restrict__ labels, int H, int W, int N, const int* __restrict__ ymin,
                                                                       const int* __restrict__ ymax, const long long* __restrict__ off, long long E,
                                                                       int* __restrict__ xmin, int* __restrict__ xmax) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if ((long long)blockIdx.x * kRowWaves + wave >= H) return;    // (the whole wave: no barrier below)
    const int y = blockIdx.x * kRowWaves + wave;
    const int* row = labels + (size_t)y * W;
    runs_of_row(
        W, lane, [&](int x) { const int v = row[x]; return v >= 1 && v <= N ? v - 1 : -1; },
        [&](int key, int start, int len) {
            const int lo = ymin[key];
            if (y < lo || y > ymax[key]) return;
            const long long e = off[key] + (y - lo);
            if (e < 0 || e >= E) return;
            atomicMin(xmin + e, start);
            atomicMax(xmax + e, start + len);
        });
}

// a candidate as its difference to the current vertex: dx to the chain's own side, dy > 0 levels beyond it; dy == 0: none
struct Step {
    int dx, dy;
};
__device__ inline bool better(Step a, Step b) {
    if (a.dy == 0) return false;
    if (b.dy == 0) return true;
    const long long l = (long long)a.dx * b.dy, r = (long long)b.dx * a.dy;   // (|dx|, dy <= 2^16)
    return l > r || (l == r && a.dy > b.dy);
}
__device__ inline Step wave_best(Step s) {
    for (int d = 32; d > 0; d >>= 1) {
        Step o;
        o.dx = __shfl_xor(s.dx, d);
        o.dy = __shfl_xor(s.dy, d);
        if (better(o, s)) s = o;
    }
    return s;
}

// grid ceil(N / 4), one wave per label j = object + 1.  ymin, ymax, off, xmin and xmax are only read: xmin / xmax at entries off[object]
// + 0 .. h - 1, which is inside 0 .. E (checked).  The vertices go to scratch[2 * (off[object] + object) + 0 .. 2 * h + 2), the places of
// this object alone, written by lane 0 and read back by the wave behind a fence; at most 2 * h + 2 of them (counted).  rec[object] by
// lane 0.  A chain step that finds no candidate ends the chain (it cannot with entries the passes before left; a walk never loops).
__global__ void __launch_bounds__(64 * kRowWaves) hull_wrap_kernel(const int* __restrict__ ymin, const int* __restrict__ ymax,
                                                                   const long long* __restrict__ off, const int* __restrict__ xmin,
                                                                   const int* __restrict__ xmax, long long N, long long E,
                                                                   umx_label_hull* __restrict__ rec, umx_label_hull_vertex* scratch) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long object = (long long)blockIdx.x * kRowWaves + wave;
    if (object >= N) return;                              // (the whole wave: no barrier below)
    const int lo = ymin[object], hi = ymax[object];
    const long long e0 = off[object];
    umx_label_hull r;
    r.area2 = 0; r.feret_max_sq = 0; r.first = 0; r.n_vertices = 0; r.rows = 0;
    if (hi < lo || e0 < 0 || e0 + (hi - lo + 1) > E) {    // no pixel carries the label
        if (lane == 0) rec[object] = r;
        return;
    }
    const int h = hi - lo + 1;
    const int* xl = xmin + e0;
    const int* xr = xmax + e0;
    umx_label_hull_vertex* out = scratch + 2 * (e0 + object);
    const int room = 2 * h + 2;
    // the candidates of level k, 0 <= k <= h: rows k - 1 and k of the box meet there
    auto left = [&](int k) {
        const int a = k > 0 ? xl[k - 1] : kNoX, b = k < h ? xl[k] : kNoX;
        return a < b ? a : b;                             // kNoX: none
    };
    auto right = [&](int k) {
        const int a = k > 0 ? xr[k - 1] : 0, b = k < h ? xr[k] : 0;
        return a > b ? a : b;                             // 0: none
    };
    int rows = 0;
    for (int k0 = 0; k0 < h; k0 += 64) rows += __popcll(__ballot(k0 + lane < h && xl[k0 + lane] != kNoX));

    int n = 0;
    long long area2 = 0;
    int py = 0, px = 0;                                   // the vertex before (wave-uniform, as everything below but the searches)
    auto emit = [&](int y, int x) {
        if (n > 0) area2 += (long long)px * y - (long long)x * py;
        if (n < room && lane == 0) { out[n].y = y; out[n].x = x; }
        if (n < room) ++n;
        py = y; px = x;
    };
    const int y0 = lo, x0 = xl[0];
    emit(y0, x0);
    int k = 0, xk = xr[0];
    emit(lo, xk);
    while (k < h) {                                       // down the right chain: the candidate farthest right per level
        Step best = {0, 0};
        for (int m = k + 1 + lane; m <= h; m += 64) {
            const int x = right(m);
            const Step s = {x - xk, m - k};
            if (x > 0 && better(s, best)) best = s;
        }
        best = wave_best(best);
        if (best.dy == 0) break;
        k += best.dy; xk += best.dx;
        emit(lo + k, xk);
    }
    k = h; xk = left(h);
    emit(lo + h, xk);
    while (k > 0) {                                       // up the left chain: the candidate farthest left per level
        Step best = {0, 0};
        for (int m = k - 1 - lane; m >= 0; m -= 64) {
            const int x = left(m);
            const Step s = {xk - x, k - m};
            if (x != kNoX && better(s, best)) best = s;
        }
        best = wave_best(best);
        if (best.dy == 0) break;
        k -= best.dy; xk -= best.dx;
        if (k > 0) emit(lo + k, xk);                      // (level 0 is the first vertex again)
    }
    area2 += (long long)px * y0 - (long long)x0 * py;     // the edge that closes the polygon

    __threadfence_block();                                // lane 0's vertices, for every lane of this wave
    long long far = 0;
    for (int i = 0; i + 1 < n; ++i) {
        const umx_label_hull_vertex a = out[i];
        for (int q = i + 1 + lane; q < n; q += 64) {
            const umx_label_hull_vertex b = out[q];
            const long long dy = b.y - a.y, dx = b.x - a.x;
            const long long d2 = dy * dy + dx * dx;       // (<= 2^33)
            far = d2 > far ? d2 : far;
        }
    }
    for (int d = 32; d > 0; d >>= 1) {
        const long long o = __shfl_xor(far, d);
        far = o > far ? o : far;
    }
    r.area2 = area2; r.feret_max_sq = far; r.n_vertices = n; r.rows = rows;
    if (lane == 0) rec[object] = r;
}

// grid ceil(N / 4), one wave per object.  rec and off are only read; scratch as hull_wrap_kernel left it.  verts[first .. first + n) of
// this object alone, inside 0 .. V (checked).
__global__ void __launch_bounds__(64 * kRowWaves) hull_compact_kernel(const umx_label_hull* __restrict__ rec, const long long* __restrict__ off,
                                                                      const umx_label_hull_vertex* __restrict__ scratch, long long N, long long V,
                                                                      umx_label_hull_vertex* __restrict__ verts) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long object = (long long)blockIdx.x * kRowWaves + wave;
    if (object >= N) return;
    const int n = rec[object].n_vertices;
    const long long first = rec[object].first;
    if (n <= 0 || first < 0 || first + n > V) return;
    const umx_label_hull_vertex* src = scratch + 2 * (off[object] + object);
    for (int i = lane; i < n; i += 64) verts[first + i] = src[i];
}

inline unsigned row_grid(long long rows) { return (unsigned)((rows - 1) / kRowWaves + 1); }

// The hulls of `labels` (device, H x W, objects 1..N >= 1).  The caller has checked the arguments: out (null: only V is wanted, and
// then verts is null too) holds N records, verts (may be null) vcap vertices.  Returns with the stream idle.
int hull_any(umx_labeler* lb, const int* labels, long long N, int H, int W, umx_label_hull* out, umx_label_hull_vertex* verts, long long vcap,
             int64_t* v_out) {
    L_HIP(lb, hipSetDevice(lb->device));
    lb->hms[0] = lb->hms[1] = 0.0;
    if (v_out) *v_out = 0;
    if (N == 0) return UMX_OK;
    hipStream_t s = lb->stream;
    const size_t nblocks = hull_label_blocks(N, kScanBlock);
    int rc = ensure_measure_buffer(lb, &lb->d_hrange, &lb->hrange_cap, 2 * (size_t)N, sizeof(int), "hull row ranges");
    if (rc) return rc;
    if ((rc = ensure_measure_buffer(lb, &lb->d_hoff, &lb->hoff_cap, hull_offset_words(N, kScanBlock, kWords), sizeof(long long), "hull offsets")))
        return rc;
    int* const ymin = lb->d_hrange;
    int* const ymax = ymin + N;
    long long* const off = lb->d_hoff;
    long long* const bsum = off + N;
    long long* const words = bsum + nblocks;
    const dim3 label_grid((unsigned)nblocks), object_grid(row_grid(N));
    L_HIP(lb, hipEventRecord(lb->ev[1], s));
    L_HIP(lb, hipMemsetAsync(ymin, 0x7f, (size_t)N * sizeof(int), s));
    L_HIP(lb, hipMemsetAsync(ymax, 0xff, (size_t)N * sizeof(int), s));
    L_HIP(lb, hipMemsetAsync(words, 0, kWords * sizeof(long long), s));
    const HeightOf height{ymin, ymax};
    hipLaunchKernelGGL(hull_rowrange_kernel, dim3(row_grid(H)), dim3(64 * kRowWaves), 0, s, labels, H, W, (int)N, ymin, ymax);
    hipLaunchKernelGGL(hull_blocksum_kernel<HeightOf>, label_grid, dim3(kPixThreads), 0, s, height, N, bsum);
    hipLaunchKernelGGL(hull_scan_kernel, dim3(1), dim3(kScanThreads), 0, s, bsum, (int)nblocks, words + kWordE);
    hipLaunchKernelGGL((hull_offsets_kernel<HeightOf, ToOffsets>), label_grid, dim3(kPixThreads), 0, s, height, N, bsum, ToOffsets{off});
    L_HIP(lb, hipGetLastError());
    long long E = 0, V = 0;
    L_HIP(lb, hipMemcpyAsync(&E, words + kWordE, sizeof E, hipMemcpyDeviceToHost, s));
    L_HIP(lb, hipStreamSynchronize(s));
    char msg[240];
    hull_rows_message(E, N, H, msg, sizeof msg);
    if (msg[0]) return lfail(lb, E >= 0 && E <= N * (long long)H ? UMX_ERR_OOM : UMX_ERR_HIP, "%s", msg);
    if ((rc = ensure_measure_buffer(lb, &lb->d_hrows, &lb->hrows_cap, hull_row_words(E), sizeof(int), "hull row entries"))) return rc;
    if ((rc = ensure_measure_buffer(lb, &lb->d_hscratch, &lb->hscratch_cap, hull_scratch_vertices(E, N), sizeof(umx_label_hull_vertex),
                                    "hull scratch vertices")))
        return rc;
    if ((rc = ensure_measure_buffer(lb, &lb->d_hrec, &lb->hrec_cap, (size_t)N, sizeof(umx_label_hull), "hull records"))) return rc;
    int* const xmin = lb->d_hrows;
    int* const xmax = xmin + E;
    if (E > 0) {
        L_HIP(lb, hipMemsetAsync(xmin, 0x7f, (size_t)E * sizeof(int), s));
        L_HIP(lb, hipMemsetAsync(xmax, 0, (size_t)E * sizeof(int), s));
        hipLaunchKernelGGL(hull_extremes_kernel, dim3(row_grid(H)), dim3(64 * kRowWaves), 0, s, labels, H, W, (int)N, ymin, ymax, off, E, xmin, xmax);
    }
    const CountOf count{lb->d_hrec};
    hipLaunchKernelGGL(hull_wrap_kernel, object_grid, dim3(64 * kRowWaves), 0, s, ymin, ymax, off, xmin, xmax, N, E, lb->d_hrec, lb->d_hscratch);
    hipLaunchKernelGGL(hull_blocksum_kernel<CountOf>, label_grid, dim3(kPixThreads), 0, s, count, N, bsum);
    hipLaunchKernelGGL(hull_scan_kernel, dim3(1), dim3(kScanThreads), 0, s, bsum, (int)nblocks, words + kWordV);
    hipLaunchKernelGGL((hull_offsets_kernel<CountOf, ToFirst>), label_grid, dim3(kPixThreads), 0, s, count, N, bsum, ToFirst{lb->d_hrec});
    L_HIP(lb, hipGetLastError());
    L_HIP(lb, hipMemcpyAsync(&V, words + kWordV, sizeof V, hipMemcpyDeviceToHost, s));
    L_HIP(lb, hipStreamSynchronize(s));
    if (V < 0 || (size_t)V > hull_scratch_vertices(E, N))
        return lfail(lb, UMX_ERR_HIP, "the hull pass counted %lld vertices for %lld box rows of %lld labels", V, E, N);
    if (v_out) *v_out = V;
    const bool refused = out && V > 0 && (!verts || vcap < V);
    if (out && !refused) {
        if (V > 0) {
            if ((rc = ensure_measure_buffer(lb, &lb->d_hverts, &lb->hverts_cap, (size_t)V, sizeof(umx_label_hull_vertex), "hull vertices"))) return rc;
            hipLaunchKernelGGL(hull_compact_kernel, object_grid, dim3(64 * kRowWaves), 0, s, lb->d_hrec, off, lb->d_hscratch, N, V, lb->d_hverts);
            L_HIP(lb, hipGetLastError());
        }
        L_HIP(lb, hipEventRecord(lb->ev[2], s));
        L_HIP(lb, hipMemcpyAsync(out, lb->d_hrec, (size_t)N * sizeof(umx_label_hull), hipMemcpyDeviceToHost, s));
        if (V > 0) L_HIP(lb, hipMemcpyAsync(verts, lb->d_hverts, (size_t)V * sizeof(umx_label_hull_vertex), hipMemcpyDeviceToHost, s));
    } else {
        L_HIP(lb, hipEventRecord(lb->ev[2], s));
    }
    L_HIP(lb, hipEventRecord(lb->ev[3], s));
    L_HIP(lb, hipStreamSynchronize(s));
    for (int k = 0; k < 2; ++k) {
        float f = 0.f;
        if (hipEventElapsedTime(&f, lb->ev[k + 1], lb->ev[k + 2]) == hipSuccess) lb->hms[k] = f;
    }
    std::string gmsg;
    if ((rc = arena_check(lb->mem, &gmsg)) != UMX_OK) return lfail(lb, rc, "%s", gmsg.c_str());
    if (refused)
        return lfail(lb, UMX_ERR_INVALID, "verts holds %lld vertices: the hulls have %lld", verts ? vcap : 0ll, V);
    return UMX_OK;
}

// the buffers of a call: UMX_OK and *count_only, or the refusal
int hull_buffers_check(umx_labeler* lb, const void* out, long long cap, const void* verts, long long vcap, long long N, bool* count_only) {
    if (cap < 0 || (!out && cap > 0)) return lfail(lb, UMX_ERR_INVALID, "out is %s and holds %lld records", out ? "set" : "null", cap);
    if (vcap < 0 || (!verts && vcap > 0)) return lfail(lb, UMX_ERR_INVALID, "verts is %s and holds %lld vertices", verts ? "set" : "null", vcap);
    *count_only = !out && !verts;
    if (*count_only) return UMX_OK;
    if (cap < N || (!out && N > 0)) return lfail(lb, UMX_ERR_INVALID, "out holds %lld records: %lld objects need as many", out ? cap : 0ll, N);
    return UMX_OK;
}

}  // namespace

}  // namespace umx

using namespace umx;

extern "C" {

int umx_label_hull_check(int H, int W, int64_t n_objects, char* msg, size_t cap) {
    char buf[240] = "";
    hull_check_message(H, W, (long long)n_objects, buf, sizeof buf);
    if (msg && cap) snprintf(msg, cap, "%s", buf);
    return buf[0] ? UMX_ERR_INVALID : UMX_OK;
}

int umx_labeler_hull(umx_labeler* lb, int H, int W, umx_label_hull* out, int64_t cap, int64_t* n, umx_label_hull_vertex* verts, int64_t vcap,
                     int64_t* v) {
    if (!lb) return lfail(nullptr, UMX_ERR_INVALID, "null labeler");
    char msg[240];
    if (umx_label_hull_check(H, W, 0, msg, sizeof msg) != UMX_OK) return lfail(lb, UMX_ERR_INVALID, "%s", msg);
    if (lb->res_why) return lfail(lb, UMX_ERR_INVALID, "umx_labeler_hull has no labels to take the hulls of: %s", lb->res_why);
    if (H != lb->res_H || W != lb->res_W)
        return lfail(lb, UMX_ERR_INVALID, "the call names %d x %d and the labels of the last run are %d x %d", H, W, lb->res_H, lb->res_W);
    const long long N = lb->res_N;
    if (n) *n = N;
    bool count_only = false;
    const int rc = hull_buffers_check(lb, out, (long long)cap, verts, (long long)vcap, N, &count_only);
    if (rc) return rc;
    return hull_any(lb, lb->d_P, N, H, W, count_only ? nullptr : out, count_only ? nullptr : verts, (long long)vcap, v);
}

int umx_labeler_hull_dev(umx_labeler* lb, const int32_t* labels_dev, int64_t n_objects, int H, int W, umx_label_hull* out_host, int64_t cap,
                         umx_label_hull_vertex* verts_host, int64_t vcap, int64_t* v) {
    if (!lb) return lfail(nullptr, UMX_ERR_INVALID, "null labeler");
    char msg[240];
    if (umx_label_hull_check(H, W, n_objects, msg, sizeof msg) != UMX_OK) return lfail(lb, UMX_ERR_INVALID, "%s", msg);
    if (!labels_dev) return lfail(lb, UMX_ERR_INVALID, "null labels");
    bool count_only = false;
    const int rc = hull_buffers_check(lb, out_host, (long long)cap, verts_host, (long long)vcap, (long long)n_objects, &count_only);
    if (rc) return rc;
    return hull_any(lb, labels_dev, (long long)n_objects, H, W, count_only ? nullptr : out_host, count_only ? nullptr : verts_host, (long long)vcap, v);
}

int umx_labeler_hull_last_ms(const umx_labeler* lb, double* kernel_ms, double* download_ms) {
    if (!lb) return lfail(nullptr, UMX_ERR_INVALID, "null labeler");
    if (kernel_ms) *kernel_ms = lb->hms[0];
    if (download_ms) *download_ms = lb->hms[1];
    return UMX_OK;
}

}  // extern "C"
