// libumx label mask: whole-slide object labelling on the device -- the kernels and the C ABI behind umx_labeler_* (include/umx.h,
// DESIGN.md section 8.1 "Label mask").  Two int32 planes of H * W: P (parents, then roots, then the labels) and Q (roots of the run
// heads, then areas, then numbers).  A run is a maximal row segment of object pixels, its head the first pixel of it.  One call is this
// sequence of launches on the labeler's stream:
//
//   label_runs_kernel     one wave per row: the class rule (first maximum of the K planes == cls) and the row runs; every object pixel
//                         points at its run's head, every other pixel holds -1 (phase 0 of border_label_kernel)
//   label_strip_kernel    one workgroup per strip of UMX_LABEL_STRIP_ROWS rows: the vertical merges between the rows of the strip
//                         (phase 1 of border_label_kernel, the same pruning, atomicMin unions)
//   label_seam_kernel     level l = 0, 1, ...: groups of 2^(l+1) strips; one workgroup per group merges across the one seam in the
//                         group's middle, where its two halves -- each joined by the levels before -- meet
//   label_heads_kernel    one thread per pixel: the root of every run head into Q (P is only read)
//   label_flatten_kernel  one wave per row: every object pixel takes Q of its run's head into P: P = root, -1 off the objects
//   (Q is cleared)
//   label_area_kernel     one wave per row: every run adds its length to Q[root]
//   label_count_kernel    kept(i) = P[i] == i and Q[i] >= min_area; per block of UMX_LABEL_SCAN_BLOCK pixels the number of kept roots
//   label_scan_kernel     ONE workgroup: exclusive prefix sum of the block counts in place, the total N to a word the host reads
//   label_number_kernel   per block again: Q[root] = 1 + (kept roots before it in raster order), 0 at a root that is not kept
//   (N comes back to the host: the only synchronisation inside a call; the table is sized for it)
//   label_table_init_kernel, label_write_kernel   one wave per row: labels = Q[P], 0 off the objects, in place over P or into the
//                         caller's plane; every run adds its length, y * length, the sum of its x and its extent to record label - 1
// With a growth (grow_radius R > 0) the last launch is replaced by
//   label_seed_kernel     one thread per pixel: the seed labels Q[P] in place over P, no table; Q is free from here on
//   label_grow_kernel<false>  ceil(R / UMX_LABEL_GROW_HALO) launches, P -> Q -> P ...: one workgroup per tile of 64 x 64 pixels loads the
//                         tile and a halo of 8 into LDS, runs up to 8 synchronous levels there and writes its tile to the other plane
//   label_grown_kernel    one wave per row: the labels from the plane the last launch wrote to where the call wants them, and the table
// A split run (umx_labeler_run_split / _run_split_dev) uses a third int32 plane R and a byte
// plane B of flags; its sequence of launches stands at run_split_launches.  New in it are
//   label_erode_kernel    one workgroup per tile of 64 x 64: "belongs to a kept object" of the tile and a halo of 8 as one bit per
//                         pixel in LDS, up to 8 levels of erosion on the bit string, the flags of its tile into B
//   label_runs_mask_kernel, label_core_mark_kernel, label_split_ids_kernel   the eroded set's row runs into R; which objects hold a
//                         core; the seed components' ids in place over P, which the count / scan / number kernels then number
//   label_grow_kernel<true>   the growth kernel over the label class itself, counting the pixels it claims so that the host can stop
// A flood run (umx_labeler_run_flood / _run_flood_dev) is a split run with, in the regrow's place,
//   label_flood_kernel    the growth's tile and halo at one level t of a relief taken from the planes: up to 8 steps over the empty
//                         pixels of class cls with relief <= t; it counts its claims and reports the least relief that waits beside
//                         a label, from which the host picks the next level (run_flood_launches)
// An h-maxima run (umx_labeler_run_hmax / _run_hmax_dev) is a flood run whose set E comes from
// the kernels of umx_label_hmax.hip (a relief of the planes, two grey-scale reconstructions) instead of from label_erode_kernel.
// A measurement (umx_labeler_measure / _measure_dev) is, per group of up to 4 image planes,
//   label_measure_init_kernel, label_measure_kernel   one wave per row: the labels (the P plane a run left, or the caller's) read once
//                         for the group's planes; every row run adds its count, its sums of v and v * v and its extremes of every plane
//                         to record [plane][label - 1]
// The shapes (umx_labeler_shape / _shape_dev) are
//   label_shape_init_kernel, label_shape_kernel   one wave per row: the labels of the row and of the rows above and below it; every
//                         row run adds its moments (closed forms of its row and its two ends) and the counts of the 2x2 windows
//                         that its pixels own to record label - 1
// The contacts (umx_labeler_contacts / _contacts_dev) live in umx_label_contact.hip; the
// labeler's state, which both sources share, in umx_label_state.h.  From here they use
//   label_grow_kernel<false, true>   the growth kernel over "every pixel without a label", no class consulted (the reach, step 23)
//   label_scan_kernel     the one-workgroup scan of the numbering, for the prefix sums of the contacts per label
//
// Why no workgroup waits for another one, and none reads inside a kernel what another one writes in it: in the strip launch a workgroup
// touches only pixels of its strip -- a link made there joins two run heads of the strip, so a walk from a pixel of the strip stays in
// it.  By induction a tree that exists before level l lies inside one half-group of that level; the workgroup of a group walks and
// changes only trees of its own two halves, and the groups of a level are disjoint.  Every other kernel writes only its own pixel's
// word (or an atomic sum / min / max that nothing reads before the launch ends) and reads words that the launches before it
// finished.  The launch boundary is the only synchronisation: no spin, no flag, no look-back.
// Why the result does not depend on any order: links only decrease, so a component's root is its least flat index however the unions
// interleave; every accumulated value is an integer sum, minimum or maximum.
#include "../../include/umx.h"
#include "../../include/umx_train.h"
#include "umx_internal.h"
#include "umx_label_state.h"
#include "umx_unionfind.h"

#include <climits>
#include <cstdarg>
#include <cstdio>

namespace umx {

namespace {

constexpr int kRowWaves = 4;                             // rows of the image per workgroup of the one-wave-per-row kernels
constexpr int kStripRows = UMX_LABEL_STRIP_ROWS;
constexpr int kMergeThreads = UMX_LABEL_THREADS;
constexpr int kPixThreads = 256;                         // one thread per pixel
constexpr int kScanBlock = UMX_LABEL_SCAN_BLOCK;
constexpr int kScanWaves = 4;                            // a block of the scan: 4 waves x 8 chunks x 64 pixels
constexpr int kScanChunks = kScanBlock / (64 * kScanWaves);
static_assert(kScanChunks * 64 * kScanWaves == kScanBlock, "a scan block is a whole number of 64-pixel chunks per wave");
constexpr int kGrowTile = UMX_LABEL_GROW_TILE, kGrowHalo = UMX_LABEL_GROW_HALO;
constexpr int kGrowSide = kGrowTile + 2 * kGrowHalo;     // the region a growth workgroup holds in LDS: 80 x 80 int32 = 25 600 B
constexpr int kGrowPix = kGrowSide * kGrowSide;
constexpr int kGrowThreads = 256;
constexpr int kGrowPer = kGrowPix / kGrowThreads;        // region pixels per thread
static_assert(kGrowPer * kGrowThreads == kGrowPix && (kGrowTile * kGrowTile) % kGrowThreads == 0, "whole rounds over the region and the tile");
static_assert(kGrowHalo >= 1 && kGrowPix * sizeof(int) <= 32 * 1024, "five growth workgroups or more per CU by LDS");
static_assert(UMX_LABEL_MAX_MIN_AREA == UMX_OBJECT_MAX_MIN_AREA, "one bound on min_area");
static_assert(UMX_BORDER_CONNECTIVITY == 4, "the merges below join a pixel with the one above it and row runs: 4-connectivity");
static_assert(sizeof(umx_label_object) == 40, "the table's record");

// The row runs of one row by one wave: obj_at(x) is called once for every pixel of the row; every object pixel's word of P gets the
// flat index of its run's head, every other pixel's -1.  Bounds: ceil(W / 64) chunks; a lane is in the row iff lane < W - x0 (no
// x0 + lane is formed past the row's end, W may be 2^31 - 1); the word written is row + x < H * W <= INT_MAX, its value row + start
// likewise.
template <typename ObjAt>
__device__ inline void write_row_runs(int W, int lane, size_t row, int* __restrict__ P, ObjAt obj_at) {
    const int nchunks = (W - 1) / 64 + 1;
    int carry = -1;   // first column of the run that reaches the end of the previous chunk; -1: none
    for (int c = 0; c < nchunks; ++c) {
        const int x0 = c * 64;
        const bool in = lane < W - x0;
        const int x = in ? x0 + lane : x0;
        const bool obj = in && obj_at(x);
        const unsigned long long mask = __ballot(obj);
        if (in) {
            int v = -1;
            if (obj) {
                const unsigned long long gaps = ~mask & ((1ull << lane) - 1ull);   // pixels off the object left of this one
                const int start = gaps ? x0 + (64 - __clzll((long long)gaps)) : (carry >= 0 ? carry : x0);
                v = (int)(row + start);
            }
            P[row + x] = v;
        }
        if (mask >> 63) {
            const unsigned long long gaps = ~mask;
            carry = gaps ? x0 + (64 - __clzll((long long)gaps)) : (carry >= 0 ? carry : x0);
        } else {
            carry = -1;
        }
    }
}

// grid ceil(H / 4).  planes [K][H][W].  Bounds: row y < H; the rest is write_row_runs'.
__global__ void __launch_bounds__(64 * kRowWaves) label_runs_kernel(const uint8_t* __restrict__ planes, int K, int H, int W, int cls,
                                                                     int* __restrict__ P) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if ((long long)blockIdx.x * kRowWaves + wave >= H) return;    // (the whole wave: no barrier below)
    const int y = blockIdx.x * kRowWaves + wave;
    const size_t npix = (size_t)H * W, row = (size_t)y * W;
    write_row_runs(W, lane, row, P, [&](int x) {
        int arg = 0, best = planes[row + x];
        for (int k = 1; k < K; ++k) {
            const int v = planes[(size_t)k * npix + row + x];
            if (v > best) { best = v; arg = k; }      // first maximum, as object_planes_kernel
        }
        return arg == cls;
    });
}

// the merge of pixel i (row >= 1, column x) with the one above it, pruned as in border_label_kernel: skipped when the left neighbour
// and that one's upper neighbour are object pixels too -- then the left neighbour's merge connects the same two runs
__device__ inline void merge_up(int* P, int i, int x, int W) {
    if (parent_load(P + i) < 0 || parent_load(P + i - W) < 0) return;
    if (x > 0 && parent_load(P + i - 1) >= 0 && parent_load(P + i - 1 - W) >= 0) return;
    union_trees(P, i, i - W);
}

// grid ceil(H / 32).  Strip rows [y0, y1), y1 - y0 <= 32; the pixels of rows y0 + 1 .. y1 - 1 are merged upwards: n = (y1 - y0 - 1) * W
// of them, ceil(n / 1024) rounds; i = (y0 + 1) * W + j < y1 * W <= H * W.  Every word read or changed lies in rows [y0, y1).
__global__ void __launch_bounds__(kMergeThreads) label_strip_kernel(int* __restrict__ P, int H, int W) {
    const int y0 = blockIdx.x * kStripRows;
    const int rows = H - y0 > kStripRows ? kStripRows : H - y0;
    const long long n = (long long)(rows - 1) * W;
    const long long first = (long long)(y0 + 1) * W;
    for (long long j = threadIdx.x; j < n; j += kMergeThreads) merge_up(P, (int)(first + j), (int)(j % W), W);
}

// span = 32 * 2^level rows.  grid: the groups g whose seam row y = (2 g + 1) * span is < H (host).  ceil(W / 1024) rounds (a seam
// exists only when H > 32, so W < 2^26 and x + 1024 fits).  Words read or changed: rows [2 g span, min(H, (2 g + 2) span)).
__global__ void __launch_bounds__(kMergeThreads) label_seam_kernel(int* __restrict__ P, int H, int W, long long span) {
    const long long y = (2ll * blockIdx.x + 1ll) * span;
    if (y >= H) return;
    const long long first = y * W;
    for (int x = threadIdx.x; x < W; x += kMergeThreads) merge_up(P, (int)(first + x), x, W);
}

// one thread per pixel, i < npix.  P is not written in this launch; Q[i] only by the thread of pixel i.
__global__ void __launch_bounds__(kPixThreads) label_heads_kernel(const int* __restrict__ P, int* __restrict__ Q, long long npix, int W) {
    const long long i = (long long)blockIdx.x * kPixThreads + threadIdx.x;
    if (i >= npix) return;
    if (P[i] < 0 || (i % W > 0 && P[i - 1] >= 0)) return;
    Q[i] = find_root(P, (int)i);
}

// grid ceil(H / 4).  An object pixel that is not a head still holds its head's index (unions change heads only): it reads Q there; a
// head reads its own.  Which one a pixel is comes from the ballot and the bit carried over from the chunk before, not from memory:
// a thread reads P only at its own pixel, which is the only word it writes.
__global__ void __launch_bounds__(64 * kRowWaves) label_flatten_kernel(int* __restrict__ P, const int* __restrict__ Q, int H, int W) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if ((long long)blockIdx.x * kRowWaves + wave >= H) return;    // (the whole wave: no barrier below)
    const int y = blockIdx.x * kRowWaves + wave;
    const size_t row = (size_t)y * W;
    const int nchunks = (W - 1) / 64 + 1;
    unsigned left_of_chunk = 0;                           // the last pixel of the chunk before is an object pixel
    for (int c = 0; c < nchunks; ++c) {
        const int x0 = c * 64;
        const bool in = lane < W - x0;
        const int x = in ? x0 + lane : x0;
        const int p = in ? P[row + x] : -1;
        const unsigned long long mask = __ballot(p >= 0);
        const unsigned left = lane > 0 ? (unsigned)((mask >> (lane - 1)) & 1ull) : left_of_chunk;
        if (p >= 0) P[row + x] = Q[left ? (size_t)p : row + x];
        left_of_chunk = (unsigned)(mask >> 63);
    }
}

// The runs of one row by one wave: key_at(x) is called once for every pixel of the row (>= 0: the pixel's object; < 0: none), and
// flush(key, start, len) once for every maximal segment [start, start + len) of equal key >= 0 -- by one lane, the others idle.  A
// segment that reaches the end of a 64-pixel chunk is carried into the next one (the wave walks its chunks in order), so a long run
// costs one flush, not one per chunk.  ceil(W / 64) rounds; len <= W.
template <typename KeyAt, typename Flush>
__device__ inline void for_each_run(int W, int lane, KeyAt key_at, Flush flush) {
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

// grid ceil(H / 4).  P: roots (-1 off the objects), read only; Q (zero on entry): atomicAdd at the roots, read by nobody here.
__global__ void __launch_bounds__(64 * kRowWaves) label_area_kernel(const int* __restrict__ P, int* __restrict__ Q, int H, int W) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if ((long long)blockIdx.x * kRowWaves + wave >= H) return;    // (the whole wave: no barrier below)
    const int y = blockIdx.x * kRowWaves + wave;
    const int* row = P + (size_t)y * W;
    for_each_run(W, lane, [&](int x) { return row[x]; }, [&](int key, int, int len) { atomicAdd(Q + key, len); });
}

// Block b of the scan covers pixels [2048 b, 2048 b + 2048), wave w of it 512 consecutive ones in 8 chunks; a pixel >= npix is
// never read.  The kept roots of the wave's pixels, in every lane.
__device__ inline int wave_kept(const int* P, const int* Q, long long base, long long npix, int min_area, int lane) {
    int n = 0;
    for (int c = 0; c < kScanChunks; ++c) {
        const long long i = base + c * 64 + lane;
        const bool kept = i < npix && P[i] == (int)i && Q[i] >= min_area;
        n += __popcll(__ballot(kept));
    }
    return n;
}

// grid nblocks = ceil(npix / 2048).
__global__ void __launch_bounds__(64 * kScanWaves) label_count_kernel(const int* __restrict__ P, const int* __restrict__ Q, long long npix,
                                                                       int min_area, int* __restrict__ counts) {
    __shared__ int wn[kScanWaves];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int n = wave_kept(P, Q, (long long)blockIdx.x * kScanBlock + wave * (kScanBlock / kScanWaves), npix, min_area, lane);
    if (lane == 0) wn[wave] = n;
    __syncthreads();
    if (threadIdx.x == 0) {
        int s = 0;
        for (int k = 0; k < kScanWaves; ++k) s += wn[k];
        counts[blockIdx.x] = s;
    }
}

// ONE workgroup.  counts[0 .. nblocks) -> their exclusive prefix sums, in place (a thread reads and writes its own element of a
// round); *total = the sum (<= npix <= INT_MAX).  ceil(nblocks / 1024) rounds, nblocks <= 2^20.
__global__ void __launch_bounds__(kMergeThreads) label_scan_kernel(int* __restrict__ counts, int nblocks, long long* __restrict__ total) {
    __shared__ int wsum[kMergeThreads / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int carry = 0;
    for (int base = 0; base < nblocks; base += kMergeThreads) {
        const int idx = base + threadIdx.x;
        const int v = idx < nblocks ? counts[idx] : 0;
        int s = v;
        for (int d = 1; d < 64; d <<= 1) {
            const int t = __shfl_up(s, d);
            if (lane >= d) s += t;
        }
        if (lane == 63) wsum[wave] = s;
        __syncthreads();
        int before = 0, all = 0;
        for (int k = 0; k < kMergeThreads / 64; ++k) {
            if (k < wave) before += wsum[k];
            all += wsum[k];
        }
        if (idx < nblocks) counts[idx] = carry + before + s - v;
        carry += all;
        __syncthreads();
    }
    if (threadIdx.x == 0) *total = carry;
}

// grid nblocks.  counts: the exclusive prefix sums.  Q[i] is read (the area) and written (the number) by the thread of pixel i alone,
// and only at roots.
__global__ void __launch_bounds__(64 * kScanWaves) label_number_kernel(const int* __restrict__ P, int* __restrict__ Q, long long npix,
                                                                        int min_area, const int* __restrict__ counts) {
    __shared__ int wn[kScanWaves];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long base = (long long)blockIdx.x * kScanBlock + wave * (kScanBlock / kScanWaves);
    const int n = wave_kept(P, Q, base, npix, min_area, lane);
    if (lane == 0) wn[wave] = n;
    __syncthreads();
    int off = counts[blockIdx.x];
    for (int k = 0; k < wave; ++k) off += wn[k];
    for (int c = 0; c < kScanChunks; ++c) {
        const long long i = base + c * 64 + lane;
        const bool root = i < npix && P[i] == (int)i;
        const bool kept = root && Q[i] >= min_area;
        const unsigned long long mask = __ballot(kept);
        if (root) Q[i] = kept ? off + __popcll(mask & ((1ull << lane) - 1ull)) + 1 : 0;
        off += __popcll(mask);
    }
}

// one thread per record, j < n
__global__ void __launch_bounds__(kPixThreads) label_table_init_kernel(umx_label_object* __restrict__ table, long long n) {
    const long long j = (long long)blockIdx.x * kPixThreads + threadIdx.x;
    if (j >= n) return;
    umx_label_object o;
    o.area = 0; o.y0 = INT_MAX; o.x0 = INT_MAX; o.y1 = -1; o.x1 = -1; o.reserved = 0; o.sum_y = 0; o.sum_x = 0;
    table[j] = o;
}

// one row run [start, start + len) of row y into its object's record: integer atomics that nothing reads in the launch
__device__ inline void table_add(umx_label_object* o, int y, int start, int len) {
    atomicAdd(&o->area, len);
    atomicMin(&o->y0, y);
    atomicMax(&o->y1, y);
    atomicMin(&o->x0, start);
    atomicMax(&o->x1, start + len - 1);
    const unsigned long long l = (unsigned long long)len;
    atomicAdd(reinterpret_cast<unsigned long long*>(&o->sum_y), (unsigned long long)y * l);
    atomicAdd(reinterpret_cast<unsigned long long*>(&o->sum_x), (unsigned long long)start * l + l * (l - 1ull) / 2ull);
}

// grid ceil(H / 4).  P: roots; Q: the numbers at the roots (0: dropped).  out (may be null, may be P itself): a thread reads P at its
// own pixel and writes out there; Q is only read.  table[label - 1], label <= N: integer atomics that nothing reads in this launch.
__global__ void __launch_bounds__(64 * kRowWaves) label_write_kernel(const int* P, const int* __restrict__ Q, int H, int W, int* out,
                                                                      umx_label_object* __restrict__ table) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if ((long long)blockIdx.x * kRowWaves + wave >= H) return;    // (the whole wave: no barrier below)
    const int y = blockIdx.x * kRowWaves + wave;
    const size_t row = (size_t)y * W;
    for_each_run(
        W, lane,
        [&](int x) {
            const int p = P[row + x];
            const int label = p >= 0 ? Q[p] : 0;
            if (out) out[row + x] = label;
            return label - 1;
        },
        [&](int key, int start, int len) { table_add(table + key, y, start, len); });
}

// ---- the growth ----
// one thread per pixel, i < npix: the seed labels in place over P (roots, -1 off the objects) from the numbers at the roots in Q.  A
// thread writes P at its own pixel only and nobody writes Q.  No table: the seeds' records would count their pixels twice.
__global__ void __launch_bounds__(kPixThreads) label_seed_kernel(int* __restrict__ P, const int* __restrict__ Q, long long npix) {
    const long long i = (long long)blockIdx.x * kPixThreads + threadIdx.x;
    if (i >= npix) return;
    const int p = P[i];
    P[i] = p >= 0 ? Q[p] : 0;
}

// `levels` (1 .. kGrowHalo) synchronous levels of the growth, src -> dst (two different planes).  grid tiles_y * tiles_x, one
// workgroup per tile of 64 x 64 pixels: it loads the tile and a halo of 8 into LDS as one int per pixel -- the label (> 0), -1 for a
// pixel of the domain that is still empty (label 0 and first maximum of the planes in G), 0 for any other and for every pixel
// outside the image -- runs the levels there and writes its own tile.  A level: every thread reads its empty pixels' four
// neighbours (a neighbour outside the loaded region counts as absent) and keeps the least label among them in a register, a
// barrier, the changed pixels are written, a barrier.  The pixels whose value may be wrong for want of a neighbour are the
// region's outer ring after the first level and one ring more after each further one: after <= 8 levels they have not reached the
// tile.  The levels end early, for the whole workgroup, when the region has no empty domain pixel or no label, or when a level
// changed nothing (then no later one can).
// Bounds: region pixel r = j * 256 + thread < 6400 = 25 * 256; its image row and column are formed in 64 bits (y0 + 79 may pass
// 2^31) and a word of src, planes or dst is touched only at 0 <= gy < H, 0 <= gx < W, i.e. flat index < H * W <= INT_MAX.
// A workgroup reads src and planes, which nobody writes in this launch, and writes the words of dst of its own tile only.
// kCount (the regrow of the split, step 14): the workgroup also adds the pixels of its own tile that it claimed to *claimed -- one
// integer atomic per workgroup that claimed any, which nothing reads before the launch ends.  A claim inside the tile is never one
// of the possibly wrong ones, so the sum over the tiles is the number of pixels the launch labelled.  Without kCount the kernel
// is the one the plain growth always launched, and `claimed` is not touched.
// kFree (the reach of the contacts, step 23): every pixel whose value in src is outside 1..n_labels counts as 0 and is domain; no
// class is consulted and `planes` is never read (it may be null).  Chosen at compile time: without kFree n_labels is not looked
// at and the kernel is what it was.
template <bool kCount, bool kFree = false>
__global__ void __launch_bounds__(kGrowThreads) label_grow_kernel(const uint8_t* __restrict__ planes, int K, int H, int W, unsigned classes,
                                                                  const int* __restrict__ src, int* __restrict__ dst, int levels,
                                                                  int tiles_x, long long* __restrict__ claimed, int n_labels) {
    __shared__ int L[kGrowPix];
    int mine = 0;                                             // (kCount) claims of this thread inside the tile
    const int tid = threadIdx.x;
    const long long ty = blockIdx.x / tiles_x, tx = blockIdx.x % tiles_x;
    const long long y0 = ty * kGrowTile - kGrowHalo, x0 = tx * kGrowTile - kGrowHalo;
    const size_t npix = (size_t)H * W;
    int open = 0, seen = 0;
#pragma unroll 5
    for (int j = 0; j < kGrowPer; ++j) {
        const int r = j * kGrowThreads + tid;
        const long long gy = y0 + r / kGrowSide, gx = x0 + r % kGrowSide;
        int v = 0;
        if (gy >= 0 && gy < H && gx >= 0 && gx < W) {
            const size_t i = (size_t)gy * W + (size_t)gx;
            v = src[i];
            if (kFree) {
                if (v < 1 || v > n_labels) v = -1;
            } else if (v == 0) {                              // (a labelled pixel's class is never asked for)
                int arg = 0, best = planes[i];
                for (int k = 1; k < K; ++k) {
                    const int p = planes[(size_t)k * npix + i];
                    if (p > best) { best = p; arg = k; }      // first maximum, as label_runs_kernel
                }
                if ((classes >> arg) & 1u) v = -1;
            }
        }
        L[r] = v;
        open |= v < 0;
        seen |= v > 0;
    }
    const int any_open = __syncthreads_or(open);              // (the barriers that make L whole, too)
    const int any_seen = __syncthreads_or(seen);
    if (any_open && any_seen) {
        for (int t = 0; t < levels; ++t) {
            int nv[kGrowPer];
            int changed = 0;
#pragma unroll
            for (int j = 0; j < kGrowPer; ++j) {
                const int r = j * kGrowThreads + tid;
                int m = 0;
                if (L[r] < 0) {
                    const int ry = r / kGrowSide, rx = r % kGrowSide;
                    const int up = ry > 0 ? L[r - kGrowSide] : 0, down = ry < kGrowSide - 1 ? L[r + kGrowSide] : 0;
                    const int left = rx > 0 ? L[r - 1] : 0, right = rx < kGrowSide - 1 ? L[r + 1] : 0;
                    m = INT_MAX;
                    if (up > 0) m = up;
                    if (down > 0 && down < m) m = down;
                    if (left > 0 && left < m) m = left;
                    if (right > 0 && right < m) m = right;
                    if (m == INT_MAX) m = 0;
                    if (kCount && m > 0 && ry >= kGrowHalo && ry < kGrowHalo + kGrowTile && rx >= kGrowHalo && rx < kGrowHalo + kGrowTile) ++mine;
                }
                nv[j] = m;                                    // > 0: the pixel is claimed at this level
                changed |= m;
            }
            if (!__syncthreads_or(changed)) break;            // the same answer in every thread
#pragma unroll
            for (int j = 0; j < kGrowPer; ++j)
                if (nv[j] > 0) L[j * kGrowThreads + tid] = nv[j];
            __syncthreads();
        }
    }
#pragma unroll 4
    for (int j = 0; j < kGrowTile * kGrowTile / kGrowThreads; ++j) {
        const int q = j * kGrowThreads + tid;
        const int iy = q / kGrowTile, ix = q % kGrowTile;
        const long long gy = ty * kGrowTile + iy, gx = tx * kGrowTile + ix;
        if (gy < H && gx < W) {
            const int v = L[(iy + kGrowHalo) * kGrowSide + ix + kGrowHalo];
            dst[(size_t)gy * W + (size_t)gx] = v > 0 ? v : 0;
        }
    }
    if (kCount) {
        __shared__ int tile_claims;
        if (tid == 0) tile_claims = 0;
        __syncthreads();
        if (mine) atomicAdd(&tile_claims, mine);              // (LDS)
        __syncthreads();
        if (tid == 0 && tile_claims) atomicAdd(reinterpret_cast<unsigned long long*>(claimed), (unsigned long long)tile_claims);
    }
}

// grid ceil(H / 4).  F: the grown labels, read by a thread at its own pixel only; out (may be null, may be F itself, may be another
// plane): written there.  table[label - 1], label <= N, as in label_write_kernel.
__global__ void __launch_bounds__(64 * kRowWaves) label_grown_kernel(const int* F, int H, int W, int* out, umx_label_object* __restrict__ table) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if ((long long)blockIdx.x * kRowWaves + wave >= H) return;    // (the whole wave: no barrier below)
    const int y = blockIdx.x * kRowWaves + wave;
    const size_t row = (size_t)y * W;
    for_each_run(
        W, lane,
        [&](int x) {
            const int label = F[row + x];
            if (out && out != F) out[row + x] = label;
            return label - 1;
        },
        [&](int key, int start, int len) { table_add(table + key, y, start, len); });
}

// ---- the split ----
// A third int32 plane R (the components of the eroded set E, as P holds those of the objects) and a byte plane B of flags per pixel,
// the kFlag* of umx_label_state.h.
constexpr int kSplitWords = 4, kSplitBefore = 0, kSplitPacked = 1, kSplitClaimed = 2;   // the words of umx_labeler::d_split
constexpr int kErodeWords = kGrowPix / 64;                // the region of an erosion workgroup as one string of bits: 100 words, 800 B
constexpr int kErodeShift = kGrowSide - 64;               // a row down is kGrowSide bits on: one word and this many bits
static_assert(kErodeWords * 64 == kGrowPix && kErodeShift > 0 && kErodeShift < 64, "whole words; a row is between 64 and 128 bits");
static_assert(UMX_SPLIT_MAX_DEPTH <= kGrowHalo, "the erosion's halo argument");
static_assert(UMX_SPLIT_MAX_REGROW <= UMX_LABEL_MAX_GROW && UMX_SPLIT_MAX_CORE_AREA == UMX_LABEL_MAX_MIN_AREA, "the split's bounds");
static_assert(sizeof(umx_label_split_options) == 64 && sizeof(umx_label_split_counts) == 32, "the split's records");

// grid ceil(H / 4).  B: the flags, only read; R: every pixel of E gets its row run's head, every other one -1.
__global__ void __launch_bounds__(64 * kRowWaves) label_runs_mask_kernel(const uint8_t* __restrict__ B, int H, int W, int* __restrict__ R) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if ((long long)blockIdx.x * kRowWaves + wave >= H) return;    // (the whole wave: no barrier below)
    const int y = blockIdx.x * kRowWaves + wave;
    const size_t row = (size_t)y * W;
    write_row_runs(W, lane, row, R, [&](int x) { return (B[row + x] & kFlagEroded) != 0; });
}

// `depth` (1 .. 8) levels of erosion by the city-block ball.  grid tiles_y * tiles_x, the geometry of label_grow_kernel: one workgroup
// per tile of 64 x 64 pixels loads "the pixel belongs to a kept object" -- P[i] >= 0 and Q[P[i]] >= min_area: P holds the roots and Q
// the areas at the roots -- for the tile and a halo of 8 into LDS as ONE BIT per pixel, 0 for every pixel outside the image (step 11:
// outside the image is not in M).  Region pixel r = ry * 80 + rx is bit r of a string of 6400 bits = 100 words of 64: a wave's ballot
// over 64 consecutive region pixels IS one word, so the load needs no atomic and no shuffle.  A level is, per word,
//     m & (m << 1) & (m >> 1) & (m << 80) & (m >> 80)
// on the string (the shifts carry across words; past either end of the string they bring in 0): 100 threads, one word each, from one
// buffer into the other, one barrier.
// Why a halo of 8 suffices: a shift by 1 takes the left neighbour of a pixel of column 0 from column 79 of the row above, and the first
// and the last row get zeros for their missing neighbours -- so after the first level the region's outer ring may be wrong, and after
// each further level one ring more (a pixel's new value depends on its own and its four neighbours' old ones only).  After
// depth <= 8 levels the wrong pixels lie in the 8 outer rings, which is the halo: every pixel of the tile is right.  Equivalently:
// E(p) depends on the pixels of the ball of radius depth round p, and for p in the tile that ball lies in the region.
// Bounds: r < 6400; image row and column in 64 bits as in the growth; P and B are touched at 0 <= gy < H, 0 <= gx < W only, Q at a
// root P[i] < H * W.  A workgroup reads P and Q, which nobody writes in this launch, and writes the bytes of B of its own tile only:
// kFlagKept | kFlagEroded, every byte of the tile (B needs no clearing).
__global__ void __launch_bounds__(kGrowThreads) label_erode_kernel(const int* __restrict__ P, const int* __restrict__ Q, int H, int W, int min_area,
                                                                   int depth, int tiles_x, uint8_t* __restrict__ B) {
    __shared__ unsigned long long M0[kErodeWords], E[2][kErodeWords];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long ty = blockIdx.x / tiles_x, tx = blockIdx.x % tiles_x;
    const long long y0 = ty * kGrowTile - kGrowHalo, x0 = tx * kGrowTile - kGrowHalo;
    int seen = 0;
    for (int w = wave; w < kErodeWords; w += kGrowThreads / 64) {
        const int r = w * 64 + lane;
        const long long gy = y0 + r / kGrowSide, gx = x0 + r % kGrowSide;
        bool kept = false;
        if (gy >= 0 && gy < H && gx >= 0 && gx < W) {
            const int p = P[(size_t)gy * W + (size_t)gx];
            kept = p >= 0 && Q[p] >= min_area;
        }
        const unsigned long long mask = __ballot(kept);
        if (lane == 0) { M0[w] = mask; E[0][w] = mask; }
        seen |= mask != 0ull;
    }
    int cur = 0;
    if (__syncthreads_or(seen)) {                             // (the barrier that makes the string whole, too)
        for (int t = 0; t < depth; ++t) {
            if (tid < kErodeWords) {
                const unsigned long long* m = E[cur];
                const unsigned long long c = m[tid];
                const unsigned long long b1 = tid >= 1 ? m[tid - 1] : 0ull, b2 = tid >= 2 ? m[tid - 2] : 0ull;
                const unsigned long long a1 = tid + 1 < kErodeWords ? m[tid + 1] : 0ull, a2 = tid + 2 < kErodeWords ? m[tid + 2] : 0ull;
                const unsigned long long left = (c << 1) | (b1 >> 63), right = (c >> 1) | (a1 << 63);
                const unsigned long long up = (b1 << kErodeShift) | (b2 >> (64 - kErodeShift));
                const unsigned long long down = (a1 >> kErodeShift) | (a2 << (64 - kErodeShift));
                E[cur ^ 1][tid] = c & left & right & up & down;
            }
            __syncthreads();
            cur ^= 1;
        }
    }
#pragma unroll 4
    for (int j = 0; j < kGrowTile * kGrowTile / kGrowThreads; ++j) {
        const int q = j * kGrowThreads + tid;
        const int iy = q / kGrowTile, ix = q % kGrowTile;
        const long long gy = ty * kGrowTile + iy, gx = tx * kGrowTile + ix;
        if (gy < H && gx < W) {
            const int r = (iy + kGrowHalo) * kGrowSide + ix + kGrowHalo;
            const unsigned k = (unsigned)(M0[r >> 6] >> (r & 63)) & 1u, e = (unsigned)(E[cur][r >> 6] >> (r & 63)) & 1u;
            B[(size_t)gy * W + (size_t)gx] = (uint8_t)(k * kFlagKept | e * kFlagEroded);
        }
    }
}

// one thread per pixel, i < npix.  R: the roots of E's components, Q: their areas at the roots, P: the roots of the objects -- all
// only read.  The root pixel of every core (area >= core_min: one thread per core) sets kFlagCored in the byte of its OBJECT's root:
// an integer atomic OR on the aligned word that holds the byte (B is a whole number of words), which nothing reads in this launch.
__global__ void __launch_bounds__(kPixThreads) label_core_mark_kernel(const int* __restrict__ P, const int* __restrict__ R, const int* __restrict__ Q,
                                                                      long long npix, int core_min, uint8_t* __restrict__ B) {
    const long long i = (long long)blockIdx.x * kPixThreads + threadIdx.x;
    if (i >= npix) return;
    if (R[i] != (int)i || Q[i] < core_min) return;
    const int p = P[i];                                       // (>= 0: E is a subset of the objects' pixels)
    if (p < 0) return;
    atomicOr(reinterpret_cast<unsigned*>(B + ((size_t)p & ~(size_t)3)), kFlagCored << (8 * (p & 3)));
}

// grid ceil(npix / 2048), 256 threads, 8 pixels each.  The component id of every seed pixel (step 13) in place over P, -1 elsewhere:
// the core's root in R for a pixel of a core, the object's root in P for a pixel of a kept object that is not cored.  Both are flat
// indices of first pixels in raster order and distinct components have distinct ids, so label_count / _scan / _number_kernel number
// them as they number objects: a pixel is a seed root iff P[i] == i afterwards, and Q[i] >= 0 there (an area of E, or 0), so the
// numbering is asked with min_area 0.  A thread reads P at its own pixel only, which is the only word of P it writes; R, Q and B are
// only read.  *packed += (kept pixels that are no seed pixels) << 32 | (roots of cored objects): one 64-bit integer atomic per
// workgroup that has any, which nothing reads in this launch; the low half cannot carry (with h-maxima seeds a cored object may be one
// pixel, but there are at most H * W < 2^31 roots).
__global__ void __launch_bounds__(kPixThreads) label_split_ids_kernel(int* __restrict__ P, const int* __restrict__ R, const int* __restrict__ Q,
                                                                      const uint8_t* __restrict__ B, long long npix, int core_min,
                                                                      unsigned long long* __restrict__ packed) {
    __shared__ unsigned s_pending, s_cored;
    if (threadIdx.x == 0) { s_pending = 0; s_cored = 0; }
    __syncthreads();
    unsigned pending = 0, cored = 0;
    for (int j = 0; j < kScanBlock / kPixThreads; ++j) {
        const long long i = (long long)blockIdx.x * kScanBlock + j * kPixThreads + threadIdx.x;
        if (i >= npix) break;
        const unsigned b = B[i];
        int id = -1;
        if (b & kFlagKept) {
            const int p = P[i], r = R[i];
            if (r >= 0 && Q[r] >= core_min) id = r;
            else if (!(B[p] & kFlagCored)) id = p;
            pending += id < 0;
            cored += p == (int)i && (b & kFlagCored);
        }
        P[i] = id;
    }
    if (pending) atomicAdd(&s_pending, pending);              // (LDS)
    if (cored) atomicAdd(&s_cored, cored);
    __syncthreads();
    if (threadIdx.x == 0 && (s_pending | s_cored)) atomicAdd(packed, ((unsigned long long)s_pending << 32) | s_cored);
}

// ---- the level flood ----
constexpr int kFloodWords = 2, kFloodClaimed = 0, kFloodLeast = 1;   // the words of umx_labeler::d_flood
constexpr int kFloodNone = 0x7f7f7f7f;                               // the least-relief word before a launch: above every relief
static_assert(UMX_FLOOD_LAUNCH_STEPS == kGrowHalo && UMX_FLOOD_MAX_STEP == 256, "a flood launch runs a halo's worth of steps; reliefs are bytes");
static_assert(sizeof(umx_label_flood_options) == 96 && sizeof(umx_label_flood_counts) == 64, "the flood's records");
static_assert(sizeof(umx_label_hmax_options) == 128 && sizeof(umx_label_hmax_counts) == 96, "the h-maxima records");

// Up to `steps` (1 .. kGrowHalo) synchronous steps of the flood at ONE level t, src -> dst (two different planes): the geometry of
// label_grow_kernel -- grid tiles_y * tiles_x, one workgroup per tile of 64 x 64 pixels, the tile and a halo of 8 in LDS as one int
// per pixel:
//     > 0            the label
//     -1             an empty pixel of the level's domain: label 0, first maximum of the planes == cls, relief r <= t
//     -2 - r         an empty pixel of class cls that the level does not admit yet, with its relief r in t + 1 .. 255
//     0              any other pixel, and every pixel outside the image
// (the relief r = planes[relief_plane], or 255 - that with invert, is read for the empty pixels of class cls only: the LDS holds what
// the launch needs of it inside the state word).  A step is the growth's: every -1 pixel takes the least label among its four
// neighbours of the step before; the steps end, for the whole workgroup, when one changed nothing.  The admission is fixed for the
// launch and a pixel's new value depends on its own and its four neighbours' old ones only, so the halo argument is the growth's
// word for word: after s <= 8 steps from an exact global state the wrong pixels lie in the s outer rings, and the tile is exact.
// What a launch reports besides its tile, both by integer atomics that nothing reads before the launch ends:
//   *claimed += the pixels of its own tile that it labelled (one 64-bit add per workgroup that claimed any);
//   *least = min(*least, r) over the pixels of its own tile that are -2 - r and have a labelled 4-neighbour in the LDS state at the
//            end of the launch (one 32-bit atomicMin per workgroup that has one).  A tile pixel has all four neighbours in the
//            region.  The LDS state of the halo may be stale while the launch still claims; the host uses the word only of a launch
//            that claimed nothing, in which every LDS state is the global one (run_flood_launches).
// Bounds: as label_grow_kernel -- region pixel r < 6400, image row and column in 64 bits, src / planes / dst touched at
// 0 <= gy < H, 0 <= gx < W only; relief_plane < K (umx_label_flood_check), so its word is below K * H * W.  A workgroup reads src
// and planes, which nobody writes in this launch, and writes the words of dst of its own tile only.
__global__ void __launch_bounds__(kGrowThreads) label_flood_kernel(const uint8_t* __restrict__ planes, int K, int H, int W, int cls,
                                                                   int relief_plane, int invert, int t, const int* __restrict__ src,
                                                                   int* __restrict__ dst, int steps, int tiles_x,
                                                                   long long* __restrict__ claimed, int* __restrict__ least) {
    __shared__ int L[kGrowPix];
    __shared__ int tile_claims, tile_least;
    int mine = 0;                                             // claims of this thread inside the tile
    const int tid = threadIdx.x;
    const long long ty = blockIdx.x / tiles_x, tx = blockIdx.x % tiles_x;
    const long long y0 = ty * kGrowTile - kGrowHalo, x0 = tx * kGrowTile - kGrowHalo;
    const size_t npix = (size_t)H * W;
    if (tid == 0) { tile_claims = 0; tile_least = kFloodNone; }
    int open = 0, seen = 0, later = 0;
#pragma unroll 5
    for (int j = 0; j < kGrowPer; ++j) {
        const int r = j * kGrowThreads + tid;
        const long long gy = y0 + r / kGrowSide, gx = x0 + r % kGrowSide;
        int v = 0;
        if (gy >= 0 && gy < H && gx >= 0 && gx < W) {
            const size_t i = (size_t)gy * W + (size_t)gx;
            v = src[i];
            if (v == 0) {                                     // (a labelled pixel's class and relief are never asked for)
                int arg = 0, best = planes[i];
                for (int k = 1; k < K; ++k) {
                    const int p = planes[(size_t)k * npix + i];
                    if (p > best) { best = p; arg = k; }      // first maximum, as label_runs_kernel
                }
                if (arg == cls) {
                    const int b = planes[(size_t)relief_plane * npix + i];
                    const int relief = invert ? 255 - b : b;
                    v = relief <= t ? -1 : -2 - relief;
                }
            }
        }
        L[r] = v;
        open |= v == -1;
        seen |= v > 0;
        later |= v < -1;
    }
    const int any_open = __syncthreads_or(open);              // (the barriers that make L and the two tile words whole, too)
    const int any_seen = __syncthreads_or(seen);
    const int any_later = __syncthreads_or(later);
    if (any_open && any_seen) {
        for (int s = 0; s < steps; ++s) {
            int nv[kGrowPer];
            int changed = 0;
#pragma unroll
            for (int j = 0; j < kGrowPer; ++j) {
                const int r = j * kGrowThreads + tid;
                int m = 0;
                if (L[r] == -1) {
                    const int ry = r / kGrowSide, rx = r % kGrowSide;
                    const int up = ry > 0 ? L[r - kGrowSide] : 0, down = ry < kGrowSide - 1 ? L[r + kGrowSide] : 0;
                    const int left = rx > 0 ? L[r - 1] : 0, right = rx < kGrowSide - 1 ? L[r + 1] : 0;
                    m = INT_MAX;
                    if (up > 0) m = up;
                    if (down > 0 && down < m) m = down;
                    if (left > 0 && left < m) m = left;
                    if (right > 0 && right < m) m = right;
                    if (m == INT_MAX) m = 0;
                    if (m > 0 && ry >= kGrowHalo && ry < kGrowHalo + kGrowTile && rx >= kGrowHalo && rx < kGrowHalo + kGrowTile) ++mine;
                }
                nv[j] = m;                                    // > 0: the pixel is claimed at this step
                changed |= m;
            }
            if (!__syncthreads_or(changed)) break;            // the same answer in every thread
#pragma unroll
            for (int j = 0; j < kGrowPer; ++j)
                if (nv[j] > 0) L[j * kGrowThreads + tid] = nv[j];
            __syncthreads();
        }
    }
    int low = kFloodNone;                                     // the least relief of this thread's waiting tile pixels beside a label
#pragma unroll 4
    for (int j = 0; j < kGrowTile * kGrowTile / kGrowThreads; ++j) {
        const int q = j * kGrowThreads + tid;
        const int iy = q / kGrowTile, ix = q % kGrowTile;
        const long long gy = ty * kGrowTile + iy, gx = tx * kGrowTile + ix;
        if (gy < H && gx < W) {
            const int r = (iy + kGrowHalo) * kGrowSide + ix + kGrowHalo;   // (kGrowHalo >= 1: the four neighbours are region pixels)
            const int v = L[r];
            dst[(size_t)gy * W + (size_t)gx] = v > 0 ? v : 0;
            if (any_seen && any_later && v < -1 && -2 - v < low &&
                (L[r - kGrowSide] > 0 || L[r + kGrowSide] > 0 || L[r - 1] > 0 || L[r + 1] > 0))
                low = -2 - v;
        }
    }
    if (mine) atomicAdd(&tile_claims, mine);                  // (LDS)
    if (low != kFloodNone) atomicMin(&tile_least, low);
    __syncthreads();
    if (tid == 0) {
        if (tile_claims) atomicAdd(reinterpret_cast<unsigned long long*>(claimed), (unsigned long long)tile_claims);
        if (tile_least != kFloodNone) atomicMin(least, tile_least);
    }
}

// ---- the measurement ----
// What one row run carries of G planes: its pixel count and, per plane, the sum, the sum of squares, the least and the largest value.
template <int G>
struct RunSums {
    unsigned count;
    unsigned long long sum[G], sq[G];
    unsigned mn[G], mx[G];
};

// lane 63's value in every lane, wave-uniform (one v_readlane per word: no LDS crossing)
__device__ inline unsigned of_lane63(unsigned v) { return (unsigned)__builtin_amdgcn_readlane((int)v, 63); }
__device__ inline unsigned long long of_lane63(unsigned long long v) {
    return ((unsigned long long)of_lane63((unsigned)(v >> 32)) << 32) | of_lane63((unsigned)v);
}

// The sibling of for_each_run that carries a payload: key_at(x) once for every pixel of the row as there; val_at(x, g) <= 65535 once
// for every pixel with key >= 0 and plane g < G; flush(key, sums) once for every maximal segment of equal key >= 0 -- by one lane, the
// LAST pixel of the segment (or lane 0 for a carried segment that the next chunk does not continue).  Inside a chunk the sums of a
// segment are a segmented inclusive scan over the lanes (6 steps; a lane adds the value d lanes to its left iff that lane is in its
// segment), of two words per plane:
//   (v << 38) | v * v   64 pixels of v <= 65535: the squares sum to < 64 * 2^32 = 2^38, the values to <= 64 * 65535 < 2^22: 60 bits;
//   (v << 16) | v       the largest value in the upper half, the least in the lower one, compared half by half.
// A segment that reaches the end of a chunk is carried in wave-uniform registers with 64-bit sums (one row run of 70 000 pixels of
// 65535 passes 2^32) and joined to the first segment of the next chunk when the keys agree: one flush however long the run is.
// ceil(W / 64) rounds; count <= W.  A chunk without any key >= 0 costs its keys and one ballot: no value of it is read.
template <int G, typename KeyAt, typename ValAt, typename Flush>
__device__ inline void for_each_run_sums(int W, int lane, KeyAt key_at, ValAt val_at, Flush flush) {
    constexpr unsigned long long kSqMask = (1ull << 38) - 1ull;
    RunSums<G> carry;                                     // the carried segment, the same in every lane; ckey < 0: none
    int ckey = -1;
    carry.count = 0;
#pragma unroll
    for (int g = 0; g < G; ++g) { carry.sum[g] = carry.sq[g] = 0; carry.mn[g] = carry.mx[g] = 0; }
    const int nchunks = (W - 1) / 64 + 1;
    for (int c = 0; c < nchunks; ++c) {
        const int x0 = c * 64;
        const bool in = lane < W - x0;
        const int x = in ? x0 + lane : x0;
        const int t = in ? key_at(x) : -2;                // past the row's end: a key no pixel has
        const bool last = c + 1 == nchunks;
        if (__ballot(t >= 0) == 0ull) {                   // (the same answer in every lane)
            if (ckey >= 0 && lane == 0) flush(ckey, carry);
            ckey = -1;
            continue;
        }
        const int tl = __shfl_up(t, 1);
        const bool head = lane == 0 || t != tl;
        const unsigned long long heads = __ballot(head);  // (bit 0 is always set)
        const int first = 63 - __clzll((long long)(heads & (~0ull >> (63 - lane))));   // the lane of this segment's head, <= lane
        const bool tail = lane == 63 || ((heads >> (lane + 1)) & 1ull);
        unsigned long long pk[G];
        unsigned mm[G];
#pragma unroll
        for (int g = 0; g < G; ++g) {
            const unsigned v = t >= 0 ? val_at(x, g) : 0u;
            pk[g] = ((unsigned long long)v << 38) | (unsigned long long)(v * v);   // (v * v < 2^32)
            mm[g] = (v << 16) | v;
        }
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {                // 6 steps
            const bool take = lane - d >= first;
#pragma unroll
            for (int g = 0; g < G; ++g) {
                const unsigned long long p = __shfl_up(pk[g], d);
                const unsigned m = __shfl_up(mm[g], d);
                if (take) {
                    pk[g] += p;
                    const unsigned hi = max(mm[g] >> 16, m >> 16), lo = min(mm[g] & 0xffffu, m & 0xffffu);
                    mm[g] = (hi << 16) | lo;
                }
            }
        }
        RunSums<G> r;                                     // of the segment's pixels up to this lane: the whole segment at its tail
        r.count = (unsigned)(lane - first + 1);
#pragma unroll
        for (int g = 0; g < G; ++g) { r.sum[g] = pk[g] >> 38; r.sq[g] = pk[g] & kSqMask; r.mn[g] = mm[g] & 0xffffu; r.mx[g] = mm[g] >> 16; }
        if (ckey >= 0) {
            if (__shfl(t, 0) == ckey) {                   // the chunk's first segment continues the carried one
                if (first == 0) {
                    r.count += carry.count;
#pragma unroll
                    for (int g = 0; g < G; ++g) {
                        r.sum[g] += carry.sum[g]; r.sq[g] += carry.sq[g];
                        r.mn[g] = min(r.mn[g], carry.mn[g]); r.mx[g] = max(r.mx[g], carry.mx[g]);
                    }
                }
            } else if (lane == 0) {
                flush(ckey, carry);
            }
        }
        if (tail && t >= 0 && (lane != 63 || last)) flush(t, r);
        const int t63 = __builtin_amdgcn_readlane(t, 63);
        if (!last && t63 >= 0) {
            ckey = t63;
            carry.count = of_lane63(r.count);
#pragma unroll
            for (int g = 0; g < G; ++g) {
                carry.sum[g] = of_lane63(r.sum[g]); carry.sq[g] = of_lane63(r.sq[g]);
                carry.mn[g] = of_lane63(r.mn[g]); carry.mx[g] = of_lane63(r.mx[g]);
            }
        } else {
            ckey = -1;
        }
    }
}

// one thread per record, j < n: the record of a label that no pixel carries
__global__ void __launch_bounds__(kPixThreads) label_measure_init_kernel(umx_label_measure* __restrict__ rec, long long n) {
    const long long j = (long long)blockIdx.x * kPixThreads + threadIdx.x;
    if (j >= n) return;
    umx_label_measure m;
    m.sum = 0; m.sum_sq = 0; m.min = UINT_MAX; m.max = 0; m.count = 0; m.reserved = 0;
    rec[j] = m;
}

// grid ceil(H / 4).  labels [H][W] and planes [G][H][W] are only read, the labels once for the G planes.  A label outside 1..N is
// key -1: no record is addressed for it.  rec [G][N]: record g * N + label - 1 < G * N takes, per row run, two 64-bit adds, one
// 32-bit add, one min and one max -- integer atomics that nothing reads in this launch.  Bounds: row y < H; a pixel word is
// y * W + x < H * W <= INT_MAX, plane g's at g * H * W + that, formed in 64 bits.
// Known limit ("salt"): an object made of 10^7 one-pixel runs sends 10^7 sets of atomics to one record, which
// the memory system serialises; nothing here spreads them.
template <typename T, int G>
__global__ void __launch_bounds__(64 * kRowWaves) label_measure_kernel(const int* __restrict__ labels, const T* __restrict__ planes, int H,
                                                                        int W, int N, umx_label_measure* __restrict__ rec) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if ((long long)blockIdx.x * kRowWaves + wave >= H) return;    // (the whole wave: no barrier below)
    const int y = blockIdx.x * kRowWaves + wave;
    const size_t npix = (size_t)H * W, row = (size_t)y * W;
    for_each_run_sums<G>(
        W, lane,
        [&](int x) {
            const int l = labels[row + x];
            return l >= 1 && l <= N ? l - 1 : -1;
        },
        [&](int x, int g) { return (unsigned)planes[(size_t)g * npix + row + x]; },
        [&](int key, const RunSums<G>& r) {
#pragma unroll
            for (int g = 0; g < G; ++g) {
                umx_label_measure* o = rec + (size_t)g * N + key;
                atomicAdd(reinterpret_cast<unsigned long long*>(&o->sum), r.sum[g]);
                atomicAdd(reinterpret_cast<unsigned long long*>(&o->sum_sq), r.sq[g]);
                atomicAdd(&o->count, r.count);
                atomicMin(&o->min, r.mn[g]);
                atomicMax(&o->max, r.mx[g]);
            }
        });
}

// ---- the shapes ----
// The five window counts of step 16 as one word: fields of kQuadBits bits, q1 lowest.  A pixel adds at most 4 (one per window that
// holds it), a 64-pixel chunk at most 256 to a field: 9 bits would do, 12 leave room and still fit five fields.
constexpr int kQuads = 5, kQuadBits = 12;
constexpr unsigned long long kQ1 = 1ull, kQ2 = 1ull << kQuadBits, kQd = 1ull << (2 * kQuadBits), kQ3 = 1ull << (3 * kQuadBits),
                             kQ4 = 1ull << (4 * kQuadBits);
static_assert(4 * 64 < (1 << kQuadBits) && kQuads * kQuadBits <= 64, "a chunk's counts fit their fields, the fields one word");
static_assert(sizeof(umx_label_shape) == 64, "the shape record");

// What one row run carries: its pixel count (its columns are [xb - count + 1, xb] at the flush) and its five window counts.
struct RunQuads {
    unsigned count;
    unsigned q[kQuads];
};

// The sibling of for_each_run_sums whose payload is one packed word of small counts: key_at(x) once for every pixel of the row as
// there; word_at(x, t) -- t the pixel's key, -2 past the row's end -- is called by ALL 64 lanes together in every chunk that holds a
// key >= 0 (so it may shuffle) and returns the pixel's fields, 0 where t < 0; flush(key, xb, r) once for every maximal segment of
// equal key >= 0, xb its last column -- by one lane, the last pixel of the segment (or lane 0 for a carried segment that the next
// chunk does not continue).  Inside a chunk the fields of a segment are one segmented inclusive scan of the word (6 steps); a
// segment that reaches the end of a chunk is carried unpacked in wave-uniform registers (a run of 65536 pixels counts to 2^18) and
// joined to the first segment of the next chunk when the keys agree.  ceil(W / 64) rounds; count <= W.
template <typename KeyAt, typename WordAt, typename Flush>
__device__ inline void for_each_run_quads(int W, int lane, KeyAt key_at, WordAt word_at, Flush flush) {
    constexpr unsigned kField = (1u << kQuadBits) - 1u;
    RunQuads carry;                                       // the carried segment, the same in every lane; ckey < 0: none
    int ckey = -1, cend = 0;                              // cend: the last column of the chunk the carry ends in
    carry.count = 0;
#pragma unroll
    for (int k = 0; k < kQuads; ++k) carry.q[k] = 0;
    const int nchunks = (W - 1) / 64 + 1;
    for (int c = 0; c < nchunks; ++c) {
        const int x0 = c * 64;
        const bool in = lane < W - x0;
        const int x = in ? x0 + lane : x0;
        const int t = in ? key_at(x) : -2;                // past the row's end: a key no pixel has
        const bool last = c + 1 == nchunks;
        if (__ballot(t >= 0) == 0ull) {                   // (the same answer in every lane)
            if (ckey >= 0 && lane == 0) flush(ckey, cend, carry);
            ckey = -1;
            continue;
        }
        const int tl = __shfl_up(t, 1);
        const bool head = lane == 0 || t != tl;
        const unsigned long long heads = __ballot(head);  // (bit 0 is always set)
        const int first = 63 - __clzll((long long)(heads & (~0ull >> (63 - lane))));   // the lane of this segment's head, <= lane
        const bool tail = lane == 63 || ((heads >> (lane + 1)) & 1ull);
        unsigned long long pk = word_at(x, t);
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {                // 6 steps
            const unsigned long long p = __shfl_up(pk, d);
            if (lane - d >= first) pk += p;
        }
        RunQuads r;                                       // of the segment's pixels up to this lane: the whole segment at its tail
        r.count = (unsigned)(lane - first + 1);
#pragma unroll
        for (int k = 0; k < kQuads; ++k) r.q[k] = (unsigned)(pk >> (k * kQuadBits)) & kField;
        if (ckey >= 0) {
            if (__shfl(t, 0) == ckey) {                   // the chunk's first segment continues the carried one
                if (first == 0) {
                    r.count += carry.count;
#pragma unroll
                    for (int k = 0; k < kQuads; ++k) r.q[k] += carry.q[k];
                }
            } else if (lane == 0) {
                flush(ckey, cend, carry);
            }
        }
        if (tail && t >= 0 && (lane != 63 || last)) flush(t, x, r);
        const int t63 = __builtin_amdgcn_readlane(t, 63);
        if (!last && t63 >= 0) {
            ckey = t63;
            cend = x0 + 63;
            carry.count = of_lane63(r.count);
#pragma unroll
            for (int k = 0; k < kQuads; ++k) carry.q[k] = of_lane63(r.q[k]);
        } else {
            ckey = -1;
        }
    }
}

// one thread per record, j < n: the record of a label that no pixel carries
__global__ void __launch_bounds__(kPixThreads) label_shape_init_kernel(umx_label_shape* __restrict__ rec, long long n) {
    const long long j = (long long)blockIdx.x * kPixThreads + threadIdx.x;
    if (j >= n) return;
    umx_label_shape z;
    z.sum_y = z.sum_x = z.sum_yy = z.sum_xy = z.sum_xx = 0;
    z.q1 = z.q2 = z.qd = z.q3 = z.q4 = z.reserved = 0;
    rec[j] = z;
}

// 0^2 + 1^2 + ... + m^2 for -1 <= m < 65536: the product is below 2^49
__device__ inline long long squares_to(long long m) { return m * (m + 1) * (2 * m + 1) / 6; }

// grid ceil(H / 4).  labels [H][W] is only read: row y by its wave's lanes, rows y - 1 and y + 1 alongside it (outside the image is
// 0, which no object carries).  A label outside 1..N is key -1: no record is addressed for it, and as a neighbour it equals no label
// that is.  rec [N]: record label - 1 takes, per row run, the moments -- closed forms of y and the run's two ends -- and the window
// counts: integer atomic adds that nothing reads in this launch, those with an addend of 0 left out.
// The windows: a pixel lies in four 2x2 windows of the padded plane, as their down-right, down-left, up-right and up-left corner.  A
// (window, label) pair is counted by the FIRST pixel of that label in the window in the order up-left, up-right, down-left,
// down-right, so exactly once, and by a function of the pixel's 3x3 neighbourhood: e.g. as the down-right corner a pixel counts
// the window only when none of the three others has its label, and then the window holds one pixel of it.
// Bounds: row y < H; a pixel word is r * W + x < H * W <= INT_MAX for 0 <= r < H and 0 <= x < W, formed in 64 bits; the columns
// x0 - 1 and x0 + 64 are read by one lane each and only where they are >= 0 and < W; H, W <= 65536 (umx_label_shape_check), so
// m * (m + 1) * (2 m + 1) and y * y * W stay far inside 64 bits.
// Known limit ("salt"): an object made of 10^7 one-pixel runs sends 10^7 sets of atomics to one record.
__global__ void __launch_bounds__(64 * kRowWaves) label_shape_kernel(const int* __restrict__ labels, int H, int W, int N,
                                                                      umx_label_shape* __restrict__ rec) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if ((long long)blockIdx.x * kRowWaves + wave >= H) return;    // (the whole wave: no barrier below)
    const int y = blockIdx.x * kRowWaves + wave;
    const int* mid = labels + (size_t)y * W;
    const int* up = y > 0 ? labels + (size_t)(y - 1) * W : nullptr;
    const int* dn = y + 1 < H ? labels + (size_t)(y + 1) * W : nullptr;
    // the labels at columns x - 1 and x + 1 of one row (null: outside the image) from the lanes' own m at column x, by all lanes
    // together; a lane past the row's end holds an m that is no label
    auto three = [&](const int* row, int x, bool in, int& l, int& m, int& r) {
        l = __shfl_up(m, 1);
        r = __shfl_down(m, 1);
        if (lane == 0) l = row && in && x > 0 ? row[x - 1] : 0;
        if (lane == 63) r = row && in && x + 1 < W ? row[x + 1] : 0;
    };
    for_each_run_quads(
        W, lane,
        [&](int x) {
            const int l = mid[x];
            return l >= 1 && l <= N ? l - 1 : -1;
        },
        [&](int x, int t) {
            const bool in = t != -2;
            const int L = t + 1;                          // the pixel's label; 0 or less where it has no record: equal to no label
            int ul, uc = up && in ? up[x] : 0, ur, ml, mc = L, mr, dl, dc = dn && in ? dn[x] : 0, dr;
            three(up, x, in, ul, uc, ur);
            three(mid, x, in, ml, mc, mr);
            three(dn, x, in, dl, dc, dr);
            if (t < 0) return 0ull;
            const bool e_ul = ul == L, e_uc = uc == L, e_ur = ur == L, e_ml = ml == L, e_mr = mr == L, e_dl = dl == L, e_dc = dc == L,
                       e_dr = dr == L;
            unsigned long long w = 0;
            if (!e_ul && !e_uc && !e_ml) w += kQ1;                               // down-right corner: alone in it
            if (!e_uc && !e_ur) w += e_mr ? kQ2 : kQ1;                           // down-left: with its right neighbour at most
            if (!e_ml) w += e_dl ? (e_dc ? kQ3 : kQd) : (e_dc ? kQ2 : kQ1);      // up-right: the row below decides
            const int n = (int)e_mr + (int)e_dc + (int)e_dr;                     // up-left: always the first
            w += n == 0 ? kQ1 : n == 3 ? kQ4 : n == 2 ? kQ3 : e_dr ? kQd : kQ2;
            return w;
        },
        [&](int key, int xb, const RunQuads& r) {
            umx_label_shape* o = rec + key;
            const long long n = r.count, xa = xb - n + 1;
            const long long sx = (xa + xb) * n / 2;       // (xa + xb and n are not both odd)
            const long long sxx = squares_to(xb) - squares_to(xa - 1);
            auto add64 = [](int64_t* p, long long v) {
                if (v) atomicAdd(reinterpret_cast<unsigned long long*>(p), (unsigned long long)v);
            };
            add64(&o->sum_y, (long long)y * n);
            add64(&o->sum_x, sx);
            add64(&o->sum_yy, (long long)y * y * n);
            add64(&o->sum_xy, (long long)y * sx);
            add64(&o->sum_xx, sxx);
            unsigned* const q[kQuads] = {&o->q1, &o->q2, &o->qd, &o->q3, &o->q4};
#pragma unroll
            for (int k = 0; k < kQuads; ++k)
                if (r.q[k]) atomicAdd(q[k], r.q[k]);
        });
}

}  // namespace

}  // namespace umx

namespace umx {

int lfail(umx_labeler* lb, int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (lb) lb->err = buf;
    g_err = buf;
    return code;
}

namespace {

// Buffers for K planes of H x W.  Nothing shrinks; when one is too small the arena is emptied and every buffer allocated again at the
// larger of its old and its needed size (the arena frees as a whole, and the red zones of guard mode are per allocation).
// split: the call is a split run, which also needs the third plane and the flags; once allocated they are kept and grow with the rest.
int ensure_buffers(umx_labeler* lb, size_t plane_bytes, size_t npix, size_t nblocks, bool split) {
    const size_t split_need = split ? npix : 0;
    if (plane_bytes <= lb->planes_cap && npix <= lb->pix_cap && nblocks <= lb->counts_cap && split_need <= lb->split_cap && lb->d_n) return UMX_OK;
    L_HIP(lb, hipStreamSynchronize(lb->stream));
    arena_free(&lb->mem);
    lb->d_planes = nullptr; lb->d_P = lb->d_Q = lb->d_counts = nullptr; lb->d_n = nullptr; lb->d_table = nullptr;
    lb->d_R = nullptr; lb->d_B = nullptr; lb->d_split = nullptr; lb->d_flood = nullptr; lb->d_hmax = nullptr;
    lb->d_mplanes = nullptr; lb->d_mrec = nullptr; lb->mplanes_cap = lb->mrec_cap = 0;   // (the measurement allocates its own again)
    lb->d_srec = nullptr; lb->srec_cap = 0;                                              // (and so do the shapes)
    contact_buffers_forget(lb);                                                          // (and the contacts)
    hull_buffers_forget(lb);                                                             // (and the hulls)
    relabel_buffers_forget(lb);                                                          // (and the relabel)
    const size_t pb = std::max(plane_bytes, lb->planes_cap), px = std::max(npix, lb->pix_cap), nb = std::max(nblocks, lb->counts_cap);
    const size_t tc = std::max<size_t>(lb->table_cap, 1024);
    const size_t sp = std::max(split_need, lb->split_cap);
    lb->planes_cap = lb->pix_cap = lb->counts_cap = lb->table_cap = lb->split_cap = 0;
    L_HIP(lb, arena_alloc(&lb->mem, (void**)&lb->d_P, px * sizeof(int), false, "label parents"));
    L_HIP(lb, arena_alloc(&lb->mem, (void**)&lb->d_Q, px * sizeof(int), false, "label areas"));
    L_HIP(lb, arena_alloc(&lb->mem, (void**)&lb->d_counts, nb * sizeof(int), false, "label block counts"));
    L_HIP(lb, arena_alloc(&lb->mem, (void**)&lb->d_n, sizeof(long long), true, "label count"));
    L_HIP(lb, arena_alloc(&lb->mem, (void**)&lb->d_table, tc * sizeof(umx_label_object), false, "label table"));
    if (pb) L_HIP(lb, arena_alloc(&lb->mem, (void**)&lb->d_planes, pb, false, "label planes"));
    if (sp) {
        L_HIP(lb, arena_alloc(&lb->mem, (void**)&lb->d_R, sp * sizeof(int), false, "label core parents"));
        L_HIP(lb, arena_alloc(&lb->mem, (void**)&lb->d_B, (sp + 3) / 4 * 4, false, "label split flags"));
        L_HIP(lb, arena_alloc(&lb->mem, (void**)&lb->d_split, kSplitWords * sizeof(long long), true, "label split counts"));
        L_HIP(lb, arena_alloc(&lb->mem, (void**)&lb->d_flood, kFloodWords * sizeof(long long), true, "label flood words"));
        L_HIP(lb, arena_alloc(&lb->mem, (void**)&lb->d_hmax, kHmaxWords * sizeof(long long), true, "label h-maxima words"));
    }
    lb->planes_cap = pb; lb->pix_cap = px; lb->counts_cap = nb; lb->table_cap = tc; lb->split_cap = sp;
    return UMX_OK;
}

// (a table that grows leaves its old block in the arena until the arena is next emptied: sizes double, so that is less than the new one)
int ensure_table(umx_labeler* lb, size_t n) {
    if (n <= lb->table_cap) return UMX_OK;
    const size_t tc = std::max(n, 2 * lb->table_cap);
    L_HIP(lb, hipStreamSynchronize(lb->stream));
    lb->table_cap = 0;
    L_HIP(lb, arena_alloc(&lb->mem, (void**)&lb->d_table, tc * sizeof(umx_label_object), false, "label table"));
    lb->table_cap = tc;
    return UMX_OK;
}

inline unsigned row_grid(int H) { return (unsigned)((H - 1) / kRowWaves + 1); }

// The components of the run heads in X (label_runs_kernel's or label_runs_mask_kernel's): X = the root of every object pixel, -1 off
// the objects; Q = the areas at the roots, 0 elsewhere.
int launch_components(umx_labeler* lb, int* X, int* Q, int H, int W) {
    const long long npix = (long long)H * W;
    const unsigned pix_grid = (unsigned)((npix + kPixThreads - 1) / kPixThreads);
    hipStream_t s = lb->stream;
    hipLaunchKernelGGL(label_strip_kernel, dim3((unsigned)((H - 1) / kStripRows + 1)), dim3(kMergeThreads), 0, s, X, H, W);
    for (long long span = kStripRows; span < H; span *= 2) {   // at most 26 levels
        const long long seams = (H - span + 2 * span - 1) / (2 * span);
        hipLaunchKernelGGL(label_seam_kernel, dim3((unsigned)seams), dim3(kMergeThreads), 0, s, X, H, W, span);
    }
    hipLaunchKernelGGL(label_heads_kernel, dim3(pix_grid), dim3(kPixThreads), 0, s, X, Q, npix, W);
    hipLaunchKernelGGL(label_flatten_kernel, dim3(row_grid(H)), dim3(64 * kRowWaves), 0, s, X, Q, H, W);
    L_HIP(lb, hipMemsetAsync(Q, 0, (size_t)npix * sizeof(int), s));
    hipLaunchKernelGGL(label_area_kernel, dim3(row_grid(H)), dim3(64 * kRowWaves), 0, s, X, Q, H, W);
    return UMX_OK;
}

// The count of the numbering (kept(i) = P[i] == i and Q[i] >= min_area) to *total on the device.
void launch_count(umx_labeler* lb, const int* P, const int* Q, long long npix, int min_area, long long* total) {
    const int nblocks = (int)((npix + kScanBlock - 1) / kScanBlock);
    hipLaunchKernelGGL(label_count_kernel, dim3((unsigned)nblocks), dim3(64 * kScanWaves), 0, lb->stream, P, Q, npix, min_area, lb->d_counts);
    hipLaunchKernelGGL(label_scan_kernel, dim3(1), dim3(kMergeThreads), 0, lb->stream, lb->d_counts, nblocks, total);
}

// n (the count the device left in d_n) to the host -- the stream is idle afterwards -- and the table sized and cleared for it
int read_count_and_init_table(umx_labeler* lb, long long npix, long long* n_out) {
    hipStream_t s = lb->stream;
    L_HIP(lb, hipGetLastError());
    long long n = 0;
    L_HIP(lb, hipMemcpyAsync(&n, lb->d_n, sizeof n, hipMemcpyDeviceToHost, s));
    L_HIP(lb, hipStreamSynchronize(s));
    if (n < 0 || n > npix) return lfail(lb, UMX_ERR_HIP, "the label scan counted %lld objects in %lld pixels", n, npix);
    const int rc = ensure_table(lb, (size_t)n);
    if (rc) return rc;
    if (n > 0)
        hipLaunchKernelGGL(label_table_init_kernel, dim3((unsigned)((n + kPixThreads - 1) / kPixThreads)), dim3(kPixThreads), 0, s, lb->d_table, n);
    *n_out = n;
    return UMX_OK;
}

// The rim growth (step 6) from the labels in src, with dst as the other plane -- ceil(R / 8) launches between the two, the last one
// of R mod 8 levels (8 when that is 0); none when grow_radius is 0 -- then one pass over the plane that holds the result: the labels
// to where the call wants them, the table.
void launch_grow_and_table(umx_labeler* lb, const uint8_t* planes, int K, int H, int W, const umx_label_options* o, int* src, int* dst, int* out) {
    hipStream_t s = lb->stream;
    const int tiles_x = (W - 1) / kGrowTile + 1, tiles_y = (H - 1) / kGrowTile + 1;   // tiles_y * tiles_x <= 2^25 + 2^19: H * W <= INT_MAX
    for (int left = o->grow_radius; left > 0; left -= kGrowHalo) {
        hipLaunchKernelGGL(label_grow_kernel<false>, dim3((unsigned)tiles_y * (unsigned)tiles_x), dim3(kGrowThreads), 0, s, planes, K, H, W,
                           o->grow_classes, src, dst, std::min(left, kGrowHalo), tiles_x, (long long*)nullptr, 0);
        std::swap(src, dst);
    }
    hipLaunchKernelGGL(label_grown_kernel, dim3(row_grid(H)), dim3(64 * kRowWaves), 0, s, src, H, W, out, lb->d_table);
}

// the launches of one call on planes already on the device; out: null, the caller's plane or lb->d_P.  Returns with the stream idle
// up to the count's read-back and the last launches enqueued.
int run_launches(umx_labeler* lb, const uint8_t* planes, int K, int H, int W, const umx_label_options* o, int* out, long long* n_out) {
    const long long npix = (long long)H * W;
    const int nblocks = (int)((npix + kScanBlock - 1) / kScanBlock);
    const unsigned pix_grid = (unsigned)((npix + kPixThreads - 1) / kPixThreads);
    hipStream_t s = lb->stream;
    int *P = lb->d_P, *Q = lb->d_Q;
    hipLaunchKernelGGL(label_runs_kernel, dim3(row_grid(H)), dim3(64 * kRowWaves), 0, s, planes, K, H, W, o->cls, P);
    int rc = launch_components(lb, P, Q, H, W);
    if (rc) return rc;
    launch_count(lb, P, Q, npix, o->min_area, lb->d_n);
    hipLaunchKernelGGL(label_number_kernel, dim3((unsigned)nblocks), dim3(64 * kScanWaves), 0, s, P, Q, npix, o->min_area, lb->d_counts);
    long long n = 0;
    if ((rc = read_count_and_init_table(lb, npix, &n))) return rc;
    if (o->grow_radius == 0) {
        hipLaunchKernelGGL(label_write_kernel, dim3(row_grid(H)), dim3(64 * kRowWaves), 0, s, P, Q, H, W, out, lb->d_table);
    } else {
        // the seeds into P; Q is free from here on
        hipLaunchKernelGGL(label_seed_kernel, dim3(pix_grid), dim3(kPixThreads), 0, s, P, Q, npix);
        launch_grow_and_table(lb, planes, K, H, W, o, P, Q, out);
    }
    L_HIP(lb, hipGetLastError());
    *n_out = n;
    return UMX_OK;
}

// The flood from the seed labels in *src, with *dst as the other plane; on return *src holds the
// flooded labels.  `pending`: the pixels of kept objects that are no seed pixels -- what there is to claim.
//   At a level t the host launches label_flood_kernel (8 steps each, src -> dst -> src ...) until a launch claims nothing: the state
//   is closed under the steps of that level.  After every launch one 16-byte read-back: the pixels claimed so far and the launch's
//   least waiting relief.
//   In a launch that claimed nothing every workgroup's LDS state is the global state (its first step changed nothing anywhere: a
//   halo pixel that one workgroup could claim is a tile pixel that its owner would claim and count), so the least-relief word m of
//   that launch -- and of no other -- is exact: the least r > t over the empty pixels of class cls beside a labelled pixel.  No pixel
//   can be claimed at a level below m: a level t' < m admits no pixel beside a label, so its first step claims nothing.  The flood
//   continues at the first level t_j >= m, j = m / q; the levels in between would each cost one launch and change nothing.
//   No candidate (the word is untouched), or every pending pixel claimed: the flood is over.
// Every launch but the last of a level claims a pixel or more, so there are at most pending + 256 / q launches.
int run_flood_launches(umx_labeler* lb, const uint8_t* planes, int K, int H, int W, const umx_label_flood_options* fo, int** src, int** dst,
                       long long pending, umx_label_flood_counts* fc) {
    const int tiles_x = (W - 1) / kGrowTile + 1, tiles_y = (H - 1) / kGrowTile + 1;
    const dim3 tile_grid((unsigned)tiles_y * (unsigned)tiles_x);
    hipStream_t s = lb->stream;
    const int q = fo->level_step, nlevels = UMX_FLOOD_MAX_STEP / q;
    long long claimed = 0, levels_claimed = 0, launches = 0;
    for (int j = 0; j < nlevels && claimed < pending;) {
        const int t = std::min(255, (j + 1) * q - 1);
        long long words[kFloodWords] = {0, 0};
        bool level_claimed = false;
        for (;;) {
            L_HIP(lb, hipMemsetAsync(lb->d_flood + kFloodLeast, kFloodNone & 0xff, sizeof(long long), s));
            hipLaunchKernelGGL(label_flood_kernel, tile_grid, dim3(kGrowThreads), 0, s, planes, K, H, W, fo->split.base.cls, fo->relief_plane,
                               fo->invert, t, (const int*)*src, *dst, kGrowHalo, tiles_x, lb->d_flood + kFloodClaimed,
                               reinterpret_cast<int*>(lb->d_flood + kFloodLeast));
            std::swap(*src, *dst);
            ++launches;
            L_HIP(lb, hipGetLastError());
            L_HIP(lb, hipMemcpyAsync(words, lb->d_flood, sizeof words, hipMemcpyDeviceToHost, s));
            L_HIP(lb, hipStreamSynchronize(s));
            const long long now = words[kFloodClaimed];
            if (now < claimed || now > pending) return lfail(lb, UMX_ERR_HIP, "the flood claimed %lld of %lld pixels", now, pending);
            if (now == claimed) break;
            claimed = now;
            level_claimed = true;
            if (claimed == pending) break;
        }
        levels_claimed += level_claimed;
        if (claimed == pending) break;
        const int m = (int)(words[kFloodLeast] & 0xffffffffll);   // of a launch that claimed nothing
        if (m == kFloodNone) break;
        if (m <= t || m > 255) return lfail(lb, UMX_ERR_HIP, "the flood reported a waiting relief of %d at level %d", m, t);
        j = m / q;                                            // t_j = (j + 1) q - 1 >= m > t: a later level
    }
    fc->unreached = pending - claimed; fc->levels_claimed = levels_claimed; fc->claimed = claimed; fc->launches = launches;
    return UMX_OK;
}

// The launches of a split run, in the same frame as run_launches:
//   the objects as there up to label_area_kernel: P = roots, Q = areas; label_count / _scan_kernel: N0 to a word of its own
//   label_erode_kernel        B = kept | eroded per pixel (the last reader of the objects' areas)
//   label_runs_mask_kernel    E's row runs into R; strip, seams, heads, flatten, area as for the objects: R = roots of E's components,
//                             Q = their areas
//   label_core_mark_kernel    kFlagCored at the root of every object that holds a core
//   label_split_ids_kernel    the seed components' ids in place over P; label_count / _scan / _number_kernel number them (min_area 0)
//   (N, N0 and the counts come back to the host; the table is sized for N)
//   label_seed_kernel         the seed labels in place over P; Q and R are free from here on
//   label_grow_kernel<true>   the regrow over class cls, P -> Q -> P ..., up to ceil(L / 8) launches; after each one the host reads the
//                             number of pixels claimed so far and stops when a launch claimed none: the state is closed -- nothing but
//                             these launches changes it -- so every later level would claim nothing either
//   the rim growth and label_grown_kernel as in run_launches
// A flood run (fo: its options, so == &fo->split; fc takes its counts) has run_flood_launches in the regrow's place.
// An h-maxima run (ho: its options, fo == &ho->flood; hc takes seed_pixels and recon_launches) is a flood run with launch_hmax_seeds
// (umx_label_hmax.hip: the relief, two reconstructions, the mark; steps 33 to 35) in the place of the label_erode_kernel launch.
int run_split_launches(umx_labeler* lb, const uint8_t* planes, int K, int H, int W, const umx_label_split_options* so, int* out,
                       umx_label_split_counts* counts, const umx_label_flood_options* fo = nullptr, umx_label_flood_counts* fc = nullptr,
                       const umx_label_hmax_options* ho = nullptr, umx_label_hmax_counts* hc = nullptr) {
    const umx_label_options* o = &so->base;
    const long long npix = (long long)H * W;
    const int nblocks = (int)((npix + kScanBlock - 1) / kScanBlock);
    const unsigned pix_grid = (unsigned)((npix + kPixThreads - 1) / kPixThreads);
    const int tiles_x = (W - 1) / kGrowTile + 1, tiles_y = (H - 1) / kGrowTile + 1;
    const dim3 tile_grid((unsigned)tiles_y * (unsigned)tiles_x);
    hipStream_t s = lb->stream;
    int *P = lb->d_P, *Q = lb->d_Q, *R = lb->d_R;
    uint8_t* B = lb->d_B;
    L_HIP(lb, hipMemsetAsync(lb->d_split, 0, kSplitWords * sizeof(long long), s));
    if (fo) L_HIP(lb, hipMemsetAsync(lb->d_flood, 0, kFloodWords * sizeof(long long), s));
    hipLaunchKernelGGL(label_runs_kernel, dim3(row_grid(H)), dim3(64 * kRowWaves), 0, s, planes, K, H, W, o->cls, P);
    int rc = launch_components(lb, P, Q, H, W);
    if (rc) return rc;
    launch_count(lb, P, Q, npix, o->min_area, lb->d_split + kSplitBefore);
    if (ho) {
        if ((rc = launch_hmax_seeds(lb, planes, H, W, P, Q, o->min_area, ho, hc->recon_launches))) return rc;
    } else {
        hipLaunchKernelGGL(label_erode_kernel, tile_grid, dim3(kGrowThreads), 0, s, P, Q, H, W, o->min_area, so->depth, tiles_x, B);
    }
    hipLaunchKernelGGL(label_runs_mask_kernel, dim3(row_grid(H)), dim3(64 * kRowWaves), 0, s, B, H, W, R);
    if ((rc = launch_components(lb, R, Q, H, W))) return rc;
    hipLaunchKernelGGL(label_core_mark_kernel, dim3(pix_grid), dim3(kPixThreads), 0, s, P, R, Q, npix, so->core_min_area, B);
    hipLaunchKernelGGL(label_split_ids_kernel, dim3((unsigned)nblocks), dim3(kPixThreads), 0, s, P, R, Q, B, npix, so->core_min_area,
                       reinterpret_cast<unsigned long long*>(lb->d_split + kSplitPacked));
    launch_count(lb, P, Q, npix, 0, lb->d_n);
    hipLaunchKernelGGL(label_number_kernel, dim3((unsigned)nblocks), dim3(64 * kScanWaves), 0, s, P, Q, npix, 0, lb->d_counts);
    long long words[kSplitWords] = {0, 0, 0, 0};
    L_HIP(lb, hipMemcpyAsync(words, lb->d_split, sizeof words, hipMemcpyDeviceToHost, s));
    long long seed_pixels = 0;
    if (ho) L_HIP(lb, hipMemcpyAsync(&seed_pixels, lb->d_hmax + kHmaxSeeds, sizeof seed_pixels, hipMemcpyDeviceToHost, s));
    long long n = 0;
    if ((rc = read_count_and_init_table(lb, npix, &n))) return rc;
    if (seed_pixels < 0 || seed_pixels > npix) return lfail(lb, UMX_ERR_HIP, "the h-maxima counted %lld seed pixels in %lld pixels", seed_pixels, npix);
    if (ho) hc->seed_pixels = seed_pixels;
    const long long n_before = words[kSplitBefore], n_cored = words[kSplitPacked] & 0xffffffffll;
    const long long pending = (long long)((unsigned long long)words[kSplitPacked] >> 32);
    if (n_before < 0 || n_before > n || n_cored > n_before || pending > npix)
        return lfail(lb, UMX_ERR_HIP, "the split counted %lld objects before, %lld cored, %lld after and %lld pixels to regrow in %lld pixels",
                     n_before, n_cored, n, pending, npix);
    hipLaunchKernelGGL(label_seed_kernel, dim3(pix_grid), dim3(kPixThreads), 0, s, P, Q, npix);
    int *src = P, *dst = Q;
    long long claimed = 0;
    if (fo) {
        if ((rc = run_flood_launches(lb, planes, K, H, W, fo, &src, &dst, pending, fc))) return rc;
        claimed = fc->claimed;
    }
    for (int left = fo ? 0 : so->regrow; left > 0 && claimed < pending; left -= kGrowHalo) {
        hipLaunchKernelGGL(label_grow_kernel<true>, tile_grid, dim3(kGrowThreads), 0, s, planes, K, H, W, 1u << o->cls, src, dst,
                           std::min(left, kGrowHalo), tiles_x, lb->d_split + kSplitClaimed, 0);
        std::swap(src, dst);
        L_HIP(lb, hipGetLastError());
        long long now = 0;
        L_HIP(lb, hipMemcpyAsync(&now, lb->d_split + kSplitClaimed, sizeof now, hipMemcpyDeviceToHost, s));
        L_HIP(lb, hipStreamSynchronize(s));
        if (now < claimed || now > pending) return lfail(lb, UMX_ERR_HIP, "the regrow claimed %lld of %lld pixels", now, pending);
        if (now == claimed) break;
        claimed = now;
    }
    launch_grow_and_table(lb, planes, K, H, W, o, src, dst, out);
    L_HIP(lb, hipGetLastError());
    counts->n_objects = n; counts->n_before = n_before; counts->n_cored = n_cored; counts->unreached = pending - claimed;
    return UMX_OK;
}

// split: a split run -- so holds its options (o is not looked at) and counts takes the four counts.  fo: a flood run -- its options
// (then split is set and so is &fo->split) and fcounts takes its counts, the four of the split among them.  ho: an h-maxima run -- its
// options (then fo is &ho->flood) and hcounts takes its counts, the flood's among them (fcounts is not used).
int run_any(umx_labeler* lb, const uint8_t* planes, bool on_host, int K, int H, int W, const umx_label_options* o, int32_t* labels,
            int64_t* n_objects, bool split = false, const umx_label_split_options* so = nullptr, umx_label_split_counts* counts = nullptr,
            const umx_label_flood_options* fo = nullptr, umx_label_flood_counts* fcounts = nullptr,
            const umx_label_hmax_options* ho = nullptr, umx_label_hmax_counts* hcounts = nullptr) {
    if (!lb) return lfail(nullptr, UMX_ERR_INVALID, "null labeler");
    char msg[200];
    const int refused = ho ? umx_label_hmax_check(ho, K, H, W, msg, sizeof msg)
                           : fo ? umx_label_flood_check(fo, K, H, W, msg, sizeof msg)
                           : split ? umx_label_split_check(so, K, H, W, msg, sizeof msg) : umx_label_options_check(o, K, H, W, msg, sizeof msg);
    if (refused != UMX_OK) return lfail(lb, UMX_ERR_INVALID, "%s", msg);
    if (!planes) return lfail(lb, UMX_ERR_INVALID, "null planes");
    L_HIP(lb, hipSetDevice(lb->device));
    const size_t npix = (size_t)H * W, plane_bytes = (size_t)K * npix;
    lb->res_why = "the last run of this labeler failed";       // from here on the arena may be emptied and d_P is overwritten
    int rc = ensure_buffers(lb, on_host ? plane_bytes : 0, npix, (npix + kScanBlock - 1) / kScanBlock, split);
    if (rc) return rc;
    hipStream_t s = lb->stream;
    lb->table.clear();
    lb->ms[0] = lb->ms[1] = lb->ms[2] = 0.0;
    L_HIP(lb, hipEventRecord(lb->ev[0], s));
    if (on_host) L_HIP(lb, hipMemcpyAsync(lb->d_planes, planes, plane_bytes, hipMemcpyHostToDevice, s));
    L_HIP(lb, hipEventRecord(lb->ev[1], s));
    long long n = 0;
    int* out = !labels ? nullptr : on_host ? lb->d_P : labels;
    umx_label_split_counts sc = {0, 0, 0, 0};
    umx_label_flood_counts fc = {0, 0, 0, 0, 0, 0, 0, 0};
    umx_label_hmax_counts hc = {fc, 0, {0, 0}, 0};
    if (split) {
        rc = run_split_launches(lb, on_host ? lb->d_planes : planes, K, H, W, so, out, &sc, fo, &fc, ho, &hc);
        n = sc.n_objects;
    } else {
        rc = run_launches(lb, on_host ? lb->d_planes : planes, K, H, W, o, out, &n);
    }
    if (rc) {
        (void)hipStreamSynchronize(s);
        return rc;
    }
    L_HIP(lb, hipEventRecord(lb->ev[2], s));
    if (on_host && labels) L_HIP(lb, hipMemcpyAsync(labels, lb->d_P, npix * sizeof(int), hipMemcpyDeviceToHost, s));
    lb->table.resize((size_t)n);
    if (n > 0) L_HIP(lb, hipMemcpyAsync(lb->table.data(), lb->d_table, (size_t)n * sizeof(umx_label_object), hipMemcpyDeviceToHost, s));
    L_HIP(lb, hipEventRecord(lb->ev[3], s));
    L_HIP(lb, hipStreamSynchronize(s));
    for (int k = 0; k < 3; ++k) {
        float f = 0.f;
        if (hipEventElapsedTime(&f, lb->ev[k], lb->ev[k + 1]) == hipSuccess) lb->ms[k] = f;
    }
    if (!on_host) lb->ms[0] = 0.0;
    std::string gmsg;
    if ((rc = arena_check(lb->mem, &gmsg)) != UMX_OK) return lfail(lb, rc, "%s", gmsg.c_str());
    if (n_objects) *n_objects = n;
    if (counts) *counts = sc;
    if (fcounts) {
        fc.n_objects = sc.n_objects; fc.n_before = sc.n_before; fc.n_cored = sc.n_cored;   // (unreached is the flood's own)
        *fcounts = fc;
    }
    if (hcounts) {
        fc.n_objects = sc.n_objects; fc.n_before = sc.n_before; fc.n_cored = sc.n_cored;
        hc.flood = fc;
        *hcounts = hc;
    }
    if (on_host && labels) { lb->res_H = H; lb->res_W = W; lb->res_N = n; lb->res_why = nullptr; }
    else lb->res_why = on_host ? "the last umx_labeler_run was given no label plane (labels_host was NULL)"
                               : "the last run was umx_labeler_run_dev, which leaves its labels with the caller: use umx_labeler_measure_dev";
    return UMX_OK;
}

template <typename T>
void launch_measure(hipStream_t s, int g, const int* labels, const void* planes, int H, int W, int N, umx_label_measure* rec) {
    const T* p = static_cast<const T*>(planes);
    const dim3 grid(row_grid(H)), block(64 * kRowWaves);
    switch (g) {
        case 1: hipLaunchKernelGGL((label_measure_kernel<T, 1>), grid, block, 0, s, labels, p, H, W, N, rec); break;
        case 2: hipLaunchKernelGGL((label_measure_kernel<T, 2>), grid, block, 0, s, labels, p, H, W, N, rec); break;
        case 3: hipLaunchKernelGGL((label_measure_kernel<T, 3>), grid, block, 0, s, labels, p, H, W, N, rec); break;
        default: hipLaunchKernelGGL((label_measure_kernel<T, 4>), grid, block, 0, s, labels, p, H, W, N, rec); break;
    }
}

// C planes against `labels` (device, H x W, objects 1..N), group by group of up to UMX_LABEL_MEASURE_GROUP planes: the group's planes
// up (on_host), its records cleared, one launch, its records down to out[c0 * N ...]; then the stream is idle.  At most
// ceil(1024 / 4) = 256 rounds.  The caller has checked the arguments; out holds C * N records.
int measure_any(umx_labeler* lb, const int* labels, long long N, const void* planes, bool on_host, int dtype, int C, int H, int W,
                umx_label_measure* out) {
    L_HIP(lb, hipSetDevice(lb->device));
    lb->mms[0] = lb->mms[1] = lb->mms[2] = 0.0;
    if (N == 0) return UMX_OK;
    const size_t npix = (size_t)H * W, esz = dtype == UMX_MEASURE_U16 ? 2 : 1;
    const int gmax = std::min(C, (int)UMX_LABEL_MEASURE_GROUP);
    int rc = on_host ? ensure_measure_buffer(lb, &lb->d_mplanes, &lb->mplanes_cap, (size_t)gmax * npix * esz, 1, "measure planes") : UMX_OK;
    if (rc) return rc;
    if ((rc = ensure_measure_buffer(lb, &lb->d_mrec, &lb->mrec_cap, (size_t)gmax * (size_t)N, sizeof(umx_label_measure), "measure records"))) return rc;
    hipStream_t s = lb->stream;
    for (int c0 = 0; c0 < C; c0 += UMX_LABEL_MEASURE_GROUP) {
        const int g = std::min(C - c0, (int)UMX_LABEL_MEASURE_GROUP);
        const char* src = static_cast<const char*>(planes) + (size_t)c0 * npix * esz;
        const long long nrec = (long long)g * N;
        L_HIP(lb, hipEventRecord(lb->ev[0], s));
        if (on_host) L_HIP(lb, hipMemcpyAsync(lb->d_mplanes, src, (size_t)g * npix * esz, hipMemcpyHostToDevice, s));
        L_HIP(lb, hipEventRecord(lb->ev[1], s));
        hipLaunchKernelGGL(label_measure_init_kernel, dim3((unsigned)((nrec + kPixThreads - 1) / kPixThreads)), dim3(kPixThreads), 0, s,
                           lb->d_mrec, nrec);
        const void* dev = on_host ? lb->d_mplanes : src;
        if (dtype == UMX_MEASURE_U16) launch_measure<uint16_t>(s, g, labels, dev, H, W, (int)N, lb->d_mrec);
        else launch_measure<uint8_t>(s, g, labels, dev, H, W, (int)N, lb->d_mrec);
        L_HIP(lb, hipGetLastError());
        L_HIP(lb, hipEventRecord(lb->ev[2], s));
        L_HIP(lb, hipMemcpyAsync(out + (size_t)c0 * (size_t)N, lb->d_mrec, (size_t)nrec * sizeof(umx_label_measure), hipMemcpyDeviceToHost, s));
        L_HIP(lb, hipEventRecord(lb->ev[3], s));
        L_HIP(lb, hipStreamSynchronize(s));
        for (int k = 0; k < 3; ++k) {
            float f = 0.f;
            if (hipEventElapsedTime(&f, lb->ev[k], lb->ev[k + 1]) == hipSuccess && (k > 0 || on_host)) lb->mms[k] += f;
        }
    }
    std::string gmsg;
    if ((rc = arena_check(lb->mem, &gmsg)) != UMX_OK) return lfail(lb, rc, "%s", gmsg.c_str());
    return UMX_OK;
}

// The shapes of `labels` (device, H x W, objects 1..N): the records cleared, one launch, the records down to out; then the stream is
// idle.  The caller has checked the arguments; out holds N records.
int shape_any(umx_labeler* lb, const int* labels, long long N, int H, int W, umx_label_shape* out) {
    L_HIP(lb, hipSetDevice(lb->device));
    lb->sms[0] = lb->sms[1] = 0.0;
    if (N == 0) return UMX_OK;
    int rc = ensure_measure_buffer(lb, &lb->d_srec, &lb->srec_cap, (size_t)N, sizeof(umx_label_shape), "shape records");
    if (rc) return rc;
    hipStream_t s = lb->stream;
    L_HIP(lb, hipEventRecord(lb->ev[1], s));
    hipLaunchKernelGGL(label_shape_init_kernel, dim3((unsigned)((N + kPixThreads - 1) / kPixThreads)), dim3(kPixThreads), 0, s, lb->d_srec, N);
    hipLaunchKernelGGL(label_shape_kernel, dim3(row_grid(H)), dim3(64 * kRowWaves), 0, s, labels, H, W, (int)N, lb->d_srec);
    L_HIP(lb, hipGetLastError());
    L_HIP(lb, hipEventRecord(lb->ev[2], s));
    L_HIP(lb, hipMemcpyAsync(out, lb->d_srec, (size_t)N * sizeof(umx_label_shape), hipMemcpyDeviceToHost, s));
    L_HIP(lb, hipEventRecord(lb->ev[3], s));
    L_HIP(lb, hipStreamSynchronize(s));
    for (int k = 0; k < 2; ++k) {
        float f = 0.f;
        if (hipEventElapsedTime(&f, lb->ev[k + 1], lb->ev[k + 2]) == hipSuccess) lb->sms[k] = f;
    }
    std::string gmsg;
    if ((rc = arena_check(lb->mem, &gmsg)) != UMX_OK) return lfail(lb, rc, "%s", gmsg.c_str());
    return UMX_OK;
}

}  // namespace

void launch_grow_free(hipStream_t s, int H, int W, int N, const int* src, int* dst, int levels) {
    const int tiles_x = (W - 1) / kGrowTile + 1, tiles_y = (H - 1) / kGrowTile + 1;   // tiles_y * tiles_x <= 2^25 + 2^19: H * W <= INT_MAX
    hipLaunchKernelGGL((label_grow_kernel<false, true>), dim3((unsigned)tiles_y * (unsigned)tiles_x), dim3(kGrowThreads), 0, s,
                       (const uint8_t*)nullptr, 0, H, W, 0u, src, dst, levels, tiles_x, (long long*)nullptr, N);
}

void launch_block_scan(hipStream_t s, int* counts, int nblocks, long long* total) {
    hipLaunchKernelGGL(label_scan_kernel, dim3(1), dim3(kMergeThreads), 0, s, counts, nblocks, total);
}

}  // namespace umx

using namespace umx;

extern "C" {

int umx_label_options_check(const umx_label_options* o, int K, int H, int W, char* msg, size_t cap) {
    char buf[200] = "";
    if (!o) snprintf(buf, sizeof buf, "null label options");
    else if (H < 1 || W < 1) snprintf(buf, sizeof buf, "the image is %d x %d: both sides must be at least 1", H, W);
    else if ((long long)H * W > INT_MAX)
        snprintf(buf, sizeof buf, "the image is %d x %d: a flat pixel index is an int32, so H * W may be at most %d", H, W, INT_MAX);
    else if (K < 1 || K > UMX_LABEL_MAX_CLASSES) snprintf(buf, sizeof buf, "there are %d planes: 1..%d classes", K, UMX_LABEL_MAX_CLASSES);
    else if (o->cls < 0 || o->cls >= K) snprintf(buf, sizeof buf, "cls is %d: the class is 0..%d, in the model's class order", o->cls, K - 1);
    else if (o->min_area < 1 || o->min_area > UMX_LABEL_MAX_MIN_AREA)
        snprintf(buf, sizeof buf, "min_area is %d: it must be 1..%d pixels", o->min_area, UMX_LABEL_MAX_MIN_AREA);
    // (grow_radius and grow_classes were reserved words: a caller that set one of them alone is told so as well)
    else if (o->grow_radius < 0 || o->grow_radius > UMX_LABEL_MAX_GROW)
        snprintf(buf, sizeof buf, "grow_radius is %d: 0 (no growth) or 1..%d levels", o->grow_radius, (int)UMX_LABEL_MAX_GROW);
    else if (o->grow_radius > 0 && o->grow_classes == 0)
        snprintf(buf, sizeof buf, "grow_radius is %d and grow_classes is empty: a growth needs a class to grow over (both were reserved words: "
                                  "both zero is no growth)", o->grow_radius);
    else if (o->grow_radius == 0 && o->grow_classes != 0)
        snprintf(buf, sizeof buf, "grow_classes is 0x%x and grow_radius is 0: without a growth the class word must be zero (it was a reserved "
                                  "word)", o->grow_classes);
    else if (K < 32 && (o->grow_classes >> K) != 0)
        snprintf(buf, sizeof buf, "grow_classes is 0x%x: a bit at or above %d, and the classes are 0..%d", o->grow_classes, K, K - 1);
    for (int i = 0; o && !buf[0] && i < 4; ++i)
        if (o->reserved[i]) snprintf(buf, sizeof buf, "reserved must be zero");
    if (msg && cap) snprintf(msg, cap, "%s", buf);
    return buf[0] ? UMX_ERR_INVALID : UMX_OK;
}

int umx_labeler_create(int device_ordinal, umx_labeler** out) {
    if (!out) return lfail(nullptr, UMX_ERR_INVALID, "null output pointer");
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1)
        return lfail(nullptr, UMX_ERR_NO_DEVICE, "no HIP device available (libumx has no CPU fallback)");
    if (device_ordinal < 0 || device_ordinal >= ndev)
        return lfail(nullptr, UMX_ERR_INVALID, "device ordinal %d out of range (%d devices)", device_ordinal, ndev);
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device_ordinal) != hipSuccess) return lfail(nullptr, UMX_ERR_HIP, "hipGetDeviceProperties failed");
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return lfail(nullptr, UMX_ERR_NO_DEVICE, "device %d is %s; libumx is built for gfx950 only", device_ordinal, prop.gcnArchName);
    std::unique_ptr<umx_labeler> lb(new umx_labeler());
    lb->device = device_ordinal;
    std::string why;
    int rc = arena_init(&lb->mem, &why);
    if (rc) return lfail(nullptr, rc, "%s", why.c_str());
    L_HIP(nullptr, hipSetDevice(device_ordinal));
    hipError_t e = hipStreamCreateWithFlags(&lb->stream, hipStreamNonBlocking);
    for (int k = 0; k < 4 && e == hipSuccess; ++k) e = hipEventCreate(&lb->ev[k]);
    if (e != hipSuccess) {
        umx_labeler_destroy(lb.release());
        return lfail(nullptr, UMX_ERR_HIP, "creating the labeler's stream and events failed: %s", hipGetErrorString(e));
    }
    *out = lb.release();
    return UMX_OK;
}

void umx_labeler_destroy(umx_labeler* lb) {
    if (!lb) return;
    (void)hipSetDevice(lb->device);
    if (lb->stream) (void)hipStreamSynchronize(lb->stream);
    arena_free(&lb->mem);
    for (hipEvent_t ev : lb->ev)
        if (ev) (void)hipEventDestroy(ev);
    if (lb->stream) (void)hipStreamDestroy(lb->stream);
    delete lb;
}

const char* umx_labeler_last_error(const umx_labeler* lb) { return lb ? lb->err.c_str() : g_err.c_str(); }

int umx_labeler_run(umx_labeler* lb, const uint8_t* planes_host, int K, int H, int W, const umx_label_options* o, int32_t* labels_host,
                    int64_t* n_objects) {
    return run_any(lb, planes_host, true, K, H, W, o, labels_host, n_objects);
}

int umx_labeler_run_dev(umx_labeler* lb, const uint8_t* planes_dev, int K, int H, int W, const umx_label_options* o, int32_t* labels_dev,
                        int64_t* n_objects) {
    return run_any(lb, planes_dev, false, K, H, W, o, labels_dev, n_objects);
}

int umx_label_split_check(const umx_label_split_options* o, int K, int H, int W, char* msg, size_t cap) {
    char buf[200] = "";
    if (!o) snprintf(buf, sizeof buf, "null label split options");
    else if (umx_label_options_check(&o->base, K, H, W, buf, sizeof buf) != UMX_OK) {}   // (its words, unchanged)
    else if (o->depth < 1 || o->depth > UMX_SPLIT_MAX_DEPTH)
        snprintf(buf, sizeof buf, "depth is %d: the split erodes 1..%d levels", o->depth, (int)UMX_SPLIT_MAX_DEPTH);
    else if (o->core_min_area < 1 || o->core_min_area > UMX_SPLIT_MAX_CORE_AREA)
        snprintf(buf, sizeof buf, "core_min_area is %d: it must be 1..%d pixels", o->core_min_area, (int)UMX_SPLIT_MAX_CORE_AREA);
    else if (o->regrow < 1 || o->regrow > UMX_SPLIT_MAX_REGROW)
        snprintf(buf, sizeof buf, "regrow is %d: it must be 1..%d levels", o->regrow, (int)UMX_SPLIT_MAX_REGROW);
    for (int i = 0; o && !buf[0] && i < 5; ++i)
        if (o->reserved[i]) snprintf(buf, sizeof buf, "reserved must be zero (word %d of the split's reserved words is %d)", i, o->reserved[i]);
    if (msg && cap) snprintf(msg, cap, "%s", buf);
    return buf[0] ? UMX_ERR_INVALID : UMX_OK;
}

int umx_labeler_run_split(umx_labeler* lb, const uint8_t* planes_host, int K, int H, int W, const umx_label_split_options* o,
                          int32_t* labels_host, umx_label_split_counts* counts) {
    return run_any(lb, planes_host, true, K, H, W, nullptr, labels_host, nullptr, true, o, counts);
}

int umx_labeler_run_split_dev(umx_labeler* lb, const uint8_t* planes_dev, int K, int H, int W, const umx_label_split_options* o,
                              int32_t* labels_dev, umx_label_split_counts* counts) {
    return run_any(lb, planes_dev, false, K, H, W, nullptr, labels_dev, nullptr, true, o, counts);
}

int umx_label_flood_check(const umx_label_flood_options* o, int K, int H, int W, char* msg, size_t cap) {
    char buf[200] = "";
    if (!o) snprintf(buf, sizeof buf, "null label flood options");
    else if (umx_label_split_check(&o->split, K, H, W, buf, sizeof buf) != UMX_OK) {}   // (its words, unchanged)
    else if (o->split.regrow != UMX_SPLIT_MAX_REGROW)
        snprintf(buf, sizeof buf, "regrow is %d: the flood's steps have no bound, so a flood call must name %d", o->split.regrow,
                 (int)UMX_SPLIT_MAX_REGROW);
    else if (o->relief_plane < 0 || o->relief_plane >= K)
        snprintf(buf, sizeof buf, "relief_plane is %d: the plane is 0..%d, in the model's class order", o->relief_plane, K - 1);
    else if (o->invert != 0 && o->invert != 1) snprintf(buf, sizeof buf, "invert is %d: 0 or 1", o->invert);
    else if (o->level_step < 1 || o->level_step > UMX_FLOOD_MAX_STEP || (o->level_step & (o->level_step - 1)) != 0)
        snprintf(buf, sizeof buf, "level_step is %d: a power of two, 1..%d", o->level_step, (int)UMX_FLOOD_MAX_STEP);
    for (int i = 0; o && !buf[0] && i < 5; ++i)
        if (o->reserved[i]) snprintf(buf, sizeof buf, "reserved must be zero (word %d of the flood's reserved words is %d)", i, o->reserved[i]);
    if (msg && cap) snprintf(msg, cap, "%s", buf);
    return buf[0] ? UMX_ERR_INVALID : UMX_OK;
}

int umx_labeler_run_flood(umx_labeler* lb, const uint8_t* planes_host, int K, int H, int W, const umx_label_flood_options* o,
                          int32_t* labels_host, umx_label_flood_counts* counts) {
    if (lb && !o) return lfail(lb, UMX_ERR_INVALID, "null label flood options");
    return run_any(lb, planes_host, true, K, H, W, nullptr, labels_host, nullptr, true, o ? &o->split : nullptr, nullptr, o, counts);
}

int umx_labeler_run_flood_dev(umx_labeler* lb, const uint8_t* planes_dev, int K, int H, int W, const umx_label_flood_options* o,
                              int32_t* labels_dev, umx_label_flood_counts* counts) {
    if (lb && !o) return lfail(lb, UMX_ERR_INVALID, "null label flood options");
    return run_any(lb, planes_dev, false, K, H, W, nullptr, labels_dev, nullptr, true, o ? &o->split : nullptr, nullptr, o, counts);
}

int umx_label_hmax_check(const umx_label_hmax_options* o, int K, int H, int W, char* msg, size_t cap) {
    char buf[200] = "";
    if (!o) snprintf(buf, sizeof buf, "null label h-maxima options");
    else if (umx_label_flood_check(&o->flood, K, H, W, buf, sizeof buf) != UMX_OK) {}   // (its words, unchanged)
    else if (o->seed_plane < 0 || o->seed_plane >= K)
        snprintf(buf, sizeof buf, "seed_plane is %d: the plane is 0..%d, in the model's class order", o->seed_plane, K - 1);
    else if (o->seed_invert != 0 && o->seed_invert != 1) snprintf(buf, sizeof buf, "seed_invert is %d: 0 or 1", o->seed_invert);
    else if (o->height < 1 || o->height > UMX_HMAX_MAX_HEIGHT)
        snprintf(buf, sizeof buf, "height is %d: a peak must stand 1..%d grey values above its saddle", o->height, (int)UMX_HMAX_MAX_HEIGHT);
    for (int i = 0; o && !buf[0] && i < 5; ++i)
        if (o->reserved[i]) snprintf(buf, sizeof buf, "reserved must be zero (word %d of the h-maxima's reserved words is %d)", i, o->reserved[i]);
    if (msg && cap) snprintf(msg, cap, "%s", buf);
    return buf[0] ? UMX_ERR_INVALID : UMX_OK;
}

int umx_labeler_run_hmax(umx_labeler* lb, const uint8_t* planes_host, int K, int H, int W, const umx_label_hmax_options* o,
                         int32_t* labels_host, umx_label_hmax_counts* counts) {
    if (lb && !o) return lfail(lb, UMX_ERR_INVALID, "null label h-maxima options");
    return run_any(lb, planes_host, true, K, H, W, nullptr, labels_host, nullptr, true, o ? &o->flood.split : nullptr, nullptr,
                   o ? &o->flood : nullptr, nullptr, o, counts);
}

int umx_labeler_run_hmax_dev(umx_labeler* lb, const uint8_t* planes_dev, int K, int H, int W, const umx_label_hmax_options* o,
                             int32_t* labels_dev, umx_label_hmax_counts* counts) {
    if (lb && !o) return lfail(lb, UMX_ERR_INVALID, "null label h-maxima options");
    return run_any(lb, planes_dev, false, K, H, W, nullptr, labels_dev, nullptr, true, o ? &o->flood.split : nullptr, nullptr,
                   o ? &o->flood : nullptr, nullptr, o, counts);
}

int umx_labeler_objects(const umx_labeler* lb, umx_label_object* out, int64_t cap, int64_t* n) {
    if (!lb || cap < 0 || (cap > 0 && !out)) return lfail(nullptr, UMX_ERR_INVALID, "umx_labeler_objects: null labeler, or a capacity without a buffer");
    const int64_t have = (int64_t)lb->table.size(), m = std::min(cap, have);
    if (m > 0) memcpy(out, lb->table.data(), (size_t)m * sizeof(umx_label_object));
    if (n) *n = have;
    return UMX_OK;
}

int umx_labeler_last_ms(const umx_labeler* lb, double* upload_ms, double* kernel_ms, double* download_ms) {
    if (!lb) return lfail(nullptr, UMX_ERR_INVALID, "null labeler");
    if (upload_ms) *upload_ms = lb->ms[0];
    if (kernel_ms) *kernel_ms = lb->ms[1];
    if (download_ms) *download_ms = lb->ms[2];
    return UMX_OK;
}

int umx_label_measure_check(int dtype, int C, int H, int W, int64_t n_objects, char* msg, size_t cap) {
    char buf[200] = "";
    if (dtype != UMX_MEASURE_U8 && dtype != UMX_MEASURE_U16)
        snprintf(buf, sizeof buf, "dtype is %d: UMX_MEASURE_U8 (%d) or UMX_MEASURE_U16 (%d)", dtype, UMX_MEASURE_U8, UMX_MEASURE_U16);
    else if (C < 1 || C > UMX_LABEL_MAX_MEASURE_PLANES) snprintf(buf, sizeof buf, "there are %d planes: 1..%d", C, (int)UMX_LABEL_MAX_MEASURE_PLANES);
    else if (H < 1 || W < 1) snprintf(buf, sizeof buf, "the image is %d x %d: both sides must be at least 1", H, W);
    else if ((long long)H * W > INT_MAX)
        snprintf(buf, sizeof buf, "the image is %d x %d: a flat pixel index is an int32, so H * W may be at most %d", H, W, INT_MAX);
    else if (n_objects < 0 || n_objects > INT_MAX)
        snprintf(buf, sizeof buf, "n_objects is %lld: a label is an int32, so 0..%d objects", (long long)n_objects, INT_MAX);
    if (msg && cap) snprintf(msg, cap, "%s", buf);
    return buf[0] ? UMX_ERR_INVALID : UMX_OK;
}

int umx_labeler_measure(umx_labeler* lb, const void* planes_host, int dtype, int C, int H, int W, umx_label_measure* out, int64_t cap,
                        int64_t* n) {
    if (!lb) return lfail(nullptr, UMX_ERR_INVALID, "null labeler");
    char msg[200];
    if (umx_label_measure_check(dtype, C, H, W, 0, msg, sizeof msg) != UMX_OK) return lfail(lb, UMX_ERR_INVALID, "%s", msg);
    if (lb->res_why) return lfail(lb, UMX_ERR_INVALID, "umx_labeler_measure has no labels to measure against: %s", lb->res_why);
    if (H != lb->res_H || W != lb->res_W)
        return lfail(lb, UMX_ERR_INVALID, "the planes are %d x %d and the labels of the last run %d x %d", H, W, lb->res_H, lb->res_W);
    const long long N = lb->res_N;
    if (n) *n = N;
    if (!out && cap == 0) return UMX_OK;                  // the count alone, like umx_labeler_objects
    if (!out || cap < (long long)C * N)
        return lfail(lb, UMX_ERR_INVALID, "out holds %lld records: %d planes of %lld objects need %lld", out ? (long long)cap : 0ll, C, N,
                     (long long)C * N);
    if (!planes_host) return lfail(lb, UMX_ERR_INVALID, "null planes");
    return measure_any(lb, lb->d_P, N, planes_host, true, dtype, C, H, W, out);
}

int umx_labeler_measure_dev(umx_labeler* lb, const int32_t* labels_dev, int64_t n_objects, const void* planes_dev, int dtype, int C, int H,
                            int W, umx_label_measure* out_host, int64_t cap) {
    if (!lb) return lfail(nullptr, UMX_ERR_INVALID, "null labeler");
    char msg[200];
    if (umx_label_measure_check(dtype, C, H, W, n_objects, msg, sizeof msg) != UMX_OK) return lfail(lb, UMX_ERR_INVALID, "%s", msg);
    if (!labels_dev || !planes_dev) return lfail(lb, UMX_ERR_INVALID, "null labels or planes");
    if (cap < (long long)C * n_objects || (!out_host && n_objects > 0))
        return lfail(lb, UMX_ERR_INVALID, "out_host holds %lld records: %d planes of %lld objects need %lld", out_host ? (long long)cap : 0ll,
                     C, (long long)n_objects, (long long)C * n_objects);
    return measure_any(lb, labels_dev, n_objects, planes_dev, false, dtype, C, H, W, out_host);
}

int umx_labeler_measure_last_ms(const umx_labeler* lb, double* upload_ms, double* kernel_ms, double* download_ms) {
    if (!lb) return lfail(nullptr, UMX_ERR_INVALID, "null labeler");
    if (upload_ms) *upload_ms = lb->mms[0];
    if (kernel_ms) *kernel_ms = lb->mms[1];
    if (download_ms) *download_ms = lb->mms[2];
    return UMX_OK;
}

int umx_label_shape_check(int H, int W, int64_t n_objects, char* msg, size_t cap) {
    char buf[200] = "";
    if (H < 1 || W < 1) snprintf(buf, sizeof buf, "the image is %d x %d: both sides must be at least 1", H, W);
    else if (H > UMX_SHAPE_MAX_SIDE || W > UMX_SHAPE_MAX_SIDE)
        snprintf(buf, sizeof buf, "the image is %d x %d: a side may be at most %d, so that the square of a coordinate stays below 2^32", H, W,
                 UMX_SHAPE_MAX_SIDE);
    else if ((long long)H * W > INT_MAX)
        snprintf(buf, sizeof buf, "the image is %d x %d: a flat pixel index is an int32, so H * W may be at most %d", H, W, INT_MAX);
    else if (n_objects < 0 || n_objects > INT_MAX)
        snprintf(buf, sizeof buf, "n_objects is %lld: a label is an int32, so 0..%d objects", (long long)n_objects, INT_MAX);
    if (msg && cap) snprintf(msg, cap, "%s", buf);
    return buf[0] ? UMX_ERR_INVALID : UMX_OK;
}

int umx_labeler_shape(umx_labeler* lb, int H, int W, umx_label_shape* out, int64_t cap, int64_t* n) {
    if (!lb) return lfail(nullptr, UMX_ERR_INVALID, "null labeler");
    char msg[200];
    if (umx_label_shape_check(H, W, 0, msg, sizeof msg) != UMX_OK) return lfail(lb, UMX_ERR_INVALID, "%s", msg);
    if (lb->res_why) return lfail(lb, UMX_ERR_INVALID, "umx_labeler_shape has no labels to take the shapes of: %s", lb->res_why);
    if (H != lb->res_H || W != lb->res_W)
        return lfail(lb, UMX_ERR_INVALID, "the call names %d x %d and the labels of the last run are %d x %d", H, W, lb->res_H, lb->res_W);
    const long long N = lb->res_N;
    if (n) *n = N;
    if (!out && cap == 0) return UMX_OK;                  // the count alone, like umx_labeler_objects
    if (!out || cap < N)
        return lfail(lb, UMX_ERR_INVALID, "out holds %lld records: %lld objects need as many", out ? (long long)cap : 0ll, N);
    return shape_any(lb, lb->d_P, N, H, W, out);
}

int umx_labeler_shape_dev(umx_labeler* lb, const int32_t* labels_dev, int64_t n_objects, int H, int W, umx_label_shape* out_host,
                          int64_t cap) {
    if (!lb) return lfail(nullptr, UMX_ERR_INVALID, "null labeler");
    char msg[200];
    if (umx_label_shape_check(H, W, n_objects, msg, sizeof msg) != UMX_OK) return lfail(lb, UMX_ERR_INVALID, "%s", msg);
    if (!labels_dev) return lfail(lb, UMX_ERR_INVALID, "null labels");
    if (cap < n_objects || (!out_host && n_objects > 0))
        return lfail(lb, UMX_ERR_INVALID, "out_host holds %lld records: %lld objects need as many", out_host ? (long long)cap : 0ll,
                     (long long)n_objects);
    return shape_any(lb, labels_dev, n_objects, H, W, out_host);
}

int umx_labeler_shape_last_ms(const umx_labeler* lb, double* kernel_ms, double* download_ms) {
    if (!lb) return lfail(nullptr, UMX_ERR_INVALID, "null labeler");
    if (kernel_ms) *kernel_ms = lb->sms[0];
    if (download_ms) *download_ms = lb->sms[1];
    return UMX_OK;
}

}  // extern "C"
