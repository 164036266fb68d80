// libumx label mask: h-maxima seeds (include/umx.h, umx_labeler_run_hmax).  The producer of the
// seed set E of a split or flood run from a relief of the planes, in the place of the erosion: launch_hmax_seeds below is what
// run_split_launches (umx_label.hip) calls where it otherwise launches label_erode_kernel; everything after it is unchanged.
//
//   label_hmax_relief_kernel   one thread per pixel: "belongs to a kept object" (P = roots, Q = areas: the last reader of the objects'
//                              areas) as kFlagKept into B, the relief f and the marker max(f - h, 0) as bytes
//   label_recon_kernel         the grey-scale reconstruction by dilation, the growth kernel's geometry: one workgroup per tile of
//                              64 x 64 pixels, the tile and a halo of 8 of the mask and the marker in LDS, up to
//                              UMX_HMAX_LAUNCH_STEPS steps of g <- min(mask, max(g, g of the four neighbours)) there, its own tile to
//                              the other marker plane, the tile pixels it raised added to one word
//   label_hmax_mark_kernel     one thread per pixel: kFlagEroded into B where g > r; |E| to one word
//
// The byte planes live in the int32 plane R, which is free until label_runs_mask_kernel writes it: four planes of H * W bytes, the
// relief f, and three that the two reconstructions pass round (mask, ping, pong).  A row of a byte plane starts at a multiple of W,
// so words of four pixels are used only when W is a multiple of 4 (then every plane, every row and every region's first column are
// word-aligned); any other W goes byte by byte.
//
// Why the reconstruction needs no synchronous levels, unlike the growth: the operator T(g)(p) = min(mask(p), max(g(p), g(q): q a
// 4-neighbour of p)) is monotone and the state starts at the marker, which is below the reconstruction g* (the least fixed point of T
// above the marker).  By induction every value any workgroup ever holds is a lower bound of g*: it is the marker, a value another
// launch wrote, or T applied to lower bounds (a neighbour that the region does not hold counts as 0, which is a lower bound too), and
// T(lower bounds) <= T(g*) = g*.  Values only rise.  So a stale halo, steps that read a neighbour before or after its own update
// of the same step, and any number of inner steps change how fast the state rises and never where it ends: a launch in which NO
// tile pixel was raised has, at every pixel, T(state)(p) == state(p) against the global state (a tile pixel's four neighbours lie
// in its workgroup's region, and its first step saw them at their global values or higher ones), so the state is a fixed point
// above the marker and below g*: it is g*.  The final bytes do not depend on any order; the number of launches may.
// How fast: a value that must travel along a path reaches, in one launch, at least the next 8 pixels of the path -- each of them lies
// in a tile whose region holds the 8 pixels before it -- and up to UMX_HMAX_LAUNCH_STEPS of them while the path stays in one
// region.  UMX_HMAX_MAX_LAUNCHES * 8 > 10 000: a path of 10 000 pixels converges whatever its course.
// Synchronisation is the file's rule (umx_label.hip): in a launch a workgroup writes only bytes of its own tile in a plane that
// nobody reads in that launch; the only exception is integer atomics that nothing reads before the launch ends.  No flag, no spin:
// the inner loop's trip count is bounded by the step cap, the host's by UMX_HMAX_MAX_LAUNCHES.
#include "../../include/umx.h"
#include "umx_internal.h"
#include "umx_label_state.h"

namespace umx {

namespace {

constexpr int kPixThreads = 256;
constexpr int kTile = UMX_LABEL_GROW_TILE, kHalo = UMX_LABEL_GROW_HALO, kSide = kTile + 2 * kHalo;   // 64, 8, 80
constexpr int kThreads = 256;
constexpr int kRowWords = kSide / 4, kWords = kSide * kRowWords;                // the region as words of 4 pixels: 20 a row, 1600
constexpr int kTileRowWords = kTile / 4, kTileWords = kTile * kTileRowWords;    // the tile: 16 a row, 1024
constexpr int kRounds = (kWords + kThreads - 1) / kThreads;                     // 7 (the last one partly)
static_assert(kSide % 4 == 0 && kHalo % 4 == 0 && kTile % 4 == 0, "tile, halo and region are whole words of 4 pixels");
static_assert(kTileWords % kThreads == 0, "whole rounds over the tile");
static_assert(UMX_HMAX_LAUNCH_STEPS >= kHalo, "a launch carries a value at least a halo's width along any path");
static_assert((long long)UMX_HMAX_MAX_LAUNCHES * kHalo > 10000, "a path of 10 000 pixels converges");
static_assert((2 * kWords + kTileWords) * sizeof(unsigned) <= 20 * 1024, "eight reconstruction workgroups per CU by LDS");

// byte-wise max, min and saturating a - d of four pixels in a word
__device__ inline unsigned bmax4(unsigned a, unsigned b) {
    unsigned r = 0;
#pragma unroll
    for (int k = 0; k < 32; k += 8) r |= max((a >> k) & 0xffu, (b >> k) & 0xffu) << k;
    return r;
}
__device__ inline unsigned bmin4(unsigned a, unsigned b) {
    unsigned r = 0;
#pragma unroll
    for (int k = 0; k < 32; k += 8) r |= min((a >> k) & 0xffu, (b >> k) & 0xffu) << k;
    return r;
}
__device__ inline unsigned bsub4(unsigned a, unsigned d) {
    unsigned r = 0;
#pragma unroll
    for (int k = 0; k < 32; k += 8) {
        const unsigned v = (a >> k) & 0xffu;
        r |= (v > d ? v - d : 0u) << k;
    }
    return r;
}

// The four pixels (gy, gx .. gx + 3) of a byte plane as one word, pixel gx lowest; 0 for every pixel outside the image.  gx is a
// multiple of 4 (it may be negative).  aligned (W % 4 == 0): the word is wholly inside or wholly outside, and inside it is aligned.
// Bounds: a byte is touched at 0 <= gy < H, 0 <= gx + b < W only: flat index < H * W.
__device__ inline unsigned load4(const uint8_t* __restrict__ plane, int H, int W, long long gy, long long gx, bool aligned) {
    if (gy < 0 || gy >= H || gx >= W || gx + 3 < 0) return 0u;
    const size_t row = (size_t)gy * W;
    if (aligned) return *reinterpret_cast<const unsigned*>(plane + row + (size_t)gx);
    unsigned v = 0;
#pragma unroll
    for (int b = 0; b < 4; ++b)
        if (gx + b >= 0 && gx + b < W) v |= (unsigned)plane[row + (size_t)(gx + b)] << (8 * b);
    return v;
}

// one thread per pixel, i < npix.  P (roots, -1 off the objects), Q (areas at the roots) and the seed plane are only read; a thread
// writes B, F and M at its own pixel.  seed_plane < K (umx_label_hmax_check), so its byte is below K * H * W.
__global__ void __launch_bounds__(kPixThreads) label_hmax_relief_kernel(const uint8_t* __restrict__ planes, const int* __restrict__ P,
                                                                        const int* __restrict__ Q, long long npix, int min_area, int seed_plane,
                                                                        int invert, int h, uint8_t* __restrict__ B, uint8_t* __restrict__ F,
                                                                        uint8_t* __restrict__ M) {
    const long long i = (long long)blockIdx.x * kPixThreads + threadIdx.x;
    if (i >= npix) return;
    const int p = P[i];
    const bool kept = p >= 0 && Q[p] >= min_area;
    int f = 0;
    if (kept) {
        const int v = planes[(size_t)seed_plane * (size_t)npix + (size_t)i];
        f = invert ? 255 - v : v;
    }
    B[i] = kept ? (uint8_t)kFlagKept : (uint8_t)0;
    F[i] = (uint8_t)f;
    M[i] = (uint8_t)(f > h ? f - h : 0);
}

// Up to `steps` (1 .. UMX_HMAX_LAUNCH_STEPS) steps of the reconstruction by dilation of the marker in src under `mask`, src -> dst
// (three different byte planes of H x W; with dec > 0 the marker is max(mask - dec, 0) and src is never read: the first launch of the
// second reconstruction).  grid tiles_y * tiles_x, one workgroup per tile of 64 x 64 pixels: the mask and the marker of the tile and
// a halo of 8 into LDS as words of 4 pixels (0 outside the image), and the tile's marker once more, to count against.  A step: every
// thread takes its words whose marker is still below the mask, reads the words above and below and the bytes left and right of it,
// and writes min(mask, max of the five) back IN PLACE -- a neighbour may be read before or after its own update of this step: both
// are lower bounds (the head of the file) -- then one barrier that also tells whether any word rose; when none did the region is
// locally stable and the steps end.  The trip count is bounded by `steps`; the rest is the next launch's.
// A workgroup whose region has an all-zero mask, or whose marker equals its mask, has nothing to raise and skips the steps.
// *raised += the pixels of its own tile whose value it raised: one integer atomic per workgroup that raised any, which nothing reads
// before the launch ends.
// Bounds: region word w = j * 256 + thread < 1600 is checked (7 rounds cover 1792); its image row and first column are formed in
// 64 bits and a byte of mask / src / dst is touched at 0 <= gy < H, 0 <= gx < W only (load4 and the stores below).  A workgroup reads
// mask and src, which nobody writes in this launch, and writes the bytes of dst of its own tile only.
__global__ void __launch_bounds__(kThreads) label_recon_kernel(const uint8_t* __restrict__ mask, const uint8_t* __restrict__ src,
                                                               uint8_t* __restrict__ dst, int H, int W, int dec, int steps, int tiles_x,
                                                               unsigned long long* __restrict__ raised) {
    __shared__ unsigned Mk[kWords], G[kWords], G0[kTileWords];
    __shared__ unsigned tile_raised;
    const int tid = threadIdx.x;
    const long long ty = blockIdx.x / tiles_x, tx = blockIdx.x % tiles_x;
    const long long y0 = ty * kTile - kHalo, x0 = tx * kTile - kHalo;
    const bool aligned = (W & 3) == 0;
    if (tid == 0) tile_raised = 0;
    int open = 0;
    for (int j = 0; j < kRounds; ++j) {
        const int w = j * kThreads + tid;
        if (w >= kWords) break;
        const int ry = w / kRowWords, cx = w % kRowWords;
        const long long gy = y0 + ry, gx = x0 + 4 * cx;
        const unsigned m = load4(mask, H, W, gy, gx, aligned);
        const unsigned g = dec > 0 ? bsub4(m, (unsigned)dec) : load4(src, H, W, gy, gx, aligned);
        Mk[w] = m;
        G[w] = g;
        if (ry >= kHalo && ry < kHalo + kTile && cx >= kHalo / 4 && cx < (kHalo + kTile) / 4)
            G0[(ry - kHalo) * kTileRowWords + cx - kHalo / 4] = g;
        open |= g != m;
    }
    if (__syncthreads_or(open)) {                             // (the barrier that makes the LDS image whole, too)
        volatile unsigned* Gv = G;                            // words that other threads raise between two barriers
        for (int s = 0; s < steps; ++s) {
            int changed = 0;
            for (int j = 0; j < kRounds; ++j) {
                const int w = j * kThreads + tid;
                if (w >= kWords) break;
                const unsigned m = Mk[w], g = Gv[w];
                if (g == m) continue;
                const int ry = w / kRowWords, cx = w % kRowWords;
                const unsigned up = ry > 0 ? Gv[w - kRowWords] : 0u, down = ry < kSide - 1 ? Gv[w + kRowWords] : 0u;
                const unsigned lb = cx > 0 ? Gv[w - 1] >> 24 : 0u, rb = cx < kRowWords - 1 ? Gv[w + 1] & 0xffu : 0u;
                const unsigned left = (g << 8) | lb, right = (g >> 8) | (rb << 24);   // pixel b's left and right neighbours at byte b
                const unsigned n = bmin4(m, bmax4(bmax4(g, bmax4(up, down)), bmax4(left, right)));
                if (n != g) { Gv[w] = n; changed = 1; }
            }
            if (!__syncthreads_or(changed)) break;            // the same answer in every thread
        }
    }
    unsigned mine = 0;
#pragma unroll
    for (int j = 0; j < kTileWords / kThreads; ++j) {
        const int q = j * kThreads + tid;
        const int iy = q / kTileRowWords, ic = q % kTileRowWords;
        const long long gy = ty * kTile + iy, gx = tx * kTile + 4 * ic;
        if (gy >= H || gx >= W) continue;
        const unsigned g = G[(iy + kHalo) * kRowWords + ic + kHalo / 4], g0 = G0[q];
        const size_t at = (size_t)gy * W + (size_t)gx;
        if (aligned) {
            *reinterpret_cast<unsigned*>(dst + at) = g;
        } else {
#pragma unroll
            for (int b = 0; b < 4; ++b)
                if (gx + b < W) dst[at + b] = (uint8_t)(g >> (8 * b));
        }
#pragma unroll
        for (int b = 0; b < 32; b += 8) mine += ((g >> b) & 0xffu) != ((g0 >> b) & 0xffu);   // (outside the image both are 0)
    }
    if (mine) atomicAdd(&tile_raised, mine);                  // (LDS)
    __syncthreads();
    if (tid == 0 && tile_raised) atomicAdd(raised, (unsigned long long)tile_raised);
}

// one thread per pixel, i < npix.  g and r are only read; a thread ORs kFlagEroded into its own byte of B where g > r (step 35: the
// pixel is in E).  *seeds += |E| of the workgroup: one integer atomic per workgroup that has any, which nothing reads in this launch.
__global__ void __launch_bounds__(kPixThreads) label_hmax_mark_kernel(const uint8_t* __restrict__ g, const uint8_t* __restrict__ r, long long npix,
                                                                      uint8_t* __restrict__ B, unsigned long long* __restrict__ seeds) {
    __shared__ unsigned s_seeds;
    if (threadIdx.x == 0) s_seeds = 0;
    __syncthreads();
    const long long i = (long long)blockIdx.x * kPixThreads + threadIdx.x;
    const bool in = i < npix && g[i] > r[i];
    if (in) B[i] = (uint8_t)(B[i] | kFlagEroded);
    const unsigned n = (unsigned)__popcll(__ballot(in));
    if ((threadIdx.x & 63) == 0 && n) atomicAdd(&s_seeds, n);  // (LDS)
    __syncthreads();
    if (threadIdx.x == 0 && s_seeds) atomicAdd(seeds, (unsigned long long)s_seeds);
}

// One reconstruction: launches src -> dst -> src ... until one raised nothing, one 8-byte read-back after each (as
// run_flood_launches).  On return *src holds the reconstruction.  dec > 0: the first launch takes its marker from the mask.
int run_recon(umx_labeler* lb, const uint8_t* mask, uint8_t** src, uint8_t** dst, int H, int W, int dec, long long* word, int64_t* launches) {
    const int tiles_x = (W - 1) / kTile + 1, tiles_y = (H - 1) / kTile + 1;     // tiles_y * tiles_x <= 2^25 + 2^19: H * W <= INT_MAX
    const long long npix = (long long)H * W;
    hipStream_t s = lb->stream;
    long long raised = 0;
    for (long long n = 1;; ++n) {
        if (n > UMX_HMAX_MAX_LAUNCHES)
            return lfail(lb, UMX_ERR_RANGE, "a reconstruction of the h-maxima seeds was still rising after UMX_HMAX_MAX_LAUNCHES = %d "
                                              "launches: an object's relief sends a value along a path of more than %d pixels",
                         (int)UMX_HMAX_MAX_LAUNCHES, (int)UMX_HMAX_MAX_LAUNCHES * kHalo);
        hipLaunchKernelGGL(label_recon_kernel, dim3((unsigned)tiles_y * (unsigned)tiles_x), dim3(kThreads), 0, s, mask, (const uint8_t*)*src, *dst,
                           H, W, n == 1 ? dec : 0, (int)UMX_HMAX_LAUNCH_STEPS, tiles_x, reinterpret_cast<unsigned long long*>(word));
        std::swap(*src, *dst);
        L_HIP(lb, hipGetLastError());
        long long now = 0;
        L_HIP(lb, hipMemcpyAsync(&now, word, sizeof now, hipMemcpyDeviceToHost, s));
        L_HIP(lb, hipStreamSynchronize(s));
        if (now < raised || now - raised > npix) return lfail(lb, UMX_ERR_HIP, "a reconstruction launch raised %lld of %lld pixels", now - raised, npix);
        *launches = n;
        if (now == raised) return UMX_OK;
        raised = now;
    }
}

}  // namespace

int launch_hmax_seeds(umx_labeler* lb, const uint8_t* planes, int H, int W, const int* P, const int* Q, int min_area,
                      const umx_label_hmax_options* ho, int64_t recon_launches[2]) {
    const long long npix = (long long)H * W;
    const unsigned pix_grid = (unsigned)((npix + kPixThreads - 1) / kPixThreads);
    hipStream_t s = lb->stream;
    uint8_t* plane[4];
    for (int k = 0; k < 4; ++k) plane[k] = reinterpret_cast<uint8_t*>(lb->d_R) + (size_t)k * (size_t)npix;
    L_HIP(lb, hipMemsetAsync(lb->d_hmax, 0, kHmaxWords * sizeof(long long), s));
    hipLaunchKernelGGL(label_hmax_relief_kernel, dim3(pix_grid), dim3(kPixThreads), 0, s, planes, P, Q, npix, min_area, ho->seed_plane,
                       ho->seed_invert, ho->height, lb->d_B, plane[0], plane[1]);
    // step 34: g under f from the marker the relief kernel wrote, between planes 1 and 2
    uint8_t *src = plane[1], *dst = plane[2];
    int rc = run_recon(lb, plane[0], &src, &dst, H, W, 0, lb->d_hmax + kHmaxRaised, &recon_launches[0]);
    if (rc) return rc;
    // step 35: r under g from max(g - 1, 0), between the plane g does not stand in and plane 3 (the first launch never reads its src)
    uint8_t *g = src, *a = dst, *b = plane[3];
    if ((rc = run_recon(lb, g, &a, &b, H, W, 1, lb->d_hmax + kHmaxRaised + 1, &recon_launches[1]))) return rc;
    hipLaunchKernelGGL(label_hmax_mark_kernel, dim3(pix_grid), dim3(kPixThreads), 0, s, (const uint8_t*)g, (const uint8_t*)a, npix, lb->d_B,
                       reinterpret_cast<unsigned long long*>(lb->d_hmax + kHmaxSeeds));
    L_HIP(lb, hipGetLastError());
    return UMX_OK;
}

}  // namespace umx
