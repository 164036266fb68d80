// libumx border weight maps of a device-resident training set: the two kernels behind umx_trainset_border_weights / _border_planes
// (include/umx_train.h, DESIGN.md section 9.2 "Border weight maps") and the host check of their options.
//
//   border_label_kernel  4-connected components of (annotation == code) of one sample per workgroup, by union-find in an int32 plane of
//                        the set's workspace: every object pixel ends up holding the flat index y * S + x of its component's first pixel
//                        in raster order (the root: links only ever point at smaller indices), every other pixel -1
//   border_map_kernel    one thread per pixel of a 32 x 32 tile; the tile's labels (root + 1, 0 off objects and outside the image) and a
//                        halo of R pixels are staged in LDS; two scans of the disc dy^2 + dx^2 <= R^2 give the squared distance to the
//                        nearest object pixel and to the nearest one of another component; W = float32(exp(-(d1 + d2)^2 / (2 sigma^2)))
//
// No workgroup reads what another one writes inside a kernel: a sample is labelled by one workgroup, and the map kernel reads the
// finished labels of the launch before it.
#include "../../include/umx_train.h"
#include "umx_internal.h"
#include "umx_unionfind.h"   // parent_load / parent_store / find_root / union_trees

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdio>

namespace umx {

namespace {

constexpr int kLabelThreads = 1024;                      // one workgroup per sample: 16 waves
constexpr int kBorderTile = 32;                          // output tile of one workgroup of the map kernel
constexpr int kBorderMaxR = 32;                          // ceil(4 * UMX_BORDER_MAX_SIGMA)
constexpr int kBorderWin = kBorderTile + 2 * kBorderMaxR;   // 96 x 96 int32 = 36 KiB of LDS
static_assert(kBorderMaxR == (int)(4.0f * UMX_BORDER_MAX_SIGMA), "the LDS window is sized for the largest sigma");

// between two phases of the labelling: every store of the workgroup has reached L2 before any thread goes on
__device__ inline void phase_barrier() {
    __threadfence();
    __syncthreads();
}

// P: the sample's [S][S] plane of the workspace.  Four phases, a barrier between them:
//   0  per row, every pixel of a run of object pixels points at the run's first pixel (ballots over 64-pixel chunks); others get -1.
//      From here on a link's target is always the first pixel of a run, so only those are ever changed.
//   1  every object pixel with an object pixel above it merges the two trees -- unless its left neighbour and that one's upper
//      neighbour are object pixels too: then the left neighbour's merge connects the same two runs.
//   2  every run's first pixel is pointed at its root (roots no longer change).
//   3  every other object pixel takes the (final) value of its run's first pixel.
__global__ void __launch_bounds__(kLabelThreads) border_label_kernel(const uint8_t* __restrict__ ann, int S, int row_a, int code,
                                                                     int* __restrict__ ws) {
    const uint8_t* A = ann + (size_t)blockIdx.x * S * row_a;
    int* P = ws + (size_t)blockIdx.x * S * S;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int npix = S * S;
    for (int y = wave; y < S; y += kLabelThreads / 64) {
        int carry = -1;   // first column of the run that reaches the end of the previous chunk; -1: none
        for (int x0 = 0; x0 < S; x0 += 64) {
            const int x = x0 + lane;
            const bool obj = x < S && A[(size_t)y * row_a + x] == code;
            const unsigned long long mask = __ballot(obj);
            if (x < S) {
                int v = -1;
                if (obj) {
                    const unsigned long long gaps = ~mask & ((1ull << lane) - 1ull);   // pixels off the object left of this one
                    const int start = gaps ? x0 + 64 - __clzll((long long)gaps) : (carry >= 0 ? carry : x0);
                    v = y * S + start;
                }
                parent_store(P + y * S + x, v);
            }
            if (mask >> 63) {
                const unsigned long long gaps = ~mask;
                carry = gaps ? x0 + 64 - __clzll((long long)gaps) : (carry >= 0 ? carry : x0);
            } else {
                carry = -1;
            }
        }
    }
    phase_barrier();
    for (int i = threadIdx.x; i < npix; i += kLabelThreads) {
        const int x = i % S;
        if (i < S || parent_load(P + i) < 0 || parent_load(P + i - S) < 0) continue;
        if (x > 0 && parent_load(P + i - 1) >= 0 && parent_load(P + i - 1 - S) >= 0) continue;
        union_trees(P, i, i - S);
    }
    phase_barrier();
    for (int i = threadIdx.x; i < npix; i += kLabelThreads) {
        const int p = parent_load(P + i);
        if (p < 0 || (i % S > 0 && parent_load(P + i - 1) >= 0)) continue;
        const int r = find_root(P, i);
        if (r != p) parent_store(P + i, r);
    }
    phase_barrier();
    for (int i = threadIdx.x; i < npix; i += kLabelThreads) {
        const int p = parent_load(P + i);
        if (p < 0 || i % S == 0 || parent_load(P + i - 1) < 0) continue;
        parent_store(P + i, parent_load(P + p));   // (p: the run's first pixel, in this row, not rewritten in this phase)
    }
}

// float32(exp(-(sqrt(d1) + sqrt(d2))^2 / den)) in float64, every operation one rounding
__device__ inline float border_weight(int d1sq, int d2sq, double den) {
#pragma clang fp contract(off)
    const double s = sqrt((double)d1sq) + sqrt((double)d2sq);
    const double q = s * s;
    return (float)exp(-q / den);
}

// the least dy^2 + dx^2 over the disc's pixels with a label other than 0 and `skip`; *label: that pixel's.  INT_MAX: none.
__device__ inline int disc_nearest(const int* centre, int W, int R, const int* half, int skip, int* label) {
    int best = INT_MAX, lab = 0;
    for (int dy = -R; dy <= R; ++dy) {
        const int* row = centre + dy * W;
        const int w = half[dy + R], dd = dy * dy;
        for (int dx = -w; dx <= w; ++dx) {
            const int l = row[dx], d = dd + dx * dx;
            if (l != 0 && l != skip && d < best) { best = d; lab = l; }
        }
    }
    *label = lab;
    return best;
}

// grid (tiles^2, samples).  Window element (r, q) is pixel (ty0 - R + r, tx0 - R + q) of the sample; pixels outside the image hold
// label 0 like every pixel off the objects: they do not exist.  A thread scans rows r = yy + R + dy, dy = -R..R, and columns
// q = xx + R + dx, |dx| <= half[dy + R] <= R, of its own pixel (yy, xx) of the tile: inside the (32 + 2R)^2 window.
__global__ void __launch_bounds__(256) border_map_kernel(const int* __restrict__ ws, int S, int R, double den, float* __restrict__ wmap,
                                                         int row_w, size_t plane_w, int* __restrict__ labels, int* __restrict__ d1sq,
                                                         int* __restrict__ d2sq) {
    __shared__ int win[kBorderWin * kBorderWin];
    __shared__ int half[2 * kBorderMaxR + 1];             // half[dy + R]: the largest |dx| with dy^2 + dx^2 <= R^2
    const size_t plane = (size_t)S * S;
    const int* L = ws + blockIdx.y * plane;
    const int tiles = (S + kBorderTile - 1) / kBorderTile;
    const int ty0 = (blockIdx.x / tiles) * kBorderTile, tx0 = (blockIdx.x % tiles) * kBorderTile;
    const int W = kBorderTile + 2 * R;
    for (int e = threadIdx.x; e < W * W; e += 256) {
        const int y = ty0 - R + e / W, x = tx0 - R + e % W;
        win[e] = (y >= 0 && y < S && x >= 0 && x < S) ? L[(size_t)y * S + x] + 1 : 0;
    }
    if ((int)threadIdx.x <= 2 * R) {
        const int dy = (int)threadIdx.x - R, rem = R * R - dy * dy;
        int w = 0;
        while (w < R && (w + 1) * (w + 1) <= rem) ++w;     // (at most R steps)
        half[threadIdx.x] = w;
    }
    __syncthreads();
    const int xx = threadIdx.x & 31;
    for (int k = 0; k < kBorderTile / 8; ++k) {
        const int yy = (threadIdx.x >> 5) + 8 * k;
        const int y = ty0 + yy, x = tx0 + xx;
        if (y >= S || x >= S) continue;
        const int* centre = &win[(yy + R) * W + xx + R];
        int l1 = *centre, l2 = 0, a = 0, b = INT_MAX;
        if (l1 == 0) a = disc_nearest(centre, W, R, half, 0, &l1);       // (inside an object the nearest pixel is the pixel itself)
        if (l1 != 0) b = disc_nearest(centre, W, R, half, l1, &l2);
        const int d1 = l1 != 0 ? a : -1, d2 = l2 != 0 ? b : -1;
        wmap[blockIdx.y * plane_w + (size_t)y * row_w + x] = d2 >= 0 ? border_weight(d1, d2, den) : 0.f;
        const size_t o = blockIdx.y * plane + (size_t)y * S + x;
        if (labels) labels[o] = *centre;
        if (d1sq) d1sq[o] = d1;
        if (d2sq) d2sq[o] = d2;
    }
}

}  // namespace

hipError_t launch_border_label(const uint8_t* ann, int n, int S, int row_a, int code, int* ws, hipStream_t stream) {
    if (n < 1 || S < 1 || (long long)S * S > INT_MAX || row_a < S || code < 1 || code > 255) return hipErrorInvalidValue;
    hipLaunchKernelGGL(border_label_kernel, dim3((unsigned)n), dim3(kLabelThreads), 0, stream, ann, S, row_a, code, ws);
    return hipGetLastError();
}

hipError_t launch_border_map(const int* ws, int n, int S, int R, double den, float* wmap, int row_w, size_t plane_w, int* labels,
                             int* d1sq, int* d2sq, hipStream_t stream) {
    if (n < 1 || S < 1 || (long long)S * S > INT_MAX || R < 1 || R > kBorderMaxR || !(den > 0.0) || row_w < S) return hipErrorInvalidValue;
    const unsigned tiles = (unsigned)((S + kBorderTile - 1) / kBorderTile);
    const size_t plane = (size_t)S * S;
    constexpr int kPerLaunch = 32768;                     // (gridDim.y holds 65535)
    for (int s0 = 0; s0 < n; s0 += kPerLaunch) {
        const int m = std::min(kPerLaunch, n - s0);
        hipLaunchKernelGGL(border_map_kernel, dim3(tiles * tiles, (unsigned)m), dim3(256), 0, stream, ws + s0 * plane, S, R, den,
                           wmap + s0 * plane_w, row_w, plane_w, labels ? labels + s0 * plane : nullptr, d1sq ? d1sq + s0 * plane : nullptr,
                           d2sq ? d2sq + s0 * plane : nullptr);
    }
    return hipGetLastError();
}

int border_radius(float sigma) { return (int)std::ceil(4.0 * (double)sigma); }

}  // namespace umx

extern "C" {

int umx_border_options_check(const umx_border_options* o, int n_classes, char* msg, size_t cap) {
    char buf[160] = "";
    if (!o) snprintf(buf, sizeof buf, "null border options");
    else if (o->object_code < 1 || o->object_code > n_classes)
        snprintf(buf, sizeof buf, "object_code is %d: the objects' class code is 1..%d", o->object_code, n_classes);
    else if (!(o->sigma > 0.f && o->sigma <= UMX_BORDER_MAX_SIGMA))   // (a NaN fails both comparisons)
        snprintf(buf, sizeof buf, "sigma is %g: it must be above 0 and at most %g", (double)o->sigma, (double)UMX_BORDER_MAX_SIGMA);
    for (int i = 0; o && !buf[0] && i < 6; ++i)
        if (o->reserved[i]) snprintf(buf, sizeof buf, "reserved must be zero");
    if (msg && cap) snprintf(msg, cap, "%s", buf);
    return buf[0] ? UMX_ERR_INVALID : UMX_OK;
}

}  // extern "C"
