// libumx device-resident training set: the kernels that write a step's data / labels / weights buffers from the set, their device
// helpers and their launchers (umx_internal.h).  Storage, the host checks, the chunking of a batch (enqueue_batch) and the C ABI are in
// umx_trainset.hip.  DESIGN.md section 9.2.
//
//   assemble_batch_kernel  data[b,y,x,c] = float32((double)v * contrast + brightness) at the transformed crop coordinate;
//                          labels[b,y,x,k] = (code == k+1); weights[b,y,x,k] = float32((double)iw[k] * wmap + cw[k])
//   assemble_augmented_kernel  the data planes of the images that ask for a blur level or a saturation gain (umx_augment_desc):
//                          page plane -> separable Gaussian blur -> saturation -> crop + transform -> jitter, float64 in a fixed order
//   assemble_augmented_kernel<true>  the same for the images with a rotation / zoom (umx_warp_desc): the window is resampled
//                          (mirror fold, bilinear, float64 in a fixed order) instead of copied
//   assemble_augmented_kernel<true, true>  the images with an elastic deformation (umx_elastic_desc): the B-spline displacement of the
//                          lattice is added to the pixel's coordinate in front of the warp matrix; one resampling
//   assemble_resampled_labels_kernel<AugChunk / ElasticChunk>  the labels and weights of the warped resp. deformed images, from the
//                          nearest source pixel
#include "../../include/umx_train.h"
#include "umx_internal.h"

#include <type_traits>

static_assert(sizeof(umx::DescChunk) <= 2048, "a descriptor chunk travels as kernel arguments");
static_assert(sizeof(umx::AugChunk) <= 2048, "a chunk of augmented images travels as kernel arguments");
static_assert(sizeof(umx::AugImage) == 112, "an augmented image is 112 bytes of kernel arguments");
static_assert(sizeof(umx::ElasticImage) == 404, "an elastic image is 404 bytes of kernel arguments");
// the widest launch: TrainSetView, the chunk, P, K (or mean, std) and up to two pointers -- inside the 4 KB of arguments a launch may carry
static_assert(sizeof(umx::TrainSetView) + sizeof(umx::ElasticChunk) + 2 * sizeof(float) + 8 + 2 * sizeof(void*) <= 4096,
              "a chunk of elastic images travels as kernel arguments");

namespace umx {

namespace {

// float32(a * b + c) with the product and the sum rounded in float64, never fused into one fma (HIP's __dmul_rn / __dadd_rn are plain
// operators that the default -ffp-contract=fast fuses): what numpy computes for (a * b + c).astype(float32) on float64 operands
__device__ inline float mul_add_f64_rn(double a, double b, double c) {
#pragma clang fp contract(off)
    return (float)(a * b + c);
}

// the dihedral transform of the P x P crop: bit 2 swaps the axes, then bit 1 flips the rows, then bit 0 flips the columns.  out[y, x]
// reads crop[cy, cx] with (u, v) = (flipped y, flipped x) and (cy, cx) = swap ? (v, u) : (u, v).  No other code maps a pixel
// through the transform bits (the data kernel looks at bit 2 once more, to choose the axis of its tile that a wave walks).
struct Pixel { int y, x; };
constexpr Pixel crop_pixel(int transform, int P, int y, int x) {
    const int u = (transform & 2) ? P - 1 - y : y;
    const int v = (transform & 1) ? P - 1 - x : x;
    return (transform & 4) ? Pixel{v, u} : Pixel{u, v};
}
// its inverse: the output pixel that reads crop[cy, cx]
constexpr Pixel output_pixel(int transform, int P, int cy, int cx) {
    const int u = (transform & 4) ? cx : cy, v = (transform & 4) ? cy : cx;
    return Pixel{(transform & 2) ? P - 1 - u : u, (transform & 1) ? P - 1 - v : v};
}
constexpr bool dihedral_round_trip(int P) {
    for (int t = 0; t < 8; ++t)
        for (int y = 0; y < P; ++y)
            for (int x = 0; x < P; ++x) {
                const Pixel c = crop_pixel(t, P, y, x), o = output_pixel(t, P, c.y, c.x);
                if (o.y != y || o.x != x) return false;
            }
    return true;
}
static_assert(dihedral_round_trip(3), "output_pixel is the inverse of crop_pixel");

// the K labels and, where wp, the K weights of one output pixel from source pixel (sy, sx) of sample `index`
__device__ inline void write_labels_weights(const TrainSetView& ts, int index, int sy, int sx, int K, float* lp, float* wp) {
    const int code = ts.ann[((size_t)index * ts.S + sy) * ts.row_a + sx];
    for (int k = 0; k < K; ++k) lp[k] = code == k + 1 ? 1.f : 0.f;   // (im == i + 1), UnMicst1-5.py:306
    if (wp) {
        const double w = (double)ts.wmap[((size_t)index * ts.S + sy) * ts.row_f + sx];
        for (int k = 0; k < K; ++k)   // W * intersectWeight + classWeight, UnMicst1-5.py:307-312
            wp[k] = mul_add_f64_rn((double)ts.iw[k], w, (double)ts.cw[k]);
    }
}

// one thread per output pixel (y, x) of image blockIdx.y of the chunk; every thread writes its C data, K label and K weight
// values, so a wave stores one contiguous run of the NHWC outputs.  The source pixel is read through L2: a transform that swaps
// the axes reads a column of the crop per wave (S floats apart), which at these sizes (a few MB per step) is not worth an LDS
// transpose.
__global__ void __launch_bounds__(256) assemble_batch_kernel(TrainSetView ts, DescChunk dc, int b0, int P, int K,
                                                             float* __restrict__ data, float* __restrict__ labels,
                                                             float* __restrict__ weights) {
    const int j = blockIdx.y;
    const int pix = blockIdx.x * 256 + threadIdx.x;
    if (pix >= P * P) return;
    const umx_sample_desc d = dc.d[j];
    const size_t o = (size_t)(b0 + j) * P * P + pix;
    float* dp = data + o * ts.C;
    float* lp = labels + o * K;
    float* wp = weights ? weights + o * K : nullptr;
    if (d.index < 0) {   // padding row
        for (int c = 0; c < ts.C; ++c) dp[c] = 0.f;
        for (int k = 0; k < K; ++k) lp[k] = 0.f;
        if (wp)
            for (int k = 0; k < K; ++k) wp[k] = 0.f;
        return;
    }
    const Pixel cp = crop_pixel(d.transform, P, pix / P, pix - (pix / P) * P);
    const int sy = d.y0 + cp.y, sx = d.x0 + cp.x;
    const size_t plane = (size_t)ts.S * ts.row_f;
    const float* src = ts.planes + ((size_t)d.index * ts.C * ts.pages + d.page) * plane + (size_t)sy * ts.row_f + sx;
    const double cont = (double)d.contrast, brig = (double)d.brightness;
    // float64 product and sum, one rounding to float32 (the reference jitters its float64 arrays, UnMicst1-5.py:473-477)
    for (int c = 0; c < ts.C; ++c) dp[c] = mul_add_f64_rn((double)src[(size_t)c * ts.pages * plane], cont, brig);
    write_labels_weights(ts, d.index, sy, sx, K, lp, wp);
}

constexpr int kAugTile = 32;                                         // output tile of one workgroup, in crop orientation
constexpr int kAugWin = kAugTile + 2 * UMX_AUGMENT_MAX_RADIUS;       // its source window at the largest radius
constexpr int kAugHStride = kAugTile + 1;                            // (odd: a wave may walk a column of `hor` without bank conflicts)

// float32(sum over t = -R..R, ascending, of w[|t|] * p[t]); p points at t = -R.  The sum starts at 0.0 and every product and every
// sum is rounded in float64 on its own, as numpy does it tap by tap.
__device__ inline float blur_taps(const float* p, int stride, int R, const double* w) {
#pragma clang fp contract(off)
    double acc = 0.0;
    for (int t = -R; t <= R; ++t) acc = acc + w[t < 0 ? -t : t] * (double)p[(t + R) * stride];
    return (float)acc;
}

// back to the im2double scale, amplified, clipped at 1 (np.minimum: a NaN stays), normalised again; one rounding per operation
__device__ inline float saturate_f64_rn(float b, double gain, double mean, double std) {
#pragma clang fp contract(off)
    const double r = (double)b * std + mean;
    const double rg = r * gain;
    const double r2 = rg > 1.0 ? 1.0 : rg;
    return (float)((r2 - mean) / std);
}

// a source coordinate mirrored into 0 .. S-1 about the centres of the sample's edge pixels (d c b | a b c d | c b a), S >= 2.  A
// quotient that rounds up to the next integer leaves t a hair below 0: that is the edge pixel.
__device__ inline double warp_fold(double s, int S) {
#pragma clang fp contract(off)
    const double T = 2.0 * (double)(S - 1);
    const double q = floor(s / T);
    double t = s - T * q;
    if (t > (double)(S - 1)) t = T - t;
    return t < 0.0 ? 0.0 : t;
}

// where the point (y, x) of the crop's own grid lies in the sample: M (y - c, x - c) + the crop's centre, folded.  (y, x) is a pixel
// (any integer, also outside 0 .. P-1) or, under a lattice, that pixel plus its displacement (recipe 1' of umx_elastic_desc).  Every
// product and every sum is rounded in float64 on its own.
__device__ inline void warp_source(const float* m, double y, double x, int P, int y0, int x0, int S, double* ty, double* tx) {
#pragma clang fp contract(off)
    const double c = 0.5 * (double)(P - 1);
    const double dy = y - c, dx = x - c;
    *ty = warp_fold(((double)m[0] * dy + (double)m[1] * dx) + ((double)y0 + c), S);
    *tx = warp_fold(((double)m[2] * dy + (double)m[3] * dx) + ((double)x0 + c), S);
}

// bilinear value of a sample plane at a folded coordinate: along the row first, then between the two rows, one float32 rounding
__device__ inline float warp_bilinear(const float* plane, int row_f, int S, double ty, double tx) {
#pragma clang fp contract(off)
    const int iy = min(max((int)ty, 0), S - 1), ix = min(max((int)tx, 0), S - 1);   // (0 <= t <= S-1: truncation is floor; the clamp is for a NaN)
    const double fy = ty - (double)iy, fx = tx - (double)ix;
    const int iy1 = min(iy + 1, S - 1), ix1 = min(ix + 1, S - 1);
    const float* r0 = plane + (size_t)iy * row_f;
    const float* r1 = plane + (size_t)iy1 * row_f;
    const double gx = 1.0 - fx;
    const double top = gx * (double)r0[ix] + fx * (double)r0[ix1];
    const double bot = gx * (double)r1[ix] + fx * (double)r1[ix1];
    return (float)((1.0 - fy) * top + fy * bot);
}

// the nearest source pixel of a folded coordinate (labels and weight maps are never interpolated)
__device__ inline int warp_nearest(double t, int S) {
#pragma clang fp contract(off)
    return min(max((int)(t + 0.5), 0), S - 1);
}

// six times the uniform cubic B-spline's weights at integer coordinate t of an axis of the crop's grid (recipe 0a of umx_elastic_desc):
// n - 3 spline cells across 0 .. P-1, a coordinate outside the crop clamped to its edge.  *i0: the first of the 4 lattice points.
__device__ inline void elastic_weights(int t, int P, int n, double* W, int* i0) {
#pragma clang fp contract(off)
    const double tc = (double)min(max(t, 0), P - 1);
    const double scale = (double)(n - 3) / (double)(P - 1);
    const double u = tc * scale;
    const int i = min(max((int)u, 0), n - 4);   // (u >= 0: truncation is floor; the lower clamp is for a NaN)
    const double f = u - (double)i;
    const double g = 1.0 - f, f2 = f * f, f3 = f2 * f;
    W[0] = (g * g) * g;
    W[1] = (3.0 * f3 - 6.0 * f2) + 4.0;
    W[2] = ((-3.0 * f3 + 3.0 * f2) + 3.0 * f) + 1.0;
    W[3] = f3;
    *i0 = i;
}

// one component of the displacement (recipe 0b): D the component's 6 x 6 lattice, along the lattice rows first, then between them
__device__ inline double elastic_disp(const double* D, const double* Wy, int iy, const double* Wx, int ix) {
#pragma clang fp contract(off)
    double row[4];
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        const double* r = D + (iy + a) * UMX_ELASTIC_MAX_GRID + ix;
        row[a] = ((Wx[0] * r[0] + Wx[1] * r[1]) + Wx[2] * r[2]) + Wx[3] * r[3];
    }
    return (((Wy[0] * row[0] + Wy[1] * row[1]) + Wy[2] * row[2]) + Wy[3] * row[3]) / 36.0;
}

// the kernels' argument types: an image's lattice rides behind its AugImage
template <bool kElastic> struct ChunkOf { using type = AugChunk; };
template <> struct ChunkOf<true> { using type = ElasticChunk; };
__host__ __device__ inline const AugImage& aug_image(const AugChunk& c, unsigned j) { return c.im[j]; }
__host__ __device__ inline const AugImage& aug_image(const ElasticChunk& c, unsigned j) { return c.im[j].a; }
constexpr int kLattice = 2 * UMX_ELASTIC_MAX_GRID * UMX_ELASTIC_MAX_GRID;   // the floats of an image's lattice

// one workgroup per (32 x 32 tile of the crop, channel, image).  The (32 + 2R)^2 source window goes to LDS with both coordinates
// clamped to the sample, so a crop at the sample's edge sees the replicated edge and a crop inside it its real neighbours; the row pass
// writes `hor` (float32, the rounding the recipe asks for), the column pass reads it.  A wave owns one row of the tile -- or, under a
// transform that swaps the axes, one column, so that its 32 stores are neighbours in the NHWC output either way.
// kWarp: every window element is resampled from the plane instead (im.m: rotation and zoom about the crop's centre).  The warped
// image exists at every integer coordinate, so the window needs no clamp; without a blur each thread resamples its own pixel.
// kElastic (with kWarp): the source coordinate of a window element also takes the lattice's displacement.  The spline weights depend on
// the integer coordinate alone, so the workgroup computes those of its window's rows and of its columns once (2 (32 + 2R) sets), next to
// the lattice as float64, and an element combines them with 16 lattice values per component.
template <bool kWarp, bool kElastic = false>
__global__ void __launch_bounds__(256) assemble_augmented_kernel(TrainSetView ts, typename ChunkOf<kElastic>::type ac, int P, float mean,
                                                                 float std, float* __restrict__ data) {
    static_assert(kWarp || !kElastic, "the elastic displacement is a term of the warp's source coordinate");
    __shared__ float win[kAugWin * kAugWin];
    __shared__ float hor[kAugWin * kAugHStride];
    __shared__ double w64[UMX_AUGMENT_MAX_RADIUS + 1];
    __shared__ double lat64[kElastic ? kLattice : 1];
    __shared__ double ew64[kElastic ? 2 * kAugWin * 4 : 1];   // [axis][window row resp. column][4]
    __shared__ int ei[kElastic ? 2 * kAugWin : 1];            // the first lattice point of each
    const AugImage& im = aug_image(ac, blockIdx.z);
    const umx_sample_desc d = im.d;
    const int c = blockIdx.y;
    const int tiles = (P + kAugTile - 1) / kAugTile;
    const int cy0 = (blockIdx.x / tiles) * kAugTile, cx0 = (blockIdx.x % tiles) * kAugTile;
    const int lane = threadIdx.x & 31, grp = threadIdx.x >> 5;
    const int R = im.R;
    const bool swap = (d.transform & 4) != 0;
    const float* src = ts.planes + (((size_t)d.index * ts.C + c) * ts.pages + d.page) * ((size_t)ts.S * ts.row_f);
    const int halo = R >= 0 ? R : 0;    // window element (r, q) is pixel (cy0 - halo + r, cx0 - halo + q) of the crop's grid
    if constexpr (kElastic) {
        const ElasticImage& el = ac.im[blockIdx.z];
        const int W = kAugTile + 2 * halo;
        const int n = min(max(el.n, 4), UMX_ELASTIC_MAX_GRID);
        if ((int)threadIdx.x < kLattice) lat64[threadIdx.x] = (double)(&el.d[0][0][0])[threadIdx.x];
        if ((int)threadIdx.x < 2 * W) {
            const int axis = (int)threadIdx.x >= W, r = (int)threadIdx.x - axis * W;
            elastic_weights((axis ? cx0 : cy0) - halo + r, P, n, &ew64[(axis * kAugWin + r) * 4], &ei[axis * kAugWin + r]);
        }
        __syncthreads();
    }
    // the image at window element (r, q): copied (clamped to the sample), resampled under im.m, or resampled at the coordinate the
    // lattice displaces, from the tables above
    auto source = [&](int r, int q) -> float {
#pragma clang fp contract(off)
        const int gy = cy0 - halo + r, gx = cx0 - halo + q;
        if constexpr (kWarp) {
            double py = (double)gy, px = (double)gx, ty, tx;
            if constexpr (kElastic) {
                const double* wy = &ew64[r * 4];
                const double* wx = &ew64[(kAugWin + q) * 4];
                const int iy = ei[r], ix = ei[kAugWin + q];
                py = py + elastic_disp(lat64, wy, iy, wx, ix);
                px = px + elastic_disp(lat64 + kLattice / 2, wy, iy, wx, ix);
            }
            warp_source(im.m, py, px, P, d.y0, d.x0, ts.S, &ty, &tx);
            return warp_bilinear(src, ts.row_f, ts.S, ty, tx);
        } else {
            const int sy = min(max(d.y0 + gy, 0), ts.S - 1), sx = min(max(d.x0 + gx, 0), ts.S - 1);
            return src[(size_t)sy * ts.row_f + sx];
        }
    };
    if (R >= 0) {
        const int W = kAugTile + 2 * R;
        for (int r = grp; r < W; r += 8)
            for (int q = lane; q < W; q += 32) win[r * W + q] = source(r, q);
        if ((int)threadIdx.x <= R) w64[threadIdx.x] = (double)im.taps[threadIdx.x];
        __syncthreads();
        for (int r = grp; r < W; r += 8) hor[r * kAugHStride + lane] = blur_taps(&win[r * W + lane], 1, R, w64);
        __syncthreads();
    }
    const double gain = (double)im.gain, cont = (double)d.contrast, brig = (double)d.brightness;
    for (int i = 0; i < kAugTile / 8; ++i) {
        const int yy = swap ? lane : grp + 8 * i, xx = swap ? grp + 8 * i : lane;   // pixel of the tile, crop orientation
        const int cy = cy0 + yy, cx = cx0 + xx;
        if (cy >= P || cx >= P) continue;
        float v = R >= 0 ? blur_taps(&hor[yy * kAugHStride + xx], kAugHStride, R, w64) : source(yy, xx);
        if (im.gain != 1.f) v = saturate_f64_rn(v, gain, (double)mean, (double)std);
        const Pixel o = output_pixel(d.transform, P, cy, cx);
        data[(((size_t)im.row * P + o.y) * P + o.x) * ts.C + c] = mul_add_f64_rn((double)v, cont, brig);
    }
}

// labels and weights of the resampled images, written over what assemble_batch_kernel wrote: one thread per output pixel, its K values
// each, as there.  The pixel's place in the crop is that kernel's map; its label and its weight come from the one source pixel
// nearest to the warped coordinate.  ElasticChunk: the pixel's place in the crop is displaced by its lattice first; a thread computes
// the spline weights of its own row and column (once per pixel here, not once per window element and channel).
template <typename Chunk>
__global__ void __launch_bounds__(256) assemble_resampled_labels_kernel(TrainSetView ts, Chunk ch, int P, int K,
                                                                        float* __restrict__ labels, float* __restrict__ weights) {
    constexpr bool kElastic = std::is_same<Chunk, ElasticChunk>::value;
    __shared__ double lat64[kElastic ? kLattice : 1];
    if constexpr (kElastic) {
        if ((int)threadIdx.x < kLattice) lat64[threadIdx.x] = (double)(&ch.im[blockIdx.y].d[0][0][0])[threadIdx.x];
        __syncthreads();
    }
    const int pix = blockIdx.x * 256 + threadIdx.x;
    if (pix >= P * P) return;
    const AugImage& im = aug_image(ch, blockIdx.y);
    const umx_sample_desc d = im.d;
    const Pixel cp = crop_pixel(d.transform, P, pix / P, pix - (pix / P) * P);
    double py = (double)cp.y, px = (double)cp.x, ty, tx;
    if constexpr (kElastic) {
#pragma clang fp contract(off)
        const int n = min(max(ch.im[blockIdx.y].n, 4), UMX_ELASTIC_MAX_GRID);
        double wy[4], wx[4];
        int iy, ix;
        elastic_weights(cp.y, P, n, wy, &iy);
        elastic_weights(cp.x, P, n, wx, &ix);
        py = py + elastic_disp(lat64, wy, iy, wx, ix);
        px = px + elastic_disp(lat64 + kLattice / 2, wy, iy, wx, ix);
    }
    warp_source(im.m, py, px, P, d.y0, d.x0, ts.S, &ty, &tx);
    const size_t o = ((size_t)im.row * P * P + pix) * K;
    write_labels_weights(ts, d.index, warp_nearest(ty, ts.S), warp_nearest(tx, ts.S), K, labels + o, weights ? weights + o : nullptr);
}

// m images in the chunk, each with a blur radius the LDS window is sized for
template <typename Chunk>
bool chunk_in_range(const Chunk& ch, int m) {
    if (m < 1 || m > (int)(sizeof ch.im / sizeof ch.im[0])) return false;
    for (int j = 0; j < m; ++j)
        if (aug_image(ch, j).R < -1 || aug_image(ch, j).R > UMX_AUGMENT_MAX_RADIUS) return false;
    return true;
}

template <bool kWarp, bool kElastic, typename Chunk>
void launch_data_planes(const TrainSetView& ts, const Chunk& ch, int m, int P, float mean, float std, float* data, hipStream_t stream) {
    const unsigned tiles = (unsigned)((P + kAugTile - 1) / kAugTile);
    hipLaunchKernelGGL((assemble_augmented_kernel<kWarp, kElastic>), dim3(tiles * tiles, (unsigned)ts.C, (unsigned)m), dim3(256), 0, stream,
                       ts, ch, P, mean, std, data);
}

}  // namespace

hipError_t launch_assemble_batch(const TrainSetView& ts, const DescChunk& dc, int m, int b0, int P, int K, float* data, float* labels,
                                 float* weights, hipStream_t stream) {
    if (m < 1 || m > kDescChunk || K < 1 || K > 8) return hipErrorInvalidValue;
    hipLaunchKernelGGL(assemble_batch_kernel, dim3((unsigned)((P * P + 255) / 256), (unsigned)m), dim3(256), 0, stream, ts, dc, b0, P, K,
                       data, labels, weights);
    return hipGetLastError();
}

hipError_t launch_assemble_augmented(const TrainSetView& ts, const AugChunk& ac, int m, int P, float mean, float std, float* data,
                                     hipStream_t stream) {
    if (!chunk_in_range(ac, m) || P < 1) return hipErrorInvalidValue;
    launch_data_planes<false, false>(ts, ac, m, P, mean, std, data, stream);
    return hipGetLastError();
}

template <typename Chunk>
hipError_t launch_assemble_resampled(const TrainSetView& ts, const Chunk& ch, int m, int P, int K, float mean, float std, float* data,
                                     float* labels, float* weights, hipStream_t stream) {
    constexpr bool kElastic = std::is_same<Chunk, ElasticChunk>::value;
    // (S = 1 has no mirror period, P = 1 no spline cell)
    if (!chunk_in_range(ch, m) || P < (kElastic ? 2 : 1) || K < 1 || K > 8 || ts.S < 2) return hipErrorInvalidValue;
    if constexpr (kElastic)
        for (int j = 0; j < m; ++j)
            if (ch.im[j].n < 4 || ch.im[j].n > UMX_ELASTIC_MAX_GRID) return hipErrorInvalidValue;   // (the LDS lattice is 6 x 6)
    launch_data_planes<true, kElastic>(ts, ch, m, P, mean, std, data, stream);
    hipLaunchKernelGGL(assemble_resampled_labels_kernel<Chunk>, dim3((unsigned)((P * P + 255) / 256), (unsigned)m), dim3(256), 0, stream, ts,
                       ch, P, K, labels, weights);
    return hipGetLastError();
}
template hipError_t launch_assemble_resampled(const TrainSetView&, const AugChunk&, int, int, int, float, float, float*, float*, float*, hipStream_t);
template hipError_t launch_assemble_resampled(const TrainSetView&, const ElasticChunk&, int, int, int, float, float, float*, float*, float*, hipStream_t);

}  // namespace umx
