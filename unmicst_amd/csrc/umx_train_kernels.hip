// Kernels of the training step of libumx (gfx950 only): weight repacking, batch-statistics BN forward/backward,
// activation / dropout / max-pool forward and backward, the top layer with the weighted cross-entropy, and the
// optimiser.  The convolutions themselves (forward, input gradient, transposed forward, transposed input gradient on
// a space-to-depth tensor) run on conv_mfma_f32 (umx_kernels.hip) with operands packed by pack_weights_kernel; the
// weight gradient of a convolution is umx_wgrad.hip.
//
// Every reduction has a fixed summation order (per-thread serial sums, in-block sums in thread order, partials summed
// in block order, fp64): a step is bit-reproducible from run to run.  No floating-point atomics anywhere.
#include "../../include/umx_train.h"
#include "umx_kernels.h"

#include <algorithm>
#include <mutex>

#pragma clang fp contract(off)

namespace umx {

typedef float f32x4 __attribute__((ext_vector_type(4)));

// ------------------------------------------------------------------------------------------------ weight packing
__global__ void __launch_bounds__(256) pack_weights_kernel(const PackDesc* __restrict__ descs) {
    const PackDesc& d = descs[blockIdx.y];
    const size_t n = (size_t)d.ntaps * d.Cp * d.Np;
    for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < n; e += (size_t)gridDim.x * 256) {
        const int nn = (int)(e % d.Np);
        const size_t r = e / d.Np;
        const int c = (int)(r % d.Cp);
        const int t = (int)(r / d.Cp);
        float v = 0.f;
        if (c < d.C && nn < d.N) {
            const int par = c / d.Cblk, cc = c - par * d.Cblk;
            const int m = d.mtap[t * d.npar + par];
            if (m >= 0) {
                const size_t idx = d.transpose ? ((size_t)m * d.d2 + d.c_off + nn) * d.d3 + cc
                                               : ((size_t)m * d.d2 + d.c_off + cc) * d.d3 + nn;
                v = d.w[idx];
                if (d.w2) v += d.w2[idx];
            }
        }
        d.dst[e] = v;
    }
}

hipError_t launch_pack_weights(const PackDesc* descs_dev, int ndesc, size_t max_elems, hipStream_t stream) {
    if (ndesc <= 0) return hipSuccess;
    const unsigned gx = (unsigned)std::min<size_t>(512, (max_elems + 255) / 256);
    hipLaunchKernelGGL(pack_weights_kernel, dim3(gx ? gx : 1, (unsigned)ndesc), dim3(256), 0, stream, descs_dev);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------ per-element passes
// The per-element passes of the step (BN statistics, BN + activation + pool + dropout forward, their backward with the BN sums,
// the BN input gradient, the transposed convolution's activation backward) are each one template over the channels a thread
// owns, V, and the index type, I.  Two instantiations of each run:
//   <4, unsigned>  C % 4 == 0 and 32-bit indices suffice (every layer of the shipped widths): four consecutive channels per
//                  thread, 16-byte loads and stores, the per-channel constants in registers, 32-bit index arithmetic.  The
//                  scalar form spends most of its time on 4-byte accesses and 64-bit index arithmetic there (act_bwd on lu0,
//                  19 M elements: 149 us against 50 us of memory time; leaky_bwd_s2d at 8 x 256 x 256 x 36: 146 us for 3 x 75 MB).
//   <1, size_t>    every other shape (the v2 head's 2 - 3 classes, odd test widths): one channel per thread, 64-bit indices
//                  (bn_bwd_apply's planes form: <1, unsigned>, its planes being limited to 32-bit indices anyway).
// The two do not sum a block's rows in the same order, so which one a shape takes is fixed by its launcher.
//
// An NHWC tensor is [N rows][C channels], i.e. [N rows][C / V units].  The reductions run blocks of Ub * R threads (Ub =
// min(C / V, 256), R = 256 / Ub) that walk R rows at a time: thread (r, u) always sees unit u, so per-channel sums live in
// registers and the loads are contiguous.  Their partials are part[block][2][C] (fp64, fixed order) for either V.
struct ChanLayout { int Ub, R, threads, cblocks; };
static inline ChanLayout chan_layout(int C, int V) {
    ChanLayout l;
    const int U = C / V;
    l.Ub = std::min(U, 256);
    l.R = std::max(1, 256 / l.Ub);
    l.threads = V == 1 ? l.Ub * l.R : 256;   // (the float4 reductions always run 256 threads; the spare ones idle)
    l.cblocks = (U + 255) / 256;
    return l;
}

int chan_blocks(size_t N, int C) {
    const ChanLayout l = chan_layout(C, 1);
    // (a handful of rows per block: the deep layers have 512 - 2048 rows, and 17 blocks walking 30 rows each left their
    //  activation-backward kernel latency-bound at 158 us for 1.2 MB -- round 4 time line)
    const size_t want = N / ((size_t)l.R * 4) + 1;
    const size_t cap = std::max(64, 1024 / l.cblocks);
    return (int)std::min<size_t>(cap, std::max<size_t>(1, want));
}

// unit i of p (V consecutive floats): one float4 or one float
template <int V> __device__ __forceinline__ void ldv(float (&d)[V], const float* p, size_t i = 0) {
    if constexpr (V == 4) {
        const float4 t = reinterpret_cast<const float4*>(p)[i];
        d[0] = t.x; d[1] = t.y; d[2] = t.z; d[3] = t.w;
    } else {
        d[0] = p[i];
    }
}
template <int V> __device__ __forceinline__ void stv(float* p, size_t i, const float (&s)[V]) {
    if constexpr (V == 4) reinterpret_cast<float4*>(p)[i] = make_float4(s[0], s[1], s[2], s[3]);
    else p[i] = s[0];
}
// V values as (hi, lo) binary16 pairs; bad: a value binary16 cannot hold
template <int V> __device__ __forceinline__ void st_planes(_Float16* hi, _Float16* lo, const float (&y)[V], bool& bad) {
    union { _Float16 h[4]; uint2 u; } a, b;
#pragma unroll
    for (int k = 0; k < V; ++k) {
        bad = bad || !(fabsf(y[k]) < 60000.f);
        a.h[k] = (_Float16)y[k];
        b.h[k] = (_Float16)(y[k] - (float)a.h[k]);
    }
    if constexpr (V == 4) {
        *reinterpret_cast<uint2*>(hi) = a.u;
        *reinterpret_cast<uint2*>(lo) = b.u;
    } else {
        *hi = a.h[0];
        *lo = b.h[0];
    }
}

template <int V, typename I>
__global__ void __launch_bounds__(256) chan_stats_kernel(const float* __restrict__ x, I N, int C, int Ub, int R,
                                                         double* __restrict__ part) {
    __shared__ double sm[2][256][V];
    const int tid = threadIdx.x;
    const int r = tid / Ub, ul = tid - r * Ub;
    const int U = C >> (V / 2), u = ul + blockIdx.y * 256;   // (U = C / V)
    const I rpb = (N + gridDim.x - 1) / gridDim.x;
    const I r0 = (I)blockIdx.x * rpb, r1 = min(N, r0 + rpb);
    double s[V] = {}, w[V] = {};
    if (r < R && u < U)
        for (I row = r0 + r; row < r1; row += R) {
            float xv[V];
            ldv<V>(xv, x, (size_t)row * U + u);
#pragma unroll
            for (int k = 0; k < V; ++k) {
                const double v = (double)xv[k];
                s[k] += v;
                w[k] += v * v;
            }
        }
#pragma unroll
    for (int k = 0; k < V; ++k) { sm[0][tid][k] = s[k]; sm[1][tid][k] = w[k]; }
    __syncthreads();
    if (r == 0 && u < U) {
#pragma unroll
        for (int k = 0; k < V; ++k) {
            for (int j = 1; j < R; ++j) { s[k] += sm[0][j * Ub + ul][k]; w[k] += sm[1][j * Ub + ul][k]; }
            part[((size_t)blockIdx.x * 2 + 0) * C + V * u + k] = s[k];
            part[((size_t)blockIdx.x * 2 + 1) * C + V * u + k] = w[k];
        }
    }
}

hipError_t launch_chan_stats(const float* x, size_t N, int C, double* part, int nblk, hipStream_t stream) {
    if (C % 4 == 0 && N < 0x7fffffffull) {
        const ChanLayout l = chan_layout(C, 4);
        hipLaunchKernelGGL((chan_stats_kernel<4, unsigned>), dim3((unsigned)nblk, (unsigned)l.cblocks), dim3(l.threads), 0, stream,
                           x, (unsigned)N, C, l.Ub, l.R, part);
        return hipGetLastError();
    }
    const ChanLayout l = chan_layout(C, 1);
    hipLaunchKernelGGL((chan_stats_kernel<1, size_t>), dim3((unsigned)nblk, (unsigned)l.cblocks), dim3(l.threads), 0, stream,
                       x, N, C, l.Ub, l.R, part);
    return hipGetLastError();
}

// fixed-order sum of the per-block partials of one channel by a 64-lane block: lane l adds partials l, l+64, ... in
// order, then a binary tree over the lanes
__device__ __forceinline__ void block64_sum2(double& a, double& b, double (*sm)[64]) {
    const int l = threadIdx.x;
    sm[0][l] = a;
    sm[1][l] = b;
    __syncthreads();
    for (int st = 32; st > 0; st >>= 1) {
        if (l < st) { sm[0][l] += sm[0][l + st]; sm[1][l] += sm[1][l + st]; }
        __syncthreads();
    }
    a = sm[0][0];
    b = sm[1][0];
}

__global__ void __launch_bounds__(64) bn_finalize_kernel(const double* __restrict__ part, int nblk, double N, int C,
                                                         const float* __restrict__ gamma, const float* __restrict__ beta,
                                                         float* mov_mean, float* mov_var, float momentum,
                                                         float* __restrict__ stat, unsigned* smax) {
    __shared__ double sm[2][64];
    const int c = blockIdx.x;
    double s = 0.0, q = 0.0;
    for (int b = threadIdx.x; b < nblk; b += 64) {
        s += part[((size_t)b * 2 + 0) * C + c];
        q += part[((size_t)b * 2 + 1) * C + c];
    }
    block64_sum2(s, q, sm);
    if (threadIdx.x != 0) return;
    const double mean = s / N;
    double var = q / N - mean * mean;
    if (var < 0.0) var = 0.0;
    const double rstd = 1.0 / sqrt(var + 1e-3);   // eps of tf.layers.batch_normalization in the reference graphs
    const double scale = (double)gamma[c] * rstd;
    stat[c] = (float)mean;
    stat[C + c] = (float)rstd;
    stat[2 * C + c] = (float)scale;
    stat[3 * C + c] = (float)((double)beta[c] - mean * scale);
    if (smax) atomicMax(smax, __float_as_uint(fabsf((float)scale)));   // max_c |gamma * rstd|: bounds the BN input gradient (bn_bwd_apply)
    const double mom = (double)momentum;
    const double unbiased = N > 1.0 ? var * (N / (N - 1.0)) : var;
    mov_mean[c] = (float)((double)mov_mean[c] * mom + mean * (1.0 - mom));
    mov_var[c] = (float)((double)mov_var[c] * mom + unbiased * (1.0 - mom));
}

hipError_t launch_bn_finalize(const double* part, int nblk, size_t N, int C, const float* gamma, const float* beta,
                              float* mov_mean, float* mov_var, float momentum, float* stat, unsigned* smax, hipStream_t stream) {
    hipLaunchKernelGGL(bn_finalize_kernel, dim3((unsigned)C), dim3(64), 0, stream, part, nblk, (double)N, C, gamma, beta,
                       mov_mean, mov_var, momentum, stat, smax);
    return hipGetLastError();
}

__global__ void __launch_bounds__(256) bn_stat_from_moving_kernel(int C, const float* __restrict__ gamma,
                                                                  const float* __restrict__ beta,
                                                                  const float* __restrict__ mov_mean,
                                                                  const float* __restrict__ mov_var,
                                                                  float* __restrict__ stat) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= C) return;
    const double rstd = 1.0 / sqrt((double)mov_var[c] + 1e-3);
    const double scale = (double)gamma[c] * rstd;
    stat[c] = mov_mean[c];
    stat[C + c] = (float)rstd;
    stat[2 * C + c] = (float)scale;
    stat[3 * C + c] = (float)((double)beta[c] - (double)mov_mean[c] * scale);
}

hipError_t launch_bn_stat_from_moving(int C, const float* gamma, const float* beta, const float* mov_mean,
                                      const float* mov_var, float* stat, hipStream_t stream) {
    hipLaunchKernelGGL(bn_stat_from_moving_kernel, dim3((unsigned)((C + 255) / 256)), dim3(256), 0, stream, C, gamma, beta,
                       mov_mean, mov_var, stat);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------ dropout stream
// == oracle/train_oracle.py dropout_mask: u = top 24 bits of mix(key ^ flat NHWC index); keep iff u >= rate
__device__ __forceinline__ unsigned long long mix64(unsigned long long x) {
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}
__device__ __forceinline__ float drop_mul(unsigned long long key, size_t idx, float rate, float keep_scale) {
    if (rate <= 0.f) return 1.f;
    const unsigned long long h = mix64((unsigned long long)idx ^ key);
    const float u = (float)(unsigned)(h >> 40) * (1.0f / 16777216.0f);
    return u >= rate ? keep_scale : 0.f;
}
__device__ __forceinline__ float act_of(float v, int act) {
    if (act == ACT_LEAKY) return v > 0.f ? v : 0.2f * v;
    if (act == ACT_RELU) return fmaxf(v, 0.f);
    return v;
}
__device__ __forceinline__ float dact_of(float v, int act) {
    if (act == ACT_LEAKY) return v > 0.f ? 1.f : 0.2f;
    if (act == ACT_RELU) return v > 0.f ? 1.f : 0.f;
    return 1.f;
}

// max |v| over a block -> one atomicMax on the tensor's word (uint order == float order for non-negative floats;
// integer max is associative: the result does not depend on the order of the blocks)
__device__ __forceinline__ void block_absmax_to(unsigned* dst, float v) {
    __shared__ unsigned smax[4];
    unsigned u = __float_as_uint(fabsf(v));
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) u = max(u, (unsigned)__shfl_xor((int)u, off));
    if ((threadIdx.x & 63) == 0) smax[threadIdx.x >> 6] = u;
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned m = max(max(smax[0], smax[1]), max(smax[2], smax[3]));
        // most blocks cannot raise the maximum once a few have reported: a plain (possibly stale, never too large) read
        // keeps them off the atomic unit; the atomic itself stays the arbiter
        if (m > *reinterpret_cast<volatile unsigned*>(dst)) atomicMax(dst, m);
    }
}

// (grid-stride over units; the block's max |output| goes to the tensor's max word with at most one atomic; hi != NULL: the
// output also as the (hi, lo) planes the next convolution reads, unscaled)
template <int V, typename I>
__global__ void __launch_bounds__(256) act_fwd_kernel(const ActParams a, float* __restrict__ out, I nu, unsigned* omax,
                                                      _Float16* __restrict__ hi, _Float16* __restrict__ lo, int Cs,
                                                      int* __restrict__ overflow) {
    const int C = a.C;
    const I U = (unsigned)C / V;
    const float ks = 1.0f / (1.0f - a.drop_rate);
    const I OW = a.W >> 1, OH = a.H >> 1;
    float mx = 0.f;
    bool bad = false;
    for (I i = (I)blockIdx.x * 256 + threadIdx.x; i < nu; i += (I)gridDim.x * 256) {
        const I row = i / U, u = i - row * U;
        const int c = V * (int)u;
        float sc[V], sh[V], y[V];
        ldv<V>(sc, a.stat + 2 * C + c);
        ldv<V>(sh, a.stat + 3 * C + c);
        if (!a.pool) {
            float zz[V];
            ldv<V>(zz, a.z, i);
            const size_t e = (size_t)row * C + c;
#pragma unroll
            for (int k = 0; k < V; ++k) y[k] = act_of(zz[k] * sc[k] + sh[k], a.act) * drop_mul(a.drop_key, e + k, a.drop_rate, ks);
        } else {
            const I ox = row % OW, t = row / OW, oy = t % OH, b = t / OH;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const size_t px = ((size_t)b * a.H + 2 * oy + (j >> 1)) * a.W + 2 * ox + (j & 1);
                float zz[V];
                ldv<V>(zz, a.z, px * U + u);
#pragma unroll
                for (int k = 0; k < V; ++k) {
                    const float yj = act_of(zz[k] * sc[k] + sh[k], a.act) * drop_mul(a.drop_key, px * C + c + k, a.drop_rate, ks);
                    if (j == 0 || yj > y[k]) y[k] = yj;
                }
            }
        }
        stv<V>(out, i, y);
#pragma unroll
        for (int k = 0; k < V; ++k) mx = fmaxf(mx, fabsf(y[k]));
        if (hi) {
            const size_t at = (size_t)row * Cs + c;
            st_planes<V>(hi + at, lo + at, y, bad);
        }
    }
    if (bad) atomicOr(overflow, 1);
    if (omax) block_absmax_to(omax, mx);
}

hipError_t launch_act_fwd(const ActParams& a, float* out, unsigned* omax, _Float16* hi, _Float16* lo, int Cs, int* overflow,
                          hipStream_t stream) {
    const size_t nout = (size_t)a.B * (a.pool ? a.H / 2 : a.H) * (a.pool ? a.W / 2 : a.W) * a.C;
    if (a.C % 4 == 0 && (!hi || Cs % 4 == 0) && nout < 0xfffffff0ull) {
        const unsigned nq = (unsigned)(nout / 4);
        const unsigned blocks = std::min<unsigned>(4096, (nq + 255) / 256);
        hipLaunchKernelGGL((act_fwd_kernel<4, unsigned>), dim3(blocks ? blocks : 1), dim3(256), 0, stream, a, out, nq, omax, hi, lo, Cs,
                           overflow);
        return hipGetLastError();
    }
    const unsigned blocks = (unsigned)std::min<size_t>(2048, (nout + 255) / 256);
    hipLaunchKernelGGL((act_fwd_kernel<1, size_t>), dim3(blocks ? blocks : 1), dim3(256), 0, stream, a, out, nout, omax, hi, lo, Cs,
                       overflow);
    return hipGetLastError();
}

__global__ void __launch_bounds__(256) absmax_kernel(const float* __restrict__ x, size_t n, unsigned* omax) {
    float mx = 0.f;
    for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < n; e += (size_t)gridDim.x * 256) mx = fmaxf(mx, fabsf(x[e]));
    block_absmax_to(omax, mx);
}

hipError_t launch_absmax(const float* x, size_t n, unsigned* omax, hipStream_t stream) {
    const unsigned blocks = (unsigned)std::min<size_t>(4096, (n + 255) / 256);
    hipLaunchKernelGGL(absmax_kernel, dim3(blocks ? blocks : 1), dim3(256), 0, stream, x, n, omax);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------------------
// Forward / input-gradient convolutions on conv_f16x3 (round 4).  The filters change every step: this kernel gathers them into
// the LDS-image order the planner laid out once (HWRef, umx_internal.h) -- straight from the master tensors where the trainer
// could rewrite the planner's references into master coordinates (estride != 0), else from the fp32 operands [tap][Cp][Np]
// pack_weights_kernel rebuilds -- scaled by the power of two that puts the layer's largest |w| of the START of training in
// [2^10, 2^11) -- 32 x headroom; a weight that outgrows binary16 raises the range flag -- as (hi, lo) binary16 pairs.
// One thread per 16-byte unit; consecutive lanes read consecutive output channels of the fp32 operand (coalesced per element).
// ------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) repack_f16x3_kernel(const RepackDesc* __restrict__ descs, int* __restrict__ overflow) {
    const RepackDesc d = descs[blockIdx.y];
    bool bad = false;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < d.n; i += gridDim.x * 256) {
        const HWRefDev r = d.refs[i];
        const float* const src = d.arr[r.arr] + r.base;
        const float* const src2 = d.arr2[r.arr] ? d.arr2[r.arr] + r.base : nullptr;
        const int es = d.estride[r.arr] ? d.estride[r.arr] : d.stride;
        union { _Float16 h[8]; uint4 u; } vh, vl;
        vh.u = make_uint4(0, 0, 0, 0);
        vl.u = make_uint4(0, 0, 0, 0);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            if (e < (int)r.nvalid) {
                float w = src[(size_t)e * es];
                if (src2) w += src2[(size_t)e * es];   // (the sum pack_weights_kernel makes, same order)
                const float v = w * d.scale;
                bad = bad || !(fabsf(v) < 60000.f);
                vh.h[e] = (_Float16)v;
                vl.h[e] = (_Float16)(v - (float)vh.h[e]);
            }
        }
        d.slab[r.dst] = vh.u;
        d.slab[r.dst + 64] = vl.u;
    }
    if (bad) atomicOr(overflow, 1);
}

hipError_t launch_repack_f16x3(const RepackDesc* descs_dev, int ndesc, int max_n, int* overflow, hipStream_t stream) {
    if (ndesc <= 0) return hipSuccess;
    const unsigned bx = (unsigned)std::min(512, (max_n + 255) / 256);
    hipLaunchKernelGGL(repack_f16x3_kernel, dim3(bx ? bx : 1, (unsigned)ndesc), dim3(256), 0, stream, descs_dev, overflow);
    return hipGetLastError();
}

// fp32 NHWC [npix, C] -> (hi, lo) binary16 NHWC [npix, Cs] (Cs = C rounded up to 8, pad channels zero) for conv_f16x3.  `maxw`
// (nullable): the tensor's max |v| as float bits, written by its producer -- a gradient tensor is scaled by the power of two that
// puts that maximum in [2^11, 2^12) (gradients would flush to zero otherwise) and the inverse factor goes to *inv_scale for the
// consuming convolution's epilogue (HConvParams::dyn); without it the tensor is stored as it is.  Non-finite or out-of-range
// values raise the flag.
__global__ void __launch_bounds__(256) split_dyn_kernel(const float* __restrict__ x, size_t npix, int C, int Cs,
                                                       const unsigned* __restrict__ maxw, float* __restrict__ inv_scale,
                                                       _Float16* __restrict__ hi, _Float16* __restrict__ lo, int* __restrict__ overflow,
                                                       unsigned* __restrict__ omax) {
    float scale = 1.f, mx = 0.f;   // (omax: the tensor's max |v| for the weight-gradient kernel, one integer atomicMax per block)
    if (maxw) {
        const unsigned mb = *maxw;
        const int e = (int)((mb >> 23) & 0xFFu);
        if (mb != 0u && e > 0 && e < 255) {
            const int sh = max(-100, min(100, 11 - (e - 127)));
            scale = __uint_as_float((unsigned)(127 + sh) << 23);
        }
        if (inv_scale && blockIdx.x == 0 && threadIdx.x == 0) *inv_scale = 1.f / scale;
    }
    const size_t total = npix * (size_t)Cs;
    bool bad = false;
    if ((C & 3) == 0 && Cs == C) {   // whole float4 / 8-byte units
        const size_t n4 = total / 4;
        for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (size_t)gridDim.x * 256) {
            float f[4];
            ldv<4>(f, x, i);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                f[k] *= scale;
                mx = fmaxf(mx, fabsf(f[k]));
            }
            st_planes<4>(hi + 4 * i, lo + 4 * i, f, bad);
        }
    } else {
        for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (size_t)gridDim.x * 256) {
            const size_t px = e / Cs;
            const int c = (int)(e - px * Cs);
            const float v[1] = {c < C ? x[px * C + c] * scale : 0.f};
            mx = fmaxf(mx, fabsf(v[0]));
            st_planes<1>(hi + e, lo + e, v, bad);
        }
    }
    if (bad) atomicOr(overflow, 1);
    if (omax) block_absmax_to(omax, mx);   // (only asked for unscaled tensors: scale == 1)
}

hipError_t launch_split_dyn(const float* x, size_t npix, int C, int Cs, const unsigned* maxw, float* inv_scale, _Float16* hi,
                            _Float16* lo, int* overflow, unsigned* omax, hipStream_t stream) {
    if (npix == 0) return hipSuccess;
    const size_t total = npix * (size_t)Cs;
    const unsigned blocks = (unsigned)std::min<size_t>(4096, (total / 4 + 255) / 256 + 1);
    hipLaunchKernelGGL(split_dyn_kernel, dim3(blocks), dim3(256), 0, stream, x, npix, C, Cs, maxw, inv_scale, hi, lo, overflow, omax);
    return hipGetLastError();
}

// (max |g| and max |xhat| of the block go to gx[0], gx[1]: with max |gamma rstd| they bound |dz| (bn_bwd_apply))
template <int V, typename I>
__global__ void __launch_bounds__(256) act_bwd_kernel(const ActParams a, const float* __restrict__ dy0,
                                                      const float* __restrict__ dy1, float* __restrict__ g, I Nrows,
                                                      int Ub, int R, double* __restrict__ part, unsigned* gx) {
    __shared__ double sm[2][256][V];
    __shared__ unsigned smx[2][256];
    const int tid = threadIdx.x;
    const int r = tid / Ub, ul = tid - r * Ub;
    const int C = a.C, U = C >> (V / 2);   // (U = C / V)
    const int u = ul + blockIdx.y * 256;
    const I rpb = (Nrows + gridDim.x - 1) / gridDim.x;
    const I r0 = (I)blockIdx.x * rpb, r1 = min(Nrows, r0 + rpb);
    double s1[V] = {}, s2[V] = {};
    float mg = 0.f, mxh = 0.f;
    if (r < R && u < U) {
        const int c = V * u;
        float mean[V], rstd[V], sc[V], sh[V];
        ldv<V>(mean, a.stat + c);
        ldv<V>(rstd, a.stat + C + c);
        ldv<V>(sc, a.stat + 2 * C + c);
        ldv<V>(sh, a.stat + 3 * C + c);
        const float ks = 1.0f / (1.0f - a.drop_rate);
        const I OW = a.W >> 1, OH = a.H >> 1;
        for (I row = r0 + r; row < r1; row += R) {
            const size_t o = (size_t)row * U + u;
            float d[V];
            ldv<V>(d, dy0, o);
            if (dy1) {
                float d1[V];
                ldv<V>(d1, dy1, o);
#pragma unroll
                for (int k = 0; k < V; ++k) d[k] += d1[k];
            }
            if (!a.pool) {
                const size_t e = (size_t)row * C + c;
                float zz[V], gg[V];
                ldv<V>(zz, a.z, o);
#pragma unroll
                for (int k = 0; k < V; ++k) {
                    const float v = zz[k] * sc[k] + sh[k];
                    gg[k] = d[k] * drop_mul(a.drop_key, e + k, a.drop_rate, ks) * dact_of(v, a.act);
                    const float xh = (zz[k] - mean[k]) * rstd[k];
                    s1[k] += (double)gg[k];
                    s2[k] += (double)gg[k] * (double)xh;
                    mg = fmaxf(mg, fabsf(gg[k]));
                    mxh = fmaxf(mxh, fabsf(xh));
                }
                stv<V>(g, o, gg);
            } else {
                const I ox = row % OW, t = row / OW, oy = t % OH, b = t / OH;
                size_t ow[4];   // (unit index of each pixel of the window)
                float zz[4][V], vv[4][V], dm[4][V];
                int arg[V] = {};
                float best[V] = {};
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const size_t px = ((size_t)b * a.H + 2 * oy + (j >> 1)) * a.W + 2 * ox + (j & 1);
                    ow[j] = px * U + u;
                    ldv<V>(zz[j], a.z, ow[j]);
#pragma unroll
                    for (int k = 0; k < V; ++k) {
                        vv[j][k] = zz[j][k] * sc[k] + sh[k];
                        dm[j][k] = drop_mul(a.drop_key, px * C + c + k, a.drop_rate, ks);
                        const float y = act_of(vv[j][k], a.act) * dm[j][k];
                        if (j == 0 || y > best[k]) { best[k] = y; arg[k] = j; }
                    }
                }
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    float gg[V];
#pragma unroll
                    for (int k = 0; k < V; ++k) {
                        gg[k] = j == arg[k] ? d[k] * dm[j][k] * dact_of(vv[j][k], a.act) : 0.f;
                        const float xh = (zz[j][k] - mean[k]) * rstd[k];
                        mxh = fmaxf(mxh, fabsf(xh));
                        if (j == arg[k]) {
                            s1[k] += (double)gg[k];
                            s2[k] += (double)gg[k] * (double)xh;
                            mg = fmaxf(mg, fabsf(gg[k]));
                        }
                    }
                    stv<V>(g, ow[j], gg);
                }
            }
        }
    }
#pragma unroll
    for (int k = 0; k < V; ++k) { sm[0][tid][k] = s1[k]; sm[1][tid][k] = s2[k]; }
    smx[0][tid] = __float_as_uint(mg);
    smx[1][tid] = __float_as_uint(mxh);
    __syncthreads();
    if (r == 0 && u < U) {
#pragma unroll
        for (int k = 0; k < V; ++k) {
            for (int j = 1; j < R; ++j) { s1[k] += sm[0][j * Ub + ul][k]; s2[k] += sm[1][j * Ub + ul][k]; }
            part[((size_t)blockIdx.x * 2 + 0) * C + V * u + k] = s1[k];
            part[((size_t)blockIdx.x * 2 + 1) * C + V * u + k] = s2[k];
        }
    }
    if (gx && tid < 2) {   // (over the Ub * R threads that walk rows; integer max of non-negative float bits: order-independent)
        unsigned m = 0u;
        for (int j = 0; j < Ub * R; ++j) m = max(m, smx[tid][j]);
        if (m > *reinterpret_cast<volatile unsigned*>(gx + tid)) atomicMax(gx + tid, m);
    }
}

hipError_t launch_act_bwd(const ActParams& a, const float* dy0, const float* dy1, float* g, double* part, int nblk,
                          unsigned* gx, hipStream_t stream) {
    const size_t rows = (size_t)a.B * (a.pool ? a.H / 2 : a.H) * (a.pool ? a.W / 2 : a.W);
    if (a.C % 4 == 0 && rows < 0x7fffffffull) {
        const ChanLayout l = chan_layout(a.C, 4);
        hipLaunchKernelGGL((act_bwd_kernel<4, unsigned>), dim3((unsigned)nblk, (unsigned)l.cblocks), dim3(l.threads), 0, stream, a, dy0,
                           dy1, g, (unsigned)rows, l.Ub, l.R, part, gx);
        return hipGetLastError();
    }
    const ChanLayout l = chan_layout(a.C, 1);
    hipLaunchKernelGGL((act_bwd_kernel<1, size_t>), dim3((unsigned)nblk, (unsigned)l.cblocks), dim3(l.threads), 0, stream, a, dy0,
                       dy1, g, rows, l.Ub, l.R, part, gx);
    return hipGetLastError();
}

__global__ void __launch_bounds__(64) bn_bwd_finalize_kernel(const double* __restrict__ part, int nblk, double N, int C,
                                                             float* dgamma, float* dbeta, float* __restrict__ m12) {
    __shared__ double sm[2][64];
    const int c = blockIdx.x;
    double s1 = 0.0, s2 = 0.0;
    for (int b = threadIdx.x; b < nblk; b += 64) {
        s1 += part[((size_t)b * 2 + 0) * C + c];
        s2 += part[((size_t)b * 2 + 1) * C + c];
    }
    block64_sum2(s1, s2, sm);
    if (threadIdx.x != 0) return;
    m12[c] = (float)(s1 / N);
    m12[C + c] = (float)(s2 / N);
    dgamma[c] = (float)s2;
    dbeta[c] = (float)s1;
}

hipError_t launch_bn_bwd_finalize(const double* part, int nblk, size_t N, int C, float* dgamma, float* dbeta, float* m12,
                                  hipStream_t stream) {
    hipLaunchKernelGGL(bn_bwd_finalize_kernel, dim3((unsigned)C), dim3(64), 0, stream, part, nblk, (double)N, C, dgamma,
                       dbeta, m12);
    return hipGetLastError();
}

// dz = gamma rstd (g - mean g - xhat mean(g xhat)) in place (grid-stride over units; at most one atomic per block on the tensor's
// max word).  PLANES: the (hi, lo) planes conv_f16x3's input-gradient launches read, written in the same pass (round 4; no second
// trip through the tensor).  Their power-of-two scale has to be known before the first element: |dz| <= max_c|gamma rstd| * (|g| +
// |mean g| + |xhat| |mean g xhat|) <= smax * gmax * (2 + xhmax)  (|mean g| <= gmax, |mean g xhat| <= gmax * E|xhat| <= gmax), the
// three maxima tracked by bn_finalize / act_bwd -- a true bound, 2^2 .. 2^3 above the real maximum, placed at 2^14.
template <int V, typename I, bool PLANES>
__global__ void __launch_bounds__(256) bn_bwd_apply_kernel(float* __restrict__ g, const float* __restrict__ z,
                                                           const float* __restrict__ stat, const float* __restrict__ m12,
                                                           I n, int C, int Cs, unsigned* gmax, const unsigned* __restrict__ bw,
                                                           float* __restrict__ inv_scale, _Float16* __restrict__ hi,
                                                           _Float16* __restrict__ lo, int* __restrict__ overflow) {
    float scale = 1.f;
    if constexpr (PLANES) {
        const float bound = __uint_as_float(bw[0]) * __uint_as_float(bw[1]) * (2.f + __uint_as_float(bw[2]));
        const unsigned bb = __float_as_uint(bound);
        const int e = (int)((bb >> 23) & 0xFFu);
        if (bb != 0u && e > 0 && e < 255) {
            const int sh = max(-100, min(100, 14 - (e - 127)));   // bound -> [2^14, 2^15)
            scale = __uint_as_float((unsigned)(127 + sh) << 23);
        }
        if (blockIdx.x == 0 && threadIdx.x == 0) *inv_scale = 1.f / scale;
    }
    float mx = 0.f;
    bool bad = false;
    const I nu = n / V;
    for (I i = (I)blockIdx.x * 256 + threadIdx.x; i < nu; i += (I)gridDim.x * 256) {
        const I e = i * V, px = e / (I)C;
        const int c = (int)(e - px * (I)C);
        float gv[V], zv[V], mean[V], rstd[V], sc[V], m1[V], m2[V], v[V];
        ldv<V>(gv, g, i);
        ldv<V>(zv, z, i);
        ldv<V>(mean, stat + c);
        ldv<V>(rstd, stat + (C + c));
        ldv<V>(sc, stat + (2 * C + c));
        ldv<V>(m1, m12 + c);
        ldv<V>(m2, m12 + (C + c));
#pragma unroll
        for (int k = 0; k < V; ++k) v[k] = sc[k] * (gv[k] - m1[k] - (zv[k] - mean[k]) * rstd[k] * m2[k]);
        stv<V>(g, i, v);
        float f[V];
#pragma unroll
        for (int k = 0; k < V; ++k) {
            mx = fmaxf(mx, fabsf(v[k]));
            f[k] = v[k] * scale;
        }
        if constexpr (PLANES) {
            const size_t at = (size_t)px * Cs + c;
            st_planes<V>(hi + at, lo + at, f, bad);
            if (c + V == C) {   // the pad channels C .. Cs-1 of the pixel's last octet (the slot is shared between layers)
                const float zero[V] = {};
#pragma unroll
                for (int k = V; k < 8; k += V)   // (Cs - C < 8: launch_bn_bwd_apply_max)
                    if (c + k < Cs) st_planes<V>(hi + at + k, lo + at + k, zero, bad);
            }
        }
    }
    if (bad) atomicOr(overflow, 1);
    if (gmax) block_absmax_to(gmax, mx);
}

// (hi == NULL: the fp32 tensor only -- the top layer, the first down layer, the exact-fp32 route)
hipError_t launch_bn_bwd_apply_max(float* g, const float* z, const float* stat, const float* m12, size_t N, int C,
                                   unsigned* gmax, const unsigned* bw, float* inv_scale, _Float16* hi, _Float16* lo, int Cs,
                                   int* overflow, hipStream_t stream) {
    const size_t n = N * C;
    const unsigned blocks = (unsigned)std::min<size_t>(1024, (n + 255) / 256);
    // (planes asked for on a tensor the 32-bit-index kernel cannot address: refuse -- the caller's convolutions and weight
    // gradients would read planes and an inverse scale nobody wrote.  Batch x resolution x channels >= 2^32: not a shape of this graph)
    if (hi && n >= 0xFFFFFFF0ull) return hipErrorInvalidValue;
    if (hi && (Cs < C || Cs - C >= 8)) return hipErrorInvalidValue;   // (the planes are C rounded up to 8 channels)
    if (hi) {
        const unsigned bv = (unsigned)std::min<size_t>(2048, (n / 4 + 255) / 256 + 1);
        if (C % 4 == 0 && Cs % 4 == 0)
            hipLaunchKernelGGL((bn_bwd_apply_kernel<4, unsigned, true>), dim3(bv), dim3(256), 0, stream, g, z, stat, m12, (unsigned)n, C, Cs,
                               gmax, bw, inv_scale, hi, lo, overflow);
        else
            hipLaunchKernelGGL((bn_bwd_apply_kernel<1, unsigned, true>), dim3(blocks ? blocks : 1), dim3(256), 0, stream, g, z, stat, m12,
                               (unsigned)n, C, Cs, gmax, bw, inv_scale, hi, lo, overflow);
        return hipGetLastError();
    }
    hipLaunchKernelGGL((bn_bwd_apply_kernel<1, size_t, false>), dim3(blocks ? blocks : 1), dim3(256), 0, stream, g, z, stat, m12, n, C, 0,
                       gmax, nullptr, nullptr, nullptr, nullptr, nullptr);
    return hipGetLastError();
}

template <int V, typename I>
__global__ void __launch_bounds__(256) leaky_bwd_s2d_kernel(const float* __restrict__ d_us, const float* __restrict__ us, I S, I U,
                                                            float* __restrict__ gS, I nu, float slope, unsigned* gmax) {
    float mx = 0.f;
    for (I e = (I)blockIdx.x * 256 + threadIdx.x; e < nu; e += (I)gridDim.x * 256) {
        const I u = e % U;
        I r = e / U;
        const I q = r & 3; r >>= 2;
        const I j = r % S; r /= S;
        const I i = r % S;
        const I b = r / S;
        const I src = ((b * (2 * S) + 2 * i + (q >> 1)) * (2 * S) + 2 * j + (q & 1)) * U + u;
        float d[V], y[V], v[V];
        ldv<V>(d, d_us, src);
        ldv<V>(y, us, src);
#pragma unroll
        for (int k = 0; k < V; ++k) v[k] = d[k] * (y[k] > 0.f ? 1.f : slope);
        stv<V>(gS, e, v);
#pragma unroll
        for (int k = 0; k < V; ++k) mx = fmaxf(mx, fabsf(v[k]));
    }
    if (gmax) block_absmax_to(gmax, mx);
}

hipError_t launch_leaky_bwd_s2d_max(const float* d_us, const float* us, int B, int S, int C, float slope, float* gS, unsigned* gmax,
                                    hipStream_t stream) {
    const size_t n = (size_t)B * S * S * 4 * C;
    if (C % 4 == 0 && n < 0xffffffffull) {
        const unsigned n4 = (unsigned)(n / 4);
        const unsigned blocks = std::min(2048u, (n4 + 255u) / 256u);
        hipLaunchKernelGGL((leaky_bwd_s2d_kernel<4, unsigned>), dim3(blocks ? blocks : 1), dim3(256), 0, stream, d_us, us, (unsigned)S,
                           (unsigned)(C / 4), gS, n4, slope, gmax);
        return hipGetLastError();
    }
    const unsigned blocks = (unsigned)std::min<size_t>(1024, (n + 255) / 256);
    hipLaunchKernelGGL((leaky_bwd_s2d_kernel<1, size_t>), dim3(blocks ? blocks : 1), dim3(256), 0, stream, d_us, us, (size_t)S, (size_t)C,
                       gS, n, slope, gmax);
    return hipGetLastError();
}

// ReLU backward of the legacy graph (reference UnMicst.py:92,101,114,157,163): g = dy where v > 0, else 0 (v: the value in
// front of the ReLU, or behind it -- the same decision); in place allowed; tracks max |g| for the planes and weight gradients
__global__ void __launch_bounds__(256) relu_bwd_kernel(const float* dy, const float* __restrict__ v, float* g,
                                                       size_t n, unsigned* gmax) {
    float mx = 0.f;
    for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < n; e += (size_t)gridDim.x * 256) {
        const float r = v[e] > 0.f ? dy[e] : 0.f;
        g[e] = r;
        mx = fmaxf(mx, fabsf(r));
    }
    if (gmax) block_absmax_to(gmax, mx);
}

hipError_t launch_relu_bwd_max(const float* dy, const float* v, float* g, size_t n, unsigned* gmax, hipStream_t stream) {
    const unsigned blocks = (unsigned)std::min<size_t>(2048, (n + 255) / 256);
    hipLaunchKernelGGL(relu_bwd_kernel, dim3(blocks ? blocks : 1), dim3(256), 0, stream, dy, v, g, n, gmax);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------ top layer
constexpr int kMaxK = 8;

// 256 pixels per block: the [256][C] slab is loaded with consecutive threads on consecutive addresses and parked in LDS
// (pixel pitch C+1: a thread walking its own pixel then touches a new bank every step), each thread reduces one pixel
__global__ void __launch_bounds__(256) head_fwd_kernel(const float* __restrict__ x, size_t N, int C, int K,
                                                       const float* __restrict__ w, float* __restrict__ t0) {
    extern __shared__ float hl[];    // [C][K] weights, then [256][C+1] pixels
    float* const wl = hl;
    float* const xl = hl + C * K;
    const size_t p0 = (size_t)blockIdx.x * 256;
    const int npx = (int)min((size_t)256, N - p0);
    for (int i = threadIdx.x; i < C * K; i += 256) wl[i] = w[i];
    for (int i = threadIdx.x; i < npx * C; i += 256) {
        const int px = i / C, c = i - px * C;
        xl[px * (C + 1) + c] = x[p0 * C + i];
    }
    __syncthreads();
    if ((int)threadIdx.x >= npx) return;
    float acc[kMaxK];
#pragma unroll
    for (int k = 0; k < kMaxK; ++k) acc[k] = 0.f;
    const float* xp = xl + threadIdx.x * (C + 1);
    for (int c = 0; c < C; ++c) {
        const float v = xp[c];
#pragma unroll
        for (int k = 0; k < kMaxK; ++k)
            if (k < K) acc[k] = fmaf(v, wl[c * K + k], acc[k]);
    }
    const size_t p = p0 + threadIdx.x;
#pragma unroll
    for (int k = 0; k < kMaxK; ++k)
        if (k < K) t0[p * K + k] = acc[k];
}

hipError_t launch_head_fwd(const float* x, size_t N, int C, int K, const float* w, float* t0, hipStream_t stream) {
    if (K > kMaxK) return hipErrorInvalidValue;
    const size_t lds = sizeof(float) * ((size_t)C * K + 256 * (size_t)(C + 1));
    if (lds > 160 * 1024) return hipErrorInvalidValue;
    if (lds > 64 * 1024) {   // (nOut0 > 63, the solo model's 80 features: more dynamic LDS than a kernel gets by default)
        static std::once_flag once;
        static hipError_t err = hipSuccess;
        std::call_once(once, [] {
            err = hipFuncSetAttribute(reinterpret_cast<const void*>(head_fwd_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
        });
        if (err != hipSuccess) return err;
    }
    hipLaunchKernelGGL(head_fwd_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), lds, stream, x, N, C, K, w, t0);
    return hipGetLastError();
}

int loss_blocks(size_t N) { return (int)std::min<size_t>(1024, (N + 255) / 256); }

// reference UnMicst1-5.py:362-367: mean over pixels of -sum_k weights*labels*log(clip(p, eps, 1-eps)); duo: log(p)
__global__ void __launch_bounds__(256) softmax_loss_kernel(const float* __restrict__ t0, const float* __restrict__ stat,
                                                           const float* __restrict__ labels,
                                                           const float* __restrict__ weights, size_t N, int K,
                                                           float clip_eps, float* __restrict__ probs,
                                                           float* __restrict__ dt, double* __restrict__ part) {
    __shared__ double sm[256];
    double lsum = 0.0;
    const float invN = (float)(1.0 / (double)N);
    for (size_t p = (size_t)blockIdx.x * 256 + threadIdx.x; p < N; p += (size_t)gridDim.x * 256) {
        float t[kMaxK], pr[kMaxK], dp[kMaxK];
        float mx = -3.0e38f;
#pragma unroll
        for (int k = 0; k < kMaxK; ++k)
            if (k < K) { t[k] = t0[p * K + k] * stat[2 * K + k] + stat[3 * K + k]; mx = fmaxf(mx, t[k]); }
        float den = 0.f;
#pragma unroll
        for (int k = 0; k < kMaxK; ++k)
            if (k < K) { pr[k] = expf(t[k] - mx); den += pr[k]; }
        float dot = 0.f, L = 0.f;
#pragma unroll
        for (int k = 0; k < kMaxK; ++k)
            if (k < K) {
                pr[k] = pr[k] / den;
                const float wy = weights[p * K + k] * labels[p * K + k];
                float pc = pr[k];
                bool pass = true;
                if (clip_eps > 0.f) {
                    pass = pc >= clip_eps && pc <= 1.0f - clip_eps;
                    pc = fminf(fmaxf(pc, clip_eps), 1.0f - clip_eps);
                }
                L -= wy * logf(pc);
                dp[k] = (pass && wy != 0.f) ? -wy / pc : 0.f;
                dot += dp[k] * pr[k];
                if (probs) probs[p * K + k] = pr[k];
            }
#pragma unroll
        for (int k = 0; k < kMaxK; ++k)
            if (k < K) dt[p * K + k] = pr[k] * (dp[k] - dot) * invN;
        lsum += (double)L;
    }
    sm[threadIdx.x] = lsum;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) sm[threadIdx.x] += sm[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) part[blockIdx.x] = sm[0];
}

hipError_t launch_softmax_loss(const float* t0, const float* stat, const float* labels, const float* weights, size_t N,
                               int K, float clip_eps, float* probs, float* dt, double* part, int nblk, hipStream_t stream) {
    if (K > kMaxK) return hipErrorInvalidValue;
    hipLaunchKernelGGL(softmax_loss_kernel, dim3((unsigned)nblk), dim3(256), 0, stream, t0, stat, labels, weights, N, K,
                       clip_eps, probs, dt, part);
    return hipGetLastError();
}

__global__ void __launch_bounds__(256) softmax_only_kernel(const float* __restrict__ t0, const float* __restrict__ stat,
                                                           size_t N, int K, float* __restrict__ probs) {
    const size_t p = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= N) return;
    float t[kMaxK];
    float mx = -3.0e38f, den = 0.f;
#pragma unroll
    for (int k = 0; k < kMaxK; ++k)
        if (k < K) { t[k] = t0[p * K + k] * stat[2 * K + k] + stat[3 * K + k]; mx = fmaxf(mx, t[k]); }
#pragma unroll
    for (int k = 0; k < kMaxK; ++k)
        if (k < K) { t[k] = expf(t[k] - mx); den += t[k]; }
#pragma unroll
    for (int k = 0; k < kMaxK; ++k)
        if (k < K) probs[p * K + k] = t[k] / den;
}

hipError_t launch_softmax_only(const float* t0, const float* stat, size_t N, int K, float* probs, hipStream_t stream) {
    if (K > kMaxK) return hipErrorInvalidValue;
    hipLaunchKernelGGL(softmax_only_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, stream, t0, stat, N, K, probs);
    return hipGetLastError();
}

__global__ void __launch_bounds__(256) head_bwd_kernel(const float* __restrict__ x, const float* __restrict__ dt0,
                                                       const float* __restrict__ w, size_t N, int C, int K, int Cb, int k,
                                                       float* __restrict__ dx, double* __restrict__ part) {
    __shared__ double sm[kMaxK][256];
    const int tid = threadIdx.x;
    const int r = tid / Cb, cl = tid - r * Cb;
    const int c = cl + blockIdx.y * 256;
    const size_t rpb = (N + gridDim.x - 1) / gridDim.x;
    const size_t r0 = (size_t)blockIdx.x * rpb, r1 = std::min(N, r0 + rpb);
    double acc[kMaxK];
    float wk[kMaxK];
#pragma unroll
    for (int j = 0; j < kMaxK; ++j) { acc[j] = 0.0; wk[j] = (c < C && j < K) ? w[c * K + j] : 0.f; }
    if (c < C)
        for (size_t row = r0 + r; row < r1; row += k) {
            const float xv = x[row * C + c];
            float d = 0.f;
#pragma unroll
            for (int j = 0; j < kMaxK; ++j)
                if (j < K) {
                    const float g = dt0[row * K + j];
                    acc[j] += (double)xv * (double)g;
                    d = fmaf(g, wk[j], d);
                }
            dx[row * C + c] = d;
        }
#pragma unroll
    for (int j = 0; j < kMaxK; ++j) sm[j][tid] = acc[j];
    __syncthreads();
    if (r == 0 && c < C) {
#pragma unroll
        for (int j = 0; j < kMaxK; ++j)
            if (j < K) {
                double s = acc[j];
                for (int i = 1; i < k; ++i) s += sm[j][i * Cb + cl];
                part[((size_t)blockIdx.x * C + c) * K + j] = s;
            }
    }
}

hipError_t launch_head_bwd(const float* x, const float* dt0, const float* w, size_t N, int C, int K, float* dx,
                           double* part, int nblk, hipStream_t stream) {
    if (K > kMaxK) return hipErrorInvalidValue;
    const ChanLayout l = chan_layout(C, 1);
    hipLaunchKernelGGL(head_bwd_kernel, dim3((unsigned)nblk, (unsigned)l.cblocks), dim3((unsigned)l.threads), 0, stream, x,
                       dt0, w, N, C, K, l.Ub, l.R, dx, part);
    return hipGetLastError();
}

__global__ void __launch_bounds__(64) reduce_partials_kernel(const double* __restrict__ part, int nblk, int n,
                                                             double scale, float* __restrict__ dst,
                                                             const float* __restrict__ w, int reg_kind, float reg_c) {
    __shared__ double sm[2][64];
    const int i = blockIdx.x;
    double s = 0.0, unused = 0.0;
    for (int b = threadIdx.x; b < nblk; b += 64) s += part[(size_t)b * n + i];
    block64_sum2(s, unused, sm);
    if (threadIdx.x != 0) return;
    float v = (float)(s * scale);
    if (w && reg_kind) v += reg_grad(w[i], reg_kind, reg_c);
    dst[i] = v;
}

hipError_t launch_reduce_partials(const double* part, int nblk, int n, double scale, float* dst, const float* w,
                                  int reg_kind, float reg_c, hipStream_t stream) {
    hipLaunchKernelGGL(reduce_partials_kernel, dim3((unsigned)n), dim3(64), 0, stream, part, nblk, n, scale, dst, w,
                       reg_kind, reg_c);
    return hipGetLastError();
}

// (one block of 256: thread t adds the contiguous run [t * per, (t + 1) * per) in order, thread 0 adds the 256 run sums in order --
//  a fixed order; the single-thread loop it replaces took 61 us for 1024 partials at the head of the backward pass)
__global__ void __launch_bounds__(256) sum_to_scalar_kernel(const double* __restrict__ part, int n, double scale, double* out, int slot,
                                                            int accumulate) {
    __shared__ double sm[256];
    const int per = (n + 255) / 256;
    const int i0 = threadIdx.x * per, i1 = min(n, i0 + per);
    double s = 0.0;
    for (int i = i0; i < i1; ++i) s += part[i];
    sm[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x != 0) return;
    double t = 0.0;
    for (int j = 0; j < 256; ++j) t += sm[j];
    t *= scale;
    out[slot] = accumulate ? out[slot] + t : t;
}

hipError_t launch_sum_to_scalar(const double* part, int n, double scale, double* out, int slot, int accumulate,
                                hipStream_t stream) {
    hipLaunchKernelGGL(sum_to_scalar_kernel, dim3(1), dim3(256), 0, stream, part, n, scale, out, slot, accumulate);
    return hipGetLastError();
}

// regularisation loss of every regularised tensor in two launches: part[seg][64] = sum |w| or w^2 over a strided share,
// then out[slot] += sum_seg coef[seg] * sum_b part[seg][b]
__global__ void __launch_bounds__(256) reg_partials_kernel(const RegSeg* __restrict__ segs, int kind,
                                                           double* __restrict__ part) {
    __shared__ double sm[256];
    const RegSeg sg = segs[blockIdx.y];
    double s = 0.0;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < sg.n; i += (size_t)gridDim.x * 256) {
        const double v = (double)sg.w[i];
        s += kind == 1 ? fabs(v) : v * v;
    }
    sm[threadIdx.x] = s;
    __syncthreads();
    for (int st = 128; st > 0; st >>= 1) {
        if ((int)threadIdx.x < st) sm[threadIdx.x] += sm[threadIdx.x + st];
        __syncthreads();
    }
    if (threadIdx.x == 0) part[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = sm[0];
}

__global__ void reg_finalize_kernel(const RegSeg* __restrict__ segs, int nseg, const double* __restrict__ part, int nb,
                                    double* out, int slot) {
    double total = 0.0;
    for (int g = 0; g < nseg; ++g) {
        double s = 0.0;
        for (int b = 0; b < nb; ++b) s += part[(size_t)g * nb + b];
        total += (double)segs[g].coef * s;
    }
    out[slot] += total;
}

hipError_t launch_reg_loss(const RegSeg* segs_dev, int nseg, int kind, double* part, double* out, int slot,
                           hipStream_t stream) {
    if (nseg <= 0) return hipSuccess;
    hipLaunchKernelGGL(reg_partials_kernel, dim3(64, (unsigned)nseg), dim3(256), 0, stream, segs_dev, kind, part);
    hipLaunchKernelGGL(reg_finalize_kernel, dim3(1), dim3(1), 0, stream, segs_dev, nseg, part, 64, out, slot);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------ K-split convolutions
__global__ void __launch_bounds__(256) split_reduce_kernel(const float* __restrict__ part, int nsplit, size_t stride,
                                                           size_t n, int act, float* __restrict__ dst) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    float s = part[i];
    for (int k = 1; k < nsplit; ++k) s += part[(size_t)k * stride + i];
    dst[i] = act_of(s, act);
}

hipError_t launch_split_reduce(const float* part, int nsplit, size_t stride, size_t n, int act, float* dst,
                               hipStream_t stream) {
    hipLaunchKernelGGL(split_reduce_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, part, nsplit, stride, n,
                       act, dst);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------ optimiser
// Adam as tf.train.AdamOptimizer applies it (reference UnMicst1-5.py:371): m, v slots, lr_t = lr*sqrt(1-b2^t)/(1-b1^t)
// formed on the host, w -= lr_t * m / (sqrt(v) + eps).  Momentum as tf.train.MomentumOptimizer (UnMicst.py:279).
// Positions whose gradient is always zero (BN moving statistics) are left untouched by both rules.
__global__ void __launch_bounds__(256) optimizer_kernel(const OptParams o, float* __restrict__ w,
                                                        const float* __restrict__ g, float* __restrict__ m,
                                                        float* __restrict__ v, size_t n) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float gi = g[i];
    if (o.kind == 0) {
        const float mi = o.beta1 * m[i] + (1.0f - o.beta1) * gi;
        const float vi = o.beta2 * v[i] + (1.0f - o.beta2) * gi * gi;
        m[i] = mi;
        v[i] = vi;
        w[i] = w[i] - o.lr_t * mi / (sqrtf(vi) + o.eps);
    } else {
        const float mi = o.momentum * m[i] + gi;
        m[i] = mi;
        w[i] = w[i] - o.lr * mi;
    }
}

hipError_t launch_optimizer(const OptParams& o, float* w, const float* g, float* m, float* v, size_t n, hipStream_t stream) {
    hipLaunchKernelGGL(optimizer_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, o, w, g, m, v, n);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------ initial state
// tf.global_variables_initializer() of the graph, written into the flat parameter vector (include/umx_train.h, umx_trainer_init;
// == tests/init_ref.py).  A value depends on its tensor's key and its index inside the tensor only: the grid is free.
__device__ __forceinline__ float init_draw(unsigned long long key, unsigned long long e, double sigma) {
    double z = 0.0;   // (every attempt refused: 0)
    for (int a = 0; a < UMX_INIT_MAX_ATTEMPTS; ++a) {
        const unsigned long long c = e * UMX_INIT_MAX_ATTEMPTS + a;
        const double u1 = (double)((mix64(key ^ (2 * c)) >> 11) + 1) * 0x1p-53;
        const double u2 = (double)(mix64(key ^ (2 * c + 1)) >> 11) * 0x1p-53;
        const double r = sqrt(-2.0 * log(u1));
        const double zz = r * cos(UMX_INIT_TWO_PI * u2);
        if (fabs(zz) <= 2.0) { z = zz; break; }
    }
    return (float)(z * sigma);
}

__global__ void __launch_bounds__(256) init_params_kernel(const InitSeg* __restrict__ segs, int nseg, size_t n,
                                                          float* __restrict__ w) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        int lo = 0, hi = nseg - 1;   // the last segment that starts at or before i
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (segs[mid].off <= i) lo = mid; else hi = mid - 1;
        }
        const InitSeg sg = segs[lo];
        const unsigned long long e = i - sg.off;
        float v = 0.f;
        if (e < sg.count) v = sg.kind == INIT_ONE ? 1.f : sg.kind == INIT_FILTER ? init_draw(sg.key, e, sg.sigma) : 0.f;
        w[i] = v;
    }
}

hipError_t launch_init_params(const InitSeg* segs_dev, int nseg, size_t n, float* w, hipStream_t stream) {
    if (nseg < 1 || n == 0) return hipErrorInvalidValue;
    const unsigned blocks = (unsigned)std::min<size_t>((n + 255) / 256, 4096);
    hipLaunchKernelGGL(init_params_kernel, dim3(blocks), dim3(256), 0, stream, segs_dev, nseg, n, w);
    return hipGetLastError();
}

}  // namespace umx
