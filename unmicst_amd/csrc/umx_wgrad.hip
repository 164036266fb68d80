// Weight gradient of a convolution (gfx950 only): three GEMM kernels in 16 instantiations, the planner that fixes a layer's geometry and
// kind of kernel at build (wgrad_setup -> WgradPlan), the one selection that turns a plan and a launch's operands into an instantiation,
// its grid, its LDS bytes and the reduce's scale handling (wgrad_select), the launcher, and the ordered reduce (fixed order, no atomics).
#include "umx_internal.h"

#include <mutex>

#pragma clang fp contract(off)

namespace umx {

typedef float f32x4 __attribute__((ext_vector_type(4)));

// GEMM view: M = input channels of a slab (16*MI per workgroup, MI = 1..3 chosen per layer), N = output channels
// (64 per workgroup, 16 per wave), K = pixels.  A workgroup walks pixel tiles of 128 pixels (imgs x TH x TW) of its
// slice: the X halo tile and the G tile are staged in LDS once and serve every slab (filter tap) of the group --
// 9 taps x MI channel tiles accumulator tiles per wave, one ds_read_b32 per MFMA.  LDS pitches (16 or 48 / 80 floats
// per pixel) put the four pixels of a 16x16x4 fragment on disjoint bank quarters.  Partial sums go to ws[slice];
// wgrad_reduce_kernel adds the slices in order.
constexpr int kWgCO = 64, kWgPG = 80, kWgNS = 9, kWgPix = 128;
__host__ __device__ constexpr int wg_px(int mi) { return mi == 1 ? 16 : 48; }   // X pitch: = 16 or 48 (mod 64)
// halo pixels of one tile: 10 x 18 = 180 (8 x 16 tile, 3 x 3 taps), 2 x 10 x 10 = 200; the 4 x 4 layers (8 images
// x 6 x 6 = 288) use the BIG variants, which exist for MI <= 2 only (register budget of the staging slots)
constexpr int kWgHalo = 208, kWgHaloBig = 288;
__host__ __device__ constexpr int wg_hx(int mi, bool big) { return ((big ? kWgHaloBig : kWgHalo) * 4 * mi + 255) / 256; }

template <int MI, bool BIG>
__global__ void __launch_bounds__(256, 2) wgrad_mfma_f32(const WgradParams p) {
    constexpr int CI = 16 * MI, PX = wg_px(MI);
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* const Xl = smem;                  // [nhalo][PX]
    float* const Gl = smem + p.nhalo * PX;   // [128][kWgPG]
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int kq = lane >> 4, li = lane & 15;
    const int TW = 1 << p.tw_log2, TH = 1 << p.th_log2;

    const int slice = blockIdx.x;
    const int nco = (p.Cg + kWgCO - 1) / kWgCO;
    const int ci0 = (blockIdx.y / nco) * CI, co0 = (blockIdx.y % nco) * kWgCO;
    const int slab0 = p.gstart[blockIdx.z], ns = p.gcount[blockIdx.z];
    const int coff = p.coff[slab0];
    const bool wave_live = co0 + wave * 16 < p.Cg;

    f32x4 acc[kWgNS][MI];
#pragma unroll
    for (int s = 0; s < kWgNS; ++s)
#pragma unroll
        for (int t2 = 0; t2 < MI; ++t2) acc[s][t2] = (f32x4){0.f, 0.f, 0.f, 0.f};

    // register-staged pipeline: the next tile's global loads are issued before the MFMA block of the current tile and
    // written to LDS after it
    constexpr int HX = wg_hx(MI, BIG);
    float4 xr[HX], gr[kWgPix * (kWgCO / 4) / 256];
    const int nx4 = p.nhalo * (CI / 4);
    auto load_tile = [&](int t) {
        const int tx = t % p.tiles_x;
        const int ty = (t / p.tiles_x) % p.tiles_y;
        const int img0 = (t / (p.tiles_x * p.tiles_y)) * p.imgs;
        const int y0 = ty * TH, x0 = tx * TW;
        int tid_o = tid;
        asm volatile("" : "+v"(tid_o));   // opaque per call: keeps the slot decode out of the tile loop's live registers
#pragma unroll
        for (int i = 0; i < HX; ++i) {
            const int e = tid_o + i * 256;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (e < nx4) {
                const int hp = e / (CI / 4), q = e - hp * (CI / 4);
                const int il = hp / p.imgplane;
                const int rr = hp - il * p.imgplane;
                const int hy = rr / p.hw, hx = rr - hy * p.hw;
                const int gy = y0 + p.ymin + hy, gx = x0 + p.xmin + hx, img = img0 + il;
                const int c = ci0 + 4 * q;
                if (img < p.B && gy >= 0 && gy < p.H && gx >= 0 && gx < p.W && c < p.Cx) {
                    const float* src = p.X + ((size_t)(img * p.H + gy) * p.W + gx) * p.Cxt + coff + c;
                    if (p.vecx && c + 3 < p.Cx) v = *reinterpret_cast<const float4*>(src);
                    else {
                        v.x = src[0];
                        if (c + 1 < p.Cx) v.y = src[1];
                        if (c + 2 < p.Cx) v.z = src[2];
                        if (c + 3 < p.Cx) v.w = src[3];
                    }
                }
            }
            xr[i] = v;
        }
#pragma unroll
        for (int i = 0; i < kWgPix * (kWgCO / 4) / 256; ++i) {
            const int e = tid_o + i * 256;
            const int px = e >> 4, q = e & 15;
            const int il = px >> (p.th_log2 + p.tw_log2);
            const int y = (px >> p.tw_log2) & (TH - 1), x = px & (TW - 1);
            const int img = img0 + il;
            const int co = co0 + 4 * q;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (il < p.imgs && img < p.B && co < p.Cg) {   // (tiny layers: fewer images than pixel slots -> zero rows of G)
                const float* src = p.G + ((size_t)(img * p.H + y0 + y) * p.W + x0 + x) * p.Cg + co;
                if (p.vecg && co + 3 < p.Cg) v = *reinterpret_cast<const float4*>(src);
                else {
                    v.x = src[0];
                    if (co + 1 < p.Cg) v.y = src[1];
                    if (co + 2 < p.Cg) v.z = src[2];
                    if (co + 3 < p.Cg) v.w = src[3];
                }
            }
            gr[i] = v;
        }
    };
    auto store_tile = [&]() {
        int tid_o = tid;
        asm volatile("" : "+v"(tid_o));
#pragma unroll
        for (int i = 0; i < HX; ++i) {
            const int e = tid_o + i * 256;
            if (e < nx4) {
                const int hp = e / (CI / 4), q = e - hp * (CI / 4);
                *reinterpret_cast<float4*>(Xl + hp * PX + 4 * q) = xr[i];
            }
        }
#pragma unroll
        for (int i = 0; i < kWgPix * (kWgCO / 4) / 256; ++i) {
            const int e = tid_o + i * 256;
            *reinterpret_cast<float4*>(Gl + (e >> 4) * kWgPG + 4 * (e & 15)) = gr[i];
        }
    };

    int so[kWgNS];   // LDS offset of each slab of the group (wave-uniform)
#pragma unroll
    for (int s = 0; s < kWgNS; ++s) {
        const int sb = slab0 + (s < ns ? s : 0);
        so[s] = __builtin_amdgcn_readfirstlane(((p.dy[sb] - p.ymin) * p.hw + (p.dx[sb] - p.xmin)) * PX);
    }
    const int t_begin = slice * p.tiles_per_slice;
    const int t_end = min(p.ntiles, (slice + 1) * p.tiles_per_slice);
    if (t_begin < t_end) load_tile(t_begin);
    for (int t = t_begin; t < t_end; ++t) {
        __syncthreads();   // the previous tile's fragment reads are done
        store_tile();
        __syncthreads();
        if (t + 1 < t_end) load_tile(t + 1);
        if (wave_live) {
            for (int ks = 0; ks < kWgPix / 4; ++ks) {
                const int px = 4 * ks + kq;
                const int il = min(px >> (p.th_log2 + p.tw_log2), p.imgs - 1);   // unused slots: any finite X (their G is 0)
                const int y = (px >> p.tw_log2) & (TH - 1), x = px & (TW - 1);
                const float* ap = Xl + (il * p.imgplane + y * p.hw + x) * PX + li;
                const float b = Gl[px * kWgPG + wave * 16 + li];
                float a[kWgNS][MI];
#pragma unroll
                for (int s = 0; s < kWgNS; ++s)
                    if (s < ns) {
#pragma unroll
                        for (int t2 = 0; t2 < MI; ++t2) a[s][t2] = ap[so[s] + 16 * t2];
                    }
#pragma unroll
                for (int s = 0; s < kWgNS; ++s)
                    if (s < ns) {
#pragma unroll
                        for (int t2 = 0; t2 < MI; ++t2)
                            acc[s][t2] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[s][t2], b, acc[s][t2], 0, 0, 0);
                    }
            }
        }
    }

    // D tile: row (input channel) = 4*kq + r, column (output channel) = li
    const size_t slab_sz = (size_t)p.Cx * p.Cg;
    const int co = co0 + wave * 16 + li;
#pragma unroll
    for (int s = 0; s < kWgNS; ++s) {
        if (s < ns && co < p.Cg) {
            float* dst = p.ws + ((size_t)slice * p.nslab + slab0 + s) * slab_sz;
#pragma unroll
            for (int t2 = 0; t2 < MI; ++t2)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int ci = ci0 + t2 * 16 + 4 * kq + r;
                    if (ci < p.Cx) dst[(size_t)ci * p.Cg + co] = acc[s][t2][r];
                }
        }
    }
}


// ------------------------------------------------------------------------------------------------ weight gradient, thin X
// The first layer (and the v2 graph's top skip connection) has 1 - 4 input channels: a 16-channel MFMA tile is 6 - 25 % full and
// the 128-pixel tiles of the kernel above spend their time staging (165 - 277 us for 2 x 36 channels at 8 x 256 x 256, the last
// kernel of the backward pass with nothing left to hide behind).  Here the GEMM runs on the vector ALUs: a workgroup owns `thin`
// whole image rows, stages their X halo (a few KB) in LDS, and thread (output channel co, pixel group pg) walks the strip's
// pixels pg, pg + PG, ... with one coalesced load of G (four output channels) per pixel and nslab * CX broadcast LDS reads.  The PG
// partial sums are added in a fixed order; the slices by wgrad_reduce_kernel as before (same ws layout).
template <int CX, int V>   // V output channels per thread: 4 (Cg % 4 == 0: 16-byte loads of G) or 1
__global__ void __launch_bounds__(256) wgrad_thin_kernel(const WgradParams p) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int tid = threadIdx.x;
    const int R = p.thin, hw = p.hw, hh = p.hh;
    const int slice = blockIdx.x;
    const int row0 = slice * R;                       // global row = img * H + y; R divides H: a strip stays inside one image
    const int img = row0 / p.H, y0 = row0 - img * p.H;
    const int ns = p.gcount[0];
    const int coff = p.coff[0];
    float* const Xl = smem;                            // [hh][hw][CX]
    float* const red = smem + ((hh * hw * CX + 3) & ~3);   // [ceil(PG / 4)][ns * CX][Cg]
    for (int e = tid; e < hh * hw; e += 256) {
        const int hy = e / hw, hx = e - hy * hw;
        const int gy = y0 + p.ymin + hy, gx = p.xmin + hx;
        const bool in = gy >= 0 && gy < p.H && gx >= 0 && gx < p.W;
        const float* src = p.X + ((size_t)(img * p.H + (in ? gy : 0)) * p.W + (in ? gx : 0)) * p.Cxt + coff;
#pragma unroll
        for (int c = 0; c < CX; ++c) Xl[e * CX + c] = in ? src[c] : 0.f;
    }
    int so[kWgNS];
#pragma unroll
    for (int s = 0; s < kWgNS; ++s) {
        const int sb = s < ns ? s : 0;
        so[s] = __builtin_amdgcn_readfirstlane(((p.dy[sb] - p.ymin) * hw + (p.dx[sb] - p.xmin)) * CX);
    }
    __syncthreads();
    const int Cg = p.Cg, Q = Cg / V, PG = 256 / Q;
    const int pg = tid / Q, co = (tid - pg * Q) * V;
    float acc[kWgNS][CX][V];
#pragma unroll
    for (int s = 0; s < kWgNS; ++s)
#pragma unroll
        for (int c = 0; c < CX; ++c)
#pragma unroll
            for (int v = 0; v < V; ++v) acc[s][c][v] = 0.f;
    const int nout = ns * CX * Cg;                     // (s, ci, co) in the order of the ws slab: [slab][Cx][Cg]
    {   // branch-free: every thread walks ceil(npx / PG) pixels, a pixel past the strip is clamped and its G taken as zero (the four
        // threads past the last pixel group do the same and drop their sums) -- the compiler keeps two loads of G in flight
        const int npx = R * p.W;
        const int wl = 31 - __builtin_clz(p.W);      // W is a power of two (wgrad_setup)
        const float* const G = p.G + (size_t)row0 * p.W * Cg + co;
        auto load_g = [&](int px, float* g) {
            const int pc = min(px, npx - 1);
            if constexpr (V == 4) {
                const float4 g4 = *reinterpret_cast<const float4*>(G + (size_t)pc * Cg);
                g[0] = g4.x; g[1] = g4.y; g[2] = g4.z; g[3] = g4.w;
            } else {
                g[0] = G[(size_t)pc * Cg];
            }
        };
        auto step = [&](int px, const float* gin) {
            const bool live = px < npx;
            const int pc = min(px, npx - 1);
            float g[V];
#pragma unroll
            for (int v = 0; v < V; ++v) g[v] = live ? gin[v] : 0.f;
            const int y = pc >> wl, x = pc & (p.W - 1);
            const float* const xp = Xl + (y * hw + x) * CX;
            float xv[kWgNS][CX];   // (all kWgNS slabs: a slab past ns re-reads slab 0 and its sums are dropped)
#pragma unroll
            for (int s = 0; s < kWgNS; ++s)
#pragma unroll
                for (int c = 0; c < CX; ++c) xv[s][c] = xp[so[s] + c];
#pragma unroll
            for (int s = 0; s < kWgNS; ++s)
#pragma unroll
                for (int c = 0; c < CX; ++c)
#pragma unroll
                    for (int v = 0; v < V; ++v) acc[s][c][v] = __builtin_fmaf(xv[s][c], g[v], acc[s][c][v]);
        };
        const int niter = (npx + PG - 1) / PG;
        int ahead = 2 * PG;   // (opaque: hipcc otherwise proves the prefetch is the next iteration's own load and sinks it back there)
        asm volatile("" : "+s"(ahead));
        float ga[V], gb[V];
        load_g(pg, ga);
        load_g(pg + PG, gb);
        for (int i = 0; i < niter; i += 2) {
            const int px = pg + i * PG;
            float g0[V], g1[V];
#pragma unroll
            for (int v = 0; v < V; ++v) { g0[v] = ga[v]; g1[v] = gb[v]; }
            load_g(px + ahead, ga);
            load_g(px + ahead + PG, gb);
            step(px, g0);
            step(px + PG, g1);
        }
    }
    // the PG partial sums, in a fixed order and through S = ceil(PG / 4) LDS slots (a slot per group would cost 36 KB for 36 output
    // channels and leave a CU three workgroups, one short of the 1024-workgroup launch fitting in one round): the top m = min(S, n - S)
    // groups are folded into the bottom m until S are left, and those are added in group order
    const int S = (PG + 3) / 4;
    auto slot = [&](int g, int s, int c, int v) { return (size_t)g * nout + (size_t)(s * CX + c) * Cg + co + v; };
    int n = PG;
    while (n > S) {
        const int m = min(S, n - S);
        if (pg >= n - m && pg < n) {
#pragma unroll
            for (int s = 0; s < kWgNS; ++s)
                if (s < ns) {
#pragma unroll
                    for (int c = 0; c < CX; ++c)
#pragma unroll
                        for (int v = 0; v < V; ++v) red[slot(pg - (n - m), s, c, v)] = acc[s][c][v];
                }
        }
        __syncthreads();
        if (pg < m) {
#pragma unroll
            for (int s = 0; s < kWgNS; ++s)
                if (s < ns) {
#pragma unroll
                    for (int c = 0; c < CX; ++c)
#pragma unroll
                        for (int v = 0; v < V; ++v) acc[s][c][v] += red[slot(pg, s, c, v)];
                }
        }
        __syncthreads();
        n -= m;
    }
    if (pg < n) {
#pragma unroll
        for (int s = 0; s < kWgNS; ++s)
            if (s < ns) {
#pragma unroll
                for (int c = 0; c < CX; ++c)
#pragma unroll
                    for (int v = 0; v < V; ++v) red[slot(pg, s, c, v)] = acc[s][c][v];
            }
    }
    __syncthreads();
    float* const dst = p.ws + (size_t)slice * p.nslab * CX * Cg;
    for (int e = tid; e < nout; e += 256) {
        float t = red[e];
        for (int j = 1; j < n; ++j) t += red[(size_t)j * nout + e];
        dst[e] = t;
    }
}

static int wgrad_thin_v(const WgradPlan& p) { return p.Cg % 4 == 0 ? 4 : 1; }
static size_t wgrad_thin_lds(const WgradPlan& p) {
    const int V = wgrad_thin_v(p), PG = 256 / (p.Cg / V);
    return sizeof(float) * ((size_t)((p.hh * p.hw * p.Cx + 3) & ~3) + (size_t)((PG + 3) / 4) * p.gcount[0] * p.Cx * p.Cg);
}

// ------------------------------------------------------------------------------------------------ weight gradient, f16x3
// The same GEMM on the binary16 matrix cores with fp32-equivalent products: x*g = xh*gh + xh*gl + xl*gh, (hi, lo) exact
// binary16 pairs, fp32 accumulation (the scheme of conv_f16x3).  One v_mfma_f32_16x16x32_f16 covers
// 32 pixels of K where the fp32 MFMA covers 4: 3 x 16 cycles instead of 8 x 32.
//   * Operands are converted while they are staged: fp32 NHWC from HBM -> scaled -> (hi, lo) -> channel-planar LDS
//     [plane][channel][pixel] (a fragment = 8 consecutive pixels of one channel = one ds_read_b128).  Every operand is
//     scaled by the power of two that brings its tracked max |v| (written by its producer) to [2^11, 2^12): gradients
//     would flush to zero in binary16 otherwise, and activations keep their lo parts normal; the reduce kernel divides
//     the product of the two scales out.
//   * A tap shifts the X window by dx pixels = dx halves: the fragment is read as an aligned b128 + b32 and funnel-
//     shifted (v_alignbit) -- no per-tap copies of the halo.
//   * 48 x 48 channel tiles (the 36*2^k and 80*2^k widths of the shipped models pad to multiples of 48 with <= 1.33x):
//     the 9 taps x 3 channel tiles = 27 (tap, tile) pairs are dealt 7/7/7/6 to the four waves, each wave against all
//     three output-channel tiles, so every X fragment is read once per workgroup and every wave is busy.
typedef _Float16 h8v __attribute__((ext_vector_type(8)));
constexpr int kHwC = 48, kHwPW = 7, kHwXT = 5, kHwGT = 3;
constexpr int kOX = 3, kOG = 2;                          // octet tasks per thread: 256 * 3 >= imgs * hh * prow * 6, 256 * 2 >= 64 * 6

__device__ __forceinline__ float wg_scale(const unsigned* mx) {
    const int e = (int)((*mx >> 23) & 0xff);          // biased exponent of the tensor's tracked max |v|
    if (e == 0 || e == 255) return 1.f;
    const int se = min(max(127 + 11 - (e - 127), 1), 254);
    return __uint_as_float((unsigned)se << 23);        // max * scale in [2^11, 2^12)
}

__device__ __forceinline__ unsigned pack_h2(_Float16 a, _Float16 b) {
    return (unsigned)__builtin_bit_cast(unsigned short, a) | ((unsigned)__builtin_bit_cast(unsigned short, b) << 16);
}

// PL = true (round 4): the operands are staged from the (hi, lo) binary16 NHWC planes their producers already wrote for conv_f16x3
// (WgradParams::Xhi ..): half the bytes, no conversion, and a staging task is 16 bit operations instead of ~56 conversions and
// subtractions.  X planes are unscaled, G planes carry the power of two of their tensor (undone by the reduce through *ginv).
// OC (with PL): a staging task is (pixel pair, channel OCTET) with octets fastest over the lanes -- 16-byte loads, six lanes on one
// pixel's 96 contiguous bytes -- instead of (pixel pair, channel quad) with pixel pairs fastest, whose 8-byte loads put every lane of
// an instruction on a cache line of its own (timing ablation, profiles/r04/train_wgrad_ablation.txt: this kernel's global loads are
// 30 % of its time and slow the main stream's memory-bound kernels by 7 - 25 %).  Needs 16-byte aligned octets: channel offsets
// and stored channel counts that are multiples of 8.
template <bool PL, bool OC = false>
__global__ void __launch_bounds__(256, 2) wgrad_f16x3(const WgradParams p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_b[];
    _Float16* const Xh = reinterpret_cast<_Float16*>(smem_b);   // [2][48][xs]
    _Float16* const Gh = Xh + 2 * kHwC * p.xs;                  // [2][48][gs]
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int kq = lane >> 4, li = lane & 15;
    const int TW = 1 << p.tw_log2, TH = 1 << p.th_log2;
    const int imgplaneP = p.hh * p.hp;

    const int slice = blockIdx.x;
    const int nco = (p.Cg + kHwC - 1) / kHwC;
    const int ci0 = (blockIdx.y / nco) * kHwC, co0 = (blockIdx.y % nco) * kHwC;
    const int slab0 = p.gstart[blockIdx.z], ns = p.gcount[blockIdx.z];
    const int coff = p.coff[slab0];
    const float sx = PL ? 1.f : wg_scale(p.xmax), sg = PL ? 1.f : wg_scale(p.gmax);

    // this wave's (slab, channel tile) pairs
    // (pairs dealt evenly: a transposed convolution's parity groups have 1 - 4 slabs = 3 - 12 pairs, and seven per wave in wave order
    //  left two or three of the four waves without work)
    const int npairs = ns * 3;
    const int ppw = __builtin_amdgcn_readfirstlane((npairs + 3) >> 2), pair0 = wave * ppw, pair1 = min(npairs, pair0 + ppw);
    int aoff[kHwPW], dxs[kHwPW], sbi[kHwPW], t2i[kHwPW];
#pragma unroll
    for (int i = 0; i < kHwPW; ++i) {
        const int id = min(pair0 + i, npairs - 1);
        const int sb = id / 3, t2 = id - sb * 3;
        sbi[i] = __builtin_amdgcn_readfirstlane(sb);
        t2i[i] = __builtin_amdgcn_readfirstlane(t2);
        aoff[i] = __builtin_amdgcn_readfirstlane(t2 * 16 * p.xs + (p.dy[slab0 + sb] - p.ymin) * p.hp);
        dxs[i] = __builtin_amdgcn_readfirstlane(p.dx[slab0 + sb] - p.xmin);
    }
    f32x4 acc[kHwPW][3];
#pragma unroll
    for (int i = 0; i < kHwPW; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};

    const int prow = (p.hw + 1) >> 1;                       // pixel pairs per halo row
    const int nxt = p.imgs * p.hh * prow * (kHwC / 4);      // X staging tasks: (halo row, pixel pair, channel quad)
    // e / prow and r / hh by reciprocal multiplication (e < kHwXT * 256 = 1280, divisors < 32: exact) -- three runtime integer
    // divisions per staging task, twice per tile, were ~35 instructions each
    const unsigned inv_prow = 65536u / (unsigned)prow + 1u, inv_hh = 65536u / (unsigned)p.hh + 1u;
    float4 xr[OC ? 1 : kHwXT][2], gr[OC ? 1 : kHwGT][2];
    uint4 xo[OC ? kOX : 1][4], go[OC ? kOG : 1][4];          // [task][px0 hi, px1 hi, px0 lo, px1 lo]
    const int nxo = p.imgs * p.hh * prow * 6;
    auto load_tile = [&](int t) {
        const int tx = t % p.tiles_x;
        const int ty = (t / p.tiles_x) % p.tiles_y;
        const int img0 = (t / (p.tiles_x * p.tiles_y)) * p.imgs;
        const int y0 = ty * TH, x0 = tx * TW;
        int tid_o = tid;
        asm volatile("" : "+v"(tid_o));
        if constexpr (OC) {
            const uint4 z4 = make_uint4(0u, 0u, 0u, 0u);
#pragma unroll
            for (int i = 0; i < kOX; ++i) {
                const int e = tid_o + i * 256;
                xo[i][0] = xo[i][1] = xo[i][2] = xo[i][3] = z4;
                if (e < nxo) {
                    const int e2 = (int)(((unsigned)e * 10923u) >> 16);   // e / 6 (e < 768: exact)
                    const int o = e - e2 * 6;
                    int r = (int)(((unsigned)e2 * inv_prow) >> 16);
                    const int pr = e2 - r * prow;
                    const int il = (int)(((unsigned)r * inv_hh) >> 16), hy = r - il * p.hh;
                    const int gy = y0 + p.ymin + hy, gx = x0 + p.xmin + 2 * pr, img = img0 + il;
                    const int c = ci0 + 8 * o;
                    if (img < p.B && gy >= 0 && gy < p.H && c < p.Cx) {
                        const size_t row = ((size_t)(img * p.H + gy) * p.W) * p.XCs + coff + c;
#pragma unroll
                        for (int h = 0; h < 2; ++h) {
                            const int gxx = gx + h;
                            if (gxx >= 0 && gxx < p.W && 2 * pr + h < p.hw) {
                                xo[i][h] = *reinterpret_cast<const uint4*>(p.Xhi + row + (size_t)gxx * p.XCs);
                                xo[i][2 + h] = *reinterpret_cast<const uint4*>(p.Xlo + row + (size_t)gxx * p.XCs);
                            }
                        }
                    }
                }
            }
#pragma unroll
            for (int i = 0; i < kOG; ++i) {
                const int e = tid_o + i * 256;              // 64 pixel pairs x 6 channel octets = 384 tasks
                go[i][0] = go[i][1] = go[i][2] = go[i][3] = z4;
                const int pp = (int)(((unsigned)e * 10923u) >> 16), o = e - pp * 6;
                const int px = 2 * pp;
                const int il = px >> (p.th_log2 + p.tw_log2);
                const int y = (px >> p.tw_log2) & (TH - 1), x = px & (TW - 1);
                const int img = img0 + il;
                const int co = co0 + 8 * o;
                if (pp < 64 && img < p.B && co < p.Cg) {
                    const size_t at = ((size_t)(img * p.H + y0 + y) * p.W + x0 + x) * p.GCs + co;
#pragma unroll
                    for (int h = 0; h < 2; ++h) {
                        go[i][h] = *reinterpret_cast<const uint4*>(p.Ghi + at + (size_t)h * p.GCs);
                        go[i][2 + h] = *reinterpret_cast<const uint4*>(p.Glo + at + (size_t)h * p.GCs);
                    }
                }
            }
            return;
        }
#pragma unroll
        for (int i = 0; i < kHwXT; ++i) {
            const int e = tid_o + i * 256;
            float4 v0 = make_float4(0.f, 0.f, 0.f, 0.f), v1 = v0;
            if (e < nxt) {
                int r = (int)(((unsigned)e * inv_prow) >> 16);
                const int pr = e - r * prow;                  // pixel pair fastest: conflict-free LDS stores
                const int q = r % (kHwC / 4); r /= (kHwC / 4);
                const int il = (int)(((unsigned)r * inv_hh) >> 16), hy = r - il * p.hh;
                const int gy = y0 + p.ymin + hy, gx = x0 + p.xmin + 2 * pr, img = img0 + il;
                const int c = ci0 + 4 * q;
                if (PL && img < p.B && gy >= 0 && gy < p.H && c < p.Cx) {
                    // (planes: 4 halves of hi and of lo per pixel -- the pad channels of a tensor's last octet are zeros)
                    const size_t row = ((size_t)(img * p.H + gy) * p.W) * p.XCs + coff + c;
#pragma unroll
                    for (int h = 0; h < 2; ++h) {
                        const int gxx = gx + h;
                        if (gxx >= 0 && gxx < p.W && 2 * pr + h < p.hw) {
                            const uint2 vh = *reinterpret_cast<const uint2*>(p.Xhi + row + (size_t)gxx * p.XCs);
                            const uint2 vl = *reinterpret_cast<const uint2*>(p.Xlo + row + (size_t)gxx * p.XCs);
                            const float4 v = make_float4(__uint_as_float(vh.x), __uint_as_float(vh.y), __uint_as_float(vl.x),
                                                         __uint_as_float(vl.y));
                            if (h == 0) v0 = v; else v1 = v;
                        }
                    }
                } else if (!PL && img < p.B && gy >= 0 && gy < p.H && c < p.Cx) {
                    const float* row = p.X + ((size_t)(img * p.H + gy) * p.W) * p.Cxt + coff + c;
#pragma unroll
                    for (int h = 0; h < 2; ++h) {
                        const int gxx = gx + h;
                        if (gxx >= 0 && gxx < p.W && 2 * pr + h < p.hw) {
                            const float* src = row + (size_t)gxx * p.Cxt;
                            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
                            if (p.vecx && c + 3 < p.Cx) v = *reinterpret_cast<const float4*>(src);
                            else {
                                v.x = src[0];
                                if (c + 1 < p.Cx) v.y = src[1];
                                if (c + 2 < p.Cx) v.z = src[2];
                                if (c + 3 < p.Cx) v.w = src[3];
                            }
                            if (h == 0) v0 = v; else v1 = v;
                        }
                    }
                }
            }
            xr[i][0] = v0;
            xr[i][1] = v1;
        }
#pragma unroll
        for (int i = 0; i < kHwGT; ++i) {
            const int e = tid_o + i * 256;              // 64 pixel pairs x 12 channel quads = 768 tasks
            const int pp = e & 63, q = e >> 6;
            const int px = 2 * pp;
            const int il = px >> (p.th_log2 + p.tw_log2);
            const int y = (px >> p.tw_log2) & (TH - 1), x = px & (TW - 1);
            const int img = img0 + il;
            const int co = co0 + 4 * q;
            float4 v0 = make_float4(0.f, 0.f, 0.f, 0.f), v1 = v0;
            if (PL && img < p.B && co < p.Cg) {
                const size_t at = ((size_t)(img * p.H + y0 + y) * p.W + x0 + x) * p.GCs + co;
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    const uint2 vh = *reinterpret_cast<const uint2*>(p.Ghi + at + (size_t)h * p.GCs);
                    const uint2 vl = *reinterpret_cast<const uint2*>(p.Glo + at + (size_t)h * p.GCs);
                    const float4 v = make_float4(__uint_as_float(vh.x), __uint_as_float(vh.y), __uint_as_float(vl.x), __uint_as_float(vl.y));
                    if (h == 0) v0 = v; else v1 = v;
                }
            } else if (!PL && img < p.B && co < p.Cg) {
                const float* src = p.G + ((size_t)(img * p.H + y0 + y) * p.W + x0 + x) * p.Cg + co;
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    const float* s2 = src + (size_t)h * p.Cg;
                    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
                    if (p.vecg && co + 3 < p.Cg) v = *reinterpret_cast<const float4*>(s2);
                    else {
                        v.x = s2[0];
                        if (co + 1 < p.Cg) v.y = s2[1];
                        if (co + 2 < p.Cg) v.z = s2[2];
                        if (co + 3 < p.Cg) v.w = s2[3];
                    }
                    if (h == 0) v0 = v; else v1 = v;
                }
            }
            gr[i][0] = v0;
            gr[i][1] = v1;
        }
    };
    auto split_store = [&](_Float16* base, int plane_stride, int chan_stride, int pos, float4 a, float4 b, float sc) {
        if constexpr (PL) {
            // a, b = pixels 2 pr and 2 pr + 1: {hi(c0, c1), hi(c2, c3), lo(c0, c1), lo(c2, c3)} as bit patterns; the LDS image wants, per
            // channel, the pixel pair in one word
            const unsigned ah0 = __float_as_uint(a.x), ah1 = __float_as_uint(a.y), al0 = __float_as_uint(a.z), al1 = __float_as_uint(a.w);
            const unsigned bh0 = __float_as_uint(b.x), bh1 = __float_as_uint(b.y), bl0 = __float_as_uint(b.z), bl1 = __float_as_uint(b.w);
            const unsigned hw[4] = {(ah0 & 0xffffu) | (bh0 << 16), (ah0 >> 16) | (bh0 & 0xffff0000u), (ah1 & 0xffffu) | (bh1 << 16),
                                    (ah1 >> 16) | (bh1 & 0xffff0000u)};
            const unsigned lw[4] = {(al0 & 0xffffu) | (bl0 << 16), (al0 >> 16) | (bl0 & 0xffff0000u), (al1 & 0xffffu) | (bl1 << 16),
                                    (al1 >> 16) | (bl1 & 0xffff0000u)};
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                *reinterpret_cast<unsigned*>(base + k * chan_stride + pos) = hw[k];
                *reinterpret_cast<unsigned*>(base + plane_stride + k * chan_stride + pos) = lw[k];
            }
            return;
        }
        const float va[4] = {a.x * sc, a.y * sc, a.z * sc, a.w * sc};
        const float vb[4] = {b.x * sc, b.y * sc, b.z * sc, b.w * sc};
        float big = 0.f;
#pragma unroll
        for (int k = 0; k < 4; ++k) big = fmaxf(big, fmaxf(fabsf(va[k]), fabsf(vb[k])));
        if (!(big < 6.0e4f)) atomicOr(p.overflow, 1);   // also catches NaN
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const _Float16 ha = (_Float16)va[k], hb = (_Float16)vb[k];
            const _Float16 la = (_Float16)(va[k] - (float)ha), lb = (_Float16)(vb[k] - (float)hb);
            *reinterpret_cast<unsigned*>(base + k * chan_stride + pos) = pack_h2(ha, hb);
            *reinterpret_cast<unsigned*>(base + plane_stride + k * chan_stride + pos) = pack_h2(la, lb);
        }
    };
    // an octet task's two pixels -> per channel one word (the pixel pair), hi and lo planes
    auto store_octet = [&](_Float16* base, int plane_stride, int chan_stride, int pos, const uint4 (&v)[4]) {
        const unsigned a[4] = {v[0].x, v[0].y, v[0].z, v[0].w}, b[4] = {v[1].x, v[1].y, v[1].z, v[1].w};
        const unsigned c[4] = {v[2].x, v[2].y, v[2].z, v[2].w}, d[4] = {v[3].x, v[3].y, v[3].z, v[3].w};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            *reinterpret_cast<unsigned*>(base + (2 * j) * chan_stride + pos) = (a[j] & 0xffffu) | (b[j] << 16);
            *reinterpret_cast<unsigned*>(base + (2 * j + 1) * chan_stride + pos) = (a[j] >> 16) | (b[j] & 0xffff0000u);
            *reinterpret_cast<unsigned*>(base + plane_stride + (2 * j) * chan_stride + pos) = (c[j] & 0xffffu) | (d[j] << 16);
            *reinterpret_cast<unsigned*>(base + plane_stride + (2 * j + 1) * chan_stride + pos) = (c[j] >> 16) | (d[j] & 0xffff0000u);
        }
    };
    auto store_tile = [&]() {
        int tid_o = tid;
        asm volatile("" : "+v"(tid_o));
        if constexpr (OC) {
#pragma unroll
            for (int i = 0; i < kOX; ++i) {
                const int e = tid_o + i * 256;
                if (e < nxo) {
                    const int e2 = (int)(((unsigned)e * 10923u) >> 16);
                    const int o = e - e2 * 6;
                    const int r = (int)(((unsigned)e2 * inv_prow) >> 16);   // = il * hh + hy
                    const int pr = e2 - r * prow;
                    store_octet(Xh + (8 * o) * p.xs, kHwC * p.xs, p.xs, r * p.hp + 2 * pr, xo[i]);
                }
            }
#pragma unroll
            for (int i = 0; i < kOG; ++i) {
                const int e = tid_o + i * 256;
                const int pp = (int)(((unsigned)e * 10923u) >> 16), o = e - pp * 6;
                if (pp < 64) store_octet(Gh + (8 * o) * p.gs, kHwC * p.gs, p.gs, 2 * pp, go[i]);
            }
            return;
        }
#pragma unroll
        for (int i = 0; i < kHwXT; ++i) {
            const int e = tid_o + i * 256;
            if (e < nxt) {
                int r = (int)(((unsigned)e * inv_prow) >> 16);
                const int pr = e - r * prow;
                const int q = r % (kHwC / 4); r /= (kHwC / 4);   // r = il * hh + hy
                split_store(Xh + (4 * q) * p.xs, kHwC * p.xs, p.xs, r * p.hp + 2 * pr, xr[i][0], xr[i][1], sx);
            }
        }
#pragma unroll
        for (int i = 0; i < kHwGT; ++i) {
            const int e = tid_o + i * 256;
            const int pp = e & 63, q = e >> 6;
            split_store(Gh + (4 * q) * p.gs, kHwC * p.gs, p.gs, 2 * pp, gr[i][0], gr[i][1], sg);
        }
    };

    const bool live1 = co0 + 16 < p.Cg, live2 = co0 + 32 < p.Cg;
    const int t_begin = slice * p.tiles_per_slice;
    const int t_end = min(p.ntiles, (slice + 1) * p.tiles_per_slice);
    if (t_begin < t_end) load_tile(t_begin);
    for (int t = t_begin; t < t_end; ++t) {
        __syncthreads();
        store_tile();
        __syncthreads();
        if (t + 1 < t_end) load_tile(t + 1);
        // (not unrolled: the four k-steps of a tile unrolled cost 54 more registers and 10 scratch spills inside this loop -- found by a
        // timing ablation whose run-time loop bound kept hipcc from unrolling: backward pass 4.35 -> 4.08 ms)
#pragma unroll 1
        for (int ks = 0; ks < kWgPix / 32; ++ks) {
            const int p0 = 32 * ks + 8 * kq;
            const int il = p0 >> (p.th_log2 + p.tw_log2);
            const int y = (p0 >> p.tw_log2) & (TH - 1), x = p0 & (TW - 1);
            const _Float16* const gp = Gh + li * p.gs + p0;
            h8v gh[3], gl[3];
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                gh[j] = *reinterpret_cast<const h8v*>(gp + j * 16 * p.gs);
                gl[j] = *reinterpret_cast<const h8v*>(gp + (kHwC + j * 16) * p.gs);
            }
            const _Float16* const xp = Xh + li * p.xs + il * imgplaneP + y * p.hp + x;
#pragma unroll
            for (int i = 0; i < kHwPW; ++i) {
                if (pair0 + i < pair1) {
                    h8v xf[2];
#pragma unroll
                    for (int pl = 0; pl < 2; ++pl) {
                        const _Float16* a = xp + aoff[i] + pl * kHwC * p.xs;
                        const uint4 d = *reinterpret_cast<const uint4*>(a);
                        const unsigned d4 = *reinterpret_cast<const unsigned*>(a + 8);
                        uint4 f;
                        if (dxs[i] == 0) f = d;
                        else if (dxs[i] == 1) {
                            f.x = __builtin_amdgcn_alignbit(d.y, d.x, 16);
                            f.y = __builtin_amdgcn_alignbit(d.z, d.y, 16);
                            f.z = __builtin_amdgcn_alignbit(d.w, d.z, 16);
                            f.w = __builtin_amdgcn_alignbit(d4, d.w, 16);
                        } else f = make_uint4(d.y, d.z, d.w, d4);
                        xf[pl] = __builtin_bit_cast(h8v, f);
                    }
#pragma unroll
                    for (int j = 0; j < 3; ++j) {
                        if (j == 0 || (j == 1 && live1) || (j == 2 && live2)) {
                            f32x4 c = acc[i][j];
                            c = __builtin_amdgcn_mfma_f32_16x16x32_f16(xf[0], gl[j], c, 0, 0, 0);
                            c = __builtin_amdgcn_mfma_f32_16x16x32_f16(xf[1], gh[j], c, 0, 0, 0);
                            acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(xf[0], gh[j], c, 0, 0, 0);
                        }
                    }
                }
            }
        }
    }

    const size_t slab_sz = (size_t)p.Cx * p.Cg;
#pragma unroll
    for (int i = 0; i < kHwPW; ++i) {
        if (pair0 + i < pair1) {
            float* dst = p.ws + ((size_t)slice * p.nslab + slab0 + sbi[i]) * slab_sz;
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                const int co = co0 + j * 16 + li;
                if (co < p.Cg) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int ci = ci0 + t2i[i] * 16 + 4 * kq + r;
                        if (ci < p.Cx) dst[(size_t)ci * p.Cg + co] = acc[i][j][r];
                    }
                }
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------ plan, selection, launch
// dynamic LDS of the three kernels (wgrad_thin_lds is above, beside its kernel) and what a workgroup may ask for
static size_t wgrad_f16_lds(const WgradPlan& p) { return sizeof(_Float16) * 2 * kHwC * ((size_t)p.xs + p.gs); }
static size_t wgrad_f32_lds(const WgradPlan& p) { return sizeof(float) * ((size_t)p.nhalo * wg_px(p.mi) + (size_t)kWgPix * kWgPG); }
static size_t wgrad_lds(const WgradPlan& p) { return p.thin > 0 ? wgrad_thin_lds(p) : p.f16 ? wgrad_f16_lds(p) : wgrad_f32_lds(p); }
constexpr size_t kWgMaxLds = 160 * 1024, kWgThinMaxLds = 64 * 1024;

// channel chunks of a launch: (input-channel tiles) x (output-channel tiles) of the plan's kernel; a thin workgroup owns every channel
static int wgrad_chunks(const WgradPlan& p) {
    if (p.thin > 0) return 1;
    const int ci = p.f16 ? kHwC : 16 * p.mi, co = p.f16 ? kHwC : kWgCO;
    return ((p.Cx + ci - 1) / ci) * ((p.Cg + co - 1) / co);
}

WgGrid wgrad_grid(const WgradPlan& p) { return {(unsigned)p.nslices, (unsigned)wgrad_chunks(p), (unsigned)p.ngroups}; }

bool wgrad_setup(WgradPlan* p, bool f32_route, std::string* why) {
    auto lg2 = [](int v) { int l = 0; while ((1 << l) < v) ++l; return l; };
    if (p->nslab < 1 || p->nslab > kWgMaxSlabs) { *why = "wgrad: too many filter taps"; return false; }
    p->vecx = (p->Cxt % 4 == 0);
    for (int s = 0; s < p->nslab; ++s)
        if (p->coff[s] % 4) p->vecx = 0;
    p->vecg = (p->Cg % 4 == 0);
    const int TW = std::min(16, p->W), TH = std::min(8, p->H);
    if ((TW & (TW - 1)) || (TH & (TH - 1)) || p->H % TH || p->W % TW || kWgPix % (TH * TW)) {
        *why = "wgrad: layer size must be a power of two";
        return false;
    }
    p->tw_log2 = lg2(TW);
    p->th_log2 = lg2(TH);
    p->imgs = kWgPix / (TH * TW);
    int ymin = 0, ymax = 0, xmin = 0, xmax = 0;
    for (int s = 0; s < p->nslab; ++s) {
        ymin = std::min<int>(ymin, p->dy[s]); ymax = std::max<int>(ymax, p->dy[s]);
        xmin = std::min<int>(xmin, p->dx[s]); xmax = std::max<int>(xmax, p->dx[s]);
    }
    p->ymin = ymin;
    p->xmin = xmin;
    p->hh = TH + ymax - ymin;
    p->hw = TW + xmax - xmin;
    p->imgplane = p->hh * p->hw;
    // tiny layers (2x2, 4x4): 128 pixel slots would span dozens of images and their halos; use as many images as the
    // staging budget holds and leave the other slots empty (their rows of G are staged as zeros)
    p->imgs = std::max(1, std::min(p->imgs, kWgHaloBig / p->imgplane));
    p->nhalo = p->imgs * p->imgplane;
    p->tiles_y = p->H / TH;
    p->tiles_x = p->W / TW;
    p->ntiles = ((p->B + p->imgs - 1) / p->imgs) * p->tiles_y * p->tiles_x;
    // slab groups: runs of <= 9 consecutive slabs with one channel offset
    p->ngroups = 0;
    for (int s = 0; s < p->nslab;) {
        int n = 1;
        while (s + n < p->nslab && n < kWgNS && p->coff[s + n] == p->coff[s]) ++n;
        p->gstart[p->ngroups] = (short)s;
        p->gcount[p->ngroups] = (short)n;
        ++p->ngroups;
        s += n;
    }
    // the tiles dealt to about `target` workgroups a launch, given the plan's kind of kernel
    auto slice = [p](int target) {
        const int nslices = std::max(1, std::min(p->ntiles, target / std::max(1, wgrad_chunks(*p) * p->ngroups)));
        p->tiles_per_slice = (p->ntiles + nslices - 1) / nslices;
        p->nslices = (p->ntiles + p->tiles_per_slice - 1) / p->tiles_per_slice;
    };
    p->f16 = 0;
    p->thin = 0;
    if (p->Cx <= 4 && p->ngroups == 1 && p->Cg <= 128 && (p->W & (p->W - 1)) == 0) {
        // whole rows per workgroup, ~1024 workgroups, the strip's halo + the partial sums inside 64 KB of LDS
        int R = 1;
        while (R * 2 <= p->H && p->H % (R * 2) == 0 && (long)p->B * p->H / (R * 2) >= 1024) R *= 2;
        WgradPlan q = *p;
        for (;; R /= 2) {
            q.thin = R;
            q.hh = R + ymax - ymin;
            q.hw = p->W + xmax - xmin;
            if (wgrad_thin_lds(q) <= kWgThinMaxLds || R == 1) break;
        }
        if (wgrad_thin_lds(q) <= kWgThinMaxLds) {
            p->thin = q.thin; p->hh = q.hh; p->hw = q.hw;
            p->imgplane = p->hh * p->hw;
            p->nslices = p->B * p->H / p->thin;
            p->ntiles = p->nslices;
            p->tiles_per_slice = 1;
            p->mi = 1;
            return true;
        }
    }
    if (TW >= 8 && p->Cx > 4 && !f32_route) {
        auto stride_halves = [](int halves) { int dw = (halves + 1) / 2; while (dw % 16 != 8) ++dw; return 2 * dw; };
        p->hp = (p->hw + 7) / 8 * 8;
        p->xs = stride_halves(p->imgs * p->hh * p->hp);
        p->gs = stride_halves(kWgPix);
        const int tasks = p->imgs * p->hh * ((p->hw + 1) / 2) * (kHwC / 4);
        if (tasks <= kHwXT * 256 && wgrad_f16_lds(*p) <= kWgMaxLds) {
            p->f16 = 1;
            p->mi = 3;
            // ~384 workgroups a launch (A/B on the box: 128 -> 1162 images/s at batch 8, 256 -> 1293, 384 -> 1294, 512 -> 1279,
            // 1024 -> 1247, 2048 -> 1172): fewer slices mean fewer prologues / accumulator flushes and a shorter reduce; below
            // one workgroup per CU the launch no longer fills the chip beside the main stream's kernels
            slice(384);
            return true;
        }
    }
    // input-channel tiles per workgroup: fewest padded tiles, each chunk charged one tile for its G traffic
    if (p->nhalo > kWgHaloBig) { *why = "wgrad: halo too large"; return false; }
    const int mi_max = p->nhalo > kWgHalo ? 2 : 3;
    int best = 1;
    double best_cost = 1e300;
    for (int mi = 1; mi <= mi_max; ++mi) {
        const double cost = (double)((p->Cx + 16 * mi - 1) / (16 * mi)) * (mi + 1.0);
        if (cost <= best_cost) { best = mi; best_cost = cost; }
    }
    p->mi = best;
    slice(1024);
    if (wgrad_f32_lds(*p) > kWgMaxLds) { *why = "wgrad: halo too large for the LDS"; return false; }
    return true;
}

size_t wgrad_ws_floats(const WgradPlan& p) { return (size_t)wgrad_grid(p).x * p.nslab * p.Cx * p.Cg; }

// The 16 instantiations.  big_lds: asks for more dynamic LDS than the default limit of a kernel (wgrad_init raises it).
typedef void (*WgKernel)(const WgradParams);
struct WgEntry { WgKernel fn; const char* name; bool big_lds; };
#define UMX_WG(big_lds, ...) {__VA_ARGS__, #__VA_ARGS__, big_lds}
static const WgEntry kWgTable[] = {
    UMX_WG(true, wgrad_mfma_f32<1,false>), UMX_WG(true, wgrad_mfma_f32<1,true>), UMX_WG(true, wgrad_mfma_f32<2,false>),
    UMX_WG(true, wgrad_mfma_f32<2,true>), UMX_WG(true, wgrad_mfma_f32<3,false>),
    UMX_WG(false, wgrad_thin_kernel<1,4>), UMX_WG(false, wgrad_thin_kernel<1,1>), UMX_WG(false, wgrad_thin_kernel<2,4>), UMX_WG(false, wgrad_thin_kernel<2,1>),
    UMX_WG(false, wgrad_thin_kernel<3,4>), UMX_WG(false, wgrad_thin_kernel<3,1>), UMX_WG(false, wgrad_thin_kernel<4,4>), UMX_WG(false, wgrad_thin_kernel<4,1>),
    UMX_WG(true, wgrad_f16x3<false,false>), UMX_WG(true, wgrad_f16x3<true,false>), UMX_WG(true, wgrad_f16x3<true,true>),
};
#undef UMX_WG
constexpr int kWgFirstThin = 5, kWgFirstF16 = 13;

WgradLaunch wgrad_select(const WgradPlan& p, const WgradOperands& o) {
    WgradLaunch l = {-1, "none", wgrad_grid(p), wgrad_lds(p), WG_SCALES_NONE};
    if (p.thin > 0) {
        if (p.Cx >= 1 && p.Cx <= 4) l.kernel = kWgFirstThin + 2 * (p.Cx - 1) + (wgrad_thin_v(p) == 4 ? 0 : 1);
    } else if (p.f16) {
        // octet staging: 16-byte aligned octets in both planes, and the halo's octet tasks inside the kernel's kOX per thread
        bool oc = o.planes && o.XCs % 8 == 0 && o.GCs % 8 == 0 && p.imgs * p.hh * ((p.hw + 1) / 2) * (kHwC / 8) <= kOX * 256;
        for (int sb = 0; sb < p.nslab && oc; ++sb) oc = p.coff[sb] % 8 == 0;
        l.kernel = kWgFirstF16 + (oc ? 2 : o.planes ? 1 : 0);
        l.scales = o.planes ? WG_SCALES_INV : WG_SCALES_MAX;
    } else {
        const bool big = p.nhalo > kWgHalo;   // the BIG variants exist for MI <= 2 only
        if (p.nhalo <= kWgHaloBig && p.mi >= 1 && p.mi <= (big ? 2 : 3)) l.kernel = 2 * (p.mi - 1) + (big ? 1 : 0);
    }
    if (l.kernel >= 0) l.name = kWgTable[l.kernel].name;
    return l;
}

// once per process: the LDS limit of every instantiation that needs more than the default; the first error is kept for every launch
static hipError_t wgrad_init() {
    static std::once_flag once;
    static hipError_t err = hipSuccess;
    std::call_once(once, [] {
        for (const WgEntry& k : kWgTable)
            if (k.big_lds && err == hipSuccess)
                err = hipFuncSetAttribute(reinterpret_cast<const void*>(k.fn), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kWgMaxLds);
    });
    return err;
}

hipError_t launch_wgrad(const WgradPlan& p, const WgradOperands& o, const WgradLaunch& l, hipStream_t stream) {
    if (l.kernel < 0) return hipErrorInvalidValue;
    if (const hipError_t e = wgrad_init()) return e;
    hipLaunchKernelGGL(kWgTable[l.kernel].fn, dim3(l.grid.x, l.grid.y, l.grid.z), dim3(256), l.lds, stream, WgradParams{p, o});
    return hipGetLastError();
}

struct WgReduce : WgradParams {
    int Ctot, c_off, reg_kind;
    float reg_c;
    float *g, *g2;
    const float* w;
    int scales;               // WG_SCALES_*: split-precision launches have their operand scales divided out here
};

// 256 threads = OUT outputs x SP slice partitions (SP a power of two chosen by the host): thread (o, sp) adds slices
// sp, sp+SP, ... in order; the SP partial sums are then added in order by the sp == 0 thread.
__global__ void __launch_bounds__(256) wgrad_reduce_kernel(const WgReduce q, int SP) {
    __shared__ double sm[256];
    const int OUT = 256 / SP;
    const int o = threadIdx.x % OUT, sp = threadIdx.x / OUT;
    const size_t n = (size_t)q.nslab * q.Cx * q.Cg;
    const size_t e = (size_t)blockIdx.x * OUT + o;
    double s = 0.0;
    if (e < n)
        for (int sl = sp; sl < q.nslices; sl += SP) s += (double)q.ws[(size_t)sl * n + e];
    sm[threadIdx.x] = s;
    __syncthreads();
    if (sp != 0 || e >= n) return;
    for (int j = 1; j < SP; ++j) s += sm[j * OUT + o];
    const int co = (int)(e % q.Cg);
    const size_t r = e / q.Cg;
    const int ci = (int)(r % q.Cx);
    const int sb = (int)(r / q.Cx);
    const size_t dsti = ((size_t)q.mslab[sb] * q.Ctot + q.c_off + ci) * q.Cg + co;
    if (q.scales == WG_SCALES_INV) s *= (double)(q.xinv ? *q.xinv : 1.f) * (double)(q.ginv ? *q.ginv : 1.f);
    else if (q.scales == WG_SCALES_MAX) s /= (double)wg_scale(q.xmax) * (double)wg_scale(q.gmax);
    float v = (float)s;
    if (q.g2) q.g2[dsti] = v;
    if (q.w && q.reg_kind) v += reg_grad(q.w[dsti], q.reg_kind, q.reg_c);
    q.g[dsti] = v;
}

hipError_t launch_wgrad_reduce(const WgradPlan& p, const WgradOperands& o, const WgradLaunch& l, int Ctot, int c_off, float* g,
                               const float* w, int reg_kind, float reg_c, float* g2, hipStream_t stream) {
    const WgReduce q{{p, o}, Ctot, c_off, reg_kind, reg_c, g, g2, w, l.scales};
    const size_t n = (size_t)p.nslab * p.Cx * p.Cg;
    int SP = 1;
    while (SP < 64 && SP * 8 < p.nslices) SP *= 2;
    const int OUT = 256 / SP;
    hipLaunchKernelGGL(wgrad_reduce_kernel, dim3((unsigned)((n + OUT - 1) / OUT)), dim3(256), 0, stream, q, SP);
    return hipGetLastError();
}

// "wgrad <what>: ..." as UMX_DEBUG_PLAN prints a layer's plan
std::string wgrad_describe(const WgradPlan& w, const char* what) {
    std::string groups;
    for (int g = 0; g < w.ngroups; ++g) groups += (g ? "/" : "") + std::to_string(w.gcount[g]);
    const WgGrid grid = wgrad_grid(w);
    char b[512];
    snprintf(b, sizeof b, "wgrad %s: %d x %d, X %d (of %d) ch x G %d ch, %d slabs in groups %s, %s, %d img/tile, %d tiles, %d slices x %d tiles, "
                          "grid %u x %u x %u",
             what, w.H, w.W, w.Cx, w.Cxt, w.Cg, w.nslab, groups.c_str(), w.thin ? "thin" : w.f16 ? "f16x3" : "fp32 mfma", w.imgs, w.ntiles,
             w.nslices, w.tiles_per_slice, grid.x, grid.y, grid.z);
    return b;
}

}  // namespace umx
