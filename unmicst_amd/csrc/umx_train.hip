// libumx training step: host side (the graphs' builds, buffers, launch sequence) and the C ABI of include/umx_train.h.  The plan of one
// convolution is umx_tconv.hip's, of one weight gradient umx_wgrad.hip's, the v2 step's stream schedule umx_tstep.hip's; the device
// arena is umx_arena.hip.
//
// The step is written out layer by layer rather than as a generic autograd tape: the v2 graph is fixed
// (reference UnMicst1-5.py:83-237), so every tensor the backward pass needs is known at create time and lives in a
// preallocated HBM buffer (pre-BN conv outputs z, layer inputs, up-sampled tensors); nothing is recomputed except the
// cheap element-wise BN/activation/dropout chain, and nothing is allocated during a step.
//
//   forward   conv (fp32 MFMA, raw) -> per-channel batch statistics -> BN + LeakyReLU + dropout (+ 2x2 max-pool)
//   backward  activation/pool/dropout backward + BN reductions -> BN input gradient -> weight gradient (fp32 MFMA,
//             umx_train_kernels.hip) and input gradient (the forward conv kernel on flipped/transposed filters; for a
//             stride-2 transposed conv: a 2x2-tap conv over the space-to-depth form of the output gradient)
//   update    Adam / Momentum over the flat parameter vector
#include "../../include/umx_train.h"
#include "umx_internal.h"
#include "umx_kernels.h"

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

using namespace umx;

namespace {

thread_local std::string g_terr;

struct TConv {                       // one convolution of the step: its host plan (umx_tconv.hip), then what upload_conv bound to it.  Run by
    TConvSpec spec;                  // conv_mfma_f32 on device-packed fp32 operands [tap][Cp][Np], rebuilt every step -- or (hidx >= 0, the
    TConvPlan plan;                  // default since round 4) repacked into conv_f16x3's weight images and run in split precision
    int order = -1;                  // position in the build (-1: the graph has no such convolution)
    ConvParams cp;                   // plan.cp with the operands bound
    float* packed[4][2] = {{nullptr, nullptr}, {nullptr, nullptr}, {nullptr, nullptr}, {nullptr, nullptr}};
    int hidx = -1;                   // index into umx_trainer::hls (split-precision plan), -1: fp32 kernel
    float* winv = nullptr;           // device scalar 2^-s: undoes the scale of the repacked weights in the epilogue
    int wsh = 0;                     // s (refresh_wscales re-derives it from plan.wsrc)
};

struct H16 {                         // (hi, lo) binary16 NHWC planes of one tensor, channels padded to Cs (what conv_f16x3 reads)
    _Float16* hi = nullptr;
    _Float16* lo = nullptr;
    int Cs = 0;
};

struct Act {                         // one fp32 NHWC tensor of the step and what travels with it
    float* x = nullptr;              // [B, S, S, C]
    H16 h;                           // its (hi, lo) planes; empty where none exist (the exact-fp32 route, cv[0]) or are withheld
    unsigned* max = nullptr;         // its max-|x| word in d_maxw, or NULL
    float* inv = nullptr;            // inverse scale its planes were stored with (a gradient: written with the planes), NULL for activations
    int S = 0, C = 0;
    size_t npix(int B) const { return (size_t)B * S * S; }
    Act without_planes() const { Act a = *this; a.h = H16(); return a; }
};

struct GradSlot {                    // a gradient buffer the layers take turns in
    float* x = nullptr;              // fp32, max_act floats
    _Float16 *hi = nullptr, *lo = nullptr;   // plane storage for the widest gradient the slot holds (NULL on the exact-fp32 route)
    float* inv = nullptr;            // where in d_xinv the writer of the planes leaves their inverse scale
    // the slot as the [B, S, S, C] gradient whose max word is `max` (planes false: withheld from its readers, and not written)
    Act view(int S, int C, unsigned* max, bool planes = true) const {
        Act a{x, H16(), max, inv, S, C};
        if (planes && hi) a.h = H16{hi, lo, round_up(C, 8)};
        return a;
    }
};

struct BnSite {            // one batch-normalised tensor
    int C = 0, H = 0, W = 0;
    size_t gamma = 0, beta = 0, mean = 0, var = 0;   // offsets in the parameter vector
    float* z = nullptr;    // [B,H,W,C] pre-BN
    float* stat = nullptr; // [4][C]
    float* m12 = nullptr;  // [2][C]
    unsigned* gmax = nullptr;   // max |dz| of the current step (float bits), for the split-precision weight gradient
    unsigned* bw = nullptr;     // three words: max_c |gamma rstd| (bn_finalize), max |g| and max |xhat| (act_bwd) -- the bound on |dz|
                                // that scales its (hi, lo) planes before the tensor exists (bn_bwd_apply)
};

struct Seg { std::string name; size_t off, n; float reg; int last; };   // last: the filter's last dimension (0: a BN block of 4 C)

struct LBlock {                 // one block of the legacy graph: a chain of nExtraConvs + 1 convolutions with ReLUs between them
    std::vector<TConv> fwd;     // fwd[0] reads the block input (down: w1; up: unused, c_fwd_u is the concat conv), fwd[e >= 1] reads
                                // a[e-1] (wextra_{e-1}); a down block's last one also reads the block input through the 1x1 shortcut
    std::vector<TConv> dg;      // dg[e >= 1]: input gradient of fwd[e] into a[e-1]
    std::vector<WgradPlan> wg;   // wg[e >= 1]: weight gradient of wextra_{e-1}
    std::vector<size_t> o_wx;   // wextra offsets in the parameter vector
    std::vector<float*> y;      // y[e]: output of conv e, pre-ReLU (down: y[E] = z = main + shortcut)
    std::vector<Act> a;         // a[e] = relu(y[e]) for the convolution after it: e < E (down), e <= E (up: a[E] is the output)
    std::vector<unsigned*> gmax;   // max |d loss / d y[e]| of the current step
    float* ident = nullptr;     // [4][C] identity statistics: act_fwd as a plain ReLU with the plane writer
    TConv dg_sh;                // (down) input gradient of the shortcut
    WgradPlan wg_sh;            // (down) weight gradient of the shortcut: one slab
};

}  // namespace

struct umx_trainer {
    umx_hparams hp;
    umx_train_options o;
    int device = 0, B = 0, L = 0, K = 0, P = 0;
    std::vector<int> n;                 // channel widths
    hipStream_t stream = nullptr;
    std::string err;
    umx::DevArena mem;                  // every device buffer below (UMX_DEBUG_GUARD: with red zones)
    int64_t step = 0;
    // parameters
    size_t nparams = 0;
    std::vector<Seg> segs;
    float *d_w = nullptr, *d_g = nullptr, *d_m = nullptr, *d_v = nullptr;
    // per-layer offsets into the parameter vector
    std::vector<size_t> o_w1, o_ws, o_wt, o_w2, o_bn_d, o_bn_u;
    size_t o_lb = 0, o_lt = 0, o_bn_b = 0, o_bn_t = 0;
    // activations, each with its planes and its max word (max |activation|, for the split-precision weight gradients)
    std::vector<Act> ds;                // ds[0] = data, ds[i+1] = pooled output of down layer i
    std::vector<BnSite> bn_d, bn_u;     // down layers / up layers (index = idx)
    BnSite bn_b, bn_t;
    Act act_b;                          // bottom output
    std::vector<Act> us, cv;            // per up layer idx
    float *d_labels = nullptr, *d_weights = nullptr, *d_probs = nullptr, *d_dt = nullptr;
    std::vector<float*> dskip;          // gradient w.r.t. ds[idx] from the up path (idx >= 1)
    float *DA = nullptr, *DB = nullptr;
    GradSlot dz[kSlots];       // gradient w.r.t. a conv output, one per slot: the weight gradients of layer l run on a side stream
    GradSlot gs[kSlots];       // while the main stream moves on to layers l+1 .. l+kSlots-1 (legacy: a chain alternates between dz[0] and
                               // dz[1]; gs[0] is the transposed conv's space-to-depth gradient)
    StepPlan plan;                                  // the v2 step's schedule (umx_tstep.hip), built once at create: enqueue_step walks it
    hipStream_t streams[kStepStreams] = {};         // by TStream: [TS_MAIN] == stream, the two side streams, the aux stream
    std::vector<hipEvent_t> events;                 // by the plan's event ids
    bool serial = false;                            // umx_test_trainer_serial: every step on the main stream in plan order, no events
    double* d_part = nullptr;  size_t part_doubles = 0;
    double* d_part2 = nullptr;          // the side stream's own partial sums (regularisation loss under the forward pass)
    double* d_loss = nullptr;           // [0] data term, [1] regularisation
    unsigned* d_maxw = nullptr;  int n_maxw = 0;   // per-tensor max |gradient| words, then the binary16 range flag
    std::vector<unsigned*> smax;        // max |gS| per up layer
    float* d_ws = nullptr;  size_t ws_floats = 0;
    float* d_ws2 = nullptr;             // ... of the second side stream
    float* d_split = nullptr;  size_t split_floats = 0;   // partial outputs of K-split convolutions
    float* d_split2 = nullptr;                            // ... of those enqueued on the side stream
    float* d_split3 = nullptr;                            // ... on the aux stream
    // forward / input-gradient convolutions on conv_f16x3 (UMX_TRAIN_CONV_F32=1: the exact-fp32 kernels of rounds 1-3)
    bool range_pending = false;         // a training step raised the range flag and an eval pass cleared it before umx_trainer_loss saw it
    bool hconv = true;
    bool wg_f32 = false;                // UMX_TRAIN_WGRAD_F32: no weight gradient takes the split-precision kernel
    bool wg_planes = true;              // the split-precision weight gradient stages from the planes
    bool no_ksplit = false;             // UMX_TRAIN_NO_KSPLIT: no convolution splits its K loop
    PlanSwitches sw;                    // the planner's switches (sw.debug_plan, UMX_DEBUG_PLAN: every plan's line on stderr)
    int nconvs = 0;                     // (during build) convolutions planned so far: TConv::order
    const float* h_blob = nullptr;      // (during build) the initial parameters on the host: weight scales
    std::vector<HConvParams> hls;       // the split-precision plans' launch parameters
    std::vector<TConv*> hconvs;         // the convolutions that took the split-precision route, index = RepackDesc::owner
    int wscale_every = 256;             // steps between two refreshes of the weight scales (UMX_TRAIN_WSCALE_EVERY)
    std::vector<float> h_params;        // (refresh) host copy of the parameters
    std::vector<RepackDesc> rdescs;
    RepackDesc* d_rdescs = nullptr;
    int max_refs = 0;
    int n_fwd_packs = 0, n_fwd_rdescs = 0;   // descriptors [0, n_fwd) serve the forward pass, the rest the backward pass only
    float* d_xinv = nullptr;            // [2 * kSlots] inverse scales of the dz / gS slots' planes, written by split_dyn_kernel
    // launches
    std::vector<TConv> c_fwd_d, c_dg_d, c_T, c_fwd_u, c_dg_us, c_dg_skip, c_dg_T;
    TConv c_fwd_b, c_dg_b;
    std::vector<WgradPlan> wg_d, wg_u0, wg_u1, wg_T;
    WgradPlan wg_b;
    std::vector<PackDesc> packs;
    PackDesc* d_packs = nullptr;
    RegSeg* d_regsegs = nullptr;  int n_regsegs = 0;
    InitSeg* d_initsegs = nullptr;  int cap_initsegs = 0;   // umx_trainer_init's table (allocated by its first call)
    size_t max_pack = 0;
    double flops_per_image = 0.0;
    // profiling
    bool prof = false;
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    double t_fwd = 0, t_bwd = 0, t_opt = 0;
    int t_steps = 0;
    bool pending = false;
    // legacy graph (GRAPH_LEGACY, reference UnMicst.py:80-186): build_legacy / forward_legacy / enqueue_legacy
    bool legacy = false;
    int E = 0;                          // nExtraConvs
    std::vector<LBlock> ldb, lub;       // down layer i / up layer idx
    float* lb_z = nullptr;              // bottom conv output, pre-ReLU
    float* lb_ident = nullptr;          // identity statistics of the bottom ReLU
    unsigned* lb_gmax = nullptr;
    float* lt_z = nullptr;              // logits
    float* ident_k = nullptr;           // identity statistics of the logits: the loss / softmax kernels without BN
    float* d_ones = nullptr;            // all-ones weights: the unweighted loss (weights == NULL)
    float* DSUM = nullptr;              // [2][max_act]: first-conv and shortcut input gradients, summed in that order
    size_t max_act = 0;
};

namespace {

int tfail(umx_trainer* tr, int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (tr) tr->err = buf; else g_terr = buf;
    return code;
}

#define T_HIP(tr, call)                                                                                   \
    do {                                                                                                  \
        hipError_t e_ = (call);                                                                           \
        if (e_ != hipSuccess)                                                                             \
            return tfail(tr, e_ == hipErrorOutOfMemory ? UMX_ERR_OOM : UMX_ERR_HIP, "%s failed: %s", #call, \
                         hipGetErrorString(e_));                                                          \
    } while (0)
#define T_TRY(call)                  \
    do {                             \
        int rc_ = (call);            \
        if (rc_ != UMX_OK) return rc_; \
    } while (0)

// every device buffer of the trainer: arena_alloc (guard mode: red zones); the macros record the destination as the buffer's label
template <typename T>
int talloc_(umx_trainer* tr, T** out, size_t count, bool zero, const char* label) {
    void* d = nullptr;
    T_HIP(tr, arena_alloc(&tr->mem, &d, count * sizeof(T), zero, label));
    *out = reinterpret_cast<T*>(d);
    return UMX_OK;
}

template <typename T>
int tupload_(umx_trainer* tr, T** out, const T* host, size_t count, const char* label) {
    T_TRY(talloc_(tr, out, count, false, label));
    if (count) T_HIP(tr, hipMemcpy(*out, host, count * sizeof(T), hipMemcpyHostToDevice));
    return UMX_OK;
}

#define talloc(tr, out, count) talloc_(tr, out, count, false, #out)
#define tzero(tr, out, count) talloc_(tr, out, count, true, #out)
#define tupload(tr, out, host, count) tupload_(tr, out, host, count, #out)

// ---- a convolution of the step: the host pass plans it (plan_conv -> umx_tconv.hip), the device pass uploads the plan (upload_conv)

// host pass: tc's plan and its place in the build; with UMX_DEBUG_PLAN its line.  A shape the planner refuses is the build's error.
int plan_conv(umx_trainer* tr, TConv& tc, const char* what, int H, int W, int Cout, int act, int nphase, int o_mul, const int* oy,
              const int* ox, int ngroups, const GroupSpec* gs, bool bwd) {
    TConvSpec& s = tc.spec;
    s.name = what;
    s.H = H; s.W = W; s.Cout = Cout; s.act = act; s.nphase = nphase; s.o_mul = o_mul;
    for (int ph = 0; ph < nphase; ++ph) { s.oy[ph] = oy ? oy[ph] : 0; s.ox[ph] = ox ? ox[ph] : 0; }
    s.ngroups = ngroups;
    for (int g = 0; g < ngroups; ++g) s.g[g] = gs[g];
    s.bwd = bwd;
    tc.order = tr->nconvs++;
    TConvEnv env;
    env.B = tr->B; env.imSize = tr->hp.imSize; env.hconv = tr->hconv; env.no_ksplit = tr->no_ksplit; env.params = tr->h_blob; env.sw = tr->sw;
    std::string why;
    if (!tconv_plan(s, env, &tc.plan, &why)) return tfail(tr, UMX_ERR_INVALID, "%s", why.c_str());
    if (tr->sw.debug_plan) {
        if (!tc.plan.refused.empty()) fprintf(stderr, "[umx train] %s stays on the fp32 kernel: %s\n", what, tc.plan.refused.c_str());
        fprintf(stderr, "[umx train] %s\n", tc.plan.text.c_str());
    }
    return UMX_OK;
}

// device pass: the plan's buffers in the order a convolution always had them -- fp32 operands per (phase, group), stages, epilogue
// constants, slabs per phase, winv, references per phase -- their pointers bound, and its pack / repack descriptors appended.
// (A direct convolution's fp32 operands stay allocated, though nothing reads them: the trainer's buffer sequence is unchanged.)
int upload_conv(umx_trainer* tr, TConv& tc) {
    const TConvSpec& s = tc.spec;
    TConvPlan& p = tc.plan;
    tc.cp = p.cp;
    for (size_t k = 0; k < p.operands.size(); ++k) {
        const int ph = p.operands[k].ph, g = p.operands[k].g;
        T_TRY(talloc(tr, &tc.packed[ph][g], p.operands[k].elems));
        tc.cp.ph[ph].w[g] = tc.packed[ph][g];
        if (p.packs.empty()) continue;
        PackDesc d = p.packs[k];
        d.dst = tc.packed[ph][g];
        d.w = tr->d_w + s.g[g].w_off;
        d.w2 = s.g[g].w2_off == SIZE_MAX ? nullptr : tr->d_w + s.g[g].w2_off;
        tr->packs.push_back(d);
    }
    tr->max_pack = std::max(tr->max_pack, p.max_pack);
    tr->split_floats = std::max(tr->split_floats, p.split_floats);
    if (p.split) {
        HConvParams h = p.P.h;
        HStage* stages = nullptr;
        float* econst = nullptr;
        T_TRY(tupload(tr, &stages, p.P.stages.data(), p.P.stages.size()));
        T_TRY(tupload(tr, &econst, p.P.econst.data(), p.P.econst.size()));
        h.stages = stages;
        h.econst = reinterpret_cast<const uint4*>(econst);
        for (int ph = 0; ph < s.nphase; ++ph) {
            _Float16* slab = nullptr;
            if (!p.P.wimg[ph].empty()) T_TRY(tupload(tr, &slab, p.P.wimg[ph].data(), p.P.wimg[ph].size()));
            h.ph[ph].w = reinterpret_cast<const uint4*>(slab);
        }
        tc.wsh = p.wsh;
        const float inv = std::ldexp(1.f, -tc.wsh);
        T_TRY(tupload(tr, &tc.winv, &inv, 1));
        for (int ph = 0; ph < s.nphase; ++ph) {
            const std::vector<HWRef>& refs = p.P.wrefs[ph];
            if (refs.empty()) continue;
            HWRefDev* d = nullptr;
            T_TRY(talloc(tr, &d, refs.size()));
            T_HIP(tr, hipMemcpy(d, refs.data(), refs.size() * sizeof(HWRefDev), hipMemcpyHostToDevice));
            RepackDesc rd;
            memset(&rd, 0, sizeof rd);
            rd.refs = d;
            rd.n = (int)refs.size();
            for (int g = 0; g < s.ngroups; ++g) {
                rd.arr[g] = p.direct ? tr->d_w + s.g[g].w_off : tc.packed[ph][g];
                rd.arr2[g] = p.direct && s.g[g].w2_off != SIZE_MAX ? tr->d_w + s.g[g].w2_off : nullptr;
                rd.estride[g] = p.direct ? (s.g[g].transpose ? 1 : s.g[g].d3) : 0;
            }
            rd.stride = tc.cp.Np;
            rd.scale = std::ldexp(1.f, tc.wsh);
            rd.slab = const_cast<uint4*>(h.ph[ph].w);
            rd.bwd = s.bwd ? 1 : 0;
            rd.owner = (int)tr->hconvs.size();
            tr->rdescs.push_back(rd);
            tr->max_refs = std::max(tr->max_refs, rd.n);
        }
        tc.hidx = (int)tr->hls.size();
        tr->hls.push_back(h);
        tr->hconvs.push_back(&tc);
    }
    p.P = HostPlan();   // (the tables are on the device now)
    return UMX_OK;
}

// Every convolution the host pass planned, in build order.  Called once the containers that hold them have their final size: the
// pointers stay good for the trainer's life (upload_conv, refresh_wscales).
std::vector<TConv*> planned_convs(umx_trainer* tr) {
    std::vector<TConv*> all;
    auto add = [&](TConv& tc) { if (tc.order >= 0) all.push_back(&tc); };
    for (std::vector<TConv>* v : {&tr->c_fwd_d, &tr->c_dg_d, &tr->c_T, &tr->c_fwd_u, &tr->c_dg_us, &tr->c_dg_skip, &tr->c_dg_T})
        for (TConv& tc : *v) add(tc);
    add(tr->c_fwd_b);
    add(tr->c_dg_b);
    for (std::vector<LBlock>* v : {&tr->ldb, &tr->lub})
        for (LBlock& b : *v) {
            for (TConv& tc : b.fwd) add(tc);
            for (TConv& tc : b.dg) add(tc);
            add(b.dg_sh);
        }
    std::sort(all.begin(), all.end(), [](const TConv* a, const TConv* b) { return a->order < b->order; });
    return all;
}

int upload_convs(umx_trainer* tr) {
    for (TConv* tc : planned_convs(tr)) T_TRY(upload_conv(tr, *tc));
    return UMX_OK;
}

std::string label_of(const std::string& array, int i) { return array + "[" + std::to_string(i) + "]"; }

// The planes of a (nothing on the exact-fp32 route: they stay empty)
int alloc_planes(umx_trainer* tr, Act& a, const std::string& label) {
    if (!tr->hconv) return UMX_OK;
    a.h.Cs = round_up(std::max(a.C, 1), 8);
    T_TRY(talloc_(tr, &a.h.hi, a.npix(tr->B) * a.h.Cs, true, (label + ".hi").c_str()));
    T_TRY(talloc_(tr, &a.h.lo, a.npix(tr->B) * a.h.Cs, true, (label + ".lo").c_str()));
    return UMX_OK;
}

// One tensor of the step (label: its name in the guard mode's messages): the fp32 buffer [B, S, S, C] and, unless withheld, its planes
int alloc_act(umx_trainer* tr, Act& a, const std::string& label, int S, int C, bool planes = true) {
    a.S = S; a.C = C;
    T_TRY(talloc_(tr, &a.x, a.npix(tr->B) * C, false, label.c_str()));
    return planes ? alloc_planes(tr, a, label) : UMX_OK;
}

// The gradient slots of a graph, in the order `slots` lists them (k < kSlots: dz[k], else gs[k - kSlots]; slot k's inverse scale is
// d_xinv[k]): their fp32 buffers of max_act floats ...
GradSlot& slot_of(umx_trainer* tr, int k) { return k < kSlots ? tr->dz[k] : tr->gs[k - kSlots]; }
std::string slot_label(int k) { return k < kSlots ? label_of("dz", k) : label_of("gs", k - kSlots); }
int alloc_slots(umx_trainer* tr, const std::vector<int>& slots, size_t max_act) {
    for (int k : slots) T_TRY(talloc_(tr, &slot_of(tr, k).x, max_act, false, slot_label(k).c_str()));
    return UMX_OK;
}
// ... and their planes, max_dz / max_gs halves each (the widest tensor a slot holds), with the inverse scales
int alloc_slot_planes(umx_trainer* tr, const std::vector<int>& slots, size_t max_dz, size_t max_gs) {
    if (!tr->hconv) return UMX_OK;
    for (int k : slots) {
        GradSlot& s = slot_of(tr, k);
        T_TRY(talloc_(tr, &s.hi, k < kSlots ? max_dz : max_gs, true, (slot_label(k) + ".hi").c_str()));
        T_TRY(talloc_(tr, &s.lo, k < kSlots ? max_dz : max_gs, true, (slot_label(k) + ".lo").c_str()));
    }
    T_TRY(tzero(tr, &tr->d_xinv, 2 * kSlots));
    for (int k : slots) slot_of(tr, k).inv = tr->d_xinv + k;
    return UMX_OK;
}

// a's fp32 tensor -> the (hi, lo) planes conv_f16x3 reads.  A gradient (a.inv) is scaled by its max word, which its writer has left in
// place; an activation is stored as it is and (omax) gets its max word written in the same pass
int to_h16(umx_trainer* tr, const Act& a, hipStream_t st, bool omax = false) {
    if (!tr->hconv) return UMX_OK;
    T_HIP(tr, launch_split_dyn(a.x, a.npix(tr->B), a.C, a.h.Cs, a.inv ? a.max : nullptr, a.inv, a.h.hi, a.h.lo,
                               reinterpret_cast<int*>(tr->d_maxw + tr->n_maxw), omax ? a.max : nullptr, st));
    return UMX_OK;
}

int pack_all(umx_trainer* tr, hipStream_t st, int part);
int refresh_wscales(umx_trainer* tr);

// a convolution on stream st, on whichever route its plan took: conv_f16x3 reads the (hi, lo) planes of src (+ src1; src.inv: the
// inverse scale of its planes where they hold a gradient), conv_mfma_f32 their fp32 tensors.  A K-split launch writes raw partial
// sums to `scratch` (one per stream: d_split is the main stream's), then the ordered reduce applies the activation.
int run_tconv(umx_trainer* tr, TConv& tc, const Act& src, float* dst, const Act* src1, hipStream_t st, float* scratch) {
    if (tc.hidx < 0) {
        ConvParams p = tc.cp;
        p.src[0] = src.x;
        p.src[1] = src1 ? src1->x : nullptr;
        p.dst = dst;
        p.B = tr->B;
        if (p.ksplit > 1) {
            p.dst = scratch;
            p.act = ACT_NONE;
        }
        T_HIP(tr, launch_conv(p, tc.plan.nt, tc.plan.hpix, st));
        if (p.ksplit > 1) T_HIP(tr, launch_split_reduce(scratch, p.ksplit, p.split_stride, p.split_stride, tc.cp.act, dst, st));
        return UMX_OK;
    }
    HConvParams p = tr->hls[tc.hidx];
    p.B = tr->B;
    p.overflow_flag = reinterpret_cast<int*>(tr->d_maxw + tr->n_maxw);
    const H16* h16[2] = {&src.h, src1 ? &src1->h : &src.h};
    for (int gi = 0; gi < 2; ++gi) {
        p.src_hi[gi] = gi == 0 || src1 ? h16[gi]->hi : nullptr;
        p.src_lo[gi] = gi == 0 || src1 ? h16[gi]->lo : nullptr;
        p.Cs[gi] = h16[gi]->Cs;
        p.srcA[gi] = h16[gi]->Cs * 2;
        p.srcB[gi] = 16;
    }
    p.dst_f32 = dst;
    p.dyn[0] = tc.winv;
    p.dyn[1] = src.inv;
    if (p.ksplit > 1) {
        const int act = p.act;
        p.act = ACT_NONE;
        p.dst_f32 = scratch;
        T_HIP(tr, launch_conv_f16(p, st));
        T_HIP(tr, launch_split_reduce(scratch, p.ksplit, p.split_stride, p.split_stride, act, dst, st));
        return UMX_OK;
    }
    T_HIP(tr, launch_conv_f16(p, st));
    return UMX_OK;
}

int run_tconv(umx_trainer* tr, TConv& tc, const Act& src, float* dst, const Act* src1, hipStream_t st) {   // (on the main stream)
    return run_tconv(tr, tc, src, dst, src1, st, tr->d_split);
}

// an activation written by a kernel without a plane writer (the input batch, the transposed convolutions' outputs): its max |x|
// for the split-precision weight gradient (training) and, on the split-precision route, its planes -- there in the same pass
int track_act(umx_trainer* tr, const Act& a, bool training) {
    if (training && !tr->hconv) T_HIP(tr, launch_absmax(a.x, a.npix(tr->B) * a.C, a.max, tr->stream));
    return to_h16(tr, a, tr->stream, training);
}

int setup_wgrad(umx_trainer* tr, WgradPlan& w, const char* what, int H, int Cxt, int Cx, int Cg, const TapSet& slabs,
                const std::vector<int>& coff) {
    memset(&w, 0, sizeof w);
    w.B = tr->B; w.H = H; w.W = H;
    w.Cxt = Cxt; w.Cx = Cx; w.Cg = Cg;
    w.nslab = (int)slabs.off.size();
    if (w.nslab > kWgMaxSlabs) return tfail(tr, UMX_ERR_INVALID, "%s: too many filter taps", what);
    for (int s = 0; s < w.nslab; ++s) {
        w.dy[s] = (short)slabs.off[s].first;
        w.dx[s] = (short)slabs.off[s].second;
        w.mslab[s] = (short)slabs.m[s];
        w.coff[s] = coff.empty() ? 0 : coff[s];
    }
    std::string why;
    if (!wgrad_setup(&w, tr->wg_f32, &why)) return tfail(tr, UMX_ERR_INVALID, "%s: %s", what, why.c_str());
    tr->ws_floats = std::max(tr->ws_floats, wgrad_ws_floats(w));
    if (tr->sw.debug_plan) fprintf(stderr, "[umx train] %s\n", wgrad_describe(w, what).c_str());
    return UMX_OK;
}

unsigned long long mix64_host(unsigned long long x) {
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}
unsigned long long drop_key(const umx_trainer* tr, int layer_id) {
    return mix64_host(tr->o.seed + 0x9E3779B97F4A7C15ull * (unsigned long long)(64 * tr->step + layer_id + 1));
}

int bn_alloc(umx_trainer* tr, BnSite& s, int C, int H, size_t off_gamma) {
    s.C = C; s.H = s.W = H;
    s.gamma = off_gamma; s.beta = off_gamma + C; s.mean = off_gamma + 2 * (size_t)C; s.var = off_gamma + 3 * (size_t)C;
    T_TRY(talloc(tr, &s.z, (size_t)tr->B * H * H * C));
    T_TRY(talloc(tr, &s.stat, 4 * (size_t)C));
    T_TRY(talloc(tr, &s.m12, 2 * (size_t)C));
    return UMX_OK;
}

// z -> statistics -> stat (and the moving averages when updating)
int bn_forward_stats(umx_trainer* tr, BnSite& s, bool update, bool training = true) {
    if (!training) {
        T_HIP(tr, launch_bn_stat_from_moving(s.C, tr->d_w + s.gamma, tr->d_w + s.beta, tr->d_w + s.mean, tr->d_w + s.var,
                                             s.stat, tr->stream));
        return UMX_OK;
    }
    const size_t N = (size_t)tr->B * s.H * s.W;
    const int nblk = chan_blocks(N, s.C);
    T_HIP(tr, launch_chan_stats(s.z, N, s.C, tr->d_part, nblk, tr->stream));
    T_HIP(tr, launch_bn_finalize(tr->d_part, nblk, N, s.C, tr->d_w + s.gamma, tr->d_w + s.beta, tr->d_w + s.mean,
                                 tr->d_w + s.var, update ? tr->o.bn_momentum : 1.0f, s.stat, s.bw, tr->stream));
    return UMX_OK;
}

ActParams act_params(const umx_trainer* tr, const BnSite& s, int pool, int act, float rate, int layer_id) {
    ActParams a;
    a.z = s.z; a.stat = s.stat;
    a.B = tr->B; a.H = s.H; a.W = s.W; a.C = s.C;
    a.pool = pool; a.act = act;
    a.drop_rate = rate > 0.f ? rate : 0.f;
    a.drop_key = drop_key(tr, layer_id);
    return a;
}

// dy (+dy1) -> gradient w.r.t. z in dz (its max word: s.gmax); BN parameter gradients into the gradient vector
// (where dz has planes -- an input-gradient convolution on conv_f16x3 reads it -- they and their inverse scale are written in the same pass)
int bn_backward(umx_trainer* tr, BnSite& s, const ActParams& a, const float* dy0, const float* dy1, const Act& dz) {
    const size_t N = (size_t)tr->B * s.H * s.W;
    const size_t rows = a.pool ? N / 4 : N;
    const int nblk = chan_blocks(rows, s.C);
    const bool planes = dz.h.hi != nullptr;
    T_HIP(tr, launch_act_bwd(a, dy0, dy1, dz.x, tr->d_part, nblk, planes ? s.bw + 1 : nullptr, tr->stream));
    T_HIP(tr, launch_bn_bwd_finalize(tr->d_part, nblk, N, s.C, tr->d_g + s.gamma, tr->d_g + s.beta, s.m12, tr->stream));
    T_HIP(tr, launch_bn_bwd_apply_max(dz.x, s.z, s.stat, s.m12, N, s.C, s.gmax, s.bw, dz.inv, dz.h.hi, dz.h.lo, dz.h.Cs,
                                      reinterpret_cast<int*>(tr->d_maxw + tr->n_maxw), tr->stream));
    return UMX_OK;
}

// (where both operands have (hi, lo) planes the split-precision kernel stages from them -- half the bytes, no conversion -- and undoes
// the inverse scales they were stored with; ws: the slice workspace of the stream it runs on)
int run_wgrad(umx_trainer* tr, const WgradPlan& w, const Act& X, const Act& G, int Ctot, int c_off, size_t w_off, float reg,
              size_t pair_off /* SIZE_MAX: none */, float* ws, hipStream_t stream) {
    WgradOperands o = {};
    o.X = X.x;
    o.G = G.x;
    if (w.f16 && tr->wg_planes && X.h.hi && G.h.hi && w.Cxt <= X.h.Cs && w.Cg <= G.h.Cs) {
        o.planes = 1;
        o.Xhi = X.h.hi; o.Xlo = X.h.lo; o.XCs = X.h.Cs;
        o.Ghi = G.h.hi; o.Glo = G.h.lo; o.GCs = G.h.Cs;
        o.xinv = X.inv; o.ginv = G.inv;
    }
    o.ws = ws;
    o.xmax = X.max;
    o.gmax = G.max;
    o.overflow = reinterpret_cast<int*>(tr->d_maxw + tr->n_maxw);
    const WgradLaunch l = wgrad_select(w, o);
    T_HIP(tr, launch_wgrad(w, o, l, stream));
    T_HIP(tr, launch_wgrad_reduce(w, o, l, Ctot, c_off, tr->d_g + w_off, tr->d_w + w_off, reg > 0.f ? tr->o.reg_kind : 0, reg,
                                  pair_off == SIZE_MAX ? nullptr : tr->d_g + pair_off, stream));
    return UMX_OK;
}

float up_rate(const umx_trainer* tr, int idx) { return tr->o.drop_up0 - tr->o.drop_up_step * idx; }
float down_rate(const umx_trainer* tr, int i) { return tr->o.drop_down_step * i; }

enum { LAYER_DOWN = 0, LAYER_BOTTOM = 16, LAYER_UP = 32 };   // dropout stream ids (oracle/train_oracle.py)

// forward of the graph up to the top layer's pre-BN output (UnMicst1-5.py:83-222).  training: batch statistics + dropout;
// otherwise the moving statistics, no dropout (tfTraining: 0)
int forward_pass(umx_trainer* tr, const float* data, bool training, bool update) {
    const int L = tr->L;
    hipStream_t st = tr->stream;
    const umx_train_options& o = tr->o;
    int* const flagp = reinterpret_cast<int*>(tr->d_maxw + tr->n_maxw);
    // (training: every activation that the backward pass feeds to the split-precision weight gradient gets its max |v|
    // tracked by the kernel that writes it -- the input batch and the transposed-conv outputs by a pass of their own)
    // BN + LeakyReLU (+ 2x2 max-pool) + dropout of site s into out, which gets its (hi, lo) planes written by the same kernel
    // (the exact-fp32 route has no plane buffers: out.h is empty then)
    auto act = [&](BnSite& s, int pool, float rate, int layer_id, const Act& out) -> int {
        T_HIP(tr, launch_act_fwd(act_params(tr, s, pool, ACT_LEAKY, training ? rate : 0.f, layer_id), out.x, training ? out.max : nullptr,
                                 out.h.hi, out.h.lo, out.h.Cs, flagp, st));
        return UMX_OK;
    };
    tr->ds[0].x = const_cast<float*>(data);
    T_TRY(track_act(tr, tr->ds[0], training));
    for (int i = 0; i < L; ++i) {
        BnSite& s = tr->bn_d[i];
        T_TRY(run_tconv(tr, tr->c_fwd_d[i], tr->ds[i], s.z, nullptr, st));
        T_TRY(bn_forward_stats(tr, s, update, training));
        T_TRY(act(s, 1, down_rate(tr, i), LAYER_DOWN + i, tr->ds[i + 1]));
    }
    T_TRY(run_tconv(tr, tr->c_fwd_b, tr->ds[L], tr->bn_b.z, nullptr, st));
    T_TRY(bn_forward_stats(tr, tr->bn_b, update, training));
    T_TRY(act(tr->bn_b, 0, o.drop_bottom, LAYER_BOTTOM, tr->act_b));
    const Act* cur = &tr->act_b;
    for (int idx = L - 1; idx >= 0; --idx) {
        BnSite& s = tr->bn_u[idx];
        T_TRY(run_tconv(tr, tr->c_T[idx], *cur, tr->us[idx].x, nullptr, st));
        T_TRY(track_act(tr, tr->us[idx], training));
        T_TRY(run_tconv(tr, tr->c_fwd_u[idx], tr->ds[idx], s.z, &tr->us[idx], st));
        T_TRY(bn_forward_stats(tr, s, update, training));
        // (cv[0] has no planes: only the 1x1 head reads it)
        T_TRY(act(s, 0, up_rate(tr, idx), LAYER_UP + idx, tr->cv[idx]));
        cur = &tr->cv[idx];
    }
    BnSite& t = tr->bn_t;
    T_HIP(tr, launch_head_fwd(tr->cv[0].x, (size_t)tr->B * tr->P * tr->P, tr->n[1], tr->K, tr->d_w + tr->o_lt, t.z, st));
    T_TRY(bn_forward_stats(tr, t, update, training));
    return UMX_OK;
}

// start of a step (both graphs): the weight scales' periodic refresh, the profile's first event, loss and max words zeroed
int step_begin(umx_trainer* tr, bool update) {
    hipStream_t st = tr->stream;
    if (update && tr->step > 0 && tr->wscale_every > 0 && tr->step % tr->wscale_every == 0) T_TRY(refresh_wscales(tr));
    if (tr->prof) T_HIP(tr, hipEventRecord(tr->ev[0], st));
    T_HIP(tr, hipMemsetAsync(tr->d_loss, 0, 2 * sizeof(double), st));
    // (the range flag behind the max words is NOT cleared here: it stays up until umx_trainer_loss / umx_trainer_eval has
    // reported it, so an overflow in a step whose loss is never read is not lost under the next step -- ADVICE r4)
    T_HIP(tr, hipMemsetAsync(tr->d_maxw, 0, tr->n_maxw * sizeof(unsigned), st));
    return UMX_OK;
}

// softmax + weighted cross-entropy of the logits (normalised by stat) -> probs, d loss / d logits (d_dt) and the data term
int loss_head(umx_trainer* tr, const float* logits, const float* stat, const float* labels, const float* weights) {
    const size_t Npix = (size_t)tr->B * tr->P * tr->P;
    const int nblk = loss_blocks(Npix);
    T_HIP(tr, launch_softmax_loss(logits, stat, labels, weights, Npix, tr->K, tr->o.clip_eps, tr->d_probs, tr->d_dt, tr->d_part, nblk,
                                  tr->stream));
    T_HIP(tr, launch_sum_to_scalar(tr->d_part, nblk, 1.0 / (double)Npix, tr->d_loss, 0, 0, tr->stream));
    return UMX_OK;
}

// end of a step (both graphs, every gradient in place on the main stream): the optimiser over the flat vector (UnMicst1-5.py:361-380,
// UnMicst.py:270-279; BN moving statistics were updated in the forward pass) and the profile's last events
int step_end(umx_trainer* tr, bool update) {
    hipStream_t st = tr->stream;
    const umx_train_options& o = tr->o;
    if (tr->prof) T_HIP(tr, hipEventRecord(tr->ev[2], st));
    if (update) {
        OptParams op;
        op.kind = o.optimizer;
        const double lr = (double)o.lr0 * std::pow((double)o.decay_rate, (double)(tr->step / std::max(1, o.decay_steps)));
        const double tt = (double)(tr->step + 1);
        op.lr = (float)lr;
        op.lr_t = (float)(lr * std::sqrt(1.0 - std::pow((double)o.beta2, tt)) / (1.0 - std::pow((double)o.beta1, tt)));
        op.beta1 = o.beta1; op.beta2 = o.beta2; op.eps = o.adam_eps; op.momentum = o.momentum;
        T_HIP(tr, launch_optimizer(op, tr->d_w, tr->d_g, tr->d_m, tr->d_v, tr->nparams, st));
        tr->step += 1;
    }
    if (tr->prof) {
        T_HIP(tr, hipEventRecord(tr->ev[3], st));
        tr->pending = true;
    }
    return UMX_OK;
}

struct SiteRef { BnSite* s; int pool, act; float rate; int layer_id; };   // a BN site of the plan and its activation in this graph
SiteRef site_ref(umx_trainer* tr, int site) {
    const int L = tr->L, i = 2 * L - site;
    if (site == site_top(L)) return {&tr->bn_t, 0, ACT_NONE, 0.f, 0};
    if (site == site_bottom(L)) return {&tr->bn_b, 0, ACT_LEAKY, tr->o.drop_bottom, LAYER_BOTTOM};
    if (site < L) return {&tr->bn_u[site], 0, ACT_LEAKY, up_rate(tr, site), LAYER_UP + site};
    return {&tr->bn_d[i], 1, ACT_LEAKY, down_rate(tr, i), LAYER_DOWN + i};
}

// A buffer of a step at `site` by its id in the plan (umx_tstep.hip): an activation with its planes and max word; a dz slot as the
// site's gradient w.r.t. its conv output (down layer 0: no convolution reads dz's planes, so none are written, and the weight
// gradient stages from the fp32 tensors); a gS slot as up layer `site`'s space-to-depth gradient; anything else as its pointer in .x.
// enqueue_step takes every operand it hands to a helper from here: a step cannot touch a buffer its plan line does not declare.
Act buffer(umx_trainer* tr, int id, int site) {
    const int k = id % 32, idx = std::min(site, tr->L - 1);
    const BnSite& s = *site_ref(tr, site).s;
    float* raw = nullptr;
    switch (id / 32) {
    case TB_DS: return tr->ds[k];
    case TB_US: return tr->us[k];
    case TB_CV: return tr->cv[k];
    case TB_ACTB: return tr->act_b;
    case TB_DZ: return tr->dz[k].view(s.H, s.C, s.gmax, site != site_down(tr->L, 0));
    case TB_GS: return tr->gs[k].view(tr->us[idx].S / 2, 4 * tr->n[idx + 1], tr->smax[idx]);
    case TB_DA: raw = tr->DA; break;
    case TB_DB: raw = tr->DB; break;
    case TB_DT: raw = tr->d_dt; break;
    case TB_DSKIP: raw = tr->dskip[k]; break;
    case TB_PART: raw = reinterpret_cast<float*>(tr->d_part); break;
    case TB_PART2: raw = reinterpret_cast<float*>(tr->d_part2); break;
    case TB_WS: raw = tr->d_ws; break;
    case TB_WS2: raw = tr->d_ws2; break;
    case TB_SPLIT: raw = tr->d_split; break;
    case TB_SPLIT2: raw = tr->d_split2; break;
    case TB_SPLIT3: raw = tr->d_split3; break;
    }   // (z / stat / m12, the packs, the loss words and the gradient segments reach their kernels through the site, the descriptors and
    return Act{raw};   // the parameter offsets: declared for the hazard check, never resolved)
}

// One v2 training step: a walk over the plan.  Per step: its stream waits on the step's events, the step's helper is enqueued on it
// with the buffers the step names, and the step's events are recorded.  Which wait protects which buffer is the plan's business
// (step_plan; tests/test_step_plan_cpu.py checks it); every kernel has a fixed summation order, so the step is bit-reproducible and
// equal to the serial walk (tr->serial: everything on the main stream in plan order).
int enqueue_step(umx_trainer* tr, const float* data, const float* labels, const float* weights, bool update) {
    const StepPlan& p = tr->plan;
    const umx_train_options& o = tr->o;
    const int L = tr->L, K = tr->K;
    const std::vector<int>& n = tr->n;
    const size_t Npix = (size_t)tr->B * tr->P * tr->P;
    for (const TStep& s : p.steps) {
        hipStream_t st = tr->streams[tr->serial ? TS_MAIN : s.stream];
        for (int k = 0; k < s.nwait && !tr->serial; ++k) T_HIP(tr, hipStreamWaitEvent(st, tr->events[s.wait[k]], 0));
        const SiteRef sr = site_ref(tr, s.site);
        const int idx = s.site < L ? s.site : 0, i = s.site > L ? 2 * L - s.site : 0;   // the up / down layer of a step that has one
        const int Cskip = n[idx], Cup = n[idx + 1];
        auto R = [&](int k) { return buffer(tr, p.rd(s, k), s.site); };
        auto W = [&](int k) { return buffer(tr, p.wr(s, k), s.site); };
        auto wgrad = [&](const WgradPlan& w, const Act& X, int Ctot, int c_off, size_t w_off, float reg, size_t pair = SIZE_MAX) {
            return run_wgrad(tr, w, X, R(1), Ctot, c_off, w_off, reg, pair, W(1).x, st);
        };
        auto conv = [&](TConv& tc) { return run_tconv(tr, tc, R(0), W(0).x, nullptr, st, W(1).x); };
        switch (s.op) {
        case T_BEGIN: T_TRY(step_begin(tr, update)); break;
        case T_PACK0: T_TRY(pack_all(tr, st, 0)); break;
        case T_PACK1: T_TRY(pack_all(tr, st, 1)); break;
        case T_REG: T_HIP(tr, launch_reg_loss(tr->d_regsegs, tr->n_regsegs, o.reg_kind, reinterpret_cast<double*>(W(0).x), tr->d_loss, 1, st)); break;
        case T_FWD: T_TRY(forward_pass(tr, data, true, update)); break;
        case T_LOSS: T_TRY(loss_head(tr, tr->bn_t.z, tr->bn_t.stat, labels, weights)); break;
        case T_MARK: if (tr->prof) T_HIP(tr, hipEventRecord(tr->ev[1], st)); break;
        case T_HEAD: {   // top layer: softmax/CE gradient -> BN (in place: dt -> dt0) -> 1x1 conv
            float* const dt = R(0).x;
            double* const part = reinterpret_cast<double*>(W(2).x);
            const int nblk = chan_blocks(Npix, n[1]);
            T_TRY(bn_backward(tr, *sr.s, act_params(tr, *sr.s, 0, ACT_NONE, 0.f, 0), dt, nullptr, Act{dt}));
            T_HIP(tr, launch_head_bwd(R(3).x, dt, tr->d_w + tr->o_lt, Npix, n[1], K, W(3).x, part, nblk, st));
            T_HIP(tr, launch_reduce_partials(part, nblk, n[1] * K, 1.0, tr->d_g + tr->o_lt, tr->d_w + tr->o_lt,
                                             o.reg_top > 0.f ? o.reg_kind : 0, o.reg_top, st));
            break;
        }
        case T_DZ:
            T_TRY(bn_backward(tr, *sr.s, act_params(tr, *sr.s, sr.pool, sr.act, sr.rate, sr.layer_id), R(0).x, s.nr > 3 ? R(3).x : nullptr, W(0)));
            break;
        case T_WG_U0: T_TRY(wgrad(tr->wg_u0[idx], R(0), Cskip + Cup, 0, tr->o_w2[idx], o.reg_up)); break;
        case T_WG_U1: T_TRY(wgrad(tr->wg_u1[idx], R(0), Cskip + Cup, Cskip, tr->o_w2[idx], o.reg_up)); break;
        case T_WG_T: {   // (the transposed convolution's filter: X is gS, G the layer's input)
            const bool gs_planes = tr->hconv && (tr->c_dg_T[idx].hidx >= 0 || tr->wg_planes);
            T_TRY(wgrad(tr->wg_T[idx], gs_planes ? R(0) : R(0).without_planes(), Cup, 0, tr->o_wt[idx], o.reg_up));
            break;
        }
        case T_WG_B: T_TRY(wgrad(tr->wg_b, R(0), n[L], 0, tr->o_lb, o.reg_bottom)); break;
        case T_WG_D:   // c00 + shortcut = conv(x, W1 + Wshort): both filters receive the same data gradient (UnMicst1-5.py:102-114)
            T_TRY(wgrad(tr->wg_d[i], i >= 1 ? R(0) : R(0).without_planes(), n[i], 0, tr->o_ws[i], o.reg_down, tr->o_w1[i]));
            break;
        case T_CV_US: T_TRY(conv(tr->c_dg_us[idx])); break;
        case T_CV_SKIP: T_TRY(conv(tr->c_dg_skip[idx])); break;
        case T_CV_T: T_TRY(conv(tr->c_dg_T[idx])); break;
        case T_CV_B: T_TRY(conv(tr->c_dg_b)); break;
        case T_CV_D: T_TRY(conv(tr->c_dg_d[i])); break;
        case T_S2D: T_HIP(tr, launch_leaky_bwd_s2d_max(R(0).x, R(1).x, tr->B, W(0).S, Cup, 0.2f, W(0).x, W(0).max, st)); break;
        case T_GSP: T_TRY(to_h16(tr, W(0), st)); break;
        case T_JOIN: break;
        case T_OPT: T_TRY(step_end(tr, update)); break;
        }
        for (int k = 0; k < s.nrec && !tr->serial; ++k) T_HIP(tr, hipEventRecord(tr->events[s.rec[k]], st));
    }
    return UMX_OK;
}

int fold_profile(umx_trainer* tr) {
    if (!tr->pending) return UMX_OK;
    T_HIP(tr, hipEventSynchronize(tr->ev[3]));
    float a = 0, b = 0, c = 0;
    T_HIP(tr, hipEventElapsedTime(&a, tr->ev[0], tr->ev[1]));
    T_HIP(tr, hipEventElapsedTime(&b, tr->ev[1], tr->ev[2]));
    T_HIP(tr, hipEventElapsedTime(&c, tr->ev[2], tr->ev[3]));
    tr->t_fwd += a; tr->t_bwd += b; tr->t_opt += c;
    tr->t_steps += 1;
    tr->pending = false;
    return UMX_OK;
}

void fill_common(umx_train_options* o) {
    memset(o, 0, sizeof *o);
    o->optimizer = UMX_OPT_ADAM;
    o->momentum = 0.9f;
    o->beta1 = 0.9f; o->beta2 = 0.999f; o->adam_eps = 1e-8f;
    o->bn_momentum = 0.99f;
    o->seed = 1234;
}

// One up layer's convolutions (shared by both graphs): the stride-2 transposed conv (forward with `act_T` fused, input gradient on
// the space-to-depth output gradient, weight gradient), then the concat conv [ds_idx, us] -> Cup (forward, input gradients into us and
// -- idx >= 1 -- into the skip, weight gradients of both halves).  S: the layer's input size on entry, its output size on return.
int setup_up_layer(umx_trainer* tr, int idx, int& S, int act_T, double& mac_total) {
    const std::vector<int>& n = tr->n;
    const int ks = tr->hp.ks;
    const TapSet fwd = same_taps(ks, false), flp = same_taps(ks, true);
    char nm[64];
    snprintf(nm, sizeof nm, "lu%d", idx);
    const int Cskip = n[idx], Cup = n[idx + 1], Cin = n[idx + 2];
    {   // transposed conv forward: 4 sub-pixel phases; its activation fused
        GroupSpec g = one_group(Cin, tr->o_wt[idx], SIZE_MAX, Cup, Cin, 1, 0, TapSet());
        int oy[4], ox[4];
        transposed_fwd_taps(ks, &g, oy, ox);
        T_TRY(plan_conv(tr, tr->c_T[idx], nm, S, S, Cup, act_T, 4, 2, oy, ox, 1, &g, false));
        mac_total += (double)S * S * ks * ks * Cin * Cup;
    }
    {   // transposed conv backward: a stride-1 conv over the space-to-depth form of the output gradient
        GroupSpec g = one_group(4 * Cup, tr->o_wt[idx], SIZE_MAX, Cup, Cin, 0, 0, TapSet());
        TapSet slabs;
        std::vector<int> coff;
        transposed_bwd_taps(ks, Cup, &g, &slabs, &coff);
        T_TRY(plan_conv(tr, tr->c_dg_T[idx], nm, S, S, Cin, ACT_NONE, 1, 1, nullptr, nullptr, 1, &g, true));
        T_TRY(setup_wgrad(tr, tr->wg_T[idx], nm, S, 4 * Cup, Cup, Cin, slabs, coff));
        mac_total += 2.0 * S * S * ks * ks * Cin * Cup;
    }
    S *= 2;
    {
        GroupSpec g2[2] = {one_group(Cskip, tr->o_w2[idx], SIZE_MAX, Cskip + Cup, Cup, 0, 0, fwd),
                           one_group(Cup, tr->o_w2[idx], SIZE_MAX, Cskip + Cup, Cup, 0, Cskip, fwd)};
        T_TRY(plan_conv(tr, tr->c_fwd_u[idx], nm, S, S, Cup, ACT_NONE, 1, 1, nullptr, nullptr, 2, g2, false));
        mac_total += tr->c_fwd_u[idx].plan.mac;
        GroupSpec gu = one_group(Cup, tr->o_w2[idx], SIZE_MAX, Cskip + Cup, Cup, 1, Cskip, flp);
        T_TRY(plan_conv(tr, tr->c_dg_us[idx], nm, S, S, Cup, ACT_NONE, 1, 1, nullptr, nullptr, 1, &gu, true));
        mac_total += tr->c_dg_us[idx].plan.mac;
        if (idx >= 1) {
            GroupSpec gk = one_group(Cup, tr->o_w2[idx], SIZE_MAX, Cskip + Cup, Cup, 1, 0, flp);
            T_TRY(plan_conv(tr, tr->c_dg_skip[idx], nm, S, S, Cskip, ACT_NONE, 1, 1, nullptr, nullptr, 1, &gk, true));
            mac_total += tr->c_dg_skip[idx].plan.mac;
        }
        T_TRY(setup_wgrad(tr, tr->wg_u0[idx], nm, S, Cskip, Cskip, Cup, fwd, {}));
        T_TRY(setup_wgrad(tr, tr->wg_u1[idx], nm, S, Cup, Cup, Cup, fwd, {}));
        mac_total += (double)S * S * ks * ks * (Cskip + Cup) * Cup;
    }
    return UMX_OK;
}

// ---- the build frame both graphs share

// L, K, P and the channel widths n[0..L+1] from the hyper-parameters
void set_shape(umx_trainer* tr) {
    const umx_hparams& hp = tr->hp;
    tr->L = hp.nLayers; tr->K = hp.nClasses; tr->P = hp.imSize;
    tr->n = {hp.nChannels, hp.nOut0};
    for (int i = 0; i < tr->L; ++i) tr->n.push_back(tr->n.back() * hp.featMapsFact);
}

// (host pass) the blob is the parameter vector of nparams floats the graph's build has laid out: the plans' weight scales come from it
int take_blob(umx_trainer* tr, const float* blob, size_t blob_floats, size_t nparams) {
    tr->nparams = nparams;
    if (blob_floats != nparams)
        return tfail(tr, UMX_ERR_BLOB, "weight blob has %zu floats, the graph needs %zu", blob_floats, nparams);
    tr->h_blob = blob;
    tr->ds.resize(tr->L + 1); tr->us.resize(tr->L);
    return UMX_OK;
}

// (device pass) the parameter vector from the blob; its gradient and the optimiser's two slots
int alloc_params(umx_trainer* tr) {
    const size_t nparams = tr->nparams;
    const float* blob = tr->h_blob;
    T_TRY(tupload(tr, &tr->d_w, blob, nparams));
    T_TRY(tzero(tr, &tr->d_g, nparams));
    T_TRY(tzero(tr, &tr->d_m, nparams));
    T_TRY(tzero(tr, &tr->d_v, nparams));
    return UMX_OK;
}

// the route of the forward / input-gradient convolutions: split precision (planes of every tensor they read; the graph's build
// allocates them) unless UMX_TRAIN_CONV_F32 asks for the exact-fp32 kernels -- and the other switches of the environment, each read here, once
void select_route(umx_trainer* tr) {
    tr->hconv = !getenv("UMX_TRAIN_CONV_F32");
    tr->wg_f32 = getenv("UMX_TRAIN_WGRAD_F32") != nullptr;
    tr->no_ksplit = getenv("UMX_TRAIN_NO_KSPLIT") != nullptr;
    tr->sw = plan_switches_from_env();
    if (const char* e = getenv("UMX_TRAIN_WSCALE_EVERY")) tr->wscale_every = atoi(e);
}

// the bottom layer (the same in both graphs) at size S: forward conv, input gradient, weight gradient
int setup_bottom(umx_trainer* tr, int S, double& mac_total) {
    const std::vector<int>& n = tr->n;
    const int L = tr->L, ks = tr->hp.ks;
    const TapSet fwd = same_taps(ks, false), flp = same_taps(ks, true);
    GroupSpec g = one_group(n[L], tr->o_lb, SIZE_MAX, n[L], n[L + 1], 0, 0, fwd);
    T_TRY(plan_conv(tr, tr->c_fwd_b, "lb", S, S, n[L + 1], ACT_NONE, 1, 1, nullptr, nullptr, 1, &g, false));
    GroupSpec gd = one_group(n[L + 1], tr->o_lb, SIZE_MAX, n[L], n[L + 1], 1, 0, flp);
    T_TRY(plan_conv(tr, tr->c_dg_b, "lb", S, S, n[L], ACT_NONE, 1, 1, nullptr, nullptr, 1, &gd, true));
    T_TRY(setup_wgrad(tr, tr->wg_b, "lb", S, n[L], n[L], n[L + 1], fwd, {}));
    mac_total += tr->c_fwd_b.plan.mac + tr->c_dg_b.plan.mac + (double)S * S * ks * ks * n[L] * n[L + 1];
    return UMX_OK;
}

// end of the host pass: FLOPs per image (+ the 1x1 head)
void finish_plan(umx_trainer* tr, double mac_total) {
    mac_total += 3.0 * tr->P * tr->P * tr->n[1] * tr->K;
    tr->flops_per_image = 2.0 * mac_total;
}

// end of the device pass, once every convolution is uploaded: the weight gradients' slice workspace and the K-split scratch
// (side_streams: also those of the side streams), the regularised segments, and the pack / repack descriptors
int finish_build(umx_trainer* tr, bool side_streams) {
    T_TRY(talloc(tr, &tr->d_ws, tr->ws_floats));
    if (side_streams) T_TRY(talloc(tr, &tr->d_ws2, tr->ws_floats));
    T_TRY(talloc(tr, &tr->d_split, tr->split_floats));
    if (side_streams) {
        T_TRY(talloc(tr, &tr->d_split2, tr->split_floats));
        T_TRY(talloc(tr, &tr->d_split3, tr->split_floats));
    }
    std::vector<RegSeg> rs;
    for (const Seg& sg : tr->segs)
        if (sg.reg > 0.f) rs.push_back(RegSeg{tr->d_w + sg.off, sg.n, sg.reg});
    tr->n_regsegs = (int)rs.size();
    if (!rs.empty()) T_TRY(tupload(tr, &tr->d_regsegs, rs.data(), rs.size()));
    // forward operands first: the backward-only ones are packed on the side stream while the forward pass runs
    tr->n_fwd_packs = (int)(std::stable_partition(tr->packs.begin(), tr->packs.end(), [](const PackDesc& d) { return d.bwd == 0; }) -
                            tr->packs.begin());
    tr->n_fwd_rdescs = (int)(std::stable_partition(tr->rdescs.begin(), tr->rdescs.end(), [](const RepackDesc& d) { return d.bwd == 0; }) -
                             tr->rdescs.begin());
    T_TRY(tupload(tr, &tr->d_packs, tr->packs.data(), tr->packs.size()));
    if (!tr->rdescs.empty()) T_TRY(tupload(tr, &tr->d_rdescs, tr->rdescs.data(), tr->rdescs.size()));
    tr->h_blob = nullptr;
    return UMX_OK;
}

// The v2 graph's host pass: shape, parameter layout, and the plan of every convolution and weight gradient.  Nothing is allocated.
int plan_trainer(umx_trainer* tr, const float* blob, size_t blob_floats) {
    set_shape(tr);
    const int L = tr->L, ks = tr->hp.ks, P = tr->P, K = tr->K;
    const std::vector<int>& n = tr->n;
    const umx_train_options& o = tr->o;

    // ---- parameter vector layout (== unmicst_amd/model.py tensor_specs, nExtraConvs == 0)
    size_t pos = 0;
    auto seg = [&](const std::string& name, size_t cnt, float reg, int last) { tr->segs.push_back({name, pos, cnt, reg, last}); pos += cnt; return pos - cnt; };
    tr->o_bn_d.resize(L); tr->o_bn_u.resize(L);
    tr->o_w1.resize(L); tr->o_ws.resize(L); tr->o_wt.resize(L); tr->o_w2.resize(L);
    char nm[64];
    for (int i = 0; i < L; ++i) {
        snprintf(nm, sizeof nm, "ld%d", i);
        tr->o_w1[i] = seg(std::string(nm) + ".w1", (size_t)ks * ks * n[i] * n[i + 1], 0.f, n[i + 1]);
        tr->o_ws[i] = seg(std::string(nm) + ".wshort", (size_t)ks * ks * n[i] * n[i + 1], o.reg_down, n[i + 1]);
        tr->o_bn_d[i] = seg(std::string(nm) + ".bn", 4 * (size_t)n[i + 1], 0.f, 0);
    }
    tr->o_lb = seg("lb.w", (size_t)ks * ks * n[L] * n[L + 1], o.reg_bottom, n[L + 1]);
    tr->o_bn_b = seg("lb.bn", 4 * (size_t)n[L + 1], 0.f, 0);
    for (int idx = L - 1; idx >= 0; --idx) {
        snprintf(nm, sizeof nm, "lu%d", idx);
        tr->o_wt[idx] = seg(std::string(nm) + ".wt", (size_t)ks * ks * n[idx + 1] * n[idx + 2], o.reg_up, n[idx + 2]);
        tr->o_w2[idx] = seg(std::string(nm) + ".w2", (size_t)ks * ks * (n[idx] + n[idx + 1]) * n[idx + 1], o.reg_up, n[idx + 1]);
        tr->o_bn_u[idx] = seg(std::string(nm) + ".bn", 4 * (size_t)n[idx + 1], 0.f, 0);
    }
    tr->o_lt = seg("lt.w", (size_t)n[1] * K, o.reg_top, K);
    tr->o_bn_t = seg("lt.bn", 4 * (size_t)K, 0.f, 0);
    T_TRY(take_blob(tr, blob, blob_floats, pos));

    // ---- conv launches
    tr->wg_planes = tr->hconv;
    tr->c_fwd_d.resize(L); tr->c_dg_d.resize(L); tr->c_T.resize(L); tr->c_fwd_u.resize(L);
    tr->c_dg_us.resize(L); tr->c_dg_skip.resize(L); tr->c_dg_T.resize(L);
    tr->wg_d.resize(L); tr->wg_u0.resize(L); tr->wg_u1.resize(L); tr->wg_T.resize(L);
    const TapSet fwd = same_taps(ks, false), flp = same_taps(ks, true);
    double mac_total = 0.0;
    int S = P;
    for (int i = 0; i < L; ++i) {
        snprintf(nm, sizeof nm, "ld%d", i);
        GroupSpec g = one_group(n[i], tr->o_w1[i], tr->o_ws[i], n[i], n[i + 1], 0, 0, fwd);
        T_TRY(plan_conv(tr, tr->c_fwd_d[i], nm, S, S, n[i + 1], ACT_NONE, 1, 1, nullptr, nullptr, 1, &g, false));
        mac_total += tr->c_fwd_d[i].plan.mac;
        if (i >= 1) {
            GroupSpec gd = one_group(n[i + 1], tr->o_w1[i], tr->o_ws[i], n[i], n[i + 1], 1, 0, flp);
            T_TRY(plan_conv(tr, tr->c_dg_d[i], nm, S, S, n[i], ACT_NONE, 1, 1, nullptr, nullptr, 1, &gd, true));
            mac_total += tr->c_dg_d[i].plan.mac;
        }
        T_TRY(setup_wgrad(tr, tr->wg_d[i], nm, S, n[i], n[i], n[i + 1], fwd, {}));
        mac_total += (double)S * S * ks * ks * n[i] * n[i + 1];
        S /= 2;
    }
    T_TRY(setup_bottom(tr, S, mac_total));
    for (int idx = L - 1; idx >= 0; --idx) T_TRY(setup_up_layer(tr, idx, S, ACT_LEAKY, mac_total));
    finish_plan(tr, mac_total);
    return UMX_OK;
}

// The v2 graph's device pass: parameters, activations, planes, every convolution's upload in build order, the shared buffers.
int alloc_trainer(umx_trainer* tr) {
    const int L = tr->L, P = tr->P, K = tr->K, B = tr->B;
    const std::vector<int>& n = tr->n;
    T_TRY(alloc_params(tr));

    // ---- activations: shapes and fp32 buffers; their planes follow below
    tr->bn_d.resize(L); tr->bn_u.resize(L);
    tr->cv.resize(L); tr->dskip.assign(L, nullptr);
    size_t max_act = (size_t)B * P * P * std::max(n[0], K), max_dz = 0, max_gs = 0;
    auto grad_size = [&](size_t npix, int C) { max_act = std::max(max_act, npix * C); max_dz = std::max(max_dz, npix * round_up(C, 8)); };
    int S = P;
    for (int i = 0; i < L; ++i) {
        T_TRY(bn_alloc(tr, tr->bn_d[i], n[i + 1], S, tr->o_bn_d[i]));
        grad_size((size_t)B * S * S, n[i + 1]);
        T_TRY(alloc_act(tr, tr->ds[i + 1], label_of("ds", i + 1), S / 2, n[i + 1], false));
        if (i + 1 <= L - 1) T_TRY(talloc(tr, &tr->dskip[i + 1], (size_t)B * (S / 2) * (S / 2) * n[i + 1]));
        S /= 2;
    }
    T_TRY(bn_alloc(tr, tr->bn_b, n[L + 1], S, tr->o_bn_b));
    T_TRY(alloc_act(tr, tr->act_b, "act_b", S, n[L + 1], false));
    grad_size((size_t)B * S * S, n[L + 1]);
    for (int idx = L - 1; idx >= 0; --idx) {
        max_gs = std::max(max_gs, (size_t)B * S * S * round_up(4 * n[idx + 1], 8));
        S *= 2;
        T_TRY(alloc_act(tr, tr->us[idx], label_of("us", idx), S, n[idx + 1], false));
        T_TRY(bn_alloc(tr, tr->bn_u[idx], n[idx + 1], S, tr->o_bn_u[idx]));
        T_TRY(alloc_act(tr, tr->cv[idx], label_of("cv", idx), S, n[idx + 1], false));
        grad_size((size_t)B * S * S, n[idx + 1]);
    }
    T_TRY(bn_alloc(tr, tr->bn_t, K, P, tr->o_bn_t));
    T_TRY(talloc(tr, &tr->d_labels, (size_t)B * P * P * K));
    T_TRY(talloc(tr, &tr->d_weights, (size_t)B * P * P * K));
    T_TRY(talloc(tr, &tr->d_probs, (size_t)B * P * P * K));
    T_TRY(talloc(tr, &tr->d_dt, (size_t)B * P * P * K));
    T_TRY(alloc_act(tr, tr->ds[0], label_of("ds", 0), P, n[0], false));
    T_TRY(talloc(tr, &tr->DA, max_act));
    T_TRY(talloc(tr, &tr->DB, max_act));
    std::vector<int> slots;   // dz[0], gs[0], dz[1], gs[1], ...
    for (int sl = 0; sl < kSlots; ++sl) { slots.push_back(sl); slots.push_back(kSlots + sl); }
    T_TRY(alloc_slots(tr, slots, max_act));
    int maxC = K;
    for (int v : n) maxC = std::max(maxC, v);
    tr->part_doubles = std::max<size_t>((size_t)1024 * 2 * maxC, (size_t)1024 * n[1] * K) + 1024;
    T_TRY(talloc(tr, &tr->d_part, tr->part_doubles));
    T_TRY(talloc(tr, &tr->d_part2, tr->part_doubles));
    T_TRY(tzero(tr, &tr->d_loss, 2));
    {   // max-|gradient| words: one per batch-normalised tensor and per up layer, + the range flag
        tr->n_maxw = 6 * L + 4 + 3 * (2 * L + 2);
        T_TRY(tzero(tr, &tr->d_maxw, (size_t)tr->n_maxw + 1));
        int k = 0;
        for (int i = 0; i < L; ++i) tr->bn_d[i].gmax = tr->d_maxw + k++;
        for (int i = 0; i < L; ++i) tr->bn_u[i].gmax = tr->d_maxw + k++;
        tr->bn_b.gmax = tr->d_maxw + k++;
        tr->bn_t.gmax = tr->d_maxw + k++;
        tr->smax.assign(L, nullptr);
        for (int i = 0; i < L; ++i) tr->smax[i] = tr->d_maxw + k++;
        for (std::vector<Act>* v : {&tr->ds, &tr->us, &tr->cv})
            for (Act& a : *v) a.max = tr->d_maxw + k++;
        tr->act_b.max = tr->d_maxw + k++;
        for (int i = 0; i < L; ++i) { tr->bn_d[i].bw = tr->d_maxw + k; k += 3; }
        for (int i = 0; i < L; ++i) { tr->bn_u[i].bw = tr->d_maxw + k; k += 3; }
        tr->bn_b.bw = tr->d_maxw + k; k += 3;
        tr->bn_t.bw = tr->d_maxw + k; k += 3;
    }

    // ---- split-precision route of the forward / input-gradient convolutions: planes of every tensor they read
    // (after every fp32 buffer, in this order: the allocation sequence, and with it the address layout, is the one this graph always had)
    for (int i = 0; i <= L; ++i) T_TRY(alloc_planes(tr, tr->ds[i], label_of("ds", i)));
    T_TRY(alloc_planes(tr, tr->act_b, "act_b"));
    for (int idx = L - 1; idx >= 0; --idx) {
        T_TRY(alloc_planes(tr, tr->us[idx], label_of("us", idx)));
        if (idx >= 1) T_TRY(alloc_planes(tr, tr->cv[idx], label_of("cv", idx)));   // (cv[0] has none: only the 1x1 head reads it)
    }
    T_TRY(alloc_slot_planes(tr, slots, max_dz, max_gs));

    T_TRY(upload_convs(tr));
    return finish_build(tr, true);
}

int build_trainer(umx_trainer* tr, const float* blob, size_t blob_floats) {
    T_TRY(plan_trainer(tr, blob, blob_floats));
    return alloc_trainer(tr);
}

// the step's weights -> the operands of every convolution: fp32 [tap][Cp][Np] (both routes), then conv_f16x3's weight images
// (part 0: the forward pass's operands, 1: the backward-only ones, 2: all)
// Every `wscale_every` steps the per-layer weight scales are re-derived from the parameters as they are now (one copy of the vector
// to the host: 124 MB for the synthetic-256 graph, < 1 % of 256 steps), so that a long run cannot grow a filter out of the
// 32 x headroom the scale of step 0 left it.  Called with nothing in flight that reads the scales.
int refresh_wscales(umx_trainer* tr) {
    if (tr->hconvs.empty()) return UMX_OK;
    T_HIP(tr, hipStreamSynchronize(tr->stream));
    tr->h_params.resize(tr->nparams);
    T_HIP(tr, hipMemcpy(tr->h_params.data(), tr->d_w, tr->nparams * sizeof(float), hipMemcpyDeviceToHost));
    bool changed = false;
    for (size_t k = 0; k < tr->hconvs.size(); ++k) {
        TConv& tc = *tr->hconvs[k];
        const int sh = wscale_shift(operand_wmax(tc.plan.wsrc, tr->h_params.data()));
        if (sh == tc.wsh) continue;
        tc.wsh = sh;
        const float inv = std::ldexp(1.f, -sh);
        T_HIP(tr, hipMemcpy(tc.winv, &inv, sizeof inv, hipMemcpyHostToDevice));
        for (RepackDesc& rd : tr->rdescs)
            if (rd.owner == (int)k) rd.scale = std::ldexp(1.f, sh);
        changed = true;
    }
    if (changed)
        T_HIP(tr, hipMemcpy(tr->d_rdescs, tr->rdescs.data(), tr->rdescs.size() * sizeof(RepackDesc), hipMemcpyHostToDevice));
    return UMX_OK;
}

int pack_all(umx_trainer* tr, hipStream_t st, int part) {
    const int p0 = part == 1 ? tr->n_fwd_packs : 0, p1 = part == 0 ? tr->n_fwd_packs : (int)tr->packs.size();
    const int r0 = part == 1 ? tr->n_fwd_rdescs : 0, r1 = part == 0 ? tr->n_fwd_rdescs : (int)tr->rdescs.size();
    if (p1 > p0) T_HIP(tr, launch_pack_weights(tr->d_packs + p0, p1 - p0, tr->max_pack, st));
    if (r1 > r0)
        T_HIP(tr, launch_repack_f16x3(tr->d_rdescs + r0, r1 - r0, tr->max_refs, reinterpret_cast<int*>(tr->d_maxw + tr->n_maxw), st));
    return UMX_OK;
}

// ================================================================================================================================
// The legacy graph (GRAPH_LEGACY, reference UnMicst.py:80-186, the graph of every shipped checkpoint), trained as UnMicst.py:270-279:
//   down i   y_0 = conv(x, w1); y_e = conv(relu(y_{e-1}), wextra_{e-1}); z = y_E + conv1x1(x, wshort) (second K slab of the last conv);
//            ds_{i+1} = maxpool2(BN(relu(z))) with batch statistics -- ReLU, then BN, then the pool (on the BN output: gamma may be < 0)
//   bottom   relu(conv(ds_L, lb.w))
//   up idx   us = relu(convT_s2(x, wt)); y_0 = conv([ds_idx, us], w2); y_e = conv(relu(y_{e-1}), wextra_{e-1}); output relu(y_E)
//   top      softmax(conv1x1(x, lt.w)); loss mean_{b,y,x}(-sum_k w labels log p) (w = 1: weights == NULL)
// No BN outside the down blocks: the loss and softmax kernels read identity statistics.  ReLU forward = act_fwd on identity statistics
// (it writes the planes of what the next convolution reads); ReLU backward = relu_bwd_kernel, then the planes (split_dyn).  Every
// launch is on the main stream, in a fixed order; every reduction has a fixed order (no float atomics).
// ================================================================================================================================
int alloc_ident(umx_trainer* tr, float** out, int C) {
    std::vector<float> h(4 * (size_t)C, 0.f);
    for (int c = 0; c < C; ++c) { h[C + c] = 1.f; h[2 * C + c] = 1.f; }   // mean 0 | rstd 1 | scale 1 | shift 0
    return tupload(tr, out, h.data(), h.size());
}

// The legacy graph's host pass: shape, parameter layout, and the plan of every convolution and weight gradient.  Nothing is allocated.
int plan_legacy(umx_trainer* tr, const float* blob, size_t blob_floats) {
    set_shape(tr);
    const int L = tr->L, ks = tr->hp.ks, P = tr->P, K = tr->K, E = tr->hp.nExtraConvs;
    tr->E = E;
    const std::vector<int>& n = tr->n;

    // ---- parameter vector layout (== unmicst_amd/model.py tensor_specs, GRAPH_LEGACY)
    size_t pos = 0;
    auto seg = [&](const std::string& name, size_t cnt, int last) { tr->segs.push_back({name, pos, cnt, 0.f, last}); pos += cnt; return pos - cnt; };
    tr->o_bn_d.resize(L);
    tr->o_w1.resize(L); tr->o_ws.resize(L); tr->o_wt.resize(L); tr->o_w2.resize(L);
    tr->ldb.resize(L); tr->lub.resize(L);
    char nm[64];
    for (int i = 0; i < L; ++i) {
        const std::string p = "ld" + std::to_string(i);
        tr->o_w1[i] = seg(p + ".w1", (size_t)ks * ks * n[i] * n[i + 1], n[i + 1]);
        for (int e = 0; e < E; ++e) tr->ldb[i].o_wx.push_back(seg(p + ".wextra" + std::to_string(e), (size_t)ks * ks * n[i + 1] * n[i + 1], n[i + 1]));
        tr->o_ws[i] = seg(p + ".wshort", (size_t)n[i] * n[i + 1], n[i + 1]);
        tr->o_bn_d[i] = seg(p + ".bn", 4 * (size_t)n[i + 1], 0);
    }
    tr->o_lb = seg("lb.w", (size_t)ks * ks * n[L] * n[L + 1], n[L + 1]);
    for (int idx = L - 1; idx >= 0; --idx) {
        const std::string p = "lu" + std::to_string(idx);
        tr->o_wt[idx] = seg(p + ".wt", (size_t)ks * ks * n[idx + 1] * n[idx + 2], n[idx + 2]);
        tr->o_w2[idx] = seg(p + ".w2", (size_t)ks * ks * (n[idx] + n[idx + 1]) * n[idx + 1], n[idx + 1]);
        for (int e = 0; e < E; ++e) tr->lub[idx].o_wx.push_back(seg(p + ".wextra" + std::to_string(e), (size_t)ks * ks * n[idx + 1] * n[idx + 1], n[idx + 1]));
    }
    tr->o_lt = seg("lt.w", (size_t)n[1] * K, K);
    T_TRY(take_blob(tr, blob, blob_floats, pos));

    // ---- conv launches
    tr->wg_planes = tr->hconv;
    tr->c_dg_d.resize(L); tr->c_T.resize(L); tr->c_fwd_u.resize(L);
    tr->c_dg_us.resize(L); tr->c_dg_skip.resize(L); tr->c_dg_T.resize(L);
    tr->wg_d.resize(L); tr->wg_u0.resize(L); tr->wg_u1.resize(L); tr->wg_T.resize(L);
    for (std::vector<LBlock>* v : {&tr->ldb, &tr->lub})
        for (LBlock& b : *v) { b.fwd.resize(E + 1); b.dg.resize(E + 1); b.wg.resize(E + 1); }
    const TapSet fwd = same_taps(ks, false), flp = same_taps(ks, true);
    TapSet ctr;   // the 1x1 shortcut: one tap at the centre
    ctr.off.push_back({0, 0});
    ctr.m.push_back(0);
    double mac_total = 0.0;
    // extra conv e >= 1 of a chain at size S with C channels: forward (ngroups 2: + the shortcut group g1), input and weight gradient
    auto extra = [&](LBlock& b, int e, int S, int C, int ngroups, const GroupSpec* g1) -> int {
        GroupSpec g[2] = {one_group(C, b.o_wx[e - 1], SIZE_MAX, C, C, 0, 0, fwd), g1 ? *g1 : GroupSpec()};
        T_TRY(plan_conv(tr, b.fwd[e], nm, S, S, C, ACT_NONE, 1, 1, nullptr, nullptr, ngroups, g, false));
        GroupSpec gd = one_group(C, b.o_wx[e - 1], SIZE_MAX, C, C, 1, 0, flp);
        T_TRY(plan_conv(tr, b.dg[e], nm, S, S, C, ACT_NONE, 1, 1, nullptr, nullptr, 1, &gd, true));
        T_TRY(setup_wgrad(tr, b.wg[e], nm, S, C, C, C, fwd, {}));
        mac_total += b.fwd[e].plan.mac + b.dg[e].plan.mac + (double)S * S * ks * ks * C * C;
        return UMX_OK;
    };
    int S = P;
    for (int i = 0; i < L; ++i) {
        snprintf(nm, sizeof nm, "ld%d", i);
        LBlock& b = tr->ldb[i];
        const int Ci = n[i], C = n[i + 1];
        const GroupSpec gsh = one_group(Ci, tr->o_ws[i], SIZE_MAX, Ci, C, 0, 0, ctr);
        GroupSpec g[2] = {one_group(Ci, tr->o_w1[i], SIZE_MAX, Ci, C, 0, 0, fwd), gsh};
        T_TRY(plan_conv(tr, b.fwd[0], nm, S, S, C, ACT_NONE, 1, 1, nullptr, nullptr, E == 0 ? 2 : 1, g, false));
        mac_total += b.fwd[0].plan.mac;
        for (int e = 1; e <= E; ++e) T_TRY(extra(b, e, S, C, e == E ? 2 : 1, &gsh));
        if (i >= 1) {
            GroupSpec gd = one_group(C, tr->o_w1[i], SIZE_MAX, Ci, C, 1, 0, flp);
            GroupSpec gs = one_group(C, tr->o_ws[i], SIZE_MAX, Ci, C, 1, 0, ctr);
            T_TRY(plan_conv(tr, tr->c_dg_d[i], nm, S, S, Ci, ACT_NONE, 1, 1, nullptr, nullptr, 1, &gd, true));
            T_TRY(plan_conv(tr, b.dg_sh, nm, S, S, Ci, ACT_NONE, 1, 1, nullptr, nullptr, 1, &gs, true));
            mac_total += tr->c_dg_d[i].plan.mac + b.dg_sh.plan.mac;
        }
        T_TRY(setup_wgrad(tr, tr->wg_d[i], nm, S, Ci, Ci, C, fwd, {}));
        T_TRY(setup_wgrad(tr, b.wg_sh, nm, S, Ci, Ci, C, ctr, {}));
        mac_total += (double)S * S * (ks * ks + 1) * Ci * C;
        S /= 2;
    }
    T_TRY(setup_bottom(tr, S, mac_total));
    for (int idx = L - 1; idx >= 0; --idx) {
        T_TRY(setup_up_layer(tr, idx, S, ACT_RELU, mac_total));
        snprintf(nm, sizeof nm, "lu%d", idx);
        for (int e = 1; e <= E; ++e) T_TRY(extra(tr->lub[idx], e, S, n[idx + 1], 1, nullptr));
    }
    finish_plan(tr, mac_total);
    return UMX_OK;
}

// The legacy graph's device pass: parameters, activations with their planes, every convolution's upload in build order, the shared buffers.
int alloc_legacy(umx_trainer* tr) {
    const int L = tr->L, P = tr->P, K = tr->K, B = tr->B, E = tr->E;
    const std::vector<int>& n = tr->n;
    T_TRY(alloc_params(tr));

    // ---- max words (zeroed every step), then the range flag; handed out below, once the tensors exist
    tr->n_maxw = 16 + 4 * (L + 1) * (2 * E + 6);
    T_TRY(tzero(tr, &tr->d_maxw, (size_t)tr->n_maxw + 1));

    // ---- activations
    tr->bn_d.resize(L);
    tr->dskip.assign(L, nullptr);
    // a chain's tensors: y[0..E], a[0..na)
    auto chain = [&](LBlock& b, const std::string& name, int S, int C, int na) -> int {
        b.y.assign(E + 1, nullptr); b.a.resize(na);
        for (int e = 0; e <= E; ++e) T_TRY(talloc(tr, &b.y[e], (size_t)B * S * S * C));
        for (int e = 0; e < na; ++e) T_TRY(alloc_act(tr, b.a[e], label_of(name + ".a", e), S, C));
        return alloc_ident(tr, &b.ident, C);
    };
    size_t max_act = (size_t)B * P * P * std::max(n[0], K), max_dz = 0, max_gs = 0;
    auto grad_size = [&](size_t npix, int C) { max_act = std::max(max_act, npix * C); max_dz = std::max(max_dz, npix * round_up(C, 8)); };
    int S = P;
    T_TRY(alloc_act(tr, tr->ds[0], label_of("ds", 0), P, n[0]));
    for (int i = 0; i < L; ++i) {
        T_TRY(chain(tr->ldb[i], label_of("ldb", i), S, n[i + 1], E));
        T_TRY(bn_alloc(tr, tr->bn_d[i], n[i + 1], S, tr->o_bn_d[i]));   // (its z: relu(z), what BN normalises)
        grad_size((size_t)B * S * S, n[i + 1]);
        T_TRY(alloc_act(tr, tr->ds[i + 1], label_of("ds", i + 1), S / 2, n[i + 1]));
        if (i + 1 <= L - 1) T_TRY(talloc(tr, &tr->dskip[i + 1], (size_t)B * (S / 2) * (S / 2) * n[i + 1]));
        S /= 2;
    }
    T_TRY(talloc(tr, &tr->lb_z, (size_t)B * S * S * n[L + 1]));
    T_TRY(alloc_act(tr, tr->act_b, "act_b", S, n[L + 1]));
    T_TRY(alloc_ident(tr, &tr->lb_ident, n[L + 1]));
    grad_size((size_t)B * S * S, n[L + 1]);
    for (int idx = L - 1; idx >= 0; --idx) {
        max_gs = std::max(max_gs, (size_t)B * S * S * round_up(4 * n[idx + 1], 8));
        S *= 2;
        T_TRY(alloc_act(tr, tr->us[idx], label_of("us", idx), S, n[idx + 1]));
        T_TRY(chain(tr->lub[idx], label_of("lub", idx), S, n[idx + 1], E + 1));
        grad_size((size_t)B * S * S, n[idx + 1]);
    }
    T_TRY(talloc(tr, &tr->lt_z, (size_t)B * P * P * K));
    T_TRY(alloc_ident(tr, &tr->ident_k, K));
    T_TRY(talloc(tr, &tr->d_labels, (size_t)B * P * P * K));
    T_TRY(talloc(tr, &tr->d_weights, (size_t)B * P * P * K));
    T_TRY(talloc(tr, &tr->d_probs, (size_t)B * P * P * K));
    T_TRY(talloc(tr, &tr->d_dt, (size_t)B * P * P * K));
    const std::vector<float> ones((size_t)B * P * P * K, 1.f);
    T_TRY(tupload(tr, &tr->d_ones, ones.data(), ones.size()));
    tr->max_act = max_act;
    T_TRY(talloc(tr, &tr->DA, max_act));
    T_TRY(talloc(tr, &tr->DB, max_act));
    const std::vector<int> slots = {0, 1, kSlots};   // gradient slots: dz[0] and dz[1] for a chain (alternating), gs[0] for the
    T_TRY(alloc_slots(tr, slots, max_act));          // transposed conv's space-to-depth gradient
    T_TRY(talloc(tr, &tr->DSUM, 2 * max_act));
    int maxC = K;
    for (int v : n) maxC = std::max(maxC, v);
    tr->part_doubles = std::max<size_t>((size_t)1024 * 2 * maxC, (size_t)1024 * n[1] * K) + 1024;
    T_TRY(talloc(tr, &tr->d_part, tr->part_doubles));
    T_TRY(tzero(tr, &tr->d_loss, 2));

    T_TRY(alloc_slot_planes(tr, slots, max_dz, max_gs));

    // ---- every tensor's max word
    int k = 0;
    auto word = [&]() { return tr->d_maxw + k++; };
    tr->smax.assign(L, nullptr);
    for (Act& a : tr->ds) a.max = word();
    for (int i = 0; i < L; ++i) { tr->us[i].max = word(); tr->smax[i] = word(); }
    tr->act_b.max = word();
    tr->lb_gmax = word();
    for (std::vector<LBlock>* v : {&tr->ldb, &tr->lub})
        for (LBlock& b : *v) {
            for (Act& a : b.a) a.max = word();
            for (int e = 0; e <= E; ++e) b.gmax.push_back(word());
        }
    if (k > tr->n_maxw) return tfail(tr, UMX_ERR_INVALID, "internal: %d max words for %d", k, tr->n_maxw);

    T_TRY(upload_convs(tr));
    return finish_build(tr, false);
}

int build_legacy(umx_trainer* tr, const float* blob, size_t blob_floats) {
    T_TRY(plan_legacy(tr, blob, blob_floats));
    return alloc_legacy(tr);
}

// forward of the legacy graph up to the logits.  training: batch statistics (moving averages updated when `update`) and the max
// words of every tensor a weight gradient reads; otherwise the moving statistics (tfTraining: 0)
int forward_legacy(umx_trainer* tr, const float* data, bool training, bool update) {
    const int L = tr->L, E = tr->E;
    hipStream_t st = tr->stream;
    int* const flagp = reinterpret_cast<int*>(tr->d_maxw + tr->n_maxw);
    // act(z) (pool: + the 2x2 max-pool) into out, with its max word and the planes it has (none on the exact-fp32 route)
    auto act = [&](const float* z, const float* stat, int pool, int a_kind, const Act& out) -> int {
        ActParams a;
        a.z = z; a.stat = stat;
        a.B = tr->B; a.H = a.W = pool ? 2 * out.S : out.S; a.C = out.C;
        a.pool = pool; a.act = a_kind;
        a.drop_rate = 0.f; a.drop_key = 0;
        T_HIP(tr, launch_act_fwd(a, out.x, training ? out.max : nullptr, out.h.hi, out.h.lo, out.h.Cs, flagp, st));
        return UMX_OK;
    };
    tr->ds[0].x = const_cast<float*>(data);
    T_TRY(track_act(tr, tr->ds[0], training));
    for (int i = 0; i < L; ++i) {
        LBlock& b = tr->ldb[i];
        BnSite& s = tr->bn_d[i];
        for (int e = 0; e <= E; ++e) {
            const bool last = e == E;   // (+ the shortcut on the block input)
            T_TRY(run_tconv(tr, b.fwd[e], e == 0 ? tr->ds[i] : b.a[e - 1], b.y[e], last ? &tr->ds[i] : nullptr, st));
            if (!last) T_TRY(act(b.y[e], b.ident, 0, ACT_RELU, b.a[e]));
        }
        T_TRY(act(b.y[E], b.ident, 0, ACT_RELU, Act{s.z, H16(), nullptr, nullptr, s.H, s.C}));      // relu(z): what BN normalises
        T_TRY(bn_forward_stats(tr, s, update, training));
        T_TRY(act(s.z, s.stat, 1, ACT_NONE, tr->ds[i + 1]));   // BN, then the pool
    }
    T_TRY(run_tconv(tr, tr->c_fwd_b, tr->ds[L], tr->lb_z, nullptr, st));
    T_TRY(act(tr->lb_z, tr->lb_ident, 0, ACT_RELU, tr->act_b));
    const Act* cur = &tr->act_b;
    for (int idx = L - 1; idx >= 0; --idx) {
        LBlock& b = tr->lub[idx];
        T_TRY(run_tconv(tr, tr->c_T[idx], *cur, tr->us[idx].x, nullptr, st));   // (ReLU fused)
        T_TRY(track_act(tr, tr->us[idx], training));
        for (int e = 0; e <= E; ++e) {
            if (e == 0) T_TRY(run_tconv(tr, tr->c_fwd_u[idx], tr->ds[idx], b.y[0], &tr->us[idx], st));
            else T_TRY(run_tconv(tr, b.fwd[e], b.a[e - 1], b.y[e], nullptr, st));
            T_TRY(act(b.y[e], b.ident, 0, ACT_RELU, b.a[e]));
        }
        cur = &b.a[E];
    }
    T_HIP(tr, launch_head_fwd(cur->x, cur->npix(tr->B), cur->C, tr->K, tr->d_w + tr->o_lt, tr->lt_z, st));
    return UMX_OK;
}

int enqueue_legacy(umx_trainer* tr, const float* data, const float* labels, const float* weights, bool update) {
    const int L = tr->L, K = tr->K, B = tr->B, P = tr->P, E = tr->E;
    const std::vector<int>& n = tr->n;
    hipStream_t st = tr->stream;
    const size_t Npix = (size_t)B * P * P;
    int* const flagp = reinterpret_cast<int*>(tr->d_maxw + tr->n_maxw);
    T_TRY(step_begin(tr, update));
    T_TRY(pack_all(tr, st, 2));
    T_TRY(forward_legacy(tr, data, true, update));
    T_TRY(loss_head(tr, tr->lt_z, tr->ident_k, labels, weights ? weights : tr->d_ones));
    if (tr->prof) T_HIP(tr, hipEventRecord(tr->ev[1], st));

    // ------------------------------------------------------------------ backward
    {   // top: d loss / d logits -> 1x1 conv
        const int nblk = chan_blocks(Npix, n[1]);
        T_HIP(tr, launch_head_bwd(tr->lub[0].a[E].x, tr->d_dt, tr->d_w + tr->o_lt, Npix, n[1], K, tr->DA, tr->d_part, nblk, st));
        T_HIP(tr, launch_reduce_partials(tr->d_part, nblk, n[1] * K, 1.0, tr->d_g + tr->o_lt, tr->d_w + tr->o_lt, 0, 0.f, st));
    }
    // A chain's gradients alternate between the slots dz[0] and dz[1].
    // gradient w.r.t. y (pre-ReLU, [B, S, S, C]) from the gradient w.r.t. relu(y): *g is slot pl's view of it, with its max word gw and planes
    auto relu_bwd = [&](const float* dy, const float* y, int pl, int S, int C, unsigned* gw, Act* g) -> int {
        *g = tr->dz[pl].view(S, C, gw);
        T_HIP(tr, launch_relu_bwd_max(dy, y, g->x, g->npix(B) * C, gw, st));
        return to_h16(tr, *g, st);
    };
    auto wgrad = [&](const WgradPlan& w, const Act& X, const Act& G, int Ctot, int c_off, size_t w_off) -> int {
        return run_wgrad(tr, w, X, G, Ctot, c_off, w_off, 0.f, SIZE_MAX, tr->d_ws, st);
    };
    // the extra convolutions of a chain, last first: *g is d/dy[E] (slot 0) on entry, d/dy[e] in slot (E - e) & 1 on the way, d/dy[0] on return
    auto extras_bwd = [&](LBlock& b, Act* g) -> int {
        for (int e = E; e >= 1; --e) {
            T_TRY(wgrad(b.wg[e], b.a[e - 1], *g, g->C, 0, b.o_wx[e - 1]));
            T_TRY(run_tconv(tr, b.dg[e], *g, tr->DA, nullptr, st));
            T_TRY(relu_bwd(tr->DA, b.y[e - 1], ((E - e) & 1) ^ 1, g->S, g->C, b.gmax[e - 1], g));
        }
        return UMX_OK;
    };
    Act g;
    for (int idx = 0; idx < L; ++idx) {    // up layers, output side first; DA: d loss / d (layer output)
        LBlock& b = tr->lub[idx];
        const int Cskip = n[idx], Cup = n[idx + 1], S = tr->us[idx].S;
        T_TRY(relu_bwd(tr->DA, b.y[E], 0, S, Cup, b.gmax[E], &g));
        T_TRY(extras_bwd(b, &g));
        T_TRY(wgrad(tr->wg_u0[idx], tr->ds[idx], g, Cskip + Cup, 0, tr->o_w2[idx]));
        T_TRY(wgrad(tr->wg_u1[idx], tr->us[idx], g, Cskip + Cup, Cskip, tr->o_w2[idx]));
        T_TRY(run_tconv(tr, tr->c_dg_us[idx], g, tr->DB, nullptr, st));
        if (idx >= 1) T_TRY(run_tconv(tr, tr->c_dg_skip[idx], g, tr->dskip[idx], nullptr, st));
        const Act gs = tr->gs[0].view(S / 2, 4 * Cup, tr->smax[idx]);
        T_HIP(tr, launch_leaky_bwd_s2d_max(tr->DB, tr->us[idx].x, B, S / 2, Cup, 0.f, gs.x, gs.max, st));   // ReLU: slope 0
        T_TRY(to_h16(tr, gs, st));
        // (the transposed convolution's filter: X is gS, G the layer's input)
        T_TRY(wgrad(tr->wg_T[idx], gs, idx == L - 1 ? tr->act_b : tr->lub[idx + 1].a[E], Cup, 0, tr->o_wt[idx]));
        T_TRY(run_tconv(tr, tr->c_dg_T[idx], gs, tr->DA, nullptr, st));
    }
    {   // bottom
        T_TRY(relu_bwd(tr->DA, tr->lb_z, 0, tr->act_b.S, n[L + 1], tr->lb_gmax, &g));
        T_TRY(wgrad(tr->wg_b, tr->ds[L], g, n[L], 0, tr->o_lb));
        T_TRY(run_tconv(tr, tr->c_dg_b, g, tr->DB, nullptr, st));
    }
    for (int i = L - 1; i >= 0; --i) {     // down layers; DB (+ dskip[i+1]): d loss / d ds[i+1]
        LBlock& b = tr->ldb[i];
        BnSite& s = tr->bn_d[i];
        const int Ci = n[i], C = n[i + 1];
        const size_t npix = (size_t)B * s.H * s.W;
        {   // pool -> BN backward on relu(z) (gamma / beta gradients in a fixed order) -> the ReLU mask
            float* const g0 = tr->dz[0].x;
            ActParams a = act_params(tr, s, 1, ACT_NONE, 0.f, 0);
            const int nblk = chan_blocks(npix / 4, C);
            T_HIP(tr, launch_act_bwd(a, tr->DB, i + 1 <= L - 1 ? tr->dskip[i + 1] : nullptr, g0, tr->d_part, nblk, nullptr, st));
            T_HIP(tr, launch_bn_bwd_finalize(tr->d_part, nblk, npix, C, tr->d_g + s.gamma, tr->d_g + s.beta, s.m12, st));
            T_HIP(tr, launch_bn_bwd_apply_max(g0, s.z, s.stat, s.m12, npix, C, nullptr, nullptr, nullptr, nullptr, nullptr, 0, flagp, st));
            T_TRY(relu_bwd(g0, b.y[E], 0, s.H, C, b.gmax[E], &g));
        }
        // the shortcut: weight gradient and (i >= 1) input gradient, before the chain reuses slot 0
        T_TRY(wgrad(b.wg_sh, tr->ds[i], g, Ci, 0, tr->o_ws[i]));
        if (i >= 1) T_TRY(run_tconv(tr, b.dg_sh, g, tr->DSUM + tr->max_act, nullptr, st));
        T_TRY(extras_bwd(b, &g));
        T_TRY(wgrad(tr->wg_d[i], tr->ds[i], g, Ci, 0, tr->o_w1[i]));
        if (i >= 1) {   // d ds[i] = first-conv input gradient + shortcut input gradient
            T_TRY(run_tconv(tr, tr->c_dg_d[i], g, tr->DSUM, nullptr, st));
            T_HIP(tr, launch_split_reduce(tr->DSUM, 2, tr->max_act, npix * Ci, ACT_NONE, tr->DB, st));
        }
    }
    return step_end(tr, update);
}

// what umx_trainer_create asks of the hyper-parameters and options, before it touches a device
int check_create(const umx_hparams* hp, const umx_train_options* opts) {
    const bool legacy = hp->graph == UMX_GRAPH_LEGACY;
    if (legacy) {
        if (hp->nExtraConvs < 0 || hp->nExtraConvs > 2)
            return tfail(nullptr, UMX_ERR_INVALID, "the training step covers the legacy graph with nExtraConvs 0..2");
        if (opts->reg_kind != UMX_REG_NONE || opts->drop_down_step != 0.f || opts->drop_bottom != 0.f || opts->drop_up0 != 0.f ||
            opts->drop_up_step != 0.f)
            return tfail(nullptr, UMX_ERR_INVALID, "the legacy graph has no dropout and no regulariser (umx_train_options_legacy)");
    } else if (hp->graph != UMX_GRAPH_V2 || hp->nExtraConvs != 0) {
        return tfail(nullptr, UMX_ERR_INVALID, "the training step covers the v2 graph with nExtraConvs == 0");
    }
    // one class: the softmax is identically 1, so the cross-entropy and every gradient of it are 0 -- nothing could be learnt
    if (hp->nClasses < 2 || hp->nClasses > 8) return tfail(nullptr, UMX_ERR_INVALID, "nClasses must be 2..8 (a one-class softmax has no gradient)");
    if (hp->nLayers < 1 || hp->nLayers > 8 || (hp->ks != 3 && hp->ks != 5) || hp->featMapsFact < 1 ||
        hp->nChannels < 1 || hp->nOut0 < 1)
        return tfail(nullptr, UMX_ERR_INVALID, "unsupported hyper-parameters");
    if ((hp->imSize & (hp->imSize - 1)) || (hp->imSize >> hp->nLayers) < 1)
        return tfail(nullptr, UMX_ERR_INVALID, "imSize must be a power of two, at least 2^nLayers");
    for (int i = 0; i < 8; ++i)
        if (opts->reserved[i]) return tfail(nullptr, UMX_ERR_INVALID, "umx_train_options.reserved must be zero");
    auto bad_rate = [](float r) { return !(r < 1.0f); };
    if (bad_rate(opts->drop_bottom) || bad_rate(opts->drop_up0) || bad_rate(opts->drop_down_step * hp->nLayers))
        return tfail(nullptr, UMX_ERR_INVALID, "dropout rates must be below 1");
    return UMX_OK;
}

// what the v2 step's schedule depends on (after the host pass)
StepEnv step_env(const umx_trainer* tr) {
    StepEnv env;
    env.L = tr->L; env.hconv = tr->hconv; env.wg_planes = tr->wg_planes; env.reg = tr->o.reg_kind != UMX_REG_NONE;
    for (int idx = 0; idx < tr->L; ++idx) { env.skip_split[idx] = tr->c_dg_skip[idx].plan.split; env.T_split[idx] = tr->c_dg_T[idx].plan.split; }
    return env;
}

// the test entries that run a graph's host pass alone: the trainer they plan (solo options, or the legacy graph's), on the route
// conv_f32 / no_ksplit select (UMX_TRAIN_CONV_F32 / UMX_TRAIN_NO_KSPLIT) ...
int plan_for_test(umx_trainer* tr, const char* who, const umx_hparams* hp, int B, int conv_f32, int no_ksplit, const float* blob,
                  size_t blob_floats, char* text, size_t cap, size_t* needed) {
    if (!hp || !blob || !needed || (!text && cap)) return umx::fail(nullptr, UMX_ERR_INVALID, "%s: null argument", who);
    *needed = 0;
    umx_train_options o;
    if (hp->graph == UMX_GRAPH_LEGACY) umx_train_options_legacy(&o); else umx_train_options_solo(&o);
    if (const int rc = check_create(hp, &o)) return umx::fail(nullptr, rc, "%s", g_terr.c_str());
    tr->hp = *hp;
    tr->o = o;
    tr->B = B > 0 ? B : 8;
    tr->legacy = hp->graph == UMX_GRAPH_LEGACY;
    tr->hconv = !conv_f32;
    tr->no_ksplit = no_ksplit != 0;
    const int rc = tr->legacy ? plan_legacy(tr, blob, blob_floats) : plan_trainer(tr, blob, blob_floats);
    return rc == UMX_OK ? UMX_OK : umx::fail(nullptr, rc, "%s", tr->err.c_str());
}

// ... and the text they return.  *needed: bytes of the text with its terminator; UMX_ERR_INVALID where cap is smaller.
int text_out(const char* who, const std::string& out, char* text, size_t cap, size_t* needed) {
    *needed = out.size() + 1;
    if (cap < *needed) return umx::fail(nullptr, UMX_ERR_INVALID, "%s: the text takes %zu bytes", who, *needed);
    memcpy(text, out.c_str(), *needed);
    return UMX_OK;
}

}  // namespace

// ---- the internal interface of umx_trainset.hip (umx_internal.h) ----
namespace umx {

TrainerIO trainer_io(umx_trainer* tr) {
    TrainerIO io;
    io.device = tr->device; io.B = tr->B; io.P = tr->P; io.C = tr->n[0]; io.K = tr->K;
    io.legacy = tr->legacy;
    io.stream = tr->stream;
    io.data = tr->ds[0].x; io.labels = tr->d_labels; io.weights = tr->d_weights; io.probs = tr->d_probs;
    return io;
}

int trainer_fail(umx_trainer* tr, int code, const char* msg) { return tfail(tr, code, "%s", msg); }

// umx_trainer_eval in three parts, so that umx_trainer_evaluate can assemble its batch on the device and keep the probabilities there.
// begin: the range flag is shared with the training steps: what is up now belongs to a step whose loss was not read yet -- remember
// it for umx_trainer_loss, so that the flag this pass raises (repack + split-precision forward) is this pass's own
int trainer_eval_begin(umx_trainer* tr) {
    T_HIP(tr, hipSetDevice(tr->device));
    T_TRY(fold_profile(tr));
    unsigned before = 0;
    T_HIP(tr, hipMemcpyAsync(&before, tr->d_maxw + tr->n_maxw, sizeof before, hipMemcpyDeviceToHost, tr->stream));
    T_HIP(tr, hipStreamSynchronize(tr->stream));
    if (before) {
        tr->range_pending = true;
        T_HIP(tr, hipMemsetAsync(tr->d_maxw + tr->n_maxw, 0, sizeof(unsigned), tr->stream));   // (in the order of the work that can raise the flag)
    }
    return UMX_OK;
}

// forward: the eval-mode pass (moving statistics, no dropout) on the batch in ds[0] -> softmax in d_probs
int trainer_eval_forward(umx_trainer* tr) {
    const size_t npx = (size_t)tr->B * tr->P * tr->P;
    float* own = tr->ds[0].x;
    T_TRY(pack_all(tr, tr->stream, 0));
    const int rc = tr->legacy ? forward_legacy(tr, own, false, false) : forward_pass(tr, own, false, false);
    tr->ds[0].x = own;
    T_TRY(rc);
    if (tr->legacy) T_HIP(tr, launch_softmax_only(tr->lt_z, tr->ident_k, npx, tr->K, tr->d_probs, tr->stream));
    else T_HIP(tr, launch_softmax_only(tr->bn_t.z, tr->bn_t.stat, npx, tr->K, tr->d_probs, tr->stream));
    return UMX_OK;
}

// end: wait for the pass and report the flag it raised
int trainer_eval_end(umx_trainer* tr) {
    unsigned flag = 0;
    T_HIP(tr, hipMemcpyAsync(&flag, tr->d_maxw + tr->n_maxw, sizeof flag, hipMemcpyDeviceToHost, tr->stream));
    T_HIP(tr, hipStreamSynchronize(tr->stream));
    if (flag) {
        T_HIP(tr, hipMemsetAsync(tr->d_maxw + tr->n_maxw, 0, sizeof(unsigned), tr->stream));   // (in the order of the work that can raise the flag)
        return tfail(tr, UMX_ERR_RANGE, "an operand of the split-precision forward pass of umx_trainer_eval left the binary16 range (|v| >= 6e4 or "
                                        "not finite): the probabilities are not valid; UMX_TRAIN_CONV_F32=1 selects the exact-fp32 kernels");
    }
    return UMX_OK;
}

int trainer_guard_check(umx_trainer* tr) {
    if (tr->mem.fill < 0) return UMX_OK;
    T_HIP(tr, hipSetDevice(tr->device));
    for (hipStream_t s : tr->streams)
        if (s) T_HIP(tr, hipStreamSynchronize(s));
    std::string msg;
    const int rc = arena_check(tr->mem, &msg);
    return rc == UMX_OK ? UMX_OK : tfail(tr, rc, "%s", msg.c_str());
}

}  // namespace umx

extern "C" {

void umx_train_options_solo(umx_train_options* o) {
    fill_common(o);
    o->lr0 = 5e-5f; o->decay_steps = 5000; o->decay_rate = 0.98f;          // UnMicst1-5.py:362-365
    o->reg_kind = UMX_REG_L1;                                               // :84,125,160,213
    o->reg_down = o->reg_bottom = o->reg_up = o->reg_top = 0.00008f;
    o->clip_eps = 1e-7f;                                                    // :369-370
    o->drop_bottom = 0.35f;                                                 // :139
}

void umx_train_options_duo(umx_train_options* o) {
    fill_common(o);
    o->lr0 = 0.00006f; o->decay_steps = 4000; o->decay_rate = 0.99f;       // UnMicst2.py:357-360
    o->reg_kind = UMX_REG_L2;                                               // :82,123,158,211
    o->reg_down = o->reg_bottom = 0.01f;
    o->reg_up = o->reg_top = 0.005f;
    o->clip_eps = 0.f;                                                      // :364-366 (no clip)
    o->drop_down_step = 0.05f; o->drop_bottom = 0.3f;                       // :114,137
    o->drop_up0 = 0.25f; o->drop_up_step = 0.05f;                           // :203
}

void umx_train_options_legacy(umx_train_options* o) {
    fill_common(o);
    o->optimizer = UMX_OPT_MOMENTUM;                                        // UnMicst.py:270-279
    o->lr0 = 0.01f; o->decay_steps = 1000; o->decay_rate = 0.95f;
    o->momentum = 0.9f;
    o->reg_kind = UMX_REG_NONE;                                             // :276 (unweighted, no clip, no regulariser)
}

const char* umx_trainer_last_error(const umx_trainer* tr) { return tr ? tr->err.c_str() : g_terr.c_str(); }

int umx_trainer_create(const umx_hparams* hp, const float* weight_blob, size_t blob_floats, const umx_train_options* opts,
                       umx_trainer** out) {
    if (!hp || !weight_blob || !opts || !out) return tfail(nullptr, UMX_ERR_INVALID, "null argument");
    *out = nullptr;
    T_TRY(check_create(hp, opts));
    const bool legacy = hp->graph == UMX_GRAPH_LEGACY;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return tfail(nullptr, UMX_ERR_NO_DEVICE, "no HIP device");
    if (opts->device_ordinal < 0 || opts->device_ordinal >= ndev)
        return tfail(nullptr, UMX_ERR_INVALID, "device ordinal %d out of range", opts->device_ordinal);
    umx_trainer* tr = new umx_trainer();
    tr->hp = *hp;
    tr->o = *opts;
    tr->device = opts->device_ordinal;
    tr->B = opts->batch > 0 ? opts->batch : 8;
    tr->legacy = legacy;
    int rc = UMX_OK;
    std::string why;
    if (arena_init(&tr->mem, &why) != UMX_OK) rc = tfail(tr, UMX_ERR_INVALID, "%s", why.c_str());
    if (rc == UMX_OK && hipSetDevice(tr->device) != hipSuccess) rc = tfail(tr, UMX_ERR_HIP, "hipSetDevice failed");
    if (rc == UMX_OK && hipStreamCreateWithFlags(&tr->stream, hipStreamNonBlocking) != hipSuccess)
        rc = tfail(tr, UMX_ERR_HIP, "hipStreamCreate failed");
    tr->streams[TS_MAIN] = tr->stream;
    select_route(tr);
    if (rc == UMX_OK) rc = legacy ? build_legacy(tr, weight_blob, blob_floats) : build_trainer(tr, weight_blob, blob_floats);
    if (rc == UMX_OK)
        for (int i = 0; i < 4; ++i)
            if (hipEventCreate(&tr->ev[i]) != hipSuccess) rc = tfail(tr, UMX_ERR_HIP, "hipEventCreate failed");
    if (rc == UMX_OK) {   // the side and aux streams, and (v2) the step's schedule with its events
        for (int k = TS_MAIN + 1; k < kStepStreams; ++k)
            if (hipStreamCreateWithFlags(&tr->streams[k], hipStreamNonBlocking) != hipSuccess) rc = tfail(tr, UMX_ERR_HIP, "hipStreamCreate failed");
        if (!legacy) tr->plan = step_plan(step_env(tr));
        tr->events.assign(tr->plan.nevents, nullptr);
        for (hipEvent_t& e : tr->events)
            if (rc == UMX_OK && hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess)
                rc = tfail(tr, UMX_ERR_HIP, "hipEventCreate failed");
    }
    if (rc != UMX_OK) {
        g_terr = tr->err;
        umx_trainer_destroy(tr);
        return rc;
    }
    if (tr->mem.fill >= 0)
        fprintf(stderr, "[umx train] UMX_DEBUG_GUARD=0x%02x: %zu trainer buffers between red zones\n", tr->mem.fill, tr->mem.blocks.size());
    *out = tr;
    return UMX_OK;
}

int umx_test_trainer_serial(umx_trainer* tr, int on) {
    if (!tr) return tfail(tr, UMX_ERR_INVALID, "null argument");
    tr->serial = on != 0;
    return UMX_OK;
}

// The host pass of umx_trainer_create alone (no device): one line per forward / input-gradient convolution, in build order -- its
// UMX_DEBUG_PLAN text, then its groups (as the master tensors see them), the fused activation, `direct`, the weight shift, the counts of pack descriptors and weight references, the K-split
// scratch and tconv_digest of everything upload_conv would send.  conv_f32 / no_ksplit: the routes UMX_TRAIN_CONV_F32 /
// UMX_TRAIN_NO_KSPLIT select.  *needed: bytes of the text with its terminator; UMX_ERR_INVALID where cap is smaller.
int umx_test_train_plan(const umx_hparams* hp, int B, int conv_f32, int no_ksplit, const float* blob, size_t blob_floats, char* text,
                        size_t cap, size_t* needed) {
    umx_trainer tr;
    if (const int rc = plan_for_test(&tr, "umx_test_train_plan", hp, B, conv_f32, no_ksplit, blob, blob_floats, text, cap, needed)) return rc;
    std::string out;
    for (const TConv* tc : planned_convs(&tr)) {
        const TConvPlan& p = tc->plan;
        std::string groups;
        size_t nrefs = 0;
        for (int g = 0; g < tc->spec.ngroups; ++g) {
            const GroupSpec& G = tc->spec.g[g];
            char gb[96];   // channels x taps @ channel offset in the master [taps][d2][d3], T: transposed, s: a second master summed in
            std::string taps;   // (per phase)
            for (int ph = 0; ph < tc->spec.nphase; ++ph) taps += (ph ? "/" : "") + std::to_string(G.taps[ph].off.size());
            snprintf(gb, sizeof gb, "%s%dx%s@%d/%dx%d%s%s", g ? "+" : "", G.C, taps.c_str(), G.c_off, G.d2, G.d3, G.transpose ? "T" : "",
                     G.w2_off != SIZE_MAX ? "s" : "");
            groups += gb;
        }
        for (int ph = 0; ph < 4; ++ph) nrefs += p.P.wrefs[ph].size();
        char buf[256];
        snprintf(buf, sizeof buf, "; groups %s, act %d, direct %d, wsh %d, packs %zu, refs %zu, scratch %zu, digest %016llx\n", groups.c_str(),
                 tc->spec.act, p.direct ? 1 : 0, p.wsh, p.packs.size(), nrefs, p.split_floats,
                 tconv_digest(p.cp, p.nt, p.hpix, p.packs.data(), p.packs.size(), p.split ? &p.P : nullptr));
        out += p.text + buf;
    }
    return text_out("umx_test_train_plan", out, text, cap, needed);
}

// The schedule of the v2 training step for these hyper-parameters on a route (conv_f32 / no_ksplit as above), with (reg) or without a
// regulariser: the host pass, then step_plan's lines (step_describe).  No device.
int umx_test_step_plan(const umx_hparams* hp, int B, int conv_f32, int no_ksplit, int reg, const float* blob, size_t blob_floats,
                       char* text, size_t cap, size_t* needed) {
    umx_trainer tr;
    if (const int rc = plan_for_test(&tr, "umx_test_step_plan", hp, B, conv_f32, no_ksplit, blob, blob_floats, text, cap, needed)) return rc;
    if (tr.legacy) return umx::fail(nullptr, UMX_ERR_INVALID, "umx_test_step_plan: the legacy step has no schedule (one stream, no events)");
    if (!reg) tr.o.reg_kind = UMX_REG_NONE;
    return text_out("umx_test_step_plan", step_describe(step_plan(step_env(&tr))), text, cap, needed);
}

int umx_trainer_init(umx_trainer* tr, const umx_init_options* init) {
    if (!tr || !init) return tfail(tr, UMX_ERR_INVALID, "null argument");
    if (!std::isfinite(init->std_dev0) || !(init->std_dev0 > 0.f))
        return tfail(tr, UMX_ERR_INVALID, "umx_init_options.std_dev0 must be finite and > 0, got %g", (double)init->std_dev0);
    for (int i = 0; i < 5; ++i)
        if (init->reserved[i]) return tfail(tr, UMX_ERR_INVALID, "umx_init_options.reserved must be zero");
    // one entry per tensor of unmicst_amd/model.py tensor_specs, in that order (t counts the BN tensors too)
    std::vector<InitSeg> tab;
    unsigned long long t = 0, pos = 0;
    for (const Seg& sg : tr->segs) {
        if (sg.off != pos) return tfail(tr, UMX_ERR_INVALID, "parameter segments are not contiguous at %s", sg.name.c_str());
        pos += sg.n;
        if (sg.last == 0) {   // gamma 1 | beta 0 | moving mean 0 | moving variance 1
            const unsigned long long C = sg.n / 4;
            for (int k = 0; k < 4; ++k) tab.push_back(InitSeg{sg.off + k * C, C, 0, 0.0, k == 0 || k == 3 ? INIT_ONE : INIT_ZERO, 0});
            t += 4;
            continue;
        }
        const bool first = sg.name.size() > 3 && sg.name.compare(sg.name.size() - 3, 3, ".w1") == 0;   // kernel1 / kernelD<i>
        const double fan_in = (double)(sg.n / (size_t)sg.last);
        const double sigma = tr->legacy || first ? (double)init->std_dev0 : std::sqrt(1.0 / fan_in) / UMX_INIT_TRUNC_STD;
        const unsigned long long key = mix64_host((init->seed ^ UMX_INIT_DOMAIN) + 0x9E3779B97F4A7C15ull * (t + 1));
        tab.push_back(InitSeg{sg.off, sg.n, key, sigma, INIT_FILTER, 0});
        t += 1;
    }
    if (pos != tr->nparams || tab.empty()) return tfail(tr, UMX_ERR_INVALID, "parameter segments cover %llu of %zu floats", pos, tr->nparams);
    T_HIP(tr, hipSetDevice(tr->device));
    T_TRY(fold_profile(tr));
    for (hipStream_t s : tr->streams)
        if (s) T_HIP(tr, hipStreamSynchronize(s));
    if (!tr->d_initsegs) {
        T_TRY(talloc(tr, &tr->d_initsegs, tab.size()));
        tr->cap_initsegs = (int)tab.size();
    }
    if ((int)tab.size() != tr->cap_initsegs) return tfail(tr, UMX_ERR_INVALID, "the initial state's table changed size");
    T_HIP(tr, hipMemcpy(tr->d_initsegs, tab.data(), tab.size() * sizeof(InitSeg), hipMemcpyHostToDevice));
    T_HIP(tr, launch_init_params(tr->d_initsegs, (int)tab.size(), tr->nparams, tr->d_w, tr->stream));
    T_HIP(tr, hipMemsetAsync(tr->d_g, 0, tr->nparams * sizeof(float), tr->stream));
    T_HIP(tr, hipMemsetAsync(tr->d_m, 0, tr->nparams * sizeof(float), tr->stream));
    T_HIP(tr, hipMemsetAsync(tr->d_v, 0, tr->nparams * sizeof(float), tr->stream));
    T_HIP(tr, hipMemsetAsync(tr->d_maxw + tr->n_maxw, 0, sizeof(unsigned), tr->stream));   // the range flag of the old variables
    tr->range_pending = false;
    tr->step = 0;
    // the derived copies: packed operands and weight images are rebuilt from the variables by every step; the scales they are stored
    // with were derived from the variables the trainer was created with
    T_TRY(refresh_wscales(tr));
    T_HIP(tr, hipStreamSynchronize(tr->stream));
    return umx::trainer_guard_check(tr);
}

void umx_trainer_destroy(umx_trainer* tr) {
    if (!tr) return;
    (void)hipSetDevice(tr->device);
    if (tr->stream) (void)hipStreamSynchronize(tr->stream);
    arena_free(&tr->mem);
    for (int i = 0; i < 4; ++i)
        if (tr->ev[i]) (void)hipEventDestroy(tr->ev[i]);
    for (int k = TS_MAIN + 1; k < kStepStreams; ++k)
        if (tr->streams[k]) { (void)hipStreamSynchronize(tr->streams[k]); (void)hipStreamDestroy(tr->streams[k]); }
    for (hipEvent_t e : tr->events)
        if (e) (void)hipEventDestroy(e);
    if (tr->stream) (void)hipStreamDestroy(tr->stream);
    delete tr;
}

int umx_train_step_dev(umx_trainer* tr, const float* data_dev, const float* labels_dev, const float* weights_dev,
                       int apply_update) {
    if (!tr || !data_dev || !labels_dev || (!weights_dev && !tr->legacy)) return tfail(tr, UMX_ERR_INVALID, "null argument");
    T_HIP(tr, hipSetDevice(tr->device));
    T_TRY(fold_profile(tr));
    float* own = tr->ds[0].x;
    const int rc = tr->legacy ? enqueue_legacy(tr, data_dev, labels_dev, weights_dev, apply_update != 0)
                              : enqueue_step(tr, data_dev, labels_dev, weights_dev, apply_update != 0);
    tr->ds[0].x = own;
    T_TRY(rc);
    return umx::trainer_guard_check(tr);
}

int umx_trainer_loss(umx_trainer* tr, double* loss3) {
    if (!tr || !loss3) return tfail(tr, UMX_ERR_INVALID, "null argument");
    T_HIP(tr, hipSetDevice(tr->device));
    double h[2] = {0, 0};
    unsigned flag = 0;
    T_HIP(tr, hipMemcpyAsync(h, tr->d_loss, sizeof h, hipMemcpyDeviceToHost, tr->stream));
    T_HIP(tr, hipMemcpyAsync(&flag, tr->d_maxw + tr->n_maxw, sizeof flag, hipMemcpyDeviceToHost, tr->stream));
    T_HIP(tr, hipStreamSynchronize(tr->stream));
    if (flag || tr->range_pending) {   // sticky: raised by any step since the last report; reported once, then cleared
        flag = 1;
        tr->range_pending = false;
        T_HIP(tr, hipMemsetAsync(tr->d_maxw + tr->n_maxw, 0, sizeof(unsigned), tr->stream));   // (in the order of the work that can raise the flag)
    }
    if (flag)
        return tfail(tr, UMX_ERR_RANGE, "an operand of a split-precision convolution or weight gradient left the binary16 range "
                                        "(|v| >= 6e4 after scaling or not finite): a diverging run, or a filter that outgrew its scale "
                                        "between two refreshes (UMX_TRAIN_WSCALE_EVERY); UMX_TRAIN_CONV_F32=1 / UMX_TRAIN_WGRAD_F32=1 "
                                        "select the exact-fp32 kernels");
    loss3[0] = h[0] + h[1];
    loss3[1] = h[0];
    loss3[2] = h[1];
    return UMX_OK;
}

int umx_train_step(umx_trainer* tr, const float* data, const float* labels, const float* weights, int apply_update,
                   double* loss3) {
    if (!tr || !data || !labels || (!weights && !tr->legacy)) return tfail(tr, UMX_ERR_INVALID, "null argument");
    T_HIP(tr, hipSetDevice(tr->device));
    const size_t npx = (size_t)tr->B * tr->P * tr->P;
    T_HIP(tr, hipMemcpyAsync(tr->ds[0].x, data, npx * tr->n[0] * sizeof(float), hipMemcpyHostToDevice, tr->stream));
    T_HIP(tr, hipMemcpyAsync(tr->d_labels, labels, npx * tr->K * sizeof(float), hipMemcpyHostToDevice, tr->stream));
    if (weights) T_HIP(tr, hipMemcpyAsync(tr->d_weights, weights, npx * tr->K * sizeof(float), hipMemcpyHostToDevice, tr->stream));
    T_TRY(umx_train_step_dev(tr, tr->ds[0].x, tr->d_labels, weights ? tr->d_weights : nullptr, apply_update));
    double l[3];
    T_TRY(umx_trainer_loss(tr, l));
    if (loss3) { loss3[0] = l[0]; loss3[1] = l[1]; loss3[2] = l[2]; }
    return UMX_OK;
}

int umx_trainer_eval(umx_trainer* tr, const float* data, float* probs_host) {
    if (!tr || !data || !probs_host) return tfail(tr, UMX_ERR_INVALID, "null argument");
    T_TRY(umx::trainer_eval_begin(tr));
    const size_t npx = (size_t)tr->B * tr->P * tr->P;
    T_HIP(tr, hipMemcpyAsync(tr->ds[0].x, data, npx * tr->n[0] * sizeof(float), hipMemcpyHostToDevice, tr->stream));
    T_TRY(umx::trainer_eval_forward(tr));
    T_HIP(tr, hipMemcpyAsync(probs_host, tr->d_probs, npx * tr->K * sizeof(float), hipMemcpyDeviceToHost, tr->stream));
    const int rc = umx::trainer_eval_end(tr);
    T_TRY(umx::trainer_guard_check(tr));   // (a damaged zone before a range report)
    return rc;
}

int umx_trainer_read(umx_trainer* tr, int which, float* out, size_t n_floats) {
    if (!tr || !out) return tfail(tr, UMX_ERR_INVALID, "null argument");
    if (n_floats != tr->nparams) return tfail(tr, UMX_ERR_INVALID, "vector has %zu floats, asked for %zu", tr->nparams, n_floats);
    const float* src = which == UMX_TV_PARAMS ? tr->d_w : which == UMX_TV_GRADS ? tr->d_g : which == UMX_TV_SLOT_M ? tr->d_m
                     : which == UMX_TV_SLOT_V ? tr->d_v : nullptr;
    if (!src) return tfail(tr, UMX_ERR_INVALID, "unknown vector %d", which);
    T_HIP(tr, hipSetDevice(tr->device));
    T_HIP(tr, hipStreamSynchronize(tr->stream));
    T_HIP(tr, hipMemcpy(out, src, n_floats * sizeof(float), hipMemcpyDeviceToHost));
    return UMX_OK;
}

int umx_trainer_read_tensor(umx_trainer* tr, const char* name, float* out, size_t* n_floats) {
    if (!tr || !name || !n_floats) return tfail(tr, UMX_ERR_INVALID, "null argument");
    const std::string nm(name);
    const size_t dot = nm.find('.');
    const std::string layer = nm.substr(0, dot), what = dot == std::string::npos ? "" : nm.substr(dot + 1);
    const float* src = nullptr;
    size_t n = 0;
    auto index_of = [&](const char* prefix, int count) -> int {   // "<prefix><i>" -> i, or -1
        const size_t pl = strlen(prefix);
        if (layer.compare(0, pl, prefix) != 0 || layer.size() == pl) return -1;
        for (size_t k = pl; k < layer.size(); ++k) if (layer[k] < '0' || layer[k] > '9') return -1;
        const int i = atoi(layer.c_str() + pl);
        return i < count ? i : -1;
    };
    const BnSite* site = nullptr;
    int i;
    // the legacy graph's decision sites: ld<i>.x<e> / lu<i>.x<e> (what extra conv e reads, pre-ReLU), ld<i>.z (main + shortcut) and
    // lu<i>.z / lb.z (pre-ReLU), ld<i>.stat (statistics of relu(z)), lt.z (logits); lu<i>.us and ds<i> as in v2
    if (tr->legacy && what.size() >= 2 && what[0] == 'x' && what.find_first_not_of("0123456789", 1) == std::string::npos) {
        const int e = atoi(what.c_str() + 1);
        const LBlock* b = (i = index_of("ld", tr->L)) >= 0 ? &tr->ldb[i] : (i = index_of("lu", tr->L)) >= 0 ? &tr->lub[i] : nullptr;
        if (b && e < tr->E) { src = b->y[e]; n = (size_t)tr->B * (tr->P >> i) * (tr->P >> i) * tr->n[i + 1]; }
    } else if (tr->legacy && what == "z" && (layer == "lb" || layer == "lt")) {
        const int S = layer == "lb" ? tr->P >> tr->L : tr->P;
        src = layer == "lb" ? tr->lb_z : tr->lt_z;
        n = (size_t)tr->B * S * S * (layer == "lb" ? tr->n[tr->L + 1] : tr->K);
    } else if (tr->legacy && what == "z" && ((i = index_of("ld", tr->L)) >= 0 || (i = index_of("lu", tr->L)) >= 0)) {
        src = (layer[1] == 'd' ? tr->ldb[i] : tr->lub[i]).y[tr->E];
        n = (size_t)tr->B * (tr->P >> i) * (tr->P >> i) * tr->n[i + 1];
    } else if (tr->legacy && what == "stat" && (i = index_of("ld", tr->L)) >= 0) {
        site = &tr->bn_d[i];
    } else if (tr->legacy) {
        // (us / ds below)
    } else if (layer == "lb") site = &tr->bn_b;
    else if (layer == "lt") site = &tr->bn_t;
    else if ((i = index_of("ld", tr->L)) >= 0) site = &tr->bn_d[i];
    else if ((i = index_of("lu", tr->L)) >= 0) site = &tr->bn_u[i];
    if (site && what == "z") { src = site->z; n = (size_t)tr->B * site->H * site->W * site->C; }
    else if (site && what == "stat") { src = site->stat; n = 4 * (size_t)site->C; }
    else {
        const Act* a = what == "us" && (i = index_of("lu", tr->L)) >= 0 ? &tr->us[i]
                       : what.empty() && (i = index_of("ds", tr->L + 1)) >= 0 ? &tr->ds[i] : nullptr;
        if (a) { src = a->x; n = a->npix(tr->B) * a->C; }
    }
    if (!src) return tfail(tr, UMX_ERR_INVALID, "unknown tensor %s", name);
    const size_t cap = *n_floats;
    *n_floats = n;
    if (!out) return UMX_OK;
    if (cap < n) return tfail(tr, UMX_ERR_INVALID, "%s has %zu floats, the buffer holds %zu", name, n, cap);
    T_HIP(tr, hipSetDevice(tr->device));
    T_HIP(tr, hipStreamSynchronize(tr->stream));
    T_HIP(tr, hipMemcpy(out, src, n * sizeof(float), hipMemcpyDeviceToHost));
    return UMX_OK;
}

int umx_trainer_probs(umx_trainer* tr, float* probs_host) {
    if (!tr || !probs_host) return tfail(tr, UMX_ERR_INVALID, "null argument");
    T_HIP(tr, hipSetDevice(tr->device));
    T_HIP(tr, hipStreamSynchronize(tr->stream));
    T_HIP(tr, hipMemcpy(probs_host, tr->d_probs, (size_t)tr->B * tr->P * tr->P * tr->K * sizeof(float), hipMemcpyDeviceToHost));
    return UMX_OK;
}

int64_t umx_trainer_step_count(const umx_trainer* tr) { return tr ? tr->step : -1; }
int umx_trainer_batch(const umx_trainer* tr) { return tr ? tr->B : 0; }
double umx_trainer_flops_per_image(const umx_trainer* tr) { return tr ? tr->flops_per_image : 0.0; }

int umx_trainer_profile(umx_trainer* tr, int enable, double* fwd_ms, double* bwd_ms, double* opt_ms, int* steps) {
    if (!tr) return tfail(tr, UMX_ERR_INVALID, "null argument");
    T_HIP(tr, hipSetDevice(tr->device));
    T_TRY(fold_profile(tr));
    if (fwd_ms) *fwd_ms = tr->t_fwd;
    if (bwd_ms) *bwd_ms = tr->t_bwd;
    if (opt_ms) *opt_ms = tr->t_opt;
    if (steps) *steps = tr->t_steps;
    tr->t_fwd = tr->t_bwd = tr->t_opt = 0.0;
    tr->t_steps = 0;
    tr->prof = enable != 0;
    return UMX_OK;
}

}  // extern "C"
