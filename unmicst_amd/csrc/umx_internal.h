// Internal host-side interface of libumx (gfx950 only): the graph / plan / context structures shared by the graph builder
// (umx_graph.hip), the split-precision planner (umx_plan.hip), the engine and C ABI (umx_engine.hip), the schedules of the
// whole-slide entries (umx_pipeline.hip) and their executors: the host pipeline (umx_host.hip) and the sharded one (umx_shard.hip).
// Nothing here is part of the C ABI (include/umx.h).
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <functional>
#include <map>
#include <memory>
#include <string>
#include <vector>

#include "../../include/umx.h"
#include "../../include/umx_train.h"
#include "umx_kernels.h"


namespace umx {

struct HostTensor {
    const float* p;
    int d0, d1, d2, d3;  // [kh,kw,a,b]
    float at(int i, int j, int a, int b) const { return p[(((size_t)i * d1 + j) * d2 + a) * d3 + b]; }
};

struct BN {
    const float *g, *b, *m, *v;
};

struct Group {           // one operand group of a launch, host description
    int src;             // buffer id
    int C;               // channels
    std::vector<std::pair<int, int>> taps[4];  // per phase: (dy, dx) input offsets
    std::vector<float> packed[4];              // per phase: [ntaps][Cp][Np]
    // (training) per phase, [tap][octet]: 1 = every weight of this (tap, 8 input channels) pair is a structural zero -- the input
    // gradient of a stride-2 transposed convolution on the space-to-depth tensor has 9 real (window position, parity block) pairs
    // of 16 -- and the planner leaves the pair out of the K loop.  Empty: none.
    std::vector<unsigned char> dead[4];
};

// Training (umx_train.hip): where one 16-byte unit of a packed weight image comes from.  The filters change every step, so the
// planner records, instead of values, for every (k-step, N-tile, lane) unit of a launch's weight slab the 8 source elements of the
// fp32 operand the trainer repacks on the device ([tap][Cp][Np], the layout Group::packed has on the host): element e of the unit =
// arr[base + e * stride] for e < nvalid, else 0.
struct HWRef {
    int dst;                   // uint4 index of the unit's hi image inside the (phase list's) slab; its lo image is 64 units on
    int base;                  // first source element
    unsigned short nvalid;     // 1..8 real input channels in the octet
    unsigned short arr;        // operand group the unit reads
};

struct Launch {
    std::string name;
    bool train = false;        // split-precision plan for the trainer: plain / per-phase kernels only, fp32 output, weights by reference
    bool head = false;
    int ngroups = 0;
    Group g[2];
    int nphase = 1, o_mul = 1;
    int oy_off[4] = {0, 0, 0, 0}, ox_off[4] = {0, 0, 0, 0};
    int H = 0, W = 0, Cout = 0;
    int dst = -1, outH = 0, outW = 0, pool = 0, act = 0;
    std::vector<float> pre_s, pre_b, post_s, post_b;  // size Cout or empty
    // split-precision plan only: this launch's epilogue also drops `app_C` (<= 2) channels of buffer `app_src` (same pixel grid as
    // its output) into the spare channels [app_c0, app_c0 + app_C) of its last stored octet -- the raw-input skip of the top
    // up-layer rides in the up-sampled tensor, so that layer's convolution reads ONE 5-octet tensor instead of 1 + 5 octets
    int app_src = -1, app_C = 0, app_c0 = 0;
    int bn = 0;               // where the BatchNorm affine sits: 0 none, 1 before the activation (pre_*), 2 after it (post_*)
    int summed_shortcut = 0;  // > 0: a same-source shortcut filter of this size is summed into the main filter (exact algebra)
    // head only
    std::vector<float> head_w;  // [C][K]
    int head_C = 0, head_K = 0;
    // derived
    int nt = 1, Np = 16, hpix = 2;
    double flops = 0.0;       // algorithmic FLOPs per tile (per image of the batch)
    double exec_flops = 0.0;  // executed incl. channel/N padding
    double bytes = 0.0;       // compulsory HBM bytes per tile: sources + destination (weights excluded)
    // device
    ConvParams cp;
    // split-precision plan (UMX_PREC_F16X3)
    HConvParams hcp;
    FirstParams first;        // dense-K plan of the first down-sampling layer (use_first; umx_conv_first.hip)
    bool use_first = false;
    // depth-to-space form of a stride-2 transposed convolution (make_d2s): nphase = number of N-blocks, each a plain convolution
    // over the union of its phases' taps with the N axis [phase slot][full octets] (+ one remainder tile of <= 4 channels per phase)
    int d2s = 0;              // 1: rewritten
    int d2s_Cout = 0;         // the real output channels (Cout holds the N extent of one block)
    int d2s_F = 0, d2s_R = 0; // full octets / remainder channels per phase
    int d2s_npb = 0;          // phases per block (4 or 2)
    int d2s_oy[2][4] = {{0, 0, 0, 0}, {0, 0, 0, 0}}, d2s_ox[2][4] = {{0, 0, 0, 0}, {0, 0, 0, 0}};   // sub-pixel offset of (block, phase slot)
    unsigned char d2s_tapmask[2][16] = {{0}, {0}};   // per block and tap of its window: bit j set = phase slot j has that tap
    int nt16 = 1;             // N-tiles per workgroup of the split-precision kernel
    std::string kernel;       // ... and its instantiation's name in a profile (HostPlan::kernel)
    float* d_head_w = nullptr;
    float *d_pre_s = nullptr, *d_pre_b = nullptr, *d_post_s = nullptr, *d_post_b = nullptr;
};

struct Buffer {
    size_t floats_per_tile = 0;
    int S = 0, C = 0;        // spatial size and real channels of the tensor
    int Cs = 0;              // stored channels of the (hi, lo) binary16 form
    bool as_f32 = true;      // fp32 NHWC (f32 path, and the head's input in the f16 path) or (hi, lo) binary16 planes
    bool planar = false;     // (hi, lo) planes stored per image as [octet][pixel][8] instead of NHWC (tensors of >= 16 x 16 pixels)
    float* d = nullptr;
};

struct ProfSite {
    std::string name, kernel;
    int64_t launches = 0, seen = 0;
    double total_ms = 0.0, flops = 0.0, bytes = 0.0, exec = 0.0;
    int xcd_order = 0;   // of the site's last launch (conv_f16x3 only)
};

struct PendingEvent {
    int site;
    hipEvent_t a, b;
};

// ---- device memory of a trainer / training set / labeler / inference context (umx_arena.hip) ----
// Every allocation goes through arena_alloc.  Debug guard mode (UMX_DEBUG_GUARD=<byte>, read at umx_trainer_create /
// umx_trainset_create / umx_create_opts) puts a red zone of max(64 KiB, round_up(bytes, 4 KiB)) in front of and behind each buffer,
// fills both zones -- and the buffer itself unless the caller zeroes or uploads it -- with that byte, and arena_check names the first
// buffer whose zones changed.  Off (the default), an allocation is the plain hipMalloc it always was.
struct DevBlock {
    void* base;                        // what hipMalloc returned
    size_t front, bytes, back;         // the buffer is [base + front, base + front + bytes)
    std::string label;
    bool scoped;                       // call-scoped (arena_refill poisons it again), not resident
};
struct DevArena {
    int fill = -1;                     // guard mode: the fill byte 0..255; -1 off
    size_t serial = 0;                 // (guard mode) allocations so far: the "#n" of a label
    std::vector<void*> allocs;         // what hipFree takes
    std::vector<DevBlock> blocks;      // (guard mode) one per live allocation, in allocation order
};
// UMX_DEBUG_GUARD -> a->fill; UMX_ERR_INVALID (with *why) for a value that is not a byte
int arena_init(DevArena* a, std::string* why);
// bytes (at least 16) of device memory -> *out; zero: cleared, else uninitialised (guard mode: filled).  scoped: the buffer holds
// nothing from one call to the next (the inference context's activations and per-call scratch)
hipError_t arena_alloc(DevArena* a, void** out, size_t bytes, bool zero, const char* label, bool scoped = false);
// frees the one allocation arena_alloc returned as p (its zones are not checked); the work that uses it must be done
hipError_t arena_release(DevArena* a, void* p);
// guard mode only: every scoped buffer filled again, in the order of `stream` (which the call then waits for)
hipError_t arena_refill(const DevArena& a, hipStream_t stream);
// guard mode only, with every stream writing the arena idle: UMX_OK, or UMX_ERR_GUARD with the first damaged zone in *msg
int arena_check(const DevArena& a, std::string* msg);
void arena_free(DevArena* a);

struct Shard;   // umx_shard.hip: the communicator, transport and buffers umx_shard_init attaches to a context

}  // namespace umx

struct umx_ctx {
    using Launch = umx::Launch;
    using Buffer = umx::Buffer;
    using ProfSite = umx::ProfSite;
    using PendingEvent = umx::PendingEvent;
    umx_hparams hp;
    int device = 0;
    int max_batch = 0;
    hipStream_t own_stream = nullptr, stream = nullptr;
    std::vector<Launch> plan;
    std::vector<Buffer> bufs;   // bufs[0] = input tiles
    // Second "lane": the tile batches of one band alternate between two activation-buffer sets on two streams, so that
    // the kernels of batch i+1 fill the CUs the tail of batch i's current layer leaves idle and MFMA-bound layers of one
    // batch share a CU with the load-bound full-resolution layers of the other.
    std::vector<Buffer> bufs2;
    hipStream_t stream2 = nullptr;
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    float* d_tiles32_2 = nullptr;
    int nlanes = 1;
    int ncu = 256;
    // host entry points: uploads / downloads on their own streams, slab by slab, under the tile kernels
    hipStream_t up_stream = nullptr, dn_stream = nullptr;
    struct HostSlot {   // device buffers + events of one in-flight host call (two slots: slide i+1 uploads while slide i computes)
        double* d_image = nullptr;  size_t image_cap = 0;
        float* d_probs = nullptr;   size_t probs_cap = 0;
        void* d_out = nullptr;      size_t out_cap = 0;
        std::vector<hipEvent_t> events;
        hipEvent_t done = nullptr;
        int* flag_host = nullptr;   // pinned copy of the range flag, read back behind the slot's last download
        bool busy = false;
    } hs[2];
    umx::DevArena mem;          // every device buffer of the context (UMX_DEBUG_GUARD: with red zones, the call-scoped ones poisoned)
    int guard_depth = 0;        // (guard mode) public entries on the stack: the outermost one refills and checks
    std::string err;
    // whole-image scratch (grown on demand)
    double* d_image = nullptr;  size_t image_cap = 0;
    float* d_probs = nullptr;   size_t probs_cap = 0;
    void* d_out = nullptr;      size_t out_cap = 0;
    float* d_io_tiles = nullptr; size_t io_tiles_cap = 0;
    float* d_io_probs = nullptr; size_t io_probs_cap = 0;
    // profiling
    int prof = 0;               // 0 off, 1 every launch, N >= 2 every N-th launch of a site bracketed by events
    std::vector<ProfSite> sites;
    std::vector<PendingEvent> pending;
    std::vector<hipEvent_t> free_events;
    int site_gather = -1, site_stitch = -1, site_split = -1;
    // precision
    int precision = UMX_PREC_F16X3;
    bool f6 = false;            // split precision with the cross terms of the deep layers on the block-scaled fp6 matrix instruction (UMX_PREC_F16X3_F6)
    bool f6_used = false;       // ... and at least one layer of this model runs in that form (what umx_precision_of reports)
    int act_shift = 0;          // activations are stored times 2^act_shift in the (hi, lo) binary16 form
    float* d_tiles32 = nullptr; // fp32 staging of gathered tiles before the split (f16 path)
    int* d_flag = nullptr;      // binary16 range overflow flags (64 words): word 0 for the synchronous entry points, words 16 and
                                // 32 for the two slots of the submit / wait API -- a flag is cleared and read in stream order by
                                // the call that owns it, never from the host while another call is in flight
    int flag_word = 0;          // the word the launches being enqueued report to
    int in_cw = 0;              // > 0: the input tiles (buffer 0) are stored in the compact form [pixel]{hi[in_cw] | lo[in_cw]} -- their
                                // only readers are the dense-K first layer and the raw-skip append of the top transposed convolution
    uint4* d_zeros = nullptr;
    bool head_fused = false;
    std::string stamps;         // UMX_DEBUG_STAMPS as umx_create_opts read it: the layer whose launches run the stamped kernel
    umx::Shard* shard = nullptr;   // set by umx_shard_init / umx_shard_init_transport once it has fully succeeded
};

namespace umx {

extern thread_local std::string g_err;

// One lane of a context: the activation buffers, stream and fp32 tile staging a tile batch runs on (umx_ctx: lane 0 = bufs, stream,
// d_tiles32; lane 1 = bufs2, stream2, d_tiles32_2).  A value handed down the launch path, never kept.
struct Lane {
    std::vector<Buffer>* bufs;
    hipStream_t stream;
    float* tiles32;
};
inline Lane lane_of(umx_ctx* ctx, int i) {
    return i ? Lane{&ctx->bufs2, ctx->stream2, ctx->d_tiles32_2} : Lane{&ctx->bufs, ctx->stream, ctx->d_tiles32};
}

int fail(umx_ctx* ctx, int code, const char* fmt, ...);

#define HIP_TRY(ctx, expr)                                                                                  \
    do {                                                                                                    \
        hipError_t e__ = (expr);                                                                            \
        if (e__ != hipSuccess)                                                                              \
            return fail(ctx, e__ == hipErrorOutOfMemory ? UMX_ERR_OOM : UMX_ERR_HIP, "%s failed: %s", #expr, \
                        hipGetErrorString(e__));                                                            \
    } while (0)


inline int round_up(int a, int b) { return (a + b - 1) / b * b; }

// ---- umx_graph.hip: hyper-parameters -> launch list (reference UnMicst1-5.py:55-237, UnMicst.py:51-187)
int check_hp(const umx_hparams* hp, std::string* why);
std::vector<int> widths(const umx_hparams& hp);
size_t blob_floats_needed(const umx_hparams& hp);
// builds the launch list and the activation-buffer list (per-tile floats, (spatial size, channels)); blob may be NULL
// (describe only); *pos = floats of the blob consumed
int build_graph(const umx_hparams& hp, const float* blob, std::vector<Launch>* plan, std::vector<size_t>* buf_floats,
                std::vector<std::pair<int, int>>* buf_geom, size_t* pos, bool fold_top_skip = false);
bool conv_geometry(Launch& L, std::string* why);

// ---- umx_plan.hip: split-precision plan of one launch and of a model, on the host (no context, no HIP call, no getenv)
int mx_pack_e2m3(const double (&v)[32], double amax, unsigned char (&out)[24]);   // umx_plan.hip: one OCP MX fp6 (e2m3) block of 32
// The planner's tuning and debug switches as a value.  plan_switches_from_env is the one place that reads them from the environment;
// its callers are umx_create_opts, umx_plan_check and the trainer's select_route.  Default-constructed: no switch.
struct PlanSwitches {
    bool have_nt = false;          // UMX_PLAN_NT is set (even malformed: the narrower-N-tile trial is then off) ...
    std::string nt_layer;          // ... "layer:NT" forces that layer's N-tiles per workgroup
    int nt = 0;
    struct Override { std::string item, layer; int oc, s, mp; };   // one well-formed "layer:OC:S[:pieces]" entry (mp 0: no fourth field)
    bool have_override = false;    // UMX_PLAN_OVERRIDE is set ...
    std::vector<Override> overrides;   // ... its entries in order
    int threads = 0;               // UMX_PLAN_THREADS: host threads of the weight fill (0: by the size of the images)
    bool debug_plan = false;       // UMX_DEBUG_PLAN: the caller prints every plan's line (plan_describe) on stderr
    bool have_stamps = false;      // UMX_DEBUG_STAMPS is set (no layer takes the packed or fp6 form: the stamped kernels have neither) ...
    std::string stamps;            // ... to this layer's name
};
// (a null string: the variable is not set)
PlanSwitches plan_switches_parse(const char* nt, const char* override_list, const char* threads, bool debug_plan, const char* stamps);
PlanSwitches plan_switches_from_env();
struct PlanInputs {                // what the plan of a launch depends on besides the launch
    bool f6 = false;               // the model may take the F6 form (UMX_PREC_F16X3_F6)
    int imSize = 0, act_shift = 0; // the model's tile size; activations are stored times 2^act_shift
    bool out_f32 = false;          // the launch writes fp32 (the head's input; every trainer launch)
    bool dst_planar = false;       // the destination buffer is octet-planar (the depth-to-space table)
    const Launch* head = nullptr;  // the softmax head its epilogue may fuse
    PlanSwitches sw;
};
struct HostPlan {
    HConvParams h;                      // device pointers null: the engine's upload_plan / the trainer's upload_conv set them
    int S = 0, slots = 1;               // the chosen k-steps per stage and halo slots (the octets per chunk are h.OC)
    std::string kernel;                 // the instantiation the launch runs under, as rocprofv3 names it: conv_f16x3<NT, KMT, NPH, DBG,
                                        // MAXP, PK, D2S, F6, W2> (W2 == F6 always) or, with use_first, conv_first<NT, CW, NKS, DBG>
    std::vector<HStage> stages;         // the stage table, every list's stages and a dummy behind them
    std::vector<_Float16> wimg[4];      // per stage list: weight slab [N-block][stage blocks] (training plans: k-maps only)
    std::vector<float> econst;          // epilogue constants per N-block (+ depth-to-space table, fused-head constants)
    std::vector<_Float16> head_frag;    // the fused head's MFMA A-fragments, or empty
    std::vector<HWRef> wrefs[4];        // (train) per stage list
    int nt16 = 1, wshift = 0;           // N-tiles per workgroup; weights are stored times 2^wshift
    int n_ksteps = 0;                   // K-slots of 32 executed per output tile, all phases ...
    double exec_flops = 0.0;            // ... and the executed-FLOP figure
    bool use_first = false;             // plan_first: the dense-K kernel takes the layer, with these parameters (pointers null) ...
    FirstParams first;
    std::vector<_Float16> first_w;      // ... and weight image
};
// UMX_ERR_INVALID with the reason in *why where the split-precision kernel cannot take the launch
int plan_f16(const Launch& L, const PlanInputs& in, HostPlan* P, std::string* why);
// dense-K plan of the first down-sampling layer, for a launch plan_f16 has just planned (sets P->use_first when it applies)
void plan_first(const Launch& L, HostPlan* P);
// depth-to-space rewrite of a narrow stride-2 transposed convolution (before conv_geometry / plan_f16); true if L was rewritten
bool make_d2s(Launch& L);
// the same decision from the hyper-parameters alone (the graph builder folds the raw skip only when the first layer takes this kernel)
bool conv_first_eligible(const umx_hparams& hp);
// the plan's line(s) of UMX_DEBUG_PLAN, each "[umx plan] ...\n" (a dense-K first layer: a second line)
std::string plan_describe(const Launch& L, const HostPlan& P);
// the host half of an upload: what the launch path reads of a plan besides the device parameters (nt16, exec_flops, use_first, kernel)
void adopt_plan(Launch& L, const HostPlan& P);
// A model planned on the host: the graph, the layout of each activation buffer (which depends on the graph alone) and, for the
// split-precision engine (f16), the host plan of every launch.  UMX_ERR_INVALID with "<layer>: <reason>" in *why for a refused layer.
struct ModelPlan {
    std::vector<Launch> plan;
    std::vector<Buffer> bufs;           // no device memory yet
    std::vector<HostPlan> hplans;       // per launch (f16; nothing for the head)
    size_t pos = 0;                     // blob floats the graph consumed
};
int plan_model(const umx_hparams& hp, const float* blob, bool f16, bool f6, int act_shift, const PlanSwitches& sw, ModelPlan* m,
               std::string* why);
// the workgroup order of one launch of an adopted plan on a batch of n tiles (the batch decides: run_launch_f16 asks per launch)
struct LaunchShape { int xcd_order, ntiles_grid, tiles_per_xcd; };
LaunchShape launch_shape(const Launch& L, const HConvParams& p, int n);
// 64-bit FNV-1a, and the serialisation of a host plan both digests share (documented in umx_tconv.hip)
struct Fnv {
    unsigned long long v = 0xcbf29ce484222325ull;
    void bytes(const void* p, size_t n) {
        const unsigned char* b = static_cast<const unsigned char*>(p);
        for (size_t i = 0; i < n; ++i) v = (v ^ b[i]) * 0x100000001b3ull;
    }
    void i(long long x) {
        unsigned char b[8];
        for (int k = 0; k < 8; ++k) b[k] = (unsigned char)((unsigned long long)x >> (8 * k));
        bytes(b, 8);
    }
    void f(float x) { bytes(&x, 4); }
    template <typename... T> void is(T... xs) { (i((long long)xs), ...); }
};
void digest_host_plan(Fnv& d, const HostPlan& P);
unsigned long long infer_digest(const HostPlan& P);   // everything upload_plan sends for one inference launch

// ---- umx_tconv.hip: the host plan of one forward / input-gradient convolution of the training step (no HIP call, no trainer, no getenv)
struct TapSet {
    std::vector<std::pair<int, int>> off;   // (dy, dx) input offsets
    std::vector<int> m;                     // master tap index per (tap, parity) : size off.size() * npar
};
// One operand group of a training convolution: a source of C channels and, per phase, a TapSet over the master tensor at w_off;
// transpose flag, channel offset on the master's d2 axis, (npar, Cblk) parity blocks, optional second tensor summed in
struct GroupSpec {
    int C;                      // source channels seen by the kernel
    size_t w_off, w2_off;       // master tensor(s) in the parameter vector (w2_off = SIZE_MAX: none)
    int d2, d3;                 // master dims [taps][d2][d3]
    int transpose, c_off, npar, Cblk;
    TapSet taps[4];
};
TapSet same_taps(int ks, bool flipped);
GroupSpec one_group(int C, size_t w_off, size_t w2_off, int d2, int d3, int transpose, int c_off, const TapSet& ts);
// the stride-2 transposed convolution: the four sub-pixel phases of its forward (taps of g, output offsets oy / ox [4]) ...
void transposed_fwd_taps(int ks, GroupSpec* g, int* oy, int* ox);
// ... and its backward on the space-to-depth output gradient: the 2 x 2 (ks 3) window and parity table of g, and the weight
// gradient's slabs with their channel offsets
void transposed_bwd_taps(int ks, int Cup, GroupSpec* g, TapSet* slabs, std::vector<int>* coff);
void choose_nt(int Cout, int mtiles, int* nt, int* Np);
struct WSrc { size_t off, off2, cnt; };   // master tensor(s) an operand group reads: where its weight scale is derived from
double operand_wmax(const std::vector<WSrc>& wsrc, const float* params);
int wscale_shift(double wmax);

struct TConvSpec {                     // one convolution as the graph's build describes it
    std::string name;
    int H = 0, W = 0, Cout = 0, act = 0, nphase = 1, o_mul = 1;
    int oy[4] = {0, 0, 0, 0}, ox[4] = {0, 0, 0, 0};
    int ngroups = 0;
    GroupSpec g[2];
    bool bwd = false;                  // it belongs to the backward pass only (its operands are packed on the side stream under the forward pass)
};
struct TConvEnv {                      // what its plan depends on besides
    int B = 0, imSize = 0;
    bool hconv = true;                 // the route: split precision (conv_f16x3) where the planner takes the shape, else the fp32 kernel
    bool no_ksplit = false;            // UMX_TRAIN_NO_KSPLIT
    const float* params = nullptr;     // the parameter vector on the host: weight scales
    PlanSwitches sw;                   // the planner's switches as select_route read them (umx_test_train_plan: none)
};
struct TConvPlan {
    ConvParams cp;                     // the fp32 kernel's launch (pointers null)
    int nt = 1, hpix = 2;
    double mac = 0.0;                  // algorithmic multiply-accumulates per image
    struct Operand { int ph, g; size_t elems; };
    std::vector<Operand> operands;     // the fp32 operands [tap][Cp][Np], one per (phase, group) with taps
    std::vector<PackDesc> packs;       // their descriptors (pointers null), index for index -- none for a direct convolution
    size_t max_pack = 0;
    bool split = false;                // the split-precision planner took it: P, direct, wsrc and wsh hold
    std::string refused;               // ... or why not
    HostPlan P;                        // references already in the coordinates the repack reads; ks0 / split_stride set
    bool direct = false;               // its weight images are gathered straight from the master tensors (no fp32 operand is read)
    std::vector<WSrc> wsrc;
    int wsh = 0;                       // the weights are stored times 2^wsh
    size_t split_floats = 0;           // K-split scratch either kernel needs
    std::string text;                  // tconv_describe
};
// false with *why ("<name>: <reason>") for a shape the trainer cannot run
bool tconv_plan(const TConvSpec& s, const TConvEnv& env, TConvPlan* out, std::string* why);
std::string tconv_describe(const TConvSpec& s, const TConvEnv& env, const TConvPlan& p);   // the plan's line of UMX_DEBUG_PLAN
// FNV-1a over everything the upload sends (serialisation: umx_tconv.hip); P null: the convolution stays on the fp32 kernel
unsigned long long tconv_digest(const ConvParams& cp, int nt, int hpix, const PackDesc* packs, size_t npacks, const HostPlan* P);

// ---- umx_tstep.hip: the stream schedule of the v2 training step as data (no HIP call, no trainer, no getenv)
constexpr int kSlots = 4;          // dz / gS buffers the main stream may run ahead of the weight gradients by
constexpr int kMaxLayers = 8;      // (check_create)
enum TOp {                         // what a step enqueues (enqueue_step's dispatch; T_JOIN: nothing, only its record)
    T_BEGIN, T_PACK0, T_PACK1, T_REG, T_FWD, T_LOSS, T_MARK, T_HEAD, T_DZ, T_WG_U0, T_WG_U1, T_WG_T, T_WG_B, T_WG_D,
    T_CV_US, T_CV_SKIP, T_CV_T, T_CV_B, T_CV_D, T_S2D, T_GSP, T_JOIN, T_OPT, T_NOPS
};
enum TStream { TS_MAIN, TS_SIDE0, TS_SIDE1, TS_AUX, kStepStreams };
// A BN site of the step, in the order the backward pass visits them: up layer idx, the bottom, down layer i, and the top (1x1 head)
inline int site_up(int idx) { return idx; }
inline int site_bottom(int L) { return L; }
inline int site_down(int L, int i) { return 2 * L - i; }
inline int site_top(int L) { return 2 * L + 1; }
// A buffer id: kind * 32 + index (layer, site or slot; 0 where the kind has one buffer)
enum TBufKind {
    TB_DS, TB_US, TB_CV, TB_ACTB, TB_Z, TB_STAT, TB_M12, TB_DA, TB_DB, TB_DT, TB_DSKIP, TB_DZ, TB_GS, TB_PART, TB_PART2, TB_WS, TB_WS2,
    TB_SPLIT, TB_SPLIT2, TB_SPLIT3, TB_FPACK, TB_BPACK, TB_LOSS0, TB_LOSS1,
    TB_G_LT, TB_G_W2, TB_G_WT, TB_G_LB, TB_G_WD, TB_G_BN,   // gradient segments: lt.w, lu<idx>.w2, lu<idx>.wt, lb.w, ld<i>.wshort + .w1, a site's gamma / beta
    TB_NKINDS
};
inline int tbuf(int kind, int index = 0) { return kind * 32 + index; }
// Event ids: begin, packed, join0 / join1, then per slot dz, gs, side, aux, then skip<idx> per up layer
enum { TE_BEGIN = 0, TE_PACKED = 1, TE_JOIN = 2, TE_DZ = 4, TE_GS = TE_DZ + kSlots, TE_SIDE = TE_GS + kSlots, TE_AUX = TE_SIDE + kSlots,
       TE_SKIP = TE_AUX + kSlots };
struct TStep {
    unsigned char op, site, stream;          // site: of T_HEAD / T_DZ / T_WG_* / T_CV_* / T_S2D / T_GSP, else 0
    unsigned char nwait, nrec, nr, nw;
    unsigned char wait[3], rec[2];           // event ids: waited on by `stream` before the step, recorded on it after
    unsigned short r0, w0;                   // its reads are StepPlan::bufs[r0, r0 + nr), its writes bufs[w0, w0 + nw)
};
struct StepPlan {
    std::vector<TStep> steps;                // in host enqueue order
    std::vector<unsigned short> bufs;
    int L = 0, nevents = 0;
    int rd(const TStep& s, int k) const { return bufs[s.r0 + k]; }
    int wr(const TStep& s, int k) const { return bufs[s.w0 + k]; }
};
struct StepEnv {                             // what the schedule depends on
    int L = 0;
    bool hconv = true, wg_planes = true, reg = false;
    bool skip_split[kMaxLayers] = {}, T_split[kMaxLayers] = {};   // c_dg_skip[idx] / c_dg_T[idx] took the split-precision route
};
StepPlan step_plan(const StepEnv& env);
std::string step_describe(const StepPlan& p);   // one line per step: "op site stream; wait e..; record e..; r buf..; w buf.."

// ---- umx_engine.hip
// Device memory of a context: ctx->mem (DevArena above).  Resident buffers -- weights, epilogue constants, stage lists, head
// fragments, the zero line and the range flags -- are uploaded or cleared at create and never refilled; everything else is
// call-scoped (`scoped`): in guard mode it is poisoned at allocation and again at the start of every public entry that enqueues work.
// `label` names the buffer in a guard error.
int dev_alloc(umx_ctx* ctx, void** out, size_t bytes, const std::string& label, bool scoped);
template <typename T>
int upload_raw(umx_ctx* ctx, const std::vector<T>& h, T** out, const std::string& label) {
    *out = nullptr;
    if (h.empty()) return UMX_OK;
    void* d = nullptr;
    int rc = dev_alloc(ctx, &d, h.size() * sizeof(T), label, false);
    if (rc) return rc;
    HIP_TRY(ctx, hipMemcpy(d, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice));
    *out = (T*)d;
    return UMX_OK;
}

// a (call-scoped) buffer is freed to grow once the context's stream -- or, for one other streams read, the whole device
// (device_wide) -- is idle
int grow(umx_ctx* ctx, void** buf, size_t* cap, size_t bytes, const char* label, bool device_wide = false);
// Guard mode (ctx->mem.fill >= 0) around the body of a public entry; off, guarded() is body().  The outermost entry on the stack,
// if it enqueues work (refill), waits for every stream of the context and poisons the call-scoped buffers before the body's first
// copy or launch; after a body that succeeded -- check: not a submit, whose umx_infer_image_wait does it -- it waits for
// the streams again and checks every red zone (UMX_ERR_GUARD).  Nothing inside the body changes: same launches, streams and events.
int guard_begin(umx_ctx* ctx, bool refill);
int guard_end(umx_ctx* ctx, int rc, bool check);
template <class F>
int guarded(umx_ctx* ctx, bool refill, bool check, F&& body) {
    if (!ctx || ctx->mem.fill < 0) return body();
    if (const int rc = guard_begin(ctx, refill)) return rc;
    return guard_end(ctx, body(), check);
}
int site_of(umx_ctx* ctx, const std::string& name, const std::string& kernel);
int prof_fold(umx_ctx* ctx);
struct ProfScope {
    umx_ctx* ctx;
    hipStream_t stream;
    int site;
    hipEvent_t a = nullptr, b = nullptr;
    bool on;
    ProfScope(umx_ctx* c, hipStream_t st, int s, double flops, double bytes, double exec = 0.0) : ctx(c), stream(st), site(s), on(c->prof && s >= 0) {
        if (!on) return;
        const int64_t k = ctx->sites[site].seen++;
        if (ctx->prof > 1 && k % ctx->prof != 0) { on = false; return; }   // sampling: this launch runs unbracketed
        auto get = [&](hipEvent_t* e) {
            if (!ctx->free_events.empty()) { *e = ctx->free_events.back(); ctx->free_events.pop_back(); }
            else if (hipEventCreate(e) != hipSuccess) *e = nullptr;
        };
        get(&a);
        get(&b);
        if (!a || !b) { on = false; return; }
        ctx->sites[site].launches += 1;
        ctx->sites[site].flops += flops;
        ctx->sites[site].bytes += bytes;
        ctx->sites[site].exec += exec;
        hipEventRecord(a, stream);
    }
    ~ProfScope() {
        if (!on) return;
        hipEventRecord(b, stream);
        ctx->pending.push_back({site, a, b});
    }
};

inline _Float16* hi_of(const Buffer& b) { return reinterpret_cast<_Float16*>(b.d); }
inline _Float16* lo_of(const Buffer& b, int n) { return reinterpret_cast<_Float16*>(b.d) + (size_t)n * b.S * b.S * b.Cs; }

int check_range_flag(umx_ctx* ctx);   // call with the stream idle
// umx_stitch_dev's body with the internal forms: stitch = kStitchU8 (uint8 planes), plane_rows > 0 (rows per class plane of `out_dev`)
int stitch_rows(umx_ctx* ctx, const float* probs_dev, int tpr0, int tpr1, int H, int W, int mode, int stitch, int y0, int y1,
                void* out_dev, int plane_rows);
// tiles [t0, t1) of the slide (row-major tile index) -> probs_dev (tile t0 first): gather + normalise + UNet
// (raw_dev / raw_bits: the same planes as raw uint8 / uint16 values, for an engine that gathers from them -- gathers_raw())
int tiles_range(umx_ctx* ctx, const double* image_dev, int C_img, const TileGeom& g, int band_row0, int band_rows,
                double mean, double stdv, int t0, int t1, float* probs_dev, const void* raw_dev = nullptr, int raw_bits = 0,
                const unsigned* mm_dev = nullptr /* raw planes: rescale_intensity to each plane's (min, max) words, 16 words apart */);
// the tile gather of this engine can read raw integer planes (im2double in the gather: no float64 image is written or read)
bool gathers_raw(const umx_ctx* ctx);

// ---- umx_host.hip: the image entries' argument checks (nothing enqueued; raw: 8 / 16-bit planes, else float64; range may be NULL)
int check_image(umx_ctx* ctx, bool ptrs, int C_img, int H, int W, bool raw, int bits, double stdv, int mode, int stitch,
                const uint32_t* range);
// a call on host slot `slot` (umx_ctx::hs): slot checks, hipSetDevice, the slot's prologue (its range-flag word cleared and made the
// launches'), then `enqueue`, which ends in slot_finish; an error after the checks drains the upload, context and download streams
int slot_submit(umx_ctx* ctx, int slot, const std::function<int()>& enqueue);
// the slot's range flag goes down on dn_s behind what that stream holds, `done` is recorded there and the slot is busy
int slot_finish(umx_ctx* ctx, int slot, hipStream_t dn_s);
// a caller's planes' (min, max) -> each plane's mm words (16 apart), on the context's stream
int put_range(umx_ctx* ctx, unsigned* mm, const uint32_t* range, int C_img);

// ---- umx_pipeline.hip: the schedules of the whole-slide entries as data (no HIP call, no context, no getenv)
// A step of a slide's schedule: one thing the executor (umx_host.hip host_enqueue) enqueues, in the plan's order.  Rows are image
// rows of every plane, tiles row-major tile indices, events indices into the slot's events.
enum StepKind {
    kStepUpload,          // rows [a, b) go up on the upload stream; event c is recorded behind them (c < 0: none)
    kStepWaitUpload,      // the compute stream waits for event a
    kStepMinMaxInit,      // the planes' (min, max) words are reset
    kStepPutRange,        // ... and set to the range the caller handed in or the host pass found
    kStepHostRange,       // the host finds the planes' (min, max) while the rows enqueued so far cross the bus
    kStepMinMax,          // rows [a, b) are reduced into the (min, max) words on the device
    kStepConvert,         // raw rows [a, b) -> float64 rows (im2double [+ rescale])
    kStepTiles,           // tiles [a, b): gather + normalise + UNet
    kStepStitch,          // output rows [a, b) are stitched from the patch rows < c
    kStepDownloadEvent,   // event a is recorded on the compute stream and the download stream waits for it
    kStepDownload,        // output rows [a, b) go down on the download stream
    kStepFlag             // the range flag's hand-over to the download stream through event a (an engine without the flag skips it)
};
TileGeom geom_of(const umx_hparams& hp, int H, int W);
struct Step { int kind, a, b, c; };
struct SlideSpec {                 // what the schedule of a slide depends on besides its tile geometry
    int max_batch = 1, K = 1, C_img = 1;
    int src_bits = 0;              // 0: float64 planes; 8 / 16: raw integer planes
    int rescale = 0;
    bool has_range = false;        // the caller handed the planes' (min, max) in
    bool sync_call = true;         // a synchronous entry (else submitted: umx_infer_image_raw_submit)
    bool host_range_ok = true;     // the host may find the range itself (UMX_HOST_RANGE is not 0)
    size_t stitch_el = 2;          // bytes of a stitched element (fp16-compatible: 2, fp32: 4)
    int out_u8 = 0;                // the drivers' uint8 planes go down instead of the stitch result
    bool raw_gather = false;       // the engine's tile gather reads raw planes (gathers_raw)
    double tile_flops = 0.0;       // algorithmic FLOPs of one tile: the 0.6 TFLOP rule of `single`
};
struct SlidePlan {
    // the slot's d_out: [stitched planes pm_b | uint8 planes u8_b | raw planes at raw_off | (min, max) words at mm_off], out_b in all;
    // image_b: the float64 image (0: never made); probs_b: the tile probabilities
    size_t pm_b = 0, u8_b = 0, raw_off = 0, mm_off = 0, out_b = 0, image_b = 0, probs_b = 0;
    int S = 1;                     // slabs = launch groups
    bool single = false;           // one in-order stream: no copy streams, no events
    int nev = 0;                   // events the steps index
    std::vector<Step> steps;
};
SlidePlan slide_plan(const TileGeom& g, const SlideSpec& sp);
std::string slide_describe(const SlidePlan& p);   // a header line, then one line per step

struct BandSpec {                  // what the schedule of one rank's band depends on besides the slide's tile geometry
    int world = 1, rank = 0, nslabs = 1, max_batch = 1;
    int band_row0 = 0, band_rows = 0;
    int K = 1;
    size_t gather_el = 2;          // bytes of a gathered element (uint8 result: 1, else the stitched element)
    bool staged = false;           // a host band goes up piece by piece ahead of the tiles that read it ...
    bool own_stream = false;       // ... on a stream of its own (an event hands each piece to the compute stream)
};
struct BandPlan {
    std::vector<int> A, B, active; // every rank's patch rows [A[q], B[q]); the ranks that have any
    int n = 1;                     // slabs
    int pa = 0, pb = 0, lo = 0;    // this rank's patch rows; the first patch row in `probs` (pa - 1 with a previous rank's halo row)
    int F = 0;                     // tiles of the first launch group: the band's last ones
    int send_peer = -1, recv_peer = -1;   // halo: the band's last patch row goes to the next active rank, the previous one's comes in
    int own0 = 0, own1 = 0;        // output rows this rank stitches
    int mx_all = 1;                // rows of the largest slab of any rank: the padding of the gather buffers
    size_t probs_b = 0, send_b = 0, gathered_b = 0;
    int nev = 0;
    struct Group { int t0, t1, r0, r1, ev; };   // tiles [t0, t1); staged image rows [r0, r1) in front of them (none: r1 <= r0) and their event (none: < 0)
    std::vector<Group> groups;     // in launch order; before slab 0's: the first group
    struct Slab {
        int g0 = 0, g1 = 0;        // the launch groups it still needs: groups [g0, g1)
        int s0 = 0, s1 = 0;        // this rank's rows of it
        std::vector<int> ra, rb;   // every rank's rows of it
        int mx = 1;                // rows of its largest piece: the padding of this gather
        int ev = 0;                // recorded behind its stitch
    };
    std::vector<Slab> slabs;
};
BandPlan band_plan(const TileGeom& g, const BandSpec& sp);
std::string band_describe(const BandPlan& p);     // a header line, then one line per launch group and per slab, in order

}  // namespace umx

namespace umx_geom {   // band geometry (the C twin of unmicst_amd/sharding.py)
void band(int npr, int world, int rank, int* pa, int* pb);
void owned(int pa, int pb, int npr, int sub, int margin, int H, int* y0, int* y1);
void needed(int pa, int pb, int sub, int margin, int patch, int H, int* r0, int* r1);
int cut(int pa, int pb, int n, int i);
void slab(int pa, int pb, int npr, int sub, int margin, int H, int n, int i, int* s0, int* s1);
}  // namespace umx_geom

namespace umx {

// ---- umx_shard.hip
void shard_release(umx_ctx* ctx);               // frees ctx->shard and its buffers in ctx->mem
hipStream_t shard_stream(const umx_ctx* ctx);   // the communication stream of a sharded context, else null
int shard_wait(umx_ctx* ctx, hipEvent_t ev);    // the bounded wait of a submitted call on a sharded context

// ---- training step (umx_train.hip) as the training set (umx_trainset.hip) sees it ----
struct TrainerIO {
    int device, B, P, C, K;            // batch, tile, input channels, classes
    bool legacy;
    hipStream_t stream;
    float *data, *labels, *weights;    // the step's own input buffers [B,P,P,C] / [B,P,P,K] (what umx_train_step uploads into)
    const float* probs;                // softmax of the last forward pass [B,P,P,K]
};
TrainerIO trainer_io(umx_trainer* tr);
int trainer_fail(umx_trainer* tr, int code, const char* msg);   // -> code, with msg as umx_trainer_last_error
// umx_trainer_eval = begin (device, range-flag bookkeeping), batch into io.data, forward (-> io.probs), read-back, end (sync, flag)
int trainer_eval_begin(umx_trainer* tr);
int trainer_eval_forward(umx_trainer* tr);
int trainer_eval_end(umx_trainer* tr);
// guard mode: wait for every stream of the trainer, then check its red zones (UMX_OK when the mode is off)
int trainer_guard_check(umx_trainer* tr);

// ---- training-set kernels (assembly: umx_trainset_assemble.hip; class counts: umx_trainset.hip) ----
constexpr int kDescChunk = 64;         // descriptors per assembly launch (passed by value: 2 KiB of kernel arguments)
struct DescChunk { umx_sample_desc d[kDescChunk]; };
struct TrainSetView {                  // device layout of one training set
    const float* planes;               // [N][C][pages][S][row_f]
    const uint8_t* ann;                // [N][S][row_a]
    const float* wmap;                 // [N][S][row_f], or null (unweighted)
    int S, pages, C, row_f, row_a;
    float cw[8], iw[8];
};
// rows b0 .. b0+m-1 of data [B,P,P,C] / labels, weights [B,P,P,K] (weights null: none); a descriptor with index < 0 writes zeros
hipError_t launch_assemble_batch(const TrainSetView& ts, const DescChunk& dc, int m, int b0, int P, int K, float* data, float* labels,
                                 float* weights, hipStream_t stream);
// the data planes of the images that ask for blur or saturation (umx_augment_desc), written over what launch_assemble_batch wrote
constexpr int kAugChunk = 16;          // such images per launch (passed by value: 1.75 KiB of kernel arguments)
struct AugImage {
    umx_sample_desc d;
    int row;                           // image of the batch
    int R;                             // blur radius; -1: no blur (level 0)
    float gain;
    float taps[UMX_AUGMENT_MAX_RADIUS + 1];
    float m[4];                        // umx_warp_desc (read by the warped launches only)
};
struct AugChunk { AugImage im[kAugChunk]; };
hipError_t launch_assemble_augmented(const TrainSetView& ts, const AugChunk& ac, int m, int P, float mean, float std, float* data,
                                     hipStream_t stream);
// an image with an elastic deformation (umx_elastic_desc, n != 0): the lattice rides behind the image's other arguments; a.m is
// always read (the identity for an image without a rotation / zoom)
constexpr int kElasticChunk = 8;       // such images per launch (passed by value: 3.2 KiB of the 4 KiB a launch may carry)
struct ElasticImage {
    AugImage a;
    int n;                             // lattice points per axis, 4..6
    float d[2][UMX_ELASTIC_MAX_GRID][UMX_ELASTIC_MAX_GRID];
};
struct ElasticChunk { ElasticImage im[kElasticChunk]; };
// the same for images with a rotation / zoom (Chunk = AugChunk: umx_warp_desc, never the identity) or an elastic deformation (Chunk =
// ElasticChunk): the data planes resampled, then blur, saturation, transform and jitter as above, and their labels / weights (null:
// none) from the nearest source pixel.  Needs ts.S >= 2, and P >= 2 under a lattice.  Instantiated for these two chunk types.
template <typename Chunk>
hipError_t launch_assemble_resampled(const TrainSetView& ts, const Chunk& ch, int m, int P, int K, float mean, float std, float* data,
                                     float* labels, float* weights, hipStream_t stream);
// counts [2K] int64 (correct | labelled) and loss [1] double over npix pixels of probs / labels [npix, K]; part: class_counts_parts(npix)
// doubles of workspace
size_t class_counts_parts(size_t npix, int K);
hipError_t launch_class_counts(const float* probs, const float* labels, size_t npix, int K, double* part, long long* counts,
                               double* loss, hipStream_t stream);

// ---- object score (umx_trainset_objects.hip; the labelling is launch_border_label below) ----
constexpr int kObjectMaxTile = 4096;   // P^2 fits an int32 with room to spare and a pair key t * P^2 + p + 1 a uint64
// the device memory of the pass, for B images of P x P (allocated by the first call of an object entry, in the set's arena)
struct ObjectWorkspace {
    int B = 0, P = 0;
    size_t slots = 0;                  // object_table_slots(P), per image
    uint8_t* planes = nullptr;         // [2][B][P][P] class codes: truth | prediction
    int* words = nullptr;              // [6][B][P^2]: roots of truth | of the prediction | areas at the roots, twice | partner counts, twice
    unsigned long long* keys = nullptr;   // [B][slots] pair keys, 0 = empty
    int* overlap = nullptr;            // [B][slots] shared pixels of the slot's pair
    long long* counts = nullptr;       // [B][UMX_OBJECT_COUNTS]
};
size_t object_table_slots(int P);      // the least power of two >= max(64, 2 P^2)
// truth / pred [n][P][P] from probs / labels [n,P,P,K]: the label's code (0: none) and 1 + argmax (first maximum; 0 where the truth is 0)
hipError_t launch_object_planes(const float* probs, const float* labels, int n, int P, int K, uint8_t* truth, uint8_t* pred,
                                hipStream_t stream);
// pred = 0 where truth = 0, in place: the same rule for planes that came from the host
hipError_t launch_object_rule(const uint8_t* truth, uint8_t* pred, int n, int P, hipStream_t stream);
// from the planes of images 0..n-1 on: clears areas, partner counts and tables, labels both planes (roots in words[0] / words[1]),
// counts areas and overlaps, reduces to counts[n][8]
hipError_t launch_object_counts(const ObjectWorkspace& w, int n, int code, int min_area, hipStream_t stream);

// ---- border weight maps (umx_trainset_border.hip) ----
// 4-connected components of (annotation == code) of n samples (ann: the first one's plane, [S][row_a] each) into ws [n][S][S]: the
// flat index of the component's first pixel in raster order, -1 off the objects.  One workgroup per sample; S * S fits an int32.
hipError_t launch_border_label(const uint8_t* ann, int n, int S, int row_a, int code, int* ws, hipStream_t stream);
// from those planes: wmap (sample stride plane_w, row stride row_w floats) and, where given, labels (root + 1; 0 off the objects),
// d1sq and d2sq [n][S][S].  R = border_radius(sigma) <= 32, den = 2 sigma^2.
hipError_t launch_border_map(const int* ws, int n, int S, int R, double den, float* wmap, int row_w, size_t plane_w, int* labels,
                             int* d1sq, int* d2sq, hipStream_t stream);
int border_radius(float sigma);        // ceil(4 sigma)

}  // namespace umx
