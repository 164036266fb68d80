// libumx label mask: the labeler's state and the few host pieces that its five sources share -- umx_label.hip (labelling, growth,
// split, flood, measurement, shapes), umx_label_hmax.hip (h-maxima seeds), umx_label_contact.hip (contacts), umx_label_hull.hip
// (hulls) and umx_label_relabel.hip (relabel).  Nothing here is part of the C ABI (include/umx.h).
#pragma once

#include "umx_internal.h"

struct umx_labeler {
    int device = 0;
    hipStream_t stream = nullptr;
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};   // upload begins | launches begin | downloads begin | all done
    umx::DevArena mem;
    uint8_t* d_planes = nullptr;  size_t planes_cap = 0;       // bytes
    int* d_P = nullptr;
    int* d_Q = nullptr;           size_t pix_cap = 0;          // words of either plane
    int* d_counts = nullptr;      size_t counts_cap = 0;       // words
    long long* d_n = nullptr;
    umx_label_object* d_table = nullptr;  size_t table_cap = 0;   // records
    // the split's own (allocated from the first split run on, then kept like the others): the third plane, the flags, three words
    int* d_R = nullptr;
    uint8_t* d_B = nullptr;       size_t split_cap = 0;        // words of d_R = bytes of d_B (rounded up to a whole word); 0: never asked for
    long long* d_split = nullptr;                              // kSplitWords words the kernels of a split run add to
    long long* d_flood = nullptr;                              // kFloodWords words a flood launch reports in (allocated with d_split)
    long long* d_hmax = nullptr;                               // kHmaxWords words the h-maxima seeds report in (allocated with d_split)
    std::vector<umx_label_object> table;                       // of the last run
    double ms[3] = {0.0, 0.0, 0.0};
    // the resident labels: d_P holds the int32 [res_H][res_W] label plane of res_N objects iff res_why is null; else why it does not
    int res_H = 0, res_W = 0;
    long long res_N = 0;
    const char* res_why = "no umx_labeler_run has given this labeler a label plane yet";
    // the measurement's own allocations (of the same arena, never part of ensure_buffers' sizes): staging for one group of planes,
    // the records of one group
    void* d_mplanes = nullptr;    size_t mplanes_cap = 0;      // bytes
    umx_label_measure* d_mrec = nullptr;  size_t mrec_cap = 0; // records
    double mms[3] = {0.0, 0.0, 0.0};
    // the shapes' own allocation, as the measurement's: the records
    umx_label_shape* d_srec = nullptr;    size_t srec_cap = 0; // records
    double sms[2] = {0.0, 0.0};                                // launches | download
    // the contacts' own allocations, as the measurement's (umx_label_contact.hip): the table's keys and counts, the per-label words
    // (contacts per label, their prefix sums, the block sums of the scan), the records twice (scattered | ordered), the words the
    // host reads, and the scratch planes of a reach where d_Q and d_R do not serve
    unsigned long long* d_ckeys = nullptr;  size_t ckeys_cap = 0;    // entries
    unsigned* d_cedges = nullptr;           size_t cedges_cap = 0;   // entries
    int* d_crows = nullptr;                 size_t crows_cap = 0;    // words
    umx_label_contact* d_crec = nullptr;    size_t crec_cap = 0;     // records (twice the list)
    long long* d_cwords = nullptr;          size_t cwords_cap = 0;   // words
    int* d_cplane[2] = {nullptr, nullptr};  size_t cplane_cap[2] = {0, 0};   // words
    size_t ctable = 0;                                         // entries the next pass starts with (0: the least)
    double cms[2] = {0.0, 0.0};                                // launches | download
    umx_label_contact_stats cstats = {0, 0, 0, 0, 0};
    // the hulls' own allocations, as the measurement's (umx_label_hull.hip): the row range of every label (ymin [N] | ymax [N]), the
    // 64-bit words (an offset per label, a sum per block of labels, the words the host reads), the row entries (least x [E] | largest
    // x + 1 [E]), the scratch vertices, the records and the vertex list
    int* d_hrange = nullptr;                 size_t hrange_cap = 0;    // words
    long long* d_hoff = nullptr;             size_t hoff_cap = 0;      // words
    int* d_hrows = nullptr;                  size_t hrows_cap = 0;     // words
    umx_label_hull_vertex* d_hscratch = nullptr;  size_t hscratch_cap = 0;   // vertices
    umx_label_hull* d_hrec = nullptr;        size_t hrec_cap = 0;      // records
    umx_label_hull_vertex* d_hverts = nullptr;    size_t hverts_cap = 0;     // vertices
    double hms[2] = {0.0, 0.0};                                // launches | download
    // the relabel's own allocations, as the measurement's (umx_label_relabel.hip): the map, and the second object table -- after a
    // relabel of the resident labels it and d_table have changed places, capacities included
    int* d_rmap = nullptr;                   size_t rmap_cap = 0;      // words
    umx_label_object* d_rtable = nullptr;    size_t rtable_cap = 0;    // records
    double rms[3] = {0.0, 0.0, 0.0};                           // upload | launches | download
    std::string err;
};

namespace umx {

// The byte plane B of a split run (umx_label.hip, umx_label_hmax.hip): flags per pixel
constexpr unsigned kFlagKept = 1u;    // the pixel belongs to a kept object (step 10: a pixel of M)
constexpr unsigned kFlagEroded = 2u;  // the pixel is in E (step 11, or step 35 with h-maxima seeds); not read any more once R holds E's components
constexpr unsigned kFlagCored = 4u;   // at the ROOT pixel of an object only: the object contains a core (step 12)
// the words of umx_labeler::d_hmax: the pixels the launches of either reconstruction raised so far, |E|
constexpr int kHmaxWords = 3, kHmaxRaised = 0, kHmaxSeeds = 2;

// the message into the labeler (and the thread's), the code back
int lfail(umx_labeler* lb, int code, const char* fmt, ...);

#define L_HIP(lb, expr)                                                                                                  \
    do {                                                                                                                 \
        hipError_t e__ = (expr);                                                                                         \
        if (e__ != hipSuccess)                                                                                           \
            return lfail(lb, e__ == hipErrorOutOfMemory ? UMX_ERR_OOM : UMX_ERR_HIP, "%s failed: %s", #expr, hipGetErrorString(e__)); \
    } while (0)

// A buffer of the measurement, the shapes or the contacts at least `need` (bytes or records) large: its own allocation of the arena,
// released and made again when it must grow.  Nothing else of the arena moves, so the resident labels stay.
template <typename P>
int ensure_measure_buffer(umx_labeler* lb, P** buf, size_t* cap, size_t need, size_t unit, const char* what) {
    if (*buf && need <= *cap) return UMX_OK;
    L_HIP(lb, hipStreamSynchronize(lb->stream));
    if (*buf) L_HIP(lb, arena_release(&lb->mem, *buf));
    *buf = nullptr; *cap = 0;
    const size_t n = std::max<size_t>(need, 1);
    L_HIP(lb, arena_alloc(&lb->mem, (void**)buf, n * unit, false, what));
    *cap = n;
    return UMX_OK;
}

// the contacts' allocations are gone with the arena (ensure_buffers of umx_label.hip empties it): they are made again when asked for
inline void contact_buffers_forget(umx_labeler* lb) {
    lb->d_ckeys = nullptr; lb->d_cedges = nullptr; lb->d_crows = nullptr; lb->d_crec = nullptr; lb->d_cwords = nullptr;
    lb->d_cplane[0] = lb->d_cplane[1] = nullptr;
    lb->ckeys_cap = lb->cedges_cap = lb->crows_cap = lb->crec_cap = lb->cwords_cap = lb->cplane_cap[0] = lb->cplane_cap[1] = 0;
}

// and so are the hulls'
inline void hull_buffers_forget(umx_labeler* lb) {
    lb->d_hrange = nullptr; lb->d_hoff = nullptr; lb->d_hrows = nullptr; lb->d_hscratch = nullptr; lb->d_hrec = nullptr; lb->d_hverts = nullptr;
    lb->hrange_cap = lb->hoff_cap = lb->hrows_cap = lb->hscratch_cap = lb->hrec_cap = lb->hverts_cap = 0;
}

// and so are the relabel's
inline void relabel_buffers_forget(umx_labeler* lb) {
    lb->d_rmap = nullptr; lb->d_rtable = nullptr;
    lb->rmap_cap = lb->rtable_cap = 0;
}

// Launches of kernels that live in umx_label.hip, for umx_label_contact.hip.
// label_grow_kernel's "every zero pixel is domain" form: `levels` (1 .. UMX_LABEL_GROW_HALO) levels of the growth src -> dst (two
// different planes of H x W) over the pixels whose value is outside 1..N, which count as 0
void launch_grow_free(hipStream_t s, int H, int W, int N, const int* src, int* dst, int levels);
// label_scan_kernel: counts[0 .. nblocks) -> their exclusive prefix sums in place, the sum to *total; nblocks <= 2^20
void launch_block_scan(hipStream_t s, int* counts, int nblocks, long long* total);

// The h-maxima seeds (umx_label_hmax.hip), for run_split_launches in the erosion's place.  P:
// the objects' roots, Q: their areas at the roots (read here for the last time).  B gets kFlagKept | kFlagEroded for every pixel as
// label_erode_kernel leaves them, with E the extended maxima; the int32 plane R is used as four byte planes.  d_hmax is cleared and
// takes the raised counts and |E|; recon_launches: the launches of the two reconstructions.  The stream is idle on return but for
// the last launch.
int launch_hmax_seeds(umx_labeler* lb, const uint8_t* planes, int H, int W, const int* P, const int* Q, int min_area,
                      const umx_label_hmax_options* ho, int64_t recon_launches[2]);

}  // namespace umx
