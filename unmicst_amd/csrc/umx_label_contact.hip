// libumx label mask, contacts: which labelled objects touch and along how many pixel edges -- the kernels and the C ABI behind
// umx_labeler_contacts / _contacts_dev (include/umx.h).  One call is this sequence of launches
// on the labeler's stream, from a label plane that is only read:
//
//   label_grow_kernel<false, true>   (reach R > 0 only; umx_label.hip) ceil(R / 8) launches of the growth over "every pixel that
//                            carries no label", labels -> S0 -> S1 -> S0 ...: the scratch plane the pass below reads instead
//   (keys, edge counts and the per-label counts are cleared)
//   contact_emit_kernel      one wave per row: the pairs (row, row) between horizontal neighbours and (row, row + 1) between vertical
//                            ones; equal pairs on consecutive pixels -- a shared border that runs along the row -- collapse in the
//                            wave to one segment, carried across chunk ends, and one lane inserts the pair with the segment's
//                            length: a 64-bit atomicCAS into an open-addressing table of keys a << 32 | b (0: empty; a >= 1), a
//                            32-bit atomicAdd into the count of the slot, and for the lane that created the key one more into
//                            rows[a - 1], the contacts of label a
//   contact_rowsum_kernel    per block of 2048 labels the sum of rows[] (and the largest of them, to a word the host reads)
//   label_scan_kernel        (umx_label.hip) ONE workgroup: the block sums to their exclusive prefix sums, the total M to the host's word
//   contact_offsets_kernel   per block again: start[a - 1] = contacts of all labels below a, start[N] = M
//   (M, the overflow word and the longest row come back to the host: the only synchronisation.  Overflow: the table is doubled and
//   everything from the clearing on runs again)
//   contact_scatter_kernel   one thread per slot: a used slot takes the next free place of its label's row, start[a - 1] + (--rows[a - 1])
//   contact_rank_kernel      one thread per record: its place inside its row is the number of records of the row with a smaller b
//                            (they are distinct) -- quadratic in the row, so only when no row is longer than
//                            UMX_CONTACT_DEVICE_SORT_MAX; else the scattered list goes down and contact_sort_rows orders it
//
// Why no thread waits for another one: an insertion walks at most `probes` slots, a bound fixed at launch, and gives up into the
// overflow word; a slot's key changes once, from 0 to its key, by the one CAS that wins, and every other thread that meets the slot
// sees either 0 (and loses its CAS to the key that is there, which it then compares) or the key.  A read that is stale can only
// show 0 for a key that is there: the CAS corrects it.  Nothing reads a count, rows[] or a word in the launch that adds to it.
// Why the result does not depend on any order: the set of keys and the integer sums are order-free; where a key lands in the table
// and in its row before the ranking is not, and the ranking (or the host's sort) by b inside rows that are in order of a removes it.
#include "../../include/umx.h"
#include "umx_contact_host.h"
#include "umx_internal.h"
#include "umx_label_state.h"

#include <climits>

namespace umx {

namespace {

constexpr int kRowWaves = 4;                             // rows of the image per workgroup, as the one-wave-per-row kernels of umx_label.hip
constexpr int kPixThreads = 256;                         // one thread per slot / record / 8 labels
constexpr int kScanBlock = UMX_LABEL_SCAN_BLOCK;
constexpr int kPerThread = kScanBlock / kPixThreads;     // labels per thread of the two per-label kernels
constexpr int kWordTotal = 0, kWordOverflow = 1, kWordLongest = 2, kWords = 4;   // umx_labeler::d_cwords (64-bit words)
static_assert(kPerThread * kPixThreads == kScanBlock, "a block of labels is a whole number per thread");
static_assert(sizeof(umx_label_contact) == 16 && sizeof(umx_label_contact_stats) == 32, "the contact records");
static_assert((UMX_CONTACT_TABLE_MIN & (UMX_CONTACT_TABLE_MIN - 1)) == 0 && (UMX_CONTACT_TABLE_MAX & (UMX_CONTACT_TABLE_MAX - 1)) == 0 &&
                  UMX_CONTACT_TABLE_MIN <= UMX_CONTACT_TABLE_MAX && UMX_CONTACT_PROBE_MAX <= UMX_CONTACT_TABLE_MIN,
              "table sizes are powers of two; a probe walk is never longer than the table");
static_assert(UMX_CONTACT_MAX_REACH <= UMX_LABEL_MAX_GROW, "the reach is a growth");

struct Table {
    unsigned long long* keys;   // [mask + 1], 0: empty
    unsigned* edges;            // [mask + 1]
    int* rows;                  // [N]: keys created with this smaller label
    unsigned* overflow;         // one word: an insertion found no slot
    unsigned mask, probes;      // entries - 1 (a power of two); slots an insertion looks at, <= entries
};

__device__ inline unsigned long long pair_key(int p, int q) {
    if (p <= 0 || q <= 0 || p == q) return 0ull;
    return p < q ? ((unsigned long long)(unsigned)p << 32) | (unsigned)q : ((unsigned long long)(unsigned)q << 32) | (unsigned)p;
}

// `n` edges of the pair `key` (!= 0; its upper word is 1..N).  At most t.probes rounds; slot <= t.mask; rows index < N.
__device__ inline void contact_insert(const Table& t, unsigned long long key, unsigned n) {
    unsigned long long h = key;
    h ^= h >> 33; h *= 0xff51afd7ed558ccdull; h ^= h >> 33; h *= 0xc4ceb9fe1a85ec53ull; h ^= h >> 33;
    unsigned slot = (unsigned)h & t.mask;
    for (unsigned i = 0; i < t.probes; ++i) {
        unsigned long long k = __hip_atomic_load(t.keys + slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (k == 0ull) {
            k = atomicCAS(t.keys + slot, 0ull, key);
            if (k == 0ull) {                              // this lane created the key
                atomicAdd(t.rows + ((int)(key >> 32) - 1), 1);
                k = key;
            }
        }
        if (k == key) {
            atomicAdd(t.edges + slot, n);
            return;
        }
        slot = (slot + 1u) & t.mask;
    }
    atomicOr(t.overflow, 1u);
}

// The segments of equal key of one row, chunk by chunk: called by all 64 lanes once per chunk with the lane's key (0: no pair; a lane
// past the row's end holds 0); insert(key, len) once for every maximal segment of equal key != 0 -- by one lane.  A segment that
// reaches the end of a chunk is carried in wave-uniform registers and joined to the first segment of the next chunk when the keys
// agree (for_each_run of umx_label.hip, with a 64-bit key and no start).  len <= the row's length.
struct Carried {
    unsigned long long key = 0ull;
    unsigned len = 0;
};
template <typename Insert>
__device__ inline void segments_of_chunk(int lane, unsigned long long key, bool last, Carried& c, Insert insert) {
    const unsigned long long kl = __shfl_up(key, 1);
    const bool head = lane == 0 || key != kl;
    const unsigned long long heads = __ballot(head);      // (bit 0 is always set)
    const unsigned long long later = lane == 63 ? 0ull : heads >> (lane + 1);
    unsigned len = later ? (unsigned)__ffsll((long long)later) : 64u - (unsigned)lane;   // pixels up to the next head, or to the chunk's end
    const unsigned long long k0 = __shfl(key, 0);
    if (lane == 0 && c.key != 0ull) {
        if (k0 == c.key) len += c.len;
        else insert(c.key, c.len);
    }
    if (head && key != 0ull && (later || last)) insert(key, len);
    const int hl = 63 - __clzll((long long)heads);        // the head of the chunk's last segment
    const unsigned long long lk = __shfl(key, hl);
    const unsigned ll = __shfl(len, hl);
    c.key = last ? 0ull : lk;
    c.len = ll;
}

// grid ceil(H / 4).  labels [H][W] is only read: row y by its wave's lanes, row y + 1 alongside it (none below the last row); a value
// outside 1..N is 0 and forms no pair.  Bounds: row y < H; a lane is in the row iff lane < W - x0 (no x0 + lane is formed past the
// row's end, W may be 2^31 - 1); a pixel word is r * W + x < H * W <= INT_MAX for r <= H - 1; column x0 + 64 is read by lane 63
// alone and only where it is < W.  The table: contact_insert.
__global__ void __launch_bounds__(64 * kRowWaves) contact_emit_kernel(const int* __restrict__ labels, int H, int W, int N, Table t) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if ((long long)blockIdx.x * kRowWaves + wave >= H) return;    // (the whole wave: no barrier below)
    const int y = blockIdx.x * kRowWaves + wave;
    const int* mid = labels + (size_t)y * W;
    const int* dn = y + 1 < H ? labels + (size_t)(y + 1) * W : nullptr;
    auto clean = [&](int v) { return v >= 1 && v <= N ? v : 0; };
    auto insert = [&](unsigned long long key, unsigned n) { contact_insert(t, key, n); };
    Carried across, below;
    const int nchunks = (W - 1) / 64 + 1;
    for (int c = 0; c < nchunks; ++c) {
        const int x0 = c * 64;
        const bool in = lane < W - x0;
        const int x = in ? x0 + lane : x0;
        const int m = in ? clean(mid[x]) : 0;
        const int d = in && dn ? clean(dn[x]) : 0;
        int r = __shfl_down(m, 1);                        // (a lane past the row's end holds 0)
        if (lane == 63) r = in && x < W - 1 ? clean(mid[x + 1]) : 0;
        const bool last = c + 1 == nchunks;
        segments_of_chunk(lane, pair_key(m, r), last, across, insert);
        segments_of_chunk(lane, pair_key(m, d), last, below, insert);
    }
}

// grid ceil(N / 2048), 256 threads of 8 labels.  rows [N] is only read; bsum[block] by thread 0; *longest: an integer atomicMax per
// workgroup that nothing reads in this launch.
__global__ void __launch_bounds__(kPixThreads) contact_rowsum_kernel(const int* __restrict__ rows, long long N, int* __restrict__ bsum,
                                                                     int* __restrict__ longest) {
    __shared__ int s_sum, s_max;
    if (threadIdx.x == 0) { s_sum = 0; s_max = 0; }
    __syncthreads();
    const long long base = (long long)blockIdx.x * kScanBlock + (long long)threadIdx.x * kPerThread;
    int sum = 0, mx = 0;
    for (int j = 0; j < kPerThread; ++j)
        if (base + j < N) {
            const int v = rows[base + j];
            sum += v;
            mx = v > mx ? v : mx;
        }
    if (sum) { atomicAdd(&s_sum, sum); atomicMax(&s_max, mx); }   // (LDS)
    __syncthreads();
    if (threadIdx.x == 0) {
        bsum[blockIdx.x] = s_sum;
        if (s_max) atomicMax(longest, s_max);
    }
}

// grid ceil(N / 2048), 256 threads of 8 consecutive labels.  bsum: the exclusive prefix sums of the blocks.  start [N + 1]: word i
// by the thread of label i alone, word N by the thread of label N - 1.  All sums are <= M <= the table's entries <= 2^28.
__global__ void __launch_bounds__(kPixThreads) contact_offsets_kernel(const int* __restrict__ rows, long long N, const int* __restrict__ bsum,
                                                                      int* __restrict__ start) {
    __shared__ int wsum[kPixThreads / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long base = (long long)blockIdx.x * kScanBlock + (long long)threadIdx.x * kPerThread;
    int v[kPerThread], mine = 0;
#pragma unroll
    for (int j = 0; j < kPerThread; ++j) {
        v[j] = base + j < N ? rows[base + j] : 0;
        mine += v[j];
    }
    int s = mine;                                         // inclusive over the wave's threads
    for (int d = 1; d < 64; d <<= 1) {
        const int u = __shfl_up(s, d);
        if (lane >= d) s += u;
    }
    if (lane == 63) wsum[wave] = s;
    __syncthreads();
    int off = bsum[blockIdx.x] + s - mine;
    for (int k = 0; k < wave; ++k) off += wsum[k];
#pragma unroll
    for (int j = 0; j < kPerThread; ++j) {
        if (base + j < N) {
            start[base + j] = off;
            if (base + j == N - 1) start[N] = off + v[j];
        }
        off += v[j];
    }
}

// one thread per slot, i < entries.  keys and edges are only read; rows[a - 1] counts down from the row's length to 0, so the
// places start[a - 1] + 0 .. length - 1 are given out once each: rec[place] < rec[M].  start is only read.
__global__ void __launch_bounds__(kPixThreads) contact_scatter_kernel(const unsigned long long* __restrict__ keys, const unsigned* __restrict__ edges,
                                                                      long long entries, const int* __restrict__ start, int* __restrict__ rows,
                                                                      umx_label_contact* __restrict__ rec) {
    const long long i = (long long)blockIdx.x * kPixThreads + threadIdx.x;
    if (i >= entries) return;
    const unsigned long long key = keys[i];
    if (key == 0ull) return;
    umx_label_contact r;
    r.a = (int)(key >> 32); r.b = (int)(unsigned)key; r.edges = edges[i]; r.reserved = 0;
    const int place = atomicSub(rows + (r.a - 1), 1) - 1;
    rec[(size_t)start[r.a - 1] + (size_t)place] = r;
}

// one thread per record, i < M.  in: the scattered list, only read; out: the record's row [start[a - 1], start[a]) ordered by b.  At
// most UMX_CONTACT_DEVICE_SORT_MAX rounds (the host launches this only then); rank < the row's length.
__global__ void __launch_bounds__(kPixThreads) contact_rank_kernel(const umx_label_contact* __restrict__ in, long long M, const int* __restrict__ start,
                                                                   umx_label_contact* __restrict__ out) {
    const long long i = (long long)blockIdx.x * kPixThreads + threadIdx.x;
    if (i >= M) return;
    const umx_label_contact me = in[i];
    const int s = start[me.a - 1], e = start[me.a];
    int rank = 0;
    for (int j = s; j < e; ++j) rank += in[j].b < me.b;
    out[(size_t)s + (size_t)rank] = me;
}

inline unsigned row_grid(int H) { return (unsigned)((H - 1) / kRowWaves + 1); }
inline unsigned per_thread_grid(long long n) { return (unsigned)((n + kPixThreads - 1) / kPixThreads); }

// The scratch plane S of a reach (step 23) from `labels`, which is only read: ceil(reach / 8) growth launches, the first from the
// labels into plane 0, then between the two planes.  Plane 0 is the labeler's second plane d_Q (free between runs: nothing reads it
// after a run) and plane 1 the split's third plane d_R, where a run has allocated them at least H * W words large; else allocations
// of the contacts' own.  Neither holds the resident labels.  *S: the plane the last launch wrote.
int grow_reach(umx_labeler* lb, const int* labels, int N, int H, int W, int reach, const int** S) {
    const size_t npix = (size_t)H * W;
    int* plane[2] = {lb->d_Q && lb->pix_cap >= npix ? lb->d_Q : nullptr, lb->d_R && lb->split_cap >= npix ? lb->d_R : nullptr};
    for (int k = 0; k < (reach > UMX_LABEL_GROW_HALO ? 2 : 1); ++k) {
        if (plane[k]) continue;
        const int rc = ensure_measure_buffer(lb, &lb->d_cplane[k], &lb->cplane_cap[k], npix, sizeof(int), "contact reach plane");
        if (rc) return rc;
        plane[k] = lb->d_cplane[k];
    }
    const int* src = labels;
    int k = 0;
    for (int left = reach; left > 0; left -= UMX_LABEL_GROW_HALO, k ^= 1) {
        launch_grow_free(lb->stream, H, W, N, src, plane[k], std::min(left, (int)UMX_LABEL_GROW_HALO));
        src = plane[k];
    }
    *S = src;
    return UMX_OK;
}

// The contacts of `labels` (device, H x W, objects 1..N).  The caller has checked the arguments; out (may be null with cap 0) holds
// cap records.  Returns with the stream idle.
int contacts_any(umx_labeler* lb, const int* labels, long long N, int H, int W, int reach, umx_label_contact* out, long long cap,
                 int64_t* m_out) {
    L_HIP(lb, hipSetDevice(lb->device));
    lb->cms[0] = lb->cms[1] = 0.0;
    lb->cstats = umx_label_contact_stats{0, 0, 0, UMX_CONTACT_ORDER_NONE, 0};
    if (m_out) *m_out = 0;
    if (N == 0) return UMX_OK;
    hipStream_t s = lb->stream;
    const size_t nblocks = (size_t)((N + kScanBlock - 1) / kScanBlock);
    int rc = ensure_measure_buffer(lb, &lb->d_cwords, &lb->cwords_cap, kWords, sizeof(long long), "contact words");
    if (rc) return rc;
    if ((rc = ensure_measure_buffer(lb, &lb->d_crows, &lb->crows_cap, 2 * (size_t)N + 1 + nblocks, sizeof(int), "contact rows"))) return rc;
    int* const rows = lb->d_crows;
    int* const start = rows + N;
    int* const bsum = start + N + 1;
    L_HIP(lb, hipEventRecord(lb->ev[1], s));
    const int* S = labels;
    if (reach > 0 && (rc = grow_reach(lb, labels, (int)N, H, W, reach, &S))) return rc;
    size_t entries = std::max(lb->ctable, contact_first_table(N));
    long long M = 0, longest = 0;
    for (;;) {
        if ((rc = ensure_measure_buffer(lb, &lb->d_ckeys, &lb->ckeys_cap, entries, sizeof(unsigned long long), "contact keys"))) return rc;
        if ((rc = ensure_measure_buffer(lb, &lb->d_cedges, &lb->cedges_cap, entries, sizeof(unsigned), "contact edge counts"))) return rc;
        lb->ctable = entries;
        lb->cstats.table_capacity = (int64_t)entries;
        L_HIP(lb, hipMemsetAsync(lb->d_ckeys, 0, entries * sizeof(unsigned long long), s));
        L_HIP(lb, hipMemsetAsync(lb->d_cedges, 0, entries * sizeof(unsigned), s));
        L_HIP(lb, hipMemsetAsync(rows, 0, (size_t)N * sizeof(int), s));
        L_HIP(lb, hipMemsetAsync(lb->d_cwords, 0, kWords * sizeof(long long), s));
        Table t;
        t.keys = lb->d_ckeys; t.edges = lb->d_cedges; t.rows = rows;
        t.overflow = reinterpret_cast<unsigned*>(lb->d_cwords + kWordOverflow);
        t.mask = (unsigned)(entries - 1);
        t.probes = (unsigned)std::min<size_t>(entries, UMX_CONTACT_PROBE_MAX);
        hipLaunchKernelGGL(contact_emit_kernel, dim3(row_grid(H)), dim3(64 * kRowWaves), 0, s, S, H, W, (int)N, t);
        hipLaunchKernelGGL(contact_rowsum_kernel, dim3((unsigned)nblocks), dim3(kPixThreads), 0, s, rows, N, bsum,
                           reinterpret_cast<int*>(lb->d_cwords + kWordLongest));
        launch_block_scan(s, bsum, (int)nblocks, lb->d_cwords + kWordTotal);
        hipLaunchKernelGGL(contact_offsets_kernel, dim3((unsigned)nblocks), dim3(kPixThreads), 0, s, rows, N, bsum, start);
        L_HIP(lb, hipGetLastError());
        long long words[kWords] = {0, 0, 0, 0};
        L_HIP(lb, hipMemcpyAsync(words, lb->d_cwords, sizeof words, hipMemcpyDeviceToHost, s));
        L_HIP(lb, hipStreamSynchronize(s));
        if (words[kWordOverflow] == 0) {
            M = words[kWordTotal];
            longest = words[kWordLongest];
            break;
        }
        if (entries >= (size_t)UMX_CONTACT_TABLE_MAX)
            return lfail(lb, UMX_ERR_OOM, "the contact table of %zu entries is too small and UMX_CONTACT_TABLE_MAX is %lld: the plane has more contacts "
                                          "than the library lists", entries, (long long)UMX_CONTACT_TABLE_MAX);
        entries *= 2;
        ++lb->cstats.reruns;
    }
    if (M < 0 || M > (long long)entries || longest < 0 || longest > M)
        return lfail(lb, UMX_ERR_HIP, "the contact pass counted %lld contacts, the longest row %lld, in a table of %zu entries", M, longest, entries);
    lb->cstats.longest_row = longest;
    if (m_out) *m_out = M;
    const bool count_only = !out && cap == 0;
    const bool refused = !count_only && (!out || cap < M);
    if (M > 0 && !count_only && !refused) {
        if ((rc = ensure_measure_buffer(lb, &lb->d_crec, &lb->crec_cap, 2 * (size_t)M, sizeof(umx_label_contact), "contact records"))) return rc;
        umx_label_contact* const scattered = lb->d_crec;
        umx_label_contact* const ordered = lb->d_crec + M;
        const bool on_device = longest <= UMX_CONTACT_DEVICE_SORT_MAX;
        hipLaunchKernelGGL(contact_scatter_kernel, dim3(per_thread_grid((long long)entries)), dim3(kPixThreads), 0, s, lb->d_ckeys, lb->d_cedges,
                           (long long)entries, start, rows, scattered);
        if (on_device)
            hipLaunchKernelGGL(contact_rank_kernel, dim3(per_thread_grid(M)), dim3(kPixThreads), 0, s, scattered, M, start, ordered);
        L_HIP(lb, hipGetLastError());
        L_HIP(lb, hipEventRecord(lb->ev[2], s));
        L_HIP(lb, hipMemcpyAsync(out, on_device ? ordered : scattered, (size_t)M * sizeof(umx_label_contact), hipMemcpyDeviceToHost, s));
        L_HIP(lb, hipEventRecord(lb->ev[3], s));
        L_HIP(lb, hipStreamSynchronize(s));
        if (!on_device) contact_sort_rows(out, M);
        lb->cstats.ordered_by = on_device ? UMX_CONTACT_ORDER_DEVICE : UMX_CONTACT_ORDER_HOST;
    } else {
        L_HIP(lb, hipEventRecord(lb->ev[2], s));
        L_HIP(lb, hipEventRecord(lb->ev[3], s));
        L_HIP(lb, hipStreamSynchronize(s));
    }
    for (int k = 0; k < 2; ++k) {
        float f = 0.f;
        if (hipEventElapsedTime(&f, lb->ev[k + 1], lb->ev[k + 2]) == hipSuccess) lb->cms[k] = f;
    }
    std::string gmsg;
    if ((rc = arena_check(lb->mem, &gmsg)) != UMX_OK) return lfail(lb, rc, "%s", gmsg.c_str());
    if (refused)
        return lfail(lb, UMX_ERR_INVALID, "out holds %lld records: %lld contacts need as many", out ? cap : 0ll, M);
    return UMX_OK;
}

}  // namespace

}  // namespace umx

using namespace umx;

extern "C" {

int umx_label_contact_check(int H, int W, int64_t n_objects, int reach, char* msg, size_t cap) {
    char buf[200] = "";
    contact_check_message(H, W, (long long)n_objects, reach, buf, sizeof buf);
    if (msg && cap) snprintf(msg, cap, "%s", buf);
    return buf[0] ? UMX_ERR_INVALID : UMX_OK;
}

int umx_labeler_contacts(umx_labeler* lb, int H, int W, int reach, umx_label_contact* out, int64_t cap, int64_t* m) {
    if (!lb) return lfail(nullptr, UMX_ERR_INVALID, "null labeler");
    char msg[200];
    if (umx_label_contact_check(H, W, 0, reach, msg, sizeof msg) != UMX_OK) return lfail(lb, UMX_ERR_INVALID, "%s", msg);
    if (lb->res_why) return lfail(lb, UMX_ERR_INVALID, "umx_labeler_contacts has no labels to take the contacts of: %s", lb->res_why);
    if (H != lb->res_H || W != lb->res_W)
        return lfail(lb, UMX_ERR_INVALID, "the call names %d x %d and the labels of the last run are %d x %d", H, W, lb->res_H, lb->res_W);
    if (cap < 0 || (!out && cap > 0)) return lfail(lb, UMX_ERR_INVALID, "out is %s and holds %lld records", out ? "set" : "null", (long long)cap);
    return contacts_any(lb, lb->d_P, lb->res_N, H, W, reach, out, cap, m);
}

int umx_labeler_contacts_dev(umx_labeler* lb, const int32_t* labels_dev, int64_t n_objects, int H, int W, int reach,
                             umx_label_contact* out_host, int64_t cap, int64_t* m) {
    if (!lb) return lfail(nullptr, UMX_ERR_INVALID, "null labeler");
    char msg[200];
    if (umx_label_contact_check(H, W, n_objects, reach, msg, sizeof msg) != UMX_OK) return lfail(lb, UMX_ERR_INVALID, "%s", msg);
    if (!labels_dev) return lfail(lb, UMX_ERR_INVALID, "null labels");
    if (cap < 0 || (!out_host && cap > 0))
        return lfail(lb, UMX_ERR_INVALID, "out_host is %s and holds %lld records", out_host ? "set" : "null", (long long)cap);
    return contacts_any(lb, labels_dev, n_objects, H, W, reach, out_host, cap, m);
}

int umx_labeler_contacts_last_ms(const umx_labeler* lb, double* kernel_ms, double* download_ms) {
    if (!lb) return lfail(nullptr, UMX_ERR_INVALID, "null labeler");
    if (kernel_ms) *kernel_ms = lb->cms[0];
    if (download_ms) *download_ms = lb->cms[1];
    return UMX_OK;
}

int umx_labeler_contacts_last_stats(const umx_labeler* lb, umx_label_contact_stats* stats) {
    if (!lb || !stats) return lfail(nullptr, UMX_ERR_INVALID, lb ? "null stats" : "null labeler");
    *stats = lb->cstats;
    return UMX_OK;
}

}  // extern "C"
