// libumx label mask, relabel: the host part of umx_label_relabel.hip that needs no device -- the limits of a call, the validation of
// `keep` and `pairs`, and the classes and their numbering: a union-find over the N + 1 words
// of `map` itself, with path compression, that leaves map[j] = the new number of label j.  Plain C++ on include/umx.h alone, so that
// tools/relabel_host_check.cpp drives it under the host sanitizers without a HIP runtime.
#pragma once

#include <climits>
#include <cstddef>
#include <cstdint>
#include <cstdio>

#include "../../include/umx.h"

namespace umx {

constexpr long long kRelabelMaxObjects = (long long)INT_MAX - 1;   // map has N + 1 words and an index into it is an int32

// umx_label_relabel_check without the C linkage: "" into buf when the call is accepted, else the reason
inline void relabel_check_message(int H, int W, long long n_objects, long long n_pairs, char* buf, size_t cap) {
    if (!buf || !cap) return;
    buf[0] = 0;
    if (H < 1 || W < 1) snprintf(buf, cap, "the image is %d x %d: both sides must be at least 1", H, W);
    else if ((long long)H * W > INT_MAX)
        snprintf(buf, cap, "the image is %d x %d: a flat pixel index is an int32, so H * W may be at most %d", H, W, INT_MAX);
    else if (n_objects < 0 || n_objects > kRelabelMaxObjects)
        snprintf(buf, cap, "n_objects is %lld: the map has n_objects + 1 int32 words, so 0..%lld objects", n_objects, kRelabelMaxObjects);
    else if (n_pairs < 0 || n_pairs > (long long)UMX_RELABEL_MAX_PAIRS)
        snprintf(buf, cap, "n_pairs is %lld: 0..%lld pairs (UMX_RELABEL_MAX_PAIRS)", n_pairs, (long long)UMX_RELABEL_MAX_PAIRS);
}

// the root of j's tree: the least member of its class (a parent is always below its child).  The walk is compressed in a second pass,
// so a chain (1,2),(2,3),... costs its length once and one step afterwards.
inline int32_t relabel_find(int32_t* parent, int32_t j) {
    int32_t r = j;
    while (parent[r] != r) r = parent[r];
    while (parent[j] != r) {
        const int32_t up = parent[j];
        parent[j] = r;
        j = up;
    }
    return r;
}

// Steps 29 and 30.  keep: N bytes or null (keep all); pairs: 2 * M int32 (a, b), may be null when M is 0; map: N + 1 words, or null
// when the arguments are only to be validated (then *n_new is not written and nothing of size N is touched but keep at the labels the
// pairs name).  UMX_OK, or UMX_ERR_INVALID with the reason in buf; a refused call may have written map.
inline int relabel_map(long long N, const uint8_t* keep, const int32_t* pairs, long long M, int32_t* map, long long* n_new, char* buf,
                       size_t cap) {
    char local[8];
    if (!buf || !cap) { buf = local; cap = sizeof local; }
    relabel_check_message(1, 1, N, M, buf, cap);
    if (buf[0]) return UMX_ERR_INVALID;
    if (M > 0 && !pairs) {
        snprintf(buf, cap, "pairs is null and n_pairs is %lld", M);
        return UMX_ERR_INVALID;
    }
    for (long long k = 0; k < M; ++k) {
        const int32_t a = pairs[2 * k], b = pairs[2 * k + 1];
        if (a < 1 || a > N || b < 1 || b > N) {
            snprintf(buf, cap, "pair %lld is (%d, %d): the labels are 1..%lld", k, a, b, N);
            return UMX_ERR_INVALID;
        }
        if (keep && (!keep[a - 1] || !keep[b - 1])) {
            snprintf(buf, cap, "pair %lld is (%d, %d) and keep drops label %d: a label is dropped or merged, not both", k, a, b,
                     !keep[a - 1] ? a : b);
            return UMX_ERR_INVALID;
        }
    }
    if (!map) return UMX_OK;
    for (long long j = 0; j <= N; ++j) map[j] = (int32_t)j;
    for (long long k = 0; k < M; ++k) {
        const int32_t ra = relabel_find(map, pairs[2 * k]), rb = relabel_find(map, pairs[2 * k + 1]);
        if (ra < rb) map[rb] = ra;                        // the lesser root stays the root: it is the class's least member
        else if (rb < ra) map[ra] = rb;
    }
    // ascending: a root takes the next number (0 when dropped: its class is itself alone); any other label has a parent below it,
    // which already holds its class's number
    long long n = 0;
    for (long long j = 1; j <= N; ++j) {
        const int32_t p = map[j];
        if (p == j) map[j] = !keep || keep[j - 1] ? (int32_t)++n : 0;
        else map[j] = map[p];
    }
    if (n_new) *n_new = n;
    return UMX_OK;
}

}  // namespace umx
