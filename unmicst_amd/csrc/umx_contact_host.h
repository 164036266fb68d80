// libumx label mask, contacts: the host arithmetic of umx_label_contact.hip that needs no device -- the limits of a call, the size of
// the first table, the ordering of a list whose rows the device left unordered.  Plain C++ on include/umx.h alone, so that
// tools/contact_host_check.cpp drives it under the host sanitizers without a HIP runtime.
#pragma once

#include <algorithm>
#include <climits>
#include <cstdio>

#include "../../include/umx.h"

namespace umx {

// umx_label_contact_check without the C linkage: "" into buf when the call is accepted, else the reason
inline void contact_check_message(int H, int W, long long n_objects, int reach, char* buf, size_t cap) {
    if (!buf || !cap) return;
    buf[0] = 0;
    if (H < 1 || W < 1) snprintf(buf, cap, "the image is %d x %d: both sides must be at least 1", H, W);
    else if ((long long)H * W > INT_MAX)
        snprintf(buf, cap, "the image is %d x %d: a flat pixel index is an int32, so H * W may be at most %d", H, W, INT_MAX);
    else if (n_objects < 0 || n_objects > INT_MAX)
        snprintf(buf, cap, "n_objects is %lld: a label is an int32, so 0..%d objects", n_objects, INT_MAX);
    else if (reach < 0 || reach > UMX_CONTACT_MAX_REACH)
        snprintf(buf, cap, "reach is %d: 0 (the labels themselves) or 1..%d levels", reach, UMX_CONTACT_MAX_REACH);
}

// the entries of the table a labeler's first pass on n_objects labels uses: the least power of two that is at least n_objects, inside
// UMX_CONTACT_TABLE_MIN .. UMX_CONTACT_TABLE_MAX
inline size_t contact_first_table(long long n_objects) {
    size_t c = UMX_CONTACT_TABLE_MIN;
    while (c < (size_t)UMX_CONTACT_TABLE_MAX && (long long)c < n_objects) c *= 2;
    return c;
}

// rec[0 .. m): rows of equal a, the rows in ascending order of a (what the scatter leaves) -> every row ordered by b.  The longest
// row is returned.  O(m log longest).
inline long long contact_sort_rows(umx_label_contact* rec, long long m) {
    long long longest = 0;
    for (long long i = 0; i < m;) {
        long long j = i + 1;
        while (j < m && rec[j].a == rec[i].a) ++j;
        std::sort(rec + i, rec + j, [](const umx_label_contact& x, const umx_label_contact& y) { return x.b < y.b; });
        longest = std::max(longest, j - i);
        i = j;
    }
    return longest;
}

}  // namespace umx
