// libumx label mask, hulls: the host arithmetic of umx_label_hull.hip that needs no device -- the limits of a call, the second limit
// on E (the rows of all labels' boxes) and the sizes of the buffers that E and N give, each with its overflow check.  Plain C++ on
// include/umx.h alone, so that tools/hull_host_check.cpp drives it under the host sanitizers without a HIP runtime.
#pragma once

#include <climits>
#include <cstddef>
#include <cstdio>

#include "../../include/umx.h"

namespace umx {

// umx_label_hull_check without the C linkage: "" into buf when the call is accepted, else the reason
inline void hull_check_message(int H, int W, long long n_objects, char* buf, size_t cap) {
    if (!buf || !cap) return;
    buf[0] = 0;
    if (H < 1 || W < 1) snprintf(buf, cap, "the image is %d x %d: both sides must be at least 1", H, W);
    else if (H > UMX_HULL_MAX_SIDE || W > UMX_HULL_MAX_SIDE)
        snprintf(buf, cap, "the image is %d x %d: a side may be at most %d, so that a cross product of two corner differences stays below 2^33",
                 H, W, UMX_HULL_MAX_SIDE);
    else if ((long long)H * W > INT_MAX)
        snprintf(buf, cap, "the image is %d x %d: a flat pixel index is an int32, so H * W may be at most %d", H, W, INT_MAX);
    else if (n_objects < 0 || n_objects > INT_MAX)
        snprintf(buf, cap, "n_objects is %lld: a label is an int32, so 0..%d objects", n_objects, INT_MAX);
}

// E as the device summed it, against what an accepted call can give and against the limit: "" when the call goes on, else the reason.
// E <= N * H holds for any labels (a box is at most H rows high); a sum outside 0 .. N * H is the device's error, not the caller's.
inline void hull_rows_message(long long E, long long n_objects, int H, char* buf, size_t cap) {
    if (!buf || !cap) return;
    buf[0] = 0;
    if (E < 0 || E > n_objects * (long long)H)                       // (n_objects <= 2^31 - 1, H <= 2^16: below 2^47)
        snprintf(buf, cap, "the row-range pass summed %lld box rows for %lld labels on %d rows", E, n_objects, H);
    else if (E > (long long)UMX_HULL_MAX_ROWS)
        snprintf(buf, cap, "the boxes of the labels have %lld rows in all and UMX_HULL_MAX_ROWS is %lld: the labels lie in far-apart pieces "
                           "and the row entries would take %lld bytes", E, (long long)UMX_HULL_MAX_ROWS, 8 * E);
}

// blocks of `block` labels that cover n_objects (>= 0) labels
inline size_t hull_label_blocks(long long n_objects, int block) { return (size_t)((n_objects + block - 1) / block); }

// int32 words of the row entries: the least x and the largest x + 1 of every row of every box.  E <= UMX_HULL_MAX_ROWS: at most 2^29.
inline size_t hull_row_words(long long E) { return 2 * (size_t)E; }

// the scratch vertex area: a hull has at most 2 * rows + 2 vertices (two pixels on a diagonal attain it, and so do rows that step in
// convexly on both sides) and a box at least as many rows as the label has, so label j's place begins at 2 * (offset[j] + j - 1) and
// 2 * (E + N) places hold them all.  At most 2^29 + 2^32.
inline size_t hull_scratch_vertices(long long E, long long n_objects) { return 2 * ((size_t)E + (size_t)n_objects); }

// 64-bit words of the per-label buffer: an offset per label, a sum per block, and kWords words the host reads
inline size_t hull_offset_words(long long n_objects, int block, int words) {
    return (size_t)n_objects + hull_label_blocks(n_objects, block) + (size_t)words;
}

}  // namespace umx
