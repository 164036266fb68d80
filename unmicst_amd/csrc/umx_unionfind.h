// Union-find in an int32 parent plane, shared by the per-sample labelling (umx_trainset_border.hip) and the whole-slide labelling
// (umx_label.hip).  An object pixel holds a link: the flat index of a pixel of its component that is no larger than its own; a pixel
// that holds its own index (or, on the way there, any value >= its index) is a root; every other pixel holds -1.  Links only ever
// decrease, so a tree's root is the least index the unions have reached: the component's first pixel in raster order in the end.
#pragma once
#include <hip/hip_runtime.h>

namespace umx {

// The parent plane is read and written through L2 only (relaxed, agent scope): the unions below change it with atomicMin, which
// executes in L2, so a copy of a line in the CU's L1 could be stale inside the kernel.
__device__ inline int parent_load(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ inline void parent_store(int* p, int v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// The root of object pixel i.  Bound: a link of a non-root points at a strictly smaller index, so the walk takes at most i steps; a
// value that is not such a link (>= i: the root; negative: never on an object pixel) ends it.
__device__ inline int find_root(const int* P, int i) {
    for (;;) {
        const int p = parent_load(P + i);
        if (p >= i || p < 0) return i;
        i = p;
    }
}

// Merge the trees of a and b: the larger root is hung under the smaller one with atomicMin.  When the larger one stopped being a root
// in between (old != a), its link now points at min(old, b) and the pair (old, b) is still to be merged.  Bound: a retry only happens
// with old < a, so the larger index of the pair strictly decreases from retry to retry: at most max(a, b) retries.
__device__ inline void union_trees(int* P, int a, int b) {
    for (;;) {
        a = find_root(P, a);
        b = find_root(P, b);
        if (a == b) return;
        if (a < b) { const int t = a; a = b; b = t; }
        const int old = atomicMin(P + a, b);
        if (old == a) return;
        a = old;
    }
}

}  // namespace umx
