// sc_unionfind.h -- the lock-free union-find that dbscan.hip (rule 4, the link launch) and graph.hip (the components)
// share.  Device text, included by both units; each has its own copy.
//
// parent[] only ever holds a smaller-or-equal index of the same component: a root (parent[a] == a) is hung under a
// smaller root with a compare-and-swap, so when the launch ends each component's root is its smallest index whatever
// the order of the atomics was.  Blocks on different XCDs share parent[] inside the launch that unites and their L2s
// are not coherent: EVERY access here is a relaxed agent-scope atomic, none a plain load.  (Behind the kernel boundary
// that follows, parent[] is final and plain loads read it.)
#pragma once

#include <hip/hip_runtime.h>

#define DB_RLX __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT

__device__ __forceinline__ int find_root(int *parent, int a) {
    for (;;) {
        const int p = __hip_atomic_load(&parent[a], DB_RLX);
        if (p == a) return a;
        const int gp = __hip_atomic_load(&parent[p], DB_RLX);
        if (gp != p) (void)__hip_atomic_fetch_min(&parent[a], gp, DB_RLX);  // path halving: a non-root only moves up
        a = p;
    }
}

__device__ __forceinline__ void unite(int *parent, int a, int b) {
    for (;;) {
        a = find_root(parent, a);
        b = find_root(parent, b);
        if (a == b) return;
        if (a < b) { const int t = a; a = b; b = t; }  // a > b: hang a under b
        int expect = a;
        if (__hip_atomic_compare_exchange_strong(&parent[a], &expect, b, __ATOMIC_RELAXED, DB_RLX)) return;
    }
}
