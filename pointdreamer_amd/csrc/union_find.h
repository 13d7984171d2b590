// The lock-free union-find of mesh_components.hip (connected components of a face list) and mesh_clean.hip (classes of close vertices): the device
// functions of one walk and one union.  parent[v] <= v at every moment, and every value parent[v] ever holds is v or a vertex connected to v, so the
// forest is acyclic whatever the threads' order, every walk goes to strictly smaller indices, and the one root a class ends with is its smallest
// index.  parent[] is shared between workgroups on different XCDs while unions run, so every access here is an agent-scope atomic (relaxed: an
// ancestor is all a walk needs).  No thread waits for another; every loop spends a budget of the caller's that strictly decreasing walks cannot
// use up.  Internal linkage: each including unit gets its own copy.
#pragma once
#include "common.h"

namespace pdhip {
namespace {

__device__ __forceinline__ int ld_agent(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void st_agent(int* p, int v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// representative of x; halves the path on the way (parent[prev] = its grandparent, an ancestor and < prev).  -1: the budget ran out
__device__ __forceinline__ int find_root(int* parent, int x, long long& budget) {
    int cur = ld_agent(parent + x);
    if (cur == x) return x;
    int prev = x, next = ld_agent(parent + cur);
    while (next < cur) {
        if (--budget < 0) return -1;
        st_agent(parent + prev, next);
        prev = cur; cur = next; next = ld_agent(parent + cur);
    }
    return cur;
}

// one component for the trees of ra and rb (representatives when they were found).  The CAS hooks a vertex that is its own parent below a
// smaller vertex of the other tree (a root or not: either keeps parent[v] <= v); if it finds the vertex hooked already, the walk goes on
// from the parent it read (< hi).  Returns the smaller representative, -1 when the budget ran out
__device__ __forceinline__ int unite(int* parent, int ra, int rb, long long& budget) {
    while (ra >= 0 && rb >= 0 && ra != rb) {
        if (--budget < 0) return -1;
        const int hi = ra > rb ? ra : rb, lo = ra > rb ? rb : ra;
        int seen = hi;
        if (__hip_atomic_compare_exchange_strong(parent + hi, &seen, lo, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) return lo;
        ra = find_root(parent, seen, budget);
        rb = lo;
    }
    return (ra < 0 || rb < 0) ? -1 : ra;
}

}  // namespace
}  // namespace pdhip
