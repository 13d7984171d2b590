// The lock-free union-find of mesh_components.hip (connected components of a face list, over the vertices), mesh_clean.hip (classes of close
// vertices) and uv_atlas.hip (charts: components of equally labelled faces, over the faces): one walk, one union, one read-only walk, and the
// identity forest.  parent[v] <= v at every moment, and every value parent[v] ever holds is v or a vertex connected to v, so the forest is
// acyclic whatever the threads' order, every walk goes to strictly smaller indices, and the one root a class ends with is its smallest index:
// the partition AND its roots are functions of the united pairs alone.  parent[] is shared between workgroups on different XCDs while unions
// run, so find_root and unite access it by agent-scope atomics (relaxed: an ancestor is all a walk needs).  No thread waits for another;
// every loop spends a budget of the caller's that strictly decreasing walks cannot use up (a caller that sees -1 reports it: the forest is not
// the one described here).  Internal linkage: each including unit gets its own copy; tests/test_gpu_prims.py runs the copy in prims_debug.hip.
#pragma once
#include "common.h"

namespace pdhip {
namespace {

__device__ __forceinline__ int ld_agent(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void st_agent(int* p, int v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

__global__ void k_uf_identity(int* __restrict__ parent, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) parent[i] = i;
}

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

// the root of v in a forest that an EARLIER launch finished, or -1 when `steps` ran out (a strictly decreasing walk from v has at most v
// steps).  Plain loads suffice across a kernel boundary: the launch that wrote parent[] has completed, and a launch that rewrites it while it
// walks (k_mc_compress) stores only ancestors, so whichever of the two values a thread reads, it is an ancestor of v.
__device__ __forceinline__ int walk_root(const int* parent, int v, int& steps) {
    int r = v;
    for (int p = parent[r]; p < r; p = parent[r]) {
        r = p;
        if (--steps < 0) return -1;
    }
    return r;
}

// ---- the parity variant (mesh_orient.hip: patches of faces across manifold edges, each edge saying whether its two faces agree).  One word per
// node: parent << 1 | parity, parity = the node's bit relative to its parent; word[v] >> 1 <= v at every moment, as above, so the partition and the
// roots are again functions of the united pairs alone.  A hook joins two DIFFERENT trees, so the hooks form a spanning forest, and every word
// ever stored is the XOR of forest relations along a path: a relation the forest implies.  Where the pairs' parities are consistent (a 2-colouring
// exists) every spanning forest implies the same relations, so rel[] (the parity to the root) does not depend on the threads' order either.  A pair
// whose ends already share a root is NOT examined here, consistent or not: a caller re-checks every pair in a later launch (rel[a] ^ rel[b] != e in
// any spanning forest of a component that has no 2-colouring, in none of one that has), so that flag is deterministic too.
__global__ void k_ufp_identity(int* __restrict__ word, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) word[i] = i << 1;
}

// representative of x, par = the parity of x relative to it; halves the path on the way: word[prev] = (its grandparent, the XOR of the two
// parities), one 32-bit store.  -1: the budget ran out
__device__ __forceinline__ int find_root_parity(int* word, int x, int& par, long long& budget) {
    const int wx = ld_agent(word + x);
    par = 0;
    if ((wx >> 1) == x) return x;
    int prev = x, pprev = wx & 1, cur = wx >> 1, acc = 0;          // pprev: prev -> cur; acc: x -> prev
    int wc = ld_agent(word + cur);
    while ((wc >> 1) < cur) {
        if (--budget < 0) return -1;
        const int next = wc >> 1, pc = wc & 1;
        st_agent(word + prev, (next << 1) | (pprev ^ pc));
        acc ^= pprev;
        prev = cur; pprev = pc; cur = next;
        wc = ld_agent(word + cur);
    }
    par = acc ^ pprev;
    return cur;
}

// one component for the trees of ra and rb, q = the parity of ra relative to rb (for nodes a, b with parities pa, pb to ra, rb and an edge that
// says rel[a] ^ rel[b] == e: q = pa ^ pb ^ e).  The CAS hooks a node that is its own parent below the smaller one with the parity between the two;
// if it finds the node hooked already, it goes on from that node's root with the parity carried along.  Returns the smaller representative, -1
// when the budget ran out.  Two nodes that turn out to share a root end the loop whatever q says (the header above)
__device__ __forceinline__ int unite_parity(int* word, int ra, int rb, int q, long long& budget) {
    while (ra >= 0 && rb >= 0 && ra != rb) {
        if (--budget < 0) return -1;
        const int hi = ra > rb ? ra : rb, lo = ra > rb ? rb : ra;
        int seen = hi << 1;
        if (__hip_atomic_compare_exchange_strong(word + hi, &seen, (lo << 1) | q, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) return lo;
        int ps;
        ra = find_root_parity(word, seen >> 1, ps, budget);        // hi -> its root: (seen & 1) ^ ps
        q ^= (seen & 1) ^ ps;
        rb = lo;
    }
    return (ra < 0 || rb < 0) ? -1 : ra;
}

// the root of v in a forest that an EARLIER launch finished and par = the parity of v relative to it, read-only; -1 when `steps` ran out
__device__ __forceinline__ int walk_root_parity(const int* word, int v, int& par, int& steps) {
    int r = v;
    par = 0;
    for (int w = word[r]; (w >> 1) < r; w = word[r]) {
        par ^= w & 1;
        r = w >> 1;
        if (--steps < 0) return -1;
    }
    return r;
}

}  // namespace
}  // namespace pdhip
