// Test-only entries onto the shared device primitives: the radix sort, the one-workgroup scan and the tiled scans of radix_sort.h, the sort
// half of cell_list.h (k_cell_keys, k_cell_starts, sort_by_cell), and the union-find of union_find.h.  include/pdhip.h has the contracts;
// tests/test_gpu_prims.py holds each of them to an exact numpy reference at the tile edges, tests/test_prims_cpu.py the references, the size
// query and the refusals; tests/test_gpu_parity_union.py holds the union-find's parity variant (pdhip_debug_parity_union) to a sequential one.
// Nothing the product calls.
//
// Every kernel of the headers has internal linkage, so each including unit carries a copy of its own, and no test can run the copy inside
// uv_atlas.hip or knn.hip.  What the tests run is THIS unit's copy: compiled from the same source with the same flags (GEO_SRC of the Makefile)
// as every consumer's.  The unit's own kernels are the key functor below, which k_cell_keys instantiates, and the three of the union-find
// entry, which only call the header's device functions the way the product's kernels do.
#include "cell_list.h"
#include "mesh_common.h"
#include "union_find.h"

namespace pdhip {
namespace {

constexpr int MAX_N = 1 << 26, MAX_NC = 1 << 26;                   // the limits of the neighbouring entries (pdhip_knn_points)
constexpr int UF_T = 256;
enum { UF_UNITE = 1, UF_WALK = 2 };                                // pdhip_debug_union_pairs' status: which budget ran out

__global__ void k_ufd_check(const int32_t* __restrict__ pairs, int n_pairs, int n, int32_t* __restrict__ bad) {
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p < n_pairs && !(index_ok(pairs[2 * (size_t)p], n) && index_ok(pairs[2 * (size_t)p + 1], n))) atomicAdd(bad, 1);
}

// one thread per pair, the budget mesh_components.hip gives a face
__global__ __launch_bounds__(UF_T) void k_ufd_unite(const int32_t* __restrict__ pairs, int n_pairs, int n, int* parent, int32_t* __restrict__ status) {
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n_pairs) return;
    long long budget = 2ll * n + 64;
    const int a = pairs[2 * (size_t)p], b = pairs[2 * (size_t)p + 1];
    if (unite(parent, find_root(parent, a, budget), find_root(parent, b, budget), budget) < 0) atomicOr(status, UF_UNITE);
}

__global__ void k_ufd_roots(const int* __restrict__ parent, int n, int32_t* __restrict__ root, int32_t* __restrict__ status) {
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= n) return;
    int steps = n;
    const int r = walk_root(parent, v, steps);
    if (r < 0) atomicOr(status, UF_WALK);
    root[v] = r;
}

// ---- the parity variant: the pairs' check, the unions, the flatten, the re-check of every pair and the spread of the flag over the classes
__global__ void k_ufp_check(const int32_t* __restrict__ pairs, const uint8_t* __restrict__ parity, int n_pairs, int n, int32_t* __restrict__ bad) {
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p < n_pairs && !(index_ok(pairs[2 * (size_t)p], n) && index_ok(pairs[2 * (size_t)p + 1], n) && parity[p] <= 1)) atomicAdd(bad, 1);
}

// one thread per pair, the budget mesh_orient.hip gives an edge
__global__ __launch_bounds__(UF_T) void k_ufp_unite(const int32_t* __restrict__ pairs, const uint8_t* __restrict__ parity, int n_pairs, int n, int* word,
                                                    int32_t* __restrict__ status) {
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n_pairs) return;
    long long budget = 2ll * n + 64;
    const int a = pairs[2 * (size_t)p], b = pairs[2 * (size_t)p + 1];
    int pa, pb;
    const int ra = find_root_parity(word, a, pa, budget), rb = find_root_parity(word, b, pb, budget);
    if (unite_parity(word, ra, rb, pa ^ pb ^ (int)parity[p], budget) < 0) atomicOr(status, UF_UNITE);
}

__global__ void k_ufp_roots(const int* __restrict__ word, int n, int32_t* __restrict__ root, uint8_t* __restrict__ rel, uint8_t* __restrict__ conflict,
                            int32_t* __restrict__ status) {
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= n) return;
    int steps = n, par;
    const int r = walk_root_parity(word, v, par, steps);
    if (r < 0) atomicOr(status, UF_WALK);
    root[v] = r;
    rel[v] = (uint8_t)par;
    conflict[v] = 0;
}

// a pair that the relations of the forest contradict flags its class, at the root
__global__ void k_ufp_recheck(const int32_t* __restrict__ pairs, const uint8_t* __restrict__ parity, int n_pairs, const int32_t* __restrict__ root,
                              const uint8_t* __restrict__ rel, uint8_t* __restrict__ conflict, const int32_t* __restrict__ status) {
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n_pairs || *status) return;
    const int a = pairs[2 * (size_t)p], b = pairs[2 * (size_t)p + 1];
    if ((rel[a] ^ rel[b]) != parity[p]) conflict[root[a]] = 1;
}

// (a root keeps its own flag; every other node writes a byte that nobody reads in this launch)
__global__ void k_ufp_spread(const int32_t* __restrict__ root, int n, uint8_t* conflict, const int32_t* __restrict__ status) {
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= n || *status) return;
    const int r = root[v];
    if (r != v && conflict[r]) conflict[v] = 1;
}

// KeyFn of sort_by_cell: the key of point i, read from an array
struct ArrayKey {
    const uint64_t* key;
    __device__ uint64_t operator()(int i) const { return key[i]; }
};

struct PrimsWs {
    SortBufs sb;
    int* cstart;
    void *tsum, *toff;                                             // scan_tiles(n) elements of 8 bytes each: an int scan uses the front half
};
static size_t carve_prims(PrimsWs& w, void* base, int n, int nc) {
    Carve c{static_cast<char*>(base), 0};
    carve_sort(c, w.sb, (size_t)n);
    w.cstart = c.take<int>((size_t)nc + 1);
    w.tsum = c.take<uint64_t>(scan_tiles((size_t)n)); w.toff = c.take<uint64_t>(scan_tiles((size_t)n));
    return c.off + 256;
}
static bool sizes_ok(int n, int nc) { return n >= 1 && n <= MAX_N && nc >= 1 && nc <= MAX_NC; }

template <class T>
static void launch_scan(const void* in, void* out, int n, int mode, int inclusive, const PrimsWs& w, hipStream_t s) {
    const T* i = static_cast<const T*>(in);
    T* o = static_cast<T*>(out);
    if (mode == 0) k_scan<T><<<1, SC_T, 0, s>>>(i, o, n, inclusive ? 0 : 1);
    else if (inclusive) scan_inclusive<T>(i, o, n, static_cast<T*>(w.tsum), static_cast<T*>(w.toff), s);
    else scan_exclusive<T>(i, o, n, static_cast<T*>(w.tsum), static_cast<T*>(w.toff), s);
}

}  // namespace
}  // namespace pdhip

using namespace pdhip;

extern "C" size_t pdhip_debug_prims_workspace_bytes(int n, int nc) {
    if (!sizes_ok(n, nc)) return 0;
    PrimsWs w;
    return carve_prims(w, nullptr, n, nc);
}

extern "C" int pdhip_debug_radix_sort(const uint64_t* keys, const int32_t* vals, int n, int bits, uint64_t* keys_out, int32_t* vals_out, void* ws,
                                      void* stream) {
#define PR_PTR(p) PD_REQUIRE(p, "pdhip_debug_radix_sort: null pointer (" #p ")")
    PR_PTR(keys); PR_PTR(vals); PR_PTR(keys_out); PR_PTR(vals_out); PR_PTR(ws);
#undef PR_PTR
    PD_REQUIRE(n >= 1 && n <= MAX_N, "pdhip_debug_radix_sort: n=%d outside [1, 2^26]", n);
    PD_REQUIRE(bits >= 0 && bits <= 64, "pdhip_debug_radix_sort: bits=%d outside [0, 64]", bits);
    hipStream_t s = as_stream(stream);
    PrimsWs w;
    carve_prims(w, ws, n, 1);
    PD_HIP(hipMemcpyAsync(w.sb.k[0], keys, (size_t)n * sizeof(uint64_t), hipMemcpyDeviceToDevice, s));
    PD_HIP(hipMemcpyAsync(w.sb.v[0], vals, (size_t)n * sizeof(int), hipMemcpyDeviceToDevice, s));
    const int cur = radix_sort(w.sb, n, bits, s);
    PD_LAUNCH_CHECK();
    PD_HIP(hipMemcpyAsync(keys_out, w.sb.k[cur], (size_t)n * sizeof(uint64_t), hipMemcpyDeviceToDevice, s));
    PD_HIP(hipMemcpyAsync(vals_out, w.sb.v[cur], (size_t)n * sizeof(int), hipMemcpyDeviceToDevice, s));
    return PDHIP_OK;
}

extern "C" int pdhip_debug_sort_by_cell(const uint64_t* keys, int n, int nc, uint64_t* keys_out, int32_t* idx_out, int32_t* cstart_out, void* ws,
                                        void* stream) {
#define PR_PTR(p) PD_REQUIRE(p, "pdhip_debug_sort_by_cell: null pointer (" #p ")")
    PR_PTR(keys); PR_PTR(keys_out); PR_PTR(idx_out); PR_PTR(cstart_out); PR_PTR(ws);
#undef PR_PTR
    PD_REQUIRE(n >= 1 && n <= MAX_N, "pdhip_debug_sort_by_cell: n=%d outside [1, 2^26]", n);
    PD_REQUIRE(nc >= 1 && nc <= MAX_NC, "pdhip_debug_sort_by_cell: nc=%d outside [1, 2^26]", nc);
    hipStream_t s = as_stream(stream);
    PrimsWs w;
    carve_prims(w, ws, n, nc);
    const int cur = sort_by_cell(w.sb, n, ArrayKey{keys}, (unsigned long long)nc, w.cstart, s);
    PD_LAUNCH_CHECK();
    PD_HIP(hipMemcpyAsync(keys_out, w.sb.k[cur], (size_t)n * sizeof(uint64_t), hipMemcpyDeviceToDevice, s));
    PD_HIP(hipMemcpyAsync(idx_out, w.sb.v[cur], (size_t)n * sizeof(int), hipMemcpyDeviceToDevice, s));
    PD_HIP(hipMemcpyAsync(cstart_out, w.cstart, ((size_t)nc + 1) * sizeof(int), hipMemcpyDeviceToDevice, s));
    return PDHIP_OK;
}

extern "C" int pdhip_debug_scan(const void* in, void* out, int n, int elem_bytes, int mode, int inclusive, int nc, void* ws, void* stream) {
#define PR_PTR(p) PD_REQUIRE(p, "pdhip_debug_scan: null pointer (" #p ")")
    PR_PTR(in); PR_PTR(out); PR_PTR(ws);
#undef PR_PTR
    PD_REQUIRE(n >= 1 && n <= MAX_N, "pdhip_debug_scan: n=%d outside [1, 2^26]", n);
    PD_REQUIRE(elem_bytes == 4 || elem_bytes == 8, "pdhip_debug_scan: elem_bytes=%d is neither 4 (int) nor 8 (uint64_t)", elem_bytes);
    PD_REQUIRE(mode == 0 || mode == 1, "pdhip_debug_scan: mode=%d is neither 0 (k_scan) nor 1 (tiled)", mode);
    PD_REQUIRE(nc >= 1 && nc <= MAX_NC, "pdhip_debug_scan: nc=%d outside [1, 2^26]", nc);
    hipStream_t s = as_stream(stream);
    PrimsWs w;
    carve_prims(w, ws, n, nc);
    if (elem_bytes == 4) launch_scan<int>(in, out, n, mode, inclusive, w, s);
    else launch_scan<uint64_t>(in, out, n, mode, inclusive, w, s);
    PD_LAUNCH_CHECK();
    return PDHIP_OK;
}

extern "C" int pdhip_debug_union_pairs(const int32_t* pairs, int n_pairs, int n, int32_t* parent, int32_t* root, int32_t* status, void* stream) {
#define PR_PTR(p) PD_REQUIRE(p, "pdhip_debug_union_pairs: null pointer (" #p ")")
    PR_PTR(parent); PR_PTR(root); PR_PTR(status);
#undef PR_PTR
    PD_REQUIRE(n >= 1 && n <= MAX_N, "pdhip_debug_union_pairs: n=%d outside [1, 2^26]", n);
    PD_REQUIRE(n_pairs >= 0 && n_pairs <= MAX_N, "pdhip_debug_union_pairs: n_pairs=%d outside [0, 2^26]", n_pairs);
    PD_REQUIRE(pairs || n_pairs == 0, "pdhip_debug_union_pairs: null pointer (pairs) with n_pairs=%d", n_pairs);
    hipStream_t s = as_stream(stream);
    const int gp = cdiv(n_pairs, UF_T), gn = cdiv(n, UF_T);
    PD_HIP(hipMemsetAsync(status, 0, sizeof(int32_t), s));
    if (n_pairs > 0) {                                              // no index outside [0, n) reaches parent[]: counted before the unions start
        k_ufd_check<<<gp, UF_T, 0, s>>>(pairs, n_pairs, n, status);
        PD_LAUNCH_CHECK();
        int bad = 0;
        const int rc = read_words(status, &bad, 1, s);
        if (rc) return rc;
        PD_REQUIRE(bad == 0, "pdhip_debug_union_pairs: %d pair(s) with an index outside [0, n=%d)", bad, n);
    }
    k_uf_identity<<<gn, UF_T, 0, s>>>(parent, n);
    if (n_pairs > 0) k_ufd_unite<<<gp, UF_T, 0, s>>>(pairs, n_pairs, n, parent, status);
    k_ufd_roots<<<gn, UF_T, 0, s>>>(parent, n, root, status);
    PD_LAUNCH_CHECK();
    return PDHIP_OK;
}

extern "C" int pdhip_debug_parity_union(const int32_t* pairs, const uint8_t* parity, int n_pairs, int n, int32_t* word, int32_t* root, uint8_t* rel,
                                        uint8_t* conflict, int32_t* status, void* stream) {
#define PR_PTR(p) PD_REQUIRE(p, "pdhip_debug_parity_union: null pointer (" #p ")")
    PR_PTR(word); PR_PTR(root); PR_PTR(rel); PR_PTR(conflict); PR_PTR(status);
#undef PR_PTR
    PD_REQUIRE(n >= 1 && n <= MAX_N, "pdhip_debug_parity_union: n=%d outside [1, 2^26]", n);
    PD_REQUIRE(n_pairs >= 0 && n_pairs <= MAX_N, "pdhip_debug_parity_union: n_pairs=%d outside [0, 2^26]", n_pairs);
    PD_REQUIRE((pairs && parity) || n_pairs == 0, "pdhip_debug_parity_union: null pointer (%s) with n_pairs=%d", pairs ? "parity" : "pairs", n_pairs);
    hipStream_t s = as_stream(stream);
    const int gp = cdiv(n_pairs, UF_T), gn = cdiv(n, UF_T);
    PD_HIP(hipMemsetAsync(status, 0, sizeof(int32_t), s));
    if (n_pairs > 0) {                                              // no index outside [0, n) reaches word[]: counted before the unions start
        k_ufp_check<<<gp, UF_T, 0, s>>>(pairs, parity, n_pairs, n, status);
        PD_LAUNCH_CHECK();
        int bad = 0;
        const int rc = read_words(status, &bad, 1, s);
        if (rc) return rc;
        PD_REQUIRE(bad == 0, "pdhip_debug_parity_union: %d pair(s) with an index outside [0, n=%d) or a parity other than 0 and 1", bad, n);
    }
    k_ufp_identity<<<gn, UF_T, 0, s>>>(word, n);
    if (n_pairs > 0) k_ufp_unite<<<gp, UF_T, 0, s>>>(pairs, parity, n_pairs, n, word, status);
    k_ufp_roots<<<gn, UF_T, 0, s>>>(word, n, root, rel, conflict, status);
    if (n_pairs > 0) {
        k_ufp_recheck<<<gp, UF_T, 0, s>>>(pairs, parity, n_pairs, root, rel, conflict, status);
        k_ufp_spread<<<gn, UF_T, 0, s>>>(root, n, conflict, status);
    }
    PD_LAUNCH_CHECK();
    return PDHIP_OK;
}
