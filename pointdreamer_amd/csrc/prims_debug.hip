// Test-only entries onto the shared device primitives: the radix sort, the one-workgroup scan and the tiled scans of radix_sort.h, and the sort
// half of cell_list.h (k_cell_keys, k_cell_starts, sort_by_cell).  include/pdhip.h has the contracts; tests/test_gpu_prims.py holds each of them
// to an exact numpy reference at the tile edges, tests/test_prims_cpu.py the references, the size query and the refusals.  Nothing the product
// calls.
//
// Every kernel of the two headers has internal linkage, so each including unit carries a copy of its own, and no test can run the copy inside
// uv_atlas.hip or knn.hip.  What the tests run is THIS unit's copy: compiled from the same source with the same flags (GEO_SRC of the Makefile)
// as every consumer's.  The unit adds no kernel of its own except the key functor below, which k_cell_keys instantiates.
#include "cell_list.h"

namespace pdhip {
namespace {

constexpr int MAX_N = 1 << 26, MAX_NC = 1 << 26;                   // the limits of the neighbouring entries (pdhip_knn_points)

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
