// What two or more of the mesh units (uv_atlas.hip, neighbor_mesh.hip, simplify_mesh.hip, mesh_components.hip, mesh_smooth.hip, mesh_clean.hip)
// would otherwise each write out: the size limits, the small per-lane tests, the pair key, the heads of sorted runs, the host's read of an
// entry's status words.  Internal linkage, like radix_sort.h, which it includes: each including unit gets its own copy.
#pragma once
#include "radix_sort.h"

namespace pdhip {
namespace {

constexpr int MESH_MAX_V = 1 << 26, MESH_MAX_F = 1 << 23;          // vertices and faces the mesh entries take (pdhip_knn_points' point limit; 3 F < 2^31)

// the active lanes of a wave add one each: one atomic per wave.  Every lane of the wave calls this
__device__ __forceinline__ void wave_count(int32_t* p, bool pred, int lane) {
    const unsigned long long m = __ballot(pred);
    if (lane == 0 && m) atomicAdd(p, __popcll(m));
}

__device__ __forceinline__ bool finite3(float x, float y, float z) {
    return fabsf(x) <= 3.402823466e38f && fabsf(y) <= 3.402823466e38f && fabsf(z) <= 3.402823466e38f;
}

// a is an index into a table of n entries
__device__ __forceinline__ bool index_ok(int64_t a, int n) { return a >= 0 && a < (int64_t)n; }

// the ordered pair (a, b) of indices below n as one sort key, a major; which end a caller puts first is its own choice
__device__ __forceinline__ uint64_t pair_key(uint64_t a, uint64_t b, int n) { return a * (uint64_t)n + b; }
__device__ __forceinline__ uint64_t pair_first(uint64_t key, int n) { return key / (uint64_t)n; }
__device__ __forceinline__ uint64_t pair_second(uint64_t key, int n) { return key % (uint64_t)n; }

// flag[i] = 1 for the first entry of every run of equal sorted keys among the first `live` of n, 0 elsewhere; live = *limit (a count the
// device holds), or n when limit is null.  Entries equal to `none` start no run (~0ull: no key is the sentinel).  A template, like k_scan, so
// that only the units that launch it carry a copy
template <class K>
__global__ void k_run_heads(const K* __restrict__ keys, int n, const int* __restrict__ limit, K none, int* __restrict__ flag) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int live = limit ? *limit : n;
    flag[i] = (i < live && keys[i] != none && (i == 0 || keys[i] != keys[i - 1])) ? 1 : 0;
}

// the one read of an entry's status words: n words to the host, and the stream synchronised
static int read_words(const int* dev, int* host, int n, hipStream_t s) {
    PD_HIP(hipMemcpyAsync(host, dev, (size_t)n * sizeof(int), hipMemcpyDeviceToHost, s));
    PD_HIP(hipStreamSynchronize(s));
    return PDHIP_OK;
}

}  // namespace
}  // namespace pdhip
