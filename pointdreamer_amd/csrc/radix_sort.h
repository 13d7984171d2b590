// Radix sort (LSD, 8-bit digits, stable) of 64-bit keys with int32 values, a one-workgroup scan and a tiled scan over many
// workgroups (both templated on the element type): shared by the geometry units that sort or scan on the device.  Through cell_list.h: the
// cell keys of surface_recon.hip (and its vertex / triangle offsets), cloud_metrics.hip, occupancy.hip, mesh_distance.hip, subsample.hip,
// knn.hip and mesh_clean.hip (and its face triples).  Through mesh_common.h: uv_atlas.hip (edge keys, packing order, UV entries),
// neighbor_mesh.hip (edge and pair keys), simplify_mesh.hip (directed-edge keys, adjacency / winner / face offsets), mesh_components.hip (root
// and compaction offsets); mesh_smooth.hip includes it that way and launches none of it.  Directly: sample_mesh.hip (the uint64 CDF).  Written
// here because rocPRIM's sort carries scratch on gfx950.  Every kernel has internal linkage: each including unit gets its own copy.
// tests/test_gpu_prims.py holds the sort and the scans to exact references at the tile edges, through the copy in prims_debug.hip.
#pragma once
#include "common.h"

namespace pdhip {
namespace {

constexpr int RS_T = 256, RS_ITEMS = 8, RS_TILE = RS_T * RS_ITEMS;

__global__ __launch_bounds__(RS_T) void k_rs_hist(const uint64_t* __restrict__ keys, int n, int shift, int* __restrict__ hist, int nblk) {
    __shared__ int h[256];
    const int t = threadIdx.x;
    h[t] = 0;
    __syncthreads();
    const int base = blockIdx.x * RS_TILE;
    for (int k = 0; k < RS_ITEMS; ++k) {
        const int i = base + k * RS_T + t;
        if (i < n) atomicAdd(&h[(int)((keys[i] >> shift) & 255ull)], 1);
    }
    __syncthreads();
    hist[t * nblk + blockIdx.x] = h[t];
}

// digit offsets (exclusive scan of hist, digit-major) -> stable scatter: element order = (item round, wave, lane)
__global__ __launch_bounds__(RS_T) void k_rs_scatter(const uint64_t* __restrict__ kin, const int* __restrict__ vin, int n, int shift,
                                                     const int* __restrict__ offs, int nblk, uint64_t* __restrict__ kout,
                                                     int* __restrict__ vout) {
    __shared__ int run[256];
    __shared__ int wc[RS_T / 64][256];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    run[t] = offs[t * nblk + blockIdx.x];
    const int base = blockIdx.x * RS_TILE;
    const unsigned long long lt = (1ull << lane) - 1ull;
    for (int k = 0; k < RS_ITEMS; ++k) {
        const int i = base + k * RS_T + t;
        const bool valid = i < n;
        const uint64_t key = valid ? kin[i] : 0ull;
        const int val = valid ? vin[i] : 0;
        const int d = (int)((key >> shift) & 255ull);
#pragma unroll
        for (int w = 0; w < RS_T / 64; ++w) wc[w][t] = 0;
        __syncthreads();
        unsigned long long peers = __ballot(valid);
#pragma unroll
        for (int b = 0; b < 8; ++b) {
            const bool bit = (d >> b) & 1;
            const unsigned long long bal = __ballot(bit);
            peers &= bit ? bal : ~bal;
        }
        const int rank = __popcll(peers & lt);
        if (valid && rank == 0) wc[wave][d] = __popcll(peers);
        __syncthreads();
        int r = run[t];
#pragma unroll
        for (int w = 0; w < RS_T / 64; ++w) {
            const int c = wc[w][t];
            wc[w][t] = r;
            r += c;
        }
        run[t] = r;
        __syncthreads();
        if (valid) {
            const int pos = wc[wave][d] + rank;
            kout[pos] = key;
            vout[pos] = val;
        }
        __syncthreads();
    }
}

// one workgroup: out[i] = sum of in[0..i] (inclusive) or in[0..i) (exclusive).  T: int (every unit above) or uint64_t (sample_mesh.hip:
// the integer CDF); the launches deduce it from their pointers
constexpr int SC_T = 1024;
template <class T>
__global__ __launch_bounds__(SC_T) void k_scan(const T* __restrict__ in, T* __restrict__ out, int n, int exclusive) {
    __shared__ T part[SC_T];
    const int t = threadIdx.x;
    const int chunk = (n + SC_T - 1) / SC_T;
    const int b = min(n, t * chunk), e = min(n, b + chunk);
    T s = 0;
    for (int i = b; i < e; ++i) s += in[i];
    part[t] = s;
    __syncthreads();
    for (int off = 1; off < SC_T; off <<= 1) {                    // Hillis-Steele inclusive scan of the chunk sums
        const T add = t >= off ? part[t - off] : 0;
        __syncthreads();
        part[t] += add;
        __syncthreads();
    }
    T run = part[t] - s;
    for (int i = b; i < e; ++i) {
        const T x = in[i];
        out[i] = exclusive ? run : run + x;
        run += x;
    }
}

// scan of n elements over many workgroups: tiles of 2048 (their sums scanned by the one-workgroup k_scan), then the offsets added.
// INCL = false: out[i] = in[0] + ... + in[i - 1]; true: ... + in[i]
constexpr int SCB_T = 256, SCB_ITEMS = 8, SCB_TILE = SCB_T * SCB_ITEMS;
template <class T, bool INCL>
__global__ __launch_bounds__(SCB_T) void k_scan_tiles(const T* __restrict__ in, T* __restrict__ out, long long n, T* __restrict__ sums) {
    __shared__ T part[SCB_T];
    const int t = threadIdx.x;
    const long long base = (long long)blockIdx.x * SCB_TILE + (long long)t * SCB_ITEMS;
    T v[SCB_ITEMS];
    T s = 0;
#pragma unroll
    for (int k = 0; k < SCB_ITEMS; ++k) {
        if (!INCL) v[k] = s;
        s += base + k < n ? in[base + k] : 0;
        if (INCL) v[k] = s;
    }
    part[t] = s;
    __syncthreads();
    for (int off = 1; off < SCB_T; off <<= 1) {
        const T add = t >= off ? part[t - off] : 0;
        __syncthreads();
        part[t] += add;
        __syncthreads();
    }
    const T excl = part[t] - s;
#pragma unroll
    for (int k = 0; k < SCB_ITEMS; ++k)
        if (base + k < n) out[base + k] = excl + v[k];
    if (t == SCB_T - 1) sums[blockIdx.x] = part[t];
}
template <class T>
__global__ void k_scan_add(T* __restrict__ out, long long n, const T* __restrict__ offs) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] += offs[i / SCB_TILE];
}
// elements that tsum and toff must each hold for a scan of n elements (what a carve function takes for them)
constexpr size_t scan_tiles(size_t n) { return n / SCB_TILE + 1; }
template <class T, bool INCL>
static void scan_tiled(const T* in, T* out, long long n, T* tsum, T* toff, hipStream_t s) {
    const int nt = cdiv(n, SCB_TILE);
    k_scan_tiles<T, INCL><<<nt, SCB_T, 0, s>>>(in, out, n, tsum);
    k_scan<T><<<1, SC_T, 0, s>>>(tsum, toff, nt, 1);
    k_scan_add<T><<<cdiv(n, 256), 256, 0, s>>>(out, n, toff);
}
// out[i] = in[0] + ... + in[i - 1] for 0 < n <= 2^31 elements whose sum fits a T
template <class T>
static void scan_exclusive(const T* in, T* out, long long n, T* tsum, T* toff, hipStream_t s) { scan_tiled<T, false>(in, out, n, tsum, toff, s); }
// out[i] = in[0] + ... + in[i]
template <class T>
static void scan_inclusive(const T* in, T* out, long long n, T* tsum, T* toff, hipStream_t s) { scan_tiled<T, true>(in, out, n, tsum, toff, s); }

struct SortBufs {
    uint64_t* k[2];
    int* v[2];
    int* hist;
};
static void carve_sort(Carve& c, SortBufs& sb, size_t N) {
    sb.k[0] = c.take<uint64_t>(N); sb.k[1] = c.take<uint64_t>(N); sb.v[0] = c.take<int>(N); sb.v[1] = c.take<int>(N);
    sb.hist = c.take<int>(2 * 256 * (size_t)cdiv((long long)N, RS_TILE));
}

static int bits_for(unsigned long long maxkey) {
    int b = 0;
    while (b < 64 && (maxkey >> b) != 0ull) ++b;
    return b;
}

// sorts keys / values k[0] / v[0] (n > 0 elements), stably, by bits [0, 8 * ceil(bits / 8)): whole 8-bit digits, so the bits of a partial top
// digit above `bits` take part in the order; callers keep their keys < 2^bits.  Bits above the last digit are carried along unread; bits == 0
// sorts nothing.  Returns the index (0 / 1) of the buffer pair holding the result
static int radix_sort(SortBufs& sb, int n, int bits, hipStream_t s) {
    const int nblk = cdiv(n, RS_TILE);
    int cur = 0;
    for (int shift = 0; shift < bits; shift += 8) {
        k_rs_hist<<<nblk, RS_T, 0, s>>>(sb.k[cur], n, shift, sb.hist, nblk);
        k_scan<int><<<1, SC_T, 0, s>>>(sb.hist, sb.hist + 256 * nblk, 256 * nblk, 1);
        k_rs_scatter<<<nblk, RS_T, 0, s>>>(sb.k[cur], sb.v[cur], n, shift, sb.hist + 256 * nblk, nblk, sb.k[cur ^ 1], sb.v[cur ^ 1]);
        cur ^= 1;
    }
    return cur;
}

}  // namespace
}  // namespace pdhip
