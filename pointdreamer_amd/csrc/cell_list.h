// Point cell list: the box a uniform grid is laid over, the points sorted by cell key (radix_sort.h) with cstart[c] = first sorted point whose
// key is >= c, the sorted (x, y, z, index) copy, the cube of cells a scan visits.  Shared by surface_recon.hip (f32 3-D grid), cloud_metrics.hip
// (f64 3-D grid) and occupancy.hip (f64 xy grid); each keeps its grid struct, the key functor that repeats its cell arithmetic operation for
// operation, its face bound and its refusal messages.  Internal linkage: each including unit gets its own copy.  Zero scratch.
#pragma once
#include "radix_sort.h"
#include <string.h>

namespace pdhip {
namespace {

constexpr int CL_T = 256;

// ---------------------------------------------------------------------------------------------------------------------------
// the box.  faces == nullptr: the n points of P.  Otherwise: the n faces over the Vn vertices of P; a face with an index outside [0, Vn) is counted
// in box[BOX_IDX] and none of its vertices is read.  box[BOX_MIN ..] / box[BOX_MAX ..] = min / max of the finite coordinates as order-preserving
// keys, box[BOX_BAD] = points / referenced vertices (counted per reference) with a non-finite coordinate.  send_box == 0: only the two counts are
// sent (atomics on one address are served one after the other; the launches keep the grid small for the same reason)
enum { BOX_MIN = 0, BOX_MAX = 3, BOX_BAD = 6, BOX_IDX = 7, BOX_WORDS = 8 };
__global__ __launch_bounds__(CL_T) void k_point_box(const float* __restrict__ P, int Vn, const int64_t* __restrict__ faces, int n, int send_box,
                                                    uint32_t* __restrict__ box) {
    __shared__ uint32_t sh[BOX_WORDS];
    const int t = threadIdx.x;
    if (t < BOX_WORDS) sh[t] = t < BOX_MAX ? 0xffffffffu : 0u;
    __syncthreads();
    uint32_t mn0 = 0xffffffffu, mn1 = 0xffffffffu, mn2 = 0xffffffffu, mx0 = 0u, mx1 = 0u, mx2 = 0u, bad = 0u, badidx = 0u;
    for (long long i = (long long)blockIdx.x * CL_T + t; i < n; i += (long long)gridDim.x * CL_T) {
        long long v[3] = {i, 0, 0};
        int nv = 1;
        if (faces != nullptr) {
            v[0] = faces[3 * i]; v[1] = faces[3 * i + 1]; v[2] = faces[3 * i + 2];
            nv = 3;
            if (v[0] < 0 || v[0] >= Vn || v[1] < 0 || v[1] >= Vn || v[2] < 0 || v[2] >= Vn) { ++badidx; continue; }
        }
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            if (k >= nv) break;
            const float x = P[3 * v[k]], y = P[3 * v[k] + 1], z = P[3 * v[k] + 2];
            if (!(fabsf(x) <= 3.4028234e38f) || !(fabsf(y) <= 3.4028234e38f) || !(fabsf(z) <= 3.4028234e38f)) { ++bad; continue; }
            const uint32_t a = f2ord(x), b = f2ord(y), c = f2ord(z);
            mn0 = min(mn0, a); mn1 = min(mn1, b); mn2 = min(mn2, c);
            mx0 = max(mx0, a); mx1 = max(mx1, b); mx2 = max(mx2, c);
        }
    }
    for (int off = 32; off > 0; off >>= 1) {                       // one LDS atomic per wave and word, not one per thread
        mn0 = min(mn0, (uint32_t)__shfl_xor((int)mn0, off)); mn1 = min(mn1, (uint32_t)__shfl_xor((int)mn1, off));
        mn2 = min(mn2, (uint32_t)__shfl_xor((int)mn2, off)); mx0 = max(mx0, (uint32_t)__shfl_xor((int)mx0, off));
        mx1 = max(mx1, (uint32_t)__shfl_xor((int)mx1, off)); mx2 = max(mx2, (uint32_t)__shfl_xor((int)mx2, off));
        bad += (uint32_t)__shfl_xor((int)bad, off);
        badidx += (uint32_t)__shfl_xor((int)badidx, off);
    }
    if ((t & 63) == 0) {
        atomicMin(&sh[0], mn0); atomicMin(&sh[1], mn1); atomicMin(&sh[2], mn2);
        atomicMax(&sh[3], mx0); atomicMax(&sh[4], mx1); atomicMax(&sh[5], mx2);
        if (bad) atomicAdd(&sh[BOX_BAD], bad);
        if (badidx) atomicAdd(&sh[BOX_IDX], badidx);
    }
    __syncthreads();
    if (t < BOX_MAX) { if (send_box) atomicMin(&box[t], sh[t]); }
    else if (t < BOX_BAD) { if (send_box) atomicMax(&box[t], sh[t]); }
    else if (t < BOX_WORDS && sh[t]) atomicAdd(&box[t], sh[t]);
}

// a box on the host; mn / mx mean nothing for a box that was not sent or that no finite point reached
struct HostBox {
    double mn[3], mx[3];
    uint32_t bad, bad_index;
};

static double host_ord2f(uint32_t u) {
    const uint32_t b = (u & 0x80000000u) ? (u & 0x7fffffffu) : ~u;
    float f;
    memcpy(&f, &b, sizeof(f));
    return (double)f;
}

// clears the nwords >= nboxes * BOX_WORDS words at `words` (the boxes, then the counters a unit keeps behind them) and primes the mins
static int clear_boxes(uint32_t* words, int nboxes, int nwords, hipStream_t s) {
    PD_HIP(hipMemsetAsync(words, 0, nwords * sizeof(uint32_t), s));
    for (int b = 0; b < nboxes; ++b) PD_HIP(hipMemsetAsync(words + b * BOX_WORDS + BOX_MIN, 0xff, 3 * sizeof(uint32_t), s));
    return PDHIP_OK;
}

// one small read that synchronises the stream
template <int NB>
static int read_boxes(const uint32_t* words, HostBox (&box)[NB], hipStream_t s) {
    uint32_t h[NB * BOX_WORDS];
    PD_HIP(hipMemcpyAsync(h, words, sizeof(h), hipMemcpyDeviceToHost, s));
    PD_HIP(hipStreamSynchronize(s));
    for (int b = 0; b < NB; ++b) {
        const uint32_t* w = h + b * BOX_WORDS;
        for (int a = 0; a < 3; ++a) {
            box[b].mn[a] = host_ord2f(w[BOX_MIN + a]);
            box[b].mx[a] = host_ord2f(w[BOX_MAX + a]);
        }
        box[b].bad = w[BOX_BAD];
        box[b].bad_index = w[BOX_IDX];
    }
    return PDHIP_OK;
}

// ---------------------------------------------------------------------------------------------------------------------------
// the sort.  KeyFn: a small struct passed by value with __device__ uint64_t operator()(int i) const = the cell key of point i
template <class KeyFn>
__global__ void k_cell_keys(int n, KeyFn f, uint64_t* __restrict__ key, int* __restrict__ val) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    key[i] = f(i);
    val[i] = i;
}

// cstart[c] = first sorted position whose key is >= c, c = 0 .. nc (one thread per cell: a binary search in the sorted keys).  The points of
// the cells c0 .. c1 are the ONE run cstart[c0] .. cstart[c1 + 1] of the sorted array; points with a key >= nc start at cstart[nc]
__global__ void k_cell_starts(const uint64_t* __restrict__ key, int n, int* __restrict__ cstart, int nc) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c > nc) return;
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (key[mid] < (uint64_t)c) lo = mid + 1; else hi = mid;
    }
    cstart[c] = lo;
}

// sorted points as (x, y, z, index)
__global__ void k_gather_xyzi(const int* __restrict__ val, const float* __restrict__ P, int n, float4* __restrict__ sp) {
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    const int i = val[p];
    sp[p] = make_float4(P[3 * (size_t)i], P[3 * (size_t)i + 1], P[3 * (size_t)i + 2], __int_as_float(i));
}

// keys f(0 .. n) < 2^bits_for(nc) into sb, sorted; cstart != nullptr: cstart[0 .. nc] as well.  Returns the index (0 / 1) of the buffer pair
// that holds the sorted keys and, as values, the points' indices
template <class KeyFn>
static int sort_by_cell(SortBufs& sb, int n, KeyFn f, unsigned long long nc, int* cstart, hipStream_t s) {
    k_cell_keys<<<cdiv(n, CL_T), CL_T, 0, s>>>(n, f, sb.k[0], sb.v[0]);
    const int cur = radix_sort(sb, n, bits_for(nc), s);
    if (cstart != nullptr) k_cell_starts<<<cdiv((long long)nc + 1, CL_T), CL_T, 0, s>>>(sb.k[cur], n, cstart, (int)nc);
    return cur;
}

// ---------------------------------------------------------------------------------------------------------------------------
// the cube of cells [c - r, c + r] per axis, clamped into a grid of C cells per axis
struct CellCube {
    int x0, x1, y0, y1, z0, z1;
    __device__ __forceinline__ bool covers(int C) const { return x0 == 0 && y0 == 0 && z0 == 0 && x1 == C - 1 && y1 == C - 1 && z1 == C - 1; }
};
__device__ __forceinline__ CellCube cube_around(int cx, int cy, int cz, int r, int C) {
    return CellCube{max(cx - r, 0), min(cx + r, C - 1), max(cy - r, 0), min(cy + r, C - 1), max(cz - r, 0), min(cz + r, C - 1)};
}

}  // namespace
}  // namespace pdhip
