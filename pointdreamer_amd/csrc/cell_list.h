// Point cell list: the box a uniform grid is laid over, the points sorted by cell key (radix_sort.h) with cstart[c] = first sorted point whose
// key is >= c, the sorted (x, y, z, index) copy, the cube of cells a scan visits.  Shared by surface_recon.hip (f32 3-D grid, cell_of, ring_bound)
// and occupancy.hip (f64 xy grid over `inv`), each of which keeps its grid struct, the key functor that repeats its cell arithmetic operation for
// operation, its face bound and its refusal messages: their arithmetic differs and goldens pin it; and by cloud_metrics.hip, knn.hip, subsample.hip
// and mesh_distance.hip, which share the f64 3-D grid of the last section: the grid, the key, the certificate's face bound, the (d2, index)
// minimum and the staged scan of everything for the queries the certificate leaves.  Internal linkage: each including unit gets its own copy.
// Zero scratch.  tests/test_gpu_prims.py holds the sort half (k_cell_keys, k_cell_starts, sort_by_cell) to exact references, through the copy in
// prims_debug.hip.
#pragma once
#include "radix_sort.h"
#include <string.h>
#include <math.h>
#include <limits.h>
#include <algorithm>

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

// ---------------------------------------------------------------------------------------------------------------------------
// the f64 3-D grid: C^3 cubic cells of edge cs from the corner (ox, oy, oz).  A point outside is clamped into a boundary cell.  Host code as well:
// a host program can run the very cull against an oracle without a device
struct Grid3 {
    double ox, oy, oz, cs;
    int C;
    __host__ __device__ __forceinline__ int cell(double x, double o) const { return (int)fmin(fmax(floor((x - o) / cs), 0.0), (double)(C - 1)); }
};

// KeyFn of sort_by_cell: the key of the cell that point i of P falls (or is clamped) into
struct GridPointKey {
    const float* P;
    Grid3 g;
    __device__ uint64_t operator()(int i) const {
        const int cx = g.cell((double)P[3 * (size_t)i], g.ox), cy = g.cell((double)P[3 * (size_t)i + 1], g.oy),
                  cz = g.cell((double)P[3 * (size_t)i + 2], g.oz);
        return (uint64_t)((cz * g.C + cy) * g.C + cx);
    }
};

// The certificate.  A scan that has visited every target of the cells [c0, c1] per axis may stop when its worst kept d2 is <= b * b, b = the
// smallest grid_face_bound of the three axes, and b > 0: a target that was not visited lies in another cell, that is beyond a face of the cube that
// is NOT a face of the whole grid (clamping moves points into boundary cells only, so a grid face has nothing behind it -- which is also why points
// outside the grid cost nothing: only non-grid faces bound), so its distance along that axis is at least q's distance to that face.  The face is
// pulled in by 1e-12 of the coordinates' magnitude, far more than the f64 rounding of the cell arithmetic (x - o) / cs, of f = o + c cs and of d2:
// the unvisited target's COMPUTED d2 is then strictly larger than the winner's, and cannot tie with it, so the result equals a brute-force scan bit
// for bit.  No such face on either side: 1e300, i.e. the cube spans the axis.  (mesh_distance.hip keeps md_face_bound: a triangle's closest point
// needs a guard of 1e-7 (|q| + gmax) that does not depend on the face, computed once; a guard parameter would change the operations of one side.)
__host__ __device__ __forceinline__ double grid_face_bound(double q, double o, double cs, int C, int c0, int c1) {
    double b = 1.0e300;
    if (c0 > 0) {
        const double f = o + (double)c0 * cs;
        b = fmin(b, (q - f) - 1.0e-12 * (fabs(q) + fabs(f)));
    }
    if (c1 < C - 1) {
        const double f = o + (double)(c1 + 1) * cs;
        b = fmin(b, (f - q) - 1.0e-12 * (fabs(q) + fabs(f)));
    }
    return b;
}
__host__ __device__ __forceinline__ double grid_cube_bound(const Grid3& g, double qx, double qy, double qz, const CellCube& q) {
    return fmin(fmin(grid_face_bound(qx, g.ox, g.cs, g.C, q.x0, q.x1), grid_face_bound(qy, g.oy, g.cs, g.C, q.y0, q.y1)),
                grid_face_bound(qz, g.oz, g.cs, g.C, q.z0, q.z1));
}

// the lexicographic order of (d2, index): the minimum, and of the candidates that attain it the smallest index, depend on no scan order.  A NaN
// never wins (both comparisons are false for it).  (take_min spells the condition out: through pair_less the compiler selects where it branched,
// and the scans' registers grow)
__host__ __device__ __forceinline__ bool pair_less(double d, int k, double bd, int bi) { return d < bd || (d == bd && k < bi); }
__host__ __device__ __forceinline__ void take_min(double d, int k, double& bd, int& bi) {
    if (d < bd || (d == bd && k < bi)) { bd = d; bi = k; }
}

// d2 = (dx dx + dy dy) + dz dz with the f32 inputs widened to f64, op by op
__host__ __device__ __forceinline__ double point_d2(double qx, double qy, double qz, const float4& a) {
    const double dx = qx - (double)a.x, dy = qy - (double)a.y, dz = qz - (double)a.z;
    return (dx * dx + dy * dy) + dz * dz;
}

// host: C cells per axis over the cube of edge ext at mn, stretched by 1e-6 so that the box's far corner falls inside the last cell.  A box
// without extent: one cell
static Grid3 grid_over(const double mn[3], double ext, int C) {
    Grid3 g;
    g.C = ext > 0.0 ? C : 1;
    g.cs = ext > 0.0 ? ext / g.C * (1.0 + 1.0e-6) : 1.0;
    g.ox = mn[0]; g.oy = mn[1]; g.oz = mn[2];
    return g;
}
static double box_extent(const double mn[3], const double mx[3]) {
    double ext = 0.0;
    for (int a = 0; a < 3; ++a) ext = std::max(ext, mx[a] - mn[a]);
    return ext;
}
// host: mn = the corner of the part of the targets' box [tmn, tmx] that the queries' box meets (of the whole box if they do not meet), returns its
// extent: a few outliers among the targets do not coarsen the cells where the queries are.  Points outside the grid are clamped into its boundary
// cells, which the certificate allows
static double meet_boxes(const double tmn[3], const double tmx[3], const HostBox& q, double mn[3]) {
    double lo[3], hi[3];
    bool meet = true;
    for (int a = 0; a < 3; ++a) {
        lo[a] = std::max(tmn[a], q.mn[a]);
        hi[a] = std::min(tmx[a], q.mx[a]);
        meet = meet && lo[a] <= hi[a];
    }
    for (int a = 0; a < 3; ++a) mn[a] = meet ? lo[a] : tmn[a];
    return meet ? box_extent(lo, hi) : box_extent(tmn, tmx);
}

// host: the boxes of the targets and of the queries into words[0 .. 2 BOX_WORDS), the nwords words cleared (launches only) ...
static void launch_point_box(const float* P, int n, uint32_t* box, hipStream_t s) {
    k_point_box<<<std::min(cdiv(n, CL_T), 1024), CL_T, 0, s>>>(P, n, nullptr, n, 1, box);
}
static int launch_cloud_boxes(const float* targets, int M, const float* queries, int Q, uint32_t* words, int nwords, hipStream_t s) {
    const int rc = clear_boxes(words, 2, nwords, s);
    if (rc) return rc;
    launch_point_box(targets, M, words, s);
    launch_point_box(queries, Q, words + BOX_WORDS, s);
    PD_LAUNCH_CHECK();
    return PDHIP_OK;
}
// ... and their read (the one synchronisation: what the entry enqueued in between arrives with it), which refuses non-finite coordinates
static int read_cloud_boxes(const char* entry, const uint32_t* words, HostBox (&box)[2], hipStream_t s) {
    const int rc = read_boxes(words, box, s);
    if (rc) return rc;
    PD_REQUIRE(box[0].bad == 0, "%s: %u target(s) with a non-finite coordinate", entry, box[0].bad);
    PD_REQUIRE(box[1].bad == 0, "%s: %u query point(s) with a non-finite coordinate", entry, box[1].bad);
    return PDHIP_OK;
}

// counts[] of a two-way split of Q queries: {certified, left to the scan of everything (all of them when `all`), cells per axis, 0}
__global__ void k_split_counts(const int* __restrict__ left_n, int Q, int C, int all, int32_t* __restrict__ counts) {
    const int n = all ? Q : min(*left_n, Q);
    counts[0] = Q - n; counts[1] = n; counts[2] = C; counts[3] = 0;
}

// ---------------------------------------------------------------------------------------------------------------------------
// The staged scan of everything, for the queries far_list[0 .. *far_n) that a ring scan gave up (far from every element: a thread of its own would
// scan most of the grid; or in crowded cells): every element against every such query, no certificate needed.  Workgroup (tile, slab): T queries of
// the list against one of SLABS slabs of st[0 .. f.live()), staged in LDS in chunks of CHUNK -> part[slab][i]; k_far_pick takes the minimum over the
// slabs.  Far: a small struct passed by value with
//   __device__ int live() const                                                          how many elements of st count
//   __device__ double d2(double qx, double qy, double qz, const Elem& a, int& k) const   the squared distance to element a, k = its index
//   static __device__ double none()  /  static __device__ int index(int bi)              the d2 of "nothing yet"; the index to report (bi == INT_MAX: nothing)
template <int T, int CHUNK, int SLABS, class Elem, class Far>
__global__ __launch_bounds__(T) void k_far_scan(const float4* __restrict__ sq, const int* __restrict__ far_list, const int* __restrict__ far_n, int Q,
                                                const Elem* __restrict__ st, Far f, double* __restrict__ part_d2, int* __restrict__ part_idx) {
    __shared__ Elem s_t[CHUNK];
    const int t = threadIdx.x;
    const int n = min(*far_n, Q);
    if ((int)blockIdx.x * T >= n) return;                          // (the whole workgroup)
    const int i = blockIdx.x * T + t;
    const bool have = i < n;
    double qx = 0.0, qy = 0.0, qz = 0.0;
    if (have) {
        const float4 me = sq[far_list[i]];
        qx = (double)me.x; qy = (double)me.y; qz = (double)me.z;
    }
    const int M = f.live();
    const int per = (M + SLABS - 1) / SLABS;
    const int b0 = min(M, (int)blockIdx.y * per), e0 = min(M, b0 + per);
    double bd = Far::none();
    int bi = INT_MAX;
    for (int base = b0; base < e0; base += CHUNK) {
        const int nc = min(CHUNK, e0 - base);
        __syncthreads();
        for (int j = t; j < nc; j += T) s_t[j] = st[base + j];
        __syncthreads();
        if (have) {
            for (int j = 0; j < nc; ++j) {
                const Elem a = s_t[j];
                int k;
                const double d = f.d2(qx, qy, qz, a, k);
                take_min(d, k, bd, bi);
            }
        }
    }
    if (have) {
        part_d2[(size_t)blockIdx.y * Q + i] = bd;
        part_idx[(size_t)blockIdx.y * Q + i] = bi;
    }
}

template <int T, int SLABS, class Far>
__global__ __launch_bounds__(T) void k_far_pick(const float4* __restrict__ sq, const int* __restrict__ far_list, const int* __restrict__ far_n, int Q,
                                                const double* __restrict__ part_d2, const int* __restrict__ part_idx, double* __restrict__ d2,
                                                int* __restrict__ idx) {
    const int i = blockIdx.x * T + threadIdx.x;
    if (i >= min(*far_n, Q)) return;
    double bd = Far::none();
    int bi = INT_MAX;
    for (int sl = 0; sl < SLABS; ++sl) take_min(part_d2[(size_t)sl * Q + i], part_idx[(size_t)sl * Q + i], bd, bi);
    const int o = __float_as_int(sq[far_list[i]].w);
    d2[o] = bd;
    idx[o] = Far::index(bi);
}

}  // namespace
}  // namespace pdhip
