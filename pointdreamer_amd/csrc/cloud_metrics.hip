// Geometry scores of a reconstruction on the device (models/POCO/eval/src/eval.py: distance_p2p, get_threshold_percentage and the sums behind
// eval_pointcloud): the exact nearest neighbour of every point of one cloud in another, and the reduction of the distances.
//
//   pdhip_nearest_points
//     a. bounding boxes and a finiteness test of both clouds (integer atomics on order-preserving keys; one small read that synchronises the
//        stream); a uniform grid of C^3 cells, C ~ sqrt(M / 8): a few targets per occupied cell of a surface, over the cube of the part of the
//        targets' box that the queries' box meets.  Points outside the grid are clamped into its boundary cells;
//     b. targets sorted by cell key (cell_list.h, as is a.'s box kernel), cstart[c] = first sorted target whose key is >= c, for c = 0 .. C^3 (a binary search per cell): the targets of the
//        cells x0 .. x1 of a grid row are ONE run of the sorted array; queries sorted by the key of the cell they fall (or are clamped) into;
//     c. phase 1 (k_cm_stage_scan): a workgroup owns CM_T consecutive sorted queries, takes the bounding cell box of their cells plus one ring,
//        stages the targets of that box into LDS as (x, y, z, index) in chunks of CM_CHUNK, and every thread scans each chunk for its own query
//        in f64.  A query is CERTIFIED when its best d2 is <= the squared distance from the query to the nearest face of the staged box that is
//        not a face of the whole grid (a target that was not staged lies beyond such a face); the faces are pulled in by 1e-12 of the
//        coordinates' magnitude, far more than the f64 rounding of the cell arithmetic and of d2, so that an unstaged target's d2 is strictly
//        larger.  A box of more than CM_ROWS grid rows or CM_BOX_CHUNKS chunks certifies nobody;
//     d. phase 2 (k_cm_ring_scan): one thread per query that phase 1 left, the cube of cells [c - r, c + r] scanned from global memory with
//        r = 1, 2, 4, 8 until the same certificate holds or the cube is the whole grid;
//     e. far scan (k_cm_far_scan, k_cm_far_pick): a query still open after r = 8 is far from every target, and a thread of its own would scan most of the
//        grid; a query whose rings hold more than CM_RING_WORK targets sits in crowded cells.  Such queries are scanned against ALL targets, a tile of CM_T of them per workgroup and the targets staged in LDS, the targets cut into
//        CM_FAR_SLABS slabs over the second grid axis; the minimum over the slabs (smallest index on a tie) is taken by a second kernel.
//     Shipped: d + e for every query (in cell order, so that neighbouring threads scan the same cells); c + d + e behind pdhip_debug_set_nearest_path(1).
//     Measured at 10^5 x 10^5 points (profiles/geometry_metrics_bench.txt) the staged scan loses: a workgroup's 256 queries in row-major cell order span
//     whole grid rows, every thread scans every target of that box, and the cell list already sits in the L2 -- staging it saves no traffic that matters.
//     d2 = (dx dx + dy dy) + dz dz with the f32 inputs widened to f64, op by op; the minimum over all targets, and of the targets that attain
//     it the smallest index: neither depends on the scan order, so the result equals a brute-force scan bit for bit.
//   pdhip_cloud_metrics
//     sum sqrt(d2), sum d2, sum |n_src . n_tgt[idx]| by a fixed tree (per-thread strided sums, workgroup tree, one workgroup over the partials),
//     and within[j] = #{sqrt(d2) <= thresholds[j]}: per-query bin by binary search, an integer histogram in LDS, integer global atomics, prefix sum.
// No floating-point atomics: two calls give equal bytes.  Compiled with -ffp-contract=off.  Every kernel keeps zero scratch.
#include "common.h"
#include "cell_list.h"
#include <math.h>
#include <limits.h>
#include <algorithm>
using namespace pdhip;

namespace {

constexpr int CM_T = 256;                     // queries per workgroup of phase 1
constexpr int CM_CHUNK = 2048;                // targets staged at a time: 32 KiB of LDS (four workgroups per CU)
constexpr int CM_BOX_CHUNKS = 16;             // a box with more targets than this many chunks goes to phase 2
constexpr int CM_ROWS = 2 * CM_T;             // grid rows (y, z) of a staged box
constexpr int CM_CELLS_MAX = 128;             // cells per axis
constexpr double CM_OCC = 8.0;                // C = sqrt(M / CM_OCC)
constexpr int CM_P2_T = 64;
constexpr int CM_RING_MAX = 8;                // the ring scan gives up after the cube [c - 8, c + 8], or after CM_RING_WORK targets (crowded cells) ...
constexpr int CM_RING_WORK = 4096;
constexpr int CM_FAR_SLABS = 16;              // ... and the far scan cuts the targets into this many slabs per tile of CM_T queries
constexpr int CM_NB = 256;                    // workgroups of the reduction (== CM_T: one finalize workgroup reads them all)
constexpr int CM_TMAX = 4096;                 // thresholds
constexpr int CM_NMAX = 1 << 26;
enum { MISC_UNC = 2 * BOX_WORDS, MISC_FAR = MISC_UNC + 1, MISC_WORDS = 32 };      // behind the two boxes (cell_list.h)

struct CmGrid {
    double ox, oy, oz, cs;
    int C;
};

__device__ __forceinline__ int cm_cell(double x, double o, double cs, int C) {
    return (int)fmin(fmax(floor((x - o) / cs), 0.0), (double)(C - 1));
}

// distance from q to the nearest face of the cells [c0, c1] that is not a face of the whole grid, less the safety margin
__device__ __forceinline__ double cm_face_bound(double q, double o, double cs, int C, int c0, int c1) {
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

// ---------------------------------------------------------------------------------------------------------------------------
// b. the key of the cell that point i of P falls (or is clamped) into
struct CmKey {
    const float* P;
    CmGrid g;
    __device__ uint64_t operator()(int i) const {
        const int cx = cm_cell((double)P[3 * (size_t)i], g.ox, g.cs, g.C), cy = cm_cell((double)P[3 * (size_t)i + 1], g.oy, g.cs, g.C),
                  cz = cm_cell((double)P[3 * (size_t)i + 2], g.oz, g.cs, g.C);
        return (uint64_t)((cz * g.C + cy) * g.C + cx);
    }
};

// ---------------------------------------------------------------------------------------------------------------------------
// c. phase 1
__global__ __launch_bounds__(CM_T) void k_cm_stage_scan(const float4* __restrict__ sq, int Q, const float4* __restrict__ st,
                                                        const int* __restrict__ cstart, CmGrid g, double* __restrict__ d2,
                                                        int* __restrict__ idx, int* __restrict__ unc_list, int* __restrict__ unc_n) {
    __shared__ float4 s_t[CM_CHUNK];
    __shared__ int s_rs[CM_ROWS];                                  // first sorted target of a row of the box
    __shared__ int s_ro[CM_ROWS + 1];                              // targets of the box before that row
    __shared__ int s_scan[CM_T];
    __shared__ int s_box[6];
    const int t = threadIdx.x, C = g.C;
    const int p = blockIdx.x * CM_T + t;
    const bool have = p < Q;
    if (t < 3) s_box[t] = INT_MAX;
    else if (t < 6) s_box[t] = -1;
    __syncthreads();
    float4 me = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    double qx = 0.0, qy = 0.0, qz = 0.0;
    if (have) {
        me = sq[p];
        qx = (double)me.x; qy = (double)me.y; qz = (double)me.z;
        const int cx = cm_cell(qx, g.ox, g.cs, C), cy = cm_cell(qy, g.oy, g.cs, C), cz = cm_cell(qz, g.oz, g.cs, C);
        atomicMin(&s_box[0], cx); atomicMin(&s_box[1], cy); atomicMin(&s_box[2], cz);
        atomicMax(&s_box[3], cx); atomicMax(&s_box[4], cy); atomicMax(&s_box[5], cz);
    }
    __syncthreads();
    const int x0 = max(s_box[0] - 1, 0), y0 = max(s_box[1] - 1, 0), z0 = max(s_box[2] - 1, 0);
    const int x1 = min(s_box[3] + 1, C - 1), y1 = min(s_box[4] + 1, C - 1), z1 = min(s_box[5] + 1, C - 1);
    const int ny = y1 - y0 + 1, nrows = ny * (z1 - z0 + 1);
    bool ok = nrows <= CM_ROWS;                                    // (the same for every thread of the workgroup)
    int total = 0;
    if (ok) {
        int cnt[2] = {0, 0};
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const int r = 2 * t + k;
            if (r < nrows) {
                const int base = ((z0 + r / ny) * C + (y0 + r % ny)) * C;
                const int b = cstart[base + x0];
                s_rs[r] = b;
                cnt[k] = cstart[base + x1 + 1] - b;
            }
        }
        const int mine = cnt[0] + cnt[1];
        s_scan[t] = mine;
        __syncthreads();
        for (int off = 1; off < CM_T; off <<= 1) {
            const int add = t >= off ? s_scan[t - off] : 0;
            __syncthreads();
            s_scan[t] += add;
            __syncthreads();
        }
        const int before = s_scan[t] - mine;
        if (2 * t < nrows) s_ro[2 * t] = before;
        if (2 * t + 1 < nrows) s_ro[2 * t + 1] = before + cnt[0];
        total = s_scan[CM_T - 1];
        if (t == 0) s_ro[nrows] = total;
        ok = total <= CM_BOX_CHUNKS * CM_CHUNK;
    }
    double bd = 1.0e300;
    int bi = INT_MAX;
    if (ok) {
        for (int base = 0; base < total; base += CM_CHUNK) {
            const int n = min(CM_CHUNK, total - base);
            __syncthreads();                                       // (s_ro is written; the chunk before is consumed)
            for (int j = t; j < n; j += CM_T) {
                const int gp = base + j;
                int lo = 0, hi = nrows;                            // the row r with s_ro[r] <= gp < s_ro[r + 1]
                while (hi - lo > 1) {
                    const int mid = (lo + hi) >> 1;
                    if (s_ro[mid] <= gp) lo = mid; else hi = mid;
                }
                s_t[j] = st[s_rs[lo] + (gp - s_ro[lo])];
            }
            __syncthreads();
            if (have) {
                for (int j = 0; j < n; ++j) {
                    const float4 a = s_t[j];
                    const double dx = qx - (double)a.x, dy = qy - (double)a.y, dz = qz - (double)a.z;
                    const double d = (dx * dx + dy * dy) + dz * dz;
                    const int i = __float_as_int(a.w);
                    if (d < bd || (d == bd && i < bi)) { bd = d; bi = i; }
                }
            }
        }
    }
    if (!have) return;
    bool cert = false;
    if (ok && bi != INT_MAX) {
        const double b = fmin(fmin(cm_face_bound(qx, g.ox, g.cs, C, x0, x1), cm_face_bound(qy, g.oy, g.cs, C, y0, y1)),
                              cm_face_bound(qz, g.oz, g.cs, C, z0, z1));
        cert = b > 0.0 && bd <= b * b;
    }
    if (cert) {
        const int o = __float_as_int(me.w);
        d2[o] = bd;
        idx[o] = bi;
    } else {
        unc_list[atomicAdd(unc_n, 1)] = p;
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
// d. phase 2: the queries list[0 .. *n_ptr) (list == nullptr: all n_all sorted queries)
__global__ __launch_bounds__(CM_P2_T) void k_cm_ring_scan(const float4* __restrict__ sq, const int* __restrict__ list, const int* __restrict__ n_ptr,
                                                          int n_all, const float4* __restrict__ st, const int* __restrict__ cstart, CmGrid g,
                                                          double* __restrict__ d2, int* __restrict__ idx, int* __restrict__ far_list,
                                                          int* __restrict__ far_n) {
    const int i = blockIdx.x * CM_P2_T + threadIdx.x;
    const int n = list != nullptr ? min(*n_ptr, n_all) : n_all;
    if (i >= n) return;
    const int sp = list != nullptr ? list[i] : i;
    const float4 me = sq[sp];
    const double qx = (double)me.x, qy = (double)me.y, qz = (double)me.z;
    const int C = g.C;
    const int cx = cm_cell(qx, g.ox, g.cs, C), cy = cm_cell(qy, g.oy, g.cs, C), cz = cm_cell(qz, g.oz, g.cs, C);
    double bd = 1.0e300;
    int bi = INT_MAX, work = 0;
    for (int r = 1;; r *= 2) {
        const CellCube q = cube_around(cx, cy, cz, r, C);
        for (int z = q.z0; z <= q.z1; ++z)
            for (int y = q.y0; y <= q.y1; ++y) {
                const int base = (z * C + y) * C;
                const int b = cstart[base + q.x0], e = cstart[base + q.x1 + 1];
                work += e - b;
                if (work > CM_RING_WORK) {                         // crowded cells: the far scan's staged sweep is the cheaper way
                    far_list[atomicAdd(far_n, 1)] = sp;
                    return;
                }
                for (int p = b; p < e; ++p) {
                    const float4 a = st[p];
                    const double dx = qx - (double)a.x, dy = qy - (double)a.y, dz = qz - (double)a.z;
                    const double d = (dx * dx + dy * dy) + dz * dz;
                    const int k = __float_as_int(a.w);
                    if (d < bd || (d == bd && k < bi)) { bd = d; bi = k; }
                }
            }
        const double b = fmin(fmin(cm_face_bound(qx, g.ox, g.cs, C, q.x0, q.x1), cm_face_bound(qy, g.oy, g.cs, C, q.y0, q.y1)),
                              cm_face_bound(qz, g.oz, g.cs, C, q.z0, q.z1));
        if (q.covers(C) || (bi != INT_MAX && b > 0.0 && bd <= b * b)) break;
        if (r >= CM_RING_MAX) {                                    // far from every target: a thread of its own would scan most of the grid
            far_list[atomicAdd(far_n, 1)] = sp;
            return;
        }
    }
    const int o = __float_as_int(me.w);
    d2[o] = bd;
    idx[o] = bi;
}

// e. the queries the ring scan gave up: every target against every such query, no certificate needed.  Workgroup (tile, slab): CM_T queries of the
// list against one slab of the sorted targets, staged in LDS in chunks of CM_CHUNK -> part[slab][i]; k_cm_far_pick takes the minimum over the slabs.
__global__ __launch_bounds__(CM_T) void k_cm_far_scan(const float4* __restrict__ sq, const int* __restrict__ far_list, const int* __restrict__ far_n,
                                                      int Q, const float4* __restrict__ st, int M, double* __restrict__ part_d2,
                                                      int* __restrict__ part_idx) {
    __shared__ float4 s_t[CM_CHUNK];
    const int t = threadIdx.x;
    const int n = min(*far_n, Q);
    if ((int)blockIdx.x * CM_T >= n) return;                       // (the whole workgroup)
    const int i = blockIdx.x * CM_T + t;
    const bool have = i < n;
    double qx = 0.0, qy = 0.0, qz = 0.0;
    if (have) {
        const float4 me = sq[far_list[i]];
        qx = (double)me.x; qy = (double)me.y; qz = (double)me.z;
    }
    const int per = (M + CM_FAR_SLABS - 1) / CM_FAR_SLABS;
    const int b0 = min(M, (int)blockIdx.y * per), e0 = min(M, b0 + per);
    double bd = 1.0e300;
    int bi = INT_MAX;
    for (int base = b0; base < e0; base += CM_CHUNK) {
        const int nc = min(CM_CHUNK, e0 - base);
        __syncthreads();
        for (int j = t; j < nc; j += CM_T) s_t[j] = st[base + j];
        __syncthreads();
        if (have) {
            for (int j = 0; j < nc; ++j) {
                const float4 a = s_t[j];
                const double dx = qx - (double)a.x, dy = qy - (double)a.y, dz = qz - (double)a.z;
                const double d = (dx * dx + dy * dy) + dz * dz;
                const int k = __float_as_int(a.w);
                if (d < bd || (d == bd && k < bi)) { bd = d; bi = k; }
            }
        }
    }
    if (have) {
        part_d2[(size_t)blockIdx.y * Q + i] = bd;
        part_idx[(size_t)blockIdx.y * Q + i] = bi;
    }
}

__global__ __launch_bounds__(CM_T) void k_cm_far_pick(const float4* __restrict__ sq, const int* __restrict__ far_list, const int* __restrict__ far_n,
                                                      int Q, const double* __restrict__ part_d2, const int* __restrict__ part_idx,
                                                      double* __restrict__ d2, int* __restrict__ idx) {
    const int i = blockIdx.x * CM_T + threadIdx.x;
    if (i >= min(*far_n, Q)) return;
    double bd = 1.0e300;
    int bi = INT_MAX;
    for (int sl = 0; sl < CM_FAR_SLABS; ++sl) {
        const double d = part_d2[(size_t)sl * Q + i];
        const int k = part_idx[(size_t)sl * Q + i];
        if (d < bd || (d == bd && k < bi)) { bd = d; bi = k; }
    }
    const int o = __float_as_int(sq[far_list[i]].w);
    d2[o] = bd;
    idx[o] = bi;
}

__global__ void k_cm_counts(const int* __restrict__ unc_n, int Q, int C, int forced, int32_t* __restrict__ counts) {
    const int n = forced ? Q : *unc_n;
    counts[0] = Q - n; counts[1] = n; counts[2] = C; counts[3] = 0;
}

// ---------------------------------------------------------------------------------------------------------------------------
// the reduction: part[w][block], w = 0 sqrt(d2), 1 d2, 2 |n . n|; hist[b] = queries whose distance falls into bin b (T: beyond every threshold)
__global__ __launch_bounds__(CM_T) void k_cm_reduce(const double* __restrict__ d2, const int* __restrict__ idx, int Q, const float* __restrict__ ns,
                                                    const float* __restrict__ nt, int M, const double* __restrict__ thr, int T,
                                                    double* __restrict__ part, unsigned long long* __restrict__ hist) {
    __shared__ double sh[3][CM_T];
    __shared__ int s_h[CM_TMAX + 1];
    const int t = threadIdx.x;
    for (int j = t; j <= T; j += CM_T) s_h[j] = 0;
    __syncthreads();
    double s0 = 0.0, s1 = 0.0, s2 = 0.0;
    for (long long q = (long long)blockIdx.x * CM_T + t; q < Q; q += (long long)gridDim.x * CM_T) {
        const double d = d2[q], r = sqrt(d);
        s0 += r; s1 += d;
        int lo = 0, hi = T;                                        // the first threshold with r <= thr[j]
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (r <= thr[mid]) hi = mid; else lo = mid + 1;
        }
        atomicAdd(&s_h[lo], 1);
        if (ns != nullptr && nt != nullptr) {
            const int i = idx[q];
            if (i >= 0 && i < M) {
                const double ax = (double)ns[3 * q], ay = (double)ns[3 * q + 1], az = (double)ns[3 * q + 2];
                const double bx = (double)nt[3 * (size_t)i], by = (double)nt[3 * (size_t)i + 1], bz = (double)nt[3 * (size_t)i + 2];
                const double la = sqrt((ax * ax + ay * ay) + az * az), lb = sqrt((bx * bx + by * by) + bz * bz);
                if (la > 0.0 && lb > 0.0 && la < 1.0e300 && lb < 1.0e300) {
                    const double v = fabs(((ax / la) * (bx / lb) + (ay / la) * (by / lb)) + (az / la) * (bz / lb));
                    if (v == v) s2 += v;
                }
            }
        }
    }
    sh[0][t] = s0; sh[1][t] = s1; sh[2][t] = s2;
    __syncthreads();
    for (int off = CM_T / 2; off > 0; off >>= 1) {
        if (t < off) {
#pragma unroll
            for (int w = 0; w < 3; ++w) sh[w][t] = sh[w][t] + sh[w][t + off];
        }
        __syncthreads();
    }
    if (t < 3) part[t * CM_NB + blockIdx.x] = sh[t][0];
    for (int j = t; j <= T; j += CM_T)
        if (s_h[j]) atomicAdd(&hist[j], (unsigned long long)s_h[j]);
}

__global__ __launch_bounds__(CM_T) void k_cm_finalize(const double* __restrict__ part, int nb, int with_normals, double* __restrict__ sums) {
    __shared__ double sh[3][CM_T];
    const int t = threadIdx.x;
#pragma unroll
    for (int w = 0; w < 3; ++w) sh[w][t] = t < nb ? part[w * CM_NB + t] : 0.0;
    __syncthreads();
    for (int off = CM_T / 2; off > 0; off >>= 1) {
        if (t < off) {
#pragma unroll
            for (int w = 0; w < 3; ++w) sh[w][t] = sh[w][t] + sh[w][t + off];
        }
        __syncthreads();
    }
    if (t < 3) sums[t] = (t == 2 && !with_normals) ? 0.0 : sh[t][0];
    if (t == 3) sums[3] = 0.0;
}

// ---------------------------------------------------------------------------------------------------------------------------
static int cells_axis_max(int M) { return std::max(1, std::min(CM_CELLS_MAX, (int)floor(sqrt((double)M / CM_OCC)))); }

struct NearWs {
    SortBufs sb;
    float4 *st, *sq;
    int *cstart, *unc_list, *far_list, *part_idx;
    double* part_d2;
    uint32_t* misc;                                                // box of the targets, box of the queries, the phase 2 counter
};
static size_t carve_nearest(NearWs& w, void* base, int Q, int M) {
    Carve c{static_cast<char*>(base), 0};
    const size_t C = (size_t)cells_axis_max(M);
    carve_sort(c, w.sb, (size_t)std::max(Q, M));
    w.st = c.take<float4>((size_t)M);
    w.sq = c.take<float4>((size_t)Q);
    w.cstart = c.take<int>(C * C * C + 1);
    w.unc_list = c.take<int>((size_t)Q);
    w.far_list = c.take<int>((size_t)Q);
    w.part_d2 = c.take<double>((size_t)CM_FAR_SLABS * Q);
    w.part_idx = c.take<int>((size_t)CM_FAR_SLABS * Q);
    w.misc = c.take<uint32_t>(MISC_WORDS);
    return c.off + 256;
}

struct MetricWs {
    double* part;
    unsigned long long* hist;
};
static size_t carve_metrics(MetricWs& w, void* base, int T) {
    Carve c{static_cast<char*>(base), 0};
    w.part = c.take<double>(3 * CM_NB);
    w.hist = c.take<unsigned long long>((size_t)T + 1);
    return c.off + 256;
}

}  // namespace

// tuning / test hook: 0 = the ring scan for every query (shipped: the faster form at 10^5 x 10^5 points, profiles/geometry_metrics_bench.txt);
// 1 = the LDS phase first, the ring scan for the queries it could not certify.  Same results either way.
static thread_local int g_nearest_path = 0;
extern "C" int pdhip_debug_set_nearest_path(int path) { int old = g_nearest_path; g_nearest_path = path; return old; }
extern "C" int pdhip_nearest_points_stage_chunk(void) { return CM_CHUNK; }

extern "C" size_t pdhip_nearest_points_workspace_bytes(int Q, int M) {
    if (Q < 0 || M < 1 || Q > CM_NMAX || M > CM_NMAX) return 0;
    NearWs w;
    return carve_nearest(w, nullptr, Q, M);
}

extern "C" int pdhip_nearest_points(const float* queries, int Q, const float* targets, int M, double* d2, int32_t* idx, int32_t* counts,
                                    void* ws, void* stream) {
    PD_REQUIRE(Q >= 0 && Q <= CM_NMAX, "pdhip_nearest_points: Q=%d queries, need 0 .. 2^26", Q);
    PD_REQUIRE(M >= 1 && M <= CM_NMAX, "pdhip_nearest_points: M=%d targets, need 1 .. 2^26", M);
    PD_REQUIRE(targets && counts && ws && (Q == 0 || (queries && d2 && idx)), "pdhip_nearest_points: null pointer");
    hipStream_t s = as_stream(stream);
    if (Q == 0) {
        PD_HIP(hipMemsetAsync(counts, 0, 4 * sizeof(int32_t), s));
        return PDHIP_OK;
    }
    NearWs w;
    carve_nearest(w, ws, Q, M);
    // a. the targets' box, finiteness of both clouds
    int rc = clear_boxes(w.misc, 2, MISC_WORDS, s);
    if (rc) return rc;
    k_point_box<<<std::min(cdiv(M, CL_T), 1024), CL_T, 0, s>>>(targets, M, nullptr, M, 1, w.misc);
    k_point_box<<<std::min(cdiv(Q, CL_T), 1024), CL_T, 0, s>>>(queries, Q, nullptr, Q, 1, w.misc + BOX_WORDS);
    PD_LAUNCH_CHECK();
    HostBox box[2];                                                // targets, queries
    rc = read_boxes(w.misc, box, s);
    if (rc) return rc;
    PD_REQUIRE(box[0].bad == 0, "pdhip_nearest_points: %u target(s) with a non-finite coordinate", box[0].bad);
    PD_REQUIRE(box[1].bad == 0, "pdhip_nearest_points: %u query point(s) with a non-finite coordinate", box[1].bad);
    double mn[3], ext = 0.0;
    for (int a = 0; a < 3; ++a) {
        mn[a] = box[0].mn[a];
        ext = std::max(ext, box[0].mx[a] - mn[a]);
    }
    // the grid covers the part of the targets' box that the queries' box meets (the whole box if they do not meet): a few outliers among the targets do
    // not coarsen the cells where the queries are.  Points outside the grid are clamped into its boundary cells, which the certificate allows: it
    // bounds only by faces that are not faces of the grid.
    double lo[3], hi[3];
    bool meet = true;
    for (int a = 0; a < 3; ++a) {
        lo[a] = std::max(mn[a], box[1].mn[a]);
        hi[a] = std::min(box[0].mx[a], box[1].mx[a]);
        meet = meet && lo[a] <= hi[a];
    }
    if (meet) {
        ext = 0.0;
        for (int a = 0; a < 3; ++a) {
            mn[a] = lo[a];
            ext = std::max(ext, hi[a] - lo[a]);
        }
    }
    CmGrid g;
    g.C = ext > 0.0 ? cells_axis_max(M) : 1;                       // (a box without extent: one cell)
    g.cs = ext > 0.0 ? ext / g.C * (1.0 + 1.0e-6) : 1.0;
    g.ox = mn[0]; g.oy = mn[1]; g.oz = mn[2];
    const int nc = g.C * g.C * g.C;
    // b. both clouds in cell order
    int cur = sort_by_cell(w.sb, M, CmKey{targets, g}, (unsigned long long)nc, w.cstart, s);
    k_gather_xyzi<<<cdiv(M, CL_T), CL_T, 0, s>>>(w.sb.v[cur], targets, M, w.st);
    cur = sort_by_cell(w.sb, Q, CmKey{queries, g}, (unsigned long long)nc, nullptr, s);      // (the queries need the order only)
    k_gather_xyzi<<<cdiv(Q, CL_T), CL_T, 0, s>>>(w.sb.v[cur], queries, Q, w.sq);
    PD_LAUNCH_CHECK();
    // c, d.
    int* unc_n = reinterpret_cast<int*>(w.misc + MISC_UNC);
    int* far_n = reinterpret_cast<int*>(w.misc + MISC_FAR);
    const int forced = g_nearest_path != 1;
    if (!forced) {
        k_cm_stage_scan<<<cdiv(Q, CM_T), CM_T, 0, s>>>(w.sq, Q, w.st, w.cstart, g, d2, idx, w.unc_list, unc_n);
        k_cm_ring_scan<<<cdiv(Q, CM_P2_T), CM_P2_T, 0, s>>>(w.sq, w.unc_list, unc_n, Q, w.st, w.cstart, g, d2, idx, w.far_list, far_n);
    } else {
        k_cm_ring_scan<<<cdiv(Q, CM_P2_T), CM_P2_T, 0, s>>>(w.sq, nullptr, nullptr, Q, w.st, w.cstart, g, d2, idx, w.far_list, far_n);
    }
    k_cm_far_scan<<<dim3(cdiv(Q, CM_T), CM_FAR_SLABS), CM_T, 0, s>>>(w.sq, w.far_list, far_n, Q, w.st, M, w.part_d2, w.part_idx);
    k_cm_far_pick<<<cdiv(Q, CM_T), CM_T, 0, s>>>(w.sq, w.far_list, far_n, Q, w.part_d2, w.part_idx, d2, idx);
    k_cm_counts<<<1, 1, 0, s>>>(unc_n, Q, g.C, forced, counts);
    PD_LAUNCH_CHECK();
    return PDHIP_OK;
}

extern "C" size_t pdhip_cloud_metrics_workspace_bytes(int T) {
    if (T < 0 || T > CM_TMAX) return 0;
    MetricWs w;
    return carve_metrics(w, nullptr, T);
}

extern "C" int pdhip_cloud_metrics(const double* d2, const int32_t* idx, int Q, const float* normals_src, const float* normals_tgt, int M,
                                   const double* thresholds, int T, double* sums, int64_t* within, void* ws, void* stream) {
    PD_REQUIRE(Q >= 0 && Q <= CM_NMAX, "pdhip_cloud_metrics: Q=%d distances, need 0 .. 2^26", Q);
    PD_REQUIRE(M >= 1 && M <= CM_NMAX, "pdhip_cloud_metrics: M=%d targets, need 1 .. 2^26", M);
    PD_REQUIRE(T >= 0 && T <= CM_TMAX, "pdhip_cloud_metrics: T=%d thresholds, need 0 .. %d", T, CM_TMAX);
    PD_REQUIRE(sums && ws && (T == 0 || (thresholds && within)) && (Q == 0 || (d2 && idx)), "pdhip_cloud_metrics: null pointer");
    hipStream_t s = as_stream(stream);
    MetricWs w;
    carve_metrics(w, ws, T);
    const int with_normals = normals_src != nullptr && normals_tgt != nullptr;
    const int nb = std::min(CM_NB, cdiv(Q, CM_T));                 // (a function of Q alone: the tree is the same on every call)
    PD_HIP(hipMemsetAsync(w.hist, 0, ((size_t)T + 1) * sizeof(unsigned long long), s));
    if (nb > 0) k_cm_reduce<<<nb, CM_T, 0, s>>>(d2, idx, Q, normals_src, normals_tgt, M, thresholds, T, w.part, w.hist);
    k_cm_finalize<<<1, CM_T, 0, s>>>(w.part, nb, with_normals, sums);
    if (T > 0) k_scan<unsigned long long><<<1, SC_T, 0, s>>>(w.hist, reinterpret_cast<unsigned long long*>(within), T, 0);
    PD_LAUNCH_CHECK();
    return PDHIP_OK;
}
