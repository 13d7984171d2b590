// Geometry scores of a reconstruction on the device (models/POCO/eval/src/eval.py: distance_p2p, get_threshold_percentage and the sums behind
// eval_pointcloud): the exact nearest neighbour of every point of one cloud in another, and the reduction of the distances.
//
//   pdhip_nearest_points
//     a. bounding boxes and a finiteness test of both clouds (integer atomics on order-preserving keys; one small read that synchronises the
//        stream); a uniform grid of C^3 cells (cell_list.h's Grid3), C ~ sqrt(M / 8): a few targets per occupied cell of a surface, over the cube of the
//        part of the targets' box that the queries' box meets (meet_boxes).  Points outside the grid are clamped into its boundary cells;
//     b. targets sorted by cell key (cell_list.h, as is a.'s box kernel), cstart[c] = first sorted target whose key is >= c, for c = 0 .. C^3 (a binary search per cell): the targets of the
//        cells x0 .. x1 of a grid row are ONE run of the sorted array; queries sorted by the key of the cell they fall (or are clamped) into;
//     c. phase 1 (k_cm_stage_scan): a workgroup owns CM_T consecutive sorted queries, takes the bounding cell box of their cells plus one ring,
//        stages the targets of that box into LDS as (x, y, z, index) in chunks of CM_CHUNK, and every thread scans each chunk for its own query
//        in f64.  A query is CERTIFIED when its best d2 is <= the squared distance from the query to the nearest face of the staged box that is
//        not a face of the whole grid (cell_list.h's grid_face_bound, which has the argument why an unstaged target's d2 is then strictly
//        larger).  A box of more than CM_ROWS grid rows or CM_BOX_CHUNKS chunks certifies nobody;
//     d. phase 2 (k_cm_ring_scan): one thread per query that phase 1 left, the cube of cells [c - r, c + r] scanned from global memory with
//        r = 1, 2, 4, 8 until the same certificate holds or the cube is the whole grid;
//     e. far scan (cell_list.h's k_far_scan, k_far_pick with CmFar): a query still open after r = 8 is far from every target, and a thread of its own
//        would scan most of the grid; a query whose rings hold more than CM_RING_WORK targets sits in crowded cells.  Such queries are scanned
//        against ALL targets, a tile of CM_T of them per workgroup and the targets staged in LDS, the sorted targets cut into CM_FAR_SLABS slabs;
//        the minimum over the slabs (smallest index on a tie) is taken by the second kernel.
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

// ---------------------------------------------------------------------------------------------------------------------------
// c. phase 1
__global__ __launch_bounds__(CM_T) void k_cm_stage_scan(const float4* __restrict__ sq, int Q, const float4* __restrict__ st,
                                                        const int* __restrict__ cstart, Grid3 g, double* __restrict__ d2,
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
        const int cx = g.cell(qx, g.ox), cy = g.cell(qy, g.oy), cz = g.cell(qz, g.oz);
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
                    take_min(point_d2(qx, qy, qz, a), __float_as_int(a.w), bd, bi);
                }
            }
        }
    }
    if (!have) return;
    bool cert = false;
    if (ok && bi != INT_MAX) {
        const double b = grid_cube_bound(g, qx, qy, qz, CellCube{x0, x1, y0, y1, z0, z1});
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
                                                          int n_all, const float4* __restrict__ st, const int* __restrict__ cstart, Grid3 g,
                                                          double* __restrict__ d2, int* __restrict__ idx, int* __restrict__ far_list,
                                                          int* __restrict__ far_n) {
    const int i = blockIdx.x * CM_P2_T + threadIdx.x;
    const int n = list != nullptr ? min(*n_ptr, n_all) : n_all;
    if (i >= n) return;
    const int sp = list != nullptr ? list[i] : i;
    const float4 me = sq[sp];
    const double qx = (double)me.x, qy = (double)me.y, qz = (double)me.z;
    const int C = g.C;
    const int cx = g.cell(qx, g.ox), cy = g.cell(qy, g.oy), cz = g.cell(qz, g.oz);
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
                    const double d = point_d2(qx, qy, qz, a);
                    const int k = __float_as_int(a.w);
                    if (d < bd || (d == bd && k < bi)) { bd = d; bi = k; }       // (take_min, spelled out: through it this kernel takes two VGPRs more)
                }
            }
        const double b = grid_cube_bound(g, qx, qy, qz, q);
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

// e. the queries the ring scan gave up against all M sorted targets (cell_list.h's k_far_scan / k_far_pick)
struct CmFar {
    int M;
    __device__ int live() const { return M; }
    __device__ double d2(double qx, double qy, double qz, const float4& a, int& k) const {
        k = __float_as_int(a.w);
        return point_d2(qx, qy, qz, a);
    }
    static __device__ double none() { return 1.0e300; }
    static __device__ int index(int bi) { return bi; }
};

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
    // a. the boxes, finiteness of both clouds; the grid over the part of the targets' box that the queries' box meets
    int rc = launch_cloud_boxes(targets, M, queries, Q, w.misc, MISC_WORDS, s);
    if (rc) return rc;
    HostBox box[2];                                                // targets, queries
    rc = read_cloud_boxes("pdhip_nearest_points", w.misc, box, s);
    if (rc) return rc;
    double mn[3];
    const double ext = meet_boxes(box[0].mn, box[0].mx, box[1], mn);
    const Grid3 g = grid_over(mn, ext, cells_axis_max(M));
    const int nc = g.C * g.C * g.C;
    // b. both clouds in cell order
    int cur = sort_by_cell(w.sb, M, GridPointKey{targets, g}, (unsigned long long)nc, w.cstart, s);
    k_gather_xyzi<<<cdiv(M, CL_T), CL_T, 0, s>>>(w.sb.v[cur], targets, M, w.st);
    cur = sort_by_cell(w.sb, Q, GridPointKey{queries, g}, (unsigned long long)nc, nullptr, s);      // (the queries need the order only)
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
    k_far_scan<CM_T, CM_CHUNK, CM_FAR_SLABS><<<dim3(cdiv(Q, CM_T), CM_FAR_SLABS), CM_T, 0, s>>>(w.sq, w.far_list, far_n, Q, w.st, CmFar{M}, w.part_d2, w.part_idx);
    k_far_pick<CM_T, CM_FAR_SLABS, CmFar><<<cdiv(Q, CM_T), CM_T, 0, s>>>(w.sq, w.far_list, far_n, Q, w.part_d2, w.part_idx, d2, idx);
    k_split_counts<<<1, 1, 0, s>>>(unc_n, Q, g.C, forced, counts);             // (unc_n <= Q: a query enters the list once)
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
