// Exact k nearest neighbours on the device and statistical outlier removal on top of them (no reference counterpart: the reference's
// `input_already_noisy` only picks a POCO weight set; PCL's StatisticalOutlierRemoval and Open3D's remove_statistical_outlier are the definition).
//
//   pdhip_knn_points
//     a. bounding boxes and a finiteness test of both clouds (cell_list.h's k_point_box) and a histogram of the targets' coordinates per axis
//        over their box (k_kn_axis_hist), all three read at once (the call's one synchronisation); a uniform f64 grid of C^3 cells (cell_list.h's
//        Grid3), C ~ sqrt(M / occ) with occ = max(8, k / 2) targets per occupied cell of a surface, over the part of the targets' SPAN that the queries' box meets.
//        The span is the box cut, per axis, to the bins between the 1 % and 99 % quantiles and widened by a tenth: a clean cloud keeps its box,
//        and a few points far outside -- what the filter on top exists for -- no longer blow the cells up until the object sits in a handful of
//        them.  Points outside the grid are clamped into its boundary cells;
//     b. targets and queries sorted by cell key (cell_list.h); the sorted queries make neighbouring lanes scan the same cells;
//     c. ring scan (k_kn_ring_scan): one wave per workgroup, one query per thread.  The thread's candidate list lives in LDS, column-major
//        ([slot][lane], one f64 plane and one i32 plane, KN_LD = 65 words per slot: the scan touches consecutive words, and the epilogue's
//        transposed read, slot per lane, is free of bank conflicts as well).  The list is a max-heap under the lexicographic order of (d2, index);
//        the thread keeps its root, the worst entry, in registers; a candidate that is smaller replaces the root and sinks.  The cube of cells
//        [c - r, c + r] grows by ONE ring at a time and only the new shell is visited, so that no target is inserted twice.  A query is
//        CERTIFIED when its list is full and its worst d2 is <= the squared distance to the nearest face of the cube that is not a face of the
//        grid, the faces pulled in by 1e-12 of the coordinates' magnitude (cell_list.h's grid_face_bound has the argument): a target outside the cube
//        is then strictly farther than the list's worst, and cannot tie with it.  A cube that covers the grid ends the scan unconditionally.  A query
//        that has seen more than KN_RING_WORK targets (crowded cells) or passed ring KN_RING_MAX (far from every target) goes onto a list;
//     d. sweep (k_kn_sweep): the queries on that list against ALL targets, staged through LDS in chunks of KN_CHUNK, the same list per thread,
//        no certificate needed;
//     e. epilogue of both kernels: each thread orders its list by (d2, index) in LDS, then the wave writes the rows co-operatively, lanes j < k
//        the k contiguous entries of one query after the other.
//     The set of the k smallest pairs (d2, index) under the lexicographic order and its ascending order depend on neither the scan order nor the
//     grid, so both outputs equal the brute-force f64 scan followed by a stable sort, bit for bit.
//   pdhip_sor_filter
//     mean_d[i] = (sum over slots 1 .. kk - 1 of sqrt(d2[i][slot])) / (kk - 1), sequentially; mu and sigma over a fixed tree that is a function of N
//     alone (per-thread strided sums, workgroup tree, one workgroup over the partials), two passes; keep = mean_d <= mu + ratio sigma; the kept
//     indices by an exclusive scan (radix_sort.h).
// No floating-point atomics: two calls give equal bytes.  Compiled with -ffp-contract=off.  Every kernel keeps zero scratch.
#include "common.h"
#include "cell_list.h"
#include <math.h>
#include <limits.h>
#include <algorithm>
using namespace pdhip;

namespace {

constexpr int KN_T = 64;                      // one wave per workgroup, one query per thread
constexpr int KN_LD = 65;                     // words between two slots of the column-major list
constexpr int KN_KMAX = 64;                   // (lanes j < k write a row: k <= the wave)
constexpr int KN_CHUNK = 512;                 // targets staged at a time by the sweep: 8 KiB beside the list's 12 * 65 * k bytes
constexpr int KN_CELLS_MAX = 128;             // cells per axis
constexpr int KN_CELLS_HOOK = 64;             // ... that the test hook may ask for
constexpr int KN_RING_MAX = 8;                // the ring scan gives up after the cube [c - 8, c + 8], or after KN_RING_WORK targets (crowded cells)
constexpr int KN_RING_WORK = 4096;
constexpr int KN_NMAX = 1 << 26;
constexpr int KN_HB = 1024;                   // bins per axis of the targets' coordinate histograms
constexpr double KN_TRIM = 0.01;              // the grid spans the targets between these quantiles of every axis ...
constexpr double KN_TRIM_PAD = 0.1;           // ... widened by this share of that span on either side
constexpr int SOR_T = 256;
constexpr int SOR_NB = 256;                   // workgroups of the reductions (== SOR_T: one finalize workgroup reads them all)
enum { MISC_FAR = 2 * BOX_WORDS, MISC_WORDS = 32 };                // behind the two boxes (cell_list.h)

// a. hist[a][b] = targets whose coordinate a falls into bin b of KN_HB equal bins over the targets' box (read from the device: k_point_box ran
// before on the same stream).  Integer atomics only
__global__ __launch_bounds__(CL_T) void k_kn_axis_hist(const float* __restrict__ P, int n, const uint32_t* __restrict__ box, uint32_t* __restrict__ hist) {
    __shared__ uint32_t sh[3 * KN_HB];
    const int t = threadIdx.x;
    for (int j = t; j < 3 * KN_HB; j += CL_T) sh[j] = 0u;
    __syncthreads();
    double mn[3], sc[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        mn[a] = (double)ord2f(box[BOX_MIN + a]);
        const double ext = (double)ord2f(box[BOX_MAX + a]) - mn[a];
        sc[a] = ext > 0.0 ? (double)KN_HB / ext : 0.0;
    }
    for (long long i = (long long)blockIdx.x * CL_T + t; i < n; i += (long long)gridDim.x * CL_T) {
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const float x = P[3 * i + a];
            if (!(fabsf(x) <= 3.4028234e38f)) continue;
            const int b = (int)fmin(fmax(floor(((double)x - mn[a]) * sc[a]), 0.0), (double)(KN_HB - 1));       // (fmax(NaN, 0) = 0)
            atomicAdd(&sh[a * KN_HB + b], 1u);
        }
    }
    __syncthreads();
    for (int j = t; j < 3 * KN_HB; j += CL_T)
        if (sh[j]) atomicAdd(&hist[j], sh[j]);
}

// ---------------------------------------------------------------------------------------------------------------------------
// the candidate list of one thread: sd / si point at the thread's column (slot j at [j * KN_LD]); cnt entries are filled; once cnt == k,
// (wd, wi) at slot ws is the lexicographically largest entry
struct KnList {
    double* sd;
    int* si;
    int k, cnt, wi;
    double wd;
};

__device__ __forceinline__ KnList kn_list(double* lds, int k, int t) {
    return KnList{lds + t, reinterpret_cast<int*>(lds + KN_LD * k) + t, k, 0, INT_MAX, 1.0e300};
}

// the pair (d, i) into the max-heap at slots [0, k), from slot p downwards: a child that is larger moves up, the pair settles where none is
__device__ __forceinline__ void kn_sift(KnList& l, int p, double d, int i) {
    for (int c = 2 * p + 1; c < l.k; c = 2 * p + 1) {
        double cd = l.sd[c * KN_LD];
        int ci = l.si[c * KN_LD];
        if (c + 1 < l.k) {
            const double ed = l.sd[(c + 1) * KN_LD];
            const int ei = l.si[(c + 1) * KN_LD];
            if (pair_less(cd, ci, ed, ei)) { ++c; cd = ed; ci = ei; }
        }
        if (!pair_less(d, i, cd, ci)) break;
        l.sd[p * KN_LD] = cd;
        l.si[p * KN_LD] = ci;
        p = c;
    }
    l.sd[p * KN_LD] = d;
    l.si[p * KN_LD] = i;
}

// the first k candidates fill the slots; the k-th makes them a max-heap under the lexicographic order of (d2, index), whose root -- the worst entry
// -- the thread keeps in registers.  A later candidate that is smaller than the root replaces it and sinks: log2 k steps, where a rescan of the
// list for its new worst (k_sr_knn_normals' way) takes k -- and a query far from every target, which the sweep serves, replaces at most targets
__device__ __forceinline__ void kn_offer(KnList& l, double d, int i) {
    if (l.cnt < l.k) {
        l.sd[l.cnt * KN_LD] = d;
        l.si[l.cnt * KN_LD] = i;
        if (++l.cnt < l.k) return;
        for (int p = l.k / 2 - 1; p >= 0; --p) kn_sift(l, p, l.sd[p * KN_LD], l.si[p * KN_LD]);
    } else if (pair_less(d, i, l.wd, l.wi)) {
        kn_sift(l, 0, d, i);
    } else {
        return;
    }
    l.wd = l.sd[0];
    l.wi = l.si[0];
}

__device__ __forceinline__ void kn_scan_run(KnList& l, const float4* __restrict__ st, int b, int e, double qx, double qy, double qz) {
    for (int p = b; p < e; ++p) {
        const float4 a = st[p];
        kn_offer(l, point_d2(qx, qy, qz, a), __float_as_int(a.w));
    }
}

// e. `done` threads (every thread of the wave calls this) order their full lists and the wave writes row `out` of each
__device__ __forceinline__ void kn_epilogue(KnList& l, double* lds, int t, bool done, int out, double* __restrict__ d2, int* __restrict__ idx) {
    const int k = l.k;
    if (done) {
        for (int a = 1; a < k; ++a) {                              // insertion sort by (d2, index)
            const double d = l.sd[a * KN_LD];
            const int i = l.si[a * KN_LD];
            int b = a - 1;
            while (b >= 0) {
                const double e = l.sd[b * KN_LD];
                const int ei = l.si[b * KN_LD];
                if (!(e > d || (e == d && ei > i))) break;
                l.sd[(b + 1) * KN_LD] = e;
                l.si[(b + 1) * KN_LD] = ei;
                --b;
            }
            l.sd[(b + 1) * KN_LD] = d;
            l.si[(b + 1) * KN_LD] = i;
        }
    }
    __syncthreads();
    const int* li = reinterpret_cast<const int*>(lds + KN_LD * k);
    const int mine = done ? out : -1;
    for (int o = 0; o < KN_T; ++o) {
        const int row = __shfl(mine, o);                           // (the same for every lane)
        if (row < 0) continue;
        if (t < k) {
            d2[(size_t)row * k + t] = lds[t * KN_LD + o];
            idx[(size_t)row * k + t] = li[t * KN_LD + o];
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
// c. the ring scan over the Q sorted queries
__global__ __launch_bounds__(KN_T) void k_kn_ring_scan(const float4* __restrict__ sq, int Q, const float4* __restrict__ st,
                                                       const int* __restrict__ cstart, Grid3 g, int k, double* __restrict__ d2,
                                                       int* __restrict__ idx, int* __restrict__ far_list, int* __restrict__ far_n) {
    extern __shared__ double kn_lds[];
    const int t = threadIdx.x;
    const int sp = blockIdx.x * KN_T + t;
    KnList l = kn_list(kn_lds, k, t);
    bool done = false;
    int out = -1;
    if (sp < Q) {
        const float4 me = sq[sp];
        out = __float_as_int(me.w);
        const double qx = (double)me.x, qy = (double)me.y, qz = (double)me.z;
        const int C = g.C;
        const int cx = g.cell(qx, g.ox), cy = g.cell(qy, g.oy), cz = g.cell(qz, g.oz);
        CellCube in{1, 0, 1, 0, 1, 0};                             // the cube already scanned (none yet)
        int work = 0;
        bool giveup = false;
        for (int r = 1; !giveup; ++r) {
            const CellCube q = cube_around(cx, cy, cz, r, C);
            for (int z = q.z0; z <= q.z1 && !giveup; ++z)
                for (int y = q.y0; y <= q.y1 && !giveup; ++y) {
                    const int base = (z * C + y) * C;
                    const bool inner = y >= in.y0 && y <= in.y1 && z >= in.z0 && z <= in.z1;       // the row crosses the scanned cube:
                    int xa[2] = {q.x0, 1}, xb[2] = {q.x1, 0};                                      // only the cells on either side of it
                    if (inner) { xb[0] = in.x0 - 1; xa[1] = in.x1 + 1; xb[1] = q.x1; }
#pragma unroll
                    for (int s = 0; s < 2; ++s) {
                        if (xa[s] > xb[s] || giveup) continue;
                        const int b = cstart[base + xa[s]], e = cstart[base + xb[s] + 1];
                        work += e - b;
                        if (work > KN_RING_WORK) { giveup = true; continue; }                      // crowded cells: the sweep is the cheaper way
                        kn_scan_run(l, st, b, e, qx, qy, qz);
                    }
                }
            if (giveup) break;
            const double b = grid_cube_bound(g, qx, qy, qz, q);
            if (q.covers(C) || (l.cnt == k && b > 0.0 && l.wd <= b * b)) { done = true; break; }
            if (r >= KN_RING_MAX) giveup = true;                   // far from every target: a thread of its own would scan most of the grid
            in = q;
        }
        if (giveup) far_list[atomicAdd(far_n, 1)] = sp;
    }
    kn_epilogue(l, kn_lds, t, done, out, d2, idx);
}

// d. the queries far_list[0 .. *far_n) (far_list == nullptr: all Q sorted queries) against every target.  The targets are taken in the order
// (j * stride) mod M, not in cell order: a far query that walks the cells towards itself would replace its worst entry at most targets, where a
// scattered order replaces it about k ln(M / k) times
__global__ __launch_bounds__(KN_T) void k_kn_sweep(const float4* __restrict__ sq, const int* __restrict__ far_list, const int* __restrict__ far_n,
                                                   int Q, const float4* __restrict__ st, int M, int stride, int k, double* __restrict__ d2,
                                                   int* __restrict__ idx) {
    extern __shared__ double kn_lds[];
    __shared__ float4 s_t[KN_CHUNK];
    const int t = threadIdx.x;
    const int n = far_list != nullptr ? min(*far_n, Q) : Q;
    if ((int)blockIdx.x * KN_T >= n) return;                       // (the whole workgroup)
    const int i = blockIdx.x * KN_T + t;
    const bool have = i < n;
    KnList l = kn_list(kn_lds, k, t);
    double qx = 0.0, qy = 0.0, qz = 0.0;
    int out = -1;
    if (have) {
        const float4 me = sq[far_list != nullptr ? far_list[i] : i];
        qx = (double)me.x; qy = (double)me.y; qz = (double)me.z;
        out = __float_as_int(me.w);
    }
    for (int base = 0; base < M; base += KN_CHUNK) {
        const int nc = min(KN_CHUNK, M - base);
        __syncthreads();
        for (int j = t; j < nc; j += KN_T) s_t[j] = st[(int)(((long long)(base + j) * stride) % M)];      // (a bijection of [0, M): gcd(stride, M) = 1)
        __syncthreads();
        if (have) kn_scan_run(l, s_t, 0, nc, qx, qy, qz);
    }
    kn_epilogue(l, kn_lds, t, have, out, d2, idx);                 // (k <= M: the list is full)
}

// ---------------------------------------------------------------------------------------------------------------------------
// statistical outlier removal
__global__ __launch_bounds__(SOR_T) void k_sor_check(const double* __restrict__ d2, long long n, uint32_t* __restrict__ bad) {
    uint32_t c = 0u;
    for (long long i = (long long)blockIdx.x * SOR_T + threadIdx.x; i < n; i += (long long)gridDim.x * SOR_T) {
        const double d = d2[i];
        if (!(d >= 0.0 && d <= 1.7976931348623157e308)) ++c;
    }
    for (int off = 32; off > 0; off >>= 1) c += (uint32_t)__shfl_xor((int)c, off);
    if ((threadIdx.x & 63) == 0 && c) atomicAdd(bad, c);
}

__global__ __launch_bounds__(SOR_T) void k_sor_mean(const double* __restrict__ d2, int N, int kk, double* __restrict__ mean_d) {
    const int i = blockIdx.x * SOR_T + threadIdx.x;
    if (i >= N) return;
    const double* row = d2 + (size_t)i * kk;
    double s = 0.0;
    for (int j = 1; j < kk; ++j) s += sqrt(row[j]);
    mean_d[i] = s / (double)(kk - 1);
}

// part[block] = sum over the block's strided elements of x (pass 0) or (x - *mu)^2 (pass 1): a fixed tree
__global__ __launch_bounds__(SOR_T) void k_sor_reduce(const double* __restrict__ x, int N, int pass, const double* __restrict__ stats,
                                                      double* __restrict__ part) {
    __shared__ double sh[SOR_T];
    const int t = threadIdx.x;
    const double mu = pass ? stats[0] : 0.0;
    double s = 0.0;
    for (long long i = (long long)blockIdx.x * SOR_T + t; i < N; i += (long long)gridDim.x * SOR_T) {
        const double v = x[i];
        if (pass) { const double c = v - mu; s += c * c; }
        else s += v;
    }
    sh[t] = s;
    __syncthreads();
    for (int off = SOR_T / 2; off > 0; off >>= 1) {
        if (t < off) sh[t] = sh[t] + sh[t + off];
        __syncthreads();
    }
    if (t == 0) part[blockIdx.x] = sh[0];
}

// pass 0: stats[0] = mu; pass 1: stats[1] = sigma, stats[2] = t, stats[3] = 0
__global__ __launch_bounds__(SOR_T) void k_sor_finalize(const double* __restrict__ part, int nb, int N, int pass, double std_ratio,
                                                        double* __restrict__ stats) {
    __shared__ double sh[SOR_T];
    const int t = threadIdx.x;
    sh[t] = t < nb ? part[t] : 0.0;
    __syncthreads();
    for (int off = SOR_T / 2; off > 0; off >>= 1) {
        if (t < off) sh[t] = sh[t] + sh[t + off];
        __syncthreads();
    }
    if (t != 0) return;
    if (!pass) {
        stats[0] = sh[0] / (double)N;
    } else {
        const double sd = sqrt(sh[0] / (double)(N - 1));
        stats[1] = sd;
        stats[2] = stats[0] + std_ratio * sd;
        stats[3] = 0.0;
    }
}

__global__ __launch_bounds__(SOR_T) void k_sor_keep(const double* __restrict__ mean_d, int N, const double* __restrict__ stats,
                                                    uint8_t* __restrict__ keep, int* __restrict__ flag) {
    const int i = blockIdx.x * SOR_T + threadIdx.x;
    if (i >= N) return;
    const int f = mean_d[i] <= stats[2] ? 1 : 0;
    keep[i] = (uint8_t)f;
    flag[i] = f;
}

__global__ __launch_bounds__(SOR_T) void k_sor_compact(const int* __restrict__ flag, const int* __restrict__ pos, int N,
                                                       int32_t* __restrict__ kept_idx, int32_t* __restrict__ counts) {
    const int i = blockIdx.x * SOR_T + threadIdx.x;
    if (i >= N) return;
    if (flag[i]) kept_idx[pos[i]] = i;
    if (i == N - 1) {
        const int kept = pos[i] + flag[i];
        counts[0] = kept; counts[1] = N - kept; counts[2] = 0; counts[3] = 0;
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
static double kn_occupancy(int k) { return std::max(8.0, 0.5 * (double)k); }
static int kn_cells_axis(int M, int k) { return std::max(1, std::min(KN_CELLS_MAX, (int)floor(sqrt((double)M / kn_occupancy(k))))); }
// (the cell starts are sized for k = 1, the finest grid, and for every grid the hook may ask for: the size grows with Q and M and not with k)
static size_t kn_cells_cap(int M) { return (size_t)std::max(kn_cells_axis(M, 1), KN_CELLS_HOOK); }
static size_t kn_lds_bytes(int k) { return (size_t)KN_LD * k * (sizeof(double) + sizeof(int)); }

struct KnnWs {
    SortBufs sb;
    float4 *st, *sq;
    int *cstart, *far_list;
    uint32_t* misc;                                                // box of the targets, box of the queries, the sweep's counter
    uint32_t* hist;                                                // the targets' coordinate histograms, [3][KN_HB]
};
static size_t carve_knn(KnnWs& w, void* base, int Q, int M) {
    Carve c{static_cast<char*>(base), 0};
    const size_t C = kn_cells_cap(M);
    carve_sort(c, w.sb, (size_t)std::max(Q, M));
    w.st = c.take<float4>((size_t)M);
    w.sq = c.take<float4>((size_t)Q);
    w.cstart = c.take<int>(C * C * C + 1);
    w.far_list = c.take<int>((size_t)Q);
    w.misc = c.take<uint32_t>(MISC_WORDS);
    w.hist = c.take<uint32_t>(3 * KN_HB);
    return c.off + 256;
}

// the span of one axis that the grid is laid over: [mn, mx] cut to the bins between the KN_TRIM and 1 - KN_TRIM quantiles of the targets, widened
// by KN_TRIM_PAD of that span on either side, never beyond [mn, mx].  A few points far outside then no longer decide the size of the cells: they
// are clamped into the boundary cells.  Fewer than 1 / KN_TRIM targets: the whole box
static void kn_trimmed_span(const uint32_t* h, int M, double mn, double mx, double& lo, double& hi) {
    lo = mn; hi = mx;
    const long long trim = (long long)floor(KN_TRIM * (double)M);
    if (!(mx > mn) || trim < 1) return;
    int b0 = 0, b1 = KN_HB - 1;
    long long acc = 0;
    while (b0 < KN_HB - 1 && acc + h[b0] <= trim) acc += h[b0++];
    acc = 0;
    while (b1 > b0 && acc + h[b1] <= trim) acc += h[b1--];
    const double w = (mx - mn) / (double)KN_HB;
    const double a = mn + (double)b0 * w, b = mn + (double)(b1 + 1) * w, pad = KN_TRIM_PAD * (b - a);
    lo = std::max(mn, a - pad);
    hi = std::min(mx, b + pad);
}

struct SorWs {
    int *flag, *pos, *tsum, *toff;
    double* part;
    uint32_t* bad;
};
static size_t carve_sor(SorWs& w, void* base, int N) {
    Carve c{static_cast<char*>(base), 0};
    w.flag = c.take<int>((size_t)N);
    w.pos = c.take<int>((size_t)N);
    w.tsum = c.take<int>(scan_tiles((size_t)N));
    w.toff = c.take<int>(scan_tiles((size_t)N));
    w.part = c.take<double>(SOR_NB);
    w.bad = c.take<uint32_t>(1);
    return c.off + 256;
}

}  // namespace

// tuning / test hook: cells_per_axis 0 = the grid follows M and k, 1 .. 64: that many; path 0 = ring scan, then the sweep for the queries it gave
// up, 1 = the sweep for every query, 2 = as 0 with the grid over the targets' whole box (no quantile cut).  Same results under every setting.
static thread_local int g_knn_cells = 0, g_knn_path = 0;
extern "C" int pdhip_debug_set_knn(int cells_per_axis, int path) {
    const int old = 4 * g_knn_cells + g_knn_path;
    if (cells_per_axis < 0 || cells_per_axis > KN_CELLS_HOOK || path < 0 || path > 2) return -1;
    g_knn_cells = cells_per_axis;
    g_knn_path = path;
    return old;
}
extern "C" int pdhip_knn_max_k(void) { return KN_KMAX; }
extern "C" size_t pdhip_knn_lds_bytes(int k) { return k >= 1 && k <= KN_KMAX ? kn_lds_bytes(k) : 0; }

extern "C" size_t pdhip_knn_points_workspace_bytes(int Q, int M, int k) {
    if (Q < 0 || M < 1 || Q > KN_NMAX || M > KN_NMAX || k < 1 || k > KN_KMAX || k > M) return 0;
    KnnWs w;
    return carve_knn(w, nullptr, Q, M);
}

extern "C" int pdhip_knn_points(const float* queries, int Q, const float* targets, int M, int k, double* d2, int32_t* idx, int32_t* counts, void* ws,
                                void* stream) {
    PD_REQUIRE(Q >= 0 && Q <= KN_NMAX, "pdhip_knn_points: Q=%d queries, need 0 .. 2^26", Q);
    PD_REQUIRE(M >= 1 && M <= KN_NMAX, "pdhip_knn_points: M=%d targets, need 1 .. 2^26", M);
    PD_REQUIRE(k >= 1 && k <= KN_KMAX, "pdhip_knn_points: k=%d neighbours, need 1 .. %d", k, KN_KMAX);
    PD_REQUIRE(k <= M, "pdhip_knn_points: k=%d neighbours of M=%d targets, need k <= M", k, M);
    PD_REQUIRE(targets != nullptr, "pdhip_knn_points: null pointer (targets)");
    PD_REQUIRE(counts != nullptr, "pdhip_knn_points: null pointer (counts)");
    PD_REQUIRE(ws != nullptr, "pdhip_knn_points: null pointer (ws)");
    PD_REQUIRE(Q == 0 || queries != nullptr, "pdhip_knn_points: null pointer (queries)");
    PD_REQUIRE(Q == 0 || d2 != nullptr, "pdhip_knn_points: null pointer (d2)");
    PD_REQUIRE(Q == 0 || idx != nullptr, "pdhip_knn_points: null pointer (idx)");
    hipStream_t s = as_stream(stream);
    if (Q == 0) {
        PD_HIP(hipMemsetAsync(counts, 0, 4 * sizeof(int32_t), s));
        return PDHIP_OK;
    }
    KnnWs w;
    carve_knn(w, ws, Q, M);
    // a. the boxes, finiteness of both clouds
    int rc = launch_cloud_boxes(targets, M, queries, Q, w.misc, MISC_WORDS, s);
    if (rc) return rc;
    const bool trimmed = g_knn_path != 2;
    static thread_local uint32_t h_hist[3 * KN_HB];
    if (trimmed) {
        PD_HIP(hipMemsetAsync(w.hist, 0, sizeof(h_hist), s));
        k_kn_axis_hist<<<std::min(cdiv(M, CL_T), 1024), CL_T, 0, s>>>(targets, M, w.misc, w.hist);
        PD_LAUNCH_CHECK();
        PD_HIP(hipMemcpyAsync(h_hist, w.hist, sizeof(h_hist), hipMemcpyDeviceToHost, s));       // (arrives with the boxes: one synchronisation)
    }
    HostBox box[2];                                                // targets, queries
    rc = read_cloud_boxes("pdhip_knn_points", w.misc, box, s);
    if (rc) return rc;
    // the grid covers the part of the targets' span (their box between the outer quantiles of every axis) that the queries' box meets, or the whole
    // span if they do not meet
    double t0[3], t1[3], mn[3];
    for (int a = 0; a < 3; ++a) {
        t0[a] = box[0].mn[a]; t1[a] = box[0].mx[a];
        if (trimmed) kn_trimmed_span(h_hist + a * KN_HB, M, box[0].mn[a], box[0].mx[a], t0[a], t1[a]);
    }
    const double ext = meet_boxes(t0, t1, box[1], mn);
    const Grid3 g = grid_over(mn, ext, g_knn_cells >= 1 ? g_knn_cells : kn_cells_axis(M, k));
    const int nc = g.C * g.C * g.C;
    // b. both clouds in cell order
    int cur = sort_by_cell(w.sb, M, GridPointKey{targets, g}, (unsigned long long)nc, w.cstart, s);
    k_gather_xyzi<<<cdiv(M, CL_T), CL_T, 0, s>>>(w.sb.v[cur], targets, M, w.st);
    cur = sort_by_cell(w.sb, Q, GridPointKey{queries, g}, (unsigned long long)nc, nullptr, s);       // (the queries need the order only)
    k_gather_xyzi<<<cdiv(Q, CL_T), CL_T, 0, s>>>(w.sb.v[cur], queries, Q, w.sq);
    PD_LAUNCH_CHECK();
    // c, d, e.
    int* far_n = reinterpret_cast<int*>(w.misc + MISC_FAR);
    const int all_swept = g_knn_path == 1;
    const size_t lds = kn_lds_bytes(k);
    if (!all_swept) k_kn_ring_scan<<<cdiv(Q, KN_T), KN_T, lds, s>>>(w.sq, Q, w.st, w.cstart, g, k, d2, idx, w.far_list, far_n);
    int stride = 1;
    for (int p : {7919, 7907, 7901, 7883})                         // (primes: one of them does not divide M <= 2^26 < 7919 * 7907)
        if (M % p != 0) { stride = p; break; }
    k_kn_sweep<<<cdiv(Q, KN_T), KN_T, lds, s>>>(w.sq, all_swept ? nullptr : w.far_list, far_n, Q, w.st, M, stride, k, d2, idx);
    k_split_counts<<<1, 1, 0, s>>>(far_n, Q, g.C, all_swept, counts);
    PD_LAUNCH_CHECK();
    return PDHIP_OK;
}

extern "C" size_t pdhip_sor_filter_workspace_bytes(int N) {
    if (N < 2 || N > KN_NMAX) return 0;
    SorWs w;
    return carve_sor(w, nullptr, N);
}

extern "C" int pdhip_sor_filter(const double* knn_d2, int N, int kk, double std_ratio, double* mean_d, double* stats, uint8_t* keep,
                                int32_t* kept_idx, int32_t* counts, void* ws, void* stream) {
    PD_REQUIRE(N >= 2 && N <= KN_NMAX, "pdhip_sor_filter: N=%d points, need 2 .. 2^26", N);
    PD_REQUIRE(kk >= 2 && kk <= KN_KMAX, "pdhip_sor_filter: kk=%d columns (the point itself and its neighbours), need 2 .. %d", kk, KN_KMAX);
    PD_REQUIRE(std_ratio >= 0.0 && std_ratio <= 1.7976931348623157e308, "pdhip_sor_filter: std_ratio=%g, need a finite value >= 0", std_ratio);
    PD_REQUIRE(knn_d2 != nullptr, "pdhip_sor_filter: null pointer (knn_d2)");
    PD_REQUIRE(mean_d != nullptr, "pdhip_sor_filter: null pointer (mean_d)");
    PD_REQUIRE(stats != nullptr, "pdhip_sor_filter: null pointer (stats)");
    PD_REQUIRE(keep != nullptr, "pdhip_sor_filter: null pointer (keep)");
    PD_REQUIRE(kept_idx != nullptr, "pdhip_sor_filter: null pointer (kept_idx)");
    PD_REQUIRE(counts != nullptr, "pdhip_sor_filter: null pointer (counts)");
    PD_REQUIRE(ws != nullptr, "pdhip_sor_filter: null pointer (ws)");
    hipStream_t s = as_stream(stream);
    SorWs w;
    carve_sor(w, ws, N);
    const int nb = std::min(SOR_NB, cdiv(N, SOR_T));               // (a function of N alone: the tree is the same on every call)
    uint32_t bad = 0u;
    PD_HIP(hipMemsetAsync(w.bad, 0, sizeof(uint32_t), s));
    k_sor_check<<<std::min(cdiv((long long)N * kk, SOR_T), 1024), SOR_T, 0, s>>>(knn_d2, (long long)N * kk, w.bad);
    PD_LAUNCH_CHECK();
    PD_HIP(hipMemcpyAsync(&bad, w.bad, sizeof(bad), hipMemcpyDeviceToHost, s));
    PD_HIP(hipStreamSynchronize(s));
    PD_REQUIRE(bad == 0, "pdhip_sor_filter: %u negative or non-finite squared distance(s) in knn_d2", bad);
    k_sor_mean<<<cdiv(N, SOR_T), SOR_T, 0, s>>>(knn_d2, N, kk, mean_d);
    for (int pass = 0; pass < 2; ++pass) {
        k_sor_reduce<<<nb, SOR_T, 0, s>>>(mean_d, N, pass, stats, w.part);
        k_sor_finalize<<<1, SOR_T, 0, s>>>(w.part, nb, N, pass, std_ratio, stats);
    }
    k_sor_keep<<<cdiv(N, SOR_T), SOR_T, 0, s>>>(mean_d, N, stats, keep, w.flag);
    scan_exclusive<int>(w.flag, w.pos, N, w.tsum, w.toff, s);
    k_sor_compact<<<cdiv(N, SOR_T), SOR_T, 0, s>>>(w.flag, w.pos, N, kept_idx, counts);
    PD_LAUNCH_CHECK();
    return PDHIP_OK;
}
