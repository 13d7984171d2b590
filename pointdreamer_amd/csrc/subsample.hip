// Farthest-point subsampling of a cloud on the device, and the mean colour of the points each sample stands for.  The reference ships no subsampler
// (demo.py:371-374 refuses clouds above 30 000 points and asks for one); its only sampling code, models/POCO/lightconvpoint/src sampling_fps, is
// never built by its installer.
//
//   pdhip_fps        idx[0] = start, min_d2[0] = +inf; after pick k every unselected point i carries mind[i] = min over the picks so far of d2(i, pick),
//                    d2 = (dx dx + dy dy) + dz dz with the f32 inputs widened to f64, op by op (pdhip_nearest_points' convention); pick k + 1 is the
//                    unselected point with the largest mind (the smallest original index on a tie), min_d2[k + 1] that value.
//     a. the box and a finiteness test (cell_list.h; one small read that synchronises the stream); a uniform grid of C^3 cells (cell_list.h's Grid3), C ~ cbrt(N / 32) <= 40;
//     b. the points sorted by cell key, cstart, the sorted (x, y, z, index) copy (cell_list.h);
//     c. k_fps_init: mind against `start` (-1 marks a selected point); k_fps_cells, a wave per cell: the TIGHT box of the cell's own points and the
//        cell's entry (largest mind among its unselected points, tag = original index << 32 | sorted position of the smallest index that attains it);
//     d. k_fps_picks, ONE workgroup of 1024 threads, __syncthreads only: per pick
//          - the entries of the groups of FPS_G consecutive cells that changed are recomputed, a wave per group, into LDS; the arg-max over the <= 1024
//            group entries (value, then smaller tag) is the pick s, its value R^2;
//          - only points with d2(i, s) < mind[i] <= R^2 change, and they lie in the cube of cells that [s - R, s + R] reaches.  A wave tests 64 cells of
//            the cube at a time, a cell per lane; a cell is skipped when its lower bound is >= its entry (fps_lower_bound has the argument why that is
//            exact); every other cell is updated and its entry recomputed by the whole wave.  The cell of s is always taken: s leaves its entry.
//        Neither the minimum nor the arg-max depends on the order in which cells and points are visited, so the result equals the brute-force scan bit
//        for bit.  A launch per pick would be host-bound at 30 000 picks, and a loop over several workgroups needs a grid-wide barrier, which hangs
//        the device when the workgroups are not co-resident: neither is built.
//   pdhip_owner_mean_colors
//        per sample and channel the integer sum of llrint(c 2^32) over the points it owns and their count (integer atomics), out = (sum / count) / 2^32
//        in f64, rounded to f32; a sample that owns nothing takes its fallback colour.  Exact and independent of the order.
// No floating-point atomics: two calls give equal bytes.  Compiled with -ffp-contract=off.  Every kernel keeps zero scratch.
#include "common.h"
#include "cell_list.h"
#include <math.h>
#include <limits.h>
#include <algorithm>
using namespace pdhip;

namespace {

constexpr int FPS_NMAX = 1 << 24;
constexpr int FPS_T = 1024;                   // threads of the pick loop: 16 waves
constexpr int FPS_WAVES = FPS_T / 64;
constexpr int FPS_G = 64;                     // cells per group: a wave recomputes a group's entry, a lane per cell
constexpr int FPS_U = 4;                      // points per lane and step of a cell's update
constexpr int FPS_CELLS_MAX = 40;             // cells per axis: 40^3 cells are 1000 groups, one per thread of the pick loop
constexpr double FPS_OCC = 32.0;              // C = cbrt(N / FPS_OCC)
constexpr int OMC_NMAX = 1 << 26;
enum { MISC_OCC = BOX_WORDS, MISC_WORDS = 16 };               // behind the box (cell_list.h)

// an entry: the largest value, and of those that attain it the smallest tag.  (-1, ~0) is the entry of nothing: every mind is >= 0
struct Entry {
    double v;
    unsigned long long tag;
};
__device__ __forceinline__ void entry_take(Entry& a, double v, unsigned long long tag) {
    if (v > a.v || (v == a.v && tag < a.tag)) { a.v = v; a.tag = tag; }
}
__device__ __forceinline__ Entry entry_wave(Entry a) {             // the entry of the 64 lanes' entries, in every lane
    for (int off = 32; off > 0; off >>= 1) {
        const double v = __shfl_xor(a.v, off);
        const unsigned long long tag = __shfl_xor(a.tag, off);
        entry_take(a, v, tag);
    }
    return a;
}

__device__ __forceinline__ double fps_d2(double ax, double ay, double az, double bx, double by, double bz) {
    const double dx = ax - bx, dy = ay - by, dz = az - bz;
    return (dx * dx + dy * dy) + dz * dz;
}

// A lower bound of d2(i, s) over the points i of a cell with the tight box [lo, hi] (the min / max of the members' own coordinates): per axis the gap
// from s to the box, 0 inside, squared and summed in the order of d2.  It never exceeds a member's COMPUTED d2: with s below the box the gap is
// fl(lo - s) and the member's |dx| is fl(x - s) with x >= lo -- the same subtraction from a coordinate that is no smaller, and rounding is monotone
// (above the box alike with hi; inside, 0 <= anything); squaring non-negative numbers, and each of the two additions, are monotone in every operand
// too.  So when the bound is >= the cell's entry, no member has d2 < mind: the cell is provably unchanged, and skipping it changes no bit.
__device__ __forceinline__ double fps_lower_bound(double sx, double sy, double sz, const float4& lo, const float4& hi) {
    const double gx = sx < (double)lo.x ? (double)lo.x - sx : (sx > (double)hi.x ? sx - (double)hi.x : 0.0);
    const double gy = sy < (double)lo.y ? (double)lo.y - sy : (sy > (double)hi.y ? sy - (double)hi.y : 0.0);
    const double gz = sz < (double)lo.z ? (double)lo.z - sz : (sz > (double)hi.z ? sz - (double)hi.z : 0.0);
    return (gx * gx + gy * gy) + gz * gz;
}

// ---------------------------------------------------------------------------------------------------------------------------
// c. mind against `start`
__global__ __launch_bounds__(CL_T) void k_fps_init(const float4* __restrict__ sp, int N, const float* __restrict__ P, int start,
                                                   double* __restrict__ mind) {
    const int p = blockIdx.x * CL_T + threadIdx.x;
    if (p >= N) return;
    const float4 a = sp[p];
    if (__float_as_int(a.w) == start) {
        mind[p] = -1.0;
        return;
    }
    mind[p] = fps_d2((double)a.x, (double)a.y, (double)a.z, (double)P[3 * (size_t)start], (double)P[3 * (size_t)start + 1],
                     (double)P[3 * (size_t)start + 2]);
}

// the tight box and the entry of every cell (ncp >= nc cells, the padding of the last group included: an empty cell has the entry of nothing)
__global__ __launch_bounds__(CL_T) void k_fps_cells(const float4* __restrict__ sp, const double* __restrict__ mind, const int* __restrict__ cstart,
                                                    int nc, int ncp, double* __restrict__ cmax, unsigned long long* __restrict__ ctag,
                                                    float4* __restrict__ cbox) {
    const int c = blockIdx.x * (CL_T / 64) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (c >= ncp) return;                                           // (the whole wave)
    const int b = c < nc ? cstart[c] : 0, e = c < nc ? cstart[c + 1] : 0;
    Entry en{-1.0, ~0ull};
    float lx = INFINITY, ly = INFINITY, lz = INFINITY, hx = -INFINITY, hy = -INFINITY, hz = -INFINITY;
    for (int p = b + lane; p < e; p += 64) {
        const float4 a = sp[p];
        lx = fminf(lx, a.x); ly = fminf(ly, a.y); lz = fminf(lz, a.z);
        hx = fmaxf(hx, a.x); hy = fmaxf(hy, a.y); hz = fmaxf(hz, a.z);
        const double m = mind[p];
        if (m >= 0.0) entry_take(en, m, ((unsigned long long)(uint32_t)__float_as_int(a.w) << 32) | (uint32_t)p);
    }
    for (int off = 32; off > 0; off >>= 1) {
        lx = fminf(lx, __shfl_xor(lx, off)); ly = fminf(ly, __shfl_xor(ly, off)); lz = fminf(lz, __shfl_xor(lz, off));
        hx = fmaxf(hx, __shfl_xor(hx, off)); hy = fmaxf(hy, __shfl_xor(hy, off)); hz = fmaxf(hz, __shfl_xor(hz, off));
    }
    en = entry_wave(en);
    if (lane == 0) {
        cmax[c] = en.v;
        ctag[c] = en.tag;
        cbox[2 * (size_t)c] = make_float4(lx, ly, lz, 0.0f);
        cbox[2 * (size_t)c + 1] = make_float4(hx, hy, hz, 0.0f);
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
// d. the pick loop.  mind, cmax and ctag are written by one wave and read by another after a __syncthreads: no __restrict__ on them
__global__ __launch_bounds__(FPS_T) void k_fps_picks(const float4* __restrict__ sp, int N, int M, int start, const int* __restrict__ cstart,
                                                     const float4* __restrict__ cbox, Grid3 g, int ng, double* mind, double* cmax,
                                                     unsigned long long* ctag, const uint32_t* __restrict__ misc, int32_t* __restrict__ idx,
                                                     double* __restrict__ min_d2, int32_t* __restrict__ counts) {
    __shared__ double s_gv[FPS_T];
    __shared__ unsigned long long s_gt[FPS_T];
    __shared__ int s_dirty[FPS_T];
    __shared__ int s_list[FPS_T];
    __shared__ double s_pv[FPS_WAVES];
    __shared__ unsigned long long s_pt[FPS_WAVES];
    __shared__ int s_nlist;
    __shared__ unsigned long long s_work;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, C = g.C;
    s_dirty[t] = t < ng;                                            // every group's entry is computed before the first arg-max
    s_gv[t] = -1.0;
    s_gt[t] = ~0ull;
    if (t == 0) {
        s_nlist = 0;
        s_work = 0ull;
        idx[0] = start;
        min_d2[0] = INFINITY;
    }
    unsigned long long work = 0ull;                                 // points evaluated by this wave (the same in every lane)
    __syncthreads();
    for (int k = 1; k < M; ++k) {
        // the groups that changed
        if (s_dirty[t]) {
            s_list[atomicAdd(&s_nlist, 1)] = t;
            s_dirty[t] = 0;
        }
        __syncthreads();
        const int nlist = s_nlist;
        for (int j = wave; j < nlist; j += FPS_WAVES) {
            const int gi = s_list[j], c = gi * FPS_G + lane;
            const Entry en = entry_wave(Entry{cmax[c], ctag[c]});
            if (lane == 0) { s_gv[gi] = en.v; s_gt[gi] = en.tag; }
        }
        __syncthreads();
        // the arg-max over the groups
        {
            const Entry en = entry_wave(Entry{s_gv[t], s_gt[t]});
            if (lane == 0) { s_pv[wave] = en.v; s_pt[wave] = en.tag; }
            if (t == 0) s_nlist = 0;
        }
        __syncthreads();
        Entry pick{-1.0, ~0ull};
#pragma unroll
        for (int w = 0; w < FPS_WAVES; ++w) entry_take(pick, s_pv[w], s_pt[w]);
        const int pos = (int)(uint32_t)(pick.tag & 0xffffffffull);
        if (pos < 0 || pos >= N) return;                            // (never: M <= N leaves an unselected point.  The whole workgroup)
        if (t == 0) {
            idx[k] = (int32_t)(pick.tag >> 32);
            min_d2[k] = pick.v;
            mind[pos] = -1.0;
        }
        if (k == M - 1) break;                                      // (nobody reads the update behind the last pick)
        const float4 sf = sp[pos];
        const double sx = (double)sf.x, sy = (double)sf.y, sz = (double)sf.z;
        __syncthreads();
        // the cube of cells that [s - R, s + R] reaches.  A point that changes has fl(dx dx) <= d2 < R^2 (adding non-negative terms is monotone), so its
        // |x - s| is below R (1 + 2^-52); R is widened by 1e-9 of itself, far more, and Grid3::cell is monotone in x: no such point's cell is left out.
        // A cell too many costs one bound test
        const double R = sqrt(pick.v) * (1.0 + 1.0e-9) + 1.0e-300;
        const int x0 = g.cell(sx - R, g.ox), x1 = g.cell(sx + R, g.ox);
        const int y0 = g.cell(sy - R, g.oy), y1 = g.cell(sy + R, g.oy);
        const int z0 = g.cell(sz - R, g.oz), z1 = g.cell(sz + R, g.oz);
        const int cs_ = (g.cell(sz, g.oz) * C + g.cell(sy, g.oy)) * C + g.cell(sx, g.ox);
        const int nx = x1 - x0 + 1, ny = y1 - y0 + 1, ncube = nx * ny * (z1 - z0 + 1);
        for (int base = 0; base < ncube; base += FPS_T) {           // (cell j of the cube goes to wave j % 16: neighbouring cells, which pass the
            const int j = base + lane * FPS_WAVES + wave;          // test together, are updated by different waves at the same time)
            int c = -1;
            bool take = false;
            if (j < ncube) {
                const int jx = j % nx, jy = (j / nx) % ny, jz = j / (nx * ny);
                c = ((z0 + jz) * C + (y0 + jy)) * C + (x0 + jx);
                if (cstart[c + 1] > cstart[c])
                    take = c == cs_ || fps_lower_bound(sx, sy, sz, cbox[2 * (size_t)c], cbox[2 * (size_t)c + 1]) < cmax[c];
            }
            unsigned long long todo = __ballot(take);
            while (todo) {                                          // (uniform over the wave)
                const int l = __ffsll((long long)todo) - 1;
                todo &= todo - 1ull;
                const int cc = __shfl(c, l);
                const int b = cstart[cc], e = cstart[cc + 1];
                Entry en{-1.0, ~0ull};
                for (int p0 = b + lane; p0 < e; p0 += 64 * FPS_U) {      // FPS_U points per lane with their loads in flight together
                    float4 a[FPS_U];
                    double m[FPS_U];
#pragma unroll
                    for (int u = 0; u < FPS_U; ++u) {
                        const int p = min(p0 + 64 * u, e - 1);
                        a[u] = sp[p];
                        m[u] = mind[p];
                    }
#pragma unroll
                    for (int u = 0; u < FPS_U; ++u) {
                        const int p = p0 + 64 * u;
                        if (p < e && m[u] >= 0.0) {
                            const double d = fps_d2((double)a[u].x, (double)a[u].y, (double)a[u].z, sx, sy, sz);
                            if (d < m[u]) { m[u] = d; mind[p] = d; }
                            entry_take(en, m[u], ((unsigned long long)(uint32_t)__float_as_int(a[u].w) << 32) | (uint32_t)p);
                        }
                    }
                }
                work += (unsigned long long)(e - b);
                en = entry_wave(en);
                if (lane == 0) {
                    cmax[cc] = en.v;
                    ctag[cc] = en.tag;
                    s_dirty[cc / FPS_G] = 1;
                }
            }
        }
        __syncthreads();
    }
    if (lane == 0 && work) atomicAdd(&s_work, work);
    __syncthreads();
    if (t == 0) {
        const unsigned long long total = s_work + (unsigned long long)N;          // (k_fps_init's pass against `start`)
        counts[0] = C;
        counts[1] = (int32_t)misc[MISC_OCC];
        counts[2] = total > (unsigned long long)INT_MAX ? INT_MAX : (int32_t)total;
        counts[3] = 0;
    }
}

// occupied cells: one integer atomic per workgroup
__global__ __launch_bounds__(CL_T) void k_fps_occupied(const int* __restrict__ cstart, int nc, uint32_t* __restrict__ misc) {
    const int c = blockIdx.x * CL_T + threadIdx.x;
    const bool occ = c < nc && cstart[c + 1] > cstart[c];
    const int n = __popcll(__ballot(occ));
    if ((threadIdx.x & 63) == 0 && n) atomicAdd(&misc[MISC_OCC], (uint32_t)n);
}

// ---------------------------------------------------------------------------------------------------------------------------
// mean colours
__global__ __launch_bounds__(CL_T) void k_omc_accum(const int32_t* __restrict__ owner, const float* __restrict__ colors, int N, int M,
                                                    unsigned long long* __restrict__ sums, unsigned long long* __restrict__ cnt,
                                                    uint32_t* __restrict__ bad) {
    const int i = blockIdx.x * CL_T + threadIdx.x;
    if (i >= N) return;
    const int o = owner[i];
    const float r = colors[3 * (size_t)i], gr = colors[3 * (size_t)i + 1], b = colors[3 * (size_t)i + 2];
    if (o < 0 || o >= M) { atomicAdd(&bad[0], 1u); return; }
    if (!(r >= 0.0f && r <= 1.0f) || !(gr >= 0.0f && gr <= 1.0f) || !(b >= 0.0f && b <= 1.0f)) { atomicAdd(&bad[1], 1u); return; }
    atomicAdd(&sums[3 * (size_t)o], (unsigned long long)llrint((double)r * 4294967296.0));
    atomicAdd(&sums[3 * (size_t)o + 1], (unsigned long long)llrint((double)gr * 4294967296.0));
    atomicAdd(&sums[3 * (size_t)o + 2], (unsigned long long)llrint((double)b * 4294967296.0));
    atomicAdd(&cnt[o], 1ull);
}

__global__ __launch_bounds__(CL_T) void k_omc_final(const unsigned long long* __restrict__ sums, const unsigned long long* __restrict__ cnt, int M,
                                                    const float* __restrict__ fallback, float* __restrict__ out) {
    const int j = blockIdx.x * CL_T + threadIdx.x;
    if (j >= 3 * M) return;
    const unsigned long long n = cnt[j / 3];
    out[j] = n == 0ull ? fallback[j] : (float)(((double)(long long)sums[j] / (double)(long long)n) / 4294967296.0);
}

// ---------------------------------------------------------------------------------------------------------------------------
static int cells_axis(int N) { return std::max(1, std::min(FPS_CELLS_MAX, (int)floor(cbrt((double)N / FPS_OCC)))); }

struct FpsWs {
    SortBufs sb;
    float4 *sp, *cbox;
    double *mind, *cmax;
    unsigned long long* ctag;
    int* cstart;
    uint32_t* misc;                                                // the box, the occupied cells
};
static size_t carve_fps(FpsWs& w, void* base, int N) {
    Carve c{static_cast<char*>(base), 0};
    const size_t C = (size_t)FPS_CELLS_MAX;                        // (pdhip_debug_set_fps_cells may ask for any grid up to this one)
    const size_t ncp = (size_t)cdiv((long long)(C * C * C), FPS_G) * FPS_G;
    carve_sort(c, w.sb, (size_t)N);
    w.sp = c.take<float4>((size_t)N);
    w.mind = c.take<double>((size_t)N);
    w.cstart = c.take<int>(C * C * C + 1);
    w.cmax = c.take<double>(ncp);
    w.ctag = c.take<unsigned long long>(ncp);
    w.cbox = c.take<float4>(2 * ncp);
    w.misc = c.take<uint32_t>(MISC_WORDS);
    return c.off + 256;
}

struct OmcWs {
    unsigned long long *sums, *cnt;
    uint32_t* bad;
};
static size_t carve_omc(OmcWs& w, void* base, int M) {
    Carve c{static_cast<char*>(base), 0};
    w.sums = c.take<unsigned long long>(4 * (size_t)M);            // [3 M] sums, [M] counts: cleared by one memset
    w.cnt = w.sums ? w.sums + 3 * (size_t)M : nullptr;
    w.bad = c.take<uint32_t>(2);
    return c.off + 256;
}

}  // namespace

// tuning / test hook: 0 = the cells per axis follow N; 1 .. 40: that many.  Same results under every setting.
static thread_local int g_fps_cells = 0;
extern "C" int pdhip_debug_set_fps_cells(int cells_per_axis) { int old = g_fps_cells; g_fps_cells = cells_per_axis; return old; }

extern "C" size_t pdhip_fps_workspace_bytes(int N, int M) {
    if (N < 1 || N > FPS_NMAX || M < 1 || M > N) return 0;
    FpsWs w;
    return carve_fps(w, nullptr, N);
}

extern "C" int pdhip_fps(const float* points, int N, int M, int start, int32_t* idx, double* min_d2, int32_t* counts, void* ws, void* stream) {
    PD_REQUIRE(points != nullptr, "pdhip_fps: null pointer (points)");
    PD_REQUIRE(idx != nullptr, "pdhip_fps: null pointer (idx)");
    PD_REQUIRE(min_d2 != nullptr, "pdhip_fps: null pointer (min_d2)");
    PD_REQUIRE(counts != nullptr, "pdhip_fps: null pointer (counts)");
    PD_REQUIRE(ws != nullptr, "pdhip_fps: null pointer (ws)");
    PD_REQUIRE(N >= 1 && N <= FPS_NMAX, "pdhip_fps: N=%d points, need 1 .. 2^24", N);
    PD_REQUIRE(M >= 1 && M <= N, "pdhip_fps: M=%d picks, need 1 .. N=%d", M, N);
    PD_REQUIRE(start >= 0 && start < N, "pdhip_fps: start=%d, need 0 .. N-1=%d", start, N - 1);
    hipStream_t s = as_stream(stream);
    FpsWs w;
    carve_fps(w, ws, N);
    // a. the box, finiteness
    int rc = clear_boxes(w.misc, 1, MISC_WORDS, s);
    if (rc) return rc;
    launch_point_box(points, N, w.misc, s);
    PD_LAUNCH_CHECK();
    HostBox box[1];
    rc = read_boxes(w.misc, box, s);
    if (rc) return rc;
    PD_REQUIRE(box[0].bad == 0, "pdhip_fps: %u point(s) with a non-finite coordinate", box[0].bad);
    const Grid3 g = grid_over(box[0].mn, box_extent(box[0].mn, box[0].mx), g_fps_cells >= 1 && g_fps_cells <= FPS_CELLS_MAX ? g_fps_cells : cells_axis(N));
    const int nc = g.C * g.C * g.C, ng = cdiv(nc, FPS_G), ncp = ng * FPS_G;
    // b. the points in cell order
    const int cur = sort_by_cell(w.sb, N, GridPointKey{points, g}, (unsigned long long)nc, w.cstart, s);
    k_gather_xyzi<<<cdiv(N, CL_T), CL_T, 0, s>>>(w.sb.v[cur], points, N, w.sp);
    // c. mind against `start`, the cells' boxes and entries
    k_fps_init<<<cdiv(N, CL_T), CL_T, 0, s>>>(w.sp, N, points, start, w.mind);
    k_fps_cells<<<cdiv(ncp, CL_T / 64), CL_T, 0, s>>>(w.sp, w.mind, w.cstart, nc, ncp, w.cmax, w.ctag, w.cbox);
    k_fps_occupied<<<cdiv(nc, CL_T), CL_T, 0, s>>>(w.cstart, nc, w.misc);
    PD_LAUNCH_CHECK();
    // d. the picks
    k_fps_picks<<<1, FPS_T, 0, s>>>(w.sp, N, M, start, w.cstart, w.cbox, g, ng, w.mind, w.cmax, w.ctag, w.misc, idx, min_d2, counts);
    PD_LAUNCH_CHECK();
    return PDHIP_OK;
}

extern "C" size_t pdhip_owner_mean_colors_workspace_bytes(int M) {
    if (M < 1 || M > OMC_NMAX) return 0;
    OmcWs w;
    return carve_omc(w, nullptr, M);
}

extern "C" int pdhip_owner_mean_colors(const int32_t* owner, const float* colors, int N, int M, const float* fallback, float* out, void* ws_or_null,
                                       void* stream) {
    PD_REQUIRE(N >= 0 && N <= OMC_NMAX, "pdhip_owner_mean_colors: N=%d points, need 0 .. 2^26", N);
    PD_REQUIRE(M >= 1 && M <= OMC_NMAX, "pdhip_owner_mean_colors: M=%d samples, need 1 .. 2^26", M);
    PD_REQUIRE(N == 0 || owner != nullptr, "pdhip_owner_mean_colors: null pointer (owner)");
    PD_REQUIRE(N == 0 || colors != nullptr, "pdhip_owner_mean_colors: null pointer (colors)");
    PD_REQUIRE(fallback != nullptr, "pdhip_owner_mean_colors: null pointer (fallback)");
    PD_REQUIRE(out != nullptr, "pdhip_owner_mean_colors: null pointer (out)");
    hipStream_t s = as_stream(stream);
    void* own = nullptr;
    if (ws_or_null == nullptr) PD_HIP(hipMalloc(&own, pdhip_owner_mean_colors_workspace_bytes(M)));
    OmcWs w;
    carve_omc(w, ws_or_null ? ws_or_null : own, M);
    uint32_t bad[2] = {0u, 0u};
    hipError_t e = hipMemsetAsync(w.sums, 0, 4 * (size_t)M * sizeof(unsigned long long), s);
    if (e == hipSuccess) e = hipMemsetAsync(w.bad, 0, sizeof(bad), s);
    if (e == hipSuccess && N > 0) {
        k_omc_accum<<<cdiv(N, CL_T), CL_T, 0, s>>>(owner, colors, N, M, w.sums, w.cnt, w.bad);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(bad, w.bad, sizeof(bad), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e == hipSuccess && bad[0] == 0 && bad[1] == 0) {
        k_omc_final<<<cdiv(3 * (long long)M, CL_T), CL_T, 0, s>>>(w.sums, w.cnt, M, fallback, out);
        e = hipGetLastError();
        if (e == hipSuccess && own != nullptr) e = hipStreamSynchronize(s);      // (the entry's own workspace is freed below)
    }
    if (own != nullptr) (void)hipFree(own);
    if (e != hipSuccess) {
        set_error("pdhip_owner_mean_colors: %s", hipGetErrorString(e));
        return PDHIP_E_HIP;
    }
    PD_REQUIRE(bad[0] == 0, "pdhip_owner_mean_colors: %u owner(s) outside [0, M=%d)", bad[0], M);
    PD_REQUIRE(bad[1] == 0, "pdhip_owner_mean_colors: %u point(s) with a colour outside [0, 1] or non-finite", bad[1]);
    return PDHIP_OK;
}
