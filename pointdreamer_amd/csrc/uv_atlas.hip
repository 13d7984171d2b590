// UV-atlas unwrapping on the device (the `xatlas.parametrize` half of xatlas_uvmap_w_face_id,
// models/get3d/extract_texture_map.py:42-64): chart segmentation by dominant signed normal axis, orthographic projection per
// chart, shelf packing with one global texel density, and an overlap check that uses the rasteriser's own coverage rules.
//
//   a. face set-up: unit normal, dominant signed axis (labels 0..5 = +x -x +y -y +z -z), degenerate faces (zero / non-finite
//      area, or an index outside [0, Vn)) get label 6;
//   b. edge adjacency: edge keys min * Vn + max, radix-sorted; a key held by exactly two faces joins them;
//   c. label smoothing: Jacobi passes, a face takes the label two of its neighbours share if n.axis >= cos 70;
//   d. charts = connected components of equal labels (union_find.h, over the faces); the chart id is the smallest face index of the
//      component;
//   e. charts of fewer than MERGE_K faces take the label of an adjacent chart whose axis all their faces accept, then d again;
//   f. per-chart projection onto the axis plane, one UV entry per (chart, vertex);
//   g. shelf packing at the largest common scale that fits (one workgroup, one candidate scale per thread), then a coverage
//      count per texel: a chart that covers a texel centre twice is split at the median of its face centroids and the atlas
//      re-packed; after SPLIT_ROUNDS rounds the charts still overlapping become one chart per face.
// No float atomics: bounding boxes are order-preserving integer keys, counts are integer adds, every result is independent of
// scheduling (two calls give identical bytes).  The host reads one word per packing round (overlap / error flags).
// Compiled with -ffp-contract=off.
#include "raster_rules.h"
#include "mesh_common.h"
#include "union_find.h"
#include <algorithm>
using namespace pdhip;

namespace {

constexpr float COS70 = 0.342020143325668733f;
constexpr int DEGEN = 6;
constexpr int MERGE_K = 8;
constexpr int SMOOTH_PASSES = 3;
constexpr int MERGE_ROUNDS = 6;
constexpr int SPLIT_ROUNDS = 8;
constexpr int SINGLE_ROUNDS = 4;     // after SPLIT_ROUNDS: overlapping charts become one chart per face (a re-pack at a smaller scale can
                                     // expose an overlap in a chart checked at the larger one, so the check goes on)
constexpr int FLAG_OVERLAP = 1, ERR_INDEX = 2, ERR_PACK = 4, ERR_STATE = 8;
enum { M_FLAG = 0, M_CHARTS = 1, M_SCALE = 2, M_WORDS = 64 };

// orientation-preserving orthographic projection onto the plane of axis `lab` (u x v = the axis)
__device__ __forceinline__ void axis_proj(int lab, float x, float y, float z, float& u, float& v) {
    switch (lab) {
        case 0: u = y; v = z; break;
        case 1: u = z; v = y; break;
        case 2: u = z; v = x; break;
        case 3: u = x; v = z; break;
        case 4: u = x; v = y; break;
        default: u = y; v = x; break;
    }
}
__device__ __forceinline__ float axis_dot(int lab, float nx, float ny, float nz) {
    const float c = lab < 2 ? nx : (lab < 4 ? ny : nz);
    return (lab & 1) ? -c : c;
}

// ---------------------------------------------------------------------------------------------------------------------------
// a. faces: sanitised int32 indices, unit normals, labels, edge keys
__global__ void k_uva_faces(const float* __restrict__ V, int Vn, const int64_t* __restrict__ faces, int F, int* __restrict__ idx,
                            float* __restrict__ nrm, int* __restrict__ lab, uint64_t* __restrict__ ekey, int* __restrict__ eval,
                            int* __restrict__ misc) {
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= F) return;
    int id[3];
    bool ok = true;
    for (int k = 0; k < 3; ++k) {
        const int64_t a = faces[3 * (size_t)f + k];
        const bool in = index_ok(a, Vn);
        ok = ok && in;
        id[k] = in ? (int)a : 0;
        idx[3 * f + k] = id[k];
    }
    if (!ok) atomicOr(&misc[M_FLAG], ERR_INDEX);
    const double x0 = V[3 * id[0]], y0 = V[3 * id[0] + 1], z0 = V[3 * id[0] + 2];
    const double ax = V[3 * id[1]] - x0, ay = V[3 * id[1] + 1] - y0, az = V[3 * id[1] + 2] - z0;
    const double bx = V[3 * id[2]] - x0, by = V[3 * id[2] + 1] - y0, bz = V[3 * id[2] + 2] - z0;
    const double nx = ay * bz - az * by, ny = az * bx - ax * bz, nz = ax * by - ay * bx;
    const double len = sqrt(nx * nx + ny * ny + nz * nz);
    int L = DEGEN;
    float fx = 0.f, fy = 0.f, fz = 0.f;
    if (ok && len > 0.0 && len <= 1.0e300) {
        fx = (float)(nx / len); fy = (float)(ny / len); fz = (float)(nz / len);
        const float mx = fabsf(fx), my = fabsf(fy), mz = fabsf(fz);
        if (mx >= my && mx >= mz) L = fx < 0.f ? 1 : 0;
        else if (my >= mz) L = fy < 0.f ? 3 : 2;
        else L = fz < 0.f ? 5 : 4;
    }
    nrm[3 * f] = fx; nrm[3 * f + 1] = fy; nrm[3 * f + 2] = fz;
    lab[f] = L;
    for (int k = 0; k < 3; ++k) {
        const int a = id[k], b = id[(k + 1) % 3];
        ekey[3 * f + k] = ok ? pair_key(min(a, b), max(a, b), Vn) : (uint64_t)Vn * (uint64_t)Vn;   // (Vn^2: joins nothing)
        eval[3 * f + k] = 3 * f + k;
    }
}

// b. a key held by exactly two face edges (of two different faces) joins them
__global__ void k_uva_adj(const uint64_t* __restrict__ key, const int* __restrict__ val, int n, uint64_t none, int* __restrict__ adj) {
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    const uint64_t k = key[p];
    if (k == none || (p > 0 && key[p - 1] == k)) return;
    if (p + 1 < n && key[p + 1] == k && (p + 2 >= n || key[p + 2] != k)) {
        const int e0 = val[p], e1 = val[p + 1];
        if (e0 / 3 != e1 / 3) { adj[e0] = e1 / 3; adj[e1] = e0 / 3; }
    }
}

// c. label smoothing (one Jacobi pass)
__global__ void k_uva_smooth(const int* __restrict__ adj, const float* __restrict__ nrm, const int* __restrict__ lin, int* __restrict__ lout, int F) {
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= F) return;
    const int l = lin[f];
    int out = l;
    if (l != DEGEN) {
        int nl[3];
        for (int k = 0; k < 3; ++k) {
            const int g = adj[3 * f + k];
            nl[k] = g >= 0 ? lin[g] : -1;
        }
        int c = -1;
        if (nl[0] >= 0 && nl[0] != DEGEN && (nl[0] == nl[1] || nl[0] == nl[2])) c = nl[0];
        else if (nl[1] >= 0 && nl[1] != DEGEN && nl[1] == nl[2]) c = nl[1];
        if (c >= 0 && c != l && axis_dot(c, nrm[3 * f], nrm[3 * f + 1], nrm[3 * f + 2]) >= COS70) out = c;
    }
    lout[f] = out;
}

// d. connected components of equal labels: the union-find of union_find.h over the faces.  Every union keeps par[f] <= f and ends each
// component with its smallest face index as the one root, whatever the threads' order, so chart[] is a function of adj and lab alone (any
// union-find with these two properties, however it hooks and halves, gives the same bytes).  A spent budget (the forest is not the descending one)
// leaves chart[f] = f, an index in range for every later kernel, and sets ERR_STATE, which the entry reads with the packing round's flags
__global__ void k_uva_cc_hook(const int* __restrict__ adj, const int* __restrict__ lab, int* par, int F, int* __restrict__ misc) {
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= F) return;
    const int l = lab[f];
    long long budget = 2ll * F + 64;
    for (int k = 0; k < 3; ++k) {
        const int g = adj[3 * f + k];
        if (g <= f || lab[g] != l) continue;
        if (unite(par, find_root(par, f, budget), find_root(par, g, budget), budget) < 0) atomicOr(&misc[M_FLAG], ERR_STATE);
    }
}
__global__ void k_uva_cc_flatten(const int* __restrict__ par, int* __restrict__ chart, int F, int* __restrict__ misc) {
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= F) return;
    int steps = F;
    int r = walk_root(par, f, steps);                            // = the smallest face index of the component
    if (r < 0) { atomicOr(&misc[M_FLAG], ERR_STATE); r = f; }
    chart[f] = r;
}

// e. small-chart merge
__global__ void k_uva_chart_stats(const int* __restrict__ chart, const int* __restrict__ lab, const float* __restrict__ nrm,
                                  int* __restrict__ csize, int* __restrict__ cmask, int F) {
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= F) return;
    const int r = chart[f];
    atomicAdd(&csize[r], 1);
    int m = 0;
    if (lab[f] != DEGEN)
        for (int L = 0; L < 6; ++L)
            if (axis_dot(L, nrm[3 * f], nrm[3 * f + 1], nrm[3 * f + 2]) >= COS70) m |= 1 << L;
    atomicAnd(&cmask[r], m);
}
// preferred target of a small chart: the largest acceptable adjacent chart, ties to the smaller id
__global__ void k_uva_merge_target(const int* __restrict__ adj, const int* __restrict__ chart, const int* __restrict__ lab,
                                   const int* __restrict__ csize, const int* __restrict__ cmask, unsigned long long* __restrict__ tgt, int F) {
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= F) return;
    const int S = chart[f];
    if (csize[S] >= MERGE_K || lab[f] == DEGEN) return;
    const int m = cmask[S];
    for (int k = 0; k < 3; ++k) {
        const int g = adj[3 * f + k];
        if (g < 0) continue;
        const int T = chart[g];
        const int lt = lab[T];
        if (T == S || lt == DEGEN || !((m >> lt) & 1)) continue;
        atomicMax(&tgt[S], ((unsigned long long)(unsigned)csize[T] << 32) | (unsigned long long)(~(unsigned)T));
    }
}
// a small chart moves into its target unless the target moves too and has the smaller id (no chains or cycles within a round)
__global__ void k_uva_merge_apply(const int* __restrict__ chart, const unsigned long long* __restrict__ tgt, const int* __restrict__ lin,
                                  int* __restrict__ lout, int F) {
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= F) return;
    const int S = chart[f];
    const unsigned long long key = tgt[S];
    int l = lin[f];
    if (key != 0ull) {
        const int T = (int)(~(unsigned)(key & 0xffffffffull));
        if (tgt[T] == 0ull || S < T) l = lin[T];
    }
    lout[f] = l;
}

// ---------------------------------------------------------------------------------------------------------------------------
// f / g. per-chart projected bounding boxes, packing, UVs
__global__ void k_uva_box_init(unsigned* __restrict__ box, int F) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < 4 * F) box[i] = (i & 2) ? 0u : 0xffffffffu;          // (min u, min v, max u, max v)
}
__global__ void k_uva_box(const float* __restrict__ V, const int* __restrict__ idx, const int* __restrict__ chart, const int* __restrict__ lab,
                          unsigned* __restrict__ box, int* __restrict__ csize, int F) {
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= F) return;
    const int r = chart[f], L = lab[f];
    atomicAdd(&csize[r], 1);
    if (L == DEGEN) return;
    float umin = 3.0e38f, vmin = 3.0e38f, umax = -3.0e38f, vmax = -3.0e38f;
    for (int k = 0; k < 3; ++k) {
        const int a = idx[3 * f + k];
        float u, v;
        axis_proj(L, V[3 * a], V[3 * a + 1], V[3 * a + 2], u, v);
        umin = fminf(umin, u); vmin = fminf(vmin, v); umax = fmaxf(umax, u); vmax = fmaxf(vmax, v);
    }
    atomicMin(&box[4 * r], f2ord(umin)); atomicMin(&box[4 * r + 1], f2ord(vmin));
    atomicMax(&box[4 * r + 2], f2ord(umax)); atomicMax(&box[4 * r + 3], f2ord(vmax));
}

__device__ __forceinline__ void chart_extent(const unsigned* box, int r, int L, float& W, float& H) {
    if (L == DEGEN) { W = 0.f; H = 0.f; return; }
    W = ord2f(box[4 * r + 2]) - ord2f(box[4 * r]);
    H = ord2f(box[4 * r + 3]) - ord2f(box[4 * r + 1]);
}

// packing order: taller first, then wider, then the smaller chart id (stable sort of ids in ascending order); non-roots last
__global__ void k_uva_pack_keys(const int* __restrict__ chart, const int* __restrict__ lab, const unsigned* __restrict__ box,
                                uint64_t* __restrict__ key, int* __restrict__ val, int* __restrict__ misc, int F) {
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= F) return;
    uint64_t k = ~0ull;
    if (chart[f] == f) {
        float W, H;
        chart_extent(box, f, lab[f], W, H);
        k = ((uint64_t)(~f2ord(H)) << 32) | (uint64_t)(~f2ord(W));
        atomicAdd(&misc[M_CHARTS], 1);
    }
    key[f] = k;
    val[f] = f;
}

__device__ __forceinline__ int rect_side(float s, float ext, int gutter) {
    return max(1, (int)ceilf(s * ext)) + 2 * gutter;
}

constexpr int PK_T = 256, PK_CH = 2048;
// One workgroup.  Pass 0: upper bound s_hi of the scale (every chart alone fits, total area fits); pass 1: 256 candidates
// s_hi * (k+1) / 256, one per thread, each shelf-packed; pass 2: 256 candidates between the best fitting one and the next;
// pass 3: thread 0 places the charts at the chosen scale.
__global__ __launch_bounds__(PK_T) void k_uva_pack(const int* __restrict__ order, const int* __restrict__ lab, const unsigned* __restrict__ box,
                                                   int R, int gutter, int* __restrict__ cpos, int* __restrict__ misc) {
    __shared__ float s_w[PK_CH], s_h[PK_CH];
    __shared__ double s_red[3][PK_T];
    __shared__ int s_best[PK_T];
    const int t = threadIdx.x;
    const int C = misc[M_CHARTS];
    double mw = 0.0, mh = 0.0, area = 0.0;
    for (int c = t; c < C; c += PK_T) {
        float W, H;
        const int r = order[c];
        chart_extent(box, r, lab[r], W, H);
        mw = fmax(mw, (double)W); mh = fmax(mh, (double)H); area += (double)W * (double)H;
    }
    s_red[0][t] = mw; s_red[1][t] = mh; s_red[2][t] = area;
    __syncthreads();
    for (int off = PK_T / 2; off > 0; off >>= 1) {
        if (t < off) {
            s_red[0][t] = fmax(s_red[0][t], s_red[0][t + off]);
            s_red[1][t] = fmax(s_red[1][t], s_red[1][t + off]);
            s_red[2][t] = s_red[2][t] + s_red[2][t + off];
        }
        __syncthreads();
    }
    const double room = (double)(R - 2 * gutter - 1);
    double shi = 1.0e30;
    if (s_red[0][0] > 0.0) shi = fmin(shi, room / s_red[0][0]);
    if (s_red[1][0] > 0.0) shi = fmin(shi, room / s_red[1][0]);
    if (s_red[2][0] > 0.0) shi = fmin(shi, (double)R / sqrt(s_red[2][0]));
    if (shi > 1.0e29) shi = 1.0;
    __syncthreads();

    // shelf-pack all charts at scale s; place = write the positions (thread 0 only)
    auto pack = [&](float s, bool place) -> bool {
        int x = 0, y = 0, sh = 0;
        bool ok = true;
        for (int c0 = 0; c0 < C; c0 += PK_CH) {
            const int n = min(PK_CH, C - c0);
            __syncthreads();
            for (int c = t; c < n; c += PK_T) {
                const int r = order[c0 + c];
                chart_extent(box, r, lab[r], s_w[c], s_h[c]);
            }
            __syncthreads();
            for (int c = 0; c < n && ok; ++c) {
                const float fw = s * s_w[c], fh = s * s_h[c];
                if (!(fw <= (float)R) || !(fh <= (float)R)) { ok = false; break; }
                const int w = rect_side(s, s_w[c], gutter), h = rect_side(s, s_h[c], gutter);
                if (w > R || h > R) { ok = false; break; }
                if (x + w > R) { y += sh; x = 0; sh = 0; }
                if (place) { const int r = order[c0 + c]; cpos[2 * r] = x; cpos[2 * r + 1] = y; }
                x += w;
                sh = max(sh, h);
                if (y + sh > R) ok = false;
            }
        }
        return ok && y + sh <= R;
    };

    const float s1 = (float)(shi * (double)(t + 1) / PK_T);
    s_best[t] = pack(s1, false) ? t : -1;
    __syncthreads();
    for (int off = PK_T / 2; off > 0; off >>= 1) {
        if (t < off) s_best[t] = max(s_best[t], s_best[t + off]);
        __syncthreads();
    }
    const int k1 = s_best[0];
    __syncthreads();
    float s = 0.f;
    if (k1 >= 0) {
        const double lo = shi * (double)(k1 + 1) / PK_T, hi = fmin(shi, shi * (double)(k1 + 2) / PK_T);
        const float s2 = (float)(lo + (hi - lo) * (double)(t + 1) / PK_T);
        const bool ok2 = hi > lo && pack(s2, false);
        s_best[t] = ok2 ? t : -1;
        __syncthreads();
        for (int off = PK_T / 2; off > 0; off >>= 1) {
            if (t < off) s_best[t] = max(s_best[t], s_best[t + off]);
            __syncthreads();
        }
        const int k2 = s_best[0];
        s = k2 >= 0 ? (float)(lo + (hi - lo) * (double)(k2 + 1) / PK_T) : (float)lo;
        __syncthreads();
    }
    if (k1 < 0 || C == 0) {
        if (t == 0) { atomicOr(&misc[M_FLAG], ERR_PACK); misc[M_SCALE] = 0; }
        return;
    }
    if (t == 0) misc[M_SCALE] = __float_as_int(s);
    // placement: every thread takes part in the chunk loads (one call site: the barriers inside must not diverge), thread 0 writes
    pack(s, t == 0);
}

// UV of vertex `a` in chart r (label L): one affine map per chart, u = (px + g + s (P(a).u - min u)) / R
__device__ __forceinline__ void chart_uv(const float* V, int a, int r, int L, const unsigned* box, const int* cpos, float s, int gutter,
                                         int R, float& u, float& v) {
    float tu = (float)(cpos[2 * r] + gutter), tv = (float)(cpos[2 * r + 1] + gutter);
    if (L != DEGEN) {
        float pu, pv;
        axis_proj(L, V[3 * a], V[3 * a + 1], V[3 * a + 2], pu, pv);
        tu = tu + s * (pu - ord2f(box[4 * r]));
        tv = tv + s * (pv - ord2f(box[4 * r + 1]));
    }
    u = fminf(fmaxf(tu / (float)R, 0.f), 1.f);
    v = fminf(fmaxf(tv / (float)R, 0.f), 1.f);
}

// the texel rectangle each face can cover, from the rasteriser's snapped triangle of its UVs (uv_clip = uv * 2 - 1)
__global__ void k_uva_tri_box(const float* __restrict__ V, const int* __restrict__ idx, const int* __restrict__ chart, const int* __restrict__ lab,
                              const unsigned* __restrict__ box, const int* __restrict__ cpos, const int* __restrict__ misc, int gutter, int R,
                              float* __restrict__ fuv, short4* __restrict__ tbox, int F) {
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= F) return;
    const float s = __int_as_float(misc[M_SCALE]);
    const int r = chart[f], L = lab[f];
    float c[6];
    for (int k = 0; k < 3; ++k) {
        float u, v;
        chart_uv(V, idx[3 * f + k], r, L, box, cpos, s, gutter, R, u, v);
        c[2 * k] = u; c[2 * k + 1] = v;
        fuv[6 * f + 2 * k] = u; fuv[6 * f + 2 * k + 1] = v;
    }
    int jmin = 1, jmax = 0, imin = 1, imax = 0;
    const SnapTri st = snap_tri(c[0] * 2.0f - 1.0f, c[1] * 2.0f - 1.0f, c[2] * 2.0f - 1.0f, c[3] * 2.0f - 1.0f, c[4] * 2.0f - 1.0f,
                                c[5] * 2.0f - 1.0f, R);
    if (st.area != 0) snap_tri_box(st, R, jmin, jmax, imin, imax);
    if (jmin > jmax || imin > imax) { jmin = 1; jmax = 0; imin = 1; imax = 0; }
    tbox[f] = make_short4((short)jmin, (short)jmax, (short)imin, (short)imax);
}

// coverage count per texel of a 64 x 64 tile in LDS; a texel covered twice flags the chart that owns it
constexpr int CV_TILE = 64, CV_T = 256;
__global__ __launch_bounds__(CV_T) void k_uva_cover(const float* __restrict__ fuv, const short4* __restrict__ tbox, const int* __restrict__ chart,
                                                    int F, int R, int* __restrict__ cflag, int* __restrict__ misc) {
    __shared__ int s_cnt[CV_TILE * CV_TILE];
    __shared__ int s_own[CV_TILE * CV_TILE];
    const int tiles_x = (R + CV_TILE - 1) / CV_TILE;
    const int tx0 = (blockIdx.x % tiles_x) * CV_TILE, ty0 = (blockIdx.x / tiles_x) * CV_TILE;
    const int t = threadIdx.x;
    for (int k = t; k < CV_TILE * CV_TILE; k += CV_T) { s_cnt[k] = 0; s_own[k] = -1; }
    __syncthreads();
    for (int f = t; f < F; f += CV_T) {
        const short4 b = tbox[f];
        const int j0 = max((int)b.x, tx0), j1 = min((int)b.y, tx0 + CV_TILE - 1);
        const int i0 = max((int)b.z, ty0), i1 = min((int)b.w, ty0 + CV_TILE - 1);
        if (j0 > j1 || i0 > i1) continue;
        const float* c = fuv + 6 * (size_t)f;
        const SnapTri st = snap_tri(c[0] * 2.0f - 1.0f, c[1] * 2.0f - 1.0f, c[2] * 2.0f - 1.0f, c[3] * 2.0f - 1.0f, c[4] * 2.0f - 1.0f,
                                    c[5] * 2.0f - 1.0f, R);
        const int r = chart[f];
        for (int i = i0; i <= i1; ++i)
            for (int j = j0; j <= j1; ++j) {
                long long E0, E1, E2;
                if (!snap_tri_covers(st, j, i, E0, E1, E2)) continue;
                const int o = (i - ty0) * CV_TILE + (j - tx0);
                atomicAdd(&s_cnt[o], 1);
                s_own[o] = r;                                       // (chart rectangles are disjoint: one chart per texel)
            }
    }
    __syncthreads();
    bool any = false;
    for (int k = t; k < CV_TILE * CV_TILE; k += CV_T)
        if (s_cnt[k] > 1) { cflag[s_own[k]] = 1; any = true; }
    if (__ballot(any) != 0ull && (t & 63) == 0) atomicOr(&misc[M_FLAG], FLAG_OVERLAP);
}

// split of an overlapping chart at the median of its face centroids along its longer projected axis
__global__ void k_uva_split_keys(const float* __restrict__ fuv, const int* __restrict__ chart, const unsigned* __restrict__ box,
                                 const int* __restrict__ cflag, uint64_t* __restrict__ key, int* __restrict__ val, int F) {
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= F) return;
    const int r = chart[f];
    unsigned c = 0u;
    if (cflag[r]) {
        const float W = ord2f(box[4 * r + 2]) - ord2f(box[4 * r]), H = ord2f(box[4 * r + 3]) - ord2f(box[4 * r + 1]);
        const int o = W >= H ? 0 : 1;
        c = f2ord((fuv[6 * f + o] + fuv[6 * f + 2 + o]) + fuv[6 * f + 4 + o]);
    }
    key[f] = ((uint64_t)(unsigned)r << 32) | c;
    val[f] = f;
}
__global__ void k_uva_split_start(const uint64_t* __restrict__ key, int* __restrict__ cstart, int F) {
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= F) return;
    if (p == 0 || (key[p] >> 32) != (key[p - 1] >> 32)) cstart[(int)(key[p] >> 32)] = p;
}
__global__ void k_uva_split_mark(const uint64_t* __restrict__ key, const int* __restrict__ val, const int* __restrict__ cstart,
                                 const int* __restrict__ csize, const int* __restrict__ cflag, int* __restrict__ upper, int* __restrict__ hmin, int F) {
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= F) return;
    const int r = (int)(key[p] >> 32), f = val[p];
    if (!cflag[r]) return;
    const int up = (p - cstart[r]) >= csize[r] / 2 ? 1 : 0;
    upper[f] = up;
    atomicMin(&hmin[2 * r + up], f);
}
__global__ void k_uva_split_apply(int* __restrict__ chart, const int* __restrict__ cflag, const int* __restrict__ upper, const int* __restrict__ hmin,
                                  int singleton, int F) {
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= F) return;
    const int r = chart[f];
    if (!cflag[r]) return;
    chart[f] = singleton ? f : hmin[2 * r + upper[f]];
}

// final UV entries: one per (chart, vertex) pair, in (chart, vertex) order
__global__ void k_uva_entry_keys(const int* __restrict__ chart, const int* __restrict__ idx, int Vn, uint64_t* __restrict__ key,
                                 int* __restrict__ val, int n) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= n) return;
    key[c] = pair_key((unsigned)chart[c / 3], (unsigned)idx[c], Vn);
    val[c] = c;
}
__global__ void k_uva_entry_write(const float* __restrict__ V, const int* __restrict__ idx, const int* __restrict__ chart, const int* __restrict__ lab,
                                  const unsigned* __restrict__ box, const int* __restrict__ cpos, const int* __restrict__ misc, int gutter, int R,
                                  const int* __restrict__ val, const int* __restrict__ flag, const int* __restrict__ incl,
                                  float* __restrict__ uvs, int64_t* __restrict__ tex_idx, int n) {
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    const int c = val[p], e = incl[p] - 1;
    tex_idx[c] = e;
    if (flag[p]) {
        const int f = c / 3, r = chart[f];
        float u, v;
        chart_uv(V, idx[c], r, lab[f], box, cpos, __int_as_float(misc[M_SCALE]), gutter, R, u, v);
        uvs[2 * e] = u;
        uvs[2 * e + 1] = v;
    }
}
__global__ void k_uva_finish(const int* __restrict__ chart, int32_t* __restrict__ face_chart, const int* __restrict__ incl, int n,
                             const int* __restrict__ misc, int rounds, int32_t* __restrict__ counts, int F) {
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f < F) face_chart[f] = chart[f];
    if (f == 0) {
        counts[0] = incl[n - 1];
        counts[1] = misc[M_CHARTS];
        counts[2] = rounds;
        counts[3] = misc[M_FLAG] & ~FLAG_OVERLAP;
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
struct Ws {
    int *idx, *lab[2], *adj, *par, *chart, *csize, *cmask, *cflag, *cpos, *hmin, *upper, *cstart, *flag, *incl, *misc;
    float *nrm, *fuv;
    unsigned* box;
    unsigned long long* tgt;
    short4* tbox;
    SortBufs sb;
};

static size_t carve(Ws& w, void* base, int F) {
    const size_t N = 3 * (size_t)F;
    Carve c{static_cast<char*>(base), 0};
    w.idx = c.take<int>(N); w.nrm = c.take<float>(N); w.lab[0] = c.take<int>(F); w.lab[1] = c.take<int>(F);
    w.adj = c.take<int>(N); w.par = c.take<int>(F); w.chart = c.take<int>(F);
    w.csize = c.take<int>(F); w.cmask = c.take<int>(F); w.cflag = c.take<int>(F); w.cpos = c.take<int>(2 * (size_t)F);
    w.hmin = c.take<int>(2 * (size_t)F); w.upper = c.take<int>(F); w.cstart = c.take<int>(F);
    w.flag = c.take<int>(N); w.incl = c.take<int>(N); w.misc = c.take<int>(M_WORDS);
    w.fuv = c.take<float>(6 * (size_t)F); w.box = c.take<unsigned>(4 * (size_t)F); w.tgt = c.take<unsigned long long>(F);
    w.tbox = c.take<short4>(F);
    carve_sort(c, w.sb, N);
    return c.off + 256;
}

}  // namespace

extern "C" size_t pdhip_uv_atlas_ws_bytes(int Vn, int F) {
    if (Vn <= 0 || F <= 0) return 0;
    Ws w;
    return carve(w, nullptr, F);
}

extern "C" int pdhip_uv_atlas(const float* vertices, int Vn, const int64_t* faces, int F, int resolution, int gutter, float* uvs,
                              int64_t* tex_idx, int32_t* face_chart, int32_t* counts, void* ws, void* stream) {
    PD_REQUIRE(vertices && faces && uvs && tex_idx && face_chart && counts && ws, "pdhip_uv_atlas: null pointer");
    PD_REQUIRE(Vn > 0 && F > 0, "pdhip_uv_atlas: empty mesh (Vn=%d F=%d)", Vn, F);
    PD_REQUIRE(F <= (1 << 28), "pdhip_uv_atlas: F=%d faces exceeds 2^28", F);
    PD_REQUIRE(gutter >= 0 && resolution >= 2 * gutter + 1 && resolution <= 16384,
               "pdhip_uv_atlas: resolution %d must be in [2 * gutter + 1, 16384] (gutter %d)", resolution, gutter);
    hipStream_t s = as_stream(stream);
    Ws w;
    carve(w, ws, F);
    const int N = 3 * F, R = resolution, TB = 256;
    const int gF = cdiv(F, TB), gN = cdiv(N, TB);
    PD_HIP(hipMemsetAsync(w.misc, 0, M_WORDS * sizeof(int), s));
    PD_HIP(hipMemsetAsync(w.adj, 0xff, (size_t)N * sizeof(int), s));

    // a, b
    k_uva_faces<<<gF, TB, 0, s>>>(vertices, Vn, faces, F, w.idx, w.nrm, w.lab[0], w.sb.k[0], w.sb.v[0], w.misc);
    const uint64_t none = (uint64_t)Vn * (uint64_t)Vn;
    int cur = radix_sort(w.sb, N, bits_for(none), s);
    k_uva_adj<<<gN, TB, 0, s>>>(w.sb.k[cur], w.sb.v[cur], N, none, w.adj);
    // c
    int L = 0;
    for (int it = 0; it < SMOOTH_PASSES; ++it, L ^= 1) k_uva_smooth<<<gF, TB, 0, s>>>(w.adj, w.nrm, w.lab[L], w.lab[L ^ 1], F);
    // d, e
    auto components = [&]() {
        k_uf_identity<<<gF, TB, 0, s>>>(w.par, F);
        k_uva_cc_hook<<<gF, TB, 0, s>>>(w.adj, w.lab[L], w.par, F, w.misc);
        k_uva_cc_flatten<<<gF, TB, 0, s>>>(w.par, w.chart, F, w.misc);
    };
    components();
    for (int m = 0; m < MERGE_ROUNDS; ++m) {
        PD_HIP(hipMemsetAsync(w.csize, 0, (size_t)F * sizeof(int), s));
        PD_HIP(hipMemsetAsync(w.cmask, 0xff, (size_t)F * sizeof(int), s));
        PD_HIP(hipMemsetAsync(w.tgt, 0, (size_t)F * sizeof(unsigned long long), s));
        k_uva_chart_stats<<<gF, TB, 0, s>>>(w.chart, w.lab[L], w.nrm, w.csize, w.cmask, F);
        k_uva_merge_target<<<gF, TB, 0, s>>>(w.adj, w.chart, w.lab[L], w.csize, w.cmask, w.tgt, F);
        k_uva_merge_apply<<<gF, TB, 0, s>>>(w.chart, w.tgt, w.lab[L], w.lab[L ^ 1], F);
        L ^= 1;
        components();
    }
    const int* lab = w.lab[L];

    // f, g: pack, check, split; the host reads the flag word once per round
    int rounds = 0;
    for (int round = 0;; ++round) {
        PD_HIP(hipMemsetAsync(w.csize, 0, (size_t)F * sizeof(int), s));
        PD_HIP(hipMemsetAsync(w.misc + M_CHARTS, 0, sizeof(int), s));
        k_uva_box_init<<<cdiv(4ll * F, TB), TB, 0, s>>>(w.box, F);
        k_uva_box<<<gF, TB, 0, s>>>(vertices, w.idx, w.chart, lab, w.box, w.csize, F);
        k_uva_pack_keys<<<gF, TB, 0, s>>>(w.chart, lab, w.box, w.sb.k[0], w.sb.v[0], w.misc, F);
        cur = radix_sort(w.sb, F, 64, s);
        k_uva_pack<<<1, PK_T, 0, s>>>(w.sb.v[cur], lab, w.box, R, gutter, w.cpos, w.misc);
        k_uva_tri_box<<<gF, TB, 0, s>>>(vertices, w.idx, w.chart, lab, w.box, w.cpos, w.misc, gutter, R, w.fuv, w.tbox, F);
        const bool check = round < SPLIT_ROUNDS + SINGLE_ROUNDS;
        if (check) {
            PD_HIP(hipMemsetAsync(w.cflag, 0, (size_t)F * sizeof(int), s));
            k_uva_cover<<<cdiv(R, CV_TILE) * cdiv(R, CV_TILE), CV_T, 0, s>>>(w.fuv, w.tbox, w.chart, F, R, w.cflag, w.misc);
        }
        PD_LAUNCH_CHECK();
        int word = 0;
        const int rc = read_words(w.misc + M_FLAG, &word, 1, s);
        if (rc != PDHIP_OK) return rc;
        if (word & ERR_STATE) {
            set_error("pdhip_uv_atlas: a union-find walk used up its budget of steps: the forest is not the descending one the kernels keep; "
                      "nothing was written");
            return PDHIP_E_STATE;
        }
        PD_REQUIRE(!(word & ERR_INDEX), "pdhip_uv_atlas: a face index lies outside [0, Vn=%d)", Vn);
        PD_REQUIRE(!(word & ERR_PACK), "pdhip_uv_atlas: the charts do not fit a %d x %d atlas with gutter %d", R, R, gutter);
        if (!check || !(word & FLAG_OVERLAP)) break;
        PD_HIP(hipMemsetAsync(w.misc + M_FLAG, 0, sizeof(int), s));
        ++rounds;
        const bool singleton = round >= SPLIT_ROUNDS;
        if (!singleton) {
            PD_HIP(hipMemsetAsync(w.hmin, 0x7f, 2 * (size_t)F * sizeof(int), s));
            k_uva_split_keys<<<gF, TB, 0, s>>>(w.fuv, w.chart, w.box, w.cflag, w.sb.k[0], w.sb.v[0], F);
            cur = radix_sort(w.sb, F, 32 + bits_for((unsigned long long)F), s);
            k_uva_split_start<<<gF, TB, 0, s>>>(w.sb.k[cur], w.cstart, F);
            k_uva_split_mark<<<gF, TB, 0, s>>>(w.sb.k[cur], w.sb.v[cur], w.cstart, w.csize, w.cflag, w.upper, w.hmin, F);
        }
        k_uva_split_apply<<<gF, TB, 0, s>>>(w.chart, w.cflag, w.upper, w.hmin, singleton ? 1 : 0, F);
    }

    // f: UV entries
    k_uva_entry_keys<<<gN, TB, 0, s>>>(w.chart, w.idx, Vn, w.sb.k[0], w.sb.v[0], N);
    cur = radix_sort(w.sb, N, bits_for((unsigned long long)F * (unsigned long long)Vn), s);
    k_run_heads<uint64_t><<<gN, TB, 0, s>>>(w.sb.k[cur], N, nullptr, ~0ull, w.flag);
    k_scan<<<1, SC_T, 0, s>>>(w.flag, w.incl, N, 0);
    k_uva_entry_write<<<gN, TB, 0, s>>>(vertices, w.idx, w.chart, lab, w.box, w.cpos, w.misc, gutter, R, w.sb.v[cur], w.flag, w.incl, uvs,
                                        tex_idx, N);
    k_uva_finish<<<gF, TB, 0, s>>>(w.chart, face_chart, w.incl, N, w.misc, rounds, counts, F);
    PD_LAUNCH_CHECK();
    return PDHIP_OK;
}
