// Surface reconstruction from an oriented point cloud on the device (what baselines/spr.py:recon_one_shape_SPR asks pymeshlab for:
// normals for a point set + screened Poisson reconstruction), on a dense grid.
//
//   pdhip_estimate_normals
//     a. uniform cell grid over the cloud (cell_list.h: cell keys, radix sort, cell starts), k nearest neighbours by scanning the ring of
//        cells round each point, the ring growing until the k-th distance is certified by the scanned cube;
//     b. normal = eigenvector of the smallest eigenvalue of the neighbourhood covariance (f64 about the neighbourhood mean,
//        closed-form 3 x 3 symmetric solve in registers);
//     c. sign: n_eyes Fibonacci eyes on a sphere round the cloud, pdhip_hidden_point_removal for all of them, per point the sum of
//        sign(n . (eye - p)) over the eyes that see it; then Jacobi rounds of the majority sign of the oriented k neighbours; then
//        the sign of the nearest oriented neighbour.  counts = points oriented by rule 1 / 2 / 3 / left as they were.
//   pdhip_surface_recon
//     d. Poisson: V = -sum_p a_p w(|x - p|) n_p (w = (1 - r^2 / R^2)^3, a_p = 1 / local sample density), the right-hand side
//        div V GATHERED per grid node from the sorted cell list (analytic gradient of w, fixed order), 7-point Laplacian with zero
//        boundary values, conjugate gradients with fixed-tree f64 reductions: TWO launches per iteration;
//     e. iso value = mean of chi interpolated trilinearly at the points; chi is HIGHER INSIDE the solid;
//     f. marching cubes with welded vertices (a vertex per crossing grid edge, ids by exclusive scan; csrc/mc_tables.h), triangles
//        wound counter-clockwise seen from outside; vertex colours = colour of the nearest cloud point.
// No float atomics: every sum has a fixed order, two calls give identical bytes.  Compiled with -ffp-contract=off.
#include "common.h"
#include "cell_list.h"
#include "mc_tables.h"
#include <math.h>
#include <string.h>
#include <algorithm>
using namespace pdhip;

namespace {

constexpr int KMAX = 32, KNN_T = 64;
constexpr int CG_NB = 512, CG_T = 256, CG_CHUNK = 32;
constexpr int ORIENT_ROUNDS = 32;
constexpr double HPR_RADIUS = 100.0;                 // the pipeline's hidden_point_removal_radius default
constexpr float CG_TOL = 1.0e-4f;                    // |r| <= CG_TOL |f|
constexpr int TB = 256;
// M_DONE is written by k_sr_cg_pq and read by k_sr_cg_xr, M_SEEN is written by k_sr_cg_xr and read by k_sr_cg_pq: a launch never reads a
// flag that the same launch writes
enum { M_NV = 0, M_NF = 1, M_ITERS = 2, M_DONE = 3, M_SEEN = 4, M_ISO = 5, M_RES = 6, M_WORDS = 64 };
enum { MOM_MIN = 0, MOM_MAX = 3, MOM_SUM = 6, MOM_PROD = 9, MOM_BAD = 15, MOM_WORDS = 16 };

struct CellGrid {
    float ox, oy, oz, cs;
    int C;
};

__device__ __forceinline__ int cell_of(float x, float o, float cs, int C) {
    const int c = (int)floorf((x - o) / cs);
    return min(max(c, 0), C - 1);
}

// ---------------------------------------------------------------------------------------------------------------------------
// bounding box + first and second moments of the cloud (one workgroup, fixed order)
__global__ __launch_bounds__(TB) void k_sr_moments(const float* __restrict__ P, int N, double* __restrict__ out) {
    __shared__ double sh[MOM_WORDS][TB];
    const int t = threadIdx.x;
    double mn0 = 1e300, mn1 = 1e300, mn2 = 1e300, mx0 = -1e300, mx1 = -1e300, mx2 = -1e300;
    double s0 = 0, s1 = 0, s2 = 0, p00 = 0, p01 = 0, p02 = 0, p11 = 0, p12 = 0, p22 = 0, bad = 0;
    const double x0 = P[0], y0 = P[1], z0 = P[2];           // moments about the first point
    for (int i = t; i < N; i += TB) {
        const float fx = P[3 * i], fy = P[3 * i + 1], fz = P[3 * i + 2];
        if (!(fabsf(fx) <= 1.0e18f) || !(fabsf(fy) <= 1.0e18f) || !(fabsf(fz) <= 1.0e18f)) { bad += 1.0; continue; }
        const double x = fx, y = fy, z = fz;
        mn0 = fmin(mn0, x); mn1 = fmin(mn1, y); mn2 = fmin(mn2, z);
        mx0 = fmax(mx0, x); mx1 = fmax(mx1, y); mx2 = fmax(mx2, z);
        const double dx = x - x0, dy = y - y0, dz = z - z0;
        s0 += dx; s1 += dy; s2 += dz;
        p00 += dx * dx; p01 += dx * dy; p02 += dx * dz; p11 += dy * dy; p12 += dy * dz; p22 += dz * dz;
    }
    sh[0][t] = mn0; sh[1][t] = mn1; sh[2][t] = mn2; sh[3][t] = mx0; sh[4][t] = mx1; sh[5][t] = mx2;
    sh[6][t] = s0; sh[7][t] = s1; sh[8][t] = s2;
    sh[9][t] = p00; sh[10][t] = p01; sh[11][t] = p02; sh[12][t] = p11; sh[13][t] = p12; sh[14][t] = p22; sh[15][t] = bad;
    __syncthreads();
    for (int off = TB / 2; off > 0; off >>= 1) {
        if (t < off) {
#pragma unroll
            for (int w = 0; w < 3; ++w) sh[w][t] = fmin(sh[w][t], sh[w][t + off]);
#pragma unroll
            for (int w = 3; w < 6; ++w) sh[w][t] = fmax(sh[w][t], sh[w][t + off]);
#pragma unroll
            for (int w = 6; w < MOM_WORDS; ++w) sh[w][t] = sh[w][t] + sh[w][t + off];
        }
        __syncthreads();
    }
    if (t < MOM_WORDS) out[t] = sh[t][0];
}

// ---------------------------------------------------------------------------------------------------------------------------
// cell list (cell_list.h): the key of the cell of point i of P.  The scans below visit the cells of a cube in the order z, y, x ascending and a
// cell's points cstart[c] .. cstart[c + 1] ascending: the f32 sums of k_sr_sample_weights and k_sr_rhs and the ties of k_sr_nearest_color
// rest on that order
struct SrKey {
    const float* P;
    CellGrid g;
    __device__ uint64_t operator()(int i) const {
        const int cx = cell_of(P[3 * i], g.ox, g.cs, g.C), cy = cell_of(P[3 * i + 1], g.oy, g.cs, g.C), cz = cell_of(P[3 * i + 2], g.oz, g.cs, g.C);
        return (uint64_t)((cz * g.C + cy) * g.C + cx);
    }
};

// distance^2 from q to the nearest face of the scanned cube of cells [c - r, c + r] that is not a face of the whole grid
__device__ __forceinline__ float ring_bound(float q, float o, float cs, int C, int c, int r) {
    float b = 3.0e38f;
    if (c - r > 0) b = fminf(b, q - (o + (float)(c - r) * cs));
    if (c + r < C - 1) b = fminf(b, (o + (float)(c + r + 1) * cs) - q);
    return b;
}

// ---------------------------------------------------------------------------------------------------------------------------
// a, b. k nearest neighbours (the point itself included) and the unoriented normal
// unit eigenvector of A for its eigenvalue lam: orthogonal to the three rows of A - lam I, the largest of their three cross products.
// false: all three vanish
__device__ __forceinline__ bool null_direction(double a00, double a01, double a02, double a11, double a12, double a22, double lam, double& nx,
                                               double& ny, double& nz) {
    const double r0x = a00 - lam, r0y = a01, r0z = a02, r1x = a01, r1y = a11 - lam, r1z = a12, r2x = a02, r2y = a12, r2z = a22 - lam;
    const double ax = r0y * r1z - r0z * r1y, ay = r0z * r1x - r0x * r1z, az = r0x * r1y - r0y * r1x;
    const double bx = r0y * r2z - r0z * r2y, by = r0z * r2x - r0x * r2z, bz = r0x * r2y - r0y * r2x;
    const double cx = r1y * r2z - r1z * r2y, cy = r1z * r2x - r1x * r2z, cz = r1x * r2y - r1y * r2x;
    const double la = ax * ax + ay * ay + az * az, lb = bx * bx + by * by + bz * bz, lc = cx * cx + cy * cy + cz * cz;
    double vx = ax, vy = ay, vz = az, l = la;
    if (lb > l) { vx = bx; vy = by; vz = bz; l = lb; }
    if (lc > l) { vx = cx; vy = cy; vz = cz; l = lc; }
    if (!(l > 0.0)) return false;
    const double s = 1.0 / sqrt(l);
    nx = vx * s; ny = vy * s; nz = vz * s;
    return true;
}

// Eigenvalues of A in closed form: q + 2 p cos(phi + 2 pi k / 3), phi = acos(r) / 3, r = half the determinant of (A - q I) / p.  The eigenvalue
// asked for directly is good to a few ulp of p while it is the isolated one (r <= 0: the two LARGEST are the close pair, a surface patch).  For
// r > 0 the two SMALLEST are the close pair (a neighbourhood stretched along a line) and acos is ill-conditioned towards 1: the error of the direct
// form grows with (lambda_2 / (lambda_1 - lambda_0))^2.  There the isolated, largest eigenvalue gives its eigenvector first, and the smallest one
// comes from the symmetric 2 x 2 problem in the plane orthogonal to it, whose error grows with lambda_2 / (lambda_1 - lambda_0) only.
__device__ __forceinline__ void smallest_eigvec(double a00, double a01, double a02, double a11, double a12, double a22, double& nx, double& ny,
                                                double& nz) {
    const double p1 = a01 * a01 + a02 * a02 + a12 * a12;
    const double q = (a00 + a11 + a22) / 3.0;
    const double b00 = a00 - q, b11 = a11 - q, b22 = a22 - q;
    const double p2 = b00 * b00 + b11 * b11 + b22 * b22 + 2.0 * p1;
    double lam = q;
    if (p2 > 0.0) {
        const double p = sqrt(p2 / 6.0);
        const double c00 = b00 / p, c11 = b11 / p, c22 = b22 / p, c01 = a01 / p, c02 = a02 / p, c12 = a12 / p;
        double r = 0.5 * (c00 * (c11 * c22 - c12 * c12) - c01 * (c01 * c22 - c12 * c02) + c02 * (c01 * c12 - c11 * c02));
        r = fmin(1.0, fmax(-1.0, r));
        const double phi = acos(r) / 3.0;
        double ex, ey, ez;
        if (r > 0.0 && null_direction(a00, a01, a02, a11, a12, a22, q + 2.0 * p * cos(phi), ex, ey, ez)) {
            // u, w: an orthonormal basis of the plane orthogonal to e
            double ux, uy, uz;
            if (fabs(ex) > fabs(ey)) {
                const double s = 1.0 / sqrt(ex * ex + ez * ez);
                ux = -ez * s; uy = 0.0; uz = ex * s;
            } else {
                const double s = 1.0 / sqrt(ey * ey + ez * ez);
                ux = 0.0; uy = ez * s; uz = -ey * s;
            }
            const double wx = ey * uz - ez * uy, wy = ez * ux - ex * uz, wz = ex * uy - ey * ux;
            const double aux = a00 * ux + a01 * uy + a02 * uz, auy = a01 * ux + a11 * uy + a12 * uz, auz = a02 * ux + a12 * uy + a22 * uz;
            const double awx = a00 * wx + a01 * wy + a02 * wz, awy = a01 * wx + a11 * wy + a12 * wz, awz = a02 * wx + a12 * wy + a22 * wz;
            const double m00 = ux * aux + uy * auy + uz * auz, m01 = wx * aux + wy * auy + wz * auz, m11 = wx * awx + wy * awy + wz * awz;
            // the smaller eigenvalue of (m00 m01; m01 m11) is (m00 + m11) / 2 - h; its eigenvector is orthogonal to the row of M - lambda I whose
            // diagonal entry, hd + h or h - hd, is a sum of two non-negative numbers
            const double hd = 0.5 * (m00 - m11), h = sqrt(hd * hd + m01 * m01);
            double c = 1.0, s = 0.0;
            if (h > 0.0) {
                if (hd >= 0.0) { c = -m01; s = hd + h; }
                else { c = h - hd; s = -m01; }
            }
            const double tx = c * ux + s * wx, ty = c * uy + s * wy, tz = c * uz + s * wz;
            const double t = 1.0 / sqrt(tx * tx + ty * ty + tz * tz);
            nx = tx * t; ny = ty * t; nz = tz * t;
            return;
        }
        lam = q + 2.0 * p * cos(phi + 2.0943951023931954923);      // the smallest eigenvalue
    }
    if (!null_direction(a00, a01, a02, a11, a12, a22, lam, nx, ny, nz)) {      // isotropic neighbourhood: no direction is preferred
        nx = 0.0; ny = 0.0; nz = 1.0;
    }
}

__global__ __launch_bounds__(KNN_T) void k_sr_knn_normals(const float4* __restrict__ spos, const int* __restrict__ cstart, CellGrid g, int N,
                                                          int k, int* __restrict__ knn, float* __restrict__ nrm) {
    __shared__ float s_d[KMAX][KNN_T];
    __shared__ int s_p[KMAX][KNN_T];
    const int t = threadIdx.x;
    const int sp = blockIdx.x * KNN_T + t;                        // queries in sorted order: neighbouring threads scan the same cells
    if (sp >= N) return;
    const float4 me = spos[sp];
    const int i = __float_as_int(me.w);
    const int C = g.C;
    const int cx = cell_of(me.x, g.ox, g.cs, C), cy = cell_of(me.y, g.oy, g.cs, C), cz = cell_of(me.z, g.oz, g.cs, C);
    for (int r = 1;; ++r) {
        int cnt = 0, maxs = 0;
        float maxd = -1.0f;
        const CellCube q = cube_around(cx, cy, cz, r, C);
        for (int z = q.z0; z <= q.z1; ++z)
            for (int y = q.y0; y <= q.y1; ++y)
                for (int x = q.x0; x <= q.x1; ++x) {
                    const int c = (z * C + y) * C + x;
                    const int e = cstart[c + 1];
                    for (int p = cstart[c]; p < e; ++p) {
                        const float4 s = spos[p];
                        const float dx = s.x - me.x, dy = s.y - me.y, dz = s.z - me.z;
                        const float d = (dx * dx + dy * dy) + dz * dz;
                        if (cnt < k) {
                            s_d[cnt][t] = d; s_p[cnt][t] = p;
                            if (d > maxd) { maxd = d; maxs = cnt; }
                            ++cnt;
                        } else if (d < maxd) {
                            s_d[maxs][t] = d; s_p[maxs][t] = p;
                            maxd = -1.0f;
                            for (int j = 0; j < k; ++j) {
                                const float dj = s_d[j][t];
                                if (dj > maxd) { maxd = dj; maxs = j; }
                            }
                        }
                    }
                }
        const float b = fminf(fminf(ring_bound(me.x, g.ox, g.cs, C, cx, r), ring_bound(me.y, g.oy, g.cs, C, cy, r)),
                              ring_bound(me.z, g.oz, g.cs, C, cz, r));
        if (q.covers(C) || (cnt == k && b > 0.0f && maxd <= b * b)) break;
    }
    double mx = 0.0, my = 0.0, mz = 0.0;
    for (int j = 0; j < k; ++j) {
        const float4 s = spos[s_p[j][t]];
        knn[(size_t)i * k + j] = __float_as_int(s.w);
        mx += (double)s.x; my += (double)s.y; mz += (double)s.z;
    }
    mx /= (double)k; my /= (double)k; mz /= (double)k;
    double a00 = 0, a01 = 0, a02 = 0, a11 = 0, a12 = 0, a22 = 0;
    for (int j = 0; j < k; ++j) {
        const float4 s = spos[s_p[j][t]];
        const double dx = (double)s.x - mx, dy = (double)s.y - my, dz = (double)s.z - mz;
        a00 += dx * dx; a01 += dx * dy; a02 += dx * dz; a11 += dy * dy; a12 += dy * dz; a22 += dz * dz;
    }
    double nx, ny, nz;
    smallest_eigvec(a00, a01, a02, a11, a12, a22, nx, ny, nz);
    nrm[3 * (size_t)i] = (float)nx; nrm[3 * (size_t)i + 1] = (float)ny; nrm[3 * (size_t)i + 2] = (float)nz;
}

// ---------------------------------------------------------------------------------------------------------------------------
// c. orientation
__global__ void k_sr_eyes(double cx, double cy, double cz, double radius, int V, double* __restrict__ eyes) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= V) return;
    const double y = 1.0 - 2.0 * ((double)i + 0.5) / (double)V;
    const double r = sqrt(fmax(0.0, 1.0 - y * y));
    const double th = (double)i * 2.39996322972865332;             // pi (3 - sqrt 5)
    eyes[3 * i] = cx + radius * r * cos(th);
    eyes[3 * i + 1] = cy + radius * y;
    eyes[3 * i + 2] = cz + radius * r * sin(th);
}

// rule 1: the eyes that see a point vote with the side of its tangent plane they are on.  state: 0 undecided, 1 / 2 / 3 = the rule
__global__ void k_sr_orient_eyes(const float* __restrict__ P, int N, const double* __restrict__ eyes, int V, const uint8_t* __restrict__ vis,
                                 float* __restrict__ nrm, int* __restrict__ state, int* __restrict__ cnt) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    const double px = P[3 * i], py = P[3 * i + 1], pz = P[3 * i + 2];
    const double nx = nrm[3 * i], ny = nrm[3 * i + 1], nz = nrm[3 * i + 2];
    int s = 0;
    for (int v = 0; v < V; ++v) {
        if (!vis[(size_t)v * N + i]) continue;
        const double d = nx * (eyes[3 * v] - px) + ny * (eyes[3 * v + 1] - py) + nz * (eyes[3 * v + 2] - pz);
        s += d > 0.0 ? 1 : (d < 0.0 ? -1 : 0);
    }
    if (s < 0) { nrm[3 * i] = -nrm[3 * i]; nrm[3 * i + 1] = -nrm[3 * i + 1]; nrm[3 * i + 2] = -nrm[3 * i + 2]; }
    state[i] = s != 0 ? 1 : 0;
    if (s != 0) atomicAdd(&cnt[0], 1);
}

// rule 2, one Jacobi round: an undecided point takes the majority of sign(n_i . n_j) over its decided neighbours.  The round
// copies everything else, so once a round changes nothing both buffers are equal and the later rounds return at once.
__global__ void k_sr_orient_round(const int* __restrict__ knn, int k, int N, const float* __restrict__ nin, const int* __restrict__ sin,
                                  float* __restrict__ nout, int* __restrict__ sout, const int* __restrict__ changed_prev,
                                  int* __restrict__ changed, int* __restrict__ cnt) {
    if (changed_prev && *changed_prev == 0) return;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    float nx = nin[3 * i], ny = nin[3 * i + 1], nz = nin[3 * i + 2];
    int st = sin[i];
    if (st == 0) {
        int s = 0;
        for (int j = 0; j < k; ++j) {
            const int q = knn[(size_t)i * k + j];
            if (sin[q] == 0) continue;
            const float d = (nx * nin[3 * q] + ny * nin[3 * q + 1]) + nz * nin[3 * q + 2];
            s += d > 0.f ? 1 : (d < 0.f ? -1 : 0);
        }
        if (s != 0) {
            if (s < 0) { nx = -nx; ny = -ny; nz = -nz; }
            st = 2;
            atomicAdd(changed, 1);
            atomicAdd(&cnt[1], 1);
        }
    }
    nout[3 * i] = nx; nout[3 * i + 1] = ny; nout[3 * i + 2] = nz;
    sout[i] = st;
}

// rule 3: what is still undecided keeps the sign of its nearest decided neighbour (none among its k: it stays as it is, counts[3])
__global__ void k_sr_orient_last(const float* __restrict__ P, const int* __restrict__ knn, int k, int N, const float* __restrict__ nin,
                                 const int* __restrict__ sin, float* __restrict__ nout, int* __restrict__ cnt) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    float nx = nin[3 * i], ny = nin[3 * i + 1], nz = nin[3 * i + 2];
    if (sin[i] == 0) {
        int best = -1;
        float bd = 3.0e38f;
        for (int j = 0; j < k; ++j) {
            const int q = knn[(size_t)i * k + j];
            if (sin[q] == 0) continue;
            const float dx = P[3 * q] - P[3 * i], dy = P[3 * q + 1] - P[3 * i + 1], dz = P[3 * q + 2] - P[3 * i + 2];
            const float d = (dx * dx + dy * dy) + dz * dz;
            if (d < bd || (d == bd && q < best)) { bd = d; best = q; }
        }
        if (best >= 0) {
            const float d = (nx * nin[3 * best] + ny * nin[3 * best + 1]) + nz * nin[3 * best + 2];
            if (d < 0.f) { nx = -nx; ny = -ny; nz = -nz; }
            atomicAdd(&cnt[2], 1);
        } else {
            atomicAdd(&cnt[3], 1);
        }
    }
    nout[3 * i] = nx; nout[3 * i + 1] = ny; nout[3 * i + 2] = nz;
}

// ---------------------------------------------------------------------------------------------------------------------------
// d. Poisson.  Sample weights: a_p = 1 / sum_q w(|p - q|); snrm (sorted order) = a_p * unit normal
__global__ void k_sr_sample_weights(const float4* __restrict__ spos, const int* __restrict__ cstart, CellGrid g, int N, float invR2,
                                    const float* __restrict__ nrm, float4* __restrict__ snrm) {
    const int sp = blockIdx.x * blockDim.x + threadIdx.x;
    if (sp >= N) return;
    const float4 me = spos[sp];
    const int C = g.C;
    const int cx = cell_of(me.x, g.ox, g.cs, C), cy = cell_of(me.y, g.oy, g.cs, C), cz = cell_of(me.z, g.oz, g.cs, C);
    float rho = 0.f;
    const CellCube q = cube_around(cx, cy, cz, 1, C);
    for (int z = q.z0; z <= q.z1; ++z)
        for (int y = q.y0; y <= q.y1; ++y)
            for (int x = q.x0; x <= q.x1; ++x) {
                const int c = (z * C + y) * C + x;
                const int e = cstart[c + 1];
                for (int p = cstart[c]; p < e; ++p) {
                    const float4 s = spos[p];
                    const float dx = s.x - me.x, dy = s.y - me.y, dz = s.z - me.z;
                    const float u = 1.0f - ((dx * dx + dy * dy) + dz * dz) * invR2;
                    if (u > 0.f) rho += (u * u) * u;
                }
            }
    const int i = __float_as_int(me.w);
    const float nx = nrm[3 * i], ny = nrm[3 * i + 1], nz = nrm[3 * i + 2];
    const float l = sqrtf((nx * nx + ny * ny) + nz * nz);
    float a = 0.f;
    if (l > 0.f && l <= 3.0e38f && rho > 0.f) a = 1.0f / (l * rho);
    snrm[sp] = make_float4(nx * a, ny * a, nz * a, 0.f);
}

struct Grid {
    float ox, oy, oz, h;          // node (i, j, k) lies at o + (i, j, k) h
    int M;                        // nodes per axis = 2^depth + 1
};

// right-hand side of A chi = f, A = 6 I - (sum of the six neighbours), f = -div V (the factor h^2 is dropped: only the level set counts)
__global__ void k_sr_rhs(const float4* __restrict__ spos, const float4* __restrict__ snrm, const int* __restrict__ cstart, CellGrid g, Grid G,
                         float R, float* __restrict__ f) {
    const long long n = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const int M = G.M;
    if (n >= (long long)M * M * M) return;
    const int i = (int)(n % M), j = (int)((n / M) % M), k = (int)(n / ((long long)M * M));
    float acc = 0.f;
    if (i > 0 && j > 0 && k > 0 && i < M - 1 && j < M - 1 && k < M - 1) {
        const float x = G.ox + (float)i * G.h, y = G.oy + (float)j * G.h, z = G.oz + (float)k * G.h;
        const int C = g.C;
        const int cx = (int)floorf((x - g.ox) / g.cs), cy = (int)floorf((y - g.oy) / g.cs), cz = (int)floorf((z - g.oz) / g.cs);
        const float invR2 = 1.0f / (R * R);
        const CellCube q = cube_around(cx, cy, cz, 1, C);          // (a node outside the cell grid: the cells within one of it, maybe none)
        for (int zz = q.z0; zz <= q.z1; ++zz)
            for (int yy = q.y0; yy <= q.y1; ++yy)
                for (int xx = q.x0; xx <= q.x1; ++xx) {
                    const int c = (zz * C + yy) * C + xx;
                    const int e = cstart[c + 1];
                    for (int p = cstart[c]; p < e; ++p) {
                        const float4 s = spos[p];
                        const float dx = x - s.x, dy = y - s.y, dz = z - s.z;
                        const float u = 1.0f - ((dx * dx + dy * dy) + dz * dz) * invR2;
                        if (u > 0.f) {
                            const float4 nn = snrm[p];
                            acc += (u * u) * ((nn.x * dx + nn.y * dy) + nn.z * dz);       // div V up to the constant 6 / R^2
                        }
                    }
                }
    }
    f[n] = -acc;
}

// sum of a[0 .. n) by every thread of the block, fixed order
__device__ __forceinline__ double block_sum(const double* __restrict__ a, int n, double* sh) {
    const int t = threadIdx.x;
    double v = 0.0;
    for (int i = t; i < n; i += CG_T) v += a[i];
    sh[t] = v;
    __syncthreads();
    for (int off = CG_T / 2; off > 0; off >>= 1) {
        if (t < off) sh[t] += sh[t + off];
        __syncthreads();
    }
    const double r = sh[0];
    __syncthreads();
    return r;
}
__device__ __forceinline__ void block_reduce_store(double v, double* sh, double* __restrict__ out) {
    const int t = threadIdx.x;
    sh[t] = v;
    __syncthreads();
    for (int off = CG_T / 2; off > 0; off >>= 1) {
        if (t < off) sh[t] += sh[t + off];
        __syncthreads();
    }
    if (t == 0) out[blockIdx.x] = sh[0];
    __syncthreads();
}

// x = 0, r = f, partial sums of f . f
__global__ __launch_bounds__(CG_T) void k_sr_cg_init(const float* __restrict__ f, float* __restrict__ x, float* __restrict__ r, long long n3,
                                                     double* __restrict__ part_ff, double* __restrict__ part_rr) {
    __shared__ double sh[CG_T];
    double acc = 0.0;
    for (long long n = (long long)blockIdx.x * CG_T + threadIdx.x; n < n3; n += (long long)CG_NB * CG_T) {
        const float v = f[n];
        x[n] = 0.f;
        r[n] = v;
        acc += (double)v * (double)v;
    }
    block_reduce_store(acc, sh, part_ff);
    if (threadIdx.x == 0) part_rr[blockIdx.x] = part_ff[blockIdx.x];
}

// first launch of iteration `it`: beta = rr / rr_prev, p = r + beta p, q = A p = A r + beta q, partial sums of p . q
__global__ __launch_bounds__(CG_T) void k_sr_cg_pq(const float* __restrict__ r, float* __restrict__ p, float* __restrict__ q, int M, int it,
                                                   const double* __restrict__ part_ff, const double* __restrict__ part_rr_cur,
                                                   const double* __restrict__ part_rr_prev, double* __restrict__ part_pq, float tol2,
                                                   int* __restrict__ misc) {
    __shared__ double sh[CG_T];
    if (misc[M_SEEN]) return;
    const double ff = block_sum(part_ff, CG_NB, sh);
    const double rr = block_sum(part_rr_cur, CG_NB, sh);
    if (!(rr > (double)tol2 * ff)) {                              // converged (or f = 0, or a NaN: the host looks at the residual)
        if (blockIdx.x == 0 && threadIdx.x == 0) {
            misc[M_ITERS] = it;
            misc[M_RES] = __float_as_int(ff > 0.0 ? (float)sqrt(rr / ff) : 0.f);
            misc[M_DONE] = 1;
        }
        return;
    }
    float beta = 0.f;
    if (it > 0) beta = (float)(rr / block_sum(part_rr_prev, CG_NB, sh));
    const long long M2 = (long long)M * M, n3 = M2 * M;
    double acc = 0.0;
    for (long long n = (long long)blockIdx.x * CG_T + threadIdx.x; n < n3; n += (long long)CG_NB * CG_T) {
        const int i = (int)(n % M), j = (int)((n / M) % M), k = (int)(n / M2);
        if (i == 0 || j == 0 || k == 0 || i == M - 1 || j == M - 1 || k == M - 1) continue;      // boundary nodes stay 0
        const float rc = r[n];
        const float ar = 6.0f * rc - (((r[n - 1] + r[n + 1]) + (r[n - M] + r[n + M])) + (r[n - M2] + r[n + M2]));
        float pn = rc, qn = ar;
        if (it > 0) { pn = rc + beta * p[n]; qn = ar + beta * q[n]; }
        p[n] = pn;
        q[n] = qn;
        acc += (double)pn * (double)qn;
    }
    block_reduce_store(acc, sh, part_pq);
}

// second launch: alpha = rr / (p . q), x += alpha p, r -= alpha q, partial sums of the new r . r
__global__ __launch_bounds__(CG_T) void k_sr_cg_xr(float* __restrict__ x, float* __restrict__ r, const float* __restrict__ p,
                                                   const float* __restrict__ q, long long n3, const double* __restrict__ part_rr_cur,
                                                   const double* __restrict__ part_pq, double* __restrict__ part_rr_next,
                                                   int* __restrict__ misc) {
    __shared__ double sh[CG_T];
    if (misc[M_DONE]) {
        if (blockIdx.x == 0 && threadIdx.x == 0) misc[M_SEEN] = 1;
        return;
    }
    const double rr = block_sum(part_rr_cur, CG_NB, sh);
    const double pq = block_sum(part_pq, CG_NB, sh);
    const float alpha = pq > 0.0 ? (float)(rr / pq) : 0.f;
    double acc = 0.0;
    for (long long n = (long long)blockIdx.x * CG_T + threadIdx.x; n < n3; n += (long long)CG_NB * CG_T) {
        const float pn = p[n], qn = q[n];
        x[n] = x[n] + alpha * pn;
        const float rn = r[n] - alpha * qn;
        r[n] = rn;
        acc += (double)rn * (double)rn;
    }
    block_reduce_store(acc, sh, part_rr_next);
}
// (p and q are read on the boundary by k_sr_cg_xr: they are cleared once before the first iteration)

__global__ __launch_bounds__(CG_T) void k_sr_cg_status(const double* __restrict__ part_ff, const double* __restrict__ part_rr, int* __restrict__ misc) {
    __shared__ double sh[CG_T];
    const double ff = block_sum(part_ff, CG_NB, sh);
    const double rr = block_sum(part_rr, CG_NB, sh);
    if (threadIdx.x == 0 && !misc[M_DONE]) misc[M_RES] = __float_as_int(ff > 0.0 ? (float)sqrt(rr / ff) : 0.f);
}

// e. iso value
__device__ __forceinline__ float trilinear(const float* __restrict__ chi, Grid G, float x, float y, float z) {
    const int M = G.M;
    const float gx = fminf(fmaxf((x - G.ox) / G.h, 0.f), (float)(M - 1)), gy = fminf(fmaxf((y - G.oy) / G.h, 0.f), (float)(M - 1)),
                gz = fminf(fmaxf((z - G.oz) / G.h, 0.f), (float)(M - 1));
    const int i = min((int)gx, M - 2), j = min((int)gy, M - 2), k = min((int)gz, M - 2);
    const float tx = gx - (float)i, ty = gy - (float)j, tz = gz - (float)k;
    const size_t M2 = (size_t)M * M, n = (size_t)k * M2 + (size_t)j * M + i;
    const float c00 = chi[n] + tx * (chi[n + 1] - chi[n]), c10 = chi[n + M] + tx * (chi[n + M + 1] - chi[n + M]);
    const float c01 = chi[n + M2] + tx * (chi[n + M2 + 1] - chi[n + M2]), c11 = chi[n + M2 + M] + tx * (chi[n + M2 + M + 1] - chi[n + M2 + M]);
    const float c0 = c00 + ty * (c10 - c00), c1 = c01 + ty * (c11 - c01);
    return c0 + tz * (c1 - c0);
}
__global__ __launch_bounds__(CG_T) void k_sr_iso(const float* __restrict__ chi, Grid G, const float* __restrict__ P, int N, int* __restrict__ misc) {
    __shared__ double sh[CG_T];
    double acc = 0.0;
    for (int i = threadIdx.x; i < N; i += CG_T) acc += (double)trilinear(chi, G, P[3 * i], P[3 * i + 1], P[3 * i + 2]);
    const int t = threadIdx.x;
    sh[t] = acc;
    __syncthreads();
    for (int off = CG_T / 2; off > 0; off >>= 1) {
        if (t < off) sh[t] += sh[t + off];
        __syncthreads();
    }
    if (t == 0) misc[M_ISO] = __float_as_int((float)(sh[0] / (double)N));
}

// ---------------------------------------------------------------------------------------------------------------------------
// f. marching cubes.  A node owns the three grid edges that leave it in +x, +y, +z; inside = chi > iso
__global__ void k_sr_mc_mark(const float* __restrict__ chi, int M, const int* __restrict__ misc, int* __restrict__ vcnt, uint8_t* __restrict__ eflag) {
    const long long n = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long M2 = (long long)M * M;
    if (n >= M2 * M) return;
    const float iso = __int_as_float(misc[M_ISO]);
    const int i = (int)(n % M), j = (int)((n / M) % M), k = (int)(n / M2);
    const bool in0 = chi[n] > iso;
    int fl = 0;
    if (i + 1 < M && (chi[n + 1] > iso) != in0) fl |= 1;
    if (j + 1 < M && (chi[n + M] > iso) != in0) fl |= 2;
    if (k + 1 < M && (chi[n + M2] > iso) != in0) fl |= 4;
    eflag[n] = (uint8_t)fl;
    vcnt[n] = __popc(fl);
}
__device__ __forceinline__ int mc_case(const float* __restrict__ chi, long long n, int M, long long M2, float iso) {
    int m = 0;
    m |= (chi[n] > iso) ? 1 : 0;
    m |= (chi[n + 1] > iso) ? 2 : 0;
    m |= (chi[n + M] > iso) ? 4 : 0;
    m |= (chi[n + M + 1] > iso) ? 8 : 0;
    m |= (chi[n + M2] > iso) ? 16 : 0;
    m |= (chi[n + M2 + 1] > iso) ? 32 : 0;
    m |= (chi[n + M2 + M] > iso) ? 64 : 0;
    m |= (chi[n + M2 + M + 1] > iso) ? 128 : 0;
    return m;
}
__global__ void k_sr_mc_count(const float* __restrict__ chi, int M, const int* __restrict__ misc, int* __restrict__ tcnt) {
    const long long n = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long M2 = (long long)M * M;
    if (n >= M2 * M) return;
    const int i = (int)(n % M), j = (int)((n / M) % M), k = (int)(n / M2);
    int c = 0;
    if (i + 1 < M && j + 1 < M && k + 1 < M) c = c_mc_ntri[mc_case(chi, n, M, M2, __int_as_float(misc[M_ISO]))];
    tcnt[n] = c;
}
__global__ void k_sr_mc_totals(const int* __restrict__ vcnt, const int* __restrict__ vbase, const int* __restrict__ tcnt,
                               const int* __restrict__ tbase, long long n3, int* __restrict__ misc) {
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        misc[M_NV] = vbase[n3 - 1] + vcnt[n3 - 1];
        misc[M_NF] = tbase[n3 - 1] + tcnt[n3 - 1];
    }
}
__global__ void k_sr_mc_vertices(const float* __restrict__ chi, Grid G, const int* __restrict__ misc, const uint8_t* __restrict__ eflag,
                                 const int* __restrict__ vbase, float* __restrict__ verts, int vcap) {
    const long long n = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const int M = G.M;
    const long long M2 = (long long)M * M;
    if (n >= M2 * M) return;
    const int fl = eflag[n];
    if (!fl) return;
    const float iso = __int_as_float(misc[M_ISO]);
    const int i = (int)(n % M), j = (int)((n / M) % M), k = (int)(n / M2);
    const float a = chi[n];
    int id = vbase[n];
#pragma unroll
    for (int ax = 0; ax < 3; ++ax) {
        if (!((fl >> ax) & 1)) continue;
        const float b = chi[n + (ax == 0 ? 1 : (ax == 1 ? (long long)M : M2))];
        float t = (iso - a) / (b - a);
        t = fminf(fmaxf(t, 1.0f / 1024.0f), 1.0f - 1.0f / 1024.0f);      // a vertex never sits on a node: no two vertices coincide
        if (!(t == t)) t = 0.5f;
        if (id < vcap) {
            verts[3 * (size_t)id] = G.ox + ((float)i + (ax == 0 ? t : 0.f)) * G.h;
            verts[3 * (size_t)id + 1] = G.oy + ((float)j + (ax == 1 ? t : 0.f)) * G.h;
            verts[3 * (size_t)id + 2] = G.oz + ((float)k + (ax == 2 ? t : 0.f)) * G.h;
        }
        ++id;
    }
}
__global__ void k_sr_mc_faces(const float* __restrict__ chi, int M, const int* __restrict__ misc, const uint8_t* __restrict__ eflag,
                              const int* __restrict__ vbase, const int* __restrict__ tcnt, const int* __restrict__ tbase,
                              int64_t* __restrict__ faces, int fcap) {
    const long long n = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long M2 = (long long)M * M;
    if (n >= M2 * M) return;
    const int nt = tcnt[n];
    if (!nt) return;
    const int m = mc_case(chi, n, M, M2, __int_as_float(misc[M_ISO]));
    const int base = tbase[n];
    for (int t = 0; t < nt; ++t) {
        if (base + t >= fcap) return;
        for (int c = 0; c < 3; ++c) {
            const int e = c_mc_tri[m][3 * t + c];
            const int ax = e >> 2, u = e & 1, v = (e >> 1) & 1;
            // offsets along the two other axes, in increasing axis order
            const int dx = ax == 0 ? 0 : u, dy = ax == 1 ? 0 : (ax == 0 ? u : v), dz = ax == 2 ? 0 : v;
            const long long nn = n + dx + (long long)dy * M + (long long)dz * M2;
            const int fl = eflag[nn];
            const int rank = __popc(fl & ((1 << ax) - 1));
            faces[3 * (size_t)(base + t) + c] = (int64_t)(vbase[nn] + rank);
        }
    }
}

// colour of the nearest cloud point (ties: the first in cell order)
__global__ void k_sr_nearest_color(const float* __restrict__ Q, int nq, const float4* __restrict__ spos, const int* __restrict__ cstart,
                                   CellGrid g, const float* __restrict__ colors, float* __restrict__ out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nq) return;
    const float qx = Q[3 * i], qy = Q[3 * i + 1], qz = Q[3 * i + 2];
    const int C = g.C;
    const int cx = cell_of(qx, g.ox, g.cs, C), cy = cell_of(qy, g.oy, g.cs, C), cz = cell_of(qz, g.oz, g.cs, C);
    int best = -1;
    float bd = 3.0e38f;
    for (int r = 1;; ++r) {
        best = -1; bd = 3.0e38f;
        const CellCube q = cube_around(cx, cy, cz, r, C);
        for (int z = q.z0; z <= q.z1; ++z)
            for (int y = q.y0; y <= q.y1; ++y)
                for (int x = q.x0; x <= q.x1; ++x) {
                    const int c = (z * C + y) * C + x;
                    const int e = cstart[c + 1];
                    for (int p = cstart[c]; p < e; ++p) {
                        const float4 s = spos[p];
                        const float dx = s.x - qx, dy = s.y - qy, dz = s.z - qz;
                        const float d = (dx * dx + dy * dy) + dz * dz;
                        if (d < bd) { bd = d; best = __float_as_int(s.w); }
                    }
                }
        // (the bound is measured from the query itself to the faces of the scanned cube that are not faces of the grid: a point that was
        // not scanned lies beyond one of them, also when the query is outside the grid and its cell was clamped)
        const float b = fminf(fminf(ring_bound(qx, g.ox, g.cs, C, cx, r), ring_bound(qy, g.oy, g.cs, C, cy, r)),
                              ring_bound(qz, g.oz, g.cs, C, cz, r));
        if (q.covers(C) || (best >= 0 && b > 0.0f && bd <= b * b)) break;
    }
    out[3 * i] = colors[3 * best]; out[3 * i + 1] = colors[3 * best + 1]; out[3 * i + 2] = colors[3 * best + 2];
}

// ---------------------------------------------------------------------------------------------------------------------------
constexpr int CELLS_MAX = 128;                                     // cells per axis of a point cell list

struct Cells {
    SortBufs sb;
    int* cstart;
    float4* spos;
    double* mom;
};
static void carve_cells(Carve& c, Cells& w, int N) {
    carve_sort(c, w.sb, N);
    // cstart[0 .. nc] needs CELLS_MAX^3 + 1 ints.  It takes twice CELLS_MAX^3: this region was a start and an end table of that size, back to
    // back, and the sizes that pdhip_estimate_normals_ws_bytes / pdhip_surface_recon_ws_bytes report are pinned (tests/test_ws_bytes_cpu.py)
    w.cstart = c.take<int>(2 * (size_t)CELLS_MAX * CELLS_MAX * CELLS_MAX);
    w.spos = c.take<float4>(N);
    w.mom = c.take<double>(MOM_WORDS);
}

struct Box {
    double mn[3], mx[3], ext;
};

// bounding box and a rank test of the cloud; synchronises the stream (one small read)
static int cloud_box(const char* who, const float* P, int N, double* mom, hipStream_t s, Box& b) {
    k_sr_moments<<<1, TB, 0, s>>>(P, N, mom);
    PD_LAUNCH_CHECK();
    double h[MOM_WORDS];
    PD_HIP(hipMemcpyAsync(h, mom, sizeof(h), hipMemcpyDeviceToHost, s));
    PD_HIP(hipStreamSynchronize(s));
    PD_REQUIRE(h[MOM_BAD] == 0.0, "%s: %d point(s) with a non-finite coordinate", who, (int)h[MOM_BAD]);
    b.ext = 0.0;
    for (int a = 0; a < 3; ++a) {
        b.mn[a] = h[MOM_MIN + a]; b.mx[a] = h[MOM_MAX + a];
        b.ext = std::max(b.ext, b.mx[a] - b.mn[a]);
    }
    PD_REQUIRE(b.ext > 0.0, "%s: all %d points are equal", who, N);
    const double n = (double)N, m0 = h[MOM_SUM] / n, m1 = h[MOM_SUM + 1] / n, m2 = h[MOM_SUM + 2] / n;
    const double c00 = h[9] / n - m0 * m0, c01 = h[10] / n - m0 * m1, c02 = h[11] / n - m0 * m2, c11 = h[12] / n - m1 * m1,
                 c12 = h[13] / n - m1 * m2, c22 = h[14] / n - m2 * m2;
    const double det = c00 * (c11 * c22 - c12 * c12) - c01 * (c01 * c22 - c12 * c02) + c02 * (c01 * c12 - c11 * c02);
    const double tr = (c00 + c11 + c22) / 3.0;
    PD_REQUIRE(det > 1.0e-9 * tr * tr * tr, "%s: the points lie on a plane or a line (covariance determinant %.3g, mean variance %.3g): "
               "no closed surface to reconstruct", who, det, tr);
    return PDHIP_OK;
}

// cell list of cell size >= cs_min over the cloud's bounding cube
static int build_cells(Cells& w, const float* P, int N, const Box& b, double cs_min, int cmax, CellGrid& g, hipStream_t s) {
    int C = (int)floor(b.ext / cs_min);
    C = std::max(1, std::min(C, std::min(cmax, CELLS_MAX)));
    g.C = C;
    g.cs = (float)(b.ext / C * (1.0 + 1.0e-6));
    g.ox = (float)b.mn[0]; g.oy = (float)b.mn[1]; g.oz = (float)b.mn[2];
    const int cur = sort_by_cell(w.sb, N, SrKey{P, g}, (unsigned long long)C * C * C, w.cstart, s);
    k_gather_xyzi<<<cdiv(N, TB), TB, 0, s>>>(w.sb.v[cur], P, N, w.spos);
    PD_LAUNCH_CHECK();
    return PDHIP_OK;
}

struct NormWs {
    Cells cells;
    int *knn, *state[2], *changed, *cnt;
    float* nbuf;
    double* eyes;
    uint8_t* vis;
    void* hpr;
};
static size_t carve_norm(NormWs& w, void* base, int N, int k, int V) {
    Carve c{static_cast<char*>(base), 0};
    carve_cells(c, w.cells, N);
    w.knn = c.take<int>((size_t)N * k);
    w.state[0] = c.take<int>(N); w.state[1] = c.take<int>(N);
    w.changed = c.take<int>(ORIENT_ROUNDS + 8);
    w.cnt = w.changed + ORIENT_ROUNDS;
    w.nbuf = c.take<float>(3 * (size_t)N);
    w.eyes = c.take<double>(3 * (size_t)V);
    w.vis = c.take<uint8_t>((size_t)V * N);
    w.hpr = c.take<char>(pdhip_hpr_ws_bytes(V, N));
    return c.off + 256;
}

struct ReconWs {
    Cells cells;
    float4* snrm;
    float *chi, *r, *p, *q, *f;
    uint8_t* eflag;
    double *part_ff, *part_rr[2], *part_pq;
    int *misc, *tsum, *toff;
};
static size_t carve_recon(ReconWs& w, void* base, int N, int depth) {
    const size_t M = ((size_t)1 << depth) + 1, n3 = M * M * M;
    Carve c{static_cast<char*>(base), 0};
    carve_cells(c, w.cells, N);
    w.snrm = c.take<float4>(N);
    w.chi = c.take<float>(n3); w.r = c.take<float>(n3); w.p = c.take<float>(n3); w.q = c.take<float>(n3); w.f = c.take<float>(n3);
    w.eflag = c.take<uint8_t>(n3);
    w.part_ff = c.take<double>(CG_NB); w.part_rr[0] = c.take<double>(CG_NB); w.part_rr[1] = c.take<double>(CG_NB);
    w.part_pq = c.take<double>(CG_NB);
    w.misc = c.take<int>(M_WORDS);
    w.tsum = c.take<int>(scan_tiles(n3)); w.toff = c.take<int>(scan_tiles(n3));
    return c.off + 256;
}

// the front half of pdhip_surface_recon, which pdhip_debug_surface_recon_rhs runs alone: the box, the grid, the splat radius, the cell list, the
// sample weights and the right-hand side in w.f
static int recon_rhs(const char* who, const float* points, const float* normals, int N, int depth, ReconWs& w, Grid& G, CellGrid& g, float& R,
                     hipStream_t s) {
    Box b;
    int rc = cloud_box(who, points, N, w.cells.mom, s, b);
    if (rc) return rc;
    // grid: 2^depth cells per axis, the cloud's bounding cube in the middle with 2^depth / 8 cells of margin on every side
    const int Gc = 1 << depth, M = Gc + 1, margin = Gc / 8;
    G.M = M;
    G.h = (float)(b.ext / (double)(Gc - 2 * margin));
    G.ox = (float)(0.5 * (b.mn[0] + b.mx[0]) - 0.5 * Gc * (double)G.h);
    G.oy = (float)(0.5 * (b.mn[1] + b.mx[1]) - 0.5 * Gc * (double)G.h);
    G.oz = (float)(0.5 * (b.mn[2] + b.mx[2]) - 0.5 * Gc * (double)G.h);
    // support radius of the splat: 2.5 cells, but not below ~2.3 sample spacings of a surface of area ext^2 * 3
    R = (float)std::max(2.5 * (double)G.h, 4.0 * b.ext / sqrt((double)N));
    rc = build_cells(w.cells, points, N, b, (double)R, CELLS_MAX, g, s);
    if (rc) return rc;
    const long long n3 = (long long)M * M * M;
    k_sr_sample_weights<<<cdiv(N, TB), TB, 0, s>>>(w.cells.spos, w.cells.cstart, g, N, 1.0f / (R * R), normals, w.snrm);
    k_sr_rhs<<<cdiv(n3, TB), TB, 0, s>>>(w.cells.spos, w.snrm, w.cells.cstart, g, G, R, w.f);
    PD_LAUNCH_CHECK();
    return PDHIP_OK;
}

}  // namespace

extern "C" size_t pdhip_estimate_normals_ws_bytes(int N, int k, int n_eyes) {
    if (N < 16 || k < 3 || k > KMAX || k > N || n_eyes < 1 || n_eyes > 64) return 0;
    NormWs w;
    return carve_norm(w, nullptr, N, k, n_eyes);
}

extern "C" int pdhip_estimate_normals(const float* points, int N, int k, int n_eyes, double eye_radius, float* normals, int32_t* counts,
                                      void* ws, void* stream) {
    PD_REQUIRE(points && normals && counts && ws, "pdhip_estimate_normals: null pointer");
    PD_REQUIRE(N >= 16 && N <= (1 << 24), "pdhip_estimate_normals: N=%d points, need 16 .. 2^24", N);
    PD_REQUIRE(k >= 3 && k <= KMAX && k <= N, "pdhip_estimate_normals: k=%d neighbours, need 3 .. %d", k, KMAX);
    PD_REQUIRE(n_eyes >= 1 && n_eyes <= 64, "pdhip_estimate_normals: n_eyes=%d, need 1 .. 64", n_eyes);
    PD_REQUIRE(eye_radius > 0.0 && eye_radius <= 1.0e6, "pdhip_estimate_normals: eye_radius=%g (in units of the cloud's largest extent) must be positive", eye_radius);
    hipStream_t s = as_stream(stream);
    NormWs w;
    carve_norm(w, ws, N, k, n_eyes);
    Box b;
    int rc = cloud_box("pdhip_estimate_normals", points, N, w.cells.mom, s, b);
    if (rc) return rc;
    // about k + 2 points per occupied cell of a surface: the k-th neighbour is usually certified by the first ring
    CellGrid g;
    rc = build_cells(w.cells, points, N, b, b.ext / std::max(1.0, sqrt((double)N / (k + 2.0))), CELLS_MAX, g, s);
    if (rc) return rc;
    k_sr_knn_normals<<<cdiv(N, KNN_T), KNN_T, 0, s>>>(w.cells.spos, w.cells.cstart, g, N, k, w.knn, normals);
    // rule 1
    k_sr_eyes<<<1, 64, 0, s>>>(0.5 * (b.mn[0] + b.mx[0]), 0.5 * (b.mn[1] + b.mx[1]), 0.5 * (b.mn[2] + b.mx[2]), eye_radius * b.ext, n_eyes, w.eyes);
    PD_LAUNCH_CHECK();
    rc = pdhip_hidden_point_removal(points, N, w.eyes, n_eyes, HPR_RADIUS, nullptr, w.vis, w.hpr, stream);
    if (rc) return rc;
    PD_HIP(hipMemsetAsync(w.changed, 0, (ORIENT_ROUNDS + 8) * sizeof(int), s));
    k_sr_orient_eyes<<<cdiv(N, TB), TB, 0, s>>>(points, N, w.eyes, n_eyes, w.vis, normals, w.state[0], w.cnt);
    // rule 2 (normals <-> nbuf, an even number of rounds: the result is back in `normals`)
    float* nb[2] = {normals, w.nbuf};
    for (int r = 0; r < ORIENT_ROUNDS; ++r)
        k_sr_orient_round<<<cdiv(N, TB), TB, 0, s>>>(w.knn, k, N, nb[r & 1], w.state[r & 1], nb[(r & 1) ^ 1], w.state[(r & 1) ^ 1],
                                                     r > 0 ? w.changed + r - 1 : nullptr, w.changed + r, w.cnt);
    // rule 3 (a skipped round leaves both buffers equal, so reading buffer 0 is right either way; the result goes to nbuf, then home)
    k_sr_orient_last<<<cdiv(N, TB), TB, 0, s>>>(points, w.knn, k, N, normals, w.state[0], w.nbuf, w.cnt);
    PD_LAUNCH_CHECK();
    PD_HIP(hipMemcpyAsync(normals, w.nbuf, 3 * (size_t)N * sizeof(float), hipMemcpyDeviceToDevice, s));
    PD_HIP(hipMemcpyAsync(counts, w.cnt, 4 * sizeof(int), hipMemcpyDeviceToDevice, s));
    return PDHIP_OK;
}

extern "C" size_t pdhip_surface_recon_ws_bytes(int N, int depth) {
    if (N < 16 || depth < 6 || depth > 8) return 0;
    ReconWs w;
    return carve_recon(w, nullptr, N, depth);
}

extern "C" int pdhip_surface_recon(const float* points, const float* normals, const float* colors, int N, int depth, float* vertices,
                                   int vertex_capacity, int64_t* faces, int face_capacity, float* vertex_colors, int32_t* counts,
                                   float* info, void* ws, void* stream) {
    PD_REQUIRE(points && normals && vertices && faces && counts && info && ws, "pdhip_surface_recon: null pointer");
    PD_REQUIRE((colors == nullptr) == (vertex_colors == nullptr), "pdhip_surface_recon: colors and vertex_colors go together");
    PD_REQUIRE(N >= 16 && N <= (1 << 24), "pdhip_surface_recon: N=%d points, need 16 .. 2^24", N);
    PD_REQUIRE(depth >= 6 && depth <= 8, "pdhip_surface_recon: depth=%d, the dense grid supports 6 .. 8", depth);
    PD_REQUIRE(vertex_capacity > 0 && face_capacity > 0, "pdhip_surface_recon: capacities must be positive (got %d vertices, %d faces)",
               vertex_capacity, face_capacity);
    hipStream_t s = as_stream(stream);
    ReconWs w;
    carve_recon(w, ws, N, depth);
    Grid G;
    CellGrid g;
    float R;
    int rc = recon_rhs("pdhip_surface_recon", points, normals, N, depth, w, G, g, R, s);
    if (rc) return rc;
    const int Gc = 1 << depth, M = G.M;
    const long long n3 = (long long)M * M * M;
    const int gN3 = cdiv(n3, TB);
    PD_HIP(hipMemsetAsync(w.misc, 0, M_WORDS * sizeof(int), s));
    PD_HIP(hipMemsetAsync(w.p, 0, (size_t)n3 * sizeof(float), s));
    PD_HIP(hipMemsetAsync(w.q, 0, (size_t)n3 * sizeof(float), s));
    k_sr_cg_init<<<CG_NB, CG_T, 0, s>>>(w.f, w.chi, w.r, n3, w.part_ff, w.part_rr[0]);
    PD_LAUNCH_CHECK();
    const int cap = 24 * Gc;
    int hm[M_WORDS];
    int it = 0;
    while (true) {
        for (int c = 0; c < CG_CHUNK; ++c, ++it) {
            k_sr_cg_pq<<<CG_NB, CG_T, 0, s>>>(w.r, w.p, w.q, M, it, w.part_ff, w.part_rr[it & 1], w.part_rr[(it & 1) ^ 1], w.part_pq,
                                              CG_TOL * CG_TOL, w.misc);
            k_sr_cg_xr<<<CG_NB, CG_T, 0, s>>>(w.chi, w.r, w.p, w.q, n3, w.part_rr[it & 1], w.part_pq, w.part_rr[(it & 1) ^ 1], w.misc);
        }
        k_sr_cg_status<<<1, CG_T, 0, s>>>(w.part_ff, w.part_rr[it & 1], w.misc);
        PD_LAUNCH_CHECK();
        PD_HIP(hipMemcpyAsync(hm, w.misc, sizeof(hm), hipMemcpyDeviceToHost, s));
        PD_HIP(hipStreamSynchronize(s));
        if (hm[M_DONE]) break;
        float res;
        memcpy(&res, &hm[M_RES], sizeof(float));
        PD_REQUIRE(res == res && it < cap, "pdhip_surface_recon: the Poisson solve did not reach a relative residual of %.1e in %d "
                   "iterations (residual %.3e): no mesh is returned", (double)CG_TOL, it, (double)res);
    }
    float res;
    memcpy(&res, &hm[M_RES], sizeof(float));
    PD_REQUIRE(res == res && (res > 0.f || hm[M_ITERS] > 0), "pdhip_surface_recon: the normal field has no divergence on the grid (zero or "
               "non-finite normals?): empty surface");
    // e, f
    int* vcnt = reinterpret_cast<int*>(w.r);
    int* vbase = reinterpret_cast<int*>(w.p);
    int* tcnt = reinterpret_cast<int*>(w.q);
    int* tbase = reinterpret_cast<int*>(w.f);
    k_sr_iso<<<1, CG_T, 0, s>>>(w.chi, G, points, N, w.misc);
    k_sr_mc_mark<<<gN3, TB, 0, s>>>(w.chi, M, w.misc, vcnt, w.eflag);
    scan_exclusive(vcnt, vbase, n3, w.tsum, w.toff, s);
    k_sr_mc_count<<<gN3, TB, 0, s>>>(w.chi, M, w.misc, tcnt);
    scan_exclusive(tcnt, tbase, n3, w.tsum, w.toff, s);
    k_sr_mc_totals<<<1, 64, 0, s>>>(vcnt, vbase, tcnt, tbase, n3, w.misc);
    k_sr_mc_vertices<<<gN3, TB, 0, s>>>(w.chi, G, w.misc, w.eflag, vbase, vertices, vertex_capacity);
    k_sr_mc_faces<<<gN3, TB, 0, s>>>(w.chi, M, w.misc, w.eflag, vbase, tcnt, tbase, faces, face_capacity);
    PD_LAUNCH_CHECK();
    PD_HIP(hipMemcpyAsync(hm, w.misc, sizeof(hm), hipMemcpyDeviceToHost, s));
    PD_HIP(hipStreamSynchronize(s));
    float iso;
    memcpy(&iso, &hm[M_ISO], sizeof(float));
    const int32_t hc[4] = {hm[M_NV], hm[M_NF], hm[M_ITERS], 0};
    const float hi[8] = {G.h, G.ox, G.oy, G.oz, iso, res, R, (float)M};
    PD_HIP(hipMemcpyAsync(counts, hc, sizeof(hc), hipMemcpyHostToDevice, s));
    PD_HIP(hipMemcpyAsync(info, hi, sizeof(hi), hipMemcpyHostToDevice, s));
    PD_HIP(hipStreamSynchronize(s));                              // (hc / hi live on this frame)
    PD_REQUIRE(iso > 0.f && hm[M_NV] > 0 && hm[M_NF] > 0, "pdhip_surface_recon: empty or inverted surface (iso value %.3g, %d vertices, %d "
               "faces): are the normals oriented outwards?", (double)iso, hm[M_NV], hm[M_NF]);
    PD_REQUIRE(hm[M_NV] <= vertex_capacity && hm[M_NF] <= face_capacity, "pdhip_surface_recon: capacities too small: the mesh has %d "
               "vertices and %d faces, the buffers hold %d and %d", hm[M_NV], hm[M_NF], vertex_capacity, face_capacity);
    if (colors) {
        k_sr_nearest_color<<<cdiv(hm[M_NV], TB), TB, 0, s>>>(vertices, hm[M_NV], w.cells.spos, w.cells.cstart, g, colors, vertex_colors);
        PD_LAUNCH_CHECK();
    }
    return PDHIP_OK;
}

// ---- test hooks (include/pdhip.h): where the stages' intermediates lie in the caller's workspace, and the right-hand side, which the solve overwrites.
// (A Carve on a null base hands out null pointers, so the layouts are carved on an address that is never dereferenced and subtracted again.)
static char* const LAYOUT_BASE = reinterpret_cast<char*>((uintptr_t)1 << 20);
static uint64_t layout_offset(const void* p) { return (uint64_t)(static_cast<const char*>(p) - LAYOUT_BASE); }

extern "C" int pdhip_debug_estimate_normals_layout(int N, int k, int n_eyes, uint64_t* off) {
    PD_REQUIRE(off, "pdhip_debug_estimate_normals_layout: null pointer");
    PD_REQUIRE(pdhip_estimate_normals_ws_bytes(N, k, n_eyes) > 0, "pdhip_debug_estimate_normals_layout: N=%d k=%d n_eyes=%d: not a size "
               "pdhip_estimate_normals accepts", N, k, n_eyes);
    NormWs w;
    const size_t total = carve_norm(w, LAYOUT_BASE, N, k, n_eyes);
    const void* at[5] = {w.cells.cstart, w.cells.spos, w.knn, w.eyes, w.vis};
    for (int i = 0; i < 5; ++i) off[i] = layout_offset(at[i]);
    off[5] = (uint64_t)total;
    return PDHIP_OK;
}

extern "C" int pdhip_debug_surface_recon_layout(int N, int depth, uint64_t* off) {
    PD_REQUIRE(off, "pdhip_debug_surface_recon_layout: null pointer");
    PD_REQUIRE(pdhip_surface_recon_ws_bytes(N, depth) > 0, "pdhip_debug_surface_recon_layout: N=%d depth=%d: not a size pdhip_surface_recon "
               "accepts", N, depth);
    ReconWs w;
    const size_t total = carve_recon(w, LAYOUT_BASE, N, depth);
    const void* at[7] = {w.cells.cstart, w.cells.spos, w.snrm, w.chi, w.eflag, w.misc, w.f};
    for (int i = 0; i < 7; ++i) off[i] = layout_offset(at[i]);
    off[7] = (uint64_t)total;
    return PDHIP_OK;
}

extern "C" int pdhip_debug_surface_recon_rhs(const float* points, const float* normals, int N, int depth, float* f_out, float* info, void* ws,
                                             void* stream) {
    PD_REQUIRE(points && normals && f_out && info && ws, "pdhip_debug_surface_recon_rhs: null pointer");
    PD_REQUIRE(N >= 16 && N <= (1 << 24), "pdhip_debug_surface_recon_rhs: N=%d points, need 16 .. 2^24", N);
    PD_REQUIRE(depth >= 6 && depth <= 8, "pdhip_debug_surface_recon_rhs: depth=%d, the dense grid supports 6 .. 8", depth);
    hipStream_t s = as_stream(stream);
    ReconWs w;
    carve_recon(w, ws, N, depth);
    Grid G;
    CellGrid g;
    float R;
    const int rc = recon_rhs("pdhip_debug_surface_recon_rhs", points, normals, N, depth, w, G, g, R, s);
    if (rc) return rc;
    const size_t n3 = (size_t)G.M * G.M * G.M;
    const float hi[8] = {G.h, G.ox, G.oy, G.oz, g.cs, (float)g.C, R, (float)G.M};
    PD_HIP(hipMemcpyAsync(f_out, w.f, n3 * sizeof(float), hipMemcpyDeviceToDevice, s));
    PD_HIP(hipMemcpyAsync(info, hi, sizeof(hi), hipMemcpyHostToDevice, s));
    PD_HIP(hipStreamSynchronize(s));                              // (hi lives on this frame)
    return PDHIP_OK;
}
