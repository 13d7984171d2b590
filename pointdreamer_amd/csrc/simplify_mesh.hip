// Quadric-error edge-collapse decimation of a closed, consistently oriented 2-manifold triangle mesh to a target face count (what
// baselines/spr.py:63-64 asks pymeshlab's meshing_decimation_quadric_edge_collapse(preservetopology=True) for on the CPU; the mesh here
// is this library's own).  Rounds of mutually independent collapses, every phase a launch of its own:
//   once      k_sm_edge_keys -> sort -> k_sm_check      every directed edge once, its reverse once, indices in [0, V), no repeated corner
//             k_sm_init / k_sm_quadrics                 P, colours, remap; Q[v] = sum of area * plane quadric over the sorted edge run of v
//   per round k_sm_count -> scan -> k_sm_fill           vertex -> incident faces (CSR); rows are used as SETS only (tests, integer mins)
//             k_sm_cost                                 per edge (the corner with f[i] < f[i+1]): position, cost, validity; cost histogram
//             k_sm_tau                                  threshold bin so that about need = (F - target) / 2 edges lie at or below it
//             k_sm_claim / k_sm_win                     atomicMin of a unique 64-bit key (hash | u | v) over N[u] + N[v]; all words held = winner
//             scan -> k_sm_winners -> k_sm_apply        winner list in slot order; more than `need`: the `need` smallest (cost, u, v) by rank
//             k_sm_rewrite -> scan -> k_sm_compact      faces through remap, the two collapsed faces per winner dropped, order kept
//             k_sm_round_end                            F, round, stop / stalled
//   once      k_sm_mark -> scan -> k_sm_out_*           referenced vertices in input order, faces as int64, counts
// Quadrics, costs and positions are f64 (positions are rounded to f32 BEFORE cost and validity, so what is judged is what is stored).
// Nothing depends on the order the CSR rows were filled in or on the order atomics arrive (integer add / sub / min only): two calls give
// equal bytes.  The host reads the status words once per BATCH rounds; kernels launched after the stop return at once.
#include "mesh_common.h"
using namespace pdhip;

namespace {

constexpr int TB = 256;
constexpr int ID_BITS = 22;                                       // vertex id width inside the 64-bit claim key (hash 20 | u 22 | v 22)
constexpr int MAX_V = 1 << ID_BITS, MAX_F = MESH_MAX_F;           // (MAX_V: the key width, not MESH_MAX_V)
constexpr int MAX_ROUNDS = 1024, BATCH = 8;
constexpr int NBIN = 4096;                                        // cost bins: 256 binary exponents x 16 mantissa steps
constexpr int FLAG_STALLED = 1, FLAG_BAD_INPUT = 2;
constexpr int M_ERR = 0, M_F = 1, M_ROUND = 2, M_STOP = 3, M_FLAGS = 4, M_TAU = 5, M_W = 6, M_READ = 8, M_WORDS = 16;   // the host reads M_READ
constexpr uint64_t INVALID = ~0ull;

struct Quad { double a00, a01, a02, a11, a12, a22, b0, b1, b2, c; };

__device__ __forceinline__ Quad load_quad(const double* __restrict__ Q, int v) {
    const double* q = Q + 10 * (size_t)v;
    return Quad{q[0], q[1], q[2], q[3], q[4], q[5], q[6], q[7], q[8], q[9]};
}
__device__ __forceinline__ void store_quad(double* __restrict__ Q, int v, const Quad& k) {
    double* q = Q + 10 * (size_t)v;
    q[0] = k.a00; q[1] = k.a01; q[2] = k.a02; q[3] = k.a11; q[4] = k.a12; q[5] = k.a22; q[6] = k.b0; q[7] = k.b1; q[8] = k.b2; q[9] = k.c;
}
__device__ __forceinline__ Quad add_quad(const Quad& p, const Quad& q) {
    return Quad{p.a00 + q.a00, p.a01 + q.a01, p.a02 + q.a02, p.a11 + q.a11, p.a12 + q.a12, p.a22 + q.a22, p.b0 + q.b0, p.b1 + q.b1,
                p.b2 + q.b2, p.c + q.c};
}
// x^T A x + 2 b . x + c
__device__ __forceinline__ double eval_quad(const Quad& k, double x, double y, double z) {
    const double ax = (k.a00 * x + k.a01 * y) + k.a02 * z, ay = (k.a01 * x + k.a11 * y) + k.a12 * z, az = (k.a02 * x + k.a12 * y) + k.a22 * z;
    return (((x * ax + y * ay) + z * az) + 2.0 * ((k.b0 * x + k.b1 * y) + k.b2 * z)) + k.c;
}

// the two other corners of face g, in the face's cyclic order after u
__device__ __forceinline__ void ring(const int* __restrict__ face, int g, int u, int& n1, int& n2) {
    const int p = face[3 * (size_t)g], q = face[3 * (size_t)g + 1], r = face[3 * (size_t)g + 2];
    n1 = p == u ? q : (q == u ? r : p);
    n2 = p == u ? r : (q == u ? p : q);
}

// ---- input check + initial state ---------------------------------------------------------------------------------------------------
__global__ void k_sm_edge_keys(const int64_t* __restrict__ faces, int F, int V, uint64_t* __restrict__ keys, int* __restrict__ vals,
                               int* __restrict__ face32, int* __restrict__ misc) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= 3 * F) return;
    const int f = i / 3, c = i - 3 * f;
    int64_t a = faces[i], b = faces[3 * (size_t)f + (c == 2 ? 0 : c + 1)];
    if (!(index_ok(a, V) && index_ok(b, V)) || a == b) {
        atomicOr(&misc[M_ERR], FLAG_BAD_INPUT);
        a = 0; b = 0;
    }
    keys[i] = pair_key(a, b, V);
    vals[i] = i;
    face32[i] = (int)a;
}

__device__ __forceinline__ int lower_bound(const uint64_t* __restrict__ keys, int n, uint64_t key) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = lo + (hi - lo) / 2;
        if (keys[mid] < key) lo = mid + 1; else hi = mid;
    }
    return lo;
}

__global__ void k_sm_check(const uint64_t* __restrict__ keys, int N, int V, int* __restrict__ misc) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    const uint64_t key = keys[i];
    const uint64_t rev = pair_key(pair_second(key, V), pair_first(key, V), V);
    bool bad = i > 0 && keys[i - 1] == key;
    const int j = lower_bound(keys, N, rev);
    bad = bad || j >= N || keys[j] != rev;
    if (bad) atomicOr(&misc[M_ERR], FLAG_BAD_INPUT);
}

__global__ void k_sm_init(const float* __restrict__ vertices, const float* __restrict__ colors, int V, int F, float* __restrict__ P,
                          float* __restrict__ C, int* __restrict__ remap, int* __restrict__ misc) {
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v == 0) misc[M_F] = F;
    if (v >= V) return;
    remap[v] = v;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        P[3 * (size_t)v + k] = vertices[3 * (size_t)v + k];
        if (colors) C[3 * (size_t)v + k] = colors[3 * (size_t)v + k];
    }
}

// the sorted directed edges (v, *) are one run per vertex, ordered by the neighbour: a summation order that no launch can change
__global__ void k_sm_quadrics(const uint64_t* __restrict__ keys, const int* __restrict__ vals, int N, int V, const int* __restrict__ face,
                              const float* __restrict__ P, double* __restrict__ Q) {
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= V) return;
    const uint64_t end = pair_key(v + 1, 0, V);
    Quad k{0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (int i = lower_bound(keys, N, pair_key(v, 0, V)); i < N && keys[i] < end; ++i) {
        const int g = vals[i] / 3;
        const int a = face[3 * (size_t)g], b = face[3 * (size_t)g + 1], c = face[3 * (size_t)g + 2];
        const double ax = P[3 * (size_t)a], ay = P[3 * (size_t)a + 1], az = P[3 * (size_t)a + 2];
        const double ux = (double)P[3 * (size_t)b] - ax, uy = (double)P[3 * (size_t)b + 1] - ay, uz = (double)P[3 * (size_t)b + 2] - az;
        const double wx = (double)P[3 * (size_t)c] - ax, wy = (double)P[3 * (size_t)c + 1] - ay, wz = (double)P[3 * (size_t)c + 2] - az;
        const double cx = uy * wz - uz * wy, cy = uz * wx - ux * wz, cz = ux * wy - uy * wx;
        const double len = sqrt((cx * cx + cy * cy) + cz * cz);
        if (!(len > 0.0)) continue;                                 // a face without area has no plane
        const double nx = cx / len, ny = cy / len, nz = cz / len, d = -((nx * ax + ny * ay) + nz * az), w = 0.5 * len;
        k.a00 += w * nx * nx; k.a01 += w * nx * ny; k.a02 += w * nx * nz; k.a11 += w * ny * ny; k.a12 += w * ny * nz; k.a22 += w * nz * nz;
        k.b0 += w * nx * d; k.b1 += w * ny * d; k.b2 += w * nz * d; k.c += w * d * d;
    }
    store_quad(Q, v, k);
}

// ---- one round -----------------------------------------------------------------------------------------------------------------------
__global__ void k_sm_count(const int* __restrict__ face, int V, int* __restrict__ deg, unsigned long long* __restrict__ claim,
                           const int* __restrict__ misc) {
    if (misc[M_STOP]) return;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < V) claim[i] = INVALID;
    if (i < 3 * misc[M_F]) atomicAdd(&deg[face[i]], 1);
}

// (deg counts back down to zero: ready for the next round)
__global__ void k_sm_fill(const int* __restrict__ face, int* __restrict__ deg, const int* __restrict__ rowptr, int* __restrict__ adj,
                          const int* __restrict__ misc) {
    if (misc[M_STOP]) return;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= 3 * misc[M_F]) return;
    const int v = face[i];
    adj[rowptr[v] + atomicSub(&deg[v], 1) - 1] = i / 3;
}

__device__ __forceinline__ int cost_bin(uint64_t bits) {
    const int e16 = (int)(bits >> 48), lo = (1023 - 200) << 4;      // sign 0, 11 exponent bits, 4 mantissa bits; from 2^-200 up
    return min(max(e16 - lo, 0), NBIN - 1);
}

// every face of star(a) that does not hold b: positive area after a moves to x, and the normal turns by less than acos(0.2)
__device__ __forceinline__ bool star_keeps_shape(const int* __restrict__ face, const int* __restrict__ adj, int r0, int r1, int a, int b,
                                                 const float* __restrict__ P, double ox, double oy, double oz, double x, double y, double z) {
    bool ok = true;
    for (int r = r0; r < r1; ++r) {
        int n1, n2;
        ring(face, adj[r], a, n1, n2);
        if (n1 == b || n2 == b) continue;
        const double px = P[3 * (size_t)n1], py = P[3 * (size_t)n1 + 1], pz = P[3 * (size_t)n1 + 2];
        const double qx = P[3 * (size_t)n2], qy = P[3 * (size_t)n2 + 1], qz = P[3 * (size_t)n2 + 2];
        const double ax = px - ox, ay = py - oy, az = pz - oz, bx = qx - ox, by = qy - oy, bz = qz - oz;
        const double mx = ay * bz - az * by, my = az * bx - ax * bz, mz = ax * by - ay * bx;              // old normal * 2 area
        const double cx = px - x, cy = py - y, cz = pz - z, dx = qx - x, dy = qy - y, dz = qz - z;
        const double nx = cy * dz - cz * dy, ny = cz * dx - cx * dz, nz = cx * dy - cy * dx;              // new
        const double dot = (mx * nx + my * ny) + mz * nz, l0 = (mx * mx + my * my) + mz * mz, l1 = (nx * nx + ny * ny) + nz * nz;
        ok = ok && l1 > 0.0 && dot > 0.0 && dot * dot > 0.04 * (l0 * l1);
    }
    return ok;
}

// cost bits (order = order of the non-negative doubles) of edge slot e, INVALID for a slot that holds no edge or an edge that must stay
__device__ __forceinline__ uint64_t edge_cost(const int* __restrict__ face, int e, const int* __restrict__ rowptr, const int* __restrict__ adj,
                                              const float* __restrict__ P, const double* __restrict__ Q, float4* __restrict__ xs) {
    const int g = e / 3, c = e - 3 * g;
    const int u = face[e], v = face[3 * (size_t)g + (c == 2 ? 0 : c + 1)];
    if (u >= v) return INVALID;
    const int u0 = rowptr[u], u1 = rowptr[u + 1], v0 = rowptr[v], v1 = rowptr[v + 1];
    // link condition: exactly two common neighbours; and at least three vertices round the pair
    int common = 0;
    for (int r = u0; r < u1; ++r) {
        int n1, n2;
        ring(face, adj[r], u, n1, n2);
        if (n1 == v) continue;
        for (int t = v0; t < v1; ++t) {
            int m1, m2;
            ring(face, adj[t], v, m1, m2);
            common += m1 == n1 ? 1 : 0;
        }
    }
    if (common != 2 || (u1 - u0) + (v1 - v0) - 2 - common < 3) return INVALID;
    const Quad k = add_quad(load_quad(Q, u), load_quad(Q, v));
    const double ux = P[3 * (size_t)u], uy = P[3 * (size_t)u + 1], uz = P[3 * (size_t)u + 2];
    const double vx = P[3 * (size_t)v], vy = P[3 * (size_t)v + 1], vz = P[3 * (size_t)v + 2];
    const double mx = 0.5 * (ux + vx), my = 0.5 * (uy + vy), mz = 0.5 * (uz + vz);
    const double len2 = ((ux - vx) * (ux - vx) + (uy - vy) * (uy - vy)) + (uz - vz) * (uz - vz);
    // minimiser of the quadric: A x = -b by cofactors
    const double c00 = k.a11 * k.a22 - k.a12 * k.a12, c01 = k.a02 * k.a12 - k.a01 * k.a22, c02 = k.a01 * k.a12 - k.a02 * k.a11;
    const double c11 = k.a00 * k.a22 - k.a02 * k.a02, c12 = k.a01 * k.a02 - k.a00 * k.a12, c22 = k.a00 * k.a11 - k.a01 * k.a01;
    const double det = (k.a00 * c00 + k.a01 * c01) + k.a02 * c02, tr = ((k.a00 + k.a11) + k.a22) / 3.0;
    double x = ux, y = uy, z = uz;
    bool solved = false;
    if (det > 1e-9 * ((tr * tr) * tr)) {
        x = -((c00 * k.b0 + c01 * k.b1) + c02 * k.b2) / det;
        y = -((c01 * k.b0 + c11 * k.b1) + c12 * k.b2) / det;
        z = -((c02 * k.b0 + c12 * k.b1) + c22 * k.b2) / det;
        const double d2 = ((x - mx) * (x - mx) + (y - my) * (y - my)) + (z - mz) * (z - mz);
        solved = d2 <= 4.0 * len2;                                  // (false for NaN as well)
    }
    if (!solved) {                                                  // the cheapest of u, v, midpoint; u, then v on a tie
        const double cu = eval_quad(k, ux, uy, uz), cv = eval_quad(k, vx, vy, vz), cm = eval_quad(k, mx, my, mz);
        x = ux; y = uy; z = uz;
        double best = cu;
        if (cv < best) { best = cv; x = vx; y = vy; z = vz; }
        if (cm < best) { x = mx; y = my; z = mz; }
    }
    const float xf = (float)x, yf = (float)y, zf = (float)z;
    x = xf; y = yf; z = zf;
    const double cost = fmax(0.0, eval_quad(k, x, y, z));
    if (!(cost <= 1.7e308)) return INVALID;                         // NaN or infinity
    if (!star_keeps_shape(face, adj, u0, u1, u, v, P, ux, uy, uz, x, y, z)) return INVALID;
    if (!star_keeps_shape(face, adj, v0, v1, v, u, P, vx, vy, vz, x, y, z)) return INVALID;
    const double du = ((x - ux) * (x - ux) + (y - uy) * (y - uy)) + (z - uz) * (z - uz);
    const double dv = ((x - vx) * (x - vx) + (y - vy) * (y - vy)) + (z - vz) * (z - vz);
    xs[e] = make_float4(xf, yf, zf, dv < du ? 1.0f : 0.0f);         // .w: the colour comes from v
    return (uint64_t)__double_as_longlong(cost);
}

__global__ __launch_bounds__(TB) void k_sm_cost(const int* __restrict__ face, const int* __restrict__ rowptr, const int* __restrict__ adj,
                                                const float* __restrict__ P, const double* __restrict__ Q, unsigned long long* __restrict__ cost,
                                                float4* __restrict__ xs, int* __restrict__ hist, const int* __restrict__ misc) {
    __shared__ int h[NBIN];
    if (misc[M_STOP]) return;
    for (int b = threadIdx.x; b < NBIN; b += TB) h[b] = 0;
    __syncthreads();
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e < 3 * misc[M_F]) {
        const uint64_t bits = edge_cost(face, e, rowptr, adj, P, Q, xs);
        cost[e] = bits;
        if (bits != INVALID) atomicAdd(&h[cost_bin(bits)], 1);
    }
    __syncthreads();
    for (int b = threadIdx.x; b < NBIN; b += TB)
        if (h[b]) atomicAdd(&hist[b], h[b]);
}

// the first bin at which the running count reaches need; the histogram is left zeroed for the next round
__global__ __launch_bounds__(1024) void k_sm_tau(int* __restrict__ hist, int target, int* __restrict__ misc) {
    __shared__ int part[1024];
    __shared__ int tau;
    if (misc[M_STOP]) return;
    const int t = threadIdx.x, need = (misc[M_F] - target) / 2;
    constexpr int PER = NBIN / 1024;
    const int h0 = hist[PER * t], h1 = hist[PER * t + 1], h2 = hist[PER * t + 2], h3 = hist[PER * t + 3];
    static_assert(PER == 4, "four bins per thread");
    hist[PER * t] = 0; hist[PER * t + 1] = 0; hist[PER * t + 2] = 0; hist[PER * t + 3] = 0;
    const int s = (h0 + h1) + (h2 + h3);
    part[t] = s;
    if (t == 0) tau = NBIN - 1;
    __syncthreads();
    for (int off = 1; off < 1024; off <<= 1) {
        const int add = t >= off ? part[t - off] : 0;
        __syncthreads();
        part[t] += add;
        __syncthreads();
    }
    const int before = part[t] - s;
    if (before < need && before + s >= need) {
        int b = PER * t, run = before + h0;
        if (run < need) { ++b; run += h1; }
        if (run < need) { ++b; run += h2; }
        if (run < need) ++b;
        tau = b;
    }
    __syncthreads();
    if (t == 0) misc[M_TAU] = tau;
}

__device__ __forceinline__ unsigned long long edge_key(int u, int v, int round) {
    uint64_t z = (((uint64_t)(uint32_t)u << 32) | (uint64_t)(uint32_t)v) + 0x9E3779B97F4A7C15ull * (uint64_t)(round + 1);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z ^= z >> 31;
    return ((z >> (2 * ID_BITS)) << (2 * ID_BITS)) | ((uint64_t)u << ID_BITS) | (uint64_t)v;
}

// CLAIM: atomicMin of the key onto u, v and every neighbour of either; else: do all those words hold the key?
template <bool CLAIM>
__device__ __forceinline__ bool walk_claims(const int* __restrict__ face, const int* __restrict__ rowptr, const int* __restrict__ adj, int u, int v,
                                            unsigned long long key, unsigned long long* __restrict__ claim) {
    bool all = true;
    if (CLAIM) { atomicMin(&claim[u], key); atomicMin(&claim[v], key); }
    else all = claim[u] == key && claim[v] == key;
    for (int side = 0; side < 2; ++side) {
        const int a = side ? v : u;
        for (int r = rowptr[a]; r < rowptr[a + 1]; ++r) {
            int n1, n2;
            ring(face, adj[r], a, n1, n2);
            if (CLAIM) atomicMin(&claim[n1], key);
            else all = all && claim[n1] == key;
        }
    }
    return all;
}

template <bool CLAIM>
__global__ void k_sm_claim(const int* __restrict__ face, const int* __restrict__ rowptr, const int* __restrict__ adj,
                           const unsigned long long* __restrict__ cost, unsigned long long* __restrict__ claim, int* __restrict__ wflag, int n_host,
                           const int* __restrict__ misc) {
    if (misc[M_STOP]) return;
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n_host) return;
    bool win = false;
    if (e < 3 * misc[M_F]) {
        const uint64_t bits = cost[e];
        if (bits != INVALID && cost_bin(bits) <= misc[M_TAU]) {
            const int g = e / 3, c = e - 3 * g;
            const int u = face[e], v = face[3 * (size_t)g + (c == 2 ? 0 : c + 1)];
            win = walk_claims<CLAIM>(face, rowptr, adj, u, v, edge_key(u, v, misc[M_ROUND]), claim);
        }
    }
    if (!CLAIM) wflag[e] = win ? 1 : 0;                              // (zero past the current faces too: the scan runs over n_host)
}

__global__ void k_sm_winners(const int* __restrict__ face, const unsigned long long* __restrict__ cost, const int* __restrict__ wflag,
                             const int* __restrict__ wexcl, int* __restrict__ wslot, unsigned long long* __restrict__ wcost,
                             unsigned long long* __restrict__ wuv, int* __restrict__ misc) {
    if (misc[M_STOP]) return;
    const int e = blockIdx.x * blockDim.x + threadIdx.x, n = 3 * misc[M_F];
    if (e >= n) return;
    if (e == n - 1) misc[M_W] = wexcl[e] + wflag[e];
    if (!wflag[e]) return;
    const int g = e / 3, c = e - 3 * g, i = wexcl[e];
    wslot[i] = e;
    wcost[i] = cost[e];
    wuv[i] = ((uint64_t)face[e] << ID_BITS) | (uint64_t)face[3 * (size_t)g + (c == 2 ? 0 : c + 1)];
}

// winner i collapses v into u -- unless there are more winners than needed and `need` of them are cheaper by (cost, u, v)
__global__ void k_sm_apply(const int* __restrict__ wslot, const unsigned long long* __restrict__ wcost, const unsigned long long* __restrict__ wuv,
                           const float4* __restrict__ xs, int target, float* __restrict__ P, double* __restrict__ Q, float* __restrict__ C,
                           int* __restrict__ remap, const int* __restrict__ misc) {
    if (misc[M_STOP]) return;
    const int i = blockIdx.x * blockDim.x + threadIdx.x, W = misc[M_W], need = (misc[M_F] - target) / 2;
    if (i >= W) return;
    const unsigned long long uv = wuv[i];
    if (W > need) {
        const unsigned long long ci = wcost[i];
        int rank = 0;
        for (int j = 0; j < W; ++j) {
            const unsigned long long cj = wcost[j];
            rank += (cj < ci || (cj == ci && wuv[j] < uv)) ? 1 : 0;
        }
        if (rank >= need) return;
    }
    const int u = (int)(uv >> ID_BITS), v = (int)(uv & (unsigned long long)(MAX_V - 1));
    const float4 x = xs[wslot[i]];
    P[3 * (size_t)u] = x.x; P[3 * (size_t)u + 1] = x.y; P[3 * (size_t)u + 2] = x.z;
    store_quad(Q, u, add_quad(load_quad(Q, u), load_quad(Q, v)));
    remap[v] = u;
    if (C && x.w != 0.0f) {
#pragma unroll
        for (int k = 0; k < 3; ++k) C[3 * (size_t)u + k] = C[3 * (size_t)v + k];
    }
}

__global__ void k_sm_rewrite(int* __restrict__ face, const int* __restrict__ remap, int* __restrict__ kflag, int n_host,
                             const int* __restrict__ misc) {
    if (misc[M_STOP]) return;
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= n_host) return;
    int keep = 0;
    if (f < misc[M_F]) {
        const int a = remap[face[3 * (size_t)f]], b = remap[face[3 * (size_t)f + 1]], c = remap[face[3 * (size_t)f + 2]];
        face[3 * (size_t)f] = a; face[3 * (size_t)f + 1] = b; face[3 * (size_t)f + 2] = c;
        keep = (a != b && b != c && a != c) ? 1 : 0;
    }
    kflag[f] = keep;
}

__global__ void k_sm_compact(const int* __restrict__ src, int* __restrict__ dst, const int* __restrict__ kflag, const int* __restrict__ kexcl,
                             const int* __restrict__ misc) {
    if (misc[M_STOP]) return;
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= misc[M_F] || !kflag[f]) return;
    const size_t d = 3 * (size_t)kexcl[f], s = 3 * (size_t)f;
    dst[d] = src[s]; dst[d + 1] = src[s + 1]; dst[d + 2] = src[s + 2];
}

__global__ void k_sm_round_end(const int* __restrict__ kflag, const int* __restrict__ kexcl, int target, int* __restrict__ misc) {
    if (misc[M_STOP]) return;
    const int F = misc[M_F], Fn = kexcl[F - 1] + kflag[F - 1];
    misc[M_F] = Fn;
    misc[M_ROUND] += 1;
    if (misc[M_W] == 0) { misc[M_FLAGS] |= FLAG_STALLED; misc[M_STOP] = 1; }
    else if (Fn <= target + 1) misc[M_STOP] = 1;
}

// ---- output ----------------------------------------------------------------------------------------------------------------------------
__global__ void k_sm_mark(const int* __restrict__ face, int n, int* __restrict__ vflag) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) vflag[face[i]] = 1;
}

__global__ void k_sm_out_vertices(const float* __restrict__ P, const float* __restrict__ C, const int* __restrict__ vflag,
                                  const int* __restrict__ vexcl, int V, float* __restrict__ out_v, float* __restrict__ out_c,
                                  int32_t* __restrict__ counts) {
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= V) return;
    if (v == V - 1) counts[0] = vexcl[v] + vflag[v];
    if (!vflag[v]) return;
    const size_t d = 3 * (size_t)vexcl[v], s = 3 * (size_t)v;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        out_v[d + k] = P[s + k];
        if (out_c) out_c[d + k] = C[s + k];
    }
}

__global__ void k_sm_out_faces(const int* __restrict__ face, int n, const int* __restrict__ vexcl, int64_t* __restrict__ out_f) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out_f[i] = (int64_t)vexcl[face[i]];
}

__global__ void k_sm_counts(int32_t* __restrict__ counts, int first, int v, int f, int rounds, int flags) {
    if (first <= 0) counts[0] = v;
    counts[1] = f; counts[2] = rounds; counts[3] = flags;
}

struct SimWs {
    float *P, *C;
    double* Q;
    int *face[2], *remap, *deg, *rowptr, *adj, *hist, *wflag, *wexcl, *wslot, *kflag, *kexcl, *tsum, *toff, *misc;
    unsigned long long *cost, *claim, *wcost, *wuv;
    float4* xs;
    SortBufs sb;
};

static size_t carve_sim(SimWs& w, void* base, int V, int F) {
    const size_t nv = (size_t)V, nf = (size_t)F, n = 3 * nf;
    Carve c{static_cast<char*>(base), 0};
    w.P = c.take<float>(3 * nv); w.C = c.take<float>(3 * nv); w.Q = c.take<double>(10 * nv);
    w.face[0] = c.take<int>(n); w.face[1] = c.take<int>(n); w.remap = c.take<int>(nv);
    w.deg = c.take<int>(nv + 1); w.rowptr = c.take<int>(nv + 1); w.adj = c.take<int>(n);
    w.cost = c.take<unsigned long long>(n); w.xs = c.take<float4>(n); w.claim = c.take<unsigned long long>(nv); w.hist = c.take<int>(NBIN);
    w.wflag = c.take<int>(n); w.wexcl = c.take<int>(n);
    w.wslot = c.take<int>(nf); w.wcost = c.take<unsigned long long>(nf); w.wuv = c.take<unsigned long long>(nf);   // (winners' stars are disjoint: < F / 5)
    w.kflag = c.take<int>(nf); w.kexcl = c.take<int>(nf);
    const size_t tiles = scan_tiles(n > nv + 1 ? n : nv + 1);
    w.tsum = c.take<int>(tiles); w.toff = c.take<int>(tiles); w.misc = c.take<int>(M_WORDS);
    carve_sort(c, w.sb, n);
    return c.off + 256;
}

static bool sizes_ok(int V, int F) { return V >= 4 && F >= 4 && V <= MAX_V && F <= MAX_F; }

}  // namespace

extern "C" size_t pdhip_simplify_mesh_workspace_bytes(int Vn, int F) {
    if (!sizes_ok(Vn, F)) return 0;
    SimWs w;
    return carve_sim(w, nullptr, Vn, F);
}

extern "C" int pdhip_simplify_mesh(const float* vertices, int Vn, const int64_t* faces, int F, const float* vertex_colors, int target_faces,
                                   float* out_vertices, int64_t* out_faces, float* out_colors, int32_t* counts, void* ws, void* stream) {
    PD_REQUIRE(vertices && faces && out_vertices && out_faces && counts && ws, "pdhip_simplify_mesh: null pointer");
    PD_REQUIRE((vertex_colors != nullptr) == (out_colors != nullptr), "pdhip_simplify_mesh: vertex_colors and out_colors go together");
    PD_REQUIRE(Vn >= 4 && F >= 4, "pdhip_simplify_mesh: a closed mesh has at least 4 vertices and 4 faces (Vn=%d F=%d)", Vn, F);
    PD_REQUIRE(Vn <= MAX_V && F <= MAX_F, "pdhip_simplify_mesh: Vn=%d F=%d exceed the key widths (Vn <= 2^22, F <= 2^23)", Vn, F);
    PD_REQUIRE(target_faces >= 4, "pdhip_simplify_mesh: target_faces=%d, a closed mesh has at least 4 faces", target_faces);
    hipStream_t s = as_stream(stream);
    const int V = Vn, N = 3 * F;
    if (target_faces >= F) {                                        // nothing to do: the mesh goes through bit for bit
        PD_HIP(hipMemcpyAsync(out_vertices, vertices, 3 * (size_t)V * sizeof(float), hipMemcpyDeviceToDevice, s));
        PD_HIP(hipMemcpyAsync(out_faces, faces, 3 * (size_t)F * sizeof(int64_t), hipMemcpyDeviceToDevice, s));
        if (out_colors) PD_HIP(hipMemcpyAsync(out_colors, vertex_colors, 3 * (size_t)V * sizeof(float), hipMemcpyDeviceToDevice, s));
        k_sm_counts<<<1, 1, 0, s>>>(counts, 0, V, F, 0, 0);
        PD_LAUNCH_CHECK();
        return PDHIP_OK;
    }
    SimWs w;
    carve_sim(w, ws, V, F);
    int h[M_READ];
    // ---- input check: one sort of the directed edges
    PD_HIP(hipMemsetAsync(w.misc, 0, M_WORDS * sizeof(int), s));
    PD_HIP(hipMemsetAsync(w.deg, 0, ((size_t)V + 1) * sizeof(int), s));
    PD_HIP(hipMemsetAsync(w.hist, 0, NBIN * sizeof(int), s));
    k_sm_edge_keys<<<cdiv(N, TB), TB, 0, s>>>(faces, F, V, w.sb.k[0], w.sb.v[0], w.face[0], w.misc);
    const int cur = radix_sort(w.sb, N, bits_for((unsigned long long)V * (unsigned long long)V - 1ull), s);
    k_sm_check<<<cdiv(N, TB), TB, 0, s>>>(w.sb.k[cur], N, V, w.misc);
    k_sm_init<<<cdiv(V, TB), TB, 0, s>>>(vertices, vertex_colors, V, F, w.P, w.C, w.remap, w.misc);
    k_sm_quadrics<<<cdiv(V, TB), TB, 0, s>>>(w.sb.k[cur], w.sb.v[cur], N, V, w.face[0], w.P, w.Q);
    PD_LAUNCH_CHECK();
    int rc = read_words(w.misc, h, M_READ, s);
    if (rc != PDHIP_OK) return rc;
    if (h[M_ERR]) {
        k_sm_counts<<<1, 1, 0, s>>>(counts, 0, 0, 0, 0, FLAG_BAD_INPUT);
        PD_LAUNCH_CHECK();
        PD_REQUIRE(false, "pdhip_simplify_mesh: the input is not a closed, consistently oriented 2-manifold with indices in [0, Vn=%d) "
                          "(every directed edge once, its reverse once, three different corners per face)", V);
    }
    // ---- rounds; the status words are read once per BATCH
    float* C = vertex_colors ? w.C : nullptr;
    int Fh = F, r = 0;
    bool stop = false;
    while (!stop && r < MAX_ROUNDS) {
        const int n = 3 * Fh, gn = cdiv(n, TB), gf = cdiv(Fh, TB);
        for (int k = 0; k < BATCH && r < MAX_ROUNDS; ++k, ++r) {
            int* fc = w.face[r & 1];
            k_sm_count<<<cdiv(n > V ? n : V, TB), TB, 0, s>>>(fc, V, w.deg, w.claim, w.misc);
            scan_exclusive(w.deg, w.rowptr, (long long)V + 1, w.tsum, w.toff, s);
            k_sm_fill<<<gn, TB, 0, s>>>(fc, w.deg, w.rowptr, w.adj, w.misc);
            k_sm_cost<<<gn, TB, 0, s>>>(fc, w.rowptr, w.adj, w.P, w.Q, w.cost, w.xs, w.hist, w.misc);
            k_sm_tau<<<1, 1024, 0, s>>>(w.hist, target_faces, w.misc);
            k_sm_claim<true><<<gn, TB, 0, s>>>(fc, w.rowptr, w.adj, w.cost, w.claim, w.wflag, n, w.misc);
            k_sm_claim<false><<<gn, TB, 0, s>>>(fc, w.rowptr, w.adj, w.cost, w.claim, w.wflag, n, w.misc);
            scan_exclusive(w.wflag, w.wexcl, n, w.tsum, w.toff, s);
            k_sm_winners<<<gn, TB, 0, s>>>(fc, w.cost, w.wflag, w.wexcl, w.wslot, w.wcost, w.wuv, w.misc);
            k_sm_apply<<<gf, TB, 0, s>>>(w.wslot, w.wcost, w.wuv, w.xs, target_faces, w.P, w.Q, C, w.remap, w.misc);
            k_sm_rewrite<<<gf, TB, 0, s>>>(fc, w.remap, w.kflag, Fh, w.misc);
            scan_exclusive(w.kflag, w.kexcl, Fh, w.tsum, w.toff, s);
            k_sm_compact<<<gf, TB, 0, s>>>(fc, w.face[(r + 1) & 1], w.kflag, w.kexcl, w.misc);
            k_sm_round_end<<<1, 1, 0, s>>>(w.kflag, w.kexcl, target_faces, w.misc);
        }
        PD_LAUNCH_CHECK();
        rc = read_words(w.misc, h, M_READ, s);
        if (rc != PDHIP_OK) return rc;
        stop = h[M_STOP] != 0;
        Fh = h[M_F];
    }
    PD_REQUIRE(stop, "pdhip_simplify_mesh: %d faces after %d rounds, target %d: more than %d rounds", Fh, r, target_faces, MAX_ROUNDS);
    // ---- output: referenced vertices in input order (deg / rowptr serve as flag / offset; deg is zero after every round)
    const int rounds = h[M_ROUND], No = 3 * Fh;
    const int* ff = w.face[rounds & 1];
    k_sm_mark<<<cdiv(No, TB), TB, 0, s>>>(ff, No, w.deg);
    scan_exclusive(w.deg, w.rowptr, V, w.tsum, w.toff, s);
    k_sm_out_vertices<<<cdiv(V, TB), TB, 0, s>>>(w.P, C, w.deg, w.rowptr, V, out_vertices, out_colors, counts);
    k_sm_out_faces<<<cdiv(No, TB), TB, 0, s>>>(ff, No, w.rowptr, out_faces);
    k_sm_counts<<<1, 1, 0, s>>>(counts, 1, 0, Fh, rounds, h[M_FLAGS]);
    PD_LAUNCH_CHECK();
    return PDHIP_OK;
}
