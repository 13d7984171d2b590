// Taubin lambda | mu smoothing of an indexed triangle mesh with uniform ("umbrella") weights, and the boundary vertices of a mesh
// (include/pdhip.h has the contracts; DESIGN.md section 6, "Smoothing").  No reference counterpart: the reference lets POCO absorb the
// cloud's noise; this is MeshLab's "Taubin Smooth" over the neighbour CSR of pdhip_neighbour_csr (unique neighbours, ascending rows).
//
// Smoothing: the state is f64, [Vn, 4] (x y z and a pad word, so that a neighbour is one aligned 32-byte read), ping-pong between two
// buffers of the caller.  One pass, factor s: x'[v] = x[v] + s * (m - x[v]), m = (sum of the row's vertices, added one by one in row order)
// / |row|: a sequential sum, one division, one subtraction, one multiplication, one addition, no FMA (the geometry rule of the Makefile
// compiles with -ffp-contract=off).  A held vertex and a vertex with an empty row keep their position.  Every pass reads the old state
// only (Jacobi), so the result depends on neither the threads' order nor anything but the rows.  The first pass reads the f32 input, the
// last one rounds to the f32 output: steps * (1 or 2) launches of k_msm_pass behind one launch of k_msm_check.
//   k_msm_check   one thread per vertex: rowptr[0] == 0 and monotone up to rowptr[Vn], every colidx of the row in [0, Vn), the vertex
//                 finite when its row is not empty; ORs the cause into the check word (counts[3]) and counts moved / held / isolated
//   k_msm_pass    one thread per vertex, the row walked by a plain loop (a row of any length); writes nothing when the check word is set
// Boundary: pair_faces[pos] = the faces on the ordered pair (row a, colidx[pos] = b), found by a binary search in the ascending row a
// and an integer atomicAdd; a vertex is a boundary vertex when one of its pairs lies on exactly one face.  No sort, integer atomics only.
#include "mesh_common.h"

namespace pdhip {
namespace {

constexpr int TB = 256;
constexpr int MAX_STEPS = 10000;
enum { C_MOVED = 0, C_HELD, C_ISOLATED, C_CHECK };                 // pdhip_smooth_mesh's counts
enum { B_VERTICES = 0, B_EDGES, B_NONMANIFOLD, B_CHECK };          // pdhip_mesh_boundary_vertices' counts
enum { ERR_ROWPTR = 1, ERR_COLIDX = 2, ERR_NONFINITE = 4, ERR_FACE = 8, ERR_PAIR = 16 };

// row v is [rowptr[v], rowptr[v + 1]) inside [0, nnz = rowptr[Vn]): false sets nothing -- the caller flags it.  Only a row that passes is
// walked, so no index outside colidx[0, nnz) is ever formed
__device__ __forceinline__ bool row_ok(const int32_t* __restrict__ rowptr, int v, int nnz, int& r0, int& r1) {
    r0 = rowptr[v]; r1 = rowptr[v + 1];
    return nnz >= 0 && r0 >= 0 && r0 <= r1 && r1 <= nnz && (v != 0 || r0 == 0);
}

// ---- smoothing
__global__ __launch_bounds__(TB) void k_msm_check(const float* __restrict__ P, int Vn, const int32_t* __restrict__ rowptr,
                                                  const int32_t* __restrict__ colidx, const uint8_t* __restrict__ held, int32_t* __restrict__ counts) {
    const int v = blockIdx.x * blockDim.x + threadIdx.x, lane = threadIdx.x & 63;
    const bool in = v < Vn;
    int err = 0, r0 = 0, r1 = 0;
    if (in) {
        if (!row_ok(rowptr, v, rowptr[Vn], r0, r1)) { err = ERR_ROWPTR; r1 = r0; }
        for (int k = r0; k < r1; ++k) {
            const int j = colidx[k];
            if (!index_ok(j, Vn)) err |= ERR_COLIDX;
        }
        if (r1 > r0 && !finite3(P[3 * (size_t)v], P[3 * (size_t)v + 1], P[3 * (size_t)v + 2])) err |= ERR_NONFINITE;
    }
    if (err) atomicOr(&counts[C_CHECK], err);
    const bool isolated = in && r1 == r0, hold = in && !isolated && held && held[v] != 0;
    wave_count(&counts[C_ISOLATED], isolated, lane);
    wave_count(&counts[C_HELD], hold, lane);
    wave_count(&counts[C_MOVED], in && !isolated && !hold, lane);
}

template <bool F32>
__device__ __forceinline__ void load3(const void* __restrict__ src, int v, double& x, double& y, double& z) {
    if (F32) {
        const float* p = static_cast<const float*>(src) + 3 * (size_t)v;
        x = (double)p[0]; y = (double)p[1]; z = (double)p[2];
    } else {
        const double4 q = static_cast<const double4*>(src)[v];
        x = q.x; y = q.y; z = q.z;
    }
}

// IN32: src is the f32 input [Vn, 3], otherwise a state [Vn, 4] f64; OUT32: dst is the f32 output, the state rounded once
template <bool IN32, bool OUT32>
__global__ __launch_bounds__(TB) void k_msm_pass(const void* __restrict__ src, void* __restrict__ dst, int Vn, const int32_t* __restrict__ rowptr,
                                                 const int32_t* __restrict__ colidx, const uint8_t* __restrict__ held, double s,
                                                 const int32_t* __restrict__ counts) {
    if (counts[C_CHECK]) return;                                   // (the rows and indices below were checked by k_msm_check)
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= Vn) return;
    double x, y, z;
    load3<IN32>(src, v, x, y, z);
    const int r0 = rowptr[v], r1 = rowptr[v + 1];
    if (r1 > r0 && !(held && held[v] != 0)) {
        double sx = 0.0, sy = 0.0, sz = 0.0;
        for (int k = r0; k < r1; ++k) {
            double nx, ny, nz;
            load3<IN32>(src, colidx[k], nx, ny, nz);
            sx = sx + nx; sy = sy + ny; sz = sz + nz;
        }
        const double n = (double)(r1 - r0);
        x = x + s * (sx / n - x);
        y = y + s * (sy / n - y);
        z = z + s * (sz / n - z);
    }
    if (OUT32) {
        float* o = static_cast<float*>(dst) + 3 * (size_t)v;
        o[0] = (float)x; o[1] = (float)y; o[2] = (float)z;
    } else {
        static_cast<double4*>(dst)[v] = make_double4(x, y, z, 0.0);
    }
}

// ---- boundary
// pair_faces[0, nnz) = 0 and the rows checked (the grid covers max(6 F, Vn) threads)
__global__ __launch_bounds__(TB) void k_msm_pair_zero(int F, int Vn, const int32_t* __restrict__ rowptr, int32_t* __restrict__ pair_faces,
                                                      int32_t* __restrict__ counts) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const int nnz = rowptr[Vn];
    int r0, r1;
    if (nnz < 0 || nnz > 6ll * F || (i < Vn && !row_ok(rowptr, (int)i, nnz, r0, r1))) { atomicOr(&counts[B_CHECK], ERR_ROWPTR); return; }
    if (i < nnz) pair_faces[i] = 0;
}

// one thread per ordered pair of a face (edge e of the face, direction d): the position of b in row a gets one more face
__global__ __launch_bounds__(TB) void k_msm_pair_count(const int64_t* __restrict__ faces, int F, int Vn, const int32_t* __restrict__ rowptr,
                                                       const int32_t* __restrict__ colidx, int32_t* __restrict__ pair_faces, int32_t* __restrict__ counts) {
    if (counts[B_CHECK]) return;
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= 6ll * F) return;
    const int f = (int)(i / 6), p = (int)(i % 6), e = p >> 1;
    int64_t a = faces[3 * (size_t)f + e], b = faces[3 * (size_t)f + (e + 1) % 3];
    if (!(index_ok(a, Vn) && index_ok(b, Vn))) { atomicOr(&counts[B_CHECK], ERR_FACE); return; }
    if (a == b) return;
    if (p & 1) { const int64_t t = a; a = b; b = t; }
    int lo = rowptr[a], hi = rowptr[a + 1];                        // (a monotone rowptr inside [0, nnz]: k_msm_pair_zero)
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        if (colidx[mid] < (int)b) lo = mid + 1; else hi = mid;
    }
    if (lo < rowptr[a + 1] && colidx[lo] == (int)b) atomicAdd(&pair_faces[lo], 1);
    else atomicOr(&counts[B_CHECK], ERR_PAIR);
}

// boundary[v] = a pair of row v lies on exactly one face; the edges are counted at their smaller end
__global__ __launch_bounds__(TB) void k_msm_boundary(int Vn, const int32_t* __restrict__ rowptr, const int32_t* __restrict__ colidx,
                                                     const int32_t* __restrict__ pair_faces, uint8_t* __restrict__ boundary, int32_t* __restrict__ counts) {
    if (counts[B_CHECK]) return;
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= Vn) return;
    int any = 0, open = 0, many = 0;
    for (int k = rowptr[v], r1 = rowptr[v + 1]; k < r1; ++k) {
        const int n = pair_faces[k], up = colidx[k] > v;
        any |= n == 1;
        open += (n == 1) & up;
        many += (n > 2) & up;
    }
    boundary[v] = (uint8_t)any;
    if (any) atomicAdd(&counts[B_VERTICES], 1);
    if (open) atomicAdd(&counts[B_EDGES], open);
    if (many) atomicAdd(&counts[B_NONMANIFOLD], many);
}

static bool aligned32(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 31u) == 0; }

template <bool IN32, bool OUT32>
static void launch_pass(const void* src, void* dst, int Vn, const int32_t* rowptr, const int32_t* colidx, const uint8_t* held, double s,
                        const int32_t* counts, hipStream_t st) {
    k_msm_pass<IN32, OUT32><<<cdiv(Vn, TB), TB, 0, st>>>(src, dst, Vn, rowptr, colidx, held, s, counts);
}

}  // namespace
}  // namespace pdhip

using namespace pdhip;

extern "C" int pdhip_mesh_boundary_vertices(const int64_t* faces, int F, int Vn, const int32_t* rowptr, const int32_t* colidx, int32_t* pair_faces,
                                            uint8_t* boundary, int32_t* counts, void* stream) {
#define MB_PTR(p) PD_REQUIRE(p, "pdhip_mesh_boundary_vertices: null pointer (" #p ")")
    MB_PTR(faces); MB_PTR(rowptr); MB_PTR(colidx); MB_PTR(pair_faces); MB_PTR(boundary); MB_PTR(counts);
#undef MB_PTR
    PD_REQUIRE(Vn >= 1 && F >= 1, "pdhip_mesh_boundary_vertices: Vn=%d F=%d: at least one vertex and one face", Vn, F);
    PD_REQUIRE(Vn <= MESH_MAX_V && F <= MESH_MAX_F, "pdhip_mesh_boundary_vertices: Vn=%d F=%d exceed the limits (Vn <= 2^26, F <= 2^23)", Vn, F);
    hipStream_t s = as_stream(stream);
    const long long pairs = 6ll * F;
    PD_HIP(hipMemsetAsync(counts, 0, 4 * sizeof(int32_t), s));
    k_msm_pair_zero<<<cdiv(pairs > Vn ? pairs : Vn, TB), TB, 0, s>>>(F, Vn, rowptr, pair_faces, counts);
    k_msm_pair_count<<<cdiv(pairs, TB), TB, 0, s>>>(faces, F, Vn, rowptr, colidx, pair_faces, counts);
    k_msm_boundary<<<cdiv(Vn, TB), TB, 0, s>>>(Vn, rowptr, colidx, pair_faces, boundary, counts);
    PD_LAUNCH_CHECK();
    int32_t h[4];
    const int rc = read_words(counts, h, 4, s);
    if (rc) return rc;
    PD_REQUIRE(!(h[B_CHECK] & ERR_ROWPTR), "pdhip_mesh_boundary_vertices: rowptr is not a CSR of these faces (rowptr[0] == 0, ascending, "
               "rowptr[Vn=%d] <= 6 F)", Vn);
    PD_REQUIRE(!(h[B_CHECK] & ERR_FACE), "pdhip_mesh_boundary_vertices: a face index outside [0, Vn=%d)", Vn);
    PD_REQUIRE(!(h[B_CHECK] & ERR_PAIR), "pdhip_mesh_boundary_vertices: a pair of a face is not in its row of the CSR (the CSR belongs to other "
               "faces, or its rows do not ascend)");
    return PDHIP_OK;
}

extern "C" int pdhip_smooth_mesh(const float* vertices, int Vn, const int32_t* rowptr, const int32_t* colidx, const uint8_t* held, int steps,
                                 double lambda, double mu, double* state_a, double* state_b, float* out_vertices, int32_t* counts, void* stream) {
#define SM_PTR(p) PD_REQUIRE(p, "pdhip_smooth_mesh: null pointer (" #p ")")
    SM_PTR(vertices); SM_PTR(rowptr); SM_PTR(colidx); SM_PTR(state_a); SM_PTR(state_b); SM_PTR(out_vertices); SM_PTR(counts);
#undef SM_PTR
    PD_REQUIRE(Vn >= 1 && Vn <= MESH_MAX_V, "pdhip_smooth_mesh: Vn=%d: at least one vertex, at most 2^26", Vn);
    PD_REQUIRE(steps >= 1 && steps <= MAX_STEPS, "pdhip_smooth_mesh: steps=%d: 1 .. %d", steps, MAX_STEPS);
    PD_REQUIRE(lambda > 0.0 && lambda <= 1.0, "pdhip_smooth_mesh: lambda=%g is not in (0, 1]", lambda);
    PD_REQUIRE(mu <= 0.0 && mu >= -1.7976931348623157e308, "pdhip_smooth_mesh: mu=%g: a finite number <= 0 (0: the plain Laplacian)", mu);
    PD_REQUIRE(mu == 0.0 || mu < -lambda, "pdhip_smooth_mesh: lambda=%g mu=%g is not a Taubin pair: mu < -lambda keeps the pass band "
               "1/lambda + 1/mu positive", lambda, mu);
    const double top = (1.0 - 2.0 * lambda) * (1.0 - 2.0 * mu);
    PD_REQUIRE(top >= -1.0 && top <= 1.0, "pdhip_smooth_mesh: lambda=%g mu=%g amplify the highest frequency: |(1 - 2 lambda)(1 - 2 mu)| = %g > 1",
               lambda, mu, top < 0.0 ? -top : top);
    PD_REQUIRE(aligned32(state_a) && aligned32(state_b), "pdhip_smooth_mesh: state_a and state_b hold [Vn, 4] f64 rows read 32 bytes at a time: "
               "align them to 32 bytes");
    PD_REQUIRE(state_a != state_b, "pdhip_smooth_mesh: state_a and state_b are one buffer (every pass reads one and writes the other)");
    hipStream_t s = as_stream(stream);
    PD_HIP(hipMemsetAsync(counts, 0, 4 * sizeof(int32_t), s));
    k_msm_check<<<cdiv(Vn, TB), TB, 0, s>>>(vertices, Vn, rowptr, colidx, held, counts);
    const int per = mu == 0.0 ? 1 : 2, passes = steps * per;
    for (int p = 0; p < passes; ++p) {
        const double f = (per == 2 && (p & 1)) ? mu : lambda;
        const void* src = p == 0 ? static_cast<const void*>(vertices) : ((p & 1) ? state_a : state_b);
        void* dst = p == passes - 1 ? static_cast<void*>(out_vertices) : ((p & 1) ? state_b : state_a);
        const bool in32 = p == 0, out32 = p == passes - 1;
        if (in32 && out32) launch_pass<true, true>(src, dst, Vn, rowptr, colidx, held, f, counts, s);
        else if (in32) launch_pass<true, false>(src, dst, Vn, rowptr, colidx, held, f, counts, s);
        else if (out32) launch_pass<false, true>(src, dst, Vn, rowptr, colidx, held, f, counts, s);
        else launch_pass<false, false>(src, dst, Vn, rowptr, colidx, held, f, counts, s);
    }
    PD_LAUNCH_CHECK();
    int32_t h[4];
    const int rc = read_words(counts, h, 4, s);
    if (rc) return rc;
    PD_REQUIRE(!(h[C_CHECK] & ERR_ROWPTR), "pdhip_smooth_mesh: rowptr is not monotone from rowptr[0] == 0 to rowptr[Vn=%d]; nothing was written", Vn);
    PD_REQUIRE(!(h[C_CHECK] & ERR_COLIDX), "pdhip_smooth_mesh: a colidx outside [0, Vn=%d); nothing was written", Vn);
    PD_REQUIRE(!(h[C_CHECK] & ERR_NONFINITE), "pdhip_smooth_mesh: a vertex with neighbours is not finite; nothing was written");
    return PDHIP_OK;
}
