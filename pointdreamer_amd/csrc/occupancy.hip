// Point-in-mesh test on the device (models/POCO/eval/src/utils/libmesh/inside_mesh.py: check_mesh_contains, with triangle_hash.pyx as its cull) and
// the two counts behind the volumetric IoU (eval/src/common.py: compute_iou).
//
//   pdhip_mesh_contains
//     a. k_point_box (cell_list.h): faces checked against [0, Vn), the bounding box of the REFERENCED vertices (integer atomics on order-preserving keys), the
//        finiteness of those vertices and of the points; one small read that synchronises the stream.  On the host, in f64 as numpy does:
//        scale = (R - 1) / (max - min), translate = 0.5 - scale * min.  A mesh without extent on an axis is refused (the reference divides by zero);
//     b. the POINTS are binned, not the triangles: x' = scale * x + translate (two roundings), a point outside [0, R]^3 takes the key G * G and sorts
//        behind every cell; the others are sorted (cell_list.h) by the xy cell key cx * G + cy, y fastest, of a G x G grid with G ~ sqrt(Q / 4).  The
//        points of the cells y0 .. y1 of one x column are then ONE run of the sorted array (cstart[c] = first sorted point whose key is >= c);
//     c. k_occ_tri: one group of lanes per (triangle, column slab): a wave, or 16 lanes from 32 768 faces on.  The group rescales its triangle, forms
//        the constants of check_triangles and of compute_intersection_depth once, takes the cell box of the triangle's xy extent and walks the columns
//        cx0 + slab, cx0 + slab + S, ... of that box, its lanes striding over each column's run.  A lane applies the reference's predicate to its point,
//        op by op in f64, and XORs bit 0 (depth >= pz |n2|) or bit 1 (depth < pz |n2|) into the point's parity word: integer atomics, so neither the
//        order of the faces nor the schedule shows in the result.  S, the slabs per triangle, is a function of F alone (many for a mesh of few
//        faces, whose triangles each span many columns; one from 16 384 faces on);
//     d. k_occ_finish: occ = both parities odd, and the three counts.
//   The cull is conservative, so the result equals the all-pairs evaluation bit for bit.  The predicate, evaluated in f64, accepts a point only
//   inside the triangle widened by m = 8 E R / |detA| + 1e-12 R with E = 4e-15 R^2: each of u, v, u + v, detA is a difference of two products of
//   magnitudes <= R, wrong by at most 4 * 2^-53 R^2 < E / 4, so that the barycentric coordinates u / |detA|, v / |detA| of an accepted point lie
//   within 2 E / |detA| of [0, 1] and their sum within 3 E / |detA|, and the edges are no longer than R; the second term covers the roundings of
//   y = p - t3 and of A.  The box is widened by m before it is turned into cells, with the same monotone cell function the points use.  For a
//   sliver whose |detA| is down in the rounding noise m exceeds the grid and the triangle walks every column: slow, but it ends.
//   Every loop bound is a function of (F, Q, G); a face with an index outside [0, Vn) or a non-finite vertex never reaches c.
//   pdhip_occupancy_iou
//     intersection and union of (a >= 1), (b >= 1): per-thread counts, a wave reduction, an LDS sum per workgroup, one 64-bit integer atomic per workgroup.
//
// Tried and measured (profiles/occupancy_bench.txt: 100 000 points, the whole Python call with its read-back, median of 15;
// profiles/occupancy_kernel_stats.txt: per kernel): 0.153 ms against a 9 680-face sphere and 0.186 ms against 200 000 faces, against 85 ms / 2 480 ms
// for the same predicate over all pairs in f64 torch ops.
//   * One slab per triangle (pdhip_debug_set_mesh_contains_slabs(1)) leaves the 12-face box, where every triangle spans the grid, to 12 waves of
//     Q / 64 iterations each: 0.72 ms, SLOWER than the torch evaluation (0.55 ms); with its columns dealt to 64 waves per triangle 0.150 ms.  64
//     slabs everywhere cost the 200 000-face sphere 0.72 ms (groups that mostly leave at once), hence S from F.
//   * A wave per triangle took k_occ_tri 98 us against 200 000 faces (a triangle there meets one or two columns of a handful of points: most lanes
//     idle); 16 lanes per triangle 34 us, hence the narrower group from 32 768 faces on.
//   * Atomics on one address are served one after the other.  k_occ_finish with one global atomicAdd per wave and count: 17.5 us; with an LDS
//     reduction per workgroup and at most 256 workgroups: 5.5 us.  The box kernel, which sent the box of the points as well (nobody reads it) from up to
//     1 024 workgroups: 2 x 8.7 us; now 2 x 4.2 us.
//   * What is left is the sort of the points (53 of about 105 us of kernels).  Binning the triangles instead (the reference's layout) needs a pair
//     list whose size only the data knows; binning the points needs none.  A precomputed per-triangle table was not built: the constants are
//     uniform over the group and cost it a few dozen f64 instructions.
// No floating-point atomics: two calls give equal bytes.  Compiled with -ffp-contract=off.  Every kernel keeps zero scratch.
#include "common.h"
#include "cell_list.h"
#include <math.h>
#include <algorithm>
using namespace pdhip;

namespace {

constexpr int OC_T = 256;
constexpr int OC_FMAX = 1 << 22;
constexpr int OC_QMAX = 1 << 26;
constexpr int OC_RMIN = 2, OC_RMAX = 4096;
constexpr int OC_GMAX = 2048;                 // cells per axis of the point grid
constexpr double OC_OCC = 4.0;                // G = sqrt(Q / OC_OCC)
constexpr int OC_SLAB_WAVES = 16384;          // slabs per triangle = OC_SLAB_WAVES / F, within 1 .. OC_SLABS_MAX
constexpr int OC_SLABS_MAX = 64;
constexpr int OC_SUBWAVE_F = 32768;           // from this many faces on, 16 lanes per triangle instead of a wave
constexpr int OC_NB = 256;                    // workgroups of the strided passes: each ends in a few atomics on the same addresses
enum { CNT_IN = 2 * BOX_WORDS, CNT_WARN, CNT_OUT, MISC_WORDS = 32 };      // behind the two boxes (cell_list.h)

struct OcMap {
    double sx, sy, sz, tx, ty, tz;            // x' = s * x + t
    double R, inv;                            // inv = G / R: cell = min(G - 1, floor(x' * inv))
    int G;
};

// cell of a rescaled coordinate, clamped into the grid: monotone in v, which is all the cull needs
__device__ __forceinline__ int oc_cell(double v, double inv, int G) { return (int)fmin(fmax(floor(v * inv), 0.0), (double)(G - 1)); }

// ---------------------------------------------------------------------------------------------------------------------------
// b. the points in cell order
__device__ __forceinline__ void oc_rescale(const float* __restrict__ P, size_t i, const OcMap& m, double& x, double& y, double& z) {
    x = m.sx * (double)P[3 * i] + m.tx;
    y = m.sy * (double)P[3 * i + 1] + m.ty;
    z = m.sz * (double)P[3 * i + 2] + m.tz;
}

// the xy cell key of point i of P; outside the box: G * G, behind every cell
struct OcKey {
    const float* P;
    OcMap m;
    __device__ uint64_t operator()(int i) const {
        double x, y, z;
        oc_rescale(P, (size_t)i, m, x, y, z);
        const bool in = 0.0 <= x && x <= m.R && 0.0 <= y && y <= m.R && 0.0 <= z && z <= m.R;
        return in ? (uint64_t)(oc_cell(x, m.inv, m.G) * m.G + oc_cell(y, m.inv, m.G)) : (uint64_t)(m.G * m.G);
    }
};

// sorted points as (x', y', z', index); their parity words cleared
__global__ void k_occ_gather(const int* __restrict__ val, const float* __restrict__ P, int Q, OcMap m, double4* __restrict__ sp,
                            uint32_t* __restrict__ par) {
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= Q) return;
    const int i = val[p];
    double x, y, z;
    oc_rescale(P, (size_t)i, m, x, y, z);
    sp[p] = make_double4(x, y, z, __longlong_as_double((long long)i));
    par[p] = 0u;
}

// ---------------------------------------------------------------------------------------------------------------------------
// c. group (f, slab) of LANES threads (64: a wave; 16: a quarter of one, for meshes of many small triangles, whose runs hold a handful of points):
// blockIdx.x * (OC_T / LANES) + group = f, blockIdx.y = slab of gridDim.y
template <int LANES>
__global__ __launch_bounds__(OC_T) void k_occ_tri(const float* __restrict__ V, const int64_t* __restrict__ faces, int F, OcMap m,
                                                 const double4* __restrict__ sp, const int* __restrict__ cstart, uint32_t* __restrict__ par) {
    const int lane = threadIdx.x & (LANES - 1);
    const int f = blockIdx.x * (OC_T / LANES) + threadIdx.x / LANES;
    if (f >= F) return;                                            // (the whole group of LANES threads)
    double t[3][3];
#pragma unroll
    for (int k = 0; k < 3; ++k) oc_rescale(V, (size_t)faces[3 * (size_t)f + k], m, t[k][0], t[k][1], t[k][2]);
    // check_triangles: A = [t1 - t3, t2 - t3] in xy
    const double A00 = t[0][0] - t[2][0], A01 = t[1][0] - t[2][0], A10 = t[0][1] - t[2][1], A11 = t[1][1] - t[2][1];
    const double detA = A00 * A11 - A01 * A10;
    if (detA == 0.0) return;
    const double sdet = detA > 0.0 ? 1.0 : -1.0, adet = fabs(detA);
    // compute_intersection_depth: n = cross(t3 - t1, t2 - t1)
    const double v1x = t[2][0] - t[0][0], v1y = t[2][1] - t[0][1], v1z = t[2][2] - t[0][2];
    const double v2x = t[1][0] - t[0][0], v2y = t[1][1] - t[0][1], v2z = t[1][2] - t[0][2];
    const double n0 = v1y * v2z - v1z * v2y, n1 = v1z * v2x - v1x * v2z, n2 = v1x * v2y - v1y * v2x;
    const double sn2 = n2 > 0.0 ? 1.0 : (n2 < 0.0 ? -1.0 : 0.0), an2 = fabs(n2);
    const double t1zn = t[0][2] * an2;
    // the cell box of the widened xy extent (header comment)
    const double marg = 8.0 * (4.0e-15 * m.R * m.R) * m.R / adet + 1.0e-12 * m.R;
    const double xlo = fmin(fmin(t[0][0], t[1][0]), t[2][0]) - marg, xhi = fmax(fmax(t[0][0], t[1][0]), t[2][0]) + marg;
    const double ylo = fmin(fmin(t[0][1], t[1][1]), t[2][1]) - marg, yhi = fmax(fmax(t[0][1], t[1][1]), t[2][1]) + marg;
    const int G = m.G;
    const int cx0 = oc_cell(xlo, m.inv, G), cx1 = oc_cell(xhi, m.inv, G), cy0 = oc_cell(ylo, m.inv, G), cy1 = oc_cell(yhi, m.inv, G);
    for (int cx = cx0 + (int)blockIdx.y; cx <= cx1; cx += (int)gridDim.y) {
        const int b = cstart[cx * G + cy0], e = cstart[cx * G + cy1 + 1];
        for (int p = b + lane; p < e; p += LANES) {
            const double4 q = sp[p];
            const double y0 = q.x - t[2][0], y1 = q.y - t[2][1];
            const double u = (A11 * y0 - A01 * y1) * sdet;
            const double v = (-A10 * y0 + A00 * y1) * sdet;
            const double uv = u + v;
            if (!(0.0 < u && u < adet && 0.0 < v && v < adet && 0.0 < uv && uv < adet)) continue;
            if (an2 == 0.0) continue;                              // depth is NaN: the hit counts in neither direction
            const double alpha = n0 * (t[0][0] - q.x) + n1 * (t[0][1] - q.y);
            const double depth = t1zn + alpha * sn2;
            const double rhs = q.z * an2;
            if (depth >= rhs) atomicXor(&par[p], 1u);
            else if (depth < rhs) atomicXor(&par[p], 2u);
        }
    }
}

// d. occ and the counts; cnt[0..2] = contained, parities disagree, outside the box
__global__ __launch_bounds__(OC_T) void k_occ_finish(const double4* __restrict__ sp, const uint32_t* __restrict__ par, const int* __restrict__ n_in_ptr,
                                                    int Q, uint8_t* __restrict__ occ, uint32_t* __restrict__ cnt) {
    __shared__ uint32_t sh[3];
    if (threadIdx.x < 3) sh[threadIdx.x] = 0u;
    __syncthreads();
    const int n_in = *n_in_ptr;
    uint32_t c_in = 0u, c_warn = 0u, c_out = 0u;
    for (long long p = (long long)blockIdx.x * OC_T + threadIdx.x; p < Q; p += (long long)gridDim.x * OC_T) {
        const int o = (int)__double_as_longlong(sp[p].w);
        const uint32_t bits = par[p] & 3u;
        const bool inside = p < n_in;
        const bool yes = inside && bits == 3u;
        occ[o] = yes ? 1 : 0;
        c_in += yes ? 1u : 0u;
        c_warn += (inside && (bits == 1u || bits == 2u)) ? 1u : 0u;
        c_out += inside ? 0u : 1u;
    }
    for (int off = 32; off > 0; off >>= 1) {
        c_in += (uint32_t)__shfl_xor((int)c_in, off);
        c_warn += (uint32_t)__shfl_xor((int)c_warn, off);
        c_out += (uint32_t)__shfl_xor((int)c_out, off);
    }
    if ((threadIdx.x & 63) == 0) {
        if (c_in) atomicAdd(&sh[0], c_in);
        if (c_warn) atomicAdd(&sh[1], c_warn);
        if (c_out) atomicAdd(&sh[2], c_out);
    }
    __syncthreads();
    if (threadIdx.x < 3 && sh[threadIdx.x]) atomicAdd(&cnt[threadIdx.x], sh[threadIdx.x]);      // one global atomic per workgroup and count
}

__global__ void k_occ_counts(const uint32_t* __restrict__ cnt, int32_t* __restrict__ counts) {
    counts[0] = (int32_t)cnt[0]; counts[1] = (int32_t)cnt[1]; counts[2] = (int32_t)cnt[2]; counts[3] = 0;
}

// ---------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(OC_T) void k_occ_iou(const uint8_t* __restrict__ a, const uint8_t* __restrict__ b, int Q,
                                                 unsigned long long* __restrict__ out) {
    __shared__ uint32_t sh[2];
    if (threadIdx.x < 2) sh[threadIdx.x] = 0u;
    __syncthreads();
    uint32_t ci = 0u, cu = 0u;
    for (long long i = (long long)blockIdx.x * OC_T + threadIdx.x; i < Q; i += (long long)gridDim.x * OC_T) {
        const bool x = a[i] >= 1, y = b[i] >= 1;
        ci += (x && y) ? 1u : 0u;
        cu += (x || y) ? 1u : 0u;
    }
    for (int off = 32; off > 0; off >>= 1) {
        ci += (uint32_t)__shfl_xor((int)ci, off);
        cu += (uint32_t)__shfl_xor((int)cu, off);
    }
    if ((threadIdx.x & 63) == 0) {
        if (ci) atomicAdd(&sh[0], ci);
        if (cu) atomicAdd(&sh[1], cu);
    }
    __syncthreads();
    if (threadIdx.x < 2 && sh[threadIdx.x]) atomicAdd(&out[threadIdx.x], (unsigned long long)sh[threadIdx.x]);
}

// ---------------------------------------------------------------------------------------------------------------------------
static int grid_cells(int Q) { return std::max(1, std::min(OC_GMAX, (int)floor(sqrt((double)Q / OC_OCC)))); }
static int tri_slabs(int F) { return std::max(1, std::min(OC_SLABS_MAX, OC_SLAB_WAVES / F)); }
static int tri_lanes(int F) { return F >= OC_SUBWAVE_F ? 16 : 64; }

struct OccWs {
    SortBufs sb;
    double4* sp;
    uint32_t* par;
    int* cstart;
    uint32_t* misc;                                                // box of the mesh, box of the points, the three counts
};
static size_t carve_occupancy(OccWs& w, void* base, int Q) {
    Carve c{static_cast<char*>(base), 0};
    const size_t G = (size_t)grid_cells(Q);
    carve_sort(c, w.sb, (size_t)std::max(Q, 1));
    w.sp = c.take<double4>((size_t)Q);
    w.par = c.take<uint32_t>((size_t)Q);
    w.cstart = c.take<int>(G * G + 1);
    w.misc = c.take<uint32_t>(MISC_WORDS);
    return c.off + 256;
}

}  // namespace

// tuning / test hook: 0 = slabs per triangle from F (shipped), 1 .. 64 = that many.  Same results either way.
static thread_local int g_contains_slabs = 0;
extern "C" int pdhip_debug_set_mesh_contains_slabs(int slabs) {
    int old = g_contains_slabs;
    g_contains_slabs = std::max(0, std::min(OC_SLABS_MAX, slabs));
    return old;
}

extern "C" size_t pdhip_mesh_contains_workspace_bytes(int Vn, int F, int Q, int resolution) {
    if (Vn < 1 || F < 1 || F > OC_FMAX || Q < 0 || Q > OC_QMAX || resolution < OC_RMIN || resolution > OC_RMAX) return 0;
    OccWs w;
    return carve_occupancy(w, nullptr, Q);
}

extern "C" int pdhip_mesh_contains(const float* vertices, int Vn, const int64_t* faces, int F, const float* points, int Q, int resolution,
                                   uint8_t* occ, int32_t* counts, void* ws, void* stream) {
    PD_REQUIRE(Vn >= 1, "pdhip_mesh_contains: Vn=%d vertices, need >= 1", Vn);
    PD_REQUIRE(F >= 1 && F <= OC_FMAX, "pdhip_mesh_contains: F=%d faces, need 1 .. 2^22", F);
    PD_REQUIRE(Q >= 0 && Q <= OC_QMAX, "pdhip_mesh_contains: Q=%d points, need 0 .. 2^26", Q);
    PD_REQUIRE(resolution >= OC_RMIN && resolution <= OC_RMAX, "pdhip_mesh_contains: resolution=%d, need %d .. %d", resolution, OC_RMIN, OC_RMAX);
    PD_REQUIRE(vertices, "pdhip_mesh_contains: null pointer (vertices)");
    PD_REQUIRE(faces, "pdhip_mesh_contains: null pointer (faces)");
    PD_REQUIRE(counts, "pdhip_mesh_contains: null pointer (counts)");
    PD_REQUIRE(ws, "pdhip_mesh_contains: null pointer (ws)");
    PD_REQUIRE(Q == 0 || points, "pdhip_mesh_contains: null pointer (points)");
    PD_REQUIRE(Q == 0 || occ, "pdhip_mesh_contains: null pointer (occ)");
    hipStream_t s = as_stream(stream);
    OccWs w;
    carve_occupancy(w, ws, Q);
    // a. the box of the referenced vertices, finiteness, the face indices
    int rc = clear_boxes(w.misc, 2, MISC_WORDS, s);
    if (rc) return rc;
    k_point_box<<<std::min(cdiv(F, CL_T), OC_NB), CL_T, 0, s>>>(vertices, Vn, faces, F, 1, w.misc);
    if (Q > 0) k_point_box<<<std::min(cdiv(Q, CL_T), OC_NB), CL_T, 0, s>>>(points, Q, nullptr, Q, 0, w.misc + BOX_WORDS);   // (its box: nobody reads it)
    PD_LAUNCH_CHECK();
    HostBox box[2];                                                // referenced vertices, points (counts only)
    rc = read_boxes(w.misc, box, s);
    if (rc) return rc;
    PD_REQUIRE(box[0].bad_index == 0, "pdhip_mesh_contains: %u face(s) with a vertex index outside [0, %d)", box[0].bad_index, Vn);
    PD_REQUIRE(box[0].bad == 0, "pdhip_mesh_contains: %u referenced vertex coordinate triple(s) not finite", box[0].bad);
    PD_REQUIRE(box[1].bad == 0, "pdhip_mesh_contains: %u point(s) with a non-finite coordinate", box[1].bad);
    OcMap m;
    double sc[3], tr[3];
    for (int a = 0; a < 3; ++a) {
        const double mn = box[0].mn[a], mx = box[0].mx[a];
        PD_REQUIRE(mx > mn, "pdhip_mesh_contains: flat mesh, no extent on axis %d (%g .. %g)", a, mn, mx);
        sc[a] = (double)(resolution - 1) / (mx - mn);
        const double sm = sc[a] * mn;
        tr[a] = 0.5 - sm;
    }
    m.sx = sc[0]; m.sy = sc[1]; m.sz = sc[2]; m.tx = tr[0]; m.ty = tr[1]; m.tz = tr[2];
    m.R = (double)resolution;
    m.G = grid_cells(Q);
    m.inv = (double)m.G / m.R;
    if (Q == 0) {
        PD_HIP(hipMemsetAsync(counts, 0, 4 * sizeof(int32_t), s));
        return PDHIP_OK;
    }
    // b. the points in cell order
    const int nc = m.G * m.G;
    const int cur = sort_by_cell(w.sb, Q, OcKey{points, m}, (unsigned long long)nc, w.cstart, s);      // (cstart[nc] = the points inside the box)
    k_occ_gather<<<cdiv(Q, OC_T), OC_T, 0, s>>>(w.sb.v[cur], points, Q, m, w.sp, w.par);
    PD_LAUNCH_CHECK();
    // c, d.
    const int slabs = g_contains_slabs > 0 ? g_contains_slabs : tri_slabs(F);
    if (tri_lanes(F) == 16) k_occ_tri<16><<<dim3(cdiv(F, OC_T / 16), slabs), OC_T, 0, s>>>(vertices, faces, F, m, w.sp, w.cstart, w.par);
    else k_occ_tri<64><<<dim3(cdiv(F, OC_T / 64), slabs), OC_T, 0, s>>>(vertices, faces, F, m, w.sp, w.cstart, w.par);
    k_occ_finish<<<std::min(cdiv(Q, OC_T), OC_NB), OC_T, 0, s>>>(w.sp, w.par, w.cstart + nc, Q, occ, w.misc + CNT_IN);
    k_occ_counts<<<1, 1, 0, s>>>(w.misc + CNT_IN, counts);
    PD_LAUNCH_CHECK();
    return PDHIP_OK;
}

extern "C" int pdhip_occupancy_iou(const uint8_t* a, const uint8_t* b, int Q, int64_t* out, void* stream) {
    PD_REQUIRE(Q >= 0 && Q <= OC_QMAX, "pdhip_occupancy_iou: Q=%d points, need 0 .. 2^26", Q);
    PD_REQUIRE(out, "pdhip_occupancy_iou: null pointer (out)");
    PD_REQUIRE(Q == 0 || a, "pdhip_occupancy_iou: null pointer (a)");
    PD_REQUIRE(Q == 0 || b, "pdhip_occupancy_iou: null pointer (b)");
    hipStream_t s = as_stream(stream);
    PD_HIP(hipMemsetAsync(out, 0, 2 * sizeof(int64_t), s));
    if (Q > 0) k_occ_iou<<<std::min(cdiv(Q, OC_T), OC_NB), OC_T, 0, s>>>(a, b, Q, reinterpret_cast<unsigned long long*>(out));
    PD_LAUNCH_CHECK();
    return PDHIP_OK;
}
