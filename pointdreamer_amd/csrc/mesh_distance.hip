// Point-to-mesh distance on the device (models/POCO/eval/src/eval.py: distance_p2m, i.e. trimesh.proximity.closest_point): for every point the
// closest point of the surface, its squared distance and the face.
//
//   pdhip_closest_on_mesh
//     The definition (include/pdhip.h) is Ericson's region walk per (point, face) in f64, op by op, and the minimum over the faces with the smallest
//     index on a tie.  A per-face value depends on nothing but the point and the face, so the result equals an all-pairs scan bit for bit whatever
//     is culled, as long as every face that is culled has a LARGER value than the winner.
//     a. k_point_box (cell_list.h): faces checked against [0, Vn), the box of the REFERENCED vertices, their finiteness and that of the points;
//        k_md_degenerate counts the faces whose normal is exactly zero; one small read that synchronises the stream.  A grid of C^3 cells over the
//        mesh's box (cell_list.h's Grid3, plus gmax), C ~ sqrt(F / 32);
//     b. every face gets a key (MdFaceKey): the cell of its box's min corner when it is SMALL (the cells of the two corners differ by at most one
//        per axis, so the face lies inside the cells [k, k + 1] per axis, and its closest-point arithmetic is well conditioned: below), C^3 when it is
//        LARGE, C^3 + 1 when it is degenerate.  One sort (cell_list.h) leaves [small faces by cell | large | degenerate], cstart[C^3] and
//        cstart[C^3 + 1] are where the last two start; the faces are gathered in that order as nine f32 coordinates and the index (widened where
//        they are used: 40 bytes per face instead of 80, which doubles the faces of an LDS chunk of the all-faces scan);
//     c. the queries are sorted by the cell they fall (or are clamped) into (cell_list.h's GridPointKey), so that neighbouring threads scan the same cells;
//     d. k_md_ring_scan, one thread per query: the large list first, then the keys [c - r - 1, c + r] per axis for r = 1, 2, 4, 8.  A small face that
//        was not scanned lies outside the cells [c - r, c + r], beyond a face of that cube that is not a face of the grid; the query is CERTIFIED when
//        its best d2 is <= the square of its distance to the nearest such face (md_face_bound), or when the cube is the whole grid;
//     e. a query still open after r = 8, or whose rings hold more than MD_RING_WORK faces, or facing a large list of more than MD_LARGE_WORK, or whose next cube is the whole grid of a mesh of more than
//        MD_COVER_WORK live faces (one thread would scan them all), goes to the all-faces scan (cell_list.h's k_far_scan, k_far_pick with MdFar):
//        a tile of MD_T such queries per workgroup, the live faces staged in LDS, cut into MD_FAR_SLABS slabs; no certificate needed;
//     f. k_md_closest recomputes the winner's closest point from the caller's arrays (the same operations, so the same bits): the scans keep only
//        (d2, face) in registers.
//   The guard of the certificate.  cell_list.h's grid_face_bound pulls a cube's faces in by 1e-12 of the coordinates' magnitude, which covers the
//   rounding of a point difference.  A triangle's closest point is computed less accurately: in the interior region x = a + ab v + ac w with v = vb / (va + vb + vc),
//   and va, vb, vc are differences of products of magnitude (L D)^2 (L the edge length, D the distance of the query) while their sum is |n|^2, so
//   the computed x can leave the triangle, within its plane, by about 2^-53 D^2 L^3 / |n|^2.  Hence (i) the guard here is 1e-7 of (|q| + the largest
//   coordinate magnitude of the mesh's box), and (ii) a face for which 64 * 2^-53 Dc^2 Lmax^3 / |n|^2, with Dc = 18 cells + Lmax the largest
//   distance at which the certificate can still be decided by it, exceeds a quarter of that guard is put on the large list, which every query scans:
//   slivers and faces that are tiny against the cells never rely on the certificate.  This is an error estimate, not a proof; the tests hold every
//   path to bit equality with the all-pairs oracle, including slivers.
//   pdhip_debug_set_closest_on_mesh(cells, path): cells > 0 overrides C, path 1 puts every live face on the large list, path 2 sends every query to
//   the all-faces scan.  Same bytes under all of them.
// No floating-point atomics: two calls give equal bytes.  Compiled with -ffp-contract=off.  Every kernel keeps zero scratch.
#include "common.h"
#include "cell_list.h"
#include <math.h>
#include <limits.h>
#include <algorithm>
using namespace pdhip;

namespace {

constexpr int MD_T = 256;                     // queries per workgroup of the all-faces scan
constexpr int MD_CHUNK = 512;                 // faces staged at a time: 20 KiB of LDS
constexpr int MD_P2_T = 64;
constexpr int MD_RING_MAX = 8;                // the ring scan gives up after the cube [c - 8, c + 8], or after MD_RING_WORK faces ...
constexpr int MD_RING_WORK = 2048;
constexpr int MD_LARGE_WORK = 8192;           // ... or when the large list, which every query scans first, is longer than this ...
constexpr int MD_COVER_WORK = 256;            // ... or when its cube becomes the whole grid of a mesh of more live faces than this ...
constexpr int MD_FAR_SLABS = 16;              // ... and the all-faces scan cuts the faces into this many slabs per tile of MD_T queries
constexpr int MD_CELLS_MAX = 96;              // cells per axis (the workspace holds MD_CELLS_MAX^3 + 2 cell starts whatever C is)
constexpr double MD_OCC = 32.0;               // C = sqrt(F / MD_OCC)
constexpr int MD_FMAX = 1 << 23;              // simplify_mesh's limit
constexpr int MD_QMAX = 1 << 26;              // cloud_metrics' limit
constexpr int MD_NB = 256;                    // workgroups of the strided passes
constexpr double MD_GUARD = 1.0e-7;
// behind the two boxes (cell_list.h) a third block of BOX_WORDS words read with them: its BOX_BAD word counts the degenerate faces
enum { MISC_DEG = 2 * BOX_WORDS + BOX_BAD, MISC_FAR = 3 * BOX_WORDS, MISC_WORDS = 32 };

struct MdGrid : Grid3 {
    double gmax;                              // largest coordinate magnitude of the mesh's box
};

struct alignas(8) MdFace {
    float a[3], b[3], c[3];
    int idx;
};

__host__ __device__ __forceinline__ int md_imax(int a, int b) { return a > b ? a : b; }
__host__ __device__ __forceinline__ int md_imin(int a, int b) { return a < b ? a : b; }

// distance from q to the nearest face of the cells [c0, c1] that is not a face of the whole grid, less the guard
__host__ __device__ __forceinline__ double md_face_bound(double q, double o, double cs, int C, int c0, int c1, double gmax) {
    double b = 1.0e300;
    const double guard = MD_GUARD * (fabs(q) + gmax);
    if (c0 > 0) b = fmin(b, (q - (o + (double)c0 * cs)) - guard);
    if (c1 < C - 1) b = fmin(b, ((o + (double)(c1 + 1) * cs) - q) - guard);
    return b;
}

__host__ __device__ __forceinline__ double md_dot(double ux, double uy, double uz, double vx, double vy, double vz) { return (ux * vx + uy * vy) + uz * vz; }

// the definition: closest point x of triangle (a, b, c) to q and d2 = |q - x|^2.  The first region that holds decides; one division serves them all
// (an edge region's num / den, the interior's 1 / ((va + vb) + vc)), the rest is selects: the regions diverge from lane to lane.
__host__ __device__ __forceinline__ double md_closest(double qx, double qy, double qz, double ax, double ay, double az, double bx, double by, double bz,
                                                      double cx, double cy, double cz, double& xx, double& xy, double& xz) {
    const double abx = bx - ax, aby = by - ay, abz = bz - az;
    const double acx = cx - ax, acy = cy - ay, acz = cz - az;
    const double bcx = cx - bx, bcy = cy - by, bcz = cz - bz;
    const double d1 = md_dot(abx, aby, abz, qx - ax, qy - ay, qz - az), d2 = md_dot(acx, acy, acz, qx - ax, qy - ay, qz - az);
    const double d3 = md_dot(abx, aby, abz, qx - bx, qy - by, qz - bz), d4 = md_dot(acx, acy, acz, qx - bx, qy - by, qz - bz);
    const double d5 = md_dot(abx, aby, abz, qx - cx, qy - cy, qz - cz), d6 = md_dot(acx, acy, acz, qx - cx, qy - cy, qz - cz);
    const double vc = d1 * d4 - d3 * d2, vb = d5 * d2 - d1 * d6, va = d3 * d6 - d5 * d4, e43 = d4 - d3, e56 = d5 - d6;
    const bool r1 = d1 <= 0.0 && d2 <= 0.0;
    const bool r2 = !r1 && d3 >= 0.0 && d4 <= d3;
    const bool r12 = r1 || r2;
    const bool r3 = !r12 && vc <= 0.0 && d1 >= 0.0 && d3 <= 0.0;
    const bool r123 = r12 || r3;
    const bool r4 = !r123 && d6 >= 0.0 && d5 <= d6;
    const bool r1234 = r123 || r4;
    const bool r5 = !r1234 && vb <= 0.0 && d2 >= 0.0 && d6 <= 0.0;
    const bool r12345 = r1234 || r5;
    const bool r6 = !r12345 && va <= 0.0 && e43 >= 0.0 && e56 >= 0.0;
    const bool r7 = !r12345 && !r6;
    const bool vertex = r1 || r2 || r4;
    const double num = r3 ? d1 : r5 ? d2 : r6 ? e43 : 1.0;
    const double den = r3 ? d1 - d3 : r5 ? d2 - d6 : r6 ? e43 + e56 : r7 ? (va + vb) + vc : 1.0;
    const double t = num / den;
    // vertex regions: the vertex; edge regions: base + t * dir; interior: (a + ab (vb t)) + ac (vc t)
    const double px = r2 ? bx : r4 ? cx : r6 ? bx : ax, py = r2 ? by : r4 ? cy : r6 ? by : ay, pz = r2 ? bz : r4 ? cz : r6 ? bz : az;
    const double ux = r5 ? acx : r6 ? bcx : abx, uy = r5 ? acy : r6 ? bcy : aby, uz = r5 ? acz : r6 ? bcz : abz;
    const double s = r7 ? vb * t : t;
    double ex = px + s * ux, ey = py + s * uy, ez = pz + s * uz;   // (regions 3, 5, 6: a + t ab, a + t ac, b + t bc; 7: a + ab (vb den))
    if (r7) {
        const double w = vc * t;
        ex = ex + acx * w; ey = ey + acy * w; ez = ez + acz * w;
    }
    xx = vertex ? px : ex; xy = vertex ? py : ey; xz = vertex ? pz : ez;
    const double rx = qx - xx, ry = qy - xy, rz = qz - xz;
    return md_dot(rx, ry, rz, rx, ry, rz);
}

__host__ __device__ __forceinline__ double md_face_d2(double qx, double qy, double qz, const MdFace& f) {
    double x, y, z;
    return md_closest(qx, qy, qz, (double)f.a[0], (double)f.a[1], (double)f.a[2], (double)f.b[0], (double)f.b[1], (double)f.b[2], (double)f.c[0],
                      (double)f.c[1], (double)f.c[2], x, y, z);
}

__host__ __device__ __forceinline__ bool md_degenerate(double ax, double ay, double az, double bx, double by, double bz, double cx, double cy, double cz,
                                              double& n2) {
    const double abx = bx - ax, aby = by - ay, abz = bz - az, acx = cx - ax, acy = cy - ay, acz = cz - az;
    const double nx = aby * acz - abz * acy, ny = abz * acx - abx * acz, nz = abx * acy - aby * acx;
    n2 = (nx * nx + ny * ny) + nz * nz;
    return nx == 0.0 && ny == 0.0 && nz == 0.0;
}

// ---------------------------------------------------------------------------------------------------------------------------
// a. faces whose normal is exactly zero (a face with an index outside [0, Vn) is skipped: k_point_box counts those, and the call is refused)
__global__ __launch_bounds__(CL_T) void k_md_degenerate(const float* __restrict__ V, int Vn, const int64_t* __restrict__ faces, int F,
                                                        uint32_t* __restrict__ count) {
    __shared__ uint32_t sh;
    if (threadIdx.x == 0) sh = 0u;
    __syncthreads();
    uint32_t n = 0u;
    for (long long i = (long long)blockIdx.x * CL_T + threadIdx.x; i < F; i += (long long)gridDim.x * CL_T) {
        const long long i0 = faces[3 * i], i1 = faces[3 * i + 1], i2 = faces[3 * i + 2];
        if (i0 < 0 || i0 >= Vn || i1 < 0 || i1 >= Vn || i2 < 0 || i2 >= Vn) continue;
        double n2;
        n += md_degenerate((double)V[3 * i0], (double)V[3 * i0 + 1], (double)V[3 * i0 + 2], (double)V[3 * i1], (double)V[3 * i1 + 1],
                           (double)V[3 * i1 + 2], (double)V[3 * i2], (double)V[3 * i2 + 1], (double)V[3 * i2 + 2], n2) ? 1u : 0u;
    }
    for (int off = 32; off > 0; off >>= 1) n += (uint32_t)__shfl_xor((int)n, off);
    if ((threadIdx.x & 63) == 0 && n) atomicAdd(&sh, n);
    __syncthreads();
    if (threadIdx.x == 0 && sh) atomicAdd(count, sh);
}

// b. the key of face i (the call has validated the indices and the vertices by now)
struct MdFaceKey {
    const float* V;
    const int64_t* faces;
    MdGrid g;
    int all_large;
    __host__ __device__ uint64_t operator()(int i) const {
        const long long i0 = faces[3 * (size_t)i], i1 = faces[3 * (size_t)i + 1], i2 = faces[3 * (size_t)i + 2];
        const double ax = (double)V[3 * i0], ay = (double)V[3 * i0 + 1], az = (double)V[3 * i0 + 2];
        const double bx = (double)V[3 * i1], by = (double)V[3 * i1 + 1], bz = (double)V[3 * i1 + 2];
        const double cx = (double)V[3 * i2], cy = (double)V[3 * i2 + 1], cz = (double)V[3 * i2 + 2];
        const int C = g.C;
        const uint64_t large = (uint64_t)C * C * C;
        double n2;
        if (md_degenerate(ax, ay, az, bx, by, bz, cx, cy, cz, n2)) return large + 1;
        if (all_large) return large;
        const int x0 = g.cell(fmin(fmin(ax, bx), cx), g.ox), x1 = g.cell(fmax(fmax(ax, bx), cx), g.ox);
        const int y0 = g.cell(fmin(fmin(ay, by), cy), g.oy), y1 = g.cell(fmax(fmax(ay, by), cy), g.oy);
        const int z0 = g.cell(fmin(fmin(az, bz), cz), g.oz), z1 = g.cell(fmax(fmax(az, bz), cz), g.oz);
        if (x1 - x0 > 1 || y1 - y0 > 1 || z1 - z0 > 1) return large;
        // conditioning of the closest-point arithmetic (header comment)
        const double l1 = md_dot(bx - ax, by - ay, bz - az, bx - ax, by - ay, bz - az), l2 = md_dot(cx - ax, cy - ay, cz - az, cx - ax, cy - ay, cz - az),
                     l3 = md_dot(cx - bx, cy - by, cz - bz, cx - bx, cy - by, cz - bz);
        const double lm2 = fmax(fmax(l1, l2), l3), lm = sqrt(lm2), dc = 18.0 * g.cs + lm;
        const double est = 64.0 * 1.1102230246251565e-16 * (dc * dc) * (lm2 * lm) / n2;
        if (!(est <= 0.25 * MD_GUARD * g.gmax)) return large;
        return (uint64_t)((z0 * C + y0) * C + x0);
    }
};

__global__ void k_md_gather(const int* __restrict__ val, const float* __restrict__ V, const int64_t* __restrict__ faces, int F,
                            MdFace* __restrict__ sf) {
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= F) return;
    const int i = val[p];
    const long long i0 = faces[3 * (size_t)i], i1 = faces[3 * (size_t)i + 1], i2 = faces[3 * (size_t)i + 2];
    MdFace f;
#pragma unroll
    for (int k = 0; k < 3; ++k) { f.a[k] = V[3 * i0 + k]; f.b[k] = V[3 * i1 + k]; f.c[k] = V[3 * i2 + k]; }
    f.idx = i;
    sf[p] = f;
}

// ---------------------------------------------------------------------------------------------------------------------------
// d. one query against the large list and the rings of the cell list.  cstart[nc] / cstart[nc + 1]: where the large / the degenerate faces start in
// sf.  True: (bd, bi) is the result.  False: the query goes to the all-faces scan.  (Host code as well, like the functions it calls: a host program can run the very cull against the oracle without a device.)
__host__ __device__ __forceinline__ bool md_ring_query(double qx, double qy, double qz, const MdFace* __restrict__ sf, const int* __restrict__ cstart,
                                                       const MdGrid& g, double& bd, int& bi) {
    const int C = g.C, nc = C * C * C;
    const int lb = cstart[nc], le = cstart[nc + 1];
    if (le - lb > MD_LARGE_WORK) return false;                     // a long large list: the staged sweep of all faces is the cheaper way
    int work = 0;
    bd = INFINITY;
    bi = INT_MAX;
    for (int p = lb; p < le; ++p) {
        const MdFace f = sf[p];
        take_min(md_face_d2(qx, qy, qz, f), f.idx, bd, bi);
    }
    if (lb == 0) return true;                                      // no small face: every live face has been scanned
    const int cx = g.cell(qx, g.ox), cy = g.cell(qy, g.oy), cz = g.cell(qz, g.oz);
    for (int r = 1;; r *= 2) {
        // the cells [c - r, c + r] the certificate speaks about; a face that can reach them has a key in [c - r - 1, c + r]
        const int x0 = md_imax(cx - r, 0), x1 = md_imin(cx + r, C - 1), y0 = md_imax(cy - r, 0), y1 = md_imin(cy + r, C - 1), z0 = md_imax(cz - r, 0),
                  z1 = md_imin(cz + r, C - 1);
        const int kx0 = md_imax(cx - r - 1, 0), ky0 = md_imax(cy - r - 1, 0), kz0 = md_imax(cz - r - 1, 0);
        const bool covers = x0 == 0 && y0 == 0 && z0 == 0 && x1 == C - 1 && y1 == C - 1 && z1 == C - 1;
        if (covers && le > MD_COVER_WORK) return false;            // this ring would be a scan of all faces by one thread: the staged sweep does that better
        for (int z = kz0; z <= z1; ++z)
            for (int y = ky0; y <= y1; ++y) {
                const int base = (z * C + y) * C;
                const int b = cstart[base + kx0], e = cstart[base + x1 + 1];
                work += e - b;
                if (work > MD_RING_WORK) return false;             // crowded cells
                for (int p = b; p < e; ++p) {
                    const MdFace f = sf[p];
                    take_min(md_face_d2(qx, qy, qz, f), f.idx, bd, bi);
                }
            }
        const double b = fmin(fmin(md_face_bound(qx, g.ox, g.cs, C, x0, x1, g.gmax), md_face_bound(qy, g.oy, g.cs, C, y0, y1, g.gmax)),
                              md_face_bound(qz, g.oz, g.cs, C, z0, z1, g.gmax));
        if (covers || (bi != INT_MAX && b > 0.0 && bd <= b * b)) return true;
        if (r >= MD_RING_MAX) return false;                        // far from the surface: a thread of its own would scan most of the grid
    }
}

// one thread per sorted query
__global__ __launch_bounds__(MD_P2_T) void k_md_ring_scan(const float4* __restrict__ sq, int Q, const MdFace* __restrict__ sf,
                                                          const int* __restrict__ cstart, MdGrid g, int all_far, double* __restrict__ d2,
                                                          int* __restrict__ face, int* __restrict__ far_list, int* __restrict__ far_n) {
    const int sp = blockIdx.x * MD_P2_T + threadIdx.x;
    if (sp >= Q) return;
    const float4 me = sq[sp];
    double bd = INFINITY;
    int bi = INT_MAX;
    if (all_far || !md_ring_query((double)me.x, (double)me.y, (double)me.z, sf, cstart, g, bd, bi)) {
        far_list[atomicAdd(far_n, 1)] = sp;
        return;
    }
    const int o = __float_as_int(me.w);
    d2[o] = bd;
    face[o] = bi == INT_MAX ? -1 : bi;
}

// e. every live face sf[0 .. cstart[nc + 1]) against every query of the list (cell_list.h's k_far_scan / k_far_pick)
struct MdFar {
    const int* n_live;
    int F;
    __device__ int live() const { return min(max(*n_live, 0), F); }
    __device__ double d2(double qx, double qy, double qz, const MdFace& f, int& k) const {
        k = f.idx;
        return md_face_d2(qx, qy, qz, f);
    }
    static __device__ double none() { return INFINITY; }
    static __device__ int index(int bi) { return bi == INT_MAX ? -1 : bi; }
};

// f. the winner's closest point, from the caller's arrays
__global__ __launch_bounds__(MD_T) void k_md_closest(const float* __restrict__ V, const int64_t* __restrict__ faces, const float* __restrict__ P, int Q,
                                                     const int* __restrict__ face, double* __restrict__ closest) {
    const int q = blockIdx.x * MD_T + threadIdx.x;
    if (q >= Q) return;
    const int f = face[q];
    double x = NAN, y = NAN, z = NAN;
    if (f >= 0) {
        const long long i0 = faces[3 * (size_t)f], i1 = faces[3 * (size_t)f + 1], i2 = faces[3 * (size_t)f + 2];
        md_closest((double)P[3 * (size_t)q], (double)P[3 * (size_t)q + 1], (double)P[3 * (size_t)q + 2], (double)V[3 * i0], (double)V[3 * i0 + 1],
                   (double)V[3 * i0 + 2], (double)V[3 * i1], (double)V[3 * i1 + 1], (double)V[3 * i1 + 2], (double)V[3 * i2], (double)V[3 * i2 + 1],
                   (double)V[3 * i2 + 2], x, y, z);
    }
    closest[3 * (size_t)q] = x; closest[3 * (size_t)q + 1] = y; closest[3 * (size_t)q + 2] = z;
}

__global__ void k_md_counts(const int* __restrict__ far_n, const int* __restrict__ cstart, int nc, int Q, int F, int32_t* __restrict__ counts) {
    const int n = min(*far_n, Q);
    counts[0] = Q - n; counts[1] = n; counts[2] = cstart[nc + 1] - cstart[nc]; counts[3] = F - cstart[nc + 1];
}

// ---------------------------------------------------------------------------------------------------------------------------
static int cells_axis(int F) { return std::max(1, std::min(MD_CELLS_MAX, (int)floor(sqrt((double)F / MD_OCC)))); }

struct MeshDistWs {
    SortBufs sb;
    MdFace* sf;
    float4* sq;
    int *cstart, *far_list, *part_idx;
    double* part_d2;
    uint32_t* misc;                                                // box of the mesh, box of the points, the degenerate count, the far counter
};
static size_t carve_mesh_distance(MeshDistWs& w, void* base, int F, int Q) {
    Carve c{static_cast<char*>(base), 0};
    carve_sort(c, w.sb, (size_t)std::max(std::max(F, Q), 1));
    w.sf = c.take<MdFace>((size_t)F);
    w.sq = c.take<float4>((size_t)Q);
    w.cstart = c.take<int>((size_t)MD_CELLS_MAX * MD_CELLS_MAX * MD_CELLS_MAX + 2);
    w.far_list = c.take<int>((size_t)Q);
    w.part_d2 = c.take<double>((size_t)MD_FAR_SLABS * Q);
    w.part_idx = c.take<int>((size_t)MD_FAR_SLABS * Q);
    w.misc = c.take<uint32_t>(MISC_WORDS);
    return c.off + 256;
}

}  // namespace

// tuning / test hook (include/pdhip.h).  Same results under every setting.
static thread_local int g_md_cells = 0, g_md_path = 0;
extern "C" int pdhip_debug_set_closest_on_mesh(int cells_per_axis, int path) {
    const int old = g_md_cells * 4 + g_md_path;
    g_md_cells = std::max(0, std::min(MD_CELLS_MAX, cells_per_axis));
    g_md_path = (path == 1 || path == 2) ? path : 0;
    return old;
}

extern "C" size_t pdhip_closest_on_mesh_workspace_bytes(int Vn, int F, int Q) {
    if (Vn < 1 || F < 1 || F > MD_FMAX || Q < 0 || Q > MD_QMAX) return 0;
    MeshDistWs w;
    return carve_mesh_distance(w, nullptr, F, Q);
}

extern "C" int pdhip_closest_on_mesh(const float* vertices, int Vn, const int64_t* faces, int F, const float* points, int Q, double* d2,
                                     int32_t* face, double* closest, int32_t* counts, void* ws, void* stream) {
    PD_REQUIRE(F != 0, "pdhip_closest_on_mesh: F=0 faces: a degenerate mesh, no surface to measure against");
    PD_REQUIRE(Vn >= 1, "pdhip_closest_on_mesh: Vn=%d vertices, need >= 1", Vn);
    PD_REQUIRE(F >= 1 && F <= MD_FMAX, "pdhip_closest_on_mesh: F=%d faces, need 1 .. 2^23", F);
    PD_REQUIRE(Q >= 0 && Q <= MD_QMAX, "pdhip_closest_on_mesh: Q=%d points, need 0 .. 2^26", Q);
    PD_REQUIRE(vertices, "pdhip_closest_on_mesh: null pointer (vertices)");
    PD_REQUIRE(faces, "pdhip_closest_on_mesh: null pointer (faces)");
    PD_REQUIRE(counts, "pdhip_closest_on_mesh: null pointer (counts)");
    PD_REQUIRE(ws, "pdhip_closest_on_mesh: null pointer (ws)");
    PD_REQUIRE(Q == 0 || points, "pdhip_closest_on_mesh: null pointer (points)");
    PD_REQUIRE(Q == 0 || d2, "pdhip_closest_on_mesh: null pointer (d2)");
    PD_REQUIRE(Q == 0 || face, "pdhip_closest_on_mesh: null pointer (face)");
    hipStream_t s = as_stream(stream);
    MeshDistWs w;
    carve_mesh_distance(w, ws, F, Q);
    // a. the box of the referenced vertices, finiteness, the face indices, the degenerate faces
    int rc = clear_boxes(w.misc, 2, MISC_WORDS, s);
    if (rc) return rc;
    k_point_box<<<std::min(cdiv(F, CL_T), MD_NB), CL_T, 0, s>>>(vertices, Vn, faces, F, 1, w.misc);
    if (Q > 0) k_point_box<<<std::min(cdiv(Q, CL_T), MD_NB), CL_T, 0, s>>>(points, Q, nullptr, Q, 0, w.misc + BOX_WORDS);   // (its box: nobody reads it)
    k_md_degenerate<<<std::min(cdiv(F, CL_T), MD_NB), CL_T, 0, s>>>(vertices, Vn, faces, F, w.misc + MISC_DEG);
    PD_LAUNCH_CHECK();
    HostBox box[3];                                                // referenced vertices, points (counts only), [2].bad = degenerate faces
    rc = read_boxes(w.misc, box, s);
    if (rc) return rc;
    PD_REQUIRE(box[0].bad_index == 0, "pdhip_closest_on_mesh: %u face(s) with a vertex index outside [0, %d)", box[0].bad_index, Vn);
    PD_REQUIRE(box[0].bad == 0, "pdhip_closest_on_mesh: %u referenced vertex coordinate triple(s) not finite", box[0].bad);
    PD_REQUIRE(box[1].bad == 0, "pdhip_closest_on_mesh: %u point(s) with a non-finite coordinate", box[1].bad);
    PD_REQUIRE(box[2].bad < (uint32_t)F, "pdhip_closest_on_mesh: every one of the %d face(s) is degenerate (a zero normal): no surface to measure against", F);
    if (Q == 0) {
        PD_HIP(hipMemsetAsync(counts, 0, 4 * sizeof(int32_t), s));
        return PDHIP_OK;
    }
    MdGrid g{grid_over(box[0].mn, box_extent(box[0].mn, box[0].mx), g_md_cells > 0 ? g_md_cells : cells_axis(F)), 0.0};
    for (int a = 0; a < 3; ++a) g.gmax = std::max(g.gmax, std::max(fabs(box[0].mn[a]), fabs(box[0].mx[a])));
    const int nc = g.C * g.C * g.C;
    // b. the faces: [small by cell | large | degenerate]
    int cur = sort_by_cell(w.sb, F, MdFaceKey{vertices, faces, g, g_md_path == 1}, (unsigned long long)nc + 1, w.cstart, s);
    k_md_gather<<<cdiv(F, CL_T), CL_T, 0, s>>>(w.sb.v[cur], vertices, faces, F, w.sf);
    // c. the queries in cell order
    cur = sort_by_cell(w.sb, Q, GridPointKey{points, g}, (unsigned long long)nc, nullptr, s);
    k_gather_xyzi<<<cdiv(Q, CL_T), CL_T, 0, s>>>(w.sb.v[cur], points, Q, w.sq);
    PD_LAUNCH_CHECK();
    // d, e, f.
    int* far_n = reinterpret_cast<int*>(w.misc + MISC_FAR);
    k_md_ring_scan<<<cdiv(Q, MD_P2_T), MD_P2_T, 0, s>>>(w.sq, Q, w.sf, w.cstart, g, g_md_path == 2, d2, face, w.far_list, far_n);
    k_far_scan<MD_T, MD_CHUNK, MD_FAR_SLABS><<<dim3(cdiv(Q, MD_T), MD_FAR_SLABS), MD_T, 0, s>>>(w.sq, w.far_list, far_n, Q, w.sf, MdFar{w.cstart + nc + 1, F}, w.part_d2, w.part_idx);
    k_far_pick<MD_T, MD_FAR_SLABS, MdFar><<<cdiv(Q, MD_T), MD_T, 0, s>>>(w.sq, w.far_list, far_n, Q, w.part_d2, w.part_idx, d2, face);
    if (closest != nullptr) k_md_closest<<<cdiv(Q, MD_T), MD_T, 0, s>>>(vertices, faces, points, Q, face, closest);
    k_md_counts<<<1, 1, 0, s>>>(far_n, w.cstart, nc, Q, F, counts);
    PD_LAUNCH_CHECK();
    return PDHIP_OK;
}
