// Welding of close vertices and the cleaning of a face list (include/pdhip.h has the contracts; DESIGN.md section 6, "Cleaning").  The first step of
// the mesh chain for meshes that users supply: a triangle soup, an unwelded marching-cubes export or a mesh with seams has no shared vertex INDICES,
// which is all that the components filter, the smoothing, the decimation, the unwrap and the neighbour CSR look at.  Counterparts: trimesh's
// merge_vertices, MeshLab's "Merge Close Vertices", "Remove Duplicate Faces", "Remove Unreferenced Vertices".  The compaction is mesh_components.hip's
// pdhip_compact_mesh: after relabelling no face names a vertex that is not a representative, so it drops them with the unreferenced ones.
//
// pdhip_weld_vertices.  i and j are close when d2(i, j) <= tol * tol, d2 = cell_list.h's point_d2 (symmetric bit for bit: dx -> -dx leaves dx * dx
// as it is); a class is a connected component of that graph (single linkage), its representative its smallest index.
//   a. k_point_box: the box, and the count of non-finite vertices (the entry's one read before the final check words; a non-finite vertex is refused)
//   b. a Grid3 of C^3 cells over the box, C = min(sqrt(Vn / 8), 256, ext / (1.001 tol + 4e-12 max|x|)): the cell edge exceeds tol; sort_by_cell, the
//      sorted (x, y, z, index) copy
//   c. k_mw_scan, one thread per SORTED vertex (neighbouring lanes read the same cells): the smallest ring r whose cube [c - r, c + r] is certified,
//      then one pass over that cube: every vertex j < i with d2 <= tol * tol is united with i (the pair is seen from its larger end: one union each)
//   d. k_mw_flatten: rep[v] = the root of v, read-only on parent[]; the classes counted by integer atomics
// Exactness.  The cube of query q is certified when it covers the grid, or when b = grid_cube_bound(q, cube) > 0 and tol * tol <= b * b.
//   - An unvisited vertex t lies in a cell outside the cube, beyond a face f of the cube that is not a face of the grid: its computed cell index is
//     beyond the cube's along some axis, so t is on the far side of f up to the rounding of (x - o) / cs and of f = o + c cs (some 1e-16 of the
//     coordinates' magnitude), and |q - t| along that axis exceeds b, which grid_face_bound pulled in by 1e-12 of that magnitude -- by far more than
//     those roundings and than the one rounding that b * b >= tol * tol can hide.  d2 >= fl(dx * dx) (adding a non-negative term and rounding never
//     goes below a representable summand), and fl is monotone, so the COMPUTED d2 of t is > fl(b * b) >= tol * tol: t is not close, whatever the
//     order.  The scan therefore sees every close pair, and tests each with the very expression of the definition.
//   - A pair at exactly tol * tol: both are in each other's certified cubes (the above, read backwards: a vertex outside has d2 > tol * tol), the
//     test is d2 <= tol2 with tol2 = tol * tol computed once on the host in f64, as the definition has it: it merges.  The next f64 above does not.
//   - A pair that straddles a cell face lies in two cells of one cube: r >= 1 always, so the 26 neighbours are scanned, and the certificate measures
//     q's distance to the cube's OUTER faces, at least one cell edge > tol away when q's cell is computed exactly, and re-measured from q's own
//     coordinates when it is not: a query that the rounding of its cell index put on the wrong side of a face just gets a smaller b, and a wider ring.
//   - Clamped boundary cells: a vertex outside the grid (none here: the grid spans the box, but the stretch of 1e-6 and rounding may put the far
//     corner's cell at C) is clamped INTO a boundary cell; nothing lies behind a face of the grid, which is why only non-grid faces bound b.
//   - tol == 0 is the same path: tol2 = 0, the certificate asks b > 0, equal coordinates give d2 == 0 (-0.0 and +0.0 too: their difference is 0).
//   The ring loop ends at r <= C (cube_around clamps: r = C - 1 covers the grid).  rep is then a function of the closeness graph alone: the
//   union-find of union_find.h ends with each class's smallest index as its one root, whatever the threads' order.
// Cost: a thread visits every vertex of its cube, so a cell with n vertices costs n * (vertices of its 27 cells) >= n^2 steps: QUADRATIC in a crowded
// cell, bounded by Vn per thread and Vn^2 <= 2^52 in all (no loop depends on data beyond that; profiles/mesh_clean_bench.txt has a crowded row).
// A close j whose parent is already an ancestor of i costs one load and no union.
//
// pdhip_clean_faces.  k_mcf_keys: per face the key (lo, mid, hi) of its relabelled, sorted indices, `bits` bits each (bits = those of Vn - 1, <= 21:
// three fit below bit 63), a degenerate face the key 1 << 3 bits, which sorts last; a face index or a rep value outside [0, Vn) is counted and
// nothing but the temporaries is written.  A STABLE radix sort with the face index as value: of a run of equal keys the first is the smallest face
// index.  k_mcf_out: out_faces, keep, counts.
// Integer atomics only, no floating-point atomics, zero scratch; two calls give equal bytes.  Every temporary is a typed array of the caller's.
#include "cell_list.h"
#include "mesh_common.h"
#include "union_find.h"

namespace pdhip {
namespace {

constexpr int TB = 256;
constexpr int MAX_V_FACES = 1 << 21;                               // pdhip_clean_faces: three indices of 21 bits in one key
constexpr int CELLS_MAX = 256;
constexpr int MISC_WORDS = 64;                                     // one 256-byte line
enum { W_CAP = BOX_WORDS, W_CLASSES, W_WIDE };                     // pdhip_weld_vertices' misc, behind the box
enum { F_BADIDX = 0, F_BADREP };                                   // pdhip_clean_faces' misc
enum { C_DEGENERATE = 0, C_DUPLICATE, C_KEPT };

static int cells_axis_for(int Vn) { return std::max(1, std::min(CELLS_MAX, (int)floor(sqrt((double)Vn / 8.0)))); }
static size_t hist_len(size_t n) { return 2 * 256 * (size_t)cdiv((long long)n, RS_TILE); }

// ---- welding
__global__ __launch_bounds__(TB) void k_mw_scan(const float4* __restrict__ sp, int Vn, const int* __restrict__ cstart, Grid3 g, double tol2, int* parent,
                                                int* __restrict__ misc) {
    const int p = blockIdx.x * blockDim.x + threadIdx.x, lane = threadIdx.x & 63;
    bool wide = false;
    if (p < Vn) {
        const float4 me = sp[p];
        const int i = __float_as_int(me.w), C = g.C;
        const double qx = (double)me.x, qy = (double)me.y, qz = (double)me.z;
        const int cx = g.cell(qx, g.ox), cy = g.cell(qy, g.oy), cz = g.cell(qz, g.oz);
        CellCube q = cube_around(cx, cy, cz, 1, C);
        for (int r = 1; r < C; ++r) {                              // (r = C - 1 covers the grid from any cell)
            q = cube_around(cx, cy, cz, r, C);
            const double b = grid_cube_bound(g, qx, qy, qz, q);
            if (q.covers(C) || (b > 0.0 && tol2 <= b * b)) break;
            wide = true;
        }
        int known = i;                                             // an ancestor of i, or i: a close j below it needs no union
        bool spent = false;
        for (int z = q.z0; z <= q.z1; ++z)
            for (int y = q.y0; y <= q.y1; ++y) {
                const int base = (z * C + y) * C;
                const int b = cstart[base + q.x0], e = cstart[base + q.x1 + 1];
                for (int k = b; k < e; ++k) {
                    const float4 a = sp[k];
                    const int j = __float_as_int(a.w);
                    if (j >= i || !(point_d2(qx, qy, qz, a) <= tol2)) continue;
                    const int pj = ld_agent(parent + j);
                    if (pj == known) continue;
                    long long budget = 2ll * Vn + 64;
                    const int r = unite(parent, find_root(parent, known, budget), find_root(parent, pj, budget), budget);
                    if (r < 0) spent = true; else known = r;
                }
            }
        if (spent) atomicOr(&misc[W_CAP], 1);
    }
    wave_count(&misc[W_WIDE], wide, lane);
}

// rep[v] = the class's smallest index (parent[] is read only here: equal bytes on repeats)
__global__ __launch_bounds__(TB) void k_mw_flatten(const int* __restrict__ parent, int Vn, int32_t* __restrict__ rep, int* __restrict__ misc) {
    const int v = blockIdx.x * blockDim.x + threadIdx.x, lane = threadIdx.x & 63;
    bool root = false;
    if (v < Vn && !misc[W_CAP]) {
        int steps = Vn;
        int r = walk_root(parent, v, steps);
        if (r < 0) { atomicOr(&misc[W_CAP], 2); r = v; }
        rep[v] = r;
        root = r == v;
    }
    wave_count(&misc[W_CLASSES], root, lane);
}

__global__ void k_mw_counts(const int* __restrict__ misc, int Vn, int C, int32_t* __restrict__ counts) {
    if (misc[W_CAP]) return;
    counts[0] = misc[W_CLASSES]; counts[1] = Vn - misc[W_CLASSES]; counts[2] = C; counts[3] = misc[W_WIDE];
}

// ---- faces
__global__ __launch_bounds__(TB) void k_mcf_keys(const int64_t* __restrict__ faces, int F, int Vn, const int32_t* __restrict__ rep, int bits,
                                                 uint64_t* __restrict__ key, int* __restrict__ val, int* __restrict__ misc) {
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= F) return;
    const int64_t a = faces[3 * (size_t)f], b = faces[3 * (size_t)f + 1], c = faces[3 * (size_t)f + 2];
    uint64_t k = 1ull << (3 * bits);                               // a degenerate face (and a refused one: nothing reads its key then)
    if (!(index_ok(a, Vn) && index_ok(b, Vn) && index_ok(c, Vn))) {
        atomicAdd(&misc[F_BADIDX], 1);
    } else {
        const int ra = rep[a], rb = rep[b], rc = rep[c];
        if (!(index_ok(ra, Vn) && index_ok(rb, Vn) && index_ok(rc, Vn))) {
            atomicAdd(&misc[F_BADREP], 1);
        } else if (ra != rb && rb != rc && ra != rc) {
            const int lo = min(ra, min(rb, rc)), hi = max(ra, max(rb, rc)), mid = ra + rb + rc - lo - hi;
            k = ((uint64_t)lo << (2 * bits)) | ((uint64_t)mid << bits) | (uint64_t)hi;
        }
    }
    key[f] = k;
    val[f] = f;
}

// one thread per sorted position: the face's relabelled indices, and keep = not degenerate and the first of its run of equal keys
__global__ __launch_bounds__(TB) void k_mcf_out(const int64_t* __restrict__ faces, int F, const int32_t* __restrict__ rep, int bits,
                                                const uint64_t* __restrict__ key, const int* __restrict__ val, int64_t* __restrict__ out_faces,
                                                uint8_t* __restrict__ keep, int32_t* __restrict__ counts, const int* __restrict__ misc) {
    if (misc[F_BADIDX] | misc[F_BADREP]) return;
    const int p = blockIdx.x * blockDim.x + threadIdx.x, lane = threadIdx.x & 63;
    bool deg = false, dup = false;
    if (p < F) {
        const int f = val[p];
        const uint64_t k = key[p];
        deg = (k >> (3 * bits)) != 0ull;
        dup = !deg && p > 0 && key[p - 1] == k;
#pragma unroll
        for (int e = 0; e < 3; ++e) out_faces[3 * (size_t)f + e] = (int64_t)rep[faces[3 * (size_t)f + e]];
        keep[f] = (deg || dup) ? 0 : 1;
    }
    wave_count(&counts[C_DEGENERATE], deg, lane);
    wave_count(&counts[C_DUPLICATE], dup, lane);
    wave_count(&counts[C_KEPT], p < F && !deg && !dup, lane);
}

static bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

}  // namespace
}  // namespace pdhip

using namespace pdhip;

extern "C" int pdhip_weld_cells_axis(int Vn) { return Vn >= 1 && Vn <= MESH_MAX_V ? cells_axis_for(Vn) : 0; }

extern "C" int pdhip_weld_vertices(const float* vertices, int Vn, double tol, int32_t* rep, int32_t* counts, uint64_t* keys_a, uint64_t* keys_b,
                                   int32_t* vals_a, int32_t* vals_b, size_t sort_len, int32_t* hist, size_t hist_words, int32_t* cstart,
                                   size_t cstart_len, float* sorted_xyzi, size_t sorted_len, int32_t* parent, size_t parent_len, int32_t* misc,
                                   size_t misc_len, void* stream) {
#define WV_PTR(p) PD_REQUIRE(p, "pdhip_weld_vertices: null pointer (" #p ")")
    WV_PTR(vertices); WV_PTR(rep); WV_PTR(counts); WV_PTR(keys_a); WV_PTR(keys_b); WV_PTR(vals_a); WV_PTR(vals_b); WV_PTR(hist); WV_PTR(cstart);
    WV_PTR(sorted_xyzi); WV_PTR(parent); WV_PTR(misc);
#undef WV_PTR
    PD_REQUIRE(Vn >= 1 && Vn <= MESH_MAX_V, "pdhip_weld_vertices: Vn=%d: at least one vertex, at most 2^26", Vn);
    PD_REQUIRE(tol >= 0.0 && tol <= 1.7976931348623157e308, "pdhip_weld_vertices: tol=%g: a finite number >= 0", tol);
    const size_t nv = (size_t)Vn, cmax = (size_t)cells_axis_for(Vn);
#define WV_LEN(have, need, name) PD_REQUIRE((have) >= (need), "pdhip_weld_vertices: " name " holds %zu elements, Vn=%d needs %zu", (size_t)(have), Vn, (size_t)(need))
    WV_LEN(sort_len, nv, "keys_a / keys_b / vals_a / vals_b");
    WV_LEN(hist_words, hist_len(nv), "hist");
    WV_LEN(cstart_len, cmax * cmax * cmax + 1, "cstart");
    WV_LEN(sorted_len, nv, "sorted_xyzi");
    WV_LEN(parent_len, nv, "parent");
    WV_LEN(misc_len, (size_t)MISC_WORDS, "misc");
#undef WV_LEN
    PD_REQUIRE(aligned16(sorted_xyzi), "pdhip_weld_vertices: sorted_xyzi holds [Vn, 4] f32 rows read 16 bytes at a time: align it to 16 bytes");
    hipStream_t s = as_stream(stream);
    uint32_t* words = reinterpret_cast<uint32_t*>(misc);
    // a. the box and the finiteness of the vertices
    int rc = clear_boxes(words, 1, MISC_WORDS, s);
    if (rc) return rc;
    launch_point_box(vertices, Vn, words, s);
    k_uf_identity<<<cdiv(Vn, TB), TB, 0, s>>>(parent, Vn);
    PD_LAUNCH_CHECK();
    HostBox box[1];
    rc = read_boxes(words, box, s);
    if (rc) return rc;
    PD_REQUIRE(box[0].bad == 0, "pdhip_weld_vertices: %u vertex / vertices with a non-finite coordinate", box[0].bad);
    // b. the grid: the cell edge exceeds tol and the certificate's guard
    const double ext = box_extent(box[0].mn, box[0].mx);
    double mag = 0.0;
    for (int a = 0; a < 3; ++a) mag = std::max(mag, std::max(fabs(box[0].mn[a]), fabs(box[0].mx[a])));
    const double edge = 1.001 * tol + 4.0e-12 * mag;
    int C = (int)cmax;
    if (ext > 0.0 && edge > 0.0 && ext / edge < (double)C) C = std::max(1, (int)floor(ext / edge));
    const Grid3 g = grid_over(box[0].mn, ext, C);
    const int nc = g.C * g.C * g.C;
    SortBufs sb;
    sb.k[0] = keys_a; sb.k[1] = keys_b; sb.v[0] = vals_a; sb.v[1] = vals_b; sb.hist = hist;
    const int cur = sort_by_cell(sb, Vn, GridPointKey{vertices, g}, (unsigned long long)nc, cstart, s);
    float4* sp = reinterpret_cast<float4*>(sorted_xyzi);
    k_gather_xyzi<<<cdiv(Vn, CL_T), CL_T, 0, s>>>(sb.v[cur], vertices, Vn, sp);
    // c, d.
    k_mw_scan<<<cdiv(Vn, TB), TB, 0, s>>>(sp, Vn, cstart, g, tol * tol, parent, misc);
    k_mw_flatten<<<cdiv(Vn, TB), TB, 0, s>>>(parent, Vn, rep, misc);
    k_mw_counts<<<1, 1, 0, s>>>(misc, Vn, g.C, counts);
    PD_LAUNCH_CHECK();
    int h[MISC_WORDS];
    rc = read_words(misc, h, MISC_WORDS, s);
    if (rc) return rc;
    if (h[W_CAP]) {
        set_error("pdhip_weld_vertices: a union-find walk used up its budget of steps (word %d): the forest is not the descending one the kernels "
                  "keep; rep and counts are not valid", h[W_CAP]);
        return PDHIP_E_STATE;
    }
    return PDHIP_OK;
}

extern "C" int pdhip_clean_faces(const int64_t* faces, int F, const int32_t* rep, int Vn, int64_t* out_faces, uint8_t* keep, int32_t* counts,
                                 uint64_t* keys_a, uint64_t* keys_b, int32_t* vals_a, int32_t* vals_b, size_t sort_len, int32_t* hist,
                                 size_t hist_words, int32_t* misc, size_t misc_len, void* stream) {
#define CF_PTR(p) PD_REQUIRE(p, "pdhip_clean_faces: null pointer (" #p ")")
    CF_PTR(faces); CF_PTR(rep); CF_PTR(out_faces); CF_PTR(keep); CF_PTR(counts); CF_PTR(keys_a); CF_PTR(keys_b); CF_PTR(vals_a); CF_PTR(vals_b);
    CF_PTR(hist); CF_PTR(misc);
#undef CF_PTR
    PD_REQUIRE(Vn >= 1 && F >= 1, "pdhip_clean_faces: Vn=%d F=%d: at least one vertex and one face", Vn, F);
    PD_REQUIRE(Vn <= MAX_V_FACES, "pdhip_clean_faces: Vn=%d exceeds 2^21 = %d: the three indices of a face share one 64-bit sort key, 21 bits each", Vn,
               MAX_V_FACES);
    PD_REQUIRE(F <= MESH_MAX_F, "pdhip_clean_faces: F=%d exceeds the limit (F <= 2^23)", F);
    const size_t nf = (size_t)F;
#define CF_LEN(have, need, name) PD_REQUIRE((have) >= (need), "pdhip_clean_faces: " name " holds %zu elements, F=%d needs %zu", (size_t)(have), F, (size_t)(need))
    CF_LEN(sort_len, nf, "keys_a / keys_b / vals_a / vals_b");
    CF_LEN(hist_words, hist_len(nf), "hist");
    CF_LEN(misc_len, (size_t)MISC_WORDS, "misc");
#undef CF_LEN
    hipStream_t s = as_stream(stream);
    const int bits = std::max(1, bits_for((unsigned long long)(Vn - 1)));
    PD_HIP(hipMemsetAsync(misc, 0, MISC_WORDS * sizeof(int32_t), s));
    PD_HIP(hipMemsetAsync(counts, 0, 4 * sizeof(int32_t), s));
    SortBufs sb;
    sb.k[0] = keys_a; sb.k[1] = keys_b; sb.v[0] = vals_a; sb.v[1] = vals_b; sb.hist = hist;
    k_mcf_keys<<<cdiv(F, TB), TB, 0, s>>>(faces, F, Vn, rep, bits, sb.k[0], sb.v[0], misc);
    const int cur = radix_sort(sb, F, 3 * bits + 1, s);
    k_mcf_out<<<cdiv(F, TB), TB, 0, s>>>(faces, F, rep, bits, sb.k[cur], sb.v[cur], out_faces, keep, counts, misc);
    PD_LAUNCH_CHECK();
    int h[2];
    const int rc = read_words(misc, h, 2, s);
    if (rc) return rc;
    PD_REQUIRE(h[F_BADIDX] == 0, "pdhip_clean_faces: %d face(s) with an index outside [0, Vn=%d)", h[F_BADIDX], Vn);
    PD_REQUIRE(h[F_BADREP] == 0, "pdhip_clean_faces: %d face(s) whose vertices' rep lies outside [0, Vn=%d): rep is not pdhip_weld_vertices' output "
               "for these vertices", h[F_BADREP], Vn);
    return PDHIP_OK;
}
