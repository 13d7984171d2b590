// Connected components of an indexed triangle list, and the compaction of a mesh to a subset of its faces (include/pdhip.h has the
// contracts; DESIGN.md section 6, "Connected components").  No reference counterpart: the reference reconstructs by POCO and never meets
// the floating pieces a Poisson solve leaves; MeshLab's "Remove isolated pieces" is the filter built on top (mesh_components.py).
//
// Components: the lock-free union-find of union_find.h over the vertices (its header has the invariant: the partition AND its labels are
// functions of the mesh alone).  Four launches:
//   k_mc_hook      one thread per face: atomicMin(parent[v], smallest index of the face) for its vertices -- a first forest for free
//   k_mc_compress  one thread per vertex: parent[v] = the root of that forest (walk_root; the roots themselves are not written, so their
//                  hot lines stay in the caches)
//   k_mc_union     one thread per face: nothing to do when its three vertices show one parent (nearly every face of a mesh numbered with
//                  some locality); otherwise unite (a, b) and (b, c)
//   k_mc_flatten   one thread per vertex: root[v], read-only on parent[]
// The budgets are 2 Vn + 64 steps per face and Vn per vertex; M_CAP says if a walk used one up.
#include "mesh_common.h"
#include "union_find.h"

namespace pdhip {
namespace {

constexpr int TB = 256;
constexpr int SMALL_SCAN = 16384;                                  // up to here the one-workgroup scan of radix_sort.h: one launch, not three
enum { M_ERR = 0, M_CAP, M_C, M_NREF, M_WORDS = 8 };
constexpr int MISC_LINE = 256 / sizeof(int);                        // carve_compact: misc as one whole 256-byte line (M_WORDS of it used)
enum { ERR_INDEX = 1, ERR_NONFINITE = 2 };

static void scan_flags(const int* in, int* out, int n, int* tsum, int* toff, hipStream_t s) {
    if (n <= SMALL_SCAN) k_scan<int><<<1, SC_T, 0, s>>>(in, out, n, 1);
    else scan_exclusive(in, out, n, tsum, toff, s);
}

// ---- union-find
__global__ void k_mc_init(int* __restrict__ parent, int* __restrict__ ref, int Vn, int* __restrict__ misc) {
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v < M_WORDS) misc[v] = 0;
    if (v < Vn) { parent[v] = v; ref[v] = 0; }
}

// a face index outside [0, Vn) sets ERR_INDEX (and the face touches nothing); otherwise the face's vertices are flagged and hooked below
// its smallest one
__global__ void k_mc_hook(const int64_t* __restrict__ faces, int F, int Vn, int* __restrict__ parent, int* __restrict__ ref, int* __restrict__ misc) {
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= F) return;
    const int64_t a = faces[3 * (size_t)f], b = faces[3 * (size_t)f + 1], c = faces[3 * (size_t)f + 2];
    if (!(index_ok(a, Vn) && index_ok(b, Vn) && index_ok(c, Vn))) { atomicOr(&misc[M_ERR], ERR_INDEX); return; }
    ref[a] = 1; ref[b] = 1; ref[c] = 1;
    const int m = (int)(a < b ? (a < c ? a : c) : (b < c ? b : c));
    if (a != m) atomicMin(&parent[a], m);
    if (b != m) atomicMin(&parent[b], m);
    if (c != m) atomicMin(&parent[c], m);
}

__global__ void k_mc_compress(int* parent, int Vn, int* __restrict__ misc) {
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= Vn || misc[M_ERR]) return;
    int steps = Vn;                                                // (a strictly decreasing walk has at most Vn - 1 steps)
    const int r = walk_root(parent, v, steps);
    if (r < 0) atomicOr(&misc[M_CAP], 4);
    else if (r != v) parent[v] = r;
}

__global__ __launch_bounds__(TB) void k_mc_union(const int64_t* __restrict__ faces, int F, int Vn, int* parent, int* __restrict__ misc) {
    if (misc[M_ERR] | misc[M_CAP]) return;                         // (an index outside [0, Vn) must not reach parent[])
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= F) return;
    const int a = (int)faces[3 * (size_t)f], b = (int)faces[3 * (size_t)f + 1], c = (int)faces[3 * (size_t)f + 2];
    const int pa = ld_agent(parent + a), pb = ld_agent(parent + b), pc = ld_agent(parent + c);
    if (pa == pb && pb == pc) return;                              // one ancestor in common: one tree already
    long long budget = 2ll * Vn + 64;
    int r = unite(parent, find_root(parent, pa, budget), find_root(parent, pb, budget), budget);
    if (r >= 0 && pc != pa && pc != pb) r = unite(parent, r, find_root(parent, pc, budget), budget);
    if (r < 0) atomicOr(&misc[M_CAP], 1);
}

// root[v] = the component's smallest index (parent[] is read only here: equal bytes on repeats); isroot[v] = v is a referenced root.
// P != nullptr (boxes asked for): a referenced vertex that is not finite sets ERR_NONFINITE
__global__ void k_mc_flatten(const int* __restrict__ parent, const int* __restrict__ ref, const float* __restrict__ P, int Vn, int* __restrict__ root,
                             int* __restrict__ isroot, int* __restrict__ misc) {
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= Vn) return;
    int r = v, steps = Vn;
    if (!(misc[M_ERR] & ERR_INDEX) && !misc[M_CAP]) {
        r = walk_root(parent, v, steps);
        if (r < 0) { atomicOr(&misc[M_CAP], 2); r = v; }
        if (P && ref[v] && !finite3(P[3 * (size_t)v], P[3 * (size_t)v + 1], P[3 * (size_t)v + 2])) atomicOr(&misc[M_ERR], ERR_NONFINITE);
    }
    root[v] = r;
    isroot[v] = (ref[v] && r == v) ? 1 : 0;
}

// ---- outputs.  Components 0 .. min(C, cap) - 1 have entries in the per-component arrays
__global__ void k_mc_comp_init(const int* __restrict__ isroot, const int* __restrict__ cid, int Vn, int cap, int32_t* __restrict__ comp_vertices,
                               int32_t* __restrict__ comp_faces, uint32_t* __restrict__ box, int* __restrict__ misc) {
    if (misc[M_ERR] | misc[M_CAP]) return;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const int C = cid[Vn - 1] + isroot[Vn - 1];
    if (i == 0) misc[M_C] = C;
    if (i >= cap || i >= C) return;
    comp_vertices[i] = 0;
    comp_faces[i] = 0;
    if (box) {
#pragma unroll
        for (int k = 0; k < 3; ++k) { box[6 * (size_t)i + k] = 0xffffffffu; box[6 * (size_t)i + 3 + k] = 0u; }
    }
}

__device__ __forceinline__ uint32_t wave_min(uint32_t x) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) x = min(x, (uint32_t)__shfl_xor((int)x, o));
    return x;
}
__device__ __forceinline__ uint32_t wave_max(uint32_t x) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) x = max(x, (uint32_t)__shfl_xor((int)x, o));
    return x;
}

// The active lanes of a wave add one each to cnt[id] and, with box, their point (ordered encoding o) to the box of id: one round per
// DISTINCT id of the wave (a mesh's neighbouring vertices and faces mostly share one), its first lane adding for all of them -- a million
// single adds to one word would queue up at about 11 ns each.  Every lane of the wave calls this (the loop is wave-uniform)
__device__ __forceinline__ void wave_accumulate(int32_t* __restrict__ cnt, uint32_t* __restrict__ box, int id, bool active, const uint32_t (&o)[3], int lane) {
    unsigned long long todo = __ballot(active);
    while (todo) {
        const int leader = __ffsll((long long)todo) - 1;
        const int lid = __shfl(id, leader);
        const bool mine = active && id == lid;
        const unsigned long long same = __ballot(mine);
        const int n = __popcll(same);
        if (!box) {
            if (lane == leader) atomicAdd(&cnt[lid], n);
        } else if (n >= 8) {
            uint32_t lo[3], hi[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) { lo[k] = wave_min(mine ? o[k] : 0xffffffffu); hi[k] = wave_max(mine ? o[k] : 0u); }
            if (lane == leader) {
                atomicAdd(&cnt[lid], n);
#pragma unroll
                for (int k = 0; k < 3; ++k) { atomicMin(&box[6 * (size_t)lid + k], lo[k]); atomicMax(&box[6 * (size_t)lid + 3 + k], hi[k]); }
            }
        } else if (mine) {
            atomicAdd(&cnt[lid], 1);
#pragma unroll
            for (int k = 0; k < 3; ++k) { atomicMin(&box[6 * (size_t)lid + k], o[k]); atomicMax(&box[6 * (size_t)lid + 3 + k], o[k]); }
        }
        todo &= ~same;
    }
}

__global__ __launch_bounds__(TB) void k_mc_vertex_out(const float* __restrict__ P, const int* __restrict__ ref, const int* __restrict__ root,
                                                      const int* __restrict__ cid, int Vn, int cap, int32_t* __restrict__ vertex_comp,
                                                      int32_t* __restrict__ comp_root, int32_t* __restrict__ comp_vertices, uint32_t* __restrict__ box,
                                                      int* __restrict__ misc) {
    if (misc[M_ERR] | misc[M_CAP]) return;
    const int v = blockIdx.x * blockDim.x + threadIdx.x, lane = threadIdx.x & 63;
    const bool in = v < Vn, r = in && ref[v] != 0;
    int id = -1;
    if (r) {
        const int rt = root[v];
        id = cid[rt];
        if (rt == v && id < cap) comp_root[id] = v;
    }
    if (in) vertex_comp[v] = id;
    const int nref = __syncthreads_count(r);
    if (threadIdx.x == 0 && nref) atomicAdd(&misc[M_NREF], nref);
    const bool cnt = r && id < cap;
    uint32_t o[3] = {0u, 0u, 0u};
    if (cnt && box) {
#pragma unroll
        for (int k = 0; k < 3; ++k) o[k] = f2ord(P[3 * (size_t)v + k]);
    }
    wave_accumulate(comp_vertices, box, id, cnt, o, lane);
}

// face_comp and the faces per component; the first 6 min(C, cap) threads also bring the boxes back from the ordered encoding, in place (the
// launch before this one finished them), and thread 0 writes counts = C, referenced, unreferenced, 0.  The grid covers max(F, 6 cap) threads
__global__ __launch_bounds__(TB) void k_mc_face_out(const int64_t* __restrict__ faces, int F, int Vn, const int* __restrict__ root,
                                                    const int* __restrict__ cid, int cap, int32_t* __restrict__ face_comp, int32_t* __restrict__ comp_faces,
                                                    uint32_t* __restrict__ box, int32_t* __restrict__ counts, const int* __restrict__ misc) {
    if (misc[M_ERR] | misc[M_CAP]) return;
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const int lane = threadIdx.x & 63, C = misc[M_C];
    if (i == 0) { counts[0] = C; counts[1] = misc[M_NREF]; counts[2] = Vn - misc[M_NREF]; counts[3] = 0; }
    if (box && i < 6ll * (C < cap ? C : cap)) box[i] = __float_as_uint(ord2f(box[i]));
    const bool in = i < F;
    int id = -1;
    if (in) {
        id = cid[root[faces[3 * (size_t)i]]];
        face_comp[i] = id;
    }
    const uint32_t none[3] = {0u, 0u, 0u};
    wave_accumulate(comp_faces, nullptr, id, in && id < cap, none, lane);
}

__global__ void k_mc_empty(int Vn, int32_t* __restrict__ vertex_comp, int32_t* __restrict__ counts) {
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v < Vn) vertex_comp[v] = -1;
    if (v == 0) { counts[0] = 0; counts[1] = 0; counts[2] = Vn; counts[3] = 0; }
}

struct CompWs {
    int *parent, *ref, *root, *isroot, *cid, *tsum, *toff, *misc;
};
static size_t carve_comp(CompWs& w, void* base, int Vn, int F) {
    const size_t nv = (size_t)Vn;
    Carve c{static_cast<char*>(base), 0};
    w.parent = c.take<int>(nv); w.ref = c.take<int>(nv); w.root = c.take<int>(nv); w.isroot = c.take<int>(nv); w.cid = c.take<int>(nv);
    w.tsum = c.take<int>(scan_tiles(nv)); w.toff = c.take<int>(scan_tiles(nv)); w.misc = c.take<int>(M_WORDS);
    (void)F;                                                       // (the faces are read in place: nothing per face)
    return c.off + 256;
}

// ---- compaction
// fflag[f] = keep[f] != 0; the kept faces flag their vertices; a face index outside [0, Vn) (in a dropped face too) sets ERR_INDEX
__global__ void k_mc_pack_mark(const int64_t* __restrict__ faces, int F, int Vn, const uint8_t* __restrict__ keep, int* __restrict__ fflag,
                               int* __restrict__ vflag, int* __restrict__ misc) {
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= F) return;
    const int64_t a = faces[3 * (size_t)f], b = faces[3 * (size_t)f + 1], c = faces[3 * (size_t)f + 2];
    const bool k = keep[f] != 0;
    fflag[f] = k ? 1 : 0;
    if (!(index_ok(a, Vn) && index_ok(b, Vn) && index_ok(c, Vn))) { atomicOr(&misc[M_ERR], ERR_INDEX); return; }
    if (k) { vflag[a] = 1; vflag[b] = 1; vflag[c] = 1; }
}

__global__ void k_mc_pack_vertices(const float* __restrict__ P, const float* __restrict__ C, const int* __restrict__ vflag, const int* __restrict__ vexcl,
                                   int Vn, int F, float* __restrict__ out_v, float* __restrict__ out_c, int32_t* __restrict__ vmap,
                                   int32_t* __restrict__ counts, const int* __restrict__ misc) {
    if (misc[M_ERR]) return;
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= Vn) return;
    const int keep = vflag[v], n = vexcl[v];
    if (v == Vn - 1) {
        counts[0] = n + keep; counts[2] = 0; counts[3] = 0;
        if (F == 0) counts[1] = 0;
    }
    if (vmap) vmap[v] = keep ? n : -1;
    if (!keep) return;
    const size_t d = 3 * (size_t)n, s = 3 * (size_t)v;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        out_v[d + k] = P[s + k];
        if (out_c) out_c[d + k] = C[s + k];
    }
}

__global__ void k_mc_pack_faces(const int64_t* __restrict__ faces, int F, const int* __restrict__ fflag, const int* __restrict__ fexcl,
                                const int* __restrict__ vexcl, int64_t* __restrict__ out_f, int32_t* __restrict__ counts, const int* __restrict__ misc) {
    if (misc[M_ERR]) return;
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= F) return;
    if (f == F - 1) counts[1] = fexcl[f] + fflag[f];
    if (!fflag[f]) return;
    const size_t d = 3 * (size_t)fexcl[f], s = 3 * (size_t)f;
#pragma unroll
    for (int k = 0; k < 3; ++k) out_f[d + k] = (int64_t)vexcl[faces[s + k]];
}

struct CompactWs {
    int *misc, *vflag, *vexcl, *fflag, *fexcl, *tsum, *toff;
    size_t zero_bytes;                                             // misc and vflag lie back to back: one memset clears both
};
static size_t carve_compact(CompactWs& w, void* base, int Vn, int F) {
    const size_t nv = (size_t)Vn, nf = (size_t)F;
    Carve c{static_cast<char*>(base), 0};
    w.misc = c.take<int>(MISC_LINE); w.vflag = c.take<int>(nv);      // (a whole line: the one fill below clears misc and vflag, and what lies between)
    w.zero_bytes = c.off;
    w.vexcl = c.take<int>(nv); w.fflag = c.take<int>(nf); w.fexcl = c.take<int>(nf);
    const size_t tiles = scan_tiles(nv > nf ? nv : nf);
    w.tsum = c.take<int>(tiles); w.toff = c.take<int>(tiles);
    return c.off + 256;
}

static bool sizes_ok(int Vn, int F) { return Vn >= 1 && F >= 0 && Vn <= MESH_MAX_V && F <= MESH_MAX_F; }

}  // namespace
}  // namespace pdhip

using namespace pdhip;

extern "C" size_t pdhip_mesh_components_workspace_bytes(int Vn, int F) {
    if (!sizes_ok(Vn, F)) return 0;
    CompWs w;
    return carve_comp(w, nullptr, Vn, F);
}

extern "C" int pdhip_mesh_components(const int64_t* faces, int F, const float* vertices, int Vn, int32_t* vertex_comp, int32_t* face_comp,
                                     int32_t* comp_root, int32_t* comp_vertices, int32_t* comp_faces, float* comp_box, int comp_capacity,
                                     int32_t* counts, void* ws, void* stream) {
#define MC_PTR(p) PD_REQUIRE(p, "pdhip_mesh_components: null pointer (" #p ")")
    MC_PTR(faces); MC_PTR(vertex_comp); MC_PTR(face_comp); MC_PTR(comp_root); MC_PTR(comp_vertices); MC_PTR(comp_faces); MC_PTR(counts); MC_PTR(ws);
#undef MC_PTR
    PD_REQUIRE(!comp_box || vertices, "pdhip_mesh_components: null pointer (vertices): the boxes (comp_box) are taken over the vertices");
    PD_REQUIRE(Vn >= 1 && F >= 0, "pdhip_mesh_components: Vn=%d F=%d: at least one vertex, no negative face count", Vn, F);
    PD_REQUIRE(Vn <= MESH_MAX_V && F <= MESH_MAX_F, "pdhip_mesh_components: Vn=%d F=%d exceed the limits (Vn <= 2^26, F <= 2^23)", Vn, F);
    PD_REQUIRE(comp_capacity >= 0, "pdhip_mesh_components: comp_capacity=%d is negative", comp_capacity);
    hipStream_t s = as_stream(stream);
    if (F == 0) {                                                   // no face: no component, every vertex unreferenced
        k_mc_empty<<<cdiv(Vn, TB), TB, 0, s>>>(Vn, vertex_comp, counts);
        PD_LAUNCH_CHECK();
        return PDHIP_OK;
    }
    CompWs w;
    carve_comp(w, ws, Vn, F);
    const int gv = cdiv(Vn, TB), gf = cdiv(F, TB), cap = comp_capacity;
    const long long decode = comp_box ? 6ll * cap : 0;
    uint32_t* box = reinterpret_cast<uint32_t*>(comp_box);
    k_mc_init<<<gv, TB, 0, s>>>(w.parent, w.ref, Vn, w.misc);
    k_mc_hook<<<gf, TB, 0, s>>>(faces, F, Vn, w.parent, w.ref, w.misc);
    k_mc_compress<<<gv, TB, 0, s>>>(w.parent, Vn, w.misc);
    k_mc_union<<<gf, TB, 0, s>>>(faces, F, Vn, w.parent, w.misc);
    k_mc_flatten<<<gv, TB, 0, s>>>(w.parent, w.ref, comp_box ? vertices : nullptr, Vn, w.root, w.isroot, w.misc);
    scan_flags(w.isroot, w.cid, Vn, w.tsum, w.toff, s);
    k_mc_comp_init<<<cdiv(cap > 0 ? cap : 1, TB), TB, 0, s>>>(w.isroot, w.cid, Vn, cap, comp_vertices, comp_faces, box, w.misc);
    k_mc_vertex_out<<<gv, TB, 0, s>>>(vertices, w.ref, w.root, w.cid, Vn, cap, vertex_comp, comp_root, comp_vertices, box, w.misc);
    k_mc_face_out<<<cdiv(decode > F ? decode : F, TB), TB, 0, s>>>(faces, F, Vn, w.root, w.cid, cap, face_comp, comp_faces, box, counts, w.misc);
    PD_LAUNCH_CHECK();
    int h[M_WORDS];
    const int rc = read_words(w.misc, h, M_WORDS, s);
    if (rc != PDHIP_OK) return rc;
    PD_REQUIRE(!(h[M_ERR] & ERR_INDEX), "pdhip_mesh_components: a face index outside [0, Vn=%d)", Vn);
    PD_REQUIRE(!(h[M_ERR] & ERR_NONFINITE), "pdhip_mesh_components: a referenced vertex is not finite (the boxes need finite coordinates)");
    if (h[M_CAP]) {
        set_error("pdhip_mesh_components: a union-find walk used up its budget of steps (word %d): the forest is not the descending one the "
                  "kernels keep; nothing was written", h[M_CAP]);
        return PDHIP_E_STATE;
    }
    return PDHIP_OK;
}

extern "C" size_t pdhip_compact_mesh_workspace_bytes(int Vn, int F) {
    if (!sizes_ok(Vn, F)) return 0;
    CompactWs w;
    return carve_compact(w, nullptr, Vn, F);
}

extern "C" int pdhip_compact_mesh(const float* vertices, int Vn, const int64_t* faces, int F, const float* colors, const uint8_t* face_keep,
                                  float* out_vertices, int64_t* out_faces, float* out_colors, int32_t* vertex_map, int32_t* counts, void* ws,
                                  void* stream) {
#define CM_PTR(p) PD_REQUIRE(p, "pdhip_compact_mesh: null pointer (" #p ")")
    CM_PTR(vertices); CM_PTR(faces); CM_PTR(face_keep); CM_PTR(out_vertices); CM_PTR(out_faces); CM_PTR(counts); CM_PTR(ws);
#undef CM_PTR
    PD_REQUIRE((colors != nullptr) == (out_colors != nullptr), "pdhip_compact_mesh: colors and out_colors go together");
    PD_REQUIRE(Vn >= 1 && F >= 0, "pdhip_compact_mesh: Vn=%d F=%d: at least one vertex, no negative face count", Vn, F);
    PD_REQUIRE(Vn <= MESH_MAX_V && F <= MESH_MAX_F, "pdhip_compact_mesh: Vn=%d F=%d exceed the limits (Vn <= 2^26, F <= 2^23)", Vn, F);
    hipStream_t s = as_stream(stream);
    CompactWs w;
    carve_compact(w, ws, Vn, F);
    const int gv = cdiv(Vn, TB), gf = cdiv(F, TB);
    PD_HIP(hipMemsetAsync(w.misc, 0, w.zero_bytes, s));
    if (F > 0) {
        k_mc_pack_mark<<<gf, TB, 0, s>>>(faces, F, Vn, face_keep, w.fflag, w.vflag, w.misc);
        scan_flags(w.fflag, w.fexcl, F, w.tsum, w.toff, s);
    }
    scan_flags(w.vflag, w.vexcl, Vn, w.tsum, w.toff, s);
    k_mc_pack_vertices<<<gv, TB, 0, s>>>(vertices, colors, w.vflag, w.vexcl, Vn, F, out_vertices, out_colors, vertex_map, counts, w.misc);
    if (F > 0) k_mc_pack_faces<<<gf, TB, 0, s>>>(faces, F, w.fflag, w.fexcl, w.vexcl, out_faces, counts, w.misc);
    PD_LAUNCH_CHECK();
    int h[M_WORDS];
    const int rc = read_words(w.misc, h, M_WORDS, s);
    if (rc != PDHIP_OK) return rc;
    PD_REQUIRE(!(h[M_ERR] & ERR_INDEX), "pdhip_compact_mesh: a face index outside [0, Vn=%d)", Vn);
    return PDHIP_OK;
}
