// Coherent orientation of an indexed triangle list, patch by patch, closed patches outward (include/pdhip.h has the contract and the definitions in
// full; DESIGN.md section 6, "Orientation").  The step behind mesh_clean.hip in the chain for meshes that users supply: cleaning repairs the
// indexing, this repairs the winding, which pdhip_simplify_mesh (a consistently oriented 2-manifold), the unwrap (charts by the signed normal axis)
// and the renderers (shading by the face normal) all rely on.  Counterparts: trimesh.repair.fix_normals, MeshLab's "Re-Orient all faces coherently".
// The reference gets it from those loaders and has no code of its own for it.
//
// The launches, in order (every kernel after the first returns at once when the first found a face index outside [0, Vn) or a referenced vertex
// that is not finite, so the outputs stay as the caller left them):
//   k_mo_keys        per face: the checks; its three half-edges as (pair_key(lo, hi), (3 f + k) << 1 | (a > b)); word[f] = f << 1; a face with two
//                    equal indices gets the key `none` = Vn * Vn three times (it sorts last and starts no run) and the bit FB_DEG
//   radix_sort       the 3 F keys, stably
//   k_mo_edges       per sorted position, the heads of runs only (a head reads its one or two successors itself, by index and against the end:
//                    nothing assumes that neighbouring lanes share a run): 1 half-edge = boundary, FB_OPEN on its face; 2 = manifold, the two faces
//                    are parity-united with e = (d1 == d2); 3 or more = non-manifold, FB_OPEN on every face of the run
//   k_mo_flatten     per face: root, FB_REL (the parity to the root), isroot; read-only on word[].  Then the shared scan: isroot -> patch ids
//   k_mo_patch_init  per patch: the accumulators cleared; patch_root
//   k_mo_recheck     per manifold edge again: rel[fa] ^ rel[fb] != e flags the patch non-orientable (union_find.h: in every spanning forest of such a
//                    patch some edge disagrees, in none of an orientable one)
//   k_mo_face_stats  per face: faces and rel = 1 faces per patch, the open bit, the box over the ordered bits of the coordinates (f2ord)
//   k_mo_vol         per face of a patch the volume rule applies to: (1 - 2 rel) det(A, B, C) on the 12-bit grid of the patch's own box, 64-bit
//                    integer adds (a wave whose faces share a patch adds once)
//   k_mo_decide      per patch: c, the flags, the flipped count;  k_mo_write  per face: out_faces, flip, face_patch; counts
// Integer atomics only (or, add, min, max: all commutative and exact), zero scratch; two calls give equal bytes.  Every temporary is a typed array of
// the caller's.  A union-find walk spends a budget of 2 F + 64 steps; M_CAP says if one ran out.
#include "mesh_common.h"
#include "union_find.h"

namespace pdhip {
namespace {

constexpr int TB = 256;
constexpr int SMALL_SCAN = 16384;                                  // up to here the one-workgroup scan of radix_sort.h: one launch, not three
constexpr int MISC_WORDS = 64;                                     // one 256-byte line
constexpr int FACE_ARRAYS = 5;                                     // word, root, isroot, pid, fbits: F words each of face_tmp
enum { M_ERR = 0, M_CAP, M_P, M_FLIPPED, M_NONORIENT, M_INCOHERENT, M_BOUNDARY, M_NONMANIFOLD, M_DEGENERATE };
enum { ERR_INDEX = 1, ERR_NONFINITE = 2 };
enum { FB_REL = 1, FB_OPEN = 2, FB_DEG = 4 };
enum { PF_CLOSED = 1, PF_NONORIENT = 2, PF_VOLUME = 4, PF_COMPLEMENT = 8, PF_OPEN_TMP = 16 };      // (PF_OPEN_TMP: between face_stats and decide only)
constexpr int GRID_MAX = 4095;                                     // the volume rule's grid: 12 bits per axis, |det| < 2^39

static size_t hist_len(size_t n) { return 2 * 256 * (size_t)cdiv((long long)n, RS_TILE); }

__device__ __forceinline__ int face_of(int val) { return (val >> 1) / 3; }

__global__ __launch_bounds__(TB) void k_mo_keys(const int64_t* __restrict__ faces, int F, const float* __restrict__ P, int Vn, uint64_t* __restrict__ key,
                                                int* __restrict__ val, int* __restrict__ word, int* __restrict__ fbits, int* __restrict__ misc) {
    const int f = blockIdx.x * blockDim.x + threadIdx.x, lane = threadIdx.x & 63;
    bool deg = false;
    if (f < F) {
        const int64_t v[3] = {faces[3 * (size_t)f], faces[3 * (size_t)f + 1], faces[3 * (size_t)f + 2]};
        const uint64_t none = (uint64_t)Vn * (uint64_t)Vn;
        uint64_t k[3] = {none, none, none};
        int d[3] = {0, 0, 0};
        if (!(index_ok(v[0], Vn) && index_ok(v[1], Vn) && index_ok(v[2], Vn))) {
            atomicOr(&misc[M_ERR], ERR_INDEX);
        } else {
            bool fin = true;
#pragma unroll
            for (int e = 0; e < 3; ++e) fin = fin && finite3(P[3 * (size_t)v[e]], P[3 * (size_t)v[e] + 1], P[3 * (size_t)v[e] + 2]);
            if (!fin) atomicOr(&misc[M_ERR], ERR_NONFINITE);
            deg = v[0] == v[1] || v[1] == v[2] || v[0] == v[2];
            if (!deg) {
#pragma unroll
                for (int e = 0; e < 3; ++e) {
                    const uint64_t a = (uint64_t)v[e], b = (uint64_t)v[(e + 1) % 3];
                    k[e] = a < b ? pair_key(a, b, Vn) : pair_key(b, a, Vn);
                    d[e] = a > b ? 1 : 0;
                }
            }
        }
#pragma unroll
        for (int e = 0; e < 3; ++e) {
            key[3 * (size_t)f + e] = k[e];
            val[3 * (size_t)f + e] = ((3 * f + e) << 1) | d[e];
        }
        word[f] = f << 1;
        fbits[f] = deg ? FB_DEG : 0;
    }
    wave_count(&misc[M_DEGENERATE], deg, lane);
}

// the run that starts at sorted position p: 0 when p starts none, else min(its length, 3)
__device__ __forceinline__ int run_at(const uint64_t* __restrict__ key, int n, uint64_t none, int p) {
    const uint64_t k = key[p];
    if (k == none || (p > 0 && key[p - 1] == k)) return 0;
    if (!(p + 1 < n && key[p + 1] == k)) return 1;
    return (p + 2 < n && key[p + 2] == k) ? 3 : 2;
}

__global__ __launch_bounds__(TB) void k_mo_edges(const uint64_t* __restrict__ key, const int* __restrict__ val, int n, int F, uint64_t none, int* word,
                                                 int* __restrict__ fbits, int* __restrict__ misc) {
    if (misc[M_ERR]) return;
    const int p = blockIdx.x * blockDim.x + threadIdx.x, lane = threadIdx.x & 63;
    const int run = p < n ? run_at(key, n, none, p) : 0;
    bool inco = false, spent = false;
    if (run == 1) {
        atomicOr(&fbits[face_of(val[p])], FB_OPEN);
    } else if (run == 2) {
        const int va = val[p], vb = val[p + 1];
        const int e = ((va ^ vb) & 1) ^ 1;                         // the same direction twice: one of the two faces must flip
        inco = e != 0;
        long long budget = 2ll * F + 64;
        int pa, pb;
        const int ra = find_root_parity(word, face_of(va), pa, budget), rb = find_root_parity(word, face_of(vb), pb, budget);
        spent = unite_parity(word, ra, rb, pa ^ pb ^ e, budget) < 0;
    } else if (run == 3) {
        const uint64_t k = key[p];
        for (int q = p; q < n && key[q] == k; ++q) atomicOr(&fbits[face_of(val[q])], FB_OPEN);
    }
    if (spent) atomicOr(&misc[M_CAP], 1);
    wave_count(&misc[M_BOUNDARY], run == 1, lane);
    wave_count(&misc[M_INCOHERENT], inco, lane);
    wave_count(&misc[M_NONMANIFOLD], run == 3, lane);
}

__global__ __launch_bounds__(TB) void k_mo_flatten(const int* __restrict__ word, int F, int* __restrict__ root, int* __restrict__ isroot,
                                                   int* __restrict__ fbits, int* __restrict__ misc) {
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= F) return;
    int r = f, par = 0;
    if (!(misc[M_ERR] | misc[M_CAP])) {
        int steps = F;
        r = walk_root_parity(word, f, par, steps);
        if (r < 0) { atomicOr(&misc[M_CAP], 2); r = f; par = 0; }
    }
    const int bits = fbits[f];
    root[f] = r;
    fbits[f] = bits | (par ? FB_REL : 0);
    isroot[f] = (!(bits & FB_DEG) && r == f) ? 1 : 0;
}

__global__ void k_mo_patch_init(const int* __restrict__ isroot, const int* __restrict__ pid, int F, int32_t* __restrict__ patch_root,
                                int32_t* __restrict__ patch_faces, int32_t* __restrict__ patch_rel1, int32_t* __restrict__ patch_flags,
                                unsigned long long* __restrict__ patch_vol, uint32_t* __restrict__ box, int* __restrict__ misc) {
    if (misc[M_ERR] | misc[M_CAP]) return;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const int P = pid[F - 1] + isroot[F - 1];
    if (i == 0) misc[M_P] = P;
    if (i < F && isroot[i]) patch_root[pid[i]] = i;
    if (i >= P) return;
    patch_faces[i] = 0; patch_rel1[i] = 0; patch_flags[i] = 0; patch_vol[i] = 0ull;
#pragma unroll
    for (int k = 0; k < 3; ++k) { box[6 * (size_t)i + k] = 0xffffffffu; box[6 * (size_t)i + 3 + k] = 0u; }
}

__global__ __launch_bounds__(TB) void k_mo_recheck(const uint64_t* __restrict__ key, const int* __restrict__ val, int n, uint64_t none,
                                                   const int* __restrict__ root, const int* __restrict__ pid, const int* __restrict__ fbits,
                                                   int32_t* __restrict__ patch_flags, const int* __restrict__ misc) {
    if (misc[M_ERR] | misc[M_CAP]) return;
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n || run_at(key, n, none, p) != 2) return;
    const int va = val[p], vb = val[p + 1], fa = face_of(va), fb = face_of(vb);
    const int e = ((va ^ vb) & 1) ^ 1;
    if (((fbits[fa] ^ fbits[fb]) & FB_REL) != e) atomicOr(&patch_flags[pid[root[fa]]], PF_NONORIENT);
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
__device__ __forceinline__ long long wave_sum(long long x) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const int lo = __shfl_xor((int)(x & 0xffffffffll), o), hi = __shfl_xor((int)(x >> 32), o);
        x += (long long)(((unsigned long long)(uint32_t)hi << 32) | (unsigned long long)(uint32_t)lo);
    }
    return x;
}

// the patch of face f, -1 for a degenerate face and for a thread beyond F
__device__ __forceinline__ int patch_of(int f, int F, const int* __restrict__ root, const int* __restrict__ pid, const int* __restrict__ fbits, int& bits) {
    bits = f < F ? fbits[f] : FB_DEG;
    return (bits & FB_DEG) ? -1 : pid[root[f]];
}

// One round per DISTINCT patch of the wave (neighbouring faces of a mesh mostly share one), its first lane adding for all of them, as
// mesh_components.hip's wave_accumulate does.  Every lane of the wave runs this kernel to its end (the loop is wave-uniform)
__global__ __launch_bounds__(TB) void k_mo_face_stats(const int64_t* __restrict__ faces, int F, const float* __restrict__ P, const int* __restrict__ root,
                                                      const int* __restrict__ pid, const int* __restrict__ fbits, int32_t* __restrict__ patch_faces,
                                                      int32_t* __restrict__ patch_rel1, int32_t* __restrict__ patch_flags, uint32_t* __restrict__ box,
                                                      const int* __restrict__ misc) {
    if (misc[M_ERR] | misc[M_CAP]) return;
    const int f = blockIdx.x * blockDim.x + threadIdx.x, lane = threadIdx.x & 63;
    int bits;
    const int id = patch_of(f, F, root, pid, fbits, bits);
    const bool active = id >= 0;
    uint32_t lo[3] = {0xffffffffu, 0xffffffffu, 0xffffffffu}, hi[3] = {0u, 0u, 0u};
    if (active) {
#pragma unroll
        for (int e = 0; e < 3; ++e) {
            const size_t v = (size_t)faces[3 * (size_t)f + e];
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const uint32_t o = f2ord(P[3 * v + k]);
                lo[k] = min(lo[k], o); hi[k] = max(hi[k], o);
            }
        }
    }
    unsigned long long todo = __ballot(active);
    while (todo) {
        const int leader = __ffsll((long long)todo) - 1;
        const int lid = __shfl(id, leader);
        const bool mine = active && id == lid;
        const unsigned long long same = __ballot(mine);
        const int n = __popcll(same), n1 = __popcll(__ballot(mine && (bits & FB_REL)));
        const bool open = __ballot(mine && (bits & FB_OPEN)) != 0ull;
        if (n >= 8) {
            uint32_t wl[3], wh[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) { wl[k] = wave_min(mine ? lo[k] : 0xffffffffu); wh[k] = wave_max(mine ? hi[k] : 0u); }
            if (lane == leader) {
#pragma unroll
                for (int k = 0; k < 3; ++k) { atomicMin(&box[6 * (size_t)lid + k], wl[k]); atomicMax(&box[6 * (size_t)lid + 3 + k], wh[k]); }
            }
        } else if (mine) {
#pragma unroll
            for (int k = 0; k < 3; ++k) { atomicMin(&box[6 * (size_t)lid + k], lo[k]); atomicMax(&box[6 * (size_t)lid + 3 + k], hi[k]); }
        }
        if (lane == leader) {
            atomicAdd(&patch_faces[lid], n);
            if (n1) atomicAdd(&patch_rel1[lid], n1);
            if (open) atomicOr(&patch_flags[lid], PF_OPEN_TMP);
        }
        todo &= ~same;
    }
}

// the volume rule applies to an orientable patch that is closed, or to every orientable patch with open_patches == 1
__device__ __forceinline__ bool volume_rule(int flags, int open_patches) {
    return !(flags & PF_NONORIENT) && (open_patches == 1 || !(flags & PF_OPEN_TMP));
}

__global__ __launch_bounds__(TB) void k_mo_vol(const int64_t* __restrict__ faces, int F, const float* __restrict__ P, const int* __restrict__ root,
                                               const int* __restrict__ pid, const int* __restrict__ fbits, const int32_t* __restrict__ patch_flags,
                                               const uint32_t* __restrict__ box, int open_patches, unsigned long long* __restrict__ patch_vol,
                                               const int* __restrict__ misc) {
    if (misc[M_ERR] | misc[M_CAP]) return;
    const int f = blockIdx.x * blockDim.x + threadIdx.x, lane = threadIdx.x & 63;
    int bits;
    const int id = patch_of(f, F, root, pid, fbits, bits);
    const bool active = id >= 0 && volume_rule(patch_flags[id], open_patches);
    long long det = 0;
    if (active) {
        double lo[3], ext = 0.0;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            lo[k] = (double)ord2f(box[6 * (size_t)id + k]);
            ext = fmax(ext, (double)ord2f(box[6 * (size_t)id + 3 + k]) - lo[k]);
        }
        const double s = ext == 0.0 ? 0.0 : (double)GRID_MAX / ext;
        long long c[3][3];
#pragma unroll
        for (int e = 0; e < 3; ++e) {
            const size_t v = (size_t)faces[3 * (size_t)f + e];
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const double q = fmin(fmax(floor(((double)P[3 * v + k] - lo[k]) * s), 0.0), (double)GRID_MAX);
                c[e][k] = 2 * (long long)q - GRID_MAX;
            }
        }
        det = c[0][0] * (c[1][1] * c[2][2] - c[1][2] * c[2][1]) - c[0][1] * (c[1][0] * c[2][2] - c[1][2] * c[2][0]) +
              c[0][2] * (c[1][0] * c[2][1] - c[1][1] * c[2][0]);
        if (bits & FB_REL) det = -det;
    }
    unsigned long long todo = __ballot(active);
    while (todo) {
        const int leader = __ffsll((long long)todo) - 1;
        const int lid = __shfl(id, leader);
        const bool mine = active && id == lid;
        const unsigned long long same = __ballot(mine);
        if (__popcll(same) >= 8) {
            const long long sum = wave_sum(mine ? det : 0ll);
            if (lane == leader && sum) atomicAdd(&patch_vol[lid], (unsigned long long)sum);
        } else if (mine && det) {
            atomicAdd(&patch_vol[lid], (unsigned long long)det);
        }
        todo &= ~same;
    }
}

// (a soup has a patch per face: the two totals are summed per wave first, one add per wave, like the unit's other counters.  Every lane of the
// wave runs this kernel to its end)
__global__ __launch_bounds__(TB) void k_mo_decide(int open_patches, int32_t* __restrict__ patch_faces, int32_t* __restrict__ patch_flipped,
                                                  int32_t* __restrict__ patch_flags, int64_t* __restrict__ patch_vol, int* __restrict__ misc) {
    if (misc[M_ERR] | misc[M_CAP]) return;
    const int i = blockIdx.x * blockDim.x + threadIdx.x, lane = threadIdx.x & 63;
    const bool in = i < misc[M_P];
    bool non = false;
    int flipped = 0;
    if (in) {
        const int fl = patch_flags[i], n = patch_faces[i], n1 = patch_flipped[i];
        int out = (fl & PF_OPEN_TMP) ? 0 : PF_CLOSED;
        int64_t vol = 0;
        non = (fl & PF_NONORIENT) != 0;
        if (non) {
            out |= PF_NONORIENT;
        } else {
            if (volume_rule(fl, open_patches)) vol = patch_vol[i];
            int c;
            if (vol != 0) { out |= PF_VOLUME; c = vol < 0 ? 1 : 0; }
            else c = n1 > n - n1 ? 1 : 0;                          // (a tie keeps the root's winding)
            if (c) out |= PF_COMPLEMENT;
            flipped = c ? n - n1 : n1;
        }
        patch_flags[i] = out;
        patch_flipped[i] = flipped;
        patch_vol[i] = vol;
    }
    wave_count(&misc[M_NONORIENT], non, lane);
    const int total = (int)wave_sum((long long)flipped);           // (at most F < 2^31 in all)
    if (lane == 0 && total) atomicAdd(&misc[M_FLIPPED], total);
}

__global__ __launch_bounds__(TB) void k_mo_write(const int64_t* __restrict__ faces, int F, const int* __restrict__ root, const int* __restrict__ pid,
                                                 const int* __restrict__ fbits, const int32_t* __restrict__ patch_flags, int64_t* __restrict__ out_faces,
                                                 uint8_t* __restrict__ flip, int32_t* __restrict__ face_patch, int32_t* __restrict__ counts,
                                                 const int* __restrict__ misc) {
    if (misc[M_ERR] | misc[M_CAP]) return;
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f == 0) {
        counts[0] = misc[M_P]; counts[1] = misc[M_FLIPPED]; counts[2] = misc[M_NONORIENT]; counts[3] = misc[M_INCOHERENT];
        counts[4] = misc[M_BOUNDARY]; counts[5] = misc[M_NONMANIFOLD]; counts[6] = misc[M_DEGENERATE]; counts[7] = 0;
    }
    if (f >= F) return;
    int bits;
    const int id = patch_of(f, F, root, pid, fbits, bits);
    int fl = 0;
    if (id >= 0) {
        const int pf = patch_flags[id];
        if (!(pf & PF_NONORIENT)) fl = ((bits & FB_REL) ? 1 : 0) ^ ((pf & PF_COMPLEMENT) ? 1 : 0);
    }
    const int64_t a = faces[3 * (size_t)f], b = faces[3 * (size_t)f + 1], c = faces[3 * (size_t)f + 2];
    out_faces[3 * (size_t)f] = a;
    out_faces[3 * (size_t)f + 1] = fl ? c : b;
    out_faces[3 * (size_t)f + 2] = fl ? b : c;
    flip[f] = (uint8_t)fl;
    face_patch[f] = id;
}

}  // namespace
}  // namespace pdhip

using namespace pdhip;

extern "C" int pdhip_orient_faces(const float* vertices, int Vn, const int64_t* faces, int F, int open_patches, int64_t* out_faces, uint8_t* flip,
                                  int32_t* face_patch, int32_t* patch_root, int32_t* patch_faces, int32_t* patch_flipped, int32_t* patch_flags,
                                  int64_t* patch_vol, int32_t* counts, uint64_t* keys_a, uint64_t* keys_b, int32_t* vals_a, int32_t* vals_b,
                                  size_t sort_len, int32_t* hist, size_t hist_words, int32_t* face_tmp, size_t face_tmp_len, int32_t* box,
                                  size_t box_len, int32_t* tiles, size_t tiles_len, int32_t* misc, size_t misc_len, void* stream) {
#define OF_PTR(p) PD_REQUIRE(p, "pdhip_orient_faces: null pointer (" #p ")")
    OF_PTR(vertices); OF_PTR(faces); OF_PTR(out_faces); OF_PTR(flip); OF_PTR(face_patch); OF_PTR(patch_root); OF_PTR(patch_faces); OF_PTR(patch_flipped);
    OF_PTR(patch_flags); OF_PTR(patch_vol); OF_PTR(counts); OF_PTR(keys_a); OF_PTR(keys_b); OF_PTR(vals_a); OF_PTR(vals_b); OF_PTR(hist);
    OF_PTR(face_tmp); OF_PTR(box); OF_PTR(tiles); OF_PTR(misc);
#undef OF_PTR
    PD_REQUIRE(Vn >= 1 && F >= 1, "pdhip_orient_faces: Vn=%d F=%d: at least one vertex and one face", Vn, F);
    PD_REQUIRE(Vn <= MESH_MAX_V && F <= MESH_MAX_F, "pdhip_orient_faces: Vn=%d F=%d exceed the limits (Vn <= 2^26, F <= 2^23)", Vn, F);
    PD_REQUIRE(open_patches == 0 || open_patches == 1, "pdhip_orient_faces: open_patches=%d is neither 0 (majority) nor 1 (volume)", open_patches);
    const size_t nf = (size_t)F, ne = 3 * nf;
#define OF_LEN(have, need, name) PD_REQUIRE((have) >= (need), "pdhip_orient_faces: " name " holds %zu elements, F=%d needs %zu", (size_t)(have), F, (size_t)(need))
    OF_LEN(sort_len, ne, "keys_a / keys_b / vals_a / vals_b");
    OF_LEN(hist_words, hist_len(ne), "hist");
    OF_LEN(face_tmp_len, FACE_ARRAYS * nf, "face_tmp");
    OF_LEN(box_len, 6 * nf, "box");
    OF_LEN(tiles_len, 2 * scan_tiles(nf), "tiles");
    OF_LEN(misc_len, (size_t)MISC_WORDS, "misc");
#undef OF_LEN
    hipStream_t s = as_stream(stream);
    int *word = face_tmp, *root = face_tmp + nf, *isroot = face_tmp + 2 * nf, *pid = face_tmp + 3 * nf, *fbits = face_tmp + 4 * nf;
    int *tsum = tiles, *toff = tiles + scan_tiles(nf);
    uint32_t* ubox = reinterpret_cast<uint32_t*>(box);
    unsigned long long* uvol = reinterpret_cast<unsigned long long*>(patch_vol);
    const uint64_t none = (uint64_t)Vn * (uint64_t)Vn;
    const int n = 3 * F, gf = cdiv(F, TB), ge = cdiv(n, TB);
    PD_HIP(hipMemsetAsync(misc, 0, MISC_WORDS * sizeof(int32_t), s));
    SortBufs sb;
    sb.k[0] = keys_a; sb.k[1] = keys_b; sb.v[0] = vals_a; sb.v[1] = vals_b; sb.hist = hist;
    k_mo_keys<<<gf, TB, 0, s>>>(faces, F, vertices, Vn, sb.k[0], sb.v[0], word, fbits, misc);
    const int cur = radix_sort(sb, n, bits_for(none), s);
    k_mo_edges<<<ge, TB, 0, s>>>(sb.k[cur], sb.v[cur], n, F, none, word, fbits, misc);
    k_mo_flatten<<<gf, TB, 0, s>>>(word, F, root, isroot, fbits, misc);
    if (F <= SMALL_SCAN) k_scan<int><<<1, SC_T, 0, s>>>(isroot, pid, F, 1);
    else scan_exclusive(isroot, pid, F, tsum, toff, s);
    k_mo_patch_init<<<gf, TB, 0, s>>>(isroot, pid, F, patch_root, patch_faces, patch_flipped, patch_flags, uvol, ubox, misc);
    k_mo_recheck<<<ge, TB, 0, s>>>(sb.k[cur], sb.v[cur], n, none, root, pid, fbits, patch_flags, misc);
    k_mo_face_stats<<<gf, TB, 0, s>>>(faces, F, vertices, root, pid, fbits, patch_faces, patch_flipped, patch_flags, ubox, misc);
    k_mo_vol<<<gf, TB, 0, s>>>(faces, F, vertices, root, pid, fbits, patch_flags, ubox, open_patches, uvol, misc);
    k_mo_decide<<<gf, TB, 0, s>>>(open_patches, patch_faces, patch_flipped, patch_flags, patch_vol, misc);
    k_mo_write<<<gf, TB, 0, s>>>(faces, F, root, pid, fbits, patch_flags, out_faces, flip, face_patch, counts, misc);
    PD_LAUNCH_CHECK();
    int h[2];
    const int rc = read_words(misc, h, 2, s);
    if (rc) return rc;
    PD_REQUIRE(!(h[M_ERR] & ERR_INDEX), "pdhip_orient_faces: a face index outside [0, Vn=%d)", Vn);
    PD_REQUIRE(!(h[M_ERR] & ERR_NONFINITE), "pdhip_orient_faces: a referenced vertex is not finite (the volume rule needs finite coordinates)");
    if (h[M_CAP]) {
        set_error("pdhip_orient_faces: a union-find walk used up its budget of steps (word %d): the forest is not the descending one the kernels "
                  "keep; the outputs are not valid", h[M_CAP]);
        return PDHIP_E_STATE;
    }
    return PDHIP_OK;
}
