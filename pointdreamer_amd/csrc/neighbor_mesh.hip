// SURVEY 8(f)-2, the mesh side of complete_unseen_by='neighbor' (pointdreamer/unproject.py:105-127, 145-155, utils/mesh_utils.py:7-114): what
// pointdreamer_amd/mesh_utils.py computes with numpy on the host, on the device and bit for bit.
//   pdhip_subdivide_with_uv    one round of midpoint subdivision of the picked faces, positions and UVs
//     k_nm_pick / k_nm_fill      picked-face flags from the index list (duplicates collapse), or all faces
//     k_nm_edge_keys             one key (larger endpoint, smaller endpoint) per corner of a picked face, in picked-face order
//     k_run_heads                first entry of every run of equal sorted keys  -> scan -> id of the run's midpoint
//     k_nm_midpoints             midpoint id per corner; the first entry of a run writes (x[lo] + x[hi]) / 2
//     k_nm_children              untouched faces first, then (v0 m01 m20) (m01 v1 m12) (m20 m12 v2) (m01 m12 m20) per picked face
//   pdhip_vertex_uv_table      k_nm_best_uv (atomicMax of the UV index per vertex) / k_nm_uv_gather
//   pdhip_neighbour_csr        k_nm_pair_keys (6 directed pairs per face, self pairs dropped) -> sort -> unique -> k_nm_csr_write
//   pdhip_compact_zero_count   k_nm_zero_flags -> scan -> k_nm_compact
// Ordering comes from the stable radix sort and the scans of radix_sort.h only; the atomics used (max of an index, add of a count) are
// order-independent, so two runs give equal bytes.  All sizes are int32 and checked on entry.  Each entry reads its counts and error
// flags back ONCE, at its end (one stream synchronisation), and hands the same read to the caller through counts_host.
#include "mesh_common.h"
using namespace pdhip;

namespace {

constexpr int TB = 256;
constexpr int ERR_PICK = 1, ERR_FACE = 2, ERR_TEX = 4;
// misc words
constexpr int M_ERR = 0, M_C0 = 1, M_LIVE = 5, M_WORDS = 8;        // M_C0 .. M_C0 + 3: the counts as the host reads them; M_LIVE: the 3 T edge keys
constexpr int M_READ = 5;                                          // the one read of an entry: misc[0 .. 4] = error flags + counts

// ---- subdivision -------------------------------------------------------------------------------------------------------------
__global__ void k_nm_fill(int* __restrict__ p, int n, int value) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) p[i] = value;
}

__global__ void k_nm_pick(const int64_t* __restrict__ face_index, int K, int F, int* __restrict__ pick, int* __restrict__ misc) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= K) return;
    const int64_t f = face_index[k];
    if (!index_ok(f, F)) atomicOr(&misc[M_ERR], ERR_PICK);
    else pick[f] = 1;
}

// thread i < F: the three edge keys of face i if it is picked (slot 3 * rank + corner); thread i in [3T, N): padding that sorts last;
// thread 0 leaves 3 T, the number of keys that are edges, in misc[M_LIVE] for k_run_heads
__global__ void k_nm_edge_keys(const int64_t* __restrict__ tri, int F, int n_index, int err_bit, const int* __restrict__ pinc, int N,
                               uint64_t* __restrict__ keys, int* __restrict__ vals, int* __restrict__ misc) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const int T = pinc[F - 1];
    if (i == 0) misc[M_LIVE] = 3 * T;
    if (i < N && i >= 3 * T) {
        keys[i] = pair_key(n_index - 1, n_index - 1, n_index);
        vals[i] = i;
    }
    if (i >= F) return;
    const int inc = pinc[i];
    if (inc == (i ? pinc[i - 1] : 0)) return;                   // not picked
    const int r = inc - 1;
    int64_t a[3] = {tri[3 * (size_t)i], tri[3 * (size_t)i + 1], tri[3 * (size_t)i + 2]};
    bool bad = false;
#pragma unroll
    for (int c = 0; c < 3; ++c)
        if (!index_ok(a[c], n_index)) { bad = true; a[c] = 0; }
    if (bad) atomicOr(&misc[M_ERR], err_bit);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const uint64_t p = (uint64_t)a[c], q = (uint64_t)a[c == 2 ? 0 : c + 1];
        const uint64_t lo = p < q ? p : q, hi = p < q ? q : p;
        keys[3 * r + c] = pair_key(hi, lo, n_index);
        vals[3 * r + c] = 3 * r + c;
    }
}

template <int C>
__global__ void k_nm_midpoints(const uint64_t* __restrict__ keys, const int* __restrict__ vals, const int* __restrict__ flag,
                               const int* __restrict__ incl, int N, const int* __restrict__ pinc, int F, int n_index,
                               const float* __restrict__ x, float* __restrict__ out, int* __restrict__ mid) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N || i >= 3 * pinc[F - 1]) return;
    const int id = n_index + incl[i] - 1;
    mid[vals[i]] = id;
    if (!flag[i]) return;
    const uint64_t key = keys[i];
    const size_t hi = (size_t)pair_first(key, n_index), lo = (size_t)pair_second(key, n_index);
#pragma unroll
    for (int c = 0; c < C; ++c) out[(size_t)id * C + c] = (x[lo * C + c] + x[hi * C + c]) / 2.0f;
}

__device__ __forceinline__ void put3(int64_t* __restrict__ o, size_t row, int64_t a, int64_t b, int64_t c) {
    o[3 * row] = a; o[3 * row + 1] = b; o[3 * row + 2] = c;
}

__global__ void k_nm_children(const int64_t* __restrict__ faces, const int64_t* __restrict__ fuv, int F, const int* __restrict__ pinc,
                              const int* __restrict__ mid, const int* __restrict__ mid_uv, int64_t* __restrict__ out_faces,
                              int64_t* __restrict__ out_fuv) {
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= F) return;
    const int T = pinc[F - 1], inc = pinc[f];
    const size_t s = 3 * (size_t)f;
    const int64_t v0 = faces[s], v1 = faces[s + 1], v2 = faces[s + 2];
    const int64_t t0 = fuv[s], t1 = fuv[s + 1], t2 = fuv[s + 2];
    if (inc == (f ? pinc[f - 1] : 0)) {
        put3(out_faces, (size_t)(f - inc), v0, v1, v2);
        put3(out_fuv, (size_t)(f - inc), t0, t1, t2);
        return;
    }
    const int r = inc - 1;
    const size_t base = (size_t)(F - T) + 4 * (size_t)r;
    {
        const int64_t m01 = mid[3 * r], m12 = mid[3 * r + 1], m20 = mid[3 * r + 2];
        put3(out_faces, base, v0, m01, m20); put3(out_faces, base + 1, m01, v1, m12);
        put3(out_faces, base + 2, m20, m12, v2); put3(out_faces, base + 3, m01, m12, m20);
    }
    {
        const int64_t m01 = mid_uv[3 * r], m12 = mid_uv[3 * r + 1], m20 = mid_uv[3 * r + 2];
        put3(out_fuv, base, t0, m01, m20); put3(out_fuv, base + 1, m01, t1, m12);
        put3(out_fuv, base + 2, m20, m12, t2); put3(out_fuv, base + 3, m01, m12, m20);
    }
}

// counts = V', U', F', T (E / Euv: the last words of the two unique scans, kept in misc by k_nm_keep)
__global__ void k_nm_keep(const int* __restrict__ incl, int N, int* __restrict__ dst) { *dst = N > 0 ? incl[N - 1] : 0; }

__global__ void k_nm_sub_counts(int V, int U, int F, const int* __restrict__ pinc, int* __restrict__ misc, int32_t* __restrict__ counts) {
    const int T = pinc[F - 1];
    const int c[4] = {V + misc[M_C0], U + misc[M_C0 + 1], F + 3 * T, T};
#pragma unroll
    for (int k = 0; k < 4; ++k) { misc[M_C0 + k] = c[k]; counts[k] = c[k]; }
}

struct SubWs {
    int *pick, *pinc, *mid, *mid_uv, *flag, *incl, *misc;
    SortBufs sb;
};

static size_t carve_sub(SubWs& w, void* base, int F, int Tm) {
    const size_t N = 3 * (size_t)Tm;
    Carve c{static_cast<char*>(base), 0};
    w.pick = c.take<int>(F); w.pinc = c.take<int>(F); w.mid = c.take<int>(N); w.mid_uv = c.take<int>(N);
    w.flag = c.take<int>(N); w.incl = c.take<int>(N); w.misc = c.take<int>(M_WORDS);
    carve_sort(c, w.sb, N);
    return c.off + 256;
}

static int picked_max(int F, int K) { return K < 0 ? F : (K < F ? K : F); }

constexpr int MAX_FACES = 1 << 27, MAX_POINTS = 1 << 29;          // V + 3F, U + 3F, 4F, 3F and 6F all stay below 2^31

// the midpoints of one index space (positions or UVs): keys -> sort -> unique -> ids + values
template <int C>
static int midpoints(SubWs& w, const int64_t* tri, int F, int n_index, int err_bit, int N, const float* x, float* out, int* mid, int* keep,
                     hipStream_t s) {
    const int g = cdiv(F > N ? F : N, TB), gN = cdiv(N, TB);
    k_nm_edge_keys<<<g, TB, 0, s>>>(tri, F, n_index, err_bit, w.pinc, N, w.sb.k[0], w.sb.v[0], w.misc);
    const int cur = radix_sort(w.sb, N, bits_for((unsigned long long)n_index * (unsigned long long)n_index - 1ull), s);
    k_run_heads<uint64_t><<<gN, TB, 0, s>>>(w.sb.k[cur], N, w.misc + M_LIVE, ~0ull, w.flag);
    k_scan<<<1, SC_T, 0, s>>>(w.flag, w.incl, N, 0);
    k_nm_midpoints<C><<<gN, TB, 0, s>>>(w.sb.k[cur], w.sb.v[cur], w.flag, w.incl, N, w.pinc, F, n_index, x, out, mid);
    k_nm_keep<<<1, 1, 0, s>>>(w.incl, N, keep);
    PD_LAUNCH_CHECK();
    return PDHIP_OK;
}

// ---- per-vertex UV table -------------------------------------------------------------------------------------------------------
__global__ void k_nm_best_uv(const int64_t* __restrict__ faces, const int64_t* __restrict__ fuv, int n, int V, int U, int* __restrict__ best,
                             int32_t* __restrict__ skipped) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int64_t v = faces[i], t = fuv[i];
    if (!(index_ok(v, V) && index_ok(t, U))) atomicAdd(skipped, 1);
    else atomicMax(&best[v], (int)t);
}

__global__ void k_nm_uv_gather(const int* __restrict__ best, int V, const float* __restrict__ uvs, float* __restrict__ out) {
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= V) return;
    const int b = best[v];
    out[2 * (size_t)v] = b >= 0 ? uvs[2 * (size_t)b] : 0.0f;
    out[2 * (size_t)v + 1] = b >= 0 ? uvs[2 * (size_t)b + 1] : 0.0f;
}

// ---- neighbour CSR -------------------------------------------------------------------------------------------------------------
// pair p of face f: (a, b) = corners (p, p + 1) for p < 3, (p + 1, p) for p >= 3; self pairs and bad indices get the key V * V - 1,
// which no real pair has (it would be the self pair of the last vertex)
__global__ void k_nm_pair_keys(const int64_t* __restrict__ faces, int F, int V, uint64_t* __restrict__ keys, int* __restrict__ vals,
                               int* __restrict__ misc) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= 6 * F) return;
    const int f = i / 6, p = i - 6 * f, c = p < 3 ? p : p - 3;
    int64_t a = faces[3 * (size_t)f + c], b = faces[3 * (size_t)f + (c == 2 ? 0 : c + 1)];
    if (p >= 3) { const int64_t t = a; a = b; b = t; }
    uint64_t key = pair_key(V - 1, V - 1, V);
    if (!(index_ok(a, V) && index_ok(b, V))) atomicOr(&misc[M_ERR], ERR_FACE);
    else if (a != b) key = pair_key(a, b, V);
    keys[i] = key;
    vals[i] = i;
}

__global__ void k_nm_csr_write(const uint64_t* __restrict__ keys, const int* __restrict__ flag, const int* __restrict__ incl, int N, int V,
                               int* __restrict__ deg, int32_t* __restrict__ colidx) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N || !flag[i]) return;
    const uint64_t key = keys[i];
    const int row = (int)pair_first(key, V);
    colidx[incl[i] - 1] = (int32_t)pair_second(key, V);
    atomicAdd(&deg[row + 1], 1);
}

__global__ void k_nm_one_count(const int* __restrict__ incl, int N, int* __restrict__ misc, int32_t* __restrict__ counts) {
    const int n = incl[N - 1];
    misc[M_C0] = n;
    counts[0] = n;
}

struct CsrWs {
    int *flag, *incl, *deg, *misc;
    SortBufs sb;
};

static size_t carve_csr(CsrWs& w, void* base, int V, int F) {
    const size_t N = 6 * (size_t)F;
    Carve c{static_cast<char*>(base), 0};
    w.flag = c.take<int>(N); w.incl = c.take<int>(N); w.deg = c.take<int>((size_t)V + 1); w.misc = c.take<int>(M_WORDS);
    carve_sort(c, w.sb, N);
    return c.off + 256;
}

// ---- vertices without a colour ---------------------------------------------------------------------------------------------------
__global__ void k_nm_zero_flags(const float* __restrict__ count, int V, int* __restrict__ flag) {
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v < V) flag[v] = count[v] == 0.0f ? 1 : 0;
}

__global__ void k_nm_compact(const int* __restrict__ flag, const int* __restrict__ incl, int V, int32_t* __restrict__ out) {
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v < V && flag[v]) out[incl[v] - 1] = v;
}

}  // namespace

extern "C" size_t pdhip_subdivide_with_uv_ws_bytes(int V, int U, int F, int K) {
    if (V <= 0 || U <= 0 || F <= 0 || F > MAX_FACES) return 0;
    SubWs w;
    return carve_sub(w, nullptr, F, picked_max(F, K));
}

extern "C" int pdhip_subdivide_with_uv(const float* vertices, int V, const int64_t* faces, int F, const float* uvs, int U,
                                       const int64_t* face_uv_idx, const int64_t* face_index, int K, float* out_vertices,
                                       int64_t* out_faces, float* out_uvs, int64_t* out_face_uv_idx, int32_t* counts,
                                       int32_t* counts_host, void* ws, void* stream) {
    PD_REQUIRE(vertices && faces && uvs && face_uv_idx && out_vertices && out_faces && out_uvs && out_face_uv_idx && counts && ws,
               "pdhip_subdivide_with_uv: null pointer");
    PD_REQUIRE(V > 0 && U > 0 && F > 0, "pdhip_subdivide_with_uv: empty mesh (V=%d U=%d F=%d)", V, U, F);
    PD_REQUIRE(F <= MAX_FACES && V <= MAX_POINTS && U <= MAX_POINTS,
               "pdhip_subdivide_with_uv: V=%d U=%d F=%d exceed the int32 index range (F <= 2^27, V, U <= 2^29)", V, U, F);
    PD_REQUIRE(K >= -1 && K <= (1 << 30), "pdhip_subdivide_with_uv: K=%d index entries, need -1 (all faces) .. 2^30", K);
    PD_REQUIRE((K > 0) == (face_index != nullptr) || (K == 0),
               "pdhip_subdivide_with_uv: face_index goes with K > 0; NULL with K = -1 picks all faces (K=%d)", K);
    hipStream_t s = as_stream(stream);
    SubWs w;
    const int Tm = picked_max(F, K), N = 3 * Tm, gF = cdiv(F, TB);
    carve_sub(w, ws, F, Tm);
    PD_HIP(hipMemsetAsync(w.misc, 0, M_WORDS * sizeof(int), s));
    if (K < 0) {
        k_nm_fill<<<gF, TB, 0, s>>>(w.pick, F, 1);
    } else {
        PD_HIP(hipMemsetAsync(w.pick, 0, (size_t)F * sizeof(int), s));
        if (K > 0) k_nm_pick<<<cdiv(K, TB), TB, 0, s>>>(face_index, K, F, w.pick, w.misc);
    }
    k_scan<<<1, SC_T, 0, s>>>(w.pick, w.pinc, F, 0);
    PD_HIP(hipMemcpyAsync(out_vertices, vertices, 3 * (size_t)V * sizeof(float), hipMemcpyDeviceToDevice, s));
    PD_HIP(hipMemcpyAsync(out_uvs, uvs, 2 * (size_t)U * sizeof(float), hipMemcpyDeviceToDevice, s));
    if (N > 0) {
        int rc = midpoints<3>(w, faces, F, V, ERR_FACE, N, vertices, out_vertices, w.mid, w.misc + M_C0, s);
        if (rc != PDHIP_OK) return rc;
        rc = midpoints<2>(w, face_uv_idx, F, U, ERR_TEX, N, uvs, out_uvs, w.mid_uv, w.misc + M_C0 + 1, s);
        if (rc != PDHIP_OK) return rc;
    }
    k_nm_children<<<gF, TB, 0, s>>>(faces, face_uv_idx, F, w.pinc, w.mid, w.mid_uv, out_faces, out_face_uv_idx);
    k_nm_sub_counts<<<1, 1, 0, s>>>(V, U, F, w.pinc, w.misc, counts);
    PD_LAUNCH_CHECK();
    int h[M_READ];
    const int rc = read_words(w.misc, h, M_READ, s);
    if (rc != PDHIP_OK) return rc;
    PD_REQUIRE(!(h[M_ERR] & ERR_PICK), "pdhip_subdivide_with_uv: a face_index entry lies outside [0, F=%d)", F);
    PD_REQUIRE(!(h[M_ERR] & ERR_FACE), "pdhip_subdivide_with_uv: a picked face has a vertex index outside [0, V=%d)", V);
    PD_REQUIRE(!(h[M_ERR] & ERR_TEX), "pdhip_subdivide_with_uv: a picked face has a UV index outside [0, U=%d)", U);
    if (counts_host)
        for (int k = 0; k < 4; ++k) counts_host[k] = h[M_C0 + k];
    return PDHIP_OK;
}

extern "C" size_t pdhip_vertex_uv_table_ws_bytes(int V, int F) {
    if (V <= 0 || F <= 0) return 0;
    return (size_t)V * sizeof(int) + 256;
}

extern "C" int pdhip_vertex_uv_table(int V, const int64_t* faces, const int64_t* face_uv_idx, int F, const float* uvs, int U,
                                     float* vert_uvs, int32_t* counts, void* ws, void* stream) {
    PD_REQUIRE(faces && face_uv_idx && uvs && vert_uvs && counts && ws, "pdhip_vertex_uv_table: null pointer");
    PD_REQUIRE(V > 0 && U > 0 && F > 0, "pdhip_vertex_uv_table: empty mesh (V=%d U=%d F=%d)", V, U, F);
    PD_REQUIRE(F <= 4 * MAX_FACES, "pdhip_vertex_uv_table: F=%d faces exceed the int32 index range (3F < 2^31)", F);
    hipStream_t s = as_stream(stream);
    int* best = static_cast<int*>(ws);
    PD_HIP(hipMemsetAsync(best, 0xff, (size_t)V * sizeof(int), s));
    PD_HIP(hipMemsetAsync(counts, 0, sizeof(int32_t), s));
    k_nm_best_uv<<<cdiv(3ll * F, TB), TB, 0, s>>>(faces, face_uv_idx, 3 * F, V, U, best, counts);
    k_nm_uv_gather<<<cdiv(V, TB), TB, 0, s>>>(best, V, uvs, vert_uvs);
    PD_LAUNCH_CHECK();
    return PDHIP_OK;
}

extern "C" size_t pdhip_neighbour_csr_ws_bytes(int V, int F) {
    if (V <= 0 || F <= 0 || F > 2 * MAX_FACES) return 0;
    CsrWs w;
    return carve_csr(w, nullptr, V, F);
}

extern "C" int pdhip_neighbour_csr(int V, const int64_t* faces, int F, int32_t* rowptr, int32_t* colidx, int32_t* counts,
                                   int32_t* counts_host, void* ws, void* stream) {
    PD_REQUIRE(faces && rowptr && colidx && counts && ws, "pdhip_neighbour_csr: null pointer");
    PD_REQUIRE(V > 0 && F > 0, "pdhip_neighbour_csr: empty mesh (V=%d F=%d)", V, F);
    PD_REQUIRE(F <= 2 * MAX_FACES && V < 2147483647,
               "pdhip_neighbour_csr: V=%d F=%d exceed the int32 index range (6F < 2^31, V + 1 < 2^31)", V, F);
    hipStream_t s = as_stream(stream);
    CsrWs w;
    carve_csr(w, ws, V, F);
    const int N = 6 * F, gN = cdiv(N, TB);
    PD_HIP(hipMemsetAsync(w.misc, 0, M_WORDS * sizeof(int), s));
    PD_HIP(hipMemsetAsync(w.deg, 0, ((size_t)V + 1) * sizeof(int), s));
    k_nm_pair_keys<<<gN, TB, 0, s>>>(faces, F, V, w.sb.k[0], w.sb.v[0], w.misc);
    const int cur = radix_sort(w.sb, N, bits_for((unsigned long long)V * (unsigned long long)V - 1ull), s);
    k_run_heads<uint64_t><<<gN, TB, 0, s>>>(w.sb.k[cur], N, nullptr, (uint64_t)V * (uint64_t)V - 1ull, w.flag);
    k_scan<<<1, SC_T, 0, s>>>(w.flag, w.incl, N, 0);
    k_nm_csr_write<<<gN, TB, 0, s>>>(w.sb.k[cur], w.flag, w.incl, N, V, w.deg, colidx);
    k_scan<<<1, SC_T, 0, s>>>(w.deg, rowptr, V + 1, 0);
    k_nm_one_count<<<1, 1, 0, s>>>(w.incl, N, w.misc, counts);
    PD_LAUNCH_CHECK();
    int h[M_READ];
    const int rc = read_words(w.misc, h, M_READ, s);
    if (rc != PDHIP_OK) return rc;
    PD_REQUIRE(!(h[M_ERR] & ERR_FACE), "pdhip_neighbour_csr: a face has a vertex index outside [0, V=%d)", V);
    if (counts_host) counts_host[0] = h[M_C0];
    return PDHIP_OK;
}

extern "C" size_t pdhip_compact_zero_count_ws_bytes(int V) {
    if (V <= 0) return 0;
    Carve c{nullptr, 0};
    c.take<int>(V); c.take<int>(V); c.take<int>(M_WORDS);
    return c.off + 256;
}

extern "C" int pdhip_compact_zero_count(const float* count, int V, int32_t* invalid, int32_t* counts, int32_t* counts_host, void* ws,
                                        void* stream) {
    PD_REQUIRE(count && invalid && counts && ws, "pdhip_compact_zero_count: null pointer");
    PD_REQUIRE(V > 0, "pdhip_compact_zero_count: V=%d vertices", V);
    hipStream_t s = as_stream(stream);
    Carve c{static_cast<char*>(ws), 0};
    int* flag = c.take<int>(V);
    int* incl = c.take<int>(V);
    int* misc = c.take<int>(M_WORDS);
    const int g = cdiv(V, TB);
    PD_HIP(hipMemsetAsync(misc, 0, M_WORDS * sizeof(int), s));
    k_nm_zero_flags<<<g, TB, 0, s>>>(count, V, flag);
    k_scan<<<1, SC_T, 0, s>>>(flag, incl, V, 0);
    k_nm_compact<<<g, TB, 0, s>>>(flag, incl, V, invalid);
    k_nm_one_count<<<1, 1, 0, s>>>(incl, V, misc, counts);
    PD_LAUNCH_CHECK();
    int h[M_READ];
    const int rc = read_words(misc, h, M_READ, s);
    if (rc != PDHIP_OK) return rc;
    if (counts_host) counts_host[0] = h[M_C0];
    return PDHIP_OK;
}
