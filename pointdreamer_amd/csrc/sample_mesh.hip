// Coloured point clouds from textured meshes (data/sample_colored_pc_from_mesh.py:50-184: kaolin's face_areas + sample_points and one
// grid_sample per material there; one draw kernel here).  Contract: include/pdhip.h, DESIGN.md "Sampling a textured mesh".
//   k_smp_area    per face: index checks (nothing outside a table is ever read), A_f in f64, Amax by an integer atomic max
//   k_smp_weight  w_f = floor(A_f * (2^40 / Amax)) as uint64
//   scan          inclusive uint64 prefix sum (radix_sort.h): the CDF is exact integer arithmetic, so it is monotone and the chosen face
//                 does not depend on the order in which tiles were added
//   k_smp_draw    one thread per sample: t = (W * m) >> 24 in 128 bits, binary search, fold, position / UV / normal, texture lookup
// No floating-point atomics; the host reads two words once (error flags, Amax).
#include "radix_sort.h"
#include "texture_lookup.h"

namespace pdhip {
namespace {

constexpr int TB = 256;
constexpr int MAX_F = 1 << 22;                                     // F * 2^40 <= 2^62: W * m fits 2^86, t fits 2^62
enum { E_VERTEX = 1, E_UV = 2, E_MATERIAL = 4, E_NONFINITE = 8, E_MATSET = 16 };

struct Misc {
    unsigned long long amax;                                       // bit pattern of the largest (non-negative) double area
    int err, pad;
};

__global__ __launch_bounds__(TB) void k_smp_area(const float* __restrict__ vertices, int Vn, const int64_t* __restrict__ faces, int F, int T,
                                                 const int64_t* __restrict__ face_uvs_idx, const int32_t* __restrict__ face_material,
                                                 const uint8_t* __restrict__ face_keep, long long texel_bytes,
                                                 const int64_t* __restrict__ mat_offset, const int32_t* __restrict__ mat_wh, int M,
                                                 double* __restrict__ area, Misc* __restrict__ misc) {
    const int f = blockIdx.x * TB + threadIdx.x;
    if (f < M) {                                                   // the material set: every image lies inside `texels`
        const long long off = mat_offset[f], w = mat_wh[2 * f], h = mat_wh[2 * f + 1];
        const bool kd = w == 0 && h == 0;
        if (!kd && (w <= 0 || h <= 0 || off < 0 || off > texel_bytes || 3 * w * h > texel_bytes - off)) atomicOr(&misc->err, E_MATSET);
    }
    if (f >= F) return;
    const int64_t i0 = faces[3 * f], i1 = faces[3 * f + 1], i2 = faces[3 * f + 2];
    int err = 0;
    if (i0 < 0 || i0 >= Vn || i1 < 0 || i1 >= Vn || i2 < 0 || i2 >= Vn) err |= E_VERTEX;
    if (face_uvs_idx) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const int64_t t = face_uvs_idx[3 * f + k];
            if (t < -1 || t >= T) err |= E_UV;
        }
    }
    if (face_material) {
        const int m = face_material[f];
        if (m < 0 || m >= M) err |= E_MATERIAL;
    }
    double A = 0.0;
    if (!err && (!face_keep || face_keep[f])) {
        const double ax = vertices[3 * i0], ay = vertices[3 * i0 + 1], az = vertices[3 * i0 + 2];
        const double e1x = (double)vertices[3 * i1] - ax, e1y = (double)vertices[3 * i1 + 1] - ay, e1z = (double)vertices[3 * i1 + 2] - az;
        const double e2x = (double)vertices[3 * i2] - ax, e2y = (double)vertices[3 * i2 + 1] - ay, e2z = (double)vertices[3 * i2 + 2] - az;
        const double cx = e1y * e2z - e1z * e2y, cy = e1z * e2x - e1x * e2z, cz = e1x * e2y - e1y * e2x;
        A = 0.5 * sqrt((cx * cx + cy * cy) + cz * cz);
        if (!(A < __builtin_huge_val())) { err |= E_NONFINITE; A = 0.0; }
        else if (A > 0.0) atomicMax(&misc->amax, (unsigned long long)__double_as_longlong(A));
    }
    if (err) atomicOr(&misc->err, err);
    area[f] = A;
}

__global__ __launch_bounds__(TB) void k_smp_weight(const double* __restrict__ area, int F, const Misc* __restrict__ misc, uint64_t* __restrict__ w) {
    const int f = blockIdx.x * TB + threadIdx.x;
    if (f >= F) return;
    const double scale = 1099511627776.0 / __longlong_as_double((long long)misc->amax);     // 2^40 / Amax
    w[f] = (uint64_t)floor(area[f] * scale);
}

__global__ __launch_bounds__(TB) void k_smp_draw(const float* __restrict__ vertices, const int64_t* __restrict__ faces, int F,
                                                 const float* __restrict__ uvs, const int64_t* __restrict__ face_uvs_idx,
                                                 const int32_t* __restrict__ face_material, const uint8_t* __restrict__ texels,
                                                 const int64_t* __restrict__ mat_offset, const int32_t* __restrict__ mat_wh,
                                                 const float* __restrict__ mat_kd, const uint64_t* __restrict__ cdf,
                                                 const float* __restrict__ rnd, int N, float* __restrict__ coords, float* __restrict__ colors,
                                                 float* __restrict__ normals, float* __restrict__ uvs_out, int32_t* __restrict__ face_idx,
                                                 int32_t* __restrict__ material_idx) {
    const int i = blockIdx.x * TB + threadIdx.x;
    if (i >= N) return;
    const float r0 = rnd[3 * i];
    float u = rnd[3 * i + 1], v = rnd[3 * i + 2];
    // face: the smallest f with cdf[f] > t, t = (W * m) >> 24.  m is held below 2^24 whatever the caller passed, so t < W = cdf[F - 1]
    // and the search ends inside the table, on a face of positive weight (one the area pass has checked)
    const float mf = floorf(r0 * 16777216.0f);
    const uint32_t m = mf >= 16777215.0f ? 16777215u : (mf > 0.0f ? (uint32_t)mf : 0u);
    const uint64_t Wt = cdf[F - 1];
    const uint64_t t = (__umul64hi(Wt, (uint64_t)m) << 40) | ((Wt * (uint64_t)m) >> 24);
    int lo = 0, hi = F - 1;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (cdf[mid] > t) hi = mid; else lo = mid + 1;
    }
    const int f = lo;
    const int64_t i0 = faces[3 * f], i1 = faces[3 * f + 1], i2 = faces[3 * f + 2];
    const float ax = vertices[3 * i0], ay = vertices[3 * i0 + 1], az = vertices[3 * i0 + 2];
    const float e1x = vertices[3 * i1] - ax, e1y = vertices[3 * i1 + 1] - ay, e1z = vertices[3 * i1 + 2] - az;
    const float e2x = vertices[3 * i2] - ax, e2y = vertices[3 * i2 + 1] - ay, e2z = vertices[3 * i2 + 2] - az;
    if (u + v > 1.0f) { u = 1.0f - u; v = 1.0f - v; }              // kaolin's fold
    coords[3 * i] = (ax + u * e1x) + v * e2x;
    coords[3 * i + 1] = (ay + u * e1y) + v * e2y;
    coords[3 * i + 2] = (az + u * e1z) + v * e2z;
    // camera_utils.face_normals_unit
    const float nx = e1y * e2z - e1z * e2y, ny = e1z * e2x - e1x * e2z, nz = e1x * e2y - e1y * e2x;
    const float len = fmaxf(sqrtf((nx * nx + ny * ny) + nz * nz), 1e-30f);
    normals[3 * i] = nx / len; normals[3 * i + 1] = ny / len; normals[3 * i + 2] = nz / len;
    // corner UVs: (0, 0) where the record has none
    float u0 = 0.f, v0 = 0.f, u1 = 0.f, v1 = 0.f, u2 = 0.f, v2 = 0.f;
    if (uvs && face_uvs_idx) {
        const int64_t t0 = face_uvs_idx[3 * f], t1 = face_uvs_idx[3 * f + 1], t2 = face_uvs_idx[3 * f + 2];
        if (t0 >= 0) { u0 = uvs[2 * t0]; v0 = uvs[2 * t0 + 1]; }
        if (t1 >= 0) { u1 = uvs[2 * t1]; v1 = uvs[2 * t1 + 1]; }
        if (t2 >= 0) { u2 = uvs[2 * t2]; v2 = uvs[2 * t2 + 1]; }
    }
    const float pu = (u0 + u * (u1 - u0)) + v * (u2 - u0);
    const float pv = (v0 + u * (v1 - v0)) + v * (v2 - v0);
    uvs_out[2 * i] = pu; uvs_out[2 * i + 1] = pv;                 // before the wrap, as the reference saves it
    face_idx[i] = f;
    const int mat = face_material ? face_material[f] : 0;
    material_idx[i] = mat;
    const int W = mat_wh[2 * mat], H = mat_wh[2 * mat + 1];
    float cr, cg, cb;
    if (W == 0 && H == 0) {
        cr = mat_kd[3 * mat]; cg = mat_kd[3 * mat + 1]; cb = mat_kd[3 * mat + 2];
    } else {
        material_lookup(texels + mat_offset[mat], W, H, pu, pv, cr, cg, cb);                // texture_lookup.h, shared with the renderer
    }
    colors[3 * i] = cr; colors[3 * i + 1] = cg; colors[3 * i + 2] = cb;
}

struct SampleWs {
    double* area;
    uint64_t *w, *cdf, *tsum, *toff;
    Misc* misc;
};

static size_t carve_sample(SampleWs& w, void* base, int F, int N) {
    (void)N;                                                       // (per-sample state lives in registers)
    const size_t nf = (size_t)F;
    Carve c{static_cast<char*>(base), 0};
    w.area = c.take<double>(nf); w.w = c.take<uint64_t>(nf); w.cdf = c.take<uint64_t>(nf);
    w.tsum = c.take<uint64_t>(scan_tiles(nf)); w.toff = c.take<uint64_t>(scan_tiles(nf));
    w.misc = c.take<Misc>(1);
    return c.bytes();
}

}  // namespace
}  // namespace pdhip

using namespace pdhip;

extern "C" size_t pdhip_sample_mesh_workspace_bytes(int F, int N) {
    if (F < 1 || F > MAX_F || N < 0) return 0;
    SampleWs w;
    return carve_sample(w, nullptr, F, N);
}

extern "C" int pdhip_sample_mesh(const float* vertices, int Vn, const int64_t* faces, int F, const float* uvs, int T,
                                 const int64_t* face_uvs_idx, const int32_t* face_material, const uint8_t* face_keep,
                                 const uint8_t* texels, int64_t texel_bytes, const int64_t* mat_offset, const int32_t* mat_wh,
                                 const float* mat_kd, int M, const float* rand, int N, float* coords, float* colors, float* normals,
                                 float* uvs_out, int32_t* face_idx, int32_t* material_idx, void* ws, void* stream) {
    PD_REQUIRE(F <= MAX_F, "pdhip_sample_mesh: F=%d exceeds 2^22 faces (the width of the integer CDF)", F);
    PD_REQUIRE(Vn >= 1 && F >= 1 && M >= 1 && N >= 0 && T >= 0 && texel_bytes >= 0, "pdhip_sample_mesh: bad size (Vn=%d F=%d T=%d M=%d N=%d)", Vn, F, T, M, N);
    PD_REQUIRE(vertices && faces && mat_offset && mat_wh && mat_kd && ws, "pdhip_sample_mesh: null pointer");
    PD_REQUIRE((uvs != nullptr) == (face_uvs_idx != nullptr), "pdhip_sample_mesh: uvs and face_uvs_idx go together");
    PD_REQUIRE(texels || texel_bytes == 0, "pdhip_sample_mesh: texels is null but texel_bytes=%lld", (long long)texel_bytes);
    PD_REQUIRE(N == 0 || (rand && coords && colors && normals && uvs_out && face_idx && material_idx), "pdhip_sample_mesh: null pointer");
    hipStream_t s = as_stream(stream);
    SampleWs w;
    carve_sample(w, ws, F, N);
    PD_HIP(hipMemsetAsync(w.misc, 0, sizeof(Misc), s));
    k_smp_area<<<cdiv(F > M ? F : M, TB), TB, 0, s>>>(vertices, Vn, faces, F, uvs ? T : 0, face_uvs_idx, face_material, face_keep,
                                                      (long long)texel_bytes, mat_offset, mat_wh, M, w.area, w.misc);
    PD_LAUNCH_CHECK();
    Misc h;
    PD_HIP(hipMemcpyAsync(&h, w.misc, sizeof(Misc), hipMemcpyDeviceToHost, s));
    PD_HIP(hipStreamSynchronize(s));
    PD_REQUIRE(!(h.err & E_VERTEX), "pdhip_sample_mesh: a face has a vertex index outside [0, %d)", Vn);
    PD_REQUIRE(!(h.err & E_UV), "pdhip_sample_mesh: a face has a uv index outside [-1, %d)", T);
    PD_REQUIRE(!(h.err & E_MATERIAL), "pdhip_sample_mesh: a face has a material index outside [0, %d)", M);
    PD_REQUIRE(!(h.err & E_MATSET), "pdhip_sample_mesh: a material's image (mat_offset, mat_wh) does not lie inside the %lld texel bytes",
               (long long)texel_bytes);
    PD_REQUIRE(!(h.err & E_NONFINITE), "pdhip_sample_mesh: a face has a non-finite area (NaN or infinite vertex)");
    PD_REQUIRE(h.amax != 0ull, "pdhip_sample_mesh: no face with positive area");
    if (N == 0) return PDHIP_OK;
    k_smp_weight<<<cdiv(F, TB), TB, 0, s>>>(w.area, F, w.misc, w.w);
    scan_inclusive<uint64_t>(w.w, w.cdf, F, w.tsum, w.toff, s);
    k_smp_draw<<<cdiv(N, TB), TB, 0, s>>>(vertices, faces, F, uvs, face_uvs_idx, face_material, texels, mat_offset, mat_wh, mat_kd, w.cdf,
                                          rand, N, coords, colors, normals, uvs_out, face_idx, material_idx);
    PD_LAUNCH_CHECK();
    return PDHIP_OK;
}
