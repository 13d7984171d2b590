// Shading stage of the evaluation renderer (utils/camera_utils.py:379-554 render_textured_mesh, :735-828 render_per_vertex_color_mesh):
// from the rasteriser's face_idx + barycentrics to a coloured, optionally lit image, in ONE pass per pixel -- attribute interpolation
// (the contract of pdhip_interpolate), `% 1` wrap + bilinear atlas lookup (grid_sample, align_corners=False, padding_mode='border'),
// Lambert lighting with the normal turned towards the camera, clip, gamma, vertical flip, and the 8-bit RGBA form the PNG writer takes.
// No uv_map [V,R,R,2] and no albedo image ever reach HBM.
#include "common.h"
#include "texture_lookup.h"

namespace pdhip {

constexpr int SHADE_MAX_LIGHTS = 16;

// The tail both shading kernels share: Lambert lighting with the normal turned towards the camera, clip, gamma (covered pixels only),
// then the f32 image and the 8-bit RGBA of OUTPUT pixel idx = (v, rem).  An uncovered pixel arrives with colour 0 and leaves as 0.
__device__ __forceinline__ void shade_finish(bool covered, float c0, float c1, float c2, long long f, int v, int rem, long long idx,
                                             long long RR, const float* __restrict__ fnorm, const float* __restrict__ cams,
                                             const float* __restrict__ lights, int L, int double_side, float inv_gamma,
                                             float* __restrict__ images, uint8_t* __restrict__ rgba) {
    if (covered && L > 0) {
        float nx = fnorm[3 * f], ny = fnorm[3 * f + 1], nz = fnorm[3 * f + 2];
        const float* cr = cams + (size_t)v * 16 + 6;                                 // R[2]: the camera's back axis
        if ((nx * cr[0] + ny * cr[1]) + nz * cr[2] < 0.0f) { nx = -nx; ny = -ny; nz = -nz; }
        float s0 = 0.f, s1 = 0.f, s2 = 0.f;
        for (int l = 0; l < L; ++l) {
            float d = (nx * lights[3 * l] + ny * lights[3 * l + 1]) + nz * lights[3 * l + 2];
            if (double_side) d = fabsf(d);
            d = fminf(fmaxf(d, 0.0f), 1.0f);
            s0 += c0 * d; s1 += c1 * d; s2 += c2 * d;
        }
        c0 = fminf(fmaxf(s0, 0.0f), 1.0f);
        c1 = fminf(fmaxf(s1, 0.0f), 1.0f);
        c2 = fminf(fmaxf(s2, 0.0f), 1.0f);
        if (inv_gamma > 0.0f) {
            c0 = powf(c0, inv_gamma); c1 = powf(c1, inv_gamma); c2 = powf(c2, inv_gamma);
        }
    }
    if (images) {
        float* o = images + (size_t)v * 3 * RR + rem;
        o[0] = c0; o[RR] = c1; o[2 * RR] = c2;
    }
    if (rgba) {
        uchar4 q = make_uchar4(0, 0, 0, 0);
        if (covered) {
            q.x = (unsigned char)fminf(fmaxf(rintf(c0 * 255.0f), 0.0f), 255.0f);
            q.y = (unsigned char)fminf(fmaxf(rintf(c1 * 255.0f), 0.0f), 255.0f);
            q.z = (unsigned char)fminf(fmaxf(rintf(c2 * 255.0f), 0.0f), 255.0f);
            q.w = 255;
        }
        reinterpret_cast<uchar4*>(rgba)[idx] = q;
    }
}

// TEX: attr = UVs [Na,2] looked up in atlas [A,A,3] (row 0 is v = 0); else attr = colours [Na,3]
template <bool TEX>
__global__ __launch_bounds__(256) void k_shade_views(const int64_t* __restrict__ fid, const float* __restrict__ bary, int R, long long n,
                                                     const float* __restrict__ attr, int Na, const int32_t* __restrict__ tri, int F,
                                                     const float* __restrict__ atlas, int A, const float* __restrict__ fnorm,
                                                     const float* __restrict__ cams, const float* __restrict__ lights, int L,
                                                     int double_side, float inv_gamma, float* __restrict__ images,
                                                     uint8_t* __restrict__ rgba) {
    const long long RR = (long long)R * R;
    for (long long idx = blockIdx.x * (long long)blockDim.x + threadIdx.x; idx < n; idx += (long long)gridDim.x * blockDim.x) {
        // idx = OUTPUT pixel (v, i, j), row 0 at the top; the rasteriser's row is R - 1 - i
        const int v = (int)(idx / RR);
        const int rem = (int)(idx - (long long)v * RR);
        const int i = rem / R, j = rem - i * R;
        const long long src = (long long)v * RR + (long long)(R - 1 - i) * R + j;
        const long long f = fid[src];
        float c0 = 0.f, c1 = 0.f, c2 = 0.f;
        bool covered = f >= 0 && f < F;
        int i0 = 0, i1 = 0, i2 = 0;
        if (covered) {
            i0 = tri[3 * f]; i1 = tri[3 * f + 1]; i2 = tri[3 * f + 2];
            covered = (unsigned)i0 < (unsigned)Na && (unsigned)i1 < (unsigned)Na && (unsigned)i2 < (unsigned)Na;
        }
        if (covered) {
            const float u = bary[2 * src], w1 = bary[2 * src + 1], w2 = (1.0f - u) - w1;
            if (TEX) {
                const float2 a0 = reinterpret_cast<const float2*>(attr)[i0], a1 = reinterpret_cast<const float2*>(attr)[i1],
                             a2 = reinterpret_cast<const float2*>(attr)[i2];
                float tu = (u * a0.x + w1 * a1.x) + w2 * a2.x;
                float tv = (u * a0.y + w1 * a1.y) + w2 * a2.y;
                tu = tu - floorf(tu);                                                // the reference's `% 1`
                tv = tv - floorf(tv);
                const float hi = (float)(A - 1);
                const float x = fminf(fmaxf(tu * (float)A - 0.5f, 0.0f), hi);        // align_corners=False, clamp to border
                const float y = fminf(fmaxf(tv * (float)A - 0.5f, 0.0f), hi);
                const float xf = floorf(x), yf = floorf(y);
                const int x0 = (int)xf, y0 = (int)yf;
                const int x1 = min(x0 + 1, A - 1), y1 = min(y0 + 1, A - 1);
                const float fx = x - xf, fy = y - yf;
                const float* t00 = atlas + ((size_t)y0 * A + x0) * 3;
                const float* t01 = atlas + ((size_t)y0 * A + x1) * 3;
                const float* t10 = atlas + ((size_t)y1 * A + x0) * 3;
                const float* t11 = atlas + ((size_t)y1 * A + x1) * 3;
                const float top0 = t00[0] + fx * (t01[0] - t00[0]), bot0 = t10[0] + fx * (t11[0] - t10[0]);
                const float top1 = t00[1] + fx * (t01[1] - t00[1]), bot1 = t10[1] + fx * (t11[1] - t10[1]);
                const float top2 = t00[2] + fx * (t01[2] - t00[2]), bot2 = t10[2] + fx * (t11[2] - t10[2]);
                c0 = top0 + fy * (bot0 - top0);
                c1 = top1 + fy * (bot1 - top1);
                c2 = top2 + fy * (bot2 - top2);
            } else {
                const float* a0 = attr + (size_t)i0 * 3;
                const float* a1 = attr + (size_t)i1 * 3;
                const float* a2 = attr + (size_t)i2 * 3;
                c0 = (u * a0[0] + w1 * a1[0]) + w2 * a2[0];
                c1 = (u * a0[1] + w1 * a1[1]) + w2 * a2[1];
                c2 = (u * a0[2] + w1 * a1[2]) + w2 * a2[2];
            }
        }
        shade_finish(covered, c0, c1, c2, f, v, rem, idx, RR, fnorm, cams, lights, L, double_side, inv_gamma, images, rgba);
    }
}

// Per-face materials (pdhip_shade_views_materials): corner UVs through face_uvs_idx (-1 or no table: (0,0)), the material of the face,
// its Kd colour or the lookup of texture_lookup.h in its own W x H u8 image, then the shared tail.  Nothing outside a table is read: a
// face, uv index or material outside its table, or an image that does not lie inside the texel bytes, leaves the pixel uncovered.
__global__ __launch_bounds__(256) void k_shade_views_materials(const int64_t* __restrict__ fid, const float* __restrict__ bary, int R, long long n,
                                                               const float* __restrict__ uvs, int T, const int64_t* __restrict__ face_uvs_idx,
                                                               const int32_t* __restrict__ face_material, int F,
                                                               const uint8_t* __restrict__ texels, long long texel_bytes,
                                                               const int64_t* __restrict__ mat_offset, const int32_t* __restrict__ mat_wh,
                                                               const float* __restrict__ mat_kd, int M, const float* __restrict__ fnorm,
                                                               const float* __restrict__ cams, const float* __restrict__ lights, int L,
                                                               int double_side, float inv_gamma, float* __restrict__ images,
                                                               uint8_t* __restrict__ rgba, int32_t* __restrict__ material_idx) {
    const long long RR = (long long)R * R;
    for (long long idx = blockIdx.x * (long long)blockDim.x + threadIdx.x; idx < n; idx += (long long)gridDim.x * blockDim.x) {
        // idx = OUTPUT pixel (v, i, j), row 0 at the top; the rasteriser's row is R - 1 - i
        const int v = (int)(idx / RR);
        const int rem = (int)(idx - (long long)v * RR);
        const int i = rem / R, j = rem - i * R;
        const long long src = (long long)v * RR + (long long)(R - 1 - i) * R + j;
        const long long f = fid[src];
        float c0 = 0.f, c1 = 0.f, c2 = 0.f;
        bool covered = f >= 0 && f < F;
        int m = 0, W = 0, H = 0;
        long long off = 0;
        if (covered) {
            if (face_material) m = face_material[f];
            covered = (unsigned)m < (unsigned)M;
        }
        if (covered) {
            W = mat_wh[2 * m]; H = mat_wh[2 * m + 1];
            if (W != 0 || H != 0) {                                                  // an image: it must lie inside `texels`
                off = mat_offset[m];
                covered = W > 0 && H > 0 && off >= 0 && off <= texel_bytes && (long long)W * H <= (texel_bytes - off) / 3;
            }
        }
        long long t0 = -1, t1 = -1, t2 = -1;
        if (covered && face_uvs_idx) {
            t0 = face_uvs_idx[3 * f]; t1 = face_uvs_idx[3 * f + 1]; t2 = face_uvs_idx[3 * f + 2];
            covered = t0 >= -1 && t0 < T && t1 >= -1 && t1 < T && t2 >= -1 && t2 < T;
        }
        if (covered) {
            if (W == 0) {                                                            // (then H == 0 too) no image: the Kd colour
                c0 = mat_kd[3 * m]; c1 = mat_kd[3 * m + 1]; c2 = mat_kd[3 * m + 2];
            } else {
                const float u = bary[2 * src], w1 = bary[2 * src + 1], w2 = (1.0f - u) - w1;
                float2 a0 = make_float2(0.f, 0.f), a1 = a0, a2 = a0;                 // (0, 0) where the record has no vt
                if (t0 >= 0) a0 = reinterpret_cast<const float2*>(uvs)[t0];
                if (t1 >= 0) a1 = reinterpret_cast<const float2*>(uvs)[t1];
                if (t2 >= 0) a2 = reinterpret_cast<const float2*>(uvs)[t2];
                const float tu = (u * a0.x + w1 * a1.x) + w2 * a2.x;
                const float tv = (u * a0.y + w1 * a1.y) + w2 * a2.y;
                material_lookup(texels + off, W, H, tu, tv, c0, c1, c2);
            }
        }
        if (material_idx) material_idx[idx] = covered ? m : -1;
        shade_finish(covered, c0, c1, c2, f, v, rem, idx, RR, fnorm, cams, lights, L, double_side, inv_gamma, images, rgba);
    }
}

}  // namespace pdhip

using namespace pdhip;

extern "C" int pdhip_shade_views(const int64_t* face_idxs, const float* bary, int V, int R, const float* attr, int Na, int C,
                                 const int32_t* tri, int F, const float* atlas, int A, const float* face_normals,
                                 const float* cam_params, const float* light_dirs, int L, int double_side, double gamma, float* images,
                                 uint8_t* rgba, void* stream) {
    PD_REQUIRE(face_idxs && bary && attr && tri, "pdhip_shade_views: face_idxs, bary, attr and tri must not be NULL");
    PD_REQUIRE(V > 0 && R > 0 && Na > 0 && F > 0, "pdhip_shade_views: V, R, Na and F must be positive (got %d, %d, %d, %d)", V, R, Na, F);
    PD_REQUIRE(R <= 16384 && V <= 65536, "pdhip_shade_views: R = %d (<= 16384), V = %d (<= 65536)", R, V);
    PD_REQUIRE(C == 2 || C == 3, "pdhip_shade_views: C = %d (2 = UVs looked up in an atlas, 3 = per-vertex colours)", C);
    PD_REQUIRE(C == 3 || (atlas && A > 0), "pdhip_shade_views: UV mode (C = 2) needs an atlas [A,A,3] with A > 0");
    PD_REQUIRE(C == 2 || !atlas, "pdhip_shade_views: per-vertex colours (C = 3) take no atlas");
    PD_REQUIRE(images || rgba, "pdhip_shade_views: images and rgba are both NULL");
    PD_REQUIRE(L >= 0 && L <= SHADE_MAX_LIGHTS, "pdhip_shade_views: L = %d lights (0 .. %d)", L, SHADE_MAX_LIGHTS);
    PD_REQUIRE(L == 0 ? !light_dirs : (light_dirs && face_normals && cam_params),
               "pdhip_shade_views: lighting needs light_dirs [L,3] with L > 0, face_normals [F,3] and cam_params [V,16] together");
    PD_REQUIRE(gamma == 0.0 || (gamma > 0.0 && L > 0), "pdhip_shade_views: gamma = %g (0 = none; > 0 only with lights)", gamma);
    const long long n = (long long)V * R * R;
    const float inv_gamma = gamma > 0.0 ? (float)(1.0 / gamma) : 0.0f;
    const int grid = min(cdiv(n, 256), 65536);
    if (C == 2)
        k_shade_views<true><<<grid, 256, 0, as_stream(stream)>>>(face_idxs, bary, R, n, attr, Na, tri, F, atlas, A, face_normals,
                                                                 cam_params, light_dirs, L, double_side, inv_gamma, images, rgba);
    else
        k_shade_views<false><<<grid, 256, 0, as_stream(stream)>>>(face_idxs, bary, R, n, attr, Na, tri, F, nullptr, 0, face_normals,
                                                                  cam_params, light_dirs, L, double_side, inv_gamma, images, rgba);
    PD_LAUNCH_CHECK();
    return PDHIP_OK;
}

extern "C" int pdhip_shade_views_materials(const int64_t* face_idxs, const float* bary, int V, int R, const float* uvs, int T,
                                           const int64_t* face_uvs_idx, const int32_t* face_material, int F, const uint8_t* texels,
                                           int64_t texel_bytes, const int64_t* mat_offset, const int32_t* mat_wh, const float* mat_kd, int M,
                                           const float* face_normals, const float* cam_params, const float* light_dirs, int L,
                                           int double_side, double gamma, float* images, uint8_t* rgba, int32_t* material_idx,
                                           void* stream) {
    PD_REQUIRE(face_idxs && bary, "pdhip_shade_views_materials: face_idxs and bary must not be NULL");
    PD_REQUIRE(V > 0 && R > 0 && F > 0, "pdhip_shade_views_materials: V, R and F must be positive (got %d, %d, %d)", V, R, F);
    PD_REQUIRE(R <= 16384 && V <= 65536, "pdhip_shade_views_materials: R = %d (<= 16384), V = %d (<= 65536)", R, V);
    PD_REQUIRE(M >= 1 && M <= 255, "pdhip_shade_views_materials: M = %d materials (1 .. 255)", M);
    PD_REQUIRE(mat_offset && mat_wh && mat_kd, "pdhip_shade_views_materials: mat_offset, mat_wh and mat_kd must not be NULL");
    PD_REQUIRE((uvs != nullptr) == (face_uvs_idx != nullptr), "pdhip_shade_views_materials: uvs and face_uvs_idx go together");
    PD_REQUIRE(!uvs || T > 0, "pdhip_shade_views_materials: T = %d uv records (> 0 when uvs is given)", T);
    PD_REQUIRE(texel_bytes >= 0 && (texels || texel_bytes == 0), "pdhip_shade_views_materials: texels is NULL but texel_bytes = %lld",
               (long long)texel_bytes);
    PD_REQUIRE(images || rgba, "pdhip_shade_views_materials: images and rgba are both NULL");
    PD_REQUIRE(L >= 0 && L <= SHADE_MAX_LIGHTS, "pdhip_shade_views_materials: L = %d lights (0 .. %d)", L, SHADE_MAX_LIGHTS);
    PD_REQUIRE(L == 0 ? !light_dirs : (light_dirs && face_normals && cam_params),
               "pdhip_shade_views_materials: lighting needs light_dirs [L,3] with L > 0, face_normals [F,3] and cam_params [V,16] together");
    PD_REQUIRE(gamma == 0.0 || (gamma > 0.0 && L > 0), "pdhip_shade_views_materials: gamma = %g (0 = none; > 0 only with lights)", gamma);
    const long long n = (long long)V * R * R;
    const float inv_gamma = gamma > 0.0 ? (float)(1.0 / gamma) : 0.0f;
    const int grid = min(cdiv(n, 256), 65536);
    k_shade_views_materials<<<grid, 256, 0, as_stream(stream)>>>(face_idxs, bary, R, n, uvs, uvs ? T : 0, face_uvs_idx, face_material, F, texels,
                                                                 (long long)texel_bytes, mat_offset, mat_wh, mat_kd, M, face_normals,
                                                                 cam_params, light_dirs, L, double_side, inv_gamma, images, rgba,
                                                                 material_idx);
    PD_LAUNCH_CHECK();
    return PDHIP_OK;
}
