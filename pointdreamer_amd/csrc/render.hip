// Shading stage of the evaluation renderer (utils/camera_utils.py:379-554 render_textured_mesh, :735-828 render_per_vertex_color_mesh):
// from the rasteriser's face_idx + barycentrics to a coloured, optionally lit image, in ONE pass per pixel -- attribute interpolation
// (the contract of pdhip_interpolate), `% 1` wrap + bilinear atlas lookup (grid_sample, align_corners=False, padding_mode='border'),
// Lambert lighting with the normal turned towards the camera, clip, gamma, vertical flip, and the 8-bit RGBA form the PNG writer takes.
// No uv_map [V,R,R,2] and no albedo image ever reach HBM.
#include "common.h"

namespace pdhip {

constexpr int SHADE_MAX_LIGHTS = 16;

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
            if (L > 0) {
                float nx = fnorm[3 * f], ny = fnorm[3 * f + 1], nz = fnorm[3 * f + 2];
                const float* cr = cams + (size_t)v * 16 + 6;                         // R[2]: the camera's back axis
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
