// The material-image lookup shared by the mesh sampler (sample_mesh.hip, k_smp_draw) and the multi-material shading kernel (render.hip,
// k_shade_views_materials): one definition, so the two cannot drift apart.  Contract: include/pdhip.h under pdhip_sample_mesh
// (sample_colored_pc_from_mesh.py:161-170 and camera_utils.py:455-470 of the reference: (uv % 1) * 2 - 1, v negated,
// grid_sample(align_corners=False, padding_mode='border') on the image as its file stores it, row 0 at the top).
// The units that include this are built with -ffp-contract=off: every operation below rounds once, in the order written.
#pragma once
#include "common.h"

namespace pdhip {

__device__ __forceinline__ float material_texel(const uint8_t* __restrict__ img, int W, int x, int y, int c) {
    return (float)img[((size_t)y * W + x) * 3 + c] / 255.0f;
}

// img: W x H RGB bytes, row-major; (pu, pv): the UV before the wrap.  The caller has checked that the image lies inside its buffer.
__device__ __forceinline__ void material_lookup(const uint8_t* __restrict__ img, int W, int H, float pu, float pv, float& cr, float& cg,
                                                float& cb) {
    const float fu = pu - floorf(pu), fv = pv - floorf(pv);
    const float gx = fu * 2.0f - 1.0f, gy = -(fv * 2.0f - 1.0f);
    float x = ((gx + 1.0f) * (float)W - 1.0f) / 2.0f, y = ((gy + 1.0f) * (float)H - 1.0f) / 2.0f;
    x = fminf(fmaxf(x, 0.0f), (float)(W - 1));
    y = fminf(fmaxf(y, 0.0f), (float)(H - 1));
    if (!(x == x)) x = 0.0f;
    if (!(y == y)) y = 0.0f;
    const int x0 = (int)x, y0 = (int)y, x1 = min(x0 + 1, W - 1), y1 = min(y0 + 1, H - 1);
    const float fx = x - (float)x0, fy = y - (float)y0;
    float out[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float t00 = material_texel(img, W, x0, y0, c), t01 = material_texel(img, W, x1, y0, c);
        const float t10 = material_texel(img, W, x0, y1, c), t11 = material_texel(img, W, x1, y1, c);
        const float top = t00 + fx * (t01 - t00), bot = t10 + fx * (t11 - t10);
        out[c] = top + fy * (bot - top);
    }
    cr = out[0]; cg = out[1]; cb = out[2];
}

}  // namespace pdhip
