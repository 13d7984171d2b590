// The rasteriser's coverage rules (raster.hip), shared with the UV-atlas overlap check (uv_atlas.hip) so that both decide
// "texel centre covered by triangle" identically: 1/256-pixel snapped vertices, int64 edge functions at pixel centres,
// the top-left-style tie rule of the watertight rasteriser.  Include from translation units compiled with -ffp-contract=off.
#pragma once
#include "common.h"

#define SUBPIX 256
#define FIX_CLAMP (1 << 24)

namespace pdhip {

__device__ __forceinline__ long long snap_fix(float ndc, int R) {
    float v = (ndc * 0.5f + 0.5f) * (float)(R * SUBPIX);
    if (!(fabsf(v) <= 3.0e38f)) v = 0.f;           // NaN / inf -> 0
    v = rintf(v);
    v = fminf(fmaxf(v, (float)(-FIX_CLAMP)), (float)FIX_CLAMP);
    return (long long)v;
}

__device__ __forceinline__ long long floor_div(long long a, long long b) {   // b > 0
    long long q = a / b;
    return (a % b != 0 && a < 0) ? q - 1 : q;
}

// A snapped triangle with positive winding: vertex k at (x[k], y[k]) in 1/SUBPIX pixel units.
struct SnapTri {
    long long x0, y0, x1, y1, x2, y2;
    long long area;                                // twice the snapped area (> 0), 0 for a degenerate triangle
    bool swapped;                                  // vertices 1 and 2 were exchanged to make the winding positive
};

// Snap three NDC vertices; swaps vertices 1 and 2 when the winding is negative (as the rasteriser does).
__device__ __forceinline__ SnapTri snap_tri(float ax, float ay, float bx, float by, float cx, float cy, int R) {
    SnapTri t;
    t.x0 = snap_fix(ax, R); t.y0 = snap_fix(ay, R);
    t.x1 = snap_fix(bx, R); t.y1 = snap_fix(by, R);
    t.x2 = snap_fix(cx, R); t.y2 = snap_fix(cy, R);
    t.area = (t.x1 - t.x0) * (t.y2 - t.y0) - (t.y1 - t.y0) * (t.x2 - t.x0);
    t.swapped = t.area < 0;
    if (t.swapped) {
        long long q;
        q = t.x1; t.x1 = t.x2; t.x2 = q;
        q = t.y1; t.y1 = t.y2; t.y2 = q;
        t.area = -t.area;
    }
    return t;
}

// Pixel bounding box [jmin, jmax] x [imin, imax] of the pixel centres a triangle can cover, clipped to the R x R image
// (empty when jmin > jmax or imin > imax).
__device__ __forceinline__ void snap_tri_box(const SnapTri& t, int R, int& jmin, int& jmax, int& imin, int& imax) {
    const long long minx = min(t.x0, min(t.x1, t.x2)), maxx = max(t.x0, max(t.x1, t.x2));
    const long long miny = min(t.y0, min(t.y1, t.y2)), maxy = max(t.y0, max(t.y1, t.y2));
    jmin = (int)max(0ll, -floor_div(-(minx - 128), SUBPIX));
    jmax = (int)min((long long)R - 1, floor_div(maxx - 128, SUBPIX));
    imin = (int)max(0ll, -floor_div(-(miny - 128), SUBPIX));
    imax = (int)min((long long)R - 1, floor_div(maxy - 128, SUBPIX));
}

// Coverage of the centre of pixel (j, i) by a snapped triangle of positive winding: every edge function positive, or zero on an
// edge the tie rule includes (edge k runs between the two vertices other than k; weight of v0 <- edge v1->v2, v1 <- v2->v0, v2 <- v0->v1).
__device__ __forceinline__ bool snap_tri_covers(const SnapTri& t, int j, int i, long long& E0, long long& E1, long long& E2) {
    const long long dx0 = t.x2 - t.x1, dy0 = t.y2 - t.y1;
    const long long dx1 = t.x0 - t.x2, dy1 = t.y0 - t.y2;
    const long long dx2 = t.x1 - t.x0, dy2 = t.y1 - t.y0;
    const bool inc0 = (dy0 > 0) || (dy0 == 0 && dx0 > 0);
    const bool inc1 = (dy1 > 0) || (dy1 == 0 && dx1 > 0);
    const bool inc2 = (dy2 > 0) || (dy2 == 0 && dx2 > 0);
    const long long px = (long long)j * SUBPIX + 128, py = (long long)i * SUBPIX + 128;
    E0 = dx0 * (py - t.y1) - dy0 * (px - t.x1);
    E1 = dx1 * (py - t.y2) - dy1 * (px - t.x2);
    E2 = dx2 * (py - t.y0) - dy2 * (px - t.x0);
    return (E0 > 0 || (E0 == 0 && inc0)) && (E1 > 0 || (E1 == 0 && inc1)) && (E2 > 0 || (E2 == 0 && inc2));
}

}  // namespace pdhip
