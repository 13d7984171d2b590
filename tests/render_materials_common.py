"""Float64 reference, float32 emulation and error model of the multi-material shading kernel (pdhip_shade_views_materials,
csrc/render.hip) -- numpy only, nothing here touches the GPU or the product's kernel.

Reference: render_common.interpolate64 over the corner UVs with (0,0) where face_uvs_idx is -1 (a padded uv row, as the reference
renderer does), sample_pc_common.lookup64 per material on the image as its file stores it, the Kd colour for a material without an
image, then the lighting, clip, gamma, vertical flip and zero background of render_common.render_reference.

Error model (u = 2^-24, the float32 unit roundoff; every rounding is at most u times the magnitude of its result):
  * interpolation uv = (u0*a0 + u1*a1) + u2*a2 with u2 = (1-u0)-u1: two roundings in u2, three products, two sums, all of values
    <= M = max(1, max|uv|): 7 M u;
  * the lookup's coordinate, x = ((gx+1) W - 1)/2 with gx = fr*2 - 1, fr = uv - floor(uv): fr rounds once (u; exact for uv >= 0),
    *2 is exact, -1 rounds once (u), the negation of gy is exact, +1 once (2u, the result is <= 2), *W once (2 W u), -1 once
    (2 W u), /2 is exact.  Carried through: x is within W (14 M u + 2u + u + 2u)/2 + (2 W u + 2 W u)/2 = (7 M + 4.5) W u <=
    11.5 W M u of its float64 value.  The issue counts 7 + 5 roundings of values <= 2 W M, halved: e_t = 12 max(W,H) M u texels;
    the count above confirms it with 0.5 W M u to spare, and e_t is used as the issue states it;
  * the blend top + fy (bot - top), top = t00 + fx (t01 - t00) is bilinear with slope <= D in either coordinate (D =
    sample_pc_common.texel_spread: the spread of the footprint's 2 x 2 block grown by one texel on every side): 2 e_t D.  Its own
    arithmetic: t/255.0f rounds once (u), the two final additions of values <= 1 round twice each way (4u), one spare: 6u.  The
    differences and products inside are relative to D (<= 4 u D) and sit in the 0.5 W M u spare of e_t (2 * 0.5 W u D >= 8 u D for
    W >= 8, the smallest image used).  Colour error <= 2 e_t D + 6u;
  * a Kd material: the colour is mat_kd bit for bit -- bound 0;
  * seam pixels: where float64 frac(uv) lies within e_t / W (u) or e_t / H (v) of 0 or 1 the wrap may land on the other side in
    float32 and the lookup jumps: left out.  Exception: a pixel whose three corner UVs are identical is never left out and is held
    to 6u of the lookup at that UV.  In the fixture such faces are exactly the `-1` faces, whose UV is 0 in both precisions
    (0 * w is exact), so the blend degenerates to one texel (fx = fy = 0 after the clamp) and only t/255.0f rounds;
    test_render_materials_cpu asserts that every identical-corner pixel has uv == 0.
"""
import numpy as np

import render_common as rc
import sample_pc_common as spc

U = rc.U
F32 = np.float32
CAP = 0.005                                                  # at most 0.5 % of the covered pixels may be left out (a condition)


# ----------------------------------------------------------------------------- fixture
def fixture():
    """sample_pc_common.fixture() (icosphere(4), 320 faces, wrapped UVs, -1 on every 11th face, materials f % 3: 32 x 16 image, Kd,
    8 x 8 image) rendered with ALL faces (`keep` is ignored) at V = 3, R = 64 with the three lights of render_common.sphere_fixture."""
    fx = dict(spc.fixture())
    fx.update(V=3, R=64, lights=rc.sphere_fixture()['lights'])
    return fx


def padded_uvs(uvs, face_uvs_idx, F):
    """(uv table with a trailing (0,0) row, [F,3] indices with -1 -> that row): the reference's own padding (:397, :427-428)."""
    if uvs is None or face_uvs_idx is None:
        return np.zeros((1, 2), np.float64), np.zeros((F, 3), np.int64)
    uvs = np.asarray(uvs, F32).astype(np.float64)
    idx = np.asarray(face_uvs_idx, np.int64)
    return np.concatenate([uvs, np.zeros((1, 2))]), np.where(idx < 0, len(uvs), idx)


# ----------------------------------------------------------------------------- float64 reference
def reference(fid, bary, uvs, face_uvs_idx, face_material, materials, normals=None, cam_params=None, lights=None, double_side=False,
              gamma=None):
    """float64 reference from the (unflipped) face_idx [V,R,R] / bary [V,R,R,2].  Returns a dict, everything flipped vertically:
    images / pre_gamma [V,3,R,R], albedo [V,R,R,3], mask, material [V,R,R] (-1 uncovered), uv, frac [V,R,R,2], D, e_t, bound
    [V,R,R] (the albedo bound per pixel), same3 (identical corner UVs), excluded (seam pixels left out); with lights also clipsum
    and ndotcam."""
    fid = np.asarray(fid)
    F = len(face_material) if face_material is not None else int(fid.max()) + 1
    mask = fid >= 0
    fsafe = np.where(mask, fid, 0)
    fm = np.zeros(F, np.int64) if face_material is None else np.asarray(face_material, np.int64)
    mat = np.where(mask, fm[fsafe], -1)
    table, tri = padded_uvs(uvs, face_uvs_idx, F)
    a = rc.interpolate64(table, tri, fid, bary)                                          # [V,R,R,2], zeros where empty
    corner = table[tri]                                                                  # [F,3,2]
    same3 = mask & (np.all(corner[:, 0] == corner[:, 1], -1) & np.all(corner[:, 0] == corner[:, 2], -1))[fsafe]
    frac = a - np.floor(a)
    M = max(1.0, float(np.abs(a[mask]).max())) if mask.any() else 1.0
    alb = np.zeros(fid.shape + (3,))
    D = np.zeros(fid.shape)
    e_t = np.zeros(fid.shape)
    near = np.zeros(fid.shape, bool)
    for m, material in enumerate(materials):
        sel = mat == m
        if 'map_Kd' not in material:
            alb[sel] = np.asarray(material['Kd'], F32).astype(np.float64)
            continue
        img = np.asarray(material['map_Kd'])
        H, W = img.shape[:2]
        col, x0, y0 = spc.lookup64(img, a[sel])
        alb[sel] = col
        D[sel] = spc.texel_spread(img, x0, y0)
        e = 12.0 * max(W, H) * M * U
        e_t[sel] = e
        fr = frac[sel]
        near[sel] = (fr[:, 0] < e / W) | (fr[:, 0] > 1.0 - e / W) | (fr[:, 1] < e / H) | (fr[:, 1] > 1.0 - e / H)
    textured = e_t > 0
    bound = np.where(textured, np.where(same3, 6.0 * U, 2.0 * e_t * D + 6.0 * U), 0.0)
    out = dict(uv=a[:, ::-1], frac=frac[:, ::-1], D=D[:, ::-1], e_t=e_t[:, ::-1], bound=bound[:, ::-1], same3=same3[:, ::-1],
               excluded=(textured & near & ~same3)[:, ::-1], material=mat[:, ::-1], M=M)
    img_ = alb
    if lights is not None:                                                               # render_common.render_reference's lighting
        n = np.asarray(normals, np.float64)[fsafe]
        back = np.asarray(cam_params, np.float64)[:, 6:9]
        ndc = (n * back[:, None, None, :]).sum(-1)
        n = np.where((ndc < 0)[..., None], -n, n)
        img_ = np.zeros_like(alb)
        clipsum = np.zeros(mask.shape)
        for l in np.asarray(lights, np.float64):
            d = (n * l).sum(-1)
            if double_side:
                d = np.abs(d)
            d = np.clip(d, 0, 1)
            img_ = img_ + alb * d[..., None]
            clipsum += d
        img_ = np.clip(img_ * mask[..., None], 0, 1)
        out.update(clipsum=clipsum[:, ::-1], ndotcam=ndc[:, ::-1])
    pre = img_
    if lights is not None and gamma is not None:
        img_ = img_ ** (1.0 / gamma)
    chw = lambda x: np.ascontiguousarray(x[:, ::-1].transpose(0, 3, 1, 2))
    out.update(images=chw(img_), pre_gamma=chw(pre), albedo=np.ascontiguousarray(alb[:, ::-1]), mask=np.ascontiguousarray(mask[:, ::-1]))
    return {k: (np.ascontiguousarray(v) if isinstance(v, np.ndarray) else v) for k, v in out.items()}


# ----------------------------------------------------------------------------- float32 emulation of the kernel, operation for operation
def lookup32(img, tu, tv):
    """csrc/texture_lookup.h in numpy float32: one rounding per operation, in the kernel's order."""
    img = np.asarray(img)
    H, W = img.shape[:2]
    one, two = F32(1.0), F32(2.0)
    fu, fv = tu - np.floor(tu), tv - np.floor(tv)
    gx, gy = fu * two - one, -(fv * two - one)
    x = ((gx + one) * F32(W) - one) / two
    y = ((gy + one) * F32(H) - one) / two
    x = np.minimum(np.maximum(x, F32(0)), F32(W - 1))
    y = np.minimum(np.maximum(y, F32(0)), F32(H - 1))
    x0, y0 = x.astype(np.int64), y.astype(np.int64)
    x1, y1 = np.minimum(x0 + 1, W - 1), np.minimum(y0 + 1, H - 1)
    fx, fy = (x - x0.astype(F32))[:, None], (y - y0.astype(F32))[:, None]
    t = img.astype(F32) / F32(255.0)
    top = t[y0, x0] + fx * (t[y0, x1] - t[y0, x0])
    bot = t[y1, x0] + fx * (t[y1, x1] - t[y1, x0])
    out = top + fy * (bot - top)
    assert out.dtype == F32
    return out


def emulate32(fid, bary, uvs, face_uvs_idx, face_material, materials):
    """The kernel's albedo [V,R,R,3] float32 (flipped, 0 where uncovered) from the unflipped raster: (u*a0 + w1*a1) + w2*a2 with
    w2 = (1-u) - w1 over the corner UVs ((0,0) at -1), the Kd colour or lookup32."""
    fid = np.asarray(fid)
    mask = fid >= 0
    F = len(face_material)
    f = fid[mask]
    table, tri = padded_uvs(uvs, face_uvs_idx, F)
    table = table.astype(F32)
    b = np.asarray(bary, F32)[mask]
    u, w1 = b[:, 0:1], b[:, 1:2]
    w2 = (F32(1.0) - u) - w1
    a0, a1, a2 = table[tri[f, 0]], table[tri[f, 1]], table[tri[f, 2]]
    uv = (u * a0 + w1 * a1) + w2 * a2
    assert uv.dtype == F32
    mat = np.asarray(face_material, np.int64)[f]
    col = np.zeros((len(f), 3), F32)
    for m, material in enumerate(materials):
        sel = mat == m
        if 'map_Kd' in material:
            col[sel] = lookup32(material['map_Kd'], uv[sel, 0], uv[sel, 1])
        else:
            col[sel] = np.asarray(material['Kd'], F32)
    out = np.zeros(fid.shape + (3,), F32)
    out[mask] = col
    return np.ascontiguousarray(out[:, ::-1])


# ----------------------------------------------------------------------------- files
def write_obj(path, verts, faces, uvs, face_uvs_idx, face_material, materials, mtl_name=None):
    """OBJ (%.9g: float32 round-trips) + MTL + one PNG per image, faces in their own order with a `usemtl` wherever the material
    changes; a -1 corner is written without a vt index."""
    import os
    import PIL.Image
    here, stem = os.path.dirname(str(path)), os.path.splitext(os.path.basename(str(path)))[0]
    mtl_name = mtl_name or stem + '.mtl'
    with open(os.path.join(here, mtl_name), 'w') as f:
        for m in materials:
            f.write(f"newmtl {m['name']}\n")
            if 'map_Kd' in m:
                PIL.Image.fromarray(np.asarray(m['map_Kd'], np.uint8), 'RGB').save(os.path.join(here, f"{stem}_{m['name']}.png"))
                f.write(f"Kd 1 1 1\nmap_Kd {stem}_{m['name']}.png\n")
            else:
                f.write('Kd %.9g %.9g %.9g\n' % tuple(np.asarray(m['Kd'], F32)))
    with open(str(path), 'w') as f:
        f.write(f'mtllib {mtl_name}\n')
        for p in np.asarray(verts, F32):
            f.write('v %.9g %.9g %.9g\n' % tuple(p))
        for t in np.asarray(uvs, F32):
            f.write('vt %.9g %.9g\n' % tuple(t))
        cur = None
        for k, tri in enumerate(np.asarray(faces)):
            m = 0 if face_material is None else int(face_material[k])
            if m != cur:
                f.write(f"usemtl {materials[m]['name']}\n")
                cur = m
            f.write('f ' + ' '.join(f'{a + 1}/{t + 1}' if t >= 0 else f'{a + 1}' for a, t in zip(tri, face_uvs_idx[k])) + '\n')
