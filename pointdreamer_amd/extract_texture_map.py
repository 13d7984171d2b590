"""UV-atlas producer: the reference's models/get3d/extract_texture_map.xatlas_uvmap_w_face_id
(models/get3d/extract_texture_map.py:42-64).  `uv_unwrap` replaces the chart parametrisation (`xatlas.parametrize`,
CPU third-party) with the device unwrap of csrc/uv_atlas.hip; `uvmap_w_face_id` is the rasterise-in-UV-space + interpolate half,
for callers that bring their own `uvs` / `mesh_tex_idx`.
Returns the wire format of demo.py:445-448: uvs, mesh_tex_idx, gb_pos[1,R,R,3], mask[1,R,R,1], per_atlas_pixel_face_id[1,R,R]."""
import torch

from . import _lib
from ._lib import ptr, as_u8, stream, check, PdhipError


def rasterize(pos, tri, resolution):
    """pos [V,Vn,4] f32 clip-space (w = 1), tri [F,3] -> face_idx [V,R,R] i64 (-1 empty), bary [V,R,R,2], depth, mask."""
    L = _lib.lib()
    pos = pos.float().contiguous()
    tri32 = tri.to(torch.int32).contiguous()
    V, Vn = pos.shape[:2]
    R = int(resolution)
    dev = pos.device
    zkey = torch.empty(((L.pdhip_raster_mesh_ws_bytes(V, tri32.shape[0], R) + 7) // 8,), dtype=torch.int64, device=dev)
    hard = torch.empty((V, R, R), dtype=torch.bool, device=dev)
    fidx = torch.empty((V, R, R), dtype=torch.int64, device=dev)
    depth = torch.empty((V, R, R), device=dev)
    check(L.pdhip_raster_mesh_ws(ptr(pos), V, Vn, ptr(tri32), tri32.shape[0], R, ptr(zkey), zkey.numel() * 8, ptr(as_u8(hard)), ptr(fidx),
                                 ptr(depth), stream()), 'pdhip_raster_mesh')
    bary = torch.empty((V, R, R, 2), device=dev)
    check(L.pdhip_raster_barycentrics(ptr(pos), V, Vn, ptr(tri32), R, ptr(fidx), ptr(bary), stream()), 'pdhip_raster_barycentrics')
    return fidx, bary, depth, hard


def interpolate(attr, fidx, bary, tri):
    """nvdiffrast.interpolate(attr[None], rast, tri): attr [Na,C], tri [F,3] -> [V,R,R,C]."""
    L = _lib.lib()
    attr = attr.float().contiguous()
    tri32 = tri.to(torch.int32).contiguous()
    C = attr.shape[1]
    out = torch.empty(tuple(fidx.shape) + (C,), device=attr.device)
    check(L.pdhip_interpolate(ptr(attr), C, ptr(tri32), ptr(fidx.contiguous()), ptr(bary.contiguous()), fidx.numel(), ptr(out),
                              stream()), 'pdhip_interpolate')
    return out


def uvmap_w_face_id(mesh_v, mesh_pos_idx, uvs, mesh_tex_idx, resolution):
    """extract_texture_map.py:48-64 given the parametrisation: rasterise the UV triangles, interpolate world positions."""
    uv_clip = uvs.float()[None] * 2.0 - 1.0
    uv_clip4 = torch.cat((uv_clip, torch.zeros_like(uv_clip[..., 0:1]), torch.ones_like(uv_clip[..., 0:1])), dim=-1).contiguous()
    fidx, bary, _, hard = rasterize(uv_clip4, mesh_tex_idx, resolution)
    gb_pos = interpolate(mesh_v, fidx, bary, mesh_pos_idx)
    return uvs, mesh_tex_idx, gb_pos, hard.unsqueeze(-1), fidx


def uv_unwrap(mesh_v, mesh_pos_idx, resolution, gutter=2, return_charts=False):
    """Chart-based UV parametrisation on the device (pdhip_uv_atlas): mesh_v [Vn,3], mesh_pos_idx [F,3] -> uvs [T,2] f32 in [0,1]
    (one entry per (chart, vertex) pair), mesh_tex_idx [F,3] i64, and face_chart [F] i32 with return_charts=True.  Charts group
    faces of one dominant signed normal axis, each projected orthographically onto that axis's plane at one common texel density
    and shelf-packed into a resolution x resolution atlas with `gutter` texels around every chart; no texel centre lies in two
    UV triangles.  Device tensors only."""
    if not (torch.is_tensor(mesh_v) and torch.is_tensor(mesh_pos_idx) and mesh_v.is_cuda and mesh_pos_idx.is_cuda):
        raise PdhipError("uv_unwrap needs mesh_v and mesh_pos_idx on the GPU (cuda:N == HIP device); there is no CPU path")
    if mesh_v.dim() != 2 or mesh_v.shape[1] != 3 or mesh_pos_idx.dim() != 2 or mesh_pos_idx.shape[1] != 3:
        raise PdhipError(f"uv_unwrap: expected mesh_v [Vn,3] and mesh_pos_idx [F,3], got {tuple(mesh_v.shape)} / {tuple(mesh_pos_idx.shape)}")
    L = _lib.lib()
    v = mesh_v.detach().float().contiguous()
    f = mesh_pos_idx.detach().to(torch.int64).contiguous()
    Vn, F, dev = v.shape[0], f.shape[0], v.device
    ws = torch.empty((max(1, L.pdhip_uv_atlas_ws_bytes(Vn, F)),), dtype=torch.uint8, device=dev)
    uvs = torch.empty((max(1, 3 * F), 2), dtype=torch.float32, device=dev)
    tex_idx = torch.empty((F, 3), dtype=torch.int64, device=dev)
    face_chart = torch.empty((F,), dtype=torch.int32, device=dev)
    counts = torch.zeros((4,), dtype=torch.int32, device=dev)
    check(L.pdhip_uv_atlas(ptr(v, torch.float32), Vn, ptr(f, torch.int64), F, int(resolution), int(gutter), ptr(uvs), ptr(tex_idx),
                           ptr(face_chart), ptr(counts), ptr(ws), stream()), 'pdhip_uv_atlas')
    T = int(counts.cpu()[0])
    uvs = uvs[:T].contiguous()
    return (uvs, tex_idx, face_chart) if return_charts else (uvs, tex_idx)


def xatlas_uvmap_w_face_id(ctx, mesh_v, mesh_pos_idx, resolution):
    """extract_texture_map.py:42-64 with the reference's name, arguments and 5-tuple: (uvs [T,2], mesh_tex_idx [F,3], gb_pos [1,R,R,3],
    mask [1,R,R,1], per_atlas_pixel_face_id [1,R,R]).  `ctx` (the nvdiffrast context) is ignored.  The chart layout is this project's
    own device unwrap (uv_unwrap), NOT xatlas's: charts, their placement and the number of UV entries differ from what
    xatlas.parametrize would return; the wire format and the contract of the atlas (every texel of the mask maps to one face) are
    the same."""
    uvs, tex_idx = uv_unwrap(mesh_v, mesh_pos_idx, resolution)
    return uvmap_w_face_id(mesh_v, mesh_pos_idx, uvs, tex_idx, resolution)
