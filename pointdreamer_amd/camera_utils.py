"""Cameras for the texturing path (row C0).  Mirrors the interface of the reference's
utils/camera_utils.py:86-245 (`fibonacci_sphere`, `calculate_up_vector`, `create_cameras`) but the
camera object is a plain 16-float struct consumed by the HIP kernels instead of a kaolin Camera:
R (9, row-major world->camera), t (3), fx, fy, A, B  with  NDC = (fx*xc/-zc, fy*yc/-zc, (A*zc+B)/-zc),
vertical fov pi/4, near 1e-2, far 1e2 (kaolin's defaults; kaolin itself is not a dependency).
"""
import math
import numpy as np
import torch


def fibonacci_sphere(samples, radius):
    pts = []
    phi = math.pi * (3. - math.sqrt(5.))
    for i in range(samples):
        y = 1 - (i / float(samples - 1)) * 2
        ry = math.sqrt(1 - y * y)
        th = phi * i
        pts.append((math.cos(th) * ry * radius, y * radius, math.sin(th) * ry * radius))
    return np.array(pts)


def calculate_up_vector(eye_position, target_position, world_up=None):
    gaze = target_position - eye_position
    if world_up is None:
        world_up = np.array([0, 1, 0])
    if np.allclose(np.cross(gaze, world_up), 0):
        return np.array([0.0, 0.0, 1.0])
    side = np.cross(gaze, world_up)
    up = np.cross(side, gaze)
    return up / np.linalg.norm(up)


def look_at_params(eye, at, up, fov=math.pi / 4, near=1e-2, far=1e2):
    eye, at, up = (np.asarray(a, np.float64) for a in (eye, at, up))
    back = eye - at
    back /= np.linalg.norm(back)
    right = np.cross(up, back)
    right /= np.linalg.norm(right)
    up2 = np.cross(back, right)
    R = np.stack([right, up2, back], 0)
    t = -R @ eye
    f = 1.0 / math.tan(fov / 2.0)
    return np.concatenate([R.reshape(9), t, [f, f, -(far + near) / (far - near), -2.0 * far * near / (far - near)]]
                          ).astype(np.float32)


class Camera:
    """Drop-in for the kaolin Camera as far as the hot path uses it: .transform, .height, .width."""

    def __init__(self, params, res, device):
        self.params = torch.as_tensor(params, dtype=torch.float32).reshape(16).to(device).contiguous()
        self.height = self.width = int(res)

    def transform(self, pts):
        from .ours_utils import transform_points
        return transform_points([self], pts)[0]


def stack_params(cams):
    from . import _lib
    return _lib.memo([c.params for c in cams], 'stack_params', lambda ps: torch.stack(list(ps), 0).contiguous())


def _dodecahedron():
    phi = (1 + math.sqrt(5)) / 2.
    return np.array([[-1, -1, -1], [1, -1, -1], [1, 1, -1], [-1, 1, -1], [-1, -1, 1], [1, -1, 1], [1, 1, 1], [-1, 1, 1],
                     [0, -phi, -1 / phi], [0, -phi, 1 / phi], [0, phi, -1 / phi], [0, phi, 1 / phi],
                     [-1 / phi, 0, -phi], [-1 / phi, 0, phi], [1 / phi, 0, -phi], [1 / phi, 0, phi],
                     [-phi, -1 / phi, 0], [-phi, 1 / phi, 0], [phi, -1 / phi, 0], [phi, 1 / phi, 0]]).astype(float)


def create_cameras(num_views=8, distance=1.6, res=512, distribution='fibonacci_sphere',
                   device=torch.device('cuda'), vis=False):
    """Same return contract as the reference: cams, base_dirs[V,3], eye_positions (numpy), up_dirs[V,3]."""
    if distribution not in ('fibonacci_sphere', 'self_defined', 'blender', 'exact_blender'):
        raise ValueError(f"camera distribution {distribution!r} (camera_utils.py:129: fibonacci_sphere, self_defined, blender, exact_blender)")
    fov = math.pi * 45 / 180
    if distribution == 'fibonacci_sphere':
        eyes = fibonacci_sphere(num_views, distance)
    elif distribution in ('blender', 'exact_blender'):
        # camera_utils.py:132-164: the 20 vertices of a dodecahedron, 1.2 x its circumradius away, y-up -> z-up; always 20 views
        num_views = 20
        eyes = (_dodecahedron() * 1.2).dot(np.array([[1, 0, 0], [0, 0, 1], [0, -1, 0.0]]).T)
        if distribution == 'exact_blender':
            fov = 0.8575560450553894
    else:
        # camera_utils.py:165-201: six axis views at `distance`, or the raw dodecahedron vertices
        if num_views == 6:
            eyes = distance * np.array([[0, 0, -1.0], [0, 0, 1.0], [0, -1.0, 0], [0, 1.0, 0], [-1.0, 0, 0], [1.0, 0, 0]])
        elif num_views == 20:
            eyes = _dodecahedron()
        else:
            raise ValueError("camera distribution 'self_defined' knows 6 or 20 views (camera_utils.py:165-201)")
    cams = []
    base_dirs = torch.zeros((num_views, 3), dtype=torch.float32)
    up_dirs = torch.zeros((num_views, 3), dtype=torch.float32)
    at = np.array([0, 0, 0])
    for i, eye in enumerate(eyes):
        up = calculate_up_vector(eye, at)
        cams.append(Camera(look_at_params(eye, at, up, fov=fov), res, device))
        base_dirs[i] = torch.tensor(eye - at).float()
        up_dirs[i] = torch.tensor(up).float()
    return cams, base_dirs.to(device), eyes, up_dirs.to(device)


def get_cam_Ks_RTs_from_locations(cam_locations):
    """camera_utils.py:940-985: world -> camera [R | t] (rows U, V, N = right, up, look direction) of cameras at `cam_locations`
    [V,3] looking at the origin, y-up (z-up when the view direction is vertical), and the fixed 512-pixel intrinsics.
    Returns (cam_K [3,3], cam_RTs [V,3,4]) as float64 numpy arrays."""
    loc = cam_locations.detach().cpu().numpy() if torch.is_tensor(cam_locations) else np.asarray(cam_locations)
    loc = loc.astype(np.float64)
    cam_RTs = np.zeros((len(loc), 3, 4))
    target = np.array([0.0, 0.0, 0.0])
    for i, eye in enumerate(loc):
        N = target - eye
        N = N / np.linalg.norm(N)
        up = np.array([0.0, 0.0, 1.0]) if (N[0] == 0 and N[2] == 0) else np.array([0.0, 1.0, 0.0])
        U = np.cross(N, up)
        U = U / np.linalg.norm(U)
        V = np.cross(U, N)
        V = V / np.linalg.norm(V)
        cam_RTs[i] = np.array([[U[0], U[1], U[2], np.dot(-U, eye)],
                               [V[0], V[1], V[2], np.dot(-V, eye)],
                               [N[0], N[1], N[2], np.dot(-N, eye)]])
    cam_K = np.array([[560.0, 0, 256], [0, 560, 256], [0, 0, 1]])
    return cam_K, cam_RTs


# ----------------------------------------------------------------------------- evaluation renderers (camera_utils.py:251-828)
def _clip_positions(cams, vertices):
    """pos [V,Vn,4] = (cam.transform(vertices), 1) for every camera (pdhip_project_points), and the stacked camera parameters."""
    from . import _lib
    from ._lib import ptr, stream, check
    L = _lib.lib()
    V, Vn, dev = len(cams), vertices.shape[0], vertices.device
    cp = stack_params(cams)
    pos = torch.empty((V, Vn, 4), device=dev)
    vuv = torch.empty((V, Vn, 2), device=dev)
    ws = torch.empty((4 * V,), dtype=torch.int32, device=dev)
    check(L.pdhip_project_points(ptr(cp), V, ptr(vertices), Vn, None, 0, 0, 0.0, ptr(pos), ptr(vuv), None, None, None, None,
                                 ptr(ws), stream()), 'pdhip_project_points')
    return pos, cp


def _normalized(vertices):
    """camera_utils.py:432-436 on a copy: centre of the bounding box to the origin, largest extent to 1."""
    vmin, vmax = vertices.min(0)[0], vertices.max(0)[0]
    return (vertices - (vmax + vmin) / 2.) / (vmax - vmin).max()


def face_normals_unit(vertices, faces):
    """kal.ops.mesh.face_normals(unit=True) (camera_utils.py:392): [F,3] on the device."""
    fv = vertices[faces.long()]
    n = torch.cross(fv[:, 1] - fv[:, 0], fv[:, 2] - fv[:, 0], dim=1)
    return (n / n.norm(dim=1, keepdim=True).clamp_min(1e-30)).float().contiguous()


def shade_views(face_idxs, bary, attr, tri, atlas=None, face_normals=None, cam_params=None, light_dirs=None, double_side=False,
                gamma=None, want_images=True, want_rgba=False):
    """pdhip_shade_views: face_idxs [V,R,R] i64 / bary [V,R,R,2] as rasterize() returns them, attr [Na,2] UVs with atlas [A,A,3]
    (row 0 is v = 0) or attr [Na,3] colours, tri [F,3] -> (images [V,3,R,R] f32 or None, rgba [V,R,R,4] u8 or None), both with
    row 0 at the top.  Lighting only when light_dirs [L,3] is given (then face_normals [F,3] and cam_params [V,16] as well)."""
    from . import _lib
    from ._lib import ptr, stream, check
    L = _lib.lib()
    dev = face_idxs.device
    V, R = face_idxs.shape[0], face_idxs.shape[1]
    if face_idxs.shape[2] != R:
        raise ValueError(f"shade_views: square views only, got {tuple(face_idxs.shape)}")
    if tuple(bary.shape) != (V, R, R, 2):
        raise ValueError(f"shade_views: bary must be [V,R,R,2] = {(V, R, R, 2)}, got {tuple(bary.shape)}")
    attr = attr.float().contiguous()
    tri32 = tri.to(torch.int32).contiguous()
    if attr.dim() != 2 or tri32.dim() != 2 or tri32.shape[1] != 3:
        raise ValueError(f"shade_views: attr [Na,C] and tri [F,3] expected, got {tuple(attr.shape)} / {tuple(tri32.shape)}")
    C = attr.shape[1]
    A = 0
    if atlas is not None:
        atlas = atlas.float().contiguous()
        if atlas.dim() != 3 or atlas.shape[0] != atlas.shape[1] or atlas.shape[2] != 3:
            raise ValueError(f"shade_views: atlas must be [A,A,3], got {tuple(atlas.shape)}")
        A = atlas.shape[0]
    nl = 0
    if light_dirs is not None:
        light_dirs = torch.as_tensor(light_dirs, dtype=torch.float32, device=dev).reshape(-1, 3).contiguous()
        nl = light_dirs.shape[0]
        if face_normals is None or cam_params is None:
            raise ValueError("shade_views: light_dirs needs face_normals and cam_params")
        face_normals = face_normals.float().contiguous()
        if face_normals.shape[0] != tri32.shape[0]:
            raise ValueError("shade_views: one face normal per face")
        cam_params = cam_params.float().contiguous()
        if tuple(cam_params.shape) != (V, 16):
            raise ValueError(f"shade_views: cam_params must be [V,16], got {tuple(cam_params.shape)}")
    else:
        face_normals = cam_params = None
    images = torch.empty((V, 3, R, R), device=dev) if want_images else None
    rgba = torch.empty((V, R, R, 4), dtype=torch.uint8, device=dev) if want_rgba else None
    check(L.pdhip_shade_views(ptr(face_idxs.contiguous(), torch.int64), ptr(bary.contiguous(), torch.float32), V, R, ptr(attr), attr.shape[0], C,
                              ptr(tri32), tri32.shape[0], ptr(atlas, allow_none=True), A, ptr(face_normals, allow_none=True),
                              ptr(cam_params, allow_none=True), ptr(light_dirs, allow_none=True), nl, int(bool(double_side)),
                              float(gamma) if (gamma is not None and nl) else 0.0, ptr(images, allow_none=True),
                              ptr(rgba, allow_none=True), stream()), 'pdhip_shade_views')
    return images, rgba


def check_packed_materials(materials):
    """Host-side check of a packed material set (texels u8 [B], mat_offset i64 [M], mat_wh i32 [M,2], mat_kd f32 [M,3], the four
    tensors of sample_colored_pc_from_mesh.pack_materials): 1 <= M <= 255, shapes, dtypes, and every image inside `texels`.
    ValueError with the cause; returns M.  Reads mat_offset and mat_wh on the host (one synchronisation for device tensors)."""
    if not isinstance(materials, (tuple, list)) or len(materials) != 4 or not all(torch.is_tensor(t) for t in materials):
        raise ValueError("packed materials: expected the four tensors (texels, mat_offset, mat_wh, mat_kd) of pack_materials")
    texels, off, wh, kd = materials
    if texels.dtype != torch.uint8 or texels.dim() != 1:
        raise ValueError(f"packed materials: texels must be uint8 [bytes], got {texels.dtype} {tuple(texels.shape)}")
    M = off.shape[0] if off.dim() == 1 else -1
    if off.dtype != torch.int64 or wh.dtype != torch.int32 or kd.dtype != torch.float32:
        raise ValueError(f"packed materials: mat_offset / mat_wh / mat_kd must be int64 / int32 / float32, got {off.dtype} / {wh.dtype} / {kd.dtype}")
    if M < 0 or tuple(wh.shape) != (M, 2) or tuple(kd.shape) != (M, 3):
        raise ValueError(f"packed materials: mat_offset [M], mat_wh [M,2], mat_kd [M,3] expected, got {tuple(off.shape)} / "
                         f"{tuple(wh.shape)} / {tuple(kd.shape)}")
    if not 1 <= M <= 255:
        raise ValueError(f"packed materials: {M} materials (1 .. 255)")
    total = int(texels.numel())
    for m, (o, (w, h)) in enumerate(zip(off.cpu().tolist(), wh.cpu().tolist())):
        if w == 0 and h == 0:
            continue
        if w <= 0 or h <= 0 or o < 0 or o + 3 * w * h > total:
            raise ValueError(f"packed materials: image of material {m} ({w} x {h} at byte {o}) does not lie inside the {total} texel bytes")
    return M


def shade_views_materials(face_idxs, bary, uvs, face_uvs_idx, face_material, materials, face_normals=None, cam_params=None,
                          light_dirs=None, double_side=False, gamma=None, want_images=True, want_rgba=False, want_material_idx=False):
    """pdhip_shade_views_materials (include/pdhip.h has the contract): face_idxs [V,R,R] i64 / bary [V,R,R,2] as rasterize() returns
    them, uvs [T,2] with face_uvs_idx [F,3] (-1: that corner's UV is (0,0); both may be None), face_material [F] (None: material 0),
    materials: the list load_obj_with_materials returns, or the four tensors of pack_materials (checked on the host once per tuple:
    check_packed_materials) -> (images [V,3,R,R] f32 or None, rgba [V,R,R,4] u8 or None), row 0 at the top, and with
    want_material_idx a third value, the material per pixel [V,R,R] i32 (-1 where uncovered).  Lighting as in shade_views; the number
    of faces F is that of face_material, else of face_uvs_idx, else of face_normals."""
    from . import _lib
    from ._lib import ptr, stream, check
    from .sample_colored_pc_from_mesh import pack_materials, _on as move
    dev = face_idxs.device
    # (a tensor that is already in place costs nothing: one call is tens of microseconds)
    _on = lambda x, dev, dtype: x if (torch.is_tensor(x) and x.device == dev and x.dtype == dtype and x.is_contiguous()) else move(x, dev, dtype)
    if isinstance(materials, tuple):
        _lib.memo(list(materials), 'check_packed_materials', check_packed_materials)
        texels, mat_offset, mat_wh, mat_kd = (_on(t, dev, t.dtype) for t in materials)
    else:
        texels, mat_offset, mat_wh, mat_kd = pack_materials(materials, dev)
    L = _lib.lib()
    V, R = face_idxs.shape[0], face_idxs.shape[1]
    if face_idxs.shape[2] != R:
        raise ValueError(f"shade_views_materials: square views only, got {tuple(face_idxs.shape)}")
    if tuple(bary.shape) != (V, R, R, 2):
        raise ValueError(f"shade_views_materials: bary must be [V,R,R,2] = {(V, R, R, 2)}, got {tuple(bary.shape)}")
    uvs, face_uvs_idx = _on(uvs, dev, torch.float32), _on(face_uvs_idx, dev, torch.int64)
    face_material = _on(face_material, dev, torch.int32)
    if face_uvs_idx is not None and (face_uvs_idx.dim() != 2 or face_uvs_idx.shape[1] != 3):
        raise ValueError(f"shade_views_materials: face_uvs_idx must be [F,3], got {tuple(face_uvs_idx.shape)}")
    if face_material is not None and face_material.dim() != 1:
        raise ValueError(f"shade_views_materials: face_material must be [F], got {tuple(face_material.shape)}")
    if uvs is not None and uvs.numel() and (uvs.dim() != 2 or uvs.shape[1] != 2):
        raise ValueError(f"shade_views_materials: uvs must be [T,2], got {tuple(uvs.shape)}")
    sizes = [t.shape[0] for t in (face_material, face_uvs_idx, face_normals) if t is not None]
    if not sizes or any(n != sizes[0] for n in sizes):
        raise ValueError(f"shade_views_materials: face_material, face_uvs_idx and face_normals must agree on the number of faces (got {sizes})")
    F = sizes[0]
    if uvs is None or face_uvs_idx is None or uvs.numel() == 0:
        if uvs is not None and face_uvs_idx is not None and bool((face_uvs_idx >= 0).any()):
            raise ValueError("shade_views_materials: face_uvs_idx refers to an empty uv table")
        uvs = face_uvs_idx = None
    nl = 0
    if light_dirs is not None:
        light_dirs = torch.as_tensor(light_dirs, dtype=torch.float32, device=dev).reshape(-1, 3).contiguous()
        nl = light_dirs.shape[0]
        if face_normals is None or cam_params is None:
            raise ValueError("shade_views_materials: light_dirs needs face_normals and cam_params")
        face_normals = face_normals.float().contiguous()
        cam_params = cam_params.float().contiguous()
        if tuple(cam_params.shape) != (V, 16):
            raise ValueError(f"shade_views_materials: cam_params must be [V,16], got {tuple(cam_params.shape)}")
    else:
        face_normals = cam_params = None
    images = torch.empty((V, 3, R, R), device=dev) if want_images else None
    rgba = torch.empty((V, R, R, 4), dtype=torch.uint8, device=dev) if want_rgba else None
    midx = torch.empty((V, R, R), dtype=torch.int32, device=dev) if want_material_idx else None
    opt = lambda t, dt=None: ptr(t, dt, allow_none=True) if t is not None and t.numel() else ptr(None, allow_none=True)
    check(L.pdhip_shade_views_materials(
        ptr(face_idxs.contiguous(), torch.int64), ptr(bary.contiguous(), torch.float32), V, R, opt(uvs), 0 if uvs is None else uvs.shape[0],
        opt(face_uvs_idx), opt(face_material), F, opt(texels, torch.uint8), int(texels.numel()), ptr(mat_offset, torch.int64),
        ptr(mat_wh, torch.int32), ptr(mat_kd, torch.float32), mat_offset.shape[0], opt(face_normals), opt(cam_params), opt(light_dirs), nl,
        int(bool(double_side)), float(gamma) if (gamma is not None and nl) else 0.0, opt(images), opt(rgba), opt(midx), stream()),
        'pdhip_shade_views_materials')
    return (images, rgba, midx) if want_material_idx else (images, rgba)


def _save_views(rgba, save_path):
    """albedo_001.png ... as RGBA (camera_utils.py:534-550); the 8-bit images come from the kernel as they are written."""
    import os
    from . import io_utils
    os.makedirs(save_path, exist_ok=True)
    for i in range(rgba.shape[0]):
        arr, wait = io_utils._host_u8(rgba[i])
        io_utils.save_HWC_u8_img(arr, os.path.join(save_path, 'albedo_{:s}.png'.format(str(i + 1).zfill(3))), wait=wait)


def _render(vertices, faces, attr, tri, atlas, cams, res, save_path, save, light_dirs, gamma, double_side, return_mask, pos_hook=None):
    from .extract_texture_map import rasterize
    pos, cp = _clip_positions(cams, vertices)
    if pos_hook is not None:
        pos_hook(pos)
    fidx, bary, _, hard = rasterize(pos, faces, res)
    fn = face_normals_unit(vertices, faces) if light_dirs is not None else None
    images, rgba = shade_views(fidx, bary, attr, tri, atlas=atlas, face_normals=fn, cam_params=cp, light_dirs=light_dirs,
                               double_side=double_side, gamma=gamma, want_images=True, want_rgba=bool(save and save_path))
    if rgba is not None:
        _save_views(rgba, save_path)
    return (images, hard.flip(1)) if return_mask else images


def render_textured_mesh2(vertices, faces, uvs, face_uvs_idx, atlas_img, cams, rescale=False, uv_centers=0, uv_scales=2, padding=0,
                          inpaint_scale_factors=None, glctx=None, save_path=None, save=False, normalize_mesh=False, render_height=None,
                          render_width=None, light_dirs=None, gamma=None, double_side=False, return_mask=False):
    """Render a textured mesh held in tensors (camera_utils.py:251-377): vertices [Vn,3], faces [F,3], uvs [T,2], face_uvs_idx [F,3],
    atlas_img [A,A,3] in the orientation colorize_one_mesh returns (row 0 is v = 0; a loader of a saved model_normalized.png flips
    it back first) -> images [V,3,R,R] with row 0 at the top, uncovered pixels exactly 0 (with return_mask=True also the hard mask
    [V,R,R], flipped alike).  `rescale=True` applies the crop transform of the texturing path (pdhip_rescale_vertices, as
    optimize.texture_coordinates does).  `glctx` is ignored.  The caller's `vertices` are never modified.

    This follows render_textured_mesh (camera_utils.py:379-554), not the body of the reference's render_textured_mesh2, for the v
    flip and the background: that body negates `_texcoords[:, 1]` on a [1,R,R,2] tensor (:338), which negates image row 1 instead of
    the v channel, and it samples the uncovered pixels at uv = 0 instead of leaving them 0 -- both slips of a function the path
    never calls.  Lighting follows :489-529 with the normal turned towards each view's own camera."""
    from . import _lib
    from ._lib import ptr, stream, check
    vertices = vertices.detach().float().contiguous()
    if normalize_mesh:
        vertices = _normalized(vertices).contiguous()
    if atlas_img.dim() == 4:
        atlas_img = atlas_img[0]
    if atlas_img.shape[-1] != 3 and atlas_img.shape[0] == 3:
        atlas_img = atlas_img.permute(1, 2, 0)
    res = int(render_height) if render_height is not None else int(cams[0].height)
    if render_width is not None and int(render_width) != res:
        raise NotImplementedError("render_textured_mesh2: square views only (render_height == render_width)")
    hook = None
    if rescale:
        from .ours_utils import crop_params

        def hook(pos):
            V, dev = pos.shape[0], pos.device
            uvc, uvs_, pad, sf = crop_params(V, dev, uv_centers, uv_scales, padding, inpaint_scale_factors)
            check(_lib.lib().pdhip_rescale_vertices(ptr(pos), V, pos.shape[1], ptr(uvc), ptr(uvs_), ptr(sf), float(pad), stream()),
                  'pdhip_rescale_vertices')
    return _render(vertices, faces, uvs.reshape(-1, 2), face_uvs_idx, atlas_img, cams, res, save_path, save, light_dirs, gamma, double_side,
                   return_mask, hook)


def render_material_mesh(vertices, faces, uvs, face_uvs_idx, face_material, materials, cams, save_path=None, save=False,
                         normalize_mesh=False, light_dirs=None, gamma=None, double_side=False, return_mask=False):
    """The tensor-level renderer of a mesh with per-face materials (camera_utils.py:379-554 after the loading): vertices [Vn,3],
    faces [F,3], uvs [T,2] with face_uvs_idx [F,3] (-1: (0,0); both may be None), face_material [F] (None: material 0), materials
    (the loader's list or the four tensors of pack_materials) -> images [V,3,R,R] with row 0 at the top, uncovered pixels exactly 0
    (with return_mask=True also the hard mask [V,R,R], flipped alike); with save and save_path also albedo_001.png ... as RGBA.
    _render's stages: clip positions, rasterize, face normals when lit, one shading pass (pdhip_shade_views_materials), _save_views.
    The caller's `vertices` are never modified."""
    from .extract_texture_map import rasterize
    from .sample_colored_pc_from_mesh import _on
    if not (torch.is_tensor(vertices) and vertices.is_cuda):
        from . import _lib
        raise _lib.PdhipError("render_material_mesh: expected vertices on the GPU; pointdreamer_amd has no CPU path")
    vertices = vertices.detach().float().contiguous()
    if normalize_mesh:
        vertices = _normalized(vertices).contiguous()
    faces = _on(faces, vertices.device, torch.int64)
    res = int(cams[0].height)
    pos, cp = _clip_positions(cams, vertices)
    fidx, bary, _, hard = rasterize(pos, faces, res)
    fn = face_normals_unit(vertices, faces) if light_dirs is not None else None
    if face_material is None and face_uvs_idx is None:
        face_material = torch.zeros((faces.shape[0],), dtype=torch.int32, device=vertices.device)
    images, rgba = shade_views_materials(fidx, bary, uvs, face_uvs_idx, face_material, materials, face_normals=fn, cam_params=cp,
                                         light_dirs=light_dirs, double_side=double_side, gamma=gamma, want_images=True,
                                         want_rgba=bool(save and save_path))
    if rgba is not None:
        _save_views(rgba, save_path)
    return (images, hard.flip(1)) if return_mask else images


def _load_mtl(path):
    """[(name, dict)] of an MTL file: Kd as three floats, map_Kd as a path relative to the file."""
    mats = []
    with open(path) as f:
        for line in f:
            t = line.split()
            if not t:
                continue
            if t[0] == 'newmtl':
                mats.append((t[1] if len(t) > 1 else '', {}))
            elif mats and t[0] == 'Kd':
                mats[-1][1]['Kd'] = [float(x) for x in t[1:4]]
            elif mats and t[0] == 'map_Kd':
                mats[-1][1]['map_Kd'] = t[-1]
    return mats


def load_textured_obj(mesh_file, device):
    """vertices, faces, uvs, face_uvs_idx and the atlas [A,A,3] f32 (row 0 is v = 0) of an OBJ with ONE material: its `map_Kd` image
    flipped back from the PNG's orientation, or its `Kd` colour as a 1x1 atlas."""
    import os
    import PIL.Image
    from . import io_utils
    v, f, vt, ft = io_utils.load_obj_mesh(mesh_file, with_uv=True)
    mtllib, used = None, []
    with open(mesh_file) as fh:
        for line in fh:
            t = line.split()
            if t and t[0] == 'mtllib':
                mtllib = t[1]
            elif t and t[0] == 'usemtl' and t[1] not in used:
                used.append(t[1])
    mats = _load_mtl(os.path.join(os.path.dirname(mesh_file), mtllib)) if mtllib else []
    if len(mats) > 1 or len(used) > 1:
        raise NotImplementedError(f"{mesh_file}: {max(len(mats), len(used))} materials -- the device renderer takes a mesh with a single "
                                  "material (one map_Kd atlas or one Kd colour); multi-material OBJ files are not supported")
    mat = mats[0][1] if mats else {}
    if 'map_Kd' in mat:
        im = PIL.Image.open(os.path.join(os.path.dirname(mesh_file), mat['map_Kd'])).convert('RGB')
        a = np.asarray(im, np.uint8)
        if a.shape[0] != a.shape[1]:
            raise NotImplementedError(f"{mesh_file}: the atlas is {a.shape[1]} x {a.shape[0]}; square atlases only")
        atlas = torch.from_numpy(np.ascontiguousarray(a[::-1])).to(device).float() / 255.
    else:
        atlas = torch.tensor(mat.get('Kd', [0.5, 0.5, 0.5]), dtype=torch.float32, device=device).reshape(1, 1, 3)
    T = lambda x: torch.from_numpy(x).to(device)
    if vt is None:                                    # no vt records: every corner looks up uv = 0 (camera_utils.py:397, 415-428)
        vt, ft = np.zeros((1, 2), np.float32), np.zeros_like(f)
    return T(v), T(f), T(vt), T(ft), atlas


def _single_atlas_file(mesh_file):
    """True when load_textured_obj takes the file: at most one material (MTL entries and `usemtl` names), whose image, if any, is
    square.  Reads the MTL and the image's header only."""
    import os
    import PIL.Image
    mtllib, used = None, []
    with open(mesh_file) as fh:
        for line in fh:
            t = line.split()
            if t and t[0] == 'mtllib' and len(t) > 1:
                mtllib = t[1]
            elif t and t[0] == 'usemtl' and len(t) > 1 and t[1] not in used:
                used.append(t[1])
    mats = _load_mtl(os.path.join(os.path.dirname(mesh_file), mtllib)) if mtllib else []
    if len(mats) > 1 or len(used) > 1:
        return False
    if mats and 'map_Kd' in mats[0][1]:
        with PIL.Image.open(os.path.join(os.path.dirname(mesh_file), mats[0][1]['map_Kd'])) as im:
            return im.size[0] == im.size[1]
    return True


def render_textured_mesh(mesh_file, cams, device, save_path, glctx=None, save=True, vertices=None, normalize_mesh=True, light_dirs=None,
                         gamma=None, double_side=False, geo_only=False, color=[0.5, 0.5, 0.5]):
    """camera_utils.py:379-554: render an OBJ + MTL (+ images) from every camera -> images [V,3,R,R]; with save=True also
    <save_path>/albedo_001.png ... as RGBA (alpha = coverage).  A file with one material -- its square `map_Kd`, or its `Kd` as a
    1x1 atlas -- goes through load_textured_obj and render_textured_mesh2 (pdhip_shade_views).  Every other file -- several
    `newmtl` / `usemtl`, a non-square `map_Kd` -- goes through sample_colored_pc_from_mesh.load_obj_with_materials and
    render_material_mesh (pdhip_shade_views_materials: the material of the face per pixel, `map_Kd` images of any size next to `Kd`
    colours).  geo_only renders the constant `color` for every material.  `glctx` is ignored; the caller's `vertices` are not modified."""
    if _single_atlas_file(mesh_file):
        v, f, vt, ft, atlas = load_textured_obj(mesh_file, device)
        if vertices is not None:
            assert vertices.shape[0] == v.shape[0]
            v = vertices.to(device)
        if geo_only:
            atlas = torch.tensor(list(color), dtype=torch.float32, device=device).reshape(1, 1, 3)
        return render_textured_mesh2(v, f, vt, ft, atlas, cams, save_path=save_path, save=save, normalize_mesh=normalize_mesh,
                                     light_dirs=light_dirs, gamma=gamma, double_side=double_side)
    from .sample_colored_pc_from_mesh import load_obj_with_materials
    v, f, vt, ft, fm, materials = load_obj_with_materials(mesh_file)
    if vertices is not None:
        assert vertices.shape[0] == v.shape[0]
        v = vertices.to(device)
    else:
        v = torch.from_numpy(v).to(device)
    if geo_only:
        materials = [{'name': m['name'], 'Kd': np.asarray(list(color), np.float32)} for m in materials]
    return render_material_mesh(v, f, vt, ft, fm, materials, cams, save_path=save_path, save=save, normalize_mesh=normalize_mesh,
                                light_dirs=light_dirs, gamma=gamma, double_side=double_side)


def render_textured_mesh_w_mask(mesh_file, cams, device, save_path, glctx=None, save=True, vertices=None, normalize_mesh=True):
    """camera_utils.py:556-676: render_textured_mesh without lighting.  Returns the images [V,3,R,R], as the reference's does
    despite its name (the coverage is the alpha of the saved files)."""
    return render_textured_mesh(mesh_file, cams, device, save_path, glctx=glctx, save=save, vertices=vertices, normalize_mesh=normalize_mesh)


def render_per_vertex_color_mesh(vertices, faces, vertex_colors, cams, save_path=None, light_dirs=None, gamma=None, double_side=False):
    """camera_utils.py:735-828 on tensors (what spr.recon_one_shape_SPR returns): vertices [Vn,3], faces [F,3], vertex_colors [Vn,3]
    in [0,1] -> images [V,3,R,R], row 0 at the top; with save_path also albedo_001.png ... as RGBA."""
    vertices = vertices.detach().float().contiguous()
    return _render(vertices, faces, vertex_colors, faces, None, cams, int(cams[0].height), save_path, save_path is not None, light_dirs,
                   gamma, double_side, False)


def _find_mesh_file(root_path, cls_id, name):
    import os
    for rel in (('models', 'model_normalized.obj'), ('models', f'{name}.obj'), ('meshes', 'model.obj'), ('Scan', 'Scan.obj')):
        p = os.path.join(root_path, 'meshes', cls_id, name, *rel)
        if os.path.exists(p):
            return p
    return os.path.join(root_path, 'meshes', cls_id, name, 'models', 'model_normalized.obj')


def render_textured_meshes_shapenet2(names=None, root_path=None, device=None, save_root_path=None, glctx=None, per_vertex=False):
    """camera_utils.py:680-730: every <root_path>/meshes/<cls_id>/<name>/models/model_normalized.obj (or the reference's three other
    layouts) from the 20 'self_defined' views at 1024^2 into <root_path>/rendered_imgs/<cls_id>/<name>/albedo_%03d.png (RGBA).  Files
    with several materials and `map_Kd` images of any size are rendered (render_textured_mesh routes them to render_material_mesh).
    A shape whose 20 files exist is skipped; a shape that fails is logged and the run goes on.  Returns the number of shapes rendered."""
    import os
    import logging
    import traceback
    from . import io_utils
    device = device if device is not None else torch.device('cuda')
    log = logging.getLogger('pointdreamer_amd.render')
    cams, _, _, _ = create_cameras(num_views=20, distance=1.6, res=1024, device=device, distribution='self_defined')
    out_root = save_root_path if save_root_path is not None else root_path
    done = 0
    for cls_id in sorted(os.listdir(os.path.join(root_path, 'meshes'))):
        if cls_id.endswith(('.log', '.yaml', '.py')) or not os.path.isdir(os.path.join(root_path, 'meshes', cls_id)):
            continue
        shape_names = sorted(os.listdir(os.path.join(root_path, 'meshes', cls_id)))
        for i, name in enumerate(shape_names):
            if names is not None and name not in names:
                continue
            save_path = os.path.join(out_root, 'rendered_imgs', cls_id, name)
            if os.path.isdir(save_path) and len(os.listdir(save_path)) == 20:
                continue
            print(cls_id, i, '/', len(shape_names), name)
            try:
                mesh_file = _find_mesh_file(root_path, cls_id, name)
                if per_vertex:
                    v, f, c = io_utils.load_obj_vertex_colors(mesh_file)
                    T = lambda x: torch.from_numpy(x).to(device)
                    render_per_vertex_color_mesh(T(v), T(f), T(c), cams, save_path=save_path)
                else:
                    render_textured_mesh(mesh_file, cams, device, save_path, save=True)
                io_utils.flush()
                done += 1
            except KeyboardInterrupt:
                raise
            except Exception:                      # noqa: BLE001 -- the reference logs the shape and goes on (:728-730)
                log.error(f'{i},{name}')
                log.error(traceback.format_exc())
    return done
