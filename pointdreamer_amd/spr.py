"""Geometry from the cloud alone (`geo_from: 'SPR'`): the reference's baselines/spr.py:recon_one_shape_SPR asks pymeshlab (CPU) for
normals for a point set, screened Poisson reconstruction and quadric decimation.  Here the first two run on the device
(csrc/surface_recon.hip): oriented normals from k nearest neighbours + visibility votes, a Poisson solve on a dense grid of
2^depth cells per axis, marching cubes with welded vertices.  The mesh is this project's own (not pymeshlab's): a closed,
consistently oriented triangle mesh, every component of the iso-surface included (`keep_components=` drops the small floating ones on the
device: mesh_components.py).  The third, decimation to a face count, is this
build's own as well (csrc/simplify_mesh.hip, `simplify_mesh` / `target_faces=`): quadric-error edge collapses in rounds of independent
collapses on the device, topology preserved; pymeshlab's decimator is not reproduced."""
import numpy as np
import torch

from . import _lib
from ._lib import ptr, rows, stream, check, PdhipError

DEPTHS = (6, 7, 8)
DEFAULT_DEPTH = 6                    # 7-36 k faces, the size the stages downstream were tuned at (DESIGN, surface reconstruction)
DEFAULT_KNN = 16
EYE_RADIUS = 1.6                     # the cameras' distance (demo.py:337), in units of the cloud's largest extent


def _points(points, what):
    return rows(points, what, '[N,3]', 3, torch.float32)


def estimate_normals(points, k=DEFAULT_KNN, n_eyes=32, return_counts=False, eye_radius=EYE_RADIUS):
    """points [N,3] (GPU) -> unit normals [N,3] f32 pointing out of the solid.  return_counts: also a dict with the number of points
    oriented by the eyes that see them (`eyes`), by the majority of their oriented neighbours (`neighbours`), by their nearest oriented
    neighbour (`nearest`) and left as computed (`unoriented`); they add up to N (synchronises)."""
    p = _points(points, 'estimate_normals')
    L = _lib.lib()
    N = p.shape[0]
    nbytes = L.pdhip_estimate_normals_ws_bytes(N, int(k), int(n_eyes))
    ws = torch.empty((max(1, nbytes),), dtype=torch.uint8, device=p.device)
    normals = torch.empty((N, 3), dtype=torch.float32, device=p.device)
    counts = torch.zeros((4,), dtype=torch.int32, device=p.device)
    check(L.pdhip_estimate_normals(ptr(p), N, int(k), int(n_eyes), float(eye_radius), ptr(normals), ptr(counts), ptr(ws), stream()),
          'pdhip_estimate_normals')
    if return_counts:
        c = counts.cpu().tolist()
        return normals, dict(eyes=c[0], neighbours=c[1], nearest=c[2], unoriented=c[3])
    return normals


def capacities(depth):
    """Default (vertex, face) capacities of poisson_reconstruct: a surface of 6 (2^depth)^2 cells' area -- four times a sphere that
    fills the grid's inner 3/4.  A mesh that needs more is reconstructed again with the sizes the first call reported."""
    g2 = (1 << int(depth)) ** 2
    return 8 * g2, 16 * g2


def poisson_reconstruct(points, normals, depth=DEFAULT_DEPTH, return_counts=False, colors=None, capacity=None):
    """points, normals [N,3] (GPU; normals point outwards) -> (vertices f32 [Vn,3], faces int64 [F,3]).  colors [N,3]: a third result,
    the colour of the nearest cloud point per vertex.  return_counts: a last result, dict(vertices, faces, iterations, h, origin,
    iso, residual, splat_radius).  capacity: (vertices, faces) to allocate instead of capacities(depth); too small is a PdhipError
    that names the sizes needed."""
    if int(depth) not in DEPTHS:
        raise ValueError(f"depth={depth}: the dense grid supports depth 6, 7 or 8 (2^depth cells per axis); the reference's default 12 "
                         "is an octree depth")
    p = _points(points, 'poisson_reconstruct')
    n = _points(normals, 'poisson_reconstruct')
    if n.shape != p.shape:
        raise PdhipError(f"poisson_reconstruct: points {tuple(p.shape)} and normals {tuple(n.shape)} differ")
    c = None
    if colors is not None:
        c = _points(colors, 'poisson_reconstruct')
        if c.shape != p.shape:
            raise PdhipError(f"poisson_reconstruct: points {tuple(p.shape)} and colors {tuple(c.shape)} differ")
    N, dev = p.shape[0], p.device
    L = _lib.lib()
    ws = torch.empty((max(1, L.pdhip_surface_recon_ws_bytes(N, int(depth))),), dtype=torch.uint8, device=dev)
    counts = torch.zeros((4,), dtype=torch.int32, device=dev)
    info = torch.zeros((8,), dtype=torch.float32, device=dev)
    vcap, fcap = capacity if capacity is not None else capacities(depth)
    for attempt in (0, 1):
        verts = torch.empty((int(vcap), 3), dtype=torch.float32, device=dev)
        faces = torch.empty((int(fcap), 3), dtype=torch.int64, device=dev)
        vcol = torch.empty((int(vcap), 3), dtype=torch.float32, device=dev) if c is not None else None
        rc = L.pdhip_surface_recon(ptr(p), ptr(n), ptr(c, allow_none=True), N, int(depth), ptr(verts), int(vcap), ptr(faces), int(fcap),
                                   ptr(vcol, allow_none=True), ptr(counts), ptr(info), ptr(ws), stream())
        nv, nf, iters, _ = counts.cpu().tolist()
        if rc != 0 and attempt == 0 and capacity is None and (nv > vcap or nf > fcap):
            vcap, fcap = max(nv, vcap), max(nf, fcap)       # the call reported the sizes: once more, exactly
            continue
        check(rc, 'pdhip_surface_recon')
        break
    out = [verts[:nv].contiguous(), faces[:nf].contiguous()]
    if c is not None:
        out.append(vcol[:nv].contiguous())
    if return_counts:
        i = info.cpu().tolist()
        out.append(dict(vertices=nv, faces=nf, iterations=iters, h=i[0], origin=tuple(i[1:4]), iso=i[4], residual=i[5], splat_radius=i[6],
                        nodes=int(i[7])))
    return tuple(out)


def simplify_mesh(vertices, faces, target_faces, colors=None, return_counts=False):
    """vertices [Vn,3], faces [F,3] (GPU; a closed, consistently oriented 2-manifold, any number of components) -> (vertices f32,
    faces int64) with target_faces (+ 1 for an odd target) faces, the topology preserved.  colors [Vn,3]: a third result, per vertex the
    colour of the collapsed endpoint nearer to it.  return_counts: a last result, dict(vertices, faces, rounds, stalled); stalled = no
    further collapse keeps the topology and the shape, the mesh has more faces than asked for.  target_faces >= F returns the input."""
    v = _points(vertices, 'simplify_mesh')
    f = rows(faces, 'simplify_mesh', 'faces [F,3]', 3, torch.int64)
    c = None
    if colors is not None:
        c = _points(colors, 'simplify_mesh')
        if c.shape != v.shape:
            raise PdhipError(f"simplify_mesh: vertices {tuple(v.shape)} and colors {tuple(c.shape)} differ")
    Vn, F, dev = v.shape[0], f.shape[0], v.device
    L = _lib.lib()
    nbytes = L.pdhip_simplify_mesh_workspace_bytes(Vn, F)
    if nbytes == 0:
        raise PdhipError(f"simplify_mesh: Vn={Vn} F={F}: a closed mesh has at least 4 vertices and 4 faces, and at most 2^22 / 2^23")
    ws = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
    ov, of = torch.empty_like(v), torch.empty_like(f)
    oc = torch.empty_like(c) if c is not None else None
    counts = torch.zeros((4,), dtype=torch.int32, device=dev)
    check(L.pdhip_simplify_mesh(ptr(v), Vn, ptr(f), F, ptr(c, allow_none=True), int(target_faces), ptr(ov), ptr(of), ptr(oc, allow_none=True),
                                ptr(counts), ptr(ws), stream()), 'pdhip_simplify_mesh')
    nv, nf, rounds, flags = counts.cpu().tolist()
    out = [ov[:nv].contiguous(), of[:nf].contiguous()]
    if c is not None:
        out.append(oc[:nv].contiguous())
    if return_counts:
        out.append(dict(vertices=nv, faces=nf, rounds=rounds, stalled=bool(flags & 1)))
    return tuple(out)


def _to_device(a, name):
    if torch.is_tensor(a):
        if not a.is_cuda:
            raise PdhipError(f"recon_one_shape_SPR: {name} is a CPU tensor; pass a GPU tensor or a numpy array (there is no CPU path)")
        return a
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, np.float32))).to(torch.device('cuda', torch.cuda.current_device()))


def recon_one_shape_SPR(coords, colors, gt_normals=None, save_path=None, depth=DEFAULT_DEPTH, simplify_face_num=None, *, knn=DEFAULT_KNN,
                        return_counts=False, target_faces=None, keep_components=None, smooth=None):
    """baselines/spr.py:16-75 with its argument order and 3-tuple (vertices [Vn,3], faces [F,3], vertex_colors [Vn,3]), as GPU
    tensors.  coords / colors / gt_normals: GPU tensors or numpy arrays (numpy goes to the current device).  gt_normals None: the
    normals are estimated.  save_path: the mesh is written as an OBJ.  depth: 6, 7 or 8 (a dense grid of 2^depth cells per axis, not
    the reference's octree depth 12).  simplify_face_num: pymeshlab's decimation is not reproduced -- anything but None is refused.
    target_faces: this build's own decimator (simplify_mesh) after the reconstruction, before save_path is written; with return_counts
    the dict gains faces_reconstructed and simplify_rounds.  keep_components: 'largest' or a dict of mesh_components.filter_components' rules
    (keep, min_faces, min_face_share, min_diameter_share): the floating pieces of the iso-surface that fail them are dropped after the
    reconstruction and BEFORE the decimation, so target_faces budgets only the kept geometry; the vertex colours are carried through and with
    return_counts the dict gains components and components_kept (and faces_reconstructed).  None: nothing new is called.  smooth: an int (Taubin steps
    with MeshLab's lambda 0.5 and mu -0.53) or a dict of steps, lam, mu (mesh_smooth.taubin_smooth, boundary vertices held): the vertices are smoothed
    AFTER keep_components and BEFORE target_faces, so the decimator's quadrics see the smoothed surface; faces and vertex colours stay as they are, and
    with return_counts the dict gains smooth_steps and smooth_moved.  None: nothing new is called."""
    if simplify_face_num is not None:
        raise NotImplementedError("recon_one_shape_SPR: pymeshlab's quadric edge-collapse decimation (simplify_face_num) is not reproduced; "
                                  "this build's own decimator is the keyword target_faces=")
    if int(depth) not in DEPTHS:
        raise ValueError(f"depth={depth}: the dense grid supports depth 6, 7 or 8 (2^depth cells per axis); the reference's default 12 "
                         "is an octree depth")
    if keep_components is not None:
        rules = dict(keep='largest') if keep_components == 'largest' else keep_components
        if not isinstance(rules, dict) or not rules or any(k not in ('keep', 'min_faces', 'min_face_share', 'min_diameter_share') for k in rules):
            raise ValueError(f"keep_components={keep_components!r}: 'largest' or a dict of filter_components' rules (keep, min_faces, "
                             "min_face_share, min_diameter_share)")
    if smooth is not None:
        from . import mesh_smooth
        sm = dict(steps=smooth) if isinstance(smooth, int) and not isinstance(smooth, bool) else smooth
        if not isinstance(sm, dict) or 'steps' not in sm or any(k not in ('steps', 'lam', 'mu') for k in sm):
            raise ValueError(f"smooth={smooth!r}: a number of Taubin steps or a dict of steps, lam, mu")
        try:
            sm = dict(zip(('steps', 'lam', 'mu'), mesh_smooth.check_params(sm['steps'], sm.get('lam', mesh_smooth.DEFAULT_LAMBDA),
                                                                         sm.get('mu', mesh_smooth.DEFAULT_MU))))
        except ValueError as e:
            raise ValueError(f"smooth={smooth!r}: {e}") from None
    xyz = _to_device(coords, 'coords')
    rgb = _to_device(colors, 'colors')
    counts = None
    if gt_normals is None:
        normals, counts = estimate_normals(xyz, k=knn, return_counts=True)
    else:
        normals = _to_device(gt_normals, 'gt_normals')
    verts, faces, vcol, rc = poisson_reconstruct(xyz, normals, depth=depth, colors=rgb, return_counts=True)
    if keep_components is not None:
        from . import mesh_components
        verts, faces, vcol, cc = mesh_components.filter_components(verts, faces, colors=vcol, return_counts=True, **rules)
        rc = dict(rc, faces_reconstructed=rc['faces'], vertices=cc['vertices_after'], faces=cc['faces_after'], components=cc['components'],
                  components_kept=cc['components_kept'], faces_dropped=cc['faces_before'] - cc['faces_after'])
    if smooth is not None:
        verts, mc = mesh_smooth.taubin_smooth(verts, faces, return_counts=True, **sm)
        rc = dict(rc, smooth_steps=mc['steps'], smooth_moved=mc['moved'])
    if target_faces is not None:
        verts, faces, vcol, sc = simplify_mesh(verts, faces, target_faces, colors=vcol, return_counts=True)
        rc = dict(rc, faces_reconstructed=rc.get('faces_reconstructed', rc['faces']), vertices=sc['vertices'], faces=sc['faces'],
                  simplify_rounds=sc['rounds'])
    if save_path is not None:
        from . import io_utils
        io_utils.save_obj_mesh(verts.cpu().numpy(), faces.cpu().numpy(), save_path)
    if return_counts:
        return verts, faces, vcol, dict(orientation=counts, **rc)
    return verts, faces, vcol
