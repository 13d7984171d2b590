"""Coherent orientation of a supplied mesh on the device (csrc/mesh_orient.hip; include/pdhip.h has the contract and the definitions in full).  The
reference gets this from its loaders: trimesh re-orients on load (`fix_normals`) and pymeshlab has "Re-Orient all faces coherently".  A soup welded
back from an STL, a scan exported by a tool that does not care or a ShapeNet model has flipped faces as often as seams, and the later stages rely on
the winding: spr.simplify_mesh asks for a consistently oriented 2-manifold, the unwrap cuts charts by the signed normal axis, the renderers shade by
the face normal.

  clean -> orient (this module) -> components -> smooth -> decimate -> unwrap -> texture

  orient_faces(vertices, faces, open_patches='majority', return_flip=False, return_patches=False, return_counts=False)
                                                                                   -> faces[, flip][, patches][, counts]
  orientation_report(vertices, faces)                                              -> dict

Orientation crosses manifold edges only (edges on exactly two faces); a patch is a connected component of the faces across them, its root its
smallest face index.  Inside a patch the faces are made to agree; a closed patch (no boundary, no non-manifold edge) is then turned outward by the
sign of an exact integer volume on a 12-bit grid of its own box, an open patch keeps the winding of the majority of its faces (a tie: of its root),
or follows the volume rule too with open_patches='volume'.  A non-orientable patch (a Moebius strip) is reported and left alone; degenerate faces
are kept as given.  Each closed patch is turned outward on its own: a nested cavity is NOT turned inward (as trimesh does for multibody meshes).  A
flipped face (a, b, c) becomes (a, c, b).  CPU tensors raise PdhipError: there is no CPU path."""
import torch

from . import _lib, mesh_components
from ._lib import ptr, stream, check

OPEN_PATCHES = ('majority', 'volume')
MISC_WORDS = 64
FLAG_CLOSED, FLAG_NONORIENTABLE, FLAG_BY_VOLUME, FLAG_COMPLEMENTED = 1, 2, 4, 8

_vertices, _faces = mesh_components._vertices, mesh_components._faces


def _open_patches(open_patches):
    if open_patches not in OPEN_PATCHES:
        raise ValueError(f"open_patches={open_patches!r}: open patches are oriented by 'majority' (the fewest flips) or by 'volume' (the closed "
                         "patches' rule)")
    return OPEN_PATCHES.index(open_patches)


def _orient(v, f, mode, what):
    """-> (out_faces, flip u8, face_patch i32, dict of per-patch tensors, counts list) of pdhip_orient_faces."""
    Vn, F, dev = v.shape[0], f.shape[0], f.device
    if F == 0:
        raise ValueError(f"{what}: the mesh has no face")
    if Vn == 0:
        raise ValueError(f"{what}: the mesh has no vertex")
    n = 3 * F
    keys = torch.empty((2, n), dtype=torch.int64, device=dev)
    vals = torch.empty((2, n), dtype=torch.int32, device=dev)
    hist = torch.empty((512 * ((n + 2047) // 2048),), dtype=torch.int32, device=dev)
    face_tmp = torch.empty((5 * F,), dtype=torch.int32, device=dev)
    box = torch.empty((6 * F,), dtype=torch.int32, device=dev)
    tiles = torch.empty((2 * (F // 2048 + 1),), dtype=torch.int32, device=dev)
    misc = torch.empty((MISC_WORDS,), dtype=torch.int32, device=dev)
    out = torch.empty_like(f)
    flip = torch.empty((F,), dtype=torch.uint8, device=dev)
    face_patch = torch.empty((F,), dtype=torch.int32, device=dev)
    p_root, p_faces, p_flipped, p_flags = (torch.empty((F,), dtype=torch.int32, device=dev) for _ in range(4))
    p_vol = torch.empty((F,), dtype=torch.int64, device=dev)
    counts = torch.empty((8,), dtype=torch.int32, device=dev)
    check(_lib.lib().pdhip_orient_faces(ptr(v), Vn, ptr(f), F, mode, ptr(out), ptr(flip), ptr(face_patch), ptr(p_root), ptr(p_faces),
                                        ptr(p_flipped), ptr(p_flags), ptr(p_vol), ptr(counts), ptr(keys[0]), ptr(keys[1]), ptr(vals[0]), ptr(vals[1]),
                                        keys.shape[1], ptr(hist), hist.shape[0], ptr(face_tmp), face_tmp.shape[0], ptr(box), box.shape[0], ptr(tiles),
                                        tiles.shape[0], ptr(misc), misc.shape[0], stream()), 'pdhip_orient_faces')
    c = counts.tolist()
    P = c[0]
    patches = dict(root=p_root[:P], faces=p_faces[:P], flipped=p_flipped[:P], flags=p_flags[:P], vol=p_vol[:P])
    return out, flip, face_patch, patches, c


def _counts(c):
    return dict(patches=c[0], flipped=c[1], nonorientable_patches=c[2], incoherent_edges=c[3], boundary_edges=c[4], nonmanifold_edges=c[5],
                degenerate=c[6])


def orient_faces(vertices, faces, open_patches='majority', return_flip=False, return_patches=False, return_counts=False):
    """vertices [Vn,3], faces [F,3] (GPU; any indexed triangle list) -> faces [F,3] int64 coherently oriented, closed patches outward (module
    docstring); every face stays, in its place.  return_flip: flip [F] uint8, 1 where the face was flipped (to flip per-face rows such as an OBJ's
    `ft` by the same (1, 2) swap).  return_patches: a dict of device tensors -- face_patch [F] int32 (-1: degenerate), and per patch root (smallest
    face index; patches are numbered by ascending root), faces, flipped (int32), flags (int32: 1 closed, 2 non-orientable, 4 decided by volume,
    8 complemented), vol (int64).  return_counts: dict(patches, flipped, nonorientable_patches, incoherent_edges (manifold edges whose two faces
    disagreed as given), boundary_edges, nonmanifold_edges, degenerate).  A function of the mesh alone; two calls give equal bytes.  Synchronises."""
    what = 'orient_faces'
    mode = _open_patches(open_patches)
    v, f = _vertices(vertices, what), _faces(faces, what)
    out, flip, face_patch, patches, c = _orient(v, f, mode, what)
    res = (out,)
    if return_flip:
        res += (flip,)
    if return_patches:
        res += (dict(patches, face_patch=face_patch),)
    if return_counts:
        res += (_counts(c),)
    return res if len(res) > 1 else out


def orientation_report(vertices, faces):
    """What orient_faces would do to the mesh as it is with the default open_patches='majority' (would_flip on OPEN patches differs from what
    open_patches='volume' does; closed patches are the same under both): dict(patches, would_flip, nonorientable_patches, incoherent_edges, boundary_edges,
    nonmanifold_edges, closed_patches).  A closed, consistently oriented, outward 2-manifold has would_flip = incoherent_edges = boundary_edges =
    nonmanifold_edges = 0 and as many closed patches as pieces.  Synchronises."""
    what = 'orientation_report'
    v, f = _vertices(vertices, what), _faces(faces, what)
    _, _, _, patches, c = _orient(v, f, 0, what)
    closed = int((patches['flags'] & FLAG_CLOSED).ne(0).sum())
    return dict(patches=c[0], would_flip=c[1], nonorientable_patches=c[2], incoherent_edges=c[3], boundary_edges=c[4], nonmanifold_edges=c[5],
                closed_patches=closed)
