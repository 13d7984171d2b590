"""Welding of close vertices and cleaning of a supplied mesh on the device (csrc/mesh_clean.hip; include/pdhip.h has the contracts).  The reference
gets this from its loaders: trimesh merges vertices by default, and pymeshlab's first filters are "Merge Close Vertices", "Remove Duplicate Faces" and
"Remove Unreferenced Vertices".  Every later mesh stage here (components, smoothing, decimation, the UV unwrap, 'neighbor' completion) finds
neighbours by vertex INDEX, so a triangle soup, an unwelded marching-cubes export or a mesh with seams must be welded first:

  clean (this module) -> components -> smooth -> decimate -> unwrap -> texture

  weld_vertices(vertices, tolerance=0.0, return_counts=False)                      -> rep [Vn] int32[, counts]
  clean_mesh(vertices, faces, colors=None, tolerance=0.0, return_map=False, return_face_index=False, return_counts=False)
                                                                                   -> (vertices, faces[, colors][, vertex_map][, face_index][, counts])
  mesh_report(vertices, faces)                                                     -> dict

Vertices i and j are close when d2(i, j) <= tolerance^2 (f64, on the f32 coordinates); a class is a connected component of that graph (single
linkage), its representative the smallest index.  Faces are relabelled to representatives; a face with two equal indices is degenerate, two faces with
the same index set are duplicates (the smallest face index stays), both are dropped, as are the vertices nothing names any more.  Surviving faces
and vertices keep their input order; positions and colours are the representative's, bit for bit.  CPU tensors raise PdhipError: there is no CPU
path."""
import math

import torch

from . import _lib, mesh_components, mesh_smooth, mesh_utils
from ._lib import ptr, stream, check, PdhipError

MAX_VERTICES_FACES = 1 << 21               # pdhip_clean_faces: three indices of a face share one 64-bit sort key
MISC_WORDS = 64


_vertices, _faces = mesh_components._vertices, mesh_components._faces


def _tolerance(tolerance):
    if isinstance(tolerance, bool) or not isinstance(tolerance, (int, float)) or not (math.isfinite(tolerance) and tolerance >= 0):
        raise ValueError(f"tolerance={tolerance!r}: the welding distance is a finite number >= 0 (0: exactly equal coordinates)")
    return float(tolerance)


def _sort_arrays(n, dev):
    """keys x2, vals x2, hist for a radix sort of n elements (the lengths include/pdhip.h states)."""
    n = max(int(n), 1)
    keys = torch.empty((2, n), dtype=torch.int64, device=dev)
    vals = torch.empty((2, n), dtype=torch.int32, device=dev)
    hist = torch.empty((512 * ((n + 2047) // 2048),), dtype=torch.int32, device=dev)
    return keys, vals, hist


def _weld(v, tol):
    Vn, dev = v.shape[0], v.device
    L = _lib.lib()
    ca = max(int(L.pdhip_weld_cells_axis(Vn)), 1)                 # (0: the entry refuses Vn)
    keys, vals, hist = _sort_arrays(Vn, dev)
    cstart = torch.empty((ca ** 3 + 1,), dtype=torch.int32, device=dev)
    sorted_xyzi = torch.empty((max(Vn, 1), 4), dtype=torch.float32, device=dev)
    parent = torch.empty((max(Vn, 1),), dtype=torch.int32, device=dev)
    misc = torch.empty((MISC_WORDS,), dtype=torch.int32, device=dev)
    rep = torch.empty((max(Vn, 1),), dtype=torch.int32, device=dev)
    counts = torch.empty((4,), dtype=torch.int32, device=dev)
    check(L.pdhip_weld_vertices(ptr(v) if Vn else ptr(sorted_xyzi), Vn, tol, ptr(rep), ptr(counts), ptr(keys[0]), ptr(keys[1]), ptr(vals[0]),
                                ptr(vals[1]), keys.shape[1], ptr(hist), hist.shape[0], ptr(cstart), cstart.shape[0], ptr(sorted_xyzi),
                                sorted_xyzi.shape[0], ptr(parent), parent.shape[0], ptr(misc), misc.shape[0], stream()), 'pdhip_weld_vertices')
    return rep[:Vn], counts


def weld_vertices(vertices, tolerance=0.0, return_counts=False):
    """vertices [Vn,3] (GPU) -> rep [Vn] int32 on the device: the smallest index of the class of every vertex (module docstring).  return_counts: a
    second result, dict(classes, merged, cells_per_axis, wide_queries).  Quadratic in the number of vertices that share one grid cell.  Synchronises."""
    tol = _tolerance(tolerance)
    v = _vertices(vertices, 'weld_vertices')
    rep, counts = _weld(v, tol)
    if return_counts:
        c = counts.tolist()
        return rep, dict(classes=c[0], merged=c[1], cells_per_axis=c[2], wide_queries=c[3])
    return rep


def _clean_faces(f, rep, Vn):
    F, dev = f.shape[0], f.device
    keys, vals, hist = _sort_arrays(F, dev)
    misc = torch.empty((MISC_WORDS,), dtype=torch.int32, device=dev)
    out = torch.empty_like(f)
    keep = torch.empty((F,), dtype=torch.uint8, device=dev)
    counts = torch.empty((4,), dtype=torch.int32, device=dev)
    check(_lib.lib().pdhip_clean_faces(ptr(f), F, ptr(rep), Vn, ptr(out), ptr(keep), ptr(counts), ptr(keys[0]), ptr(keys[1]), ptr(vals[0]), ptr(vals[1]),
                                       keys.shape[1], ptr(hist), hist.shape[0], ptr(misc), misc.shape[0], stream()), 'pdhip_clean_faces')
    return out, keep, counts


def _clean(v, f, c, tol, what):
    """-> (vertices, faces, colors or None, vertex_map [Vn] i32, face_index [F'] i64, counts dict); ValueError when no face is left."""
    Vn, F = v.shape[0], f.shape[0]
    if F == 0:
        raise ValueError(f"{what}: the mesh has no face; an empty mesh is not returned")
    if Vn > MAX_VERTICES_FACES:                                    # (pdhip_clean_faces' limit, refused here before the welding runs)
        raise PdhipError(f"{what}: {Vn} vertices exceed 2^21 = {MAX_VERTICES_FACES}: the three indices of a face share one 64-bit sort key")
    rep, wc = _weld(v, tol)
    rf, keep, fc = _clean_faces(f, rep.contiguous(), Vn)
    classes, merged = wc.tolist()[:2]
    degenerate, duplicate, kept = fc.tolist()[:3]
    if kept == 0:
        raise ValueError(f"{what}: none of the {F} faces is left ({degenerate} degenerate after welding at tolerance {tol!r}, {duplicate} "
                         "duplicate); an empty mesh is not returned")
    out = mesh_components.compact_mesh(v, rf, keep, colors=c, return_map=True)
    vmap = out[-1]
    vertex_map = vmap[rep.long()].contiguous()
    face_index = torch.nonzero(keep, as_tuple=False).reshape(-1)
    nv = out[0].shape[0]
    counts = dict(vertices_before=Vn, vertices_after=nv, merged=merged, unreferenced=classes - nv, faces_before=F, faces_after=out[1].shape[0],
                  degenerate=degenerate, duplicate=duplicate)
    return out[0], out[1], (out[2] if c is not None else None), vertex_map, face_index, counts


def clean_mesh(vertices, faces, colors=None, tolerance=0.0, return_map=False, return_face_index=False, return_counts=False):
    """vertices [Vn,3], faces [F,3] (GPU; any triangle list: a soup, a mesh with seams, repeated or collapsed faces) -> (vertices, faces[, colors])
    welded at `tolerance` (an absolute distance; 0: exactly equal coordinates) and cleaned: no degenerate face, no duplicate face, no unreferenced
    vertex (module docstring).  return_map: vertex_map [Vn] int32, the output index of every input vertex's representative, -1 when it was dropped.
    return_face_index: face_index [F'] int64, the input face of every output face (to filter per-face data such as an OBJ's `ft` rows).
    return_counts: dict(vertices_before, vertices_after, merged, unreferenced, faces_before, faces_after, degenerate, duplicate).  A mesh with no
    face left: ValueError (never an empty mesh).  At most 2^21 vertices.  Synchronises."""
    what = 'clean_mesh'
    tol = _tolerance(tolerance)
    v, f = _vertices(vertices, what), _faces(faces, what)
    c = None
    if colors is not None:
        c = _vertices(colors, what, 'colors')
        if c.shape != v.shape:
            raise PdhipError(f"{what}: vertices {tuple(v.shape)} and colors {tuple(c.shape)} differ")
    ov, of, oc, vmap, fidx, counts = _clean(v, f, c, tol, what)
    out = (ov, of)
    if c is not None:
        out += (oc,)
    if return_map:
        out += (vmap,)
    if return_face_index:
        out += (fidx,)
    if return_counts:
        out += (counts,)
    return out


def _topology(f, Vn):
    """boundary_edges, nonmanifold_pairs, components of the faces as they are (pdhip_neighbour_csr, pdhip_mesh_boundary_vertices, label_components)."""
    rowptr, colidx = mesh_smooth._csr(Vn, f)
    _, counts = mesh_smooth._boundary(f, Vn, rowptr, colidx)
    _, nb, nm, _ = counts.tolist()
    stats = mesh_components.label_components(f, n_vertices=Vn, return_stats=True)[2]
    return dict(boundary_edges=nb, nonmanifold_pairs=nm, components=stats['count'])


def mesh_report(vertices, faces):
    """What cleaning would do to the mesh, and whether the mesh as it is suits the stages that need a closed 2-manifold (spr_faces-style decimation):
    the counts of clean_mesh at tolerance 0, and boundary_edges (edges on one face), nonmanifold_pairs (edges on more than two), components of the
    faces AS GIVEN -- a closed manifold has 0, 0 and as many components as it has pieces; a soup has 3 F, 0 and F.  Call it on clean_mesh's output to
    see what cleaning achieved.  No kernel of its own.  Synchronises."""
    what = 'mesh_report'
    v, f = _vertices(vertices, what), _faces(faces, what)
    if f.shape[0] == 0:
        raise ValueError(f"{what}: the mesh has no face")
    try:
        counts = _clean(v, f, None, 0.0, what)[5]
    except ValueError:                                            # nothing would be left: the counts of that
        rep, wc = _weld(v, 0.0)
        _, _, fc = _clean_faces(f, rep.contiguous(), v.shape[0])
        classes, merged = wc.tolist()[:2]
        degenerate, duplicate, _ = fc.tolist()[:3]
        counts = dict(vertices_before=v.shape[0], vertices_after=0, merged=merged, unreferenced=classes, faces_before=f.shape[0], faces_after=0,
                      degenerate=degenerate, duplicate=duplicate)
    counts.update(_topology(f, v.shape[0]))
    return counts
