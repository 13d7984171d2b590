"""Connected components of a mesh and the removal of its small floating pieces on the device (csrc/mesh_components.hip; include/pdhip.h has the
contracts).  The reference has no counterpart: it reconstructs by POCO.  The dense-grid Poisson solve of spr.py turns every clump of stray points
into a blob of its own; MeshLab users run "Remove isolated pieces" after every screened Poisson reconstruction, and this is that filter.

  label_components(faces, n_vertices=None, vertices=None, return_stats=False)  -> (vertex_comp [Vn] int32, face_comp [F] int32[, stats])
  filter_components(vertices, faces, colors=None, keep=None, min_faces=None, min_face_share=None, min_diameter_share=None, return_counts=False)
                                                                                -> (vertices, faces[, colors][, counts])

Two vertices are connected when a face names both; a component's root is its smallest vertex index and the components are numbered by ascending
root, so labels are a function of the mesh alone (not of the order of its faces, nor of the threads').  CPU tensors raise PdhipError: there is no
CPU path."""
import torch

from . import _lib
from ._lib import ptr, ptr_or_null, rows, stream, check, PdhipError

DEFAULT_CAPACITY = 4096                # components the first call has room for; a mesh with more is labelled once more with exactly C
RULES = ('keep', 'min_faces', 'min_face_share', 'min_diameter_share')


def _faces(faces, what):
    return rows(faces, what, 'faces [F,3]', 3, torch.int64)


def _vertices(x, what, name='vertices'):
    return rows(x, what, f'{name} [Vn,3]', 3, torch.float32)


def label_components(faces, n_vertices=None, vertices=None, return_stats=False):
    """faces [F,3] (GPU, any indexed triangle list) -> (vertex_comp [Vn] int32: the component of every vertex, -1 where no face names it;
    face_comp [F] int32).  n_vertices: Vn (default: len(vertices), or the largest index + 1).  return_stats: a third result, a dict of device
    tensors per component -- root (smallest vertex index), vertices, faces (counts), box ([C,6] float32, min xyz then max xyz; only when
    `vertices` is given) -- and the ints count, referenced, unreferenced.  Synchronises."""
    f = _faces(faces, 'label_components')
    v = _vertices(vertices, 'label_components') if vertices is not None else None
    F, dev = f.shape[0], f.device
    if n_vertices is None:
        n_vertices = v.shape[0] if v is not None else (int(f.max()) + 1 if F else 1)
    Vn = int(n_vertices)
    if v is not None and v.shape[0] != Vn:
        raise PdhipError(f"label_components: vertices {tuple(v.shape)} and n_vertices={Vn} differ")
    L = _lib.lib()
    ws = torch.empty((max(int(L.pdhip_mesh_components_workspace_bytes(Vn, F)), 8),), dtype=torch.uint8, device=dev)   # (0: the entry refuses the sizes)
    vcomp = torch.empty((max(Vn, 0),), dtype=torch.int32, device=dev)
    fcomp = torch.empty((F,), dtype=torch.int32, device=dev)
    counts = torch.empty((4,), dtype=torch.int32, device=dev)
    cap = DEFAULT_CAPACITY
    one = None if F else torch.zeros((8,), dtype=torch.int64, device=dev)      # (a non-null pointer for the arrays of an empty face list)
    while True:
        root, nv, nf = (torch.empty((cap,), dtype=torch.int32, device=dev) for _ in range(3))
        box = torch.empty((cap, 6), dtype=torch.float32, device=dev) if v is not None else None
        check(L.pdhip_mesh_components(ptr(f) if F else ptr(one), F, ptr_or_null(v), Vn, ptr_or_null(vcomp), ptr(fcomp) if F else ptr(one), ptr(root), ptr(nv), ptr(nf),
                                      ptr(box, allow_none=True), cap, ptr(counts), ptr(ws), stream()), 'pdhip_mesh_components')
        C, referenced, unreferenced, _ = counts.tolist()
        if C <= cap:
            break
        cap = C                                                   # the call reported C: once more, exactly
    if not return_stats:
        return vcomp, fcomp
    stats = dict(root=root[:C], vertices=nv[:C], faces=nf[:C], count=C, referenced=referenced, unreferenced=unreferenced)
    if box is not None:
        stats['box'] = box[:C]
    return vcomp, fcomp, stats


def compact_mesh(vertices, faces, face_keep, colors=None, return_map=False):
    """The faces with face_keep[f] set ([F] bool / uint8 on the GPU) and the vertices they name, both in input order, re-indexed: (vertices f32,
    faces int64[, colors]); vertices and colours are copied bit for bit and every output vertex is referenced.  return_map: a last result,
    [Vn] int32, the new index of every input vertex or -1.  Synchronises."""
    v, f = _vertices(vertices, 'compact_mesh'), _faces(faces, 'compact_mesh')
    c = None
    if colors is not None:
        c = _vertices(colors, 'compact_mesh', 'colors')
        if c.shape != v.shape:
            raise PdhipError(f"compact_mesh: vertices {tuple(v.shape)} and colors {tuple(c.shape)} differ")
    if not (torch.is_tensor(face_keep) and face_keep.is_cuda):
        raise PdhipError("compact_mesh needs tensors on the GPU (cuda:N == HIP device); there is no CPU path")
    k = _lib.as_u8(face_keep.detach()).to(torch.uint8).contiguous()
    Vn, F, dev = v.shape[0], f.shape[0], v.device
    if k.shape != (F,):
        raise PdhipError(f"compact_mesh: face_keep {tuple(k.shape)} for {F} faces")
    L = _lib.lib()
    ws = torch.empty((max(int(L.pdhip_compact_mesh_workspace_bytes(Vn, F)), 8),), dtype=torch.uint8, device=dev)
    ov, of = torch.empty_like(v), torch.empty_like(f)
    oc = torch.empty_like(c) if c is not None else None
    vmap = torch.empty((Vn,), dtype=torch.int32, device=dev) if return_map else None
    counts = torch.empty((4,), dtype=torch.int32, device=dev)
    one = None if F else torch.zeros((8,), dtype=torch.int64, device=dev)      # (a non-null pointer for the arrays of an empty face list)
    check(L.pdhip_compact_mesh(ptr_or_null(v), Vn, ptr(f) if F else ptr(one), F, ptr(c, allow_none=True), ptr(k) if F else ptr(one), ptr_or_null(ov),
                               ptr(of) if F else ptr(one), ptr(oc, allow_none=True), ptr(vmap, allow_none=True), ptr(counts), ptr(ws), stream()),
          'pdhip_compact_mesh')
    nv, nf = counts.tolist()[:2]
    out = [ov[:nv].contiguous(), of[:nf].contiguous()]
    if c is not None:
        out.append(oc[:nv].contiguous())
    if return_map:
        out.append(vmap)
    return tuple(out)


def select_components(stats, keep=None, min_faces=None, min_face_share=None, min_diameter_share=None):
    """[C] bool on the device: the components of label_components' stats that pass EVERY rule given.  keep='largest': the one with the most faces,
    the smaller root on a tie.  min_faces: at least that many faces.  min_face_share: at least that share of the largest component's face count.
    min_diameter_share: the diagonal of its box at least that share of the diagonal of the box of all referenced vertices (MeshLab's "wrt
    diameter"; both widened to f64, their squares compared)."""
    if keep is None and min_faces is None and min_face_share is None and min_diameter_share is None:
        raise ValueError(f"filter_components: no rule given (one or more of {RULES})")
    if keep not in (None, 'largest'):
        raise ValueError(f"keep={keep!r}: 'largest' (the component with the most faces) or None")
    if min_faces is not None and (isinstance(min_faces, bool) or not isinstance(min_faces, int) or min_faces < 0):
        raise ValueError(f"min_faces={min_faces!r}: a face count is an integer >= 0")
    for name, s in (('min_face_share', min_face_share), ('min_diameter_share', min_diameter_share)):
        if s is not None and (isinstance(s, bool) or not isinstance(s, (int, float)) or not 0.0 <= s <= 1.0):
            raise ValueError(f"{name}={s!r}: a share is a number in [0, 1]")
    if min_diameter_share is not None and 'box' not in stats:
        raise ValueError("min_diameter_share needs the components' boxes (label_components(..., vertices=...))")
    nf = stats['faces']
    ok = torch.ones_like(nf, dtype=torch.bool)
    if stats['count'] == 0:
        return ok
    top = nf.max()
    if keep == 'largest':
        ids = torch.arange(nf.shape[0], device=nf.device)
        ok &= ids == torch.where(nf == top, ids, nf.shape[0]).min()      # (ids ascend with the roots: the first is the smaller root)
    if min_faces is not None:
        ok &= nf >= int(min_faces)
    if min_face_share is not None:
        ok &= nf.double() >= float(min_face_share) * top.double()
    if min_diameter_share is not None:
        box = stats['box'].double()
        e = box[:, 3:] - box[:, :3]
        d2 = e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1] + e[:, 2] * e[:, 2]
        a = box[:, 3:].max(0)[0] - box[:, :3].min(0)[0]
        all2 = a[0] * a[0] + a[1] * a[1] + a[2] * a[2]
        ok &= d2 >= (float(min_diameter_share) * float(min_diameter_share)) * all2
    return ok


def filter_components(vertices, faces, colors=None, keep=None, min_faces=None, min_face_share=None, min_diameter_share=None, return_counts=False):
    """vertices [Vn,3], faces [F,3] (GPU) -> (vertices, faces[, colors]) of the components that pass every rule given (select_components), faces and
    surviving vertices in input order, vertices and colours bit for bit.  No rule given, or no component left: ValueError (never an empty mesh).
    return_counts: a last result, dict(components, components_kept, faces_before, faces_after, vertices_before, vertices_after)."""
    if keep is None and min_faces is None and min_face_share is None and min_diameter_share is None:
        raise ValueError(f"filter_components: no rule given (one or more of {RULES})")
    v, f = _vertices(vertices, 'filter_components'), _faces(faces, 'filter_components')
    if colors is not None and not (torch.is_tensor(colors) and colors.is_cuda):
        raise PdhipError("filter_components needs tensors on the GPU (cuda:N == HIP device); there is no CPU path")
    _, fcomp, stats = label_components(f, n_vertices=v.shape[0], vertices=v if min_diameter_share is not None else None, return_stats=True)
    ok = select_components(stats, keep=keep, min_faces=min_faces, min_face_share=min_face_share, min_diameter_share=min_diameter_share)
    out = compact_mesh(v, f, ok[fcomp.long()], colors=colors) if stats['count'] else (v[:0], f[:0])
    if out[1].shape[0] == 0:                                      # (every component has a face: no face left = no component left)
        raise ValueError(f"filter_components: none of the {stats['count']} components passes the rules (keep={keep!r}, min_faces={min_faces!r}, "
                         f"min_face_share={min_face_share!r}, min_diameter_share={min_diameter_share!r}); an empty mesh is not returned")
    if return_counts:
        out += (dict(components=stats['count'], components_kept=int(ok.sum()), faces_before=f.shape[0], faces_after=out[1].shape[0],
                     vertices_before=v.shape[0], vertices_after=out[0].shape[0]),)
    return out
