"""Mesh helpers of the `complete_unseen_by='neighbor'` path.  Each of the three public functions has two forms with
equal results: given CUDA tensors (float32 / int64) it runs the HIP entries of csrc/neighbor_mesh.hip and returns CUDA tensors; given
numpy or host input it runs the numpy code below, the pinned host form.

`subdivide_with_uv` keeps the name, argument order and return tuple of /root/reference/utils/mesh_utils.py:7-114
(numpy on the host there as well; the reference builds it on trimesh's `grouping.unique_rows` / `faces_to_edges`).
The numbering contract that downstream code depends on: new vertices (UVs) are appended after the old ones, one per unique
undirected edge of the selected faces, ordered by (larger endpoint, smaller endpoint); untouched faces come first, then
four children per selected face in the order (v0 m01 m20) (m01 v1 m12) (m20 m12 v2) (m01 m12 m20).
"""
import ctypes as C

import numpy as np


def _on_device(*xs):
    """True when every argument is a CUDA tensor (the device form is asked for); a mix of device and host input is an error."""
    import torch
    dev = [torch.is_tensor(x) and x.is_cuda for x in xs]
    if any(dev) and not all(dev):
        from ._lib import PdhipError
        raise PdhipError("mesh_utils: all mesh arguments must be on the GPU, or all on the host")
    return all(dev)


def _typed(t, dtype):
    if t.dtype != dtype:
        from ._lib import PdhipError
        raise PdhipError(f"mesh_utils: the device form takes float32 coordinates and int64 indices, got {t.dtype}")
    return t.detach().contiguous()


def _f32(t):
    import torch
    return _typed(t, torch.float32)


def _i64(t):
    import torch
    return _typed(t, torch.int64)


def _subdivide_device(vertices, faces, face_uv_idx, uvs, face_index):
    import torch
    from . import _lib
    from ._lib import ptr, stream, check
    L = _lib.lib()
    v, f, fu, u = _f32(vertices), _i64(faces), _i64(face_uv_idx), _f32(uvs)
    dev = v.device
    V, F, U = v.shape[0], f.shape[0], u.shape[0]
    if face_index is None:
        fi, K = None, -1
    else:
        fi = face_index if torch.is_tensor(face_index) else torch.from_numpy(np.ascontiguousarray(np.asarray(face_index).reshape(-1)))
        fi = fi.to(dev).to(torch.int64).reshape(-1).contiguous()
        K = fi.shape[0]
    Tm = F if K < 0 else min(K, F)
    nv = torch.empty((V + 3 * Tm, 3), dtype=torch.float32, device=dev)
    nu = torch.empty((U + 3 * Tm, 2), dtype=torch.float32, device=dev)
    nf = torch.empty((F + 3 * Tm, 3), dtype=torch.int64, device=dev)
    nfu = torch.empty((F + 3 * Tm, 3), dtype=torch.int64, device=dev)
    counts = torch.empty((4,), dtype=torch.int32, device=dev)
    host = (C.c_int32 * 4)()
    ws = torch.empty((max(1, L.pdhip_subdivide_with_uv_ws_bytes(V, U, F, K)),), dtype=torch.uint8, device=dev)
    check(L.pdhip_subdivide_with_uv(ptr(v), V, ptr(f), F, ptr(u), U, ptr(fu), ptr(fi) if K > 0 else None, K, ptr(nv),
                                    ptr(nf), ptr(nu), ptr(nfu), ptr(counts), host, ptr(ws), stream()), 'pdhip_subdivide_with_uv')
    return nv[:host[0]], nf[:host[2]], nu[:host[1]], nfu[:host[2]]


def _vertex_uv_table_device(num_vertices, faces, face_uv_idx, uvs):
    import torch
    from . import _lib
    from ._lib import ptr, stream, check
    L = _lib.lib()
    f, fu, u = _i64(faces), _i64(face_uv_idx), _f32(uvs)
    dev, V, F, U = f.device, int(num_vertices), f.shape[0], u.shape[0]
    out = torch.empty((V, 2), dtype=torch.float32, device=dev)
    counts = torch.empty((1,), dtype=torch.int32, device=dev)
    ws = torch.empty((max(1, L.pdhip_vertex_uv_table_ws_bytes(V, F)),), dtype=torch.uint8, device=dev)
    check(L.pdhip_vertex_uv_table(V, ptr(f), ptr(fu), F, ptr(u), U, ptr(out), ptr(counts), ptr(ws), stream()), 'pdhip_vertex_uv_table')
    return out


def _neighbour_csr_device(num_vertices, faces):
    import torch
    from . import _lib
    from ._lib import ptr, stream, check
    L = _lib.lib()
    f = _i64(faces)
    dev, V, F = f.device, int(num_vertices), f.shape[0]
    rowptr = torch.empty((V + 1,), dtype=torch.int32, device=dev)
    colidx = torch.empty((6 * F,), dtype=torch.int32, device=dev)
    counts = torch.empty((1,), dtype=torch.int32, device=dev)
    host = (C.c_int32 * 1)()
    ws = torch.empty((max(1, L.pdhip_neighbour_csr_ws_bytes(V, F)),), dtype=torch.uint8, device=dev)
    check(L.pdhip_neighbour_csr(V, ptr(f), F, ptr(rowptr), ptr(colidx), ptr(counts), host, ptr(ws), stream()), 'pdhip_neighbour_csr')
    return rowptr, colidx[:host[0]]


def zero_count_vertices(count):
    """Ascending int32 list of the vertices with count[v] == 0 (unproject.py:145-147), on the device: count [V] f32 CUDA tensor."""
    import torch
    from . import _lib
    from ._lib import ptr, stream, check
    L = _lib.lib()
    c = _f32(count)
    V, dev = c.shape[0], c.device
    out = torch.empty((V,), dtype=torch.int32, device=dev)
    counts = torch.empty((1,), dtype=torch.int32, device=dev)
    host = (C.c_int32 * 1)()
    ws = torch.empty((max(1, L.pdhip_compact_zero_count_ws_bytes(V)),), dtype=torch.uint8, device=dev)
    check(L.pdhip_compact_zero_count(ptr(c), V, ptr(out), ptr(counts), host, ptr(ws), stream()), 'pdhip_compact_zero_count')
    return out[:host[0]]


def _edge_midpoints(tri, n_existing):
    """Per-corner midpoint ids (m01, m12, m20) for triangles `tri` [T,3] and the endpoint pairs of the new points."""
    a = tri[:, [0, 1, 2]].reshape(-1)
    b = tri[:, [1, 2, 0]].reshape(-1)
    lo, hi = np.minimum(a, b).astype(np.int64), np.maximum(a, b).astype(np.int64)
    key = lo | (hi << 32)                                   # sort key: larger endpoint major, smaller endpoint minor
    uniq, first, inv = np.unique(key, return_index=True, return_inverse=True)
    ends = np.stack([lo[first], hi[first]], 1)
    return inv.reshape(-1, 3) + n_existing, ends


def _children(tri, mid):
    v0, v1, v2 = tri[:, 0], tri[:, 1], tri[:, 2]
    m01, m12, m20 = mid[:, 0], mid[:, 1], mid[:, 2]
    kids = np.stack([np.stack([v0, m01, m20], 1), np.stack([m01, v1, m12], 1), np.stack([m20, m12, v2], 1),
                     np.stack([m01, m12, m20], 1)], 1)      # [T,4,3]
    return kids.reshape(-1, 3)


def subdivide_with_uv(vertices, faces, face_uv_idx, uvs, face_index=None):
    """Midpoint-subdivide the faces in `face_index` (all faces if None); their neighbours are left untouched, so the result
    is not watertight -- exactly what the reference does.  Returns (new_vertices, new_faces, new_uvs, new_face_uv_idx)."""
    if _on_device(vertices, faces, face_uv_idx, uvs):
        return _subdivide_device(vertices, faces, face_uv_idx, uvs, face_index)
    vertices, faces, face_uv_idx, uvs = (np.asarray(x) for x in (vertices, faces, face_uv_idx, uvs))
    pick = np.zeros(len(faces), bool)
    if face_index is None:
        pick[:] = True
    else:
        pick[np.asarray(face_index)] = True
    tri, tri_uv = faces[pick], face_uv_idx[pick]
    mid, ends = _edge_midpoints(tri, len(vertices))
    mid_uv, ends_uv = _edge_midpoints(tri_uv, len(uvs))
    new_vertices = np.concatenate([vertices, vertices[ends].mean(axis=1)], 0)
    new_uvs = np.concatenate([uvs, uvs[ends_uv].mean(axis=1)], 0)
    new_faces = np.concatenate([faces[~pick], _children(tri, mid)], 0)
    new_face_uv_idx = np.concatenate([face_uv_idx[~pick], _children(tri_uv, mid_uv)], 0)
    return new_vertices, new_faces, new_uvs, new_face_uv_idx


def vertex_uv_table(num_vertices, faces, face_uv_idx, uvs):
    """One UV per vertex (unproject.py:123-127): of the UVs a vertex is used with, the one with the largest index."""
    if _on_device(faces, face_uv_idx, uvs):
        return _vertex_uv_table_device(num_vertices, faces, face_uv_idx, uvs)
    v = np.asarray(faces).reshape(-1).astype(np.int64)
    t = np.asarray(face_uv_idx).reshape(-1).astype(np.int64)
    best = np.full(num_vertices, -1, np.int64)
    np.maximum.at(best, v, t)
    out = np.zeros((num_vertices, 2), np.float32)
    used = best >= 0
    out[used] = np.asarray(uvs, np.float32)[best[used]]
    return out


def neighbour_csr(num_vertices, faces):
    """Unique undirected vertex neighbours as CSR (int32 rowptr[V+1], colidx ascending per row)."""
    if _on_device(faces):
        return _neighbour_csr_device(num_vertices, faces)
    f = np.asarray(faces).astype(np.int64)
    a = np.concatenate([f[:, 0], f[:, 1], f[:, 2], f[:, 1], f[:, 2], f[:, 0]])
    b = np.concatenate([f[:, 1], f[:, 2], f[:, 0], f[:, 0], f[:, 1], f[:, 2]])
    keep = a != b
    key = np.unique(a[keep] * num_vertices + b[keep])
    rows, cols = key // num_vertices, key % num_vertices
    rowptr = np.zeros(num_vertices + 1, np.int64)
    np.add.at(rowptr, rows + 1, 1)
    return np.cumsum(rowptr).astype(np.int32), cols.astype(np.int32)
