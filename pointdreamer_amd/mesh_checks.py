"""Host-side (numpy) checks of a triangle mesh, used by the tests and the tools of the surface reconstruction: closedness and
orientation from the faces alone, signed volume, components and Euler characteristics, point-to-mesh distances.  Checkers only:
nothing on the texturing path calls them."""
import numpy as np


def directed_edge_defects(faces):
    """Number of directed edges that do not occur exactly once with their reverse occurring exactly once.  0 = closed, consistently
    oriented 2-manifold (edge-wise)."""
    f = np.asarray(faces, np.int64)
    a = np.concatenate([f[:, 0], f[:, 1], f[:, 2]])
    b = np.concatenate([f[:, 1], f[:, 2], f[:, 0]])
    n = int(max(a.max(), b.max())) + 1 if len(a) else 1
    key, rev = a * n + b, b * n + a
    uk, cnt = np.unique(key, return_counts=True)
    bad = int((cnt != 1).sum())
    pos = np.searchsorted(uk, rev)
    pos = np.minimum(pos, len(uk) - 1)
    has_rev = uk[pos] == rev
    bad += int((~has_rev).sum())
    bad += int((a == b).sum())
    return bad


def signed_volume(vertices, faces):
    v = np.asarray(vertices, np.float64)
    f = np.asarray(faces, np.int64)
    return float(np.einsum('ij,ij->i', v[f[:, 0]], np.cross(v[f[:, 1]], v[f[:, 2]])).sum() / 6.0)


def face_areas(vertices, faces):
    v = np.asarray(vertices, np.float64)
    f = np.asarray(faces, np.int64)
    return 0.5 * np.linalg.norm(np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]]), axis=1)


def components_euler(n_vertices, faces):
    """[(vertices, edges, faces, euler characteristic)] per connected component, largest first."""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    f = np.asarray(faces, np.int64)
    a = np.concatenate([f[:, 0], f[:, 1], f[:, 2]])
    b = np.concatenate([f[:, 1], f[:, 2], f[:, 0]])
    g = coo_matrix((np.ones(len(a), np.int8), (a, b)), shape=(n_vertices, n_vertices))
    nc, lab = connected_components(g, directed=False)
    e = np.unique(np.minimum(a, b) * n_vertices + np.maximum(a, b))
    ev = lab[e // n_vertices]
    out = []
    for c in range(nc):
        nv, ne, nf = int((lab == c).sum()), int((ev == c).sum()), int((lab[f[:, 0]] == c).sum())
        out.append((nv, ne, nf, nv - ne + nf))
    return sorted(out, key=lambda t: -t[2])


def _point_triangle(p, a, b, c):
    """Distance from points p [n,3] to triangles (a, b, c) [n,3] each (Ericson, Real-Time Collision Detection 5.1.5)."""
    ab, ac, ap = b - a, c - a, p - a
    d1, d2 = (ab * ap).sum(1), (ac * ap).sum(1)
    bp = p - b
    d3, d4 = (ab * bp).sum(1), (ac * bp).sum(1)
    cp = p - c
    d5, d6 = (ab * cp).sum(1), (ac * cp).sum(1)
    vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
    den = va + vb + vc
    den = np.where(den == 0, 1.0, den)
    v, w = vb / den, vc / den
    q = a + ab * v[:, None] + ac * w[:, None]                                    # interior
    def put(mask, val):
        q[mask] = val[mask]
    t = (d4 - d3) / np.where((d4 - d3) + (d5 - d6) == 0, 1.0, (d4 - d3) + (d5 - d6))
    put((va <= 0) & (d4 - d3 >= 0) & (d5 - d6 >= 0), b + (c - b) * t[:, None])
    t = d2 / np.where(d2 - d6 == 0, 1.0, d2 - d6)
    put((vb <= 0) & (d2 >= 0) & (d6 <= 0), a + ac * t[:, None])
    t = d1 / np.where(d1 - d3 == 0, 1.0, d1 - d3)
    put((vc <= 0) & (d1 >= 0) & (d3 <= 0), a + ab * t[:, None])
    put((d6 >= 0) & (d5 <= d6), c)
    put((d3 >= 0) & (d4 <= d3), b)
    put((d1 <= 0) & (d2 <= 0), a)
    return np.linalg.norm(p - q, axis=1)


def point_mesh_distance(points, vertices, faces, candidates=12):
    """Distance from each point to the mesh: the nearest of the `candidates` faces whose centroids are closest (cKDTree)."""
    from scipy.spatial import cKDTree
    p = np.asarray(points, np.float64)
    v = np.asarray(vertices, np.float64)
    f = np.asarray(faces, np.int64)
    cen = v[f].mean(1)
    k = min(candidates, len(f))
    _, idx = cKDTree(cen).query(p, k=k)
    idx = idx.reshape(len(p), k)
    best = np.full(len(p), np.inf)
    for j in range(k):
        t = f[idx[:, j]]
        best = np.minimum(best, _point_triangle(p, v[t[:, 0]], v[t[:, 1]], v[t[:, 2]]))
    return best
