"""Helpers of the connected-component tests (tests/test_mesh_components_cpu.py, tests/test_gpu_mesh_components.py): a SEQUENTIAL union-find
that implements the definition of include/pdhip.h (two vertices are connected when a face names both; root = smallest index; ids by ascending
root; -1 for a vertex no face names; counts; boxes), the selection rules of mesh_components.filter_components with their tie rule, the compaction,
and the mesh builders of the cases.  Nothing here calls libpdhip."""
import functools

import numpy as np

from mesh_simplify_common import grid_torus


# ---- the oracle
def oracle_components(faces, n_vertices, vertices=None):
    """dict(vertex_comp [Vn] i32, face_comp [F] i32, root, n_vertices, n_faces [C] i32, count[, box [C,6] f32])."""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    Vn = int(n_vertices)
    assert f.size == 0 or (f.min() >= 0 and f.max() < Vn)
    parent = list(range(Vn))

    def find(x):
        r = x
        while parent[r] != r:
            r = parent[r]
        while parent[x] != r:
            parent[x], x = r, parent[x]
        return r

    for a, b, c in f.tolist():
        for p, q in ((a, b), (b, c)):
            rp, rq = find(p), find(q)
            if rp != rq:
                parent[max(rp, rq)] = min(rp, rq)               # the smaller index stays the root
    root = np.array([find(v) for v in range(Vn)], np.int64)
    ref = np.zeros(Vn, bool)
    ref[f.reshape(-1)] = True
    roots = np.unique(root[ref])                                # ascending
    cid = -np.ones(Vn, np.int64)
    cid[roots] = np.arange(len(roots))
    vcomp = np.where(ref, cid[root], -1).astype(np.int32)
    fcomp = vcomp[f[:, 0]].astype(np.int32) if len(f) else np.zeros(0, np.int32)
    C = len(roots)
    out = dict(vertex_comp=vcomp, face_comp=fcomp, root=roots.astype(np.int32), n_vertices=np.bincount(vcomp[ref], minlength=C).astype(np.int32),
               n_faces=np.bincount(fcomp, minlength=C).astype(np.int32), count=C)
    if vertices is not None:
        v = np.asarray(vertices, np.float32)
        box = np.empty((C, 6), np.float32)
        for c in range(C):
            m = v[vcomp == c]
            box[c, :3], box[c, 3:] = m.min(0), m.max(0)
        out['box'] = box
    return out


def oracle_select(o, keep=None, min_faces=None, min_face_share=None, min_diameter_share=None):
    """[C] bool: the components that pass every rule given (the rules and the tie rule of mesh_components.select_components)."""
    assert not (keep is None and min_faces is None and min_face_share is None and min_diameter_share is None)
    nf = o['n_faces'].astype(np.int64)
    ok = np.ones(o['count'], bool)
    top = int(nf.max())
    if keep == 'largest':
        ok &= np.arange(o['count']) == int(np.flatnonzero(nf == top)[0])            # the smaller root on a tie (ids ascend with the roots)
    if min_faces is not None:
        ok &= nf >= int(min_faces)
    if min_face_share is not None:
        ok &= nf.astype(np.float64) >= float(min_face_share) * float(top)
    if min_diameter_share is not None:
        box = o['box'].astype(np.float64)
        e = box[:, 3:] - box[:, :3]
        d2 = e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1] + e[:, 2] * e[:, 2]
        a = box[:, 3:].max(0) - box[:, :3].min(0)
        all2 = a[0] * a[0] + a[1] * a[1] + a[2] * a[2]
        ok &= d2 >= (float(min_diameter_share) * float(min_diameter_share)) * all2
    return ok


def oracle_compact(vertices, faces, face_keep, colors=None):
    """The kept faces and the vertices they name, both in input order: (vertices, faces[, colors], vertex_map)."""
    v, f, k = np.asarray(vertices, np.float32), np.asarray(faces, np.int64), np.asarray(face_keep, bool)
    used = np.zeros(len(v), bool)
    used[f[k].reshape(-1)] = True
    new = -np.ones(len(v), np.int64)
    new[used] = np.arange(int(used.sum()))
    out = (v[used], new[f[k]])
    if colors is not None:
        out += (np.asarray(colors, np.float32)[used],)
    return out + (new.astype(np.int32),)


def oracle_filter(vertices, faces, colors=None, **rules):
    """(vertices, faces[, colors], vertex_map, dict(components, components_kept)) of the sequential definition."""
    o = oracle_components(faces, len(vertices), vertices)
    ok = oracle_select(o, **rules)
    assert ok.any()
    return oracle_compact(vertices, faces, ok[o['face_comp']], colors) + (dict(components=o['count'], components_kept=int(ok.sum())),)


def relabel(faces, perm):
    """The same mesh with vertex v renamed perm[v] (vertex arrays go through scatter: new[perm] = old)."""
    return np.asarray(perm, np.int64)[np.asarray(faces, np.int64)]


def same_partition(a, b, perm):
    """vertex_comp a of a mesh and b of its relabelling (b[perm[v]] belongs to a[v]) split the vertices the same way."""
    a, b = np.asarray(a), np.asarray(b)[np.asarray(perm)]
    if not np.array_equal(a < 0, b < 0):
        return False
    pairs = np.unique(np.stack([a, b], 1), axis=0)
    return len(np.unique(pairs[:, 0])) == len(pairs) == len(np.unique(pairs[:, 1]))


# ---- the meshes
TET = np.array([[0, 1, 2], [0, 3, 1], [1, 3, 2], [2, 3, 0]], np.int64)
TET_V = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], np.float32)


def two_tetrahedra():
    """Case 1: two tetrahedra with no shared vertex and one unreferenced vertex in the middle of the index range (Vn = 9, F = 8)."""
    f = np.concatenate([TET, TET + 5])
    v = np.concatenate([TET_V * 0.25 - 0.5, [[9.0, 9.0, 9.0]], TET_V * 0.5 + 0.125]).astype(np.float32)
    return v, f


def bow_tie():
    """Case 2a: two tetrahedra sharing exactly vertex 3 (Vn = 7, F = 8): one component."""
    second = np.array([3, 4, 5, 6])[TET]
    v = np.concatenate([TET_V - 1.0, TET_V[1:] + 1.0]).astype(np.float32)
    v[3] = 0.0
    return v, np.concatenate([TET, second])


def joined_triangles():
    """Case 2b: two triangles with no common vertex and the face (2, 2, 3) between them: a repeated index still connects."""
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [3, 0, 0], [4, 0, 0], [3, 1, 0]], np.float32)
    return v, np.array([[0, 1, 2], [3, 4, 5], [2, 2, 3]], np.int64)


def strip(n_faces=4000, order='ascending', seed=0):
    """Case 3: a triangle strip, face k = (k, k + 1, k + 2) along the strip -- vertex indices ascending, descending (every union re-roots) or randomly
    permuted with the faces shuffled.  -> (vertices, faces, perm) with perm[v] the index of strip vertex v."""
    n = n_faces + 2
    k = np.arange(n_faces)
    f = np.stack([k, k + 1 + (k & 1), k + 2 - (k & 1)], 1)                             # alternating, so that the strip is oriented
    base = np.stack([(np.arange(n) // 2) * 0.001, (np.arange(n) % 2) * 0.001, np.zeros(n)], 1).astype(np.float32)
    rng = np.random.default_rng(seed)
    perm = {'ascending': np.arange(n), 'descending': np.arange(n)[::-1].copy(), 'random': rng.permutation(n)}[order]
    f = relabel(f, perm)
    if order == 'random':
        f = f[rng.permutation(n_faces)]
    v = np.empty_like(base)
    v[perm] = base
    return v, np.ascontiguousarray(f), perm


def separate_triangles(n=5000):
    """Case 4: n triangles with no shared vertex (Vn = 3 n)."""
    f = np.arange(3 * n, dtype=np.int64).reshape(n, 3)
    k = np.arange(3 * n)
    v = np.stack([(k // 3) * 0.01 + (k % 3 == 1) * 0.004, (k % 3 == 2) * 0.004, np.zeros(3 * n)], 1).astype(np.float32)
    return v, f


@functools.lru_cache(maxsize=None)
def _three_tori(nu, nv, seed):
    tv, tf = grid_torus(nu, nv)
    n = len(tv)
    v = np.concatenate([tv + np.float32(s) for s in (-1.0, 0.0, 1.0)]).astype(np.float32)
    f = np.stack([tf + k * n for k in range(3)], 1).reshape(-1, 3)                     # round-robin: faces 0 1 2 of tori 0 1 2, ...
    perm = np.random.default_rng(seed).permutation(3 * n)
    pv = np.empty_like(v)
    pv[perm] = v
    return pv, relabel(f, perm), perm


def three_tori(nu=24, nv=12, seed=3):
    """Case 5: three grid_torus(nu, nv) translated apart, faces interleaved round-robin, vertex indices randomly permuted -> (vertices, faces,
    perm) with perm[k n + i] the index of vertex i of torus k."""
    v, f, p = _three_tori(nu, nv, seed)
    return v.copy(), f.copy(), p.copy()


def shuffled_and_rotated(faces, seed=0):
    """The same faces in another order, each with its indices rotated by 0, 1 or 2 places."""
    f = np.asarray(faces, np.int64)
    rng = np.random.default_rng(seed)
    f = f[rng.permutation(len(f))]
    r = rng.integers(0, 3, len(f))
    return np.ascontiguousarray(np.stack([f[np.arange(len(f)), (r + k) % 3] for k in range(3)], 1))


def icosphere(level, radius=0.5, center=(0.0, 0.0, 0.0)):
    """The icosahedron subdivided `level` times (20 * 4^level faces: level 0 is the icosahedron itself), vertices on the sphere."""
    from pointdreamer_amd import synthetic
    v, f = synthetic.icosphere(2 ** level, radius=radius)
    return (v + np.asarray(center, np.float32)).astype(np.float32), f


@functools.lru_cache(maxsize=None)
def _blobs():
    parts = [icosphere(3)]
    rng = np.random.default_rng(11)
    d = rng.standard_normal((12, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    parts += [icosphere(0, 0.02, 0.7 * d[k]) for k in range(12)]
    parts += [icosphere(2, 0.1, (0.0, 0.8, 0.0))]
    # the big sphere is NOT first in the index range: six blobs, the sphere, the middle one, six blobs
    order = [1, 2, 3, 4, 5, 6, 0, 13, 7, 8, 9, 10, 11, 12]
    vs, fs, off = [], [], 0
    for k in order:
        v, f = parts[k]
        vs.append(v)
        fs.append(f + off)
        off += len(v)
    v, f = np.concatenate(vs).astype(np.float32), np.concatenate(fs)
    f = f[np.random.default_rng(12).permutation(len(f))]                               # the components' faces interleaved
    col = np.random.default_rng(13).random((len(v), 3), dtype=np.float32)
    return v, np.ascontiguousarray(f), col


def blobs():
    """Case 6: icosphere(3) (1 280 faces), twelve icosphere(0) blobs of radius 0.02 (20 faces each) and one icosphere(2) of radius 0.1 (320 faces),
    disjoint, with colours -> (vertices, faces, colors)."""
    v, f, c = _blobs()
    return v.copy(), f.copy(), c.copy()


FILTER_SETTINGS = (dict(keep='largest'), dict(min_faces=100), dict(min_face_share=0.05), dict(min_diameter_share=0.1),
                   dict(min_faces=100, min_diameter_share=0.5))
FILTER_KEPT = (1, 2, 2, 2, 1)                                                          # components each setting keeps of the 14


def twin_tetrahedra(swapped=False):
    """Case 7: two identical tetrahedra, four faces each; swapped: their index ranges exchanged (the second one's vertices come first)."""
    v = np.concatenate([TET_V, TET_V + 2.0]).astype(np.float32)
    f = np.concatenate([TET, TET + 4])
    if swapped:
        perm = np.array([4, 5, 6, 7, 0, 1, 2, 3])
        nv = np.empty_like(v)
        nv[perm] = v
        v, f = nv, relabel(f, perm)
    return v, f
