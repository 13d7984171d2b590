"""Helpers of the mesh-cleaning tests (tests/test_mesh_clean_cpu.py, tests/test_gpu_mesh_clean.py): the definitions of include/pdhip.h in numpy --
an all-pairs f64 d2 matrix with the exact expression (dx dx + dy dy) + dz dz, a SEQUENTIAL union-find toward the smaller index, Python's sorted
triples for the faces, mesh_components_common's compaction -- and the meshes of the cases.  Nothing here calls libpdhip."""
import numpy as np

from mesh_components_common import oracle_compact, icosphere, shuffled_and_rotated, TET, TET_V  # noqa: F401  (re-exported to the tests)

ALL_PAIRS_MAX = 8000                        # vertices an all-pairs matrix is built for (in row blocks)


def close_pairs(vertices, tol):
    """[P,2] i64, i < j: the pairs with d2(i, j) <= tol * tol, d2 = (dx dx + dy dy) + dz dz on the f32 coordinates widened to f64, op by op."""
    x = np.asarray(vertices, np.float32).astype(np.float64)
    n = len(x)
    assert n <= ALL_PAIRS_MAX
    tol2 = np.float64(tol) * np.float64(tol)
    out = []
    for b in range(0, n, 1024):
        q = x[b:b + 1024]
        dx, dy, dz = (q[:, None, k] - x[None, :, k] for k in range(3))
        d2 = (dx * dx + dy * dy) + dz * dz
        i, j = np.nonzero(d2 <= tol2)
        i += b
        m = i < j
        out.append(np.stack([i[m], j[m]], 1))
    return np.concatenate(out).astype(np.int64)


def union_find(n, pairs):
    """rep [n] i32 of a sequential union-find over the pairs, the smaller index staying the root."""
    parent = list(range(n))

    def find(x):
        r = x
        while parent[r] != r:
            r = parent[r]
        while parent[x] != r:
            parent[x], x = r, parent[x]
        return r

    for a, b in np.asarray(pairs).tolist():
        ra, rb = find(a), find(b)
        if ra != rb:
            parent[max(ra, rb)] = min(ra, rb)
    return np.array([find(v) for v in range(n)], np.int32)


def rep_of_labels(labels):
    """rep [n] i32: the smallest index of every label's class."""
    labels = np.asarray(labels)
    first = np.full(int(labels.max()) + 1, len(labels), np.int64)
    np.minimum.at(first, labels, np.arange(len(labels)))
    return first[labels].astype(np.int32)


def oracle_weld(vertices, tol, max_pairs=400000):
    """rep [Vn] i32 of the definition.  Up to max_pairs close pairs by the sequential union-find; beyond (a crowd: millions of pairs of one class)
    by scipy's connected components of the SAME exact close-pair graph, which test_mesh_clean_cpu shows to agree with the union-find."""
    p = close_pairs(vertices, tol)
    n = len(vertices)
    if len(p) <= max_pairs:
        return union_find(n, p)
    return rep_of_labels(graph_labels(n, p))


def graph_labels(n, pairs):
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    g = coo_matrix((np.ones(len(pairs), np.int8), (pairs[:, 0], pairs[:, 1])), shape=(n, n))
    return connected_components(g, directed=False)[1]


def oracle_weld_exact(vertices):
    """rep at tol = 0 through np.unique(axis=0) (any Vn).  -0.0 is brought to +0.0 first: the definition calls them equal."""
    v = np.asarray(vertices, np.float32) + np.float32(0.0)
    _, inv = np.unique(v, axis=0, return_inverse=True)
    return rep_of_labels(inv.reshape(-1))


def oracle_clean_faces(faces, rep):
    """(relabelled faces [F,3] i64, keep [F] bool, dict(degenerate, duplicate, kept))."""
    f = np.asarray(rep, np.int64)[np.asarray(faces, np.int64)]
    keep = np.zeros(len(f), bool)
    seen, deg, dup = set(), 0, 0
    for k, (a, b, c) in enumerate(f.tolist()):
        if a == b or b == c or a == c:
            deg += 1
            continue
        key = tuple(sorted((a, b, c)))
        if key in seen:
            dup += 1
            continue
        seen.add(key)
        keep[k] = True
    return f, keep, dict(degenerate=deg, duplicate=dup, kept=int(keep.sum()))


def oracle_clean(vertices, faces, colors=None, tol=0.0, rep=None):
    """dict(rep, vertices, faces[, colors], vertex_map, face_index, counts) of the definition."""
    v = np.asarray(vertices, np.float32)
    rep = oracle_weld(v, tol) if rep is None else rep
    rf, keep, fc = oracle_clean_faces(faces, rep)
    out = oracle_compact(v, rf, keep, colors)
    ov, of, vmap = out[0], out[1], out[-1]
    classes = int((rep == np.arange(len(v))).sum())
    res = dict(rep=rep, vertices=ov, faces=of, vertex_map=vmap[rep].astype(np.int32), face_index=np.flatnonzero(keep).astype(np.int64),
               counts=dict(vertices_before=len(v), vertices_after=len(ov), merged=len(v) - classes, unreferenced=classes - len(ov),
                           faces_before=len(rf), faces_after=len(of), degenerate=fc['degenerate'], duplicate=fc['duplicate']))
    if colors is not None:
        res['colors'] = out[2]
    return res


# ---- the meshes
def soup(vertices, faces):
    """Three private vertices per face, as an STL round trip leaves them."""
    f = np.asarray(faces, np.int64)
    return np.ascontiguousarray(np.asarray(vertices, np.float32)[f.reshape(-1)]), np.arange(3 * len(f), dtype=np.int64).reshape(-1, 3)


def two_tetrahedra_soup(negative_zero=False):
    """Case 1: two disjoint tetrahedra as a soup (24 vertices, 8 faces).  negative_zero: every second copy of a zero coordinate is -0.0."""
    v = np.concatenate([TET_V - 0.0, TET_V + 2.0]).astype(np.float32)
    sv, sf = soup(v, np.concatenate([TET, TET + 4]))
    if negative_zero:
        z = np.flatnonzero(sv.reshape(-1) == 0.0)
        sv.reshape(-1)[z[::2]] = np.float32(-0.0)
        assert np.signbit(sv).any() and not np.signbit(sv).all()
    return sv, sf


def permuted(vertices, faces, seed, colors=None):
    """The same mesh with its vertex indices randomly permuted (new[perm] = old)."""
    perm = np.random.default_rng(seed).permutation(len(vertices))
    v = np.empty_like(vertices)
    v[perm] = vertices
    out = (v, perm[np.asarray(faces, np.int64)])
    if colors is not None:
        c = np.empty_like(colors)
        c[perm] = colors
        out += (c,)
    return out


def chain(n, spacing, seed, direction=(1.0, 2.0, 3.0)):
    """Case 5: n collinear points `spacing` apart along `direction`, at random indices."""
    d = np.asarray(direction, np.float64)
    d /= np.linalg.norm(d)
    p = (np.arange(n, dtype=np.float64)[:, None] * spacing * d[None, :]).astype(np.float32)
    v = np.empty_like(p)
    v[np.random.default_rng(seed).permutation(n)] = p
    return v


def crowd(copies=5000, cloud=2000, seed=7):
    """Case 7: `copies` copies of one point and a jittered cloud of `cloud` points (pairs of near-duplicates), shuffled."""
    rng = np.random.default_rng(seed)
    base = rng.random((cloud // 2, 3), dtype=np.float32)
    twin = (base + rng.uniform(-2e-4, 2e-4, base.shape)).astype(np.float32)
    v = np.concatenate([np.tile(np.array([[0.25, 0.5, 0.75]], np.float32), (copies, 1)), base, twin])
    return np.ascontiguousarray(v[rng.permutation(len(v))])


def jittered_copies(vertices, faces, copies, radius, seed):
    """Case 8: every vertex `copies` times, each copy moved by at most `radius` (per axis radius / sqrt 3); face corners pick a copy at random."""
    rng = np.random.default_rng(seed)
    n = len(vertices)
    j = rng.uniform(-1.0, 1.0, (copies, n, 3)) * (radius / np.sqrt(3.0))
    v = (np.asarray(vertices, np.float64)[None] + j).astype(np.float32).reshape(-1, 3)
    f = np.asarray(faces, np.int64) + n * rng.integers(0, copies, np.asarray(faces).shape)
    return v, f


def seam_sphere(n_lat=24, n_lon=48):
    """An indexed UV sphere written with a duplicated seam column (as an export with UV seams leaves it): the faces of the last longitude strip
    name private copies of the vertices on the meridian of longitude 0, so the strip's far edge is open on both sides."""
    from pointdreamer_amd import synthetic
    v, f, _ = synthetic.uv_sphere(n_lat, n_lon)
    f = f.copy()
    ring = lambda i: (i >= 1) & (i <= len(v) - 2)                                  # not a pole
    col = lambda i: (i - 1) % n_lon
    last = ((ring(f) & (col(f) == n_lon - 1)).any(1))[:, None] & ring(f) & (col(f) == 0)      # column-0 corners of the faces of the last strip
    seam = 1 + n_lon * np.arange(n_lat - 1)                                        # the vertices of column 0, one per ring
    copy = -np.ones(len(v), np.int64)
    copy[seam] = len(v) + np.arange(len(seam))
    f[last] = copy[f[last]]
    return np.concatenate([v, v[seam]]).astype(np.float32), f
