"""Helpers of the orientation tests (tests/test_mesh_orient_cpu.py, tests/test_gpu_mesh_orient.py, tests/test_gpu_parity_union.py): the definitions
of include/pdhip.h (pdhip_orient_faces) in numpy and plain Python -- half-edges by a stable argsort, patches and rel[] by a SEQUENTIAL traversal
from each root in ascending order, the box, the 12-bit grid and the integer volume op by op in f64 / int64 -- a sequential union-find with parity
for pdhip_debug_parity_union, and the meshes of the cases.  Nothing here calls libpdhip."""
import numpy as np

from mesh_components_common import icosphere, TET, TET_V  # noqa: F401  (re-exported to the tests)

CLOSED, NONORIENTABLE, BY_VOLUME, COMPLEMENTED = 1, 2, 4, 8
GRID_MAX = 4095


def half_edges(faces, n_vertices):
    """The half-edge table of the non-degenerate faces, sorted by key (stable): dict(face, d, key [3 L]; deg [F] bool)."""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    deg = (f[:, 0] == f[:, 1]) | (f[:, 1] == f[:, 2]) | (f[:, 0] == f[:, 2])
    live = np.flatnonzero(~deg)
    a, b = f[live].reshape(-1), f[live][:, [1, 2, 0]].reshape(-1)
    key = np.minimum(a, b) * np.int64(n_vertices) + np.maximum(a, b)
    o = np.argsort(key, kind='stable')
    return dict(face=np.repeat(live, 3)[o], d=(a > b)[o], key=key[o], deg=deg)


def oracle_orient(vertices, faces, open_patches='majority'):
    """dict(faces [F,3] i64, flip [F] u8, face_patch [F] i32, root / n_faces / flipped / flags [P] i32, vol [P] i64, counts [8] list) of the
    definition."""
    assert open_patches in ('majority', 'volume')
    v = np.asarray(vertices, np.float32)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    F, Vn = len(f), len(v)
    assert F >= 1 and f.min() >= 0 and f.max() < Vn and np.isfinite(v[np.unique(f)]).all()
    h = half_edges(f, Vn)
    deg = h['deg']
    _, start, cnt = np.unique(h['key'], return_index=True, return_counts=True)
    run = np.repeat(cnt, cnt)                                       # the length of the run every half-edge lies in
    open_face = np.zeros(F, bool)
    open_face[h['face'][run != 2]] = True
    m = start[cnt == 2]
    fa, fb, e = h['face'][m], h['face'][m + 1], (h['d'][m] == h['d'][m + 1]).astype(np.int64)
    # adjacency lists across manifold edges
    src, dst, par = np.concatenate([fa, fb]), np.concatenate([fb, fa]), np.concatenate([e, e])
    o = np.argsort(src, kind='stable')
    ptr = np.searchsorted(src[o], np.arange(F + 1)).tolist()
    nbr, npar = dst[o].tolist(), par[o].tolist()
    patch, rel, roots = [-1] * F, [0] * F, []
    for r in range(F):                                              # ascending: the first face of a patch met is its smallest index
        if deg[r] or patch[r] >= 0:
            continue
        pid = len(roots)
        roots.append(r)
        patch[r] = pid
        stack = [r]
        while stack:
            x = stack.pop()
            for j in range(ptr[x], ptr[x + 1]):
                y = nbr[j]
                if patch[y] < 0:
                    patch[y], rel[y] = pid, rel[x] ^ npar[j]
                    stack.append(y)
    patch, rel, P = np.array(patch, np.int64), np.array(rel, np.int64), len(roots)
    if P == 0:                                                      # every face is degenerate
        z = np.zeros(0, np.int32)
        return dict(faces=f.copy(), flip=np.zeros(F, np.uint8), face_patch=patch.astype(np.int32), root=z, n_faces=z, flipped=z, flags=z,
                    vol=np.zeros(0, np.int64), counts=[0, 0, 0, 0, 0, 0, int(deg.sum()), 0])
    live = patch >= 0
    nonorient = np.zeros(P, bool)
    nonorient[patch[fa[(rel[fa] ^ rel[fb]) != e]]] = True
    closed = np.ones(P, bool)
    closed[patch[open_face & live]] = False
    n = np.bincount(patch[live], minlength=P).astype(np.int64)
    n1 = np.bincount(patch[live], weights=rel[live], minlength=P).astype(np.int64)
    # the volume rule: the patch's own box, the 12-bit grid, the integer determinant
    x = v.astype(np.float64)[f]                                     # [F,3,3]: face, corner, axis
    lo, hi = np.full((P, 3), np.inf), np.full((P, 3), -np.inf)
    np.minimum.at(lo, patch[live], x[live].min(1))
    np.maximum.at(hi, patch[live], x[live].max(1))
    ext = (hi - lo).max(1) if P else np.zeros(0)
    s = np.zeros(P)
    s[ext != 0] = np.float64(GRID_MAX) / ext[ext != 0]
    pl = np.where(live, patch, 0)
    q = np.clip(np.floor((x - lo[pl][:, None, :]) * s[pl][:, None, None]), 0, GRID_MAX) if P else np.zeros_like(x)
    c = 2 * q.astype(np.int64) - GRID_MAX
    A, B, C = c[:, 0], c[:, 1], c[:, 2]
    det = (A[:, 0] * (B[:, 1] * C[:, 2] - B[:, 2] * C[:, 1]) - A[:, 1] * (B[:, 0] * C[:, 2] - B[:, 2] * C[:, 0])
           + A[:, 2] * (B[:, 0] * C[:, 1] - B[:, 1] * C[:, 0]))
    assert np.abs(det[live]).max(initial=0) < 2 ** 39
    applies = ~nonorient & (closed | (open_patches == 'volume'))
    vol = np.zeros(P, np.int64)
    np.add.at(vol, patch[live], ((1 - 2 * rel) * det)[live])
    vol[~applies] = 0
    comp = np.where(vol != 0, vol < 0, n1 > n - n1) & ~nonorient
    flags = (closed * CLOSED + nonorient * NONORIENTABLE + (applies & (vol != 0)) * BY_VOLUME + comp * COMPLEMENTED).astype(np.int32)
    flip = np.zeros(F, np.uint8)
    ok = live & ~nonorient[pl]
    flip[ok] = (rel[ok] ^ comp[pl[ok]]).astype(np.uint8)
    out = f.copy()
    out[flip == 1] = f[flip == 1][:, [0, 2, 1]]
    flipped = np.bincount(patch[live], weights=flip[live], minlength=P).astype(np.int32)
    counts = [P, int(flip.sum()), int(nonorient.sum()), int(e.sum()), int((cnt == 1).sum()), int((cnt >= 3).sum()), int(deg.sum()), 0]
    return dict(faces=out, flip=flip, face_patch=patch.astype(np.int32), root=np.array(roots, np.int32).reshape(-1), n_faces=n.astype(np.int32),
                flipped=flipped, flags=flags, vol=vol, counts=counts)


OUTPUT_KEYS = ('faces', 'flip', 'face_patch', 'root', 'n_faces', 'flipped', 'flags', 'vol')


# ---- the sequential union-find with parity (pdhip_debug_parity_union)
def oracle_parity_union(n, pairs, parity):
    """(root [n] i32, rel [n] u8, conflict [n] u8): a sequential union-find toward the smaller index that carries the parity to the parent; a pair
    whose ends share a root and contradict the stored relations flags the class.  rel means something only where conflict == 0."""
    parent, par = list(range(n)), [0] * n

    def find(x):
        p = 0
        while parent[x] != x:
            p ^= par[x]
            x = parent[x]
        return x, p

    bad = []
    for (a, b), e in zip(np.asarray(pairs).reshape(-1, 2).tolist(), np.asarray(parity).tolist()):
        (ra, pa), (rb, pb) = find(a), find(b)
        if ra == rb:
            if pa ^ pb != e:
                bad.append(a)
            continue
        hi, lo = max(ra, rb), min(ra, rb)
        parent[hi], par[hi] = lo, pa ^ pb ^ e
    fr = [find(x) for x in range(n)]
    root = np.array([r for r, _ in fr], np.int32)
    rel = np.array([p for _, p in fr], np.uint8)
    conflict = np.zeros(n, np.uint8)
    conflict[np.isin(root, root[bad])] = 1
    return root, rel, conflict


# ---- the meshes
TET_OUT = np.ascontiguousarray(TET[:, [0, 2, 1]])                   # TET_V's tetrahedron, outward


def flipped(faces, which):
    """The faces with those of `which` (indices or a bool mask) flipped: (a, b, c) -> (a, c, b)."""
    f = np.array(faces, np.int64)
    f[which] = f[which][:, [0, 2, 1]]
    return f


def random_flips(faces, seed, share=0.5):
    """(faces with a random `share` of them flipped, the bool mask)."""
    mask = np.random.default_rng(seed).random(len(faces)) < share
    return flipped(faces, mask), mask


def shuffle_rotate(faces, seed):
    """(faces in another order with corners rotated, perm, rot): new face k is old face perm[k] rotated left by rot[k]."""
    f = np.asarray(faces, np.int64)
    rng = np.random.default_rng(seed)
    perm, rot = rng.permutation(len(f)), rng.integers(0, 3, len(f))
    g = f[perm]
    return np.ascontiguousarray(np.stack([g[np.arange(len(f)), (rot + k) % 3] for k in range(3)], 1)), perm, rot


def join(parts):
    """Disjoint meshes as one: (vertices, faces, face ranges)."""
    vs, fs, off = [], [], 0
    for v, f in parts:
        vs.append(np.asarray(v, np.float32))
        fs.append(np.asarray(f, np.int64) + off)
        off += len(v)
    return np.concatenate(vs).astype(np.float32), np.concatenate(fs)


def moebius(n=8):
    """A Moebius strip of n quads (2 n faces, 2 n vertices): coherent along the strip, the last quad joins the ends with a half twist."""
    t = 2 * np.pi * np.arange(n) / n
    w = 0.2
    top = np.stack([(1 + w * np.cos(t / 2)) * np.cos(t), (1 + w * np.cos(t / 2)) * np.sin(t), w * np.sin(t / 2)], 1)
    bot = np.stack([(1 - w * np.cos(t / 2)) * np.cos(t), (1 - w * np.cos(t / 2)) * np.sin(t), -w * np.sin(t / 2)], 1)
    v = np.stack([top, bot], 1).reshape(-1, 3).astype(np.float32)
    f = []
    for i in range(n):
        a, b, c, d = 2 * i, 2 * i + 1, 2 * ((i + 1) % n), 2 * ((i + 1) % n) + 1
        if i == n - 1:
            c, d = d, c
        f += [[a, b, d], [a, d, c]]
    return v, np.array(f, np.int64)


def pillow():
    """Two faces on the same three vertices, back to back: closed, volume 0."""
    return np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float32), np.array([[0, 1, 2], [0, 2, 1]], np.int64)


def sheet(nq=5):
    """An open sheet of nq x nq quads in the plane z = 0, every face with the normal +z."""
    g = np.arange(nq + 1)
    v = np.stack([np.tile(g, nq + 1), np.repeat(g, nq + 1), np.zeros((nq + 1) ** 2)], 1).astype(np.float32) / nq
    f = []
    for j in range(nq):
        for i in range(nq):
            a = j * (nq + 1) + i
            f += [[a, a + 1, a + nq + 2], [a, a + nq + 2, a + nq + 1]]
    return v, np.array(f, np.int64)


def two_face_strip():
    return np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0]], np.float32), np.array([[0, 1, 2], [2, 1, 3]], np.int64)


def cap(level=2, z_min=0.2):
    """The faces of icosphere(level) whose centroid lies above z_min: an open cap, outward."""
    v, f = icosphere(level)
    return v, np.ascontiguousarray(f[v[f][:, :, 2].mean(1) > z_min])


def fan():
    """Three triangles on the edge (0, 1): a non-manifold edge and six boundary edges."""
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1]], np.float32)
    return v, np.array([[0, 1, 2], [0, 1, 3], [1, 0, 4]], np.int64)


def tets_on_an_edge():
    """Two outward tetrahedra that share the edge (0, 1) only (Vn = 6, F = 8): the edge lies on four faces."""
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1], [0, -1, 0], [0, 0, -1]], np.float32)
    second = np.array([0, 1, 4, 5])[TET_OUT]
    if signed_volume6(v, second) < 0:
        second = flipped(second, slice(None))
    return v, np.concatenate([TET_OUT, second])


def signed_volume6(vertices, faces):
    """Six times the signed volume, in f64: positive for a closed mesh with outward faces."""
    x = np.asarray(vertices, np.float64)[np.asarray(faces, np.int64)]
    return float(np.einsum('ij,ij->i', x[:, 0], np.cross(x[:, 1], x[:, 2])).sum())


def three_spheres():
    """icosphere(2), icosphere(1) of radius 5e-5 at (50, 50, 50) INVERTED, icosphere(1) of radius 0.3 at (2, 0, 0); the faces' truth (all outward)
    comes second."""
    parts = [icosphere(2), icosphere(1, 5e-5, (50.0, 50.0, 50.0)), icosphere(1, 0.3, (2.0, 0.0, 0.0))]
    v, truth = join(parts)
    f = truth.copy()
    f[320:400] = f[320:400][:, [0, 2, 1]]
    return v, f, truth
