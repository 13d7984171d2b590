"""Helpers of the mesh decimation tests (tests/test_mesh_simplify_cpu.py, tests/test_gpu_mesh_simplify.py): a grid torus, the textbook
SEQUENTIAL greedy quadric-error edge collapse (one priority queue, the cheapest valid edge first) with the validity rules and the position
rule of csrc/simplify_mesh.hip, and the two error metrics.  Nothing here calls libpdhip: the sequential decimator is the yardstick the
device's rounds of independent collapses are measured against."""
import functools
import heapq

import numpy as np

R_MAJOR, R_MINOR = 0.35, 0.15                                     # the torus of synthetic.Solid('torus'): axis y


def torus_sdf(x):
    x = np.asarray(x, np.float64)
    q = np.stack([np.hypot(x[:, 0], x[:, 2]) - R_MAJOR, x[:, 1]], 1)
    return np.linalg.norm(q, axis=1) - R_MINOR


def grid_torus(nu, nv, noise=0.0, seed=0):
    """nu x nv quads round the major / minor circle, two triangles each, counter-clockwise seen from outside; every vertex moved along
    its normal by noise * N(0, 1) -> (vertices f32 [nu nv, 3], faces int64 [2 nu nv, 3])."""
    i, j = np.meshgrid(np.arange(nu), np.arange(nv), indexing='ij')
    a, b = 2 * np.pi * i / nu, 2 * np.pi * j / nv
    nrm = np.stack([np.cos(b) * np.cos(a), np.sin(b), np.cos(b) * np.sin(a)], -1)
    ctr = np.stack([R_MAJOR * np.cos(a), np.zeros_like(a), R_MAJOR * np.sin(a)], -1)
    rng = np.random.default_rng(seed)
    v = ctr + nrm * (R_MINOR + noise * rng.standard_normal((nu, nv, 1)))
    vid = lambda p, q: (p % nu) * nv + (q % nv)
    f = np.concatenate([np.stack([vid(i, j), vid(i, j + 1), vid(i + 1, j + 1)], -1).reshape(-1, 3),
                        np.stack([vid(i, j), vid(i + 1, j + 1), vid(i + 1, j)], -1).reshape(-1, 3)])
    v, f = v.reshape(-1, 3).astype(np.float32), f.astype(np.int64)
    vol = np.einsum('ij,ij->i', v[f[:, 0]].astype(np.float64), np.cross(v[f[:, 1]], v[f[:, 2]]).astype(np.float64)).sum()
    return v, (f if vol > 0 else np.ascontiguousarray(f[:, ::-1]))


def _f32(x):
    return float(np.float32(x))


def _cross(a, b):
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def _sub(a, b):
    return (a[0] - b[0], a[1] - b[1], a[2] - b[2])


def _dot(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def _eval(q, x):
    a00, a01, a02, a11, a12, a22, b0, b1, b2, c = q
    ax = (a00 * x[0] + a01 * x[1] + a02 * x[2], a01 * x[0] + a11 * x[1] + a12 * x[2], a02 * x[0] + a12 * x[1] + a22 * x[2])
    return _dot(x, ax) + 2.0 * (b0 * x[0] + b1 * x[1] + b2 * x[2]) + c


class _Mesh:
    def __init__(self, vertices, faces):
        self.P = [tuple(float(c) for c in p) for p in np.asarray(vertices, np.float32)]
        self.F = [tuple(int(c) for c in t) for t in np.asarray(faces)]
        self.alive = [True] * len(self.F)
        self.star = [set() for _ in self.P]
        for g, t in enumerate(self.F):
            for a in t:
                self.star[a].add(g)
        self.Q = [np.zeros(10) for _ in self.P]
        for t in self.F:
            a, b, c = (self.P[k] for k in t)
            n = _cross(_sub(b, a), _sub(c, a))
            ln = _dot(n, n) ** 0.5
            if not ln > 0:
                continue
            n = (n[0] / ln, n[1] / ln, n[2] / ln)
            d = -_dot(n, a)
            k = 0.5 * ln * np.array([n[0] * n[0], n[0] * n[1], n[0] * n[2], n[1] * n[1], n[1] * n[2], n[2] * n[2], n[0] * d, n[1] * d, n[2] * d, d * d])
            for v in t:
                self.Q[v] = self.Q[v] + k

    def ring(self, g, u):
        p, q, r = self.F[g]
        return (q, r) if p == u else ((r, p) if q == u else (p, q))

    def neighbours(self, u):
        return {self.ring(g, u)[0] for g in self.star[u]}

    def _star_keeps_shape(self, a, b, x):
        o = self.P[a]
        for g in self.star[a]:
            n1, n2 = self.ring(g, a)
            if n1 == b or n2 == b:
                continue
            p, q = self.P[n1], self.P[n2]
            m, n = _cross(_sub(p, o), _sub(q, o)), _cross(_sub(p, x), _sub(q, x))
            dot, l0, l1 = _dot(m, n), _dot(m, m), _dot(n, n)
            if not (l1 > 0.0 and dot > 0.0 and dot * dot > 0.04 * (l0 * l1)):
                return False
        return True

    def edge(self, u, v):
        """(cost, position) of collapsing v into u (u < v), or None if the edge must stay."""
        nu, nv = self.neighbours(u), self.neighbours(v)
        common = len(nu & nv)
        if common != 2 or len(nu) + len(nv) - 2 - common < 3:
            return None
        q = self.Q[u] + self.Q[v]
        a00, a01, a02, a11, a12, a22, b0, b1, b2, _ = q
        pu, pv = self.P[u], self.P[v]
        mid = (0.5 * (pu[0] + pv[0]), 0.5 * (pu[1] + pv[1]), 0.5 * (pu[2] + pv[2]))
        len2 = _dot(_sub(pu, pv), _sub(pu, pv))
        c00, c01, c02 = a11 * a22 - a12 * a12, a02 * a12 - a01 * a22, a01 * a12 - a02 * a11
        c11, c12, c22 = a00 * a22 - a02 * a02, a01 * a02 - a00 * a12, a00 * a11 - a01 * a01
        det, tr = a00 * c00 + a01 * c01 + a02 * c02, (a00 + a11 + a22) / 3.0
        x = None
        if det > 1e-9 * tr * tr * tr:
            x = (-(c00 * b0 + c01 * b1 + c02 * b2) / det, -(c01 * b0 + c11 * b1 + c12 * b2) / det, -(c02 * b0 + c12 * b1 + c22 * b2) / det)
            if not _dot(_sub(x, mid), _sub(x, mid)) <= 4.0 * len2:
                x = None
        if x is None:
            x, best = pu, _eval(q, pu)
            if _eval(q, pv) < best:
                x, best = pv, _eval(q, pv)
            if _eval(q, mid) < best:
                x = mid
        x = (_f32(x[0]), _f32(x[1]), _f32(x[2]))
        cost = max(0.0, _eval(q, x))
        if not cost <= 1.7e308:
            return None
        if not (self._star_keeps_shape(u, v, x) and self._star_keeps_shape(v, u, x)):
            return None
        return cost, x

    def collapse(self, u, v, x):
        self.P[u] = x
        self.Q[u] = self.Q[u] + self.Q[v]
        for g in list(self.star[v]):
            t = tuple(u if a == v else a for a in self.F[g])
            self.star[v].discard(g)
            if len(set(t)) < 3:
                self.alive[g] = False
                for a in self.F[g]:
                    self.star[a].discard(g)
            else:
                self.F[g] = t
                self.star[u].add(g)


@functools.lru_cache(maxsize=None)
def _sequential(vkey, fkey, shape_v, shape_f, target):
    v = np.frombuffer(vkey, np.float32).reshape(shape_v)
    f = np.frombuffer(fkey, np.int64).reshape(shape_f)
    m = _Mesh(v, f)
    stamp = [0] * len(m.P)
    heap = []

    def push_edges_of(w):
        for z in m.neighbours(w):
            a, b = (w, z) if w < z else (z, w)
            e = m.edge(a, b)
            if e is not None:
                heapq.heappush(heap, (e[0], a, b, stamp[a], stamp[b], e[1]))

    for t in m.F:
        for k in range(3):
            a, b = t[k], t[(k + 1) % 3]
            if a < b:
                e = m.edge(a, b)
                if e is not None:
                    heapq.heappush(heap, (e[0], a, b, 0, 0, e[1]))
    nf = len(m.F)
    while nf > target + 1 and heap:
        _, a, b, sa, sb, x = heapq.heappop(heap)
        if stamp[a] != sa or stamp[b] != sb or not m.star[a] or not m.star[b]:
            continue
        m.collapse(a, b, x)
        nf -= 2
        # what an edge's cost or validity reads changed for every edge with an end in the closed neighbourhood of a
        touched = {a} | m.neighbours(a)
        for w in touched:
            stamp[w] += 1
        stamp[b] += 1
        done = set()
        for w in touched:
            for z in m.neighbours(w):
                p, q = (w, z) if w < z else (z, w)
                if (p, q) in done:
                    continue
                done.add((p, q))
                e = m.edge(p, q)
                if e is not None:
                    heapq.heappush(heap, (e[0], p, q, stamp[p], stamp[q], e[1]))
    faces = np.array([t for t, ok in zip(m.F, m.alive) if ok], np.int64)
    used = np.unique(faces)
    new = -np.ones(len(m.P), np.int64)
    new[used] = np.arange(len(used))
    return np.array([m.P[k] for k in used], np.float32), new[faces]


def sequential_qem(vertices, faces, target):
    """The sequential reference: (vertices f32, faces int64) with target (or target + 1) faces, or more if no valid collapse is left.
    Cached per input: compute once, share, leave unchanged."""
    v = np.ascontiguousarray(vertices, np.float32)
    f = np.ascontiguousarray(faces, np.int64)
    ov, of = _sequential(v.tobytes(), f.tobytes(), v.shape, f.shape, int(target))
    return ov.copy(), of.copy()


def face_samples(vertices, faces, per_face=4, seed=0):
    """per_face uniform random points on every face."""
    v = np.asarray(vertices, np.float64)
    f = np.asarray(faces, np.int64)
    rng = np.random.default_rng(seed)
    r1, r2 = np.sqrt(rng.random((len(f), per_face, 1))), rng.random((len(f), per_face, 1))
    a, b, c = v[f[:, 0]][:, None], v[f[:, 1]][:, None], v[f[:, 2]][:, None]
    return ((1 - r1) * a + r1 * (1 - r2) * b + r1 * r2 * c).reshape(-1, 3)


def metrics(in_vertices, out_vertices, out_faces, sdf=torus_sdf):
    """(mean, max) of |sdf| at 4 random points per output face, (mean, max) of the input vertices' distance to the output mesh."""
    from pointdreamer_amd import mesh_checks as mc
    s = np.abs(sdf(face_samples(out_vertices, out_faces)))
    d = mc.point_mesh_distance(in_vertices, out_vertices, out_faces)
    return dict(sdf_mean=float(s.mean()), sdf_max=float(s.max()), v2m_mean=float(d.mean()), v2m_max=float(d.max()))


def topology(n_vertices, faces):
    """Sorted [(faces, euler)] per component."""
    from pointdreamer_amd import mesh_checks as mc
    return sorted((c[2], c[3]) for c in mc.components_euler(n_vertices, faces))
