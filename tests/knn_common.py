"""Shared by tests/test_knn_cpu.py, tests/test_gpu_knn.py and tests/test_gpu_outliers.py: the clouds and the numpy float64 oracles of
pdhip_knn_points and pdhip_sor_filter (include/pdhip.h).  Nothing here is imported by the product.

knn oracle: all pairs, d2 = (dx*dx + dy*dy) + dz*dz with the float32 inputs widened to float64, one numpy operation per rounding; per row the k
smallest (d2, index) pairs in ascending lexicographic order.  A stable argsort of d2 along the row IS np.lexsort((index, d2)) per row (equal keys
keep their index order); test_knn_cpu.py checks the two against each other on a cloud full of ties."""
import functools
import math

import numpy as np

SOR_K, SOR_RATIO = 20, 2.0


def all_pairs_d2(q, t):
    q, t = np.asarray(q, np.float32).astype(np.float64), np.asarray(t, np.float32).astype(np.float64)
    dx = q[:, None, 0] - t[None, :, 0]
    dy = q[:, None, 1] - t[None, :, 1]
    dz = q[:, None, 2] - t[None, :, 2]
    return (dx * dx + dy * dy) + dz * dz


def oracle_knn(q, t, k):
    """(d2 [Q,k] float64, idx [Q,k] int32)."""
    d2 = all_pairs_d2(q, t)
    order = np.argsort(d2, axis=1, kind='stable')[:, :k]
    return np.take_along_axis(d2, order, axis=1), order.astype(np.int32)


def lexsort_knn(q, t, k):
    """The same by np.lexsort((index, d2)) row by row."""
    d2 = all_pairs_d2(q, t)
    index = np.arange(d2.shape[1])
    order = np.stack([np.lexsort((index, row))[:k] for row in d2])
    return np.take_along_axis(d2, order, axis=1), order.astype(np.int32)


def lattice(n=8):
    g = np.arange(n, dtype=np.float32)
    return np.stack(np.meshgrid(g, g, g, indexing='ij'), -1).reshape(-1, 3)


def _case(name):
    """(queries, targets, k, hook) -- hook: the (cells_per_axis, path) the case is meant to run under, (0, 0) = the shipped routing."""
    rng = np.random.default_rng(sum(map(ord, name)))               # (a seed per case that does not change between processes)
    u = lambda n: rng.random((n, 3), dtype=np.float32)
    if name == 'random_k1':
        return u(1500), u(3000), 1, (0, 0)
    if name == 'random_k64':
        return u(700), u(3000), 64, (0, 0)
    if name == 'surface_k21':                                      # the filter's own shape: a cloud against itself
        v = rng.standard_normal((3000, 3))
        p = (0.5 * v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)
        return p, p, 21, (0, 0)
    if name == 'k_eq_m':
        return u(100), u(40), 40, (7, 0)                           # every cube short of the whole grid holds fewer than k targets
    if name == 'one_target':
        return u(50), u(1), 1, (0, 0)
    if name == 'q1':
        return u(1), u(2000), 10, (0, 0)
    if name == 'q65':
        return u(65), u(1500), 5, (0, 0)
    if name == 'q129':
        return u(129), u(1500), 5, (0, 0)
    if name == 'lattice_k7':
        return lattice(), lattice(), 7, (0, 0)
    if name == 'lattice_k27':
        return lattice(), lattice(), 27, (0, 0)
    if name == 'identical':
        p = np.tile(np.array([[0.25, -1.5, 3.0]], np.float32), (200, 1))
        return p, p, 10, (0, 0)
    if name == 'dup_boundary':
        # multiples of 0.25 in [0, 1]^3 lie on the faces of a 4-cell grid; every point is there twice (indices i and i + n), and a copy shifted by
        # one ulp sits on the other side of each face
        a = lattice(5) * np.float32(0.25)
        b = np.nextafter(a, np.float32(-1.0)).astype(np.float32)
        base = np.concatenate([a, b, u(150)])
        p = np.concatenate([base, base])
        return p, p, 9, (4, 0)
    if name == 'ring_growth':
        p = u(300)
        return p, p, 32, (32, 0)                                   # 32^3 cells for 300 targets: the first cube holds fewer than k, and a ball of
    if name == 'ring_growth16':                                    # 32 targets has a radius of ~9 cells: most queries pass the last ring
        p = u(300)
        return p, p, 32, (16, 0)                                   # ... of ~5 cells here: the rings grow until the certificate holds
    if name == 'far':
        t = u(4000)
        q = u(200)
        q[:, 0] += np.float32(50.0)                                # 50 box lengths outside the targets
        return q, t, 4, (0, 0)
    if name in ('crowded', 'crowded_box'):
        # 5 000 targets inside one cell's width of a grid over the BOX, 20 elsewhere.  (0, 2) lays the grid over the box: the crowded-cell path;
        # the shipped grid spans the targets between the outer quantiles of every axis, i.e. the cluster
        rng = np.random.default_rng(sum(map(ord, 'crowded')))
        t = np.concatenate([np.float32(0.5) + np.float32(1.0e-3) * rng.random((5000, 3), dtype=np.float32), rng.random((20, 3), dtype=np.float32)])
        t = t[rng.permutation(len(t))]
        return t[::10].copy(), t, 8, ((0, 2) if name == 'crowded_box' else (0, 0))
    if name == 'paths':
        return u(300), u(1200), 12, (0, 0)
    raise KeyError(name)


CASES = ('random_k1', 'random_k64', 'surface_k21', 'k_eq_m', 'one_target', 'q1', 'q65', 'q129', 'lattice_k7', 'lattice_k27', 'identical',
         'dup_boundary', 'ring_growth', 'ring_growth16', 'far', 'crowded', 'crowded_box', 'paths')


@functools.lru_cache(maxsize=None)
def case(name):
    q, t, k, hook = _case(name)
    q, t = np.ascontiguousarray(q, np.float32), np.ascontiguousarray(t, np.float32)
    q.setflags(write=False)
    t.setflags(write=False)
    return q, t, k, hook


@functools.lru_cache(maxsize=None)
def oracle_case(name):
    q, t, k, _ = case(name)
    d2, idx = oracle_knn(q, t, k)
    d2.setflags(write=False)
    idx.setflags(write=False)
    return d2, idx


# ---- statistical outlier removal
@functools.lru_cache(maxsize=None)
def sor_cloud():
    """(points [2032,3] float32, is_surface [2032] bool): 2 000 points on the sphere of radius 0.5 and 32 points uniform in [-1.5, 1.5]^3 that keep
    at least 0.25 from the surface, shuffled."""
    rng = np.random.default_rng(7)
    v = rng.standard_normal((2000, 3))
    sphere = 0.5 * v / np.linalg.norm(v, axis=1, keepdims=True)
    far = []
    while len(far) < 32:
        p = rng.uniform(-1.5, 1.5, 3)
        if abs(np.linalg.norm(p) - 0.5) >= 0.25:
            far.append(p)
    pts = np.concatenate([sphere, np.array(far)])
    surf = np.arange(len(pts)) < 2000
    perm = rng.permutation(len(pts))
    pts, surf = np.ascontiguousarray(pts[perm].astype(np.float32)), surf[perm]
    pts.setflags(write=False)
    return pts, surf


def oracle_sor(knn_d2, std_ratio):
    """dict(mean_d, mean, std, threshold, keep) from knn_d2 [N, k + 1]: slot 0 skipped, the sum sequential in slot order, mu and sigma by math.fsum."""
    d = np.asarray(knn_d2, np.float64)
    N, k = d.shape[0], d.shape[1] - 1
    s = np.zeros(N)
    for j in range(1, k + 1):
        s = s + np.sqrt(d[:, j])
    mean_d = s / float(k)
    mu = math.fsum(mean_d.tolist()) / N
    sd = math.sqrt(math.fsum(((mean_d - mu) ** 2).tolist()) / (N - 1))
    t = mu + std_ratio * sd
    return dict(mean_d=mean_d, mean=mu, std=sd, threshold=t, keep=mean_d <= t)


@functools.lru_cache(maxsize=None)
def oracle_sor_cloud():
    pts, _ = sor_cloud()
    d2, _ = oracle_knn(pts, pts, SOR_K + 1)
    return oracle_sor(d2, SOR_RATIO)


def sor_bounds(N, k):
    """(relative bound of mean_d, relative bound of mu / sigma / t): sqrt within 1 ulp, k sequential adds and one divide; any summation order of N
    non-negative terms, doubled."""
    return (k + 4) * 2.0 ** -52, N * 2.0 ** -52
