"""Helpers of the mesh smoothing tests (tests/test_mesh_smooth_cpu.py, tests/test_gpu_mesh_smooth.py): the numpy oracle of the definition in
include/pdhip.h (f64 state, per vertex the neighbours of its CSR row added ONE BY ONE in row order, one division, one subtraction, one
multiplication, one addition; Jacobi passes; one rounding to f32 at the end), the boundary oracle (ordered pairs that occur exactly once among the
6 F pairs of the faces) and the meshes of the cases.  Nothing here calls libpdhip."""
import functools

import numpy as np

from mesh_simplify_common import grid_torus

MESHLAB = (0.5, -0.53)                                             # MeshLab's defaults for "Taubin Smooth"
TAUBIN = (0.33, -0.34)                                             # the pair of Taubin's paper


def csr(num_vertices, faces):
    """(rowptr, colidx) int32: unique neighbours, ascending rows, self pairs dropped (mesh_utils.neighbour_csr's host path)."""
    from pointdreamer_amd import mesh_utils
    return mesh_utils.neighbour_csr(int(num_vertices), np.asarray(faces, np.int64))


def oracle_pass(x, rowptr, colidx, s, held):
    """One Jacobi pass on the f64 state x [Vn,3]: the row sum by a loop over k = 0 .. max degree - 1 that adds x[colidx[rowptr + k]] under a mask, so
    every vertex's sum runs in row order."""
    rp = rowptr.astype(np.int64)
    deg = rp[1:] - rp[:-1]
    acc = np.zeros_like(x)
    for k in range(int(deg.max()) if len(deg) else 0):
        on = deg > k
        j = colidx[np.where(on, rp[:-1] + k, 0)]
        acc = np.where(on[:, None], acc + x[j], acc)
    move = (deg > 0) & ~held
    with np.errstate(divide='ignore', invalid='ignore'):
        m = acc / deg.astype(np.float64)[:, None]
    d = m - x
    t = s * d
    return np.where(move[:, None], x + t, x)


def oracle_smooth(vertices, faces, steps=10, lam=0.5, mu=-0.53, boundary='fixed', fixed=None, return_counts=False):
    v = np.asarray(vertices, np.float32)
    Vn = len(v)
    rowptr, colidx = csr(Vn, faces)
    held = np.zeros(Vn, bool)
    if boundary == 'fixed':
        held |= oracle_boundary(faces, Vn)[0]
    if fixed is not None:
        held |= np.asarray(fixed) != 0
    x = v.astype(np.float64)
    for _ in range(steps):
        x = oracle_pass(x, rowptr, colidx, np.float64(lam), held)
        if mu != 0:
            x = oracle_pass(x, rowptr, colidx, np.float64(mu), held)
    out = x.astype(np.float32)
    if return_counts:
        deg = np.diff(rowptr.astype(np.int64))
        return out, dict(moved=int(((deg > 0) & ~held).sum()), held=int(((deg > 0) & held).sum()), isolated=int((deg == 0).sum()), steps=steps)
    return out


def oracle_boundary(faces, num_vertices):
    """(mask [Vn] bool, dict(boundary_vertices, boundary_edges, nonmanifold_edges)) from the list of the 6 F ordered pairs, self pairs dropped."""
    f = np.asarray(faces, np.int64)
    Vn = int(num_vertices)
    a = np.concatenate([f[:, 0], f[:, 1], f[:, 2], f[:, 1], f[:, 2], f[:, 0]])
    b = np.concatenate([f[:, 1], f[:, 2], f[:, 0], f[:, 0], f[:, 1], f[:, 2]])
    keep = a != b
    key, n = np.unique(a[keep] * Vn + b[keep], return_counts=True)
    mask = np.zeros(Vn, bool)
    mask[key[n == 1] // Vn] = True
    up = key // Vn < key % Vn
    return mask, dict(boundary_vertices=int(mask.sum()), boundary_edges=int(((n == 1) & up).sum()), nonmanifold_edges=int(((n > 2) & up).sum()))


# ---- the meshes
TET = np.array([[0, 1, 2], [0, 3, 1], [1, 3, 2], [2, 3, 0]], np.int64)
TET_V = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], np.float32)


def bipyramid(n=300):
    """Two apexes (vertices 0 and 1) over a rim of n vertices: rows of n and of 4 (Vn = n + 2, F = 2 n)."""
    k = np.arange(n)
    a = 2 * np.pi * k / n
    rim = np.stack([0.4 * np.cos(a) * (1 + 0.05 * np.sin(7 * a)), 0.03 * np.cos(5 * a), 0.4 * np.sin(a)], 1)
    v = np.concatenate([[[0, 0.3, 0], [0, -0.3, 0]], rim]).astype(np.float32)
    r0, r1 = 2 + k, 2 + (k + 1) % n
    f = np.concatenate([np.stack([np.zeros(n, np.int64), r1, r0], 1), np.stack([np.ones(n, np.int64), r0, r1], 1)])
    return v, f.astype(np.int64)


@functools.lru_cache(maxsize=None)
def _noisy_sphere():
    from pointdreamer_amd import synthetic
    return synthetic.icosphere(16, noise=0.01, seed=1)


def noisy_sphere():
    """synthetic.icosphere(16, noise=0.01, seed=1): radius 0.5, radial noise of 0.005 RMS (Vn = 2562, F = 5120)."""
    v, f = _noisy_sphere()
    return v.copy(), f.copy()


def noisy_torus(nu=96, nv=40, noise=0.005, seed=0):
    return grid_torus(nu, nv, noise=noise, seed=seed)


def torus_with_spare(n):
    """grid_torus(n, n) with noise and one vertex no face names at the end (Vn = n n + 1: 257 for n = 16, 1025 for n = 32)."""
    v, f = grid_torus(n, n, noise=0.004, seed=n)
    return np.concatenate([v, [[9.0, -9.0, 0.25]]]).astype(np.float32), f


def sphere_cap():
    """The faces of the noisy icosphere with centroid y > 0.1: an open mesh with one rim; the vertices below it are unreferenced."""
    v, f = noisy_sphere()
    keep = v[f].astype(np.float64).mean(1)[:, 1] > 0.1
    return v, np.ascontiguousarray(f[keep])


def fan():
    """Three triangles on the edge (0, 1): that edge is not a boundary edge, the six outer ones are."""
    v = np.array([[0, 0, 0], [0, 0, 1], [1, 0, 0.5], [-0.5, 0.8, 0.5], [-0.5, -0.8, 0.5]], np.float32)
    return v, np.array([[0, 1, 2], [0, 1, 3], [0, 1, 4]], np.int64)


def relabel(vertices, faces, perm):
    """The same mesh with vertex v renamed perm[v]."""
    perm = np.asarray(perm, np.int64)
    v = np.empty_like(vertices)
    v[perm] = vertices
    return v, perm[np.asarray(faces, np.int64)]


def rms(x):
    return float(np.sqrt(np.mean(np.square(np.asarray(x, np.float64)))))
