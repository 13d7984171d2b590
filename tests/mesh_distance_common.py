"""Helpers of the point-to-mesh tests (tests/test_mesh_distance_cpu.py, tests/test_gpu_mesh_distance.py, tools/bench_mesh_distance.py): the all-pairs
float64 oracle of pdhip_closest_on_mesh -- Ericson's region walk as include/pdhip.h states it, every point against every face, op by op in numpy --,
the meshes and points the tests share, analytic distances, and the workspace layout restated.  Nothing here calls libpdhip."""
import functools

import numpy as np

from occupancy_common import _frozen, box_mesh, icosphere, tetrahedron, uniform_points


def _dot(u, w):
    return (u[..., 0] * w[..., 0] + u[..., 1] * w[..., 1]) + u[..., 2] * w[..., 2]


def live_faces(vertices, faces):
    """bool [F]: the face's normal ab x ac is not exactly (0, 0, 0) in float64."""
    v = np.asarray(vertices, np.float32).astype(np.float64)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    with np.errstate(invalid='ignore', over='ignore'):
        a, ab, ac = v[f[:, 0]], v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]]
        nx = ab[:, 1] * ac[:, 2] - ab[:, 2] * ac[:, 1]
        ny = ab[:, 2] * ac[:, 0] - ab[:, 0] * ac[:, 2]
        nz = ab[:, 0] * ac[:, 1] - ab[:, 1] * ac[:, 0]
    return ~((nx == 0) & (ny == 0) & (nz == 0))


def oracle_closest(vertices, faces, points, chunk=128):
    """(d2 [Q] f64, face [Q] i32, closest [Q,3] f64, degenerate faces skipped): float32 inputs widened to float64; the minimum over the live faces
    and the FIRST (= smallest) index that attains it.  A NaN value never wins; a point without any value gets (inf, -1, NaN)."""
    v = np.asarray(vertices, np.float32).astype(np.float64)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    p = np.asarray(points, np.float32).astype(np.float64).reshape(-1, 3)
    live = live_faces(vertices, f)
    index = np.nonzero(live)[0]
    a, b, c = (v[f[index, k]][None] for k in range(3))             # [1, F', 3]
    ab, ac, bc = b - a, c - a, c - b
    d2, face, closest = np.full(len(p), np.inf), np.full(len(p), -1, np.int32), np.full((len(p), 3), np.nan)
    if len(index) == 0:
        return d2, face, closest, int((~live).sum())
    for s in range(0, len(p), chunk):
        q = p[s:s + chunk, None, :]                                # [n, 1, 3]
        with np.errstate(invalid='ignore', divide='ignore', over='ignore'):
            d1, dd2 = _dot(ab, q - a), _dot(ac, q - a)
            d3, d4 = _dot(ab, q - b), _dot(ac, q - b)
            d5, d6 = _dot(ab, q - c), _dot(ac, q - c)
            vc, vb, va, e43, e56 = d1 * d4 - d3 * dd2, d5 * dd2 - d1 * d6, d3 * d6 - d5 * d4, d4 - d3, d5 - d6
            den = 1.0 / ((va + vb) + vc)
            cond = [(d1 <= 0) & (dd2 <= 0), (d3 >= 0) & (d4 <= d3), (vc <= 0) & (d1 >= 0) & (d3 <= 0), (d6 >= 0) & (d5 <= d6),
                    (vb <= 0) & (dd2 >= 0) & (d6 <= 0), (va <= 0) & (e43 >= 0) & (e56 >= 0)]
            cand = [a + 0 * q, b + 0 * q, a + (d1 / (d1 - d3))[..., None] * ab, c + 0 * q, a + (dd2 / (dd2 - d6))[..., None] * ac,
                    b + (e43 / (e43 + e56))[..., None] * bc, (a + ab * (vb * den)[..., None]) + ac * (vc * den)[..., None]]
            x = cand[6]
            for k in range(5, -1, -1):                             # the first case that holds
                x = np.where(cond[k][..., None], cand[k], x)
            val = _dot(q - x, q - x)
        val = np.where(np.isnan(val), np.inf, val)
        j = np.argmin(val, axis=1)
        rows = np.arange(len(j))
        best = val[rows, j]
        ok = np.isfinite(best)
        d2[s:s + chunk] = best
        face[s:s + chunk] = np.where(ok, index[j], -1)
        closest[s:s + chunk] = np.where(ok[:, None], x[rows, j], np.nan)
    return d2, face, closest, int((~live).sum())


# ---- analytic distances
def box_distance(points, half=0.5):
    """The distance to the surface of the axis-aligned box [-half, half]^3, float64: |max(|q| - half, 0)| outside, half - max|q| inside."""
    q = np.abs(np.asarray(points, np.float32).astype(np.float64))
    e = np.maximum(q - half, 0.0)
    outside = np.sqrt((e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2])
    return np.where(q.max(axis=1) > half, outside, half - q.max(axis=1))


def convex_radii(vertices, faces):
    """(r_in, r_out) of a convex mesh round the origin: the smallest distance of a face plane, the largest norm of a vertex."""
    tri = np.asarray(vertices, np.float64)[np.asarray(faces)]
    n = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    plane = np.abs((n * tri[:, 0]).sum(1)) / np.linalg.norm(n, axis=1)
    return float(plane.min()), float(np.linalg.norm(np.asarray(vertices, np.float64), axis=1).max())


def assert_sandwich(points, d, r_in, r_out, slack=1e-12):
    """R - r_out <= d <= R - r_in outside the circumscribed sphere, r_in - R <= d <= r_out - R inside the inscribed one."""
    R = np.linalg.norm(np.asarray(points, np.float32).astype(np.float64), axis=1)
    out, inn = R > r_out, R < r_in
    print('sandwich: outside', int(out.sum()), 'inside', int(inn.sum()), 'of', len(R), 'r_in', r_in, 'r_out', r_out)
    assert out.sum() > len(R) // 5 and inn.sum() > len(R) // 10
    assert np.all(d[out] >= R[out] - r_out - slack) and np.all(d[out] <= R[out] - r_in + slack)
    assert np.all(d[inn] >= r_in - R[inn] - slack) and np.all(d[inn] <= r_out - R[inn] + slack)


# ---- the shared cases (float32 vertices, int64 faces, float32 points).  Cached: shared, leave unchanged.
@functools.lru_cache(maxsize=None)
def mixed_mesh():
    """icosphere(8) with: one triangle spanning the whole box, three repeated-index faces, one collinear face, one unreferenced non-finite vertex:
    the small list, the large list and the skipped faces together.  (vertices, faces, number of degenerate faces)"""
    v, f = icosphere(8)
    n = len(v)
    extra_v = np.array([[-0.5, -0.5, -0.5], [0.5, 0.5, -0.45], [-0.4, 0.5, 0.5],      # spans the box
                        [0.1, 0.1, 0.1], [0.2, 0.2, 0.2], [0.4, 0.4, 0.4],            # collinear (exactly: powers of two times one vector)
                        [np.nan, np.inf, 0.0]], np.float32)                           # never referenced
    extra_v[3:6] = np.array([[0.125, 0.25, 0.0625]], np.float32) * np.array([[1.0], [2.0], [4.0]], np.float32)
    extra_f = np.array([[n, n + 1, n + 2], [3, 3, 9], [5, 7, 5], [11, 11, 11], [n + 3, n + 4, n + 5]], np.int64)
    order = np.concatenate([np.arange(100), [len(f), len(f) + 1], np.arange(100, len(f)), np.arange(len(f) + 2, len(f) + 5)])
    return _frozen(np.concatenate([v, extra_v]), np.ascontiguousarray(np.concatenate([f, extra_f])[order])) + (4,)


@functools.lru_cache(maxsize=None)
def sliver_mesh():
    """icosphere(4) with faces whose closest-point arithmetic is badly conditioned: needle-thin triangles (live: the normal is not exactly zero) and
    triangles far smaller than a cell.  These must reach the large list, and no path may change a bit."""
    v, f = icosphere(4)
    n = len(v)
    rng = np.random.default_rng(77)
    extra_v, extra_f = [], []
    for k in range(24):
        a = rng.uniform(-0.45, 0.45, 3)
        d = rng.normal(size=3)
        d /= np.linalg.norm(d)
        e = np.cross(d, rng.normal(size=3))
        e /= np.linalg.norm(e)
        if k < 12:                                                 # a needle: 0.08 long, 1e-7 .. 1e-5 wide
            tri = [a, a + 0.08 * d, a + 0.04 * d + 10.0 ** rng.uniform(-7, -5) * e]
        else:                                                      # a speck: edges of 1e-6 .. 1e-4
            h = 10.0 ** rng.uniform(-6, -4)
            tri = [a, a + h * d, a + h * e]
        extra_f.append([n + len(extra_v) + i for i in range(3)])
        extra_v += tri
    return _frozen(np.concatenate([v, np.array(extra_v, np.float32)]), np.concatenate([f, np.array(extra_f, np.int64)]))


@functools.lru_cache(maxsize=None)
def shared_case(kind):
    """(vertices, faces, points)"""
    if kind == 'ico8':
        return icosphere(8) + (uniform_points(3001, 51, 0.7),)
    if kind == 'box':
        return box_mesh() + (uniform_points(3001, 52, 0.7),)
    if kind == 'tetra':
        v, f = tetrahedron()
        return v, f, _scaled(uniform_points(2003, 53, 0.5), 0.03, 0.105)
    if kind == 'single':
        v, f = icosphere(4)
        return v, np.ascontiguousarray(f[17:18]), uniform_points(1001, 54, 0.7)
    if kind == 'mixed':
        return mixed_mesh()[:2] + (uniform_points(2001, 55, 0.7),)
    if kind == 'far':
        return icosphere(4) + (_scaled(uniform_points(1501, 56, 0.7), 40.0, 0.0),)
    if kind == 'sliver':
        return sliver_mesh() + (uniform_points(1501, 57, 0.6),)
    if kind == 'crowded':                                         # 5 120 faces: with 8 cells per axis the rings of a point near the centre hold more than the ring scan takes
        return icosphere(16) + (np.ascontiguousarray(np.concatenate([uniform_points(301, 58, 0.2), uniform_points(200, 59, 0.7)])),)
    if kind == 'long_large':                                      # 8 820 faces: all on the large list (path 1) they are more than a query scans by itself
        return icosphere(21) + (uniform_points(129, 60, 0.7),)
    raise ValueError(kind)


def _scaled(points, scale, shift):
    return _frozen((points.astype(np.float64) * scale + shift).astype(np.float32))[0]


@functools.lru_cache(maxsize=None)
def oracle_cached(kind):
    """(d2, face, closest, degenerate faces) of the oracle on a shared case."""
    d2, face, closest, ndeg = oracle_closest(*shared_case(kind))
    return _frozen(d2, face, closest) + (ndeg,)


@functools.lru_cache(maxsize=None)
def vertex_and_midpoint_queries():
    """The vertices of icosphere(8) (642) and the float32 midpoint of the first edge of every face (1 280)."""
    v, f = icosphere(8)
    mid = ((v[f[:, 0]] + v[f[:, 1]]) * np.float32(0.5)).astype(np.float32)
    return _frozen(np.ascontiguousarray(np.concatenate([v, mid])))[0]


# ---- the workspace layout of pdhip_closest_on_mesh, restated (csrc/mesh_distance.hip: carve_mesh_distance; every region starts on a multiple of 256 bytes)
CELLS_MAX, F_MAX, Q_MAX = 96, 1 << 23, 1 << 26


def closest_workspace_bytes(F, Q):
    n = max(F, Q, 1)
    regions = [8 * n, 8 * n, 4 * n, 4 * n, 4 * 2 * 256 * ((n + 2047) // 2048),      # radix sort: keys x 2, values x 2, digit histograms
               40 * F,                                                               # faces in key order: nine f32 coordinates and the index
               16 * Q,                                                               # sorted queries as (x, y, z, index)
               4 * (CELLS_MAX ** 3 + 2),                                             # cell starts, start of the large list, start of the degenerate faces
               4 * Q, 8 * 16 * Q, 4 * 16 * Q,                                        # queries left to the all-faces scan, its per-slab minima (d2, face)
               4 * 32]                                                               # boxes, bad-input counts, counters
    off = 0
    for r in regions:
        off = (off + 255) // 256 * 256 + r
    return off + 256
