"""Helpers of the occupancy tests (tests/test_occupancy_cpu.py, tests/test_gpu_occupancy.py, tools/gen_golden_occupancy.py, tools/bench_occupancy.py):
the all-pairs float64 oracle of pdhip_mesh_contains -- the reference's check_mesh_contains (models/POCO/eval/src/utils/libmesh/inside_mesh.py)
without its triangle hash, every point against every triangle, op by op in numpy's order of operations --, the meshes and points the tests
share, and the workspace layout restated.  Nothing here calls libpdhip."""
import functools
import math

import numpy as np


def oracle_contains(vertices, faces, points, resolution=512, chunk=256, return_counts=False):
    """bool [Q] (and the counts: contained, parities disagree, outside the box).  float32 inputs widened to float64."""
    v = np.asarray(vertices, np.float32).astype(np.float64)
    f = np.asarray(faces, np.int64)
    p = np.asarray(points, np.float32).astype(np.float64).reshape(-1, 3)
    tri = v[f]
    flat = tri.reshape(-1, 3)
    bmin, bmax = flat.min(axis=0), flat.max(axis=0)
    with np.errstate(divide='ignore', invalid='ignore'):
        scale = (resolution - 1) / (bmax - bmin)
        translate = 0.5 - scale * bmin
        tri = scale * tri + translate
        p = scale * p + translate
    inside = np.all((0 <= p) & (p <= resolution), axis=1)
    t1, t2, t3 = tri[:, 0], tri[:, 1], tri[:, 2]
    # check_triangles
    A00, A01, A10, A11 = t1[:, 0] - t3[:, 0], t2[:, 0] - t3[:, 0], t1[:, 1] - t3[:, 1], t2[:, 1] - t3[:, 1]
    detA = A00 * A11 - A01 * A10
    ok = np.abs(detA) != 0.
    s_detA, abs_detA = np.sign(detA), np.abs(detA)
    # compute_intersection_depth
    v1, v2 = t3 - t1, t2 - t1
    n0 = v1[:, 1] * v2[:, 2] - v1[:, 2] * v2[:, 1]
    n1 = v1[:, 2] * v2[:, 0] - v1[:, 0] * v2[:, 2]
    n2 = v1[:, 0] * v2[:, 1] - v1[:, 1] * v2[:, 0]
    s_n2, abs_n2 = np.sign(n2), np.abs(n2)
    above, below = np.zeros(len(p), np.int64), np.zeros(len(p), np.int64)
    for b in range(0, len(p), chunk):
        c = p[b:b + chunk]
        px, py, pz = c[:, None, 0], c[:, None, 1], c[:, None, 2]
        y0, y1 = px - t3[None, :, 0], py - t3[None, :, 1]
        u = (A11[None] * y0 - A01[None] * y1) * s_detA[None]
        w = (-A10[None] * y0 + A00[None] * y1) * s_detA[None]
        uw = u + w
        hit = ok[None] & (0 < u) & (u < abs_detA[None]) & (0 < w) & (w < abs_detA[None]) & (0 < uw) & (uw < abs_detA[None])
        alpha = n0[None] * (t1[None, :, 0] - px) + n1[None] * (t1[None, :, 1] - py)
        depth = np.where(abs_n2[None] != 0, t1[None, :, 2] * abs_n2[None] + alpha * s_n2[None], np.nan)
        rhs = pz * abs_n2[None]
        with np.errstate(invalid='ignore'):
            above[b:b + chunk] = (hit & (depth >= rhs)).sum(axis=1)
            below[b:b + chunk] = (hit & (depth < rhs)).sum(axis=1)
    c1, c2 = inside & (above % 2 == 1), inside & (below % 2 == 1)
    occ = c1 & c2
    if return_counts:
        return occ, [int(occ.sum()), int((c1 != c2).sum()), int((~inside).sum())]
    return occ


# ---- meshes (float32 vertices, int64 faces) and points.  Cached: shared, leave unchanged.
def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def icosphere(n, noise=0.0, seed=0):
    from pointdreamer_amd import synthetic
    return _frozen(*synthetic.icosphere(n, noise=noise, seed=seed))


@functools.lru_cache(maxsize=None)
def uv_sphere(stacks=12, slices=24):
    from pointdreamer_amd import synthetic
    v, f, _ = synthetic.uv_sphere(stacks, slices)
    return _frozen(v, f)


@functools.lru_cache(maxsize=None)
def open_uv_sphere(stacks=12, slices=24, cut=0.2):
    """The uv sphere without the faces whose centroid has y >= cut: not closed, so that the two parities disagree for some points."""
    v, f = uv_sphere(stacks, slices)
    keep = v[f].astype(np.float64).mean(axis=1)[:, 1] < cut
    return _frozen(v, np.ascontiguousarray(f[keep]))


@functools.lru_cache(maxsize=None)
def box_mesh(half=0.5):
    """12 faces: every triangle spans the whole box; the four walls parallel to z project to segments in xy (detA == 0)."""
    v = np.array([[x, y, z] for x in (-half, half) for y in (-half, half) for z in (-half, half)], np.float32)
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    f = np.array([t for a, b, c, d in quads for t in ((a, b, c), (a, c, d))], np.int64)
    return _frozen(v, f)


@functools.lru_cache(maxsize=None)
def tetrahedron(size=0.01):
    v = (np.array([[0, 0, 0], [1, 0, 0.1], [0.2, 1, 0.3], [0.3, 0.3, 1]], np.float64) * size + 0.1).astype(np.float32)
    f = np.array([[0, 2, 1], [0, 1, 3], [1, 2, 3], [0, 3, 2]], np.int64)
    return _frozen(v, f)


@functools.lru_cache(maxsize=None)
def uniform_points(n, seed, half=0.55):
    """n float32 points uniform in [-half, half]^3."""
    rng = np.random.default_rng(seed)
    return _frozen(rng.uniform(-half, half, (n, 3)).astype(np.float32))[0]


@functools.lru_cache(maxsize=None)
def vertex_and_edge_points(seed=5):
    """Points exactly on the xy of every vertex of uv_sphere(12, 24) (266) and on the float32 midpoint of the first edge of every face (528), z
    uniform in [-0.55, 0.55]: the cases the strict inequalities of check_triangles decide."""
    v, f = uv_sphere(12, 24)
    mid = ((v[f[:, 0]] + v[f[:, 1]]) * np.float32(0.5)).astype(np.float32)
    xy = np.concatenate([v[:, :2], mid[:, :2]])
    rng = np.random.default_rng(seed)
    z = rng.uniform(-0.55, 0.55, (len(xy), 1)).astype(np.float32)
    return _frozen(np.ascontiguousarray(np.concatenate([xy, z], axis=1)))[0]


GOLDEN_CASES = ('icosphere', 'edges', 'open')


def golden_inputs(case):
    """(vertices, faces, points, hash_resolution) of the three cases of tests/golden/occupancy_ref.npz (tools/gen_golden_occupancy.py)."""
    if case == 'icosphere':
        return icosphere(12, 0.02, 3) + (uniform_points(4096, 21), 512)
    if case == 'edges':
        return uv_sphere(12, 24) + (vertex_and_edge_points(), 512)
    if case == 'open':
        return open_uv_sphere() + (uniform_points(4096, 22), 512)
    raise ValueError(case)


@functools.lru_cache(maxsize=None)
def oracle_cached(kind, resolution=512):
    """(occ, counts) of the oracle on the shared meshes and points of the GPU tests."""
    v, f, p = shared_case(kind)
    return oracle_contains(v, f, p, resolution, return_counts=True)


def shared_case(kind):
    if kind == 'ico4':
        return icosphere(4) + (uniform_points(5003, 31),)
    if kind == 'ico12':
        return icosphere(12, 0.02, 3) + (uniform_points(4099, 32),)
    if kind in ('ico40', 'ico41'):                             # 32 000 / 33 620 faces: either side of the 32 768 from which 16 lanes take a triangle
        return icosphere(int(kind[3:]), 0.002, 4) + (uniform_points(503, 35),)
    if kind == 'box':
        return box_mesh() + (uniform_points(3001, 33, 0.6),)
    if kind == 'tetra':
        v, f = tetrahedron()
        p = (uniform_points(2003, 34, 0.5).astype(np.float64) * 0.012 + 0.105).astype(np.float32)
        return v, f, p
    raise ValueError(kind)


# ---- the workspace layout of pdhip_mesh_contains, restated (csrc/occupancy.hip: carve_occupancy; every region starts on a multiple of 256 bytes)
def grid_cells(Q):
    return max(1, min(2048, int(math.floor(math.sqrt(Q / 4.0)))))


def contains_workspace_bytes(Q):
    G, n = grid_cells(Q), max(Q, 1)
    regions = [8 * n, 8 * n, 4 * n, 4 * n, 4 * 2 * 256 * ((n + 2047) // 2048),      # radix sort: keys x 2, values x 2, digit histograms
               32 * Q,                                                               # sorted points as (x', y', z', index) in f64
               4 * Q,                                                                # parity words
               4 * (G * G + 1),                                                      # cell starts
               4 * 32]                                                               # boxes, bad-input counts, the three counts
    off = 0
    for r in regions:
        off = (off + 255) // 256 * 256 + r
    return off + 256
