"""The stages of the surface reconstruction (pointdreamer_amd/csrc/surface_recon.hip), one plain numpy function each, written from the definitions in
that file's header comment and in include/pdhip.h: no torch, no scipy, nothing of the kernels' structure (no cell list, no gather, no workgroups).
tests/test_gpu_spr_stages.py holds the device's intermediates to these functions, tests/test_spr_stages_cpu.py holds these functions to analytic cases.

Where a stage's result must equal the device's bit for bit, the function evaluates the kernel's expression in np.float32 with the kernel's association
(the geometry units are compiled without contraction: one rounding per operation).  Where it carries a bound, it is evaluated in float64.

A grid is a dict(h, ox, oy, oz, M) of np.float32 values and an int: node (i, j, k) lies at o + (i, j, k) h, M nodes per axis, arrays are [k, j, i]
(x fastest), as the `info` of pdhip_surface_recon describes it."""
import os
import sys

import numpy as np

F32, F64 = np.float32, np.float64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def make_grid(h, ox, oy, oz, M):
    return dict(h=F32(h), ox=F32(ox), oy=F32(oy), oz=F32(oz), M=int(M))


def d2_f32(S, q):
    """(dx dx + dy dy) + dz dz in float32, dx = s - q, for points S [..., 3] against q [..., 3] (broadcast)."""
    S, q = np.asarray(S, F32), np.asarray(q, F32)
    dx, dy, dz = S[..., 0] - q[..., 0], S[..., 1] - q[..., 1], S[..., 2] - q[..., 2]
    return (dx * dx + dy * dy) + dz * dz


# ---- a. k nearest neighbours
def knn_rows(P, k, chunk=512):
    """The k smallest of the float32 distances from every point to all points (itself included), ascending: [N, k] float32."""
    P = np.asarray(P, F32)
    out = np.empty((len(P), k), F32)
    for a in range(0, len(P), chunk):
        d = d2_f32(P[None, :, :], P[a:a + chunk, None, :])
        out[a:a + chunk] = np.sort(np.partition(d, k - 1, axis=1)[:, :k], axis=1)
    return out


def row_distances(P, knn):
    """The same float32 distances from point i to the points knn[i, :]: [N, k] float32, in the order of knn."""
    P = np.asarray(P, F32)
    return d2_f32(P[knn], P[:, None, :])


# ---- b. the unoriented normal
def normal_direction(P, rows):
    """rows [N, k] indices.  float64 covariance (not divided by k) of the k points about their mean, np.linalg.eigh -> (unit eigenvector of the
    smallest eigenvalue [N, 3], eigenvalues ascending [N, 3])."""
    X = np.asarray(P, F32)[rows].astype(F64)
    D = X - X.mean(axis=1, keepdims=True)
    lam, vec = np.linalg.eigh(np.einsum('nka,nkb->nab', D, D))
    return vec[:, :, 0], lam


# ---- c. orientation
def cloud_box(P):
    P = np.asarray(P, F32).astype(F64)
    mn, mx = P.min(0), P.max(0)
    return mn, mx, float((mx - mn).max())


def fibonacci_eyes(P, n_eyes, eye_radius):
    """n_eyes points of the Fibonacci lattice on the sphere of radius eye_radius * (largest extent) round the centre of the cloud's box: [V, 3] f64."""
    mn, mx, ext = cloud_box(P)
    c, radius = 0.5 * (mn + mx), eye_radius * ext
    i = np.arange(n_eyes, dtype=F64)
    y = 1.0 - 2.0 * (i + 0.5) / F64(n_eyes)
    r = np.sqrt(np.maximum(0.0, 1.0 - y * y))
    th = i * 2.39996322972865332
    return np.stack([c[0] + radius * r * np.cos(th), c[1] + radius * y, c[2] + radius * r * np.sin(th)], 1)


def _dot_f32(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def orient(P, n, knn, eyes, vis, rounds=32):
    """The three rules on normals n [N, 3] f32 (any signs) -> (normals f32, state [N] in 0 (left as it came) / 1 / 2 / 3 = the rule, counts [4]).
    1. the eyes that see point i vote with the sign of n . (eye - p), float64, summed left to right; the normal turns when the sum is negative, and is
       decided when the sum is not zero;
    2. up to `rounds` Jacobi rounds: an undecided point takes the majority of sign(n_i . n_j), float32 (x x + y y) + z z, over the neighbours j that
       were decided BEFORE the round; rounds stop when one decides nobody;
    3. what is left takes the sign of its nearest decided neighbour (float32 distance, ties to the smaller index); none among its k: it stays."""
    P, n = np.asarray(P, F32), np.array(n, F32)
    knn, vis = np.asarray(knn).astype(np.int64), np.asarray(vis).astype(bool)
    N = len(P)
    p64, n64 = P.astype(F64), n.astype(F64)
    s = np.zeros(N, np.int64)
    for v in range(len(eyes)):
        d = n64[:, 0] * (eyes[v, 0] - p64[:, 0]) + n64[:, 1] * (eyes[v, 1] - p64[:, 1]) + n64[:, 2] * (eyes[v, 2] - p64[:, 2])
        s += np.where(vis[v], np.sign(d).astype(np.int64), 0)
    n[s < 0] = -n[s < 0]
    state = (s != 0).astype(np.int64)
    counts = [int(state.sum()), 0, 0, 0]
    for _ in range(rounds):
        und = np.flatnonzero(state == 0)
        nb = knn[und]
        d = _dot_f32(n[und][:, None, :], n[nb])
        votes = np.where(state[nb] != 0, np.sign(d).astype(np.int64), 0).sum(1)
        hit = votes != 0
        if not hit.any():
            break
        new_n, new_state = n.copy(), state.copy()
        turn = und[votes < 0]
        new_n[turn] = -n[turn]
        new_state[und[hit]] = 2
        n, state = new_n, new_state
        counts[1] += int(hit.sum())
    und = np.flatnonzero(state == 0)
    nb = knn[und]
    d2 = np.where(state[nb] != 0, d2_f32(P[nb], P[und][:, None, :]), np.inf)
    has = np.isfinite(d2).any(1)
    best_d = d2.min(1, keepdims=True)
    best = np.where(d2 == best_d, nb, np.iinfo(np.int64).max).min(1)            # ties: the smaller index
    und, best = und[has], best[has]
    d = _dot_f32(n[und], n[best])
    out = n.copy()
    out[und[d < 0]] = -n[und[d < 0]]
    state[und] = 3
    counts[2], counts[3] = int(len(und)), int((state == 0).sum())
    return out, state, counts


# ---- d. sample weights
def sample_weights(P, n, R, chunk=512, terms=False):
    """a_p n_p / |n_p|, a_p = 1 / sum_q w(|p - q|), w(r) = (1 - r^2 / R^2)^3 inside R (the point counts itself), float64, all pairs: [N, 3].
    terms: also dict(rho, m = points within R, s2 = sum u^2, s3 = sum u^3) per point, for the bound of the test."""
    P64, n64, R = np.asarray(P, F32).astype(F64), np.asarray(n, F32).astype(F64), F64(R)
    N = len(P64)
    rho, m, s2 = np.zeros(N), np.zeros(N, np.int64), np.zeros(N)
    x, y, z = (np.ascontiguousarray(P64[:, a]) for a in range(3))
    for a in range(0, N, chunk):
        dx, dy, dz = x[None, :] - x[a:a + chunk, None], y[None, :] - y[a:a + chunk, None], z[None, :] - z[a:a + chunk, None]
        u = 1.0 - (dx * dx + dy * dy + dz * dz) / (R * R)
        u = np.where(u > 0, u, 0.0)
        u2 = u * u
        rho[a:a + chunk], m[a:a + chunk], s2[a:a + chunk] = (u2 * u).sum(1), (u > 0).sum(1), u2.sum(1)
    l = np.linalg.norm(n64, axis=1)
    out = n64 / (l * rho)[:, None]
    return (out, dict(rho=rho, m=m, s2=s2, s3=rho)) if terms else out


# ---- d. the right-hand side
def node_coords(grid):
    """o + float32(i) h in float32, promoted: three [M] float64 arrays."""
    i = np.arange(grid['M'], dtype=F32)
    return tuple((grid[o] + i * grid['h']).astype(F64) for o in ('ox', 'oy', 'oz'))


def rhs(P, snrm, grid, R, chunk=1000, terms=False, rim=2.0 ** -18):
    """f = -div V up to a constant: f(x) = - sum_p u^2 (a_p . (x - p)) over the points with u = 1 - |x - p|^2 / R^2 > 0, float64, SCATTERED from
    every point to the nodes round it; boundary nodes are 0.  P [N, 3] and snrm [N, 3] (normal times sample weight) in the same order: [M, M, M].
    terms: also the per-node sums of the test's bound, dict(m = contributing points, su = sum u S, su2 = sum u^2 S, srim = sum of S over the points
    with |u| <= rim, whether they contribute or not), S = |a_x d_x| + |a_y d_y| + |a_z d_z|."""
    P64, A, R = np.asarray(P, F32).astype(F64), np.asarray(snrm, F32).astype(F64), F64(R)
    M, h = grid['M'], F64(grid['h'])
    X = node_coords(grid)
    W = int(np.ceil(2.0 * R / h)) + 3
    off = np.arange(W)
    n3 = M * M * M
    acc = np.zeros(n3)
    T = dict(m=np.zeros(n3), su=np.zeros(n3), su2=np.zeros(n3), srim=np.zeros(n3)) if terms else None
    for a in range(0, len(P64), chunk):
        p, av = P64[a:a + chunk], A[a:a + chunk]
        idx, d = [], []
        for ax in range(3):
            i0 = np.floor((p[:, ax] - R - X[ax][0]) / h).astype(np.int64) - 1
            ii = i0[:, None] + off[None, :]
            ok = (ii >= 1) & (ii <= M - 2)                           # interior nodes only
            ii = np.clip(ii, 0, M - 1)
            idx.append((ii, ok))
            d.append(X[ax][ii] - p[:, ax:ax + 1])
        dx, dy, dz = d[0][:, None, None, :], d[1][:, None, :, None], d[2][:, :, None, None]
        u = 1.0 - (dx * dx + dy * dy + dz * dz) / (R * R)
        ok = idx[0][1][:, None, None, :] & idx[1][1][:, None, :, None] & idx[2][1][:, :, None, None]
        flat = (idx[2][0][:, :, None, None] * M + idx[1][0][:, None, :, None]) * M + idx[0][0][:, None, None, :]
        live = ok & (u >= -rim)                                      # the pairs that count: inside the support, or on its rim
        ex, ey, ez = (np.broadcast_to(av[:, c][:, None, None, None], u.shape)[live] * np.broadcast_to(dd, u.shape)[live]
                      for c, dd in enumerate((dx, dy, dz)))
        u, flat = u[live], flat[live]
        use = u > 0
        acc += np.bincount(flat[use], weights=(u * u * (ex + ey + ez))[use], minlength=n3)
        if terms:
            S = np.abs(ex) + np.abs(ey) + np.abs(ez)
            T['m'] += np.bincount(flat[use], minlength=n3)
            T['su'] += np.bincount(flat[use], weights=(u * S)[use], minlength=n3)
            T['su2'] += np.bincount(flat[use], weights=(u * u * S)[use], minlength=n3)
            near = np.abs(u) <= rim
            T['srim'] += np.bincount(flat[near], weights=S[near], minlength=n3)
    f = (-acc).reshape(M, M, M)
    if terms:
        return f, {k: v.reshape(M, M, M) for k, v in T.items()}
    return f


# ---- d. the solve
def laplacian(x):
    """A x, A = 6 I - (the six neighbours), the unknowns are the interior nodes and the boundary values are zero: [M, M, M] in the dtype of x, 0 on the
    boundary.  The neighbours are added as ((x- + x+) + (y- + y+)) + (z- + z+)."""
    out = np.zeros_like(x)
    c = x[1:-1, 1:-1, 1:-1]
    s = ((x[1:-1, 1:-1, :-2] + x[1:-1, 1:-1, 2:]) + (x[1:-1, :-2, 1:-1] + x[1:-1, 2:, 1:-1])) + (x[:-2, 1:-1, 1:-1] + x[2:, 1:-1, 1:-1])
    out[1:-1, 1:-1, 1:-1] = x.dtype.type(6) * c - s
    return out


def true_residual(f, x):
    """|f - A x| / |f| in float64."""
    f64, x64 = np.asarray(f).astype(F64), np.asarray(x).astype(F64)
    return float(np.sqrt(((f64 - laplacian(x64)) ** 2).sum() / (f64 ** 2).sum()))


def _dot64(a, b):
    return float((a.astype(F64) * b.astype(F64)).sum())


def cg_f32(f, tol=1.0e-4, cap=100000):
    """Conjugate gradients with the kernel's recurrence in float32 and float64 reductions: x = 0, r = f; per iteration stop unless rr > tol^2 ff, beta =
    float32(rr / rr_prev), p = r + beta p and q = A r + beta q on the interior, alpha = float32(rr / pq), x += alpha p, r -= alpha q.
    -> (x, iterations, recurrence residual sqrt(rr / ff) as float32, true residual in float64).  It measures rounding drift, nothing else."""
    f = np.asarray(f, F32)
    x, r = np.zeros_like(f), f.copy()
    p, q = np.zeros_like(f), np.zeros_like(f)
    inner = (slice(1, -1),) * 3
    ff = rr = _dot64(f, f)
    tol2 = F64(F32(tol) * F32(tol))
    rr_prev, it = 0.0, 0
    while rr > tol2 * ff and it < cap:
        ar = laplacian(r)
        if it == 0:
            p[inner], q[inner] = r[inner], ar[inner]
        else:
            beta = F32(rr / rr_prev)
            p[inner], q[inner] = r[inner] + beta * p[inner], ar[inner] + beta * q[inner]
        pq = _dot64(p, q)
        alpha = F32(rr / pq) if pq > 0.0 else F32(0)
        x = x + alpha * p
        r = r - alpha * q
        rr_prev, rr = rr, _dot64(r, r)
        it += 1
    res = F32(np.sqrt(rr / ff)) if ff > 0.0 else F32(0)
    return x, it, res, true_residual(f, x)


def cg_f64(f, tol=1.0e-4, cap=100000):
    """Textbook conjugate gradients in float64 on the same system -> (x, iterations)."""
    f = np.asarray(f).astype(F64)
    x, r = np.zeros_like(f), f.copy()
    r[0] = r[-1] = r[:, 0] = r[:, -1] = 0.0
    r[:, :, 0] = r[:, :, -1] = 0.0
    p = r.copy()
    ff = rr = float((r * r).sum())
    it = 0
    while rr > tol * tol * ff and it < cap:
        q = laplacian(p)
        alpha = rr / float((p * q).sum())
        x += alpha * p
        r -= alpha * q
        rr, rr_prev = float((r * r).sum()), rr
        p = r + (rr / rr_prev) * p
        it += 1
    return x, it


# ---- e. the iso value
def trilinear_f32(chi, grid, P):
    """chi interpolated at the points P, every operation in float32 in the kernel's order: [N] float32."""
    chi, P = np.asarray(chi, F32), np.asarray(P, F32)
    M, h = grid['M'], grid['h']
    top = F32(M - 1)
    g = [np.minimum(np.maximum((P[:, a] - grid[o]) / h, F32(0)), top) for a, o in enumerate(('ox', 'oy', 'oz'))]
    i, j, k = (np.minimum(v.astype(np.int64), M - 2) for v in g)
    tx, ty, tz = g[0] - i.astype(F32), g[1] - j.astype(F32), g[2] - k.astype(F32)
    c = lambda dk, dj, di: chi[k + dk, j + dj, i + di]
    c00 = c(0, 0, 0) + tx * (c(0, 0, 1) - c(0, 0, 0))
    c10 = c(0, 1, 0) + tx * (c(0, 1, 1) - c(0, 1, 0))
    c01 = c(1, 0, 0) + tx * (c(1, 0, 1) - c(1, 0, 0))
    c11 = c(1, 1, 0) + tx * (c(1, 1, 1) - c(1, 1, 0))
    c0, c1 = c00 + ty * (c10 - c00), c01 + ty * (c11 - c01)
    return c0 + tz * (c1 - c0)


def iso_value(chi, grid, P):
    """The mean of chi at the points: float32 interpolation, float64 mean (a float64)."""
    return float(trilinear_f32(chi, grid, P).astype(F64).sum() / F64(len(P)))


# ---- f. marching cubes
_TABLE = []


def mc_table():
    """tools/gen_mc_tables.build(): per corner mask the triangles as triples of edge ids (edge e = 4 axis + u + 2 v)."""
    if not _TABLE:
        tools = os.path.join(ROOT, 'tools')
        if tools not in sys.path:
            sys.path.insert(0, tools)
        import gen_mc_tables
        _TABLE.append(gen_mc_tables.build())
    return _TABLE[0]


def marching_cubes(chi, iso, grid):
    """chi [M, M, M] float32, inside = chi > iso -> (eflag [M, M, M] uint8, vertices [Vn, 3] float32, faces [F, 3] int64).
    A node owns the grid edges that leave it along +x, +y, +z (bits 0, 1, 2 of eflag: the edge crosses); one vertex per crossing edge, numbered in
    node order (x fastest), then axis order; t = (iso - a) / (b - a) clamped to [1/1024, 1 - 1/1024], a at the owning node; the vertex lies at
    o + (float32(i) + t) h along the edge's axis, all float32.  Faces: cells in node order, the table's triangles in table order."""
    chi, iso = np.asarray(chi, F32), F32(iso)
    M, h = grid['M'], grid['h']
    ins = chi > iso
    fl = np.zeros((M, M, M), np.uint8)
    fl[:, :, :-1] |= (ins[:, :, 1:] != ins[:, :, :-1]).astype(np.uint8)
    fl[:, :-1, :] |= (ins[:, 1:, :] != ins[:, :-1, :]).astype(np.uint8) << 1
    fl[:-1, :, :] |= (ins[1:, :, :] != ins[:-1, :, :]).astype(np.uint8) << 2
    flat = fl.ravel()
    pop = np.array([bin(v).count('1') for v in range(8)], np.int64)
    vcnt = pop[flat]
    vbase = np.cumsum(vcnt) - vcnt
    nv = int(vcnt.sum())
    verts = np.zeros((nv, 3), F32)
    cf = chi.ravel()
    step = (1, M, M * M)
    lo, hi = F32(1.0) / F32(1024.0), F32(1.0) - F32(1.0) / F32(1024.0)
    for ax in range(3):
        n = np.flatnonzero((flat >> ax) & 1)
        a, b = cf[n], cf[n + step[ax]]
        with np.errstate(invalid='ignore', divide='ignore'):
            t = (iso - a) / (b - a)
        t = np.fmin(np.fmax(t, lo), hi)                              # (fmaxf / fminf return the other operand for a NaN)
        t = np.where(np.isnan(t), F32(0.5), t).astype(F32)
        vid = vbase[n] + pop[flat[n] & ((1 << ax) - 1)]
        ijk = (n % M, (n // M) % M, n // (M * M))
        for c, o in enumerate(('ox', 'oy', 'oz')):
            e = ijk[c].astype(F32)
            verts[vid, c] = grid[o] + (e + t if c == ax else e) * h
    # faces
    table = mc_table()
    w = np.zeros((M - 1, M - 1, M - 1), np.int64)
    for c in range(8):
        di, dj, dk = c & 1, (c >> 1) & 1, c >> 2
        w |= ins[dk:M - 1 + dk, dj:M - 1 + dj, di:M - 1 + di].astype(np.int64) << c
    mask = np.zeros((M, M, M), np.int64)
    mask[:-1, :-1, :-1] = w
    mask = mask.ravel()
    ntri = np.array([len(t) for t in table], np.int64)
    tcnt = ntri[mask]
    tbase = np.cumsum(tcnt) - tcnt
    faces = np.zeros((int(tcnt.sum()), 3), np.int64)
    for m in np.unique(mask):
        if not ntri[m]:
            continue
        n = np.flatnonzero(mask == m)
        for t, tri in enumerate(table[m]):
            for c, e in enumerate(tri):
                ax, u, v = e >> 2, e & 1, (e >> 1) & 1
                dx, dy, dz = (0 if ax == 0 else u), (0 if ax == 1 else (u if ax == 0 else v)), (0 if ax == 2 else v)
                nn = n + dx + dy * M + dz * M * M
                faces[tbase[n] + t, c] = vbase[nn] + pop[flat[nn] & ((1 << ax) - 1)]
    return fl, verts, faces
