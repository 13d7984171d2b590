"""Shared by tests/test_gpu_spr_stages.py and tests/test_spr_stages_cpu.py: the clouds, the cases and the bounds at which every stage of
csrc/surface_recon.hip is held to oracle/spr_stages.py, and float32 emulations of two stages that show, without a GPU, that the bounds have room for
float32 rounding and none for a wrong result.  Nothing here is imported by the product.

The bounds (u = unit roundoff of float32 = 2^-24; every one is derived from the operations, none from what the device returned):

  b. normal direction: sin(angle(+-n_dev, n_eigh)) <= 2^-23 + 2^-40 lambda_2 / (lambda_1 - lambda_0).  The kernel's eigenvector is computed in float64
     and rounded to float32 once per component: 2^-23 covers the rounding of a unit vector (sqrt(3) u < 2 u).  The closed form's smallest eigenvalue
     carries an ABSOLUTE error of about 4 000 ulp of the largest (trigonometric form: cancellation in q + 2 p cos(...)), 2^-40 lambda_2 with room; an
     eigenvalue error e turns the null vector of A - lambda I by about e / (lambda_1 - lambda_0).  Rows with lambda_1 - lambda_0 < 2^-20 lambda_2 have
     no direction to speak of (collinear neighbours) and are left out, at most 0.5 % of a case.  (The absolute error holds for an eigenvalue that is
     isolated; asked directly for one of a close pair, the trigonometric form is off by (lambda_2 / gap)^2 ulp, and the kernel does not do that:
     closed_form_normal below, both ways.)
  d. sample weights: relative error per component <= u (8 + sum_q (24 u_q^2 + (m + 4) u_q^3) / rho).  u_q = 1 - d2 / R^2 carries at most 8 u absolute
     error (three differences, three squares, two sums, the product with 1 / R^2 rounded twice, the subtraction; all terms <= 1), so u_q^3 moves by
     3 u_q^2 * 8 u; the m-term sum adds (m - 1) u relative to every partial sum and the two products of (u u) u add 2 u, rounded up to (m + 4) u u_q^3;
     the 8 in front: sqrt and its three products, l * rho, the reciprocal, the product with the component, and the rounding of the reference.
  e. right-hand side, per node: |f_dev - f_ref| <= u sum_p (32 u_p + (m + 8) u_p^2) S_p + 2^-36 sum_rim S_p, S_p = |a_x d_x| + |a_y d_y| + |a_z d_z|.
     The term is u_p^2 (a . d): u_p moves by 8 u as above, so u_p^2 by 16 u u_p, and the node's own coordinate o + i h adds as much again to d
     (32 u u_p S_p together); the dot product, the square, the product and the m-term sum are (m + 8) u relative.  A point with |u_p| <= 2^-18 may be
     inside the support in one precision and outside in the other; either way its term is at most u_p^2 S_p <= 2^-36 S_p."""
import functools

import numpy as np

F32, F64 = np.float32, np.float64
U = 2.0 ** -24
DEPTH = 6
H6 = 1.0 / (0.75 * 2 ** DEPTH)                                      # the cell size of a unit-extent cloud at depth 6
SOLIDS = ('cup', 'torus', 'rounded_box')
SIZES = (1500, 6000)                                               # splat radius 4 ext / sqrt(N) and 2.5 h at depth 6
NOISES = ('0', 'q')                                                # none, h / 4
SOLID_CLOUDS = tuple(f'{s}-{n}-{z}' for s in SOLIDS for n in SIZES for z in NOISES)
ADVERSARIAL = ('lattice', 'duplicates', 'clustered', 'tiny')
KS = (3, 16, 32)
KNN_CASES = [(c, k) for c in SOLID_CLOUDS + ADVERSARIAL for k in KS if not (c == 'tiny' and k > 16)]      # (k <= N = 16)
NORMAL_CASES = [(c, k) for c in SOLID_CLOUDS for k in KS]
ORIENT_CASES = [('cup-6000-0', 16, 32), ('torus-6000-0', 3, 1)]    # (cloud, k, eyes)
RECON_CASES = [(c, DEPTH) for c in SOLID_CLOUDS]
DEEP_CASE = ('torus-6000-0', 7)                                    # iso, marching cubes and the right-hand side only
EYE_RADIUS = 1.6
HPR_RADIUS = 100.0                                                 # csrc/surface_recon.hip: HPR_RADIUS


@functools.lru_cache(maxsize=None)
def cloud(name):
    """name -> (points f32 [N,3], outward normals f32 [N,3] or None).  The arrays are shared: nobody writes to them."""
    from pointdreamer_amd import synthetic
    if name in ADVERSARIAL:
        rng = np.random.default_rng(7)
        if name == 'lattice':                                      # 12^3 integers times 2^-4: exact distances, massive ties, points on planes x = const
            g = np.arange(12, dtype=F32)
            P = np.stack(np.meshgrid(g, g, g, indexing='ij'), -1).reshape(-1, 3) * F32(2.0 ** -4)
        elif name == 'duplicates':                                 # 300 points, four times each
            P = np.tile(synthetic.solid('cup').sample(300, seed=1)[0], (4, 1))[rng.permutation(1200)]
        elif name == 'clustered':                                  # two blobs of diameter 0.01 at opposite corners and a thin uniform filling
            def blob(c):
                d = rng.standard_normal((700, 3))
                return c + 0.005 * d / np.linalg.norm(d, axis=1, keepdims=True) * rng.uniform(0, 1, (700, 1)) ** (1 / 3)
            P = np.concatenate([blob(np.full(3, -0.495)), blob(np.full(3, 0.495)), rng.uniform(-0.5, 0.5, (100, 3))])[rng.permutation(1500)]
        else:
            P = rng.uniform(-0.5, 0.5, (16, 3))
        P = np.ascontiguousarray(P, F32)
        P.setflags(write=False)
        return P, None
    solid, n, z = name.split('-')
    P, _, nrm = synthetic.solid(solid).sample(int(n), seed=1, noise=0.25 * H6 if z == 'q' else 0.0)
    P.setflags(write=False)
    nrm.setflags(write=False)
    return P, nrm


# ---- the bounds
def normal_bound(lam):
    """lam [N,3] ascending -> (bound on sin(angle) [N], rows that are compared [N] bool)."""
    gap = lam[:, 1] - lam[:, 0]
    keep = gap >= 2.0 ** -20 * lam[:, 2]
    return 2.0 ** -23 + 2.0 ** -40 * lam[:, 2] / np.where(keep, gap, 1.0), keep


def sin_angle(a, b):
    """|a x b| / (|a| |b|) in float64."""
    a, b = np.asarray(a, F64), np.asarray(b, F64)
    return np.linalg.norm(np.cross(a, b), axis=1) / (np.linalg.norm(a, axis=1) * np.linalg.norm(b, axis=1))


def weight_bound(t):
    """t = the terms of oracle.spr_stages.sample_weights -> relative bound per point [N]."""
    return U * (8.0 + (24.0 * t['s2'] + (t['m'] + 4.0) * t['s3']) / t['rho'])


def rhs_bound(t):
    """t = the terms of oracle.spr_stages.rhs -> absolute bound per node [M,M,M]."""
    return U * (32.0 * t['su'] + (t['m'] + 8.0) * t['su2']) + 2.0 ** -36 * t['srim']


# ---- float32 emulations (CPU only: tests/test_spr_stages_cpu.py)
def _null_direction(A, lam):
    """The largest of the three cross products of the rows of A - lam I, normalised -> (vectors [N,3], their squared lengths before that [N])."""
    Rw = A - lam[:, None, None] * np.eye(3)
    cands = np.stack([np.cross(Rw[:, 0], Rw[:, 1]), np.cross(Rw[:, 0], Rw[:, 2]), np.cross(Rw[:, 1], Rw[:, 2])], 1)
    l = (cands ** 2).sum(2)
    v, ln = cands[np.arange(len(l)), l.argmax(1)], l.max(1)
    return v / np.sqrt(np.where(ln > 0, ln, 1.0))[:, None], ln


def closed_form_normal(P, rows, two_step=True):
    """The closed form of a symmetric 3 x 3 eigenproblem in float64 numpy, rounded to float32: what a correct float64 kernel of that form can return.
    Trigonometric eigenvalues; the eigenvector is the largest of the three cross products of the rows of A - lambda I.  two_step: where the two SMALLEST
    eigenvalues are the close pair (determinant of the normalised matrix > 0), that is done for the largest, isolated eigenvalue, and the smallest
    eigenvector comes from the 2 x 2 problem in the plane orthogonal to it -- the direct form loses (lambda_2 / gap)^2 ulp there, not lambda_2 / gap,
    because the arccos is ill-conditioned at 1 (without two_step: that direct form, which misses bound b on near-collinear neighbourhoods).  [N,3] f32."""
    X = np.asarray(P, F32)[rows].astype(F64)
    D = X - X.mean(axis=1, keepdims=True)
    A = np.einsum('nka,nkb->nab', D, D)
    a00, a01, a02, a11, a12, a22 = A[:, 0, 0], A[:, 0, 1], A[:, 0, 2], A[:, 1, 1], A[:, 1, 2], A[:, 2, 2]
    p1 = a01 * a01 + a02 * a02 + a12 * a12
    q = (a00 + a11 + a22) / 3.0
    b00, b11, b22 = a00 - q, a11 - q, a22 - q
    p2 = b00 * b00 + b11 * b11 + b22 * b22 + 2.0 * p1
    p = np.sqrt(np.where(p2 > 0, p2, 1.0) / 6.0)
    B = (A - q[:, None, None] * np.eye(3)) / p[:, None, None]
    r = np.clip(0.5 * np.linalg.det(B), -1.0, 1.0)
    phi = np.arccos(r) / 3.0
    lam = np.where(p2 > 0, q + 2.0 * p * np.cos(phi + 2.0943951023931954923), q)
    v, ln = _null_direction(A, lam)
    v = np.where((ln > 0)[:, None], v, np.array([0.0, 0.0, 1.0]))
    if two_step:
        e, le = _null_direction(A, q + 2.0 * p * np.cos(phi))       # the eigenvector of the largest eigenvalue
        first = (np.abs(e[:, 0]) > np.abs(e[:, 1]))[:, None]
        zero = np.zeros(len(e))
        u = np.where(first, np.stack([-e[:, 2], zero, e[:, 0]], 1), np.stack([zero, e[:, 2], -e[:, 1]], 1))
        u = u / np.linalg.norm(u, axis=1, keepdims=True)
        w = np.cross(e, u)
        Au, Aw = np.einsum('nab,nb->na', A, u), np.einsum('nab,nb->na', A, w)
        m00, m01, m11 = (u * Au).sum(1), (w * Au).sum(1), (w * Aw).sum(1)
        hd = 0.5 * (m00 - m11)
        h = np.sqrt(hd * hd + m01 * m01)
        c, s = np.where(hd >= 0, -m01, h - hd), np.where(hd >= 0, hd + h, -m01)
        c, s = np.where(h > 0, c, 1.0), np.where(h > 0, s, 0.0)
        t = c[:, None] * u + s[:, None] * w
        t = t / np.linalg.norm(t, axis=1, keepdims=True)
        v = np.where(((p2 > 0) & (r > 0) & (le > 0))[:, None], t, v)
    return v.astype(F32)


def rhs_f32_emulation(P, snrm, grid, R):
    """The right-hand side's expression in float32 -- u = 1 - ((dx dx + dy dy) + dz dz) / R^2 with the reciprocal rounded first, (u u) ((a_x d_x +
    a_y d_y) + a_z d_z), a float32 running sum -- over all points in the order they come (NOT the kernel's cell order): [M,M,M] float32."""
    P, A, R = np.asarray(P, F32), np.asarray(snrm, F32), F32(R)
    M = grid['M']
    i = np.arange(M, dtype=F32)
    X, Y, Z = grid['ox'] + i * grid['h'], grid['oy'] + i * grid['h'], grid['oz'] + i * grid['h']
    inv = F32(1.0) / (R * R)
    acc = np.zeros((M, M, M), F32)
    for p, a in zip(P, A):
        sel = [np.flatnonzero(np.abs(c - v) <= R * F32(1.01)) for c, v in ((X, p[0]), (Y, p[1]), (Z, p[2]))]
        if min(len(s) for s in sel) == 0:
            continue
        dx, dy, dz = (X[sel[0]] - p[0])[None, None, :], (Y[sel[1]] - p[1])[None, :, None], (Z[sel[2]] - p[2])[:, None, None]
        u = F32(1.0) - ((dx * dx + dy * dy) + dz * dz) * inv
        t = np.where(u > 0, (u * u) * ((a[0] * dx + a[1] * dy) + a[2] * dz), F32(0))
        acc[sel[2][0]:sel[2][-1] + 1, sel[1][0]:sel[1][-1] + 1, sel[0][0]:sel[0][-1] + 1] += t
    f = -acc
    f[0] = f[-1] = f[:, 0] = f[:, -1] = 0
    f[:, :, 0] = f[:, :, -1] = 0
    return f


def recon_grid(P, depth):
    """The grid, the splat radius and the cell list's (origin, cell size, cells per axis) of pdhip_surface_recon for the cloud P, from the entry's
    documented rules (include/pdhip.h; host arithmetic in float64, stored as float32)."""
    from oracle import spr_stages as st
    mn, mx, ext = st.cloud_box(P)
    Gc = 1 << depth
    h = F32(ext / (Gc - 2 * (Gc // 8)))
    o = [F32(0.5 * (mn[a] + mx[a]) - 0.5 * Gc * F64(h)) for a in range(3)]
    R = F32(max(2.5 * F64(h), 4.0 * ext / np.sqrt(F64(len(P)))))
    C = max(1, min(int(np.floor(ext / F64(R))), 128))
    return st.make_grid(h, o[0], o[1], o[2], Gc + 1), R, (mn.astype(F32), F32(ext / C * (1.0 + 1.0e-6)), C)


def cell_keys(P, origin, cs, C):
    """floor((x - o) / cs) in float32, clamped to [0, C): the key (z C + y) C + x of every point."""
    c = [np.clip(np.floor((np.asarray(P, F32)[:, a] - F32(origin[a])) / F32(cs)).astype(np.int64), 0, C - 1) for a in range(3)]
    return (c[2] * C + c[1]) * C + c[0]
