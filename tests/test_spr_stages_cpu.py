"""oracle/spr_stages.py without a GPU: every function that tests/test_gpu_spr_stages.py compares the device with is held to an analytic case here,
the float32 emulations of tests/spr_stages_common.py lie inside the bounds of checks b and e (so the bounds have room for float32 rounding), and
the three test hooks of csrc/surface_recon.hip report the offsets the carve log reports and refuse bad arguments before any device work."""
import ctypes as C
import os

import numpy as np
import pytest

import spr_stages_common as sc
import workspace_common as wc
from conftest import ROOT
from oracle import spr_stages as st

F32, F64 = np.float32, np.float64
LIB = os.path.join(ROOT, 'pointdreamer_amd', 'libpdhip.so')
needs_lib = pytest.mark.skipif(not os.path.exists(LIB), reason="libpdhip.so not built")


def brute_rows(P, k):
    """Indices of the k nearest points of every point (float32 distances, ties to the smaller index): [N,k]."""
    d = st.d2_f32(P[None, :, :], P[:, None, :])
    return np.argsort(d, axis=1, kind='stable')[:, :k]


def test_knn_rows_are_the_sorted_smallest_distances():
    P = sc.cloud('tiny')[0]
    d = st.d2_f32(P[None, :, :], P[:, None, :])
    for k in (3, 16):
        rows = st.knn_rows(P, k, chunk=5)
        assert rows.dtype == F32 and np.array_equal(rows, np.sort(d, axis=1)[:, :k]) and np.all(rows[:, 0] == 0)
        assert np.array_equal(np.sort(st.row_distances(P, brute_rows(P, k)), axis=1), rows)
    L = sc.cloud('lattice')[0]
    rows = st.knn_rows(L, 7)
    inner = np.all((L > 0) & (L < 11 / 16), axis=1)
    assert np.all(rows[inner] == np.array([0] + [2.0 ** -8] * 6, F32))          # the point and its six lattice neighbours, exactly


def test_marching_cubes_of_a_sphere_field_is_a_closed_oriented_sphere():
    """chi = r0 - |x| on a 33^3 grid, iso 0.  The surface error of a chord of length <= sqrt(3) h on a sphere of radius r0 is 3 h^2 / (8 r0), and
    the linear interpolation of |x| along an edge is off by at most h^2 / (8 r0): the volume differs by at most area * h^2 / (2 r0) = 2 pi r0 h^2."""
    from pointdreamer_amd import mesh_checks as mc
    M, h, r0 = 33, 1.0 / 32, 0.35
    grid = st.make_grid(h, -0.5, -0.5, -0.5, M)
    X = st.node_coords(grid)
    chi = (r0 - np.sqrt(X[2][:, None, None] ** 2 + X[1][None, :, None] ** 2 + X[0][None, None, :] ** 2)).astype(F32)
    fl, v, f = st.marching_cubes(chi, 0.0, grid)
    assert v.dtype == F32 and f.dtype == np.int64 and fl.dtype == np.uint8 and len(v) == int(np.unpackbits(fl).sum())
    assert mc.directed_edge_defects(f) == 0
    assert [c[3] for c in mc.components_euler(len(v), f)] == [2]
    assert np.abs(np.linalg.norm(v.astype(F64), axis=1) - r0).max() <= h * h / (8 * r0) + 1e-6
    vol = mc.signed_volume(v.astype(F64), f)
    assert vol > 0 and abs(vol - 4 / 3 * np.pi * r0 ** 3) <= 2 * np.pi * r0 * h * h
    # a vertex never sits on a node: a field that equals the iso value's neighbour exactly is clamped to 1 / 1024 of the edge
    chi2 = np.full((5, 5, 5), -1.0, F32)
    chi2[2, 2, 2] = 1.0e6
    g2 = st.make_grid(1.0, 0.0, 0.0, 0.0, 5)
    fl2, v2, f2 = st.marching_cubes(chi2, 0.0, g2)
    assert len(v2) == 6 and len(f2) == 8 and mc.directed_edge_defects(f2) == 0
    assert sorted(np.abs(v2 - 2.0).max(1).tolist()) == [F32(1 - 1 / 1024)] * 6


def test_cg_f32_agrees_with_a_float64_solve():
    """Both reach the tolerance on the same system; the float32 recurrence's true residual stays within 1e-5 of the one it reports, and it needs
    about as many iterations."""
    rng = np.random.default_rng(3)
    f = np.zeros((33, 33, 33), F32)
    f[8:25, 8:25, 8:25] = rng.standard_normal((17, 17, 17)).astype(F32)
    x32, it32, res, true = st.cg_f32(f, 1.0e-4)
    x64, it64 = st.cg_f64(f, 1.0e-4)
    print(f"cg_f32 {it32} iterations, residual {res:.3e} true {true:.3e}; float64 {it64} iterations, true {st.true_residual(f, x64):.3e}")
    assert res <= 1.0e-4 and abs(true - float(res)) <= 1.0e-5 and st.true_residual(f, x64) <= 1.0e-4 * (1 + 1e-9)
    assert abs(it32 - it64) <= max(2, it64 // 10)
    assert np.all(x32[0] == 0) and np.all(x32[:, :, -1] == 0)
    # |A (x32 - x64)| <= the two residuals, and A's smallest eigenvalue on 31^3 unknowns is 12 sin^2(pi / 64): the solutions agree accordingly
    lam_min = 12.0 * np.sin(np.pi / 64) ** 2
    err = np.linalg.norm(x32.astype(F64) - x64) / np.linalg.norm(f.astype(F64))
    assert err <= (true + 1.0e-4) / lam_min
    lap = st.laplacian(np.arange(27, dtype=F64).reshape(3, 3, 3))
    assert lap[1, 1, 1] == 6 * 13 - (12 + 14 + 10 + 16 + 4 + 22) and np.count_nonzero(lap) == 0      # (the middle of a linear ramp: zero)


def test_orient_restores_analytic_normals_of_random_sign():
    """A sphere seen by two eyes on one side: rule 1 decides the half they see, rules 2 and 3 carry the sign round the back."""
    rng = np.random.default_rng(5)
    P = rng.standard_normal((2000, 3))
    P = (0.5 * P / np.linalg.norm(P, axis=1, keepdims=True)).astype(F32)
    out = (P.astype(F64) / np.linalg.norm(P.astype(F64), axis=1, keepdims=True)).astype(F32)
    n = out * rng.choice([-1.0, 1.0], (2000, 1)).astype(F32)
    knn = brute_rows(P, 8)
    eyes = st.fibonacci_eyes(P, 8, 1.6)[:2]
    assert np.allclose(np.linalg.norm(eyes - 0.5 * (P.min(0) + P.max(0)).astype(F64), axis=1), 1.6 * (P.max(0) - P.min(0)).max())
    vis = np.stack([((e - P.astype(F64)) * out).sum(1) > 0.3 for e in eyes])
    got, state, counts = st.orient(P, n, knn, eyes, vis)
    print("counts", counts)
    assert sum(counts) == 2000 and counts[0] == int(vis.any(0).sum()) and counts[1] > 0 and counts[3] == 0
    assert np.array_equal(got.view(np.uint32), out.view(np.uint32))
    again, _, c2 = st.orient(P, got, knn, eyes, vis)               # the rules do not depend on the signs they are given
    assert np.array_equal(again.view(np.uint32), got.view(np.uint32)) and c2 == counts
    # one round per ring: with a single round the back stays for rule 3 or stays undecided
    _, s1, c1 = st.orient(P, n, knn, eyes, vis, rounds=1)
    assert c1[1] < counts[1] and c1[2] + c1[3] > 0 and sum(c1) == 2000


@pytest.mark.parametrize("name,k", [('cup-1500-0', 3), ('cup-1500-0', 16), ('torus-6000-q', 32), ('cup-6000-0', 3), ('rounded_box-6000-0', 3)])
def test_a_float64_closed_form_rounded_to_float32_lies_inside_bound_b(name, k):
    """The form the kernel uses (smallest_eigvec: direct where the smallest eigenvalue is isolated, through the largest eigenvector and a 2 x 2 problem
    where the two smallest are the close pair).  The direct form alone misses the bound about tenfold on the near-collinear triples of the two
    noise-free 6 000-point clouds, which is how the kernel came to its second branch: the check can fail."""
    P = sc.cloud(name)[0]
    rows = np.concatenate([np.argsort(st.d2_f32(P[None, :, :], P[a:a + 500, None, :]), axis=1, kind='stable')[:, :k]
                           for a in range(0, len(P), 500)])        # (brute force, 500 rows at a time)
    ref, lam = st.normal_direction(P, rows)
    bound, keep = sc.normal_bound(lam)
    emu = sc.closed_form_normal(P, rows)
    ratio = (sc.sin_angle(emu, ref) / bound)[keep]
    print(f"{name} k={k}: worst ratio {ratio.max():.3f}, rows left out {int((~keep).sum())} of {len(P)}")
    assert ratio.max() <= 1.0 and (~keep).sum() <= 0.005 * len(P)
    assert np.abs(np.linalg.norm(emu.astype(F64), axis=1) - 1.0).max() <= 2.0 ** -22
    # the bound has no room for a wrong direction: the second eigenvector misses it by orders of magnitude
    assert bound[keep].max() < 1.0e-2
    if len(P) == 6000 and k == 3:
        direct = (sc.sin_angle(sc.closed_form_normal(P, rows, two_step=False), ref) / bound)[keep]
        print(f"{name} k={k}: the direct form alone: worst ratio {direct.max():.2f}")
        assert direct.max() > 5.0


@pytest.mark.parametrize("name", ['cup-1500-0', 'torus-6000-q'])
def test_a_float32_evaluation_in_another_order_lies_inside_bounds_d_and_e(name):
    P, nrm = sc.cloud(name)
    grid, R, _ = sc.recon_grid(P, sc.DEPTH)
    w, tw = st.sample_weights(P, nrm, R, terms=True)
    assert tw['m'].min() >= 1 and tw['rho'].min() >= 1.0           # every point counts itself
    snrm = w.astype(F32)
    ref, t = st.rhs(P, snrm, grid, R, terms=True)
    B = sc.rhs_bound(t)
    emu = sc.rhs_f32_emulation(P, snrm, grid, R).astype(F64)
    err = np.abs(emu - ref)
    ratio = (err[B > 0] / B[B > 0]).max()
    print(f"{name}: R / h = {float(R) / float(grid['h']):.3f}, worst |f32 - f64| / bound {ratio:.3f}, max bound / max |f| {B.max() / np.abs(ref).max():.2e}")
    assert np.all(err <= B) and np.all(emu[B == 0] == 0)
    assert B.max() <= 1.0e-5 * np.abs(ref).max()
    assert np.all(ref[0] == 0) and np.all(ref[:, -1] == 0) and np.all(ref[:, :, 0] == 0)
    # scatter against a direct gather at a few nodes
    X = st.node_coords(grid)
    rng = np.random.default_rng(1)
    hot = np.argwhere(t['m'] > 0)
    for k, j, i in hot[rng.integers(0, len(hot), 20)]:
        d = np.array([X[0][i], X[1][j], X[2][k]]) - P.astype(F64)
        u = 1.0 - (d * d).sum(1) / F64(R) ** 2
        want = -(np.where(u > 0, u * u * (snrm.astype(F64) * d).sum(1), 0.0)).sum()
        assert abs(ref[k, j, i] - want) <= 1e-12 * max(1.0, abs(want)) and int((u > 0).sum()) == t['m'][k, j, i]
    # the sample weights in float32, all pairs in the order they come
    P32 = P.astype(F32)
    inv = F32(1.0) / (R * R)
    rho = np.array([np.cumsum(np.where((u := F32(1.0) - st.d2_f32(P32, q) * inv) > 0, (u * u) * u, F32(0)), dtype=F32)[-1] for q in P32[:300]])
    l = np.sqrt((nrm[:300, 0] * nrm[:300, 0] + nrm[:300, 1] * nrm[:300, 1]) + nrm[:300, 2] * nrm[:300, 2])
    emu_w = nrm[:300] * (F32(1.0) / (l * rho))[:, None]
    assert np.all(np.abs(emu_w.astype(F64) - w[:300]) <= sc.weight_bound(tw)[:300, None] * np.abs(w[:300]))


def test_iso_value_of_a_linear_field_is_the_field_at_the_centroid():
    grid = st.make_grid(0.125, -1.0, -1.0, -1.0, 17)
    X = st.node_coords(grid)
    chi = (0.5 * X[0][None, None, :] - 0.25 * X[1][None, :, None] + 2.0 * X[2][:, None, None] + 1.0).astype(F32)
    P = np.random.default_rng(2).uniform(-0.9, 0.9, (500, 3)).astype(F32)
    want = (0.5 * P[:, 0].astype(F64) - 0.25 * P[:, 1] + 2.0 * P[:, 2] + 1.0)
    assert np.abs(st.trilinear_f32(chi, grid, P) - want).max() <= 16 * 2.0 ** -24 * 4.0
    assert abs(st.iso_value(chi, grid, P) - want.mean()) <= 16 * 2.0 ** -24 * 4.0
    outside = np.array([[-5, 0, 0], [5, 5, 5]], F32)                # clamped into the grid
    assert np.allclose(st.trilinear_f32(chi, grid, outside), [0.5 * -1 + 1.0, 0.5 - 0.25 + 2.0 + 1.0])


# ---- the hooks
def _layout(L, which, args):
    n = 6 if which == 'pdhip_debug_estimate_normals_layout' else 8
    off = (C.c_uint64 * n)()
    assert getattr(L, which)(*args, off) == 0, L.pdhip_last_error()
    return [int(v) for v in off]


@needs_lib
@pytest.mark.parametrize("query,hook", [('pdhip_estimate_normals_ws_bytes', 'pdhip_debug_estimate_normals_layout'),
                                        ('pdhip_surface_recon_ws_bytes', 'pdhip_debug_surface_recon_layout')])
def test_layout_hooks_report_offsets_of_the_carve_log(query, hook):
    from pointdreamer_amd import _lib
    L = _lib.lib()
    for args in wc.SHAPES[query].values():
        with wc.CarveLog(L) as log:
            size = getattr(L, query)(*args)
            carved, triples = log.read()
        outer = [(int(o), int(b)) for base, o, b in triples[wc.carves(triples)[-1][0]]]      # the Carve on the workspace itself: (offset, bytes)
        off = _layout(L, hook, args)
        assert off[-1] == size > 0
        regions = dict(outer)
        assert all(o in regions and o % 256 == 0 for o in off[:-1]), (off, outer)
        assert len(set(off)) == len(off)
        N = args[0]
        if hook == 'pdhip_debug_estimate_normals_layout':
            k, V = args[1], args[2]
            assert [regions[o] for o in off[:-1]] == [8 * 128 ** 3, 16 * N, 4 * N * k, 24 * V, V * N]
        else:
            n3 = (2 ** args[1] + 1) ** 3
            assert [regions[o] for o in off[:-1]] == [8 * 128 ** 3, 16 * N, 16 * N, 4 * n3, n3, 256, 4 * n3]
        assert L.pdhip_debug_carve_log_read(None, 0) == 0          # (the log is off again and was cleared)


@needs_lib
def test_the_three_hooks_validate_their_arguments_before_any_device_work():
    from pointdreamer_amd import _lib
    L = _lib.lib()
    err = lambda: L.pdhip_last_error().decode()
    off = (C.c_uint64 * 8)()
    null = C.c_void_p(0)
    for args in ((5003, 16, 32, null), (15, 16, 32, off), (5003, 2, 32, off), (5003, 33, 32, off), (5003, 16, 0, off), (5003, 16, 65, off), (20, 24, 1, off)):
        assert L.pdhip_debug_estimate_normals_layout(*args) == -1 and 'pdhip_debug_estimate_normals_layout' in err(), args
    for args in ((5003, 6, null), (15, 6, off), (5003, 5, off), (5003, 9, off)):
        assert L.pdhip_debug_surface_recon_layout(*args) == -1 and 'pdhip_debug_surface_recon_layout' in err(), args
    buf = (C.c_char * 64)()
    p = C.cast(buf, C.c_void_p)
    ok = dict(points=p, normals=p, N=100, depth=6, f_out=p, info=p, ws=p)
    for k, bad in (('points', null), ('normals', null), ('f_out', null), ('info', null), ('ws', null), ('N', 15), ('N', -1), ('N', (1 << 24) + 1),
                   ('depth', 5), ('depth', 9)):
        a = dict(ok)
        a[k] = bad
        assert L.pdhip_debug_surface_recon_rhs(*a.values(), null) == -1 and 'pdhip_debug_surface_recon_rhs' in err(), (k, bad)
