"""Taubin smoothing and the boundary vertices on the device (csrc/mesh_smooth.hip, pointdreamer_amd/mesh_smooth.py) against the numpy oracle of
tests/mesh_smooth_common.py: smoothed vertices byte for byte, masks and counts exactly."""
import functools
import os
import re

import numpy as np
import pytest
import torch

import mesh_smooth_common as msc
from mesh_components_common import bow_tie, shuffled_and_rotated

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = 'cuda'
T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def smooth(v, f, **kw):
    """taubin_smooth with counts, as numpy; called twice, the two results must have equal bytes and the inputs must stay as they were."""
    from pointdreamer_amd import mesh_smooth as M
    tv, tf = T(v), T(f)
    runs = [M.taubin_smooth(tv, tf, return_counts=True, **{k: (T(a) if isinstance(a, np.ndarray) else a) for k, a in kw.items()}) for _ in range(2)]
    a, b = (r[0].cpu().numpy() for r in runs)
    assert a.dtype == np.float32 and a.shape == v.shape and a.tobytes() == b.tobytes() and runs[0][1] == runs[1][1]
    assert tv.cpu().numpy().tobytes() == np.ascontiguousarray(v).tobytes() and np.array_equal(tf.cpu().numpy(), f)
    return a, runs[0][1]


def check(v, f, **kw):
    got, cnt = smooth(v, f, **kw)
    want, wcnt = msc.oracle_smooth(v, f, return_counts=True, **kw)
    assert got.tobytes() == want.tobytes(), f'{(got != want).any(1).sum()} of {len(v)} vertices differ, by at most {np.abs(got - want).max()}'
    assert cnt == wcnt
    return got, cnt


# ---- 1, 2: the smallest cases and the longest rows
def test_a_tetrahedron_by_hand():
    got, cnt = check(msc.TET_V, msc.TET, steps=1, lam=0.5, mu=0.0)
    s = 1 / 6
    assert np.array_equal(got, np.array([[s, s, s], [0.5, s, s], [s, 0.5, s], [s, s, 0.5]]).astype(np.float32))
    assert cnt == dict(moved=4, held=0, isolated=0, steps=1)
    check(msc.TET_V, msc.TET, steps=1)
    from pointdreamer_amd import mesh_smooth as M
    lap = M.laplacian_smooth(T(msc.TET_V), T(msc.TET))
    assert lap.cpu().numpy().tobytes() == got.tobytes()


def test_rows_longer_than_a_wave_and_than_a_workgroup():
    v, f = msc.bipyramid(300)
    rowptr, _ = msc.csr(len(v), f)
    assert sorted(set(np.diff(rowptr).tolist())) == [4, 300]
    check(v, f, steps=2)
    check(v, f, steps=3, lam=0.33, mu=0.0)


# ---- 3: the noisy sphere
@pytest.mark.parametrize('pair', [msc.MESHLAB, msc.TAUBIN, (0.5, 0.0)])
def test_noisy_sphere_ten_steps(pair):
    v, f = msc.noisy_sphere()
    got, cnt = check(v, f, steps=10, lam=pair[0], mu=pair[1])
    assert cnt == dict(moved=len(v), held=0, isolated=0, steps=10) and (got != v).any(1).all()


# ---- 4: sizes round a workgroup, an unreferenced vertex
@pytest.mark.parametrize('n', [16, 32])
def test_torus_grid_with_an_unreferenced_vertex(n):
    v, f = msc.torus_with_spare(n)
    assert len(v) == n * n + 1
    got, cnt = check(v, f, steps=4)
    assert got[-1].tobytes() == v[-1].tobytes() and cnt['isolated'] == 1 and cnt['moved'] == n * n
    check(v, f, steps=1, lam=0.5, mu=0.0)                          # one launch: f32 in, f32 out
    check(v, f, steps=1)                                           # two launches: no pass between two states


# ---- 5: what the result depends on
def test_face_order_does_not_matter_and_vertex_labels_follow_the_oracle():
    v, f = msc.noisy_sphere()
    a, _ = check(v, f, steps=5)
    b, _ = smooth(v, shuffled_and_rotated(f), steps=5)
    assert a.tobytes() == b.tobytes()
    perm = np.random.default_rng(4).permutation(len(v))
    pv, pf = msc.relabel(v, f, perm)
    c, _ = check(pv, pf, steps=5)
    assert np.abs(c[perm] - a).max() < 1e-6                        # the same surface (other sum orders: not the same bytes)


# ---- 6: open and non-manifold meshes
def boundary(f, n):
    from pointdreamer_amd import mesh_smooth as M
    runs = [M.boundary_vertices(T(f), n, return_counts=True) for _ in range(2)]
    assert runs[0][0].dtype == torch.bool and torch.equal(runs[0][0], runs[1][0]) and runs[0][1] == runs[1][1]
    assert torch.equal(M.boundary_vertices(T(f), n), runs[0][0])
    return runs[0][0].cpu().numpy(), runs[0][1]


def test_sphere_cap_boundary_fixed_free_and_a_user_mask():
    v, f = msc.sphere_cap()
    mask, cnt = boundary(f, len(v))
    omask, ocnt = msc.oracle_boundary(f, len(v))
    assert np.array_equal(mask, omask) and cnt == ocnt and cnt['boundary_vertices'] == cnt['boundary_edges'] > 20
    fixed, c1 = check(v, f, steps=10)
    assert fixed[omask].tobytes() == v[omask].tobytes() and c1['held'] == ocnt['boundary_vertices'] and c1['isolated'] > 0
    free, c2 = check(v, f, steps=10, boundary='free')
    assert c2['held'] == 0 and (free[omask] != v[omask]).any(1).all()
    user = np.zeros(len(v), np.uint8)
    inner = np.flatnonzero(~omask & (np.diff(msc.csr(len(v), f)[0]) > 0))[::7]
    user[inner] = 1
    both, c3 = check(v, f, steps=10, fixed=user)
    assert both[inner].tobytes() == v[inner].tobytes() and both[omask].tobytes() == v[omask].tobytes()
    assert c3['held'] == ocnt['boundary_vertices'] + len(inner)
    only, c4 = check(v, f, steps=10, boundary='free', fixed=user.astype(bool))
    assert only[inner].tobytes() == v[inner].tobytes() and c4['held'] == len(inner)


def test_three_triangles_on_one_edge_and_the_bow_tie():
    v, f = msc.fan()
    mask, cnt = boundary(f, len(v))
    assert mask.all() and cnt == msc.oracle_boundary(f, len(v))[1] == dict(boundary_vertices=5, boundary_edges=6, nonmanifold_edges=1)
    got, c = check(v, f, steps=2)
    assert got.tobytes() == v.tobytes() and c['held'] == 5
    check(v, f, steps=2, boundary='free')
    v, f = bow_tie()
    mask, cnt = boundary(f, len(v))
    assert not mask.any() and cnt == dict(boundary_vertices=0, boundary_edges=0, nonmanifold_edges=0)
    check(v, f, steps=3)
    mask, cnt = boundary(msc.TET[:3], 4)
    assert mask.tolist() == [True, False, True, True] and cnt == dict(boundary_vertices=3, boundary_edges=3, nonmanifold_edges=0)


# ---- 7, 8: the C entries on buffers of the test's own
def _raw(v, f, fill, steps=3, lam=0.5, mu=-0.53, spoil=None):
    """Both entries on buffers pre-filled with the byte `fill`: (rc, message, out, state, pair_faces, boundary, counts of both) as numpy."""
    from pointdreamer_amd import _lib, mesh_utils
    from pointdreamer_amd._lib import ptr, stream
    L = _lib.lib()
    tv, tf = T(v), T(f)
    Vn = len(v)
    rowptr, colidx = mesh_utils.neighbour_csr(Vn, tf)
    rowptr, colidx = rowptr.clone(), colidx.clone()
    nbytes = lambda n, dt: (n * torch.empty((), dtype=dt).element_size(),)
    mk = lambda n, dt: torch.full(nbytes(n, dt), fill, dtype=torch.uint8, device=DEV).view(dt)
    pair, bnd, bc = mk(colidx.shape[0], torch.int32), mk(Vn, torch.uint8), mk(4, torch.int32)
    rc_b = L.pdhip_mesh_boundary_vertices(ptr(tf), len(f), Vn, ptr(rowptr), ptr(colidx), ptr(pair), ptr(bnd), ptr(bc), stream())
    assert rc_b == 0, L.pdhip_last_error()
    if spoil is not None:
        spoil(tv, rowptr, colidx)
    sa, sb, out, sc = mk(4 * Vn, torch.float64), mk(4 * Vn, torch.float64), mk(3 * Vn, torch.float32), mk(4, torch.int32)
    rc = L.pdhip_smooth_mesh(ptr(tv), Vn, ptr(rowptr), ptr(colidx), ptr(bnd), steps, lam, mu, ptr(sa), ptr(sb), ptr(out), ptr(sc), stream())
    msg = L.pdhip_last_error().decode() if rc else ''
    n = lambda t: t.cpu().numpy()
    return rc, msg, n(out.view(torch.uint8)), n(torch.cat([sa, sb]).view(torch.uint8)), n(pair), n(bnd), n(bc), n(sc)


def test_dirty_buffers_give_the_same_bytes_as_clean_ones():
    v, f = msc.sphere_cap()
    clean, dirty = _raw(v, f, 0), _raw(v, f, 0xFF)
    assert clean[0] == dirty[0] == 0
    for a, b, name in zip(clean[2:], dirty[2:], ('out', 'state', 'pair_faces', 'boundary', 'boundary counts', 'counts')):
        if name != 'state':                                        # (scratch: its rows' padding word aside it is equal too, but it means nothing)
            assert a.tobytes() == b.tobytes(), name
    want, wcnt = msc.oracle_smooth(v, f, steps=3, return_counts=True)
    assert dirty[2].tobytes() == want.tobytes()
    assert dirty[7].tolist() == [wcnt['moved'], wcnt['held'], wcnt['isolated'], 0]
    omask, ocnt = msc.oracle_boundary(f, len(v))
    assert np.array_equal(dirty[5].astype(bool), omask) and dirty[6].tolist() == [ocnt['boundary_vertices'], ocnt['boundary_edges'], 0, 0]
    assert set(dirty[4].tolist()) == {1, 2} and (dirty[4] == 1).sum() == 2 * ocnt['boundary_edges']


def _nan_vertex(tv, rowptr, colidx):
    tv[int(colidx[5]), 1] = float('nan')


def _inf_vertex(tv, rowptr, colidx):
    tv[int(colidx[0]), 2] = float('inf')


def _col_high(tv, rowptr, colidx):
    colidx[colidx.shape[0] // 2] = tv.shape[0]


def _col_negative(tv, rowptr, colidx):
    colidx[3] = -1


def _row_back(tv, rowptr, colidx):
    rowptr[rowptr.shape[0] // 2] = 0


def _row_start(tv, rowptr, colidx):
    rowptr[0] = 1


def _row_end(tv, rowptr, colidx):
    rowptr[-1] -= 1


@pytest.mark.parametrize('spoil,word', [(_nan_vertex, 'not finite'), (_inf_vertex, 'not finite'), (_col_high, 'colidx'), (_col_negative, 'colidx'),
                                        (_row_back, 'rowptr'), (_row_start, 'rowptr'), (_row_end, 'rowptr')])
def test_refusals_from_the_device_leave_every_output_untouched(spoil, word):
    v, f = msc.torus_with_spare(16)
    rc, msg, out, state, *_ = _raw(v, f, 0xA5, spoil=spoil)
    assert rc == -1 and 'pdhip_smooth_mesh' in msg and word in msg and 'nothing was written' in msg, msg
    assert (out == 0xA5).all() and (state == 0xA5).all()


def test_a_non_finite_vertex_no_face_names_is_copied():
    from pointdreamer_amd import mesh_smooth as M
    v, f = msc.torus_with_spare(16)
    v[-1] = [np.nan, np.inf, -np.inf]
    got = M.taubin_smooth(T(v), T(f), steps=2).cpu().numpy()
    assert got[-1].tobytes() == v[-1].tobytes() and got[:-1].tobytes() == msc.oracle_smooth(v, f, steps=2)[:-1].tobytes()


def test_boundary_entry_refuses_a_csr_of_other_faces():
    from pointdreamer_amd import _lib, mesh_utils
    from pointdreamer_amd._lib import ptr, stream
    L = _lib.lib()
    v, f = msc.noisy_sphere()
    rowptr, colidx = mesh_utils.neighbour_csr(len(v), T(f))
    other = T(np.ascontiguousarray(f[:, [0, 1, 1]] * 0 + np.array([0, 1, len(v) - 1])))       # the pair (0, Vn - 1) is in no row
    pair = torch.zeros_like(colidx)
    bnd = torch.full((len(v),), 0xA5, dtype=torch.uint8, device=DEV)
    cnt = torch.zeros((4,), dtype=torch.int32, device=DEV)
    assert L.pdhip_mesh_boundary_vertices(ptr(other), len(f), len(v), ptr(rowptr), ptr(colidx), ptr(pair), ptr(bnd), ptr(cnt), stream()) == -1
    assert b'pdhip_mesh_boundary_vertices' in L.pdhip_last_error() and b'not in its row' in L.pdhip_last_error()
    assert (bnd == 0xA5).all()
    bad = T(np.array([[0, 1, len(v)]], np.int64))
    assert L.pdhip_mesh_boundary_vertices(ptr(bad), 1, len(v), ptr(rowptr), ptr(colidx), ptr(pair), ptr(bnd), ptr(cnt), stream()) == -1
    assert b'rowptr' in L.pdhip_last_error()                       # (rowptr[Vn] > 6 F: the CSR of 5120 faces against one face)


# ---- 9: behind the reconstruction
@functools.lru_cache(maxsize=None)
def torus_cloud():
    from pointdreamer_amd import synthetic
    xyz, rgb, _ = synthetic.solid('torus').sample(25000, seed=1, noise=0.005)
    return T(xyz), T(rgb)


def test_smoothing_behind_the_reconstruction():
    from pointdreamer_amd import mesh_checks as mc, spr
    xyz, rgb = torus_cloud()
    pv, pf, pc, prc = spr.recon_one_shape_SPR(xyz, rgb, depth=6, return_counts=True)
    none = spr.recon_one_shape_SPR(xyz, rgb, depth=6, smooth=None)
    assert all(a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes() for a, b in zip(none, (pv, pf, pc)))
    assert 'smooth_steps' not in prc and 'smooth_moved' not in prc
    sv, sf, sc, src = spr.recon_one_shape_SPR(xyz, rgb, depth=6, return_counts=True, smooth=10)
    v, f = pv.cpu().numpy(), pf.cpu().numpy()
    want, wcnt = msc.oracle_smooth(v, f, steps=10, return_counts=True)
    assert sv.cpu().numpy().tobytes() == want.tobytes() and sv.cpu().numpy().tobytes() != v.tobytes()
    assert sf.cpu().numpy().tobytes() == f.tobytes() and sc.cpu().numpy().tobytes() == pc.cpu().numpy().tobytes()
    assert src['smooth_steps'] == 10 and src['smooth_moved'] == wcnt['moved'] and src['faces'] == prc['faces'] == len(f)
    assert mc.directed_edge_defects(f) == 0
    assert [c[3] for c in mc.components_euler(len(v), sf.cpu().numpy())] == [c[3] for c in mc.components_euler(len(v), f)]
    dv, df, dcol = spr.recon_one_shape_SPR(xyz, rgb, depth=6, smooth=dict(steps=3, lam=0.33, mu=-0.34))
    assert dv.cpu().numpy().tobytes() == msc.oracle_smooth(v, f, steps=3, lam=0.33, mu=-0.34).tobytes()
    tv, tf, _, trc = spr.recon_one_shape_SPR(xyz, rgb, depth=6, return_counts=True, smooth=10, target_faces=4000)
    assert trc['smooth_steps'] == 10 and trc['faces_reconstructed'] == len(f) and trc['faces'] == len(tf) <= 4001
    assert mc.directed_edge_defects(tf.cpu().numpy()) == 0
    assert [c[3] for c in mc.components_euler(len(tv), tf.cpu().numpy())] == [c[3] for c in mc.components_euler(len(v), f)]


# ---- 10: the demo key
def test_demo_key_smooths_the_cached_geometry(tmp_path, caplog):
    import logging
    from pointdreamer_amd import demo, io_utils, synthetic
    xyz, rgb, _ = synthetic.solid('two_spheres').sample(16000, seed=5)
    pc = str(tmp_path / 'two.ply')
    io_utils.save_colored_pc_ply(xyz * 1.7 + 0.3, rgb, pc)
    base = ["--config", os.path.join(ROOT, "configs", "nearest.yaml"), "--pc_file", pc, "--set", "geo_from=SPR", "xatlas_texture_res=256", "cam_res=128",
            "res=64", "point_validation_by_o3d=False"]

    def geometry(out):
        return io_utils.load_obj_mesh(os.path.join(out, 'geo', f'{os.path.basename(out)}_untextured', 'models', 'model_normalized.obj'))

    with caplog.at_level(logging.INFO, logger='pointdreamer_amd'):
        out = demo.main(base + [f"output_path={tmp_path / 'smooth'}", "spr_smooth=5"])[0]
    v1, f1 = geometry(out)
    line = re.search(r'SPR smoothing: 5 Taubin steps \(lambda 0\.5, mu -0\.53\): (\d+) vertices moved', caplog.text)
    assert line and 0.9 * len(v1) < int(line.group(1)) <= len(v1)
    caplog.clear()
    with caplog.at_level(logging.INFO, logger='pointdreamer_amd'):
        out = demo.main(base + [f"output_path={tmp_path / 'plain'}"])[0]
    v2, f2 = geometry(out)
    assert 'SPR smoothing' not in caplog.text
    assert len(f1) == len(f2) and np.array_equal(f1, f2) and v1.shape == v2.shape and (v1 != v2).any(1).mean() > 0.9
