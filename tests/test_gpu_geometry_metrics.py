"""Geometry scores on the device (csrc/cloud_metrics.hip, pointdreamer_amd/geometry_metrics.py, run_geometry_evaluation.py).
pdhip_nearest_points is held to BIT EQUALITY with the brute-force float64 oracle of tests/geometry_metrics_common.py (d2 as uint64,
idx exactly): a minimum, and the smallest index that attains it, do not depend on the scan order.  pdhip_cloud_metrics: the counts
exactly, the f64 sums within Q 2^-53 relative of the exactly rounded sum (Q non-negative terms, each added once).  The scores
against the values of the reference (tests/golden/geometry_metrics_ref.npz) within the bounds of tests/test_geometry_metrics_cpu.py."""
import os

import numpy as np
import pytest
import torch

from conftest import load_golden
import geometry_metrics_common as gm

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
SENT_D2, SENT_IDX, SENT_CNT = -7.0, -77, -777
# pdhip_debug_set_nearest_path: 0 = the shipped ring scan for every query, 1 = the LDS phase first (the ring scan for what it cannot certify)
RING, STAGED = 0, 1
BOTH = pytest.mark.parametrize("path", [RING, STAGED], ids=["ring", "staged"])


def T(a):
    return torch.from_numpy(np.array(a)).to(DEV)                  # (a writable copy: the cached clouds are read-only)


def run_nearest(q, t, same_buffer=False, path=RING, ws=None):
    """(rc, d2, idx, counts) of pdhip_nearest_points; the outputs start as sentinels.  ws: the workspace to use instead of a fresh one."""
    from pointdreamer_amd import _lib
    from pointdreamer_amd._lib import ptr, stream
    L = _lib.lib()
    tq = T(np.asarray(q, np.float32))
    tt = tq if same_buffer else T(np.asarray(t, np.float32))
    Q, M = tq.shape[0], tt.shape[0]
    d2 = torch.full((max(Q, 1),), SENT_D2, dtype=torch.float64, device=DEV)
    idx = torch.full((max(Q, 1),), SENT_IDX, dtype=torch.int32, device=DEV)
    counts = torch.full((4,), SENT_CNT, dtype=torch.int32, device=DEV)
    if ws is None:
        ws = torch.empty((L.pdhip_nearest_points_workspace_bytes(Q, M),), dtype=torch.uint8, device=DEV)
    old = L.pdhip_debug_set_nearest_path(path)
    try:
        rc = L.pdhip_nearest_points(ptr(tq), Q, ptr(tt), M, ptr(d2), ptr(idx), ptr(counts), ptr(ws), stream())
    finally:
        L.pdhip_debug_set_nearest_path(old)
    torch.cuda.synchronize()
    assert old == RING
    return rc, d2.cpu().numpy()[:Q], idx.cpu().numpy()[:Q], counts.cpu().numpy()


def check_against_oracle(q, t, oracle=None, same_buffer=False, path=RING):
    rc, d2, idx, counts = run_nearest(q, t, same_buffer, path)
    assert rc == 0
    od2, oidx = oracle if oracle is not None else gm.oracle_nearest(q, t)
    print('Q', len(q), 'M', len(t), 'counts', counts.tolist(), 'd2 unequal', int((d2.view(np.uint64) != od2.view(np.uint64)).sum()),
          'idx unequal', int((idx != oidx).sum()))
    assert np.array_equal(d2.view(np.uint64), od2.view(np.uint64))
    assert np.array_equal(idx, oidx)
    assert counts[0] + counts[1] == len(q) and counts[0] >= 0 and counts[1] >= 0 and 1 <= counts[2] <= 128 and counts[3] == 0
    assert path == STAGED or counts[0] == 0
    return counts


# ---- bit equality
@BOTH
def test_two_solids_equal_the_oracle_bit_for_bit(path):
    q, t = gm.main_pair()
    counts = check_against_oracle(q, t, gm.oracle_main(), path=path)
    assert path == RING or counts[0] > 0                          # the LDS phase certified something


@BOTH
def test_two_solids_with_the_roles_swapped(path):
    q, t = gm.main_pair()
    check_against_oracle(t, q, gm.oracle_main(swapped=True), path=path)


@BOTH
def test_a_cloud_against_itself_from_one_buffer(path):
    q, _ = gm.main_pair()
    rc, d2, idx, _ = run_nearest(q, None, same_buffer=True, path=path)
    od2, oidx = gm.oracle_nearest(q, q)
    assert rc == 0 and np.all(d2 == 0.0)
    assert np.array_equal(d2.view(np.uint64), od2.view(np.uint64)) and np.array_equal(idx, oidx)


def test_the_two_paths_give_equal_bytes():
    q, t = gm.main_pair()
    a, b = run_nearest(q, t, path=RING), run_nearest(q, t, path=STAGED)
    assert a[0] == 0 and b[0] == 0 and a[1].tobytes() == b[1].tobytes() and a[2].tobytes() == b[2].tobytes()
    assert a[3].tolist()[:2] == [0, len(q)] and b[3][0] > 0 and a[3][2] == b[3][2]


@BOTH
def test_two_calls_give_equal_bytes(path):
    q, t = gm.main_pair()
    a, b = run_nearest(q, t, path=path), run_nearest(q, t, path=path)
    assert all(np.array_equal(x.view(np.uint8), y.view(np.uint8)) for x, y in zip(a[1:], b[1:]))


# ---- corners
@BOTH
def test_one_target(path):
    q, _ = gm.main_pair()
    counts = check_against_oracle(q[:1000], np.array([[0.1, -0.2, 0.3]], np.float32), path=path)
    assert counts[2] == 1


@BOTH
@pytest.mark.parametrize("Q", [1, 259])
def test_query_counts_off_the_workgroup_size(Q, path):
    q, t = gm.main_pair()
    check_against_oracle(q[7:7 + Q], t, path=path)


@BOTH
def test_queries_far_outside_go_to_the_ring_scan(path):
    """200 queries at ten times the targets' extent outside their box, among 1 500 ordinary ones: the certificate cannot hold for them in a
    staged box, so phase 2 finishes them -- and phase 1 still certifies ordinary queries (both counts positive in one call)."""
    q, t = gm.main_pair()
    rng = np.random.default_rng(5)
    ext = float((t.max(0) - t.min(0)).max())
    far = rng.uniform(-0.5, 0.5, (200, 3))
    axis, sign = rng.integers(0, 3, 200), rng.choice([-1.0, 1.0], 200)
    far[np.arange(200), axis] = sign * 10.0 * ext
    qq = np.concatenate([q[:1500], far.astype(np.float32)])[rng.permutation(1700)]
    counts = check_against_oracle(qq, t, path=path)
    assert counts[1] >= 200 and (path == RING or counts[0] > 0)


@BOTH
def test_targets_on_a_plane(path):
    """z = const: the grid has zero extent on one axis."""
    q, t = gm.main_pair()
    flat = t.copy()
    flat[:, 2] = 0.125
    check_against_oracle(q[:2000], flat, path=path)
    check_against_oracle(flat[:777], flat, path=path)


@BOTH
def test_one_crowded_cell_takes_more_than_one_staging_chunk(path):
    from pointdreamer_amd import _lib
    chunk = _lib.lib().pdhip_nearest_points_stage_chunk()
    assert 6000 > chunk                                           # the crowded cell alone is more than one chunk
    rng = np.random.default_rng(6)
    crowd = (np.array([0.2, -0.1, 0.3]) + rng.uniform(0, 1e-3, (6000, 3))).astype(np.float32)
    spread = rng.uniform(-0.5, 0.5, (100, 3)).astype(np.float32)
    t = np.concatenate([crowd, spread])[rng.permutation(6100)]
    q = np.concatenate([(np.array([0.2, -0.1, 0.3]) + rng.uniform(-1e-3, 2e-3, (1000, 3))), rng.uniform(-0.5, 0.5, (900, 3))]).astype(np.float32)
    counts = check_against_oracle(q, t, path=path)
    assert path == RING or counts[0] >= 1000                      # (the LDS phase certified at least the queries round the crowd)


@BOTH
def test_copies_of_one_target_the_smallest_index_wins(path):
    q, t = gm.main_pair()
    rng = np.random.default_rng(7)
    tt = t.copy()
    where = rng.choice(len(tt), 2000, replace=False)
    tt[where] = tt[where[0]]
    qq = np.concatenate([q[:500], tt[where[:1]] + rng.normal(0, 0.01, (300, 3)).astype(np.float32), tt[where[:1]]])
    rc, d2, idx, _ = run_nearest(qq, tt, path=path)
    od2, oidx = gm.oracle_nearest(qq, tt)
    assert rc == 0 and np.array_equal(d2.view(np.uint64), od2.view(np.uint64)) and np.array_equal(idx, oidx)
    assert idx[-1] == where.min() and (idx == where.min()).sum() >= 1 and not np.isin(idx, np.setdiff1d(where, [where.min()])).any()


@BOTH
def test_a_true_tie_takes_the_smaller_index(path):
    """Two targets placed symmetrically about a query at exactly representable coordinates; the one with the LARGER index comes first in cell
    order (smaller x), so the order of the scan alone would pick it."""
    rng = np.random.default_rng(8)
    t = rng.uniform(1.0, 2.0, (600, 3)).astype(np.float32)
    t[400], t[13] = (-0.5, 0.25, 0.25), (0.5, 0.25, 0.25)
    q = np.concatenate([np.array([[0.0, 0.25, 0.25]], np.float32), rng.uniform(-0.5, 2.0, (300, 3)).astype(np.float32)])
    rc, d2, idx, _ = run_nearest(q, t, path=path)
    od2, oidx = gm.oracle_nearest(q, t)
    assert rc == 0 and np.array_equal(d2.view(np.uint64), od2.view(np.uint64)) and np.array_equal(idx, oidx)
    assert d2[0] == 0.25 and idx[0] == 13


@BOTH
@pytest.mark.parametrize("bad", [np.nan, np.inf])
@pytest.mark.parametrize("side", ["queries", "targets"])
def test_non_finite_coordinates_are_refused_and_nothing_is_written(bad, side, path):
    from pointdreamer_amd import _lib
    q, t = (x.copy() for x in gm.main_pair())
    (q if side == "queries" else t)[1234, 1] = bad
    rc, d2, idx, counts = run_nearest(q, t, path=path)
    assert rc == -1
    msg = _lib.lib().pdhip_last_error()
    assert b'non-finite' in msg and (b'query' if side == "queries" else b'target') in msg
    assert np.all(d2 == SENT_D2) and np.all(idx == SENT_IDX) and np.all(counts == SENT_CNT)


def test_no_queries_is_ok():
    _, t = gm.main_pair()
    rc, d2, idx, counts = run_nearest(np.zeros((0, 3), np.float32), t)
    assert rc == 0 and len(d2) == 0 and counts.tolist() == [0, 0, 0, 0]


# ---- pdhip_cloud_metrics
def run_metrics(d2, idx, ns, nt, M, thresholds, ws=None):
    from pointdreamer_amd import _lib
    from pointdreamer_amd._lib import ptr, stream
    L = _lib.lib()
    thr = T(np.asarray(thresholds, np.float64))
    sums = torch.full((4,), -1.0, dtype=torch.float64, device=DEV)
    within = torch.full((len(thresholds),), -1, dtype=torch.int64, device=DEV)
    if ws is None:
        ws = torch.empty((L.pdhip_cloud_metrics_workspace_bytes(len(thresholds)),), dtype=torch.uint8, device=DEV)
    d2t, idxt = T(np.asarray(d2, np.float64)), T(np.asarray(idx, np.int32))
    nst, ntt = (None if ns is None else T(np.asarray(ns, np.float32))), (None if nt is None else T(np.asarray(nt, np.float32)))
    rc = L.pdhip_cloud_metrics(ptr(d2t), ptr(idxt), len(d2), ptr(nst, allow_none=True), ptr(ntt, allow_none=True), M, ptr(thr), len(thresholds),
                               ptr(sums), ptr(within), ptr(ws), stream())
    torch.cuda.synchronize()
    assert rc == 0
    return sums.cpu().numpy(), within.cpu().numpy()


@pytest.fixture(scope="module")
def ref():
    g = load_golden('geometry_metrics_ref.npz')
    g['scores'] = dict(zip((str(k) for k in g['keys']), (float(v) for v in g['values'])))
    g['oracle'] = gm.oracle_eval_pointcloud(g['pointcloud'], g['pointcloud_tgt'], g['normals'], g['normals_tgt'])
    return g


def check_sums(sums, want, Q):
    for k in range(3):
        print('sum', k, sums[k], want[k], 'rel', abs(sums[k] - want[k]) / max(abs(want[k]), 1e-300), 'bound', Q * gm.EPS)
        assert abs(sums[k] - want[k]) <= Q * gm.EPS * abs(want[k])
    assert sums[3] == 0.0


def test_cloud_metrics_on_the_golden_fixture(ref):
    for side, src_n, dst_n, M in (('_completeness', ref['normals_tgt'], ref['normals'], 4096), ('_accuracy', ref['normals'], ref['normals_tgt'], 3500)):
        o = ref['oracle'][side]
        a = run_metrics(o['d2'], o['idx'], src_n, dst_n, M, gm.THRESHOLDS)
        b = run_metrics(o['d2'], o['idx'], src_n, dst_n, M, gm.THRESHOLDS)
        assert np.array_equal(a[1], o['within'])
        check_sums(a[0], o['sums'], len(o['d2']))
        assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()          # two calls, equal bytes
        no_normals = run_metrics(o['d2'], o['idx'], None, dst_n, M, gm.THRESHOLDS)
        assert no_normals[0][2] == 0.0 and no_normals[0][:2].tobytes() == a[0][:2].tobytes()


def test_cloud_metrics_with_thresholds_below_and_above_every_distance(ref):
    o = ref['oracle']['_accuracy']
    r = o['r']
    thr = np.array([0.0, r.min() * 0.5, r.min(), np.median(r), r.max(), r.max() * 2.0, 10.0])      # (r.min() and r.max() themselves: <= holds)
    _, within = run_metrics(o['d2'], o['idx'], None, None, 3500, thr)
    want = np.array([(r <= t).sum() for t in thr])
    assert np.array_equal(within, want) and within[0] == 0 and within[1] == 0 and within[2] >= 1 and within[4] == len(r) and within[-1] == len(r)


def test_zero_length_normals_contribute_zero_not_nan(ref):
    o = ref['oracle']['_accuracy']
    ns, nt = ref['normals'].copy(), ref['normals_tgt'].copy()
    ns[::7] = 0.0
    nt[::5] = 0.0
    ns[3] *= 1.0e-30                                              # (tiny but not zero: still normalised)
    sums, _ = run_metrics(o['d2'], o['idx'], ns, nt, 3500, gm.THRESHOLDS[:20])
    want = gm.fsum(gm.oracle_normal_dots(ns, nt, o['idx']))
    print(sums[2], want)
    assert np.isfinite(sums).all() and abs(sums[2] - want) <= len(ns) * gm.EPS * want
    assert sums[2] < o['sums'][2]


# ---- the Python interface
def test_eval_pointcloud_reproduces_the_reference(ref):
    from pointdreamer_amd import geometry_metrics as G
    got = G.eval_pointcloud(T(ref['pointcloud']), T(ref['pointcloud_tgt']), T(ref['normals']), T(ref['normals_tgt']))
    assert list(got) == [str(k) for k in ref['keys']]
    gm.assert_scores_close(got, ref['scores'], 4096)
    again = G.eval_pointcloud(ref['pointcloud'], T(ref['pointcloud_tgt']), ref['normals'], ref['normals_tgt'])      # (numpy follows the GPU tensor)
    assert again == got
    bare = G.eval_pointcloud(T(ref['pointcloud']), T(ref['pointcloud_tgt']))
    assert all(np.isnan(bare[k]) for k in ('normals completeness', 'normals accuracy', 'normals'))
    assert all(bare[k] == got[k] for k in got if not k.startswith('normals'))


def test_nearest_points_interface():
    from pointdreamer_amd import geometry_metrics as G
    q, t = gm.main_pair()
    d2, idx, counts = G.nearest_points(T(q), T(t), return_counts=True)
    od2, oidx = gm.oracle_main()
    assert d2.dtype == torch.float64 and idx.dtype == torch.int32 and d2.is_cuda
    assert np.array_equal(d2.cpu().numpy().view(np.uint64), od2.view(np.uint64)) and np.array_equal(idx.cpu().numpy(), oidx)
    assert counts.cpu().tolist()[:2] == [0, len(q)]


def test_empty_prediction_returns_the_reference_constants(ref):
    from pointdreamer_amd import geometry_metrics as G
    e = torch.zeros((0, 3), device=DEV)
    assert G.eval_pointcloud(e, T(ref['pointcloud_tgt'])) == {'completeness': np.sqrt(3), 'accuracy': np.sqrt(3), 'completeness2': 3, 'accuracy2': 3,
                                                              'chamfer': 6}
    full = G.eval_pointcloud(e, T(ref['pointcloud_tgt']), e, T(ref['normals_tgt']))
    assert full['normals completeness'] == -1. and full['normals accuracy'] == -1. and full['normals'] == -1. and len(full) == 8
    v = torch.zeros((0, 3), device=DEV)
    assert G.eval_mesh(v, torch.zeros((0, 3), dtype=torch.int64, device=DEV), T(ref['pointcloud_tgt']), T(ref['normals_tgt'])) == full


@pytest.fixture(scope="module")
def torus_mesh():
    import mesh_simplify_common as ms
    v, f = ms.grid_torus(40, 20)
    return T(v), T(f)


def test_eval_mesh_equals_eval_pointcloud_over_the_same_samples(ref, torus_mesh):
    from pointdreamer_amd import geometry_metrics as G
    from pointdreamer_amd.sample_colored_pc_from_mesh import sample_points
    v, f = torus_mesh
    tgt, ntgt = T(ref['pointcloud_tgt']), T(ref['normals_tgt'])
    rand = torch.rand((5000, 3), device=DEV, generator=torch.Generator(device=DEV).manual_seed(3))
    got = G.eval_mesh(v, f, tgt, ntgt, n_points=5000, rand=rand)
    s = sample_points(v, f, None, None, None, [{'Kd': np.zeros(3, np.float32)}], 5000, rand=rand)
    want = G.eval_pointcloud(s['coords'], tgt, s['normals'], ntgt)
    assert got == want and 'iou' not in got
    assert 0.0 < got['chamfer-L1'] < 0.05 and got['normals'] > 0.9


def test_eval_mesh_seed(ref, torus_mesh):
    from pointdreamer_amd import geometry_metrics as G
    v, f = torus_mesh
    tgt, ntgt = T(ref['pointcloud_tgt']), T(ref['normals_tgt'])
    a, b, c = (G.eval_mesh(v, f, tgt, ntgt, n_points=5000, seed=s) for s in (0, 0, 1))
    assert a == b and a != c
    assert abs(a['chamfer-L1'] - c['chamfer-L1']) < 0.1 * a['chamfer-L1']


# ---- the command-line tool
def test_run_geometry_evaluation(tmp_path, capsys):
    from pointdreamer_amd import geometry_metrics as G, io_utils, run_geometry_evaluation as rge, spr
    from pointdreamer_amd.sample_colored_pc_from_mesh import save_one_mesh_npy
    pred_root, gt_root = tmp_path / 'out' / 'pred', tmp_path / 'data' / 'pc_kaolin'
    shapes = {'solids/torus': 'torus', 'solids/sphere': 'sphere'}
    for name, solid in shapes.items():
        xyz, nrm = (np.array(x) for x in gm.solid_cloud(solid, 8000, 11))      # (writable copies: the cached clouds are read-only)
        spr.recon_one_shape_SPR(xyz, np.full_like(xyz, 0.5), gt_normals=nrm, depth=6, target_faces=3000,
                                save_path=str(pred_root / name / 'models' / 'model_normalized.obj'))
        n = len(xyz)
        save_one_mesh_npy(dict(name=name, coords=xyz, colors=np.full((n, 3), 0.5, np.float32), normals=nrm, uvs=np.zeros((n, 2), np.float32),
                               material_idx=np.zeros(n, np.uint8), face_idx=np.zeros(n, np.int32)), save_root=str(gt_root))
    res = rge.main(['--pred_root_path', str(pred_root), '--gt_root_path', str(gt_root), '--n_points', '6000', '--seed', '4'])
    out = capsys.readouterr().out
    assert res['sample_num'] == 2 and sorted(res['per_shape']) == sorted(shapes)
    api = {}
    for name in shapes:
        v, f = io_utils.load_obj_mesh(str(pred_root / name / 'models' / 'model_normalized.obj'))
        xyz, nrm = gm.solid_cloud(shapes[name], 8000, 11)
        api[name] = G.eval_mesh(T(v), T(f), T(xyz), T(nrm), n_points=6000, seed=4)
        assert res['per_shape'][name] == api[name]
        assert name in out and repr(api[name]['chamfer-L1']) in out
        assert api[name]['chamfer-L1'] < 0.03 and api[name]['f-score-20'] > 0.5          # a sound reconstruction of an 8 000-point cloud
    for k in api['solids/torus']:
        assert res['mean'][k] == float(np.mean([api[n][k] for n in api]))
    assert repr(res['mean']['chamfer-L1']) in out
    assert os.path.exists(res['result_file']) and os.path.dirname(res['result_file']) == str(tmp_path / 'out')
    txt = open(res['result_file']).read()
    assert 'chamfer-L1' in txt and repr(res['mean']['chamfer-L1']) in txt and 'sample num: 2' in txt
    os.remove(gt_root / 'solids' / 'sphere' / 'normals.npy')
    with pytest.raises(FileNotFoundError, match='solids/sphere'):
        rge.main(['--pred_root_path', str(pred_root), '--gt_root_path', str(gt_root)])
