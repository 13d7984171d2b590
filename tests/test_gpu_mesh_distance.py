"""The point-to-mesh distance on the device (csrc/mesh_distance.hip, pointdreamer_amd/geometry_metrics.py: closest_on_mesh, distance_p2m, eval_mesh's
p2m scores; run_geometry_evaluation --p2m).  pdhip_closest_on_mesh is held to BIT EQUALITY with the all-pairs float64 oracle of
tests/mesh_distance_common.py (d2 as uint64, the face, the closest point) on every path: a face's value depends on no other face, so neither the cell
list nor the order of the scan may show in the result."""
import os

import numpy as np
import pytest
import torch

import geometry_metrics_common as gm
import mesh_distance_common as md
import occupancy_common as oc

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
SENT_D2, SENT_FACE, SENT_CNT = -7.5, -777, -777


def T(a):
    return torch.from_numpy(np.array(a)).to(DEV)                  # (a writable copy: the cached arrays are read-only)


def run_closest(v, f, p, want_closest=True, ws=None):
    """(rc, d2, face, closest, counts) of pdhip_closest_on_mesh; the outputs start as sentinels.  ws: the workspace to use instead of a fresh one."""
    from pointdreamer_amd import _lib
    from pointdreamer_amd._lib import ptr, stream
    L = _lib.lib()
    tv, tf, tp = T(np.asarray(v, np.float32)), T(np.asarray(f, np.int64).reshape(-1, 3)), T(np.asarray(p, np.float32).reshape(-1, 3))
    Vn, F, Q = tv.shape[0], tf.shape[0], tp.shape[0]
    d2 = torch.full((max(Q, 1),), SENT_D2, dtype=torch.float64, device=DEV)
    face = torch.full((max(Q, 1),), SENT_FACE, dtype=torch.int32, device=DEV)
    closest = torch.full((max(Q, 1), 3), SENT_D2, dtype=torch.float64, device=DEV)
    counts = torch.full((4,), SENT_CNT, dtype=torch.int32, device=DEV)
    if ws is None:
        ws = torch.empty((max(L.pdhip_closest_on_mesh_workspace_bytes(Vn, F, Q), 8),), dtype=torch.uint8, device=DEV)
    opt = lambda x: ptr(x) if x.numel() else None
    rc = L.pdhip_closest_on_mesh(ptr(tv), Vn, opt(tf), F, opt(tp), Q, ptr(d2), ptr(face), ptr(closest) if want_closest else None, ptr(counts), ptr(ws),
                                 stream())
    torch.cuda.synchronize()
    return rc, d2.cpu().numpy()[:Q], face.cpu().numpy()[:Q], closest.cpu().numpy()[:Q], counts.cpu().numpy()


def assert_equal_bits(got, want, what=''):
    d2, face, closest = got
    wd2, wface, wclosest = want
    print(what, 'Q', len(wd2), 'unequal d2', int((d2.view(np.uint64) != wd2.view(np.uint64)).sum()), 'face', int((face != wface).sum()), 'closest',
          int((closest.view(np.uint64) != wclosest.view(np.uint64)).any(axis=1).sum()))
    assert np.array_equal(d2.view(np.uint64), wd2.view(np.uint64))
    assert np.array_equal(face, wface)
    assert np.array_equal(closest.view(np.uint64), wclosest.view(np.uint64))


def check_against_oracle(v, f, p, oracle=None, what=''):
    rc, d2, face, closest, counts = run_closest(v, f, p)
    assert rc == 0
    wd2, wface, wclosest, ndeg = oracle if oracle is not None else md.oracle_closest(v, f, p)
    print(what, 'F', len(f), 'counts', counts.tolist(), 'degenerate', ndeg)
    assert_equal_bits((d2, face, closest), (wd2, wface, wclosest), what)
    assert counts[3] == ndeg and counts[0] + counts[1] == len(wd2) and counts[0] >= 0 and counts[1] >= 0
    assert 0 <= counts[2] <= len(f) - ndeg
    return d2, face, closest, counts


class hook:
    """pdhip_debug_set_closest_on_mesh(cells, path) for a `with` block; the old setting comes back at its end."""
    def __init__(self, cells, path):
        self.args = (cells, path)

    def __enter__(self):
        from pointdreamer_amd import _lib
        self.L = _lib.lib()
        self.old = self.L.pdhip_debug_set_closest_on_mesh(*self.args)
        return self

    def __exit__(self, *exc):
        assert self.L.pdhip_debug_set_closest_on_mesh(self.old // 4, self.old % 4) == 4 * self.args[0] + self.args[1]


# ---- bit equality with the oracle
@pytest.mark.parametrize("kind", ['ico8', 'box', 'tetra', 'single', 'mixed', 'far', 'sliver'])
def test_equals_the_oracle(kind):
    v, f, p = md.shared_case(kind)
    d2, face, closest, counts = check_against_oracle(v, f, p, md.oracle_cached(kind), kind)
    if kind == 'box':                                             # (12 faces: one cell, so none is large; with three cells per axis all are)
        assert len(f) == 12 and np.abs(np.sqrt(d2) - md.box_distance(p)).max() == 0.0
        with hook(3, 0):
            assert check_against_oracle(v, f, p, md.oracle_cached(kind), 'box, 3 cells per axis')[3][2] == 12
    if kind == 'mixed':
        assert counts[3] == 4 and 1 <= counts[2] < 100 and counts[0] > 0          # the small list, the large list and the skipped faces together
    if kind == 'far':
        assert counts[1] > 0                                      # many mesh diameters away: the all-faces scan
    if kind == 'sliver':
        assert counts[2] >= 12                                    # the twelve needles (smallest angle below 3e-4 rad) at least never rely on the certificate
    if kind == 'ico8':
        assert counts[0] > 0.9 * len(p) and counts[2] == 0


@pytest.mark.parametrize("cells,path", [(1, 0), (3, 0), (64, 0), (0, 1), (0, 2), (3, 1), (64, 2)])
@pytest.mark.parametrize("kind", ['mixed', 'sliver'])
def test_grid_and_path_do_not_show_in_the_result(kind, cells, path):
    v, f, p = md.shared_case(kind)
    with hook(cells, path):
        d2, face, closest, counts = check_against_oracle(v, f, p, md.oracle_cached(kind), f'{kind} cells={cells} path={path}')
    if path == 1:
        assert counts[2] == md.live_faces(v, f).sum()
    if path == 2:
        assert counts[0] == 0 and counts[1] == len(p)
    from pointdreamer_amd import _lib
    assert _lib.lib().pdhip_debug_set_closest_on_mesh(0, 0) == 0  # restored


@pytest.mark.parametrize("cells,path", [(0, 0), (8, 0), (0, 1)])
def test_crowded_rings_go_to_the_all_faces_scan(cells, path):
    """5 120 faces: the rings of a point near the centre hold more faces than one thread takes (2 048), which hands the query to the staged scan of
    all faces; the points near the surface stay with the ring scan.  With every face on the large list (5 120 <= 8 192) each query scans that list
    and is done."""
    v, f, p = md.shared_case('crowded')
    assert len(f) == 5120
    with hook(cells, path):
        d2, face, closest, counts = check_against_oracle(v, f, p, md.oracle_cached('crowded'), f'crowded cells={cells} path={path}')
    if path == 1:
        assert counts[2] == 5120 and counts[0] == len(p)
    else:
        assert counts[0] > 100 and counts[1] > 100


def test_a_long_large_list_goes_to_the_all_faces_scan():
    """8 820 faces, all on the large list: more than the 8 192 a query scans by itself, so every query takes the staged scan."""
    v, f, p = md.shared_case('long_large')
    assert len(f) == 8820
    with hook(0, 1):
        d2, face, closest, counts = check_against_oracle(v, f, p, md.oracle_cached('long_large'), 'long large list')
    assert counts[2] == 8820 and counts[1] == len(p)
    check_against_oracle(v, f, p, md.oracle_cached('long_large'), 'the same, shipped')


def test_queries_on_vertices_and_edge_midpoints():
    v, f = oc.icosphere(8)
    q = md.vertex_and_midpoint_queries()
    want = md.oracle_closest(v, f, q)
    d2, face, closest, _ = check_against_oracle(v, f, q, want, 'vertices + midpoints')
    nv = len(v)
    assert np.all(d2[:nv] == 0.0) and np.array_equal(closest[:nv], v.astype(np.float64))
    first = np.array([np.nonzero((f == i).any(axis=1))[0][0] for i in range(nv)])
    assert np.array_equal(face[:nv], first)                      # of the faces round a vertex, the smallest index
    assert d2[nv:].max() < 1e-12


def test_order_of_points_and_faces():
    v, f, p = md.shared_case('ico8')
    p = p[:1201]
    wd2, wface, wclosest, _ = (x[:1201] if isinstance(x, np.ndarray) else x for x in md.oracle_cached('ico8'))
    rng = np.random.default_rng(2)
    pp, pf = rng.permutation(len(p)), rng.permutation(len(f))
    rc, d2, face, closest, _ = run_closest(v, f, p[pp])
    assert rc == 0
    assert_equal_bits((d2, face, closest), (wd2[pp], wface[pp], wclosest[pp]), 'permuted points')
    # permuted faces: every d2 bit stays; the winner of a true tie (a point nearest to a shared edge or vertex) follows the new order, so the
    # comparison is with the oracle on the permuted faces
    pd2, pface, pclosest, _ = md.oracle_closest(v, f[pf], p)
    assert np.array_equal(pd2.view(np.uint64), wd2.view(np.uint64))
    rc, d2, face, closest, _ = run_closest(v, f[pf], p)
    assert rc == 0
    assert_equal_bits((d2, face, closest), (pd2, pface, pclosest), 'permuted faces')
    print('winners that moved with the order', int((pf[face] != wface).sum()))


def test_two_calls_give_equal_bytes():
    v, f, p = md.shared_case('mixed')
    a, b = run_closest(v, f, p), run_closest(v, f, p)
    assert a[0] == 0 and b[0] == 0
    for x, y in zip(a[1:], b[1:]):
        assert x.tobytes() == y.tobytes()


@pytest.mark.parametrize("Q", [1, 63, 65, 257])
def test_small_point_counts(Q):
    v, f, p = md.shared_case('ico8')
    want = md.oracle_cached('ico8')
    check_against_oracle(v, f, p[:Q], (want[0][:Q], want[1][:Q], want[2][:Q], want[3]))


def test_no_points_is_ok():
    v, f = oc.icosphere(4)
    rc, d2, face, closest, counts = run_closest(v, f, np.zeros((0, 3), np.float32))
    assert rc == 0 and len(d2) == 0 and counts.tolist() == [0, 0, 0, 0]


def test_closest_is_optional():
    v, f, p = md.shared_case('mixed')
    rc, d2, face, closest, counts = run_closest(v, f, p, want_closest=False)
    wd2, wface, _, _ = md.oracle_cached('mixed')
    assert rc == 0 and np.array_equal(d2.view(np.uint64), wd2.view(np.uint64)) and np.array_equal(face, wface)
    assert np.all(closest == SENT_D2)


@pytest.mark.parametrize("what", ['vertex_nan', 'vertex_inf', 'point_nan', 'point_inf', 'index_high', 'index_negative', 'degenerate_all',
                                  'degenerate_no_faces'])
def test_bad_inputs_are_refused_by_name_and_nothing_is_written(what):
    from pointdreamer_amd import _lib
    v, f = (np.array(x) for x in oc.icosphere(4))
    p = np.array(oc.uniform_points(700, 46))
    word = what.split('_')[0].encode()
    if what.startswith('vertex'):
        v[f[100, 1], 2] = np.nan if what.endswith('nan') else -np.inf
    elif what.startswith('point'):
        p[333, 0] = np.nan if what.endswith('nan') else np.inf
    elif what.startswith('index'):
        f[200, 2] = len(v) if what.endswith('high') else -1
    elif what == 'degenerate_all':
        f[:, 2] = f[:, 0]
    else:
        f = f[:0]
    rc, d2, face, closest, counts = run_closest(v, f, p)
    msg = _lib.lib().pdhip_last_error()
    print(what, msg)
    assert rc == -1 and b'pdhip_closest_on_mesh' in msg and word in msg
    assert np.all(d2 == SENT_D2) and np.all(face == SENT_FACE) and np.all(closest == SENT_D2) and np.all(counts == SENT_CNT)


def test_sizes_beyond_the_limits_are_refused():
    from pointdreamer_amd import _lib
    L = _lib.lib()
    assert L.pdhip_closest_on_mesh_workspace_bytes(8, md.F_MAX + 1, 5) == 0 and L.pdhip_closest_on_mesh_workspace_bytes(8, 12, md.Q_MAX + 1) == 0
    one = torch.zeros((64,), dtype=torch.uint8, device=DEV)
    from pointdreamer_amd._lib import ptr
    for F, Q, word in ((md.F_MAX + 1, 5, b'F='), (12, md.Q_MAX + 1, b'Q=')):
        assert L.pdhip_closest_on_mesh(ptr(one), 8, ptr(one), F, ptr(one), Q, ptr(one), ptr(one), None, ptr(one), ptr(one), None) == -1
        assert word in L.pdhip_last_error()
    assert not one.cpu().numpy().any()


def test_unreferenced_vertices_change_nothing():
    v, f, p = md.shared_case('ico8')
    v2 = np.concatenate([v, np.array([[50.0, -60.0, 70.0], [np.inf, np.nan, 0.0]], np.float32)])
    want = md.oracle_cached('ico8')
    check_against_oracle(v2, f, p[:1001], (want[0][:1001], want[1][:1001], want[2][:1001], 0))


# ---- an independent analytic bound on the device result
def test_convex_sphere_lies_in_the_analytic_sandwich():
    v, f = oc.icosphere(8)
    p = oc.uniform_points(6007, 64, 0.7)
    rc, d2, _, _, _ = run_closest(v, f, p)
    assert rc == 0
    md.assert_sandwich(p, np.sqrt(d2), *md.convex_radii(v, f))


# ---- the Python interface
def test_closest_on_mesh_and_distance_p2m_interface():
    from pointdreamer_amd import geometry_metrics as G
    v, f, p = md.shared_case('mixed')
    wd2, wface, wclosest, ndeg = md.oracle_cached('mixed')
    out = G.closest_on_mesh(T(v), T(f), T(p))
    assert len(out) == 2
    d2, face = out
    assert d2.dtype == torch.float64 and face.dtype == torch.int32 and d2.is_cuda and face.is_cuda and tuple(d2.shape) == tuple(face.shape) == (len(p),)
    assert np.array_equal(d2.cpu().numpy().view(np.uint64), wd2.view(np.uint64)) and np.array_equal(face.cpu().numpy(), wface)
    d2b, faceb, closest, counts = G.closest_on_mesh(T(v), np.array(f), np.array(p), return_closest=True, return_counts=True)      # numpy follows the vertices
    assert torch.equal(d2b, d2) and torch.equal(faceb, face)
    assert closest.dtype == torch.float64 and tuple(closest.shape) == (len(p), 3) and closest.is_cuda
    assert np.array_equal(closest.cpu().numpy().view(np.uint64), wclosest.view(np.uint64))
    assert counts.dtype == torch.int32 and counts.cpu().tolist()[3] == ndeg and int(counts[0] + counts[1]) == len(p)
    assert len(G.closest_on_mesh(T(v), T(f), T(p), return_counts=True)) == 3
    d = G.distance_p2m(T(p), T(v), T(f))
    assert d.dtype == torch.float64 and d.is_cuda and np.array_equal(d.cpu().numpy().view(np.uint64), np.sqrt(wd2).view(np.uint64))
    assert torch.equal(G.distance_p2m(np.array(p), T(v), np.array(f)), d)
    e = G.closest_on_mesh(T(v), T(f), torch.zeros((0, 3), device=DEV), return_closest=True)
    assert tuple(e[0].shape) == (0,) and tuple(e[2].shape) == (0, 3)


def host_p2m(v, f, tgt, n_tgt):
    """The three p2m scores on the host from the oracle's (d2, face): exactly rounded sums over the target cloud."""
    d2, face, _, _ = md.oracle_closest(v, f, tgt)
    tri = np.asarray(v, np.float32).astype(np.float64)[f]
    fn = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]).astype(np.float32)
    n = float(len(tgt))
    return {'completeness-p2m': gm.fsum(np.sqrt(d2)) / n, 'completeness2-p2m': gm.fsum(d2) / n,
            'normals completeness-p2m': gm.fsum(gm.oracle_normal_dots(n_tgt, fn, face)) / n}


def test_eval_mesh_p2m():
    from pointdreamer_amd import geometry_metrics as G
    v, f = oc.icosphere(8)
    tgt, ntgt = gm.solid_cloud('sphere', 3000, 5)
    base = G.eval_mesh(T(v), T(f), T(tgt), T(ntgt), n_points=300, seed=2)
    got = G.eval_mesh(T(v), T(f), T(tgt), T(ntgt), n_points=300, seed=2, p2m=True)
    assert len(base) == 12 and set(got) == set(base) | set(G.P2M_KEYS) and list(got)[:12] == list(base)
    assert all(got[k] == base[k] for k in base)                  # the twelve old scores: the same bits
    want = host_p2m(v, f, tgt, ntgt)
    bound = (len(tgt) + 8) * gm.EPS
    for k in G.P2M_KEYS:
        print(k, got[k], want[k], 'rel', abs(got[k] - want[k]) / abs(want[k]), 'bound', bound)
        assert abs(got[k] - want[k]) <= bound * abs(want[k]), k
    # 300 samples of a sphere of radius 0.5 lie about 0.1 apart, so the nearest SAMPLE is some 0.04 away while the surface itself is within the
    # sagitta of a face (below 0.003): the distance to a surface is at most the distance to any of its points
    print('completeness', got['completeness'], 'completeness-p2m', got['completeness-p2m'])
    assert got['completeness-p2m'] <= got['completeness'] and got['completeness2-p2m'] <= got['completeness2']
    assert got['completeness-p2m'] < 0.003 and got['completeness'] > 0.02
    assert got['normals completeness-p2m'] > 0.99
    e = torch.zeros((0, 3), device=DEV)
    empty = G.eval_mesh(e, torch.zeros((0, 3), dtype=torch.int64, device=DEV), T(tgt), T(ntgt), p2m=True)
    assert empty['completeness-p2m'] == G.EMPTY_PCL_DICT['completeness'] and empty['completeness2-p2m'] == G.EMPTY_PCL_DICT['completeness2']
    assert empty['normals completeness-p2m'] == G.EMPTY_PCL_DICT_NORMALS['normals completeness']
    assert not set(G.P2M_KEYS) & set(G.eval_mesh(e, torch.zeros((0, 3), dtype=torch.int64, device=DEV), T(tgt), T(ntgt)))


# ---- end to end: the evaluation tool
def test_run_geometry_evaluation_p2m(tmp_path, capsys):
    from pointdreamer_amd import geometry_metrics as G, run_geometry_evaluation as rge
    from pointdreamer_amd.sample_colored_pc_from_mesh import save_one_mesh_npy
    v, f = oc.icosphere(8)
    root = tmp_path / 'data'
    mesh_file = root / 'meshes' / 'c' / 's' / 'models' / 'model_normalized.obj'
    os.makedirs(mesh_file.parent)
    with open(mesh_file, 'w') as fh:
        fh.write(''.join('v %.9g %.9g %.9g\n' % tuple(x) for x in v.tolist()) + ''.join('f %d %d %d\n' % tuple(i + 1 for i in t) for t in f.tolist()))
    gt_root = root / 'pc_kaolin'
    xyz, nrm = (np.array(x) for x in gm.solid_cloud('sphere', 3000, 5))
    n = len(xyz)
    save_one_mesh_npy(dict(name='c/s', coords=xyz, colors=np.full((n, 3), 0.5, np.float32), normals=nrm, uvs=np.zeros((n, 2), np.float32),
                           material_idx=np.zeros(n, np.uint8), face_idx=np.zeros(n, np.int32)), save_root=str(gt_root))
    args = ['--pred_root_path', str(root / 'meshes'), '--gt_root_path', str(gt_root), '--n_points', '4000', '--seed', '1']
    res = rge.main(args + ['--p2m'])
    out = capsys.readouterr().out.splitlines()
    header = 'shape\t' + '\t'.join(rge.KEYS)
    assert out[0] == header + '\t' + '\t'.join(G.P2M_KEYS)
    row = out[1].split('\t')
    assert row[0] == 'c/s' and len(row) == 1 + len(rge.KEYS) + 3
    want = host_p2m(v, f, xyz, nrm)
    shape = res['per_shape']['c/s']
    for j, k in enumerate(G.P2M_KEYS):
        assert float(row[1 + len(rge.KEYS) + j]) == shape[k] == res['mean'][k]
        assert abs(shape[k] - want[k]) <= (n + 8) * gm.EPS * abs(want[k]), k
    mean_at = out.index('\t'.join(rge.KEYS + G.P2M_KEYS))
    assert out[mean_at + 1].split('\t')[-3:] == [repr(res['mean'][k]) for k in G.P2M_KEYS]
    text = open(res['result_file']).read()
    assert all(k in text for k in G.P2M_KEYS) and all(repr(res['mean'][k]) in text for k in G.P2M_KEYS)
    # without the flag: the output of before
    bare = rge.main(args)
    bare_out = capsys.readouterr().out.splitlines()
    assert bare_out[0] == header and not any('p2m' in line for line in bare_out)
    assert not set(G.P2M_KEYS) & set(bare['per_shape']['c/s']) and not set(G.P2M_KEYS) & set(bare['mean'])
    assert all(bare['per_shape']['c/s'][k] == shape[k] for k in bare['per_shape']['c/s'])
    assert bare_out[1] == '\t'.join(row[:1 + len(rge.KEYS)])
    assert 'p2m' not in open(bare['result_file']).read().splitlines()[-2]       # (the keys of the last record; both runs may share a file name)
