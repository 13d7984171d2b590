"""The point-in-mesh test and the volumetric IoU on the device (csrc/occupancy.hip, pointdreamer_amd/geometry_metrics.py: check_mesh_contains,
compute_iou, eval_mesh's `iou`; sample_colored_pc_from_mesh --occupancy; run_geometry_evaluation --points_root_path).
pdhip_mesh_contains is held to BYTE EQUALITY with the output of the reference's check_mesh_contains (tests/golden/occupancy_ref.npz) and with the
all-pairs float64 oracle of tests/occupancy_common.py: parities of integer counts do not depend on the order of the points or of the faces."""
import os

import numpy as np
import pytest
import torch

from conftest import load_golden
import occupancy_common as oc

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
SENT_OCC, SENT_CNT = 7, -777


def T(a):
    return torch.from_numpy(np.array(a)).to(DEV)                  # (a writable copy: the cached arrays are read-only)


def run_contains(v, f, p, resolution=512, ws=None):
    """(rc, occ, counts) of pdhip_mesh_contains; the outputs start as sentinels.  ws: the workspace to use instead of a fresh one."""
    from pointdreamer_amd import _lib
    from pointdreamer_amd._lib import ptr, stream
    L = _lib.lib()
    tv, tf, tp = T(np.asarray(v, np.float32)), T(np.asarray(f, np.int64)), T(np.asarray(p, np.float32).reshape(-1, 3))
    Vn, F, Q = tv.shape[0], tf.shape[0], tp.shape[0]
    occ = torch.full((max(Q, 1),), SENT_OCC, dtype=torch.uint8, device=DEV)
    counts = torch.full((4,), SENT_CNT, dtype=torch.int32, device=DEV)
    if ws is None:
        ws = torch.empty((L.pdhip_mesh_contains_workspace_bytes(Vn, F, Q, resolution),), dtype=torch.uint8, device=DEV)
    assert ws.numel() > 0
    rc = L.pdhip_mesh_contains(ptr(tv), Vn, ptr(tf), F, ptr(tp, allow_none=True) if Q else None, Q, resolution, ptr(occ), ptr(counts), ptr(ws),
                               stream())
    torch.cuda.synchronize()
    return rc, occ.cpu().numpy()[:Q], counts.cpu().numpy()


def check_against_oracle(v, f, p, resolution=512, oracle=None):
    rc, occ, counts = run_contains(v, f, p, resolution)
    assert rc == 0
    want, wcounts = oracle if oracle is not None else oc.oracle_contains(v, f, p, resolution, return_counts=True)
    print('F', len(f), 'Q', len(p), 'R', resolution, 'counts', counts.tolist(), 'oracle', wcounts, 'unequal', int((occ != want.astype(np.uint8)).sum()))
    assert np.array_equal(occ, want.astype(np.uint8))
    assert counts.tolist() == wcounts + [0]
    return occ, counts


# ---- parity with the reference and the oracle
@pytest.fixture(scope="module")
def ref():
    return load_golden('occupancy_ref.npz')


@pytest.mark.parametrize("case", oc.GOLDEN_CASES)
def test_golden_cases_equal_the_reference(ref, case):
    v, f, p, res = (ref[f'{case}_{k}'] for k in ('vertices', 'faces', 'points', 'hash_resolution'))
    rc, occ, counts = run_contains(v, f, p, int(res))
    assert rc == 0
    assert occ.tobytes() == ref[f'{case}_contains'].astype(np.uint8).tobytes()
    _, wcounts = oc.oracle_contains(v, f, p, int(res), return_counts=True)
    print(case, counts.tolist(), wcounts)
    assert counts.tolist() == wcounts + [0]


@pytest.mark.parametrize("resolution", [64, 512, 1000])
@pytest.mark.parametrize("kind", ['ico4', 'ico12'])
def test_equals_the_oracle(kind, resolution):
    v, f, p = oc.shared_case(kind)
    assert len(p) == {'ico4': 5003, 'ico12': 4099}[kind]
    occ, counts = check_against_oracle(v, f, p, resolution, oracle=oc.oracle_cached(kind, resolution))
    assert 0.3 * len(p) < counts[0] < 0.5 * len(p)              # (a ball of radius 0.5 in a cube of side 1.1)


@pytest.mark.parametrize("kind", ['ico40', 'ico41'])
def test_either_side_of_the_lanes_per_triangle_threshold(kind):
    """Below 32 768 faces a wave takes a triangle, from there on 16 lanes do: 32 000 and 33 620 faces against the oracle."""
    v, f, p = oc.shared_case(kind)
    assert len(f) == {'ico40': 32000, 'ico41': 33620}[kind]
    occ, counts = check_against_oracle(v, f, p, oracle=oc.oracle_cached(kind))
    assert 0.3 * len(p) < counts[0] < 0.5 * len(p)
    from pointdreamer_amd import _lib
    L = _lib.lib()
    old = L.pdhip_debug_set_mesh_contains_slabs(5)               # (several slabs with either group size)
    try:
        check_against_oracle(v, f, p, oracle=oc.oracle_cached(kind))
    finally:
        L.pdhip_debug_set_mesh_contains_slabs(old)


def test_two_calls_give_equal_bytes():
    v, f, p = oc.shared_case('ico12')
    a, b = run_contains(v, f, p), run_contains(v, f, p)
    assert a[0] == 0 and b[0] == 0 and a[1].tobytes() == b[1].tobytes() and a[2].tobytes() == b[2].tobytes()


def test_order_of_points_and_faces():
    v, f, p = oc.shared_case('ico12')
    want, wcounts = oc.oracle_cached('ico12')
    rng = np.random.default_rng(2)
    pp, pf = rng.permutation(len(p)), rng.permutation(len(f))
    rc, occ, counts = run_contains(v, f, p[pp])
    assert rc == 0 and np.array_equal(occ, want[pp].astype(np.uint8)) and counts.tolist() == wcounts + [0]
    rc, occ, counts = run_contains(v, f[pf], p)
    assert rc == 0 and np.array_equal(occ, want.astype(np.uint8)) and counts.tolist() == wcounts + [0]


# ---- edge cases of the reference's definition
def test_unreferenced_vertex_outside_points_and_the_box_boundary():
    v, f = oc.icosphere(4)
    lo, hi = v.min(axis=0), v.max(axis=0)
    v2 = np.concatenate([v, np.array([[50.0, -60.0, 70.0], [np.inf, np.nan, 0.0]], np.float32)])      # never referenced: neither moves the box
    p = np.array(oc.uniform_points(600, 41, 0.7))
    p[0], p[1], p[2] = (hi[0], 0.0, 0.0), (0.0, lo[1], 0.0), (0.0, 0.0, hi[2])                     # exactly on the box boundary
    p[3], p[4] = (np.nextafter(hi[0], np.float32(9)), 0.0, 0.0), (0.0, 0.0, np.nextafter(lo[2], np.float32(-9)))
    edge = np.float32(lo[0] - (hi[0] - lo[0]) * 0.5 / 511)        # x' ~ 0: the boundary of the rescaled box [0, R]^3, which is half a cell wider
    p[5], p[6], p[7] = (edge, 0.0, 0.0), (np.nextafter(edge, np.float32(9)), 0.0, 0.0), (np.nextafter(edge, np.float32(-9)), 0.0, 0.0)
    want = oc.oracle_contains(v, f, p, return_counts=True)
    occ, counts = check_against_oracle(v2, f, p, oracle=want)
    outside = np.any((p < lo) | (p > hi), axis=1)
    assert 100 < counts[2] <= outside.sum() and not occ[outside].any()
    assert not occ[:8].any()


def test_degenerate_faces_contribute_nothing():
    v, f = oc.icosphere(4)
    n = len(v)
    extra_v = np.array([[-0.2, -0.2, -0.3], [0.3, 0.3, 0.4], [0.3, 0.3, -0.1],      # a wall over the segment (-0.2, -0.2) .. (0.3, 0.3) of xy: vertical
                        [0.1, -0.3, 0.2], [0.1, 0.0, 0.0], [0.1, 0.4, -0.2]], np.float32)      # x constant: projects to a segment
    extra_f = np.array([[3, 3, 9], [5, 7, 5], [11, 11, 11],                          # repeated indices
                        [n, n + 1, n + 2], [n + 3, n + 4, n + 5]], np.int64)
    v2, f2 = np.concatenate([v, extra_v]), np.concatenate([f, extra_f])
    p = np.array(oc.uniform_points(2001, 42))
    p[:3, :2] = (0.05, 0.05), (0.1, -0.1), (0.1, 0.2)            # on the xy of the two walls
    occ, _ = check_against_oracle(v2, f2, p)
    assert np.array_equal(occ, oc.oracle_contains(v, f, p).astype(np.uint8))          # the extra faces changed nothing


@pytest.mark.parametrize("kind", ['box', 'tetra'])
def test_few_large_and_few_tiny_faces(kind):
    v, f, p = oc.shared_case(kind)
    occ, counts = check_against_oracle(v, f, p, oracle=oc.oracle_cached(kind))
    assert len(f) == {'box': 12, 'tetra': 4}[kind] and counts[0] > 20 and counts[2] > 20
    if kind == 'box':                                            # the box itself: inside is |coordinate| < 0.5 (no sample lies on a diagonal)
        assert np.array_equal(occ.astype(bool), np.all(np.abs(p) < 0.5, axis=1))


@pytest.mark.parametrize("kind", ['box', 'ico12'])
def test_waves_per_triangle_do_not_show_in_the_result(kind):
    """pdhip_debug_set_mesh_contains_slabs: 1, 3 and 64 column slabs per triangle against the oracle (the shipped choice follows F)."""
    from pointdreamer_amd import _lib
    L = _lib.lib()
    v, f, p = oc.shared_case(kind)
    for slabs in (1, 3, 64):
        old = L.pdhip_debug_set_mesh_contains_slabs(slabs)
        try:
            check_against_oracle(v, f, p, oracle=oc.oracle_cached(kind))
        finally:
            assert L.pdhip_debug_set_mesh_contains_slabs(old) == slabs
        assert old == 0


def test_one_face_contains_nothing():
    v, f = oc.icosphere(4)
    tri = v[f[17]]
    lo, hi = tri.min(axis=0), tri.max(axis=0)
    p = ((lo + hi) / 2 + (hi - lo) * 1.2 * oc.uniform_points(1001, 43, 0.5)).astype(np.float32)      # around the face's box: a hit has one parity only
    occ, counts = check_against_oracle(v, f[17:18], p)
    assert not occ.any() and counts[0] == 0 and counts[1] > 100 and counts[2] > 100


# ---- an independent analytic bound: a convex mesh inscribed in the sphere of radius 0.5
def test_convex_mesh_between_its_inscribed_and_circumscribed_spheres():
    v, f = oc.icosphere(8)
    p = oc.uniform_points(6007, 44)
    tri = v.astype(np.float64)[f]
    n = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    plane = np.abs((n * tri[:, 0]).sum(1)) / np.linalg.norm(n, axis=1)      # distance of each face plane from the centre
    r_in, r_out = plane.min() * (1 - 1e-6), np.linalg.norm(v.astype(np.float64), axis=1).max() * (1 + 1e-6)
    rc, occ, _ = run_contains(v, f, p)
    r = np.linalg.norm(p.astype(np.float64), axis=1)
    print('inscribed', r_in, 'circumscribed', r_out, 'inside', int((r < r_in).sum()), 'outside', int((r > r_out).sum()), 'between',
          int(((r >= r_in) & (r <= r_out)).sum()))
    assert rc == 0 and 0.48 < r_in < 0.5 < r_out < 0.5001
    assert occ[r < r_in].all() and not occ[r > r_out].any() and (r < r_in).sum() > 1500 and (r > r_out).sum() > 1500


# ---- sizes and refusals
@pytest.mark.parametrize("Q", [1, 63, 65, 257])
def test_small_point_counts(Q):
    v, f = oc.icosphere(4)
    p = oc.uniform_points(257, 45, 0.4)[:Q]
    check_against_oracle(v, f, p)


def test_no_points_is_ok():
    v, f = oc.icosphere(4)
    rc, occ, counts = run_contains(v, f, np.zeros((0, 3), np.float32))
    assert rc == 0 and len(occ) == 0 and counts.tolist() == [0, 0, 0, 0]


@pytest.mark.parametrize("what", ['vertex_nan', 'vertex_inf', 'point_nan', 'point_inf', 'face_high', 'face_negative', 'flat'])
def test_bad_inputs_are_refused_by_name_and_nothing_is_written(what):
    from pointdreamer_amd import _lib
    v, f = (np.array(x) for x in oc.icosphere(4))
    p = np.array(oc.uniform_points(700, 46))
    word = {'vertex': b'vertex', 'point': b'point', 'face': b'index', 'flat': b'flat'}[what.split('_')[0]]
    if what.startswith('vertex'):
        v[f[100, 1], 2] = np.nan if what.endswith('nan') else -np.inf
    elif what.startswith('point'):
        p[333, 0] = np.nan if what.endswith('nan') else np.inf
    elif what.startswith('face'):
        f[200, 2] = len(v) if what.endswith('high') else -1
    else:
        v[:, 1] = 0.25
    rc, occ, counts = run_contains(v, f, p)
    msg = _lib.lib().pdhip_last_error()
    print(what, msg)
    assert rc == -1 and b'pdhip_mesh_contains' in msg and word in msg
    assert np.all(occ == SENT_OCC) and np.all(counts == SENT_CNT)


# ---- the Python interface
def test_check_mesh_contains_interface():
    from pointdreamer_amd import geometry_metrics as G
    v, f, p = oc.shared_case('ico12')
    want, wcounts = oc.oracle_cached('ico12')
    occ, counts = G.check_mesh_contains(T(v), T(f), T(p), return_counts=True)
    assert occ.dtype == torch.bool and occ.is_cuda and tuple(occ.shape) == (len(p),)
    assert np.array_equal(occ.cpu().numpy(), want) and counts.cpu().tolist() == wcounts + [0]
    assert torch.equal(G.check_mesh_contains(T(v), np.array(f), np.array(p)), occ)        # numpy faces / points follow the vertices
    want64, _ = oc.oracle_cached('ico12', 64)
    assert np.array_equal(G.check_mesh_contains(T(v), T(f), T(p), hash_resolution=64).cpu().numpy(), want64)


def test_compute_iou():
    from pointdreamer_amd import geometry_metrics as G
    rng = np.random.default_rng(9)
    a = rng.random(5003) < 0.4
    b = rng.random(5003) < 0.5
    assert G.compute_iou(T(a), T(a)) == 1.0
    assert G.compute_iou(T(a), T(~a)) == 0.0
    want = float(np.float32((a & b).sum()) / np.float32((a | b).sum()))
    assert G.compute_iou(T(a), T(b)) == want and 0.2 < want < 0.4
    assert G.compute_iou(T(a), b) == want                        # a numpy array follows the tensor
    soft = np.where(b, 0.5, 0.49999).astype(np.float32)           # binarised at >= 0.5
    assert G.compute_iou(T(a.astype(np.float32)), T(soft)) == want
    assert G.compute_iou(T(a.astype(np.uint8)), T(b.astype(np.int64))) == want
    assert np.isnan(G.compute_iou(T(np.zeros(100, bool)), T(np.zeros(100, bool))))
    assert np.isnan(G.compute_iou(T(np.zeros(0, bool)), T(np.zeros(0, bool))))


def test_eval_mesh_iou():
    from pointdreamer_amd import geometry_metrics as G
    import geometry_metrics_common as gm
    v, f, p = oc.shared_case('ico12')
    gv, gf = oc.icosphere(8)
    occ_tgt = oc.oracle_contains(gv, gf, p)
    tgt, ntgt = (T(x) for x in gm.solid_cloud('sphere', 3000, 5))
    base = G.eval_mesh(T(v), T(f), tgt, ntgt, n_points=4000, seed=2)
    got = G.eval_mesh(T(v), T(f), tgt, ntgt, n_points=4000, seed=2, points_iou=T(p), occ_tgt=T(occ_tgt))
    assert 'iou' not in base and len(base) == 12 and set(got) == set(base) | {'iou'}
    assert all(got[k] == base[k] for k in base)
    mine = oc.oracle_cached('ico12')[0]
    want = float(np.float32((mine & occ_tgt).sum()) / np.float32((mine | occ_tgt).sum()))
    print('iou', got['iou'], want)
    assert got['iou'] == want and 0.8 < want < 1.0
    packed = np.packbits(occ_tgt)
    assert len(packed) == (len(p) + 7) // 8 != len(p)
    for form in (packed, T(packed), occ_tgt, T(occ_tgt.astype(np.float32))):
        assert G.eval_mesh(T(v), T(f), tgt, ntgt, n_points=4000, seed=2, points_iou=np.array(p), occ_tgt=form) == got
    e = torch.zeros((0, 3), device=DEV)
    empty = G.eval_mesh(e, torch.zeros((0, 3), dtype=torch.int64, device=DEV), tgt, ntgt, points_iou=T(p), occ_tgt=T(occ_tgt))
    assert empty['iou'] == 0.0 and 'iou' not in G.eval_mesh(e, torch.zeros((0, 3), dtype=torch.int64, device=DEV), tgt, ntgt)
    only_one = G.eval_mesh(T(v), T(f), tgt, ntgt, n_points=4000, seed=2, points_iou=T(p))
    assert only_one == base


# ---- end to end: the ground-truth writer and the evaluation tool
def test_occupancy_files_and_the_iou_column(tmp_path, capsys):
    from pointdreamer_amd import camera_utils, run_geometry_evaluation as rge, sample_colored_pc_from_mesh as scp
    from pointdreamer_amd.sample_colored_pc_from_mesh import save_one_mesh_npy
    import geometry_metrics_common as gm
    v, f = oc.icosphere(8)
    root = tmp_path / 'data'
    mesh_file = root / 'meshes' / 'c' / 's' / 'models' / 'model_normalized.obj'
    os.makedirs(mesh_file.parent)
    with open(mesh_file, 'w') as fh:
        fh.write(''.join('v %.9g %.9g %.9g\n' % tuple(x) for x in v.tolist()) + ''.join('f %d %d %d\n' % tuple(i + 1 for i in t) for t in f.tolist()))
    assert scp.main(['--rootpath', str(root), '--occupancy', '4099', '--seed', '3']) == 0
    assert 'occupancies of 1 shape' in capsys.readouterr().out
    npz = root / 'point' / 'c' / 's.npz'
    with np.load(npz) as z:
        assert sorted(z.files) == ['occupancies', 'points']
        points, packed = z['points'], z['occupancies']
    assert points.dtype == np.float32 and points.shape == (4099, 3) and packed.dtype == np.uint8 and packed.shape == ((4099 + 7) // 8,)
    assert np.abs(points).max() <= 0.55 and np.abs(points).max() > 0.54
    normalised = camera_utils._normalized(T(v)).cpu().numpy()
    want = oc.oracle_contains(normalised, f, points)
    assert np.array_equal(np.unpackbits(packed)[:4099].astype(bool), want) and 0.3 * 4099 < want.sum() < 0.5 * 4099
    stamp = os.stat(npz).st_mtime_ns
    assert scp.main(['--rootpath', str(root), '--occupancy', '4099', '--seed', '3']) == 0      # an existing file is skipped
    assert 'occupancies of 0 shape' in capsys.readouterr().out and os.stat(npz).st_mtime_ns == stamp
    # the same mesh as the prediction
    gt_root = root / 'pc_kaolin'
    xyz, nrm = (np.array(x) for x in gm.solid_cloud('sphere', 3000, 5))
    n = len(xyz)
    save_one_mesh_npy(dict(name='c/s', coords=xyz, colors=np.full((n, 3), 0.5, np.float32), normals=nrm, uvs=np.zeros((n, 2), np.float32),
                           material_idx=np.zeros(n, np.uint8), face_idx=np.zeros(n, np.int32)), save_root=str(gt_root))
    args = ['--pred_root_path', str(root / 'meshes'), '--gt_root_path', str(gt_root), '--n_points', '4000', '--seed', '1']
    res = rge.main(args + ['--points_root_path', str(root / 'point')])
    out = capsys.readouterr().out.splitlines()
    assert res['per_shape']['c/s']['iou'] == 1.0 and res['mean']['iou'] == 1.0
    header = 'shape\t' + '\t'.join(rge.KEYS)
    assert out[0] == header + '\tiou' and out[1].startswith('c/s\t') and out[1].endswith('\t1.0')
    mean_at = out.index('\t'.join(rge.KEYS) + '\tiou')
    assert out[mean_at + 1].endswith('\t1.0') and len(out[mean_at + 1].split('\t')) == len(rge.KEYS) + 1
    assert 'iou' in open(res['result_file']).read()
    bare = rge.main(args)
    out = capsys.readouterr().out.splitlines()
    assert out[0] == header and 'iou' not in bare['per_shape']['c/s'] and 'iou' not in bare['mean'] and not any('\tiou' in line for line in out)
    assert all(bare['per_shape']['c/s'][k] == res['per_shape']['c/s'][k] for k in bare['per_shape']['c/s'])
    # a shape without an .npz under the flag: no iou for it, NaN in its column
    os.remove(npz)
    none = rge.main(args + ['--points_root_path', str(root / 'point')])
    assert 'iou' not in none['per_shape']['c/s'] and np.isnan(none['mean']['iou'])
