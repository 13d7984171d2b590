"""Surface reconstruction stage by stage (csrc/surface_recon.hip) against oracle/spr_stages.py, observed in the workspace the caller owns.

pdhip_estimate_normals and pdhip_surface_recon carve every intermediate from the caller's workspace; pdhip_debug_estimate_normals_layout and
pdhip_debug_surface_recon_layout say where, and pdhip_debug_surface_recon_rhs returns the one stage the solve overwrites.  No kernel is run that the
product does not run.  Checks a, c and h are exact (bit for bit); b, d, e, f and g carry the bounds derived in tests/spr_stages_common.py, which
tests/test_spr_stages_cpu.py shows to hold for float32 emulations of the same stages.  Cases and clouds: spr_stages_common.

  a  k nearest neighbours: the float32 distances of the device's k indices are the k smallest, on every cloud and k (ties: any member)
  b  normal direction against np.linalg.eigh of the device's own neighbourhoods
  c  orientation: the three rules, applied to the device's final normals, return them; counts, eyes, visibility
  d  cell list (a stable sort by cell) and sample weights
  e  right-hand side, per node
  f  solve: true residual against the reported one plus the rounding drift of a float32 reference recurrence
  g  iso value to 1 ulp
  h  marching cubes: edge flags, vertices, faces

SPR_STAGES_RECORD=<path>: the worst ratio to every bound, the rows left out, the iteration counts and the drifts are written there when the module
is done (profiles/spr_stages_parity.txt is one such run)."""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

import spr_stages_common as sc
from oracle import spr_stages as st

pytestmark = pytest.mark.gpu
DEV = 'cuda'
F32, F64 = np.float32, np.float64
RECORD = {}
NULL = C.c_void_p(0)


def T(a):
    return torch.from_numpy(np.array(a)).to(DEV)                    # (a copy: the shared clouds are read-only)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def note(stage, case, **kw):
    RECORD.setdefault(stage, {})[case] = kw
    print(stage, case, ' '.join(f"{k}={v:.4g}" if isinstance(v, float) else f"{k}={v}" for k, v in kw.items()))


@pytest.fixture(scope="module", autouse=True)
def record_file():
    yield
    path = os.environ.get('SPR_STAGES_RECORD')
    if path and RECORD:
        with open(path, 'w') as f:
            f.write("Surface reconstruction stage by stage on one MI355X (tests/test_gpu_spr_stages.py against oracle/spr_stages.py): per case the worst\n"
                    "ratio of the device's error to the bound of the check (<= 1 passes), the rows check b leaves out, the solver's iterations on the\n"
                    "device and in the float32 reference recurrence, and that recurrence's drift |true - reported residual|.  Checks a, c and h are\n"
                    "exact and list what they compared.\n")
            for stage in sorted(RECORD):
                f.write(f"\n{stage}\n")
                for case, kw in RECORD[stage].items():
                    f.write(f"  {case:28s} " + '  '.join(f"{k} {v:.4g}" if isinstance(v, float) else f"{k} {v}" for k, v in kw.items()) + "\n")


def region(ws, off, nbytes, dtype):
    """A copy of ws[off : off + nbytes] on the host, viewed as dtype."""
    return ws[int(off):int(off) + int(nbytes)].cpu().numpy().view(dtype)


def lib():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from pointdreamer_amd import _lib
    return _lib, _lib.lib()


def eyes_for(name):
    return 4 if name in sc.ADVERSARIAL else 32


@functools.lru_cache(maxsize=None)
def normals_run(name, k, n_eyes):
    """pdhip_estimate_normals on a workspace of 0x55 bytes -> normals, counts and the regions the layout hook names."""
    m, L = lib()
    P = sc.cloud(name)[0]
    N = len(P)
    nbytes = L.pdhip_estimate_normals_ws_bytes(N, k, n_eyes)
    off = (C.c_uint64 * 6)()
    assert nbytes > 0 and L.pdhip_debug_estimate_normals_layout(N, k, n_eyes, off) == 0 and off[5] == nbytes
    ws = torch.full((nbytes,), 0x55, dtype=torch.uint8, device=DEV)
    X = T(P)
    nrm = torch.empty((N, 3), dtype=torch.float32, device=DEV)
    counts = torch.zeros((4,), dtype=torch.int32, device=DEV)
    rc = L.pdhip_estimate_normals(m.ptr(X), N, k, n_eyes, sc.EYE_RADIUS, m.ptr(nrm), m.ptr(counts), m.ptr(ws), m.stream())
    assert rc == 0, L.pdhip_last_error()
    torch.cuda.synchronize()
    return dict(P=P, normals=nrm.cpu().numpy(), counts=counts.cpu().tolist(), knn=region(ws, off[2], 4 * N * k, np.int32).reshape(N, k),
                eyes=region(ws, off[3], 24 * n_eyes, F64).reshape(n_eyes, 3), vis=region(ws, off[4], n_eyes * N, np.uint8).reshape(n_eyes, N))


@functools.lru_cache(maxsize=None)
def knn_reference(name):
    P = sc.cloud(name)[0]
    return st.knn_rows(P, min(32, len(P)))


@functools.lru_cache(maxsize=None)
def recon_run(name, depth):
    """pdhip_debug_surface_recon_rhs, then pdhip_surface_recon on a workspace of its own, with the cloud's analytic normals."""
    from pointdreamer_amd import spr
    m, L = lib()
    P, nrm = sc.cloud(name)
    N, M = len(P), 2 ** depth + 1
    n3 = M ** 3
    nbytes = L.pdhip_surface_recon_ws_bytes(N, depth)
    off = (C.c_uint64 * 8)()
    assert nbytes > 0 and L.pdhip_debug_surface_recon_layout(N, depth, off) == 0 and off[7] == nbytes
    X, Nn = T(P), T(nrm)
    ws = torch.full((nbytes,), 0x55, dtype=torch.uint8, device=DEV)
    f_out = torch.empty((n3,), dtype=torch.float32, device=DEV)
    rinfo = torch.zeros((8,), dtype=torch.float32, device=DEV)
    rc = L.pdhip_debug_surface_recon_rhs(m.ptr(X), m.ptr(Nn), N, depth, m.ptr(f_out), m.ptr(rinfo), m.ptr(ws), m.stream())
    assert rc == 0, L.pdhip_last_error()
    torch.cuda.synchronize()
    rinfo = rinfo.cpu().numpy()
    cells = int(rinfo[5]) ** 3 + 1
    front = lambda w: dict(cstart=region(w, off[0], 4 * cells, np.int32), spos=region(w, off[1], 16 * N, F32).reshape(N, 4),
                           snrm=region(w, off[2], 16 * N, F32).reshape(N, 4))
    out = dict(P=P, nrm=nrm, f=f_out.cpu().numpy().reshape(M, M, M), rhs_info=rinfo, **front(ws))
    ws2 = torch.full((nbytes,), 0x55, dtype=torch.uint8, device=DEV)
    vcap, fcap = spr.capacities(depth)
    verts = torch.empty((vcap, 3), dtype=torch.float32, device=DEV)
    faces = torch.empty((fcap, 3), dtype=torch.int64, device=DEV)
    counts = torch.zeros((4,), dtype=torch.int32, device=DEV)
    info = torch.zeros((8,), dtype=torch.float32, device=DEV)
    rc = L.pdhip_surface_recon(m.ptr(X), m.ptr(Nn), NULL, N, depth, m.ptr(verts), vcap, m.ptr(faces), fcap, NULL, m.ptr(counts), m.ptr(info),
                               m.ptr(ws2), m.stream())
    assert rc == 0, L.pdhip_last_error()
    torch.cuda.synchronize()
    nv, nf, iters, _ = counts.cpu().tolist()
    info = info.cpu().numpy()
    out.update(product=front(ws2), chi=region(ws2, off[3], 4 * n3, F32).reshape(M, M, M), eflag=region(ws2, off[4], n3, np.uint8).reshape(M, M, M),
               misc=region(ws2, off[5], 256, np.int32), verts=verts[:nv].cpu().numpy(), faces=faces[:nf].cpu().numpy(), nv=nv, nf=nf, iters=iters,
               info=info, grid=st.make_grid(info[0], info[1], info[2], info[3], int(info[7])))
    return out


def ids(cases):
    return ['-'.join(str(v) for v in c) for c in cases]


# ---- a
@pytest.mark.parametrize("name,k", sc.KNN_CASES, ids=ids(sc.KNN_CASES))
def test_a_knn_rows_hold_the_k_smallest_distances(name, k):
    r = normals_run(name, k, eyes_for(name))
    P, knn = r['P'], r['knn']
    N = len(P)
    assert knn.min() >= 0 and knn.max() < N
    srt = np.sort(knn, axis=1)
    assert np.all(srt[:, 1:] != srt[:, :-1]), "a row names a point twice"
    ref = knn_reference(name)
    got = np.sort(st.row_distances(P, knn), axis=1)
    bad = np.flatnonzero((bits(got) != bits(ref[:, :k])).any(1))
    assert len(bad) == 0, (len(bad), bad[:5], got[bad[:2]], ref[bad[:2], :k])
    cols = ref.shape[1]
    zero = (ref == 0).sum(1)                                       # the point's multiplicity, as far as the reference's columns show it
    known = zero < cols if cols < N else np.ones(N, bool)          # (all zero: there may be more copies than columns)
    allows = known & (zero <= k)
    has_self = (knn == np.arange(N)[:, None]).any(1)
    assert np.all(has_self[allows]), np.flatnonzero(~has_self & allows)[:5]
    note('a knn', f'{name} k={k}', rows=N, ties_at_k=int((ref[:, k - 1] == ref[:, k]).sum()) if k < cols else 0)


# ---- b
@pytest.mark.parametrize("name,k", sc.NORMAL_CASES, ids=ids(sc.NORMAL_CASES))
def test_b_normal_is_the_smallest_eigenvector_of_the_devices_neighbourhood(name, k):
    """sin(angle) <= 2^-23 + 2^-40 lambda_2 / (lambda_1 - lambda_0) on the rows with a direction to speak of (spr_stages_common).  With the direct
    trigonometric form alone the kernel missed this 10.3- and 11.8-fold on three near-collinear triples each of cup-6000-0 and rounded_box-6000-0
    at k = 3 (and reached 0.81 on torus-6000-0); smallest_eigvec's second branch brought every case to 0.31 - 0.38, the rounding to float32."""
    r = normals_run(name, k, 32)
    P, n = r['P'], r['normals']
    ref, lam = st.normal_direction(P, r['knn'])
    bound, keep = sc.normal_bound(lam)
    unit = np.abs(np.linalg.norm(n.astype(F64), axis=1) - 1.0).max()
    ratio = (sc.sin_angle(n, ref) / bound)[keep]
    note('b normal', f'{name} k={k}', worst_ratio=float(ratio.max()), left_out=int((~keep).sum()), rows=len(P), unit_error=float(unit))
    assert unit <= 2.0 ** -22
    assert (~keep).sum() <= 0.005 * len(P)
    assert ratio.max() <= 1.0, (int(ratio.argmax()), float(ratio.max()))


def test_b_coincident_neighbours_give_the_z_axis():
    r = normals_run('duplicates', 3, eyes_for('duplicates'))
    P, knn, n = r['P'], r['knn'], r['normals']
    same = np.all(P[knn] == P[knn[:, :1]], axis=(1, 2))
    assert same.sum() >= 0.9 * len(P)                              # four copies of every point, k = 3
    assert np.all(n[same, 0] == 0) and np.all(n[same, 1] == 0) and np.all(np.abs(n[same, 2]) == 1)


# ---- c
@pytest.mark.parametrize("name,k,n_eyes", sc.ORIENT_CASES, ids=ids(sc.ORIENT_CASES))
def test_c_orientation_rules_return_the_devices_normals(name, k, n_eyes):
    """The rules do not depend on the signs they are given (tests/test_spr_stages_cpu.py), so the oracle applied to the device's FINAL normals, with the
    device's neighbours, eyes and visibility, returns them bit for bit -- unless the device gave a point the wrong sign.  The eyes: within 4 ulp (float64)
    of the sphere's scale |centre| + radius (cos and sin are not correctly rounded, and a coordinate near zero has a smaller ulp of its own)."""
    from pointdreamer_amd import hpr
    r = normals_run(name, k, n_eyes)
    P, n = r['P'], r['normals']
    eyes = st.fibonacci_eyes(P, n_eyes, sc.EYE_RADIUS)
    mn, mx, ext = st.cloud_box(P)
    scale = np.abs(0.5 * (mn + mx)).max() + sc.EYE_RADIUS * ext
    assert np.abs(r['eyes'] - eyes).max() <= 4 * np.spacing(scale)
    vis = hpr.hidden_point_removal(T(P), r['eyes'], sc.HPR_RADIUS).cpu().numpy()
    assert np.array_equal(vis, r['vis'] != 0) and r['vis'].max() <= 1
    got, state, counts = st.orient(P, n, r['knn'], r['eyes'], r['vis'])
    note('c orientation', f'{name} k={k} eyes={n_eyes}', device_counts=r['counts'], oracle_counts=counts)
    assert counts == r['counts'] and sum(counts) == len(P)
    rows = state != 0
    assert np.array_equal(bits(got[rows]), bits(n[rows])), np.flatnonzero((bits(got) != bits(n)).any(1) & rows)[:5]
    if n_eyes == 1:
        assert min(counts) > 0, "one eye and two neighbours: all three rules and 'left as computed' must occur"
    else:
        assert counts[1] > 0, "the cup's inside must exercise the neighbour rule"


# ---- d
@pytest.mark.parametrize("name,depth", sc.RECON_CASES, ids=ids(sc.RECON_CASES))
def test_d_cell_list_and_sample_weights(name, depth):
    r = recon_run(name, depth)
    P, nrm, spos, snrm, cstart = r['P'], r['nrm'], r['spos'], r['snrm'], r['cstart']
    N = len(P)
    for key in ('spos', 'snrm', 'cstart'):                         # the hook leaves what the product leaves
        assert np.array_equal(bits(r[key]), bits(r['product'][key])), key
    # the grid, the radius and the cell list follow the documented rules
    grid, R, (origin, cs, Cn) = sc.recon_grid(P, depth)
    want = np.array([grid['h'], grid['ox'], grid['oy'], grid['oz'], cs, Cn, R, grid['M']], F32)
    assert np.array_equal(bits(r['rhs_info']), bits(want)), (r['rhs_info'], want)
    assert np.array_equal(bits(r['info'][[0, 1, 2, 3, 6, 7]]), bits(want[[0, 1, 2, 3, 6, 7]]))
    # spos: the cloud, sorted by cell, stable
    idx = np.ascontiguousarray(spos[:, 3]).view(np.int32)
    assert np.array_equal(np.sort(idx), np.arange(N)) and np.array_equal(bits(spos[:, :3]), bits(P[idx]))
    keys = sc.cell_keys(spos[:, :3], origin, cs, Cn)
    assert np.all(np.diff(keys) >= 0) and np.all((np.diff(keys) > 0) | (np.diff(idx) > 0))
    assert np.array_equal(cstart, np.searchsorted(keys, np.arange(Cn ** 3 + 1), side='left'))
    # the weights
    w, t = st.sample_weights(spos[:, :3], nrm[idx], R, terms=True)
    assert np.all(snrm[:, 3] == 0) and t['rho'].min() >= 1.0
    err, lim = np.abs(snrm[:, :3].astype(F64) - w), sc.weight_bound(t)[:, None] * np.abs(w)
    ratio = float((err[lim > 0] / lim[lim > 0]).max())
    note('d weights', f'{name} d{depth}', worst_ratio=ratio, R_over_h=float(R) / float(grid['h']), cells=Cn, most_neighbours=int(t['m'].max()))
    assert np.all(err <= lim), ratio


# ---- e
E_CASES = sc.RECON_CASES + [sc.DEEP_CASE]


@pytest.mark.parametrize("name,depth", E_CASES, ids=ids(E_CASES))
def test_e_right_hand_side(name, depth):
    r = recon_run(name, depth)
    i = r['rhs_info']
    grid, R = st.make_grid(i[0], i[1], i[2], i[3], int(i[7])), i[6]
    ref, t = st.rhs(r['spos'][:, :3], r['snrm'][:, :3], grid, R, terms=True)
    B = sc.rhs_bound(t)
    f = r['f']
    err = np.abs(f.astype(F64) - ref)
    ratio = float((err[B > 0] / B[B > 0]).max())
    note('e rhs', f'{name} d{depth}', worst_ratio=ratio, bound_over_f=float(B.max() / np.abs(ref).max()), nodes_with_points=int((t['m'] > 0).sum()),
         most_points=int(t['m'].max()))
    assert np.all(err <= B), (ratio, np.argwhere(err > B)[:5])
    assert np.all(f[(t['m'] == 0) & (t['srim'] == 0)] == 0)        # no point within R: exactly +-0
    edge = np.ones_like(f, bool)
    edge[1:-1, 1:-1, 1:-1] = False
    assert np.all(f[edge] == 0) and np.all(B[edge] == 0)
    assert B.max() <= 1.0e-5 * np.abs(ref).max()                   # the bound is not vacuous


# ---- f
@pytest.mark.parametrize("name,depth", sc.RECON_CASES, ids=ids(sc.RECON_CASES))
def test_f_solve(name, depth):
    r = recon_run(name, depth)
    chi, f = r['chi'], r['f']
    edge = np.ones_like(f, bool)
    edge[1:-1, 1:-1, 1:-1] = False
    assert np.all(bits(chi[edge]) == 0)
    true = st.true_residual(f, chi)
    _, it_ref, res_ref, true_ref = st.cg_f32(f, 1.0e-4)
    drift = abs(true_ref - float(res_ref))
    res = float(r['info'][5])
    note('f solve', f'{name} d{depth}', excess_over_8_drifts=(true - res) / (8 * drift), true_residual=true, reported=res, iterations=r['iters'], reference_iterations=it_ref,
         reference_drift=drift)
    assert 0 < r['iters'] == r['misc'][2] and bits(r['info'][5:6])[0] == r['misc'].view(np.uint32)[6]
    assert res <= 1.0e-4
    assert true <= res + 8 * drift


# ---- g, h
GH_CASES = sc.RECON_CASES + [sc.DEEP_CASE]


@pytest.mark.parametrize("name,depth", GH_CASES, ids=ids(GH_CASES))
def test_g_iso_value(name, depth):
    r = recon_run(name, depth)
    want = F32(st.iso_value(r['chi'], r['grid'], r['P']))
    dev = r['info'][4:5]
    assert bits(dev)[0] == r['misc'].view(np.uint32)[5] and dev[0] > 0
    ulps = abs(int(bits(dev)[0]) - int(bits(np.array([want]))[0]))
    note('g iso', f'{name} d{depth}', ulps=ulps, iso=float(dev[0]))
    assert ulps <= 1


@pytest.mark.parametrize("name,depth", GH_CASES, ids=ids(GH_CASES))
def test_h_marching_cubes(name, depth):
    r = recon_run(name, depth)
    fl, v, f = st.marching_cubes(r['chi'], r['info'][4], r['grid'])
    note('h marching cubes', f'{name} d{depth}', vertices=r['nv'], faces=r['nf'], crossing_edges=int(np.unpackbits(fl).sum()))
    assert np.array_equal(fl, r['eflag'])
    assert (r['nv'], r['nf']) == (len(v), len(f)) == (int(r['misc'][0]), int(r['misc'][1]))
    assert np.array_equal(bits(v), bits(r['verts']))
    assert np.array_equal(f, r['faces'])
