"""The point-to-mesh distance without a GPU: the tests' all-pairs float64 oracle (tests/mesh_distance_common.py) against analytic distances, the
closest point against its face, the argument validation of the new entry points, the workspace size against the layout, and zero scratch on the new
kernels."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import ROOT
import mesh_distance_common as md
import occupancy_common as oc

LIB = os.path.join(ROOT, 'pointdreamer_amd', 'libpdhip.so')


def _lib():
    import __graft_entry__ as ge
    ge.build()
    from pointdreamer_amd import _lib
    return _lib.lib()


# ---- the oracle against analytic distances
def test_oracle_equals_the_box_distance_exactly():
    v, f = oc.box_mesh()
    p = oc.uniform_points(5003, 61, 0.7)
    d2, face, closest, ndeg = md.oracle_closest(v, f, p)
    want = md.box_distance(p)
    err = np.abs(np.sqrt(d2) - want)
    print('box: max error', err.max(), 'inside', int((np.abs(p).max(axis=1) < 0.5).sum()), 'of', len(p))
    assert ndeg == 0 and err.max() == 0.0
    assert 500 < (np.abs(p).max(axis=1) < 0.5).sum() < 4000 and face.min() >= 0 and face.max() <= 11


def test_oracle_on_a_convex_sphere_lies_in_the_analytic_sandwich():
    v, f = oc.icosphere(8)
    p = oc.uniform_points(5003, 62, 0.7)
    d2, _, _, ndeg = md.oracle_closest(v, f, p)
    r_in, r_out = md.convex_radii(v, f)
    assert ndeg == 0 and 0.49 < r_in < 0.5 < r_out < 0.5001
    md.assert_sandwich(p, np.sqrt(d2), r_in, r_out)


@pytest.mark.parametrize("kind", ['ico8', 'mixed', 'sliver', 'far', 'single'])
def test_closest_lies_on_its_face_and_gives_d2(kind):
    v, f, p = md.shared_case(kind)
    d2, face, closest, ndeg = md.oracle_cached(kind)
    assert ndeg == (md.mixed_mesh()[2] if kind == 'mixed' else 0) and face.min() >= 0 and np.all(md.live_faces(v, f)[face])
    r = p.astype(np.float64) - closest
    assert np.array_equal(((r[:, 0] * r[:, 0] + r[:, 1] * r[:, 1]) + r[:, 2] * r[:, 2]).view(np.uint64), d2.view(np.uint64))
    # barycentric coordinates of `closest` in its face, by least squares: inside the triangle, and the residual (distance from its plane) is rounding
    tri = v.astype(np.float64)[f[face]]
    a, ab, ac = tri[:, 0], tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]
    scale = np.abs(tri).max(axis=(1, 2))
    g11, g12, g22 = (ab * ab).sum(1), (ab * ac).sum(1), (ac * ac).sum(1)
    rhs1, rhs2 = ((closest - a) * ab).sum(1), ((closest - a) * ac).sum(1)
    det = g11 * g22 - g12 * g12
    well = det > 1e-6 * g11 * g22                                  # (a sliver's coordinates are ill conditioned: only the residual is checked)
    with np.errstate(divide='ignore', invalid='ignore'):
        u, w = (g22 * rhs1 - g12 * rhs2) / det, (g11 * rhs2 - g12 * rhs1) / det
    res = np.linalg.norm(closest - (a + u[:, None] * ab + w[:, None] * ac), axis=1)
    print(kind, 'well conditioned', int(well.sum()), 'of', len(well), 'max residual / scale', (res[well] / scale[well]).max(), 'min u, w, 1 - u - w',
          u[well].min(), w[well].min(), (1 - u - w)[well].min())
    assert well.sum() > 0.9 * len(well)
    assert np.all(res[well] <= 1e-12 * scale[well])
    assert np.all(u[well] >= -1e-9) and np.all(w[well] >= -1e-9) and np.all((u + w)[well] <= 1 + 1e-9)


def test_shared_cases_are_what_the_gpu_tests_expect():
    v, f, ndeg = md.mixed_mesh()
    assert len(f) == 1285 and ndeg == 4 and (~md.live_faces(v, f)).sum() == 4 and not np.isfinite(v[-1]).all() and (f != len(v) - 1).all()
    assert len(md.shared_case('ico8')[2]) == 3001 and len(md.shared_case('ico8')[1]) == 1280 and len(md.shared_case('far')[1]) == 320
    assert np.sqrt(md.oracle_cached('far')[0]).min() > 3.0         # every point of the far case is many mesh diameters away
    assert md.live_faces(*md.sliver_mesh()).all() and len(md.sliver_mesh()[1]) == 344


def test_ties_across_shared_edges_follow_the_face_order():
    """Queries at the mesh's own vertices: d2 == 0 exactly and the smallest incident face wins; a permutation of the faces keeps every d2 bit."""
    v, f = oc.icosphere(4)
    d2, face, closest, _ = md.oracle_closest(v, f, v)
    first = np.array([np.nonzero((f == i).any(axis=1))[0][0] for i in range(len(v))])
    assert np.all(d2 == 0.0) and np.array_equal(face, first) and np.array_equal(closest, v.astype(np.float64))
    perm = np.random.default_rng(4).permutation(len(f))
    d2p, facep, _, _ = md.oracle_closest(v, f[perm], v)
    assert np.array_equal(d2p.view(np.uint64), d2.view(np.uint64)) and not np.array_equal(perm[facep], face)


# ---- the entry points
def test_argument_validation_names_the_cause():
    L = _lib()
    one = C.c_void_p(256)                                        # (never dereferenced: the arguments are refused first)
    ok = dict(vertices=one, Vn=8, faces=one, F=12, points=one, Q=5, d2=one, face=one, closest=one, counts=one, ws=one, stream=None)
    order = list(ok)
    call = lambda **kw: L.pdhip_closest_on_mesh(*[dict(ok, **kw)[k] for k in order])
    for name in ('vertices', 'faces', 'points', 'd2', 'face', 'counts', 'ws'):
        assert call(**{name: None}) == -1
        msg = L.pdhip_last_error()
        assert b'pdhip_closest_on_mesh' in msg and b'null pointer' in msg and ('(%s)' % name).encode() in msg, msg
    for kw, word in ((dict(Vn=0), b'Vn=0'), (dict(F=0), b'degenerate'), (dict(F=-1), b'F=-1'), (dict(F=(1 << 23) + 1), b'F=8388609'), (dict(Q=-1), b'Q=-1'),
                     (dict(Q=(1 << 26) + 1), b'Q=67108865')):
        assert call(**kw) == -1
        assert b'pdhip_closest_on_mesh' in L.pdhip_last_error() and word in L.pdhip_last_error(), (kw, L.pdhip_last_error())


def test_debug_hook_returns_the_previous_setting():
    L = _lib()
    assert L.pdhip_debug_set_closest_on_mesh(3, 2) == 0
    assert L.pdhip_debug_set_closest_on_mesh(64, 1) == 4 * 3 + 2
    assert L.pdhip_debug_set_closest_on_mesh(1000, 7) == 4 * 64 + 1          # clamped to the largest grid / an unknown path is the shipped one
    assert L.pdhip_debug_set_closest_on_mesh(0, 0) == 4 * md.CELLS_MAX + 0
    assert L.pdhip_debug_set_closest_on_mesh(0, 0) == 0


def test_workspace_size_refuses_what_the_entry_refuses():
    ws = _lib().pdhip_closest_on_mesh_workspace_bytes
    assert ws(8, 12, 5) > 0 and ws(8, 12, 0) > 0 and ws(1, md.F_MAX, md.Q_MAX) > 0 and ws(1, 1, 0) > 0
    for args in ((0, 12, 5), (8, 0, 5), (8, -1, 5), (8, md.F_MAX + 1, 5), (8, 12, -1), (8, 12, md.Q_MAX + 1)):
        assert ws(*args) == 0, args


@pytest.mark.parametrize("Q", [0, 1, 63, 65, 257, 4099, 100000])
@pytest.mark.parametrize("F", [1, 12, 1280, 200000])
def test_workspace_size_is_the_carve_of_the_layout(F, Q):
    got = _lib().pdhip_closest_on_mesh_workspace_bytes(1000, F, Q)
    print(F, Q, got, md.closest_workspace_bytes(F, Q))
    assert got == md.closest_workspace_bytes(F, Q)
    assert got == _lib().pdhip_closest_on_mesh_workspace_bytes(7, F, Q)      # a function of (F, Q) alone


def test_product_has_no_cpu_path():
    import torch
    from pointdreamer_amd import _lib, geometry_metrics as G
    v, f, p = torch.zeros((4, 3)), torch.zeros((1, 3), dtype=torch.int64), torch.zeros((5, 3))
    with pytest.raises(_lib.PdhipError):
        G.closest_on_mesh(v, f, p)
    with pytest.raises(_lib.PdhipError):
        G.distance_p2m(p, v, f)
    with pytest.raises(_lib.PdhipError):
        G.distance_p2m(np.zeros((5, 3), np.float32), np.zeros((4, 3), np.float32), np.zeros((1, 3), np.int64))
    assert G.P2M_KEYS == ('completeness-p2m', 'completeness2-p2m', 'normals completeness-p2m')


def test_no_scratch_on_the_mesh_distance_kernels():
    if not os.path.exists(LIB):
        _lib()
    pytest.importorskip('msgpack')                          # (as tests/test_code_objects_cpu.py: the metadata note is msgpack)
    from tools import code_object_notes
    # (GridPointKey: csrc/cell_list.h's key of the shared f64 grid, every including unit's copy; MdFar: its far scan pair instantiated for this unit)
    mine = [k for k in code_object_notes.kernels(LIB)
            if 'k_md_' in k['name'] or 'MdFaceKey' in k['name'] or 'GridPointKey' in k['name'] or 'MdFar' in k['name']]
    for must in (('k_md_degenerate',), ('MdFaceKey',), ('k_cell_keys', 'GridPointKey'), ('k_md_gather',), ('k_md_ring_scan',), ('k_far_scan', 'MdFar'),
                 ('k_far_pick', 'MdFar'), ('k_md_closest',), ('k_md_counts',)):
        assert any(all(m in k['name'] for m in must) for k in mine), must            # (both parts in ONE kernel's name)
    for k in mine:
        print(k['name'], 'vgprs', k['vgpr_count'], 'lds', k['group_segment_fixed_size'], 'scratch', k['private_segment_fixed_size'])
        assert k['arch'] == 'gfx950'
        assert k['vgpr_spill_count'] == 0 and k['private_segment_fixed_size'] == 0, k
