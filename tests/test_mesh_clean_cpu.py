"""Mesh cleaning without a GPU: the oracle of tests/mesh_clean_common.py against independent implementations (scipy's k-d tree and connected
components; np.unique), and the argument checks of pdhip_weld_vertices / pdhip_clean_faces, which refuse before any device call."""
import ctypes as C

import numpy as np
import pytest
import torch

import mesh_clean_common as mcc


@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as ge
    ge.build()
    from pointdreamer_amd import _lib
    return _lib.lib()


def cloud_with_near_duplicates(seed, n=1500, tol=1e-3):
    rng = np.random.default_rng(seed)
    base = rng.random((n // 3, 3))
    v = np.concatenate([base, base + rng.uniform(-0.45, 0.45, base.shape) * tol, base + rng.uniform(-0.45, 0.45, base.shape) * tol])
    return np.ascontiguousarray(v[rng.permutation(len(v))].astype(np.float32))


@pytest.mark.parametrize("seed", [0, 1])
def test_oracle_classes_equal_kdtree_pairs_and_connected_components(seed):
    from scipy.spatial import cKDTree
    tol = 1e-3
    v = cloud_with_near_duplicates(seed, tol=tol)
    x = v.astype(np.float64)
    d = np.sqrt(((x[:, None] - x[None]) ** 2).sum(-1))
    assert not (np.abs(d - tol) <= 1e-9 * tol).any()              # no pair near the threshold: the two definitions of "close" cannot differ
    pairs = cKDTree(x).query_pairs(tol, output_type='ndarray')
    want = mcc.rep_of_labels(mcc.graph_labels(len(v), pairs))
    got = mcc.oracle_weld(v, tol)
    assert np.array_equal(got, want)
    assert 400 < len(np.unique(got)) < len(v)
    # the graph route the oracle takes for a crowd agrees with its sequential union-find
    assert np.array_equal(mcc.oracle_weld(v, tol, max_pairs=0), got)


def test_oracle_at_tolerance_zero_equals_unique_rows():
    sv, sf = mcc.soup(*mcc.icosphere(2))
    assert np.array_equal(mcc.oracle_weld(sv, 0.0), mcc.oracle_weld_exact(sv))
    nv, _ = mcc.two_tetrahedra_soup(negative_zero=True)
    rep = mcc.oracle_weld(nv, 0.0)
    assert np.array_equal(rep, mcc.oracle_weld_exact(nv)) and len(np.unique(rep)) == 8


def test_oracle_cleans_the_icosphere_soup_back_to_the_indexed_mesh():
    v, f = mcc.icosphere(2)
    sv, sf = mcc.soup(v, f)
    o = mcc.oracle_clean(sv, sf)
    assert len(o['vertices']) == 162 and len(o['faces']) == 320 and o['counts']['merged'] == 960 - 162
    assert np.array_equal(o['vertices'][o['faces']], v[f])         # the same triangles, corner for corner


def test_oracle_faces_rules():
    rep = np.array([0, 1, 2, 3, 0, 5], np.int32)                   # vertex 4 welds onto 0
    f = np.array([[0, 1, 2], [1, 2, 4], [2, 1, 0], [4, 0, 3], [3, 5, 1], [2, 0, 1]], np.int64)
    rf, keep, c = mcc.oracle_clean_faces(f, rep)
    assert keep.tolist() == [True, False, False, False, True, False] and c == dict(degenerate=1, duplicate=3, kept=2)
    assert rf[1].tolist() == [1, 2, 0] and rf[3].tolist() == [0, 0, 3]


# ---- the entries refuse before any device call
P = C.c_void_p(4096)


def weld(L, vertices=P, Vn=8, tol=0.0, rep=P, counts=P, ka=P, kb=P, va=P, vb=P, sort_len=8, hist=P, hist_words=512, cstart=P, cstart_len=2, sxyzi=P,
         sorted_len=8, parent=P, parent_len=8, misc=P, misc_len=64):
    return L.pdhip_weld_vertices(vertices, Vn, tol, rep, counts, ka, kb, va, vb, sort_len, hist, hist_words, cstart, cstart_len, sxyzi, sorted_len,
                                 parent, parent_len, misc, misc_len, None)


def faces(L, f=P, F=8, rep=P, Vn=8, out=P, keep=P, counts=P, ka=P, kb=P, va=P, vb=P, sort_len=8, hist=P, hist_words=512, misc=P, misc_len=64):
    return L.pdhip_clean_faces(f, F, rep, Vn, out, keep, counts, ka, kb, va, vb, sort_len, hist, hist_words, misc, misc_len, None)


@pytest.mark.parametrize("name", ['vertices', 'rep', 'counts', 'ka', 'kb', 'va', 'vb', 'hist', 'cstart', 'sxyzi', 'parent', 'misc'])
def test_weld_refuses_null_pointers(L, name):
    assert weld(L, **{name: None}) == -1
    msg = L.pdhip_last_error()
    assert b'pdhip_weld_vertices: null pointer' in msg


def test_weld_refuses_sizes_and_tolerances(L):
    for Vn in (0, -3, (1 << 26) + 1):
        assert weld(L, Vn=Vn) == -1 and f'Vn={Vn}'.encode() in L.pdhip_last_error()
    for tol in (-1e-30, float('nan'), float('inf'), -float('inf')):
        assert weld(L, tol=tol) == -1 and b'tol=' in L.pdhip_last_error() and b'finite number >= 0' in L.pdhip_last_error()


@pytest.mark.parametrize("arg,short,name", [('sort_len', 2999, b'keys_a / keys_b / vals_a / vals_b'), ('hist_words', 1023, b'hist'),
                                            ('cstart_len', 19 ** 3, b'cstart'), ('sorted_len', 2999, b'sorted_xyzi'), ('parent_len', 2999, b'parent'),
                                            ('misc_len', 63, b'misc')])
def test_weld_refuses_short_temporaries_by_name(L, arg, short, name):
    full = dict(Vn=3000, sort_len=3000, hist_words=1024, cstart_len=19 ** 3 + 1, sorted_len=3000, parent_len=3000, misc_len=64)
    assert L.pdhip_weld_cells_axis(3000) == 19 and L.pdhip_weld_cells_axis(1) == 1 and L.pdhip_weld_cells_axis(1 << 26) == 256
    assert L.pdhip_weld_cells_axis(0) == 0
    assert weld(L, **dict(full, **{arg: short})) == -1
    msg = L.pdhip_last_error()
    assert b'pdhip_weld_vertices: ' + name + b' holds ' + str(short).encode() in msg and b'Vn=3000 needs' in msg
    assert weld(L, **dict(full, sxyzi=C.c_void_p(4100))) == -1 and b'16 bytes' in L.pdhip_last_error()      # every length right: the alignment


@pytest.mark.parametrize("name", ['f', 'rep', 'out', 'keep', 'counts', 'ka', 'kb', 'va', 'vb', 'hist', 'misc'])
def test_clean_faces_refuses_null_pointers(L, name):
    assert faces(L, **{name: None}) == -1 and b'pdhip_clean_faces: null pointer' in L.pdhip_last_error()


def test_clean_faces_refuses_sizes_and_short_temporaries(L):
    assert faces(L, Vn=0) == -1 and b'Vn=0' in L.pdhip_last_error()
    assert faces(L, F=0) == -1 and b'F=0' in L.pdhip_last_error()
    assert faces(L, Vn=(1 << 21) + 1) == -1
    assert b'Vn=2097153 exceeds 2^21 = 2097152' in L.pdhip_last_error()
    assert faces(L, F=(1 << 23) + 1, sort_len=1 << 24, hist_words=1 << 24) == -1 and b'F=8388609' in L.pdhip_last_error()
    big = dict(F=5000, sort_len=5000, hist_words=1536)
    for arg, short, name in (('sort_len', 4999, b'keys_a / keys_b / vals_a / vals_b'), ('hist_words', 1535, b'hist'), ('misc_len', 8, b'misc')):
        assert faces(L, **dict(big, **{arg: short})) == -1
        assert b'pdhip_clean_faces: ' + name + b' holds ' + str(short).encode() in L.pdhip_last_error()


def test_mesh_clean_refuses_cpu_tensors():
    from pointdreamer_amd import mesh_clean as M
    from pointdreamer_amd._lib import PdhipError
    v, f = torch.zeros((4, 3)), torch.zeros((2, 3), dtype=torch.int64)
    with pytest.raises(PdhipError):
        M.weld_vertices(v)
    with pytest.raises(PdhipError):
        M.clean_mesh(v, f)
    with pytest.raises(PdhipError):
        M.mesh_report(v, f)
    for bad in (-1.0, float('nan'), float('inf'), True, '0'):
        with pytest.raises(ValueError):
            M.weld_vertices(v, tolerance=bad)


def test_demo_validates_the_clean_keys(tmp_path):
    import os
    from pointdreamer_amd import demo
    cfg = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'configs', 'nearest.yaml')
    assert demo.load_config(cfg, dict(mesh_clean='weld', mesh_weld_tolerance=0.001)).mesh_clean == 'weld'
    assert 'mesh_clean' not in demo.load_config(cfg)
    for over in (dict(mesh_clean='merge'), dict(mesh_weld_tolerance=0.001), dict(mesh_clean='weld', mesh_weld_tolerance=0.2),
                 dict(mesh_clean='weld', mesh_weld_tolerance=-1e-9), dict(mesh_clean='weld', mesh_weld_tolerance=True)):
        with pytest.raises(ValueError):
            demo.load_config(cfg, over)
