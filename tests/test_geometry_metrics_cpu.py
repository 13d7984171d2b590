"""Geometry scores without a GPU: the tests' float64 oracle against the values the reference's MeshEvaluator.eval_pointcloud gave
(tests/golden/geometry_metrics_ref.npz from tools/gen_golden_geometry_metrics.py), the argument validation of the new entry points, the
workspace size against the layout, and zero scratch on the new kernels."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import ROOT, load_golden
import geometry_metrics_common as gm

LIB = os.path.join(ROOT, 'pointdreamer_amd', 'libpdhip.so')


@pytest.fixture(scope="module")
def ref():
    g = load_golden('geometry_metrics_ref.npz')
    g['scores'] = dict(zip((str(k) for k in g['keys']), (float(v) for v in g['values'])))
    return g


def test_fixture_keeps_thresholds_and_ties_out_of_the_scores(ref):
    assert ref['pointcloud'].shape == (4096, 3) and ref['pointcloud_tgt'].shape == (3500, 3)
    assert ref['pointcloud'].dtype == np.float32 and ref['normals_tgt'].dtype == np.float32
    assert len(ref['scores']) == 12
    gap, ties = gm.fixture_conditions(ref['pointcloud'], ref['pointcloud_tgt'])
    print('smallest |distance - threshold|', gap, 'tied queries', ties)
    assert gap > 1e-9 and ties == 0


def test_oracle_reproduces_the_reference(ref):
    got = gm.oracle_eval_pointcloud(ref['pointcloud'], ref['pointcloud_tgt'], ref['normals'], ref['normals_tgt'])
    assert set(ref['scores']) == set(gm.KEYS_MEAN + gm.KEYS_F)
    gm.assert_scores_close(got, ref['scores'], 4096)


def test_oracle_takes_the_smallest_index_on_a_tie():
    t = np.array([[2, 0, 0], [-0.5, 0, 0], [0.5, 0, 0], [0.5, 0, 0]], np.float32)
    d2, idx, second = gm.oracle_nearest(np.zeros((1, 3), np.float32), t, want_second=True)
    assert d2[0] == 0.25 and idx[0] == 1 and second[0] == 0.25


def _lib():
    import __graft_entry__ as ge
    ge.build()
    from pointdreamer_amd import _lib
    return _lib.lib()


def test_argument_validation_sets_error_message():
    L = _lib()
    one = C.c_void_p(256)                                        # (never dereferenced: the sizes are refused first)
    for args in ((one, -1, one, 5, one, one, one, one, None), (one, 5, one, 0, one, one, one, one, None),
                 (None, 5, one, 5, one, one, one, one, None), (one, 5, None, 5, one, one, one, one, None),
                 (one, 5, one, 5, None, one, one, one, None), (one, 5, one, 5, one, one, None, one, None),
                 (one, 5, one, 5, one, one, one, None, None)):
        assert L.pdhip_nearest_points(*args) == -1
        assert b'pdhip_nearest_points' in L.pdhip_last_error()
    assert L.pdhip_nearest_points(one, 5, one, -3, one, one, one, one, None) == -1 and b'M=-3' in L.pdhip_last_error()
    for args in ((one, one, -1, None, None, 5, one, 10, one, one, one, None), (one, one, 5, None, None, 0, one, 10, one, one, one, None),
                 (one, one, 5, None, None, 5, one, 5000, one, one, one, None), (one, one, 5, None, None, 5, one, -1, one, one, one, None),
                 (None, one, 5, None, None, 5, one, 10, one, one, one, None), (one, one, 5, None, None, 5, None, 10, one, one, one, None),
                 (one, one, 5, None, None, 5, one, 10, None, one, one, None), (one, one, 5, None, None, 5, one, 10, one, None, one, None),
                 (one, one, 5, None, None, 5, one, 10, one, one, None, None)):
        assert L.pdhip_cloud_metrics(*args) == -1
        assert b'pdhip_cloud_metrics' in L.pdhip_last_error()
    assert L.pdhip_nearest_points_stage_chunk() >= 256


def test_product_has_no_cpu_path():
    import torch
    from pointdreamer_amd import _lib, geometry_metrics as G
    x = torch.zeros((4, 3))
    with pytest.raises(_lib.PdhipError):
        G.nearest_points(x, x)
    with pytest.raises(_lib.PdhipError):
        G.eval_pointcloud(x, x)
    with pytest.raises(_lib.PdhipError):
        G.eval_mesh(x, torch.zeros((1, 3), dtype=torch.int64), x, x)
    # the empty prediction never reaches the device (eval.py:103-108)
    assert G.eval_pointcloud(np.empty((0, 3)), x) == G.EMPTY_PCL_DICT
    assert G.eval_pointcloud(np.empty((0, 3)), x, np.empty((0, 3)), x) == dict(G.EMPTY_PCL_DICT, **G.EMPTY_PCL_DICT_NORMALS)


@pytest.mark.parametrize("Q,M", [(5003, 3001), (3001, 5003), (1, 1), (1, 700), (259, 1), (8000, 8000), (4096, 3500), (0, 10), (100000, 100000)])
def test_workspace_size_is_the_carve_of_the_layout(Q, M):
    L = _lib()
    got = L.pdhip_nearest_points_workspace_bytes(Q, M)
    print(Q, M, got, gm.nearest_workspace_bytes(Q, M))
    assert got == gm.nearest_workspace_bytes(Q, M)


def test_workspace_size_refuses_what_the_entry_refuses():
    L = _lib()
    assert L.pdhip_nearest_points_workspace_bytes(5, 0) == 0 and L.pdhip_nearest_points_workspace_bytes(-1, 5) == 0
    assert L.pdhip_cloud_metrics_workspace_bytes(-1) == 0 and L.pdhip_cloud_metrics_workspace_bytes(4097) == 0
    assert L.pdhip_cloud_metrics_workspace_bytes(1000) >= 3 * 256 * 8 + 1001 * 8


def test_no_scratch_on_the_cloud_metrics_kernels():
    if not os.path.exists(LIB):
        _lib()
    pytest.importorskip('msgpack')                          # (as tests/test_code_objects_cpu.py: the metadata note is msgpack)
    from tools import code_object_notes
    shared = ('k_point_box', 'k_cell_keys', 'k_cell_starts', 'k_gather_xyzi', 'k_split_counts')      # csrc/cell_list.h: every including unit's copy is looked at
    mine = [k for k in code_object_notes.kernels(LIB) if 'k_cm_' in k['name'] or 'CmFar' in k['name'] or any(s in k['name'] for s in shared)]
    # (the key of the shared f64 grid, and cell_list.h's far scan pair instantiated with this unit's CmFar: both parts in ONE kernel's name)
    for must in (('k_point_box',), ('k_cell_keys', 'GridPointKey'), ('k_gather_xyzi',), ('k_cell_starts',), ('k_cm_stage_scan',), ('k_cm_ring_scan',),
                 ('k_far_scan', 'CmFar'), ('k_far_pick', 'CmFar'), ('k_split_counts',), ('k_cm_reduce',), ('k_cm_finalize',)):
        assert any(all(m in k['name'] for m in must) for k in mine), must
    for k in mine:
        print(k['name'], 'vgprs', k['vgpr_count'], 'lds', k['group_segment_fixed_size'], 'scratch', k['private_segment_fixed_size'])
        assert k['arch'] == 'gfx950'
        assert k['vgpr_spill_count'] == 0 and k['private_segment_fixed_size'] == 0, k
        if 'k_cm_stage_scan' in k['name'] or ('k_far_scan' in k['name'] and 'CmFar' in k['name']):
            assert k['group_segment_fixed_size'] <= 80 * 1024, k      # at least two workgroups per CU in the 160 KiB
