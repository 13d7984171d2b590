"""Exact k-NN and statistical outlier removal without a GPU: the oracles of tests/knn_common.py against each other and against hand cases, the C ABI
(declared, exported, bound; the size queries), the refusals that come before anything is dereferenced, the refusal of CPU tensors, the demo's opt-in
keys, and zero scratch on the new kernels."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT
import knn_common as kc

LIB = os.path.join(ROOT, 'pointdreamer_amd', 'libpdhip.so')
SYMBOLS = ('pdhip_knn_points_workspace_bytes', 'pdhip_knn_points', 'pdhip_knn_max_k', 'pdhip_knn_lds_bytes', 'pdhip_debug_set_knn',
           'pdhip_sor_filter_workspace_bytes', 'pdhip_sor_filter')
NEAREST = os.path.join(ROOT, 'configs', 'nearest.yaml')
NMAX = 1 << 26


def _lib():
    import __graft_entry__ as ge
    ge.build()
    from pointdreamer_amd import _lib
    return _lib.lib()


# ---- the oracles
def test_stable_argsort_is_the_lexsort_on_a_cloud_full_of_ties():
    p = kc.lattice(4)
    d2, idx = kc.oracle_knn(p, p, 27)
    ld2, lidx = kc.lexsort_knn(p, p, 27)
    assert np.array_equal(idx, lidx) and np.array_equal(d2.view(np.uint64), ld2.view(np.uint64))
    assert np.array_equal(idx[:, 0], np.arange(64)) and np.all(d2[:, 0] == 0.0) and np.all(np.diff(d2, axis=1) >= 0.0)
    ties = d2[:, 1:] == d2[:, :-1]
    assert ties.sum() > 64 * 10 and np.all(np.diff(idx, axis=1)[ties] > 0)        # equal distances: ascending index


def test_oracle_on_hand_cases():
    t = np.array([[0, 0, 0], [1, 0, 0], [0, 2, 0], [1, 0, 0], [0, 0, -3]], np.float32)
    d2, idx = kc.oracle_knn(np.array([[0, 0, 0], [1, 0, 0]], np.float32), t, 4)
    assert d2.tolist() == [[0.0, 1.0, 1.0, 4.0], [0.0, 0.0, 1.0, 5.0]] and idx.tolist() == [[0, 1, 3, 2], [1, 3, 0, 2]]
    d2, idx = kc.oracle_case('identical')
    assert np.all(d2 == 0.0) and np.all(idx == np.arange(10))
    d2, idx = kc.oracle_case('lattice_k7')                         # an interior lattice point: itself and its six face neighbours
    centre = (3 * 8 + 3) * 8 + 3
    assert d2[centre].tolist() == [0.0] + [1.0] * 6 and idx[centre].tolist() == sorted([centre, centre - 1, centre + 1, centre - 8, centre + 8,
                                                                                         centre - 64, centre + 64], key=lambda i: (i != centre, i))


def test_sor_oracle_on_a_hand_case():
    d2 = np.array([[0.0, 1.0, 4.0], [0.0, 1.0, 1.0], [0.0, 4.0, 4.0], [0.0, 100.0, 144.0]])
    o = kc.oracle_sor(d2, 1.0)
    assert o['mean_d'].tolist() == [1.5, 1.0, 2.0, 11.0] and o['mean'] == 3.875
    assert abs(o['std'] - np.std([1.5, 1.0, 2.0, 11.0], ddof=1)) < 1e-15 and o['keep'].tolist() == [True, True, True, False]


def test_the_sor_cloud_is_what_the_gpu_tests_expect():
    """The conditions the GPU test of the mask relies on, asserted on the oracle alone."""
    pts, surf = kc.sor_cloud()
    o = kc.oracle_sor_cloud()
    N = len(pts)
    b_mean, b_stat = kc.sor_bounds(N, kc.SOR_K)
    gap = np.abs(o['mean_d'] - o['threshold']).min()
    print('removed', int((~o['keep']).sum()), 'surface removed', int((~o['keep'] & surf).sum()), 'mean', o['mean'], 'std', o['std'], 'threshold',
          o['threshold'], 'nearest mean_d to it', gap, 'sum of the bounds', (b_mean + b_stat) * o['threshold'])
    assert N == 2032 and surf.sum() == 2000 and pts.dtype == np.float32
    assert (~o['keep']).sum() == 31 and not (~o['keep'] & surf).any()              # 31 of the 32 far points go, no surface point does
    assert abs(o['threshold'] - 0.3113) < 5e-5 and abs(gap - 0.0137) < 5e-5
    assert gap > b_mean * o['mean_d'].max() + b_stat * o['threshold']              # no point within the sum of the two bounds of the threshold


# ---- the C ABI
def test_header_declares_and_library_exports_the_symbols():
    L = _lib()
    from pointdreamer_amd import _lib as lib_mod
    txt = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'pdhip.h')).read(), flags=re.S)
    for s in SYMBOLS:
        assert re.search(r'\b%s\s*\(' % s, txt), f"{s} is not declared in include/pdhip.h"
        assert hasattr(L, s) and s in lib_mod._SIGS, s
    assert len(lib_mod._SIGS['pdhip_knn_points'][1]) == 10 and len(lib_mod._SIGS['pdhip_sor_filter'][1]) == 11
    assert not any(s.endswith('_ws_bytes') for s in SYMBOLS)       # (tests/test_ws_bytes_cpu.py fixes that set)
    assert L.pdhip_knn_max_k() == 64
    assert L.pdhip_knn_lds_bytes(0) == 0 and L.pdhip_knn_lds_bytes(65) == 0
    assert L.pdhip_knn_lds_bytes(21) == 12 * 65 * 21 and L.pdhip_knn_lds_bytes(64) == 12 * 65 * 64 <= 64 * 1024 - 8192


def test_size_queries_refuse_bad_sizes_and_are_monotone():
    L = _lib()
    q = L.pdhip_knn_points_workspace_bytes
    for Q, M, k in ((-1, 10, 1), (NMAX + 1, 10, 1), (10, 0, 1), (10, -3, 1), (10, NMAX + 1, 1), (10, 10, 0), (10, 10, -1), (10, 100, 65), (10, 10, 11)):
        assert q(Q, M, k) == 0, (Q, M, k)
    assert q(0, 1, 1) > 0 and q(NMAX, NMAX, 64) > 0
    sizes = [q(Q, 1000, 8) for Q in (0, 1, 1000, 100000, 1000000, NMAX)]
    assert all(a < b for a, b in zip(sizes, sizes[1:])), sizes
    sizes = [q(1000, M, 8) for M in (8, 1000, 100000, 1000000, NMAX)]
    assert all(a < b for a, b in zip(sizes, sizes[1:])), sizes
    sizes = [q(100000, 100000, k) for k in (1, 2, 21, 63, 64)]
    assert all(a <= b for a, b in zip(sizes, sizes[1:])), sizes
    assert q(1000000, 1000000, 21) < 1000000 * 200                 # sort buffers, two sorted copies, the cell starts: a few dozen bytes per point
    s = L.pdhip_sor_filter_workspace_bytes
    for N in (-1, 0, 1, NMAX + 1):
        assert s(N) == 0, N
    sizes = [s(N) for N in (2, 3000, 100000, 1000000, NMAX)]
    assert sizes[0] > 0 and all(a < b for a, b in zip(sizes, sizes[1:])), sizes


def test_knn_refuses_null_pointers_and_sizes_by_name_before_any_launch():
    L = _lib()
    one = C.c_void_p(256)                                          # (never dereferenced: the arguments are refused first)
    ok = dict(queries=one, Q=5, targets=one, M=12, k=3, d2=one, idx=one, counts=one, ws=one, stream=None)
    order = list(ok)
    call = lambda **kw: L.pdhip_knn_points(*[dict(ok, **kw)[k] for k in order])
    for name in ('queries', 'targets', 'd2', 'idx', 'counts', 'ws'):
        assert call(**{name: None}) == -1
        msg = L.pdhip_last_error()
        assert b'pdhip_knn_points' in msg and b'null pointer' in msg and ('(%s)' % name).encode() in msg, msg
    for kw, word in ((dict(k=0), b'k=0'), (dict(k=-2), b'k=-2'), (dict(k=65, M=100), b'k=65'), (dict(k=13), b'k=13 neighbours of M=12'),
                     (dict(M=0), b'M=0'), (dict(M=NMAX + 1), b'M=67108865'), (dict(Q=-1), b'Q=-1'), (dict(Q=NMAX + 1), b'Q=67108865')):
        assert call(**kw) == -1
        assert b'pdhip_knn_points' in L.pdhip_last_error() and word in L.pdhip_last_error(), (kw, L.pdhip_last_error())


def test_sor_refuses_null_pointers_sizes_and_ratios_by_name_before_any_launch():
    L = _lib()
    one = C.c_void_p(256)
    ok = dict(knn_d2=one, N=50, kk=21, std_ratio=2.0, mean_d=one, stats=one, keep=one, kept_idx=one, counts=one, ws=one, stream=None)
    order = list(ok)
    call = lambda **kw: L.pdhip_sor_filter(*[dict(ok, **kw)[k] for k in order])
    for name in ('knn_d2', 'mean_d', 'stats', 'keep', 'kept_idx', 'counts', 'ws'):
        assert call(**{name: None}) == -1
        msg = L.pdhip_last_error()
        assert b'pdhip_sor_filter' in msg and b'null pointer' in msg and ('(%s)' % name).encode() in msg, msg
    for kw, word in ((dict(N=1), b'N=1'), (dict(N=0), b'N=0'), (dict(N=NMAX + 1), b'N=67108865'), (dict(kk=1), b'kk=1'), (dict(kk=0), b'kk=0'),
                     (dict(kk=65), b'kk=65'), (dict(std_ratio=-0.5), b'std_ratio=-0.5'), (dict(std_ratio=float('nan')), b'std_ratio=nan'),
                     (dict(std_ratio=float('inf')), b'std_ratio=inf')):
        assert call(**kw) == -1
        assert b'pdhip_sor_filter' in L.pdhip_last_error() and word in L.pdhip_last_error(), (kw, L.pdhip_last_error())


def test_debug_hook_returns_the_previous_setting_and_refuses_unknown_values():
    L = _lib()
    assert L.pdhip_debug_set_knn(7, 1) == 0
    assert L.pdhip_debug_set_knn(64, 0) == 4 * 7 + 1
    for cells, path in ((65, 0), (-1, 0), (3, 3), (3, -1)):
        assert L.pdhip_debug_set_knn(cells, path) == -1            # (and nothing changes)
    assert L.pdhip_debug_set_knn(5, 2) == 4 * 64 + 0
    assert L.pdhip_debug_set_knn(0, 0) == 4 * 5 + 2
    assert L.pdhip_debug_set_knn(0, 0) == 0


def test_no_scratch_on_the_new_kernels():
    if not os.path.exists(LIB):
        _lib()
    pytest.importorskip('msgpack')                                 # (as tests/test_code_objects_cpu.py: the metadata note is msgpack)
    from tools import code_object_notes
    # (GridPointKey, k_split_counts: csrc/cell_list.h's key of the shared f64 grid and its counts kernel; every including unit's copy is looked at)
    mine = [k for k in code_object_notes.kernels(LIB)
            if 'k_kn_' in k['name'] or 'k_sor_' in k['name'] or 'GridPointKey' in k['name'] or 'k_split_counts' in k['name']]
    names = ' '.join(k['name'] for k in mine)
    for must in ('k_kn_axis_hist', 'k_kn_ring_scan', 'k_kn_sweep', 'k_split_counts', 'GridPointKey', 'k_sor_check', 'k_sor_mean', 'k_sor_reduce', 'k_sor_finalize', 'k_sor_keep',
                 'k_sor_compact'):
        assert must in names, must
    for k in mine:
        print(k['name'], 'vgprs', k['vgpr_count'], 'lds', k['group_segment_fixed_size'], 'scratch', k['private_segment_fixed_size'])
        assert k['arch'] == 'gfx950'
        assert k['vgpr_spill_count'] == 0 and k['private_segment_fixed_size'] == 0, k
        if 'k_kn_ring_scan' in k['name']:
            assert k['group_segment_fixed_size'] == 0              # the list is dynamic LDS, sized by k
        if 'k_kn_sweep' in k['name']:
            assert k['group_segment_fixed_size'] == 8192           # the staged chunk; the list comes on top


# ---- python
def test_cpu_tensors_are_refused():
    from pointdreamer_amd import outliers
    from pointdreamer_amd._lib import PdhipError
    p, c = torch.rand(50, 3), torch.rand(50, 3)
    with pytest.raises(PdhipError, match='no CPU path'):
        outliers.knn_points(p, p, 3)
    with pytest.raises(PdhipError, match='no CPU path'):
        outliers.statistical_outlier_mask(p)
    with pytest.raises(PdhipError, match='no CPU path'):
        outliers.remove_statistical_outliers(p, c)
    with pytest.raises(PdhipError, match='no CPU path'):
        outliers.sor_filter(torch.rand(50, 21, dtype=torch.float64), 2.0)
    with pytest.raises(PdhipError, match='no CPU path'):
        outliers.knn_points(np.zeros((5, 3), np.float32), np.zeros((5, 3), np.float32), 1)
    assert outliers.MAX_NEIGHBORS == 63


def test_the_product_does_not_import_the_oracle():
    src = open(os.path.join(ROOT, 'pointdreamer_amd', 'outliers.py')).read()
    assert 'oracle' not in src and 'knn_common' not in src


# ---- demo config
def test_demo_accepts_the_outlier_keys_and_validates_them():
    from pointdreamer_amd import demo
    assert demo.OUTLIER_KEYS == ('remove_outliers', 'outlier_neighbors', 'outlier_std_ratio')
    cfg = demo.load_config(NEAREST)
    assert not any(k in cfg for k in demo.OUTLIER_KEYS)            # opt-in: no default is filled in
    cfg = demo.load_config(NEAREST, dict(remove_outliers='statistical'))
    assert cfg.remove_outliers == 'statistical' and 'outlier_neighbors' not in cfg and 'outlier_std_ratio' not in cfg
    cfg = demo.load_config(NEAREST, dict(remove_outliers='statistical', outlier_neighbors=63, outlier_std_ratio=0))
    assert cfg.outlier_neighbors == 63 and cfg.outlier_std_ratio == 0
    assert demo.load_config(NEAREST, dict(remove_outliers='statistical', outlier_neighbors=1, outlier_std_ratio=1.5)).outlier_std_ratio == 1.5
    kw = demo._pipeline_kwargs(cfg)
    assert not any(k in kw for k in demo.OUTLIER_KEYS)
    assert kw == demo._pipeline_kwargs(demo.load_config(NEAREST))
    for bad in (dict(remove_outliers='radius'), dict(remove_outliers=True), dict(remove_outliers='statistical', outlier_neighbors=0),
                dict(remove_outliers='statistical', outlier_neighbors=64), dict(remove_outliers='statistical', outlier_neighbors=2.5),
                dict(remove_outliers='statistical', outlier_neighbors=True), dict(remove_outliers='statistical', outlier_std_ratio=-1.0),
                dict(remove_outliers='statistical', outlier_std_ratio=float('nan')), dict(remove_outliers='statistical', outlier_std_ratio=float('inf')),
                dict(remove_outliers='statistical', outlier_std_ratio='2'), dict(remove_outliers='statistical', outlier_std_ratio=True)):
        with pytest.raises(ValueError, match='outlier'):
            demo.load_config(NEAREST, bad)
    with pytest.raises(KeyError, match='remove_outlier'):
        demo.load_config(NEAREST, dict(remove_outlier='statistical'))


def test_no_shipped_config_sets_the_keys_and_noisy_yaml_parses_as_before():
    import yaml
    from pointdreamer_amd import demo
    d = os.path.join(ROOT, 'configs')
    for f in sorted(os.listdir(d)):
        assert not any(k in demo.load_config(os.path.join(d, f)) for k in demo.OUTLIER_KEYS), f
    noisy = yaml.safe_load(open(os.path.join(d, 'noisy.yaml')))
    assert noisy['input_already_noisy'] is True
    assert 'remove_outliers' in open(os.path.join(d, 'noisy.yaml')).read()         # (the header's comment points at the key)


def test_without_the_key_a_cloud_above_the_limit_is_still_refused(tmp_path, capsys):
    import logging
    from pointdreamer_amd import demo, io_utils
    rng = np.random.default_rng(0)
    pc = str(tmp_path / 'big.ply')
    io_utils.save_colored_pc_ply(rng.random((30001, 3), dtype=np.float32), rng.random((30001, 3), dtype=np.float32), pc)
    cfg = demo.load_config(NEAREST, dict(output_path=str(tmp_path / 'out')))
    with pytest.raises(NotImplementedError):
        demo._load_shape(cfg, pc, 'big_nearest', 'cpu', logging.getLogger('test_knn'))
    said = capsys.readouterr().out
    assert said == f"Point number > 30000! (30001 points)({pc}) \n Please try uniformly subsampling the input point cloud first\n"
    assert not os.path.exists(tmp_path / 'out' / 'big_nearest' / 'input_pc.ply')
    assert not os.path.exists(tmp_path / 'out' / 'big_nearest' / 'others' / 'removed_outliers.ply')
