"""Farthest-point subsampling without a GPU: the brute-force oracle of tests/subsample_common.py against a plain-Python triple loop and against the two
properties the definition implies, the C ABI (declared, exported, bound; the size query), the demo's opt-in keys, and the refusal of CPU tensors."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT
import subsample_common as sc

SYMBOLS = ('pdhip_fps_workspace_bytes', 'pdhip_fps', 'pdhip_owner_mean_colors_workspace_bytes', 'pdhip_owner_mean_colors', 'pdhip_debug_set_fps_cells')
NEAREST = os.path.join(ROOT, 'configs', 'nearest.yaml')


# ---- the oracle
def test_oracle_equals_a_plain_python_triple_loop():
    p = np.random.default_rng(1).random((12, 3), dtype=np.float32)
    p[7] = p[2]                                                    # a duplicate: mind 0, picked last
    idx, d2 = sc.oracle_fps(p, 12, 4)
    lidx, ld2 = sc.loops_fps(p, 12, 4)
    assert np.array_equal(idx, lidx) and np.array_equal(d2.view(np.uint64), ld2.view(np.uint64))
    assert sorted(idx.tolist()) == list(range(12)) and d2[-1] == 0.0 and idx[0] == 4 and np.isinf(d2[0])


def test_oracle_breaks_ties_by_the_smallest_index_and_never_reselects():
    p, M, start = sc.case('identical')
    idx, d2 = sc.oracle_case('identical')
    assert idx.tolist() == list(range(M)) and np.all(d2[1:] == 0.0)
    p, M, start = sc.case('lattice')
    idx, d2, ties = sc.oracle_fps(p, M, start, return_ties=True)
    assert len(set(idx.tolist())) == M and ties > M // 2
    lidx, ld2 = sc.loops_fps(p[:60], 20, 7)                        # ties in the triple loop as well
    oidx, od2 = sc.oracle_fps(p[:60], 20, 7)
    assert np.array_equal(oidx, lidx) and np.array_equal(od2, ld2)


@pytest.mark.parametrize("name", ['plane', 'random', 'clustered'])
def test_oracle_is_monotone_and_prefix_stable(name):
    p, M, start = sc.case(name)
    idx, d2 = sc.oracle_case(name)
    assert np.all(np.diff(d2[1:]) <= 0.0) and len(set(idx.tolist())) == M
    m = M // 3
    pidx, pd2 = sc.oracle_fps(p, m, start)
    assert np.array_equal(pidx, idx[:m]) and np.array_equal(pd2.view(np.uint64), d2[:m].view(np.uint64))


def test_mean_colour_oracle_on_a_hand_case():
    owner = np.array([0, 0, 2, 2, 2], np.int32)
    colors = np.array([[0.0, 1.0, 0.5], [1.0, 1.0, 0.25], [0.25] * 3, [0.5] * 3, [0.75] * 3], np.float32)
    fallback = np.full((3, 3), 0.125, np.float32)
    out = sc.oracle_mean_colors(owner, colors, 3, fallback)
    assert out.dtype == np.float32
    assert np.array_equal(out, np.array([[0.5, 1.0, 0.375], [0.125] * 3, [0.5] * 3], np.float32))


# ---- the C ABI
def test_header_declares_and_library_exports_the_symbols():
    import __graft_entry__ as ge
    ge.build()
    from pointdreamer_amd import _lib
    txt = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'pdhip.h')).read(), flags=re.S)
    L = _lib.lib()
    for s in SYMBOLS:
        assert re.search(r'\b%s\s*\(' % s, txt), f"{s} is not declared in include/pdhip.h"
        assert hasattr(L, s) and s in _lib._SIGS, s
    assert len(_lib._SIGS['pdhip_fps'][1]) == 9 and len(_lib._SIGS['pdhip_owner_mean_colors'][1]) == 8
    assert not any(s.endswith('_ws_bytes') for s in SYMBOLS)       # (tests/test_ws_bytes_cpu.py fixes that set)


def test_workspace_query_refuses_bad_sizes_and_grows_with_n():
    from pointdreamer_amd import _lib
    L = _lib.lib()
    q = L.pdhip_fps_workspace_bytes
    for N, M in ((0, 1), (-5, 1), ((1 << 24) + 1, 10), (10, 0), (10, 11), (10, -1)):
        assert q(N, M) == 0, (N, M)
    sizes = [q(N, min(N, 30000)) for N in (1, 1000, 100000, 1000000, 1 << 24)]
    assert sizes[0] > 0 and all(a < b for a, b in zip(sizes, sizes[1:]))
    assert sizes[-1] < (1 << 24) * 64                              # sort buffers, the sorted copy, mind: a few dozen bytes per point
    assert q(100000, 1) == q(100000, 100000)                       # (a function of N alone)
    assert L.pdhip_debug_set_fps_cells(7) == 0 and L.pdhip_debug_set_fps_cells(0) == 7      # (returns the previous value)
    m = L.pdhip_owner_mean_colors_workspace_bytes
    assert m(0) == 0 and m(-1) == 0 and 0 < m(1) < m(30000)


def test_entries_refuse_null_pointers_and_sizes_before_any_launch():
    from pointdreamer_amd import _lib
    L = _lib.lib()
    one = ctypes.c_void_p(8)                                       # (never dereferenced: the refusals come first)
    for args, word in (((None, 5, 2, 0, one, one, one, one), b'points'), ((one, 5, 2, 0, None, one, one, one), b'idx'),
                       ((one, 5, 2, 0, one, None, one, one), b'min_d2'), ((one, 5, 2, 0, one, one, None, one), b'counts'),
                       ((one, 5, 2, 0, one, one, one, None), b'ws'), ((one, 0, 1, 0, one, one, one, one), b'N=0'),
                       ((one, (1 << 24) + 1, 1, 0, one, one, one, one), b'2^24'), ((one, 5, 0, 0, one, one, one, one), b'M=0'),
                       ((one, 5, 6, 0, one, one, one, one), b'M=6'), ((one, 5, 2, 5, one, one, one, one), b'start=5'),
                       ((one, 5, 2, -1, one, one, one, one), b'start=-1')):
        assert L.pdhip_fps(*args, None) == -1, args
        assert b'pdhip_fps' in L.pdhip_last_error() and word in L.pdhip_last_error(), (word, L.pdhip_last_error())
    for args, word in (((None, one, 5, 2, one, one), b'owner'), ((one, None, 5, 2, one, one), b'colors'), ((one, one, 5, 2, None, one), b'fallback'),
                       ((one, one, 5, 2, one, None), b'out'), ((one, one, -1, 2, one, one), b'N=-1'), ((one, one, 5, 0, one, one), b'M=0')):
        assert L.pdhip_owner_mean_colors(*args, None, None) == -1, args
        assert b'pdhip_owner_mean_colors' in L.pdhip_last_error() and word in L.pdhip_last_error(), (word, L.pdhip_last_error())


# ---- python
def test_cpu_tensors_are_refused():
    from pointdreamer_amd import subsample
    from pointdreamer_amd._lib import PdhipError
    p, c = torch.rand(50, 3), torch.rand(50, 3)
    with pytest.raises(PdhipError, match='no CPU path'):
        subsample.farthest_point_sample(p, 10)
    with pytest.raises(PdhipError, match='no CPU path'):
        subsample.subsample_cloud(p, c, num=10)
    with pytest.raises(PdhipError, match='no CPU path'):
        subsample.subsample_cloud(p, c, num=100)                   # (also when nothing would be subsampled)
    with pytest.raises(ValueError, match='colors_from'):
        subsample.subsample_cloud(p, c, num=10, colors_from='median')


def test_the_product_does_not_import_the_oracle():
    src = open(os.path.join(ROOT, 'pointdreamer_amd', 'subsample.py')).read()
    assert 'oracle' not in src and 'subsample_common' not in src


# ---- demo config
def test_demo_accepts_the_subsample_keys_and_validates_them():
    from pointdreamer_amd import demo
    assert demo.SUBSAMPLE_KEYS == ('subsample', 'subsample_num', 'subsample_colors')
    cfg = demo.load_config(NEAREST)
    assert not any(k in cfg for k in demo.SUBSAMPLE_KEYS)          # opt-in: no default is filled in
    cfg = demo.load_config(NEAREST, dict(subsample='fps'))
    assert cfg.subsample == 'fps' and 'subsample_num' not in cfg and 'subsample_colors' not in cfg
    cfg = demo.load_config(NEAREST, dict(subsample='fps', subsample_num=1, subsample_colors='mean'))
    assert cfg.subsample_num == 1 and cfg.subsample_colors == 'mean'
    assert demo.load_config(NEAREST, dict(subsample='fps', subsample_num=30000, subsample_colors='point')).subsample_num == 30000
    kw = demo._pipeline_kwargs(cfg)
    assert not any(k in kw for k in demo.SUBSAMPLE_KEYS)
    assert kw == demo._pipeline_kwargs(demo.load_config(NEAREST))
    for bad in (dict(subsample='random'), dict(subsample=True), dict(subsample='fps', subsample_num=0), dict(subsample='fps', subsample_num=30001),
                dict(subsample='fps', subsample_num=2.5), dict(subsample='fps', subsample_num=True), dict(subsample='fps', subsample_colors='median')):
        with pytest.raises(ValueError, match='subsample'):
            demo.load_config(NEAREST, bad)
    with pytest.raises(KeyError, match='subsampel'):
        demo.load_config(NEAREST, dict(subsampel='fps'))


def test_no_shipped_config_sets_the_key():
    from pointdreamer_amd import demo
    d = os.path.join(ROOT, 'configs')
    for f in sorted(os.listdir(d)):
        assert not any(k in demo.load_config(os.path.join(d, f)) for k in demo.SUBSAMPLE_KEYS), f


def test_without_the_key_a_cloud_above_the_limit_is_still_refused(tmp_path, capsys):
    import logging
    from pointdreamer_amd import demo, io_utils
    rng = np.random.default_rng(0)
    pc = str(tmp_path / 'big.ply')
    io_utils.save_colored_pc_ply(rng.random((30001, 3), dtype=np.float32), rng.random((30001, 3), dtype=np.float32), pc)
    cfg = demo.load_config(NEAREST, dict(output_path=str(tmp_path / 'out')))
    with pytest.raises(NotImplementedError):
        demo._load_shape(cfg, pc, 'big_nearest', 'cpu', logging.getLogger('test_subsample'))
    said = capsys.readouterr().out
    assert said == f"Point number > 30000! (30001 points)({pc}) \n Please try uniformly subsampling the input point cloud first\n"
    assert not os.path.exists(tmp_path / 'out' / 'big_nearest' / 'input_pc.ply')
