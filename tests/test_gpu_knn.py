"""Exact k nearest neighbours on the device (csrc/knn.hip, pointdreamer_amd/outliers.py: knn_points).  pdhip_knn_points is held to BIT EQUALITY with
the all-pairs float64 oracle of tests/knn_common.py (d2 as uint64, idx exactly) on every path: the k smallest (d2, index) pairs under the
lexicographic order, and their ascending order, depend on neither the order the targets are visited in nor the grid."""
import numpy as np
import pytest
import torch

import knn_common as kc

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
SENT_D2, SENT_IDX, SENT_CNT = -7.0, -77, -777


def T(a):
    return torch.from_numpy(np.array(a)).to(DEV)                  # (a writable copy: the cached clouds are read-only)


@pytest.fixture(autouse=True)
def restore_the_hook():
    from pointdreamer_amd import _lib
    yield
    assert _lib.lib().pdhip_debug_set_knn(0, 0) >= 0


def run_knn(q, t, k, hook=(0, 0), null=None, Q=None, M=None, ws=None):
    """(rc, d2 [Q,k], idx [Q,k], counts) of pdhip_knn_points under pdhip_debug_set_knn(*hook); the outputs start as sentinels.  null: the name of an
    argument passed as NULL.  Q / M: the sizes passed, when they are not the arrays' own.  ws: the workspace to use instead of a fresh torch.empty one."""
    from pointdreamer_amd import _lib
    from pointdreamer_amd._lib import ptr, stream
    L = _lib.lib()
    tq, tt = T(np.asarray(q, np.float32).reshape(-1, 3)), T(np.asarray(t, np.float32).reshape(-1, 3))
    rows = tq.shape[0]
    Q = rows if Q is None else Q
    M = tt.shape[0] if M is None else M
    cols = max(min(k, 64), 1)
    d2 = torch.full((max(rows, 1), cols), SENT_D2, dtype=torch.float64, device=DEV)
    idx = torch.full((max(rows, 1), cols), SENT_IDX, dtype=torch.int32, device=DEV)
    counts = torch.full((4,), SENT_CNT, dtype=torch.int32, device=DEV)
    if ws is None:
        ws = torch.empty((max(L.pdhip_knn_points_workspace_bytes(Q, M, k), 8),), dtype=torch.uint8, device=DEV)
    a = dict(queries=ptr(tq) if rows else None, targets=ptr(tt), d2=ptr(d2), idx=ptr(idx), counts=ptr(counts), ws=ptr(ws))
    if null is not None:
        a[null] = None
    assert L.pdhip_debug_set_knn(*hook) >= 0
    rc = L.pdhip_knn_points(a['queries'], Q, a['targets'], M, k, a['d2'], a['idx'], a['counts'], a['ws'], stream())
    torch.cuda.synchronize()
    L.pdhip_debug_set_knn(0, 0)
    return rc, d2.cpu().numpy()[:rows], idx.cpu().numpy()[:rows], counts.cpu().numpy()


def check_case(name, hook=None):
    q, t, k, case_hook = kc.case(name)
    od2, oidx = kc.oracle_case(name)
    rc, d2, idx, counts = run_knn(q, t, k, case_hook if hook is None else hook)
    assert rc == 0
    print(name, 'Q', len(q), 'M', len(t), 'k', k, 'hook', case_hook if hook is None else hook, 'counts', counts.tolist(), 'd2 unequal',
          int((d2.view(np.uint64) != od2.view(np.uint64)).sum()), 'idx unequal', int((idx != oidx).sum()))
    assert np.array_equal(d2.view(np.uint64), od2.view(np.uint64))
    assert np.array_equal(idx, oidx)
    assert counts[0] + counts[1] == len(q) and counts[0] >= 0 and counts[1] >= 0 and 1 <= counts[2] <= 128 and counts[3] == 0
    return d2, idx, counts


# ---- bit equality
@pytest.mark.parametrize("name", kc.CASES)
def test_rows_equal_the_oracle_bit_for_bit(name):
    q, t, k, hook = kc.case(name)
    d2, idx, counts = check_case(name)
    if name == 'random_k64':
        from pointdreamer_amd import _lib
        assert k == _lib.lib().pdhip_knn_max_k()
    if name == 'k_eq_m':
        assert k == len(t) and counts[2] == 7                      # k == M: only the cube that covers the grid ends the scan
        assert np.array_equal(np.sort(idx, axis=1), np.tile(np.arange(k, dtype=np.int32), (len(q), 1)))
    if name in ('one_target', 'identical'):
        assert counts[2] == 1                                      # a box without extent: one cell
    if name == 'identical':
        assert np.all(idx == np.arange(k)) and np.all(d2 == 0.0)
    if name == 'ring_growth':
        assert counts[2] == 32 and counts[1] > 0                   # the first cubes hold fewer than k targets; most queries pass the last ring
    if name == 'ring_growth16':
        assert counts[2] == 16 and counts[0] > len(q) // 2         # the rings grow until the certificate holds
    if name == 'far':
        assert counts[1] > 0                                       # far from every target: the sweep
    if name == 'crowded_box':
        assert counts[1] > 0                                       # more than the work limit in the first rings: the sweep
    if name == 'crowded':
        assert counts[0] > 0.9 * len(q)                            # the shipped grid spans the cluster, not the 20 targets elsewhere
    if name == 'dup_boundary':
        n = len(t) // 2
        assert np.all(d2[:, 0] == 0.0) and np.all(d2[:, 1] == 0.0) and np.array_equal(idx[:n, :2], idx[n:, :2])    # a point and its copy, in index order


def test_k1_gives_the_bytes_of_nearest_points():
    from pointdreamer_amd import geometry_metrics as G, outliers
    q, t, k, _ = kc.case('random_k1')
    d2, idx = outliers.knn_points(T(q), T(t), 1)
    nd2, nidx = G.nearest_points(T(q), T(t))
    assert d2.shape == (len(q), 1) and idx.shape == (len(q), 1) and d2.dtype == torch.float64 and idx.dtype == torch.int32
    assert torch.equal(d2[:, 0].view(torch.int64), nd2.view(torch.int64)) and torch.equal(idx[:, 0], nidx)
    assert np.array_equal(idx.cpu().numpy(), kc.oracle_case('random_k1')[1])


# ---- every path and grid gives the same bytes
@pytest.mark.parametrize("name", ['paths', 'lattice_k27', 'far', 'crowded', 'dup_boundary'])
def test_forced_paths_and_grids_give_equal_bytes(name):
    for hook in ((0, 0), (0, 1), (0, 2), (1, 0), (2, 0), (7, 0), (1, 1), (7, 1), (7, 2), (64, 0)):
        d2, idx, counts = check_case(name, hook)
        if hook[1] == 1:
            assert counts[0] == 0 and counts[1] == len(d2)         # every query through the sweep
        if hook[0]:
            assert counts[2] in (hook[0], 1)
        if hook == (1, 0):
            assert counts[1] == 0 or name == 'crowded'             # one cell: the cube covers the grid at once (5 020 targets pass the work limit)
        if hook == (0, 2) and name == 'crowded':
            assert counts[1] > 0                                   # the grid over the whole box: crowded cells


# ---- invariance, repeats
def test_permuted_queries_give_permuted_rows():
    q, t, k, _ = kc.case('paths')
    od2, oidx = kc.oracle_case('paths')
    perm = np.random.default_rng(3).permutation(len(q))
    rc, d2, idx, _ = run_knn(q[perm], t, k)
    assert rc == 0 and np.array_equal(d2.view(np.uint64), od2[perm].view(np.uint64)) and np.array_equal(idx, oidx[perm])


def test_permuted_targets_keep_the_distances_and_remap_the_indices():
    q, t, k, _ = kc.case('paths')
    od2, oidx = kc.oracle_case('paths')
    assert np.all(np.diff(od2, axis=1) > 0.0)                      # tie-free: the rows are then a function of the SET of targets
    perm = np.random.default_rng(4).permutation(len(t))
    rc, d2, idx, _ = run_knn(q, t[perm], k)
    assert rc == 0 and np.array_equal(d2.view(np.uint64), od2.view(np.uint64)) and np.array_equal(perm[idx], oidx)


@pytest.mark.parametrize("name", ['surface_k21', 'crowded'])
def test_two_calls_give_equal_bytes(name):
    q, t, k, hook = kc.case(name)
    a, b = run_knn(q, t, k, hook), run_knn(q, t, k, hook)
    assert a[0] == 0 and b[0] == 0
    for x, y in zip(a[1:], b[1:]):
        assert x.tobytes() == y.tobytes()


def test_no_queries_zero_the_counts():
    rc, d2, idx, counts = run_knn(np.zeros((0, 3), np.float32), kc.case('paths')[1], 5)
    assert rc == 0 and counts.tolist() == [0, 0, 0, 0]


# ---- refusals leave the outputs untouched
def untouched(d2, idx, counts):
    return np.all(d2 == SENT_D2) and np.all(idx == SENT_IDX) and np.all(counts == SENT_CNT)


@pytest.mark.parametrize("null", ['queries', 'targets', 'd2', 'idx', 'counts', 'ws'])
def test_refuses_a_null_pointer_by_name(null):
    from pointdreamer_amd import _lib
    q, t, k, _ = kc.case('q65')
    rc, d2, idx, counts = run_knn(q, t, k, null=null)
    assert rc == -1 and b'null pointer (%s)' % null.encode() in _lib.lib().pdhip_last_error() and untouched(d2, idx, counts)


@pytest.mark.parametrize("k,Q,M,word", [(0, None, None, b'k=0'), (65, None, None, b'k=65'), (5, None, 4, b'k=5 neighbours of M=4'),
                                        (5, None, 0, b'M=0'), (5, -1, None, b'Q=-1'), (5, (1 << 26) + 1, None, b'Q=67108865')])
def test_refuses_bad_sizes(k, Q, M, word):
    from pointdreamer_amd import _lib
    q, t, _, _ = kc.case('q65')
    rc, d2, idx, counts = run_knn(q, t, k, Q=Q, M=M)               # (refused before any launch: the buffers are never read)
    assert rc == -1 and word in _lib.lib().pdhip_last_error() and untouched(d2, idx, counts)


@pytest.mark.parametrize("bad", [float('nan'), float('inf'), float('-inf')])
@pytest.mark.parametrize("which", ['query', 'target'])
def test_refuses_a_non_finite_coordinate(which, bad):
    from pointdreamer_amd import _lib, outliers
    q, t, k, _ = kc.case('q129')
    q, t = np.array(q), np.array(t)
    (q if which == 'query' else t)[[3, 100], [1, 2]] = bad
    rc, d2, idx, counts = run_knn(q, t, k)
    word = b'2 query point(s)' if which == 'query' else b'2 target(s)'
    assert rc == -1 and word in _lib.lib().pdhip_last_error() and b'non-finite' in _lib.lib().pdhip_last_error() and untouched(d2, idx, counts)
    with pytest.raises(_lib.PdhipError, match='non-finite'):
        outliers.knn_points(T(q), T(t), k)


def test_wrapper_refuses_k_above_the_targets_and_returns_counts():
    from pointdreamer_amd import _lib, outliers
    q, t, k, _ = kc.case('q65')
    with pytest.raises(_lib.PdhipError, match='k=1501'):
        outliers.knn_points(T(q), T(t), len(t) + 1)
    with pytest.raises(_lib.PdhipError, match='k=0'):
        outliers.knn_points(T(q), T(t), 0)
    d2, idx, counts = outliers.knn_points(T(q), T(t), k, return_counts=True)
    assert np.array_equal(idx.cpu().numpy(), kc.oracle_case('q65')[1]) and int(counts[0] + counts[1]) == len(q)
