"""The parity variant of the shared union-find (csrc/union_find.h) on the device, through pdhip_debug_parity_union, against the sequential
union-find with parity of tests/mesh_orient_common.py: roots and conflict flags bit for bit, rel[] wherever the class has no conflict (there it is a
function of the pairs alone; in a class with a conflict it depends on which pairs were hooked).  Every call is repeated once."""
import numpy as np
import pytest
import torch

import mesh_orient_common as moc

pytestmark = pytest.mark.gpu
DEV = 'cuda'


def parity_union(n, pairs, parity):
    from pointdreamer_amd import _lib
    from pointdreamer_amd._lib import ptr, stream, check
    L = _lib.lib()
    tp = torch.from_numpy(np.ascontiguousarray(pairs, np.int32)).to(DEV)
    te = torch.from_numpy(np.ascontiguousarray(parity, np.uint8)).to(DEV)
    runs = []
    for _ in range(2):
        word, root = (torch.full((n,), -5, dtype=torch.int32, device=DEV) for _ in range(2))
        rel, conflict = (torch.full((n,), 7, dtype=torch.uint8, device=DEV) for _ in range(2))
        status = torch.full((1,), -5, dtype=torch.int32, device=DEV)
        check(L.pdhip_debug_parity_union(ptr(tp), ptr(te), len(pairs), n, ptr(word), ptr(root), ptr(rel), ptr(conflict), ptr(status), stream()),
              'pdhip_debug_parity_union')
        assert status.item() == 0
        w = word.cpu().numpy()
        assert ((w >> 1) <= np.arange(n)).all() and ((w >> 1) >= 0).all()                  # the forest descends
        runs.append((root.cpu().numpy(), rel.cpu().numpy(), conflict.cpu().numpy()))
    (r0, l0, c0), (r1, l1, c1) = runs
    assert np.array_equal(r0, r1) and np.array_equal(c0, c1) and np.array_equal(l0[c0 == 0], l1[c1 == 0])
    return r0, l0, c0


def check_against_oracle(n, pairs, parity):
    root, rel, conflict = parity_union(n, pairs, parity)
    wr, wl, wc = moc.oracle_parity_union(n, pairs, parity)
    assert root.dtype == np.int32 and np.array_equal(root, wr) and np.array_equal(conflict, wc)
    assert np.array_equal(rel[wc == 0], wl[wc == 0])
    return root, rel, conflict


@pytest.mark.parametrize("order", ["reverse", "random"])
def test_path_of_4096_nodes(order):
    n = 4096
    rng = np.random.default_rng(1)
    parity = rng.integers(0, 2, n - 1).astype(np.uint8)            # pair k joins k and k + 1
    pairs = np.stack([np.arange(n - 1), np.arange(1, n)], 1)
    o = np.arange(n - 2, -1, -1) if order == "reverse" else rng.permutation(n - 1)
    root, rel, conflict = check_against_oracle(n, pairs[o], parity[o])
    assert (root == 0).all() and not conflict.any()
    assert np.array_equal(rel, np.concatenate([[0], np.cumsum(parity) & 1]).astype(np.uint8))


def random_graph(seed=2, n=1000, m=3000):
    rng = np.random.default_rng(seed)
    colour = rng.integers(0, 2, n)
    pairs = rng.integers(0, n, (m, 2))                              # (a pair (a, a) says rel[a] ^ rel[a] == 0: true)
    return n, pairs, colour, (colour[pairs[:, 0]] ^ colour[pairs[:, 1]]).astype(np.uint8)


def test_random_graph_with_a_hidden_colouring_has_no_conflict():
    n, pairs, colour, parity = random_graph()
    root, rel, conflict = check_against_oracle(n, pairs, parity)
    assert not conflict.any() and np.array_equal(rel, (colour ^ colour[root]).astype(np.uint8))
    assert len(np.unique(root)) < 50


def test_one_toggled_parity_on_a_cycle_flags_that_component_only():
    n, pairs, colour, parity = random_graph()
    lone = np.array([[n, n + 1], [n + 1, n + 2]])                   # a second component: a path of three nodes of its own
    pairs, parity = np.concatenate([pairs, lone]), np.concatenate([parity, [1, 0]]).astype(np.uint8)
    root0 = moc.oracle_parity_union(n + 3, pairs, parity)[0]
    big = np.flatnonzero(root0 == root0[pairs[0, 0]])
    assert len(big) > 900
    # an edge that lies on a cycle: its ends stay connected without it
    for k in range(len(pairs) - 2):
        rest = np.delete(np.arange(len(pairs)), k)
        r = moc.oracle_parity_union(n + 3, pairs[rest], parity[rest])[0]
        if r[pairs[k, 0]] == r[pairs[k, 1]]:
            break
    toggled = parity.copy()
    toggled[k] ^= 1
    root, rel, conflict = check_against_oracle(n + 3, pairs, toggled)
    assert np.array_equal(np.flatnonzero(conflict), big) and conflict[n:].tolist() == [0, 0, 0] and rel[n:].tolist() == [0, 1, 1]


@pytest.mark.parametrize("k", [3, 4, 5])
def test_cycles_odd_and_even(k):
    cyc = np.stack([np.arange(k), (np.arange(k) + 1) % k], 1)
    root, rel, conflict = check_against_oracle(k, cyc, np.ones(k, np.uint8))
    assert (root == 0).all() and conflict.tolist() == [k % 2] * k
    if k == 4:
        assert rel.tolist() == [0, 1, 0, 1]
    _, _, conflict = check_against_oracle(k, cyc, np.zeros(k, np.uint8))
    assert not conflict.any()
