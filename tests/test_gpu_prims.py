"""The shared device primitives, called directly: the LSD radix sort, the one-workgroup k_scan and the tiled scans of csrc/radix_sort.h, and
sort_by_cell with k_cell_starts of csrc/cell_list.h, through the test entries of csrc/prims_debug.hip (that unit's copy of the kernels: the same
source and flags as every consumer's).  Each case is held to an exact numpy reference (tests/prims_common.py, itself checked in
tests/test_prims_cpu.py): integers, np.array_equal, no tolerance.  Every output starts as 0xA5 bytes, the workspace as 0x55 bytes of exactly the
size the query reports.

The sizes are the ones at which these kernels change path: one wave (64), one item round (256), one tile (2048) and one element either side of
each; more than 8192 elements, where the digit histograms outgrow one k_scan chunk per thread (11017: 6 tiles, 300001: 147); key widths with a
partial top digit; 1024 and 1025 tiles of the tiled scan, where the scan of the tile sums goes from one element per thread to two.

The union-find of csrc/union_find.h (find_root, unite, walk_root, k_uf_identity) is held to a sequential union-find: chains of 4096 in three
orders (the longest walks), stars onto the first and the last vertex (every CAS meets one root), repeated pairs, a random graph, and 255 / 256 /
257 pairs, the workgroup edge of the one-thread-per-pair launch."""
import numpy as np
import pytest
import torch

import prims_common as pc

DEV = 'cuda:0'
pytestmark = pytest.mark.gpu
NP = {'int': np.int32, 'uint64': np.uint64}
PAD = 64                                                           # elements allocated behind out[n): they keep the sentinel


@pytest.fixture(scope="module")
def pd():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from pointdreamer_amd import _lib
    return dict(lib=_lib, L=_lib.lib())


def dev(a):
    """numpy -> device, bytes unchanged (torch has no uint64 arithmetic: the arrays travel as int64 / int32 and come back as views)."""
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a).to(DEV)


def sentinel(n, dtype):
    return torch.full((n * np.dtype(dtype).itemsize,), pc.SENTINEL, dtype=torch.uint8, device=DEV)


def host(t, dtype):
    return t.cpu().numpy().view(dtype)


def workspace(pd, n, nc):
    nbytes = pd['L'].pdhip_debug_prims_workspace_bytes(n, nc)
    assert nbytes > 0
    return torch.full((nbytes,), pc.WS_FILL, dtype=torch.uint8, device=DEV)


def ok(pd, rc):
    assert rc == 0, (rc, pd['L'].pdhip_last_error())


# ---- radix sort
def run_sort(pd, keys, vals, bits):
    P, S, n = pd['lib'].ptr, pd['lib'].stream, len(keys)
    k, v, ws = dev(keys), dev(vals), workspace(pd, n, 1)
    ko, vo = sentinel(n + PAD, np.uint64), sentinel(n + PAD, np.int32)
    ok(pd, pd['L'].pdhip_debug_radix_sort(P(k), P(v), n, bits, P(ko), P(vo), P(ws), S()))
    ko, vo = host(ko, np.uint64), host(vo, np.int32)
    assert np.all(ko[n:].view(np.uint8) == pc.SENTINEL) and np.all(vo[n:].view(np.uint8) == pc.SENTINEL), "written behind keys_out / vals_out"
    return ko[:n], vo[:n]


@pytest.mark.parametrize("name,n,bits", pc.SORT_CASES, ids=[f"{g}-n{n}-b{b}" for g, n, b in pc.SORT_CASES])
def test_radix_sort(pd, name, n, bits):
    keys = pc.gen_keys(name, n, bits)
    vals = pc.gen_vals(keys, bits)
    ko, vo = run_sort(pd, keys, vals, bits)
    pc.check_sort(keys, vals, bits, ko, vo)
    ko2, vo2 = run_sort(pd, keys, vals, bits)
    assert ko2.tobytes() == ko.tobytes() and vo2.tobytes() == vo.tobytes(), "a second call gave other bytes"


# ---- sort_by_cell
@pytest.mark.parametrize("name,n,nc", pc.CELL_CASES, ids=[f"{s}-n{n}-nc{nc}" for s, n, nc in pc.CELL_CASES])
def test_sort_by_cell(pd, name, n, nc):
    P, S = pd['lib'].ptr, pd['lib'].stream
    keys = pc.cell_keys(name, n, nc)
    k, ws = dev(keys), workspace(pd, n, nc)
    ko, io, cs = sentinel(n + PAD, np.uint64), sentinel(n + PAD, np.int32), sentinel(nc + 1 + PAD, np.int32)
    ok(pd, pd['L'].pdhip_debug_sort_by_cell(P(k), n, nc, P(ko), P(io), P(cs), P(ws), S()))
    ko, io, cs = host(ko, np.uint64), host(io, np.int32), host(cs, np.int32)
    for o, m in ((ko, n), (io, n), (cs, nc + 1)):
        assert np.all(o[m:].view(np.uint8) == pc.SENTINEL), "written behind an output"
    pc.check_sort_by_cell(keys, nc, ko[:n], io[:n], cs[:nc + 1])


# ---- scans
def run_scan(pd, x, mode, inclusive):
    P, S, n = pd['lib'].ptr, pd['lib'].stream, len(x)
    xi, ws = dev(x), workspace(pd, n, 1)
    out = sentinel(n + PAD, x.dtype)
    ok(pd, pd['L'].pdhip_debug_scan(P(xi), P(out), n, x.dtype.itemsize, mode, inclusive, 1, P(ws), S()))
    out = host(out, x.dtype)
    assert np.all(out[n:].view(np.uint8) == pc.SENTINEL), f"the element just past n = {n} lost its sentinel: {out[n:n + 2]}"
    pc.check_scan(x, inclusive, out[:n])


@pytest.mark.parametrize("n", pc.KSCAN_SIZES)
@pytest.mark.parametrize("elem,inclusive", pc.SCAN_FORMS, ids=[f"{e}-{'incl' if i else 'excl'}" for e, i in pc.SCAN_FORMS])
def test_one_workgroup_scan(pd, elem, inclusive, n):
    for x in pc.scan_inputs(elem, n, tiled=False).values():
        assert x.dtype == NP[elem]
        run_scan(pd, x, 0, inclusive)


TILED_CASES = [(e, i, n) for e, i in pc.SCAN_FORMS for n in pc.TILED_SIZES if n not in pc.TILED_LARGE or (e, i) in (('int', 0), ('uint64', 1))]


@pytest.mark.parametrize("elem,inclusive,n", TILED_CASES, ids=[f"{e}-{'incl' if i else 'excl'}-n{n}" for e, i, n in TILED_CASES])
def test_tiled_scan(pd, elem, inclusive, n):
    for x in pc.scan_inputs(elem, n, tiled=True).values():
        assert x.dtype == NP[elem]
        run_scan(pd, x, 1, inclusive)


# ---- the union-find of csrc/union_find.h: k_uf_identity, unite(find_root, find_root) per pair, walk_root per vertex
def run_union(pd, n, pairs):
    P, S = pd['lib'].ptr, pd['lib'].stream
    p = dev(pairs) if len(pairs) else None
    parent, root, status = sentinel(n + PAD, np.int32), sentinel(n + PAD, np.int32), sentinel(1 + PAD, np.int32)
    rc = pd['L'].pdhip_debug_union_pairs(P(p, allow_none=True), len(pairs), n, P(parent), P(root), P(status), S())
    parent, root, status = host(parent, np.int32), host(root, np.int32), host(status, np.int32)
    for o, m in ((parent, n), (root, n), (status, 1)):
        assert np.all(o[m:].view(np.uint8) == pc.SENTINEL), "written behind an output"
    return rc, parent[:n], root[:n], int(status[0])


@pytest.mark.parametrize("name", pc.UNION_CASES)
def test_union_pairs(pd, name):
    n, pairs = pc.union_case(name)
    rc, parent, root, status = run_union(pd, n, pairs)
    ok(pd, rc)
    assert status == 0, f"a budget ran out (status {status})"
    pc.check_equal(root, pc.ref_union(n, pairs), f"union-find roots ({name}, n={n}, {len(pairs)} pairs)")
    assert np.all(parent <= np.arange(n)), "parent[v] > v: the forest does not descend"
    assert np.array_equal(root[parent], root), "a vertex and its parent in different classes"


def test_union_pairs_refuses_an_index_outside(pd):
    n, pairs = pc.union_case('pairs_257')
    for where, value in ((0, -1), (256, n), (100, 1 << 30)):
        bad = pairs.copy()
        bad[where, 1] = value
        rc, parent, _, _ = run_union(pd, n, bad)
        assert rc == -1 and b'outside [0, n=600)' in pd['L'].pdhip_last_error() and b'1 pair(s)' in pd['L'].pdhip_last_error()
        assert np.all(parent.view(np.uint8) == pc.SENTINEL), "parent was touched before the refusal"
