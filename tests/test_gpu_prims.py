"""The shared device primitives, called directly: the LSD radix sort, the one-workgroup k_scan and the tiled scans of csrc/radix_sort.h, and
sort_by_cell with k_cell_starts of csrc/cell_list.h, through the test entries of csrc/prims_debug.hip (that unit's copy of the kernels: the same
source and flags as every consumer's).  Each case is held to an exact numpy reference (tests/prims_common.py, itself checked in
tests/test_prims_cpu.py): integers, np.array_equal, no tolerance.  Every output starts as 0xA5 bytes, the workspace as 0x55 bytes of exactly the
size the query reports.

The sizes are the ones at which these kernels change path: one wave (64), one item round (256), one tile (2048) and one element either side of
each; more than 8192 elements, where the digit histograms outgrow one k_scan chunk per thread (11017: 6 tiles, 300001: 147); key widths with a
partial top digit; 1024 and 1025 tiles of the tiled scan, where the scan of the tile sums goes from one element per thread to two."""
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
