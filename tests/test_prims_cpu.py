"""The shared device primitives without a GPU: the references of tests/prims_common.py against slower independent ones, the checkers shown to
fail on the faults they are there for, the key generators' promises, the union-find's reference and cases, the size query
pdhip_debug_prims_workspace_bytes and the refusals of the four test entries (include/pdhip.h; they return before any HIP call).
tests/test_gpu_prims.py runs the kernels."""
import ctypes

import numpy as np
import pytest

import prims_common as pc
import workspace_common as wc

M64 = (1 << 64) - 1


@pytest.fixture(scope="module")
def L():
    from pointdreamer_amd import _lib
    return _lib.lib()


# ---- the references against slower independent ones
@pytest.mark.parametrize("name,bits", [(g, b) for g in pc.GENERATORS for b in (19, 45)] + [('uniform', b) for b in pc.SORT_BITS])
def test_sort_reference_against_python_sorted(name, bits):
    for n in (1, 2, 65, 300):
        keys = pc.gen_keys(name, n, bits)
        vals = pc.gen_vals(keys, bits)
        width = 8 * ((bits + 7) // 8)
        order = sorted(range(n), key=lambda i: int(keys[i]) % (1 << width))        # (Python's sort is stable; bits == 0: every key 0, the identity)
        k, v = pc.ref_sort(keys, vals, bits)
        assert [int(x) for x in k] == [int(keys[i]) for i in order]
        assert [int(x) for x in v] == [int(vals[i]) for i in order]


def test_sort_reference_orders_by_whole_digits_and_keeps_the_bits_above():
    keys = np.array([0b1_0000_0001, 0b0_1000_0000, 0b1_0000_0000 | (1 << 40), 0b0_0000_0001], np.uint64)
    k, v = pc.ref_sort(keys, np.arange(4, dtype=np.int32), 7)      # 7 bits: one digit, bit 7 takes part, bits 8 and 40 do not
    assert v.tolist() == [2, 0, 3, 1] and k.tolist() == keys[[2, 0, 3, 1]].tolist()
    k, v = pc.ref_sort(keys, np.arange(4, dtype=np.int32), 9)      # two digits: bit 8 takes part, bit 40 does not
    assert v.tolist() == [3, 1, 2, 0]
    assert pc.ref_sort(keys, np.arange(4, dtype=np.int32), 0)[1].tolist() == [0, 1, 2, 3]
    assert pc.ref_sort(keys, np.arange(4, dtype=np.int32), 64)[1].tolist() == [3, 1, 0, 2]


@pytest.mark.parametrize("n", [1, 2, 7, 300])
def test_scan_references_against_python_integers(n):
    rng = np.random.default_rng(n)
    cases = [rng.integers(0, 4, n).astype(np.int32), rng.integers(0, 1 << 40, n, dtype=np.uint64),
             np.full(n, (1 << 62) + 12345, np.uint64)]             # the running sum passes 2^63 at the second element and 2^64 at the fourth
    for x in cases:
        run, inc, exc = 0, [], []
        for a in x.tolist():
            exc.append(run & M64)
            run += a
            inc.append(run & M64)
        if n >= 4 and x.dtype == np.uint64 and int(x[0]) > 1 << 62:
            assert inc[1] > 1 << 63 and run > M64
        assert [int(a) for a in pc.ref_scan(x, True)] == inc
        assert [int(a) for a in pc.ref_scan(x, False)] == exc
    with pytest.raises(AssertionError, match='does not fit'):
        pc.ref_scan(np.full(3, (1 << 30) + 1, np.int32), True)


def test_cell_start_reference_against_a_count():
    for name, n, nc in [c for c in pc.CELL_CASES if c[1] <= 4097 and c[2] <= 300]:
        keys = pc.cell_keys(name, n, nc)
        k, idx, cstart = pc.ref_sort_by_cell(keys, nc)
        assert cstart.tolist() == [int((keys < c).sum()) for c in range(nc + 1)]
        assert k.tolist() == sorted(keys.tolist()) and keys[idx].tolist() == k.tolist()
        same = k[1:] == k[:-1]
        assert np.all(idx[1:][same] > idx[:-1][same])             # equal keys keep the points' order


# ---- the generators keep their promises
@pytest.mark.parametrize("bits", [19, 45])
def test_generators(bits):
    n, sb = 11017, pc.sorted_bits(bits)
    for name in pc.GENERATORS:
        k = pc.gen_keys(name, n, bits)
        assert np.array_equal(k, pc.gen_keys(name, n, bits))      # seeded
        if name != 'above_bits':
            assert int(k.max()) < 1 << bits, name
    assert len(np.unique(pc.gen_keys('equal', n, bits))) == 1
    frac = np.unique(pc.gen_keys('two_values', n, bits), return_counts=True)[1] / n
    assert len(frac) == 2 and 0.07 < frac.min() < 0.13
    assert np.all(np.diff(pc.gen_keys('sorted', n, bits).astype(np.int64)) >= 0)
    assert np.all(np.diff(pc.gen_keys('reversed', n, bits).astype(np.int64)) <= 0)
    top = pc.gen_keys('top_byte_only', n, bits)
    d = (bits - 1) // 8
    assert len(np.unique(top & np.uint64((1 << 8 * d) - 1))) == 1 and len(np.unique(top >> np.uint64(8 * d))) > 4
    dg = pc.gen_keys('digits_0_255', n, bits)
    for j in range(d):
        assert set(np.unique((dg >> np.uint64(8 * j)) & np.uint64(255)).tolist()) == {0, 255}
    assert set(np.unique(dg >> np.uint64(8 * d)).tolist()) == {0, (1 << (bits - 8 * d)) - 1}
    wu = pc.gen_keys('wave_uniform', n, bits)
    assert all(len(np.unique(wu[i:i + 64])) == 1 for i in range(0, n, 64))
    wd = pc.gen_keys('wave_distinct', n, bits) & np.uint64(255)
    assert all(len(np.unique(wd[i:i + 64])) == len(wd[i:i + 64]) for i in range(0, n, 64))
    ab = pc.gen_keys('above_bits', n, bits)
    assert len(np.unique((ab >> np.uint64(bits)) & np.uint64((1 << (sb - bits)) - 1))) == 1 << (sb - bits)        # every pattern of the partial digit's top
    assert len(np.unique(ab >> np.uint64(sb))) > n // 2                                                             # and bits above the last digit
    ko, vo = pc.ref_sort(ab, pc.gen_vals(ab, bits), bits)
    assert np.any(np.diff((ko & np.uint64((1 << bits) - 1)).astype(np.int64)) < 0)            # the order is NOT the order by [0, bits)
    assert np.array_equal(np.sort(ko), np.sort(ab))


def test_values_carry_the_two_negative_slots_on_repeated_keys():
    for name, n, bits in pc.SORT_CASES:
        if n > 11017:
            continue
        keys = pc.gen_keys(name, n, bits)
        vals = pc.gen_vals(keys, bits)
        assert vals.dtype == np.int32 and (vals == pc.INT32_MIN).sum() == 1 and (vals == -1).sum() == (n > 1)
        rest = np.sort(vals[vals >= 0])
        assert len(rest) == n - 1 - (n > 1) and len(np.unique(rest)) == len(rest) and (n < 3 or rest[-1] < n)
        masked = keys & (pc.sort_mask(bits) if bits else np.uint64(0))
        if n - len(np.unique(masked)) >= 2 or (n >= 2 and len(np.unique(masked)) == 1):
            for s in np.flatnonzero(vals < 0):
                assert (masked == masked[s]).sum() > 1, (name, n, bits)


def test_case_tables_are_what_the_gpu_file_runs():
    assert len(pc.SORT_CASES) == 15 * 2 + 11 + 10 * 2 and len(set(pc.SORT_CASES)) == len(pc.SORT_CASES)
    assert len(pc.CELL_CASES) == 6 * 5 - 2                         # ('outside' needs nc > 1)
    assert len(pc.KSCAN_SIZES) == 10 and len(pc.TILED_SIZES) == 12 and pc.TILED_LARGE == (2048 * 1024, 2048 * 1025 + 3)
    f = pc.scan_inputs('int', 6145, True)['tile_edge_flags']
    assert np.flatnonzero(f).tolist() == [0, 2047, 2048, 4095, 4096, 6143, 6144]
    u = pc.scan_inputs('uint64', 6145, True)
    assert set(u) == {'random_2_40', 'all_2_32_minus_1'}
    inc = pc.ref_scan(u['random_2_40'], True)
    assert int(inc[2047]) > 1 << 32 or (int(inc[2048]) < 1 << 32 < int(inc[4095]))            # the sum passes 2^32 no later than in the second tile


# ---- the checkers can fail: each input is the correct answer with ONE fault
def test_checker_sees_two_equal_keys_swapped():
    keys = pc.gen_keys('two_values', 300, 19)
    vals = pc.gen_vals(keys, 19)
    k, v = pc.ref_sort(keys, vals, 19)
    pc.check_sort(keys, vals, 19, k, v)
    i = int(np.flatnonzero(k[1:] == k[:-1])[5])
    v2 = v.copy()
    v2[[i, i + 1]] = v[[i + 1, i]]
    with pytest.raises(AssertionError, match=rf'values .*first at index {i} \(tile 0, position {i}\)'):
        pc.check_sort(keys, vals, 19, k, v2)


def test_checker_sees_a_cleared_bit_above_the_sorted_width():
    keys = pc.gen_keys('above_bits', 4097, 19)
    vals = pc.gen_vals(keys, 19)
    k, v = pc.ref_sort(keys, vals, 19)
    i = int(np.flatnonzero(k[2048:] >> np.uint64(40) & np.uint64(1))[0]) + 2048
    k2 = k.copy()
    k2[i] &= ~np.uint64(1 << 40)
    with pytest.raises(AssertionError, match=rf'keys .*1 of 4097 .*index {i} \(tile 1, position {i - 2048}\)'):
        pc.check_sort(keys, vals, 19, k2, v)


@pytest.mark.parametrize("elem", ['int', 'uint64'])
def test_checker_sees_a_scan_without_the_first_tile_sum(elem):
    x = pc.scan_inputs(elem, 4097, True)['random_0_3' if elem == 'int' else 'random_2_40']
    for inclusive in (0, 1):
        out = pc.ref_scan(x, inclusive)
        pc.check_scan(x, inclusive, out)
        bad = out.copy()
        bad[2048:] -= x[:2048].sum(dtype=x.dtype)
        with pytest.raises(AssertionError, match=r'2049 of 4097 .*index 2048 \(tile 1, position 0\)'):
            pc.check_scan(x, inclusive, bad)


def test_checker_sees_inclusive_for_exclusive():
    x = pc.scan_inputs('int', 2049, False)['ones']
    with pytest.raises(AssertionError, match=r'exclusive .*index 0 \(tile 0, position 0\)'):
        pc.check_scan(x, 0, pc.ref_scan(x, 1))
    with pytest.raises(AssertionError, match='inclusive'):
        pc.check_scan(x, 1, pc.ref_scan(x, 0))


def test_checker_sees_cstart_off_by_one_in_an_empty_cell():
    keys = pc.cell_keys('third_empty', 4097, 300)
    k, idx, cstart = pc.ref_sort_by_cell(keys, 300)
    pc.check_sort_by_cell(keys, 300, k, idx, cstart)
    empty = 149                                                    # (149 % 3 == 2: an empty cell between two cells that hold points)
    assert cstart[empty - 1] < cstart[empty] == cstart[empty + 1] < cstart[empty + 2]
    bad = cstart.copy()
    bad[empty] -= 1
    with pytest.raises(AssertionError, match=rf'k_cell_starts .*1 of 301 .*index {empty} '):
        pc.check_sort_by_cell(keys, 300, k, idx, bad)


# ---- the union-find reference and its cases
@pytest.mark.parametrize("name", pc.UNION_CASES)
def test_union_reference_against_connected_components(name):
    """The sequential union-find against scipy's connected components of the same graph, relabelled to each class's smallest index."""
    import mesh_clean_common as cc
    n, pairs = pc.union_case(name)
    assert pairs.dtype == np.int32 and pairs.shape[1:] == (2,) and (len(pairs) == 0 or (pairs.min() >= 0 and pairs.max() < n))
    root = pc.ref_union(n, pairs)
    assert root.dtype == np.int32 and root.shape == (n,)
    assert np.array_equal(root, cc.rep_of_labels(cc.graph_labels(n, pairs.astype(np.int64))))
    assert np.all(root <= np.arange(n)) and np.array_equal(root[root], root)       # the smallest index of the class, itself a root


def test_union_cases_are_what_they_say():
    sizes = {name: (pc.union_case(name)[0], len(pc.union_case(name)[1])) for name in pc.UNION_CASES}
    assert sizes['single'] == (1, 0) and sizes['self_pair'] == (1, 1) and pc.union_case('self_pair')[1].tolist() == [[0, 0]]
    for name in ('chain_ascending', 'chain_descending', 'chain_shuffled', 'star_on_first', 'star_on_last'):
        assert sizes[name] == (4096, 4095)
        assert not pc.ref_union(*pc.union_case(name)).any()                        # one class: every root is 0
    assert pc.union_case('chain_ascending')[1][:2].tolist() == [[0, 1], [1, 2]] and pc.union_case('chain_descending')[1][0].tolist() == [4094, 4095]
    assert np.all(pc.union_case('star_on_last')[1][:, 0] == 4095) and np.all(pc.union_case('star_on_first')[1][:, 0] == 0)
    assert sizes['chain_four_times'] == (4096, 4 * 4095) and sizes['random_3000_on_1000'] == (1000, 3000)
    assert [sizes[f'pairs_{k}'][1] for k in (255, 256, 257)] == [255, 256, 257]
    assert len(np.unique(pc.ref_union(*pc.union_case('random_3000_on_1000')))) > 1  # more than one class: the labels matter


# ---- the size query
def test_size_query_domain(L):
    q = L.pdhip_debug_prims_workspace_bytes
    for n, nc in [(0, 1), (-1, 1), ((1 << 26) + 1, 1), (1, 0), (1, -5), (1, (1 << 26) + 1)]:
        assert q(n, nc) == 0, (n, nc)
    for n, nc in [(1, 1), (2048, 256), (2113, 300), (1 << 26, 1 << 26)]:
        assert q(n, nc) > 0, (n, nc)
    assert q(1 << 26, 1 << 26) > 24 * (1 << 26) + 4 * (1 << 26)   # two key and two value buffers, cstart


@pytest.mark.parametrize("n", [2048, 2049])
def test_size_query_carves_the_histograms_per_tile(L, n):
    nc = 300
    with wc.CarveLog(L) as log:
        size = L.pdhip_debug_prims_workspace_bytes(n, nc)
        carved, t = log.read()
    cover = wc.check_layout(carved, t, 0, size)
    tiles = n // 2048 + 1
    assert cover[:, 1].tolist() == [8 * n, 8 * n, 4 * n, 4 * n, 4 * 2 * 256 * pc.cdiv(n, 2048), 4 * (nc + 1), 8 * tiles, 8 * tiles]


# ---- refusals: PDHIP_E_ARG with the cause, before any HIP call
def test_entries_refuse_bad_arguments(L):
    buf = (ctypes.c_uint64 * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)                           # a host address: the refusals never look behind it

    def refused(rc, *words):
        assert rc == -1
        msg = L.pdhip_last_error()
        for w in words:
            assert w in msg, (w, msg)

    sort, cell, scan = L.pdhip_debug_radix_sort, L.pdhip_debug_sort_by_cell, L.pdhip_debug_scan
    refused(sort(p, p, 0, 8, p, p, p, None), b'pdhip_debug_radix_sort', b'n=0')
    refused(sort(p, p, (1 << 26) + 1, 8, p, p, p, None), b'pdhip_debug_radix_sort', b'n=')
    refused(sort(p, p, 8, 65, p, p, p, None), b'pdhip_debug_radix_sort', b'bits=65')
    refused(sort(p, p, 8, -1, p, p, p, None), b'pdhip_debug_radix_sort', b'bits=-1')
    refused(sort(p, p, 8, 8, p, p, None, None), b'pdhip_debug_radix_sort', b'null pointer (ws)')
    refused(sort(None, p, 8, 8, p, p, p, None), b'pdhip_debug_radix_sort', b'null pointer (keys)')
    refused(sort(p, p, 8, 8, p, None, p, None), b'pdhip_debug_radix_sort', b'null pointer (vals_out)')
    refused(cell(p, 0, 4, p, p, p, p, None), b'pdhip_debug_sort_by_cell', b'n=0')
    refused(cell(p, 8, 0, p, p, p, p, None), b'pdhip_debug_sort_by_cell', b'nc=0')
    refused(cell(p, 8, 4, p, p, p, None, None), b'pdhip_debug_sort_by_cell', b'null pointer (ws)')
    refused(cell(p, 8, 4, p, p, None, p, None), b'pdhip_debug_sort_by_cell', b'null pointer (cstart_out)')
    for mode in (0, 1):
        refused(scan(p, p, 0, 4, mode, 0, 1, p, None), b'pdhip_debug_scan', b'n=0')
        refused(scan(p, p, 8, 2, mode, 0, 1, p, None), b'pdhip_debug_scan', b'elem_bytes=2')
        refused(scan(p, p, 8, 4, mode, 0, 1, None, None), b'pdhip_debug_scan', b'null pointer (ws)')
        refused(scan(None, p, 8, 8, mode, 1, 1, p, None), b'pdhip_debug_scan', b'null pointer (in)')
        refused(scan(p, p, 8, 8, mode, 1, 0, p, None), b'pdhip_debug_scan', b'nc=0')
    refused(scan(p, p, 8, 4, 2, 0, 1, p, None), b'pdhip_debug_scan', b'mode=2')
    union = L.pdhip_debug_union_pairs                               # (pairs, n_pairs, n, parent, root, status, stream)
    refused(union(p, 4, 0, p, p, p, None), b'pdhip_debug_union_pairs', b'n=0')
    refused(union(p, 4, (1 << 26) + 1, p, p, p, None), b'pdhip_debug_union_pairs', b'n=')
    refused(union(p, -1, 8, p, p, p, None), b'pdhip_debug_union_pairs', b'n_pairs=-1')
    refused(union(p, (1 << 26) + 1, 8, p, p, p, None), b'pdhip_debug_union_pairs', b'n_pairs=')
    refused(union(None, 4, 8, p, p, p, None), b'pdhip_debug_union_pairs', b'null pointer (pairs)', b'n_pairs=4')
    refused(union(p, 4, 8, None, p, p, None), b'pdhip_debug_union_pairs', b'null pointer (parent)')
    refused(union(p, 4, 8, p, None, p, None), b'pdhip_debug_union_pairs', b'null pointer (root)')
    refused(union(p, 4, 8, p, p, None, None), b'pdhip_debug_union_pairs', b'null pointer (status)')
