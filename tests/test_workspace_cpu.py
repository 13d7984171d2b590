"""Workspace layouts without a GPU: every size query of include/pdhip.h, called with the carve log on (pdhip_debug_carve_log), reports regions on a
null base that start on multiples of 256 bytes, ascend without overlap and end inside the size it returns.  The argument sets are those of
tests/golden/ws_bytes_parent.json where the query is in it, and the rows of workspace_common.SHAPES (the shapes tests/test_gpu_workspace.py runs the
entries at) for every query.  Plus the unit test of the interval bookkeeping both files share."""
import json
import os

import numpy as np
import pytest

import workspace_common as wc
from conftest import GOLDEN

TABLE = json.load(open(os.path.join(GOLDEN, 'ws_bytes_parent.json')))
# the queries that carve nothing, read off the code: pdhip_raster_mesh_ws_bytes is the larger of two uses of ONE buffer (raster.hip), pdhip_nearest_fill_ws_ints
# counts the ints of two arrays laid end to end by pointer arithmetic (nearest.hip), pdhip_unet_head_ws_floats likewise in floats (nn_head.hip), and
# pdhip_vertex_uv_table_ws_bytes is one array of V ints + 256 (neighbor_mesh.hip).  A new unit that sizes its workspace without a Carve fails
# test_the_queries_without_regions_are_these_four.
NO_CARVE = {'pdhip_raster_mesh_ws_bytes', 'pdhip_nearest_fill_ws_ints', 'pdhip_unet_head_ws_floats', 'pdhip_vertex_uv_table_ws_bytes'}
UNIT = {'pdhip_nearest_fill_ws_ints': 4, 'pdhip_unet_head_ws_floats': 4}          # bytes per unit of what the query returns


def queries():
    from pointdreamer_amd import _lib
    import pointdreamer_amd.ddnm_inpainting  # noqa: F401  (registers the UNet entry points)
    return sorted(n for n in _lib._SIGS if n.endswith(('_ws_bytes', '_workspace_bytes', '_ws_ints', '_ws_floats')))


def argument_sets(name):
    return [tuple(a) for a, _ in TABLE.get(name, [])] + list(wc.SHAPES[name].values())


def logged_query(name, args):
    """(returned size in bytes, regions carved, triples) of one size query with the log on."""
    from pointdreamer_amd import _lib
    L = _lib.lib()
    with wc.CarveLog(L) as log:
        size = getattr(L, name)(*args)
        carved, triples = log.read()
    return size * UNIT.get(name, 1), carved, triples


def test_all_28_queries_have_shapes():
    q = queries()
    assert len(q) == 28 and q == sorted(wc.SHAPES)
    assert set(TABLE) <= set(q)
    for name in q:
        assert len(set(argument_sets(name))) >= 3, name


def test_the_log_is_off_by_default_and_restores_its_state():
    from pointdreamer_amd import _lib
    L = _lib.lib()
    assert L.pdhip_debug_carve_log(0) == 0                         # off by default
    assert L.pdhip_hpr_ws_bytes(2, 5000) > 0 and L.pdhip_debug_carve_log_read(None, 0) == 0           # ... and nothing is recorded
    with wc.CarveLog(L) as log:
        assert L.pdhip_debug_carve_log(1) == 1                     # (switching it on again clears it)
        L.pdhip_hpr_ws_bytes(2, 5000)
        n, t = log.read()
        L.pdhip_hpr_ws_bytes(2, 5000)
        assert n > 0 and log.read()[0] == 2 * n                    # two queries: the log accumulates until it is cleared
    assert L.pdhip_debug_carve_log(0) == 0 and L.pdhip_debug_carve_log_read(None, 0) == 0


def test_the_log_counts_what_it_cannot_keep():
    from pointdreamer_amd import _lib
    L = _lib.lib()
    with wc.CarveLog(L) as log:
        n = 0
        while n <= 256:
            L.pdhip_hpr_ws_bytes(2, 5000)
            n = L.pdhip_debug_carve_log_read(None, 0)
        carved, triples = log.read()
        assert carved == n > 256 and len(triples) == 256           # kept 256, counted all
        with pytest.raises(AssertionError, match='kept 256'):
            wc.check_layout(carved, triples, 0, 1 << 40)


@pytest.mark.parametrize("name", sorted(wc.SHAPES))
def test_regions_of_every_query_are_aligned_ascending_and_inside_the_size(name):
    carving = 0
    for args in argument_sets(name):
        size, carved, triples = logged_query(name, args)
        cover = wc.check_layout(carved, triples, 0, size)          # (a refused size returns 0 and must then have carved nothing that needs room)
        print(name, args, 'bytes', size, 'regions', carved, 'of the query itself', len(cover), 'slack', wc.slack_bytes(size, cover) if carved else '-')
        carving += carved > 0
        if name in wc.SHAPES and args in wc.SHAPES[name].values():
            assert size > 0, (name, args)                          # the GPU rows are shapes the entry accepts
    assert (carving == 0) == (name in NO_CARVE), (name, carving)


def test_the_queries_without_regions_are_these_four():
    silent = {name for name in queries() if all(logged_query(name, a)[1] == 0 for a in argument_sets(name))}
    assert silent == NO_CARVE


# ---- the interval bookkeeping
def gaps(length, regions):
    return wc.uncovered(length, regions).tolist()


def test_uncovered_ranges_of_hand_made_regions():
    assert gaps(1000, []) == [[0, 1000]]                           # no region: everything is canary
    assert gaps(0, []) == [] and gaps(0, [(0, 0)]) == []
    assert gaps(1000, [(0, 1000)]) == []
    assert gaps(1000, [(0, 100), (256, 44)]) == [[100, 256], [300, 1000]]
    assert gaps(512, [(0, 256), (256, 256)]) == []                 # touching regions leave no gap between them
    assert gaps(768, [(0, 256), (256, 100), (512, 256)]) == [[356, 512]]      # ... and one that ends at the length leaves no tail
    assert gaps(768, [(512, 256), (0, 256), (256, 100)]) == [[356, 512]]      # any order
    assert gaps(600, [(0, 10), (256, 0), (512, 8)]) == [[10, 512], [520, 600]]      # a zero-byte region covers nothing
    assert gaps(600, [(256, 0)]) == [[0, 600]]
    assert gaps(300, [(0, 200), (100, 50), (256, 10)]) == [[200, 256], [266, 300]]  # a region inside another does not shorten the cover
    assert gaps(300, [(256, 100)]) == [[0, 256]]                   # the part past the length does not count
    assert wc.slack_bytes(1000, [(0, 100), (256, 44)]) == 156 + 700
    assert wc.uncovered(10, []).dtype == np.int64 and wc.uncovered(10, []).shape == (1, 2)


def test_check_layout_refuses_what_it_should():
    ok = np.array([[0, 0, 100], [0, 256, 256], [0, 512, 0], [0, 512, 8]], np.int64)
    wc.check_layout(4, ok, 0, 520)
    for bad, nbytes, base in [(np.array([[0, 0, 100], [0, 128, 8]]), 4096, 0),             # not on a multiple of 256
                              (np.array([[0, 0, 300], [0, 256, 8]]), 4096, 0),             # overlap
                              (np.array([[0, 256, 8], [0, 0, 8]]), 4096, 0),               # descending
                              (ok, 519, 0),                                                # ends past the size
                              (ok, 520, 4096),                                             # another base
                              (np.array([[0, 0, 8], [7, 256, 8]]), 4096, 0)]:              # two bases
        with pytest.raises(AssertionError):
            wc.check_layout(len(bad), bad.astype(np.int64), base, nbytes)


def test_check_layout_follows_a_workspace_nested_in_a_region():
    """An outer unit with regions at 0 and 256 asks an inner size query (regions at 0 and 256, 556 bytes in all) and takes 1024 bytes for it at 512;
    its entry, on base B, hands B + 512 to the inner entry.  What may be touched: the outer's first two regions and the inner's two, not the slack
    behind the inner's last region inside the outer's third."""
    B = 1 << 20
    query = np.array([[0, 0, 100], [0, 256, 8], [0, 0, 10], [0, 256, 300], [0, 512, 1024]], np.int64)
    assert wc.carves(query) == [([2, 3], 4), ([0, 1, 4], -1)]
    assert wc.check_layout(5, query, 0, 1536).tolist() == [[0, 100], [256, 8], [512, 1024]]
    entry = np.concatenate([query + B * np.array([[1, 0, 0]] * 2 + [[0, 0, 0]] * 2 + [[1, 0, 0]]), [[B + 512, 0, 10], [B + 512, 256, 300]]])
    assert wc.check_layout(7, entry, B, 1536).tolist() == [[0, 100], [256, 8], [512, 10], [768, 300]]
    assert wc.uncovered(1536 + 16, wc.check_layout(7, entry, B, 1536)).tolist() == [[100, 256], [264, 512], [522, 768], [1068, 1552]]
    for bad in (np.concatenate([entry[:6], [[B + 512, 256, 800]]]),                        # the inner Carve outgrows the region taken for it
                np.concatenate([entry[:5], [[B + 300, 0, 10]]]),                           # a Carve on a base that no region starts at
                np.concatenate([query[:2], [[0, 0, 10], [0, 256, 300]], [[0, 512, 500]]])):     # the inner query is larger than the take behind it
        with pytest.raises(AssertionError):
            wc.check_layout(len(bad), bad, B if bad[0, 0] else 0, 1536)
