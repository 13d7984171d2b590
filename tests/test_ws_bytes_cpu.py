"""Workspace sizes without a GPU: every pdhip_*_ws_bytes query against the values recorded from the library before the queries and
the entries were made to share one carve function per unit (tests/golden/ws_bytes_parent.json: query -> [[arguments, bytes], ...]).
The Python wrappers ask for the size on every call, so a query may grow by alignment padding but must never shrink."""
import json
import os

import pytest

from conftest import GOLDEN

TABLE = json.load(open(os.path.join(GOLDEN, 'ws_bytes_parent.json')))
# pdhip_linear_fill packed its regions unaligned; each of its nine regions (sites, query list, counts, the two counters, boundary list,
# row starts, row queries, fallback counts, todo bytes) now starts on a multiple of 256 bytes: at most 256 bytes more per region
GROWTH = {'pdhip_linear_fill_ws_bytes': 9 * 256}


def test_the_table_covers_all_eleven_queries():
    from pointdreamer_amd import _lib
    queries = sorted(n for n in _lib._SIGS if n.endswith('_ws_bytes') and n != 'pdhip_raster_mesh_ws_bytes')   # (raster: a max of two uses)
    assert queries == sorted(TABLE) and len(queries) == 11
    assert [a for a, _ in TABLE['pdhip_hpr_ws_bytes']] == [[1, 1], [4, 300], [2, 5000], [64, 30000]]
    assert [a for a, _ in TABLE['pdhip_optimize_color_ws_bytes']] == [[1, 8, 8], [2, 32, 32], [8, 256, 1024], [20, 1024, 1024]]
    assert [a for a, _ in TABLE['pdhip_sparse_views_ws_bytes']] == [[1, 0, 8], [2, 500, 32], [8, 30000, 256]]
    assert [a for a, _ in TABLE['pdhip_linear_fill_ws_bytes']] == [[1, 1, 1], [2, 40, 40], [8, 256, 256]]


@pytest.mark.parametrize("name", sorted(TABLE))
def test_ws_bytes_equal_the_recorded_values(name):
    from pointdreamer_amd import _lib
    fn = getattr(_lib.lib(), name)
    for args, want in TABLE[name]:
        got = fn(*args)
        print(name, args, 'recorded', want, 'now', got)
        assert want <= got <= want + GROWTH.get(name, 0), (name, args, want, got)
