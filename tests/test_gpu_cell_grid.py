"""The four entries on the shared f64 grid of csrc/cell_list.h (pdhip_nearest_points, pdhip_knn_points, pdhip_fps, pdhip_closest_on_mesh) against
tests/golden/cell_grid_parent.npz, recorded on an MI355X at the commit before the grid, its key and its face bound moved into the header
(tools/bench_geometry_metrics.py bytes).  The units' own tests hold the results to brute-force oracles; those do not see how the queries split
between the certificate and the scan of everything, which is what the face bound decides, and counts[] does."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def test_bytes_and_counts_equal_the_recorded_ones():
    from tools import bench_geometry_metrics as ev
    want = np.load(ev.BYTES_PATH)
    for case in ev.SPLIT_CASES:                                    # (a fixture in which every query goes one way does not test the bound)
        c = want[case + '.counts']
        assert c[0] > 0 and c[1] > 0, (case, c.tolist())
    got = ev.cell_grid_bytes()
    assert sorted(got) == sorted(want.files)
    for k in sorted(want.files):
        a, b = got[k], want[k]
        if k.endswith('.counts'):
            print(k, a.tolist(), b.tolist())
        assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b), k
