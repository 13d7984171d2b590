"""Shared by tests/test_workspace_cpu.py and tests/test_gpu_workspace.py: the carve log of libpdhip (pdhip_debug_carve_log, include/pdhip.h), the
interval bookkeeping over the regions it reports, and the shapes at which every workspace-taking entry is held to its regions.  Nothing here is
imported by the product.

A region is (offset, bytes) inside a workspace of `length` bytes.  Everything outside the regions -- the slack that Carve::take (csrc/common.h)
leaves in front of the next multiple of 256, the `+ 256` some units add behind their last region, a tail the test appends -- belongs to nobody, and
a kernel that writes there has left its region."""
import ctypes

import numpy as np

LOG_CAPACITY = 256                                                 # what the library keeps (CARVE_LOG_CAP, csrc/capi.hip); it counts what it dropped
ALIGN = 256


def uncovered(length, regions):
    """The byte ranges [start, end) of [0, length) that no region covers, ascending, as an int64 array [n, 2].  regions: (offset, bytes) pairs in any
    order; they may touch, overlap, be empty, or reach past `length` (only the part inside [0, length) counts)."""
    length = int(length)
    r = np.asarray(list(regions), np.int64).reshape(-1, 2)
    r = r[r[:, 1] > 0]                                             # a zero-byte region covers nothing
    lo, hi = np.clip(r[:, 0], 0, length), np.clip(r[:, 0] + r[:, 1], 0, length)
    order = np.argsort(lo, kind='stable')
    lo, hi = lo[order], hi[order]
    reach = np.maximum.accumulate(np.concatenate([[0], hi]))       # reach[i]: the end of everything covered by the first i regions
    ends = np.concatenate([lo, [length]])                          # a gap opens where the covered prefix ends and closes at the next
    gaps = np.stack([reach, ends], 1).astype(np.int64)             # region's start, the last one at `length`
    return gaps[gaps[:, 1] > gaps[:, 0]]


def slack_bytes(length, regions):
    g = uncovered(length, regions)
    return int((g[:, 1] - g[:, 0]).sum())


class CarveLog:
    """with CarveLog(L) as log: ...; log.read() -> (carved, triples int64 [n,3] = base, offset, bytes).  The previous state comes back on exit."""

    def __init__(self, L):
        self.L = L

    def __enter__(self):
        self.old = self.L.pdhip_debug_carve_log(1)
        return self

    def __exit__(self, *exc):
        self.L.pdhip_debug_carve_log(self.old)

    def read(self):
        buf = (ctypes.c_uint64 * (3 * LOG_CAPACITY))()
        carved = self.L.pdhip_debug_carve_log_read(buf, LOG_CAPACITY)
        kept = min(carved, LOG_CAPACITY)
        return carved, np.frombuffer(buf, np.uint64)[:3 * kept].astype(np.int64).reshape(-1, 3)


def _up(n):
    return (int(n) + ALIGN - 1) // ALIGN * ALIGN


def carves(triples):
    """The log split into the Carves that made it: [(indices of its rows, index of its parent row or -1)].  A unit may nest another unit's workspace in
    one of its regions (pdhip_estimate_normals holds pdhip_hidden_point_removal's): its carve function asks the inner size query in the middle of its
    own takes (a Carve on a null base), and its entry hands the region to the inner entry, which carves it on a base of its own.  A row belongs to the
    Carve on top of the stack when it has that Carve's base and starts at or behind its end; a row at offset 0 opens a new Carve; any other row closes
    the top Carve and is the take that made room for it.  A Carve still open at the end has no parent row behind it (-1)."""
    t = np.asarray(triples, np.int64).reshape(-1, 3)
    stack, closed = [], []
    for i, row in enumerate(t):
        while True:
            if stack:
                last = t[stack[-1][-1]]
                if len(stack) > 1:                                 # the next take of the Carve below starts exactly at that Carve's rounded end
                    below = t[stack[-2][-1]]
                    if row[0] == below[0] and row[1] == _up(below[1] + below[2]) and (row[0] != last[0] or row[1] != _up(last[1] + last[2])):
                        closed.append((stack.pop(), i))
                        continue
                if row[0] == last[0] and row[1] >= last[1] + last[2]:
                    stack[-1].append(i)
                    break
                if row[1] != 0:
                    closed.append((stack.pop(), i))
                    continue
            stack.append([i])
            break
    return closed + [(rows, -1) for rows in stack]


def check_layout(carved, triples, base, nbytes):
    """What must hold for the log of ONE size query (base 0) or of ONE entry on the workspace at address `base`, which reports `nbytes`: nothing was
    dropped from the log; in every Carve the offsets are multiples of 256 and ascend without overlap; there is one Carve on `base` itself, and it ends
    inside nbytes; every other Carve fits the region that was taken for it -- for a size query asked while carving (null base) the take that follows
    it, else the region that starts at its base.  Returns the (offset, bytes) pairs, relative to `base`, of the regions that claim memory and hold no
    other Carve: what the entry may touch."""
    assert carved == len(triples), f"the carve log kept {len(triples)} of {carved} regions"
    t = np.asarray(triples, np.int64).reshape(-1, 3)
    start = t[:, 0] + t[:, 1]
    outer, claims, parents = 0, [], set()
    for rows, parent in carves(t):
        b, off, size = t[rows[0], 0], t[rows, 1], t[rows, 2]
        assert np.all(off % ALIGN == 0), off[off % ALIGN != 0]
        assert np.all(size >= 0)
        assert np.all(off[1:] >= off[:-1] + size[:-1]), "regions overlap or descend: " + str(t[rows, 1:].tolist())
        end = int(off[-1] + size[-1])
        if b == base and parent < 0:
            outer += 1
            assert end <= nbytes, (end, nbytes)
            claims += rows
        elif b == 0:                                               # a size query asked while carving: it claims no memory
            assert parent >= 0 and end <= t[parent, 2], ("no take with room for the size query in front of it", end, t[max(parent, 0)].tolist())
        else:
            at = np.flatnonzero((start == b) & (t[:, 0] != b) & (t[:, 2] >= end))
            assert len(at), ("a Carve on a base that no region starts at, or larger than that region", hex(int(b)), end)
            parents.add(int(at[0]))
            claims += rows
    assert outer == (1 if len(t) else 0), f"{outer} Carves on the workspace itself"
    keep = np.array(sorted(set(claims) - parents), np.int64)
    cover = np.stack([start[keep] - base, t[keep, 2]], 1).reshape(-1, 2)
    assert np.all(cover[:, 0] >= 0) and np.all(cover[:, 0] + cover[:, 1] <= nbytes), "a region outside the workspace"
    return cover


# ---- the shapes.  Per size query three rows (test_gpu_workspace.py runs the entry at each; test_workspace_cpu.py checks the layout there):
#   ragged  every sized argument above 2048 (more than one tile of the sort and of the tiled scan) and no multiple of 64 (slack behind every 4-
#           and 8-byte region),
#   tile    exactly 2048 (4096 where two arguments have to differ): no slack inside N-sized regions, cdiv(N, 2048) and N / 2048 + 1 at their edge,
#   min     the smallest the entry accepts,
# and further rows where the unit changes path by size or by a debug hook.  Closed meshes are tori of a x b quads: Vn = a b, F = 2 a b.
TORUS = {'ragged': (47, 45), 'tile': (32, 64), 'switch': (131, 127)}                    # Vn 2115 / 2048 / 16637; the minima: a tetrahedron, a bipyramid, one triangle
SHAPES = {
    'pdhip_knn_points_workspace_bytes': {'ragged': (2113, 5003, 5), 'tile': (2048, 4096, 5), 'min': (1, 1, 1)},
    'pdhip_sor_filter_workspace_bytes': {'ragged': (5003,), 'tile': (2048,), 'min': (2,)},
    'pdhip_fps_workspace_bytes': {'ragged': (5003, 2113), 'tile': (4096, 2048), 'min': (1, 1)},
    'pdhip_owner_mean_colors_workspace_bytes': {'ragged': (2113,), 'tile': (2048,), 'min': (1,)},
    'pdhip_nearest_points_workspace_bytes': {'ragged': (2113, 5003), 'tile': (2048, 4096), 'min': (1, 1)},
    'pdhip_cloud_metrics_workspace_bytes': {'ragged': (2113,), 'tile': (2048,), 'min': (1,)},
    'pdhip_mesh_contains_workspace_bytes': {'ragged': (2115, 4230, 5003, 512), 'tile': (2048, 4096, 2048, 512), 'min': (4, 4, 1, 512)},
    'pdhip_closest_on_mesh_workspace_bytes': {'ragged': (2115, 4230, 5003), 'tile': (2048, 4096, 2048), 'min': (3, 1, 1)},
    'pdhip_mesh_components_workspace_bytes': {'ragged': (2115, 4230), 'tile': (2048, 4096), 'min': (3, 1), 'switch': (16637, 33274)},
    'pdhip_compact_mesh_workspace_bytes': {'ragged': (2115, 4230), 'tile': (2048, 4096), 'min': (3, 1), 'switch': (16637, 33274)},
    'pdhip_simplify_mesh_workspace_bytes': {'ragged': (2115, 4230), 'tile': (2048, 4096), 'min': (5, 6)},
    'pdhip_sample_mesh_workspace_bytes': {'ragged': (4230, 5003), 'tile': (4096, 2048), 'min': (1, 1)},
    'pdhip_uv_atlas_ws_bytes': {'ragged': (2115, 4230), 'tile': (2048, 4096), 'min': (3, 1)},
    'pdhip_estimate_normals_ws_bytes': {'ragged': (5003, 16, 32), 'tile': (2048, 16, 32), 'min': (16, 3, 1)},
    'pdhip_surface_recon_ws_bytes': {'ragged': (5003, 6), 'tile': (2048, 6), 'min': (16, 6)},
    'pdhip_subdivide_with_uv_ws_bytes': {'ragged': (2115, 2115, 4230, 2113), 'tile': (2048, 2048, 4096, 2048), 'min': (3, 3, 1, 1)},
    'pdhip_vertex_uv_table_ws_bytes': {'ragged': (2115, 4230), 'tile': (2048, 4096), 'min': (3, 1)},
    'pdhip_neighbour_csr_ws_bytes': {'ragged': (2115, 4230), 'tile': (2048, 4096), 'min': (3, 1)},
    'pdhip_compact_zero_count_ws_bytes': {'ragged': (5003,), 'tile': (2048,), 'min': (1,)},
    'pdhip_image_metrics_workspace_bytes': {'ragged': (3, 67, 45), 'tile': (2, 64, 64), 'min': (1, 7, 7)},
    'pdhip_raster_mesh_ws_bytes': {'ragged': (3, 4230, 67), 'tile': (2, 4096, 64), 'min': (1, 1, 8)},
    'pdhip_nearest_fill_ws_ints': {'ragged': (3, 67, 45), 'tile': (2, 64, 64), 'min': (1, 1, 1)},
    'pdhip_hpr_ws_bytes': {'one_level': (4, 300), 'two_level': (2, 5000), 'ragged': (3, 5003), 'tile': (2, 4096), 'two_tiles': (2, 8192), 'min': (1, 1)},
    'pdhip_optimize_color_ws_bytes': {'parent': (2, 32, 32), 'ragged': (3, 47, 45), 'tile': (2, 64, 32), 'min': (1, 8, 8)},
    'pdhip_sparse_views_ws_bytes': {'parent': (2, 500, 32), 'ragged': (3, 2113, 47), 'tile': (2, 2048, 64), 'min': (1, 1, 8)},
    'pdhip_linear_fill_ws_bytes': {'parent': (2, 40, 40), 'ragged': (3, 47, 45), 'tile': (2, 64, 32), 'min': (1, 1, 1)},
    'pdhip_debug_prims_workspace_bytes': {'ragged': (2113, 300), 'tile': (2048, 256), 'min': (1, 1)},
    'pdhip_unet_head_ws_floats': {'ragged': (3, 24, 40, 64, 6), 'tile': (2, 64, 64, 32, 3), 'min': (1, 8, 8, 32, 3)},
}
