"""The mesh side of complete_unseen_by='neighbor' on the device (csrc/neighbor_mesh.hip through mesh_utils / unproject): midpoint
subdivision with UVs, the per-vertex UV table, the neighbour CSR and the list of uncoloured vertices.  The oracle is the numpy code of
pointdreamer_amd/mesh_utils.py run on the host inside the test (itself pinned to the reference's outputs by the neighbor_*.npz
fixtures); everything is compared with np.array_equal, floats included."""
import ctypes

import numpy as np
import pytest
import torch

from conftest import load_golden

pytestmark = pytest.mark.gpu
DEV = 'cuda'


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def N_(t):
    return t.detach().cpu().numpy()


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b)


def check_mesh(mesh, face_index, rounds=1):
    """`rounds` chained subdivisions (the same index list every round, as unproject.py:111-114 does), then the UV table and the CSR:
    device against host, every array."""
    from pointdreamer_amd import mesh_utils as mu
    h = mesh
    d = tuple(T(x) for x in mesh)
    fi_d = None if face_index is None else T(np.asarray(face_index, np.int64))
    for _ in range(rounds):
        hv, hf, hu, hfu = mu.subdivide_with_uv(h[0], h[1], h[2], h[3], face_index=face_index)
        dv, df, du, dfu = mu.subdivide_with_uv(d[0], d[1], d[2], d[3], face_index=fi_d)
        assert all(x.is_cuda for x in (dv, df, du, dfu))
        assert same(N_(dv), hv) and same(N_(df), hf) and same(N_(du), hu) and same(N_(dfu), hfu)
        h, d = (hv, hf, hfu, hu), (dv, df, dfu, du)
    V = len(h[0])
    tab = mu.vertex_uv_table(V, d[1], d[2], d[3])
    assert tab.is_cuda and same(N_(tab), mu.vertex_uv_table(V, h[1], h[2], h[3]))
    rowptr, colidx = mu.neighbour_csr(V, d[1])
    href = mu.neighbour_csr(V, h[1])
    assert same(N_(rowptr), href[0]) and same(N_(colidx), href[1])
    return h, d


# ---- meshes: (vertices, faces, face_uv_idx, uvs), the argument order of subdivide_with_uv
@pytest.fixture(scope="module")
def ico():
    """icosphere(8): 1 280 faces, 642 vertices, per-corner UVs (U = 3F: the UV edges are not the position edges).  3 840 corner keys
    span two 2 048-element sort tiles; the endpoints need more than one 8-bit digit each."""
    from pointdreamer_amd import synthetic
    v, f = synthetic.icosphere(8)
    assert v.shape == (642, 3) and f.shape == (1280, 3)
    fu = np.arange(3 * len(f), dtype=np.int64).reshape(-1, 3)
    u = np.random.default_rng(5).uniform(0.02, 0.98, (3 * len(f), 2)).astype(np.float32)
    return v, f, fu, u


@pytest.fixture(scope="module")
def sphere():
    from pointdreamer_amd import synthetic
    v, f, _ = synthetic.uv_sphere(16, 32)
    u, fu = synthetic.uv_sphere_uvs(16, 32, 256, gutter=2)
    return v.astype(np.float32), f.astype(np.int64), fu.astype(np.int64), u.astype(np.float32)


@pytest.fixture(scope="module")
def handmade():
    """A face [i,i,j], a duplicated face, an edge (1,2) shared by three faces (four with the duplicate), a vertex (6) no face uses.  The
    degenerate face holds the LAST vertex twice: its edge (7,7) has the largest key there is, the one the sort's padding uses too."""
    v = np.random.default_rng(1).normal(size=(8, 3)).astype(np.float32)
    f = np.array([[7, 7, 0], [1, 2, 3], [1, 2, 3], [2, 1, 4], [1, 2, 5], [0, 3, 4]], np.int64)
    fu = np.array([[0, 1, 2], [3, 4, 5], [3, 4, 5], [4, 3, 6], [7, 8, 9], [2, 5, 6]], np.int64)
    u = np.random.default_rng(2).uniform(0, 1, (11, 2)).astype(np.float32)          # UV 10 is unused
    return v, f, fu, u


@pytest.mark.parametrize("name", ["neighbor_small.npz", "neighbor_seam.npz"])
def test_golden_fixtures_two_rounds(name):
    g = load_golden(name)
    h, d = check_mesh((g['vertices'], g['faces'], g['face_uv_idx'], g['uvs']), g['to_inpaint_face_id'], rounds=2)
    assert same(N_(d[0]), g['ref_sub_vertices']) and same(N_(d[1]), g['ref_sub_faces'])


@pytest.mark.parametrize("pick", ["all", "third", "duplicates"])
def test_icosphere_two_chained_rounds(ico, pick):
    rng = np.random.default_rng(7)
    F = len(ico[1])
    fi = {"all": None, "third": np.sort(rng.choice(F, F // 3, replace=False)),
          "duplicates": rng.integers(0, F, 2 * F // 3)}[pick]                       # unsorted, with repeats
    if pick == "duplicates":
        assert len(np.unique(fi)) < len(fi)
    h, _ = check_mesh(ico, fi, rounds=2)
    assert len(h[1]) > F


@pytest.mark.parametrize("pick", ["all", "third"])
def test_uv_sphere_seams_and_poles(sphere, pick):
    F = len(sphere[1])
    fi = None if pick == "all" else np.random.default_rng(3).choice(F, F // 3, replace=False)
    check_mesh(sphere, fi, rounds=2 if pick == "third" else 1)


@pytest.mark.parametrize("fi", [None, [], [3], [0], [0, 0, 0], [0, 1, 2, 3, 4, 5], [4, 1, 4, 2, 2]], ids=str)
def test_handmade_mesh(handmade, fi):
    h, d = check_mesh(handmade, None if fi is None else np.asarray(fi, np.int64))
    if fi == []:                                                    # K = 0: the input comes back unchanged
        assert all(same(a, b) for a, b in zip(h, handmade))
    if fi in ([0], [0, 0, 0]):              # [7,7,0]: the midpoint of the edge (7,7) is x[7], as numpy computes it; (0,7) sorts before it
        x = handmade[0]
        assert np.array_equal(h[0][8:], np.stack([(x[0] + x[7]) / np.float32(2), x[7]]))


def test_counts_of_the_c_entry_and_a_bad_index(handmade):
    from pointdreamer_amd import _lib, mesh_utils as mu
    from pointdreamer_amd._lib import ptr
    L = _lib.lib()
    v, f, fu, u = (T(x) for x in handmade)
    V, F, U = len(v), len(f), len(u)

    def run(fi):
        K = -1 if fi is None else len(fi)
        Tm = F if K < 0 else min(K, F)
        fi_d = T(np.asarray(fi, np.int64)) if K > 0 else None
        out = [torch.empty((V + 3 * Tm, 3), device=DEV), torch.empty((F + 3 * Tm, 3), dtype=torch.int64, device=DEV),
               torch.empty((U + 3 * Tm, 2), device=DEV), torch.empty((F + 3 * Tm, 3), dtype=torch.int64, device=DEV)]
        counts = torch.full((4,), -7, dtype=torch.int32, device=DEV)
        host = (ctypes.c_int32 * 4)()
        ws = torch.empty((L.pdhip_subdivide_with_uv_ws_bytes(V, U, F, K),), dtype=torch.uint8, device=DEV)
        rc = L.pdhip_subdivide_with_uv(ptr(v), V, ptr(f), F, ptr(u), U, ptr(fu), ptr(fi_d) if K > 0 else None, K, *[ptr(o) for o in out],
                                       ptr(counts), host, ptr(ws), _lib.stream())
        return rc, list(host), N_(counts).tolist()

    assert run([]) == (0, [V, U, F, 0], [V, U, F, 0])                                   # K = 0: T = 0
    rc, host, dev = run([3])
    assert rc == 0 and host == dev == [V + 3, U + 3, F + 3, 1]
    rc, host, dev = run([1, 2, 2, 1])                                                   # the duplicated face twice over: T = 2, 3 edges
    assert rc == 0 and host == dev == [V + 3, U + 3, F + 6, 2]
    rc, host, dev = run(None)
    assert rc == 0 and host == dev and host[3] == F and host[2] == 4 * F
    for bad in ([0, F], [-1]):
        assert run(bad)[0] == -1 and b'face_index' in L.pdhip_last_error()
        with pytest.raises(_lib.PdhipError, match='face_index'):
            mu.subdivide_with_uv(v, f, fu, u, face_index=np.asarray(bad))


@pytest.mark.parametrize("case", ["no_zero", "all_zero", "ends", "random"])
def test_compact_zero_count(case):
    """V = 5 000: the one-workgroup scan gives each of its 1 024 threads a chunk of 5, the last chunks are short or empty."""
    from pointdreamer_amd import mesh_utils as mu
    V = 5000
    count = np.ones(V, np.float32)
    if case == "all_zero":
        count[:] = 0
    elif case == "ends":
        count[[0, V - 1]] = 0
    elif case == "random":
        count = (np.random.default_rng(0).uniform(size=V) > 0.4).astype(np.float32)
    got = mu.zero_count_vertices(T(count))
    assert got.is_cuda and same(N_(got), np.nonzero(count == 0)[0].astype(np.int32))


def _paint_inputs(mesh, fi, A, seed):
    v, f, fu, u = mesh
    rng = np.random.default_rng(seed)
    atlas = rng.uniform(0, 1, (A, A, 3)).astype(np.float32)
    painted = rng.uniform(size=(A, A)) > 0.5
    return [T(v), T(f), T(u), T(fu), np.asarray(fi, np.int64), T(atlas), T(painted)]


@pytest.fixture
def d2h(monkeypatch):
    """Sizes in bytes of the device-to-host copies made through Tensor.cpu / .item / .numpy / .tolist."""
    seen = []
    for name in ('cpu', 'item', 'numpy', 'tolist'):
        orig = getattr(torch.Tensor, name)

        def wrapped(self, *a, _orig=orig, **kw):
            if self.is_cuda:
                seen.append(self.numel() * self.element_size())
            return _orig(self, *a, **kw)
        monkeypatch.setattr(torch.Tensor, name, wrapped)
    return seen


@pytest.mark.parametrize("case", ["seam", "ico"])
def test_route_identity_and_no_mesh_transfer(case, ico, d2h):
    """mesh_on='device' against mesh_on='host': the same atlas and the same use_atlas=False triple; the device route copies nothing
    larger than 64 bytes to the host (its counts come back inside the C entries; the loop control reads one word per round)."""
    from pointdreamer_amd import unproject as up
    if case == "seam":
        g = load_golden("neighbor_seam.npz")
        args = [T(g['vertices']), T(g['faces']), T(g['uvs']), T(g['face_uv_idx']), g['to_inpaint_face_id'], T(g['atlas']), T(g['painted'])]
    else:
        F = len(ico[1])
        args = _paint_inputs(ico, np.sort(np.random.default_rng(11).choice(F, F // 3, replace=False)), 64, 12)
    del d2h[:]
    a_dev = up.paint_invisible_areas_by_neighbors(*args, use_atlas=True, mesh_on='device')
    t_dev = up.paint_invisible_areas_by_neighbors(*args, use_atlas=False, mesh_on='device')
    a_def = up.paint_invisible_areas_by_neighbors(*args, use_atlas=True)              # None = device for these inputs
    torch.cuda.synchronize()
    dev_copies = list(d2h)
    assert dev_copies and max(dev_copies) <= 64, dev_copies
    del d2h[:]
    a_host = up.paint_invisible_areas_by_neighbors(*args, use_atlas=True, mesh_on='host')
    t_host = up.paint_invisible_areas_by_neighbors(*args, use_atlas=False, mesh_on='host')
    assert max(d2h) > 64                                             # (the probe sees the host route's mesh download)
    assert torch.equal(a_dev, a_host) and torch.equal(a_def, a_host)
    for x, y in zip(t_dev, t_host):
        assert x.dtype == y.dtype and torch.equal(x, y)
    with pytest.raises(Exception, match='mesh_on'):
        up.paint_invisible_areas_by_neighbors(*args, mesh_on='gpu')


def test_two_calls_give_equal_bytes(ico):
    from pointdreamer_amd import mesh_utils as mu
    d = tuple(T(x) for x in ico)
    fi = T(np.random.default_rng(4).integers(0, len(ico[1]), 700))
    runs = []
    for _ in range(2):
        out = mu.subdivide_with_uv(*d, face_index=fi)
        V = len(out[0])
        runs.append(out + (mu.vertex_uv_table(V, out[1], out[3], out[2]),) + mu.neighbour_csr(V, out[1]))
    for a, b in zip(*runs):
        assert a.data_ptr() != b.data_ptr() and torch.equal(a, b)
        assert a.dtype != torch.float32 or torch.equal(a.view(torch.int32), b.view(torch.int32))
