"""Mesh decimation on the device (csrc/simplify_mesh.hip, spr.simplify_mesh) against the sequential greedy quadric-error decimator of
tests/mesh_simplify_common.py: the smallest meshes, the invariants (closed, oriented, topology, face count), accuracy within 2 x the
sequential result, refused inputs, determinism, colours, real reconstructions, recon_one_shape_SPR(target_faces=) and the CLI's
`spr_faces`."""
import functools
import logging
import os
import re

import numpy as np
import PIL.Image
import pytest
import torch

import mesh_simplify_common as ms

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = 'cuda'
T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)

TETRA_V = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], np.float32)
TETRA_F = np.array([[0, 2, 1], [0, 1, 3], [0, 3, 2], [1, 2, 3]], np.int64)
OCTA_V = 0.5 * np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], np.float32)
OCTA_F = np.array([[0, 2, 4], [2, 1, 4], [1, 3, 4], [3, 0, 4], [2, 0, 5], [1, 2, 5], [3, 1, 5], [0, 3, 5]], np.int64)


@functools.lru_cache(maxsize=None)
def case(name):
    """(vertices, faces, target) of the three synthetic cases of the invariants."""
    from pointdreamer_amd import synthetic
    if name == 'torus':
        return ms.grid_torus(40, 20) + (400,)
    if name == 'noisy_torus':
        return ms.grid_torus(48, 24, noise=0.004, seed=1) + (460,)
    return synthetic.icosphere(12) + (500,)


def simplify(v, f, target, colors=None):
    from pointdreamer_amd import spr
    out = spr.simplify_mesh(T(v), T(f), target, colors=None if colors is None else T(colors), return_counts=True)
    return tuple(t.cpu().numpy() for t in out[:-1]) + (out[-1],)


def check_invariants(v, f, ov, of, info, target, tag, ref=None):
    """Item 2 on one result (numpy arrays); ref = the sequential decimator's (vertices, faces) where there is one."""
    from pointdreamer_amd import mesh_checks as mc
    assert ov.dtype == np.float32 and ov.ndim == 2 and ov.shape[1] == 3 and of.dtype == np.int64 and of.ndim == 2 and of.shape[1] == 3
    assert len(ov) == info['vertices'] and len(of) == info['faces']
    assert of.min() >= 0 and of.max() < len(ov)
    assert (of[:, 0] != of[:, 1]).all() and (of[:, 1] != of[:, 2]).all() and (of[:, 0] != of[:, 2]).all()
    assert len(np.unique(ov.view(np.uint32).reshape(-1, 3), axis=0)) == len(ov), "two vertices equal bit for bit"
    print(f"{tag}: {len(f)} -> {len(of)} faces (target {target}) in {info['rounds']} rounds, stalled {info['stalled']}")
    assert target <= len(of) <= target + 1 and not info['stalled'] and 0 < info['rounds'] <= 1024
    assert mc.directed_edge_defects(of) == 0
    assert [c[1] for c in ms.topology(len(ov), of)] == [c[1] for c in ms.topology(len(v), f)]
    assert len(ms.topology(len(ov), of)) == len(ms.topology(len(v), f))
    assert mc.face_areas(ov, of).min() > 0.0
    assert len(np.unique(of)) == len(ov), "unreferenced vertex"
    vol0, vol = mc.signed_volume(v, f), mc.signed_volume(ov, of)
    assert vol > 0
    if ref is not None:
        dref = abs(mc.signed_volume(*ref) - vol0)
        print(f"{tag}: volume {vol0:.6f} -> {vol:.6f} (sequential reference changes it by {dref:.6f})")
        assert abs(vol - vol0) <= 2 * dref + 1e-6


# ---- 1. the smallest meshes
def test_smallest_meshes():
    from pointdreamer_amd import spr, synthetic, mesh_checks as mc
    from pointdreamer_amd._lib import PdhipError
    v, f, info = simplify(TETRA_V, TETRA_F, 4)
    assert np.array_equal(v.view(np.uint32), TETRA_V.view(np.uint32)) and np.array_equal(f, TETRA_F)
    assert info == dict(vertices=4, faces=4, rounds=0, stalled=False)
    with pytest.raises(PdhipError, match='target_faces'):
        spr.simplify_mesh(T(OCTA_V), T(OCTA_F), 3)
    # a torus cannot have four faces: the call stalls on a valid torus
    tv, tf = ms.grid_torus(4, 3)
    v, f, info = simplify(tv, tf, 4)
    print(f"torus 4 x 3: {len(tf)} -> {len(f)} faces, {info}")
    assert info['stalled'] and 6 <= len(f) <= len(tf) and mc.directed_edge_defects(f) == 0 and ms.topology(len(v), f) == [(len(f), 0)]
    assert len(np.unique(f)) == len(v)
    v, f, info = simplify(OCTA_V, OCTA_F, 4)
    assert len(f) == 4 and len(v) == 4 and not info['stalled'] and mc.directed_edge_defects(f) == 0 and mc.signed_volume(v, f) > 0
    iv, jf = synthetic.icosphere(2)
    v, f, info = simplify(iv, jf, 20)
    assert len(f) == 20 and mc.directed_edge_defects(f) == 0 and ms.topology(len(v), f) == [(20, 2)] and mc.signed_volume(v, f) > 0
    # two tetrahedra next to a sphere: nothing of them may collapse
    sv, sf = synthetic.icosphere(4)
    allv = np.concatenate([0.1 * TETRA_V + [0.7, 0, 0], sv, 0.1 * TETRA_V + [-0.9, 0, 0]]).astype(np.float32)
    allf = np.concatenate([TETRA_F, sf + 4, TETRA_F + 4 + len(sv)])
    v, f, info = simplify(allv, allf, 100)
    assert len(f) == 100 and not info['stalled'] and mc.directed_edge_defects(f) == 0
    assert ms.topology(len(v), f) == [(4, 2), (4, 2), (92, 2)]
    assert np.array_equal(v[:4], allv[:4]) and np.array_equal(v[-4:], allv[-4:]) and np.array_equal(f[:4], TETRA_F)


# ---- 2. invariants, 3. accuracy
@pytest.mark.parametrize("name", ['torus', 'noisy_torus', 'icosphere12'])
def test_invariants(name):
    v, f, target = case(name)
    ov, of, info = simplify(v, f, target)
    check_invariants(v, f, ov, of, info, target, name, ref=ms.sequential_qem(v, f, target))


@pytest.mark.parametrize("name", ['torus', 'noisy_torus'])
def test_accuracy_against_the_sequential_reference(name):
    """Max and mean of both metrics <= 2 x the sequential decimator's on the same input and target (a numpy prototype of the round
    scheme measured ratios of 0.93 - 1.42)."""
    v, f, target = case(name)
    ov, of, _ = simplify(v, f, target)
    got, ref = ms.metrics(v, ov, of), ms.metrics(v, *ms.sequential_qem(v, f, target))
    for k in ('sdf_mean', 'sdf_max', 'v2m_mean', 'v2m_max'):
        print(f"{name} {k}: device {got[k]:.6f} sequential {ref[k]:.6f} ratio {got[k] / ref[k]:.3f}")
    for k in ('sdf_mean', 'sdf_max', 'v2m_mean', 'v2m_max'):
        assert got[k] <= 2 * ref[k], (k, got[k], ref[k])


# ---- 4. odd target, target >= F
def test_odd_target_and_pass_through():
    v, f, _ = case('torus')
    ov, of, info = simplify(v, f, 401)
    assert len(of) in (401, 402) and not info['stalled']
    rgb = np.random.default_rng(0).random(v.shape).astype(np.float32)
    for target in (len(f), len(f) + 7, 10 ** 6):
        pv, pf, pc, info = simplify(v, f, target, colors=rgb)
        assert np.array_equal(pv.view(np.uint32), v.view(np.uint32)) and np.array_equal(pf, f) and np.array_equal(pc, rgb)
        assert info == dict(vertices=len(v), faces=len(f), rounds=0, stalled=False)


# ---- 5. refused inputs
def test_bad_input_is_refused_and_nothing_but_counts_is_written():
    from pointdreamer_amd import spr, _lib
    from pointdreamer_amd._lib import ptr, stream, PdhipError
    L = _lib.lib()
    v, f, _ = case('torus')
    flipped, beyond = f.copy(), f.copy()
    flipped[7] = flipped[7][::-1]
    beyond[11, 2] = len(v)
    same = f.copy()
    same[5, 1] = same[5, 0]
    bad = dict(boundary=np.delete(f, 3, axis=0), flipped=flipped, index_beyond_V=beyond, duplicated_face=np.concatenate([f, f[20:21]]),
               negative_index=np.where(f == 9, -1, f), repeated_corner=same)
    V = len(v)
    for what, faces in bad.items():
        with pytest.raises(PdhipError, match='closed, consistently oriented'):
            spr.simplify_mesh(T(v), T(faces), 400)
        F = len(faces)
        ov = torch.full((V * 3,), -123.0, device=DEV)
        of = torch.full((F * 3,), -77, dtype=torch.int64, device=DEV)
        oc = torch.full((V * 3,), -5.0, device=DEV)
        counts = torch.full((4,), -1, dtype=torch.int32, device=DEV)
        ws = torch.empty((L.pdhip_simplify_mesh_workspace_bytes(V, F),), dtype=torch.uint8, device=DEV)
        X, Fc, Cc = T(v), T(faces), T(np.zeros_like(v))
        rc = L.pdhip_simplify_mesh(ptr(X), V, ptr(Fc), F, ptr(Cc), 400, ptr(ov), ptr(of), ptr(oc), ptr(counts), ptr(ws), stream())
        torch.cuda.synchronize()
        assert rc == -1, what
        assert counts.cpu().tolist() == [0, 0, 0, 2], what
        assert (ov == -123.0).all() and (of == -77).all() and (oc == -5.0).all(), what
    ov, of, info = simplify(v, f, 400)                              # and the library still works
    assert len(of) == 400


# ---- 6. determinism
def test_determinism_also_with_another_stream_busy():
    from pointdreamer_amd import spr
    v, f, target = case('noisy_torus')
    rgb = np.random.default_rng(1).random(v.shape).astype(np.float32)
    X, Fc, Cc = T(v), T(f), T(rgb)
    a = spr.simplify_mesh(X, Fc, target, colors=Cc, return_counts=True)
    b = spr.simplify_mesh(X, Fc, target, colors=Cc, return_counts=True)
    side = torch.cuda.Stream()
    m = torch.randn((2048, 2048), device=DEV)
    with torch.cuda.stream(side):
        for _ in range(20):
            m = m @ m * 1e-3
    c = spr.simplify_mesh(X, Fc, target, colors=Cc, return_counts=True)
    torch.cuda.synchronize()
    for other in (b, c):
        assert torch.equal(a[0].view(torch.int32), other[0].view(torch.int32)) and torch.equal(a[1], other[1])
        assert torch.equal(a[2].view(torch.int32), other[2].view(torch.int32)) and a[3] == other[3]


# ---- 7. colours
@functools.lru_cache(maxsize=None)
def torus_cloud():
    from pointdreamer_amd import synthetic
    S = synthetic.solid('torus')
    return (S,) + S.sample(25000, seed=1)


@functools.lru_cache(maxsize=None)
def reconstruction(name, depth):
    """(S, vertices, faces, colours (numpy), info) of the reconstruction of a 25 000-point cloud with analytic normals."""
    from pointdreamer_amd import spr, synthetic
    S = synthetic.solid(name)
    xyz, rgb, nrm = torus_cloud()[1:] if name == 'torus' else S.sample(25000, seed=1)
    v, f, c, info = spr.poisson_reconstruct(T(xyz), T(nrm), depth=depth, colors=T(rgb), return_counts=True)
    return S, v.cpu().numpy(), f.cpu().numpy(), c.cpu().numpy(), info


def test_colours():
    from scipy.spatial import cKDTree
    v, f, target = case('torus')
    rgb = np.random.default_rng(2).random(v.shape).astype(np.float32)
    ov, of, oc, info = simplify(v, f, target, colors=rgb)
    rows = {r.tobytes() for r in rgb}
    assert oc.shape == ov.shape and oc.dtype == np.float32 and all(r.tobytes() in rows for r in oc)
    S, rv, rf, rc, _ = reconstruction('torus', 6)
    ov, of, oc, info = simplify(rv, rf, 4000, colors=rc)
    rows = {r.tobytes() for r in rc}
    assert len(of) == 4000 and all(r.tobytes() in rows for r in oc)
    err = np.abs(oc - S.color(ov)).mean()
    near = np.abs(rc[cKDTree(rv).query(ov)[1]] - S.color(ov)).mean()
    print(f"mean |colour - colour field|: carried {err:.5f}, nearest input vertex {near:.5f}")
    assert err <= 2 * near


# ---- 8. real reconstructions
@pytest.mark.parametrize("name,depth,target", [('torus', 7, 10000), ('two_spheres', 6, 4000), ('cup', 6, 4000)])
def test_on_reconstructions(name, depth, target):
    S, v, f, _, rinfo = reconstruction(name, depth)
    ov, of, info = simplify(v, f, target)
    check_invariants(v, f, ov, of, info, target, f'{name} d{depth}')
    h = rinfo['h']
    sd_in, sd_out = np.abs(S.sdf(v)).max(), np.abs(S.sdf(ov)).max()
    print(f"{name} d{depth}: {len(f)} -> {len(of)} faces, rounds {info['rounds']} ({(len(f) - len(of)) / info['rounds']:.0f} faces per round); "
          f"max |sdf| of the vertices {sd_in / h:.3f} h -> {sd_out / h:.3f} h")
    assert sd_out <= sd_in + h
    assert info['rounds'] <= 1024


# ---- 9. the reference's signature
def test_recon_one_shape_SPR_with_target_faces(tmp_path):
    from pointdreamer_amd import spr, io_utils, mesh_checks as mc
    S, xyz, rgb, nrm = torus_cloud()
    path = str(tmp_path / 'geo' / 'mesh.obj')
    out = spr.recon_one_shape_SPR(xyz, rgb, None, path, 7, target_faces=10000)
    assert len(out) == 3
    v, f, c = out
    assert v.is_cuda and f.is_cuda and f.shape == (10000, 3) and c.shape == v.shape and c.dtype == torch.float32
    assert mc.directed_edge_defects(f.cpu().numpy()) == 0
    v2, f2 = io_utils.load_obj_mesh(path)
    assert np.array_equal(v2, v.cpu().numpy()) and np.array_equal(f2, f.cpu().numpy())
    *_, info = spr.recon_one_shape_SPR(xyz, rgb, None, None, 7, target_faces=10000, return_counts=True)
    assert info['faces'] == 10000 and info['faces_reconstructed'] > 40000 and 0 < info['simplify_rounds'] <= 1024
    assert info['vertices'] == len(v)
    with pytest.raises(NotImplementedError, match='decimation'):
        spr.recon_one_shape_SPR(xyz, rgb, None, None, 7, simplify_face_num=10000)


# ---- 10. the CLI
def test_cli_spr_faces(tmp_path, caplog):
    from pointdreamer_amd import demo, io_utils, synthetic, mesh_checks as mc
    pc = str(tmp_path / 'torus.ply')
    xyz, rgb, _ = synthetic.solid('torus').sample(20000, seed=1)
    io_utils.save_colored_pc_ply(xyz * 1.7 + 0.3, rgb, pc)
    cfgf = os.path.join(ROOT, "configs", "nearest.yaml")
    base = ["--config", cfgf, "--pc_file", pc, "--set", "geo_from=SPR", "spr_depth=7", "xatlas_texture_res=512"]
    args = base + [f"output_path={tmp_path / 'out'}", "spr_faces=4000"]
    with caplog.at_level(logging.INFO, logger='pointdreamer_amd'):
        out = demo.main(args)[0]
    found = re.search(r'4000 faces, decimated from (\d+) faces in (\d+) rounds', caplog.text)
    assert found, caplog.text
    name = os.path.basename(out)
    geo = os.path.join(out, 'geo', f'{name}_untextured', 'models', 'model_normalized.obj')
    gv, gf = io_utils.load_obj_mesh(geo)
    assert len(gf) == 4000 and mc.directed_edge_defects(gf) == 0 and mc.signed_volume(gv, gf) > 0
    assert ms.topology(len(gv), gf) == [(4000, 0)] and mc.face_areas(gv, gf).min() > 0 and len(np.unique(gf)) == len(gv)
    mv, mf = io_utils.load_obj_mesh(os.path.join(out, 'models', 'model_normalized.obj'))
    assert len(mf) == 4000 and len(mv) == len(gv)
    atlas = os.path.join(out, "models", "model_normalized.png")
    png = np.array(PIL.Image.open(atlas))
    assert png.shape[:2] == (512, 512) and os.path.exists(os.path.join(out, 'geo', 'xatlas_512.pth'))
    t_geo = os.stat(geo).st_mtime_ns
    for k in range(8):                                              # (a resumed directory re-uses its {k}_inpainted.png files: geometry caches only)
        os.remove(os.path.join(out, "others", f"{k}_inpainted.png"))
    out2 = demo.main(args)[0]
    assert out2 == out and os.stat(geo).st_mtime_ns == t_geo
    assert np.array_equal(np.array(PIL.Image.open(atlas)), png)
    # without the key: the reconstruction as it was
    out3 = demo.main(base + [f"output_path={tmp_path / 'plain'}"])[0]
    pv, pf = io_utils.load_obj_mesh(os.path.join(out3, 'models', 'model_normalized.obj'))
    assert len(pf) == int(found.group(1))
