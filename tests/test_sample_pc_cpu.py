"""The mesh sampler's host side without a GPU: the multi-material OBJ loader on files written here, the packed material set, the .npy
round trip, and self-checks of the CPU oracle (tests/sample_pc_common.py) and of the fixture the GPU tests rely on."""
import os

import numpy as np
import PIL.Image
import pytest
import torch

import sample_pc_common as sc


def write_mesh(d, obj, mtl=None, images=()):
    os.makedirs(d, exist_ok=True)
    with open(os.path.join(d, 'm.obj'), 'w') as f:
        f.write(obj)
    if mtl is not None:
        with open(os.path.join(d, 'm.mtl'), 'w') as f:
            f.write(mtl)
    for name, arr in images:
        PIL.Image.fromarray(arr).save(os.path.join(d, name))
    return os.path.join(d, 'm.obj')


VERTS = "v 0 0 0\nv 1 0 0\nv 1 1 0\nv 0 1 0\nv 0 0 1\nvt 0 0\nvt 1 0\nvt 1 1\nvt 0 1\n"
MTL3 = "newmtl wood\nKd 0.1 0.2 0.3\nmap_Kd wood.png\n\nnewmtl paint\nKd 0.9 0.8 0.7\n\nnewmtl cloth\nmap_Kd cloth.png\n"


def images3():
    rng = np.random.default_rng(3)
    return [('wood.png', rng.integers(0, 256, (5, 9, 3), dtype=np.uint8)), ('cloth.png', rng.integers(0, 256, (7, 4, 3), dtype=np.uint8))]


def test_loader_reads_three_materials_a_polygon_and_a_face_without_vt(tmp_path):
    """Materials are numbered in MTL order (wood, paint, cloth) although the OBJ uses cloth first; the quad becomes two triangles of
    cloth; the face written without vt carries -1; the two images keep their own, non-square sizes; a grey PNG comes back as RGB."""
    from pointdreamer_amd.sample_colored_pc_from_mesh import load_obj_with_materials
    imgs = images3()
    obj = ("mtllib m.mtl\n" + VERTS + "usemtl cloth\nf 1/1 2/2 3/3 4/4\nusemtl paint\nf 1 2 5\nusemtl wood\nf 2/2 3/3 5/1\n"
           "usemtl cloth\nf 3/3 4//1 5/2\n")
    v, f, vt, ft, fm, mats = load_obj_with_materials(write_mesh(str(tmp_path), obj, MTL3, imgs))
    assert v.shape == (5, 3) and v.dtype == np.float32 and vt.shape == (4, 2) and vt.dtype == np.float32
    assert f.dtype == np.int64 and ft.dtype == np.int64 and fm.dtype == np.int32
    assert f.tolist() == [[0, 1, 2], [0, 2, 3], [0, 1, 4], [1, 2, 4], [2, 3, 4]]
    assert ft.tolist() == [[0, 1, 2], [0, 2, 3], [-1, -1, -1], [1, 2, 0], [2, -1, 1]]
    assert fm.tolist() == [2, 2, 1, 0, 2]
    assert [m['name'] for m in mats] == ['wood', 'paint', 'cloth']
    assert np.array_equal(mats[0]['map_Kd'], imgs[0][1]) and mats[0]['map_Kd'].shape == (5, 9, 3)
    assert np.array_equal(mats[2]['map_Kd'], imgs[1][1]) and mats[2]['map_Kd'].shape == (7, 4, 3)
    assert 'map_Kd' not in mats[1] and mats[1]['Kd'].dtype == np.float32 and np.allclose(mats[1]['Kd'], [0.9, 0.8, 0.7])
    grey = np.arange(12, dtype=np.uint8).reshape(3, 4)
    d2 = str(tmp_path / 'grey')
    _, _, _, _, _, m2 = load_obj_with_materials(write_mesh(d2, "mtllib m.mtl\n" + VERTS + "usemtl g\nf 1/1 2/2 3/3\n",
                                                           "newmtl g\nmap_Kd g.png\n", [('g.png', grey)]))
    assert m2[0]['map_Kd'].shape == (3, 4, 3) and np.array_equal(m2[0]['map_Kd'][..., 1], grey)


def test_loader_refuses_broken_files_by_name(tmp_path):
    from pointdreamer_amd.sample_colored_pc_from_mesh import load_obj_with_materials
    imgs = images3()
    p = write_mesh(str(tmp_path / 'a'), "mtllib m.mtl\n" + VERTS + "usemtl steel\nf 1 2 3\n", MTL3, imgs)
    with pytest.raises(ValueError, match='steel') as e:
        load_obj_with_materials(p)
    assert p in str(e.value)
    p = write_mesh(str(tmp_path / 'b'), "mtllib m.mtl\n" + VERTS + "f 1 2 3\nusemtl wood\nf 1 2 5\n", MTL3, imgs)
    with pytest.raises(ValueError, match='precedes the first usemtl') as e:
        load_obj_with_materials(p)
    assert p in str(e.value)
    many = ''.join(f"newmtl k{i}\nKd 0 0 {i / 300:.4f}\n" for i in range(256))
    p = write_mesh(str(tmp_path / 'c'), "mtllib m.mtl\n" + VERTS + "usemtl k0\nf 1 2 3\n", many)
    with pytest.raises(ValueError, match='256 materials') as e:
        load_obj_with_materials(p)
    assert p in str(e.value)
    ok = ''.join(f"newmtl k{i}\nKd 0 0 {i / 300:.4f}\n" for i in range(255))              # 255 is the limit, not beyond it
    _, _, _, _, fm, mats = load_obj_with_materials(write_mesh(str(tmp_path / 'd'), "mtllib m.mtl\n" + VERTS + "usemtl k254\nf 1 2 3\n", ok))
    assert len(mats) == 255 and fm.tolist() == [254]


def test_loader_gives_a_mesh_without_mtl_one_grey_material(tmp_path):
    from pointdreamer_amd.sample_colored_pc_from_mesh import load_obj_with_materials
    v, f, vt, ft, fm, mats = load_obj_with_materials(write_mesh(str(tmp_path), "v 0 0 0\nv 1 0 0\nv 0 1 0\nusemtl whatever\nf 1 2 3\n"))
    assert len(mats) == 1 and 'map_Kd' not in mats[0] and mats[0]['Kd'].tolist() == [0.5, 0.5, 0.5]
    assert fm.tolist() == [0] and vt.shape == (0, 2) and ft.tolist() == [[-1, -1, -1]]


def test_pack_materials_offsets_and_sizes():
    from pointdreamer_amd.sample_colored_pc_from_mesh import pack_materials
    fx = sc.fixture()
    texels, off, wh, kd = pack_materials(fx['materials'], 'cpu')
    assert texels.dtype == torch.uint8 and off.dtype == torch.int64 and wh.dtype == torch.int32 and kd.dtype == torch.float32
    assert texels.numel() == 16 * 32 * 3 + 8 * 8 * 3
    assert off.tolist() == [0, 1536, 1536] and wh.tolist() == [[32, 16], [0, 0], [8, 8]]
    assert np.array_equal(kd[1].numpy(), fx['materials'][1]['Kd']) and kd[0].tolist() == [0, 0, 0]
    assert np.array_equal(texels[:1536].numpy().reshape(16, 32, 3), fx['materials'][0]['map_Kd'])        # rows as the file stores them
    assert np.array_equal(texels[1536:].numpy().reshape(8, 8, 3), fx['materials'][2]['map_Kd'])
    t2, o2, w2, k2 = pack_materials([{'Kd': np.array([1, 0, 0], np.float32)}], 'cpu')
    assert t2.numel() == 0 and o2.tolist() == [0] and w2.tolist() == [[0, 0]] and k2.tolist() == [[1, 0, 0]]
    with pytest.raises(ValueError):
        pack_materials([], 'cpu')


def test_npy_round_trip_keeps_dtypes_and_large_face_indices(tmp_path):
    from pointdreamer_amd.sample_colored_pc_from_mesh import save_one_mesh_npy, load_pc_npy, NPY_FILES
    n = 5
    rng = np.random.default_rng(0)
    colors = np.array([[0.0, 1.0, 0.5], [254.9 / 255, 0.999, 1 / 255], [0.2, 0.4, 0.6], [0.003, 0.996, 0.75], [1, 1, 1]], np.float32)
    inp = dict(coords=torch.from_numpy(rng.normal(size=(n, 3))), colors=torch.from_numpy(colors), normals=rng.normal(size=(n, 3)),
               uvs=rng.normal(size=(n, 2)), material_idx=np.array([0, 1, 254, 3, 4], np.int32),
               face_idx=torch.tensor([0, 255, 256, 70000, 4000000], dtype=torch.int32), name='cls/shape')
    d = save_one_mesh_npy(inp, str(tmp_path))
    assert d == os.path.join(str(tmp_path), 'cls', 'shape') and sorted(os.listdir(d)) == sorted(NPY_FILES)
    coords, cols, mat, fid, uvs = load_pc_npy(d)
    assert coords.dtype == np.float32 and uvs.dtype == np.float32 and np.load(os.path.join(d, 'normals.npy')).dtype == np.float32
    assert np.array_equal(coords, inp['coords'].numpy().astype('f4')) and uvs.shape == (n, 2)
    assert fid.dtype == np.int32 and fid.tolist() == [0, 255, 256, 70000, 4000000]          # (uint8, the reference's cast, would wrap)
    assert mat.dtype == np.uint8 and mat.tolist() == [0, 1, 254, 3, 4]
    assert cols.dtype == np.uint8 and np.array_equal(cols, (colors * 255).astype(np.uint8))
    assert cols[0].tolist() == [0, 255, 127] and cols[1, 0] == 254                          # truncated, not rounded


# ----------------------------------------------------------------------------- the oracle itself
def test_oracle_samples_lie_inside_their_faces():
    """Barycentric recomputation in float64: every oracle position lies in its face's plane and inside the triangle, up to the float32
    rounding of the position (a few u of the edge lengths)."""
    fx, ref = sc.fixture_reference()
    v = fx['verts'].astype(np.float64)[fx['faces'][ref['face']]]
    p = ref['coords'].astype(np.float64)
    e1, e2, d = v[:, 1] - v[:, 0], v[:, 2] - v[:, 0], p - v[:, 0]
    n = np.cross(e1, e2)
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    assert np.abs((d * n).sum(1)).max() < 8 * sc.U
    G = np.stack([np.stack([(e1 * e1).sum(1), (e1 * e2).sum(1)], -1), np.stack([(e1 * e2).sum(1), (e2 * e2).sum(1)], -1)], -2)
    uv = np.linalg.solve(G, np.stack([(d * e1).sum(1), (d * e2).sum(1)], -1)[..., None])[..., 0]
    tol = 64 * sc.U
    assert uv.min() > -tol and (uv.sum(1) < 1 + tol).all()
    assert np.abs(uv[:, 0] - ref['u']).max() < tol and np.abs(uv[:, 1] - ref['v']).max() < tol


def test_oracle_never_draws_a_dropped_or_degenerate_face():
    fx, ref = sc.fixture_reference()
    w = np.array(ref['weights'], dtype=object)
    assert all(w[f] > 0 for f in ref['face']) and fx['keep'][ref['face']].all()
    verts = fx['verts'].copy()
    faces = fx['faces'].copy()
    faces[5] = [faces[5, 0], faces[5, 0], faces[5, 1]]                                     # a zero-area face among the kept ones
    r2 = sc.sample_reference(verts, faces, None, None, None, fx['keep'], fx['rand'])
    assert r2['weights'][5] == 0 and fx['keep'][5] and 5 not in set(r2['face'].tolist())
    assert sum(1 for x in r2['weights'] if x == 0) == int((~fx['keep']).sum()) + 1
    # the CDF is strictly increasing exactly on the drawable faces, and the end points of the uniform range land on real faces
    f0, _ = sc.draw_faces(ref['cdf'], np.array([0.0, np.nextafter(np.float32(1), np.float32(0))], np.float32))
    assert f0[0] == 1 and ref['weights'][0] == 0 and f0[1] == 319                          # (face 0 is dropped: t = 0 goes to face 1)


def test_fixture_facts_the_gpu_tests_rely_on():
    """The margin, the hit counts and the CDF's width as recorded: a change of fixture cannot silently weaken the GPU tests."""
    fx, ref = sc.fixture_reference()
    assert ref['cdf'][-1].bit_length() == 48
    assert min(ref['margin']) == 84606621 and min(ref['margin']) > fx['faces'].shape[0]
    assert len(set(ref['face'].tolist())) == 274
    assert (np.bincount(ref['material'], minlength=3) > 1300).all()
    assert int((np.asarray(fx['face_uvs_idx'])[ref['face']] < 0).all(1).sum()) > 100         # faces without UVs are drawn too
    assert (fx['uvs'].min() < -0.3) and (fx['uvs'].max() > 1.3)                               # the wrap is exercised
    assert 0.5 < sc.min_corner_sine(fx['verts'], fx['faces']) <= 1.0


def test_oracle_lookup_matches_grid_sample():
    """lookup64 against torch's grid_sample (float64, align_corners=False, border padding) fed as the reference feeds it (:161-170)."""
    fx, ref = sc.fixture_reference()
    img = fx['materials'][0]['map_Kd']
    uv = ref['uvs'].astype(np.float64)
    got, _, _ = sc.lookup64(img, uv)
    g = torch.from_numpy((uv % 1) * 2 - 1)
    g[:, 1] = -g[:, 1]
    tex = torch.from_numpy(img.astype(np.float64) / 255.0).permute(2, 0, 1)[None]
    want = torch.nn.functional.grid_sample(tex, g.reshape(1, 1, -1, 2), mode='bilinear', align_corners=False, padding_mode='border')
    assert np.abs(got - want[0, :, 0, :].permute(1, 0).numpy()).max() < 1e-12


def test_fan_areas_span_one_to_a_hundred():
    verts, faces = sc.fan()
    A = sc.face_areas64(verts, faces)
    assert len(A) == 20 and abs(A.max() / A.min() - 100.0) < 1e-3 and (np.diff(A) > 0).all()
