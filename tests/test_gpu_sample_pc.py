"""pdhip_sample_mesh (csrc/sample_mesh.hip) and pointdreamer_amd/sample_colored_pc_from_mesh.py on the GPU against the CPU oracle of
tests/sample_pc_common.py (its docstring has the error model): the face choice through the integer CDF, float32 positions and UVs bit
for bit, normals and colours under derived bounds, the tile hand-off of the uint64 scan, the distribution, repeatability, the refusals,
the visibility composition against the oracle's stages and the batch driver.  Measured ratios are printed (run with -s);
profiles/sample_pc_parity.txt keeps a copy."""
import logging
import os

import numpy as np
import PIL.Image
import pytest
import torch

import sample_pc_common as sc

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
KEYS = ('coords', 'face_idx', 'material_idx', 'uvs', 'colors', 'normals')


def run(fx, rand=None, **over):
    from pointdreamer_amd.sample_colored_pc_from_mesh import sample_points
    a = dict(fx, **over)
    rand = a['rand'] if rand is None else rand
    return sample_points(T(a['verts']), T(a['faces']), None if a['uvs'] is None else T(a['uvs']),
                         None if a['face_uvs_idx'] is None else T(a['face_uvs_idx']),
                         None if a['face_material'] is None else T(a['face_material']), a['materials'], len(rand),
                         face_keep=None if a['keep'] is None else T(a['keep']), rand=T(rand))


@pytest.fixture(scope="module")
def drawn():
    """The fixture, its oracle draw and the device's outputs as numpy arrays, computed once."""
    fx, ref = sc.fixture_reference()
    out = run(fx)
    torch.cuda.synchronize()
    return fx, ref, {k: v.cpu().numpy() for k, v in out.items()}, out


def faces_agree(got, ref, F):
    """The margin rule: equal everywhere, except (tolerated) where the oracle's own margin is below F weight units.  Returns the number
    of samples left out."""
    close = np.array([m < F for m in ref['margin']])
    bad = (got != ref['face']) & ~close
    assert not bad.any(), (np.nonzero(bad)[0][:8], got[bad][:8], ref['face'][bad][:8])
    return int(close.sum())


def test_faces_and_materials_equal_the_oracle(drawn):
    fx, ref, got, _ = drawn
    assert got['face_idx'].dtype == np.int32 and got['material_idx'].dtype == np.int32
    left_out = faces_agree(got['face_idx'], ref, fx['faces'].shape[0])
    assert left_out == 0                                                   # on this fixture the oracle puts no sample near a boundary
    assert np.array_equal(got['face_idx'], ref['face']) and np.array_equal(got['material_idx'], ref['material'])
    assert fx['keep'][got['face_idx']].all()                               # indices are those of the caller's faces, dropped ones never drawn


def test_positions_and_uvs_equal_the_float32_oracle_bit_for_bit(drawn):
    fx, ref, got, _ = drawn
    assert np.array_equal(got['coords'].view(np.uint32), ref['coords'].view(np.uint32))
    assert np.array_equal(got['uvs'].view(np.uint32), ref['uvs'].view(np.uint32))
    none = (fx['face_uvs_idx'][ref['face']] < 0).all(1)
    assert none.sum() > 100 and (got['uvs'][none] == 0).all()              # a face without vt records looks up uv = (0, 0)
    assert got['uvs'].min() < 0 and got['uvs'].max() > 1                   # stored before the wrap


def test_normals_within_the_derived_bound(drawn):
    """13 roundings (6 per cross-product component relative to |e1||e2|, i.e. 6u / sin(theta) of the unit normal, the other two
    components through the norm, then 3.5u for the norm and 1 for the division): below 16u / sin(theta_min)."""
    fx, ref, got, _ = drawn
    bound = 16 * sc.U / sc.min_corner_sine(fx['verts'], fx['faces'])
    err = np.abs(got['normals'].astype(np.float64) - ref['normals']).max()
    print(f"normals: max error {err / sc.U:.2f} u, bound {bound / sc.U:.2f} u")
    assert err <= bound
    assert np.abs(np.linalg.norm(got['normals'].astype(np.float64), axis=1) - 1).max() < 4 * sc.U


def test_colours_kd_exact_and_textures_within_the_derived_bound(drawn):
    fx, ref, got, _ = drawn
    kd = ref['material'] == 1
    assert kd.sum() > 1300 and np.array_equal(got['colors'][kd].view(np.uint32),
                                              np.broadcast_to(fx['materials'][1]['Kd'], (int(kd.sum()), 3)).copy().view(np.uint32))
    for m in (0, 2):
        sel = ref['material'] == m
        img = fx['materials'][m]['map_Kd']
        want, x0, y0 = sc.lookup64(img, got['uvs'][sel].astype(np.float64))
        bound = sc.colour_bound(img, x0, y0)
        err = np.abs(got['colors'][sel].astype(np.float64) - want).max(1)
        print(f"material {m} ({img.shape[1]} x {img.shape[0]}): {int(sel.sum())} samples, max error {err.max() / sc.U:.2f} u, "
              f"max error / bound {(err / bound).max():.3f}")
        assert sel.sum() > 1300 and (err <= bound).all()
        assert got['colors'][sel].min() >= 0 and got['colors'][sel].max() <= 1


def test_scan_hand_off_over_three_tiles():
    """icosphere(16), 5120 faces = three scan tiles of 2048, the whole second tile's worth of faces dropped: every later CDF entry
    depends on the tile sums being carried over."""
    from pointdreamer_amd import synthetic
    verts, faces = synthetic.icosphere(16)
    F = faces.shape[0]
    assert F == 5120
    keep = np.ones(F, bool)
    keep[2048:4096] = False
    rand = torch.rand((4096, 3), generator=torch.Generator().manual_seed(23)).numpy()
    ref = sc.sample_reference(verts, faces, None, None, None, keep, rand)
    assert sum(1 for m in ref['margin'] if m < F) <= 2                     # (more: change the seed, not the cap)
    fx = dict(verts=verts, faces=faces, uvs=None, face_uvs_idx=None, face_material=None, keep=keep,
              materials=[{'Kd': np.array([0.1, 0.2, 0.3], np.float32)}], rand=rand)
    out = run(fx)
    got = out['face_idx'].cpu().numpy()
    left_out = faces_agree(got, ref, F)
    print(f"three tiles: {left_out} samples left out by the margin rule, {len(set(got.tolist()))} faces hit")
    assert keep[got].all() and (got >= 4096).sum() > 1000 and (got < 2048).sum() > 1000
    assert np.array_equal(out['coords'].cpu().numpy()[got == ref['face']].view(np.uint32), ref['coords'][got == ref['face']].view(np.uint32))
    assert (out['material_idx'] == 0).all() and (out['uvs'] == 0).all()


def test_distribution_follows_the_areas():
    """A 20-face fan with areas 1 : 100, 200 000 seeded samples: every face's count within 5 sigma of N A_f / sum(A), sigma the binomial
    sqrt(N p (1 - p)).  Derived: at 5 sigma a correct sampler fails one face in 1.7 million, 20 faces in 87 000 seeds."""
    verts, faces = sc.fan()
    A = sc.face_areas64(verts, faces)
    p = A / A.sum()
    N = 200000
    from pointdreamer_amd.sample_colored_pc_from_mesh import sample_points
    out = sample_points(T(verts), T(faces), None, None, None, [{'Kd': np.zeros(3, np.float32)}], N,
                        generator=torch.Generator().manual_seed(5))
    counts = np.bincount(out['face_idx'].cpu().numpy(), minlength=20)
    z = (counts - N * p) / np.sqrt(N * p * (1 - p))
    print("fan: largest |z| =", float(np.abs(z).max()))
    assert counts.sum() == N and (np.abs(z) <= 5).all(), z
    assert (out['coords'][:, 2] == 0).all()


def test_two_calls_give_equal_bits(drawn):
    fx, _, _, first = drawn
    again = run(fx)
    for k in KEYS:
        assert torch.equal(first[k].view(torch.int32), again[k].view(torch.int32)), k


def test_refusals_name_the_cause():
    """Each bad index is exactly one past the end of its table; the area pass never reads through it."""
    from pointdreamer_amd._lib import PdhipError
    from pointdreamer_amd.sample_colored_pc_from_mesh import sample_points
    fx, _ = sc.fixture_reference()
    rand = fx['rand'][:64]
    faces = fx['faces'].copy()
    faces[17, 2] = fx['verts'].shape[0]
    with pytest.raises(PdhipError, match='vertex index'):
        run(fx, rand, faces=faces)
    ft = fx['face_uvs_idx'].copy()
    ft[5, 1] = fx['uvs'].shape[0]
    with pytest.raises(PdhipError, match='uv index'):
        run(fx, rand, face_uvs_idx=ft)
    fm = fx['face_material'].copy()
    fm[300] = 3
    with pytest.raises(PdhipError, match='material index'):
        run(fx, rand, face_material=fm)
    with pytest.raises(PdhipError, match='no face with positive area'):
        run(fx, rand, keep=np.zeros(320, bool))
    big = torch.zeros(((1 << 22) + 1, 3), dtype=torch.int64, device=DEV)
    with pytest.raises(PdhipError, match=r'2\^22'):
        sample_points(T(fx['verts']), big, None, None, None, fx['materials'][1:2], 64, rand=T(rand))
    out = run(fx, rand)                                                    # the same inputs unbroken still work afterwards
    assert out['coords'].shape == (64, 3)
    empty = run(fx, fx['rand'][:0])                                        # N = 0: OK, nothing written
    assert empty['coords'].shape == (0, 3) and empty['face_idx'].shape == (0,)


# ----------------------------------------------------------------------------- visibility, drivers
def fixture_mesh_data(name='cls/fixture'):
    from pointdreamer_amd.sample_colored_pc_from_mesh import MeshData
    fx, _ = sc.fixture_reference()
    return fx, MeshData(fx['verts'].copy(), fx['faces'], fx['uvs'], fx['face_uvs_idx'], fx['face_material'], fx['materials'], name=name)


def test_visible_sampling_matches_the_oracle_composition():
    """3 oracle-matched cameras at 64^2, point_per_shape = 256: the kept mask over the 1280 drawn samples equals project_batch ->
    rasterize -> point_validation_by_depth (offset 0) -> OR over the views of the oracle bit for bit; the output is 256 distinct rows
    of the kept set; asking for more points than survive raises ValueError; the caller's vertices are untouched."""
    import pointdreamer_amd.camera_utils as cu
    from pointdreamer_amd import sample_colored_pc_from_mesh as sm
    from oracle import camera as ocam, project as oproj
    fx, md = fixture_mesh_data()
    before = md.vertices.copy()
    cams, _, _, _ = cu.create_cameras(3, 1.6, 64, device=DEV)
    ocams, _, _, _ = ocam.create_cameras(3, 1.6, 64)
    seed, pps = 31, 256
    # the function's own draw, replayed: torch.rand((5 pps, 3)) from the generator, on normalised vertices
    rand = torch.rand((5 * pps, 3), generator=torch.Generator().manual_seed(seed))
    verts_n = cu._normalized(T(fx['verts'])).contiguous()
    s = sm.sample_points(verts_n, T(fx['faces']), fx['uvs'], fx['face_uvs_idx'], fx['face_material'], fx['materials'], 5 * pps, rand=rand)
    kept = sm.visible_point_mask(verts_n, T(fx['faces']), s['coords'], cams).cpu().numpy()
    pts = s['coords'].cpu().numpy()
    o = oproj.project_batch(ocams, verts_n.cpu().numpy(), pts, False)
    _, _, od = oproj.rasterize(o['pos'], fx['faces'], 64)
    ovis, _ = oproj.point_validation_by_depth(64, o['point_uvs'], o['point_depths'], od, 0.0)
    assert kept.shape == (1280,) and np.array_equal(kept, ovis.any(0))
    assert 256 <= kept.sum() < 1280
    coords, colors, mat, fid, uvs = sm.sample_one_mesh_w_o_invisible_points(md, pps, cams, DEV, None, generator=torch.Generator().manual_seed(seed))
    assert coords.shape == (256, 3) and colors.shape == (256, 3) and mat.shape == (256,) and fid.shape == (256,) and uvs.shape == (256, 2)
    rows = {r.tobytes(): i for i, r in enumerate(pts)}
    idx = np.array([rows[r.tobytes()] for r in coords])                    # every output row is a drawn sample ...
    assert len(set(idx.tolist())) == 256 and kept[idx].all()              # ... distinct, and of the kept set
    assert np.array_equal(fid, s['face_idx'].cpu().numpy()[idx]) and np.array_equal(colors, s['colors'].cpu().numpy()[idx])
    assert not np.array_equal(idx, np.sort(idx))                           # left in the random order
    assert np.array_equal(md.vertices, before)
    # too few survivors: ten copies of a slightly smaller sphere inside carry 89 % of the area and are hidden by the outer one
    v, f = fx['verts'], fx['faces']
    nested = sm.MeshData(np.concatenate([v] + [v * np.float32(0.9)] * 10), np.concatenate([f + k * len(v) for k in range(11)]),
                         None, None, None, fx['materials'][1:2], name='cls/nested')
    with pytest.raises(ValueError, match=r'cls/nested: \d+ of 320 samples are visible, fewer than the 64'):
        sm.sample_one_mesh_w_o_invisible_points(nested, 64, cams, DEV, None, generator=torch.Generator().manual_seed(1))


def write_shape(root, cls_id, name, layout, broken=False):
    """A tetrahedron-like closed mesh (an octahedron) with two materials, one image and one Kd, in one of the dataset layouts."""
    d = os.path.join(root, 'meshes', cls_id, name, layout[0])
    os.makedirs(d, exist_ok=True)
    v = [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)]
    f = [(1, 3, 5), (3, 2, 5), (2, 4, 5), (4, 1, 5), (3, 1, 6), (2, 3, 6), (4, 2, 6), (1, 4, 6)]
    with open(os.path.join(d, layout[1]), 'w') as fh:
        fh.write('mtllib model.mtl\n' + ''.join(f'v {a} {b} {c}\n' for a, b, c in v) + 'vt 0.1 0.1\nvt 0.9 0.1\nvt 0.5 0.9\n')
        for k, (a, b, c) in enumerate(f):
            fh.write(f"usemtl {'ghost' if broken and k == 3 else ('tex' if k % 2 == 0 else 'flat')}\nf {a}/1 {b}/2 {c}/3\n")
    with open(os.path.join(d, 'model.mtl'), 'w') as fh:
        fh.write('newmtl tex\nmap_Kd tex.png\nnewmtl flat\nKd 0.25 0.5 0.75\n')
    PIL.Image.fromarray(np.random.default_rng(2).integers(0, 256, (6, 10, 3), dtype=np.uint8)).save(os.path.join(d, 'tex.png'))


def test_batch_driver_in_process(tmp_path, caplog):
    from pointdreamer_amd import io_utils
    from pointdreamer_amd import sample_colored_pc_from_mesh as sm
    root = str(tmp_path)
    write_shape(root, 'toys', 'alpha', ('models', 'model_normalized.obj'))
    write_shape(root, 'toys', 'beta', ('Scan', 'Scan.obj'))
    write_shape(root, 'toys', 'gamma', ('meshes', 'model.obj'), broken=True)
    with caplog.at_level(logging.INFO, logger='pointdreamer_amd.sample_pc'):
        done = sm.sample_omniobject3d_batch(root, cls_id='toys', point_num=500, seed=3, ply=True, device=DEV)
    assert done == 2
    errors = [r.getMessage() for r in caplog.records if r.levelno >= logging.ERROR]
    assert any('toys/gamma' in e for e in errors) and any('ghost' in e and 'Traceback' in e for e in errors)
    for name in ('alpha', 'beta'):
        d = os.path.join(root, 'pc_kaolin', 'toys', name)
        assert sorted(os.listdir(d)) == sorted(sm.NPY_FILES)
        want = {'coords.npy': ((500, 3), np.float32), 'colors.npy': ((500, 3), np.uint8), 'normals.npy': ((500, 3), np.float32),
                'uvs.npy': ((500, 2), np.float32), 'material_idx.npy': ((500,), np.uint8), 'face_idx.npy': ((500,), np.int32)}
        for fn, (shape, dt) in want.items():
            a = np.load(os.path.join(d, fn))
            assert a.shape == shape and a.dtype == dt, fn
        coords, colors, mat, fid, _ = sm.load_pc_npy(d)
        assert set(mat.tolist()) == {0, 1} and np.array_equal(mat, fid % 2) and fid.max() < 8      # material = face parity, as written
        assert (colors[mat == 1] == np.array([63, 127, 191], np.uint8)).all()                      # (Kd * 255) truncated
        assert np.abs(coords).max() <= 0.5 + 1e-6                                                  # the unit box
        xyz, rgb = io_utils.read_ply_xyzrgb(os.path.join(root, 'pc_kaolin', 'toys', name + '.ply'))
        assert np.array_equal(xyz, coords) and np.array_equal(rgb, colors)
    assert not os.path.exists(os.path.join(root, 'pc_kaolin', 'toys', 'gamma', 'coords.npy'))
    stamp = {n: os.path.getmtime(os.path.join(root, 'pc_kaolin', 'toys', n, 'coords.npy')) for n in ('alpha', 'beta')}
    caplog.clear()
    with caplog.at_level(logging.INFO, logger='pointdreamer_amd.sample_pc'):
        assert sm.main(['--rootpath', root, '--cls_id', 'toys', '--point_num', '500', '--seed', '3', '--ply']) == 0     # second run: both skipped
    assert sum('skip exist' in r.getMessage() for r in caplog.records) == 2
    assert stamp == {n: os.path.getmtime(os.path.join(root, 'pc_kaolin', 'toys', n, 'coords.npy')) for n in ('alpha', 'beta')}
