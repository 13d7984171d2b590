"""pdhip_shade_views_materials (csrc/render.hip) and the multi-material renderers of camera_utils on the GPU: parity against the
float64 reference of tests/render_materials_common.py fed with the device's own face_idx / barycentrics under the per-pixel bound
derived there, the material image and the 8-bit output, an orientation check that needs no oracle, agreement with the one-atlas
kernel, lighting, OBJ + MTL files through both routes of render_textured_mesh, and the render_meshes CLI on a three-material
shape.  The largest measured error / bound ratios are printed (run with -s); profiles/render_materials_parity.txt keeps a copy."""
import os

import numpy as np
import PIL.Image
import pytest
import torch

import render_common as rc
import render_materials_common as rmc

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def note(line):
    print(line)


@pytest.fixture(scope="module")
def scene():
    """The fixture on the device, its device raster from three cameras and the float64 reference of the unlit render, computed once."""
    import pointdreamer_amd.camera_utils as cu
    from pointdreamer_amd.extract_texture_map import rasterize
    from pointdreamer_amd.sample_colored_pc_from_mesh import pack_materials
    fx = rmc.fixture()
    cams, _, _, _ = cu.create_cameras(fx['V'], 1.6, fx['R'], device=DEV)
    pos, cp = cu._clip_positions(cams, T(fx['verts']))
    fidx, bary, _, hard = rasterize(pos, T(fx['faces']), fx['R'])
    s = dict(fx=fx, cams=cams, fidx=fidx, bary=bary, hard=hard, cp=cp, fid_np=fidx.cpu().numpy(), bary_np=bary.cpu().numpy().astype(np.float64),
             cp_np=cp.cpu().numpy(), uvs=T(fx['uvs']), ft=T(fx['face_uvs_idx']), fm=T(fx['face_material']),
             packed=pack_materials(fx['materials'], DEV))
    s['ref'] = rmc.reference(s['fid_np'], s['bary_np'], fx['uvs'], fx['face_uvs_idx'], fx['face_material'], fx['materials'])
    return s


def shade(s, **kw):
    import pointdreamer_amd.camera_utils as cu
    return cu.shade_views_materials(s['fidx'], s['bary'], s['uvs'], s['ft'], s['fm'], s['packed'], **kw)


# ----------------------------------------------------------------------------- 1. parity
def test_parity_within_the_derived_bound(scene):
    """|kernel - float64 reference| <= 2 e_t D + 6 * 2^-24 per covered pixel and channel outside the seam pixels, e_t = 12 max(W,H) M
    2^-24 (derivation: render_materials_common); 6 * 2^-24 on the pixels of the faces without vt records; Kd pixels equal mat_kd and
    uncovered pixels equal 0 bit for bit; at most 0.5 % of the covered pixels are left out."""
    s, ref = scene, scene['ref']
    images, _ = shade(s)
    img = images.permute(0, 2, 3, 1).cpu().numpy()
    covered = int(ref['mask'].sum())
    assert covered > 1000 and ref['images'].std() > 0.1
    assert ref['excluded'].sum() <= rmc.CAP * covered, (int(ref['excluded'].sum()), covered)
    err = np.abs(img.astype(np.float64) - ref['albedo']).max(-1)
    keep = ref['mask'] & ~ref['excluded']
    textured = keep & (ref['material'] != 1)
    ratio = (err[textured] / ref['bound'][textured]).max()
    note(f'materials parity (V=3 R=64, 32x16 + Kd + 8x8, uv in [{ref["uv"].min():.2f},{ref["uv"].max():.2f}]): '
         f'{int(ref["excluded"].sum())} of {covered} covered pixels left out, max error {err[keep].max():.3e}, max error/bound {ratio:.4f}')
    for m in range(3):
        assert (ref['material'] == m).sum() > 200
    assert ref['same3'].sum() > 0
    assert np.all(err[keep] <= ref['bound'][keep]), ratio
    kd = ref['material'] == 1
    assert np.all(img[kd] == np.asarray(s['fx']['materials'][1]['Kd'], np.float32))
    assert np.all(img[~ref['mask']] == 0)
    again, _ = shade(s)
    assert torch.equal(images, again)


# ----------------------------------------------------------------------------- 2. material_idx and the 8-bit output
def test_material_idx_alpha_and_rgba_are_exact(scene):
    s = scene
    images, rgba, midx = shade(s, want_rgba=True, want_material_idx=True)
    want = torch.where(s['fidx'] >= 0, s['fm'][s['fidx'].clamp_min(0)].to(torch.int32), torch.full_like(s['fidx'], -1, dtype=torch.int32)).flip(1)
    assert midx.dtype == torch.int32 and torch.equal(midx, want)
    assert torch.equal(midx.cpu(), torch.from_numpy(scene['ref']['material']).to(torch.int32))
    mask = s['hard'].flip(1).cpu().numpy()
    got = rgba.cpu().numpy()
    assert np.array_equal(got[..., 3], np.where(mask, 255, 0).astype(np.uint8))              # alpha = rasterize()'s hard mask, flipped
    img = images.permute(0, 2, 3, 1).cpu().numpy()
    assert np.array_equal(got[..., :3], np.clip(np.rint(img * np.float32(255)), 0, 255).astype(np.uint8))
    assert np.all(got[~mask] == 0)
    only, alone = shade(s, want_images=False, want_rgba=True)
    assert only is None and torch.equal(alone, rgba)


# ----------------------------------------------------------------------------- 3. orientation, no oracle
@pytest.mark.parametrize("R,image", [
    (8, [[[255, 0, 0], [255, 0, 0], [0, 255, 0], [0, 255, 0]], [[0, 0, 255], [0, 0, 255], [255, 255, 128], [255, 255, 128]]]),
    (16, [[[255, 0, 0], [10, 20, 30], [40, 50, 60], [0, 255, 0]], [[0, 0, 255], [70, 80, 90], [100, 110, 120], [255, 255, 128]]]),
], ids=["8x8-view", "16x16-view"])
def test_quad_corners_show_the_expected_texels_of_a_non_square_image(R, image):
    """The quad of test_gpu_render.test_quad_corners_show_the_expected_texels (camera on the -z axis: right = -x, up = +y, so the
    top-left covered pixel shows world (+x,+y); UV (0,0) at world (-x,-y), (1,1) at (+x,+y)) with its two faces on two materials:
    a 4 x 2 image (W = 4, H = 2) and a Kd.  v is negated and image row 0 is the top, so v ~ 1 shows row 0 and u ~ 1 shows column 3:
    top-left = image[0,3], top-right = image[0,0], bottom-left = image[1,3], bottom-right = image[1,0].  Face 0 = (0,1,2) owns the
    bottom-left corner, face 1 = (0,2,3) the top-right one, the two corners on the diagonal go to either: each run checks every
    corner against the material the kernel reports for it, and the two assignments together show all four corner texels.
    A swapped W / H (stride 2 instead of 4) or a missing flip shows other texels.

    Exact texels need the corner pixel's centre inside the clamped border half-texel.  With H = 2 that holds at any view size; with
    W = 4 the half-texel is 1/8 of the quad, while at 8 x 8 the corner centres sit 0.19 of the quad's width inside it.  So the
    8 x 8 view of the issue uses an image whose columns 0-1 and 2-3 are equal (the blend of equal texels is exact), and a 16 x 16
    view (corner centres 0.03 inside) shows eight distinct texels exactly."""
    import pointdreamer_amd.camera_utils as cu
    cams, _, _, _ = cu.create_cameras(6, 1.6, R, distribution='self_defined', device=DEV)
    verts = T(np.array([[-.4, -.4, 0], [.4, -.4, 0], [.4, .4, 0], [-.4, .4, 0]], np.float32))
    faces = T(np.array([[0, 1, 2], [0, 2, 3]], np.int64))
    uvs = T(np.array([[0, 0], [1, 0], [1, 1], [0, 1]], np.float32))
    image = np.array(image, np.uint8)
    assert image.shape == (2, 4, 3)
    kd = np.array([0.125, 0.375, 0.625], np.float32)
    materials = [{'name': 'img', 'map_Kd': image}, {'name': 'flat', 'Kd': kd}]
    texel = lambda r, c: image[r, c].astype(np.float32) / np.float32(255.0)
    shown = set()
    for fm in ([0, 1], [1, 0]):
        img, mask = cu.render_material_mesh(verts, faces, uvs, faces, T(np.array(fm, np.int32)), materials, cams[:1], return_mask=True)
        pos, _ = cu._clip_positions(cams[:1], verts)
        from pointdreamer_amd.extract_texture_map import rasterize
        fidx, bary, _, _ = rasterize(pos, faces, R)
        _, _, midx = cu.shade_views_materials(fidx, bary, uvs, faces, T(np.array(fm, np.int32)), materials, want_material_idx=True)
        img, mask, midx = img[0].permute(1, 2, 0).cpu().numpy(), mask[0].cpu().numpy(), midx[0].cpu().numpy()
        assert img.shape == (R, R, 3) and 9 <= mask.sum() < R * R
        rows, cols = np.nonzero(mask.any(1))[0], np.nonzero(mask.any(0))[0]
        t, b, l, r = rows[0], rows[-1], cols[0], cols[-1]
        assert mask[t, l] and mask[t, r] and mask[b, l] and mask[b, r]
        assert midx[b, l] == fm[0] and midx[t, r] == fm[1]                                # the corners off the diagonal: one owner each
        for (i, j), (row, col) in (((t, l), (0, 3)), ((t, r), (0, 0)), ((b, l), (1, 3)), ((b, r), (1, 0))):
            if midx[i, j] == 0:
                assert np.array_equal(img[i, j], texel(row, col)), (fm, i, j, img[i, j])
                shown.add((row, col))
            else:
                assert midx[i, j] == 1 and np.array_equal(img[i, j], kd), (fm, i, j)
        assert np.all(img[midx == 1] == kd)                                                # the Kd face shows its colour exactly
        assert np.all(img[~mask] == 0) and np.all(midx[~mask] == -1)
    assert shown == {(0, 3), (0, 0), (1, 3), (1, 0)}


# ----------------------------------------------------------------------------- 4. agreement with the one-atlas kernel
def test_one_square_material_agrees_with_the_one_atlas_kernel(scene):
    """One material with a square 32 x 32 u8 image against shade_views with atlas = flip(image) / 255: the two kernels evaluate the
    same function in different operation orders, so they differ by at most the sum of their bounds outside both seam sets."""
    import pointdreamer_amd.camera_utils as cu
    s, fx = scene, scene['fx']
    image = np.random.default_rng(23).integers(0, 256, size=(32, 32, 3), dtype=np.uint8)
    materials = [{'name': 'one', 'map_Kd': image}]
    faces = T(fx['faces'])
    a, _ = cu.shade_views_materials(s['fidx'], s['bary'], s['uvs'], faces, None, materials)
    atlas = T(image[::-1].astype(np.float32) / np.float32(255.0))                          # (divided on the host: t / 255.0f as the kernel rounds it)
    b, _ = cu.shade_views(s['fidx'], s['bary'], s['uvs'], faces, atlas=atlas)
    ref_m = rmc.reference(s['fid_np'], s['bary_np'], fx['uvs'], fx['faces'], np.zeros(320, np.int32), materials)
    ref_a = rc.render_reference(s['fid_np'], s['bary_np'], fx['uvs'], fx['faces'], atlas=atlas.cpu().numpy())
    bound_a, e_a = rc.texture_bound(ref_a, 32)
    ex = ref_m['excluded'] | rc.wrap_excluded(ref_a, 32, e_a)
    assert np.array_equal(ref_m['mask'], ref_a['mask']) and ex.sum() <= 2 * rmc.CAP * ref_m['mask'].sum()
    # the two float64 references agree up to the float32 rounding of the atlas texels (the `u` for t/255.0f inside the 6u)
    assert np.abs(ref_m['albedo'] - ref_a['albedo'])[~ex].max() <= rmc.U
    bound = ref_m['bound'] + bound_a
    err = (a - b).abs().permute(0, 2, 3, 1).cpu().numpy().astype(np.float64).max(-1)
    keep = ref_m['mask'] & ~ex
    ratio = (err[keep] / bound[keep]).max()
    note(f'one 32x32 material against the one-atlas kernel: {int(ex.sum())} pixels left out, max difference {err[keep].max():.3e}, '
         f'max difference / (sum of the two bounds) {ratio:.4f}')
    assert a.std() > 0.1 and np.all(err[keep] <= bound[keep]), ratio
    assert np.all(a.permute(0, 2, 3, 1).cpu().numpy()[~ref_m['mask']] == 0)


# ----------------------------------------------------------------------------- 5. lighting
@pytest.mark.parametrize("double_side", [False, True])
def test_lighting_within_the_bound_before_and_after_gamma(scene, double_side):
    """The bound and the treatment of test_gpu_render.test_lighting_within_the_bound_before_and_after_gamma: before the power
    (albedo bound) * sum_l clip(n.l) + render_common.light_rounding; after it only values >= 1e-3, with the slope of x ** (1/2.2) at
    the lower end of [ref - bound, ref + bound] plus 4 * 2^-24."""
    import pointdreamer_amd.camera_utils as cu
    s, fx = scene, scene['fx']
    fn = cu.face_normals_unit(T(fx['verts']), T(fx['faces']))
    kw = dict(face_normals=fn, cam_params=s['cp'], light_dirs=T(fx['lights']), double_side=double_side)
    pre, _ = shade(s, **kw)
    post, _ = shade(s, gamma=2.2, **kw)
    ref = rmc.reference(s['fid_np'], s['bary_np'], fx['uvs'], fx['face_uvs_idx'], fx['face_material'], fx['materials'],
                        normals=fn.cpu().numpy(), cam_params=s['cp_np'], lights=fx['lights'], double_side=double_side, gamma=2.2)
    flat = ref['mask'] & (np.abs(ref['ndotcam']) < 1e-6)
    assert flat.sum() <= 0.01 * ref['mask'].sum() and ref['excluded'].sum() <= rmc.CAP * ref['mask'].sum()
    ex = flat | ref['excluded']
    bound = (ref['bound'] * ref['clipsum'] + rc.light_rounding(fx['lights'], 1.0))[:, None]
    keep = np.broadcast_to((ref['mask'] & ~ex)[:, None], ref['images'].shape)
    err = np.abs(pre.cpu().numpy().astype(np.float64) - ref['pre_gamma'])
    r1 = (err / bound)[keep].max()
    assert np.all((err <= bound)[keep]), r1
    big = keep & (ref['pre_gamma'] >= 1e-3)
    lo = np.maximum(ref['pre_gamma'] - bound, 5e-4)
    bound2 = (1 / 2.2) * lo ** (1 / 2.2 - 1) * bound + 4 * rc.U
    err2 = np.abs(post.cpu().numpy().astype(np.float64) - ref['images'])
    r2 = (err2 / bound2)[big].max()
    note(f'materials lighting parity (3 lights, double_side={double_side}): {int(ex.sum())} pixels left out, max error/bound {r1:.4f} '
         f'before gamma, {r2:.4f} after gamma 2.2 ({int(big.sum())} values >= 1e-3)')
    assert big.sum() > 1000 and ref['pre_gamma'].max() > 0.3
    assert np.all((err2 <= bound2)[big]), r2
    assert np.all(post.permute(0, 2, 3, 1).cpu().numpy()[~ref['mask']] == 0)


# ----------------------------------------------------------------------------- 6. files
def test_files_render_like_their_tensors_on_both_routes(scene, tmp_path):
    import pointdreamer_amd.camera_utils as cu
    s, fx = scene, scene['fx']
    verts, faces = T(fx['verts']), T(fx['faces'])
    mask = s['hard'].flip(1).cpu().numpy()
    # three materials: OBJ (%.9g) + MTL + two PNGs -> the new route, bit for bit what render_material_mesh gives on the tensors
    three = tmp_path / 'three.obj'
    rmc.write_obj(three, fx['verts'], fx['faces'], fx['uvs'], fx['face_uvs_idx'], fx['face_material'], fx['materials'])
    assert sorted(os.listdir(tmp_path)) == ['three.mtl', 'three.obj', 'three_m0.png', 'three_m2.png']
    keep = verts.clone()
    want = cu.render_material_mesh(verts, faces, s['uvs'], s['ft'], s['fm'], fx['materials'], s['cams'])
    got = cu.render_textured_mesh(str(three), s['cams'], DEV, None, save=False, normalize_mesh=False)
    assert torch.equal(got, want) and got.std() > 0.1
    images, _ = shade(s)
    assert torch.equal(got, images)                                                        # (the same raster, the same kernel)
    assert torch.equal(cu.render_textured_mesh_w_mask(str(three), s['cams'], DEV, None, save=False, normalize_mesh=False), want)
    lit = dict(light_dirs=T(fx['lights']), gamma=2.2, double_side=True)
    assert torch.equal(cu.render_textured_mesh(str(three), s['cams'], DEV, None, save=False, normalize_mesh=False, **lit),
                       cu.render_material_mesh(verts, faces, s['uvs'], s['ft'], s['fm'], fx['materials'], s['cams'], **lit))
    norm = cu.render_textured_mesh(str(three), s['cams'], DEV, None, save=False, vertices=verts * 3.0)      # normalize_mesh=True
    assert torch.equal(verts, keep) and tuple(norm.shape) == (3, 3, 64, 64) and norm.std() > 0.1
    geo = cu.render_textured_mesh(str(three), s['cams'], DEV, str(tmp_path / 'geo'), normalize_mesh=False, geo_only=True, color=[0.25, 0.5, 0.75])
    geo = geo.permute(0, 2, 3, 1).cpu().numpy()
    assert np.all(geo[mask] == np.array([0.25, 0.5, 0.75], np.float32)) and np.all(geo[~mask] == 0)
    png = np.array(PIL.Image.open(tmp_path / 'geo' / 'albedo_003.png'))
    assert png.shape == (64, 64, 4) and np.array_equal(png[..., 3] == 255, mask[2]) and np.all(png[mask[2]][:, :3] == [64, 128, 191])
    # one material, square image: the old route and its bits (render_textured_mesh2 with the image flipped back)
    sq = np.random.default_rng(29).integers(0, 256, size=(32, 32, 3), dtype=np.uint8)
    one = tmp_path / 'one.obj'
    rmc.write_obj(one, fx['verts'], fx['faces'], fx['uvs'], fx['faces'], None, [{'name': 'a', 'map_Kd': sq}])
    old = cu.render_textured_mesh2(verts, faces, s['uvs'], faces, T(sq[::-1]).float() / 255., s['cams'])
    got1 = cu.render_textured_mesh(str(one), s['cams'], DEV, None, save=False, normalize_mesh=False)
    assert torch.equal(got1, old) and got1.std() > 0.1
    # one material, 32 x 16 image: load_textured_obj still refuses it, render_textured_mesh takes the new route
    wide = tmp_path / 'wide.obj'
    rmc.write_obj(wide, fx['verts'], fx['faces'], fx['uvs'], fx['faces'], None, [fx['materials'][0]])
    with pytest.raises(NotImplementedError, match='square'):
        cu.load_textured_obj(str(wide), DEV)
    got2 = cu.render_textured_mesh(str(wide), s['cams'], DEV, None, save=False, normalize_mesh=False)
    want2 = cu.render_material_mesh(verts, faces, s['uvs'], faces, None, [fx['materials'][0]], s['cams'])
    assert torch.equal(got2, want2) and got2.std() > 0.1 and np.all(got2.permute(0, 2, 3, 1).cpu().numpy()[~mask] == 0)


# ----------------------------------------------------------------------------- 7. the CLI
def test_render_meshes_cli_renders_a_three_material_shape(scene, tmp_path):
    """<root>/meshes/<cls>/<shape>/models/model_normalized.obj with three materials -> 20 RGBA views at 1024^2 showing all three;
    a second run finds the 20 files and renders nothing."""
    from pointdreamer_amd import render_meshes
    fx = scene['fx']
    models = tmp_path / 'meshes' / 'cls' / 'ball' / 'models'
    os.makedirs(models)
    rmc.write_obj(models / 'model_normalized.obj', fx['verts'], fx['faces'], fx['uvs'], fx['face_uvs_idx'], fx['face_material'], fx['materials'])
    assert render_meshes.main(['--rootpath', str(tmp_path), '--by', 'kaolin']) == 1
    out = tmp_path / 'rendered_imgs' / 'cls' / 'ball'
    assert sorted(os.listdir(out)) == [f'albedo_{i:03d}.png' for i in range(1, 21)]
    # what the CLI's route computes for the first view, from the tensors: the PNG is that image rounded, alpha its coverage
    import pointdreamer_amd.camera_utils as cu
    cams, _, _, _ = cu.create_cameras(num_views=20, distance=1.6, res=1024, device=DEV, distribution='self_defined')
    args = (T(fx['verts']), T(fx['faces']), T(fx['uvs']), T(fx['face_uvs_idx']), T(fx['face_material']))
    want, mask = cu.render_material_mesh(*args, fx['materials'], cams[:1], normalize_mesh=True, return_mask=True)
    tag = [{'name': 'r', 'Kd': np.array([1, 0, 0], np.float32)}, {'name': 'g', 'Kd': np.array([0, 1, 0], np.float32)},
           {'name': 'b', 'Kd': np.array([0, 0, 1], np.float32)}]
    which = cu.render_material_mesh(*args, tag, cams[:1], normalize_mesh=True)[0].permute(1, 2, 0).cpu().numpy()      # one-hot material
    want, mask = want[0].permute(1, 2, 0).cpu().numpy(), mask[0].cpu().numpy()
    kd = np.clip(np.rint(np.asarray(fx['materials'][1]['Kd'], np.float32) * np.float32(255)), 0, 255).astype(np.uint8)
    for name in (f'albedo_{i:03d}.png' for i in range(1, 21)):
        im = np.array(PIL.Image.open(out / name))
        assert im.shape == (1024, 1024, 4) and set(np.unique(im[..., 3])) == {0, 255} and 0.2 < (im[..., 3] == 255).mean() < 0.9, name
        assert np.all(im[im[..., 3] == 0] == 0), name
    im = np.array(PIL.Image.open(out / 'albedo_001.png'))
    assert np.array_equal(im[..., 3] == 255, mask)
    assert np.array_equal(im[..., :3], np.clip(np.rint(want * np.float32(255)), 0, 255).astype(np.uint8))
    for m in range(3):                                                                     # colours of all three materials are present
        sel = which[..., m] == 1
        assert sel.sum() > 0.05 * mask.sum(), m
        if m == 1:
            assert np.all(im[..., :3][sel] == kd)
        else:
            assert im[..., :3][sel].std() > 20 and len(np.unique(im[..., :3][sel], axis=0)) > 100, m
    assert render_meshes.main(['--rootpath', str(tmp_path), '--by', 'kaolin']) == 0
