"""The shading kernel (csrc/render.hip) and the renderers of camera_utils on the GPU: orientation checks that need no oracle, parity
against the float64 reference of tests/render_common.py fed with the device's own face_idx / barycentrics (both pinned elsewhere)
under the per-pixel bound derived there, wrap, lighting, the 8-bit output, per-vertex colours, a saved-mesh round trip and the demo's
opt-in `render_views` key.  The largest measured error / bound ratios are printed (run with -s); profiles/render_parity.txt keeps a copy."""
import os

import numpy as np
import PIL.Image
import pytest
import torch

import render_common as rc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = 'cuda:0'
T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def note(line):
    print(line)


def device_raster(cams, verts, faces, R):
    import pointdreamer_amd.camera_utils as cu
    from pointdreamer_amd.extract_texture_map import rasterize
    pos, cp = cu._clip_positions(cams, verts)
    fidx, bary, _, hard = rasterize(pos, faces, R)
    return fidx, bary, hard, cp


@pytest.fixture(scope="module")
def scene():
    """Fixture tensors, the device raster of the sphere from three cameras, and the float64 references, computed once."""
    import pointdreamer_amd.camera_utils as cu
    out = {}
    for wrap in (False, True):
        fx = rc.sphere_fixture(wrap)
        cams, _, _, _ = cu.create_cameras(fx['V'], 1.6, fx['R'], device=DEV)
        fidx, bary, hard, cp = device_raster(cams, T(fx['verts']), T(fx['faces']), fx['R'])
        out[wrap] = dict(fx=fx, cams=cams, fidx=fidx, bary=bary, hard=hard, cp=cp, fid_np=fidx.cpu().numpy(),
                         bary_np=bary.cpu().numpy().astype(np.float64), cp_np=cp.cpu().numpy())
    return out


# ----------------------------------------------------------------------------- orientation, no oracle
def test_quad_corners_show_the_expected_texels():
    """One quad in the z = 0 plane seen from the camera on the -z axis (right = -x, up = +y): the top-left covered pixel shows
    world (+x, +y).  UV (0,0) sits at world (-x,-y) and (1,1) at (+x,+y), atlas row 0 is v = 0, so top-left is atlas[1,1], top-right
    atlas[1,0], bottom-left atlas[0,1], bottom-right atlas[0,0] -- exactly, the corner pixels lie in the clamped border half-texel."""
    import pointdreamer_amd.camera_utils as cu
    cams, _, _, _ = cu.create_cameras(6, 1.6, 8, distribution='self_defined', device=DEV)
    verts = T(np.array([[-.4, -.4, 0], [.4, -.4, 0], [.4, .4, 0], [-.4, .4, 0]], np.float32))
    faces = T(np.array([[0, 1, 2], [0, 2, 3]], np.int64))
    uvs = T(np.array([[0, 0], [1, 0], [1, 1], [0, 1]], np.float32))
    atlas = np.array([[[1, 0, 0], [0, 1, 0]], [[0, 0, 1], [1, 1, 0.5]]], np.float32)
    img, mask = cu.render_textured_mesh2(verts, faces, uvs, faces, T(atlas), cams[:1], return_mask=True)
    img, mask = img[0].permute(1, 2, 0).cpu().numpy(), mask[0].cpu().numpy()
    assert img.shape == (8, 8, 3) and 9 <= mask.sum() < 64
    rows, cols = np.nonzero(mask.any(1))[0], np.nonzero(mask.any(0))[0]
    t, b, l, r = rows[0], rows[-1], cols[0], cols[-1]
    assert mask[t, l] and mask[t, r] and mask[b, l] and mask[b, r]
    assert np.array_equal(img[t, l], atlas[1, 1]) and np.array_equal(img[t, r], atlas[1, 0])
    assert np.array_equal(img[b, l], atlas[0, 1]) and np.array_equal(img[b, r], atlas[0, 0])
    assert np.all(img[~mask] == 0)


def test_constant_atlas_background_and_alpha(scene):
    import pointdreamer_amd.camera_utils as cu
    s = scene[False]
    fx = s['fx']
    colour = np.array([0.3, 0.6, 0.9], np.float32)
    atlas = np.broadcast_to(colour, (32, 32, 3)).copy()
    images, rgba = cu.shade_views(s['fidx'], s['bary'], T(fx['uvs']), T(fx['faces']), atlas=T(atlas), want_rgba=True)
    img = images.permute(0, 2, 3, 1).cpu().numpy()
    mask = s['hard'].flip(1).cpu().numpy()
    assert mask.sum() > 1000
    assert np.all(img[mask] == colour) and np.all(img[~mask] == 0)
    rgba = rgba.cpu().numpy()
    assert np.array_equal(rgba[..., 3], np.where(mask, 255, 0).astype(np.uint8))          # alpha = rasterize()'s hard mask, flipped
    assert np.all(rgba[~mask] == 0)


# ----------------------------------------------------------------------------- parity against the float64 reference
def test_texture_parity_within_the_derived_bound(scene):
    """|kernel - float64 reference| <= 2*e_t*D + 4*2^-24 per pixel and channel, e_t = 10*A*M*2^-24 (derivation: render_common)."""
    import pointdreamer_amd.camera_utils as cu
    s = scene[False]
    fx = s['fx']
    images, _ = cu.shade_views(s['fidx'], s['bary'], T(fx['uvs']), T(fx['faces']), atlas=T(fx['atlas']))
    ref = rc.render_reference(s['fid_np'], s['bary_np'], fx['uvs'], fx['faces'], atlas=fx['atlas'])
    bound, _ = rc.texture_bound(ref, fx['A'])
    err = np.abs(images.cpu().numpy().astype(np.float64) - ref['images'])
    ratio = (err / bound[:, None]).max()
    note(f'texture parity (V=3 R=64 A=32, uv in [0.05,0.95]): max error {err.max():.3e}, max error/bound {ratio:.4f}')
    assert ref['mask'].sum() > 1000 and ref['images'].std() > 0.1
    assert np.all(err <= bound[:, None]), ratio
    assert np.all(images.permute(0, 2, 3, 1).cpu().numpy()[~ref['mask']] == 0)


def test_wrapped_uvs_within_the_bound_outside_the_seam_pixels(scene):
    import pointdreamer_amd.camera_utils as cu
    s = scene[True]
    fx = s['fx']
    images, _ = cu.shade_views(s['fidx'], s['bary'], T(fx['uvs']), T(fx['faces']), atlas=T(fx['atlas']))
    ref = rc.render_reference(s['fid_np'], s['bary_np'], fx['uvs'], fx['faces'], atlas=fx['atlas'])
    bound, e_t = rc.texture_bound(ref, fx['A'])
    ex = rc.wrap_excluded(ref, fx['A'], e_t)
    assert ex.sum() <= 0.005 * ref['mask'].sum()
    err = np.abs(images.cpu().numpy().astype(np.float64) - ref['images'])
    keep = ~ex
    ratio = (err / bound[:, None]).transpose(0, 2, 3, 1)[keep].max()
    note(f'wrap parity (uv in [-0.5,1.5]): {int(ex.sum())} of {int(ref["mask"].sum())} covered pixels left out, max error/bound {ratio:.4f}')
    assert ref['uv'].min() < -0.2 and ref['uv'].max() > 1.2
    assert np.all((err <= bound[:, None]).transpose(0, 2, 3, 1)[keep]), ratio


@pytest.mark.parametrize("double_side", [False, True])
def test_lighting_within_the_bound_before_and_after_gamma(scene, double_side):
    """Bound before the power: (albedo bound) * sum_l clip(n.l) + the rounding of the lighting sum (render_common.light_rounding).
    After the power only values >= 1e-3 are compared: x ** (1/2.2) has slope (1/2.2) * x ** (1/2.2 - 1), largest at the lower end
    of [ref - bound, ref + bound], plus 4 * 2^-24 for powf and the rounding of 1/gamma."""
    import pointdreamer_amd.camera_utils as cu
    s = scene[False]
    fx = s['fx']
    fn = cu.face_normals_unit(T(fx['verts']), T(fx['faces']))
    kw = dict(atlas=T(fx['atlas']), face_normals=fn, cam_params=s['cp'], light_dirs=T(fx['lights']), double_side=double_side)
    pre, _ = cu.shade_views(s['fidx'], s['bary'], T(fx['uvs']), T(fx['faces']), **kw)
    post, _ = cu.shade_views(s['fidx'], s['bary'], T(fx['uvs']), T(fx['faces']), gamma=2.2, **kw)
    ref = rc.render_reference(s['fid_np'], s['bary_np'], fx['uvs'], fx['faces'], atlas=fx['atlas'], normals=fn.cpu().numpy(),
                              cam_params=s['cp_np'], lights=fx['lights'], double_side=double_side, gamma=2.2)
    ex = ref['mask'] & (np.abs(ref['ndotcam']) < 1e-6)
    assert ex.sum() <= 0.01 * ref['mask'].sum()
    tb, _ = rc.texture_bound(ref, fx['A'])
    bound = (tb * ref['clipsum'] + rc.light_rounding(fx['lights'], 1.0))[:, None]
    keep = np.broadcast_to((~ex)[:, None], ref['images'].shape)
    err = np.abs(pre.cpu().numpy().astype(np.float64) - ref['pre_gamma'])
    r1 = (err / bound)[keep].max()
    assert np.all((err <= bound)[keep]), r1
    big = keep & (ref['pre_gamma'] >= 1e-3)
    lo = np.maximum(ref['pre_gamma'] - bound, 5e-4)
    bound2 = (1 / 2.2) * lo ** (1 / 2.2 - 1) * bound + 4 * rc.U
    err2 = np.abs(post.cpu().numpy().astype(np.float64) - ref['images'])
    r2 = (err2 / bound2)[big].max()
    note(f'lighting parity (3 lights, double_side={double_side}): {int(ex.sum())} pixels left out, max error/bound {r1:.4f} before gamma, '
         f'{r2:.4f} after gamma 2.2 ({int(big.sum())} values >= 1e-3)')
    assert big.sum() > 1000 and ref['pre_gamma'].max() > 0.3
    assert np.all((err2 <= bound2)[big]), r2
    assert np.all(post.permute(0, 2, 3, 1).cpu().numpy()[~ref['mask']] == 0)


# ----------------------------------------------------------------------------- other checks
def test_rgba_is_the_rounded_image_exactly(scene):
    import pointdreamer_amd.camera_utils as cu
    s = scene[False]
    fx = s['fx']
    fn = cu.face_normals_unit(T(fx['verts']), T(fx['faces']))
    for kw in (dict(), dict(face_normals=fn, cam_params=s['cp'], light_dirs=T(fx['lights'] * 3), gamma=2.2)):    # (x3: some values clip at 1)
        images, rgba = cu.shade_views(s['fidx'], s['bary'], T(fx['uvs']), T(fx['faces']), atlas=T(fx['atlas']), want_rgba=True, **kw)
        only, _ = cu.shade_views(s['fidx'], s['bary'], T(fx['uvs']), T(fx['faces']), atlas=T(fx['atlas']), **kw)
        assert torch.equal(images, only)
        img = images.permute(0, 2, 3, 1).cpu().numpy()
        want = np.clip(np.rint(img * np.float32(255)), 0, 255).astype(np.uint8)
        got = rgba.cpu().numpy()
        assert np.array_equal(got[..., :3], want)
        assert np.array_equal(got[..., 3] == 255, s['hard'].flip(1).cpu().numpy())
        _, alone = cu.shade_views(s['fidx'], s['bary'], T(fx['uvs']), T(fx['faces']), atlas=T(fx['atlas']), want_images=False, want_rgba=True, **kw)
        assert torch.equal(alone, rgba)


def test_per_vertex_colours_equal_interpolate_bit_for_bit(scene, tmp_path):
    import pointdreamer_amd.camera_utils as cu
    from pointdreamer_amd.extract_texture_map import interpolate
    from oracle import project as oproj
    s = scene[False]
    fx = s['fx']
    want = interpolate(T(fx['colors']), s['fidx'], s['bary'], T(fx['faces'])).flip(1).permute(0, 3, 1, 2)
    got = cu.render_per_vertex_color_mesh(T(fx['verts']), T(fx['faces']), T(fx['colors']), s['cams'], save_path=str(tmp_path / 'pv'))
    assert torch.equal(got, want)
    o = oproj.interpolate(fx['colors'], fx['faces'], s['fid_np'], s['bary_np'].astype(np.float32))
    assert np.array_equal(got.permute(0, 2, 3, 1).cpu().numpy(), o[:, ::-1])
    png = np.array(PIL.Image.open(tmp_path / 'pv' / 'albedo_002.png'))
    assert png.shape == (64, 64, 4)
    assert np.array_equal(png[..., :3], np.clip(np.rint(got[1].permute(1, 2, 0).cpu().numpy() * np.float32(255)), 0, 255).astype(np.uint8))
    assert np.array_equal(png[..., 3] == 255, s['hard'][1].flip(0).cpu().numpy())


def test_saved_mesh_renders_like_the_tensors_it_was_saved_from(scene, tmp_path):
    """save_textured_mesh -> render_textured_mesh (OBJ + MTL + PNG, the atlas flipped back) against render_textured_mesh2 on the
    tensors: within 1/255 (the atlas went through uint8) plus the bound of each of the two float32 evaluations.  Vertices and UVs
    are rounded to the six decimals the OBJ writer prints, so both renders see the same geometry."""
    import pointdreamer_amd.camera_utils as cu
    from pointdreamer_amd import demo
    s = scene[False]
    fx = s['fx']
    verts, uvs = T(np.round(fx['verts'].astype(np.float64), 6).astype(np.float32)), T(np.round(fx['uvs'].astype(np.float64), 6).astype(np.float32))
    faces, atlas = T(fx['faces']), T(fx['atlas'])
    for d in ('models', 'others'):
        os.makedirs(tmp_path / d)
    demo.save_textured_mesh(verts, uvs, faces, faces, atlas, torch.ones((1, 32, 32, 1), dtype=torch.bool, device=DEV), str(tmp_path))
    a = cu.render_textured_mesh2(verts, faces, uvs, faces, atlas, s['cams'])
    keep = verts.clone()
    b = cu.render_textured_mesh(str(tmp_path / 'models' / 'model_normalized.obj'), s['cams'], DEV, None, save=False, normalize_mesh=False)
    fidx, bary, _, _ = device_raster(s['cams'], verts, faces, fx['R'])
    ref = rc.render_reference(fidx.cpu().numpy(), bary.cpu().numpy().astype(np.float64), uvs.cpu().numpy(), fx['faces'], atlas=fx['atlas'])
    bound = 1.0 / 255.0 + 2.0 * rc.texture_bound(ref, fx['A'])[0][:, None]
    err = (a - b).abs().cpu().numpy().astype(np.float64)
    assert a.std() > 0.1 and np.all(err <= bound), (err / bound).max()
    c = cu.render_textured_mesh2(verts, faces, uvs, faces, atlas, s['cams'], normalize_mesh=True)      # must not touch the caller's tensor
    assert torch.equal(verts, keep) and tuple(c.shape) == (3, 3, 64, 64)


def _write_cloud(path, n=20000, seed=3):
    from pointdreamer_amd import synthetic, io_utils
    xyz, rgb = synthetic.sphere_points(n, seed=seed)
    io_utils.save_colored_pc_ply(xyz, rgb, path)


def test_demo_render_views_is_opt_in(tmp_path):
    from pointdreamer_amd import demo
    pc = str(tmp_path / 'ball.ply')
    _write_cloud(pc)
    base = ["--config", os.path.join(ROOT, "configs", "nearest.yaml"), "--pc_file", pc, "--set", "xatlas_texture_res=512",
            "point_validation_by_o3d=False"]
    out = demo.main(base + [f"output_path={tmp_path / 'a'}", "render_views=6", "render_res=64"])[0]
    files = sorted(os.listdir(os.path.join(out, 'rendered_imgs')))
    assert files == [f'albedo_{i:03d}.png' for i in range(1, 7)]
    for f in files:
        im = np.array(PIL.Image.open(os.path.join(out, 'rendered_imgs', f)))
        assert im.shape == (64, 64, 4) and set(np.unique(im[..., 3])) == {0, 255}
        assert (im[..., 3] == 255).mean() > 0.2 and im[..., :3][im[..., 3] == 255].std() > 5 and np.all(im[im[..., 3] == 0] == 0)
    out2 = demo.main(base + [f"output_path={tmp_path / 'b'}"])[0]
    assert not os.path.exists(os.path.join(out2, 'rendered_imgs'))
    tree = lambda o: sorted(os.path.relpath(os.path.join(d, f), o) for d, _, fs in os.walk(o) for f in fs)
    assert [f for f in tree(out) if not f.startswith('rendered_imgs')] == tree(out2)


def test_render_meshes_cli_writes_twenty_views_and_skips_finished_shapes(scene, tmp_path):
    """data/render_meshes.py layout: <root>/meshes/<cls>/<shape>/models/model_normalized.obj -> <root>/rendered_imgs/<cls>/<shape>/
    albedo_001.png ... albedo_020.png (RGBA, 1024^2); a second run finds the 20 files and renders nothing; `kaolin_per_vertex` draws
    an OBJ with `v x y z r g b` records."""
    from pointdreamer_amd import demo, render_meshes
    fx = scene[False]['fx']
    shape = tmp_path / 'tex' / 'meshes' / 'cls' / 'ball'
    for d in ('models', 'others'):
        os.makedirs(shape / d)
    demo.save_textured_mesh(T(fx['verts']), T(fx['uvs']), T(fx['faces']), T(fx['faces']), T(fx['atlas']),
                            torch.ones((1, 32, 32, 1), dtype=torch.bool, device=DEV), str(shape))
    assert render_meshes.main(['--rootpath', str(tmp_path / 'tex'), '--by', 'kaolin']) == 1
    out = tmp_path / 'tex' / 'rendered_imgs' / 'cls' / 'ball'
    assert sorted(os.listdir(out)) == [f'albedo_{i:03d}.png' for i in range(1, 21)]
    im = np.array(PIL.Image.open(out / 'albedo_020.png'))
    assert im.shape == (1024, 1024, 4) and set(np.unique(im[..., 3])) == {0, 255} and 0.2 < (im[..., 3] == 255).mean() < 0.9
    assert im[..., :3][im[..., 3] == 255].std() > 20 and np.all(im[im[..., 3] == 0] == 0)
    assert render_meshes.main(['--rootpath', str(tmp_path / 'tex'), '--by', 'kaolin']) == 0
    pv = tmp_path / 'pv' / 'meshes' / 'cls' / 'ball' / 'models'
    os.makedirs(pv)
    with open(pv / 'model_normalized.obj', 'w') as f:
        for p, c in zip(fx['verts'], fx['colors']):
            f.write('v %.9g %.9g %.9g %.9g %.9g %.9g\n' % (*p, *c))
        for a, b, c in fx['faces'] + 1:
            f.write(f'f {a} {b} {c}\n')
    assert render_meshes.main(['--rootpath', str(tmp_path / 'pv'), '--by', 'kaolin_per_vertex']) == 1
    im = np.array(PIL.Image.open(tmp_path / 'pv' / 'rendered_imgs' / 'cls' / 'ball' / 'albedo_001.png'))
    assert im.shape == (1024, 1024, 4) and (im[..., 3] == 255).mean() > 0.2 and im[..., :3][im[..., 3] == 255].std() > 20


def test_kd_only_material_renders_as_a_one_texel_atlas(scene, tmp_path):
    """An MTL without map_Kd: the Kd colour is a 1 x 1 atlas, every covered pixel shows exactly it; geo_only replaces it by `color`."""
    import pointdreamer_amd.camera_utils as cu
    s = scene[False]
    fx = s['fx']
    with open(tmp_path / 'ball.obj', 'w') as f:
        f.write('mtllib ball.mtl\n')
        for p in fx['verts']:
            f.write('v %.9g %.9g %.9g\n' % tuple(p))
        for t in fx['uvs']:
            f.write('vt %.9g %.9g\n' % tuple(t))
        f.write('usemtl m\n')
        for a, b, c in fx['faces'] + 1:
            f.write(f'f {a}/{a} {b}/{b} {c}/{c}\n')
    (tmp_path / 'ball.mtl').write_text('newmtl m\nKd 0.25 0.5 0.75\n')
    mask = s['hard'].flip(1).cpu().numpy()
    img = cu.render_textured_mesh(str(tmp_path / 'ball.obj'), s['cams'], DEV, None, save=False, normalize_mesh=False)
    img = img.permute(0, 2, 3, 1).cpu().numpy()
    assert np.all(img[mask] == np.array([0.25, 0.5, 0.75], np.float32)) and np.all(img[~mask] == 0)
    geo = cu.render_textured_mesh(str(tmp_path / 'ball.obj'), s['cams'], DEV, str(tmp_path / 'geo'), normalize_mesh=False, geo_only=True)
    assert np.all(geo.permute(0, 2, 3, 1).cpu().numpy()[mask] == 0.5)
    png = np.array(PIL.Image.open(tmp_path / 'geo' / 'albedo_003.png'))
    assert np.array_equal(png[..., 3] == 255, mask[2]) and np.all(png[mask[2]][:, :3] == 128)      # rint(0.5 * 255) = 128 (half to even)
