"""Render / image-metric feature, the part that needs no GPU: the ABI surface (header and ctypes table), argument refusal at the C ABI,
closed forms of the numpy metric references (tests/render_common.py), the float64 render reference against the oracle's float32
interpolate, and the exclusion shares of the GPU fixtures (computed with the oracle's CPU rasteriser) against their caps."""
import ctypes as C
import math
import os

import numpy as np
import pytest

from conftest import ROOT
import render_common as rc

NEW = ('pdhip_shade_views', 'pdhip_image_metrics_workspace_bytes', 'pdhip_image_metrics')


def test_header_and_ctypes_table_declare_the_new_entry_points():
    from pointdreamer_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'pdhip.h')).read()
    for name in NEW:
        assert f'{name}(' in header, name
        assert name in _lib._SIGS, name
    assert len(_lib._SIGS['pdhip_shade_views'][1]) == 20 and len(_lib._SIGS['pdhip_image_metrics'][1]) == 11


@pytest.fixture(scope="module")
def L():
    from pointdreamer_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libpdhip.so not built")
    return _lib.lib()


def test_entry_points_refuse_bad_arguments_without_a_device(L):
    fake = C.c_void_p(4096)
    assert L.pdhip_image_metrics_workspace_bytes(3, 64, 64) >= 3 * 4 * 2 * 16 and L.pdhip_image_metrics_workspace_bytes(0, 64, 64) == 0
    assert L.pdhip_image_metrics(fake, fake, 1, 6, 64, 3, 0, fake, fake, fake, None) == -1            # smaller than the 7 x 7 window
    assert b'smaller than the 7 x 7' in L.pdhip_last_error()
    assert L.pdhip_image_metrics(fake, fake, 1, 64, 10, 3, 1, fake, fake, fake, None) == -1           # smaller than the 11 x 11 window
    assert b'smaller than the 11 x 11' in L.pdhip_last_error()
    assert L.pdhip_image_metrics(fake, fake, 1, 64, 64, 5, 0, fake, fake, fake, None) == -1 and b'channels' in L.pdhip_last_error()
    assert L.pdhip_image_metrics(fake, fake, 1, 64, 64, 3, 0, None, None, fake, None) == -1
    assert L.pdhip_image_metrics(None, fake, 1, 64, 64, 3, 0, fake, fake, fake, None) == -1
    sv = lambda **k: L.pdhip_shade_views(*[k.get(n, d) for n, d in (
        ('fid', fake), ('bary', fake), ('V', 1), ('R', 8), ('attr', fake), ('Na', 4), ('C', 2), ('tri', fake), ('F', 2), ('atlas', fake), ('A', 2),
        ('fn', None), ('cam', None), ('lights', None), ('L', 0), ('ds', 0), ('gamma', 0.0), ('images', fake), ('rgba', None), ('stream', None))])
    assert sv(C=4) == -1 and b'C = 4' in L.pdhip_last_error()
    assert sv(atlas=None) == -1 and b'atlas' in L.pdhip_last_error()
    assert sv(C=3) == -1 and b'no atlas' in L.pdhip_last_error()
    assert sv(images=None) == -1 and b'both NULL' in L.pdhip_last_error()
    assert sv(lights=fake, L=3) == -1 and b'lighting needs' in L.pdhip_last_error()                   # lights without normals / cameras
    assert sv(gamma=2.2) == -1 and b'gamma' in L.pdhip_last_error()                                    # gamma without lights
    assert sv(fid=None) == -1 and sv(R=0) == -1 and sv(L=17, lights=fake, fn=fake, cam=fake) == -1


# ----------------------------------------------------------------------------- metric references: closed forms
@pytest.mark.parametrize("use_sk", [True, False])
@pytest.mark.parametrize("a,b", [(10, 200), (0, 255), (37, 38), (128, 128)])
def test_constant_images_have_the_closed_form_ssim_and_psnr(a, b, use_sk):
    x = np.full((13, 17, 3), a, np.uint8)
    y = np.full((13, 17, 3), b, np.uint8)
    want = (2.0 * a * b + rc.C1) / (a * a + b * b + rc.C1)
    assert abs(rc.ssim_ref(x, y, use_sk) - want) <= 1e-12
    p, sse = rc.psnr_ref(x, y)
    if a == b:
        assert p == float('inf') and sse == 0 and abs(rc.ssim_ref(x, y, use_sk) - 1.0) <= 1e-12
    else:
        assert abs(p - 20.0 * math.log10(255.0 / abs(a - b))) <= 1e-12 and sse == (a - b) ** 2 * x.size


@pytest.mark.parametrize("use_sk", [True, False])
def test_identical_random_images_give_ssim_one_and_psnr_inf(use_sk):
    x = np.random.default_rng(1).integers(0, 256, size=(20, 23, 3), dtype=np.uint8)
    assert abs(rc.ssim_ref(x, x, use_sk) - 1.0) <= 1e-12
    assert rc.psnr_ref(x, x) == (float('inf'), 0)
    y = np.random.default_rng(2).integers(0, 256, size=(20, 23, 3), dtype=np.uint8)
    assert rc.ssim_ref(x, y, use_sk) < 0.2                          # unrelated noise
    with pytest.raises(ValueError):
        rc.ssim_ref(x[:6], y[:6], True)


def test_gaussian_taps_are_normalised_and_symmetric():
    g = rc.gaussian_taps()
    assert len(g) == 11 and abs(g.sum() - 1.0) <= 1e-15 and np.allclose(g, g[::-1], atol=0) and g.argmax() == 5
    assert abs(g[4] / g[5] - math.exp(-1.0 / 4.5)) <= 1e-15


# ----------------------------------------------------------------------------- render reference and fixtures
@pytest.fixture(scope="module")
def raster():
    out = {}
    for wrap in (False, True):
        fx = rc.sphere_fixture(wrap)
        fid, bary, cams = rc.cpu_raster(fx)
        out[wrap] = (fx, fid, bary, cams)
    return out


def test_float64_interpolation_agrees_with_the_oracle_float32_one(raster):
    from oracle import project as oproj
    fx, fid, bary, _ = raster[False]
    a64 = rc.interpolate64(fx['uvs'], fx['faces'], fid, bary)
    a32 = oproj.interpolate(fx['uvs'], fx['faces'], fid, bary)
    assert (fid >= 0).mean() > 0.1
    assert np.abs(a64 - a32).max() <= 8 * rc.U                      # 7 float32 roundings of values <= 1
    assert np.all(a64[fid < 0] == 0)


def test_reference_orientation_on_a_two_by_two_atlas():
    """uv = (0.25, 0.25) is the centre of texel (row 0, col 0): row 0 of the atlas is v = 0."""
    atlas = np.arange(12, dtype=np.float64).reshape(2, 2, 3) / 12.0
    fid = np.zeros((1, 1, 1), np.int64)
    bary = np.array([[[[1.0, 0.0]]]])
    for uv, texel in (((0.25, 0.25), atlas[0, 0]), ((0.75, 0.25), atlas[0, 1]), ((0.25, 0.75), atlas[1, 0]), ((0.75, 0.75), atlas[1, 1])):
        attr = np.array([uv, uv, uv])
        ref = rc.render_reference(fid, bary, attr, np.array([[0, 1, 2]]), atlas=atlas)
        assert np.allclose(ref['images'][0, :, 0, 0], texel, atol=1e-15), uv


def test_wrap_fixture_exclusions_stay_below_their_cap(raster):
    fx, fid, bary, _ = raster[True]
    assert fx['uvs'].min() < -0.3 and fx['uvs'].max() > 1.3
    ref = rc.render_reference(fid, bary, fx['uvs'], fx['faces'], atlas=fx['atlas'])
    _, e_t = rc.texture_bound(ref, fx['A'])
    ex = rc.wrap_excluded(ref, fx['A'], e_t)
    assert ref['mask'].sum() > 1000 and ex.sum() <= 0.005 * ref['mask'].sum(), (ex.sum(), ref['mask'].sum())
    fx0, fid0, bary0, _ = raster[False]
    ref0 = rc.render_reference(fid0, bary0, fx0['uvs'], fx0['faces'], atlas=fx0['atlas'])
    assert ref0['uv'][ref0['mask']].min() >= 0.05 - 1e-6 and ref0['uv'][ref0['mask']].max() <= 0.95 + 1e-6
    assert not rc.wrap_excluded(ref0, fx0['A'], rc.texture_bound(ref0, fx0['A'])[1]).any()


def test_lighting_fixture_exclusions_stay_below_their_cap(raster):
    fx, fid, bary, cams = raster[False]
    n = rc.face_normals64(fx['verts'], fx['faces'])
    ref = rc.render_reference(fid, bary, fx['uvs'], fx['faces'], atlas=fx['atlas'], normals=n, cam_params=cams, lights=fx['lights'])
    ex = ref['mask'] & (np.abs(ref['ndotcam']) < 1e-6)
    assert ex.sum() <= 0.01 * ref['mask'].sum(), (ex.sum(), ref['mask'].sum())
    assert ref['images'].max() <= 1.0 and ref['images'][:, :, ~ref['mask'][0]].shape[0] == 3
    assert np.all(ref['images'].transpose(0, 2, 3, 1)[~ref['mask']] == 0)


def test_demo_config_knows_the_render_keys(tmp_path):
    from pointdreamer_amd import demo
    cfg = demo.load_config(os.path.join(ROOT, 'configs', 'nearest.yaml'), dict(render_views=6, render_res=64))
    assert cfg.render_views == 6 and cfg.render_res == 64
    assert 'render_views' not in demo.load_config(os.path.join(ROOT, 'configs', 'nearest.yaml'))
    assert 'render_after_inference' in demo.UPSTREAM_KEYS                  # still accepted and ignored
    with pytest.raises(ValueError):
        demo.load_config(os.path.join(ROOT, 'configs', 'nearest.yaml'), dict(render_views=8))
    with pytest.raises(ValueError):
        demo.load_config(os.path.join(ROOT, 'configs', 'nearest.yaml'), dict(render_views=6, render_res=0))


def test_metric_and_loader_argument_checks_need_no_device(tmp_path):
    import torch
    from pointdreamer_amd import metric_utils, camera_utils
    a = torch.zeros((1, 6, 20, 3), dtype=torch.uint8)
    with pytest.raises(ValueError):
        metric_utils.calculate_ssim_batch(a, a)                            # smaller than the 7 x 7 window
    with pytest.raises(ValueError):
        metric_utils.calculate_ssim_batch(a[:, :, :10].repeat(1, 2, 1, 1), a[:, :, :10].repeat(1, 2, 1, 1), use_sk=False)   # 12 x 10 < 11 x 11
    with pytest.raises(ValueError):
        metric_utils.calculate_psnr_batch(a, a[:, :5])
    obj = tmp_path / 'two.obj'
    obj.write_text('mtllib two.mtl\nv 0 0 0\nv 1 0 0\nv 0 1 0\nvt 0 0\nusemtl a\nf 1/1 2/1 3/1\nusemtl b\nf 1/1 3/1 2/1\n')
    (tmp_path / 'two.mtl').write_text('newmtl a\nKd 1 0 0\nnewmtl b\nKd 0 1 0\n')
    with pytest.raises(NotImplementedError, match='single material'):
        camera_utils.load_textured_obj(str(obj), 'cpu')
    one = tmp_path / 'one.obj'
    one.write_text('mtllib one.mtl\nv 0 0 0\nv 1 0 0\nv 0 1 0\nvt 0 0\nusemtl a\nf 1/1 2/1 3/1\n')
    (tmp_path / 'one.mtl').write_text('newmtl a\nKd 0.25 0.5 0.75\n')
    v, f, vt, ft, atlas = camera_utils.load_textured_obj(str(one), 'cpu')
    assert tuple(atlas.shape) == (1, 1, 3) and atlas.flatten().tolist() == [0.25, 0.5, 0.75] and tuple(f.shape) == (1, 3)
