"""Multi-material rendering, the part that needs no GPU: the exclusion share of the GPU fixture against its cap (oracle CPU raster),
the derived bound checked against a float32 emulation of the kernel's arithmetic before a GPU sees it, argument refusal of
pdhip_shade_views_materials at the C ABI, and the host-side check of a packed material set."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import render_common as rc
import render_materials_common as rmc


@pytest.fixture(scope="module")
def cpu_scene():
    """The fixture, the oracle's CPU raster of it and the float64 reference, computed once; read-only."""
    fx = rmc.fixture()
    fid, bary, cams = rc.cpu_raster(fx)
    ref = rmc.reference(fid, bary, fx['uvs'], fx['face_uvs_idx'], fx['face_material'], fx['materials'])
    return fx, fid, bary, ref


def test_fixture_exclusions_stay_below_the_cap_and_every_material_shows(cpu_scene):
    fx, fid, bary, ref = cpu_scene
    covered = int(ref['mask'].sum())
    assert covered > 1000 and ref['excluded'].sum() <= rmc.CAP * covered, (int(ref['excluded'].sum()), covered)
    for m in range(3):
        assert (ref['material'] == m).sum() > 200, m
    assert np.all(ref['material'][~ref['mask']] == -1)
    no_vt = np.all(fx['face_uvs_idx'] < 0, axis=1)
    assert no_vt.sum() == 30 and np.isin(fid[fid >= 0], np.nonzero(no_vt)[0]).any()          # at least one `-1` face is visible
    # the identical-corner pixels are exactly the pixels of the `-1` faces, and their UV is 0 in both precisions
    assert ref['same3'].sum() > 0 and np.all(ref['uv'][ref['same3']] == 0)
    assert ref['uv'].min() < -0.2 and ref['uv'].max() > 1.2 and ref['M'] >= 1.0
    assert not (ref['excluded'] & ref['same3']).any()
    # a Kd pixel carries bound 0, a textured one at least 6u
    kd = ref['material'] == 1
    assert np.all(ref['bound'][kd] == 0) and np.all(ref['bound'][ref['mask'] & ~kd] >= 6 * rmc.U)


def test_float32_emulation_of_the_kernel_stays_inside_the_derived_bound(cpu_scene):
    fx, fid, bary, ref = cpu_scene
    emu = rmc.emulate32(fid, bary.astype(np.float32), fx['uvs'], fx['face_uvs_idx'], fx['face_material'], fx['materials'])
    err = np.abs(emu.astype(np.float64) - ref['albedo']).max(-1)
    keep = ref['mask'] & ~ref['excluded']
    textured = keep & (ref['material'] != 1)
    ratio = (err[textured] / ref['bound'][textured]).max()
    print(f'float32 emulation against the float64 reference: max error {err[keep].max():.3e}, max error/bound {ratio:.4f}')
    assert np.all(err[keep] <= ref['bound'][keep]), ratio
    assert ratio > 1e-3                                                                    # the bound is not vacuous
    kd = ref['material'] == 1
    assert np.all(emu[kd] == np.asarray(fx['materials'][1]['Kd'], np.float32)) and np.all(emu[~ref['mask']] == 0)
    # the float64 reference itself: a constant image looks up its constant, a -1 face looks up the texel at uv = 0 (bottom-left)
    img = fx['materials'][0]['map_Kd']
    sel = ref['same3'] & (ref['material'] == 0)
    if sel.any():
        assert np.allclose(ref['albedo'][sel], img[-1, 0] / 255.0, atol=1e-15)


@pytest.fixture(scope="module")
def L():
    from pointdreamer_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libpdhip.so not built")
    return _lib.lib()


def test_header_and_ctypes_table_declare_the_entry():
    from conftest import ROOT
    from pointdreamer_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'pdhip.h')).read()
    assert 'pdhip_shade_views_materials(' in header
    assert len(_lib._SIGS['pdhip_shade_views_materials'][1]) == 25


def test_entry_refuses_bad_arguments_before_any_launch(L):
    fake = C.c_void_p(4096)
    names = (('fid', fake), ('bary', fake), ('V', 1), ('R', 8), ('uvs', fake), ('T', 4), ('ft', fake), ('fm', fake), ('F', 2),
             ('texels', fake), ('bytes', 24), ('off', fake), ('wh', fake), ('kd', fake), ('M', 2), ('fn', None), ('cam', None),
             ('lights', None), ('L', 0), ('ds', 0), ('gamma', 0.0), ('images', fake), ('rgba', None), ('midx', None), ('stream', None))
    sv = lambda **k: L.pdhip_shade_views_materials(*[k.get(n, d) for n, d in names])
    E_ARG = -1
    assert sv(M=0) == E_ARG and b'M = 0' in L.pdhip_last_error()
    assert sv(M=256) == E_ARG and b'M = 256' in L.pdhip_last_error()
    assert sv(ft=None) == E_ARG and b'go together' in L.pdhip_last_error()                 # uvs without face_uvs_idx
    assert sv(uvs=None) == E_ARG and b'go together' in L.pdhip_last_error()
    assert sv(images=None) == E_ARG and b'both NULL' in L.pdhip_last_error()
    assert sv(L=17, lights=fake, fn=fake, cam=fake) == E_ARG and b'L = 17' in L.pdhip_last_error()
    assert sv(gamma=2.2) == E_ARG and b'gamma' in L.pdhip_last_error()                     # gamma without lights
    assert sv(lights=fake, L=3) == E_ARG and b'lighting needs' in L.pdhip_last_error()
    assert sv(T=0) == E_ARG and b'T = 0' in L.pdhip_last_error()
    assert sv(texels=None) == E_ARG and b'texel_bytes' in L.pdhip_last_error()
    assert sv(fid=None) == E_ARG and sv(R=0) == E_ARG and sv(F=0) == E_ARG and sv(V=0) == E_ARG and sv(off=None) == E_ARG
    for msg in (b'pdhip_shade_views_materials',):
        assert msg in L.pdhip_last_error()


def _packed():
    from pointdreamer_amd.sample_colored_pc_from_mesh import pack_materials
    return pack_materials(rmc.fixture()['materials'], 'cpu')


def test_packed_material_check_accepts_the_packer_and_names_what_is_wrong():
    from pointdreamer_amd import camera_utils as cu
    tex, off, wh, kd = _packed()
    assert cu.check_packed_materials((tex, off, wh, kd)) == 3
    assert int(tex.numel()) == 3 * (32 * 16 + 8 * 8) and off.tolist() == [0, 1536, 1536] and wh.tolist() == [[32, 16], [0, 0], [8, 8]]
    with pytest.raises(ValueError, match='does not lie inside'):
        cu.check_packed_materials((tex[:-1], off, wh, kd))                                  # the last image ends one byte past the end
    bad = off.clone()
    bad[2] = 1537
    with pytest.raises(ValueError, match='material 2'):
        cu.check_packed_materials((tex, bad, wh, kd))
    with pytest.raises(ValueError, match='int64 / int32 / float32'):
        cu.check_packed_materials((tex, off.int(), wh, kd))
    with pytest.raises(ValueError, match='uint8'):
        cu.check_packed_materials((tex.float(), off, wh, kd))
    with pytest.raises(ValueError, match=r'mat_wh \[M,2\]'):
        cu.check_packed_materials((tex, off, wh[:2], kd))
    with pytest.raises(ValueError, match='1 .. 255'):
        cu.check_packed_materials((tex, off.repeat(100), wh.repeat(100, 1), kd.repeat(100, 1)))
    with pytest.raises(ValueError, match='four tensors'):
        cu.check_packed_materials((tex, off, wh))


def test_wrapper_refuses_a_malformed_packed_tuple_before_the_library_is_called():
    """An image past the end of `texels`: ValueError from shade_views_materials itself, raised by the host check that runs first --
    the tensors here live on the CPU, which the library call would refuse with PdhipError."""
    from pointdreamer_amd import camera_utils as cu
    tex, off, wh, kd = _packed()
    fid = torch.zeros((1, 4, 4), dtype=torch.int64)
    bary = torch.zeros((1, 4, 4, 2))
    with pytest.raises(ValueError, match='does not lie inside'):
        cu.shade_views_materials(fid, bary, None, None, torch.zeros(2, dtype=torch.int32), (tex[:100], off, wh, kd))
