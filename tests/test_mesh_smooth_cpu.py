"""Mesh smoothing without a GPU: the C ABI (declared, exported, bound; no workspace query), every refusal that comes before a device call, the
refusal of CPU tensors and of bad keywords and demo keys, zero scratch on the new kernels, and the definition itself on the numpy oracle of
tests/mesh_smooth_common.py: Taubin's pair removes noise and keeps the volume, the plain Laplacian shrinks."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT
import mesh_smooth_common as msc
from mesh_components_common import bow_tie

LIB = os.path.join(ROOT, 'pointdreamer_amd', 'libpdhip.so')
SYMBOLS = ('pdhip_mesh_boundary_vertices', 'pdhip_smooth_mesh')
NEAREST = os.path.join(ROOT, 'configs', 'nearest.yaml')
VMAX, FMAX = 1 << 26, 1 << 23


def _lib():
    import __graft_entry__ as ge
    ge.build()
    from pointdreamer_amd import _lib
    return _lib.lib()


# ---- the C ABI
def test_header_declares_and_library_exports_the_symbols():
    L = _lib()
    from pointdreamer_amd import _lib as lib_mod
    txt = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'pdhip.h')).read(), flags=re.S)
    for s in SYMBOLS:
        assert re.search(r'\b%s\s*\(' % s, txt), f"{s} is not declared in include/pdhip.h"
        assert hasattr(L, s) and s in lib_mod._SIGS, s
    assert len(lib_mod._SIGS['pdhip_mesh_boundary_vertices'][1]) == 9 and len(lib_mod._SIGS['pdhip_smooth_mesh'][1]) == 13
    assert lib_mod._SIGS['pdhip_smooth_mesh'][1][6:8] == [C.c_double, C.c_double]
    # every buffer is an argument: no size query came with the entries
    assert not any(('smooth' in s or 'boundary' in s) and s.endswith(('_ws_bytes', '_workspace_bytes', '_ws_ints')) for s in lib_mod._SIGS)


def _smooth_call(L):
    one, two = C.c_void_p(256), C.c_void_p(512)                    # (never dereferenced: the arguments are refused first)
    ok = dict(vertices=one, Vn=9, rowptr=one, colidx=one, held=one, steps=10, lam=0.5, mu=-0.53, state_a=one, state_b=two, out_vertices=one,
              counts=one, stream=None)
    order = list(ok)
    return lambda **kw: L.pdhip_smooth_mesh(*[dict(ok, **kw)[k] for k in order])


def test_smooth_refuses_null_pointers_and_sizes_by_name_before_any_launch():
    L = _lib()
    call = _smooth_call(L)
    for name in ('vertices', 'rowptr', 'colidx', 'state_a', 'state_b', 'out_vertices', 'counts'):
        assert call(**{name: None}) == -1
        msg = L.pdhip_last_error()
        assert b'pdhip_smooth_mesh' in msg and b'null pointer' in msg and ('(%s)' % name).encode() in msg, msg
    for kw, word in ((dict(Vn=0), b'Vn=0'), (dict(Vn=-4), b'Vn=-4'), (dict(Vn=VMAX + 1), b'Vn=67108865'), (dict(steps=0), b'steps=0'),
                     (dict(steps=-1), b'steps=-1'), (dict(steps=10001), b'steps=10001'), (dict(state_a=C.c_void_p(264)), b'32 bytes'),
                     (dict(state_b=C.c_void_p(520)), b'32 bytes'), (dict(state_b=C.c_void_p(256)), b'one buffer')):
        assert call(**kw) == -1
        assert b'pdhip_smooth_mesh' in L.pdhip_last_error() and word in L.pdhip_last_error(), (kw, L.pdhip_last_error())


BAD_FACTORS = (
    (dict(lam=0.0), 'lambda'), (dict(lam=-0.5), 'lambda'), (dict(lam=1.0000001), 'lambda'), (dict(lam=float('nan')), 'lambda'),
    (dict(lam=float('inf')), 'lambda'),
    (dict(mu=0.1), 'mu='), (dict(mu=float('nan')), 'mu='), (dict(mu=float('-inf')), 'mu='), (dict(mu=float('inf')), 'mu='),
    (dict(mu=-0.5), 'Taubin pair'), (dict(mu=-0.3), 'Taubin pair'), (dict(lam=1.0, mu=-1.0), 'Taubin pair'),      # -lambda <= mu < 0
    (dict(lam=1.0, mu=-1.5), 'highest frequency'), (dict(lam=0.9, mu=-1.0), 'highest frequency'),                 # |(1 - 2 l)(1 - 2 mu)| = 4, 2.4
    (dict(lam=0.1, mu=-0.2), 'highest frequency'),                                                                # 0.8 * 1.4 = 1.12
)


def test_smooth_refuses_the_factors_of_the_contract():
    L = _lib()
    call = _smooth_call(L)
    for kw, word in BAD_FACTORS:
        assert call(**kw) == -1, kw
        msg = L.pdhip_last_error().decode()
        assert 'pdhip_smooth_mesh' in msg and word in msg, (kw, msg)


def test_python_refuses_the_same_factors_and_accepts_the_usual_pairs():
    from pointdreamer_amd import mesh_smooth as M
    for kw, _ in BAD_FACTORS:
        with pytest.raises(ValueError):
            M.check_params(**dict(dict(steps=10, lam=0.5, mu=-0.53), **kw))
    for bad in (0, -1, 10001, 2.0, True, '3', None):
        with pytest.raises(ValueError, match='steps'):
            M.check_params(bad, 0.5, -0.53)
    for bad in ('0.5', None, True):
        with pytest.raises(ValueError):
            M.check_params(3, bad, -0.53)
    assert M.check_params(10, *msc.MESHLAB) == (10, 0.5, -0.53) and M.check_params(1, *msc.TAUBIN) == (1, 0.33, -0.34)
    assert M.check_params(10000, 1, 0) == (10000, 1.0, 0.0) and M.check_params(1, 0.5, -0.5000001)[2] == -0.5000001
    assert (M.DEFAULT_STEPS, M.DEFAULT_LAMBDA, M.DEFAULT_MU) == (10,) + msc.MESHLAB


def test_the_usual_pairs_pass_the_entrys_host_checks():
    """Accepted factors get past every host-side refusal: the next one, a misaligned state buffer, is checked after them."""
    L = _lib()
    call = _smooth_call(L)
    for lam, mu in (msc.MESHLAB, msc.TAUBIN, (0.5, 0.0), (1.0, 0.0), (0.5, -0.5000001), (0.25, -0.5)):     # (the last: the product is exactly 1)
        assert call(lam=lam, mu=mu, state_a=C.c_void_p(264)) == -1
        assert b'32 bytes' in L.pdhip_last_error(), (lam, mu, L.pdhip_last_error())


def test_boundary_refuses_null_pointers_and_sizes_by_name_before_any_launch():
    L = _lib()
    one = C.c_void_p(256)
    ok = dict(faces=one, F=8, Vn=9, rowptr=one, colidx=one, pair_faces=one, boundary=one, counts=one, stream=None)
    order = list(ok)
    call = lambda **kw: L.pdhip_mesh_boundary_vertices(*[dict(ok, **kw)[k] for k in order])
    for name in ('faces', 'rowptr', 'colidx', 'pair_faces', 'boundary', 'counts'):
        assert call(**{name: None}) == -1
        msg = L.pdhip_last_error()
        assert b'pdhip_mesh_boundary_vertices' in msg and b'null pointer' in msg and ('(%s)' % name).encode() in msg, msg
    for kw, word in ((dict(Vn=0), b'Vn=0'), (dict(F=0), b'F=0'), (dict(F=-1), b'F=-1'), (dict(F=FMAX + 1), b'F=8388609'),
                     (dict(Vn=VMAX + 1), b'Vn=67108865')):
        assert call(**kw) == -1
        assert b'pdhip_mesh_boundary_vertices' in L.pdhip_last_error() and word in L.pdhip_last_error(), (kw, L.pdhip_last_error())


def test_no_scratch_and_no_lds_on_the_new_kernels():
    if not os.path.exists(LIB):
        _lib()
    pytest.importorskip('msgpack')                                 # (as tests/test_code_objects_cpu.py: the metadata note is msgpack)
    from tools import code_object_notes
    mine = [k for k in code_object_notes.kernels(LIB) if 'k_msm_' in k['name']]
    names = ' '.join(k['name'] for k in mine)
    for must in ('k_msm_check', 'k_msm_pass', 'k_msm_pair_zero', 'k_msm_pair_count', 'k_msm_boundary'):
        assert must in names, must
    assert sum('k_msm_pass' in k['name'] for k in mine) == 4       # f32 or f64 in, f32 or f64 out
    for k in mine:
        print(k['name'], 'vgprs', k['vgpr_count'], 'lds', k['group_segment_fixed_size'], 'scratch', k['private_segment_fixed_size'])
        assert k['arch'] == 'gfx950'
        assert k['vgpr_spill_count'] == 0 and k['private_segment_fixed_size'] == 0 and k['group_segment_fixed_size'] == 0, k


# ---- python
def test_cpu_tensors_and_bad_keywords_are_refused():
    from pointdreamer_amd import mesh_smooth as M
    from pointdreamer_amd._lib import PdhipError
    v, f = torch.from_numpy(msc.TET_V), torch.from_numpy(msc.TET)
    with pytest.raises(PdhipError, match='no CPU path'):
        M.taubin_smooth(v, f)
    with pytest.raises(PdhipError, match='no CPU path'):
        M.laplacian_smooth(v, f)
    with pytest.raises(PdhipError, match='no CPU path'):
        M.boundary_vertices(f, 4)
    with pytest.raises(PdhipError, match='no CPU path'):
        M.taubin_smooth(v.numpy(), f.numpy())
    with pytest.raises(ValueError, match='boundary'):
        M.taubin_smooth(v, f, boundary='open')
    with pytest.raises(ValueError, match='Taubin pair'):
        M.taubin_smooth(v, f, lam=0.5, mu=-0.5)
    p = inspect.signature(M.taubin_smooth).parameters
    assert list(p) == ['vertices', 'faces', 'steps', 'lam', 'mu', 'boundary', 'fixed', 'return_counts']
    assert [p[k].default for k in ('steps', 'lam', 'mu', 'boundary', 'fixed')] == [10, 0.5, -0.53, 'fixed', None]
    p = inspect.signature(M.laplacian_smooth).parameters
    assert 'mu' not in p and p['steps'].default == 1 and p['lam'].default == 0.5
    assert list(inspect.signature(M.boundary_vertices).parameters) == ['faces', 'num_vertices', 'return_counts']
    src = open(os.path.join(ROOT, 'pointdreamer_amd', 'mesh_smooth.py')).read()
    assert 'oracle' not in src and 'mesh_smooth_common' not in src and 'scipy' not in src


def test_recon_one_shape_SPR_takes_smooth_and_refuses_bad_values():
    from pointdreamer_amd import spr
    p = inspect.signature(spr.recon_one_shape_SPR).parameters
    assert p['smooth'].kind == inspect.Parameter.KEYWORD_ONLY and p['smooth'].default is None
    assert list(p)[:6] == ['coords', 'colors', 'gt_normals', 'save_path', 'depth', 'simplify_face_num']
    z = np.zeros((10, 3), np.float32)
    for bad in ('x', True, 0, -3, 2.5, {}, dict(lam=0.5), dict(steps=3, lamda=0.5), dict(steps=3, lam=0.5, mu=-0.5), dict(steps=3, mu=0.2), [10]):
        with pytest.raises(ValueError, match='smooth'):
            spr.recon_one_shape_SPR(z, z, smooth=bad)


def test_demo_accepts_the_smoothing_keys_and_validates_them():
    from pointdreamer_amd import demo
    assert demo.SMOOTH_KEYS == ('spr_smooth', 'spr_smooth_lambda', 'spr_smooth_mu')
    assert demo.COMPONENT_KEYS == ('spr_components', 'spr_min_component_share') and demo.GEOMETRY_KEYS == ('spr_depth', 'spr_knn', 'spr_faces')
    cfg = demo.load_config(NEAREST)
    assert not any(k in cfg for k in demo.SMOOTH_KEYS) and demo._smooth_rules(cfg) == {}
    cfg = demo.load_config(NEAREST, dict(geo_from='SPR', spr_smooth=10))
    assert demo._smooth_rules(cfg) == dict(smooth=dict(steps=10, lam=0.5, mu=-0.53))
    cfg = demo.load_config(NEAREST, dict(spr_smooth=5, spr_smooth_lambda=0.33, spr_smooth_mu=-0.34))
    assert demo._smooth_rules(cfg) == dict(smooth=dict(steps=5, lam=0.33, mu=-0.34))
    assert demo._smooth_rules(demo.load_config(NEAREST, dict(spr_smooth=2, spr_smooth_mu=0))) == dict(smooth=dict(steps=2, lam=0.5, mu=0.0))
    kw = demo._pipeline_kwargs(cfg)
    assert not any(k in kw for k in demo.SMOOTH_KEYS) and kw == demo._pipeline_kwargs(demo.load_config(NEAREST))
    for bad in (dict(spr_smooth=0), dict(spr_smooth=-1), dict(spr_smooth=True), dict(spr_smooth='10'), dict(spr_smooth=2.5), dict(spr_smooth=10001),
                dict(spr_smooth=3, spr_smooth_lambda=0), dict(spr_smooth=3, spr_smooth_lambda=1.5), dict(spr_smooth=3, spr_smooth_lambda='0.5'),
                dict(spr_smooth=3, spr_smooth_mu=0.1), dict(spr_smooth=3, spr_smooth_mu=-0.5), dict(spr_smooth=3, spr_smooth_mu=float('nan')),
                dict(spr_smooth=3, spr_smooth_lambda=1.0, spr_smooth_mu=-1.5), dict(spr_smooth_lambda=0.5), dict(spr_smooth_mu=-0.53)):
        with pytest.raises(ValueError, match='spr_smooth'):
            demo.load_config(NEAREST, bad)
    with pytest.raises(KeyError, match='spr_smoothing'):
        demo.load_config(NEAREST, dict(spr_smoothing=10))
    d = os.path.join(ROOT, 'configs')
    for f in sorted(os.listdir(d)):
        assert not any(k in demo.load_config(os.path.join(d, f)) for k in demo.SMOOTH_KEYS), f


# ---- the oracle
def test_oracle_on_a_tetrahedron_by_hand():
    """Every vertex of a tetrahedron has the other three as neighbours: one Laplacian pass with factor 1/2 moves it half way to their centroid."""
    out = msc.oracle_smooth(msc.TET_V, msc.TET, steps=1, lam=0.5, mu=0.0)
    s = 1 / 6
    assert np.array_equal(out, np.array([[s, s, s], [0.5, s, s], [s, 0.5, s], [s, s, 0.5]]).astype(np.float32))
    x = msc.TET_V.astype(np.float64)
    m0 = ((x[1] + x[2]) + x[3]) / 3.0
    assert np.array_equal(out[0], (x[0] + 0.5 * (m0 - x[0])).astype(np.float32))
    # held vertices and vertices no face names stay, bit for bit
    v = np.concatenate([msc.TET_V, [[7.0, 8.0, 9.0]]]).astype(np.float32)
    out, cnt = msc.oracle_smooth(v, msc.TET, steps=3, fixed=np.array([0, 1, 0, 0, 0]), return_counts=True)
    assert out[1].tobytes() == v[1].tobytes() and out[4].tobytes() == v[4].tobytes() and cnt == dict(moved=3, held=1, isolated=1, steps=3)


def test_boundary_oracle_on_hand_cases():
    mask, cnt = msc.oracle_boundary(msc.TET, 4)
    assert not mask.any() and cnt == dict(boundary_vertices=0, boundary_edges=0, nonmanifold_edges=0)
    mask, cnt = msc.oracle_boundary(msc.TET[:3], 4)                 # one face removed: its three edges and vertices are open
    assert mask.tolist() == [True, False, True, True] and cnt == dict(boundary_vertices=3, boundary_edges=3, nonmanifold_edges=0)
    v, f = msc.fan()
    mask, cnt = msc.oracle_boundary(f, len(v))
    assert mask.all() and cnt == dict(boundary_vertices=5, boundary_edges=6, nonmanifold_edges=1)
    v, f = bow_tie()
    assert not msc.oracle_boundary(f, len(v))[0].any()
    v, f = msc.sphere_cap()
    mask, cnt = msc.oracle_boundary(f, len(v))
    assert cnt['boundary_vertices'] == cnt['boundary_edges'] > 20 and cnt['nonmanifold_edges'] == 0       # one closed rim
    assert mask.sum() < len(np.unique(f)) < len(v)


def test_oracle_does_not_depend_on_face_order_or_rotation():
    from mesh_components_common import shuffled_and_rotated
    v, f = msc.noisy_sphere()
    a = msc.oracle_smooth(v, f, steps=3)
    assert a.tobytes() == msc.oracle_smooth(v, shuffled_and_rotated(f), steps=3).tobytes()


@pytest.mark.parametrize('mesh', ['sphere', 'torus'])
def test_taubin_removes_noise_and_keeps_the_volume_where_the_laplacian_shrinks(mesh):
    """10 steps of MeshLab's pair bring the RMS distance to the analytic surface to at most half and move the volume by at most 1 %; the same steps
    with mu = 0 lose more than 3 % of it.  (Figures of the oracle: RMS ratio 0.379 on the sphere, about 0.385 on the torus; volume 0.25 % / 0.53 %
    with the pair, 4.2 % / 9.2 % lost without.)"""
    from pointdreamer_amd import mesh_checks as mc, synthetic
    v, f = msc.noisy_sphere() if mesh == 'sphere' else msc.noisy_torus()
    sdf = synthetic.solid(mesh).sdf
    before, vol = msc.rms(sdf(v)), mc.signed_volume(v, f)
    assert 0.0045 < before < 0.0055
    t = msc.oracle_smooth(v, f, steps=10, lam=0.5, mu=-0.53)
    l = msc.oracle_smooth(v, f, steps=10, lam=0.5, mu=0.0)
    ratio, dv, lost = msc.rms(sdf(t)) / before, abs(mc.signed_volume(t, f) - vol) / vol, (vol - mc.signed_volume(l, f)) / vol
    print(f'{mesh}: rms {before:.5f} -> {msc.rms(sdf(t)):.5f} (ratio {ratio:.3f}), volume moved {100 * dv:.2f} %, Laplacian lost {100 * lost:.2f} %, '
          f'Laplacian rms {msc.rms(sdf(l)):.5f}')
    assert ratio <= 0.5
    assert dv <= 0.01
    assert lost > 0.03
