"""Connected components and the removal of small pieces without a GPU: the sequential oracle of tests/mesh_components_common.py against scipy's
labelling (mesh_checks.components_euler) and hand cases, the C ABI (declared, exported, bound; the size queries), the refusals that come before
anything is dereferenced, the refusal of CPU tensors, the demo's opt-in keys, recon_one_shape_SPR's signature and zero scratch on the new kernels."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT
import mesh_components_common as mcc

LIB = os.path.join(ROOT, 'pointdreamer_amd', 'libpdhip.so')
SYMBOLS = ('pdhip_mesh_components_workspace_bytes', 'pdhip_mesh_components', 'pdhip_compact_mesh_workspace_bytes', 'pdhip_compact_mesh')
NEAREST = os.path.join(ROOT, 'configs', 'nearest.yaml')
VMAX, FMAX = 1 << 26, 1 << 23


def _lib():
    import __graft_entry__ as ge
    ge.build()
    from pointdreamer_amd import _lib
    return _lib.lib()


# ---- the oracle
def _sizes(o):
    return sorted(zip(o['n_vertices'].tolist(), o['n_faces'].tolist()))


def test_oracle_agrees_with_scipy_on_three_tori_and_the_bow_tie():
    from pointdreamer_amd import mesh_checks as mc
    for v, f in (mcc.three_tori()[:2], mcc.bow_tie()):
        o = mcc.oracle_components(f, len(v), v)
        ref = mc.components_euler(len(v), f)
        assert o['count'] == len(ref)
        assert _sizes(o) == sorted((c[0], c[2]) for c in ref)
    assert _sizes(mcc.oracle_components(mcc.three_tori()[1], 864)) == [(288, 576)] * 3
    assert mcc.oracle_components(mcc.bow_tie()[1], 7)['count'] == 1


def test_oracle_on_hand_cases():
    v, f = mcc.two_tetrahedra()
    o = mcc.oracle_components(f, 9, v)
    assert o['vertex_comp'].tolist() == [0, 0, 0, 0, -1, 1, 1, 1, 1] and o['face_comp'].tolist() == [0] * 4 + [1] * 4
    assert o['root'].tolist() == [0, 5] and o['n_vertices'].tolist() == [4, 4] and o['n_faces'].tolist() == [4, 4]
    assert o['box'].tolist() == [[-0.5] * 3 + [-0.25] * 3, [0.125] * 3 + [0.625] * 3]     # (vertex 4, at 9, is in no box)
    v, f = mcc.joined_triangles()
    assert mcc.oracle_components(f, 6)['count'] == 1 and mcc.oracle_components(f[:2], 6)['count'] == 2
    for order in ('ascending', 'descending', 'random'):
        v, f, perm = mcc.strip(4000, order)
        o = mcc.oracle_components(f, 4002, v)
        assert o['count'] == 1 and o['root'].tolist() == [0] and o['n_faces'].tolist() == [4000] and (o['vertex_comp'] == 0).all()
    v, f = mcc.separate_triangles(5000)
    o = mcc.oracle_components(f, 15000)
    assert o['count'] == 5000 and np.array_equal(o['root'], 3 * np.arange(5000)) and np.array_equal(o['face_comp'], np.arange(5000))
    o = mcc.oracle_components(np.zeros((0, 3), np.int64), 5)
    assert o['count'] == 0 and o['vertex_comp'].tolist() == [-1] * 5


def test_oracle_does_not_depend_on_face_order_rotation_or_labels():
    v, f, perm = mcc.three_tori()
    a = mcc.oracle_components(f, len(v))
    b = mcc.oracle_components(mcc.shuffled_and_rotated(f), len(v))
    assert np.array_equal(a['vertex_comp'], b['vertex_comp']) and a['root'].tolist() == b['root'].tolist()
    plain = np.repeat(np.arange(3), 288)                           # torus k of the unpermuted vertex k n + i
    assert mcc.same_partition(plain, a['vertex_comp'], perm) and not mcc.same_partition(np.roll(plain, 1), a['vertex_comp'], perm)


def test_selection_rules_and_the_tie_rule():
    v, f, col = mcc.blobs()
    o = mcc.oracle_components(f, len(v), v)
    assert o['count'] == 14 and sorted(o['n_faces'].tolist()) == [20] * 12 + [320, 1280]
    for rules, kept in zip(mcc.FILTER_SETTINGS, mcc.FILTER_KEPT):
        ok = mcc.oracle_select(o, **rules)
        assert ok.sum() == kept and ok[np.argmax(o['n_faces'])], rules
        ov, of, oc, vmap, cnt = mcc.oracle_filter(v, f, col, **rules)
        assert cnt == dict(components=14, components_kept=kept) and len(np.unique(of)) == len(ov) == (vmap >= 0).sum() and len(oc) == len(ov)
        assert np.array_equal(ov[of], v[f[ok[o['face_comp']]]])      # the same triangles, in input order
    for swapped in (False, True):
        tv, tf = mcc.twin_tetrahedra(swapped)
        o = mcc.oracle_components(tf, 8, tv)
        assert o['n_faces'].tolist() == [4, 4] and mcc.oracle_select(o, keep='largest').tolist() == [True, False]
        ov, of, _, _ = mcc.oracle_filter(tv, tf, keep='largest')
        assert np.array_equal(ov, tv[:4])                           # the one with the smaller root: whichever tetrahedron holds vertex 0


# ---- the C ABI
def test_header_declares_and_library_exports_the_symbols():
    L = _lib()
    from pointdreamer_amd import _lib as lib_mod
    txt = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'pdhip.h')).read(), flags=re.S)
    for s in SYMBOLS:
        assert re.search(r'\b%s\s*\(' % s, txt), f"{s} is not declared in include/pdhip.h"
        assert hasattr(L, s) and s in lib_mod._SIGS, s
    assert len(lib_mod._SIGS['pdhip_mesh_components'][1]) == 14 and len(lib_mod._SIGS['pdhip_compact_mesh'][1]) == 13
    assert lib_mod._SIGS['pdhip_mesh_components_workspace_bytes'] == (C.c_size_t, [C.c_int, C.c_int]) == lib_mod._SIGS['pdhip_compact_mesh_workspace_bytes']
    assert not any(s.endswith('_ws_bytes') for s in SYMBOLS)       # (tests/test_ws_bytes_cpu.py fixes that set)


def test_size_queries_are_non_zero_and_monotone():
    L = _lib()
    for q in (L.pdhip_mesh_components_workspace_bytes, L.pdhip_compact_mesh_workspace_bytes):
        for Vn, F in ((0, 10), (-1, 10), (10, -1), (VMAX + 1, 10), (10, FMAX + 1)):
            assert q(Vn, F) == 0, (Vn, F)
        assert q(1, 0) > 0 and q(VMAX, FMAX) > 0
        sizes = [q(Vn, 20000) for Vn in (1, 9, 10000, 1000000, VMAX)]
        assert all(a <= b for a, b in zip(sizes, sizes[1:])) and sizes[0] > 0 and sizes[-1] > sizes[0], sizes
        sizes = [q(10000, F) for F in (0, 8, 20000, 2000000, FMAX)]
        assert all(a <= b for a, b in zip(sizes, sizes[1:])) and sizes[0] > 0, sizes
    assert L.pdhip_compact_mesh_workspace_bytes(10000, FMAX) > L.pdhip_compact_mesh_workspace_bytes(10000, 8)
    assert L.pdhip_mesh_components_workspace_bytes(1000000, 2000000) < 1000000 * 32     # five ints per vertex, nothing per face


def test_components_refuses_null_pointers_and_sizes_by_name_before_any_launch():
    L = _lib()
    one = C.c_void_p(256)                                          # (never dereferenced: the arguments are refused first)
    ok = dict(faces=one, F=8, vertices=one, Vn=9, vertex_comp=one, face_comp=one, comp_root=one, comp_vertices=one, comp_faces=one, comp_box=one,
              comp_capacity=16, counts=one, ws=one, stream=None)
    order = list(ok)
    call = lambda **kw: L.pdhip_mesh_components(*[dict(ok, **kw)[k] for k in order])
    for name in ('faces', 'vertex_comp', 'face_comp', 'comp_root', 'comp_vertices', 'comp_faces', 'counts', 'ws', 'vertices'):
        assert call(**{name: None}) == -1
        msg = L.pdhip_last_error()
        assert b'pdhip_mesh_components' in msg and b'null pointer' in msg and ('(%s)' % name).encode() in msg, msg
    for kw, word in ((dict(Vn=0), b'Vn=0'), (dict(Vn=-4), b'Vn=-4'), (dict(F=-1), b'F=-1'), (dict(F=FMAX + 1), b'F=8388609'),
                     (dict(Vn=VMAX + 1), b'Vn=67108865'), (dict(comp_capacity=-1), b'comp_capacity=-1')):
        assert call(**kw) == -1
        assert b'pdhip_mesh_components' in L.pdhip_last_error() and word in L.pdhip_last_error(), (kw, L.pdhip_last_error())


def test_compact_refuses_null_pointers_and_sizes_by_name_before_any_launch():
    L = _lib()
    one = C.c_void_p(256)
    ok = dict(vertices=one, Vn=9, faces=one, F=8, colors=one, face_keep=one, out_vertices=one, out_faces=one, out_colors=one, vertex_map=one,
              counts=one, ws=one, stream=None)
    order = list(ok)
    call = lambda **kw: L.pdhip_compact_mesh(*[dict(ok, **kw)[k] for k in order])
    for name in ('vertices', 'faces', 'face_keep', 'out_vertices', 'out_faces', 'counts', 'ws'):
        assert call(**{name: None}) == -1
        msg = L.pdhip_last_error()
        assert b'pdhip_compact_mesh' in msg and b'null pointer' in msg and ('(%s)' % name).encode() in msg, msg
    for kw in (dict(colors=None), dict(out_colors=None)):
        assert call(**kw) == -1 and b'go together' in L.pdhip_last_error()
    for kw, word in ((dict(Vn=0), b'Vn=0'), (dict(F=-1), b'F=-1'), (dict(F=FMAX + 1), b'F=8388609'), (dict(Vn=VMAX + 1), b'Vn=67108865')):
        assert call(**kw) == -1
        assert b'pdhip_compact_mesh' in L.pdhip_last_error() and word in L.pdhip_last_error(), (kw, L.pdhip_last_error())


def test_no_scratch_on_the_new_kernels():
    if not os.path.exists(LIB):
        _lib()
    pytest.importorskip('msgpack')                                 # (as tests/test_code_objects_cpu.py: the metadata note is msgpack)
    from tools import code_object_notes
    mine = [k for k in code_object_notes.kernels(LIB) if 'k_mc_' in k['name']]
    names = ' '.join(k['name'] for k in mine)
    for must in ('k_mc_init', 'k_mc_hook', 'k_mc_compress', 'k_mc_union', 'k_mc_flatten', 'k_mc_comp_init', 'k_mc_vertex_out', 'k_mc_face_out',
                 'k_mc_empty', 'k_mc_pack_mark', 'k_mc_pack_vertices', 'k_mc_pack_faces'):
        assert must in names, must
    for k in mine:
        print(k['name'], 'vgprs', k['vgpr_count'], 'lds', k['group_segment_fixed_size'], 'scratch', k['private_segment_fixed_size'])
        assert k['arch'] == 'gfx950'
        assert k['vgpr_spill_count'] == 0 and k['private_segment_fixed_size'] == 0, k
        assert k['group_segment_fixed_size'] == (256 if 'k_mc_vertex_out' in k['name'] else 0), k      # (the block's count of referenced vertices)


# ---- python
def test_cpu_tensors_are_refused_and_rules_are_checked_first():
    from pointdreamer_amd import mesh_components as M
    from pointdreamer_amd._lib import PdhipError
    v, f = (torch.from_numpy(a) for a in mcc.two_tetrahedra())
    with pytest.raises(PdhipError, match='no CPU path'):
        M.label_components(f)
    with pytest.raises(PdhipError, match='no CPU path'):
        M.label_components(f, vertices=v, return_stats=True)
    with pytest.raises(PdhipError, match='no CPU path'):
        M.filter_components(v, f, keep='largest')
    with pytest.raises(PdhipError, match='no CPU path'):
        M.compact_mesh(v, f, torch.ones(8, dtype=torch.bool))
    with pytest.raises(PdhipError, match='no CPU path'):
        M.label_components(f.numpy())
    with pytest.raises(ValueError, match='no rule given'):
        M.filter_components(v, f)
    assert M.DEFAULT_CAPACITY == 4096
    src = open(os.path.join(ROOT, 'pointdreamer_amd', 'mesh_components.py')).read()
    assert 'oracle' not in src and 'mesh_components_common' not in src and 'scipy' not in src


def test_select_components_equals_the_oracle_on_host_tensors():
    """The selection is torch plumbing over the per-component arrays: on the blobs' oracle statistics it gives the oracle's mask."""
    from pointdreamer_amd import mesh_components as M
    v, f, _ = mcc.blobs()
    o = mcc.oracle_components(f, len(v), v)
    stats = dict(root=torch.from_numpy(o['root']), vertices=torch.from_numpy(o['n_vertices']), faces=torch.from_numpy(o['n_faces']),
                 box=torch.from_numpy(o['box']), count=o['count'])
    for rules in mcc.FILTER_SETTINGS:
        assert np.array_equal(M.select_components(stats, **rules).numpy(), mcc.oracle_select(o, **rules)), rules
    for bad in (dict(keep='biggest'), dict(min_faces=-1), dict(min_faces=2.5), dict(min_face_share=1.5), dict(min_diameter_share=-0.1),
                dict(min_face_share='0.5'), dict()):
        with pytest.raises(ValueError):
            M.select_components(stats, **bad)


def test_recon_one_shape_SPR_keeps_the_reference_signature():
    from pointdreamer_amd import spr
    p = inspect.signature(spr.recon_one_shape_SPR).parameters
    names = list(p)
    assert names[:6] == ['coords', 'colors', 'gt_normals', 'save_path', 'depth', 'simplify_face_num']
    assert all(p[n].kind == inspect.Parameter.POSITIONAL_OR_KEYWORD for n in names[:6])
    assert names.index('keep_components') > names.index('target_faces')
    assert p['keep_components'].kind == inspect.Parameter.KEYWORD_ONLY and p['keep_components'].default is None
    for bad in ('biggest', {}, dict(largest=True), ['largest']):
        with pytest.raises(ValueError, match='keep_components'):
            spr.recon_one_shape_SPR(np.zeros((10, 3), np.float32), np.zeros((10, 3), np.float32), keep_components=bad)


# ---- demo config
def test_demo_accepts_the_component_keys_and_validates_them():
    from pointdreamer_amd import demo
    assert demo.COMPONENT_KEYS == ('spr_components', 'spr_min_component_share')
    assert demo.GEOMETRY_KEYS == ('spr_depth', 'spr_knn', 'spr_faces')
    cfg = demo.load_config(NEAREST)
    assert not any(k in cfg for k in demo.COMPONENT_KEYS) and demo._component_rules(cfg) == {}
    assert demo._component_rules(demo.load_config(NEAREST, dict(spr_components='all'))) == {}
    cfg = demo.load_config(NEAREST, dict(geo_from='SPR', spr_components='largest'))
    assert demo._component_rules(cfg) == dict(keep_components=dict(keep='largest'))
    cfg = demo.load_config(NEAREST, dict(spr_components='largest', spr_min_component_share=1))
    assert demo._component_rules(cfg) == dict(keep_components=dict(keep='largest', min_face_share=1.0))
    cfg = demo.load_config(NEAREST, dict(spr_min_component_share=0.05))
    assert demo._component_rules(cfg) == dict(keep_components=dict(min_face_share=0.05))
    kw = demo._pipeline_kwargs(cfg)
    assert not any(k in kw for k in demo.COMPONENT_KEYS) and kw == demo._pipeline_kwargs(demo.load_config(NEAREST))
    for bad in (dict(spr_components='biggest'), dict(spr_components=True), dict(spr_components=1)):
        with pytest.raises(ValueError, match='spr_components'):
            demo.load_config(NEAREST, bad)
    for bad in (dict(spr_min_component_share=0), dict(spr_min_component_share=0.0), dict(spr_min_component_share=1.5),
                dict(spr_min_component_share=-0.1), dict(spr_min_component_share='0.5'), dict(spr_min_component_share=True),
                dict(spr_min_component_share=float('nan'))):
        with pytest.raises(ValueError, match='spr_min_component_share'):
            demo.load_config(NEAREST, bad)
    with pytest.raises(KeyError, match='spr_component'):
        demo.load_config(NEAREST, dict(spr_component='largest'))


def test_no_shipped_config_sets_the_keys():
    from pointdreamer_amd import demo
    d = os.path.join(ROOT, 'configs')
    for f in sorted(os.listdir(d)):
        assert not any(k in demo.load_config(os.path.join(d, f)) for k in demo.COMPONENT_KEYS), f
