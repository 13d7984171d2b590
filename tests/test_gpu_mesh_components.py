"""Connected components, compaction and the removal of small pieces on the device (csrc/mesh_components.hip, pointdreamer_amd/mesh_components.py)
against the sequential oracle of tests/mesh_components_common.py: labels, roots and counts exactly, boxes numerically (== : a zero bound may carry
either sign), compacted vertices and colours byte for byte."""
import functools
import os

import numpy as np
import pytest
import torch

import mesh_components_common as mcc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = 'cuda'
T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def label(v, f, n=None):
    """label_components with statistics and boxes, as numpy; the call is made twice and the two results must have equal bytes."""
    from pointdreamer_amd import mesh_components as M
    n = len(v) if n is None else n
    runs = []
    for _ in range(2):
        vc, fc, st = M.label_components(T(f), n_vertices=n, vertices=T(v), return_stats=True)
        runs.append(dict(vertex_comp=vc.cpu().numpy(), face_comp=fc.cpu().numpy(), root=st['root'].cpu().numpy(), n_vertices=st['vertices'].cpu().numpy(),
                         n_faces=st['faces'].cpu().numpy(), box=st['box'].cpu().numpy(), count=st['count'], referenced=st['referenced'],
                         unreferenced=st['unreferenced']))
    for k, a in runs[0].items():
        assert (a.tobytes() == runs[1][k].tobytes()) if isinstance(a, np.ndarray) else a == runs[1][k], k
    return runs[0]


def check(got, v, f, n=None):
    o = mcc.oracle_components(f, len(v) if n is None else n, v)
    assert got['count'] == o['count']
    for k in ('vertex_comp', 'face_comp', 'root', 'n_vertices', 'n_faces'):
        assert got[k].dtype == np.int32 and np.array_equal(got[k], o[k]), k
    assert got['box'].dtype == np.float32 and got['box'].shape == o['box'].shape and (got['box'] == o['box']).all()
    assert got['referenced'] == (o['vertex_comp'] >= 0).sum() and got['unreferenced'] == (o['vertex_comp'] < 0).sum()
    return o


# ---- 1, 2: the smallest cases
def test_two_tetrahedra_and_an_unreferenced_vertex():
    v, f = mcc.two_tetrahedra()
    got = label(v, f)
    check(got, v, f)
    assert got['vertex_comp'].tolist() == [0, 0, 0, 0, -1, 1, 1, 1, 1] and got['root'].tolist() == [0, 5] and got['unreferenced'] == 1


def test_one_shared_vertex_or_a_repeated_index_connects():
    v, f = mcc.bow_tie()
    assert check(label(v, f), v, f)['count'] == 1
    v, f = mcc.joined_triangles()
    assert check(label(v, f), v, f)['count'] == 1
    assert check(label(v, f[:2]), v, f[:2])['count'] == 2


def test_without_vertices_and_without_statistics():
    from pointdreamer_amd import mesh_components as M
    v, f = mcc.two_tetrahedra()
    o = mcc.oracle_components(f, 9)
    vc, fc = M.label_components(T(f))                              # Vn from the largest index
    assert vc.dtype == torch.int32 and np.array_equal(vc.cpu().numpy(), o['vertex_comp']) and np.array_equal(fc.cpu().numpy(), o['face_comp'])
    vc, fc, st = M.label_components(T(f), n_vertices=12, return_stats=True)
    assert 'box' not in st and st['count'] == 2 and st['unreferenced'] == 4 and vc.cpu().numpy().tolist() == o['vertex_comp'].tolist() + [-1] * 3
    vc, fc, st = M.label_components(T(np.zeros((0, 3), np.int64)), n_vertices=5, return_stats=True)
    assert st['count'] == 0 and vc.cpu().numpy().tolist() == [-1] * 5 and fc.shape == (0,) and st['unreferenced'] == 5


# ---- 3: the long chain
def test_a_strip_of_4000_faces_in_three_index_orders():
    got = {}
    for order in ('ascending', 'descending', 'random'):
        v, f, perm = mcc.strip(4000, order)
        got[order] = (label(v, f), perm)
        o = check(got[order][0], v, f)
        assert o['count'] == 1 and got[order][0]['root'].tolist() == [0] and got[order][0]['n_faces'].tolist() == [4000]
    base, _ = got['ascending']
    for order in ('descending', 'random'):
        assert mcc.same_partition(base['vertex_comp'], got[order][0]['vertex_comp'], got[order][1])


# ---- 4: more components than the default capacity
def test_5000_separate_triangles_take_the_retry_path():
    from pointdreamer_amd import mesh_components as M
    v, f = mcc.separate_triangles(5000)
    assert 5000 > M.DEFAULT_CAPACITY
    got = label(v, f)
    check(got, v, f)
    assert got['count'] == 5000 and np.array_equal(got['root'], 3 * np.arange(5000)) and (np.diff(got['root']) > 0).all()
    assert (got['n_vertices'] == 3).all() and (got['n_faces'] == 1).all()


# ---- 5: three interleaved components
def test_three_interleaved_tori_do_not_depend_on_face_order_or_rotation():
    v, f, perm = mcc.three_tori(24, 12)
    got = label(v, f)
    check(got, v, f)
    assert got['count'] == 3 and got['n_faces'].tolist() == [576] * 3 and got['n_vertices'].tolist() == [288] * 3
    assert mcc.same_partition(np.repeat(np.arange(3), 288), got['vertex_comp'], perm)
    f2 = mcc.shuffled_and_rotated(f, seed=4)
    got2 = label(v, f2)
    check(got2, v, f2)
    for k in ('vertex_comp', 'root', 'n_vertices', 'n_faces', 'box'):
        assert got[k].tobytes() == got2[k].tobytes(), k


# ---- 6: the filter
@pytest.mark.parametrize("setting", range(len(mcc.FILTER_SETTINGS)), ids=['largest', 'min_faces', 'min_face_share', 'min_diameter_share', 'two_rules'])
def test_filter_components_equals_the_oracles_compaction(setting):
    from pointdreamer_amd import mesh_components as M, mesh_checks as mc
    rules = mcc.FILTER_SETTINGS[setting]
    v, f, col = mcc.blobs()
    assert mc.directed_edge_defects(f) == 0
    ov, of, oc, vmap, ocnt = mcc.oracle_filter(v, f, col, **rules)
    gv, gf, gc, cnt = M.filter_components(T(v), T(f), colors=T(col), return_counts=True, **rules)
    gv, gf, gc = gv.cpu().numpy(), gf.cpu().numpy(), gc.cpu().numpy()
    assert gv.dtype == np.float32 and gf.dtype == np.int64 and gc.dtype == np.float32
    assert gv.shape == ov.shape and gv.tobytes() == ov.tobytes() and gc.tobytes() == oc.tobytes() and np.array_equal(gf, of)
    assert np.array_equal(np.unique(gf), np.arange(len(gv)))       # every output vertex is referenced
    assert mc.directed_edge_defects(gf) == 0
    assert cnt == dict(components=14, components_kept=mcc.FILTER_KEPT[setting], faces_before=len(f), faces_after=len(of), vertices_before=len(v),
                       vertices_after=len(ov))
    gv2, gf2 = M.filter_components(T(v), T(f), **rules)            # without colours: the same mesh
    assert gv2.cpu().numpy().tobytes() == ov.tobytes() and np.array_equal(gf2.cpu().numpy(), of)


def test_compact_mesh_keeps_any_subset_of_faces_in_input_order():
    from pointdreamer_amd import mesh_components as M
    v, f, col = mcc.blobs()
    keep = np.random.default_rng(2).random(len(f)) < 0.3
    ov, of, oc, vmap = mcc.oracle_compact(v, f, keep, col)
    gv, gf, gc, gm = M.compact_mesh(T(v), T(f), T(keep), colors=T(col), return_map=True)
    assert gv.cpu().numpy().tobytes() == ov.tobytes() and gc.cpu().numpy().tobytes() == oc.tobytes()
    assert np.array_equal(gf.cpu().numpy(), of) and np.array_equal(gm.cpu().numpy(), vmap)
    gv, gf = M.compact_mesh(T(v), T(f), T(np.zeros(len(f), np.uint8)))
    assert gv.shape == (0, 3) and gf.shape == (0, 3)
    gv, gf = M.compact_mesh(T(v), T(f), T(np.ones(len(f), bool)))
    assert gv.cpu().numpy().tobytes() == v.tobytes() and np.array_equal(gf.cpu().numpy(), f)


# ---- 7: the tie
@pytest.mark.parametrize("swapped", [False, True], ids=['in-order', 'ranges-swapped'])
def test_largest_keeps_the_smaller_root_on_a_tie(swapped):
    from pointdreamer_amd import mesh_components as M
    v, f = mcc.twin_tetrahedra(swapped)
    check(label(v, f), v, f)
    ov, of, _, _ = mcc.oracle_filter(v, f, keep='largest')
    gv, gf, cnt = M.filter_components(T(v), T(f), keep='largest', return_counts=True)
    assert gv.cpu().numpy().tobytes() == ov.tobytes() == v[:4].tobytes() and np.array_equal(gf.cpu().numpy(), of)
    assert cnt['components'] == 2 and cnt['components_kept'] == 1


# ---- 8: refusals
def test_refusals():
    from pointdreamer_amd import mesh_components as M
    from pointdreamer_amd._lib import PdhipError
    v, f = mcc.two_tetrahedra()
    with pytest.raises(PdhipError, match='no CPU path'):
        M.label_components(torch.from_numpy(f))
    with pytest.raises(PdhipError, match='no CPU path'):
        M.filter_components(T(v), torch.from_numpy(f), keep='largest')
    bad = f.copy()
    bad[5, 1] = 9                                                  # == Vn
    with pytest.raises(PdhipError, match=r'pdhip_mesh_components.*face index outside \[0, Vn=9\)'):
        M.label_components(T(bad), n_vertices=9)
    with pytest.raises(PdhipError, match='pdhip_mesh_components'):
        M.filter_components(T(v), T(bad), keep='largest')
    with pytest.raises(PdhipError, match=r'pdhip_compact_mesh.*face index outside'):
        M.compact_mesh(T(v), T(bad), T(np.ones(8, bool)))
    nan = v.copy()
    nan[6, 1] = np.nan
    with pytest.raises(PdhipError, match='not finite'):
        M.label_components(T(f), vertices=T(nan), return_stats=True)
    nan = v.copy()
    nan[4] = np.inf                                                # the unreferenced vertex may hold anything
    check(label(nan, f), nan, f)
    with pytest.raises(ValueError, match='no rule given'):
        M.filter_components(T(v), T(f))
    with pytest.raises(ValueError, match='none of the 2 components'):
        M.filter_components(T(v), T(f), min_faces=5)
    with pytest.raises(ValueError, match='none of the 2 components'):
        M.filter_components(T(v), T(f), keep='largest', min_faces=5)


# ---- 9: end to end behind the reconstruction
@functools.lru_cache(maxsize=None)
def two_spheres_cloud():
    from pointdreamer_amd import synthetic
    xyz, rgb, _ = synthetic.solid('two_spheres').sample(25000, seed=1)
    return T(xyz), T(rgb)


def test_largest_component_of_a_two_spheres_reconstruction():
    from pointdreamer_amd import mesh_components as M, mesh_checks as mc, spr
    xyz, rgb = two_spheres_cloud()
    normals = spr.estimate_normals(xyz)
    mv, mf, mcol = spr.poisson_reconstruct(xyz, normals, depth=6, colors=rgb)
    v, f, col = mv.cpu().numpy(), mf.cpu().numpy(), mcol.cpu().numpy()
    assert len(mc.components_euler(len(v), f)) == 2
    ov, of, oc, _, ocnt = mcc.oracle_filter(v, f, col, keep='largest')
    gv, gf, gc = M.filter_components(mv, mf, colors=mcol, keep='largest')
    assert gv.cpu().numpy().tobytes() == ov.tobytes() and gc.cpu().numpy().tobytes() == oc.tobytes() and np.array_equal(gf.cpu().numpy(), of)
    plain = spr.recon_one_shape_SPR(xyz, rgb, depth=6, return_counts=True)
    assert plain[3]['faces'] == len(f) and plain[3]['vertices'] == len(v) and 'components' not in plain[3]
    none = spr.recon_one_shape_SPR(xyz, rgb, depth=6, return_counts=True, keep_components=None)
    assert none[0].shape == plain[0].shape and none[1].shape == plain[1].shape and none[3]['faces'] == len(f) and 'components' not in none[3]
    rv, rf, rcol, rc = spr.recon_one_shape_SPR(xyz, rgb, depth=6, return_counts=True, keep_components='largest')
    assert rc['components'] == 2 and rc['components_kept'] == 1 and rc['faces'] == len(of) and rc['faces_reconstructed'] == len(f)
    assert rv.cpu().numpy().tobytes() == ov.tobytes() and rcol.cpu().numpy().tobytes() == oc.tobytes() and np.array_equal(rf.cpu().numpy(), of)
    comps = mc.components_euler(len(rv), rf.cpu().numpy())
    assert len(comps) == 1 and comps[0][3] == 2 and mc.directed_edge_defects(rf.cpu().numpy()) == 0
    dv, df, _, dc = spr.recon_one_shape_SPR(xyz, rgb, depth=6, return_counts=True, keep_components=dict(keep='largest'), target_faces=2000)
    assert dc['components'] == 2 and dc['components_kept'] == 1 and dc['faces_reconstructed'] == len(f) and dc['faces'] == len(df) <= 2001
    comps = mc.components_euler(len(dv), df.cpu().numpy())
    assert len(comps) == 1 and comps[0][3] == 2


# ---- 10: the demo key
def test_demo_key_keeps_the_largest_component(tmp_path, caplog):
    import logging
    from pointdreamer_amd import demo, io_utils, mesh_checks as mc, synthetic
    xyz, rgb, _ = synthetic.solid('two_spheres').sample(16000, seed=5)
    pc = str(tmp_path / 'two.ply')
    io_utils.save_colored_pc_ply(xyz * 1.7 + 0.3, rgb, pc)
    base = ["--config", os.path.join(ROOT, "configs", "nearest.yaml"), "--pc_file", pc, "--set", "geo_from=SPR", "xatlas_texture_res=256", "cam_res=128",
            "res=64", "point_validation_by_o3d=False"]

    def geometry(out):
        path = os.path.join(out, 'geo', f'{os.path.basename(out)}_untextured', 'models', 'model_normalized.obj')
        v, f = io_utils.load_obj_mesh(path)
        return v, f, mc.components_euler(len(v), f)

    with caplog.at_level(logging.INFO, logger='pointdreamer_amd'):
        out = demo.main(base + [f"output_path={tmp_path / 'largest'}", "spr_components=largest"])[0]
    v1, f1, comps = geometry(out)
    assert len(comps) == 1 and comps[0][3] == 2 and mc.directed_edge_defects(f1) == 0
    assert 'SPR components: 2 found, 1 kept' in caplog.text and 'reconstructed faces dropped' in caplog.text
    mv, mf = io_utils.load_obj_mesh(os.path.join(out, 'models', 'model_normalized.obj'))
    assert len(mv) == len(v1) and len(mf) == len(f1)               # the textured mesh is the filtered one
    caplog.clear()
    with caplog.at_level(logging.INFO, logger='pointdreamer_amd'):
        out = demo.main(base + [f"output_path={tmp_path / 'all'}"])[0]
    v2, f2, comps = geometry(out)
    assert len(comps) == 2 and 'SPR components' not in caplog.text and len(f2) > len(f1)
