"""Welding and cleaning on the device (csrc/mesh_clean.hip, pointdreamer_amd/mesh_clean.py) against the numpy oracle of tests/mesh_clean_common.py.
Every assertion is bit equality: rep, vertices, colours, faces, maps, counts."""
import os
import re

import numpy as np
import pytest
import torch

import mesh_clean_common as mcc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = 'cuda'
T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def weld(v, tol=0.0):
    """weld_vertices with counts, as numpy; called twice: equal bytes (case 11), and the input stays as it was."""
    from pointdreamer_amd import mesh_clean as M
    tv = T(v)
    runs = [M.weld_vertices(tv, tolerance=tol, return_counts=True) for _ in range(2)]
    a, b = (r[0].cpu().numpy() for r in runs)
    assert a.dtype == np.int32 and a.shape == (len(v),) and a.tobytes() == b.tobytes() and runs[0][1] == runs[1][1]
    assert tv.cpu().numpy().tobytes() == np.ascontiguousarray(v).tobytes()
    c = runs[0][1]
    assert c['classes'] == int((a == np.arange(len(v))).sum()) and c['merged'] == len(v) - c['classes']
    return a, c


def check_weld(v, tol=0.0, want=None):
    got, c = weld(v, tol)
    want = mcc.oracle_weld(v, tol) if want is None else want
    assert got.tobytes() == want.tobytes(), f'{(got != want).sum()} of {len(v)} representatives differ'
    return got, c


def clean(v, f, colors=None, tol=0.0):
    from pointdreamer_amd import mesh_clean as M
    args = (T(v), T(f)) + ((T(colors),) if colors is not None else ())
    kw = dict(tolerance=tol, return_map=True, return_face_index=True, return_counts=True)
    runs = [M.clean_mesh(*args[:2], colors=args[2] if colors is not None else None, **kw) for _ in range(2)]
    outs = [[t.cpu().numpy() for t in r[:-1]] for r in runs]
    assert all(a.tobytes() == b.tobytes() and a.dtype == b.dtype for a, b in zip(*outs)) and runs[0][-1] == runs[1][-1]
    keys = ['vertices', 'faces'] + (['colors'] if colors is not None else []) + ['vertex_map', 'face_index']
    return dict(zip(keys, outs[0]), counts=runs[0][-1])


def check_clean(v, f, colors=None, tol=0.0, rep=None):
    got = clean(v, f, colors, tol)
    want = mcc.oracle_clean(v, f, colors, tol, rep=rep)
    for k, dt in (('vertices', np.float32), ('faces', np.int64), ('colors', np.float32), ('vertex_map', np.int32), ('face_index', np.int64)):
        if k in want:
            assert got[k].dtype == dt and got[k].shape == want[k].shape and got[k].tobytes() == want[k].tobytes(), k
    assert got['counts'] == want['counts']
    return got


# ---- 1: the smallest soup
@pytest.mark.parametrize("negative_zero", [False, True])
def test_two_tetrahedra_soup_welds_to_eight_vertices(negative_zero):
    v, f = mcc.two_tetrahedra_soup(negative_zero)
    rep, c = check_weld(v)
    assert c['classes'] == 8 and c['merged'] == 16
    got = check_clean(v, f)
    assert len(got['vertices']) == 8 and len(got['faces']) == 8 and got['counts']['degenerate'] == got['counts']['duplicate'] == 0
    assert got['vertices'].tobytes() == v[np.unique(rep)].tobytes()              # the representative's own bits (its -0.0 too)


# ---- 2, 3, 4: icosphere soups
def test_icosphere_2_soup_becomes_the_indexed_icosphere():
    from pointdreamer_amd import mesh_checks as mc
    v, f = mcc.icosphere(2)
    sv, sf = mcc.soup(v, f)
    got = check_clean(sv, sf)
    assert len(got['vertices']) == 162 and len(got['faces']) == 320
    assert got['vertices'][got['faces']].tobytes() == v[f].tobytes()              # the same triangles, corner for corner, in face order
    assert mc.directed_edge_defects(got['faces']) == 0


def test_icosphere_4_soup_several_sort_tiles():
    v, f = mcc.icosphere(4)
    sv, sf = mcc.soup(v, f)
    assert len(sv) == 15360
    rep = mcc.oracle_weld_exact(sv)
    check_weld(sv, want=rep)
    got = check_clean(sv, sf, rep=rep)
    assert len(got['vertices']) == len(v) and len(got['faces']) == len(f)


def test_icosphere_5_soup_past_the_one_workgroup_scan():
    v, f = mcc.icosphere(5)
    sv, sf = mcc.soup(v, f)
    assert len(sv) == 61440 and len(sf) == 20480
    rep = mcc.oracle_weld_exact(sv)
    check_weld(sv, want=rep)
    got = check_clean(sv, sf, rep=rep)
    assert len(got['vertices']) == len(v) == 10242 and len(got['faces']) == 20480


# ---- 5: chains (single linkage)
def test_chains_close_spacing_is_one_class_wide_spacing_none():
    tol = 1e-3
    v = mcc.chain(3000, 0.9 * tol, seed=3)
    x = v.astype(np.float64)
    step = np.sort(np.linalg.norm(np.diff(x[np.argsort(x[:, 0])], axis=0), axis=1))
    assert step[-1] < 0.95 * tol and step[0] > 0.85 * tol
    rep, c = check_weld(v, tol)
    assert c['classes'] == 1 and (rep == 0).all() and c['cells_per_axis'] >= 16
    print('chain: cells per axis', c['cells_per_axis'], 'wide queries', c['wide_queries'])
    w = mcc.chain(3000, 1.1 * tol, seed=4)
    rep, c = check_weld(w, tol)
    assert c['classes'] == 3000 and np.array_equal(rep, np.arange(3000))


# ---- 6: exact thresholds, across a cell face and in clamped boundary cells
def threshold_cloud(rng_seed=5):
    """2 048 points in [0, 8]^3: the two box corners, six slots for the pairs (filled by the caller), a filler far from the pairs."""
    rng = np.random.default_rng(rng_seed)
    v = (rng.random((2048, 3)) * np.array([7.0, 2.0, 2.0]) + np.array([0.5, 5.0, 5.0])).astype(np.float32)
    v[0], v[1] = (0.0, 0.0, 0.0), (8.0, 8.0, 8.0)
    return v


@pytest.mark.parametrize("apart", ["exact", "next"])
def test_pairs_at_exactly_the_tolerance_merge_and_the_next_float_does_not(apart):
    tol = 0.25
    v = threshold_cloud()
    v[2:8] = 4.0                                                   # placeholders: Vn, the box and tol fix the grid
    _, c = weld(v, tol)
    C = c['cells_per_axis']
    cs = 8.0 / C * (1.0 + 1.0e-6)                                  # the cell edge (include/pdhip.h)
    assert 8 <= C <= 31 and cs > tol
    far = np.float32(0.25) if apart == "exact" else np.nextafter(np.float32(0.25), np.float32(1.0))
    face = 3 * cs                                                  # a cell face in the interior
    xa = np.float32(np.floor(face * 64.0 - 8.0) / 64.0)            # a multiple of 1/64 about 1/8 below the face: xa + 1/4 is exact in f32
    v[2], v[3] = (xa, 1.0, 1.0), (np.float32(xa + np.float32(0.25)), 1.0, 1.0)
    assert np.floor(float(v[2, 0]) / cs) == 2 and np.floor(float(v[3, 0]) / cs) == 3      # the pair straddles the face
    if apart == "next":
        v[3, 0] = np.nextafter(v[3, 0], np.float32(100.0))
    v[4] = (far, 0.0, 0.0)                                         # with the corner (0, 0, 0): boundary cell 0
    v[5] = (8.0, np.float32(8.0) - far, 8.0)                       # with the corner (8, 8, 8): the last cell, which the far corner is clamped into
    v[6], v[7] = (2.0, 2.0, 0.0), (2.0, 2.0, far)                  # a pair along z in the boundary layer z = 0
    if apart == "next":
        v[5, 1] = np.nextafter(np.float32(7.75), np.float32(0.0))
    x = v.astype(np.float64)
    d2 = lambda i, j: ((x[i, 0] - x[j, 0]) ** 2 + (x[i, 1] - x[j, 1]) ** 2) + (x[i, 2] - x[j, 2]) ** 2
    pairs = [(2, 3), (0, 4), (1, 5), (6, 7)]
    for i, j in pairs:
        assert (d2(i, j) == tol * tol) if apart == "exact" else (tol * tol < d2(i, j) < tol * tol * (1 + 1e-5)), (i, j, d2(i, j))
    rep, c2 = check_weld(v, tol)
    assert c2['cells_per_axis'] == C
    for i, j in pairs:
        assert (rep[j] == rep[i] == i) if apart == "exact" else (rep[j] == j and rep[i] == i), (i, j)
    # the same pairs with the tolerance one f64 below 1/4: apart
    rep, _ = check_weld(v, np.nextafter(0.25, 0.0))
    assert all(rep[j] == j for _, j in pairs)


# ---- 7: a crowded cell (the quadratic path)
@pytest.mark.parametrize("tol", [0.0, 5e-4])
def test_crowd_of_copies_of_one_point(tol):
    v = mcc.crowd()
    assert len(v) == 7000
    want = mcc.oracle_weld_exact(v) if tol == 0.0 else mcc.oracle_weld(v, tol)
    rep, c = check_weld(v, tol, want=want)
    assert c['classes'] == (1 + 2000 if tol == 0.0 else len(np.unique(want))) and c['classes'] < 2001 + (tol == 0.0)


# ---- 8: jittered duplicates, permuted and shuffled
def test_jittered_triplicates_of_icosphere_3():
    tol = 2e-3
    v, f = mcc.icosphere(3)
    jv, jf = mcc.jittered_copies(v, f, 3, 0.4 * tol, seed=8)
    pv, pf = mcc.permuted(jv, jf, seed=9)
    pf = mcc.shuffled_and_rotated(pf, seed=10)
    got = check_clean(pv, pf, tol=tol)
    assert len(got['vertices']) == len(v) == 642 and len(got['faces']) == len(f) == 1280 and got['counts']['merged'] == 2 * 642


# ---- 9: faces
def test_duplicate_degenerate_and_collapsing_faces():
    from pointdreamer_amd import mesh_clean as M
    base = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1], [1, 1, 1], [2, 2, 2]], np.float32)
    v = np.concatenate([base, base[[0, 1]], [[5.0, 5.0, 5.0]]]).astype(np.float32)       # 6, 7 are copies of 0, 1; 8 is unreferenced
    f = np.array([[0, 1, 2],                                         # kept
                  [1, 2, 0],                                         # rotated duplicate
                  [2, 1, 0],                                         # reversed duplicate
                  [6, 7, 2],                                         # a duplicate only after welding: the third of the set
                  [0, 6, 3],                                         # collapses only after welding
                  [3, 3, 4],                                         # degenerate as given
                  [5, 4, 3],                                         # kept
                  [3, 4, 5],                                         # its duplicate
                  [1, 3, 2]], np.int64)
    got = check_clean(v, f)
    assert got['face_index'].tolist() == [0, 6, 8] and got['counts']['degenerate'] == 2 and got['counts']['duplicate'] == 4
    assert got['counts']['merged'] == 2 and got['counts']['unreferenced'] == 1 and len(got['vertices']) == 6
    assert got['faces'].tolist() == [[0, 1, 2], [5, 4, 3], [1, 3, 2]]
    rep = M.weld_vertices(T(v))
    rf, keep, counts = M._clean_faces(T(f), rep, len(v))
    wf, wkeep, wc = mcc.oracle_clean_faces(f, rep.cpu().numpy())
    assert rf.cpu().numpy().tobytes() == wf.tobytes() and np.array_equal(keep.cpu().numpy().astype(bool), wkeep)
    assert counts.tolist() == [wc['degenerate'], wc['duplicate'], wc['kept'], 0]
    # the smallest face index of a set stays, wherever the set lies: the same faces in reverse order
    check_clean(v, f[::-1].copy())


# ---- 10: colours and maps
def test_colours_are_the_representatives_and_the_maps_compose():
    tol = 1e-3
    v, f = mcc.icosphere(2)
    jv, jf = mcc.jittered_copies(v, f, 2, 0.4 * tol, seed=11)
    extra = np.array([[3.0, 3.0, 3.0], [3.0, 3.0, 3.0], [-3.0, 0.0, 0.0]], np.float32)      # unreferenced: a welded pair and a single
    jv = np.concatenate([jv[:100], extra, jv[100:]]).astype(np.float32)
    jf = jf + 3 * (jf >= 100)
    col = np.random.default_rng(12).random((len(jv), 3), dtype=np.float32)
    got = check_clean(jv, jf, col, tol)
    rep = mcc.oracle_weld(jv, tol)
    vm, fi = got['vertex_map'], got['face_index']
    assert got['counts']['unreferenced'] >= 2 and (vm[100:103] == -1).all() and got['counts']['merged'] >= 162 + 1
    live = vm >= 0
    assert got['vertices'][vm[live]].tobytes() == jv[rep[live]].tobytes() and got['colors'][vm[live]].tobytes() == col[rep[live]].tobytes()
    assert np.array_equal(got['faces'], vm[jf[fi]])                 # output face k is input face face_index[k] through vertex_map


# ---- 12: refusals on the device
def test_device_refusals():
    from pointdreamer_amd import mesh_clean as M
    from pointdreamer_amd._lib import PdhipError
    v, f = mcc.two_tetrahedra_soup()
    bad = v.copy()
    bad[3, 1], bad[17, 0] = np.nan, np.inf
    with pytest.raises(PdhipError, match=r'pdhip_weld_vertices: 2 vertex / vertices with a non-finite coordinate'):
        M.weld_vertices(T(bad))
    with pytest.raises(PdhipError, match=r'non-finite'):
        M.clean_mesh(T(bad), T(f))
    g = f.copy()
    g[2, 1], g[5, 0] = 24, -1
    with pytest.raises(PdhipError, match=r'pdhip_clean_faces: 2 face\(s\) with an index outside \[0, Vn=24\)'):
        M.clean_mesh(T(v), T(g))
    flat = np.zeros((6, 3), np.float32)                            # every face collapses
    with pytest.raises(ValueError, match=r'none of the 2 faces is left \(2 degenerate'):
        M.clean_mesh(T(flat), T(np.arange(6).reshape(2, 3)))
    with pytest.raises(ValueError, match=r'no face'):
        M.clean_mesh(T(v), T(f[:0]))
    rep = M.mesh_report(T(flat), T(np.arange(6).reshape(2, 3)))    # the report of a mesh that cleaning would leave nothing of
    assert (rep['faces_after'], rep['vertices_after'], rep['degenerate'], rep['merged'], rep['unreferenced']) == (0, 0, 2, 5, 1)
    assert rep['components'] == 2 and rep['boundary_edges'] == 6
    with pytest.raises(PdhipError, match=r'2097153 vertices exceed 2\^21'):
        M.clean_mesh(torch.zeros(((1 << 21) + 1, 3), device=DEV), T(f))
    rep = M.mesh_report(T(v), T(f))
    assert rep['boundary_edges'] == 24 and rep['components'] == 8 and rep['merged'] == 16 and rep['vertices_after'] == 8
    cv, cf = M.clean_mesh(T(v), T(f))
    rep = M.mesh_report(cv, cf)
    assert rep['boundary_edges'] == 0 and rep['nonmanifold_pairs'] == 0 and rep['components'] == 2 and rep['merged'] == 0


# ---- 13: the demo keys
def test_demo_key_welds_a_supplied_soup(tmp_path, caplog):
    import logging
    from pointdreamer_amd import demo, io_utils, synthetic
    from pointdreamer_amd.extract_texture_map import uv_unwrap
    xyz, rgb = synthetic.sphere_points(20000, seed=3)
    v, f = mcc.icosphere(2)
    sv, sf = mcc.soup(v * np.float32(1.7) + np.float32(0.3), f)    # off-centre / scaled like the cloud: the driver normalises both
    pc = str(tmp_path / 'ball.ply')
    io_utils.save_colored_pc_ply(xyz * 1.7 + 0.3, rgb, pc)
    io_utils.save_obj_mesh(sv, sf, str(tmp_path / 'ball_untextured_mesh.obj'))
    base = ["--config", os.path.join(ROOT, "configs", "nearest.yaml"), "--pc_file", pc, "--set", "xatlas_texture_res=256", "cam_res=128", "res=64",
            "point_validation_by_o3d=False"]

    def charts(out):
        ov, of = io_utils.load_obj_mesh(os.path.join(out, 'models', 'model_normalized.obj'))
        fc = uv_unwrap(T(np.asarray(ov, np.float32)), T(np.asarray(of, np.int64)), 256, return_charts=True)[2]
        return len(ov), len(of), len(torch.unique(fc))

    with caplog.at_level(logging.INFO, logger='pointdreamer_amd'):
        out = demo.main(base + [f"output_path={tmp_path / 'weld'}", "mesh_clean=weld"])[0]
    line = re.search(r'mesh_clean: weld at tolerance 0: vertices 960 -> 162 \(798 merged, 0 unreferenced\), faces 320 -> 320 \(0 degenerate, 0 '
                     r'duplicate\); after cleaning: 0 boundary edges, 0 non-manifold edges, 1 components', caplog.text)
    assert line, caplog.text[-2000:]
    assert os.path.exists(os.path.join(out, 'geo', 'xatlas_256_weld.pth')) and not os.path.exists(os.path.join(out, 'geo', 'xatlas_256.pth'))
    nv_w, nf_w, charts_welded = charts(out)
    caplog.clear()
    with caplog.at_level(logging.INFO, logger='pointdreamer_amd'):
        out = demo.main(base + [f"output_path={tmp_path / 'plain'}"])[0]
    assert 'mesh_clean' not in caplog.text
    assert os.path.exists(os.path.join(out, 'geo', 'xatlas_256.pth')) and not os.path.exists(os.path.join(out, 'geo', 'xatlas_256_weld.pth'))
    nv_s, nf_s, charts_soup = charts(out)
    print('charts welded', charts_welded, 'charts soup', charts_soup)
    assert (nv_w, nf_w) == (162, 320) and (nv_s, nf_s) == (960, 320)
    assert charts_welded < charts_soup
