"""Coherent orientation on the device (csrc/mesh_orient.hip, pointdreamer_amd/mesh_orient.py) against the numpy oracle of tests/mesh_orient_common.py.
Every assertion on the entry is bit equality, on ALL its outputs, and every call is repeated once for equal bytes."""
import os
import re

import numpy as np
import pytest
import torch

import mesh_orient_common as moc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = 'cuda'
T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
DTYPES = dict(faces=np.int64, flip=np.uint8, face_patch=np.int32, root=np.int32, n_faces=np.int32, flipped=np.int32, flags=np.int32, vol=np.int64)
COUNT_KEYS = ('patches', 'flipped', 'nonorientable_patches', 'incoherent_edges', 'boundary_edges', 'nonmanifold_edges', 'degenerate')


def orient(v, f, open_patches='majority'):
    """orient_faces with every optional result, as numpy arrays under the oracle's keys; called twice: equal bytes, and the inputs stay as they were."""
    from pointdreamer_amd import mesh_orient as M
    tv, tf = T(v), T(f)
    runs = []
    for _ in range(2):
        faces, flip, p, c = M.orient_faces(tv, tf, open_patches=open_patches, return_flip=True, return_patches=True, return_counts=True)
        r = dict(faces=faces, flip=flip, face_patch=p['face_patch'], root=p['root'], n_faces=p['faces'], flipped=p['flipped'], flags=p['flags'],
                 vol=p['vol'])
        runs.append((dict((k, t.cpu().numpy()) for k, t in r.items()), c))
    for k in moc.OUTPUT_KEYS:
        assert runs[0][0][k].tobytes() == runs[1][0][k].tobytes() and runs[0][0][k].dtype == DTYPES[k], k
    assert runs[0][1] == runs[1][1]
    assert tv.cpu().numpy().tobytes() == np.ascontiguousarray(v).tobytes() and tf.cpu().numpy().tobytes() == np.ascontiguousarray(f).tobytes()
    return dict(runs[0][0], counts=[runs[0][1][k] for k in COUNT_KEYS] + [0])


def check(v, f, open_patches='majority'):
    got, want = orient(v, f, open_patches), moc.oracle_orient(v, f, open_patches)
    for k in moc.OUTPUT_KEYS:
        assert got[k].shape == want[k].shape and np.array_equal(got[k], want[k]), f'{k}: {int((got[k] != want[k]).sum())} of {want[k].size} differ'
    assert got['counts'] == want['counts']
    return got


@pytest.fixture(scope="module")
def ico2():
    return moc.icosphere(2)


def test_tetrahedron_every_flip_subset_comes_out_outward():
    for bits in range(16):
        mask = np.array([(bits >> k) & 1 for k in range(4)], bool)
        got = check(moc.TET_V, moc.flipped(moc.TET_OUT, mask))
        assert got['faces'].tobytes() == moc.TET_OUT.tobytes() and got['flip'].tolist() == mask.astype(int).tolist(), bits
        assert got['flags'].tolist() == [moc.CLOSED | moc.BY_VOLUME | (moc.COMPLEMENTED if mask[0] else 0)]


def test_icosphere_2_random_half_flipped_gives_the_original_bytes(ico2):
    v, f = ico2
    g, mask = moc.random_flips(f, seed=3)
    got = check(v, g)
    assert got['faces'].tobytes() == f.tobytes() and got['counts'][:3] == [1, int(mask.sum()), 0] and 100 < mask.sum() < 220


def test_icosphere_2_inverted_is_decided_by_volume_and_complemented(ico2):
    v, f = ico2
    got = check(v, moc.flipped(f, slice(None)))
    assert got['faces'].tobytes() == f.tobytes() and got['counts'][1] == 320 and got['flipped'].tolist() == [320]
    assert got['flags'].tolist() == [moc.CLOSED | moc.BY_VOLUME | moc.COMPLEMENTED] and got['vol'][0] < 0 and got['counts'][3] == 0


def test_icosphere_2_shuffled_and_rotated_equals_the_oracle(ico2):
    from pointdreamer_amd import mesh_checks as mc
    v, f = ico2
    g, perm, rot = moc.shuffle_rotate(moc.random_flips(f, seed=4)[0], seed=5)
    got = check(v, g)
    assert mc.directed_edge_defects(got['faces']) == 0 and mc.signed_volume(v, got['faces']) > 0


def test_icosphere_5_several_sort_tiles_and_the_tiled_scan():
    v, f = moc.icosphere(5)
    assert len(f) == 20480                                         # 61 440 half-edges: 30 sort tiles; F is past the one-workgroup scan
    g, mask = moc.random_flips(f, seed=6)
    got = check(v, g)
    assert got['faces'].tobytes() == f.tobytes() and got['counts'][1] == int(mask.sum())


def test_three_spheres_shuffled_patch_numbering_and_the_per_patch_box():
    v, f, truth = moc.three_spheres()
    got = check(v, f)
    assert got['faces'].tobytes() == truth.tobytes() and got['root'].tolist() == [0, 320, 400] and got['flipped'].tolist() == [0, 80, 0]
    assert got['vol'][1] < -10 ** 11 and (got['flags'] & moc.BY_VOLUME).all()
    g, perm, _ = moc.shuffle_rotate(f, seed=7)
    got = check(v, g)
    assert (np.diff(got['root']) > 0).all() and sorted(got['n_faces'].tolist()) == [80, 80, 320]
    assert np.array_equal(got['flip'], (np.arange(len(f)) // 80 == 4)[perm].astype(np.uint8))       # faces 320 .. 399, wherever they went


def test_moebius_strip_is_flagged_and_left_alone():
    v, f = moc.moebius()
    for rule in ('majority', 'volume'):
        got = check(v, f, rule)
        assert got['counts'][:3] == [1, 0, 1] and got['flags'].tolist() == [moc.NONORIENTABLE] and got['faces'].tobytes() == f.tobytes()


def test_open_sheet_is_restored_by_the_majority_and_a_tie_keeps_the_root():
    v, f = moc.sheet()
    got = check(v, moc.flipped(f, [3, 10, 11, 24, 30, 41, 49]))
    assert got['faces'].tobytes() == f.tobytes() and got['counts'][1] == 7 and got['flags'].tolist() == [0]
    v, f = moc.two_face_strip()
    got = check(v, moc.flipped(f, [1]))
    assert got['flip'].tolist() == [0, 1] and got['faces'].tobytes() == f.tobytes()
    assert check(v, moc.flipped(f, [0]))['flip'].tolist() == [0, 1]


def test_open_cap_volume_rule_turns_it_outward_majority_leaves_it():
    v, f = moc.cap()
    inv = moc.flipped(f, slice(None))
    assert check(v, inv, 'majority')['faces'].tobytes() == inv.tobytes()
    got = check(v, inv, 'volume')
    assert got['faces'].tobytes() == f.tobytes() and got['flags'].tolist() == [moc.BY_VOLUME | moc.COMPLEMENTED]


def test_nonmanifold_edges_carry_no_orientation():
    v, f = moc.fan()
    got = check(v, f)
    assert got['counts'] == [3, 0, 0, 0, 6, 1, 0, 0] and got['face_patch'].tolist() == [0, 1, 2]
    v, f = moc.tets_on_an_edge()
    g = moc.flipped(f, [4, 5, 6, 7])
    got = check(v, g)
    assert got['counts'] == [2, 0, 0, 0, 0, 1, 0, 0] and got['faces'].tobytes() == g.tobytes() and got['flags'].tolist() == [0, 0]
    assert check(v, g, 'volume')['faces'].tobytes() == f.tobytes()
    assert check(v, moc.flipped(f, [2, 6]))['faces'].tobytes() == f.tobytes()


def test_soup_has_a_patch_per_face_and_pairs_agree():
    """1 280 single-face patches and 300 two-face strips with one face flipped each: the per-patch decision over many waves, its totals summed per wave."""
    v, f = moc.icosphere(3)
    sv, sf = v[f.reshape(-1)], np.arange(3 * len(f), dtype=np.int64).reshape(-1, 3)
    tv, tf = moc.two_face_strip()
    strips = [(tv + np.float32(k), moc.flipped(tf, [k % 2])) for k in range(300)]
    jv, jf = moc.join([(sv, sf)] + strips)
    got = check(jv, jf)
    assert got['counts'][:3] == [1280 + 300, 300, 0] and got['counts'][4] == 3 * 1280 + 4 * 300 and (got['flags'] == 0).all()


def test_pillow_is_closed_with_zero_volume_and_untouched():
    v, f = moc.pillow()
    got = check(v, f)
    assert got['flags'].tolist() == [moc.CLOSED] and got['vol'].tolist() == [0] and got['faces'].tobytes() == f.tobytes()


def test_degenerate_faces_are_kept_as_given():
    v, f = moc.icosphere(0)
    g = moc.flipped(np.concatenate([[[3, 3, 5]], f[:7], [[1, 2, 1]], f[7:], [[4, 4, 4]]]), [2, 9, 15])
    got = check(v, g)
    assert got['face_patch'][[0, 8, 22]].tolist() == [-1] * 3 and got['counts'][6] == 3 and got['root'].tolist() == [1]
    assert got['faces'][[0, 8, 22]].tolist() == [[3, 3, 5], [1, 2, 1], [4, 4, 4]]
    got = check(v, np.array([[0, 0, 1], [2, 2, 2]]))
    assert got['counts'] == [0, 0, 0, 0, 0, 0, 2, 0]


def test_simplify_refuses_the_flipped_icosphere_and_takes_the_oriented_one(ico2):
    from pointdreamer_amd import mesh_orient as M, spr
    from pointdreamer_amd._lib import PdhipError
    v, f = ico2
    g = moc.random_flips(f, seed=8)[0]
    with pytest.raises(PdhipError):
        spr.simplify_mesh(T(v), T(g), target_faces=160)
    out = spr.simplify_mesh(T(v), M.orient_faces(T(v), T(g)), target_faces=160)
    assert 4 <= len(out[1]) <= 200
    rep = M.orientation_report(T(v), T(g))
    assert rep == dict(patches=1, would_flip=moc.oracle_orient(v, g)['counts'][1], nonorientable_patches=0, incoherent_edges=rep['incoherent_edges'],
                       boundary_edges=0, nonmanifold_edges=0, closed_patches=1) and rep['incoherent_edges'] > 0


def test_device_refusals_leave_the_outputs_untouched(ico2):
    from pointdreamer_amd import _lib, mesh_orient as M
    from pointdreamer_amd._lib import PdhipError, ptr, stream
    v, f = ico2
    bad_f = f.copy()
    bad_f[7, 1], bad_f[100, 0] = len(v), -1
    bad_v = v.copy()
    bad_v[f[5, 2], 1] = np.nan
    with pytest.raises(PdhipError, match=r'pdhip_orient_faces: a face index outside \[0, Vn=162\)'):
        M.orient_faces(T(v), T(bad_f))
    with pytest.raises(PdhipError, match=r'pdhip_orient_faces: a referenced vertex is not finite'):
        M.orient_faces(T(bad_v), T(f))
    lone = np.concatenate([v, [[np.inf, 0.0, 0.0]]]).astype(np.float32)      # an UNREFERENCED vertex may be anything
    assert M.orient_faces(T(lone), T(f)).cpu().numpy().tobytes() == f.tobytes()
    with pytest.raises(ValueError, match=r'no face'):
        M.orient_faces(T(v), T(f[:0]))
    # the entry itself, outputs filled with a sentinel
    L, F, dev = _lib.lib(), len(f), DEV
    i32 = lambda n: torch.full((n,), -7, dtype=torch.int32, device=dev)
    outs = dict(out_faces=torch.full((F, 3), -7, dtype=torch.int64, device=dev), flip=torch.full((F,), 9, dtype=torch.uint8, device=dev),
                face_patch=i32(F), patch_root=i32(F), patch_faces=i32(F), patch_flipped=i32(F), patch_flags=i32(F),
                patch_vol=torch.full((F,), -7, dtype=torch.int64, device=dev), counts=i32(8))
    keys, vals = torch.empty((2, 3 * F), dtype=torch.int64, device=dev), torch.empty((2, 3 * F), dtype=torch.int32, device=dev)
    hist, tmp, box, tiles, misc = i32(512), i32(5 * F), i32(6 * F), i32(2), i32(64)

    def call(tv, tf, Vn=len(v), open_patches=0, tmp_len=5 * F):
        return L.pdhip_orient_faces(ptr(tv), Vn, ptr(tf), F, open_patches, *[ptr(t) for t in outs.values()], ptr(keys[0]), ptr(keys[1]), ptr(vals[0]),
                                    ptr(vals[1]), 3 * F, ptr(hist), 512, ptr(tmp), tmp_len, ptr(box), 6 * F, ptr(tiles), 2, ptr(misc), 64, stream())

    for args, word in (((T(v), T(bad_f)), b'a face index outside'), ((T(bad_v), T(f)), b'not finite'), ((T(v), T(f), len(v), 2), b'open_patches=2'),
                       ((T(v), T(f), len(v), 0, 5 * F - 1), b'face_tmp holds'), ((T(v), T(f), 0), b'Vn=0')):
        assert call(*args) == -1 and word in L.pdhip_last_error(), word
        torch.cuda.synchronize()
        for name, t in outs.items():
            assert bool((t == (9 if name == 'flip' else -7)).all()), (word, name)
    assert call(T(v), T(f)) == 0 and outs['out_faces'].cpu().numpy().tobytes() == f.tobytes() and outs['counts'].tolist() == [1, 0, 0, 0, 0, 0, 0, 0]


def test_demo_key_orients_a_supplied_mesh(tmp_path, caplog, ico2):
    import logging
    from pointdreamer_amd import demo, io_utils, mesh_checks as mc, synthetic
    xyz, rgb = synthetic.sphere_points(20000, seed=3)
    v, f = ico2
    g, mask = moc.random_flips(f, seed=9)
    pc = str(tmp_path / 'ball.ply')
    io_utils.save_colored_pc_ply(xyz * 1.7 + 0.3, rgb, pc)
    io_utils.save_obj_mesh(v * np.float32(1.7) + np.float32(0.3), g, str(tmp_path / 'ball_untextured_mesh.obj'))
    base = ["--config", os.path.join(ROOT, "configs", "nearest.yaml"), "--pc_file", pc, "--set", "xatlas_texture_res=256", "cam_res=128", "res=64",
            "point_validation_by_o3d=False"]
    faces_of = lambda out: io_utils.load_obj_mesh(os.path.join(out, 'models', 'model_normalized.obj'))[1]
    with caplog.at_level(logging.INFO, logger='pointdreamer_amd'):
        out = demo.main(base + [f"output_path={tmp_path / 'plain'}"])[0]
    assert 'mesh_orient' not in caplog.text and mc.directed_edge_defects(faces_of(out)) > 0
    assert os.path.exists(os.path.join(out, 'geo', 'xatlas_256.pth')) and not os.path.exists(os.path.join(out, 'geo', 'xatlas_256_orient.pth'))
    caplog.clear()
    with caplog.at_level(logging.INFO, logger='pointdreamer_amd'):
        out = demo.main(base + [f"output_path={tmp_path / 'orient'}", "mesh_orient=coherent"])[0]
    line = re.search(r'mesh_orient: coherent \(open patches by majority\): 1 patches, (\d+) of 320 faces flipped, 0 non-orientable patches, (\d+) '
                     r'incoherent edges before', caplog.text)
    assert line and int(line.group(1)) == int(mask.sum()) and int(line.group(2)) > 0, caplog.text[-2000:]
    assert os.path.exists(os.path.join(out, 'geo', 'xatlas_256_orient.pth')) and not os.path.exists(os.path.join(out, 'geo', 'xatlas_256.pth'))
    got = np.asarray(faces_of(out), np.int64)
    assert mc.directed_edge_defects(got) == 0 and got.tobytes() == f.tobytes()
