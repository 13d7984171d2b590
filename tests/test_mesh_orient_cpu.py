"""Orientation without a GPU: the oracle of tests/mesh_orient_common.py on the cases of the definition (include/pdhip.h, pdhip_orient_faces) against
what is known about them -- the original winding, mesh_checks' directed-edge defects and signed volume -- its invariance under face shuffles and
corner rotations, the sequential parity union-find against a 2-colouring, and the argument checks, which refuse before any device call."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import mesh_orient_common as moc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as ge
    ge.build()
    from pointdreamer_amd import _lib
    return _lib.lib()


@pytest.mark.parametrize("level", [0, 2])
def test_oracle_restores_randomly_flipped_and_inverted_icospheres(level):
    from pointdreamer_amd import mesh_checks as mc
    v, f = moc.icosphere(level)
    assert mc.directed_edge_defects(f) == 0 and mc.signed_volume(v, f) > 0
    g, mask = moc.random_flips(f, seed=level + 1)
    assert 0 < mask.sum() < len(f) and mc.directed_edge_defects(g) > 0
    o = moc.oracle_orient(v, g)
    assert o['faces'].tobytes() == f.tobytes() and np.array_equal(o['flip'], mask.astype(np.uint8))
    assert mc.directed_edge_defects(o['faces']) == 0 and mc.signed_volume(v, o['faces']) > 0
    assert o['counts'][:3] == [1, int(mask.sum()), 0] and o['counts'][3] > 0 and o['counts'][4:] == [0, 0, 0, 0]
    assert o['flags'].tolist() == [moc.CLOSED | moc.BY_VOLUME | (moc.COMPLEMENTED if mask[0] else 0)] and o['root'].tolist() == [0]
    inv = moc.flipped(f, slice(None))
    o = moc.oracle_orient(v, inv)
    assert o['faces'].tobytes() == f.tobytes() and o['counts'][1] == len(f) and o['counts'][3] == 0
    assert o['flags'].tolist() == [moc.CLOSED | moc.BY_VOLUME | moc.COMPLEMENTED] and o['vol'][0] < 0


def test_oracle_tetrahedron_every_flip_subset():
    from pointdreamer_amd import mesh_checks as mc
    assert mc.signed_volume(moc.TET_V, moc.TET_OUT) > 0
    for bits in range(16):
        mask = np.array([(bits >> k) & 1 for k in range(4)], bool)
        o = moc.oracle_orient(moc.TET_V, moc.flipped(moc.TET_OUT, mask))
        assert o['faces'].tobytes() == moc.TET_OUT.tobytes() and o['flip'].tolist() == mask.astype(int).tolist(), bits


def test_oracle_moebius_pillow_and_tiny_far_sphere():
    v, f = moc.moebius()
    assert len(f) == 16
    o = moc.oracle_orient(v, f)
    assert o['counts'][:3] == [1, 0, 1] and o['flags'].tolist() == [moc.NONORIENTABLE] and o['faces'].tobytes() == f.tobytes()
    assert o['counts'][4] == 16 and o['counts'][5] == 0 and o['vol'].tolist() == [0]
    assert moc.oracle_orient(v, f, 'volume')['flags'].tolist() == [moc.NONORIENTABLE]
    v, f = moc.pillow()
    o = moc.oracle_orient(v, f)
    assert o['flags'].tolist() == [moc.CLOSED] and o['vol'].tolist() == [0] and o['counts'] == [1, 0, 0, 0, 0, 0, 0, 0]
    assert o['faces'].tobytes() == f.tobytes()
    v, f, truth = moc.three_spheres()
    o = moc.oracle_orient(v, f)
    assert o['faces'].tobytes() == truth.tobytes() and o['root'].tolist() == [0, 320, 400] and o['flipped'].tolist() == [0, 80, 0]
    assert o['vol'][1] < -10 ** 11 and (o['flags'] & moc.BY_VOLUME).all()          # decided on the patch's OWN box: the sphere spans a few f32 steps
    print('tiny far sphere: vol', o['vol'].tolist())


def test_oracle_open_patches_ties_and_nonmanifold_edges():
    v, f = moc.sheet()
    g = moc.flipped(f, [3, 10, 11, 24, 30, 41, 49])
    o = moc.oracle_orient(v, g)
    assert o['faces'].tobytes() == f.tobytes() and o['flags'].tolist() == [0] and o['counts'][1] == 7 and o['counts'][4] == 20
    v, f = moc.two_face_strip()
    o = moc.oracle_orient(v, moc.flipped(f, [1]))
    assert o['flip'].tolist() == [0, 1] and o['faces'].tobytes() == f.tobytes() and o['flags'].tolist() == [0]
    o = moc.oracle_orient(v, moc.flipped(f, [0]))                   # the tie keeps the ROOT's winding: face 1 follows face 0
    assert o['flip'].tolist() == [0, 1] and o['flags'].tolist() == [0]
    v, f = moc.cap()
    inv = moc.flipped(f, slice(None))
    assert 20 < len(f) < 320
    assert moc.oracle_orient(v, inv, 'majority')['faces'].tobytes() == inv.tobytes()
    o = moc.oracle_orient(v, inv, 'volume')
    assert o['faces'].tobytes() == f.tobytes() and o['flags'].tolist() == [moc.BY_VOLUME | moc.COMPLEMENTED] and o['counts'][4] > 0
    v, f = moc.fan()
    o = moc.oracle_orient(v, f)
    assert o['counts'] == [3, 0, 0, 0, 6, 1, 0, 0] and o['face_patch'].tolist() == [0, 1, 2] and o['faces'].tobytes() == f.tobytes()
    v, f = moc.tets_on_an_edge()
    g = moc.flipped(f, [4, 5, 6, 7])
    o = moc.oracle_orient(v, g)                                    # the inverted tetrahedron is an OPEN patch: nothing is carried across the edge
    assert o['counts'] == [2, 0, 0, 0, 0, 1, 0, 0] and o['face_patch'].tolist() == [0] * 4 + [1] * 4 and o['faces'].tobytes() == g.tobytes()
    assert moc.oracle_orient(v, g, 'volume')['faces'].tobytes() == f.tobytes()
    o = moc.oracle_orient(v, moc.flipped(f, [2, 6]))               # (faces without the shared edge: three manifold edges each)
    assert o['faces'].tobytes() == f.tobytes() and o['counts'][1] == 2 and o['counts'][3] == 6


def test_oracle_keeps_degenerate_faces():
    v, f = moc.icosphere(0)
    g = np.concatenate([[[3, 3, 5]], f[:7], [[1, 2, 1]], f[7:], [[4, 4, 4]]])
    g = moc.flipped(g, [2, 9, 15])
    o = moc.oracle_orient(v, g)
    keep = np.ones(len(g), bool)
    keep[[0, 8, 22]] = False
    assert o['faces'][keep].tobytes() == f.tobytes() and o['faces'][~keep].tobytes() == g[~keep].tobytes()
    assert o['face_patch'][~keep].tolist() == [-1] * 3 and o['counts'] == [1, 3, 0, o['counts'][3], 0, 0, 3, 0] and o['root'].tolist() == [1]
    o = moc.oracle_orient(v, np.array([[0, 0, 1], [2, 2, 2]]))
    assert o['counts'] == [0, 0, 0, 0, 0, 0, 2, 0] and len(o['root']) == 0


@pytest.mark.parametrize("case", ["icosphere", "spheres", "sheet"])
def test_oracle_is_invariant_under_face_shuffles_and_corner_rotations(case):
    if case == "icosphere":
        v, f = moc.icosphere(2)
        f = moc.random_flips(f, seed=5)[0]
    elif case == "spheres":
        v, f, _ = moc.three_spheres()
    else:
        v, f = moc.sheet()
        f = moc.flipped(f, [3, 10, 11, 24, 30, 41, 49])
    a = moc.oracle_orient(v, f)
    g, perm, rot = moc.shuffle_rotate(f, seed=6)
    b = moc.oracle_orient(v, g)
    # new face k is old face perm[k]: flips and patches map back through the patches' faces, the oriented faces are the same triangles
    assert np.array_equal(np.sort(b['n_faces']), np.sort(a['n_faces'])) and b['counts'] == a['counts']
    ids = {}
    for k in range(len(g)):
        ids.setdefault(int(b['face_patch'][k]), int(a['face_patch'][perm[k]]))
        assert ids[int(b['face_patch'][k])] == int(a['face_patch'][perm[k]])
    back = {pb: pa for pb, pa in ids.items()}
    for pb, pa in back.items():
        # (rel is relative to the root, the smallest face index, which the shuffle changes: a root of the other winding complements the patch
        # and negates its volume; everything else is the same)
        other = int(b['flags'][pb] ^ a['flags'][pa])
        assert other in (0, moc.COMPLEMENTED) and b['vol'][pb] == (-a['vol'][pa] if other else a['vol'][pa]) and b['n_faces'][pb] == a['n_faces'][pa]
    assert np.array_equal(b['flip'], a['flip'][perm])               # (no tie in these cases: the flips do not depend on which face is the root)
    canon = lambda t: np.stack([np.roll(r, -int(np.argmin(r))) for r in t])
    assert np.array_equal(canon(b['faces']), canon(a['faces'][perm]))


def test_sequential_parity_union_against_a_colouring():
    rng = np.random.default_rng(7)
    n = 300
    colour = rng.integers(0, 2, n)
    pairs = rng.integers(0, n, (500, 2))
    parity = (colour[pairs[:, 0]] ^ colour[pairs[:, 1]]).astype(np.uint8)
    root, rel, conflict = moc.oracle_parity_union(n, pairs, parity)
    assert not conflict.any() and np.array_equal(rel, colour ^ colour[root])
    for k in (3, 4, 5):
        cyc = np.stack([np.arange(k), (np.arange(k) + 1) % k], 1)
        assert moc.oracle_parity_union(k, cyc, np.ones(k, np.uint8))[2].tolist() == [k % 2] * k


# ---- the driver's keys, the binding, the refusals
def test_demo_validates_the_orient_keys():
    from pointdreamer_amd import demo
    cfg = os.path.join(ROOT, 'configs', 'nearest.yaml')
    c = demo.load_config(cfg, dict(mesh_orient='coherent', mesh_orient_open='volume'))
    assert c.mesh_orient == 'coherent' and c.mesh_orient_open == 'volume'
    assert demo.load_config(cfg, dict(mesh_orient='coherent')).get('mesh_orient_open') is None
    assert 'mesh_orient' not in demo.load_config(cfg)
    assert demo.load_config(cfg, dict(mesh_clean='weld', mesh_orient='coherent')).mesh_clean == 'weld'
    for over in (dict(mesh_orient='outward'), dict(mesh_orient=True), dict(mesh_orient_open='majority'), dict(mesh_orient='coherent', mesh_orient_open='area'),
                 dict(mesh_clean='coherent')):
        with pytest.raises(ValueError):
            demo.load_config(cfg, over)


def test_entries_are_exported_and_declared(L):
    import re
    from pointdreamer_amd import _lib
    txt = open(os.path.join(ROOT, 'include', 'pdhip.h')).read()
    for s in ('pdhip_orient_faces', 'pdhip_debug_parity_union'):
        assert hasattr(L, s) and s in _lib._SIGS and re.search(r'\bint ' + s + r'\(', txt), s
    assert len(_lib._SIGS['pdhip_orient_faces'][1]) == 30 and len(_lib._SIGS['pdhip_debug_parity_union'][1]) == 10
    assert not any('orient' in s and s.endswith(('_ws_bytes', '_workspace_bytes', '_ws_ints')) for s in _lib._SIGS)
    src = open(os.path.join(ROOT, 'pointdreamer_amd', 'csrc', 'Makefile')).read()
    assert 'mesh_orient.hip' in src


P = C.c_void_p(4096)
ORIENT_ARGS = ('vertices', 'Vn', 'faces', 'F', 'open_patches', 'out_faces', 'flip', 'face_patch', 'patch_root', 'patch_faces', 'patch_flipped',
               'patch_flags', 'patch_vol', 'counts', 'keys_a', 'keys_b', 'vals_a', 'vals_b', 'sort_len', 'hist', 'hist_words', 'face_tmp', 'face_tmp_len',
               'box', 'box_len', 'tiles', 'tiles_len', 'misc', 'misc_len')
SIZES = dict(Vn=8, F=8, open_patches=0, sort_len=24, hist_words=512, face_tmp_len=40, box_len=48, tiles_len=2, misc_len=64)


def orient(L, **kw):
    args = [kw.get(a, SIZES.get(a, P)) for a in ORIENT_ARGS]
    return L.pdhip_orient_faces(*args, None)


@pytest.mark.parametrize("name", [a for a in ORIENT_ARGS if a not in SIZES])
def test_orient_refuses_null_pointers_by_name(L, name):
    assert orient(L, **{name: None}) == -1
    assert b'pdhip_orient_faces: null pointer (' + name.encode() + b')' in L.pdhip_last_error()


def test_orient_refuses_sizes_and_short_temporaries(L):
    for kw, word in ((dict(Vn=0), b'Vn=0'), (dict(F=0), b'F=0'), (dict(F=-2), b'F=-2'), (dict(Vn=(1 << 26) + 1), b'Vn=67108865'),
                     (dict(F=(1 << 23) + 1, sort_len=1 << 26, hist_words=1 << 26, face_tmp_len=1 << 26, box_len=1 << 26, tiles_len=1 << 26), b'F=8388609'),
                     (dict(open_patches=2), b'open_patches=2'), (dict(open_patches=-1), b'open_patches=-1')):
        assert orient(L, **kw) == -1 and word in L.pdhip_last_error(), kw
    big = dict(F=5000, sort_len=15000, hist_words=512 * 8, face_tmp_len=25000, box_len=30000, tiles_len=6)
    for arg, short, name in (('sort_len', 14999, b'keys_a / keys_b / vals_a / vals_b'), ('hist_words', 512 * 8 - 1, b'hist'),
                             ('face_tmp_len', 24999, b'face_tmp'), ('box_len', 29999, b'box'), ('tiles_len', 5, b'tiles'), ('misc_len', 63, b'misc')):
        assert orient(L, **dict(big, **{arg: short})) == -1
        msg = L.pdhip_last_error()
        assert b'pdhip_orient_faces: ' + name + b' holds ' + str(short).encode() in msg and b'F=5000 needs' in msg, msg


def test_parity_union_refuses_before_any_device_call(L):
    pu = L.pdhip_debug_parity_union                                # (pairs, parity, n_pairs, n, word, root, rel, conflict, status, stream)
    for args, words in (((P, P, 4, 0, P, P, P, P, P), (b'n=0',)), ((P, P, -1, 8, P, P, P, P, P), (b'n_pairs=-1',)),
                        ((P, P, 4, (1 << 26) + 1, P, P, P, P, P), (b'n=',)), ((None, P, 4, 8, P, P, P, P, P), (b'null pointer (pairs)', b'n_pairs=4')),
                        ((P, None, 4, 8, P, P, P, P, P), (b'null pointer (parity)',)), ((P, P, 4, 8, None, P, P, P, P), (b'null pointer (word)',)),
                        ((P, P, 4, 8, P, None, P, P, P), (b'null pointer (root)',)), ((P, P, 4, 8, P, P, None, P, P), (b'null pointer (rel)',)),
                        ((P, P, 4, 8, P, P, P, None, P), (b'null pointer (conflict)',)), ((P, P, 4, 8, P, P, P, P, None), (b'null pointer (status)',))):
        assert pu(*args, None) == -1
        msg = L.pdhip_last_error()
        assert b'pdhip_debug_parity_union' in msg and all(w in msg for w in words), msg


def test_mesh_orient_refuses_cpu_tensors_and_unknown_rules():
    from pointdreamer_amd import mesh_orient as M
    from pointdreamer_amd._lib import PdhipError
    v, f = torch.zeros((4, 3)), torch.zeros((2, 3), dtype=torch.int64)
    with pytest.raises(PdhipError):
        M.orient_faces(v, f)
    with pytest.raises(PdhipError):
        M.orientation_report(v, f)
    for bad in ('area', None, 1, True):
        with pytest.raises(ValueError):
            M.orient_faces(v, f, open_patches=bad)
