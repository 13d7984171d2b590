"""Farthest-point subsampling on the device (csrc/subsample.hip, pointdreamer_amd/subsample.py, the demo's opt-in `subsample` key).  pdhip_fps is held
to BIT EQUALITY with the brute-force float64 oracle of tests/subsample_common.py (idx exactly, min_d2 as uint64): the pruning skips a cell only when a
lower bound that never exceeds a member's computed d2 proves it unchanged, and neither the minimum nor the arg-max (value, then smaller index) depends
on the visiting order.  pdhip_owner_mean_colors is held to bit equality with the int64 oracle: integer sums do not depend on the order either."""
import os

import numpy as np
import pytest
import torch

import subsample_common as sc

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENT_D2, SENT_IDX, SENT_CNT, SENT_COL = -7.0, -77, -777, -5.0


def T(a):
    return torch.from_numpy(np.array(a)).to(DEV)                  # (a writable copy: the cached clouds are read-only)


def run_fps(points, M, start=0, null=None, N=None, ws=None):
    """(rc, idx, min_d2, counts) of pdhip_fps; the outputs start as sentinels.  null: the name of an argument passed as NULL.  ws: the workspace to use instead of a
    fresh torch.empty one."""
    from pointdreamer_amd import _lib
    from pointdreamer_amd._lib import ptr, stream
    L = _lib.lib()
    tp = T(np.asarray(points, np.float32).reshape(-1, 3))
    N = tp.shape[0] if N is None else N
    cap = max(min(M, 1 << 20), 1)
    idx = torch.full((cap,), SENT_IDX, dtype=torch.int32, device=DEV)
    d2 = torch.full((cap,), SENT_D2, dtype=torch.float64, device=DEV)
    counts = torch.full((4,), SENT_CNT, dtype=torch.int32, device=DEV)
    if ws is None:
        ws = torch.empty((max(L.pdhip_fps_workspace_bytes(N, M), 8),), dtype=torch.uint8, device=DEV)
    a = dict(points=ptr(tp), idx=ptr(idx), min_d2=ptr(d2), counts=ptr(counts), ws=ptr(ws))
    if null is not None:
        a[null] = None
    rc = L.pdhip_fps(a['points'], N, M, start, a['idx'], a['min_d2'], a['counts'], a['ws'], stream())
    torch.cuda.synchronize()
    return rc, idx.cpu().numpy(), d2.cpu().numpy(), counts.cpu().numpy()


def check_case(name):
    p, M, start = sc.case(name)
    oidx, od2 = sc.oracle_case(name)
    rc, idx, d2, counts = run_fps(p, M, start)
    assert rc == 0
    print(name, 'N', len(p), 'M', M, 'counts', counts.tolist(), 'N*M', len(p) * M, 'idx unequal', int((idx != oidx).sum()),
          'min_d2 unequal', int((d2.view(np.uint64) != od2.view(np.uint64)).sum()))
    assert np.array_equal(idx, oidx)
    assert np.array_equal(d2.view(np.uint64), od2.view(np.uint64))
    assert 1 <= counts[0] <= 40 and 1 <= counts[1] <= counts[0] ** 3 and counts[3] == 0
    assert len(p) <= counts[2] <= len(p) * M                       # never more work than the brute-force scan
    return counts


# ---- bit equality
@pytest.mark.parametrize("name", ['one', 'five', 'identical', 'lattice', 'plane', 'line', 'clustered'])
def test_picks_equal_the_oracle_bit_for_bit(name):
    counts = check_case(name)
    if name in ('one', 'identical'):
        assert counts[0] == 1 and counts[1] == 1                   # a box without extent: one cell
    if name == 'identical':
        assert sc.oracle_case(name)[0].tolist() == list(range(10))


def test_large_cloud_equals_the_oracle_and_is_pruned():
    """100 000 -> 2 000 on a noisy sphere.  The brute-force scan performs N M = 2e8 point updates; the cell list must stay below a tenth of that
    (a condition that pruning happened, not a tuning target; profiles/subsample_parity.txt has the measured value)."""
    p, M, _ = sc.case('large')
    counts = check_case('large')
    assert counts[2] < len(p) * M // 10


@pytest.mark.parametrize("cells", [1, 3, 40])
def test_every_grid_gives_the_same_bytes(cells):
    """pdhip_debug_set_fps_cells: one cell (every pick updates every point), a coarse grid, the finest one (most cells empty)."""
    from pointdreamer_amd import _lib
    L = _lib.lib()
    for name in ('lattice', 'random', 'plane'):
        p, M, start = sc.case(name)
        oidx, od2 = sc.oracle_case(name)
        old = L.pdhip_debug_set_fps_cells(cells)
        try:
            rc, idx, d2, counts = run_fps(p, M, start)
        finally:
            L.pdhip_debug_set_fps_cells(old)
        assert old == 0 and rc == 0 and counts[0] == cells
        assert np.array_equal(idx, oidx) and np.array_equal(d2.view(np.uint64), od2.view(np.uint64))
        assert cells > 1 or counts[2] == len(p) * (M - 1)          # one cell: the brute-force scan, less the update behind the last pick


# ---- properties
def test_prefix_of_a_longer_run():
    p, M, start = sc.case('random')
    _, idx, d2, _ = run_fps(p, M, start)
    for m in (1, 2, 57, M - 1):
        rc, pidx, pd2, _ = run_fps(p, m, start)
        assert rc == 0 and np.array_equal(pidx, idx[:m]) and np.array_equal(pd2.view(np.uint64), d2[:m].view(np.uint64))
    assert np.all(np.diff(d2[1:]) <= 0.0) and np.isinf(d2[0]) and idx[0] == start


def test_two_calls_give_equal_bytes():
    p, M, start = sc.case('clustered')
    a, b = run_fps(p, M, start), run_fps(p, M, start)
    for x, y in zip(a[1:], b[1:]):
        assert x.tobytes() == y.tobytes()


def test_permuted_input_selects_the_same_points():
    p, M, start = sc.case('random')
    oidx, od2, ties = sc.oracle_fps(p, M, start, return_ties=True)
    assert ties == 0                                               # the precondition: without ties the index rule never decides
    perm = np.random.default_rng(4).permutation(len(p))           # new[j] = old[perm[j]]
    inv = np.argsort(perm)
    rc, idx, d2, _ = run_fps(p[perm], M, int(inv[start]))
    assert rc == 0
    assert np.array_equal(perm[idx], oidx) and np.array_equal(d2.view(np.uint64), od2.view(np.uint64))


def test_python_wrapper_returns_int64_picks_and_subsample_cloud_gathers():
    from pointdreamer_amd import subsample
    p, M, start = sc.case('random')
    oidx, od2 = sc.oracle_case('random')
    tp = T(p)
    idx, d2, counts = subsample.farthest_point_sample(tp, M, start=start, return_min_d2=True, return_counts=True)
    assert idx.dtype == torch.int64 and idx.shape == (M,) and np.array_equal(idx.cpu().numpy(), oidx)
    assert np.array_equal(d2.cpu().numpy().view(np.uint64), od2.view(np.uint64)) and counts.shape == (4,)
    assert torch.equal(subsample.farthest_point_sample(tp, 5, start=start), idx[:5])
    tc = torch.rand((len(p), 3), device=DEV)
    sp, scol, sidx = subsample.subsample_cloud(tp, tc, num=M, start=start)
    assert torch.equal(sidx, idx) and torch.equal(sp, tp[idx]) and torch.equal(scol, tc[idx])
    same = subsample.subsample_cloud(tp, tc, num=len(p))          # N <= num: the inputs themselves, no kernel
    assert same[0] is tp and same[1] is tc and torch.equal(same[2], torch.arange(len(p), device=DEV))


# ---- mean colours
def run_mean(owner, colors, M, fallback, with_ws=True, null=None, ws=None):
    from pointdreamer_amd import _lib
    from pointdreamer_amd._lib import ptr, stream
    L = _lib.lib()
    to, tc, tf = T(np.asarray(owner, np.int32)), T(np.asarray(colors, np.float32)), T(np.asarray(fallback, np.float32))
    out = torch.full((M, 3), SENT_COL, dtype=torch.float32, device=DEV)
    if ws is None:
        ws = torch.empty((L.pdhip_owner_mean_colors_workspace_bytes(M),), dtype=torch.uint8, device=DEV)
    a = dict(owner=ptr(to), colors=ptr(tc), fallback=ptr(tf), out=ptr(out))
    if null is not None:
        a[null] = None
    rc = L.pdhip_owner_mean_colors(a['owner'], a['colors'], to.shape[0], M, a['fallback'], a['out'], ptr(ws) if with_ws else None, stream())
    torch.cuda.synchronize()
    return rc, out.cpu().numpy()


def test_mean_colours_equal_the_integer_oracle_and_do_not_depend_on_the_order():
    from pointdreamer_amd import subsample
    p, c, idx = sc.color_case()
    owner = sc.oracle_nearest_sample(p, p[idx])
    want = sc.oracle_mean_colors(owner, c, len(idx), c[idx])
    for with_ws in (True, False):
        rc, out = run_mean(owner, c, len(idx), c[idx], with_ws)
        assert rc == 0 and np.array_equal(out.view(np.uint32), want.view(np.uint32))
    perm = np.random.default_rng(6).permutation(len(p))
    rc, out = run_mean(owner[perm], c[perm], len(idx), c[idx])
    assert rc == 0 and np.array_equal(out.view(np.uint32), want.view(np.uint32))
    # the python path: owners from pdhip_nearest_points
    got = subsample.owner_mean_colors(T(p), T(c), T(idx.astype(np.int64)))
    assert np.array_equal(got.cpu().numpy().view(np.uint32), want.view(np.uint32))
    sp, scol, sidx = subsample.subsample_cloud(T(p), T(c), num=len(idx), colors_from='mean')
    assert np.array_equal(sidx.cpu().numpy(), idx) and np.array_equal(scol.cpu().numpy().view(np.uint32), want.view(np.uint32))
    assert np.abs(want - c[idx]).max() > 0.05                      # (it is a filter: the means differ from the samples' own colours)


def test_a_duplicate_sample_owns_nothing_and_takes_its_fallback():
    p = np.array([[0, 0, 0], [1, 0, 0], [0, 0, 0], [0.1, 0, 0], [0.9, 0, 0]], np.float32)
    c = np.array([[0.0] * 3, [1.0] * 3, [0.5] * 3, [0.25] * 3, [0.75] * 3], np.float32)
    idx = np.array([0, 1, 2], np.int32)                            # sample 2 duplicates sample 0: the smallest position owns the tie
    owner = sc.oracle_nearest_sample(p, p[idx])
    assert owner.tolist() == [0, 1, 0, 0, 1]
    rc, out = run_mean(owner, c, 3, c[idx])
    assert rc == 0 and np.array_equal(out, sc.oracle_mean_colors(owner, c, 3, c[idx]))
    assert np.array_equal(out, np.array([[0.25] * 3, [0.875] * 3, [0.5] * 3], np.float32))


@pytest.mark.parametrize("bad,word", [(1.5, b'outside [0, 1]'), (-0.25, b'outside [0, 1]'), (float('nan'), b'non-finite'), (float('inf'), b'non-finite')])
def test_mean_colours_refuse_a_bad_colour(bad, word):
    from pointdreamer_amd import _lib
    p, c, idx = sc.color_case()
    owner = np.zeros(len(p), np.int32)
    c = np.array(c)
    c[1234, 1] = bad
    rc, out = run_mean(owner, c, len(idx), c[idx])
    assert rc == -1 and word in _lib.lib().pdhip_last_error() and np.all(out == SENT_COL)


def test_mean_colours_refuse_an_owner_outside_the_selection_and_null_pointers():
    from pointdreamer_amd import _lib
    p, c, idx = sc.color_case()
    owner = np.zeros(len(p), np.int32)
    owner[77] = len(idx)
    rc, out = run_mean(owner, c, len(idx), c[idx])
    assert rc == -1 and b'owner' in _lib.lib().pdhip_last_error() and np.all(out == SENT_COL)
    for name in ('owner', 'colors', 'fallback', 'out'):
        rc, out = run_mean(np.zeros(len(p), np.int32), c, len(idx), c[idx], null=name)
        assert rc == -1 and name.encode() in _lib.lib().pdhip_last_error() and np.all(out == SENT_COL)


# ---- refusals
def untouched(idx, d2, counts):
    return np.all(idx == SENT_IDX) and np.all(d2 == SENT_D2) and np.all(counts == SENT_CNT)


@pytest.mark.parametrize("null", ['points', 'idx', 'min_d2', 'counts', 'ws'])
def test_fps_refuses_a_null_pointer_by_name(null):
    from pointdreamer_amd import _lib
    p, _, _ = sc.case('five')
    rc, idx, d2, counts = run_fps(p, 3, 0, null=null)
    assert rc == -1 and b'null pointer (%s)' % null.encode() in _lib.lib().pdhip_last_error() and untouched(idx, d2, counts)


@pytest.mark.parametrize("N,M,start,word", [(0, 1, 0, b'N=0'), ((1 << 24) + 1, 5, 0, b'2^24'), (5, 0, 0, b'M=0'), (5, 6, 0, b'M=6'),
                                            (5, 3, 5, b'start=5'), (5, 3, -1, b'start=-1')])
def test_fps_refuses_bad_sizes_and_starts(N, M, start, word):
    from pointdreamer_amd import _lib
    p, _, _ = sc.case('five')
    rc, idx, d2, counts = run_fps(p, M, start, N=N)                # (refused before any launch: the buffer of 5 points is never read)
    assert rc == -1 and word in _lib.lib().pdhip_last_error() and untouched(idx, d2, counts)


@pytest.mark.parametrize("bad", [float('nan'), float('inf'), float('-inf')])
def test_fps_refuses_a_non_finite_coordinate(bad):
    from pointdreamer_amd import _lib, subsample
    p = np.array(sc.case('plane')[0])
    p[1501, 1] = bad
    p[17, 2] = bad
    rc, idx, d2, counts = run_fps(p, 100, 0)
    assert rc == -1 and b'2 point(s) with a non-finite coordinate' in _lib.lib().pdhip_last_error() and untouched(idx, d2, counts)
    with pytest.raises(_lib.PdhipError, match='non-finite'):
        subsample.farthest_point_sample(T(p), 100)


# ---- demo
def test_demo_subsamples_a_cloud_above_the_limit(tmp_path):
    from pointdreamer_amd import demo, io_utils, synthetic
    sh = synthetic.make_shape(40000, A=64, stacks=8, slices=16, seed=7)
    pc = str(tmp_path / 'big.ply')
    io_utils.save_colored_pc_ply(sh['points'] * 1.7 + 0.3, sh['colors'], pc)
    base = ["--config", os.path.join(ROOT, "configs", "nearest.yaml"), "--pc_file", pc, "--set", "xatlas_texture_res=256",
            "point_validation_by_o3d=False"]
    with pytest.raises(NotImplementedError):
        demo.main(base + [f"output_path={tmp_path / 'refused'}"])
    assert not os.path.exists(tmp_path / 'refused' / 'big_nearest' / 'input_pc.ply')
    out = demo.main(base + [f"output_path={tmp_path / 'out'}", "subsample=fps", "subsample_colors=mean"])[0]
    for f in ("input_pc.ply", "models/model_normalized.obj", "models/model_normalized.mtl", "models/model_normalized.png",
              "others/atlas_wo_background.png", "others/0_sparse.png"):
        assert os.path.exists(os.path.join(out, f)), f
    xyz, rgb = io_utils.read_ply_xyzrgb(os.path.join(out, "input_pc.ply"))
    assert len(xyz) == 30000 and len(rgb) == 30000
    xyz = np.asarray(xyz, np.float64)
    assert np.abs(xyz).max() <= 0.5 + 1e-6 and np.abs(np.linalg.norm(xyz, axis=1) - 0.5).max() < 0.01      # normalised by the FULL cloud's box
    import PIL.Image
    atlas = np.array(PIL.Image.open(os.path.join(out, "models/model_normalized.png")))
    assert atlas.shape == (256, 256, 3) and atlas.std() > 5
    out2 = demo.main(base + [f"output_path={tmp_path / 'small'}", "subsample=fps", "subsample_num=5000"])[0]
    assert len(io_utils.read_ply_xyzrgb(os.path.join(out2, "input_pc.ply"))[0]) == 5000


def test_demo_reconstructs_from_the_full_cloud_and_textures_from_the_subsample(tmp_path, monkeypatch):
    """geo_from=SPR with `subsample`: the reconstruction gets all 40 000 normalised points, input_pc.ply and the texturing path the subsample."""
    from pointdreamer_amd import demo, io_utils, spr, synthetic
    xyz, rgb, _ = synthetic.solid('torus').sample(40000, seed=2)
    pc = str(tmp_path / 'torus.ply')
    io_utils.save_colored_pc_ply(xyz * 1.3 - 0.2, rgb, pc)
    seen = []
    orig = spr.recon_one_shape_SPR

    def spy(coords, colors, *a, **k):
        seen.append((tuple(coords.shape), tuple(colors.shape), float(coords.abs().max())))
        return orig(coords, colors, *a, **k)
    monkeypatch.setattr(spr, 'recon_one_shape_SPR', spy)
    out = demo.main(["--config", os.path.join(ROOT, "configs", "nearest.yaml"), "--pc_file", pc, "--set", f"output_path={tmp_path / 'out'}",
                     "geo_from=SPR", "spr_depth=6", "xatlas_texture_res=256", "point_validation_by_o3d=False", "subsample=fps",
                     "subsample_num=8000"])[0]
    assert seen == [((40000, 3), (40000, 3), seen[0][2])] and seen[0][2] <= 0.5 + 1e-6
    assert len(io_utils.read_ply_xyzrgb(os.path.join(out, "input_pc.ply"))[0]) == 8000
    assert os.path.exists(os.path.join(out, 'geo', f'{os.path.basename(out)}_untextured', 'models', 'model_normalized.obj'))
    mv, _ = io_utils.load_obj_mesh(os.path.join(out, 'models', 'model_normalized.obj'))
    assert len(mv) != 49 * 100 + 2 and os.path.exists(os.path.join(out, "models/model_normalized.png"))
