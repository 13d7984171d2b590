"""GPU parity tests (rows P1-P6, I0, N1-N3, Uq1-Uq5): HIP path through the C ABI vs the oracle on the
same seeded inputs, vs the golden vectors made by the imported reference, and size-independent
properties at BASELINE sizes.  Integer / index / mask outputs must be bit-identical; colour outputs are
exact copies of inputs, so they are compared bit-exactly too."""
import os
import numpy as np
import pytest
import torch

from conftest import load_golden
from oracle import camera as ocam, project as oproj, sparse as osparse, inpaint as oinp, nbf as onbf
from oracle import unproject as ounp

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pd():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import pointdreamer_amd.ours_utils as ou
    import pointdreamer_amd.unproject as up
    import pointdreamer_amd.camera_utils as cu
    from pointdreamer_amd import synthetic, _lib
    _lib.lib()                                    # fails loudly if libpdhip.so is missing
    return dict(ou=ou, up=up, cu=cu, syn=synthetic, lib=_lib)


DEV = 'cuda:0'


def T(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return t if dtype is None else t.to(dtype)


def N_(t):
    return t.detach().cpu().numpy()


def make_cams(pd, params, res):
    return [pd['cu'].Camera(p, res, DEV) for p in params]


def test_camera_params_match_oracle(pd):
    cams, base_dirs, eyes, ups = pd['cu'].create_cameras(8, 1.6, 512, device=DEV)
    ocams, obd, oeyes, oups = ocam.create_cameras(8, 1.6, 512)
    for c, o in zip(cams, ocams):
        assert np.array_equal(N_(c.params), o.params)
    assert np.array_equal(N_(base_dirs), obd)
    pts = np.random.default_rng(0).uniform(-0.5, 0.5, (1000, 3)).astype(np.float32)
    for c, o in zip(cams, ocams):
        assert np.array_equal(N_(c.transform(T(pts))), o.transform(pts))


@pytest.mark.parametrize("n_points,stacks,slices,V,R", [(2000, 12, 24, 3, 128), (2000, 9, 14, 2, 100), (30000, 50, 100, 8, 512)])
def test_p1_p2_project_and_raster_vs_oracle(pd, n_points, stacks, slices, V, R):
    syn = pd['syn']
    verts, faces, _ = syn.uv_sphere(stacks, slices)
    xyz, rgb = syn.sphere_points(n_points, seed=5)
    ocams, _, _, _ = ocam.create_cameras(V, 1.6, R)
    cams = make_cams(pd, [c.params for c in ocams], R)
    hard, fidx, depth, vuv, uvc, uvs, pad, puv, pdep = pd['ou'].get_rendered_hard_mask_and_face_idx_batch(
        cams, T(verts), T(faces), T(xyz), None, True, 0.05)
    o = oproj.project_batch(ocams, verts, xyz, True, 0.05)
    assert np.array_equal(N_(uvc), o['uv_centers'])
    assert np.array_equal(N_(uvs), o['uv_scales'])
    assert np.array_equal(N_(vuv), o['vertice_uvs'])
    assert np.array_equal(N_(puv), o['point_uvs'])
    assert np.array_equal(N_(pdep), o['point_depths'])
    oh, of, od = oproj.rasterize(o['pos'], faces, R)
    assert np.array_equal(N_(hard), oh)
    assert np.array_equal(N_(fidx), of)
    assert np.array_equal(N_(depth), od)
    # properties
    assert hard.any() and (~hard).any()
    assert np.array_equal(N_(hard), N_(fidx) >= 0)
    # the global-atomic fallback (meshes above 65 536 faces) draws the same images as the LDS-tiled path
    from pointdreamer_amd import _lib
    L = _lib.lib()
    old = L.pdhip_debug_set_raster_path(1)
    try:
        h2, f2, d2 = pd['ou'].get_rendered_hard_mask_and_face_idx_batch(cams, T(verts), T(faces), T(xyz), None, True, 0.05)[:3]
    finally:
        L.pdhip_debug_set_raster_path(old)
    assert np.array_equal(N_(h2), oh) and np.array_equal(N_(f2), of) and np.array_equal(N_(d2), od)
    assert (N_(depth)[~N_(hard)] == 0).all()
    # non-rescale branch
    out2 = pd['ou'].get_rendered_hard_mask_and_face_idx_batch(cams, T(verts), T(faces), T(xyz), None, False, 0.05)
    o2 = oproj.project_batch(ocams, verts, xyz, False, 0.05)
    assert np.array_equal(N_(out2[7]), o2['point_uvs'])
    assert out2[4] == 0 and out2[5] == 2 and out2[6] == 0


def test_p3_fused_visibility_and_pixels_equal_the_two_entries(pd):
    """pdhip_point_visibility_pixels = pdhip_point_visibility (its verdicts) + pdhip_point_pixels, bit for bit, incl. out-of-range uvs."""
    rng = np.random.default_rng(4)
    V, N, R, res = 3, 5003, 128, 64
    uvs = rng.uniform(-0.2, 1.2, (V, N, 2)).astype(np.float32)
    uvs[0, :5] = [[0, 0], [1, 1], [np.nan, 0.5], [np.inf, -np.inf], [0.999999, 1e-8]]
    dep = rng.uniform(-1, 1, (V, N)).astype(np.float32)
    mesh = rng.uniform(-1, 1, (V, R, R)).astype(np.float32)
    ou = pd['ou']
    v1, _ = ou.get_point_validation_by_depth(R, T(uvs), T(dep), T(mesh), offset=0.0001)
    p1 = ou.get_point_pixels(T(uvs), res)
    v2, p2 = ou.get_point_validation_and_pixels(R, T(uvs), T(dep), T(mesh), res, offset=0.0001)
    assert torch.equal(v1, v2) and torch.equal(p1, p2)


def hostile_triangles():
    rng = np.random.default_rng(11)
    c = rng.uniform(-1.1, 1.1, (100, 1, 2))
    small = (c + rng.uniform(-0.15, 0.15, (100, 3, 2))).reshape(300, 2)                  # 100 small triangles, some across the border
    mid = rng.uniform(-400, 400, (9, 2)); mid[::3] = rng.uniform(-1, 1, (3, 2))          # 3 long slivers reaching far outside
    huge = rng.uniform(-3e4, 3e4, (6, 2))                                                # 2 triangles with vertices beyond the fixed-point clamp
    far = np.array([[300.0, 0.1], [301.0, 0.3], [300.5, 0.9], [-300.0, 0.1], [-301.0, 0.3], [-300.5, 0.9],
                    [0.1, 500.0], [0.3, 501.0], [0.9, 500.5], [0.1, -500.0], [0.3, -501.0], [0.9, -500.5],
                    [1000.0, 0.1], [1001.0, 0.3], [1000.5, 0.9], [-1000.0, 0.1], [-1001.0, 0.3], [-1000.5, 0.9],
                    [0.1, 1400.0], [0.3, 1401.0], [0.9, 1400.5], [0.1, -1400.0], [0.3, -1401.0], [0.9, -1400.5]])   # wholly off-screen, each side (the last four beyond +-32767 pixels)
    xy = np.concatenate([small, mid, huge, far]).astype(np.float32)
    n = xy.shape[0]
    z = rng.uniform(-1.3, 1.3, n).astype(np.float32)                                     # part of the depths outside [-1, 1]
    pos = np.stack([xy[:, 0], xy[:, 1], z, np.ones(n, np.float32)], 1)[None].repeat(2, 0).copy()
    pos[1, :, :2] = pos[1, :, 1::-1] * np.float32(0.7)                                   # a second, different view
    pos[1, 5, 0] = np.nan; pos[1, 7, 1] = np.inf
    faces = np.arange(n).reshape(-1, 3)
    extra = np.array([[0, 0, 1], [3, 4, 4], [6, 6, 6], [0, 1, 2], [2, 1, 0], [9, 10, 12], [9, 12, 13], [0, 4, 8], [0, 8, 12]])  # zero-area, duplicates, shared edges
    return pos, np.concatenate([faces, extra]).astype(np.int64)


def test_p2_raster_offscreen_huge_and_degenerate_faces_vs_oracle(pd):
    """P2 on hostile triangles: wholly outside the screen on every side (bounding boxes beyond the 16-bit pixel range), vertices beyond
    the fixed-point clamp, slivers straddling the border, zero-area faces, duplicated faces in both windings, shared edges (fill
    rule), depths outside [-1, 1], non-finite vertices.  Both paths (LDS tiles, global atomics) against the oracle, bit for bit."""
    from pointdreamer_amd import extract_texture_map as etm, _lib
    R = 96
    pos, faces = hostile_triangles()
    oh, of, od = oproj.rasterize(pos, faces, R)
    assert oh.any() and (~oh).any() and len(np.unique(of)) > 40
    L = _lib.lib()
    for path in (0, 1):
        old = L.pdhip_debug_set_raster_path(path)
        try:
            fidx, _, depth, hard = etm.rasterize(T(pos), T(faces), R)
        finally:
            L.pdhip_debug_set_raster_path(old)
        assert np.array_equal(N_(hard), oh), path
        assert np.array_equal(N_(fidx), of), path
        assert np.array_equal(N_(depth), od), path


@pytest.mark.parametrize("name", ["proj_sparse_dense.npz", "proj_sparse_rescale.npz", "proj_sparse_ps2.npz",
                                  "proj_sparse_scale_near1.npz"])
def test_p1_to_p6_vs_reference_golden(pd, name):
    g = load_golden(name)
    R, r = int(g['cam_res']), int(g['res'])
    cams = make_cams(pd, g['cam_params'], R)
    V = len(cams)
    hard, fidx, depth, vuv, uvc, uvs, pad, puv, pdep = pd['ou'].get_rendered_hard_mask_and_face_idx_batch(
        cams, T(g['vertices']), T(g['faces']), T(g['points']), None, True, 0.05)
    assert np.array_equal(N_(puv), g['point_uvs']) and np.array_equal(N_(pdep), g['point_depths'])
    assert np.array_equal(N_(depth), g['mesh_depths']) and np.array_equal(N_(fidx), g['face_idxs'])
    hard_r = pd['ou'].resize_masks(hard, r)
    assert np.array_equal(N_(hard_r), g['hard_masks_r'])
    vis, pix = pd['ou'].get_point_validation_by_depth(R, puv, pdep, depth, offset=0.0001)
    assert np.array_equal(N_(vis), g['ref_visibility'])             # reference output
    assert np.array_equal(N_(pix), g['ref_point_pixels_R'])         # reference output
    pp = pd['ou'].get_point_pixels(puv, r)
    assert np.array_equal(N_(pp), g['point_pixels_r'])
    sparse, m0, m2, sf = pd['ou'].get_sparse_images(pp, T(g['colors']), vis, hard_r, None, V, r, int(g['point_size']),
                                                    int(g['edge_point_size']), 0.82)
    assert np.array_equal(N_(m0), g['ref_mask0'])                   # reference outputs, bit-identical
    assert np.array_equal(N_(m2), g['ref_mask2'])
    assert np.array_equal(N_(sf), g['ref_scale_factors'])
    assert np.array_equal(N_(sparse), g['ref_sparse'])


def test_p4_degenerate_and_ragged_views(pd):
    g = load_golden("proj_sparse_dense.npz")
    r = int(g['res'])
    V = g['point_pixels_r'].shape[0]
    vis = g['ref_visibility'].copy()
    vis[0] = False                                                   # view 0: no valid point
    hard = g['hard_masks_r'].copy()
    hard[1] = False                                                  # view 1: empty foreground
    sparse, m0, m2, sf = pd['ou'].get_sparse_images(T(g['point_pixels_r']), T(g['colors']), T(vis), T(hard), None, V, r, 1, 1, 0.82)
    os_, om0, om2, osf = osparse.get_sparse_images(g['point_pixels_r'], g['colors'], vis, hard, V, r, 1, 1, 0.82)
    assert np.array_equal(N_(sparse), os_) and np.array_equal(N_(m0), om0) and np.array_equal(N_(m2), om2)
    assert np.array_equal(N_(sf), osf)
    assert not N_(sparse)[0].any() and not N_(sparse)[1].any()
    # empty point cloud
    e = pd['ou'].get_sparse_images(torch.zeros((V, 0, 2), dtype=torch.int64, device=DEV), torch.zeros((0, 3), device=DEV),
                                   torch.zeros((V, 0), dtype=torch.bool, device=DEV), T(hard), None, V, r, 1, 1, 0.82)
    assert not N_(e[0]).any()


@pytest.mark.parametrize("name", ["nearest_dense.npz", "nearest_rescale.npz"])
def test_i0_nearest_vs_oracle_and_reference(pd, name):
    g = load_golden(name)
    out = pd['ou'].get_inpainted_images(T(g['sparse']), None, T(g['mask2']), None, None, g['sparse'].shape[0], method='nearest')
    out = N_(out)
    for v in range(out.shape[0]):
        o = oinp.nearest_inpaint(g['sparse'][v], g['mask2'][v])
        assert np.array_equal(out[v], o)                            # bit-identical to the oracle (same tie rule)
        sites = g['mask2'][v][0].astype(bool)
        sr, sc = np.nonzero(sites)
        H, W = sites.shape
        qi, qj = np.meshgrid(np.arange(H), np.arange(W), indexing='ij')
        d2 = (qi.reshape(-1, 1) - sr[None]) ** 2 + (qj.reshape(-1, 1) - sc[None]) ** 2
        unique = ((d2 == d2.min(1, keepdims=True)).sum(1) == 1).reshape(H, W)
        assert np.array_equal(out[v][:, unique], g['ref_inpainted'][v].astype(np.float32)[:, unique])   # reference
    single = pd['ou'].naive_inpainting(T(g['sparse'][0]), T(g['mask2'][0]), method='nearest')
    assert np.array_equal(N_(single), out[0])


@pytest.mark.parametrize("H,W", [(37, 70), (16, 64), (17, 65), (130, 33), (5, 3)])
def test_i0_nearest_ragged_sizes_vs_oracle(pd, H, W):
    """Nearest fill at sizes that are not multiples of the 16-row segment / the 64-column wavefront: sparse sites, empty columns
    and rows, one image with a single site; uint8 and float masks, CHW and HWC layouts -- bit-identical to the oracle."""
    rng = np.random.default_rng(H * 131 + W)
    B = 3
    img = rng.uniform(0, 1, (B, 3, H, W)).astype(np.float32)
    sites = rng.uniform(0, 1, (B, H, W)) > 0.93
    sites[0, :, : W // 2] = False                                   # empty left half
    sites[0, H // 2, W - 1] = True
    sites[1] = False
    sites[1, H - 1, 0] = True                                        # a single site in a corner
    sites[2, : H // 3] = False                                       # empty top rows
    sites[2, H - 1, W // 2] = True
    want = np.stack([img[b][:, rr, cc] for b in range(B) for rr, cc in [oinp.nearest_site_index(sites[b])]])
    got = pd['ou'].nearest_fill(T(img), T(sites), 'CHW')
    assert np.array_equal(N_(got), want)
    got = pd['ou'].nearest_fill(T(img), T(sites.astype(np.float32)), 'CHW')
    assert np.array_equal(N_(got), want)
    got = pd['ou'].nearest_fill(T(np.ascontiguousarray(img.transpose(0, 2, 3, 1))), T(sites), 'HWC')
    assert np.array_equal(N_(got), want.transpose(0, 2, 3, 1))


def test_i0_nearest_full_size_properties(pd):
    rng = np.random.default_rng(7)
    B, H = 8, 256
    img = rng.uniform(0, 1, (B, 3, H, H)).astype(np.float32)
    sites = rng.uniform(0, 1, (B, H, H)) > 0.7
    sites[3] = False
    sites[3, 100, 17] = True                                         # a single site
    sites[4, :, :128] = False                                        # half the image empty
    out = N_(pd['ou'].nearest_fill(T(img), T(sites), 'CHW'))
    for b in range(B):
        rr, cc = oinp.nearest_site_index(sites[b])
        assert np.array_equal(out[b], img[b][:, rr, cc])
    assert (out[3] == img[3][:, 100:101, 17:18]).all()
    again = N_(pd['ou'].nearest_fill(T(out), T(sites), 'CHW'))       # idempotence
    assert np.array_equal(again, out)


def test_n1_n3_nbf_vs_oracle_and_reference(pd):
    g = load_golden("unproject_k21.npz")
    rng = np.random.default_rng(11)
    A, V = 256, 4
    mask = g['mask'][0, :, :, 0]
    vis = (rng.uniform(0, 1, (V, A, A)) > 0.4) & mask[None]
    vis[1, 60:200, 40:220] = mask[60:200, 40:220]
    for ks in ([21], [21, 11, 7], [3], [0], [1]):
        out = N_(pd['up'].shrink_visibility(T(mask), T(vis), ks))
        o = onbf.shrink_visibility(mask, vis.transpose(1, 2, 0), ks)
        assert out.shape == o.shape and np.array_equal(out, o)
        assert not (out & ~vis[None]).any()                          # shrunk is a subset of visible
    # reference layout entry point
    out = pd['up'].get_shrinked_per_view_per_pixel_visibility_torch(T(mask), T(vis.transpose(1, 2, 0)), [21])
    assert np.array_equal(N_(out), onbf.shrink_visibility(mask, vis.transpose(1, 2, 0), [21]))


@pytest.mark.parametrize("name", ["unproject_k21.npz", "unproject_k21_complete.npz", "unproject_k0.npz", "unproject_multi.npz"])
def test_uq_unproject_vs_reference_golden_and_oracle(pd, name):
    g = load_golden(name)
    R, r = int(g['cam_res']), int(g['res'])
    cams = make_cams(pd, g['cam_params'], R)
    ks = [int(k) for k in g['kernels']]
    atlas, shr, vids, coords, points, painted = pd['up'].unproject(
        T(g['inpainted']), None, T(g['f_normals']), r, cams, R, T(g['base_dirs']), T(g['gb_pos']), T(g['mask']),
        T(g['face_id']), T(g['uv_centers']), T(g['uv_scales']), float(g['padding']), T(g['scale_factors']),
        T(g['mesh_depths']), ks, None, bool(g['complete']))
    assert np.array_equal(N_(coords), g['ref_coords'])               # reference outputs
    assert np.array_equal(N_(points), g['ref_points'])
    assert np.array_equal(N_(shr), g['ref_shrinked'])
    ocams = [ocam.Camera(p, R) for p in g['cam_params']]
    o = ounp.unproject(g['inpainted'], g['f_normals'], r, ocams, R, g['base_dirs'], g['gb_pos'], g['mask'], g['face_id'],
                       g['uv_centers'], g['uv_scales'], float(g['padding']), g['scale_factors'], g['mesh_depths'], ks,
                       bool(g['complete']))
    assert np.array_equal(N_(vids), o['point_view_ids'])             # bit-identical to the oracle
    assert np.array_equal(N_(atlas), o['atlas_img'])
    assert np.array_equal(N_(painted), o['atlas_painted_mask'])
    diff = N_(vids) != g['ref_view_ids']                             # vs the reference: only sgemm-order near-ties may differ
    if diff.any():
        sim = np.sort(o['sim'][diff], 1)
        assert (sim[:, -1] - sim[:, -2] < 1e-6).all() and diff.mean() < 1e-3
    else:
        assert np.array_equal(N_(atlas), g['ref_atlas'])
        assert np.array_equal(N_(painted), g['ref_painted'])
    dil = pd['up'].dilate_atlas(atlas, T(g['mask']))
    assert np.array_equal(N_(dil), oinp.dilate_atlas(N_(atlas), g['mask']))
    m = g['mask'][0, :, :, 0]
    assert np.array_equal(N_(dil)[m], N_(atlas)[m])


def test_full_size_shape_properties(pd):
    """BASELINE sizes: 30k points, 8 views, cam_res 512, res 256, atlas 1024."""
    syn = pd['syn']
    sh = syn.make_shape(30000, 1024)
    cams, base_dirs, eyes, ups = pd['cu'].create_cameras(8, 1.6, 512, device=DEV)
    ou, up = pd['ou'], pd['up']
    hard, fidx, depth, vuv, uvc, uvs, pad, puv, pdep = ou.get_rendered_hard_mask_and_face_idx_batch(
        cams, T(sh['vertices']), T(sh['faces']), T(sh['points']), None, True, 0.05)
    hard_r = ou.resize_masks(hard, 256)
    # 2x2 OR-pool identity at R = 2r
    assert np.array_equal(N_(hard_r), N_(hard).reshape(8, 256, 2, 256, 2).any((2, 4)))
    vis0, _ = ou.get_point_validation_by_depth(512, puv, pdep, depth, offset=0.0001)
    vis1, _ = ou.get_point_validation_by_depth(512, puv, pdep, depth, offset=0.01)
    assert not (N_(vis0) & ~N_(vis1)).any()                          # monotone in the offset
    frac = N_(vis0).mean()
    assert 0.3 < frac < 0.7                                          # about half of a sphere faces each camera
    pp = ou.get_point_pixels(puv, 256)
    sparse, m0, m2, sf = ou.get_sparse_images(pp, T(sh['colors']), vis0, hard_r, None, 8, 256, 1, 1, 0.82)
    s, a, b = N_(sparse), N_(m0), N_(m2)
    assert set(np.unique(a)) <= {0.0, 1.0} and set(np.unique(b)) <= {0.0, 1.0}
    assert (b[a == 0] == 1).all()                                    # background is always a "keep" pixel
    assert (s[a == 0] == 0).all()
    assert np.array_equal(a[:, :, ::-1], np.repeat(N_(hard_r)[:, None].astype(np.float32), 3, 1)) or (N_(sf) < 1).any()
    inp = ou.get_inpainted_images(sparse, m0, m2, None, None, 8, method='nearest')
    keep = b[:, 0] == 1
    assert np.array_equal(N_(inp).transpose(0, 2, 3, 1)[keep], s.transpose(0, 2, 3, 1)[keep])
    atlas, shr, view_ids, painted, vis = up.unproject_dense(
        inp, T(sh['f_normals']), 256, cams, 512, base_dirs, T(sh['gb_pos']), T(sh['mask']),
        T(sh['per_atlas_pixel_face_id']), uvc, uvs, pad, sf, depth, [21], True)
    m = sh['mask'][0, :, :, 0]
    assert not (N_(vis) & ~m[None]).any() and not (N_(shr) & ~N_(vis)).any()
    assert (N_(view_ids)[~m] == -1).all() and (N_(view_ids)[m] >= 0).all()
    assert np.array_equal(N_(painted), m)
    # every painted texel holds a colour that exists in the chosen view's image
    vid = N_(view_ids)
    assert len(np.unique(vid[m])) == 8
    dil = up.dilate_atlas(atlas, T(sh['mask']))
    assert np.array_equal(N_(dil)[m], N_(atlas)[m])
    # oracle cross-check at full size for the cheap-to-restate stages
    ocams = [ocam.Camera(N_(c.params), 512) for c in cams]
    ovis = oproj.point_validation_by_depth(512, N_(puv), N_(pdep), N_(depth), 0.0001)[0]
    assert np.array_equal(N_(vis0), ovis)
    osp = osparse.get_sparse_images(N_(pp), sh['colors'], ovis, N_(hard_r), 8, 256, 1, 1, 0.82)
    assert np.array_equal(s, osp[0]) and np.array_equal(b, osp[2])
    o = ounp.unproject(N_(inp), sh['f_normals'], 256, ocams, 512, N_(base_dirs), sh['gb_pos'], sh['mask'],
                       sh['per_atlas_pixel_face_id'], N_(uvc), N_(uvs), pad, N_(sf), N_(depth), [21], True)
    assert np.array_equal(N_(shr), o['shrinked'])
    assert np.array_equal(vid[m], o['point_view_ids'])
    assert np.array_equal(N_(atlas), o['atlas_img'])


@pytest.mark.parametrize("n,shape", [(3000, 'sphere'), (30000, 'sphere'), (4000, 'blob'), (30000, 'noisy')])
def test_p3b_hidden_point_removal_vs_qhull(pd, n, shape):
    """Device HPR (per-point certified GJK hull-vertex test + double-double fallback) vs the oracle (same spherical flip +
    qhull through scipy; open3d itself is absent -- parity unpinned).  Row P3b is an index row: the verdicts must be
    IDENTICAL.  The only admissible exception is a point inside qhull's own merge tolerance of a hull facet (the device
    answers for the exact hull): each such point must have |signed distance to the hull of the other points| < 1e-9
    (radius 100 => coordinates ~ 200, qhull's roundoff ~ 1e-13), and no query may be left uncertified."""
    from pointdreamer_amd import hpr
    rng = np.random.default_rng(n)
    if shape == 'sphere':
        pts, _ = pd['syn'].sphere_points(n, seed=n)
    elif shape == 'noisy':                                 # a rough surface: many points just above / below the hull facets
        pts, _ = pd['syn'].sphere_points(n, seed=n + 1)
        pts = (pts * (1.0 + 0.02 * rng.standard_normal((n, 1)))).astype(np.float32)
    else:                                                  # a solid blob: most points are interior, hence hidden
        pts = (rng.standard_normal((n, 3)) * 0.15).astype(np.float32)
    _, _, eyes, _ = pd['cu'].create_cameras(8, 1.6, 512, device=DEV)
    got, st = hpr.hidden_point_removal(T(pts), eyes, 100, return_stats=True)
    got = N_(got)
    want = oproj.point_validation_by_hpr(pts, eyes, 100)
    assert got.shape == want.shape == (8, n)
    assert st['unresolved'] == 0, st
    assert st['exact_fallback'] <= 0.01 * 8 * n, st       # the f64 certificates decide all but a handful
    bad = np.argwhere(got != want)
    for v, i in bad[:50]:
        m = oproj.hpr_margin(oproj.hpr_flip(pts, eyes[v], 100), i)
        assert abs(m) < 1e-9, (v, i, m, bool(got[v, i]), bool(want[v, i]))
        assert bool(got[v, i]) == (m > 0), (v, i, m)      # the device verdict is the exact one
    assert len(bad) <= 2, (len(bad), st)
    frac = want.mean()
    assert 0.05 < frac < 0.8
    if shape == 'sphere':
        # sanity: points facing the eye are kept, points on the far side are removed
        for v in range(8):
            facing = (pts @ eyes[v]) / (np.linalg.norm(pts, axis=1) * np.linalg.norm(eyes[v]))
            assert got[v][facing > 0.6].mean() > 0.98 and got[v][facing < -0.3].mean() < 0.02
    # through the reference-signature entry point
    got2 = pd['ou'].get_point_validation_by_o3d(T(pts), eyes, 100)
    assert np.array_equal(N_(got2), got)


def test_p3b_large_support_set(pd):
    """100k points on a sphere, no skip mask: the level-2 support set (the points outside the coarse hull) spans more than 256
    chunks, so the box-culled scans walk several chunk groups, and every point is a query of the working-set kernel."""
    from pointdreamer_amd import hpr
    n = 100000
    pts, _ = pd['syn'].sphere_points(n, seed=11)
    _, _, eyes, _ = pd['cu'].create_cameras(8, 1.6, 512, device=DEV)
    eyes = eyes[:2]
    got, st = hpr.hidden_point_removal(T(pts), eyes, 100, return_stats=True)
    got = N_(got)
    want = oproj.point_validation_by_hpr(pts, eyes, 100)
    assert st['unresolved'] == 0, st
    bad = np.argwhere(got != want)
    for v, i in bad[:20]:
        m = oproj.hpr_margin(oproj.hpr_flip(pts, eyes[v], 100), i)
        assert abs(m) < 1e-9 and bool(got[v, i]) == (m > 0), (v, i, m)
    assert len(bad) <= 2, (len(bad), st)
    assert (want.sum(1) > 16384).all()                       # more hull vertices per view than 256 chunks hold


@pytest.mark.parametrize("kind", ['cube', 'gauss', 'plane', 'cylinder', 'clusters', 'shell_grid', 'two_level_plane'])
def test_p3b_cloud_zoo_vs_qhull(pd, kind):
    """Clouds of different character through all three levels: box (flat faces: many coplanar flipped neighbours), Gaussian blob,
    a thin noisy plate and an exactly planar grid (the flip of a plane is a sphere through the eye: every point is a hull vertex,
    neighbours nearly cospherical), a cylinder, tight clusters, a latitude / longitude grid on a sphere (exact symmetries)."""
    from pointdreamer_amd import hpr
    rng = np.random.default_rng(abs(hash(kind)) % (2 ** 31))
    n = 6000
    if kind == 'cube':
        pts = rng.uniform(-0.5, 0.5, (n, 3)); ax = rng.integers(0, 3, n); pts[np.arange(n), ax] = np.sign(pts[np.arange(n), ax]) * 0.5
    elif kind == 'gauss':
        pts = rng.standard_normal((n, 3)) * 0.2
    elif kind == 'plane':
        pts = np.concatenate([rng.uniform(-0.6, 0.6, (n, 2)), 0.15 + 0.002 * rng.standard_normal((n, 1))], 1)
    elif kind == 'cylinder':
        th = rng.uniform(0, 2 * np.pi, n); pts = np.stack([0.4 * np.cos(th), 0.4 * np.sin(th), rng.uniform(-0.6, 0.6, n)], 1)
    elif kind == 'clusters':
        c = rng.uniform(-0.5, 0.5, (12, 3)); pts = c[rng.integers(0, 12, n)] + 0.01 * rng.standard_normal((n, 3))
    elif kind == 'shell_grid':
        a, b = np.meshgrid(np.linspace(0.05, np.pi - 0.05, 60), np.linspace(0, 2 * np.pi, 100, endpoint=False), indexing='ij')
        pts = 0.5 * np.stack([np.sin(a) * np.cos(b), np.sin(a) * np.sin(b), np.cos(a)], -1).reshape(-1, 3)
    else:                                                  # exactly planar grid, above the two-level threshold
        a, b = np.meshgrid(np.linspace(-0.6, 0.6, 80), np.linspace(-0.6, 0.6, 80), indexing='ij')
        pts = np.stack([a, b, 0.2 + 0.3 * a - 0.1 * b], -1).reshape(-1, 3)
    pts = pts.astype(np.float32)
    _, _, eyes, _ = pd['cu'].create_cameras(8, 1.6, 512, device=DEV)
    eyes = eyes[::2]
    got, st = hpr.hidden_point_removal(T(pts), eyes, 100, return_stats=True)
    got = N_(got)
    want = oproj.point_validation_by_hpr(pts, eyes, 100)
    bad = np.argwhere(got != want)
    for v, i in bad[:50]:                                  # only inside qhull's own merge tolerance, and then the device has the exact verdict
        m = oproj.hpr_margin(oproj.hpr_flip(pts, eyes[v], 100), i)
        assert abs(m) < 1e-9, (kind, v, i, m, bool(got[v, i]), bool(want[v, i]))
        assert bool(got[v, i]) == (m > 0) or st['unresolved'] > 0, (kind, v, i, m)
    assert len(bad) <= max(2, st['unresolved']), (kind, len(bad), st)


def test_p3b_eye_inside_the_cloud(pd):
    """Eyes inside the cloud's bounding box (the direction grid of level 0 has no face to project on: that level switches itself
    off) and just outside a dense blob."""
    from pointdreamer_amd import hpr
    rng = np.random.default_rng(21)
    pts = rng.standard_normal((6000, 3)); pts = (0.5 * pts / np.linalg.norm(pts, axis=1, keepdims=True) * rng.uniform(0.7, 1.0, (6000, 1))).astype(np.float32)
    eyes = np.array([[0.1, 0.05, 0.0], [0.0, 0.0, 0.3], [0.45, 0.45, 0.45], [0.0, 0.6, 0.0]], np.float64)
    got, st = hpr.hidden_point_removal(T(pts), eyes, 100, return_stats=True)
    got = N_(got)
    want = oproj.point_validation_by_hpr(pts, eyes, 100)
    bad = np.argwhere(got != want)
    for v, i in bad[:50]:
        m = oproj.hpr_margin(oproj.hpr_flip(pts, eyes[v], 100), i)
        assert abs(m) < 1e-9 and bool(got[v, i]) == (m > 0), (v, i, m)
    assert len(bad) <= 2 and st['unresolved'] == 0, (len(bad), st)


def test_p3b_duplicates_and_tiny_clouds(pd):
    """Coinciding points: the smallest index is the hull vertex, the copies are hidden (qhull keeps one of them, which one is
    its processing order); clouds below the two-level threshold and of a handful of points take the one-level path."""
    from pointdreamer_amd import hpr
    pts, _ = pd['syn'].sphere_points(2000, seed=5)
    pts = np.concatenate([pts, pts[:40]], 0)               # 40 exact duplicates appended
    _, _, eyes, _ = pd['cu'].create_cameras(4, 1.6, 512, device=DEV)
    got, st = hpr.hidden_point_removal(T(pts), eyes, 100, return_stats=True)
    got = N_(got)
    base = oproj.point_validation_by_hpr(pts[:2000], eyes, 100)
    assert st['unresolved'] == 0, st
    assert np.array_equal(got[:, :2000], base)
    assert not got[:, 2000:].any()
    for n in (1, 2, 3, 4, 5, 17):
        p = pts[:n]
        g = N_(hpr.hidden_point_removal(T(p), eyes, 100))
        if n >= 4:
            assert np.array_equal(g, oproj.point_validation_by_hpr(p, eyes, 100))
        else:                                              # fewer than 4 points: every point is extreme (qhull refuses such input)
            assert g.all()


def test_p3b_skip_mask_gives_the_or(pd):
    from pointdreamer_amd import hpr
    pts, _ = pd['syn'].sphere_points(5000, seed=77)
    _, _, eyes, _ = pd['cu'].create_cameras(4, 1.6, 512, device=DEV)
    full = hpr.hidden_point_removal(T(pts), eyes, 100)
    pre = torch.from_numpy(np.random.default_rng(1).uniform(0, 1, (4, 5000)) > 0.5).to(DEV)
    ored = hpr.hidden_point_removal(T(pts), eyes, 100, already_valid=pre)
    assert torch.equal(ored, torch.logical_or(full, pre))
    allv = hpr.hidden_point_removal(T(pts), eyes, 100, already_valid=torch.ones_like(pre))
    assert bool(allv.all())


def test_p3b_writes_every_verdict_into_a_dirty_buffer(pd):
    """The verdict array need not be cleared by the caller: the C entry on a buffer full of 0xAA gives the wrapper's result, with and
    without a skip mask, for a two-level (30 k points) and a one-level (3 k points) cloud."""
    import ctypes as C
    from pointdreamer_amd import hpr, _lib
    L = _lib.lib()
    _, _, eyes, _ = pd['cu'].create_cameras(4, 1.6, 512, device=DEV)
    eyes_d = torch.from_numpy(np.asarray(eyes, np.float64).reshape(-1, 3)).to(DEV).contiguous()
    for n in (30000, 3000):
        pts, _ = pd['syn'].sphere_points(n, seed=3)
        p = T(pts).float().contiguous()
        pre = torch.from_numpy(np.random.default_rng(2).uniform(0, 1, (4, n)) > 0.6).to(DEV)
        for skip in (None, pre):
            want = hpr.hidden_point_removal(p, eyes, 100, already_valid=skip)
            vis = torch.full((4, n), 0xAA, dtype=torch.uint8, device=DEV)
            ws = torch.full((L.pdhip_hpr_ws_bytes(4, n),), 0x55, dtype=torch.uint8, device=DEV)
            sk = None if skip is None else _lib.as_u8(skip.contiguous())
            rc = L.pdhip_hidden_point_removal(_lib.ptr(p), n, _lib.ptr(eyes_d), 4, 100.0, _lib.ptr(sk, allow_none=True), _lib.ptr(vis),
                                              _lib.ptr(ws), _lib.stream())
            assert rc == 0
            assert torch.equal(vis, _lib.as_u8(want)), (n, skip is not None, int((vis != _lib.as_u8(want)).sum()))


def test_uv_atlas_producer_vs_oracle(pd):
    """rasterise the UV triangles + interpolate world positions (extract_texture_map.py:48-64)."""
    from pointdreamer_amd import extract_texture_map as etm
    syn = pd['syn']
    verts, faces, _ = syn.uv_sphere(12, 24)
    rng = np.random.default_rng(3)
    # a toy parametrisation: every face gets its own little right triangle in a grid of UV cells (3 vt per face)
    F = faces.shape[0]
    g = int(np.ceil(np.sqrt(F)))
    cell = 1.0 / g
    fi = np.arange(F)
    ox, oy = (fi % g) * cell, (fi // g) * cell
    tri_uv = np.stack([np.stack([ox + 0.1 * cell, oy + 0.1 * cell], -1), np.stack([ox + 0.9 * cell, oy + 0.1 * cell], -1),
                       np.stack([ox + 0.1 * cell, oy + 0.9 * cell], -1)], 1)
    uvs = tri_uv.reshape(-1, 2).astype(np.float32)
    tex_idx = np.arange(F * 3).reshape(F, 3)
    R = 256
    _, _, gb_pos, mask, fid = etm.uvmap_w_face_id(T(verts), T(faces), T(uvs), T(tex_idx), R)
    pos = np.concatenate([uvs * 2 - 1, np.zeros((F * 3, 1), np.float32), np.ones((F * 3, 1), np.float32)], 1)[None]
    oh, of, od = oproj.rasterize(pos, tex_idx, R)
    assert np.array_equal(N_(fid), of) and np.array_equal(N_(mask)[..., 0], oh)
    ob = oproj.raster_barycentrics(pos, tex_idx, of, R)
    og = oproj.interpolate(verts, faces, of, ob)
    assert np.array_equal(N_(gb_pos), og)
    m = of[0] >= 0
    assert m.mean() > 0.15
    # interpolated positions lie on the (flat) faces: inside the unit-ish ball and close to the sphere
    r = np.linalg.norm(N_(gb_pos)[0][m], axis=1)
    assert r.max() <= 0.5 + 1e-5 and r.min() > 0.45
    # each covered texel belongs to the face whose UV triangle contains it
    ii, jj = np.nonzero(m)
    u, v = (jj + 0.5) / R, (ii + 0.5) / R
    assert np.array_equal(of[0][ii, jj], (np.floor(v / cell) * g + np.floor(u / cell)).astype(np.int64))


@pytest.mark.parametrize("use_shr,iters,A", [(True, 3, 64), (False, 3, 64), (True, 25, 64), (True, 3, 80), (False, 3, 48)])
def test_optimize_color_vs_oracle(pd, use_shr, iters, A):
    """texture coordinates bit-identical, optimised atlas within 1e-4 of the torch-autograd oracle
    (f64 atomics reorder sums; Adam amplifies nothing at lr 5e-2)."""
    from oracle import optimize as oopt
    from pointdreamer_amd import optimize as popt
    syn = pd['syn']
    verts, faces, _ = syn.uv_sphere(12, 24)
    # (A = 80 / 48: atlas widths that are not a multiple of the backward pass's 64-texel wave segments -- a wave then spans two rows)
    V, R, res, r = 3, 64, 96, 32
    ocams, _, _, _ = ocam.create_cameras(V, 1.6, R)
    cams = make_cams(pd, [c.params for c in ocams], R)
    pr = oproj.project_batch(ocams, verts, verts[:4], True, 0.05)
    rng = np.random.default_rng(5)
    F_ = faces.shape[0]
    g = int(np.ceil(np.sqrt(F_))); cell = 1.0 / g; fi = np.arange(F_)
    ox, oy = (fi % g) * cell, (fi // g) * cell
    uvs = np.stack([np.stack([ox + 0.05 * cell, oy + 0.05 * cell], -1), np.stack([ox + 0.95 * cell, oy + 0.05 * cell], -1),
                    np.stack([ox + 0.05 * cell, oy + 0.95 * cell], -1)], 1).reshape(-1, 2).astype(np.float32)
    tex = np.arange(F_ * 3).reshape(F_, 3)
    sf = np.array([1.0, 0.85, 1.0], np.float32)
    o_uv, o_mask = oopt.texture_coordinates(ocams, verts, faces, uvs, tex, pr['uv_centers'], pr['uv_scales'], 0.05, sf, res)
    uv_map, fidx = popt.texture_coordinates(cams, T(verts), T(faces), T(uvs), T(tex), T(pr['uv_centers']), T(pr['uv_scales']), 0.05,
                                            T(sf), res)
    assert np.array_equal(N_(uv_map)[:, ::-1], o_uv) and np.array_equal((N_(fidx) >= 0)[:, ::-1], o_mask)
    atlas0 = rng.uniform(0, 1, (3, A, A)).astype(np.float32)
    inp = rng.uniform(0, 1, (V, 3, r, r)).astype(np.float32)
    shr = (rng.uniform(0, 1, (V, A, A)) > 0.3) if use_shr else None
    oa, oim = oopt.optimize_color(atlas0, inp, o_uv, o_mask, shr, iterations=iters)
    a, im = popt.optimize_color(T(atlas0), T(inp), T(verts), T(faces), T(uvs), T(tex), cams, None, None, None, T(pr['uv_centers']),
                                T(pr['uv_scales']), 0.05, T(sf), None, None if shr is None else T(shr), iterations=iters, res=res)
    assert a.shape == (1, 3, A, A)
    moved = np.abs(oa.numpy()[0] - atlas0).max()
    assert moved > 0.05                                             # the optimisation actually changes the atlas
    da = np.abs(N_(a) - oa.numpy())
    if iters <= 3:
        assert da.max() <= 1e-4 and np.abs(N_(im) - oim.numpy()).max() <= 1e-4
    else:
        # an L1 loss under Adam is chaotic once texels start to converge (sign(d) flips on 1e-7 differences move a texel by
        # ~lr): require agreement on the bulk and the same achieved loss instead of element-wise equality
        assert (da <= 1e-3).mean() > 0.97, (da <= 1e-3).mean()
        assert np.isfinite(N_(im)).all() and N_(im).min() >= 0 and N_(im).max() <= 1
    untouched = np.abs(oa.numpy()[0] - atlas0).max(0) == 0          # texels no view samples stay exactly as they were
    assert untouched.any() and np.array_equal(N_(a)[0][:, untouched], atlas0[:, untouched])


@pytest.mark.parametrize("name", ["neighbor_small.npz", "neighbor_seam.npz"])
def test_8f2_neighbor_completion_vs_oracle_and_reference_golden(name):
    """complete_unseen_by='neighbor' through the C ABI: bit-exact against the oracle (same float32 op order, same tie rules),
    and against the imported reference's outputs (1e-6; nearest-fill ties excepted)."""
    from oracle import neighbor as onb
    from pointdreamer_amd import unproject as up
    g = load_golden(name)
    o = onb.paint_invisible_areas_by_neighbors(g['vertices'], g['faces'], g['uvs'], g['face_uv_idx'], g['to_inpaint_face_id'],
                                               g['atlas'], g['painted'], return_intermediates=True)
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    atlas = up.paint_invisible_areas_by_neighbors(T(g['vertices']), T(g['faces']), T(g['uvs']), T(g['face_uv_idx']),
                                                  g['to_inpaint_face_id'], T(g['atlas']), T(g['painted']), use_atlas=True)
    out = atlas.cpu().numpy()
    assert np.array_equal(out, o['atlas'])
    sv, sf, vc = up.paint_invisible_areas_by_neighbors(T(g['vertices']), T(g['faces']), T(g['uvs']), T(g['face_uv_idx']),
                                                       g['to_inpaint_face_id'], T(g['atlas']), T(g['painted']), use_atlas=False)
    assert np.array_equal(vc.cpu().numpy(), o['vert_colors'])
    assert np.array_equal(sf.cpu().numpy(), g['ref_sub_faces']) and np.array_equal(sv.cpu().numpy(), g['ref_sub_vertices'])
    assert np.abs(vc.cpu().numpy() - g['ref_vert_colors']).max() <= 1e-6
    m = g['ref_mask_before_fill'] > 0
    assert np.abs(out[m] - g['ref_atlas'][m]).max() <= 1e-6
    # unpainted-face marking (demo.py:180-181)
    A = g['painted'].shape[0]
    rng = np.random.default_rng(3)
    fid = rng.integers(-1, 50, (1, A, A)).astype(np.int64)
    painted = rng.uniform(0, 1, (A, A)) > 0.3
    ids = up.unpainted_face_ids(T(fid), T(painted), 50)
    ref = np.unique(fid[0][~painted]); ref = ref[ref > -1]
    assert np.array_equal(ids, ref)


def test_8f2_pipeline_neighbor_branch_vs_oracle(pd):
    """colorize_one_mesh(complete_unseen_by='neighbor') on a shape with a large never-seen area (3 views of a sphere): the
    pipeline's atlas equals unproject (no projection completion) -> oracle neighbour completion of the same tensors."""
    from oracle import neighbor as onb
    syn, ou, up = pd['syn'], pd['ou'], pd['up']
    from pointdreamer_amd import pipeline
    stacks, slices, A, V, R, r = 16, 32, 256, 3, 256, 128
    verts, faces, lut = syn.uv_sphere(stacks, slices)
    uvs, fuv = syn.uv_sphere_uvs(stacks, slices, A, gutter=2)
    gb_pos, mask, fid = syn.latlong_atlas(A, stacks, slices, gutter=2, lut=lut)
    xyz, rgb = syn.sphere_points(4000, seed=9)
    cams, base_dirs, eyes, ups = pd['cu'].create_cameras(V, 1.6, R, device=DEV)
    xat = dict(gb_pos=T(gb_pos), mask=T(mask), per_atlas_pixel_face_id=T(fid), uvs=T(uvs), mesh_tex_idx=T(fuv))
    cam_info = dict(cams=cams, base_dirs=base_dirs, eye_positions=eyes, up_dirs=ups)
    kw = dict(view_num=V, res=r, cam_res=R, point_validation_by_o3d=False, texture_gen_method='nearest', point_size=1,
              edge_point_size=1, crop_img=True, crop_padding=0.05, mask_ratio_thresh=0.82, optimize_from=None,
              edge_dilate_kernels=[21])
    fn = T(syn.face_normals(verts, faces))
    out = pipeline.colorize_one_mesh(T(xyz), T(rgb), T(verts), T(faces), fn, xat, cam_info, complete_unseen_by='neighbor',
                                     return_intermediates=True, **kw)
    painted = N_(out['painted'])
    m = mask[0, :, :, 0]
    assert (m & ~painted).mean() > 0.05                       # a real unseen area
    ref_run = pipeline.colorize_one_mesh(T(xyz), T(rgb), T(verts), T(faces), fn, xat, cam_info, complete_unseen_by='unproject',
                                         return_intermediates=True, **kw)
    # the pre-completion atlas: painted texels are the same in both runs; unpainted ones are zero before completion
    atlas0 = np.where(painted[..., None], N_(ref_run['atlas']), 0.0).astype(np.float32)
    tif = np.unique(fid[0][~painted]); tif = tif[tif > -1]
    o = onb.paint_invisible_areas_by_neighbors(verts, faces, uvs, fuv, tif, atlas0, painted)
    assert np.array_equal(N_(out['atlas']), o)
    assert np.array_equal(N_(out['atlas'])[painted], atlas0[painted])


def test_8f4_device_u8_conversion_and_native_png(tmp_path):
    """pdhip_chw_f32_to_hwc_u8 = (img * 255).clip(0, 255).astype(uint8) with CHW -> HWC; PNG written from a GPU tensor."""
    import PIL.Image
    from pointdreamer_amd import io_utils
    rng = np.random.default_rng(4)
    img = rng.uniform(-0.2, 1.2, (4, 65, 130)).astype(np.float32)
    img[0, 0, :4] = [0.999, 1.0, 0.0, 254.5 / 255]
    p = str(tmp_path / 'g.png')
    io_utils.save_CHW_RGBA_img(T(img), p)
    assert np.array_equal(np.array(PIL.Image.open(p)), (img.transpose(1, 2, 0) * 255).clip(0, 255).astype(np.uint8))


def test_batched_shapes_equal_one_by_one(pd):
    """colorize_meshes_batched (BASELINE configs[4]: several shapes per pass, views batched through the inpainter together) gives
    exactly the atlases of colorize_one_mesh shape by shape ('nearest' inpainting: deterministic)."""
    from pointdreamer_amd import pipeline
    syn = pd['syn']
    stacks, slices, A, V, R, r = 16, 32, 256, 4, 256, 128
    verts, faces, lut = syn.uv_sphere(stacks, slices)
    gb_pos, mask, fid = syn.latlong_atlas(A, stacks, slices, gutter=2, lut=lut)
    cams, base_dirs, eyes, ups = pd['cu'].create_cameras(V, 1.6, R, device=DEV)
    xat = dict(gb_pos=T(gb_pos), mask=T(mask), per_atlas_pixel_face_id=T(fid), uvs=None, mesh_tex_idx=None)
    cam_info = dict(cams=cams, base_dirs=base_dirs, eye_positions=eyes, up_dirs=ups)
    fn = T(syn.face_normals(verts, faces))
    kw = dict(view_num=V, res=r, cam_res=R, point_validation_by_o3d=True, texture_gen_method='nearest', point_size=1,
              edge_point_size=1, crop_img=True, crop_padding=0.05, mask_ratio_thresh=0.82, edge_dilate_kernels=[21])
    clouds = [syn.sphere_points(3000, seed=s) for s in (1, 2, 3)]
    shapes = [dict(coords=T(x), colors=T(c), vertices=T(verts), faces=T(faces), f_normals=fn, xatlas=xat) for x, c in clouds]
    got = pipeline.colorize_meshes_batched(shapes, cam_info, **kw)
    for (x, c), atlas in zip(clouds, got):
        one = pipeline.colorize_one_mesh(T(x), T(c), T(verts), T(faces), fn, xat, cam_info, complete_unseen_by='unproject',
                                         optimize_from=None, return_intermediates=True, **kw)
        assert np.array_equal(N_(atlas), N_(one['atlas']))


def test_batched_shapes_with_neighbor_completion_and_optimize_equal_one_by_one(pd, tmp_path):
    """The batched entry point runs the full option set (the shipped configs: complete_unseen_by='neighbor', optimize_from='ours')
    shape by shape behind the shared inpainter batch, and writes each shape's per-view PNGs into its own directory."""
    from pointdreamer_amd import pipeline
    syn = pd['syn']
    stacks, slices, A, V, R, r = 16, 32, 256, 4, 256, 128
    verts, faces, lut = syn.uv_sphere(stacks, slices)
    gb_pos, mask, fid = syn.latlong_atlas(A, stacks, slices, gutter=2, lut=lut)
    uvs, fuv = syn.uv_sphere_uvs(stacks, slices, A, gutter=2)
    cams, base_dirs, eyes, ups = pd['cu'].create_cameras(V, 1.6, R, device=DEV)
    xat = dict(gb_pos=T(gb_pos), mask=T(mask), per_atlas_pixel_face_id=T(fid), uvs=T(uvs), mesh_tex_idx=T(fuv))
    cam_info = dict(cams=cams, base_dirs=base_dirs, eye_positions=eyes, up_dirs=ups)
    fn = T(syn.face_normals(verts, faces))
    kw = dict(view_num=V, res=r, cam_res=R, point_validation_by_o3d=True, texture_gen_method='nearest', point_size=1,
              edge_point_size=1, crop_img=True, crop_padding=0.05, mask_ratio_thresh=0.82, edge_dilate_kernels=[21],
              complete_unseen_by='neighbor', optimize_from='ours')
    clouds = [syn.sphere_points(3000, seed=s) for s in (4, 5)]
    shapes = [dict(coords=T(x), colors=T(c), vertices=T(verts), faces=T(faces), f_normals=fn, xatlas=xat) for x, c in clouds]
    dirs = [str(tmp_path / f"s{i}") for i in range(2)]
    got = pipeline.colorize_meshes_batched(shapes, cam_info, save_img_paths=dirs, return_full=True, **kw)
    for (x, c), full, d in zip(clouds, got, dirs):
        one = pipeline.colorize_one_mesh(T(x), T(c), T(verts), T(faces), fn, xat, cam_info, **kw)
        assert len(full) == 6 and np.array_equal(N_(full[4]), N_(one[4]))
        for k in range(V):
            for sfx in ("sparse", "mask0", "mask2", "inpainted"):
                assert os.path.exists(os.path.join(d, f"{k}_{sfx}.png"))


def test_degenerate_sizes_do_not_break_the_entry_points(pd):
    """Empty and tiny inputs: no points, fewer points than a tetrahedron (every point is a hull vertex = visible), no faces."""
    from pointdreamer_amd import hpr
    cams, base_dirs, eyes, ups = pd['cu'].create_cameras(3, 1.6, 128, device=DEV)
    verts, faces, _ = pd['syn'].uv_sphere(8, 12)
    for n in (0, 1, 2, 3, 4):
        pts = np.random.default_rng(n).normal(size=(n, 3)).astype(np.float32) * 0.3
        vis = hpr.hidden_point_removal(T(pts).reshape(n, 3), eyes, 100)
        assert tuple(vis.shape) == (3, n) and bool(vis.all())
    out = pd['ou'].get_rendered_hard_mask_and_face_idx_batch(cams, T(verts), T(faces[:0].reshape(0, 3)), T(np.zeros((5, 3), np.float32)),
                                                            None, True, 0.05)
    assert int(out[0].sum()) == 0 and bool((out[1] == -1).all()) and bool((out[2] == 0).all())
    out = pd['ou'].get_rendered_hard_mask_and_face_idx_batch(cams, T(verts), T(faces), T(np.zeros((0, 3), np.float32)), None, True, 0.05)
    assert tuple(out[7].shape) == (3, 0, 2) and int(out[0].sum()) > 0


def _site_list(mask):
    ys, xs = np.nonzero(mask)                                   # row-major order == the kernel's site order
    return np.stack([xs, ys], 1)


@pytest.mark.parametrize("local", [1, 2, 0])
@pytest.mark.parametrize("case", ["random64", "ring_only", "no_corners", "golden_view", "odd_37x53", "sparse_odd_91x45"])
def test_i0_linear_inpaint_vs_scipy_delaunay(pd, case, local):
    """texture_gen_method='linear' (ours_utils.py:610-643 -> scipy griddata linear = qhull Delaunay + barycentric interpolation).
    The device finds, per unknown pixel, its Delaunay triangle exactly (integer predicates).  Equality with scipy is required
    wherever the values agree to 1e-5; every other pixel must sit in a co-circular configuration where the device's triangle is
    still a valid Delaunay triangle containing the pixel (exact brute-force check), and NaN (outside the hull) must coincide."""
    rng = np.random.default_rng(11)
    if case == "golden_view":
        g = load_golden("proj_sparse_dense.npz")
        img, m2 = g['ref_sparse'][0].astype(np.float32), g['ref_mask2'][0]
    else:
        H, W = (37, 53) if case == "odd_37x53" else (91, 45) if case == "sparse_odd_91x45" else (64, 64)   # (odd sizes: ragged 8x8 / 16x16 tiles)
        m = rng.uniform(0, 1, (H, W)) > (0.9 if case not in ("ring_only", "sparse_odd_91x45") else 2.0 if case == "ring_only" else 0.985)
        if case != "no_corners":
            m[0, :] = m[-1, :] = m[:, 0] = m[:, -1] = True      # the reference's images: background border = sites
        else:
            m[:6, :] = False; m[:, :5] = False                  # queries outside the hull -> NaN
        img = rng.uniform(0, 1, (3, H, W)).astype(np.float32) * m[None]
        m2 = np.repeat(m[None].astype(np.float32), 3, 0)
    sites = m2[0] != 0
    want = oinp.reference_linear_inpaint_scipy(img, m2)
    # local = 1: two window passes (8x8 tiles / 20x20 windows, then 16x16 tiles / 48x48 windows, round 5), the global scans only for what they cannot
    # certify; 2: the 48x48 window pass only (round 3); 0: global scans only
    old_local = pd['lib'].lib().pdhip_debug_set_linear_local(local)
    try:
        got, tri = pd['ou'].linear_fill(T(img[None]), T(sites[None]), return_triangles=True)
    finally:
        pd['lib'].lib().pdhip_debug_set_linear_local(old_local)
    got, tri = N_(got)[0], N_(tri)[0]
    assert np.array_equal(got[:, sites], img[:, sites])                     # sites keep their values
    nan_w, nan_g = np.isnan(want).any(0), np.isnan(got).any(0)
    P = _site_list(sites)
    qs = np.argwhere(~sites)
    diff = np.abs(np.nan_to_num(got) - np.nan_to_num(want)).max(0)
    bad = (diff > 1e-5) | (nan_w != nan_g)
    assert bad[sites].sum() == 0
    frac = bad[~sites].mean() if (~sites).any() else 0.0
    if case != "ring_only":                                                 # (a bare square ring of sites is co-circular through and through)
        assert frac < 0.35, frac                                           # co-circular ambiguity only; most pixels agree outright
    if sites[0].all() and sites[-1].all() and sites[:, 0].all() and sites[:, -1].all() and case != "ring_only":
        # the image diagonals: pixels collinear with the two far-apart support sites phase 0 starts from (round-2 bug: lerp of the
        # two corner sites).  Each must agree with scipy or sit in a valid Delaunay triangle (checked below for every `bad` pixel);
        # a corner-to-corner segment can never be the answer when other sites exist
        seg = (tri[..., 1] == tri[..., 2]) & (tri[..., 0] >= 0) & ~sites
        assert seg.sum() == 0, int(seg.sum())                              # a full border of sites: no query on the hull boundary
    checked = 0
    for (y, x) in qs:
        t = tri[y, x]
        if nan_g[y, x]:
            assert (t == -2).all()
            continue
        if not bad[y, x] and case != "random64":
            continue                                                       # (random64: check EVERY pixel's triangle)
        assert (t >= 0).all()
        if t[1] == t[2]:                                                   # on a segment between two sites: only a HULL edge qualifies
            a, b = P[t[0]].astype(np.int64), P[t[1]].astype(np.int64)
            qv = np.array([x, y], np.int64)
            assert (b[0] - a[0]) * (y - a[1]) == (b[1] - a[1]) * (x - a[0])            # q on line ab ...
            assert ((qv - a) * (b - a)).sum() > 0 and ((qv - b) * (a - b)).sum() > 0   # ... strictly between a and b
            side = (b[0] - a[0]) * (P[:, 1].astype(np.int64) - a[1]) - (b[1] - a[1]) * (P[:, 0].astype(np.int64) - a[0])
            assert (side >= 0).all() or (side <= 0).all(), (case, y, x, t)            # ab supports the hull of the sites
            on = side == 0
            par = ((P[on].astype(np.int64) - a) * (b - a)).sum(1)
            assert not ((par > 0) & (par < ((b - a) ** 2).sum())).any(), (case, y, x, t)   # no site strictly between: a hull EDGE
        else:
            assert oinp.delaunay_triangle_is_valid(P, t, (x, y)), (case, y, x, t)
        checked += 1
        if checked > 1500:
            break
    if case == "no_corners":
        assert nan_g.any() and (nan_g & ~nan_w).sum() <= 8                  # NaN set == scipy's up to hull-boundary pixels
    # through the reference-signature entry points (same pass configuration: at co-circular pixels the two routes may pick
    # different valid triangles)
    old_local = pd['lib'].lib().pdhip_debug_set_linear_local(local)
    try:
        one = pd['ou'].naive_inpainting(T(img), T(m2), method='linear')
        views = pd['ou'].get_inpainted_images(T(img[None]), T(m2[None]), T(m2[None]), None, None, 1, method='linear')
    finally:
        pd['lib'].lib().pdhip_debug_set_linear_local(old_local)
    assert np.array_equal(np.nan_to_num(N_(one), nan=-1), np.nan_to_num(got, nan=-1))
    assert np.array_equal(np.nan_to_num(N_(views)[0], nan=-1), np.nan_to_num(got, nan=-1))


@pytest.mark.parametrize("entry", ["hpr_one_level", "hpr_two_level", "optimize_color", "sparse_views", "linear_local", "linear_global"])
def test_entries_stay_inside_the_workspace_their_query_reports(pd, entry):
    """Every entry that carves a workspace, on a dirty (0x55) buffer of pdhip_*_ws_bytes + 4096 bytes: the 4096 bytes behind the
    reported size keep their pattern, and the results equal those of a run on a zero-filled workspace of exactly the reported size.
    Shapes: the smallest that reach every region (HPR: one level, and two levels since N > 4 * 1024).  The builders and the checks live in
    tests/test_gpu_workspace.py, which runs these six rows and every other entry through them and also holds the slack between the regions."""
    import test_gpu_workspace as tw
    row = {"hpr_one_level": "one_level", "hpr_two_level": "two_level", "optimize_color": "parent", "sparse_views": "parent",
           "linear_local": "parent", "linear_global": "parent"}[entry]
    import workspace_common as wc
    assert wc.SHAPES[tw.ENTRIES[entry][0]][row] == {"hpr_one_level": (4, 300), "hpr_two_level": (2, 5000), "optimize_color": (2, 32, 32),
                                                    "sparse_views": (2, 500, 32), "linear_local": (2, 40, 40), "linear_global": (2, 40, 40)}[entry]
    regions, slack, nbytes = tw.run_guarded(pd, entry, row)
    assert nbytes > 0 and regions > 0
