"""Device UV unwrap (csrc/uv_atlas.hip, extract_texture_map.uv_unwrap / xatlas_uvmap_w_face_id): the atlas contract on meshes built
here in numpy -- wire format, one affine map per chart, no texel centre inside two UV triangles (independent float64 check), coverage,
determinism, the small-chart merge postcondition -- and the demo CLI on an OBJ without `vt` records."""
import os

import numpy as np
import PIL.Image
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = 'cuda'
COS70 = float(np.cos(np.radians(70.0)))
MERGE_K = 8
# orientation-preserving projection of each signed axis (+x -x +y -y +z -z): the two coordinates of the chart's plane
PROJ = [(1, 2), (2, 1), (2, 0), (0, 2), (0, 1), (1, 0)]
AXES = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], np.float64)


# ---- meshes
def _weld(v, f, decimals=6):
    key = np.round(v.astype(np.float64), decimals)
    _, first, inv = np.unique(key, axis=0, return_index=True, return_inverse=True)
    return v[first].astype(np.float32), inv.reshape(-1)[f].astype(np.int64)


def mesh_uv_sphere():
    from pointdreamer_amd import synthetic
    v, f, _ = synthetic.uv_sphere(50, 100)
    return v, f


def mesh_box(n=12):
    vs, fs = [], []
    g = np.linspace(-0.4, 0.4, n + 1)
    for ax in range(3):
        for sgn in (-1.0, 1.0):
            a, b = np.meshgrid(g, g, indexing='ij')
            p = np.zeros((n + 1, n + 1, 3))
            p[..., ax] = 0.4 * sgn
            p[..., (ax + 1) % 3] = a
            p[..., (ax + 2) % 3] = b
            base = sum(len(x) for x in vs)
            vs.append(p.reshape(-1, 3))
            i, j = np.meshgrid(np.arange(n), np.arange(n), indexing='ij')
            q = base + i * (n + 1) + j
            t = np.stack([np.stack([q, q + n + 1, q + 1], -1), np.stack([q + 1, q + n + 1, q + n + 2], -1)], 2).reshape(-1, 3)
            if sgn < 0:
                t = t[:, ::-1]
            fs.append(t)
    return _weld(np.concatenate(vs), np.concatenate(fs))


def mesh_torus(nu=64, nv=32, R=0.35, r=0.13):
    u, v = np.meshgrid(np.arange(nu) * 2 * np.pi / nu, np.arange(nv) * 2 * np.pi / nv, indexing='ij')
    p = np.stack([(R + r * np.cos(v)) * np.cos(u), r * np.sin(v), (R + r * np.cos(v)) * np.sin(u)], -1).reshape(-1, 3)
    i, j = np.meshgrid(np.arange(nu), np.arange(nv), indexing='ij')
    a, b = i * nv + j, ((i + 1) % nu) * nv + j
    c, d = i * nv + (j + 1) % nv, ((i + 1) % nu) * nv + (j + 1) % nv
    f = np.concatenate([np.stack([a, c, b], -1).reshape(-1, 3), np.stack([b, c, d], -1).reshape(-1, 3)])
    return p.astype(np.float32), f.astype(np.int64)


def mesh_icosphere(n, seed=0):
    """20 n^2 faces; radial noise of about 8 % of the edge length (a marching-cubes-like surface, not a smooth sphere)."""
    from pointdreamer_amd import synthetic
    return synthetic.icosphere(n, noise=0.09 / n, seed=seed)


def mesh_two_components():
    from pointdreamer_amd import synthetic
    v, f, _ = synthetic.uv_sphere(16, 32, radius=0.2)
    return np.concatenate([v - [0.3, 0, 0], v + [0.3, 0.05, 0]]).astype(np.float32), np.concatenate([f, f + len(v)])


def mesh_dirty():
    """A box with degenerate faces (repeated vertex, collinear vertices), a duplicated face and a non-manifold fin."""
    v, f = mesh_box(6)
    extra_v = np.array([[0.9, 0.9, 0.9], [1.0, 1.0, 1.0], [1.1, 1.1, 1.1], [0.0, 0.8, 0.0]], np.float32)
    n = len(v)
    e0 = f[0]
    extra_f = np.array([[f[5, 0], f[5, 0], f[5, 1]],               # repeated vertex
                        [n, n + 1, n + 2],                          # collinear
                        list(f[10]),                                # duplicate
                        [e0[0], e0[1], n + 3]], np.int64)           # fin on a manifold edge: the edge now has three faces
    return np.concatenate([v, extra_v]), np.concatenate([f, extra_f])


MESHES = {'uv_sphere': (mesh_uv_sphere, 512), 'box': (mesh_box, 512), 'torus': (mesh_torus, 512),
          'ico_10k': (lambda: mesh_icosphere(22), 1024), 'ico_160k': (lambda: mesh_icosphere(90), 2048),
          'two_components': (mesh_two_components, 512), 'dirty': (mesh_dirty, 512)}
_CACHE = {}


def unwrap(name):
    if name not in _CACHE:
        from pointdreamer_amd.extract_texture_map import uv_unwrap, uvmap_w_face_id
        build, R = MESHES[name]
        v, f = build()
        tv, tf = torch.from_numpy(v).to(DEV), torch.from_numpy(f).to(DEV)
        uvs, tex, chart = uv_unwrap(tv, tf, R, return_charts=True)
        out = uvmap_w_face_id(tv, tf, uvs, tex, R)
        _CACHE[name] = dict(v=v, f=f, R=R, uvs=uvs.cpu().numpy(), tex=tex.cpu().numpy(), chart=chart.cpu().numpy(),
                            gb_pos=out[2], mask=out[3], fid=out[4])
    return _CACHE[name]


def _area3d(v, f):
    p = v.astype(np.float64)[f]
    n = np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0])
    ln = np.linalg.norm(n, axis=1)
    with np.errstate(invalid='ignore', divide='ignore'):
        return 0.5 * ln, n / ln[:, None]


def _uv_area(c):           # [F,3,2] texel coordinates -> signed area
    return 0.5 * ((c[:, 1, 0] - c[:, 0, 0]) * (c[:, 2, 1] - c[:, 0, 1]) - (c[:, 1, 1] - c[:, 0, 1]) * (c[:, 2, 0] - c[:, 0, 0]))


def chart_maps(d):
    """Per chart: the signed axis whose projection fits UV = sigma * P + o best, that sigma, and the worst residual."""
    v, f, chart = d['v'].astype(np.float64), d['f'], d['chart']
    ids, cinv = np.unique(chart, return_inverse=True)
    uv = d['uvs'].astype(np.float64)[d['tex']].reshape(-1, 2)
    cc = np.repeat(cinv, 3)
    C = len(ids)
    cnt = np.bincount(cc, minlength=C).astype(np.float64)
    best = (np.full(C, np.inf), np.zeros(C, np.int64), np.zeros(C))
    for ax, (a, b) in enumerate(PROJ):
        P = v[f.reshape(-1)][:, [a, b]]
        mp = np.stack([np.bincount(cc, P[:, k], C) / cnt for k in range(2)], 1)
        mu = np.stack([np.bincount(cc, uv[:, k], C) / cnt for k in range(2)], 1)
        Pc, Uc = P - mp[cc], uv - mu[cc]
        num = np.bincount(cc, (Pc * Uc).sum(1), C)
        den = np.bincount(cc, (Pc * Pc).sum(1), C)
        sig = np.where(den > 0, num / np.where(den > 0, den, 1), 0.0)
        res = np.zeros(C)
        np.maximum.at(res, cc, np.abs(Uc - sig[cc, None] * Pc).max(1))
        better = res < best[0]
        best[0][better], best[1][better], best[2][better] = res[better], ax, sig[better]
    spread = np.bincount(cc, (uv - mu[cc]).__pow__(2).sum(1), C)            # 0 for a chart collapsed to one point (degenerate faces)
    return ids, cinv, best[1], best[2], best[0], spread


def overlap_count(c, R):
    """Texel centres strictly inside each UV triangle (float64, no snapping), counted per texel: [R,R] int."""
    cnt = np.zeros(R * R, np.int64)
    area = _uv_area(c)
    ok = np.abs(area) > 0
    c = c[ok].copy()
    neg = _uv_area(c) < 0
    c[neg] = c[neg][:, [0, 2, 1]]
    lo = np.floor(c.min(1) - 0.5).astype(np.int64) + 1
    hi = np.ceil(c.max(1) - 0.5).astype(np.int64) - 1
    lo, hi = np.clip(lo, 0, R - 1), np.clip(hi, -1, R - 1)
    w, h = hi[:, 0] - lo[:, 0] + 1, hi[:, 1] - lo[:, 1] + 1
    for dx in range(max(0, w.max())):
        for dy in range(max(0, h.max())):
            sel = np.nonzero((w > dx) & (h > dy))[0]
            if len(sel) == 0:
                continue
            px, py = lo[sel, 0] + dx + 0.5, lo[sel, 1] + dy + 0.5
            t = c[sel]
            inside = np.ones(len(sel), bool)
            for k in range(3):
                a, b = t[:, (k + 1) % 3], t[:, (k + 2) % 3]
                inside &= (b[:, 0] - a[:, 0]) * (py - a[:, 1]) - (b[:, 1] - a[:, 1]) * (px - a[:, 0]) > 0
            np.add.at(cnt, (lo[sel, 1] + dy)[inside] * R + (lo[sel, 0] + dx)[inside], 1)
    return cnt.reshape(R, R)


# ---- contract items 1-5 on every mesh
@pytest.mark.parametrize("name", list(MESHES))
def test_wire_format(name):
    d = unwrap(name)
    R, F = d['R'], len(d['f'])
    uvs, tex = d['uvs'], d['tex']
    assert uvs.dtype == np.float32 and uvs.ndim == 2 and uvs.shape[1] == 2 and 0 < len(uvs) <= 3 * F
    assert np.isfinite(uvs).all() and uvs.min() >= 0.0 and uvs.max() <= 1.0
    assert tex.dtype == np.int64 and tex.shape == (F, 3) and tex.min() >= 0 and tex.max() < len(uvs)
    assert set(np.unique(tex)) == set(range(len(uvs)))                        # every entry is used
    assert d['chart'].dtype == np.int32 and d['chart'].shape == (F,)
    assert tuple(d['gb_pos'].shape) == (1, R, R, 3) and d['gb_pos'].dtype == torch.float32
    assert tuple(d['mask'].shape) == (1, R, R, 1) and d['mask'].dtype == torch.bool
    assert tuple(d['fid'].shape) == (1, R, R) and d['fid'].dtype == torch.int64
    # chart ids: the smallest face index of each chart; one UV entry per (chart, vertex) pair
    ids, first = np.unique(d['chart'], return_index=True)
    assert np.array_equal(ids, first)
    pairs = np.unique(np.stack([np.repeat(d['chart'], 3), d['f'].reshape(-1)], 1), axis=0)
    assert len(pairs) == len(uvs)


@pytest.mark.parametrize("name", list(MESHES))
def test_one_affine_map_per_chart(name):
    d = unwrap(name)
    R = d['R']
    ids, cinv, ax, sig, res, den = chart_maps(d)
    assert res.max() < 2e-6 * 1024 / R + 1e-6, res.max()                      # UV = sigma * P_axis(v) + o_chart to f32 rounding
    live = den > 0
    s = np.median(sig[live])
    assert s > 0 and np.abs(sig[live] - s).max() <= 1e-4 * s                 # one texel density for every chart
    area, nrm = _area3d(d['v'], d['f'])
    nondeg = np.isfinite(area) & (area > 0)
    c = d['uvs'].astype(np.float64)[d['tex']] * R
    uva = np.abs(_uv_area(c))
    big = nondeg & (uva >= 8.0)
    ratio = uva[big] / (s * s * R * R * area[big])
    assert ratio.min() >= COS70 - 1e-4 and ratio.max() <= 1 + 1e-4, (ratio.min(), ratio.max())
    # every non-degenerate face's normal meets the cos 70 rule for its chart's axis
    assert (np.einsum('fk,fk->f', nrm[nondeg], AXES[ax[cinv[nondeg]]]) >= COS70 - 1e-5).all()
    # degenerate faces: a zero-area UV triangle
    assert (uva[~nondeg] == 0).all()


@pytest.mark.parametrize("name", list(MESHES))
def test_no_overlap_and_disjoint_rectangles(name):
    d = unwrap(name)
    R = d['R']
    c = d['uvs'].astype(np.float64)[d['tex']] * R
    cnt = overlap_count(c, R)
    assert cnt.max() <= 1, f"{int((cnt > 1).sum())} texel centres lie strictly inside two UV triangles"
    # chart rectangles with their gutters (2 texels) are disjoint
    ids, cinv = np.unique(d['chart'], return_inverse=True)
    pts = c.reshape(-1, 2)
    cc = np.repeat(cinv, 3)
    lo = np.full((len(ids), 2), np.inf)
    hi = np.full((len(ids), 2), -np.inf)
    np.minimum.at(lo, cc, pts)
    np.maximum.at(hi, cc, pts)
    lo, hi = lo - 2.0 + 1e-3, hi + 2.0 - 1e-3
    for s in range(0, len(ids), 512):
        ox = np.minimum(hi[s:s + 512, None, 0], hi[None, :, 0]) - np.maximum(lo[s:s + 512, None, 0], lo[None, :, 0])
        oy = np.minimum(hi[s:s + 512, None, 1], hi[None, :, 1]) - np.maximum(lo[s:s + 512, None, 1], lo[None, :, 1])
        both = (ox > 0) & (oy > 0)
        both[np.arange(min(512, len(ids) - s)), np.arange(s, min(s + 512, len(ids)))] = False
        assert not both.any(), "two chart rectangles (with gutters) overlap"


@pytest.mark.parametrize("name", list(MESHES))
def test_coverage_every_face_owns_a_texel(name):
    d = unwrap(name)
    R = d['R']
    c = d['uvs'].astype(np.float64)[d['tex']] * R
    uva = np.abs(_uv_area(c))
    fid = d['fid'][0].cpu().numpy()
    owned = np.zeros(len(d['f']), bool)
    owned[fid[fid >= 0]] = True
    need = uva >= 2.0
    assert owned[need].all(), f"{int((need & ~owned).sum())} faces of UV area >= 2 texels own no texel"
    m = d['mask'][0, ..., 0].cpu().numpy()
    assert np.array_equal(m, fid >= 0)


@pytest.mark.parametrize("name", ['uv_sphere', 'ico_10k', 'dirty'])
def test_deterministic(name):
    from pointdreamer_amd.extract_texture_map import xatlas_uvmap_w_face_id
    build, R = MESHES[name]
    v, f = build()
    tv, tf = torch.from_numpy(v).to(DEV), torch.from_numpy(f).to(DEV)
    a = xatlas_uvmap_w_face_id(None, tv, tf, R)
    b = xatlas_uvmap_w_face_id(None, tv, tf, R)
    for x, y in zip(a, b):
        assert x.dtype == y.dtype and x.shape == y.shape and torch.equal(x, y)


# ---- 6: merge postcondition
@pytest.mark.parametrize("name", ['ico_10k', 'ico_160k'])
def test_merge_postcondition(name):
    d = unwrap(name)
    f, chart = d['f'], d['chart']
    F = len(f)
    ids, cinv, ax, sig, res, den = chart_maps(d)
    area, nrm = _area3d(d['v'], f)
    # manifold edges: held by exactly two faces
    e = np.sort(np.stack([f, np.roll(f, -1, 1)], 2).reshape(-1, 2), 1)
    key = e[:, 0] * len(d['v']) + e[:, 1]
    order = np.argsort(key, kind='stable')
    ks = key[order]
    uniq, start, count = np.unique(ks, return_index=True, return_counts=True)
    two = start[count == 2]
    fa, fb = order[two] // 3, order[two + 1] // 3
    size = np.bincount(cinv)
    ca, cb = cinv[fa], cinv[fb]
    cross = ca != cb
    # per chart: bit L set iff every face accepts axis L (with a margin against f32 / f64 normal rounding)
    ok = np.ones((len(ids), 6), bool)
    for L in range(6):
        np.logical_and.at(ok[:, L], cinv, (nrm @ AXES[L]) >= COS70 + 1e-4)
    bad = 0
    for s_, t_ in ((ca[cross], cb[cross]), (cb[cross], ca[cross])):
        small = size[s_] < MERGE_K
        bad += int((small & ok[s_, ax[t_]]).sum())
    assert bad == 0, f"{bad} small-chart / neighbour pairs the merge would accept remain"
    assert len(ids) < F / 10                                                # charts, not faces


# ---- errors
def test_rejects_bad_indices_and_cpu_tensors():
    from pointdreamer_amd import _lib
    from pointdreamer_amd.extract_texture_map import uv_unwrap
    v, f = mesh_box(2)
    f = f.copy()
    f[3, 1] = len(v) + 5
    with pytest.raises(_lib.PdhipError, match='outside'):
        uv_unwrap(torch.from_numpy(v).to(DEV), torch.from_numpy(f).to(DEV), 256)
    with pytest.raises(_lib.PdhipError):
        uv_unwrap(torch.from_numpy(v), torch.from_numpy(f), 256)


# ---- demo CLI on an OBJ without vt
def _write_obj_without_uv(path, v, f):
    with open(path, 'w') as fh:
        for p in v:
            fh.write(f"v {p[0]:.6f} {p[1]:.6f} {p[2]:.6f}\n")
        for t in f + 1:
            fh.write(f"f {t[0]} {t[1]} {t[2]}\n")


def test_cli_textures_obj_without_uv(tmp_path):
    """demo.py:391-449 on the reference's real input: `<pc>_untextured_mesh.obj` WITHOUT vt records (what POCO / SPR emit).  The
    driver unwraps it on the device, caches geo/xatlas_512.pth in the wire format and textures it; a second run from the cache
    (with the per-view inpainted PNGs removed, as in test_gpu_demo) is bit-identical."""
    from pointdreamer_amd import demo, synthetic, io_utils
    pc = str(tmp_path / 'ball.ply')
    xyz, rgb = synthetic.sphere_points(20000, seed=3)
    io_utils.save_colored_pc_ply(xyz * 1.7 + 0.3, rgb, pc)
    verts, faces, _ = synthetic.uv_sphere(24, 48)
    _write_obj_without_uv(str(tmp_path / 'ball_untextured_mesh.obj'), verts, faces)
    args = ["--config", os.path.join(ROOT, "configs", "nearest.yaml"), "--pc_file", pc, "--set", f"output_path={tmp_path / 'out'}",
            "xatlas_texture_res=512", "point_validation_by_o3d=False"]
    out = demo.main(args)[0]
    cache = os.path.join(out, "geo", "xatlas_512.pth")
    assert os.path.exists(cache)
    d = torch.load(cache)
    assert set(d) == {"uvs", "mesh_tex_idx", "gb_pos", "mask", "per_atlas_pixel_face_id"}
    assert d["uvs"].dtype == torch.float32 and d["uvs"].shape[1] == 2 and d["mesh_tex_idx"].shape == (len(faces), 3)
    assert tuple(d["gb_pos"].shape) == (1, 512, 512, 3) and tuple(d["mask"].shape) == (1, 512, 512, 1)
    assert tuple(d["per_atlas_pixel_face_id"].shape) == (1, 512, 512) and d["per_atlas_pixel_face_id"].dtype == torch.int64
    assert 0.2 < d["mask"].float().mean() < 1.0
    obj = open(os.path.join(out, "models", "model_normalized.obj")).read()
    assert "\nvt " in obj
    a1 = np.array(PIL.Image.open(os.path.join(out, "models/model_normalized.png")))
    assert a1.shape == (512, 512, 3) and a1.std() > 5
    for k in range(8):
        os.remove(os.path.join(out, "others", f"{k}_inpainted.png"))
    out2 = demo.main(args)[0]
    a2 = np.array(PIL.Image.open(os.path.join(out2, "models/model_normalized.png")))
    assert np.array_equal(a1, a2)


# ---- the texture does not depend on the layout
# Measured on the MI355X: mean |difference| 0.0118 over 19 596 sampled points (p99 0.13: texels next to a colour edge of the
# views, where the two atlases resample differently); the bound is twice the mean.
LAYOUT_MEAN_BOUND = 0.024


def test_texture_does_not_depend_on_layout():
    """The UV sphere textured twice with 'nearest' + 'unproject' and no NBF: once with the analytic lat-long atlas of the stand-in
    geometry, once with the device unwrap.  At surface points well inside a chart in both atlases (the texel and its 8 neighbours
    belong to the sampled face's chart), the two atlases give the same colour up to resampling."""
    from pointdreamer_amd import demo, synthetic, pipeline
    from pointdreamer_amd.camera_utils import create_cameras
    from pointdreamer_amd.extract_texture_map import xatlas_uvmap_w_face_id
    A = 512
    verts, faces, lat = demo._standin_geometry(A, DEV)
    xyz, rgb = synthetic.sphere_points(20000, seed=5)
    cams, base_dirs, eyes, ups = create_cameras(num_views=8, distance=1.6, res=512, device=DEV)
    cam_info = dict(cams=cams, base_dirs=base_dirs, eye_positions=eyes, up_dirs=ups)
    fn = torch.from_numpy(synthetic.face_normals(verts.cpu().numpy(), faces.cpu().numpy())).to(DEV)
    uvs, tex, gb, m, fid = xatlas_uvmap_w_face_id(None, verts, faces, A)
    ours = dict(uvs=uvs, mesh_tex_idx=tex, gb_pos=gb, mask=m, per_atlas_pixel_face_id=fid)
    kw = dict(view_num=8, res=256, cam_res=512, point_validation_by_o3d=False, texture_gen_method='nearest', optimize_from=None,
              edge_dilate_kernels=(0,), complete_unseen_by='unproject', xatlas_texture_res=A, reuse_inpainted=False)
    T = lambda a: torch.from_numpy(np.asarray(a)).to(DEV)
    atl = {}
    for key, xd in (('latlong', lat), ('unwrap', ours)):
        atl[key] = pipeline.colorize_one_mesh(T(xyz), T(rgb), verts, faces, fn, xd, cam_info, **kw)[4].cpu().numpy()
    rng = np.random.default_rng(0)
    F = faces.shape[0]
    fs = rng.integers(0, F, 20000)
    b = rng.dirichlet((4.0, 4.0, 4.0), len(fs))
    cols = {}
    good = np.ones(len(fs), bool)
    for key, xd in (('latlong', lat), ('unwrap', ours)):
        uv = xd['uvs'].cpu().numpy().astype(np.float64)[xd['mesh_tex_idx'].cpu().numpy()[fs]]
        p = (b[:, :, None] * uv).sum(1) * A
        j, i = np.floor(p[:, 0]).astype(np.int64), np.floor(p[:, 1]).astype(np.int64)
        fmap = xd['per_atlas_pixel_face_id'][0].cpu().numpy()
        # the chart of every face: the 3x3 texel block around the sample must belong to faces of the sampled face's chart
        inside = (i >= 1) & (i < A - 1) & (j >= 1) & (j < A - 1)
        i, j = np.clip(i, 1, A - 2), np.clip(j, 1, A - 2)
        for di in (-1, 0, 1):
            for dj in (-1, 0, 1):
                inside &= fmap[i + di, j + dj] >= 0
        if key == 'unwrap':
            from pointdreamer_amd.extract_texture_map import uv_unwrap
            chart = uv_unwrap(verts, faces, A, return_charts=True)[2].cpu().numpy()
            for di in (-1, 0, 1):
                for dj in (-1, 0, 1):
                    nb = fmap[i + di, j + dj]
                    inside &= chart[np.maximum(nb, 0)] == chart[fs]
        good &= inside
        cols[key] = atl[key][i, j]
    assert good.mean() > 0.5, good.mean()
    diff = np.abs(cols['latlong'][good] - cols['unwrap'][good])
    assert diff.mean() <= LAYOUT_MEAN_BOUND, \
        f"points {int(good.sum())} mean {diff.mean():.5f} p99 {np.quantile(diff, 0.99):.5f} max {diff.max():.5f}"
