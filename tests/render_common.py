"""Shared references of the render / image-metric tests -- numpy float64 only, no GPU, no skimage / cv2.

Render reference: attribute interpolation in float64 (the formula of oracle.project.interpolate, which itself stores float32), the
`% 1` wrap, oracle.optimize.texture_mapping_bilinear (grid_sample in float64: align_corners=False, border padding) on the atlas in
the orientation the kernel takes (row 0 is v = 0; the oracle function negates v, so it is fed the atlas flipped), Lambert lighting
with the normal turned towards the camera, clip, gamma, the vertical flip and the zero background.

Metric references: PSNR and the two SSIM definitions written out with explicit window loops.

Error model of the shading kernel (u = 2^-24, the float32 unit roundoff), used by tests/test_gpu_render.py:
  * texel coordinate: uv = (u0*a0 + u1*a1) + u2*a2 with u2 = (1-u0)-u1 takes 2 + 3 + 2 roundings of values <= M = max(1, max|uv|),
    uv - floor(uv) one, uv*A one and -0.5 one: below 10 roundings of at most A*M*u each, e_t <= 10*A*M*u (the bound the issue states);
  * the lookup is top + fy*(bot - top) with top = t00 + fx*(t01 - t00): a bilinear function of the coordinates whose slope in
    either coordinate is at most D, the largest texel difference around the footprint -> 2*e_t*D; its own arithmetic adds at most
    2u (the two final additions of values <= 1) + 4u*D (differences and products), and 4u*D <= (2*e_t*D) * 0.01 is carried by the
    slack between the ~7 roundings counted above and the 10 of e_t.  Colour error <= 2*e_t*D + 4u, as the issue states.
"""
import numpy as np
import torch

from oracle import optimize as oopt

U = 2.0 ** -24
C1 = (0.01 * 255) ** 2
C2 = (0.03 * 255) ** 2


# ----------------------------------------------------------------------------- fixtures
def sphere_fixture(wrap=False, seed=5):
    """The stand-in sphere at 320 faces with seeded per-vertex UVs inside [0.05, 0.95] (wrap: scaled into [-0.5, 1.5]), a random
    32 x 32 atlas in [0,1], per-vertex colours and three lights (camera_utils.py:483-487)."""
    from pointdreamer_amd import synthetic
    verts, faces = synthetic.icosphere(4)
    assert faces.shape[0] == 320
    rng = np.random.default_rng(seed)
    uvs = rng.uniform(0.05, 0.95, size=(verts.shape[0], 2)).astype(np.float32)
    if wrap:
        uvs = ((uvs.astype(np.float64) - 0.5) * (2.0 / 0.9) + 0.5).astype(np.float32)
    atlas = rng.uniform(0.0, 1.0, size=(32, 32, 3)).astype(np.float32)
    colors = rng.uniform(0.0, 1.0, size=(verts.shape[0], 3)).astype(np.float32)
    lights = np.array([[0.8, 0, 0], [0.0, 0.5, 0.0], [0.0, 0.0, -0.5]], np.float32)
    return dict(verts=verts, faces=faces, uvs=uvs, atlas=atlas, colors=colors, lights=lights, V=3, R=64, A=32)


def face_normals64(verts, faces):
    v = np.asarray(verts, np.float64)[np.asarray(faces)]
    n = np.cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 0])
    return n / np.linalg.norm(n, axis=1, keepdims=True)


def cpu_raster(fx):
    """face_idx [V,R,R] and bary [V,R,R,2] of the fixture from the oracle's CPU rasteriser, and the oracle cameras' parameters."""
    from oracle import camera as ocam, project as oproj
    cams, _, _, _ = ocam.create_cameras(fx['V'], 1.6, fx['R'])
    o = oproj.project_batch(cams, fx['verts'], np.zeros((1, 3), np.float32), False)
    _, fid, _ = oproj.rasterize(o['pos'], fx['faces'], fx['R'])
    bary = oproj.raster_barycentrics(o['pos'], fx['faces'], fid, fx['R'])
    return fid, bary, np.stack([c.params for c in cams])


# ----------------------------------------------------------------------------- render reference
def interpolate64(attr, tri, fid, bary):
    """u*a0 + v*a1 + ((1-u)-v)*a2 in float64, zeros where empty (oracle.project.interpolate's formula, kept in float64)."""
    attr = np.asarray(attr, np.float64)
    tri = np.asarray(tri, np.int64)
    bary = np.asarray(bary, np.float64)
    out = np.zeros(fid.shape + (attr.shape[1],), np.float64)
    m = fid >= 0
    f = fid[m]
    u, v = bary[m][:, 0:1], bary[m][:, 1:2]
    out[m] = (u * attr[tri[f, 0]] + v * attr[tri[f, 1]]) + ((1.0 - u) - v) * attr[tri[f, 2]]
    return out


def texel_spread(atlas, uvw):
    """D per pixel: the largest difference (over the channels) between texels of the footprint's 2 x 2 block grown by one texel on
    every side, clamped to the atlas."""
    atlas = np.asarray(atlas, np.float64)
    A = atlas.shape[0]
    pad = np.pad(atlas, ((1, 2), (1, 2), (0, 0)), mode='edge')
    win = np.lib.stride_tricks.sliding_window_view(pad, (4, 4), axis=(0, 1))            # [A, A, 3, 4, 4], window at (y0 - 1, x0 - 1)
    spread = (win.max((3, 4)) - win.min((3, 4))).max(2)                                # [A, A]
    x0 = np.floor(np.clip(uvw[..., 0] * A - 0.5, 0, A - 1)).astype(np.int64)
    y0 = np.floor(np.clip(uvw[..., 1] * A - 0.5, 0, A - 1)).astype(np.int64)
    return spread[y0, x0]


def render_reference(fid, bary, attr, tri, atlas=None, normals=None, cam_params=None, lights=None, double_side=False, gamma=None):
    """float64 reference of pdhip_shade_views from the (unflipped) face_idx / bary.  Returns a dict, every image flipped vertically:
    images [V,3,R,R], pre_gamma [V,3,R,R], albedo [V,R,R,3], mask [V,R,R], and in texture mode uv (before the wrap), frac (after)
    and D [V,R,R]; with lights also clipsum [V,R,R] (sum of the clipped n.l) and ndotcam [V,R,R]."""
    fid = np.asarray(fid)
    V, R = fid.shape[:2]
    mask = fid >= 0
    a = interpolate64(attr, tri, fid, bary)
    out = {}
    if atlas is not None:
        frac = a - np.floor(a)
        at = torch.from_numpy(np.ascontiguousarray(np.asarray(atlas, np.float64)[::-1])).permute(2, 0, 1)[None]
        alb = oopt.texture_mapping_bilinear(torch.from_numpy(frac), at.repeat(V, 1, 1, 1)).numpy()
        out.update(uv=a[:, ::-1], frac=frac[:, ::-1], D=texel_spread(atlas, frac)[:, ::-1])
    else:
        alb = a
    alb = alb * mask[..., None]
    img = alb
    if lights is not None:
        n = np.asarray(normals, np.float64)[np.where(mask, fid, 0)]                     # [V,R,R,3]
        back = np.asarray(cam_params, np.float64)[:, 6:9]
        ndc = (n * back[:, None, None, :]).sum(-1)
        n = np.where((ndc < 0)[..., None], -n, n)
        img = np.zeros_like(alb)
        clipsum = np.zeros(mask.shape)
        for l in np.asarray(lights, np.float64):
            d = (n * l).sum(-1)
            if double_side:
                d = np.abs(d)
            d = np.clip(d, 0, 1)
            img = img + alb * d[..., None]
            clipsum += d
        img = np.clip(img * mask[..., None], 0, 1)
        out.update(clipsum=clipsum[:, ::-1], ndotcam=ndc[:, ::-1])
    pre = img
    if lights is not None and gamma is not None:
        img = img ** (1.0 / gamma)
    chw = lambda x: np.ascontiguousarray(x[:, ::-1].transpose(0, 3, 1, 2))
    out.update(images=chw(img), pre_gamma=chw(pre), albedo=np.ascontiguousarray(alb[:, ::-1]), mask=np.ascontiguousarray(mask[:, ::-1]))
    return out


def texture_bound(ref, A):
    """Per-pixel colour bound 2*e_t*D + 4u with e_t = 10*A*M*u (module docstring), and e_t."""
    M = max(1.0, float(np.abs(ref['uv']).max()))
    e_t = 10.0 * A * M * U
    return 2.0 * e_t * ref['D'] + 4.0 * U, e_t


def wrap_excluded(ref, A, e_t):
    """Covered pixels whose float64 frac(uv) lies within e_t / A of 0 or 1 in either coordinate: the lookup jumps there."""
    eps = e_t / A
    fr = ref['frac']
    return ref['mask'] & ((fr < eps) | (fr > 1.0 - eps)).any(-1)


def light_rounding(lights, amax):
    """Rounding of the lighting sum in float32: per light the 3-term dot product (5 roundings of at most u*|l|_1) and the product
    with the albedo (u), plus L accumulations of a sum of at most L*amax (u*L each); clip is 1-Lipschitz."""
    l1 = np.abs(np.asarray(lights, np.float64)).sum(1)
    L = len(l1)
    return U * max(1.0, amax) * (float((5.0 * l1 + 1.0).sum()) + L * L)


# ----------------------------------------------------------------------------- metric references
def psnr_ref(a, b):
    a, b = np.asarray(a, np.int64), np.asarray(b, np.int64)
    sse = int(((a - b) ** 2).sum())
    if sse == 0:
        return float('inf'), 0
    return 10.0 * np.log10(255.0 ** 2 / (sse / a.size)), sse


def gaussian_taps(n=11, sigma=1.5):
    k = np.exp(-((np.arange(n) - (n - 1) / 2.0) ** 2) / (2.0 * sigma * sigma))
    return k / k.sum()


def _window_means(x, win):
    """Valid-region correlation of x [H,W] float64 with the 2-D window `win`, by an explicit loop over the taps."""
    k = win.shape[0]
    H, W = x.shape
    out = np.zeros((H - k + 1, W - k + 1))
    for i in range(k):
        for j in range(k):
            out += win[i, j] * x[i:i + H - k + 1, j:j + W - k + 1]
    return out


def ssim_ref(a, b, use_sk=True):
    """Mean SSIM of two uint8 [H,W,C] images under the definition of the issue's section 2."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    if a.ndim == 2:
        a, b = a[..., None], b[..., None]
    k = 7 if use_sk else 11
    if a.shape[0] < k or a.shape[1] < k:
        raise ValueError('image smaller than the window')
    win = np.full((7, 7), 1.0 / 49.0) if use_sk else np.outer(gaussian_taps(), gaussian_taps())
    cov = 49.0 / 48.0 if use_sk else 1.0
    per_channel = []
    for c in range(a.shape[2]):
        x, y = a[..., c], b[..., c]
        ux, uy = _window_means(x, win), _window_means(y, win)
        vx = cov * (_window_means(x * x, win) - ux * ux)
        vy = cov * (_window_means(y * y, win) - uy * uy)
        vxy = cov * (_window_means(x * y, win) - ux * uy)
        S = ((2 * ux * uy + C1) * (2 * vxy + C2)) / ((ux ** 2 + uy ** 2 + C1) * (vx + vy + C2))
        per_channel.append(S.mean())
    return float(np.mean(per_channel))
