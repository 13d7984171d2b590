"""Case builders and per-stage references for csrc/unproject.hip, numpy only (no torch, no device): shared by tests/test_unproject_stages_cpu.py,
which holds the references to slow restatements, and tests/test_gpu_unproject_stages.py, which holds the kernels to the references.

Four stages, each with inputs of its own so that no stage is checked through the one before it:
  NBF         oracle.nbf.shrink_visibility on images built by name (nbf_image)
  visibility  ref_visibility: the float32 contract of oracle/camera.py and oracle.project.point_validation_by_depth, restated for a dense
              [S,A,A] atlas at any A; ref_visibility_f64: the same formula in float64, with the texels whose verdict rounding may decide
  selection   ref_view_select: oracle/unproject.py:56-86 restated per texel, taking the visibility and the shrunk levels as inputs
  compaction  np.argwhere order; np.packbits(bitorder='little') for the bit transport
Everything the kernels produce here is a verdict, an index or a copied colour: the GPU file compares with equality."""
import numpy as np

from oracle import camera as ocam
from oracle import nbf as onbf

F32 = np.float32
FILL = 0x55                                                        # every output and workspace starts as these bytes
GUARD = 256                                                        # bytes in front of and behind `out` that must keep them

# pdhip_nbf_path values (include/pdhip.h)
BYTES, BITS_PACK16, BITS_BALLOT, COPY = 0, 1, 2, 3
PATH_NAME = {BYTES: 'bytes', BITS_PACK16: 'bits+pack16', BITS_BALLOT: 'bits+ballot', COPY: 'copy'}


def align_mask(mask=0, visibility=0, out=0, ws=0):
    """The align_mask argument of pdhip_nbf_path from four addresses."""
    return ((mask | visibility) & 15) | ((out & 15) << 4) | ((ws & 7) << 8)


# ------------------------------------------------------------------------------------------------------------------------ NBF
NBF_SIZES = [1, 5, 63, 64, 65, 100, 128, 192, 320]
NBF_VIEWS = [1, 2, 3, 5]
NBF_IMAGES = ['all', 'none', 'one_top_left', 'one_top_right', 'one_bottom_left', 'one_bottom_right', 'one_31_63', 'one_32_64', 'checker',
              'vertical_edge', 'horizontal_edge', 'mask_edge', 'blobs', 'blobs_bytes']
TRUE_BYTES = np.array([1, 2, 0x7f, 0x80, 0xff], np.uint8)


def nbf_kernel_lists(A):
    return [[1], [3], [21, 11, 7], [21, 21, 7], [127], [129], [2 * A + 1], [0]]


def blobs(A, rng, block=16, p=0.7):
    """Random blocky regions: a coarse grid of set / clear blocks, shifted by a random offset so that block edges fall on every column phase."""
    nb = A // block + 2
    coarse = rng.random((nb, nb)) < p
    oy, ox = rng.integers(0, block, 2)
    return np.kron(coarse, np.ones((block, block), bool))[oy:oy + A, ox:ox + A].copy()


def _one(A, y, x):
    img = np.zeros((A, A), bool)
    img[min(y, A - 1), min(x, A - 1)] = True
    return img


def nbf_image(name, A, V, seed=0):
    """(mask [A,A] u8, visibility [V,A,A] u8) of the named image.  View 0 carries the image as named, odd views its transpose, even views its
    point reflection (the blob images draw every view afresh), so that a kernel indexing the wrong view cannot pass."""
    rng = np.random.default_rng([seed, A, V, NBF_IMAGES.index(name)])
    mask = np.ones((A, A), bool)
    yy, xx = np.mgrid[0:A, 0:A]
    if name == 'all':
        base = np.ones((A, A), bool)
    elif name == 'none':
        base = np.zeros((A, A), bool)
    elif name.startswith('one_'):
        pos = {'one_top_left': (0, 0), 'one_top_right': (0, A - 1), 'one_bottom_left': (A - 1, 0), 'one_bottom_right': (A - 1, A - 1),
               'one_31_63': (31, 63), 'one_32_64': (32, 64)}[name]
        base = _one(A, *pos)
    elif name == 'checker':
        base = ((yy + xx) & 1) == 0
    elif name == 'vertical_edge':                                  # columns 0 .. 63 set: the edge sits on the word boundary 63 | 64
        base = xx < (64 if A > 64 else (A + 1) // 2)
    elif name == 'horizontal_edge':                                # rows 0 .. 31 set: the edge sits on the band boundary 31 | 32
        base = yy < (32 if A > 32 else (A + 1) // 2)
    elif name == 'mask_edge':
        # the chart ends at a column and at a row; visibility ends with it there (suppressed edges) and once more inside it (a live edge)
        cx, cy = (64 if A > 64 else (A + 1) // 2), max(1, (3 * A) // 4)
        mask = (xx < cx) & (yy < cy)
        base = mask & (yy >= cy // 3)
    else:
        mask = blobs(A, rng, 32, 0.8)
        base = None
    vis = np.zeros((V, A, A), bool)
    for v in range(V):
        if base is None:
            vis[v] = blobs(A, rng) & mask
        else:
            vis[v] = base if v == 0 else (base.T if v & 1 else base[::-1, ::-1])
        if name == 'mask_edge' and v > 0:
            vis[v] &= mask
    mask8, vis8 = mask.astype(np.uint8), vis.astype(np.uint8)
    if name == 'blobs_bytes':                                      # any non-zero byte is "true"
        mask8 = np.where(mask, rng.choice(TRUE_BYTES, mask.shape), 0).astype(np.uint8)
        vis8 = np.where(vis, rng.choice(TRUE_BYTES, vis.shape), 0).astype(np.uint8)
    return mask8, vis8


def ref_nbf(mask8, vis8, kernels):
    """[K,V,A,A] u8 (0 / 1) of oracle.nbf.shrink_visibility; K = 1 for kernels[0] == 0, where the launcher copies the visibility BYTES."""
    if kernels[0] == 0:
        return vis8[None].copy()
    # (a clamped window of radius >= A - 1 is the whole row / column, and the oracle's shifted slices need r <= A: same result, held to the
    # reflect-padded maximum in tests/test_unproject_stages_cpu.py)
    A = mask8.shape[-1]
    clamped = [min(int(k), 2 * A - 1) for k in kernels]
    return onbf.shrink_visibility(mask8 != 0, (vis8 != 0).transpose(1, 2, 0), clamped).astype(np.uint8)


def nbf_cases(A):
    """(image, V, kernels) of size A: every image with every kernel list, the view count cycling so that each image and each list meets each V."""
    out = []
    for i, name in enumerate(NBF_IMAGES):
        for j, ks in enumerate(nbf_kernel_lists(A)):
            out.append((name, NBF_VIEWS[(i + j) % len(NBF_VIEWS)], ks))
    return out


def slow_nbf(mask8, vis8, kernels):
    """The reference's formulation, texel by texel: float Scharr response (|gx| + |gy|) / 2 > 125 on the 0 / 255 image with zero padding,
    edges of a view minus edges of the chart mask, reflect-padded k x k maximum, visibility minus that border."""
    kx = np.array([[-3, 0, 3], [-10, 0, 10], [-3, 0, 3]], np.float32)
    ky = kx.T

    def edges(img):
        A = img.shape[0]
        p = np.zeros((A + 2, A + 2), np.float32)
        p[1:-1, 1:-1] = np.where(img, 255.0, 0.0)
        e = np.zeros((A, A), bool)
        for y in range(A):
            for x in range(A):
                w = p[y:y + 3, x:x + 3]
                e[y, x] = (abs(float((w * kx).sum())) + abs(float((w * ky).sum()))) / 2 > 125
        return e

    V, A, _ = vis8.shape
    bg = edges(mask8 != 0)
    out = np.zeros((len(kernels), V, A, A), np.uint8)
    for v in range(V):
        ev = edges(vis8[v] != 0) & ~bg
        for ki, k in enumerate(kernels):
            r = (k - 1) // 2
            p = np.pad(ev.astype(np.float32), r, mode='reflect') if r else ev.astype(np.float32)
            for y in range(A):
                for x in range(A):
                    out[ki, v, y, x] = 1 if (vis8[v, y, x] != 0 and not p[y:y + k, x:x + k].max() > 0) else 0
    return out


# ------------------------------------------------------------------------------------------------------------------------ cameras and texels
def cameras(V, distance=1.6):
    """[V,16] f32 camera parameters and [V,3] f32 view directions: the Fibonacci sphere of oracle/camera.py (one fixed eye at V = 1, where its
    spacing divides by zero)."""
    eyes = ocam.fibonacci_sphere(V, distance) if V > 1 else np.array([[0.4, 0.5, 1.4663]])
    at = np.zeros(3)
    params = np.stack([ocam.camera_params(e, at, ocam.calculate_up_vector(e, at)) for e in eyes])
    return params.astype(F32), (eyes - at).astype(F32)


def texels(S, A, rng, masked=0.8):
    """gb_pos [S,A,A,3] f32 in the cube |x| <= 0.55 and mask [S,A,A] u8.  Texels outside the mask hold garbage (NaN, 1e30, -1e30): never read."""
    gb = rng.uniform(-0.55, 0.55, (S, A, A, 3)).astype(F32)
    mask = (rng.random((S, A, A)) < masked)
    if A == 1:
        mask[:] = True
    junk = rng.choice(np.array([np.nan, 1e30, -1e30], F32), (S, A, A, 3))
    gb = np.where(mask[..., None], gb, junk).astype(F32)
    return gb, mask.astype(np.uint8)


def crop_params(S, V, rng):
    """uv_centers [S*V,2], uv_scales [S*V]: different for every view of every shape; scales small enough that some texels project outside."""
    return rng.uniform(-0.06, 0.06, (S * V, 2)).astype(F32), rng.uniform(1.25, 1.9, S * V).astype(F32)


def _project(cams, gb, uvc, uvs, sf, pad9, dt):
    """xn-, yn-derived uv [S,V,A,A,2] and zn [S,V,A,A] in dtype dt, one rounding per operation, the order of oracle/camera.py and
    oracle/unproject.py (sf None: the depth-test form without the scale factor)."""
    S, A = gb.shape[0], gb.shape[1]
    V = cams.shape[0]
    p = cams.astype(dt)
    x, y, z = (gb[..., i].astype(dt)[:, None] for i in range(3))           # [S,1,A,A]
    c = lambda i: p[:, i].reshape(1, V, 1, 1)
    with np.errstate(all='ignore'):
        cam = [((c(3 * r) * x + c(3 * r + 1) * y) + c(3 * r + 2) * z) + c(9 + r) for r in range(3)]
        w = -cam[2]
        xn, yn, zn = (c(12) * cam[0]) / w, (c(13) * cam[1]) / w, (c(14) * cam[2] + c(15)) / w
        cen = uvc.astype(dt).reshape(S, V, 1, 1, 2)
        sc = uvs.astype(dt).reshape(S, V, 1, 1)
        u, t = (xn - cen[..., 0]) / sc, (yn - cen[..., 1]) / sc
        if sf is not None:
            f = sf.astype(dt).reshape(S, V, 1, 1)
            u, t = u * f, t * f
        u, t = u * dt(pad9) + dt(0.5), t * dt(pad9) + dt(0.5)
    return u, t, zn


def _pixel(u, R, dt):
    """clip(u * R, 0, R - 1) truncated to an integer; NaN -> 0 (common.h clip_to_int: the reference itself would index out of range)."""
    with np.errstate(invalid='ignore'):
        c = np.clip(u * dt(R), dt(0), dt(R - 1))
        return np.where(np.isnan(c), 0, c).astype(np.int64)


# ------------------------------------------------------------------------------------------------------------------------ visibility
VIS_SIZES = [1, 17, 64, 96]
VIS_RES = [1, 5, 128]
VIEWS = [1, 2, 7, 8, 9, 31, 32]
VIS_SHAPES = [1, 3]
OFFSET = F32(0.0001)
PADDING = 0.05
# Largest difference between the float32 contract and the float64 restatement over every case of vis_cases() and the A = 1088 case, measured by
# tests/test_unproject_stages_cpu.py::test_visibility_bands_bound_the_measured_rounding (which asserts that these figures still bound it):
#   depth margin zn - ref - offset: 1.44e-7 (a little over two ulp of a zn just below 1);  uv: 3.16e-7 (texels that project far outside the view)
# The bands are four times that: they bound rounding, not the kernel.  A texel-view pair whose float64 margin lies inside ZN_BAND, or whose float64
# pixel coordinate lies within UV_BAND * R of a cell edge, is left out of the float64 check (and only of that one).
ZN_DIFF_MEASURED, UV_DIFF_MEASURED = 1.45e-7, 3.2e-7
ZN_BAND, UV_BAND = 4 * ZN_DIFF_MEASURED, 4 * UV_DIFF_MEASURED
LEFT_OUT_CAP = 0.02


def vis_case(A, R, V, S, seed=0):
    """One visibility case.  Depth maps are white noise over the range of zn the texels reach: the verdict of a texel then depends on the very
    cell it reads (row and column, view and shape), and its margin is spread over 1e-2 where rounding moves it by 1e-7.  A few texels have a NaN
    coordinate; a few cells hold exactly zn - offset of a texel that reads them, as the float32 reference computes it."""
    rng = np.random.default_rng([seed, A, R, V, S])
    cams, dirs = cameras(V)
    gb, mask = texels(S, A, rng)
    uvc, uvs = crop_params(S, V, rng)
    mesh = rng.uniform(0.980, 0.993, (S * V, R, R)).astype(F32)
    case = dict(A=A, R=R, V=V, S=S, cams=cams, dirs=dirs, gb_pos=gb, mask=mask, uv_centers=uvc, uv_scales=uvs, padding=PADDING,
                mesh=mesh, offset=OFFSET)
    n = A * A
    if n >= 64:
        flat = np.flatnonzero(mask.reshape(-1))
        nan_at = rng.choice(flat, max(1, len(flat) // 200), replace=False)
        g = gb.reshape(-1, 3)
        g[nan_at, rng.integers(0, 3, len(nan_at))] = np.nan
        # ties: texel t of shape s, view v -> the cell it reads holds f32(zn - offset), and the next float above and below for two more
        u, t, zn = _project(cams, gb, uvc, uvs, None, F32(1 - 2 * PADDING), F32)
        col, row = _pixel(u, R, F32), _pixel(t, R, F32)
        ok = np.flatnonzero((mask[:, None] != 0).repeat(V, 1).reshape(-1) & np.isfinite(zn.reshape(-1)))
        ties = rng.choice(ok, min(len(ok), max(3, len(ok) // 400)), replace=False)
        for i, k in enumerate(ties):
            sv, rem = divmod(int(k), n)
            val = F32(zn.reshape(-1)[k] - OFFSET)
            val = [val, np.nextafter(val, F32(2)), np.nextafter(val, F32(0))][i % 3]
            mesh[sv, row.reshape(-1)[k], col.reshape(-1)[k]] = val
        case['n_ties'] = len(ties)
    return case


def vis_cases(V):
    return [(A, R, S) for A in VIS_SIZES for R in VIS_RES for S in VIS_SHAPES]


def _project32(c):
    """The float32 projection of a visibility case, computed once per case."""
    if '_p32' not in c:
        c['_p32'] = _project(c['cams'], c['gb_pos'], c['uv_centers'], c['uv_scales'], None, F32(1 - 2 * c['padding']), F32)
    return c['_p32']


def ref_visibility(c):
    """[S*V,A,A] u8: the float32 contract (oracle.camera.transform_points, oracle.project.point_validation_by_depth) on the dense atlas."""
    S, V, A, R = c['S'], c['V'], c['A'], c['R']
    u, t, zn = _project32(c)
    col, row = _pixel(u, R, F32), _pixel(t, R, F32)
    ref = c['mesh'].reshape(S, V, R, R)[np.arange(S)[:, None, None, None], np.arange(V)[None, :, None, None], row, col]
    with np.errstate(invalid='ignore'):
        vis = ((zn - ref) <= c['offset']) & (c['mask'][:, None] != 0)
    return vis.astype(np.uint8).reshape(S * V, A, A)


def ref_visibility_f64(c):
    """(verdict, counted, diff_zn, diff_uv): the float64 restatement, the pairs whose float64 verdict binds the kernel (inside the mask, cell
    unambiguous, margin outside ZN_BAND; a NaN position counts, its verdict is 'hidden'), and the largest difference to the float32 contract
    in the margin and in uv over the finite pairs inside the mask."""
    S, V, A, R = c['S'], c['V'], c['A'], c['R']
    pad9 = F32(1 - 2 * c['padding'])                                # (the kernel's pad9 is a float)
    u, t, zn = _project(c['cams'], c['gb_pos'], c['uv_centers'], c['uv_scales'], None, pad9, np.float64)
    u32, t32, zn32 = _project32(c)
    col, row = _pixel(u, R, np.float64), _pixel(t, R, np.float64)
    sI, vI = np.arange(S)[:, None, None, None], np.arange(V)[None, :, None, None]
    mesh = c['mesh'].reshape(S, V, R, R).astype(np.float64)
    ref = mesh[sI, vI, row, col]
    off = np.float64(c['offset'])
    inside = np.broadcast_to(c['mask'][:, None] != 0, zn.shape)
    with np.errstate(invalid='ignore'):
        margin = zn - ref - off
        verdict = (margin <= 0) & inside
        b = UV_BAND * R
        same_cell = (_pixel(u - UV_BAND, R, np.float64) == _pixel(u + UV_BAND, R, np.float64)) & \
                    (_pixel(t - UV_BAND, R, np.float64) == _pixel(t + UV_BAND, R, np.float64)) & (b < 0.5)
        nan = np.isnan(zn) | np.isnan(u) | np.isnan(t)
        counted = inside & ((same_cell & (np.abs(margin) > ZN_BAND)) | nan)
        fin = inside & np.isfinite(zn) & np.isfinite(u) & np.isfinite(t)
        ref32 = c['mesh'].reshape(S, V, R, R)[sI, vI, _pixel(t32, R, F32), _pixel(u32, R, F32)]
        m32 = (zn32 - ref32).astype(np.float64) - off
        both = fin & (_pixel(u32, R, F32) == col) & (_pixel(t32, R, F32) == row)
        dz = float(np.abs(m32 - margin)[both].max()) if both.any() else 0.0
        du = float(max(np.abs(u32 - u)[fin].max(), np.abs(t32 - t)[fin].max())) if fin.any() else 0.0
    return verdict.astype(np.uint8).reshape(S * V, A, A), counted.reshape(S * V, A, A), dz, du


# ------------------------------------------------------------------------------------------------------------------------ view selection
SEL_SIZES = [1, 17, 64, 96]
SEL_LEVELS = [1, 2, 3]
SEL_RES = [1, 7, 64]
SEL_KERNELS = [7, 3, 1]                                            # shrunk levels of a case: the first K of these
SEL_FACES = 257
MIN_PER_CLASS = 50


def sel_cases(V):
    """(A, K, complete, r, S) for view count V: every size with every level count, both settings of `complete` and both shape counts, the image
    resolution cycling so that each r meets each A and each K."""
    out = []
    for ia, A in enumerate(SEL_SIZES):
        for ik, K in enumerate(SEL_LEVELS):
            for complete in (0, 1):
                for isx, S in enumerate((1, 3)):
                    out.append((A, K, complete, SEL_RES[(ia + ik + isx + complete) % 3], S))
    return out


def sel_case(A, V, K, r, S, seed=0):
    """One selection case.  Its visibility is blobs per view (so dense that a texel sees about two views, whatever V) with a common unseen
    region cut out; its shrunk levels are the oracle's NBF of that with SEL_KERNELS[:K]; neither comes from the stages under test."""
    rng = np.random.default_rng([seed, A, V, K, r, S, 7])
    cams, dirs = cameras(V)
    gb, mask = texels(S, A, rng, masked=0.85)
    uvc, uvs = crop_params(S, V, rng)
    sf = rng.uniform(0.8, 1.25, S * V).astype(F32)
    p = min(0.7, 2.5 / V)
    vis = np.zeros((S * V, A, A), np.uint8)
    shr = np.zeros((K, S * V, A, A), np.uint8)
    for s in range(S):
        unseen = blobs(A, rng, 8, 0.15)
        for v in range(V):
            vis[s * V + v] = blobs(A, rng, 8, p) & ~unseen & (mask[s] != 0)
        shr[:, s * V:(s + 1) * V] = ref_nbf(mask[s], vis[s * V:(s + 1) * V], SEL_KERNELS[:K])
    if V == 32 and A > 1:                                           # bit 31 of the candidate mask: a stripe only the last view sees
        for s in range(S):
            stripe = slice(A // 3, A // 3 + max(1, A // 8))
            vis[s * V:(s + 1) * V - 1, stripe] = 0
            shr[:, s * V:(s + 1) * V - 1, stripe] = 0
            vis[(s + 1) * V - 1, stripe] = mask[s, stripe]
            shr[:, (s + 1) * V - 1, stripe] = mask[s, stripe]
    F = SEL_FACES
    face_id = rng.integers(0, F, (S, A, A)).astype(np.int64)
    bd = dirs.astype(np.float64)
    a, b = rng.integers(0, V, (S, F)), rng.integers(0, V, (S, F))
    push = rng.choice([0.0, 1e-7, 3e-7, 1e-6, 3e-6, 1e-5, 3e-5, 1e-4], (S, F))
    fn = bd[a] + bd[b] + push[..., None] * bd[b]                    # bisector of two view directions (+ a push towards one of them)
    with np.errstate(invalid='ignore'):
        fn = fn / np.linalg.norm(fn, axis=-1, keepdims=True)      # (opposite directions: 0 / 0, one more NaN normal)
    rnd = rng.normal(size=(S, F, 3))
    rnd /= np.linalg.norm(rnd, axis=-1, keepdims=True)
    fn = np.where((rng.random((S, F)) < 0.6)[..., None], fn, rnd).astype(F32)   # distinct normals per shape
    with np.errstate(invalid='ignore'):
        big = rng.random((S, F)) < 0.15                             # unnormalised: the far views' softmax weights underflow
        fn[big] = (fn[big] * rng.choice([60.0, 3000.0], (int(big.sum()), 1))).astype(F32)
        fn[:, 6:9] *= F32(60.0)
        fn[:, 9:12] *= F32(3000.0)
    fn[:, 0:3] = 0.0
    fn[:, 3:6] = np.nan
    img = rng.random((S * V, 3, r, r), dtype=np.float32)
    return dict(A=A, V=V, K=K, r=r, S=S, F=F, cams=cams, dirs=dirs, gb_pos=gb, mask=mask, uv_centers=uvc, uv_scales=uvs, padding=PADDING,
                scale_factors=sf, vis=vis, shrinked=shr, face_id=face_id, f_normals=fn, inpainted=img)


def sel_candidates(c, complete):
    """cand [S,V,A,A] bool and the class of every texel: 0 candidate at level 0, 1 only at a looser level, 2 only in raw visibility, 3 none,
    -1 outside the mask (oracle/unproject.py:66-74; the class ignores `complete`, the candidates do not)."""
    S, V, A, K = c['S'], c['V'], c['A'], c['K']
    shr = c['shrinked'].reshape(K, S, V, A, A) != 0
    vis = c['vis'].reshape(S, V, A, A) != 0
    cand = shr[0].copy()
    cls = np.where(cand.any(1), 0, 3)
    for k in range(1, K):
        left = ~cand.any(1)
        cand |= shr[k] & left[:, None]
        cls = np.where(left & cand.any(1), 1, cls)
    left = ~cand.any(1)
    cls = np.where(left & vis.any(1), 2, cls)
    if complete:
        cand |= vis & left[:, None]
    cls = np.where(c['mask'] != 0, cls, -1)
    return cand, cls


def ref_view_select(c, complete):
    """(atlas [S,A,A,3] f32, painted [S,A,A] u8, view_ids [S,A,A] i32, sim [S,V,A,A] f32) of oracle/unproject.py:56-86 on the dense atlas."""
    S, V, A, r = c['S'], c['V'], c['A'], c['r']
    inside = c['mask'] != 0
    cand, _ = sel_candidates(c, complete)
    nrm = c['f_normals'][np.arange(S)[:, None, None], c['face_id']]            # [S,A,A,3]
    bd = c['dirs']
    with np.errstate(all='ignore'):
        sim = np.stack([(nrm[..., 0] * bd[v, 0] + nrm[..., 1] * bd[v, 1]) + nrm[..., 2] * bd[v, 2] for v in range(V)], 1).astype(F32)
        m = sim.max(1, keepdims=True)
        e = np.exp((sim - m).astype(np.float64)).astype(F32)
        tot = np.zeros((S, A, A), F32)
        for v in range(V):
            tot = tot + e[:, v]
        w = e / tot[:, None]
    w = np.where(cand, w, F32(-100))
    vid = w.argmax(1).astype(np.int32)                              # first maximum; the first NaN counts as the maximum (as torch.argmax)
    if not complete:
        vid = np.where(cand.any(1), vid, -100).astype(np.int32)
    vid = np.where(inside, vid, -1).astype(np.int32)
    u, t, _ = _project(c['cams'], c['gb_pos'], c['uv_centers'], c['uv_scales'], c['scale_factors'], F32(1 - 2 * c['padding']), F32)
    col, row = _pixel(u, r, F32), _pixel(t, r, F32)
    atlas = np.zeros((S, A, A, 3), F32)
    painted = vid >= 0
    sI, yI, xI = np.nonzero(painted)
    vI = vid[sI, yI, xI]
    img = c['inpainted'].reshape(S, V, 3, r, r)
    atlas[sI, yI, xI] = img[sI, vI, :, r - 1 - row[sI, vI, yI, xI], col[sI, vI, yI, xI]]      # rows flipped: img[:, ::-1, :]
    return atlas, painted.astype(np.uint8), vid, sim


def f64_selection(c, complete):
    """(view [S,A,A], decided [S,A,A]): the float64 argmax of the similarity over the candidates, and where it binds the kernel.  It binds where
    the best candidate leads the second best by more than the kernel's own shortcut margin 1e-5 AND by more than the float32 rounding of two
    similarities (each three roundings: 3 * 2^-24 * (|n0 d0| + |n1 d1| + |n2 d2|)), and where its softmax weight stays a normal float32 (best -
    max over ALL views > -80: below that the reference's own weights underflow and its argmax takes the first zero, csrc/unproject.hip)."""
    S, V = c['S'], c['V']
    cand, _ = sel_candidates(c, complete)
    nrm = c['f_normals'][np.arange(S)[:, None, None], c['face_id']].astype(np.float64)
    bd = c['dirs'].astype(np.float64)
    with np.errstate(all='ignore'):
        sim = np.stack([nrm[..., 0] * bd[v, 0] + nrm[..., 1] * bd[v, 1] + nrm[..., 2] * bd[v, 2] for v in range(V)], 1)
        mag = np.stack([np.abs(nrm[..., 0] * bd[v, 0]) + np.abs(nrm[..., 1] * bd[v, 1]) + np.abs(nrm[..., 2] * bd[v, 2]) for v in range(V)], 1)
        finite = np.isfinite(sim).all(1)
        sc = np.where(cand & finite[:, None], sim, -np.inf)
        order = np.sort(sc, 1)
        top, second = order[:, -1], (order[:, -2] if V > 1 else np.full_like(order[:, -1], -np.inf))
        gap = top - second
        need = np.maximum(1e-5, 2 * 3 * 2.0 ** -24 * np.where(finite, mag.max(1), np.inf))
        decided = (c['mask'] != 0) & cand.any(1) & finite & (gap > need) & (top - np.where(finite, sim.max(1), np.inf) > -80.0)
    return sc.argmax(1).astype(np.int32), decided


# ------------------------------------------------------------------------------------------------------------------------ compaction, bits
COMPACT_SIZES = [1, 63, 64, 65, 130, 300]
COMPACT_MASKS = ['empty', 'full', 'random', 'last_column']
PACK_SIZES = [64, 128, 64 * 17]
PACK_BYTES = np.array([0, 1, 2, 0x80, 0xff], np.uint8)


def compact_case(A, name, seed=0):
    rng = np.random.default_rng([seed, A, COMPACT_MASKS.index(name)])
    mask = {'empty': lambda: np.zeros((A, A), bool), 'full': lambda: np.ones((A, A), bool), 'random': lambda: rng.random((A, A)) < 0.4,
            'last_column': lambda: _one(A, A // 2, A - 1)}[name]()
    mask8 = np.where(mask, rng.choice(TRUE_BYTES, mask.shape), 0).astype(np.uint8)
    gb = rng.normal(size=(A, A, 3)).astype(F32)
    view_ids = rng.integers(-100, 32, (A, A)).astype(np.int32)
    return mask8, gb, view_ids


def ref_compact(mask8, gb, view_ids):
    """points [P,3], coords [P,2] i64, point_view_ids [P] i64, row offsets [A+1] i32 in np.argwhere (row-major) order."""
    m = mask8 != 0
    coords = np.argwhere(m).astype(np.int64)
    offs = np.concatenate([[0], np.cumsum(m.sum(1))]).astype(np.int32)
    return gb[m], coords, view_ids[m].astype(np.int64), offs


def pack_case(n, seed=0):
    return np.random.default_rng([seed, n]).choice(PACK_BYTES, n).astype(np.uint8)


def ref_pack(b):
    return np.packbits(b != 0, bitorder='little').view(np.uint64)
