"""Shared by tests/test_gpu_conv_epilogue.py and tests/test_conv_epilogue_cpu.py: what the GroupNorm octet partials of a conv output must be, how
far an honest f32 summation may stray from that, and what a GroupNorm statistic assembled from such partials may stray -- all from float64 sums over
the f16 tensor the kernel wrote, none of it from a measurement.

Octet partials (csrc/nn_gemm.hip, k_conv_igemm's epilogue): part[n][chunk][C / 8][2] = (sum, sum of squares) over the f16 values of the chunk's pixels in
channels 8 o .. 8 o + 7.  A chunk is a contiguous range of H * W / chunks pixels of image n for every producer except the halo-resident kernel's
128-column strips of a 256-wide image (4 rows x 128 columns each), where only the image totals are compared.

The bound.  A slot is an f32 sum of n = rows * 8 numbers in an order the kernel is free to choose; each addend is exact in f32 (an f16 value, or the
square of one: 22 significant bits).  Any order of n - 1 rounded additions is off by at most (n - 1) u sum|v| to first order, u = 2^-24 (Higham,
Accuracy and Stability of Numerical Algorithms, section 4.2); the tests use n u sum|v|, and the same over v^2 for the sum of squares.
"""
import torch

U32 = 2.0 ** -24
KERNELS = {'halo': 0, 'rr': 1, 'ht': 2, 'sk': 3, 'igemm': 4, 'phase': 5}      # the ConvKernel codes pdhip_debug_conv_launch_nhwc_f16 reports


def expected_partials(y, chunks):
    """y [N, H, W, C] f16 -> (exp [N, chunks, C / 8, 2] float64, bound [N, chunks, C / 8, 2] float64) for contiguous chunks."""
    N, C = y.shape[0], y.shape[-1]
    v = y.reshape(N, chunks, -1, C // 8, 8).double()
    n = v.shape[2] * 8
    s, q = v.sum(dim=(2, 4)), (v * v).sum(dim=(2, 4))
    exp = torch.stack([s, q], dim=-1)
    bound = torch.stack([n * U32 * v.abs().sum(dim=(2, 4)), n * U32 * q], dim=-1)
    return exp, bound


def partials_errors(part, y, chunks, contiguous=True):
    """Every way in which `part` ([N, chunks, C / 8, 2], what a launch left) disagrees with the f16 tensor y it is said to describe; [] = agrees."""
    N, C = y.shape[0], y.shape[-1]
    errs = []
    part = part.reshape(N, chunks, C // 8, 2).double().cpu()
    if not torch.isfinite(part).all():
        errs.append(f"{int((~torch.isfinite(part)).sum())} slots are not finite (never written?)")
        return errs
    exp, bound = expected_partials(y.cpu(), chunks)
    names = ('sum', 'sum of squares')
    # per image and octet, over the chunks: what both consumers use (the bounds of the chunks add up)
    dt, bt = (part.sum(dim=1) - exp.sum(dim=1)).abs(), bound.sum(dim=1)
    for k in range(2):
        if (dt[..., k] > bt[..., k]).any():
            n, o = [int(i) for i in torch.nonzero(dt[..., k] > bt[..., k])[0]]
            errs.append(f"image total {names[k]}: image {n} octet {o} off by {dt[n, o, k]:.3e} > {bt[n, o, k]:.3e}")
    if contiguous:
        d = (part - exp).abs()
        for k in range(2):
            if (d[..., k] > bound[..., k]).any():
                n, c, o = [int(i) for i in torch.nonzero(d[..., k] > bound[..., k])[0]]
                errs.append(f"chunk {names[k]}: image {n} chunk {c} octet {o} off by {d[n, c, o, k]:.3e} > {bound[n, c, o, k]:.3e} "
                            f"({int((d[..., k] > bound[..., k]).sum())} slots)")
    return errs


def group_stats(tensors, eps=1e-5):
    """float64 GroupNorm(32) (mean, rstd) [N, 32] of the channel concat of the f16 tensors [N, HW, C_i]."""
    x = torch.cat([t.double().cpu() for t in tensors], dim=-1)
    N, HW, C = x.shape
    g = x.reshape(N, HW, 32, C // 32)
    mean = g.mean(dim=(1, 3))
    var = (g * g).mean(dim=(1, 3)) - mean * mean
    return mean, (var + eps) ** -0.5


def stats_bounds(tensors, chunks, eps=1e-5):
    """How far (mean, rstd) assembled from f32 octet partials may lie from group_stats(tensors): (bound_mean, bound_rstd) [N, 32].
    Every slot of source i carries at most n_i u sum|v| (n_i u sum v^2) with n_i = 8 HW / chunks_i; the slots of a group add up to dS <= sum_i n_i u S|.|_i,
    dQ alike; mean = S / cnt, var = Q / cnt - mean^2 gives dvar <= dQ / cnt + (2 |mean| + dmean) dmean; rstd = (var + eps)^-1/2 is monotone, so the
    worst case is at var - dvar (clamped at 0 like the kernel).  The combine is in f64; the results are stored as f32 (one rounding, 2^-24 relative)."""
    N, HW = tensors[0].shape[:2]
    C = sum(t.shape[-1] for t in tensors)
    cg = C // 32
    ab = torch.cat([(8 * HW // ch) * U32 * t.double().cpu().abs() for t, ch in zip(tensors, chunks)], dim=-1).reshape(N, HW, 32, cg)
    dS, dQ = ab.sum(dim=(1, 3)), (ab * torch.cat([t.double().cpu().abs() for t in tensors], dim=-1).reshape(N, HW, 32, cg)).sum(dim=(1, 3))
    cnt = HW * cg
    mean, rstd = group_stats(tensors, eps)
    var = rstd ** -2 - eps
    dmean = dS / cnt
    dvar = dQ / cnt + (2 * mean.abs() + dmean) * dmean
    worst = ((var - dvar).clamp(min=0) + eps) ** -0.5
    return dmean + U32 * mean.abs(), (worst - rstd) + U32 * worst


def stats_errors(stats, tensors, chunks):
    """stats [N, 32, 2] f32 (mean, rstd) against the float64 statistics of the concat of `tensors` under stats_bounds; [] = agrees."""
    mean, rstd = group_stats(tensors)
    bm, br = stats_bounds(tensors, chunks)
    st = stats.reshape(-1, 32, 2).double().cpu()
    errs = []
    if not torch.isfinite(st).all():
        return ["statistics are not finite"]
    for name, got, want, b in (('mean', st[..., 0], mean, bm), ('rstd', st[..., 1], rstd, br)):
        d = (got - want).abs()
        if (d > b).any():
            n, g = [int(i) for i in torch.nonzero(d > b)[0]]
            errs.append(f"{name}: image {n} group {g} off by {d[n, g]:.3e} > {b[n, g]:.3e} (value {want[n, g]:.6g})")
    return errs


def make_operands(N, H, W, Cin, Cout, taps, res, seed, Cs=0, res_hw=None):
    """f16-representable operands of one case (float32 tensors, NCHW / OIHW): a bias of order 1 (channel means far from zero, each channel its own) and a
    residual whose scale and offset differ per image (a wrong image index is an O(1) error)."""
    g = torch.Generator().manual_seed(seed)
    k = 3 if taps == 9 else 1
    op = dict(x=torch.randn((N, Cin, H, W), generator=g).half().float(),
              w=(torch.randn((Cout, Cin, k, k), generator=g) / (Cin * taps) ** 0.5).half().float(),
              b=((0.75 + 0.75 * torch.rand((Cout,), generator=g)) * (1 - 2 * (torch.arange(Cout) % 3 == 1).float())).half().float())
    if res:
        rh, rw = res_hw or (H, W)
        scale = 0.5 + 0.75 * torch.arange(N, dtype=torch.float32)
        op['r'] = (torch.randn((N, Cout, rh, rw), generator=g) * scale[:, None, None, None] + (scale - 1)[:, None, None, None]).half().float()
    if Cs:
        op['xs'] = (torch.randn((N, Cs, H, W), generator=g) * 1.5).half().float()
        op['ws'] = (torch.randn((Cout, Cs, 1, 1), generator=g) / Cs ** 0.5).half().float()
        op['bs'] = (0.5 * torch.randn((Cout,), generator=g)).half().float()
    return op


def reference_f64(op):
    """float64 convolution (+ skip 1x1 + both biases) (+ residual, nearest x2 when it is half resolution) -> [N, H, W, Cout]."""
    import torch.nn.functional as F
    x, w = op['x'].double(), op['w'].double()
    ref = F.conv2d(x, w, op['b'].double(), padding=w.shape[-1] // 2)
    if 'xs' in op:
        ref = ref + F.conv2d(op['xs'].double(), op['ws'].double(), op['bs'].double())
    if 'r' in op:
        r = op['r'].double()
        if r.shape[-1] != ref.shape[-1]:
            r = F.interpolate(r, scale_factor=2, mode='nearest')
        ref = ref + r
    return ref.permute(0, 2, 3, 1).contiguous()


# ---- the cases of tests/test_gpu_conv_epilogue.py.  hooks: tile = pdhip_debug_set_conv_tile, sk = (mode, tile, splits) of pdhip_debug_set_conv_sk,
# splits = forced split-K factor (needs the workspace), strips = pdhip_debug_set_conv_halo_strips, ht = (mode, slabs) of pdhip_debug_set_conv_ht,
# rr = (variant, slabs) of pdhip_debug_set_conv_rr under mode 2 (None: mode 0).  chunks = the producer's documented chunk count per image;
# contiguous = each chunk is a contiguous pixel range.  entry: 'launch' = pdhip_debug_conv_launch_nhwc_f16; 'rr' = pdhip_conv_rr_f16 (fragment-major
# weights, which the debug launch does not carry); 'phase' = pdhip_conv3x3_up2_phase_nhwc_f16 (the engine picks that kernel, not conv_plan).
def _case(name, kernel, N, H, W, Cin, Cout, taps=9, res=True, tile=0, sk=(1, 0, 0), splits=0, ws=False, strips=0, chunks=0, contiguous=True, Cs=0, Cs1=0,
          ht=(0, 0), rr=None, entry='launch'):
    return dict(name=name, kernel=kernel, N=N, H=H, W=W, Cin=Cin, Cout=Cout, taps=taps, res=res and not Cs, tile=tile, sk=sk, splits=splits,
                ws=ws or splits > 0 or sk[2] > 1 or ht[1] > 1 or (rr is not None and rr[1] > 1), strips=strips, chunks=chunks, contiguous=contiguous,
                Cs=Cs, Cs1=Cs1, ht=ht, rr=rr, entry=entry)


def _cases():
    cs = []
    # k_conv_igemm's direct epilogue: 128-row tiles (geometry 2) or 256-row tiles (4, 8, 16); chunks = H W / tile rows.  Cout 136 = 17 octets: the last
    # n-tile is ragged (and geometry 8's 256-wide n-tile holds 15 octets beyond Cout)
    for geo in (2, 4, 8, 16):
        bmt = 128 if geo == 2 else 256
        for res in (False, True):
            cs.append(_case(f"igemm-geo{geo}-3x16x16{'-res' if res else ''}", 'igemm', 3, 16, 16, 64, 136, res=res, tile=geo, chunks=256 // bmt))
            cs.append(_case(f"igemm-geo{geo}-2x32x16{'-res' if res else ''}", 'igemm', 2, 32, 16, 64, 136, res=res, tile=geo, chunks=512 // bmt))
    # an image that is no whole number of tiles: the epilogue must leave NO partials (chunks 0) and touch nothing
    cs.append(_case("igemm-geo2-3x8x8-no-partials", 'igemm', 3, 8, 8, 64, 136, tile=2, chunks=0))
    # split igemm -> k_splitk_reduce: 16-row chunks.  3 x 8x8 = 192 rows: the second 128-row tile of the GEMM is half empty
    for sp in (2, 3):
        cs.append(_case(f"igemm-split{sp}-2x8x8", 'igemm', 2, 8, 8, 128, 136, tile=2, splits=sp, chunks=4))
    cs.append(_case("igemm-split2-3x8x8-ragged-tile", 'igemm', 3, 8, 8, 128, 136, tile=2, splits=2, chunks=4))
    cs.append(_case("igemm-split3-2x8x8-nores", 'igemm', 2, 8, 8, 128, 136, res=False, tile=2, splits=3, chunks=4))
    # halo-resident kernel, direct epilogue: 512-pixel tiles of whole rows (contiguous) or, 256 wide, 4 x 128 strips
    for (N, H, W) in ((2, 16, 32), (1, 32, 32), (1, 8, 64), (1, 4, 128)):
        cs.append(_case(f"halo-{N}x{H}x{W}", 'halo', N, H, W, 96, 136, tile=32, chunks=H * W // 512))
    cs.append(_case("halo-2x16x32-nores", 'halo', 2, 16, 32, 96, 136, res=False, tile=32, chunks=1))
    cs.append(_case("halo-2x16x256-strips", 'halo', 2, 16, 256, 32, 136, tile=32, strips=0, chunks=8, contiguous=False))
    cs.append(_case("halo-2x16x256-rows", 'halo', 2, 16, 256, 32, 136, tile=32, strips=1, chunks=8))
    # split halo -> k_splitk_reduce
    for sp in (2, 3):
        cs.append(_case(f"halo-split{sp}-1x16x32", 'halo', 1, 16, 32, 96, 136, tile=32, splits=sp, chunks=32))
        cs.append(_case(f"halo-split{sp}-2x32x32", 'halo', 2, 32, 32, 96, 136, tile=32, splits=sp, chunks=64))
    # k_conv_sk: tiles 128x128, 128x64, 64x64, 64x32; chunks = max(H W / tile rows, 1).  3 x 8x8 on 128-row tiles: two images per tile, the last tile holds
    # image 2 and nothing (the img < N guard)
    BM = {1: 128, 2: 128, 3: 64, 4: 64}
    for t in (1, 2, 3, 4):
        for sp in (1, 3):
            cs.append(_case(f"sk-tile{t}-split{sp}-3x8x8", 'sk', 3, 8, 8, 128, 136, sk=(2, t, sp), chunks=1))
            cs.append(_case(f"sk-tile{t}-split{sp}-1x16x16", 'sk', 1, 16, 16, 256, 136, sk=(2, t, sp), chunks=256 // BM[t]))
            cs.append(_case(f"sk-tile{t}-split{sp}-2x32x32", 'sk', 2, 32, 32, 64, 136, res=(t % 2 == 0), sk=(2, t, sp), chunks=1024 // BM[t]))
    cs.append(_case("sk-1x1-tile1-2x8x8", 'sk', 2, 8, 8, 1024, 256, taps=1, sk=(2, 1, 1), chunks=1))
    cs.append(_case("sk-1x1-tile4-split3-2x8x8", 'sk', 2, 8, 8, 1024, 256, taps=1, sk=(2, 4, 3), chunks=1))
    # k_conv_sk<10>: the skip 1x1 over xs = [xs | xs2] appended to the K loop
    cs.append(_case("skip-tile1-1x16x16", 'sk', 1, 16, 16, 256, 256, sk=(2, 1, 1), chunks=2, Cs=384, Cs1=256))
    cs.append(_case("skip-tile4-split3-1x16x16", 'sk', 1, 16, 16, 256, 256, sk=(2, 4, 3), chunks=4, Cs=384, Cs1=256))
    cs.append(_case("skip-tile2-2x8x8", 'sk', 2, 8, 8, 128, 136, sk=(2, 2, 1), chunks=1, Cs=64))
    cs.append(_case("skip-tile3-split2-2x8x8", 'sk', 2, 8, 8, 128, 136, sk=(2, 3, 2), chunks=1, Cs=64))
    return cs


CASES = _cases()


# ---- the kernels the list above does not reach, at the smallest shapes their planners take (tests/conv_tail_common.py launches them; the float64
# test and the parent-bytes test of the shared conv tail run CASES + TAIL_CASES).  H, W: the output's.
def _tail_cases():
    cs = []
    # k_conv_ht: 256-pixel x 64-channel tiles of whole rows, chunks = H W / 256; one K-slab (no hand-off) and several (in-launch combine); the three widths
    cs.append(_case("ht-1x32x32-slab1", 'ht', 1, 32, 32, 64, 136, ht=(2, 1), chunks=4))
    cs.append(_case("ht-1x32x32-slab2", 'ht', 1, 32, 32, 64, 136, ht=(2, 2), chunks=4))
    cs.append(_case("ht-2x64x64-slab4-nores", 'ht', 2, 64, 64, 128, 72, res=False, ht=(2, 4), chunks=16))
    cs.append(_case("ht-1x128x128-slab1", 'ht', 1, 128, 128, 32, 64, ht=(2, 1), chunks=64))
    # k_conv_rr: chunks = bands per image.  Variant 5 (8 wide, 64 data rows in 128 row slots: fewer data rows than rows per pass), 2 (16 wide, 32-channel
    # tiles: 128 rows in two passes of 64), 7 (16 wide, 16-channel tiles: 128 rows, one pass), 8 (64 wide: 256 rows in four passes); one slab and several
    for sl in (1, 2):
        cs.append(_case(f"rr-v5-2x8x8-slab{sl}", 'rr', 2, 8, 8, 256, 48, rr=(5, sl), chunks=1, entry='rr'))
        cs.append(_case(f"rr-v2-1x16x16-slab{sl}", 'rr', 1, 16, 16, 256, 96, rr=(2, sl), chunks=2, entry='rr'))
    cs.append(_case("rr-v7-3x16x16-slab2-nores", 'rr', 3, 16, 16, 256, 48, res=False, rr=(7, 2), chunks=2, entry='rr'))
    cs.append(_case("rr-v8-1x64x64-slab2", 'rr', 1, 64, 64, 256, 32, rr=(8, 2), chunks=16, entry='rr'))
    # the four-phase up conv (k_conv_igemm<4>): conv3x3(nearest_x2(x)) over the half-resolution x, 256-row tiles per phase, chunk = 4 tile + phase (the
    # pixels of one parity: not a contiguous range); 256x256 tiles (padded Cout 256) and 256x128
    cs.append(_case("phase-2x32x32-geo8", 'phase', 2, 32, 32, 64, 136, res=False, chunks=4, contiguous=False, entry='phase'))
    cs.append(_case("phase-1x64x64-geo16", 'phase', 1, 64, 64, 64, 72, res=False, chunks=16, contiguous=False, entry='phase'))
    return cs


TAIL_CASES = _tail_cases()


def workspace_floats(c):
    """split-K workspace of a case: 4096 ticket words + room for `splits` f32 copies of the padded output (every kernel's need is below that)."""
    if not c['ws']:
        return 0
    pad = (c['Cout'] + 127) // 128 * 128
    M = c['N'] * c['H'] * c['W']
    return 4096 + max(c['splits'], c['sk'][2], c['ht'][1], (c['rr'] or (0, 0))[1], 1) * (M + 128) * pad


class Hooks:
    """Sets the routing hooks of a case and restores every one of them on exit (L: the loaded library)."""

    def __init__(self, L, c):
        self.L, self.c = L, c

    def __enter__(self):
        L, c = self.L, self.c
        self.old = (L.pdhip_debug_set_conv_tile(c['tile']), L.pdhip_debug_set_conv_sk(*c['sk']), L.pdhip_debug_set_conv_halo_strips(c['strips']),
                    L.pdhip_debug_set_conv_ht(*c['ht']), L.pdhip_debug_set_conv_rr(*((2,) + tuple(c['rr']) if c['rr'] else (0, 0, 0))))
        # (the forced split factor travels with pdhip_debug_set_conv_splitk; its workspace pointer serves pdhip_conv2d_nhwc_f16 only)
        L.pdhip_debug_set_conv_splitk(None, 0, c['splits'])
        return self

    def __exit__(self, *exc):
        L, o = self.L, self.old
        L.pdhip_debug_set_conv_tile(o[0]); L.pdhip_debug_set_conv_sk(o[1], 0, 0); L.pdhip_debug_set_conv_halo_strips(o[2])
        L.pdhip_debug_set_conv_ht(o[3], 0); L.pdhip_debug_set_conv_rr(o[4], 0, 0)
        L.pdhip_debug_set_conv_splitk(None, 0, 0)
        return False
