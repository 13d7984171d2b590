"""Shared by tests/test_gpu_conv_exact.py and tests/test_conv_exact_cpu.py: conv operands whose f32 accumulation is EXACT in any order, the one f16 bit
pattern a conv kernel must then write, and a comparison that says where a wrong element sits.

The construction.  x in {-16 .. 16} / 8, w in {-16 .. 16} / 256, bias in {-2048 .. 2048} / 2048 (f32), the residual any f16 values.  Every product is a
multiple of 2^-11, so is every partial sum in any order and any split, and all of them are bounded in magnitude by sum|x||w| + |b|.  While that stays
below 2^24 2^-11 = 8192 every intermediate is exactly representable in f32 -- whatever the MFMA's internal add order, the K-slab or split-K combine order
or the pipeline depth.  acc + bias is then exact, the conversions to f16 are IEEE round-to-nearest-even, and the f32 add of two f16 values followed by the
f16 conversion equals the correctly rounded f16 sum (24 >= 2 * 11 + 2 bits: the double rounding is innocuous).  The kernel's output is ONE determined
f16 tensor; the tests compare with it bit for bit (mismatches() == []).

expected_f16 asserts the precondition for every case it serves and prints the headroom 8192 / max(sum|x||w| + |b|).
"""
import torch
import torch.nn.functional as F

import conv_epilogue_common as ce

X_UNIT, W_UNIT, B_UNIT = 2.0 ** -3, 2.0 ** -8, 2.0 ** -11         # the grids of x, w and the bias: X_UNIT * W_UNIT == B_UNIT == the unit of every sum
EXACT_LIMIT = 2.0 ** 24 * B_UNIT                                  # 8192: below it every multiple of B_UNIT is an f32 number

# ---- the rounding forms of the epilogues
# y = f16(f16(acc + bias) + residual): acc + bias rounded to f16 into the LDS staging tile, the residual added to that f16 value in f32 and rounded again.
#   nn_gemm.hip:423 / 448 (k_conv_igemm), 534 / 538 (k_splitk_reduce), nn_conv_sk.hip:469 / 500, nn_conv_halo.hip:412 / 431, nn_conv_ht.hip:277 / 298,
#   nn_conv_rr.hip:482 / 505.  Without a residual the second step is absent.
FORM_BIAS_THEN_RESIDUAL = 'f16(f16(S + b) + r)'
# y = f16(S + b), S over the 3x3 K loop AND the appended skip 1x1, b the sum of both biases: the skip takes the residual's place inside the accumulator,
#   one rounding.  nn_conv_sk.hip:469 (k_conv_sk<10>), nn_conv_rr.hip:482 (skip source).
FORM_FUSED_SKIP = 'f16(S3x3 + S1x1 + b)'
# y = f16(S + b), no residual operand at all: nn_norm.hip:454 (gs_epilogue, the sk output of k_gn_skip), nn_gemm.hip:423 with TAPS == 4 (the phase conv).
FORM_NO_RESIDUAL = 'f16(S + b)'
FORMS = (FORM_BIAS_THEN_RESIDUAL, FORM_FUSED_SKIP, FORM_NO_RESIDUAL)


class NotExact(AssertionError):
    """The operands of a case leave the range in which f32 accumulation is exact: the case proves nothing and must not run."""


def _grid(shape, lo, hi, unit, g):
    return torch.randint(lo, hi + 1, shape, generator=g).float() * unit


def make_exact_operands(N, H, W, Cin, Cout, taps, res, seed, Cs=0, res_hw=None):
    """The dyadic operands of one case in the dict layout of conv_epilogue_common.make_operands (float32 tensors, NCHW / OIHW; xs / ws / bs: the appended
    skip 1x1; r: the residual, at res_hw when given).  The residual is f16-representable with a scale and an offset of its own per image (a wrong image
    index is an O(1) error), as in make_operands."""
    g = torch.Generator().manual_seed(seed)
    k = 3 if taps == 9 else 1
    op = dict(x=_grid((N, Cin, H, W), -16, 16, X_UNIT, g), w=_grid((Cout, Cin, k, k), -16, 16, W_UNIT, g), b=_grid((Cout,), -2048, 2048, B_UNIT, g))
    if res:
        rh, rw = res_hw or (H, W)
        scale = 0.5 + 0.75 * torch.arange(N, dtype=torch.float32)
        op['r'] = (torch.randn((N, Cout, rh, rw), generator=g) * scale[:, None, None, None] + (scale - 1)[:, None, None, None]).half().float()
    if Cs:
        op['xs'] = _grid((N, Cs, H, W), -16, 16, X_UNIT, g)
        op['ws'] = _grid((Cout, Cs, 1, 1), -16, 16, W_UNIT, g)
        op['bs'] = _grid((Cout,), -2048, 2048, B_UNIT, g)
    return op


def _on_grid(t, unit):
    v = t.double() / unit
    return bool((v == v.round()).all())


def exact_sum_f64(op):
    """S + b in float64 [N, Cout, H, W] (conv + skip 1x1 + both biases) and the headroom factor, after asserting that an f32 accumulation of these operands
    is exact in any order: the operands sit on their grids, sum|x||w| + |b| < 8192 everywhere, and S + b survives the round trip through f32."""
    pairs = [('x', 'w', 'b')] + ([('xs', 'ws', 'bs')] if 'xs' in op else [])
    S = bound = 0
    for xn, wn, bn in pairs:
        x, w, b = op[xn].double(), op[wn].double(), op[bn].double()
        if not (_on_grid(x, X_UNIT) and _on_grid(w, W_UNIT) and _on_grid(b, B_UNIT)):
            raise NotExact(f"{xn} / {wn} / {bn} leave the grids 2^-3 / 2^-8 / 2^-11: a product is no multiple of 2^-11")
        S = S + F.conv2d(x, w, b, padding=w.shape[-1] // 2)
        bound = bound + F.conv2d(x.abs(), w.abs(), b.abs(), padding=w.shape[-1] // 2)
    top = bound.max().item()
    if not top < EXACT_LIMIT:
        raise NotExact(f"sum|x||w| + |b| reaches {top:.1f} >= {EXACT_LIMIT:.0f}: a partial sum may need more than 24 bits")
    if not torch.equal(S.float().double(), S):
        raise NotExact("S + b is not an f32 number")
    return S, EXACT_LIMIT / top


HEADROOM = {}      # case label -> headroom factor of every reference computed in this process (the smallest is reported)


def expected_f16(op, form, label=None):
    """The f16 tensor [N, H, W, Cout] a conv kernel must write for the exact operands `op` under the rounding form `form`."""
    assert form in FORMS, form
    S, headroom = exact_sum_f64(op)
    HEADROOM[label or f"case {len(HEADROOM)}"] = headroom
    print(f"  exact reference {label or ''}: K = {op['w'][0].numel() + (op['ws'][0].numel() if 'xs' in op else 0)}, headroom {headroom:.1f}")
    v = S.float().half()                                  # S + b is an f32 number (asserted): ONE rounding, to nearest even
    if form == FORM_FUSED_SKIP:
        assert 'xs' in op and 'r' not in op, "the fused-skip form has a skip source and no residual"
    elif form == FORM_NO_RESIDUAL:
        assert 'xs' not in op and 'r' not in op, "this form has neither a skip source nor a residual"
    else:
        assert 'xs' not in op, "a skip source rounds once: FORM_FUSED_SKIP"
        if 'r' in op:
            r = op['r'].double()
            assert torch.equal(r.half().double(), r), "the residual must be f16-representable"
            if r.shape[-1] != v.shape[-1]:
                r = F.interpolate(r, scale_factor=2, mode='nearest')
            v = (v.double() + r).half()                   # exact in float64 (<= 40 bits), rounded once: what f16(f32(v) + f32(r)) gives
    return v.permute(0, 2, 3, 1).contiguous()


def form_of(op):
    return FORM_FUSED_SKIP if 'xs' in op else FORM_BIAS_THEN_RESIDUAL if 'r' in op else FORM_NO_RESIDUAL


def up2_operands(op):
    """conv3x3(nearest_x2(x)) as a plain conv case: the operands with x up-sampled (for expected_f16)."""
    return dict(op, x=op['x'].repeat_interleave(2, dim=2).repeat_interleave(2, dim=3))


# (output phase, source tap) -> the 3x3 taps that land on that source pixel, per axis
_TAPS_OF = {(0, 0): (0,), (0, 1): (1, 2), (1, 0): (0, 1), (1, 1): (2,)}


def phase_weights_f64(w):
    """The tap sums of the four 2x2 phase convs of conv3x3(nearest_x2(.)): w [Cout, Cin, 3, 3] -> float64 [4, Cout, 4, Cin] (phase 2 py + px, tap
    2 ty + tx).  With w on its grid a sum of up to four taps is a multiple of 2^-8 of magnitude <= 64 / 256: an exact f16, so
    pdhip_pack_conv_up2_phase_f16 must reproduce these numbers bit for bit (and the phase conv's products stay multiples of 2^-11)."""
    w = w.double()
    out = torch.zeros((4, w.shape[0], 4, w.shape[1]), dtype=torch.float64)
    for py in range(2):
        for px in range(2):
            for ty in range(2):
                for tx in range(2):
                    for ky in _TAPS_OF[(py, ty)]:
                        for kx in _TAPS_OF[(px, tx)]:
                            out[2 * py + px, :, 2 * ty + tx, :] += w[:, :, ky, kx]
    assert torch.equal(out.half().double(), out)
    return out


# ---- the comparison
def _ordered(t):
    """f16 -> int32 that grows with the value (so a difference counts the f16 numbers in between); zeros of either sign -> 0."""
    b = t.contiguous().view(torch.int16).to(torch.int32) & 0xFFFF
    mag = b & 0x7FFF
    return torch.where((b & 0x8000) != 0, -mag, mag)


def _hist(idx, mod, top=6):
    v, n = torch.unique(idx % mod, return_counts=True)
    order = torch.argsort(n, descending=True)[:top]
    return ' '.join(f"{int(v[i])}:{int(n[i])}" for i in order) + (' ...' if len(v) > top else '')


def mismatches(y, want, tile=None):
    """[] when the f16 tensors y and want [N, H, W, C] agree bit for bit (zeros of either sign agree: the sign of an exactly cancelling sum depends on the
    summation order, which a kernel is free to choose; a NaN never agrees), else readable lines: how many elements differ, the first few as
    (n, row, col, channel, got, want, ulps apart), and where they sit -- image, border or interior pixel, channel mod 8 / 64 / 128 and, with
    tile = rows or (rows, columns) of the kernel's pixel tile, row (and column) mod the tile."""
    y, want = y.detach().cpu(), want.detach().cpu()
    assert y.dtype == want.dtype == torch.float16 and y.shape == want.shape, (y.dtype, y.shape, want.dtype, want.shape)
    assert not torch.isnan(want).any()
    bad = ~(y == want)                                     # NaN != anything, -0 == +0
    nbad = int(bad.sum())
    if nbad == 0:
        return []
    N, H, W, Cc = y.shape
    n, r, c, ch = torch.nonzero(bad, as_tuple=True)
    ulps = (_ordered(y) - _ordered(want)).abs()[bad]
    nan = torch.isnan(y[bad])
    lines = [f"{nbad} of {y.numel()} elements differ ({100.0 * nbad / y.numel():.3g} %), {int(nan.sum())} of them NaN (never written); "
             f"largest distance {int(ulps[~nan].max()) if (~nan).any() else 0} ulps"]
    for i in range(min(nbad, 8)):
        got, exp = y[n[i], r[i], c[i], ch[i]].item(), want[n[i], r[i], c[i], ch[i]].item()
        lines.append(f"  (n {int(n[i])}, row {int(r[i])}, col {int(c[i])}, channel {int(ch[i])}): got {got!r}, want {exp!r}, "
                     f"{'NaN' if nan[i] else str(int(ulps[i])) + ' ulps apart'}")
    border = (r == 0) | (r == H - 1) | (c == 0) | (c == W - 1)
    nb_all = H * W - max(H - 2, 0) * max(W - 2, 0)
    lines.append(f"  border pixels {int(border.sum())} (the tensor has {N * nb_all * Cc} border elements), interior {int((~border).sum())}; "
                 f"pixels hit {len(torch.unique((n * H + r) * W + c))} of {N * H * W}")
    lines.append(f"  value:count -- image {_hist(n, N)} | channel mod 8: {_hist(ch, 8, 8)} | mod 64: {_hist(ch, 64)} | mod 128: {_hist(ch, 128)}")
    if tile is not None:
        th, tw = (tile, None) if isinstance(tile, int) else tile
        s = f"  row mod {th}: {_hist(r, th, 8)}"
        if tw:
            s += f" | col mod {tw}: {_hist(c, tw, 8)}"
        lines.append(s + f" | flat pixel mod 16: {_hist((r * W + c), 16, 8)}")
    return lines


# ---- further cases through pdhip_debug_conv_launch_nhwc_f16 (beyond conv_epilogue_common.CASES): the _case dict plus x2 = channels of the first tensor of a
# two-source 1x1, res_up, lab = ((hook name, value), ...) of the pdhip_debug_set_conv_* hooks that conv_epilogue_common.Hooks does not carry
def _x(name, kernel, N, H, W, Cin, Cout, x2=0, res_up=False, lab=(), **kw):
    c = ce._case(name, kernel, N, H, W, Cin, Cout, **kw)
    c.update(x2=x2, res_up=res_up, lab=tuple(lab), chunks=0)
    return c


IGEMM_VARIANTS = [(32, 2, 2), (32, 3, 2), (32, 4, 4), (64, 2, 2), (64, 3, 4), (64, 2, 4), (32, 3, 4), (64, 2, 8), (64, 12, 2), (64, 12, 8), (64, 12, 16)]


def _extra_cases():
    cs = []
    # the two-source 1x1 (the never-materialised channel concat) on both kernels that read it
    for kernel in ('igemm', 'sk'):
        for Cin1, Cin in ((64, 192), (512, 768)):
            cs.append(_x(f"two-source-{kernel}-{Cin1}+{Cin - Cin1}", kernel, 2, 16, 16, Cin, 136, x2=Cin1, taps=1, tile=2 if kernel == 'igemm' else 0,
                         sk=(2, 3, 1) if kernel == 'sk' else (1, 0, 0)))
    # the residual read at half resolution: k_conv_sk (tiles 1 and 3) and the halo kernel where it runs unsplit by itself (>= 256 tiles)
    for t, sp in ((1, 1), (3, 3)):
        cs.append(_x(f"res-up-sk-tile{t}-split{sp}", 'sk', 2, 16, 16, 128, 136, res_up=True, sk=(2, t, sp)))
    cs.append(_x("res-up-halo-4x128x128", 'halo', 4, 128, 128, 32, 136, res_up=True))
    # every (K-step, stages, tile geometry) instantiation of k_conv_igemm on a 3x3 with residual and on a 1x1 whose M = 400 is no multiple of a tile
    for bk, st, geo in IGEMM_VARIANTS:
        lab = (('bk', bk), ('stages', st))
        cs.append(_x(f"igemm-bk{bk}-st{st}-geo{geo}-3x3", 'igemm', 2, 16, 16, 128, 192, tile=geo, lab=lab))
        cs.append(_x(f"igemm-bk{bk}-st{st}-geo{geo}-1x1", 'igemm', 1, 20, 20, 64, 512, taps=1, res=False, tile=geo, lab=lab))
    # the lab hooks of k_conv_sk, per tile, on a 3x3 (K-steps 27, two slices: 14 + 13) and a 1x1 (K-steps 5: 3 + 2); a value the tile has no
    # instantiation for falls back to the tile's default inside conv_sk
    for t in (1, 2, 3, 4):
        for hook, vals in (('sk_stages', (2, 3, 4)), ('sk_kgroups', (1, 2, 4, 8, 12)), ('sk_order', (1, 2))):
            for v in vals:
                cs.append(_x(f"sk-tile{t}-{hook}{v}-3x3", 'sk', 2, 16, 16, 192, 136, sk=(2, t, 2), lab=((hook, v),)))
                cs.append(_x(f"sk-tile{t}-{hook}{v}-1x1", 'sk', 2, 16, 16, 320, 136, taps=1, sk=(2, t, 2), lab=((hook, v),)))
    # deep K: one product of 9216 (3072) is worth less than the max-norm bound of the older tests
    cs.append(_x("deep-igemm-split4-1x8x8x1024", 'igemm', 1, 8, 8, 1024, 136, tile=2, splits=4))
    cs.append(_x("deep-sk-tile4-split3-1x8x8x1024", 'sk', 1, 8, 8, 1024, 136, sk=(2, 4, 3)))
    cs.append(_x("deep-sk-1x1-tile1-2x8x8x3072", 'sk', 2, 8, 8, 3072, 256, taps=1, sk=(2, 1, 1)))
    cs.append(_x("deep-sk-1x1-tile4-split3-2x8x8x3072", 'sk', 2, 8, 8, 3072, 256, taps=1, sk=(2, 4, 3)))
    return cs


EXTRA_CASES = _extra_cases()


def launch_case(c):
    """A case of conv_epilogue_common.CASES in the layout of EXTRA_CASES."""
    return dict(dict(x2=0, res_up=False, lab=()), **c)


class LabHooks:
    """The hooks conv_epilogue_common.Hooks carries plus the lab hooks of a case (K-step and stages of k_conv_igemm; stages, K-groups and tile order of
    k_conv_sk); every one restored on exit."""
    SETTERS = dict(bk='pdhip_debug_set_conv_bk', stages='pdhip_debug_set_conv_stages', sk_stages='pdhip_debug_set_conv_sk_stages',
                   sk_kgroups='pdhip_debug_set_conv_sk_kgroups', sk_order='pdhip_debug_set_conv_sk_order')

    def __init__(self, L, c):
        self.L, self.c, self.inner = L, c, ce.Hooks(L, c)

    def __enter__(self):
        self.inner.__enter__()
        self.old = [(name, getattr(self.L, self.SETTERS[name])(v)) for name, v in self.c.get('lab', ())]
        return self

    def __exit__(self, *exc):
        for name, v in reversed(self.old):
            getattr(self.L, self.SETTERS[name])(v)
        return self.inner.__exit__(*exc)


# ---- pdhip_conv_rr_f16 with raw input (gn_mode 0).  The rows of tests/test_gpu_round6.py's CASES (its GroupNorm rows re-run raw) and one row per remaining
# tile variant, slab count and operand.  Variants (nn_conv_rr.hip, rr_variant): 1, 5 at 8^2; 2, 7 at 16^2; 3, 6 at 32^2; 8 at 64^2 (there is no 4).
# N, HW, Ca, Cb, Cout, skip (Cs1, Cs2) or None, res (0 none, 1 same size, 2 half resolution), taps, variant, slabs
RR_CASES = [
    (1, 8, 1024, 0, 1024, None, 1, 9, 0, 0),              # K = 9216 at 8^2, variant 1 by itself, automatic slabs
    (1, 8, 1024, 1024, 1024, None, 0, 9, 0, 0),           # two-tensor source, K = 18432
    (1, 8, 1024, 0, 1024, (1024, 1024), 0, 9, 0, 0),      # appended skip over two tensors
    (2, 8, 512, 0, 256, None, 0, 9, 5, 0),
    (1, 8, 256, 0, 512, None, 0, 9, 5, 2),
    (1, 16, 1024, 0, 1024, None, 2, 9, 0, 0),             # half-resolution residual
    (1, 16, 1024, 512, 1024, None, 0, 9, 0, 0),
    (1, 16, 512, 0, 1024, None, 0, 9, 0, 4),
    (1, 16, 1024, 0, 1024, (1024, 512), 0, 9, 0, 0),
    (2, 16, 256, 0, 128, None, 1, 9, 2, 1),
    (1, 32, 512, 0, 512, None, 1, 9, 0, 0),
    (1, 32, 512, 256, 512, None, 0, 9, 0, 0),
    (1, 32, 512, 0, 512, (512, 256), 0, 9, 0, 0),
    (3, 32, 128, 0, 64, None, 2, 9, 0, 0),
    # every variant x forced slabs 1 / 2 / 4, batch 1 / 2 / 3
    (3, 8, 1024, 0, 48, None, 1, 9, 1, 1), (2, 8, 1024, 0, 48, None, 2, 9, 1, 2), (1, 8, 1024, 0, 48, None, 1, 9, 1, 4),
    (3, 8, 512, 0, 48, None, 2, 9, 5, 1), (1, 8, 512, 0, 48, (256, 0), 0, 9, 5, 4),
    (1, 16, 512, 0, 96, None, 1, 9, 2, 2), (3, 16, 512, 0, 96, None, 2, 9, 2, 4), (2, 16, 256, 0, 96, (128, 128), 0, 9, 2, 0),
    (1, 16, 512, 0, 48, None, 1, 9, 7, 1), (2, 16, 512, 0, 48, None, 2, 9, 7, 2), (3, 16, 512, 0, 48, None, 0, 9, 7, 4),
    (1, 32, 256, 0, 96, None, 2, 9, 3, 1), (2, 32, 256, 0, 96, None, 1, 9, 3, 2), (1, 32, 512, 0, 96, None, 0, 9, 3, 4),
    (1, 32, 256, 0, 48, None, 1, 9, 6, 1), (3, 32, 256, 0, 48, None, 2, 9, 6, 2), (1, 32, 512, 0, 48, (128, 0), 0, 9, 6, 4),
    (1, 64, 128, 0, 96, None, 1, 9, 8, 1), (2, 64, 256, 0, 32, None, 2, 9, 8, 2),
    # taps 1, single and two-tensor source
    (2, 8, 1024, 0, 64, None, 1, 1, 1, 2), (1, 16, 512, 256, 96, None, 2, 1, 2, 0), (3, 32, 256, 0, 96, None, 0, 1, 3, 2),
]

# ---- pdhip_conv_ht_f16: N, HW, Cin, Cout, res (0 / 1 / 2), slabs forced.  Cout 136 -> Cout_pad 192 (three 64-channel tiles, the last holds one octet).
# A slab count that does not divide Cin / 32 falls back to 1 inside conv_ht_slabs (Cin 64: 4 slabs, Cin 192: 4 slabs): the test asserts the count taken.
HT_CASES = [
    (1, 32, 64, 64, 1, 1), (1, 32, 64, 136, 2, 2), (3, 32, 64, 64, 0, 4), (3, 32, 192, 136, 2, 1), (1, 32, 192, 64, 1, 2), (1, 32, 192, 136, 1, 4),
    (1, 64, 64, 136, 1, 2), (3, 64, 64, 64, 2, 1), (1, 64, 192, 64, 2, 2), (1, 64, 192, 136, 1, 1), (3, 32, 128, 136, 1, 4), (1, 64, 256, 64, 2, 4),
]



def ht_slabs_taken(Cin, slabs):
    return slabs if (Cin // 32) % slabs == 0 else 1


def ht_workspace_floats(N, HW, Cout_pad):
    """4096 ticket words + four 64 KB slices per 256-pixel x 64-channel tile (pdhip_conv_ht_f16)."""
    return 4096 + N * (HW * HW // 256) * (Cout_pad // 64) * 4 * 16384


# ---- the up conv: hs (half-resolution size), Cin, Cout, N.  The two smallest layers of test_up2_phase_layer_vs_f64_conv, and 5 images of 10 x 10 (500
# rows: image borders inside the 256-row tiles, the second tile ragged) and 3 of 16 x 16 at Cout 136 (a ragged n-tile).  The 9-tap halo form takes a layer
# when 2 hs is one of its widths (32 ... 256); below 256 tiles it needs the tile hook 32.
UP_CASES = [(8, 1024, 1024, 1), (16, 1024, 1024, 1), (10, 64, 136, 5), (16, 64, 136, 3)]

# ---- the sk output of pdhip_gn_silu_skip1x1_nhwc_f16: Ca, Cb, H, W, N
GN_SKIP_CASES = [(Ca, Cb, H, W, N) for (Ca, Cb) in ((256, 0), (512, 256)) for (H, W) in ((8, 16), (16, 24)) for N in (1, 2)]
