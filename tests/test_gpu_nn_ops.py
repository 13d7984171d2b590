"""GPU: attention (csrc/nn_attn.hip) and the GroupNorm-apply family (csrc/nn_norm.hip: k_gn_partial / k_gn_finalize, k_gn_apply in every template form,
k_gn_table, k_resample, k_concat), one operator at a time against float64 references under per-element bounds.

The references and bounds live in tests/nn_ops_common.py; tests/test_nn_ops_cpu.py shows on these very inputs that an honest evaluation at the kernels'
rounding points passes them and that the bugs looked for here (a skipped or repeated key chunk, a lost rescale, a wrong logit scale, swapped k / v or
keys, an rstd off by 2^-9, swapped FiLM halves, a neighbouring group's statistics, a pixel pooled twice, H and W exchanged, an unwritten tail) do not.
Every output buffer starts as NaN and is followed by a guard band that must come back untouched.  Every test records its largest error / bound ratio
with note_measured: the file it appends to (r05_u1_measured.jsonl, tests/conftest.py) is the record of the measured ratios (tests 'nn_ops_*').  A ratio near 1 would mean a derivation
is wrong, not that a bound needs widening -- except where nn_ops_common.py says the bound is attained by rounding to nearest itself."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

import nn_ops_common as oc
from conftest import note_measured

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
GUARD32 = 0x7F8ABCDE          # a NaN payload no kernel produces
GUARD16 = 0x7E5A
TAIL = 1024                   # guard elements behind every output


@pytest.fixture(scope="module")
def L():
    assert torch.cuda.is_available()
    from pointdreamer_amd import _lib
    import pointdreamer_amd.ddnm_inpainting  # noqa: F401  (registers the entry points)
    return _lib.lib()


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


class Guarded:
    """n elements of NaN (f32 / f16) followed by TAIL elements of a guard pattern, in one allocation."""

    def __init__(self, n, dtype=torch.float32):
        self.n, self.pattern = n, GUARD32 if dtype == torch.float32 else GUARD16
        itype = torch.int32 if dtype == torch.float32 else torch.int16
        self.raw = torch.full((n + TAIL,), self.pattern, dtype=itype, device=DEV)
        self.t = self.raw.view(dtype)[:n]
        self.t.fill_(float('nan'))

    def intact(self):
        return bool((self.raw[self.n:] == self.pattern).all())


def _check(got, ref, bound, what):
    """Every element finite and inside its bound; returns the largest error / bound ratio."""
    got = got.double()
    bad = ~torch.isfinite(got)
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} of {got.numel()} elements were never written, first {torch.nonzero(bad)[0].tolist()}"
    ratio = (got - ref).abs() / bound
    r = float(ratio.max())
    assert r <= 1.0, f"{what}: {int((ratio > 1).sum())} of {got.numel()} elements outside the bound, worst {r:.3g} at {torch.nonzero(ratio == ratio.max())[0].tolist()}"
    return r


# ================================================================================================ attention
@pytest.fixture(scope="module")
def att_refs():
    """float64 references on the device, one per distinct input: computed once, shared, never modified."""
    return {}


def _att_ref(cache, N, T, Cc, D, regime):
    key = (N, T, Cc, D, regime)
    if key not in cache:
        qkv = oc.attention_inputs(N, T, Cc, D, regime).to(DEV)
        cache[key] = (qkv, oc.attention_ref(qkv, D))
    return cache[key]


@pytest.mark.parametrize("case", oc.ATT_CASES, ids=[c[0] for c in oc.ATT_CASES])
def test_attention_vs_f64(L, att_refs, case):
    """k_attention<32 | 64> (vt_ws = NULL) and k_attention_t64<QTN, NBUF, TR> in all eight (qt, nbuf, vt_form) variants, each variant against the
    reference (not only against its siblings): every (image, head) has its own q, k, v, so a wrong head or image offset is an O(1) error."""
    name, kernel, N, T, Cc, D, regime = case
    qkv, ref = _att_ref(att_refs, N, T, Cc, D, regime)
    bound = oc.attention_bound(ref, T, D, oc.attention_form(kernel))
    ratios = {}
    if kernel == 'generic':
        out = Guarded(N * T * Cc, torch.float16)
        assert L.pdhip_attention_f16(_ptr(qkv), _ptr(out.t), N, T, Cc, D, None, _stream()) == 0, L.pdhip_last_error()
        torch.cuda.synchronize()
        assert out.intact(), "the halfs behind out were written"
        ratios['generic'] = _check(out.t.reshape(N, T, Cc), ref['o'], bound, name)
    else:
        assert D == 64 and T % 128 == 0 and (N * (Cc // D)) % 8 == 0          # what selects k_attention_t64
        try:
            for qt, nbuf, vtf in oc.ATT_VARIANTS:
                L.pdhip_debug_set_attn(nbuf, vtf, qt)
                out, vt = Guarded(N * T * Cc, torch.float16), Guarded(N * T * Cc, torch.float16)
                assert L.pdhip_attention_f16(_ptr(qkv), _ptr(out.t), N, T, Cc, D, _ptr(vt.t), _stream()) == 0, L.pdhip_last_error()
                torch.cuda.synchronize()
                assert out.intact() and vt.intact(), f"qt={qt} nbuf={nbuf} vt_form={vtf}: a guard band was written"
                ratios[f'qt{qt}_nbuf{nbuf}_vt{vtf}'] = _check(out.t.reshape(N, T, Cc), ref['o'], bound, f"{name} qt={qt} nbuf={nbuf} vt_form={vtf}")
        finally:
            L.pdhip_debug_set_attn(0, 0, 0)
    note_measured(test='nn_ops_attention', case=name, ratio=max(ratios.values()), **{f'ratio_{k}': v for k, v in ratios.items()})


# ================================================================================================ GroupNorm: statistics + apply, one source
def _dev(*ts):
    return [None if t is None else t.to(DEV).contiguous() for t in ts]


def _worse(worst, fl, silu, res, r):
    """Largest ratio per class of flag sets: 'one_rounding' (no FiLM, SiLU or pooling: the bound is half an f16 spacing, which rounding to nearest attains --
    ratios just below 1 by construction, nn_ops_common.py) and 'several' (two to five f16 roundings behind one another)."""
    k = 'several' if fl or silu or res == 1 else 'one_rounding'
    worst[k] = max(worst[k], r)


def _stats_check(stats, mean, rstd, dm, dr, what):
    st = stats.reshape(-1, 32, 2).double()
    assert bool(torch.isfinite(st).all()), f"{what}: statistics never written"
    rm, rr = float(((st[..., 0] - mean).abs() / dm).max()), float(((st[..., 1] - rstd).abs() / dr).max())
    assert rm <= 1.0 and rr <= 1.0, f"{what}: statistics outside the bound, mean {rm:.3g} rstd {rr:.3g}"
    return max(rm, rr)


@pytest.mark.parametrize("H,W", oc.GN_SIZES)
@pytest.mark.parametrize("Cc", oc.GN_CHANNELS)
def test_groupnorm_stats_and_apply_vs_f64(L, Cc, H, W):
    """pdhip_groupnorm_nhwc_f16 = k_gn_partial + k_gn_finalize + k_gn_apply<RES, false, FILM, false> over film x silu x resample (8 flag sets): stats_ws
    against the statistics bound in every one, y against the composed bound.  C 96 / 160: octets per pixel do not divide 256; C 768 / 1536: part of a
    workgroup idles; 16 x 18: a second statistics chunk of 32 pixels; non-square: yo = p / Wo."""
    N = oc.GN_N
    x, gamma, beta, film = _dev(*oc.gn_inputs(N, H, W, Cc))
    mean, rstd = oc.gn_stats_ref(x)
    dm, dr = oc.gn_stats_bounds(x, oc.partial_terms(Cc))
    chunks = (H * W + 255) // 256
    worst_y, worst_s = {'one_rounding': 0.0, 'several': 0.0}, 0.0
    for fl, silu, res in oc.GN_FLAGS:
        what = f"C={Cc} {H}x{W} film={fl} silu={silu} resample={res}"
        fm = film if fl else None
        ref, bound = oc.gn_ref(x, gamma, beta, fm, silu, res, mean, rstd, dm, dr)
        y, stats, ws = Guarded(ref.numel(), torch.float16), Guarded(N * 64), Guarded(N * 64 * chunks)
        rc = L.pdhip_groupnorm_nhwc_f16(_ptr(x), _ptr(gamma), _ptr(beta), _ptr(fm), N, H, W, Cc, silu, res, _ptr(y.t), _ptr(stats.t), _ptr(ws.t),
                                        N * 64 * chunks, _stream())
        assert rc == 0, L.pdhip_last_error()
        torch.cuda.synchronize()
        assert y.intact() and stats.intact() and ws.intact(), f"{what}: a guard band was written"
        worst_s = max(worst_s, _stats_check(stats.t, mean, rstd, dm, dr, what))
        _worse(worst_y, fl, silu, res, _check(y.t.reshape(ref.shape), ref, bound, what))
    note_measured(test='nn_ops_groupnorm', C=Cc, H=H, W=W, ratio_stats=worst_s, **{f'ratio_{k}': v for k, v in worst_y.items()})


def _gn_apply(L, x, x2, Ca, Cc, stats, parts, gamma, beta, film, N, H, W, silu, res, want_raw=False):
    """pdhip_gn_apply_f16 into guarded buffers -> (y [N, Ho, Wo, C], y_raw or None)."""
    Ho, Wo = (H // 2, W // 2) if res == 1 else ((2 * H, 2 * W) if res == 2 else (H, W))
    y = Guarded(N * Ho * Wo * Cc, torch.float16)
    raw = Guarded(N * Ho * Wo * Cc, torch.float16) if want_raw else None
    pa, cha, pb, chb = parts if parts is not None else (None, 0, None, 0)
    rc = L.pdhip_gn_apply_f16(_ptr(x), _ptr(x2), Ca, Cc, _ptr(stats), _ptr(pa), cha, _ptr(pb), chb, _ptr(gamma), _ptr(beta), _ptr(film), 2 * Cc, N, H, W,
                              silu, res, _ptr(y.t), _ptr(raw.t) if raw else None, _stream())
    assert rc == 0, L.pdhip_last_error()
    torch.cuda.synchronize()
    assert y.intact() and (raw is None or raw.intact()), "a guard band was written"
    return y.t.reshape(N, Ho, Wo, Cc), (raw.t.reshape(N, Ho, Wo, Cc) if raw else None)


def _f32_stats(mean, rstd):
    """Finished statistics [N, 32, 2] f32 = the float64 statistics rounded once: dm = u32 |mean|, dr = u32 rstd."""
    return torch.stack([mean, rstd], dim=-1).float().contiguous(), oc.U32 * mean.abs(), oc.U32 * rstd


@pytest.mark.parametrize("Ca,Cc", oc.GN_TWO_SOURCE)
def test_groupnorm_two_source_with_finished_statistics(L, Ca, Cc):
    """k_gn_apply<RES, false, FILM, false> on the never-materialised concat [x (Ca) | x2 (C - Ca)]: pixel strides Ca and C - Ca, one statistics row."""
    N, H, W = 2, 6, 10
    x, gamma, beta, film = _dev(*oc.gn_inputs(N, H, W, Cc))
    xa, xb = x[..., :Ca].contiguous(), x[..., Ca:].contiguous()
    mean, rstd = oc.gn_stats_ref(x)
    stats, dm, dr = _f32_stats(mean, rstd)
    worst = {'one_rounding': 0.0, 'several': 0.0}
    for fl, silu, res in oc.GN_FLAGS:
        fm = film if fl else None
        ref, bound = oc.gn_ref(x, gamma, beta, fm, silu, res, mean, rstd, dm, dr)
        y, _ = _gn_apply(L, xa, xb, Ca, Cc, stats, None, gamma, beta, fm, N, H, W, silu, res)
        _worse(worst, fl, silu, res, _check(y, ref, bound, f"Ca={Ca} C={Cc} film={fl} silu={silu} resample={res}"))
    note_measured(test='nn_ops_groupnorm_two_source', Ca=Ca, C=Cc, **{f'ratio_{k}': v for k, v in worst.items()})


def _octet_partials(L, t, N, HW, chunks):
    p = Guarded(N * chunks * (t.shape[-1] // 8) * 2)
    assert L.pdhip_gn_octet_partials_f16(_ptr(t), N, HW, t.shape[-1], chunks, _ptr(p.t), _stream()) == 0, L.pdhip_last_error()
    torch.cuda.synchronize()
    assert p.intact() and bool(torch.isfinite(p.t).all())
    return p.t


@pytest.mark.parametrize("Ca,Cc", [(256, 768), (512, 1536), (0, 256)])
def test_groupnorm_in_kernel_statistics_with_resampling(L, Ca, Cc):
    """k_gn_apply<RES, false, FILM, true>: the statistics reduced inside the kernel from octet partials (two sources chunked 2 and 3 ways; Ca = 0: one source,
    with the raw average-pool side output next to resample 1), combined with resample 0 / 1 / 2 and FiLM.  16 x 18: 288 pixels."""
    N, H, W = 2, 16, 18
    HW = H * W
    x, gamma, beta, film = _dev(*oc.gn_inputs(N, H, W, Cc))
    if Ca:
        xa, xb = x[..., :Ca].contiguous(), x[..., Ca:].contiguous()
        parts = (_octet_partials(L, xa, N, HW, 2), 2, _octet_partials(L, xb, N, HW, 3), 3)
        nt = torch.cat([torch.full((Ca,), 8.0 * HW / 2), torch.full((Cc - Ca,), 8.0 * HW / 3)]).to(DEV)
    else:
        xa, xb = x, None
        parts = (_octet_partials(L, x, N, HW, 4), 4, None, 0)
        nt = 8.0 * HW / 4
    mean, rstd = oc.gn_stats_ref(x)
    dm, dr = oc.gn_stats_bounds(x, nt)
    worst, worst_raw = {'one_rounding': 0.0, 'several': 0.0}, 0.0
    for fl, silu, res in oc.GN_FLAGS:
        fm = film if fl else None
        what = f"Ca={Ca} C={Cc} film={fl} silu={silu} resample={res}"
        ref, bound = oc.gn_ref(x, gamma, beta, fm, silu, res, mean, rstd, dm, dr)
        y, raw = _gn_apply(L, xa, xb, Ca, Cc, None, parts, gamma, beta, fm, N, H, W, silu, res, want_raw=(res == 1 and not Ca))
        _worse(worst, fl, silu, res, _check(y, ref, bound, what))
        if raw is not None:
            worst_raw = max(worst_raw, _check(raw, *oc.raw_pool_ref(x), what + " y_raw"))
    note_measured(test='nn_ops_groupnorm_in_kernel_stats', Ca=Ca, C=Cc, ratio_raw=worst_raw, **{f'ratio_{k}': v for k, v in worst.items()})


@pytest.mark.parametrize("Cc,H,W", [(32, 6, 10), (160, 16, 18), (1536, 4, 4), (256, 16, 18)])
def test_groupnorm_raw_average_pool_side_output(L, Cc, H, W):
    """resample 1 with y_raw: AvgPool2d(2) of the RAW input from the pixels the pass reads anyway -- one f16 ulp against float64, and bit-equal to k_resample,
    whose sum order it documents as its own."""
    N = 3
    x, gamma, beta, _ = _dev(*oc.gn_inputs(N, H, W, Cc))
    mean, rstd = oc.gn_stats_ref(x)
    stats, dm, dr = _f32_stats(mean, rstd)
    out = {}
    for silu in (0, 1):
        ref, bound = oc.gn_ref(x, gamma, beta, None, silu, 1, mean, rstd, dm, dr)
        y, raw = _gn_apply(L, x, None, 0, Cc, stats, None, gamma, beta, None, N, H, W, silu, 1, want_raw=True)
        out[f'ratio_silu{silu}'] = _check(y, ref, bound, f"C={Cc} {H}x{W} silu={silu}")
        rref, rbound = oc.raw_pool_ref(x)
        out[f'ratio_raw_silu{silu}'] = _check(raw, rref, rbound, f"C={Cc} {H}x{W} y_raw")
        out['raw_bit_equal_share'] = float((raw == rref.half()).float().mean())
    pooled = Guarded(raw.numel(), torch.float16)
    assert L.pdhip_resample2x_nhwc_f16(_ptr(x), N, H, W, Cc, 1, _ptr(pooled.t), _stream()) == 0, L.pdhip_last_error()
    torch.cuda.synchronize()
    assert pooled.intact() and torch.equal(pooled.t.reshape(raw.shape).view(torch.int16), raw.contiguous().view(torch.int16))
    note_measured(test='nn_ops_groupnorm_raw_pool', C=Cc, H=H, W=W, **out)


def _gn_iters(N, HoWo, Cc, in_kernel_stats=False):
    """gn_apply's pixels per thread (csrc/nn_norm.hip): GNA_ITERS = 8, halved while the grid has fewer than tgt_blocks workgroups."""
    pps = max(1, 256 // (Cc // 8))
    tgt, iters = (512 if in_kernel_stats and N <= 8 else 2048), 8
    while iters > 1 and -(-HoWo // (pps * iters)) * N < tgt:
        iters >>= 1
    return iters, pps


@pytest.mark.parametrize("fl", [0, 1])
def test_groupnorm_unrolled_loop_and_its_tail(L, fl):
    """The four-wide unrolled loop of k_gn_apply<0, ...> and the scalar tail behind it, both against float64.  Size from the tgt_blocks rule of gn_apply:
    without in-kernel statistics the grid must keep 2048 workgroups, so N ceil(H W / (pps iters)) >= 2048 at iters = 8; C = 2048 has pps = 1 (a workgroup
    walks 8 pixels, every thread all 8), N = 4 then needs H W > 511 x 8 = 4088.  63 x 65 = 4095 = 511 x 8 + 7: iters stays 8, the first 511 workgroups
    of an image run the unrolled loop twice, the last one runs it once (4 pixels) and the tail three times."""
    N, H, W, Cc = 4, 63, 65, 2048
    iters, pps = _gn_iters(N, H * W, Cc)
    assert iters == 8 and pps == 1 and (H * W) % (pps * iters) == 7
    g = torch.Generator(device=DEV).manual_seed(63 + fl)
    x = (torch.randn((N, H, W, Cc), generator=g, device=DEV) * (0.5 + 1.5 * torch.rand((N, 1, 1, Cc), generator=g, device=DEV))
         + torch.randn((N, 1, 1, Cc), generator=g, device=DEV)).half()
    _, gamma, beta, film = _dev(*oc.gn_inputs(N, 1, 1, Cc))
    fm = film if fl else None
    mean, rstd = oc.gn_stats_ref(x)
    dm, dr = oc.gn_stats_bounds(x, oc.partial_terms(Cc))
    ref, bound = oc.gn_ref(x, gamma, beta, fm, 1, 0, mean, rstd, dm, dr)
    chunks = (H * W + 255) // 256
    y, stats, ws = Guarded(ref.numel(), torch.float16), Guarded(N * 64), Guarded(N * 64 * chunks)
    rc = L.pdhip_groupnorm_nhwc_f16(_ptr(x), _ptr(gamma), _ptr(beta), _ptr(fm), N, H, W, Cc, 1, 0, _ptr(y.t), _ptr(stats.t), _ptr(ws.t), N * 64 * chunks,
                                    _stream())
    assert rc == 0, L.pdhip_last_error()
    torch.cuda.synchronize()
    assert y.intact() and stats.intact() and ws.intact()
    rs = _stats_check(stats.t, mean, rstd, dm, dr, "statistics")
    got = y.t.reshape(ref.shape)
    r_tail = _check(got.reshape(N, H * W, Cc)[:, -7:], ref.reshape(N, H * W, Cc)[:, -7:], bound.reshape(N, H * W, Cc)[:, -7:], "the last workgroup's 7 pixels")
    r_all = _check(got, ref, bound, "all pixels")
    note_measured(test='nn_ops_groupnorm_unrolled', film=fl, ratio=r_all, ratio_tail=r_tail, ratio_stats=rs)


# ================================================================================================ k_gn_table
@pytest.mark.parametrize("fl", [0, 1])
@pytest.mark.parametrize("Cc", [32, 160, 2048])
def test_gn_table_vs_f64(L, Cc, fl):
    N = 3
    _, gamma, beta, film = _dev(*oc.gn_inputs(N, 2, 2, Cc))
    g = torch.Generator().manual_seed(Cc)
    stats = torch.stack([torch.randn((N, 32), generator=g), 0.5 + 1.5 * torch.rand((N, 32), generator=g)], dim=-1).to(DEV).contiguous()
    fm = film if fl else None
    A, B, dA, dB = oc.gn_table_ref(stats, gamma, beta, fm, Cc)
    table = Guarded(N * Cc * 2)
    assert L.pdhip_gn_table_f32(_ptr(stats), _ptr(gamma), _ptr(beta), _ptr(fm), 2 * Cc, N, Cc, _ptr(table.t), _stream()) == 0, L.pdhip_last_error()
    torch.cuda.synchronize()
    assert table.intact()
    a, b = oc.table_columns(table.t, N, Cc)
    ra, rb = _check(a, A, dA, f"A C={Cc} film={fl}"), _check(b, B, dB, f"B C={Cc} film={fl}")
    note_measured(test='nn_ops_gn_table', C=Cc, film=fl, ratio_A=ra, ratio_B=rb)


# ================================================================================================ k_resample, k_concat: copies and one rounding -- bit-equal
def _pool_as_the_kernel_rounds(x):
    """f16 of the f32 sum of the four pixels in row-major order, times 0.25 (k_resample)."""
    f = x.float()
    return ((((f[:, 0::2, 0::2] + f[:, 0::2, 1::2]) + f[:, 1::2, 0::2]) + f[:, 1::2, 1::2]) * 0.25).half()


def _bits(t):
    return t.contiguous().view(torch.int16)


@pytest.mark.parametrize("Ca,Cb", oc.CONCAT_SPLITS)
@pytest.mark.parametrize("N,H,W", oc.RESAMPLE_SHAPES)
def test_resample_and_concat_are_bit_equal_to_torch(L, N, H, W, Ca, Cb):
    Cc = Ca + Cb
    g = torch.Generator().manual_seed(N * 1000 + H * 10 + W + Cc)
    x = (torch.randn((N, H, W, Cc), generator=g) * 3).half().to(DEV)
    nchw = x.permute(0, 3, 1, 2).float()
    want = {1: _pool_as_the_kernel_rounds(x), 2: F.interpolate(nchw, scale_factor=2, mode='nearest').permute(0, 2, 3, 1).half()}
    assert (want[1].double() - F.avg_pool2d(nchw.double(), 2).permute(0, 2, 3, 1)).abs().max() <= float(oc.ulp16(x.double()).max())
    for mode in (1, 2):
        y = Guarded(want[mode].numel(), torch.float16)
        assert L.pdhip_resample2x_nhwc_f16(_ptr(x), N, H, W, Cc, mode, _ptr(y.t), _stream()) == 0, L.pdhip_last_error()
        torch.cuda.synchronize()
        assert y.intact() and torch.equal(_bits(y.t.reshape(want[mode].shape)), _bits(want[mode])), f"mode {mode}"
    a, b = x[..., :Ca].contiguous(), x[..., Ca:].contiguous()
    y = Guarded(x.numel(), torch.float16)
    assert L.pdhip_concat_channels_f16(_ptr(a), Ca, _ptr(b), Cb, N * H * W, _ptr(y.t), _stream()) == 0, L.pdhip_last_error()
    torch.cuda.synchronize()
    assert y.intact() and torch.equal(_bits(y.t.reshape(x.shape)), _bits(torch.cat([a, b], dim=-1)))


@pytest.mark.parametrize("mode", [1, 2])
def test_resample_beyond_the_grid_cap(L, mode):
    """4096 x 4098 output pixels of one octet = 16 785 408 octets against 65 536 x 256 = 16 777 216 threads: the last 8 192 are written on the second trip of
    the grid-stride loop.  Compared in full on the device."""
    Ho, Wo, Cc = 4096, 4098, 8
    assert 0 < Ho * Wo * (Cc // 8) - oc.GRID_CAP_OCTETS <= 8192
    H, W = (2 * Ho, 2 * Wo) if mode == 1 else (Ho // 2, Wo // 2)
    g = torch.Generator(device=DEV).manual_seed(mode)
    x = (torch.randn((1, H, W, Cc), generator=g, device=DEV) * 3).half()
    want = _pool_as_the_kernel_rounds(x) if mode == 1 else x.repeat_interleave(2, dim=1).repeat_interleave(2, dim=2)
    y = Guarded(Ho * Wo * Cc, torch.float16)
    assert L.pdhip_resample2x_nhwc_f16(_ptr(x), 1, H, W, Cc, mode, _ptr(y.t), _stream()) == 0, L.pdhip_last_error()
    torch.cuda.synchronize()
    assert y.intact()
    got = y.t.reshape(want.shape)
    assert torch.equal(_bits(got).reshape(-1)[-8192 * 8:], _bits(want).reshape(-1)[-8192 * 8:]), "the second trip of the stride loop"
    assert torch.equal(_bits(got), _bits(want))


def test_concat_beyond_the_grid_cap(L):
    """8 388 708 pixels of 8 + 8 channels = 16 777 416 octets: 200 beyond one trip of the 65 536-workgroup grid."""
    P, Ca, Cb = 8388708, 8, 8
    assert 0 < P * 2 - oc.GRID_CAP_OCTETS <= 256
    g = torch.Generator(device=DEV).manual_seed(3)
    a, b = (torch.randn((P, c), generator=g, device=DEV).half() for c in (Ca, Cb))
    y = Guarded(P * (Ca + Cb), torch.float16)
    assert L.pdhip_concat_channels_f16(_ptr(a), Ca, _ptr(b), Cb, P, _ptr(y.t), _stream()) == 0, L.pdhip_last_error()
    torch.cuda.synchronize()
    assert y.intact() and torch.equal(_bits(y.t.reshape(P, Ca + Cb)), _bits(torch.cat([a, b], dim=-1)))
