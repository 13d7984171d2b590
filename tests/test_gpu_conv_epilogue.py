"""GPU: the GroupNorm octet partials every conv epilogue leaves, and the two kernels that consume them, one launch at a time.

Producers, through pdhip_debug_conv_launch_nhwc_f16 (conv_plan + conv_launch with every operand, routed by the debug hooks): k_conv_igemm's direct
epilogue in its four tile geometries, k_splitk_reduce behind the split implicit GEMM and the split halo kernel, the halo-resident kernel's direct epilogue
(row tiles and 128-column strips), k_conv_sk in its four tiles with and without in-launch split-K, and k_conv_sk<10> (skip 1x1 appended).  y is compared
with a float64 convolution of the same f16 operands under the suite's single-kernel bound; the partials with float64 sums over the f16 y the launch wrote
under the derived f32 summation bound of tests/conv_epilogue_common.py (whose teeth tests/test_conv_epilogue_cpu.py proves).

Consumers: k_gn_finalize_oct (pdhip_gn_finalize_oct_f32) against float64 group statistics under the bound propagated from the partials, and the chain
launch -> partials -> finalize / GroupNorm-apply with in-kernel statistics."""
import ctypes as C
import pytest
import torch
import torch.nn.functional as F

import conv_epilogue_common as ce
import conv_tail_common as ct
from conv_tail_common import DEV, GUARD, TAIL, _nhwc, _pack, _ptr, _stream

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def L():
    assert torch.cuda.is_available()
    from pointdreamer_amd import _lib
    import pointdreamer_amd.ddnm_inpainting  # noqa: F401  (registers the entry points)
    return _lib.lib()


def launch(L, c, op, x2_split=0, res_up=False, want_gn=True):
    """One pdhip_debug_conv_launch_nhwc_f16 under the hooks of case c.  Returns (y [N,H,W,Cout] f16 on the device, partials or None, chunks, kernel)."""
    N, H, W, Cin, Cout, taps = c['N'], c['H'], c['W'], c['Cin'], c['Cout'], c['taps']
    pad = (Cout + 127) // 128 * 128
    x = _nhwc(op['x'])
    xa, xb = (x[..., :x2_split].contiguous(), x[..., x2_split:].contiguous()) if x2_split else (x, None)
    wp, bias = _pack(L, op['w']), op['b']
    xs = xs2 = None
    if c['Cs']:                    # [Cout_pad][9 Cin + Cs]: the packed 3x3 rows followed by the packed 1x1 rows; the biases summed
        wp = torch.cat([wp, _pack(L, op['ws'])], dim=1).contiguous()
        bias = op['b'] + op['bs']
        xs = _nhwc(op['xs'])
        if c['Cs1']:
            xs, xs2 = xs[..., :c['Cs1']].contiguous(), xs[..., c['Cs1']:].contiguous()
    bd = bias.float().to(DEV)
    r = _nhwc(op['r']) if 'r' in op else None
    y = torch.full((N, H, W, Cout), float('nan'), dtype=torch.float16, device=DEV)
    zp = torch.zeros((128,), dtype=torch.float16, device=DEV)
    wsf = ce.workspace_floats(c)
    ws = torch.zeros((wsf,), device=DEV) if wsf else None
    need = N * c['chunks'] * (Cout // 8) * 2
    gp = None
    if want_gn:
        gp = torch.full((need + TAIL,), float('nan'), device=DEV)
        gp.view(torch.int32)[need:] = GUARD
    k, ch = C.c_int(-1), C.c_int(-1)
    with ce.Hooks(L, c):
        rc = L.pdhip_debug_conv_launch_nhwc_f16(_ptr(xa), _ptr(xb), x2_split, _ptr(wp), _ptr(bd), _ptr(r), 1 if res_up else 0, _ptr(xs), _ptr(xs2), c['Cs1'], c['Cs'],
                                                _ptr(y), N, H, W, Cin, Cout, pad, taps, _ptr(zp), _ptr(ws), wsf, _ptr(gp), need, C.byref(ch), C.byref(k), _stream())
    assert rc == 0, L.pdhip_last_error()
    torch.cuda.synchronize()
    if want_gn:
        assert (gp.view(torch.int32)[need:] == GUARD).all(), "the launch wrote behind its partials"
    return y, (gp[:need] if want_gn else None), ch.value, k.value


def check_y(y, op):
    ref = ce.reference_f64(op)
    err = (y.double().cpu() - ref).abs().max().item()
    print(f"  y: max err {err:.3e}, bound {2e-3 * ref.abs().max().item() + 1e-3:.3e}")
    assert err <= 2e-3 * ref.abs().max().item() + 1e-3


@pytest.mark.parametrize("c", ce.CASES, ids=[c['name'] for c in ce.CASES])
def test_conv_epilogue_partials(L, c):
    op = ce.make_operands(c['N'], c['H'], c['W'], c['Cin'], c['Cout'], c['taps'], c['res'], 1000 + ce.CASES.index(c), Cs=c['Cs'])
    y, part, chunks, kernel = launch(L, c, op)
    assert kernel == ce.KERNELS[c['kernel']], f"routed to kernel {kernel}"
    assert chunks == c['chunks'], f"{chunks} chunks per image, the kernel documents {c['chunks']}"
    check_y(y, op)
    if c['chunks'] == 0:
        return                     # (no partials for this geometry: the guard check covered every float of the buffer)
    errs = ce.partials_errors(part, y, chunks, contiguous=c['contiguous'])
    assert errs == [], errs


@pytest.mark.parametrize("c", ce.TAIL_CASES, ids=[c['name'] for c in ce.TAIL_CASES])
def test_conv_epilogue_partials_of_the_other_entries(L, c):
    """k_conv_ht, k_conv_rr and the four-phase up conv (tests/conv_tail_common.py launches them): the same checks as above."""
    op = ct.operands(c)
    y, part, chunks, kernel = ct.prepare(L, c, op)()
    assert kernel == ce.KERNELS[c['kernel']], f"routed to kernel {kernel}"
    assert chunks == c['chunks'], f"{chunks} chunks per image, the kernel documents {c['chunks']}"
    ref = ct.reference_f64(c, op)
    err = (y.double().cpu() - ref).abs().max().item()
    print(f"  y: max err {err:.3e}, bound {2e-3 * ref.abs().max().item() + 1e-3:.3e}")
    assert err <= 2e-3 * ref.abs().max().item() + 1e-3
    if c['entry'] == 'phase':      # chunk 4 t + p = the pixels of parity p = (py, px) of the t-th run of 256 half-resolution pixels: gathered, then as everywhere
        N, H, W, Cc = y.shape
        yp = y.reshape(N, H // 2, 2, W // 2, 2, Cc).permute(0, 1, 3, 2, 4, 5).reshape(N, chunks // 4, 256, 4, Cc).permute(0, 1, 3, 2, 4)
        errs = ce.partials_errors(part, yp.reshape(N, H * W, Cc), chunks)
    else:
        errs = ce.partials_errors(part, y, chunks, contiguous=c['contiguous'])
    assert errs == [], errs


# ---- operands only the network reached so far
@pytest.mark.parametrize("kernel", ['igemm', 'sk'])
@pytest.mark.parametrize("Cin1,Cin", [(64, 192), (512, 768)])
def test_two_source_1x1_equals_the_materialised_concat(L, kernel, Cin1, Cin):
    c = ce._case(f"two-source-{kernel}", kernel, 2, 16, 16, Cin, 136, taps=1, tile=2 if kernel == 'igemm' else 0, sk=(2, 3, 1) if kernel == 'sk' else (1, 0, 0),
                 chunks=2 if kernel == 'igemm' else 4)
    op = ce.make_operands(2, 16, 16, Cin, 136, 1, True, Cin + Cin1)
    y1, p1, ch1, k1 = launch(L, c, op)
    y2, p2, ch2, k2 = launch(L, c, op, x2_split=Cin1)
    assert k1 == k2 == ce.KERNELS[kernel] and ch1 == ch2 == c['chunks']
    assert torch.equal(y1, y2) and torch.equal(p1, p2)
    check_y(y2, op)
    assert ce.partials_errors(p2, y2, ch2) == []


def test_res_up_on_sk_equals_the_materialised_residual(L):
    for t, sp in ((1, 1), (3, 3)):
        c = ce._case("res-up-sk", 'sk', 2, 16, 16, 128, 136, sk=(2, t, sp), chunks=256 // (128 if t == 1 else 64))
        op = ce.make_operands(2, 16, 16, 128, 136, 9, True, 77 + t, res_hw=(8, 8))
        full = dict(op, r=F.interpolate(op['r'], scale_factor=2, mode='nearest'))
        y1, p1, ch1, k1 = launch(L, c, full)
        y2, p2, ch2, k2 = launch(L, c, op, res_up=True)
        assert k1 == k2 == ce.KERNELS['sk'] and ch1 == ch2 == c['chunks']
        assert torch.equal(y1, y2) and torch.equal(p1, p2)
        check_y(y2, op)
        assert ce.partials_errors(p2, y2, ch2) == []


def test_res_up_on_the_halo_kernel_equals_the_materialised_residual(L):
    """The halo-resident kernel reads a half-resolution residual only where it runs unsplit by the automatic routing: >= 256 tiles of 512 pixels x 128
    channels.  4 x 128x128 pixels x 136 (-> 256 padded) channels is the smallest such layer; Cin 32 keeps it at 5 GFLOP.  Bit-identity with the
    materialised residual is the check (a float64 convolution of this size belongs to no unit test); the partials are checked as everywhere."""
    c = ce._case("res-up-halo", 'halo', 4, 128, 128, 32, 136, chunks=32)
    op = ce.make_operands(4, 128, 128, 32, 136, 9, True, 99, res_hw=(64, 64))
    full = dict(op, r=F.interpolate(op['r'], scale_factor=2, mode='nearest'))
    y1, p1, ch1, k1 = launch(L, c, full)
    y2, p2, ch2, k2 = launch(L, c, op, res_up=True)
    assert k1 == k2 == ce.KERNELS['halo'] and ch1 == ch2 == 32
    assert torch.equal(y1, y2) and torch.equal(p1, p2)
    assert ce.partials_errors(p2, y2, ch2) == []
    # one image's corner against float64, the residual index included
    ref = ce.reference_f64(dict(x=op['x'][3:, :, :10, :10], w=op['w'], b=op['b'], r=op['r'][3:, :, :5, :5]))[0, :8, :8]
    assert (y2[3, :8, :8].double().cpu() - ref).abs().max().item() <= 2e-3 * ref.abs().max().item() + 1e-3


# ---- consumers
def _octet_partials(L, t, chunks):
    N, HW, Cc = t.shape
    p = torch.full((N * chunks * (Cc // 8) * 2,), float('nan'), device=DEV)
    assert L.pdhip_gn_octet_partials_f16(_ptr(t), N, HW, Cc, chunks, _ptr(p), _stream()) == 0, L.pdhip_last_error()
    return p


def _finalize(L, parts, Cs, chunks, N, HW):
    stats = torch.full((N * 64 + 64,), float('nan'), device=DEV)
    stats.view(torch.int32)[N * 64:] = GUARD
    pb, Cb, chb = (parts[1], Cs[1], chunks[1]) if len(parts) == 2 else (None, 0, 0)
    rc = L.pdhip_gn_finalize_oct_f32(_ptr(parts[0]), Cs[0], chunks[0], _ptr(pb), Cb, chb, N, HW, _ptr(stats), _stream())
    assert rc == 0, L.pdhip_last_error()
    torch.cuda.synchronize()
    assert (stats.view(torch.int32)[N * 64:] == GUARD).all()
    return stats[:N * 64]


def _tensor(N, HW, Cc, seed):
    """[N, HW, Cc] f16 with an offset and a scale of its own per image and per channel block of 8 (so per group, and per octet inside a group)."""
    g = torch.Generator().manual_seed(seed)
    off = torch.randn((N, 1, Cc // 8, 1), generator=g) * 2 + torch.arange(N).float()[:, None, None, None]
    sc = 0.25 + torch.rand((N, 1, Cc // 8, 1), generator=g) * (1 + torch.arange(N).float()[:, None, None, None])
    return (torch.randn((N, HW, Cc // 8, 8), generator=g) * sc + off).reshape(N, HW, Cc).half().to(DEV)


@pytest.mark.parametrize("N,HW,Cs,chunks", [
    (3, 64, (256,), (4,)),                    # 8 channels per group: one octet each
    (3, 64, (1024,), (1,)),
    (2, 320, (256,), (40,)),                  # more chunks than the 32 slices of the kernel, and no multiple of them
    (3, 64, (1024, 512), (1, 4)),             # 48 per group: group 21 straddles A | B, the sources are chunked differently
    (3, 64, (512, 256), (16, 4)),             # 24 per group: group 21 again (octets 63 | 64)
    (3, 256, (256, 256), (64, 16)),
])
def test_gn_finalize_oct_vs_float64(L, N, HW, Cs, chunks):
    ts = [_tensor(N, HW, Cc, 11 * Cc + i) for i, Cc in enumerate(Cs)]
    parts = [_octet_partials(L, t, ch) for t, ch in zip(ts, chunks)]
    stats = _finalize(L, parts, Cs, chunks, N, HW)
    errs = ce.stats_errors(stats, ts, chunks)
    assert errs == [], errs


def test_gn_finalize_oct_offset_case_against_the_derived_bound_and_the_statistics_kernel(L):
    """Group mean 8, standard deviation 0.25 (E[x^2] = 64.06: the variance is the small difference of two large numbers).  The bound on rstd comes from the
    data (conv_epilogue_common.stats_bounds: 16-pixel chunks, n = 128 per slot).  The stand-alone statistics kernel (stats_ws of pdhip_groupnorm_nhwc_f16)
    on the same tensor must hold the same bound, and the partials' result may be no further from float64 than that kernel's plus the bound."""
    N, H, W, Cc, chunks = 2, 16, 16, 256, 16
    g = torch.Generator().manual_seed(8)
    x = (8 + 0.25 * torch.randn((N, H * W, Cc), generator=g)).half().to(DEV)
    parts = [_octet_partials(L, x, chunks)]
    stats = _finalize(L, parts, (Cc,), (chunks,), N, H * W)
    errs = ce.stats_errors(stats, [x], (chunks,))
    assert errs == [], errs
    y = torch.empty_like(x)
    sa = torch.empty((N * 64,), device=DEV)
    ws = torch.empty((N * 64 * ((H * W + 255) // 256),), device=DEV)
    gamma, beta = torch.ones((Cc,), device=DEV), torch.zeros((Cc,), device=DEV)
    rc = L.pdhip_groupnorm_nhwc_f16(_ptr(x), _ptr(gamma), _ptr(beta), None, N, H, W, Cc, 0, 0, _ptr(y), _ptr(sa), _ptr(ws), ws.numel(), _stream())
    assert rc == 0, L.pdhip_last_error()
    torch.cuda.synchronize()
    errs = ce.stats_errors(sa, [x], (chunks,))
    assert errs == [], errs
    mean, rstd = ce.group_stats([x])
    _, br = ce.stats_bounds([x], (chunks,))
    e_fin = (stats.reshape(N, 32, 2)[..., 1].double().cpu() - rstd).abs()
    e_alone = (sa.reshape(N, 32, 2)[..., 1].double().cpu() - rstd).abs()
    print(f"  rstd ~ {rstd.mean():.4f}: finalize err {e_fin.max():.3e}, stand-alone err {e_alone.max():.3e}, bound {br.min():.3e} .. {br.max():.3e}")
    assert (e_fin <= e_alone + br).all()


@pytest.mark.parametrize("kernel", ['sk', 'igemm'])
def test_partials_of_a_launch_through_both_consumers(L, kernel):
    """launch -> octet partials -> k_gn_finalize_oct: within the derived bound of the float64 statistics of the launch's y; the same partials ->
    GroupNorm-apply with in-kernel statistics: within the suite's GroupNorm bound of F.group_norm on y."""
    N, H, W, Cout = 3, 16, 16, 256
    c = ce._case(f"chain-{kernel}", kernel, N, H, W, 128, Cout, tile=2 if kernel == 'igemm' else 0, sk=(2, 2, 3) if kernel == 'sk' else (1, 0, 0), chunks=2)
    op = ce.make_operands(N, H, W, 128, Cout, 9, True, 321)
    y, part, chunks, k = launch(L, c, op)
    assert k == ce.KERNELS[kernel] and chunks == 2
    assert ce.partials_errors(part, y, chunks) == []
    yt = y.reshape(N, H * W, Cout)
    stats = _finalize(L, [part], (Cout,), (chunks,), N, H * W)
    errs = ce.stats_errors(stats, [yt], (chunks,))
    assert errs == [], errs
    g = torch.Generator().manual_seed(5)
    gamma, beta = (1 + 0.1 * torch.randn((Cout,), generator=g)), 0.1 * torch.randn((Cout,), generator=g)
    gd, bd = gamma.to(DEV), beta.to(DEV)
    out = torch.empty_like(y)
    rc = L.pdhip_gn_apply_parts_f16(_ptr(y), None, Cout, Cout, _ptr(part), chunks, None, 0, _ptr(gd), _ptr(bd), None, 2 * Cout, N, H, W, 0, _ptr(out), _stream())
    assert rc == 0, L.pdhip_last_error()
    torch.cuda.synchronize()
    ref = F.group_norm(y.float().cpu().permute(0, 3, 1, 2), 32, gamma, beta, eps=1e-5).permute(0, 2, 3, 1)
    assert (out.float().cpu() - ref).abs().max().item() <= 6e-3 * max(1.0, ref.abs().max().item())
