"""The in_layers conv of the up-ResBlocks, conv3x3(nearest_x2(h)) (unet.py:190-192, 236-242), as four 2x2 phase convs over the half-resolution h
(csrc/nn_gemm.hip k_conv_igemm<4>): the load-time weight table bit for bit, the layer alone at the five up-block shapes
against a float64 CPU convolution, and the whole UNet under pdhip_debug_set_up_phase 0 / 1 / 2."""
import ctypes as C
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import load_golden, note_measured, U1_FP32_LINF, U1_FP32_L2, U1_ROUTE_LINF, U1_ROUTE_L2
from oracle import unet as ounet

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
TAPS_OF = {(0, 0): (0,), (0, 1): (1, 2), (1, 0): (0, 1), (1, 1): (2,)}      # (output phase, source tap) -> 3x3 taps, per axis


@pytest.fixture(scope="module")
def nn():
    assert torch.cuda.is_available()
    from pointdreamer_amd import _lib
    import pointdreamer_amd.ddnm_inpainting as di
    return dict(L=_lib.lib(), lib=_lib, di=di)


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _pack9(L, w_oihw, pad):
    """f32 OIHW on the device -> the engine's [pad][9 Cin] f16 layout (rows >= Cout zero)."""
    co, ci = w_oihw.shape[:2]
    w9 = torch.zeros((pad, 9 * ci), dtype=torch.float16, device=DEV)
    assert L.pdhip_pack_conv_weight_f16(_ptr(w_oihw.contiguous()), co, ci, 9, _ptr(w9), None) == 0
    return w9


def test_phase_weight_table_is_f16_of_the_f32_sum_of_f16_taps(nn):
    """pdhip_pack_conv_up2_phase_f16 against a host restatement: entry (phase, o, tap, c) = f16( sum in (ky, kx) order, in f32, of the f16-rounded 3x3
    taps that land on source tap (ty, tx) ) -- bit for bit, padded rows zero."""
    L = nn['L']
    co, ci, pad = 72, 64, 128
    g = torch.Generator().manual_seed(5)
    w = torch.randn((co, ci, 3, 3), generator=g) * 0.05
    w9 = _pack9(L, w.to(DEV), pad)
    wph = torch.full((4, pad, 4 * ci), 7.0, dtype=torch.float16, device=DEV)
    assert L.pdhip_pack_conv_up2_phase_f16(_ptr(w9), ci, pad, _ptr(wph), None) == 0, L.pdhip_last_error()
    torch.cuda.synchronize()
    w16 = w.half().float().numpy()                       # the f16-rounded originals, exactly representable in f32
    want = np.zeros((4, pad, 4, ci), dtype=np.float16)
    for py in range(2):
        for px in range(2):
            for ty in range(2):
                for tx in range(2):
                    acc = np.zeros((co, ci), dtype=np.float32)
                    for ky in TAPS_OF[(py, ty)]:
                        for kx in TAPS_OF[(px, tx)]:
                            acc = (acc + w16[:, :, ky, kx]).astype(np.float32)
                    want[2 * py + px, :co, 2 * ty + tx, :] = acc.astype(np.float16)
    got = wph.cpu().numpy().reshape(4, pad, 4, ci)
    assert np.array_equal(got.view(np.uint16), want.view(np.uint16))


# (half-resolution size, Cin, Cout): the in_layers conv of the five up-ResBlocks of the 256^2 model (-> 256^2, 128^2, 64^2, 32^2, 16^2)
UP_LAYERS = [(128, 256, 256), (64, 512, 512), (32, 512, 512), (16, 1024, 1024), (8, 1024, 1024)]


@pytest.mark.parametrize("N", [1, 8])
@pytest.mark.parametrize("hs,cin,cout", UP_LAYERS)
def test_up2_phase_layer_vs_f64_conv(nn, hs, cin, cout, N):
    """The layer alone: the phase entry and the route it replaces (9 taps per up-sampled pixel: the halo kernel's index arithmetic where that kernel
    takes the layer unsplit, else the materialised x2 tensor through pdhip_conv2d_nhwc_f16) against a float64 CPU conv3x3(nearest_x2(x)) of the
    UN-combined f16 weights.  The phase route rounds each combined weight to f16 once more -- an error of the size of the output's own f16 rounding --
    so its error variance at most doubles: err_new <= 2 err_old (sqrt(2) expected).
    Measured (MI355X, relative L2 against the f64 conv): old route 2.07e-4, phase route 2.92e-4, ratio 1.41 at all ten cases (profiles/up_phase_headline.txt)."""
    L = nn['L']
    g = torch.Generator().manual_seed(hs * 7 + N)
    x = torch.randn((N, hs, hs, cin), generator=g).half()
    w = (torch.randn((cout, cin, 3, 3), generator=g) * 0.05).half()
    b = (torch.randn((cout,), generator=g) * 0.1).half().float()
    pad = (cout + 127) // 128 * 128
    xd, bd = x.to(DEV), b.to(DEV)
    w9 = _pack9(L, w.float().to(DEV), pad)
    wph = torch.empty((4, pad, 4 * cin), dtype=torch.float16, device=DEV)
    assert L.pdhip_pack_conv_up2_phase_f16(_ptr(w9), cin, pad, _ptr(wph), None) == 0
    zp = torch.zeros(128, dtype=torch.float16, device=DEV)
    H2 = 2 * hs
    y_new = torch.full((N, H2, H2, cout), float('nan'), dtype=torch.float16, device=DEV)
    y_old = torch.full((N, H2, H2, cout), float('nan'), dtype=torch.float16, device=DEV)
    chunks = 4 * hs * hs // 256
    part = torch.zeros((N, max(chunks, 1), cout // 8, 2), device=DEV) if (hs * hs) % 256 == 0 else None
    assert L.pdhip_conv3x3_up2_phase_nhwc_f16(_ptr(xd), _ptr(wph), _ptr(bd), _ptr(y_new), N, hs, hs, cin, cout, pad, _ptr(zp), _ptr(part), None) == 0, \
        L.pdhip_last_error()
    rc = L.pdhip_conv3x3_up2_halo_nhwc_f16(_ptr(xd), _ptr(w9), _ptr(bd), _ptr(y_old), N, hs, hs, cin, cout, pad, _ptr(zp), None)
    old_route = 'halo in_up'
    if rc != 0:                                          # not a layer the halo kernel takes unsplit: the engine's other form, x2 pass + 9-tap conv
        old_route = 'x2 tensor + conv2d'
        xu = xd.repeat_interleave(2, dim=1).repeat_interleave(2, dim=2).contiguous()
        assert L.pdhip_conv2d_nhwc_f16(_ptr(xu), _ptr(w9), _ptr(bd), None, _ptr(y_old), N, H2, H2, cin, cout, pad, 9, _ptr(zp), None) == 0, L.pdhip_last_error()
    torch.cuda.synchronize()
    torch.set_num_threads(min(16, max(1, torch.get_num_threads())))
    xu64 = x.double().permute(0, 3, 1, 2).repeat_interleave(2, dim=2).repeat_interleave(2, dim=3)
    ref = F.conv2d(xu64, w.double(), b.double(), padding=1).permute(0, 2, 3, 1)
    nrm = ref.norm().item()
    err_new = (y_new.cpu().double() - ref).norm().item() / nrm
    err_old = (y_old.cpu().double() - ref).norm().item() / nrm
    print(f"up2 layer {hs}^2 -> {H2}^2, {cin} -> {cout}, N {N}: rel L2 vs f64 conv: old ({old_route}) {err_old:.3e}, phase {err_new:.3e}, ratio {err_new / err_old:.3f}")
    note_measured(test='up2_phase_layer', hs=hs, cin=cin, cout=cout, N=N, old_route=old_route, err_old=err_old, err_new=err_new)
    assert np.isfinite(err_new) and np.isfinite(err_old) and err_old > 0
    assert err_new <= 2.0 * err_old, (hs, cin, cout, N, err_old, err_new)
    if part is not None:                                 # the fused GroupNorm octet partials are the sums of the f16 output just written
        yv = y_new.float().view(N, hs, 2, hs, 2, cout // 8, 8)
        s_all = yv.sum(dim=(1, 2, 3, 4, 6)).double().cpu()
        q_all = (yv * yv).sum(dim=(1, 2, 3, 4, 6)).double().cpu()
        ps = part.double().cpu().sum(dim=1)
        assert torch.allclose(ps[..., 0], s_all, rtol=1e-3, atol=1e-2 * float(q_all.max().sqrt()))
        assert torch.allclose(ps[..., 1], q_all, rtol=1e-3)


@pytest.fixture(scope="module")
def full_model32(nn):
    cfg = ounet.make_config(256, 256, 2, "32,16,8", 64, True)
    w = ounet.random_weights(cfg, 12)
    m = nn['di'].UNetModel(max_batch=32, device=DEV, **nn['di'].IMAGENET_256)
    m.load_state_dict(w, strict=True)
    del w
    return m


def _rel(a, b):
    a, b = a.double(), b.double()
    return ((a - b).abs().max() / b.abs().max()).item(), ((a - b).norm() / b.norm()).item()


@pytest.mark.parametrize("N", [1, 8, 32])
def test_unet_full_up_phase_hook_0_1_2(nn, full_model32, N):
    """Whole 256^2 UNet with the hook at 0 (never), 1 (automatic), 2 (every eligible layer): each against the reference's fp32 golden inside the
    U1 bounds, hook 1 / 2 against hook 0 inside the routing-variant bounds, repeats bit-identical, and at batch 32 -- where bench.py runs -- the
    automatic routing really takes the phase conv."""
    L = nn['L']
    g = load_golden('unet_full.npz')
    x = torch.from_numpy(g['x']).to(DEV).repeat(N, 1, 1, 1).contiguous()
    t = torch.from_numpy(g['t']).to(DEV).repeat(N).contiguous()
    st = int(g['stride'])
    ref = torch.from_numpy(g['ref_out'])
    outs = {}
    for mode in (0, 1, 2):
        old = L.pdhip_debug_set_up_phase(mode)
        try:
            outs[mode] = full_model32(x, t).cpu()
            again = full_model32(x, t).cpu()
        finally:
            L.pdhip_debug_set_up_phase(old)
        assert torch.equal(outs[mode], again), (N, mode)
        worst = [0.0, 0.0]
        for b in range(N):
            linf, l2 = _rel(outs[mode][b:b + 1, :, ::st, ::st], ref)
            worst = [max(worst[0], linf), max(worst[1], l2)]
            assert linf <= U1_FP32_LINF and l2 <= U1_FP32_L2, (N, mode, b, linf, l2)
        note_measured(test='unet_full_fp32_up_phase', batch=N, mode=mode, linf=worst[0], l2=worst[1])
        print(f"UNet batch {N}, up_phase {mode}: vs fp32 golden rel L-inf {worst[0]:.3e}, rel L2 {worst[1]:.3e}")
    for mode in (1, 2):
        linf, l2 = _rel(outs[mode], outs[0])
        note_measured(test='unet_full_up_phase_vs_off', batch=N, mode=mode, linf=linf, l2=l2)
        print(f"UNet batch {N}, up_phase {mode} vs 0: rel L-inf {linf:.3e}, rel L2 {l2:.3e}")
        assert linf <= U1_ROUTE_LINF and l2 <= U1_ROUTE_L2, (N, mode, linf, l2)
    assert not torch.equal(outs[2], outs[0]), "hook 2 takes the phase conv somewhere at every batch"
    if N == 32:
        assert not torch.equal(outs[1], outs[0]), "the automatic routing takes the phase conv at the benchmark's batch"
