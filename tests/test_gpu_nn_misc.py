"""GPU: the UNet's f32 side ops and the DDNM step (csrc/nn_misc.hip), one operator at a time against float64 references under derived bounds.

The references and bounds live in tests/nn_misc_common.py (tests/test_nn_misc_cpu.py shows that an honest f32 evaluation passes them and that the bugs
looked for here do not).  Every output buffer starts as NaN and is followed by a guard band that must come back untouched; every test records its largest
error / bound ratio with note_measured -- a ratio near 1 would mean a derivation is wrong, not that a bound needs widening.

Noise streams: the sampler draws x_T from Philox stream 0 and the noise of step k from stream k + 1 (csrc/nn_unet.hip, pdhip_ddnm_sample_keyed), so the
stream that pdhip_ddnm_step(eps = NULL, step = k) must reproduce bit for bit is pdhip_philox_normal(stream_id = k + 1)."""
import ctypes as C
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import nn_misc_common as nm
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


@pytest.fixture(scope="module")
def coefs():
    import pointdreamer_amd.ddnm_inpainting as di
    return di.ddnm_schedule()[4]             # [100][6] f32: sqrt(1 - a_t), sqrt(a_t), sqrt(a_next), sigma_t, c1, c2


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


class Guarded:
    """n elements of NaN (f32 / f16) followed by TAIL elements of a guard pattern, in one allocation."""

    def __init__(self, n, dtype=torch.float32, fill=float('nan')):
        self.n, self.pattern = n, GUARD32 if dtype == torch.float32 else GUARD16
        itype = torch.int32 if dtype == torch.float32 else torch.int16
        self.raw = torch.full((n + TAIL,), self.pattern, dtype=itype, device=DEV)
        self.t = self.raw.view(dtype)[:n]
        if fill is not None:
            self.t.fill_(fill)

    def intact(self):
        return bool((self.raw[self.n:] == self.pattern).all())


def _ratio(err, bound):
    return float((err / bound).max())


# ================================================================================================ a. GEMV
def _gemv_inputs(R, K, N, big=False):
    g = torch.Generator().manual_seed(R * 1000003 + K * 101 + N)
    W = torch.randn((R, K), generator=g) / math.sqrt(K)
    b = torch.linspace(-100.0, 100.0, R) if big else torch.randn((R,), generator=g)
    x = torch.randn((N, K), generator=g)           # every row differs: a batch-slot mix-up shows
    return W, b, x


def _run_gemv(L, W, b, x, silu):
    R, K = W.shape
    N = x.shape[0]
    y = Guarded(N * R)
    Wd, bd, xd = W.to(DEV), b.to(DEV), x.to(DEV)
    rc = L.pdhip_gemv_rows_f32(_ptr(Wd), _ptr(bd), _ptr(xd), _ptr(y.t), R, K, N, silu, _stream())
    assert rc == 0, L.pdhip_last_error()
    torch.cuda.synchronize()
    assert y.intact(), "the floats behind y were written"
    return y.t.cpu().reshape(N, R)


# Between them: K 32 / 100 / 128 (generic loop, 100 no multiple of 64), 256 / 512 / 1024 (the three specialisations); R 1, 3 (clamped rows of a 4-row group),
# 4, 127 / 129 / 130 (a wave's 32-row slice ends inside / one past / two past a group), 128 (a full block), 515 (five blocks, the last with 3 rows);
# N 1, 7, 8, 9, 16, 20 (passes of 8 with and without a zeroed tail), 100 (13 passes, the last holding 4: the sampler's call).
GEMV_CASES = [(1, 32, 1, 0), (3, 100, 7, 1), (4, 128, 8, 0), (127, 256, 9, 1), (128, 512, 16, 0), (129, 1024, 20, 1), (130, 100, 100, 0),
              (515, 256, 100, 1), (130, 1024, 7, 0), (515, 512, 9, 1), (4, 32, 16, 1), (129, 128, 20, 0)]


@pytest.mark.parametrize("R,K,N,silu", GEMV_CASES)
def test_gemv_rows_vs_f64(L, R, K, N, silu):
    W, b, x = _gemv_inputs(R, K, N)
    y = _run_gemv(L, W, b, x, silu).double()
    ref, bound = nm.gemv_ref(W, b, x)              # (K + 2) u (sum |w x| + |b|)
    if silu:
        ref, bound = nm.silu_ref(ref, bound)       # + 1.1 E + 0.5 E^2 + 8 u |silu| (nm.silu_ref)
    assert torch.isfinite(y).all(), f"{int((~torch.isfinite(y)).sum())} of {y.numel()} outputs were never written"
    err = (y - ref).abs()
    ratio = _ratio(err, bound)
    note_measured(test='nn_misc_gemv', R=R, K=K, N=N, silu=silu, ratio=ratio)
    bad = torch.nonzero(err > bound)
    assert len(bad) == 0, f"{len(bad)} outputs outside the bound, first (n, r) = {bad[0].tolist()}, ratio {ratio:.3g}"


def test_gemv_rows_silu_where_expf_overflows(L):
    """Pre-activations from -100 to +100 (the bias): expf(-a) is inf below -88.7 and 0 above +104, SiLU must stay finite and right."""
    R, K, N = 129, 128, 9
    W, b, x = _gemv_inputs(R, K, N, big=True)
    y = _run_gemv(L, W, b, x, 1).double()
    a, ea = nm.gemv_ref(W, b, x)
    assert float(a.min()) < -95 and float(a.max()) > 95
    ref, bound = nm.silu_ref(a, ea)
    assert torch.isfinite(y).all()
    err = (y - ref).abs()
    note_measured(test='nn_misc_gemv_silu_overflow', ratio=_ratio(err, bound))
    assert (err <= bound).all(), _ratio(err, bound)


def test_gemv_rows_refuses_k_beyond_the_lds_stage(L):
    R, K, N = 4, 2052, 2
    W, b, x = _gemv_inputs(R, K, N)
    y = Guarded(N * R)
    Wd, bd, xd = W.to(DEV), b.to(DEV), x.to(DEV)
    assert L.pdhip_gemv_rows_f32(_ptr(Wd), _ptr(bd), _ptr(xd), _ptr(y.t), R, K, N, 0, _stream()) == -1
    assert b'K too large (2052)' in L.pdhip_last_error()
    torch.cuda.synchronize()
    assert torch.isnan(y.t).all() and y.intact(), "a refused call launched something"


# ================================================================================================ b. timestep embedding + MLP
@pytest.mark.parametrize("N", [1, 5, 100])
@pytest.mark.parametrize("mc", [6, 32, 256])
def test_timestep_embedding_and_mlp_vs_f64(L, mc, N):
    g = torch.Generator().manual_seed(mc * 7 + N)
    w0, b0 = torch.randn((4 * mc, mc), generator=g) / math.sqrt(mc), torch.randn((4 * mc,), generator=g) * 0.1
    w2, b2 = torch.randn((4 * mc, 4 * mc), generator=g) / math.sqrt(4 * mc), torch.randn((4 * mc,), generator=g) * 0.1
    t = nm.timesteps(N)
    emb, tmp = Guarded(N * 4 * mc), Guarded(N * 5 * mc)
    dev = [v.to(DEV) for v in (t, w0, b0, w2, b2)]
    rc = L.pdhip_timestep_mlp_f32(_ptr(dev[0]), N, mc, _ptr(dev[1]), _ptr(dev[2]), _ptr(dev[3]), _ptr(dev[4]), _ptr(emb.t), _ptr(tmp.t), _stream())
    assert rc == 0, L.pdhip_last_error()
    torch.cuda.synchronize()
    assert emb.intact() and tmp.intact()
    tmp_h = tmp.t.cpu().double()
    temb, h1 = tmp_h[:N * mc].reshape(N, mc), tmp_h[N * mc:].reshape(N, 4 * mc)        # the documented layout of tmp
    out = emb.t.cpu().double().reshape(N, 4 * mc)
    assert torch.isfinite(tmp_h).all() and torch.isfinite(out).all()
    # the raw embedding: |t| freq_i (4 |z_i| + 3) u + 2 * 2^-23 (nm.temb_bound), which separates swapped halves, i + 1 and half - 1 (the CPU file)
    ref_t, bound_t = nm.temb_ref(t, mc), nm.temb_bound(t, mc)
    err = (temb - ref_t).abs()
    r_t = _ratio(err, bound_t)
    assert (err <= bound_t).all(), f"temb: first (n, column) = {torch.nonzero(err > bound_t)[0].tolist()}, ratio {r_t:.3g}"
    # each layer on its own, from what the layer before it left on the device: the plain GEMV + SiLU bound of (a)
    a1, e1 = nm.gemv_ref(w0, b0, temb)
    ref_h, bound_h = nm.silu_ref(a1, e1)
    r_h = _ratio((h1 - ref_h).abs(), bound_h)
    assert r_h <= 1.0, f"hidden layer: ratio {r_h:.3g}"
    a2, e2 = nm.gemv_ref(w2, b2, h1)
    ref_o, bound_o = nm.silu_ref(a2, e2)
    r_o = _ratio((out - ref_o).abs(), bound_o)
    assert r_o <= 1.0, f"output layer: ratio {r_o:.3g}"
    # end to end from t: the GEMV bound composed through both layers on top of the embedding's (nm.mlp_ref)
    _, _, ref_e, _, bound_e = nm.mlp_ref(t, mc, w0, b0, w2, b2)
    r_e = _ratio((out - ref_e).abs(), bound_e)
    note_measured(test='nn_misc_timestep_mlp', mc=mc, N=N, ratio_temb=r_t, ratio_hidden=r_h, ratio_out=r_o, ratio_end_to_end=r_e)
    assert r_e <= 1.0, f"emb_silu from t: ratio {r_e:.3g}"


# ================================================================================================ c. conv_in
def _conv_in_operands(N, H, W, Cout, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.rand((N, 3, H, W), generator=g) * 2 - 1
    w = torch.randn((Cout, 3, 3, 3), generator=g) / math.sqrt(27)      # no symmetry: a transposed or permuted tap order shows
    b = torch.randn((Cout,), generator=g) * 0.1
    return x, w, b


def _run_conv_in(L, xd, w, b, N, H, W, Cout):
    pad = (Cout + 127) // 128 * 128
    wt = nm.pack_conv_in_weight(w, pad).to(DEV)
    bd = b.float().to(DEV)
    y, ws = Guarded(N * H * W * Cout, torch.float16), Guarded(N * H * W * 32, torch.float16, fill=None)
    zp = torch.zeros((128,), dtype=torch.float16, device=DEV)
    rc = L.pdhip_conv_in_f16(_ptr(xd), _ptr(wt), _ptr(bd), _ptr(y.t), N, H, W, Cout, pad, _ptr(ws.t), _ptr(zp), _stream())
    assert rc == 0, L.pdhip_last_error()
    torch.cuda.synchronize()
    assert y.intact() and ws.intact(), "conv_in wrote behind its output or its im2col rows"
    return y.t.reshape(N, H, W, Cout)


# Shapes: what conv_igemm serves as a 1x1 over 32 channels (Cin % 32 == 0, Cout % 8 == 0, Cout_pad % 128 == 0, any N * H * W): a single 128-row tile, ragged
# tiles (180 and 126 pixels), non-square images, Cout below Cout_pad (32, 40, 8), two 128-column tiles (256), and the production layer (256^2, 256
# channels: the 256 x 256 tile geometry).
@pytest.mark.parametrize("N,H,W,Cout", [(1, 8, 8, 32), (3, 5, 12, 40), (2, 7, 9, 8), (1, 16, 16, 256), (1, 256, 256, 256)])
def test_conv_in_vs_conv2d_f64(L, N, H, W, Cout):
    x, w, b = _conv_in_operands(N, H, W, Cout, N * 100 + H + Cout)
    y = _run_conv_in(L, x.to(DEV), w, b, N, H, W, Cout).cpu().double().permute(0, 3, 1, 2)
    xh, wh, bd = x.half().double(), w.half().double(), b.double()
    ref = F.conv2d(xh, wh, bd, padding=1)
    bound = nm.conv_in_bound(ref, F.conv2d(xh.abs(), wh.abs(), bd.abs(), padding=1))      # 2^-11 |ref| + 30 u sum |w| |x|
    assert torch.isfinite(y).all(), "pixels never written"
    ratio = (y - ref).abs() / bound
    yy, xx = torch.meshgrid(torch.arange(H), torch.arange(W), indexing='ij')
    edge_y, edge_x = (yy == 0) | (yy == H - 1), (xx == 0) | (xx == W - 1)
    regions = {'corner': edge_y & edge_x, 'border': (edge_y | edge_x) & ~(edge_y & edge_x), 'interior': ~(edge_y | edge_x)}
    worst = {name: float(ratio[:, :, m].max()) for name, m in regions.items()}
    note_measured(test='nn_misc_conv_in', N=N, H=H, W=W, Cout=Cout, **{f'ratio_{k}': v for k, v in worst.items()})
    for name, r in worst.items():
        assert r <= 1.0, f"{name} pixels: ratio {r:.3g}"


def test_conv_in_beyond_the_im2col_grid_cap(L):
    """33 images of 256^2: 2 162 688 pixels against the 8192 x 256 = 2 097 152 threads of the im2col grid, so the last image's last 65 536 pixels are gathered
    on the second trip of the grid-stride loop.  Compared on the last 2 W pixels of the last image and on every 4099th pixel of the rest, against float64
    sums over the taps evaluated on the device."""
    N, H, W, Cout = 33, 256, 256, 8
    P = N * H * W
    assert P > 8192 * 256
    g = torch.Generator(device=DEV).manual_seed(33)
    xd = torch.rand((N, 3, H, W), generator=g, device=DEV) * 2 - 1
    _, w, b = _conv_in_operands(1, 1, 1, Cout, 34)
    y = _run_conv_in(L, xd, w, b, N, H, W, Cout).reshape(P, Cout)
    pix = torch.unique(torch.cat([torch.arange(0, P, 4099), torch.arange(P - 2 * W, P)])).to(DEV)
    assert int((pix >= 8192 * 256).sum()) >= 2 * W
    xp = F.pad(xd.half().double(), (1, 1, 1, 1))
    wh, bd = w.half().double().to(DEV), b.double().to(DEV)
    n, py, px = pix // (H * W), (pix // W) % H, pix % W
    ref, absref = bd[None].repeat(len(pix), 1), bd.abs()[None].repeat(len(pix), 1)
    for ky in range(3):
        for kx in range(3):
            v = xp[n, :, py + ky, px + kx]                                  # [P', 3]: x[n, :, y + ky - 1, x + kx - 1], zero outside
            ref += (v[:, None, :] * wh[None, :, :, ky, kx]).sum(-1)
            absref += (v[:, None, :].abs() * wh[None, :, :, ky, kx].abs()).sum(-1)
    got = y[pix].double()
    assert torch.isfinite(got).all()
    ratio = (got - ref).abs() / nm.conv_in_bound(ref, absref)
    tail = pix >= P - 2 * W
    note_measured(test='nn_misc_conv_in_grid_cap', ratio_tail=float(ratio[tail].max()), ratio_sample=float(ratio[~tail].max()))
    assert float(ratio[tail].max()) <= 1.0, f"last 2 W pixels: ratio {float(ratio[tail].max()):.3g}"
    assert float(ratio[~tail].max()) <= 1.0, f"strided sample: ratio {float(ratio[~tail].max()):.3g}"


# ================================================================================================ d. DDNM prepare / step
STEPS = (0, 1, 50, 98, 99)


def _et(et3, Cet):
    """[N,Cet,HW]: the three channels the update reads, followed (learn_sigma) by three it must not read -- NaN."""
    if Cet == 3:
        return et3.contiguous()
    return torch.cat([et3, torch.full_like(et3, float('nan'))], dim=1).contiguous()


@pytest.mark.parametrize("HW", [4, 64])
@pytest.mark.parametrize("Cet", [3, 6])
def test_ddnm_prepare_and_step_vs_f64(L, coefs, Cet, HW):
    N = 3
    x, et3, img, eps, mask = nm.ddnm_inputs(N, HW, 7 * HW + Cet)
    imgd, maskd, etd, epsd = img.to(DEV), mask.to(DEV), _et(et3, Cet).to(DEV), eps.to(DEV)
    y = Guarded(N * 3 * HW)
    assert L.pdhip_ddnm_prepare(_ptr(imgd), _ptr(maskd), _ptr(y.t), N, HW, _stream()) == 0, L.pdhip_last_error()
    torch.cuda.synchronize()
    assert y.intact()
    yh = y.t.cpu().reshape(N, 3, HW)
    ref_y, bound_y = nm.ddnm_prepare_ref(img, mask)                         # 2 u |m| (2 |img| + 1)
    worst = {'prepare': _ratio((yh.double() - ref_y).abs(), bound_y)}
    assert worst['prepare'] <= 1.0, worst
    for k in STEPS:
        xg = Guarded(N * 3 * HW)
        xg.t.copy_(x.reshape(-1))
        rc = L.pdhip_ddnm_step(_ptr(xg.t), _ptr(etd), Cet, _ptr(y.t), _ptr(maskd), _ptr(epsd), 0, k, N, HW, _stream())
        assert rc == 0, L.pdhip_last_error()
        torch.cuda.synchronize()
        assert xg.intact()
        got = xg.t.cpu().reshape(N, 3, HW).double()
        assert torch.isfinite(got).all(), f"step {k}: the update read et channels 3..5 or left elements unwritten"
        ref, bound = nm.ddnm_step_ref(x, et3, yh, mask, eps, coefs[k])      # 9 u x (the update over absolute values), nm.DDNM_C
        err = (got - ref).abs()
        worst[f'step{k}'] = _ratio(err, bound)
        bad = torch.nonzero(err > bound)
        assert len(bad) == 0, f"step {k}: {len(bad)} elements outside the bound, first (n, c, p) = {bad[0].tolist()}, ratio {worst[f'step{k}']:.3g}"
    note_measured(test='nn_misc_ddnm', Cet=Cet, HW=HW, **{f'ratio_{k}': v for k, v in worst.items()})


def _device_inputs(N, HW, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    x, et3, eps = (torch.randn((N, 3, HW), generator=g, device=DEV) for _ in range(3))
    img = torch.rand((N, 3, HW), generator=g, device=DEV)
    mask = torch.rand((N, HW), generator=g, device=DEV)
    mask = torch.where(mask < 0.3, torch.zeros_like(mask), torch.where(mask > 0.7, torch.ones_like(mask), mask))
    return x, et3, img, eps, mask


def test_ddnm_prepare_beyond_the_grid_cap(L):
    """3 x 3 x 116 513 = 1 048 617 elements against 4096 x 256 = 1 048 576 threads: the last 41 are written on the second trip.  Compared in full on the
    device with the same formula in float64."""
    N, HW = 3, 116513
    assert N * 3 * HW > 4096 * 256
    _, _, img, _, mask = _device_inputs(N, HW, 5)
    y = Guarded(N * 3 * HW)
    assert L.pdhip_ddnm_prepare(_ptr(img), _ptr(mask), _ptr(y.t), N, HW, _stream()) == 0, L.pdhip_last_error()
    torch.cuda.synchronize()
    assert y.intact()
    ref, bound = nm.ddnm_prepare_ref(img, mask)
    got = y.t.reshape(N, 3, HW).double()
    assert torch.isfinite(got).all()
    ratio = _ratio((got - ref).abs(), bound)
    note_measured(test='nn_misc_ddnm_prepare_grid_cap', ratio=ratio)
    assert ratio <= 1.0, ratio


def test_ddnm_step_beyond_the_grid_cap(L, coefs):
    """3 x 3 x 466 036 = 4 194 324 elements against 4096 x 256 threads of 4 elements: the last 5 quads are updated on the second trip."""
    N, HW, k = 3, 466036, 50
    assert N * 3 * HW > 4096 * 256 * 4 and HW % 4 == 0
    x, et3, img, eps, mask = _device_inputs(N, HW, 6)
    y = (mask[:, None] * (2 * img - 1)).contiguous()
    xg = Guarded(N * 3 * HW)
    xg.t.copy_(x.reshape(-1))
    assert L.pdhip_ddnm_step(_ptr(xg.t), _ptr(et3), 3, _ptr(y), _ptr(mask), _ptr(eps), 0, k, N, HW, _stream()) == 0, L.pdhip_last_error()
    torch.cuda.synchronize()
    assert xg.intact()
    ref, bound = nm.ddnm_step_ref(x, et3, y, mask, eps, coefs[k])
    got = xg.t.reshape(N, 3, HW).double()
    assert torch.isfinite(got).all()
    ratio = _ratio((got - ref).abs(), bound)
    note_measured(test='nn_misc_ddnm_step_grid_cap', ratio=ratio)
    assert ratio <= 1.0, ratio


# ================================================================================================ e. the Philox stream, exactly
@pytest.mark.parametrize("seed,stream_id", [(0x123456789ABCDEF1, 0x100000003), (0xFFFFFFFF00000000, 0x8000000000000001)])
def test_philox_normal_is_philox4x32_10_box_muller(L, seed, stream_id):
    """n = 4096 x 256 x 4 + 5: two quads beyond one trip of the 4096-block grid, the last of them a single value (n % 4 == 1).  The first and the last 4096
    values against Philox4x32-10 on python integers (known-answer tested in the CPU file), the exact f32 uniforms and a float64 Box-Muller, under
    max(1, r) 21 u (nm.PHILOX_K)."""
    n = 4096 * 256 * 4 + 5
    buf = Guarded(n, fill=None)                   # the whole buffer carries the guard pattern: a skipped element shows as well
    assert L.pdhip_philox_normal(_ptr(buf.t), n, seed, stream_id, _stream()) == 0, L.pdhip_last_error()
    torch.cuda.synchronize()
    assert buf.intact(), "elements n.. were written"
    assert not bool((buf.raw[:n] == GUARD32).any()), "elements left unwritten"
    worst = {}
    for name, lo in (('first', 0), ('last', n - 4096)):
        q0, q1 = lo // 4, (lo + 4096 + 3) // 4
        z, bound = nm.normal_ref(nm.philox_words(seed, stream_id, q0, q1 - q0))
        z, bound = z[lo - 4 * q0:][:4096], bound[lo - 4 * q0:][:4096]
        got = buf.t[lo:lo + 4096].cpu().double().numpy()
        err = np.abs(got - z)
        worst[name] = float((err / bound).max())
        assert (err <= bound).all(), f"{name} 4096: element {lo + int(np.argmax(err / bound))}, ratio {worst[name]:.3g}"
    note_measured(test='nn_misc_philox', seed=hex(seed), stream=hex(stream_id), ratio_first=worst['first'], ratio_last=worst['last'])


# ================================================================================================ f. one stream, two doors
def test_ddnm_step_device_noise_is_the_philox_normal_stream(L):
    """eps = NULL draws, inside the update, exactly the values pdhip_philox_normal hands out for (seed, stream k + 1): bit-equal results."""
    N, HW, seed = 3, 64, 0x5EED0000BEEF0001
    n = N * 3 * HW
    x, et3, img, _, mask = nm.ddnm_inputs(N, HW, 99)
    y = (mask[:, None] * (2 * img - 1)).contiguous().to(DEV)
    etd, maskd = et3.contiguous().to(DEV), mask.to(DEV)
    for k in STEPS:
        eps, other = Guarded(n), Guarded(n)
        assert L.pdhip_philox_normal(_ptr(eps.t), n, seed, k + 1, _stream()) == 0, L.pdhip_last_error()
        assert L.pdhip_philox_normal(_ptr(other.t), n, seed, k, _stream()) == 0, L.pdhip_last_error()
        xa, xb, xc = (x.reshape(-1).to(DEV).clone() for _ in range(3))
        assert L.pdhip_ddnm_step(_ptr(xa), _ptr(etd), 3, _ptr(y), _ptr(maskd), _ptr(eps.t), 0, k, N, HW, _stream()) == 0, L.pdhip_last_error()
        assert L.pdhip_ddnm_step(_ptr(xb), _ptr(etd), 3, _ptr(y), _ptr(maskd), None, seed, k, N, HW, _stream()) == 0, L.pdhip_last_error()
        assert L.pdhip_ddnm_step(_ptr(xc), _ptr(etd), 3, _ptr(y), _ptr(maskd), _ptr(other.t), 0, k, N, HW, _stream()) == 0, L.pdhip_last_error()
        torch.cuda.synchronize()
        assert eps.intact() and torch.isfinite(xa).all()
        assert torch.equal(xa.view(torch.int32), xb.view(torch.int32)), f"step {k}: the two doors disagree"
        if k < 99:                                # (at the last step a_next = 1: sigma_t = 0 and the noise does not enter)
            assert not torch.equal(xa, xc), f"step {k}: stream {k} and stream {k + 1} give the same update"
