"""CPU: what tests/test_gpu_nn_misc.py relies on, checked without a GPU.  The Philox reference against the Random123 known-answer vectors; every bound of
tests/nn_misc_common.py from both sides -- an honest f32 evaluation of the formula (torch on the CPU) lies inside it, and the bugs the GPU tests are there
to find (a shifted bias row, swapped embedding halves, an off-by-one frequency, half - 1, m (x0 - y) for m (m x0 - y), a reused counter word, a transposed
tap order) lie outside it; and the argument checks of the three new entries, which refuse on the host before anything is launched."""
import ctypes as C
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import nn_misc_common as nm


# ---- Philox4x32-10: Random123's kat_vectors (philox4x32 10 <counter> <key> <expected>)
KAT = [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


@pytest.mark.parametrize("ctr,key,want", KAT)
def test_philox4x32_10_known_answers(ctr, key, want):
    assert nm.philox4x32_10(ctr, key) == want


def test_philox_words_counter_and_key_layout():
    """counter = {quad lo, quad hi, stream lo, stream hi}, key = {seed lo, seed hi}: the third known-answer vector read as (quad, stream, seed)."""
    quad, stream, seed = 0x85a308d3243f6a88, 0x0370734413198a2e, 0x299f31d0a4093822
    w = nm.philox_words(seed, stream, quad - 1, 2)
    assert tuple(int(v) for v in w[1]) == KAT[2][2]
    assert tuple(int(v) for v in w[0]) != KAT[2][2]
    assert tuple(int(v) for v in nm.philox_words(0, 0, 0, 1)[0]) == KAT[0][2]


def test_uniform_and_box_muller_edges():
    """Words 0 and 2^32 - 1: u = 2^-33 and u = 1 (float(2^32 - 1) + 0.5 rounds to 2^32), both finite through the logarithm; an f32 Box-Muller over the
    same words lies inside the bound, one that uses word 1 twice does not."""
    w = np.array([[0, 0, 0xFFFFFFFF, 0xFFFFFFFF], [0xFFFFFFFF, 0x80000000, 0, 0x40000000]], dtype=np.uint32)
    z, b = nm.normal_ref(w)
    assert np.isfinite(z).all() and abs(z[0] - math.sqrt(-2 * math.log(2.0 ** -33)) * math.cos(2 * math.pi * 2.0 ** -33)) < 1e-12
    assert z[2] == 0 and z[3] == 0 and z[4] == 0                           # r = sqrt(-2 ln 1) = 0
    words = nm.philox_words(0x123456789ABCDEF1, 0x100000003, 0, 512)
    z, b = nm.normal_ref(words)

    def f32_normals(wd):
        u = (wd.astype(np.float32) + np.float32(0.5)) * np.float32(2.0 ** -32)
        r0, r1 = np.sqrt(np.float32(-2) * np.log(u[:, 0])), np.sqrt(np.float32(-2) * np.log(u[:, 2]))
        t0, t1 = np.float32(6.283185307179586) * u[:, 1], np.float32(6.283185307179586) * u[:, 3]
        out = np.stack([r0 * np.cos(t0), r0 * np.sin(t0), r1 * np.cos(t1), r1 * np.sin(t1)], axis=1)
        assert out.dtype == np.float32
        return out.reshape(-1).astype(np.float64)
    assert (np.abs(f32_normals(words) - z) <= b).all()
    reused = words.copy()
    reused[:, 3] = reused[:, 1]
    assert (np.abs(f32_normals(reused) - z) > b).mean() > 0.4              # (out[2], out[3] of every quad change)
    assert abs(z.mean()) < 0.1 and abs(z.std() - 1) < 0.1


# ---- timestep embedding
@pytest.mark.parametrize("mc", [6, 32, 256])
@pytest.mark.parametrize("N", [1, 5, 100])
def test_temb_f32_formula_inside_the_bound_and_wrong_formulas_outside(mc, N):
    t = nm.timesteps(N)
    ref, bound = nm.temb_ref(t, mc), nm.temb_bound(t, mc)
    assert float(bound.max()) < 2.5e-3 and float(bound[0, 0]) < 2e-4       # t = 999: i = 0 carries 3 roundings, the largest entry c_i freq_i peaks near i / half = 0.1
    # nn.py:103-121 in f32 on the CPU, as the reference project evaluates it
    half = mc // 2
    freqs = torch.exp(-math.log(10000) * torch.arange(start=0, end=half, dtype=torch.float32) / half)
    args = t[:, None].float() * freqs[None]
    f32 = torch.cat([torch.cos(args), torch.sin(args)], dim=-1)
    assert f32.dtype == torch.float32
    ratio = ((f32.double() - ref).abs() / bound).max().item()
    assert ratio <= 1.0, ratio
    for variant in ('swapped', 'i+1', 'half-1'):
        wrong = nm.temb_ref(t, mc, variant)
        assert ((wrong - ref).abs() > bound).any(), f"the bound does not separate '{variant}' at mc = {mc}, N = {N}"
        assert ((wrong - ref).abs() > bound)[0].any(), f"... not even at t = {float(t[0])}"


# ---- GEMV + SiLU
def _gemv_case(R, K, N, seed, big=False):
    g = torch.Generator().manual_seed(seed)
    W = torch.randn((R, K), generator=g) / math.sqrt(K)
    b = torch.linspace(-100.0, 100.0, R) if big else torch.randn((R,), generator=g)
    x = torch.randn((N, K), generator=g)
    return W, b, x


@pytest.mark.parametrize("R,K,N,big", [(3, 100, 7, False), (129, 256, 9, False), (130, 1024, 20, False), (129, 128, 9, True)])
def test_gemv_bound_holds_for_f32_and_catches_a_shifted_bias(R, K, N, big):
    W, b, x = _gemv_case(R, K, N, 5, big)
    a, ea = nm.gemv_ref(W, b, x)
    s, es = nm.silu_ref(a, ea)
    a32 = x @ W.T + b
    s32 = a32 / (1.0 + torch.exp(-a32))
    assert a32.dtype == torch.float32 and torch.isfinite(s32).all()
    assert ((a32.double() - a).abs() <= ea).all() and ((s32.double() - s).abs() <= es).all()
    if big:
        assert float(a.min()) < -95 and float(a.max()) > 95                # expf(-a) overflows at the low end
    wrong = x @ W.T + b.roll(1)                                            # b[r - 1] for b[r]
    assert ((wrong.double() - a).abs() > ea).float().mean() > 0.9
    wrong = x.roll(1, dims=0) @ W.T + b                                    # the x row of the neighbouring batch slot
    if N > 1:
        assert ((wrong.double() - a).abs() > ea).float().mean() > 0.9


def test_mlp_bound_composes_and_holds_for_f32():
    mc, N = 32, 5
    g = torch.Generator().manual_seed(11)
    w0, b0 = torch.randn((4 * mc, mc), generator=g) / math.sqrt(mc), torch.randn((4 * mc,), generator=g) * 0.1
    w2, b2 = torch.randn((4 * mc, 4 * mc), generator=g) / math.sqrt(4 * mc), torch.randn((4 * mc,), generator=g) * 0.1
    t = nm.timesteps(N)
    temb, h1, out, bh1, bout = nm.mlp_ref(t, mc, w0, b0, w2, b2)
    half = mc // 2
    freqs = torch.exp(-math.log(10000) * torch.arange(start=0, end=half, dtype=torch.float32) / half)
    e32 = torch.cat([torch.cos(t[:, None] * freqs[None]), torch.sin(t[:, None] * freqs[None])], dim=-1)
    h32 = F.silu(F.linear(e32, w0, b0))
    o32 = F.silu(F.linear(h32, w2, b2))
    assert ((h32.double() - h1).abs() <= bh1).all() and ((o32.double() - out).abs() <= bout).all()
    assert float(bout.max()) < 1e-2                                        # the composed bound still means something


# ---- conv_in
def test_conv_in_packed_layout_reproduces_conv2d():
    """The documented layout ([Cout_pad][32], k = (ky * 3 + kx) * 3 + c): patches gathered in that order, times the packed rows, is conv2d -- and a (kx, ky)
    gather is not."""
    g = torch.Generator().manual_seed(2)
    N, H, W, Cout, pad = 2, 5, 7, 8, 128
    x = torch.rand((N, 3, H, W), generator=g) * 2 - 1
    w = torch.randn((Cout, 3, 3, 3), generator=g) / math.sqrt(27)
    b = torch.randn((Cout,), generator=g) * 0.1
    wt = nm.pack_conv_in_weight(w, pad)
    assert wt.shape == (pad, 32) and wt.dtype == torch.float16 and not wt[:, 27:].any() and not wt[Cout:].any()
    xh, wh = x.half().double(), w.half().double()
    ref = F.conv2d(xh, wh, b.double(), padding=1)
    bound = nm.conv_in_bound(ref, F.conv2d(xh.abs(), wh.abs(), b.double().abs(), padding=1))
    xp = F.pad(xh, (1, 1, 1, 1))

    def gathered(transposed):
        rows = torch.zeros((N, H, W, 32), dtype=torch.float64)
        for ky in range(3):
            for kx in range(3):
                k = (kx * 3 + ky) * 3 if transposed else (ky * 3 + kx) * 3
                rows[..., k:k + 3] = xp[:, :, ky:ky + H, kx:kx + W].permute(0, 2, 3, 1)
        return (rows @ wt.double().T)[..., :Cout].permute(0, 3, 1, 2) + b.double()[None, :, None, None]
    assert ((gathered(False) - ref).abs() <= 1e-12).all()
    assert ((gathered(False).half().double() - ref).abs() <= bound).all()
    assert ((gathered(True) - ref).abs() > bound).float().mean() > 0.5


# ---- DDNM
@pytest.mark.parametrize("HW", [4, 64])
def test_ddnm_bound_holds_for_f32_and_needs_fractional_masks(HW):
    x, e, img, z, m = nm.ddnm_inputs(3, HW, 40 + HW)
    for n in range(3):
        assert (m[n] == 0).any() and (m[n] == 1).any() and ((m[n] > 0) & (m[n] < 1)).any()
    assert not torch.equal(m[0], m[1]) and not torch.equal(m[1], m[2])
    y, by = nm.ddnm_prepare_ref(img, m)
    y32 = (2.0 * img - 1.0) * m[:, None]
    assert ((y32.double() - y).abs() <= by).all()
    co = np.array([0.9, 0.43, 0.5, 0.7, 0.4, 0.3], dtype=np.float32)
    out, bound = nm.ddnm_step_ref(x, e, y32, m, z, co)
    s1, sa, san, sig, c1, c2 = [torch.tensor(v) for v in co]
    mm = m[:, None]
    x0 = (x - e * s1) / sa
    o32 = san * (x0 - mm * (mm * x0 - y32)) + sig * (c1 * z + c2 * e)
    assert o32.dtype == torch.float32 and ((o32.double() - out).abs() <= bound).all()
    wrong = san * (x0 - mm * (x0 - y32)) + sig * (c1 * z + c2 * e)          # A^T (A x - y) with the second mask factor lost
    bad = (wrong.double() - out).abs() > bound
    frac = ((mm > 0) & (mm < 1)).expand_as(bad)
    assert bad[frac].float().mean() > 0.9 and not bad[~frac].any()         # only a fractional mask tells the two apart


# ---- the entries refuse on the host (no GPU is touched: every check precedes the first launch)
def test_new_entries_refuse_bad_arguments():
    import __graft_entry__ as ge
    ge.build()
    from pointdreamer_amd import _lib
    import pointdreamer_amd.ddnm_inpainting  # noqa: F401
    L = _lib.lib()
    buf = (C.c_float * 4)()
    p = C.cast(buf, C.c_void_p)
    assert L.pdhip_gemv_rows_f32(p, p, p, p, 4, 2052, 1, 0, None) == -1
    assert b'K too large (2052)' in L.pdhip_last_error()
    assert L.pdhip_gemv_rows_f32(p, None, p, p, 4, 32, 1, 0, None) == -1 and b'pdhip_gemv_rows_f32' in L.pdhip_last_error()
    assert L.pdhip_gemv_rows_f32(p, p, p, p, 0, 32, 1, 0, None) == -1
    assert L.pdhip_timestep_mlp_f32(p, 1, 7, p, p, p, p, p, p, None) == -1 and b'pdhip_timestep_mlp_f32' in L.pdhip_last_error()
    assert L.pdhip_timestep_mlp_f32(p, 1, 32, p, p, p, p, p, None, None) == -1
    assert L.pdhip_conv_in_f16(p, p, p, p, 1, 8, 8, 32, 128, None, p, None) == -1 and b'pdhip_conv_in_f16' in L.pdhip_last_error()
    assert L.pdhip_conv_in_f16(p, p, p, p, 0, 8, 8, 32, 128, p, p, None) == -1
