"""Shared by tests/test_gpu_nn_misc.py and tests/test_nn_misc_cpu.py: float64 references of the UNet's f32 side ops (csrc/nn_misc.hip) and how far an
honest f32 evaluation may stray from them.  The references are written from the formulas of the reference project (guided_diffusion/nn.py:103-121,
unet.py:472-476, diffusion.py:529-552) and from the published Philox algorithm (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3",
SC'11), not from the kernels; the bounds come from counting roundings, none from a measurement.

u = 2^-24 is the largest relative error of one round-to-nearest f32 operation.  The device's expf / logf / sinf / cosf are taken as good to 1, 1, 2 and 2
ulp (1 ulp <= 2 u relative), division and square root as correctly rounded (the build asks for neither fast-math nor the approximate forms).  Every
bound is first order in u with the next integer taken where a second-order term could matter.
"""
import math

import numpy as np
import torch

U32 = 2.0 ** -24
TINY = 2.0 ** -126          # a result below the smallest normal f32 may be flushed to zero


# ------------------------------------------------------------------------------------------------ GEMV + SiLU
def silu64(a):
    return a / (1.0 + torch.exp(-a))


def gemv_ref(W, b, x, x_err=None):
    """W [R,K], b [R], x [N,K] (any float dtype) -> (a [N,R] float64, bound [N,R] float64) of a = x W^T + b.

    Bound: each product w_k x_k is rounded once (or not at all under FMA), the K products and the bias are joined by K additions in an order the kernel
    is free to choose, so a term passes through at most K + 1 roundings: |err| <= (K + 1) u (sum_k |w_k x_k| + |b|) to first order (Higham, Accuracy and
    Stability of Numerical Algorithms, section 3.1); K + 2 pays for the second-order terms.
    x_err [N,K] (optional): how far the x the kernel read may lie from the x given here; it passes through as |W| x_err, and the rounding bound is then
    taken over |x| + x_err."""
    W, b, x = W.double(), b.double(), x.double()
    K = W.shape[1]
    a = x @ W.T + b
    ax = x.abs() if x_err is None else x.abs() + x_err
    bound = (K + 2) * U32 * (ax @ W.abs().T + b.abs())
    if x_err is not None:
        bound = bound + x_err @ W.abs().T
    return a, bound


def silu_ref(a, a_bound):
    """silu(a) in float64 and the bound of an f32 a / (1 + expf(-a)) whose argument is off by at most a_bound.

    Argument: |silu'| = |s (1 + a (1 - s))|, s = sigmoid(a), peaks at 1.0998 (a = 2.3994) and |silu''| <= 0.5, so the argument error passes through as
    1.1 E + 0.5 E^2.  Own arithmetic, relative to |silu(a)|: expf is off by 1 ulp = 2 u, which reaches the denominator 1 + e scaled by e / (1 + e) < 1;
    the addition rounds once (u); the division once (u): 4 u, taken as 8 u so that a 2.5 ulp division would pass as well.  Where expf(-a) overflows
    (a < -88.7) the quotient is -0 against a true value below 89 e^-88.7 = 3e-37, and results under 2^-126 may be flushed: both are far inside the
    absolute term TINY + 1.1 E, E being at least u |a| there."""
    s = silu64(a)
    return s, 1.1 * a_bound + 0.5 * a_bound ** 2 + 8 * U32 * s.abs() + TINY


# ------------------------------------------------------------------------------------------------ timestep embedding
def temb_ref(t, mc, variant='right'):
    """nn.py:103-121 in float64: freqs_i = exp(-ln(10000) i / half), i = 0 .. half - 1, emb = [cos(t freqs) | sin(t freqs)].
    variant names a deliberately wrong formula (the bugs the bound has to separate): 'swapped' halves, 'i+1' frequencies, 'half-1' as the divisor."""
    t = torch.as_tensor(t, dtype=torch.float64)
    half = mc // 2
    i = torch.arange(half, dtype=torch.float64)
    if variant == 'i+1':
        i = i + 1
    div = half - 1 if variant == 'half-1' else half
    freqs = torch.exp(-math.log(10000.0) * i / div)
    args = t[:, None] * freqs[None]
    parts = [torch.sin(args), torch.cos(args)] if variant == 'swapped' else [torch.cos(args), torch.sin(args)]
    return torch.cat(parts, dim=-1)


def temb_bound(t, mc):
    """[N, mc] float64: how far an f32 evaluation of the embedding may lie from temb_ref.

    The phase is a = t freq_i with freq_i = expf(z_i), z_i = -logf(10000) i / half.  Roundings, in units of u relative:
      z_i:  logf(10000) 2 (1 ulp), the product with i 1, the division by half 1                                    -> c_z = 4
      freq: exp turns a relative error e of its argument into |z_i| e of its result, then its own 1 ulp             -> c_z |z_i| + 2
      a:    the product t freq rounds once more                                                                      -> c_i = c_z |z_i| + 3
    so |a_f32 - a| <= |t| freq_i c_i u with c_i between 3 (i = 0, where z = 0 and expf(0) = 1 are exact) and 4 ln(10000) + 3 = 39.9.  cos and sin have
    slope <= 1 in the phase and add their own 2 ulp of a value <= 1: 2 * 2^-23.  At t = 999, i = 0 that is 999 * 3 u + 2.4e-7 = 1.8e-4."""
    t = torch.as_tensor(t, dtype=torch.float64)
    half = mc // 2
    z = math.log(10000.0) * torch.arange(half, dtype=torch.float64) / half
    phase = t.abs()[:, None] * torch.exp(-z)[None] * (4 * z + 3)[None] * U32
    b = phase + 2 * 2.0 ** -23
    return torch.cat([b, b], dim=-1)


def mlp_ref(t, mc, w0, b0, w2, b2, temb=None, temb_err=None):
    """unet.py:472-476 followed by the SiLU every emb_layers starts with, float64: (temb, h1, emb_silu, bound_h1, bound_emb).  The bounds compose gemv_ref /
    silu_ref through the two layers: the input error of a layer is the bound of the layer before it."""
    if temb is None:
        temb, temb_err = temb_ref(t, mc), temb_bound(t, mc)
    a1, e1 = gemv_ref(w0, b0, temb, temb_err)
    h1, bh1 = silu_ref(a1, e1)
    a2, e2 = gemv_ref(w2, b2, h1, bh1)
    out, bout = silu_ref(a2, e2)
    return temb, h1, out, bh1, bout


# ------------------------------------------------------------------------------------------------ conv_in
def pack_conv_in_weight(w, cout_pad):
    """w [Cout,3,3,3] (OIHW) -> the layout pdhip_conv_in_f16 documents: [Cout_pad][32] f16, k = (ky * 3 + kx) * 3 + c, k >= 27 and rows >= Cout zero."""
    cout = w.shape[0]
    wt = torch.zeros((cout_pad, 32), dtype=torch.float16)
    wt[:cout, :27] = w.permute(0, 2, 3, 1).reshape(cout, 27).half()
    return wt


def conv_in_bound(ref, absref):
    """ref = conv2d(x.half(), w.half()) + b in float64, absref = conv2d(|x.half()|, |w.half()|) + |b|.  The products of two f16 numbers are exact in f32; the
    27 of them and the bias are added in f32 by the matrix pipe in an order of its own (at most 28 additions on a term's path, 30 with the zero taps of
    the 32-wide row): 30 u sum|w||x|.  The result is rounded once to f16: 2^-11 |ref|.
    (The f16 term is half an ulp at the bottom of a binade, so over thousands of outputs the largest error / bound ratio comes close to 1 by construction;
    the slack of this bound is the f32 term, which an honest accumulation uses a tenth of.)"""
    return 2.0 ** -11 * ref.abs() + 30 * U32 * absref


# ------------------------------------------------------------------------------------------------ DDNM
DDNM_C = 9
"""Roundings on the longest path of the update (diffusion.py:529-552 with sigma_y = 0, so lambda_t = 1 and gamma_t = sigma_t):
   x0  = (x - e s1) / sa          e s1 (1), the difference (2), the quotient (3)
   x0h = x0 - m (m x0 - y)        m x0 (4), minus y (5), times m (6), the difference (7)
   x'  = san x0h + sig (c1 z + c2 e)     san x0h (8), the final sum (9); the noise branch is shorter (c1 z, c2 e, their sum, times sig: 4, then the sum).
An FMA only removes roundings.  Each rounding is relative to an intermediate no larger than the same expression over absolute values, and everything
after it multiplies by coefficients that are no larger in the absolute form either, so |err| <= 9 u A with A the update evaluated with every term replaced
by its absolute value and every subtraction by an addition."""


def ddnm_prepare_ref(img, mask):
    """y = mask * (2 img - 1) (diffusion.py:477-485: data_transform, then A(z) = z * mask): (y, bound) float64.  2 img is exact; the difference and the
    product round once each (an FMA makes it one): 2 u |m| (2 |img| + 1), with TINY for a flushed subnormal product."""
    img, m = img.double(), mask.double()[:, None]
    return m * (2 * img - 1), 2 * U32 * m.abs() * (2 * img.abs() + 1) + TINY


def ddnm_step_ref(x, et3, y, mask, eps, co):
    """One update in float64 from f32 operands; co = (sqrt(1 - a_t), sqrt(a_t), sqrt(a_next), sigma_t, c1, c2), the f32 values pdhip_ddnm_schedule reports.
    x, et3, y, eps [N,3,HW], mask [N,HW] -> (x', bound)."""
    s1, sa, san, sig, c1, c2 = [float(v) for v in co]
    x, e, y, z, m = x.double(), et3.double(), y.double(), eps.double(), mask.double()[:, None]
    x0 = (x - e * s1) / sa
    out = san * (x0 - m * (m * x0 - y)) + sig * (c1 * z + c2 * e)
    ax0 = (x.abs() + e.abs() * s1) / sa
    A = san * (ax0 + m.abs() * (m.abs() * ax0 + y.abs())) + sig * (c1 * z.abs() + c2 * e.abs())
    return out, DDNM_C * U32 * (1 + 1e-6) * A + TINY


# ------------------------------------------------------------------------------------------------ Philox4x32-10 + Box-Muller
PHILOX_M0, PHILOX_M1 = 0xD2511F53, 0xCD9E8D57
PHILOX_W0, PHILOX_W1 = 0x9E3779B9, 0xBB67AE85
M32 = 0xFFFFFFFF


def philox4x32_10(ctr, key):
    """Philox4x32 with 10 rounds on python integers.  A round maps (c0, c1, c2, c3) to (hi(M1 c2) ^ c1 ^ k0, lo(M1 c2), hi(M0 c0) ^ c3 ^ k1, lo(M0 c0));
    the key is bumped by the Weyl constants between rounds."""
    c0, c1, c2, c3 = ctr
    k0, k1 = key
    for r in range(10):
        if r:
            k0, k1 = (k0 + PHILOX_W0) & M32, (k1 + PHILOX_W1) & M32
        p0, p1 = PHILOX_M0 * c0, PHILOX_M1 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & M32, (p0 >> 32) ^ c3 ^ k1, p0 & M32
    return c0, c1, c2, c3


def philox_words(seed, stream_id, quad0, nquads):
    """[nquads, 4] uint32: the words of quads quad0 .. quad0 + nquads - 1 of stream (seed, stream_id): counter {quad lo, quad hi, stream lo, stream hi},
    key {seed lo, seed hi}."""
    key = (seed & M32, (seed >> 32) & M32)
    out = np.empty((nquads, 4), dtype=np.uint32)
    for j in range(nquads):
        q = quad0 + j
        out[j] = philox4x32_10((q & M32, (q >> 32) & M32, stream_id & M32, (stream_id >> 32) & M32), key)
    return out


PHILOX_K = 21
"""Box-Muller from exact uniforms, z = r cos(theta) (or sin), r = sqrt(-2 ln u0), theta = 2 pi u1, in units of u:
   r:      logf 1 ulp = 2 relative, times -2 exact; the square root halves that (1) and rounds itself, taken as 1 ulp (2)        -> 3 relative
   theta:  the f32 constant 6.2831855 is 0.47 u from 2 pi (1), the product rounds (1): 2 relative, times theta <= 2 pi            -> 12.6 absolute
   cos:    slope <= 1 in theta (12.6), own 2 ulp of a value <= 1 (4)                                                             -> 16.6 absolute
   z:      r (16.6 + 3 |cos| + 1 for the product's rounding) <= 20.6 r, rounded up                                               -> k = 21
and the bound is max(1, r) k u (max(1, .) keeps an absolute floor where r is tiny)."""


def normal_ref(words):
    """words [Q, 4] uint32 -> (z [Q*4] float64, bound [Q*4]).  u = (float(c) + 0.5) 2^-32 is reproduced with the same three f32 operations (conversion with
    round-to-nearest-even, addition, multiplication by a power of two), which is exact; Box-Muller then runs in float64."""
    u = (words.astype(np.float32) + np.float32(0.5)) * np.float32(2.0 ** -32)
    assert u.dtype == np.float32
    u = u.astype(np.float64)
    r0, r1 = np.sqrt(-2.0 * np.log(u[:, 0])), np.sqrt(-2.0 * np.log(u[:, 2]))
    t0, t1 = 2.0 * math.pi * u[:, 1], 2.0 * math.pi * u[:, 3]
    z = np.stack([r0 * np.cos(t0), r0 * np.sin(t0), r1 * np.cos(t1), r1 * np.sin(t1)], axis=1).reshape(-1)
    r = np.stack([r0, r0, r1, r1], axis=1).reshape(-1)
    return z, np.maximum(1.0, r) * PHILOX_K * U32


# ------------------------------------------------------------------------------------------------ inputs both test files use
T_FIXED = [999.0, 0.0, 0.5, 1.0, 10.0, 499.0, 1000.0, 3.25, 123.456, 777.7]


def timesteps(N):
    """[N] float32: 999 first (the largest phase), then the fixed list and seeded non-integers in [0, 1000)."""
    g = torch.Generator().manual_seed(1000 + N)
    extra = (torch.rand((max(N - len(T_FIXED), 0),), generator=g) * 1000.0).tolist()
    return torch.tensor((T_FIXED + extra)[:N], dtype=torch.float32)


def ddnm_inputs(N, HW, seed):
    """x, et3, img, eps [N,3,HW] and mask [N,HW] f32: every image has its own mask, a third of each 0, a third 1, a third fractional in (0, 1)."""
    g = torch.Generator().manual_seed(seed)
    x, et3, eps = (torch.randn((N, 3, HW), generator=g) for _ in range(3))
    img = torch.rand((N, 3, HW), generator=g)
    kind = torch.randint(0, 3, (N, HW), generator=g)
    kind[:, :3] = torch.tensor([0, 1, 2])                       # (every kind in every image, however small HW)
    for n in range(N):
        kind[n] = kind[n].roll(n)
    frac = torch.rand((N, HW), generator=g) * 0.98 + 0.01
    mask = torch.where(kind == 0, torch.zeros(()), torch.where(kind == 1, torch.ones(()), frac))
    return x, et3, img, eps, mask
