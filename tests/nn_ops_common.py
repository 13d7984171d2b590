"""Shared by tests/test_gpu_nn_ops.py and tests/test_nn_ops_cpu.py: float64 references of attention (csrc/nn_attn.hip) and of the GroupNorm-apply family
(csrc/nn_norm.hip), and per-element bounds on how far an honest evaluation at the kernels' documented rounding points may stray from them.  Plain torch
float64, device-agnostic (the GPU tests evaluate the references on the device), nothing imported from the product, nothing taken from a measurement.

Notation: u32 = 2^-24 and u16 = 2^-11 are the unit roundoffs of f32 and f16; an f16 result below the normal range (2^-14) is off by at most 2^-25.

-------------------------------------------------------------------------------------------------------------------------------------------------
Attention.  Per head, w = softmax(q.k / sqrt(D)) and o = w v on the f16 inputs; A = sum_s w_s |v_s| is returned next to o.

Both kernels run an online softmax over chunks of 64 keys.  With M the row maximum, Z = sum_s exp(s_s - M) and P*_s = exp(s_s - M) (so w_s = P*_s / Z),
the kernel accumulates numerator sum_s P_s v_s and denominator sum_s P'_s with P_s = P*_s (1 + eta_s) and divides at the end; the running maximum a
probability was formed against cancels between the two (every rescale factor multiplies both), so only these terms remain:

  * the logit: an f32 matrix-pipe sum of D exact products, the scale, the subtraction of the maximum -- (2 D + 8) u32 |q|.|k| / sqrt(D), taken at the
    row's largest |q|.|k| (the factor 2 allows the pipe to truncate where the VALU rounds);
  * __expf / exp2: 2^-21 on a probability, and 2^-22 + 2 u32 per chunk on the rescale factor applied to what was accumulated before it;
  * f16 rounding of the probability RELATIVE TO THE RUNNING MAXIMUM AT THE TIME IT IS FORMED: u16 P*_s while it is a normal f16 there.  A probability
    that is below 2^-14 against that maximum is a subnormal f16: kept, it is off by at most 2^-25; flushed by the matrix pipe, it is lost entirely.
    MI355X_MICROARCH.md does not say which, so the bound holds both ways: every key with P*_s < 2^-14 (1 % slack for the computed logit) may be off by
    max(P*_s, 2^-25) (the running maximum is never above M, so a probability that is subnormal when formed has P*_s < 2^-14, and what is lost or
    mis-rounded scales down with the later rescales).  These enter as subN = sum_sub max(P*_s, 2^-25) |v_s| / Z and subD = the same without |v_s|;
  * the denominator.  k_attention sums the UNROUNDED f32 probabilities (form 'f32': no u16 and no subnormal term in the denominator);
    k_attention_t64 takes the sum of the f16-ROUNDED probabilities from the matrix pipe (form 'mfma': the numerator's terms);
  * f32 accumulation over the T keys: 2 T u32 of sum P |v| (of sum P for the denominator);
  * the reciprocal, the product and the final f16 rounding: (u16 + 4 u32) |o| + 2^-25.

  form 'f32':   E = A (u16 + eps + acc) + |o| (eps + acc) + subN
  form 'mfma':  E = (A + |o|) (u16 + eps + acc) + subN + |o| subD
  bound = 1.01 E + (u16 + 4 u32) |o| + 2^-25           (1.01: the second-order terms of a quotient of two sums perturbed by < 1e-3)

Every term scales with this element's own A, |o| and its row's logits; none with a global maximum.

-------------------------------------------------------------------------------------------------------------------------------------------------
GroupNorm-apply.  Reference: GroupNorm32 -> [FiLM] -> [SiLU] -> [AvgPool2d(2) | nearest x2] in float64 on the f16 input with float64 statistics; the
FiLM row is read as the reference project reads it, scale and shift as f16 tensors: t1 = 1 + f16(scale), sh = f16(shift).

The bound follows the rounding points of gn_elem (csrc/nn_common.h) and k_gn_apply: with dm, dr the statistics' own error (below),
  ga = f32(rstd gamma)           dga = |gamma| dr + u32 (|ga| + |gamma| dr)
  gb = f32(beta - f32(mean ga))  dgb = |ga| dm + (|mean| + dm) dga + 2 u32 (|mean ga| + |beta|)
  y0 = f16(fma(x, ga, gb))       e = |x| dga + dgb, then R(y0, e) = e' + half the f16 spacing at |y0| + e' (<= u16 of it; 2^-25 below the normal
                                 range) with e' = e + u32 (|y0| + e)
  y1 = f16(y0 f16(t1))           e = E |t1| + (|y0| + E) u16 |t1|, then R;      y2 = f16(y1 + sh): R(y2, E)
  y3 = f16(silu(y2))             e = |silu'(y2)| E + 0.25 E^2 + (16 + |y2|) u32 |silu| (|silu''| <= 0.5; exp, add, reciprocal, product), then the f16 rounding
  y4 = f16(f32 mean of four)     e = mean of the four E + 4 u32 mean(|y3| + E), then the f16 rounding;      nearest x2 repeats y3 and its bound.
With no FiLM, SiLU or resampling the bound is half an f16 spacing plus f32 terms a thousand times smaller, and rounding to nearest attains half a
spacing: the largest error / bound ratio of that flag set is just below 1 by construction (0.99 in the CPU emulation), not by a loose derivation.
The raw average-pool side output is f16 of an f32 sum of four f16 values times 0.25: one f16 ulp of the reference.

Statistics.  k_gn_partial: a thread sums ONE channel over its ceil(256 / pps) pixels of a 256-pixel chunk in f32 (pps = max(1, 256 / (C / 8)) pixel
slots), the slots and the channels of a group are combined in f64, the chunk's (sum, sum of squares) is stored as f32, k_gn_finalize combines the chunks in
f64.  So a group's sum is off by at most n u32 sum|x| with n = ceil(256 / pps) + 1 (the + 1: the f32 store of the chunk partial), the sum of squares by
n u32 sum x^2; from there like conv_epilogue_common.stats_bounds: dmean = dS / cnt, dvar = dQ / cnt + (2 |mean| + dmean) dmean, rstd monotone in var,
one f32 rounding of each result.  Octet partials (pdhip_gn_octet_partials_f16, the conv epilogues): n = 8 HW / chunks per source.

Table.  k_gn_table: A = f32(ga t1), B = f32(gb t1 + sh) with the f16 FiLM terms above:
  dA = dga |t1| + (|ga| + dga) u16 |t1| + u32 |A|,   dB = dgb |t1| + (|gb| + dgb) u16 |t1| + 2 u32 (|gb t1| + |sh|).
With FiLM the table bound is the f16 rounding of 1 + scale (u16 |t1|, attained for t1 just above a power of two) plus f32 terms: ratios just below 1 there too.
"""
import math

import torch

U32 = 2.0 ** -24
U16 = 2.0 ** -11
SUB16 = 2.0 ** -25            # half the spacing of the f16 subnormals
MIN16 = 2.0 ** -14            # smallest normal f16
EPS = 1e-5


def worst_ratio(got, ref, bound):
    """max |got - ref| / bound over ALL elements; inf when an element of `got` is not finite (never written)."""
    got = got.double()
    if not bool(torch.isfinite(got).all()):
        return float('inf')
    return float(((got - ref).abs() / bound).max())


# ================================================================================================ attention
# name, kernel ('generic': vt_ws = None, 't64': vt_ws given), N, T, C, D, regime
ATT_CASES = [
    ('generic-d32-2x64x64', 'generic', 2, 64, 64, 32, 'moderate'),
    ('generic-d32-1x192x96', 'generic', 1, 192, 96, 32, 'moderate'),
    ('generic-d64-1x64x64', 'generic', 1, 64, 64, 64, 'moderate'),
    ('generic-d64-3x192x128', 'generic', 3, 192, 128, 64, 'moderate'),
    ('t64-8x128x64', 't64', 8, 128, 64, 64, 'moderate'),              # one 128-query block, two chunks
    ('t64-1x384x512', 't64', 1, 384, 512, 64, 'moderate'),            # an odd number of blocks
    ('t64-2x1024x256', 't64', 2, 1024, 256, 64, 'moderate'),          # the network's longest sequence
    ('t64-2x1024x256-flat', 't64', 2, 1024, 256, 64, 'flat'),
    ('t64-2x1024x256-jump', 't64', 2, 1024, 256, 64, 'jump'),
    ('generic-d64-2x1024x256-flat', 'generic', 2, 1024, 256, 64, 'flat'),
    ('generic-d64-2x1024x256-jump', 'generic', 2, 1024, 256, 64, 'jump'),
    ('generic-d64-2x1024x256', 'generic', 2, 1024, 256, 64, 'moderate'),
]
ATT_VARIANTS = [(qt, nbuf, vt) for qt in (1, 2) for nbuf in (2, 3) for vt in (0, 1)]      # pdhip_debug_set_attn(nbuf, vt_form, qt)
JUMP_QUERIES = 4              # per (image, head) of the 'jump' regime


def jump_pairs(n, h, T):
    """(query, key) pairs of the late-jump construction: the key sits in the LAST 64-key chunk, so the row maximum jumps after everything else is summed."""
    return [((17 + 37 * i + 5 * h + 11 * n) % (T - 64), T - 1 - 7 * i - h - 2 * n) for i in range(JUMP_QUERIES)]


def attention_inputs(N, T, C, D, regime, seed=0):
    """qkv [N, T, 3 C] f16 (per head h: q | k | v at channels 3 D h ..), every image and head its own values.  flat: x 0.05 (1024 nearly equal weights);
    moderate: x 1.5; jump: x 0.5 with, per (image, head), four keys of the last chunk set to 6 x a query (the construction of
    test_attention_online_softmax_rescale_branch: logit 6 |q|^2 / 8 ~ 12 against a spread of 0.25)."""
    g = torch.Generator().manual_seed(1000 * T + C + D + seed)
    x = torch.randn((N, T, 3 * C), generator=g) * {'flat': 0.05, 'moderate': 1.5, 'jump': 0.5}[regime]
    if regime == 'jump':
        for n in range(N):
            for h in range(C // D):
                b = 3 * D * h
                for tq, tk in jump_pairs(n, h, T):
                    x[n, tk, b + D:b + 2 * D] = x[n, tq, b:b + D] * 6.0
    return x.half()


def attention_ref(qkv, D):
    """qkv [N, T, 3 C] f16 (any device) -> dict of float64 [N, T, C] tensors: o, A = sum w |v|, subN, and per row (repeated over the head's D columns)
    absmax = max_s |q|.|k_s| / sqrt(D) and subD.  One (image, head) at a time: T x T float64 matrices."""
    N, T, C3 = qkv.shape
    C = C3 // 3
    heads = C // D
    out = {k: torch.empty((N, T, C), dtype=torch.float64, device=qkv.device) for k in ('o', 'A', 'subN', 'subD', 'absmax')}
    x = qkv.double().reshape(N, T, heads, 3, D)
    for n in range(N):
        for h in range(heads):
            q, k, v = x[n, :, h, 0], x[n, :, h, 1], x[n, :, h, 2]
            S = (q @ k.T) / math.sqrt(D)
            P = torch.exp(S - S.max(dim=-1, keepdim=True).values)
            Z = P.sum(dim=-1, keepdim=True)
            w = P / Z
            lost = torch.where(P < MIN16 * 1.01, P.clamp(min=SUB16), torch.zeros_like(P)) / Z
            sl = slice(h * D, (h + 1) * D)
            out['o'][n, :, sl] = w @ v
            out['A'][n, :, sl] = w @ v.abs()
            out['subN'][n, :, sl] = lost @ v.abs()
            out['subD'][n, :, sl] = lost.sum(dim=-1, keepdim=True)
            out['absmax'][n, :, sl] = ((q.abs() @ k.abs().T) / math.sqrt(D)).max(dim=-1, keepdim=True).values
    return out


def attention_bound(ref, T, D, form):
    """Per-element bound [N, T, C] for the kernel form 'f32' (k_attention) or 'mfma' (k_attention_t64); derivation in the module docstring."""
    o, A = ref['o'].abs(), ref['A']
    eps = (2 * D + 8) * U32 * ref['absmax'] + 2.0 ** -21 + (T // 64) * (2.0 ** -22 + 2 * U32)
    acc = 2 * T * U32
    if form == 'f32':
        E = A * (U16 + eps + acc) + o * (eps + acc) + ref['subN']
    else:
        assert form == 'mfma'
        E = (A + o) * (U16 + eps + acc) + ref['subN'] + o * ref['subD']
    return 1.01 * E + (U16 + 4 * U32) * o + SUB16


def attention_form(kernel):
    return 'mfma' if kernel == 't64' else 'f32'


# ================================================================================================ GroupNorm
GN_CHANNELS = (32, 96, 160, 256, 768, 1536, 2048)
GN_SIZES = ((4, 4), (6, 10), (16, 18))        # 16 x 18 = 288 pixels: two statistics chunks, the second with 32 pixels
GN_FLAGS = [(film, silu, res) for film in (0, 1) for silu in (0, 1) for res in (0, 1, 2) if not (film and res)]      # gn_apply: FiLM only without resampling
GN_TWO_SOURCE = ((64, 192), (256, 768), (512, 1536))
GN_N = 3


def gn_inputs(N, H, W, C, seed=0):
    """x [N, H, W, C] f16 with a scale and an offset per (image, channel) (a wrong image, group or channel is an O(1) error), gamma, beta [C] f32,
    film [N, 2 C] f32 = (scale | shift) rows."""
    g = torch.Generator().manual_seed(100003 * C + 101 * H + W + seed)
    x = torch.randn((N, H, W, C), generator=g) * (0.5 + 1.5 * torch.rand((N, 1, 1, C), generator=g)) + torch.randn((N, 1, 1, C), generator=g)
    gamma = 1.0 + 0.2 * torch.randn((C,), generator=g)
    beta = 0.2 * torch.randn((C,), generator=g)
    film = 0.3 * torch.randn((N, 2 * C), generator=g)
    return x.half(), gamma, beta, film


def gn_stats_ref(x):
    """x [N, H, W, C] (f16 values) -> float64 (mean, rstd) [N, 32] of GroupNorm(32), eps 1e-5."""
    N, C = x.shape[0], x.shape[-1]
    g = x.double().reshape(N, -1, 32, C // 32)
    mean = g.mean(dim=(1, 3))
    var = (g * g).mean(dim=(1, 3)) - mean * mean
    return mean, (var.clamp(min=0) + EPS) ** -0.5


def partial_terms(C):
    """n of k_gn_partial + k_gn_finalize for a C-channel tensor: per-thread f32 sum over ceil(256 / pps) pixels, + 1 for the f32 store of the chunk partial."""
    pps = max(1, 256 // (C // 8))
    return -(-256 // pps) + 1


def gn_stats_bounds(x, n_terms):
    """(dmean, drstd) [N, 32]: how far f32-summed statistics may lie from gn_stats_ref(x).  n_terms: the f32 summation length behind every channel's
    contribution -- a number, or a [C] tensor (two sources chunked differently)."""
    N, C = x.shape[0], x.shape[-1]
    cg = C // 32
    xa = x.double().abs().reshape(N, -1, C)
    nt = torch.as_tensor(n_terms, dtype=torch.float64, device=x.device).expand(C)
    dS = (U32 * nt * xa).reshape(N, -1, 32, cg).sum(dim=(1, 3))
    dQ = (U32 * nt * xa * xa).reshape(N, -1, 32, cg).sum(dim=(1, 3))
    cnt = xa.shape[1] * cg
    mean, rstd = gn_stats_ref(x)
    var = rstd ** -2 - EPS
    dmean = dS / cnt
    dvar = dQ / cnt + (2 * mean.abs() + dmean) * dmean
    worst = ((var - dvar).clamp(min=0) + EPS) ** -0.5
    return dmean + U32 * mean.abs(), (worst - rstd) + U32 * worst


def ulp16(v):
    """Spacing of the f16 grid at |v| (float64 tensor); 2^-24 below the normal range."""
    e = torch.floor(torch.log2(v.abs().clamp(min=MIN16)))
    return 2.0 ** (e - 10)


def _r16(val, err, op=True):
    """Error after (an f32 operation and) the rounding to f16 of a quantity whose exact value is `val` and that carried `err` before: half the f16
    spacing at the largest magnitude the computed value can have (at most u16 of it, half of that at the top of a binade)."""
    if op:
        err = err + U32 * (val.abs() + err)
    return err + 0.5 * ulp16(val.abs() + err)


def _per_channel(t, C):
    return t.repeat_interleave(C // 32, dim=1)                 # [N, 32] -> [N, C]


def _affine(mean, rstd, dm, dr, gamma, beta, C):
    """ga, gb [N, C] float64 and the bounds on their f32 forms."""
    g, b = gamma.double()[None], beta.double()[None]
    m, r, dm, dr = (_per_channel(t, C) for t in (mean, rstd, dm, dr))
    ga = r * g
    dga = g.abs() * dr + U32 * (ga.abs() + g.abs() * dr)
    gb = b - m * ga
    dgb = ga.abs() * dm + (m.abs() + dm) * dga + 2 * U32 * ((m * ga).abs() + b.abs())
    return ga, gb, dga, dgb


def _film_terms(film, C):
    f = film.half().double()
    return 1.0 + f[:, :C], f[:, C:]                            # t1 (before its own f16 rounding), sh


def pool4(t):
    """AvgPool2d(2) of [N, H, W, C] in the tensor's own arithmetic."""
    return (t[:, 0::2, 0::2] + t[:, 0::2, 1::2] + t[:, 1::2, 0::2] + t[:, 1::2, 1::2]) * 0.25


def up2(t):
    return t.repeat_interleave(2, dim=1).repeat_interleave(2, dim=2)


def gn_ref(x, gamma, beta, film, silu, resample, mean, rstd, dm, dr):
    """x [N, H, W, C] f16 values, statistics (mean, rstd) [N, 32] float64 with their bounds (dm, dr) -> (reference, bound) [N, Ho, Wo, C] float64."""
    C = x.shape[-1]
    x = x.double()
    ga, gb, dga, dgb = (t[:, None, None, :] for t in _affine(mean, rstd, dm, dr, gamma, beta, C))
    y = x * ga + gb
    E = _r16(y, x.abs() * dga + dgb)
    if film is not None:
        t1, sh = (t[:, None, None, :] for t in _film_terms(film, C))
        z = y * t1
        E = _r16(z, E * t1.abs() + (y.abs() + E) * U16 * t1.abs())
        y = z + sh
        E = _r16(y, E)
    if silu:
        s = y * torch.sigmoid(y)
        sg = torch.sigmoid(y)
        d1 = (sg * (1 + y * (1 - sg))).abs()                    # |silu'(y)|; |silu''| <= 0.5 everywhere (Taylor with the Lagrange remainder)
        E = _r16(s, d1 * E + 0.25 * E * E + (16 + y.abs()) * U32 * s.abs(), op=False)      # (|y| u32: the product y log2(e) in front of the exp2)
        y = s
    if resample == 1:
        p = pool4(y)
        E = _r16(p, pool4(E) + 4 * U32 * pool4(y.abs() + E), op=False)
        y = p
    elif resample == 2:
        y, E = up2(y), up2(E)
    return y, E


def raw_pool_ref(x):
    """AvgPool2d(2) of the raw input: (reference, bound = one f16 ulp)."""
    p = pool4(x.double())
    return p, ulp16(p)


def gn_table_ref(stats, gamma, beta, film, C):
    """stats [N, 32, 2] f32 as handed to k_gn_table (taken as exact) -> (A, B, dA, dB) [N, C] float64."""
    st = stats.double().reshape(-1, 32, 2)
    zero = torch.zeros_like(st[..., 0])
    ga, gb, dga, dgb = _affine(st[..., 0], st[..., 1], zero, zero, gamma, beta, C)
    if film is None:
        return ga, gb, dga + U32 * ga.abs(), dgb + 2 * U32 * gb.abs()
    t1, sh = _film_terms(film, C)
    A, B = ga * t1, gb * t1 + sh
    dA = dga * t1.abs() + (ga.abs() + dga) * U16 * t1.abs() + U32 * A.abs()
    dB = dgb * t1.abs() + (gb.abs() + dgb) * U16 * t1.abs() + 2 * U32 * ((gb * t1).abs() + sh.abs())
    return A, B, dA, dB


def table_columns(table, N, C):
    """table [N][C / 8][16] = (A0..A7, B0..B7) per octet -> A, B [N, C]."""
    t = table.reshape(N, C // 8, 16)
    return t[..., :8].reshape(N, C), t[..., 8:].reshape(N, C)


# resample / concat shapes: (N, H, W) non-square, with the channel splits of the concat
RESAMPLE_SHAPES = ((2, 6, 10), (1, 4, 18), (3, 2, 6))
CONCAT_SPLITS = ((8, 8), (64, 128), (256, 512))
GRID_CAP_OCTETS = 65536 * 256
