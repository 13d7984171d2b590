"""CPU: what tests/test_gpu_nn_ops.py relies on, checked without a GPU.  Every kernel of the GPU file is emulated at its documented rounding points in
f32 / f16 torch on the CPU and run on the exact inputs of the GPU cases (tests/nn_ops_common.py):

  * the honest emulation stays inside the bound on EVERY element (no mask) -- for attention with both denominator forms (the f32 sum of unrounded
    probabilities of k_attention, the sum of f16-rounded probabilities of k_attention_t64) and with f16 subnormals kept and flushed;
  * every planted bug leaves the bound on those inputs, wherever the inputs can show it at all (the exemptions are listed next to the assertion, each
    with the reason why no bound could separate the bug there).

Each test prints its largest error / bound ratio (pytest -s).  A ratio near 1 on the honest side would mean a derivation is wrong, not that a bound
needs widening.  The one GPU case left out here is the 4 x 63 x 65 x 2048 tensor of the unrolled-loop test (33 M elements; same code path as the others
in this emulation)."""
import ctypes as C
import math

import pytest
import torch

import nn_ops_common as oc


# ================================================================================================ attention
def emulate_attention(qkv, D, form, flush, bug=None):
    """The online softmax of csrc/nn_attn.hip in f32 / f16 on the CPU: chunks of 64 keys, running maximum m, rescale factor alpha, probabilities rounded to
    f16 for the PV product (flush: f16 subnormals read as zero), denominator from the unrounded ('f32') or the rounded ('mfma') probabilities, o / l -> f16."""
    N, T, C3 = qkv.shape
    Cc = C3 // 3
    heads, nch = Cc // D, T // 64
    x = qkv.float().reshape(N, T, heads, 3, D)
    out = torch.empty((N, T, Cc), dtype=torch.float16)
    jb = min(1, nch - 1)                                       # the chunk the tile bugs act on
    tile = torch.zeros((T,), dtype=torch.bool)
    tile[16:32] = True
    for n in range(N):
        for h in range(heads):
            q, k, v = x[n, :, h, 0], x[n, :, h, 1], x[n, :, h, 2]
            if bug == 'kv_swap' and n == 0 and h == 0:
                k, v = v, k
            S = (q @ k.T) * torch.tensor(D ** -0.25 if bug == 'quarter_scale' else 1.0 / math.sqrt(D), dtype=torch.float32)
            m = torch.full((T,), -math.inf)
            l, o = torch.zeros((T,)), torch.zeros((T, D))
            visits = [(j, None) for j in range(nch)]
            if bug == 'chunk_twice':
                visits.insert(jb + 1, (jb, tile))
            for j, rows in visits:
                sc = S[:, 64 * j:64 * j + 64]
                mn = torch.maximum(m, sc.max(dim=-1).values)
                alpha = torch.exp(m - mn)
                p = torch.exp(sc - mn[:, None])
                p16 = p.half()
                if flush:
                    p16 = torch.where(p16.float().abs() < oc.MIN16, torch.zeros_like(p16), p16)
                psum = p.sum(dim=-1) if form == 'f32' else p16.float().sum(dim=-1)
                if bug == 'key_swap' and j == 0:                # keys 4 and 5 against each other's values (one 4-key group)
                    p16 = p16.clone()
                    p16[:, [4, 5]] = p16[:, [5, 4]]
                ln = (l if bug == 'no_rescale' else l * alpha) + psum
                on = o * alpha[:, None] + p16.float() @ v[64 * j:64 * j + 64]
                act = torch.ones((T,), dtype=torch.bool) if rows is None else rows
                if bug == 'chunk_skip' and j == jb:
                    act = ~tile
                m, l, o = torch.where(act, mn, m), torch.where(act, ln, l), torch.where(act[:, None], on, o)
            out[n, :, h * D:(h + 1) * D] = (o / l[:, None]).half()
    return out


ATT_BUGS = ('chunk_skip', 'chunk_twice', 'no_rescale', 'quarter_scale', 'kv_swap', 'key_swap')


def _att_exempt(bug, T, regime):
    """Where the inputs cannot show a bug, whatever the bound."""
    if regime == 'flat' and bug in ('quarter_scale', 'key_swap', 'no_rescale'):
        return "flat logits: all weights are 1 / T to 0.3 %, so neither the logit scale nor which key a weight belongs to nor the maximum matters"
    if T == 64 and bug in ('chunk_twice', 'no_rescale'):
        return "a single chunk: visiting it twice doubles numerator and denominator alike, and nothing is ever rescaled"
    return None


@pytest.fixture(scope="module")
def att_refs():
    refs = {}
    for name, kernel, N, T, Cc, D, regime in oc.ATT_CASES:
        key = (N, T, Cc, D, regime)
        if key not in refs:
            qkv = oc.attention_inputs(N, T, Cc, D, regime)
            refs[key] = (qkv, oc.attention_ref(qkv, D))
    return refs


@pytest.mark.parametrize("case", oc.ATT_CASES, ids=[c[0] for c in oc.ATT_CASES])
def test_attention_emulation_inside_the_bound_and_planted_bugs_outside(att_refs, case):
    name, kernel, N, T, Cc, D, regime = case
    qkv, ref = att_refs[(N, T, Cc, D, regime)]
    form = oc.attention_form(kernel)
    bound = oc.attention_bound(ref, T, D, form)
    if regime == 'jump':
        for n in range(N):
            for h in range(Cc // D):
                for tq, tk in oc.jump_pairs(n, h, T):
                    assert tk >= T - 64 and tq < T - 64
        assert float(ref['subD'].max()) > 0                    # the jump pushes the other keys of those rows below the f16 normal range
    for flush in (False, True):
        r = oc.worst_ratio(emulate_attention(qkv, D, form, flush), ref['o'], bound)
        print(f"attention {name} form={form} flush={int(flush)}: honest ratio {r:.3f}")
        assert r < 1.0, (name, form, flush, r)
    for bug in ATT_BUGS:
        r = oc.worst_ratio(emulate_attention(qkv, D, form, False, bug), ref['o'], bound)
        why = _att_exempt(bug, T, regime)
        print(f"attention {name} bug={bug}: ratio {r:.3g}" + (f"   (exempt: {why})" if why else ""))
        if why is None:
            assert r > 1.0, (name, bug, r)


def test_attention_bound_has_no_global_term():
    """Scaling v of ONE head by 2^-6 scales that head's bound with it (up to the 2^-25 floor) and leaves the other heads' bounds alone."""
    N, T, Cc, D = 1, 128, 128, 64
    qkv = oc.attention_inputs(N, T, Cc, D, 'moderate')
    small = qkv.clone()
    small[:, :, 2 * D:3 * D] = (small[:, :, 2 * D:3 * D].float() / 64).half()
    b0 = oc.attention_bound(oc.attention_ref(qkv, D), T, D, 'mfma')
    b1 = oc.attention_bound(oc.attention_ref(small, D), T, D, 'mfma')
    assert torch.equal(b0[..., D:], b1[..., D:])
    assert float((b1[..., :D] / b0[..., :D]).max()) < 1.0 / 32


# ================================================================================================ GroupNorm
def emulate_stats(x):
    """(mean, rstd) [N, 32] f32 from f32 sums (torch's own summation order), combined in f64 like k_gn_finalize."""
    N, Cc = x.shape[0], x.shape[-1]
    g = x.float().reshape(N, -1, 32, Cc // 32).permute(0, 2, 1, 3).reshape(N, 32, -1)
    s, q = g.sum(dim=-1).double(), (g * g).sum(dim=-1).double()
    mean = s / g.shape[-1]
    var = (q / g.shape[-1] - mean * mean).clamp(min=0)
    return mean.float(), ((var + oc.EPS) ** -0.5).float()


def _pool_f32(f, bug):
    a, b, c, d = f[:, 0::2, 0::2], f[:, 0::2, 1::2], f[:, 1::2, 0::2], f[:, 1::2, 1::2]
    if bug == 'pool_twice':
        d = c
    return (a + b + c + d) * 0.25


def emulate_gn(x, gamma, beta, film, silu, resample, mean, rstd, bug=None, Ca=0):
    """gn_elem (csrc/nn_common.h) and k_gn_apply's resampling in f32 / f16 torch; mean, rstd [N, 32] f32."""
    N, H, W, Cc = x.shape
    cg = Cc // 32
    grp = torch.arange(Cc) // cg
    if bug == 'group_shift':                                   # the second source indexes its statistics one group low
        grp[Ca:] = (grp[Ca:] - 1).clamp(min=0)
    m, r = mean[:, grp], rstd[:, grp]
    if bug == 'rstd':
        r = r * (1 + 2.0 ** -9)
    ga = r * gamma[None]
    gb = beta[None] - m * ga
    f = (x.float() * ga[:, None, None] + gb[:, None, None]).half().float()
    if film is not None:
        sc, sh = film[:, :Cc].clone(), film[:, Cc:].clone()
        if bug == 'film_swap':                                 # scale and shift halves exchanged in the second octet
            sc[:, 8:16], sh[:, 8:16] = film[:, Cc + 8:Cc + 16], film[:, 8:16]
        t1 = (1.0 + sc.half().float()).half().float()
        f = (f * t1[:, None, None]).half().float()
        f = (f + sh.half().float()[:, None, None]).half().float()
    if silu:
        f = (f / (1.0 + torch.exp(-f))).half().float()
    if bug == 'hw_swap' and resample:                          # yo = p / Ho: the image walked as W rows of H pixels
        f = f.reshape(N, W, H, Cc)
    if resample == 1:
        f = _pool_f32(f, bug).half().float()
    elif resample == 2:
        f = oc.up2(f)
    if bug == 'hw_swap' and resample:
        f = f.reshape(N, H // 2 if resample == 1 else 2 * H, W // 2 if resample == 1 else 2 * W, Cc)
    out = f.half()
    if bug == 'tail':                                          # the last pixel keeps the NaN the buffer was filled with
        out[-1, -1, -1, :] = float('nan')
    return out


def _gn_case(N, H, W, Cc):
    x, gamma, beta, film = oc.gn_inputs(N, H, W, Cc)
    mean, rstd = oc.gn_stats_ref(x)
    dm, dr = oc.gn_stats_bounds(x, oc.partial_terms(Cc))
    return x, gamma, beta, film, mean, rstd, dm, dr


@pytest.mark.parametrize("H,W", oc.GN_SIZES)
@pytest.mark.parametrize("Cc", oc.GN_CHANNELS)
def test_groupnorm_emulation_inside_the_bound_and_planted_bugs_outside(Cc, H, W):
    x, gamma, beta, film, mean, rstd, dm, dr = _gn_case(oc.GN_N, H, W, Cc)
    m32, r32 = emulate_stats(x)
    rs = max(float(((m32.double() - mean).abs() / dm).max()), float(((r32.double() - rstd).abs() / dr).max()))
    print(f"gn statistics C={Cc} {H}x{W}: honest ratio {rs:.3f}")
    assert rs < 1.0
    # the last pixel of the partial chunk never read (the first counted twice in its place) leaves the statistics bound
    mb, rb = emulate_stats(torch.cat([x.reshape(oc.GN_N, H * W, 1, Cc)[:, :-1], x.reshape(oc.GN_N, H * W, 1, Cc)[:, :1]], dim=1))
    assert float(((mb.double() - mean).abs() / dm).max()) > 1.0
    worst = 0.0
    for fl, silu, res in oc.GN_FLAGS:
        fm = film if fl else None
        ref, bound = oc.gn_ref(x, gamma, beta, fm, silu, res, mean, rstd, dm, dr)
        r = oc.worst_ratio(emulate_gn(x, gamma, beta, fm, silu, res, m32, r32), ref, bound)
        worst = max(worst, r)
        assert r < 1.0, (fl, silu, res, r)
        bugs = ['rstd', 'tail'] + (['film_swap'] if fl else []) + (['pool_twice'] if res == 1 else []) + (['hw_swap'] if res and H != W else [])
        for bug in bugs:
            rb_ = oc.worst_ratio(emulate_gn(x, gamma, beta, fm, silu, res, m32, r32, bug), ref, bound)
            print(f"gn C={Cc} {H}x{W} film={fl} silu={silu} res={res} bug={bug}: ratio {rb_:.3g}")
            assert rb_ > 1.0, (bug, fl, silu, res, rb_)
    print(f"gn apply C={Cc} {H}x{W}: honest ratio {worst:.3f} over {len(oc.GN_FLAGS)} flag sets")


@pytest.mark.parametrize("Ca,Cc", oc.GN_TWO_SOURCE)
def test_groupnorm_two_source_neighbouring_group_statistics(Ca, Cc):
    """Finished statistics handed over as f32(float64 statistics): dm = u32 |mean|, dr = u32 rstd."""
    N, H, W = 2, 6, 10
    x, gamma, beta, film = oc.gn_inputs(N, H, W, Cc)
    mean, rstd = oc.gn_stats_ref(x)
    dm, dr = oc.U32 * mean.abs(), oc.U32 * rstd
    for fl, silu, res in oc.GN_FLAGS:
        fm = film if fl else None
        ref, bound = oc.gn_ref(x, gamma, beta, fm, silu, res, mean, rstd, dm, dr)
        r = oc.worst_ratio(emulate_gn(x, gamma, beta, fm, silu, res, mean.float(), rstd.float()), ref, bound)
        rb = oc.worst_ratio(emulate_gn(x, gamma, beta, fm, silu, res, mean.float(), rstd.float(), 'group_shift', Ca), ref, bound)
        print(f"gn two-source Ca={Ca} C={Cc} film={fl} silu={silu} res={res}: honest ratio {r:.3f}, neighbouring group's statistics {rb:.3g}")
        assert r < 1.0 and rb > 1.0, (fl, silu, res, r, rb)


def test_octet_partial_statistics_bound_holds_for_f32_sums():
    """Statistics from octet partials (n = 8 HW / chunks per source, the sources chunked differently): f32 sums per (chunk, octet), f64 combine."""
    N, H, W, Ca, Cc = 2, 16, 18, 256, 768
    x = oc.gn_inputs(N, H, W, Cc)[0]
    HW = H * W
    parts = []
    for t, ch in ((x[..., :Ca], 2), (x[..., Ca:], 3)):
        v = t.float().reshape(N, ch, HW // ch, t.shape[-1] // 8, 8)
        parts.append((v.sum(dim=(2, 4)).double().sum(dim=1), (v * v).sum(dim=(2, 4)).double().sum(dim=1)))       # [N, octets]
    S, Q = torch.cat([p[0] for p in parts], dim=1), torch.cat([p[1] for p in parts], dim=1)
    opg = Cc // 32 // 8
    cnt = HW * (Cc // 32)
    m = S.reshape(N, 32, opg).sum(-1) / cnt
    var = (Q.reshape(N, 32, opg).sum(-1) / cnt - m * m).clamp(min=0)
    r = (var + oc.EPS) ** -0.5
    nt = torch.cat([torch.full((Ca,), 8.0 * HW / 2), torch.full((Cc - Ca,), 8.0 * HW / 3)])
    mean, rstd = oc.gn_stats_ref(x)
    dm, dr = oc.gn_stats_bounds(x, nt)
    ratio = max(float(((m.float().double() - mean).abs() / dm).max()), float(((r.float().double() - rstd).abs() / dr).max()))
    print(f"gn octet-partial statistics: honest ratio {ratio:.3f}")
    assert ratio < 1.0


def test_raw_pool_bound_is_one_f16_ulp():
    x = oc.gn_inputs(3, 6, 10, 96)[0]
    ref, bound = oc.raw_pool_ref(x)
    got = _pool_f32(x.float(), None).half()
    assert oc.worst_ratio(got, ref, bound) <= 0.5 + 1e-3       # f32 sum of four f16 values, one rounding to f16
    assert oc.worst_ratio(_pool_f32(x.float(), 'pool_twice').half(), ref, bound) > 1.0
    assert float(oc.ulp16(torch.tensor([1.0, 1.5, 2.0, 1e-6], dtype=torch.float64))[3]) == 2.0 ** -24
    assert oc.ulp16(torch.tensor([1.0, 1.5, 2.0], dtype=torch.float64)).tolist() == [2.0 ** -10, 2.0 ** -10, 2.0 ** -9]


@pytest.mark.parametrize("Cc", [32, 160, 2048])
@pytest.mark.parametrize("fl", [0, 1])
def test_gn_table_emulation_inside_the_bound(fl, Cc):
    N = 3
    _, gamma, beta, film = oc.gn_inputs(N, 2, 2, Cc)
    g = torch.Generator().manual_seed(Cc)
    stats = torch.stack([torch.randn((N, 32), generator=g), 0.5 + 1.5 * torch.rand((N, 32), generator=g)], dim=-1)
    fm = film if fl else None
    A, B, dA, dB = oc.gn_table_ref(stats, gamma, beta, fm, Cc)
    grp = torch.arange(Cc) // (Cc // 32)
    ga = stats[:, grp, 1] * gamma[None]
    gb = beta[None] - stats[:, grp, 0] * ga

    def table(swap=False):
        if not fl:
            return ga, gb
        sc, sh = (film[:, Cc:], film[:, :Cc]) if swap else (film[:, :Cc], film[:, Cc:])
        t1 = (1.0 + sc.half().float()).half().float()
        return ga * t1, gb * t1 + sh.half().float()
    a, b = table()
    r = max(oc.worst_ratio(a, A, dA), oc.worst_ratio(b, B, dB))
    print(f"gn table C={Cc} film={fl}: honest ratio {r:.3f}")
    assert r < 1.0
    if fl:
        a, b = table(swap=True)
        assert oc.worst_ratio(a, A, dA) > 1.0 and oc.worst_ratio(b, B, dB) > 1.0
    assert oc.worst_ratio(gb, A, dA) > 1.0                     # the A and B halves of an octet row exchanged
    t = torch.arange(2 * 16 * 16, dtype=torch.float32).reshape(2, 16, 16)
    At, Bt = oc.table_columns(t, 2, 128)
    assert At[1, 9] == 256 + 16 + 1 and Bt[1, 9] == 256 + 16 + 8 + 1


# ---- the entries refuse on the host (every check precedes the first launch: no GPU is touched)
def test_new_entries_refuse_bad_arguments():
    import __graft_entry__ as ge
    ge.build()
    from pointdreamer_amd import _lib
    import pointdreamer_amd.ddnm_inpainting  # noqa: F401
    L = _lib.lib()
    buf = (C.c_float * 4)()
    p = C.cast(buf, C.c_void_p)

    def apply(x2=None, Ca=0, Cc=256, stats=p, pa=None, cha=0, pb=None, chb=0, film=None, res=0, yraw=None, H=4, W=4):
        return L.pdhip_gn_apply_f16(p, x2, Ca, Cc, stats, pa, cha, pb, chb, p, p, film, 2 * Cc, 1, H, W, 1, res, p, yraw, None)
    assert apply(pa=p, cha=1) == -1 and b'pdhip_gn_apply_f16' in L.pdhip_last_error()          # finished statistics and partials
    assert apply(stats=None) == -1                                                              # neither
    assert apply(stats=None, pa=p, cha=0) == -1                                                 # partials without a chunk count
    assert apply(x2=p, Ca=64, stats=None, pa=p, cha=1) == -1                                    # two sources, one set of partials
    assert apply(Cc=96, stats=None, pa=p, cha=1) == -1 and b'octet partials' in L.pdhip_last_error()   # group size no multiple of 8
    assert apply(film=p, res=1) == -1 and b'FiLM only without resampling' in L.pdhip_last_error()
    assert apply(res=1, H=3) == -1 and b'even H, W' in L.pdhip_last_error()
    assert apply(yraw=p, res=2) == -1 and b'raw avg-pool' in L.pdhip_last_error()
    assert apply(x2=p, Ca=64, yraw=p, res=1) == -1
    assert apply(x2=p, Ca=260) == -1 and b'two-source split' in L.pdhip_last_error()
    assert apply(Cc=48) == -1
    assert L.pdhip_gn_table_f32(p, p, p, None, 0, 1, 48, p, None) == -1 and b'gn_table' in L.pdhip_last_error()
    assert L.pdhip_gn_table_f32(p, p, p, p, 32, 1, 32, p, None) == -1
    assert L.pdhip_gn_table_f32(None, p, p, None, 0, 1, 32, p, None) == -1
    assert L.pdhip_resample2x_nhwc_f16(p, 1, 4, 4, 8, 3, p, None) == -1 and b'resample2x' in L.pdhip_last_error()
    assert L.pdhip_resample2x_nhwc_f16(p, 1, 4, 4, 12, 2, p, None) == -1
    assert L.pdhip_resample2x_nhwc_f16(p, 1, 3, 4, 8, 1, p, None) == -1 and b'even H, W' in L.pdhip_last_error()
    assert L.pdhip_concat_channels_f16(p, 8, p, 12, 4, p, None) == -1 and b'multiples of 8' in L.pdhip_last_error()
    assert L.pdhip_concat_channels_f16(p, 8, None, 8, 4, p, None) == -1
