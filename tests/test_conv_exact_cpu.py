"""CPU: the bit-equality comparison of tests/test_gpu_conv_exact.py (tests/conv_exact_common.py) has teeth.  A conv kernel is emulated in plain torch --
f32 products and sums per channel chunk and tap, the chunks combined in f32 like split-K partials, then bias, the two roundings and the residual -- and
    * the honest emulation reproduces the float64 reference bit for bit under every channel permutation, 1 .. 4 K-chunks and both tap orders, at
      K = 576, 9216 and 27648;
    * the reference refuses operands for which that would not be guaranteed;
    * each way a kernel goes subtly wrong is caught -- and at K = 9216 the rounding-form and single-product mistakes PASS the max-norm bound
      2e-3 max|ref| + 1e-3 the older conv tests assert: the gap this comparison closes;
and every further case of the GPU test that goes through pdhip_debug_conv_launch_nhwc_f16 is planned onto the kernel it names (host code, no launch)."""
import ctypes as C
import itertools

import pytest
import torch
import torch.nn.functional as F

import conv_epilogue_common as ce
import conv_exact_common as cx

N, H, W, COUT = 2, 8, 8, 32
CIN_OF_K = {576: 64, 9216: 1024, 27648: 3072}
_OPS = {}


def operands(K, res_hw=None):
    key = (K, res_hw)
    if key not in _OPS:
        _OPS[key] = cx.make_exact_operands(N, H, W, CIN_OF_K[K], COUT, 9, True, 7 * K + (1 if res_hw else 0), res_hw=res_hw)
    return _OPS[key]


_WANT = {}


def want(K, res_hw=None):
    if (K, res_hw) not in _WANT:
        _WANT[(K, res_hw)] = cx.expected_f16(operands(K, res_hw), cx.FORM_BIAS_THEN_RESIDUAL, f"cpu K {K}")
    return _WANT[(K, res_hw)]


# ---- f32 -> f16 conversions a kernel might use instead of round-to-nearest-even
def _step_toward_zero(h):
    b = h.view(torch.int16).to(torch.int32) & 0xFFFF
    b = (b & 0x8000) | ((b & 0x7FFF) - 1)
    return (b - ((b & 0x8000) << 1)).to(torch.int16).view(torch.float16)


def f16_truncate(v):
    h = v.half()
    over = h.double().abs() > v.double().abs()
    return torch.where(over, _step_toward_zero(h), h)


def f16_ties_away(v):
    lo = f16_truncate(v)                                   # |lo| <= |v| < |hi|, neighbours in f16
    b = lo.view(torch.int16).to(torch.int32) & 0xFFFF
    b = (b & 0x8000) | ((b & 0x7FFF) + 1)
    hi = (b - ((b & 0x8000) << 1)).to(torch.int16).view(torch.float16)
    tie = (v.double() - lo.double()).abs() == (hi.double() - v.double()).abs()
    return torch.where(tie & (lo.double() != v.double()), hi, v.half())


def emulate(op, perm=None, chunks=1, tap_order=None, mutant=None):
    """An emulated conv kernel: y [N, H, W, Cout] f16.  perm: channel order of the K loop; chunks: K cut in that many channel chunks, each summed in f32 on
    its own, the partial tiles then added in f32 in order; tap_order: order of the nine taps inside a chunk.  mutant: one of MUTANTS."""
    x, w, b, r = op['x'], op['w'], op['b'], op['r']
    Cin = x.shape[1]
    perm = torch.arange(Cin) if perm is None else perm
    taps = tap_order or [(ky, kx) for ky in range(3) for kx in range(3)]
    xp = F.pad(x, (1, 1, 1, 1))
    parts = []
    for idx in torch.chunk(perm, chunks):
        acc = torch.zeros((N, COUT, H, W), dtype=torch.float32)
        for ky, kx in taps:
            acc = acc + torch.einsum('nchw,oc->nohw', xp[:, idx, ky:ky + H, kx:kx + W], w[:, idx, ky, kx])
        parts.append(acc)
    if mutant == 'f16 split-K partials':
        parts = [p.half().float() for p in parts]
    S = parts[0]
    for p in parts[1:]:
        S = S + p
    if mutant in ('interior product dropped', 'border product added'):
        S = S.clone()
        n, py, px = 1, (3, 0)[mutant.startswith('border')], 4
        ky, kx = (1, 1) if mutant.startswith('interior') else (0, 1)            # border: the tap above row 0 reads the padding ...
        sy = min(max(py + ky - 1, 0), H - 1)                                     # ... a kernel that clamps reads the edge pixel instead
        c = int(torch.nonzero(x[n, :, sy, px + kx - 1].abs() == 0.25)[0])        # a product of middling size: |x| = 1 / 4, |w| <= 1 / 16
        delta = x[n, c, sy, px + kx - 1] * w[:, c, ky, kx]
        S[n, :, py, px] += delta if mutant.startswith('border') else -delta
    if r.shape[-1] != W:
        if mutant == 'half-resolution residual at (y >> 1, x)':
            flat = r.reshape(N, COUT, -1)
            yy, xx = torch.meshgrid(torch.arange(H), torch.arange(W), indexing='ij')
            r = flat[:, :, ((yy >> 1) * (W >> 1) + xx).reshape(-1) % flat.shape[-1]].reshape(N, COUT, H, W)
        else:
            r = F.interpolate(r, scale_factor=2, mode='nearest')
    if mutant == 'residual of image n - 1':
        r = torch.roll(r, 1, dims=0)
    bb = b[None, :, None, None]
    if mutant == 'single rounding':
        y = ((S + bb) + r).half()
    elif mutant == 'truncation':
        y = f16_truncate(f16_truncate(S + bb).float() + r)
    elif mutant == 'ties away from zero':
        y = f16_ties_away(f16_ties_away(S + bb).float() + r)
    elif mutant == 'bias after the first rounding':
        y = ((S.half().float() + bb) + r).half()
    else:
        y = ((S + bb).half().float() + r).half()
    return y.permute(0, 2, 3, 1).contiguous()


# mutant -> does the older max-norm bound see it?  The residual-index mistakes are O(1) errors by the construction of the residual (a scale and an offset per
# image): they are listed for the comparison's sake, the older bound tells them too.
MUTANTS = {'single rounding': False, 'truncation': False, 'ties away from zero': False, 'f16 split-K partials': False, 'interior product dropped': False,
           'border product added': False, 'bias after the first rounding': False, 'residual of image n - 1': True,
           'half-resolution residual at (y >> 1, x)': True}


def old_bound_passes(y, op):
    ref = ce.reference_f64(op)
    return (y.double() - ref).abs().max().item() <= 2e-3 * ref.abs().max().item() + 1e-3


def test_rounding_helpers_are_what_they_say():
    v = torch.tensor([1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, -(1.0 + 2.0 ** -11), 1.0 + 2.0 ** -12, 1.0 + 2.0 ** -10, -3.0 - 2.0 ** -10 - 2.0 ** -13])
    assert v.half().tolist() == [1.0, 1.0 + 2.0 ** -9, -1.0, 1.0, 1.0 + 2.0 ** -10, -3.0 - 2.0 ** -9]                  # nearest, ties to even
    assert f16_truncate(v).tolist() == [1.0, 1.0 + 2.0 ** -10, -1.0, 1.0, 1.0 + 2.0 ** -10, -3.0]
    assert f16_ties_away(v).tolist() == [1.0 + 2.0 ** -10, 1.0 + 2.0 ** -9, -1.0 - 2.0 ** -10, 1.0, 1.0 + 2.0 ** -10, -3.0 - 2.0 ** -9]


@pytest.mark.parametrize("K", [576, 9216, 27648])
def test_honest_emulation_is_bit_identical_in_any_order(K):
    op = operands(K)
    g = torch.Generator().manual_seed(K)
    perms = [None, torch.randperm(CIN_OF_K[K], generator=g), torch.arange(CIN_OF_K[K]).flip(0)]
    nat = [(ky, kx) for ky in range(3) for kx in range(3)]
    orders = [nat, nat[::-1], [nat[i] for i in (4, 0, 8, 2, 6, 1, 7, 3, 5)]]
    for perm, chunks, order in itertools.product(perms, (1, 2, 3, 4), orders):
        assert cx.mismatches(emulate(op, perm, chunks, order), want(K)) == [], (chunks, order)
    # the construction exercises the roundings: a fair share of S + b is no f16 number, and the two rounding forms differ
    S, headroom = cx.exact_sum_f64(op)
    inexact = (S.half().double() != S).double().mean().item()
    forms = (emulate(op, mutant='single rounding') != want(K)).double().mean().item()
    print(f"K {K}: headroom {headroom:.1f}, S + b not f16-representable {inexact:.1%}, single != double rounding {forms:.1%}, output std {want(K).float().std():.2f}")
    assert inexact >= {576: 0.15, 9216: 0.45, 27648: 0.55}[K] and forms >= 0.05
    # half-resolution residual
    assert cx.mismatches(emulate(operands(K, (4, 4)), perms[1], 3, orders[1]), want(K, (4, 4))) == []


def test_the_reference_refuses_operands_that_are_not_exactly_summable():
    op = operands(9216)
    _, headroom = cx.exact_sum_f64(op)
    assert 20 < headroom < 35
    with pytest.raises(cx.NotExact, match='8192'):                      # w scaled (still on its grid) until the sum bound passes 8192
        cx.expected_f16(dict(op, w=op['w'] * 32), cx.FORM_BIAS_THEN_RESIDUAL)
    cx.expected_f16(dict(op, w=op['w'] * 16), cx.FORM_BIAS_THEN_RESIDUAL)
    x = op['x'].clone()
    x[0, 0, 0, 0] += 2.0 ** -4                                           # one more fractional bit than the budget: products of 2^-12
    with pytest.raises(cx.NotExact, match='grids'):
        cx.expected_f16(dict(op, x=x), cx.FORM_BIAS_THEN_RESIDUAL)
    with pytest.raises(cx.NotExact, match='grids'):
        cx.expected_f16(dict(op, b=op['b'] + 2.0 ** -12), cx.FORM_BIAS_THEN_RESIDUAL)
    with pytest.raises(AssertionError):                                  # a residual that is no f16 tensor
        cx.expected_f16(dict(op, r=op['r'] + 2.0 ** -20), cx.FORM_BIAS_THEN_RESIDUAL)


@pytest.mark.parametrize("K", [576, 9216, 27648])
@pytest.mark.parametrize("mutant", list(MUTANTS))
def test_each_mistake_is_caught_and_the_old_bound_lets_the_subtle_ones_pass(K, mutant):
    half = mutant.startswith('half-resolution')
    op = operands(K, (4, 4) if half else None)
    y = emulate(op, chunks=4, mutant=mutant)
    lines = cx.mismatches(y, want(K, (4, 4) if half else None), tile=4)
    assert lines != [], mutant
    print('\n'.join(lines))
    assert old_bound_passes(want(K, (4, 4) if half else None), op)                        # (the reference itself is inside the old bound)
    if K == 9216:
        assert old_bound_passes(y, op) == (not MUTANTS[mutant]), mutant                    # the written proof of the gap
    if mutant in ('interior product dropped', 'border product added'):                     # one pixel: the report says where it sits
        text = '\n'.join(lines)
        assert 'pixels hit 1 of' in text and ('border pixels 0 ' if mutant.startswith('interior') else ', interior 0;') in text


def test_mismatches_reports_unwritten_elements_and_ignores_the_sign_of_zero():
    a = want(576).clone()
    b = a.clone()
    b[0, 0, 0, 0] = float('nan')
    lines = cx.mismatches(b, a)
    assert lines and '1 of them NaN' in lines[0] and 'NaN' in lines[1]
    z = torch.zeros((1, 2, 2, 8), dtype=torch.float16)
    assert cx.mismatches(-z, z) == []
    z2 = z.clone()
    z2[0, 1, 1, 3] = 2.0 ** -24                                         # the smallest subnormal: one ulp from zero
    lines = cx.mismatches(z2, z, tile=(2, 2))
    assert lines and '1 ulps apart' in lines[1] and 'row mod 2: 1:1' in lines[-1]


def test_phase_weight_sums_are_exact_f16_and_give_the_up_conv():
    """conv3x3(nearest_x2(x)) == the four 2x2 phase convs with the summed taps, in float64, on the exact operands."""
    op = cx.make_exact_operands(2, 5, 6, 8, 4, 9, False, 3)
    ref = cx.exact_sum_f64(cx.up2_operands(op))[0]
    wph = cx.phase_weights_f64(op['w'])
    x = F.pad(op['x'].double(), (1, 1, 1, 1))
    for py in range(2):
        for px in range(2):
            acc = op['b'].double()[None, :, None, None]
            for ty in range(2):
                for tx in range(2):
                    sy, sx = py + ty, px + tx                            # source window of phase (py, px): rows y - 1 + py + ty of the padded half-resolution image
                    acc = acc + torch.einsum('nchw,oc->nohw', x[:, :, sy:sy + 5, sx:sx + 6], wph[2 * py + px, :, 2 * ty + tx, :])
            assert torch.equal(acc, ref[:, :, py::2, px::2])


# ---- routing of the GPU test's further cases, on the host
@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as ge
    ge.build()
    from pointdreamer_amd import _lib
    import pointdreamer_amd.ddnm_inpainting  # noqa: F401  (registers the entry points)
    return _lib.lib()


@pytest.mark.parametrize("c", cx.EXTRA_CASES, ids=[c['name'] for c in cx.EXTRA_CASES])
def test_every_further_gpu_case_is_planned_onto_the_kernel_it_names(L, c):
    fake = C.c_void_p(4096)
    k, ch = C.c_int(-1), C.c_int(-1)
    pad = (c['Cout'] + 127) // 128 * 128
    wsf = ce.workspace_floats(c)
    with cx.LabHooks(L, c):
        rc = L.pdhip_debug_conv_launch_nhwc_f16(fake, fake if c['x2'] else None, c['x2'], fake, fake, fake if c['res'] else None, 1 if c['res_up'] else 0,
                                                None, None, 0, 0, fake, c['N'], c['H'], c['W'], c['Cin'], c['Cout'], pad, c['taps'], fake,
                                                fake if wsf else None, wsf, fake, -1, C.byref(ch), C.byref(k), None)
    # refused for the partial buffer alone (or planned without partials: a geometry that leaves none): nothing else was wrong
    assert rc == -1 and b'gn_part holds' in L.pdhip_last_error(), L.pdhip_last_error()
    assert k.value == ce.KERNELS[c['kernel']], k.value


@pytest.mark.parametrize("N,HW,Cin,Cout,res,slabs", cx.HT_CASES)
def test_ht_cases_take_the_slab_count_they_name(L, N, HW, Cin, Cout, res, slabs):
    pad = (Cout + 63) // 64 * 64
    old = L.pdhip_debug_set_conv_ht(2, slabs)
    try:
        routed, s = C.c_int(-1), C.c_int(-1)
        assert L.pdhip_conv_ht_plan(N, HW, HW, Cin, Cout, pad, cx.ht_workspace_floats(N, HW, pad), C.byref(routed), C.byref(s)) == 0
    finally:
        L.pdhip_debug_set_conv_ht(old, 0)
    assert routed.value == 1 and s.value == cx.ht_slabs_taken(Cin, slabs)
