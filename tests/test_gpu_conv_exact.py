"""GPU: every conv main loop held to BIT EQUALITY with a float64 reference on exactly summable operands (tests/conv_exact_common.py: f32 accumulation of
these operands is exact in any order, so the kernel's output is one determined f16 tensor; tests/test_conv_exact_cpu.py proves the comparison's teeth and
that the max-norm bound of the older conv tests lets a wrong rounding form or one wrong product of 9216 pass).

    * k_conv_igemm (four geometries x K-step x stages, direct and split + k_splitk_reduce), the halo-resident kernel (row tiles, 128-column strips, split,
      residual at half resolution), k_conv_sk (four tiles x in-launch split-K x stages / K-groups / tile order, two-source 1x1, skip 1x1 appended, residual
      at half resolution) -- through pdhip_debug_conv_launch_nhwc_f16, the kernel code asserted;
    * k_conv_rr with raw input (every tile variant x slabs, two-tensor source, appended skip, both residual forms, 1x1), k_conv_ht (slabs, padded Cout);
    * the four-phase up conv, its weight table, and the 9-tap halo form of the same layer;
    * the sk output of the one-pass GroupNorm + skip 1x1 kernel.
Every output is prefilled with NaN; a ticket workspace must be back at zero after the launch."""
import ctypes as C

import pytest
import torch

import conv_epilogue_common as ce
import conv_exact_common as cx

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
GUARD = 0x7F8ABCDE            # bit pattern of the floats behind the partials (a NaN payload no kernel produces)
TAIL = 4096


@pytest.fixture(scope="module")
def L():
    assert torch.cuda.is_available()
    from pointdreamer_amd import _lib
    import pointdreamer_amd.ddnm_inpainting  # noqa: F401  (registers the entry points)
    yield _lib.lib()
    if cx.HEADROOM:
        k = min(cx.HEADROOM, key=cx.HEADROOM.get)
        print(f"\nsmallest headroom over {len(cx.HEADROOM)} references: {cx.HEADROOM[k]:.2f} ({k})")


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous().half().to(DEV)


def _pack(L, w, pad):
    """w [Cout, Cin, k, k] f32 -> the engine's [pad][k k Cin] f16 layout (rows >= Cout zero)."""
    Cout, Cin, k = w.shape[0], w.shape[1], w.shape[2]
    wp = torch.zeros((pad, k * k * Cin), dtype=torch.float16, device=DEV)
    wd = w.contiguous().float().to(DEV)
    assert L.pdhip_pack_conv_weight_f16(_ptr(wd), Cout, Cin, k * k, _ptr(wp), _stream()) == 0
    torch.cuda.synchronize()
    return wp


# one reference per distinct operand set, shared by the cases that differ in hooks only (the last few are kept)
_REFS = {}


def operands_and_reference(N, H, W, Cin, Cout, taps, res, Cs=0, res_hw=None, up=False):
    key = (N, H, W, Cin, Cout, taps, bool(res), Cs, res_hw, up)
    if key not in _REFS:
        while len(_REFS) >= 4:
            _REFS.pop(next(iter(_REFS)))
        seed = 1 + sum(int(v) * m for v, m in zip((N, H, W, Cin, Cout, taps, bool(res), Cs, (res_hw or (0,))[0]), (3, 5, 7, 11, 13, 17, 19, 23, 29)))
        op = cx.make_exact_operands(N, H, W, Cin, Cout, taps, res, seed, Cs=Cs, res_hw=res_hw)
        ref = cx.up2_operands(op) if up else op
        _REFS[key] = (op, cx.expected_f16(ref, cx.form_of(op), f"{'up ' if up else ''}{key[:6]} res {res} Cs {Cs}"))
    return _REFS[key]


def assert_equal(y, want, tile=None):
    lines = cx.mismatches(y, want, tile)
    assert lines == [], '\n' + '\n'.join(lines)


def assert_tickets_zero(ws):
    if ws is not None:
        assert int((ws[:4096].view(torch.int32) != 0).sum()) == 0, "the ticket words are not back at zero"


# ---- through pdhip_debug_conv_launch_nhwc_f16
def launch(L, c, op):
    """One pdhip_debug_conv_launch_nhwc_f16 under the hooks of case c: planned first (for the size of the partial buffer), then launched with every
    operand of the case.  Returns (y [N, H, W, Cout] f16, kernel code)."""
    N, H, W, Cin, Cout, taps = c['N'], c['H'], c['W'], c['Cin'], c['Cout'], c['taps']
    pad = (Cout + 127) // 128 * 128
    x = _nhwc(op['x'])
    xa, xb = (x[..., :c['x2']].contiguous(), x[..., c['x2']:].contiguous()) if c['x2'] else (x, None)
    wp, bias = _pack(L, op['w'], pad), op['b']
    xs = xs2 = None
    if c['Cs']:                    # [Cout_pad][9 Cin + Cs]: the packed 3x3 rows followed by the packed 1x1 rows; the biases summed (exact: multiples of 2^-11)
        wp = torch.cat([wp, _pack(L, op['ws'], pad)], dim=1).contiguous()
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
    k, ch = C.c_int(-1), C.c_int(-1)
    ru = 1 if c['res_up'] else 0
    with cx.LabHooks(L, c):
        args = (_ptr(xa), _ptr(xb), c['x2'], _ptr(wp), _ptr(bd), _ptr(r), ru, _ptr(xs), _ptr(xs2), c['Cs1'], c['Cs'], _ptr(y), N, H, W, Cin, Cout, pad, taps,
                _ptr(zp), _ptr(ws), wsf)
        assert L.pdhip_debug_conv_launch_nhwc_f16(*args, _ptr(y), -1, C.byref(ch), C.byref(k), _stream()) == -1 and b'gn_part holds' in L.pdhip_last_error(), \
            L.pdhip_last_error()                                                 # planned only: ch = the chunks the launch will leave
        need = N * ch.value * (Cout // 8) * 2
        gp = torch.full((need + TAIL,), float('nan'), device=DEV)
        gp.view(torch.int32)[need:] = GUARD
        rc = L.pdhip_debug_conv_launch_nhwc_f16(*args, _ptr(gp), need, C.byref(ch), C.byref(k), _stream())
    assert rc == 0, L.pdhip_last_error()
    torch.cuda.synchronize()
    assert (gp.view(torch.int32)[need:] == GUARD).all(), "the launch wrote behind its partials"
    assert_tickets_zero(ws)
    return y, k.value


ALL_CASES = [cx.launch_case(c) for c in ce.CASES] + cx.EXTRA_CASES
TILE_ROWS = {'igemm': 128, 'sk': 64, 'halo': 512}


@pytest.mark.parametrize("c", ALL_CASES, ids=[c['name'] for c in ALL_CASES])
def test_conv_launch_is_bit_identical_to_float64(L, c):
    op, want = operands_and_reference(c['N'], c['H'], c['W'], c['Cin'], c['Cout'], c['taps'], c['res'], Cs=c['Cs'],
                                      res_hw=(c['H'] // 2, c['W'] // 2) if c['res_up'] else None)
    y, kernel = launch(L, c, op)
    assert kernel == ce.KERNELS[c['kernel']], f"routed to kernel {kernel}"
    rows = TILE_ROWS[c['kernel']] // c['W']                                      # image rows of the smallest pixel tile of the kernel (0: less than a row)
    strips = c['kernel'] == 'halo' and c['W'] == 256 and c['strips'] == 0        # (4 rows x 128 columns)
    assert_equal(y, want, tile=(4, 128) if strips else (max(rows, 1), None))


# ---- k_conv_rr, raw input
def _pack_rr(L, w3, w1):
    """w3 [Cout, Cin, k, k] f32 (+ w1 [Cout, Cs] of an appended skip 1x1) -> the engine's [Cout][taps * Cin + Cs] f16 layout -> fragment-major."""
    Cout, Cin, k, _ = w3.shape
    taps = k * k
    wp = w3.permute(0, 2, 3, 1).reshape(Cout, taps * Cin)
    Cs = 0
    if w1 is not None:
        Cs = w1.shape[1]
        wp = torch.cat([wp, w1], dim=1)
    wp = wp.half().contiguous().to(DEV)
    wf = torch.empty((L.pdhip_conv_rr_weight_halfs(Cin, taps, Cs, Cout),), dtype=torch.float16, device=DEV)
    assert L.pdhip_conv_rr_pack_f16(_ptr(wp), Cin, taps, Cs, Cout, _ptr(wf), _stream()) == 0, L.pdhip_last_error()
    return wf


@pytest.mark.parametrize("N,HW,Ca,Cb,Cout,skip,res,taps,variant,slabs", cx.RR_CASES)
def test_conv_rr_raw_input_is_bit_identical_to_float64(L, N, HW, Ca, Cb, Cout, skip, res, taps, variant, slabs):
    Cc, Cs = Ca + Cb, (skip[0] + skip[1]) if skip else 0
    op, want = operands_and_reference(N, HW, HW, Cc, Cout, taps, res != 0, Cs=Cs, res_hw=(HW // 2, HW // 2) if res == 2 else None)
    x = _nhwc(op['x'])
    xa, xb = (x[..., :Ca].contiguous(), x[..., Ca:].contiguous()) if Cb else (x, None)
    xsa = xsb = None
    bias = op['b']
    if skip:
        xs = _nhwc(op['xs'])
        xsa, xsb = (xs[..., :skip[0]].contiguous(), xs[..., skip[0]:].contiguous()) if skip[1] else (xs, None)
        bias = op['b'] + op['bs']
    wf = _pack_rr(L, op['w'], op['ws'][:, :, 0, 0] if skip else None)
    bd = bias.to(DEV)
    rd = _nhwc(op['r']) if res else None
    ws = torch.zeros((4096 + 4 * 1024 * 1024,), dtype=torch.float32, device=DEV)
    y = torch.full((N, HW, HW, Cout), float('nan'), dtype=torch.float16, device=DEV)
    part = torch.full((N * 64 * (Cout // 8) * 2,), float('nan'), dtype=torch.float32, device=DEV)
    chunks = C.c_int(-1)
    old = L.pdhip_debug_set_conv_rr(2, variant, slabs)
    try:
        rc = L.pdhip_conv_rr_f16(_ptr(xa), _ptr(xb), Cc, Ca, 0, None, None, None, 0, None, 0, None, 0, _ptr(xsa), _ptr(xsb), Cs, skip[0] if skip else 0, taps,
                                 _ptr(wf), _ptr(bd), _ptr(rd), 1 if res == 2 else 0, _ptr(y), N, HW, HW, Cout, _ptr(ws), ws.numel(), _ptr(part),
                                 C.byref(chunks), _stream())
    finally:
        L.pdhip_debug_set_conv_rr(old, 0, 0)
    assert rc == 0, L.pdhip_last_error()
    torch.cuda.synchronize()
    assert_tickets_zero(ws)
    assert 1 <= chunks.value <= 64
    assert_equal(y, want, tile=max(HW // chunks.value, 1))                       # (a band of HW / chunks rows per workgroup)


# ---- k_conv_ht
@pytest.mark.parametrize("N,HW,Cin,Cout,res,slabs", cx.HT_CASES)
def test_conv_ht_is_bit_identical_to_float64(L, N, HW, Cin, Cout, res, slabs):
    op, want = operands_and_reference(N, HW, HW, Cin, Cout, 9, res != 0, res_hw=(HW // 2, HW // 2) if res == 2 else None)
    pad = (Cout + 63) // 64 * 64
    wp = _pack(L, op['w'], pad)
    zp = torch.zeros((128,), dtype=torch.float16, device=DEV)
    xd, bd = _nhwc(op['x']), op['b'].to(DEV)
    rd = _nhwc(op['r']) if res else None
    ws = torch.zeros((cx.ht_workspace_floats(N, HW, pad),), dtype=torch.float32, device=DEV)
    ws[4096:] = float('nan')
    y = torch.full((N, HW, HW, Cout), float('nan'), dtype=torch.float16, device=DEV)
    part = torch.full((N * (HW * HW // 256) * (Cout // 8) * 2,), float('nan'), dtype=torch.float32, device=DEV)
    ch = C.c_int(-1)
    old = L.pdhip_debug_set_conv_ht(2, slabs)
    try:
        routed, taken = C.c_int(-1), C.c_int(-1)
        assert L.pdhip_conv_ht_plan(N, HW, HW, Cin, Cout, pad, ws.numel(), C.byref(routed), C.byref(taken)) == 0
        assert routed.value == 1 and taken.value == cx.ht_slabs_taken(Cin, slabs)
        rc = L.pdhip_conv_ht_f16(_ptr(xd), _ptr(wp), _ptr(bd), _ptr(rd), 1 if res == 2 else 0, _ptr(y), N, HW, HW, Cin, Cout, pad, _ptr(zp), _ptr(ws), ws.numel(),
                                 _ptr(part), C.byref(ch), _stream())
    finally:
        L.pdhip_debug_set_conv_ht(old, 0)
    assert rc == 0, L.pdhip_last_error()
    torch.cuda.synchronize()
    assert_tickets_zero(ws)
    if taken.value > 1:
        assert not torch.isnan(ws[4096:4096 + 16384]).any(), "the split form must have been taken"
    assert ch.value == HW * HW // 256
    assert_equal(y, want, tile=(256 // HW, None))                                # (256-pixel tiles of whole rows)


# ---- the up conv
@pytest.mark.parametrize("hs,cin,cout,N", cx.UP_CASES)
def test_up_conv_weight_table_phase_conv_and_halo_form_are_bit_identical_to_float64(L, hs, cin, cout, N):
    op, want = operands_and_reference(N, hs, hs, cin, cout, 9, False, up=True)
    pad = (cout + 127) // 128 * 128
    w9 = _pack(L, op['w'], pad)
    wph = torch.full((4, pad, 4 * cin), 7.0, dtype=torch.float16, device=DEV)
    assert L.pdhip_pack_conv_up2_phase_f16(_ptr(w9), cin, pad, _ptr(wph), _stream()) == 0, L.pdhip_last_error()
    torch.cuda.synchronize()
    table = wph.cpu().reshape(4, pad, 4, cin)
    assert torch.equal(table[:, :cout], cx.phase_weights_f64(op['w']).half()), "the phase weights are not the exact tap sums"
    assert int((table[:, cout:] != 0).sum()) == 0
    xd, bd = _nhwc(op['x']), op['b'].to(DEV)
    zp = torch.zeros((128,), dtype=torch.float16, device=DEV)
    H2 = 2 * hs
    y = torch.full((N, H2, H2, cout), float('nan'), dtype=torch.float16, device=DEV)
    chunks = 4 * hs * hs // 256
    part = torch.full((N * chunks * (cout // 8) * 2 + TAIL,), float('nan'), device=DEV) if (hs * hs) % 256 == 0 else None
    rc = L.pdhip_conv3x3_up2_phase_nhwc_f16(_ptr(xd), _ptr(wph), _ptr(bd), _ptr(y), N, hs, hs, cin, cout, pad, _ptr(zp), _ptr(part), _stream())
    assert rc == 0, L.pdhip_last_error()
    torch.cuda.synchronize()
    assert_equal(y, want, tile=2)
    if H2 in (32, 64, 128, 256) and (H2 * H2) % 512 == 0:                        # a width of the halo-resident kernel; tile hook 32: also below 256 tiles
        y9 = torch.full((N, H2, H2, cout), float('nan'), dtype=torch.float16, device=DEV)
        old = L.pdhip_debug_set_conv_tile(32)
        try:
            rc = L.pdhip_conv3x3_up2_halo_nhwc_f16(_ptr(xd), _ptr(w9), _ptr(bd), _ptr(y9), N, hs, hs, cin, cout, pad, _ptr(zp), _stream())
        finally:
            L.pdhip_debug_set_conv_tile(old)
        assert rc == 0, L.pdhip_last_error()
        torch.cuda.synchronize()
        assert_equal(y9, want, tile=(512 // H2, None))


# ---- the skip 1x1 of the one-pass GroupNorm + skip kernel
@pytest.mark.parametrize("Ca,Cb,H,W,N", cx.GN_SKIP_CASES)
def test_gn_skip_sk_output_is_bit_identical_to_float64(L, Ca, Cb, H, W, N):
    """sk = conv1x1(x) + bias over the RAW block input [xa | xb]: exact on these operands.  h0 = silu(GroupNorm(x)) of the same launch is not (its
    bit identity with the stand-alone GroupNorm-apply kernel is test_gn_skip_one_pass_equals_two_launches'); the statistics it needs come from float64."""
    Cc = Ca + Cb
    op, want = operands_and_reference(N, H, W, Cc, 256, 1, False)
    x = _nhwc(op['x'])
    xa, xb = (x[..., :Ca].contiguous(), x[..., Ca:].contiguous()) if Cb else (x, None)
    mean, rstd = ce.group_stats([x.reshape(N, H * W, Cc)])
    stats = torch.stack([mean, rstd], dim=-1).float().contiguous().to(DEV)
    g = torch.Generator().manual_seed(Cc + H)
    gamma, beta = (1 + 0.2 * torch.randn((Cc,), generator=g)).to(DEV), (0.2 * torch.randn((Cc,), generator=g)).to(DEV)
    wp, bd = _pack(L, op['w'], 256), op['b'].to(DEV)
    for variant in (1, 2):                               # (1: 64-pixel tiles where 128-pixel tiles would not fill the chip; 2: 128-pixel tiles always)
        h0 = torch.full((N, H, W, Cc), float('nan'), dtype=torch.float16, device=DEV)
        sk = torch.full((N, H, W, 256), float('nan'), dtype=torch.float16, device=DEV)
        old = L.pdhip_debug_set_gn_skip_variant(variant)
        try:
            rc = L.pdhip_gn_silu_skip1x1_nhwc_f16(_ptr(xa), _ptr(xb), Ca, Cc, _ptr(stats), _ptr(gamma), _ptr(beta), _ptr(wp), _ptr(bd), _ptr(h0), _ptr(sk),
                                                  N, H, W, _stream())
        finally:
            L.pdhip_debug_set_gn_skip_variant(old)
        assert rc == 0, L.pdhip_last_error()
        torch.cuda.synchronize()
        assert not torch.isnan(h0).any(), variant
        lines = cx.mismatches(sk, want, tile=(64 if variant == 1 else 128) // W or 1)
        assert lines == [], f"variant {variant}\n" + '\n'.join(lines)
