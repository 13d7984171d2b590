"""Shared by tests/test_gpu_conv_tail_parent.py, tests/test_gpu_conv_epilogue.py and tools/record_conv_tail_digests.py: every case of
tests/conv_epilogue_common.py (CASES + TAIL_CASES) launched through the entry point that reaches its kernel, each output reduced to a SHA-256.

The conv kernels share one split-K hand-off, one workspace layout and one partial-slot address (csrc/nn_conv_tail.h).  tests/golden/conv_tail_parent.json
holds the digests of y and of the octet partials recorded with the library of the commit before they were shared; a refactor of those tails returns the same bytes.  The
results are deterministic by construction -- every combine sums its slices in slice order whoever arrives last, every reduce has a fixed order -- so a
digest that differs is a changed summation order or address.  Every case runs twice on ONE workspace: the second launch only ends if the first put its
tickets back to zero, and must give the same bytes."""
import ctypes as C
import hashlib
import os

import torch
import torch.nn.functional as F

import conv_epilogue_common as ce

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'conv_tail_parent.json')
DEV = 'cuda:0'
GUARD = 0x7F8ABCDE            # bit pattern of the floats behind the partials (a NaN payload no kernel produces)
TAIL = 4096                   # floats kept behind the partials: all of them carry the guard pattern and are checked
CASES = ce.CASES + ce.TAIL_CASES


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous().half().to(DEV)


def _pack(L, w):
    Cout, Cin, k = w.shape[0], w.shape[1], w.shape[2]
    wp = torch.zeros(((Cout + 127) // 128 * 128, k * k * Cin), dtype=torch.float16, device=DEV)
    wd = w.contiguous().float().to(DEV)
    assert L.pdhip_pack_conv_weight_f16(_ptr(wd), Cout, Cin, k * k, _ptr(wp), _stream()) == 0
    torch.cuda.synchronize()
    return wp


def operands(c):
    """The operands of a case (conv_epilogue_common.make_operands; the phase conv's input is the half-resolution tensor), seeded by its place in CASES."""
    up = c['entry'] == 'phase'
    return ce.make_operands(c['N'], c['H'] // 2 if up else c['H'], c['W'] // 2 if up else c['W'], c['Cin'], c['Cout'], c['taps'], c['res'],
                            1000 + CASES.index(c), Cs=c['Cs'])


def reference_f64(c, op):
    if c['entry'] == 'phase':
        op = dict(op, x=F.interpolate(op['x'], scale_factor=2, mode='nearest'))
    return ce.reference_f64(op)


def prepare(L, c, op):
    """Uploads the operands of case c once and returns run(): one launch under the case's hooks on the case's ONE workspace (zeroed here, never again)
    -> (y [N, H, W, Cout] f16, partials [N * chunks * Cout / 8 * 2] f32 or None, chunks per image, ConvKernel code)."""
    N, H, W, Cin, Cout, taps = c['N'], c['H'], c['W'], c['Cin'], c['Cout'], c['taps']
    pad = (Cout + 127) // 128 * 128
    x, bias = _nhwc(op['x']), op['b']
    r = _nhwc(op['r']) if 'r' in op else None
    zp = torch.zeros((128,), dtype=torch.float16, device=DEV)
    wsf = ce.workspace_floats(c)
    ws = torch.zeros((wsf,), device=DEV) if wsf else None
    need = N * c['chunks'] * (Cout // 8) * 2
    xs = xs2 = None
    if c['entry'] == 'rr':                                   # [Cout][9 Cin] f16 -> fragment-major
        wp = op['w'].permute(0, 2, 3, 1).reshape(Cout, taps * Cin).half().contiguous().to(DEV)
        w = torch.empty((L.pdhip_conv_rr_weight_halfs(Cin, taps, 0, Cout),), dtype=torch.float16, device=DEV)
        assert L.pdhip_conv_rr_pack_f16(_ptr(wp), Cin, taps, 0, Cout, _ptr(w), _stream()) == 0, L.pdhip_last_error()
    elif c['entry'] == 'phase':
        w = torch.empty((4, pad, 4 * Cin), dtype=torch.float16, device=DEV)
        assert L.pdhip_pack_conv_up2_phase_f16(_ptr(_pack(L, op['w'])), Cin, pad, _ptr(w), _stream()) == 0, L.pdhip_last_error()
    else:
        w = _pack(L, op['w'])
        if c['Cs']:                # [Cout_pad][9 Cin + Cs]: the packed 3x3 rows followed by the packed 1x1 rows; the biases summed
            w = torch.cat([w, _pack(L, op['ws'])], dim=1).contiguous()
            bias = op['b'] + op['bs']
            xs = _nhwc(op['xs'])
            if c['Cs1']:
                xs, xs2 = xs[..., :c['Cs1']].contiguous(), xs[..., c['Cs1']:].contiguous()
    bd = bias.float().to(DEV)
    torch.cuda.synchronize()

    def run():
        y = torch.full((N, H, W, Cout), float('nan'), dtype=torch.float16, device=DEV)
        gp = torch.full((need + TAIL,), float('nan'), device=DEV)
        gp.view(torch.int32)[need:] = GUARD
        k, ch = C.c_int(-1), C.c_int(-1)
        with ce.Hooks(L, c):
            if c['entry'] == 'rr':
                rc = L.pdhip_conv_rr_f16(_ptr(x), None, Cin, Cin, 0, None, None, None, 0, None, 0, None, 0, None, None, 0, 0, taps, _ptr(w), _ptr(bd), _ptr(r), 0,
                                         _ptr(y), N, H, W, Cout, _ptr(ws), wsf, _ptr(gp), C.byref(ch), _stream())
                k.value = ce.KERNELS['rr']
            elif c['entry'] == 'phase':
                rc = L.pdhip_conv3x3_up2_phase_nhwc_f16(_ptr(x), _ptr(w), _ptr(bd), _ptr(y), N, H // 2, W // 2, Cin, Cout, pad, _ptr(zp), _ptr(gp), _stream())
                k.value, ch.value = ce.KERNELS['phase'], H * W // 256
            else:
                rc = L.pdhip_debug_conv_launch_nhwc_f16(_ptr(x), None, 0, _ptr(w), _ptr(bd), _ptr(r), 0, _ptr(xs), _ptr(xs2), c['Cs1'], c['Cs'], _ptr(y), N, H, W,
                                                        Cin, Cout, pad, taps, _ptr(zp), _ptr(ws), wsf, _ptr(gp), need, C.byref(ch), C.byref(k), _stream())
        assert rc == 0, L.pdhip_last_error()
        torch.cuda.synchronize()
        assert (gp.view(torch.int32)[need:] == GUARD).all(), "the launch wrote behind its partials"
        if ws is not None:
            assert int((ws[:4096].view(torch.int32) != 0).sum()) == 0, "the ticket words are not back at zero"
        return y, (gp[:need] if need else None), ch.value, k.value
    return run


def digest(t):
    """SHA-256 of a tensor's dtype, shape and bytes ('' for None)."""
    if t is None:
        return ''
    a = t.detach().cpu().contiguous()
    h = hashlib.sha256(f"{a.dtype}{tuple(a.shape)}".encode())
    h.update(a.view(torch.uint8).numpy().tobytes())
    return h.hexdigest()


def run_case(L, c):
    """Two launches of case c on one workspace -> [{kernel, chunks, y, partials}, the same of the second launch]."""
    run = prepare(L, c, operands(c))
    out = []
    for _ in range(2):
        y, part, chunks, kernel = run()
        out.append(dict(kernel=kernel, chunks=chunks, y=digest(y), partials=digest(part)))
    return out
