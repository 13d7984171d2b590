"""CPU: the comparison tests/test_gpu_conv_epilogue.py applies to a conv epilogue's GroupNorm octet partials (tests/conv_epilogue_common.py) has teeth --
an honest f32 summation in any order passes it, each of the ways an epilogue goes wrong fails it -- and every case of the GPU test is planned onto
the kernel it is named for (conv_plan is host code: pdhip_debug_conv_launch_nhwc_f16 with a negative gn_part_floats plans and launches nothing)."""
import ctypes as C
import numpy as np
import pytest
import torch

import conv_epilogue_common as ce

N_IMG, COUT = 3, 136
ROWS = [16, 64, 128, 256, 512]          # rows per chunk of the producers: k_splitk_reduce, k_conv_sk (64, 128), k_conv_igemm (128, 256), the halo kernel


def synth(rows, chunks=2, seed=0):
    """A conv output with the GPU test's statistics: pre = f32 accumulator + bias (order 1, per channel), h = f16(pre), y = f16(h + residual) with a
    residual whose scale and offset differ per image.  Returns (pre f32, h f16, y f16), each [N, chunks * rows, 1, Cout] (H = chunks * rows, W = 1)."""
    op = ce.make_operands(N_IMG, chunks * rows, 1, 32, COUT, 1, True, seed)
    g = torch.Generator().manual_seed(seed + 1)
    pre = (torch.randn((N_IMG, chunks * rows, 1, COUT), generator=g) + op['b']).float()
    h = pre.half()
    y = (h.float() + op['r'].permute(0, 2, 3, 1)).half()
    return pre, h, y


def f32_partials(v, chunks, order):
    """(sum, sum of squares) per (image, chunk, octet) of v [N, HW, 1, C] in float32 arithmetic, three honest summation orders."""
    a = v.float().numpy().reshape(v.shape[0], chunks, -1, v.shape[-1] // 8, 8).astype(np.float32)
    rows = a.shape[2]
    out = []
    for t in (a, a * a):
        if order == 'rows-then-octet':           # pixel after pixel, the 8 channels of a pixel first (k_gn_octet_partials)
            acc = np.zeros(t.shape[:2] + (t.shape[3],), np.float32)
            for r in range(rows):
                s8 = np.zeros_like(acc)
                for e in range(8):
                    s8 = s8 + t[:, :, r, :, e]
                acc = acc + s8
        elif order == 'strided-threads':         # 16 threads take every 16th row, eight of them are added, then the two halves (the conv epilogues)
            th = np.zeros((16,) + t.shape[:2] + (t.shape[3],), np.float32)
            for r in range(rows):
                for e in range(8):
                    th[r % 16] = th[r % 16] + t[:, :, r, :, e]
            lo, hi = np.zeros_like(th[0]), np.zeros_like(th[0])
            for j in range(8):
                lo, hi = lo + th[j], hi + th[8 + j]
            acc = lo + hi
        else:                                    # numpy's pairwise tree over the whole slot
            acc = np.ascontiguousarray(t.transpose(0, 1, 3, 2, 4)).reshape(t.shape[:2] + (t.shape[3], -1)).sum(axis=-1, dtype=np.float32)
        out.append(acc)
    return torch.from_numpy(np.stack(out, axis=-1))


@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("order", ['rows-then-octet', 'strided-threads', 'pairwise'])
def test_honest_f32_summation_passes_in_any_order(rows, order):
    _, _, y = synth(rows)
    part = f32_partials(y, 2, order)
    assert ce.partials_errors(part, y, 2) == []
    assert ce.partials_errors(part, y, 2, contiguous=False) == []


@pytest.mark.parametrize("rows", ROWS)
def test_each_epilogue_mistake_fails_the_comparison(rows):
    pre, h, y = synth(rows)
    good = f32_partials(y, 2, 'strided-threads')
    assert ce.partials_errors(good, y, 2) == []
    # one row of one chunk left out (a ragged last tile that drops its rows)
    holed = y.clone()
    holed[1, rows + rows // 2] = 0
    bad = f32_partials(holed, 2, 'strided-threads')
    assert ce.partials_errors(bad, y, 2) and ce.partials_errors(bad, y, 2, contiguous=False)
    # the chunks of image n written at image n - 1 (a chunk / image index off by one at an image boundary)
    bad = torch.roll(good, -1, dims=0)
    assert ce.partials_errors(bad, y, 2) and ce.partials_errors(bad, y, 2, contiguous=False)
    # one octet shifted by one (an n-tile offset; the octet beyond Cout lands on the next chunk's first slot)
    bad = torch.roll(good.reshape(N_IMG, -1, 2), 1, dims=1).reshape(good.shape)
    assert ce.partials_errors(bad, y, 2) and ce.partials_errors(bad, y, 2, contiguous=False)
    # sums taken before the residual add
    bad = f32_partials(h, 2, 'strided-threads')
    assert ce.partials_errors(bad, y, 2) and ce.partials_errors(bad, y, 2, contiguous=False)
    # two chunks of an image swapped: the image totals still agree (the consumers see no difference), the per-chunk comparison tells
    bad = torch.flip(good, dims=(1,))
    assert ce.partials_errors(bad, y, 2) and ce.partials_errors(bad, y, 2, contiguous=False) == []
    # a slot never written
    bad = good.clone()
    bad[2, 1, 16, 1] = float('nan')
    assert ce.partials_errors(bad, y, 2)


@pytest.mark.parametrize("rows", [16, 64])
def test_sums_of_the_unrounded_accumulator_fail_the_comparison(rows):
    """Sums of the f32 values before their rounding to f16 differ from the sums over the stored f16 values by a random walk of the rounding errors, which
    grows like sqrt(n), n = 8 rows, while the worst-case bound n 2^-24 sum|v| grows like n^2: the ratio falls like n^-1.5.  On this data the largest ratio
    over the slots is 7 (sums) / 19-24 (sums of squares) at the 16-row chunks of k_splitk_reduce and 1 / 2.4-3.5 at the 64-row tiles of k_conv_sk -- told;
    0.4 / 0.9-1.1 at 128 rows, 0.1 / 0.4 at 256, 0.05 / 0.14 at 512 -- not told by a worst-case bound.  There the mistake is left to the chunked producers'
    siblings: every kernel with 128-row and larger tiles shares its epilogue code with a 16- or 64-row form checked here (k_splitk_reduce behind the
    implicit GEMM and the halo kernel, the 64-row tiles of k_conv_sk)."""
    op = ce.make_operands(N_IMG, 2 * rows, 1, 32, COUT, 1, True, 5)
    g = torch.Generator().manual_seed(6)
    pre = (torch.randn((N_IMG, 2 * rows, 1, COUT), generator=g) + op['b']).float() + op['r'].permute(0, 2, 3, 1)      # the f32 value the epilogue rounds last
    y = pre.half()
    assert ce.partials_errors(f32_partials(y, 2, 'strided-threads'), y, 2) == []
    assert ce.partials_errors(f32_partials(pre, 2, 'strided-threads'), y, 2)


# ---- the statistics bound
def _stats_from_partials(parts, C_list, HW):
    """(mean, rstd) [N, 32, 2] f32 the way k_gn_finalize_oct combines octet partials (f64 combine of f32 slots)."""
    octs = torch.cat([p.double().sum(dim=1) for p in parts], dim=1)         # [N, octets of the concat, 2]
    Cc = sum(C_list)
    g = octs.reshape(octs.shape[0], 32, Cc // 32 // 8, 2).sum(dim=2)
    cnt = HW * (Cc // 32)
    mean = g[..., 0] / cnt
    var = (g[..., 1] / cnt - mean * mean).clamp(min=0)
    return torch.stack([mean, (var + 1e-5) ** -0.5], dim=-1).float()


@pytest.mark.parametrize("Ca,Cb,cha,chb", [(256, 0, 4, 0), (1024, 512, 1, 4), (512, 256, 16, 4)])
def test_statistics_bound_passes_honest_partials_and_fails_a_dropped_chunk(Ca, Cb, cha, chb):
    N, HW = 3, 64
    g = torch.Generator().manual_seed(Ca + Cb)
    ts, chunks = [], []
    for Cx, ch in ((Ca, cha), (Cb, chb)):
        if Cx:
            off = torch.randn((N, 1, Cx), generator=g) * 2
            ts.append((torch.randn((N, HW, Cx), generator=g) * (0.5 + torch.rand((N, 1, Cx), generator=g)) + off).half())
            chunks.append(ch)
    parts = [f32_partials(t.reshape(N, HW, 1, -1), ch, 'rows-then-octet') for t, ch in zip(ts, chunks)]
    assert ce.stats_errors(_stats_from_partials(parts, [t.shape[-1] for t in ts], HW), ts, chunks) == []
    # one chunk of one image dropped from the LAST source (the one whose chunk count differs)
    bad = [p.clone() for p in parts]
    bad[-1][1, chunks[-1] - 1] = 0
    assert ce.stats_errors(_stats_from_partials(bad, [t.shape[-1] for t in ts], HW), ts, chunks)
    # source B read with source A's chunk stride is the same kind of mistake: chunks of B's image n + 1 taken for image n
    if len(parts) == 2:
        bad = [parts[0], torch.roll(parts[1], -1, dims=0)]
        assert ce.stats_errors(_stats_from_partials(bad, [t.shape[-1] for t in ts], HW), ts, chunks)


# ---- routing of the GPU test's cases, on the host
@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as ge
    ge.build()
    from pointdreamer_amd import _lib
    import pointdreamer_amd.ddnm_inpainting  # noqa: F401  (registers the entry points)
    return _lib.lib()


def plan_only(L, c, x2=False, res_up=False, ws_floats=None):
    """(rc, kernel, chunks) of a case planned without a launch: the pointers are never read."""
    fake = C.c_void_p(4096)
    k, ch = C.c_int(-1), C.c_int(-1)
    pad = (c['Cout'] + 127) // 128 * 128
    wsf = ce.workspace_floats(c) if ws_floats is None else ws_floats
    with ce.Hooks(L, c):
        rc = L.pdhip_debug_conv_launch_nhwc_f16(fake, fake if x2 else None, c.get('Cin1', 0), fake, fake, fake if (c['res'] or res_up) else None, 1 if res_up else 0,
                                                fake if c['Cs'] else None, fake if c['Cs1'] else None, c['Cs1'], c['Cs'], fake, c['N'], c['H'], c['W'], c['Cin'],
                                                c['Cout'], pad, c['taps'], fake, fake if wsf else None, wsf, fake, -1, C.byref(ch), C.byref(k), None)
    return rc, k.value, ch.value


@pytest.mark.parametrize("c", ce.CASES, ids=[c['name'] for c in ce.CASES])
def test_every_gpu_case_is_planned_onto_the_kernel_it_names(L, c):
    rc, kernel, chunks = plan_only(L, c)
    assert rc == -1 and b'gn_part holds' in L.pdhip_last_error(), L.pdhip_last_error()      # refused for the partial buffer alone: nothing else was wrong
    assert kernel == ce.KERNELS[c['kernel']] and chunks == c['chunks'], (kernel, chunks)


def test_debug_conv_launch_refuses_what_the_planned_kernel_would_drop(L):
    """res_up on a kernel that reads its residual at full resolution only, a skip source or a second tensor the plan does not take, a residual next to a
    skip source, a partial buffer that is too small: PDHIP_E_ARG, no launch (none is possible here: there is no device)."""
    assert L.pdhip_version() == 211
    by = {c['name']: c for c in ce.CASES}
    rc, kernel, _ = plan_only(L, by['igemm-geo2-3x16x16-res'], res_up=True)
    assert rc == -1 and kernel == ce.KERNELS['igemm'] and b'half resolution' in L.pdhip_last_error()
    rc, kernel, _ = plan_only(L, by['halo-2x16x32'], res_up=True)                   # the halo kernel takes it only where it runs unsplit by itself
    assert rc == -1 and kernel == ce.KERNELS['halo'] and b'half resolution' in L.pdhip_last_error()
    skip = dict(by['skip-tile2-2x8x8'], tile=2, sk=(0, 0, 0))                      # k_conv_sk switched off: the implicit GEMM has no skip K loop
    rc, kernel, _ = plan_only(L, skip)
    assert rc == -1 and kernel == ce.KERNELS['igemm'] and b'skip 1x1' in L.pdhip_last_error()
    rc, _, _ = plan_only(L, dict(by['skip-tile2-2x8x8'], res=True))
    assert rc == -1 and b"residual's place" in L.pdhip_last_error()
    rc, _, _ = plan_only(L, dict(by['sk-tile1-split1-3x8x8'], Cin1=64), x2=True)    # a two-source 3x3 does not exist
    assert rc == -1 and b'two-source' in L.pdhip_last_error()
    assert L.pdhip_gn_finalize_oct_f32(None, 256, 1, None, 0, 0, 1, 64, None, None) == -1
    assert L.pdhip_gn_finalize_oct_f32(C.c_void_p(4096), 256, 1, None, 256, 1, 1, 64, C.c_void_p(4096), None) == -1      # Cb without partB
