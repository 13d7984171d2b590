"""csrc/unproject.hip stage by stage, through the C entries: the Non-Border-First shrink on every path of its launcher, texel visibility and view
selection with the run-time-V kernels up to the view limit (and both kernels at V = 8), the multi-shape entries, texel compaction and the bit
transport.  References and cases: tests/unproject_stages_common.py (held to slow restatements in tests/test_unproject_stages_cpu.py).

Every comparison is an equality: these stages produce verdicts, indices and copied colours.  Every output and workspace starts as 0x55 bytes and
every output sits between two guard bands of 0x55 that must come back untouched.  Sizes are the ones at which the kernels change path: below
one 64-texel word, one word, word + 1, no multiple of 64, several 32-row bands; radius 63 | 64; the 64 KiB LDS limit of the bit kernel."""
import ctypes as C

import numpy as np
import pytest
import torch

import unproject_stages_common as uc

DEV = 'cuda:0'
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pd():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from pointdreamer_amd import _lib
    return dict(lib=_lib, L=_lib.lib())


def dev(a, off=0):
    """numpy -> device, bytes unchanged; off > 0: the array starts `off` bytes into its (16-byte aligned) allocation."""
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint64:
        a = a.view(np.int64)                                       # (torch moves the bytes; it has no use for the sign)
    if off == 0:
        t = torch.from_numpy(a).to(DEV)
        assert t.data_ptr() % 16 == 0
        return t, C.c_void_p(t.data_ptr())
    raw = torch.from_numpy(np.concatenate([np.full(off, uc.FILL, np.uint8), a.reshape(-1).view(np.uint8)])).to(DEV)
    assert raw.data_ptr() % 16 == 0
    return raw, C.c_void_p(raw.data_ptr() + off)


class Out:
    """nbytes of output (or workspace) between two guard bands, all 0x55; off > 0 misaligns the output by that many bytes."""

    def __init__(self, nbytes, off=0):
        self.n, self.start = int(nbytes), uc.GUARD + off
        self.t = torch.full((self.start + self.n + uc.GUARD,), uc.FILL, dtype=torch.uint8, device=DEV)
        assert self.t.data_ptr() % 16 == 0
        self.addr = self.t.data_ptr() + self.start
        self.ptr = C.c_void_p(self.addr)

    def get(self, dtype=np.uint8):
        h = self.t.cpu().numpy()
        assert (h[:self.start] == uc.FILL).all(), "written in front of the output"
        assert (h[self.start + self.n:] == uc.FILL).all(), "written behind the output"
        return h[self.start:self.start + self.n].copy().view(dtype)


def ok(pd, rc):
    assert rc == 0, (rc, pd['L'].pdhip_last_error())


def ks(k):
    return (C.c_int32 * len(k))(*k)


# ---------------------------------------------------------------------------------------------------------------------------- NBF
def run_nbf(pd, mask8, vis8, kernels, mode=0, S=1, vis_off=0, out_off=0, ws_off=0):
    """(out [K,VT,A,A] u8, path taken) of pdhip_nbf_shrink (S == 1) or pdhip_nbf_shrink_shapes under hook `mode`."""
    L, st = pd['L'], pd['lib'].stream
    VT, A = vis8.shape[0], vis8.shape[-1]
    K = len(kernels)
    Kout = 1 if kernels[0] == 0 else K
    m, mp = dev(mask8)
    v, vp = dev(vis8, vis_off)
    out, ws = Out(Kout * VT * A * A, out_off), Out(2 * VT * A * A, ws_off)
    old = L.pdhip_debug_set_nbf_path(mode)
    try:
        path = L.pdhip_nbf_path(VT, A, ks(kernels), K, uc.align_mask(mp.value, vp.value, out.addr, ws.addr))
        assert path >= 0, L.pdhip_last_error()
        if S == 1:
            ok(pd, L.pdhip_nbf_shrink(mp, vp, VT, A, ks(kernels), K, out.ptr, ws.ptr, st()))
        else:
            ok(pd, L.pdhip_nbf_shrink_shapes(mp, vp, VT // S, S, A, ks(kernels), K, out.ptr, ws.ptr, st()))
    finally:
        L.pdhip_debug_set_nbf_path(old)
    torch.cuda.synchronize()
    ws.get()                                                       # (guards of the workspace)
    return out.get().reshape(Kout, VT, A, A), path


def modes_for(path):
    """Hook modes to run for a case whose automatic path is `path`, with the path each must report."""
    if path == uc.BITS_PACK16:
        return [(0, uc.BITS_PACK16), (2, uc.BITS_BALLOT), (1, uc.BYTES)]
    if path == uc.BITS_BALLOT:
        return [(0, uc.BITS_BALLOT), (1, uc.BYTES)]
    return [(0, path)]


def check_nbf_every_path(pd, mask8, vis8, kernels, want, label, **kw):
    got, auto = run_nbf(pd, mask8, vis8, kernels, **kw)
    taken = []
    for mode, expect in modes_for(auto):
        if mode:
            got, path = run_nbf(pd, mask8, vis8, kernels, mode=mode, **kw)
        else:
            path = auto
        assert path == expect, (label, mode, uc.PATH_NAME[path])
        bad = np.argwhere(got != want)
        assert len(bad) == 0, f"{label} path {uc.PATH_NAME[path]}: {len(bad)} texels differ, first at [level, view, row, col] = {bad[0].tolist()}"
        taken.append(path)
    return taken


@pytest.mark.parametrize("A", uc.NBF_SIZES)
def test_nbf_shrink_equals_the_oracle_on_every_eligible_path(pd, A):
    seen = set()
    for name, V, kernels in uc.nbf_cases(A):
        mask8, vis8 = uc.nbf_image(name, A, V)
        want = uc.ref_nbf(mask8, vis8, kernels)
        seen.update(check_nbf_every_path(pd, mask8, vis8, kernels, want, f"A={A} image={name} V={V} kernels={kernels}"))
    assert seen == ({uc.BYTES, uc.COPY} if A % 64 else {uc.BYTES, uc.BITS_PACK16, uc.BITS_BALLOT, uc.COPY})


def test_nbf_shrink_on_both_sides_of_the_lds_limit(pd):
    """A = 2048, V = 2: k = 97 needs exactly 64 KiB of LDS and runs on bits, k = 99 takes the whole call to the byte kernels (whose grid-stride
    loop runs at this size only: 2048 workgroups of 256 for 4 194 304 texels)."""
    A, V = 2048, 2
    rng = np.random.default_rng(2048)
    mask = uc.blobs(A, rng, 256, 0.85)
    vis8 = np.stack([uc.blobs(A, rng, 128, 0.6) & mask for _ in range(V)]).astype(np.uint8)
    mask8 = mask.astype(np.uint8)
    want = uc.ref_nbf(mask8, vis8, [97, 99])
    assert 0 < want[1].sum() < want[0].sum() < (vis8 != 0).sum()
    assert check_nbf_every_path(pd, mask8, vis8, [97, 99], want, "A=2048 kernels=[97, 99]") == [uc.BYTES]
    assert check_nbf_every_path(pd, mask8, vis8, [97], want[:1], "A=2048 kernels=[97]") == [uc.BITS_PACK16, uc.BITS_BALLOT, uc.BYTES]
    assert check_nbf_every_path(pd, mask8, vis8, [99], want[1:], "A=2048 kernels=[99]") == [uc.BYTES]


@pytest.mark.parametrize("A", [64, 128])
def test_nbf_shrink_follows_the_alignment_of_its_pointers(pd, A):
    """Visibility one byte off: the ballot packer.  out or ws one byte off: the byte kernels (the bit kernel stores 16 bytes at a time to out and
    reads ws as 64-bit words) -- never a bit-path launch with such a pointer."""
    for name in ('blobs', 'blobs_bytes', 'vertical_edge'):
        mask8, vis8 = uc.nbf_image(name, A, 3)
        kernels = [21, 11, 7]
        want = uc.ref_nbf(mask8, vis8, kernels)
        assert check_nbf_every_path(pd, mask8, vis8, kernels, want, f"A={A} {name} visibility+1", vis_off=1) == [uc.BITS_BALLOT, uc.BYTES]
        assert check_nbf_every_path(pd, mask8, vis8, kernels, want, f"A={A} {name} out+1", out_off=1) == [uc.BYTES]
        assert check_nbf_every_path(pd, mask8, vis8, kernels, want, f"A={A} {name} ws+1", ws_off=1) == [uc.BYTES]
        assert check_nbf_every_path(pd, mask8, vis8, kernels, want, f"A={A} {name} out+1 ws+1", out_off=1, ws_off=1) == [uc.BYTES]
        assert check_nbf_every_path(pd, mask8, vis8, kernels, want, f"A={A} {name} out+8 ws+4", out_off=8, ws_off=4) == [uc.BYTES]


@pytest.mark.parametrize("A", [64, 100])
def test_nbf_shrink_shapes_equals_single_calls_and_the_oracle(pd, A):
    """S = 3 shapes with V = 2 views each and three different chart masks: out is level-major over ALL views, [K][S*V][A][A], and view g uses
    the mask of shape g / V."""
    S, V, kernels = 3, 2, [7, 3, 7]
    pairs = [uc.nbf_image(name, A, V) for name in ('blobs', 'mask_edge', 'blobs_bytes')]
    masks, vis = np.stack([p[0] for p in pairs]), np.concatenate([p[1] for p in pairs])
    assert len({m.tobytes() for m in masks}) == 3
    want = np.zeros((3, S * V, A, A), np.uint8)
    for s in range(S):
        want[:, s * V:(s + 1) * V] = uc.ref_nbf(masks[s], vis[s * V:(s + 1) * V], kernels)
        # the mask matters: another shape's mask gives another result
        assert not np.array_equal(want[:, s * V:(s + 1) * V], uc.ref_nbf(masks[(s + 1) % S], vis[s * V:(s + 1) * V], kernels))
    taken = check_nbf_every_path(pd, masks, vis, kernels, want, f"shapes A={A}", S=S)
    assert taken == ([uc.BITS_PACK16, uc.BITS_BALLOT, uc.BYTES] if A == 64 else [uc.BYTES])
    for s in range(S):
        single, _ = run_nbf(pd, masks[s], vis[s * V:(s + 1) * V], kernels)
        assert np.array_equal(single, want[:, s * V:(s + 1) * V]), s
    for mode, _ in modes_for(taken[0]):                            # the layout, spelled out on the raw bytes
        flat = run_nbf(pd, masks, vis, kernels, mode=mode, S=S)[0].reshape(-1)
        for k in range(3):
            for s in range(S):
                for v in range(V):
                    at = ((k * S * V) + s * V + v) * A * A
                    assert np.array_equal(flat[at:at + A * A].reshape(A, A), want[k, s * V + v]), (mode, k, s, v)


# ---------------------------------------------------------------------------------------------------------------------------- visibility
def run_visibility(pd, c, generic):
    L, st = pd['L'], pd['lib'].stream
    S, V, A, R = c['S'], c['V'], c['A'], c['R']
    keep = [dev(c[k]) for k in ('cams', 'gb_pos', 'mask', 'uv_centers', 'uv_scales', 'mesh')]
    cams, gb, mask, uvc, uvs, mesh = (p for _, p in keep)
    out = Out(S * V * A * A)
    old = L.pdhip_debug_set_unproject_generic(1 if generic else 0)
    try:
        if S == 1:
            ok(pd, L.pdhip_texel_visibility(cams, V, gb, mask, A, uvc, uvs, c['padding'], mesh, R, float(c['offset']), out.ptr, st()))
        else:
            ok(pd, L.pdhip_texel_visibility_shapes(cams, V, S, gb, mask, A, uvc, uvs, c['padding'], mesh, R, float(c['offset']), out.ptr, st()))
    finally:
        L.pdhip_debug_set_unproject_generic(old)
    torch.cuda.synchronize()
    return out.get().reshape(S * V, A, A)


def check_visibility(pd, c, label):
    want = uc.ref_visibility(c)
    f64, counted, _, _ = uc.ref_visibility_f64(c)
    for generic in ((False, True) if c['V'] == 8 else (False,)):
        got = run_visibility(pd, c, generic)
        bad = np.argwhere(got != want)
        assert len(bad) == 0, f"{label} generic={generic}: {len(bad)} verdicts differ from the float32 contract, first at [view, row, col] = {bad[0].tolist()}"
        assert np.array_equal(got[counted], f64[counted]), f"{label} generic={generic}: differs from the float64 verdict outside the rounding band"


@pytest.mark.parametrize("V", uc.VIEWS)
def test_texel_visibility_equals_the_contract_and_the_f64_verdict(pd, V):
    for A, R, S in uc.vis_cases(V):
        check_visibility(pd, uc.vis_case(A, R, V, S), f"A={A} R={R} V={V} S={S}")


def test_texel_visibility_grid_stride(pd):
    """A = 1088: 1 183 744 texels for the 4096 x 256 threads of a one-shape launch, so 135 168 texels take a second trip of the loop."""
    check_visibility(pd, uc.vis_case(1088, 128, 8, 1), "A=1088 R=128 V=8 S=1")


# ---------------------------------------------------------------------------------------------------------------------------- view selection
def run_select(pd, c, complete, generic):
    L, st = pd['L'], pd['lib'].stream
    S, V, A, K, r, F = c['S'], c['V'], c['A'], c['K'], c['r'], c['F']
    keep = [dev(c[k]) for k in ('cams', 'gb_pos', 'mask', 'face_id', 'f_normals', 'dirs', 'uv_centers', 'uv_scales', 'scale_factors', 'shrinked',
                                'vis', 'inpainted')]
    cams, gb, mask, fid, fn, bd, uvc, uvs, sf, shr, vis, img = (p for _, p in keep)
    atlas, painted, vid = Out(S * A * A * 3 * 4), Out(S * A * A), Out(S * A * A * 4)
    old = L.pdhip_debug_set_unproject_generic(1 if generic else 0)
    try:
        if S == 1:
            ok(pd, L.pdhip_view_select_blend(cams, V, gb, mask, fid, A, fn, bd, uvc, uvs, c['padding'], sf, shr, K, vis, complete, img, r,
                                             atlas.ptr, painted.ptr, vid.ptr, st()))
        else:
            ok(pd, L.pdhip_view_select_blend_shapes(cams, V, S, gb, mask, fid, A, fn, F, bd, uvc, uvs, c['padding'], sf, shr, K, vis, complete,
                                                    img, r, atlas.ptr, painted.ptr, vid.ptr, st()))
    finally:
        L.pdhip_debug_set_unproject_generic(old)
    torch.cuda.synchronize()
    return atlas.get(np.float32).reshape(S, A, A, 3), painted.get().reshape(S, A, A), vid.get(np.int32).reshape(S, A, A)


@pytest.mark.parametrize("V", uc.VIEWS)
def test_view_select_blend_equals_the_reference(pd, V):
    for A, K, complete, r, S in uc.sel_cases(V):
        c = uc.sel_case(A, V, K, r, S)
        label = f"A={A} V={V} K={K} complete={complete} r={r} S={S}"
        atlas, painted, vid, _ = uc.ref_view_select(c, complete)
        f64, decided = uc.f64_selection(c, complete)
        inside = c['mask'] != 0
        for generic in ((False, True) if V == 8 else (False,)):
            g_atlas, g_painted, g_vid = run_select(pd, c, complete, generic)
            bad = np.argwhere(g_vid != vid)
            assert len(bad) == 0, (f"{label} generic={generic}: {len(bad)} view ids differ, first at [shape, row, col] = {bad[0].tolist()}: "
                                   f"{g_vid[tuple(bad[0])]} for {vid[tuple(bad[0])]}")
            assert np.array_equal(g_painted, painted), f"{label} generic={generic}: painted"
            bad = np.argwhere((g_atlas != atlas).any(-1))
            assert len(bad) == 0, f"{label} generic={generic}: {len(bad)} colours differ, first at [shape, row, col] = {bad[0].tolist()}"
            assert (g_vid[~inside] == -1).all() and g_vid.max() <= V - 1          # ids are local to a shape
            if not complete:
                assert ((g_vid == -100) == (inside & (painted == 0))).all()
            if V == 32 and A > 1:
                assert (g_vid == 31).any(), f"{label}: the last view never wins"
            assert np.array_equal(g_vid[decided], f64[decided]), f"{label} generic={generic}: float64 argmax of the similarity"


# ---------------------------------------------------------------------------------------------------------------------------- compaction, bits
@pytest.mark.parametrize("A", uc.COMPACT_SIZES)
def test_compact_texels_in_argwhere_order(pd, A):
    L, st = pd['L'], pd['lib'].stream
    n = A * A
    for name in uc.COMPACT_MASKS:
        mask8, gb, view_ids = uc.compact_case(A, name)
        pts, coords, pv, offs = uc.ref_compact(mask8, gb, view_ids)
        P = len(pts)
        keep = [dev(mask8), dev(gb), dev(view_ids)]
        mp, gp, vp = (p for _, p in keep)
        for skip in (None, 'points', 'coords', 'pvid', 'all'):
            o_pts, o_co, o_pv, cnt, ws = Out(n * 12), Out(n * 16), Out(n * 8), Out(4), Out((A + 1) * 4)
            null = C.c_void_p(0)
            a_pts = null if skip in ('points', 'all') else o_pts.ptr
            a_co = null if skip in ('coords', 'all') else o_co.ptr
            a_pv = null if skip in ('pvid', 'all') else o_pv.ptr
            # (without points gb_pos may be null, without point_view_ids so may view_ids)
            ok(pd, L.pdhip_compact_texels(null if a_pts is null else gp, mp, A, null if a_pv is null else vp, a_pts, a_co, a_pv, cnt.ptr, ws.ptr, st()))
            torch.cuda.synchronize()
            label = (A, name, skip)
            assert cnt.get(np.int32)[0] == P, label
            assert np.array_equal(ws.get(np.int32), offs), label
            for o, dtype, width, want, off in ((o_pts, np.float32, 3, pts, a_pts is null), (o_co, np.int64, 2, coords, a_co is null),
                                               (o_pv, np.int64, 1, pv, a_pv is null)):
                h = o.get(dtype).reshape(n, width)
                if off:
                    assert (h.view(np.uint8) == uc.FILL).all(), label
                else:
                    assert np.array_equal(h[:P].view(np.uint8), np.ascontiguousarray(want).reshape(P, width).view(np.uint8)), label
                    assert (h[P:].view(np.uint8) == uc.FILL).all(), label


@pytest.mark.parametrize("n", uc.PACK_SIZES)
def test_pack_and_unpack_bits(pd, n):
    L, st = pd['L'], pd['lib'].stream
    b = uc.pack_case(n)
    assert set(np.unique(b)) == set(uc.PACK_BYTES.tolist()) or n == 64
    want = uc.ref_pack(b)
    keep = dev(b)
    words = Out(n // 8)
    ok(pd, L.pdhip_pack_bits(keep[1], n, words.ptr, st()))
    torch.cuda.synchronize()
    got = words.get(np.uint64)
    assert np.array_equal(got, want)
    back = Out(n)
    keep2 = dev(want)
    ok(pd, L.pdhip_unpack_bits(keep2[1], n, back.ptr, st()))
    torch.cuda.synchronize()
    assert np.array_equal(back.get(), (b != 0).astype(np.uint8))
