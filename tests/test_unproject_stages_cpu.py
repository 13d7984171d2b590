"""The references of tests/unproject_stages_common.py against slow restatements, the NBF routing table of pdhip_nbf_path, the refusals of the
unprojection entries (each returns before any device call) and the properties the GPU cases rely on: every class of texel present in the
selection cases, and the float64 visibility check leaving out at most 2 % of a case.  Nothing here needs a device."""
import ctypes as C

import numpy as np
import pytest

import unproject_stages_common as uc

E_ARG = -1
PTR = 0x1000                                                       # a non-null, 16-byte aligned address that is never dereferenced


@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as ge
    ge.build()
    from pointdreamer_amd import _lib
    return _lib.lib()


def ks(*k):
    return (C.c_int32 * len(k))(*k)


# ---------------------------------------------------------------------------------------------------------------------------- references
@pytest.mark.parametrize("A", [5, 65])
def test_nbf_oracle_equals_the_float_scharr_and_reflect_padded_maximum(A):
    """oracle.nbf.shrink_visibility (integer gx != 0 or gy != 0, clamped-window OR) against the reference's own formulation texel by texel:
    float Scharr response on the 0 / 255 image, reflect-padded k x k maximum, k in {1, 3, 7, 2A + 1}."""
    kernels = [1, 3, 7, 2 * A + 1] + ([21, 129] if A == 5 else [])  # (far wider than the image: numpy reflects as often as it takes)
    for name in ('blobs', 'mask_edge', 'checker', 'one_bottom_right', 'all'):
        mask, vis = uc.nbf_image(name, A, 2)
        assert np.array_equal(uc.ref_nbf(mask, vis, kernels), uc.slow_nbf(mask, vis, kernels)), name


def test_nbf_images_are_what_their_names_say():
    for A in uc.NBF_SIZES:
        for name in uc.NBF_IMAGES:
            mask, vis = uc.nbf_image(name, A, 3)
            assert mask.shape == (A, A) and vis.shape == (3, A, A) and mask.dtype == vis.dtype == np.uint8
            if name.startswith('one_'):
                assert (vis != 0).reshape(3, -1).sum(1).tolist() == [1, 1, 1]
    m, v = uc.nbf_image('vertical_edge', 128, 2)
    assert v[0, :, 63].all() and not v[0, :, 64].any() and v[1, 63].all() and not v[1, 64].any()
    m, v = uc.nbf_image('horizontal_edge', 128, 1)
    assert v[0, 31].all() and not v[0, 32].any()
    m, v = uc.nbf_image('one_32_64', 128, 1)
    assert v[0, 32, 64] == 1
    m, v = uc.nbf_image('blobs_bytes', 128, 2)
    assert set(np.unique(v)) == {0, 1, 2, 0x7f, 0x80, 0xff} and set(np.unique(m)) >= {0, 0x80}
    # the chart edge suppresses the visibility edge that coincides with it: without the mask the shrink removes more
    m, v = uc.nbf_image('mask_edge', 128, 1)
    with_mask, without = uc.ref_nbf(m, v, [3]), uc.ref_nbf(np.ones_like(m), v, [3])
    assert with_mask.sum() > without.sum() and 0 < with_mask.sum() < (v != 0).sum()
    # every (image, V) and every (kernel list, V) pair occurs at every size
    cases = uc.nbf_cases(100)
    assert {(n, V) for n, V, _ in cases} == {(n, V) for n in uc.NBF_IMAGES for V in uc.NBF_VIEWS}
    assert {(tuple(k), V) for _, V, k in cases} == {(tuple(k), V) for k in uc.nbf_kernel_lists(100) for V in uc.NBF_VIEWS}


# ---------------------------------------------------------------------------------------------------------------------------- NBF routing
def test_nbf_routing_table(L):
    path = lambda V, A, k, am=0: L.pdhip_nbf_path(V, A, ks(*k), len(k), am)
    bits = (uc.BITS_PACK16, uc.BITS_BALLOT)
    assert L.pdhip_debug_set_nbf_path(0) == 0
    assert path(2, 128, [127]) == uc.BITS_PACK16                   # radius 63
    assert path(2, 128, [129]) == uc.BYTES                         # radius 64
    assert path(2, 2048, [97]) == uc.BITS_PACK16                   # (32 + 96) * 32 * 16 = 65536 bytes of LDS
    assert path(2, 2048, [99]) == uc.BYTES
    assert path(2, 2048, [97, 99]) == uc.BYTES                     # one level over the limit takes the whole call
    assert path(2, 4096, [33]) == uc.BITS_PACK16
    assert path(2, 4096, [35]) == uc.BYTES
    assert path(1, 128, [21]) == uc.BYTES                          # V = 1: the bitmaps do not fit the byte workspace
    assert path(2, 4160, [3]) == uc.BYTES                          # a multiple of 64 above 4096
    for A in (1, 5, 63, 65, 100, 127, 129):
        assert path(2, A, [3]) == uc.BYTES
    assert path(2, 128, [21], uc.align_mask(visibility=1)) == uc.BITS_BALLOT
    assert path(2, 128, [21], uc.align_mask(mask=8)) == uc.BITS_BALLOT
    assert path(2, 128, [21], uc.align_mask(out=1)) == uc.BYTES
    assert path(2, 128, [21], uc.align_mask(out=8)) == uc.BYTES    # 8-byte aligned is not enough for a 16-byte store
    assert path(2, 128, [21], uc.align_mask(ws=4)) == uc.BYTES
    assert path(2, 128, [21], uc.align_mask(ws=8)) in bits
    assert path(2, 128, [0]) == uc.COPY and path(1, 5, [0, 2]) == uc.COPY
    assert path(2, 64, [21, 11, 7]) == uc.BITS_PACK16 and path(5, 320, [21, 21, 7]) == uc.BITS_PACK16


def test_nbf_path_hook_forces_and_refuses(L):
    path = lambda V, A, k, am=0: L.pdhip_nbf_path(V, A, ks(*k), len(k), am)
    assert L.pdhip_debug_set_nbf_path(1) == 0
    try:
        assert path(2, 128, [21]) == uc.BYTES and path(2, 128, [0]) == uc.COPY
        assert L.pdhip_debug_set_nbf_path(2) == 1
        assert path(2, 128, [21]) == uc.BITS_BALLOT and path(2, 128, [0]) == uc.COPY
        for args in ((2, 100, [21]), (1, 128, [21]), (2, 128, [129]), (2, 2048, [99]), (2, 128, [21], uc.align_mask(out=1)),
                     (2, 128, [21], uc.align_mask(ws=1))):
            assert path(*args) == E_ARG, args
            assert b'forced' in L.pdhip_last_error()
        # the launcher asks the same function: a forced, ineligible bit path is refused and nothing is launched (no device here to launch on)
        assert L.pdhip_nbf_shrink(PTR, PTR, 2, 100, ks(21), 1, PTR, PTR, None) == E_ARG
        assert L.pdhip_nbf_shrink(PTR, PTR, 2, 128, ks(21), 1, PTR + 1, PTR, None) == E_ARG
        assert L.pdhip_nbf_shrink_shapes(PTR, PTR, 1, 3, 100, ks(21), 1, PTR, PTR, None) == E_ARG
    finally:
        assert L.pdhip_debug_set_nbf_path(0) == 2
    assert path(2, 128, [21]) == uc.BITS_PACK16


# ---------------------------------------------------------------------------------------------------------------------------- refusals
def test_nbf_refusals(L):
    shrink = lambda mask, vis, V, A, k, K, out, ws: L.pdhip_nbf_shrink(mask, vis, V, A, k, K, out, ws, None)
    assert shrink(PTR, PTR, 2, 64, ks(20), 1, PTR, PTR) == E_ARG and b'odd' in L.pdhip_last_error()
    assert shrink(PTR, PTR, 2, 64, ks(21, 4), 2, PTR, PTR) == E_ARG
    assert shrink(PTR, PTR, 2, 64, ks(-3), 1, PTR, PTR) == E_ARG
    assert shrink(PTR, PTR, 2, 64, ks(21), 0, PTR, PTR) == E_ARG   # K = 0
    assert shrink(PTR, PTR, 0, 64, ks(21), 1, PTR, PTR) == E_ARG   # V = 0
    assert shrink(PTR, PTR, 2, 0, ks(21), 1, PTR, PTR) == E_ARG
    assert shrink(PTR, PTR, 2, 64, None, 1, PTR, PTR) == E_ARG
    assert shrink(None, PTR, 2, 64, ks(21), 1, PTR, PTR) == E_ARG and b'null' in L.pdhip_last_error()
    assert shrink(PTR, None, 2, 64, ks(21), 1, PTR, PTR) == E_ARG
    assert shrink(PTR, PTR, 2, 64, ks(21), 1, None, PTR) == E_ARG
    assert shrink(PTR, PTR, 2, 64, ks(21), 1, PTR, None) == E_ARG and b'workspace' in L.pdhip_last_error()
    assert L.pdhip_nbf_shrink_shapes(PTR, PTR, 0, 3, 64, ks(21), 1, PTR, PTR, None) == E_ARG
    assert L.pdhip_nbf_shrink_shapes(PTR, PTR, 2, 0, 64, ks(21), 1, PTR, PTR, None) == E_ARG
    assert L.pdhip_nbf_path(2, 64, ks(20), 1, 0) == E_ARG and L.pdhip_nbf_path(0, 64, ks(21), 1, 0) == E_ARG
    assert L.pdhip_nbf_path(2, 64, ks(21), 0, 0) == E_ARG and L.pdhip_nbf_path(2, 64, None, 1, 0) == E_ARG


def test_view_count_and_bit_transport_refusals(L):
    vis = lambda V, S=1: L.pdhip_texel_visibility_shapes(PTR, V, S, PTR, PTR, 64, PTR, PTR, 0.05, PTR, 128, 1e-4, PTR, None)
    assert vis(33) == E_ARG and b'V=33' in L.pdhip_last_error()
    assert vis(0) == E_ARG and vis(-1) == E_ARG and vis(8, 0) == E_ARG
    assert L.pdhip_texel_visibility(PTR, 33, PTR, PTR, 64, PTR, PTR, 0.05, PTR, 128, 1e-4, PTR, None) == E_ARG
    assert L.pdhip_texel_visibility(PTR, 8, PTR, None, 64, PTR, PTR, 0.05, PTR, 128, 1e-4, PTR, None) == E_ARG
    sel = lambda V, S=1, F=0, K=1, r=64: L.pdhip_view_select_blend_shapes(PTR, V, S, PTR, PTR, PTR, 64, PTR, F, PTR, PTR, PTR, 0.05, PTR, PTR, K,
                                                                          PTR, 1, PTR, r, PTR, PTR, PTR, None)
    assert sel(33) == E_ARG and sel(0) == E_ARG and sel(8, K=0) == E_ARG and sel(8, r=0) == E_ARG
    assert sel(8, S=3, F=0) == E_ARG                               # several shapes need the face count
    assert L.pdhip_view_select_blend(PTR, 33, PTR, PTR, PTR, 64, PTR, PTR, PTR, PTR, 0.05, PTR, PTR, 1, PTR, 1, PTR, 64, PTR, PTR, PTR, None) == E_ARG
    for n in (0, 1, 63, 65, 100):
        assert L.pdhip_pack_bits(PTR, n, PTR, None) == E_ARG and L.pdhip_unpack_bits(PTR, n, PTR, None) == E_ARG, n
    assert L.pdhip_pack_bits(PTR + 1, 64, PTR, None) == E_ARG and L.pdhip_pack_bits(PTR + 8, 64, PTR, None) == E_ARG
    assert L.pdhip_unpack_bits(PTR, 64, PTR + 1, None) == E_ARG and L.pdhip_unpack_bits(PTR, 64, PTR + 8, None) == E_ARG
    assert L.pdhip_pack_bits(None, 64, PTR, None) == E_ARG and L.pdhip_unpack_bits(PTR, 64, None, None) == E_ARG
    assert L.pdhip_compact_texels(PTR, PTR, 0, PTR, PTR, PTR, PTR, PTR, PTR, None) == E_ARG
    assert L.pdhip_compact_texels(None, PTR, 8, PTR, PTR, PTR, PTR, PTR, PTR, None) == E_ARG      # points without gb_pos
    assert L.pdhip_compact_texels(PTR, PTR, 8, None, PTR, PTR, PTR, PTR, PTR, None) == E_ARG      # point_view_ids without view_ids
    assert L.pdhip_compact_texels(PTR, PTR, 8, PTR, PTR, PTR, PTR, None, PTR, None) == E_ARG      # no count


# ---------------------------------------------------------------------------------------------------------------------------- visibility
def test_visibility_reference_equals_the_oracle_on_compacted_points():
    """ref_visibility (dense, any A) against oracle.camera.Camera.transform + oracle.project.point_validation_by_depth on the compacted points,
    the way oracle/unproject.py:37-53 drives them."""
    from oracle import camera as ocam, project as oproj
    for A, R, V, S in ((17, 5, 2, 1), (64, 128, 8, 3), (96, 128, 32, 1)):
        c = uc.vis_case(A, R, V, S)
        got = uc.ref_visibility(c).reshape(S, V, A, A)
        for s in range(S):
            m = c['mask'][s] != 0
            pts = c['gb_pos'][s][m]
            keep = ~np.isnan(pts).any(1)                            # (the oracle indexes out of range on a NaN position, as the reference would)
            tp = np.stack([ocam.Camera(c['cams'][v], R).transform(pts[keep]) for v in range(V)])
            uv = (tp[..., :2] - c['uv_centers'][s * V:(s + 1) * V, None]) / c['uv_scales'][s * V:(s + 1) * V, None, None]
            uv = uv * np.float32(1 - 2 * c['padding']) + np.float32(0.5)
            want, _ = oproj.point_validation_by_depth(R, uv, tp[..., 2], c['mesh'][s * V:(s + 1) * V], offset=0.0001)
            assert np.array_equal(got[s][:, m][:, keep] != 0, want), (A, R, V, S, s)
            assert not got[s][:, m][:, ~keep].any() and not got[s][:, ~m].any()


def test_visibility_cases_hold_what_they_promise():
    c = uc.vis_case(96, 128, 8, 3)
    ref = uc.ref_visibility(c)
    inside = np.broadcast_to((c['mask'] != 0)[:, None], (3, 8, 96, 96)).reshape(24, 96, 96)
    assert 0.2 < ref[inside].mean() < 0.8                            # both verdicts in numbers
    assert np.isnan(c['gb_pos'][c['mask'] != 0]).any() and c['n_ties'] >= 3
    u, t, _ = uc._project(c['cams'], c['gb_pos'], c['uv_centers'], c['uv_scales'], None, np.float32(0.9), np.float32)
    with np.errstate(invalid='ignore'):
        outside = ((u < 0) | (u > 1) | (t < 0) | (t > 1)) & inside.reshape(u.shape)
    assert outside.sum() > 100                                       # texels that project outside the view and are clamped
    assert not np.array_equal(c['uv_scales'][:8], c['uv_scales'][8:16])


@pytest.mark.parametrize("V", uc.VIEWS)
def test_visibility_bands_bound_the_measured_rounding(V):
    """Over every case: the float32 contract and the float64 restatement differ by at most the figures written down in the common module (so
    the bands are four times what rounding does), the float64 check leaves out at most 2 % of the texel-view pairs inside the mask, and where
    it binds the float32 reference gives the float64 verdict."""
    worst = [0.0, 0.0]
    for A, R, S in uc.vis_cases(V) + ([(1088, 128, 1)] if V == 8 else []):
        c = uc.vis_case(A, R, V, S)
        verdict, counted, dz, du = uc.ref_visibility_f64(c)
        worst = [max(worst[0], dz), max(worst[1], du)]
        inside = np.broadcast_to((c['mask'] != 0)[:, None], (S, V, A, A)).reshape(S * V, A, A)
        left_out = int((inside & ~counted).sum())
        assert left_out <= uc.LEFT_OUT_CAP * inside.sum(), (A, R, S, left_out, int(inside.sum()))
        ref = uc.ref_visibility(c)
        assert np.array_equal(ref[counted], verdict[counted]), (A, R, S)
    print(f"V={V}: largest f32 - f64 difference: margin {worst[0]:.3g}, uv {worst[1]:.3g}")
    assert worst[0] <= uc.ZN_DIFF_MEASURED and worst[1] <= uc.UV_DIFF_MEASURED, worst


# ---------------------------------------------------------------------------------------------------------------------------- selection
def test_selection_reference_equals_the_oracle_unproject():
    """ref_view_select against oracle.unproject.unproject at A = 256 (the smallest size the oracle accepts): same visibility and levels in, same
    view ids, colours and painted mask out."""
    from oracle import camera as ocam, unproject as ounp
    A, V, R, r = 256, 8, 128, 64
    rng = np.random.default_rng(5)
    c = uc.sel_case(A, V, 2, r, 1)
    c['scale_factors'] = rng.uniform(0.8, 1.25, V).astype(np.float32)
    mesh = rng.uniform(0.980, 0.993, (V, R, R)).astype(np.float32)
    keep = ~np.isnan(c['gb_pos'][0]).any(-1) & (c['mask'][0] != 0)
    mask = keep[None, :, :, None]
    ocams = [ocam.Camera(c['cams'][v], R) for v in range(V)]
    for complete in (False, True):
        o = ounp.unproject(c['inpainted'], c['f_normals'][0], r, ocams, R, c['dirs'], c['gb_pos'], mask, c['face_id'], c['uv_centers'][:, None],
                           c['uv_scales'][:, None, None], c['padding'], c['scale_factors'], mesh, [7, 3], complete)
        d = dict(c, mask=keep[None].astype(np.uint8), vis=o['visibility'].transpose(2, 0, 1).astype(np.uint8),
                 shrinked=o['per_kernel'][:2].astype(np.uint8))
        atlas, painted, vid, _ = uc.ref_view_select(d, complete)
        assert np.array_equal(vid[0][keep], o['point_view_ids'])
        assert np.array_equal(atlas[0], o['atlas_img']) and np.array_equal(painted[0] != 0, o['atlas_painted_mask'])
        assert (vid[0][~keep] == -1).all()


@pytest.mark.parametrize("V", uc.VIEWS)
def test_selection_cases_hold_every_class_of_texel(V):
    for A, K, complete, r, S in uc.sel_cases(V):
        c = uc.sel_case(A, V, K, r, S)
        cand, cls = uc.sel_candidates(c, complete)
        counts = [int((cls == k).sum()) for k in range(4)]
        if A >= 64:
            for k in range(4):
                if k == 1 and K == 1:
                    assert counts[1] == 0                           # one level: nothing looser to fall back to
                else:
                    assert counts[k] >= uc.MIN_PER_CLASS, (A, K, complete, r, S, counts)
        atlas, painted, vid, sim = uc.ref_view_select(c, complete)
        inside = c['mask'] != 0
        assert (vid[~inside] == -1).all() and not painted[~inside].any() and not atlas[~inside].any()
        none = (cls == 3) if complete else (cls >= 2)
        if complete:
            assert (vid[inside] >= 0).all() and (vid[none] == 0).all()      # no candidate anywhere: every weight is -100, the first view wins
        else:
            assert (vid[none] == -100).all() and not painted[none].any()
        assert vid.max() <= V - 1
        if V == 32 and A > 1:
            assert (vid == 31).any()
        f64, decided = uc.f64_selection(c, complete)
        assert np.array_equal(vid[decided], f64[decided]), (A, K, complete, r, S)
        if A >= 64:
            assert decided.sum() > 0.3 * (inside & cand.any(1)).sum()
            nrm = c['f_normals'][np.arange(S)[:, None, None], c['face_id']]
            assert np.isnan(nrm[inside]).any() and (nrm[inside] == 0).all(-1).any() and (np.linalg.norm(nrm[inside & ~np.isnan(nrm).any(-1)], axis=-1) > 2000).any()


# ---------------------------------------------------------------------------------------------------------------------------- compaction, bits
def test_compaction_and_packing_references():
    for A in uc.COMPACT_SIZES:
        for name in uc.COMPACT_MASKS:
            mask, gb, vid = uc.compact_case(A, name)
            pts, coords, pv, offs = uc.ref_compact(mask, gb, vid)
            P = int((mask != 0).sum())
            assert len(pts) == len(coords) == len(pv) == P == offs[A] and offs[0] == 0
            assert P == {'empty': 0, 'full': A * A, 'last_column': 1}.get(name, P)
            for i in (0, P // 2, P - 1) if P else ():
                y, x = coords[i]
                assert mask[y, x] and np.array_equal(pts[i], gb[y, x]) and pv[i] == vid[y, x] and offs[y] <= i < offs[y + 1]
    b = uc.pack_case(128)
    w = uc.ref_pack(b)
    assert w.dtype == np.uint64 and len(w) == 2
    for i in range(128):
        assert ((int(w[i // 64]) >> (i % 64)) & 1) == (b[i] != 0)
