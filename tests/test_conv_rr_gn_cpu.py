"""CPU: what tests/test_gpu_conv_rr_gn.py relies on, checked without a device (tests/conv_rr_gn_common.py).  The comparison has teeth: a torch emulation of
the staged element map passes it, each mistake the kernel's statistics code can make fails it on the group it touches.  The grid covers what its docstring
claims.  The host's bound on the groups of a staged unit is the kernel's own expression.  And every GPU case is planned onto the variant it names
(conv_rr_plan is host code, asked through pdhip_conv_rr_plan: pdhip_debug_conv_launch_nhwc_f16 plans without fragment-major weights and a GroupNorm wish, so it
never reaches this kernel's variants)."""
import ctypes as C
import itertools

import pytest
import torch

import conv_rr_gn_common as cm
import nn_ops_common as oc

ENGINE_CFG = cm.ENGINE_CFG


# ---- the comparison has teeth
def _emulated(Cs, chunks, mode, film, mistake=None, at=(1, 0)):
    """(staged map from the kernel's statistics arithmetic with `mistake`, reference, bound, x) for an 8 x 8 image."""
    C_ = sum(Cs)
    c = dict(W=8, C=C_, Ca=Cs[0], Cb=C_ - Cs[0], chunksA=chunks[0], chunksB=chunks[-1])
    x, gamma, beta, fl = cm.inputs(c)
    fl = fl if film else None
    pa, pb = cm.case_partials(c, x)
    parts = [pa] + ([pb] if pb is not None else [])
    mean, rstd = cm.implied_stats(parts, 64)
    ref, bound = cm.reference(x, gamma, beta, fl, mode, mean, rstd)
    m32, r32 = cm.kernel_stats(parts, list(Cs), 64, mistake, at)
    return cm.staged_map(x, gamma, beta, fl, mode, m32, r32), ref, bound


TEETH = [((256,), (9,)), ((1536,), (5,)), ((512, 256), (5, 3)), ((1024, 512), (7, 2))]


@pytest.mark.parametrize("Cs,chunks", TEETH)
@pytest.mark.parametrize("mode,film", [(1, False), (2, True)])
def test_honest_emulation_passes_and_each_statistics_mistake_fails(Cs, chunks, mode, film):
    got, ref, bound = _emulated(Cs, chunks, mode, film)
    assert oc.worst_ratio(got, ref, bound) <= 1
    C_ = sum(Cs)
    cg = C_ // 32
    # the group that lies across the A | B boundary where there is one, else one in the middle; image 1, so that a missing per-image offset shows
    g = Cs[0] // cg if len(Cs) == 2 and Cs[0] % cg else 13
    mistakes = ['zero_mean', 'neighbour', 'drop_last_chunk', 'image0'] + (['chunks_of_b'] if len(Cs) == 2 and Cs[0] % cg else [])
    for mistake in mistakes:
        bad, _, _ = _emulated(Cs, chunks, mode, film, mistake, (1, g))
        assert cm.group_ratio(bad, ref, bound, 1, g) > 1, mistake
        assert oc.worst_ratio(bad, ref, bound) > 1, mistake
        # ... and nothing but that group moved
        same = torch.ones(C_, dtype=torch.bool)
        same[g * cg:(g + 1) * cg] = False
        assert torch.equal(bad[..., same], got[..., same]) and torch.equal(bad[0], got[0]), mistake


def test_an_element_never_written_fails_the_comparison():
    got, ref, bound = _emulated((256,), (9,), 2, True)
    got = got.clone()
    got[1, 3, 5, 77] = float('nan')
    assert oc.worst_ratio(got, ref, bound) == float('inf')


# ---- the grid covers what it claims
def test_grid_covers_every_class_with_every_variant():
    configs = [(C_, 0) for C_ in cm.SINGLE_C] + list(cm.TWO_SOURCE)
    names = [c['name'] for c in cm.CASES]
    assert len(set(names)) == len(names)
    for v, (W, cs) in cm.VARIANTS.items():
        mine = [c for c in cm.CASES if c['variant'] == v]
        assert {(c['Ca'], c['Cb']) for c in mine} == set(configs), v
        assert {c['cls'] for c in mine} == set(cm.CHUNK_CLASSES), v
        assert {(c['mode'], c['film']) for c in mine} == set(itertools.product((1, 2), (False, True))), v
        assert {c['slabs'] > 1 for c in mine} == {False, True}, v
        assert any(c['Cb'] and c['slabs'] > 1 for c in mine) and any(c['Cb'] and c['film'] for c in mine), v
        for c in mine:
            assert c['W'] == W and c['C'] % cs == 0 and c['Ca'] % cs == 0 and (c['C'] // 32) % 8 == 0 and (c['C'] // cs) % c['slabs'] == 0
            pps = cm.pps_of(c['C'])
            assert 1 <= c['chunksA'] <= 8 * pps and (not c['Cb'] or (1 <= c['chunksB'] <= 8 * pps and c['chunksB'] != c['chunksA'])), c['name']
            if c['cls'] == 'odd':
                assert c['chunksA'] % 2 == 1 and 2 * pps < c['chunksA'] < 8 * pps
        assert {c['cls'] for c in mine if c['slabs'] == c['C'] // cs and c['slabs'] > 1}, v
    one = [c for c in cm.CASES if (c['variant'], c['Ca'], c['Cb']) == (1, 256, 0)]
    assert {c['cls'] for c in one} == set(cm.CHUNK_CLASSES)
    # every refusal is one chunk beyond what a slot can load, or a group size that is no multiple of 8
    for name, v, Ca, Cb, chA, chB, msg in cm.REFUSALS:
        pps = cm.pps_of(Ca + Cb)
        assert max(chA, chB) == 8 * pps + 1 or ((Ca + Cb) // 32) % 8 != 0, name
    assert {v for _, v, *_ in cm.REFUSALS} == set(cm.VARIANTS)


def test_grid_reaches_32_groups_only_at_variant_1_with_256_channels_and_flags_every_straddle():
    assert max(c['groups_max'] for c in cm.CASES) == 32
    assert {(c['variant'], c['Ca'], c['Cb']) for c in cm.CASES if c['groups_max'] == 32} == {(1, 256, 0)}
    for c in cm.CASES:
        cg = c['C'] // 32
        # from the channel ranges alone: group g = channels [g cg, (g + 1) cg)
        across_ab = any(g * cg < c['Ca'] < (g + 1) * cg for g in range(32)) if c['Cb'] else False
        across_unit = any(g * cg < u < (g + 1) * cg for g in range(32) for u in range(c['cs'], c['C'], c['cs']))
        assert c['straddles_ab'] == across_ab and c['straddles_unit'] == across_unit, c['name']
    for v in cm.VARIANTS:
        assert {(c['Ca'], c['Cb']) for c in cm.CASES if c['variant'] == v and c['straddles_ab']} == {(512, 256), (1024, 512)}
    assert {c['C'] for c in cm.CASES if c['straddles_unit'] and not c['Cb']} == {768, 1536}


# ---- the host side
@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as ge
    ge.build()
    from pointdreamer_amd import _lib
    import pointdreamer_amd.ddnm_inpainting  # noqa: F401  (registers the entry points)
    return _lib.lib()


def accepted_channels():
    """Every C the launcher's checks (conv_rr's fill) accept with gn_mode != 0: a multiple of 32 with 8 k channels per group, C / 8 <= 256 octets, a power of two
    of pixel slots, at most 8 statistics threads per group."""
    out = []
    for C_ in range(32, 4097, 32):
        cg, pps = C_ // 32, max(1, 256 // (C_ // 8))
        if cg % 8 == 0 and C_ // 8 <= 256 and pps & (pps - 1) == 0 and (cg // 8) * pps <= 8:
            out.append(C_)
    return out


def test_host_group_bound_is_the_kernels_expression(L):
    cap = C.c_int(-1)
    acc = accepted_channels()
    assert set(cm.SINGLE_C) | {a + b for a, b in cm.TWO_SOURCE} <= set(acc)
    worst = {}
    for cs in (128, 256):
        for C_ in range(32, 4097, 32):
            want = max(cm.unit_groups(cs, C_))
            assert L.pdhip_conv_rr_gn_groups_max(cs, C_, C.byref(cap)) == want, (cs, C_)
            assert cap.value == min(cs // 8 + 1, 32)
            if C_ in acc and C_ % cs == 0:
                worst[cs] = max(worst.get(cs, 0), want)
                assert want <= cap.value, (cs, C_, want)                     # no accepted source has a unit beyond its variant's tables
    assert worst == {128: 16, 256: 32}
    # the table the fix was derived from, worked by hand (768 = 24 per group: channels 128 ... 255 lie in groups 5 ... 10; 1536 = 48 per group: 256 ... 511 alike)
    table = {cs: [max(cm.unit_groups(cs, C_)) for C_ in cm.SINGLE_C] for cs in (256, 128)}
    assert table == {256: [32, 16, 12, 8, 6, 4], 128: [16, 8, 6, 4, 4, 2]}
    assert L.pdhip_conv_rr_gn_groups_max(256, 0, None) == 0 and L.pdhip_conv_rr_gn_groups_max(0, 256, None) == 0 and L.pdhip_conv_rr_gn_groups_max(128, 8192, None) == 0


def _rr_plan(L, c_or_shape, variant, slabs, want_gn=1, taps=1, ws_floats=1 << 40):
    N, W, Cin, Cout = c_or_shape
    plan = (C.c_int * 7)()
    old = L.pdhip_debug_set_conv_rr(2, variant, slabs)
    try:
        v = L.pdhip_conv_rr_plan(N, W, W, Cin, Cout, taps, 0, ws_floats, want_gn, plan)
    finally:
        L.pdhip_debug_set_conv_rr(old, 0, 0)
    assert v == plan[0]
    return list(plan)


@pytest.mark.parametrize("c", cm.CASES, ids=[c['name'] for c in cm.CASES])
def test_every_gpu_case_plans_onto_the_variant_and_slabs_it_names(L, c):
    v, s0, u0, s1, u1, bands, ntiles = _rr_plan(L, (cm.N_IMG, c['W'], c['C'], c['C']), c['variant'], c['slabs'])
    assert (v, s0, s0 * u0, s1) == (c['variant'], c['slabs'], c['C'] // c['cs'], 0), (v, s0, u0, s1)
    assert cm.N_IMG * bands * ntiles <= 4096                                # the ticket table


def test_automatic_selection_serves_the_32_group_unit(L):
    """pdhip_conv_rr_f16(gn_mode != 0, C = 256, 8 x 8) selects variant 1 by itself -- whose tables now hold the 32 groups of its one unit -- for the probe and for the
    two 3x3 rows added to test_gpu_round6.py."""
    for want_gn in (0, 1):
        assert _rr_plan(L, (cm.N_IMG, 8, 256, 256), 0, 0, want_gn)[0] == 1
    for row in cm.ROUND6_ROWS:
        N, HW, Ca, Cb, Cout = row[:5]
        assert (Ca, Cb, row[11], row[12]) == (256, 0, 0, 0)
        for want_gn in (0, 1):                                             # (the two-pass form the row is compared with runs the raw input on the same tiles)
            assert _rr_plan(L, (N, HW, Ca, Cout), 0, 0, want_gn, taps=9, ws_floats=4096 + 4 * 1024 * 1024)[0] == 1


def test_forced_variant_without_room_is_not_planned(L):
    """A variant is never planned for a GroupNorm source whose units touch more groups than its tables serve: 128 channels (4 per group) give a 128-channel unit 32
    groups against 17 rows.  The same layer with a raw input is planned."""
    assert L.pdhip_conv_rr_gn_groups_max(128, 128, None) == 32
    assert _rr_plan(L, (1, 8, 128, 128), 5, 0, want_gn=1)[0] == 0
    assert _rr_plan(L, (1, 8, 128, 128), 5, 0, want_gn=0)[0] == 5


def test_engine_case_has_in_staging_layers_at_variant_1_with_256_channels(L):
    import pointdreamer_amd.ddnm_inpainting as di
    from nn_hooks_common import hook
    base = di.unet_route_table(1, **ENGINE_CFG)
    with hook('rr_gn', 8):
        rows = [r.split() for r in di.unet_route_table(1, **ENGINE_CFG)]
    assert di.unet_route_table(1, **ENGINE_CFG) == base
    hit = [r for r in rows if r[1] == '8x8' and r[2] == '256->256' and r[3] == 'rr' and r[4].startswith('variant=1,') and 'in_gn' in r[6].split(',')]
    assert len(hit) >= 2 and any('in_layers' in r[0] for r in hit) and any('out_layers' in r[0] for r in hit), rows
    assert not any('in_gn' in r for r in base)
    # the same layers run the same tile variant without the hook: the two forwards can be compared bit for bit
    by = {r.split()[0]: r.split() for r in base}
    assert all(by[r[0]][3:5] == r[3:5] for r in hit)
