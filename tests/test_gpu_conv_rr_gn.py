"""GPU: the GroupNorm (+ FiLM) + SiLU that k_conv_rr applies while staging its input (csrc/nn_conv_rr.hip), pinned for every tile variant that carries it.
The probe of tests/conv_rr_gn_common.py -- a 1x1 conv with identity weights, so that the output IS the staged tensor -- is held to the float64 reference
under the per-element bound the stand-alone k_gn_apply passes (tests/nn_ops_common.py; no tolerance of this file's own), and to bit equality with
pdhip_gn_apply_parts_f16 on the same octet partials, which holds the in-kernel statistics to the same summation order: one wrong group mean fails every
element of the group.  The partials are built in torch over uneven pixel runs, so the chunk counts need not divide H * W.  tests/test_conv_rr_gn_cpu.py shows
on the host that the comparison has teeth and that every case is planned onto the variant it names."""
import ctypes as C
import functools

import pytest
import torch

import conv_rr_gn_common as cm
import nn_ops_common as oc
from conftest import note_measured
from nn_hooks_common import hook

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
ENGINE_CFG = cm.ENGINE_CFG
TILE_FRAGMENTS = {1: 4, 2: 16, 3: 16, 5: 4}              # MT x NF of the variant: one split-K slice is that many KiB of f32


@pytest.fixture(scope="module")
def L():
    assert torch.cuda.is_available()
    from pointdreamer_amd import _lib
    import pointdreamer_amd.ddnm_inpainting  # noqa: F401
    return _lib.lib()


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


@functools.lru_cache(maxsize=None)
def _identity_fragments(L, Cc):
    """The C x C f16 identity as a 1x1 conv's weights, fragment-major."""
    wp = torch.eye(Cc, dtype=torch.float16, device=DEV)
    wf = torch.empty((L.pdhip_conv_rr_weight_halfs(Cc, 1, 0, Cc),), dtype=torch.float16, device=DEV)
    assert L.pdhip_conv_rr_pack_f16(_ptr(wp), Cc, 1, 0, Cc, _ptr(wf), _stream()) == 0, L.pdhip_last_error()
    torch.cuda.synchronize()
    return wf


@functools.lru_cache(maxsize=2)
def _inputs(W, Cc):
    return tuple(t.to(DEV) for t in oc.gn_inputs(cm.N_IMG, W, W, Cc))


def _probe(L, variant, slabs, x, Ca, mode, gamma, beta, film, pa, pb, ws):
    """(rc, y): pdhip_conv_rr_f16 as the probe into a NaN-filled y.  x [N, W, W, C]; Ca < C: two sources."""
    N, W, Cc = x.shape[0], x.shape[1], x.shape[-1]
    xa = x[..., :Ca].contiguous()
    xb = x[..., Ca:].contiguous() if Ca < Cc else None
    y = torch.full((N, W, W, Cc), float('nan'), dtype=torch.float16, device=DEV)
    with hook('conv_rr', 2, variant, slabs):
        rc = L.pdhip_conv_rr_f16(_ptr(xa), _ptr(xb), Cc, Ca, mode, _ptr(gamma), _ptr(beta), _ptr(film), 2 * Cc, _ptr(pa), pa.shape[1], _ptr(pb),
                                 pb.shape[1] if pb is not None else 0, None, None, 0, 0, 1, _ptr(_identity_fragments(L, Cc)), None, None, 0, _ptr(y), N, W, W, Cc,
                                 _ptr(ws), ws.numel(), None, None, _stream())
    torch.cuda.synchronize()
    return rc, y


def _workspace(c):
    tiles = cm.N_IMG * (c['W'] * c['W'] // {8: 64, 16: 128, 32: 128}[c['W']]) * (c['C'] // (16 if c['W'] == 8 else 32))
    return torch.zeros((4096 + (tiles * c['slabs'] * TILE_FRAGMENTS[c['variant']] * 256 if c['slabs'] > 1 else 0),), dtype=torch.float32, device=DEV)


@pytest.mark.parametrize("c", cm.CASES, ids=[c['name'] for c in cm.CASES])
def test_staged_groupnorm_vs_f64_bound_and_stand_alone_pass(L, c):
    """Per case: the probe lies within the per-element bound of the float64 reference fed the statistics the partials imply, with no element left unwritten;
    it equals pdhip_gn_apply_parts_f16 on the same partials bit for bit; a repeated call gives the same bits and the tickets are back at zero.
    Largest error / bound ratio on an MI355X: 0.9998 for each of the variants 1, 2, 3 and 5, in cases without FiLM and SiLU, where the bound is half an f16
    spacing and rounding to nearest attains it (nn_ops_common.py) -- a record, not a threshold: the assertion is <= 1."""
    N, W, Cc, Ca = cm.N_IMG, c['W'], c['C'], c['Ca']
    x, gamma, beta, film = _inputs(W, Cc)
    film = film if c['film'] else None
    pa, pb = cm.case_partials(c, x)
    mean, rstd = cm.implied_stats([pa] + ([pb] if pb is not None else []), W * W)
    ref, bound = cm.reference(x, gamma, beta, film, c['mode'], mean, rstd)
    ws = _workspace(c)
    rc, y = _probe(L, c['variant'], c['slabs'], x, Ca, c['mode'], gamma, beta, film, pa, pb, ws)
    assert rc == 0, L.pdhip_last_error()
    ratio = oc.worst_ratio(y, ref, bound)
    print(f"{c['name']}: worst error / bound = {ratio:.4f}")
    note_measured(test='conv_rr_gn_probe', case=c['name'], variant=c['variant'], ratio=ratio)
    assert not bool(torch.isnan(y).any()), "elements never written"
    assert ratio <= 1, ratio
    # the stand-alone pass on the same partials
    h = torch.full_like(y, float('nan'))
    xa = x[..., :Ca].contiguous()
    xb = x[..., Ca:].contiguous() if c['Cb'] else None
    rc = L.pdhip_gn_apply_parts_f16(_ptr(xa), _ptr(xb), Ca, Cc, _ptr(pa), c['chunksA'], _ptr(pb), c['chunksB'], _ptr(gamma), _ptr(beta), _ptr(film), 2 * Cc, N, W, W,
                                    1 if c['mode'] == 2 else 0, _ptr(h), _stream())
    assert rc == 0, L.pdhip_last_error()
    torch.cuda.synchronize()
    assert torch.equal(y, h), f"{int((y != h).sum())} elements differ from the two-pass form, channels {sorted(set((y != h).nonzero()[:, 3].tolist()))[:8]}"
    rc, y2 = _probe(L, c['variant'], c['slabs'], x, Ca, c['mode'], gamma, beta, film, pa, pb, ws)
    assert rc == 0 and torch.equal(y, y2)
    assert int(ws[:4096].abs().sum().item()) == 0


@pytest.mark.parametrize("name,variant,Ca,Cb,chA,chB,msg", cm.REFUSALS, ids=[r[0] for r in cm.REFUSALS])
def test_refused_sources_name_their_reason_and_launch_nothing(L, name, variant, Ca, Cb, chA, chB, msg):
    W, Cc = cm.VARIANTS[variant][0], Ca + Cb
    x, gamma, beta, film = _inputs(W, Cc)
    c = dict(Ca=Ca, Cb=Cb, chunksA=chA, chunksB=chB)
    pa, pb = cm.case_partials(c, x)
    ws = torch.zeros((4096,), dtype=torch.float32, device=DEV)
    rc, y = _probe(L, variant, 1, x, Ca, 2, gamma, beta, film, pa, pb, ws)
    assert rc != 0 and msg in L.pdhip_last_error(), L.pdhip_last_error()
    assert bool(torch.isnan(y).all()) and int(ws.abs().sum().item()) == 0


def test_engine_forward_with_in_staging_groupnorm_at_256_channels(L):
    """The smallest UNet whose 8^2 level has 256 channels (its ResBlock convs there run on variant 1, one 256-channel unit of 32 groups: test_conv_rr_gn_cpu.py reads
    that off the route table): the forward with the in-staging GroupNorm equals the two-pass routing bit for bit."""
    from oracle import unet as ounet
    import pointdreamer_amd.ddnm_inpainting as di
    cfg = ounet.make_config(ENGINE_CFG['image_size'], ENGINE_CFG['num_channels'], ENGINE_CFG['num_res_blocks'], ENGINE_CFG['attention_resolutions'],
                            ENGINE_CFG['num_head_channels'], True, channel_mult=tuple(int(v) for v in ENGINE_CFG['channel_mult'].split(',')))
    w = ounet.random_weights(cfg, 5)
    m = di.UNetModel(max_batch=2, device=DEV, **ENGINE_CFG)
    assert m.load_state_dict(w, strict=True) == len(w)
    g = torch.Generator().manual_seed(11)
    x = torch.randn((2, 3, 32, 32), generator=g).to(DEV)
    t = torch.tensor([650.0, 40.0], device=DEV)
    base = m(x, t).cpu()
    try:
        L.pdhip_debug_set_rr_gn(8)
        fused = m(x, t).cpu()
    finally:
        L.pdhip_debug_set_rr_gn(0)
    assert bool(torch.isfinite(base).all()) and float(base.abs().max()) > 0
    assert torch.equal(fused, base), (fused - base).abs().max().item()
    assert torch.equal(m(x, t).cpu(), base)                # the hook is back at its default
