"""Round-3 GPU parity tests: D1 o U1 at full size over several sampler steps against the reference's own sampler driving the
reference's own fp32 UNet (tools/gen_golden_nn.py ddnm_full), the small-batch routing of the UNet engine (in-kernel split-K
combine, GroupNorm statistics reduced inside the apply kernel), and the RCCL all-gather of the view-parallel driver executed on
the one GPU there is."""
import ctypes as C
import math
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import load_golden, note_measured, U1_FP32_LINF, U1_FP32_L2
from oracle import unet as ounet

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = 'cuda:0'


@pytest.fixture(scope="module")
def nn():
    assert torch.cuda.is_available()
    from pointdreamer_amd import _lib
    import pointdreamer_amd.ddnm_inpainting as di
    return dict(L=_lib.lib(), lib=_lib, di=di)


def _ptr(t):
    return C.c_void_p(t.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _rel(a, b):
    a, b = a.double(), b.double()
    return ((a - b).abs().max() / b.abs().max()).item(), ((a - b).norm() / b.norm()).item()


@pytest.fixture(scope="module")
def full_model(nn):
    cfg = ounet.make_config(256, 256, 2, "32,16,8", 64, True)
    w = ounet.random_weights(cfg, 12)
    m = nn['di'].UNetModel(max_batch=8, device=DEV, **nn['di'].IMAGENET_256)
    m.load_state_dict(w, strict=True)
    del w
    return m


# D1 o U1 drift bound: relative L2 of the sampler state x_k against the reference's fp32 run after k + 1
# updates <= DRIFT_L2 * sqrt(k + 1), relative L-inf <= DRIFT_LINF * sqrt(k + 1).  The per-forward budget of U1 is 5e-3 / 2e-2;
# the DDNM update maps an error of e_t one-to-one into x (the 1/sqrt(a_t) of Eq. 12 is undone by sqrt(a_{t-1}) of the re-noising),
# so independent per-step errors compound like a random walk.
DRIFT_L2, DRIFT_LINF = 1.0e-3, 1.5e-3       # measured (round 3): 3.3e-4 / 3.4e-4 at batch 1 and 8


@pytest.mark.parametrize("batch", [1, 8])
def test_ddnm_unet_full_multistep_vs_reference_sampler(nn, full_model, batch):
    """The reference's simplified_ddnm_inpainting (diffusion.py:459-570) with the reference's fp32 UNetModel (unet.py:396-664,
    552.8 M parameters) for the first 10 steps of the 100-step schedule, state recorded after every update; the engine runs the
    same steps (pdhip_unet_forward + pdhip_ddnm_step with the fixture's noise tape) at UNet batch 1 and 8."""
    from tools.gen_golden_nn import ddnm_full_inputs
    L = nn['L']
    g = load_golden('ddnm_unet_full.npz')
    steps, n_img, st = int(g['steps']), int(g['n_img']), int(g['stride'])
    masked, masks, tape = ddnm_full_inputs(int(g['seed']), n_img, steps)
    sel = [i % n_img for i in range(batch)]                       # batch 8: the two fixture images four times each
    mk = torch.from_numpy(masked[sel]).to(DEV).contiguous()
    ms = torch.from_numpy(masks[sel]).to(DEV).contiguous()
    tp = torch.from_numpy(tape[sel]).to(DEV)                      # [batch, steps + 1, 3, S, S]
    HW = 256 * 256
    y = torch.empty_like(mk)
    assert L.pdhip_ddnm_prepare(_ptr(mk), _ptr(ms), _ptr(y), batch, HW, _stream()) == 0
    x = tp[:, 0].clone().contiguous()
    _, _, t_sched, _, _ = nn['di'].ddnm_schedule()
    worst = (0.0, 0.0)
    for k in range(steps):
        tt = torch.full((batch,), float(t_sched[k]), device=DEV)
        et = full_model(x, tt)
        eps = tp[:, k + 1].contiguous()
        assert L.pdhip_ddnm_step(_ptr(x), _ptr(et), 6, _ptr(y), _ptr(ms), _ptr(eps), 0, k, batch, HW, _stream()) == 0, L.pdhip_last_error()
        xs = x[:, :, ::st, ::st].cpu()
        for b in range(batch):
            linf, l2 = _rel(xs[b], torch.from_numpy(g['xs'][sel[b], k]))
            worst = (max(worst[0], linf / np.sqrt(k + 1)), max(worst[1], l2 / np.sqrt(k + 1)))
            assert l2 <= DRIFT_L2 * np.sqrt(k + 1) and linf <= DRIFT_LINF * np.sqrt(k + 1), (batch, b, k, linf, l2)
    print(f"D1oU1 drift, batch {batch}: worst rel L-inf / sqrt(k) {worst[0]:.2e}, rel L2 / sqrt(k) {worst[1]:.2e}")
    for b in range(batch):
        linf, l2 = _rel(x[b].cpu(), torch.from_numpy(g['x_last'][sel[b]]))
        assert l2 <= DRIFT_L2 * np.sqrt(steps) and linf <= DRIFT_LINF * np.sqrt(steps), (batch, b, linf, l2)
    # the sampler entry point (one call, no host in the loop) composes the same steps: identical to the step-by-step run
    inp = nn['di'].Inpainter.__new__(nn['di'].Inpainter)
    inp.device, inp.model, inp.seed, inp.n_steps, inp._images, inp.max_batch = torch.device(DEV), full_model, 1234, steps, 0, 8
    out = inp.inpaint_views(mk, ms, x_T=tp[:, 0].contiguous(), eps_tape=tp[:, 1:].permute(1, 0, 2, 3, 4).contiguous(), n_steps=steps)
    assert torch.equal(out, torch.clamp((x + 1) / 2, 0, 1))


def test_unet_small_batch_routing_variants(nn, full_model):
    """Batch-1 / batch-2 forwards under the small-batch routing (GroupNorm statistics reduced inside the apply kernel, in-kernel
    split-K combine) against the two-launch forms they replace: same tolerance class as batched-vs-batch-1."""
    L = nn['L']
    g = load_golden('unet_full.npz')
    x1 = torch.from_numpy(g['x']).to(DEV)
    t1 = torch.from_numpy(g['t']).to(DEV)
    st = int(g['stride'])
    for N in (1, 2):
        x, t = x1.repeat(N, 1, 1, 1).contiguous(), t1.repeat(N).contiguous()
        outs = {}
        for fin, sk in ((4, 1), (0, 1), (4, 0), (0, 0)):
            old, olds = L.pdhip_debug_set_fold_finalize(fin), L.pdhip_debug_set_conv_sk(sk, 0, 0)
            try:
                outs[(fin, sk)] = full_model(x, t).cpu()
                again = full_model(x, t).cpu()
            finally:
                L.pdhip_debug_set_fold_finalize(old); L.pdhip_debug_set_conv_sk(olds, 0, 0)
            assert torch.equal(outs[(fin, sk)], again), "a forward is deterministic (fixed-order in-launch split-K combine)"
            for b in range(N):
                linf, l2 = _rel(outs[(fin, sk)][b:b + 1, :, ::st, ::st], torch.from_numpy(g['ref_out']))
                note_measured(test='unet_full_fp32_routing', batch=N, fin=fin, sk=sk, linf=linf, l2=l2)
                assert linf <= U1_FP32_LINF and l2 <= U1_FP32_L2, (N, fin, sk, b, linf, l2)
        for key in ((0, 1), (4, 0), (0, 0)):
            linf, l2 = _rel(outs[(4, 1)], outs[key])
            assert linf <= 4e-3 and l2 <= 2.5e-3, (N, key, linf, l2)   # (two f16 routings of the same net: both inside the U1 budget, and this close to each other)


@pytest.mark.parametrize("tile,splits", [(1, 1), (1, 2), (2, 1), (2, 3), (3, 1), (3, 5), (4, 1), (4, 8), (4, 16), (0, 0)])
@pytest.mark.parametrize("N,H,W,Cin,Cout,k,res", [
    (1, 8, 8, 128, 256, 3, True),          # one 64-pixel image: the 8^2 level (weight stream)
    (3, 8, 8, 192, 136, 3, False),         # M = 192 (not a multiple of 128), Cout not a multiple of the tile
    (1, 16, 16, 256, 128, 3, True),
    (2, 32, 32, 64, 64, 3, False),
    (1, 16, 16, 320, 384, 1, True),        # 1x1 (qkv / proj / skip shapes), K-steps 5: uneven slices
    (2, 8, 8, 1024, 256, 1, False),
])
def test_conv_sk_small_m_kernel_vs_torch_fp32(nn, N, H, W, Cin, Cout, k, res, tile, splits):
    """k_conv_sk (nn_conv_sk.hip): every tile shape, split factors incl. uneven K slices, in-launch combine; vs F.conv2d in fp32 on
    the same f16-rounded operands, and bit-identical when repeated (the combine order does not depend on the arrival order)."""
    from test_gpu_nn import hip_conv
    import torch.nn.functional as F
    L = nn['L']
    if tile in (1, 2) and (H * W) % 128 != 0 and H * W != 64:
        pytest.skip("128-row tiles need H * W % 128 == 0 (or two whole 64-pixel images per tile)")
    g = torch.Generator().manual_seed(1000 * tile + splits + Cin)
    x = torch.randn((N, Cin, H, W), generator=g).half().float()
    w = (torch.randn((Cout, Cin, k, k), generator=g) / np.sqrt(Cin * k * k)).half().float()
    b = torch.randn((Cout,), generator=g).half().float()
    r = torch.randn((N, Cout, H, W), generator=g).half().float() if res else None
    ws = torch.empty((4096 + 64 * 4096 * 16,), dtype=torch.float32, device=DEV)
    ref = F.conv2d(x, w, b, padding=k // 2) + (r if res else 0)
    L.pdhip_debug_set_conv_splitk(_ptr(ws), ws.numel(), 0)
    old = L.pdhip_debug_set_conv_sk(2 if tile else 1, tile, splits)
    try:
        for kg in (0, 1, 2, 4, 8, 12):              # K-groups per workgroup (4-wave groups on alternate K-steps of one tile); 8 = loader-specialised, 12 = with eight loader waves
            L.pdhip_debug_set_conv_sk_kgroups(kg)
            y1 = hip_conv(nn, x, w, b, r)
            y2 = hip_conv(nn, x, w, b, r)
            err = (y1 - ref).abs().max().item() / ref.abs().max().item()
            assert err <= 2e-3, (kg, err)
            assert torch.equal(y1, y2), kg
    finally:
        L.pdhip_debug_set_conv_sk_kgroups(0)
        L.pdhip_debug_set_conv_sk(old, 0, 0)
        L.pdhip_debug_set_conv_splitk(None, 0, 0)


def _free_port():
    s = socket.socket(); s.bind(('127.0.0.1', 0)); p = s.getsockname()[1]; s.close()
    return p


def test_rccl_all_gather_views_world1(nn):
    """north_star's 'single RCCL all-gather': dist.all_gather_views on DEVICE uint8 records through backend 'nccl' (= RCCL),
    executed in-process at world size 1 -- the code path the 8-GPU run takes, un-patched."""
    import torch.distributed as dist
    from pointdreamer_amd import dist as pdd
    if dist.is_initialized():
        pytest.skip("a process group already exists in this process")
    os.environ.setdefault('MASTER_ADDR', '127.0.0.1')
    os.environ['MASTER_PORT'] = str(_free_port())
    dist.init_process_group('nccl', rank=0, world_size=1, device_id=torch.device(DEV))
    try:
        rec = torch.arange(3 * 1000, dtype=torch.int64, device=DEV).remainder(251).to(torch.uint8).view(3, 1000)
        out = pdd.all_gather_views(rec, 3, 0, 1, None, force_collective=True)
        torch.cuda.synchronize()
        assert out.is_cuda and out.dtype == torch.uint8 and out.data_ptr() != rec.data_ptr() and torch.equal(out, rec)
        # the whole view-parallel driver with the real HIP stages, its all_gather going through RCCL (one rank owns all views)
        from pointdreamer_amd import synthetic, pipeline
        import pointdreamer_amd.camera_utils as cu
        V, RES, CAM, A = 4, 256, 512, 512
        sh = synthetic.make_shape(8000, A, seed=5)
        T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
        gd = {k: T(v) for k, v in sh.items()}
        cams, base_dirs, eyes, ups = cu.create_cameras(V, 1.6, CAM, device=DEV)
        ci = dict(cams=cams, base_dirs=base_dirs, eye_positions=eyes, up_dirs=ups)
        xa = dict(gb_pos=gd['gb_pos'], mask=gd['mask'], per_atlas_pixel_face_id=gd['per_atlas_pixel_face_id'], uvs=None, mesh_tex_idx=None)
        cfg = dict(view_num=V, res=RES, cam_res=CAM, point_validation_by_o3d=True, texture_gen_method='nearest', point_size=1,
                   edge_point_size=1, crop_img=True, crop_padding=0.05, mask_ratio_thresh=0.82, optimize_from=None,
                   edge_dilate_kernels=[21], complete_unseen_by='unproject', inpainter=None)
        a_par = pdd.colorize_one_mesh_view_parallel(gd['points'], gd['colors'], gd['vertices'], gd['faces'], gd['f_normals'], xa, ci,
                                                    rank=0, world=1, force_collective=True, **cfg)
        a_one = pipeline.colorize_one_mesh(gd['points'], gd['colors'], gd['vertices'], gd['faces'], gd['f_normals'], xa, ci, **cfg)
        a_one = a_one[4]                                                       # (vertices, uvs, faces, mesh_tex_idx, atlas, mask)
        assert torch.equal(a_par, a_one)
    finally:
        dist.destroy_process_group()


def test_p2_raster_large_mesh_stays_on_tiled_path(nn):
    """A 39 600-face mesh at R = 512 (more faces than the V*R*R*8-byte z-key workspace holds setups for: 15.4 k): the wrappers size
    the workspace with pdhip_raster_mesh_ws_bytes so that the LDS-tiled path still runs; it must equal the global-atomic path bit
    for bit, and the historical entry point (which falls back for such a mesh) too."""
    from pointdreamer_amd import synthetic, extract_texture_map as etm
    import pointdreamer_amd.camera_utils as cu
    import pointdreamer_amd.ours_utils as ou
    L = nn['L']
    V, R = 3, 512
    verts, faces, _ = synthetic.uv_sphere(100, 200)
    assert faces.shape[0] > 30000 and L.pdhip_raster_mesh_ws_bytes(V, faces.shape[0], R) > V * R * R * 8
    xyz, _ = synthetic.sphere_points(2000, seed=3)
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    cams, _, _, _ = cu.create_cameras(V, 1.6, R, device=DEV)
    outs = []
    for path in (0, 1):
        old = L.pdhip_debug_set_raster_path(path)
        try:
            outs.append([t.cpu() for t in ou.get_rendered_hard_mask_and_face_idx_batch(cams, T(verts), T(faces), T(xyz), None, True, 0.05)[:3]])
        finally:
            L.pdhip_debug_set_raster_path(old)
    for a, b in zip(*outs):
        assert torch.equal(a, b)
    assert outs[0][0].any() and (outs[0][1] >= 0).sum() > 10000


def test_shape_graphs_replay_equals_eager(nn):
    """pipeline.ShapeGraphs: the 'nearest' path of a shape captured into HIP graphs (three slots on three streams); replays on fresh
    clouds -- fed in a different order than at capture -- give the eager colorize_one_mesh atlases bit for bit."""
    from pointdreamer_amd import synthetic, pipeline
    import pointdreamer_amd.camera_utils as cu
    V, RES, CAM, A, NP = 4, 128, 256, 256, 5000
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    sh = synthetic.make_shape(NP, A, seed=0)
    g = {k: T(v) for k, v in sh.items()}
    cams, base_dirs, eyes, ups = cu.create_cameras(V, 1.6, CAM, device=DEV)
    ci = dict(cams=cams, base_dirs=base_dirs, eye_positions=eyes, up_dirs=ups)
    xa = dict(gb_pos=g['gb_pos'], mask=g['mask'], per_atlas_pixel_face_id=g['per_atlas_pixel_face_id'], uvs=None, mesh_tex_idx=None)
    cfg = dict(point_validation_by_o3d=True, texture_gen_method='nearest', point_size=1, edge_point_size=1, crop_img=True,
               crop_padding=0.05, mask_ratio_thresh=0.82, optimize_from=None, edge_dilate_kernels=[21], complete_unseen_by='unproject')
    clouds = []
    for i in range(5):
        c = synthetic.make_shape(NP, A, seed=40 + i)
        clouds.append((T(c['points']), T(c['colors'])))
    eager = [pipeline.colorize_one_mesh(p, c, g['vertices'], g['faces'], g['f_normals'], xa, ci, view_num=V, res=RES, cam_res=CAM,
                                        inpainter=None, **cfg)[4].clone() for p, c in clouds]
    sg = pipeline.ShapeGraphs(3, NP, g['vertices'], g['faces'], g['f_normals'], xa, ci, V, RES, CAM, **cfg)
    got = sg.run(clouds[:3]) + sg.run(clouds[3:]) + sg.run([clouds[4], clouds[0]])
    torch.cuda.synchronize()
    for a, b in zip(got, eager + [eager[4], eager[0]]):
        assert torch.equal(a, b)
    with pytest.raises(ValueError):
        pipeline.ShapeGraphs(1, NP, g['vertices'], g['faces'], g['f_normals'], xa, ci, V, RES, CAM, **dict(cfg, optimize_from='ours'))
    with pytest.raises(ValueError):
        sg.run([(clouds[0][0][:100], clouds[0][1][:100])])


@pytest.mark.parametrize("film", [False, True])
def test_groupnorm_apply_is_independent_of_pixels_per_thread(nn, film):
    """k_gn_apply picks its pixels-per-thread from the launch size, so the same image goes through the 4-pixel main loop at batch 8 and
    through the 1-pixel tail loop at batch 1: the bits must not depend on that (they did, by one f16 ulp in 4e-5 of the elements,
    while the compiler was free to fuse an op with the f16 rounding behind it in one copy of the loop and not in the other)."""
    L = nn['L']
    H = W = 128; Cc = 256
    g = torch.Generator().manual_seed(3)
    x1 = (torch.randn((1, H, W, Cc), generator=g) * 1.3 + 0.2).half()
    gamma = (1 + 0.2 * torch.randn((Cc,), generator=g)).to(DEV); beta = (0.2 * torch.randn((Cc,), generator=g)).to(DEV)
    fl1 = 0.3 * torch.randn((1, 2 * Cc), generator=g)
    outs = []
    for N in (1, 8):
        xd = x1.repeat(N, 1, 1, 1).contiguous().to(DEV)
        fd = fl1.repeat(N, 1).contiguous().to(DEV) if film else None
        y = torch.empty_like(xd)
        stats = torch.empty((N * 64,), device=DEV); ws = torch.empty((N * 64 * ((H * W + 255) // 256),), device=DEV)
        rc = L.pdhip_groupnorm_nhwc_f16(_ptr(xd), _ptr(gamma), _ptr(beta), _ptr(fd) if film else None, N, H, W, Cc, 1, 0, _ptr(y), _ptr(stats),
                                        _ptr(ws), ws.numel(), _stream())
        assert rc == 0, L.pdhip_last_error()
        torch.cuda.synchronize()
        outs.append(y.cpu())
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[1][0], outs[1][7])


@pytest.mark.parametrize("N,H,W,Ca,Cb", [(2, 16, 16, 256, 256), (1, 32, 16, 512, 256), (3, 8, 16, 512, 0), (1, 64, 64, 256, 256),
                                          (1, 256, 256, 256, 256), (2, 128, 128, 512, 256)])     # the last two: the UNet's own decoder shapes
def test_gn_skip_one_pass_equals_two_launches(nn, N, H, W, Ca, Cb):
    """k_gn_skip (in_layers GroupNorm -> SiLU and the skip 1x1 of a channel-changing ResBlock in one pass over the never-materialised
    concat, unet.py:197-209 / 236-256 / 657-659): h0 must equal the stand-alone GroupNorm-apply kernel bit for bit on the same
    statistics, the skip output must equal the engine's own 1x1 conv within f16 rounding of the f32 accumulation order and torch fp32
    within the single-kernel tolerance."""
    L = nn['L']
    Cc = Ca + Cb
    g = torch.Generator().manual_seed(Ca + 7 * Cb + H)
    x = (torch.randn((N, H, W, Cc), generator=g) * 1.4 + 0.25).half()
    gamma = (1 + 0.2 * torch.randn((Cc,), generator=g)).to(DEV); beta = (0.2 * torch.randn((Cc,), generator=g)).to(DEV)
    w = (torch.randn((256, Cc, 1, 1), generator=g) / math.sqrt(Cc)).half().float()
    b = (0.1 * torch.randn((256,), generator=g)).to(DEV)
    xd = x.to(DEV)
    xa = xd[..., :Ca].contiguous(); xb = xd[..., Ca:].contiguous() if Cb else None
    # two-launch form on the materialised concat
    y_ref = torch.empty_like(xd)
    stats = torch.empty((N * 64,), device=DEV); ws = torch.empty((N * 64 * ((H * W + 255) // 256),), device=DEV)
    assert L.pdhip_groupnorm_nhwc_f16(_ptr(xd), _ptr(gamma), _ptr(beta), None, N, H, W, Cc, 1, 0, _ptr(y_ref), _ptr(stats), _ptr(ws),
                                      ws.numel(), _stream()) == 0, L.pdhip_last_error()
    wp = torch.zeros((256, Cc), dtype=torch.float16, device=DEV)
    wd = w.contiguous().to(DEV)
    assert L.pdhip_pack_conv_weight_f16(_ptr(wd), 256, Cc, 1, _ptr(wp), _stream()) == 0
    zp = torch.zeros((128,), dtype=torch.float16, device=DEV)
    sk_ref = torch.empty((N, H, W, 256), dtype=torch.float16, device=DEV)
    assert L.pdhip_conv2d_nhwc_f16(_ptr(xd), _ptr(wp), _ptr(b), None, _ptr(sk_ref), N, H, W, Cc, 256, 256, 1, _ptr(zp), _stream()) == 0
    # one pass, both launch forms of the kernel
    t_ref = F.conv2d(x.float().permute(0, 3, 1, 2), w, b.cpu()).permute(0, 2, 3, 1)
    scale = t_ref.abs().max().item()
    sks = []
    for variant in (1, 2):                               # (1: 64-pixel tiles where 128-pixel tiles would not fill the chip -- round 4; 2: 128 always)
        old = L.pdhip_debug_set_gn_skip_variant(variant)
        try:
            h0 = torch.full_like(xd, float('nan')); sk = torch.full_like(sk_ref, float('nan'))
            rc = L.pdhip_gn_silu_skip1x1_nhwc_f16(_ptr(xa), _ptr(xb) if Cb else None, Ca, Cc, _ptr(stats), _ptr(gamma), _ptr(beta), _ptr(wp),
                                                  _ptr(b), _ptr(h0), _ptr(sk), N, H, W, _stream())
            assert rc == 0, L.pdhip_last_error()
            torch.cuda.synchronize()
        finally:
            L.pdhip_debug_set_gn_skip_variant(old)
        assert torch.equal(h0, y_ref), variant
        assert (sk.float().cpu() - t_ref).abs().max().item() <= 2e-3 * scale + 1e-3
        assert (sk.float() - sk_ref.float()).abs().max().item() <= 2e-3 * scale          # (one f16 ulp at most: same products, f32 sums)
        sks.append(sk)
    assert torch.equal(sks[0], sks[1])                                     # same K order, same fragments: the forms agree bit for bit
    # shapes the kernel does not serve are refused, not mis-computed
    assert L.pdhip_gn_silu_skip1x1_nhwc_f16(_ptr(xa), _ptr(xb) if Cb else None, Ca, Cc, _ptr(stats), _ptr(gamma), _ptr(beta), _ptr(wp), _ptr(b),
                                            _ptr(h0), _ptr(sk), N, 1, 127, _stream()) != 0      # (H * W not a multiple of the 128-pixel tile)


def test_unet_full_256_fused_skip_equals_two_launch_routing(nn):
    """The full 552.8 M UNet with the one-pass GroupNorm + skip kernel forced on for every eligible ResBlock against the two-launch
    routing, batch 2: same activations up to the f32 summation order of the skip GEMM (h0 is bit-identical), so the outputs agree
    far inside the U1 tolerance."""
    di, L = nn['di'], nn['L']
    cfg = ounet.make_config(256, 256, 2, "32,16,8", 64, True)
    w = ounet.random_weights(cfg, 11)
    m = di.UNetModel(max_batch=2, device=DEV, **di.IMAGENET_256)
    m.load_state_dict(w, strict=True)
    del w
    g = torch.Generator().manual_seed(5)
    x = torch.randn((2, 3, 256, 256), generator=g).to(DEV); t = torch.tensor([37.0, 801.0], device=DEV)
    outs = []
    for mode in (0, 2):
        old = L.pdhip_debug_set_fuse_skip(mode, 0)
        try:
            outs.append(m(x, t).float().cpu())
        finally:
            L.pdhip_debug_set_fuse_skip(old, 0)
    d = (outs[0] - outs[1]).abs().max().item()
    assert d <= 2e-3 * outs[0].abs().max().item(), d
    assert d > 0 or torch.equal(outs[0], outs[1])


def test_refine_point_validation_vs_oracle(nn):
    """ours_utils.refine_point_validation (ours_utils.py:227-305): pixel arithmetic, mask resize and the nearest fill on the device,
    the blob test on the host -- against the oracle's literal composition (oracle/refine.py with the oracle's P2b / I0 functions).
    The scene: a smooth depth field seen from two cameras, with clusters of 'see-through' points 0.45 farther than their
    neighbourhood; those, and only points on such regions, lose their visibility."""
    import pointdreamer_amd.ours_utils as ou
    from oracle import refine as oref, project as oproj, inpaint as oinp
    V, N, res, hres = 2, 6000, 128, 64
    rng = np.random.default_rng(11)
    uv = rng.uniform(0.12, 0.88, (V, N, 2)).astype(np.float32)
    yy, xx = np.mgrid[0:hres, 0:hres]
    hard = np.stack([((yy - hres / 2) ** 2 + (xx - hres / 2) ** 2) < (0.47 * hres) ** 2] * V)
    # camera 0 reads z, camera 1 reads 1.6 - x; the points are built so that both depth fields are smooth in the view's own uv
    RT = np.zeros((V, 3, 4)); RT[0, 2] = [0, 0, 1, 0]; RT[1, 2] = [-1, 0, 0, 1.6]
    pts = np.zeros((N, 3), np.float32)
    pts[:, 2] = 1.0 + 0.25 * uv[0, :, 0] + 0.02 * np.sin(7 * uv[0, :, 1])
    pts[:, 0] = 1.6 - (1.2 + 0.2 * uv[1, :, 1])
    planted = np.zeros((V, N), bool)
    for v, centres in enumerate([[(0.3, 0.3), (0.6, 0.55), (0.45, 0.7)], [(0.35, 0.6), (0.65, 0.35)]]):
        for cx, cy in centres:
            sel = ((uv[v, :, 0] - cx) ** 2 + (uv[v, :, 1] - cy) ** 2) < 0.045 ** 2
            planted[v] |= sel
    pts[planted[0], 2] += 0.45
    pts[planted[1] & ~planted[0], 0] -= 0.45
    valid = rng.uniform(size=(V, N)) < 0.9
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    got = ou.refine_point_validation(RT, None, res, T(hard), T(valid), T(uv), T(pts), None).cpu().numpy()
    want = oref.refine_point_validation(RT, res, hard, valid, uv, pts, oproj.resize_mask_bilinear_nonzero, oinp.nearest_inpaint)
    assert np.array_equal(got, want)
    removed = valid & ~got
    assert removed.any() and not (got & ~valid).any()                   # visibility is only ever taken away
    assert removed[0].sum() > 20 and (removed[0] & planted[0]).sum() >= 0.8 * removed[0].sum()      # what goes is what was planted
    assert (valid[0] & planted[0] & ~removed[0]).sum() <= 0.5 * (valid[0] & planted[0]).sum()


def test_colorize_one_mesh_with_refine_option(nn, tmp_path):
    """`refine_point_validation_by_remove_abnormal_depth=True` (demo.py:115-117) runs through the pipeline: cam_RTs derived from the eye
    positions (demo.py:334-335), `{i}_depth.png` panels written, an atlas comes out; with nothing abnormal in the cloud the atlas
    equals the one without the option."""
    from pointdreamer_amd import synthetic, pipeline
    import pointdreamer_amd.camera_utils as cu
    V, RES, CAM, A, NP = 3, 128, 256, 256, 5000
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    g = {k: T(v) for k, v in synthetic.make_shape(NP, A, seed=3).items()}
    cams, base_dirs, eyes, ups = cu.create_cameras(V, 1.6, CAM, device=DEV)
    ci = dict(cams=cams, base_dirs=base_dirs, eye_positions=eyes, up_dirs=ups)
    xa = dict(gb_pos=g['gb_pos'], mask=g['mask'], per_atlas_pixel_face_id=g['per_atlas_pixel_face_id'], uvs=None, mesh_tex_idx=None)
    cfg = dict(point_validation_by_o3d=True, texture_gen_method='nearest', point_size=1, edge_point_size=1, crop_img=True,
               crop_padding=0.05, mask_ratio_thresh=0.82, optimize_from=None, edge_dilate_kernels=[21], complete_unseen_by='unproject')
    outs = {}
    for on in (False, True):
        d = str(tmp_path / f"o{int(on)}")
        outs[on] = pipeline.colorize_one_mesh(g['points'], g['colors'], g['vertices'], g['faces'], g['f_normals'], xa, ci, view_num=V, res=RES,
                                              cam_res=CAM, inpainter=None, save_img_path=d, return_intermediates=True,
                                              refine_point_validation_by_remove_abnormal_depth=on, refine_res=256, **cfg)
    from pointdreamer_amd import io_utils
    io_utils.flush()
    for i in range(V):
        assert os.path.exists(str(tmp_path / "o1" / f"{i}_depth.png")) and not os.path.exists(str(tmp_path / "o0" / f"{i}_depth.png"))
    pv0, pv1 = outs[False]['point_validation'], outs[True]['point_validation']
    assert not (pv1 & ~pv0).any()                                      # refinement only removes
    assert (pv0 & ~pv1).float().mean().item() < 0.02                   # a clean sphere: (almost) nothing to remove
    if torch.equal(pv0, pv1):
        assert torch.equal(outs[False]['atlas'], outs[True]['atlas'])


def test_optimize_color_is_deterministic_and_leaves_unsampled_texels(nn):
    """optimize_color (ours_utils.py:1583-1785) on compact lists: the CSR entries are sorted inside a texel and every sum runs in list
    order, so two runs on the same inputs agree bit for bit (the reference's grid_sample backward uses atomics and does not); texels
    no masked pixel samples are never touched; the final render is zero outside the mask."""
    from pointdreamer_amd import synthetic, optimize as popt
    import pointdreamer_amd.camera_utils as cu
    from pointdreamer_amd.demo import standin_geometry
    import logging
    V, CAM, A, res, r = 3, 256, 256, 192, 64
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    xyz, _ = synthetic.sphere_points(2000, seed=2)
    vv, ff, xd = standin_geometry(T(xyz), A, torch.device(DEV), logging.getLogger('t'))
    cams, _, _, _ = cu.create_cameras(V, 1.6, CAM, device=DEV)
    g = torch.Generator().manual_seed(9)
    atlas0 = torch.rand((3, A, A), generator=g).to(DEV)
    inp = torch.rand((V, 3, r, r), generator=g).to(DEV)
    shr = (torch.rand((V, A, A), generator=g) > 0.25).to(DEV)
    uvc = torch.zeros((V, 1, 2), device=DEV); uvs = torch.full((V, 1, 1), 1.1, device=DEV); sf = torch.ones((V,), device=DEV)
    runs = []
    for _ in range(2):
        popt._DEBUG_COUNTS = [0, 0, 0, 0]
        a, im = popt.optimize_color(atlas0, inp, vv, ff, xd['uvs'], xd['mesh_tex_idx'], cams, None, None, None, uvc, uvs, 0.05, sf, None, shr,
                                    iterations=12, res=res)
        counts = list(popt._DEBUG_COUNTS); popt._DEBUG_COUNTS = None
        runs.append((a.clone(), im.clone()))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    masked, active, pixels, texels = counts
    assert 0 < masked < pixels and 0 < active <= texels
    moved = (runs[0][0][0] != atlas0).any(0)
    assert 0 < int(moved.sum()) <= active                       # only texels that receive a contribution can move
    assert int((runs[0][1] != 0).any(1).sum()) <= masked        # the render is zero outside the masked pixels
    assert runs[0][1].min() >= 0 and runs[0][1].max() <= 1
