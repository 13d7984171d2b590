"""Times of the evaluation renderer's shading stage and of the image metrics on one MI355X -> profiles/render_bench.txt.

  python tools/bench_render.py     # 20 'self_defined' views at 512^2 of a 9 680-face sphere (icosphere 22), atlas 1024^2
                                   #   fused     : pdhip_shade_views (csrc/render.hip), images [V,3,R,R] f32
                                   #   composed  : what the parent commit offers -- pdhip_interpolate (uv_map [V,R,R,2] in HBM) +
                                   #               torch.nn.functional.grid_sample on the device + mask + flip + permute
                                   #   metrics   : pdhip_image_metrics on 20 x 512^2 x 3 (SSE + SSIM, both definitions; SSE alone)
HIP events round CALLS calls in a row (one call is tens of microseconds), WARMUP warm-up windows, median and range of REPEAT windows,
the two renderers alternating inside one process.  The raster (shared by both) is outside the timed window.  A run without a GPU fails."""
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from pointdreamer_amd import synthetic, metric_utils      # noqa: E402
import pointdreamer_amd.camera_utils as cu      # noqa: E402
from pointdreamer_amd.extract_texture_map import rasterize, interpolate      # noqa: E402

OUT = os.path.join(ROOT, 'profiles', 'render_bench.txt')
V, R, A, N_ICO = 20, 512, 1024, 22
WARMUP, REPEAT, CALLS = 3, 15, 20


def window(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(CALLS):
        r = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / CALLS, r


def composed(uvs, fidx, bary, faces, atlas_nchw):
    """The parent commit's pieces: uv_map through HBM, grid_sample (v looked up at y = v*A - 0.5: atlas row 0 is v = 0), background, flip."""
    uv = interpolate(uvs, fidx, bary, faces)
    g = (uv - torch.floor(uv)) * 2.0 - 1.0
    img = torch.nn.functional.grid_sample(atlas_nchw.expand(uv.shape[0], -1, -1, -1), g, mode='bilinear', align_corners=False,
                                          padding_mode='border')
    return (img * (fidx >= 0).unsqueeze(1)).flip(2)


def main():
    assert torch.cuda.is_available(), "bench_render.py measures on the GPU; there is no CPU path"
    dev = 'cuda:0'
    verts, faces = synthetic.icosphere(N_ICO)
    rng = np.random.default_rng(0)
    T = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    verts, faces = T(verts), T(faces)
    uvs = T(rng.uniform(0.02, 0.98, size=(verts.shape[0], 2)).astype(np.float32))
    atlas = T(rng.uniform(0, 1, size=(A, A, 3)).astype(np.float32))
    atlas_nchw = atlas.permute(2, 0, 1)[None].contiguous()
    cams, _, _, _ = cu.create_cameras(V, 1.6, R, distribution='self_defined', device=dev)
    pos, cp = cu._clip_positions(cams, verts)
    fidx, bary, _, _ = rasterize(pos, faces, R)
    faces32 = faces.to(torch.int32)
    fused = lambda: cu.shade_views(fidx, bary, uvs, faces32, atlas=atlas)[0]
    comp = lambda: composed(uvs, fidx, bary, faces32, atlas_nchw)
    fused_rgba = lambda: cu.shade_views(fidx, bary, uvs, faces32, atlas=atlas, want_images=False, want_rgba=True)[1]
    fn = cu.face_normals_unit(verts, faces)
    lights = T(np.array([[0.8, 0, 0], [0.0, 0.5, 0.0], [0.0, 0.0, -0.5]], np.float32))
    fused_lit = lambda: cu.shade_views(fidx, bary, uvs, faces32, atlas=atlas, face_normals=fn, cam_params=cp, light_dirs=lights, gamma=2.2)[0]
    diff = (fused() - comp()).abs().max().item()
    covered = (fidx >= 0).float().mean().item()
    tf, tc, tr, tl = [], [], [], []
    for it in range(WARMUP + REPEAT):
        a, _ = window(fused)
        b, _ = window(comp)
        c, _ = window(fused_rgba)
        d, _ = window(fused_lit)
        if it >= WARMUP:
            tf.append(a); tc.append(b); tr.append(c); tl.append(d)
    med = statistics.median
    px = V * R * R
    gbs = lambda ms, bytes_px: px * bytes_px / (ms * 1e-3) / 1e9
    L = [f"Shading stage of the evaluation renderer on one MI355X (tools/bench_render.py): {V} 'self_defined' views at {R}^2, sphere of "
         f"{faces.shape[0]} faces,", f"atlas {A}^2, {covered * 100:.1f} % of the pixels covered.  HIP events round {CALLS} calls, {WARMUP} warm-up windows, "
         f"median [min .. max] of {REPEAT} windows, the variants", "alternating in one process; ms per call of all 20 views (python wrapper included).  "
         "GB/s: compulsory bytes only (face_idx 8 + bary 8 + output), atlas gathers not counted.", "",
         f"fused, images f32      (pdhip_shade_views)                        {med(tf):8.4f} ms [{min(tf):.4f} .. {max(tf):.4f}]   {gbs(med(tf), 28):7.0f} GB/s",
         f"fused, rgba u8 only                                               {med(tr):8.4f} ms [{min(tr):.4f} .. {max(tr):.4f}]   {gbs(med(tr), 20):7.0f} GB/s",
         f"fused, images f32, 3 lights + gamma 2.2                           {med(tl):8.4f} ms [{min(tl):.4f} .. {max(tl):.4f}]",
         f"composed (pdhip_interpolate + grid_sample + mask + flip)          {med(tc):8.4f} ms [{min(tc):.4f} .. {max(tc):.4f}]",
         f"composed / fused                                                  {med(tc) / med(tf):8.2f} x",
         f"largest |fused - composed| over the images                        {diff:.3e}", ""]
    for l in L:
        print(l, flush=True)
    g = torch.Generator(device='cpu').manual_seed(1)
    a8 = torch.randint(0, 256, (V, R, R, 3), dtype=torch.uint8, generator=g).to(dev)
    b8 = (a8.int() + torch.randint(-20, 21, a8.shape, generator=g).to(dev)).clamp(0, 255).to(torch.uint8)
    M = [f"Image metrics on {V} x {R}^2 x 3 u8 (pdhip_image_metrics + its finalize launch, workspace allocation and python wrapper included; no host read):"]
    for tag, f in (("SSE + SSIM, 7x7 uniform window (use_sk=True)", lambda: metric_utils.image_metrics(a8, b8, True)),
                   ("SSE + SSIM, 11x11 Gaussian window (use_sk=False)", lambda: metric_utils.image_metrics(a8, b8, False)),
                   ("SSE alone (PSNR)", lambda: metric_utils.image_metrics(a8, b8, True, want_ssim=False))):
        ts = []
        for it in range(WARMUP + REPEAT):
            t, _ = window(f)
            if it >= WARMUP:
                ts.append(t)
        M.append(f"{tag:66s}{med(ts):8.4f} ms [{min(ts):.4f} .. {max(ts):.4f}]   {2 * V * R * R * 3 / (med(ts) * 1e-3) / 1e9:7.0f} GB/s of input")
        print(M[-1], flush=True)
    open(OUT, 'w').write('\n'.join(L + M) + '\n')


if __name__ == '__main__':
    main()
