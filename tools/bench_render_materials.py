"""Times of the multi-material shading kernel on one MI355X -> profiles/render_materials_bench.txt.

  python tools/bench_render_materials.py
        # 20 'self_defined' views at 512^2 of a 9 680-face sphere (icosphere 22); three materials assigned f % 3: two 1024 x 512 u8
        # images and one Kd colour
        #   (a) materials : pdhip_shade_views_materials (csrc/render.hip), images [V,3,R,R] f32
        #   (b) one atlas : pdhip_shade_views on the same face_idxs / bary with one 1024^2 f32 atlas
        #   (c) composed  : what the parent commit allows -- pdhip_interpolate (uv_map [V,R,R,2] in HBM) + one masked
        #                   torch.nn.functional.grid_sample per material per view (the reference's loop, camera_utils.py:468-480)
The method of tools/bench_render.py: HIP events round CALLS calls in a row, WARMUP warm-up windows, median and range of REPEAT windows,
the candidates alternating inside one process, the raster (shared by all) outside the timed window.  A run without a GPU fails."""
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from pointdreamer_amd import synthetic      # noqa: E402
import pointdreamer_amd.camera_utils as cu      # noqa: E402
from pointdreamer_amd.extract_texture_map import rasterize, interpolate      # noqa: E402
from pointdreamer_amd.sample_colored_pc_from_mesh import pack_materials      # noqa: E402

OUT = os.path.join(ROOT, 'profiles', 'render_materials_bench.txt')
V, R, A, N_ICO, W, H = 20, 512, 1024, 22, 1024, 512
WARMUP, REPEAT, CALLS, CALLS_COMPOSED = 3, 15, 20, 2


def window(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        r = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / calls, r


def composed(uvs, fidx, bary, faces32, face_material, mats_nchw):
    """The reference's loop on the parent commit's pieces: uv_map through HBM, then per view and per material a mask, a gather, a
    grid_sample (v negated: the images are stored row 0 at the top) and a scatter; background 0, flip, permute."""
    uv = interpolate(uvs, fidx, bary, faces32)                                   # [V,R,R,2]
    mat = torch.where(fidx >= 0, face_material[fidx.clamp_min(0)], torch.full_like(fidx, -1, dtype=torch.int32))
    out = torch.zeros(fidx.shape + (3,), device=fidx.device)
    for v in range(fidx.shape[0]):
        for m, img in enumerate(mats_nchw):
            sel = mat[v] == m
            g = (uv[v][sel] % 1) * 2.0 - 1.0
            g[:, 1] = -g[:, 1]
            val = torch.nn.functional.grid_sample(img, g.reshape(1, 1, -1, 2), mode='bilinear', align_corners=False, padding_mode='border')
            out[v][sel] = val[0, :, 0].permute(1, 0)
    return out.flip(1).permute(0, 3, 1, 2)


def main():
    assert torch.cuda.is_available(), "bench_render_materials.py measures on the GPU; there is no CPU path"
    dev = 'cuda:0'
    verts, faces = synthetic.icosphere(N_ICO)
    rng = np.random.default_rng(0)
    T = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    verts, faces = T(verts), T(faces)
    F = faces.shape[0]
    uvs = T(rng.uniform(0.02, 0.98, size=(verts.shape[0], 2)).astype(np.float32))
    atlas = T(rng.uniform(0, 1, size=(A, A, 3)).astype(np.float32))
    materials = [{'name': 'a', 'map_Kd': rng.integers(0, 256, size=(H, W, 3), dtype=np.uint8)},
                 {'name': 'b', 'map_Kd': rng.integers(0, 256, size=(H, W, 3), dtype=np.uint8)},
                 {'name': 'c', 'Kd': np.array([0.2, 0.55, 0.9], np.float32)}]
    packed = pack_materials(materials, dev)
    face_material = (torch.arange(F, device=dev) % 3).to(torch.int32)
    mats_nchw = [T(m['map_Kd']).permute(2, 0, 1)[None].float() / 255. if 'map_Kd' in m else T(m['Kd']).reshape(1, 3, 1, 1) for m in materials]
    cams, _, _, _ = cu.create_cameras(V, 1.6, R, distribution='self_defined', device=dev)
    pos, cp = cu._clip_positions(cams, verts)
    fidx, bary, _, _ = rasterize(pos, faces, R)
    faces32 = faces.to(torch.int32)
    fa = lambda: cu.shade_views_materials(fidx, bary, uvs, faces, face_material, packed)[0]
    fb = lambda: cu.shade_views(fidx, bary, uvs, faces32, atlas=atlas)[0]
    fc = lambda: composed(uvs, fidx, bary, faces32, face_material, mats_nchw)
    fa_rgba = lambda: cu.shade_views_materials(fidx, bary, uvs, faces, face_material, packed, want_images=False, want_rgba=True)[1]
    diff = (fa() - fc()).abs().max().item()
    covered = (fidx >= 0).float().mean().item()
    ta, tb, tc, tr = [], [], [], []
    for it in range(WARMUP + REPEAT):
        a, _ = window(fa, CALLS)
        b, _ = window(fb, CALLS)
        c, _ = window(fc, CALLS_COMPOSED)
        d, _ = window(fa_rgba, CALLS)
        if it >= WARMUP:
            ta.append(a); tb.append(b); tc.append(c); tr.append(d)
    med = statistics.median
    row = lambda tag, t: f"{tag:68s}{med(t):9.4f} ms [{min(t):.4f} .. {max(t):.4f}]"
    L = [f"Multi-material shading on one MI355X (tools/bench_render_materials.py): {V} 'self_defined' views at {R}^2, sphere of {F} faces, "
         f"{covered * 100:.1f} % of the", f"pixels covered; materials f % 3: two {W} x {H} u8 images and one Kd.  HIP events round {CALLS} calls "
         f"({CALLS_COMPOSED} for the composed loop), {WARMUP} warm-up windows,", f"median [min .. max] of {REPEAT} windows, the candidates alternating "
         "in one process; ms per call of all 20 views (python wrapper included).", "",
         row("(a) materials, images f32   (pdhip_shade_views_materials)", ta),
         row("    materials, rgba u8 only", tr),
         row(f"(b) one atlas {A}^2 f32, images f32   (pdhip_shade_views)", tb),
         row("(c) composed (pdhip_interpolate + a masked grid_sample per material per view)", tc),
         f"(a) / (b)                                                           {med(ta) / med(tb):9.3f} x     (expected <= 1.25)",
         f"(c) / (a)                                                           {med(tc) / med(ta):9.1f} x",
         f"largest |(a) - (c)| over the images                                 {diff:.3e}", ""]
    for l in L:
        print(l, flush=True)
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    open(OUT, 'w').write('\n'.join(L))


if __name__ == '__main__':
    main()
