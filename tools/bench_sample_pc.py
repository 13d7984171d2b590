"""Times of the mesh sampler on one MI355X -> profiles/sample_pc_bench.txt.

  python tools/bench_sample_pc.py  # 150 000 samples (5 x 30 000) of seeded spheres of 9 680 faces (icosphere 22) and 200 000 faces
                                   # (icosphere 100), four materials: three 1024 x 512 images and one Kd colour
                                   #   kernel    : pdhip_sample_mesh (csrc/sample_mesh.hip) through sample_points
                                   #   composed  : what the parent commit offers -- torch.multinomial over f32 areas on the device,
                                   #               gathers, the fold, one grid_sample per material (the reference's loop)
                                   #   whole     : sample_one_mesh_w_o_invisible_points, 30 000 points, 20 views at 256^2, no files
HIP events round CALLS calls in a row, WARMUP warm-up windows, median and range of REPEAT windows, the two versions alternating inside
one process.  Equivalence at the timed size: both versions get the same uniforms (the composed one through an inverse CDF of its f64
cumulative areas instead of multinomial); the share of samples on the same face and the largest colour difference on those are recorded.
A run without a GPU fails."""
import math
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
from pointdreamer_amd import sample_colored_pc_from_mesh as sm      # noqa: E402

OUT = os.path.join(ROOT, 'profiles', 'sample_pc_bench.txt')
N, TEX_W, TEX_H = 150000, 1024, 512
WARMUP, REPEAT, CALLS = 2, 9, 10


def window(fn, calls=CALLS):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        r = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / calls, r


def composed(verts, faces, uvs, ft, fm, mats_nchw, rand, inverse_cdf=False):
    """The parent commit's pieces (sample_colored_pc_from_mesh.py:132-184 with torch in kaolin's place)."""
    fv = verts[faces]
    n = torch.cross(fv[:, 1] - fv[:, 0], fv[:, 2] - fv[:, 0], dim=1)
    areas = 0.5 * n.norm(dim=1)
    if inverse_cdf:
        cdf = torch.cumsum(areas.double(), 0)
        face = torch.searchsorted(cdf, rand[:, 0].double() * cdf[-1], right=True).clamp_max(faces.shape[0] - 1)
    else:
        face = torch.multinomial(areas, rand.shape[0], replacement=True)
    u, v = rand[:, 1:2], rand[:, 2:3]
    over = (u + v) > 1
    u, v = torch.where(over, 1 - u, u), torch.where(over, 1 - v, v)
    p = fv[face]
    coords = (p[:, 0] + u * (p[:, 1] - p[:, 0])) + v * (p[:, 2] - p[:, 0])
    q = uvs[ft[face]]
    uv = (q[:, 0] + u * (q[:, 1] - q[:, 0])) + v * (q[:, 2] - q[:, 0])
    mat = fm[face]
    colors = torch.zeros((rand.shape[0], 3), device=rand.device)
    g = (uv % 1) * 2 - 1
    g = torch.stack([g[:, 0], -g[:, 1]], 1)
    for i, m in enumerate(mats_nchw):
        mask = mat == i
        c = torch.nn.functional.grid_sample(m, g[mask].reshape(1, 1, -1, 2), mode='bilinear', align_corners=False, padding_mode='border')
        colors[mask] = c[0, :, 0, :].permute(1, 0)
    normals = (n / n.norm(dim=1, keepdim=True).clamp_min(1e-30))[face]
    return dict(coords=coords, face_idx=face, material_idx=mat, uvs=uv, colors=colors, normals=normals)


def main():
    assert torch.cuda.is_available(), "bench_sample_pc.py measures on the GPU; there is no CPU path"
    dev = 'cuda:0'
    T = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    rng = np.random.default_rng(0)
    materials = [{'map_Kd': rng.integers(0, 256, (TEX_H, TEX_W, 3), dtype=np.uint8)} for _ in range(3)] + [{'Kd': np.array([0.3, 0.6, 0.9], np.float32)}]
    packed = sm.pack_materials(materials, dev)
    mats_nchw = [T(m['map_Kd']).permute(2, 0, 1)[None].float() / 255. if 'map_Kd' in m else T(m['Kd']).reshape(1, 3, 1, 1) for m in materials]
    rand = torch.rand((N, 3), generator=torch.Generator().manual_seed(1)).to(dev)
    med = statistics.median
    L = [f"Mesh sampler on one MI355X (tools/bench_sample_pc.py): {N} samples, four materials (three {TEX_W} x {TEX_H} images, one Kd).  HIP events "
         f"round {CALLS} calls,", f"{WARMUP} warm-up windows, median [min .. max] of {REPEAT} windows, the versions alternating in one process; ms per call "
         "(python wrapper, workspace allocation and the call's one", "host read included).  Bytes the algorithm must move per sample: 12 of uniforms in, "
         "52 out (coords, colors, normals 12 each, uvs 8, two indices 4 each), and as", "gathers a face row 24, three vertices 36, three uv indices 24, "
         "three uvs 24, a material index 4, four texels 12, and 8 per step of the binary search", "over the uint64 CDF (ceil(log2 F) steps).  "
         "No coarse LDS table over the CDF: not tried, so not claimed.", ""]
    for n_ico in (22, 100):
        verts, faces = synthetic.icosphere(n_ico, noise=0.01, seed=1)
        F = faces.shape[0]
        uvs = rng.uniform(-0.5, 1.5, size=(verts.shape[0], 2)).astype(np.float32)
        fm = rng.integers(0, 4, F).astype(np.int32)
        verts, faces, uvs, fm = T(verts), T(faces), T(uvs), T(fm)
        fm64 = fm.long()
        kern = lambda: sm.sample_points(verts, faces, uvs, faces, fm, packed, N, rand=rand)
        comp = lambda: composed(verts, faces, uvs, faces, fm64, mats_nchw, rand)
        a, b = kern(), composed(verts, faces, uvs, faces, fm64, mats_nchw, rand, inverse_cdf=True)
        same = a['face_idx'].long() == b['face_idx']
        cdiff = (a['colors'] - b['colors'])[same].abs().max().item()
        pdiff = (a['coords'] - b['coords'])[same].abs().max().item()
        tk, tc = [], []
        for it in range(WARMUP + REPEAT):
            x, _ = window(kern)
            y, _ = window(comp)
            if it >= WARMUP:
                tk.append(x); tc.append(y)
        steps = math.ceil(math.log2(F))
        per = 64 + 124 + 8 * steps
        L += [f"sphere of {F} faces (icosphere {n_ico}), CDF {F * 8 / 1e6:.2f} MB, {per} B per sample ({per * N / 1e6:.1f} MB per call)",
              f"  pdhip_sample_mesh (area, weight, scan, draw: 6 launches)        {med(tk):8.4f} ms [{min(tk):.4f} .. {max(tk):.4f}]   "
              f"{per * N / (med(tk) * 1e-3) / 1e9:7.1f} GB/s",
              f"  composed (multinomial + gathers + 4 grid_sample)                {med(tc):8.4f} ms [{min(tc):.4f} .. {max(tc):.4f}]",
              f"  composed / kernel                                               {med(tc) / med(tk):8.2f} x",
              f"  same uniforms through an inverse CDF: same face {same.float().mean().item() * 100:.3f} % of the samples; on those, largest "
              f"|colour difference| {cdiff:.3e}, largest |position difference| {pdiff:.3e}", ""]
        for l in L[-6:]:
            print(l, flush=True)
        if n_ico == 22:
            md = sm.MeshData(verts, faces, uvs, faces, fm, packed, name='bench/sphere')
            cams, _, _, _ = cu.create_cameras(num_views=20, distance=1.6, res=256, device=dev)
            gen = torch.Generator().manual_seed(2)
            whole = lambda: sm.sample_one_mesh_w_o_invisible_points(md, 30000, cams, dev, None, generator=gen)
            tw = []
            for it in range(WARMUP + REPEAT):
                t, _ = window(whole, calls=1)
                if it >= WARMUP:
                    tw.append(t)
            L += [f"  sample_one_mesh_w_o_invisible_points, 30 000 points, 20 views at 256^2 (draw, project, raster, depth test, subset, copy to "
                  f"the host; no files)   {med(tw):8.3f} ms [{min(tw):.3f} .. {max(tw):.3f}]", ""]
            print(L[-2], flush=True)
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    open(OUT, 'w').write('\n'.join(L))


if __name__ == '__main__':
    main()
