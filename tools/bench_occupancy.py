"""Times and parity of the point-in-mesh test (csrc/occupancy.hip) on one MI355X -> profiles/occupancy_bench.txt and profiles/occupancy_parity.txt.

  python tools/bench_occupancy.py [out_dir]      # out_dir: where the two files go (default: profiles/)

Workload: 100 000 float32 points uniform in [-0.55, 0.55]^3 (what sample_occupancy_batch draws) against
  sphere 9 680      synthetic.icosphere(22, noise=0.01, seed=1), the sphere of the other benches
  sphere 200 000    synthetic.icosphere(100, noise=0.01, seed=1)
  box 12            the cube [-0.5, 0.5]^3: every triangle spans the whole box, the worst case of one wave per (triangle, column slab)
  SPR torus         recon_one_shape_SPR at depth 6 of 30 000 points of the torus
Per case, HIP events round the calls (their one stream synchronisation and host read included), 3 warm-up runs, median of 15 (min .. max):
  check_mesh_contains        the whole call: validation, rescale, sort of the points, the per-triangle pass, the counts
  1 / 64 slabs per triangle  the same call with pdhip_debug_set_mesh_contains_slabs(1) and (64): the shipped choice takes 64 for few faces and 1 from
                             16 384 faces on (a slab is a wave's, from 32 768 faces on 16 lanes', share of a triangle's columns)
  torch all pairs            the same predicate in float64 torch ops on the same device, every point against every triangle, in chunks of points
                             of at most 2^25 pairs; 1 warm-up, median of 3
  numpy oracle               tests/occupancy_common.py:oracle_contains on the host, once, at the smallest size (the 12-face box) and on the first
                             10 000 points of the 9 680-face sphere: for context only
Parity: the kernel against the torch evaluation (all points) and against the numpy oracle (where it ran); the IoU of the SPR torus against
Solid.sdf < 0 at the same points is reported, not asserted."""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)
from pointdreamer_amd import _lib, synthetic, spr, geometry_metrics as G      # noqa: E402
from tools.bench_geometry_metrics import median_ms, clocks, WARMUP, REPEAT      # noqa: E402
import occupancy_common as oc      # noqa: E402

N = 100000
PAIRS = 1 << 25


def torch_contains(vertices, faces, points, resolution=512):
    """The all-pairs evaluation of include/pdhip.h's definition in float64 torch ops (one kernel per operation: no contraction)."""
    v, p = vertices.double(), points.double()
    tri = v[faces]
    flat = tri.reshape(-1, 3)
    bmin, bmax = flat.min(0).values, flat.max(0).values
    scale = (resolution - 1) / (bmax - bmin)
    translate = 0.5 - scale * bmin
    tri, p = scale * tri + translate, scale * p + translate
    inside = ((0 <= p) & (p <= resolution)).all(1)
    t1, t2, t3 = tri[:, 0], tri[:, 1], tri[:, 2]
    A00, A01, A10, A11 = t1[:, 0] - t3[:, 0], t2[:, 0] - t3[:, 0], t1[:, 1] - t3[:, 1], t2[:, 1] - t3[:, 1]
    detA = A00 * A11 - A01 * A10
    ok, s_detA, abs_detA = detA != 0, torch.sign(detA), detA.abs()
    v1, v2 = t3 - t1, t2 - t1
    n0 = v1[:, 1] * v2[:, 2] - v1[:, 2] * v2[:, 1]
    n1 = v1[:, 2] * v2[:, 0] - v1[:, 0] * v2[:, 2]
    n2 = v1[:, 0] * v2[:, 1] - v1[:, 1] * v2[:, 0]
    s_n2, abs_n2 = torch.sign(n2), n2.abs()
    t1zn = t1[:, 2] * abs_n2
    above = torch.zeros((p.shape[0],), dtype=torch.int64, device=p.device)
    below = torch.zeros_like(above)
    chunk = max(1, PAIRS // faces.shape[0])
    for b in range(0, p.shape[0], chunk):
        c = p[b:b + chunk]
        px, py, pz = c[:, 0:1], c[:, 1:2], c[:, 2:3]
        y0, y1 = px - t3[None, :, 0], py - t3[None, :, 1]
        u = (A11[None] * y0 - A01[None] * y1) * s_detA[None]
        w = (-A10[None] * y0 + A00[None] * y1) * s_detA[None]
        uw = u + w
        hit = ok[None] & (0 < u) & (u < abs_detA[None]) & (0 < w) & (w < abs_detA[None]) & (0 < uw) & (uw < abs_detA[None]) & (abs_n2[None] != 0)
        depth = t1zn[None] + (n0[None] * (t1[None, :, 0] - px) + n1[None] * (t1[None, :, 1] - py)) * s_n2[None]
        rhs = pz * abs_n2[None]
        above[b:b + chunk] = (hit & (depth >= rhs)).sum(1)
        below[b:b + chunk] = (hit & (depth < rhs)).sum(1)
    return inside & (above % 2 == 1) & (below % 2 == 1)


def main(out_dir):
    L = _lib.lib()
    dev = torch.device('cuda', torch.cuda.current_device())
    T = lambda x: torch.from_numpy(np.array(x)).to(dev)
    points_h = np.array(oc.uniform_points(N, 7))
    points = T(points_h)
    xyz, rgb, nrm = synthetic.solid('torus').sample(30000, seed=1)
    sv, sf, _ = spr.recon_one_shape_SPR(xyz, rgb, gt_normals=nrm, depth=6)
    cases = [('sphere 9 680', *map(T, synthetic.icosphere(22, noise=0.01, seed=1)), 10000),
             ('sphere 200 000', *map(T, synthetic.icosphere(100, noise=0.01, seed=1)), 0),
             ('box 12', *map(T, oc.box_mesh()), N),
             ('SPR torus depth 6', sv.float().contiguous(), sf.long().contiguous(), 0)]
    B = [f"Point-in-mesh test on one MI355X (tools/bench_occupancy.py): {N} float32 points uniform in [-0.55, 0.55]^3, hash_resolution 512;",
         f"HIP events round the calls, {WARMUP} warm-up runs, median of {REPEAT} (min .. max); the torch baseline 1 warm-up, median of 3.",
         f"device: {torch.cuda.get_device_name(dev)}; clocks after the run: CLOCKS", ""]
    P = ["Parity of the point-in-mesh test (tools/bench_occupancy.py).", ""]
    for name, v, f, n_host in cases:
        occ, counts = G.check_mesh_contains(v, f, points, return_counts=True)
        counts = counts.cpu().tolist()
        mine = median_ms(lambda: G.check_mesh_contains(v, f, points))
        forced = {}
        for slabs in (1, 64):
            old = L.pdhip_debug_set_mesh_contains_slabs(slabs)
            try:
                forced[slabs] = (median_ms(lambda: G.check_mesh_contains(v, f, points)), torch.equal(G.check_mesh_contains(v, f, points), occ))
            finally:
                L.pdhip_debug_set_mesh_contains_slabs(old)
        base = median_ms(lambda: torch_contains(v, f, points), warmup=1, repeat=3)
        want = torch_contains(v, f, points)
        again = G.check_mesh_contains(v, f, points)
        B += [f"case {name}: {f.shape[0]} faces; contained {counts[0]}, parities disagree {counts[1]}, outside the box {counts[2]} of {N}",
              f"  check_mesh_contains (whole call)    {mine[0]:10.3f} ms  ({mine[1]:.3f} .. {mine[2]:.3f})",
              f"    one slab per triangle             {forced[1][0][0]:10.3f} ms  ({forced[1][0][1]:.3f} .. {forced[1][0][2]:.3f})   = {forced[1][0][0] / mine[0]:.2f} x the shipped choice",
              f"    64 slabs per triangle             {forced[64][0][0]:10.3f} ms  ({forced[64][0][1]:.3f} .. {forced[64][0][2]:.3f})   = {forced[64][0][0] / mine[0]:.2f} x the shipped choice",
              f"  torch all pairs, f64                {base[0]:10.3f} ms  ({base[1]:.3f} .. {base[2]:.3f})   = {base[0] / mine[0]:.2f} x the kernel's time"]
        P += [f"case {name} ({f.shape[0]} faces, {N} points):",
              f"  against the torch all-pairs evaluation: {int((occ != want).sum())} of {N} differ; two calls give {'EQUAL' if torch.equal(occ, again) else 'DIFFERENT'} bytes",
              f"  1 and 64 slabs per triangle against the shipped choice: bytes {'EQUAL' if forced[1][1] and forced[64][1] else 'DIFFER'}"]
        if n_host:
            t0 = time.perf_counter()
            host = oc.oracle_contains(v.cpu().numpy(), f.cpu().numpy(), points_h[:n_host])
            ms = (time.perf_counter() - t0) * 1e3
            B.append(f"  numpy oracle (host, once)           {ms:10.1f} ms  for the first {n_host} points")
            P.append(f"  against the numpy oracle on the first {n_host} points: {int((occ[:n_host].cpu().numpy() != host).sum())} differ")
        if name.startswith('SPR'):
            truth = T(synthetic.solid('torus').sdf(points_h) < 0)
            iou = G.compute_iou(occ, truth)
            P.append(f"  IoU of the depth-6 reconstruction of the torus ({xyz.shape[0]} points) against Solid.sdf < 0 at the {N} points: {iou!r} "
                     f"({int(truth.sum())} points inside the solid)   [reported, not asserted]")
        B.append("")
        P.append("")
        for line in B[-8:] + P[-6:]:
            print(line, flush=True)
    B[2] = B[2].replace('CLOCKS', clocks())
    os.makedirs(out_dir, exist_ok=True)
    open(os.path.join(out_dir, 'occupancy_bench.txt'), 'w').write('\n'.join(B) + '\n')
    open(os.path.join(out_dir, 'occupancy_parity.txt'), 'w').write('\n'.join(P) + '\n')


if __name__ == '__main__':
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, 'profiles'))
