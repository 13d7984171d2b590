"""The grid density of pdhip_closest_on_mesh, measured through its hook (pdhip_debug_set_closest_on_mesh(C, 0)) on one MI355X: 100 000 points
(`surface`: on a second mesh / the analytic solid; `uniform`: [-0.55, 0.55]^3) against the two noisy icospheres of tools/bench_mesh_distance.py and
the SPR torus at depth 6 and 7, with C = floor(sqrt(F / occ)) for occ = 32 (shipped), 48, 64, 96; HIP events round the whole call, 1 warm-up, median
of 5.  Prints one line per setting (-> profiles/mesh_distance_grid_sweep.txt).

  python tools/sweep_mesh_distance.py"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)
from pointdreamer_amd import _lib, synthetic, spr, geometry_metrics as G      # noqa: E402
from tools.bench_surface_recon import timed      # noqa: E402
import occupancy_common as oc      # noqa: E402

N = 100000
OCC = (32, 48, 64, 96)


def main():
    L = _lib.lib()
    dev = torch.device('cuda', torch.cuda.current_device())
    T = lambda x: torch.from_numpy(np.array(x)).to(dev)
    uniform = T(oc.uniform_points(N, 7))
    xyz, rgb, nrm = synthetic.solid('torus').sample(30000, seed=1)
    torus = T(synthetic.solid('torus').sample(N, seed=3)[0].astype(np.float32))
    cases = []
    for n in (22, 100):
        v, f = map(T, synthetic.icosphere(n, noise=0.01, seed=1))
        cases.append((f'sphere {f.shape[0]}', v, f, G.sample_mesh_cloud(*map(T, synthetic.icosphere(n, noise=0.01, seed=2)), N, seed=3)[0]))
    for depth in (6, 7):
        sv, sf, _ = spr.recon_one_shape_SPR(xyz, rgb, gt_normals=nrm, depth=depth)
        cases.append((f'SPR{depth} {sf.shape[0]}', sv.float().contiguous(), sf.long().contiguous(), torus))
    for name, v, f, surf in cases:
        for pname, pts in (('surface', surf), ('uniform', uniform)):
            for occ in OCC:
                C = max(1, min(96, int(np.floor(np.sqrt(f.shape[0] / occ)))))
                old = L.pdhip_debug_set_closest_on_mesh(C, 0)
                try:
                    runs = [timed(lambda: G.closest_on_mesh(v, f, pts, return_closest=True, return_counts=True)) for _ in range(6)]
                finally:
                    L.pdhip_debug_set_closest_on_mesh(old // 4, old % 4)
                print(f'{name:16s} {pname:8s} occ {occ:3d} C {C:3d}: {np.median([t for t, _ in runs[1:]]):8.3f} ms  '
                      f'counts {runs[-1][1][3].cpu().tolist()}', flush=True)


if __name__ == '__main__':
    main()
