"""One case of tools/bench_mesh_distance.py, 8 calls of geometry_metrics.closest_on_mesh after one warm-up, for a kernel trace of its own:

  rocprofv3 --kernel-trace --stats -d <dir> -- python tools/prof_mesh_distance.py <faces: 9680 | 200000> <uniform | surface>
  python tools/rocpd_stats.py <dir>/*/*.db          # -> the per-kernel table of profiles/mesh_distance_kernel_stats.txt"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)
from pointdreamer_amd import synthetic, geometry_metrics as G      # noqa: E402
import occupancy_common as oc      # noqa: E402

N = 100000


def main(faces, which):
    dev = torch.device('cuda', torch.cuda.current_device())
    T = lambda x: torch.from_numpy(np.array(x)).to(dev)
    n = {9680: 22, 200000: 100}[faces]
    v, f = map(T, synthetic.icosphere(n, noise=0.01, seed=1))
    points = T(oc.uniform_points(N, 7)) if which == 'uniform' else G.sample_mesh_cloud(*map(T, synthetic.icosphere(n, noise=0.01, seed=2)), N, seed=3)[0]
    for _ in range(9):
        counts = G.closest_on_mesh(v, f, points, return_closest=True, return_counts=True)[3]
    torch.cuda.synchronize()
    print('faces', f.shape[0], which, 'counts', counts.cpu().tolist())


if __name__ == '__main__':
    main(int(sys.argv[1]), sys.argv[2])
