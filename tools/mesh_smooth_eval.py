"""What Taubin smoothing (pointdreamer_amd/mesh_smooth.py) does to the RECONSTRUCTED surface, measured on one MI355X ->
profiles/mesh_smooth_accuracy.txt.

  python tools/mesh_smooth_eval.py [out_dir]      # out_dir: where the file goes (default: profiles/)

The six solids of synthetic.Solid, 25 000 points each (seed 1), with Gaussian noise along the normal of standard deviation 0, h/4 and h/2 (h = the
cell of the reconstruction grid at that depth, read from a reconstruction of the clean cloud), reconstructed at depth 6 and 7 (estimated normals, as
the demo does), then smoothed with 0, 5, 10 and 20 steps of MeshLab's pair (lambda 0.5, mu -0.53), boundary vertices held.  Per row:
  rms, max   of |sdf| over the mesh's vertices, in units of h
  volume     signed volume of the mesh over Solid.volume()
  min area   the smallest face area, in units of h^2
  charts     the charts uv_unwrap (resolution 1024) cuts the mesh into
Every row is reported as it comes out; the closing lines count where smoothing lowered the rms and where it did not."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from pointdreamer_amd import mesh_checks as mc, mesh_smooth as M, spr, synthetic      # noqa: E402
from pointdreamer_amd.extract_texture_map import uv_unwrap      # noqa: E402

N_POINTS, SEED, DEPTHS, STEPS, NOISE = 25000, 1, (6, 7), (0, 5, 10, 20), ((0.0, '0'), (0.25, 'h/4'), (0.5, 'h/2'))


def charts(v, f):
    try:
        return str(len(torch.unique(uv_unwrap(v, f, 1024, return_charts=True)[2])))
    except Exception as e:                                          # noqa: BLE001
        return f'failed ({type(e).__name__})'


def main(out_dir):
    dev = torch.device('cuda', torch.cuda.current_device())
    T = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    B = ["Taubin smoothing behind the reconstruction on one MI355X (tools/mesh_smooth_eval.py): six solids, 25 000 points (seed 1), noise along the",
         "normal of standard deviation 0, h/4, h/2 (h = the grid cell), depth 6 and 7, estimated normals; 0 / 5 / 10 / 20 steps of lambda 0.5, mu -0.53,",
         "boundary vertices held.  rms and max: |sdf| of the vertices over h; volume: mesh over solid; min area: smallest face over h^2; charts: uv_unwrap.",
         f"device: {torch.cuda.get_device_name(dev)}", "",
         f"{'solid':<12} {'depth':>5} {'noise':>5} {'steps':>5} {'vertices':>9} {'faces':>8} {'rms/h':>8} {'max/h':>8} {'volume':>8} {'min area/h2':>12} {'charts':>7}"]
    better = {k: [0, 0] for _, k in NOISE}                          # per noise level: rows where the rms fell, rows with steps > 0
    for name in synthetic.Solid.NAMES:
        solid = synthetic.solid(name)
        vol = solid.volume()
        for depth in DEPTHS:
            clean = T(solid.sample(N_POINTS, seed=SEED)[0])
            h = spr.poisson_reconstruct(clean, spr.estimate_normals(clean), depth=depth, return_counts=True)[-1]['h']
            for scale, label in NOISE:
                xyz = T(solid.sample(N_POINTS, seed=SEED, noise=scale * h)[0])
                v0, f = spr.poisson_reconstruct(xyz, spr.estimate_normals(xyz), depth=depth)
                hf = f.cpu().numpy()
                base = None
                for steps in STEPS:
                    v = v0 if steps == 0 else M.taubin_smooth(v0, f, steps=steps)
                    hv = v.cpu().numpy()
                    d = np.abs(solid.sdf(hv))
                    rms = float(np.sqrt(np.mean(d * d)))
                    if steps == 0:
                        base = rms
                    else:
                        better[label][1] += 1
                        better[label][0] += rms < base
                    B.append(f"{name:<12} {depth:>5} {label:>5} {steps:>5} {len(hv):>9} {len(hf):>8} {rms / h:>8.4f} {d.max() / h:>8.4f} "
                             f"{mc.signed_volume(hv, hf) / vol:>8.4f} {float(mc.face_areas(hv, hf).min()) / (h * h):>12.3e} {charts(v, f):>7}")
                    print(B[-1], flush=True)
    B += ["", "Rows with steps > 0 whose rms lies below the unsmoothed mesh of the same cloud and depth: "
          + '; '.join(f"noise {k}: {a} of {b}" for k, (a, b) in better.items()) + '.']
    print(B[-1], flush=True)
    os.makedirs(out_dir, exist_ok=True)
    open(os.path.join(out_dir, 'mesh_smooth_accuracy.txt'), 'w').write('\n'.join(B) + '\n')


if __name__ == '__main__':
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, 'profiles'))
