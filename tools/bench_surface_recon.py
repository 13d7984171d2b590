"""Times of the surface reconstruction (csrc/surface_recon.hip) on one MI355X -> profiles/surface_recon_bench.txt.

  python tools/bench_surface_recon.py                # torus clouds of 10 k / 30 k points x depth 6 / 7 / 8: estimate_normals, poisson_reconstruct
                                                     #   (with vertex colours) and their sum, HIP events, 3 warm-up runs, median of 15
                                                     #   + the CLI stages downstream at each depth next to the 10 k-face stand-in
  python tools/bench_surface_recon.py --one 30000 7  # one reconstruction, for `rocprofv3 --kernel-trace --stats -- python tools/... --one`
                                                     #   (-> profiles/surface_recon_kernel_stats.txt: the per-kernel shares of the stages)
The two entry points synchronise the stream themselves (bounding box, solver status, sizes), so an event pair round a call is the
time a caller waits, host reads included."""
import logging
import os
import re
import statistics
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from pointdreamer_amd import synthetic, spr, io_utils      # noqa: E402

OUT = os.path.join(ROOT, 'profiles', 'surface_recon_bench.txt')
WARMUP, REPEAT = 3, 15


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    r = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), r


def bench_case(X, C, depth):
    tn, tr = [], []
    info = None
    for it in range(WARMUP + REPEAT):
        t1, nrm = timed(lambda: spr.estimate_normals(X))
        t2, res = timed(lambda: spr.poisson_reconstruct(X, nrm, depth=depth, colors=C, return_counts=True))
        info = res[-1]
        if it >= WARMUP:
            tn.append(t1)
            tr.append(t2)
    return statistics.median(tn), statistics.median(tr), statistics.median([a + b for a, b in zip(tn, tr)]), info


class _Grab(logging.Handler):
    def __init__(self):
        super().__init__()
        self.lines = []

    def emit(self, record):
        self.lines.append(record.getMessage())


def cli_stages(workdir, depth):
    """Second (warm) CLI run of a fresh output directory each: Get Geometry / UV unwrapping / generate texture times from the log."""
    from pointdreamer_amd import demo
    xyz, rgb, _ = synthetic.solid('torus').sample(30000, seed=1)
    pc = os.path.join(workdir, 'torus.ply')
    io_utils.save_colored_pc_ply(xyz, rgb, pc)
    got = {}
    for run in range(2):
        over = ['xatlas_texture_res=1024', f'output_path={os.path.join(workdir, f"out_{depth}_{run}")}']
        if depth:
            over += ['geo_from=SPR', f'spr_depth={depth}']
        grab = _Grab()
        logging.getLogger('pointdreamer_amd').addHandler(grab)
        try:
            out = demo.main(['--config', os.path.join(ROOT, 'configs', 'nearest.yaml'), '--pc_file', pc, '--set'] + over)[0]
        finally:
            logging.getLogger('pointdreamer_amd').removeHandler(grab)
        got = {}
        for line in grab.lines:
            for key, pat in (('geometry', r'Get Geometry time: ([\d.e-]+)'), ('unwrap', r'UV unwrapping time: ([\d.e-]+)'),
                             ('texture', r'generate texture time: ([\d.e-]+)'), ('total', r'total time: ([\d.e-]+)')):
                m = re.search(pat, line)
                if m:
                    got[key] = float(m.group(1)) * 1e3
        v, f = io_utils.load_obj_mesh(os.path.join(out, 'models', 'model_normalized.obj'))
        got['faces'] = len(f)
    return got


def main():
    if '--one' in sys.argv:
        i = sys.argv.index('--one')
        n, depth = int(sys.argv[i + 1]), int(sys.argv[i + 2])
        xyz, rgb, _ = synthetic.solid('torus').sample(n, seed=1)
        X, C = torch.from_numpy(xyz).cuda(), torch.from_numpy(rgb).cuda()
        for _ in range(2):
            nrm = spr.estimate_normals(X)
            spr.poisson_reconstruct(X, nrm, depth=depth, colors=C)
        torch.cuda.synchronize()
        return
    L = ["Surface reconstruction on one MI355X (tools/bench_surface_recon.py): torus cloud, HIP events round each call (host reads of the call",
         f"included), {WARMUP} warm-up runs, median of {REPEAT}.  normals = estimate_normals (k 16, 32 eyes, hidden-point removal included);",
         "recon = poisson_reconstruct with vertex colours (cell list, right-hand side, conjugate gradients, iso value, marching cubes).", "",
         "points  depth | normals ms  recon ms  total ms | CG iterations  launches/iteration  vertices  faces"]
    for n in (10000, 30000):
        xyz, rgb, _ = synthetic.solid('torus').sample(n, seed=1)
        X, C = torch.from_numpy(xyz).cuda(), torch.from_numpy(rgb).cuda()
        for depth in (6, 7, 8):
            tn, tr, tt, info = bench_case(X, C, depth)
            L.append(f"{n:6d}  {depth}     | {tn:9.3f}  {tr:8.3f}  {tt:8.3f} | {info['iterations']:6d}         2                   {info['vertices']:7d}  {info['faces']:7d}")
            print(L[-1], flush=True)
    L += ["", "CLI (`nearest.yaml`, atlas 1024, torus of 30 000 points, second run of the process, fresh output directory), ms from the log:",
          "geometry = 'Get Geometry time' (normals + reconstruction + writing and re-reading the OBJ cache), unwrap = 'UV unwrapping time' (device",
          "unwrap + atlas raster + cache write), texture = 'generate texture time' (project, raster, inpaint, unproject, neighbour completion).",
          "mesh              faces   | geometry   unwrap   texture   total"]
    with tempfile.TemporaryDirectory() as wd:
        for depth in (0, 6, 7, 8):
            g = cli_stages(wd, depth)
            L.append(f"{'stand-in sphere' if not depth else 'SPR depth ' + str(depth):16s} {g['faces']:7d}  | {g.get('geometry', 0.0):8.1f} {g.get('unwrap', 0.0):8.1f} "
                     f"{g['texture']:9.1f} {g['total']:8.1f}")
            print(L[-1], flush=True)
    open(OUT, 'w').write('\n'.join(L) + '\n')


if __name__ == '__main__':
    main()
