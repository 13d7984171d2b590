"""Times of the mesh decimation (csrc/simplify_mesh.hip) on one MI355X -> profiles/mesh_simplify_bench.txt.

  python tools/bench_mesh_simplify.py     # simplify_mesh (with vertex colours) to 10 000 faces on the torus reconstructed at depth 7 and 8 from
                                          #   30 000 points: HIP events, 3 warm-up runs, median of 15, rounds and faces per round
                                          #   + the CLI's per-shape total at depth 7 and 8 with spr_faces=10000 against the same run without it
The entry synchronises the stream itself (input check, one status read per 8 rounds), so an event pair round a call is the time a caller
waits, host reads included."""
import logging
import os
import re
import statistics
import sys
import tempfile

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from pointdreamer_amd import synthetic, spr      # noqa: E402
from pointdreamer_amd import io_utils      # noqa: E402
from tools.bench_surface_recon import timed, _Grab      # noqa: E402  (the event timer and the log grabber are shared)

OUT = os.path.join(ROOT, 'profiles', 'mesh_simplify_bench.txt')
WARMUP, REPEAT, TARGET = 3, 15, 10000


def cli_stages(workdir, depth, faces):
    """Second (warm) CLI run of a fresh output directory each, with or without `spr_faces`: stage times in ms from the log."""
    from pointdreamer_amd import demo
    xyz, rgb, _ = synthetic.solid('torus').sample(30000, seed=1)
    pc = os.path.join(workdir, 'torus.ply')
    io_utils.save_colored_pc_ply(xyz, rgb, pc)
    got = {}
    for run in range(2):
        over = ['xatlas_texture_res=1024', f'output_path={os.path.join(workdir, f"out_{depth}_{faces}_{run}")}', 'geo_from=SPR', f'spr_depth={depth}']
        if faces:
            over.append(f'spr_faces={faces}')
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
        got['faces'] = len(io_utils.load_obj_mesh(os.path.join(out, 'models', 'model_normalized.obj'))[1])
    return got


def main():
    L = ["Mesh decimation on one MI355X (tools/bench_mesh_simplify.py): the torus reconstructed from 30 000 points, simplify_mesh with vertex",
         f"colours to {TARGET} faces, HIP events round the call (its host reads included), {WARMUP} warm-up runs, median of {REPEAT}.", "",
         "depth  faces in  faces out | simplify ms | rounds  faces per round"]
    xyz, rgb, nrm = synthetic.solid('torus').sample(30000, seed=1)
    X, C, Nn = torch.from_numpy(xyz).cuda(), torch.from_numpy(rgb).cuda(), torch.from_numpy(nrm).cuda()
    for depth in (7, 8):
        v, f, c = spr.poisson_reconstruct(X, Nn, depth=depth, colors=C)
        ts, info = [], None
        for it in range(WARMUP + REPEAT):
            t, res = timed(lambda: spr.simplify_mesh(v, f, TARGET, colors=c, return_counts=True))
            info = res[-1]
            if it >= WARMUP:
                ts.append(t)
        L.append(f"{depth}      {len(f):8d}  {info['faces']:9d} | {statistics.median(ts):11.3f} | {info['rounds']:6d}  "
                 f"{(len(f) - info['faces']) / max(1, info['rounds']):15.0f}")
        print(L[-1], flush=True)
    L += ["", "CLI (`nearest.yaml`, atlas 1024, torus of 30 000 points, second run of the process, fresh output directory), ms from the log, the same",
          "box and process for both rows of a depth: geometry = 'Get Geometry time' (normals + reconstruction [+ decimation] + writing and re-reading",
          "the OBJ cache), unwrap = 'UV unwrapping time', texture = 'generate texture time'.",
          "mesh                          faces   | geometry   unwrap   texture   total"]
    with tempfile.TemporaryDirectory() as wd:
        for depth in (6, 7, 8):
            for faces in ((0,) if depth == 6 else (0, TARGET)):
                g = cli_stages(wd, depth, faces)
                tag = f"SPR depth {depth}" + (f" spr_faces={faces}" if faces else "")
                L.append(f"{tag:28s} {g['faces']:7d}  | {g.get('geometry', 0.0):8.1f} {g.get('unwrap', 0.0):8.1f} {g['texture']:9.1f} {g['total']:8.1f}")
                print(L[-1], flush=True)
    open(OUT, 'w').write('\n'.join(L) + '\n')


if __name__ == '__main__':
    main()
