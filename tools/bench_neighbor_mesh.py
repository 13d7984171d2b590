"""Times unproject.paint_invisible_areas_by_neighbors per shape with the mesh work on the host (mesh_on='host': numpy subdivision,
UV table and CSR plus their transfers -- what every commit before the device entries did) and on the device (mesh_on='device',
csrc/neighbor_mesh.hip), in one process on one GPU, on two inputs:
  icosphere   synthetic.icosphere(32), 20 480 faces, a random third picked, per-corner UVs, a half-painted 1024^2 atlas
  clock       the arguments the pipeline hands to the stage for tests/golden/clock.ply under configs/nearest.yaml
Each route is warmed up, then timed `--reps` times: wall clock around the call (with a device synchronisation) and HIP events on the
stream.  Both routes must return the same bytes.  Writes profiles/neighbor_mesh_bench.txt (or --out).

  python tools/bench_neighbor_mesh.py [--reps 10] [--warmup 3] [--out profiles/neighbor_mesh_bench.txt]"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
DEV = 'cuda'


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def icosphere_case(A=1024):
    from pointdreamer_amd import synthetic
    v, f = synthetic.icosphere(32)
    rng = np.random.default_rng(0)
    fu = np.arange(3 * len(f), dtype=np.int64).reshape(-1, 3)
    u = rng.uniform(0.02, 0.98, (3 * len(f), 2)).astype(np.float32)
    tif = np.sort(rng.choice(len(f), len(f) // 3, replace=False)).astype(np.int64)
    atlas = rng.uniform(0, 1, (A, A, 3)).astype(np.float32)
    painted = rng.uniform(size=(A, A)) > 0.5
    return [T(v), T(f), T(u), T(fu), tif, T(atlas), T(painted)]


def clock_case(tmp):
    """Runs the pipeline once on clock.ply and keeps the arguments of its paint_invisible_areas_by_neighbors call."""
    from pointdreamer_amd import demo, pipeline, io_utils, unproject as up
    cfg, inpainter, camera_info, logger = demo.prepare(os.path.join(ROOT, 'configs', 'nearest.yaml'), torch.device(DEV),
                                                       overrides={'output_path': tmp, 'optimize_from': None})
    sh = demo._load_shape(cfg, os.path.join(ROOT, 'tests', 'golden', 'clock.ply'), 'clock', DEV, logger)
    kept, orig = [], up.paint_invisible_areas_by_neighbors

    def keep(*a, **kw):
        kept.append([x.clone() if torch.is_tensor(x) else np.array(x) for x in a[:7]])
        return orig(*a, **kw)
    up.paint_invisible_areas_by_neighbors = keep
    try:
        pipeline.colorize_one_mesh(sh['coords'], sh['colors'], sh['vertices'], sh['faces'], sh['f_normals'], sh['xatlas'], camera_info,
                                   inpainter=None, **demo._pipeline_kwargs(cfg))
    finally:
        up.paint_invisible_areas_by_neighbors = orig
    io_utils.flush()
    assert len(kept) == 1, "configs/nearest.yaml completes by 'neighbor'"
    return kept[0]


def time_route(args, route, warmup, reps):
    from pointdreamer_amd import unproject as up
    out = None
    wall, dev = [], []
    for k in range(warmup + reps):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record()
        out = up.paint_invisible_areas_by_neighbors(*args, use_atlas=True, mesh_on=route)
        e1.record()
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        if k >= warmup:
            wall.append((t1 - t0) * 1e3)
            dev.append(e0.elapsed_time(e1))
    return out, np.array(wall), np.array(dev)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'neighbor_mesh_bench.txt'))
    ap.add_argument('--skip-clock', action='store_true')
    a = ap.parse_args()
    import tempfile
    lines = [f"paint_invisible_areas_by_neighbors per shape, mesh_on='host' vs 'device'; {torch.cuda.get_device_name(0)}; "
             f"warmup {a.warmup}, reps {a.reps}; ms as median (min .. max)"]
    cases = [('icosphere(32) third picked', icosphere_case())]
    if not a.skip_clock:
        with tempfile.TemporaryDirectory() as tmp:
            cases.append(('clock.ply nearest.yaml', clock_case(tmp)))
    for name, args in cases:
        F, K = args[1].shape[0], len(args[4])
        res = {}
        for route in ('host', 'device'):
            res[route] = time_route(args, route, a.warmup, a.reps)
        same = torch.equal(res['host'][0], res['device'][0])
        lines.append(f"{name}: V={args[0].shape[0]} F={F} picked={K} A={args[5].shape[0]} identical={same}")
        for route in ('host', 'device'):
            _, w, d = res[route]
            lines.append(f"  {route:6s} wall {np.median(w):8.3f} ({w.min():.3f} .. {w.max():.3f})   "
                         f"events {np.median(d):8.3f} ({d.min():.3f} .. {d.max():.3f})")
        lines.append(f"  device / host wall: {np.median(res['device'][1]) / np.median(res['host'][1]):.3f}")
        assert same, name
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write(text)


if __name__ == '__main__':
    main()
