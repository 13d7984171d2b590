"""Times and parity of the geometry scores (csrc/cloud_metrics.hip) on one MI355X -> profiles/geometry_metrics_bench.txt and
profiles/geometry_metrics_parity.txt.

  python tools/bench_geometry_metrics.py [out_dir]      # out_dir: where the two files go (default: profiles/)

Workload: 100 000 x 100 000 points, both directions plus the reduction (what eval_mesh does at the reference's n_points).
  torus        two samplings (seeds 0 and 1) of the torus reconstructed at depth 7 from 30 000 points
  adversarial  the same with a tenth of the second sampling moved to ten times the extent outside the box
Per case, HIP events round the calls (their one stream synchronisation and host read included), 3 warm-up runs, median of 15:
  eval_pointcloud            both directions, both reductions, the read-back and the host divisions
  nearest_points x 2         both directions, the shipped path: one thread per query, rings of cells from global memory, nothing staged
  LDS phase first x 2        pdhip_debug_set_nearest_path(1): the targets of a workgroup's cell box staged in LDS, the ring scan for what it left
  torch.cdist + min x 2      float64, query chunks of 2 048 rows (1.6 GB of distances per chunk), same process, same box; 1 warm-up, median of 3
  scipy cKDTree x 2          on the host (build + query), once: for context only
Parity: the twelve scores on the golden fixture against the reference's values, and at the timed size the shipped path against the LDS-phase
path (bytes) and against cdist (whose distances are sqrt of a differently rounded sum: a relative figure)."""
import os
import statistics
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from pointdreamer_amd import _lib, synthetic, spr, geometry_metrics as G      # noqa: E402
from tools.bench_surface_recon import timed      # noqa: E402

WARMUP, REPEAT, N = 3, 15, 100000


def median_ms(fn, warmup=WARMUP, repeat=REPEAT):
    ts = []
    for it in range(warmup + repeat):
        t, _ = timed(fn)
        if it >= warmup:
            ts.append(t)
    return statistics.median(ts), min(ts), max(ts)


def cdist_min(q, t, chunk=2048):
    q, t = q.double(), t.double()
    d = torch.empty((q.shape[0],), dtype=torch.float64, device=q.device)
    i = torch.empty((q.shape[0],), dtype=torch.int64, device=q.device)
    for b in range(0, q.shape[0], chunk):
        d[b:b + chunk], i[b:b + chunk] = torch.cdist(q[b:b + chunk], t).min(dim=1)
    return d, i


def clocks():
    try:
        out = subprocess.run(['rocm-smi', '--showclocks'], capture_output=True, text=True, timeout=30).stdout
        rows = [' '.join(l.split()) for l in out.splitlines() if 'GPU[0]' in l and ('sclk' in l or 'mclk' in l)]
        return '; '.join(rows) if rows else 'not reported'
    except Exception as e:                                          # noqa: BLE001
        return f'not read ({type(e).__name__})'


def main(out_dir):
    L = _lib.lib()
    dev = torch.device('cuda', torch.cuda.current_device())
    xyz, rgb, nrm = synthetic.solid('torus').sample(30000, seed=1)
    v, f, _ = spr.poisson_reconstruct(torch.from_numpy(xyz).to(dev), torch.from_numpy(nrm).to(dev), depth=7, colors=torch.from_numpy(rgb).to(dev))
    a, na = G.sample_mesh_cloud(v, f, N, seed=0)
    b, nb = G.sample_mesh_cloud(v, f, N, seed=1)
    ext = float((a.max(0).values - a.min(0).values).max())
    far = b.clone()
    gen = torch.Generator(device=dev).manual_seed(2)
    axis = torch.randint(0, 3, (N // 10,), device=dev, generator=gen)
    sign = torch.randint(0, 2, (N // 10,), device=dev, generator=gen).float() * 2 - 1
    far[torch.arange(N // 10, device=dev) * 10, axis] = sign * 10.0 * ext
    cases = [('torus', a, na, b, nb), ('adversarial', a, na, far, nb)]
    B = [f"Geometry scores on one MI355X (tools/bench_geometry_metrics.py): {N} x {N} points, both directions; the torus reconstructed at depth 7",
         f"from 30 000 points ({len(f)} faces), sampled with seeds 0 and 1; HIP events round the calls, {WARMUP} warm-up runs, median of {REPEAT} (min .. max).",
         f"device: {torch.cuda.get_device_name(dev)}; clocks after the run: CLOCKS", ""]
    P = ["Parity of the geometry scores (tools/bench_geometry_metrics.py).", ""]
    for name, p, n_p, t, n_t in cases:
        both = lambda: (G.nearest_points(t, p), G.nearest_points(p, t))
        full = median_ms(lambda: G.eval_pointcloud(p, t, n_p, n_t))
        lds = median_ms(both)
        ref = both()
        old = L.pdhip_debug_set_nearest_path(1)
        try:
            counts = [G.nearest_points(x, y, return_counts=True)[2].cpu().tolist() for x, y in ((t, p), (p, t))]
            ring = median_ms(both)
            forced = both()
        finally:
            L.pdhip_debug_set_nearest_path(old)
        same = all(torch.equal(x[0].view(torch.int64), y[0].view(torch.int64)) and torch.equal(x[1], y[1]) for x, y in zip(ref, forced))
        cd = median_ms(lambda: (cdist_min(t, p), cdist_min(p, t)), warmup=1, repeat=3)
        cref = (cdist_min(t, p), cdist_min(p, t))
        rel = max(float(((c[0] - r[0].sqrt()).abs() / r[0].sqrt().clamp_min(1e-300)).max()) for c, r in zip(cref, ref))
        idx_diff = sum(int((c[1] != r[1].long()).sum()) for c, r in zip(cref, ref))
        pn, tn = p.cpu().numpy().astype(np.float64), t.cpu().numpy().astype(np.float64)
        from scipy.spatial import cKDTree
        t0 = time.perf_counter()
        kd = (cKDTree(pn).query(tn), cKDTree(tn).query(pn))
        host = (time.perf_counter() - t0) * 1e3
        kd_rel = max(float(np.max(np.abs(k[0] - np.sqrt(r[0].cpu().numpy())) / np.maximum(k[0], 1e-300))) for k, r in zip(kd, ref))
        share = [c[0] / float(N) for c in counts]
        B += [f"case {name}: cells per axis {counts[0][2]}; the LDS phase (when it runs) certifies {counts[0][0]} of {N} (target -> prediction) and "
              f"{counts[1][0]} of {N} (prediction -> target) queries = {100 * share[0]:.2f} % / {100 * share[1]:.2f} %",
              f"  eval_pointcloud (whole call)        {full[0]:10.3f} ms  ({full[1]:.3f} .. {full[2]:.3f})",
              f"  nearest_points x 2, shipped path    {lds[0]:10.3f} ms  ({lds[1]:.3f} .. {lds[2]:.3f})",
              f"  nearest_points x 2, LDS phase first {ring[0]:10.3f} ms  ({ring[1]:.3f} .. {ring[2]:.3f})   = {ring[0] / lds[0]:.2f} x the shipped path",
              f"  torch.cdist f64 + min x 2           {cd[0]:10.3f} ms  ({cd[1]:.3f} .. {cd[2]:.3f})   = {cd[0] / lds[0]:.1f} x the shipped path",
              f"  scipy cKDTree x 2 (host, once)      {host:10.1f} ms", ""]
        P += [f"case {name} ({N} x {N}, both directions):",
              f"  shipped path against the LDS-phase path: d2 and idx bytes {'EQUAL' if same else 'DIFFER'}",
              f"  against torch.cdist + min (f64): largest relative difference of the distance {rel:.3e}; {idx_diff} of {2 * N} indices differ (cdist",
              "    rounds another expression: near-ties may fall the other way)",
              f"  against scipy cKDTree: largest relative difference of the distance {kd_rel:.3e}", ""]
        for line in B[-7:]:
            print(line, flush=True)
    B[2] = B[2].replace('CLOCKS', clocks())
    # the golden fixture against the reference's values
    g = dict(np.load(os.path.join(ROOT, 'tests', 'golden', 'geometry_metrics_ref.npz'), allow_pickle=False))
    T = lambda x: torch.from_numpy(np.array(x)).to(dev)
    got = G.eval_pointcloud(T(g['pointcloud']), T(g['pointcloud_tgt']), T(g['normals']), T(g['normals_tgt']))
    P += ["golden fixture (4 096 x 3 500 points with normals) against MeshEvaluator.eval_pointcloud of the reference on the CPU:",
          "  score                   device                    reference                 relative difference"]
    for k, want in zip((str(k) for k in g['keys']), (float(x) for x in g['values'])):
        P.append(f"  {k:22s}  {got[k]!r:24s}  {want!r:24s}  {abs(got[k] - want) / abs(want):.3e}")
    P.append(f"  bounds of the tests: (4096 + 8) 2^-53 = {(4096 + 8) * 2.0 ** -53:.3e} for the means, 4 2^-53 = {4 * 2.0 ** -53:.3e} for the F-scores")
    os.makedirs(out_dir, exist_ok=True)
    open(os.path.join(out_dir, 'geometry_metrics_bench.txt'), 'w').write('\n'.join(B) + '\n')
    open(os.path.join(out_dir, 'geometry_metrics_parity.txt'), 'w').write('\n'.join(P) + '\n')
    print('\n'.join(P))


if __name__ == '__main__':
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, 'profiles'))
