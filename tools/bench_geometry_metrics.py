"""Times and parity of the geometry scores (csrc/cloud_metrics.hip) on one MI355X -> profiles/geometry_metrics_bench.txt and
profiles/geometry_metrics_parity.txt.

  python tools/bench_geometry_metrics.py [out_dir]      # out_dir: where the two files go (default: profiles/)
  python tools/bench_geometry_metrics.py bytes          # -> tests/golden/cell_grid_parent.npz: run at the commit whose bytes a refactor of the
                                                        #   f64 cell-list units (cloud_metrics, knn, subsample, mesh_distance) must keep

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
import hashlib
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
BYTES_PATH = os.path.join(ROOT, 'tests', 'golden', 'cell_grid_parent.npz')


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



# ---- the bytes of the four f64 cell-list entries under every hook setting (tests/test_gpu_cell_grid.py)
def cell_grid_inputs():
    """The clouds and the mesh of cell_grid_bytes (numpy, nothing on the device):
      q, t     2 000 points each of the torus (seeds 1, 2); 20 targets moved to 10 x the extent and 20 queries to 3 x the extent along a random
               axis, so that the two boxes differ (the grid is cut to where they meet) and some queries are far from every target
      flat     the targets with y = 0.25: no extent along one axis;  one: 300 copies of one point: a box without extent, one cell
      v, f, p  icosphere(10) (2 000 faces) plus six needles, six specks and one repeated-index face; 2 000 uniform points of [-0.7, 0.7]^3
      fv, ff   a 12 x 12 grid of triangles in the plane z = 0.25: a mesh without extent along one axis"""
    rng = np.random.default_rng(2024)
    q, t = (synthetic.solid('torus').sample(2000, seed=s)[0].copy() for s in (1, 2))
    ext = float((t.max(0) - t.min(0)).max())
    for x, factor in ((t, 10.0), (q, 3.0)):
        x[rng.choice(len(x), 20, replace=False), rng.integers(0, 3, 20)] = (rng.integers(0, 2, 20) * 2 - 1) * np.float32(factor * ext)
    flat = t.copy()
    flat[:, 1] = 0.25
    one = np.tile(np.float32([[0.1, -0.2, 0.3]]), (300, 1))
    v, f = synthetic.icosphere(10)
    ev, ef = [], [[3, 3, 9]]
    for k in range(12):
        a, d = rng.uniform(-0.45, 0.45, 3), rng.normal(size=3)
        d /= np.linalg.norm(d)
        e = np.cross(d, rng.normal(size=3))
        e /= np.linalg.norm(e)
        h = 10.0 ** rng.uniform(-6, -4)
        tri = [a, a + 0.08 * d, a + 0.04 * d + 10.0 ** rng.uniform(-7, -5) * e] if k < 6 else [a, a + h * d, a + h * e]
        ef.append([len(v) + len(ev) + i for i in range(3)])
        ev += tri
    v, f = np.concatenate([v, np.array(ev, np.float32)]), np.concatenate([f[:1000], np.array(ef, np.int64), f[1000:]])
    p = rng.uniform(-0.7, 0.7, (2000, 3)).astype(np.float32)
    i, j = (x.ravel() for x in np.meshgrid(np.arange(12), np.arange(12), indexing='ij'))
    gx, gy = (x.ravel() for x in np.meshgrid(np.arange(13), np.arange(13), indexing='ij'))
    fv = np.stack([gx / 12.0 - 0.5, gy / 12.0 - 0.5, np.full(169, 0.25)], -1).astype(np.float32)
    a = i * 13 + j
    ff = np.concatenate([np.stack([a, a + 13, a + 14], -1), np.stack([a, a + 14, a + 1], -1)]).astype(np.int64)
    return dict(q=q, t=t, flat=flat, one=one, v=v, f=np.ascontiguousarray(f), p=p, fv=fv, ff=ff)


def cell_grid_bytes():
    """name -> numpy array, what tests/golden/cell_grid_parent.npz pins: per call `<case>.counts` (the int32 [4] verbatim: it shows how the queries
    split between the certificate and the scan of everything, which no oracle sees) and `<case>.<output>` = the SHA-256 of the output's bytes
    (uint8 [32]; kNN's outputs at k = 64 alone are 1.5 MB per setting, and a digest pins the same bytes).
      nearest.torus.path{0,1}                    pdhip_nearest_points(q, t)
      knn.torus.k{1,8,64}.path{0,1,2}.cells{0,5} pdhip_knn_points(q, t, k)
      fps.torus.cells{0,7}                       pdhip_fps(t, 200)
      mesh.path{0,1,2}.cells{0,6}                pdhip_closest_on_mesh(v, f, p) with the closest points
      *.flat, *.one                              the shipped setting on the inputs without extent along one axis / without any extent"""
    from pointdreamer_amd import outliers, subsample
    L = _lib.lib()
    dev = torch.device('cuda', torch.cuda.current_device())
    I = {k: torch.from_numpy(x).to(dev) for k, x in cell_grid_inputs().items()}
    out = {}

    def put(case, names, res):
        for name, x in zip(names, res):
            x = np.ascontiguousarray(x.cpu().numpy())
            out[f'{case}.{name}'] = x if name == 'counts' else np.frombuffer(hashlib.sha256(x.tobytes()).digest(), np.uint8)

    near = lambda case, a, b: put(case, ('d2', 'idx', 'counts'), G.nearest_points(a, b, return_counts=True))
    knn = lambda case, a, b, k: put(case, ('d2', 'idx', 'counts'), outliers.knn_points(a, b, k, return_counts=True))
    fps = lambda case, a, m: put(case, ('idx', 'min_d2', 'counts'), subsample.farthest_point_sample(a, m, return_min_d2=True, return_counts=True))
    mesh = lambda case, v, f, p: put(case, ('d2', 'face', 'closest', 'counts'), G.closest_on_mesh(v, f, p, return_closest=True, return_counts=True))
    try:
        for path in (0, 1):
            L.pdhip_debug_set_nearest_path(path)
            near(f'nearest.torus.path{path}', I['q'], I['t'])
        for k in (1, 8, 64):
            for path in (0, 1, 2):
                for cells in (0, 5):
                    assert L.pdhip_debug_set_knn(cells, path) >= 0
                    knn(f'knn.torus.k{k}.path{path}.cells{cells}', I['q'], I['t'], k)
        for cells in (0, 7):
            L.pdhip_debug_set_fps_cells(cells)
            fps(f'fps.torus.cells{cells}', I['t'], 200)
        for path in (0, 1, 2):
            for cells in (0, 6):
                L.pdhip_debug_set_closest_on_mesh(cells, path)
                mesh(f'mesh.path{path}.cells{cells}', I['v'], I['f'], I['p'])
    finally:
        L.pdhip_debug_set_nearest_path(0)
        L.pdhip_debug_set_knn(0, 0)
        L.pdhip_debug_set_fps_cells(0)
        L.pdhip_debug_set_closest_on_mesh(0, 0)
    for tag, n in (('flat', 50), ('one', 10)):
        near(f'nearest.{tag}', I[tag], I[tag])
        knn(f'knn.{tag}', I[tag], I[tag], 8)
        fps(f'fps.{tag}', I[tag], n)
    mesh('mesh.flat', I['fv'], I['ff'], I['p'])
    return out


# the calls whose counts[0] and counts[1] must both be non-zero: a fixture in which every query goes one way does not test the certificate's bound.
# (pdhip_nearest_points reports the split between its LDS phase and the ring scan, which is 0 / Q by construction on the shipped path 0: path 1.)
SPLIT_CASES = ('nearest.torus.path1', 'knn.torus.k1.path0.cells0', 'knn.torus.k8.path0.cells0', 'mesh.path0.cells0')


def write_cell_grid_bytes():
    got = cell_grid_bytes()
    for k in sorted(got):
        if k.endswith('.counts'):
            print(k, got[k].tolist())
    for case in SPLIT_CASES:
        c = got[case + '.counts']
        assert c[0] > 0 and c[1] > 0, (case, c.tolist())
    np.savez_compressed(BYTES_PATH, **got)
    print(f"{BYTES_PATH}: {os.path.getsize(BYTES_PATH)} bytes, {len(got)} arrays")


if __name__ == '__main__':
    if sys.argv[1:2] == ['bytes']:
        write_cell_grid_bytes()
    else:
        main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, 'profiles'))
