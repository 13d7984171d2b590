"""Times and effect of welding / cleaning supplied meshes (csrc/mesh_clean.hip) on one MI355X -> profiles/mesh_clean_bench.txt.

  python tools/bench_mesh_clean.py [out_dir]      # out_dir: where the file goes (default: profiles/)

Speed.  Soups (three private vertices per face) of synthetic.icosphere(32 / 128 / 256): 20 480 / 327 680 / 1 310 720 faces, on the device before the
clock starts.  Two settings: tol = 0 on the soup as it is, and tol = 1e-4 of the box diagonal on the soup with every copy jittered by up to 0.4 tol.
HIP events round the whole call, its stream synchronisations and host reads included: 3 warm-up calls and the median of 9 (min .. max) for the device
calls, 1 warm-up and the median of 3 for the host baselines.
  weld_vertices / clean_mesh      the entries of pointdreamer_amd/mesh_clean.py (clean_mesh takes at most 2^21 vertices: the largest soup is refused)
  torch.unique                    tol = 0 only: torch.unique(dim=0, return_inverse=True) on the same device, then the gathers that relabel the faces
                                  and pick one vertex per class.  Its ORDERING DIFFERS: classes come sorted by coordinate, not by smallest index, and
                                  it drops neither degenerate nor duplicate faces
  numpy round trip                tol = 0 only: vertices to the host, np.unique(axis=0, return_inverse=True), the relabelled faces back
  scipy round trip                tol > 0 only, up to 10^6 vertices: cKDTree.query_pairs + csgraph.connected_components on the host
Crowded rows: 10^4, 3 10^4 and 10^5 copies of one point (every vertex scans every other: the quadratic path); the last is started only if the
row before it extrapolates to under 20 s.
Effect.  The icosphere(32) soup and a UV sphere with a duplicated seam column, before and after clean_mesh: charts of the device unwrap, components of
label_components, and whether simplify_mesh accepts the mesh."""
import os
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from pointdreamer_amd import mesh_clean as M, mesh_components, spr, synthetic      # noqa: E402
from pointdreamer_amd._lib import PdhipError      # noqa: E402
from pointdreamer_amd.extract_texture_map import uv_unwrap      # noqa: E402
from tools.bench_geometry_metrics import clocks      # noqa: E402
from tools.bench_surface_recon import timed      # noqa: E402


def power():
    try:
        out = subprocess.run(['rocm-smi', '--showpower'], capture_output=True, text=True, timeout=30).stdout
        rows = [' '.join(l.split()) for l in out.splitlines() if 'GPU[0]' in l]
        return '; '.join(rows) if rows else 'not reported'
    except Exception as e:                                          # noqa: BLE001
        return f'not read ({type(e).__name__})'


def median_ms(fn, warmup=3, repeat=9):
    ts = []
    for it in range(warmup + repeat):
        t, r = timed(fn)
        if it >= warmup:
            ts.append(t)
    return float(np.median(ts)), min(ts), max(ts), r


def row(name, m, note=''):
    return f"  {name:<34}{m[0]:12.3f} ms  ({m[1]:.3f} .. {m[2]:.3f}){note}"


def torch_unique(v, f):
    u, inv = torch.unique(v, dim=0, return_inverse=True)
    return u, inv[f]


def numpy_round_trip(v, f):
    hv = v.cpu().numpy()
    u, inv = np.unique(hv, axis=0, return_inverse=True)
    return torch.from_numpy(u).to(v.device), torch.from_numpy(inv.reshape(-1)).to(v.device)[f]


def scipy_round_trip(v, tol):
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    from scipy.spatial import cKDTree
    hv = v.cpu().numpy().astype(np.float64)
    p = cKDTree(hv).query_pairs(tol, output_type='ndarray')
    n = len(hv)
    lab = connected_components(coo_matrix((np.ones(len(p), np.int8), (p[:, 0], p[:, 1])), shape=(n, n)), directed=False)[1]
    return torch.from_numpy(lab).to(v.device)


def soup(v, f):
    return np.ascontiguousarray(v[f.reshape(-1)]), np.arange(3 * len(f), dtype=np.int64).reshape(-1, 3)


def seam_sphere(n_lat=96, n_lon=192):
    """synthetic.uv_sphere written with a duplicated seam column: the last longitude strip names private copies of the meridian of longitude 0."""
    v, f, _ = synthetic.uv_sphere(n_lat, n_lon)
    f = f.copy()
    ring = lambda i: (i >= 1) & (i <= len(v) - 2)
    col = lambda i: (i - 1) % n_lon
    last = ((ring(f) & (col(f) == n_lon - 1)).any(1))[:, None] & ring(f) & (col(f) == 0)
    seam = 1 + n_lon * np.arange(n_lat - 1)
    copy = -np.ones(len(v), np.int64)
    copy[seam] = len(v) + np.arange(len(seam))
    f[last] = copy[f[last]]
    return np.concatenate([v, v[seam]]).astype(np.float32), f


def effect(name, v, f):
    def facts(v, f):
        try:
            charts = len(torch.unique(uv_unwrap(v, f, 1024, return_charts=True)[2]))
        except (PdhipError, ValueError) as e:
            charts = 'no (' + str(e)[:60] + ')'
        comps = mesh_components.label_components(f, n_vertices=v.shape[0], return_stats=True)[2]['count']
        try:
            spr.simplify_mesh(v, f, max(f.shape[0] // 4, 4))
            ok = 'accepted'
        except (PdhipError, ValueError) as e:
            ok = 'REFUSED (' + str(e).split(': ', 1)[-1][:90] + ')'
        rep = M.mesh_report(v, f)
        return (f"{v.shape[0]} vertices, {f.shape[0]} faces: {charts} charts, {comps} components, {rep['boundary_edges']} boundary edges, "
                f"simplify_mesh {ok}")
    cv, cf, cnt = M.clean_mesh(v, f, return_counts=True)
    return [f"mesh {name}", "  before: " + facts(v, f), "  after:  " + facts(cv, cf),
            f"  clean_mesh: {cnt['merged']} merged, {cnt['unreferenced']} unreferenced, {cnt['degenerate']} degenerate, {cnt['duplicate']} duplicate", ""]


def main(out_dir):
    dev = torch.device('cuda', torch.cuda.current_device())
    T = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    B = ["Welding and cleaning of supplied meshes on one MI355X (tools/bench_mesh_clean.py): HIP events round the whole call, 3 warm-up calls and the",
         "median of 9 (min .. max) for the device calls, 1 warm-up and the median of 3 for the host baselines, all in the same run.",
         f"device: {torch.cuda.get_device_name(dev)}; clocks after the run: CLOCKS; power after the run: POWER", "",
         "torch.unique's ordering differs (classes sorted by coordinate, not by smallest index) and it cleans no faces; it and the numpy round trip are",
         "baselines for tol = 0 only, the scipy round trip for tol > 0 only (up to 10^6 vertices).", ""]
    ratios = []
    for n in (32, 128, 256):
        iv, jf = synthetic.icosphere(n)
        sv, sf = soup(iv, jf)
        diag = float(np.linalg.norm(sv.max(0) - sv.min(0)))
        tol = 1e-4 * diag
        rng = np.random.default_rng(n)
        jv = (sv.astype(np.float64) + rng.uniform(-1.0, 1.0, sv.shape) * (0.4 * tol / np.sqrt(3.0))).astype(np.float32)
        for label, hv, t in (('tol = 0', sv, 0.0), (f'tol = 1e-4 diagonal = {tol:.3e}, jittered copies', jv, tol)):
            v, f = T(hv), T(sf)
            w = median_ms(lambda: M.weld_vertices(v, tolerance=t, return_counts=True))
            wc = w[3][1]
            B += [f"soup of icosphere({n}): {len(hv)} vertices, {len(sf)} faces, {label}: {wc['classes']} classes, {wc['cells_per_axis']} cells per axis, "
                  f"{wc['wide_queries']} wide queries", row('weld_vertices', w)]
            if len(hv) <= M.MAX_VERTICES_FACES:
                c = median_ms(lambda: M.clean_mesh(v, f, tolerance=t, return_counts=True))
                B += [row('clean_mesh', c, f"   -> {c[3][2]['vertices_after']} vertices, {c[3][2]['faces_after']} faces")]
            else:
                c = None
                B += [f"  clean_mesh                        refused: {len(hv)} vertices exceed 2^21 (three indices share one 64-bit sort key)"]
            if t == 0.0:
                tu = median_ms(lambda: torch_unique(v, f))
                nu = median_ms(lambda: numpy_round_trip(v, f), 1, 3)
                B += [row('torch.unique + gathers', tu, f"   = {tu[0] / w[0]:.2f} x weld_vertices" + (f", {tu[0] / c[0]:.2f} x clean_mesh" if c else '')),
                      row('numpy round trip (np.unique)', nu, f"   = {nu[0] / w[0]:.1f} x weld_vertices" + (f", {nu[0] / c[0]:.1f} x clean_mesh" if c else ''))]
                ratios.append((f"icosphere({n}) tol 0", tu[0] / w[0], nu[0] / w[0]))
            elif len(hv) <= 1000000:
                sc = median_ms(lambda: scipy_round_trip(v, t), 1, 3)
                B += [row('scipy round trip', sc, f"   = {sc[0] / w[0]:.1f} x weld_vertices")]
                ratios.append((f"icosphere({n}) tol > 0", None, sc[0] / w[0]))
            else:
                B += ["  scipy round trip                  not run (more than 10^6 vertices)"]
            B += [""]
            for line in B[-7:]:
                print(line, flush=True)
            del v, f
    B += ["crowd: n copies of one point, tol = 0 (one cell: every vertex scans every other, n^2 pair tests: the quadratic path, on record)"]
    last = 0.0
    for n in (10000, 30000, 100000):
        if last * (n / 30000.0) ** 2 > 20000.0:                    # (the step from 30 000 to 100 000 is 11 x: not started if that means over 20 s)
            B += [f"  n = {n}: not run: the n = 30000 row extrapolates to {last * (n / 30000.0) ** 2 / 1000.0:.0f} s"]
            continue
        crowd = T(np.tile(np.array([[0.25, 0.5, 0.75]], np.float32), (n, 1)))
        cw = median_ms(lambda: M.weld_vertices(crowd, return_counts=True), 1, 3)
        last = cw[0]
        B += [row(f'weld_vertices, n = {n}', cw, f"   {cw[3][1]['classes']} class, {cw[0] * 1e6 / (float(n) * n):.3f} ns per pair test")]
        print(B[-1], flush=True)
    B += [""]
    B += ["Effect of cleaning on the later stages (charts: the device unwrap at 1024; simplify_mesh to a quarter of the faces)", ""]
    iv, jf = synthetic.icosphere(32)
    sv, sf = soup(iv, jf)
    B += effect('icosphere(32) soup', T(sv), T(sf))
    ev, ef = seam_sphere()
    B += effect('uv_sphere(96, 192) with a duplicated seam column', T(ev), T(ef))
    B += ["Measured ratios (baseline / weld_vertices, medians of this run): "
          + '; '.join(f"{n}: " + (f"torch.unique {a:.2f} x, host {b:.1f} x" if a is not None else f"scipy {b:.1f} x") for n, a, b in ratios) + '.']
    B[2] = B[2].replace('CLOCKS', clocks()).replace('POWER', power())
    print('\n'.join(B[-12:]), flush=True)
    os.makedirs(out_dir, exist_ok=True)
    open(os.path.join(out_dir, 'mesh_clean_bench.txt'), 'w').write('\n'.join(B) + '\n')


if __name__ == '__main__':
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, 'profiles'))
