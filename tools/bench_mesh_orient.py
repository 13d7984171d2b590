"""Times and effect of orienting supplied meshes (csrc/mesh_orient.hip) on one MI355X -> profiles/mesh_orient_bench.txt.

  python tools/bench_mesh_orient.py [out_dir]      # out_dir: where the file goes (default: profiles/)
  python tools/bench_mesh_orient.py --one N        # synthetic.icosphere(N), half flipped: 3 + 9 calls of orient_faces and nothing else, for
                                                   #   `rocprofv3 --kernel-trace --stats -- python tools/bench_mesh_orient.py --one 128`

Speed.  synthetic.icosphere(32 / 128 / 256): 20 480 / 327 680 / 1 310 720 faces with a random half of the faces flipped, and the 327 680-face one as a
soup welded by clean_mesh first; on the device before the clock starts.  HIP events round the whole call, its stream synchronisation and host read
included: 3 warm-up calls and the median of 9 (min .. max) for the device call, 1 warm-up and the median of 3 for the host baselines.
  orient_faces                    the entry of pointdreamer_amd/mesh_orient.py
  numpy / scipy round trip        faces and vertices to the host, the half-edge table by a stable argsort, patches by csgraph.connected_components,
                                  rel by csgraph.dijkstra from every root over weights 1 (the two faces disagree) / 2 (agree), read modulo 2, the
                                  outward choice by the f64 signed volume per patch, the faces back.  It equals orient_faces on these closed meshes
                                  (checked in the run) but is not the bit-exact definition: tests/mesh_orient_common.py is
  trimesh.repair.fix_normals      when `import trimesh` works on the machine; otherwise the file says that it was absent
Effect.  The flipped icosphere(32) before and after orient_faces: charts of the device unwrap, and whether simplify_mesh accepts the mesh."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from pointdreamer_amd import mesh_clean, mesh_orient as M, spr, synthetic      # noqa: E402
from pointdreamer_amd._lib import PdhipError      # noqa: E402
from pointdreamer_amd.extract_texture_map import uv_unwrap      # noqa: E402
from tools.bench_geometry_metrics import clocks      # noqa: E402
from tools.bench_mesh_clean import median_ms, power, row, soup      # noqa: E402


def half_flipped(f, seed):
    g = f.copy()
    m = np.random.default_rng(seed).random(len(f)) < 0.5
    g[m] = g[m][:, [0, 2, 1]]
    return g, m


def host_round_trip(v, f):
    """The numpy / scipy path of the module docstring -> oriented faces on the device."""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components, dijkstra
    hv, hf = v.cpu().numpy().astype(np.float64), f.cpu().numpy()
    F, Vn = len(hf), len(hv)
    a, b = hf.reshape(-1), hf[:, [1, 2, 0]].reshape(-1)
    key = np.minimum(a, b) * np.int64(Vn) + np.maximum(a, b)
    o = np.argsort(key, kind='stable')
    face, d, key = (np.arange(3 * F) // 3)[o], (a > b)[o], key[o]
    _, start, cnt = np.unique(key, return_index=True, return_counts=True)
    m = start[cnt == 2]
    fa, fb, w = face[m], face[m + 1], 2.0 - (d[m] == d[m + 1])
    g = coo_matrix((w, (fa, fb)), shape=(F, F)).tocsr()
    P, lab = connected_components(g, directed=False)
    roots = np.full(P, F, np.int64)
    np.minimum.at(roots, lab, np.arange(F))
    dist = dijkstra(g, directed=False, indices=roots, min_only=True)
    rel = dist.astype(np.int64) & 1
    x = hv[hf]
    vol6 = np.einsum('ij,ij->i', x[:, 0], np.cross(x[:, 1], x[:, 2])) * (1 - 2 * rel)
    comp = np.bincount(lab, weights=vol6, minlength=P) < 0
    flip = (rel ^ comp[lab]).astype(bool)
    out = hf.copy()
    out[flip] = hf[flip][:, [0, 2, 1]]
    return torch.from_numpy(out).to(f.device)


def trimesh_fix(v, f):
    import trimesh
    mesh = trimesh.Trimesh(v.cpu().numpy(), f.cpu().numpy(), process=False)
    trimesh.repair.fix_normals(mesh)
    return torch.from_numpy(np.asarray(mesh.faces, np.int64)).to(f.device)


def facts(v, f):
    try:
        charts = len(torch.unique(uv_unwrap(v, f, 1024, return_charts=True)[2]))
    except (PdhipError, ValueError) as e:
        charts = 'no (' + str(e)[:60] + ')'
    try:
        spr.simplify_mesh(v, f, max(f.shape[0] // 4, 4))
        ok = 'accepted'
    except (PdhipError, ValueError) as e:
        ok = 'REFUSED (' + str(e).split(': ', 1)[-1][:90] + ')'
    rep = M.orientation_report(v, f)
    return (f"{f.shape[0]} faces: {charts} charts, simplify_mesh {ok}; report: would_flip {rep['would_flip']}, incoherent_edges "
            f"{rep['incoherent_edges']}, closed_patches {rep['closed_patches']} of {rep['patches']}")


def one(n):
    dev = torch.device('cuda', torch.cuda.current_device())
    v, f = synthetic.icosphere(n)
    g, _ = half_flipped(f, n)
    tv, tg = torch.from_numpy(v).to(dev), torch.from_numpy(g).to(dev)
    for _ in range(12):
        out = M.orient_faces(tv, tg)
    torch.cuda.synchronize()
    assert out.cpu().numpy().tobytes() == f.tobytes()
    print(f'icosphere({n}): {len(f)} faces, 12 calls of orient_faces')


def main(out_dir):
    dev = torch.device('cuda', torch.cuda.current_device())
    T = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    try:
        import trimesh      # noqa: F401
        have_trimesh = True
    except ImportError:
        have_trimesh = False
    B = ["Orientation of supplied meshes on one MI355X (tools/bench_mesh_orient.py): HIP events round the whole call, 3 warm-up calls and the median of 9",
         "(min .. max) for the device call, 1 warm-up and the median of 3 for the host baselines, all in the same run.",
         f"device: {torch.cuda.get_device_name(dev)}; clocks after the run: CLOCKS; power after the run: POWER", "",
         "trimesh: " + ("present: trimesh.repair.fix_normals is timed below" if have_trimesh else
                        "ABSENT on this machine (import trimesh fails): no trimesh.repair.fix_normals row"), ""]
    ratios = []
    cases = [(f'icosphere({n})', n, False) for n in (32, 128, 256)] + [('icosphere(128) as a soup welded by clean_mesh', 128, True)]
    for name, n, welded in cases:
        iv, jf = synthetic.icosphere(n)
        g, m = half_flipped(jf, n)
        if welded:
            sv, sf = soup(iv, g)
            v, f = mesh_clean.clean_mesh(T(sv), T(sf))
            truth = None
        else:
            v, f, truth = T(iv), T(g), jf
        d = median_ms(lambda: M.orient_faces(v, f, return_counts=True))
        c = d[3][1]
        h = median_ms(lambda: host_round_trip(v, f), 1, 3)
        same = bool((d[3][0] == h[3]).all())
        exact = '' if truth is None else f", equals the unflipped icosphere: {d[3][0].cpu().numpy().tobytes() == truth.tobytes()}"
        B += [f"{name}: {v.shape[0]} vertices, {f.shape[0]} faces, {int(m.sum())} flipped: {c['patches']} patch(es), {c['flipped']} faces flipped back, "
              f"{c['incoherent_edges']} incoherent edges before{exact}",
              row('orient_faces', d),
              row('numpy / scipy round trip', h, f"   = {h[0] / d[0]:.1f} x orient_faces; same faces: {same}")]
        ratios.append((name, h[0] / d[0]))
        if have_trimesh:
            t = median_ms(lambda: trimesh_fix(v, f), 1, 3)
            B += [row('trimesh.repair.fix_normals', t, f"   = {t[0] / d[0]:.1f} x orient_faces; same faces: {bool((d[3][0] == t[3]).all())}")]
        B += [""]
        for line in B[-5:]:
            print(line, flush=True)
        del v, f
    B += ["Effect of orienting on the later stages (charts: the device unwrap at 1024; simplify_mesh to a quarter of the faces)", ""]
    iv, jf = synthetic.icosphere(32)
    g, _ = half_flipped(jf, 32)
    v, f = T(iv), T(g)
    B += ["mesh icosphere(32), a random half of the faces flipped", "  before: " + facts(v, f), "  after:  " + facts(v, M.orient_faces(v, f)), ""]
    B += ["Measured ratios (host round trip / orient_faces, medians of this run): " + '; '.join(f"{n}: {r:.1f} x" for n, r in ratios) + '.']
    B[2] = B[2].replace('CLOCKS', clocks()).replace('POWER', power())
    print('\n'.join(B[-8:]), flush=True)
    os.makedirs(out_dir, exist_ok=True)
    open(os.path.join(out_dir, 'mesh_orient_bench.txt'), 'w').write('\n'.join(B) + '\n')


if __name__ == '__main__':
    if len(sys.argv) > 2 and sys.argv[1] == '--one':
        one(int(sys.argv[2]))
    else:
        main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, 'profiles'))
