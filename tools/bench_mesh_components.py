"""Times of the connected-component labelling and of the removal of small pieces (csrc/mesh_components.hip) on one MI355X ->
profiles/mesh_components_bench.txt.

  python tools/bench_mesh_components.py [out_dir]      # out_dir: where the file goes (default: profiles/)

Meshes, all on the device before the clock starts:
  two_spheres depth 6      the reconstruction of tests/test_gpu_mesh_components.py (25 000 points of synthetic.solid('two_spheres'), spr depth 6):
                           two closed components, 6 896 faces (the spheres have radius 0.2: the small end, where launches and the two
                           stream synchronisations are the cost)
  sphere + 1000 blobs      synthetic.icosphere(220) (968 000 faces) and 1 000 icosahedra of radius 0.002 around it (20 faces each), the blobs' vertex
                           ranges and faces placed at random positions among the sphere's: about one million faces, 1 001 components
  the same, shuffled       that mesh with its faces in random order (no two neighbouring threads on neighbouring faces)
  the same, relabelled     the shuffled mesh with its vertex indices randomly permuted as well: no locality left in the numbering, the first forest
                           of k_mc_hook is tens of thousands of small trees and k_mc_union does the work
Per mesh HIP events round the whole call -- its one stream synchronisation and host read included: 3 warm-up calls and the median of 15 (min .. max):
  label_components         vertex_comp, face_comp, per-component root / counts / boxes
  filter_components        keep='largest': labelling, selection (torch ops on the C components), compaction
  host round trip          the baseline, timed the same way in the same run: faces and vertices to the host, scipy.sparse.csgraph
                           connected_components on the edge graph (what mesh_checks.components_euler builds), the largest component by face count,
                           mask + re-index in numpy, vertices and faces back to the device
The one condition: at every mesh the device's filter_components is faster than the host round trip, both medians from this run.  The output of
the two is compared as well (the same vertices and faces)."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from pointdreamer_amd import mesh_components as M, spr, synthetic      # noqa: E402
from tools.bench_geometry_metrics import clocks      # noqa: E402
from tools.bench_surface_recon import timed      # noqa: E402

WARMUP, REPEAT = 3, 15


def host_round_trip(v, f):
    """The baseline: (vertices, faces) of the component with the most faces (the smaller root on a tie), computed on the host."""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    hv, hf = v.cpu().numpy(), f.cpu().numpy()
    n = len(hv)
    a = np.concatenate([hf[:, 0], hf[:, 1]])
    b = np.concatenate([hf[:, 1], hf[:, 2]])
    _, lab = connected_components(coo_matrix((np.ones(len(a), np.int8), (a, b)), shape=(n, n)), directed=False)
    fl = lab[hf[:, 0]]
    nf = np.bincount(fl)
    best = np.flatnonzero(nf == nf.max())
    first = np.full(len(nf), n, np.int64)
    np.minimum.at(first, lab, np.arange(n))
    keep = fl == best[np.argmin(first[best])]
    used = np.zeros(n, bool)
    used[hf[keep].reshape(-1)] = True
    new = np.cumsum(used) - 1
    return torch.from_numpy(hv[used]).to(v.device), torch.from_numpy(new[hf[keep]]).to(v.device)


def median_ms(fn):
    ts = []
    for it in range(WARMUP + REPEAT):
        t, r = timed(fn)
        if it >= WARMUP:
            ts.append(t)
    return float(np.median(ts)), min(ts), max(ts), r


def big_mesh(seed=0):
    rng = np.random.default_rng(seed)
    sv, sf = synthetic.icosphere(220)
    bv, bf = synthetic.icosphere(1, radius=0.002)
    d = rng.standard_normal((1000, 3))
    d = (0.6 * d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    # vertex ranges: the sphere's vertices cut at 1 000 random places, one blob's 12 vertices in every cut
    cuts = np.sort(rng.integers(0, len(sv) + 1, 1000))
    new_of_sphere = np.arange(len(sv)) + 12 * np.searchsorted(cuts, np.arange(len(sv)), side='right')
    blob_base = cuts + 12 * np.arange(1000)
    V = len(sv) + 12000
    v = np.empty((V, 3), np.float32)
    v[new_of_sphere] = sv
    for k in range(1000):
        v[blob_base[k]:blob_base[k] + 12] = bv + d[k]
    faces = [new_of_sphere[sf]] + [bf + blob_base[k] for k in range(1000)]
    f = np.concatenate(faces)
    # faces: the blobs' faces at random positions among the sphere's, the sphere's own order kept
    pos = np.argsort(np.concatenate([np.arange(len(sf), dtype=np.float64), rng.random(20000) * len(sf)]), kind='stable')
    return v, np.ascontiguousarray(f[pos])


def main(out_dir):
    dev = torch.device('cuda', torch.cuda.current_device())
    T = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    xyz, rgb, _ = synthetic.solid('two_spheres').sample(25000, seed=1)
    xyz = T(xyz)
    mv, mf = spr.poisson_reconstruct(xyz, spr.estimate_normals(xyz), depth=6)
    bv, bf = big_mesh()
    shuffled = bf[np.random.default_rng(1).permutation(len(bf))]
    perm = np.random.default_rng(2).permutation(len(bv))
    pv = np.empty_like(bv)
    pv[perm] = bv
    cases = [('two_spheres depth 6', mv, mf), ('sphere + 1000 blobs', T(bv), T(bf)), ('the same, shuffled', T(bv), T(shuffled)),
             ('the same, relabelled', T(pv), T(perm[shuffled]))]
    B = ["Connected components and the removal of small pieces on one MI355X (tools/bench_mesh_components.py): HIP events round the whole call,",
         f"{WARMUP} warm-up calls and the median of {REPEAT} (min .. max); the host round trip is timed the same way in the same run.",
         f"device: {torch.cuda.get_device_name(dev)}; clocks after the run: CLOCKS", ""]
    verdict = []
    for name, v, f in cases:
        lab, llo, lhi, (_, _, st) = median_ms(lambda: M.label_components(f, vertices=v, return_stats=True))
        fil, flo, fhi, (gv, gf, cnt) = median_ms(lambda: M.filter_components(v, f, keep='largest', return_counts=True))
        host, hlo, hhi, (hv, hf) = median_ms(lambda: host_round_trip(v, f))
        same = torch.equal(gv, hv) and torch.equal(gf, hf)
        verdict.append((name, fil < host and lab < host, host / fil, same))
        B += [f"mesh {name}: {v.shape[0]} vertices, {f.shape[0]} faces, {st['count']} components ({st['unreferenced']} unreferenced vertices); largest: "
              f"{cnt['faces_after']} faces, {cnt['vertices_after']} vertices",
              f"  label_components (with boxes)        {lab:10.3f} ms  ({llo:.3f} .. {lhi:.3f})",
              f"  filter_components(keep='largest')    {fil:10.3f} ms  ({flo:.3f} .. {fhi:.3f})",
              f"  host round trip (scipy + numpy)      {host:10.3f} ms  ({hlo:.3f} .. {hhi:.3f})   = {host / fil:.1f} x the device call"
              + ('' if fil < host else '   ** the device call LOSES to the baseline here **'),
              f"  the two results are {'the SAME mesh (vertices bit for bit, faces exactly)' if same else 'DIFFERENT'}", ""]
        for line in B[-6:]:
            print(line, flush=True)
    lost = [name for name, w, _, _ in verdict if not w]
    B += ["The device calls are faster than the host round trip of the same run at every mesh: "
          + ', '.join(f"{r:.1f} x at {name}" for name, _, r, _ in verdict) + '.' if not lost else "The device call LOSES to the host round trip at: " + '; '.join(lost) + '.']
    if not all(s for _, _, _, s in verdict):
        B += ["The device's result DIFFERS from the host's at: " + '; '.join(name for name, _, _, s in verdict if not s) + '.']
    B[2] = B[2].replace('CLOCKS', clocks())
    print(B[-1], flush=True)
    os.makedirs(out_dir, exist_ok=True)
    open(os.path.join(out_dir, 'mesh_components_bench.txt'), 'w').write('\n'.join(B) + '\n')


def one_call():
    """The workload of a kernel trace: the large mesh labelled and filtered three times, nothing else."""
    dev = torch.device('cuda', torch.cuda.current_device())
    bv, bf = big_mesh()
    v, f = torch.from_numpy(bv).to(dev), torch.from_numpy(bf).to(dev)
    for _ in range(3):
        _, _, st = M.label_components(f, vertices=v, return_stats=True)
        gv, gf, cnt = M.filter_components(v, f, keep='largest', return_counts=True)
    torch.cuda.synchronize()
    print('one call:', st['count'], 'components;', cnt)


if __name__ == '__main__':
    if len(sys.argv) > 1 and sys.argv[1] == '--one-call':
        one_call()
        sys.exit(0)
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, 'profiles'))
