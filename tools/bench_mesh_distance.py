"""Times and parity of the point-to-mesh distance (csrc/mesh_distance.hip) on one MI355X -> profiles/mesh_distance_bench.txt and
profiles/mesh_distance_parity.txt.

  python tools/bench_mesh_distance.py [out_dir]      # out_dir: where the two files go (default: profiles/)

Workload: 100 000 float32 points against
  sphere 9 680      synthetic.icosphere(22, noise=0.01, seed=1), the sphere of the other benches
  sphere 200 000    synthetic.icosphere(100, noise=0.01, seed=1)
  box 12            the cube [-0.5, 0.5]^3
  SPR torus         recon_one_shape_SPR at depth 6 of 30 000 points of the torus
with two point sets each: `uniform`, the [-0.55, 0.55]^3 points of the occupancy bench, and `surface`, 100 000 points on the surface of a SECOND mesh
or solid (the evaluation's own use: a ground-truth cloud against a predicted mesh): samples of the same sphere with another noise seed for the two
spheres, of the 9 680-face sphere for the box, of the analytic torus for the reconstruction.
Per case, HIP events round the whole call (its one stream synchronisation and host read included).  The shipped path, path 1 (every face on the large
list) and path 2 (every query to the all-faces scan) of pdhip_debug_set_closest_on_mesh are timed in the same run, alternating, one call of each per
round: 3 warm-up rounds and the median of 15 (min .. max) up to 20 000 faces, 1 warm-up round and the median of 5 beyond.
  torch all pairs   the same definition in float64 torch ops on the same device, every point against every face, in chunks of points of at most
                    2^24 pairs; after a warm-up on 2 000 points it runs ONCE (at 200 000 faces one run takes tens of seconds), and that run's
                    output is what the parity is checked against
  numpy oracle      tests/mesh_distance_common.py:oracle_closest on the host, once, on the first 10 000 points against the 12-face box: for context
Recorded per case: counts (certified by the ring scan, finished by the all-faces scan, faces on the large list, degenerate faces) and the share of the
large list.  Parity: d2 bit for bit and the face against the torch evaluation at full size (torch.min promises no order among equal values, so a face
that differs is looked at again: it must attain the same d2, and the kernel's must be the smaller index), closest against the face it names."""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)
from pointdreamer_amd import _lib, synthetic, spr, geometry_metrics as G      # noqa: E402
from tools.bench_geometry_metrics import clocks, WARMUP, REPEAT      # noqa: E402
from tools.bench_surface_recon import timed      # noqa: E402
import mesh_distance_common as md      # noqa: E402
import occupancy_common as oc      # noqa: E402

N = 100000
PAIRS = 1 << 24


def _dot(u, w):
    return (u[..., 0] * w[..., 0] + u[..., 1] * w[..., 1]) + u[..., 2] * w[..., 2]


def torch_closest(vertices, faces, points):
    """(d2, face) of the all-pairs evaluation of include/pdhip.h's definition in float64 torch ops (one kernel per operation: no contraction)."""
    v, p = vertices.double(), points.double()
    a, b, c = v[faces[:, 0]], v[faces[:, 1]], v[faces[:, 2]]
    ab, ac = b - a, c - a
    nx = ab[:, 1] * ac[:, 2] - ab[:, 2] * ac[:, 1]
    ny = ab[:, 2] * ac[:, 0] - ab[:, 0] * ac[:, 2]
    nz = ab[:, 0] * ac[:, 1] - ab[:, 1] * ac[:, 0]
    index = torch.nonzero(~((nx == 0) & (ny == 0) & (nz == 0))).reshape(-1)
    a, b, c = a[index][None], b[index][None], c[index][None]
    ab, ac, bc = b - a, c - a, c - b
    d2 = torch.empty((p.shape[0],), dtype=torch.float64, device=p.device)
    face = torch.empty((p.shape[0],), dtype=torch.int64, device=p.device)
    chunk = max(1, PAIRS // max(1, index.shape[0]))
    inf = torch.tensor(float('inf'), dtype=torch.float64, device=p.device)
    for s in range(0, p.shape[0], chunk):
        q = p[s:s + chunk, None, :]
        d1, dd2 = _dot(ab, q - a), _dot(ac, q - a)
        d3, d4 = _dot(ab, q - b), _dot(ac, q - b)
        d5, d6 = _dot(ab, q - c), _dot(ac, q - c)
        vc, vb, va, e43, e56 = d1 * d4 - d3 * dd2, d5 * dd2 - d1 * d6, d3 * d6 - d5 * d4, d4 - d3, d5 - d6
        den = 1.0 / ((va + vb) + vc)
        x = (a + ab * (vb * den)[..., None]) + ac * (vc * den)[..., None]
        x = torch.where(((va <= 0) & (e43 >= 0) & (e56 >= 0))[..., None], b + (e43 / (e43 + e56))[..., None] * bc, x)
        x = torch.where(((vb <= 0) & (dd2 >= 0) & (d6 <= 0))[..., None], a + (dd2 / (dd2 - d6))[..., None] * ac, x)
        x = torch.where(((d6 >= 0) & (d5 <= d6))[..., None], c, x)
        x = torch.where(((vc <= 0) & (d1 >= 0) & (d3 <= 0))[..., None], a + (d1 / (d1 - d3))[..., None] * ab, x)
        x = torch.where(((d3 >= 0) & (d4 <= d3))[..., None], b, x)
        x = torch.where(((d1 <= 0) & (dd2 <= 0))[..., None], a, x)
        val = _dot(q - x, q - x)
        val = torch.where(torch.isnan(val), inf, val)
        m, j = val.min(dim=1)
        d2[s:s + chunk], face[s:s + chunk] = m, index[j]
    return d2, face


def same_bytes(xs, ys):
    return all(torch.equal(x.contiguous().view(torch.uint8), y.contiguous().view(torch.uint8)) for x, y in zip(xs, ys))


def per_face_d2(vertices, faces, points, face):
    """The definition's value of point q on face[q], through the oracle, one pair each (host)."""
    v, f, p = vertices.cpu().numpy(), faces.cpu().numpy(), points.cpu().numpy()
    out = np.empty(len(p))
    for k in range(len(p)):
        out[k] = md.oracle_closest(v, f[face[k]:face[k] + 1], p[k:k + 1])[0][0]
    return out


def main(out_dir):
    L = _lib.lib()
    dev = torch.device('cuda', torch.cuda.current_device())
    T = lambda x: torch.from_numpy(np.array(x)).to(dev)
    uniform = T(oc.uniform_points(N, 7))
    xyz, rgb, nrm = synthetic.solid('torus').sample(30000, seed=1)
    sv, sf, _ = spr.recon_one_shape_SPR(xyz, rgb, gt_normals=nrm, depth=6)
    s1v, s1f = map(T, synthetic.icosphere(22, noise=0.01, seed=1))
    s2v, s2f = map(T, synthetic.icosphere(100, noise=0.01, seed=1))
    surf1 = G.sample_mesh_cloud(*map(T, synthetic.icosphere(22, noise=0.01, seed=2)), N, seed=3)[0]
    surf2 = G.sample_mesh_cloud(*map(T, synthetic.icosphere(100, noise=0.01, seed=2)), N, seed=3)[0]
    surf_box = G.sample_mesh_cloud(s1v, s1f, N, seed=4)[0]
    surf_torus = T(synthetic.solid('torus').sample(N, seed=3)[0].astype(np.float32))
    bv, bf = map(T, oc.box_mesh())
    cases = [('sphere 9 680', s1v, s1f, surf1, 0), ('sphere 200 000', s2v, s2f, surf2, 0), ('box 12', bv, bf, surf_box, 10000),
             ('SPR torus depth 6', sv.float().contiguous(), sf.long().contiguous(), surf_torus, 0)]
    B = [f"Point-to-mesh distance on one MI355X (tools/bench_mesh_distance.py): {N} float32 points per case; HIP events round the whole call;",
         f"shipped path, path 1 and path 2 alternate in one run: {WARMUP} warm-up rounds and the median of {REPEAT} (min .. max) up to 20 000 faces, "
         "1 and 5 beyond; the torch baseline runs once after a warm-up on 2 000 points.",
         f"device: {torch.cuda.get_device_name(dev)}; clocks after the run: CLOCKS", ""]
    P = ["Parity of the point-to-mesh distance (tools/bench_mesh_distance.py).", ""]
    verdict = []
    for name, v, f, surface, n_host in cases:
        F = f.shape[0]
        for pname, points in (('uniform', uniform), ('surface', surface)):
            d2, face, closest, counts = G.closest_on_mesh(v, f, points, return_closest=True, return_counts=True)
            counts = counts.cpu().tolist()
            rounds = (WARMUP, REPEAT) if F <= 20000 else (1, 5)
            ts = {0: [], 1: [], 2: []}
            same = {1: True, 2: True}
            for it in range(sum(rounds)):
                for path in (0, 1, 2):
                    old = L.pdhip_debug_set_closest_on_mesh(0, path)
                    try:
                        t, out = timed(lambda: G.closest_on_mesh(v, f, points, return_closest=True))
                        if path and it == 0:
                            same[path] = same_bytes(out, (d2, face, closest))
                    finally:
                        L.pdhip_debug_set_closest_on_mesh(old // 4, old % 4)
                    if it >= rounds[0]:
                        ts[path].append(t)
            med = {k: (float(np.median(x)), min(x), max(x)) for k, x in ts.items()}
            torch_closest(v, f, points[:2000])
            base, (want_d2, want_face) = timed(lambda: torch_closest(v, f, points))
            again = G.closest_on_mesh(v, f, points, return_closest=True)
            bits = int((d2.view(torch.int64) != want_d2.view(torch.int64)).sum())
            differ = torch.nonzero(face.long() != want_face).reshape(-1).cpu().numpy()
            tie_note = ''
            if len(differ):
                mine_f, torch_f = face.cpu().numpy()[differ], want_face.cpu().numpy()[differ]
                at = per_face_d2(v, f, points[differ], torch_f)
                ties = int((at.view(np.uint64) == d2.cpu().numpy()[differ].view(np.uint64)).sum())
                tie_note = f" ({ties} of them true ties: torch's face attains the same d2 bits; the kernel's index is the smaller in {int((mine_f < torch_f).sum())})"
            r = points.double() - closest
            self_d2 = (r[:, 0] * r[:, 0] + r[:, 1] * r[:, 1]) + r[:, 2] * r[:, 2]
            wins = med[0][0] < base
            verdict.append((name, pname, wins))
            B += [f"case {name}, {pname} points: {F} faces; counts {counts}: large list {counts[2]} of {F} faces = {100.0 * counts[2] / F:.2f} %, "
                  f"{counts[0]} queries certified by the ring scan, {counts[1]} by the all-faces scan",
                  f"  closest_on_mesh, shipped (whole call) {med[0][0]:10.3f} ms  ({med[0][1]:.3f} .. {med[0][2]:.3f})",
                  f"    path 1: every face large            {med[1][0]:10.3f} ms  ({med[1][1]:.3f} .. {med[1][2]:.3f})   = {med[1][0] / med[0][0]:.2f} x the shipped path",
                  f"    path 2: every query, all faces      {med[2][0]:10.3f} ms  ({med[2][1]:.3f} .. {med[2][2]:.3f})   = {med[2][0] / med[0][0]:.2f} x the shipped path",
                  f"  torch all pairs, f64 (one run)        {base:10.3f} ms   = {base / med[0][0]:.2f} x the shipped path's time"
                  + ('' if wins else '   ** the shipped path LOSES to the baseline here **')]
            P += [f"case {name}, {pname} points ({F} faces, {N} points):",
                  f"  against the torch all-pairs evaluation: d2 bits differ at {bits} of {N} points, the face at {len(differ)}{tie_note}",
                  f"  |q - closest|^2 recomputed from closest: bits differ at {int((self_d2.view(torch.int64) != d2.view(torch.int64)).sum())} of {N}",
                  f"  path 1 and path 2 against the shipped path: bytes {'EQUAL' if same[1] and same[2] else 'DIFFER'}; two calls give "
                  f"{'EQUAL' if same_bytes(again, (d2, face, closest)) else 'DIFFERENT'} bytes"]
            if n_host and pname == 'uniform':
                t0 = time.perf_counter()
                host = md.oracle_closest(v.cpu().numpy(), f.cpu().numpy(), points[:n_host].cpu().numpy())
                ms = (time.perf_counter() - t0) * 1e3
                B.append(f"  numpy oracle (host, once)             {ms:10.1f} ms  for the first {n_host} points")
                P.append(f"  against the numpy oracle on the first {n_host} points: d2 bits differ at "
                         f"{int((d2[:n_host].cpu().numpy().view(np.uint64) != host[0].view(np.uint64)).sum())}, the face at "
                         f"{int((face[:n_host].cpu().numpy() != host[1]).sum())}, closest at "
                         f"{int((closest[:n_host].cpu().numpy().view(np.uint64) != host[2].view(np.uint64)).any(axis=1).sum())}")
            B.append("")
            P.append("")
            for line in B[-8:] + P[-6:]:
                print(line, flush=True)
    lost = [f"{n}, {p}" for n, p, w in verdict if not w]
    B += ["The shipped path is faster than the all-pairs torch baseline of the same run in every case." if not lost else
          "The shipped path LOSES to the all-pairs torch baseline in: " + '; '.join(lost) + '.']
    B[2] = B[2].replace('CLOCKS', clocks())
    os.makedirs(out_dir, exist_ok=True)
    open(os.path.join(out_dir, 'mesh_distance_bench.txt'), 'w').write('\n'.join(B) + '\n')
    open(os.path.join(out_dir, 'mesh_distance_parity.txt'), 'w').write('\n'.join(P) + '\n')


if __name__ == '__main__':
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, 'profiles'))
