"""Times of the Taubin smoothing (csrc/mesh_smooth.hip) on one MI355X -> profiles/mesh_smooth_bench.txt.

  python tools/bench_mesh_smooth.py [out_dir]      # out_dir: where the file goes (default: profiles/)

Meshes, all on the device before the clock starts:
  torus depth 6, depth 8   the reconstruction of 30 000 points of synthetic.solid('torus') (noise 0.005 along the normal) at spr depth 6 and 8
  sphere + 1000 blobs      the 988 000-face mesh of tools/bench_mesh_components.py
Per mesh HIP events round each call, 3 warm-up calls and the median of 15 (min .. max); 10 steps of lambda 0.5, mu -0.53 (20 passes):
  neighbour_csr            mesh_utils.neighbour_csr: the CSR both entries work on (its own stream synchronisation included)
  boundary pass            pdhip_mesh_boundary_vertices on that CSR (3 launches, one synchronisation)
  smoothing, 10 steps      pdhip_smooth_mesh on that CSR and the boundary mask, buffers allocated before the clock: 1 + 20 launches, one synchronisation
  taubin_smooth            the public call: all of the above and its allocations
  (a) torch.sparse         the same definition as f64 CSR products on the same device: per pass m = (A x) / degree, x += s (m - x), held rows put back;
                           A (ones on the CSR) and the degrees built before the clock, f32 -> f64 and the rounding to f32 inside it
  (b) scipy on the host    vertices and the CSR to the host, scipy.sparse.csr_matrix products in f64, the result back to the device
The baselines sum each row in their own order, so their results are compared with the device's by the largest difference, not by bytes."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from pointdreamer_amd import _lib, mesh_smooth as M, mesh_utils, spr, synthetic      # noqa: E402
from pointdreamer_amd._lib import ptr, stream      # noqa: E402
from tools.bench_geometry_metrics import clocks      # noqa: E402
from tools.bench_mesh_components import big_mesh, median_ms      # noqa: E402

STEPS, LAM, MU = 10, 0.5, -0.53


def raw_smooth(v, rowptr, colidx, held, state, out, counts):
    rc = _lib.lib().pdhip_smooth_mesh(ptr(v), v.shape[0], ptr(rowptr), ptr(colidx), ptr(held), STEPS, LAM, MU, ptr(state[0]), ptr(state[1]), ptr(out),
                                      ptr(counts), stream())
    assert rc == 0, _lib.lib().pdhip_last_error()
    return out


def torch_sparse(v, A, deg, held):
    x0 = v.double()
    x = x0
    for _ in range(STEPS):
        for s in (LAM, MU):
            m = torch.sparse.mm(A, x) / deg
            x = torch.where(held, x0, x + s * (m - x))
    return x.float()


def scipy_host(v, rowptr, colidx, held):
    from scipy.sparse import csr_matrix
    hv, rp, ci, hh = v.cpu().numpy(), rowptr.cpu().numpy(), colidx.cpu().numpy(), held.cpu().numpy().astype(bool)
    n = len(hv)
    A = csr_matrix((np.ones(len(ci)), ci, rp), shape=(n, n))
    deg = np.maximum(np.diff(rp), 1).astype(np.float64)[:, None]
    stay = (hh | (np.diff(rp) == 0))[:, None]
    x0 = hv.astype(np.float64)
    x = x0
    for _ in range(STEPS):
        for s in (LAM, MU):
            m = (A @ x) / deg
            x = np.where(stay, x0, x + s * (m - x))
    return torch.from_numpy(x.astype(np.float32)).to(v.device)


def main(out_dir):
    dev = torch.device('cuda', torch.cuda.current_device())
    T = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    xyz = T(synthetic.solid('torus').sample(30000, seed=1, noise=0.005)[0])
    nrm = spr.estimate_normals(xyz)
    cases = [(f'torus depth {d}',) + spr.poisson_reconstruct(xyz, nrm, depth=d) for d in (6, 8)]
    bv, bf = big_mesh()
    cases.append(('sphere + 1000 blobs', T(bv), T(bf)))
    B = [f"Taubin smoothing on one MI355X (tools/bench_mesh_smooth.py): {STEPS} steps of lambda {LAM}, mu {MU} = {2 * STEPS} passes; HIP events round each call,",
         "3 warm-up calls and the median of 15 (min .. max); the baselines are timed the same way in the same run.",
         f"device: {torch.cuda.get_device_name(dev)}; clocks after the run: CLOCKS", ""]
    for name, v, f in cases:
        Vn = v.shape[0]
        csr, clo, chi, (rowptr, colidx) = median_ms(lambda: mesh_utils.neighbour_csr(Vn, f))
        colidx = colidx.contiguous()
        bnd, blo, bhi, (held, bc) = median_ms(lambda: M._boundary(f, Vn, rowptr, colidx))
        state = torch.empty((2, Vn, 4), dtype=torch.float64, device=dev)
        out, counts = torch.empty_like(v), torch.empty((4,), dtype=torch.int32, device=dev)
        sm, slo, shi, got = median_ms(lambda: raw_smooth(v, rowptr, colidx, held, state, out, counts))
        got = got.clone()
        pub, plo, phi, whole = median_ms(lambda: M.taubin_smooth(v, f, steps=STEPS, lam=LAM, mu=MU))
        assert torch.equal(whole, got)
        B += [f"mesh {name}: {Vn} vertices, {f.shape[0]} faces, {colidx.shape[0]} neighbour pairs; {bc.tolist()[0]} boundary vertices; counts {counts.tolist()}",
              f"  neighbour_csr                         {csr:10.3f} ms  ({clo:.3f} .. {chi:.3f})",
              f"  boundary pass                         {bnd:10.3f} ms  ({blo:.3f} .. {bhi:.3f})",
              f"  smoothing, {STEPS} steps ({1 + 2 * STEPS} launches)       {sm:10.3f} ms  ({slo:.3f} .. {shi:.3f})   = {1e3 * sm / (1 + 2 * STEPS):.1f} us per launch",
              f"  taubin_smooth (the public call)       {pub:10.3f} ms  ({plo:.3f} .. {phi:.3f})"]
        hb = held.view(torch.bool)
        try:
            deg = (rowptr[1:] - rowptr[:-1]).double()
            A = torch.sparse_csr_tensor(rowptr.long(), colidx.long(), torch.ones(colidx.shape[0], dtype=torch.float64, device=dev), size=(Vn, Vn))
            stay = (hb | (deg == 0))[:, None]
            ta, alo, ahi, ra = median_ms(lambda: torch_sparse(v, A, deg.clamp(min=1)[:, None], stay))
            B.append(f"  (a) torch.sparse CSR products, f64    {ta:10.3f} ms  ({alo:.3f} .. {ahi:.3f})   = {ta / sm:.2f} x the smoothing entry; "
                     f"largest difference {float((ra - got).abs().max()):.2e}")
        except Exception as e:                                      # noqa: BLE001
            B.append(f"  (a) torch.sparse CSR products, f64    did not run here: {type(e).__name__}: {str(e)[:120]}")
        tb, lo, hi, rb = median_ms(lambda: scipy_host(v, rowptr, colidx, hb))
        B += [f"  (b) scipy CSR products on the host    {tb:10.3f} ms  ({lo:.3f} .. {hi:.3f})   = {tb / sm:.2f} x the smoothing entry, {tb / pub:.2f} x the public call; "
              f"largest difference {float((rb - got).abs().max()):.2e}", ""]
        for line in B[-8:]:
            print(line, flush=True)
    B[2] = B[2].replace('CLOCKS', clocks())
    os.makedirs(out_dir, exist_ok=True)
    open(os.path.join(out_dir, 'mesh_smooth_bench.txt'), 'w').write('\n'.join(B) + '\n')


if __name__ == '__main__':
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, 'profiles'))
