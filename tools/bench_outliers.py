"""Times and parity of the exact k-NN and of statistical outlier removal (csrc/knn.hip) on one MI355X -> profiles/outliers_bench.txt and
profiles/outliers_parity.txt.

  python tools/bench_outliers.py [out_dir]        # out_dir: where the two files go (default: profiles/)
  python tools/bench_outliers.py --one-call       # the filter once on 10^5 sphere points and nothing else (the workload of a kernel trace)
  python tools/bench_outliers.py --sweep [out_dir]     # the 10^5 cases under pdhip_debug_set_knn(cells, 0) -> profiles/outliers_grid_sweep.txt

Workload: the 21 nearest neighbours (k = 20 and the point itself) of every point of a cloud in the cloud itself, and the whole filter
(outliers.statistical_outlier_mask, k = 20, ratio 2) on the same cloud; 30 000, 10^5 and 10^6 float32 points, `sphere` (a noisy sphere surface: what a
scan looks like) and `box` (uniform in a cube).  Per case HIP events round the whole call (its one stream synchronisation and host read included):
2 warm-up calls and the median of 7 (min .. max) up to 10^5 points, 1 and 5 at 10^6.
  torch cdist + topk   the same definition on the same device in the same run: float64 torch.cdist (no matmul form) of a chunk of queries against all
                       targets, squared, torch.topk(k, largest=False, sorted=True); 1 warm-up and the median of 3 up to 10^5 points.  A chunk
                       holds at most 2^24 distances (128 MiB): past 2^24 elements of output this torch build's cdist returned wrong distances
                       (up to 2.1 off on the unit box; a 512-row chunk equals the op-by-op reference to 2.2e-16).  At 10^6 points it runs
                       ONCE on the first 20 000 queries and the time is scaled by N / 20 000 (marked ~)
  cKDTree              scipy.spatial.cKDTree(points as float64).query(points, k = 21, workers = 16) on the host, build included, once
Recorded per case: counts (queries certified by the ring scan, queries finished by the sweep, cells per axis) and the LDS bytes per workgroup.
Parity file: per case d2 against its recomputation from idx in float64 torch ops (op by op: equal bits expected), the order of every row, the rows
whose indices differ from the torch baseline's and from the cKDTree's (neither promises an order among equal distances, and cdist rounds
differently: a differing row is reported with the largest difference of its distances), and two calls compared byte for byte."""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)
from pointdreamer_amd import _lib, outliers      # noqa: E402
from tools.bench_geometry_metrics import clocks      # noqa: E402
from tools.bench_surface_recon import timed      # noqa: E402

K = 20
KK = K + 1
SIZES = (30000, 100000, 1000000)
CHUNK_ELEMS = 1 << 24
SUBSET = 20000


def sphere_points(n, seed, radius=0.5, noise=0.002):
    rng = np.random.default_rng(seed)
    v = rng.standard_normal((n, 3))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    return (v * (radius * (1.0 + noise * rng.standard_normal((n, 1))))).astype(np.float32)


def box_points(n, seed):
    return (np.random.default_rng(seed).random((n, 3)) - 0.5).astype(np.float32)


def torch_knn(q, t, k):
    """(d2 [Q,k] f64, idx [Q,k] i64): float64 cdist + topk, chunked over the queries."""
    qd, td = q.double(), t.double()
    rows = max(1, CHUNK_ELEMS // td.shape[0])
    d2s, idxs = [], []
    for b in range(0, qd.shape[0], rows):
        d = torch.cdist(qd[b:b + rows], td, compute_mode='donot_use_mm_for_euclid_dist')
        v, i = torch.topk(d, k, dim=1, largest=False, sorted=True)
        d2s.append(v * v)
        idxs.append(i)
    return torch.cat(d2s), torch.cat(idxs)


def torch_filter(q, k, ratio):
    d2, _ = torch_knn(q, q, k + 1)
    mean_d = d2[:, 1:].sqrt().sum(1) / k
    return mean_d <= mean_d.mean() + ratio * mean_d.std()


def median_ms(fn, warmup, repeat):
    ts = []
    for it in range(warmup + repeat):
        t, r = timed(fn)
        if it >= warmup:
            ts.append(t)
    return float(np.median(ts)), min(ts), max(ts), r


def recomputed_d2(p, idx):
    """d2 of the pairs (row, idx[row, j]) in float64 torch ops, one rounding per op, in the contract's order."""
    pd = p.double()
    out = torch.empty(idx.shape, dtype=torch.float64, device=p.device)
    for j in range(idx.shape[1]):
        t = pd[idx[:, j].long()]
        dx, dy, dz = pd[:, 0] - t[:, 0], pd[:, 1] - t[:, 1], pd[:, 2] - t[:, 2]
        out[:, j] = (dx * dx + dy * dy) + dz * dz
    return out


def rows_differing(idx, d2, other_idx, other_d2):
    bad = (idx.long() != other_idx.long()).any(1)
    n = int(bad.sum())
    worst = float((d2[bad] - other_d2[bad]).abs().max()) if n else 0.0
    return n, worst


def one_call():
    dev = torch.device('cuda', torch.cuda.current_device())
    p = torch.from_numpy(sphere_points(100000, 1)).to(dev)
    keep, st = outliers.statistical_outlier_mask(p, K, 2.0, return_stats=True)
    torch.cuda.synchronize()
    print('one call: 100000 points, kept', st['kept'], 'removed', st['removed'], 'threshold', st['threshold'])


def sweep(out_dir):
    L = _lib.lib()
    dev = torch.device('cuda', torch.cuda.current_device())
    S = [f"Cells per axis of the k-NN grid on one MI355X (tools/bench_outliers.py --sweep): the {KK} nearest neighbours of 10^5 float32 points in",
         "themselves under pdhip_debug_set_knn(cells, 0); cells 0 = the shipped rule, C = sqrt(M / max(8, k / 2)) <= 128; ms of three whole calls in a row",
         "(HIP events); counts = certified by the ring scan, finished by the sweep, cells per axis; `same`: d2 and idx equal the default grid's bytes.", ""]
    for name, pts in (('sphere', sphere_points(100000, 1)), ('box', box_points(100000, 2))):
        p = torch.from_numpy(pts).to(dev)
        ref = None
        for c in (0, 16, 24, 32, 40, 48, 56, 64):
            assert L.pdhip_debug_set_knn(c, 0) >= 0
            try:
                ts = []
                for _ in range(3):
                    t, r = timed(lambda: outliers.knn_points(p, p, KK, return_counts=True))
                    ts.append(t)
            finally:
                L.pdhip_debug_set_knn(0, 0)
            ref = r if ref is None else ref
            same = torch.equal(r[0].view(torch.int64), ref[0].view(torch.int64)) and torch.equal(r[1], ref[1])
            S.append(f"{name:6s} cells {c:3d}  ms {ts[0]:8.2f} {ts[1]:8.2f} {ts[2]:8.2f}  counts {r[2].cpu().tolist()[:3]}  {'same' if same else 'DIFFERENT'}")
            print(S[-1], flush=True)
        S.append("")
    os.makedirs(out_dir, exist_ok=True)
    open(os.path.join(out_dir, 'outliers_grid_sweep.txt'), 'w').write('\n'.join(S))


def main(out_dir):
    from scipy.spatial import cKDTree
    L = _lib.lib()
    dev = torch.device('cuda', torch.cuda.current_device())
    lds = int(L.pdhip_knn_lds_bytes(KK))
    B = [f"Exact k-NN and statistical outlier removal on one MI355X (tools/bench_outliers.py): the {KK} nearest neighbours of N float32 points in",
         f"themselves and the whole filter (k = {K}, ratio 2); HIP events round the whole call; 2 warm-up calls and the median of 7 (min .. max) up to 10^5",
         "points, 1 and 5 at 10^6.  torch: float64 cdist + topk, chunked, same device, same run (median of 3; at 10^6 once on 20 000 queries, scaled: ~).",
         f"cKDTree: scipy on the host, 16 workers, build included, once.  LDS per workgroup of 64 queries at k = {KK}: {lds} bytes.",
         f"device: {torch.cuda.get_device_name(dev)}; clocks after the run: CLOCKS", ""]
    P = ["Parity of the exact k-NN (tools/bench_outliers.py).", ""]
    verdict = []
    for N in SIZES:
        for name, pts in (('sphere', sphere_points(N, 1)), ('box', box_points(N, 2))):
            p = torch.from_numpy(pts).to(dev)
            rounds = (2, 7) if N <= 100000 else (1, 5)
            med, lo, hi, (d2, idx, counts) = median_ms(lambda: outliers.knn_points(p, p, KK, return_counts=True), *rounds)
            fmed, flo, fhi, (keep, st) = median_ms(lambda: outliers.statistical_outlier_mask(p, K, 2.0, return_stats=True), *rounds)
            counts = counts.cpu().tolist()
            again = outliers.knn_points(p, p, KK)
            same = torch.equal(again[0].view(torch.int64), d2.view(torch.int64)) and torch.equal(again[1], idx)
            if N <= 100000:
                base, blo, bhi, (td2, tidx) = median_ms(lambda: torch_knn(p, p, KK), 1, 3)
                fbase, _, _, tkeep = median_ms(lambda: torch_filter(p, K, 2.0), 0, 3)
                mark, rows = '', N
                verdict.append((N, name, med < base and fmed < fbase, base / med, fbase / fmed))
            else:
                torch_knn(p[:2000], p, KK)
                t1, (td2, tidx) = timed(lambda: torch_knn(p[:SUBSET], p, KK))
                base = blo = bhi = t1 * N / SUBSET
                fbase, tkeep, mark, rows = base, None, '~', SUBSET
            t0 = time.time()
            kd, ki = cKDTree(pts.astype(np.float64)).query(pts.astype(np.float64), k=KK, workers=16)
            host = 1e3 * (time.time() - t0)
            B += [f"case {name}, N = {N}: counts {counts[:3]}: {counts[0]} queries certified by the ring scan, {counts[1]} finished by the sweep, "
                  f"{counts[2]}^3 cells",
                  f"  knn_points, k = {KK} (whole call)        {med:10.3f} ms  ({lo:.3f} .. {hi:.3f})",
                  f"  torch cdist + topk, f64                 {mark}{base:10.3f} ms  ({blo:.3f} .. {bhi:.3f})   = {base / med:.1f} x the kernel path's time"
                  + ('' if med < base else '   ** the kernel path LOSES to the baseline here **'),
                  f"  cKDTree on the host                     {host:10.3f} ms   = {host / med:.1f} x",
                  f"  statistical_outlier_mask (whole call)   {fmed:10.3f} ms  ({flo:.3f} .. {fhi:.3f})   kept {st['kept']}, removed {st['removed']}, "
                  f"threshold {st['threshold']:.6g}",
                  f"  the same filter in torch, f64           {mark}{fbase:10.3f} ms   = {fbase / fmed:.1f} x"
                  + ('' if fmed < fbase else '   ** the kernel path LOSES to the baseline here **'), ""]
            rd2 = recomputed_d2(p, idx)
            order_ok = bool(((d2[:, 1:] > d2[:, :-1]) | ((d2[:, 1:] == d2[:, :-1]) & (idx[:, 1:] > idx[:, :-1]))).all())
            nt, wt = rows_differing(idx[:rows], d2[:rows], tidx, td2)
            nk, wk = rows_differing(idx, d2, torch.from_numpy(ki).to(dev), torch.from_numpy(kd * kd).to(dev))
            P += [f"case {name}, N = {N}, k = {KK}:",
                  f"  d2 against its recomputation from idx (f64, op by op): {int((rd2.view(torch.int64) != d2.view(torch.int64)).sum())} of {d2.numel()} "
                  f"values differ in a bit; every row ascending by (d2, index): {order_ok}; slot 0 is the point itself or an earlier duplicate: "
                  f"{bool(((idx[:, 0].long() <= torch.arange(N, device=dev)) & (d2[:, 0] == 0.0)).all())}",
                  f"  against torch cdist + topk ({rows} rows): {nt} rows differ in an index, largest difference of their d2 {wt:.3g}",
                  f"  against cKDTree ({N} rows): {nk} rows differ in an index, largest difference of their d2 {wk:.3g}",
                  (f"  filter against the torch filter: {int((keep != tkeep).sum())} of {N} mask entries differ" if tkeep is not None
                   else "  filter against the torch filter: not run at this size"),
                  f"  two calls give {'EQUAL' if same else 'DIFFERENT'} bytes", ""]
            for line in B[-7:] + P[-7:]:
                print(line, flush=True)
            del td2, tidx
            torch.cuda.empty_cache()
    # the case the filter exists for: a few points far outside blow the box up, the object falls into a few crowded cells, and the queries
    # that meet more than the ring scan's work limit go through the sweep of all targets
    B += ["The same sphere with N / 1000 further points on a sphere of 20 times its radius (the box grows 20-fold; 1 warm-up call and the median of 3):"]
    for N in SIZES:
        rng = np.random.default_rng(3)
        v = rng.standard_normal((N // 1000, 3))
        far = (10.0 * v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)
        p = torch.from_numpy(np.concatenate([sphere_points(N, 1), far])[rng.permutation(N + N // 1000)]).to(dev)
        counts = outliers.knn_points(p, p, KK, return_counts=True)[2].cpu().tolist()
        fmed, flo, fhi, (keep, st) = median_ms(lambda: outliers.statistical_outlier_mask(p, K, 2.0, return_stats=True), 1, 3)
        B += [f"  N = {N} + {N // 1000}: counts {counts[:3]}; statistical_outlier_mask (whole call) {fmed:10.3f} ms  ({flo:.3f} .. {fhi:.3f})   "
              f"kept {st['kept']}, removed {st['removed']}, threshold {st['threshold']:.6g}"]
        print(B[-1], flush=True)
    B += [""]
    lost = [f"{name} {N}" for N, name, w, _, _ in verdict if not w]
    B += ["The kernel path is faster than the torch baseline of the same run at 30 000 and 10^5 points: "
          + ', '.join(f"{r:.0f} x (filter {fr:.0f} x) at {name} {N}" for N, name, _, r, fr in verdict) + '.'
          if not lost else "The kernel path LOSES to the torch baseline in: " + '; '.join(lost) + '.']
    B[4] = B[4].replace('CLOCKS', clocks())
    os.makedirs(out_dir, exist_ok=True)
    open(os.path.join(out_dir, 'outliers_bench.txt'), 'w').write('\n'.join(B) + '\n')
    open(os.path.join(out_dir, 'outliers_parity.txt'), 'w').write('\n'.join(P) + '\n')


if __name__ == '__main__':
    if len(sys.argv) > 1 and sys.argv[1] == '--one-call':
        one_call()
    elif len(sys.argv) > 1 and sys.argv[1] == '--sweep':
        sweep(sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, 'profiles'))
    else:
        main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, 'profiles'))
