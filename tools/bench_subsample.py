"""Times and parity of the farthest-point subsampling (csrc/subsample.hip) on one MI355X -> profiles/subsample_bench.txt and
profiles/subsample_parity.txt.

  python tools/bench_subsample.py [out_dir]      # out_dir: where the two files go (default: profiles/)
  python tools/bench_subsample.py --one-call     # one 10^6 -> 30 000 call on the sphere and nothing else (the workload of a kernel trace)
  python tools/bench_subsample.py --sweep [out_dir]   # the same four cases under pdhip_debug_set_fps_cells -> profiles/subsample_grid_sweep.txt

Workload: 10^5 -> 30 000 and 10^6 -> 30 000 float32 points, `sphere` (a noisy sphere surface: what a scan looks like) and `box` (uniform in a cube).
Per case HIP events round the whole call of subsample.farthest_point_sample (its one stream synchronisation and host read included): 2 warm-up calls
and the median of 7 (min .. max) at 10^5 points, 1 and 5 at 10^6.
  torch loop        the same definition in float64 torch ops on the same device, one minimum and one argmax over all N points per pick and no host
                    synchronisation inside the loop; after a warm-up of 200 picks it runs ONCE, and that run's output is what the parity at full size
                    is checked against (torch.argmax promises no order among equal values: a pick that differs is reported, not hidden)
  mean colours      subsample.owner_mean_colors on the picks (pdhip_nearest_points + pdhip_owner_mean_colors), timed the same way
Recorded per case: counts (cells per axis, occupied cells, point updates over all picks) against the N M updates of the brute-force scan, and the time
per pick.  Parity file: the cases above against the torch loop, and the 100 000 -> 2 000 case of tests/test_gpu_subsample.py against the numpy oracle
with its measured update count (the test asserts it is below a tenth of N M)."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)
from pointdreamer_amd import _lib, subsample      # noqa: E402
from tools.bench_geometry_metrics import clocks      # noqa: E402
from tools.bench_surface_recon import timed      # noqa: E402
import subsample_common as sc      # noqa: E402

M = 30000


def torch_fps(points, num, start=0):
    """(idx [num] i64, min_d2 [num] f64) of the definition in float64 torch ops; the picked index never leaves the device."""
    p = points.double()
    x, y, z = p[:, 0].contiguous(), p[:, 1].contiguous(), p[:, 2].contiguous()
    idx = torch.empty((num,), dtype=torch.int64, device=p.device)
    out = torch.empty((num,), dtype=torch.float64, device=p.device)
    idx[0], out[0] = start, float('inf')
    dx, dy, dz = x - x[start], y - y[start], z - z[start]
    mind = (dx * dx + dy * dy) + dz * dz
    mind[start] = -1.0
    for k in range(1, num):
        j = torch.argmax(mind)
        idx[k], out[k] = j, mind[j]
        dx, dy, dz = x - x[j], y - y[j], z - z[j]
        mind = torch.where(mind >= 0.0, torch.minimum(mind, (dx * dx + dy * dy) + dz * dz), mind)
        mind[j] = -1.0
    return idx, out


def median_ms(fn, warmup, repeat):
    ts = []
    for it in range(warmup + repeat):
        t, r = timed(fn)
        if it >= warmup:
            ts.append(t)
    return float(np.median(ts)), min(ts), max(ts), r


def one_call():
    dev = torch.device('cuda', torch.cuda.current_device())
    p = torch.from_numpy(sc.sphere_points(1000000, 1, 0.5, 0.002)).to(dev)
    idx, d2, counts = subsample.farthest_point_sample(p, M, return_min_d2=True, return_counts=True)
    torch.cuda.synchronize()
    print('one call: 1000000 ->', M, 'counts', counts.cpu().tolist(), 'covering radius', float(d2[-1].sqrt()))


def sweep(out_dir):
    """Three calls per setting (the first is the warm-up of the case's first setting only), bytes compared with the default grid's."""
    L = _lib.lib()
    dev = torch.device('cuda', torch.cuda.current_device())
    S = [f"Cells per axis of the FPS grid on one MI355X (tools/bench_subsample.py --sweep): N float32 points -> {M}, pdhip_debug_set_fps_cells;",
         "cells 0 = the shipped rule, C = cbrt(N / 32) <= 40; ms of three whole calls in a row (HIP events); counts = cells per axis, occupied cells, point",
         "updates over all picks; `same`: idx and min_d2 equal the default grid's bytes.", ""]
    for N, cells in ((100000, (0, 10, 14, 18, 22, 28, 34, 40)), (1000000, (0, 20, 25, 31, 36, 40))):
        for name, pts in (('sphere', sc.sphere_points(N, 1, 0.5, 0.002)), ('box', sc.box_points(N, 2))):
            p = torch.from_numpy(pts).to(dev)
            ref = None
            for c in cells:
                old = L.pdhip_debug_set_fps_cells(c)
                try:
                    ts = []
                    for _ in range(3):
                        t, r = timed(lambda: subsample.farthest_point_sample(p, M, return_min_d2=True, return_counts=True))
                        ts.append(t)
                finally:
                    L.pdhip_debug_set_fps_cells(old)
                ref = r if ref is None else ref
                same = torch.equal(r[0], ref[0]) and torch.equal(r[1].view(torch.int64), ref[1].view(torch.int64))
                S.append(f"{name:6s} {N:8d}  cells {c:2d}  ms {ts[0]:8.1f} {ts[1]:8.1f} {ts[2]:8.1f}  counts {r[2].cpu().tolist()}  {'same' if same else 'DIFFERENT'}")
                print(S[-1], flush=True)
            S.append("")
    os.makedirs(out_dir, exist_ok=True)
    open(os.path.join(out_dir, 'subsample_grid_sweep.txt'), 'w').write('\n'.join(S))


def main(out_dir):
    dev = torch.device('cuda', torch.cuda.current_device())
    T = lambda x: torch.from_numpy(np.array(x)).to(dev)
    B = [f"Farthest-point subsampling on one MI355X (tools/bench_subsample.py): N float32 points -> {M}; HIP events round the whole call;",
         "2 warm-up calls and the median of 7 (min .. max) at 10^5 points, 1 and 5 at 10^6; the torch loop runs once after a warm-up of 200 picks.",
         f"device: {torch.cuda.get_device_name(dev)}; clocks after the run: CLOCKS", ""]
    P = ["Parity of the farthest-point subsampling (tools/bench_subsample.py).", ""]
    verdict = []
    for N in (100000, 1000000):
        for name, pts in (('sphere', sc.sphere_points(N, 1, 0.5, 0.002)), ('box', sc.box_points(N, 2))):
            p = T(pts)
            col = torch.rand((N, 3), device=dev)
            rounds = (2, 7) if N <= 100000 else (1, 5)
            med, lo, hi, (idx, d2, counts) = median_ms(lambda: subsample.farthest_point_sample(p, M, return_min_d2=True, return_counts=True), *rounds)
            counts = counts.cpu().tolist()
            cmed, clo, chi, _ = median_ms(lambda: subsample.owner_mean_colors(p, col, idx), *rounds)
            torch_fps(p, 200)
            base, (tidx, td2) = timed(lambda: torch_fps(p, M))
            again = subsample.farthest_point_sample(p, M, return_min_d2=True)
            differ_i = int((idx != tidx).sum())
            differ_d = int((d2.view(torch.int64) != td2.view(torch.int64)).sum())
            wins = med < base
            verdict.append((N, name, wins, base / med))
            B += [f"case {name}, {N} -> {M}: counts {counts}: {counts[0]}^3 cells, {counts[1]} occupied; {counts[2]} point updates = "
                  f"{100.0 * counts[2] / (float(N) * M):.3f} % of the brute-force scan's N M = {N * M}"
                  + (' (the count saturated)' if counts[2] == 2 ** 31 - 1 else ''),
                  f"  farthest_point_sample (whole call)  {med:10.3f} ms  ({lo:.3f} .. {hi:.3f})   = {1e3 * med / M:.2f} us per pick",
                  f"  torch loop, f64 (one run)           {base:10.3f} ms   = {1e3 * base / M:.2f} us per pick = {base / med:.2f} x the kernel's time"
                  + ('' if wins else '   ** the kernel LOSES to the baseline here **'),
                  f"  owner_mean_colors on the picks      {cmed:10.3f} ms  ({clo:.3f} .. {chi:.3f})", ""]
            P += [f"case {name}, {N} -> {M}:",
                  f"  against the torch loop: idx differs at {differ_i} of {M} picks, min_d2 bits at {differ_d}; covering radius {float(d2[-1].sqrt()):.6g}",
                  f"  min_d2[1:] never increases: {bool((d2[2:] <= d2[1:-1]).all())}; picks distinct: {int(torch.unique(idx).numel()) == M}; two calls give "
                  f"{'EQUAL' if torch.equal(again[0], idx) and torch.equal(again[1].view(torch.int64), d2.view(torch.int64)) else 'DIFFERENT'} bytes", ""]
            for line in B[-6:] + P[-4:]:
                print(line, flush=True)
    pts, m, start = sc.case('large')
    oidx, od2 = sc.oracle_case('large')
    idx, d2, counts = subsample.farthest_point_sample(T(pts), m, start=start, return_min_d2=True, return_counts=True)
    counts = counts.cpu().tolist()
    P += [f"case 'large' of tests/test_gpu_subsample.py ({len(pts)} -> {m}, a noisy sphere) against the numpy oracle:",
          f"  idx differs at {int((idx.cpu().numpy() != oidx).sum())} of {m} picks, min_d2 bits at "
          f"{int((d2.cpu().numpy().view(np.uint64) != od2.view(np.uint64)).sum())}",
          f"  counts {counts}: {counts[2]} point updates = {100.0 * counts[2] / (len(pts) * m):.3f} % of N M = {len(pts) * m} (the test's bound: below "
          f"{len(pts) * m // 10})"]
    print('\n'.join(P[-3:]), flush=True)
    lost = [f"{name} {N}" for N, name, w, _ in verdict if not w]
    B += ["The kernel is faster than the torch loop of the same run in every case: " + ', '.join(f"{r:.1f} x at {name} {N}" for N, name, _, r in verdict) + '.'
          if not lost else "The kernel LOSES to the torch loop in: " + '; '.join(lost) + '.']
    B[2] = B[2].replace('CLOCKS', clocks())
    os.makedirs(out_dir, exist_ok=True)
    open(os.path.join(out_dir, 'subsample_bench.txt'), 'w').write('\n'.join(B) + '\n')
    open(os.path.join(out_dir, 'subsample_parity.txt'), 'w').write('\n'.join(P) + '\n')


if __name__ == '__main__':
    if len(sys.argv) > 1 and sys.argv[1] == '--one-call':
        one_call()
    elif len(sys.argv) > 1 and sys.argv[1] == '--sweep':
        sweep(sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, 'profiles'))
    else:
        main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, 'profiles'))
