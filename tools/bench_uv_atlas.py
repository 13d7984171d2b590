"""Wall time of the device UV unwrap (pdhip_uv_atlas through extract_texture_map.uv_unwrap, the final host read of `counts`
included) on noisy icospheres of about 10 k, 100 k and 500 k faces, with the chart count, the split rounds and the atlas coverage
(mask mean of xatlas_uvmap_w_face_id).  The reference's xatlas step takes 1.88 s per shape on the CPU.
Usage (GPU box): python tools/bench_uv_atlas.py [--iters 10] [--out uv_atlas_bench.json]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from pointdreamer_amd import synthetic, _lib
from pointdreamer_amd._lib import ptr, stream
from pointdreamer_amd.extract_texture_map import uv_unwrap, xatlas_uvmap_w_face_id

ap = argparse.ArgumentParser()
ap.add_argument('--iters', type=int, default=10)
ap.add_argument('--sizes', type=int, nargs='*', default=[22, 71, 158], help='icosphere subdivisions (20 n^2 faces)')
ap.add_argument('--res', type=int, nargs='*', default=[1024, 2048, 2048])
ap.add_argument('--out', default=None)
a = ap.parse_args()
dev = 'cuda'
rows = []
for n, R in zip(a.sizes, a.res):
    v, f = synthetic.icosphere(n, noise=0.09 / n, seed=0)          # (radial noise of about 8 % of the edge length)
    tv, tf = torch.from_numpy(v).to(dev), torch.from_numpy(f).to(dev)
    for _ in range(2):
        uv_unwrap(tv, tf, R)
    torch.cuda.synchronize()
    times = []
    for _ in range(a.iters):
        t0 = time.perf_counter()
        uv_unwrap(tv, tf, R)                      # (returns after reading counts back: the call's full wall time)
        times.append(time.perf_counter() - t0)
    L = _lib.lib()
    out = xatlas_uvmap_w_face_id(None, tv, tf, R)
    # chart count and split rounds: the C entry point's counts[1], counts[2]
    Vn, F = len(v), len(f)
    ws = torch.empty((L.pdhip_uv_atlas_ws_bytes(Vn, F),), dtype=torch.uint8, device=dev)
    cnt = torch.zeros(4, dtype=torch.int32, device=dev)
    u2 = torch.empty((3 * F, 2), device=dev); t2 = torch.empty((F, 3), dtype=torch.int64, device=dev)
    c2 = torch.empty((F,), dtype=torch.int32, device=dev)
    assert L.pdhip_uv_atlas(ptr(tv), Vn, ptr(tf), F, R, 2, ptr(u2), ptr(t2), ptr(c2), ptr(cnt), ptr(ws), stream()) == 0
    c = cnt.cpu().tolist()
    rows.append(dict(faces=F, vertices=Vn, resolution=R, ms_median=1e3 * float(np.median(times)), ms_min=1e3 * float(np.min(times)),
                     uv_entries=c[0], charts=c[1], split_rounds=c[2], mask_coverage=float(out[3].float().mean()),
                     ws_mib=ws.numel() / 2 ** 20))
    print(json.dumps(rows[-1]), flush=True)
if a.out:
    os.makedirs(os.path.dirname(a.out) or '.', exist_ok=True)
    with open(a.out, 'w') as fh:
        json.dump(rows, fh, indent=1)
