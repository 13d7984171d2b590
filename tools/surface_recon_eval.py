"""Measurements behind the bounds of tests/test_gpu_surface_recon.py (needs an MI355X):

  python tools/surface_recon_eval.py accuracy    # six analytic solids x depth 6, 7 x noise 0, h/4 -> tests/golden/surface_recon_measured.json
                                                 #   and the table of profiles/surface_recon_accuracy.txt
  python tools/surface_recon_eval.py texture     # texture quality of the CLI with the reconstructed mesh against the analytic mesh
                                                 #   (torus, rounded box, three cloud seeds) -> appended to the same profile file
  python tools/surface_recon_eval.py bytes       # normals / mesh / vertex colours of three small clouds -> tests/golden/surface_recon_parent.npz:
                                                 #   run at the commit whose bytes a refactor of csrc/surface_recon.hip must keep

The helpers (cases, analytic meshes, the atlas-vs-colour-field figure) are imported by the test so that both compute the same thing."""
import json
import logging
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
N_POINTS = 25000
SOLIDS = ('sphere', 'ellipsoid', 'torus', 'rounded_box', 'two_spheres', 'cup')
JSON_PATH = os.path.join(ROOT, 'tests', 'golden', 'surface_recon_measured.json')
TXT_PATH = os.path.join(ROOT, 'profiles', 'surface_recon_accuracy.txt')
BYTES_PATH = os.path.join(ROOT, 'tests', 'golden', 'surface_recon_parent.npz')
TEXTURE_MARK = "Texture quality"


def case_cloud(name, depth, noise_frac, n=N_POINTS, seed=1):
    from pointdreamer_amd import synthetic
    S = synthetic.solid(name)
    h = 1.0 / (0.75 * 2 ** depth)
    return (S,) + S.sample(n, seed=seed, noise=noise_frac * h)


def mesh_figures(S, v, f, h, xyz):
    from pointdreamer_amd import mesh_checks as mc
    sd = np.abs(S.sdf(v)) / h
    pd = mc.point_mesh_distance(xyz, v, f) / h
    return dict(vertices=len(v), faces=len(f), bad_edges=mc.directed_edge_defects(f), volume=mc.signed_volume(v, f),
                volume_analytic=S.volume(96), components=len(mc.components_euler(len(v), f)), sdf_max_h=float(sd.max()),
                sdf_mean_h=float(sd.mean()), p2m_max_h=float(pd.max()), p2m_mean_h=float(pd.mean()))


def accuracy():
    import torch
    from pointdreamer_amd import spr
    rows = {}
    for name in SOLIDS:
        for depth in (6, 7):
            for noise in (0.0, 0.25):
                S, xyz, rgb, nrm = case_cloud(name, depth, noise)
                X, Nn = torch.from_numpy(xyz).cuda(), torch.from_numpy(nrm).cuda()
                est, cnt = spr.estimate_normals(X, return_counts=True)
                dots = (est.cpu().numpy().astype(np.float64) * nrm).sum(1)
                row = dict(counts=cnt, flipped=float((dots < 0).mean()),
                           median_angle_deg=float(np.median(np.degrees(np.arccos(np.clip(np.abs(dots), 0, 1))))))
                for tag, nn in (('analytic', Nn), ('estimated', est)):
                    v, f, info = spr.poisson_reconstruct(X, nn, depth=depth, return_counts=True)
                    row[tag] = dict(iterations=info['iterations'], **mesh_figures(S, v.cpu().numpy(), f.cpu().numpy(), info['h'], xyz))
                    assert row[tag]['bad_edges'] == 0 and row[tag]['components'] == S.components, (name, depth, noise, tag, row[tag])
                rows[f'{name}|{depth}|{noise}'] = row
                print(name, depth, noise, row, flush=True)
    json.dump(rows, open(JSON_PATH, 'w'), indent=1, sort_keys=True)
    L = ["Surface reconstruction (pointdreamer_amd/spr.py, csrc/surface_recon.hip) against the analytic solids of synthetic.Solid: 25 000 points,",
         "seed 1, one MI355X; written by tools/surface_recon_eval.py.  Distances in grid cells h (h = largest extent / (0.75 * 2^depth));",
         "'analytic' / 'estimated' = which normals the Poisson solve was given.  Every mesh: 0 bad directed edges, the expected number of",
         "components and Euler characteristics.  tests/test_gpu_surface_recon.py asserts 2 x these figures",
         "(tests/golden/surface_recon_measured.json holds the same numbers).", "",
         "solid        depth noise  normals   | flipped  median angle | faces   iters  |sdf| max / mean   cloud->mesh max / mean   volume (analytic)"]
    for key in sorted(rows):
        name, depth, noise = key.split('|')
        r = rows[key]
        for tag in ('analytic', 'estimated'):
            a = r[tag]
            L.append(f"{name:12s} {depth}     {float(noise):4.2f}h  {tag:9s} | {r['flipped']:.5f}  {r['median_angle_deg']:6.3f} deg  | {a['faces']:6d}  "
                     f"{a['iterations']:4d}   {a['sdf_max_h']:.3f} / {a['sdf_mean_h']:.3f}      {a['p2m_max_h']:.3f} / {a['p2m_mean_h']:.3f}          "
                     f"{a['volume']:.5f} ({a['volume_analytic']:.5f})")
    L += ["", "Orientation rules used (eyes / neighbours / nearest / unoriented), noise-free, depth 7:"]
    L += [f"  {k.split('|')[0]:12s} {rows[k]['counts']}" for k in sorted(rows) if k.endswith('|7|0.0')]
    L += ["", "Noise along the normal of sigma = h / 4 is survived at depth 6 and 7 by every solid (components and Euler characteristics as expected)."]
    old = open(TXT_PATH).read() if os.path.exists(TXT_PATH) else ''
    tail = old[old.index(TEXTURE_MARK):] if TEXTURE_MARK in old else ''
    open(TXT_PATH, 'w').write('\n'.join(L) + '\n' + ('\n' + tail if tail else ''))


# ---- texture quality (acceptance item 9)
def analytic_mesh(name):
    """About 10 000 faces on the analytic surface: the torus by its parametrisation, the rounded box by rays from the centre."""
    from pointdreamer_amd import synthetic
    if name == 'torus':
        nu, nv = 100, 50
        u, v = np.meshgrid(np.arange(nu) * 2 * np.pi / nu, np.arange(nv) * 2 * np.pi / nv, indexing='ij')
        rr = 0.35 + 0.15 * np.cos(v)
        P = np.stack([rr * np.cos(u), 0.15 * np.sin(v), rr * np.sin(u)], -1).reshape(-1, 3)
        i, j = np.meshgrid(np.arange(nu), np.arange(nv), indexing='ij')
        a, b = i * nv + j, ((i + 1) % nu) * nv + j
        c, d = ((i + 1) % nu) * nv + (j + 1) % nv, i * nv + (j + 1) % nv
        F = np.concatenate([np.stack([a, d, c], -1).reshape(-1, 3), np.stack([a, c, b], -1).reshape(-1, 3)])
    elif name == 'rounded_box':
        S = synthetic.solid(name)
        d, F = synthetic.icosphere(22, radius=1.0)
        d = d.astype(np.float64)
        lo, hi = np.zeros(len(d)), np.ones(len(d))
        for _ in range(50):
            mid = 0.5 * (lo + hi)
            inside = S.sdf(d * mid[:, None]) < 0
            lo, hi = np.where(inside, mid, lo), np.where(inside, hi, mid)
        P = d * (0.5 * (lo + hi))[:, None]
    else:
        raise ValueError(name)
    from pointdreamer_amd import mesh_checks as mc
    if mc.signed_volume(P, F) < 0:
        F = F[:, ::-1]
    assert mc.directed_edge_defects(F) == 0
    return P.astype(np.float32), np.ascontiguousarray(F, np.int64)


def texture_mad(name, seed, reconstructed, workdir, n=20000, extra=()):
    """Mean |atlas colour - analytic colour field at gb_pos| over the valid texels of one CLI run ('nearest', atlas 512):
    reconstructed=True: PLY only + geo_from=SPR; False: the analytic mesh supplied as <pc>_untextured_mesh.obj."""
    import PIL.Image
    import torch
    from pointdreamer_amd import demo, io_utils, synthetic
    S = synthetic.solid(name)
    xyz, rgb, _ = S.sample(n, seed=seed)
    d = os.path.join(workdir, f'{name}_{seed}_{"spr" if reconstructed else "mesh"}')
    os.makedirs(d, exist_ok=True)
    pc = os.path.join(d, 'shape.ply')
    io_utils.save_colored_pc_ply(xyz * 1.7 + 0.3, rgb, pc)
    over = ['xatlas_texture_res=512', f'output_path={os.path.join(d, "out")}']
    if reconstructed:
        over.append('geo_from=SPR')
    else:
        v, f = analytic_mesh(name)
        io_utils.save_obj_mesh(v * 1.7 + 0.3, f, os.path.join(d, 'shape_untextured_mesh.obj'))
    out = demo.main(['--config', os.path.join(ROOT, 'configs', 'nearest.yaml'), '--pc_file', pc, '--set'] + over + list(extra))[0]
    xd = torch.load(os.path.join(out, 'geo', 'xatlas_512.pth'))
    mask = xd['mask'][0, :, :, 0].numpy().astype(bool)
    pos = xd['gb_pos'][0].numpy()[mask].astype(np.float64)
    atlas = np.array(PIL.Image.open(os.path.join(out, 'models', 'model_normalized.png')))[::-1].astype(np.float64) / 255.0
    # the driver normalised the cloud (centre of the bounding box, largest extent 1): back to the solid's own frame
    w = (xyz * np.float32(1.7) + np.float32(0.3)).astype(np.float64)
    centre, ext = (w.max(0) + w.min(0)) / 2, (w.max(0) - w.min(0)).max()
    world = (pos * ext + centre - 0.3) / 1.7
    return float(np.abs(atlas[mask] - S.color(world)).mean())


def texture_table(workdir, seeds=(1, 2, 3)):
    rows = {}
    for name in ('torus', 'rounded_box'):
        i = [texture_mad(name, s, True, workdir) for s in seeds]
        ii = [texture_mad(name, s, False, workdir) for s in seeds]
        rows[name] = dict(reconstructed=i, analytic=ii, spread=max(ii) - min(ii))
    return rows


def texture():
    from pointdreamer_amd import spr
    with tempfile.TemporaryDirectory() as wd:
        rows = texture_table(wd)
    L = [f"{TEXTURE_MARK} of the CLI ('nearest', atlas 512, 20 000 points, spr_depth {spr.DEFAULT_DEPTH}): mean |atlas colour - analytic colour field at gb_pos| over the",
         "valid texels, cloud seeds 1, 2, 3; (i) PLY only + geo_from=SPR, (ii) the analytic ~10 k-face mesh supplied as <pc>_untextured_mesh.obj.",
         "The test asserts (i) <= (ii) + 2 x spread of (ii) per seed."]
    for name, r in rows.items():
        L.append(f"  {name:12s} (i) {' '.join(f'{x:.5f}' for x in r['reconstructed'])}   (ii) {' '.join(f'{x:.5f}' for x in r['analytic'])}   "
                 f"spread of (ii) {r['spread']:.5f} -> margin {2 * r['spread']:.5f}")
    old = open(TXT_PATH).read()
    head = old[:old.index(TEXTURE_MARK)] if TEXTURE_MARK in old else old + '\n'
    open(TXT_PATH, 'w').write(head + '\n'.join(L) + '\n')
    print('\n'.join(L))


def recon_bytes():
    """The arrays that tests/golden/surface_recon_parent.npz pins byte for byte (name -> numpy array; faces as int32):
      sphere_16    estimate_normals at the smallest N: k = 16 = N, one cell, every scan ends by covering the grid
      cup_257      estimate_normals with N off the workgroup size and a few cells per axis
      cup_1500     estimate_normals, then poisson_reconstruct(depth=6, colors=rgb): normals, vertices, faces, vertex colours"""
    import torch
    from pointdreamer_amd import synthetic, spr
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    out = {}
    for name, n in (('sphere', 16), ('cup', 257)):
        out[f'{name}_{n}_normals'] = spr.estimate_normals(T(synthetic.solid(name).sample(n, seed=1)[0]))
    xyz, rgb, _ = synthetic.solid('cup').sample(1500, seed=1)
    nrm = spr.estimate_normals(T(xyz))
    v, f, c = spr.poisson_reconstruct(T(xyz), nrm, depth=6, colors=T(rgb))
    out.update(cup_1500_normals=nrm, cup_1500_vertices=v, cup_1500_faces=f.to(torch.int32), cup_1500_colors=c)
    return {k: a.cpu().numpy() for k, a in out.items()}


def write_recon_bytes():
    got = recon_bytes()
    np.savez_compressed(BYTES_PATH, **got)
    print(f"{BYTES_PATH}: {os.path.getsize(BYTES_PATH)} bytes; " + ', '.join(f"{k} {a.shape}" for k, a in got.items()))


if __name__ == '__main__':
    logging.getLogger('pointdreamer_amd').setLevel(logging.WARNING)
    {'accuracy': accuracy, 'texture': texture, 'bytes': write_recon_bytes}[sys.argv[1]]()
