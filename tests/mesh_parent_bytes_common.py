"""The cases of tests/test_gpu_mesh_parent_bytes.py and tools/record_mesh_digests.py: every Python wrapper of the mesh units that share
union_find.h and mesh_common.h, run on small seeded meshes, each output tensor and count reduced to a SHA-256.  The digests recorded with the
library of the commit before the units were given shared headers are tests/golden/mesh_units_parent.json; a refactor of those units returns the
same bytes.  The meshes come from pointdreamer_amd.synthetic and from the builders the other mesh tests already use."""
import hashlib
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'mesh_units_parent.json')
DEV = 'cuda'


def T(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def digest(x):
    """SHA-256 of one result: a tensor or array (dtype, shape and bytes), or anything json can write (counts, dicts of ints)."""
    import torch
    if torch.is_tensor(x):
        x = x.detach().cpu().numpy()
    h = hashlib.sha256()
    if isinstance(x, np.ndarray):
        h.update(f"{x.dtype.str}{x.shape}".encode())
        h.update(np.ascontiguousarray(x).tobytes())
    else:
        h.update(json.dumps(x, sort_keys=True).encode())
    return h.hexdigest()


def digests(named):
    return {k: digest(v) for k, v in named.items()}


def flat_grid(n=64, noise=0.0, seed=0):
    """An open n x n quad grid in the plane z = 0 (2 n n faces, one normal: one label and one chart for the unwrap); noise: seeded z offsets."""
    g = np.linspace(-0.4, 0.4, n + 1)
    x, y = np.meshgrid(g, g, indexing='ij')
    z = np.random.default_rng(seed).normal(0.0, noise, x.shape) if noise else np.zeros_like(x)
    v = np.stack([x, y, z], -1).reshape(-1, 3).astype(np.float32)
    i, j = np.meshgrid(np.arange(n), np.arange(n), indexing='ij')
    q = (i * (n + 1) + j).reshape(-1)
    f = np.concatenate([np.stack([q, q + n + 1, q + 1], 1), np.stack([q + 1, q + n + 1, q + n + 2], 1)])
    return v, f.astype(np.int64)


def _unwrap(build, R):
    def run():
        from pointdreamer_amd.extract_texture_map import uv_unwrap
        v, f = build()
        uvs, tex, chart = uv_unwrap(T(v.astype(np.float32)), T(f.astype(np.int64)), R, return_charts=True)
        return dict(uvs=uvs, tex_idx=tex, face_chart=chart)
    return run


def _ico_with_uvs():
    from pointdreamer_amd import synthetic
    v, f = synthetic.icosphere(8)
    fu = np.arange(3 * len(f), dtype=np.int64).reshape(-1, 3)
    u = np.random.default_rng(5).uniform(0.02, 0.98, (3 * len(f), 2)).astype(np.float32)
    return v, f, fu, u


def _subdivide(pick):
    def run():
        from pointdreamer_amd import mesh_utils as mu
        v, f, fu, u = _ico_with_uvs()
        fi = None if pick == 'all' else T(np.random.default_rng(7).integers(0, len(f), 2 * len(f) // 3))     # unsorted, with repeats
        nv, nf, nu, nfu = mu.subdivide_with_uv(T(v), T(f), T(fu), T(u), face_index=fi)
        return dict(vertices=nv, faces=nf, uvs=nu, face_uv_idx=nfu)
    return run


def _neighbour_csr():
    from pointdreamer_amd import mesh_utils as mu, synthetic
    v, f = synthetic.icosphere(22)
    rowptr, colidx = mu.neighbour_csr(len(v), T(f))
    return dict(rowptr=rowptr, colidx=colidx)


def _zero_count():
    from pointdreamer_amd import mesh_utils as mu
    count = (np.random.default_rng(0).uniform(size=5000) > 0.4).astype(np.float32)
    return dict(zero=mu.zero_count_vertices(T(count)))


def _simplify():
    from pointdreamer_amd import spr, synthetic
    v, f = synthetic.icosphere(22, noise=0.004, seed=2)
    c = np.random.default_rng(11).uniform(0, 1, v.shape).astype(np.float32)
    ov, of, oc, counts = spr.simplify_mesh(T(v), T(f), len(f) // 2, colors=T(c), return_counts=True)
    return dict(vertices=ov, faces=of, colors=oc, counts=counts)


def _components():
    import mesh_components_common as mc
    from pointdreamer_amd import mesh_components as pm
    v, f, c = mc.blobs()
    tv, tf = T(v), T(f)
    vcomp, fcomp, stats = pm.label_components(tf, vertices=tv, return_stats=True)
    out = dict(vertex_comp=vcomp, face_comp=fcomp, counts=[stats['count'], stats['referenced'], stats['unreferenced']])
    out.update({'stats_' + k: stats[k] for k in ('root', 'vertices', 'faces', 'box')})
    keep = np.random.default_rng(3).uniform(size=len(f)) > 0.5
    cv, cf, cc, vmap = pm.compact_mesh(tv, tf, T(keep), colors=T(c), return_map=True)
    out.update(compact_vertices=cv, compact_faces=cf, compact_colors=cc, compact_map=vmap)
    fv, ff, fc, counts = pm.filter_components(tv, tf, colors=T(c), min_face_share=0.25, min_diameter_share=0.1, return_counts=True)
    out.update(filter_vertices=fv, filter_faces=ff, filter_colors=fc, filter_counts=counts)
    return out


def _clean(rel_tol):
    def run():
        import mesh_clean_common as cc
        from pointdreamer_amd import mesh_clean as pc
        v, f = cc.icosphere(4)
        sv, sf = cc.soup(v, f)
        diag = float(np.linalg.norm(sv.max(0).astype(np.float64) - sv.min(0).astype(np.float64)))
        tol = rel_tol * diag
        rep, wc = pc.weld_vertices(T(sv), tol, return_counts=True)
        col = np.random.default_rng(6).uniform(0, 1, sv.shape).astype(np.float32)
        ov, of, oc, vmap, fidx, counts = pc.clean_mesh(T(sv), T(sf), colors=T(col), tolerance=tol, return_map=True, return_face_index=True,
                                                       return_counts=True)
        return dict(rep=rep, weld_counts=wc, vertices=ov, faces=of, colors=oc, vertex_map=vmap, face_index=fidx, counts=counts)
    return run


def _smooth():
    from pointdreamer_amd import mesh_smooth as ps
    v, f = flat_grid(48, noise=0.004, seed=9)
    mask, bc = ps.boundary_vertices(T(f), len(v), return_counts=True)
    out, sc = ps.taubin_smooth(T(v), T(f), steps=5, return_counts=True)
    free = ps.taubin_smooth(T(v), T(f), steps=3, boundary='free')
    return dict(boundary=mask.view(__import__('torch').uint8), boundary_counts=bc, smoothed=out, smooth_counts=sc, smoothed_free=free)


def _uv_meshes():
    import test_gpu_uv_atlas as uva
    return dict(uv_sphere=(uva.mesh_uv_sphere, 512), torus=(uva.mesh_torus, 512), two_components=(uva.mesh_two_components, 512),
                dirty=(uva.mesh_dirty, 512), ico_10k=(lambda: uva.mesh_icosphere(22), 1024), flat_grid=(flat_grid, 512))


UV_NAMES = ('uv_sphere', 'torus', 'two_components', 'dirty', 'ico_10k', 'flat_grid')
CASES = {f'uv_unwrap/{n}': (lambda n=n: _unwrap(*_uv_meshes()[n])()) for n in UV_NAMES}
CASES.update({
    'subdivide/all': _subdivide('all'), 'subdivide/duplicates': _subdivide('duplicates'), 'neighbour_csr': _neighbour_csr,
    'compact_zero_count': _zero_count, 'simplify_mesh': _simplify, 'components': _components, 'clean/tol0': _clean(0.0),
    'clean/tol1e-4': _clean(1.0e-4), 'smooth': _smooth,
})


def run_case(name):
    """{output name: sha256} of one case."""
    return digests(CASES[name]())
