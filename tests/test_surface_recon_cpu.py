"""Surface reconstruction without a GPU: argument validation of the four entry points (checked before any memory is touched, so
host pointers do), workspace sizes, the Python wrappers' refusals, the config keys, the host-side mesh checker, the case table."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT

LIB = os.path.join(ROOT, 'pointdreamer_amd', 'libpdhip.so')
needs_lib = pytest.mark.skipif(not os.path.exists(LIB), reason="libpdhip.so not built")


@needs_lib
def test_entry_points_validate_their_arguments():
    from pointdreamer_amd import _lib
    L = _lib.lib()
    assert L.pdhip_version() >= 209
    buf = (C.c_char * 64)()
    p = C.cast(buf, C.c_void_p)
    null = C.c_void_p(0)
    err = lambda: L.pdhip_last_error().decode()
    for args in ((null, 100, 16, 32, 1.6, p, p, p, null), (p, 100, 16, 32, 1.6, null, p, p, null), (p, 100, 16, 32, 1.6, p, p, null, null),
                 (p, 15, 16, 32, 1.6, p, p, p, null), (p, -1, 16, 32, 1.6, p, p, p, null), (p, 100, 2, 32, 1.6, p, p, p, null),
                 (p, 100, 33, 32, 1.6, p, p, p, null), (p, 20, 24, 32, 1.6, p, p, p, null), (p, 100, 16, 0, 1.6, p, p, p, null),
                 (p, 100, 16, 65, 1.6, p, p, p, null), (p, 100, 16, 32, 0.0, p, p, p, null), (p, 100, 16, 32, -1.0, p, p, p, null)):
        assert L.pdhip_estimate_normals(*args) == -1, args
        assert 'pdhip_estimate_normals' in err()
    ok = dict(points=p, normals=p, colors=null, N=100, depth=7, vertices=p, vcap=10, faces=p, fcap=10, vcol=null, counts=p, info=p, ws=p)
    for k, bad in (('points', null), ('normals', null), ('vertices', null), ('faces', null), ('counts', null), ('info', null), ('ws', null),
                   ('colors', p), ('vcol', p), ('N', 15), ('N', -3), ('depth', 5), ('depth', 9), ('depth', 12), ('vcap', 0), ('fcap', -1)):
        a = dict(ok)
        a[k] = bad
        assert L.pdhip_surface_recon(*a.values(), null) == -1, (k, bad)
        assert 'pdhip_surface_recon' in err()


@needs_lib
def test_workspace_sizes_grow_with_n_and_depth():
    from pointdreamer_amd import _lib
    L = _lib.lib()
    a = [L.pdhip_surface_recon_ws_bytes(30000, d) for d in (6, 7, 8)]
    assert 0 < a[0] < a[1] < a[2]
    assert a[1] >= 5 * 4 * 129 ** 3                                  # chi, r, p, q, f at depth 7
    assert L.pdhip_surface_recon_ws_bytes(10000, 7) < a[1]
    assert L.pdhip_surface_recon_ws_bytes(30000, 5) == 0 and L.pdhip_surface_recon_ws_bytes(30000, 9) == 0 and L.pdhip_surface_recon_ws_bytes(15, 7) == 0
    b = [L.pdhip_estimate_normals_ws_bytes(n, 16, 32) for n in (1000, 10000, 30000)]
    assert 0 < b[0] < b[1] < b[2]
    assert L.pdhip_estimate_normals_ws_bytes(30000, 32, 32) > b[2] and L.pdhip_estimate_normals_ws_bytes(30000, 16, 64) > b[2]
    assert L.pdhip_estimate_normals_ws_bytes(30000, 33, 32) == 0 and L.pdhip_estimate_normals_ws_bytes(30000, 16, 65) == 0


def test_python_wrappers_refuse_what_is_not_built():
    from pointdreamer_amd import spr
    from pointdreamer_amd._lib import PdhipError
    x = torch.zeros((100, 3))
    with pytest.raises(PdhipError, match='no CPU path'):
        spr.estimate_normals(x)
    with pytest.raises(PdhipError, match='no CPU path'):
        spr.poisson_reconstruct(x, x, depth=7)
    with pytest.raises(PdhipError, match='CPU tensor'):
        spr.recon_one_shape_SPR(x, x)
    with pytest.raises(NotImplementedError, match='decimation'):
        spr.recon_one_shape_SPR(np.zeros((100, 3)), np.zeros((100, 3)), simplify_face_num=10000)
    with pytest.raises(ValueError, match='6, 7 or 8'):
        spr.recon_one_shape_SPR(np.zeros((100, 3)), np.zeros((100, 3)), depth=12)
    with pytest.raises(ValueError, match='6, 7 or 8'):
        spr.poisson_reconstruct(x, x, depth=12)


def test_config_keys(tmp_path):
    import json
    import yaml
    from pointdreamer_amd import demo
    cfgf = os.path.join(ROOT, 'configs', 'nearest.yaml')
    cfg = demo.load_config(cfgf)
    assert 'spr_depth' not in cfg and 'spr_knn' not in cfg          # (defaults are read where the geometry is made: config.yaml copies stay as they were)
    cfg = demo.load_config(cfgf, dict(spr_depth=6, spr_knn=12, geo_from='SPR'))
    assert cfg.spr_depth == 6 and cfg.spr_knn == 12
    kw = demo._pipeline_kwargs(cfg)
    assert 'spr_depth' not in kw and 'spr_knn' not in kw and 'geo_from' not in kw
    with pytest.raises(KeyError):
        demo.load_config(cfgf, dict(spr_dept=6))
    with pytest.raises(ValueError):
        demo.load_config(cfgf, dict(spr_depth=12))
    for bad in (2, 33, 'many'):
        with pytest.raises(ValueError):
            demo.load_config(cfgf, dict(spr_knn=bad))
    ref = json.load(open(os.path.join(ROOT, 'tests', 'golden', 'reference_configs.json')))
    assert len(ref) == 5
    for fname, table in ref.items():
        p = tmp_path / fname
        p.write_text(yaml.safe_dump(table))
        assert demo.load_config(str(p))['texture_gen_method'] == table['texture_gen_method']
    assert demo.load_config(os.path.join(ROOT, 'configs', 'geo_by_SPR.yaml')).geo_from == 'SPR'


def test_mesh_checker_on_a_tetrahedron():
    from pointdreamer_amd import mesh_checks as mc
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], np.float64)
    f = np.array([[0, 2, 1], [0, 1, 3], [0, 3, 2], [1, 2, 3]])
    assert mc.directed_edge_defects(f) == 0
    assert abs(mc.signed_volume(v, f) - 1 / 6) < 1e-15
    assert mc.components_euler(4, f) == [(4, 6, 4, 2)]
    flipped = f.copy()
    flipped[0] = flipped[0][::-1]
    assert mc.directed_edge_defects(flipped) > 0
    assert mc.directed_edge_defects(f[:3]) > 0
    assert mc.signed_volume(v, f[:, ::-1]) < 0
    d = mc.point_mesh_distance(np.array([[0.1, 0.1, -0.5], [2.0, 0, 0], [0.3, 0.3, 0.3], [-1.0, -1, -1]]), v, f)
    assert np.allclose(d, [0.5, 1.0, 0.1 / 3 ** 0.5, 3 ** 0.5])


def test_case_table_is_the_generated_one_and_closes_every_field():
    """The committed header equals the generator's output, and the table gives a closed oriented surface on random fields."""
    assert subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'gen_mc_tables.py'), '--check']).returncode == 0
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import gen_mc_tables as g
    table = g.build()
    assert max(len(t) for t in table) == 5 and len(table[0]) == 0 and len(table[255]) == 0
    rng = np.random.default_rng(0)
    n = 6
    for _ in range(8):
        chi = rng.standard_normal((n, n, n))
        chi[0] = chi[-1] = chi[:, 0] = chi[:, -1] = -9
        chi[:, :, 0] = chi[:, :, -1] = -9
        seen = {}
        for i in range(n - 1):
            for j in range(n - 1):
                for k in range(n - 1):
                    m = sum(1 << c for c in range(8) if chi[i + (c & 1), j + ((c >> 1) & 1), k + (c >> 2)] > 0)
                    for t in table[m]:
                        vs = []
                        for e in t:
                            ax, uv = e // 4, e % 4
                            o = [0, 0, 0]
                            oth = [a for a in range(3) if a != ax]
                            o[oth[0]], o[oth[1]] = uv & 1, uv >> 1
                            vs.append((i + o[0], j + o[1], k + o[2], ax))
                        for a in range(3):
                            key = (vs[a], vs[(a + 1) % 3])
                            seen[key] = seen.get(key, 0) + 1
        assert all(c == 1 and seen.get((k[1], k[0]), 0) == 1 for k, c in seen.items())


def test_solids_are_consistent():
    from pointdreamer_amd import synthetic
    for name in synthetic.Solid.NAMES:
        if name == 'ellipsoid':
            continue                                               # (its Newton projection is slow; covered on the GPU box)
        S = synthetic.solid(name)
        x, rgb, nrm = S.sample(2000, seed=3)
        assert x.shape == (2000, 3) and rgb.min() >= 0 and rgb.max() <= 1
        assert np.abs(S.sdf(x)).max() < 1e-6 and np.abs(x).max() <= 0.5 + 1e-6
        assert np.allclose(np.linalg.norm(nrm, axis=1), 1, atol=1e-5)
        # (a step along the normal changes the distance by its length, except next to a concave crease such as the cup's inner corner)
        assert np.mean(np.abs(S.sdf(x + 0.01 * nrm) - 0.01) < 1e-4) > 0.97 and np.mean(np.abs(S.sdf(x - 0.01 * nrm) + 0.01) < 1e-4) > 0.97
        x2, _, _ = S.sample(2000, seed=3)
        assert np.array_equal(x, x2)
