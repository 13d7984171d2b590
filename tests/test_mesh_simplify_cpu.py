"""Mesh decimation without a GPU (csrc/simplify_mesh.hip, spr.simplify_mesh): the size query, the argument checks of the C entry (made
before any memory is touched, so null and host pointers do), the wrappers' refusal of CPU tensors, the `spr_faces` config key, and a
self-check of the sequential reference decimator the GPU tests measure against (tests/mesh_simplify_common.py)."""
import ctypes as C
import os
import time

import numpy as np
import pytest
import torch

from conftest import ROOT

LIB = os.path.join(ROOT, 'pointdreamer_amd', 'libpdhip.so')
needs_lib = pytest.mark.skipif(not os.path.exists(LIB), reason="libpdhip.so not built")


@needs_lib
def test_size_query():
    from pointdreamer_amd import _lib
    q = _lib.lib().pdhip_simplify_mesh_workspace_bytes
    assert q(4, 4) > 0
    for a, b in ((4, 5), (100, 1000), (27_000, 110_000), (110_000, 1 << 22)):
        assert 0 < q(a, 1000) <= q(b, 1000) and 0 < q(1000, a) <= q(1000, b)
    assert q(110_000, 220_000) > q(27_000, 55_000) > q(7_000, 14_000)
    assert q(110_000, 220_000) >= 110_000 * (10 * 8 + 3 * 4) + 2 * 3 * 220_000 * 4          # quadrics + positions, two face tables
    for v, f in ((3, 4), (4, 3), (0, 100), (100, 0), (-1, 100), (100, -5), ((1 << 22) + 1, 100), (100, (1 << 23) + 1)):
        assert q(v, f) == 0, (v, f)


@needs_lib
def test_entry_validates_its_arguments_before_touching_memory():
    from pointdreamer_amd import _lib
    L = _lib.lib()
    null = C.c_void_p(0)
    buf = (C.c_char * 64)()
    p = C.cast(buf, C.c_void_p)
    ok = dict(vertices=null, Vn=100, faces=null, F=196, colors=null, target=50, ov=null, of=null, oc=null, counts=null, ws=null)
    # every pointer null: the first check refuses, whatever else is wrong -- nothing is dereferenced
    for k, bad in ((None, None), ('Vn', 3), ('F', 3), ('Vn', -1), ('F', -7), ('Vn', (1 << 22) + 1), ('F', (1 << 23) + 1), ('target', 3),
                   ('target', 0), ('target', -1)):
        a = dict(ok)
        if k:
            a[k] = bad
        assert L.pdhip_simplify_mesh(*a.values(), null) == -1, (k, bad)
        assert 'pdhip_simplify_mesh' in L.pdhip_last_error().decode()
    # with (host) pointers in place each scalar check is reached by itself; these all return before the first launch or copy
    okp = dict(vertices=p, Vn=100, faces=p, F=196, colors=null, target=50, ov=p, of=p, oc=null, counts=p, ws=p)
    for k, bad, word in (('vertices', null, 'null'), ('faces', null, 'null'), ('ov', null, 'null'), ('of', null, 'null'), ('counts', null, 'null'),
                         ('ws', null, 'null'), ('colors', p, 'together'), ('oc', p, 'together'), ('Vn', 3, 'at least 4'), ('F', 2, 'at least 4'),
                         ('Vn', (1 << 22) + 1, 'key widths'), ('F', (1 << 23) + 1, 'key widths'), ('target', 3, 'target_faces'),
                         ('target', -4, 'target_faces')):
        a = dict(okp)
        a[k] = bad
        assert L.pdhip_simplify_mesh(*a.values(), null) == -1, (k, bad)
        assert word in L.pdhip_last_error().decode(), (k, bad, L.pdhip_last_error())


def test_wrappers_refuse_cpu_tensors():
    from pointdreamer_amd import spr
    from pointdreamer_amd._lib import PdhipError
    v, f = torch.zeros((100, 3)), torch.zeros((196, 3), dtype=torch.int64)
    with pytest.raises(PdhipError, match='no CPU path'):
        spr.simplify_mesh(v, f, 50)
    with pytest.raises(PdhipError, match='no CPU path'):
        spr.simplify_mesh(v, f, 50, colors=v, return_counts=True)
    with pytest.raises(PdhipError, match='CPU tensor'):
        spr.recon_one_shape_SPR(v, v, target_faces=10000)
    with pytest.raises(NotImplementedError, match='decimation.*target_faces'):
        spr.recon_one_shape_SPR(np.zeros((100, 3)), np.zeros((100, 3)), None, None, 7, 10000)
    with pytest.raises(TypeError):                                  # keyword-only: the reference's sixth positional stays simplify_face_num
        spr.recon_one_shape_SPR(np.zeros((100, 3)), np.zeros((100, 3)), None, None, 7, None, 10000)


def test_spr_faces_config_key():
    from pointdreamer_amd import demo
    cfgf = os.path.join(ROOT, 'configs', 'nearest.yaml')
    assert 'spr_faces' not in demo.load_config(cfgf) and 'spr_faces' in demo.GEOMETRY_KEYS
    assert 'spr_faces' not in demo.load_config(os.path.join(ROOT, 'configs', 'geo_by_SPR.yaml'))
    cfg = demo.load_config(cfgf, dict(geo_from='SPR', spr_depth=7, spr_faces=10000))
    assert cfg.spr_faces == 10000 and demo.load_config(cfgf, dict(spr_faces=4)).spr_faces == 4
    assert 'spr_faces' not in demo._pipeline_kwargs(cfg)
    with pytest.raises(KeyError):
        demo.load_config(cfgf, dict(spr_face=10000))
    for bad in (3, -1, 'many', 10000.0, True):
        with pytest.raises(ValueError):
            demo.load_config(cfgf, dict(spr_faces=bad))


def test_sequential_reference_on_the_torus():
    import mesh_simplify_common as ms
    from pointdreamer_amd import mesh_checks as mc
    v, f = ms.grid_torus(40, 20)
    assert len(f) == 1600 and mc.directed_edge_defects(f) == 0 and mc.signed_volume(v, f) > 0 and ms.topology(len(v), f) == [(1600, 0)]
    t = time.time()
    ov, of = ms.sequential_qem(v, f, 400)
    print(f"sequential 1600 -> {len(of)} faces in {time.time() - t:.2f} s")
    assert len(of) == 400 and mc.directed_edge_defects(of) == 0 and ms.topology(len(ov), of) == [(400, 0)]
    assert mc.face_areas(ov, of).min() > 0 and len(np.unique(of)) == len(ov)
    vol, vol0 = mc.signed_volume(ov, of), mc.signed_volume(v, f)
    assert 0.95 * vol0 < vol < 1.05 * vol0
    m = ms.metrics(v, ov, of)
    print(m)
    assert m['sdf_max'] < 0.02 and m['v2m_max'] < 0.02             # (a cell of the 40 x 20 grid is 0.05 wide)
    # a torus cannot have 4 faces: the reference stops where no valid collapse is left, still a torus
    sv, sf = ms.sequential_qem(*ms.grid_torus(4, 3), 4)
    assert len(sf) > 5 and mc.directed_edge_defects(sf) == 0 and ms.topology(len(sv), sf) == [(len(sf), 0)]
