"""CPU-side checks of the device UV unwrap's boundary (csrc/uv_atlas.hip): the Python entry keeps the reference's signature, the C
entry point validates its arguments before touching memory, and host tensors are refused (there is no CPU path)."""
import ctypes
import inspect

import pytest
import torch


@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as ge
    ge.build()
    from pointdreamer_amd import _lib
    return _lib.lib()


def test_reference_signature():
    from pointdreamer_amd import extract_texture_map as etm
    assert list(inspect.signature(etm.xatlas_uvmap_w_face_id).parameters) == ['ctx', 'mesh_v', 'mesh_pos_idx', 'resolution']
    sig = inspect.signature(etm.uv_unwrap)
    assert list(sig.parameters) == ['mesh_v', 'mesh_pos_idx', 'resolution', 'gutter', 'return_charts']
    assert sig.parameters['gutter'].default == 2 and sig.parameters['return_charts'].default is False
    assert 'xatlas' in etm.xatlas_uvmap_w_face_id.__doc__ and "own" in etm.xatlas_uvmap_w_face_id.__doc__


def _call(L, Vn=4, F=2, R=64, g=2, null=None):
    p = [ctypes.c_void_p(4096)] * 7
    if null is not None:
        p[null] = None
    v, f, uvs, tex, fc, counts, ws = p
    return L.pdhip_uv_atlas(v, Vn, f, F, R, g, uvs, tex, fc, counts, ws, None)


def test_argument_validation(L):
    for k in range(7):
        assert _call(L, null=k) == -1
        assert b'pdhip_uv_atlas' in L.pdhip_last_error() and b'null' in L.pdhip_last_error()
    assert _call(L, F=0) == -1 and b'F=0' in L.pdhip_last_error()
    assert _call(L, Vn=0) == -1 and b'Vn=0' in L.pdhip_last_error()
    assert _call(L, R=4, g=2) == -1 and b'resolution 4' in L.pdhip_last_error()
    assert _call(L, g=-1) == -1
    assert L.pdhip_uv_atlas_ws_bytes(4, 0) == 0 and L.pdhip_uv_atlas_ws_bytes(0, 4) == 0
    assert L.pdhip_uv_atlas_ws_bytes(100, 1000) > L.pdhip_uv_atlas_ws_bytes(100, 10) > 0
    assert L.pdhip_version() >= 208


def test_cpu_tensors_are_refused(L):
    from pointdreamer_amd import _lib
    from pointdreamer_amd.extract_texture_map import uv_unwrap, xatlas_uvmap_w_face_id
    v = torch.rand(4, 3)
    f = torch.tensor([[0, 1, 2], [0, 2, 3]])
    with pytest.raises(_lib.PdhipError):
        uv_unwrap(v, f, 64)
    with pytest.raises(_lib.PdhipError):
        xatlas_uvmap_w_face_id(None, v, f, 64)
