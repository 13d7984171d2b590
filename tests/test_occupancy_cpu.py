"""The point-in-mesh test without a GPU: the tests' all-pairs float64 oracle against the output of the reference's check_mesh_contains
(tests/golden/occupancy_ref.npz from tools/gen_golden_occupancy.py) bit for bit, the argument validation of the new entry points, the workspace
size against the layout, the host arithmetic of compute_iou, and zero scratch on the new kernels."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import ROOT, load_golden
import occupancy_common as oc

LIB = os.path.join(ROOT, 'pointdreamer_amd', 'libpdhip.so')


@pytest.fixture(scope="module")
def ref():
    return load_golden('occupancy_ref.npz')


@pytest.mark.parametrize("case", oc.GOLDEN_CASES)
def test_oracle_reproduces_the_reference_bit_for_bit(ref, case):
    v, f, p, res = (ref[f'{case}_{k}'] for k in ('vertices', 'faces', 'points', 'hash_resolution'))
    want = ref[f'{case}_contains']
    assert v.dtype == np.float32 and p.dtype == np.float32 and f.dtype == np.int64 and want.dtype == np.bool_ and int(res) == 512
    bv, bf, bp, _ = oc.golden_inputs(case)                   # the builders still give the inputs the reference saw
    assert np.array_equal(v, bv) and np.array_equal(f, bf) and np.array_equal(p, bp)
    got, counts = oc.oracle_contains(v, f, p, int(res), return_counts=True)
    print(case, 'faces', len(f), 'points', len(p), 'contained', int(want.sum()), 'counts', counts, 'unequal', int((got != want).sum()))
    assert np.array_equal(got, want)
    assert 0 < want.sum() < len(p)
    assert (counts[1] > 0) == (case != 'icosphere')          # on-edge points and the open mesh: the two parities disagree somewhere


def test_fixture_sizes():
    assert len(oc.golden_inputs('icosphere')[1]) == 2880 and len(oc.golden_inputs('icosphere')[2]) == 4096
    assert len(oc.golden_inputs('edges')[1]) == 528 and len(oc.golden_inputs('edges')[2]) == 794
    assert len(oc.golden_inputs('open')[1]) < 528 and len(oc.golden_inputs('open')[2]) == 4096


def _lib():
    import __graft_entry__ as ge
    ge.build()
    from pointdreamer_amd import _lib
    return _lib.lib()


def test_argument_validation_names_the_cause():
    L = _lib()
    one = C.c_void_p(256)                                        # (never dereferenced: the arguments are refused first)
    ok = dict(vertices=one, Vn=8, faces=one, F=12, points=one, Q=5, resolution=512, occ=one, counts=one, ws=one, stream=None)
    order = list(ok)
    call = lambda **kw: L.pdhip_mesh_contains(*[dict(ok, **kw)[k] for k in order])
    for name in ('vertices', 'faces', 'points', 'occ', 'counts', 'ws'):
        assert call(**{name: None}) == -1
        msg = L.pdhip_last_error()
        assert b'pdhip_mesh_contains' in msg and b'null pointer' in msg and name.encode() in msg, msg
    for kw, word in ((dict(Vn=0), b'Vn=0'), (dict(F=0), b'F=0'), (dict(F=(1 << 22) + 1), b'F=4194305'), (dict(Q=-1), b'Q=-1'),
                     (dict(Q=(1 << 26) + 1), b'Q=67108865'), (dict(resolution=1), b'resolution=1'), (dict(resolution=4097), b'resolution=4097')):
        assert call(**kw) == -1
        assert word in L.pdhip_last_error(), (kw, L.pdhip_last_error())
    iou = lambda a=one, b=one, Q=5, out=one: L.pdhip_occupancy_iou(a, b, Q, out, None)
    for kw, word in ((dict(a=None), b'(a)'), (dict(b=None), b'(b)'), (dict(out=None), b'(out)'), (dict(Q=-1), b'Q=-1'), (dict(Q=(1 << 26) + 1), b'Q=')):
        assert iou(**kw) == -1
        assert b'pdhip_occupancy_iou' in L.pdhip_last_error() and word in L.pdhip_last_error(), (kw, L.pdhip_last_error())


def test_workspace_size_refuses_what_the_entry_refuses():
    ws = _lib().pdhip_mesh_contains_workspace_bytes
    assert ws(8, 12, 5, 512) > 0 and ws(8, 12, 0, 512) > 0 and ws(8, 1 << 22, 1 << 26, 4096) > 0 and ws(1, 1, 0, 2) > 0
    for args in ((0, 12, 5, 512), (8, 0, 5, 512), (8, (1 << 22) + 1, 5, 512), (8, 12, -1, 512), (8, 12, (1 << 26) + 1, 512), (8, 12, 5, 1),
                 (8, 12, 5, 4097)):
        assert ws(*args) == 0, args


@pytest.mark.parametrize("Q", [0, 1, 3, 4, 63, 65, 257, 4099, 100000, 1 << 24, 1 << 26])
def test_workspace_size_is_the_carve_of_the_layout(Q):
    got = _lib().pdhip_mesh_contains_workspace_bytes(1000, 2000, Q, 512)
    print(Q, got, oc.contains_workspace_bytes(Q))
    assert got == oc.contains_workspace_bytes(Q)
    assert got == _lib().pdhip_mesh_contains_workspace_bytes(7, 1 << 22, Q, 64)      # a function of Q alone


def test_compute_iou_host_arithmetic():
    from pointdreamer_amd import geometry_metrics as G
    for inter, union in ((0, 5), (5, 5), (1, 3), (1627, 2880), (33333, 100000), ((1 << 24) - 1, 1 << 24)):
        want = float(np.float32(inter) / np.float32(union))
        assert G.iou_from_counts(inter, union) == want
        assert want == float(np.float32(inter / union))         # the counts are exact in float32: the quotient is the rounded true quotient
    assert G.iou_from_counts(1, 3) == float(np.float32(1) / np.float32(3)) != 1 / 3
    assert np.isnan(G.iou_from_counts(0, 0))


def test_product_has_no_cpu_path():
    import torch
    from pointdreamer_amd import _lib, geometry_metrics as G
    v, f, p = torch.zeros((4, 3)), torch.zeros((1, 3), dtype=torch.int64), torch.zeros((5, 3))
    with pytest.raises(_lib.PdhipError):
        G.check_mesh_contains(v, f, p)
    with pytest.raises(_lib.PdhipError):
        G.compute_iou(torch.zeros(5), torch.zeros(5))
    with pytest.raises(_lib.PdhipError):
        G.compute_iou(np.zeros(5), np.zeros(5))


def test_no_scratch_on_the_occupancy_kernels():
    if not os.path.exists(LIB):
        _lib()
    pytest.importorskip('msgpack')                          # (as tests/test_code_objects_cpu.py: the metadata note is msgpack)
    from tools import code_object_notes
    shared = ('k_point_box', 'k_cell_keys', 'k_cell_starts', 'k_gather_xyzi')      # csrc/cell_list.h: every including unit's copy is looked at
    mine = [k for k in code_object_notes.kernels(LIB) if 'k_occ_' in k['name'] or any(s in k['name'] for s in shared)]
    names = ' '.join(k['name'] for k in mine)
    for must in ('k_point_box', 'OcKey', 'k_occ_gather', 'k_cell_starts', 'k_occ_tri', 'k_occ_finish', 'k_occ_counts', 'k_occ_iou'):
        assert must in names, must
    for k in mine:
        print(k['name'], 'vgprs', k['vgpr_count'], 'lds', k['group_segment_fixed_size'], 'scratch', k['private_segment_fixed_size'])
        assert k['arch'] == 'gfx950'
        assert k['vgpr_spill_count'] == 0 and k['private_segment_fixed_size'] == 0, k
