"""The conv kernels return the bytes they returned before their tails were given one split-K hand-off and one GroupNorm octet reduce
(csrc/nn_conv_tail.h): y and the octet partials of every case of tests/conv_tail_common.py -- the case list of the conv-epilogue tests, every kernel
with one split / slab and with several -- have the SHA-256 that tools/record_conv_tail_digests.py recorded with the parent commit's library
(tests/golden/conv_tail_parent.json).  Equality, no tolerance: a digest that differs is a changed summation order or a changed address.  Every case is
launched twice on one workspace; the second launch finds the tickets as the first left them and must return the same bytes."""
import json

import pytest
import torch

import conv_tail_common as ct

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def recorded():
    with open(ct.GOLDEN) as fh:
        return json.load(fh)


@pytest.fixture(scope="module")
def L():
    assert torch.cuda.is_available()
    from pointdreamer_amd import _lib
    import pointdreamer_amd.ddnm_inpainting  # noqa: F401  (registers the entry points)
    return _lib.lib()


def test_every_case_is_recorded(recorded):
    assert sorted(recorded) == sorted(c['name'] for c in ct.CASES)


def test_the_list_holds_every_tail_with_one_split_and_with_several():
    """What the case list must contain (the kernels' own constants: k_conv_sk's 128-row tiles 1 and 2, k_conv_rr's variant 5 = 64 data rows in 128 row slots)."""
    cs = ct.CASES
    for k, several in (('sk', lambda c: c['sk'][2] > 1), ('rr', lambda c: c['rr'][1] > 1), ('ht', lambda c: c['ht'][1] > 1)):
        mine = [c for c in cs if c['kernel'] == k]
        assert any(several(c) for c in mine) and any(not several(c) for c in mine), k
    assert any(c['kernel'] == 'sk' and c['sk'][1] in (1, 2) and c['H'] * c['W'] == 64 and c['N'] >= 2 and c['N'] % 2 == 1 and c['chunks'] for c in cs), \
        "k_conv_sk: two 8x8 images per 128-row tile, the last tile's second segment past the batch"
    assert any(c['kernel'] == 'rr' and c['rr'][0] == 5 and c['chunks'] for c in cs), "k_conv_rr: fewer data rows than rows per pass"
    assert any(c['kernel'] == 'igemm' and c['splits'] == 0 and c['chunks'] for c in cs) and any(c['kernel'] == 'phase' and c['chunks'] for c in cs)
    assert any(c['kernel'] == 'halo' and c['splits'] == 0 for c in cs) and any(c['kernel'] == 'halo' and c['splits'] > 1 for c in cs)


@pytest.mark.parametrize("c", ct.CASES, ids=[c['name'] for c in ct.CASES])
def test_parent_bytes(L, recorded, c):
    first, second = ct.run_case(L, c)
    assert first['kernel'] == ct.ce.KERNELS[c['kernel']], f"routed to kernel {first['kernel']}"
    assert second == first, f"{c['name']}: the second launch on the same workspace returned other bytes"
    want = recorded[c['name']]
    differ = [k for k in sorted(want) if first[k] != want[k]]
    assert not differ, f"{c['name']}: other bytes than the parent commit's in {differ}"
