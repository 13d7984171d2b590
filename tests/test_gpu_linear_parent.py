"""The Delaunay-linear fill returns the bytes it returned before k_linear_tri and k_linear_local were given one query step, one arg-max merge and
one barycentric store (csrc/linear.hip): `out`, `tri` and the workspace's integers of every case of tests/linear_parent_common.py, in each of the
three `local` modes, have the SHA-256 that tools/record_linear_digests.py recorded with the parent commit's library
(tests/golden/linear_parent.json).  Equality, no tolerance: a digest that differs is a changed tie rule, pivot choice or expression grouping.  Every
case is launched twice on one workspace and must return the same bytes both times."""
import json

import pytest
import torch

import linear_parent_common as lp

pytestmark = pytest.mark.gpu
DIGESTS = ('out', 'tri', 'ints')


@pytest.fixture(scope="module")
def recorded():
    with open(lp.GOLDEN) as fh:
        return json.load(fh)


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available()
    from pointdreamer_amd import _lib
    _lib.lib()
    return _lib


def test_every_case_is_recorded(recorded):
    assert sorted(recorded) == sorted(f"{name}-local{local}" for name, local in lp.IDS)
    assert not [k for k, v in recorded.items() if 'second_launch' in v], "a case whose two parent launches differed"


def test_the_list_reaches_every_path(recorded):
    """What the parent did on the case list (its recorded integers and where its `tri` says the queries ended): every exit of the query step and
    every kernel behind it is taken by some case."""
    rec = {(name, local): recorded[f"{name}-local{local}"] for name, local in lp.IDS}
    assert any(sum(r['fbcount']) > 0 for (_, local), r in rec.items() if local == 1), "the global kernel finished nothing behind the two windows"
    assert any(r['bcount'] > 0 and r['boundary_nan'] > 0 and r['boundary_segment'] > 0 for r in rec.values()), \
        "k_linear_boundary: no case with a query beyond the last site of its hull edge (-2) and one between two sites (tri[1] == tri[2])"
    assert any(r['tri_nan'] > 0 for r in rec.values()), "no query left k_linear_tri outside the hull (state 2)"
    shapes = [m[0].shape for m, _, _ in lp.CASES.values()]
    assert any(H % 8 and W % 8 and H % 16 and W % 16 for H, W in shapes), "no ragged 8x8 and 16x16 tiles"
    assert any(0 in r['ns'] for r in rec.values()), "no image without a site"
    assert all(r['unresolved'] == 0 for r in rec.values())
    # what the issue lists besides: two images with different masks, an f32 mask, one channel
    assert any(len(m) == 2 and not (m[0] == m[1]).all() for m, _, _ in lp.CASES.values())
    assert any(dt is lp.np.float32 for _, _, dt in lp.CASES.values()) and any(Cn == 1 for _, Cn, _ in lp.CASES.values())


@pytest.mark.parametrize("name,local", lp.IDS, ids=[f"{name}-local{local}" for name, local in lp.IDS])
def test_parent_bytes(lib, recorded, name, local):
    first, second = lp.run_case(lib.lib(), lib, name, local)
    print(f"{name}-local{local}: " + ' '.join(f"{k}={v}" for k, v in first.items() if k not in DIGESTS))
    assert second == first, f"{name}: the second launch on the same workspace returned other bytes"
    want = recorded[f"{name}-local{local}"]
    differ = [k for k in DIGESTS if first[k] != want[k]]
    assert not differ, f"{name} local={local}: other bytes than the parent commit's in {differ}: " \
                       f"{ {k: (first[k], want[k]) for k in first if k not in DIGESTS and first[k] != want[k]} }"
