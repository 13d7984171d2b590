"""The mesh units return the bytes they returned before they were given shared headers (csrc/union_find.h, csrc/mesh_common.h): every
output tensor and count of the Python wrappers, on the small seeded meshes of tests/mesh_parent_bytes_common.py, has the SHA-256 that
tools/record_mesh_digests.py recorded with the parent commit's library (tests/golden/mesh_units_parent.json).  Equality, no tolerance."""
import json

import pytest

import mesh_parent_bytes_common as C

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def recorded():
    with open(C.GOLDEN) as fh:
        return json.load(fh)


def test_every_case_is_recorded(recorded):
    assert sorted(recorded) == sorted(C.CASES)


@pytest.mark.parametrize("name", list(C.CASES))
def test_parent_bytes(recorded, name):
    got = C.run_case(name)
    want = recorded[name]
    assert sorted(got) == sorted(want)
    differ = [k for k in sorted(want) if got[k] != want[k]]
    assert not differ, f"{name}: other bytes than the parent commit's in {differ}"
