"""Records tests/golden/mesh_units_parent.json: the SHA-256 of every output of the mesh units' Python wrappers on the small seeded meshes of
tests/mesh_parent_bytes_common.py, computed on one MI355X with the library that is built at the moment.

  python tools/record_mesh_digests.py [out.json]      # default: tests/golden/mesh_units_parent.json

Run it BEFORE a refactor of uv_atlas / neighbor_mesh / simplify_mesh / mesh_components / mesh_smooth / mesh_clean / sample_mesh, with the parent
commit's library; tests/test_gpu_mesh_parent_bytes.py then holds the refactored library to these digests.  Every case runs twice in this
process; a case whose two runs differ is reported and left out (nothing can be held to it)."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)
import mesh_parent_bytes_common as C      # noqa: E402


def main(out):
    rec, dropped = {}, []
    for name in C.CASES:
        a, b = C.run_case(name), C.run_case(name)
        if a != b:
            dropped.append(name)
            print(f"{name}: two runs differ in {sorted(k for k in a if a[k] != b.get(k))}: left out", flush=True)
            continue
        rec[name] = a
        print(f"{name}: {len(a)} outputs", flush=True)
    with open(out, 'w') as fh:
        json.dump(rec, fh, indent=1, sort_keys=True)
        fh.write('\n')
    print(f"{len(rec)} cases -> {out}; dropped: {dropped}")


if __name__ == '__main__':
    main(sys.argv[1] if len(sys.argv) > 1 else C.GOLDEN)
