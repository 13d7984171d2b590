"""Golden vectors for the point-in-mesh test by RUNNING THE REFERENCE's check_mesh_contains (models/POCO/eval/src/utils/libmesh/inside_mesh.py with
its Cython triangle hash) on the CPU.  Build container only:  python -m tools.gen_golden_occupancy
triangle_hash.pyx is compiled with the local Cython into a temporary directory (the numpy include path goes to the compiler) and inside_mesh.py is
imported from the reference checkout next to it; nothing compiled or copied from the reference is kept.  numpy 2 dropped the alias np.bool that
inside_mesh.py uses: it is set before the import.  The mesh is handed over as an object with .vertices and .faces (trimesh is not needed).
Writes tests/golden/occupancy_ref.npz with the three cases of tests/occupancy_common.py:golden_inputs -- a noisy icosphere with 4 096 uniform
points, the uv sphere with 794 points on the xy of its vertices and edge midpoints, an open uv sphere with 4 096 points --: per case the float32
inputs, hash_resolution and the reference's bool output.  It also checks the all-pairs oracle of the tests against that output."""
import importlib.util
import os
import shutil
import sys
import tempfile
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import occupancy_common as oc                              # noqa: E402

REF = '/root/reference'
LIBMESH = os.path.join(REF, 'models', 'POCO', 'eval', 'src', 'utils', 'libmesh')
OUT = os.path.join(ROOT, 'tests', 'golden', 'occupancy_ref.npz')


def import_reference_inside_mesh(tmp):
    """The reference's inside_mesh module, its triangle_hash extension built under `tmp`."""
    from Cython.Build import cythonize
    from setuptools import Distribution, Extension
    pkg = os.path.join(tmp, 'libmesh_ref')
    os.makedirs(pkg)
    pyx = os.path.join(tmp, 'triangle_hash.pyx')
    shutil.copy(os.path.join(LIBMESH, 'triangle_hash.pyx'), pyx)
    ext = cythonize([Extension('triangle_hash', [pyx], include_dirs=[np.get_include()], language='c++')], build_dir=tmp, quiet=True)
    cmd = Distribution({'ext_modules': ext}).get_command_obj('build_ext')
    cmd.build_lib, cmd.build_temp = pkg, os.path.join(tmp, 'obj')
    cmd.ensure_finalized()
    cmd.run()
    if not hasattr(np, 'bool'):
        np.bool = bool
    package = types.ModuleType('libmesh_ref')
    package.__path__ = [pkg]
    sys.modules['libmesh_ref'] = package
    spec = importlib.util.spec_from_file_location('libmesh_ref.inside_mesh', os.path.join(LIBMESH, 'inside_mesh.py'))
    mod = importlib.util.module_from_spec(spec)
    sys.modules['libmesh_ref.inside_mesh'] = mod
    spec.loader.exec_module(mod)
    return mod


if __name__ == '__main__':
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        inside_mesh = import_reference_inside_mesh(tmp)
        for case in oc.GOLDEN_CASES:
            v, f, p, res = oc.golden_inputs(case)
            mesh = types.SimpleNamespace(vertices=np.array(v, np.float32), faces=np.array(f, np.int64))
            ref = np.asarray(inside_mesh.check_mesh_contains(mesh, np.array(p, np.float32), hash_resolution=res), bool)
            occ, counts = oc.oracle_contains(v, f, p, res, return_counts=True)
            print(case, 'faces', len(f), 'points', len(p), 'contained', int(ref.sum()), 'oracle counts', counts, 'oracle != reference',
                  int((occ != ref).sum()))
            assert np.array_equal(occ, ref), case
            out.update({f'{case}_vertices': np.asarray(v, np.float32), f'{case}_faces': np.asarray(f, np.int64),
                        f'{case}_points': np.asarray(p, np.float32), f'{case}_hash_resolution': np.int64(res), f'{case}_contains': ref})
    np.savez_compressed(OUT, **out)
    print('wrote', OUT, os.path.getsize(OUT), 'bytes')
