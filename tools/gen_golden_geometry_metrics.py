"""Golden vector for the geometry scores by RUNNING THE REFERENCE's MeshEvaluator.eval_pointcloud (models/POCO/eval/src/eval.py:91-213) on the
CPU.  Build container only:  python -m tools.gen_golden_geometry_metrics
eval.py imports trimesh, its compiled libmesh / libkdtree and eval.src.common at module level; none is installed or built here and
eval_pointcloud uses only the kd-tree: trimesh, libmesh and common are stubbed with empty modules, libkdtree.KDTree with scipy's cKDTree
(the same query(points) -> (distances, indices) call).
Writes tests/golden/geometry_metrics_ref.npz: a prediction of 4 096 points (a noisy torus) and a target of 3 500 (the torus) with normals,
float32-representable values handed to the reference as float64, and its twelve outputs.  The seed is the first for which no nearest
distance lies within 1e-9 of one of the 1 000 thresholds and no query has two targets at equal minimal d2
(tests/geometry_metrics_common.py:fixture_conditions): then neither the rounding of a square root nor a kd-tree's choice on a tie decides a score."""
import os
import sys
import types
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import geometry_metrics_common as gm                       # noqa: E402

REF = '/root/reference'
OUT = os.path.join(ROOT, 'tests', 'golden', 'geometry_metrics_ref.npz')
N_PRED, N_TGT = 4096, 3500


def import_reference_eval():
    from scipy.spatial import cKDTree
    sys.path.insert(0, os.path.join(REF, 'models', 'POCO'))
    sys.modules['trimesh'] = types.ModuleType('trimesh')
    kd = types.ModuleType('eval.src.utils.libkdtree')
    kd.KDTree = cKDTree
    mesh = types.ModuleType('eval.src.utils.libmesh')
    mesh.check_mesh_contains = None
    common = types.ModuleType('eval.src.common')
    common.compute_iou = None
    sys.modules['eval.src.utils.libkdtree'], sys.modules['eval.src.utils.libmesh'], sys.modules['eval.src.common'] = kd, mesh, common
    import importlib
    return importlib.import_module('eval.src.eval')


def clouds(seed):
    pred, n_pred = gm.solid_cloud('torus', N_PRED, 100 + seed, 0.004)
    tgt, n_tgt = gm.solid_cloud('torus', N_TGT, 200 + seed)
    return pred, n_pred, tgt, n_tgt


if __name__ == '__main__':
    ev = import_reference_eval()
    for seed in range(64):
        pred, n_pred, tgt, n_tgt = clouds(seed)
        gap, ties = gm.fixture_conditions(pred, tgt)
        print('seed', seed, 'smallest |distance - threshold|', gap, 'tied queries', ties)
        if gap > 1e-9 and ties == 0:
            break
    else:
        raise SystemExit('no seed satisfies the fixture conditions')
    f64 = lambda x: np.asarray(x, np.float32).astype(np.float64)
    out = ev.MeshEvaluator().eval_pointcloud(f64(pred), f64(tgt), f64(n_pred), f64(n_tgt))
    assert len(out) == 12
    for k, v in out.items():
        print(k, repr(float(v)))
    np.savez_compressed(OUT, pointcloud=np.asarray(pred, np.float32), normals=np.asarray(n_pred, np.float32),
                        pointcloud_tgt=np.asarray(tgt, np.float32), normals_tgt=np.asarray(n_tgt, np.float32), seed=np.int64(seed),
                        keys=np.array(list(out)), values=np.array([float(v) for v in out.values()], np.float64))
    print('wrote', OUT, os.path.getsize(OUT), 'bytes')
