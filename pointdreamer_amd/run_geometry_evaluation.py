"""Geometry scores of a tree of results against sampled ground truth, on the device (the loop round MeshEvaluator.eval_mesh of
models/POCO/eval/src/eval.py, in the layout of this project's other tools):

  python -m pointdreamer_amd.run_geometry_evaluation --pred_root_path <out_root> --gt_root_path <data_root>/pc_kaolin

Every <cls_id>/<shape_name>/models/model_normalized.obj under the prediction root is read with io_utils.load_obj_mesh, sampled with
`--n_points` points (seeded by `--seed`) and scored against <gt_root>/<cls_id>/<shape_name>/coords.npy + normals.npy, the files
sample_colored_pc_from_mesh writes.  One line per shape, then the mean over the shapes; the result also goes to
`<parent of pred root>/<time>_geometry_eval_result.txt`.  A shape without ground truth is a FileNotFoundError that names it.
With `--points_root_path <data_root>/point` every shape that has <cls_id>/<shape_name>.npz there (points + packed occupancies, written by
`sample_colored_pc_from_mesh --occupancy`) is also scored by the volumetric IoU: an `iou` column, its mean over the shapes that have one.
With `--p2m` every shape is also scored by the completeness of the ground-truth cloud against the predicted SURFACE (geometry_metrics.P2M_KEYS:
mean distance, mean squared distance, normal consistency): three more columns and their means."""
import argparse
import os
import time

import numpy as np
import torch

from . import geometry_metrics, io_utils
from .run_evaluation import shape_names

KEYS = ('chamfer-L1', 'chamfer-L2', 'completeness', 'accuracy', 'normals', 'f-score', 'f-score-15', 'f-score-20')
MESH = os.path.join('models', 'model_normalized.obj')


def eval(pred_root_path, gt_root_path, n_points=100000, seed=0, device=None, points_root_path=None, p2m=False):
    """Returns dict(per_shape={name: the twelve scores}, mean={key: mean over the shapes}, sample_num, result_file).  points_root_path
    (<data_root>/point, what sample_colored_pc_from_mesh --occupancy writes): a shape with <cls_id>/<shape_name>.npz there is also scored
    by `iou`, and the mean of that column runs over those shapes (NaN when there is none).  p2m: the three point-to-mesh completeness scores as well."""
    device = device if device is not None else torch.device('cuda')
    names = [n for n in shape_names(pred_root_path) if os.path.exists(os.path.join(pred_root_path, n, MESH))]
    if not names:
        raise FileNotFoundError(f'no <cls_id>/<shape_name>/{MESH} under {pred_root_path}')
    per_shape = {}
    shown = KEYS + ('iou',) if points_root_path is not None else KEYS
    if p2m:
        shown = shown + geometry_metrics.P2M_KEYS
    print('shape\t' + '\t'.join(shown))
    for name in names:
        gt = [os.path.join(gt_root_path, name, f) for f in ('coords.npy', 'normals.npy')]
        for p in gt:
            if not os.path.exists(p):
                raise FileNotFoundError(f'{name}: no ground truth {p}')
        vertices, faces = io_utils.load_obj_mesh(os.path.join(pred_root_path, name, MESH))
        coords, normals = (torch.from_numpy(np.load(p).astype(np.float32)).to(device) for p in gt)
        occ_file = os.path.join(points_root_path, name + '.npz') if points_root_path is not None else None
        iou_args = {}
        if occ_file is not None and os.path.exists(occ_file):
            with np.load(occ_file) as z:
                iou_args = dict(points_iou=z['points'].astype(np.float32), occ_tgt=z['occupancies'])
        r = geometry_metrics.eval_mesh(torch.from_numpy(vertices).to(device), torch.from_numpy(faces).to(device), coords, normals,
                                       n_points=n_points, seed=seed, p2m=p2m, **iou_args)
        per_shape[name] = r
        print(name + '\t' + '\t'.join(repr(float(r.get(k, float('nan')))) for k in shown))
    keys = list(next(iter(per_shape.values())))
    if points_root_path is not None and 'iou' not in keys:
        keys.append('iou')
    have = lambda k: [float(r[k]) for r in per_shape.values() if k in r]
    mean = {k: float(np.mean(have(k))) if have(k) else float('nan') for k in keys}
    print('-----------------------------------------')
    print('pred_root_path', pred_root_path)
    print('gt_root_path', gt_root_path)
    if points_root_path is not None:
        print('points_root_path', points_root_path, 'shapes with iou', len(have('iou')))
    print('sample num', len(names))
    print('\t'.join(shown))
    print('\t'.join(repr(mean[k]) for k in shown))
    print('-----------------------------------------')
    now = time.strftime("%Y_%m_%d %H.%M.%S\n", time.localtime())
    result_file = os.path.join(os.path.dirname(os.path.abspath(pred_root_path).rstrip(os.sep)), f'{now.strip()}_geometry_eval_result.txt')
    with open(result_file, "a", encoding="utf-8") as f:
        f.write(now + f'pred root path: {pred_root_path}\nGT root path: {gt_root_path}\nsample num: {len(names)}\n'
                f'n_points: {n_points}\nseed: {seed}\n' + '\t'.join(keys) + '\n' + '\t'.join(repr(mean[k]) for k in keys) + '\t\n')
    return dict(per_shape=per_shape, mean=mean, sample_num=len(names), result_file=result_file)


def main(argv=None):
    p = argparse.ArgumentParser("run geometry evaluation")
    p.add_argument("--pred_root_path", type=str, required=True, help="root of the results: <cls_id>/<shape>/models/model_normalized.obj")
    p.add_argument("--gt_root_path", type=str, required=True, help="<data_root>/pc_kaolin: <cls_id>/<shape>/coords.npy + normals.npy")
    p.add_argument("--n_points", type=int, default=100000)
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--points_root_path", type=str, default=None,
                   help="<data_root>/point: <cls_id>/<shape>.npz with points + occupancies (sample_colored_pc_from_mesh --occupancy) -> the iou column")
    p.add_argument("--p2m", action="store_true",
                   help="also the completeness of the ground-truth cloud against the predicted surface itself (point to mesh): three more columns")
    args = p.parse_args(argv)
    return eval(args.pred_root_path, args.gt_root_path, args.n_points, args.seed, points_root_path=args.points_root_path, p2m=args.p2m)


if __name__ == '__main__':
    main()
