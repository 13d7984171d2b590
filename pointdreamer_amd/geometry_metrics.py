"""Geometry scores of a reconstruction on the device: models/POCO/eval/src/eval.py (MeshEvaluator.eval_pointcloud / eval_mesh,
distance_p2p, get_threshold_percentage) with the reference's names, keys and argument order.

  nearest_points(queries, targets)  -> (d2 [Q] float64, idx [Q] int32): the exact nearest target of every query (pdhip_nearest_points:
                                       d2 = (dx dx + dy dy) + dz dz in f64 of the f32 coordinates, the smallest index on a tie)
  eval_pointcloud(pointcloud, pointcloud_tgt, normals, normals_tgt, thresholds) -> the reference's dict
  eval_mesh(vertices, faces, pointcloud_tgt, normals_tgt, n_points, seed, rand) -> the same over n_points samples of the mesh
  check_mesh_contains(vertices, faces, points, hash_resolution) -> bool [Q]: the reference's point-in-mesh test
                                       (eval/src/utils/libmesh/inside_mesh.py; pdhip_mesh_contains, csrc/occupancy.hip)
  compute_iou(occ1, occ2)           -> the volumetric intersection over union of two occupancy arrays (eval/src/common.py:6-33)
  closest_on_mesh(vertices, faces, points) -> (d2 [Q] float64, face [Q] int32[, closest [Q,3] float64]): the exact closest point of the surface
                                       (trimesh.proximity.closest_point; pdhip_closest_on_mesh, csrc/mesh_distance.hip)
  distance_p2m(points, vertices, faces) -> sqrt(d2) [Q] float64 (eval.py:195-202 with the mesh as (vertices, faces))

Completeness is target -> prediction, accuracy is prediction -> target, each the mean over the points of its source cloud; the
normal entries are means of |n_src . n_tgt[nearest]| of the normalised normals; F = 2 P R / (P + R) with P / R the share of
accuracy / completeness distances <= the threshold.  The kernels (csrc/cloud_metrics.hip) leave per direction three f64 sums and the
integer counts per threshold; ONE device -> host copy per call brings them back, and the last handful of divisions are host Python.
Coordinates are float32 on the device (the reference casts the sampled cloud to float32 as well, eval.py:73).

`iou`, eval_mesh's fifth score (eval.py:83-87), is built from the two functions above: with `points_iou` and `occ_tgt` the prediction is tested
for containment at the points and compared with the ground-truth occupancies, which sample_colored_pc_from_mesh.sample_occupancy_batch
writes in the reference's .npz layout.  Without them the key is absent from the result.

eval_mesh(..., p2m=True) adds the completeness measured against the predicted SURFACE instead of its samples: 'completeness-p2m',
'completeness2-p2m' and 'normals completeness-p2m' are the mean distance, the mean squared distance and the mean |n_tgt . n_face| from the target
cloud to the mesh (distance_p2m's primitive, reduced by the same kernels with the faces in the place of the sampled points).

Not built: `remove_wall` (eval.py:48-69, a scene-dataset crop).  CPU tensors raise PdhipError: there is no CPU path."""
import math

import numpy as np
import torch

from . import _lib
from ._lib import ptr, stream, check

# eval.py:10-22, the values of an empty prediction (bounding box [-0.5, 0.5]^3)
EMPTY_PCL_DICT = {'completeness': math.sqrt(3), 'accuracy': math.sqrt(3), 'completeness2': 3, 'accuracy2': 3, 'chamfer': 6}
EMPTY_PCL_DICT_NORMALS = {'normals completeness': -1., 'normals accuracy': -1., 'normals': -1.}
DEFAULT_THRESHOLDS = np.linspace(1. / 1000, 1, 1000)


def _cloud(x, what, dev=None):
    """[N,3] float32 contiguous on the GPU (numpy arrays follow `dev`, the device of the call's first GPU tensor)."""
    if isinstance(x, np.ndarray) and dev is not None:
        x = torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    if not (torch.is_tensor(x) and x.is_cuda):
        raise _lib.PdhipError(f"geometry_metrics: expected {what} on the GPU; pointdreamer_amd has no CPU path")
    if x.dim() != 2 or x.shape[1] != 3:
        raise ValueError(f"{what} must be [N, 3], got {tuple(x.shape)}")
    return x.detach().to(torch.float32).contiguous()


def nearest_points(queries, targets, return_counts=False):
    """(d2 [Q] float64, idx [Q] int32) of queries [Q,3] against targets [M,3], both on the GPU (include/pdhip.h has the contract).
    return_counts: also the int32 [4] tensor (certified by the LDS phase -- 0 on the shipped path --, finished by the ring scan, cells per axis, 0)."""
    L = _lib.lib()
    q, t = _cloud(queries, 'queries'), _cloud(targets, 'targets')
    Q, M, dev = q.shape[0], t.shape[0], q.device
    d2 = torch.empty((Q,), dtype=torch.float64, device=dev)
    idx = torch.empty((Q,), dtype=torch.int32, device=dev)
    counts = torch.zeros((4,), dtype=torch.int32, device=dev)
    ws = torch.empty((max(int(L.pdhip_nearest_points_workspace_bytes(Q, M)), 8),), dtype=torch.uint8, device=dev)   # (0: the entry refuses the sizes)
    opt = lambda x: ptr(x) if x.numel() else ptr(None, allow_none=True)
    check(L.pdhip_nearest_points(opt(q), Q, opt(t), M, opt(d2), opt(idx), ptr(counts), ptr(ws), stream()), 'pdhip_nearest_points')
    return (d2, idx, counts) if return_counts else (d2, idx)


def cloud_sums(d2, idx, normals_src, normals_tgt, M, thresholds, out_sums, out_within):
    """pdhip_cloud_metrics into out_sums [4] float64 / out_within [T] int64 (views of the caller's result buffer)."""
    L = _lib.lib()
    T = thresholds.shape[0]
    ws = torch.empty((max(int(L.pdhip_cloud_metrics_workspace_bytes(T)), 8),), dtype=torch.uint8, device=d2.device)
    check(L.pdhip_cloud_metrics(ptr(d2, torch.float64), ptr(idx, torch.int32), d2.shape[0], ptr(normals_src, torch.float32, allow_none=True),
                                ptr(normals_tgt, torch.float32, allow_none=True), M, ptr(thresholds, torch.float64) if T else ptr(None, allow_none=True),
                                T, ptr(out_sums), ptr(out_within, allow_none=True), ptr(ws), stream()), 'pdhip_cloud_metrics')


def eval_pointcloud(pointcloud, pointcloud_tgt, normals=None, normals_tgt=None, thresholds=DEFAULT_THRESHOLDS):
    """eval.py:91-165 -> dict of python floats with the reference's twelve keys (the three normal entries are NaN without normals; an
    empty prediction returns the reference's constants)."""
    if pointcloud.shape[0] == 0:
        out = EMPTY_PCL_DICT.copy()
        if normals is not None and normals_tgt is not None:
            out.update(EMPTY_PCL_DICT_NORMALS)
        return out
    first = pointcloud if torch.is_tensor(pointcloud) else pointcloud_tgt
    dev = first.device if torch.is_tensor(first) and first.is_cuda else None
    pred, tgt = _cloud(pointcloud, 'pointcloud', dev), _cloud(pointcloud_tgt, 'pointcloud_tgt', dev)
    dev = pred.device
    with_normals = normals is not None and normals_tgt is not None
    n_pred = _cloud(normals, 'normals', dev) if with_normals else None
    n_tgt = _cloud(normals_tgt, 'normals_tgt', dev) if with_normals else None
    if with_normals and (n_pred.shape[0] != pred.shape[0] or n_tgt.shape[0] != tgt.shape[0]):
        raise ValueError(f"normals {tuple(n_pred.shape)} / {tuple(n_tgt.shape)} do not match the clouds {tuple(pred.shape)} / {tuple(tgt.shape)}")
    thr_host = np.ascontiguousarray(np.asarray(thresholds, dtype=np.float64).reshape(-1))
    if thr_host.shape[0] < 20:
        raise ValueError("thresholds: the reference reads entries 9, 14 and 19")
    thr = torch.from_numpy(thr_host).to(dev)
    T = thr.shape[0]
    # one result buffer of 8-byte words: [sums (4 f64) | within (T i64)] per direction, completeness first
    buf = torch.zeros((2 * (4 + T),), dtype=torch.int64, device=dev)
    for k, (src, dst, ns, nt) in enumerate(((tgt, pred, n_tgt, n_pred), (pred, tgt, n_pred, n_tgt))):
        d2, idx = nearest_points(src, dst)
        part = buf[k * (4 + T):(k + 1) * (4 + T)]
        cloud_sums(d2, idx, ns, nt, dst.shape[0], thr, part[:4].view(torch.float64), part[4:])
    host = buf.cpu()                                               # the one device -> host copy
    res = []
    for k, n in enumerate((tgt.shape[0], pred.shape[0])):
        part = host[k * (4 + T):(k + 1) * (4 + T)]
        sums = part[:4].view(torch.float64).tolist()
        within = part[4:].numpy()
        res.append((sums[0] / n, sums[1] / n, sums[2] / n if with_normals else float('nan'), within / float(n)))
    (completeness, completeness2, completeness_normals, recall), (accuracy, accuracy2, accuracy_normals, precision) = res
    with np.errstate(invalid='ignore', divide='ignore'):
        F = 2 * precision * recall / (precision + recall)          # (0 / 0 is NaN, as in the reference)
    return {
        'completeness': completeness,
        'accuracy': accuracy,
        'normals completeness': completeness_normals,
        'normals accuracy': accuracy_normals,
        'normals': 0.5 * completeness_normals + 0.5 * accuracy_normals,
        'completeness2': completeness2,
        'accuracy2': accuracy2,
        'chamfer-L2': 0.5 * (completeness2 + accuracy2),
        'chamfer-L1': 0.5 * (completeness + accuracy),
        'f-score': float(F[9]),        # threshold = 1.0%
        'f-score-15': float(F[14]),    # threshold = 1.5%
        'f-score-20': float(F[19]),    # threshold = 2.0%
    }


def sample_mesh_cloud(vertices, faces, n_points=100000, seed=0, rand=None):
    """(coords [n,3], face normals [n,3]) of n_points area-uniform samples of the mesh (pdhip_sample_mesh through sample_points).  The
    uniforms are `rand` [n,3] in [0,1), or torch.rand of a generator on the vertices' device seeded with `seed`."""
    from .sample_colored_pc_from_mesh import sample_points
    if not (torch.is_tensor(vertices) and vertices.is_cuda):
        raise _lib.PdhipError("geometry_metrics: expected vertices on the GPU; pointdreamer_amd has no CPU path")
    if rand is None:
        gen = torch.Generator(device=vertices.device)
        gen.manual_seed(int(seed))
        rand = torch.rand((int(n_points), 3), device=vertices.device, generator=gen)
    s = sample_points(vertices, faces, None, None, None, [{'Kd': np.zeros(3, np.float32)}], int(n_points), rand=rand)
    return s['coords'], s['normals']


def check_mesh_contains(vertices, faces, points, hash_resolution=512, return_counts=False):
    """inside_mesh.py:5-8 -> bool [Q] on the device: point q lies inside the mesh (include/pdhip.h has the definition; the result equals the
    reference's bit for bit).  vertices [Vn,3] on the GPU, faces [F,3] (a numpy array follows the vertices), points [Q,3] on the GPU or a
    numpy array, which follows the device of `vertices`.  return_counts: also the int32 [4] tensor (contained, points whose two ray
    parities disagree -- the reference's "contains1 != contains2" warning --, points outside the mesh's box, 0)."""
    L = _lib.lib()
    v = _cloud(vertices, 'vertices')
    dev = v.device
    p = _cloud(points, 'points', dev)
    f = _faces(faces, dev)
    Vn, F, Q, R = v.shape[0], f.shape[0], p.shape[0], int(hash_resolution)
    occ = torch.zeros((Q,), dtype=torch.uint8, device=dev)
    counts = torch.zeros((4,), dtype=torch.int32, device=dev)
    ws = torch.empty((max(int(L.pdhip_mesh_contains_workspace_bytes(Vn, F, Q, R)), 8),), dtype=torch.uint8, device=dev)   # (0: the entry refuses the sizes)
    opt = lambda x: ptr(x) if x.numel() else ptr(None, allow_none=True)
    check(L.pdhip_mesh_contains(opt(v), Vn, opt(f), F, opt(p), Q, R, opt(occ), ptr(counts), ptr(ws), stream()), 'pdhip_mesh_contains')
    occ = occ.view(torch.bool)
    return (occ, counts) if return_counts else occ


def _faces(faces, dev):
    """[F,3] int64 contiguous on the GPU (a numpy array follows `dev`)."""
    if isinstance(faces, np.ndarray):
        faces = torch.from_numpy(np.ascontiguousarray(faces)).to(dev)
    if not (torch.is_tensor(faces) and faces.is_cuda):
        raise _lib.PdhipError("geometry_metrics: expected faces on the GPU; pointdreamer_amd has no CPU path")
    if faces.dim() != 2 or faces.shape[1] != 3:
        raise ValueError(f"faces must be [F, 3], got {tuple(faces.shape)}")
    return faces.detach().to(torch.int64).contiguous()


def closest_on_mesh(vertices, faces, points, return_closest=False, return_counts=False):
    """trimesh.proximity.closest_point -> (d2 [Q] float64, face [Q] int32[, closest [Q,3] float64][, counts]) on the device: the squared distance
    of every point to the surface, the face that attains it (the smallest index on a tie) and the closest point of that face (include/pdhip.h has
    the definition; the result equals its all-pairs evaluation bit for bit).  vertices [Vn,3] on the GPU, faces [F,3] and points [Q,3] on the GPU
    or numpy arrays, which follow the device of `vertices`.  counts: the int32 [4] tensor (queries certified by the ring scan, queries finished by
    the scan of all faces, faces on the large list, degenerate faces skipped)."""
    L = _lib.lib()
    v = _cloud(vertices, 'vertices')
    dev = v.device
    p = _cloud(points, 'points', dev)
    f = _faces(faces, dev)
    Vn, F, Q = v.shape[0], f.shape[0], p.shape[0]
    d2 = torch.empty((Q,), dtype=torch.float64, device=dev)
    face = torch.empty((Q,), dtype=torch.int32, device=dev)
    closest = torch.empty((Q, 3), dtype=torch.float64, device=dev) if return_closest else None
    counts = torch.zeros((4,), dtype=torch.int32, device=dev)
    ws = torch.empty((max(int(L.pdhip_closest_on_mesh_workspace_bytes(Vn, F, Q)), 8),), dtype=torch.uint8, device=dev)   # (0: the entry refuses the sizes)
    opt = lambda x: ptr(x) if x is not None and x.numel() else ptr(None, allow_none=True)
    check(L.pdhip_closest_on_mesh(opt(v), Vn, opt(f), F, opt(p), Q, opt(d2), opt(face), opt(closest), ptr(counts), ptr(ws), stream()),
          'pdhip_closest_on_mesh')
    out = (d2, face)
    if return_closest:
        out += (closest,)
    if return_counts:
        out += (counts,)
    return out


def distance_p2m(points, vertices, faces):
    """eval.py:195-202 with the mesh as (vertices, faces) -> float64 [Q] on the device: the distance of every point to the surface."""
    return torch.sqrt(closest_on_mesh(vertices, faces, points)[0])


def face_normals(vertices, faces):
    """cross(b - a, c - a) of every face in float64 torch ops, cast to float32 [F,3] (not normalised: pdhip_cloud_metrics normalises in f64)."""
    tri = vertices.to(torch.float64)[faces]
    return torch.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0], dim=1).to(torch.float32).contiguous()


P2M_KEYS = ('completeness-p2m', 'completeness2-p2m', 'normals completeness-p2m')


def completeness_p2m(vertices, faces, pointcloud_tgt, normals_tgt):
    """{'completeness-p2m', 'completeness2-p2m', 'normals completeness-p2m'}: target cloud -> predicted mesh, reduced by pdhip_cloud_metrics with
    idx = face, M = F and the face normals as the targets' normals.  ONE device -> host copy."""
    v = _cloud(vertices, 'vertices')
    dev = v.device
    f = _faces(faces, dev)
    tgt = _cloud(pointcloud_tgt, 'pointcloud_tgt', dev)
    n_tgt = _cloud(normals_tgt, 'normals_tgt', dev) if normals_tgt is not None else None
    if n_tgt is not None and n_tgt.shape[0] != tgt.shape[0]:
        raise ValueError(f"normals_tgt {tuple(n_tgt.shape)} does not match pointcloud_tgt {tuple(tgt.shape)}")
    d2, face = closest_on_mesh(v, f, tgt)
    sums = torch.zeros((4,), dtype=torch.float64, device=dev)
    cloud_sums(d2, face, n_tgt, face_normals(v, f) if n_tgt is not None else None, f.shape[0], torch.zeros((0,), dtype=torch.float64, device=dev),
               sums, None)
    s = sums.cpu().tolist()                                        # the one device -> host copy
    n = tgt.shape[0]
    return {'completeness-p2m': s[0] / n, 'completeness2-p2m': s[1] / n,
            'normals completeness-p2m': s[2] / n if n_tgt is not None else float('nan')}


def iou_from_counts(intersection, union):
    """common.py:29-31 for one pair of arrays: the float32 quotient of the two counts (exact counts below 2^24); NaN for an empty union."""
    with np.errstate(invalid='ignore', divide='ignore'):
        return float(np.float32(intersection) / np.float32(union))


def _occupancy(x, what, dev):
    """[Q] uint8 0 / 1 on the device: bool and integer arrays as they are (nonzero = occupied), floating ones binarised at >= 0.5."""
    if isinstance(x, np.ndarray):
        if dev is None:
            raise _lib.PdhipError(f"geometry_metrics: expected {what} on the GPU; pointdreamer_amd has no CPU path")
        x = torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    if not (torch.is_tensor(x) and x.is_cuda):
        raise _lib.PdhipError(f"geometry_metrics: expected {what} on the GPU; pointdreamer_amd has no CPU path")
    x = x.detach().reshape(-1)
    x = (x >= 0.5) if x.dtype != torch.bool else x
    return x.to(torch.uint8).contiguous()


def compute_iou(occ1, occ2):
    """common.py:6-33 for one pair of occupancy arrays of equal size, binarised at >= 0.5 -> float.  The counts are taken on the device
    (pdhip_occupancy_iou) and come back in ONE device -> host copy."""
    L = _lib.lib()
    first = occ1 if torch.is_tensor(occ1) else occ2
    dev = first.device if torch.is_tensor(first) and first.is_cuda else None
    a, b = _occupancy(occ1, 'occ1', dev), _occupancy(occ2, 'occ2', dev)
    if a.shape[0] != b.shape[0]:
        raise ValueError(f"occ1 has {a.shape[0]} entries, occ2 {b.shape[0]}")
    out = torch.zeros((2,), dtype=torch.int64, device=a.device)
    opt = lambda x: ptr(x) if x.numel() else ptr(None, allow_none=True)
    check(L.pdhip_occupancy_iou(opt(a), opt(b), a.shape[0], ptr(out), stream()), 'pdhip_occupancy_iou')
    inter, union = out.cpu().tolist()                              # the one device -> host copy
    return iou_from_counts(inter, union)


def _occ_tgt(occ_tgt, Q, dev):
    """occ_tgt [Q] unpacked, or the .npz's np.packbits form (uint8 [ceil(Q / 8)], most significant bit first)."""
    if isinstance(occ_tgt, np.ndarray):
        occ_tgt = torch.from_numpy(np.ascontiguousarray(occ_tgt)).to(dev)
    n = occ_tgt.numel()
    if n != Q and occ_tgt.dtype == torch.uint8 and n == (Q + 7) // 8:
        shifts = torch.arange(7, -1, -1, dtype=torch.uint8, device=occ_tgt.device)
        occ_tgt = ((occ_tgt.reshape(-1, 1) >> shifts) & 1).reshape(-1)[:Q]
    if occ_tgt.numel() != Q:
        raise ValueError(f"occ_tgt has {n} entries for {Q} points (neither unpacked nor np.packbits of them)")
    return occ_tgt


def eval_mesh(vertices, faces, pointcloud_tgt, normals_tgt, n_points=100000, seed=0, rand=None, thresholds=DEFAULT_THRESHOLDS,
              points_iou=None, occ_tgt=None, p2m=False):
    """eval.py:37-89 without `remove_wall`: the scores of n_points samples of the mesh, their face normals as the prediction's normals.  A mesh
    without vertices or faces scores as the empty cloud.  With points_iou [Q,3] and occ_tgt (their ground-truth occupancies, [Q] or the
    np.packbits form of the .npz) the result gains 'iou' (0. for an empty mesh, eval.py:86-87); without them the key is absent.  p2m: the result
    gains P2M_KEYS, the completeness against the surface itself (completeness_p2m; the empty cloud's constants for an empty mesh), at the price of
    one more device -> host copy."""
    with_iou = points_iou is not None and occ_tgt is not None
    if vertices.shape[0] == 0 or faces.shape[0] == 0:
        out = eval_pointcloud(np.empty((0, 3)), pointcloud_tgt, np.empty((0, 3)), normals_tgt, thresholds)
        if with_iou:
            out['iou'] = 0.
        if p2m:
            out.update({'completeness-p2m': EMPTY_PCL_DICT['completeness'], 'completeness2-p2m': EMPTY_PCL_DICT['completeness2'],
                        'normals completeness-p2m': EMPTY_PCL_DICT_NORMALS['normals completeness']})
        return out
    coords, nrm = sample_mesh_cloud(vertices, faces, n_points, seed, rand)
    out = eval_pointcloud(coords, pointcloud_tgt, nrm, normals_tgt, thresholds)
    if with_iou:
        occ = check_mesh_contains(vertices, faces, points_iou)
        out['iou'] = compute_iou(occ, _occ_tgt(occ_tgt, occ.shape[0], occ.device))
    if p2m:
        out.update(completeness_p2m(vertices, faces, pointcloud_tgt, normals_tgt))
    return out
