"""Exact k nearest neighbours and statistical outlier removal on the device (csrc/knn.hip; include/pdhip.h has the contract).  The reference has no
counterpart: its `input_already_noisy` only picks a POCO weight set.  The filter is the one of PCL (StatisticalOutlierRemoval) and Open3D
(remove_statistical_outlier): the mean distance to the k nearest neighbours per point, and the points above mean + ratio * std of it removed.

  knn_points(queries, targets, k)                 -> (d2 [Q,k] float64, idx [Q,k] int32): per query the k smallest (d2, index) pairs, ascending, equal
                                                     to the brute-force f64 scan + stable sort bit for bit
  statistical_outlier_mask(points, nb_neighbors=20, std_ratio=2.0)            -> keep [N] bool
  remove_statistical_outliers(points, colors=None, nb_neighbors=20, std_ratio=2.0) -> (points[kept], colors[kept] or None, kept_idx [kept] int64)

CPU tensors raise PdhipError: there is no CPU path."""
import torch

from . import _lib
from ._lib import ptr, stream, check

MAX_NEIGHBORS = 63                     # (the point itself takes one of pdhip_knn_max_k() = 64 slots)


def _cloud(x, what):
    if not (torch.is_tensor(x) and x.is_cuda):
        raise _lib.PdhipError(f"outliers: expected {what} on the GPU; pointdreamer_amd has no CPU path")
    if x.dim() != 2 or x.shape[1] != 3:
        raise ValueError(f"{what} must be [N, 3], got {tuple(x.shape)}")
    return x.detach().to(torch.float32).contiguous()


def knn_points(queries, targets, k, return_counts=False):
    """(d2 [Q,k] float64, idx [Q,k] int32) of queries [Q,3] against targets [M,3], both on the GPU.  return_counts: also the int32 [4] tensor
    (queries certified by the ring scan, queries finished by the sweep of all targets, cells per axis, 0)."""
    L = _lib.lib()
    q, t = _cloud(queries, 'queries'), _cloud(targets, 'targets')
    Q, M, k, dev = q.shape[0], t.shape[0], int(k), q.device
    d2 = torch.empty((Q, max(k, 0)), dtype=torch.float64, device=dev)
    idx = torch.empty((Q, max(k, 0)), dtype=torch.int32, device=dev)
    counts = torch.zeros((4,), dtype=torch.int32, device=dev)
    ws = torch.empty((max(int(L.pdhip_knn_points_workspace_bytes(Q, M, k)), 8),), dtype=torch.uint8, device=dev)   # (0: the entry refuses the sizes)
    opt = lambda x: ptr(x) if x.numel() else ptr(None, allow_none=True)
    check(L.pdhip_knn_points(opt(q), Q, opt(t), M, k, opt(d2), opt(idx), ptr(counts), ptr(ws), stream()), 'pdhip_knn_points')
    return (d2, idx, counts) if return_counts else (d2, idx)


def sor_filter(knn_d2, std_ratio):
    """pdhip_sor_filter over knn_d2 [N,kk] float64 (the (k+1)-NN of a cloud against itself) -> (mean_d [N] f64, stats [4] f64 = mu, sigma, t, 0,
    keep [N] uint8, kept_idx [N] int32 of which counts[0] are valid, counts [4] int32 = kept, removed, 0, 0), all on the device."""
    L = _lib.lib()
    if not (torch.is_tensor(knn_d2) and knn_d2.is_cuda):
        raise _lib.PdhipError("outliers: expected knn_d2 on the GPU; pointdreamer_amd has no CPU path")
    if knn_d2.dim() != 2:
        raise ValueError(f"knn_d2 must be [N, k + 1], got {tuple(knn_d2.shape)}")
    d = knn_d2.detach().to(torch.float64).contiguous()
    N, kk, dev = d.shape[0], d.shape[1], d.device
    mean_d = torch.empty((N,), dtype=torch.float64, device=dev)
    stats = torch.empty((4,), dtype=torch.float64, device=dev)
    keep = torch.empty((N,), dtype=torch.uint8, device=dev)
    kept_idx = torch.empty((N,), dtype=torch.int32, device=dev)
    counts = torch.empty((4,), dtype=torch.int32, device=dev)
    ws = torch.empty((max(int(L.pdhip_sor_filter_workspace_bytes(N)), 8),), dtype=torch.uint8, device=dev)
    opt = lambda x: ptr(x) if x.numel() else ptr(None, allow_none=True)
    check(L.pdhip_sor_filter(opt(d), N, kk, float(std_ratio), opt(mean_d), ptr(stats), opt(keep), opt(kept_idx), ptr(counts), ptr(ws), stream()),
          'pdhip_sor_filter')
    return mean_d, stats, keep, kept_idx, counts


def _filter(points, nb_neighbors, std_ratio):
    p = _cloud(points, 'points')
    N = p.shape[0]
    if isinstance(nb_neighbors, bool) or not isinstance(nb_neighbors, int) or not 1 <= nb_neighbors <= min(MAX_NEIGHBORS, N - 1):
        raise ValueError(f"nb_neighbors={nb_neighbors!r}: an integer in 1 .. min({MAX_NEIGHBORS}, N - 1) = {min(MAX_NEIGHBORS, N - 1)}")
    d2, _ = knn_points(p, p, nb_neighbors + 1)
    return sor_filter(d2, std_ratio)


def statistical_outlier_mask(points, nb_neighbors=20, std_ratio=2.0, return_stats=False):
    """keep [N] bool of points [N,3] on the GPU: True where the mean distance to the nb_neighbors nearest other points is <= mean + std_ratio * std
    of that quantity over the cloud.  return_stats: also a dict with mean, std, threshold (floats), kept, removed (ints) and mean_d ([N] float64 on
    the device)."""
    mean_d, stats, keep, _, counts = _filter(points, nb_neighbors, std_ratio)
    mask = keep.view(torch.bool)
    if not return_stats:
        return mask
    s, c = stats.tolist(), counts.tolist()
    return mask, dict(mean=s[0], std=s[1], threshold=s[2], kept=c[0], removed=c[1], mean_d=mean_d)


def remove_statistical_outliers(points, colors=None, nb_neighbors=20, std_ratio=2.0, return_stats=False):
    """(points[kept], colors[kept] or None, kept_idx [kept] int64, ascending) of a cloud on the GPU.  return_stats: also statistical_outlier_mask's dict
    with the mask under 'keep'."""
    if colors is not None and not (torch.is_tensor(colors) and colors.is_cuda):
        raise _lib.PdhipError("outliers: expected colors on the GPU; pointdreamer_amd has no CPU path")
    mean_d, stats, keep, kept_idx, counts = _filter(points, nb_neighbors, std_ratio)
    if colors is not None and colors.shape[0] != points.shape[0]:
        raise ValueError(f"colors {tuple(colors.shape)} do not match points {tuple(points.shape)}")
    s, c = stats.tolist(), counts.tolist()
    kept = kept_idx[:c[0]].to(torch.int64)
    out = (points[kept], colors[kept] if colors is not None else None, kept)
    if return_stats:
        out += (dict(mean=s[0], std=s[1], threshold=s[2], kept=c[0], removed=c[1], mean_d=mean_d, keep=keep.view(torch.bool)),)
    return out
