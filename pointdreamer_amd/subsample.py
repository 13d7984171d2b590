"""Farthest-point subsampling of a cloud on the device (csrc/subsample.hip; include/pdhip.h has the contract).  The reference ships no subsampler:
demo.py:371-374 refuses a cloud above 30 000 points and asks the user to subsample it first.

  farthest_point_sample(points, num, start=0) -> idx [num] int64 in pick order: idx[0] = start, every further pick the point farthest from the picks
                                                 before it (d2 in f64 of the f32 coordinates, the smallest index on a tie) -- the most even subset
                                                 a given count allows, equal to the brute-force scan bit for bit
  owner_mean_colors(points, colors, idx)      -> [num,3] float32: per sample the mean colour of the points nearest to it (pdhip_nearest_points, then
                                                 pdhip_owner_mean_colors: exact integer sums), the box filter that keeps 10^6 -> 30 000 from aliasing
  subsample_cloud(points, colors, num=30000, colors_from='point' | 'mean', start=0) -> (points[idx], colours, idx)

CPU tensors raise PdhipError: there is no CPU path."""
import torch

from . import _lib
from ._lib import ptr, stream, check

COLORS_FROM = ('point', 'mean')


def _cloud(x, what):
    if not (torch.is_tensor(x) and x.is_cuda):
        raise _lib.PdhipError(f"subsample: expected {what} on the GPU; pointdreamer_amd has no CPU path")
    if x.dim() != 2 or x.shape[1] != 3:
        raise ValueError(f"{what} must be [N, 3], got {tuple(x.shape)}")
    return x.detach().to(torch.float32).contiguous()


def farthest_point_sample(points, num, start=0, return_min_d2=False, return_counts=False):
    """idx [num] int64 of points [N,3] on the GPU, in pick order.  return_min_d2: also the float64 [num] tensor of each pick's squared distance to the
    picks before it (+inf for the first; sqrt of the last is the covering radius of the subset).  return_counts: also the int32 [4] tensor (cells per
    axis, occupied cells, point updates performed over all picks -- a brute-force scan performs N * num --, 0)."""
    p = _cloud(points, 'points')
    L = _lib.lib()
    N, M, dev = p.shape[0], int(num), p.device
    idx = torch.empty((max(M, 1),), dtype=torch.int32, device=dev)
    min_d2 = torch.empty((max(M, 1),), dtype=torch.float64, device=dev)
    counts = torch.zeros((4,), dtype=torch.int32, device=dev)
    ws = torch.empty((max(int(L.pdhip_fps_workspace_bytes(N, M)), 8),), dtype=torch.uint8, device=dev)     # (0: the entry refuses the sizes)
    check(L.pdhip_fps(ptr(p) if N else ptr(None, allow_none=True), N, M, int(start), ptr(idx), ptr(min_d2), ptr(counts), ptr(ws), stream()), 'pdhip_fps')
    out = (idx.to(torch.int64),)
    if return_min_d2:
        out += (min_d2,)
    if return_counts:
        out += (counts,)
    return out if len(out) > 1 else out[0]


def owner_mean_colors(points, colors, idx):
    """[M,3] float32: the mean colour of the points each sample points[idx] owns; a sample that owns nothing (a duplicate of an earlier sample)
    keeps its own colour."""
    from .geometry_metrics import nearest_points
    L = _lib.lib()
    p, c = _cloud(points, 'points'), _cloud(colors, 'colors')
    if c.shape[0] != p.shape[0]:
        raise ValueError(f"colors {tuple(c.shape)} do not match points {tuple(p.shape)}")
    idx = idx.to(torch.int64)
    N, M, dev = p.shape[0], idx.shape[0], p.device
    _, owner = nearest_points(p, p[idx].contiguous())
    fallback = c[idx].contiguous()
    out = torch.empty((M, 3), dtype=torch.float32, device=dev)
    ws = torch.empty((max(int(L.pdhip_owner_mean_colors_workspace_bytes(M)), 8),), dtype=torch.uint8, device=dev)
    check(L.pdhip_owner_mean_colors(ptr(owner, torch.int32), ptr(c), N, M, ptr(fallback), ptr(out), ptr(ws), stream()), 'pdhip_owner_mean_colors')
    return out


def subsample_cloud(points, colors, num=30000, colors_from='point', start=0, return_min_d2=False):
    """(points[idx], colours [num,3], idx [num] int64) of a cloud on the GPU.  colors_from 'point': the samples' own colours; 'mean': the mean over the
    points each sample stands for.  With N <= num the inputs come back with arange(N) and no kernel runs.  return_min_d2: also
    farthest_point_sample's min_d2 (None when nothing was subsampled)."""
    if colors_from not in COLORS_FROM:
        raise ValueError(f"colors_from={colors_from!r}: one of {COLORS_FROM}")
    if not (torch.is_tensor(points) and points.is_cuda and torch.is_tensor(colors) and colors.is_cuda):
        raise _lib.PdhipError("subsample: expected points and colors on the GPU; pointdreamer_amd has no CPU path")
    N = points.shape[0]
    if N <= int(num):
        out = (points, colors, torch.arange(N, dtype=torch.int64, device=points.device))
        return out + (None,) if return_min_d2 else out
    idx, min_d2 = farthest_point_sample(points, num, start=start, return_min_d2=True)
    cols = owner_mean_colors(points, colors, idx).to(colors.dtype) if colors_from == 'mean' else colors[idx]
    out = (points[idx], cols, idx)
    return out + (min_d2,) if return_min_d2 else out
