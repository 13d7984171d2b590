"""Taubin lambda | mu smoothing of a mesh on the device, with uniform ("umbrella") weights, and the boundary vertices of a mesh
(csrc/mesh_smooth.hip; include/pdhip.h has the contracts).  The reference has no counterpart: there POCO absorbs the cloud's noise.  The marching-cubes
mesh of spr.py carries what is left of it, and MeshLab users run "Taubin Smooth" on it; this is that filter, and the plain Laplacian it is built from.

  boundary_vertices(faces, num_vertices, return_counts=False)                                                    -> [Vn] bool[, counts]
  taubin_smooth(vertices, faces, steps=10, lam=0.5, mu=-0.53, boundary='fixed', fixed=None, return_counts=False) -> [Vn,3] f32[, counts]
  laplacian_smooth(vertices, faces, steps=1, lam=0.5, boundary='fixed', fixed=None, return_counts=False)         -> the same with mu = 0

Only vertices move: faces and colours stay as they are.  The result is bit-equal to the f64 definition of include/pdhip.h; it does not depend on the
order of the faces, but it is not invariant under relabelling the vertices (each sum runs in index order).  CPU tensors raise PdhipError: there is no
CPU path."""
import math

import torch

from . import _lib, mesh_utils
from ._lib import ptr, rows, stream, check, PdhipError

DEFAULT_STEPS, DEFAULT_LAMBDA, DEFAULT_MU = 10, 0.5, -0.53             # MeshLab's "Taubin Smooth" defaults
MAX_STEPS = 10000


def check_params(steps, lam, mu):
    """ValueError unless (steps, lam, mu) is what pdhip_smooth_mesh accepts; -> (int, float, float).  The rules are the entry's own, here so that a
    caller with a long stage in front of the smoothing (spr.py, demo.py) can refuse before it."""
    if isinstance(steps, bool) or not isinstance(steps, int) or not 1 <= steps <= MAX_STEPS:
        raise ValueError(f"steps={steps!r}: the smoothing steps are an integer in 1 .. {MAX_STEPS}")
    for name, x in (('lam', lam), ('mu', mu)):
        if isinstance(x, bool) or not isinstance(x, (int, float)):
            raise ValueError(f"{name}={x!r}: a number")
    lam, mu = float(lam), float(mu)
    if not 0.0 < lam <= 1.0:
        raise ValueError(f"lam={lam!r} is not in (0, 1]")
    if not (math.isfinite(mu) and mu <= 0.0):
        raise ValueError(f"mu={mu!r}: a finite number <= 0 (0: the plain Laplacian)")
    if mu != 0.0 and not mu < -lam:
        raise ValueError(f"lam={lam!r}, mu={mu!r} is not a Taubin pair: mu < -lam keeps the pass band 1/lam + 1/mu positive")
    if abs((1.0 - 2.0 * lam) * (1.0 - 2.0 * mu)) > 1.0:
        raise ValueError(f"lam={lam!r}, mu={mu!r} amplify the highest frequency: |(1 - 2 lam)(1 - 2 mu)| > 1")
    return steps, lam, mu


def _faces(faces, what):
    return rows(faces, what, 'faces [F,3]', 3, torch.int64)


def _csr(num_vertices, f):
    rowptr, colidx = mesh_utils.neighbour_csr(num_vertices, f)
    if colidx.numel() == 0:                                        # (every face degenerate: a non-null pointer for the empty array)
        colidx = torch.zeros((8,), dtype=torch.int32, device=f.device)
    return rowptr, colidx.contiguous()


def _boundary(f, Vn, rowptr, colidx):
    pair_faces = torch.empty((max(int(colidx.shape[0]), 8),), dtype=torch.int32, device=f.device)
    mask = torch.empty((Vn,), dtype=torch.uint8, device=f.device)
    counts = torch.empty((4,), dtype=torch.int32, device=f.device)
    check(_lib.lib().pdhip_mesh_boundary_vertices(ptr(f), f.shape[0], Vn, ptr(rowptr), ptr(colidx), ptr(pair_faces), ptr(mask), ptr(counts), stream()),
          'pdhip_mesh_boundary_vertices')
    return mask, counts


def boundary_vertices(faces, num_vertices, return_counts=False):
    """faces [F,3] (GPU) -> [Vn] bool on the device: the vertices with an edge that lies on exactly one face (an edge on three faces or more is not a
    boundary edge).  return_counts: a second result, dict(boundary_vertices, boundary_edges, nonmanifold_edges).  Synchronises."""
    f = _faces(faces, 'boundary_vertices')
    Vn = int(num_vertices)
    rowptr, colidx = _csr(Vn, f)
    mask, counts = _boundary(f, Vn, rowptr, colidx)
    if return_counts:
        nb, ne, nm, _ = counts.tolist()
        return mask.view(torch.bool), dict(boundary_vertices=nb, boundary_edges=ne, nonmanifold_edges=nm)
    return mask.view(torch.bool)


def taubin_smooth(vertices, faces, steps=DEFAULT_STEPS, lam=DEFAULT_LAMBDA, mu=DEFAULT_MU, boundary='fixed', fixed=None, return_counts=False):
    """vertices [Vn,3], faces [F,3] (GPU) -> the smoothed vertices [Vn,3] f32: `steps` times a Laplacian pass with factor lam and, unless mu == 0,
    one with mu (< -lam: it undoes the shrinkage of the first).  boundary: 'fixed' holds the boundary vertices (boundary_vertices) in place, 'free'
    moves them like the rest.  fixed: [Vn] bool / uint8 on the GPU, further vertices to hold.  A vertex no face names is copied.  return_counts: a
    second result, dict(moved, held, isolated, steps).  Synchronises."""
    what = 'taubin_smooth'
    steps, lam, mu = check_params(steps, lam, mu)
    if boundary not in ('fixed', 'free'):
        raise ValueError(f"boundary={boundary!r}: 'fixed' (boundary vertices stay) or 'free'")
    f = _faces(faces, what)
    if fixed is not None and not (torch.is_tensor(fixed) and fixed.is_cuda):
        raise PdhipError(f"{what} needs tensors on the GPU (cuda:N == HIP device); there is no CPU path")
    v = rows(vertices, what, 'vertices [Vn,3]', 3, torch.float32)
    Vn, dev = v.shape[0], v.device
    if fixed is not None and tuple(fixed.shape) != (Vn,):
        raise PdhipError(f"{what}: fixed {tuple(fixed.shape)} for {Vn} vertices")
    rowptr, colidx = _csr(Vn, f)
    held = None
    if boundary == 'fixed':
        held = _boundary(f, Vn, rowptr, colidx)[0]
    if fixed is not None:
        user = (fixed.detach() != 0).view(torch.uint8)
        held = user if held is None else held | user
    state = torch.empty((2, Vn, 4), dtype=torch.float64, device=dev)
    out = torch.empty_like(v)
    counts = torch.empty((4,), dtype=torch.int32, device=dev)
    check(_lib.lib().pdhip_smooth_mesh(ptr(v), Vn, ptr(rowptr), ptr(colidx), ptr(held, allow_none=True), steps, lam, mu, ptr(state[0]), ptr(state[1]),
                                       ptr(out), ptr(counts), stream()), 'pdhip_smooth_mesh')
    if return_counts:
        moved, nheld, isolated, _ = counts.tolist()
        return out, dict(moved=moved, held=nheld, isolated=isolated, steps=steps)
    return out


def laplacian_smooth(vertices, faces, steps=1, lam=DEFAULT_LAMBDA, boundary='fixed', fixed=None, return_counts=False):
    """taubin_smooth with mu = 0: the plain umbrella Laplacian, which shrinks the shape a little with every step."""
    return taubin_smooth(vertices, faces, steps=steps, lam=lam, mu=0.0, boundary=boundary, fixed=fixed, return_counts=return_counts)
