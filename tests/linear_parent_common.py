"""Shared by tests/test_gpu_linear_parent.py and tools/record_linear_digests.py: the Delaunay-linear fill (csrc/linear.hip) launched through
pdhip_linear_fill with `tri` requested, on seeded, tiny images, each result reduced to a SHA-256.

tests/golden/linear_parent.json holds, per case and `local` mode, what the library of the commit before the two query kernels were given one step,
one arg-max merge and one store returned: the digests of `out` (int32 bit patterns, NaN included), of `tri`, and of the integers the unit leaves in
its workspace (unresolved, bcount, every image's fbcount[2b+1]) -- read at the offsets the carve log reports, as tests/workspace_common.py does.  A
query has one writer and its triangle does not depend on the order in which the atomics fill the fallback and boundary lists, so the bytes are
deterministic: a digest that differs is a changed tie rule, pivot choice or expression grouping.  test_gpu_workspace.py compares any valid runs of
one build; test_i0_linear_inpaint_vs_scipy_delaunay accepts any valid Delaunay triangle; this pins the choice.  Every case runs twice on ONE
workspace.

The shapes are the smallest at which the step can go wrong, not the workload's."""
import hashlib
import os

import numpy as np
import torch

import workspace_common as wc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'linear_parent.json')
DEV = 'cuda:0'
LOCALS = (1, 2, 0)            # two window passes (8x8 tiles / 20x20 windows, then 16x16 / 48x48) + global; the 48x48 pass only + global; global scans only
# carve_linear's regions in the order it takes them (csrc/linear.hip)
SITES, QLIST, COUNTS, UNRESOLVED, BLIST, ROWSTART, ROWQ, FBCOUNT, TODO = range(9)


def _bordered(m):
    m[0, :] = m[-1, :] = m[:, 0] = m[:, -1] = True
    return m


def _geometry_test_mask(name):
    """The synthetic masks of test_i0_linear_inpaint_vs_scipy_delaunay (tests/test_gpu_geometry.py), drawn as it draws them."""
    rng = np.random.default_rng(11)
    H, W = (37, 53) if name == "odd_37x53" else (91, 45) if name == "sparse_odd_91x45" else (64, 64)
    m = rng.uniform(0, 1, (H, W)) > (0.9 if name not in ("ring_only", "sparse_odd_91x45") else 2.0 if name == "ring_only" else 0.985)
    if name != "no_corners":
        _bordered(m)
    else:
        m[:6, :] = False; m[:, :5] = False                  # queries outside the hull, and on its right and bottom edges beyond the last site
    return m


def _far():
    """96 x 80, the full border and five interior sites: the circumcircles leave the 48 x 48 window, the global kernel finishes."""
    m = _bordered(np.zeros((80, 96), bool))
    for y, x in ((11, 17), (40, 50), (23, 77), (66, 30), (58, 81)):
        m[y, x] = True
    return m


def _one_row():
    m = np.zeros((33, 40), bool)
    m[13, [3, 4, 9, 17, 18, 30, 36]] = True
    return m


def _one_diagonal():
    m = np.zeros((33, 33), bool)
    for i in (2, 3, 8, 15, 16, 27, 31):
        m[i, i] = True
    return m


def _single():
    m = np.zeros((17, 19), bool)
    m[7, 5] = True
    return m


def _random(seed, H, W, density, border=True):
    m = np.random.default_rng(seed).uniform(0, 1, (H, W)) < density
    return _bordered(m) if border else m


# name -> (masks [B] of [H, W] bool, C, mask dtype)
CASES = {
    **{n: ([_geometry_test_mask(n)], 3, np.uint8) for n in ("random64", "ring_only", "no_corners", "odd_37x53", "sparse_odd_91x45")},
    "far_96x80": ([_far()], 3, np.uint8),
    "one_row": ([_one_row()], 3, np.uint8),
    "one_diagonal": ([_one_diagonal()], 3, np.uint8),
    "single_site": ([_single()], 3, np.uint8),
    "no_site": ([np.zeros((17, 19), bool)], 3, np.uint8),
    "two_masks_b2": ([_random(21, 40, 44, 0.12), _random(22, 40, 44, 0.02, border=False)], 3, np.uint8),
    "f32_mask": ([_random(23, 45, 37, 0.08)], 3, np.float32),
    "one_channel": ([_random(24, 50, 50, 0.05)], 1, np.uint8),
}
IDS = [(name, local) for name in CASES for local in LOCALS]


def operands(name):
    """(mask [B, H, W] of the case's dtype -- an f32 mask marks its sites with values other than 1 --, img [B, C, H, W] f32, zero off the sites)."""
    masks, Cn, dtype = CASES[name]
    m = np.stack(masks)
    rng = np.random.default_rng(1000 + list(CASES).index(name))
    img = rng.uniform(0, 1, (m.shape[0], Cn) + m.shape[1:]).astype(np.float32) * m[:, None]
    mask = m.astype(dtype) if dtype is np.uint8 else (m * rng.uniform(0.25, 2.0, m.shape)).astype(np.float32)
    return mask, img


def digest(a):
    """SHA-256 of an array's dtype, shape and bytes."""
    a = np.ascontiguousarray(a)
    h = hashlib.sha256(f"{a.dtype}{tuple(a.shape)}".encode())
    h.update(a.tobytes())
    return h.hexdigest()


def run_case(L, lib, name, local):
    """Two launches of a case on one workspace (zeroed once) -> [dict, dict]: the digests `out`, `tri`, `ints`; the integers themselves
    (`unresolved`, `bcount`, `fbcount` per image, `ns` = sites per image); and where the queries ended, counted from `tri` and the boundary
    list: `boundary_nan` / `boundary_segment` (finished by k_linear_boundary: -2, or tri[1] == tri[2]) and `tri_nan` (-2 from k_linear_tri)."""
    mask, img = operands(name)
    B, Cn, H, W = img.shape
    n = H * W
    md, im = torch.from_numpy(mask).to(DEV), torch.from_numpy(img).to(DEV)
    nbytes = L.pdhip_linear_fill_ws_bytes(B, H, W)
    ws = torch.zeros((nbytes,), dtype=torch.uint8, device=DEV)
    P = lib.ptr
    res = []
    for _ in range(2):
        out = torch.full((B, Cn, H, W), -7.0, device=DEV)
        tri = torch.full((B, H, W, 3), -9, dtype=torch.int32, device=DEV)
        old = L.pdhip_debug_set_linear_local(local)
        try:
            with wc.CarveLog(L) as log:
                rc = L.pdhip_linear_fill(P(im), P(out), B, Cn, H, W, P(md), int(mask.dtype == np.float32), n, P(ws), P(tri), lib.stream())
                carved, t = log.read()
        finally:
            L.pdhip_debug_set_linear_local(old)
        assert rc == 0, L.pdhip_last_error()
        torch.cuda.synchronize()
        assert carved == len(t) == 9 and (t[:, 0] == ws.data_ptr()).all() and int(t[-1, 1] + t[-1, 2]) <= nbytes, t.tolist()
        assert tuple(t[[COUNTS, UNRESOLVED, FBCOUNT], 2]) == (8 * B, 8, 8 * B) and t[BLIST, 2] == 12 * B * n
        w = ws.cpu().numpy()
        ints = lambda region, count: w[t[region, 1]:t[region, 1] + 4 * count].view(np.int32).copy()
        unresolved, bcount = (int(v) for v in ints(UNRESOLVED, 2))
        fbcount = [int(v) for v in ints(FBCOUNT, 2 * B)[1::2]]
        ns = [int(v) for v in ints(COUNTS, 2 * B)[0::2]]
        tr = tri.cpu().numpy().reshape(B * n, 3)
        assert 0 <= bcount <= B * n
        bl = ints(BLIST, 3 * bcount).reshape(-1, 3)[:, 0]
        assert len(np.unique(bl)) == bcount and ((bl >= 0) & (bl < B * n)).all()
        on_b = np.zeros(B * n, bool)
        on_b[bl] = True
        nan = (tr == -2).all(1)
        res.append(dict(out=digest(out.view(torch.int32).cpu().numpy()), tri=digest(tr),
                        ints=digest(np.array([unresolved, bcount] + fbcount, np.int32)),
                        unresolved=unresolved, bcount=bcount, fbcount=fbcount, ns=ns,
                        boundary_nan=int((nan & on_b).sum()), boundary_segment=int(((tr[:, 1] == tr[:, 2]) & (tr[:, 0] >= 0) & on_b).sum()),
                        tri_nan=int((nan & ~on_b).sum())))
    return res
