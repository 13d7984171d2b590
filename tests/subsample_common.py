"""Helpers of the subsampling tests (tests/test_subsample_cpu.py, tests/test_gpu_subsample.py, tools/bench_subsample.py): the brute-force float64
oracle of pdhip_fps -- the definition of include/pdhip.h with one vectorised update per pick --, the int64 oracle of pdhip_owner_mean_colors, and the
clouds the tests share (computed once, read-only).  Nothing here calls libpdhip."""
import functools

import numpy as np


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays if len(arrays) > 1 else arrays[0]


def _d2(p, q):
    """d2 of every row of p [N,3] f64 to the point q [3]: (dx dx + dy dy) + dz dz, op by op."""
    dx, dy, dz = p[:, 0] - q[0], p[:, 1] - q[1], p[:, 2] - q[2]
    return (dx * dx + dy * dy) + dz * dz


def oracle_fps(points, M, start=0, return_ties=False):
    """(idx [M] i32, min_d2 [M] f64[, ties]): float32 inputs widened to float64; idx[0] = start, min_d2[0] = +inf; every further pick the unselected
    point with the largest mind, the FIRST (= smallest) index on a tie (np.argmax).  A selected point carries -1 and every mind is >= 0, so it is
    never selected again.  ties: picks at which more than one unselected point attained the maximum.  Performs exactly N * M point updates."""
    p = np.asarray(points, np.float32).astype(np.float64).reshape(-1, 3)
    N = len(p)
    assert 1 <= M <= N and 0 <= start < N
    idx, min_d2 = np.empty(M, np.int32), np.empty(M, np.float64)
    idx[0], min_d2[0] = start, np.inf
    mind = _d2(p, p[start])
    mind[start] = -1.0
    ties = 0
    for k in range(1, M):
        j = int(np.argmax(mind))
        idx[k], min_d2[k] = j, mind[j]
        if return_ties:
            ties += int((mind == mind[j]).sum() > 1)
        np.minimum(mind, _d2(p, p[j]), out=mind, where=mind >= 0.0)
        mind[j] = -1.0
    return (idx, min_d2, ties) if return_ties else (idx, min_d2)


def loops_fps(points, M, start=0):
    """The same definition as a plain-Python triple loop (pick, point, nothing vectorised): what oracle_fps is checked against on a dozen points."""
    p = [[float(np.float64(np.float32(c))) for c in row] for row in np.asarray(points, np.float32)]
    N = len(p)
    picks, vals = [start], [float('inf')]
    for _ in range(1, M):
        best, best_v = -1, -1.0
        for i in range(N):
            if i in picks:
                continue
            m = float('inf')
            for s in picks:
                dx, dy, dz = p[i][0] - p[s][0], p[i][1] - p[s][1], p[i][2] - p[s][2]
                m = min(m, (dx * dx + dy * dy) + dz * dz)
            if m > best_v:                                         # (strict: the smallest index keeps a tie)
                best, best_v = i, m
        picks.append(best)
        vals.append(best_v)
    return np.array(picks, np.int32), np.array(vals, np.float64)


def oracle_nearest_sample(points, samples, chunk=256):
    """owner [N] i32: per point the FIRST (= smallest) position among the samples with the least d2 (pdhip_nearest_points' definition)."""
    p = np.asarray(points, np.float32).astype(np.float64).reshape(-1, 3)
    s = np.asarray(samples, np.float32).astype(np.float64).reshape(-1, 3)
    owner = np.empty(len(p), np.int32)
    for b in range(0, len(p), chunk):
        q = p[b:b + chunk, None, :]
        dx, dy, dz = q[..., 0] - s[None, :, 0], q[..., 1] - s[None, :, 1], q[..., 2] - s[None, :, 2]
        owner[b:b + chunk] = np.argmin((dx * dx + dy * dy) + dz * dz, axis=1)
    return owner


def oracle_mean_colors(owner, colors, M, fallback):
    """[M,3] f32: per sample and channel the int64 sum of rint(c 2^32) and the count; (sum / count) / 2^32 in float64, rounded to float32; a sample
    that owns nothing takes fallback."""
    c = np.asarray(colors, np.float32).astype(np.float64).reshape(-1, 3)
    q = np.rint(c * 4294967296.0).astype(np.int64)
    sums, cnt = np.zeros((M, 3), np.int64), np.zeros(M, np.int64)
    np.add.at(sums, np.asarray(owner, np.int64), q)
    np.add.at(cnt, np.asarray(owner, np.int64), 1)
    with np.errstate(invalid='ignore', divide='ignore'):
        mean = ((sums.astype(np.float64) / cnt.astype(np.float64)[:, None]) / 4294967296.0).astype(np.float32)
    return np.where((cnt == 0)[:, None], np.asarray(fallback, np.float32), mean)


# ---- the clouds
def sphere_points(n, seed, radius=0.5, noise=0.0):
    rng = np.random.default_rng(seed)
    v = rng.standard_normal((n, 3))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    v = v * radius + noise * rng.standard_normal((n, 3))
    return v.astype(np.float32)


def box_points(n, seed):
    return np.random.default_rng(seed).random((n, 3), dtype=np.float32) - np.float32(0.5)


@functools.lru_cache(maxsize=None)
def case(name):
    """(points [N,3] f32, M, start) of a named case of tests/test_gpu_subsample.py."""
    rng = np.random.default_rng(sum(map(ord, name)))           # (a seed of the case's own)
    if name == 'one':
        return _frozen(np.array([[0.25, -1.0, 3.0]], np.float32)), 1, 0
    if name == 'five':
        return _frozen(rng.random((5, 3), dtype=np.float32)), 5, 2
    if name == 'identical':                                        # the never-reselect rule: the picks are 0, 1, 2, ...
        return _frozen(np.tile(np.array([[0.5, 0.25, -0.125]], np.float32), (100, 1))), 10, 0
    if name == 'lattice':                                          # every step is a tie
        g = np.stack(np.meshgrid(*(np.arange(8),) * 3, indexing='ij'), -1).reshape(-1, 3).astype(np.float32)
        return _frozen(g[rng.permutation(len(g))]), 100, 7
    if name == 'plane':                                            # a box without extent on one axis
        p = rng.random((3000, 3), dtype=np.float32)
        p[:, 2] = np.float32(0.375)
        return _frozen(p), 300, 11
    if name == 'line':                                             # ... and on two
        t = rng.random(3000, dtype=np.float32)
        p = np.stack([t, np.full_like(t, -2.0), np.full_like(t, 0.75)], 1)
        return _frozen(p), 300, 5
    if name == 'clustered':                                        # a noisy sphere, a blob 1e-3 wide, one outlier at distance 50; start in the blob
        sph = sphere_points(20000, 3, 0.5, 0.01)
        blob = (np.array([[0.1, 0.2, 0.3]]) + 1.0e-3 * (rng.random((2000, 3)) - 0.5)).astype(np.float32)
        far = np.array([[50.0, 0.0, 0.0]], np.float32)
        return _frozen(np.concatenate([sph, blob, far])), 2000, 20000 + 17
    if name == 'large':                                            # the pruning case: 100 000 -> 2 000
        return _frozen(sphere_points(100000, 5, 0.5, 0.002)), 2000, 123
    if name == 'random':                                           # no pick of the oracle is a tie (asserted where it is used)
        return _frozen(box_points(4000, 9)), 400, 3
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def oracle_case(name):
    p, M, start = case(name)
    return _frozen(*oracle_fps(p, M, start))


@functools.lru_cache(maxsize=None)
def color_case():
    """(points [5000,3], colors [5000,3] f32 in [0, 1], idx [200] i32 = the oracle's picks)."""
    p = box_points(5000, 21)
    c = np.random.default_rng(22).random((5000, 3), dtype=np.float32)
    c[:7] = np.float32(0.0)
    c[7:13] = np.float32(1.0)
    idx, _ = oracle_fps(p, 200, 0)
    return _frozen(p, c, idx)
