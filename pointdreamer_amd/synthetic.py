"""Deterministic synthetic shapes for tests and bench.

The reference ships point clouds but neither a mesh nor a UV atlas for them, and POCO / xatlas
cannot run offline, so the benchmark geometry is a stand-in: a lat-long UV sphere (radius 0.5,
50 stacks x 100 slices = 9 800 triangles, 4 902 vertices), an analytic lat-long atlas
(`gb_pos`, `mask`, `per_atlas_pixel_face_id` in the wire format of
/root/reference/demo.py:445-448), and N colored points uniform on the sphere.
Plain numpy; no reference code involved.
"""
import math
import numpy as np

F32 = np.float32


def uv_sphere(stacks=50, slices=100, radius=0.5):
    """Returns vertices[Vn,3] f32, faces[F,3] int64, face (stack, slice, half) bookkeeping."""
    verts = [(0.0, radius, 0.0)]
    for s in range(1, stacks):
        lat = math.pi * s / stacks
        y = radius * math.cos(lat)
        rr = radius * math.sin(lat)
        for k in range(slices):
            lon = 2 * math.pi * k / slices
            verts.append((rr * math.cos(lon), y, rr * math.sin(lon)))
    verts.append((0.0, -radius, 0.0))
    south = len(verts) - 1

    def vid(s, k):
        return 1 + (s - 1) * slices + (k % slices)
    faces = []
    face_of_quad = {}
    for k in range(slices):                      # north fan (stack 0)
        face_of_quad[(0, k, 0)] = len(faces)
        face_of_quad[(0, k, 1)] = len(faces)
        faces.append((0, vid(1, k + 1), vid(1, k)))
    for s in range(1, stacks - 1):
        for k in range(slices):
            a, b, c, d = vid(s, k), vid(s, k + 1), vid(s + 1, k), vid(s + 1, k + 1)
            face_of_quad[(s, k, 0)] = len(faces)
            faces.append((a, b, c))
            face_of_quad[(s, k, 1)] = len(faces)
            faces.append((b, d, c))
    for k in range(slices):                      # south fan
        face_of_quad[(stacks - 1, k, 0)] = len(faces)
        face_of_quad[(stacks - 1, k, 1)] = len(faces)
        faces.append((south, vid(stacks - 1, k), vid(stacks - 1, k + 1)))
    lut = np.zeros((stacks, slices, 2), np.int64)
    for (s, k, h), f in face_of_quad.items():
        lut[s, k, h] = f
    return np.array(verts, F32), np.array(faces, np.int64), lut


def uv_sphere_uvs(stacks=50, slices=100, A=1024, gutter=2):
    """Explicit UVs of the lat-long sphere in the layout `latlong_atlas` rasterises (what xatlas would hand over as `uvs`,
    `mesh_tex_idx`): uvs[(stacks+1)*(slices+1), 2] f32 in [0,1] (u = column / A, v = row / A; seam column duplicated, one
    pole UV per fan triangle), face_uv_idx[F,3] int64 aligned with `uv_sphere`'s faces."""
    span = A - 2 * gutter
    uv = np.zeros(((stacks + 1) * (slices + 1), 2), np.float64)
    for s in range(stacks + 1):
        for k in range(slices + 1):
            kf = (k + 0.5) / slices if s in (0, stacks) else k / slices       # poles: one UV per fan triangle
            uv[s * (slices + 1) + k] = ((gutter + min(kf, 1.0) * span) / A, (gutter + s / stacks * span) / A)

    def uid(s, k):
        return s * (slices + 1) + k
    fuv = []
    for k in range(slices):
        fuv.append((uid(0, k), uid(1, k + 1), uid(1, k)))
    for s in range(1, stacks - 1):
        for k in range(slices):
            fuv.append((uid(s, k), uid(s, k + 1), uid(s + 1, k)))
            fuv.append((uid(s, k + 1), uid(s + 1, k + 1), uid(s + 1, k)))
    for k in range(slices):
        fuv.append((uid(stacks, k), uid(stacks - 1, k), uid(stacks - 1, k + 1)))
    return uv.astype(F32), np.array(fuv, np.int64)


def face_normals(vertices, faces):
    """Unit face normals (what kal.ops.mesh.face_normals(unit=True) provides at demo.py:422)."""
    v = vertices.astype(np.float64)
    n = np.cross(v[faces[:, 1]] - v[faces[:, 0]], v[faces[:, 2]] - v[faces[:, 0]])
    n /= np.maximum(np.linalg.norm(n, axis=1, keepdims=True), 1e-20)
    return n.astype(F32)


def latlong_atlas(A, stacks=50, slices=100, radius=0.5, gutter=2, n_charts=1, lut=None):
    """Analytic atlas: texel (row i, col j) -> (v, u) -> (lat, lon) on the sphere.
    n_charts > 1 splits the u range into strips separated by `gutter`-texel background gaps.
    Returns gb_pos[1,A,A,3] f32, mask[1,A,A,1] bool, per_atlas_pixel_face_id[1,A,A] int64 (-1 background)."""
    ii, jj = np.meshgrid(np.arange(A), np.arange(A), indexing='ij')
    mask = (ii >= gutter) & (ii < A - gutter) & (jj >= gutter) & (jj < A - gutter)
    if n_charts > 1:
        w = A // n_charts
        for c in range(1, n_charts):
            mask &= ~((jj >= c * w - gutter) & (jj < c * w + gutter))
    span = A - 2 * gutter
    v = (ii - gutter + 0.5) / span
    u = (jj - gutter + 0.5) / span
    lat = np.pi * np.clip(v, 0, 1)
    lon = 2 * np.pi * np.clip(u, 0, 1)
    pos = np.stack([radius * np.sin(lat) * np.cos(lon), radius * np.cos(lat), radius * np.sin(lat) * np.sin(lon)], -1)
    s = np.clip((np.clip(v, 0, 1) * stacks).astype(np.int64), 0, stacks - 1)
    k = np.clip((np.clip(u, 0, 1) * slices).astype(np.int64), 0, slices - 1)
    fs = np.clip(v, 0, 1) * stacks - s
    fk = np.clip(u, 0, 1) * slices - k
    half = ((fs + fk) > 1.0).astype(np.int64)
    if lut is None:
        _, _, lut = uv_sphere(stacks, slices, radius)
    fid = lut[s, k, half]
    fid = np.where(mask, fid, -1)
    gb_pos = np.where(mask[..., None], pos, 0.0).astype(F32)
    return gb_pos[None], mask[None, :, :, None], fid[None]


def sphere_points(n, radius=0.5, seed=0, noise=0.05):
    """n points uniform on the sphere + smooth-plus-noise colours in [0,1]."""
    rng = np.random.default_rng(seed)
    g = rng.standard_normal((n, 3))
    g /= np.linalg.norm(g, axis=1, keepdims=True)
    xyz = (radius * g).astype(F32)
    x, y = g[:, 0], g[:, 1]
    cols = []
    for c in range(3):
        ph = 2.0 * c
        cols.append(0.5 + 0.45 * np.sin(6 * np.pi * x * 0.5 + ph) * np.cos(4 * np.pi * y * 0.5 + 0.5 * ph))
    rgb = np.stack(cols, 1) + rng.uniform(-noise, noise, (n, 3))
    return xyz, np.clip(rgb, 0, 1).astype(F32)


def make_shape(n_points=30000, A=1024, stacks=50, slices=100, seed=0, n_charts=1, gutter=2):
    """One full synthetic shape in the reference's tensor contracts (numpy)."""
    vertices, faces, lut = uv_sphere(stacks, slices)
    gb_pos, mask, fid = latlong_atlas(A, stacks, slices, gutter=gutter, n_charts=n_charts, lut=lut)
    xyz, rgb = sphere_points(n_points, seed=seed)
    return dict(vertices=vertices, faces=faces, f_normals=face_normals(vertices, faces),
                gb_pos=gb_pos, mask=mask, per_atlas_pixel_face_id=fid, points=xyz, colors=rgb)


def icosphere(n, radius=0.5, noise=0.0, seed=0):
    """Icosahedron with every face cut into n^2 triangles (20 n^2 faces, shared vertices welded), projected onto the sphere, each
    vertex then moved radially by a factor 1 + noise * N(0, 1): a stand-in for a marching-cubes surface of a given face count."""
    t = (1 + 5 ** 0.5) / 2
    V = np.array([[-1, t, 0], [1, t, 0], [-1, -t, 0], [1, -t, 0], [0, -1, t], [0, 1, t], [0, -1, -t], [0, 1, -t],
                  [t, 0, -1], [t, 0, 1], [-t, 0, -1], [-t, 0, 1]], np.float64)
    F = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    ii, jj = np.meshgrid(np.arange(n + 1), np.arange(n + 1), indexing='ij')
    keep = ii + jj <= n
    ii, jj = ii[keep], jj[keep]
    lid = -np.ones((n + 2, n + 2), np.int64)
    lid[ii, jj] = np.arange(len(ii))
    i, j = np.meshgrid(np.arange(n), np.arange(n), indexing='ij')
    up = i + j < n
    down = i + j + 2 <= n
    tri = np.concatenate([np.stack([lid[i, j], lid[i + 1, j], lid[i, j + 1]], -1)[up],
                          np.stack([lid[i + 1, j], lid[i + 1, j + 1], lid[i, j + 1]], -1)[down]])
    vs = [V[a] + (V[b] - V[a]) * (ii[:, None] / n) + (V[c] - V[a]) * (jj[:, None] / n) for a, b, c in F]
    fs = [tri + k * len(ii) for k in range(len(F))]
    v, f = np.concatenate(vs), np.concatenate(fs)
    v = v / np.linalg.norm(v, axis=1, keepdims=True)
    _, first, inv = np.unique(np.round(v, 9), axis=0, return_index=True, return_inverse=True)
    v, f = v[first], inv.reshape(-1)[f]
    rng = np.random.default_rng(seed)
    v = v * radius * (1.0 + noise * rng.standard_normal((len(v), 1)))
    return v.astype(F32), f.astype(np.int64)


# ---- analytic test solids for the surface reconstruction (spr.py): signed distance (negative inside), outward unit normal, a smooth
# colour field, an area-uniform seeded point sampler.  All fit the box [-0.5, 0.5]^3.
def solid_color(x):
    """Smooth colour field in [0.05, 0.95]^3 at positions x [n,3]."""
    x = np.asarray(x, np.float64)
    cols = []
    for c in range(3):
        ph = 2.0 * c
        cols.append(0.5 + 0.45 * np.sin(3 * np.pi * x[:, 0] + ph) * np.cos(2 * np.pi * x[:, 1] + 0.5 * ph) * np.cos(2 * np.pi * x[:, 2] - ph))
    return np.stack(cols, 1)


def _seg_dist(p, a, b):
    pa, ba = p - a, b - a
    h = np.clip((pa @ ba) / (ba @ ba), 0.0, 1.0)
    return np.linalg.norm(pa - h[:, None] * ba, axis=1)


class Solid:
    """name, sdf(x) (exact distances, except 'ellipsoid': distance to the foot point of a Newton projection, exact to O(d^2 * curvature)),
    components, euler (per component), volume (closed form where there is one, else None: see volume())."""
    NAMES = ('sphere', 'ellipsoid', 'torus', 'rounded_box', 'two_spheres', 'cup')

    def __init__(self, name):
        if name not in self.NAMES:
            raise ValueError(f"unknown solid {name!r}: one of {self.NAMES}")
        self.name = name
        self.components, self.euler = (2, 2) if name == 'two_spheres' else (1, 0 if name == 'torus' else 2)
        self.ell = np.array([0.5, 0.35, 0.25])
        self.volume_exact = {'sphere': 4 / 3 * np.pi * 0.5 ** 3, 'ellipsoid': 4 / 3 * np.pi * float(np.prod(self.ell)),
                             'torus': 2 * np.pi ** 2 * 0.35 * 0.15 ** 2, 'two_spheres': 2 * 4 / 3 * np.pi * 0.2 ** 3}.get(name)

    def sdf(self, x):
        x = np.asarray(x, np.float64)
        n = self.name
        if n == 'sphere':
            return np.linalg.norm(x, axis=1) - 0.5
        if n == 'torus':                                       # major 0.35, minor 0.15, axis y
            q = np.stack([np.hypot(x[:, 0], x[:, 2]) - 0.35, x[:, 1]], 1)
            return np.linalg.norm(q, axis=1) - 0.15
        if n == 'rounded_box':                                 # half extents (0.5, 0.35, 0.3), corner radius 0.1
            q = np.abs(x) - (np.array([0.5, 0.35, 0.3]) - 0.1)
            return np.linalg.norm(np.maximum(q, 0.0), axis=1) + np.minimum(q.max(1), 0.0) - 0.1
        if n == 'two_spheres':                                 # radius 0.2, centres (+-0.3, 0, 0): 0.2 apart
            c = np.array([0.3, 0.0, 0.0])
            return np.minimum(np.linalg.norm(x - c, axis=1), np.linalg.norm(x + c, axis=1)) - 0.2
        if n == 'cup':                                         # a U profile of wall radius 0.07 revolved about y: open at the top
            p = np.stack([np.hypot(x[:, 0], x[:, 2]), x[:, 1]], 1)
            a, b, c = np.array([0.0, -0.4]), np.array([0.4, -0.4]), np.array([0.4, 0.43])
            return np.minimum(_seg_dist(p, a, b), _seg_dist(p, b, c)) - 0.07
        # ellipsoid: foot point by Newton steps on the Lagrange multiplier of the closest-point problem
        e2 = self.ell ** 2
        t = np.zeros(len(x))
        for _ in range(30):
            d = e2[None] / (t[:, None] + e2[None])
            g = ((d * x) ** 2 / e2[None]).sum(1) - 1.0
            dg = (-2.0 * (d * x) ** 2 / e2[None] / (t[:, None] + e2[None])).sum(1)
            t = np.maximum(t - g / np.where(dg == 0, -1.0, dg), -e2.min() * 0.999)
        foot = e2[None] / (t[:, None] + e2[None]) * x
        inside = ((x / self.ell) ** 2).sum(1) < 1.0
        return np.linalg.norm(x - foot, axis=1) * np.where(inside, -1.0, 1.0)

    def normal(self, x, eps=1e-5):
        """Outward unit normal = the normalised gradient of sdf (central differences)."""
        x = np.asarray(x, np.float64)
        g = np.stack([self.sdf(x + eps * np.eye(3)[a]) - self.sdf(x - eps * np.eye(3)[a]) for a in range(3)], 1)
        return g / np.maximum(np.linalg.norm(g, axis=1, keepdims=True), 1e-300)

    def color(self, x):
        return solid_color(x)

    def volume(self, n=160):
        """Closed form, or the midpoint rule on an n^3 grid over [-0.55, 0.55]^3 with a linear ramp across the surface."""
        if self.volume_exact is not None:
            return self.volume_exact
        h = 1.1 / n
        c = (np.arange(n) + 0.5) * h - 0.55
        tot = 0.0
        for z in c:
            X, Y = np.meshgrid(c, c, indexing='ij')
            d = self.sdf(np.stack([X.ravel(), Y.ravel(), np.full(X.size, z)], 1))
            tot += np.clip(0.5 - d / h, 0.0, 1.0).sum()
        return tot * h ** 3

    def sample(self, n, seed=0, noise=0.0, shell=0.01):
        """n points area-uniform on the surface (uniform draws in a thin shell round it, projected along the normal), optional Gaussian
        noise of standard deviation `noise` along the normal -> (xyz f32 [n,3], rgb f32 [n,3], outward normals f32 [n,3])."""
        rng = np.random.default_rng(seed)
        got = []
        have = 0
        while have < n:
            x = rng.uniform(-0.6, 0.6, (400000, 3))
            x = x[np.abs(self.sdf(x)) < shell]
            for _ in range(3):
                x = x - self.sdf(x)[:, None] * self.normal(x)
            got.append(x)
            have += len(x)
        x = np.concatenate(got)[:n]
        nrm = self.normal(x)
        rgb = self.color(x)
        if noise > 0:
            x = x + noise * rng.standard_normal((n, 1)) * nrm
        return x.astype(F32), np.clip(rgb, 0, 1).astype(F32), nrm.astype(F32)


def solid(name):
    return Solid(name)
