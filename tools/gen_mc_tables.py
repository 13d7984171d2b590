"""Generates pointdreamer_amd/csrc/mc_tables.h: the marching-cubes case table of csrc/surface_recon.hip.

The table is derived, not copied: for each of the 256 corner masks the iso-lines on the six cube faces are laid by ONE rule that
depends on the four corner signs of the face alone (an ambiguous face -- two inside corners on a diagonal -- is cut so that the
inside corners are separated), the directed segments are chained into closed loops on the cube's surface, and every loop is
triangulated without a diagonal whose two ends lie on one cube face.  Two cubes that share a face therefore lay the same segments
on it, in opposite directions, and no triangle edge other than those segments lies in a cube face: every directed edge of the mesh
occurs once, its reverse once -- a closed, consistently oriented surface for any scalar field.

Conventions: corner c = dx + 2 dy + 4 dz; bit c of the mask set = corner INSIDE (value above the iso value); edge e = 4 * axis +
u + 2 * v, where (u, v) are the edge's offsets along the other two axes in increasing axis order; triangles wind counter-clockwise
seen from outside the solid (normals point from inside to outside).

  python tools/gen_mc_tables.py            # rewrites the header
  python tools/gen_mc_tables.py --check    # exit status 1 if the committed header differs
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, 'pointdreamer_amd', 'csrc', 'mc_tables.h')


def corner(p):
    return p[0] + 2 * p[1] + 4 * p[2]


def edge_id(a, b):
    """Edge between two adjacent corners (as coordinate tuples)."""
    axis = [i for i in range(3) if a[i] != b[i]]
    assert len(axis) == 1
    ax = axis[0]
    o = [a[i] for i in range(3) if i != ax]
    return 4 * ax + o[0] + 2 * o[1]


def edge_faces(e):
    """The two cube faces (axis, side) an edge lies in."""
    ax, uv = e // 4, e % 4
    others = [i for i in range(3) if i != ax]
    return {(others[0], uv & 1), (others[1], uv >> 1)}


def face_cycles():
    """Corner cycles of the six faces, counter-clockwise seen from outside the cube."""
    out = []
    for ax in range(3):
        u, v = (ax + 1) % 3, (ax + 2) % 3                      # u x v = +axis
        for side in (0, 1):
            cyc = []
            for du, dv in ((0, 0), (1, 0), (1, 1), (0, 1)):
                p = [0, 0, 0]
                p[ax], p[u], p[v] = side, du, dv
                cyc.append(tuple(p))
            if side == 0:                                     # outward normal is -axis: reverse
                cyc.reverse()
            out.append(cyc)
    return out


def tri_ok(tris, loop):
    """No triangle edge that is not a loop segment may have both ends in one cube face."""
    seg = {(loop[i], loop[(i + 1) % len(loop)]) for i in range(len(loop))}
    for t in tris:
        for i in range(3):
            a, b = t[i], t[(i + 1) % 3]
            if (a, b) in seg:
                continue
            if edge_faces(a) & edge_faces(b):
                return False
    return True


def polygon_triangulations(poly):
    n = len(poly)
    if n == 3:
        return [[tuple(poly)]]
    res = []
    for k in range(2, n):                                     # triangle (0, 1, k) splits the polygon
        lefts = polygon_triangulations(poly[1:k + 1]) if k > 2 else [[]]
        rights = polygon_triangulations([poly[0]] + poly[k:]) if k < n - 1 else [[]]
        for l in lefts:
            for r in rights:
                res.append([(poly[0], poly[1], poly[k])] + l + r)
    return res


def build():
    faces = face_cycles()
    table = []
    for mask in range(256):
        inside = lambda p: (mask >> corner(p)) & 1
        nxt = {}
        for cyc in faces:
            s = [inside(p) for p in cyc]
            if all(s) or not any(s):
                continue
            for i in range(4):
                if s[i] and not s[(i + 1) % 4]:                # in -> out crossing: the segment's start
                    j = i
                    while s[(j - 1) % 4]:
                        j = (j - 1) % 4                        # j = first corner of the inside run that ends at i
                    P = edge_id(cyc[i], cyc[(i + 1) % 4])
                    Q = edge_id(cyc[(j - 1) % 4], cyc[j])       # out -> in crossing in front of the run
                    assert P not in nxt
                    nxt[P] = Q
        assert sorted(nxt) == sorted(nxt.values())
        tris, seen = [], set()
        for start in sorted(nxt):
            if start in seen:
                continue
            loop, e = [], start
            while e not in seen:
                seen.add(e)
                loop.append(e)
                e = nxt[e]
            assert e == start and len(loop) >= 3
            good = [t for t in polygon_triangulations(loop) if tri_ok(t, loop)]
            assert good, (mask, loop)
            tris += good[0]
        table.append(tris)
    # orientation: with corner 0 alone inside, the triangle's normal must point away from that corner
    mid = {}
    for ax in range(3):
        others = [i for i in range(3) if i != ax]
        for uv in range(4):
            p = [0.0, 0.0, 0.0]
            p[ax], p[others[0]], p[others[1]] = 0.5, uv & 1, uv >> 1
            mid[4 * ax + uv] = p
    (a, b, c), = table[1]
    A, B, Cc = mid[a], mid[b], mid[c]
    u = [B[i] - A[i] for i in range(3)]
    v = [Cc[i] - A[i] for i in range(3)]
    n = [u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0]]
    if sum(n[i] * A[i] for i in range(3)) < 0:
        table = [[(t[0], t[2], t[1]) for t in tris] for tris in table]
    return table


def render(table):
    maxt = max(len(t) for t in table)
    lines = ["// GENERATED by tools/gen_mc_tables.py -- do not edit.  Marching-cubes case table (see that file for the construction and the",
             "// conventions: corner c = dx + 2 dy + 4 dz, mask bit set = inside, edge e = 4 * axis + u + 2 * v, outward winding).",
             "#pragma once",
             "namespace pdhip {",
             f"constexpr int MC_MAX_TRI = {maxt};",
             "__constant__ signed char c_mc_ntri[256] = {"]
    for r in range(0, 256, 32):
        lines.append("    " + ", ".join(str(len(t)) for t in table[r:r + 32]) + ",")
    lines.append("};")
    lines.append(f"__constant__ signed char c_mc_tri[256][{3 * maxt}] = {{")
    for tris in table:
        flat = [e for t in tris for e in t]
        flat += [-1] * (3 * maxt - len(flat))
        lines.append("    {" + ", ".join(f"{e:2d}" for e in flat) + "},")
    lines.append("};")
    lines.append("}  // namespace pdhip")
    return "\n".join(lines) + "\n"


if __name__ == '__main__':
    text = render(build())
    if '--check' in sys.argv:
        sys.exit(0 if os.path.exists(OUT) and open(OUT).read() == text else 1)
    open(OUT, 'w').write(text)
    print(f"wrote {OUT}")
