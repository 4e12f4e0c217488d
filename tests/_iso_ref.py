"""numpy restatement of K34 as include/fpsg_hip.h defines it: the implicit field of an oriented cloud in float32,
operation for operation (vectorised over the nodes, looped over the points in ascending order, dense: no point is ever
culled), the same field in float64 with an error bound for the float32 one, the marching-tetrahedra table generated from
the header's rule, and the extraction.  Plus the analytic fields and the mesh checks the tests share."""
import itertools

import numpy as np

F32 = np.float32
U = 2.0 ** -24                                     # unit roundoff of float32
TILE = 256                                         # FPSG_FIELD_TILE: points per LDS tile of the kernel
BRICK = 8                                          # FPSG_FIELD_BRICK: nodes per brick side
CLASSES = ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 0, 1), (0, 1, 1), (1, 1, 1))
PERMS = tuple(itertools.permutations(range(3)))    # lexicographic: 012 021 102 120 201 210


# ----------------------------------------------------------------------------------------------- the field
def node_axes(origin, cell, G, dtype=F32):
    """The node coordinates per axis [3,G]: origin + (float)i * cell, the multiply rounded before the add."""
    i = np.arange(G).astype(dtype)
    o, h = np.asarray(origin, dtype), dtype(cell)
    return np.stack([o[a] + i * h for a in range(3)])


def _finite_rows(points, normals):
    return np.isfinite(points).all(axis=1) & np.isfinite(normals).all(axis=1)


def field32(points, normals, origin, cell, radius, G):
    """One cloud: (field float32 [G,G,G], weight float32 [G,G,G]), the kernel's bits."""
    P, Q = np.asarray(points, F32), np.asarray(normals, F32)
    ax = node_axes(origin, cell, G)
    X, Y, Z = (a.reshape(-1) for a in np.meshgrid(ax[0], ax[1], ax[2], indexing="ij"))
    r = F32(radius)
    with np.errstate(all="ignore"):
        inv = F32(1) / (r * r)
        num, den = np.zeros(G ** 3, F32), np.zeros(G ** 3, F32)
        ok = _finite_rows(P, Q)
        for j in range(len(P)):
            if not ok[j]:
                continue
            dx, dy, dz = X - P[j, 0], Y - P[j, 1], Z - P[j, 2]
            d2 = (dx * dx + dy * dy) + dz * dz
            t = np.fmax(F32(1) - d2 * inv, F32(0))
            w = (t * t) * t
            s = (dx * Q[j, 0] + dy * Q[j, 1]) + dz * Q[j, 2]
            num = num + w * s
            den = den + w
        field = np.where(den > 0, num / np.where(den > 0, den, F32(1)), F32(np.nan)).astype(F32)
    assert num.dtype == F32 and den.dtype == F32 and field.dtype == F32
    return field.reshape(G, G, G), den.reshape(G, G, G)


def field64(points, normals, origin, cell, radius, G):
    """One cloud in float64 on the float32 inputs: (field, bound, scale, comparable), each [G,G,G].

    ``scale`` = sum(w |s|) / sum(w), what the bound is stated against (|field| itself cancels).  ``bound`` is a bound of
    |field32 - field64| from the operation count of the definition, u = 2^-24, every term taken from the float64 values
    (nothing is fitted to the float32 output):

    - dx is one rounding; d2 = (dx dx + dy dy) + dz dz is a sum of non-negative terms, five roundings deep: relative
      5 u; inv = 1 / (r r) two more; q = d2 inv one more: relative 8 u, and q <= 1 + 8 u wherever a point can
      contribute, so t = 1 - q is off by at most 8 u (1 + 8 u) + u < dt = 10 u ABSOLUTE: the error of w = (t t) t is
      not relative to w near the edge of the support.  Per point dw = (1 + 2 u) max(t_raw + dt, 0)^3 - w covers a point
      that only float32 sees inside its ball.
    - s = (dx nx + dy ny) + dz nz: four roundings deep, against sabs = |dx nx| + |dy ny| + |dz nz| (s cancels):
      ds = 4 u sabs; the product w s one more.
    - the sums of n contributing terms: (n - 1) u of the sum of magnitudes.
    - num / den: (dnum + |field| dden) / (den - dden), and u |field| for the division.
    A factor 1 + 2^-10 covers the products of these first-order terms.  ``comparable`` is False where den <= 2 dden:
    there float32 may find no weight at all and the quotient has no bound."""
    P, Q = np.asarray(points, F32).astype(np.float64), np.asarray(normals, F32).astype(np.float64)
    ax = node_axes(origin, cell, G).astype(np.float64)       # the float32 node positions are part of the definition
    X, Y, Z = (a.reshape(-1) for a in np.meshgrid(ax[0], ax[1], ax[2], indexing="ij"))
    r = np.float64(F32(radius))
    inv = 1.0 / (r * r)
    n3 = G ** 3
    num, den, mag, dnum, dden, cnt = (np.zeros(n3) for _ in range(6))
    dt = 10 * U
    ok = _finite_rows(P, Q)
    for j in range(len(P)):
        if not ok[j]:
            continue
        dx, dy, dz = X - P[j, 0], Y - P[j, 1], Z - P[j, 2]
        t_raw = 1.0 - ((dx * dx + dy * dy) + dz * dz) * inv
        t = np.maximum(t_raw, 0.0)
        w = t * t * t
        s = dx * Q[j, 0] + dy * Q[j, 1] + dz * Q[j, 2]
        sabs = np.abs(dx * Q[j, 0]) + np.abs(dy * Q[j, 1]) + np.abs(dz * Q[j, 2])
        w_hi = (1 + 2 * U) * np.maximum(t_raw + dt, 0.0) ** 3
        dw = w_hi - w
        num += w * s
        den += w
        mag += w * np.abs(s)
        dnum += dw * np.abs(s) + w_hi * (4 * U * sabs) + U * w_hi * (np.abs(s) + 4 * U * sabs)
        dden += dw
        cnt += w_hi > 0
    dnum += cnt * U * (mag + dnum)
    dden += cnt * U * (den + dden)
    comparable = den > 2 * dden
    safe = np.where(comparable, den, 1.0)
    field = np.where(den > 0, num / np.where(den > 0, den, 1.0), np.nan)
    bound = ((dnum + np.abs(field) * dden) / (safe - dden) + U * np.abs(field)) * (1 + 2.0 ** -10)
    scale = mag / safe
    return tuple(a.reshape(G, G, G) for a in (field, np.where(comparable, bound, np.inf), scale, comparable))


# ----------------------------------------------------------------------------------------------- the table
def tet_corners(t):
    """The four path corners of tetrahedron t as (di, dj, dk)."""
    a, b, _ = PERMS[t]
    c0 = np.zeros(3, int)
    c1 = c0.copy(); c1[a] = 1
    c2 = c1.copy(); c2[b] = 1
    return [tuple(c0), tuple(c1), tuple(c2), (1, 1, 1)]


def case_triangles(t, m):
    """The triangles of case m (bit p: path corner p inside) of tetrahedron t: a list of triangles, each three edges
    (p, q) of path corners with p < q, wound by the header's rule."""
    inside = [p for p in range(4) if m >> p & 1]
    outside = [p for p in range(4) if not m >> p & 1]
    if len(inside) == 1:
        tris = [[(inside[0], o) for o in outside]]
    elif len(inside) == 3:
        tris = [[(i, outside[0]) for i in inside]]
    elif len(inside) == 2:
        (i, j), (k, l) = inside, outside
        tris = [[(i, k), (i, l), (j, l)], [(i, k), (j, l), (j, k)]]
    else:
        return []
    pos = np.asarray(tet_corners(t), np.float64)
    want = pos[outside].mean(axis=0) - pos[inside].mean(axis=0)
    mid = [0.5 * (pos[p] + pos[q]) for p, q in tris[0]]
    if np.dot(np.cross(mid[1] - mid[0], mid[2] - mid[0]), want) < 0:
        tris = [[tr[0], tr[2], tr[1]] for tr in tris]
    return [[(min(p, q), max(p, q)) for p, q in tr] for tr in tris]


def edge_class(step):
    return CLASSES.index(tuple(int(v) for v in step))


# ----------------------------------------------------------------------------------------------- the extraction
def _finite_inside(field):
    fin = np.isfinite(field)
    with np.errstate(invalid="ignore"):
        return fin, fin & (field < 0)


def edge_flags(field):
    """[G,G,G,7] bool: the active owned edges of every node."""
    G = field.shape[0]
    fin, ins = _finite_inside(field)
    act = np.zeros((G, G, G, 7), bool)
    for c, (di, dj, dk) in enumerate(CLASSES):
        lo = (slice(0, G - di), slice(0, G - dj), slice(0, G - dk))
        hi = (slice(di, G), slice(dj, G), slice(dk, G))
        act[lo + (c,)] = fin[lo] & fin[hi] & (ins[lo] != ins[hi])
    return act


def extract(field, origin, cell, dtype=F32):
    """One cloud -> dict(verts [V,3] dtype, faces [F,3] int32, node_edges [G^3] int32, cell_tris [G^3] int32)."""
    field = np.asarray(field, dtype)
    G = field.shape[0]
    act = edge_flags(field)
    node_edges = act.sum(axis=3).astype(np.int32).reshape(-1)
    offset = np.concatenate([[0], np.cumsum(node_edges, dtype=np.int64)[:-1]]).reshape(G, G, G)
    rank = np.cumsum(act, axis=3) - act                      # active classes below c
    vid = np.where(act, offset[..., None] + rank, -1)
    # vertices: node order, then class order
    I, J, K, C = np.nonzero(act)
    ax = node_axes(origin, cell, G, dtype)
    step = np.asarray(CLASSES)[C]
    f0 = field[I, J, K]
    f1 = field[I + step[:, 0], J + step[:, 1], K + step[:, 2]]
    with np.errstate(all="ignore"):
        t = f0 / (f0 - f1)
        moved = [ax[0][I] + t * dtype(cell), ax[1][J] + t * dtype(cell), ax[2][K] + t * dtype(cell)]
    verts = np.stack([np.where(step[:, a] == 1, moved[a], ax[a][(I, J, K)[a]]) for a in range(3)], axis=1).astype(dtype)
    # triangles: cell, tetrahedron, table order
    fin, ins = _finite_inside(field)
    n = G - 1
    cell_id = (np.arange(n)[:, None, None] * G + np.arange(n)[None, :, None]) * G + np.arange(n)[None, None, :]
    keys, tris = [], []
    cell_tris = np.zeros((G, G, G), np.int32)

    def corner(a, d):
        return a[d[0]:d[0] + n, d[1]:d[1] + n, d[2]:d[2] + n]

    for t_id in range(6):
        corners = tet_corners(t_id)
        ok = np.ones((n, n, n), bool)
        case = np.zeros((n, n, n), int)
        for p, d in enumerate(corners):
            ok &= corner(fin, d)
            case |= corner(ins, d).astype(int) << p
        for m in range(1, 15):
            sel = ok & (case == m)
            if not sel.any():
                continue
            for q, tri in enumerate(case_triangles(t_id, m)):
                ids = []
                for p0, p1 in tri:
                    d0, d1 = np.asarray(corners[p0]), np.asarray(corners[p1])
                    ids.append(corner(vid[..., edge_class(d1 - d0)], d0)[sel])
                tris.append(np.stack(ids, axis=1))
                keys.append((cell_id[sel] * 6 + t_id) * 2 + q)
                cell_tris[:n, :n, :n][sel] += 1
    if tris:
        tris, keys = np.concatenate(tris), np.concatenate(keys)
        faces = tris[np.argsort(keys, kind="stable")].astype(np.int32)
        assert faces.min() >= 0
    else:
        faces = np.zeros((0, 3), np.int32)
    return {"verts": verts, "faces": faces, "node_edges": node_edges, "cell_tris": cell_tris.reshape(-1)}


def canonical_faces(faces):
    """Every triangle rotated to its smallest index first, the rows sorted: what two meshes are compared by."""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    if not len(f):
        return f
    shift = np.argmin(f, axis=1)
    rolled = np.stack([f[np.arange(len(f)), (shift + k) % 3] for k in range(3)], axis=1)
    return rolled[np.lexsort((rolled[:, 2], rolled[:, 1], rolled[:, 0]))]


# ----------------------------------------------------------------------------------------------- mesh checks
def topology(faces, n_verts):
    """-> dict(boundary, nonmanifold, inconsistent, euler): counted on directed edges, independent of fpsg_amd."""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    a = np.concatenate([f[:, 0], f[:, 1], f[:, 2]])
    b = np.concatenate([f[:, 1], f[:, 2], f[:, 0]])
    und = {}
    for x, y in zip(a.tolist(), b.tolist()):
        e = und.setdefault((min(x, y), max(x, y)), [0, 0])
        e[0 if x < y else 1] += 1
    boundary = sum(1 for p, q in und.values() if p + q == 1)
    nonmanifold = sum(1 for p, q in und.values() if p + q > 2)
    inconsistent = sum(1 for p, q in und.values() if p + q == 2 and p != q)
    return {"boundary": boundary, "nonmanifold": nonmanifold, "inconsistent": inconsistent,
            "euler": int(n_verts) - len(und) + len(f)}


def volume(verts, faces):
    v, f = np.asarray(verts, np.float64), np.asarray(faces, np.int64)
    return float((v[f[:, 0]] * np.cross(v[f[:, 1]], v[f[:, 2]])).sum() / 6.0)


# ----------------------------------------------------------------------------------------------- analytic fields
def unit_grid(G):
    """origin, cell of G nodes per side on [-1, 1]^3."""
    return np.full(3, -1.0, F32), F32(2.0 / (G - 1))


def grid_points(G, dtype=np.float64):
    origin, cell = unit_grid(G)
    ax = node_axes(origin.astype(dtype), dtype(cell), G, dtype)
    return np.meshgrid(ax[0], ax[1], ax[2], indexing="ij")


def sphere_field(G, radius=0.7, centre=(0.0, 0.0, 0.0)):
    X, Y, Z = grid_points(G)
    return np.sqrt((X - centre[0]) ** 2 + (Y - centre[1]) ** 2 + (Z - centre[2]) ** 2) - radius


def torus_field(G, R=0.6, r=0.25):
    X, Y, Z = grid_points(G)
    return np.sqrt((np.sqrt(X * X + Y * Y) - R) ** 2 + Z * Z) - r


def two_spheres_field(G):
    return np.minimum(sphere_field(G, 0.3, (-0.5, -0.4, -0.45)), sphere_field(G, 0.33, (0.45, 0.5, 0.4)))


def zeros_field(G):
    """A sphere whose node values within 0.08 of the surface are exactly 0 or -0: zeros at nodes, on both sides."""
    f = sphere_field(G).astype(F32)
    near = np.abs(f) < 0.08
    return np.where(near, np.where(f < 0, F32(-0.0), F32(0.0)), f).astype(F32)


def nan_slab_field(G):
    f = sphere_field(G).astype(F32)
    f[:, G // 2, :] = np.nan
    return f


def sphere_cloud(n, radius=0.8, seed=1):
    """n points of default_rng(seed) on a sphere with exact normals: (points, normals) float32."""
    d = np.random.default_rng(seed).standard_normal((n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return (radius * d).astype(F32), d.astype(F32)
