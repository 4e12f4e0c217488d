"""numpy restatement of K26 (surface sampling) and K27 (orthographic views) as include/fpsg_hip.h defines them: float32
and int64 with the header's operation order for everything that is compared bit for bit, and a float64 form of the
geometry and of the shading for the checks that are not.  Plus the procedural meshes the tests use."""
import numpy as np

F32 = np.float32
SNAP_LIMIT = F32(2.0 ** 28)
EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)


# ------------------------------------------------------------------------------------------ meshes
def cube(lo=-0.5, hi=0.5):
    v = np.array([[x, y, z] for x in (lo, hi) for y in (lo, hi) for z in (lo, hi)], dtype=F32)
    f = np.array([[0, 1, 3], [0, 3, 2], [4, 6, 7], [4, 7, 5], [0, 4, 5], [0, 5, 1],
                  [2, 3, 7], [2, 7, 6], [0, 2, 6], [0, 6, 4], [1, 5, 7], [1, 7, 3]], dtype=np.int32)
    return v, f


def tetrahedron():
    v = np.array([[0.5, 0.5, 0.5], [-0.5, -0.5, 0.5], [-0.5, 0.5, -0.5], [0.5, -0.5, -0.5]], dtype=F32)
    return v, np.array([[0, 1, 2], [0, 3, 1], [0, 2, 3], [1, 3, 2]], dtype=np.int32)


def icosphere(level=0, radius=0.5):
    t = (1.0 + 5.0 ** 0.5) / 2.0
    v = [[-1, t, 0], [1, t, 0], [-1, -t, 0], [1, -t, 0], [0, -1, t], [0, 1, t], [0, -1, -t], [0, 1, -t],
         [t, 0, -1], [t, 0, 1], [-t, 0, -1], [-t, 0, 1]]
    f = [[0, 11, 5], [0, 5, 1], [0, 1, 7], [0, 7, 10], [0, 10, 11], [1, 5, 9], [5, 11, 4], [11, 10, 2], [10, 7, 6],
         [7, 1, 8], [3, 9, 4], [3, 4, 2], [3, 2, 6], [3, 6, 8], [3, 8, 9], [4, 9, 5], [2, 4, 11], [6, 2, 10],
         [8, 6, 7], [9, 8, 1]]
    v = [np.asarray(p, dtype=np.float64) / np.linalg.norm(p) for p in v]
    for _ in range(level):
        mid, nf = {}, []

        def m(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                p = v[a] + v[b]
                v.append(p / np.linalg.norm(p))
                mid[key] = len(v) - 1
            return mid[key]

        for a, b, c in f:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            nf += [[a, ab, ca], [b, bc, ab], [c, ca, bc], [ab, bc, ca]]
        f = nf
    return (np.asarray(v) * radius).astype(F32), np.asarray(f, dtype=np.int32)


def grid(nx, ny, lo=-0.5, hi=0.5, z=0.0):
    """nx x ny cells in the plane z: 2 nx ny triangles."""
    xs, ys = np.linspace(lo, hi, nx + 1), np.linspace(lo, hi, ny + 1)
    v = np.array([[x, y, z] for y in ys for x in xs], dtype=F32)
    f = []
    for j in range(ny):
        for i in range(nx):
            a = j * (nx + 1) + i
            f += [[a, a + 1, a + nx + 2], [a, a + nx + 2, a + nx + 1]]
    return v, np.asarray(f, dtype=np.int32)


def off_text(v, f, fused=False):
    head = f"OFF{len(v)} {len(f)} 0\n" if fused else f"OFF\n{len(v)} {len(f)} 0\n"
    return head + "".join("%.9g %.9g %.9g\n" % tuple(p) for p in v.tolist()) + \
        "".join("3 %d %d %d\n" % tuple(t) for t in f.tolist())


# --------------------------------------------------------------------------------------------- K26
def _cross(e1, e2):
    nx = e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1]
    ny = e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2]
    nz = e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]
    return nx, ny, nz


def areas(verts, faces):
    verts, faces = np.asarray(verts, F32), np.asarray(faces, np.int64)
    V = len(verts)
    ok = ((faces >= 0) & (faces < V)).all(axis=1)
    fc = np.where(ok[:, None], faces, 0)
    a, b, c = verts[fc[:, 0]], verts[fc[:, 1]], verts[fc[:, 2]]
    with np.errstate(all="ignore"):
        nx, ny, nz = _cross(b - a, c - a)
        s = (nx * nx + ny * ny) + nz * nz
        area = F32(0.5) * np.sqrt(s)
    area = np.where(np.isfinite(area) & ok, area, F32(0)).astype(F32)
    return area


def weights(verts, faces):
    """-> (q uint64 [F], C uint64 [F])."""
    area = areas(verts, faces)
    amax = area.max()
    if not amax > 0:
        q = np.zeros(len(area), np.uint64)
    else:
        q = np.rint(area.astype(np.float64) / np.float64(amax) * 4294967296.0).astype(np.uint64)
        q[area == 0] = 0
    return q, np.cumsum(q, dtype=np.uint64)


def unit_clamp(u):
    return np.fmin(np.fmax(np.asarray(u, F32), F32(0)), np.nextafter(F32(1), F32(0))).astype(F32)


def choose_faces(C, u0):
    T = C[-1]
    assert T > 0
    t = np.floor(unit_clamp(u0).astype(np.float64) * np.float64(T)).astype(np.uint64)
    t = np.minimum(t, T - np.uint64(1))
    return np.minimum(np.searchsorted(C, t, side="right"), len(C) - 1).astype(np.int64)


def sample(verts, faces, u):
    """-> (points float32 [m,3], face_idx int64 [m]), the bits of the kernel."""
    verts, faces, u = np.asarray(verts, F32), np.asarray(faces, np.int64), unit_clamp(u)
    _, C = weights(verts, faces)
    f = choose_faces(C, u[:, 0])
    a, b, c = verts[faces[f, 0]], verts[faces[f, 1]], verts[faces[f, 2]]
    s = np.sqrt(u[:, 1])
    w0, w1, w2 = (F32(1) - s)[:, None], (s * (F32(1) - u[:, 2]))[:, None], (s * u[:, 2])[:, None]
    with np.errstate(all="ignore"):
        return ((w0 * a + w1 * b) + w2 * c).astype(F32), f


def barycentric64(verts, faces, points, fidx):
    """float64: barycentric coordinates [m,3] of the points in their faces and their distances to the faces' planes."""
    v = np.asarray(verts, np.float64)
    a, b, c = (v[np.asarray(faces)[fidx, k]] for k in range(3))
    p = np.asarray(points, np.float64)
    n = np.cross(b - a, c - a)
    nn = (n * n).sum(axis=1)
    l1 = (np.cross(p - a, c - a) * n).sum(axis=1) / nn
    l2 = (np.cross(b - a, p - a) * n).sum(axis=1) / nn
    dist = np.abs(((p - a) * n).sum(axis=1)) / np.sqrt(nn)
    return np.stack([1 - l1 - l2, l1, l2], axis=1), dist


# --------------------------------------------------------------------------------------------- K27
def project(verts, views, ortho_scale, W, H):
    """-> cam float32 [NV,V,3], snapped int64 [NV,V,2], ok bool [NV,V]."""
    verts, views = np.asarray(verts, F32), np.asarray(views, F32).reshape(-1, 12)
    cams, snaps, oks = [], [], []
    S, os_ = F32(max(W, H)), F32(ortho_scale)
    with np.errstate(all="ignore"):
        for M in views:
            d = verts - M[9:12]
            x = (d[:, 0] * M[0] + d[:, 1] * M[1]) + d[:, 2] * M[2]
            y = (d[:, 0] * M[3] + d[:, 1] * M[4]) + d[:, 2] * M[5]
            z = (d[:, 0] * M[6] + d[:, 1] * M[7]) + d[:, 2] * M[8]
            px = (x / os_) * S + F32(0.5) * F32(W)
            py = F32(0.5) * F32(H) - (y / os_) * S
            ok = np.isfinite(px) & np.isfinite(py) & np.isfinite(z)

            def snap(p):
                q = np.fmin(np.fmax(p * F32(256), -SNAP_LIMIT), SNAP_LIMIT)
                return np.where(ok, np.rint(np.where(ok, q, F32(0))), 0).astype(np.int64)

            cams.append(np.stack([x, y, z], axis=1).astype(F32))
            snaps.append(np.stack([snap(px), snap(py)], axis=1))
            oks.append(ok)
    return np.stack(cams), np.stack(snaps), np.stack(oks)


def depth_key(z):
    b = np.asarray(z, F32).view(np.uint32).astype(np.uint64)
    neg = (b & np.uint64(0x80000000)) != 0
    return np.where(neg, ~b & np.uint64(0xFFFFFFFF), b | np.uint64(0x80000000))


def _owned(ax, ay, bx, by):
    dx, dy = bx - ax, by - ay
    return dy < 0 or (dy == 0 and dx > 0)


def _edge(ax, ay, bx, by, px, py):
    return (bx - ax) * (py - ay) - (by - ay) * (px - ax)


def rasterize(verts, faces, views, ortho_scale, W, H):
    """-> face_id int32 [NV,H,W] (-1 empty), depth float32 [NV,H,W] (+inf empty), hits int32 [NV,H,W]: how many faces
    cover each pixel centre, counted without the depth test."""
    faces = np.asarray(faces, np.int64)
    cam, snapped, ok = project(verts, views, ortho_scale, W, H)
    NV, V = ok.shape
    keys = np.full((NV, H, W), EMPTY, np.uint64)
    hits = np.zeros((NV, H, W), np.int32)
    for v in range(NV):
        for f, (a, b, c) in enumerate(faces.tolist()):
            if min(a, b, c) < 0 or max(a, b, c) >= V or not (ok[v, a] and ok[v, b] and ok[v, c]):
                continue
            (x0, y0), (x1, y1), (x2, y2) = (tuple(int(t) for t in snapped[v, k]) for k in (a, b, c))
            z0, z1, z2 = cam[v, a, 2], cam[v, b, 2], cam[v, c, 2]
            A2 = (x1 - x0) * (y2 - y0) - (y1 - y0) * (x2 - x0)
            if A2 == 0:
                continue
            if A2 < 0:
                x1, y1, z1, x2, y2, z2, A2 = x2, y2, z2, x1, y1, z1, -A2
            i0, i1 = max((min(x0, x1, x2) + 127) >> 8, 0), min((max(x0, x1, x2) - 128) >> 8, W - 1)
            j0, j1 = max((min(y0, y1, y2) + 127) >> 8, 0), min((max(y0, y1, y2) - 128) >> 8, H - 1)
            if i0 > i1 or j0 > j1:
                continue
            px = (256 * np.arange(i0, i1 + 1, dtype=np.int64) + 128)[None, :]
            py = (256 * np.arange(j0, j1 + 1, dtype=np.int64) + 128)[:, None]
            E0, E1, E2 = _edge(x1, y1, x2, y2, px, py), _edge(x2, y2, x0, y0, px, py), _edge(x0, y0, x1, y1, px, py)
            inside = (E0 >= (0 if _owned(x1, y1, x2, y2) else 1)) & (E1 >= (0 if _owned(x2, y2, x0, y0) else 1)) & \
                     (E2 >= (0 if _owned(x0, y0, x1, y1) else 1))
            A = F32(A2)
            with np.errstate(all="ignore"):
                l0, l1, l2 = E0.astype(F32) / A, E1.astype(F32) / A, E2.astype(F32) / A
                z = (l0 * z0 + l1 * z1) + l2 * z2
            inside &= np.isfinite(z)
            hits[v, j0:j1 + 1, i0:i1 + 1] += inside
            key = (depth_key(z) << np.uint64(32)) | np.uint64(f)
            win = keys[v, j0:j1 + 1, i0:i1 + 1]
            keys[v, j0:j1 + 1, i0:i1 + 1] = np.where(inside & (key < win), key, win)
    empty = keys == EMPTY
    face_id = np.where(empty, -1, (keys & np.uint64(0xFFFFFFFF)).astype(np.int64)).astype(np.int32)
    k = (keys >> np.uint64(32)).astype(np.uint32)
    bits = np.where((k & np.uint32(0x80000000)) != 0, k & np.uint32(0x7FFFFFFF), ~k).astype(np.uint32)
    depth = np.where(empty, F32(np.inf), bits.view(F32)).astype(F32)
    return face_id, depth, hits


def shade64(verts, faces, views, face_id, ssaa, params, log2_shininess, bg_image=None):
    """float64 radiance [NV, H/ssaa, W/ssaa, 3] of the definition's shading on a GIVEN face-id buffer [NV,H,W]."""
    verts, faces = np.asarray(verts, np.float64), np.asarray(faces, np.int64)
    views, p = np.asarray(views, np.float64).reshape(-1, 12), np.asarray(params, np.float64)
    ka, kd, ks, l, bg = p[0:3], p[3:6], p[6:9], p[9:12], p[12:15]
    NV, H, W = face_id.shape
    out = np.zeros((NV, H // ssaa, W // ssaa, 3))
    for v, M in enumerate(views):
        d = verts - M[9:12]
        cam = np.stack([d @ M[0:3], d @ M[3:6], d @ M[6:9]], axis=1)
        fid = face_id[v]
        hit = fid >= 0
        fc = faces[np.where(hit, fid, 0)]
        a, b, c = cam[fc[..., 0]], cam[fc[..., 1]], cam[fc[..., 2]]
        n = np.cross(b - a, c - a)
        ln = np.sqrt((n * n).sum(axis=-1, keepdims=True))
        n = np.where(ln > 0, n / np.where(ln > 0, ln, 1.0), np.array([0.0, 0.0, -1.0]))
        n = np.where(n[..., 2:3] > 0, -n, n)
        ndl = (n * l).sum(axis=-1)
        diff = np.maximum(ndl, 0.0)
        spec = np.where(ndl > 0, np.maximum(l[2] - 2.0 * ndl * n[..., 2], 0.0), 0.0) ** (2 ** log2_shininess)
        col = (ka + kd * diff[..., None] + ks * spec[..., None]) * hit[..., None]
        oh, ow = H // ssaa, W // ssaa
        acc = col.reshape(oh, ssaa, ow, ssaa, 3).sum(axis=(1, 3))
        cov = hit.reshape(oh, ssaa, ow, ssaa).sum(axis=(1, 3))[..., None] / float(ssaa * ssaa)
        back = bg if bg_image is None else np.asarray(bg_image, np.float64) / 255.0
        out[v] = acc / float(ssaa * ssaa) + back * (1.0 - cov)
    return out
