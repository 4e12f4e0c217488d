"""numpy restatement of K28 (K27's shade pass with materials and textures) as include/fpsg_hip.h defines it.  One
function, ``shade``, evaluates the definition operation by operation in the dtype it is given: with float32 every
operation rounds as the kernel's does, so the result is compared bit for bit; with float64 it is the yardstick of the
error bound.  Geometry (projection, snapping, face ids) comes from ``_mesh_ref``."""
import numpy as np

import _mesh_ref as ref


def repeat_unit(u):
    with np.errstate(invalid="ignore"):
        t = u - np.floor(u)                                                    # inf - inf: NaN, which becomes 0
    return np.where((t >= 0) & (t < 1), t, t.dtype.type(0))


def lookup(tex, u, v):
    """tex uint8 [h,w,3] (row 0 on top), u and v arrays of one float dtype -> base colour [...,3] in that dtype."""
    dt = u.dtype.type
    h, w = tex.shape[:2]
    tu, tv = repeat_unit(u), repeat_unit(v)
    x = tu * dt(w) - dt(0.5)
    y = (dt(1) - tv) * dt(h) - dt(0.5)
    xf, yf = np.floor(x), np.floor(y)
    fx, fy = x - xf, y - yf
    ix0, ix1 = xf.astype(np.int64) % w, (xf.astype(np.int64) + 1) % w
    iy0, iy1 = yf.astype(np.int64) % h, (yf.astype(np.int64) + 1) % h
    gx, gy = dt(1) - fx, dt(1) - fy
    w00, w10, w01, w11 = (gx * gy)[..., None], (fx * gy)[..., None], (gx * fy)[..., None], (fx * fy)[..., None]
    c = tex.astype(dt) / dt(255)
    return ((w00 * c[iy0, ix0] + w10 * c[iy0, ix1]) + w01 * c[iy1, ix0]) + w11 * c[iy1, ix1]


def sample_uv(snapped, faces, face_uv, fid, dtype):
    """The interpolated (u, v) [H,W] at every sample centre of one view for the faces ``fid`` [H,W] (-1: empty; values
    there are meaningless), and whether the face's six uv numbers are finite."""
    H, W = fid.shape
    fc = faces[np.where(fid >= 0, fid, 0)]
    uv = face_uv[np.where(fid >= 0, fid, 0)].astype(dtype)                    # [H,W,3,2]
    s0, s1, s2 = (snapped[fc[..., k]] for k in range(3))                       # int64 [H,W,2]
    A2 = (s1[..., 0] - s0[..., 0]) * (s2[..., 1] - s0[..., 1]) - (s1[..., 1] - s0[..., 1]) * (s2[..., 0] - s0[..., 0])
    swap = A2 < 0
    s1, s2 = np.where(swap[..., None], s2, s1), np.where(swap[..., None], s1, s2)
    uv1, uv2 = np.where(swap[..., None], uv[..., 2, :], uv[..., 1, :]), np.where(swap[..., None], uv[..., 1, :], uv[..., 2, :])
    uv0 = uv[..., 0, :]
    A2 = np.abs(A2)
    px = (256 * np.arange(W, dtype=np.int64) + 128)[None, :]
    py = (256 * np.arange(H, dtype=np.int64) + 128)[:, None]

    def edge(a, b):
        return (b[..., 0] - a[..., 0]) * (py - a[..., 1]) - (b[..., 1] - a[..., 1]) * (px - a[..., 0])

    A = A2.astype(dtype)
    with np.errstate(all="ignore"):
        l0, l1, l2 = edge(s1, s2).astype(dtype) / A, edge(s2, s0).astype(dtype) / A, edge(s0, s1).astype(dtype) / A
        u = (l0 * uv0[..., 0] + l1 * uv1[..., 0]) + l2 * uv2[..., 0]
        v = (l0 * uv0[..., 1] + l1 * uv1[..., 1]) + l2 * uv2[..., 1]
    return u, v, np.isfinite(uv).all(axis=(-1, -2))


def shade(verts, faces, views, ortho_scale, face_id, ssaa, params, log2_shininess, face_material, materials, face_uv,
          textures, dtype, bg_image=None):
    """Radiance [NV, H/ssaa, W/ssaa, 3] in ``dtype`` of K28's shade and resolve on a GIVEN face-id buffer [NV,H,W].
    ``params``: the entry's 17 floats; ``materials`` [M,4]; ``textures``: a list of uint8 [h,w,3] arrays, indexed by a
    material's fourth number.  Inputs are the kernel's float32 values, converted exactly."""
    dt = np.dtype(dtype).type
    verts_t, faces = np.asarray(verts, np.float32).astype(dtype), np.asarray(faces, np.int64)
    views_t, p = np.asarray(views, np.float32).reshape(-1, 12).astype(dtype), np.asarray(params, np.float32).astype(dtype)
    ka, kd, ks, l, bg, ambient, diffuse = p[0:3], p[3:6], p[6:9], p[9:12], p[12:15], p[15], p[16]
    materials = np.asarray(materials, np.float32).reshape(-1, 4)
    M = len(materials)
    face_material = np.asarray(face_material, np.int64) if M else np.full(len(faces), -1, np.int64)
    NV, H, W = face_id.shape
    oh, ow = H // ssaa, W // ssaa
    _, snapped, _ = ref.project(verts, views, ortho_scale, W, H)
    out = np.zeros((NV, oh, ow, 3), dtype)
    with np.errstate(all="ignore"):
        for v, Mv in enumerate(views_t):
            fid = face_id[v]
            hit = fid >= 0
            safe = np.where(hit, fid, 0)
            fc = faces[safe]
            a, b, c = verts_t[fc[..., 0]], verts_t[fc[..., 1]], verts_t[fc[..., 2]]
            w1, w2 = b - a, c - a

            def turn(w):
                return [(w[..., 0] * Mv[3 * r] + w[..., 1] * Mv[3 * r + 1]) + w[..., 2] * Mv[3 * r + 2] for r in range(3)]

            (e1x, e1y, e1z), (e2x, e2y, e2z) = turn(w1), turn(w2)
            nx, ny, nz = e1y * e2z - e1z * e2y, e1z * e2x - e1x * e2z, e1x * e2y - e1y * e2x
            ln = np.sqrt((nx * nx + ny * ny) + nz * nz)
            ok = (ln > 0) & np.isfinite(ln)
            d = np.where(ok, ln, dt(1))
            nx, ny, nz = np.where(ok, nx / d, dt(0)), np.where(ok, ny / d, dt(0)), np.where(ok, nz / d, dt(-1))
            flip = nz > 0
            nx, ny, nz = np.where(flip, -nx, nx), np.where(flip, -ny, ny), np.where(flip, -nz, nz)
            ndl = (nx * l[0] + ny * l[1]) + nz * l[2]
            diff = np.maximum(ndl, dt(0))
            spec = np.where(ndl > 0, np.maximum(l[2] - (dt(2) * ndl) * nz, dt(0)), dt(0))
            for _ in range(log2_shininess):
                spec = spec * spec
            m = face_material[safe]
            bare = (m < 0) | (m >= M)
            base = np.zeros((H, W, 3), dtype)
            if M:
                mat = materials[np.where(bare, 0, m)]
                base = mat[..., :3].astype(dtype)
                tex = mat[..., 3].astype(np.int64)
                if (tex >= 0).any():
                    u, vv, finite = sample_uv(snapped[v], faces, np.asarray(face_uv, np.float32), fid, dtype)
                    for t, image in enumerate(textures):
                        use = hit & ~bare & (tex == t) & finite
                        if use.any():
                            base = np.where(use[..., None], lookup(image, np.where(use, u, dt(0)), np.where(use, vv, dt(0))),
                                            base)
            diff3, spec3 = diff[..., None], spec[..., None]
            with_material = ((ambient * base) + (diffuse * base) * diff3) + ks * spec3
            without = (ka + kd * diff3) + ks * spec3
            col = np.where(hit[..., None], np.where(bare[..., None], without, with_material), dt(0)).astype(dtype)
            acc = np.zeros((oh, ow, 3), dtype)
            for sy in range(ssaa):                                             # the kernel's order: row-major samples
                for sx in range(ssaa):
                    acc = acc + col[sy::ssaa, sx::ssaa]
            covered = hit.reshape(oh, ssaa, ow, ssaa).sum(axis=(1, 3))
            inv = dt(1) / dt(ssaa * ssaa)
            rest = (dt(1) - covered.astype(dtype) * inv)[..., None]
            back = bg if bg_image is None else np.asarray(bg_image, np.uint8).astype(dtype) / dt(255)
            out[v] = acc * inv + back * rest
    return out
