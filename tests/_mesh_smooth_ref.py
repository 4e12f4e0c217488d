"""numpy restatement of K31 as include/fpsg_hip.h defines it: the area-weighted vertex normals (K31a) and the smooth
shade pass (K31b).  Each function evaluates the definition operation by operation in the dtype it is given: with float32
every operation rounds as the kernel's does and the result is compared bit for bit; with float64 it is the yardstick of
the error bounds, which are derived here next to it.  Projection, snapping, the barycentric interpolation, the texel
lookup and the resolve are K27's and K28's and come from ``_mesh_ref`` / ``_mesh_material_ref``."""
import numpy as np

import _mesh_material_ref as mref
import _mesh_ref as ref

EPS = 2.0 ** -24                 # fp32 unit roundoff


# --------------------------------------------------------------------------------------------- K31a
def _face_products(verts, faces):
    """The un-normalised cross products (b - a) x (c - a) [.., F, 3] (dtype of verts) and which faces are in range."""
    V = verts.shape[-2]
    ok = ((faces >= 0) & (faces < V)).all(axis=1)
    fc = np.where(ok[:, None], faces, 0)
    a, b, c = verts[..., fc[:, 0], :], verts[..., fc[:, 1], :], verts[..., fc[:, 2], :]
    e1, e2 = b - a, c - a
    with np.errstate(all="ignore"):
        n = np.stack([e1[..., 1] * e2[..., 2] - e1[..., 2] * e2[..., 1],
                      e1[..., 2] * e2[..., 0] - e1[..., 0] * e2[..., 2],
                      e1[..., 0] * e2[..., 1] - e1[..., 1] * e2[..., 0]], axis=-1)
    return n, ok, fc


def vertex_normals(verts, faces, dtype):
    """``verts`` [V,3] or [B,V,3] (the kernel's float32 values, converted exactly; float64 values are taken as they are),
    ``faces`` [F,3] -> normals of the same shape in ``dtype``: the faces' products summed per vertex in ascending face
    order, once per corner, then divided by the sum's length; zero where that is 0 or not finite.  Faces with an index
    outside [0, V) contribute nothing."""
    verts_t = np.asarray(verts).astype(dtype)
    faces = np.asarray(faces, np.int64)
    n, ok, fc = _face_products(verts_t, faces)
    s = np.zeros_like(verts_t)
    with np.errstate(all="ignore"):
        for f in np.nonzero(ok)[0]:
            for corner in range(3):
                s[..., fc[f, corner], :] = s[..., fc[f, corner], :] + n[..., f, :]
        ln = np.sqrt((s[..., 0] * s[..., 0] + s[..., 1] * s[..., 1]) + s[..., 2] * s[..., 2])[..., None]
        good = (ln > 0) & np.isfinite(ln)
        return np.where(good, s / np.where(good, ln, 1), 0).astype(dtype)


def normals_bound(verts, faces):
    """First-order bound, per vertex, on |fp32 normal - float64 normal| (Euclidean) for the operations the header lists,
    eps = 2^-24, evaluated on the float64 values:
      an edge component e = b - a is one rounding: eps |e| (the inputs are the same float32 numbers on both sides);
      a product's component p - q, p and q products of two edge components: each product carries 2 eps from its edges
        and eps of its own, the subtraction eps |p - q| <= eps (|p| + |q|):  dn_c <= 4 eps (|p| + |q|);
      the sum over a vertex's k corners, sequential: every addition rounds a partial sum that is at most
        A_c = sum_j |n_jc|, so the k - 1 additions (the first adds to zero) give (k - 1) eps A_c:
        ds_c <= sum_j dn_jc + (k - 1) eps A_c;   ds = the length of (ds_x, ds_y, ds_z);
      normalisation (three squares, two additions, sqrt, a division): the direction moves by ds / |s|, the arithmetic
        adds 3.5 eps, as in K27's bound (test_meshes_gpu._shading_bound).
    -> ds / |s| + 3.5 eps, [.., V]; inf where the float64 sum is zero (such vertices are compared with zero exactly)."""
    v = np.asarray(verts).astype(np.float64)
    faces = np.asarray(faces, np.int64)
    V = v.shape[-2]
    n, ok, fc = _face_products(v, faces)
    a, b, c = v[..., fc[:, 0], :], v[..., fc[:, 1], :], v[..., fc[:, 2], :]
    e1, e2 = np.abs(b - a), np.abs(c - a)
    dn = 4 * EPS * np.stack([e1[..., 1] * e2[..., 2] + e1[..., 2] * e2[..., 1],
                             e1[..., 2] * e2[..., 0] + e1[..., 0] * e2[..., 2],
                             e1[..., 0] * e2[..., 1] + e1[..., 1] * e2[..., 0]], axis=-1)
    s, ds, A = np.zeros_like(v), np.zeros_like(v), np.zeros_like(v)
    k = np.zeros(V)
    for f in np.nonzero(ok)[0]:
        for corner in range(3):
            i = fc[f, corner]
            s[..., i, :] += n[..., f, :]
            ds[..., i, :] += dn[..., f, :]
            A[..., i, :] += np.abs(n[..., f, :])
            k[i] += 1
    ds = ds + np.maximum(k - 1, 0)[:, None] * EPS * A
    ln = np.linalg.norm(s, axis=-1)
    with np.errstate(all="ignore"):
        return np.where(ln > 0, np.linalg.norm(ds, axis=-1) / ln + 3.5 * EPS, np.inf)


# --------------------------------------------------------------------------------------------- K31b
def _interpolate(snapped, faces, face_normals, fid, dtype):
    """m = (l0 n0 + l1 n1) + l2 n2 per component at every sample centre of one view -> three [H,W] arrays.  K28's
    interpolation of a corner attribute (``_mesh_material_ref.sample_uv``: its barycentrics, its swap of corners 1 and 2
    and of what they carry) applied to the normals' components, two at a time."""
    mx, my, _ = mref.sample_uv(snapped, faces, face_normals[..., 0:2], fid, dtype)
    mz, _, _ = mref.sample_uv(snapped, faces, face_normals[..., 2:3].repeat(2, axis=-1), fid, dtype)
    return mx, my, mz


def shade_smooth(verts, faces, views, ortho_scale, face_id, ssaa, params, log2_shininess, face_normals, face_material,
                 materials, face_uv, textures, dtype, bg_image=None, return_length=False):
    """Radiance [NV, H/ssaa, W/ssaa, 3] in ``dtype`` of K31b's shade and K27's resolve on a GIVEN face-id buffer
    [NV,H,W].  Arguments as ``_mesh_material_ref.shade`` plus ``face_normals`` [F,3,3] (``materials`` may be empty: M = 0).
    With ``return_length`` also |m| in the camera frame per sample [NV,H,W] (NaN where nothing is covered)."""
    dt = np.dtype(dtype).type
    verts_t, faces = np.asarray(verts, np.float32).astype(dtype), np.asarray(faces, np.int64)
    views_t, p = np.asarray(views, np.float32).reshape(-1, 12).astype(dtype), np.asarray(params, np.float32).astype(dtype)
    ka, kd, ks, l, bg, ambient, diffuse = p[0:3], p[3:6], p[6:9], p[9:12], p[12:15], p[15], p[16]
    materials = np.asarray(materials, np.float32).reshape(-1, 4)
    face_normals = np.asarray(face_normals, np.float32)
    M = len(materials)
    face_material = np.asarray(face_material, np.int64) if M else np.full(len(faces), -1, np.int64)
    NV, H, W = face_id.shape
    oh, ow = H // ssaa, W // ssaa
    _, snapped, _ = ref.project(verts, views, ortho_scale, W, H)
    out = np.zeros((NV, oh, ow, 3), dtype)
    length = np.full((NV, H, W), np.nan)
    with np.errstate(all="ignore"):
        for v, Mv in enumerate(views_t):
            fid = face_id[v]
            hit = fid >= 0
            safe = np.where(hit, fid, 0)
            fc = faces[safe]
            a, b, c = verts_t[fc[..., 0]], verts_t[fc[..., 1]], verts_t[fc[..., 2]]

            def turn(w):
                return [(w[0] * Mv[3 * r] + w[1] * Mv[3 * r + 1]) + w[2] * Mv[3 * r + 2] for r in range(3)]

            # g: K27's face normal, operation for operation
            (e1x, e1y, e1z), (e2x, e2y, e2z) = turn(np.moveaxis(b - a, -1, 0)), turn(np.moveaxis(c - a, -1, 0))
            gx, gy, gz = e1y * e2z - e1z * e2y, e1z * e2x - e1x * e2z, e1x * e2y - e1y * e2x
            ln = np.sqrt((gx * gx + gy * gy) + gz * gz)
            ok = (ln > 0) & np.isfinite(ln)
            d = np.where(ok, ln, dt(1))
            gx, gy, gz = np.where(ok, gx / d, dt(0)), np.where(ok, gy / d, dt(0)), np.where(ok, gz / d, dt(-1))
            flip = gz > 0
            gx, gy, gz = np.where(flip, -gx, gx), np.where(flip, -gy, gy), np.where(flip, -gz, gz)
            # c: the interpolated normal in the camera frame, on g's side; g where it has no length
            tx, ty, tz = turn(_interpolate(snapped[v], faces, face_normals, fid, dtype))
            ml = np.sqrt((tx * tx + ty * ty) + tz * tz)
            usable = (ml > 0) & np.isfinite(ml)
            d = np.where(usable, ml, dt(1))
            cx, cy, cz = tx / d, ty / d, tz / d
            back = ((cx * gx + cy * gy) + cz * gz) < 0
            cx, cy, cz = np.where(back, -cx, cx), np.where(back, -cy, cy), np.where(back, -cz, cz)
            nx, ny, nz = np.where(usable, cx, gx), np.where(usable, cy, gy), np.where(usable, cz, gz)
            length[v] = np.where(hit, ml, np.nan)
            ndl = (nx * l[0] + ny * l[1]) + nz * l[2]
            diff = np.maximum(ndl, dt(0))
            spec = np.where(ndl > 0, np.maximum(l[2] - (dt(2) * ndl) * nz, dt(0)), dt(0))
            for _ in range(log2_shininess):
                spec = spec * spec
            # the base colour and the resolve: K28's
            m = face_material[safe]
            bare = (m < 0) | (m >= M)
            base = np.zeros((H, W, 3), dtype)
            if M:
                mat = materials[np.where(bare, 0, m)]
                base = mat[..., :3].astype(dtype)
                tex = mat[..., 3].astype(np.int64)
                if (tex >= 0).any():
                    u, vv, finite = mref.sample_uv(snapped[v], faces, np.asarray(face_uv, np.float32), fid, dtype)
                    for t, image in enumerate(textures):
                        use = hit & ~bare & (tex == t) & finite
                        if use.any():
                            base = np.where(use[..., None],
                                            mref.lookup(image, np.where(use, u, dt(0)), np.where(use, vv, dt(0))), base)
            diff3, spec3 = diff[..., None], spec[..., None]
            with_material = ((ambient * base) + (diffuse * base) * diff3) + ks * spec3
            without = (ka + kd * diff3) + ks * spec3
            col = np.where(hit[..., None], np.where(bare[..., None], without, with_material), dt(0)).astype(dtype)
            acc = np.zeros((oh, ow, 3), dtype)
            for sy in range(ssaa):
                for sx in range(ssaa):
                    acc = acc + col[sy::ssaa, sx::ssaa]
            covered = hit.reshape(oh, ssaa, ow, ssaa).sum(axis=(1, 3))
            inv = dt(1) / dt(ssaa * ssaa)
            rest = (dt(1) - covered.astype(dtype) * inv)[..., None]
            behind = bg if bg_image is None else np.asarray(bg_image, np.uint8).astype(dtype) / dt(255)
            out[v] = acc * inv + behind * rest
    return (out, length) if return_length else out


def smooth_bound(length, params, shininess, normal_size=1.0):
    """First-order bound on |fp32 radiance - float64 radiance| of a smooth-shaded sample whose interpolated normal has the
    length ``length`` (= |m|, an array), eps = 2^-24, for the operations the header lists (K31b).  It is K27's chain
    (test_meshes_gpu._shading_bound) from the unit normal on, with the unit normal's error rho taken from the
    interpolation and the second normalisation instead of from the face's edges:
      l_k = (float) E_k / (float) A2: three roundings, 3 eps l_k, with l_k >= 0 and l0 + l1 + l2 = 1 at a covered sample;
      a component of m = (l0 n0 + l1 n1) + l2 n2: 3 eps carried, a product and at most two additions, 6 eps sum_k l_k
        |n_kc| <= 6 eps N, N the largest corner normal's length: a vector error of 6 sqrt(3) eps N = 10.4 eps N;
      turned by three 3-term dot products with unit rows: the carried error keeps its length, each component adds
        3 eps |m|: sqrt(3) 3 eps |m| = 5.2 eps |m| <= 5.2 eps N;
      normalisation: the direction moves by (10.4 + 5.2) eps N / |m|, the arithmetic adds 3.5 eps (as K27's):
        rho = 15.6 eps N / |m| + 3.5 eps;
      the side test (c.g < 0) changes nothing as long as |c.g| is far above rho and the face normal's own error, which
        the callers assert;
      n.l: rho + 3 eps;   s = l_z - (2 n.l) n_z: 2 (rho + 3 eps + rho) + 3 eps;   s^S by log2 S squarings: S ds + (S - 1) eps;
      colour: kd (d(n.l) + eps) + ks (d(spec) + eps) + 2 eps, kd and ks the largest of their three (with a material
        kd = diffuse b <= diffuse, and ambient b and diffuse b add 2 eps); the resolve: 14 eps more."""
    p = np.asarray(params, np.float64)
    kd = max(p[3:6].max(), p[16]) if len(p) > 16 else p[3:6].max()
    S = shininess
    rho = 15.6 * EPS * normal_size / length + 3.5 * EPS
    d_ndl = rho + 3 * EPS
    d_s = 2 * (d_ndl + rho) + 3 * EPS
    d_spec = S * d_s + (S - 1) * EPS
    return kd * (d_ndl + EPS) + p[6:9].max() * (d_spec + EPS) + 4 * EPS + 14 * EPS
