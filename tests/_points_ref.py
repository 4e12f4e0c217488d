"""numpy restatement of K29 (views of point clouds as shaded spheres) as include/fpsg_hip.h defines it.  The shared steps
are ``_mesh_ref``'s (K27's projection and depth key); the integer parts are int64; the shading is one function of a
dtype: float32 with one rounding per operation for what is compared bit for bit, float64 for the error bound."""
import numpy as np

from _mesh_ref import EMPTY, F32, depth_key, project

MAX_RADIUS_PX = 64


def snapped_radius(radius, ortho_scale, W, H):
    """R as the entry forms it: from the two float32 arguments, in double, rounded half to even."""
    return int(np.rint(256.0 * (np.float64(F32(radius)) / np.float64(F32(ortho_scale))) * np.float64(max(W, H))))


def _centres(lo, hi):
    return 256 * np.arange(lo, hi + 1, dtype=np.int64) + 128


def snap_all(points, views, ortho_scale, W, H):
    """The snapped X, Y of every (cloud, view, point): int64 [B,NV,N,2]."""
    return np.stack([project(p, views, ortho_scale, W, H)[1] for p in np.asarray(points, F32)])


def rasterize(points, views, ortho_scale, radius, W, H):
    """points [B,N,3] -> point_id int32 [B,NV,H,W] (-1 empty), depth float32 (+inf empty), snapped int64 [B,NV,N,2]."""
    points = np.asarray(points, F32)
    B, N, _ = points.shape
    views = np.asarray(views, F32).reshape(-1, 12)
    NV = len(views)
    R = snapped_radius(radius, ortho_scale, W, H)
    assert 1 <= R <= 256 * MAX_RADIUS_PX
    keys = np.full((B, NV, H, W), EMPTY, np.uint64)
    snaps = np.zeros((B, NV, N, 2), np.int64)
    for b in range(B):
        cam, snapped, ok = project(points[b], views, ortho_scale, W, H)
        snaps[b] = snapped
        for v in range(NV):
            for n in np.nonzero(ok[v])[0].tolist():
                X, Y = int(snapped[v, n, 0]), int(snapped[v, n, 1])
                i0, i1 = max((X - R + 127) >> 8, 0), min((X + R - 128) >> 8, W - 1)
                j0, j1 = max((Y - R + 127) >> 8, 0), min((Y + R - 128) >> 8, H - 1)
                if i0 > i1 or j0 > j1:
                    continue
                dx, dy = (_centres(i0, i1) - X)[None, :], (_centres(j0, j1) - Y)[:, None]
                q = dx * dx + dy * dy
                inside = q < R * R
                with np.errstate(all="ignore"):
                    t = q.astype(F32) / F32(R * R)
                    c = np.sqrt(F32(1) - t)
                    zs = cam[v, n, 2] - F32(radius) * c
                inside &= np.isfinite(zs)
                key = (depth_key(zs) << np.uint64(32)) | np.uint64(n)
                win = keys[b, v, j0:j1 + 1, i0:i1 + 1]
                keys[b, v, j0:j1 + 1, i0:i1 + 1] = np.where(inside & (key < win), key, win)
    empty = keys == EMPTY
    point_id = np.where(empty, -1, (keys & np.uint64(0xFFFFFFFF)).astype(np.int64)).astype(np.int32)
    k = (keys >> np.uint64(32)).astype(np.uint32)
    bits = np.where((k & np.uint32(0x80000000)) != 0, k & np.uint32(0x7FFFFFFF), ~k).astype(np.uint32)
    depth = np.where(empty, F32(np.inf), bits.view(F32)).astype(F32)
    return point_id, depth, snaps


def shade(point_id, snaps, R, ssaa, params, log2_shininess, colors=None, bg_image=None, dtype=F32, parts=False):
    """Radiance [B,NV,H/ssaa,W/ssaa,3] in ``dtype`` of the definition's shading on a GIVEN point-id buffer.  ``params``:
    the 17 floats.  With ``parts`` also the per-sample c [B,NV,H,W] (what the error bound needs)."""
    T = dtype
    p = np.asarray(params, F32).astype(T)
    ka, kd, ks, l, bg, ambient, diffuse = p[0:3], p[3:6], p[6:9], p[9:12], p[12:15], p[15], p[16]
    B, NV, H, W = point_id.shape
    oh, ow = H // ssaa, W // ssaa
    hit = point_id >= 0
    pid = np.where(hit, point_id, 0).astype(np.int64)
    bi, vi = np.arange(B)[:, None, None, None], np.arange(NV)[None, :, None, None]
    X, Y = snaps[bi, vi, pid, 0], snaps[bi, vi, pid, 1]
    dx = np.where(hit, _centres(0, W - 1)[None, None, None, :] - X, 0)
    dy = np.where(hit, _centres(0, H - 1)[None, None, :, None] - Y, 0)
    q = dx * dx + dy * dy
    with np.errstate(all="ignore"):
        t = q.astype(T) / T(R * R)
        c = np.sqrt(T(1) - t)
        nx, ny, nz = dx.astype(T) / T(R), -(dy.astype(T) / T(R)), -c
        ndl = (nx * l[0] + ny * l[1]) + nz * l[2]
        diff = np.maximum(ndl, T(0))
        spec = np.where(ndl > 0, np.maximum(l[2] - (T(2) * ndl) * nz, T(0)), T(0))
        for _ in range(log2_shininess):
            spec = spec * spec
        diff, spec = diff[..., None], spec[..., None]
        if colors is None:
            col = (ka + kd * diff) + ks * spec
        else:
            base = np.asarray(colors, np.uint8)[bi, pid].astype(T) / T(255)
            col = (ambient * base + (diffuse * base) * diff) + ks * spec
    col = np.where(hit[..., None], col, T(0)).astype(T)
    acc = np.zeros((B, NV, oh, ow, 3), T)
    cov = np.zeros((B, NV, oh, ow), np.int64)
    for sy in range(ssaa):                                  # row-major sample order
        for sx in range(ssaa):
            acc = acc + col[:, :, sy::ssaa, sx::ssaa]
            cov += hit[:, :, sy::ssaa, sx::ssaa]
    inv = T(1) / T(ssaa * ssaa)
    rest = (T(1) - cov.astype(T) * inv)[..., None]
    back = bg if bg_image is None else np.asarray(bg_image, np.uint8).astype(T) / T(255)
    out = (acc * inv + back * rest).astype(T)
    return (out, np.where(hit, c, T(0))) if parts else out


def to_image(radiance):
    r = np.asarray(radiance, F32)
    return np.rint(np.fmin(np.fmax(r, F32(0)), F32(1)) * F32(255)).astype(np.uint8)
