"""numpy restatement of K30 (``fpsg_episode_views``: the uint8 views of an episode -> the encoder's float batch) as
include/fpsg_hip.h defines it, and of ``fpsg_amd.views.draw``.  The blend is in int64, every float step an ``np.float32``
operation in the stated order, so the GPU result is compared bit for bit."""
import numpy as np

F = np.float32
MAX_OFFSET, MAX_STEP = 1 << 24, 1 << 16


def decode(src, sel, geom=None, color=None, size=None):
    """src uint8 [n_src,Hs,Ws,3]; sel [n]; geom int [n,4] or None; color float32 [n,4] or None -> float32 [n,3,Ho,Wo]."""
    src = np.asarray(src)
    assert src.dtype == np.uint8 and src.ndim == 4 and src.shape[3] == 3
    n_src, Hs, Ws = src.shape[:3]
    Ho, Wo = (Hs, Ws) if size is None else ((size, size) if isinstance(size, int) else size)
    n = len(sel)
    out = np.empty((n, 3, Ho, Wo), dtype=F)
    i, j = np.arange(Wo, dtype=np.int64), np.arange(Ho, dtype=np.int64)
    for k in range(n):
        s = int(sel[k])
        if not 0 <= s < n_src:
            out[k] = np.nan
            continue
        x0, y0, step = (0, 0, 256) if geom is None else (int(v) for v in geom[k][:3])
        x0, y0 = min(max(x0, -MAX_OFFSET), MAX_OFFSET), min(max(y0, -MAX_OFFSET), MAX_OFFSET)
        step = min(max(step, 1), MAX_STEP)
        X, Y = x0 + i * step, y0 + j * step
        ix, fx = X >> 8, (X & 255)[None, :, None]
        iy, fy = Y >> 8, (Y & 255)[:, None, None]
        ix0, ix1 = np.clip(ix, 0, Ws - 1), np.clip(ix + 1, 0, Ws - 1)
        iy0, iy1 = np.clip(iy, 0, Hs - 1), np.clip(iy + 1, 0, Hs - 1)
        p = src[s].astype(np.int64)                                      # [Hs, Ws, 3]
        a0 = p[iy0][:, ix0] * (256 - fx) + p[iy0][:, ix1] * fx           # [Ho, Wo, 3]
        a1 = p[iy1][:, ix0] * (256 - fx) + p[iy1][:, ix1] * fx
        v = a0 * (256 - fy) + a1 * fy
        assert v.min() >= 0 and v.max() <= 255 * 65536
        x = v.astype(F) / F(16711680.0)
        if color is not None:
            br, c, sa = (F(t) for t in color[k][:3])
            r, g, b = x[..., 0], x[..., 1], x[..., 2]
            lum = ((F(0.299) * r + F(0.587) * g) + F(0.114) * b)[..., None]
            t = lum + sa * (x - lum)
            u = (t - F(0.5)) * c + (F(0.5) + br)
            x = np.minimum(np.maximum(u, F(0)), F(1))
        assert x.dtype == F
        out[k] = ((x - F(0.5)) / F(0.5)).transpose(2, 0, 1)
    return out


def draw(u, counts, S, geom_jitter=0.0, color_jitter=0.0):
    """``views.draw`` from its uniforms ``u [n,7]`` (float64): (view int64 [n], geom int32 [n,4], color float32 [n,4] or
    None)."""
    u = np.asarray(u, dtype=np.float64)
    counts = np.asarray(counts, dtype=np.float64)
    J, C = float(geom_jitter), float(color_jitter)
    view = np.minimum(np.floor(u[:, 0] * counts), counts - 1).astype(np.int64)
    step = np.rint(256.0 * (1.0 - J + 2.0 * J * u[:, 1]))
    geom = np.zeros((len(counts), 4), dtype=np.int32)
    for axis in (0, 1):
        centre = (S - 1) / 2.0 + S * (J * u[:, 2 + axis] - J / 2.0)
        geom[:, axis] = np.rint(256.0 * centre - (S - 1) * step / 2.0).astype(np.int32)
    geom[:, 2] = step.astype(np.int32)
    color = None
    if C > 0.0:
        color = np.zeros((len(counts), 4), dtype=F)
        color[:, 0] = (C * (u[:, 6] - 0.5) / 2.0).astype(F)
        color[:, 1] = (1.0 - C + 2.0 * C * u[:, 4]).astype(F)
        color[:, 2] = (1.0 - C + 2.0 * C * u[:, 5]).astype(F)
    return view, geom, color
