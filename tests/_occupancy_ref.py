"""CPU restatement of K15's occupancy grid (include/fpsg_hip.h) in numpy float32: a brute-force scan
of every retained node for each point whose rounded node is not retained, exactly as the definition says.  numpy's
float32 arithmetic is IEEE round-to-nearest without fused multiply-add, and ``np.rint`` rounds half to even.
Shared by the CPU and GPU tests of the Jensen-Shannon divergence; not a test module."""
import numpy as np


def retained(r: int, in_sphere: bool = True) -> np.ndarray:
    """bool [r,r,r] by the integer rule."""
    if not in_sphere:
        return np.ones((r, r, r), dtype=bool)
    a = 2 * np.arange(r, dtype=np.int64) - (r - 1)
    A, B, C = np.meshgrid(a, a, a, indexing="ij")
    return A * A + B * B + C * C <= (r - 1) ** 2


def index_coords(p: np.ndarray, r: int, E: float) -> np.ndarray:
    """t = fl(fl(p s) + c) in float32, s and c formed in double and rounded once."""
    s = np.float32((r - 1) / (2.0 * float(np.float32(E))))
    c = np.float32((r - 1) / 2.0)
    with np.errstate(all="ignore"):
        return (p.astype(np.float32) * s).astype(np.float32) + c


def cells(p: np.ndarray, r: int, E: float = 1.0, in_sphere: bool = True) -> np.ndarray:
    """The cell (linear index, -1 for a non-finite point) of every point of ``p [P,3]`` float32."""
    p = np.ascontiguousarray(p, dtype=np.float32).reshape(-1, 3)
    keep = retained(r, in_sphere)
    finite = np.isfinite(p).all(axis=1)
    t = index_coords(p, r, E)
    with np.errstate(all="ignore"):
        n0 = np.clip(np.rint(np.where(finite[:, None], t, np.float32(0))), 0, r - 1).astype(np.int64)
    lin0 = (n0[:, 0] * r + n0[:, 1]) * r + n0[:, 2]
    out = np.where(finite, lin0, -1)
    need = np.nonzero(finite & ~keep[n0[:, 0], n0[:, 1], n0[:, 2]])[0]
    if need.size:
        nodes_i = np.argwhere(keep)                                   # row-major: ascending linear index
        lin = (nodes_i[:, 0] * r + nodes_i[:, 1]) * r + nodes_i[:, 2]
        nodes = nodes_i.astype(np.float32)
        step = max(1, (1 << 22) // len(nodes))
        for k in range(0, need.size, step):
            q = t[need[k:k + step]]
            with np.errstate(all="ignore"):
                dx = q[:, None, 0] - nodes[None, :, 0]
                dy = q[:, None, 1] - nodes[None, :, 1]
                dz = q[:, None, 2] - nodes[None, :, 2]
                d = (dx * dx + dy * dy) + dz * dz
            assert d.dtype == np.float32
            out[need[k:k + step]] = lin[np.argmin(d, axis=1)]          # first minimum: the lowest linear index
    return out


def grid(clouds: np.ndarray, r: int, E: float = 1.0, in_sphere: bool = True) -> dict:
    """``cells [S,N]``, ``counts [r^3]``, ``clouds_hit [r^3]``, ``outside [3]`` of ``clouds [S,N,3]``."""
    clouds = np.ascontiguousarray(clouds, dtype=np.float32)
    S, N, _ = clouds.shape
    cl = cells(clouds.reshape(-1, 3), r, E, in_sphere).reshape(S, N)
    counts = np.bincount(cl[cl >= 0], minlength=r ** 3).astype(np.int64)
    hit = np.zeros(r ** 3, dtype=np.int64)
    for s in range(S):
        hit[np.unique(cl[s][cl[s] >= 0])] += 1
    p = clouds.reshape(-1, 3)
    finite = np.isfinite(p).all(axis=1)
    Ef = np.float32(E)
    with np.errstate(all="ignore"):
        q = p[finite]
        o0 = int((np.abs(q) > Ef).any(axis=1).sum())
        n2 = (q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1]) + q[:, 2] * q[:, 2]
        o1 = int((n2 > Ef * Ef).sum())
    return {"cells": cl, "counts": counts, "clouds_hit": hit, "outside": np.array([o0, o1, int((~finite).sum())])}


def entropy_bits(p: np.ndarray) -> float:
    p = p[p > 0]
    return float(-(p * np.log2(p)).sum())


def jsd(counts_g: np.ndarray, counts_r: np.ndarray) -> float:
    """Direct float64 restatement of the Jensen-Shannon divergence in bits."""
    P = counts_g.astype(np.float64).ravel() / counts_g.sum()
    Q = counts_r.astype(np.float64).ravel() / counts_r.sum()
    M = (P + Q) / 2
    return entropy_bits(M) - (entropy_bits(P) + entropy_bits(Q)) / 2


def ball_clouds(rng, S, N):
    """Unit-ball clouds: uniform in the ball, centred, divided by the largest norm (N >= 4)."""
    v = rng.standard_normal((S, N, 3))
    v /= np.linalg.norm(v, axis=-1, keepdims=True)
    p = v * rng.random((S, N, 1)) ** (1.0 / 3.0)
    if N >= 4:
        p = p - p.mean(axis=1, keepdims=True)
        p = p / np.sqrt((p ** 2).sum(-1)).max(axis=1)[:, None, None]
    return p.astype(np.float32)


def tanh_clouds(rng, S, N):
    """What an untrained decoder emits: tanh of a normal variate per coordinate."""
    return np.tanh(rng.standard_normal((S, N, 3))).astype(np.float32)
