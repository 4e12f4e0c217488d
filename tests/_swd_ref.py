"""numpy references of the sliced Wasserstein distance (K22) for one pair ``x, y [N,3]`` under ``dirs [L,3]``.

``ref_keys32`` forms the fp32 keys in the kernel's order of operations -- so they are the kernel's keys bit for bit --
takes the orders with ``np.lexsort((index, key))`` and accumulates the value and the gradients in float64 from those keys
and orders.  ``ref_f64`` is the same with float64 keys: the mathematical definition."""
import itertools

import numpy as np


def keys32(p, dirs):
    """``[L,N]`` fp32: ``fl(fl(fl(x tx) + fl(y ty)) + fl(z tz)) + 0.0f`` (numpy rounds every fp32 operation once)."""
    p = np.asarray(p, dtype=np.float32)
    d = np.asarray(dirs, dtype=np.float32)
    with np.errstate(all="ignore"):
        k = (p[None, :, 0] * d[:, None, 0] + p[None, :, 1] * d[:, None, 1]) + p[None, :, 2] * d[:, None, 2]
        return (k + np.float32(0.0)).astype(np.float32)


def keys64(p, dirs):
    return np.asarray(dirs, dtype=np.float64) @ np.asarray(p, dtype=np.float64).T


def orders(keys):
    """``[L,N]`` int64: per direction the indices ascending by (key, index)."""
    idx = np.arange(keys.shape[1])
    return np.stack([np.lexsort((idx, k)) for k in keys])


def _from_keys(kx, ky, dirs):
    L, N = kx.shape
    dirs = np.asarray(dirs, dtype=np.float64)
    p1, p2 = orders(kx), orders(ky)
    kx, ky = kx.astype(np.float64), ky.astype(np.float64)
    value = 0.0
    gx, gy = np.zeros((N, 3)), np.zeros((N, 3))
    for l in range(L):
        d = kx[l, p1[l]] - ky[l, p2[l]]
        value += float((d * d).sum())
        gx[p1[l]] += d[:, None] * dirs[l][None, :]
        gy[p2[l]] -= d[:, None] * dirs[l][None, :]
    return value / (L * N), 2.0 / (L * N) * gx, 2.0 / (L * N) * gy, p1, p2


def ref_keys32(x, y, dirs):
    """``(value, gx [N,3], gy [N,3], perm1 [L,N], perm2 [L,N])`` on the kernel's fp32 keys, float64 afterwards."""
    return _from_keys(keys32(x, dirs), keys32(y, dirs), dirs)


def ref_f64(x, y, dirs):
    """The same on float64 keys."""
    return _from_keys(keys64(x, dirs), keys64(y, dirs), dirs)


def value_f64(x, y, dirs):
    kx, ky = np.sort(keys64(x, dirs), axis=1), np.sort(keys64(y, dirs), axis=1)
    return float(((kx - ky) ** 2).sum()) / kx.size


def brute_force(x, y, dirs):
    """The definition without a sort: per direction the cheapest of all N! matchings, in float64."""
    kx, ky = keys64(x, dirs), keys64(y, dirs)
    L, N = kx.shape
    total = 0.0
    for l in range(L):
        total += min(float(((kx[l] - ky[l, list(perm)]) ** 2).sum()) for perm in itertools.permutations(range(N)))
    return total / (L * N)


def lattice(L):
    """The Fibonacci lattice of ``metrics.swd_directions`` in float64."""
    i = np.arange(L, dtype=np.float64)
    z = 1.0 - 2.0 * (i + 0.5) / L
    phi = i * (np.pi * (3.0 - np.sqrt(5.0)))
    rho = np.sqrt(1.0 - z * z)
    return np.stack([rho * np.cos(phi), rho * np.sin(phi), z], axis=1)


def clouds(B, N, seed, scale=0.5):
    """Two generic batches ``[B,N,3]`` fp32 (numpy)."""
    rng = np.random.default_rng(seed)
    x = (scale * rng.standard_normal((B, N, 3))).astype(np.float32)
    y = (scale * rng.standard_normal((B, N, 3)) + 0.1).astype(np.float32)
    return x, y


def unit_directions(L, seed):
    rng = np.random.default_rng(seed)
    d = rng.standard_normal((L, 3))
    return (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
