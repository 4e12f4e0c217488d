"""Numpy restatement of K33 (normals of a point cloud, ``include/fpsg_hip.h``): the neighbour lists on K1's fp32 squared
distance, bit for bit; the PCA of each neighbourhood in float64 on that same neighbour set; the spanning forest of K33b
with its fp32 weights, its tie rules and its signs.  The kernels are checked against it, never the other way."""
import numpy as np

U = 2.0 ** -24                  # the unit roundoff of fp32


def _round_odd_sum(p, c):
    """``p + c`` in float64 rounded to odd (``p``, ``c`` float64): rounding the result to fp32 then equals rounding the
    exact sum once, so an emulated fma never rounds twice."""
    s = p + c
    bp = s - p
    err = (p - (s - bp)) + (c - bp)                                # two-sum: s + err is the exact sum
    inexact = err != 0
    toward_zero = np.where(inexact & (np.sign(err) != np.sign(s)), np.nextafter(s, 0.0), s)
    bits = toward_zero.view(np.int64) | inexact.astype(np.int64)
    return bits.view(np.float64)


def fma32(a, b, c):
    """fp32 ``fma(a, b, c)``: the product of two fp32 numbers is exact in float64."""
    p = a.astype(np.float64) * b.astype(np.float64)
    return _round_odd_sum(p, np.broadcast_to(c.astype(np.float64), p.shape).copy()).astype(np.float32)


def sq_dist32(x):
    """K1's ``d2(i,j) = fma(dz,dz, fma(dy,dy, dx*dx))``, ``dx = x_j - x_i``, as fp32 ``[N,N]`` of one cloud ``x [N,3]``."""
    x = np.asarray(x, np.float32)
    d = x[None, :, :] - x[:, None, :]                              # [i, j]: fp32 differences
    return fma32(d[..., 2], d[..., 2], fma32(d[..., 1], d[..., 1], d[..., 0] * d[..., 0]))


def neighbour_lists(x, k):
    """``K(i)`` of one cloud: ``[N,k]`` int64, the k indices ``j != i`` with the smallest ``(d2, j)``, nearest first."""
    d2 = sq_dist32(x)
    np.fill_diagonal(d2, np.inf)
    return np.argsort(d2, axis=1, kind="stable")[:, :k]


def pca64(x, idx):
    """Float64 PCA of ``{i} + idx[i]`` -> ``(normal [N,3], eigenvalues [N,3] ascending, second eigenvectors [N,3,3])``."""
    x = np.asarray(x, np.float64)
    pts = np.concatenate([x[:, None, :], x[idx]], axis=1)          # [N, k + 1, 3]
    d = pts - pts.mean(axis=1, keepdims=True)
    C = np.einsum("nka,nkb->nab", d, d)
    lam, vec = np.linalg.eigh(C)
    return vec[:, :, 0], lam, vec


def angle_bound(k, lam, gap=None):
    """The issue's Davis-Kahan bound on ``sin`` of the angle to the float64 normal: ``[2 (k + 4) + 32] u trace / gap``
    (``gap`` = ``lambda1 - lambda0`` unless given)."""
    gap = lam[:, 1] - lam[:, 0] if gap is None else gap
    with np.errstate(divide="ignore", invalid="ignore"):
        return (2 * (k + 4) + 32) * U * lam.sum(axis=1) / gap


def sin_angle(a, b):
    """``sin`` of the angle between unit-ish vectors, sign-free: the norm of the cross product over the norms."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.linalg.norm(np.cross(a, b), axis=-1) / (np.linalg.norm(a, axis=-1) * np.linalg.norm(b, axis=-1))


def canonical_sign_ok(n):
    """Mode 0 on the output: the component of largest magnitude (lowest axis on ties) is positive; zero rows pass."""
    n = np.asarray(n)
    lead = n[np.arange(len(n)), np.argmax(np.abs(n), axis=1)]       # argmax: the first of equal maxima
    return (lead > 0) | (np.abs(n).max(axis=1) == 0)


def weight32(a, b):
    """``w = 1 - |(ax bx + ay by) + az bz|`` in fp32, every operation rounded on its own."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return np.float32(1) - np.abs((a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2])


def adjacency(idx, N):
    """The symmetric neighbour graph of a table ``idx [N,k]``: a list of sorted neighbour arrays."""
    adj = [set() for _ in range(N)]
    for i in range(N):
        for j in idx[i]:
            j = int(j)
            if 0 <= j < N and j != i:
                adj[i].add(j)
                adj[j].add(i)
    return [np.array(sorted(a), np.int64) for a in adj]


def forest(xyz, normals, idx, axis):
    """K33b on one cloud -> ``(normals_out [N,3] fp32, parent [N] int64 (-1 at roots), edge weights [N] fp32 (nan at
    roots), order [N])``: Prim's over the graph of ``idx`` with the fp32 weights, a key replaced only by a strictly
    smaller weight, the smallest ``(key, index)`` next, a new root at the largest ``xyz[:, axis]`` (lowest index)."""
    xyz, normals = np.asarray(xyz, np.float32), np.asarray(normals, np.float32)
    N = len(xyz)
    adj = adjacency(np.asarray(idx), N)
    key = np.full(N, np.inf, np.float32)
    has = np.zeros(N, bool)
    par = np.full(N, -1, np.int64)
    tree = np.zeros(N, bool)
    out = np.zeros((N, 3), np.float32)
    order = []
    for _ in range(N):
        cand = has & ~tree
        if cand.any():
            u = int(np.argmin(np.where(cand, key, np.inf)))        # the first of equal minima: the lowest index
            p = int(par[u])
        else:
            u = int(np.argmax(np.where(~tree, xyz[:, axis], -np.inf)))
            p = -1
            key[u] = np.nan
        n = normals[u]
        if p < 0:
            flip = n[axis] < 0
        else:
            q = out[p]
            flip = np.float32(np.float32(q[0] * n[0] + q[1] * n[1]) + q[2] * n[2]) < 0
        out[u] = -n if flip else n
        par[u] = p
        tree[u] = True
        order.append(u)
        nb = adj[u]
        nb = nb[~tree[nb]]
        if len(nb):
            w = weight32(normals[nb], n[None, :])
            lower = ~has[nb] | (w < key[nb])
            key[nb[lower]] = w[lower]
            par[nb[lower]] = u
            has[nb[lower]] = True
    return out, par, key, np.array(order)


# ---- shapes with analytic normals ---------------------------------------------------------------------------------------
def sphere(n, seed, radius=1.0, offset=(0.0, 0.0, 0.0)):
    """``(points fp32 [n,3], outward normals float64)`` of a random sphere."""
    v = np.random.default_rng(seed).standard_normal((n, 3))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    return (v * radius + np.asarray(offset)).astype(np.float32), v


def torus(n, seed, R=1.0, r=0.4):
    rng = np.random.default_rng(seed)
    a, b = rng.uniform(0, 2 * np.pi, n), rng.uniform(0, 2 * np.pi, n)
    nrm = np.stack([np.cos(b) * np.cos(a), np.cos(b) * np.sin(a), np.sin(b)], axis=1)
    ring = np.stack([np.cos(a), np.sin(a), np.zeros(n)], axis=1)
    return (R * ring + r * nrm).astype(np.float32), nrm


def cube_surface(n, seed):
    rng = np.random.default_rng(seed)
    p = rng.uniform(-1, 1, (n, 3))
    face = rng.integers(0, 6, n)
    p[np.arange(n), face % 3] = np.where(face < 3, -1.0, 1.0)
    return p.astype(np.float32)


def blob(n, seed):
    return np.random.default_rng(seed).standard_normal((n, 3)).astype(np.float32)


def planar_grid(side=5):
    """A ``side`` x ``side`` lattice in the plane z = 0.25, spacing 1/4: every d2 is exact and many are equal."""
    g = np.arange(side, dtype=np.float32) * np.float32(0.25)
    x, y = np.meshgrid(g, g, indexing="ij")
    return np.stack([x.ravel(), y.ravel(), np.full(side * side, 0.25, np.float32)], axis=1).astype(np.float32)
