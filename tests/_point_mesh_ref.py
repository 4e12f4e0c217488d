"""numpy restatement of K32 (the nearest triangle of every point) as include/fpsg_hip.h defines it.  ``point_mesh``
evaluates the definition operation by operation in the dtype it is given: with float32 every operation rounds as the
kernel's does and the result is compared bit for bit; with float64 it is the yardstick of ``dist2_bound``, the derived
first-order bound on |fp32 dist2 - float64 dist2|, which stands next to it.  ``ericson`` is an independently written
region algorithm (Ericson, Real-Time Collision Detection, 5.1.5) that the float64 restatement is checked against."""
import numpy as np

EPS = 2.0 ** -24                 # fp32 unit roundoff
BLOCK = 256                      # points evaluated at a time ([BLOCK, F, 4, 3] temporaries)


def _dot(x, y):
    return (x[..., 0] * y[..., 0] + x[..., 1] * y[..., 1]) + x[..., 2] * y[..., 2]


def _rc(x, dt):
    good = (x > 0) & np.isfinite(x)
    return np.where(good, dt(1) / np.where(good, x, dt(1)), dt(0))


def _clamp(t, dt):
    return np.fmin(np.fmax(t, dt(0)), dt(1))


def face_records(verts, faces, dtype):
    """The per-face part of the definition -> a dict of [F, ..] arrays in ``dtype``; ``ok [F]``: every index in [0, V)."""
    dt = np.dtype(dtype).type
    v = np.asarray(verts).astype(dtype)
    faces = np.asarray(faces, np.int64)
    ok = ((faces >= 0) & (faces < len(v))).all(axis=1)
    fc = np.where(ok[:, None], faces, 0)
    a, b, c = v[fc[:, 0]], v[fc[:, 1]], v[fc[:, 2]]
    with np.errstate(all="ignore"):
        e0, e1, e2 = b - a, c - a, c - b
        d00, d01, d11, d22 = _dot(e0, e0), _dot(e0, e1), _dot(e1, e1), _dot(e2, e2)
        det = d00 * d11 - d01 * d01
        return dict(a=a, b=b, c=c, e0=e0, e1=e1, e2=e2, d00=d00, d01=d01, d11=d11, d22=d22, det=det, r0=_rc(d00, dt),
                    r1=_rc(d11, dt), r2=_rc(d22, dt), rd=_rc(det, dt), ok=ok)


def pair_candidates(p, R, dtype):
    """``p [n,3]`` against every face of ``R`` -> ``d [n,F,4]`` (the interior's +inf where it is not valid, NaN kept),
    ``q [n,F,4,3]``, ``t [n,F,3]`` (t0, t1, t2), ``v`` and ``w [n,F]``."""
    dt = np.dtype(dtype).type
    p = p[:, None, :]
    a, b, e0, e1, e2 = (R[k][None] for k in ("a", "b", "e0", "e1", "e2"))
    with np.errstate(all="ignore"):
        ap, bp = p - a, p - b
        s0, s1, s2 = _dot(ap, e0), _dot(ap, e1), _dot(bp, e2)
        t0, t1, t2 = _clamp(s0 * R["r0"], dt), _clamp(s1 * R["r1"], dt), _clamp(s2 * R["r2"], dt)
        q0, q1, q2 = a + e0 * t0[..., None], a + e1 * t1[..., None], b + e2 * t2[..., None]
        v = (R["d11"] * s0 - R["d01"] * s1) * R["rd"]
        w = (R["d00"] * s1 - R["d01"] * s0) * R["rd"]
        qi = a + (e0 * v[..., None] + e1 * w[..., None])
        valid = (R["rd"] > 0) & (v >= 0) & (w >= 0) & (v + w <= 1)
        q = np.stack([q0, q1, q2, qi], axis=2)
        r = p[:, :, None, :] - q
        d = _dot(r, r)
        d[..., 3] = np.where(valid, d[..., 3], dt(np.inf))
    return d, q, np.stack([t0, t1, t2], axis=-1), v, w


def point_mesh(points, verts, faces, dtype):
    """One cloud ``[N,3]`` against one mesh -> ``(dist2 [N], face [N] int64, closest [N,3], bary [N,3])`` in ``dtype``."""
    dt = np.dtype(dtype).type
    pts = np.asarray(points).astype(dtype)
    R = face_records(verts, faces, dtype)
    N = len(pts)
    dist2, face = np.full(N, np.inf, dtype), np.full(N, -1, np.int64)
    closest, bary = np.full((N, 3), np.nan, dtype), np.full((N, 3), np.nan, dtype)
    for lo in range(0, N, BLOCK):
        p = pts[lo:lo + BLOCK]
        d, q, t, v, w = pair_candidates(p, R, dtype)
        with np.errstate(all="ignore"):
            m = np.fmin(np.fmin(np.fmin(d[..., 0], d[..., 1]), d[..., 2]), d[..., 3])        # [n,F]
            m = np.where(R["ok"][None] & ~np.isnan(m), m, dt(np.inf))
            f = np.argmin(m, axis=1)                                                         # the first minimum
            rows = np.arange(len(p))
            best = m[rows, f]
            won = best < np.inf
            dw = d[rows, f]                                                                  # [n,4]
            k = np.argmax(dw == best[:, None], axis=1)                                       # the first equal candidate
            tk = t[rows, f, np.minimum(k, 2)]
            vv, ww = v[rows, f], w[rows, f]
            one, zero = dt(1), np.zeros_like(tk)
            weights = np.stack([np.stack([one - tk, tk, zero], -1), np.stack([one - tk, zero, tk], -1),
                                np.stack([zero, one - tk, tk], -1), np.stack([(one - vv) - ww, vv, ww], -1)], axis=1)
        dist2[lo:lo + BLOCK] = np.where(won, best, dt(np.inf))
        face[lo:lo + BLOCK] = np.where(won, f, -1)
        closest[lo:lo + BLOCK] = np.where(won[:, None], q[rows, f, k], dt(np.nan))
        bary[lo:lo + BLOCK] = np.where(won[:, None], weights[rows, k], dt(np.nan))
    return dist2, face, closest, bary


def point_mesh_batch(points, verts, faces, dtype):
    """``points [B,N,3]``, ``verts [V,3]`` or ``[B,V,3]`` -> the four outputs stacked over B."""
    points, verts = np.asarray(points), np.asarray(verts)
    outs = [point_mesh(points[b], verts if verts.ndim == 2 else verts[b], faces, dtype) for b in range(len(points))]
    return tuple(np.stack(x) for x in zip(*outs))


# ------------------------------------------------------------------------------------------- bound
def dist2_bound(points, verts, faces):
    """Bound, per point, on |fp32 dist2 - float64 dist2| for the operations the header lists, u = 2^-24, evaluated on the
    float64 values (no underflow, no overflow).  |x| of a vector is Euclidean, and the inputs are the same float32
    numbers on both sides.

    Per face:
      an edge component e = b - a is one rounding, |de| <= u |e|; so is a component of ap = p - a and bp = p - b;
      dkk = dot(e,e) of non-negative terms: 2 u carried by the edge, a product and two additions: 5 u dkk;
      d01: 5 u D01, D01 = sum_c |e0_c e1_c|;   rk = 1 / dkk: 6 u rk.
    Per pair:
      sk = dot(ap, ek): 2 u carried, a product and two additions: ds_k = 5 u A_k, A_k = sum_c |ap_c ek_c|;
      t_raw = sk rk: dt_k = ds_k / dkk + 7 u |t_raw|; the clamp does not stretch it, and when t_raw is beyond [0, 1] by
        more than dt_k both sides clamp to the same end: dt_k = 0;
      qk = a + ek t, per component an edge, a product, an addition:  |dqk| <= |ek| dt_k + 2 u |ek| t + u |qk|;
      v = (d11 s0 - d01 s1) rd: the numerator n_v carries
        dn_v = 6 u d11 |s0| + d11 ds_0 + 5 u D01 |s1| + u |d01 s1| + |d01| ds_1 + u |n_v|,
        det carries ddet = 11 u d00 d11 + 10 u D01 |d01| + u d01^2 + u |det|, rd its relative error
        rho = ddet / (det - ddet) + u (infinite when ddet >= det: a sliver's interior candidate has no bound),
        dv = dn_v rd + |v| (rho + u); dw likewise;
      qI = a + (e0 v + e1 w):  |dqI| <= |e0| dv + |e1| dw + 3 u (|e0| |v| + |e1| |w|) + u |qI|;
      d(q) = dot(r, r), r = p - q: |dr| <= |dq| + u |r|, products and additions of non-negative terms 3 u d:
        beta = 2 |r| |dr| + |dr|^2 + 3 u d.
      Validity of qI: when v, w or 1 - v - w is within its own error (dv, dw, dv + dw + 2 u) of zero, the two sides may
        disagree about it.  The plane's foot is then within sigma = (|e0| + |e1|) (dv + dw + 2 u) of a point of an edge,
        and p - qI is normal to the plane, so the nearest edge candidate lies within (|r_I| + sigma)^2: the candidate
        gets flip = 2 |r_I| sigma + sigma^2 on top of the larger of its own beta and that edge candidate's (the side
        that drops qI falls back on it), and counts whether valid or not.
    Per point, with y the float64 values and i the float64 winner over all (face, candidate) entries: the fp32 minimum is
      at most y_i + beta_i, and it is reached by an entry j that can only be one with y_j - beta_j <= y_i + beta_i, which
      it undercuts by at most beta_j: the bound is the largest beta among those entries.
    -> [N] float64 (inf where no face is usable)."""
    u = EPS
    pts = np.asarray(points).astype(np.float64)
    R = face_records(verts, faces, np.float64)
    norm = np.linalg.norm
    e0n, e1n, e2n = norm(R["e0"], axis=-1), norm(R["e1"], axis=-1), norm(R["e2"], axis=-1)
    D01 = np.abs(R["e0"] * R["e1"]).sum(-1)
    d00, d01, d11, d22, det = R["d00"], R["d01"], R["d11"], R["d22"], R["det"]
    out = np.full(len(pts), np.inf)
    with np.errstate(all="ignore"):
        ddet = 11 * u * d00 * d11 + 10 * u * D01 * np.abs(d01) + u * d01 * d01 + u * np.abs(det)
        rho = np.where(det > ddet, ddet / np.where(det > ddet, det - ddet, 1.0), np.inf) + u
        for lo in range(0, len(pts), BLOCK):
            p = pts[lo:lo + BLOCK]
            d, q, t, v, w = pair_candidates(p, R, np.float64)
            ap, bp = p[:, None] - R["a"][None], p[:, None] - R["b"][None]
            s = [_dot(ap, R["e0"][None]), _dot(ap, R["e1"][None]), _dot(bp, R["e2"][None])]
            ds = [5 * u * np.abs(x * e[None]).sum(-1) for x, e in ((ap, R["e0"]), (ap, R["e1"]), (bp, R["e2"]))]
            dq = []
            for k, (dkk, en) in enumerate(((d00, e0n), (d11, e1n), (d22, e2n))):
                traw = s[k] * _rc(dkk, np.float64)
                dtk = np.where(dkk > 0, ds[k] / np.where(dkk > 0, dkk, 1.0), 0.0) + 7 * u * np.abs(traw)
                dtk = np.where((traw - dtk > 1) | (traw + dtk < 0), 0.0, dtk)
                dq.append(en * dtk + 2 * u * en * t[..., k] + u * norm(q[:, :, k], axis=-1))
            nv, nw = d11 * s[0] - d01 * s[1], d00 * s[1] - d01 * s[0]
            dnv = 6 * u * d11 * np.abs(s[0]) + d11 * ds[0] + 5 * u * D01 * np.abs(s[1]) + u * np.abs(d01 * s[1]) + \
                np.abs(d01) * ds[1] + u * np.abs(nv)
            dnw = 6 * u * d00 * np.abs(s[1]) + d00 * ds[1] + 5 * u * D01 * np.abs(s[0]) + u * np.abs(d01 * s[0]) + \
                np.abs(d01) * ds[0] + u * np.abs(nw)
            dv = dnv * R["rd"] + np.abs(v) * (rho + u)
            dw = dnw * R["rd"] + np.abs(w) * (rho + u)
            dq.append(e0n * dv + e1n * dw + 3 * u * (e0n * np.abs(v) + e1n * np.abs(w)) + u * norm(q[:, :, 3], axis=-1))
            dq = np.stack(dq, axis=-1)                                                       # [n,F,4]
            r = p[:, None, None, :] - q
            y = _dot(r, r)                                      # the interior's value whether valid or not
            rn = np.sqrt(y)
            dr = dq + u * rn
            beta = 2 * rn * dr + dr * dr + 3 * u * y
            usable = (R["rd"] > 0) & np.isfinite(rho)
            near = usable & ((np.abs(v) <= dv) | (np.abs(w) <= dw) | (np.abs(1 - v - w) <= dv + dw + 2 * u))
            sigma = (e0n + e1n) * (dv + dw + 2 * u)
            flip = 2 * rn[..., 3] * sigma + sigma * sigma
            edge = np.take_along_axis(beta[..., :3], np.argmin(y[..., :3], axis=-1)[..., None], axis=-1)[..., 0]
            beta[..., 3] = np.where(near, np.maximum(beta[..., 3], edge) + flip, beta[..., 3])
            beta[..., 3] = np.where(R["rd"] > 0, beta[..., 3], 0.0)           # det = 0 on both sides: no candidate
            valid = np.isfinite(d[..., 3])
            y[..., 3] = np.where(valid | near, y[..., 3], np.inf)
            skip = ~R["ok"][None, :, None] | np.isnan(y)
            y = np.where(skip, np.inf, y).reshape(len(p), -1)
            beta = np.where(skip, 0.0, beta).reshape(len(p), -1)
            true = np.where(skip, np.inf, d).reshape(len(p), -1)                             # the float64 result's entries
            i = np.argmin(true, axis=1)
            rows = np.arange(len(p))
            top = true[rows, i] + beta[rows, i]
            can_win = (y - beta <= top[:, None]) & np.isfinite(y)
            out[lo:lo + BLOCK] = np.where(np.isfinite(true[rows, i]), np.where(can_win, beta, 0.0).max(axis=1), np.inf)
    return out


def _extent(verts, faces):
    """(the longest edge, the largest |vertex|) of the usable faces, float64."""
    R = face_records(verts, faces, np.float64)
    ok = R["ok"]
    longest = max(np.linalg.norm(R[k][ok], axis=-1).max() for k in ("e0", "e1", "e2"))
    return longest, max(np.linalg.norm(R[k][ok], axis=-1).max() for k in ("a", "b", "c"))


def one_sided_slacks(points, verts, faces, d64):
    """Two bounds that hold for every mesh, slivers included, because they do not pass through 1 / det.  E: the longest
    edge, Q: the largest |vertex|, u = 2^-24, ``d64`` the float64 result [N].  -> (below, above, T), [N] each.

    below: fp32 dist2 >= d64 - below.  Whatever t, v and w are worth, they are in [0, 1] (v + w <= 1 for a valid qI), so
      the exact a + e t or a + (e0 v + e1 w) is a point of the triangle and the fp32 candidate lies within
      delta = u (6 E + Q) of it (per component an edge 1 u, a product 1 u, the inner sum 1 u: 3 u (|e0| + |e1|), and the
      outer sum u |q|).  Its r = p - q carries u |r| more and dot(r, r) 3 u: fp32 dist2 >= (sqrt(d64) - delta)^2 (1 - 5 u)
      >= d64 - 2 sqrt(d64) delta - 5 u d64.
    above: fp32 dist2 <= T + above, T the float64 squared distance to the nearest vertex of a usable face.  That vertex
      ends an edge whose candidate q(t) has d(q(t)) = d* + |e|^2 (t - t*)^2 <= T + (|e| dt)^2 in exact arithmetic (t* the
      exact parameter, clamped), with |e| dt <= 5 u |ap| + 7 u |e| <= u (5 (sqrt(T) + E) + 7 E) =: s from dist2_bound's
      dt_k; the candidate's own roundings move it by dq = u (2 E + Q), the difference by u |r|, the dot by 3 u:
      fp32 dist2 <= (sqrt(T + s^2) (1 + u) + dq)^2 (1 + 3 u)."""
    u = EPS
    E, Q = _extent(verts, faces)
    pts = np.asarray(points).astype(np.float64)
    R = face_records(verts, faces, np.float64)
    used = np.concatenate([R[k][R["ok"]] for k in ("a", "b", "c")])
    T = np.full(len(pts), np.inf)
    for lo in range(0, len(used), 4096):
        T = np.minimum(T, ((pts[:, None, :] - used[None, lo:lo + 4096]) ** 2).sum(-1).min(axis=1))
    root = np.sqrt(d64)
    delta = u * (6 * E + Q)
    below = 2 * root * delta + 5 * u * d64 + delta * delta
    s = u * (5 * (np.sqrt(T) + E) + 7 * E)
    above = (np.sqrt(T + s * s) * (1 + u) + u * (2 * E + Q)) ** 2 * (1 + 3 * u) - T
    return below, above, T


# ------------------------------------------------------------------------- an independent yardstick
def ericson(p, a, b, c):
    """Squared distance from ``p`` to the triangle ``a, b, c`` (arrays [..,3], float64) by Voronoi regions."""
    p, a, b, c = (np.asarray(x, np.float64) for x in (p, a, b, c))
    ab, ac, ap = b - a, c - a, p - a
    d1, d2 = (ab * ap).sum(-1), (ac * ap).sum(-1)
    bp = p - b
    d3, d4 = (ab * bp).sum(-1), (ac * bp).sum(-1)
    cp = p - c
    d5, d6 = (ab * cp).sum(-1), (ac * cp).sum(-1)
    vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
    with np.errstate(all="ignore"):
        denom = 1.0 / (va + vb + vc)
        v_in, w_in = vb * denom, vc * denom
        t_ab = d1 / (d1 - d3)
        t_ac = d2 / (d2 - d6)
        t_bc = (d4 - d3) / ((d4 - d3) + (d5 - d6))
    X = lambda s: np.asarray(s)[..., None]
    q = a + ab * X(v_in) + ac * X(w_in)                                                   # inside the face
    cond = (va <= 0) & (d4 - d3 >= 0) & (d5 - d6 >= 0)
    q = np.where(X(cond), b + (c - b) * X(t_bc), q)
    cond = (vb <= 0) & (d2 >= 0) & (d6 <= 0)
    q = np.where(X(cond), a + ac * X(t_ac), q)
    cond = (d6 >= 0) & (d5 <= d6)
    q = np.where(X(cond), c, q)
    cond = (vc <= 0) & (d1 >= 0) & (d3 <= 0)
    q = np.where(X(cond), a + ab * X(t_ab), q)
    cond = (d3 >= 0) & (d4 <= d3)
    q = np.where(X(cond), b, q)
    cond = (d1 <= 0) & (d2 <= 0)
    q = np.where(X(cond), a, q)
    r = p - q
    return (r * r).sum(-1)
