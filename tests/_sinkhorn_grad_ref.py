"""Float64 reference for the Sinkhorn divergence's gradient (K19) -- test infrastructure, not product code.

The loop is that of ``oracle/sinkhorn_f64.py`` (geomloss' published ``sinkhorn_loop``: symmetric updates from the
previous duals, averaged, one final un-averaged extrapolation; its ``epsilon_schedule`` is imported), restated in torch
float64 with an optional fixed diameter.  Two routes to the gradient geomloss returns:

  ``closed_form``: d S / d x_i = (D_xx(i) - D_xy(i)) / N,  d S / d y_j = (D_yy(j) - D_yx(j)) / M  with
      D(i) = sum_j softmax_j(h_j - C_ij / e) (s_j - o_i) over the summed cloud s and the h of the final extrapolation;
  ``autograd_form``: torch autograd through the final extrapolation with geomloss' detach placement -- the loop under
      ``no_grad``, and in the last four soft-mins the duals, the summed cloud and the schedule as constants.
"""
from __future__ import annotations

import math

import torch

from oracle.sinkhorn_f64 import epsilon_schedule


def diameter_of(x, y) -> float:
    """geomloss' rule: the bounding-box diagonal over ALL points of both batches."""
    pts = torch.cat([x.reshape(-1, 3), y.reshape(-1, 3)]).double()
    return float((pts.amax(0) - pts.amin(0)).norm())


def _cost(a, b):
    return 0.5 * ((a[:, :, None, :] - b[:, None, :, :]) ** 2).sum(-1)


def _softmin(eps, C, h):
    """C [b,N,M], h [b,M] -> [b,N]"""
    return -eps * torch.logsumexp(h[:, None, :] - C / eps, dim=2)


def loop(x, y, eps_list):
    """Pairs x [b,N,3], y [b,M,3] (float64): ``(a_log, b_log, f_ba, g_ab, f_aa, g_bb)``, the duals in front of the final
    extrapolation (f on x, g on y; K2b's b_x, a_y, a_x, b_y)."""
    b, N, M = x.size(0), x.size(1), y.size(1)
    a_log = torch.full((b, N), -math.log(N), dtype=torch.float64)
    b_log = torch.full((b, M), -math.log(M), dtype=torch.float64)
    with torch.no_grad():
        C_xx, C_yy, C_xy, C_yx = _cost(x, x), _cost(y, y), _cost(x, y), _cost(y, x)
        eps = eps_list[0]
        g_ab, f_ba = _softmin(eps, C_yx, a_log), _softmin(eps, C_xy, b_log)
        f_aa, g_bb = _softmin(eps, C_xx, a_log), _softmin(eps, C_yy, b_log)
        for eps in eps_list:
            ft_ba = _softmin(eps, C_xy, b_log + g_ab / eps)
            gt_ab = _softmin(eps, C_yx, a_log + f_ba / eps)
            ft_aa = _softmin(eps, C_xx, a_log + f_aa / eps)
            gt_bb = _softmin(eps, C_yy, b_log + g_bb / eps)
            f_ba, g_ab = 0.5 * (f_ba + ft_ba), 0.5 * (g_ab + gt_ab)
            f_aa, g_bb = 0.5 * (f_aa + ft_aa), 0.5 * (g_bb + gt_bb)
    return a_log, b_log, f_ba, g_ab, f_aa, g_bb


def _final(x, y, xs, ys, e, duals):
    """The final extrapolation and the cost [b]: owners x / y, summed clouds xs / ys."""
    a_log, b_log, f_ba, g_ab, f_aa, g_bb = duals
    F_ba = _softmin(e, _cost(x, ys), b_log + g_ab / e)
    G_ab = _softmin(e, _cost(y, xs), a_log + f_ba / e)
    F_aa = _softmin(e, _cost(x, xs), a_log + f_aa / e)
    G_bb = _softmin(e, _cost(y, ys), b_log + g_bb / e)
    return (F_ba - F_aa).mean(1) + (G_ab - G_bb).mean(1)


def _displacement(e, owners, summed, h):
    w = torch.softmax(h[:, None, :] - _cost(owners, summed) / e, dim=2)
    return torch.einsum("bij,bjc->bic", w, summed) - owners * w.sum(2, keepdim=True)


def _prepare(x, y, blur, scaling, diameter):
    """float64 CPU clouds, the schedule, and the batch cut into pieces of at most ~2M pair entries each."""
    x, y = x.detach().double().cpu(), y.detach().double().cpu()
    if diameter is None:
        diameter = diameter_of(x, y)
    eps_list = epsilon_schedule(2, float(diameter), blur, scaling)
    n = max(x.size(1), y.size(1))
    step = max(1, (1 << 21) // (n * n))
    return eps_list, [(x[k:k + step], y[k:k + step]) for k in range(0, x.size(0), step)]


def closed_form(x, y, blur: float = 0.05, scaling: float = 0.5, diameter=None):
    """x [B,N,3], y [B,M,3] -> ``(S [B], gx [B,N,3], gy [B,M,3])`` float64: the value and the closed-form gradient."""
    eps_list, pieces = _prepare(x, y, blur, scaling, diameter)
    e = eps_list[-1]
    S, gx, gy = [], [], []
    for xb, yb in pieces:
        duals = loop(xb, yb, eps_list)
        a_log, b_log, f_ba, g_ab, f_aa, g_bb = duals
        S.append(_final(xb, yb, xb, yb, e, duals))
        gx.append((_displacement(e, xb, xb, a_log + f_aa / e) - _displacement(e, xb, yb, b_log + g_ab / e)) / xb.size(1))
        gy.append((_displacement(e, yb, yb, b_log + g_bb / e) - _displacement(e, yb, xb, a_log + f_ba / e)) / yb.size(1))
    return torch.cat(S), torch.cat(gx), torch.cat(gy)


def autograd_form(x, y, blur: float = 0.05, scaling: float = 0.5, diameter=None):
    """As ``closed_form``, the gradient from torch autograd with geomloss' detach placement."""
    eps_list, pieces = _prepare(x, y, blur, scaling, diameter)
    e = eps_list[-1]
    S, gx, gy = [], [], []
    for xb, yb in pieces:
        duals = loop(xb, yb, eps_list)
        xg, yg = xb.clone().requires_grad_(), yb.clone().requires_grad_()
        s = _final(xg, yg, xg.detach(), yg.detach(), e, duals)
        g1, g2 = torch.autograd.grad(s.sum(), [xg, yg])          # the items are independent
        S.append(s.detach())
        gx.append(g1)
        gy.append(g2)
    return torch.cat(S), torch.cat(gx), torch.cat(gy)


def value(x, y, blur: float = 0.05, scaling: float = 0.5, diameter=None):
    """The float64 divergence [B] alone."""
    eps_list, pieces = _prepare(x, y, blur, scaling, diameter)
    return torch.cat([_final(xb, yb, xb, yb, eps_list[-1], loop(xb, yb, eps_list)) for xb, yb in pieces])


def row_error(g, g64) -> float:
    """The measure of the parity tests: the largest row-wise Euclidean error over the largest float64 gradient row."""
    g, g64 = g.detach().double().cpu(), g64.double()
    return float((g - g64).norm(dim=-1).max() / g64.norm(dim=-1).max())


def gaussian_clouds(B, N, M, seed):
    """The inputs of the descent tests: a normal cloud divided by its largest norm against tanh(0.4 * randn)."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, N, 3, generator=g)
    x = x / x.norm(dim=-1).amax(dim=1)[:, None, None]
    return x.contiguous(), torch.tanh(0.4 * torch.randn(B, M, 3, generator=g)).contiguous()


def clouds(B, N, M, seed):
    """Unit-ball clouds against tanh(0.4 * randn) clouds, float32 on the CPU (the inputs of the Sinkhorn tests)."""
    import numpy as np
    from conftest import unit_ball_clouds
    rng = np.random.default_rng(seed)
    x = torch.from_numpy(unit_ball_clouds(rng, B, N))
    y = torch.tanh(0.4 * torch.from_numpy(rng.standard_normal((B, M, 3)))).float()
    return x.contiguous(), y.contiguous()
