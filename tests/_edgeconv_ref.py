"""CPU references of the fused EdgeConv layer (K4b): numpy / torch only, no oracle, no ``fpsg_amd``.

``PQ [B,N,2Co]`` fp32 holds ``P`` (first ``Co`` columns) and ``Q``; an edge activation is
``y[b,n,j,c] = P[b,idx[b,n,j],c] + Q[b,n,c]`` formed as ONE fp32 addition, which numpy reproduces bit for bit.  With
``PQ`` as the exact input the selected value and slot are therefore exact, and everything behind the selection is
smooth: ``forward_exact`` is the kernels' forward, ``backward_per_edge`` the backward from its per-edge definition in
float64 (not the kernels' regrouped closing formula), ``layer64`` the whole of ``_EdgeConvBNMax`` in float64 with torch
autograd.  float64 work runs cloud by cloud, so the largest temporary is one ``[N,k,Co]`` float64 array."""
from types import SimpleNamespace

import numpy as np
import torch

EPS32 = 2.0 ** -24          # unit roundoff of fp32


def edge_values(PQ, idx):
    """``y [B,N,k,Co]`` fp32: one fp32 addition per element."""
    PQ = np.asarray(PQ, dtype=np.float32)
    idx = np.asarray(idx)
    B, N, Co2 = PQ.shape
    Co = Co2 // 2
    P, Q = PQ[..., :Co], PQ[..., Co:]
    y = P[np.arange(B)[:, None, None], idx] + Q[:, :, None, :]
    assert y.dtype == np.float32
    return y


def in_degree(idx, N):
    """``[B,N]``: the number of edges that end in every point."""
    idx = np.asarray(idx)
    return np.stack([np.bincount(idx[b].ravel(), minlength=N) for b in range(idx.shape[0])])


def forward_exact(PQ, idx, sgn):
    """The selection and the sums of ``fpsg_edgeconv_fwd``.  ``sgn [Co]``: the minimum is taken where ``sgn < 0`` (so
    ``-0.0`` counts as non-negative), the maximum elsewhere; the lowest slot that attains it wins."""
    y = edge_values(PQ, idx)
    B, N, k, Co = y.shape
    sg = np.where(np.asarray(sgn, dtype=np.float32) < 0, np.float32(-1), np.float32(1))
    jsel = (y * sg).argmax(axis=2)                                   # first occurrence = lowest slot
    ysel = np.take_along_axis(y, jsel[:, :, None, :], axis=2)[:, :, 0, :]
    s1 = np.empty((B, N, Co))
    abs_s1 = np.empty((B, N, Co))
    sum_y, sum_y2, sum_abs = np.zeros(Co), np.zeros(Co), np.zeros(Co)
    for b in range(B):
        yb = y[b].astype(np.float64)
        s1[b] = yb.sum(axis=1)
        abs_s1[b] = np.abs(yb).sum(axis=1)
        sum_y += s1[b].sum(axis=0)
        sum_abs += abs_s1[b].sum(axis=0)
        sum_y2 += (yb * yb).sum(axis=(0, 1))
    return SimpleNamespace(ysel=ysel, jsel=jsel.astype(np.uint8), s1=s1, abs_s1=abs_s1, sum_y=sum_y, sum_y2=sum_y2,
                           sum_abs=sum_abs)


def backward_per_edge(dzs, jsel, PQ, idx, coef):
    """``fpsg_edgeconv_bwd`` from the per-edge definition, float64:

        dY[b,n,j,c] = [jsel[b,n,c] == j] dzs[b,n,c] - A_c - Bc_c (y[b,n,j,c] - mu_c)      coef = (A, Bc, mu)
        dP[b,m] = sum of dY over the edges (n,j) with idx[b,n,j] = m,     dQ[b,n] = sum_j dY[b,n,j]

    ``coef = 0`` is the eval-mode backward.  Returns ``dPQ [B,N,2Co]`` and, next to every element, ``T``: the sum of the
    absolute values of the terms that went into it.  A term of ``Bc (y - mu)`` counts as ``|Bc| (|P| + |Q| + |mu|)``:
    ``y`` is ``P + Q``, and an implementation may sum the shares of ``P``, ``Q`` and ``mu`` separately."""
    PQ = np.asarray(PQ, dtype=np.float32)
    idx = np.asarray(idx)
    y = edge_values(PQ, idx)
    B, N, k, Co = y.shape
    A, Bc, mu = (np.asarray(coef, dtype=np.float64)[i] for i in range(3))
    dzs = np.asarray(dzs, dtype=np.float64)
    jsel = np.asarray(jsel).astype(np.int64)
    dPQ = np.zeros((B, N, 2 * Co))
    T = np.zeros((B, N, 2 * Co))
    slots = np.arange(k)[None, :, None]
    for b in range(B):
        Pb, Qb = np.abs(PQ[b, :, :Co].astype(np.float64)), np.abs(PQ[b, :, Co:].astype(np.float64))
        picked = np.where(jsel[b][:, None, :] == slots, dzs[b][:, None, :], 0.0)          # [N,k,Co]
        dY = picked - A - Bc * (y[b].astype(np.float64) - mu)
        aY = np.abs(picked) + np.abs(A) + np.abs(Bc) * (Pb[idx[b]] + Qb[:, None, :] + np.abs(mu))
        dPQ[b, :, Co:] = dY.sum(axis=1)
        T[b, :, Co:] = aY.sum(axis=1)
        dst = idx[b].ravel()
        np.add.at(dPQ[b, :, :Co], dst, dY.reshape(N * k, Co))
        np.add.at(T[b, :, :Co], dst, aY.reshape(N * k, Co))
    return dPQ, T


def layer64(PQ, idx, gamma, beta, running_mean, running_var, training, momentum, eps, slope, w_out):
    """``_EdgeConvBNMax`` in float64 with torch autograd: batch statistics (eval mode: the running ones) of the fp32-added
    ``y``, biased variance for the normalisation and unbiased for the running update, the selection of ``forward_exact``
    (``gather`` on its ``jsel``: the kernels' by construction), ``LeakyReLU``, and the gradients of ``sum(out * w_out)``.

    ``kink_min``: the smallest ``|z| / (|ysel scale| + |shift|)`` over the selected activations.  ``gap_min``: the
    smallest fp32 gap between the best and the second-best candidate (``inf`` at k = 1); ``inexact_ties``: how many
    (point, channel) pairs tie in fp32 without the exact sums ``P + Q`` being equal."""
    PQ = np.ascontiguousarray(PQ, dtype=np.float32)
    idx = np.asarray(idx).astype(np.int64)
    B, N, Co2 = PQ.shape
    Co, k = Co2 // 2, idx.shape[2]
    f64 = lambda a: torch.from_numpy(np.array(a, dtype=np.float64))
    gam, bet = f64(gamma).requires_grad_(), f64(beta).requires_grad_()
    rm, rv = f64(running_mean), f64(running_var)
    PQt = f64(PQ).requires_grad_()
    it = torch.from_numpy(idx)
    y_exact = PQt[..., :Co][torch.arange(B)[:, None, None], it] + PQt[:, :, None, Co:]
    y32 = edge_values(PQ, idx)
    y = y_exact + (f64(y32) - y_exact).detach()                      # the fp32 sum as the value, d/dPQ of P + Q
    fwd = forward_exact(PQ, idx, np.asarray(gamma, dtype=np.float32))
    count = B * N * k
    if training:
        mean = y.mean(dim=(0, 1, 2))
        var = (y - mean).square().mean(dim=(0, 1, 2))
        new_rm = (1.0 - momentum) * rm + momentum * mean.detach()
        new_rv = (1.0 - momentum) * rv + momentum * var.detach() * (count / max(count - 1, 1))
    else:
        mean, var, new_rm, new_rv = rm, rv, rm.clone(), rv.clone()
    rstd = 1.0 / torch.sqrt(var + eps)
    scale = gam * rstd
    shift = bet - mean * scale
    js = torch.from_numpy(fwd.jsel.astype(np.int64))
    ysel = y.gather(2, js[:, :, None, :])[:, :, 0, :]
    z = ysel * scale + shift
    out = torch.where(z > 0, z, z * slope)
    dPQ, dgamma, dbeta = torch.autograd.grad((out * f64(w_out)).sum(), [PQt, gam, bet])
    with torch.no_grad():
        kink = float((z.abs() / ((ysel * scale).abs() + shift.abs())).min())
        gap, inexact = float("inf"), 0
        if k > 1:
            sg = np.where(np.asarray(gamma, dtype=np.float32) < 0, np.float32(-1), np.float32(1))
            top = np.sort(y32 * sg, axis=2)[:, :, -2:, :]
            gap = float((top[:, :, 1] - top[:, :, 0]).min())
            tied = torch.from_numpy(y32 == fwd.ysel[:, :, None, :])
            ysel_exact = y_exact.gather(2, js[:, :, None, :])
            inexact = int((tied & (y_exact != ysel_exact)).any(dim=2).sum())
        abs_y = fwd.sum_abs / count
    n = lambda t: t.detach().numpy()
    return SimpleNamespace(out=n(out), running_mean=n(new_rm), running_var=n(new_rv), dPQ=n(dPQ), dgamma=n(dgamma),
                           dbeta=n(dbeta), kink_min=kink, gap_min=gap, inexact_ties=inexact,
                           mean=n(mean), var=n(var), rstd=n(rstd), scale=n(scale), shift=n(shift), z=n(z), ysel=n(ysel),
                           jsel=fwd.jsel, mean_abs_y=abs_y, mean_y2=fwd.sum_y2 / count, count=count)


# ---- inputs shared by the CPU and the GPU tests ---------------------------------------------------------------------

MOMENTUM = float(np.float32(0.1))        # the kernels take these three as fp32 arguments
BN_EPS = float(np.float32(1e-5))
SLOPE = float(np.float32(0.2))

# (B, N, k, Co, offset): seed.  offset = the largest |mean| / std of a channel's edge activations.  The seeds were
# picked on the CPU so that the float64 reference stays 1e-4 away from the LeakyReLU kink in training and in eval mode
# (tests/test_edgeconv_cpu.py asserts it); the case at offset 12 asserts no kink distance.
LAYER_SEEDS = {(2, 48, 20, 64, 0.0): 4, (2, 40, 20, 128, 0.0): 3, (2, 24, 20, 256, 0.0): 2, (9, 13, 5, 64, 0.0): 14,
               (2, 48, 20, 64, 3.0): 2, (2, 40, 20, 128, 3.0): 8, (2, 24, 20, 256, 3.0): 26,
               (2, 48, 20, 64, 12.0): 2, (2, 40, 20, 128, 12.0): 8, (2, 24, 20, 256, 12.0): 26}
LAYER_CASES = [key for key in LAYER_SEEDS if key[4] <= 3.0]          # these meet the kink precondition
OFFSET12_CASES = [key for key in LAYER_SEEDS if key[4] == 12.0]


def layer_case(B, N, k, Co, offset=0.0, seed=None):
    """Inputs of one ``_EdgeConvBNMax`` call: generic ``PQ``, random neighbour lists (repeats allowed), gammas of both
    signs and none 0, running statistics near the batch's but not equal to them.  ``offset > 0`` adds per-channel
    constants to ``Q`` so that |mean| / std of the channels' edge activations is spread over [0, offset]."""
    if seed is None:
        seed = LAYER_SEEDS[(B, N, k, Co, offset)]
    rng = np.random.default_rng(seed)
    PQ = rng.standard_normal((B, N, 2 * Co)).astype(np.float32)
    idx = rng.integers(0, N, size=(B, N, k)).astype(np.int32)
    gamma = (0.7 * rng.standard_normal(Co)).astype(np.float32)
    gamma[gamma == 0] = np.float32(0.5)
    beta = (0.3 * rng.standard_normal(Co)).astype(np.float32)
    w_out = rng.standard_normal((B, N, Co)).astype(np.float32)
    y = edge_values(PQ, idx).astype(np.float64)
    mean, std = y.mean(axis=(0, 1, 2)), y.std(axis=(0, 1, 2))
    if offset > 0:
        ratio = 0.999 * rng.permutation(np.linspace(-offset, offset, Co))        # fp32 rounding of Q must not lift it past offset
        PQ[:, :, Co:] = (PQ[:, :, Co:].astype(np.float64) + (ratio * std - mean)).astype(np.float32)
        y = edge_values(PQ, idx).astype(np.float64)
        mean, std = y.mean(axis=(0, 1, 2)), y.std(axis=(0, 1, 2))
    running_mean = (mean + 0.2 * rng.standard_normal(Co)).astype(np.float32)
    running_var = (std * std * (0.5 + rng.random(Co))).astype(np.float32)
    return SimpleNamespace(PQ=PQ, idx=idx, gamma=gamma, beta=beta, running_mean=running_mean, running_var=running_var,
                           w_out=w_out, ratio=np.abs(mean) / std, B=B, N=N, k=k, Co=Co, offset=offset)


def layer_ref(case, training):
    return layer64(case.PQ, case.idx, case.gamma, case.beta, case.running_mean, case.running_var, training, MOMENTUM,
                   BN_EPS, SLOPE, case.w_out)
