"""Float64 restatement of K25 (PU-GAN's uniform loss, ``include/fpsg_hip.h``) in plain torch: the ball lists and the
nearest neighbours inside the balls by full distance tables and stable sorts (no cap shortcuts), the value on given
lists, and its gradient by autograd on given lists.  ``dtype`` lets the same expressions run in fp32.  Runs on whatever
device its input is on; the kernels are checked against it, never the other way."""
import math

import torch

HEX = 2.0 * math.pi / math.sqrt(3.0)                                 # the hexagonal-packing constant of dhat


def radii(percentages, radius, dtype=torch.float64, device=None):
    """``(p [T], r2 [T])``: the percentages as the C entry takes them (an fp32 array) and ``r2_t = fp32(p_t R R)``, the
    product formed in double; both exact in ``dtype``."""
    p = torch.tensor(list(percentages), dtype=torch.float32).double()
    r2 = (p * float(radius) * float(radius)).float()
    return p.to(dtype=dtype, device=device), r2.to(dtype=dtype, device=device)


def ball_counts(x, seeds, percentages, radius):
    """``count [B,T,S]`` alone, in float64 (one distance table per cloud)."""
    x = x.detach().double()
    N = x.size(1)
    seeds = seeds.long()
    _, r2 = radii(percentages, radius, device=x.device)
    sx = x.gather(1, seeds.clamp(0, N - 1)[:, :, None].expand(-1, -1, 3))
    D = (x[:, None, :, :] - sx[:, :, None, :]).pow(2).sum(-1)        # [B,S,N]
    inside = (D[:, None] <= r2[None, :, None, None]) & ((seeds >= 0) & (seeds < N))[:, None, :, None]
    return inside.sum(-1)


def ball_lists(x, seeds, percentages, radius, cap):
    """``(count [B,T,S], member, nn [B,T,S,cap] int64, nn_d2 [B,T,S,cap] float64)`` in float64: ball ``(j, t)`` is every
    ``i`` with ``|x_i - x_seed_j|^2 <= r2_t`` in ascending index, ``count`` its full size, ``member`` its first ``cap``
    entries (-1 behind them); ``nn`` the retained member nearest to each retained member, itself excluded by slot, ties to
    the lowest index (a stable sort over the ascending list), ``nn_d2`` that squared distance; -1 and +inf behind the list
    and in a ball of one.  A seed outside ``[0, N)`` owns an empty ball."""
    x = x.detach().double()
    B, N, _ = x.shape
    S = seeds.size(1)
    _, r2 = radii(percentages, radius, device=x.device)
    T = r2.numel()
    count = torch.zeros((B, T, S), dtype=torch.int64, device=x.device)
    member = torch.full((B, T, S, cap), -1, dtype=torch.int64, device=x.device)
    nn = torch.full((B, T, S, cap), -1, dtype=torch.int64, device=x.device)
    nn_d2 = torch.full((B, T, S, cap), float("inf"), dtype=torch.float64, device=x.device)
    every = torch.arange(N, device=x.device)
    for b in range(B):
        for j in range(S):
            s = int(seeds[b, j])
            if not 0 <= s < N:
                continue
            d = (x[b] - x[b, s]).pow(2).sum(-1)                      # [N], direct differences
            for t in range(T):
                inside = every[d <= r2[t]]                           # ascending
                count[b, t, j] = inside.numel()
                kept = inside[:cap]
                m = kept.numel()
                member[b, t, j, :m] = kept
                if m < 2:
                    continue
                y = x[b, kept]
                D = (y[:, None, :] - y[None, :, :]).pow(2).sum(-1)
                D.fill_diagonal_(float("inf"))
                val, order = torch.sort(D, dim=1, stable=True)
                nn[b, t, j, :m] = kept[order[:, 0]]
                nn_d2[b, t, j, :m] = val[:, 0]
    return count, member, nn, nn_d2


def value(x, seeds, count, member, nn, percentages, radius, dtype=torch.float64):
    """``(value [B], per_percent [B,T], ball_value [B,T,S])`` in ``dtype`` on the given lists (differentiable in ``x``):
    ``U = ((c - N p)^2 / (N p)) sum_i term_i`` over the retained members, ``term = (d - dhat)^2 / dhat`` with ``d`` the
    distance to ``nn`` and ``dhat = sqrt((2 pi / sqrt 3) r2 / c)``; a member at distance 0 from its ``nn`` contributes the
    constant ``dhat``; a ball with fewer than two retained members or a seed outside the cloud is 0."""
    x = x.to(dtype)
    B, N, _ = x.shape
    T, S, cap = member.shape[1], member.shape[2], member.shape[3]
    p, r2 = radii(percentages, radius, dtype, x.device)
    member, nn, count = member.long(), nn.long(), count.long()
    kept = (member >= 0) & (member < N) & (nn >= 0) & (nn < N)
    flat = lambda idx: x.gather(1, idx.clamp(0, N - 1).reshape(B, -1, 1).expand(-1, -1, 3)).reshape(B, T, S, cap, 3)
    e = (flat(member) - flat(nn)).pow(2).sum(-1)
    c = count.clamp_min(1).to(dtype)
    dhat = torch.sqrt(HEX * r2[None, :, None] / c)[..., None]        # [B,T,S,1]
    apart = kept & (e > 0)
    d = torch.sqrt(torch.where(apart, e, torch.ones_like(e)))
    term = torch.where(apart, (d - dhat).pow(2) / dhat, dhat.expand_as(d))
    term = torch.where(kept, term, torch.zeros_like(term))
    nhat = (N * p)[None, :, None]
    weight = (count.to(dtype) - nhat).pow(2) / nhat
    m = (member >= 0).sum(-1)
    ok = (m >= 2) & ((seeds.long() >= 0) & (seeds.long() < N))[:, None, :]
    U = torch.where(ok, weight * term.sum(-1), torch.zeros_like(weight))
    return U.sum((1, 2)) / (T * S), U.sum(2) / S, U


def value_and_grad(x, seeds, count, member, nn, percentages, radius, upstream=None, dtype=torch.float64):
    """``(value [B], per_percent, ball_value, d value / d x [B,N,3])`` in ``dtype`` by autograd with the lists held fixed;
    ``upstream [B]`` weights the clouds (default: ones)."""
    xx = x.detach().to(dtype).requires_grad_()
    v, per, U = value(xx, seeds, count, member, nn, percentages, radius, dtype)
    up = torch.ones_like(v) if upstream is None else upstream.to(dtype)
    (g,) = torch.autograd.grad((v * up).sum(), [xx])
    return v.detach(), per.detach(), U.detach(), g
