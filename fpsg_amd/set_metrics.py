"""Set-level generation metrics under the Chamfer distance (Achlioptas et al. 2018; Yang et al., PointFlow, 2019):
minimum matching distance (MMD), coverage (COV) and 1-nearest-neighbour accuracy (1-NNA) between a set G of generated
clouds and a set R of reference clouds.

``from_matrices`` works on Chamfer matrices already computed (pure torch, any device); ``generation_metrics`` builds
them with K13 (``metrics.chamfer_matrix``) on the GPU.  Definitions, with D the Chamfer matrix:

* ``mmd_cd = mean_{r in R} min_{g in G} D[g,r]``;
* ``cov_cd = |{argmin_r D[g,r] : g in G}| / |R|``, ties to the lowest r;
* ``nna_cd``: leave-one-out 1-NN classifier accuracy over ``G u R`` in the order ``[G..., R...]``: each cloud's nearest
  other cloud (self excluded, ties to the lowest index in that order) is correct when it comes from the same set;
  ``correct / (|G| + |R|)``, 0.5 is ideal (generated and reference clouds are indistinguishable).

The same three metrics under the exact EMD (``emd_generation_metrics``, K14 ``metrics.emd_matrix``) are
``from_matrices`` applied to the EMD matrices divided by N (the mean matched distance).  Each EMD entry comes with a
certificate ``cost - gap <= EMD <= cost``; ``certify_nearest`` says which nearest-neighbour decisions behind COV and
1-NNA the bounds settle.
"""
from __future__ import annotations

import torch


def _first_argmin_excluding_self(d: torch.Tensor) -> torch.Tensor:
    """For every row i of the square matrix d, the lowest column j != i at which the row's minimum over j != i is."""
    n = d.size(0)
    off = d[~torch.eye(n, dtype=torch.bool, device=d.device)].reshape(n, n - 1)   # row i without column i
    j = torch.argmin(off, dim=1)                                                  # first minimum
    return j + (j >= torch.arange(n, device=d.device)).long()


def from_matrices(d_gr: torch.Tensor, d_gg: torch.Tensor, d_rr: torch.Tensor) -> dict:
    """``{"mmd_cd", "cov_cd", "nna_cd"}`` as Python floats from ``d_gr [G,R]``, ``d_gg [G,G]`` and ``d_rr [R,R]``.
    Raises ``ValueError`` for an empty set or matrices of inconsistent shapes."""
    if d_gr.dim() != 2 or d_gg.dim() != 2 or d_rr.dim() != 2:
        raise ValueError("from_matrices expects three 2-D matrices")
    G, R = d_gr.shape
    if G < 1 or R < 1:
        raise ValueError(f"set metrics need at least one generated and one reference cloud (got {G} and {R})")
    if tuple(d_gg.shape) != (G, G) or tuple(d_rr.shape) != (R, R):
        raise ValueError(f"inconsistent shapes: d_gr {tuple(d_gr.shape)}, d_gg {tuple(d_gg.shape)}, "
                         f"d_rr {tuple(d_rr.shape)}")
    mmd = d_gr.min(dim=0).values.double().mean()
    cov = torch.unique(torch.argmin(d_gr, dim=1)).numel() / R
    full = torch.cat([torch.cat([d_gg, d_gr], dim=1), torch.cat([d_gr.t(), d_rr], dim=1)], dim=0)
    label = torch.arange(G + R, device=full.device) >= G
    nn = _first_argmin_excluding_self(full)
    nna = (label[nn] == label).sum().item() / (G + R)
    return {"mmd_cd": float(mmd), "cov_cd": float(cov), "nna_cd": float(nna)}


def generation_metrics(gen: torch.Tensor, ref: torch.Tensor) -> dict:
    """MMD, COV and 1-NNA under the Chamfer distance (``from_matrices``) between generated clouds ``gen [G,N,3]`` and
    reference clouds ``ref [R,M,3]`` (fp32 on the GPU, N, M <= 4096): three K13 launches, ``chamfer_matrix(gen, ref)``
    and the two within-set matrices in the symmetric mode.  Needs ``G >= 1``, ``R >= 1`` (so ``G + R >= 2``);
    raises ``ValueError`` otherwise."""
    from .metrics import chamfer_matrix
    if gen.dim() != 3 or ref.dim() != 3:
        raise ValueError(f"expected [G,N,3] and [R,M,3] clouds, got {tuple(gen.shape)} and {tuple(ref.shape)}")
    G, R = gen.size(0), ref.size(0)
    if G < 1 or R < 1 or G + R < 2:
        raise ValueError(f"set metrics need at least one generated and one reference cloud (got {G} and {R})")
    gen, ref = gen.contiguous(), ref.contiguous()
    return from_matrices(chamfer_matrix(gen, ref), chamfer_matrix(gen), chamfer_matrix(ref))


def certify_nearest(cost: torch.Tensor, gap: torch.Tensor, exclude_self: bool = False) -> torch.Tensor:
    """Per row of ``cost [n,m]`` (upper bounds) and ``gap [n,m]`` (``cost - gap`` the lower bounds): whether the row's
    nearest-neighbour decision -- the first argmin of ``cost`` (self excluded when ``exclude_self``, square matrices)
    -- is certified, i.e. its upper bound is strictly below every other candidate's lower bound, so no value within
    the bounds can change it.  Ties are uncertified.  A row with a single candidate is certified.  Bool ``[n]``."""
    if cost.dim() != 2 or tuple(gap.shape) != tuple(cost.shape):
        raise ValueError(f"certify_nearest expects two 2-D matrices of one shape, got {tuple(cost.shape)} and "
                         f"{tuple(gap.shape)}")
    n, m = cost.shape
    lower = cost - gap
    if exclude_self:
        if n != m:
            raise ValueError(f"exclude_self needs a square matrix, got {tuple(cost.shape)}")
        j = _first_argmin_excluding_self(cost)
    else:
        j = torch.argmin(cost, dim=1)
    rows = torch.arange(n, device=cost.device)
    chosen = cost[rows, j]
    others = torch.ones((n, m), dtype=torch.bool, device=cost.device)
    others[rows, j] = False
    if exclude_self:
        others[rows, rows] = False
    beaten = (chosen[:, None] < lower) | ~others                  # every other candidate's lower bound is above
    return beaten.all(dim=1)


def emd_from_matrices(c_gr, g_gr, c_gg, g_gg, c_rr, g_rr, n_points: int) -> dict:
    """The EMD set metrics from cost and gap matrices (pure torch, any device): ``mmd_emd``, ``cov_emd``, ``nna_emd``
    are ``from_matrices`` on the costs divided by ``n_points``; ``mmd_emd_lower`` the same MMD on ``(cost - gap) /
    n_points`` (``[mmd_emd_lower, mmd_emd]`` brackets the exact MMD); ``cov_uncertified`` and ``nna_uncertified`` the
    fractions of the nearest-neighbour decisions behind COV (one per generated cloud) and 1-NNA (one per cloud of
    ``G u R``) that the bounds do not certify (``certify_nearest``)."""
    n = float(n_points)
    m = from_matrices(c_gr / n, c_gg / n, c_rr / n)
    low = from_matrices((c_gr - g_gr) / n, c_gg / n, c_rr / n)
    G, R = c_gr.shape
    cov_ok = certify_nearest(c_gr, g_gr)
    full_c = torch.cat([torch.cat([c_gg, c_gr], dim=1), torch.cat([c_gr.t(), c_rr], dim=1)], dim=0)
    full_g = torch.cat([torch.cat([g_gg, g_gr], dim=1), torch.cat([g_gr.t(), g_rr], dim=1)], dim=0)
    nna_ok = certify_nearest(full_c, full_g, exclude_self=True)
    return {"mmd_emd": m["mmd_cd"], "cov_emd": m["cov_cd"], "nna_emd": m["nna_cd"], "mmd_emd_lower": low["mmd_cd"],
            "cov_uncertified": float((~cov_ok).sum().item()) / G,
            "nna_uncertified": float((~nna_ok).sum().item()) / (G + R)}


def emd_generation_metrics(gen: torch.Tensor, ref: torch.Tensor, eps: float | None = None,
                           max_rounds: int | None = None) -> dict:
    """MMD, COV and 1-NNA under the exact EMD between generated clouds ``gen [G,N,3]`` and reference clouds
    ``ref [R,N,3]`` (fp32 on the GPU, equal N <= 2048), with their certification (``emd_from_matrices``): three K14
    launches, ``emd_matrix(gen, ref)`` and the two within-set matrices in the symmetric mode, all with one ``eps``
    (default ``emd_exact_default_eps`` over both sets).  Needs ``G >= 1``, ``R >= 1``; raises ``ValueError``
    otherwise, for unequal N or N > 2048."""
    from .metrics import EMD_EXACT_MAX_N, emd_exact_default_eps, emd_matrix
    if gen.dim() != 3 or ref.dim() != 3 or gen.size(2) != 3 or ref.size(2) != 3:
        raise ValueError(f"expected [G,N,3] and [R,N,3] clouds, got {tuple(gen.shape)} and {tuple(ref.shape)}")
    G, R = gen.size(0), ref.size(0)
    if G < 1 or R < 1:
        raise ValueError(f"set metrics need at least one generated and one reference cloud (got {G} and {R})")
    if gen.size(1) != ref.size(1):
        raise ValueError(f"EMD set metrics need clouds of equal size, got N={gen.size(1)} and N={ref.size(1)}")
    if gen.size(1) < 1 or gen.size(1) > EMD_EXACT_MAX_N:
        raise ValueError(f"EMD set metrics support 1 to {EMD_EXACT_MAX_N} points per cloud, got {gen.size(1)}")
    gen, ref = gen.detach().contiguous(), ref.detach().contiguous()
    if eps is None:
        eps = emd_exact_default_eps(gen, ref)
    c_gr, i_gr = emd_matrix(gen, ref, eps=eps, max_rounds=max_rounds, return_info=True)
    c_gg, i_gg = emd_matrix(gen, eps=eps, max_rounds=max_rounds, return_info=True)
    c_rr, i_rr = emd_matrix(ref, eps=eps, max_rounds=max_rounds, return_info=True)
    return emd_from_matrices(c_gr, i_gr["gap"], c_gg, i_gg["gap"], c_rr, i_rr["gap"], gen.size(1))
