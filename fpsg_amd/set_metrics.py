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

The seventh column of the usual table, the Jensen-Shannon divergence between the voxel-occupancy distributions of the
two sets (``jsd``, K15 ``metrics.occupancy_grid``; ``evaluate_Network.py --jsd``), looks at where in space the sets put
their points rather than at cloud-to-cloud distances: ``jsd_from_counts`` and ``occupancy_entropy_from_counts`` work on
histograms already computed (pure torch float64, any device).  The published implementations are not pinned; the
definition in DESIGN.md (K15) is the specification.
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


def retained_nodes(resolution: int, in_sphere: bool = True) -> torch.Tensor:
    """bool ``[r,r,r]``: the grid nodes that are cells of the occupancy grid.  With ``in_sphere``, node ``(i,j,k)`` is
    retained iff ``(2i-(r-1))^2 + (2j-(r-1))^2 + (2k-(r-1))^2 <= (r-1)^2`` (integers: nodes exactly on the sphere
    inscribed in the grid are kept); without, every node."""
    r = int(resolution)
    if r < 2 or (in_sphere and r < 3):
        raise ValueError(f"resolution must be at least {3 if in_sphere else 2}, got {resolution}")
    if not in_sphere:
        return torch.ones((r, r, r), dtype=torch.bool)
    a = (2 * torch.arange(r, dtype=torch.int64) - (r - 1)) ** 2
    return a[:, None, None] + a[None, :, None] + a[None, None, :] <= (r - 1) ** 2


def _entropy_bits(p: torch.Tensor) -> torch.Tensor:
    p = p[p > 0]                                                   # 0 log 0 = 0
    return -(p * torch.log2(p)).sum()


def jsd_from_counts(counts_g: torch.Tensor, counts_r: torch.Tensor) -> float:
    """Jensen-Shannon divergence in bits between the distributions ``P = counts_g / sum`` and ``Q = counts_r / sum``:
    ``H((P + Q) / 2) - (H(P) + H(Q)) / 2`` in float64.  In [0, 1]; symmetric; 0.0 exactly for proportional histograms
    whose quotients round alike (equal ones always); 1 for disjoint supports.  ``ValueError`` for mismatched shapes
    or an all-zero histogram."""
    if tuple(counts_g.shape) != tuple(counts_r.shape):
        raise ValueError(f"histograms of different shapes: {tuple(counts_g.shape)} and {tuple(counts_r.shape)}")
    g, r = counts_g.reshape(-1).double(), counts_r.reshape(-1).double()
    sg, sr = g.sum(), r.sum()
    if not (float(sg) > 0 and float(sr) > 0):
        raise ValueError("a histogram without any point has no distribution")
    P, Q = g / sg, r / sr
    M = (P + Q) / 2
    v = float(_entropy_bits(M) - (_entropy_bits(P) + _entropy_bits(Q)) / 2)      # P = Q: M = P, the same three sums
    return min(max(v, 0.0), 1.0)                                   # rounding may leave the interval by an ulp or two


def occupancy_entropy_from_counts(clouds_hit: torch.Tensor, n_clouds: int, retained: torch.Tensor) -> float:
    """Mean over the retained nodes of the binary entropy in bits of ``clouds_hit / n_clouds``, the share of the set's
    clouds with a point in the node (float64)."""
    if tuple(clouds_hit.shape) != tuple(retained.shape):
        raise ValueError(f"clouds_hit {tuple(clouds_hit.shape)} and retained {tuple(retained.shape)} differ in shape")
    if int(n_clouds) < 1:
        raise ValueError(f"n_clouds must be positive, got {n_clouds}")
    keep = retained.to(clouds_hit.device)
    n = int(keep.sum())
    if n < 1:
        raise ValueError("no retained node")
    p = clouds_hit[keep].double() / float(n_clouds)
    q = 1.0 - p
    h = -(torch.where(p > 0, p * torch.log2(p.clamp_min(1e-300)), torch.zeros_like(p))
          + torch.where(q > 0, q * torch.log2(q.clamp_min(1e-300)), torch.zeros_like(q)))
    return float(h.sum() / n)


def jsd(gen: torch.Tensor, ref: torch.Tensor, resolution: int = 28, half_extent: float = 1.0,
        in_sphere: bool = True) -> dict:
    """The Jensen-Shannon divergence between the occupancy distributions of generated clouds ``gen [G,N,3]`` and
    reference clouds ``ref [R,M,3]`` (fp32 on the GPU): two K15 launches (``metrics.occupancy_grid``), then
    ``jsd_from_counts``.  ``{"jsd", "entropy_gen", "entropy_ref"}`` as Python floats (the entropies:
    ``occupancy_entropy_from_counts`` of each set) and ``"outside_gen"``, ``"outside_ref"``, lists of three ints (the
    grids' ``outside``).  ``half_extent`` 1.0 suits clouds in the unit ball, 0.5 the unit cube."""
    from .metrics import occupancy_grid
    g = occupancy_grid(gen, resolution, half_extent, in_sphere)
    r = occupancy_grid(ref, resolution, half_extent, in_sphere)
    return jsd_from_grids(g, r)


def jsd_from_grids(g: dict, r: dict) -> dict:
    """``jsd``'s result from two grids of ``metrics.occupancy_grid`` made with the same parameters (e.g. accumulated
    with ``out=`` while the clouds arrive)."""
    for k in ("resolution", "half_extent", "in_sphere"):
        if g[k] != r[k]:
            raise ValueError(f"the two grids differ in {k}: {g[k]!r} and {r[k]!r}")
    keep = retained_nodes(g["resolution"], g["in_sphere"])
    return {"jsd": jsd_from_counts(g["counts"], r["counts"]),
            "entropy_gen": occupancy_entropy_from_counts(g["clouds_hit"], g["n_clouds"], keep),
            "entropy_ref": occupancy_entropy_from_counts(r["clouds_hit"], r["n_clouds"], keep),
            "outside_gen": g["outside"].tolist(), "outside_ref": r["outside"].tolist()}
