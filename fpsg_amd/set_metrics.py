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
