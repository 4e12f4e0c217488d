"""Float64 restatement of K21 (the repulsion regulariser, ``include/fpsg_hip.h``) in plain torch: the neighbour lists by a
full stable sort on ``(d2, j)`` with ``d2`` in the direct-difference form, and the value with its gradient by autograd
given the lists.  Runs on whatever device its input is on; the kernels are checked against it, never the other way."""
import torch

FLOOR_D2 = 1e-12


def neighbour_lists(x: torch.Tensor, k: int, rows: int = 1024):
    """``(idx [B,N,k] int64, d2 [B,N,k] float64)``: for every point the ``k`` indices ``j != i`` with the smallest
    ``(d2(i,j), j)``, nearest first, ties to the lower index (a stable sort over ascending ``j``).  ``i`` is excluded by
    index, so a duplicate of ``i`` is a neighbour at distance 0.  Works in blocks of ``rows`` query points."""
    x = x.detach().double()
    B, N, _ = x.shape
    idx = torch.empty((B, N, k), dtype=torch.int64, device=x.device)
    d2 = torch.empty((B, N, k), dtype=torch.float64, device=x.device)
    for b in range(B):
        for i0 in range(0, N, rows):
            q = x[b, i0:i0 + rows]
            d = (x[b][None, :, :] - q[:, None, :]).pow(2).sum(-1)          # [rows, N], direct differences
            own = torch.arange(i0, i0 + q.size(0), device=x.device)
            d[torch.arange(q.size(0), device=x.device), own] = float("inf")
            val, order = torch.sort(d, dim=1, stable=True)
            idx[b, i0:i0 + rows] = order[:, :k]
            d2[b, i0:i0 + rows] = val[:, :k]
    return idx, d2


def pair_d2(x: torch.Tensor, idx: torch.Tensor) -> torch.Tensor:
    """``d2[b,i,s] = |x[b,i] - x[b,idx[b,i,s]]|^2`` (differentiable in ``x``)."""
    B, N, k = idx.shape
    nb = x.gather(1, idx.reshape(B, N * k, 1).expand(-1, -1, 3)).reshape(B, N, k, 3)
    return (x[:, :, None, :] - nb).pow(2).sum(-1)


def value(x: torch.Tensor, idx: torch.Tensor, h: float) -> torch.Tensor:
    """``R [B]`` in the dtype of ``x`` given the lists; where ``d2 <= 1e-12`` the pair term is the constant ``-1e-6 *
    exp(-d2 / h^2)`` with no dependence on ``x`` (the derivative there is defined as 0)."""
    d2 = pair_d2(x, idx.long())
    floor = d2 <= FLOOR_D2
    d2 = torch.where(floor, d2.detach(), d2)
    r = torch.sqrt(torch.clamp(d2, min=FLOOR_D2))
    rho = -r * torch.exp(-d2 / (h * h))
    return rho.sum((1, 2)) / (idx.size(1) * idx.size(2))


def value_and_grad(x: torch.Tensor, idx: torch.Tensor, h: float, upstream=None):
    """``(R [B], dR/dx [B,N,3])`` in float64 by autograd; ``upstream [B]`` weights the clouds (default: ones)."""
    x64 = x.detach().double().requires_grad_()
    R = value(x64, idx, h)
    up = torch.ones_like(R) if upstream is None else upstream.double()
    (g,) = torch.autograd.grad((R * up).sum(), [x64])
    return R.detach(), g


def closed_form_grad(x: torch.Tensor, idx: torch.Tensor, h: float) -> torch.Tensor:
    """The gradient as the issue writes it, term by term in float64 (loops; small clouds only):
    ``(2 / (N k)) [ sum_{m in K(j)} rho'(d2(j,m)) (x_j - x_m) - sum_{i: j in K(i)} rho'(d2(i,j)) (x_i - x_j) ]``."""
    x = x.detach().double()
    B, N, k = idx.shape
    g = torch.zeros_like(x)

    def slope(d2):
        if d2 <= FLOOR_D2:
            return 0.0
        r = d2 ** 0.5
        return -float(torch.exp(torch.tensor(-d2 / (h * h), dtype=torch.float64))) * (1.0 / (2.0 * r) - r / (h * h))

    for b in range(B):
        for i in range(N):
            for s in range(k):
                m = int(idx[b, i, s])
                diff = x[b, i] - x[b, m]
                w = slope(float((diff * diff).sum()))
                g[b, i] += w * diff                                        # i's own term
                g[b, m] -= w * diff                                        # the reverse term on its neighbour
    return g * (2.0 / (N * k))
