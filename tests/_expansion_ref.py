"""Float64 checker of the expansion penalty (K24), vectorised over patches: Prim's with the kernel's tie
rules, the value and its gradient by autograd on a GIVEN tree / mask, the closed-form gradient, a validity and a
minimality check of a parent array, and the clouds the value tests run on (shared by the CPU and the GPU file: the
CPU file checks, on the reference alone, that no edge of theirs sits at the penalty threshold)."""
import numpy as np
import torch

VALUE_P = (64, 128, 256, 512, 1024)                                   # 1, 2, 4, 8 and 16 vertices per lane
VALUE_LAMBDAS = (1.0, 1.5, 2.0)
# one seed per patch size, searched until `threshold_margin` (below) holds at all three lambdas for all four clouds
VALUE_SEEDS = {64: 11, 128: 28, 256: 1, 512: 27, 1024: 6}
MARGIN = 1e-4


def value_patches(P):
    """Patches per cloud of the value tests: 16 up to ``P = 128``, 4 up to 512, 2 at 1024 (the float64 side stays at
    seconds)."""
    return 16 if P <= 128 else 4 if P <= 512 else 2


def patches(x, P):
    """``x [B,N,3]`` -> float64 ``[B * K, P, 3]``."""
    B, N, _ = x.shape
    assert N % P == 0
    return x.double().reshape(B * (N // P), P, 3)


def prim(x, P):
    """Prim's tree of every patch from its vertex 0 in float64: a non-tree vertex keeps the smallest d2 to a tree vertex
    and that vertex as parent, replaced only by a STRICTLY smaller one (the earlier-added vertex wins ties); each step adds
    the non-tree vertex with the smallest (key, index).  Returns ``parent`` (long, -1 at vertex 0), ``d2`` (float64, 0 at
    vertex 0), ``order`` (long), all ``[B,N]``."""
    B, N, _ = x.shape
    y = patches(x, P)
    G = y.shape[0]
    dx, dy, dz = (y[:, :, None, c] - y[:, None, :, c] for c in range(3))
    D = dz * dz + (dy * dy + dx * dx)                                 # [G,P,P]
    rows = torch.arange(G, device=x.device)
    cols = torch.arange(P, device=x.device)
    key = D[:, 0, :].clone()
    par = torch.zeros((G, P), dtype=torch.long, device=x.device)
    order = torch.zeros((G, P), dtype=torch.long, device=x.device)
    intree = torch.zeros((G, P), dtype=torch.bool, device=x.device)
    intree[:, 0] = True
    for step in range(1, P):
        k = key.masked_fill(intree, float("inf"))
        m = k.min(dim=1, keepdim=True).values
        u = torch.where((k == m) & ~intree, cols[None, :], P).min(dim=1).values      # the lowest index at the minimum
        intree[rows, u] = True
        order[rows, u] = step
        du = D[rows, u]
        lower = ~intree & (du < key)
        key = torch.where(lower, du, key)
        par = torch.where(lower, u[:, None], par)
    par[:, 0] = -1
    key[:, 0] = 0.0
    return par.reshape(B, N), key.reshape(B, N), order.reshape(B, N)


def edge_lengths(x, P, parent):
    """``r [B*K, P]`` float64 of the tree ``parent [B,N]`` (0 at the root); differentiable in ``x``."""
    y = patches(x, P)
    par = parent.reshape(-1, P).long()
    root = par < 0
    other = torch.gather(y, 1, par.clamp_min(0)[:, :, None].expand(-1, -1, 3))
    d2 = ((y - other) ** 2).sum(-1)
    # sqrt(0) has no derivative: the root's and a zero edge's length are constants
    return torch.where(root | (d2 == 0), torch.zeros_like(d2), d2.clamp_min(1e-300).sqrt())


def mean_len(x, P, parent):
    """``l_q [B, K]`` float64."""
    return (edge_lengths(x, P, parent).sum(1) / (P - 1)).reshape(x.shape[0], -1)


def penalised(x, P, parent, lam):
    """The mask ``[B,N]``: ``r_v > lam * l_q``, strictly, in float64."""
    r = edge_lengths(x, P, parent)
    l = r.sum(1, keepdim=True) / (P - 1)
    return (r > lam * l).reshape(x.shape[0], -1)


def value_and_grad(x, P, parent, mask, up=None):
    """``E [B]`` float64 on the given tree and mask, and the gradient of ``sum_b up[b] E[b]`` by autograd."""
    B, N, _ = x.shape
    K = N // P
    xx = x.double().clone().requires_grad_()
    r = edge_lengths(xx, P, parent)
    E = (torch.where(mask.reshape(-1, P), r, torch.zeros_like(r)).sum(1) / (P - 1)).reshape(B, K).sum(1) / K
    w = torch.ones_like(E) if up is None else up.double()
    (g,) = torch.autograd.grad((E * w).sum(), [xx], allow_unused=True)
    return E.detach(), (torch.zeros_like(xx) if g is None else g)


def closed_form_grad(x, P, parent, mask):
    """dE/dx_u = (1 / (K (P - 1))) [ [u penalised] (x_u - x_par(u)) / r_u + sum_{v: par(v) = u, v penalised} (x_u - x_v) / r_v ],
    written out term by term."""
    B, N, _ = x.shape
    K = N // P
    xx = x.double()
    g = torch.zeros_like(xx)
    for b in range(B):
        for v in range(N):
            if not bool(mask[b, v]):
                continue
            q = v // P
            u = q * P + int(parent[b, v])
            d = xx[b, v] - xx[b, u]
            r = d.norm()
            g[b, v] += d / r
            g[b, u] -= d / r
    return g / (K * (P - 1))


def check_tree(parent, order, P):
    """``parent [B,N]`` is a spanning tree of every patch: P - 1 edges (the root alone has -1, every other parent is a
    local index), ``order`` a permutation of 0..P-1 per patch with the root first, and every parent added before its
    child -- so every vertex reaches the root."""
    par = parent.reshape(-1, P).long()
    od = order.reshape(-1, P).long()
    assert bool((par[:, 0] == -1).all()), "the root's parent is -1"
    assert bool(((par[:, 1:] >= 0) & (par[:, 1:] < P)).all()), "P - 1 edges, every index inside [0, P)"
    assert bool((od.sort(dim=1).values == torch.arange(P, device=od.device)[None, :]).all()), "order is a permutation"
    assert bool((od[:, 0] == 0).all())
    assert bool((torch.gather(od, 1, par[:, 1:]) < od[:, 1:]).all()), "a parent is added before its child"


def check_minimal(x, P, parent, rel=1e-5):
    """The sorted edge lengths equal, entry by entry, those of scipy's minimum spanning tree of the float64 distance
    matrix (all minimum spanning trees of a graph share one multiset of edge weights: independent of the tie rules).
    Needs distinct points: scipy reads a zero entry as a missing edge."""
    from scipy.sparse.csgraph import minimum_spanning_tree
    y = patches(x, P).cpu()
    r = edge_lengths(x, P, parent).cpu()
    worst = 0.0
    for q in range(y.shape[0]):
        D = np.sqrt(((y[q][:, None, :] - y[q][None, :, :]) ** 2).sum(-1).numpy())
        want = np.sort(minimum_spanning_tree(D).data)
        got = np.sort(r[q, 1:].numpy())
        assert want.shape == got.shape == (P - 1,), (q, want.shape)
        dev = float(np.max(np.abs(got - want) / want))
        worst = max(worst, dev)
        assert dev <= rel, (q, dev)
    return worst


def threshold_margin(x, P, parent, lam):
    """The smallest ``|r_v - lam l_q| / (lam l_q)`` over every edge of every patch."""
    r = edge_lengths(x, P, parent)
    t = lam * r.sum(1, keepdim=True) / (P - 1)
    return float(((r[:, 1:] - t).abs() / t).min())


def value_clouds(P):
    """The four clouds ``[4, N, 3]`` fp32 (CPU) of the value tests at patch size ``P``, ``N = value_patches(P) P``: two
    unit-ball clouds, one ``tanh(randn)`` cloud (the decoder's range), and one "sheet" cloud whose patches are smooth maps of a random 2-D sample scaled to 0.2 with ONE point moved 1.0 away -- every patch has a penalised edge."""
    from conftest import unit_ball_clouds
    seed = VALUE_SEEDS[P]
    K = value_patches(P)
    N = K * P
    g = torch.Generator().manual_seed(1000 * P + seed)
    ball = torch.from_numpy(unit_ball_clouds(np.random.default_rng(1000 * P + seed), 2, N)).float()
    tanh = torch.tanh(torch.randn((1, N, 3), generator=g))
    uv = torch.rand((K, P, 2), generator=g) * 0.2
    centre = (torch.rand((K, 1, 3), generator=g) - 0.5) * 0.8
    u, v = uv[..., 0], uv[..., 1]
    sheet = torch.stack([u, v, 0.05 * torch.sin(15 * u) * torch.cos(10 * v)], dim=-1) + centre
    at = torch.randint(0, P, (K,), generator=g)
    away = torch.randn((K, 3), generator=g)
    away = away / away.norm(dim=1, keepdim=True)
    sheet[torch.arange(K), at] += away
    return torch.cat([ball, tanh, sheet.reshape(1, N, 3)]).float().contiguous()
