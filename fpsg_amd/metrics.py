"""Point-set distances on HIP kernels, behind the Python call sites the reference uses.

``chamfer_distance`` / ``sided_distance`` mirror ``kaolin.metrics.pointcloud`` (Kaolin
0.9.0) as bound at reference ``src/models/few_shot.py:13,57`` and called at
``src/models/few_shot.py:110,117,167``: same argument meaning, same ``[B]`` result, same
contiguity / dtype / device assertions.  There is no CPU path.
"""
from __future__ import annotations

import ctypes
import math
import numbers

import torch

from . import _hip

# Optional launch probe (bench.py): a callable ``probe(kind, B, N, M)`` returning a context
# manager that brackets the enqueue of one kernel on the current stream (HIP events).
_launch_probe = None


def set_launch_probe(probe) -> None:
    global _launch_probe
    _launch_probe = probe


class _NoProbe:
    def __enter__(self):
        return self

    def __exit__(self, *exc):
        return False


def _probe(kind, B, N, M):
    return _NoProbe() if _launch_probe is None else _launch_probe(kind, B, N, M)


def _tiled_enabled() -> bool:
    """``FPSG_CHAMFER_TILED=0`` selects the two-pass forward kernel (A/B measurements)."""
    import os
    return os.environ.get("FPSG_CHAMFER_TILED", "1") != "0"


def _check_clouds(p1: torch.Tensor, p2: torch.Tensor):
    if p1.dim() != 3 or p2.dim() != 3 or p1.size(2) != 3 or p2.size(2) != 3:
        raise ValueError(f"expected [B,N,3] and [B,M,3] clouds, got {tuple(p1.shape)} and "
                         f"{tuple(p2.shape)}")
    if p1.size(0) != p2.size(0):
        raise ValueError(f"batch mismatch: {p1.size(0)} vs {p2.size(0)}")
    if p1.device != p2.device:
        raise ValueError(f"device mismatch: {p1.device} vs {p2.device}")
    if p1.size(0) == 0 or p1.size(1) == 0 or p2.size(1) == 0:
        raise ValueError("empty point clouds are not supported "
                         f"(got {tuple(p1.shape)} and {tuple(p2.shape)})")
    _hip.dev_tensor(p1, torch.float32, "p1")
    _hip.dev_tensor(p2, torch.float32, "p2")


def _finite_number(value, name, ok, wording, allow_bool=False, number="a number") -> float:
    """``value`` as a Python float: a number that is finite and passes ``ok`` -- ``ValueError`` ``"<name> must be
    <wording>, got ..."`` otherwise, ``"<name> must be <number>, got ..."`` where ``float()`` refuses it.  ``bool`` counts as
    a number only where ``allow_bool``."""
    try:
        v = float(value)
    except (TypeError, ValueError):
        raise ValueError(f"{name} must be {number}, got {value!r}") from None
    if (isinstance(value, bool) and not allow_bool) or not (math.isfinite(v) and ok(v)):
        raise ValueError(f"{name} must be {wording}, got {value!r}")
    return v


def _integer_in(value, name, lo, hi) -> int:
    """``value`` as a Python int: an integer (never ``bool``) in ``lo..hi`` (``ValueError`` naming ``name`` otherwise)."""
    if isinstance(value, bool) or not isinstance(value, numbers.Integral):
        raise ValueError(f"{name} must be an integer in {lo}..{hi}, got {value!r}")
    if not lo <= int(value) <= hi:
        raise ValueError(f"{name} must be in {lo}..{hi}, got {value!r}")
    return int(value)


def _check_cloud(p, fn, max_n, n_ok, n_rule):
    """What a loss of ONE cloud batch checks in front of its launch: ``p`` is ``[B,N,3]``, ``B > 0``, ``n_ok(N)`` (worded
    ``n_rule``) and ``N <= max_n``; ``ValueError`` otherwise, in that order.  Returns ``(B, N)``."""
    if not isinstance(p, torch.Tensor) or p.dim() != 3 or p.size(2) != 3:
        raise ValueError(f"expected a [B,N,3] cloud tensor, got {tuple(getattr(p, 'shape', ()))}")
    B, N, _ = p.shape
    if B == 0:
        raise ValueError(f"empty batches are not supported (got {tuple(p.shape)})")
    if not n_ok(N):
        raise ValueError(f"{fn} needs {n_rule} points per cloud, got {N}")
    if N > max_n:
        raise ValueError(f"{fn} supports at most {max_n} points per cloud, got {N}")
    return B, N


def _sided_forward(p1, p2, losses=None):
    """K1 forward through the C ABI: ``(dist1 [B,N], dist2 [B,M], idx1, idx2)``, idx int32.
    ``losses = (n_first, w_first, w_rest)``: also K1l's three sums (``out3``, a fifth result) -- fused into the
    one-pass forward's second launch where that form serves, one more launch over the distances otherwise."""
    _check_clouds(p1, p2)
    B, N, _ = p1.shape
    M = p2.size(1)
    lib = _hip.load()
    dist1 = torch.empty((B, N), dtype=torch.float32, device=p1.device)
    dist2 = torch.empty((B, M), dtype=torch.float32, device=p1.device)
    idx1 = torch.empty((B, N), dtype=torch.int32, device=p1.device)
    idx2 = torch.empty((B, M), dtype=torch.int32, device=p1.device)
    out3 = torch.empty((3,), dtype=torch.float32, device=p1.device) if losses is not None else None
    # one-pass tiled form (every d(i,j) evaluated once) for clouds of at most 4096 points; the
    # two-pass kernel (no workspace) otherwise.  Bit-identical results.
    ws_bytes = lib.fpsg_chamfer_workspace_bytes(B, N, M, -1) if _tiled_enabled() else 0
    with torch.cuda.device(p1.device), _probe("chamfer_fwd", B, N, M):
        if ws_bytes:
            ws = torch.empty((ws_bytes,), dtype=torch.uint8, device=p1.device)
            if losses is not None:
                rc = lib.fpsg_chamfer_fwd_tiled_losses(_hip.ptr(p1), _hip.ptr(p2), B, N, M, _hip.ptr(dist1),
                                                       _hip.ptr(idx1), _hip.ptr(dist2), _hip.ptr(idx2),
                                                       _hip.ptr(ws), ws_bytes, -1, int(losses[0]), float(losses[1]),
                                                       float(losses[2]), _hip.ptr(out3), _hip.stream_of(p1))
            else:
                rc = lib.fpsg_chamfer_fwd_tiled(_hip.ptr(p1), _hip.ptr(p2), B, N, M, _hip.ptr(dist1),
                                                _hip.ptr(idx1), _hip.ptr(dist2), _hip.ptr(idx2),
                                                _hip.ptr(ws), ws_bytes, -1, _hip.stream_of(p1))
        else:
            rc = lib.fpsg_chamfer_fwd(_hip.ptr(p1), _hip.ptr(p2), B, N, M, _hip.ptr(dist1),
                                      _hip.ptr(idx1), _hip.ptr(dist2), _hip.ptr(idx2),
                                      _hip.stream_of(p1))
    _hip.check(rc, "fpsg_chamfer_fwd")
    if losses is None:
        return dist1, dist2, idx1, idx2
    if not ws_bytes:
        with torch.cuda.device(p1.device):
            rc = lib.fpsg_chamfer_losses(_hip.ptr(dist1), _hip.ptr(dist2), B, N, M, int(losses[0]), float(losses[1]),
                                         float(losses[2]), _hip.ptr(out3), _hip.stream_of(p1))
        _hip.check(rc, "fpsg_chamfer_losses")
    return dist1, dist2, idx1, idx2, out3


def _sided_backward(p1, p2, idx1, idx2, g1, g2):
    """K1 backward: ``g1 [B,N]``, ``g2 [B,M]`` contiguous fp32 -> gradients of the two clouds."""
    B, N, _ = p1.shape
    M = p2.size(1)
    gx1 = torch.empty_like(p1)
    gx2 = torch.empty_like(p2)
    with torch.cuda.device(p1.device), _probe("chamfer_bwd", B, N, M):
        rc = _hip.load().fpsg_chamfer_bwd(_hip.ptr(p1), _hip.ptr(p2), _hip.ptr(idx1),
                                          _hip.ptr(idx2), _hip.ptr(g1), _hip.ptr(g2), B, N,
                                          M, _hip.ptr(gx1), _hip.ptr(gx2),
                                          _hip.stream_of(p1))
    _hip.check(rc, "fpsg_chamfer_bwd")
    return gx1, gx2


class _SidedPair(torch.autograd.Function):
    """(dist1, dist2, idx1, idx2) of two clouds in ONE launch; idx are int32, no grad."""

    @staticmethod
    def forward(ctx, p1, p2):
        ctx.set_materialize_grads(False)        # no zero tensors for the index outputs (or an unused direction)
        dist1, dist2, idx1, idx2 = _sided_forward(p1, p2)
        ctx.save_for_backward(p1, p2, idx1, idx2)
        ctx.mark_non_differentiable(idx1, idx2)
        return dist1, dist2, idx1, idx2

    @staticmethod
    def backward(ctx, g1, g2, _gi1, _gi2):
        if g1 is None and g2 is None:
            return None, None
        p1, p2, idx1, idx2 = ctx.saved_tensors
        B, N, _ = p1.shape
        M = p2.size(1)
        g1 = torch.zeros((B, N), dtype=torch.float32, device=p1.device) if g1 is None \
            else g1.contiguous().float()
        g2 = torch.zeros((B, M), dtype=torch.float32, device=p1.device) if g2 is None \
            else g2.contiguous().float()
        return _sided_backward(p1, p2, idx1, idx2, g1, g2)


class _EpisodeChamfer(torch.autograd.Function):
    """K1 + K1l: the Chamfer distances of B cloud pairs and the sums over the first ``n_first`` pairs, over the rest,
    and their weighted total -- inside the one-pass forward (``fpsg_chamfer_fwd_tiled_losses``) or one launch behind the
    two-pass one (``fpsg_chamfer_losses``); the backward forms the per-pair constant gradients inside the K1 backward
    kernel (``fpsg_chamfer_bwd_losses``; clouds beyond 4096 points: ``fpsg_chamfer_loss_grads`` + the scanning kernel)."""

    @staticmethod
    def forward(ctx, p1, p2, n_first, w_first, w_rest):
        ctx.set_materialize_grads(False)
        _, _, idx1, idx2, out = _sided_forward(p1, p2, losses=(n_first, w_first, w_rest))
        ctx.save_for_backward(p1, p2, idx1, idx2)
        ctx.cfg = (int(n_first), float(w_first), float(w_rest))
        return out[0], out[1], out[2]

    @staticmethod
    def backward(ctx, g_first, g_rest, g_total):
        if g_first is None and g_rest is None and g_total is None:
            return None, None, None, None, None
        p1, p2, idx1, idx2 = ctx.saved_tensors
        n_first, w_first, w_rest = ctx.cfg
        B, N, _ = p1.shape
        M = p2.size(1)
        keep = [None if g is None else g.reshape(1).contiguous().float() for g in (g_first, g_rest, g_total)]
        if N <= 4096 and M <= 4096:
            gx1 = torch.empty_like(p1)
            gx2 = torch.empty_like(p2)
            with torch.cuda.device(p1.device), _probe("chamfer_bwd", B, N, M):
                rc = _hip.load().fpsg_chamfer_bwd_losses(_hip.ptr(p1), _hip.ptr(p2), _hip.ptr(idx1), _hip.ptr(idx2),
                                                         *(None if g is None else _hip.ptr(g) for g in keep), B, N, M,
                                                         n_first, w_first, w_rest, _hip.ptr(gx1), _hip.ptr(gx2),
                                                         _hip.stream_of(p1))
            _hip.check(rc, "fpsg_chamfer_bwd_losses")
            return gx1, gx2, None, None, None
        g1 = torch.empty((B, N), dtype=torch.float32, device=p1.device)
        g2 = torch.empty((B, M), dtype=torch.float32, device=p1.device)
        with torch.cuda.device(p1.device):
            rc = _hip.load().fpsg_chamfer_loss_grads(*(None if g is None else _hip.ptr(g) for g in keep), B, N, M,
                                                     n_first, w_first, w_rest, _hip.ptr(g1), _hip.ptr(g2),
                                                     _hip.stream_of(p1))
        _hip.check(rc, "fpsg_chamfer_loss_grads")
        gx1, gx2 = _sided_backward(p1, p2, idx1, idx2, g1, g2)
        return gx1, gx2, None, None, None


def episode_chamfer_losses(p1: torch.Tensor, p2: torch.Tensor, n_first: int, w_first: float, w_rest: float):
    """``cd = chamfer_distance(p1, p2)`` over B pairs -> ``(cd[:n_first].sum(), cd[n_first:].sum(),
    w_first * first + w_rest * rest)`` as 0-dim tensors: the reconstruction losses of an episode whose query and
    support pairs were batched into one K1 call (reference few_shot.py:110-124), two launches instead of ten."""
    return _EpisodeChamfer.apply(p1, p2, n_first, w_first, w_rest)


def sided_distances(p1: torch.Tensor, p2: torch.Tensor):
    """Both directions at once: ``(dist1 [B,N], idx1 [B,N], dist2 [B,M], idx2 [B,M])``
    with int64 indices (as Kaolin exposes them).  Differentiable in p1 and p2."""
    d1, d2, i1, i2 = _SidedPair.apply(p1, p2)
    return d1, i1.long(), d2, i2.long()


def sided_distance(p1: torch.Tensor, p2: torch.Tensor):
    """``kaolin.metrics.pointcloud.sided_distance``: for every point of ``p1`` the squared
    distance to, and the index of, its nearest point of ``p2``: ``(dist [B,N], idx [B,N])``."""
    d1, i1, _, _ = sided_distances(p1, p2)
    return d1, i1


def chamfer_distance(p1: torch.Tensor, p2: torch.Tensor, w1: float = 1.0, w2: float = 1.0):
    """``kaolin.metrics.pointcloud.chamfer_distance`` (0.9.0):
    ``w1 * mean_i min_j |p1_i - p2_j|^2 + w2 * mean_j min_i |p2_j - p1_i|^2`` -> ``[B]``."""
    d1, d2, _, _ = _SidedPair.apply(p1, p2)
    dist_to_p2 = d1.mean(dim=-1)
    dist_to_p1 = d2.mean(dim=-1)
    if w1 == 1 and w2 == 1:
        return dist_to_p2 + dist_to_p1
    return w1 * dist_to_p2 + w2 * dist_to_p1



CHAMFER_CROSS_MAX_N = 4096      # FPSG_CHAMFER_CROSS_MAX_N (include/fpsg_hip.h)


def chamfer_matrix(A: torch.Tensor, B: torch.Tensor | None = None) -> torch.Tensor:
    """All-pairs Chamfer matrix ``[Na,Nb]`` (K13, HIP): ``out[a][b] = chamfer_distance(A[a:a+1], B[b:b+1])`` for clouds
    ``A [Na,N,3]`` and ``B [Nb,M,3]`` (N, M <= 4096), with the same per-point minima as K1 bit for bit and only the
    order of the two means' summation different (``include/fpsg_hip.h``, K13).  ``B=None``: ``A`` against itself, each
    unordered pair evaluated once, an exact-zero diagonal, bitwise symmetric and equal to ``chamfer_matrix(A, A)``.

    Deterministic: every entry is bitwise the same whatever set, slice or call it is computed in, and
    ``chamfer_matrix(B, A) == chamfer_matrix(A, B).T`` bitwise.  Forward only: the result never requires grad (it is
    an evaluation metric; there is no backward).  No CPU path: CPU tensors raise ``FpsgHipError``."""
    sym = B is None
    other = A if sym else B
    if A.dim() != 3 or other.dim() != 3 or A.size(2) != 3 or other.size(2) != 3:
        raise ValueError(f"expected [Na,N,3] and [Nb,M,3] clouds, got {tuple(A.shape)} and {tuple(other.shape)}")
    if A.device != other.device:
        raise ValueError(f"device mismatch: {A.device} vs {other.device}")
    if A.numel() == 0 or other.numel() == 0:
        raise ValueError(f"empty sets or clouds are not supported (got {tuple(A.shape)} and {tuple(other.shape)})")
    A = A.detach()
    other = other.detach()
    _hip.dev_tensor(A, torch.float32, "A")
    _hip.dev_tensor(other, torch.float32, "B")
    Na, N, _ = A.shape
    Nb, M, _ = other.shape
    lib = _hip.load()
    out = torch.empty((Na, Nb), dtype=torch.float32, device=A.device)
    with torch.cuda.device(A.device), _probe("chamfer_cross", Na * Nb, N, M):
        rc = lib.fpsg_chamfer_cross(_hip.ptr(A), None if sym else _hip.ptr(other), Na, Nb, N, M, _hip.ptr(out),
                                    _hip.stream_of(A))
    _hip.check(rc, "fpsg_chamfer_cross")
    return out

class _EmdApprox(torch.autograd.Function):
    """cost [B] of the approximate-assignment solver; the gradients (assignment held
    constant) are produced by the same solver run and cached for backward."""

    @staticmethod
    def forward(ctx, p1, p2):
        _check_clouds(p1, p2)
        B, N, _ = p1.shape
        M = p2.size(1)
        lib = _hip.load()
        dev = p1.device
        need1, need2 = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        cost = torch.empty((B,), dtype=torch.float32, device=dev)
        g1 = torch.empty_like(p1) if need1 else None
        g2 = torch.empty_like(p2) if need2 else None
        ws = torch.empty((lib.fpsg_emd_workspace_floats(B, N, M),), dtype=torch.float32, device=dev)
        with torch.cuda.device(dev), _probe("emd_approx", B, N, M):
            rc = lib.fpsg_emd_approx(_hip.ptr(p1), _hip.ptr(p2), B, N, M, _hip.ptr(cost),
                                     _hip.ptr(g1) if need1 else None,
                                     _hip.ptr(g2) if need2 else None, _hip.ptr(ws),
                                     _hip.stream_of(p1))
        _hip.check(rc, "fpsg_emd_approx")
        ctx.grads = (g1, g2)
        return cost

    @staticmethod
    def backward(ctx, gcost):
        g1, g2 = ctx.grads
        gc = gcost.reshape(-1, 1, 1)
        return (None if g1 is None else g1 * gc), (None if g2 is None else g2 * gc)


def emd_approx(p1: torch.Tensor, p2: torch.Tensor) -> torch.Tensor:
    """Transport cost ``[B]`` of the approximate assignment between ``p1 [B,N,3]`` and
    ``p2 [B,M,3]`` (sum over matched pairs of Euclidean distances, not divided by N)."""
    return _EmdApprox.apply(p1, p2)


EMD_EXACT_MAX_N = 2048          # FPSG_EMD_EXACT_MAX_N (include/fpsg_hip.h)
EMD_EXACT_MAX_ROUNDS = 1 << 18  # default round cap of emd_exact per pair


class EmdExactCapWarning(RuntimeWarning):
    """``emd_exact`` stopped a pair at its round cap: its cost is that of a complete but not certified-optimal
    assignment (still an upper bound; ``cost - gap`` is still a lower bound)."""


def emd_exact_default_eps(p1: torch.Tensor, p2: torch.Tensor) -> float:
    """Default final auction step of ``emd_exact``: ``2e-5 * D / N^(1/3)``, D the bounding-box diagonal of both clouds.

    The exact cost is N times the mean matched distance, which for N points spread over a set of extent D is of order
    ``D / N^(1/3)`` (about ``0.03 D`` for 2048-point unit-ball pairs); the auction's error is at most ``N * eps``, so this
    ``eps`` keeps it near 1e-4 of a typical cost or below (measured on unit-ball pairs: DESIGN.md K12), while leaving the
    step several fp32 ulps of the prices (at most ~D).  One host read (the diagonal)."""
    pts = torch.cat([p1.detach().reshape(-1, 3), p2.detach().reshape(-1, 3)])
    diag = float((pts.amax(0) - pts.amin(0)).norm())
    n = p1.size(1)
    return max(2e-5 * diag / n ** (1.0 / 3.0), 1e-30)


def _emd_exact_forward(p1, p2, eps, max_rounds, need1, need2):
    if p1.dim() == 3 and p2.dim() == 3:
        if p1.size(1) != p2.size(1):
            raise ValueError(f"emd_exact needs clouds of equal size, got N={p1.size(1)} and M={p2.size(1)}")
        if p1.size(1) > EMD_EXACT_MAX_N:
            raise ValueError(f"emd_exact supports at most {EMD_EXACT_MAX_N} points per cloud, got {p1.size(1)}")
    _check_clouds(p1, p2)
    B, N, _ = p1.shape
    if eps is None:
        eps = emd_exact_default_eps(p1, p2)
    if max_rounds is None:
        max_rounds = EMD_EXACT_MAX_ROUNDS
    lib = _hip.load()
    dev = p1.device
    cost = torch.empty((B,), dtype=torch.float32, device=dev)
    gap = torch.empty((B,), dtype=torch.float32, device=dev)
    assign = torch.empty((B, N), dtype=torch.int32, device=dev)
    status = torch.empty((B,), dtype=torch.int32, device=dev)
    g1 = torch.empty_like(p1) if need1 else None
    g2 = torch.empty_like(p2) if need2 else None
    ws = torch.empty((lib.fpsg_emd_exact_workspace_floats(B, N),), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev), _probe("emd_exact", B, N, N):
        rc = lib.fpsg_emd_exact(_hip.ptr(p1), _hip.ptr(p2), B, N, float(eps), int(max_rounds), _hip.ptr(cost),
                                _hip.ptr(gap), _hip.ptr(assign), _hip.ptr(status), _hip.ptr(g1) if need1 else None,
                                _hip.ptr(g2) if need2 else None, _hip.ptr(ws), _hip.stream_of(p1))
    _hip.check(rc, "fpsg_emd_exact")
    stats = ws.view(torch.int32).reshape(B, 4)
    info = {"assign": assign, "gap": gap, "status": status, "rounds": stats[:, 0], "eps": float(eps)}
    return cost, g1, g2, info


class _EmdExact(torch.autograd.Function):
    """cost [B] of the exact assignment (K12); the gradients (assignment held constant) come from the same launch."""

    @staticmethod
    def forward(ctx, p1, p2, eps, max_rounds, info_out):
        cost, g1, g2, info = _emd_exact_forward(p1, p2, eps, max_rounds, ctx.needs_input_grad[0],
                                                ctx.needs_input_grad[1])
        info_out.update(info)
        ctx.grads = (g1, g2)
        return cost

    @staticmethod
    def backward(ctx, gcost):
        g1, g2 = ctx.grads
        gc = gcost.reshape(-1, 1, 1)
        return (None if g1 is None else g1 * gc), (None if g2 is None else g2 * gc), None, None, None


def emd_exact(p1: torch.Tensor, p2: torch.Tensor, eps: float | None = None, max_rounds: int | None = None,
              return_info: bool = False):
    """Exact Earth Mover's Distance ``[B]`` between equal-size clouds ``p1, p2 [B,N,3]`` (N <= 2048): the minimum over
    permutations of the sum of Euclidean distances of matched points (not divided by N) -- what K2 (``emd_approx``)
    and K2b (``sinkhorn_divergence``) approximate.  A bounded auction (K12, HIP) finds it to within ``N * eps``.

    ``eps``: the final auction step (default ``emd_exact_default_eps``: the error bound ``N * eps`` is ~1e-4 of a
    typical cost); ``max_rounds``: round cap per pair (default ``EMD_EXACT_MAX_ROUNDS``).  Differentiable in both clouds
    with the assignment held constant (K2's convention).  ``return_info=True``: returns ``(cost, info)`` with
    ``info["assign"] [B,N]`` int32 (a permutation), ``info["gap"] [B]`` (certificate: ``cost - gap <= exact EMD <=
    cost``), ``info["status"] [B]`` int32 (0 converged, 1 round cap hit) and ``info["rounds"] [B]``.

    A pair that hits the round cap is not an error: its cost is that of a complete assignment and its gap still
    brackets the exact value, so ``emd_exact`` issues an ``EmdExactCapWarning`` naming the pairs (one host read of
    ``status``) and returns.  Raises ``ValueError`` for clouds of different sizes or beyond 2048 points."""
    info = {}
    cost = _EmdExact.apply(p1, p2, eps, max_rounds, info)
    capped = torch.nonzero(info["status"]).flatten().tolist()
    if capped:
        import warnings
        warnings.warn(f"emd_exact: pairs {capped} hit the round cap (max_rounds="
                      f"{EMD_EXACT_MAX_ROUNDS if max_rounds is None else max_rounds}); their cost is an upper bound "
                      f"within gap {info['gap'][capped].tolist()} of the exact EMD", EmdExactCapWarning, stacklevel=2)
    return (cost, info) if return_info else cost


def emd_matrix(A: torch.Tensor, B: torch.Tensor | None = None, eps: float | None = None, max_rounds: int | None = None,
               return_info: bool = False):
    """All-pairs exact EMD matrix ``[Na,Nb]`` (K14, HIP): ``out[a][b]`` is the exact EMD of ``(A[a], B[b])`` as
    ``emd_exact`` computes it (sum of matched distances, not divided by N) for clouds ``A [Na,N,3]`` and ``B [Nb,N,3]``
    of equal size N <= 2048.  ``B=None``: ``A`` against itself, each unordered pair solved once with ``A[a]`` (a < b)
    as bidders and mirrored, an exact-zero diagonal.

    One ``eps`` serves the whole call: by default ``emd_exact_default_eps`` over the union of both sets, so an entry
    is reproduced by ``emd_exact(A[a:a+1], B[b:b+1], eps=that_eps)`` -- same rounds and status, same cost and gap.
    Deterministic: every entry is bitwise the same whatever set, slice or call it is computed in.  ``emd_matrix(B, A).T``
    agrees with ``emd_matrix(A, B)`` within the gaps only (the bidder and object roles swap).

    ``return_info=True``: returns ``(cost, info)`` with ``info["gap"] [Na,Nb]`` (``cost - gap <= EMD <= cost``),
    ``info["status"]`` and ``info["rounds"]`` (int32 ``[Na,Nb]``) and ``info["eps"]``.  A pair capped at ``max_rounds``
    (default ``EMD_EXACT_MAX_ROUNDS``) issues an ``EmdExactCapWarning`` naming its ``(a, b)``.  Forward only; no CPU
    path (CPU tensors raise ``FpsgHipError``).  Raises ``ValueError`` for unequal N, N > 2048, empty sets and bad
    shapes."""
    sym = B is None
    other = A if sym else B
    if A.dim() != 3 or other.dim() != 3 or A.size(2) != 3 or other.size(2) != 3:
        raise ValueError(f"expected [Na,N,3] and [Nb,N,3] clouds, got {tuple(A.shape)} and {tuple(other.shape)}")
    if A.numel() == 0 or other.numel() == 0:
        raise ValueError(f"empty sets or clouds are not supported (got {tuple(A.shape)} and {tuple(other.shape)})")
    if A.size(1) != other.size(1):
        raise ValueError(f"emd_matrix needs clouds of equal size, got N={A.size(1)} and N={other.size(1)}")
    if A.size(1) > EMD_EXACT_MAX_N:
        raise ValueError(f"emd_matrix supports at most {EMD_EXACT_MAX_N} points per cloud, got {A.size(1)}")
    if A.device != other.device:
        raise ValueError(f"device mismatch: {A.device} vs {other.device}")
    if max_rounds is not None and int(max_rounds) < 1:
        raise ValueError(f"max_rounds must be at least 1, got {max_rounds}")
    if eps is not None and not (float(eps) > 0.0 and math.isfinite(float(eps))):
        raise ValueError(f"eps must be positive and finite, got {eps}")
    A = A.detach()
    other = other.detach()
    _hip.dev_tensor(A, torch.float32, "A")
    _hip.dev_tensor(other, torch.float32, "B")
    Na, N, _ = A.shape
    Nb = other.size(0)
    if eps is None:
        eps = emd_exact_default_eps(A, other)
    if max_rounds is None:
        max_rounds = EMD_EXACT_MAX_ROUNDS
    lib = _hip.load()
    dev = A.device
    cost = torch.empty((Na, Nb), dtype=torch.float32, device=dev)
    gap = torch.empty((Na, Nb), dtype=torch.float32, device=dev)
    status = torch.empty((Na, Nb), dtype=torch.int32, device=dev)
    rounds = torch.empty((Na, Nb), dtype=torch.int32, device=dev)
    ws_bytes = lib.fpsg_emd_cross_workspace_bytes(Na, Nb, N)
    ws = torch.empty((ws_bytes,), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev), _probe("emd_cross", Na * Nb, N, N):
        rc = lib.fpsg_emd_cross(_hip.ptr(A), None if sym else _hip.ptr(other), Na, Nb, N, float(eps), int(max_rounds),
                                _hip.ptr(cost), _hip.ptr(gap), _hip.ptr(status), _hip.ptr(rounds), _hip.ptr(ws),
                                ws_bytes, _hip.stream_of(A))
    _hip.check(rc, "fpsg_emd_cross")
    capped = [tuple(x) for x in torch.nonzero(status).tolist()]
    if capped:
        import warnings
        warnings.warn(f"emd_matrix: pairs {capped} (a, b) hit the round cap (max_rounds={max_rounds}); their cost is an "
                      f"upper bound within its gap of the exact EMD", EmdExactCapWarning, stacklevel=2)
    if return_info:
        return cost, {"gap": gap, "status": status, "rounds": rounds, "eps": float(eps)}
    return cost


OCCUPANCY_MAX_RES = 64          # FPSG_OCCUPANCY_MAX_RES (include/fpsg_hip.h)


def occupancy_grid(clouds: torch.Tensor, resolution: int = 28, half_extent: float = 1.0, in_sphere: bool = True,
                   out: dict | None = None, return_cells: bool = False) -> dict:
    """Voxel-occupancy grid of the clouds ``[S,N,3]`` (K15, HIP; the definition is in ``include/fpsg_hip.h``): a dict
    with ``"counts"`` (points per cell) and ``"clouds_hit"`` (clouds with at least one point in the cell), int32
    ``[r,r,r]`` on the clouds' device, ``"outside"`` int32 ``[3]`` (finite points with a coordinate beyond the half
    extent, finite points beyond the sphere of that radius, non-finite points -- the last have no cell),
    ``"n_clouds"`` and ``"n_points"`` (Python ints) and the parameters.  ``resolution`` 2..64 (3.. with ``in_sphere``:
    only the nodes inside the sphere inscribed in the grid are cells, a point that rounds to another node goes to the
    nearest retained one).  ``half_extent``: 1.0 for clouds in the unit ball, 0.5 for the unit cube.

    ``out``: a dict returned by an earlier call with the same parameters: this call's clouds are accumulated into it
    (running totals; ``ValueError`` on a parameter mismatch) and it is returned.  ``return_cells=True`` adds
    ``"cells"``, int32 ``[S,N]``, the linear cell index ``(i r + j) r + k`` of every point of this call (-1: none).

    Integers formed with integer atomics: bitwise the same on every run and whatever the split into calls.  Forward
    only; no CPU path (CPU tensors raise ``FpsgHipError``); ``ValueError`` for bad shapes or parameters."""
    if not isinstance(clouds, torch.Tensor) or clouds.dim() != 3 or clouds.size(2) != 3:
        raise ValueError(f"expected [S,N,3] clouds, got {tuple(getattr(clouds, 'shape', ()))}")
    if clouds.size(0) < 1 or clouds.size(1) < 1:
        raise ValueError(f"empty sets or clouds are not supported (got {tuple(clouds.shape)})")
    r = int(resolution)
    if r != resolution or r < 2 or r > OCCUPANCY_MAX_RES:
        raise ValueError(f"resolution must be an integer from 2 to {OCCUPANCY_MAX_RES}, got {resolution}")
    in_sphere = bool(in_sphere)
    if in_sphere and r < 3:
        raise ValueError("in_sphere retains no node at resolution 2; use at least 3")
    E = float(half_extent)
    if not (E > 0.0 and math.isfinite(E)):
        raise ValueError(f"half_extent must be positive and finite, got {half_extent}")
    params = {"resolution": r, "half_extent": E, "in_sphere": in_sphere}
    if out is not None:
        for k, v in params.items():
            if out.get(k) != v:
                raise ValueError(f"out= was made with {k}={out.get(k)!r}, this call has {k}={v!r}")
        if out["counts"].device != clouds.device:
            raise ValueError(f"device mismatch: out= on {out['counts'].device}, clouds on {clouds.device}")
    clouds = clouds.detach()
    _hip.dev_tensor(clouds, torch.float32, "clouds")
    S, N, _ = clouds.shape
    dev = clouds.device
    if out is None:
        out = dict(params, counts=torch.zeros((r, r, r), dtype=torch.int32, device=dev),
                   clouds_hit=torch.zeros((r, r, r), dtype=torch.int32, device=dev),
                   outside=torch.zeros((3,), dtype=torch.int32, device=dev), n_clouds=0, n_points=0)
    cells = torch.empty((S, N), dtype=torch.int32, device=dev) if return_cells else None
    lib = _hip.load()
    ws_bytes = lib.fpsg_occupancy_grid_workspace_bytes(S, N, r)
    ws = torch.empty((ws_bytes,), dtype=torch.uint8, device=dev) if ws_bytes else None
    with torch.cuda.device(dev), _probe("occupancy_grid", S, N, r):
        rc = lib.fpsg_occupancy_grid(_hip.ptr(clouds), S, N, r, E, int(in_sphere), _hip.ptr(out["counts"]),
                                     _hip.ptr(out["clouds_hit"]), _hip.ptr(out["outside"]),
                                     None if cells is None else _hip.ptr(cells), None if ws is None else _hip.ptr(ws),
                                     ws_bytes, _hip.stream_of(clouds))
    _hip.check(rc, "fpsg_occupancy_grid")
    out["n_clouds"] += S
    out["n_points"] += S * N
    out.pop("cells", None)
    if return_cells:
        out["cells"] = cells
    return out


PROFILE_MAX_T = 16              # FPSG_PROFILE_MAX_T (include/fpsg_hip.h)


def check_thresholds(thresholds) -> tuple:
    """The distance thresholds of ``distance_profile`` / ``fscore`` as a tuple of Python floats: a sequence of 1 to
    ``PROFILE_MAX_T`` finite, non-negative numbers (``ValueError`` otherwise)."""
    if isinstance(thresholds, (str, bytes, torch.Tensor)) or not hasattr(thresholds, "__len__"):
        raise ValueError(f"thresholds must be a sequence of numbers, got {thresholds!r}")
    if not 1 <= len(thresholds) <= PROFILE_MAX_T:
        raise ValueError(f"thresholds: from 1 to {PROFILE_MAX_T} values, got {len(thresholds)}")
    try:
        taus = tuple(float(t) for t in thresholds)
    except (TypeError, ValueError):
        raise ValueError(f"thresholds must be numbers, got {thresholds!r}") from None
    for t in taus:
        if not (math.isfinite(t) and t >= 0.0):
            raise ValueError(f"thresholds must be finite and non-negative, got {t!r}")
    return taus


def fscore_from_counts(counts: torch.Tensor, n1: int, n2: int) -> dict:
    """Precision, recall and F-score from K17's counts ``[B,2,T]`` (any integer dtype, any device), float64 ``[B,T]``
    each: ``precision = counts[:,0] / n1``, ``recall = counts[:,1] / n2``, ``fscore = 2 * P * R / (P + R)`` evaluated
    in that order, and exactly 0.0 where ``P + R == 0``.  ``ValueError`` for another rank, a non-integer dtype,
    ``n1`` or ``n2 < 1`` or a count outside ``[0, n]``."""
    if not isinstance(counts, torch.Tensor) or counts.dim() != 3 or counts.size(1) != 2:
        raise ValueError(f"expected counts [B,2,T], got {tuple(getattr(counts, 'shape', ()))}")
    if counts.dtype.is_floating_point or counts.dtype.is_complex or counts.dtype == torch.bool:
        raise ValueError(f"counts must have an integer dtype, got {counts.dtype}")
    if int(n1) != n1 or int(n2) != n2 or n1 < 1 or n2 < 1:
        raise ValueError(f"n1 and n2 must be positive integers, got {n1!r} and {n2!r}")
    if counts.numel():
        c = counts.long()
        if bool((c.min() < 0) | (c[:, 0].max() > n1) | (c[:, 1].max() > n2)):      # one host read
            raise ValueError(f"counts outside [0, n1={n1}] / [0, n2={n2}]")
    c = counts.to(torch.float64)
    precision, recall = c[:, 0] / int(n1), c[:, 1] / int(n2)
    s = precision + recall
    none = s == 0
    f = 2 * precision * recall / torch.where(none, torch.ones_like(s), s)
    return {"precision": precision, "recall": recall, "fscore": torch.where(none, torch.zeros_like(f), f)}


def distance_profile(dist1: torch.Tensor, dist2: torch.Tensor, thresholds):
    """K17 (HIP; the definition is in ``include/fpsg_hip.h``): for squared distances ``dist1 [B,N]`` and ``dist2
    [B,M]`` (K1's rows, or any non-negative fp32 rows) and 1 to 16 ``thresholds`` -- Euclidean distances in the clouds'
    units, finite and >= 0, in any order -- returns ``(counts, maxima)``: ``counts [B,2,T]`` int32, the number of
    entries of ``dist1[b]`` (``[:,0]``) and of ``dist2[b]`` (``[:,1]``) that are ``<= tau2[t]`` in fp32, with ``tau2[t] =
    float32(float(thresholds[t]) ** 2)`` (the square formed in double and rounded once); ``maxima [B,2]`` fp32,
    ``max(0, max_i dist[b,i])`` per direction.  A NaN entry is counted nowhere and ignored by the maximum.

    Exact and bitwise reproducible, independent of the batch.  Detached: the result never requires grad.  No CPU path
    (CPU tensors raise ``FpsgHipError``); ``ValueError`` for bad thresholds (checked first) or shapes."""
    taus = check_thresholds(thresholds)
    for t, name in ((dist1, "dist1"), (dist2, "dist2")):
        if not isinstance(t, torch.Tensor) or t.dim() != 2:
            raise ValueError(f"{name}: expected a [B,n] tensor, got {tuple(getattr(t, 'shape', ()))}")
    if dist1.size(0) != dist2.size(0):
        raise ValueError(f"batch mismatch: {dist1.size(0)} vs {dist2.size(0)}")
    if dist1.device != dist2.device:
        raise ValueError(f"device mismatch: {dist1.device} vs {dist2.device}")
    if dist1.numel() == 0 or dist2.numel() == 0:
        raise ValueError(f"empty rows are not supported (got {tuple(dist1.shape)} and {tuple(dist2.shape)})")
    dist1, dist2 = dist1.detach(), dist2.detach()
    _hip.dev_tensor(dist1, torch.float32, "dist1")
    _hip.dev_tensor(dist2, torch.float32, "dist2")
    B, N = dist1.shape
    M = dist2.size(1)
    T = len(taus)
    dev = dist1.device
    tau2 = torch.tensor([t * t for t in taus], dtype=torch.float64).to(torch.float32).to(dev)
    counts = torch.empty((B, 2, T), dtype=torch.int32, device=dev)
    maxima = torch.empty((B, 2), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev), _probe("dist_profile", B, N, M):
        rc = _hip.load().fpsg_dist_profile(_hip.ptr(dist1), _hip.ptr(dist2), B, N, M, _hip.ptr(tau2), T,
                                           _hip.ptr(counts), _hip.ptr(maxima), _hip.stream_of(dist1))
    _hip.check(rc, "fpsg_dist_profile")
    return counts, maxima


def fscore(p1: torch.Tensor, p2: torch.Tensor, thresholds) -> dict:
    """F-score at distance thresholds and the Hausdorff distance of the pairs ``p1 [B,N,3]`` (the reconstruction) and
    ``p2 [B,M,3]`` (the ground truth); ``thresholds`` as in ``distance_profile``.  K1's forward (the minima of
    ``chamfer_distance``, bit for bit), then K17, then ``fscore_from_counts``: a dict with ``"precision"`` (the share
    of reconstructed points within tau of the ground truth), ``"recall"`` (the share of ground-truth points within tau
    of the reconstruction) and ``"fscore"``, float64 ``[B,T]``; ``"hausdorff" [B]`` float64, ``sqrt(max(maxima[:,0],
    maxima[:,1]))``; and K17's ``"counts"`` and ``"maxima"``.  Forward only; no CPU path."""
    taus = check_thresholds(thresholds)
    return fscore_from_rows(nearest_rows(p1, p2), taus)


def nearest_rows(p1: torch.Tensor, p2: torch.Tensor):
    """K1's forward, detached and without autograd: ``(dist1 [B,N], dist2 [B,M], idx1, idx2)``, the squared
    nearest-neighbour distances of ``chamfer_distance`` (bit for bit) and the int32 indices of the neighbours -- the rows
    ``fscore_from_rows`` and ``dcd_from_rows`` read, so that a caller that wants both computes them once."""
    with torch.no_grad():
        return _sided_forward(p1.detach(), p2.detach())


def fscore_from_rows(rows, thresholds) -> dict:
    """``fscore(p1, p2, thresholds)`` from ``rows = nearest_rows(p1, p2)``: K17 over the two distance rows, then
    ``fscore_from_counts``.  ``ValueError`` as ``distance_profile`` (thresholds first, then the rows' shapes)."""
    taus = check_thresholds(thresholds)
    dist1, dist2 = rows[0], rows[1]
    counts, maxima = distance_profile(dist1, dist2, taus)
    out = fscore_from_counts(counts, dist1.size(1), dist2.size(1))
    out["hausdorff"] = maxima.to(torch.float64).amax(dim=1).sqrt()
    out["counts"], out["maxima"] = counts, maxima
    return out


DCD_MAX_N = 16384               # FPSG_DCD_MAX_N (include/fpsg_hip.h)
DCD_DEFAULT_ALPHA = 1000.0


def check_dcd_alpha(alpha) -> float:
    """``alpha`` of ``dcd`` as a Python float: a finite, non-negative number (``ValueError`` otherwise)."""
    return _finite_number(alpha, "alpha", lambda a: a >= 0.0, "finite and non-negative", allow_bool=True)


def _dcd_from_rows(dist1, idx1, dist2, idx2, alpha, need1, need2):
    """K18 through the C ABI on K1's rows: ``(out [B], sides [B,2], deg1 [B,N], deg2 [B,M], w1 | None, w2 | None)``."""
    B, N = dist1.shape
    M = dist2.size(1)
    dev = dist1.device
    out = torch.empty((B,), dtype=torch.float32, device=dev)
    sides = torch.empty((B, 2), dtype=torch.float32, device=dev)
    deg1 = torch.empty((B, N), dtype=torch.int32, device=dev)
    deg2 = torch.empty((B, M), dtype=torch.int32, device=dev)
    w1 = torch.empty((B, N), dtype=torch.float32, device=dev) if need1 else None
    w2 = torch.empty((B, M), dtype=torch.float32, device=dev) if need2 else None
    with torch.cuda.device(dev), _probe("dcd", B, N, M):
        rc = _hip.load().fpsg_dcd(_hip.ptr(dist1), _hip.ptr(idx1), _hip.ptr(dist2), _hip.ptr(idx2), B, N, M, float(alpha),
                                  _hip.ptr(out), _hip.ptr(sides), _hip.ptr(deg1), _hip.ptr(deg2),
                                  None if w1 is None else _hip.ptr(w1), None if w2 is None else _hip.ptr(w2),
                                  _hip.stream_of(dist1))
    _hip.check(rc, "fpsg_dcd")
    return out, sides, deg1, deg2, w1, w2


def dcd_from_rows(rows, alpha: float = DCD_DEFAULT_ALPHA) -> torch.Tensor:
    """``dcd(p1, p2, alpha)`` ``[B]`` from ``rows = nearest_rows(p1, p2)``: K18 without the weight rows, the value ``dcd``
    returns when no input needs a gradient, bit for bit.  ``ValueError`` (before anything else) for a bad ``alpha``, rows
    that are not ``[B,N]`` / ``[B,M]`` of one batch and one device, empty rows and more than 16384 entries per row."""
    alpha = check_dcd_alpha(alpha)
    dist1, dist2, idx1, idx2 = rows
    for t, like in ((dist1, dist1), (dist2, dist2), (idx1, dist1), (idx2, dist2)):
        if not isinstance(t, torch.Tensor) or t.dim() != 2 or t.shape != like.shape:
            raise ValueError("expected K1's rows dist1 [B,N], dist2 [B,M], idx1 [B,N], idx2 [B,M], got "
                             f"{[tuple(getattr(r, 'shape', ())) for r in rows]}")
    if dist1.size(0) != dist2.size(0):
        raise ValueError(f"batch mismatch: {dist1.size(0)} vs {dist2.size(0)}")
    if dist1.numel() == 0 or dist2.numel() == 0:
        raise ValueError(f"empty rows are not supported (got {tuple(dist1.shape)} and {tuple(dist2.shape)})")
    if dist1.size(1) > DCD_MAX_N or dist2.size(1) > DCD_MAX_N:
        raise ValueError(f"dcd supports at most {DCD_MAX_N} points per cloud, got {dist1.size(1)} and {dist2.size(1)}")
    if len({t.device for t in rows}) != 1:
        raise ValueError(f"device mismatch: {[str(t.device) for t in rows]}")
    _hip.dev_tensor(dist1, torch.float32, "dist1")
    _hip.dev_tensor(dist2, torch.float32, "dist2")
    _hip.dev_tensor(idx1, torch.int32, "idx1")
    _hip.dev_tensor(idx2, torch.int32, "idx2")
    return _dcd_from_rows(dist1, idx1, dist2, idx2, alpha, False, False)[0]


class _Dcd(torch.autograd.Function):
    """K1's forward, then K18 with the per-point derivatives ``w1`` / ``w2`` where an input needs a gradient; the
    backward scales them by the upstream ``[B]`` gradient and is K1's backward (the counts held constant)."""

    @staticmethod
    def forward(ctx, p1, p2, alpha, info_out):
        ctx.set_materialize_grads(False)
        need = ctx.needs_input_grad[0] or ctx.needs_input_grad[1]
        dist1, dist2, idx1, idx2 = _sided_forward(p1, p2)
        # both weight rows as soon as one cloud needs a gradient: either cloud's gradient takes both directions
        out, sides, deg1, deg2, w1, w2 = _dcd_from_rows(dist1, idx1, dist2, idx2, alpha, need, need)
        if info_out is not None:
            info_out.update(sides=sides, deg1=deg1, deg2=deg2, dist1=dist1, dist2=dist2, idx1=idx1, idx2=idx2)
        if need:
            ctx.save_for_backward(p1, p2, idx1, idx2, w1, w2)
        return out

    @staticmethod
    def backward(ctx, g):
        if g is None:
            return None, None, None, None
        p1, p2, idx1, idx2, w1, w2 = ctx.saved_tensors
        gc = g.reshape(-1, 1).float()
        gx1, gx2 = _sided_backward(p1, p2, idx1, idx2, (w1 * gc).contiguous(), (w2 * gc).contiguous())
        return (gx1 if ctx.needs_input_grad[0] else None), (gx2 if ctx.needs_input_grad[1] else None), None, None


def dcd(p1: torch.Tensor, p2: torch.Tensor, alpha: float = DCD_DEFAULT_ALPHA, return_info: bool = False):
    """Density-aware Chamfer distance ``[B]`` fp32 in ``[0, 1]`` of the pairs ``p1 [B,N,3]`` and ``p2 [B,M,3]`` (Wu et
    al., NeurIPS 2021; K18, HIP; the definition is in ``include/fpsg_hip.h``): with K1's squared nearest-neighbour
    distances ``d`` and indices, ``0.5 * (mean_i (1 - exp(-alpha d1_i) / deg2[idx1_i]) + mean_j (1 - exp(-alpha d2_j) /
    deg1[idx2_j]))``, where ``deg2[j]`` is the number of points of ``p1`` whose nearest neighbour is ``p2[j]`` and
    ``deg1`` the same the other way.  ``alpha`` multiplies the *squared* distance (default 1000, count exponent 1: the
    published code's defaults as recalled; parity UNPINNED).  ``N != M`` is the formula as it stands.

    Differentiable in both clouds, the counts held constant: K18 also writes ``d dcd / d d`` per point and the
    backward is K1's deterministic one.  Bitwise the same on every run and independent of the batch;
    ``dcd(p1, p2) == dcd(p2, p1)`` bitwise.  The call only enqueues (no host read): it can be captured in a graph.

    ``return_info=True``: returns ``(dcd, info)`` with ``info["sides"] [B,2]`` (the two means), ``"deg1" [B,N]``,
    ``"deg2" [B,M]`` (int32) and K1's ``"dist1"``, ``"dist2"``, ``"idx1"``, ``"idx2"`` (int32).

    ``ValueError`` (before anything else) for bad shapes, empty clouds, more than 16384 points per cloud, and an
    ``alpha`` that is negative or not finite.  No CPU path: CPU tensors raise ``FpsgHipError``."""
    alpha = check_dcd_alpha(alpha)
    for t in (p1, p2):
        if not isinstance(t, torch.Tensor) or t.dim() != 3 or t.size(2) != 3:
            raise ValueError(f"expected [B,N,3] and [B,M,3] clouds, got {tuple(getattr(p1, 'shape', ()))} and "
                             f"{tuple(getattr(p2, 'shape', ()))}")
    if p1.size(0) != p2.size(0):
        raise ValueError(f"batch mismatch: {p1.size(0)} vs {p2.size(0)}")
    if p1.size(0) == 0 or p1.size(1) == 0 or p2.size(1) == 0:
        raise ValueError(f"empty point clouds are not supported (got {tuple(p1.shape)} and {tuple(p2.shape)})")
    if p1.size(1) > DCD_MAX_N or p2.size(1) > DCD_MAX_N:
        raise ValueError(f"dcd supports at most {DCD_MAX_N} points per cloud, got {p1.size(1)} and {p2.size(1)}")
    if p1.device != p2.device:
        raise ValueError(f"device mismatch: {p1.device} vs {p2.device}")
    info = {} if return_info else None
    out = _Dcd.apply(p1, p2, alpha, info)
    return (out, info) if return_info else out


REPULSION_MAX_N = 16384          # FPSG_REPULSION_MAX_N (include/fpsg_hip.h)
REPULSION_MAX_K = 8             # FPSG_REPULSION_MAX_K


def check_repulsion_options(k, h):
    """``(k, h)`` of ``repulsion_loss`` as a Python int and float: ``k`` an integer in 1..8, ``h`` a positive, finite
    number (``ValueError`` naming the argument otherwise)."""
    k = _integer_in(k, "k", 1, REPULSION_MAX_K)
    return k, _finite_number(h, "h", lambda v: v > 0.0, "positive and finite")


class _Repulsion(torch.autograd.Function):
    """K21's forward (neighbour lists and the value per cloud) and its gather backward on the saved lists."""

    @staticmethod
    def forward(ctx, p, k, h, info_out):
        ctx.set_materialize_grads(False)
        B, N, _ = p.shape
        lib = _hip.load()
        idx = torch.empty((B, N, k), dtype=torch.int32, device=p.device)
        d2 = torch.empty((B, N, k), dtype=torch.float32, device=p.device)
        value = torch.empty((B,), dtype=torch.float32, device=p.device)
        ws_bytes = lib.fpsg_repulsion_workspace_bytes(B, N, k)
        ws = torch.empty((ws_bytes,), dtype=torch.uint8, device=p.device)
        with torch.cuda.device(p.device), _probe("repulsion_fwd", B, N, N):
            rc = lib.fpsg_repulsion_fwd(_hip.ptr(p), B, N, k, h, _hip.ptr(idx), _hip.ptr(d2), _hip.ptr(value),
                                        _hip.ptr(ws), ws_bytes, _hip.stream_of(p))
        _hip.check(rc, "fpsg_repulsion_fwd")
        if info_out is not None:
            info_out.update(idx=idx, d2=d2)
        if ctx.needs_input_grad[0]:
            ctx.save_for_backward(p, idx, d2)
            ctx.cfg = (k, h)
        return value

    @staticmethod
    def backward(ctx, g):
        if g is None:
            return None, None, None, None
        p, idx, d2 = ctx.saved_tensors
        k, h = ctx.cfg
        B, N, _ = p.shape
        g = g.reshape(B).contiguous().float()
        gx = torch.empty_like(p)
        with torch.cuda.device(p.device), _probe("repulsion_bwd", B, N, N):
            rc = _hip.load().fpsg_repulsion_bwd(_hip.ptr(p), _hip.ptr(idx), _hip.ptr(d2), _hip.ptr(g), B, N, k, h,
                                                _hip.ptr(gx), _hip.stream_of(p))
        _hip.check(rc, "fpsg_repulsion_bwd")
        return gx, None, None, None


def repulsion_loss(p: torch.Tensor, k: int = 4, h: float = 0.03, return_info: bool = False):
    """PU-Net's repulsion term ``[B]`` fp32 of the clouds ``p [B,N,3]`` (K21, HIP; the definition is in
    ``include/fpsg_hip.h``): ``(1 / (N k)) sum_i sum_{j in K(i)} -r_ij exp(-r_ij^2 / h^2)`` with ``K(i)`` the ``k`` nearest
    neighbours of point ``i`` in its own cloud (ties to the lower index; ``i`` itself never, a duplicate of ``i`` yes) and
    ``r = sqrt(max(d2, 1e-12))``.  In ``[-h / sqrt(2 e), 0]``: the more negative, the more neighbours sit about ``h /
    sqrt(2)`` away; points closer than that are pushed apart by the gradient.  ``h`` is a length in the clouds' units
    (default 0.03: clouds live in the unit ball).  It needs no ground truth and is added to whichever distance is trained.

    Differentiable in ``p`` with the lists held constant; a pair at distance 0 pushes nobody.  Bitwise the same on every
    run and independent of the batch, forward and backward (no atomics).  The call only enqueues: it can be captured.

    ``return_info=True``: returns ``(value, info)`` with ``info["idx"] [B,N,k]`` int32 and ``info["d2"] [B,N,k]`` fp32,
    nearest first.

    ``ValueError`` (before anything else) for a bad ``k`` or ``h``, a shape that is not ``[B,N,3]``, ``B = 0``, ``N < k + 1``
    and more than 16384 points.  No CPU path: a CPU tensor raises ``FpsgHipError``."""
    k, h = check_repulsion_options(k, h)
    _check_cloud(p, "repulsion_loss", REPULSION_MAX_N, lambda N: N >= k + 1, f"at least k + 1 = {k + 1}")
    _hip.dev_tensor(p, torch.float32, "p")
    info = {} if return_info else None
    out = _Repulsion.apply(p, k, h, info)
    return (out, info) if return_info else out


EXPANSION_MAX_P = 1024          # FPSG_EXPANSION_MAX_P (include/fpsg_hip.h)
EXPANSION_MAX_N = 16384         # FPSG_EXPANSION_MAX_N


def check_expansion_options(patch_size, lam):
    """``(patch_size, lam)`` of ``expansion_penalty`` as a Python int and float: ``patch_size`` an integer in 2..1024,
    ``lam`` a finite number of at least 1 (``ValueError`` naming the argument otherwise)."""
    patch_size = _integer_in(patch_size, "patch_size", 2, EXPANSION_MAX_P)
    return patch_size, _finite_number(lam, "lam", lambda v: v >= 1.0, "finite and at least 1")


class _Expansion(torch.autograd.Function):
    """K24's forward (the patches' spanning trees, mean edges and the value per cloud) and its gather backward on the
    saved trees."""

    @staticmethod
    def forward(ctx, p, P, lam, info_out):
        ctx.set_materialize_grads(False)
        B, N, _ = p.shape
        K = N // P
        lib = _hip.load()
        parent = torch.empty((B, N), dtype=torch.int32, device=p.device)
        d2 = torch.empty((B, N), dtype=torch.float32, device=p.device)
        order = torch.empty((B, N), dtype=torch.int32, device=p.device)
        mean_len = torch.empty((B, K), dtype=torch.float32, device=p.device)
        value = torch.empty((B,), dtype=torch.float32, device=p.device)
        ws_bytes = lib.fpsg_expansion_workspace_bytes(B, N, P)
        ws = torch.empty((ws_bytes,), dtype=torch.uint8, device=p.device)
        with torch.cuda.device(p.device), _probe("expansion_fwd", B, N, P):
            rc = lib.fpsg_expansion_fwd(_hip.ptr(p), B, N, P, lam, _hip.ptr(parent), _hip.ptr(d2), _hip.ptr(order),
                                        _hip.ptr(mean_len), _hip.ptr(value), _hip.ptr(ws), ws_bytes, _hip.stream_of(p))
        _hip.check(rc, "fpsg_expansion_fwd")
        if info_out is not None:
            info_out.update(parent=parent, d2=d2, order=order, mean_len=mean_len)
        if ctx.needs_input_grad[0]:
            ctx.save_for_backward(p, parent, d2, mean_len)
            ctx.cfg = (P, lam)
        return value

    @staticmethod
    def backward(ctx, g):
        if g is None:
            return None, None, None, None
        p, parent, d2, mean_len = ctx.saved_tensors
        P, lam = ctx.cfg
        B, N, _ = p.shape
        g = g.reshape(B).contiguous().float()
        gx = torch.empty_like(p)
        with torch.cuda.device(p.device), _probe("expansion_bwd", B, N, P):
            rc = _hip.load().fpsg_expansion_bwd(_hip.ptr(p), _hip.ptr(parent), _hip.ptr(d2), _hip.ptr(mean_len),
                                                _hip.ptr(g), B, N, P, lam, _hip.ptr(gx), _hip.stream_of(p))
        _hip.check(rc, "fpsg_expansion_bwd")
        return gx, None, None, None


def expansion_penalty(p: torch.Tensor, patch_size: int, lam: float = 1.5, return_info: bool = False):
    """MSN's expansion penalty ``[B]`` fp32 of the multi-patch clouds ``p [B,N,3]`` (K24, HIP; the definition is in
    ``include/fpsg_hip.h``): the cloud is ``K = N / patch_size`` patches of ``patch_size`` consecutive rows (the decoder's
    layout); every patch gets its minimum spanning tree (Prim's from its first point, ties to the lower index) and is
    charged ``(1 / (P - 1)) sum r_v`` over the tree edges with ``r_v > lam * (the tree's mean edge)``; the value is the mean
    over the patches, in ``[0, inf)``.  It is 0 where every sheet is evenly spread and grows with edges that stretch a
    patch across the shape.  It needs no ground truth and is added to whichever distance is trained.

    Differentiable in ``p`` with the trees, the penalised sets and the mean edges held constant.  Bitwise the same on
    every run and independent of the batch, forward and backward (no atomics).  The call only enqueues: it can be captured.

    ``return_info=True``: returns ``(value, info)`` with ``info["parent"]`` int32 (local index, -1 at each patch's first
    point), ``info["d2"]`` fp32 (the squared edge length), ``info["order"]`` int32 (the step at which Prim's added the point),
    all ``[B,N]``, and ``info["mean_len"] [B,K]`` fp32.

    ``ValueError`` (before anything else) for a bad ``patch_size`` or ``lam``, a shape that is not ``[B,N,3]``, ``B = 0``, ``N``
    not a positive multiple of ``patch_size`` and more than 16384 points.  No CPU path: a CPU tensor raises
    ``FpsgHipError``."""
    P, lam = check_expansion_options(patch_size, lam)
    _check_cloud(p, "expansion_penalty", EXPANSION_MAX_N, lambda N: N >= P and N % P == 0,
                 f"a positive multiple of patch_size = {P}")
    _hip.dev_tensor(p, torch.float32, "p")
    info = {} if return_info else None
    out = _Expansion.apply(p, P, lam, info)
    return (out, info) if return_info else out


UNIFORM_MAX_N = 16384           # FPSG_UNIFORM_MAX_N (include/fpsg_hip.h)
UNIFORM_MAX_T = 8               # FPSG_UNIFORM_MAX_T
UNIFORM_CAPS = (64, 128, 256)   # the retained members per ball; the largest is FPSG_UNIFORM_MAX_MEMBERS
UNIFORM_PERCENTAGES = (0.004, 0.006, 0.008, 0.010, 0.012)      # PU-GAN's, as fractions of the cloud


def check_uniform_options(percentages, radius):
    """``(percentages, radius)`` of ``uniform_loss`` as a tuple of Python floats and a float: 1..8 percentages, each a
    fraction in (0, 1], and a positive, finite radius (``ValueError`` naming the argument otherwise)."""
    if isinstance(percentages, (str, bytes, bool, numbers.Number)) or percentages is None:
        raise ValueError(f"percentages must be a sequence of 1..{UNIFORM_MAX_T} fractions in (0, 1], got {percentages!r}")
    try:
        ps = tuple(percentages)
    except TypeError:
        raise ValueError(f"percentages must be a sequence of 1..{UNIFORM_MAX_T} fractions in (0, 1], "
                         f"got {percentages!r}") from None
    if not 1 <= len(ps) <= UNIFORM_MAX_T:
        raise ValueError(f"percentages must hold 1..{UNIFORM_MAX_T} values, got {len(ps)}")
    ps = tuple(_finite_number(p, "percentages", lambda v: 0.0 < v <= 1.0, "in (0, 1]", number="numbers") for p in ps)
    return ps, _finite_number(radius, "radius", lambda v: v > 0.0, "positive and finite")


def _uniform_percent_array(percentages):
    return (ctypes.c_float * len(percentages))(*percentages)


class _Uniform(torch.autograd.Function):
    """K25's forward (ball lists, nearest neighbours inside the balls, the values) and its gather backward on the saved
    lists."""

    @staticmethod
    def forward(ctx, p, seeds, percentages, radius, cap, info_out):
        ctx.set_materialize_grads(False)
        B, N, _ = p.shape
        S, T = seeds.size(1), len(percentages)
        lib = _hip.load()
        dev = p.device
        count = torch.empty((B, T, S), dtype=torch.int32, device=dev)
        member = torch.empty((B, T, S, cap), dtype=torch.int32, device=dev)
        nn = torch.empty((B, T, S, cap), dtype=torch.int32, device=dev)
        nn_d2 = torch.empty((B, T, S, cap), dtype=torch.float32, device=dev)
        ball_value = torch.empty((B, T, S), dtype=torch.float32, device=dev)
        per_percent = torch.empty((B, T), dtype=torch.float32, device=dev)
        value = torch.empty((B,), dtype=torch.float32, device=dev)
        ws_bytes = lib.fpsg_uniform_workspace_bytes(B, N, S, T, cap)
        ws = torch.empty((ws_bytes,), dtype=torch.uint8, device=dev)
        with torch.cuda.device(dev), _probe("uniform_fwd", B, N, S):
            rc = lib.fpsg_uniform_fwd(_hip.ptr(p), _hip.ptr(seeds), B, N, S, _uniform_percent_array(percentages), T,
                                      radius, cap, _hip.ptr(count), _hip.ptr(member), _hip.ptr(nn), _hip.ptr(nn_d2),
                                      _hip.ptr(ball_value), _hip.ptr(per_percent), _hip.ptr(value), _hip.ptr(ws),
                                      ws_bytes, _hip.stream_of(p))
        _hip.check(rc, "fpsg_uniform_fwd")
        if info_out is not None:
            info_out.update(count=count, member=member, nn=nn, nn_d2=nn_d2, ball_value=ball_value,
                            per_percent=per_percent, seeds=seeds)
        if ctx.needs_input_grad[0]:
            ctx.save_for_backward(p, seeds, count, member, nn, nn_d2)
            ctx.cfg = (percentages, radius, cap)
        return value

    @staticmethod
    def backward(ctx, g):
        if g is None:
            return None, None, None, None, None, None
        p, seeds, count, member, nn, nn_d2 = ctx.saved_tensors
        percentages, radius, cap = ctx.cfg
        B, N, _ = p.shape
        S, T = seeds.size(1), len(percentages)
        g = g.reshape(B).contiguous().float()
        gx = torch.empty_like(p)
        with torch.cuda.device(p.device), _probe("uniform_bwd", B, N, S):
            rc = _hip.load().fpsg_uniform_bwd(_hip.ptr(p), _hip.ptr(seeds), _hip.ptr(count), _hip.ptr(member),
                                              _hip.ptr(nn), _hip.ptr(nn_d2), _hip.ptr(g), B, N, S, T,
                                              _uniform_percent_array(percentages), radius, cap, _hip.ptr(gx),
                                              _hip.stream_of(p))
        _hip.check(rc, "fpsg_uniform_bwd")
        return gx, None, None, None, None, None


def uniform_loss(p: torch.Tensor, percentages=UNIFORM_PERCENTAGES, radius: float = 1.0, seeds=None, n_seeds=None,
                 max_members=None, return_info: bool = False):
    """PU-GAN's uniform loss ``[B]`` fp32 of the clouds ``p [B,N,3]`` (K25, HIP; the definition is in
    ``include/fpsg_hip.h``): around every seed point one ball per percentage ``p_t``, of squared radius ``p_t radius^2``;
    a ball with ``c`` points is charged ``((c - N p_t)^2 / (N p_t)) * sum_i (d_i - dhat)^2 / dhat`` over its members, ``d_i``
    the distance to the nearest other member and ``dhat = sqrt((2 pi / sqrt 3) p_t radius^2 / c)`` the spacing of ``c``
    evenly spread points; the value is the mean over the balls.  It is 0 where every ball holds its expected share of an
    evenly spread surface of area ``pi radius^2`` and grows with balls that are too full, too empty or cluttered.  It
    needs no ground truth and is added to whichever distance is trained.

    ``seeds``: an integer tensor ``[B,S]`` of indices into the own cloud; ``None``: farthest point sampling (K16) from index
    0 with ``n_seeds`` picks, by default ``max(1, N // 20)`` (PU-GAN's 5 %).  An index outside ``[0, N)`` owns an empty ball.
    ``max_members``: the cap on the members a ball retains for the nearest-neighbour search, 64, 128 or 256; ``None``: the
    smallest of them that is at least ``2 N max(percentages)``, else 256.  The count in the first factor is never capped.

    Differentiable in ``p`` with the counts, the lists and the nearest-neighbour choices held constant; a duplicate pair
    pushes nobody.  Bitwise the same on every run and independent of the batch, forward and backward (no atomics).  The
    calls only enqueue: they can be captured.

    ``return_info=True``: returns ``(value, info)`` with ``info["count"] [B,T,S]`` int32 (the full counts),
    ``info["member"]``, ``info["nn"]`` int32 and ``info["nn_d2"]`` fp32 ``[B,T,S,cap]`` (-1, -1 and +inf behind a list),
    ``info["ball_value"] [B,T,S]``, ``info["per_percent"] [B,T]`` fp32 and ``info["seeds"] [B,S]`` int32.

    ``ValueError`` (before anything else) for bad percentages or radius, a shape that is not ``[B,N,3]``, ``B = 0``, ``N < 2``,
    more than 16384 points, bad seeds, ``n_seeds`` outside ``1..N`` or a bad ``max_members``.  No CPU path: a CPU tensor raises
    ``FpsgHipError``."""
    percentages, radius = check_uniform_options(percentages, radius)
    B, N = _check_cloud(p, "uniform_loss", UNIFORM_MAX_N, lambda N: N >= 2, "at least 2")
    if max_members is None:
        need = 2.0 * N * max(percentages)
        cap = next((c for c in UNIFORM_CAPS if c >= need), UNIFORM_CAPS[-1])
    elif isinstance(max_members, bool) or max_members not in UNIFORM_CAPS:
        raise ValueError(f"max_members must be one of {UNIFORM_CAPS} or None, got {max_members!r}")
    else:
        cap = int(max_members)
    if seeds is not None:
        if n_seeds is not None:
            raise ValueError("give seeds or n_seeds, not both")
        if (not isinstance(seeds, torch.Tensor) or seeds.is_floating_point() or seeds.is_complex()
                or seeds.dtype == torch.bool):
            raise ValueError(f"seeds must be an integer tensor, got {getattr(seeds, 'dtype', type(seeds))}")
        if seeds.dim() != 2 or seeds.size(0) != B or not 1 <= seeds.size(1) <= N:
            raise ValueError(f"seeds must have shape [B,S] with B = {B} and 1 <= S <= {N}, got {tuple(seeds.shape)}")
    else:
        if n_seeds is None:
            n_seeds = max(1, N // 20)
        if isinstance(n_seeds, bool) or not isinstance(n_seeds, numbers.Integral) or not 1 <= int(n_seeds) <= N:
            raise ValueError(f"n_seeds must be an integer from 1 to N = {N}, got {n_seeds!r}")
    _hip.dev_tensor(p, torch.float32, "p")
    if seeds is None:
        from .sampling import farthest_point_sample            # sampling.py imports from this module
        seeds = farthest_point_sample(p, int(n_seeds))
    seeds = seeds.detach().to(device=p.device, dtype=torch.int32).contiguous()
    info = {} if return_info else None
    out = _Uniform.apply(p, seeds, percentages, radius, cap, info)
    return (out, info) if return_info else out


SWD_MAX_N = 2048                # FPSG_SWD_MAX_N (include/fpsg_hip.h)
SWD_MAX_L = 1024                # FPSG_SWD_MAX_L
SWD_DIRECTION_MODES = ("random", "fixed")


def swd_directions(L: int, device=None) -> torch.Tensor:
    """The deterministic Fibonacci lattice of ``L`` unit vectors ``[L,3]`` fp32 on the sphere: ``z_i = 1 - 2 (i + 1/2) / L``,
    ``phi_i = i pi (3 - sqrt 5)``, ``(sqrt(1 - z^2) cos phi, sqrt(1 - z^2) sin phi, z)``, formed in float64 on the host and
    rounded once.  Its second moment is near isotropic (``3 / L sum theta theta^T`` within 3e-3 of the identity at
    ``L = 64``), so the sliced distance over it weighs every axis alike."""
    if isinstance(L, bool) or not isinstance(L, numbers.Integral) or not 1 <= int(L) <= SWD_MAX_L:
        raise ValueError(f"L must be an integer in 1..{SWD_MAX_L}, got {L!r}")
    i = torch.arange(int(L), dtype=torch.float64)
    z = 1.0 - 2.0 * (i + 0.5) / int(L)
    phi = i * (math.pi * (3.0 - math.sqrt(5.0)))
    rho = torch.sqrt(1.0 - z * z)
    dirs = torch.stack([rho * torch.cos(phi), rho * torch.sin(phi), z], dim=1).to(torch.float32)
    return dirs if device is None else dirs.to(device)


def check_swd_options(n_proj, directions):
    """``(n_proj, directions)`` of the sliced Wasserstein loss as a Python int and str: ``n_proj`` an integer in
    1..1024, ``directions`` ``"random"`` or ``"fixed"`` (``ValueError`` naming the argument otherwise)."""
    n_proj = _integer_in(n_proj, "n_proj", 1, SWD_MAX_L)
    if not isinstance(directions, str) or directions not in SWD_DIRECTION_MODES:
        raise ValueError(f"directions must be one of {SWD_DIRECTION_MODES}, got {directions!r}")
    return n_proj, directions


def _check_swd_inputs(p1, p2, directions):
    for name, t in (("p1", p1), ("p2", p2), ("directions", directions)):
        if not isinstance(t, torch.Tensor):
            raise ValueError(f"{name}: expected a torch.Tensor, got {type(t)}")
    if p1.dim() != 3 or p2.dim() != 3 or p1.size(2) != 3 or p2.size(2) != 3:
        raise ValueError(f"expected two [B,N,3] clouds, got {tuple(p1.shape)} and {tuple(p2.shape)}")
    if directions.dim() != 2 or directions.size(1) != 3 or not 1 <= directions.size(0) <= SWD_MAX_L:
        raise ValueError(f"directions must be [L,3] with L in 1..{SWD_MAX_L}, got {tuple(directions.shape)}")
    if p1.size(0) != p2.size(0):
        raise ValueError(f"batch mismatch: {p1.size(0)} vs {p2.size(0)}")
    if p1.size(1) != p2.size(1):
        raise ValueError(f"the sliced Wasserstein distance matches rank by rank: both clouds need the same number of "
                         f"points, got {p1.size(1)} and {p2.size(1)}")
    if p1.size(0) == 0 or p1.size(1) == 0:
        raise ValueError(f"empty point clouds are not supported (got {tuple(p1.shape)} and {tuple(p2.shape)})")
    if p1.size(1) > SWD_MAX_N:
        raise ValueError(f"swd supports at most {SWD_MAX_N} points per cloud, got {p1.size(1)}")
    for name, t in (("p1", p1), ("p2", p2), ("directions", directions)):
        if t.dtype != torch.float32:
            raise ValueError(f"{name}: expected dtype torch.float32, got {t.dtype}")
        if t.device.type != "cuda":
            raise ValueError(f"{name}: tensor is on '{t.device}'; swd runs on a ROCm GPU only (no CPU fallback)")
        if t.device != p1.device:
            raise ValueError(f"device mismatch: {name} is on {t.device}, p1 on {p1.device}")
        if not t.is_contiguous():
            raise ValueError(f"{name}: tensor must be contiguous")


def _swd_call(p1, p2, directions, need1, need2, matching):
    """One ``fpsg_swd`` call: ``(value [B], g1 | None, g2 | None, perm1 | None, perm2 | None)``."""
    B, N, _ = p1.shape
    L = directions.size(0)
    lib = _hip.load()
    dev = p1.device
    value = torch.empty((B,), dtype=torch.float32, device=dev)
    g1 = torch.empty_like(p1) if need1 else None
    g2 = torch.empty_like(p2) if need2 else None
    m1 = torch.empty((B, L, N), dtype=torch.int32, device=dev) if matching else None
    m2 = torch.empty((B, L, N), dtype=torch.int32, device=dev) if matching else None
    ws_bytes = lib.fpsg_swd_workspace_bytes(B, N, L)
    ws = torch.empty((ws_bytes,), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev), _probe("swd", B, N, N):
        rc = lib.fpsg_swd(_hip.ptr(p1), _hip.ptr(p2), _hip.ptr(directions), B, N, L, _hip.ptr(value),
                          _hip.ptr(g1) if need1 else None, _hip.ptr(g2) if need2 else None,
                          _hip.ptr(m1) if matching else None, _hip.ptr(m2) if matching else None, _hip.ptr(ws), ws_bytes,
                          _hip.stream_of(p1))
    _hip.check(rc, "fpsg_swd")
    return value, g1, g2, m1, m2


class _SwdLoss(torch.autograd.Function):
    """K22 in one call: the distance ``[B]`` and, for the inputs that need them, its gradients, cached for the backward."""

    @staticmethod
    def forward(ctx, p1, p2, directions):
        need1, need2 = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        value, g1, g2, _, _ = _swd_call(p1, p2, directions, need1, need2, False)
        ctx.grads = (g1, g2)
        return value

    @staticmethod
    def backward(ctx, g):
        g1, g2 = ctx.grads
        gc = g.reshape(-1, 1, 1)
        return (None if g1 is None else g1 * gc), (None if g2 is None else g2 * gc), None


def swd_loss(p1: torch.Tensor, p2: torch.Tensor, directions: torch.Tensor) -> torch.Tensor:
    """The sliced Wasserstein distance ``[B]`` fp32 of the clouds ``p1, p2 [B,N,3]`` (the SAME ``N``) under the directions
    ``[L,3]`` (K22, HIP; the definition is in ``include/fpsg_hip.h``): both clouds are projected on every direction, each
    projection is sorted and the points are matched rank by rank; the value is the mean squared difference over the
    ``L N`` matched keys.  Directions are used as given (``swd_directions`` gives unit vectors).

    Differentiable in ``p1`` and ``p2`` with the matchings held constant -- the exact gradient wherever the keys of a
    projection are distinct.  ONE kernel call in the forward forms the gradients of the inputs that require grad; the
    backward multiplies them by the upstream gradient.  No gradient flows to ``directions``.  Bitwise the same on every
    run and independent of the batch (no atomics); the value does not change when a cloud's points are permuted.  The call
    only enqueues: it can be captured in a graph.

    ``ValueError`` for shapes that are not ``[B,N,3]`` / ``[L,3]``, unequal ``N``, ``N`` above 2048, ``L`` above 1024, and
    tensors that are not contiguous fp32 on one ROCm device.  There is no CPU path."""
    _check_swd_inputs(p1, p2, directions)
    return _SwdLoss.apply(p1, p2, directions.detach())


@torch.no_grad()
def swd(p1: torch.Tensor, p2: torch.Tensor, n_proj: int = 128, directions: torch.Tensor | None = None,
        return_matching: bool = False):
    """``swd_loss`` as a metric, no grad: ``[B]``.  ``directions=None``: the Fibonacci lattice of ``n_proj`` directions
    (``swd_directions``); a ``[L,3]`` tensor is used as given and ``n_proj`` is ignored.  ``return_matching=True``: returns
    ``(value, perm1, perm2)`` with the orders ``[B,L,N]`` int32 of the two clouds per direction, ascending by (key, index):
    point ``perm1[b,l,r]`` of ``p1[b]`` is matched with point ``perm2[b,l,r]`` of ``p2[b]``."""
    if directions is None:
        if isinstance(n_proj, bool) or not isinstance(n_proj, numbers.Integral) or not 1 <= int(n_proj) <= SWD_MAX_L:
            raise ValueError(f"n_proj must be an integer in 1..{SWD_MAX_L}, got {n_proj!r}")
        directions = swd_directions(int(n_proj), p1.device if isinstance(p1, torch.Tensor) else None)
    p1, p2 = (t.detach() if isinstance(t, torch.Tensor) else t for t in (p1, p2))
    _check_swd_inputs(p1, p2, directions)
    value, _, _, m1, m2 = _swd_call(p1, p2, directions.detach(), False, False, bool(return_matching))
    return (value, m1, m2) if return_matching else value


def softmin(x: torch.Tensor, y: torch.Tensor, h: torch.Tensor, eps: float) -> torch.Tensor:
    """``out[b,i] = -eps * logsumexp_j(h[b,j] - |x_i - y_j|^2 / (2 eps))`` (K2b), no grad."""
    _check_clouds(x, y)
    _hip.dev_tensor(h, torch.float32, "h")
    B, N, _ = x.shape
    M = y.size(1)
    if h.shape != (B, M):
        raise ValueError(f"h must be [B,M] = {(B, M)}, got {tuple(h.shape)}")
    out = torch.empty((B, N), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device), _probe("softmin", B, N, M):
        rc = _hip.load().fpsg_softmin(_hip.ptr(x), _hip.ptr(y), _hip.ptr(h), B, N, M, float(eps),
                                      _hip.ptr(out), _hip.stream_of(x))
    _hip.check(rc, "fpsg_softmin")
    return out


@torch.no_grad()
def sinkhorn_divergence(p1: torch.Tensor, p2: torch.Tensor, blur: float = 0.05, scaling: float = 0.5,
                        diameter: float | None = None) -> torch.Tensor:
    """Debiased Sinkhorn divergence ``[B]`` between uniform clouds, cost ``|x-y|^2/2`` -- what the
    reference's ``emd_loss(sinkhorn=True)`` computes through ``geomloss.SamplesLoss()`` with its
    defaults (p=2, blur=.05, scaling=.5, debias): the symmetric Sinkhorn loop annealed over
    ``eps = diameter^2, ..., blur^2``, four soft-mins (K2b) per step, no [B,N,M] tensor.

    Forward value only (the reference uses it in evaluation, ``few_shot.py:168``; ``sinkhorn_loss`` is the differentiable
    form, same bits); the geomloss
    package is absent from the reference tree and unpinned, so parity is UNPINNED."""
    _check_clouds(p1, p2)
    B, N, _ = p1.shape
    M = p2.size(1)
    x, y = p1.detach(), p2.detach()
    if diameter is None:     # one host sync; pass `diameter` to stay asynchronous
        pts = torch.cat([x.reshape(-1, 3), y.reshape(-1, 3)])
        diameter = float((pts.amax(0) - pts.amin(0)).norm())
    eps_s = sinkhorn_epsilons(diameter, blur, scaling)
    # the loop itself (four soft-mins per schedule entry, symmetric averaging, final extrapolation)
    # runs inside the library: one launch per entry (K2b)
    import ctypes
    lib = _hip.load()
    eps_arr = (ctypes.c_float * len(eps_s))(*eps_s)
    out = torch.empty((B,), dtype=torch.float32, device=x.device)
    ws = torch.empty((lib.fpsg_sinkhorn_workspace_floats(B, N, M),), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device), _probe("sinkhorn", B, N, M):
        rc = lib.fpsg_sinkhorn_divergence(_hip.ptr(x), _hip.ptr(y), B, N, M, eps_arr, len(eps_s), _hip.ptr(out),
                                          _hip.ptr(ws), _hip.stream_of(x))
    _hip.check(rc, "fpsg_sinkhorn_divergence")
    return out


SINKHORN_TRAIN_DIAMETER = 2.0 * math.sqrt(3.0)      # the diagonal of [-1, 1]^3: tanh outputs and unit-ball references


def check_sinkhorn_option(value, name: str) -> float:
    """``blur`` / ``diameter`` of ``sinkhorn_loss`` as a Python float: a finite number > 0 (``ValueError`` naming the
    option otherwise)."""
    return _finite_number(value, name, lambda v: v > 0.0, "finite and positive", allow_bool=True)


class _SinkhornLoss(torch.autograd.Function):
    """K2b's loop with K19 as its last launch: the divergence ``[B]`` and, for the inputs that need them, its
    gradients (duals, summed clouds and schedule held constant), cached for the backward."""

    @staticmethod
    def forward(ctx, p1, p2, eps_s):
        import ctypes
        B, N, _ = p1.shape
        M = p2.size(1)
        lib = _hip.load()
        dev = p1.device
        need1, need2 = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        eps_arr = (ctypes.c_float * len(eps_s))(*eps_s)
        out = torch.empty((B,), dtype=torch.float32, device=dev)
        g1 = torch.empty_like(p1) if need1 else None
        g2 = torch.empty_like(p2) if need2 else None
        ws = torch.empty((lib.fpsg_sinkhorn_grad_workspace_floats(B, N, M),), dtype=torch.float32, device=dev)
        with torch.cuda.device(dev), _probe("sinkhorn_grad", B, N, M):
            rc = lib.fpsg_sinkhorn_divergence_grad(_hip.ptr(p1), _hip.ptr(p2), B, N, M, eps_arr, len(eps_s),
                                                   _hip.ptr(out), _hip.ptr(g1) if need1 else None,
                                                   _hip.ptr(g2) if need2 else None, _hip.ptr(ws), _hip.stream_of(p1))
        _hip.check(rc, "fpsg_sinkhorn_divergence_grad")
        ctx.grads = (g1, g2)
        return out

    @staticmethod
    def backward(ctx, gcost):
        g1, g2 = ctx.grads
        gc = gcost.reshape(-1, 1, 1)
        return (None if g1 is None else g1 * gc), (None if g2 is None else g2 * gc), None


def sinkhorn_loss(p1: torch.Tensor, p2: torch.Tensor, blur: float = 0.05, scaling: float = 0.5,
                  diameter: float | None = None) -> torch.Tensor:
    """``sinkhorn_divergence(p1, p2, blur, scaling, diameter)`` ``[B]``, bit for bit, as a differentiable loss: what
    ``geomloss.SamplesLoss()`` gives a training loop.  The gradient is geomloss's (K19, ``include/fpsg_hip.h``): the
    derivative of the final extrapolation with the duals, the summed clouds and the schedule held constant -- not a
    backward pass through the annealing loop -- formed in the call's last launch for the inputs that require grad.
    Bitwise reproducible; ``sinkhorn_loss(x, x.clone())`` has an exactly zero gradient.

    ``diameter=None``: geomloss's rule, the bounding-box diagonal of all points (one host read: not capturable).
    A float fixes the schedule: the call only enqueues and can be captured in a graph.  No gradient flows through
    the diameter either way.  Parity with the geomloss package is UNPINNED."""
    _check_clouds(p1, p2)
    blur = check_sinkhorn_option(blur, "blur")
    if diameter is None:     # one host sync; pass `diameter` to stay asynchronous
        pts = torch.cat([p1.detach().reshape(-1, 3), p2.detach().reshape(-1, 3)])
        diameter = float((pts.amax(0) - pts.amin(0)).norm())
    else:
        diameter = check_sinkhorn_option(diameter, "diameter")
    return _SinkhornLoss.apply(p1, p2, sinkhorn_epsilons(diameter, blur, scaling))


def sinkhorn_epsilons(diameter: float, blur: float = 0.05, scaling: float = 0.5):
    """geomloss' ``epsilon_schedule(p=2, diameter, blur, scaling)``."""
    import math
    eps_s = [diameter ** 2]
    e = 2 * math.log(diameter)
    while e > 2 * math.log(blur):
        eps_s.append(math.exp(e))
        e += 2 * math.log(scaling)
    eps_s.append(blur ** 2)
    return eps_s


def emd_loss(p1: torch.Tensor, p2: torch.Tensor, reduce: str = "mean", sinkhorn: bool = False):
    """Call-site mirror of ``neuralnet_pytorch.metrics.emd_loss(xyz1, xyz2, reduce, sinkhorn)`` as
    used by the reference's ``emd_wrapper`` (``src/models/utils.py:12-13``).

    ``sinkhorn=True`` (what the reference passes): the debiased Sinkhorn divergence of
    ``geomloss.SamplesLoss()`` (``sinkhorn_divergence``; forward only, as in the reference's
    evaluation).  ``sinkhorn=False``: the approximate-assignment solver (K2, the package's
    CUDA ``earth_mover_distance`` branch), differentiable.  Both third-party packages are
    absent from the reference tree and unversioned: parity is UNPINNED."""
    cost = sinkhorn_divergence(p1, p2) if sinkhorn else emd_approx(p1, p2)
    if reduce == "sum":
        return cost.sum()
    if reduce == "mean":
        return cost.mean()
    if reduce in (None, "none"):
        return cost
    raise ValueError(f"unknown reduce: {reduce}")
