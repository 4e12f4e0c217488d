"""Normals of bare point clouds (K33, ``include/fpsg_hip.h``): k-nearest-neighbour PCA, a sign per point, and the
normal consistency of two clouds.  Forward only, on a ROCm GPU only: there is no CPU fallback."""
from __future__ import annotations

import torch

from . import _hip

NORMALS_MIN_K = 3               # FPSG_NORMALS_POINTS_MIN_K (include/fpsg_hip.h)
NORMALS_MAX_K = 32              # FPSG_NORMALS_POINTS_MAX_K
NORMALS_MAX_N = 16384           # FPSG_NORMALS_POINTS_MAX_N
NORMALS_MAX_B = 65535           # FPSG_NORMALS_POINTS_MAX_B
ORIENT_MODES = ("mst", "outward", "none")
UP_AXES = {"x": 0, "y": 1, "z": 2}


def _check_cloud(points, k):
    if not isinstance(points, torch.Tensor) or points.dim() not in (2, 3) or points.size(-1) != 3:
        raise ValueError(f"expected [N,3] or [B,N,3] points, got {tuple(getattr(points, 'shape', ()))}")
    if points.dtype != torch.float32:
        raise ValueError(f"points must be float32, got {points.dtype}")
    if isinstance(k, bool) or int(k) != k or not NORMALS_MIN_K <= int(k) <= NORMALS_MAX_K:
        raise ValueError(f"k must be an integer from {NORMALS_MIN_K} to {NORMALS_MAX_K}, got {k}")
    k = int(k)
    B = points.size(0) if points.dim() == 3 else 1
    N = points.size(-2)
    if B < 1 or B > NORMALS_MAX_B:
        raise ValueError(f"1 to {NORMALS_MAX_B} clouds are supported, got {B}")
    if N < k + 1 or N > NORMALS_MAX_N:
        raise ValueError(f"clouds of k + 1 = {k + 1} to {NORMALS_MAX_N} points are supported, got {N}")
    return B, N, k


def point_normals(pts: torch.Tensor, k: int, sign_mode: int = 0, ref=None, *, variation: bool = False,
                  neighbors: bool = False):
    """K33a through the C ABI on ``pts [B,N,3]``: ``(normals [B,N,3], variation [B,N] | None, nbr_idx [B,N,k] int32 |
    None)``.  ``sign_mode`` 0: canonical; 1 / 2: toward / away from ``ref [B,3]``."""
    B, N, _ = pts.shape
    dev = pts.device
    lib = _hip.load()
    ws_bytes = lib.fpsg_point_normals_workspace_bytes(B, N, k)
    if ws_bytes == 0:
        raise ValueError(f"unsupported shape (B={B}, N={N}, k={k})")
    ws = torch.empty((ws_bytes // 4,), dtype=torch.int32, device=dev)
    normals = torch.empty((B, N, 3), dtype=torch.float32, device=dev)
    var = torch.empty((B, N), dtype=torch.float32, device=dev) if variation else None
    idx = torch.empty((B, N, k), dtype=torch.int32, device=dev) if neighbors else None
    with torch.cuda.device(dev):
        rc = lib.fpsg_point_normals(_hip.ptr(pts), B, N, k, sign_mode, None if ref is None else _hip.ptr(ref),
                                    _hip.ptr(normals), None if var is None else _hip.ptr(var),
                                    None if idx is None else _hip.ptr(idx), _hip.ptr(ws), ws.numel() * 4,
                                    _hip.stream_of(pts))
    _hip.check(rc, "fpsg_point_normals")
    return normals, var, idx


def orient_normals(pts: torch.Tensor, normals: torch.Tensor, nbr_idx: torch.Tensor, axis: int = 2, *,
                   parents: bool = False):
    """K33b through the C ABI: the normals ``[B,N,3]`` with their signs propagated along the minimum spanning forest of
    the neighbour graph ``nbr_idx [B,N,k]`` int32 -> ``(normals_out, parent [B,N] int32 | None)``."""
    B, N, k = nbr_idx.shape
    dev = pts.device
    for t, dt, name in ((pts, torch.float32, "points"), (normals, torch.float32, "normals"), (nbr_idx, torch.int32, "nbr_idx")):
        _hip.dev_tensor(t, dt, name)
    if tuple(pts.shape) != (B, N, 3) or tuple(normals.shape) != (B, N, 3):
        raise ValueError(f"points {tuple(pts.shape)}, normals {tuple(normals.shape)} and lists {tuple(nbr_idx.shape)} disagree")
    lib = _hip.load()
    ws_bytes = lib.fpsg_point_normals_orient_workspace_bytes(B, N, k)
    if ws_bytes == 0:
        raise ValueError(f"unsupported shape (B={B}, N={N}, k={k})")
    ws = torch.empty((ws_bytes // 4,), dtype=torch.int32, device=dev)
    out = torch.empty((B, N, 3), dtype=torch.float32, device=dev)
    parent = torch.empty((B, N), dtype=torch.int32, device=dev) if parents else None
    with torch.cuda.device(dev):
        rc = lib.fpsg_point_normals_orient(_hip.ptr(pts), _hip.ptr(normals), _hip.ptr(nbr_idx), B, N, k, axis,
                                           _hip.ptr(out), None if parent is None else _hip.ptr(parent), _hip.ptr(ws),
                                           ws.numel() * 4, _hip.stream_of(pts))
    _hip.check(rc, "fpsg_point_normals_orient")
    return out, parent


def estimate_normals(points: torch.Tensor, k: int = 16, *, orient="mst", up: str = "z", return_variation: bool = False,
                     return_neighbors: bool = False):
    """Unit normals of ``points`` (``[N,3]`` or ``[B,N,3]`` float32 on the GPU) by PCA over each point's ``k`` nearest
    neighbours and itself (K33a), in the points' shape.  A point whose neighbourhood has no extent gets (0,0,0).

    ``orient`` picks the signs: ``"none"``: the component of largest magnitude is positive (a function of the cloud
    alone); ``"outward"``: away from the cloud's mean; ``"mst"``: propagated along the minimum spanning forest of the
    neighbour graph (K33b), every tree started at its topmost point along ``up`` (``"z"``, ``"y"`` or ``"x"``) with the
    normal looking up; a ``[3]`` or ``[B,3]`` tensor: toward that viewpoint.

    With ``return_variation`` also Pauly's surface variation ``lambda0 / (lambda0 + lambda1 + lambda2)`` (``[N]`` or
    ``[B,N]``, in [0, 1/3]); with ``return_neighbors`` also the lists (``[N,k]`` or ``[B,N,k]`` int64, nearest first,
    ties to the lower index): a tuple in that order.  Forward only: inputs are detached.  Bitwise the same on every run.

    ``ValueError`` for bad shapes, ``k`` outside 3..32, clouds of fewer than ``k + 1`` or more than 16384 points, an
    unknown ``orient`` or ``up``, before any GPU work; ``FpsgHipError`` for CPU tensors."""
    B, N, k = _check_cloud(points, k)
    viewpoint = None
    if isinstance(orient, torch.Tensor):
        if tuple(orient.shape) not in ((3,), (B, 3)):
            raise ValueError(f"a viewpoint must have shape (3,) or ({B}, 3), got {tuple(orient.shape)}")
        viewpoint = orient
    elif orient not in ORIENT_MODES:
        raise ValueError(f"orient must be one of {', '.join(ORIENT_MODES)} or a viewpoint tensor, got {orient!r}")
    if up not in UP_AXES:
        raise ValueError(f"up must be one of {', '.join(sorted(UP_AXES))}, got {up!r}")
    batched = points.dim() == 3
    pts = points.detach().reshape(B, N, 3).contiguous()
    _hip.dev_tensor(pts, torch.float32, "points")
    dev = pts.device
    with torch.no_grad():
        if viewpoint is not None:
            ref = viewpoint.detach().to(device=dev, dtype=torch.float32).reshape(-1, 3).expand(B, 3).contiguous()
            normals, var, idx = point_normals(pts, k, 1, ref, variation=return_variation, neighbors=return_neighbors)
        elif orient == "outward":
            ref = pts.mean(dim=1).contiguous()
            normals, var, idx = point_normals(pts, k, 2, ref, variation=return_variation, neighbors=return_neighbors)
        elif orient == "none":
            normals, var, idx = point_normals(pts, k, 0, variation=return_variation, neighbors=return_neighbors)
        else:
            normals, var, idx = point_normals(pts, k, 0, variation=return_variation, neighbors=True)
            normals, _ = orient_normals(pts, normals, idx, UP_AXES[up])
    out = [normals if batched else normals[0]]
    if return_variation:
        out.append(var if batched else var[0])
    if return_neighbors:
        out.append(idx.long() if batched else idx[0].long())
    return out[0] if len(out) == 1 else tuple(out)


def _unit_rows(p, n, name):
    if not isinstance(p, torch.Tensor) or p.dim() not in (2, 3) or p.size(-1) != 3 or p.numel() == 0:
        raise ValueError(f"expected [N,3] or [B,N,3] points for {name}, got {tuple(getattr(p, 'shape', ()))}")
    if not isinstance(n, torch.Tensor) or n.shape != p.shape:
        raise ValueError(f"the normals of {name} must have the points' shape {tuple(p.shape)}, got "
                         f"{tuple(getattr(n, 'shape', ()))}")
    if p.dtype != torch.float32 or n.dtype != torch.float32:
        raise ValueError(f"points and normals of {name} must be float32, got {p.dtype} and {n.dtype}")
    return p.detach().reshape(-1, p.size(-2), 3).contiguous(), n.detach().reshape(-1, p.size(-2), 3).contiguous()


def normal_consistency(p1: torch.Tensor, n1: torch.Tensor, p2: torch.Tensor, n2: torch.Tensor) -> dict:
    """The normal consistency of two clouds with normals (``[N,3]`` / ``[M,3]``, or batches ``[B,N,3]`` / ``[B,M,3]``,
    float32 on the GPU) -> Python floats:

    - ``"forward"``: the mean over ``p1`` of ``|n1 . n2[nearest point of p2]|`` (the neighbours by K1);
    - ``"backward"``: the same from ``p2`` to ``p1``;
    - ``"normal_consistency"``: their mean.

    Signs do not count.  The means are taken in float64 on the device and come back in one read.
    ``ValueError`` for bad shapes or dtypes; ``FpsgHipError`` for CPU tensors."""
    from .metrics import nearest_rows
    a, na = _unit_rows(p1, n1, "p1")
    b, nb = _unit_rows(p2, n2, "p2")
    if a.size(0) != b.size(0):
        raise ValueError(f"{a.size(0)} clouds against {b.size(0)}")
    _hip.dev_tensor(a, torch.float32, "p1")
    for t, name in ((na, "n1"), (b, "p2"), (nb, "n2")):
        _hip.dev_tensor(t, torch.float32, name)
    _, _, idx1, idx2 = nearest_rows(a, b)
    with torch.no_grad():
        na64, nb64 = na.to(torch.float64), nb.to(torch.float64)
        near1 = torch.gather(nb64, 1, idx1.long().unsqueeze(-1).expand(-1, -1, 3))
        near2 = torch.gather(na64, 1, idx2.long().unsqueeze(-1).expand(-1, -1, 3))
        fwd = (na64 * near1).sum(-1).abs().mean()
        bwd = (nb64 * near2).sum(-1).abs().mean()
        values = torch.stack([fwd, bwd, 0.5 * (fwd + bwd)]).tolist()
    return dict(zip(("forward", "backward", "normal_consistency"), values))
