"""Farthest point sampling (K16, HIP; the definition is in ``include/fpsg_hip.h``): a deterministic, well-spread
subsample of a point cloud, e.g. to report the set-level metrics at fewer points.

There is no CPU path and no PyTorch restatement here: a CPU tensor raises ``FpsgHipError``.
"""
from __future__ import annotations

import torch

from . import _hip
from .metrics import _probe

FPS_MAX_N = 16384               # FPSG_FPS_MAX_N (include/fpsg_hip.h)


def _check_start(start, B: int, N: int):
    """``None``, an int or an integer tensor ``[B]`` -> ``None`` or an int64 tensor ``[B]`` on ``start``'s device."""
    if start is None:
        return None
    if isinstance(start, torch.Tensor):
        if start.dtype not in (torch.int8, torch.int16, torch.int32, torch.int64, torch.uint8):
            raise ValueError(f"start must be an integer tensor, got {start.dtype}")
        if tuple(start.shape) != (B,):
            raise ValueError(f"start must have shape ({B},), got {tuple(start.shape)}")
        lo, hi = int(start.min()), int(start.max())
        if lo < 0 or hi >= N:
            raise ValueError(f"start indices must be in [0, {N}), got {lo}..{hi}")
        return start.detach().to(torch.int64)
    if isinstance(start, bool) or int(start) != start:
        raise ValueError(f"start must be None, an int or an integer tensor, got {start!r}")
    if not 0 <= int(start) < N:
        raise ValueError(f"start must be in [0, {N}), got {start}")
    return None if int(start) == 0 else torch.full((B,), int(start), dtype=torch.int64)


def farthest_point_sample(points: torch.Tensor, n: int, start=None, return_min_dist: bool = False):
    """Indices of ``n`` of the ``N`` points of every cloud of ``points [B,N,3]`` (fp32, on the GPU, contiguous: a
    non-contiguous tensor is refused with ``ValueError``, as by every operator here), picked so that every next pick is
    the point farthest (squared Euclidean distance, the bits of K1) from those already picked; ties go to the lowest
    index.  -> ``idx`` int64 ``[B,n]``; with ``return_min_dist`` also ``min_dist`` fp32 ``[B,n]``: the squared distance of
    pick ``t`` to the picks before it (``+inf`` for the first).

    ``start``: the first pick of every cloud -- ``None`` (index 0), an int, or an integer tensor ``[B]``.  A cloud with
    fewer than ``n`` distinct points repeats its lowest index once every point has been picked.  Bitwise the same on
    every run, whatever the batch; ``idx[:, :m]`` is the result for ``n = m``.  The input is detached (the selection is
    piecewise constant).  ``ValueError`` for bad shapes, ``n`` outside ``1..N``, ``N > 16384`` or a ``start`` out of
    range, before anything else; ``FpsgHipError`` for a CPU tensor."""
    if not isinstance(points, torch.Tensor) or points.dim() != 3 or points.size(2) != 3:
        raise ValueError(f"expected [B,N,3] points, got {tuple(getattr(points, 'shape', ()))}")
    B, N, _ = points.shape
    if B < 1 or N < 1:
        raise ValueError(f"empty batches or clouds are not supported (got {tuple(points.shape)})")
    if isinstance(n, bool) or int(n) != n or not 1 <= int(n) <= N:
        raise ValueError(f"n must be an integer from 1 to N={N}, got {n}")
    n = int(n)
    if N > FPS_MAX_N:
        raise ValueError(f"clouds of more than {FPS_MAX_N} points are not supported (got N={N})")
    start = _check_start(start, B, N)
    points = points.detach()
    _hip.dev_tensor(points, torch.float32, "points")
    dev = points.device
    start32 = None if start is None else start.to(device=dev, dtype=torch.int32).contiguous()
    idx = torch.empty((B, n), dtype=torch.int32, device=dev)
    min_dist = torch.empty((B, n), dtype=torch.float32, device=dev) if return_min_dist else None
    lib = _hip.load()
    ws_bytes = lib.fpsg_fps_workspace_bytes(B, N, n)
    ws = torch.empty((ws_bytes,), dtype=torch.uint8, device=dev) if ws_bytes else None
    with torch.cuda.device(dev), _probe("fps", B, N, n):
        rc = lib.fpsg_fps(_hip.ptr(points), B, N, n, None if start32 is None else _hip.ptr(start32), _hip.ptr(idx),
                          None if min_dist is None else _hip.ptr(min_dist), None if ws is None else _hip.ptr(ws),
                          ws_bytes, _hip.stream_of(points))
    _hip.check(rc, "fpsg_fps")
    idx = idx.long()
    return (idx, min_dist) if return_min_dist else idx


def farthest_point_subsample(points: torch.Tensor, n: int, start=None) -> torch.Tensor:
    """``points[b, farthest_point_sample(points, n, start)[b]]`` -> ``[B,n,3]``.  A gather: the gradient flows to the
    picked points, the indices carry none."""
    idx = farthest_point_sample(points, n, start)
    return torch.gather(points, 1, idx.unsqueeze(-1).expand(-1, -1, 3))
