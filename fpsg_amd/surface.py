"""The generated shape as a surface: the topology of the decoder's patches on a regular grid.

The decoder (``point_cloud_net.PCDecoder``) maps points of the unit square to space, one map per patch.  Evaluated on a
regular ``g x g`` grid (``regular_grid``, ``PCDecoder.decode_grid``) and with neighbouring samples connected
(``patch_faces``), the patches are a triangle mesh.  Host code, no GPU: the arrays depend on ``g`` and the patch count
alone and are built once.  Normals (K31a), smooth-shaded views (K31b) and ``.obj`` files are in ``fpsg_amd.meshes``.
"""
from __future__ import annotations

import numpy as np

GRID_MIN, GRID_MAX = 2, 64


def _check_grid(g) -> int:
    if isinstance(g, bool) or not isinstance(g, (int, np.integer)) or not GRID_MIN <= int(g) <= GRID_MAX:
        raise ValueError(f"the grid size must be an integer from {GRID_MIN} to {GRID_MAX}, got {g!r}")
    return int(g)


def _check_patches(n_patches) -> int:
    if isinstance(n_patches, bool) or not isinstance(n_patches, (int, np.integer)) or int(n_patches) < 1:
        raise ValueError(f"n_patches must be a positive integer, got {n_patches!r}")
    return int(n_patches)


def regular_grid(g: int) -> np.ndarray:
    """float32 ``[2, g*g]``: column ``k = i*g + j`` is ``(i/(g-1), j/(g-1))``, formed in float64 and rounded once, so the
    corners are exactly 0 and 1."""
    g = _check_grid(g)
    t = np.arange(g, dtype=np.float64) / np.float64(g - 1)
    return np.stack([np.repeat(t, g), np.tile(t, g)]).astype(np.float32)


def patch_faces(g: int, n_patches: int) -> np.ndarray:
    """int32 ``[n_patches * 2 (g-1)^2, 3]``: cell ``(i, j)`` of patch ``p``, with ``k = i*g + j``, gives the faces
    ``(k, k+g, k+1)`` and ``(k+1, k+g, k+g+1)``, offset by ``p*g*g``; patch by patch, cells in row-major order.  Every
    face has the same winding in ``(u, v)``."""
    g, n_patches = _check_grid(g), _check_patches(n_patches)
    i, j = np.meshgrid(np.arange(g - 1), np.arange(g - 1), indexing="ij")
    k = (i * g + j).reshape(-1, 1)
    cell = np.concatenate([k + [0, g, 1], k + [1, g, g + 1]], axis=1).reshape(-1, 3)       # a cell's two faces together
    return (cell[None] + (np.arange(n_patches) * g * g)[:, None, None]).reshape(-1, 3).astype(np.int32)


def patch_face_material(g: int, n_patches: int) -> np.ndarray:
    """int32 ``[F]``: ``p`` for every face of patch ``p``, in ``patch_faces``' order."""
    g, n_patches = _check_grid(g), _check_patches(n_patches)
    return np.repeat(np.arange(n_patches, dtype=np.int32), 2 * (g - 1) ** 2)
