"""Surface reconstruction from point clouds (K34, ``include/fpsg_hip.h``): an implicit signed field of an oriented cloud
on a regular grid (K34a) and its zero level set as one indexed triangle mesh by marching tetrahedra (K34b).  Forward
only, on a ROCm GPU only: there is no CPU fallback."""
from __future__ import annotations

import torch

from . import _hip
from .normals import NORMALS_MAX_K, NORMALS_MAX_N, NORMALS_MIN_K, ORIENT_MODES, UP_AXES

ISO_MIN_GRID = 2                # FPSG_ISO_MIN_GRID (include/fpsg_hip.h): what the extraction takes
ISO_MAX_GRID = 256              # FPSG_ISO_MAX_GRID
ISO_MAX_NODES = 1 << 28         # FPSG_ISO_MAX_NODES, for B * G^3
FIELD_MIN_GRID = 4              # implicit_field's own: its grid keeps a radius and a cell of margin on every side


def _check_grid(grid, lowest):
    if isinstance(grid, bool) or not isinstance(grid, int) or not lowest <= grid <= ISO_MAX_GRID:
        raise ValueError(f"grid must be an integer from {lowest} to {ISO_MAX_GRID}, got {grid!r}")


def _check_oriented(points, normals):
    if not isinstance(points, torch.Tensor) or points.dim() not in (2, 3) or points.size(-1) != 3 or points.numel() == 0:
        raise ValueError(f"expected [N,3] or [B,N,3] points, got {tuple(getattr(points, 'shape', ()))}")
    if points.dtype != torch.float32:
        raise ValueError(f"points must be float32, got {points.dtype}")
    if points.size(-2) > NORMALS_MAX_N:
        raise ValueError(f"clouds of up to {NORMALS_MAX_N} points are supported, got {points.size(-2)}")
    if normals is not None:
        if not isinstance(normals, torch.Tensor) or normals.shape != points.shape:
            raise ValueError(f"normals must have the points' shape {tuple(points.shape)}, got "
                             f"{tuple(getattr(normals, 'shape', ()))}")
        if normals.dtype != torch.float32:
            raise ValueError(f"normals must be float32, got {normals.dtype}")


def _check_radius(radius, radius_scale, k, B, N):
    """-> the radius as None, a float or a [B] tensor, after the checks that need no GPU."""
    if radius is None:
        if isinstance(radius_scale, bool) or not isinstance(radius_scale, (int, float)) or not 0 < radius_scale < float("inf"):
            raise ValueError(f"radius_scale must be a positive number, got {radius_scale!r}")
        if isinstance(k, bool) or int(k) != k or not NORMALS_MIN_K <= int(k) <= NORMALS_MAX_K:
            raise ValueError(f"k must be an integer from {NORMALS_MIN_K} to {NORMALS_MAX_K}, got {k}")
        if N < int(k) + 1:
            raise ValueError(f"clouds of at least k + 1 = {int(k) + 1} points are needed for the default radius, got {N}")
        return None
    if isinstance(radius, torch.Tensor):
        if radius.numel() not in (1, B) or radius.dim() > 1:
            raise ValueError(f"a radius tensor must have 1 or {B} entries, got {tuple(radius.shape)}")
        return radius
    if isinstance(radius, bool) or not isinstance(radius, (int, float)) or not 0 < radius < float("inf"):
        raise ValueError(f"radius must be None, a positive number or a tensor, got {radius!r}")
    return float(radius)


def default_radius(points: torch.Tensor, k: int = 16, radius_scale: float = 1.5) -> torch.Tensor:
    """``radius_scale`` times the mean distance of a cloud's points to their ``k``-th nearest neighbour, per cloud of
    ``points [B,N,3]`` -> ``[B]`` float32 on the device.  The neighbour lists are K33a's, gathered on the device; nothing
    is read back.  A point without a finite distance (non-finite coordinates) does not count."""
    from .normals import point_normals
    _, _, idx = point_normals(points, int(k), 0, neighbors=True)
    kth = torch.gather(points, 1, idx[:, :, -1].long().unsqueeze(-1).expand(-1, -1, 3))
    dist = (kth - points).square().sum(-1).sqrt()
    dist = torch.where(torch.isfinite(dist), dist, torch.full_like(dist, float("nan")))
    return (torch.nanmean(dist, dim=1) * float(radius_scale)).to(torch.float32).contiguous()


def field_grid(points: torch.Tensor, radius: torch.Tensor, grid: int):
    """The cube of ``grid`` nodes per side about the bounding box's centre of each cloud of ``points [B,N,3]`` ->
    ``(origin [B,3], cell [B])`` float32 on the device.  With ``e`` the largest side of the box of the finite points:
    ``cell = (e + 2 radius) / (grid - 3)`` and ``origin = centre - cell (grid - 1) / 2``: one radius plus one cell of
    margin on every side."""
    finite = torch.isfinite(points).all(dim=-1, keepdim=True)
    lo = torch.where(finite, points, torch.full_like(points, float("inf"))).amin(dim=1)
    hi = torch.where(finite, points, torch.full_like(points, float("-inf"))).amax(dim=1)
    extent = (hi - lo).amax(dim=-1)
    cell = (extent + 2.0 * radius) / float(grid - 3)
    origin = 0.5 * (lo + hi) - (cell * (0.5 * float(grid - 1))).unsqueeze(-1)
    return origin.contiguous(), cell.contiguous()


def field_on_grid(points, normals, origin, cell, radius, grid: int, *, return_weight: bool = False):
    """K34a through the C ABI on ``points, normals [B,N,3]``, ``origin [B,3]``, ``cell [B]``, ``radius [B]`` (float32,
    contiguous, on the GPU) -> ``field [B,G,G,G]`` (and ``weight``, the sum of the weights per node)."""
    B, N, _ = points.shape
    dev = points.device
    for t, name, shape in ((points, "points", (B, N, 3)), (normals, "normals", (B, N, 3)), (origin, "origin", (B, 3)),
                           (cell, "cell", (B,)), (radius, "radius", (B,))):
        _hip.dev_tensor(t, torch.float32, name)
        if tuple(t.shape) != shape or t.device != dev:
            raise ValueError(f"{name} must be {shape} on {dev}, got {tuple(t.shape)} on {t.device}")
    _check_grid(grid, ISO_MIN_GRID)
    field = torch.empty((B, grid, grid, grid), dtype=torch.float32, device=dev)
    weight = torch.empty_like(field) if return_weight else None
    with torch.cuda.device(dev):
        rc = _hip.load().fpsg_implicit_field(_hip.ptr(points), _hip.ptr(normals), B, N, _hip.ptr(origin), _hip.ptr(cell),
                                             _hip.ptr(radius), grid, _hip.ptr(field),
                                             None if weight is None else _hip.ptr(weight), _hip.stream_of(points))
    _hip.check(rc, "fpsg_implicit_field")
    return (field, weight) if return_weight else field


def implicit_field(points: torch.Tensor, normals: torch.Tensor, *, grid: int = 64, radius=None, radius_scale: float = 1.5,
                   k: int = 16, return_weight: bool = False):
    """The signed implicit field of an oriented cloud (``points``, ``normals``: ``[N,3]`` or ``[B,N,3]`` float32 on the
    GPU) on a cube of ``grid`` (4..256) nodes per side (K34a) -> ``(field [B,G,G,G], origin [B,3], cell [B])``, with
    ``return_weight`` also ``weight [B,G,G,G]``, the sum of the weights at every node.  Node ``(i,j,k)`` lies at
    ``origin + (i,j,k) * cell``.

    The field at a node is the weighted mean of its signed distances to the points' tangent planes, the weight
    ``max(1 - d^2 / radius^2, 0)^3`` (implicit moving least squares): negative inside, positive where the normals look,
    NaN at a node no point's ball reaches.  ``radius``: a number, a ``[B]`` tensor, or None: ``radius_scale`` times the
    cloud's mean distance to its ``k``-th neighbour (K33a's lists, gathered on the device: the default path reads
    nothing back).  The grid is ``field_grid``'s.  A point with a non-finite coordinate or normal contributes nothing.

    ``radius_scale = 1.5`` is untuned on trained outputs.  On 2048 points of a sphere of radius 0.8 it gave a worst
    radial error of 0.011 (``grid=128``): tangent-plane fields swell convex shapes by roughly radius^2 times the
    curvature, so a larger radius closes holes and rounds the surface off.  Forward only: inputs are detached.  Bitwise the same on
    every run.

    ``ValueError`` for bad shapes, dtypes, ``grid``, ``radius``, ``radius_scale`` or ``k`` (3..32, fewer than ``N``),
    before any GPU work; ``FpsgHipError`` for CPU tensors."""
    _check_oriented(points, normals)
    if normals is None:
        raise ValueError("implicit_field needs normals (normals.estimate_normals, or reconstruct_surface)")
    _check_grid(grid, FIELD_MIN_GRID)
    N = points.size(-2)
    B = points.numel() // (3 * N)
    radius = _check_radius(radius, radius_scale, k, B, N)
    if B * grid ** 3 > ISO_MAX_NODES:
        raise ValueError(f"up to {ISO_MAX_NODES} nodes in all are supported, got {B} x {grid}^3")
    pts = points.detach().reshape(B, N, 3).contiguous()
    nrm = normals.detach().reshape(B, N, 3).contiguous()
    _hip.dev_tensor(pts, torch.float32, "points")
    _hip.dev_tensor(nrm, torch.float32, "normals")
    dev = pts.device
    with torch.no_grad():
        if radius is None:
            r = default_radius(pts, k, radius_scale)
        elif isinstance(radius, torch.Tensor):
            r = radius.detach().to(device=dev, dtype=torch.float32).reshape(-1).expand(B).contiguous()
        else:
            r = torch.full((B,), radius, dtype=torch.float32, device=dev)
        origin, cell = field_grid(pts, r, grid)
        out = field_on_grid(pts, nrm, origin, cell, r, grid, return_weight=return_weight)
    return (out[0], origin, cell, out[1]) if return_weight else (out, origin, cell)


def iso_counts(field: torch.Tensor):
    """K34b's first kernel on ``field [B,G,G,G]`` -> ``(node_edges, cell_tris)``, both ``[B,G^3]`` int32: every node's
    active owned edges (the vertices it emits) and the triangles of the cell whose lowest corner it is."""
    B, G = field.size(0), field.size(1)
    node_edges = torch.empty((B, G ** 3), dtype=torch.int32, device=field.device)
    cell_tris = torch.empty_like(node_edges)
    with torch.cuda.device(field.device):
        rc = _hip.load().fpsg_iso_classify(_hip.ptr(field), B, G, _hip.ptr(node_edges), _hip.ptr(cell_tris),
                                           _hip.stream_of(field))
    _hip.check(rc, "fpsg_iso_classify")
    return node_edges, cell_tris


def iso_surface_packed(field: torch.Tensor, origin: torch.Tensor, cell: torch.Tensor) -> dict:
    """K34b on ``field [B,G,G,G]``, ``origin [B,3]``, ``cell [B]`` -> the packed outputs: ``"verts" [V,3]`` float32,
    ``"faces" [F,3]`` int32 with indices local to their cloud, ``"vert_range"`` and ``"face_range"`` (lists of B + 1
    Python ints; ``"ranges" [2,B+1]`` int64: the same as the kernel wrote them), and the intermediate ``"node_edges"``,
    ``"cell_tris"`` (int32) and ``"edge_offset"``, ``"tri_offset"`` (exclusive int64 sums over all nodes).  The totals
    are read back once, with the clouds' first offsets, to size the outputs."""
    B, G = field.size(0), field.size(1)
    dev = field.device
    node_edges, cell_tris = iso_counts(field)
    edge_incl = torch.cumsum(node_edges.reshape(-1), 0, dtype=torch.int64)
    tri_incl = torch.cumsum(cell_tris.reshape(-1), 0, dtype=torch.int64)
    edge_offset = (edge_incl - node_edges.reshape(-1)).contiguous()
    tri_offset = (tri_incl - cell_tris.reshape(-1)).contiguous()
    # every cloud's first offset and the totals: the one host read, which sizes the outputs and splits them
    first = torch.stack([edge_offset[::G ** 3], tri_offset[::G ** 3]])
    vert_range, face_range = torch.cat([first, torch.stack([edge_incl[-1:], tri_incl[-1:]])], dim=1).tolist()
    n_verts, n_faces = vert_range[-1], face_range[-1]
    verts = torch.empty((n_verts, 3), dtype=torch.float32, device=dev)
    faces = torch.empty((n_faces, 3), dtype=torch.int32, device=dev)
    ranges = torch.empty((2, B + 1), dtype=torch.int64, device=dev)
    with torch.cuda.device(dev):
        rc = _hip.load().fpsg_iso_emit(_hip.ptr(field), _hip.ptr(origin), _hip.ptr(cell), B, G, _hip.ptr(edge_offset),
                                       _hip.ptr(tri_offset), n_verts, n_faces, _hip.ptr(verts) if n_verts else None,
                                       _hip.ptr(faces) if n_faces else None, _hip.ptr(ranges[0]), _hip.ptr(ranges[1]),
                                       _hip.stream_of(field))
    _hip.check(rc, "fpsg_iso_emit")
    return {"verts": verts, "faces": faces, "vert_range": vert_range, "face_range": face_range, "ranges": ranges,
            "node_edges": node_edges, "cell_tris": cell_tris, "edge_offset": edge_offset, "tri_offset": tri_offset}


def _check_field(field, origin, cell):
    if not isinstance(field, torch.Tensor) or field.dim() not in (3, 4) or field.numel() == 0 or \
            len(set(field.shape[-3:])) != 1:
        raise ValueError(f"expected a [G,G,G] or [B,G,G,G] field, got {tuple(getattr(field, 'shape', ()))}")
    if field.dtype != torch.float32:
        raise ValueError(f"field must be float32, got {field.dtype}")
    G = field.size(-1)
    B = field.size(0) if field.dim() == 4 else 1
    if not ISO_MIN_GRID <= G <= ISO_MAX_GRID or B * G ** 3 > ISO_MAX_NODES:
        raise ValueError(f"grids of {ISO_MIN_GRID} to {ISO_MAX_GRID} nodes per side and {ISO_MAX_NODES} nodes in all are "
                         f"supported, got {B} x {G}^3")
    if not isinstance(origin, torch.Tensor) or origin.numel() != 3 * B or origin.size(-1) != 3:
        raise ValueError(f"origin must be [{B},3], got {tuple(getattr(origin, 'shape', ()))}")
    if not isinstance(cell, torch.Tensor) or cell.numel() != B:
        raise ValueError(f"cell must be [{B}], got {tuple(getattr(cell, 'shape', ()))}")
    return B, G


def iso_surface(field: torch.Tensor, origin: torch.Tensor, cell: torch.Tensor) -> list:
    """The zero level set of ``field`` (``[G,G,G]`` or ``[B,G,G,G]`` float32 on the GPU, 2 <= G <= 256; node ``(i,j,k)``
    at ``origin + (i,j,k) * cell``, ``origin [B,3]``, ``cell [B]``) by marching tetrahedra on the six Kuhn tetrahedra of
    every cell (K34b) -> a list of ``(verts [V_b,3] float32, faces [F_b,3] int32)``, one per cloud.

    A node is inside where the field is negative; every triangle is counter-clockwise seen from outside.  One vertex
    per grid edge whose ends are finite and differ in side, shared by the triangles around it: where the field is finite
    the mesh is a closed, consistently oriented manifold (``meshes.mesh_topology``); NaN nodes leave a boundary.  A
    field without a sign change gives ``([0,3], [0,3])``.  Bitwise the same on every run, order included.

    ``ValueError`` for bad shapes or dtypes before any GPU work; ``FpsgHipError`` for CPU tensors."""
    B, G = _check_field(field, origin, cell)
    f = field.detach().reshape(B, G, G, G).contiguous()
    _hip.dev_tensor(f, torch.float32, "field")
    o = origin.detach().to(device=f.device, dtype=torch.float32).reshape(B, 3).contiguous()
    c = cell.detach().to(device=f.device, dtype=torch.float32).reshape(B).contiguous()
    with torch.no_grad():
        out = iso_surface_packed(f, o, c)
    vr, fr = out["vert_range"], out["face_range"]
    return [(out["verts"][vr[b]:vr[b + 1]], out["faces"][fr[b]:fr[b + 1]]) for b in range(B)]


def reconstruct_surface(points: torch.Tensor, normals=None, *, grid: int = 64, k: int = 16, orient="mst", up: str = "z",
                        radius=None, radius_scale: float = 1.5, vertex_normals: bool = False):
    """One closed, consistently oriented triangle mesh per cloud (``points``: ``[N,3]`` or ``[B,N,3]`` float32 on the
    GPU): ``implicit_field`` on ``grid`` nodes per side, then ``iso_surface``.  -> ``(verts [V,3], faces [F,3] int32)``
    for one cloud, a list of them for a batch; with ``vertex_normals`` each tuple also carries the area-weighted unit
    vertex normals ``[V,3]`` (K31a), which look outward.

    ``normals``: the cloud's oriented normals, in the points' shape; None: ``normals.estimate_normals(points, k,
    orient=orient, up=up)`` (K33; ``orient`` ``"mst"`` or ``"outward"``: an unoriented field has no inside).  ``k`` also
    sets the default ``radius`` (``implicit_field``).  Forward only.

    ``ValueError`` for bad shapes, dtypes, ``grid`` (4..256), ``k``, ``orient``, ``up``, ``radius`` or ``radius_scale``,
    before any GPU work; ``FpsgHipError`` for CPU tensors."""
    from . import meshes
    from .normals import _check_cloud, estimate_normals
    _check_oriented(points, normals)
    _check_grid(grid, FIELD_MIN_GRID)
    N = points.size(-2)
    B = points.numel() // (3 * N)
    _check_radius(radius, radius_scale, k, B, N)
    if normals is None:
        _check_cloud(points, k)
        if isinstance(orient, torch.Tensor) or orient not in ORIENT_MODES or orient == "none":
            raise ValueError(f"orient must be 'mst' or 'outward' (a surface needs oriented normals), got {orient!r}")
        if up not in UP_AXES:
            raise ValueError(f"up must be one of {', '.join(sorted(UP_AXES))}, got {up!r}")
    if B * grid ** 3 > ISO_MAX_NODES:
        raise ValueError(f"up to {ISO_MAX_NODES} nodes in all are supported, got {B} x {grid}^3")
    _hip.dev_tensor(points.detach().contiguous(), torch.float32, "points")
    if normals is None:
        normals = estimate_normals(points, k, orient=orient, up=up)
    field, origin, cell = implicit_field(points, normals, grid=grid, radius=radius, radius_scale=radius_scale, k=k)
    out = []
    for verts, faces in iso_surface(field, origin, cell):
        if not vertex_normals:
            out.append((verts, faces))
        elif faces.size(0) == 0:
            out.append((verts, faces, torch.zeros_like(verts)))
        else:
            out.append((verts, faces, meshes.vertex_normals(verts, faces)))
    return out if points.dim() == 3 else out[0]
