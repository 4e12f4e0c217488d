"""Side-by-side scatter of a generated and a ground-truth cloud, as a uint8 image.

Mirrors reference ``src/models/visualization.py:9-28`` (``visualize_point_clouds``): same
figure (6x3 in, two 3-D axes, titles ``Sample: i`` / ``Ground Truth: i``, marker size 5),
returned as ``[4, H, W]`` RGBA like the reference's renderer buffer.  PNG writing uses PIL
(``imageio``, which the reference imports, is not needed).  Host-side only.

``render_reconstruction`` is the same comparison drawn on the GPU (K29, ``meshes.render_points``): shaded spheres seen by
the cameras of the conditioning views, both clouds on one scale, the generated one in the colours of the decoder's
patches (``patch_colors``).  ``render_mesh_reconstruction`` draws the generated shape as a smooth-shaded mesh instead
(K31: ``PCDecoder.decode_grid``'s vertices, ``meshes.vertex_normals``, ``meshes.render_views(face_normals=...)``).
"""
from __future__ import annotations

import numpy as np


def visualize_point_clouds(pts, gtr, idx, pert_order=(0, 1, 2)):
    import matplotlib
    matplotlib.use("Agg")
    import matplotlib.pyplot as plt

    pts = pts.detach().cpu().numpy()[:, list(pert_order)]
    gtr = gtr.detach().cpu().numpy()[:, list(pert_order)]
    fig = plt.figure(figsize=(6, 3))
    for pos, cloud, title in ((121, pts, f"Sample: {idx}"), (122, gtr, f"Ground Truth: {idx}")):
        ax = fig.add_subplot(pos, projection="3d")
        ax.set_title(title)
        ax.scatter(cloud[:, 0], cloud[:, 1], cloud[:, 2], s=5)
    fig.canvas.draw()
    img = np.asarray(fig.canvas.buffer_rgba()).copy()
    plt.close(fig)
    return np.transpose(img, (2, 0, 1))


# 16 colours for the decoder's patches, far apart in hue and of similar lightness (fixed: images stay comparable)
PATCH_PALETTE = np.array([
    [230, 25, 75], [60, 180, 75], [255, 225, 25], [0, 130, 200], [245, 130, 48], [145, 30, 180], [70, 240, 240],
    [240, 50, 230], [210, 245, 60], [250, 190, 212], [0, 128, 128], [220, 190, 255], [170, 110, 40], [128, 0, 0],
    [170, 255, 195], [0, 0, 128]], dtype=np.uint8)
GREY = (204, 204, 204)            # PhongMaterial's default colour 0.8 as a byte


def patch_colors(n_points: int, pts_per_patch: int) -> np.ndarray:
    """``[n_points, 3]`` uint8: point ``i`` takes the colour of its patch ``i // pts_per_patch`` from the 16-entry
    ``PATCH_PALETTE``, which repeats beyond 16 patches."""
    if isinstance(n_points, bool) or int(n_points) != n_points or int(n_points) < 1:
        raise ValueError(f"n_points must be a positive integer, got {n_points}")
    if isinstance(pts_per_patch, bool) or int(pts_per_patch) != pts_per_patch or int(pts_per_patch) < 1:
        raise ValueError(f"pts_per_patch must be a positive integer, got {pts_per_patch}")
    patch = np.arange(int(n_points)) // int(pts_per_patch)
    return PATCH_PALETTE[patch % len(PATCH_PALETTE)]


def render_reconstruction(syn_pc, gt_pc, pts_per_patch=None, up="z", size=192):
    """Generated against ground-truth clouds as shaded spheres (K29, ``meshes.render_points``) -> uint8
    ``[Q * size, 2 * n_views * size, 3]``: one row per query; left the generated cloud's three views (elevation 60,
    azimuths 0, 120, 240: the cameras of the conditioning views), coloured by decoder patch when ``pts_per_patch``
    divides its point count and grey otherwise; right the ground truth's views in grey.  Camera, scale and point radius
    are the same for both, so the two halves are on one scale.  ``syn_pc`` ``[Q,N,3]`` and ``gt_pc`` ``[Q,M,3]`` on a
    GPU; ``ValueError`` for anything else about their shapes."""
    import torch
    from . import meshes
    if not (isinstance(syn_pc, torch.Tensor) and isinstance(gt_pc, torch.Tensor) and syn_pc.dim() == 3 and
            gt_pc.dim() == 3 and syn_pc.size(2) == 3 and gt_pc.size(2) == 3 and syn_pc.size(0) == gt_pc.size(0)):
        raise ValueError(f"expected [Q,N,3] and [Q,M,3] clouds, got {tuple(getattr(syn_pc, 'shape', ()))} and "
                         f"{tuple(getattr(gt_pc, 'shape', ()))}")
    Q, N = syn_pc.size(0), syn_pc.size(1)
    syn_pc, gt_pc = syn_pc.detach().float().contiguous(), gt_pc.detach().float().contiguous()
    grey = torch.tensor(GREY, dtype=torch.uint8, device=syn_pc.device)
    if pts_per_patch and N % int(pts_per_patch) == 0:
        colors = torch.from_numpy(patch_colors(N, int(pts_per_patch))).to(syn_pc.device).expand(Q, N, 3).contiguous()
    else:
        colors = grey.expand(Q, N, 3).contiguous()
    halves = [meshes.render_points(syn_pc, colors=colors, size=size, up=up),
              meshes.render_points(gt_pc, colors=grey.expand(Q, gt_pc.size(1), 3).contiguous(), size=size, up=up)]
    rows = [h.permute(0, 2, 1, 3, 4).reshape(Q, h.size(2), -1, 3) for h in halves]      # [Q, H, n_views W, 3]
    sheet = torch.cat(rows, dim=2).reshape(Q * rows[0].size(1), -1, 3)
    return sheet.cpu().numpy()


def patch_materials(n_patches: int) -> list:
    """``[(name, (r, g, b))]`` for ``meshes.write_obj_mesh``: patch ``p`` is ``patch_<p>`` with the ``Kd`` of its
    ``PATCH_PALETTE`` colour (which repeats beyond 16 patches), a byte over 255 rounded to float32."""
    kd = (PATCH_PALETTE[np.arange(int(n_patches)) % len(PATCH_PALETTE)].astype(np.float64) / 255.0).astype(np.float32)
    return [(f"patch_{p}", tuple(float(c) for c in kd[p])) for p in range(int(n_patches))]


def render_mesh_reconstruction(verts, faces, gt_pc, g, up="z", size=192):
    """Generated meshes against ground-truth clouds -> uint8 ``[Q * size, 2 * 3 * size, 3]``, ``render_reconstruction``'s
    layout on one scale: left three smooth-shaded views (K31b; elevation 60, azimuths 0, 120, 240) of each generated
    mesh, its vertex normals from K31a and one ``Kd`` material per patch from ``PATCH_PALETTE``; right the ground truth
    as K29's grey spheres.  ``verts`` ``[Q, n_patches*g*g, 3]`` and ``faces`` as ``ImgPCProtoNet.reconstruct_mesh`` returns
    them, ``gt_pc`` ``[Q,M,3]``, all on one GPU; ``ValueError`` for anything else about their shapes."""
    import torch
    from . import meshes, surface
    if not (isinstance(verts, torch.Tensor) and isinstance(gt_pc, torch.Tensor) and isinstance(faces, torch.Tensor) and
            verts.dim() == 3 and gt_pc.dim() == 3 and verts.size(2) == 3 and gt_pc.size(2) == 3 and
            verts.size(0) == gt_pc.size(0) and faces.dim() == 2 and faces.size(1) == 3):
        raise ValueError(f"expected [Q,V,3] vertices, [F,3] faces and [Q,M,3] clouds, got "
                         f"{tuple(getattr(verts, 'shape', ()))}, {tuple(getattr(faces, 'shape', ()))} and "
                         f"{tuple(getattr(gt_pc, 'shape', ()))}")
    Q, V = verts.size(0), verts.size(1)
    n_patches = V // (int(g) * int(g)) if g else 0
    if n_patches < 1 or n_patches * g * g != V or faces.size(0) != n_patches * 2 * (g - 1) ** 2:
        raise ValueError(f"{V} vertices and {faces.size(0)} faces are not patches of a {g} x {g} grid")
    dev = verts.device
    verts, gt_pc = verts.detach().float().contiguous(), gt_pc.detach().float().contiguous()
    faces = faces.to(torch.int32).contiguous()
    normals = meshes.vertex_normals(verts, faces, meshes.corner_table(faces, V))        # one table for the Q meshes
    kd = np.array([c for _, c in patch_materials(n_patches)], dtype=np.float32)
    scene = meshes.RenderScene(torch.from_numpy(surface.patch_face_material(g, n_patches)).to(dev), None,
                               np.concatenate([kd, np.full((n_patches, 1), -1.0, np.float32)], axis=1),
                               np.zeros((0, 3), np.int32), None)
    index = faces.long()
    left = torch.stack([meshes.render_views(verts[q], faces, size=size, elevations_deg=60.0, azimuths_deg=(0, 120, 240),
                                            up=up, scene=scene, face_normals=normals[q][index]) for q in range(Q)])
    grey = torch.tensor(GREY, dtype=torch.uint8, device=dev)
    right = meshes.render_points(gt_pc, colors=grey.expand(Q, gt_pc.size(1), 3).contiguous(), size=size, up=up)
    rows = [h.permute(0, 2, 1, 3, 4).reshape(Q, h.size(2), -1, 3) for h in (left, right)]   # [Q, H, n_views W, 3]
    return torch.cat(rows, dim=2).reshape(Q * rows[0].size(1), -1, 3).cpu().numpy()


def write_png(path: str, hwc: np.ndarray) -> None:
    from PIL import Image
    Image.fromarray(np.ascontiguousarray(hwc).astype(np.uint8)).save(path)
