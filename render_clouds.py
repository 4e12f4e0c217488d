#!/usr/bin/env python3
"""Point-cloud files -> one PNG contact sheet of shaded-sphere views (K29, ``fpsg_amd.meshes.render_points``).

    python render_clouds.py --input a.npy b.ply --output sheet.png --patch 128

``--input`` takes ``.npy`` files (``[N,3]``, or ``[B,N,3]``: B clouds) and ASCII ``.ply`` files (read with
``fpsg_amd.datasets.ply_reader``).  The sheet has a row per cloud, in the order given, and a column per view
(``--azimuths`` at ``--elevation`` degrees from the pole, the cameras of the data sets' views).  Clouds are drawn as they
are, on one scale: the image's side spans 2 world units.  ``--patch N`` colours every run of N consecutive points with
one of 16 colours (``fpsg_amd.visualization.patch_colors``): the patches of a generated cloud.  Clouds of different sizes
are rendered one call each.  Runs on a ROCm GPU only.
"""
from __future__ import annotations

import argparse
import os

os.environ.setdefault("HIP_FORCE_DEV_KERNARG", "1")   # before the HIP runtime initialises (fpsg_amd/__init__.py)
import sys

MAX_POINTS = 16384          # meshes.POINTS_MAX_N


def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    p.add_argument("--input", nargs="+", required=True, help=".npy ([N,3] or [B,N,3]) or ASCII .ply files")
    p.add_argument("--output", default="clouds.png", help="the contact sheet [default: clouds.png]")
    p.add_argument("--size", type=int, default=256, help="pixels per view and side [default: 256]")
    p.add_argument("--ssaa", type=int, default=2, choices=(1, 2, 4), help="samples per pixel and axis [default: 2]")
    p.add_argument("--point_radius", type=float, default=0.02, help="the spheres' radius in world units [default: 0.02]")
    p.add_argument("--elevation", type=float, default=60.0, help="degrees from the pole [default: 60]")
    p.add_argument("--azimuths", type=float, nargs="+", default=[0.0, 120.0, 240.0], help="degrees [default: 0 120 240]")
    p.add_argument("--up", choices=("z", "y"), default="z", help="the clouds' up axis [default: z]")
    p.add_argument("--background", default="1,1,1", help="r,g,b in [0,1] [default: 1,1,1]")
    p.add_argument("--patch", type=int, default=0, metavar="N",
                   help="colour every run of N consecutive points with one of 16 colours [default: 0 = grey]")
    return p


def background_colour(text: str):
    try:
        rgb = tuple(float(t) for t in text.split(","))
    except ValueError:
        rgb = ()
    if len(rgb) != 3 or not all(0.0 <= c <= 1.0 for c in rgb):
        raise ValueError(f"--background must be r,g,b in [0,1], got {text!r}")
    return rgb


def read_clouds(path: str):
    """-> float32 ``[B,N,3]`` (B = 1 for a ``.ply`` or an ``[N,3]`` array); ``ValueError`` for anything else."""
    import numpy as np
    ext = os.path.splitext(path)[1].lower()
    if ext == ".npy":
        a = np.load(path, allow_pickle=False)
    elif ext == ".ply":
        from fpsg_amd.datasets import ply_reader
        a = np.asarray(ply_reader(path, max_verts=MAX_POINTS), dtype=np.float32)
        a = a[:, :3] if a.ndim == 2 and a.shape[1] >= 3 else a
    else:
        raise ValueError(f"{path}: expected a .npy or .ply file")
    if a.ndim == 2:
        a = a[None]
    if a.ndim != 3 or a.shape[2] != 3 or a.shape[0] < 1 or a.shape[1] < 1:
        raise ValueError(f"{path}: expected [N,3] or [B,N,3] points, got {a.shape}")
    if a.shape[1] > MAX_POINTS:
        raise ValueError(f"{path}: clouds of more than {MAX_POINTS} points are not supported (got {a.shape[1]})")
    return np.ascontiguousarray(a, dtype=np.float32)


def main(argv=None) -> int:
    opt = build_parser().parse_args(argv)
    background = background_colour(opt.background)
    if opt.patch < 0:
        raise SystemExit("--patch must not be negative")
    clouds = [read_clouds(path) for path in opt.input]
    import numpy as np
    import torch

    from fpsg_amd import meshes
    from fpsg_amd._hip import FpsgHipError
    from fpsg_amd.visualization import patch_colors, write_png

    if not torch.cuda.is_available():
        raise FpsgHipError("render_clouds.py renders on a ROCm GPU only (no CPU fallback)")
    dev = torch.device("cuda:0")
    rows = []
    for a in clouds:
        B, N = a.shape[:2]
        colors = None
        if opt.patch:
            colors = torch.from_numpy(patch_colors(N, opt.patch)).to(dev).expand(B, N, 3).contiguous()
        img = meshes.render_points(torch.from_numpy(a).to(dev), colors=colors, size=opt.size,
                                   elevations_deg=opt.elevation, azimuths_deg=opt.azimuths, up=opt.up, ssaa=opt.ssaa,
                                   point_radius=opt.point_radius, background=background)
        rows.append(img.permute(0, 2, 1, 3, 4).reshape(B * opt.size, -1, 3).cpu().numpy())   # [B H, n_views W, 3]
    sheet = np.concatenate(rows, axis=0)
    write_png(opt.output, sheet)
    print(f"{opt.output}: {sheet.shape[0] // opt.size} clouds x {len(opt.azimuths)} views of {opt.size} pixels")
    return 0


if __name__ == "__main__":
    sys.exit(main())
