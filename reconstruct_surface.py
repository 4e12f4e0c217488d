#!/usr/bin/env python3
"""Point-cloud files -> closed triangle meshes as ``.obj`` files (K34, ``fpsg_amd.reconstruct.reconstruct_surface``).

    python reconstruct_surface.py --input a.npy b.ply --output surfaces --grid 64 --k 16 --orient mst --up z

``--input`` takes ``.npy`` files (``[N,3]``, or ``[B,N,3]``: B clouds) and ASCII ``.ply`` files (read with
``render_clouds.read_clouds``).  Every cloud gets oriented normals (K33: PCA over ``--k`` neighbours, the signs by
``--orient``: ``mst`` along the minimum spanning forest of the neighbour graph from the topmost point along ``--up``,
``outward`` away from the cloud's mean), an implicit signed field on ``--grid`` nodes per side whose radius is
``--radius_scale`` times the mean distance to the ``--k``-th neighbour (K34a), and the field's zero level set by marching
tetrahedra (K34b).  ``--flip`` negates the normals first: for a cloud whose orientation came out inside-out (the volume
below is negative).  Writes ``<output>/<stem>.obj`` (``<stem>_<b>.obj`` per cloud of a ``[B,N,3]`` array with B > 1) with
``v``, ``vn`` (area-weighted vertex normals, K31a) and ``f a//a b//b c//c`` records, prints one line per cloud with its
vertices, faces, whether it is watertight, and its volume, then one summary line.  Runs on a ROCm GPU only.
"""
from __future__ import annotations

import argparse
import os

os.environ.setdefault("HIP_FORCE_DEV_KERNARG", "1")   # before the HIP runtime initialises (fpsg_amd/__init__.py)
import sys


def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    p.add_argument("--input", nargs="+", required=True, help=".npy ([N,3] or [B,N,3]) or ASCII .ply files")
    p.add_argument("--output", default="surfaces", metavar="DIR", help="where the .obj files go [default: surfaces]")
    p.add_argument("--grid", type=int, default=64, metavar="G", help="nodes per side of the field, 4..256 [default: 64]")
    p.add_argument("--k", type=int, default=16, help="neighbours per point, 3..32 [default: 16]")
    p.add_argument("--radius_scale", type=float, default=1.5, metavar="S",
                   help="the weight's radius in mean distances to the k-th neighbour [default: 1.5]")
    p.add_argument("--orient", choices=("mst", "outward"), default="mst", help="the normals' signs [default: mst]")
    p.add_argument("--up", choices=("z", "y"), default="z", help="the clouds' up axis, for --orient mst [default: z]")
    p.add_argument("--flip", action="store_true", help="negate the normals: turn an inside-out surface round")
    return p


def check_options(opt) -> None:
    if not 4 <= opt.grid <= 256:
        raise SystemExit(f"--grid must be from 4 to 256, got {opt.grid}")
    if not 3 <= opt.k <= 32:
        raise SystemExit(f"--k must be from 3 to 32, got {opt.k}")
    if not 0 < opt.radius_scale < float("inf"):
        raise SystemExit(f"--radius_scale must be a positive number, got {opt.radius_scale}")


def main(argv=None) -> int:
    from render_clouds import read_clouds
    opt = build_parser().parse_args(argv)
    check_options(opt)
    try:
        clouds = [read_clouds(path) for path in opt.input]
    except (ValueError, OSError) as e:
        raise SystemExit(str(e)) from None
    for path, a in zip(opt.input, clouds):
        if a.shape[1] < opt.k + 1:
            raise SystemExit(f"{path}: {a.shape[1]} points are too few for --k {opt.k}")
    import torch

    from fpsg_amd import meshes
    from fpsg_amd._hip import FpsgHipError
    from fpsg_amd.normals import estimate_normals
    from fpsg_amd.reconstruct import reconstruct_surface

    if not torch.cuda.is_available():
        raise FpsgHipError("reconstruct_surface.py runs on a ROCm GPU only (no CPU fallback)")
    dev = torch.device("cuda:0")
    os.makedirs(opt.output, exist_ok=True)
    files = tight = 0
    for path, a in zip(opt.input, clouds):
        pts = torch.from_numpy(a).to(dev)
        normals = estimate_normals(pts, opt.k, orient=opt.orient, up=opt.up)
        if opt.flip:
            normals = -normals
        surfaces = reconstruct_surface(pts, normals, grid=opt.grid, k=opt.k, radius_scale=opt.radius_scale,
                                       vertex_normals=True)
        stem = os.path.splitext(os.path.basename(path))[0]
        for b, (verts, faces, vn) in enumerate(surfaces):
            name = f"{stem}.obj" if a.shape[0] == 1 else f"{stem}_{b}.obj"
            verts, faces = verts.cpu().numpy(), faces.cpu().numpy()
            meshes.write_obj_mesh(os.path.join(opt.output, name), verts, faces, normals=vn.cpu().numpy())
            topo = meshes.mesh_topology(faces, len(verts))
            print(f"{name}: {len(verts)} vertices, {len(faces)} faces, watertight: {'yes' if topo['watertight'] else 'no'}, "
                  f"volume: {meshes.mesh_volume(verts, faces):.6g}")
            files += 1
            tight += topo["watertight"]
    print(f"{opt.output}: {files} surfaces, {tight} watertight (grid {opt.grid}, k = {opt.k}, radius scale "
          f"{opt.radius_scale:g}, orient {opt.orient}, K33 + K34 + K31a)")
    return 0


if __name__ == "__main__":
    sys.exit(main())
