#!/usr/bin/env python3
"""Point-cloud files -> ASCII ``.ply`` files with oriented normals (K33, ``fpsg_amd.normals.estimate_normals``).

    python estimate_normals.py --input a.npy b.ply --output normals --k 16 --orient mst --up z

``--input`` takes ``.npy`` files (``[N,3]``, or ``[B,N,3]``: B clouds) and ASCII ``.ply`` files (read with
``render_clouds.read_clouds``).  Every cloud gets the PCA normal of each point's ``--k`` nearest neighbours; ``--orient``
picks the signs: ``mst`` propagates them along the minimum spanning forest of the neighbour graph from the topmost point
along ``--up`` (what a Poisson reconstruction wants), ``outward`` points them away from the cloud's mean, ``none`` leaves
the component of largest magnitude positive.  Writes ``<output>/<stem>.ply`` (``<stem>_<b>.ply`` per cloud of a
``[B,N,3]`` array with B > 1) with ``x y z nx ny nz`` per vertex and prints one summary line.  Runs on a ROCm GPU only.
"""
from __future__ import annotations

import argparse
import os

os.environ.setdefault("HIP_FORCE_DEV_KERNARG", "1")   # before the HIP runtime initialises (fpsg_amd/__init__.py)
import sys


def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    p.add_argument("--input", nargs="+", required=True, help=".npy ([N,3] or [B,N,3]) or ASCII .ply files")
    p.add_argument("--output", default="normals", metavar="DIR", help="where the .ply files go [default: normals]")
    p.add_argument("--k", type=int, default=16, help="neighbours per point, 3..32 [default: 16]")
    p.add_argument("--orient", choices=("mst", "outward", "none"), default="mst", help="the signs [default: mst]")
    p.add_argument("--up", choices=("z", "y"), default="z", help="the clouds' up axis, for --orient mst [default: z]")
    return p


def main(argv=None) -> int:
    from render_clouds import read_clouds
    opt = build_parser().parse_args(argv)
    if not 3 <= opt.k <= 32:
        raise SystemExit(f"--k must be from 3 to 32, got {opt.k}")
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

    if not torch.cuda.is_available():
        raise FpsgHipError("estimate_normals.py runs on a ROCm GPU only (no CPU fallback)")
    dev = torch.device("cuda:0")
    os.makedirs(opt.output, exist_ok=True)
    files = points = 0
    for path, a in zip(opt.input, clouds):
        normals = estimate_normals(torch.from_numpy(a).to(dev), opt.k, orient=opt.orient, up=opt.up).cpu().numpy()
        stem = os.path.splitext(os.path.basename(path))[0]
        for b in range(a.shape[0]):
            name = f"{stem}.ply" if a.shape[0] == 1 else f"{stem}_{b}.ply"
            meshes.write_ply_points(os.path.join(opt.output, name), a[b], normals[b])
            files += 1
            points += a.shape[1]
    print(f"{opt.output}: {files} clouds, {points} points with normals (k = {opt.k}, orient {opt.orient}, K33)")
    return 0


if __name__ == "__main__":
    sys.exit(main())
