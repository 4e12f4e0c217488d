#!/usr/bin/env python3
"""ModelNet40 meshes -> the files the few-shot training reads: rendered views (K27), sampled clouds (K26), list files.

The reference prepared these with Blender (``src/preprocess/view_generator.py`` / ``phong.py``), PCL's
``pcl_mesh_sampling`` and ``src/generate_dataset.py``; here one command does it on the GPU
(``fpsg_amd.meshes``; the definitions are in ``include/fpsg_hip.h``, K26 and K27):

    python prepare_dataset.py --mesh_root ModelNet40 --img_root out/img --pc_root out/pc --output out/

walks ``<mesh_root>/<label>/<train|test>/<item>.off`` and writes ``<img_root>/<label>/<split>/<item>/<item>.<k>.png``
(``--views`` views of ``--size`` pixels, 30 degrees apart at 12 views, 60 degrees from the pole),
``<pc_root>/<label>/<split>/<item>.ply`` (``--n_points`` points, thinned from ``--oversample`` times as many by farthest
point sampling) and ``<output>/modelnet_train.txt``, ``modelnet_test.txt``, ``modelnet_files/modelnet+<label>.txt``.
Every item's random numbers come from ``--seed`` and the item's relative path, so the files do not depend on the order
of the walk or on where a run resumed; outputs that exist are kept unless ``--overwrite``.  A mesh that does not parse
or has no area is reported and skipped.  Parsing and PNG encoding run in a pool of threads beside the GPU work.
"""
from __future__ import annotations

import argparse
import concurrent.futures
import hashlib
import os

os.environ.setdefault("HIP_FORCE_DEV_KERNARG", "1")   # before the HIP runtime initialises (fpsg_amd/__init__.py)
import sys
import time

MAX_WORKERS = 16            # the pool's size is fixed, never the machine's CPU count


def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    p.add_argument("--mesh_root", required=True, help="<mesh_root>/<label>/<train|test>/<item>.off (ModelNet40's layout)")
    p.add_argument("--img_root", required=True, help="where the views go")
    p.add_argument("--pc_root", required=True, help="where the clouds go")
    p.add_argument("--output", required=True, help="where the list files go")
    p.add_argument("--n_points", type=int, default=2048)
    p.add_argument("--oversample", type=int, default=4, help="samples drawn per point kept (farthest point thinning)")
    p.add_argument("--views", type=int, default=12, help="azimuths, 360 / views degrees apart")
    p.add_argument("--size", type=int, default=600)
    p.add_argument("--ssaa", type=int, default=2, help="samples per pixel and axis")
    p.add_argument("--background", default="1,1,1", help="an image file, or r,g,b in [0,1]")
    p.add_argument("--normalize", choices=("bbox", "none"), default="bbox")
    p.add_argument("--up", choices=("z", "y"), default="z")
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--classes", nargs="*", default=None, help="labels to prepare (default: every directory)")
    p.add_argument("--train_classes", nargs="*", default=None, help="base classes of the lists (default: the reference's)")
    p.add_argument("--test_classes", nargs="*", default=None, help="novel classes of the lists (default: the reference's)")
    p.add_argument("--overwrite", action="store_true")
    p.add_argument("--workers", type=int, default=8, help=f"threads for parsing and PNG encoding, at most {MAX_WORKERS}")
    return p


def item_seed(seed: int, rel_path: str) -> int:
    """63 bits from ``--seed`` and the item's path relative to the mesh root (with ``/`` separators)."""
    h = hashlib.sha256(f"{int(seed)}:{rel_path.replace(os.sep, '/')}".encode()).digest()
    return int.from_bytes(h[:8], "little") >> 1


def find_items(mesh_root: str, classes=None):
    """-> [(label, split, item, path)] in sorted order."""
    out = []
    for label in sorted(os.listdir(mesh_root)):
        if not os.path.isdir(os.path.join(mesh_root, label)) or (classes and label not in classes):
            continue
        for split in ("train", "test"):
            d = os.path.join(mesh_root, label, split)
            if os.path.isdir(d):
                out += [(label, split, os.path.splitext(n)[0], os.path.join(d, n)) for n in sorted(os.listdir(d))
                        if n.lower().endswith(".off")]
    return out


def _background(text: str, size: int):
    import numpy as np
    try:
        rgb = tuple(float(t) for t in text.split(","))
        if len(rgb) == 3:
            return rgb
    except ValueError:
        pass
    from PIL import Image
    return np.ascontiguousarray(np.asarray(Image.open(text).convert("RGB").resize((size, size), Image.BILINEAR)))


def main(argv=None) -> int:
    opt = build_parser().parse_args(argv)
    if not 1 <= opt.workers <= MAX_WORKERS:
        raise SystemExit(f"--workers must be from 1 to {MAX_WORKERS}")
    if opt.views < 1:
        raise SystemExit("--views must be positive")
    import numpy as np
    import torch
    from PIL import Image

    from fpsg_amd import meshes
    from fpsg_amd._hip import FpsgHipError

    if not torch.cuda.is_available():
        raise FpsgHipError("prepare_dataset.py renders and samples on a ROCm GPU only (no CPU fallback); "
                           "fpsg_amd.meshes.write_modelnet_lists writes the lists of an existing tree without one")
    dev = torch.device("cuda:0")
    background = _background(opt.background, opt.size)
    azimuths = [360.0 * k / opt.views for k in range(opt.views)]
    items = find_items(opt.mesh_root, opt.classes)
    t_parse = t_sample = t_render = t_png = 0.0
    done = views_written = skipped = 0
    t0 = time.perf_counter()

    def outputs(label, split, item):
        ply = os.path.join(opt.pc_root, label, split, f"{item}.ply")
        vdir = os.path.join(opt.img_root, label, split, item)
        return ply, [os.path.join(vdir, f"{item}.{k}.png") for k in range(opt.views)]

    def parse(path):
        t = time.perf_counter()
        v, f = meshes.load_mesh(path)
        if len(f) == 0 or len(v) == 0:
            raise ValueError(f"{path}: no faces")
        return meshes.normalize_mesh(v, opt.normalize), f, time.perf_counter() - t

    def encode(images, paths, pts, ply):
        t = time.perf_counter()
        os.makedirs(os.path.dirname(paths[0]), exist_ok=True)
        os.makedirs(os.path.dirname(ply), exist_ok=True)
        for img, p in zip(images, paths):
            Image.fromarray(img).save(p)
        meshes.write_ply_points(ply, pts)
        return time.perf_counter() - t

    todo = []
    for label, split, item, path in items:
        ply, pngs = outputs(label, split, item)
        if not opt.overwrite and os.path.exists(ply) and all(os.path.exists(p) for p in pngs):
            continue
        todo.append((label, split, item, path))
    ahead = max(2, opt.workers)                              # meshes parsed ahead of the GPU
    with concurrent.futures.ThreadPoolExecutor(max_workers=opt.workers) as pool:
        parsing = {i: pool.submit(parse, todo[i][3]) for i in range(min(ahead, len(todo)))}
        encoding = []
        for i, (label, split, item, path) in enumerate(todo):
            if i + ahead < len(todo):
                parsing[i + ahead] = pool.submit(parse, todo[i + ahead][3])
            rel = os.path.relpath(path, opt.mesh_root)
            try:
                v, f, dt = parsing.pop(i).result()
                t_parse += dt
                tv, tf = torch.from_numpy(v).to(dev), torch.from_numpy(f).to(dev)
                t = time.perf_counter()
                gen = torch.Generator().manual_seed(item_seed(opt.seed, rel))
                pts, _ = meshes.sample_surface(tv, tf, opt.n_points, generator=gen, oversample=opt.oversample)
                pts = pts.cpu().numpy()
                t_sample += time.perf_counter() - t
                t = time.perf_counter()
                imgs = meshes.render_views(tv, tf, size=opt.size, azimuths_deg=azimuths, up=opt.up, ssaa=opt.ssaa,
                                           background=background).cpu().numpy()
                t_render += time.perf_counter() - t
            except (ValueError, FpsgHipError, OSError) as e:
                print(f"skipped {rel}: {e}", file=sys.stderr, flush=True)
                skipped += 1
                continue
            ply, pngs = outputs(label, split, item)
            encoding.append(pool.submit(encode, imgs, pngs, pts, ply))
            done += 1
            views_written += len(pngs)
            while len(encoding) > 2 * opt.workers:           # bounded: images wait in memory until they are written
                t_png += encoding.pop(0).result()
        for fut in encoding:
            t_png += fut.result()
    lists = meshes.write_modelnet_lists(opt.img_root, opt.pc_root, opt.output, opt.train_classes, opt.test_classes)
    total = time.perf_counter() - t0
    print(f"lists: {lists['train']} train items, {lists['test']} test items, {len(lists['classes'])} classes")
    if done:
        print(f"per item: parse {1e3 * t_parse / done:.1f} ms, K26 {1e3 * t_sample / done:.1f} ms, "
              f"K27 {1e3 * t_render / done:.1f} ms, PNG+PLY {1e3 * t_png / done:.1f} ms "
              f"(parse and PNG in {opt.workers} threads beside the GPU work)")
    print(f"prepared {done} items, {views_written} views, {total:.1f} s ({done / max(total, 1e-9):.2f} items/s); "
          f"skipped {skipped}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
