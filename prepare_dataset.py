#!/usr/bin/env python3
"""Meshes -> the files the few-shot training reads: rendered views (K27 / K28), sampled clouds (K26), list files.

The reference prepared these with Blender (``src/preprocess/view_generator.py`` / ``phong.py``), PCL's
``pcl_mesh_sampling`` and ``src/generate_dataset.py``; here one command does it on the GPU
(``fpsg_amd.meshes``; the definitions are in ``include/fpsg_hip.h``, K26 to K28):

    python prepare_dataset.py --mesh_root ModelNet40 --img_root out/img --pc_root out/pc --output out/

walks ``<mesh_root>/<label>/<train|test>/<item>.off`` and writes ``<img_root>/<label>/<split>/<item>/<item>.<k>.png``
(``--views`` views of ``--size`` pixels, 30 degrees apart at 12 views, 60 degrees from the pole),
``<pc_root>/<label>/<split>/<item>.ply`` (``--n_points`` points, thinned from ``--oversample`` times as many by farthest
point sampling) and ``<output>/modelnet_train.txt``, ``modelnet_test.txt``, ``modelnet_files/modelnet+<label>.txt``.

    python prepare_dataset.py --dataset shapenet --mesh_root ShapeNetCore.v2 --pc_root out/shapenet --output out/

walks ``<mesh_root>/<synset>/<item>/models/model_normalized.obj`` and writes, where ``datasets.FewShotShapeNet`` looks
for them, ``<pc_root>/<synset>/<item>/models/npy_file.npy`` (float32 ``[n_points, 3]``) and
``<pc_root>/<synset>/<item>/models/images/<item>.<k>.png``: views in the colours of the ``.mtl``'s ``Kd`` and ``map_Kd``
textures (K28; ``--no_materials``: grey, K27).  An item is a training item iff ``item_seed(seed, path) <
train_fraction 2^63``; ``<pc_root>/<synset>_train.txt`` and ``_test.txt`` hold the split, and ``<output>/
shapenet_train.txt``, ``shapenet_test.txt`` and ``shapenet_files/shapenet+<synset>.txt`` the lists.  The defaults change
with the data set: 256 pixels, 15000 points, no thinning, no normalisation, y up.

Every item's random numbers come from ``--seed`` and the item's relative path, so the files do not depend on the order
of the walk or on where a run resumed; outputs that exist are kept unless ``--overwrite``.  A mesh that does not parse
or has no area is reported and skipped.  Parsing, texture decoding and PNG encoding run in a pool of threads beside the
GPU work.
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


DEFAULTS = {
    "modelnet": dict(n_points=2048, oversample=4, size=600, normalize="bbox", up="z"),
    "shapenet": dict(n_points=15000, oversample=1, size=256, normalize="none", up="y"),   # 256: the transform's crop
}


def build_parser(dataset: str = "modelnet") -> argparse.ArgumentParser:
    d = DEFAULTS[dataset]
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    p.add_argument("--dataset", choices=tuple(DEFAULTS), default=dataset, help="the layout of --mesh_root and of what "
                   "is written; it also sets the defaults of --n_points, --oversample, --size, --normalize and --up")
    p.add_argument("--mesh_root", required=True, help="<mesh_root>/<label>/<train|test>/<item>.off (ModelNet40's layout) "
                   "or <mesh_root>/<synset>/<item>/models/model_normalized.obj (ShapeNetCore's)")
    p.add_argument("--img_root", default=None, help="where the views go (modelnet; shapenet keeps them under --pc_root)")
    p.add_argument("--pc_root", required=True, help="where the clouds go")
    p.add_argument("--output", required=True, help="where the list files go")
    p.add_argument("--n_points", type=int, default=d["n_points"])
    p.add_argument("--oversample", type=int, default=d["oversample"],
                   help="samples drawn per point kept (farthest point thinning)")
    p.add_argument("--views", type=int, default=12, help="azimuths, 360 / views degrees apart")
    p.add_argument("--size", type=int, default=d["size"])
    p.add_argument("--ssaa", type=int, default=2, help="samples per pixel and axis")
    p.add_argument("--background", default="1,1,1", help="an image file, or r,g,b in [0,1]")
    p.add_argument("--normalize", choices=("bbox", "none"), default=d["normalize"])
    p.add_argument("--up", choices=("z", "y"), default=d["up"])
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--classes", nargs="*", default=None, help="labels to prepare (default: every directory)")
    p.add_argument("--train_classes", nargs="*", default=None, help="base classes of the lists (default: the reference's)")
    p.add_argument("--test_classes", nargs="*", default=None, help="novel classes of the lists (default: the reference's)")
    p.add_argument("--train_fraction", type=float, default=0.8, help="shapenet: the share of training items")
    p.add_argument("--max_texture", type=int, default=1024, help="shapenet: larger textures are scaled down to this side")
    p.add_argument("--no_materials", action="store_true", help="shapenet: grey views (K27), .mtl files are not read")
    p.add_argument("--overwrite", action="store_true")
    p.add_argument("--workers", type=int, default=8,
                   help=f"threads for parsing, texture decoding and PNG encoding, at most {MAX_WORKERS}")
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


def find_shapenet_items(mesh_root: str, classes=None):
    """-> [(synset, item, path)] in sorted order."""
    out = []
    for synset in sorted(os.listdir(mesh_root)):
        if not os.path.isdir(os.path.join(mesh_root, synset)) or (classes and synset not in classes):
            continue
        for item in sorted(os.listdir(os.path.join(mesh_root, synset))):
            path = os.path.join(mesh_root, synset, item, "models", "model_normalized.obj")
            if os.path.isfile(path):
                out.append((synset, item, path))
    return out


def is_train_item(seed: int, rel_path: str, train_fraction: float = 0.8) -> bool:
    """ShapeNet's split, the reference's hand-run 80/20 made reproducible: a function of the seed and the path alone."""
    return item_seed(seed, rel_path) < train_fraction * 2.0 ** 63


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
    first = argparse.ArgumentParser(add_help=False)
    first.add_argument("--dataset", choices=tuple(DEFAULTS), default="modelnet")
    parser = build_parser(first.parse_known_args(argv)[0].dataset)
    opt = parser.parse_args(argv)
    shapenet = opt.dataset == "shapenet"
    if shapenet and opt.img_root is not None:
        parser.error("--img_root is not used with --dataset shapenet: the views go under --pc_root, where the reader "
                     "looks for them")
    if not shapenet and opt.img_root is None:
        parser.error("the following arguments are required: --img_root")
    if not 1 <= opt.workers <= MAX_WORKERS:
        raise SystemExit(f"--workers must be from 1 to {MAX_WORKERS}")
    if opt.views < 1:
        raise SystemExit("--views must be positive")
    if not 0.0 <= opt.train_fraction <= 1.0:
        raise SystemExit("--train_fraction must be from 0 to 1")
    import numpy as np
    import torch
    from PIL import Image

    from fpsg_amd import meshes, sampling
    from fpsg_amd._hip import FpsgHipError

    if opt.oversample > 1 and opt.n_points * opt.oversample > sampling.FPS_MAX_N:
        raise SystemExit(f"--n_points {opt.n_points} x --oversample {opt.oversample} = {opt.n_points * opt.oversample} "
                         f"samples are more than farthest point sampling thins ({sampling.FPS_MAX_N}); lower "
                         "--oversample (1 needs no thinning) or --n_points")
    if not torch.cuda.is_available():
        raise FpsgHipError("prepare_dataset.py renders and samples on a ROCm GPU only (no CPU fallback); "
                           "fpsg_amd.meshes.write_modelnet_lists and write_shapenet_lists write the lists of an "
                           "existing tree without one")
    dev = torch.device("cuda:0")
    background = _background(opt.background, opt.size)
    azimuths = [360.0 * k / opt.views for k in range(opt.views)]
    # an item: (directory of its outputs' names, item, path of the mesh)
    if shapenet:
        items = find_shapenet_items(opt.mesh_root, opt.classes)
    else:
        items = [(os.path.join(label, split), item, path)
                 for label, split, item, path in find_items(opt.mesh_root, opt.classes)]
    with_materials = shapenet and not opt.no_materials
    t_parse = t_tex = t_sample = t_render = t_png = 0.0
    done = views_written = skipped = 0
    t0 = time.perf_counter()

    def outputs(where, item):
        if shapenet:
            models = os.path.join(opt.pc_root, where, item, "models")
            cloud, vdir = os.path.join(models, "npy_file.npy"), os.path.join(models, "images")
        else:
            cloud, vdir = os.path.join(opt.pc_root, where, f"{item}.ply"), os.path.join(opt.img_root, where, item)
        return cloud, [os.path.join(vdir, f"{item}.{k}.png") for k in range(opt.views)]

    def parse(path):
        t = time.perf_counter()
        scene = packed = None
        if with_materials:
            scene = meshes.load_obj_scene(path)
            v, f = scene.verts, scene.faces
        else:
            v, f = meshes.load_mesh(path)
        if len(f) == 0 or len(v) == 0:
            raise ValueError(f"{path}: no faces")
        v = meshes.normalize_mesh(v, opt.normalize)
        t1 = time.perf_counter()
        if with_materials:
            packed = meshes.pack_textures(scene.materials, opt.max_texture)
        return v, f, scene, packed, t1 - t, time.perf_counter() - t1

    def encode(images, paths, pts, cloud):
        t = time.perf_counter()
        os.makedirs(os.path.dirname(paths[0]), exist_ok=True)
        os.makedirs(os.path.dirname(cloud), exist_ok=True)
        for img, p in zip(images, paths):
            Image.fromarray(img).save(p)
        if shapenet:
            np.save(cloud, np.ascontiguousarray(pts, dtype=np.float32))
        else:
            meshes.write_ply_points(cloud, pts)
        return time.perf_counter() - t

    todo = []
    for where, item, path in items:
        cloud, pngs = outputs(where, item)
        if not opt.overwrite and os.path.exists(cloud) and all(os.path.exists(p) for p in pngs):
            continue
        todo.append((where, item, path))
    ahead = max(2, opt.workers)                              # meshes parsed ahead of the GPU
    with concurrent.futures.ThreadPoolExecutor(max_workers=opt.workers) as pool:
        parsing = {i: pool.submit(parse, todo[i][2]) for i in range(min(ahead, len(todo)))}
        encoding = []
        for i, (where, item, path) in enumerate(todo):
            if i + ahead < len(todo):
                parsing[i + ahead] = pool.submit(parse, todo[i + ahead][2])
            rel = os.path.relpath(path, opt.mesh_root)
            try:
                v, f, scene, packed, dt, dt_tex = parsing.pop(i).result()
                t_parse += dt
                t_tex += dt_tex
                for w in (scene.warnings + packed.warnings if scene is not None else []):
                    print(f"warning: {w}", file=sys.stderr, flush=True)
                tv, tf = torch.from_numpy(v).to(dev), torch.from_numpy(f).to(dev)
                t = time.perf_counter()
                gen = torch.Generator().manual_seed(item_seed(opt.seed, rel))
                pts, _ = meshes.sample_surface(tv, tf, opt.n_points, generator=gen, oversample=opt.oversample)
                pts = pts.cpu().numpy()
                t_sample += time.perf_counter() - t
                t = time.perf_counter()
                colours = meshes.scene_tensors(scene, packed, dev) if scene is not None else None
                imgs = meshes.render_views(tv, tf, size=opt.size, azimuths_deg=azimuths, up=opt.up, ssaa=opt.ssaa,
                                           background=background, scene=colours).cpu().numpy()
                t_render += time.perf_counter() - t
            except (ValueError, FpsgHipError, OSError) as e:
                print(f"skipped {rel}: {e}", file=sys.stderr, flush=True)
                skipped += 1
                continue
            cloud, pngs = outputs(where, item)
            encoding.append(pool.submit(encode, imgs, pngs, pts, cloud))
            done += 1
            views_written += len(pngs)
            while len(encoding) > 2 * opt.workers:           # bounded: images wait in memory until they are written
                t_png += encoding.pop(0).result()
        for fut in encoding:
            t_png += fut.result()
    if shapenet:
        split = {}
        for synset, item, path in items:
            train = is_train_item(opt.seed, os.path.relpath(path, opt.mesh_root), opt.train_fraction)
            split.setdefault((synset, "train" if train else "test"), []).append(item)
        os.makedirs(opt.pc_root, exist_ok=True)
        for synset in sorted({s for s, _ in split}):
            for part in ("train", "test"):
                with open(os.path.join(opt.pc_root, f"{synset}_{part}.txt"), "w") as fh:
                    fh.write("".join(f"{item}\n" for item in split.get((synset, part), [])))
        lists = meshes.write_shapenet_lists(opt.pc_root, opt.output, opt.train_classes, opt.test_classes)
    else:
        lists = meshes.write_modelnet_lists(opt.img_root, opt.pc_root, opt.output, opt.train_classes, opt.test_classes)
    total = time.perf_counter() - t0
    print(f"lists: {lists['train']} train items, {lists['test']} test items, {len(lists['classes'])} classes")
    if done:
        tex = f"textures {1e3 * t_tex / done:.1f} ms, " if with_materials else ""
        cloud_kind = "NPY" if shapenet else "PLY"
        print(f"per item: parse {1e3 * t_parse / done:.1f} ms, {tex}K26 {1e3 * t_sample / done:.1f} ms, "
              f"{'K28' if with_materials else 'K27'} {1e3 * t_render / done:.1f} ms, "
              f"PNG+{cloud_kind} {1e3 * t_png / done:.1f} ms "
              f"(parse and PNG in {opt.workers} threads beside the GPU work)")
    print(f"prepared {done} items, {views_written} views, {total:.1f} s ({done / max(total, 1e-9):.2f} items/s); "
          f"skipped {skipped}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
