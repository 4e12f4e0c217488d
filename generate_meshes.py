#!/usr/bin/env python3
"""Generated shapes as triangle meshes: every test item's queries as ``.obj`` files and a sheet of smooth-shaded views.

    python generate_meshes.py --synthetic --n_shot 1 --n_query 1 --sequential_eval \\
        --model_path /tmp/ckpt --name 0 --eval_model model_epoch_2.pt --output /tmp/meshes --grid 16

Takes the evaluation entry point's options for data and model (``evaluate_Network.py``: ``--synthetic`` or the list
files, ``--model_path --name --eval_model``, ``--n_shot --n_query``, ``--sequential_eval``, ``--sample_up``) and builds both
with the same helpers.  The decoder's 16 patches are evaluated on a regular ``--grid`` x ``--grid`` lattice of the unit
square and neighbouring samples connected (``ImgPCProtoNet.reconstruct_mesh``).  For each test item it writes

- ``<output>/<class>/<item>_q<k>.obj`` per query ``k``: vertices, area-weighted vertex normals (K31a) and a material per
  patch, in ``<output>/<class>/patches.mtl`` (``Kd`` = the patch's colour of ``visualization.PATCH_PALETTE``);
- ``<output>/<class>/<item>.png``: one row per query, left three smooth-shaded views of the mesh (K31b), right the
  ground-truth cloud as shaded spheres (K29), on one scale -- unless ``--no_sheet`` is given.

``<item>`` is the item's position in the test loader, five digits.  Prints one summary line.  Runs on a ROCm GPU only.

With ``--metrics`` every generated mesh is also measured against its query's ground-truth cloud
(``meshes.mesh_accuracy``: the points' distance to the surface by K32, the distance of ``--metrics_samples`` surface
samples, K26, to the cloud by K1): one line per class, ``Class: <name> -- P2S: ..; S2P: ..; Mesh CD: ..; Mesh HD: ..``,
and ``<output>/metrics.json``.  With ``--normal_consistency`` each line also ends with ``; NC: ..``
(``meshes.mesh_normal_consistency``: the cloud's normals by K33 over ``--normals_k`` neighbours against the faces'
normals, on the same samples), each class row of ``metrics.json`` gets ``"normal_consistency"`` and the report
``"normals_k"``.

With ``--implicit_grid G`` (4..256; default 0: off) every query is also reconstructed as ONE closed surface from its
generated cloud -- the lattice's vertices, with normals by K33 oriented along ``--sample_up`` -- by an implicit field on
``G`` nodes per side and marching tetrahedra (K34, ``fpsg_amd.reconstruct``): ``<item>_q<k>_surface.obj`` with vertex
normals.  With ``--metrics`` a second line per class, ``Class: <name> [surface] -- P2S: ..; S2P: ..; Mesh CD: ..; Mesh
HD: ..; Watertight: <share>``, and a ``"surface"`` block in ``metrics.json``.  Without the flag nothing changes.
"""
from __future__ import annotations

import json
import os

os.environ.setdefault("HIP_FORCE_DEV_KERNARG", "1")   # before the HIP runtime initialises (fpsg_amd/__init__.py)
import sys


METRIC_KEYS = ("completeness", "accuracy", "chamfer", "hausdorff")        # meshes.mesh_accuracy's, in the line's order
METRIC_LABELS = ("P2S", "S2P", "Mesh CD", "Mesh HD")


def build_parser():
    from fpsg_amd import cli
    p = cli.few_shot_parser(evaluation=True)          # the evaluation's options; this tool's are added to the object
    p.description = __doc__.split("\n")[0]
    g = p.add_argument_group("meshes")
    g.add_argument("--output", type=str, default="meshes", metavar="DIR", help="Where the files go [default: meshes];")
    g.add_argument("--grid", type=int, default=16, metavar="G",
                   help="Samples per patch and side, 2..64: G*G vertices and 2(G-1)^2 faces per patch [default: 16];")
    g.add_argument("--max_items", type=int, default=0, metavar="N", help="Stop after N test items [default: 0 = all];")
    g.add_argument("--no_sheet", action="store_true", help="Write the .obj files only, no .png sheets;")
    g.add_argument("--metrics", action="store_true",
                   help="Measure every mesh against its ground-truth cloud (K32 + K26 + K1): a line per class and "
                        "<output>/metrics.json;")
    g.add_argument("--metrics_samples", type=int, default=None, metavar="S",
                   help="With --metrics: surface samples per mesh [default: the cloud's size];")
    g.add_argument("--normal_consistency", action="store_true",
                   help="With --metrics: also the normal consistency of mesh and cloud (K33 + K32 + K26 + K1), 'NC';")
    g.add_argument("--normals_k", type=int, default=None, metavar="K",
                   help="With --normal_consistency: neighbours per point for the cloud's normals, 3..32 [default: 16];")
    g.add_argument("--implicit_grid", type=int, default=0, metavar="G",
                   help="Also reconstruct every query's cloud as one closed surface on G nodes per side, 4..256 (K34): "
                        "<item>_q<k>_surface.obj, and with --metrics a [surface] line per class [default: 0 = off];")
    return p


def main(opt) -> int:
    import torch

    from fpsg_amd import cli, meshes, surface
    from fpsg_amd._hip import FpsgHipError
    from fpsg_amd.engine import build_model, to_device
    from fpsg_amd.visualization import patch_materials, render_mesh_reconstruction, write_png

    cli.validate(opt)
    try:
        surface.regular_grid(opt.grid)
    except ValueError as e:
        raise SystemExit(f"--grid: {e}") from None
    if opt.implicit_grid != 0 and not 4 <= opt.implicit_grid <= 256:
        raise SystemExit(f"--implicit_grid must be 0 (off) or from 4 to 256, got {opt.implicit_grid}")
    if opt.max_items < 0:
        raise SystemExit("--max_items must not be negative")
    if opt.metrics_samples is not None and not opt.metrics:
        raise SystemExit("--metrics_samples needs --metrics")
    if opt.metrics_samples is not None and opt.metrics_samples < 1:
        raise SystemExit(f"--metrics_samples must be positive, got {opt.metrics_samples}")
    if opt.normal_consistency and not opt.metrics:
        raise SystemExit("--normal_consistency needs --metrics")
    if opt.normals_k is not None and not opt.normal_consistency:
        raise SystemExit("--normals_k needs --normal_consistency (and --metrics)")
    normals_k = 16 if opt.normals_k is None else opt.normals_k
    if not 3 <= normals_k <= 32:
        raise SystemExit(f"--normals_k must be from 3 to 32, got {normals_k}")
    if not torch.cuda.is_available():
        raise FpsgHipError("generate_meshes.py runs on a ROCm GPU only (no CPU fallback)")
    n_query = opt.n_shot if opt.n_query == 0 else opt.n_query
    device = cli.pick_device(opt)
    torch.manual_seed(0)                 # the episodes' draws (supports; the order without --sequential_eval): the same files on every run
    _, ds_test = cli.build_datasets(opt, n_query, device, views=False)
    _, dl_test = cli.build_loaders(opt, ds_test, ds_test)
    model = build_model(opt)
    weights = os.path.join(opt.model_path, opt.name, opt.eval_model)
    if opt.eval_model != "NONE" or os.path.exists(weights):
        model.load_state_dict(torch.load(weights, map_location="cpu", weights_only=True))
    else:
        print("WARNING: --eval_model not given, meshing randomly initialised weights")
    model = model.to(device).eval()

    g = opt.grid
    n_patches = model.pc_decoder.num_clusters * model.pc_decoder.num_nodes
    if opt.implicit_grid and not 17 <= n_patches * g * g <= 16384:
        raise SystemExit(f"--implicit_grid takes clouds of 17 to 16384 points (K33), --grid {g} gives {n_patches * g * g}")
    materials = patch_materials(n_patches)
    face_material = surface.patch_face_material(g, n_patches)
    table = faces = None
    items, first_layer = 0, "-"
    per_class, samples = {}, opt.metrics_samples          # --metrics: class -> one row of four means per item
    surface_class = {}                                    # --implicit_grid: class -> [P2S, S2P, CD, HD, watertight] per query
    for item, sample in enumerate(dl_test):
        if opt.max_items and item >= opt.max_items:
            break
        sample = to_device(sample, device)
        verts, item_faces = model.reconstruct_mesh(sample, grid=g)
        if faces is None:                              # the topology is the same for every item: one table
            faces = item_faces
            table = meshes.corner_table(faces, verts.size(1))
            first_layer = model.pc_decoder.first_layer_path(verts.new_zeros((verts.size(0), 1)), g * g)
        normals = meshes.vertex_normals(verts, faces, table)
        folder = os.path.join(opt.output, str(sample["class"][0]))
        os.makedirs(folder, exist_ok=True)
        host_v, host_n, host_f = verts.cpu().numpy(), normals.cpu().numpy(), faces.cpu().numpy()
        for k in range(verts.size(0)):
            meshes.write_obj_mesh(os.path.join(folder, f"{item:05d}_q{k}.obj"), host_v[k], host_f, normals=host_n[k],
                                  face_material=face_material, materials=materials, mtl_name="patches.mtl")
        pcq = sample["pcq"].squeeze(0)
        clouds = pcq.reshape(-1, *pcq.shape[-2:])          # the queries' ground truth, [Q, N, 3]
        if not opt.no_sheet:
            sheet = render_mesh_reconstruction(verts, faces, clouds, g, up=getattr(opt, "sample_up", "z"))
            write_png(os.path.join(folder, f"{item:05d}.png"), sheet)
        if opt.metrics:
            samples = samples or clouds.size(1)
            draws = torch.Generator().manual_seed(item)    # on the CPU: the same numbers on every run and device
            rows = []
            for k in range(verts.size(0)):
                u = torch.rand((samples, 3), generator=draws, dtype=torch.float32)
                acc = meshes.mesh_accuracy(verts[k], faces, clouds[k], n_samples=samples, u=u)
                rows.append([acc[name] for name in METRIC_KEYS])
                if opt.normal_consistency:
                    nc = meshes.mesh_normal_consistency(verts[k], faces, clouds[k], k=normals_k, n_samples=samples, u=u)
                    rows[-1].append(nc["normal_consistency"])
            per_class.setdefault(str(sample["class"][0]), []).append([sum(col) / len(col) for col in zip(*rows)])
        if opt.implicit_grid:
            from fpsg_amd.reconstruct import reconstruct_surface
            closed = reconstruct_surface(verts, grid=opt.implicit_grid, up=getattr(opt, "sample_up", "z"), vertex_normals=True)
            draws = torch.Generator().manual_seed(item)    # a stream of its own: the lattice meshes' numbers stay
            for k, (sv, sf, sn) in enumerate(closed):
                meshes.write_obj_mesh(os.path.join(folder, f"{item:05d}_q{k}_surface.obj"), sv, sf, normals=sn)
                if opt.metrics:
                    u = torch.rand((samples, 3), generator=draws, dtype=torch.float32)
                    tight = float(meshes.mesh_topology(sf, sv.size(0))["watertight"])
                    if sf.size(0):                         # a cloud without a surface has no distances
                        acc = meshes.mesh_accuracy(sv, sf, clouds[k], n_samples=samples, u=u)
                        surface_class.setdefault(str(sample["class"][0]), []).append([acc[n] for n in METRIC_KEYS] + [tight])
                    else:
                        surface_class.setdefault(str(sample["class"][0]), []).append([float("nan")] * 4 + [tight])
        items += 1
    kernels = f"decoder first layer {first_layer}, normals K31a" + ("" if opt.no_sheet else ", views K31b + K29")
    if opt.metrics:
        report = {"grid": g, "samples": samples, "faces": n_patches * 2 * (g - 1) ** 2, "classes": {}}
        keys, labels = METRIC_KEYS, METRIC_LABELS
        if opt.normal_consistency:
            report["normals_k"] = normals_k
            keys, labels = keys + ("normal_consistency",), labels + ("NC",)
        for name in sorted(per_class):
            means = [sum(col) / len(col) for col in zip(*per_class[name])]
            report["classes"][name] = dict(zip(keys, means), items=len(per_class[name]))
            print(f"Class: {name} -- " + "; ".join(f"{label}: {v}" for label, v in zip(labels, means)))
            if opt.implicit_grid:
                rows = surface_class[name]
                means = [sum(col) / len(col) for col in zip(*rows)]
                report.setdefault("surface", {"grid": opt.implicit_grid, "classes": {}})["classes"][name] = dict(
                    zip(METRIC_KEYS + ("watertight",), means), meshes=len(rows))
                print(f"Class: {name} [surface] -- " + "; ".join(f"{label}: {v}" for label, v in
                                                                  zip(METRIC_LABELS + ("Watertight",), means)))
        os.makedirs(opt.output, exist_ok=True)
        with open(os.path.join(opt.output, "metrics.json"), "w") as f:
            json.dump(report, f, indent=1, sort_keys=True)
            f.write("\n")
        kernels += ", distances K32 + K26 + K1" + (", normals K33" if opt.normal_consistency else "")
    if opt.implicit_grid:
        kernels += f", surfaces K33 + K34 on {opt.implicit_grid}^3"
    print(f"{opt.output}: {items} items x {n_query} queries, {n_patches * g * g} vertices and "
          f"{n_patches * 2 * (g - 1) ** 2} faces per mesh ({kernels})")
    return 0


if __name__ == "__main__":
    sys.exit(main(build_parser().parse_args()))
