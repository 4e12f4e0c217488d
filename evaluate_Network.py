#!/usr/bin/env python3
"""Evaluation entry point: per-class Chamfer and EMD of a trained model.

Same command line and report lines as reference ``src/evaluate_Network.py`` (``main :65-123``):
loads ``<model_path>/<name>/<eval_model>``, runs ``ImgPCProtoNet._return_reconstruction`` on
every test episode (HIP Chamfer K1 + the HIP Sinkhorn divergence K2b, the form ``emd_wrapper`` calls) and prints
``Class: <c> -- Rec CD: <mean>; Rec EMD: <mean>`` (``--exact_emd``: followed by ``; Exact EMD: <mean>``, the
exact transport distance of K12 divided by n_query like the other two; ``--fscore TAU [TAU ...]``: then
``; F@<tau>: <mean>`` for every threshold in the order given, ``<tau>`` as ``repr(float)``, and once ``; HD: <mean>``: the
F-score of the reconstructions at those distances and the Hausdorff distance, K17's counts and maxima over K1's minima,
averaged over an item's queries and then over the class's items like ``Rec CD``; ``--dcd [ALPHA]``: then
``; DCD: <mean>``, the density-aware Chamfer distance of the reconstructions (K18 over K1's minima and indices, in
[0, 1]), averaged the same way; ``--set_metrics``: then
``; MMD-CD: <v>; COV-CD: <v>; 1-NNA-CD: <v>``, the set-level generation metrics of ``fpsg_amd.set_metrics`` over all
the class's generated and reference query clouds, from K13's Chamfer matrices; ``--set_metrics_emd``: then
``; MMD-EMD: <v>; COV-EMD: <v>; 1-NNA-EMD: <v>``, the same under the exact EMD from K14's matrices, followed by
``; EMD-uncertified: <cov>/<nna>`` when some nearest-neighbour decisions are not certified by the EMD bounds;
``--set_metrics_points N``: the clouds of those two are first reduced to ``N`` points each by farthest point sampling from
index 0 (K16) and their six labels read ``MMD-CD@N``, ..., ``1-NNA-EMD@N``; every other column stays on the full clouds;
``--jsd``: last, ``; JSD: <v>``, the Jensen-Shannon divergence between the voxel-occupancy distributions of the class's
generated and reference query clouds, from K15's grids, accumulated as the items arrive).  With ``--npy_folder`` the generated and
ground-truth clouds (+ a side-by-side PNG) of every item are dumped instead, which is the
reference's commented-out "OPTION 2" (``:111``).

    python evaluate_Network.py --synthetic --n_shot 1 --n_query 1 --sequential_eval \
        --model_path /tmp/ckpt --name 0 --eval_model model_epoch_2.pt
"""
from __future__ import annotations

import os

os.environ.setdefault("HIP_FORCE_DEV_KERNARG", "1")   # before the HIP runtime initialises (fpsg_amd/__init__.py)
import statistics
from collections import defaultdict

import torch

from fpsg_amd import cli
from fpsg_amd.engine import EvalItem, build_model, to_device


def main(opt):
    cli.validate(opt)
    n_query = opt.n_shot if opt.n_query == 0 else opt.n_query
    device = cli.pick_device(opt)
    checkpoint_path = os.path.join(opt.model_path, opt.name)
    os.makedirs(os.path.join(checkpoint_path, "images"), exist_ok=True)

    _, ds_test = cli.build_datasets(opt, n_query, device)
    _, dl_test = cli.build_loaders(opt, ds_test, ds_test)

    model = build_model(opt)
    weights = os.path.join(checkpoint_path, opt.eval_model)
    if opt.eval_model != "NONE" or os.path.exists(weights):
        model.load_state_dict(torch.load(weights, map_location="cpu", weights_only=True))
    else:
        print("WARNING: --eval_model not given, evaluating randomly initialised weights")
    model = model.to(device).eval()

    per_class_cd, per_class_emd = defaultdict(list), defaultdict(list)
    exact = bool(getattr(opt, "exact_emd", False))
    per_class_exact = defaultdict(list)
    taus = getattr(opt, "fscore", None)
    taus = None if taus is None else tuple(taus)
    per_class_f = defaultdict(list)                     # per class and item: [fscore [T], precision [T], recall [T], hd]
    dcd_alpha = getattr(opt, "dcd", None)
    per_class_dcd = defaultdict(list)
    sets = bool(getattr(opt, "set_metrics", False))
    sets_emd = bool(getattr(opt, "set_metrics_emd", False))
    per_class_gen, per_class_ref = defaultdict(list), defaultdict(list)
    set_points = getattr(opt, "set_metrics_points", None)
    at = "" if set_points is None else f"@{set_points}"   # the labels of reduced set metrics say so
    want_jsd = bool(getattr(opt, "jsd", False))
    grid_gen, grid_ref = {}, {}                         # per class: the two occupancy grids, accumulated per item
    # the weights do not change while evaluating: transformed filters, stacked decoder weights and BatchNorm coefficients
    # are made once, not per item; on a GPU the item in front of the EMD is replayed as a hipGraph (engine.EvalItem)
    with EvalItem(model, exact_emd=exact, return_clouds=sets or sets_emd or want_jsd, fscore=taus,
                  dcd=dcd_alpha) as run_item:
        for item, sample in enumerate(dl_test):
            sample = to_device(sample, device)
            if getattr(opt, "npy_folder", ""):
                os.makedirs(opt.npy_folder, exist_ok=True)
                model.draw_reconstruction(sample, [item, opt.npy_folder])
                continue
            out = run_item(sample)
            name = sample["class"][0]
            per_class_cd[name].append(out["cd_loss"].item() / n_query)
            per_class_emd[name].append(out["emd_loss"].item() / n_query)
            if exact:
                per_class_exact[name].append(out["exact_emd"].item() / n_query)
            if taus is not None:                        # the item's means over its queries, in one host read
                per_class_f[name].append(torch.stack([out["fscore"], out["precision"], out["recall"],
                                                      out["hausdorff"].expand(len(taus))]).tolist())
            if dcd_alpha is not None:
                per_class_dcd[name].append(out["dcd"].item())
            if sets or sets_emd:                        # kept on the device; one set per class after the loop
                gen, ref = out["syn_pc"], out["ref_pc_q"]
                if set_points is not None:              # K16, two launches per item: only the reduced clouds are kept
                    from fpsg_amd.sampling import farthest_point_subsample
                    for which, c in (("generated", gen), ("reference", ref)):
                        if set_points > c.size(1):
                            raise ValueError(f"--set_metrics_points {set_points} exceeds the {c.size(1)} points of the "
                                             f"{which} clouds")
                    gen = farthest_point_subsample(gen.contiguous(), set_points, start=0)
                    ref = farthest_point_subsample(ref.contiguous(), set_points, start=0)
                per_class_gen[name].append(gen)
                per_class_ref[name].append(ref)
            if want_jsd:                                # two K15 launches per item; no cloud is kept for this
                from fpsg_amd.metrics import occupancy_grid
                grid_gen[name] = occupancy_grid(out["syn_pc"].contiguous(), out=grid_gen.get(name))
                grid_ref[name] = occupancy_grid(out["ref_pc_q"].contiguous(), out=grid_ref.get(name))
    per_class_set = {}
    if sets:
        from fpsg_amd.set_metrics import generation_metrics
        for name in sorted(per_class_gen):
            per_class_set[name] = generation_metrics(torch.cat(per_class_gen[name]), torch.cat(per_class_ref[name]))
    per_class_set_emd = {}
    if sets_emd:
        from fpsg_amd.set_metrics import emd_generation_metrics
        for name in sorted(per_class_gen):
            per_class_set_emd[name] = emd_generation_metrics(torch.cat(per_class_gen[name]),
                                                             torch.cat(per_class_ref[name]))
    per_class_jsd = {}
    if want_jsd:
        from fpsg_amd.set_metrics import jsd_from_grids
        for name in sorted(grid_gen):
            per_class_jsd[name] = jsd_from_grids(grid_gen[name], grid_ref[name])
    per_class_fscore = {}
    for name in sorted(per_class_f):
        f, p, r, hd = ([[item[k][t] for item in per_class_f[name]] for t in range(len(taus))] for k in range(4))
        per_class_fscore[name] = {"thresholds": list(taus), "fscore": [statistics.mean(v) for v in f],
                                  "precision": [statistics.mean(v) for v in p],
                                  "recall": [statistics.mean(v) for v in r], "hausdorff": statistics.mean(hd[0])}
    for name in sorted(per_class_cd):
        line = (f"Class: {name} -- Rec CD: {statistics.mean(per_class_cd[name])}; "
                f"Rec EMD: {statistics.mean(per_class_emd[name])}")
        if exact:
            line += f"; Exact EMD: {statistics.mean(per_class_exact[name])}"
        if taus is not None:
            m = per_class_fscore[name]
            line += "".join(f"; F@{tau!r}: {v}" for tau, v in zip(taus, m["fscore"])) + f"; HD: {m['hausdorff']}"
        if dcd_alpha is not None:
            line += f"; DCD: {statistics.mean(per_class_dcd[name])}"
        if sets:
            m = per_class_set[name]
            line += f"; MMD-CD{at}: {m['mmd_cd']}; COV-CD{at}: {m['cov_cd']}; 1-NNA-CD{at}: {m['nna_cd']}"
        if sets_emd:
            m = per_class_set_emd[name]
            line += f"; MMD-EMD{at}: {m['mmd_emd']}; COV-EMD{at}: {m['cov_emd']}; 1-NNA-EMD{at}: {m['nna_emd']}"
            if m["cov_uncertified"] or m["nna_uncertified"]:
                line += f"; EMD-uncertified: {m['cov_uncertified']}/{m['nna_uncertified']}"
        if want_jsd:
            line += f"; JSD: {per_class_jsd[name]['jsd']}"
        print(line)
    return (per_class_cd, per_class_emd) + ((per_class_exact,) if exact else ()) + ((per_class_set,) if sets else ()) + \
        ((per_class_set_emd,) if sets_emd else ()) + ((per_class_jsd,) if want_jsd else ()) + \
        ((per_class_fscore,) if taus is not None else ()) + ((per_class_dcd,) if dcd_alpha is not None else ())


if __name__ == "__main__":
    main(cli.few_shot_parser(evaluation=True).parse_args())
