"""Argument parsers and data plumbing shared by the three entry points.

The flag set, defaults and help semantics are those of reference
``src/trainNetwork.py:212-261`` / ``src/evaluate_Network.py:129-178`` (including the flags the
reference parses but never reads, SURVEY.md F13, so that existing command lines keep
working).  ``--sequential_eval`` is declared with ``store_true``: the reference's
``action='store_ture'`` typo makes argparse raise while the parser is being built
(SURVEY.md F4).

Additions (all optional): ``--synthetic`` (file-free corpora of the reference's shapes),
``--episodes_per_step`` (episodes per optimizer step across all ranks; data-parallel under
``torchrun``), ``--img_encoder_path`` (local VGG16-BN weights; nothing is downloaded),
``--resident`` (keep the corpora in HBM, assemble episodes on the device), ``--n_views N`` with ``--view_jitter J`` /
``--view_color_jitter C`` (training on all rendered views of the file-backed corpora: uint8 view corpora, a view, a crop
window and a colour jitter drawn per image, decoded on the GPU by K30, ``fpsg_amd.views``), ``--exact_emd`` (evaluation: the exact
EMD per class beside the two reference metrics), ``--set_metrics`` (evaluation: MMD, COV and 1-NNA under the Chamfer
distance per class, over the class's generated and reference query clouds), ``--set_metrics_emd`` (the same under the
exact EMD), ``--set_metrics_points N`` (evaluation: the clouds of the two set metrics reduced to N points each by farthest
point sampling, K16, and the labels marked ``@N``), ``--jsd`` (evaluation: the Jensen-Shannon divergence between the voxel-occupancy distributions of the class's
generated and reference query clouds), ``--fscore TAU [TAU ...]`` (evaluation: the F-score of every reconstruction at
those distances and the Hausdorff distance, per class), ``--pc_dist dcd`` with ``--dcd_alpha`` (training on the
density-aware Chamfer distance, K18), ``--dcd [ALPHA]`` (evaluation: that distance per class), ``--pc_dist sinkhorn``
with ``--sinkhorn_blur`` / ``--sinkhorn_diameter`` (training on the Sinkhorn divergence the evaluation prints as EMD, K19),
``--clip_grad_norm X`` (training: the 2-norm of every step's mean gradient clipped to X, K20, and one extra line per epoch),
``--pc_dist swd`` with ``--swd_n_proj`` / ``--swd_directions`` (training on the sliced Wasserstein distance, K22),
``--repulsion_weight W`` with ``--repulsion_k`` / ``--repulsion_h`` (training: W times the repulsion term of the decoded
clouds, K21, added to whichever ``--pc_dist`` is trained, and one extra line per epoch), ``--ema_decay D`` (training: an
exponential moving average of the weights, K23, evaluated beside the raw weights and saved as ``model_epoch_N_ema.pt``),
``--expansion_weight W`` with ``--expansion_lambda`` (training: W times the expansion penalty of the decoded clouds' patches,
K24, added like the repulsion term, and one extra line per epoch), ``--uniform_weight W`` with ``--uniform_percent`` /
``--uniform_radius`` (training: W times PU-GAN's uniform loss of the decoded clouds, K25 -- balls of the given sizes, in
percent of the cloud, around farthest-point seeds, each charged for its count's imbalance and its members' clutter --
added like the two terms above, and one extra line per epoch).

A flag that maps one-to-one onto a loss option of the model takes its default from ``few_shot.LOSS_OPTION_DEFAULTS``
(``--uniform_percent`` is in percent and keeps its own); ``validate`` runs the option checks as the rows of ``_CHECKS``,
in order, and exits with the first refusal.  A new loss term: its wrapper in ``metrics.py``, a row in
``few_shot.REGULARISERS``, its options in ``LOSS_OPTION_DEFAULTS``, its flags here.
"""
from __future__ import annotations

import argparse

import os

import torch
from torch.utils.data import DataLoader

from . import eval_report
from .ema import check_ema_decay
from .few_shot import LOSS_OPTION_DEFAULTS, check_weight
from .metrics import (UNIFORM_MAX_T, check_expansion_options, check_repulsion_options, check_sinkhorn_option,
                      check_swd_options, check_uniform_options)
from .episodes import EpisodicBatchSampler, SequentialBatchSampler, SyntheticFewShot


def _clip_norm(text: str) -> float:
    try:
        value = float(text)
    except ValueError:
        raise argparse.ArgumentTypeError(f"a non-negative number, got {text!r}") from None
    if value != value or value < 0:
        raise argparse.ArgumentTypeError(f"a non-negative number, got {text!r}")
    return value


def few_shot_parser(evaluation: bool = False) -> argparse.ArgumentParser:
    p = argparse.ArgumentParser()
    g = p.add_argument_group("data / episode")
    g.add_argument("--synthetic", action="store_true", help="Use synthetic corpora (no files needed);")
    g.add_argument("--config_path", type=str, default="", help="Path to the configuration file: {DATASET}_{SPLIT}.txt;")
    g.add_argument("--test_path", type=str, default="", help="Path to the test file: {DATASET}_{SPLIT}.txt;")
    g.add_argument("--refer_path", type=str, default="./modelnet_files/", help="Path to the reference folder [default: ./modelnet_files/];")
    g.add_argument("--dataset", type=str, default="modelnet", choices=["modelnet", "shapenet"])
    g.add_argument("--pc_encoder_path", type=str, default="", help="Path to the pre-trained pcencoder;")
    g.add_argument("--img_encoder_path", type=str, default="", help="Local VGG16-BN state dict (optional);")
    g.add_argument("--n_way", type=int, default=1)
    g.add_argument("--n_shot", type=int, default=20)
    g.add_argument("--n_query", type=int, default=0, help="Number of Query set [default: --n_shot];")
    g.add_argument("--resident", action="store_true", help="Keep corpora on the GPU (synthetic mode);")
    g.add_argument("--n_views", type=int, default=1, metavar="N",
                   help="Training: views kept per item, a random one per image and episode; 0 = all views found "
                        "[default: 1 = the first view only, as the reference].  The views are kept as uint8 pixels and "
                        "become the encoder's floats on the GPU (K30); evaluation always reads the first view;")
    g.add_argument("--view_jitter", type=float, default=0.0, metavar="J",
                   help="Training: a random square window per image, its side 1-J .. 1+J of the image's and its centre up "
                        "to J/2 of the side off the middle, resampled to the image's size (clamp to edge), J in "
                        "[0, 0.5) [default: 0 = off];")
    g.add_argument("--view_color_jitter", type=float, default=0.0, metavar="C",
                   help="Training: contrast and saturation 1-C .. 1+C and brightness -C/4 .. C/4 per image, C in [0, 1) "
                        "[default: 0 = off];")

    g = p.add_argument_group("network")
    g.add_argument("--img_encoder", type=str, default="vgg_16")
    g.add_argument("--pc_encoder", type=str, default="pointnet")
    g.add_argument("--support_factor", type=float, default=1.0)
    g.add_argument("--query_factor", type=float, default=1.0)
    g.add_argument("--intra_recon", action="store_true")
    g.add_argument("--epoch_start_recon", type=int, default=0)
    g.add_argument("--num_clusters", type=int, default=4)
    g.add_argument("--ori_dim", type=int, default=2)
    g.add_argument("--raw_dim", type=int, default=3)
    g.add_argument("--num_nodes", type=int, default=4)
    g.add_argument("--device", type=str, default="cuda")
    g.add_argument("--bottleneck_size", type=int, default=1536)
    g.add_argument("--template_type", type=str, default="SQUARE")
    g.add_argument("--activation", type=str, default="relu")
    g.add_argument("--dim_template", type=int, default=2)
    g.add_argument("--aggregate", type=str, default="single", choices=["single", "multi", "mask_single", "mask_multi"])

    g = p.add_argument_group("training")
    g.add_argument("--n_episode", type=int, default=100)
    g.add_argument("--epoch", type=int, default=500)
    g.add_argument("--lr", type=float, default=1e-3)
    g.add_argument("--lr_decay", type=float, default=350)
    g.add_argument("--resume", type=int, default=-1)
    g.add_argument("--pc_dist", type=str, default="cd", choices=["cd", "emd", "dcd", "sinkhorn", "swd"])
    g.add_argument("--dcd_alpha", type=float, default=LOSS_OPTION_DEFAULTS["dcd_alpha"],
                   help="With --pc_dist dcd: the factor on the squared nearest-neighbour distance inside the exponential "
                        "of the density-aware Chamfer distance [default: 1000];")
    g.add_argument("--sinkhorn_blur", type=float, default=LOSS_OPTION_DEFAULTS["sinkhorn_blur"],
                   help="With --pc_dist sinkhorn: the blur of the Sinkhorn divergence, the annealing ends at blur^2 "
                        "[default: 0.05, as the evaluation's EMD];")
    g.add_argument("--sinkhorn_diameter", type=float, default=LOSS_OPTION_DEFAULTS["sinkhorn_diameter"],
                   help="With --pc_dist sinkhorn: the FIXED diameter the annealing schedule starts from [default: 2*sqrt(3), "
                        "the diagonal of [-1,1]^3].  The evaluation's EMD takes each item's own bounding-box diagonal "
                        "instead, so its value differs slightly (under 1 %% on unit-ball clouds); a fixed one keeps the "
                        "training step free of host reads;")
    g.add_argument("--swd_n_proj", type=int, default=LOSS_OPTION_DEFAULTS["swd_n_proj"], metavar="L",
                   help="With --pc_dist swd: the number of directions the sliced Wasserstein distance projects on, "
                        "1..1024 [default: 64];")
    g.add_argument("--swd_directions", type=str, default=LOSS_OPTION_DEFAULTS["swd_directions"], metavar="{random,fixed}",
                   help="With --pc_dist swd: 'random' draws fresh unit vectors for every loss, 'fixed' uses one Fibonacci "
                        "lattice on the sphere throughout [default: random];")
    g.add_argument("--clip_grad_norm", type=_clip_norm, default=0.0, metavar="X",
                   help="Clip the 2-norm of every optimizer step's mean gradient to X [default: 0 = off]; prints the "
                        "largest norm and the number of clipped steps after every epoch;")
    g.add_argument("--repulsion_weight", type=float, default=LOSS_OPTION_DEFAULTS["repulsion_weight"], metavar="W",
                   help="Add W times the repulsion term of the generated clouds (each point against its nearest "
                        "neighbours in its own cloud) to the training loss, under any --pc_dist [default: 0 = off]; prints "
                        "the mean term per cloud after every epoch;")
    g.add_argument("--repulsion_k", type=int, default=LOSS_OPTION_DEFAULTS["repulsion_k"], metavar="K",
                   help="With --repulsion_weight: neighbours per point, 1..8 [default: 4];")
    g.add_argument("--repulsion_h", type=float, default=LOSS_OPTION_DEFAULTS["repulsion_h"], metavar="H",
                   help="With --repulsion_weight: the bandwidth of the term, a length -- clouds live in the unit ball "
                        "[default: 0.03];")
    g.add_argument("--expansion_weight", type=float, default=LOSS_OPTION_DEFAULTS["expansion_weight"], metavar="W",
                   help="Add W times the expansion penalty of the generated clouds (each decoder patch charged for the "
                        "edges of its minimum spanning tree that are longer than L times the tree's mean edge) to the "
                        "training loss, under any --pc_dist [default: 0 = off]; prints the mean penalty per cloud after "
                        "every epoch;")
    g.add_argument("--expansion_lambda", type=float, default=LOSS_OPTION_DEFAULTS["expansion_lambda"], metavar="L",
                   help="With --expansion_weight: an edge is charged where it is longer than L times its patch's mean "
                        "edge, L >= 1 [default: 1.5];")
    g.add_argument("--uniform_weight", type=float, default=LOSS_OPTION_DEFAULTS["uniform_weight"], metavar="W",
                   help="Add W times the uniform loss of the generated clouds (balls of several sizes around farthest-point "
                        "seeds, each charged for how far its point count is from its share and how far its members' "
                        "nearest-neighbour distances are from an even spacing) to the training loss, under any --pc_dist "
                        "[default: 0 = off]; prints the mean loss per cloud after every epoch;")
    g.add_argument("--uniform_percent", type=float, nargs="+", default=[0.4, 0.6, 0.8, 1.0, 1.2], metavar="P",
                   help="With --uniform_weight: the balls' sizes in percent of the cloud, each in (0, 100], at most 8 "
                        "[default: 0.4 0.6 0.8 1.0 1.2];")
    g.add_argument("--uniform_radius", type=float, default=LOSS_OPTION_DEFAULTS["uniform_radius"], metavar="R",
                   help="With --uniform_weight: the radius of the disc whose area the surface is taken to have, a length "
                        "-- clouds live in the unit ball [default: 1.0];")
    g.add_argument("--ema_decay", type=float, default=0.0, metavar="D",
                   help="Keep an exponential moving average of the weights with decay D in (0, 1), warmed up as "
                        "min(D, (1 + t) / (10 + t)) [default: 0 = off]; every evaluation is followed by one on the "
                        "averaged weights ([EMA] lines) and model_epoch_N_ema.pt is saved beside model_epoch_N.pt;")
    g.add_argument("--SGD", action="store_true")
    g.add_argument("--episodes_per_step", type=int, default=0,
                   help="Episodes per optimizer step over all ranks [default: one per rank];")

    g = p.add_argument_group("experiment")
    g.add_argument("--name", type=str, default="0")
    g.add_argument("--dir_name", type=str, default="")
    g.add_argument("--model_path", type=str, default="../checkpoint")
    g.add_argument("--save_interval", type=int, default=50)
    g.add_argument("--sample_interval", type=int, default=10)
    g.add_argument("--eval_interval", type=int, default=20)
    g.add_argument("--eval_model", type=str, default="NONE")
    g.add_argument("--sequential_eval", action="store_true")
    g.add_argument("--sample_renderer", type=str, default="matplotlib", choices=("matplotlib", "splat"),
                   help="What draws the sample images (generated against ground-truth clouds): 'matplotlib', the "
                        "reference's scatter panels on the host, or 'splat', shaded spheres on the GPU, generated "
                        "clouds in the decoder's patch colours, both on one scale [default: matplotlib];")
    g.add_argument("--sample_up", type=str, default="z", choices=("z", "y"),
                   help="With --sample_renderer splat: the clouds' up axis, z for ModelNet, y for ShapeNet [default: z];")
    if evaluation:
        g.add_argument("--npy_folder", type=str, default="", help="Where draw_reconstruction dumps go;")
        eval_report.add_arguments(g)
    return p


def uniform_fractions(percent) -> tuple:
    """``--uniform_percent`` (percent of the cloud) as the fractions ``metrics.uniform_loss`` takes: 1..8 finite values in
    (0, 100] (``ValueError`` otherwise)."""
    try:
        values = [float(p) for p in percent]
    except (TypeError, ValueError):
        raise ValueError(f"1..{UNIFORM_MAX_T} numbers in (0, 100], got {percent!r}") from None
    if not 1 <= len(values) <= UNIFORM_MAX_T:
        raise ValueError(f"1..{UNIFORM_MAX_T} values, got {len(values)}")
    for v in values:
        if not (v == v and 0.0 < v <= 100.0):
            raise ValueError(f"each value must be in (0, 100], got {v!r}")
    return tuple(v / 100.0 for v in values)


def _uniform_percent(opt) -> None:
    opt.uniform_percentages = uniform_fractions(opt.uniform_percent)       # what the model takes


def multi_view(opt) -> bool:
    """Whether training reads the multi-view datasets (``fpsg_amd.views``): any of ``--n_views``, ``--view_jitter``,
    ``--view_color_jitter`` away from its default.  ``ValueError`` for a bad value or a combination with ``--synthetic``;
    a namespace from before the options: False."""
    if getattr(opt, "n_views", None) is None:
        return False
    from .views import check_view_options
    return check_view_options(opt.n_views, getattr(opt, "view_jitter", 0.0), getattr(opt, "view_color_jitter", 0.0),
                              synthetic=bool(opt.synthetic))


# validate()'s option checks in the order they run: (the attribute without which -- an older namespace -- the check is
# skipped, the check: ValueError for a bad value, what goes in front of its message)
_CHECKS = (
    ("sinkhorn_blur", lambda o: check_sinkhorn_option(o.sinkhorn_blur, "sinkhorn_blur"), "--"),
    ("sinkhorn_diameter", lambda o: check_sinkhorn_option(o.sinkhorn_diameter, "sinkhorn_diameter"), "--"),
    ("swd_n_proj", lambda o: check_swd_options(o.swd_n_proj, getattr(o, "swd_directions",
                                                                      LOSS_OPTION_DEFAULTS["swd_directions"])), "--swd_"),
    ("repulsion_weight", lambda o: check_weight(o.repulsion_weight, "repulsion_weight"), "--"),
    ("repulsion_weight", lambda o: check_repulsion_options(o.repulsion_k, o.repulsion_h), "--repulsion_"),
    ("expansion_weight", lambda o: check_weight(o.expansion_weight, "expansion_weight"), "--"),
    ("expansion_weight", lambda o: check_expansion_options(2, o.expansion_lambda), "--expansion_lambda: "),
    ("uniform_weight", lambda o: check_weight(o.uniform_weight, "uniform_weight"), "--"),
    ("uniform_weight", _uniform_percent, "--uniform_percent: "),
    ("uniform_weight", lambda o: check_uniform_options(o.uniform_percentages, o.uniform_radius), "--uniform_"),
    ("ema_decay", lambda o: check_ema_decay(o.ema_decay), "--"),
    ("n_views", multi_view, "--"),
)


def validate(opt) -> None:
    if not opt.synthetic and not (opt.config_path and opt.test_path):
        raise SystemExit("--config_path and --test_path are required unless --synthetic is given")
    if opt.n_way != 1:
        raise SystemExit("only 1-way episodes are defined by the model (as in the reference)")
    eval_report.check_alpha_option(opt, "dcd_alpha")
    for gate, check, prefix in _CHECKS:
        if getattr(opt, gate, None) is not None:
            try:
                check(opt)
            except ValueError as e:
                raise SystemExit(f"{prefix}{e}") from None
    eval_report.check(opt)          # the evaluation report's options; a training namespace has none of them


def build_datasets(opt, n_query: int, device, views: bool = True):
    """(train, test) datasets with the reference's item layout.  With ``--n_views`` other than 1 or a view jitter the
    training dataset is the multi-view one (``fpsg_amd.views``: uint8 images and their tables, ``views.decode_episode``
    after the upload); the test dataset is always the default one.  ``views=False`` (evaluation): the three options are
    ignored."""
    if opt.synthetic:
        where = device if opt.resident else "cpu"
        need = opt.n_shot + max(n_query, 1)
        ds = SyntheticFewShot(n_classes=4, per_class=max(need, 8), n_support=opt.n_shot,
                              n_query=n_query, seed=1234, device=where)
        ds_test = SyntheticFewShot(n_classes=2, per_class=max(need, 8), n_support=opt.n_shot,
                                   n_query=n_query, seed=4321, device=where)
        return ds, ds_test
    from .datasets import FewShotModelNet, FewShotShapeNet, modelnet_transform, shapenet_transform
    if opt.dataset == "modelnet":
        cls, tfs = FewShotModelNet, modelnet_transform()
    else:
        cls, tfs = FewShotShapeNet, shapenet_transform()
    if views and multi_view(opt):
        from .views import MultiViewModelNet, MultiViewShapeNet
        many = MultiViewModelNet if opt.dataset == "modelnet" else MultiViewShapeNet
        ds = many(opt.config_path, opt.refer_path, n_classes=opt.n_way, n_support=opt.n_shot, n_query=n_query,
                  transform=tfs, n_views=opt.n_views, view_jitter=opt.view_jitter,
                  view_color_jitter=opt.view_color_jitter)
    else:
        ds = cls(opt.config_path, opt.refer_path, n_classes=opt.n_way, n_support=opt.n_shot,
                 n_query=n_query, transform=tfs)
    ds_test = cls(opt.test_path, opt.refer_path, n_classes=opt.n_way, n_support=opt.n_shot,
                  n_query=n_query, transform=tfs)
    return ds, ds_test


def _collate(batch):
    """One episode per batch (n_way = 1): add the leading axis DataLoader's default collate
    would add, without copying device-resident tensors through the CPU."""
    from .episodes import collate_episode
    assert len(batch) == 1
    return collate_episode(batch[0])


def build_loaders(opt, ds, ds_test):
    sampler = EpisodicBatchSampler(len(ds), opt.n_way, opt.n_episode)
    ran_sampler = EpisodicBatchSampler(len(ds_test), opt.n_way, opt.n_episode)
    seq_sampler = SequentialBatchSampler(len(ds_test))
    dl = DataLoader(ds, batch_sampler=sampler, num_workers=0, collate_fn=_collate)
    dl_test = DataLoader(ds_test, batch_sampler=seq_sampler if opt.sequential_eval else ran_sampler,
                         num_workers=0, collate_fn=_collate)
    return dl, dl_test


def usable_cores() -> int:
    """Cores this process may really use: affinity mask and cgroup CPU quota, not the host's core count (a container
    on a GPU node sees every host core but is granted a share of them).  ``FPSG_CPU_THREADS`` caps it (default 16)."""
    n = os.cpu_count() or 1
    try:
        n = min(n, len(os.sched_getaffinity(0)))
    except AttributeError:
        pass
    try:
        quota, period = open("/sys/fs/cgroup/cpu.max").read().split()
        if quota != "max":
            n = min(n, max(1, int(int(quota) / int(period))))
    except (OSError, ValueError):
        pass
    return max(1, min(n, int(os.environ.get("FPSG_CPU_THREADS", "16"))))


def limit_host_threads(world: int = 1) -> int:
    """PyTorch sizes its intra-op pool by the HOST's core count; with a 16-core share of a 200-core node every host
    op that parallelises (the row gathers of episode assembly, normalisation, collate) then thrashes -- the gather
    of one 32-shot episode took 30 ms instead of 3.  One call per process, before the first parallel op."""
    n = max(1, usable_cores() // max(world, 1))
    if torch.get_num_threads() > n:
        torch.set_num_threads(n)
    return n


def pick_device(opt) -> torch.device:
    limit_host_threads()
    if opt.device.startswith("cuda") and not torch.cuda.is_available():
        raise SystemExit("--device cuda requested but no ROCm GPU is visible "
                         "(the Chamfer / EMD / kNN ops are HIP kernels; there is no CPU fallback)")
    device = torch.device(opt.device)
    if device.type == "cuda":
        from . import gemm_tuning
        gemm_tuning.enable()          # recorded library-GEMM kernel choices for this path's shapes
    return device
