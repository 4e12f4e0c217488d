"""Episode forward / loss of the image-conditioned few-shot point-cloud generator.

Mirrors reference ``src/models/few_shot.py``: ``ImgPCProtoNet.__init__ :23-61``,
``.loss :63-73`` / ``._loss_single_class :75-129`` (training loss dict),
``._return_reconstruction :131-176`` (evaluation: Chamfer + EMD) and
``.draw_reconstruction :179-213`` -- same constructor, same ``sample`` dict contract
(``xs,xq,xad [1,S|Q|S,3,H,W]``, ``pcs,pcq,pcad [1,S|Q|S,N,3]``), same result keys.

The point-set distances are this package's HIP kernels (``fpsg_amd.metrics``) instead of
Kaolin / neuralnet_pytorch.  Deliberate fixes of reference defects:
no module-import-time ``.cuda()`` (the zero placeholder is created on the inputs' device),
and ``metric='emd'`` works instead of raising AttributeError.
"""
from __future__ import annotations

import os

import numpy as np
import torch
import torch.nn as nn

from .metrics import (DCD_DEFAULT_ALPHA, SINKHORN_TRAIN_DIAMETER, UNIFORM_PERCENTAGES, _finite_number, chamfer_distance,
                      check_dcd_alpha, check_expansion_options, check_repulsion_options, check_sinkhorn_option,
                      check_swd_options, check_uniform_options, dcd, emd_loss, episode_chamfer_losses, expansion_penalty,
                      repulsion_loss, sinkhorn_loss, swd_directions, swd_loss, uniform_loss)
from .utils import emd_wrapper

_AGGREGATOR = ["single", "multi", "mask_single", "mask_multi"]


def _fused_losses_enabled() -> bool:
    """``FPSG_FUSED_LOSSES=0``: the loss sums as separate PyTorch operations (A/B measurements)."""
    return os.environ.get("FPSG_FUSED_LOSSES", "1") != "0"


# The regularisers: scalar terms on the episode's decoded clouds, added to whichever distance is trained.  One row per
# term: (name, the key it writes into the loss dict, the model attribute that holds its weight); the model's method
# ``_<name>_term(clouds)`` gives the term's value per cloud.  The order of the rows is the order in which the terms are
# added to ``ttl_loss`` (float addition: the order is observable) and in which their keys enter the dict.
REGULARISERS = (("repulsion", "repulsion_loss", "repulsion_weight"),
                ("expansion", "expansion_loss", "expansion_weight"),
                ("uniform", "uniform_loss", "uniform_weight"))

# Every loss option of ``ImgPCProtoNet`` and its default: what ``engine.default_options``, ``engine.build_model`` and the
# parser's flags of the same names take theirs from.  The constructor's signature repeats them
# (tests/test_loss_terms_cpu.py holds the two together).
LOSS_OPTION_DEFAULTS = {
    "dcd_alpha": DCD_DEFAULT_ALPHA, "sinkhorn_blur": 0.05, "sinkhorn_diameter": SINKHORN_TRAIN_DIAMETER,
    "swd_n_proj": 64, "swd_directions": "random", "repulsion_weight": 0.0, "repulsion_k": 4, "repulsion_h": 0.03,
    "expansion_weight": 0.0, "expansion_lambda": 1.5, "uniform_weight": 0.0, "uniform_percentages": UNIFORM_PERCENTAGES,
    "uniform_radius": 1.0}


def check_weight(weight, name) -> float:
    """A regulariser's weight ``name`` as a Python float: a finite, non-negative number (``ValueError`` otherwise)."""
    return _finite_number(weight, name, lambda w: w >= 0.0, "finite and non-negative")


def check_repulsion_weight(weight) -> float:
    """``repulsion_weight`` as a Python float: a finite, non-negative number (``ValueError`` otherwise)."""
    return check_weight(weight, "repulsion_weight")


def check_expansion_weight(weight) -> float:
    """``expansion_weight`` as a Python float: a finite, non-negative number (``ValueError`` otherwise)."""
    return check_weight(weight, "expansion_weight")


def check_uniform_weight(weight) -> float:
    """``uniform_weight`` as a Python float: a finite, non-negative number (``ValueError`` otherwise)."""
    return check_weight(weight, "uniform_weight")


class _SplitRows(torch.autograd.Function):
    """``(t[:n], t[n:])`` as views; the backward is ONE concatenation.  Autograd's own slicing gives each slice a
    zero-filled full-size gradient, copies the slice's gradient in and adds the two: five launches per split."""

    @staticmethod
    def forward(ctx, t, n):
        ctx.set_materialize_grads(False)
        ctx.n, ctx.rest = n, (t.shape[0] - n,) + tuple(t.shape[1:])
        return t[:n], t[n:]

    @staticmethod
    def backward(ctx, ga, gb):
        if ga is None and gb is None:
            return None, None
        ref = ga if ga is not None else gb
        if ga is None:
            ga = ref.new_zeros((ctx.n,) + tuple(ref.shape[1:]))
        if gb is None:
            gb = ref.new_zeros(ctx.rest)
        return torch.cat([ga, gb]), None


def _split_rows(t, n):
    if t.is_cuda and t.requires_grad and torch.is_grad_enabled():
        return _SplitRows.apply(t, n)
    return t[:n], t[n:]


class ImgPCProtoNet(nn.Module):
    def __init__(self, img_encoder, pc_encoder, pc_decoder, mask_learner=None, query_factor=1.0,
                 support_factor=1.0, metric="cd", intra_support=False, aggregate="single", dcd_alpha=1000.0,
                 sinkhorn_blur=0.05, sinkhorn_diameter=SINKHORN_TRAIN_DIAMETER, repulsion_weight=0.0, repulsion_k=4,
                 repulsion_h=0.03, swd_n_proj=64, swd_directions="random", expansion_weight=0.0, expansion_lambda=1.5,
                 uniform_weight=0.0, uniform_percentages=UNIFORM_PERCENTAGES, uniform_radius=1.0):
        super().__init__()
        self.img_encoder = img_encoder
        self.pc_encoder = pc_encoder
        self.pc_decoder = pc_decoder
        self.mask_allocater = mask_learner
        self.query_factor = query_factor
        self.support_factor = support_factor
        self.intra_flag = intra_support
        if aggregate not in _AGGREGATOR:
            raise NotImplementedError(f"Found unsupported prototype aggragation: {aggregate}")
        self.aggregate = aggregate
        if metric == "cd":
            self.metric_module = None
            self.pc_metric = chamfer_distance
        elif metric == "emd":
            # training needs gradients: the differentiable approximate-assignment solver (K2)
            self.pc_metric = lambda a, b: emd_loss(a, b, reduce="sum", sinkhorn=False).reshape(1)
        elif metric == "dcd":
            # the density-aware Chamfer distance (K18) per pair, in [0, 1]; alpha multiplies the squared distance
            self.dcd_alpha = check_dcd_alpha(dcd_alpha)
            self.pc_metric = self._dcd_metric
        elif metric == "sinkhorn":
            # the Sinkhorn divergence the evaluation prints as EMD, with geomloss's gradient (K19).  The schedule starts
            # from a FIXED diameter (the evaluation's is per item): no host read, so the step can be captured
            self.sinkhorn_blur = check_sinkhorn_option(sinkhorn_blur, "sinkhorn_blur")
            self.sinkhorn_diameter = check_sinkhorn_option(sinkhorn_diameter, "sinkhorn_diameter")
            self.pc_metric = self._sinkhorn_metric
        elif metric == "swd":
            # the sliced Wasserstein distance (K22): sort-and-match on swd_n_proj directions, exact gradient.  "fixed": the
            # Fibonacci lattice, built once per device; "random": fresh unit vectors per loss call, drawn on the device
            self.swd_n_proj, self.swd_directions = check_swd_options(swd_n_proj, swd_directions)
            self._swd_lattice = {}
            self.pc_metric = self._swd_metric
        else:
            raise NotImplementedError(
                f"Found unsupported point cloud reconstruction metrics: {metric}")
        # evaluation-only distance (reference few_shot.py:168); an attribute so that a test
        # can drive the module on CPU with the oracle's implementations
        self.emd_metric = emd_wrapper
        self._batched_pairs = metric in ("dcd", "sinkhorn", "swd")      # one call over the Q + S pairs (below)
        # the regularisers (REGULARISERS) on the decoded clouds; weight 0: off, and the loss is what it is without these
        # arguments, launch for launch.  The repulsion regulariser (K21):
        self.repulsion_weight = check_weight(repulsion_weight, "repulsion_weight")
        self.repulsion_k, self.repulsion_h = check_repulsion_options(repulsion_k, repulsion_h)
        # the expansion penalty (K24) on the decoded clouds' patches.  The patch size is the decoder's: its cloud is
        # (cluster, node) patches of that many consecutive rows
        self.expansion_weight = check_weight(expansion_weight, "expansion_weight")
        _, self.expansion_lambda = check_expansion_options(2, expansion_lambda)
        self.expansion_patch = getattr(pc_decoder, "pts_per_patch", None)
        if self.expansion_weight > 0:
            if self.expansion_patch is None:
                raise ValueError("expansion_weight needs a decoder that exposes its points per patch (pts_per_patch)")
            self.expansion_patch, _ = check_expansion_options(self.expansion_patch, self.expansion_lambda)
        # the uniform loss (K25) on the decoded clouds.  The seeds are K16's farthest point sample of each decoded cloud
        # (5 % of its points)
        self.uniform_weight = check_weight(uniform_weight, "uniform_weight")
        self.uniform_percentages, self.uniform_radius = check_uniform_options(uniform_percentages, uniform_radius)
        self.overlap_encoders = False      # see _encode; switched on by bench.py / the trainer
        self._side_stream = None

    def _dcd_metric(self, a, b):
        return dcd(a, b, self.dcd_alpha)

    def _sinkhorn_metric(self, a, b):
        return sinkhorn_loss(a, b, blur=self.sinkhorn_blur, diameter=self.sinkhorn_diameter)

    def _swd_metric(self, a, b):
        if self.swd_directions == "fixed":
            dirs = self._swd_lattice.get(a.device)
            if dirs is None:
                dirs = self._swd_lattice[a.device] = swd_directions(self.swd_n_proj, a.device)
        else:       # no host read: the draw and its normalisation are device work (and replay with fresh numbers in a graph)
            dirs = torch.randn((self.swd_n_proj, 3), dtype=torch.float32, device=a.device)
            dirs = dirs / dirs.norm(dim=1, keepdim=True)
        return swd_loss(a, b, dirs)

    # ------------------------------------------------------------------ shared forward
    def _encode(self, img_s, img_q, img_ad, pc_s, pc_ad):
        """Image features of (ad ++ query) and point features of (support ++ ad), each in one
        encoder call (reference :84-100)."""
        n_support, n_query = img_s.size(1), img_q.size(1)
        img_corpus = torch.cat([img_ad.reshape(n_support, *img_ad.shape[2:]),
                                img_q.reshape(n_query, *img_q.shape[2:])], dim=0)
        pc_corpus = torch.cat([pc_s.reshape(n_support, *pc_s.shape[2:]),
                               pc_ad.reshape(n_support, *pc_ad.shape[2:])], dim=0).transpose(2, 1)
        if self.overlap_encoders and img_corpus.is_cuda:
            # the two encoders are independent: the point encoder (memory-bound BN / max
            # passes) runs on a second HIP stream beside the compute-bound image trunk;
            # autograd replays each backward on its forward stream, so they overlap there too
            cur = torch.cuda.current_stream()
            if self._side_stream is None:
                self._side_stream = torch.cuda.Stream(device=img_corpus.device)
            side = self._side_stream
            side.wait_stream(cur)
            with torch.cuda.stream(side):
                pc_z = self.pc_encoder(pc_corpus)
            img_z = self.img_encoder(img_corpus)
            cur.wait_stream(side)
            pc_z.record_stream(cur)
            pc_corpus.record_stream(side)
        else:
            img_z = self.img_encoder(img_corpus)
            pc_z = self.pc_encoder(pc_corpus)
        return (*_split_rows(img_z, n_support), *_split_rows(pc_z, n_support))

    def _encode_for_eval(self, img_q, pc_s):
        """``(img_zq, pc_z_proto)`` for the evaluation outputs.  The reference's ``_return_reconstruction``
        (``few_shot.py:131-176``) runs the training forward -- it also encodes the S "ad" images and the S "ad" clouds --
        and then drops ``img_zad`` / ``pc_z_ad`` unused (``:146,161``: only ``img_zq`` and ``pc_z_proto`` reach the
        decoder).  In evaluation mode (``model.eval()``, ``evaluate_Network.py:99``) BatchNorm normalises with its running
        statistics, so a sample's features do not depend on what else is in the batch: encoding only the Q query images
        and the S support clouds gives the same features (to the last bits of a GEMM's summation order: measured
        <= 1e-7 on ``cd_loss`` / ``emd_loss``) for 5/37 of the image trunk's and half of the point encoder's work.  Only
        when every module is in evaluation mode; ``FPSG_EVAL_PRUNE=0``: the full forward (A/B, tests)."""
        n_support, n_query = pc_s.size(1), img_q.size(1)
        img_zq = self.img_encoder(img_q.reshape(n_query, *img_q.shape[2:]))
        pc_z_proto = self.pc_encoder(pc_s.reshape(n_support, *pc_s.shape[2:]).transpose(2, 1))
        return img_zq, pc_z_proto

    def _eval_prune(self) -> bool:
        return (os.environ.get("FPSG_EVAL_PRUNE", "1") != "0" and not self.training
                and not any(m.training for m in self.modules()))

    def _decode_queries(self, img_zq, pc_z_proto, pack=None):
        """Class prototype = mean of the support features, broadcast to every query
        (reference :104-107)."""
        proto = pc_z_proto.mean(0, keepdim=True).expand(img_zq.size(0), -1)
        return self._decode(torch.cat([img_zq, proto], dim=1), pack)

    def _decode(self, hidden, pack=None):
        if pack is not None:
            return self.pc_decoder(hidden, pack=pack)
        return self.pc_decoder(hidden)

    def _decoder_pack(self):
        """Stacked decoder parameters shared by the episode's two decodes (PCDecoder.pack_parameters);
        None for a decoder without the batched form."""
        fn = getattr(self.pc_decoder, "pack_parameters", None)
        return fn() if fn is not None else None

    # ------------------------------------------------------------------------ training
    def loss(self, sample):
        return self._loss_single_class(sample["xs"], sample["xq"], sample["xad"], sample["pcs"],
                                       sample["pcq"], sample["pcad"])

    # a regulariser's value per cloud, [Q+S] fp32: ONE call of its function (K21; K24; K16 for the seeds and K25), looked
    # up in the module at call time
    def _repulsion_term(self, syn):
        return repulsion_loss(syn, self.repulsion_k, self.repulsion_h)

    def _expansion_term(self, syn):
        return expansion_penalty(syn, self.expansion_patch, self.expansion_lambda)

    def _uniform_term(self, syn):
        return uniform_loss(syn, self.uniform_percentages, self.uniform_radius)

    def _add_term(self, out, values, n_q, weight, key):
        """Adds a regulariser's values per decoded cloud (the first ``n_q`` are the queries', the rest the supports') to
        the loss dict: ``ttl_loss`` gains ``weight * (query_factor * sum_q + support_factor * sum_s)``, ``out[key]`` is the
        unweighted sum, every other entry stays as it is."""
        q_sum = values[:n_q].sum()
        weighted = self.query_factor * q_sum
        total = q_sum
        if n_q < values.size(0):
            s_sum = values[n_q:].sum()
            weighted = weighted + self.support_factor * s_sum
            total = total + s_sum
        out["ttl_loss"] = out["ttl_loss"] + weight * weighted
        out[key] = total

    def _loss_single_class(self, img_s, img_q, img_ad, pc_s, pc_q, pc_ad):
        active = [(name, key, getattr(self, attr)) for name, key, attr in REGULARISERS if getattr(self, attr) > 0]
        out, syn, n_q = self._recon_losses(img_s, img_q, img_ad, pc_s, pc_q, pc_ad, bool(active))
        if active:
            syn = syn.contiguous()
            for name, key, weight in active:
                self._add_term(out, getattr(self, f"_{name}_term")(syn), n_q, weight, key)
        return out

    def _recon_losses(self, img_s, img_q, img_ad, pc_s, pc_q, pc_ad, want_clouds=False):
        """``(loss dict, decoded clouds, number of query clouds)``; the clouds (queries first, then the supports under
        ``intra_support``) only where ``want_clouds``: their concatenation is a launch the plain loss does not make."""
        img_zad, img_zq, pc_z_proto, pc_z_ad = self._encode(img_s, img_q, img_ad, pc_s, pc_ad)
        pack = self._decoder_pack() if self.intra_flag else None
        ref_q = pc_q.squeeze(0).contiguous()
        if self.intra_flag:
            ref_s = pc_ad.squeeze(0).contiguous()
            n_q = img_zq.size(0)
            pair = getattr(self.pc_decoder, "forward_pair", None)
            if pair is not None and pack is not None:
                # the two decodes (queries, then supports) side by side: every GEMM of the decoder once (PCDecoder.forward_pair)
                proto = pc_z_proto.mean(0, keepdim=True).expand(n_q, -1)
                syn = pair(torch.cat([img_zq, proto], dim=1), torch.cat([img_zad, pc_z_ad], dim=1), pack=pack)
                syn_q, syn_s = syn[:n_q], syn[n_q:]
            else:
                syn_q = self._decode_queries(img_zq, pc_z_proto, pack)
                syn_s = self._decode(torch.cat([img_zad, pc_z_ad], dim=1), pack)
                syn = None
            if self.pc_metric is chamfer_distance and syn_q.shape[1:] == syn_s.shape[1:] \
                    and ref_q.shape[1:] == ref_s.shape[1:]:
                # the two Chamfer calls of the reference (few_shot.py:110,117) as ONE launch over
                # Q + S cloud pairs: per-pair results are independent, and a larger batch fills
                # the chip better (K1 is 6 us + 0.9 us per pair)
                if syn is None:
                    syn = torch.cat([syn_q, syn_s])
                ref = torch.cat([ref_q, ref_s])
                if syn.is_cuda and _fused_losses_enabled():
                    # K1l: the two sums and the weighted total in one launch behind K1 (and one in the backward)
                    loss_rec_q, loss_rec_s, loss_recon = episode_chamfer_losses(syn, ref, n_q, self.query_factor,
                                                                                self.support_factor)
                    return {"ttl_loss": loss_recon, "recon_loss": loss_recon, "query_rec_loss": loss_rec_q,
                            "support_rec_loss": loss_rec_s}, syn, n_q
                cd = self.pc_metric(syn, ref)
                loss_rec_q, loss_rec_s = cd[:n_q].sum(), cd[n_q:].sum()
            elif self._batched_pairs and syn_q.shape[1:] == syn_s.shape[1:] and ref_q.shape[1:] == ref_s.shape[1:]:
                # as the Chamfer branch: ONE K1 + K18 (or K2b + K19, fixed diameter; or K22) call over the Q + S pairs (a pair's
                # value does not depend on the batch, so this is only fewer launches); the fused K1l sums are Chamfer's alone
                if syn is None:
                    syn = torch.cat([syn_q, syn_s])
                d = self.pc_metric(syn, torch.cat([ref_q, ref_s]))
                loss_rec_q, loss_rec_s = d[:n_q].sum(), d[n_q:].sum()
            else:
                loss_rec_q = self.pc_metric(syn_q, ref_q).sum()
                loss_rec_s = self.pc_metric(syn_s, ref_s).sum()
            if want_clouds and syn is None:
                syn = torch.cat([syn_q, syn_s])
        else:
            syn_q = self._decode_queries(img_zq, pc_z_proto, pack)
            loss_rec_q = self.pc_metric(syn_q, ref_q).sum()
            loss_rec_s = torch.zeros(1, dtype=loss_rec_q.dtype, device=loss_rec_q.device)
            syn, n_q = syn_q, syn_q.size(0)
        loss_recon = self.query_factor * loss_rec_q + self.support_factor * loss_rec_s
        return {"ttl_loss": loss_recon, "recon_loss": loss_recon, "query_rec_loss": loss_rec_q,
                "support_rec_loss": loss_rec_s}, syn, n_q

    # ---------------------------------------------------------------------- evaluation
    def _reconstruct_queries(self, sample):
        """What both evaluation forms start with: ``(syn_pc, ref_pc_q, loss_rec_q)``, the generated and reference query
        clouds of one test item (pruned or full encode, query decode) and their summed ``pc_metric``."""
        if self._eval_prune():
            img_zq, pc_z_proto = self._encode_for_eval(sample["xq"], sample["pcs"])
        else:
            _, img_zq, pc_z_proto, _ = self._encode(sample["xs"], sample["xq"], sample["xad"], sample["pcs"], sample["pcad"])
        syn_pc = self._decode_queries(img_zq, pc_z_proto)
        ref_pc_q = sample["pcq"].squeeze(0).contiguous()
        loss_rec_q = self.pc_metric(syn_pc, ref_pc_q).sum()
        return syn_pc, ref_pc_q, loss_rec_q

    def _reconstruct_for_eval(self, sample):
        """The part of ``_return_reconstruction`` in front of the EMD: ``(syn_pc, ref_pc_q, cd_loss, diameter)`` with no host
        read in it (``engine.EvalItem`` replays it as a hipGraph).  ``diameter`` (0-dim device tensor) is what the Sinkhorn
        form's annealing schedule starts from -- ``metrics.sinkhorn_divergence`` would compute the same value itself."""
        syn_pc, ref_pc_q, loss_rec_q = self._reconstruct_queries(sample)
        pts = torch.cat([syn_pc.detach().reshape(-1, 3), ref_pc_q.reshape(-1, 3)])
        diameter = (pts.amax(0) - pts.amin(0)).norm()
        return syn_pc, ref_pc_q, self.query_factor * loss_rec_q, diameter

    def _return_reconstruction(self, sample, return_clouds: bool = False):
        """``{"cd_loss", "emd_loss"}`` of one test item; ``return_clouds=True`` also returns the generated and reference
        query clouds (``"syn_pc"``, ``"ref_pc_q"``) the two were computed on."""
        syn_pc, ref_pc_q, loss_rec_q = self._reconstruct_queries(sample)
        emd_loss = self.emd_metric(syn_pc, ref_pc_q).sum()
        if return_clouds:
            return {"cd_loss": self.query_factor * loss_rec_q, "emd_loss": emd_loss, "syn_pc": syn_pc,
                    "ref_pc_q": ref_pc_q}
        return {"cd_loss": self.query_factor * loss_rec_q, "emd_loss": emd_loss}

    @torch.no_grad()
    def reconstruct(self, sample):
        """Generated query clouds ``[Q, N, 3]`` from the support clouds and query images only
        (the forward used by ``draw_reconstruction``, reference :186-202)."""
        xs, xq, pcs = sample["xs"], sample["xq"], sample["pcs"]
        img_z = self.img_encoder(xq.reshape(-1, *xq.shape[2:]))
        pc_z = self.pc_encoder(pcs.reshape(-1, *pcs.shape[2:]).transpose(2, 1))
        return self._decode_queries(img_z, pc_z)

    @torch.no_grad()
    def reconstruct_mesh(self, sample, grid: int = 16):
        """The generated query shapes as triangle meshes -> ``(verts [Q, G*grid*grid, 3], faces [F, 3] int32)``:
        ``reconstruct``'s encode (query images and support clouds only), then the decoder's ``G`` patches evaluated on a
        regular ``grid x grid`` lattice (``PCDecoder.decode_grid``) and connected by ``surface.patch_faces``.  The faces
        are shared by the queries.  Every module must be in evaluation mode (``RuntimeError`` otherwise)."""
        from .surface import patch_faces
        if any(m.training for m in self.modules()):
            raise RuntimeError("reconstruct_mesh needs evaluation mode for every module (call .eval())")
        decode_grid = getattr(self.pc_decoder, "decode_grid", None)
        if decode_grid is None:
            raise ValueError("reconstruct_mesh needs a decoder with decode_grid (PCDecoder)")
        xq, pcs = sample["xq"], sample["pcs"]
        img_z = self.img_encoder(xq.reshape(-1, *xq.shape[2:]))
        pc_z = self.pc_encoder(pcs.reshape(-1, *pcs.shape[2:]).transpose(2, 1))
        proto = pc_z.mean(0, keepdim=True).expand(img_z.size(0), -1)
        verts = decode_grid(torch.cat([img_z, proto], dim=1), grid)
        n_patches = self.pc_decoder.num_clusters * self.pc_decoder.num_nodes
        faces = torch.from_numpy(patch_faces(grid, n_patches)).to(verts.device)
        return verts, faces

    def draw_reconstruction(self, sample, img_path, renderer="matplotlib", up="z"):
        """Writes ``<dir>/<stem>.png`` (generated vs ground truth, one column per query) and
        the clouds as ``<stem>_<code>.npy`` / ``<stem>_<code>_gt.npy``.

        ``img_path`` is ``[stem, directory]`` as ``evaluate_Network.py:111`` passes it; a plain
        path string (what ``trainNetwork.py:183,205`` passes, which makes the reference write
        garbage names -- SURVEY.md F10) is split into directory and stem instead.

        ``renderer="matplotlib"``: the reference's scatter panels.  ``renderer="splat"``: the PNG is
        ``visualization.render_reconstruction``'s (K29, on the GPU): one row per query, generated left in the decoder's
        patch colours and ground truth right, on one scale, seen by the cameras of the conditioning views for clouds
        whose ``up`` axis is ``"z"`` or ``"y"``.  The ``.npy`` files are the same either way."""
        from .visualization import render_reconstruction, visualize_point_clouds, write_png
        if renderer not in ("matplotlib", "splat"):
            raise ValueError(f"renderer must be 'matplotlib' or 'splat', got {renderer!r}")
        if up not in ("z", "y"):
            raise ValueError(f"up must be 'z' or 'y', got {up!r}")
        if isinstance(img_path, (str, os.PathLike)):
            directory, stem = os.path.split(os.fspath(img_path))
            stem = os.path.splitext(stem)[0]
        else:
            stem, directory = img_path[0], img_path[1]
        code = sample["tmp"]
        code = int(code.reshape(-1)[0]) if torch.is_tensor(code) else int(np.ravel(code)[0])
        syn_pc = self.reconstruct(sample)
        pcq = sample["pcq"].squeeze(0)
        if renderer == "splat":
            gt = pcq.reshape(-1, *pcq.shape[-2:])
            sheet = render_reconstruction(syn_pc, gt, getattr(self.pc_decoder, "pts_per_patch", None), up=up)
            write_png(os.path.join(directory, f"{stem}.png"), sheet)
        else:
            panels = [visualize_point_clouds(g, pcq[i], i) for i, g in enumerate(syn_pc)]
            write_png(os.path.join(directory, f"{stem}.png"),
                      np.concatenate(panels, axis=1).transpose(1, 2, 0))
        np.save(os.path.join(directory, f"{stem}_{code}.npy"), syn_pc.squeeze(0).cpu().numpy())
        np.save(os.path.join(directory, f"{stem}_{code}_gt.npy"), pcq.squeeze(0).cpu().numpy())
