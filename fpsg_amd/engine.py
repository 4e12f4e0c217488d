"""Model construction and the optimizer step shared by the entry points and ``bench.py``.

``build_model`` follows reference ``src/trainNetwork.py:45-64`` (same ``opt`` namespace: the
argparse result doubles as the decoder's config).  ``TrainStep`` is the hot loop body of
``trainNetwork.py:140-148`` (zero_grad -> loss -> backward -> optimizer.step) extended to
``E`` episodes per optimizer step and ``W`` ranks (``fpsg_amd.dist``); with ``E = W = 1`` it
is exactly the reference step.
"""
from __future__ import annotations

import argparse
import os

import torch
import torch.optim as optim

from . import dist as fdist
from . import bn_counters, eval_report, winograd
from .few_shot import LOSS_OPTION_DEFAULTS, ImgPCProtoNet
from .image_net import ImageEncoderWarpper
from .metrics import check_dcd_alpha, check_thresholds, nearest_rows
from .ema import WeightEma, check_ema_decay
from .optim import FlatAdam, check_max_grad_norm
from .point_cloud_net import PCDecoder, PCEncoder


def default_options(**overrides) -> argparse.Namespace:
    """The reference's argparse defaults (``trainNetwork.py:215-261``) for everything the
    model constructors read, and the model's loss options (``few_shot.LOSS_OPTION_DEFAULTS``)."""
    opt = argparse.Namespace(
        img_encoder="vgg_16", pc_encoder="pointnet", pc_encoder_path="", img_encoder_path="",
        support_factor=1.0, query_factor=1.0, intra_recon=False, num_clusters=4, ori_dim=2,
        raw_dim=3, num_nodes=4, device="cuda", bottleneck_size=1536, template_type="SQUARE",
        activation="relu", aggregate="single", pc_dist="cd", lr=1e-3, lr_decay=350, SGD=False,
        n_way=1, n_shot=20, n_query=0, clip_grad_norm=0.0, ema_decay=0.0, sample_renderer="matplotlib", sample_up="z",
        **LOSS_OPTION_DEFAULTS)
    for k, v in overrides.items():
        setattr(opt, k, v)
    return opt


def build_model(opt) -> ImgPCProtoNet:
    img_encoder = ImageEncoderWarpper(opt.img_encoder, finetune_layer=3,
                                      weights=getattr(opt, "img_encoder_path", "") or None)
    pc_encoder = PCEncoder(opt.pc_encoder)
    pc_decoder = PCDecoder(conf=opt)
    path = getattr(opt, "pc_encoder_path", "")
    if path and os.path.exists(path):
        print("Pretrained Model exist, loading")
        pc_encoder.load_state_dict(torch.load(path, map_location="cpu", weights_only=True))
    return ImgPCProtoNet(img_encoder, pc_encoder, pc_decoder, mask_learner=None,
                         query_factor=opt.query_factor, support_factor=opt.support_factor,
                         metric=getattr(opt, "pc_dist", "cd"), intra_support=opt.intra_recon,
                         aggregate=opt.aggregate,
                         **{name: getattr(opt, name, default) for name, default in LOSS_OPTION_DEFAULTS.items()})


def build_optimizer(model, opt):
    """Adam(lr, betas=(.9,.999)) or SGD(weight_decay=1e-2) + StepLR(gamma=.5)
    (``trainNetwork.py:118-130``).  ``opt.clip_grad_norm`` (0: off) becomes the optimizer's ``max_grad_norm``: K20 inside
    ``FlatAdam.step``; on any other optimizer an attribute that ``TrainStep`` reads.  ``opt.ema_decay`` (0: off) makes a
    ``WeightEma`` of the trainable parameters, ``optimizer.ema``: K23 inside ``FlatAdam.step``; on any other optimizer
    ``TrainStep`` updates it after the step."""
    on_gpu = next(model.parameters()).is_cuda
    max_norm = check_max_grad_norm(getattr(opt, "clip_grad_norm", None), "clip_grad_norm")
    decay = check_ema_decay(getattr(opt, "ema_decay", None), "ema_decay")
    if not opt.SGD:
        if on_gpu and os.environ.get("FPSG_FLAT_ADAM", "1") != "0":
            # K7: parameters, gradients and moments in flat buffers, the step is one HBM stream
            optimizer = FlatAdam(model.parameters(), lr=opt.lr, betas=(0.9, 0.999), max_grad_norm=max_norm)
        else:
            optimizer = optim.Adam(model.parameters(), lr=opt.lr, betas=(0.9, 0.999),
                                   **({"fused": True} if on_gpu else {}))
    else:
        optimizer = optim.SGD(model.parameters(), lr=opt.lr, weight_decay=1e-2)
    if max_norm is not None and not isinstance(optimizer, FlatAdam):
        optimizer.max_grad_norm = max_norm
    if decay is not None:
        ema = WeightEma(model.parameters(), decay)
        if isinstance(optimizer, FlatAdam):
            optimizer.attach_ema(ema)
        else:
            optimizer.ema = ema
    scheduler = optim.lr_scheduler.StepLR(optimizer, step_size=int(opt.lr_decay), gamma=0.5)
    return optimizer, scheduler


def to_device(sample: dict, device) -> dict:
    """``trainNetwork.py:37-43`` ``to_cuda``: moves the six tensors of an episode."""
    for k in ("xs", "xq", "xad", "pcs", "pcq", "pcad"):
        if k in sample and sample[k].device != device:
            sample[k] = sample[k].to(device, non_blocking=True)
    return sample


def _total(loss):
    """The scalar to differentiate: the loss itself when it already is one (no reduction launch)."""
    return loss if loss.dim() == 0 else loss.sum()


class TrainStep:
    """One optimizer step over the local share of a global step's episodes.

    ``graph=True`` (GPU only): the forward + backward of an episode is captured once per
    episode shape into a hipGraph and replayed -- an episode is ~1300 kernel launches, many of
    them a few microseconds long, and the eager step is partly host-bound.  Inputs are copied
    into the graph's static buffers; the captured sequence ends with the multi-tensor adds of
    the episode's gradients into the flat buffer (``FlatGradBuckets.absorb``).  With more than
    one rank the LAST local episode of a step always runs eagerly, so that its backward can
    launch the bucketed all-reduce from the autograd hooks.

    ``max_grad_norm`` (default: the optimizer's ``max_grad_norm`` attribute, as ``build_optimizer`` sets it from
    ``--clip_grad_norm``; None, 0 and inf mean off): the 2-norm of the step's MEAN gradient is clipped to it.  With
    ``FlatAdam`` that happens inside ``optimizer.step()`` (K20: no pass over the gradient, no host read); with any other
    optimizer -- CPU runs, ``--SGD``, ``FPSG_FLAT_ADAM=0`` -- the attached gradients hold the mean and
    ``torch.nn.utils.clip_grad_norm_`` runs on them in front of the step.  ``last_grad_norm`` / ``clip_stats()`` report
    either form.  Note that after a step with ``FlatAdam`` ``p.grad`` holds the SUM over the step's episodes (the ``1/E``
    is folded into the step): ``clip_grad_norm_`` called on it from outside clips at ``E`` times the wrong threshold.

    ``optimizer.ema`` (``build_optimizer`` sets it from ``--ema_decay``; absent or None: off): the ``WeightEma`` of the
    model's weights.  ``FlatAdam.step()`` updates it inside its own stream (K23); with any other optimizer the step ends
    with ``ema.update()``."""

    def __init__(self, model, optimizer, world: int = 1, bucket_mb: float = 80.0, graph: bool = False,
                 max_grad_norm=None):
        self.model, self.optimizer, self.world = model, optimizer, world
        if max_grad_norm is not None:
            optimizer.max_grad_norm = check_max_grad_norm(max_grad_norm, "TrainStep: max_grad_norm")
        self._torch_clip = None     # (last norm, counters) of the clip_grad_norm_ form
        self.buckets = fdist.FlatGradBuckets(model, bucket_mb=bucket_mb)
        if isinstance(optimizer, FlatAdam):
            optimizer.bind_gradients(self.buckets.flat)      # same layout: the step reads it in place
        self.use_graph = bool(graph) and next(model.parameters()).is_cuda
        if self.use_graph:
            self.buckets.lazy = False       # a captured episode ends with its own adds into the flat buffer, in order
        self._graphs = {}
        self._eager_runs = {}

    # ------------------------------------------------------------------ graph plumbing
    _KEYS = ("xs", "xq", "xad", "pcs", "pcq", "pcad")

    def _shape_key(self, sample, first):
        return tuple((k, tuple(sample[k].shape)) for k in self._KEYS) + (bool(first),)

    def _episode(self, sample, first=False, absorb=True):
        """Forward + backward of one episode into fresh gradient tensors, then their
        multi-tensor copy (``first``) / add into the flat buffer (``absorb=False``: the step is
        this one episode and the optimizer reads the gradients where they are)."""
        self.buckets.detach()
        with bn_counters.deferred():        # the ~20 num_batches_tracked increments as multi-tensor adds
            out = self.model.loss(sample)
        _total(out["ttl_loss"]).backward()
        if absorb:
            self.buckets.absorb(first)
        return {n: v.detach() for n, v in out.items()}

    def _episode_hooked(self, sample, first):
        """The overlapped form (last local episode of a multi-rank step): fresh gradient tensors
        as in ``_episode``; the armed hooks absorb each bucket and launch its all-reduce as soon
        as its gradients are complete."""
        self.buckets.detach()
        self.buckets.arm(first)
        with bn_counters.deferred():
            out = self.model.loss(sample)
        _total(out["ttl_loss"]).backward()
        return {n: v.detach() for n, v in out.items()}

    def _capture(self, sample, first, absorb):
        static = {k: sample[k].clone() for k in self._KEYS}
        g = torch.cuda.CUDAGraph()
        # thread_local: an RCCL watchdog thread may query events while this thread captures
        with torch.cuda.graph(g, capture_error_mode="thread_local"):
            static_out = self._episode(static, first, absorb)
        # the captured gradient tensors belong to the graph's pool: kept (static addresses) when the
        # optimizer reads them in place, dropped otherwise
        grads = None if absorb else [p.grad for p in self.buckets.params]
        self.buckets.detach()
        return g, static, static_out, grads

    def _run_graphed(self, sample, first, absorb=True):
        key = self._shape_key(sample, first) + (bool(absorb),)
        if key not in self._graphs:
            # the first eager runs of a shape let MIOpen / hipBLASLt pick their kernels and
            # warm the allocator; capture happens on the third use
            n = self._eager_runs.get(key, 0)
            if n < 2:
                self._eager_runs[key] = n + 1
                return self._episode(sample, first, absorb)
            self._graphs[key] = self._capture(sample, first, absorb)   # records only; replayed below
        g, static, static_out, grads = self._graphs[key]
        if grads is not None:
            for p, gr in zip(self.buckets.params, grads):
                p.grad = gr
        for k in self._KEYS:
            static[k].copy_(sample[k], non_blocking=True)
        winograd.check_bank_before_replay()
        g.replay()
        return {n: v.clone() for n, v in static_out.items()}

    # ------------------------------------------------------------------- clipping
    def _clip_attached(self, max_norm: float) -> None:
        """``clip_grad_norm_`` on the attached (mean) gradients, with K20's counters kept on the device."""
        params = [p for p in self.model.parameters() if p.grad is not None]
        norm = torch.nn.utils.clip_grad_norm_(params, max_norm).detach().float()
        stats = self._torch_clip[1] if self._torch_clip else torch.zeros(4, dtype=torch.float64, device=norm.device)
        finite = torch.isfinite(norm)
        stats[0] += 1
        stats[1] += (max_norm / (norm + 1e-6) < 1).double()
        stats[2] += (~finite).double()
        stats[3] = torch.maximum(stats[3], torch.where(finite, norm, torch.zeros_like(norm)).double())
        self._torch_clip = (norm, stats)

    @property
    def last_grad_norm(self):
        """The norm of the last clipped step's mean gradient, a 0-dim tensor on the model's device (no sync), or None."""
        if isinstance(self.optimizer, FlatAdam):
            return self.optimizer.last_grad_norm
        return self._torch_clip[0] if self._torch_clip else None

    def clip_stats(self, reset: bool = True) -> dict:
        """``FlatAdam.clip_stats`` for whichever form clips: one host read."""
        if isinstance(self.optimizer, FlatAdam):
            return self.optimizer.clip_stats(reset)
        if self._torch_clip is None:
            return {"steps": 0, "clipped": 0, "nonfinite": 0, "max_norm_seen": 0.0}
        s = self._torch_clip[1].tolist()
        if reset:
            self._torch_clip[1].zero_()
        return {"steps": int(s[0]), "clipped": int(s[1]), "nonfinite": int(s[2]), "max_norm_seen": float(s[3])}

    # ----------------------------------------------------------------------- the step
    def __call__(self, local_episodes: list[dict], n_episodes_global: int | None = None):
        """Returns the list of loss dicts (device tensors; call ``.item()`` outside the
        timed path).  ``n_episodes_global`` defaults to ``len(local) * world``."""
        if n_episodes_global is None:
            n_episodes_global = len(local_episodes) * self.world
        results = []
        multi = self.buckets.world_initialised()
        # one episode, one rank, K7: no flat gradient buffer at all -- the optimizer reads the
        # gradients through a pointer table (saves the 310 MB gather)
        direct = (isinstance(self.optimizer, FlatAdam) and len(local_episodes) == 1 and n_episodes_global == 1
                  and not multi and os.environ.get("FPSG_DIRECT_GRADS", "1") != "0")
        if not local_episodes:  # still take part in the step's collectives
            self.buckets.zero()
            self.buckets.attach()
            self.buckets.arm()
        last = len(local_episodes) - 1
        with winograd.weights_frozen():      # no parameter changes until optimizer.step() below
            for k, sample in enumerate(local_episodes):
                first, final = k == 0, k == last
                if final and multi:
                    results.append(self._episode_hooked(sample, first))
                elif self.use_graph:
                    results.append(self._run_graphed(sample, first, absorb=not direct))
                else:
                    results.append(self._episode(sample, first, absorb=not direct))
        if not direct:
            # K7 multiplies the gradient by 1/E as it reads it (bit-identical to scaling the buffer first: one fp32
            # product per element either way); the flat buffer then holds the SUM over the step's episodes.
            # FPSG_FOLD_GRAD_SCALE=0: the separate pass (A/B).
            fold = isinstance(self.optimizer, FlatAdam) and os.environ.get("FPSG_FOLD_GRAD_SCALE", "1") != "0"
            self.buckets.finish(n_episodes_global, scale=not fold)
            self.buckets.attach()       # the optimizer reads the step's gradient from the flat buffer
            if fold:
                self.optimizer.grad_scale = 1.0 / n_episodes_global if n_episodes_global > 1 else 1.0
        if not isinstance(self.optimizer, FlatAdam):
            max_norm = check_max_grad_norm(getattr(self.optimizer, "max_grad_norm", None), "max_grad_norm")
            if max_norm is not None:
                self._clip_attached(max_norm)
        try:
            self.optimizer.step()
        finally:
            if isinstance(self.optimizer, FlatAdam):
                self.optimizer.grad_scale = 1.0
        ema = getattr(self.optimizer, "ema", None)
        if ema is not None and not ema.fused:       # (FlatAdam's step has updated a shadow that lives in its flat buffer)
            ema.update()
        return results


class EvalItem:
    """The body of the evaluation loop (reference ``src/evaluate_Network.py:107-118``: ``_return_reconstruction`` per test
    item, then two ``.item()`` reads) for a model in eval mode on a ROCm device.

        with EvalItem(model) as item:
            for sample in loader:
                out = item(sample)            # {"cd_loss": 0-dim tensor, "emd_loss": 0-dim tensor}

    The context is one ``winograd.weights_frozen(constant=True)`` block -- weights and running statistics do not change
    while evaluating, so transformed filters, stacked decoder weights and the BatchNorms' channel coefficients are made
    once, not per item.  ``graph=True`` [default on a GPU, ``FPSG_EVAL_GRAPH=0`` to switch off]: an item is ~200 launches of a
    few microseconds and the eager loop is ~17 % host / drain-bound, so everything in front of the EMD -- both encoders,
    the query decode, K1, the clouds' diameter -- is captured once per input shape and replayed; the Sinkhorn form's
    annealing schedule depends on that diameter (geomloss' rule), so the loop reads it (its one mid-item host read, as
    before) and launches K2b's ~12 kernels eagerly.  The first two items of a shape run eagerly (the libraries pick
    their kernels, the filter bank registers the layers); capture happens on the third.  A model whose ``emd_metric`` /
    ``pc_metric`` were replaced (tests drive the module with the oracle's functions) takes the plain method.

    ``exact_emd=True``, ``fscore=(tau, ...)``, ``dcd=alpha``: the per-item parts of the report's column groups
    (``eval_report.COLUMNS`` says what each adds to an item's result; bad values raise ``ValueError`` here).  They run
    eagerly after the item -- after the replay, on the same ``syn_pc`` / ``ref_pc_q`` the graph produced, never inside a
    capture -- and the groups that read K1's rows of those clouds share one ``metrics.nearest_rows`` call.

    ``return_clouds=True``: every item also returns ``"syn_pc"`` and ``"ref_pc_q"``, the generated and reference query
    clouds, as clones: on the replay path they are the graph's static output buffers, which the next replay overwrites.
    Without any of these ``__call__`` returns what ``_item`` returns."""

    _KEYS = ("xs", "xq", "xad", "pcs", "pcq", "pcad")

    def __init__(self, model, graph: bool | None = None, exact_emd: bool = False, return_clouds: bool = False,
                 fscore=None, dcd=None):
        self.model = model
        self.exact_emd = bool(exact_emd)
        self.return_clouds = bool(return_clouds)
        self.fscore = None if fscore is None else check_thresholds(fscore)
        self.dcd = None if dcd is None else check_dcd_alpha(dcd)
        self._columns = eval_report.item_columns(self.exact_emd, self.fscore, self.dcd)
        self._needs_rows = any(c.needs_rows for c in self._columns)
        on_gpu = next(model.parameters()).is_cuda
        if graph is None:
            graph = os.environ.get("FPSG_EVAL_GRAPH", "1") != "0"
        self.use_graph = bool(graph) and on_gpu
        self._graphs = {}
        self._eager = {}
        self._block = None

    def __enter__(self):
        # constant: weights and running statistics stay as they are for the block's whole life, so a capture inside may
        # read what the eager items before it left in the block's cache (transformed filters, stacked decoder weights,
        # BatchNorm coefficients): none of those launches is in the graph
        self._block = winograd.weights_frozen(constant=True)
        self._block.__enter__()
        self._no_grad = torch.no_grad()
        self._no_grad.__enter__()
        return self

    def __exit__(self, *exc):
        self._graphs.clear()            # they read tensors of the block's cache, which ends here
        self._eager.clear()
        self._no_grad.__exit__(*exc)
        self._block.__exit__(*exc)
        self._block = None
        return False

    def _default_metrics(self) -> bool:
        from .metrics import chamfer_distance
        from .utils import emd_wrapper
        return self.model.emd_metric is emd_wrapper and self.model.pc_metric is chamfer_distance

    def __call__(self, sample):
        if not self._columns and not self.return_clouds:
            return self._item(sample)
        out = self._item(sample, clouds=True)
        syn_pc, ref_pc_q = out.pop("syn_pc"), out.pop("ref_pc_q")
        gen, ref = syn_pc.contiguous(), ref_pc_q.contiguous()
        rows = nearest_rows(gen, ref) if self._needs_rows else None
        for column in self._columns:
            out.update(column.per_item(gen, ref, rows))
        if self.return_clouds:
            out["syn_pc"], out["ref_pc_q"] = syn_pc.clone(), ref_pc_q.clone()
        return out

    def _item(self, sample, clouds: bool = False):
        from .metrics import sinkhorn_divergence
        model = self.model
        if self._block is None:
            raise RuntimeError("EvalItem: call it inside its `with` block")
        if not self.use_graph or not self._default_metrics() or model.training:
            return model._return_reconstruction(sample, return_clouds=clouds)
        key = tuple((k, tuple(sample[k].shape)) for k in self._KEYS)
        if key not in self._graphs:
            n = self._eager.get(key, 0)
            if n < 2:
                self._eager[key] = n + 1
                return model._return_reconstruction(sample, return_clouds=clouds)
            # (pruned evaluation reads only the query images and the support / query clouds: the other three inputs --
            # 2 x 19 MB of images at 32 shots -- are neither cloned nor copied per item)
            used = ("xq", "pcs", "pcq") if model._eval_prune() else self._KEYS
            static = {k: (sample[k].clone() if k in used else sample[k]) for k in self._KEYS}
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, capture_error_mode="thread_local"):
                outs = model._reconstruct_for_eval(static)
            self._graphs[key] = (g, {k: static[k] for k in used}, outs)
        g, static, (syn_pc, ref_pc_q, cd_loss, diameter) = self._graphs[key]
        for k, buf in static.items():
            buf.copy_(sample[k], non_blocking=True)
        winograd.check_bank_before_replay()
        g.replay()
        emd = sinkhorn_divergence(syn_pc, ref_pc_q, diameter=float(diameter)).sum()      # emd_wrapper's value
        if clouds:
            return {"cd_loss": cd_loss.clone(), "emd_loss": emd, "syn_pc": syn_pc, "ref_pc_q": ref_pc_q}
        return {"cd_loss": cd_loss.clone(), "emd_loss": emd}
