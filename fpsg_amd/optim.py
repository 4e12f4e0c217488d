"""Adam over flat buffers (K7): the optimizer step of the train loop as one HBM stream.

``FlatAdam`` is ``torch.optim.Adam(lr, betas, eps)`` as the reference configures it
(``src/trainNetwork.py:118-123``: no weight decay, no amsgrad) for a model whose parameters all
live on one ROCm device in fp32.  At construction the parameters are re-pointed into ONE flat
buffer (``p.data`` becomes a view; values, ``Parameter`` objects and state-dict keys are
untouched), the two moments are flat buffers of the same layout, and ``step()`` is a single
launch of ``fpsg_adam_step`` (4 reads + 3 writes per element) instead of a multi-tensor sweep
over ~600 tensors.  The layout is that of ``fpsg_amd.dist.FlatGradBuckets`` (``flat_layout``), so
the step's flat gradient buffer is consumed in place.  Gradients that are NOT views of a bound flat
buffer -- a step of one episode on one rank leaves them where autograd put them -- are read through
a table of per-parameter pointers (``fpsg_adam_step_segments``: no 310 MB gather); only
non-contiguous gradients are first gathered with one multi-tensor copy.

It is a ``torch.optim.Optimizer``: ``param_groups[0]['lr']`` (StepLR), ``state_dict()`` /
``load_state_dict()`` (per-parameter ``step`` / ``exp_avg`` / ``exp_avg_sq`` entries, i.e. the
format of ``torch.optim.Adam``) keep working.  A parameter without a gradient counts as a zero
gradient (torch skips it): with the flat gradient buffer of the train step every parameter has one.

``max_grad_norm`` (K20): ``torch.nn.utils.clip_grad_norm_`` in front of the step, without its read-modify-write pass
over the gradient and without a host read -- one read of the gradient for the norm (``fpsg_grad_clip_scale``), the clip
coefficient folded into the factor the step multiplies the gradient by anyway, taken from device memory
(``fpsg_adam_step_dscale``).  The norm is that of ``grad_scale * grad``, the gradient the update uses: under
``TrainStep``'s folded ``1/E`` the MEAN over the step's episodes, so a threshold means the same for any number of
episodes per step.  (``p.grad`` itself holds their SUM after such a step: ``clip_grad_norm_`` called on it would clip
at ``E`` times the wrong threshold.)  ``last_grad_norm`` and ``clip_stats()`` report what happened.

``attach_ema`` (K23): an exponential moving average of the weights (``fpsg_amd.ema.WeightEma``) as a fifth flat buffer
of the same layout, updated inside the step's one stream from the parameters it has just computed
(``fpsg_adam_step_ema``: 36 B per parameter instead of 28, no second launch).  A step without an attached average calls
exactly what it called before.
"""
from __future__ import annotations

import math
import numbers

import torch
from torch.optim import Optimizer

from . import _hip


def layout_order(params):
    """The parameters in the order of the flat buffers: reverse registration order (the order in which gradients
    become ready in backward), except that a *stack group* -- parameters tagged ``_fpsg_stack = (group, index, n)``
    by a module that evaluates them as one stacked tensor (``PCDecoder``: the same layer of its 16 patch MLPs) -- is
    placed whole, in index order, where its first member falls.  Densely packed, the members of a group are then the
    rows of a contiguous ``[n, ...]`` tensor inside the flat buffer: stacking them is a view.  A group that is
    incomplete among ``params`` (or whose members differ in shape) is not kept together."""
    params = list(params)
    groups = {}
    for p in params:
        tag = getattr(p, "_fpsg_stack", None)
        if tag is not None:
            groups.setdefault(tag[0], []).append((tag[1], p))
    out, placed = [], set()
    for p in reversed(params):
        if id(p) in placed:
            continue
        members = [p]
        tag = getattr(p, "_fpsg_stack", None)
        if tag is not None:
            g = sorted(groups[tag[0]], key=lambda t: t[0])
            if len(g) == tag[2] and [i for i, _ in g] == list(range(tag[2])) and all(m.shape == p.shape for _, m in g):
                members = [m for _, m in g]
        for m in members:
            out.append(m)
            placed.add(id(m))
    return out


def flat_layout(params):
    """``[(param, offset, numel)]`` of the flat buffers: ``layout_order``, densely packed."""
    out, off = [], 0
    for p in layout_order(params):
        out.append((p, off, p.numel()))
        off += p.numel()
    return out, off


def check_max_grad_norm(value, name: str = "max_grad_norm"):
    """The clipping threshold as a float, or None where it means no clipping (``None``, ``0``, ``inf``); ``ValueError``
    for a negative number, NaN or something that is no number."""
    if value is None:
        return None
    if isinstance(value, bool) or not isinstance(value, numbers.Real):
        raise ValueError(f"{name}: a non-negative number or None, got {value!r}")
    value = float(value)
    if math.isnan(value) or value < 0:
        raise ValueError(f"{name}: a non-negative number or None, got {value!r}")
    return None if value == 0 or math.isinf(value) else value


class FlatAdam(Optimizer):
    def __init__(self, params, lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8, max_grad_norm=None):
        # (not a hyper-parameter of the group: param_groups and state_dict keep torch.optim.Adam's entries)
        self.max_grad_norm = check_max_grad_norm(max_grad_norm, "FlatAdam: max_grad_norm")
        if lr < 0 or eps < 0 or not (0 <= betas[0] < 1) or not (0 <= betas[1] < 1):
            raise ValueError("FlatAdam: invalid lr / eps / betas")
        super().__init__(params, dict(lr=lr, betas=tuple(betas), eps=eps))
        if len(self.param_groups) != 1:
            raise ValueError("FlatAdam: one parameter group (the reference's configuration)")
        ps = [p for p in self.param_groups[0]["params"] if p.requires_grad]
        if not ps:
            raise ValueError("FlatAdam: no trainable parameters")
        dev = ps[0].device
        if dev.type != "cuda" or any(p.device != dev or p.dtype != torch.float32 for p in ps):
            raise ValueError("FlatAdam: all parameters must be fp32 on one ROCm device")
        self._layout, total = flat_layout(ps)
        self.flat_param = torch.empty(total, dtype=torch.float32, device=dev)
        self.flat_exp_avg = torch.zeros(total, dtype=torch.float32, device=dev)
        self.flat_exp_avg_sq = torch.zeros(total, dtype=torch.float32, device=dev)
        self._gather = None                    # private flat gradient buffer (non-contiguous gradients)
        self._bound = None                     # the train step's flat gradient buffer
        offs = [off for _, off, _ in self._layout] + [total]
        self._seg_off = torch.tensor(offs, dtype=torch.int64, device=dev)
        self._gtab = torch.zeros(len(self._layout), dtype=torch.int64, device=dev)
        self._gtab_host = None                 # the pointers currently in _gtab
        self._t = 0
        self.grad_scale = 1.0                  # multiplies the gradient as the step reads it (TrainStep: 1/E, then reset)
        self._step_tensor = torch.zeros((), dtype=torch.float32)       # shared by every state entry
        self._clip = None                      # K20's buffers: (workspace, out2, stats), made by the first clipped step
        self.ema = None                        # K23: the attached WeightEma, its shadow in flat_ema
        self.flat_ema = None
        with torch.no_grad():
            for p, off, n in self._layout:
                view = self.flat_param[off:off + n].view(p.shape)
                view.copy_(p.data)
                p.data = view
                self.state[p] = {"step": self._step_tensor,
                                 "exp_avg": self.flat_exp_avg[off:off + n].view(p.shape),
                                 "exp_avg_sq": self.flat_exp_avg_sq[off:off + n].view(p.shape)}

    # ------------------------------------------------------------------ gradients
    def bind_gradients(self, flat_grad: torch.Tensor) -> None:
        """``flat_grad``: a flat buffer with ``flat_layout`` of the same parameters (FlatGradBuckets)."""
        if flat_grad.numel() != self.flat_param.numel() or flat_grad.device != self.flat_param.device:
            raise ValueError("FlatAdam.bind_gradients: buffer does not match the parameter layout")
        self._bound = flat_grad

    def _bound_gradient(self):
        first, off0, _ = self._layout[0]
        last, off1, _ = self._layout[-1]
        b = self._bound
        if (b is not None and first.grad is not None and last.grad is not None
                and first.grad.data_ptr() == b.data_ptr() + 4 * off0 and last.grad.data_ptr() == b.data_ptr() + 4 * off1):
            return b
        return None

    def _pointer_table(self):
        """Device table of the parameters' gradient pointers (0 = no gradient), or None when a
        gradient cannot be read in place (not contiguous fp32 on the parameters' device)."""
        dev = self.flat_param.device
        ptrs = []
        for p, _, n in self._layout:
            g = p.grad
            if g is None:
                ptrs.append(0)
            elif g.dtype == torch.float32 and g.device == dev and g.is_contiguous() and g.numel() == n:
                ptrs.append(g.data_ptr())
            else:
                return None
        if ptrs != self._gtab_host:
            # a fresh pinned tensor per change: the caching host allocator keeps it until the copy ran
            self._gtab.copy_(torch.tensor(ptrs, dtype=torch.int64).pin_memory(), non_blocking=True)
            self._gtab_host = ptrs
        return self._gtab

    def _flat_gradient(self) -> torch.Tensor:
        b = self._bound_gradient()
        if b is not None:
            return b
        if self._gather is None:
            self._gather = torch.zeros_like(self.flat_param)
        dst, src, missing = [], [], []
        for p, off, n in self._layout:
            view = self._gather[off:off + n].view(p.shape)
            (missing if p.grad is None else dst).append(view)
            if p.grad is not None:
                src.append(p.grad)
        if dst:
            torch._foreach_copy_(dst, src)
        if missing:
            torch._foreach_zero_(missing)
        return self._gather

    # ------------------------------------------------------------------------ step
    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        group = self.param_groups[0]
        first = self._layout[0][0]
        if first.data_ptr() != self.flat_param.data_ptr() + 4 * self._layout[0][1]:
            raise RuntimeError("FlatAdam: the parameters were moved off the flat buffer (model.to() / "
                               "a new .data after the optimizer was built); rebuild the optimizer")
        g = self._bound_gradient()
        table = self._pointer_table() if g is None else None
        if g is None and table is None:
            g = self._flat_gradient()
        self._t += 1
        self._step_tensor.fill_(float(self._t))
        lib = _hip.load()
        if self.ema is not None:
            _hip.check(self._ema_step(lib, group, g, table), "fpsg_adam_step_ema")
            self.ema.updates += 1
            return loss
        if check_max_grad_norm(self.max_grad_norm, "FlatAdam: max_grad_norm") is not None:
            _hip.check(self._clipped_step(lib, group, g, table), "fpsg_adam_step (clipped)")
            return loss
        hyper = (float(group["lr"]), float(group["betas"][0]), float(group["betas"][1]), float(group["eps"]), self._t,
                 float(self.grad_scale), _hip.stream_of(self.flat_param))
        with torch.cuda.device(self.flat_param.device):
            if g is not None:
                rc = lib.fpsg_adam_step(_hip.ptr(self.flat_param), _hip.ptr(g), _hip.ptr(self.flat_exp_avg),
                                        _hip.ptr(self.flat_exp_avg_sq), self.flat_param.numel(), *hyper)
            else:
                rc = lib.fpsg_adam_step_segments(_hip.ptr(self.flat_param), _hip.ptr(table), _hip.ptr(self._seg_off),
                                                 len(self._layout), _hip.ptr(self.flat_exp_avg),
                                                 _hip.ptr(self.flat_exp_avg_sq), self.flat_param.numel(), *hyper)
        _hip.check(rc, "fpsg_adam_step")
        return loss

    # ------------------------------------------------------------------ clipping (K20)
    def _clip_buffers(self):
        if self._clip is None:
            dev = self.flat_param.device
            nbytes = int(_hip.load().fpsg_grad_norm_workspace_bytes(self.flat_param.numel()))
            self._clip = (torch.empty(nbytes // 8, dtype=torch.float64, device=dev),
                          torch.zeros(2, dtype=torch.float32, device=dev),
                          torch.zeros(4, dtype=torch.float64, device=dev))
        return self._clip

    def _clipped_step(self, lib, group, g, table) -> int:
        """The norm of ``grad_scale * grad`` and the factor ``grad_scale * coef`` into ``out2``, then the step that reads
        the factor from there: three launches, nothing read by the host."""
        ws, out2, stats = self._clip_buffers()
        n, stream = self.flat_param.numel(), _hip.stream_of(self.flat_param)
        tail = (float(self.grad_scale), float(self.max_grad_norm), _hip.ptr(ws), ws.numel() * 8, _hip.ptr(out2),
                _hip.ptr(stats), stream)
        hyper = (float(group["lr"]), float(group["betas"][0]), float(group["betas"][1]), float(group["eps"]), self._t,
                 _hip.ptr(out2) + 4, stream)
        with torch.cuda.device(self.flat_param.device):
            if g is not None:
                rc = lib.fpsg_grad_clip_scale(_hip.ptr(g), n, *tail)
                return rc or lib.fpsg_adam_step_dscale(_hip.ptr(self.flat_param), _hip.ptr(g), _hip.ptr(self.flat_exp_avg),
                                                       _hip.ptr(self.flat_exp_avg_sq), n, *hyper)
            rc = lib.fpsg_grad_clip_scale_segments(_hip.ptr(table), _hip.ptr(self._seg_off), len(self._layout), n, *tail)
            return rc or lib.fpsg_adam_step_segments_dscale(_hip.ptr(self.flat_param), _hip.ptr(table),
                                                            _hip.ptr(self._seg_off), len(self._layout),
                                                            _hip.ptr(self.flat_exp_avg), _hip.ptr(self.flat_exp_avg_sq),
                                                            n, *hyper)

    # ------------------------------------------------------------------ weight average (K23)
    def attach_ema(self, ema) -> None:
        """``ema``: a ``fpsg_amd.ema.WeightEma`` over this optimizer's parameters.  Its shadow moves into ``flat_ema`` (the
        layout of ``flat_param``, per-parameter views like the moments') and every later ``step()`` updates it."""
        if self.ema is not None:
            raise RuntimeError("FlatAdam.attach_ema: an average is already attached")
        if len(ema.params) != len(self._layout) or any(a is not b for a, (b, _, _) in zip(ema.params, self._layout)):
            raise ValueError("FlatAdam.attach_ema: the average was not built over this optimizer's trainable parameters")
        self.flat_ema = torch.empty_like(self.flat_param)
        views = []
        with torch.no_grad():
            for (p, off, n), e in zip(self._layout, ema.shadow):
                view = self.flat_ema[off:off + n].view(p.shape)
                view.copy_(e)
                views.append(view)
        ema._bind_flat(self.flat_param, self.flat_ema, views)
        self.ema = ema

    def _ema_step(self, lib, group, g, table) -> int:
        """The step with the shadow's update in it: the plain and the clipped form (K20's norm and factor in front, the
        factor then read from device memory) through the same pair of entries."""
        n, stream = self.flat_param.numel(), _hip.stream_of(self.flat_param)
        scale_dev = None
        with torch.cuda.device(self.flat_param.device):
            if check_max_grad_norm(self.max_grad_norm, "FlatAdam: max_grad_norm") is not None:
                ws, out2, stats = self._clip_buffers()
                tail = (float(self.grad_scale), float(self.max_grad_norm), _hip.ptr(ws), ws.numel() * 8, _hip.ptr(out2),
                        _hip.ptr(stats), stream)
                if g is not None:
                    rc = lib.fpsg_grad_clip_scale(_hip.ptr(g), n, *tail)
                else:
                    rc = lib.fpsg_grad_clip_scale_segments(_hip.ptr(table), _hip.ptr(self._seg_off), len(self._layout), n,
                                                           *tail)
                if rc:
                    return rc
                scale_dev = _hip.ptr(out2) + 4
            hyper = (float(group["lr"]), float(group["betas"][0]), float(group["betas"][1]), float(group["eps"]), self._t,
                     float(self.grad_scale), scale_dev, self.ema.next_weight(), stream)
            if g is not None:
                return lib.fpsg_adam_step_ema(_hip.ptr(self.flat_param), _hip.ptr(g), _hip.ptr(self.flat_exp_avg),
                                              _hip.ptr(self.flat_exp_avg_sq), _hip.ptr(self.flat_ema), n, *hyper)
            return lib.fpsg_adam_step_segments_ema(_hip.ptr(self.flat_param), _hip.ptr(table), _hip.ptr(self._seg_off),
                                                   len(self._layout), _hip.ptr(self.flat_exp_avg),
                                                   _hip.ptr(self.flat_exp_avg_sq), _hip.ptr(self.flat_ema), n, *hyper)

    @property
    def last_grad_norm(self):
        """The norm of the last clipped step's gradient (``grad_scale`` included) as a 0-dim device tensor: a view of the
        kernel's output, read without a synchronisation and overwritten by the next step.  None before the first one."""
        return None if self._clip is None else self._clip[1][0]

    def clip_stats(self, reset: bool = True) -> dict:
        """Counters of the clipped steps since the last reset -- the one host read of K20: ``steps``, ``clipped`` (the
        coefficient was below 1), ``nonfinite`` (the norm was inf or NaN) and ``max_norm_seen`` (over the finite norms)."""
        if self._clip is None:
            return {"steps": 0, "clipped": 0, "nonfinite": 0, "max_norm_seen": 0.0}
        s = self._clip[2].tolist()
        if reset:
            self._clip[2].zero_()
        return {"steps": int(s[0]), "clipped": int(s[1]), "nonfinite": int(s[2]), "max_norm_seen": float(s[3])}

    # ------------------------------------------------------------------ state dict
    def load_state_dict(self, state_dict) -> None:
        super().load_state_dict(state_dict)
        t = 0
        with torch.no_grad():
            for p, off, n in self._layout:
                st = self.state.get(p, {})
                for key, flat in (("exp_avg", self.flat_exp_avg), ("exp_avg_sq", self.flat_exp_avg_sq)):
                    view = flat[off:off + n].view(p.shape)
                    if key in st:
                        view.copy_(st[key])
                    else:
                        view.zero_()
                    st[key] = view
                if "step" in st:
                    t = max(t, int(float(st["step"])))
                st["step"] = self._step_tensor
                self.state[p] = st
        self._t = t
        self._step_tensor.fill_(float(t))
