"""An exponential moving average of the weights (K23): the shadow that is evaluated and saved beside the raw iterate.

``WeightEma(params, decay)`` keeps one fp32 shadow per trainable parameter.  After update number ``t`` (1 for the
first)

    d_t = min(decay, (1 + t) / (10 + t))          the usual warm-up: the average forgets the random initial weights
    w_t = fp32(1 - d_t)                           formed in double, rounded once
    e   = e + w_t * (p - e)

Buffers (the BatchNorm running statistics) are not averaged: a model evaluated on the shadow uses the live ones.

With ``FlatAdam`` the shadow is one flat buffer in the optimizer's layout (``optimizer.attach_ema(ema)``) and the update
is part of the optimizer's one stream over the parameters (``fpsg_adam_step_ema``: the ``p`` the kernel has just
computed, never re-read); ``update()`` is then not to be called.  With any other optimizer -- CPU runs, ``--SGD``,
``FPSG_FLAT_ADAM=0`` -- ``update()`` is one ``torch._foreach_lerp_`` and ``TrainStep`` calls it after
``optimizer.step()``.  Every rank of a distributed run keeps its own shadow: the ranks' parameters are identical and
the update is deterministic, so nothing is communicated.

``swapped()`` exchanges parameters and shadow for the length of a ``with`` block -- contents move, addresses do not,
so views of the flat buffer and captured graphs stay valid.
"""
from __future__ import annotations

import contextlib
import math
import numbers
import struct

import torch

from . import _hip, winograd
from .optim import layout_order


def check_ema_decay(value, name: str = "ema_decay"):
    """The decay as a float in (0, 1), or None where it means no averaging (``None``, ``0``); ``ValueError`` for a
    bool, something that is no number, NaN, a negative value or a value of 1 and above."""
    if value is None:
        return None
    if isinstance(value, bool) or not isinstance(value, numbers.Real):
        raise ValueError(f"{name}: a number in [0, 1) or None, got {value!r}")
    value = float(value)
    if math.isnan(value) or value < 0 or value >= 1:
        raise ValueError(f"{name}: a number in [0, 1) or None, got {value!r}")
    return None if value == 0 else value


def decay_at(decay: float, t: int) -> float:
    """``d_t`` of update number ``t >= 1``."""
    return min(float(decay), (1.0 + t) / (10.0 + t))


def weight_at(decay: float, t: int) -> float:
    """``w_t = 1 - d_t`` in double, rounded to fp32 once (returned as the Python float of that fp32 value)."""
    return struct.unpack("f", struct.pack("f", 1.0 - decay_at(decay, t)))[0]


class WeightEma:
    def __init__(self, params, decay: float):
        decay = check_ema_decay(decay, "WeightEma: decay")
        if decay is None:
            raise ValueError("WeightEma: decay must lie in (0, 1); 0 means no averaging -- build none")
        self.decay = decay
        self.updates = 0
        # the order of the flat buffers, so that entry i of the state dict is the same parameter in either form
        self.params = layout_order([p for p in params if p.requires_grad])
        if not self.params:
            raise ValueError("WeightEma: no trainable parameters")
        self.shadow = [p.detach().clone() for p in self.params]
        self._flat = None           # (flat_param, flat_ema) once a FlatAdam holds the shadow
        self._swapped = False

    # ------------------------------------------------------------------ schedule
    def next_weight(self) -> float:
        """``w_t`` of the update that comes next."""
        return weight_at(self.decay, self.updates + 1)

    # ------------------------------------------------------------------ FlatAdam
    def _bind_flat(self, flat_param: torch.Tensor, flat_ema: torch.Tensor, views) -> None:
        """``FlatAdam.attach_ema``: ``flat_ema`` already holds the shadow, ``views`` are its per-parameter views."""
        self._flat = (flat_param, flat_ema)
        self.shadow = list(views)

    @property
    def fused(self) -> bool:
        return self._flat is not None

    # -------------------------------------------------------------------- update
    @torch.no_grad()
    def update(self) -> None:
        if self._swapped:
            raise RuntimeError("WeightEma.update: inside swapped() the parameters hold the shadow")
        if self._flat is not None:
            raise RuntimeError("WeightEma.update: the shadow lives in FlatAdam's flat buffer and FlatAdam.step() updates it")
        torch._foreach_lerp_(self.shadow, [p.data for p in self.params], self.next_weight())
        self.updates += 1

    # ---------------------------------------------------------------------- swap
    @torch.no_grad()
    def _exchange(self) -> None:
        if self._flat is not None:
            flat_param, flat_ema = self._flat
            if self.params[0].data_ptr() != flat_param.data_ptr():
                raise RuntimeError("WeightEma: the parameters were moved off the optimizer's flat buffer")
            with torch.cuda.device(flat_param.device):
                rc = _hip.load().fpsg_flat_swap(_hip.ptr(flat_param), _hip.ptr(flat_ema), flat_param.numel(),
                                                _hip.stream_of(flat_param))
            _hip.check(rc, "fpsg_flat_swap")
            return
        data = [p.data for p in self.params]
        tmp = [d.clone() for d in data]
        torch._foreach_copy_(data, self.shadow)
        torch._foreach_copy_(self.shadow, tmp)

    @contextlib.contextmanager
    def swapped(self):
        """Inside the block the parameters hold the averaged weights and the shadow the raw ones; they are exchanged back
        on exit, exception or not, and both hold their original bits again.  Derived forms of the weights are cached per
        ``winograd.weights_frozen()`` block, so the swap refuses to start inside one: open such blocks inside it."""
        if winograd.frozen_cache_ro() is not None:
            raise RuntimeError("WeightEma.swapped: entered inside a winograd.weights_frozen() block, whose cache holds "
                               "forms of the weights as they are now; open the block inside swapped() instead")
        if self._swapped:
            raise RuntimeError("WeightEma.swapped: already swapped")
        self._exchange()
        self._swapped = True
        try:
            yield self
        finally:
            self._exchange()
            self._swapped = False

    # ---------------------------------------------------------------- state dict
    def state_dict(self) -> dict:
        return {"decay": self.decay, "updates": self.updates, "shadow": {i: e for i, e in enumerate(self.shadow)}}

    @torch.no_grad()
    def load_state_dict(self, state: dict) -> None:
        """Restores the shadow and the count of updates.  The decay stays the one this object was built with (the
        command line's); the entry records what the saved run used."""
        shadow = state["shadow"]
        if len(shadow) != len(self.shadow):
            raise ValueError(f"WeightEma.load_state_dict: {len(shadow)} shadow tensors for {len(self.shadow)} parameters")
        src = [shadow[i] for i in range(len(self.shadow))]
        for i, (e, s) in enumerate(zip(self.shadow, src)):
            if e.shape != s.shape:
                raise ValueError(f"WeightEma.load_state_dict: entry {i} has shape {tuple(s.shape)}, the parameter "
                                 f"{tuple(e.shape)}")
        for e, s in zip(self.shadow, src):
            e.copy_(s)
        self.updates = int(state["updates"])
