"""Gradient-norm clipping (K20): what needs no GPU -- the ``--clip_grad_norm`` flag, ``FlatAdam``'s
argument check, the C entries' refusals, the workspace size, and ``TrainStep``'s semantics on a CPU optimizer (the norm
of the MEAN gradient of the step's episodes is what gets clipped)."""
import copy
import ctypes
import math
import os

import numpy as np
import pytest
import torch
import torch.nn as nn

from conftest import ROOT


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    if not os.path.exists(os.path.join(ROOT, "fpsg_amd", "libfpsg_hip.so")):
        g.build()
    from fpsg_amd import _hip
    return _hip.load()


# ---- 1. the flag -------------------------------------------------------------------------------------------------

def test_flag_parses_and_defaults_to_off():
    from fpsg_amd import cli
    from fpsg_amd.engine import default_options
    p = cli.few_shot_parser()
    base = vars(p.parse_args([]))
    assert base["clip_grad_norm"] == 0.0 and type(base["clip_grad_norm"]) is float
    on = vars(p.parse_args(["--clip_grad_norm", "0.5"]))
    assert on["clip_grad_norm"] == 0.5
    assert {k: v for k, v in on.items() if k != "clip_grad_norm"} == {k: v for k, v in base.items() if k != "clip_grad_norm"}
    assert p.parse_args(["--clip_grad_norm", "inf"]).clip_grad_norm == math.inf        # accepted: never clips
    for bad in ("-1", "nan", "-inf", "x", "-0.5"):
        with pytest.raises(SystemExit):
            p.parse_args(["--clip_grad_norm", bad])
    with pytest.raises(SystemExit):
        p.parse_args(["--clip_grad_norm"])
    assert default_options().clip_grad_norm == 0.0


# ---- 2. FlatAdam's argument ----------------------------------------------------------------------------------------

def test_flat_adam_checks_the_threshold_before_the_device():
    from fpsg_amd.optim import FlatAdam, check_max_grad_norm
    params = [nn.Parameter(torch.zeros(3))]                          # CPU parameters: a good threshold reaches the device check
    for bad in (-1, -1e-30, float("nan"), -math.inf, "1", [1.0], True):
        with pytest.raises(ValueError, match="max_grad_norm"):
            FlatAdam(params, max_grad_norm=bad)
    for good in (None, 0, 0.0, 1.0, math.inf, 3):
        with pytest.raises(ValueError, match="ROCm"):
            FlatAdam(params, max_grad_norm=good)
    assert check_max_grad_norm(None) is None and check_max_grad_norm(0) is None and check_max_grad_norm(math.inf) is None
    assert check_max_grad_norm(2) == 2.0 and type(check_max_grad_norm(2)) is float
    assert check_max_grad_norm(np.float32(0.5)) == 0.5


def test_build_optimizer_passes_the_option_through():
    from fpsg_amd.engine import build_optimizer, default_options
    net = nn.Linear(3, 2)
    for sgd in (False, True):
        o, _ = build_optimizer(net, default_options(SGD=sgd))
        assert getattr(o, "max_grad_norm", None) is None
        o, _ = build_optimizer(net, default_options(SGD=sgd, clip_grad_norm=0.25))
        assert o.max_grad_norm == 0.25
        assert "max_grad_norm" not in o.param_groups[0] and "max_grad_norm" not in o.state_dict()["param_groups"][0]
    with pytest.raises(ValueError):
        build_optimizer(net, default_options(clip_grad_norm=-1.0))


# ---- 3. the C entries ----------------------------------------------------------------------------------------------

def test_workspace_size(lib):
    ws = lib.fpsg_grad_norm_workspace_bytes
    assert ws(0) == 0
    sizes = [ws(n) for n in (1, 3, 4, 5, 1023, 1024, 1025, 100003, 1 << 20, 1 << 22, (1 << 22) + 7, 77445125, 1 << 33)]
    assert all(a <= b for a, b in zip(sizes, sizes[1:])) and sizes[0] == 8
    assert all(s % 8 == 0 for s in sizes)
    assert ws(100003) == 8 * -(-(100003 // 4 + 1) // 256)           # one partial per workgroup of 256 vector slots
    assert ws(77445125) == ws(1 << 33) == 8 * 256 * 16              # the grid cap


def test_clip_entries_check_their_arguments_on_the_host(lib):
    """Every refusal comes before any HIP call (no GPU here), with its code and a message."""
    f = ctypes.c_float
    P, Q4, Q2 = 0x10000, 0x10004, 0x10002                           # never dereferenced: aligned / 4-byte / misaligned fakes
    null, shape, align = -1, -2, -3
    n = 100003
    need = lib.fpsg_grad_norm_workspace_bytes(n)

    def flat(grad=P, n=n, s=1.0, mx=1.0, ws=P, wsb=need, out=P, stats=P):
        return lib.fpsg_grad_clip_scale(grad, n, f(s), f(mx), ws, wsb, out, stats, None)

    def seg(tab=P, off=P, nseg=3, n=n, s=1.0, mx=1.0, ws=P, wsb=need, out=P, stats=P):
        return lib.fpsg_grad_clip_scale_segments(tab, off, nseg, n, f(s), f(mx), ws, wsb, out, stats, None)

    for call, name in ((flat, b"fpsg_grad_clip_scale"), (seg, b"fpsg_grad_clip_scale_segments")):
        def refused(code, **kw):
            assert call(**kw) == code, (name, kw)
            msg = lib.fpsg_last_error()
            assert msg and name in msg, (name, kw, msg)
        refused(shape, n=0)
        refused(null, ws=None)
        refused(null, out=None)
        refused(shape, wsb=need - 8)
        refused(shape, wsb=0)
        refused(align, ws=Q4)
        refused(align, stats=Q4)
        refused(align, out=Q2)
        for mx in (-1.0, -1e-30, float("nan"), -math.inf):
            refused(shape, mx=mx)
            assert b"max_norm" in lib.fpsg_last_error()
        for s in (math.inf, -math.inf, float("nan")):
            refused(shape, s=s)
            assert b"grad_scale" in lib.fpsg_last_error()
    assert flat(grad=None) == null and b"grad" in lib.fpsg_last_error()
    assert flat(grad=Q4) == align and b"16-byte" in lib.fpsg_last_error()
    assert seg(tab=None) == null and seg(off=None) == null
    assert seg(nseg=0) == shape and seg(nseg=-2) == shape


def test_dscale_entries_check_their_arguments_on_the_host(lib):
    f = ctypes.c_float
    P, Q4 = 0x10000, 0x10004
    hyper = (f(1e-3), f(0.9), f(0.999), f(1e-8))

    def flat(param=P, grad=P, n=8, step=1, scale=P):
        return lib.fpsg_adam_step_dscale(param, grad, P, P, n, *hyper, step, scale, None)

    def seg(param=P, tab=P, nseg=2, n=8, step=1, scale=P):
        return lib.fpsg_adam_step_segments_dscale(param, tab, P, nseg, P, P, n, *hyper, step, scale, None)

    for call, name in ((flat, b"fpsg_adam_step_dscale"), (seg, b"fpsg_adam_step_segments_dscale")):
        for code, kw in ((-2, {"n": 0}), (-2, {"step": 0}), (-1, {"param": None}), (-3, {"param": Q4}), (-1, {"scale": None}),
                         (-3, {"scale": 0x10002})):
            assert call(**kw) == code, (name, kw)
            assert name in lib.fpsg_last_error(), (name, kw)
    assert flat(grad=None) == -1 and flat(grad=Q4) == -3
    assert seg(tab=None) == -1 and seg(nseg=0) == -2
    # the plain entries answer as before
    assert lib.fpsg_adam_step(None, P, P, P, 8, *hyper, 1, f(1.0), None) == -1
    assert b"fpsg_adam_step: null pointer 'param'" in lib.fpsg_last_error()
    assert lib.fpsg_adam_step(P, P, P, P, 0, *hyper, 1, f(1.0), None) == -2
    assert b"fpsg_adam_step: n must be positive" in lib.fpsg_last_error()


# ---- 4. TrainStep on a CPU optimizer ---------------------------------------------------------------------------------

class _Tiny(nn.Module):
    """The smallest thing ``TrainStep`` drives: ``loss(sample)`` returns a dict with ``ttl_loss``."""

    def __init__(self):
        super().__init__()
        torch.manual_seed(0)
        self.net = nn.Sequential(nn.Linear(7, 13), nn.Tanh(), nn.Linear(13, 5))

    def loss(self, sample):
        return {"ttl_loss": (self.net(sample["x"]) - sample["y"]).square().sum()}


def _episodes():
    g = torch.Generator().manual_seed(5)
    return [{"x": torch.randn(11, 7, generator=g), "y": torch.randn(11, 5, generator=g) * 3} for _ in range(2)]


def _reference_step(model, episodes, max_norm):
    """The same backward passes, their mean, clip_grad_norm_, Adam.step -- written out."""
    ref = copy.deepcopy(model)
    opt = torch.optim.Adam(ref.parameters(), lr=1e-3, betas=(0.9, 0.999))
    grads = []
    for ep in episodes:
        ref.zero_grad(set_to_none=True)
        ref.loss(ep)["ttl_loss"].backward()
        grads.append([p.grad.clone() for p in ref.parameters()])
    for p, *gs in zip(ref.parameters(), *grads):
        p.grad = sum(gs[1:], gs[0]) / len(gs)
    norm = float(torch.sqrt(sum((p.grad.double() ** 2).sum() for p in ref.parameters())))
    if max_norm is not None:
        torch.nn.utils.clip_grad_norm_(list(ref.parameters()), max_norm)
    opt.step()
    return ref, norm


def _train_step(model, episodes, clip):
    from fpsg_amd.engine import TrainStep, build_optimizer, default_options
    m = copy.deepcopy(model)
    optimizer, _ = build_optimizer(m, default_options(lr=1e-3, clip_grad_norm=clip))
    assert isinstance(optimizer, torch.optim.Adam)
    step = TrainStep(m, optimizer)
    step(episodes, n_episodes_global=len(episodes))
    return m, step


def test_train_step_clips_the_mean_gradient_on_a_cpu_optimizer():
    model, episodes = _Tiny(), _episodes()
    _, norm = _reference_step(model, episodes, None)
    assert norm > 1.0                                                 # (the thresholds below are far from it)
    # far below the observed norm: the step of the hand-written reference (test_model_cpu.py's rtol, no atol)
    low = norm / 50
    ref, _ = _reference_step(model, episodes, low)
    got, step = _train_step(model, episodes, low)
    for a, b in zip(got.parameters(), ref.parameters()):
        np.testing.assert_allclose(a.detach().numpy(), b.detach().numpy(), rtol=1e-6)
    assert abs(float(step.last_grad_norm) - norm) <= 1e-5 * norm      # the norm of the MEAN, not of the sum
    assert step.clip_stats() == {"steps": 1, "clipped": 1, "nonfinite": 0, "max_norm_seen": pytest.approx(norm, rel=1e-5)}
    assert step.clip_stats()["steps"] == 0                            # reset by the read
    # ... and it is a different step from the unclipped one
    plain, _ = _train_step(model, episodes, 0.0)
    assert any(not torch.equal(a, b) for a, b in zip(got.parameters(), plain.parameters()))
    # far above: exactly the unclipped step
    high, step_high = _train_step(model, episodes, norm * 50)
    for a, b in zip(high.parameters(), plain.parameters()):
        assert torch.equal(a, b)
    assert step_high.clip_stats(reset=False)["clipped"] == 0 and step_high.clip_stats()["steps"] == 1
    # off: nothing is computed or counted
    _, step_off = _train_step(model, episodes, 0.0)
    assert step_off.last_grad_norm is None and step_off.clip_stats()["steps"] == 0


def test_train_step_takes_the_threshold_itself():
    from fpsg_amd.engine import TrainStep
    model, episodes = _Tiny(), _episodes()
    opt = torch.optim.SGD(model.parameters(), lr=1e-2)
    with pytest.raises(ValueError):
        TrainStep(model, opt, max_grad_norm=-2.0)
    step = TrainStep(model, opt, max_grad_norm=0.125)
    assert opt.max_grad_norm == 0.125
    step(episodes[:1])
    total = math.sqrt(sum(float((p.grad.double() ** 2).sum()) for p in model.parameters()))
    assert total == pytest.approx(0.125, rel=1e-4)                    # the attached gradients were clipped in place
    assert step.clip_stats()["clipped"] == 1
