"""Kink-free VGG stages (``conv -> BN -> ReLU -> conv -> BN -> ReLU -> pool``, torchvision ``vgg16_bn.features`` as built at
reference ``src/models/image_net.py:14``) and their float64 truth: torch on the CPU only, no ``fpsg_amd``, no GPU.

A stage-level comparison against float64 at fp32 round-off is normally spoilt by the kink: with a million pre-activations
and fp32 errors of 1e-6 of their scale, about one ReLU mask per layer differs between fp32 and float64, and one flip moves
a weight-gradient row by 1e-3 of its scale.  Here the flips are removed by construction (``construct``):

* the stage input holds integers in {0, 1, 2}, ``w1`` integers in {-1, 0, 1}, ``b1`` small integers, so ``y1`` is
  integer-valued -- exact in fp32 and float64;
* BN1: ``gamma1 = +-s1 sd`` (``s1 = 2^-3``) and the kink ``t = round(m + u sd) + 0.5`` half way between two integers
  (``beta1 = -(t - m) gamma1 / sd``): every ``|y1 - t| >= 0.5`` and ``relu(z1)`` lies on ``s1 x`` half-integers;
* ``w2`` in {-1, 0, 1}, ``b2`` multiples of ``q = s1 / 2``: ``y2`` lies on the lattice ``q``; BN2 puts its kink half way
  between two lattice points the same way, with a random ``gamma2`` in +-[0.5, 2];
* the cotangent given on the pooled output is zero on every 2x2 window whose two largest float64 values differ by less
  than 1e-3 of the largest activation (ties are common on a lattice; all-clipped windows are among them), so the
  gradient routing never depends on a near-tie;
* evaluation mode: the running statistics are the float64 batch statistics, so the same lattice holds.

The affine parameters are rounded to fp32 before anything uses them.  ``truth(name, mode)`` runs three chains on the same
fp32 parameters and caches the result: the literal ``nn.Sequential`` in float64 (the truth), the same modules in fp32
(*lib*: torch's own kernels) and the chain with each convolution replaced by F(4x4, 3x3) in plain differentiable torch ops
(*wino*: what the algorithm's rounding costs, with autograd's Winograd-domain backward).  Neither yardstick is project code.
``deviation(t, t64) = max|t - t64| / max|t64|``."""
from __future__ import annotations

import functools
from types import SimpleNamespace

import torch
import torch.nn as nn
import torch.nn.functional as F

S1 = 2.0 ** -3            # BN1's scale: relu(z1) lies on S1 x half-integers
Q = S1 / 2                # the lattice of y2
EPS = 1e-5                # nn.BatchNorm2d's default
TIE = 1e-3                # pool windows whose two largest values are closer than TIE * max carry no cotangent
MAX_OFFSET = 4.1          # largest |mean| / std of a BatchNorm input channel of the shipped checkpoint (tests/test_maxbwd_gpu.py)
NORTH_STAR = 1e-4
MARGIN_FACTOR = 16.0

# name -> N, C_in, C_mid, C_out, H, W, taps / taps2 (non-zero taps per filter of the sparse ternary w1 / w2: about 10 % / 4 %
# of a 64-channel filter; fewer in w2 keep max|y2| below 19 lattice-margin units, condition 1 of the CPU test), seed
STAGES = {
    "stem": SimpleNamespace(N=6, Cin=3, C1=64, C2=64, H=56, W=56, taps=58, taps2=24, seed=11),
    "stemw": SimpleNamespace(N=6, Cin=3, C1=64, C2=64, H=64, W=64, taps=58, taps2=24, seed=12),
    "s2": SimpleNamespace(N=6, Cin=64, C1=128, C2=128, H=56, W=56, taps=58, taps2=24, seed=13),
    "s3": SimpleNamespace(N=24, Cin=128, C1=128, C2=128, H=28, W=28, taps=58, taps2=24, seed=14),
    "s5": SimpleNamespace(N=88, Cin=64, C1=64, C2=64, H=14, W=14, taps=58, taps2=24, seed=15),
}
CONVS, BNS = ("0", "3"), ("1", "4")


def deviation(t, t64) -> float:
    t64 = t64.detach().double().cpu()
    return float((t.detach().double().cpu() - t64).abs().max()) / (float(t64.abs().max()) + 1e-300)


# ---- F(4x4, 3x3) in plain torch ops -------------------------------------------------------------------------------

_BT = [[4, 0, -5, 0, 1, 0], [0, -4, -4, 1, 1, 0], [0, 4, -4, -1, 1, 0], [0, -2, -1, 2, 1, 0], [0, 2, -1, -2, 1, 0],
       [0, 4, 0, -5, 0, 1]]
_G = [[1 / 4, 0, 0], [-1 / 6, -1 / 6, -1 / 6], [-1 / 6, 1 / 6, -1 / 6], [1 / 24, 1 / 12, 1 / 6], [1 / 24, -1 / 12, 1 / 6],
      [0, 0, 1]]
_AT = [[1, 1, 1, 1, 1, 0], [0, 1, -1, 2, -2, 0], [0, 1, 1, 4, 4, 0], [0, 1, -1, 8, -8, 1]]


def wino_conv3x3(x, w):
    """``F.conv2d(x, w, None, 1, 1)`` as Winograd F(4x4, 3x3): B / G / A transforms as einsums over 6x6 tiles, the channel
    sum in the transform domain; ragged planes are zero-padded to a multiple of 4 and cropped.  In the dtype of ``x``."""
    N, C, H, W = x.shape
    Hp, Wp = -(-H // 4) * 4, -(-W // 4) * 4
    BT, G, AT = (torch.tensor(m, dtype=torch.float64).to(x.dtype) for m in (_BT, _G, _AT))
    d = F.pad(x, (1, 1 + Wp - W, 1, 1 + Hp - H)).unfold(2, 6, 4).unfold(3, 6, 4)           # [N, C, th, tw, 6, 6]
    V = torch.einsum("ai,nchwij,bj->nchwab", BT, d, BT)
    U = torch.einsum("ai,kcij,bj->kcab", G, w, G)
    M = torch.einsum("kcab,nchwab->nkhwab", U, V)
    Y = torch.einsum("ia,nkhwab,jb->nkhiwj", AT, M, AT)                                     # [N, K, th, 4, tw, 4]
    return Y.reshape(N, w.shape[0], Hp, Wp)[:, :, :H, :W]


class WinoConv2d(nn.Conv2d):
    def forward(self, x):
        return wino_conv3x3(x, self.weight) + self.bias.view(1, -1, 1, 1)


def make_stage(p, params: dict, dtype=torch.float32, conv=nn.Conv2d, running: dict | None = None) -> nn.Sequential:
    """The stage as a literal ``nn.Sequential`` (torchvision's numbering within a stage) holding ``params``."""
    seq = nn.Sequential(conv(p.Cin, p.C1, 3, padding=1), nn.BatchNorm2d(p.C1, eps=EPS), nn.ReLU(),
                        conv(p.C1, p.C2, 3, padding=1), nn.BatchNorm2d(p.C2, eps=EPS), nn.ReLU(), nn.MaxPool2d(2, 2))
    seq = seq.to(dtype)
    with torch.no_grad():
        for k, v in params.items():
            seq.get_parameter(k).copy_(v)
        for k, v in (running or {}).items():
            seq.get_buffer(k).copy_(v)
    return seq


# ---- the construction ---------------------------------------------------------------------------------------------

def _ternary(K, C, taps, gen):
    if C == 3:
        return torch.randint(-1, 2, (K, C, 3, 3), generator=gen).double()                  # dense for the 3-channel stem
    keep = torch.rand(K, C, 3, 3, generator=gen) < taps / (9.0 * C)
    sign = torch.randint(0, 2, (K, C, 3, 3), generator=gen) * 2 - 1
    return (keep * sign).double()


def _stats(y):
    m = y.mean((0, 2, 3))
    var = y.var((0, 2, 3), unbiased=False)
    return m, var, (var + EPS).sqrt()


def _f32(t):
    return t.float().double()


@functools.lru_cache(maxsize=None)
def construct(name: str):
    """-> namespace: ``x`` (float64 integers), ``params`` (float64 holding fp32 values, keyed like the Sequential's
    parameters), ``running`` (the float64 batch statistics as fp32 values, for evaluation mode), ``t1`` / ``t2`` (the
    kinks in units of y1 / y2) and the cotangent's random part ``g0``."""
    p = STAGES[name]
    gen = torch.Generator().manual_seed(p.seed)
    x = torch.randint(0, 3, (p.N, p.Cin, p.H, p.W), generator=gen).double()
    w1 = _ternary(p.C1, p.Cin, p.taps, gen)
    b1 = torch.randint(-2, 3, (p.C1,), generator=gen).double()
    y1 = F.conv2d(x, w1, b1, padding=1)
    m1, var1, sd1 = _stats(y1)
    sign = torch.where(torch.rand(p.C1, generator=gen) < 0.3, -1.0, 1.0).double()
    u = torch.rand(p.C1, generator=gen).double() * 2 - 1
    t1 = (m1 + u * sd1).round() + 0.5
    gamma1 = _f32(sign * S1 * sd1)
    beta1 = _f32(-(t1 - m1) * gamma1 / sd1)
    a1 = F.relu((y1 - m1.view(1, -1, 1, 1)) / sd1.view(1, -1, 1, 1) * gamma1.view(1, -1, 1, 1) + beta1.view(1, -1, 1, 1))
    w2 = _ternary(p.C2, p.C1, p.taps2, gen)
    b2 = torch.randint(-4, 5, (p.C2,), generator=gen).double() * Q
    y2 = F.conv2d(a1, w2, b2, padding=1)
    m2, var2, sd2 = _stats(y2)
    u2 = torch.rand(p.C2, generator=gen).double() * 2 - 1
    t2 = (((m2 + u2 * sd2) / Q).round() + 0.5) * Q
    sign2 = torch.where(torch.rand(p.C2, generator=gen) < 0.5, -1.0, 1.0).double()
    gamma2 = _f32(sign2 * (0.5 + 1.5 * torch.rand(p.C2, generator=gen).double()))
    beta2 = _f32(-(t2 - m2) * gamma2 / sd2)
    g0 = _f32(torch.randn(p.N, p.C2, p.H // 2, p.W // 2, generator=gen).double())
    params = {"0.weight": w1, "0.bias": b1, "1.weight": gamma1, "1.bias": beta1,
              "3.weight": w2, "3.bias": b2, "4.weight": gamma2, "4.bias": beta2}
    running = {"1.running_mean": _f32(m1), "1.running_var": _f32(var1), "4.running_mean": _f32(m2), "4.running_var": _f32(var2)}
    return SimpleNamespace(p=p, x=x, params=params, running=running, t1=t1, t2=t2, g0=g0)


# ---- running a chain ----------------------------------------------------------------------------------------------

def run_chain(seq: nn.Sequential, x, g, train: bool, need_dx: bool, keep_inner: bool = True):
    """One forward (+ backward with cotangent ``g`` when given) of a stage -> ``(res, inner)``: ``res`` holds the compared
    tensors (``out``, ``dx``, every parameter's gradient, the BatchNorms' buffers); ``inner`` the pre-BatchNorm tensors
    ``y1`` / ``y2``, the BatchNorm outputs ``z1`` / ``z2`` and the pool's selections ``sel`` (flat index per window)."""
    seq.train(train)
    inner, hooks = {}, []
    if keep_inner:
        for idx, key in ((0, "y1"), (1, "z1"), (3, "y2"), (4, "z2"), (5, "a2")):
            hooks.append(seq[idx].register_forward_hook(lambda _m, _i, o, key=key: inner.__setitem__(key, o.detach())))
    xin = x.clone().requires_grad_(need_dx and g is not None)
    with torch.set_grad_enabled(g is not None):
        out = seq(xin)
    for h in hooks:
        h.remove()
    res = {"out": out.detach()}
    if g is not None:
        out.backward(g)
        if need_dx:
            res["dx"] = xin.grad
        for k, prm in seq.named_parameters():
            res["d " + k] = prm.grad
    for k, b in seq.named_buffers():
        res[k] = b.detach().clone()
    if keep_inner:
        inner["sel"] = F.max_pool2d(inner["a2"], 2, 2, return_indices=True)[1]
    return res, inner


def window_gap(a2):
    """Per 2x2 window: the difference of its two largest values."""
    w = a2.unfold(2, 2, 2).unfold(3, 2, 2).reshape(*a2.shape[:2], a2.shape[2] // 2, a2.shape[3] // 2, 4)
    top = w.topk(2, dim=-1).values
    return top[..., 0] - top[..., 1]


@functools.lru_cache(maxsize=None)
def truth(name: str, mode: str):
    """The float64 chain and the two fp32 yardsticks of stage ``name`` in ``mode`` ('train' / 'eval'), computed once.
    -> namespace: ``x`` / ``g`` / ``params`` / ``running`` (fp32, what every path under test is given), ``t64`` / ``lib`` /
    ``wino`` (compared tensors by name), ``inner64`` / ``inner_lib`` / ``inner_wino``, ``kept`` (windows with a cotangent),
    ``need_dx``."""
    c = construct(name)
    p = c.p
    train = mode == "train"
    need_dx = p.Cin != 3                                   # images carry no gradient
    running = None if train else c.running                 # training starts from the modules' defaults (0, 1)
    seq64 = make_stage(p, c.params, torch.float64, running=running)
    _, first = run_chain(seq64, c.x, None, train, False)
    kept = window_gap(first["a2"]) >= TIE * float(first["a2"].max())
    g = c.g0 * kept
    seq64 = make_stage(p, c.params, torch.float64, running=running)     # (the first pass moved the running statistics)
    t64, inner64 = run_chain(seq64, c.x, g, train, need_dx)
    params32 = {k: v.float() for k, v in c.params.items()}
    running32 = None if running is None else {k: v.float() for k, v in running.items()}
    x32, g32 = c.x.float(), g.float()
    lib, inner_lib = run_chain(make_stage(p, params32, running=running32), x32, g32, train, need_dx)
    wino, inner_wino = run_chain(make_stage(p, params32, conv=WinoConv2d, running=running32), x32, g32, train, need_dx)
    return SimpleNamespace(p=p, mode=mode, x=x32, g=g32, params=params32, running=running32, t64=t64, lib=lib, wino=wino,
                           inner64=inner64, inner_lib=inner_lib, inner_wino=inner_wino, kept=kept, need_dx=need_dx,
                           t1=c.t1, t2=c.t2)


def cancelled(name: str, mode: str) -> bool:
    """A convolution bias in front of a training-mode BatchNorm: its true gradient is exactly cancelled."""
    return mode == "train" and name in ("d 0.bias", "d 3.bias")


def bound(tr, name: str) -> float:
    """What a path under test may deviate from float64 on tensor ``name``: 4 x the worse yardstick + 2e-6 (the factor and
    the floor of ``tests/_gradcheck.py``), and never more than the north-star tolerance."""
    return min(4.0 * max(deviation(tr.lib[name], tr.t64[name]), deviation(tr.wino[name], tr.t64[name])) + 2e-6, NORTH_STAR)


def cancelled_bound(tr, name: str) -> float:
    """``max|d bias|`` allowed where the truth is zero: 10 x the larger yardstick's own round-off + 2e-6 of the gradient of
    the BatchNorm shift behind it."""
    beta = "d 1.bias" if name == "d 0.bias" else "d 4.bias"
    return 10.0 * max(float(tr.lib[name].abs().max()), float(tr.wino[name].abs().max())) + 2e-6 * float(tr.t64[beta].abs().max())
