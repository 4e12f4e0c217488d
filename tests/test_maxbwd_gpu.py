"""K5m (csrc/maxbwd.hip, ``fused_bn._ConvBNActMax``): the backward of conv1x1 -> BatchNorm (+act) -> max over the points
through K x K algebra, against a float64 evaluation of the plain chain on the CPU.

Yardstick: the same chain in fp32 on the GPU through ``nn.Conv1d`` / ``nn.BatchNorm1d`` / torch ops (the library, not
this project).  deviation(t) = max|t - t64| / max|t64|; the algebra's deviation must be at most 4x the library chain's on
the same tensor plus 2e-6 (the factor and the floor of tests/_gradcheck.py).  The dense project form
(``FPSG_MAX_BWD_ALGEBRA=0``) is measured and printed beside them; it is not a yardstick.

An arg-max that differs between fp32 and float64 moves one channel's dz between two points, so the float64 gradients are
taken with the selection forced to the kernel's ``idx`` (a gather in place of ``.max``); the selection itself is
bounded separately: at most 1e-4 of the (cloud, channel) pairs differ from the float64 arg-max / arg-min, and where one
does the two candidates' float64 pre-activations lie within 1e-5 of the row's range.

The algebra never forms x' - mean: it lets k2 sum(x' a) and k3 sum(a) cancel, so its error grows with |mean| / std of a
channel.  ``test_offset_ladder`` measures that per channel group (|mean| / std = 0, 1, 10, 100, 1000 and constant
channels); the measurements are kept in profiles/r06/maxbwd_deviation.jsonl together with the largest ratio the shipped
checkpoint produces.  Up to the ladder step at or above that ratio the 4x rule holds per group; above it the recorded
deviation times 3 is a hard ceiling."""
import copy
import json
import os

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from conftest import GOLDEN, unit_ball_clouds

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CKPT = os.path.join(GOLDEN, "pretrained_pcencoder_pointnet.pt")
RECORD = os.path.join(ROOT, "profiles", "r06", "maxbwd_deviation.jsonl")
LADDER = (0.0, 1.0, 10.0, 100.0, 1000.0)
CONST = "const"
FACTOR, FLOOR = 4.0, 2e-6          # tests/_gradcheck.py
EPS32 = 2.0 ** -23


# ---------------------------------------------------------------------------------------------------------------------
# the three fp32 paths and the float64 truth

def _act(y, act):
    if act == "relu":
        return F.relu(y)
    if isinstance(act, tuple):
        return F.leaky_relu(y, act[1])
    return y


def _count_forms(monkeypatch):
    """Which form ran: the one-op algebra (``_ConvBNActMax``), the dense project form (``_BNActMax``), and the calls of
    fpsg_max_bwd_gather on the loaded library object."""
    from fpsg_amd import _hip, fused_bn
    lib = _hip.load()
    seen = {"algebra": 0, "dense": 0, "gather": 0}
    c0, m0, g0 = fused_bn._ConvBNActMax.forward, fused_bn._BNActMax.forward, lib.fpsg_max_bwd_gather

    def c1(*a, **k):
        seen["algebra"] += 1
        return c0(*a, **k)

    def m1(*a, **k):
        seen["dense"] += 1
        return m0(*a, **k)

    def g1(*a):
        seen["gather"] += 1
        return g0(*a)

    monkeypatch.setattr(fused_bn._ConvBNActMax, "forward", staticmethod(c1))
    monkeypatch.setattr(fused_bn._BNActMax, "forward", staticmethod(m1))
    monkeypatch.setattr(lib, "fpsg_max_bwd_gather", g1)
    return seen


def _modules(gpu, W, pb, gamma, beta, rm=None, rv=None, train=True):
    C, K = W.shape
    conv, bn = nn.Conv1d(K, C, 1), nn.BatchNorm1d(C)
    with torch.no_grad():
        conv.weight.copy_(W.reshape(C, K, 1)); conv.bias.copy_(pb)
        bn.weight.copy_(gamma); bn.bias.copy_(beta)
        if rm is not None:
            bn.running_mean.copy_(rm); bn.running_var.copy_(rv)
    return conv.to(gpu), bn.to(gpu).train(train)


class _Run:
    """One forward of one path; ``grads(g)`` may be called several times (one channel group's ``g`` at a time)."""

    def __init__(self, conv, bn, a, act, path, monkeypatch):
        from fpsg_amd.fused_bn import conv_bn_act_max
        self.conv, self.bn = copy.deepcopy(conv), copy.deepcopy(bn)
        self.a = a.clone().requires_grad_()
        if path == "torch":
            self.y = _act(self.bn(self.conv(self.a)), act).max(dim=2)[0]
            self.idx = None
        else:
            monkeypatch.setenv("FPSG_MAX_BWD_ALGEBRA", "1" if path == "algebra" else "0")
            self.y = conv_bn_act_max(self.conv, self.bn, self.a, act)
            saved = getattr(self.y.grad_fn, "saved_tensors", ())
            idx = [t for t in saved if t.dtype == torch.int32]
            self.idx = idx[0].clone() if idx else None

    def grads(self, g):
        C = self.conv.out_channels
        da, dw, dpb, dgamma, dbeta = torch.autograd.grad(self.y, [self.a, self.conv.weight, self.conv.bias, self.bn.weight,
                                                                  self.bn.bias], g, retain_graph=True)
        return {"d input": da, "d weight": dw.reshape(C, -1), "d bias": dpb, "d gamma": dgamma, "d beta": dbeta}

    def forward_tensors(self):
        return {"out": self.y.detach(), "running_mean": self.bn.running_mean, "running_var": self.bn.running_var}


class _Truth:
    """conv1d -> batch_norm -> act -> max in float64 on the CPU, autograd for every gradient; ``forced(idx)`` gathers
    with the kernel's indices instead."""

    def __init__(self, conv, bn, a, act):
        C = conv.out_channels
        d = lambda t: t.detach().double().cpu()
        self.leaves = [d(a).requires_grad_(), d(conv.weight).requires_grad_(), d(conv.bias).requires_grad_(),
                       d(bn.weight).requires_grad_(), d(bn.bias).requires_grad_()]
        self.rm, self.rv = d(bn.running_mean).clone(), d(bn.running_var).clone()
        x = F.conv1d(self.leaves[0], self.leaves[1], self.leaves[2])
        y = F.batch_norm(x, self.rm, self.rv, self.leaves[3], self.leaves[4], bn.training, bn.momentum, bn.eps)
        self.z = _act(y, act)
        self.x = x.detach()
        self.out = self.z.max(dim=2)[0].detach()
        self.C = C
        self.sel = None

    def forced(self, idx):
        self.sel = self.z.gather(2, idx.cpu().long().unsqueeze(2)).squeeze(2)

    def grads(self, g):
        da, dw, dpb, dgamma, dbeta = torch.autograd.grad(self.sel, self.leaves, g.double().cpu(), retain_graph=True)
        return {"d input": da, "d weight": dw.reshape(self.C, -1), "d bias": dpb, "d gamma": dgamma, "d beta": dbeta}

    def forward_tensors(self):
        return {"out": self.out, "running_mean": self.rm, "running_var": self.rv}

    def ratio(self):
        """|mean| / std of x' per channel (biased std; inf where a channel is constant)."""
        m, s = self.x.mean((0, 2)), self.x.std((0, 2), unbiased=False)
        return m.abs() / s

    def check_selection(self, idx, what):
        """The kernel's idx against the float64 arg-max (gamma >= 0) / arg-min (gamma < 0), compared through the values so
        that exact ties count as equal."""
        xs = self.x.gather(2, idx.cpu().long().unsqueeze(2)).squeeze(2)
        hi, lo = self.x.max(dim=2)[0], self.x.min(dim=2)[0]
        ext = torch.where(self.leaves[3].detach() >= 0, hi, lo)
        differs = xs != ext
        frac = float(differs.double().mean())
        gap = (xs - ext).abs()[differs] / (hi - lo)[differs]
        print(f"{what}: idx differs from the float64 selection on {int(differs.sum())} of {differs.numel()} pairs"
              + (f", worst gap {float(gap.max()):.2e} of the row's range" if gap.numel() else ""))
        assert frac <= 1e-4, (what, frac)
        assert bool((gap <= 1e-5).all()), (what, float(gap.max()))


def _dev(got, truth, whole):
    """max|got - truth| / max|truth|; a slice whose float64 value is zero against the whole tensor (``whole``) is
    measured on the whole tensor's scale."""
    t = truth
    s = float(t.abs().max()) if t.numel() else 0.0
    den = s if s > 1e-9 * whole else max(whole, 1e-30)
    return float((got.detach().double().cpu() - t).abs().max()) / den


def _l2(got, truth, whole):
    n = float(truth.norm())
    return float((got.detach().double().cpu() - truth).norm()) / (n if n > 1e-9 * whole else max(whole, 1e-30))


def _append(line):
    """A measuring run names the file to append to in FPSG_MAXBWD_RECORD_OUT; its lines are then kept as
    profiles/r06/maxbwd_deviation.jsonl (the bounds read that committed file, never the run's own output)."""
    out = os.environ.get("FPSG_MAXBWD_RECORD_OUT")
    if out:
        with open(out, "a") as f:
            f.write(json.dumps(line) + "\n")


def _recorded():
    lines = []
    if os.path.exists(RECORD):
        with open(RECORD) as f:
            lines = [json.loads(s) for s in f if s.strip()]
    return lines


def _required_step(lines):
    """The ladder step at or above the largest |mean| / std the shipped checkpoint produces (recorded by case a)."""
    ratios = [ln["checkpoint_max_ratio"] for ln in lines if "checkpoint_max_ratio" in ln]
    assert ratios, f"{RECORD} holds no checkpoint_max_ratio line (test_trained_weights records it)"
    return min(s for s in LADDER if s >= max(ratios))


def _three_way(gpu, monkeypatch, case, conv, bn, a, g, act, groups, expect="algebra", fold=None):
    """Runs the three fp32 paths and the float64 truth, prints the deviation table per channel group and returns
    {group: {tensor: {"algebra": dev, "dense": dev, "torch": dev}}} (L2 deviations under "<tensor> l2").
    ``groups``: [(label, bool mask over the channels)].  ``fold(t)``: applied to the library chain's and the truth's
    d input before they are compared with each other (exact ties: the library may pick another of the tied points)."""
    seen = _count_forms(monkeypatch)
    mode = "train" if bn.training else "eval"
    runs = {}
    for path in ("algebra", "dense", "torch"):
        before = dict(seen)
        runs[path] = _Run(conv, bn, a, act, path, monkeypatch)
        if path == "algebra":
            took = {k: seen[k] - before[k] for k in ("algebra", "dense")}
            if expect == "algebra":
                assert took == {"algebra": 1, "dense": 0}, (case, took)
            else:
                assert took["algebra"] == 0, (case, took)
        elif path == "dense":
            assert seen["algebra"] == before["algebra"], (case, "the dense form was asked for")
    idx = runs["algebra"].idx
    truth = _Truth(conv, bn, a, act)
    if idx is None:         # the library chain ran (no project op at this length): its own selection
        with torch.no_grad():
            x32 = runs["algebra"].conv(a)
        idx = torch.where(bn.weight.detach() >= 0, x32.argmax(dim=2), x32.argmin(dim=2)).int()
    truth.check_selection(idx, f"{case} {mode}")
    truth.forced(idx)
    names = ["d input", "d weight", "d gamma", "d beta"] + (["d bias"] if mode == "eval" else [])
    table = {}
    tf = truth.forward_tensors()
    fwd = {p: r.forward_tensors() for p, r in runs.items()}
    gathers = seen["gather"]
    tgs = {label: truth.grads(g * m.to(g.dtype)) for label, m in groups}
    # a group's slice is measured on its own largest float64 entry; where that is zero (constant channels), on the tensor's
    scale = {n: max(float(t[n].abs().max()) for t in tgs.values()) for n in names}
    norm = {n: max(float(t[n].norm()) for t in tgs.values()) for n in names}
    for label, m in groups:
        mc = m.cpu()
        tg = tgs[label]
        row = {}
        got = {p: r.grads(g * m.to(g.dtype)) for p, r in runs.items()}
        for n in names:
            sl = (lambda t, mk: t) if n == "d input" else (lambda t, mk: t[mk])
            t = sl(tg[n], mc)
            row[n] = {}
            for p in runs:
                q = sl(got[p][n], m)
                tt = t
                if fold is not None and n == "d input" and p == "torch":
                    q, tt = fold(q), fold(t)
                row[n][p] = _dev(q, tt, scale[n])
                if n in ("d input", "d weight"):
                    row.setdefault(n + " l2", {})[p] = _l2(q, tt, norm[n])
        for n in ("out", "running_mean", "running_var"):
            t = tf[n][..., mc]
            row[n] = {p: _dev(fwd[p][n][..., m], t, float(tf[n].abs().max())) for p in runs}
        table[label] = row
        for n, r in row.items():
            print(f"{case} {mode} group {label} {n:13s}: algebra {r['algebra']:.2e}  dense {r['dense']:.2e}  torch chain {r['torch']:.2e}")
    if expect == "algebra":
        assert seen["gather"] - gathers == len(groups), (case, "fpsg_max_bwd_gather calls", seen["gather"] - gathers)
    else:
        assert seen["gather"] == 0, (case, seen)
    return table, truth, idx


def _assert_4x(case, label, row):
    for n, r in row.items():
        assert np.isfinite(r["algebra"]), (case, label, n, r)
        assert r["algebra"] <= FACTOR * r["torch"] + FLOOR, (case, label, n, r)


# ---------------------------------------------------------------------------------------------------------------------
# a. the trained layers the kernel serves

def _trained_inputs(gpu, B, L):
    from fpsg_amd.fused_bn import conv_bn_act
    from fpsg_amd.point_cloud_net import PCEncoder
    enc = PCEncoder("pointnet")
    enc.load_state_dict(torch.load(CKPT, map_location="cpu", weights_only=True), strict=True)
    net = enc.to(gpu).train().pc_encoder.pointnet_feat_extractor
    x = torch.from_numpy(unit_ball_clouds(np.random.default_rng(3), B, L)).transpose(1, 2).contiguous().to(gpu)
    work = copy.deepcopy(net)
    with torch.no_grad():
        trans = work.stn(x)
        h = torch.bmm(trans.transpose(1, 2), x)
        h = conv_bn_act(work.conv1, work.bn1, h, "relu")
        a_main = conv_bn_act(work.conv2, work.bn2, h, "relu").contiguous()
        h = conv_bn_act(work.stn.conv1, work.stn.bn1, x, "relu")
        a_stn = conv_bn_act(work.stn.conv2, work.stn.bn2, h, "relu").contiguous()
    return {"main": (net.conv3, net.bn3, a_main, None), "stn": (net.stn.conv3, net.stn.bn3, a_stn, "relu")}


@pytest.mark.parametrize("mode", ["train", "eval"])
@pytest.mark.parametrize("layer", ["main", "stn"])
def test_trained_weights(gpu, monkeypatch, layer, mode):
    """conv3 / bn3 of pointnet_feat_extractor (no activation) and of its STN (ReLU) from the shipped checkpoint, on the
    activations the encoder's earlier layers produce for 16 unit-ball clouds of 2048 points (above
    ``_MAX_ALGEBRA_MIN_POINTS``: the default dispatch takes the algebra).  Every tensor under the 4x rule, max and L2.
    Records the checkpoint's largest per-channel |mean| / std of x'."""
    B, L = 16, 2048
    conv, bn, a, act = _trained_inputs(gpu, B, L)[layer]
    assert a.shape == (B, 128, L) and conv.out_channels == 1024
    bn = copy.deepcopy(bn).train(mode == "train")
    g = torch.randn(B, 1024, generator=torch.Generator().manual_seed(11)).to(gpu)
    everything = torch.ones(1024, dtype=torch.bool, device=gpu)
    table, truth, _ = _three_way(gpu, monkeypatch, f"a-{layer}", conv, bn, a, g, act, [("all", everything)])
    line = {"case": f"a-{layer}", "mode": mode, "group": "all", "dev": table["all"]}
    steps = LADDER
    if mode == "train":
        ratio = float(truth.ratio().max())
        line["checkpoint_max_ratio"] = ratio
        print(f"a-{layer}: largest per-channel |mean| / std of x' = {ratio:.3f}")
        steps = [s for s in LADDER if s >= ratio]
    _append(line)
    _assert_4x(f"a-{layer} {mode}", "all", table["all"])
    if mode == "train":      # the recorded ratio decides which ladder groups carry the 4x rule: it must cover this run's
        assert steps and _required_step(_recorded()) >= steps[0], (ratio, _required_step(_recorded()))


# ---------------------------------------------------------------------------------------------------------------------
# b. channels whose mean is large against their spread

def _ladder_layer(B, K, C, L, seed):
    """a = relu(randn); W = a random layer plus a rank-one part, conv bias such that |mean_c| / std_c of x' is exactly the
    channel's ladder step (computed in float64 from a's mean vector and covariance; both signs of the offset); the last
    four channels constant (W = 0; biases whose sums are exact in fp32)."""
    gen = torch.Generator().manual_seed(seed)
    a = torch.relu(torch.randn(B, K, L, generator=gen))
    W = (torch.rand(C, K, generator=gen) * 2 - 1) / K ** 0.5
    ncst, nl = 4, len(LADDER)
    per = (C - ncst) // nl
    group = torch.zeros(C, dtype=torch.long)
    for i in range(nl):
        group[i * per:(i + 1) * per] = i
    group[C - ncst:] = nl
    R = torch.tensor(LADDER + (0.0,), dtype=torch.float64)[group]
    sign = torch.where(torch.arange(C) % 2 == 0, 1.0, -1.0).double()
    a64 = a.double()
    abar = a64.mean((0, 2))
    ac = a64 - abar.view(1, K, 1)
    cov = torch.einsum("bkl,bjl->kj", ac, ac) / (B * L)
    std0 = torch.sqrt(torch.einsum("ck,kj,cj->c", W.double(), cov, W.double()))
    t = sign * 0.5 * torch.clamp(R, max=4.0) * std0 / (float(abar.mean()) * K)    # rank-one part: up to two std of offset
    W = (W.double() + t[:, None]).float()
    W[group == nl] = 0.0
    Wd = W.double()
    mean, std = Wd @ abar, torch.sqrt(torch.einsum("ck,kj,cj->c", Wd, cov, Wd))
    pb = (sign * R * std - mean).float()
    pb[group == nl] = torch.tensor([0.5, -2.0, 1.0, -0.25])
    gamma = torch.randn(C, generator=gen)
    beta = torch.randn(C, generator=gen) * 0.3
    g = torch.randn(B, C, generator=gen)
    labels = [str(s) for s in LADDER] + [CONST]
    return a, W, pb, gamma, beta, g, [(labels[i], group == i) for i in range(nl + 1)]


@pytest.mark.parametrize("shape,act", [((16, 128, 1024, 2048), "relu"), ((5, 100, 1000, 300), None),
                                       ((3, 16, 70, 1000), ("leaky", 0.2))])
@pytest.mark.parametrize("mode", ["train", "eval"])
def test_offset_ladder(gpu, monkeypatch, shape, act, mode):
    """Per channel group of |mean| / std: the 4x rule up to the ladder step at or above the checkpoint's largest ratio
    (and for the constant channels' exactly representable values); above it, finite and at most 3x the deviation recorded
    in profiles/r06/maxbwd_deviation.jsonl.  Measured on MI355X (that file): at 16 x 128 -> 1024 x 2048 the algebra's
    d weight deviation is 6e-7 / 5e-7 / 3e-6 / 4e-4 / 4e-2 along the ladder, the dense form's 2e-6 / 1e-6 / 3e-6 / 4e-4 / 4e-2, the
    library chain's 4e-7 / 4e-7 / 1e-5 / 1e-3 / 1e-1; the checkpoint's largest ratio is 4.1, so the 4x rule runs up to 10.
    From 100 on running_var is 2e-5 / 2e-3 off on every path: the fp32 x' and its variance lose the digits, not the algebra."""
    from fpsg_amd import fused_bn
    monkeypatch.setattr(fused_bn, "_MAX_ALGEBRA_MIN_POINTS", 0)
    B, K, C, L = shape
    a, W, pb, gamma, beta, g, groups = _ladder_layer(B, K, C, L, 1)
    assert bool((gamma > 0).any()) and bool((gamma < 0).any())
    conv, bn = _modules(gpu, W, pb, gamma, beta, train=mode == "train")
    case = f"b-{B}x{K}x{C}x{L}"
    groups = [(lb, m.to(gpu)) for lb, m in groups]
    table, truth, _ = _three_way(gpu, monkeypatch, case, conv, bn, a.to(gpu), g.to(gpu), act, groups)
    ratio = truth.ratio()
    for (lb, m), step in zip(groups[:-1], LADDER):
        r = ratio[m.cpu()]
        assert float((r - step).abs().max()) <= 1e-6 * max(step, 1.0), (lb, float(r.min()), float(r.max()))
    for lb, _ in groups:
        _append({"case": case, "mode": mode, "group": lb, "dev": table[lb]})
    lines = _recorded()
    need = _required_step(lines)
    rec = {ln["group"]: ln["dev"] for ln in lines if ln.get("case") == case and ln.get("mode") == mode}
    forward = ("out", "running_mean", "running_var")
    for lb, _ in groups:
        if lb != CONST and float(lb) <= need:
            _assert_4x(f"{case} {mode}", lb, table[lb])
            continue
        # above the step.  A constant channel's ratio is infinite: its forward tensors belong here (the forward's
        # x * scale + (beta - mean * scale) rounds mean * scale = 158 gamma at rstd = 1 / sqrt(eps)), its gradients
        # hold no cancelling sums and keep the 4x rule.
        assert lb in rec, f"{RECORD}: no line for {case} {mode} group {lb}"
        if lb == CONST:
            _assert_4x(f"{case} {mode}", lb, {n: r for n, r in table[lb].items() if n not in forward})
        for n, r in table[lb].items():
            assert np.isfinite(r["algebra"]) and r["algebra"] <= 3.0 * rec[lb][n]["algebra"], (case, mode, lb, n, r, rec[lb][n])


# ---------------------------------------------------------------------------------------------------------------------
# c. concentrated and tied selections

def _dominant(B, K, C, L, points, seed, integer=True):
    """Integer-valued a (0..2) with dominant feature vectors at ``points``: point j carries 50 on the input channels
    k = j (mod J).  Integer W; gamma's sign follows the largest partial row sum, so that nearly every channel of every
    cloud selects one of the dominant points (arg-max where gamma > 0, arg-min where gamma < 0)."""
    gen = torch.Generator().manual_seed(seed)
    J = len(points)
    a = torch.randint(0, 3, (B, K, L), generator=gen).float()
    for j, p in enumerate(points):
        a[:, :, p] = 0.0
        a[:, j::J, p] = 50.0
    W = torch.randint(-3, 4, (C, K), generator=gen).float()
    first = [j for j, p in enumerate(points) if p % 128 == 0]
    if first:       # the first channel of every sorting pass on a tile's first point: the smallest key of that tile
        for c in range(0, C, 1024):
            W[c] = -1.0
            W[c, first[0]::J] = 3.0
    part = torch.stack([W[:, j::J].sum(1) for j in range(J)], 1)           # [C, J]
    big = part.abs().max(1)[0]
    lead = part.gather(1, part.abs().argmax(1, keepdim=True)).squeeze(1)
    gamma = torch.where(lead >= 0, 1.0, -1.0) * torch.randint(1, 3, (C,), generator=gen).float()
    gamma[big == 0] = 1.0
    dz = torch.randint(-4, 5, (B, C), generator=gen).float()
    return a, W, gamma, dz


def _forward_idx(gpu, a, W, gamma):
    """The forward's own idx for x = W a (bias-free, training mode, no activation) through the C ABI; lengths the
    kernels' vector loads do not take (L % 4) go through the library's arg-max / arg-min, as the module does there."""
    from fpsg_amd import _hip
    B, K, L = a.shape
    C = W.shape[0]
    x = torch.bmm(W.unsqueeze(0).expand(B, -1, -1), a).contiguous()
    assert torch.equal(x.double().cpu(), torch.einsum("ck,bkl->bcl", W.double().cpu(), a.double().cpu()))   # integers: exact
    if L % 4:
        return torch.where(gamma >= 0, x.argmax(dim=2), x.argmin(dim=2)).int().contiguous(), x
    lib = _hip.load()
    out = torch.empty(B, C, device=gpu)
    idx = torch.empty(B, C, dtype=torch.int32, device=gpu)
    chan = torch.empty(4, C, device=gpu)
    beta = torch.zeros(C, device=gpu)
    ws = torch.empty(lib.fpsg_bn_max_workspace_floats(B, C, L), device=gpu)
    _hip.check(lib.fpsg_bn_act_max_fwd(_hip.ptr(x), None, _hip.ptr(gamma), _hip.ptr(beta), None, None, -1.0, B, C, L, 1, 1e-5,
                                       0, 0.0, _hip.ptr(out), _hip.ptr(idx), _hip.ptr(chan), None, None, _hip.ptr(ws), None),
               "fpsg_bn_act_max_fwd")
    torch.cuda.synchronize()
    return idx, x


def _canary(gpu, shape, pad=256):
    """A tensor of ``shape`` inside a NaN-filled buffer (pad floats on either side; 16-byte aligned)."""
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * pad,), float("nan"), device=gpu)
    return buf, buf[pad:pad + n].view(shape)


def _canary_intact(buf, shape, pad=256):
    n = int(np.prod(shape))
    return bool(torch.isnan(buf[:pad]).all()) and bool(torch.isnan(buf[pad + n:]).all())


def _scatter(gpu, da, W, k1, dz, idx, v):
    from fpsg_amd import _hip
    lib = _hip.load()
    B, K, L = da.shape
    C = W.shape[0]
    n = lib.fpsg_max_bwd_scatter_workspace_floats(B, C, L)
    wbuf, ws = _canary(gpu, (n,))
    rc = lib.fpsg_max_bwd_scatter(_hip.ptr(da), _hip.ptr(W), _hip.ptr(k1), _hip.ptr(dz), _hip.ptr(idx), _hip.ptr(v), B, K, C, L,
                                  _hip.ptr(ws), None)
    torch.cuda.synchronize()
    assert _canary_intact(wbuf, (n,)), "the scatter wrote outside its workspace"
    return rc


DOMINANT = [  # B, K, C, L, dominant points
    (1, 128, 1024, 2048, [777]),                      # ~1000 pairs on one point: 125 eight-pair rounds in one wave
    (2, 64, 1000, 512, [3, 64, 127]),                 # three points of one tile, two of them in the same wave (l % 4)
    (3, 65, 1000, 300, [127, 128, 256, 299]),         # a tile's last and first points, the last point, L % 128 != 0
    (5, 63, 2500, 1000, [0, 999]),                    # three sorting passes, the last one ragged (452 keys)
    (7, 1, 70, 260, [259]),
    (5, 128, 2500, 2048, [128, 1920, 2047]),
    (3, 65, 1000, 301, [127, 128, 256, 300]),         # odd L: the scatter's scalar rows (pair_ok == false); no gather
    (2, 16, 70, 2051, [2050, 2048]),                  # odd and beyond the gather's 2048
]


@pytest.mark.parametrize("B,K,C,L,points", DOMINANT)
def test_concentrated_selections_exact(gpu, B, K, C, L, points):
    """fpsg_max_bwd_gather / fpsg_max_bwd_scatter called directly on the forward's own idx for inputs whose dominant
    points draw nearly all channels: integer-valued a, W, dz, k1, v, da, so every sum is exact in fp32 whatever its
    order and S, the row sums of a and da are compared bit for bit with a float64 evaluation.  The results sit inside
    NaN-filled buffers: nothing outside them is written (da is read-modify-write: the tile past L included)."""
    from fpsg_amd import _hip
    lib = _hip.load()
    a, W, gamma, dz = [t.to(gpu) for t in _dominant(B, K, C, L, points, seed=B + K + C + L)]
    idx, x = _forward_idx(gpu, a, W, gamma)
    # the selections are what the construction says: first arg-max / arg-min of the exact x, mostly on the dominant points
    xc, ic = x.double().cpu(), idx.cpu().long()
    ext = torch.where(gamma.cpu() >= 0, xc.max(dim=2)[0], xc.min(dim=2)[0])
    first = (xc == ext.unsqueeze(2)).double().argmax(dim=2)
    assert torch.equal(ic, first)
    on = torch.zeros(B, C, dtype=torch.bool)
    for p in points:
        on |= ic == p
    assert float(on.double().mean()) >= 0.8, float(on.double().mean())
    for p in points:
        assert int((ic == p).sum()) >= B * C // (2 * len(points) + 2), (p, int((ic == p).sum()))
    tile_first = [p for p in points if p % 128 == 0]
    if tile_first:
        assert bool((ic[:, ::1024] == tile_first[0]).all())
    gen = torch.Generator().manual_seed(3)
    k1 = gamma.clone()
    v = torch.randint(-5, 6, (K,), generator=gen).float().to(gpu)
    da0 = torch.randint(-9, 10, (B, K, L), generator=gen).float()
    # ---- scatter
    dbuf, da = _canary(gpu, (B, K, L))
    da.copy_(da0)
    assert _scatter(gpu, da, W, k1, dz, idx, v) == 0, lib.fpsg_last_error()
    want = da0.double() + v.double().cpu().view(1, K, 1)
    contrib = (k1 * dz).double().cpu().unsqueeze(1) * W.double().cpu().t().unsqueeze(0)            # [B, K, C]
    want.scatter_add_(2, ic.unsqueeze(1).expand(B, K, C), contrib)
    assert float(want.abs().max()) < 2 ** 24
    assert _canary_intact(dbuf, (B, K, L)), "the scatter wrote outside da"
    assert torch.equal(da.double().cpu(), want)
    # ---- gather
    sbuf, S = _canary(gpu, (C, K))
    pbuf, spart = _canary(gpu, (B, K))
    abuf, al = _canary(gpu, (B, K, L))
    al.copy_(a)
    rc = lib.fpsg_max_bwd_gather(_hip.ptr(al), _hip.ptr(dz), _hip.ptr(idx), B, K, C, L, _hip.ptr(S), _hip.ptr(spart), None)
    torch.cuda.synchronize()
    if L % 4 or L > 2048:
        assert rc != 0 and b"multiple of 4" in lib.fpsg_last_error()
        assert bool(torch.isnan(sbuf).all()) and bool(torch.isnan(pbuf).all())
        return
    assert rc == 0, lib.fpsg_last_error()
    asel = torch.gather(a.double().cpu(), 2, ic.unsqueeze(1).expand(B, K, C))                       # a[b, :, sel(b, c)]
    assert _canary_intact(sbuf, (C, K)) and _canary_intact(pbuf, (B, K)), "the gather wrote outside S / the row sums"
    assert torch.equal(S.double().cpu(), torch.einsum("bc,bkc->ck", dz.double().cpu(), asel))
    assert torch.equal(spart.double().cpu(), a.double().cpu().sum(2))


def test_scatter_sums_a_point_in_ascending_channel_order(gpu):
    """Non-integer coefficients on one dominant point per cloud: the run of ~1000 pairs must be summed as the header
    says, D = fma(k1[c] dz[b,c], W[c,k], D) over ascending c, then da + (v + D) -- bit for bit against that recurrence
    evaluated in float64 and rounded to fp32 after every step (a product of two fp32 numbers is exact in float64)."""
    from fpsg_amd import _hip
    lib = _hip.load()
    B, K, C, L, p = 2, 65, 1000, 512, 200
    a, W, gamma, _ = [t.to(gpu) for t in _dominant(B, K, C, L, [p], seed=9)]
    idx, _ = _forward_idx(gpu, a, W, gamma)
    gen = torch.Generator().manual_seed(4)
    Wf = torch.randn(C, K, generator=gen).to(gpu)
    k1 = (torch.randn(C, generator=gen) * 3).to(gpu)
    dz = torch.randn(B, C, generator=gen).to(gpu)
    v = torch.randn(K, generator=gen).to(gpu)
    da0 = torch.randn(B, K, L, generator=gen)
    da = da0.clone().to(gpu)
    assert _scatter(gpu, da, Wf, k1, dz, idx, v) == 0, lib.fpsg_last_error()
    cf = (k1.unsqueeze(0) * dz).cpu()                                   # fp32 product, as the sort kernel forms it
    ic, Wc = idx.cpu(), Wf.cpu().numpy().astype(np.float64)
    for b in range(B):
        chans = (ic[b] == p).nonzero().flatten().tolist()               # ascending
        assert len(chans) >= 800
        D = np.zeros(K, dtype=np.float32)
        for c in chans:
            D = (float(cf[b, c]) * Wc[c] + D.astype(np.float64)).astype(np.float32)
        want = da0[b, :, p].numpy() + (v.cpu().numpy() + D)
        assert np.array_equal(da[b, :, p].cpu().numpy(), want.astype(np.float32)), b


@pytest.mark.parametrize("L,expect", [(2048, "algebra"), (2052, "dense"), (302, "library")])
def test_last_point_dominant_through_the_module(gpu, monkeypatch, L, expect):
    """The last point L - 1 dominant, L not a multiple of 128.  Through the module L > 2048 takes the dense project form
    and L % 4 != 0 the library chain: asserted, and all of them under the 4x rule against the forced float64 truth."""
    from fpsg_amd import fused_bn
    monkeypatch.setattr(fused_bn, "_MAX_ALGEBRA_MIN_POINTS", 0)
    B, K, C = 3, 16, 70
    if L == 2048:
        L = 2048 - 128 + 4                   # 1924: a multiple of 4, not of 128
    gen = torch.Generator().manual_seed(L)
    a = torch.relu(torch.randn(B, K, L, generator=gen))
    a[:, :, L - 1] = 15.0 + torch.rand(B, K, generator=gen)
    W = torch.randn(C, K, generator=gen) / K ** 0.5
    gamma = torch.where(W.sum(1) >= 0, 1.0, -1.0) * (0.5 + torch.rand(C, generator=gen))
    conv, bn = _modules(gpu, W, torch.randn(C, generator=gen) * 0.3, gamma, torch.randn(C, generator=gen) * 0.3)
    g = torch.randn(B, C, generator=gen).to(gpu)
    everything = torch.ones(C, dtype=torch.bool, device=gpu)
    seen_before = _count_forms(monkeypatch)
    table, _, idx = _three_way(gpu, monkeypatch, f"c-last-{L}", conv, bn, a.to(gpu), g, "relu", [("all", everything)],
                               expect="algebra" if expect == "algebra" else "other")
    if expect == "library":
        assert seen_before["algebra"] == 0 and seen_before["dense"] == 0, seen_before
    if expect == "dense":
        assert seen_before["dense"] >= 1 and seen_before["algebra"] == 0, seen_before
    assert float((idx.cpu() == L - 1).double().mean()) >= 0.8
    _assert_4x(f"c-last-{L}", "all", table["all"])


@pytest.mark.parametrize("mode", ["train", "eval"])
def test_duplicated_columns_tie_on_the_first(gpu, monkeypatch, mode):
    """Padded clouds repeat points: a[:, :, L/2:] = a[:, :, :L/2] makes every maximum an exact tie.  idx is the first
    occurrence, all of dz lands there (d input at the duplicate holds the dense part only): the forced float64 truth.
    The library may give the tie to either column, so its own d input is compared after adding the two halves."""
    from fpsg_amd import fused_bn
    monkeypatch.setattr(fused_bn, "_MAX_ALGEBRA_MIN_POINTS", 0)
    B, K, C, L = 7, 64, 1000, 1024
    gen = torch.Generator().manual_seed(21)
    a = torch.relu(torch.randn(B, K, L, generator=gen))
    a[:, :, L // 2:] = a[:, :, :L // 2]
    W = (torch.rand(C, K, generator=gen) * 2 - 1) / K ** 0.5
    conv, bn = _modules(gpu, W, torch.randn(C, generator=gen) * 0.3, torch.randn(C, generator=gen),
                        torch.randn(C, generator=gen) * 0.3, train=mode == "train")
    g = torch.randn(B, C, generator=gen).to(gpu)
    everything = torch.ones(C, dtype=torch.bool, device=gpu)
    fold = lambda t: t[..., :L // 2] + t[..., L // 2:]
    table, truth, idx = _three_way(gpu, monkeypatch, "c-duplicates", conv, bn, a.to(gpu), g, None, [("all", everything)],
                                   fold=fold)
    assert int(idx.max()) < L // 2 and int(idx.min()) >= 0
    _assert_4x(f"c-duplicates {mode}", "all", table["all"])


# ---------------------------------------------------------------------------------------------------------------------
# d. the small kernels through the C ABI, and the limits

@pytest.mark.parametrize("B,K,C,L", [(16, 128, 1024, 2048), (5, 100, 1000, 300), (11, 1, 7, 64), (8, 65, 33, 128)])
@pytest.mark.parametrize("with_bias", [True, False])
@pytest.mark.parametrize("training", [True, False])
def test_prep_and_dw_formulas(gpu, B, K, C, L, with_bias, training):
    """fpsg_max_bwd_prep / fpsg_max_bwd_dw against the header's formulas in float64: Wk = k2 W (one rounding: bit for
    bit), u, dpre_bias, s, dw within the round-off of their few fp32 operations (2^-23 per operation on the sum of the
    terms' magnitudes).  pre_bias = NULL, WG = NULL / no row sums (eval mode), B not a multiple of 8."""
    from fpsg_amd import _hip
    lib = _hip.load()
    gen = torch.Generator().manual_seed(B * K + C)
    r = lambda *s: torch.randn(*s, generator=gen).to(gpu)
    W, coef, pb, mean, dz, spart_in = r(C, K), r(3, C), r(C), r(C) * 3, r(B, C), r(B, K) * 50
    Sm, WG = r(C, K), r(C, K) * 100
    opt = lambda t: _hip.ptr(t) if t is not None else None
    pbo = pb if with_bias else None
    bufs = {n: _canary(gpu, s) for n, s in (("Wk", (C, K)), ("u", (C,)), ("dpb", (C,)), ("s", (K,)), ("dw", (C, K)))}
    Wk, u, dpb, s, dw = (bufs[n][1] for n in ("Wk", "u", "dpb", "s", "dw"))
    rc = lib.fpsg_max_bwd_prep(_hip.ptr(W), _hip.ptr(coef), opt(pbo), _hip.ptr(mean), _hip.ptr(dz),
                               opt(spart_in if training else None), B, K, C, L, _hip.ptr(Wk), _hip.ptr(u), _hip.ptr(dpb),
                               opt(s if training else None), None)
    assert rc == 0, lib.fpsg_last_error()
    rc = lib.fpsg_max_bwd_dw(_hip.ptr(Sm), opt(WG if training else None), _hip.ptr(coef), opt(pbo), opt(s if training else None),
                             B, K, C, _hip.ptr(dw), None)
    assert rc == 0, lib.fpsg_last_error()
    torch.cuda.synchronize()
    shapes = {"Wk": (C, K), "u": (C,), "dpb": (C,), "s": (K,), "dw": (C, K)}
    for n, (buf, _) in bufs.items():
        if n == "s" and not training:
            assert bool(torch.isnan(buf).all())
            continue
        assert _canary_intact(buf, shapes[n]), n
    d = lambda t: t.double().cpu()
    k1, k2, k3 = d(coef[0]), d(coef[1]), d(coef[2])
    b64 = d(pb) if with_bias else torch.zeros(C, dtype=torch.float64)
    count = float(B * L)
    assert torch.equal(Wk.cpu(), (k2[:, None] * d(W)).float())

    def close(got, want, mag, ops, name):
        err = (d(got) - want).abs()
        assert bool((err <= ops * EPS32 * mag).all()), (name, float((err / mag).max()))

    close(u, k2 * b64 + k3, (k2 * b64).abs() + k3.abs(), 2, "u")
    sdz = d(dz).sum(0)
    close(dpb, k1 * sdz + (k2 * d(mean) + k3) * count,
          k1.abs() * d(dz).abs().sum(0) + ((k2 * d(mean)).abs() + k3.abs()) * count, B + 4, "dpre_bias")
    if training:
        s64 = d(spart_in).sum(0)
        close(s, s64, d(spart_in).abs().sum(0), B, "s")
        sk = d(s)                                     # dw is defined on the s that prep left
        want = k1[:, None] * d(Sm) + k2[:, None] * (d(WG) + b64[:, None] * sk[None]) + k3[:, None] * sk[None]
        mag = (k1[:, None] * d(Sm)).abs() + k2.abs()[:, None] * (d(WG).abs() + (b64[:, None] * sk[None]).abs()) + (k3[:, None] * sk[None]).abs()
        close(dw, want, mag, 5, "dw")
    else:
        assert torch.equal(dw.cpu(), (k1[:, None] * d(Sm)).float())


def test_limits_refuse_loudly(gpu):
    """K > 128 in the scatter; L > 2048, L % 4 != 0 and a misaligned a in the gather: a non-zero code, a message, and
    nothing written."""
    from fpsg_amd import _hip
    lib = _hip.load()
    B, C = 2, 8

    def gather(K, L, shift=0):
        store = torch.zeros(B * K * L + 4, device=gpu)
        a = store[shift:shift + B * K * L].view(B, K, L)
        dz = torch.ones(B, C, device=gpu)
        idx = torch.zeros(B, C, dtype=torch.int32, device=gpu)
        sbuf, S = _canary(gpu, (C, K))
        rc = lib.fpsg_max_bwd_gather(_hip.ptr(a), _hip.ptr(dz), _hip.ptr(idx), B, K, C, L, _hip.ptr(S), None, None)
        torch.cuda.synchronize()
        return rc, lib.fpsg_last_error(), bool(torch.isnan(sbuf).all())

    rc, msg, clean = gather(4, 2052)
    assert rc != 0 and b"at most 2048" in msg and clean
    rc, msg, clean = gather(4, 302)
    assert rc != 0 and b"multiple of 4" in msg and clean
    rc, msg, clean = gather(4, 64, shift=1)
    assert rc != 0 and b"16-byte aligned" in msg and clean
    rc, msg, clean = gather(4, 64)
    assert rc == 0 and not clean
    K, L = 129, 64
    dbuf, da = _canary(gpu, (B, K, L))
    W, k1, v = torch.ones(C, K, device=gpu), torch.ones(C, device=gpu), torch.ones(K, device=gpu)
    dz, idx = torch.ones(B, C, device=gpu), torch.zeros(B, C, dtype=torch.int32, device=gpu)
    rc = _scatter(gpu, da, W, k1, dz, idx, v)
    assert rc != 0 and b"beyond 128 input channels" in lib.fpsg_last_error()
    assert bool(torch.isnan(dbuf).all())
