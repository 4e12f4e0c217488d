"""K24 on the GPU: the trees are the float64 Prim's bit for bit where every distance is exact in fp32;
on unit-ball, tanh and sheet clouds the kernel's own trees are valid minimum spanning trees, its penalised sets are the
float64 ones exactly and the value and the gradient agree with float64 to the project's 1e-4; the corners are exact;
nothing depends on the run, the batch, the patch's place or a graph replay; and the term reaches ``model.loss`` and
``trainNetwork.py``.

The checker is ``tests/_expansion_ref.py`` (float64 torch, on the CPU)."""
import math
import os
import re
import subprocess
import sys

import pytest
import torch

from conftest import ROOT

import _expansion_ref as ref

pytestmark = pytest.mark.gpu

BOUND = 1e-4                                                         # the project's parity bar


def _grid_clouds(N, seed):
    """Three clouds with coordinates integer / 64 in [-1, 1] (every d2 an integer multiple of 2^-12 below 2^4: exact in
    fp32 whatever the fma order): random on the full grid (distance ties); random on 9 levels per axis (ties and
    repeated points); distinct points whose second half repeats the first."""
    g = torch.Generator().manual_seed(seed)
    fine = torch.randint(-64, 65, (N, 3), generator=g)
    coarse = torch.randint(-4, 5, (N, 3), generator=g) * 16
    half = N // 2
    cells = torch.randperm(129 ** 3, generator=g)[:N - half]
    uniq = torch.stack([cells % 129, (cells // 129) % 129, cells // (129 * 129)], dim=1) - 64
    dup = torch.cat([uniq, uniq[:half]])
    return (torch.stack([fine, coarse, dup]).float() / 64.0).contiguous()


def _run(p, P, lam=1.5, up=None):
    """``(value, parent, d2, order, mean_len, grad)`` of ``metrics.expansion_penalty``; ``up [B]`` is the upstream
    gradient (default: ones)."""
    from fpsg_amd.metrics import expansion_penalty
    x = p.clone().requires_grad_()
    B, N, _ = p.shape
    out, info = expansion_penalty(x, P, lam, return_info=True)
    assert out.dtype == torch.float32 and tuple(out.shape) == (B,) and set(info) == {"parent", "d2", "order", "mean_len"}
    assert info["parent"].dtype == torch.int32 and tuple(info["parent"].shape) == (B, N)
    assert info["order"].dtype == torch.int32 and tuple(info["order"].shape) == (B, N)
    assert info["d2"].dtype == torch.float32 and tuple(info["d2"].shape) == (B, N)
    assert info["mean_len"].dtype == torch.float32 and tuple(info["mean_len"].shape) == (B, N // P)
    (g,) = torch.autograd.grad((out * (torch.ones_like(out) if up is None else up)).sum(), [x])
    return out.detach(), info["parent"], info["d2"], info["order"], info["mean_len"], g


def _in_range(parent, P):
    par = parent.reshape(-1, P)
    assert bool((par[:, 0] == -1).all())
    assert bool(((par[:, 1:] >= 0) & (par[:, 1:] < P)).all()), "no index outside [0, P) except the root's -1"


# ---- 1. the trees, bit for bit -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("P,K", [(P, K) for P in (2, 3, 63, 64, 65, 128, 129) for K in (1, 3)] + [(1024, 2)]
                         + [(P, 3) for P in (256, 257, 512, 513)])
def test_trees_equal_the_float64_prim_on_exact_distances(gpu, P, K):
    """63 / 64 / 65, 128 / 129, 256 / 257 and 512 / 513 cross the vertices-per-lane steps; at 1024 the three clouds run one
    at a time (B = 1)."""
    N = K * P
    p = _grid_clouds(N, 100 * P + K)
    batches = [p] if P < 1024 else [p[i:i + 1] for i in range(3)]
    for x in batches:
        _, parent, d2, order, _, _ = _run(x.to(gpu), P)
        want_par, want_d2, want_order = ref.prim(x, P)
        _in_range(parent, P)
        assert torch.equal(parent.cpu().long(), want_par), "every vertex of every patch"
        assert torch.equal(d2.cpu().double(), want_d2)
        assert torch.equal(order.cpu().long(), want_order)
        assert bool((d2.reshape(-1, P)[:, 0] == 0).all()) and bool((order.reshape(-1, P)[:, 0] == 0).all())


# ---- 2. values and gradients against float64 on the kernel's own trees ---------------------------------------------------

_CLOUDS = {}


def _value_clouds(P):
    if P not in _CLOUDS:
        _CLOUDS[P] = ref.value_clouds(P)
    return _CLOUDS[P]


@pytest.mark.parametrize("lam", ref.VALUE_LAMBDAS)
@pytest.mark.parametrize("P", ref.VALUE_P)
def test_value_and_gradient_against_float64(gpu, P, lam):
    """Two unit-ball clouds, one tanh(randn) cloud and the sheet cloud (``_expansion_ref.value_clouds``;
    ``test_expansion_cpu.py`` holds the condition that makes the exact mask a fair demand).  The reference gets the KERNEL's
    tree, after that tree has passed the validity and minimality checks.  Prints the measured deviations (DESIGN.md K24,
    *Measured*)."""
    x = _value_clouds(P)
    B, N, _ = x.shape
    K = N // P
    up = torch.tensor([1.0, 0.5, 2.0, 1.5], device=gpu)              # the upstream gradient, not all ones
    R, parent, d2, order, mlen, grad = _run(x.to(gpu), P, lam, up)
    parent, d2, order, mlen, R, grad = (t.cpu() for t in (parent, d2, order, mlen, R, grad))
    ref.check_tree(parent, order, P)
    worst_mst = ref.check_minimal(x, P, parent)
    # the stored d2 is the edge's
    r64 = ref.edge_lengths(x, P, parent).reshape(B, N)
    assert float(((d2.double().sqrt() - r64).abs() / r64.clamp_min(1e-30)).max()) <= 1e-5
    # the mask, exactly: the fp32 test on the kernel's outputs is the float64 one
    mask64 = ref.penalised(x, P, parent, lam)
    mask32 = d2.sqrt() > torch.tensor(lam, dtype=torch.float32) * mlen.repeat_interleave(P, dim=1)
    assert torch.equal(mask32, mask64)
    assert bool(mask64[3].reshape(K, P).any(1).all()), "every patch of the sheet cloud has a penalised edge"
    l64 = ref.mean_len(x, P, parent)
    R64, g64 = ref.value_and_grad(x, P, parent, mask64, up.cpu())
    assert bool(torch.isfinite(R).all()) and bool(torch.isfinite(grad).all()) and bool((R >= 0).all())
    # ... and the kernel's own: its gradient is non-zero on exactly the rows the float64 gradient is
    assert torch.equal((grad != 0).any(-1), (g64 != 0).any(-1))
    dev_l = float(((mlen.double() - l64).abs() / l64).max())
    # a cloud without a penalised edge (a unit-ball cloud at lambda = 2 may be one) has value +0 and gradient 0, exactly
    none = R64 == 0
    assert float(R64[3]) > 0 and torch.equal(none, g64.abs().amax((1, 2)) == 0)
    assert bool((R[none] == 0).all()) and bool((grad[none] == 0).all())
    one = torch.ones_like(R64)
    dev_R = ((R.double() - R64).abs() / torch.where(none, one, R64)).tolist()
    dev_g = ((grad.double() - g64).abs().amax((1, 2)) / torch.where(none, one, g64.abs().amax((1, 2)))).tolist()
    print(f"expansion vs float64 P={P} lambda={lam}: sorted edges vs scipy {worst_mst:.3e}; mean_len {dev_l:.3e}; "
          f"|E - E64| / E64 per cloud {dev_R}; max|g - g64| / max|g64| per cloud {dev_g}; E64 {R64.tolist()}")
    assert dev_l <= BOUND and max(dev_R) <= BOUND and max(dev_g) <= BOUND, (dev_l, dev_R, dev_g)


# ---- 3. corners, exact ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("P", [2, 64, 100, 128, 512, 1024])
def test_every_point_identical(gpu, P):
    K = 2
    p = torch.tensor([0.3, -0.2, 0.7], device=gpu).expand(2, K * P, 3).contiguous()
    for lam in (1.0, 1.5):
        R, parent, d2, order, mlen, grad = _run(p, P, lam)
        assert bool((R == 0).all()) and not bool(torch.signbit(R).any()), "+0"
        assert bool((d2 == 0).all()) and bool((mlen == 0).all())
        want = torch.zeros(P, dtype=torch.int32, device=gpu)
        want[0] = -1
        assert torch.equal(parent.reshape(-1, P), want.expand(2 * K, P)), "nobody ever improves on vertex 0"
        assert torch.equal(order.reshape(-1, P), torch.arange(P, dtype=torch.int32, device=gpu).expand(2 * K, P))
        assert bool(torch.isfinite(grad).all()) and bool((grad == 0).all())


def test_two_points_per_patch_are_never_penalised(gpu):
    g = torch.Generator().manual_seed(4)
    p = torch.rand((3, 16, 3), generator=g).to(gpu)
    for lam in (1.0, 1.5):
        R, parent, d2, order, mlen, grad = _run(p, 2, lam)
        assert bool((R == 0).all()) and bool((grad == 0).all())
        assert parent.reshape(-1, 2).tolist() == [[-1, 0]] * 24 and order.reshape(-1, 2).tolist() == [[0, 1]] * 24
        assert bool((mlen > 0).all())


@pytest.mark.parametrize("P", [65, 128])
def test_equispaced_collinear_points_are_never_penalised(gpu, P):
    """All edges are 1/64 exactly, their sum and its division by P - 1 are exact: r == l, and the comparison is strict --
    at lambda = 1 too.  In natural order and shuffled."""
    g = torch.Generator().manual_seed(P)
    line = torch.zeros((P, 3))
    line[:, 0] = torch.arange(P) / 64.0 - 1.0
    p = torch.stack([torch.cat([line, line[torch.randperm(P, generator=g)]]),
                     torch.cat([line[torch.randperm(P, generator=g)], line.flip(0)])]).to(gpu).contiguous()
    for lam in (1.0, 1.5):
        R, parent, d2, order, mlen, grad = _run(p, P, lam)
        assert bool((d2.reshape(-1, P)[:, 1:] == 1.0 / 4096).all()) and bool((mlen == 1.0 / 64).all())
        assert bool((R == 0).all()) and bool((grad == 0).all())


def test_one_outlier_is_one_penalised_edge(gpu):
    """K = 4 patches of 63 collinear grid points plus, in patch 2 only, one point 1.25 away from the line (a 3-4-5
    offset: exact).  Elsewhere the 64th point continues the line."""
    P, K = 64, 4
    line = torch.zeros((P, 3))
    line[:, 0] = torch.arange(P) / 64.0 - 0.5
    cloud = line.repeat(K, 1).reshape(K, P, 3).clone()
    at, foot = 40, 41                                                # the outlier sits over the line's point `foot`
    cloud[2, at] = cloud[2, foot] + torch.tensor([0.0, 0.75, 1.0])
    p = cloud.reshape(1, K * P, 3).to(gpu).contiguous()
    R, parent, d2, order, mlen, grad = _run(p, P, 1.5)
    _in_range(parent, P)
    o, f = 2 * P + at, 2 * P + foot
    assert int(parent[0, o]) == foot and float(d2[0, o]) == 1.5625 and int(order[0, o]) == P - 1
    r = 1.25
    want = r / ((P - 1) * K)
    assert abs(float(R[0]) - want) <= want * 2.0 ** -23, "to 1 ulp of the square root"
    moved = (grad[0] != 0).any(-1).nonzero().flatten().tolist()
    assert moved == [o, f], "non-zero at the two endpoints only"
    assert torch.equal(grad[0, o], -grad[0, f]), "equal and opposite"
    unit = torch.tensor([0.0, 0.6, 0.8], dtype=torch.float64)
    got = grad[0, o].double().cpu()
    assert float((got / got.norm() - unit).abs().max()) <= 1e-6, "along the unit edge vector"
    assert abs(float(got.norm()) - 1.0 / ((P - 1) * K)) <= 1e-6 / ((P - 1) * K)


# ---- 4. independence and invariance, bit for bit ---------------------------------------------------------------------------

def _sheet_patch(P, seed):
    g = torch.Generator().manual_seed(seed)
    uv = torch.rand((P, 2), generator=g) * 0.2
    s = torch.stack([uv[:, 0], uv[:, 1], 0.05 * torch.sin(15 * uv[:, 0])], dim=1)
    s[P // 3] += torch.tensor([0.3, -0.4, 0.5])
    return s


def test_bits_do_not_depend_on_the_run_or_the_batch(gpu):
    P = 128
    p = ref.value_clouds(P).to(gpu)
    p = torch.cat([p, p[:1]]).contiguous()
    up = torch.tensor([1.5, 1.0, 0.5, 2.0, 1.5], device=gpu)
    a = _run(p, P, 1.5, up)
    b = _run(p, P, 1.5, up)
    assert all(torch.equal(s, t) for s, t in zip(a, b))
    one = _run(p[:1].contiguous(), P, 1.5, up[:1])
    for pos in (0, 4):
        assert all(torch.equal(s, t[pos:pos + 1]) for s, t in zip(one, a)), pos
    assert float(a[5].abs().max()) > 0 and float(a[0].min()) > 0


def test_bits_do_not_depend_on_the_patch_position(gpu):
    """The same 128 points as patch 0 of one cloud and patch 5 of another, the other patches a single repeated point
    (E_q = +0, so the cloud's value is the special patch's E_q / K in both): the same tree, E_q and gradient rows."""
    P, K = 128, 6
    special = _sheet_patch(P, 8)
    rest = torch.tensor([0.25, 0.5, -0.125]).expand(P, 3)
    a = torch.cat([special] + [rest] * (K - 1))
    b = torch.cat([rest] * (K - 1) + [special])
    p = torch.stack([a, b]).to(gpu).contiguous()
    R, parent, d2, order, mlen, grad = _run(p, P, 1.5)
    assert float(R[0]) > 0 and torch.equal(R[0], R[1])
    assert torch.equal(mlen[0, 0], mlen[1, K - 1])
    for t in (parent, d2, order, grad):
        assert torch.equal(t[0, :P], t[1, (K - 1) * P:]), "the special patch"
    assert float(grad[0, :P].abs().max()) > 0 and bool((grad[0, P:] == 0).all()) and bool((grad[1, :(K - 1) * P] == 0).all())


def test_a_patch_does_not_see_the_other_patches(gpu):
    P, K = 128, 4
    p = torch.cat([_sheet_patch(P, 20 + q) for q in range(K)]).reshape(1, K * P, 3).to(gpu).contiguous()
    other = p.clone()
    other[0, 2 * P:3 * P] = _sheet_patch(P, 99).to(gpu) * 2.0
    a = _run(p, P, 1.5)
    b = _run(other, P, 1.5)
    keep = torch.cat([torch.arange(0, 2 * P), torch.arange(3 * P, 4 * P)]).to(gpu)
    for s, t in zip(a[1:4] + a[5:], b[1:4] + b[5:]):                 # parent, d2, order, grad
        assert torch.equal(s[0, keep], t[0, keep])
        assert not torch.equal(s[0, 2 * P:3 * P], t[0, 2 * P:3 * P])
    assert torch.equal(a[4][0, [0, 1, 3]], b[4][0, [0, 1, 3]]) and not torch.equal(a[0], b[0])


def test_bits_survive_a_graph_capture_and_two_replays(gpu):
    from fpsg_amd.metrics import expansion_penalty
    P = 128
    p = ref.value_clouds(P).to(gpu)
    other = p.flip(0).contiguous()
    up = torch.tensor([1.0, 0.5, 2.0, 1.5], device=gpu)
    eager = _run(p, P, 1.5, up)
    x = p.clone().requires_grad_()

    def once():
        out, inf = expansion_penalty(x, P, 1.5, return_info=True)
        (g,) = torch.autograd.grad((out * up).sum(), [x])
        return out.detach(), inf["parent"], inf["d2"], inf["order"], inf["mean_len"], g

    once()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        got = once()
    for _ in range(2):
        with torch.no_grad():
            x.copy_(other)                                           # other clouds in between
        graph.replay()
        torch.cuda.synchronize()
        assert not torch.equal(got[0], eager[0])
        with torch.no_grad():
            x.copy_(p)
        graph.replay()
        torch.cuda.synchronize()
        assert all(torch.equal(s, t) for s, t in zip(got, eager))


# ---- 5. the model ----------------------------------------------------------------------------------------------------------

def _episode_model(gpu, pc_dist, **kw):
    from fpsg_amd.engine import build_model, default_options
    torch.manual_seed(5)
    return build_model(default_options(device="cuda", pc_dist=pc_dist, intra_recon=True, n_shot=2, n_query=1,
                                       **kw)).to(gpu).train()


class _Recorder:
    """A ``metrics.set_launch_probe`` probe that only notes the kinds it brackets."""

    def __init__(self):
        self.kinds = []

    def __call__(self, kind, B, N, M):
        self.kinds.append(kind)
        return self

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        return False


@pytest.mark.parametrize("rep_w", [0.0, 0.25])
@pytest.mark.parametrize("pc_dist", ["cd", "dcd"])
def test_model_loss_adds_one_call_over_the_decoded_clouds(gpu, monkeypatch, pc_dist, rep_w):
    """``cd`` takes the fused K1l path (which returns early without the term), ``dcd`` the batched one; alone and beside
    the repulsion term, each with its own key and its own single call."""
    from fpsg_amd import few_shot, metrics
    from fpsg_amd.episodes import synthetic_episode
    S, Q, W = 2, 1, 0.5
    model = _episode_model(gpu, pc_dist, expansion_weight=W, expansion_lambda=1.25, repulsion_weight=rep_w,
                           query_factor=1.0, support_factor=0.75)
    assert model.expansion_weight == W and model.expansion_patch == 128
    calls, rep_calls = [], []
    inner, inner_rep = metrics.expansion_penalty, metrics.repulsion_loss

    def spy(p, *args, **kwargs):
        calls.append((p.detach().clone(), args, kwargs))
        return inner(p, *args, **kwargs)

    def spy_rep(p, *args, **kwargs):
        rep_calls.append(p.detach().clone())
        return inner_rep(p, *args, **kwargs)

    monkeypatch.setattr(few_shot, "expansion_penalty", spy)
    monkeypatch.setattr(few_shot, "repulsion_loss", spy_rep)
    ep = synthetic_episode(S, Q, n_pts=2048, img_size=96, seed=50, device=gpu)
    rec = _Recorder()
    metrics.set_launch_probe(rec)
    try:
        torch.manual_seed(11)                                        # the decoder's random grid
        out = model.loss(ep)
        keys = {"ttl_loss", "recon_loss", "query_rec_loss", "support_rec_loss", "expansion_loss"}
        assert set(out) == (keys | {"repulsion_loss"} if rep_w else keys)
        assert len(calls) == 1, "ONE expansion_penalty call over the Q + S decoded clouds"
        assert len(rep_calls) == (1 if rep_w else 0)
        clouds, args, kwargs = calls[0]
        assert tuple(clouds.shape) == (Q + S, 2048, 3) and (args + tuple(kwargs.values())) == (128, 1.25)
        if rep_w:
            assert torch.equal(rep_calls[0], clouds), "the same tensor K21 gets"
        each = torch.cat([inner(clouds[i:i + 1].contiguous(), 128, 1.25) for i in range(Q + S)]).double()
        assert bool((each >= 0).all()) and float(each.sum()) > 0
        total = float(each.sum())
        assert abs(float(out["expansion_loss"].detach()) - total) <= 1e-6 * abs(total)
        want = float(out["recon_loss"].detach().double().sum()) + W * (1.0 * float(each[:Q].sum()) + 0.75 * float(each[Q:].sum()))
        if rep_w:
            rep = inner_rep(clouds, 4, 0.03).double()
            assert abs(float(out["repulsion_loss"].detach()) - float(rep.sum())) <= 1e-6 * abs(float(rep.sum()))
            want += rep_w * (1.0 * float(rep[:Q].sum()) + 0.75 * float(rep[Q:].sum()))
        assert abs(float(out["ttl_loss"].detach().double().sum()) - want) <= 1e-6 * abs(want)
        recon = 1.0 * float(out["query_rec_loss"].detach().sum()) + 0.75 * float(out["support_rec_loss"].detach().sum())
        assert abs(float(out["recon_loss"].detach().sum()) - recon) <= 1e-6 * abs(recon)
        assert rec.kinds.count("expansion_fwd") == 1 + Q + S        # the model's one launch pair, and this test's own calls
        out["ttl_loss"].sum().backward()
        assert rec.kinds.count("expansion_bwd") == 1
    finally:
        metrics.set_launch_probe(None)
    nonzero = 0
    for part in (model.pc_decoder, model.img_encoder):
        params = [(n, q) for n, q in part.named_parameters() if q.requires_grad]
        assert params
        for n, q in params:
            assert q.grad is not None and bool(torch.isfinite(q.grad).all()), n
            nonzero += int(bool((q.grad != 0).any()))
    assert nonzero > 0
    # the same model and episode with the weight at 0: the reconstruction losses are what they were, the term is gone
    model.expansion_weight = 0.0
    torch.manual_seed(11)
    plain = model.loss(ep)
    assert len(calls) == 1 and "expansion_loss" not in plain
    for key in ("query_rec_loss", "support_rec_loss", "recon_loss"):
        assert torch.equal(plain[key].detach(), out[key].detach()), key
    if not rep_w:
        assert torch.equal(plain["ttl_loss"].detach(), plain["recon_loss"].detach())


def test_the_expansion_gradient_alone_reaches_the_decoder(gpu):
    """``expansion_loss`` by itself (not ``ttl_loss``, whose Chamfer part reaches everything anyway)."""
    from fpsg_amd.episodes import synthetic_episode
    model = _episode_model(gpu, "cd", expansion_weight=1.0, expansion_lambda=1.0)
    ep = synthetic_episode(2, 1, n_pts=2048, img_size=96, seed=52, device=gpu)
    out = model.loss(ep)
    assert float(out["expansion_loss"].detach()) > 0
    out["expansion_loss"].sum().backward()
    grads = [q.grad for _, q in model.pc_decoder.named_parameters() if q.grad is not None]
    assert grads and all(bool(torch.isfinite(g).all()) for g in grads) and any(bool((g != 0).any()) for g in grads)


def test_weight_zero_is_the_model_without_the_arguments(gpu, monkeypatch):
    from fpsg_amd import few_shot, metrics
    from fpsg_amd.engine import build_model, default_options
    from fpsg_amd.episodes import synthetic_episode

    def never(*a, **k):
        raise AssertionError("expansion_penalty called with the weight at 0")

    monkeypatch.setattr(few_shot, "expansion_penalty", never)
    ep = synthetic_episode(2, 1, n_pts=2048, img_size=96, seed=51, device=gpu)
    outs = []
    rec = _Recorder()
    metrics.set_launch_probe(rec)
    try:
        for strip in (True, False):
            opt = default_options(device="cuda", intra_recon=True, n_shot=2, n_query=1)
            if strip:
                for f in ("expansion_weight", "expansion_lambda"):
                    delattr(opt, f)                                  # an options namespace from before the flags
            else:
                opt.expansion_weight, opt.expansion_lambda = 0.0, 3.0
            torch.manual_seed(5)
            model = build_model(opt).to(gpu).train()
            torch.manual_seed(12)
            out = model.loss(ep)
            out["ttl_loss"].sum().backward()
            outs.append({n: v.detach().clone() for n, v in out.items()})
    finally:
        metrics.set_launch_probe(None)
    assert rec.kinds and not [k for k in rec.kinds if "expansion" in k], rec.kinds
    assert list(outs[0]) == list(outs[1]) == ["ttl_loss", "recon_loss", "query_rec_loss", "support_rec_loss"]
    for key in outs[0]:
        assert torch.equal(outs[0][key], outs[1][key]), key


def _patch_grids(decoder, B, seed, device):
    """Injected grids ``[cluster][node] -> [B, 2, P]``: one constant per patch plus a small jitter (training-mode BatchNorm
    removes a constant input altogether, so a purely constant grid would decode to the same cloud whatever the constant)."""
    g = torch.Generator().manual_seed(seed)
    P = decoder.pts_per_patch
    return [[(torch.full((B, 2, P), 0.1 + 0.05 * (c * decoder.num_nodes + n)) + 0.05 * torch.rand((B, 2, P), generator=g)).to(device)
             for n in range(decoder.num_nodes)] for c in range(decoder.num_clusters)]


def test_the_decoder_emits_patch_c_n_as_consecutive_rows(gpu):
    """What K24 relies on: patch (cluster c, node n) is rows ``(c * num_nodes + n) * P ..`` of the decoded cloud, on all
    three decode paths -- ``forward``, ``forward`` with a pack, ``forward_pair``.  Decode twice with injected grids that
    differ in ONE patch: exactly that patch's rows move, in every cloud."""
    from fpsg_amd.engine import default_options
    from fpsg_amd.point_cloud_net import PCDecoder
    torch.manual_seed(3)
    dec = PCDecoder(conf=default_options(device="cuda")).to(gpu).train()
    P, R = dec.pts_per_patch, dec.num_nodes
    assert P == 128 and dec.num_clusters * R * P == 2048
    Ba, Bb = 1, 2
    hid_a, hid_b = torch.randn((Ba, 1536), device=gpu), torch.randn((Bb, 1536), device=gpu)
    c0, n0 = 2, 1
    rows = torch.zeros(2048, dtype=torch.bool, device=gpu)
    rows[(c0 * R + n0) * P:(c0 * R + n0 + 1) * P] = True

    def grids(B, seed, changed):
        gr = _patch_grids(dec, B, seed, gpu)
        if changed:
            gr[c0][n0] = 1.0 - gr[c0][n0].flip(2)
        return gr

    def check(before, after, what):
        moved = (before != after).any(-1)                            # [B, 2048]
        for b in range(before.size(0)):
            assert bool(moved[b][rows].any()), (what, b, "the changed patch's rows move")
            assert not bool(moved[b][~rows].any()), (what, b, "no other row does")

    with torch.no_grad():
        pack = dec.pack_parameters()
        for what, fn in (("forward", lambda ch: dec(hid_b, grid=grids(Bb, 7, ch))),
                         ("packed", lambda ch: dec(hid_b, grid=grids(Bb, 7, ch), pack=pack)),
                         ("forward_pair", lambda ch: dec.forward_pair(hid_a, hid_b, pack=pack,
                                                                      grids=(grids(Ba, 8, ch), grids(Bb, 7, ch))))):
            before, after = fn(False), fn(True)
            assert tuple(before.shape)[1:] == (2048, 3)
            check(before, after, what)


# ---- 6. the entry point ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("flags", [["--expansion_weight", "0.1"],
                                   ["--expansion_weight", "0.1", "--repulsion_weight", "0.1", "--clip_grad_norm", "0.5",
                                    "--episodes_per_step", "2"],
                                   []])
def test_training_entry_point_with_the_expansion_term(gpu, tmp_path, flags):
    """trainNetwork.py --expansion_weight 0.1 through the default (graph-replaying) step, alone and beside the repulsion
    term and the clip: one extra line per epoch behind the unchanged ones (and behind the repulsion line); without the
    flag, no such line."""
    env = dict(os.environ, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, "trainNetwork.py", "--synthetic", "--resident", "--n_shot", "2", "--n_query", "1",
                        "--intra_recon", "--epoch", "1", "--n_episode", "2", "--model_path", str(tmp_path), "--name", "x"]
                       + flags, cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    lines = r.stdout.splitlines()
    results = [ln for ln in lines if ln.startswith("Training Results for Epoch")]
    assert len(results) == 1, r.stdout[-3000:]
    m = re.fullmatch(r"Training Results for Epoch -- 1 are: Query_rec: (\S+), Support_rec: (\S+)", results[0])
    assert m and all(math.isfinite(float(v)) and float(v) > 0 for v in m.groups()), results[0]
    exp = [ln for ln in lines if "expansion" in ln]
    if not flags:
        assert exp == [], exp
        return
    assert len(exp) == 1, r.stdout[-3000:]
    m = re.fullmatch(r"  \[expansion: mean (\S+) per cloud\]", exp[0])
    assert m, exp[0]
    v = float(m.group(1))
    assert math.isfinite(v) and v >= 0.0, exp[0]
    at = lines.index(exp[0])
    assert any(x.startswith("Training Results for Epoch") for x in lines[max(0, at - 4):at]), lines[max(0, at - 4):at + 1]
    if "--repulsion_weight" in flags:
        assert re.fullmatch(r"  \[repulsion: mean (\S+) per cloud\]", lines[at - 1]), lines[at - 1]
