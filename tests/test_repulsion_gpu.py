"""K21 on the GPU: the neighbour lists are those of a float64 full sort bit for bit where every distance
is exact in fp32; on unit-ball clouds every list is a valid k-nearest list in float64 and the value and the gradient
agree with the float64 reference on the kernel's own lists to the project's 1e-4; the corners are exact; nothing
depends on the run, the batch or a graph replay; and the term reaches ``model.loss`` and ``trainNetwork.py``.

The checker is ``tests/_repulsion_ref.py`` (float64 torch), run on the device."""
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT, unit_ball_clouds

import _repulsion_ref as ref

pytestmark = pytest.mark.gpu

BOUND = 1e-4                                                         # the project's parity bar


def _ball(B, n, seed, device):
    return torch.from_numpy(unit_ball_clouds(np.random.default_rng(seed), B, n)).to(device).contiguous()


def _grid_clouds(N, seed, device):
    """Three clouds with coordinates integer / 64 in [-1, 1] (every d2 an integer multiple of 2^-12 below 2^4: exact in
    fp32 whatever the fma order): random on the full grid (distance ties); random on 9 levels per axis (ties and, from
    a few hundred points up, repeated points); distinct points whose second half repeats the first (point i and
    i + N // 2 coincide)."""
    g = torch.Generator().manual_seed(seed)
    fine = torch.randint(-64, 65, (N, 3), generator=g)
    coarse = torch.randint(-4, 5, (N, 3), generator=g) * 16
    half = N // 2
    cells = torch.randperm(129 ** 3, generator=g)[:N - half]
    uniq = torch.stack([cells % 129, (cells // 129) % 129, cells // (129 * 129)], dim=1) - 64
    dup = torch.cat([uniq, uniq[:half]])
    return (torch.stack([fine, coarse, dup]).float() / 64.0).to(device).contiguous(), half


def _run(p, k, h=0.03, up=None):
    """``(value, idx, d2, grad)`` of ``metrics.repulsion_loss``; ``up [B]`` is the upstream gradient (default: ones)."""
    from fpsg_amd.metrics import repulsion_loss
    x = p.clone().requires_grad_()
    out, info = repulsion_loss(x, k, h, return_info=True)
    assert out.dtype == torch.float32 and tuple(out.shape) == (p.size(0),) and set(info) == {"idx", "d2"}
    assert info["idx"].dtype == torch.int32 and tuple(info["idx"].shape) == (p.size(0), p.size(1), k)
    assert info["d2"].dtype == torch.float32 and tuple(info["d2"].shape) == (p.size(0), p.size(1), k)
    (g,) = torch.autograd.grad((out * (torch.ones_like(out) if up is None else up)).sum(), [x])
    return out.detach(), info["idx"], info["d2"], g


# ---- 1. the neighbour lists, bit for bit -----------------------------------------------------------------------------

OTHER_K = (2, 3, 5, 6, 7)           # repulsion_fwd_kernel<K> / repulsion_bwd_kernel<K> are compiled for every K in 1..8


@pytest.mark.parametrize("N,k", [(N, k) for k in (1, 4, 8) for N in ("k+1", 63, 64, 65, 257, 1000)]
                         + [(N, k) for k in OTHER_K for N in ("k+1", 65)])
def test_lists_equal_the_float64_full_sort_on_exact_distances(gpu, N, k):
    N = k + 1 if N == "k+1" else N
    p, half = _grid_clouds(N, 100 * k + N, gpu)
    _, idx, d2, _ = _run(p, k)
    want_idx, want_d2 = ref.neighbour_lists(p, k)
    assert torch.equal(idx.long(), want_idx), "every row of every cloud"
    assert torch.equal(d2.double(), want_d2)
    own = torch.arange(N, device=gpu)[None, :, None]
    assert not bool((idx == own).any()), "a point is never its own neighbour"
    # the third cloud: a duplicate of i is in K(i), first, at distance 0
    first = idx[2, :, 0].long()
    i = torch.arange(half, device=gpu)
    assert torch.equal(first[:half], i + (N - half)) and torch.equal(first[N - half:], i)
    assert bool((d2[2, :half, 0] == 0).all()) and bool((d2[2, N - half:, 0] == 0).all())


def test_lists_at_the_largest_cloud_cross_candidate_tiles(gpu):
    N, k = 16384, 4
    g = torch.Generator().manual_seed(9)
    p = (torch.randint(-64, 65, (1, N, 3), generator=g).float() / 64.0).to(gpu).contiguous()
    p[0, N - 5] = p[0, 3]                                            # a duplicate sixteen tiles away
    _, idx, d2, _ = _run(p, k)
    want_idx, want_d2 = ref.neighbour_lists(p, k)
    assert torch.equal(idx.long(), want_idx) and torch.equal(d2.double(), want_d2)
    assert int(idx[0, 3, 0]) == N - 5 and int(idx[0, N - 5, 0]) == 3


# ---- 2. values and gradients against float64 on the kernel's own lists ---------------------------------------------------

def _check_lists_valid_in_float64(p, idx, d2_32):
    """Members distinct, never i, ascending, and no non-member nearer than the farthest member -- in float64, with the
    slack 1e-5 for what fp32 may order differently: the fp32 d2 of the direct-difference form is within a few 2^-24 of
    the float64 one, so two distances closer than that may legitimately swap."""
    B, N, k = idx.shape
    x = p.double()
    D = (x[:, None, :, :] - x[:, :, None, :]).pow(2).sum(-1)        # [B,N,N]
    own = torch.arange(N, device=p.device)
    D[:, own, own] = float("inf")
    li = idx.long()
    assert bool(((li >= 0) & (li < N)).all())
    assert not bool((li == own[None, :, None]).any())
    srt = li.sort(dim=2).values
    assert bool((srt[:, :, 1:] != srt[:, :, :-1]).all()), "members are distinct"
    member = D.gather(2, li)
    assert bool((d2_32[:, :, 1:] >= d2_32[:, :, :-1]).all()), "ascending in the kernel's own fp32 distances"
    assert bool((member[:, :, :-1] <= (1 + 1e-5) * member[:, :, 1:]).all()), "ascending in float64"
    assert float(((d2_32.double() - member).abs() / member.clamp_min(1e-30)).max()) <= 1e-5
    rest = D.scatter(2, li, float("inf")).amin(2)                    # nearest non-member (inf when N = k + 1)
    assert bool((member[:, :, -1] <= (1 + 1e-5) * rest).all())


@pytest.mark.parametrize("N,k", [(N, k) for k in (1, 4, 8) for N in (65, 300, 2048)] + [(65, k) for k in OTHER_K])
def test_value_and_gradient_against_float64(gpu, N, k):
    """Two unit-ball clouds and one tanh(randn) cloud (the decoder's range), h = 0.03 and 0.3.  The reference gets the
    KERNEL's lists, so a near-tie ordered differently in fp32 excludes no row.  Prints the measured deviations
    (*Measured*)."""
    g = torch.Generator().manual_seed(N + k)
    p = torch.cat([_ball(2, N, 7 * N + k, gpu), torch.tanh(torch.randn((1, N, 3), generator=g)).to(gpu)]).contiguous()
    up = torch.tensor([1.0, 0.5, 2.0], device=gpu)                   # the upstream gradient, not all ones
    checked = False
    for h in (0.03, 0.3):
        R, idx, d2, grad = _run(p, k, h, up)
        if not checked:
            _check_lists_valid_in_float64(p, idx, d2)
            checked = True
        R64, g64 = ref.value_and_grad(p, idx, h, up)
        assert bool(torch.isfinite(R).all()) and bool(torch.isfinite(grad).all())
        assert bool((R <= 0).all()) and bool((R.double() >= -h / math.sqrt(2 * math.e) * (1 + 1e-6)).all())
        dev_R = ((R.double() - R64).abs() / R64.abs()).tolist()
        dev_g = ((grad.double() - g64).abs().amax((1, 2)) / g64.abs().amax((1, 2))).tolist()
        print(f"repulsion vs float64 N={N} k={k} h={h}: |R - R64| / |R64| per cloud {dev_R}; "
              f"max|g - g64| / max|g64| per cloud {dev_g}; R64 {R64.tolist()}")
        assert float(R64.abs().min()) > 0 and float(g64.abs().amax((1, 2)).min()) > 0
        assert max(dev_R) <= BOUND and max(dev_g) <= BOUND, (h, dev_R, dev_g)


# ---- 3. corners ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("N,k", [(64, 1), (64, 4), (64, 8), (512, 1), (512, 4), (512, 8), (100, 3)])
def test_every_point_identical(gpu, N, k):
    """Every d2 is 0: the lists are the lowest indices != i, every pair term is -1e-6 * exp(0), nobody is pushed.  Where
    N * k is a power of two and N a multiple of 64 every partial sum is a power of two times fp32(1e-6) and the mean is
    fp32(-1e-6) exactly; at (100, 3) the sums round (at most 15 additions deep, 2^-24 each): 1e-6 relative."""
    p = torch.tensor([0.3, -0.2, 0.7], device=gpu).expand(2, N, 3).contiguous()
    R, idx, d2, grad = _run(p, k)
    assert bool((d2 == 0).all())
    want = torch.stack([torch.tensor([j for j in range(k + 1) if j != i][:k]) for i in range(N)]).to(gpu)
    assert torch.equal(idx.long(), want.expand(2, N, k))
    exact = torch.full((2,), -1e-6, dtype=torch.float32, device=gpu)
    if (N, k) == (100, 3):
        assert float(((R - exact).abs() / exact.abs()).max()) <= 1e-6
    else:
        assert torch.equal(R, exact), R.tolist()
    assert bool(torch.isfinite(grad).all()) and bool((grad == 0).all())


@pytest.mark.parametrize("k", [1, 4, 8])
def test_two_far_clusters_never_share_neighbours(gpu, k):
    g = torch.Generator().manual_seed(21)
    c = torch.tensor([0.5, 0.0, 0.0])
    p = torch.cat([-c + (torch.rand((2, 32, 3), generator=g) - 0.5) * 0.02,
                   c + (torch.rand((2, 32, 3), generator=g) - 0.5) * 0.02], dim=1).to(gpu).contiguous()
    R, idx, _, grad = _run(p, k)
    assert bool((idx[:, :32] < 32).all()) and bool((idx[:, 32:] >= 32).all())
    R64, g64 = ref.value_and_grad(p, idx, 0.03)
    assert float(((R.double() - R64).abs() / R64.abs()).max()) <= BOUND
    assert float(((grad.double() - g64).abs().amax((1, 2)) / g64.abs().amax((1, 2))).max()) <= BOUND


def test_a_hub_that_is_in_every_list(gpu):
    """One point with N - 1 others on the unit sphere around it, pairwise further apart than 1, k = 1: the hub is the
    nearest neighbour of every other point, so the lane that owns it gathers N - 1 reverse terms.  Points on a unit
    sphere that are pairwise further apart than 1 are at most 12 (the kissing number in three dimensions; it also
    bounds the in-degree of any nearest-neighbour graph there), so N is 13 -- the icosahedron's vertices, edge 1.0515
    -- not the 200 the issue names, which no cloud in three dimensions can give.  Both positions of the hub."""
    t = (1 + math.sqrt(5)) / 2
    v = torch.tensor([[0, 1, t], [0, -1, t], [0, 1, -t], [0, -1, -t], [1, t, 0], [-1, t, 0], [1, -t, 0], [-1, -t, 0],
                      [t, 0, 1], [-t, 0, 1], [t, 0, -1], [-t, 0, -1]], dtype=torch.float64)
    v = v / v.norm(dim=1, keepdim=True)
    assert float(torch.cdist(v, v)[~torch.eye(12, dtype=torch.bool)].min()) > 1.05
    hub = torch.zeros((1, 3), dtype=torch.float64)
    centre = torch.tensor([0.1, -0.2, 0.05], dtype=torch.float64)
    p = torch.stack([torch.cat([hub, v]), torch.cat([v, hub])]).add(centre).float().to(gpu).contiguous()
    N = 13
    for h in (0.3, 1.0):
        R, idx, d2, grad = _run(p, 1, h)
        for b, at in ((0, 0), (1, N - 1)):
            others = [i for i in range(N) if i != at]
            assert bool((idx[b, others, 0] == at).all()), "the hub is in every list: in-degree N - 1"
            assert int((idx[b, :, 0] == at).sum()) == N - 1
        R64, g64 = ref.value_and_grad(p, idx, h)
        dev_R = float(((R.double() - R64).abs() / R64.abs()).max())
        dev_g = float(((grad.double() - g64).abs().amax((1, 2)) / g64.abs().amax((1, 2))).max())
        print(f"repulsion hub h={h}: value {dev_R:.3e} gradient {dev_g:.3e}")
        assert dev_R <= BOUND and dev_g <= BOUND


def test_bandwidth_extremes(gpu):
    p = _ball(3, 300, 77, gpu)
    # h so large that exp is 1 to rounding: R = -mean r
    R, idx, d2, grad = _run(p, 4, 1e4)
    R64, g64 = ref.value_and_grad(p, idx, 1e4)
    assert float(((R.double() - R64).abs() / R64.abs()).max()) <= BOUND
    assert float(((grad.double() - g64).abs().amax((1, 2)) / g64.abs().amax((1, 2))).max()) <= BOUND
    assert float(((R.double() + d2.double().sqrt().mean((1, 2))).abs() / R64.abs()).max()) <= 1e-6
    # h so small that every term underflows: d2 / h^2 is beyond 150 everywhere, v_exp_f32 gives +0
    for h in (2e-4, 1e-30):
        assert float(d2.min()) / (h * h) > 150
        R, _, _, grad = _run(p, 4, h)
        assert bool((R == 0).all()), R.tolist()
        assert bool(torch.isfinite(grad).all()) and bool((grad == 0).all())


# ---- 4. reproducibility --------------------------------------------------------------------------------------------------

def test_bits_do_not_depend_on_the_run_or_the_batch(gpu):
    N, k, h = 300, 4, 0.1
    p = _ball(5, N, 31, gpu)
    p[4] = p[0]
    up = torch.tensor([1.5, 1.0, 0.5, 2.0, 1.5], device=gpu)
    a = _run(p, k, h, up)
    b = _run(p, k, h, up)
    assert all(torch.equal(s, t) for s, t in zip(a, b))
    one = _run(p[:1].contiguous(), k, h, up[:1])
    for pos in (0, 4):
        assert all(torch.equal(s, t[pos:pos + 1]) for s, t in zip(one, a)), pos
    assert float(a[3].abs().max()) > 0


def test_bits_survive_a_graph_capture_and_two_replays(gpu):
    from fpsg_amd.metrics import repulsion_loss
    N, k, h = 300, 4, 0.1
    p, other = _ball(3, N, 41, gpu), _ball(3, N, 42, gpu)
    up = torch.tensor([1.0, 0.5, 2.0], device=gpu)
    eager = _run(p, k, h, up)
    x = p.clone().requires_grad_()

    def once():
        out, inf = repulsion_loss(x, k, h, return_info=True)
        (g,) = torch.autograd.grad((out * up).sum(), [x])
        return out.detach(), inf["idx"], inf["d2"], g

    once()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        got = once()
    for _ in range(2):
        with torch.no_grad():
            x.copy_(other)                                           # other clouds in between
        graph.replay()
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


@pytest.mark.parametrize("pc_dist", ["cd", "dcd"])
def test_model_loss_adds_one_call_over_the_decoded_clouds(gpu, monkeypatch, pc_dist):
    """``cd`` takes the fused K1l path (which returns early without the term), ``dcd`` the batched one."""
    from fpsg_amd import few_shot, metrics
    from fpsg_amd.episodes import synthetic_episode
    S, Q, W = 2, 1, 0.5
    model = _episode_model(gpu, pc_dist, repulsion_weight=W, query_factor=1.0, support_factor=0.75)
    assert model.repulsion_weight == W
    calls = []
    inner = metrics.repulsion_loss

    def spy(p, *args, **kwargs):
        calls.append((p.detach().clone(), args, kwargs))
        return inner(p, *args, **kwargs)

    monkeypatch.setattr(few_shot, "repulsion_loss", spy)
    ep = synthetic_episode(S, Q, n_pts=2048, img_size=96, seed=50, device=gpu)
    torch.manual_seed(11)                                            # the decoder's random grid
    out = model.loss(ep)
    assert set(out) == {"ttl_loss", "recon_loss", "query_rec_loss", "support_rec_loss", "repulsion_loss"}
    assert len(calls) == 1, "ONE repulsion_loss call over the Q + S decoded clouds"
    clouds, args, kwargs = calls[0]
    assert tuple(clouds.shape) == (Q + S, 2048, 3) and (args + tuple(kwargs.values())) == (4, 0.03)
    each = torch.cat([inner(clouds[i:i + 1].contiguous(), 4, 0.03) for i in range(Q + S)]).double()
    assert bool((each < 0).all()) and bool((each >= -0.03 / math.sqrt(2 * math.e)).all())
    total = float(each.sum())
    assert abs(float(out["repulsion_loss"].detach()) - total) <= 1e-6 * abs(total)
    want = float(out["recon_loss"].detach().double().sum()) + W * (1.0 * float(each[:Q].sum()) + 0.75 * float(each[Q:].sum()))
    assert abs(float(out["ttl_loss"].detach().double().sum()) - want) <= 1e-6 * abs(want)
    recon = 1.0 * float(out["query_rec_loss"].detach().sum()) + 0.75 * float(out["support_rec_loss"].detach().sum())
    assert abs(float(out["recon_loss"].detach().sum()) - recon) <= 1e-6 * abs(recon)
    out["ttl_loss"].sum().backward()
    nonzero = 0
    for part in (model.pc_decoder, model.img_encoder):
        params = [(n, q) for n, q in part.named_parameters() if q.requires_grad]
        assert params
        for n, q in params:
            assert q.grad is not None and bool(torch.isfinite(q.grad).all()), n
            nonzero += int(bool((q.grad != 0).any()))
    assert nonzero > 0
    # the same model and episode with the weight at 0: the reconstruction losses are what they were, the term is gone
    model.repulsion_weight = 0.0
    torch.manual_seed(11)
    plain = model.loss(ep)
    assert len(calls) == 1 and set(plain) == {"ttl_loss", "recon_loss", "query_rec_loss", "support_rec_loss"}
    for key in ("query_rec_loss", "support_rec_loss", "recon_loss"):
        assert torch.equal(plain[key].detach(), out[key].detach()), key
    assert torch.equal(plain["ttl_loss"].detach(), plain["recon_loss"].detach())


def test_weight_zero_is_the_model_without_the_arguments(gpu, monkeypatch):
    from fpsg_amd import few_shot
    from fpsg_amd.engine import build_model, default_options
    from fpsg_amd.episodes import synthetic_episode

    def never(*a, **k):
        raise AssertionError("repulsion_loss called with the weight at 0")

    monkeypatch.setattr(few_shot, "repulsion_loss", never)
    ep = synthetic_episode(2, 1, n_pts=2048, img_size=96, seed=51, device=gpu)
    outs = []
    for strip in (True, False):
        opt = default_options(device="cuda", intra_recon=True, n_shot=2, n_query=1)
        if strip:
            for f in ("repulsion_weight", "repulsion_k", "repulsion_h"):
                delattr(opt, f)                                      # an options namespace from before the flags
        else:
            opt.repulsion_weight, opt.repulsion_k, opt.repulsion_h = 0.0, 8, 0.5
        torch.manual_seed(5)
        model = build_model(opt).to(gpu).train()
        torch.manual_seed(12)
        outs.append({n: v.detach().clone() for n, v in model.loss(ep).items()})
    assert list(outs[0]) == list(outs[1]) == ["ttl_loss", "recon_loss", "query_rec_loss", "support_rec_loss"]
    for key in outs[0]:
        assert torch.equal(outs[0][key], outs[1][key]), key


# ---- 6. the entry point ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("extra", [[], ["--clip_grad_norm", "0.5", "--episodes_per_step", "2"]])
def test_training_entry_point_with_the_repulsion_term(gpu, tmp_path, extra):
    """trainNetwork.py --repulsion_weight 0.1 through the default (graph-replaying) step: eager episodes, the capture and
    replays; one extra line per epoch behind the unchanged ones."""
    env = dict(os.environ, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, "trainNetwork.py", "--synthetic", "--resident", "--n_shot", "2", "--n_query", "1",
                        "--intra_recon", "--repulsion_weight", "0.1", "--epoch", "2", "--n_episode", "4",
                        "--model_path", str(tmp_path), "--name", "r"] + extra, cwd=ROOT, env=env, capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    lines = r.stdout.splitlines()
    results = [ln for ln in lines if ln.startswith("Training Results for Epoch")]
    assert len(results) == 2, r.stdout[-3000:]
    for n, ln in enumerate(results, 1):
        m = re.fullmatch(rf"Training Results for Epoch -- {n} are: Query_rec: (\S+), Support_rec: (\S+)", ln)
        assert m, ln
        assert all(math.isfinite(float(v)) and float(v) > 0 for v in m.groups()), ln
    rep = [ln for ln in lines if "repulsion" in ln]
    assert len(rep) == 2, r.stdout[-3000:]
    for ln in rep:
        m = re.fullmatch(r"  \[repulsion: mean (\S+) per cloud\]", ln)
        assert m, ln
        v = float(m.group(1))
        assert math.isfinite(v) and -0.03 / math.sqrt(2 * math.e) <= v <= 0.0, ln
    # the new line comes after the epoch's existing lines
    for ln in rep:
        at = lines.index(ln)
        assert any(x.startswith("Training Results for Epoch") for x in lines[max(0, at - 3):at]), lines[max(0, at - 3):at + 1]
