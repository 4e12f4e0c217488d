"""K18 on the GPU: the in-degree counts equal ``torch.bincount`` of K1's argmin lists, the values equal a float64
evaluation of the definition on the same fp32 rows within a derived bound, the exact corners are exact, the results do
not depend on the run or the batch, the gradient is as close to float64 as the Chamfer distance's own, and the paths
up to ``trainNetwork.py --pc_dist dcd`` and ``evaluate_Network.py --dcd`` compute what ``metrics.dcd`` gives."""
import math
import os
import re
import statistics
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT, unit_ball_clouds

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (63, 65), (64, 64), (255, 257), (2048, 2048), (4097, 1023), (16384, 3)]
LARGE = {(4097, 1023), (16384, 3)}                                  # run at B <= 5
ALPHAS = (0.0, 1.0, 40.0, 1000.0)
# |dcd - dcd64| and |side - side64|: a term's error is one rounding of alpha * d and one of its product with log2(e)
# (each x 2^-24 e^-x <= 2.2e-8), a couple of ulps of the hardware exponential, of the division and of the subtraction
# on values in [0, 1]: below 3e-7 per term, and the mean inherits it; the fixed tree adds at most log2(N) 2^-24 <= 8.4e-7
# for N <= 16384; the rounded reciprocal and the final product two more ulps of a value <= 1.
BOUND = 2e-6


def _batches(N, M):
    return (1, 5) if (N, M) in LARGE else (1, 5, 37)


def _ball(B, n, seed, device):
    return torch.from_numpy(unit_ball_clouds(np.random.default_rng(seed), B, n)).to(device).contiguous()


def _collapse(B, N, M, seed, device):
    """Every point of p1 within 1e-3 of c = (0.5, 0, 0); p2[0] = c; the rest of p2 around (-0.5, 0, 0)."""
    g = torch.Generator(device=device).manual_seed(seed)
    c = torch.tensor([0.5, 0.0, 0.0], device=device)
    p1 = c + (torch.rand((B, N, 3), generator=g, device=device) - 0.5) * 1e-3
    p2 = -c + (torch.rand((B, M, 3), generator=g, device=device) - 0.5) * 0.2
    p2[:, 0] = c
    return p1.contiguous(), p2.contiguous()


def _bincounts(idx, n):
    return torch.stack([torch.bincount(idx[b].long(), minlength=n) for b in range(idx.size(0))]).to(torch.int32)


def _check_counts(info, N, M):
    deg1, deg2 = info["deg1"], info["deg2"]
    B = deg1.size(0)
    assert deg1.dtype == torch.int32 and tuple(deg1.shape) == (B, N)
    assert deg2.dtype == torch.int32 and tuple(deg2.shape) == (B, M)
    assert info["idx1"].dtype == torch.int32 and info["idx2"].dtype == torch.int32
    for b in range(B):
        assert torch.equal(deg2[b], torch.bincount(info["idx1"][b], minlength=M).to(torch.int32)), b
        assert torch.equal(deg1[b], torch.bincount(info["idx2"][b], minlength=N).to(torch.int32)), b
    assert (deg1.sum(-1) == M).all() and (deg2.sum(-1) == N).all()


def _dcd64(info, alpha):
    """The definition in float64 on K1's fp32 rows: ``(dcd [B], sides [B,2])``."""
    sides = []
    for d, idx, n_target in ((info["dist1"], info["idx1"], info["dist2"].size(1)),
                             (info["dist2"], info["idx2"], info["dist1"].size(1))):
        deg = _bincounts(idx, n_target).double()
        q = torch.exp(-float(alpha) * d.double()) / deg.gather(1, idx.long())
        sides.append((1.0 - q).mean(-1))
    sides = torch.stack(sides, dim=1)
    return 0.5 * (sides[:, 0] + sides[:, 1]), sides


# ---- 1. the counts -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("N,M", SHAPES)
def test_counts_equal_bincount_on_unit_ball_clouds(gpu, N, M):
    from fpsg_amd.metrics import dcd
    for B in _batches(N, M):
        p1, p2 = _ball(B, N, 100 + N, gpu), _ball(B, M, 200 + M, gpu)
        out, info = dcd(p1, p2, return_info=True)
        assert out.dtype == torch.float32 and tuple(out.shape) == (B,) and tuple(info["sides"].shape) == (B, 2)
        assert set(info) == {"sides", "deg1", "deg2", "dist1", "dist2", "idx1", "idx2"}
        _check_counts(info, N, M)
        assert bool(((out >= 0) & (out <= 1)).all())


@pytest.mark.parametrize("N,M", SHAPES)
def test_counts_when_every_point_chooses_one_target(gpu, N, M):
    """The collapse case: deg == N on one target, the LDS histogram's worst case (one address for every add)."""
    from fpsg_amd.metrics import dcd
    for B in _batches(N, M):
        p1, p2 = _collapse(B, N, M, 7 + N, gpu)
        _, info = dcd(p1, p2, return_info=True)
        _check_counts(info, N, M)
        assert (info["deg2"][:, 0] == N).all() and (info["deg2"][:, 1:] == 0).all()
        assert (info["idx1"] == 0).all()


@pytest.mark.parametrize("N,K", [(63, 33), (255, 129), (2048, 1024), (4097, 511)])
def test_counts_on_duplicated_targets_go_to_the_lowest_index(gpu, N, K):
    from fpsg_amd.metrics import dcd
    B = 5
    base = _ball(B, K, 300 + K, gpu)
    p1, p2 = _ball(B, N, 400 + N, gpu), torch.cat([base, base, base[:, :1]], dim=1).contiguous()   # M = 2 K + 1
    _, info = dcd(p1, p2, return_info=True)
    _check_counts(info, N, 2 * K + 1)
    assert (info["deg2"][:, K:] == 0).all() and (info["deg2"][:, :K].sum(-1) == N).all()
    # and the other way: duplicated sources all choose, and all count
    _, back = dcd(p2, p1, return_info=True)
    _check_counts(back, 2 * K + 1, N)
    assert torch.equal(back["deg1"], info["deg2"]) and torch.equal(back["deg2"], info["deg1"])


# ---- 2. the values against float64 on the same rows ----------------------------------------------------------------

@pytest.mark.parametrize("N,M", SHAPES)
def test_values_against_float64_on_the_same_rows(gpu, N, M):
    from fpsg_amd.metrics import dcd
    B = 5
    worst = 0.0
    for name, (p1, p2) in (("ball", (_ball(B, N, 500 + N, gpu), _ball(B, M, 600 + M, gpu))),
                           ("collapse", _collapse(B, N, M, 9 + N, gpu))):
        for alpha in ALPHAS:
            out, info = dcd(p1, p2, alpha, return_info=True)
            want, want_sides = _dcd64(info, alpha)
            err = float((out.double() - want).abs().max())
            err_s = float((info["sides"].double() - want_sides).abs().max())
            worst = max(worst, err, err_s)
            print(f"dcd vs float64 N={N} M={M} {name} alpha={alpha}: |dcd| {err:.3e} |sides| {err_s:.3e}")
            assert err <= BOUND and err_s <= BOUND, (name, alpha, err, err_s)
            assert torch.equal(out, 0.5 * (info["sides"][:, 0] + info["sides"][:, 1]))
    print(f"dcd vs float64 N={N} M={M}: worst {worst:.3e} (bound {BOUND})")


# ---- 3. exact corners --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("N", [1, 255, 2048, 4097])
def test_a_cloud_against_itself_is_exactly_zero(gpu, N):
    from fpsg_amd.metrics import dcd
    p = _ball(3, N, 700 + N, gpu)
    assert all(len(set(map(tuple, c.tolist()))) == N for c in p)    # distinct points
    for alpha in (0.0, 1.0, 1000.0, 1e30):
        out, info = dcd(p, p.clone(), alpha, return_info=True)
        assert (out == 0.0).all() and (info["sides"] == 0.0).all(), (alpha, out)
        assert (info["deg1"] == 1).all() and (info["deg2"] == 1).all()


def test_far_clouds_are_exactly_one(gpu):
    from fpsg_amd.metrics import dcd
    g = torch.Generator(device=gpu).manual_seed(11)
    c = torch.tensor([0.5, 0.0, 0.0], device=gpu)
    p1 = (c + (torch.rand((3, 2048, 3), generator=g, device=gpu) - 0.5) * 0.1).contiguous()
    p2 = (-c + (torch.rand((3, 2048, 3), generator=g, device=gpu) - 0.5) * 0.1).contiguous()
    out, info = dcd(p1, p2, 1000.0, return_info=True)
    assert float(info["dist1"].min()) >= 0.25 and float(info["dist2"].min()) >= 0.25
    # exp(-250) underflows to 0, a sum of 2048 ones and the power-of-two mean round nowhere
    assert (out == 1.0).all() and (info["sides"] == 1.0).all(), out


@pytest.mark.parametrize("N,M", [(64, 64), (2048, 2048), (16384, 3)])
def test_alpha_zero_on_the_collapse_case(gpu, N, M):
    """alpha = 0: q1 = 1 / N on every point, side1 = 1 - 1/N.  N is a power of two here, so every step is exact in fp32
    (1/N, 1 - 1/N, the sum N - 1 and the product); the check allows the one ulp the issue grants."""
    from fpsg_amd.metrics import dcd
    p1, p2 = _collapse(3, N, M, 13, gpu)
    _, info = dcd(p1, p2, 0.0, return_info=True)
    want = np.float32(1.0) - np.float32(1.0) / np.float32(N)
    ulp = float(np.spacing(want))
    assert float((info["sides"][:, 0].double() - float(want)).abs().max()) <= ulp, info["sides"]


# ---- 4. determinism ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("N,M", [(255, 257), (2048, 2048)])
def test_bits_do_not_depend_on_the_run_the_batch_or_the_order_of_the_clouds(gpu, N, M):
    from fpsg_amd.metrics import dcd
    B = 37
    p1, p2 = _ball(B, N, 800 + N, gpu), _ball(B, M, 900 + M, gpu)
    for alpha in (40.0, 1000.0):
        a, ia = dcd(p1, p2, alpha, return_info=True)
        b, ib = dcd(p1, p2, alpha, return_info=True)
        assert not a.requires_grad and a.grad_fn is None            # no input requires grad
        assert torch.equal(a, b) and all(torch.equal(ia[k], ib[k]) for k in ia)
        for k in (0, 17, 36):                                       # a pair alone equals its slice of the batch
            one, io = dcd(p1[k:k + 1].contiguous(), p2[k:k + 1].contiguous(), alpha, return_info=True)
            assert torch.equal(one, a[k:k + 1]) and torch.equal(io["sides"], ia["sides"][k:k + 1])
            assert torch.equal(io["deg1"], ia["deg1"][k:k + 1]) and torch.equal(io["deg2"], ia["deg2"][k:k + 1])
        s, is_ = dcd(p2, p1, alpha, return_info=True)               # swapped: same bits, sides and counts swapped
        assert torch.equal(s, a) and torch.equal(is_["sides"], ia["sides"].flip(1))
        assert torch.equal(is_["deg1"], ia["deg2"]) and torch.equal(is_["deg2"], ia["deg1"])
        assert 0.0 < float(a.min()) and float(a.max()) <= 1.0


def test_values_survive_a_graph_replay(gpu):
    """The call only enqueues: it can be captured, and the replay gives the eager bits."""
    from fpsg_amd.metrics import dcd
    p1, p2 = _ball(5, 255, 21, gpu), _ball(5, 257, 22, gpu)
    eager = dcd(p1, p2, 40.0)
    a, b = p1.clone(), p2.clone()
    dcd(a, b, 40.0)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = dcd(a, b, 40.0)
    a.copy_(p2[:, :255])                                            # other clouds in between
    b.copy_(torch.cat([p1, p1[:, :2]], dim=1))
    g.replay()
    a.copy_(p1)
    b.copy_(p2)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager)


# ---- 5. the gradient ---------------------------------------------------------------------------------------------

def _dev_per_cloud(g, g64):
    """max|g - g64| / max|g64| for every cloud of a [B,n,3] gradient."""
    return ((g.double() - g64).abs().amax((1, 2)) / g64.abs().amax((1, 2))).tolist()


@pytest.mark.parametrize("alpha", [1.0, 40.0])
def test_gradient_against_float64_with_chamfers_own_deviation_as_the_yardstick(gpu, alpha):
    """Reference: the float64 gradient of the definition with K1's indices and K18's counts held constant.  Yardstick:
    the deviation of the existing chamfer_distance gradient from ITS float64 counterpart on the same clouds, same norm
    (max|g - g64| / max|g64| per cloud); DCD's must be within 4x that plus 2e-6 (the factor of tests/_gradcheck.py).

    The test prints both figures; DESIGN.md K18 (*Measured*) is where they are recorded once run on an MI355X."""
    from fpsg_amd.metrics import chamfer_distance, dcd
    B, n = 3, 256
    up = torch.tensor([1.0, 0.5, 2.0], device=gpu)                  # the upstream gradient, not all ones
    p1 = _ball(B, n, 31, gpu).requires_grad_()
    p2 = _ball(B, n, 32, gpu).requires_grad_()
    out, info = dcd(p1, p2, alpha, return_info=True)
    assert out.requires_grad
    g1, g2 = torch.autograd.grad((out * up).sum(), [p1, p2])
    idx1, idx2 = info["idx1"].long(), info["idx2"].long()

    def rows64(a, b):
        d1 = (a - b.gather(1, idx1[..., None].expand(-1, -1, 3))).pow(2).sum(-1)
        d2 = (b - a.gather(1, idx2[..., None].expand(-1, -1, 3))).pow(2).sum(-1)
        return d1, d2

    a, b = p1.detach().double().requires_grad_(), p2.detach().double().requires_grad_()
    d1, d2 = rows64(a, b)
    q1 = torch.exp(-alpha * d1) / info["deg2"].double().gather(1, idx1)
    q2 = torch.exp(-alpha * d2) / info["deg1"].double().gather(1, idx2)
    ref = 0.5 * ((1 - q1).mean(-1) + (1 - q2).mean(-1))
    r1, r2 = torch.autograd.grad((ref * up.double()).sum(), [a, b])
    # (the float64 graph is the same function)
    assert float((out.detach().double() - ref.detach()).abs().max()) <= 2e-6

    c1, c2 = torch.autograd.grad((chamfer_distance(p1, p2) * up).sum(), [p1, p2])
    a, b = p1.detach().double().requires_grad_(), p2.detach().double().requires_grad_()
    d1, d2 = rows64(a, b)
    y1, y2 = torch.autograd.grad(((d1.mean(-1) + d2.mean(-1)) * up.double()).sum(), [a, b])

    dev = _dev_per_cloud(g1, r1) + _dev_per_cloud(g2, r2)
    yard = _dev_per_cloud(c1, y1) + _dev_per_cloud(c2, y2)
    print(f"dcd gradient alpha={alpha}: deviation from float64 per cloud, DCD max {max(dev):.3e} {dev} | "
          f"Chamfer (yardstick) max {max(yard):.3e} {yard}")
    assert float(r1.abs().max()) > 1e-6 and float(r2.abs().max()) > 1e-6     # the weights are far from underflow
    for k, (d, y) in enumerate(zip(dev, yard)):
        assert d <= 4.0 * y + 2e-6, (k, d, y)


def test_gradient_corners(gpu):
    from fpsg_amd.metrics import dcd
    B, n = 3, 256
    # an input that needs no gradient gets none, and the other's gradient keeps its bits
    p1, p2 = _ball(B, n, 41, gpu).requires_grad_(), _ball(B, n, 42, gpu)
    p2g = p2.clone().requires_grad_()
    both1, both2 = torch.autograd.grad(dcd(p1, p2g, 40.0).sum(), [p1, p2g])
    dcd(p1, p2, 40.0).sum().backward()
    assert p2.grad is None and p1.grad is not None and torch.equal(p1.grad, both1)
    q1, q2 = _ball(B, n, 41, gpu), _ball(B, n, 42, gpu).requires_grad_()
    dcd(q1, q2, 40.0).sum().backward()
    assert q1.grad is None and torch.equal(q2.grad, both2) and float(q2.grad.abs().max()) > 0
    # alpha = 0: the value does not depend on the coordinates, the gradients are exactly zero
    z1, z2 = _ball(B, n, 43, gpu).requires_grad_(), _ball(B, n, 44, gpu).requires_grad_()
    dcd(z1, z2, 0.0).sum().backward()
    assert (z1.grad == 0).all() and (z2.grad == 0).all()


# ---- 6. the training path ------------------------------------------------------------------------------------------

def test_episode_losses_are_the_sums_of_dcd_over_the_decoded_pairs(gpu, monkeypatch):
    from fpsg_amd import few_shot, metrics
    from fpsg_amd.engine import build_model, default_options
    from fpsg_amd.episodes import synthetic_episode
    torch.manual_seed(5)
    S, Q, alpha = 2, 1, 40.0
    model = build_model(default_options(device="cuda", pc_dist="dcd", dcd_alpha=alpha, intra_recon=True, n_shot=S,
                                        n_query=Q)).to(gpu).train()
    assert model.dcd_alpha == alpha
    calls = []
    inner = metrics.dcd

    def spy(a, b, *args, **kw):
        calls.append((a.detach().clone(), b.detach().clone(), args, kw))
        return inner(a, b, *args, **kw)

    monkeypatch.setattr(few_shot, "dcd", spy)
    ep = synthetic_episode(S, Q, n_pts=2048, img_size=96, seed=50, device=gpu)
    out = model.loss(ep)
    assert len(calls) == 1, "the query and support pairs go through ONE dcd call"
    syn, ref, args, kw = calls[0]
    assert syn.size(0) == Q + S and ref.size(0) == Q + S and (args == (alpha,) or kw == {"alpha": alpha})
    each = torch.cat([inner(syn[k:k + 1].contiguous(), ref[k:k + 1].contiguous(), alpha) for k in range(Q + S)])
    want_q, want_s = float(each[:Q].double().sum()), float(each[Q:].double().sum())
    assert abs(float(out["query_rec_loss"].detach()) - want_q) <= 1e-6 * want_q
    assert abs(float(out["support_rec_loss"].detach()) - want_s) <= 1e-6 * want_s
    want = model.query_factor * want_q + model.support_factor * want_s
    assert abs(float(out["ttl_loss"].detach()) - want) <= 1e-6 * want
    assert 0.0 < want_q <= Q and 0.0 < want_s <= S
    out["ttl_loss"].sum().backward()
    nonzero = 0
    for part in (model.pc_decoder, model.img_encoder):
        params = [(n, p) for n, p in part.named_parameters() if p.requires_grad]
        assert params
        for n, p in params:
            assert p.grad is not None and bool(torch.isfinite(p.grad).all()), n
            nonzero += int(bool((p.grad != 0).any()))
    assert nonzero > 0


def test_training_entry_point_with_dcd(gpu, tmp_path):
    """trainNetwork.py --pc_dist dcd through the default (graph-replaying) step: two eager episodes, the capture, and
    replays; every printed loss is a mean of sums of values in [0, 1]."""
    env = dict(os.environ, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, "trainNetwork.py", "--synthetic", "--resident", "--n_shot", "2", "--n_query", "1",
                        "--intra_recon", "--pc_dist", "dcd", "--dcd_alpha", "40", "--epoch", "2", "--n_episode", "4",
                        "--model_path", str(tmp_path), "--name", "d"], cwd=ROOT, env=env, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("Training Results for Epoch")]
    assert len(lines) == 2, r.stdout[-3000:]
    n_pairs, top = 2 + 1, 1.0                                        # S + Q pairs, max(query_factor, support_factor)
    for ln in lines:
        m = re.search(r"Query_rec: (\S+), Support_rec: (\S+)$", ln)
        assert m, ln
        for v in map(float, m.groups()):
            assert math.isfinite(v) and 0.0 <= v <= n_pairs * top, ln
    # the evaluation at the last epoch reports the same metric per class: "Class: <c> -- Rec CD: <mean> (<spread>)"
    classes = [ln for ln in r.stdout.splitlines() if ln.startswith("Class: ") and "Rec CD: " in ln]
    assert classes, r.stdout[-3000:]
    for ln in classes:
        v = float(ln.split("Rec CD: ")[1].split()[0])
        assert math.isfinite(v) and 0.0 <= v <= n_pairs * top, ln


# ---- 7. the evaluation path ----------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def model(gpu):
    from fpsg_amd.engine import build_model, default_options
    torch.manual_seed(3)
    return build_model(default_options(device="cuda")).to(gpu).eval()


@pytest.mark.parametrize("Q", [1, 2])
def test_evaluation_item_dcd(gpu, model, Q):
    """EvalItem(dcd=alpha): the new field is the mean of ``metrics.dcd`` over the clouds the item returns, eager items and
    graph replays alike; without it the item is what it was."""
    from fpsg_amd.engine import EvalItem
    from fpsg_amd.episodes import synthetic_episode
    from fpsg_amd.metrics import dcd
    eps = [synthetic_episode(1, Q, n_pts=2048, img_size=96, seed=60 + i, device=gpu) for i in range(4)]
    with EvalItem(model) as item:
        assert all(set(item(ep)) == {"cd_loss", "emd_loss"} for ep in eps[:1])
    with EvalItem(model, dcd=1000.0, return_clouds=True) as item:
        got = [item(ep) for ep in eps]
        assert item._graphs, "the third item of a shape is captured"
    for g in got:
        assert set(g) == {"cd_loss", "emd_loss", "dcd", "syn_pc", "ref_pc_q"}
        want = dcd(g["syn_pc"].contiguous(), g["ref_pc_q"].contiguous(), 1000.0)
        assert tuple(want.shape) == (Q,)
        assert g["dcd"].dim() == 0 and not g["dcd"].requires_grad and torch.equal(g["dcd"], want.mean())
        assert 0.0 < float(g["dcd"]) <= 1.0
    with EvalItem(model, dcd=1000.0) as item:
        alone = item(eps[0])
    assert set(alone) == {"cd_loss", "emd_loss", "dcd"}


def test_evaluation_entry_point_column_and_values(gpu, tmp_path, capsys):
    import evaluate_Network
    from fpsg_amd import cli
    argv = ["--synthetic", "--n_shot", "2", "--n_query", "2", "--sequential_eval", "--model_path", str(tmp_path),
            "--name", "x"]
    parser = cli.few_shot_parser(evaluation=True)

    def run(extra):
        torch.manual_seed(0)
        res = evaluate_Network.main(parser.parse_args(argv + extra))
        return res, [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("Class: ")]

    res_plain, plain = run([])
    res_flag, flagged = run(["--dcd"])
    assert len(res_plain) == 2 and len(res_flag) == 3               # one more element, only with the flag
    assert plain and len(plain) == len(flagged)
    for pl, ln in zip(plain, flagged):
        head, sep, tail = ln.partition("; DCD: ")
        assert sep and head == pl and "DCD" not in pl, (pl, ln)    # cut off the new column: today's line, every character
        assert ln.count("; DCD: ") == 1 and "; " not in tail
    res, lines = run(["--fscore", "0.02", "--dcd", "40", "--set_metrics"])
    assert len(res) == 5 and len(lines) == len(plain)
    per_class = res[-1]                                             # appended last
    assert set(per_class) == set(res[0])
    for ln in lines:
        name = ln.split(" -- ")[0][len("Class: "):]
        fields = ln.split(" -- ")[1].split("; ")
        assert [f.split(": ")[0] for f in fields] == ["Rec CD", "Rec EMD", "F@0.02", "HD", "DCD", "MMD-CD", "COV-CD",
                                                      "1-NNA-CD"], ln
        value = float(dict(f.split(": ") for f in fields)["DCD"])
        assert value == statistics.mean(per_class[name]) and len(per_class[name]) == len(res[0][name])
        assert all(0.0 < v <= 1.0 for v in per_class[name])
    # alpha reaches the kernel: 40 and 1000 give different values on the same items
    assert res_flag[-1] != per_class
