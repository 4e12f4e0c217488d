"""The Sinkhorn divergence's gradient on the GPU (K19): fpsg_sinkhorn_divergence_grad behind
``metrics.sinkhorn_loss`` against the float64 reference of ``tests/_sinkhorn_grad_ref.py``, its identities, graph
capture, and ``--pc_dist sinkhorn`` through the model and the training entry point."""
import math
import os
import re
import subprocess
import sys

import pytest
import torch

import _sinkhorn_grad_ref as ref
from conftest import ROOT

pytestmark = pytest.mark.gpu

FIXED = 2 * math.sqrt(3)
BOUND = 1e-4        # the project's bound for fp32 soft-mins with v_exp_f32 / v_log_f32 against float64


def _apart(seed):
    """0.2-scaled clouds 1.5 apart: every cross weight lies far below the running maximum's first candidates."""
    x, y = ref.clouds(1, 130, 65, seed)
    return (0.2 * x).contiguous(), (0.2 * y + torch.tensor([1.5, 0.0, 0.0])).contiguous()


# ceil(max(N, M) / 128) * 4 * B >= 4 * 256: sinkhorn_step_kernel<2> / sinkhorn_grad_kernel<2> on unequal clouds that fill
# no group of 128 owners
TWO_OWNERS_RAGGED = [(256, 100, 37), (256, 70, 129), (300, 1, 9)]

# (id, clouds, diameter)
PARITY = [
    ("one owner past a wave", lambda: ref.clouds(2, 65, 130, 1), None),
    ("single owner", lambda: ref.clouds(1, 1, 7, 2), None),
    ("single candidate", lambda: ref.clouds(1, 7, 1, 3), None),
    ("ragged 8-chunk", lambda: ref.clouds(3, 300, 257, 4), None),
    ("two LDS tiles", lambda: ref.clouds(1, 2100, 520, 5), None),
    ("two owners per lane", lambda: ref.clouds(64, 512, 512, 6), FIXED),
    ("clouds 1.5 apart", lambda: _apart(7), None),
] + [(f"two owners per lane, ragged {B}x{N}x{M}", lambda B=B, N=N, M=M: ref.clouds(B, N, M, 8), FIXED)
     for B, N, M in TWO_OWNERS_RAGGED]


def _loss_and_grads(x, y, gpu, diameter, weights=None):
    from fpsg_amd.metrics import sinkhorn_loss
    a, b = x.to(gpu).requires_grad_(), y.to(gpu).requires_grad_()
    out = sinkhorn_loss(a, b, diameter=diameter)
    ga, gb = torch.autograd.grad(out.sum() if weights is None else (out * weights).sum(), [a, b])
    return out.detach(), ga, gb


@pytest.mark.parametrize("what,make,diameter", PARITY, ids=[p[0] for p in PARITY])
def test_gradient_against_float64(gpu, what, make, diameter):
    """Largest row-wise Euclidean error over the largest float64 gradient row, gx and gy separately, within 1e-4; the
    value within 1e-4 (relative) as ``test_sinkhorn_vs_independent_float64`` asks of the forward entry."""
    x, y = make()
    S64, gx64, gy64 = ref.closed_form(x, y, diameter=diameter)
    out, gx, gy = _loss_and_grads(x, y, gpu, diameter)
    ex, ey = ref.row_error(gx, gx64), ref.row_error(gy, gy64)
    ev = float(((out.double().cpu() - S64).abs() / S64.abs()).max())
    print(f"sinkhorn gradient [{what}] {tuple(x.shape)} x {tuple(y.shape)}: row error gx {ex:.3e} gy {ey:.3e} "
          f"(largest rows {float(gx64.norm(dim=-1).max()):.3e} {float(gy64.norm(dim=-1).max()):.3e}), value {ev:.3e}")
    assert bool(torch.isfinite(gx).all()) and bool(torch.isfinite(gy).all())
    assert ex <= BOUND and ey <= BOUND, (what, ex, ey)
    assert ev <= BOUND, (what, ev)


@pytest.mark.parametrize("B,N,M", [(3, 300, 257), (1, 2100, 520), (64, 512, 512)] + TWO_OWNERS_RAGGED)
def test_value_is_the_forward_entrys_bit_for_bit(gpu, B, N, M):
    from fpsg_amd.metrics import sinkhorn_divergence, sinkhorn_loss
    x, y = (t.to(gpu) for t in ref.clouds(B, N, M, 11))
    for d in (FIXED, None):
        want = sinkhorn_divergence(x, y, diameter=d)
        assert torch.equal(sinkhorn_loss(x, y, diameter=d), want)                      # no gradient asked for
        a, b = x.clone().requires_grad_(), y.clone().requires_grad_()
        for p1, p2 in ((a, b), (a, y), (x, b)):                                        # both, gx only, gy only
            got = sinkhorn_loss(p1, p2, diameter=d)
            assert got.requires_grad and torch.equal(got.detach(), want), (d, p1 is a, p2 is b)
    assert torch.equal(sinkhorn_loss(x, y), sinkhorn_divergence(x, y))
    plain = sinkhorn_divergence(x.clone().requires_grad_(), y.clone().requires_grad_())
    assert plain.grad_fn is None and not plain.requires_grad


@pytest.mark.parametrize("B,N,M", TWO_OWNERS_RAGGED)
def test_two_owners_per_lane_equal_one_owner_bit_for_bit(gpu, B, N, M):
    """The whole batch takes sinkhorn_step_kernel<2> and sinkhorn_grad_kernel<2>, its first three clouds alone take the
    <1> forms; with a fixed diameter both calls share one epsilon schedule, and an owner's sums are split the same way."""
    assert -(-max(N, M) // 128) * 4 * B >= 4 * 256 > -(-max(N, M) // 128) * 4 * 3
    x, y = ref.clouds(B, N, M, 8)
    out, gx, gy = _loss_and_grads(x, y, gpu, FIXED)
    out3, gx3, gy3 = _loss_and_grads(x[:3].contiguous(), y[:3].contiguous(), gpu, FIXED)
    for whole, chunk in ((out, out3), (gx, gx3), (gy, gy3)):
        assert torch.equal(whole[:3].contiguous().view(torch.int32), chunk.view(torch.int32))


def test_autograd_plumbing(gpu):
    from fpsg_amd.metrics import sinkhorn_loss
    x, y = ref.clouds(3, 300, 257, 12)
    w = torch.tensor([1.0, 0.5, 2.0], device=gpu)
    _, gx, gy = _loss_and_grads(x, y, gpu, FIXED)
    out, wx, wy = _loss_and_grads(x, y, gpu, FIXED, weights=w)
    assert torch.equal(wx, gx * w[:, None, None]) and torch.equal(wy, gy * w[:, None, None])
    assert float(gx.abs().max()) > 0 and float(gy.abs().max()) > 0
    # two runs: the same bits
    out2, wx2, wy2 = _loss_and_grads(x, y, gpu, FIXED, weights=w)
    assert torch.equal(out, out2) and torch.equal(wx, wx2) and torch.equal(wy, wy2)
    # an input that needs no gradient gets none, and the other's keeps its bits
    p1, p2 = x.to(gpu).requires_grad_(), y.to(gpu)
    (sinkhorn_loss(p1, p2, diameter=FIXED) * w).sum().backward()
    assert p2.grad is None and torch.equal(p1.grad, wx)
    q1, q2 = x.to(gpu), y.to(gpu).requires_grad_()
    (sinkhorn_loss(q1, q2, diameter=FIXED) * w).sum().backward()
    assert q1.grad is None and torch.equal(q2.grad, wy)


@pytest.mark.parametrize("B,N", [(2, 300), (64, 512), (1, 2100)])
def test_a_cloud_against_its_copy_has_an_exactly_zero_gradient(gpu, B, N):
    """N = M and bitwise-equal clouds: the four soft-mins run one instruction sequence on equal inputs, so the two
    displacement arrays of each cloud are equal bit for bit, and so are the duals."""
    x, _ = ref.clouds(B, N, 1, 13)
    out, gx, gy = _loss_and_grads(x, x.clone(), gpu, FIXED)
    assert not out.any() and not gx.any() and not gy.any()


def test_one_step_of_the_kernels_gradient_halves_the_divergence(gpu):
    """The step of the CPU test (same clouds), with the kernel's gradient and the forward entry's values."""
    from fpsg_amd.metrics import sinkhorn_divergence
    x, y = ref.gaussian_clouds(1, 300, 257, seed=7)
    _, _, gy = _loss_and_grads(x, y, gpu, None)
    x, y = x.to(gpu), y.to(gpu)
    s0 = float(sinkhorn_divergence(x, y))
    s1 = float(sinkhorn_divergence(x, (y - 0.5 * y.size(1) * gy).contiguous()))
    print(f"descent on the device: {s0:.6e} -> {s1:.6e} (ratio {s1 / s0:.3f})")
    assert 0.0 <= s1 < 0.5 * s0


def test_forward_and_backward_survive_a_graph_replay(gpu):
    """A fixed diameter: the call only enqueues.  Captured after two eager calls, replayed on two other inputs copied
    into the static buffers: the eager bits."""
    from fpsg_amd.metrics import sinkhorn_loss
    B, N, M = 3, 300, 257
    w = torch.tensor([1.0, 0.5, 2.0], device=gpu)
    inputs = [ref.clouds(B, N, M, s) for s in (21, 22, 23)]
    eager = [_loss_and_grads(x, y, gpu, FIXED, weights=w) for x, y in inputs]
    a = inputs[0][0].to(gpu).requires_grad_()
    b = inputs[0][1].to(gpu).requires_grad_()

    def run():
        out = sinkhorn_loss(a, b, diameter=FIXED)
        return (out,) + torch.autograd.grad((out * w).sum(), [a, b])

    side = torch.cuda.Stream(device=gpu)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run()
        run()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        static = run()
    for k in (1, 2):
        with torch.no_grad():
            a.copy_(inputs[k][0])
            b.copy_(inputs[k][1])
        g.replay()
        torch.cuda.synchronize()
        for got, want in zip(static, eager[k]):
            assert torch.equal(got.detach(), want), k


# ---- the training path ---------------------------------------------------------------------------------------------

def test_episode_losses_are_the_sums_of_sinkhorn_loss_over_the_decoded_pairs(gpu, monkeypatch):
    from fpsg_amd import few_shot, metrics
    from fpsg_amd.engine import build_model, default_options
    from fpsg_amd.episodes import synthetic_episode
    torch.manual_seed(5)
    S, Q = 2, 1
    model = build_model(default_options(device="cuda", pc_dist="sinkhorn", intra_recon=True, n_shot=S,
                                        n_query=Q)).to(gpu).train()
    assert model.sinkhorn_blur == 0.05 and model.sinkhorn_diameter == FIXED
    calls = []
    inner = metrics.sinkhorn_loss

    def spy(p1, p2, **kw):
        calls.append((p1.detach().clone(), p2.detach().clone(), kw))
        return inner(p1, p2, **kw)

    monkeypatch.setattr(few_shot, "sinkhorn_loss", spy)
    ep = synthetic_episode(S, Q, n_pts=2048, img_size=96, seed=50, device=gpu)
    out = model.loss(ep)
    assert len(calls) == 1, "the query and support pairs go through ONE call (items are independent: fixed diameter)"
    syn, rf, kw = calls[0]
    assert syn.size(0) == Q + S and rf.size(0) == Q + S and kw == {"blur": 0.05, "diameter": FIXED}
    each = torch.cat([inner(syn[k:k + 1].contiguous(), rf[k:k + 1].contiguous(), **kw) for k in range(Q + S)])
    assert torch.equal(each, inner(syn, rf, **kw))                   # a pair's value does not depend on the batch
    want_q, want_s = float(each[:Q].double().sum()), float(each[Q:].double().sum())
    assert want_q > 0 and want_s > 0
    assert abs(float(out["query_rec_loss"].detach()) - want_q) <= 1e-6 * want_q
    assert abs(float(out["support_rec_loss"].detach()) - want_s) <= 1e-6 * want_s
    want = model.query_factor * want_q + model.support_factor * want_s
    assert abs(float(out["ttl_loss"].detach()) - want) <= 1e-6 * want
    out["ttl_loss"].sum().backward()
    nonzero = 0
    for part in (model.pc_decoder, model.img_encoder):
        params = [(n, p) for n, p in part.named_parameters() if p.requires_grad]
        assert params
        for n, p in params:
            assert p.grad is not None and bool(torch.isfinite(p.grad).all()), n
            nonzero += int(bool((p.grad != 0).any()))
    assert nonzero > 0


def test_train_step_captures_and_replays_the_sinkhorn_episode(gpu):
    """TrainStep(graph=True): two eager episodes, the capture, replays -- no host read in the loss, finite losses that
    the replays reproduce to within what a second eager run of the libraries' kernels gives."""
    from fpsg_amd.engine import TrainStep, build_model, build_optimizer, default_options
    from fpsg_amd.episodes import synthetic_episode
    torch.manual_seed(0)
    opt = default_options(device="cuda", pc_dist="sinkhorn", intra_recon=True, n_shot=2, n_query=1, lr=0.0)
    model = build_model(opt).to(gpu).train()
    optimizer, _ = build_optimizer(model, opt)
    step = TrainStep(model, optimizer, graph=True)
    eps = [synthetic_episode(2, 1, n_pts=2048, img_size=96, seed=s, device=gpu) for s in (3, 4)]
    losses = []
    for _ in range(4):                           # 2 eager uses, capture, replay
        losses += [float(o["ttl_loss"].sum()) for o in step(eps)]
    assert len(step._graphs) == 2                # one shape, the first (copy) / later (add) episode of a step
    assert all(math.isfinite(v) and v > 0 for v in losses), losses
    assert bool(torch.isfinite(step.buckets.flat).all()) and bool((step.buckets.flat != 0).any())


def test_training_entry_point_with_sinkhorn(gpu, tmp_path):
    env = dict(os.environ, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, "trainNetwork.py", "--synthetic", "--resident", "--n_shot", "2", "--n_query", "1",
                        "--intra_recon", "--pc_dist", "sinkhorn", "--epoch", "2", "--n_episode", "4",
                        "--model_path", str(tmp_path), "--name", "s"], cwd=ROOT, env=env, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("Training Results for Epoch")]
    assert len(lines) == 2, r.stdout[-3000:]
    for ln in lines:
        m = re.search(r"Query_rec: (\S+), Support_rec: (\S+)$", ln)
        assert m, ln
        for v in map(float, m.groups()):
            assert math.isfinite(v) and v > 0.0, ln
    classes = [ln for ln in r.stdout.splitlines() if ln.startswith("Class: ") and "Rec CD: " in ln]
    assert classes, r.stdout[-3000:]
    for ln in classes:
        assert math.isfinite(float(ln.split("Rec CD: ")[1].split()[0])), ln
    assert os.path.exists(os.path.join(str(tmp_path), "s", "model_epoch_2.pt"))
