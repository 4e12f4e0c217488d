"""The sliced Wasserstein distance on the GPU (K22): fpsg_swd behind ``metrics.swd`` / ``metrics.swd_loss``
against the numpy references of ``tests/_swd_ref.py`` -- the sort element for element, value and gradient within the
measured bounds, the exact cases, the bitwise invariances, non-finite input, autograd, descent, the model and graph
capture."""
import functools
import math

import numpy as np
import pytest
import torch

import _swd_ref as ref

pytestmark = pytest.mark.gpu

B = 3
SIZES = (1, 2, 3, 64, 65, 100, 257, 2048)     # one point; below / at / past a wave; no power of two; the largest
# both ends of every swd_kernel<P> the sizes above leave out or reach at one size only: <128> (65..128), <256>
# (129..256, never reached above), <512> (257..512) and <1024> (513..1024, never reached above)
SIZES += (128, 129, 256, 512, 513, 1024)
GROUP = 8                                     # directions per workgroup: L = 8 is one group, L = 9 two
N_DIRS = (1, 3, GROUP, GROUP + 1, 128)

# Largest deviations measured on an MI355X over SIZES x N_DIRS with the seeds below, times 4:
#   value against ref_keys32 (relative)                       measured 1.671e-7 (N = 3, L = 3)
#   gradient against ref_keys32 (over the gradient's max-abs) measured 2.085e-7 (N = 65, L = 128)
#   value against ref_f64 (relative)                          measured 6.340e-7 (N = 1, L = 1: one rounded key difference)
VALUE_K32_BOUND = 4 * 1.671e-7
GRAD_K32_BOUND = 4 * 2.085e-7
VALUE_F64_BOUND = 4 * 6.340e-7


def _call(x, y, dirs, gpu, need1=True, need2=True, matching=True):
    """One fpsg_swd call on numpy / torch inputs: ``(value, g1, g2, perm1, perm2)`` as torch CPU tensors (or None)."""
    from fpsg_amd.metrics import _swd_call
    t = [torch.as_tensor(a).to(gpu).contiguous() for a in (x, y, dirs)]
    out = _swd_call(t[0], t[1], t[2], need1, need2, matching)
    torch.cuda.synchronize()
    return tuple(None if o is None else o.cpu() for o in out)


@functools.lru_cache(maxsize=None)
def _case(N, L, gpu):
    """Inputs, the kernel's outputs and both references for one shape, computed once and shared."""
    x, y = ref.clouds(B, N, seed=1000 + N)
    dirs = ref.unit_directions(L, seed=2000 + L)
    got = _call(x, y, dirs, gpu)
    k32 = [ref.ref_keys32(x[b], y[b], dirs) for b in range(B)]
    f64 = [ref.value_f64(x[b], y[b], dirs) for b in range(B)]
    return x, y, dirs, got, k32, f64


def _assert_orders(got, want, what):
    _, _, _, m1, m2 = got
    for b, w in enumerate(want):
        assert np.array_equal(m1[b].numpy(), w[3]), (what, b, "perm1")
        assert np.array_equal(m2[b].numpy(), w[4]), (what, b, "perm2")


@pytest.mark.parametrize("N", SIZES)
def test_sort_is_the_references_order_element_for_element(gpu, N):
    for L in N_DIRS:
        x, y, dirs, got, k32, _ = _case(N, L, str(gpu))
        assert got[3].shape == (B, L, N) and got[3].dtype == torch.int32
        _assert_orders(got, k32, (N, L))


@pytest.mark.parametrize("N", [5, 64, 100, 257])
def test_sort_breaks_exact_ties_by_index(gpu, N):
    """Integer-lattice points under axis-aligned directions (a handful of distinct keys, -0 among them), and a cloud
    with duplicated points under generic directions."""
    rng = np.random.default_rng(N)
    x = rng.integers(-2, 3, size=(B, N, 3)).astype(np.float32)
    y = rng.integers(-2, 3, size=(B, N, 3)).astype(np.float32)
    axes = np.array([[1, 0, 0], [0, 1, 0], [0, 0, 1], [-1, 0, 0], [0, -1, 0], [0, 0, -1], [1, 1, 0], [0, 0, 0], [1, -1, 1]],
                    dtype=np.float32)
    got = _call(x, y, axes, gpu)
    want = [ref.ref_keys32(x[b], y[b], axes) for b in range(B)]
    _assert_orders(got, want, "lattice")
    for b in range(B):
        assert abs(float(got[0][b]) - want[b][0]) <= VALUE_K32_BOUND * max(want[b][0], 1e-30)
    a, c = ref.clouds(B, N, seed=77)
    a[:, N // 2:] = a[:, :N - N // 2]                                # every point of the first half once more
    c[:, 1::2] = c[:, 0:1]                                           # every other point a copy of point 0
    dirs = ref.unit_directions(GROUP + 1, seed=78)
    _assert_orders(_call(a, c, dirs, gpu), [ref.ref_keys32(a[b], c[b], dirs) for b in range(B)], "duplicates")


def _deviations(N, L, gpu):
    x, y, dirs, got, k32, f64 = _case(N, L, str(gpu))
    value, g1, g2 = got[0].double().numpy(), got[1].double().numpy(), got[2].double().numpy()
    ev = max(abs(value[b] - k32[b][0]) / k32[b][0] for b in range(B))
    eg = max(np.abs(g - k32[b][i]).max() / np.abs(k32[b][i]).max() for b in range(B) for g, i in ((g1[b], 1), (g2[b], 2)))
    ef = max(abs(value[b] - f64[b]) / f64[b] for b in range(B))
    return ev, eg, ef


@pytest.mark.parametrize("N", SIZES)
def test_value_and_gradient_against_the_fp32_key_reference(gpu, N):
    """The orders agree exactly (above), so what remains is fp32 arithmetic and summation against float64."""
    for L in N_DIRS:
        ev, eg, _ = _deviations(N, L, gpu)
        print(f"swd N={N} L={L}: value vs keys32 {ev:.3e}, gradient vs keys32 {eg:.3e}")
        assert ev <= VALUE_K32_BOUND, (N, L, ev)
        assert eg <= GRAD_K32_BOUND, (N, L, eg)


@pytest.mark.parametrize("N", SIZES)
def test_value_against_float64_keys(gpu, N):
    """The gradient is not compared here: a near-tie legitimately swaps two rows."""
    for L in N_DIRS:
        _, _, ef = _deviations(N, L, gpu)
        print(f"swd N={N} L={L}: value vs float64 {ef:.3e}")
        assert ef <= VALUE_F64_BOUND, (N, L, ef)


@pytest.mark.parametrize("N,L", [(1, 3), (100, GROUP + 1), (2048, GROUP)])
def test_a_cloud_against_itself_is_exactly_zero(gpu, N, L):
    x, _ = ref.clouds(B, N, seed=5)
    value, g1, g2, m1, m2 = _call(x, x.copy(), ref.unit_directions(L, seed=6), gpu)
    assert not value.any() and not g1.any() and not g2.any() and torch.equal(m1, m2)


def test_one_point_per_cloud(gpu):
    x, y = ref.clouds(B, 1, seed=8)
    dirs = ref.unit_directions(GROUP + 1, seed=9)
    value, g1, g2, m1, m2 = _call(x, y, dirs, gpu)
    assert not m1.any() and not m2.any()
    for b in range(B):
        want = ref.ref_keys32(x[b], y[b], dirs)
        assert abs(float(value[b]) - want[0]) <= VALUE_K32_BOUND * want[0]
        assert np.abs(g1[b].double().numpy() - want[1]).max() <= GRAD_K32_BOUND * np.abs(want[1]).max()
        assert torch.equal(g1[b], -g2[b])


@pytest.mark.parametrize("N,L", [(257, GROUP + 1), (2048, 3)])
def test_bitwise_invariances(gpu, N, L):
    x, y, dirs, whole, _, _ = _case(N, L, str(gpu))
    # two runs
    again = _call(x, y, dirs, gpu)
    for a, b in zip(whole, again):
        assert torch.equal(a, b)
    # a pair alone and inside the batch of three
    for b in range(B):
        alone = _call(x[b:b + 1], y[b:b + 1], dirs, gpu)
        for a, w in zip(alone, whole):
            assert torch.equal(a[0], w[b]), b
    # either gradient pointer NULL, no matchings asked for: the other outputs keep their bits
    v, g1, g2, m1, m2 = _call(x, y, dirs, gpu, need1=True, need2=False, matching=False)
    assert g2 is None and m1 is None and torch.equal(v, whole[0]) and torch.equal(g1, whole[1])
    v, g1, g2, _, _ = _call(x, y, dirs, gpu, need1=False, need2=True, matching=False)
    assert g1 is None and torch.equal(v, whole[0]) and torch.equal(g2, whole[2])
    v, g1, g2, _, m2 = _call(x, y, dirs, gpu, need1=False, need2=False, matching=True)
    assert g1 is None and g2 is None and torch.equal(v, whole[0]) and torch.equal(m2, whole[4])
    # the points of y permuted: the same value; generic clouds have no tied keys, so gy's rows move with the points
    assert all(len(np.unique(row)) == N for b in range(B) for row in ref.keys32(y[b], dirs)), "this input must be tie-free"
    sigma = np.random.default_rng(3).permutation(N)
    v, g1, g2, _, m2 = _call(x, y[:, sigma].copy(), dirs, gpu)
    assert torch.equal(v, whole[0]) and torch.equal(g1, whole[1])
    assert torch.equal(g2, whole[2][:, torch.as_tensor(sigma)])
    assert torch.equal(torch.as_tensor(sigma)[m2.long()], whole[4].long())


@pytest.mark.parametrize("N", [100, 2048])
def test_a_nan_coordinate_stays_in_its_pair(gpu, N):
    x, y, dirs, whole, _, _ = _case(N, GROUP + 1, str(gpu))
    bad = x.copy()
    bad[1, N // 3, 1] = np.nan
    value, g1, g2, m1, m2 = _call(bad, y, dirs, gpu)
    assert not math.isfinite(float(value[1]))
    for b in (0, 2):
        for got, want in zip((value, g1, g2, m1, m2), whole):
            assert torch.equal(got[b], want[b]), b
    # the matchings of the poisoned pair are still permutations: no sentinel came through
    assert torch.equal(m1[1].sort(dim=1).values, torch.arange(N, dtype=torch.int32).expand(dirs.shape[0], N))
    assert torch.equal(m2[1], whole[4][1])


def test_autograd_plumbing(gpu):
    from fpsg_amd.metrics import swd, swd_loss
    x, y, dirs, whole, _, _ = _case(257, GROUP + 1, str(gpu))
    xs, ys, d = (torch.as_tensor(a).to(gpu) for a in (x, y, dirs))
    w = torch.tensor([1.0, 0.5, 2.0], device=gpu)
    a, b = xs.clone().requires_grad_(), ys.clone().requires_grad_()
    out = swd_loss(a, b, d)
    out.sum().backward()
    assert torch.equal(out.detach().cpu(), whole[0])
    assert torch.equal(a.grad.cpu(), whole[1]) and torch.equal(b.grad.cpu(), whole[2])
    a2, b2 = xs.clone().requires_grad_(), ys.clone().requires_grad_()
    (swd_loss(a2, b2, d) * w).sum().backward()
    assert torch.equal(a2.grad, a.grad * w[:, None, None]) and torch.equal(b2.grad, b.grad * w[:, None, None])
    # an input that needs no gradient gets none, and the other's keeps its bits
    p1, p2 = xs.clone().requires_grad_(), ys.clone()
    swd_loss(p1, p2, d).sum().backward()
    assert p2.grad is None and torch.equal(p1.grad, a.grad)
    q1, q2 = xs.clone(), ys.clone().requires_grad_()
    swd_loss(q1, q2, d).sum().backward()
    assert q1.grad is None and torch.equal(q2.grad, b.grad)
    plain = swd_loss(xs, ys, d)
    assert plain.grad_fn is None and torch.equal(plain.cpu(), whole[0])
    # the metric form: no grad, the same bits, the matchings on request, the lattice by default
    metric = swd(xs.clone().requires_grad_(), ys, directions=d)
    assert metric.grad_fn is None and torch.equal(metric.cpu(), whole[0])
    v, m1, m2 = swd(xs, ys, directions=d, return_matching=True)
    assert torch.equal(m1.cpu(), whole[3]) and torch.equal(m2.cpu(), whole[4]) and torch.equal(v.cpu(), whole[0])
    from fpsg_amd.metrics import swd_directions
    assert torch.equal(swd(xs, ys, n_proj=16), swd(xs, ys, directions=swd_directions(16, gpu)))


def test_descent_moves_a_cloud_onto_its_target(gpu):
    """N = 256, L = 64, the fixed lattice; ten steps x -= 0.5 (3 N / 2) grad.  In float64 the recipe ends at 0.005-0.009
    of the starting value over three seeds."""
    from fpsg_amd.metrics import swd, swd_directions, swd_loss
    N, L = 256, 64
    g = torch.Generator().manual_seed(0)
    x = torch.randn((B, N, 3), generator=g)
    x = x / x.norm(dim=2).amax(dim=1)[:, None, None]
    y = torch.randn((B, N, 3), generator=g)
    y = 0.7 * (y / y.norm(dim=2).amax(dim=1)[:, None, None]) + 0.1
    x, y, dirs = x.to(gpu).contiguous(), y.to(gpu).contiguous(), swd_directions(L, gpu)
    first = swd(x, y, directions=dirs)
    for _ in range(10):
        p = x.clone().requires_grad_()
        swd_loss(p, y, dirs).sum().backward()
        x = (x - 0.5 * (3 * N / 2) * p.grad).contiguous()
    last = swd(x, y, directions=dirs)
    print("swd descent ratios:", (last / first).tolist())
    assert bool((first > 0).all()) and bool((last >= 0).all())
    assert bool((last <= 0.05 * first).all()), (last / first).tolist()


def test_forward_and_backward_survive_a_graph_replay(gpu):
    """The call only enqueues.  Captured after two eager calls, replayed on two other inputs copied into the static
    buffers: the eager bits."""
    from fpsg_amd.metrics import swd_loss
    N, L = 257, GROUP + 1
    w = torch.tensor([1.0, 0.5, 2.0], device=gpu)
    dirs = torch.as_tensor(ref.unit_directions(L, seed=31)).to(gpu)
    inputs = [tuple(torch.as_tensor(a).to(gpu) for a in ref.clouds(B, N, seed=s)) for s in (21, 22, 23)]

    def run(a, b):
        out = swd_loss(a, b, dirs)
        return (out,) + torch.autograd.grad((out * w).sum(), [a, b])

    eager = [run(x.clone().requires_grad_(), y.clone().requires_grad_()) for x, y in inputs]
    a = inputs[0][0].clone().requires_grad_()
    b = inputs[0][1].clone().requires_grad_()
    side = torch.cuda.Stream(device=gpu)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run(a, b)
        run(a, b)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        static = run(a, b)
    for k in (1, 2):
        with torch.no_grad():
            a.copy_(inputs[k][0])
            b.copy_(inputs[k][1])
        g.replay()
        torch.cuda.synchronize()
        for got, want in zip(static, eager[k]):
            assert torch.equal(got.detach(), want.detach()), k


# ---- the training path ---------------------------------------------------------------------------------------------

def _tiny_model(gpu, directions, S=2, Q=1, **kw):
    from fpsg_amd.engine import build_model, default_options
    opt = default_options(device="cuda", pc_dist="swd", swd_directions=directions, intra_recon=True, n_shot=S, n_query=Q,
                          **kw)
    return opt, build_model(opt).to(gpu).train()


def test_episode_losses_are_the_sums_of_swd_loss_over_the_decoded_pairs(gpu, monkeypatch):
    from fpsg_amd import few_shot, metrics
    from fpsg_amd.episodes import synthetic_episode
    torch.manual_seed(5)
    S, Q = 2, 1
    _, model = _tiny_model(gpu, "fixed", S, Q)
    assert model.swd_n_proj == 64 and model.swd_directions == "fixed"
    calls = []
    inner = metrics.swd_loss

    def spy(p1, p2, dirs):
        calls.append((p1.detach().clone(), p2.detach().clone(), dirs))
        return inner(p1, p2, dirs)

    monkeypatch.setattr(few_shot, "swd_loss", spy)
    ep = synthetic_episode(S, Q, n_pts=2048, img_size=96, seed=50, device=gpu)
    out = model.loss(ep)
    assert len(calls) == 1, "the query and support pairs go through ONE call"
    syn, rf, dirs = calls[0]
    assert syn.size(0) == Q + S and rf.size(0) == Q + S
    assert torch.equal(dirs, metrics.swd_directions(64, gpu)) and dirs is model._swd_lattice[syn.device]
    each = torch.cat([inner(syn[k:k + 1].contiguous(), rf[k:k + 1].contiguous(), dirs) for k in range(Q + S)])
    assert torch.equal(each, inner(syn, rf, dirs))                   # a pair's value does not depend on the batch
    want_q, want_s = float(each[:Q].double().sum()), float(each[Q:].double().sum())
    assert want_q > 0 and want_s > 0
    assert abs(float(out["query_rec_loss"].detach()) - want_q) <= 1e-6 * want_q
    assert abs(float(out["support_rec_loss"].detach()) - want_s) <= 1e-6 * want_s
    want = model.query_factor * want_q + model.support_factor * want_s
    assert abs(float(out["ttl_loss"].detach()) - want) <= 1e-6 * want
    out["ttl_loss"].sum().backward()
    for n, p in model.named_parameters():
        if p.requires_grad:
            assert p.grad is not None and bool(torch.isfinite(p.grad).all()), n
    assert any(bool((p.grad != 0).any()) for p in model.pc_decoder.parameters())
    # "random": fresh unit vectors per loss call
    _, rnd = _tiny_model(gpu, "random", S, Q, swd_n_proj=5)
    calls.clear()
    rnd.loss(ep), rnd.loss(ep)
    assert len(calls) == 2 and calls[0][2].shape == (5, 3) and not torch.equal(calls[0][2], calls[1][2])
    assert float((calls[0][2].norm(dim=1) - 1).abs().max()) <= 1e-6


def _train_losses(gpu, directions, rounds, seed_every_round):
    from fpsg_amd.engine import TrainStep, build_optimizer
    from fpsg_amd.episodes import synthetic_episode
    torch.manual_seed(0)
    opt, model = _tiny_model(gpu, directions, lr=0.0)
    optimizer, _ = build_optimizer(model, opt)
    step = TrainStep(model, optimizer, graph=True)
    eps = [synthetic_episode(2, 1, n_pts=2048, img_size=96, seed=s, device=gpu) for s in (3, 4)]
    losses = []
    for _ in range(rounds):                      # 2 eager uses, capture, replays
        if seed_every_round:                     # the decoder draws its patches' 2-D grids per forward: the same draws
            torch.manual_seed(1234)
        losses.append([float(o["ttl_loss"].sum()) for o in step(eps)])
    assert len(step._graphs) == 2
    assert bool(torch.isfinite(step.buckets.flat).all()) and bool((step.buckets.flat != 0).any())
    return losses


def test_train_step_replays_the_fixed_lattice_episode_bit_for_bit(gpu):
    """TrainStep(graph=True) at lr = 0 and the generator re-seeded before every round: the weights stay and the decoder
    draws the same grids, so every round sees the same two episodes; the replays (a captured generator continues from the
    current seed and offset) give the second eager round's losses bit for bit -- no host read and no hidden state in the
    loss."""
    losses = _train_losses(gpu, "fixed", 4, True)
    print("swd fixed-lattice losses per round:", losses)
    assert all(math.isfinite(v) and v > 0 for r in losses for v in r), losses
    assert losses[2] == losses[1] and losses[3] == losses[1], losses


def test_train_step_replays_random_directions_with_fresh_draws(gpu):
    """torch captures its generator's state with the graph and advances it per replay: two replays draw different
    directions (and decoder grids), so their losses differ.  The second half isolates the directions: the model's metric
    alone, captured on fixed clouds, gives another value on every replay, all close to the lattice's."""
    from fpsg_amd.metrics import swd, swd_directions
    losses = _train_losses(gpu, "random", 5, False)
    print("swd random-direction losses per round:", losses)
    assert all(math.isfinite(v) and v > 0 for r in losses for v in r), losses
    assert losses[3] != losses[4] and losses[2] != losses[3], losses
    _, model = _tiny_model(gpu, "random", swd_n_proj=64)
    a, b = (torch.as_tensor(t).to(gpu) for t in ref.clouds(B, 257, seed=41))
    side = torch.cuda.Stream(device=gpu)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        model._swd_metric(a, b)
        model._swd_metric(a, b)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        static = model._swd_metric(a, b)
    seen = []
    for _ in range(3):
        g.replay()
        torch.cuda.synchronize()
        seen.append(static.clone())
    assert not torch.equal(seen[0], seen[1]) and not torch.equal(seen[1], seen[2]) and not torch.equal(seen[0], seen[2])
    lattice = swd(a, b, directions=swd_directions(1024, gpu))
    for v in seen:                               # 64 random unit vectors estimate the same integral over the sphere
        assert bool(((v - lattice).abs() <= 0.5 * lattice).all()), (v.tolist(), lattice.tolist())
