"""The weight average inside the flat Adam step (K23; arithmetic in include/fpsg_hip.h): the ``_ema`` entries
leave parameters and moments as the entries without a shadow leave them, bit for bit; the shadow against the float64
recurrence and in two exact cases; ``fpsg_flat_swap``; ``FlatAdam.attach_ema`` on every gradient path, ``TrainStep`` with
graph replay, the model evaluated inside ``swapped()``, and ``trainNetwork.py --ema_decay`` + ``evaluate_Network.py``."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn as nn

from conftest import ROOT

pytestmark = pytest.mark.gpu

# the scalar tail alone, one vector, one full workgroup of 256 vectors and its neighbours, several workgroups + a tail
SIZES = (1, 2, 3, 4, 5, 7, 1023, 1024, 1025, 4 * 256 + 1, 4 * 256 * 3 + 2)
HYPER = (2e-3, 0.9, 0.999, 1e-8)


@pytest.fixture(scope="module")
def lib():
    from fpsg_amd import _hip
    return _hip.load()


def _tables(n):
    """Segment layouts ``(lengths, index of the NULL segment or None, index of the misaligned one or None)`` for n
    elements: ``nseg = 1``; boundaries inside a vector; a NULL segment; a gradient that starts off a 16-byte boundary."""
    out = [((n,), None, None)]
    if n >= 2:
        out.append(((1, n - 1), 0, None))
    if n >= 7:
        out.append(((1, 2, 3, n - 6), 2, 3))                       # boundaries at 1, 3, 6: inside the first two vectors
    if n >= 1025:
        out.append(((5, 1017, n - 1022), 1, 2))                    # a boundary inside vector 255 and a long NULL segment
    return out


def _segments(gpu, lengths, null_at, misaligned_at, seed):
    g = torch.Generator(device=gpu).manual_seed(seed)
    tensors, ptrs = [], []
    for k, ln in enumerate(lengths):
        if k == null_at:
            tensors.append(None)
            ptrs.append(0)
            continue
        if k == misaligned_at:
            t = torch.randn(ln + 8, device=gpu, generator=g)[1:1 + ln]
            assert t.data_ptr() % 16 == 4
        else:
            t = torch.randn(ln, device=gpu, generator=g)
        tensors.append(t)
        ptrs.append(t.data_ptr())
    off = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    table = torch.tensor(ptrs, dtype=torch.int64, device=gpu)
    flat = torch.cat([torch.zeros(ln, device=gpu) if t is None else t for t, ln in zip(tensors, lengths)])
    return tensors, table, torch.from_numpy(off).to(gpu), flat


def _state(gpu, n, seed):
    gen = torch.Generator(device=gpu).manual_seed(seed)
    p = torch.randn(n, device=gpu, generator=gen)
    m = torch.randn(n, device=gpu, generator=gen) * 0.05
    v = torch.rand(n, device=gpu, generator=gen) * 0.01
    e = p + torch.randn(n, device=gpu, generator=gen) * 0.1
    return p, m, v, e


def _flat_ema(lib, p, g, m, v, e, step, scale, scale_dev, w, hyper=HYPER):
    from fpsg_amd import _hip
    rc = lib.fpsg_adam_step_ema(_hip.ptr(p), _hip.ptr(g), _hip.ptr(m), _hip.ptr(v), _hip.ptr(e), p.numel(), *hyper, step,
                                scale, scale_dev, w, None)
    assert rc == 0, lib.fpsg_last_error()


def _seg_ema(lib, p, table, seg_off, m, v, e, step, scale, scale_dev, w, hyper=HYPER):
    from fpsg_amd import _hip
    rc = lib.fpsg_adam_step_segments_ema(_hip.ptr(p), _hip.ptr(table), _hip.ptr(seg_off), table.numel(), _hip.ptr(m),
                                         _hip.ptr(v), _hip.ptr(e), p.numel(), *hyper, step, scale, scale_dev, w, None)
    assert rc == 0, lib.fpsg_last_error()


# ---- 1. parameters and moments: the bits of the entries without a shadow ------------------------------------------------

@pytest.mark.parametrize("n", SIZES)
def test_parameters_and_moments_equal_the_existing_entries_bit_for_bit(gpu, lib, n):
    from fpsg_amd import _hip
    step, scale, w = 3, 0.3, 0.25
    p0, m0, v0, e0 = _state(gpu, n, seed=n)
    dev_scale = torch.tensor([-9.0, scale], device=gpu)              # read from out2 + 1, as FlatAdam does
    dev = _hip.ptr(dev_scale) + 4
    for lengths, null_at, mis_at in _tables(n):
        _, table, seg_off, flat = _segments(gpu, lengths, null_at, mis_at, seed=7 * n + len(lengths))

        def run(call):
            p, m, v, e = p0.clone(), m0.clone(), v0.clone(), e0.clone()
            call(p, m, v, e)
            return p, m, v, e

        def old(entry, *front, last):
            def call(p, m, v, e):
                rc = entry(_hip.ptr(p), *front, _hip.ptr(m), _hip.ptr(v), n, *HYPER, step, last, None)
                assert rc == 0, lib.fpsg_last_error()
            return run(call)

        seg_front = (_hip.ptr(table), _hip.ptr(seg_off), table.numel())
        want = old(lib.fpsg_adam_step, _hip.ptr(flat), last=scale)
        for other in (old(lib.fpsg_adam_step_dscale, _hip.ptr(flat), last=dev),
                      old(lib.fpsg_adam_step_segments, *seg_front, last=scale),
                      old(lib.fpsg_adam_step_segments_dscale, *seg_front, last=dev)):
            assert all(torch.equal(a, b) for a, b in zip(want[:3], other[:3]))
        assert not torch.equal(want[0], p0) and torch.equal(want[3], e0)
        got = [run(lambda p, m, v, e: _flat_ema(lib, p, flat, m, v, e, step, scale, None, w)),
               run(lambda p, m, v, e: _flat_ema(lib, p, flat, m, v, e, step, -77.0, dev, w)),     # grad_scale is ignored
               run(lambda p, m, v, e: _seg_ema(lib, p, table, seg_off, m, v, e, step, scale, None, w)),
               run(lambda p, m, v, e: _seg_ema(lib, p, table, seg_off, m, v, e, step, -77.0, dev, w))]
        for k, g in enumerate(got):
            for name, a, b in zip(("param", "exp_avg", "exp_avg_sq"), want, g):
                assert torch.equal(a, b), (n, lengths, k, name)
            assert torch.equal(g[3], got[0][3]), (n, lengths, k)          # one shadow, whichever form made it
        # the shadow moved towards the new parameters by about w of the way (the exact rounding is checked below)
        e1 = got[0][3].double()
        ideal = e0.double() + w * (want[0].double() - e0.double())
        assert bool(((e1 - ideal).abs() <= 2.0 ** -22 * torch.maximum(want[0].abs(), e0.abs()).double()).all())
        assert not torch.equal(got[0][3], e0)


# ---- 2. the shadow ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("form", ["flat", "segments"])
@pytest.mark.parametrize("decay", [0.5, 0.9, 0.9999])
def test_shadow_follows_the_float64_recurrence(gpu, lib, decay, form):
    """T = 12 steps with fresh random gradients; e against e64 <- e64 + w_t (p_t - e64) in float64, driven by the kernel's
    own fp32 p_t after each step and the same fp32 w_t.  One step's rounding is at most 2 * 2^-24 * max(|p|, |e|) (one
    rounding of p - e, one of the fma) and each step multiplies the earlier error by d_t < 1, so
    |e - e64| <= 4 * min(T, 1 / (1 - decay)) * 2^-24 * max(|p|, |e|) -- derived, not measured."""
    from fpsg_amd.ema import weight_at
    T, n = 12, 4 * 256 * 3 + 2
    p, m, v, _ = _state(gpu, n, seed=11)
    e = p.clone()                                                     # the shadow starts as a copy of the parameters
    e64 = e.double()
    for t in range(1, T + 1):
        w = weight_at(decay, t)
        lengths, null_at, mis_at = _tables(n)[2 + t % 2]
        _, table, seg_off, flat = _segments(gpu, lengths, null_at, mis_at, seed=100 * t)
        if form == "flat":
            _flat_ema(lib, p, flat, m, v, e, t, 1.0, None, w)
        else:
            _seg_ema(lib, p, table, seg_off, m, v, e, t, 1.0, None, w)
        e64 = e64 + w * (p.double() - e64)
    bound = 4 * min(T, 1 / (1 - decay)) * 2.0 ** -24
    size = torch.maximum(p.abs(), e.abs()).double()
    err = (e.double() - e64).abs()
    print(f"decay {decay} {form}: max |e - e64| / (2^-24 max(|p|, |e|)) = {float((err / size).max()) * 2 ** 24:.3f}, "
          f"bound {bound * 2 ** 24:.1f}")
    assert bool((err <= bound * size).all())
    assert float((e - p).abs().max()) > 0                             # the average lags the weights


@pytest.mark.parametrize("form", ["flat", "segments"])
@pytest.mark.parametrize("n", [7, 1025])
def test_exact_cases(gpu, lib, form, n):
    from fpsg_amd.ema import weight_at
    hyper0 = (0.0,) + HYPER[1:]                                       # lr = 0: the parameters stay
    lengths, null_at, mis_at = _tables(n)[-1]
    _, table, seg_off, flat = _segments(gpu, lengths, null_at, mis_at, seed=n)

    def step(p, m, v, e, t, w):
        if form == "flat":
            _flat_ema(lib, p, flat, m, v, e, t, 1.0, None, w, hyper0)
        else:
            _seg_ema(lib, p, table, seg_off, m, v, e, t, 1.0, None, w, hyper0)

    # p - e = 0: the shadow stays equal to the parameters bit for bit
    p, m, v, _ = _state(gpu, n, seed=3)
    p0, e = p.clone(), p.clone()
    for t in range(1, 21):
        step(p, m, v, e, t, weight_at(0.999, t))
        assert torch.equal(p, p0) and torch.equal(e, p0), t
    assert not torch.equal(m, _state(gpu, n, seed=3)[1])              # (the moments did move)
    # e = 0, p = 1, w = 0.5: e = 1 - 2^-k exactly
    p, m, v, e = torch.ones(n, device=gpu), torch.zeros(n, device=gpu), torch.zeros(n, device=gpu), torch.zeros(n, device=gpu)
    for k in range(1, 21):
        step(p, m, v, e, k, 0.5)
        assert torch.equal(e, torch.full((n,), 1.0 - 2.0 ** -k, device=gpu)), k
    assert torch.equal(p, torch.ones(n, device=gpu))


# ---- 3. the swap -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [1, 5, 1025])
def test_flat_swap_exchanges_and_restores_every_bit(gpu, lib, n):
    from fpsg_amd import _hip
    gen = torch.Generator(device=gpu).manual_seed(n)
    # guard elements behind both buffers (n rounded up to whole vectors, so that b stays 16-byte aligned)
    pad = -(-n // 4) * 4 + 4
    store = torch.randn(2 * pad, device=gpu, generator=gen)
    store[5 % n] = float("nan")                                        # bits, not values: a NaN travels too
    a, b = store[:n], store[pad:pad + n]
    before = store.clone()
    bits = store.view(torch.int32)
    assert lib.fpsg_flat_swap(_hip.ptr(a), _hip.ptr(b), n, None) == 0, lib.fpsg_last_error()
    want = before.clone()
    want[:n], want[pad:pad + n] = before[pad:pad + n], before[:n]
    assert torch.equal(bits, want.view(torch.int32))                   # exchanged, and nothing outside them touched
    assert lib.fpsg_flat_swap(_hip.ptr(a), _hip.ptr(b), n, None) == 0, lib.fpsg_last_error()
    assert torch.equal(bits, before.view(torch.int32))


# ---- 4. FlatAdam ---------------------------------------------------------------------------------------------------------------

class _Odd(nn.Module):
    """Parameter counts 37, 1, 5 * 7, 1023 and 3 (frozen); no matrix product, so every launch is reproducible."""

    def __init__(self):
        super().__init__()
        g = torch.Generator().manual_seed(4)
        self.a = nn.Parameter(torch.randn(37, generator=g))
        self.b = nn.Parameter(torch.randn(1, generator=g))
        self.c = nn.Parameter(torch.randn(5, 7, generator=g))
        self.d = nn.Parameter(torch.randn(1023, generator=g))
        self.frozen = nn.Parameter(torch.randn(3, generator=g), requires_grad=False)

    def forward(self, x):                                              # x [B, 37]
        h = torch.tanh(x * self.a + self.b)
        return h.sum(1, keepdim=True) * self.c.reshape(1, -1) + self.d[:35].reshape(1, -1) * self.d[35:70] + self.d.mean() \
            + self.frozen.sum()

    def loss(self, sample):
        l = (self(sample["xs"]) - sample["pcs"]).square().mean()
        return {"ttl_loss": l, "recon_loss": l, "query_rec_loss": l, "support_rec_loss": l * 0}


def _odd_sample(gpu, k):
    g = torch.Generator(device=gpu).manual_seed(30 + k)
    x = torch.randn(9, 37, device=gpu, generator=g)
    y = torch.randn(9, 35, device=gpu, generator=g)
    z = torch.zeros(1, device=gpu)
    return {"xs": x, "pcs": y, "xq": z, "xad": z, "pcq": z, "pcad": z}


@pytest.mark.parametrize("path", ["table", "flat"])
@pytest.mark.parametrize("max_norm", [None, 1.0])
def test_attached_average_changes_no_bit_of_the_step(gpu, path, max_norm):
    """An optimizer with an attached average against its twin without one, the same gradients, 5 steps: ``flat_param`` and
    both moments stay equal bit for bit; the shadow follows the recurrence (the bound of the kernel test).  The gradients
    are 1096 normal values times 10 (odd steps: a norm of hundreds) or times 0.01 (even steps: about 0.33 times the
    step's grad_scale), so a threshold of 1 clips the odd steps and leaves the even ones."""
    from fpsg_amd.ema import WeightEma, weight_at
    from fpsg_amd.optim import FlatAdam
    decay, T = 0.9, 5
    a, b = _Odd().to(gpu), _Odd().to(gpu)
    opt_a = FlatAdam(a.parameters(), lr=2e-3, max_grad_norm=max_norm)
    opt_b = FlatAdam(b.parameters(), lr=2e-3, max_grad_norm=max_norm)
    ema = WeightEma(a.parameters(), decay)
    opt_a.attach_ema(ema)
    assert opt_a.ema is ema and ema.fused and opt_b.ema is None and opt_b.flat_ema is None
    assert opt_a.flat_ema.shape == opt_a.flat_param.shape == (37 + 1 + 35 + 1023,) and torch.equal(opt_a.flat_ema, opt_a.flat_param)
    for (p, off, cnt), e in zip(opt_a._layout, ema.shadow):           # per-parameter views, as the moments'
        assert e.shape == p.shape and e.data_ptr() == opt_a.flat_ema.data_ptr() + 4 * off
    with pytest.raises(RuntimeError, match="FlatAdam"):
        ema.update()
    flats = {}
    if path == "flat":
        for opt in (opt_a, opt_b):
            flats[opt] = torch.zeros_like(opt.flat_param)
            opt.bind_gradients(flats[opt])
    gen = torch.Generator(device=gpu).manual_seed(8)
    e64 = opt_a.flat_ema.double()
    for t in range(1, T + 1):
        grads = [torch.randn(p.shape, device=gpu, generator=gen) * (10.0 if t % 2 else 0.01) for p, _, _ in opt_a._layout]
        opt_a.grad_scale = opt_b.grad_scale = (1.0, 1.0 / 3, 0.5, 1.0, 0.25)[t - 1]
        for opt in (opt_a, opt_b):
            for (p, off, cnt), g in zip(opt._layout, grads):
                if path == "flat":
                    flats[opt][off:off + cnt].copy_(g.reshape(-1))
                    p.grad = flats[opt][off:off + cnt].view(p.shape)
                else:
                    p.grad = g.clone()
            if path == "flat":
                assert opt._bound_gradient() is flats[opt]
            else:
                assert opt._bound_gradient() is None and opt._pointer_table() is not None
            opt.step()
        assert ema.updates == t
        assert torch.equal(opt_a.flat_param, opt_b.flat_param), (path, t)
        assert torch.equal(opt_a.flat_exp_avg, opt_b.flat_exp_avg) and torch.equal(opt_a.flat_exp_avg_sq, opt_b.flat_exp_avg_sq)
        e64 = e64 + weight_at(decay, t) * (opt_a.flat_param.double() - e64)
    if max_norm is not None:
        sa, sb = opt_a.clip_stats(), opt_b.clip_stats()
        assert sa == sb and sa["steps"] == T and 0 < sa["clipped"] < T          # some steps clip and some do not
    size = torch.maximum(opt_a.flat_param.abs(), opt_a.flat_ema.abs()).double()
    assert bool(((opt_a.flat_ema.double() - e64).abs() <= 4 * min(T, 1 / (1 - decay)) * 2.0 ** -24 * size).all())
    assert torch.equal(a.frozen, b.frozen) and not torch.equal(opt_a.flat_ema, opt_a.flat_param)
    # the state dict goes into another optimizer's flat buffer
    sd = ema.state_dict()
    assert sd["updates"] == T and all(torch.equal(sd["shadow"][i], e) for i, e in enumerate(ema.shadow))
    other = WeightEma(b.parameters(), decay)
    opt_b.attach_ema(other)
    other.load_state_dict(sd)
    assert other.updates == T and torch.equal(opt_b.flat_ema, opt_a.flat_ema)
    # swapped(): the flat buffers exchange their contents, the views stay where they are
    raw, avg = opt_a.flat_param.clone(), opt_a.flat_ema.clone()
    with ema.swapped():
        assert torch.equal(opt_a.flat_param, avg) and torch.equal(opt_a.flat_ema, raw)
        assert torch.equal(a.d.detach().reshape(-1), avg[opt_a._layout[0][1]:opt_a._layout[0][1] + 1023])
    assert torch.equal(opt_a.flat_param, raw) and torch.equal(opt_a.flat_ema, avg)


@pytest.mark.parametrize("count", [1, 2])
def test_train_step_with_graph_replay_gives_the_eager_shadow(gpu, count):
    """count = 1: the pointer-table path; count = 2: the flat gradient buffer with the folded 1/E.  Five steps: two eager
    runs per shape, the capture, two replays."""
    from fpsg_amd.engine import TrainStep, build_optimizer, default_options
    from fpsg_amd.optim import FlatAdam
    runs = []
    for graph in (False, True):
        model = _Odd().to(gpu).train()
        optimizer, _ = build_optimizer(model, default_options(device="cuda", lr=2e-3, ema_decay=0.9, clip_grad_norm=0.5))
        assert isinstance(optimizer, FlatAdam) and optimizer.ema.fused
        step = TrainStep(model, optimizer, graph=graph)
        for t in range(5):
            step([_odd_sample(gpu, 2 * t + k) for k in range(count)], n_episodes_global=count)
        assert len(step._graphs) == (count if graph else 0) and optimizer.ema.updates == 5
        runs.append((optimizer.flat_param.clone(), optimizer.flat_ema.clone()))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    assert not torch.equal(runs[0][0], runs[0][1])


# ---- 5. the model on the averaged weights ----------------------------------------------------------------------------------------

def test_evaluation_inside_swapped_and_after_it(gpu):
    from fpsg_amd import winograd
    from fpsg_amd.engine import TrainStep, build_model, build_optimizer, default_options
    from fpsg_amd.episodes import synthetic_episode
    torch.manual_seed(0)
    opt = default_options(device="cuda", intra_recon=True, ema_decay=0.9)
    model = build_model(opt).to(gpu).train()
    optimizer, _ = build_optimizer(model, opt)
    ema = optimizer.ema
    step = TrainStep(model, optimizer)
    for k in range(2):
        step([synthetic_episode(2, 1, n_pts=2048, img_size=64, seed=3 + k, device=gpu)])
    assert ema.updates == 2
    item = synthetic_episode(2, 1, n_pts=2048, img_size=64, seed=9, device=gpu)
    buffers = {k: v.clone() for k, v in model.named_buffers()}
    model.eval()

    def outputs():
        torch.manual_seed(5)                                           # the decoder draws its patch grids
        with torch.no_grad(), winograd.weights_frozen():
            return model.reconstruct(item).clone(), model.loss(item)["query_rec_loss"].clone()

    before = outputs()
    assert all(torch.equal(a, b) for a, b in zip(before, outputs()))   # the forward itself is reproducible
    with winograd.weights_frozen():
        with pytest.raises(RuntimeError, match="weights_frozen"):
            with ema.swapped():
                pass
    with ema.swapped():
        inside = outputs()
        state = {k: v.clone() for k, v in model.state_dict().items()}
    after = outputs()
    assert not torch.equal(inside[0], before[0]) and not torch.equal(inside[1], before[1])
    assert torch.equal(after[0], before[0]) and torch.equal(after[1], before[1])       # no cache leaked across the swap
    assert bool(torch.isfinite(inside[0]).all())
    # the state dict taken inside the swap: averaged parameters, live buffers
    live = model.state_dict()
    assert list(state) == list(live)
    assert all(torch.equal(state[k], buffers[k]) and torch.equal(live[k], buffers[k]) for k in buffers)
    assert any(not torch.equal(state[k], live[k]) for k in state)


# ---- 6. the entry points ---------------------------------------------------------------------------------------------------------

def test_training_then_evaluation_of_the_averaged_weights(gpu, tmp_path):
    env = dict(os.environ, PYTHONPATH=ROOT)
    ck = str(tmp_path)
    r = subprocess.run([sys.executable, "trainNetwork.py", "--synthetic", "--n_shot", "1", "--n_query", "1", "--epoch", "2",
                        "--n_episode", "2", "--ema_decay", "0.9", "--clip_grad_norm", "0.5", "--episodes_per_step", "2",
                        "--model_path", ck, "--name", "t"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    files = os.listdir(os.path.join(ck, "t"))
    assert "model_epoch_2.pt" in files and "model_epoch_2_ema.pt" in files
    lines = r.stdout.splitlines()
    plain = [l for l in lines if l.startswith("Class: ")]
    marked = [l for l in lines if l.startswith("[EMA] Class: ")]
    assert plain and [l.split(" -- ")[0] for l in marked] == ["[EMA] " + l.split(" -- ")[0] for l in plain]
    assert sum(l.startswith("[EMA] Avg testing results across all classes Epoch -- 2 are: Query_rec:") for l in lines) == 1
    assert any("[grad norm:" in l for l in lines)
    raw = torch.load(os.path.join(ck, "t", "model_epoch_2.pt"), weights_only=True)
    avg = torch.load(os.path.join(ck, "t", "model_epoch_2_ema.pt"), weights_only=True)
    assert list(raw) == list(avg)
    differ = [k for k in raw if not torch.equal(raw[k], avg[k])]
    assert differ and not any("running_" in k or "num_batches" in k for k in differ)
    state = torch.load(os.path.join(ck, "t", "train_state_epoch_2.pt"), map_location="cpu", weights_only=True)
    assert state["ema"]["updates"] == 2 and state["ema"]["decay"] == 0.9       # one two-episode step per epoch
    ev = subprocess.run([sys.executable, "evaluate_Network.py", "--synthetic", "--n_shot", "1", "--n_query", "1",
                         "--sequential_eval", "--model_path", ck, "--name", "t", "--eval_model", "model_epoch_2_ema.pt"],
                        cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert ev.returncode == 0, ev.stdout[-3000:] + ev.stderr[-3000:]
    assert "Class: class00 -- Rec CD:" in ev.stdout
