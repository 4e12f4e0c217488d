"""Gradient-norm clipping in the flat Adam step (K20; arithmetic pinned in include/fpsg_hip.h): the sum of
squares against float64, flat form == pointer-table form, run-to-run bits, the coefficient and the counters, the
``_dscale`` Adam entries against the plain ones, ``FlatAdam(max_grad_norm=...)`` against ``clip_grad_norm_`` +
``torch.optim.Adam``, ``TrainStep`` on both of its gradient paths, and the ``--clip_grad_norm`` line of the entry point."""
import copy
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn as nn

from conftest import ROOT

pytestmark = pytest.mark.gpu

THREADS = 256                                   # kAdamThreads
GRID_CAP = 256 * 16                             # the most workgroups of the sum-of-squares kernel
SECOND_TRIP_N = GRID_CAP * THREADS * 4 + 7      # the first n whose slots need a second trip of the full grid (+ a tail)
SIZES = (1, 3, 4, 5, 1023, 1025, 100003, SECOND_TRIP_N)


@pytest.fixture(scope="module")
def lib():
    from fpsg_amd import _hip
    return _hip.load()


def _clip(lib, g, s, mx, stats=None, stream=None):
    """fpsg_grad_clip_scale on the flat buffer g -> out2 (device)."""
    from fpsg_amd import _hip
    n = g.numel()
    nbytes = lib.fpsg_grad_norm_workspace_bytes(n)
    ws = torch.empty(nbytes // 8, dtype=torch.float64, device=g.device)
    out2 = torch.full((2,), -7.0, device=g.device)
    rc = lib.fpsg_grad_clip_scale(_hip.ptr(g), n, s, mx, _hip.ptr(ws), nbytes, _hip.ptr(out2),
                                  None if stats is None else _hip.ptr(stats), stream)
    assert rc == 0, lib.fpsg_last_error()
    return out2


def _segments(gpu, n, lengths, null_at, misaligned_at, seed):
    """Gradient tensors of the given lengths (the last one takes the rest of n): one absent, one a view that starts one
    float past an aligned address.  Returns (tensors or None, device pointer table, device offsets, gathered flat buffer)."""
    lengths = list(lengths) + [n - sum(lengths)]
    assert lengths[-1] > 0
    g = torch.Generator(device=gpu).manual_seed(seed)
    tensors, ptrs = [], []
    for k, ln in enumerate(lengths):
        if k == null_at:
            tensors.append(None)
            ptrs.append(0)
            continue
        if k == misaligned_at:
            base = torch.randn(ln + 8, device=gpu, generator=g)
            t = base[1:1 + ln]
            assert t.data_ptr() % 16 == 4
        else:
            t = torch.randn(ln, device=gpu, generator=g)
        tensors.append(t)
        ptrs.append(t.data_ptr())
    off = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    table = torch.tensor(ptrs, dtype=torch.int64, device=gpu)
    seg_off = torch.from_numpy(off).to(gpu)
    flat = torch.cat([torch.zeros(ln, device=gpu) if t is None else t for t, ln in zip(tensors, lengths)])
    assert flat.numel() == n
    return tensors, table, seg_off, flat


def _clip_segments(lib, table, seg_off, n, s, mx, stats=None):
    from fpsg_amd import _hip
    nbytes = lib.fpsg_grad_norm_workspace_bytes(n)
    ws = torch.empty(nbytes // 8, dtype=torch.float64, device=table.device)
    out2 = torch.full((2,), -7.0, device=table.device)
    rc = lib.fpsg_grad_clip_scale_segments(_hip.ptr(table), _hip.ptr(seg_off), table.numel(), n, s, mx, _hip.ptr(ws), nbytes,
                                           _hip.ptr(out2), None if stats is None else _hip.ptr(stats), None)
    assert rc == 0, lib.fpsg_last_error()
    return out2


# ---- 1. the sum of squares ---------------------------------------------------------------------------------------------

def _data(kind, n, rng):
    if kind == "zeros":
        return np.zeros(n, dtype=np.float32)
    g = rng.standard_normal(n).astype(np.float32)
    if kind == "tiny":
        return g * np.float32(1e-20)
    if kind == "large":
        return g * np.float32(1e18)
    if kind == "one_huge":
        g *= np.float32(1e-3)
        g[(7 * n) // 11] = np.float32(1e30)
    return g


@pytest.mark.parametrize("n", SIZES)
def test_norm_against_float64(gpu, lib, n):
    """out2[0] against |s| sqrt(sum g^2) in numpy float64, rounded to fp32, within ONE fp32 ulp.  The kernel's only
    roundings are fp64 adds of non-negative terms (each square is exact in fp64: 24 x 24 bits), at most n of them in a
    chain, so its S is within n 2^-53 < 1e-9 relative of the exact sum, the sqrt and the product add 2^-52; numpy's
    pairwise float64 sum is as close.  Both sides are therefore within ~1e-9 relative of the exact norm before the
    one rounding to fp32 (6e-8): they round to the same fp32 value or, when the exact value lies within 1e-9 of a
    rounding boundary, to neighbours."""
    rng = np.random.default_rng(n)
    for kind, s in (("normal", 1.0), ("normal", -0.25), ("tiny", 1.0), ("large", 0.5), ("zeros", 0.125), ("one_huge", 1.0)):
        g = _data(kind, n, rng)
        out = _clip(lib, torch.from_numpy(g).to(gpu), s, math.inf).cpu().numpy()
        want = np.float32(abs(s) * np.sqrt(np.sum(g.astype(np.float64) ** 2)))
        assert np.isfinite(want) and (want > 0 or kind == "zeros"), (kind, want)     # no underflow, no overflow
        assert abs(float(out[0]) - float(want)) <= float(np.spacing(want)), (n, kind, out[0], want)
        assert out[1] == np.float32(s), (n, kind)                                     # inf never clips
        if kind == "zeros":
            assert out[0] == 0.0
            assert _clip(lib, torch.from_numpy(g).to(gpu), s, 0.5).cpu().numpy()[1] == np.float32(s)


# ---- 2. flat form == pointer-table form ----------------------------------------------------------------------------------

@pytest.mark.parametrize("n,lengths,null_at,misaligned_at", [
    (100003, (1, 3, 111, 5, 4096), 2, 4),
    (100003, (1, 3, 111, 5, 4096), 0, 5),                      # the long last segment misaligned, the first one absent
    (SECOND_TRIP_N, (5, 2 * 1024 * 1024 + 3), 0, 2),           # both loops of the kernel, segments that end inside a vector
])
def test_segment_form_equals_flat_form(gpu, lib, n, lengths, null_at, misaligned_at):
    tensors, table, seg_off, flat = _segments(gpu, n, lengths, null_at, misaligned_at, seed=n % 1000)
    assert flat.data_ptr() % 16 == 0
    for s, mx in ((1.0, math.inf), (0.5, 3.0)):
        a = _clip(lib, flat, s, mx)
        b = _clip_segments(lib, table, seg_off, n, s, mx)
        assert torch.equal(a, b), (a, b)
        assert float(a[0]) > 0
    want = abs(0.5) * math.sqrt(float((flat.double() ** 2).sum()))
    assert abs(float(a[0]) - want) <= 2e-7 * want


# ---- 3. the same bits from run to run and from stream to stream -----------------------------------------------------------

def test_bits_do_not_depend_on_the_run_or_the_stream(gpu, lib):
    for n in (100003, SECOND_TRIP_N):
        g = torch.randn(n, device=gpu, generator=torch.Generator(device=gpu).manual_seed(n % 97))
        first = _clip(lib, g, 0.5, 1.0)
        assert torch.equal(first, _clip(lib, g, 0.5, 1.0))
        torch.cuda.synchronize()
        outs = []
        for _ in range(2):
            side = torch.cuda.Stream(device=gpu)
            with torch.cuda.stream(side):
                outs.append(_clip(lib, g, 0.5, 1.0, stream=side.cuda_stream))
            side.synchronize()
        assert torch.equal(outs[0], first) and torch.equal(outs[1], first)


# ---- 4. the coefficient and the counters --------------------------------------------------------------------------------

def _spec_factor(norm32, s, mx):
    """include/fpsg_hip.h's fp32 expression, in numpy float32, from the kernel's own norm."""
    with np.errstate(all="ignore"):
        x = np.float32(mx) / (np.float32(norm32) + np.float32(1e-6))
        coef = x if (x < 1 or np.isnan(x)) else np.float32(1.0)
        return np.float32(s) * coef, coef


def test_coefficient(gpu, lib):
    g = torch.randn(100003, device=gpu, generator=torch.Generator(device=gpu).manual_seed(1))
    norm = float(g.double().norm())
    for s in (1.0, 0.125, -1.0 / 3):
        s32 = np.float32(s)
        for mx in (2 * norm, 1e30, math.inf, abs(s) * norm * 1.001):
            assert _clip(lib, g, s, mx).cpu().numpy()[1] == s32, (s, mx)            # nothing clipped: the factor is s itself
        for mx in (abs(s) * norm * 0.999, 1.0, 0.37, 1e-6, 0.0):
            out = _clip(lib, g, s, mx).cpu().numpy()
            want, coef = _spec_factor(out[0], s, mx)
            assert coef < 1 and out[1] == want, (s, mx, out, want)


def test_nonfinite_entries_and_counters(gpu, lib):
    n = 100003
    base = torch.randn(n, device=gpu, generator=torch.Generator(device=gpu).manual_seed(2))
    norm = float(base.double().norm())
    with_nan, with_inf = base.clone(), base.clone()
    with_nan[77777] = float("nan")
    with_inf[n - 1] = float("-inf")                                                  # in the n % 4 tail
    stats = torch.zeros(4, dtype=torch.float64, device=gpu)
    out = _clip(lib, with_nan, 0.5, 1.0, stats).cpu().numpy()
    assert np.isnan(out[0]) and np.isnan(out[1])
    assert stats.tolist() == [1.0, 0.0, 1.0, 0.0]
    out = _clip(lib, with_inf, 0.5, 1.0, stats).cpu().numpy()
    assert out[0] == np.inf and out[1] == 0.0
    assert stats.tolist() == [2.0, 1.0, 2.0, 0.0]
    # a sequence of five calls with known outcomes
    stats.zero_()
    seen = []
    for g, s, mx in ((base, 1.0, 2 * norm), (base, 1.0, norm / 2), (with_nan, 1.0, 1.0), (with_inf, 1.0, 1.0),
                     (base, 3.0, 4 * norm)):
        seen.append(float(_clip(lib, g, s, mx, stats)[0]))
    assert seen[4] > seen[0] and abs(seen[4] - 3 * norm) <= 1e-6 * 3 * norm
    assert stats.tolist() == [5.0, 2.0, 2.0, seen[4]]                               # clipped: the second call and the inf one
    # without counters the call does the same
    assert float(_clip(lib, base, 3.0, 4 * norm)[0]) == seen[4]


# ---- 5. the _dscale entries -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("step", [1, 7])
def test_dscale_entries_equal_the_plain_ones_bit_for_bit(gpu, lib, step):
    from fpsg_amd import _hip
    n = 100003
    tensors, table, seg_off, flat = _segments(gpu, n, (1, 3, 111, 5, 4096), 2, 4, seed=step)
    gen = torch.Generator(device=gpu).manual_seed(10 + step)
    p0 = torch.randn(n, device=gpu, generator=gen)
    m0 = torch.randn(n, device=gpu, generator=gen) * 0.05
    v0 = torch.rand(n, device=gpu, generator=gen) * 0.01
    scale = 0.3
    dev_scale = torch.tensor([-9.0, scale], device=gpu)                              # read from out2 + 1, as FlatAdam does
    hyper = (2e-3, 0.9, 0.999, 1e-8, step)

    def run(entry, *front, last):
        p, m, v = p0.clone(), m0.clone(), v0.clone()
        rc = entry(_hip.ptr(p), *front, _hip.ptr(m), _hip.ptr(v), n, *hyper, last, None)
        assert rc == 0, lib.fpsg_last_error()
        return p, m, v

    plain = run(lib.fpsg_adam_step, _hip.ptr(flat), last=scale)
    dev = run(lib.fpsg_adam_step_dscale, _hip.ptr(flat), last=_hip.ptr(dev_scale) + 4)
    seg = run(lib.fpsg_adam_step_segments, _hip.ptr(table), _hip.ptr(seg_off), table.numel(), last=scale)
    seg_dev = run(lib.fpsg_adam_step_segments_dscale, _hip.ptr(table), _hip.ptr(seg_off), table.numel(),
                  last=_hip.ptr(dev_scale) + 4)
    for a, b, c, d in zip(plain, dev, seg, seg_dev):
        assert torch.equal(a, b) and torch.equal(c, d) and torch.equal(a, c)
    assert not torch.equal(plain[0], p0)


# ---- 6. FlatAdam against torch ----------------------------------------------------------------------------------------------

def _net():
    torch.manual_seed(0)
    # (test_optim_gpu.py's: no BatchNorm behind a biased convolution)
    return nn.Sequential(nn.Conv1d(3, 37, 1), nn.Tanh(), nn.Conv1d(37, 5, 1), nn.Flatten(), nn.Linear(5 * 31, 7))


def _loss(net, x):
    return net(x).square().mean()


def test_flat_adam_matches_clip_grad_norm_and_torch_adam(gpu):
    from fpsg_amd.optim import FlatAdam
    a = _net().to(gpu)
    b = copy.deepcopy(a)
    torch.manual_seed(1)
    xs = [torch.randn(16, 3, 31, device=gpu) for _ in range(8)]
    _loss(b, xs[0]).backward()
    max_norm = float(torch.sqrt(sum((p.grad.double() ** 2).sum() for p in b.parameters())))
    b.zero_grad(set_to_none=True)
    opt_a = FlatAdam(a.parameters(), lr=3e-3, betas=(0.9, 0.999), max_grad_norm=max_norm)
    opt_b = torch.optim.Adam(b.parameters(), lr=3e-3, betas=(0.9, 0.999))
    assert opt_a.max_grad_norm == max_norm and opt_a.last_grad_norm is None
    assert "max_grad_norm" not in opt_a.param_groups[0] and "max_grad_norm" not in opt_a.state_dict()["param_groups"][0]
    clipped = 0
    for it, x in enumerate(xs):
        weight = 4.0 if it % 2 == 0 else 0.25             # the loss, and with it the norm, well above / below the threshold
        for net, opt in ((a, opt_a), (b, opt_b)):
            opt.zero_grad(set_to_none=True)
            (weight * _loss(net, x)).backward()
        total = torch.nn.utils.clip_grad_norm_(list(b.parameters()), max_norm)
        clipped += int(max_norm / (float(total) + 1e-6) < 1)
        opt_a.step()
        opt_b.step()
        assert abs(float(opt_a.last_grad_norm) - float(total)) <= 1e-4 * float(total), it
        for pa, pb in zip(a.parameters(), b.parameters()):
            assert torch.allclose(pa, pb, rtol=2e-5, atol=2e-7), (it, float((pa - pb).abs().max()))
    assert 0 < clipped < 8                             # some steps clip and some do not
    stats = opt_a.clip_stats(reset=False)
    assert stats["steps"] == 8 and stats["clipped"] == clipped and stats["nonfinite"] == 0 and stats["max_norm_seen"] > max_norm
    assert opt_a.clip_stats()["steps"] == 8 and opt_a.clip_stats()["steps"] == 0          # the read resets
    for pa, pb in zip(a.parameters(), b.parameters()):
        sa, sb = opt_a.state[pa], opt_b.state[pb]
        assert torch.allclose(sa["exp_avg"], sb["exp_avg"], rtol=2e-4, atol=1e-9)
        assert torch.allclose(sa["exp_avg_sq"], sb["exp_avg_sq"], rtol=2e-4, atol=1e-12)


@pytest.mark.parametrize("path", ["table", "flat", "gather"])
def test_a_threshold_that_never_clips_changes_no_bit(gpu, path):
    """max_grad_norm=1e30 against no clipping, the same gradients (the library's conv backward is not bit-reproducible,
    so they are computed once and handed to both), step for step, on each of FlatAdam's three gradient paths."""
    from fpsg_amd.optim import FlatAdam
    a, b, src = _net().to(gpu), _net().to(gpu), _net().to(gpu)
    opt_a, opt_b = FlatAdam(a.parameters(), lr=2e-3, max_grad_norm=1e30), FlatAdam(b.parameters(), lr=2e-3)
    flats = {}
    if path == "flat":
        for opt in (opt_a, opt_b):
            flats[opt] = torch.zeros_like(opt.flat_param)
            opt.bind_gradients(flats[opt])
    torch.manual_seed(4)
    for it in range(4):
        src.zero_grad(set_to_none=True)
        _loss(src, torch.randn(8, 3, 31, device=gpu)).backward()
        opt_a.grad_scale = opt_b.grad_scale = (1.0, 1.0 / 3, 0.5, 1.0)[it]
        for net, opt in ((a, opt_a), (b, opt_b)):
            grads = {n_: p.grad for n_, p in src.named_parameters()}
            for (n_, p), (q, off, cnt) in zip(reversed(list(net.named_parameters())), opt._layout):
                assert q is p
                if path == "flat":
                    flats[opt][off:off + cnt].copy_(grads[n_].reshape(-1))
                    p.grad = flats[opt][off:off + cnt].view(p.shape)
                elif path == "gather" and p.dim() == 3:
                    p.grad = grads[n_].clone().transpose(0, 1).contiguous().transpose(0, 1)      # not contiguous
                    assert not p.grad.is_contiguous() or p.shape[0] == 1 or p.shape[1] == 1
                else:
                    p.grad = grads[n_].clone()
            if path == "flat":
                assert opt._bound_gradient() is flats[opt]
            elif path == "table":
                assert opt._bound_gradient() is None and opt._pointer_table() is not None
            else:
                assert opt._bound_gradient() is None and opt._pointer_table() is None
            opt.step()
        for pa, pb in zip(a.parameters(), b.parameters()):
            assert torch.equal(pa, pb), (path, it)
        want = opt_a.grad_scale * math.sqrt(sum(float((p.grad.double() ** 2).sum()) for p in src.parameters()))
        assert abs(float(opt_a.last_grad_norm) - want) <= 1e-5 * want, (path, it)
    assert torch.equal(opt_a.flat_exp_avg, opt_b.flat_exp_avg) and torch.equal(opt_a.flat_exp_avg_sq, opt_b.flat_exp_avg_sq)
    stats = opt_a.clip_stats()
    assert stats["steps"] == 4 and stats["clipped"] == 0 and stats["nonfinite"] == 0
    # the maximum is over the norms as the library rounds them to fp32: never below the last step's own, bit for bit, and
    # below that step's float64 norm by at most that rounding (one fp32 ulp, 2^-23 relative: when the last step is the
    # largest, `>= want` itself held only where the rounding went up)
    assert stats["max_norm_seen"] >= float(opt_a.last_grad_norm) and stats["max_norm_seen"] >= want * (1.0 - 2.0 ** -23)
    assert opt_b.last_grad_norm is None and opt_b.clip_stats()["steps"] == 0


# ---- 7. through TrainStep ---------------------------------------------------------------------------------------------------

def _train_step(gpu, clip, graph=False):
    from fpsg_amd.engine import TrainStep, build_model, build_optimizer, default_options
    from fpsg_amd.optim import FlatAdam
    torch.manual_seed(0)
    opt = default_options(device="cuda", intra_recon=True, clip_grad_norm=clip)
    m = build_model(opt).to(gpu).train()
    optimizer, _ = build_optimizer(m, opt)
    assert isinstance(optimizer, FlatAdam)
    return m, optimizer, TrainStep(m, optimizer, graph=graph)


def _episodes(gpu, count):
    from fpsg_amd.episodes import synthetic_episode
    return [synthetic_episode(2, 1, n_pts=2048, img_size=64, seed=3 + k, device=gpu) for k in range(count)]


def _mean_gradient_norm(step, optimizer, count):
    """In float64: from the flat buffer (it holds the SUM over the step's episodes) or, on the pointer-table path, from
    the gradient tensors."""
    if count > 1:
        assert optimizer._bound_gradient() is step.buckets.flat
        return float(step.buckets.flat.double().norm()) / count
    assert optimizer._bound_gradient() is None
    return math.sqrt(sum(float((p.grad.double() ** 2).sum()) for p, _, _ in optimizer._layout if p.grad is not None))


@pytest.mark.parametrize("count", [2, 1])
def test_train_step_reports_the_norm_of_the_mean_gradient_and_clips(gpu, count):
    """count = 2: the flat gradient buffer with the folded 1/E; count = 1: the pointer-table path (``direct``)."""
    eps = _episodes(gpu, count)
    m, optimizer, step = _train_step(gpu, clip=1e-6)                   # far below any norm: every step is clipped
    assert optimizer.max_grad_norm == 1e-6
    step(eps, n_episodes_global=count)
    assert optimizer.grad_scale == 1.0                                  # reset behind the step
    want = _mean_gradient_norm(step, optimizer, count)
    got = float(step.last_grad_norm)
    assert want > 0 and abs(got - want) <= 1e-5 * want, (count, got, want)
    assert step.clip_stats() == {"steps": 1, "clipped": 1, "nonfinite": 0, "max_norm_seen": got}
    clipped = optimizer.flat_param.clone()
    del m, optimizer, step
    m, optimizer, step = _train_step(gpu, clip=0.0)
    assert optimizer.max_grad_norm is None
    step(eps, n_episodes_global=count)
    assert step.last_grad_norm is None and optimizer._clip is None      # off: nothing allocated, nothing launched
    assert bool(torch.isfinite(clipped).all()) and not torch.equal(clipped, optimizer.flat_param)


@pytest.mark.parametrize("count", [2, 1])
def test_train_step_with_graph_replay(gpu, count):
    eps = _episodes(gpu, count)
    m, optimizer, step = _train_step(gpu, clip=0.5, graph=True)
    for _ in range(3):                                                  # two eager runs per shape, then capture + replay
        step(eps, n_episodes_global=count)
    assert len(step._graphs) == count
    want = _mean_gradient_norm(step, optimizer, count)
    got = float(step.last_grad_norm)
    assert abs(got - want) <= 1e-5 * want, (count, got, want)
    stats = step.clip_stats()
    assert stats["steps"] == 3 and stats["nonfinite"] == 0 and stats["max_norm_seen"] >= got
    assert bool(torch.isfinite(optimizer.flat_param).all())


# ---- 8. the entry point -----------------------------------------------------------------------------------------------------

def test_training_entry_point_prints_the_line_only_with_the_flag(gpu, tmp_path):
    env = dict(os.environ, PYTHONPATH=ROOT)
    base = [sys.executable, "trainNetwork.py", "--synthetic", "--resident", "--n_shot", "2", "--n_query", "1", "--intra_recon",
            "--epoch", "1", "--n_episode", "3", "--model_path", str(tmp_path)]
    on = subprocess.run(base + ["--name", "on", "--clip_grad_norm", "0.5"], cwd=ROOT, env=env, capture_output=True, text=True,
                        timeout=600)
    assert on.returncode == 0, on.stdout[-3000:] + on.stderr[-3000:]
    lines = [ln for ln in on.stdout.splitlines() if "[grad norm:" in ln]
    assert len(lines) == 1, on.stdout[-3000:]
    m = re.fullmatch(r"  \[grad norm: max (\S+); clipped (\d+) of (\d+) steps; (\d+) non-finite\]", lines[0])
    assert m, lines[0]
    assert math.isfinite(float(m.group(1))) and float(m.group(1)) > 0
    assert int(m.group(3)) == 3 and 0 <= int(m.group(2)) <= 3 and int(m.group(4)) == 0
    before = on.stdout.splitlines()[on.stdout.splitlines().index(lines[0]) - 1]
    assert "episodes/s over" in before                                   # right behind the throughput line
    logs = [f for f in os.listdir(tmp_path / "on") if f.startswith("log_")]
    assert logs and all("grad norm" not in open(tmp_path / "on" / f).read() for f in logs)
    off = subprocess.run(base + ["--name", "off"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert off.returncode == 0, off.stdout[-3000:] + off.stderr[-3000:]
    assert "grad norm" not in off.stdout
