"""K16 on the GPU: farthest point sampling equals its definition bit for bit (replayed round by round through K1, whose
squared distance it shares), picks the float64 farthest point up to fp32 rounding, is deterministic, independent of
the batch and prefix-stable, and feeds ``evaluate_Network.py --set_metrics_points``."""
import math
import re

import numpy as np
import pytest
import torch

from conftest import unit_ball_clouds

pytestmark = pytest.mark.gpu

SHAPES = [(1, 2048, 2048), (37, 2048, 512), (5, 15000, 2048), (3, 16384, 64), (64, 100, 100), (2, 1, 1), (4, 777, 333)]
EDGE_SHAPES = ([(3, N, N) for N in (2, 63, 64)] + [(3, N, 64) for N in (65, 257, 1025, 2049, 4096)]
               + [(3, N, 32) for N in (4097, 8192, 8193)])


def _ball(B, N, seed):
    return unit_ball_clouds(np.random.default_rng(seed), B, N)


def _tanh(B, N, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.tanh(torch.randn(B, N, 3, generator=g)).numpy()


def _lattice(B=3, N=2048, seed=5):
    """Coordinates in {0, 1/8, ..., 7/8}: at most 512 distinct points, every distance exact, most rounds tie."""
    g = torch.Generator().manual_seed(seed)
    return (torch.randint(0, 8, (B, N, 3), generator=g).float() / 8).numpy()


def _repeated(N=512, seed=6):
    """7 distinct points, point i a copy of point i % 7."""
    base = _ball(1, 7, seed)[0]
    assert len({tuple(p) for p in base.tolist()}) == 7
    return base[np.arange(N) % 7][None].copy()


def _cases():
    out = []
    for B, N, n in SHAPES:
        out.append((f"ball-{B}-{N}-{n}", _ball(B, N, 100 + N + B), n))
        out.append((f"tanh-{B}-{N}-{n}", _tanh(B, N, 200 + N + B), n))
    out.append(("lattice", _lattice(), 2048))
    out.append(("repeated", _repeated(), 64))
    # every fps_kernel<T, P> at both ends of its range of N (tests/_dispatch.py names these cases)
    for B, N, n in EDGE_SHAPES:
        out.append((f"ball-{B}-{N}-{n}", _ball(B, N, 100 + N + B), n))
        out.append((f"tanh-{B}-{N}-{n}", _tanh(B, N, 200 + N + B), n))
    out.append(("lattice-64", _lattice(3, 64, 8), 64))          # ties inside <64, 1>; fewer than 64 distinct points
    out.append(("lattice-4096", _lattice(3, 4096, 9), 520))     # ties inside <1024, 4>; runs past the 512 distinct points
    return out


CASES = _cases()
IDS = [c[0] for c in CASES]


def _fps(dev, x, n, start=None):
    from fpsg_amd.sampling import farthest_point_sample
    pts = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(dev)
    idx, md = farthest_point_sample(pts, n, start=start, return_min_dist=True)
    assert idx.dtype == torch.int64 and md.dtype == torch.float32 and idx.shape == md.shape == (x.shape[0], n)
    return pts, idx, md


def _rounds(n):
    """At least 16 rounds spread over 1 .. n-1, with 1, 2 and n-1 (all of them when there are fewer)."""
    if n <= 24:
        return list(range(1, n))
    return sorted({1, 2, 3, n - 2, n - 1} | {int(v) for v in np.linspace(1, n - 1, 20)})


# ---- 1. the definition, bit for bit, through K1 ------------------------------------------------------------------

@pytest.mark.parametrize("name,x,n", CASES, ids=IDS)
def test_every_checked_round_is_the_argmax_of_k1s_distances(gpu, name, x, n):
    """``sided_distance(points, points[idx[:, :t]])`` is D after t picks, by definition and with the same bits (K1 is
    pinned to the oracle bit for bit): its maximum is min_dist[:, t] and the lowest index that attains it is idx[:, t]."""
    from fpsg_amd.metrics import sided_distance
    pts, idx, md = _fps(gpu, x, n)
    B, N, _ = pts.shape
    ar = torch.arange(N, device=gpu)
    for t in _rounds(n):
        picked = torch.gather(pts, 1, idx[:, :t].unsqueeze(-1).expand(-1, -1, 3)).contiguous()
        with torch.no_grad():
            D, _ = sided_distance(pts, picked)
        top = D.max(dim=1).values
        first = torch.where(D == top[:, None], ar[None, :], N).min(dim=1).values
        print(name, "round", t, "max D", top[:3].tolist(), "min_dist", md[:3, t].tolist())
        assert torch.equal(first, idx[:, t]), (name, t, first.tolist()[:5], idx[:, t].tolist()[:5])
        assert torch.equal(top.view(torch.int32), md[:, t].contiguous().view(torch.int32)), (name, t)


# ---- 2. against float64 ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,x,n", CASES, ids=IDS)
def test_every_pick_is_the_float64_farthest_point_up_to_fp32_rounding(gpu, name, x, n):
    """Replaying the GPU's own prefix in float64: at every round t >= 1, D64(idx[t]) >= (1 - 2**-20) max_i D64(i).
    sq_dist carries at most about 6 * 2**-24 relative rounding on fp32 inputs, once on the pick and once on the true
    maximum; 2**-20 covers twice that."""
    _, idx, _ = _fps(gpu, x, n)
    idx = idx.cpu().numpy()
    x64 = x.astype(np.float64)
    B = x.shape[0]
    rows = np.arange(B)
    D = ((x64 - x64[rows, idx[:, 0]][:, None, :]) ** 2).sum(-1)
    worst = 1.0
    for t in range(1, n):
        got, top = D[rows, idx[:, t]], D.max(axis=1)
        with np.errstate(invalid="ignore", divide="ignore"):
            worst = min(worst, float(np.where(top > 0, got / np.where(top > 0, top, 1), 1.0).min()))
        assert (got >= (1 - 2.0 ** -20) * top).all(), (name, t, got[:4], top[:4])
        D = np.minimum(D, ((x64 - x64[rows, idx[:, t]][:, None, :]) ** 2).sum(-1))
    print(name, "lowest D64(pick) / max D64 over all rounds:", worst)


# ---- 3. properties -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,x,n", CASES, ids=IDS)
def test_properties_of_the_picks(gpu, name, x, n):
    _, idx, md = _fps(gpu, x, n)
    idx, md = idx.cpu().numpy(), md.cpu().numpy()
    B, N, _ = x.shape
    assert (idx[:, 0] == 0).all() and np.isposinf(md[:, 0]).all()
    assert (idx >= 0).all() and (idx < N).all()
    assert np.isfinite(md[:, 1:]).all() and (md[:, 1:] >= 0).all()
    assert (np.diff(md[:, 1:], axis=1) <= 0).all(), name          # non-increasing along t
    for b in range(B):
        distinct = len({tuple(p) for p in x[b].tolist()})
        picks = idx[b].tolist()
        k = min(n, distinct)
        assert len(set(picks[:k])) == k and len({tuple(x[b, i].tolist()) for i in picks[:k]}) == k, (name, b)
        assert (md[b, 1:k] > 0).all()
        assert all(i == 0 for i in picks[k:]) and (md[b, k:] == 0).all(), (name, b)   # exhausted: the lowest index repeats
    if name.startswith(("ball", "tanh")):
        assert all(len(set(row.tolist())) == n for row in idx)


def test_repeated_point_cloud_yields_its_distinct_points_first(gpu):
    x = _repeated()
    _, idx, md = _fps(gpu, x, 64)
    picks = idx[0].tolist()
    assert sorted(picks[:7]) == list(range(7)) and picks[7:] == [0] * 57      # the lowest index of every group, then 0
    assert (md[0, 1:7] > 0).all() and (md[0, 7:] == 0).all()
    _, idx3, _ = _fps(gpu, x, 64, start=10)                                  # 10 is a copy of point 3
    picks = idx3[0].tolist()
    assert picks[0] == 10 and sorted(picks[1:7]) == [0, 1, 2, 4, 5, 6] and picks[7:] == [0] * 57


def test_lattice_cloud_ties_in_most_rounds(gpu):
    """The input on which the tie rule bites: the float64 maximum is attained more than once in most rounds."""
    x = _lattice()
    _, idx, _ = _fps(gpu, x, 2048)
    idx = idx.cpu().numpy()
    x64 = x.astype(np.float64)
    D = ((x64[0] - x64[0, idx[0, 0]]) ** 2).sum(-1)
    ties = 0
    for t in range(1, 2048):
        top = D.max()
        ties += int((D == top).sum() > 1)
        assert idx[0, t] == int(np.argmax(D))                      # exact arithmetic here: numpy's first maximum
        D = np.minimum(D, ((x64[0] - x64[0, idx[0, t]]) ** 2).sum(-1))
    print("rounds with an exact tie:", ties, "of 2047")
    assert ties > 1500


# ---- 4. determinism and independence -----------------------------------------------------------------------------

def test_runs_batches_prefixes_and_starts(gpu):
    x = np.concatenate([_ball(19, 2048, 31), _tanh(18, 2048, 32)])
    pts, idx, md = _fps(gpu, x, 2048)
    _, idx2, md2 = _fps(gpu, x, 2048)
    assert torch.equal(idx, idx2) and torch.equal(md.view(torch.int32), md2.view(torch.int32))
    for pos in (0, 17, 36):                                        # a cloud alone = the same cloud inside the batch
        _, i1, m1 = _fps(gpu, x[pos:pos + 1], 2048)
        assert torch.equal(i1[0], idx[pos]) and torch.equal(m1[0].view(torch.int32), md[pos].view(torch.int32)), pos
    for m in (1, 2, 512, 2047):                                    # a call with fewer picks = the first columns
        _, im, mm = _fps(gpu, x, m)
        assert torch.equal(im, idx[:, :m]) and torch.equal(mm.view(torch.int32), md[:, :m].contiguous().view(torch.int32)), m
    # starts: an int, a tensor on either device, and each cloud's own start equals that cloud run alone
    g = torch.Generator().manual_seed(7)
    start = torch.randint(0, 2048, (37,), generator=g)
    start[0], start[1] = 2047, 0
    _, ist, mst = _fps(gpu, x, 300, start=start)
    _, ist_dev, _ = _fps(gpu, x, 300, start=start.to(gpu).int())
    assert torch.equal(ist, ist_dev) and torch.equal(ist[:, 0].cpu(), start)
    assert torch.isposinf(mst[:, 0]).all()
    for pos in (0, 1, 20, 36):
        _, i1, _ = _fps(gpu, x[pos:pos + 1], 300, start=int(start[pos]))
        assert torch.equal(i1[0], ist[pos]), pos
    _, i5, _ = _fps(gpu, x, 300, start=5)
    _, i5t, _ = _fps(gpu, x, 300, start=torch.full((37,), 5))
    assert torch.equal(i5, i5t) and (i5[:, 0] == 5).all() and not torch.equal(i5, idx[:, :300])


def test_c_entry_clamps_a_start_outside_the_cloud(gpu):
    """The wrapper refuses such a start; the kernel, which is the only one to see a device-side value, clamps it."""
    from fpsg_amd import _hip
    lib = _hip.load()
    pts = torch.from_numpy(_ball(3, 500, 41)).to(gpu)
    start = torch.tensor([-7, 10 ** 6, 499], dtype=torch.int32, device=gpu)
    idx = torch.full((3, 50), -1, dtype=torch.int32, device=gpu)
    with torch.cuda.device(gpu):
        rc = lib.fpsg_fps(pts.data_ptr(), 3, 500, 50, start.data_ptr(), idx.data_ptr(), None, None, 0, _hip.stream_of(pts))
    _hip.check(rc, "fpsg_fps")
    assert idx[:, 0].tolist() == [0, 499, 499] and int(idx.min()) >= 0 and int(idx.max()) < 500
    _, want, _ = _fps(gpu, pts.cpu().numpy(), 50, start=torch.tensor([0, 499, 499]))
    assert torch.equal(idx.long(), want)


def test_non_default_stream_and_non_contiguous_input(gpu):
    """Ordered on the current stream; a non-contiguous input is refused (ValueError), not copied."""
    from fpsg_amd.sampling import farthest_point_sample
    x = _tanh(6, 1500, 51)
    _, want, want_md = _fps(gpu, x, 400)
    side = torch.cuda.Stream(device=gpu)
    with torch.cuda.stream(side):
        pts = torch.from_numpy(x).to(gpu)
        for _ in range(3):
            pts = pts * 1.0                                        # work ahead of the launch on the same stream
        idx, md = farthest_point_sample(pts, 400, return_min_dist=True)
    side.synchronize()
    assert torch.equal(idx, want) and torch.equal(md.view(torch.int32), want_md.view(torch.int32))
    wide = torch.from_numpy(np.concatenate([x, x], axis=2)).to(gpu)
    with pytest.raises(ValueError, match="contiguous"):
        farthest_point_sample(wide[:, :, :3], 10)
    with pytest.raises(ValueError, match="contiguous"):
        farthest_point_sample(torch.from_numpy(x).to(gpu)[:, ::2], 10)
    with pytest.raises(TypeError):
        farthest_point_sample(torch.from_numpy(x).to(gpu).double(), 10)


# ---- 5. the gather -----------------------------------------------------------------------------------------------

def test_subsample_gathers_and_its_gradient_scatters(gpu):
    from fpsg_amd.sampling import farthest_point_sample, farthest_point_subsample
    pts = torch.from_numpy(_ball(5, 600, 61)).to(gpu).requires_grad_()
    idx = farthest_point_sample(pts, 128, start=3)
    assert not idx.requires_grad
    sub = farthest_point_subsample(pts, 128, start=3)
    assert sub.shape == (5, 128, 3) and sub.requires_grad
    for b in range(5):
        assert torch.equal(sub[b].detach(), pts.detach()[b, idx[b]])
    sub.sum().backward()
    want = torch.zeros(5, 600, 3, device=gpu)
    for b in range(5):
        want[b, idx[b]] = 1.0
    assert torch.equal(pts.grad, want) and float(pts.grad.sum()) == 5 * 128 * 3


# ---- 6. a non-finite coordinate ----------------------------------------------------------------------------------

def test_one_nan_point_returns_with_indices_in_range(gpu):
    x = _ball(2, 1000, 71)
    x[0, 123, 1] = np.nan
    _, idx, _ = _fps(gpu, x, 200)
    torch.cuda.synchronize(gpu)
    assert int(idx.min()) >= 0 and int(idx.max()) < 1000


# ---- 7. evaluate_Network.py --set_metrics_points -----------------------------------------------------------------

_FLOAT = r"[-+0-9.e]+|nan|inf"


def _main(tmp_path, extra):
    import evaluate_Network
    from fpsg_amd import cli
    opt = cli.few_shot_parser(evaluation=True).parse_args(
        ["--synthetic", "--n_shot", "2", "--n_query", "1", "--sequential_eval", "--model_path", str(tmp_path), "--name", "x"]
        + extra)
    return evaluate_Network.main(opt)


def test_entry_point_reduces_the_clouds_of_the_set_metrics(gpu, tmp_path, monkeypatch, capsys):
    from fpsg_amd import sampling, set_metrics
    full, sets = [], []
    real_sub, real_gm = sampling.farthest_point_subsample, set_metrics.generation_metrics

    def sub(points, n, start=None):
        full.append(points.clone())
        return real_sub(points, n, start)

    def gm(gen, ref, *a, **k):
        sets.append((gen.clone(), ref.clone()))
        return real_gm(gen, ref, *a, **k)

    monkeypatch.setattr(sampling, "farthest_point_subsample", sub)
    monkeypatch.setattr(set_metrics, "generation_metrics", gm)
    res = _main(tmp_path, ["--set_metrics", "--set_metrics_points", "256"])
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("Class: ")]
    per_class = res[-1]
    assert lines and len(lines) == len(per_class) == len(sets)
    # the clouds by hand: every full cloud that arrived, reduced through the index form
    hand = []
    for c in full:
        assert c.shape[1:] == (2048, 3)
        idx = sampling.farthest_point_sample(c, 256, start=0)
        hand += [c[b, idx[b]] for b in range(c.size(0))]
    rows = [r for gen, ref in sets for r in list(gen) + list(ref)]
    assert len(rows) == len(hand) and all(r.shape == (256, 3) for r in rows)
    for r in rows:
        assert sum(int(torch.equal(r, h)) for h in hand) >= 1
    for h in hand:
        assert sum(int(torch.equal(r, h)) for r in rows) >= 1
    for ln, name, (gen, ref) in zip(lines, sorted(per_class), sets):
        want = real_gm(gen, ref)
        m = re.fullmatch(rf"Class: (\S+) -- Rec CD: ({_FLOAT}); Rec EMD: ({_FLOAT}); MMD-CD@256: ({_FLOAT}); "
                         rf"COV-CD@256: ({_FLOAT}); 1-NNA-CD@256: ({_FLOAT})", ln)
        assert m and m.group(1) == str(name), ln
        assert "MMD-CD:" not in ln and "COV-CD:" not in ln and "1-NNA-CD:" not in ln
        for key, text in zip(("mmd_cd", "cov_cd", "nna_cd"), m.groups()[3:]):
            assert per_class[name][key] == want[key] and text == str(want[key]), (ln, key)
            assert math.isfinite(float(text))
    # without the option the line is the one of --set_metrics alone; too many points name both numbers
    monkeypatch.setattr(sampling, "farthest_point_subsample", real_sub)
    monkeypatch.setattr(set_metrics, "generation_metrics", real_gm)
    full.clear()
    _main(tmp_path, ["--set_metrics"])
    plain = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("Class: ")]
    assert len(plain) == len(lines) and not full
    for ln in plain:
        assert re.fullmatch(rf"Class: \S+ -- Rec CD: ({_FLOAT}); Rec EMD: ({_FLOAT}); MMD-CD: ({_FLOAT}); "
                            rf"COV-CD: ({_FLOAT}); 1-NNA-CD: ({_FLOAT})", ln), ln
        assert "@" not in ln
    with pytest.raises(ValueError, match=r"4096.*2048"):
        _main(tmp_path, ["--set_metrics", "--set_metrics_points", "4096"])
