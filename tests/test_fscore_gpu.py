"""K17 on the GPU: the distance profile equals torch on the same rows integer for integer and bit for bit, handles NaN,
infinities and -0 as defined, is independent of the batch; ``metrics.fscore`` equals a float64 brute force exactly where
fp32 rounds nowhere; and the path up to ``evaluate_Network.py --fscore`` reports what ``metrics.fscore`` gives."""
import math
import statistics

import numpy as np
import pytest
import torch

from conftest import unit_ball_clouds

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (63, 65), (64, 64), (255, 257), (256, 1), (2048, 2048), (4097, 1023), (70001, 3)]
# Euclidean thresholds: 0; one whose square is planted in the rows; one above every entry; one below every entry
TAU_ZERO, TAU_PLANTED, TAU_ABOVE, TAU_BELOW = 0.0, 0.3, 1.0, 0.1
SPECIAL = (TAU_ZERO, TAU_PLANTED, TAU_ABOVE, TAU_BELOW)


def _tau2(taus, device):
    """float32(tau ** 2), the square formed in double and rounded once: what ``distance_profile`` compares against."""
    return torch.from_numpy(np.array([float(t) ** 2 for t in taus], dtype=np.float64).astype(np.float32)).to(device)


def _rows(B, n, seed, device, zeros):
    """Random fp32 in [0.05, 0.95]; every 7th entry from index 0 is float32(0.3 ** 2) exactly; ``zeros``: every 11th entry
    from index 5 is 0 (then 0 is the minimum; without them TAU_BELOW ** 2 = 0.01 lies below every entry)."""
    g = torch.Generator(device=device).manual_seed(seed)
    d = torch.rand((B, n), generator=g, device=device) * 0.9 + 0.05
    d[:, 0::7] = _tau2([TAU_PLANTED], device)[0]
    if zeros:
        d[:, 5::11] = 0.0
    return d.contiguous()


def _torch_profile(d1, d2, tau2):
    counts = torch.stack([(d[:, None, :] <= tau2[None, :, None]).sum(-1) for d in (d1, d2)], dim=1).to(torch.int32)
    maxima = torch.stack([d.clamp_min(0).amax(-1) for d in (d1, d2)], dim=1)
    return counts, maxima


def _threshold_lists(T):
    if T == 1:
        return [(t,) for t in SPECIAL]
    if T == 2:
        return [(TAU_PLANTED, TAU_ZERO), (TAU_ABOVE, TAU_BELOW)]
    rng = np.random.default_rng(T)
    rest = rng.random(T - 4).tolist()
    order = rng.permutation(T)
    both = list(SPECIAL) + rest
    return [tuple(both[i] for i in order)]                         # any order


# ---- 5. exact parity with torch on the same rows -----------------------------------------------------------------

@pytest.mark.parametrize("T", [1, 2, 16])
@pytest.mark.parametrize("B", [1, 5, 37])
@pytest.mark.parametrize("N,M", SHAPES)
def test_profile_equals_torch_on_the_same_rows(gpu, N, M, B, T):
    from fpsg_amd.metrics import distance_profile
    d1 = _rows(B, N, 1000 + N, gpu, zeros=True)                    # odd N: the rows after the first are not 16-B aligned
    d2 = _rows(B, M, 2000 + M, gpu, zeros=False)
    for taus in _threshold_lists(T):
        counts, maxima = distance_profile(d1, d2, taus)
        assert counts.dtype == torch.int32 and tuple(counts.shape) == (B, 2, T)
        assert maxima.dtype == torch.float32 and tuple(maxima.shape) == (B, 2)
        assert not counts.requires_grad and not maxima.requires_grad
        want_c, want_m = _torch_profile(d1, d2, _tau2(taus, gpu))
        assert torch.equal(counts, want_c), (taus, counts[0].tolist(), want_c[0].tolist())
        assert torch.equal(maxima, want_m), (maxima[0].tolist(), want_m[0].tolist())
        for t, tau in enumerate(taus):                             # the inputs do what they were built for
            c = counts[:, :, t]
            if tau == TAU_ABOVE:
                assert (c[:, 0] == N).all() and (c[:, 1] == M).all()
            if tau == TAU_BELOW:
                assert (c[:, 1] == 0).all() and (c[:, 0] == len(range(5, N, 11))).all()
            if tau == TAU_ZERO:
                assert (c[:, 1] == 0).all() and (c[:, 0] == len(range(5, N, 11))).all()
            if tau == TAU_PLANTED:                                 # the planted entries equal the threshold: counted
                assert (c[:, 1] >= len(range(0, M, 7))).all()
                below = (d2 < _tau2([tau], gpu)[0]).sum(-1)
                assert torch.equal(c[:, 1] - below, torch.full_like(below, len(range(0, M, 7))))


# ---- 6. special values -------------------------------------------------------------------------------------------

def test_nan_infinity_and_negative_zero(gpu):
    from fpsg_amd.metrics import distance_profile
    N, M = 300, 77
    taus = (0.0, 0.3, 1.0, 1e18)                                   # squares 0 .. 1e36, all finite in fp32
    tau2 = _tau2(taus, gpu)
    assert torch.isfinite(tau2).all()
    d1, d2 = _rows(4, N, 31, gpu, zeros=False), _rows(4, M, 32, gpu, zeros=False)
    nan, inf = float("nan"), float("inf")
    for d, n in ((d1, N), (d2, M)):
        d[0, 3], d[0, n - 1], d[0, 10], d[0, 64 % n] = nan, nan, inf, -0.0   # NaN, +inf and -0 in one row
        d[1, 0], d[1, 20], d[1, 21] = nan, -0.0, -0.0              # NaN and -0, no infinity
        d[2, :] = nan                                              # nothing but NaN
        d[3, :] = -0.0                                             # nothing but -0
    counts, maxima = distance_profile(d1, d2, taus)
    for k, (d, n) in enumerate(((d1, N), (d2, M))):
        finite = torch.where(torch.isfinite(d), d, torch.zeros_like(d))
        for t in range(len(taus)):
            # NaN is counted nowhere; +inf under no finite threshold; -0 <= 0 counts
            want = ((d <= tau2[t]) & ~torch.isnan(d) & ~torch.isinf(d)).sum(-1).to(torch.int32)
            assert torch.equal(counts[:, k, t], want), (k, t)
        assert counts[0, k, 0] == 1 and counts[1, k, 0] == 2       # the -0 entries, and nothing else, under tau = 0
        assert counts[0, k, 3] == n - 3 and counts[1, k, 3] == n - 1
        assert counts[2, k].tolist() == [0, 0, 0, 0] and counts[3, k].tolist() == [n, n, n, n]
        assert maxima[0, k] == inf                                 # +inf is the maximum, the NaNs are ignored
        assert maxima[1, k] == finite[1].max() and maxima[1, k] > 0
        for b in (2, 3):                                           # all NaN, all -0: max(0, .) = +0
            assert maxima[b, k] == 0 and not torch.signbit(maxima[b, k])


# ---- 7. independence of the batch --------------------------------------------------------------------------------

def test_pair_alone_two_runs_and_threshold_order(gpu):
    from fpsg_amd.metrics import distance_profile
    B, N, M = 37, 2049, 777
    taus = (0.0, 0.1, 0.3, 0.55, 0.8, 1.0)
    d1, d2 = _rows(B, N, 41, gpu, zeros=True), _rows(B, M, 42, gpu, zeros=False)
    counts, maxima = distance_profile(d1, d2, taus)
    again = distance_profile(d1, d2, taus)
    assert torch.equal(counts, again[0]) and torch.equal(maxima.view(torch.int32), again[1].view(torch.int32))
    for b in range(B):
        c, m = distance_profile(d1[b:b + 1].clone(), d2[b:b + 1].clone(), taus)
        assert torch.equal(c[0], counts[b]) and torch.equal(m[0].view(torch.int32), maxima[b].view(torch.int32)), b
    c, m = distance_profile(d1, d2, taus[::-1])                    # descending: the permuted columns
    assert torch.equal(c, counts.flip(-1)) and torch.equal(m, maxima)
    assert (counts[:, :, 1:] >= counts[:, :, :-1]).all()


# ---- 8. end to end against float64, exact ------------------------------------------------------------------------

LATTICE_M = (0, 1, 2, 3, 4, 6, 8)                                  # thresholds m / 64: their squares are exact in fp32


def _lattice_pairs(N, M, seed):
    """Three pairs with coordinates k / 64, k an integer in [-64, 64]: every difference, square and three-term sum is
    exact in fp32.  Duplicated points; points of p1 planted at lattice distance m / 64 along an axis from a point of p2;
    pair 2 is the same point set on both sides."""
    g = torch.Generator().manual_seed(seed)
    k1 = torch.randint(-64, 65, (3, N, 3), generator=g)
    k2 = torch.randint(-64, 65, (3, M, 3), generator=g)
    for b in range(2):
        k1[b, 5:10] = k1[b, 0:5]                                   # duplicates on both sides
        k2[b, M - 3:] = k2[b, 0:3]
        for s, m in enumerate(LATTICE_M):                          # four plants per threshold and axis, from slot 11 on
            for axis in range(3):
                for r in range(4):
                    slot = (3 * s + axis) * 4 + r
                    i, j = 11 + slot, 5 * slot % (M - 3)
                    k1[b, i] = k2[b, j]
                    k1[b, i, axis] += m if k2[b, j, axis] + m <= 64 else -m
    k1[2] = k2[2][torch.arange(N) % M]                             # N > M: every point of p2 at least once
    return k1.float() / 64, k2.float() / 64


def _float64_fscore(p1, p2, taus):
    a, b = p1.double(), p2.double()
    d = ((a[:, :, None, :] - b[:, None, :, :]) ** 2).sum(-1)       # [B,N,M] squared distances
    d1, d2 = d.amin(2), d.amin(1)
    t2 = torch.tensor([float(t) ** 2 for t in taus], dtype=torch.float64, device=p1.device)
    counts = torch.stack([(x[:, None, :] <= t2[None, :, None]).sum(-1) for x in (d1, d2)], dim=1)
    precision, recall = counts[:, 0].double() / p1.size(1), counts[:, 1].double() / p2.size(1)
    f = [[0.0 if p + r == 0 else 2 * p * r / (p + r) for p, r in zip(ps, rs)]
         for ps, rs in zip(precision.tolist(), recall.tolist())]
    hd = [math.sqrt(max(x, y)) for x, y in zip(d1.amax(1).tolist(), d2.amax(1).tolist())]
    return {"counts": counts, "precision": precision, "recall": recall, "fscore": f, "hausdorff": hd, "d1": d1,
            "d2": d2, "t2": t2}


@pytest.mark.parametrize("N,M", [(130, 70), (2048, 2048)])
def test_fscore_equals_float64_on_a_lattice(gpu, N, M):
    from fpsg_amd.metrics import fscore, sided_distances
    taus = tuple(m / 64 for m in LATTICE_M)
    p1, p2 = (x.to(gpu).contiguous() for x in _lattice_pairs(N, M, 100 + N))
    want = _float64_fscore(p1, p2, taus)
    # the inputs do what they were built for: minima that EQUAL a threshold, for every threshold, and K1 rounds nowhere
    for t2 in want["t2"].tolist():
        assert int((want["d1"][:2] == t2).sum()) >= 1, t2
    k1 = sided_distances(p1, p2)
    assert torch.equal(k1[0].double(), want["d1"]) and torch.equal(k1[2].double(), want["d2"])
    got = fscore(p1, p2, taus)
    assert set(got) == {"precision", "recall", "fscore", "hausdorff", "counts", "maxima"}
    assert torch.equal(got["counts"].long(), want["counts"])
    assert torch.equal(got["precision"], want["precision"]) and torch.equal(got["recall"], want["recall"])
    assert got["fscore"].dtype == torch.float64 and got["fscore"].tolist() == want["fscore"]
    assert got["hausdorff"].dtype == torch.float64 and got["hausdorff"].tolist() == want["hausdorff"]
    assert not got["fscore"].requires_grad
    # the pair with the same points on both sides: F = 1 at every threshold, tau = 0 included, and HD = 0
    assert got["fscore"][2].tolist() == [1.0] * len(taus) and got["hausdorff"][2].item() == 0.0
    assert 0.0 < got["fscore"][0, 1].item() < 1.0 and got["hausdorff"][0].item() > 0.0


# ---- 9. sanity on random clouds ----------------------------------------------------------------------------------

def test_random_clouds_monotone_bounded_and_symmetric(gpu):
    from fpsg_amd.metrics import fscore, sided_distances
    rng = np.random.default_rng(9)
    p1 = torch.from_numpy(unit_ball_clouds(rng, 5, 2048)).to(gpu)
    p2 = torch.from_numpy(unit_ball_clouds(rng, 5, 2048)).to(gpu)
    taus = (0.0, 0.005, 0.01, 0.02, 0.05, 0.1, 0.2, 0.5, 2.0)
    a, b = fscore(p1, p2, taus), fscore(p2, p1, taus)
    for key in ("precision", "recall"):
        assert (a[key][:, 1:] >= a[key][:, :-1]).all(), key        # non-decreasing in tau
        assert (a[key][:, -1] == 1.0).all() and (a[key][:, 0] == 0.0).all()
    assert (a["fscore"] >= 0).all() and (a["fscore"] <= 1).all()
    assert 0.0 < a["fscore"][:, 4].min() and a["fscore"][:, 4].max() < 1.0
    assert torch.equal(a["precision"], b["recall"]) and torch.equal(a["recall"], b["precision"])
    assert torch.equal(a["fscore"].view(torch.int64), b["fscore"].view(torch.int64))
    assert torch.equal(a["hausdorff"].view(torch.int64), b["hausdorff"].view(torch.int64))
    assert torch.equal(a["counts"], b["counts"].flip(1)) and torch.equal(a["maxima"], b["maxima"].flip(1))
    d1, _, d2, _ = sided_distances(p1, p2)
    want_c, want_m = _torch_profile(d1, d2, _tau2(taus, gpu))
    assert torch.equal(a["counts"], want_c) and torch.equal(a["maxima"], want_m)
    assert torch.equal(a["hausdorff"], want_m.double().amax(1).sqrt())


# ---- 10. the evaluation item -------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def model(gpu):
    from fpsg_amd.engine import build_model, default_options
    torch.manual_seed(3)
    return build_model(default_options(device="cuda")).to(gpu).eval()


@pytest.mark.parametrize("Q", [1, 5])
def test_evaluation_item_fscore(gpu, model, monkeypatch, Q):
    """EvalItem(fscore=...): the new fields are ``metrics.fscore`` of the clouds the item returns, eager items and graph
    replays alike, and the two reference metrics keep their bits."""
    from fpsg_amd.engine import EvalItem
    from fpsg_amd.episodes import synthetic_episode
    from fpsg_amd.metrics import fscore
    taus = (0.02, 0.05)
    grids = model.pc_decoder.sample_grids(Q, gpu, torch.Generator(device=gpu).manual_seed(9))
    orig = model.pc_decoder.forward
    monkeypatch.setattr(model.pc_decoder, "forward",
                        lambda h, grid=None, generator=None, pack=None: orig(h, grid=grids, pack=pack))
    eps = [synthetic_episode(1, Q, n_pts=2048, img_size=96, seed=80 + i, device=gpu) for i in range(4)]
    for graph in (True, False):
        with EvalItem(model, graph=graph) as item:
            plain = [item(ep) for ep in eps]
        with EvalItem(model, graph=graph, fscore=taus, return_clouds=True) as item:
            got = [item(ep) for ep in eps]
            assert bool(item._graphs) == graph, "the third item of a shape is captured, with the graph on"
        with EvalItem(model, graph=graph, fscore=taus) as item:
            alone = [item(ep) for ep in eps]
        for p, g, a in zip(plain, got, alone):
            assert set(p) == {"cd_loss", "emd_loss"}
            assert set(a) == {"cd_loss", "emd_loss", "fscore", "precision", "recall", "hausdorff"}
            assert set(g) == set(a) | {"syn_pc", "ref_pc_q"}
            for key in ("cd_loss", "emd_loss"):
                assert torch.equal(p[key], g[key]) and torch.equal(p[key], a[key]), (graph, key, p[key], g[key])
            want = fscore(g["syn_pc"].contiguous(), g["ref_pc_q"].contiguous(), taus)
            assert tuple(want["fscore"].shape) == (Q, 2)
            for key in ("fscore", "precision", "recall"):
                assert g[key].dtype == torch.float64 and tuple(g[key].shape) == (2,)
                assert torch.equal(g[key], want[key].mean(dim=0)) and torch.equal(a[key], g[key]), (graph, key)
            assert g["hausdorff"].dim() == 0 and g["hausdorff"].dtype == torch.float64
            assert torch.equal(g["hausdorff"], want["hausdorff"].mean()) and torch.equal(a["hausdorff"], g["hausdorff"])
            assert float(g["hausdorff"]) > 0 and (g["precision"][1] >= g["precision"][0]).all()


# ---- 11. the entry point -----------------------------------------------------------------------------------------

def test_entry_point_columns_and_values(gpu, tmp_path, monkeypatch, capsys):
    import evaluate_Network
    from fpsg_amd import cli
    from fpsg_amd.engine import EvalItem
    from fpsg_amd.metrics import fscore
    seen = {}
    inner = EvalItem.__call__

    def spy(self, sample):
        out = inner(self, sample)
        if self.return_clouds:
            seen.setdefault(sample["class"][0], []).append((out["syn_pc"].clone(), out["ref_pc_q"].clone()))
        return out

    monkeypatch.setattr(EvalItem, "__call__", spy)
    argv = ["--synthetic", "--n_shot", "2", "--n_query", "2", "--sequential_eval", "--model_path", str(tmp_path),
            "--name", "x"]
    parser = cli.few_shot_parser(evaluation=True)

    def run(extra):
        torch.manual_seed(0)
        res = evaluate_Network.main(parser.parse_args(argv + extra))
        return res, [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("Class: ")]

    taus = (0.02, 0.05)
    flag = ["--fscore", "0.02", "0.05"]
    res_plain, plain = run([])
    res_flag, flagged = run(flag)
    assert len(res_plain) == 2 and len(res_flag) == 3               # one more element, only with the flag
    assert plain and len(plain) == len(flagged)
    for pl, ln in zip(plain, flagged):
        head, sep, tail = ln.partition("; F@")
        assert sep and head == pl, (pl, ln)                        # cut off the new columns: today's line, every character
        assert "F@" not in pl and "HD" not in pl
        assert [f.split(": ")[0] for f in (sep + tail).split("; ")[1:]] == ["F@0.02", "F@0.05", "HD"], ln
    # every optional column: after Exact EMD, before the set metrics; the values are those of the returned dict
    res, lines = run(["--exact_emd"] + flag + ["--set_metrics", "--jsd"])
    assert len(res) == 6 and len(lines) == len(plain)
    per_class = res[-1]
    assert set(per_class) == set(res[0]) == set(seen)
    for ln in lines:
        name = ln.split(" -- ")[0][len("Class: "):]
        labels = [f.split(": ")[0] for f in ln.split(" -- ")[1].split("; ")]
        assert labels == ["Rec CD", "Rec EMD", "Exact EMD", "F@0.02", "F@0.05", "HD", "MMD-CD", "COV-CD", "1-NNA-CD",
                          "JSD"], ln
        values = {f.split(": ")[0]: float(f.split(": ")[1]) for f in ln.split(" -- ")[1].split("; ")}
        m = per_class[name]
        assert set(m) == {"thresholds", "fscore", "precision", "recall", "hausdorff"}
        assert m["thresholds"] == list(taus)
        assert [values["F@0.02"], values["F@0.05"]] == m["fscore"] and values["HD"] == m["hausdorff"]
        # recomputed from the clouds the items returned: item means, then the mean over the class's items
        items = [fscore(g.contiguous(), r.contiguous(), taus) for g, r in seen[name]]
        for key in ("fscore", "precision", "recall"):
            want = [statistics.mean(it[key].mean(dim=0)[t].item() for it in items) for t in range(len(taus))]
            assert m[key] == want, (name, key, m[key], want)
        assert m["hausdorff"] == statistics.mean(it["hausdorff"].mean().item() for it in items)
        assert all(0.0 <= v <= 1.0 for v in m["fscore"] + m["precision"] + m["recall"]) and m["hausdorff"] > 0
