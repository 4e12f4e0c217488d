"""K12 (exact EMD by a bounded auction, fpsg_emd_exact) on the GPU against the float64 Hungarian solution
(oracle.ref_f64.exact_emd, scipy), on inputs that stress the auction, and through the evaluation entry point."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT, unit_ball_clouds

pytestmark = pytest.mark.gpu


def _exact(p1, p2):
    from oracle.ref_f64 import exact_emd
    return exact_emd(p1, p2)[0]


def _dist64(p1, p2, assign):
    """float64 sum of |p1_i - p2_assign(i)| per pair."""
    a = np.asarray(assign, np.int64)
    d = p1.astype(np.float64) - np.take_along_axis(p2.astype(np.float64), a[..., None], axis=1)
    return np.sqrt((d ** 2).sum(-1)).sum(-1)


def _run(gpu, p1, p2, **kw):
    from fpsg_amd.metrics import emd_exact
    t1, t2 = torch.from_numpy(p1).to(gpu), torch.from_numpy(p2).to(gpu)
    cost, info = emd_exact(t1, t2, return_info=True, **kw)
    return (cost.cpu().numpy(), info["gap"].cpu().numpy(), info["assign"].cpu().numpy(), info["status"].cpu().numpy(),
            info["eps"], info["rounds"].cpu().numpy())


def _gap_slack(p1, p2):
    """fp32 rounding of the certificate: every term (c + p) - min(c + p) is exact up to an ulp of the values, which are
    at most the prices plus one cost (each below ~2 x the bounding-box diagonal D): N ulps of 4 D."""
    pts = np.concatenate([p1.reshape(-1, 3), p2.reshape(-1, 3)])
    D = float(np.linalg.norm(pts.max(0) - pts.min(0)))
    return p1.shape[1] * 4 * max(D, 1e-30) * 2.0 ** -23


def _check_exact(p1, p2, cost, gap, assign, status, eps):
    B, N, _ = p1.shape
    assert (status == 0).all(), status
    for b in range(B):
        assert np.array_equal(np.sort(assign[b]), np.arange(N)), "assign is not a permutation"
    along = _dist64(p1, p2, assign)
    np.testing.assert_allclose(cost, along, rtol=1e-5, atol=1e-6)
    slack = _gap_slack(p1, p2)
    for b in range(B):
        exact = _exact(p1[b], p2[b])
        assert exact <= cost[b] * (1 + 1e-6) + 1e-6, (b, exact, cost[b])
        assert cost[b] <= exact + N * eps + 1e-5 * exact + 1e-6, (b, exact, cost[b], N * eps)
        assert 0 <= gap[b] <= N * eps + slack, (b, gap[b], N * eps, slack)
        assert cost[b] - gap[b] <= exact * (1 + 1e-5) + slack, (b, cost[b], gap[b], exact)   # the certificate holds


@pytest.mark.parametrize("B,N", [(1, 1), (2, 2), (3, 7), (4, 128), (2, 512), (2, 2048), (5, 2048)])
def test_exact_against_hungarian(gpu, B, N):
    rng = np.random.default_rng(1000 * B + N)
    p1, p2 = unit_ball_clouds(rng, B, N), unit_ball_clouds(rng, B, N)
    cost, gap, assign, status, eps, rounds = _run(gpu, p1, p2)
    print(f"emd_exact B={B} N={N}: rounds {rounds.tolist()}, gap/(N eps) {(gap / (N * eps)).round(3).tolist()}")
    _check_exact(p1, p2, cost, gap, assign, status, eps)


def test_permuted_copy_is_recovered(gpu):
    rng = np.random.default_rng(5)
    p1 = unit_ball_clouds(rng, 1, 2048)
    perm = rng.permutation(2048)
    p2 = np.ascontiguousarray(p1[:, perm])                 # p2[k] = p1[perm[k]]: x_i goes to y_argsort(perm)[i]
    cost, gap, assign, status, eps, _ = _run(gpu, p1, p2)
    assert status[0] == 0
    assert cost[0] <= 2048 * eps
    assert np.array_equal(assign[0], np.argsort(perm))


def test_identical_clouds(gpu):
    rng = np.random.default_rng(6)
    p1 = unit_ball_clouds(rng, 2, 1024)
    cost, gap, assign, status, eps, _ = _run(gpu, p1, p1.copy())
    assert (status == 0).all() and (cost <= 1024 * eps).all() and (gap >= 0).all()
    for b in range(2):
        assert np.array_equal(np.sort(assign[b]), np.arange(1024))
    print(f"identical clouds: {(assign == np.arange(1024)).mean():.4f} of the points matched to themselves")


def test_all_points_coincident(gpu):
    """Every cost 0, every bid tied: returns converged, well within the cap."""
    p = np.full((2, 2048, 3), 0.25, np.float32)
    cost, gap, assign, status, eps, rounds = _run(gpu, p, p.copy(), eps=1e-6, max_rounds=4096)
    assert (status == 0).all() and (cost == 0).all() and (gap == 0).all()
    for b in range(2):
        assert np.array_equal(np.sort(assign[b]), np.arange(2048))
    assert (rounds < 4096).all(), rounds


def test_two_far_apart_clusters(gpu):
    """60 % of one cloud and 40 % of the other around x = -10, the rest around x = +10: a fifth of the points must
    cross, and the prices climb from 0 to ~20 before they do."""
    rng = np.random.default_rng(7)
    N = 1024
    base = unit_ball_clouds(rng, 2, N) * 0.5
    p1, p2 = base[:1].copy(), base[1:].copy()
    p1[0, :int(0.6 * N), 0] -= 10; p1[0, int(0.6 * N):, 0] += 10
    p2[0, :int(0.4 * N), 0] -= 10; p2[0, int(0.4 * N):, 0] += 10
    cost, gap, assign, status, eps, rounds = _run(gpu, p1, p2)
    print(f"two clusters: rounds {rounds.tolist()}")
    _check_exact(p1, p2, cost, gap, assign, status, eps)


def test_heavy_duplicates(gpu):
    """2048 points drawn from 16 distinct positions in each cloud (128-fold ties in every row and column)."""
    rng = np.random.default_rng(8)
    pos1, pos2 = unit_ball_clouds(rng, 1, 16)[0], unit_ball_clouds(rng, 1, 16)[0]
    p1 = pos1[rng.integers(0, 16, 2048)][None].astype(np.float32)
    p2 = pos2[rng.integers(0, 16, 2048)][None].astype(np.float32)
    cost, gap, assign, status, eps, rounds = _run(gpu, p1, p2)
    print(f"duplicates: rounds {rounds.tolist()}")
    _check_exact(p1, p2, cost, gap, assign, status, eps)


def test_round_cap_returns_promptly_and_warns(gpu):
    from fpsg_amd.metrics import EmdExactCapWarning, emd_exact
    rng = np.random.default_rng(9)
    p1, p2 = unit_ball_clouds(rng, 1, 512), unit_ball_clouds(rng, 1, 512)
    t1, t2 = torch.from_numpy(p1).to(gpu), torch.from_numpy(p2).to(gpu)
    with pytest.warns(EmdExactCapWarning, match="round cap"):
        cost, info = emd_exact(t1, t2, max_rounds=1, return_info=True)
    assert int(info["status"][0]) == 1 and int(info["rounds"][0]) == 1
    a = info["assign"].cpu().numpy()
    assert np.array_equal(np.sort(a[0]), np.arange(512))           # still a permutation ...
    c, g = float(cost[0]), float(info["gap"][0])
    assert c == pytest.approx(_dist64(p1, p2, a)[0], rel=1e-5)
    exact = _exact(p1[0], p2[0])
    assert c - g <= exact * (1 + 1e-5) <= c * (1 + 2e-5)            # ... bracketed by its certificate


def test_bit_identical_across_calls(gpu):
    from fpsg_amd.metrics import emd_exact
    rng = np.random.default_rng(10)
    p1, p2 = unit_ball_clouds(rng, 3, 2048), unit_ball_clouds(rng, 3, 2048)
    outs = []
    for _ in range(2):
        t1 = torch.from_numpy(p1).to(gpu).requires_grad_()
        t2 = torch.from_numpy(p2).to(gpu).requires_grad_()
        cost, info = emd_exact(t1, t2, return_info=True)
        cost.sum().backward()
        outs.append([x.detach().cpu().numpy() for x in (cost, info["gap"], info["assign"], t1.grad, t2.grad)])
    for a, b in zip(*outs):
        assert np.array_equal(a, b)


def test_gradients_match_the_unit_vector_formula(gpu):
    from fpsg_amd.metrics import emd_exact
    rng = np.random.default_rng(11)
    p1, p2 = unit_ball_clouds(rng, 2, 2048), unit_ball_clouds(rng, 2, 2048)
    p2[:, :100] = p1[:, :100]                            # coincident pairs: their matched distance is 0
    t1 = torch.from_numpy(p1).to(gpu).requires_grad_()
    t2 = torch.from_numpy(p2).to(gpu).requires_grad_()
    w = torch.tensor([1.0, -2.5], device=gpu)
    cost, info = emd_exact(t1, t2, return_info=True)
    (cost * w).sum().backward()
    a = info["assign"].cpu().numpy().astype(np.int64)
    d = p1.astype(np.float64) - np.take_along_axis(p2.astype(np.float64), a[..., None], axis=1)
    n = np.sqrt((d ** 2).sum(-1, keepdims=True))
    u = np.where(n > 0, d / np.where(n > 0, n, 1), 0.0) * np.array([1.0, -2.5])[:, None, None]
    g2 = np.zeros_like(u)
    np.put_along_axis(g2, np.repeat(a[..., None], 3, axis=2), -u, axis=1)
    assert np.abs(t1.grad.cpu().numpy() - u).max() <= 1e-5
    assert np.abs(t2.grad.cpu().numpy() - g2).max() <= 1e-5
    zero = n[..., 0] == 0
    assert zero[:, :100].all()                           # the coincident points matched to each other ...
    assert (t1.grad.cpu().numpy()[zero] == 0).all()      # ... and their gradient is 0


def test_not_above_the_approximate_assignment(gpu):
    """K2's soft assignment is a transport plan too: the exact optimum is at most its cost."""
    from fpsg_amd.metrics import emd_approx, emd_exact
    rng = np.random.default_rng(12)
    p1, p2 = unit_ball_clouds(rng, 4, 2048), unit_ball_clouds(rng, 4, 2048)
    t1, t2 = torch.from_numpy(p1).to(gpu), torch.from_numpy(p2).to(gpu)
    ex, ap = emd_exact(t1, t2).cpu().numpy(), emd_approx(t1, t2).cpu().numpy()
    print(f"exact / approx: {(ex / ap).round(4).tolist()}")
    assert (ex <= ap * (1 + 1e-5)).all(), (ex, ap)


def test_evaluation_item_exact_emd_is_computed_on_the_replayed_clouds(gpu):
    """EvalItem(exact_emd=True): the eager items and the graph replays return the exact EMD of the same clouds the
    plain method generates, and the two reference metrics unchanged."""
    from fpsg_amd.engine import EvalItem, build_model, default_options
    from fpsg_amd.episodes import synthetic_episode
    from fpsg_amd.metrics import emd_exact
    torch.manual_seed(3)
    model = build_model(default_options(device="cuda")).to(gpu).eval()
    S, Q = 2, 2
    grids = model.pc_decoder.sample_grids(Q, gpu, torch.Generator(device=gpu).manual_seed(9))
    orig = model.pc_decoder.forward
    model.pc_decoder.forward = lambda h, grid=None, generator=None, pack=None: orig(h, grid=grids, pack=pack)
    eps = [synthetic_episode(S, Q, n_pts=2048, img_size=96, seed=60 + i, device=gpu) for i in range(4)]
    with EvalItem(model) as item:
        plain = [item(ep) for ep in eps]
    with EvalItem(model, exact_emd=True) as item:
        got = [item(ep) for ep in eps]
        assert item._graphs, "the third item of a shape must have been captured"
    with torch.no_grad():
        ref = [model._return_reconstruction(ep, return_clouds=True) for ep in eps]
    for p, g, r in zip(plain, got, ref):
        assert set(g) == {"cd_loss", "emd_loss", "exact_emd"}
        for key in ("cd_loss", "emd_loss"):
            assert abs(float(p[key]) - float(g[key])) <= 1e-6 * abs(float(p[key]))
        want = float(emd_exact(r["syn_pc"].contiguous(), r["ref_pc_q"].contiguous()).sum())
        assert math.isfinite(want) and want > 0
        assert abs(float(g["exact_emd"]) - want) <= 1e-5 * want, (float(g["exact_emd"]), want)


def _evaluate(tmp_path, extra):
    env = dict(os.environ, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, "evaluate_Network.py", "--synthetic", "--n_shot", "2", "--n_query", "1",
                        "--sequential_eval", "--model_path", str(tmp_path), "--name", "x"] + extra,
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return [ln for ln in r.stdout.splitlines() if ln.startswith("Class: ")]


def test_entry_point_flag(gpu, tmp_path):
    lines = _evaluate(tmp_path, ["--exact_emd"])
    assert lines
    for ln in lines:
        head, _, val = ln.partition("; Exact EMD: ")
        assert " -- Rec CD: " in head and "; Rec EMD: " in head, ln
        assert math.isfinite(float(val)) and float(val) > 0, ln
    plain = _evaluate(tmp_path, [])
    assert plain and not any("Exact EMD" in ln for ln in plain)
    assert [ln.partition("; Exact EMD: ")[0].split(" -- ")[0] for ln in lines] == [ln.split(" -- ")[0] for ln in plain]
