"""K14 (all-pairs exact EMD matrix, fpsg_emd_cross) on the GPU: against the float64 Hungarian solution
(oracle.ref_f64.exact_emd, scipy), against K12 pair by pair (same trajectory), for determinism, slicing and the
symmetric mode, on hard inputs and the round cap, and through the set metrics and the evaluation entry point."""
import math
import os
import subprocess
import sys
import warnings

import numpy as np
import pytest
import torch

from conftest import ROOT, unit_ball_clouds

pytestmark = pytest.mark.gpu


def _exact(p1, p2):
    from oracle.ref_f64 import exact_emd
    return exact_emd(p1, p2)[0]


def _slack(*sets):
    """fp32 rounding of the certificate (as tests/test_emd_exact_gpu.py): N ulps of 4 D."""
    pts = np.concatenate([s.reshape(-1, 3) for s in sets])
    D = float(np.linalg.norm(pts.max(0) - pts.min(0)))
    return sets[0].shape[1] * 4 * max(D, 1e-30) * 2.0 ** -23


def _matrix(A, B=None, **kw):
    from fpsg_amd.metrics import emd_matrix
    cost, info = emd_matrix(A, B, return_info=True, **kw)
    return cost.cpu().numpy(), info["gap"].cpu().numpy(), info["status"].cpu().numpy(), \
        info["rounds"].cpu().numpy(), info["eps"]


def _check_bracket(A, B, cost, gap, status, eps, converged=True):
    N = A.shape[1]
    slack = _slack(A, B)
    for a in range(A.shape[0]):
        for b in range(B.shape[0]):
            ref = _exact(A[a], B[b])
            assert cost[a, b] - gap[a, b] <= ref * (1 + 1e-5) + slack, (a, b, cost[a, b], gap[a, b], ref)
            assert ref <= cost[a, b] * (1 + 1e-6) + 1e-6, (a, b, cost[a, b], ref)
            if converged:
                assert status[a, b] == 0
                assert cost[a, b] - ref <= N * eps + 1e-5 * ref + 1e-6, (a, b, cost[a, b], ref, N * eps)
                assert 0 <= gap[a, b] <= N * eps + slack


def test_against_hungarian(gpu):
    rng = np.random.default_rng(140)
    A = unit_ball_clouds(rng, 3, 256)
    B = unit_ball_clouds(rng, 2, 256)
    cost, gap, status, _, eps = _matrix(torch.from_numpy(A).to(gpu), torch.from_numpy(B).to(gpu))
    _check_bracket(A, B, cost, gap, status, eps)


def test_against_hungarian_n600(gpu):
    """One pair inside emd_cross_kernel<16> (512 < N <= 1024), at a size that fills none of its 16 points per lane."""
    rng = np.random.default_rng(150)
    A = unit_ball_clouds(rng, 1, 600)
    B = unit_ball_clouds(rng, 1, 600)
    cost, gap, status, _, eps = _matrix(torch.from_numpy(A).to(gpu), torch.from_numpy(B).to(gpu))
    _check_bracket(A, B, cost, gap, status, eps)


def _same_as_k12(gpu, A, B, pairs, cost, gap, status, rounds, eps):
    from fpsg_amd.metrics import emd_exact
    for a, b in pairs:
        c12, info = emd_exact(torch.from_numpy(A[a:a + 1]).to(gpu), torch.from_numpy(B[b:b + 1]).to(gpu), eps=eps,
                              return_info=True)
        assert int(info["rounds"][0]) == rounds[a, b], (a, b)
        assert int(info["status"][0]) == status[a, b], (a, b)
        c12, g12 = float(c12[0]), float(info["gap"][0])
        assert abs(cost[a, b] - c12) <= 1e-6 * c12, (a, b, cost[a, b], c12)
        assert abs(gap[a, b] - g12) <= 1e-6 * c12, (a, b, gap[a, b], g12)


@pytest.mark.parametrize("N", [300, 512, 257, 513, 1024, 1025])
def test_same_trajectory_as_k12(gpu, N):
    """Both ends of emd_cross_kernel<8> (257, 512) and <16> (513, 1024) and the first N of <32> (1025); two clouds a
    side at the sizes that only mark a boundary."""
    sets = 3 if N in (300, 512) else 2
    rng = np.random.default_rng(141 + N)
    A = unit_ball_clouds(rng, sets, N)
    B = unit_ball_clouds(rng, sets, N)
    cost, gap, status, rounds, eps = _matrix(torch.from_numpy(A).to(gpu), torch.from_numpy(B).to(gpu))
    assert (rounds > 0).all()
    pairs = [(0, 0), (1, 2), (2, 1), (2, 2)] if sets == 3 else [(0, 0), (0, 1), (1, 0), (1, 1)]
    _same_as_k12(gpu, A, B, pairs, cost, gap, status, rounds, eps)


def test_same_trajectory_as_k12_n2048(gpu):
    rng = np.random.default_rng(142)
    A = unit_ball_clouds(rng, 2, 2048)
    cost, gap, status, rounds, eps = _matrix(torch.from_numpy(A).to(gpu))
    assert status[0, 1] == 0 and rounds[0, 1] > 0
    _same_as_k12(gpu, A, A, [(0, 1)], cost, gap, status, rounds, eps)
    print(f"\nN=2048: rounds {rounds[0, 1]}, gap / (N eps) {gap[0, 1] / (2048 * eps):.3f}")


def test_deterministic_and_slicing(gpu):
    rng = np.random.default_rng(143)
    A = torch.from_numpy(unit_ball_clouds(rng, 5, 256)).to(gpu)
    B = torch.from_numpy(unit_ball_clouds(rng, 4, 256)).to(gpu)
    from fpsg_amd.metrics import emd_exact_default_eps
    eps = emd_exact_default_eps(A, B)
    c1, g1, s1, r1, _ = _matrix(A, B, eps=eps)
    c2, g2, s2, r2, _ = _matrix(A, B, eps=eps)
    assert np.array_equal(c1.view(np.int32), c2.view(np.int32)) and np.array_equal(g1.view(np.int32), g2.view(np.int32))
    assert np.array_equal(s1, s2) and np.array_equal(r1, r2)
    cs, gs, ss, rs, _ = _matrix(A[1:4].contiguous(), B[2:4].contiguous(), eps=eps)
    assert np.array_equal(cs.view(np.int32), c1[1:4, 2:4].view(np.int32))
    assert np.array_equal(gs.view(np.int32), g1[1:4, 2:4].view(np.int32))
    assert np.array_equal(rs, r1[1:4, 2:4]) and np.array_equal(ss, s1[1:4, 2:4])


def test_symmetric_mode(gpu):
    rng = np.random.default_rng(144)
    An = unit_ball_clouds(rng, 5, 256)
    A = torch.from_numpy(An).to(gpu)
    full = _matrix(A, A)
    sym = _matrix(A)
    assert full[4] == sym[4]
    c, g, s, r = sym[:4]
    iu = np.triu_indices(5, 1)
    for x, y in zip((c, g, s, r), full[:4]):
        assert np.array_equal(x[iu].view(np.int32), y[iu].view(np.int32))     # upper triangle: bitwise the full matrix
        assert np.array_equal(x.view(np.int32), x.T.view(np.int32))           # mirrored bitwise
        assert (np.diag(x) == 0).all() and not np.signbit(np.diag(x).astype(np.float32)).any()
    # roles swapped: (B, A).T agrees with (A, B) within the gaps
    Bn = unit_ball_clouds(rng, 3, 256)
    B = torch.from_numpy(Bn).to(gpu)
    from fpsg_amd.metrics import emd_exact_default_eps
    eps = emd_exact_default_eps(A, B)
    cab, gab = _matrix(A, B, eps=eps)[:2]
    cba, gba = _matrix(B, A, eps=eps)[:2]
    slack = _slack(An, Bn)
    assert (cab - gab <= cba.T + slack).all() and (cba.T - gba.T <= cab + slack).all()


def test_hard_inputs(gpu):
    rng = np.random.default_rng(145)
    N = 256
    coincident = np.zeros((1, N, 3), np.float32) + np.float32(0.25)
    dup = np.repeat(unit_ball_clouds(rng, 1, 16), N // 16, axis=1)
    centers = rng.standard_normal((4, 3)).astype(np.float32) * 3
    clustered = (centers[rng.integers(0, 4, N)] + 0.01 * rng.standard_normal((N, 3))).astype(np.float32)[None]
    ball = unit_ball_clouds(rng, 1, N)
    S = np.concatenate([coincident, dup, clustered, ball])
    t = torch.from_numpy(S).to(gpu)
    cost, gap, status, _, eps = _matrix(t, t)
    _check_bracket(S, S, cost, gap, status, eps)
    assert (np.diag(cost) <= N * eps + 1e-6).all()                  # the same cloud in both sets


def test_round_cap(gpu):
    from fpsg_amd.metrics import EmdExactCapWarning
    rng = np.random.default_rng(146)
    A = unit_ball_clouds(rng, 2, 128)
    B = unit_ball_clouds(rng, 1, 128)
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        cost, gap, status, rounds, eps = _matrix(torch.from_numpy(A).to(gpu), torch.from_numpy(B).to(gpu),
                                                 max_rounds=5)
    assert (status == 1).all() and (rounds == 5).all()
    msgs = [str(x.message) for x in w if issubclass(x.category, EmdExactCapWarning)]
    assert msgs and "(0, 0)" in msgs[0] and "(1, 0)" in msgs[0]
    _check_bracket(A, B, cost, gap, status, eps, converged=False)


def test_nan_input_is_bounded(gpu):
    rng = np.random.default_rng(147)
    A = unit_ball_clouds(rng, 2, 128)
    A[1, 5] = np.nan
    t = torch.from_numpy(A).to(gpu)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        _, _, status, rounds, _ = _matrix(t, t, eps=1e-4, max_rounds=2000)     # (the default eps of a NaN set is NaN)
    assert (rounds <= 2000).all()
    assert status[0, 0] == 0


def test_load_balancing(gpu):
    """More pairs than run at once (2048 at N = 128), easy (identical) and hard (clustered) pairs mixed."""
    rng = np.random.default_rng(148)
    N = 128
    A = unit_ball_clouds(rng, 64, N)
    A[::4] = A[0]
    centers = rng.standard_normal((2, 3)).astype(np.float32) * 4
    A[1::8] = centers[rng.integers(0, 2, (8, N))] + 0.02 * rng.standard_normal((8, N, 3)).astype(np.float32)
    B = np.concatenate([A[:8], unit_ball_clouds(rng, 24, N)])
    t, u = torch.from_numpy(A).to(gpu), torch.from_numpy(B).to(gpu)
    cost, gap, status, rounds, eps = _matrix(t, u)
    assert (status == 0).all() and np.isfinite(cost).all() and (gap >= 0).all()
    sample = [(0, 0), (4, 0), (1, 3), (9, 17), (63, 31)]
    for a, b in sample:
        ref = _exact(A[a], B[b])
        assert cost[a, b] - gap[a, b] <= ref * (1 + 1e-5) + _slack(A, B) and ref <= cost[a, b] * (1 + 1e-6) + 1e-6
    _same_as_k12(gpu, A, B, sample[:3], cost, gap, status, rounds, eps)


def test_set_metrics_equal_pairwise_emd_exact(gpu):
    from fpsg_amd.metrics import emd_exact, emd_exact_default_eps
    from fpsg_amd.set_metrics import emd_generation_metrics, from_matrices
    rng = np.random.default_rng(149)
    G = torch.from_numpy(unit_ball_clouds(rng, 4, 128)).to(gpu)
    R = torch.from_numpy(unit_ball_clouds(rng, 3, 128)).to(gpu)
    eps = emd_exact_default_eps(G, R)
    m = emd_generation_metrics(G, R)

    def mat(X, Y, sym):
        c = torch.zeros((X.size(0), Y.size(0)), dtype=torch.float32)
        for a in range(X.size(0)):
            for b in range(Y.size(0)):
                if sym and a == b:
                    continue
                x, y = (X[a], Y[b]) if not sym or a < b else (X[b], Y[a])
                c[a, b] = emd_exact(x[None].contiguous(), y[None].contiguous(), eps=eps)[0].cpu()
        return c / 128
    ref = from_matrices(mat(G, R, False), mat(G, G, True), mat(R, R, True))
    assert m["mmd_emd"] == ref["mmd_cd"] and m["cov_emd"] == ref["cov_cd"] and m["nna_emd"] == ref["nna_cd"]
    assert m["mmd_emd_lower"] <= m["mmd_emd"]
    assert 0 <= m["cov_uncertified"] <= 1 and 0 <= m["nna_uncertified"] <= 1


def _evaluate(tmp_path, extra):
    env = dict(os.environ, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, "evaluate_Network.py", "--synthetic", "--n_shot", "2", "--n_query", "1",
                        "--sequential_eval", "--model_path", str(tmp_path), "--name", "x"] + extra,
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return [ln for ln in r.stdout.splitlines() if ln.startswith("Class: ")]


def test_entry_point_flag(gpu, tmp_path):
    lines = _evaluate(tmp_path, ["--set_metrics_emd"])
    plain = _evaluate(tmp_path, [])
    assert lines and len(lines) == len(plain)
    for ln, pl in zip(lines, plain):
        head, _, rest = ln.partition("; MMD-EMD: ")
        # the prefix has the plain line's fields (an untrained model's weights differ from process to process)
        assert head.split(" -- ")[0] == pl.split(" -- ")[0] and head.count("; ") == pl.count("; "), (ln, pl)
        assert " -- Rec CD: " in head and "; Rec EMD: " in head and "MMD-CD" not in head, ln
        mmd, _, rest = rest.partition("; COV-EMD: ")
        cov, _, rest = rest.partition("; 1-NNA-EMD: ")
        nna, _, unc = rest.partition("; EMD-uncertified: ")
        mmd, cov, nna = float(mmd), float(cov), float(nna)
        assert all(math.isfinite(v) for v in (mmd, cov, nna)), ln
        assert mmd >= 0 and 0 <= cov <= 1 and 0 <= nna <= 1, ln
        if unc:
            c, n = (float(v) for v in unc.split("/"))
            assert 0 < c + n and 0 <= c <= 1 and 0 <= n <= 1, ln
    assert not any("EMD-" in ln and "MMD-EMD" in ln for ln in plain)
