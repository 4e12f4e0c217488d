"""K13 (all-pairs Chamfer matrix, fpsg_chamfer_cross / metrics.chamfer_matrix) on the GPU: against a float64 brute
force and K1, determinism, tiling independence and symmetry (bitwise), hard inputs, the set metrics built on it, the
evaluation item's returned clouds and the --set_metrics entry point."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT, unit_ball_clouds

pytestmark = pytest.mark.gpu


def _brute64(A, B):
    """float64 Chamfer matrix: sum of the two mean nearest squared distances of every pair."""
    A, B = A.astype(np.float64), B.astype(np.float64)
    out = np.empty((A.shape[0], B.shape[0]))
    for a in range(A.shape[0]):
        for b in range(B.shape[0]):
            d = ((A[a][:, None, :] - B[b][None, :, :]) ** 2).sum(-1)
            out[a, b] = d.min(1).mean() + d.min(0).mean()
    return out


def _mat(gpu, A, B=None):
    from fpsg_amd.metrics import chamfer_matrix
    tA = torch.from_numpy(A).to(gpu)
    return chamfer_matrix(tA, None if B is None else torch.from_numpy(B).to(gpu)).cpu().numpy()


@pytest.mark.parametrize("Na,Nb", [(1, 1), (3, 5), (17, 9)])
@pytest.mark.parametrize("N,M", [(1, 1), (7, 7), (64, 64), (1000, 1000), (2047, 2047), (2048, 2048), (4096, 4096),
                                 (7, 1000), (2048, 64), (1, 4096), (4096, 2047)])
def test_against_float64_brute_force(gpu, Na, Nb, N, M):
    if Na * Nb * N * M > 17 * 9 * 2048 * 2048:
        pytest.skip("brute force too slow for the largest shapes; covered at 3 x 5")
    rng = np.random.default_rng(Na * 100003 + Nb * 1009 + N * 7 + M)
    A, B = unit_ball_clouds(rng, Na, N), unit_ball_clouds(rng, Nb, M)
    got = _mat(gpu, A, B)
    assert got.shape == (Na, Nb) and got.dtype == np.float32
    want = _brute64(A, B)
    assert np.all(np.abs(got - want) <= 1e-5 * np.abs(want) + 1e-30), np.abs(got - want).max()


def test_every_entry_matches_k1(gpu):
    from fpsg_amd.metrics import chamfer_distance, chamfer_matrix
    rng = np.random.default_rng(11)
    A = torch.from_numpy(unit_ball_clouds(rng, 12, 2048)).to(gpu)
    B = torch.from_numpy(unit_ball_clouds(rng, 10, 2048)).to(gpu)
    got = chamfer_matrix(A, B).cpu().numpy()
    pa = A.repeat_interleave(10, 0).contiguous()
    pb = B.repeat(12, 1, 1).contiguous()
    want = chamfer_distance(pa, pb).reshape(12, 10).cpu().numpy()
    assert np.all(np.abs(got - want) <= 2e-6 * np.abs(want)), np.abs(got / want - 1).max()


def test_per_point_minima_are_k1s(gpu):
    """The row and column sums of a pair are sums of K1's dist1 / dist2 bit patterns: on clouds whose minima are
    all exactly representable powers of two the two sums are exact, so K13 equals K1's mean exactly."""
    from fpsg_amd.metrics import chamfer_distance, chamfer_matrix
    g = torch.Generator().manual_seed(5)
    A = (torch.randint(-64, 64, (2, 512, 3), generator=g).float() / 8).to(gpu)
    B = (A + 0.125).contiguous()
    got = chamfer_matrix(A, B).cpu()
    want = chamfer_distance(A, B).cpu()
    assert torch.equal(got.diagonal(), want)


def test_repeated_calls_and_slices_are_bitwise_identical(gpu):
    from fpsg_amd.metrics import chamfer_matrix
    rng = np.random.default_rng(12)
    A = torch.from_numpy(unit_ball_clouds(rng, 300, 256)).to(gpu)
    B = torch.from_numpy(unit_ball_clouds(rng, 7, 300)).to(gpu)
    m = chamfer_matrix(A, B)
    for _ in range(3):
        assert torch.equal(chamfer_matrix(A, B), m)
    rows = torch.cat([chamfer_matrix(A[i:i + 37].contiguous(), B) for i in range(0, 300, 37)])
    assert torch.equal(rows, m)
    cols = torch.cat([chamfer_matrix(A, B[j:j + 2].contiguous()) for j in range(0, 7, 2)], dim=1)
    assert torch.equal(cols, m)
    single = torch.stack([chamfer_matrix(A[i:i + 1], B[j:j + 1])[0, 0] for i in (0, 151, 299) for j in (0, 6)])
    assert torch.equal(single, m[[0, 0, 151, 151, 299, 299], [0, 6, 0, 6, 0, 6]])


@pytest.mark.parametrize("Na,N", [(1, 5), (9, 100), (40, 2048), (5, 4096)])
def test_symmetric_mode(gpu, Na, N):
    from fpsg_amd.metrics import chamfer_matrix
    rng = np.random.default_rng(Na + N)
    A = torch.from_numpy(unit_ball_clouds(rng, Na, N)).to(gpu)
    s = chamfer_matrix(A)
    assert torch.equal(s, s.t())
    assert torch.equal(s.diagonal(), torch.zeros(Na, device=gpu))
    assert torch.equal(s, chamfer_matrix(A, A))
    assert not s.requires_grad


@pytest.mark.parametrize("N,M", [(2048, 2048), (100, 3000), (4096, 512)])
def test_transpose_is_bitwise(gpu, N, M):
    from fpsg_amd.metrics import chamfer_matrix
    rng = np.random.default_rng(N + 3 * M)
    A = torch.from_numpy(unit_ball_clouds(rng, 6, N)).to(gpu)
    B = torch.from_numpy(unit_ball_clouds(rng, 5, M)).to(gpu)
    assert torch.equal(chamfer_matrix(B, A), chamfer_matrix(A, B).t())


def test_hard_inputs(gpu):
    rng = np.random.default_rng(13)
    A = unit_ball_clouds(rng, 4, 300)
    dup = np.concatenate([A[:, :150], A[:, :150]], axis=1)                     # every point twice
    same = np.repeat(rng.random((4, 1, 3)).astype(np.float32), 300, axis=1)     # all points coincident
    far = (A + np.float32(1e3)).astype(np.float32)                              # translated by 1e3
    for X, Y in [(dup, A), (same, A), (same, same), (far, far[::-1].copy()), (far, dup + np.float32(1e3))]:
        got = _mat(gpu, X, Y)
        want = _brute64(X, Y)
        assert np.all(np.abs(got - want) <= 1e-5 * np.abs(want) + 1e-30), (np.abs(got - want).max(), want.max())
    s = _mat(gpu, same)
    assert np.all(np.diag(s) == 0) and np.array_equal(s, s.T)


def test_grid_beyond_65535_workgroups(gpu):
    """4100 x 300 pairs of 4-point clouds: 1.23M pairs at 16 per workgroup = 76875 workgroups on the grid's one axis
    (8.4M pairs, 525k workgroups in the symmetric mode)."""
    rng = np.random.default_rng(14)
    A = rng.random((4100, 4, 3)).astype(np.float32)
    B = rng.random((300, 4, 3)).astype(np.float32)
    got = _mat(gpu, A, B)
    want = np.empty((4100, 300))
    for i in range(0, 4100, 500):
        d = ((A[i:i + 500].astype(np.float64)[:, None, :, None, :] - B.astype(np.float64)[None, :, None, :, :]) ** 2)
        d = d.sum(-1)
        want[i:i + 500] = d.min(3).mean(2) + d.min(2).mean(2)
    assert np.all(np.abs(got - want) <= 1e-5 * want + 1e-12)
    s = _mat(gpu, A)
    assert np.array_equal(s, s.T) and np.all(np.diag(s) == 0)


def test_generation_metrics_equal_pairwise_k1_matrices(gpu):
    from fpsg_amd.metrics import chamfer_distance
    from fpsg_amd.set_metrics import from_matrices, generation_metrics
    rng = np.random.default_rng(15)
    gen = torch.from_numpy(unit_ball_clouds(rng, 6, 512)).to(gpu)
    ref = torch.from_numpy(unit_ball_clouds(rng, 7, 512)).to(gpu)

    def k1(X, Y):
        return torch.stack([torch.cat([chamfer_distance(X[i:i + 1], Y[j:j + 1]) for j in range(Y.size(0))])
                            for i in range(X.size(0))])
    got = generation_metrics(gen, ref)
    want = from_matrices(k1(gen, ref), k1(gen, gen), k1(ref, ref))
    assert got["mmd_cd"] == pytest.approx(want["mmd_cd"], rel=2e-6)
    assert got["cov_cd"] == want["cov_cd"] and got["nna_cd"] == want["nna_cd"]
    assert 0 < got["cov_cd"] <= 1 and 0 <= got["nna_cd"] <= 1


def test_evaluation_item_returns_cloned_clouds(gpu):
    """EvalItem(return_clouds=True): the clouds collected over eager and graph-replayed items equal, item for item, the
    plain method's -- a returned static graph buffer would hold only the last replay's clouds."""
    from fpsg_amd.engine import EvalItem, build_model, default_options
    from fpsg_amd.episodes import synthetic_episode
    torch.manual_seed(3)
    model = build_model(default_options(device="cuda")).to(gpu).eval()
    S, Q = 2, 2
    grids = model.pc_decoder.sample_grids(Q, gpu, torch.Generator(device=gpu).manual_seed(9))
    orig = model.pc_decoder.forward
    model.pc_decoder.forward = lambda h, grid=None, generator=None, pack=None: orig(h, grid=grids, pack=pack)
    eps = [synthetic_episode(S, Q, n_pts=2048, img_size=96, seed=70 + i, device=gpu) for i in range(5)]
    with EvalItem(model) as item:
        plain = [item(ep) for ep in eps]
    with EvalItem(model, return_clouds=True) as item:
        got = [item(ep) for ep in eps]
        assert item._graphs, "the third item of a shape must have been captured"
    with torch.no_grad():
        ref = [model._return_reconstruction(ep, return_clouds=True) for ep in eps]
    for p, g, r in zip(plain, got, ref):
        assert set(g) == {"cd_loss", "emd_loss", "syn_pc", "ref_pc_q"}
        for key in ("cd_loss", "emd_loss"):
            assert abs(float(p[key]) - float(g[key])) <= 1e-6 * abs(float(p[key]))
        assert torch.allclose(g["syn_pc"], r["syn_pc"], rtol=1e-5, atol=1e-6)
        assert torch.equal(g["ref_pc_q"], r["ref_pc_q"])
    # the replayed items differ from each other: a shared buffer would make them all equal to the last one
    assert not torch.equal(got[2]["syn_pc"], got[4]["syn_pc"])


def _evaluate(tmp_path, extra):
    env = dict(os.environ, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, "evaluate_Network.py", "--synthetic", "--n_shot", "2", "--n_query", "1",
                        "--sequential_eval", "--model_path", str(tmp_path), "--name", "x"] + extra,
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return [ln for ln in r.stdout.splitlines() if ln.startswith("Class: ")]


def test_entry_point_flag(gpu, tmp_path):
    fields = ("; MMD-CD: ", "; COV-CD: ", "; 1-NNA-CD: ")
    lines = _evaluate(tmp_path, ["--set_metrics"])
    assert lines
    for ln in lines:
        head, _, rest = ln.partition(fields[0])
        assert " -- Rec CD: " in head and "; Rec EMD: " in head, ln
        mmd, _, rest = rest.partition(fields[1])
        cov, _, nna = rest.partition(fields[2])
        mmd, cov, nna = float(mmd), float(cov), float(nna)
        assert all(math.isfinite(v) for v in (mmd, cov, nna)), ln
        assert mmd >= 0 and 0 <= cov <= 1 and 0 <= nna <= 1, ln
    plain = _evaluate(tmp_path, [])
    assert plain and not any(f.strip("; ") in ln for ln in plain for f in fields)
    assert [ln.split(" -- ")[0] for ln in lines] == [ln.split(" -- ")[0] for ln in plain]
