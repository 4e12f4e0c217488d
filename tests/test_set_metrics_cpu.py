"""Set-level generation metrics (fpsg_amd.set_metrics.from_matrices) against a direct numpy restatement, hand-built
cases, and K13's host side (fpsg_chamfer_cross argument checks, chamfer_matrix's refusals, the evaluation flag) --
no GPU needed."""
import numpy as np
import pytest
import torch

FAKE = 256          # a non-null, aligned pointer value: every call below is refused before anything dereferences it


def _np_metrics(d_gr, d_gg, d_rr):
    """The definitions, one loop at a time (first minimum wins every tie)."""
    G, R = d_gr.shape
    mmd = np.mean([min(d_gr[g, r] for g in range(G)) for r in range(R)])
    matched = set()
    for g in range(G):
        best = 0
        for r in range(1, R):
            if d_gr[g, r] < d_gr[g, best]:
                best = r
        matched.add(best)
    full = np.block([[d_gg, d_gr], [d_gr.T, d_rr]])
    correct = 0
    for i in range(G + R):
        best = None
        for j in range(G + R):
            if j != i and (best is None or full[i, j] < full[i, best]):
                best = j
        correct += (best >= G) == (i >= G)
    return {"mmd_cd": float(mmd), "cov_cd": len(matched) / R, "nna_cd": correct / (G + R)}


def _check(d_gr, d_gg, d_rr):
    from fpsg_amd.set_metrics import from_matrices
    got = from_matrices(torch.from_numpy(d_gr), torch.from_numpy(d_gg), torch.from_numpy(d_rr))
    want = _np_metrics(d_gr, d_gg, d_rr)
    assert set(got) == {"mmd_cd", "cov_cd", "nna_cd"}
    assert all(isinstance(v, float) for v in got.values())
    assert got["mmd_cd"] == pytest.approx(want["mmd_cd"], rel=1e-6)
    assert got["cov_cd"] == want["cov_cd"] and got["nna_cd"] == want["nna_cd"], (got, want)
    return got


def _sym(rng, n, levels=None):
    m = rng.random((n, n)) if levels is None else rng.integers(0, levels, (n, n)).astype(np.float64)
    m = np.triu(m, 1)
    return (m + m.T).astype(np.float32)


@pytest.mark.parametrize("G,R,seed", [(1, 1, 0), (1, 5, 1), (5, 1, 2), (6, 7, 3), (20, 13, 4), (31, 40, 5)])
def test_from_matrices_matches_the_definitions(G, R, seed):
    rng = np.random.default_rng(seed)
    _check(rng.random((G, R)).astype(np.float32), _sym(rng, G), _sym(rng, R))


@pytest.mark.parametrize("seed", range(6))
def test_ties_go_to_the_lowest_index(seed):
    """Values from {0,1,2}: nearly every row has ties, for the argmin of COV and the neighbour of 1-NNA alike."""
    rng = np.random.default_rng(100 + seed)
    G, R = int(rng.integers(2, 9)), int(rng.integers(2, 9))
    _check(rng.integers(0, 3, (G, R)).astype(np.float32), _sym(rng, G, 3), _sym(rng, R, 3))


def test_tie_rules_by_hand():
    from fpsg_amd.set_metrics import from_matrices
    # every g ties on r = 0 and r = 1: the argmin is r = 0 for all -> cov = 1/3
    d_gr = torch.tensor([[1.0, 1.0, 2.0], [1.0, 1.0, 2.0]])
    d_gg = torch.tensor([[0.0, 5.0], [5.0, 0.0]])
    d_rr = torch.tensor([[0.0, 1.0, 9.0], [1.0, 0.0, 9.0], [9.0, 9.0, 0.0]])
    m = from_matrices(d_gr, d_gg, d_rr)
    assert m["cov_cd"] == pytest.approx(1 / 3)
    # order [g0, g1, r0, r1, r2]: g0's nearest others tie at 1.0 (r0, r1) -> r0 wrong; g1 likewise wrong;
    # r0: g0, g1, r1 tie at 1.0 -> g0 (lowest) wrong; r1 likewise -> g0 wrong; r2: g0 at 2.0 -> wrong
    assert m["nna_cd"] == 0.0
    assert m["mmd_cd"] == pytest.approx((1.0 + 1.0 + 2.0) / 3)


def test_identical_sets():
    """G = R: a zero d_gr diagonal -> every reference is matched at distance 0."""
    rng = np.random.default_rng(7)
    n = 9
    d = _sym(rng, n) + 0.1 * (1 - np.eye(n, dtype=np.float32))
    m = _check(d.copy(), d.copy(), d.copy())
    assert m["mmd_cd"] == 0.0 and m["cov_cd"] == 1.0


def test_far_apart_clusters_are_perfectly_separable():
    rng = np.random.default_rng(8)
    G, R = 6, 8
    m = _check((100 + rng.random((G, R))).astype(np.float32), _sym(rng, G), _sym(rng, R))
    assert m["nna_cd"] == 1.0


def test_single_generated_cloud_covers_one_reference():
    rng = np.random.default_rng(9)
    R = 7
    m = _check(rng.random((1, R)).astype(np.float32), np.zeros((1, 1), np.float32), _sym(rng, R))
    assert m["cov_cd"] == pytest.approx(1 / R)


def test_empty_sets_are_refused():
    from fpsg_amd.set_metrics import from_matrices, generation_metrics
    with pytest.raises(ValueError):
        from_matrices(torch.zeros(0, 3), torch.zeros(0, 0), torch.zeros(3, 3))
    with pytest.raises(ValueError):
        from_matrices(torch.zeros(3, 0), torch.zeros(3, 3), torch.zeros(0, 0))
    with pytest.raises(ValueError):
        generation_metrics(torch.zeros(0, 16, 3), torch.rand(2, 16, 3))
    with pytest.raises(ValueError):
        generation_metrics(torch.rand(2, 16, 3), torch.zeros(0, 16, 3))


def test_inconsistent_matrix_shapes_are_refused():
    from fpsg_amd.set_metrics import from_matrices
    with pytest.raises(ValueError, match="inconsistent"):
        from_matrices(torch.zeros(2, 3), torch.zeros(3, 3), torch.zeros(3, 3))


@pytest.fixture(scope="module")
def lib():
    import os
    import __graft_entry__ as g
    from conftest import ROOT
    if not os.path.exists(os.path.join(ROOT, "fpsg_amd", "libfpsg_hip.so")):
        g.build()
    from fpsg_amd import _hip
    return _hip.load()


def _cross(lib, xyz1=FAKE, xyz2=FAKE, Na=2, Nb=3, N=64, M=64, out=FAKE):
    return lib.fpsg_chamfer_cross(xyz1, xyz2, Na, Nb, N, M, out, None)


@pytest.mark.parametrize("name", ["xyz1", "out"])
def test_null_required_pointer(lib, name):
    assert _cross(lib, **{name: None}) == -1
    assert b"null pointer" in lib.fpsg_last_error() and name.encode() in lib.fpsg_last_error()


@pytest.mark.parametrize("Na,Nb,N,M", [(0, 3, 64, 64), (2, 0, 64, 64), (2, 3, 0, 64), (2, 3, 64, -1), (-4, 3, 64, 64)])
def test_non_positive_sizes_are_refused(lib, Na, Nb, N, M):
    assert _cross(lib, Na=Na, Nb=Nb, N=N, M=M) == -2
    assert b"must be positive" in lib.fpsg_last_error()


def test_symmetric_mode_needs_matching_sizes(lib):
    assert _cross(lib, xyz2=None, Na=3, Nb=4) == -2
    assert b"symmetric" in lib.fpsg_last_error()
    assert _cross(lib, xyz2=None, Na=3, Nb=3, N=64, M=65) == -2


@pytest.mark.parametrize("N,M", [(5000, 64), (64, 5000), (4097, 4097)])
def test_clouds_beyond_4096_points_are_refused(lib, N, M):
    assert _cross(lib, N=N, M=M) == -4
    assert b"4096" in lib.fpsg_last_error()


def test_misaligned_pointer_is_refused(lib):
    assert _cross(lib, xyz2=FAKE + 2) == -3


def test_chamfer_matrix_has_no_cpu_fallback():
    from fpsg_amd._hip import FpsgHipError
    from fpsg_amd.metrics import chamfer_matrix
    with pytest.raises(FpsgHipError):
        chamfer_matrix(torch.rand(2, 8, 3), torch.rand(3, 8, 3))
    with pytest.raises(FpsgHipError):
        chamfer_matrix(torch.rand(2, 8, 3))


def test_chamfer_matrix_checks_shapes():
    from fpsg_amd.metrics import chamfer_matrix
    with pytest.raises(ValueError):
        chamfer_matrix(torch.rand(2, 8, 2), torch.rand(3, 8, 3))
    with pytest.raises(ValueError):
        chamfer_matrix(torch.rand(8, 3))
    with pytest.raises(ValueError):
        chamfer_matrix(torch.rand(2, 0, 3))


def test_evaluation_parser_flag():
    from fpsg_amd import cli
    p = cli.few_shot_parser(evaluation=True)
    assert p.parse_args(["--synthetic"]).set_metrics is False
    assert p.parse_args(["--synthetic", "--set_metrics"]).set_metrics is True
