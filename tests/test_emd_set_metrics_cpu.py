"""The set-level generation metrics under the exact EMD (fpsg_amd.set_metrics: emd_from_matrices, certify_nearest)
on hand-built cost and gap matrices against a direct restatement, the argument checks of emd_matrix and
emd_generation_metrics that answer before any launch, and the --set_metrics_emd flag."""
import itertools

import pytest
import torch

from fpsg_amd import cli
from fpsg_amd.metrics import emd_matrix
from fpsg_amd.set_metrics import certify_nearest, emd_from_matrices, emd_generation_metrics


def _sym(n, g):
    m = torch.rand((n, n), generator=g) * 10 + 1
    m = (m + m.t()) / 2
    m.fill_diagonal_(0)
    return m


def _restated(c_gr, g_gr, c_gg, g_gg, c_rr, g_rr, n):
    """Direct restatement: nested loops, first minimum wins, certification by definition."""
    G, R = c_gr.shape
    d = c_gr.tolist()
    mmd = sum(min(d[g][r] / n for g in range(G)) for r in range(R)) / R
    mmd_low = sum(min((d[g][r] - g_gr[g][r].item()) / n for g in range(G)) for r in range(R)) / R
    nearest = []
    cov_unc = 0
    for g in range(G):
        best = min(range(R), key=lambda r: (d[g][r] / n, r))
        nearest.append(best)
        if any(not (d[g][best] < d[g][r] - g_gr[g][r].item()) for r in range(R) if r != best):
            cov_unc += 1
    cov = len(set(nearest)) / R
    C = [[0.0] * (G + R) for _ in range(G + R)]
    P = [[0.0] * (G + R) for _ in range(G + R)]
    for i, j in itertools.product(range(G + R), repeat=2):
        if i < G and j < G:
            C[i][j], P[i][j] = c_gg[i][j].item(), g_gg[i][j].item()
        elif i < G:
            C[i][j], P[i][j] = d[i][j - G], g_gr[i][j - G].item()
        elif j < G:
            C[i][j], P[i][j] = d[j][i - G], g_gr[j][i - G].item()
        else:
            C[i][j], P[i][j] = c_rr[i - G][j - G].item(), g_rr[i - G][j - G].item()
    correct = 0
    nna_unc = 0
    for i in range(G + R):
        cand = [j for j in range(G + R) if j != i]
        best = min(cand, key=lambda j: (C[i][j] / n, j))
        correct += (best < G) == (i < G)
        if any(not (C[i][best] < C[i][j] - P[i][j]) for j in cand if j != best):
            nna_unc += 1
    return {"mmd_emd": mmd, "cov_emd": cov, "nna_emd": correct / (G + R), "mmd_emd_lower": mmd_low,
            "cov_uncertified": cov_unc / G, "nna_uncertified": nna_unc / (G + R)}


@pytest.mark.parametrize("G,R,n", [(5, 4, 256), (1, 3, 2048), (4, 1, 100), (1, 1, 7), (6, 6, 512)])
def test_against_restatement(G, R, n):
    g = torch.Generator().manual_seed(G * 100 + R * 10 + n)
    c_gr = (torch.rand((G, R), generator=g) * 10 + 1).double().float()
    g_gr = torch.rand((G, R), generator=g) * 0.5
    c_gg, c_rr = _sym(G, g), _sym(R, g)
    g_gg, g_rr = torch.rand((G, G), generator=g) * 0.5, torch.rand((R, R), generator=g) * 0.5
    got = emd_from_matrices(c_gr, g_gr, c_gg, g_gg, c_rr, g_rr, n)
    want = _restated(c_gr, g_gr, c_gg, g_gg, c_rr, g_rr, n)
    assert set(got) == set(want)
    for k in want:
        assert got[k] == pytest.approx(want[k], rel=1e-6, abs=1e-9), k


def test_ties_go_to_the_first_and_are_uncertified():
    c_gr = torch.tensor([[2.0, 2.0, 3.0], [5.0, 1.0, 1.0]])
    z = torch.zeros_like(c_gr)
    c_gg = torch.tensor([[0.0, 9.0], [9.0, 0.0]])
    c_rr = torch.tensor([[0.0, 9.0, 9.0], [9.0, 0.0, 9.0], [9.0, 9.0, 0.0]])
    m = emd_from_matrices(c_gr, z, c_gg, torch.zeros(2, 2), c_rr, torch.zeros(3, 3), 4)
    assert m["cov_emd"] == pytest.approx(2 / 3)                  # nearest: r0 and r1 (first of each tie)
    assert m["mmd_emd"] == pytest.approx((2 + 1 + 1) / 3 / 4)
    assert m["cov_uncertified"] == 1.0                            # exact ties, zero gaps: still uncertified
    want = _restated(c_gr, z, c_gg, torch.zeros(2, 2), c_rr, torch.zeros(3, 3), 4)
    for k in want:
        assert m[k] == pytest.approx(want[k]), k


def test_certification_cases():
    cost = torch.tensor([[1.0, 2.0, 3.0],      # separated: 1 < 2 - 0.5 and 1 < 3 - 0.5
                         [1.0, 1.2, 3.0],      # overlap: 1.0 is not below 1.2 - 0.5
                         [1.0, 1.0, 3.0],      # exact tie, zero gap
                         [1.0, 1.5, 3.0]])     # touching: 1.0 == 1.5 - 0.5 is not strictly below
    gap = torch.tensor([[0.9, 0.5, 0.5],
                        [0.0, 0.5, 0.5],
                        [0.0, 0.0, 0.0],
                        [0.0, 0.5, 0.5]])
    assert certify_nearest(cost, gap).tolist() == [True, False, False, False]
    # the chosen entry's own gap does not matter, only its upper bound; a single candidate is certified
    assert certify_nearest(torch.tensor([[4.0]]), torch.tensor([[4.0]])).tolist() == [True]
    sq = torch.tensor([[0.0, 1.0, 5.0], [1.0, 0.0, 1.05], [5.0, 1.05, 0.0]])
    gsq = torch.full((3, 3), 0.1)
    # self excluded: row 0 -> 1 (1 < 5 - 0.1), row 1 -> 0 (1 vs 1.05 - 0.1: overlap), row 2 -> 1 (1.05 < 5 - 0.1)
    assert certify_nearest(sq, gsq, exclude_self=True).tolist() == [True, False, True]
    with pytest.raises(ValueError):
        certify_nearest(torch.zeros(2, 3), torch.zeros(2, 3), exclude_self=True)
    with pytest.raises(ValueError):
        certify_nearest(torch.zeros(2, 3), torch.zeros(3, 2))


def test_lower_mmd_brackets():
    c_gr = torch.tensor([[4.0, 6.0], [5.0, 3.0]])
    g_gr = torch.tensor([[1.0, 0.5], [3.0, 0.25]])
    z2 = torch.zeros(2, 2)
    m = emd_from_matrices(c_gr, g_gr, z2 + 9 - torch.eye(2) * 9, z2, z2 + 9 - torch.eye(2) * 9, z2, 2)
    assert m["mmd_emd"] == pytest.approx((4 + 3) / 2 / 2)
    assert m["mmd_emd_lower"] == pytest.approx((2 + 2.75) / 2 / 2)    # min(4-1, 5-3) = 2; min(6-.5, 3-.25) = 2.75


def test_emd_matrix_argument_errors():
    a = torch.zeros((2, 16, 3))
    with pytest.raises(ValueError, match="equal size"):
        emd_matrix(a, torch.zeros((2, 8, 3)))
    with pytest.raises(ValueError, match="2048"):
        emd_matrix(torch.zeros((1, 2049, 3)))
    with pytest.raises(ValueError, match="empty"):
        emd_matrix(torch.zeros((0, 16, 3)), a)
    with pytest.raises(ValueError, match="empty"):
        emd_matrix(a, torch.zeros((0, 16, 3)))
    with pytest.raises(ValueError, match="expected"):
        emd_matrix(torch.zeros((2, 16, 2)))
    with pytest.raises(ValueError, match="expected"):
        emd_matrix(torch.zeros((16, 3)), a)
    with pytest.raises(ValueError, match="max_rounds"):
        emd_matrix(a, a, max_rounds=0)
    with pytest.raises(ValueError, match="eps"):
        emd_matrix(a, a, eps=0.0)
    with pytest.raises(ValueError, match="eps"):
        emd_matrix(a, a, eps=float("nan"))


def test_emd_generation_metrics_argument_errors():
    a = torch.zeros((2, 16, 3))
    with pytest.raises(ValueError, match="at least one"):
        emd_generation_metrics(torch.zeros((0, 16, 3)), a)
    with pytest.raises(ValueError, match="at least one"):
        emd_generation_metrics(a, torch.zeros((0, 16, 3)))
    with pytest.raises(ValueError, match="equal size"):
        emd_generation_metrics(a, torch.zeros((2, 8, 3)))
    with pytest.raises(ValueError, match="2048"):
        emd_generation_metrics(torch.zeros((1, 2049, 3)), torch.zeros((1, 2049, 3)))
    with pytest.raises(ValueError, match="expected"):
        emd_generation_metrics(torch.zeros((2, 16)), a)


def test_emd_cross_host_checks():
    """fpsg_emd_cross refuses bad arguments on the host, before any HIP call."""
    import ctypes
    from fpsg_amd import _hip
    lib = _hip.load()
    fake = ctypes.c_void_p(4096)
    assert lib.fpsg_emd_cross_workspace_bytes(2, 2, 2049) == 0
    ws = lib.fpsg_emd_cross_workspace_bytes(2, 3, 64)
    assert ws >= 8

    def call(x1=fake, x2=fake, Na=2, Nb=3, N=64, eps=1e-3, mr=10, c=fake, g=fake, s=fake, r=None, w=fake, wb=ws):
        return lib.fpsg_emd_cross(x1, x2, Na, Nb, N, eps, mr, c, g, s, r, w, wb, None)
    for kw, code in [({"x1": None}, -1), ({"c": None}, -1), ({"g": None}, -1), ({"s": None}, -1), ({"w": None}, -1),
                     ({"Na": 0}, -2), ({"N": 0}, -2), ({"N": 2049}, -4), ({"eps": 0.0}, -2),
                     ({"eps": float("inf")}, -2), ({"eps": float("nan")}, -2), ({"mr": 0}, -2), ({"wb": 0}, -2),
                     ({"x2": None, "Nb": 3}, -2), ({"x2": ctypes.c_void_p(4098)}, -3),
                     ({"w": ctypes.c_void_p(4100)}, -3)]:
        assert call(**kw) == code, kw
        assert lib.fpsg_last_error().startswith(b"fpsg_emd_cross"), kw


def test_cli_flag():
    p = cli.few_shot_parser(evaluation=True)
    assert p.parse_args(["--set_metrics_emd"]).set_metrics_emd is True
    base = vars(p.parse_args([]))
    assert base["set_metrics_emd"] is False
    assert {k: v for k, v in base.items() if k != "set_metrics_emd"} == \
        {k: v for k, v in vars(p.parse_args(["--set_metrics_emd"])).items() if k != "set_metrics_emd"}
    assert "set_metrics_emd" not in vars(cli.few_shot_parser().parse_args([]))
