"""K12 (exact EMD, fpsg_emd_exact) on the host: argument checks answer before any launch, the workspace size, and the
Python wrapper's refusals -- no GPU needed."""
import ctypes

import pytest

FAKE = 256          # a non-null, aligned pointer value: every call below is refused before anything dereferences it


@pytest.fixture(scope="module")
def lib():
    import os
    import __graft_entry__ as g
    from conftest import ROOT
    if not os.path.exists(os.path.join(ROOT, "fpsg_amd", "libfpsg_hip.so")):
        g.build()
    from fpsg_amd import _hip
    return _hip.load()


def _call(lib, B=2, N=64, eps=1e-4, rounds=100, ptrs=None, grads=(None, None)):
    p = dict(xyz1=FAKE, xyz2=FAKE, cost=FAKE, gap=FAKE, assign=FAKE, status=FAKE, ws=FAKE)
    p.update(ptrs or {})
    return lib.fpsg_emd_exact(p["xyz1"], p["xyz2"], B, N, ctypes.c_float(eps), rounds, p["cost"], p["gap"],
                              p["assign"], p["status"], grads[0], grads[1], p["ws"], None)


@pytest.mark.parametrize("name", ["xyz1", "xyz2", "cost", "gap", "assign", "status", "ws"])
def test_null_required_pointer(lib, name):
    assert _call(lib, ptrs={name: None}) == -1
    assert b"null pointer" in lib.fpsg_last_error() and name.encode() in lib.fpsg_last_error()


@pytest.mark.parametrize("B,N,eps,rounds,msg", [
    (0, 64, 1e-4, 100, b"positive"), (2, 0, 1e-4, 100, b"positive"), (2, -5, 1e-4, 100, b"positive"),
    (2, 2049, 1e-4, 100, b"maximum"), (1, 1 << 20, 1e-4, 100, b"maximum"),
    (2, 64, 0.0, 100, b"eps_final"), (2, 64, -1e-3, 100, b"eps_final"), (2, 64, float("nan"), 100, b"eps_final"),
    (2, 64, float("inf"), 100, b"eps_final"),
    (2, 64, 1e-4, 0, b"max_rounds"), (2, 64, 1e-4, -3, b"max_rounds")])
def test_bad_arguments_are_refused_before_any_launch(lib, B, N, eps, rounds, msg):
    assert _call(lib, B=B, N=N, eps=eps, rounds=rounds) == -2
    assert msg in lib.fpsg_last_error()


def test_largest_supported_size_passes_the_checks_up_to_the_gradient_alignment(lib):
    """N = 2048 (the model's cloud size) is accepted: with a misaligned gradient buffer the call gets past every shape
    check and stops at the alignment one (still before the launch)."""
    assert _call(lib, B=37, N=2048, grads=(FAKE + 2, None)) == -3


def test_workspace_is_monotone_and_zero_for_unsupported_shapes(lib):
    ws = lib.fpsg_emd_exact_workspace_floats
    sizes = [ws(B, N) for B in (1, 2, 5, 37) for N in (1, 2, 7, 128, 2048)]
    assert all(s > 0 for s in sizes)
    for B in (1, 5, 37):
        row = [ws(B, N) for N in (1, 2, 7, 128, 512, 2048)]
        assert row == sorted(row)
    for N in (1, 128, 2048):
        col = [ws(B, N) for B in (1, 2, 5, 37, 1000)]
        assert col == sorted(col) and col[0] < col[-1]
    assert ws(0, 64) == 0 and ws(2, 0) == 0 and ws(2, 2049) == 0


def test_python_wrapper_refuses_unequal_or_oversized_clouds():
    import torch
    from fpsg_amd.metrics import emd_exact
    with pytest.raises(ValueError, match="equal size"):
        emd_exact(torch.zeros(1, 8, 3), torch.zeros(1, 9, 3))
    with pytest.raises(ValueError, match="at most 2048"):
        emd_exact(torch.zeros(1, 4096, 3), torch.zeros(1, 4096, 3))


def test_python_wrapper_has_no_cpu_fallback():
    import torch
    from fpsg_amd._hip import FpsgHipError
    from fpsg_amd.metrics import emd_exact
    with pytest.raises(FpsgHipError):
        emd_exact(torch.rand(1, 8, 3), torch.rand(1, 8, 3))


def test_default_eps_is_relative_to_the_clouds_scale():
    import torch
    from fpsg_amd.metrics import emd_exact_default_eps
    g = torch.Generator().manual_seed(0)
    a, b = torch.rand(2, 2048, 3, generator=g), torch.rand(2, 2048, 3, generator=g)
    e = emd_exact_default_eps(a, b)
    assert e == pytest.approx(emd_exact_default_eps(10 * a, 10 * b) / 10, rel=1e-6)
    assert 1e-7 < e < 1e-5
    assert emd_exact_default_eps(torch.zeros(1, 4, 3), torch.zeros(1, 4, 3)) > 0      # coincident points


def test_evaluation_parser_flag():
    from fpsg_amd import cli
    p = cli.few_shot_parser(evaluation=True)
    assert p.parse_args(["--synthetic"]).exact_emd is False
    assert p.parse_args(["--synthetic", "--exact_emd"]).exact_emd is True
