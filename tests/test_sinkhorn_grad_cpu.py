"""The Sinkhorn divergence's gradient (K19): what needs no GPU -- the float64 reference against itself, the
C entry's symbols and argument checks, the ``--pc_dist sinkhorn`` flags and the model's constructor."""
import ctypes
import math
import os
import re

import pytest
import torch

import _sinkhorn_grad_ref as ref
from conftest import ROOT


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    if not os.path.exists(os.path.join(ROOT, "fpsg_amd", "libfpsg_hip.so")):
        g.build()
    from fpsg_amd import _hip
    return _hip.load()


# ---- 1. the reference ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("N,M", [(65, 130), (300, 257)])
def test_closed_form_is_autograd_through_the_final_extrapolation(N, M):
    x, y = ref.clouds(1, N, M, seed=N + M)
    S, gx, gy = ref.closed_form(x, y)
    S2, ax, ay = ref.autograd_form(x, y)
    assert torch.equal(S, S2) and float(S) > 0
    ex, ey = float((gx - ax).abs().max()), float((gy - ay).abs().max())
    print(f"closed form vs autograd at ({N},{M}): {ex:.3e} {ey:.3e}; largest rows {float(gx.norm(dim=-1).max()):.3e} "
          f"{float(gy.norm(dim=-1).max()):.3e}")
    assert ex <= 1e-12 and ey <= 1e-12
    assert float(gx.norm(dim=-1).max()) > 1e-5 and float(gy.norm(dim=-1).max()) > 1e-5
    # a fixed diameter is another schedule, the same identity
    d = 2 * math.sqrt(3)
    _, gx, gy = ref.closed_form(x, y, diameter=d)
    _, ax, ay = ref.autograd_form(x, y, diameter=d)
    assert float((gx - ax).abs().max()) <= 1e-12 and float((gy - ay).abs().max()) <= 1e-12


def test_a_cloud_against_itself_has_a_zero_gradient():
    x, _ = ref.clouds(1, 130, 1, seed=3)
    for form in (ref.closed_form, ref.autograd_form):
        S, gx, gy = form(x, x.clone())
        assert abs(float(S)) <= 1e-15 and not gx.any() and not gy.any()


def test_one_gradient_step_halves_the_divergence():
    """y <- y - 0.5 M gy moves every point of y half of the way its soft assignment asks for.  On a normal cloud scaled
    into the unit ball against tanh(0.4 randn) -- two clouds of about the same spread -- that leaves 0.35-0.44 of the
    float64 divergence (seeds 1-8).  Against a cloud uniform in the ball the float64 ratio is 0.56: the half-annealed
    plan's targets lie short of a wider cloud's rim, a property of the loop, not of the gradient."""
    x, y = ref.gaussian_clouds(1, 300, 257, seed=7)
    S, _, gy = ref.closed_form(x, y)
    S1 = ref.value(x, y.double() - 0.5 * y.size(1) * gy)
    print(f"descent: {float(S):.6e} -> {float(S1):.6e} (ratio {float(S1 / S):.3f})")
    assert 0.0 <= float(S1) < 0.5 * float(S)


# ---- 2. the C ABI --------------------------------------------------------------------------------------------------

def test_library_exports_the_two_symbols_and_the_table_binds_them(lib):
    from fpsg_amd import _hip
    for name in ("fpsg_sinkhorn_grad_workspace_floats", "fpsg_sinkhorn_divergence_grad"):
        assert name in _hip.SIGNATURES and hasattr(lib, name)
    assert _hip._RESTYPES["fpsg_sinkhorn_grad_workspace_floats"] is ctypes.c_size_t
    sig = _hip.SIGNATURES["fpsg_sinkhorn_divergence_grad"]
    assert len(sig) == len(_hip.SIGNATURES["fpsg_sinkhorn_divergence"]) + 2
    text = open(os.path.join(ROOT, "include", "fpsg_hip.h")).read()
    decl = text[text.index("int fpsg_sinkhorn_divergence_grad("):]
    assert re.sub(r"/\*.*?\*/", "", decl[:decl.index(";")]).count(",") == len(sig) - 1
    assert lib.fpsg_version() == 1
    # the duals' two sets and four displacement arrays
    assert lib.fpsg_sinkhorn_grad_workspace_floats(5, 300, 257) == \
        lib.fpsg_sinkhorn_workspace_floats(5, 300, 257) + 5 * 6 * (300 + 257)
    for bad in ((0, 4, 4), (4, 0, 4), (4, 4, -1)):
        assert lib.fpsg_sinkhorn_grad_workspace_floats(*bad) == 0


def test_grad_entry_checks_its_arguments_like_its_forward_twin(lib):
    """Every refusal comes before any HIP call (no GPU here), with the code fpsg_sinkhorn_divergence gives."""
    P, Q = 0x10000, 0x10002                                        # never dereferenced: aligned / misaligned fakes
    good = (ctypes.c_float * 3)(4.0, 1.0, 0.0025)

    def both(x=P, y=P, B=2, N=65, M=130, eps=good, n=3, out=P, gx=P, gy=P, ws=P):
        eps_p = None if eps is None else ctypes.cast(eps, ctypes.c_void_p)
        grad = lib.fpsg_sinkhorn_divergence_grad(x, y, B, N, M, eps_p, n, out, gx, gy, ws, None)
        msg = lib.fpsg_last_error()
        fwd = lib.fpsg_sinkhorn_divergence(x, y, B, N, M, eps_p, n, out, ws, None)
        assert grad == fwd and grad != 0, (grad, fwd)
        assert b"fpsg_sinkhorn_divergence_grad" in msg, msg
        return grad

    null, shape, align, limit = -1, -2, -3, -4
    for kw in ({"x": None}, {"y": None}, {"out": None}, {"ws": None}):
        assert both(**kw) == null, kw
    for kw in ({"B": 0}, {"N": 0}, {"M": 0}, {"B": -1}, {"N": -5}, {"M": -2}):
        assert both(**kw) == shape, kw
    assert both(B=65536) == limit
    assert both(eps=None) == shape and both(n=0) == shape and both(n=-3) == shape and both(n=4097) == shape
    for bad in ((4.0, 0.0, 0.0025), (4.0, 1.0, -0.0025), (float("nan"), 1.0, 0.0025)):
        assert both(eps=(ctypes.c_float * 3)(*bad)) == shape, bad
    for kw in ({"x": Q}, {"y": Q}, {"out": Q}, {"ws": Q}):
        assert both(**kw) == align, kw
    # gx and gy may be null, not misaligned (the twin has neither)
    eps_p = ctypes.cast(good, ctypes.c_void_p)
    assert lib.fpsg_sinkhorn_divergence_grad(P, P, 2, 65, 130, eps_p, 3, P, Q, None, P, None) == align
    assert lib.fpsg_sinkhorn_divergence_grad(P, P, 2, 65, 130, eps_p, 3, P, None, 0x10001, P, None) == align
    assert lib.fpsg_sinkhorn_divergence_grad(None, P, 2, 65, 130, eps_p, 3, P, None, None, P, None) == null


# ---- 3. the mirror -------------------------------------------------------------------------------------------------

def test_sinkhorn_loss_checks_before_the_library_and_has_no_cpu_path(monkeypatch):
    from fpsg_amd import _hip, metrics
    from fpsg_amd._hip import FpsgHipError
    p1, p2 = torch.rand(2, 16, 3), torch.rand(2, 8, 3)
    with pytest.raises(FpsgHipError):
        metrics.sinkhorn_loss(p1, p2, diameter=2.0)
    with pytest.raises(FpsgHipError):
        metrics.sinkhorn_loss(p1.requires_grad_(), p2)
    with pytest.raises(ValueError):
        metrics.sinkhorn_loss(torch.rand(16, 3), p2)
    assert metrics.SINKHORN_TRAIN_DIAMETER == 2 * math.sqrt(3)
    assert metrics.check_sinkhorn_option(1, "blur") == 1.0 and type(metrics.check_sinkhorn_option(1, "blur")) is float
    for bad in (0.0, -0.05, float("nan"), float("inf"), None, "a"):
        with pytest.raises(ValueError, match="sinkhorn_blur"):
            metrics.check_sinkhorn_option(bad, "sinkhorn_blur")


# ---- 4. the flags --------------------------------------------------------------------------------------------------

OURS = ("pc_dist", "sinkhorn_blur", "sinkhorn_diameter")


def test_flags_parse_and_change_nothing_else():
    from fpsg_amd import cli
    for evaluation in (False, True):
        p = cli.few_shot_parser(evaluation=evaluation)
        base = vars(p.parse_args([]))
        assert base["pc_dist"] == "cd" and base["sinkhorn_blur"] == 0.05
        assert base["sinkhorn_diameter"] == 2 * math.sqrt(3)
        on = vars(p.parse_args(["--pc_dist", "sinkhorn"]))
        assert on["pc_dist"] == "sinkhorn"
        assert {k: v for k, v in on.items() if k != "pc_dist"} == {k: v for k, v in base.items() if k != "pc_dist"}
        on = vars(p.parse_args(["--pc_dist", "sinkhorn", "--sinkhorn_blur", "0.1", "--sinkhorn_diameter", "2"]))
        assert on["sinkhorn_blur"] == 0.1 and on["sinkhorn_diameter"] == 2.0 and type(on["sinkhorn_diameter"]) is float
        assert {k: v for k, v in on.items() if k not in OURS} == {k: v for k, v in base.items() if k not in OURS}
        for other in ("cd", "emd", "dcd"):
            assert p.parse_args(["--pc_dist", other]).pc_dist == other
        with pytest.raises(SystemExit):
            p.parse_args(["--pc_dist", "x"])
        assert "item's own bounding-box diagonal" in " ".join(p.format_help().split())     # differs from the evaluation's


def test_validate_refuses_bad_blur_and_diameter():
    from fpsg_amd import cli
    tr = cli.few_shot_parser()
    cli.validate(tr.parse_args(["--synthetic"]))
    cli.validate(tr.parse_args(["--synthetic", "--pc_dist", "sinkhorn", "--sinkhorn_blur", "0.1",
                                "--sinkhorn_diameter", "2"]))
    for flag in ("--sinkhorn_blur", "--sinkhorn_diameter"):
        for bad in ("0", "-1", "nan", "inf", "-inf"):
            with pytest.raises(SystemExit) as e:
                cli.validate(tr.parse_args(["--synthetic", "--pc_dist", "sinkhorn", f"{flag}={bad}"]))
            assert flag in str(e.value), (flag, bad, str(e.value))


# ---- 5. the model --------------------------------------------------------------------------------------------------

def test_model_takes_the_sinkhorn_metric():
    from fpsg_amd.engine import build_model, default_options
    from fpsg_amd.few_shot import ImgPCProtoNet
    from fpsg_amd.metrics import chamfer_distance
    assert default_options().pc_dist == "cd"
    base = build_model(default_options(device="cpu"))
    assert base.pc_metric is chamfer_distance                        # the default is untouched
    parts = (base.img_encoder, base.pc_encoder, base.pc_decoder)
    m = ImgPCProtoNet(*parts, metric="sinkhorn")
    assert m.sinkhorn_blur == 0.05 and m.sinkhorn_diameter == 2 * math.sqrt(3) and m.pc_metric is not chamfer_distance
    m = ImgPCProtoNet(*parts, metric="sinkhorn", sinkhorn_blur=0.1, sinkhorn_diameter=2)
    assert m.sinkhorn_blur == 0.1 and m.sinkhorn_diameter == 2.0
    m = build_model(default_options(device="cpu", pc_dist="sinkhorn", sinkhorn_blur=0.2, sinkhorn_diameter=3.0))
    assert m.sinkhorn_blur == 0.2 and m.sinkhorn_diameter == 3.0
    assert build_model(default_options(device="cpu", pc_dist="sinkhorn")).sinkhorn_diameter == 2 * math.sqrt(3)
    for other in ("cd", "emd", "dcd"):
        ImgPCProtoNet(*parts, metric=other)
    with pytest.raises(NotImplementedError):
        ImgPCProtoNet(*parts, metric="x")
    for bad in (0.0, -1.0, float("nan"), math.inf):
        with pytest.raises(ValueError, match="sinkhorn_blur"):
            ImgPCProtoNet(*parts, metric="sinkhorn", sinkhorn_blur=bad)
        with pytest.raises(ValueError, match="sinkhorn_diameter"):
            ImgPCProtoNet(*parts, metric="sinkhorn", sinkhorn_diameter=bad)
