"""The repulsion regulariser (K21): what needs no GPU -- the three flags, the option checks, the options on
a CPU model, the C entries' refusals and the workspace size, and the float64 reference's gradient against the closed
form (which pins the formula, not the kernel)."""
import ctypes
import math
import os

import pytest
import torch

from conftest import ROOT

import _repulsion_ref as ref

FLAGS = ("repulsion_weight", "repulsion_k", "repulsion_h")


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    if not os.path.exists(os.path.join(ROOT, "fpsg_amd", "libfpsg_hip.so")):
        g.build()
    from fpsg_amd import _hip
    return _hip.load()


# ---- 1. the flags --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("evaluation", [False, True])
def test_flags_parse_and_change_nothing_else(evaluation):
    from fpsg_amd import cli
    p = cli.few_shot_parser(evaluation=evaluation)
    base = vars(p.parse_args([]))
    assert base["repulsion_weight"] == 0.0 and base["repulsion_k"] == 4 and base["repulsion_h"] == 0.03
    assert type(base["repulsion_weight"]) is float and type(base["repulsion_k"]) is int
    on = vars(p.parse_args(["--repulsion_weight", "0.25", "--repulsion_k", "6", "--repulsion_h", "0.1"]))
    assert (on["repulsion_weight"], on["repulsion_k"], on["repulsion_h"]) == (0.25, 6, 0.1)
    assert {k: v for k, v in on.items() if k not in FLAGS} == {k: v for k, v in base.items() if k not in FLAGS}
    assert "unit ball" in " ".join(p.format_help().split())


@pytest.mark.parametrize("flag,bad", [("repulsion_weight", -0.5), ("repulsion_weight", math.nan),
                                      ("repulsion_weight", math.inf), ("repulsion_k", 0), ("repulsion_k", 9),
                                      ("repulsion_k", -1), ("repulsion_h", 0.0), ("repulsion_h", -0.03),
                                      ("repulsion_h", math.inf), ("repulsion_h", math.nan)])
def test_validate_refuses_bad_values_and_names_the_flag(flag, bad):
    from fpsg_amd import cli
    p = cli.few_shot_parser()
    good = p.parse_args(["--synthetic", "--repulsion_weight", "0.5", "--repulsion_k", "8", "--repulsion_h", "0.3"])
    cli.validate(good)
    cli.validate(p.parse_args(["--synthetic"]))
    opt = p.parse_args(["--synthetic"])
    setattr(opt, flag, bad)
    with pytest.raises(SystemExit) as e:
        cli.validate(opt)
    assert f"--{flag}" in str(e.value)


def test_check_repulsion_options():
    from fpsg_amd.metrics import check_repulsion_options
    assert check_repulsion_options(4, 0.03) == (4, 0.03)
    k, h = check_repulsion_options(1, 2)
    assert (k, h) == (1, 2.0) and type(k) is int and type(h) is float
    assert check_repulsion_options(8, 1e-9) == (8, 1e-9)
    for bad in (0, 9, -3, 2.0, "4", None, True):
        with pytest.raises(ValueError, match=r"\bk\b"):
            check_repulsion_options(bad, 0.03)
    for bad in (0.0, -1.0, math.inf, -math.inf, math.nan, "x", None, True):
        with pytest.raises(ValueError, match=r"\bh\b"):
            check_repulsion_options(4, bad)


# ---- 2. the model carries the options ----------------------------------------------------------------------------------

def test_model_and_build_model_carry_the_options_on_cpu():
    from fpsg_amd.engine import build_model, default_options
    from fpsg_amd.few_shot import ImgPCProtoNet
    opt = default_options(device="cpu")
    assert (opt.repulsion_weight, opt.repulsion_k, opt.repulsion_h) == (0.0, 4, 0.03)
    plain = build_model(opt)
    assert (plain.repulsion_weight, plain.repulsion_k, plain.repulsion_h) == (0.0, 4, 0.03)
    model = build_model(default_options(device="cpu", repulsion_weight=0.5, repulsion_k=6, repulsion_h=0.1, pc_dist="dcd"))
    assert (model.repulsion_weight, model.repulsion_k, model.repulsion_h) == (0.5, 6, 0.1)
    direct = ImgPCProtoNet(plain.img_encoder, plain.pc_encoder, plain.pc_decoder, repulsion_weight=2, repulsion_k=1,
                           repulsion_h=1)
    assert (direct.repulsion_weight, direct.repulsion_k, direct.repulsion_h) == (2.0, 1, 1.0)
    # an options namespace from before the flags existed builds the same model as the defaults
    old = default_options(device="cpu")
    for f in FLAGS:
        delattr(old, f)
    assert build_model(old).repulsion_weight == 0.0
    for kw in ({"repulsion_weight": -1.0}, {"repulsion_weight": math.nan}, {"repulsion_k": 9}, {"repulsion_h": 0.0}):
        with pytest.raises(ValueError, match=next(iter(kw))[len("repulsion_"):]):
            ImgPCProtoNet(plain.img_encoder, plain.pc_encoder, plain.pc_decoder, **kw)


# ---- 3. the C entries ----------------------------------------------------------------------------------------------------

def test_entries_check_their_arguments_on_the_host(lib):
    """Shape and limit checks answer in front of the pointer checks, all of them before any HIP call (no GPU here)."""
    f = ctypes.c_float
    P = 0x10000                                                      # never dereferenced

    def fwd(B=2, N=64, k=4, h=0.03, xyz=None, ws_bytes=0):
        return lib.fpsg_repulsion_fwd(xyz, B, N, k, f(h), None, None, None, None, ws_bytes, None)

    def bwd(B=2, N=64, k=4, h=0.03, xyz=None):
        return lib.fpsg_repulsion_bwd(xyz, None, None, None, B, N, k, f(h), None, None)

    for call, name in ((fwd, b"fpsg_repulsion_fwd"), (bwd, b"fpsg_repulsion_bwd")):
        def refused(code, word, **kw):
            assert call(**kw) == code, (name, kw)
            msg = lib.fpsg_last_error()
            assert msg and name in msg and word in msg, (name, kw, msg)
        refused(-1, b"null pointer")                                 # a good shape reaches the pointer checks
        refused(-1, b"null pointer", N=16384, k=8)
        refused(-1, b"null pointer", N=5, k=4)                       # N = k + 1 is served
        refused(-2, b"B", B=0)
        refused(-2, b"B", B=-3)
        for k in (0, 9, -1):
            refused(-2, b"k", k=k)
        refused(-2, b"N", N=4, k=4)
        refused(-2, b"N", N=1, k=1)
        for h in (0.0, -0.03, math.inf, -math.inf, math.nan):
            refused(-2, b"h", h=h)
        refused(-4, b"16384", N=16385)
        refused(-4, b"16384", N=1 << 30)
        refused(-3, b"aligned", xyz=P + 2)
    # the forward also refuses a workspace that is too small, behind the pointers
    assert lib.fpsg_repulsion_fwd(P, 2, 600, 4, f(0.03), P, P, P, P, 8, None) == -2
    assert b"workspace" in lib.fpsg_last_error()


def test_workspace_size(lib):
    ws = lib.fpsg_repulsion_workspace_bytes
    for bad in ((0, 64, 4), (-1, 64, 4), (2, 4, 4), (2, 64, 0), (2, 64, 9), (2, 16385, 4), (2, 0, 1), (2, 1, 1)):
        assert ws(*bad) == 0, bad
    assert ws(1, 2, 1) > 0 and ws(1, 16384, 8) > 0
    sizes = [ws(3, n, 4) for n in (5, 256, 257, 2048, 16384)]
    assert all(a <= b for a, b in zip(sizes, sizes[1:])) and all(s % 4 == 0 for s in sizes)
    assert ws(37, 2048, 4) == 37 * 8 * 4                             # one fp32 partial per 256 points and cloud
    assert ws(6, 2048, 4) == 2 * ws(3, 2048, 4) and ws(3, 2048, 1) == ws(3, 2048, 8)


# ---- 4. the reference --------------------------------------------------------------------------------------------------

def test_reference_gradient_is_the_closed_form():
    """Autograd through the float64 value agrees with the issue's gradient formula written out term by term."""
    g = torch.Generator().manual_seed(3)
    x = torch.rand((2, 40, 3), generator=g, dtype=torch.float64) * 0.4
    x[1, 7] = x[1, 3]                                                # a duplicate: its pair term has derivative 0
    for h in (0.03, 0.3):
        idx, d2 = ref.neighbour_lists(x, 4)
        assert idx.shape == (2, 40, 4) and bool((d2[:, :, 1:] >= d2[:, :, :-1]).all())
        assert not bool((idx == torch.arange(40)[None, :, None]).any())
        assert int(idx[1, 7, 0]) == 3 and int(idx[1, 3, 0]) == 7 and float(d2[1, 7, 0]) == 0.0
        R, auto = ref.value_and_grad(x, idx, h)
        closed = ref.closed_form_grad(x, idx, h)
        assert float(auto.abs().max()) > 0
        assert float((auto - closed).abs().max()) <= 1e-12 * float(closed.abs().max())
        assert bool((R <= 0).all()) and bool((R >= -h / math.sqrt(2 * math.e)).all())
    # the lists break ties towards the lower index
    tie = torch.zeros((1, 6, 3), dtype=torch.float64)
    idx, d2 = ref.neighbour_lists(tie, 3)
    assert idx[0].tolist() == [[1, 2, 3], [0, 2, 3], [0, 1, 3], [0, 1, 2], [0, 1, 2], [0, 1, 2]] and float(d2.max()) == 0


# ---- 5. no CPU path ------------------------------------------------------------------------------------------------------

def test_a_cpu_tensor_raises():
    from fpsg_amd._hip import FpsgHipError
    from fpsg_amd.metrics import repulsion_loss
    with pytest.raises(FpsgHipError):
        repulsion_loss(torch.rand(2, 16, 3))
    for bad, word in ((torch.rand(2, 16, 2), "B,N,3"), (torch.rand(16, 3), "B,N,3"), (torch.rand(0, 16, 3), "empty"),
                      (torch.rand(2, 4, 3), "k \\+ 1"), (torch.rand(1, 16385, 3), "16384")):
        with pytest.raises(ValueError, match=word):
            repulsion_loss(bad)
    with pytest.raises(ValueError, match=r"\bk\b"):
        repulsion_loss(torch.rand(2, 16, 3), k=9)
    with pytest.raises(ValueError, match=r"\bh\b"):
        repulsion_loss(torch.rand(2, 16, 3), h=0.0)
