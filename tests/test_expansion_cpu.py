"""The expansion penalty (K24): what needs no GPU -- the two flags, the option checks, the options on a CPU
model, the C entries' refusals and the workspace size, the float64 reference (its gradient against the closed form, its
tree against scipy's), and the condition on the GPU value tests' inputs: no edge of theirs sits at the threshold."""
import ctypes
import math
import os

import pytest
import torch

from conftest import ROOT

import _expansion_ref as ref

FLAGS = ("expansion_weight", "expansion_lambda")


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
    assert base["expansion_weight"] == 0.0 and base["expansion_lambda"] == 1.5
    assert type(base["expansion_weight"]) is float and type(base["expansion_lambda"]) is float
    on = vars(p.parse_args(["--expansion_weight", "0.25", "--expansion_lambda", "2"]))
    assert (on["expansion_weight"], on["expansion_lambda"]) == (0.25, 2.0)
    assert {k: v for k, v in on.items() if k not in FLAGS} == {k: v for k, v in base.items() if k not in FLAGS}
    assert "minimum spanning tree" in " ".join(p.format_help().split())


@pytest.mark.parametrize("flag,bad", [("expansion_weight", -0.5), ("expansion_weight", math.nan),
                                      ("expansion_weight", math.inf), ("expansion_lambda", 0.99),
                                      ("expansion_lambda", 0.0), ("expansion_lambda", -2.0),
                                      ("expansion_lambda", math.inf), ("expansion_lambda", math.nan)])
def test_validate_refuses_bad_values_and_names_the_flag(flag, bad):
    from fpsg_amd import cli
    p = cli.few_shot_parser()
    cli.validate(p.parse_args(["--synthetic", "--expansion_weight", "0.5", "--expansion_lambda", "1"]))
    cli.validate(p.parse_args(["--synthetic"]))
    opt = p.parse_args(["--synthetic"])
    setattr(opt, flag, bad)
    with pytest.raises(SystemExit) as e:
        cli.validate(opt)
    assert f"--{flag}" in str(e.value)


def test_check_expansion_options():
    from fpsg_amd.metrics import check_expansion_options
    assert check_expansion_options(128, 1.5) == (128, 1.5)
    P, lam = check_expansion_options(2, 1)
    assert (P, lam) == (2, 1.0) and type(P) is int and type(lam) is float
    assert check_expansion_options(1024, 1e30) == (1024, 1e30)
    for bad in (0, 1, 1025, -3, 128.0, "128", None, True):
        with pytest.raises(ValueError, match=r"\bpatch_size\b"):
            check_expansion_options(bad, 1.5)
    for bad in (0.0, 0.999, -1.5, math.inf, -math.inf, math.nan, "x", None, True):
        with pytest.raises(ValueError, match=r"\blam\b"):
            check_expansion_options(128, bad)


# ---- 2. the model carries the options ----------------------------------------------------------------------------------

def test_model_and_build_model_carry_the_options_on_cpu():
    from fpsg_amd.engine import build_model, default_options
    from fpsg_amd.few_shot import ImgPCProtoNet
    opt = default_options(device="cpu")
    assert (opt.expansion_weight, opt.expansion_lambda) == (0.0, 1.5)
    plain = build_model(opt)
    assert (plain.expansion_weight, plain.expansion_lambda) == (0.0, 1.5)
    assert plain.pc_decoder.pts_per_patch == 2048 // (4 * 4) == 128
    model = build_model(default_options(device="cpu", expansion_weight=0.5, expansion_lambda=2, pc_dist="dcd",
                                        repulsion_weight=0.25))
    assert (model.expansion_weight, model.expansion_lambda, model.expansion_patch) == (0.5, 2.0, 128)
    assert model.repulsion_weight == 0.25
    small = build_model(default_options(device="cpu", expansion_weight=1.0, num_clusters=2, num_nodes=8))
    assert small.expansion_patch == 128 and small.pc_decoder.pts_per_patch == 128
    direct = ImgPCProtoNet(plain.img_encoder, plain.pc_encoder, plain.pc_decoder, expansion_weight=2, expansion_lambda=1)
    assert (direct.expansion_weight, direct.expansion_lambda, direct.expansion_patch) == (2.0, 1.0, 128)
    # an options namespace from before the flags existed builds the same model as the defaults
    old = default_options(device="cpu")
    for f in FLAGS:
        delattr(old, f)
    assert build_model(old).expansion_weight == 0.0
    for kw, word in (({"expansion_weight": -1.0}, "expansion_weight"), ({"expansion_weight": math.nan}, "expansion_weight"),
                     ({"expansion_lambda": 0.5}, "lam"), ({"expansion_weight": 1.0, "expansion_lambda": math.inf}, "lam")):
        with pytest.raises(ValueError, match=word):
            ImgPCProtoNet(plain.img_encoder, plain.pc_encoder, plain.pc_decoder, **kw)

    # the patch size is the decoder's: a decoder that does not expose it, or one outside 2..1024, is refused -- but only
    # where the term is on
    class Opaque(torch.nn.Module):
        pass

    class OnePoint(torch.nn.Module):
        pts_per_patch = 1

    class Huge(torch.nn.Module):
        pts_per_patch = 2048

    assert ImgPCProtoNet(plain.img_encoder, plain.pc_encoder, Opaque()).expansion_weight == 0.0
    with pytest.raises(ValueError, match="pts_per_patch"):
        ImgPCProtoNet(plain.img_encoder, plain.pc_encoder, Opaque(), expansion_weight=0.1)
    for dec in (OnePoint(), Huge()):
        with pytest.raises(ValueError, match="patch_size"):
            ImgPCProtoNet(plain.img_encoder, plain.pc_encoder, dec, expansion_weight=0.1)


# ---- 3. the C entries ----------------------------------------------------------------------------------------------------

def test_entries_check_their_arguments_on_the_host(lib):
    """Shape checks, then limit checks, in front of the pointer checks, all of them before any HIP call (no GPU here)."""
    f = ctypes.c_float
    PTR = 0x10000                                                    # never dereferenced

    def fwd(B=2, N=256, P=128, lam=1.5, xyz=None, ws_bytes=0):
        return lib.fpsg_expansion_fwd(xyz, B, N, P, f(lam), None, None, None, None, None, None, ws_bytes, None)

    def bwd(B=2, N=256, P=128, lam=1.5, xyz=None):
        return lib.fpsg_expansion_bwd(xyz, None, None, None, None, B, N, P, f(lam), None, None)

    for call, name in ((fwd, b"fpsg_expansion_fwd"), (bwd, b"fpsg_expansion_bwd")):
        def refused(code, word, **kw):
            assert call(**kw) == code, (name, kw)
            msg = lib.fpsg_last_error()
            assert msg and name in msg and word in msg, (name, kw, msg)
        refused(-1, b"null pointer")                                 # a good shape reaches the pointer checks
        refused(-1, b"null pointer", N=16384, P=1024)
        refused(-1, b"null pointer", N=2, P=2, lam=1.0)
        refused(-2, b"B", B=0)
        refused(-2, b"B", B=-3)
        for P in (1, 0, -128):
            refused(-2, b"P", P=P)
        for N in (255, 100, 0, -256):
            refused(-2, b"multiple", N=N)
        for lam in (0.999, 0.0, -1.5, math.inf, -math.inf, math.nan):
            refused(-2, b"lambda", lam=lam)
        refused(-4, b"1024", N=2048, P=2048)
        refused(-4, b"1024", N=1026, P=1026)
        refused(-4, b"16384", N=16384 + 128)
        refused(-4, b"16384", N=1 << 30)
        refused(-2, b"lambda", N=1 << 30, lam=0.5)                   # a shape error in front of a limit
        refused(-3, b"aligned", xyz=PTR + 2)
    # the forward also refuses a workspace that is too small, behind the pointers
    assert lib.fpsg_expansion_fwd(PTR, 2, 2048, 128, f(1.5), PTR, PTR, PTR, PTR, PTR, PTR, 8, None) == -2
    assert b"workspace" in lib.fpsg_last_error()


def test_workspace_size(lib):
    ws = lib.fpsg_expansion_workspace_bytes
    for bad in ((0, 256, 128), (-1, 256, 128), (2, 256, 1), (2, 256, 0), (2, 255, 128), (2, 0, 128), (2, 2048, 2048),
                (2, 16384 + 128, 128), (2, 64, 128)):
        assert ws(*bad) == 0, bad
    assert ws(1, 2, 2) == 4 and ws(1, 16384, 1024) == 16 * 4
    assert ws(37, 2048, 128) == 37 * 16 * 4                          # one fp32 partial per patch
    assert ws(6, 2048, 128) == 2 * ws(3, 2048, 128) and ws(3, 2048, 64) == 2 * ws(3, 2048, 128)


# ---- 4. the reference --------------------------------------------------------------------------------------------------

def test_reference_gradient_is_the_closed_form():
    """Autograd through the float64 value agrees with the issue's gradient formula written out term by term; the tree's
    tie rules on a case small enough to follow by hand."""
    g = torch.Generator().manual_seed(3)
    P = 20
    x = torch.rand((2, 3 * P, 3), generator=g, dtype=torch.float64) * 0.2
    x[0, 7] += 1.0                                                   # an outlier in patch 0 of cloud 0
    x[1, 2 * P + 4] = x[1, 2 * P + 9]                                # a duplicate: a zero edge, never penalised
    par, d2, order = ref.prim(x, P)
    ref.check_tree(par, order, P)
    for lam in (1.0, 1.5, 2.0):
        mask = ref.penalised(x, P, par, lam)
        assert bool(mask[0, :P].any()) and not bool(mask[:, ::P].any()), "the roots carry no edge"
        up = torch.tensor([1.0, 0.5], dtype=torch.float64)
        E, auto = ref.value_and_grad(x, P, par, mask, up)
        closed = ref.closed_form_grad(x, P, par, mask) * up[:, None, None]
        assert float(auto.abs().max()) > 0 and float(E[0]) > 0 and bool((E >= 0).all())
        assert float((auto - closed).abs().max()) <= 1e-12 * float(closed.abs().max())
        # the value written out: (1 / K) sum_q (1 / (P - 1)) sum_{penalised} r
        r = ref.edge_lengths(x, P, par).reshape(2, 3, P)
        want = (r * mask.reshape(2, 3, P)).sum(2).div(P - 1).mean(1)
        assert float((E - want).abs().max()) <= 1e-15
    # ties: four points on a line at 0, 1, 2 and 1 -- vertex 3 repeats vertex 1.  From vertex 0: 1 and 3 both at d2 = 1,
    # the lower index (1) is added first; then 3 at d2 = 0 from 1; then 2 at d2 = 1, whose parent stays 1 (added before 3)
    line = torch.tensor([[[0.0, 0, 0], [1.0, 0, 0], [2.0, 0, 0], [1.0, 0, 0]]], dtype=torch.float64)
    par, d2, order = ref.prim(line, 4)
    assert par[0].tolist() == [-1, 0, 1, 1] and d2[0].tolist() == [0.0, 1.0, 1.0, 0.0] and order[0].tolist() == [0, 1, 3, 2]
    # every point identical: the keys never improve, everybody hangs on vertex 0 in index order, nothing is penalised
    same = torch.zeros((1, 6, 3), dtype=torch.float64)
    par, d2, order = ref.prim(same, 6)
    assert par[0].tolist() == [-1, 0, 0, 0, 0, 0] and order[0].tolist() == [0, 1, 2, 3, 4, 5] and float(d2.max()) == 0
    assert not bool(ref.penalised(same, 6, par, 1.0).any())


@pytest.mark.parametrize("P", ref.VALUE_P)
def test_value_clouds_have_minimal_trees_and_stay_clear_of_the_threshold(P):
    """On the clouds the GPU value test uses: the reference's tree has scipy's multiset of edge lengths, and no float64
    edge length lies within 1e-4 (relative) of ``lambda * l_q`` at any of the three lambdas -- so the GPU test may demand
    the kernel's penalised mask exactly.  A condition on the inputs, not a tolerance: the seeds in ``_expansion_ref.py``
    were chosen until it held.  The sheet cloud has a penalised edge in every patch."""
    x = ref.value_clouds(P)
    K = ref.value_patches(P)
    assert tuple(x.shape) == (4, K * P, 3) and x.dtype == torch.float32
    par, d2, order = ref.prim(x, P)
    ref.check_tree(par, order, P)
    worst = ref.check_minimal(x, P, par)
    assert worst <= 1e-5
    for lam in ref.VALUE_LAMBDAS:
        margin = ref.threshold_margin(x, P, par, lam)
        assert margin > ref.MARGIN, (P, lam, margin)
        mask = ref.penalised(x, P, par, lam)
        assert bool(mask[3].reshape(K, P).any(1).all()), "every patch of the sheet cloud has a penalised edge"


# ---- 5. no CPU path ------------------------------------------------------------------------------------------------------

def test_a_cpu_tensor_raises():
    from fpsg_amd._hip import FpsgHipError
    from fpsg_amd.metrics import expansion_penalty
    with pytest.raises(FpsgHipError):
        expansion_penalty(torch.rand(2, 16, 3), 8)
    for bad, word in ((torch.rand(2, 16, 2), "B,N,3"), (torch.rand(16, 3), "B,N,3"), (torch.rand(0, 16, 3), "empty"),
                      (torch.rand(2, 20, 3), "multiple"), (torch.rand(2, 4, 3), "multiple"),
                      (torch.rand(1, 16384 + 8, 3), "16384")):
        with pytest.raises(ValueError, match=word):
            expansion_penalty(bad, 8)
    with pytest.raises(ValueError, match=r"\bpatch_size\b"):
        expansion_penalty(torch.rand(2, 16, 3), 1)
    with pytest.raises(ValueError, match=r"\blam\b"):
        expansion_penalty(torch.rand(2, 16, 3), 8, lam=0.5)
