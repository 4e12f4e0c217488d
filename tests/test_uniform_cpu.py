"""The uniform loss (K25): what needs no GPU -- the float64 reference against hand-computed cases and central
differences (which pins the formula, not the kernel), the C entries' refusals and the workspace size, the three flags,
the option checks and the options on a CPU model."""
import ctypes
import math
import os

import pytest
import torch

from conftest import ROOT

import _uniform_ref as ref

FLAGS = ("uniform_weight", "uniform_percent", "uniform_radius")
DEFAULT = (0.004, 0.006, 0.008, 0.010, 0.012)


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    if not os.path.exists(os.path.join(ROOT, "fpsg_amd", "libfpsg_hip.so")):
        g.build()
    from fpsg_amd import _hip
    return _hip.load()


# ---- 1. the reference against known answers ---------------------------------------------------------------------------

def test_reference_two_points_in_one_ball():
    """p = 1/16, R = 1: r = 1/4; the two points are 1/8 apart.  c = 2, nhat = 1/8, w = (15/8)^2 / (1/8) = 28.125, both
    members have d = 1/8; U = w * 2 (d - dhat)^2 / dhat."""
    x = torch.tensor([[[0.0, 0.0, 0.0], [0.125, 0.0, 0.0]]], dtype=torch.float64)
    seeds = torch.tensor([[0]])
    count, member, nn, nn_d2 = ref.ball_lists(x, seeds, (0.0625,), 1.0, 64)
    assert count.tolist() == [[[2]]] and member[0, 0, 0, :3].tolist() == [0, 1, -1]
    assert nn[0, 0, 0, :3].tolist() == [1, 0, -1] and nn_d2[0, 0, 0, :3].tolist() == [1 / 64, 1 / 64, math.inf]
    v, per, U, g = ref.value_and_grad(x, seeds, count, member, nn, (0.0625,), 1.0)
    dhat = math.sqrt(2 * math.pi / math.sqrt(3) * 0.0625 / 2)
    want = 28.125 * 2 * (0.125 - dhat) ** 2 / dhat
    assert abs(float(v) - want) <= 1e-14 * want and abs(float(per) - want) <= 1e-14 * want
    assert abs(float(U) - want) <= 1e-14 * want
    # each point: its own term and the other's reverse term, both 28.125 * 2 (d - dhat) / dhat along the pair
    gx = 2 * 28.125 * 2 * (0.125 - dhat) / dhat
    assert torch.allclose(g[0], torch.tensor([[-gx, 0, 0], [gx, 0, 0]], dtype=torch.float64), rtol=1e-13, atol=0)


def test_reference_a_point_exactly_on_the_sphere_is_inside():
    x = torch.tensor([[[0.0, 0.0, 0.0], [0.25, 0.0, 0.0], [0.0, 0.125, 0.0], [1.0, 1.0, 1.0]]], dtype=torch.float64)
    seeds = torch.tensor([[0, 3]])
    count, member, nn, nn_d2 = ref.ball_lists(x, seeds, (0.0625,), 1.0, 64)
    assert count[0, 0].tolist() == [3, 1]
    assert member[0, 0, 0, :4].tolist() == [0, 1, 2, -1] and member[0, 0, 1, :2].tolist() == [3, -1]
    assert nn[0, 0, 0, :4].tolist() == [2, 0, 0, -1] and nn[0, 0, 1, :2].tolist() == [-1, -1]
    assert nn_d2[0, 0, 0, :3].tolist() == [1 / 64, 1 / 16, 1 / 64] and float(nn_d2[0, 0, 1, 0]) == math.inf
    v, per, U, g = ref.value_and_grad(x, seeds, count, member, nn, (0.0625,), 1.0)
    dhat = math.sqrt(2 * math.pi / math.sqrt(3) * 0.0625 / 3)
    w = (3 - 0.25) ** 2 / 0.25
    want = w * (2 * (0.125 - dhat) ** 2 + (0.25 - dhat) ** 2) / dhat
    assert abs(float(U[0, 0, 0]) - want) <= 1e-14 * want
    assert float(U[0, 0, 1]) == 0.0, "a ball of one is worth 0"
    assert abs(float(v) - want / 2) <= 1e-14 * want and bool((g[0, 3] == 0).all())
    # a seed outside the cloud owns an empty ball and contributes 0
    bad = torch.tensor([[0, -1], ], dtype=torch.int64)
    count, member, nn, _ = ref.ball_lists(x, bad, (0.0625,), 1.0, 64)
    assert count[0, 0].tolist() == [3, 0] and bool((member[0, 0, 1] == -1).all())
    v2, _, U2, _ = ref.value_and_grad(x, bad, count, member, nn, (0.0625,), 1.0)
    assert float(U2[0, 0, 1]) == 0.0 and abs(float(v2) - want / 2) <= 1e-14 * want


def test_reference_all_coincident_cloud():
    """Every distance is 0: every ball holds all N points, every term is dhat, the gradient is exactly 0."""
    N, ps = 5, (0.0625, 0.25)
    x = torch.tensor([0.3, -0.2, 0.7], dtype=torch.float64).expand(1, N, 3).contiguous()
    seeds = torch.tensor([[0, 3]])
    count, member, nn, nn_d2 = ref.ball_lists(x, seeds, ps, 1.0, 64)
    assert bool((count == N).all()) and bool((nn_d2[..., :N] == 0).all())
    assert member[0, 1, 1, :N + 1].tolist() == [0, 1, 2, 3, 4, -1] and nn[0, 1, 1, :N + 1].tolist() == [1, 0, 0, 0, 0, -1]
    v, per, U, g = ref.value_and_grad(x, seeds, count, member, nn, ps, 1.0)
    want = []
    for p in ps:
        dhat = math.sqrt(2 * math.pi / math.sqrt(3) * p / N)
        want.append((N - N * p) ** 2 / (N * p) * N * dhat)
    assert torch.allclose(per[0], torch.tensor(want, dtype=torch.float64), rtol=1e-14, atol=0)
    assert abs(float(v) - sum(want) / 2) <= 1e-14 * sum(want)
    assert bool((g == 0).all()) and bool(torch.isfinite(g).all())


def test_reference_gradient_against_central_differences():
    """Float64 autograd on fixed lists against central differences on the same lists, N = 40; one duplicate pair (no
    gradient through it), every ball below the cap."""
    from _gradcheck import deviations
    gen = torch.Generator().manual_seed(25)
    N, ps, R = 40, (0.05, 0.15, 0.4), 1.0
    x = torch.rand((2, N, 3), generator=gen, dtype=torch.float64) * 0.8
    x[1, 7] = x[1, 3]
    seeds = torch.stack([torch.randperm(N, generator=gen)[:6] for _ in range(2)])
    seeds[1, 0] = 3
    count, member, nn, nn_d2 = ref.ball_lists(x, seeds, ps, R, 64)
    assert int((count >= 2).sum()) > count.numel() // 2 and int(count.max()) <= 64
    assert bool((nn_d2[1][member[1] == 7] == 0).all()) and int((member[1] == 7).sum()) > 0
    up = torch.tensor([1.0, 0.5], dtype=torch.float64)
    v, _, _, g = ref.value_and_grad(x, seeds, count, member, nn, ps, R, up)
    assert float(v.min()) > 0 and float(g.abs().max()) > 0
    h = 1e-6
    fd = torch.zeros_like(x)
    for b in range(2):
        for i in range(N):
            for a in range(3):
                hi, lo = x.clone(), x.clone()
                hi[b, i, a] += h
                lo[b, i, a] -= h
                fd[b, i, a] = ((ref.value(hi, seeds, count, member, nn, ps, R)[0] * up).sum()
                               - (ref.value(lo, seeds, count, member, nn, ps, R)[0] * up).sum()) / (2 * h)
    dev, _ = deviations({"g": g}, {"g": fd})
    assert dev["g"] <= 1e-7, dev                                     # central differences at h = 1e-6: O(h^2) + round-off / h
    # the same expression in fp32 stays near the float64 one
    v32, _, _, g32 = ref.value_and_grad(x.float(), seeds, count, member, nn, ps, R, up, dtype=torch.float32)
    assert v32.dtype == torch.float32 and float(((v32.double() - v).abs() / v).max()) <= 1e-5
    assert float((g32.double() - g).abs().max()) <= 1e-4 * float(g.abs().max())


# ---- 2. the C entries ----------------------------------------------------------------------------------------------------

def _percent(values):
    return (ctypes.c_float * len(values))(*values) if values is not None else None


def test_entries_check_their_arguments_on_the_host(lib):
    """The order of include/fpsg_hip.h: integer shapes, radius and cap; the limits; a null percent; the percentages; the
    other pointers; the workspace.  All of them before any HIP call (no GPU here)."""
    f = ctypes.c_float
    P = 0x10000                                                      # never dereferenced

    def fwd(B=2, N=64, S=4, percent=DEFAULT, T=None, radius=1.0, cap=64, xyz=None):
        T = len(percent) if T is None else T
        return lib.fpsg_uniform_fwd(xyz, None, B, N, S, _percent(percent), T, f(radius), cap, None, None, None, None, None,
                                    None, None, None, 0, None)

    def bwd(B=2, N=64, S=4, percent=DEFAULT, T=None, radius=1.0, cap=64, xyz=None):
        T = len(percent) if T is None else T
        return lib.fpsg_uniform_bwd(xyz, None, None, None, None, None, None, B, N, S, T, _percent(percent), f(radius), cap,
                                    None, None)

    for call, name in ((fwd, b"fpsg_uniform_fwd"), (bwd, b"fpsg_uniform_bwd")):
        def refused(code, word, **kw):
            assert call(**kw) == code, (name, kw)
            msg = lib.fpsg_last_error()
            assert msg and name in msg and word in msg, (name, kw, msg)
        refused(-1, b"null pointer 'xyz'")                           # a good shape reaches the pointer checks
        refused(-1, b"null pointer 'xyz'", N=16384, S=16384, percent=(1.0,) * 8, cap=256)
        refused(-1, b"null pointer 'xyz'", N=2, S=2, percent=(1e-30,), cap=128)
        for B in (0, -3):
            refused(-2, b"B", B=B)
        for S in (0, -1):
            refused(-2, b"S", S=S)
        refused(-2, b"T", T=0)
        refused(-2, b"T", T=-2)
        for N in (1, 0, -5):
            refused(-2, b"N", N=N, S=1)
        refused(-2, b"S must not exceed N", N=64, S=65)
        for r in (0.0, -1.0, math.inf, -math.inf, math.nan):
            refused(-2, b"radius", radius=r)
        for cap in (0, 32, 65, 192, 512, -64):
            refused(-2, b"cap", cap=cap)
        refused(-4, b"16384", N=16385)
        refused(-4, b"16384", N=1 << 30)
        refused(-4, b"8", percent=(0.01,) * 9)
        refused(-1, b"null pointer 'percent'", percent=None, T=3)
        for bad in (0.0, -0.01, 1.0000001, 2.0, math.inf, -math.inf, math.nan):
            refused(-2, b"percent[1]", percent=(0.01, bad, 0.02))
        refused(-3, b"aligned", xyz=P + 2)
        # shape in front of limit, both in front of percent and of the pointers
        refused(-2, b"B", B=0, N=1 << 30, percent=None, T=3)
        refused(-2, b"cap", cap=100, N=16385, percent=(0.01,) * 9)
        refused(-4, b"16384", N=16385, percent=(2.0,))
        refused(-4, b"8", T=9, percent=None)
        refused(-2, b"percent[0]", percent=(2.0,), xyz=P + 2)
    # the forward also refuses a workspace that is too small, behind the pointers
    need = lib.fpsg_uniform_workspace_bytes(2, 600, 30, 5, 64)
    assert need > 4
    assert lib.fpsg_uniform_fwd(P, P, 2, 600, 30, _percent(DEFAULT), 5, f(1.0), 64, P, P, P, P, P, P, P, P, need - 4,
                                None) == -2
    assert b"workspace" in lib.fpsg_last_error()
    assert lib.fpsg_uniform_fwd(P, P, 2, 600, 30, _percent(DEFAULT), 5, f(1.0), 64, P, P, P, P, P, P, P, None, need,
                                None) == -1


def test_workspace_size(lib):
    ws = lib.fpsg_uniform_workspace_bytes
    for bad in ((0, 64, 4, 5, 64), (-1, 64, 4, 5, 64), (2, 1, 1, 5, 64), (2, 64, 0, 5, 64), (2, 64, 65, 5, 64),
                (2, 64, 4, 0, 64), (2, 64, 4, 9, 64), (2, 64, 4, 5, 63), (2, 64, 4, 5, 0), (2, 64, 4, 5, 512),
                (2, 16385, 4, 5, 64)):
        assert ws(*bad) == 0, bad
    assert ws(1, 2, 1, 1, 64) > 0 and ws(1, 16384, 16384, 8, 256) > 0
    assert ws(37, 2048, 102, 5, 64) == 37 * 5 * 4                   # one fp32 row sum per cloud and percentage
    assert ws(6, 2048, 102, 5, 64) == 2 * ws(3, 2048, 102, 5, 64) and ws(3, 2048, 102, 5, 64) == ws(3, 300, 7, 5, 256)


# ---- 3. the flags ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("evaluation", [False, True])
def test_flags_parse_and_change_nothing_else(evaluation):
    from fpsg_amd import cli
    p = cli.few_shot_parser(evaluation=evaluation)
    base = vars(p.parse_args([]))
    assert base["uniform_weight"] == 0.0 and base["uniform_percent"] == [0.4, 0.6, 0.8, 1.0, 1.2]
    assert base["uniform_radius"] == 1.0
    assert type(base["uniform_weight"]) is float and type(base["uniform_radius"]) is float
    assert all(type(v) is float for v in base["uniform_percent"])
    on = vars(p.parse_args(["--uniform_weight", "0.25", "--uniform_percent", "2", "5.5", "--uniform_radius", "0.5"]))
    assert (on["uniform_weight"], on["uniform_percent"], on["uniform_radius"]) == (0.25, [2.0, 5.5], 0.5)
    assert {k: v for k, v in on.items() if k not in FLAGS} == {k: v for k, v in base.items() if k not in FLAGS}
    assert "percent of the cloud" in " ".join(p.format_help().split())


def test_validate_turns_percent_into_the_models_fractions():
    from fpsg_amd import cli
    p = cli.few_shot_parser()
    opt = p.parse_args(["--synthetic"])
    cli.validate(opt)
    assert opt.uniform_percentages == DEFAULT
    opt = p.parse_args(["--synthetic", "--uniform_weight", "0.5", "--uniform_percent", "2", "100", "--uniform_radius", "3"])
    cli.validate(opt)
    assert opt.uniform_percentages == (0.02, 1.0)
    cli.validate(p.parse_args(["--synthetic", "--uniform_percent"] + ["1"] * 8))


@pytest.mark.parametrize("flag,bad", [("uniform_weight", -0.5), ("uniform_weight", math.nan), ("uniform_weight", math.inf),
                                      ("uniform_percent", [0.4, 0.0]), ("uniform_percent", [100.5]),
                                      ("uniform_percent", [-1.0]), ("uniform_percent", [math.nan]),
                                      ("uniform_percent", [math.inf]), ("uniform_percent", [1.0] * 9),
                                      ("uniform_percent", []), ("uniform_radius", 0.0), ("uniform_radius", -1.0),
                                      ("uniform_radius", math.inf), ("uniform_radius", math.nan)])
def test_validate_refuses_bad_values_and_names_the_flag(flag, bad):
    from fpsg_amd import cli
    opt = cli.few_shot_parser().parse_args(["--synthetic"])
    setattr(opt, flag, bad)
    with pytest.raises(SystemExit) as e:
        cli.validate(opt)
    assert f"--{flag}" in str(e.value)


def test_check_uniform_options():
    from fpsg_amd.metrics import check_uniform_options
    assert check_uniform_options(DEFAULT, 1.0) == (DEFAULT, 1.0)
    ps, r = check_uniform_options([1, 0.5], 2)
    assert ps == (1.0, 0.5) and r == 2.0 and all(type(v) is float for v in ps) and type(r) is float
    assert check_uniform_options((1e-9,) * 8, 1e-9) == ((1e-9,) * 8, 1e-9)
    for bad in ((), (0.01,) * 9, (0.0,), (-0.1,), (1.5,), (math.nan,), (math.inf,), ("x",), (None,), (True,), 0.01, None,
                "0.01"):
        with pytest.raises(ValueError, match="percentages"):
            check_uniform_options(bad, 1.0)
    for bad in (0.0, -1.0, math.inf, -math.inf, math.nan, "x", None, True):
        with pytest.raises(ValueError, match="radius"):
            check_uniform_options(DEFAULT, bad)


# ---- 4. the model carries the options ----------------------------------------------------------------------------------

def test_model_and_build_model_carry_the_options_on_cpu():
    from fpsg_amd.engine import build_model, default_options
    from fpsg_amd.few_shot import ImgPCProtoNet, check_uniform_weight
    opt = default_options(device="cpu")
    assert (opt.uniform_weight, tuple(opt.uniform_percentages), opt.uniform_radius) == (0.0, DEFAULT, 1.0)
    plain = build_model(opt)
    assert (plain.uniform_weight, plain.uniform_percentages, plain.uniform_radius) == (0.0, DEFAULT, 1.0)
    model = build_model(default_options(device="cpu", uniform_weight=0.5, uniform_percentages=[0.02, 0.05],
                                        uniform_radius=0.5, pc_dist="dcd"))
    assert (model.uniform_weight, model.uniform_percentages, model.uniform_radius) == (0.5, (0.02, 0.05), 0.5)
    direct = ImgPCProtoNet(plain.img_encoder, plain.pc_encoder, plain.pc_decoder, uniform_weight=2,
                           uniform_percentages=(1,), uniform_radius=2)
    assert (direct.uniform_weight, direct.uniform_percentages, direct.uniform_radius) == (2.0, (1.0,), 2.0)
    assert check_uniform_weight(3) == 3.0
    # an options namespace from before the flags existed builds the same model as the defaults
    old = default_options(device="cpu")
    for f in ("uniform_weight", "uniform_percentages", "uniform_radius"):
        delattr(old, f)
    built = build_model(old)
    assert (built.uniform_weight, built.uniform_percentages, built.uniform_radius) == (0.0, DEFAULT, 1.0)
    for kw, word in (({"uniform_weight": -1.0}, "uniform_weight"), ({"uniform_weight": math.nan}, "uniform_weight"),
                     ({"uniform_percentages": (0.0,)}, "percentages"), ({"uniform_percentages": (0.01,) * 9}, "percentages"),
                     ({"uniform_radius": 0.0}, "radius")):
        with pytest.raises(ValueError, match=word):
            ImgPCProtoNet(plain.img_encoder, plain.pc_encoder, plain.pc_decoder, **kw)


# ---- 5. no CPU path ------------------------------------------------------------------------------------------------------

def test_a_cpu_tensor_raises():
    from fpsg_amd._hip import FpsgHipError
    from fpsg_amd.metrics import uniform_loss
    with pytest.raises(FpsgHipError):
        uniform_loss(torch.rand(2, 64, 3))
    with pytest.raises(FpsgHipError):
        uniform_loss(torch.rand(2, 64, 3), seeds=torch.zeros((2, 3), dtype=torch.int64))
    for bad, word in ((torch.rand(2, 16, 2), "B,N,3"), (torch.rand(16, 3), "B,N,3"), (torch.rand(0, 16, 3), "empty"),
                      (torch.rand(2, 1, 3), "at least 2"), (torch.rand(1, 16385, 3), "16384")):
        with pytest.raises(ValueError, match=word):
            uniform_loss(bad)
    x = torch.rand(2, 16, 3)
    with pytest.raises(ValueError, match="percentages"):
        uniform_loss(x, percentages=(0.0,))
    with pytest.raises(ValueError, match="radius"):
        uniform_loss(x, radius=0.0)
    with pytest.raises(ValueError, match="max_members"):
        uniform_loss(x, max_members=100)
    with pytest.raises(ValueError, match="n_seeds"):
        uniform_loss(x, n_seeds=17)
    for seeds in (torch.zeros((2, 3)), torch.zeros((3, 3), dtype=torch.int64), torch.zeros((2, 17), dtype=torch.int64),
                  torch.zeros((2,), dtype=torch.int64)):
        with pytest.raises(ValueError, match="seeds"):
            uniform_loss(x, seeds=seeds)
