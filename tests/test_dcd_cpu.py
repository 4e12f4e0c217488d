"""Density-aware Chamfer distance (K18): what needs no GPU -- the C entry's argument checks, the mirror's
errors and their order, the ``--pc_dist dcd`` / ``--dcd_alpha`` / ``--dcd`` flags and the model's constructor."""
import math
import os

import pytest
import torch

from conftest import ROOT


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    if not os.path.exists(os.path.join(ROOT, "fpsg_amd", "libfpsg_hip.so")):
        g.build()
    from fpsg_amd import _hip
    return _hip.load()


# ---- 1. the C entry's argument checks ----------------------------------------------------------------------------

def test_dcd_entry_checks_its_arguments_on_the_host(lib):
    """Every refusal of fpsg_dcd comes before any HIP call (no GPU here), with its code and a message."""
    P, Q = 0x10000, 0x10002                                        # never dereferenced: aligned / misaligned fakes
    names = ("dist1", "idx1", "dist2", "idx2", "out", "sides", "deg1", "deg2")

    def call(B=5, N=2048, M=2048, alpha=1000.0, w1=P, w2=P, **ptrs):
        a = {n: P for n in names}
        a.update(ptrs)
        return lib.fpsg_dcd(a["dist1"], a["idx1"], a["dist2"], a["idx2"], B, N, M, alpha, a["out"], a["sides"],
                            a["deg1"], a["deg2"], w1, w2, None)

    null, shape, align, limit = -1, -2, -3, -4
    for n in names:
        assert call(**{n: None}) == null, n
        msg = lib.fpsg_last_error()
        assert b"fpsg_dcd" in msg and b"null pointer" in msg and n.encode() in msg, (n, msg)
    for kw in ({"B": 0}, {"N": 0}, {"M": 0}, {"B": -2}, {"N": -1}, {"M": -7}):
        assert call(**kw) == shape, kw
        assert b"fpsg_dcd" in lib.fpsg_last_error(), kw
    for kw in ({"N": 16385}, {"M": 16385}, {"N": 1 << 20, "M": 1 << 20}, {"N": 2 ** 31 - 1}):
        assert call(**kw) == limit and b"16384" in lib.fpsg_last_error(), kw
    for n in names:
        assert call(**{n: Q}) == align and b"aligned" in lib.fpsg_last_error(), n
    assert call(w1=Q) == align and call(w2=0x10001) == align
    # the header's order: null, shape, limit, alignment -- whichever else is bad; the limit itself is accepted
    assert call(B=0, N=16385, out=None, sides=Q) == null
    assert call(B=0, N=16385, sides=Q) == shape
    assert call(N=16385, sides=Q) == limit
    assert call(N=16384, M=16384, sides=Q) == align
    assert call(N=16384, M=16384, w1=None, w2=None, sides=Q) == align        # w1 and w2 may be null


def test_dcd_limit_is_the_headers():
    from fpsg_amd import metrics
    text = open(os.path.join(ROOT, "include", "fpsg_hip.h")).read()
    assert f"#define FPSG_DCD_MAX_N {metrics.DCD_MAX_N}\n" in text and metrics.DCD_MAX_N == 16384
    assert metrics.DCD_DEFAULT_ALPHA == 1000.0


def test_dcd_is_bound_like_the_header_declares():
    import ctypes
    from fpsg_amd import _hip
    sig = _hip.SIGNATURES["fpsg_dcd"]
    assert len(sig) == 15 and sig[7] is ctypes.c_float and sig[4:7] == [ctypes.c_int] * 3
    text = open(os.path.join(ROOT, "include", "fpsg_hip.h")).read()
    decl = text[text.index("int fpsg_dcd("):]
    decl = decl[:decl.index(";")]
    assert decl.count(",") == 14 and "float alpha" in decl


# ---- 2. the mirror's errors --------------------------------------------------------------------------------------

BAD_ALPHAS = (-1.0, -1e-30, float("nan"), float("inf"), -float("inf"), None, "a", [1.0])


def test_dcd_value_errors_come_before_the_library_is_touched(monkeypatch):
    from fpsg_amd import _hip, metrics

    def no_library():
        raise AssertionError("the library was loaded before the arguments were checked")

    monkeypatch.setattr(_hip, "load", no_library)
    p1, p2 = torch.rand(2, 16, 3), torch.rand(2, 8, 3)             # CPU tensors: good arguments would raise FpsgHipError
    for bad in BAD_ALPHAS:
        with pytest.raises(ValueError):
            metrics.dcd(p1, p2, alpha=bad)
        with pytest.raises(ValueError):
            metrics.check_dcd_alpha(bad)
    assert metrics.check_dcd_alpha(0) == 0.0 and metrics.check_dcd_alpha(40) == 40.0
    assert type(metrics.check_dcd_alpha(1)) is float
    for a, b in ((torch.rand(16, 3), torch.rand(16, 3)), (torch.rand(2, 16, 2), torch.rand(2, 8, 3)),
                 (torch.rand(2, 16, 3), torch.rand(3, 8, 3)), (torch.rand(2, 0, 3), torch.rand(2, 8, 3)),
                 (torch.rand(2, 16, 3), torch.rand(2, 0, 3)), (torch.rand(0, 16, 3), torch.rand(0, 8, 3)),
                 (torch.rand(1, 16385, 3), torch.rand(1, 8, 3)), (torch.rand(1, 8, 3), torch.rand(1, 16385, 3)),
                 (None, p2), (p1, [[0.0, 0.0, 0.0]])):
        with pytest.raises(ValueError):
            metrics.dcd(a, b)
        with pytest.raises(ValueError):
            metrics.dcd(a, b, return_info=True)
    # a bad alpha is named even when the clouds are bad too: it is checked first
    with pytest.raises(ValueError, match="alpha"):
        metrics.dcd(torch.rand(16, 3), p2, alpha=-1.0)


def test_dcd_has_no_cpu_path():
    from fpsg_amd._hip import FpsgHipError
    from fpsg_amd.metrics import dcd
    with pytest.raises(FpsgHipError):
        dcd(torch.rand(2, 16, 3), torch.rand(2, 8, 3))
    with pytest.raises(FpsgHipError):
        dcd(torch.rand(1, 16384, 3), torch.rand(1, 1, 3), alpha=0.0, return_info=True)      # the limit itself passes
    with pytest.raises(FpsgHipError):
        dcd(torch.rand(2, 16, 3, requires_grad=True), torch.rand(2, 8, 3), alpha=40)


# ---- 3. the flags ------------------------------------------------------------------------------------------------

def test_training_flags_parse_and_keep_their_defaults():
    from fpsg_amd import cli
    for evaluation in (False, True):
        p = cli.few_shot_parser(evaluation=evaluation)
        base = vars(p.parse_args([]))
        assert base["pc_dist"] == "cd" and base["dcd_alpha"] == 1000.0 and type(base["dcd_alpha"]) is float
        on = vars(p.parse_args(["--pc_dist", "dcd", "--dcd_alpha", "40"]))
        assert on["pc_dist"] == "dcd" and on["dcd_alpha"] == 40.0 and type(on["dcd_alpha"]) is float
        assert {k: v for k, v in on.items() if k not in ("pc_dist", "dcd_alpha")} == \
            {k: v for k, v in base.items() if k not in ("pc_dist", "dcd_alpha")}
        assert p.parse_args(["--pc_dist", "emd"]).pc_dist == "emd"
        with pytest.raises(SystemExit):
            p.parse_args(["--pc_dist", "x"])
        with pytest.raises(SystemExit):
            p.parse_args(["--dcd_alpha"])


def test_dcd_flag_parses_and_changes_nothing_else():
    from fpsg_amd import cli
    p = cli.few_shot_parser(evaluation=True)
    base = vars(p.parse_args([]))
    assert base["dcd"] is None
    for args, want in ((["--dcd"], 1000.0), (["--dcd", "40"], 40.0), (["--dcd", "--jsd"], 1000.0),
                       (["--fscore", "0.02", "--dcd", "0.5"], 0.5)):
        on = vars(p.parse_args(args))
        assert on["dcd"] == want and type(on["dcd"]) is float, args
    on = vars(p.parse_args(["--dcd"]))
    assert {k: v for k, v in on.items() if k != "dcd"} == {k: v for k, v in base.items() if k != "dcd"}
    assert "--dcd [ALPHA]" in p.format_help()
    train = cli.few_shot_parser()
    assert "dcd" not in vars(train.parse_args([]))
    with pytest.raises(SystemExit):
        train.parse_args(["--dcd"])


def test_validate_refuses_bad_alphas():
    from fpsg_amd import cli
    ev = cli.few_shot_parser(evaluation=True)
    tr = cli.few_shot_parser()
    cli.validate(ev.parse_args(["--synthetic"]))
    cli.validate(ev.parse_args(["--synthetic", "--dcd"]))
    cli.validate(ev.parse_args(["--synthetic", "--dcd", "0"]))
    cli.validate(tr.parse_args(["--synthetic", "--pc_dist", "dcd", "--dcd_alpha", "40"]))
    for parser, extra, flag in ((ev, ["--dcd", "-1"], "--dcd"), (ev, ["--dcd", "nan"], "--dcd"),
                                (ev, ["--dcd", "inf"], "--dcd"), (tr, ["--dcd_alpha", "-3"], "--dcd_alpha"),
                                (tr, ["--pc_dist", "dcd", "--dcd_alpha", "nan"], "--dcd_alpha")):
        with pytest.raises(SystemExit) as e:
            cli.validate(parser.parse_args(["--synthetic"] + extra))
        assert flag in str(e.value), (extra, str(e.value))


# ---- 4. the model and the evaluation item ------------------------------------------------------------------------

def test_model_takes_the_dcd_metric():
    from fpsg_amd.engine import build_model, default_options
    from fpsg_amd.few_shot import ImgPCProtoNet
    from fpsg_amd.metrics import chamfer_distance
    base = build_model(default_options(device="cpu"))
    assert base.pc_metric is chamfer_distance                        # the default is untouched
    m = ImgPCProtoNet(base.img_encoder, base.pc_encoder, base.pc_decoder, metric="dcd")
    assert m.dcd_alpha == 1000.0 and m.pc_metric is not chamfer_distance
    m = ImgPCProtoNet(base.img_encoder, base.pc_encoder, base.pc_decoder, metric="dcd", dcd_alpha=40)
    assert m.dcd_alpha == 40.0
    assert build_model(default_options(device="cpu", pc_dist="dcd", dcd_alpha=7.0)).dcd_alpha == 7.0
    assert build_model(default_options(device="cpu", pc_dist="dcd")).dcd_alpha == 1000.0
    ImgPCProtoNet(base.img_encoder, base.pc_encoder, base.pc_decoder, metric="emd")
    with pytest.raises(NotImplementedError):
        ImgPCProtoNet(base.img_encoder, base.pc_encoder, base.pc_decoder, metric="x")
    for bad in (-1.0, float("nan"), math.inf):
        with pytest.raises(ValueError):
            ImgPCProtoNet(base.img_encoder, base.pc_encoder, base.pc_decoder, metric="dcd", dcd_alpha=bad)


def test_eval_item_checks_its_alpha():
    from fpsg_amd.engine import EvalItem, build_model, default_options
    model = build_model(default_options(device="cpu")).eval()
    assert EvalItem(model).dcd is None
    assert EvalItem(model, dcd=1000.0).dcd == 1000.0 and EvalItem(model, dcd=0).dcd == 0.0
    for bad in (-1.0, float("nan"), float("inf"), "a"):
        with pytest.raises(ValueError):
            EvalItem(model, dcd=bad)
