"""Farthest point sampling without a GPU: the refusals of the C entry (K16) and of its Python wrapper that answer
before any launch, and the --set_metrics_points flag."""
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

def test_fps_entry_checks_its_arguments_on_the_host(lib):
    """Every refusal of fpsg_fps comes before any HIP call (no GPU here), with its code and a message."""
    P, Q = 0x10000, 0x10002                                        # never dereferenced: aligned / misaligned fakes

    def call(xyz=P, B=4, N=100, n=10, start=None, idx=P, md=None):
        return lib.fpsg_fps(xyz, B, N, n, start, idx, md, None, 0, None)

    null, shape, align, limit = -1, -2, -3, -4
    for kw in ({"xyz": None}, {"idx": None}):
        assert call(**kw) == null and b"null pointer" in lib.fpsg_last_error(), kw
    for kw in ({"xyz": Q}, {"idx": Q}, {"start": Q}, {"md": Q}):
        assert call(**kw) == align and b"aligned" in lib.fpsg_last_error(), kw
    for kw in ({"B": 0}, {"B": -2}, {"N": 0}, {"n": 0}, {"n": -1}, {"n": 101}, {"N": 16384, "n": 16385}):
        assert call(**kw) == shape, kw
        assert b"fpsg_fps" in lib.fpsg_last_error(), kw
    for kw in ({"N": 16385}, {"N": 16385, "n": 16385}, {"N": 1 << 20, "n": 1}):
        assert call(**kw) == limit and b"16384" in lib.fpsg_last_error(), kw
    # shape and limit refusals do not need pointers at all
    assert lib.fpsg_fps(None, 0, 8, 4, None, None, None, None, 0, None) == shape
    assert lib.fpsg_fps(None, 1, 16385, 4, None, None, None, None, 0, None) == limit
    assert lib.fpsg_fps(None, 1, 8, 4, None, None, None, None, 0, None) == null
    # registers and LDS only: no workspace, answered on the host
    for args in ((1, 1, 1), (37, 2048, 512), (5, 15000, 2048), (3, 16384, 64)):
        assert lib.fpsg_fps_workspace_bytes(*args) == 0


# ---- 2. the wrapper's errors -------------------------------------------------------------------------------------

def test_farthest_point_sample_has_no_cpu_path_and_checks_first():
    from fpsg_amd._hip import FpsgHipError
    from fpsg_amd.sampling import FPS_MAX_N, farthest_point_sample, farthest_point_subsample
    assert FPS_MAX_N == 16384
    x = torch.rand(2, 16, 3)
    for kw in ({}, {"start": 3}, {"start": torch.tensor([0, 15])}, {"return_min_dist": True}):
        with pytest.raises(FpsgHipError):
            farthest_point_sample(x, 4, **kw)
    with pytest.raises(FpsgHipError):
        farthest_point_subsample(x, 4)
    for bad in (torch.rand(16, 3), torch.rand(2, 16, 2), torch.rand(0, 16, 3), torch.rand(2, 0, 3)):
        with pytest.raises(ValueError):
            farthest_point_sample(bad, 1)
    for n in (0, -1, 17, 2.5):
        with pytest.raises(ValueError):
            farthest_point_sample(x, n)
    with pytest.raises(ValueError, match="16384"):
        farthest_point_sample(torch.zeros(1, 16385, 3), 4)
    for start in (-1, 16, 1.5, torch.tensor([0]), torch.tensor([[0, 1]]), torch.tensor([0, 16]), torch.tensor([-1, 0]),
                  torch.tensor([0.0, 1.0])):
        with pytest.raises(ValueError):
            farthest_point_sample(x, 4, start=start)
        with pytest.raises(ValueError):
            farthest_point_subsample(x, 4, start=start)


# ---- 3. the flag -------------------------------------------------------------------------------------------------

def test_set_metrics_points_flag_parses_in_evaluation_mode_only():
    from fpsg_amd import cli
    p = cli.few_shot_parser(evaluation=True)
    base, on = vars(p.parse_args([])), vars(p.parse_args(["--set_metrics_points", "512"]))
    assert base["set_metrics_points"] is None and on["set_metrics_points"] == 512
    assert {k: v for k, v in on.items() if k != "set_metrics_points"} == \
        {k: v for k, v in base.items() if k != "set_metrics_points"}
    train = cli.few_shot_parser()
    assert "set_metrics_points" not in vars(train.parse_args([]))
    with pytest.raises(SystemExit):
        train.parse_args(["--set_metrics_points", "512"])
    with pytest.raises(SystemExit):
        p.parse_args(["--set_metrics_points", "many"])


def test_validate_wants_a_set_flag_and_a_positive_count():
    from fpsg_amd import cli
    p = cli.few_shot_parser(evaluation=True)
    for flags in (["--set_metrics"], ["--set_metrics_emd"], ["--set_metrics", "--set_metrics_emd", "--jsd"]):
        cli.validate(p.parse_args(["--synthetic", "--set_metrics_points", "512"] + flags))
        cli.validate(p.parse_args(["--synthetic"] + flags))
        for bad in ("0", "-4"):
            with pytest.raises(SystemExit, match="at least 1"):
                cli.validate(p.parse_args(["--synthetic", "--set_metrics_points", bad] + flags))
    for flags in ([], ["--jsd"], ["--exact_emd"]):
        with pytest.raises(SystemExit, match="--set_metrics"):
            cli.validate(p.parse_args(["--synthetic", "--set_metrics_points", "512"] + flags))
    cli.validate(cli.few_shot_parser().parse_args(["--synthetic"]))      # the training parsers have no such option
