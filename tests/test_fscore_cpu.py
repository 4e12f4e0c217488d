"""F-score at distance thresholds and the Hausdorff distance (K17): what needs no GPU -- precision, recall and
F from counts, the C entry's argument checks, the ``--fscore`` flag, and the mirrors' errors."""
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


# ---- 1. precision, recall and F from counts ----------------------------------------------------------------------

def test_fscore_from_counts_hand_made():
    from fpsg_amd.metrics import fscore_from_counts
    # pair 0: P = R = 1; pair 1: P = R = 0; pair 2: P = 1/2, R = 1/4; pair 3: P = 0, R = 1; second column: all / none
    counts = torch.tensor([[[8, 8], [4, 4]], [[0, 8], [0, 4]], [[4, 0], [1, 0]], [[0, 8], [4, 0]]])
    for c in (counts, counts.int(), counts.short()):
        out = fscore_from_counts(c, 8, 4)
        assert set(out) == {"precision", "recall", "fscore"}
        for v in out.values():
            assert v.dtype == torch.float64 and tuple(v.shape) == (4, 2)
        assert out["precision"].tolist() == [[1.0, 1.0], [0.0, 1.0], [0.5, 0.0], [0.0, 1.0]]
        assert out["recall"].tolist() == [[1.0, 1.0], [0.0, 1.0], [0.25, 0.0], [1.0, 0.0]]
        f = out["fscore"].tolist()
        assert f[0] == [1.0, 1.0]
        assert f[1][0] == 0.0 and f[2][1] == 0.0 and f[3] == [0.0, 0.0]      # exactly 0.0, no NaN anywhere
        assert not torch.isnan(out["fscore"]).any()
        p, r = 0.5, 0.25
        assert f[2][0] == 2 * p * r / (p + r)                                # 1/3 to the last bit, same order
        assert abs(f[2][0] - 1.0 / 3.0) <= 2.0 ** -53
    a, b = fscore_from_counts(counts.int(), 8, 4), fscore_from_counts(counts.long(), 8, 4)
    for k in a:
        assert torch.equal(a[k], b[k]), k
    # thirds and sevenths: the quotients are float64's own
    out = fscore_from_counts(torch.tensor([[[1, 2], [3, 6]]], dtype=torch.int32), 3, 7)
    assert out["precision"].tolist() == [[1 / 3, 2 / 3]] and out["recall"].tolist() == [[3 / 7, 6 / 7]]
    p, r = 1 / 3, 3 / 7
    assert out["fscore"][0, 0].item() == 2 * p * r / (p + r)


def test_fscore_from_counts_refuses_bad_input():
    from fpsg_amd.metrics import fscore_from_counts
    good = torch.tensor([[[1, 2], [0, 3]]])
    fscore_from_counts(good, 2, 3)
    for bad in (good[0], good[None], torch.zeros(2, 3, 4, dtype=torch.int64), good.double(), good.bool()):
        with pytest.raises(ValueError):
            fscore_from_counts(bad, 2, 3)
    for n1, n2 in ((0, 3), (2, 0), (-1, 3), (2, -4), (2.5, 3)):
        with pytest.raises(ValueError):
            fscore_from_counts(good, n1, n2)
    with pytest.raises(ValueError):
        fscore_from_counts(good, 1, 3)                                        # a count above n1
    with pytest.raises(ValueError):
        fscore_from_counts(good, 2, 2)                                        # a count above n2
    with pytest.raises(ValueError):
        fscore_from_counts(torch.tensor([[[1, -1], [0, 3]]]), 2, 3)           # a negative count


# ---- 2. the C entry's argument checks ----------------------------------------------------------------------------

def test_dist_profile_entry_checks_its_arguments_on_the_host(lib):
    """Every refusal of fpsg_dist_profile comes before any HIP call (no GPU here), with its code and a message."""
    P, Q = 0x10000, 0x10002                                        # never dereferenced: aligned / misaligned fakes

    def call(d1=P, d2=P, B=5, N=2048, M=2048, tau2=P, T=3, counts=P, maxima=P):
        return lib.fpsg_dist_profile(d1, d2, B, N, M, tau2, T, counts, maxima, None)

    null, shape, align, limit = -1, -2, -3, -4
    for kw in ({"B": 0}, {"N": 0}, {"M": 0}, {"T": 0}, {"B": -2}, {"N": -1}, {"M": -7}, {"T": -1}):
        assert call(**kw) == shape, kw
        assert b"fpsg_dist_profile" in lib.fpsg_last_error(), kw
    for kw in ({"T": 17}, {"T": 1000}):
        assert call(**kw) == limit and b"16" in lib.fpsg_last_error(), kw
    assert call(T=16, d1=None) == null                             # 16 itself is within the limit
    for kw in ({"d1": None}, {"d2": None}, {"tau2": None}, {"counts": None}, {"maxima": None}):
        assert call(**kw) == null and b"null pointer" in lib.fpsg_last_error(), kw
    for kw in ({"d1": Q}, {"d2": Q}, {"tau2": Q}, {"counts": Q}, {"maxima": Q}, {"d1": 0x10001}, {"maxima": 0x10003}):
        assert call(**kw) == align and b"aligned" in lib.fpsg_last_error(), kw
    # the header's order: shape, limit, null, alignment -- whichever pointers are bad
    assert call(B=0, T=17, d1=None, d2=Q) == shape
    assert call(T=17, d1=None, d2=Q) == limit
    assert call(d1=Q, maxima=None) == null
    assert lib.fpsg_dist_profile(None, None, 1, 1, 0, None, 1, None, None, None) == shape
    assert lib.fpsg_dist_profile(None, None, 1, 1, 1, None, 99, None, None, None) == limit
    assert lib.fpsg_dist_profile(None, None, 1, 1, 1, None, 1, None, None, None) == null


def test_profile_limit_is_the_headers():
    from fpsg_amd import metrics
    text = open(os.path.join(ROOT, "include", "fpsg_hip.h")).read()
    assert f"#define FPSG_PROFILE_MAX_T {metrics.PROFILE_MAX_T}\n" in text and metrics.PROFILE_MAX_T == 16


# ---- 3. the flag -------------------------------------------------------------------------------------------------

def _opt(extra):
    from fpsg_amd import cli
    return cli.few_shot_parser(evaluation=True).parse_args(["--synthetic"] + extra)


def test_fscore_flag_parses_and_changes_nothing_else():
    from fpsg_amd import cli
    p = cli.few_shot_parser(evaluation=True)
    base, on = vars(p.parse_args([])), vars(p.parse_args(["--fscore", "0.01", "0.02"]))
    assert base["fscore"] is None and on["fscore"] == [0.01, 0.02]
    assert all(type(v) is float for v in on["fscore"])
    assert {k: v for k, v in on.items() if k != "fscore"} == {k: v for k, v in base.items() if k != "fscore"}
    assert p.parse_args(["--fscore", "0.05", "--jsd"]).fscore == [0.05]
    assert "unit ball" in " ".join(p.format_help().split()) and "--fscore TAU [TAU ...]" in p.format_help()
    with pytest.raises(SystemExit):
        p.parse_args(["--fscore"])                                 # at least one value
    train = cli.few_shot_parser()
    assert "fscore" not in vars(train.parse_args([]))
    with pytest.raises(SystemExit):
        train.parse_args(["--fscore", "0.01"])


def test_validate_refuses_bad_thresholds():
    from fpsg_amd import cli
    cli.validate(_opt([]))
    cli.validate(_opt(["--fscore", "0.01", "0.02"]))
    cli.validate(_opt(["--fscore", "0", "0.5"]))
    cli.validate(_opt(["--fscore"] + ["0.01"] * 16))
    for extra, word in ((["--fscore", "-0.1"], "non-negative"), (["--fscore", "0.01", "nan"], "finite"),
                        (["--fscore", "inf"], "finite"),
                        (["--fscore"] + ["0.01"] * 17, "at most 16")):
        with pytest.raises(SystemExit) as e:
            cli.validate(_opt(extra))
        assert "--fscore" in str(e.value) and word in str(e.value), (extra, str(e.value))


# ---- 4. the mirrors' errors --------------------------------------------------------------------------------------

BAD_THRESHOLDS = ([], [0.01] * 17, [-0.1], [0.01, float("nan")], [float("inf")], [-float("inf")], 0.02, "0.02",
                  [None], ["a"], None)


def test_thresholds_are_checked_before_the_library_is_touched(monkeypatch):
    from fpsg_amd import _hip, metrics

    def no_library():
        raise AssertionError("the library was loaded before the thresholds were checked")

    monkeypatch.setattr(_hip, "load", no_library)
    d1, d2 = torch.rand(2, 16), torch.rand(2, 8)                   # CPU tensors: a good list would raise FpsgHipError
    p1, p2 = torch.rand(2, 16, 3), torch.rand(2, 8, 3)
    for bad in BAD_THRESHOLDS:
        with pytest.raises(ValueError):
            metrics.distance_profile(d1, d2, bad)
        with pytest.raises(ValueError):
            metrics.fscore(p1, p2, bad)
        with pytest.raises(ValueError):
            metrics.check_thresholds(bad)
    assert metrics.check_thresholds([0, 0.5, 1]) == (0.0, 0.5, 1.0)
    assert metrics.check_thresholds((0.02,)) == (0.02,)


def test_distance_profile_and_fscore_have_no_cpu_path():
    from fpsg_amd._hip import FpsgHipError
    from fpsg_amd.metrics import distance_profile, fscore
    with pytest.raises(FpsgHipError):
        distance_profile(torch.rand(2, 16), torch.rand(2, 8), [0.02])
    with pytest.raises(FpsgHipError):
        fscore(torch.rand(2, 16, 3), torch.rand(2, 8, 3), [0.02, 0.05])
    for d1, d2 in ((torch.rand(16), torch.rand(2, 8)), (torch.rand(2, 16), torch.rand(3, 8)),
                   (torch.rand(2, 0), torch.rand(2, 8)), (torch.rand(2, 16, 1), torch.rand(2, 8))):
        with pytest.raises(ValueError):
            distance_profile(d1, d2, [0.02])
    for p1, p2 in ((torch.rand(16, 3), torch.rand(16, 3)), (torch.rand(2, 16, 2), torch.rand(2, 8, 3)),
                   (torch.rand(2, 16, 3), torch.rand(3, 8, 3))):
        with pytest.raises(ValueError):
            fscore(p1, p2, [0.02])


def test_eval_item_checks_its_thresholds():
    from fpsg_amd.engine import EvalItem, build_model, default_options
    model = build_model(default_options(device="cpu")).eval()
    assert EvalItem(model).fscore is None
    assert EvalItem(model, fscore=[0.02, 0.05]).fscore == (0.02, 0.05)
    for bad in ([], [-1.0], [float("nan")], [0.01] * 17):
        with pytest.raises(ValueError):
            EvalItem(model, fscore=bad)
