"""The Jensen-Shannon divergence of voxel occupancy (K15): what needs no GPU -- the retained nodes, the
divergence and the occupancy entropy from histograms, the C entry's argument checks, the ``--jsd`` flag, and the
mirror's errors."""
import ctypes
import os

import numpy as np
import pytest
import torch

import _occupancy_ref as ref
from conftest import ROOT


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    if not os.path.exists(os.path.join(ROOT, "fpsg_amd", "libfpsg_hip.so")):
        g.build()
    from fpsg_amd import _hip
    return _hip.load()


# ---- 1. retained nodes -------------------------------------------------------------------------------------------

def test_retained_nodes_counts_and_integer_rule():
    from fpsg_amd.set_metrics import retained_nodes
    assert int(retained_nodes(28).sum()) == 10144
    assert int(retained_nodes(3).sum()) == 7
    assert int(retained_nodes(64).sum()) == 130536
    for r in (2, 3, 28):
        m = retained_nodes(r, in_sphere=False)
        assert m.dtype == torch.bool and tuple(m.shape) == (r, r, r) and bool(m.all())
    for r in range(3, 33):
        want = np.zeros((r, r, r), dtype=bool)                     # the rule, node by node in Python integers
        for i in range(r):
            for j in range(r):
                for k in range(r):
                    want[i, j, k] = (2 * i - (r - 1)) ** 2 + (2 * j - (r - 1)) ** 2 + (2 * k - (r - 1)) ** 2 <= (r - 1) ** 2
        got = retained_nodes(r)
        assert got.dtype == torch.bool and np.array_equal(got.numpy(), want), r
        assert np.array_equal(ref.retained(r), want), r
    with pytest.raises(ValueError):
        retained_nodes(2)                                          # retains none
    with pytest.raises(ValueError):
        retained_nodes(1, in_sphere=False)


# ---- 2. the divergence from histograms ---------------------------------------------------------------------------

def _sparse_hist(rng, n, fill, top):
    h = rng.integers(1, top, size=n) * (rng.random(n) < fill)
    if h.sum() == 0:
        h[0] = 1
    return h.astype(np.int64)


def test_jsd_from_counts_against_numpy_and_scipy():
    from fpsg_amd.set_metrics import jsd_from_counts
    try:
        from scipy.spatial.distance import jensenshannon
    except ImportError:
        jensenshannon = None
    rng = np.random.default_rng(11)
    for n, fill, top in ((50, 0.5, 10), (21952, 0.05, 400), (21952, 0.4, 5000), (1000, 1.0, 3), (7, 0.3, 100)):
        for _ in range(4):
            g, r = _sparse_hist(rng, n, fill, top), _sparse_hist(rng, n, fill, top)
            got = jsd_from_counts(torch.from_numpy(g), torch.from_numpy(r))
            assert isinstance(got, float) and 0.0 <= got <= 1.0
            assert abs(got - ref.jsd(g, r)) <= 1e-12, (n, fill, got, ref.jsd(g, r))
            if jensenshannon is not None:
                assert abs(got - jensenshannon(g / g.sum(), r / r.sum(), base=2) ** 2) <= 1e-12
            assert got == jsd_from_counts(torch.from_numpy(r), torch.from_numpy(g))          # symmetric
            # shape does not matter, only that both agree; int32 as the kernel makes them
            side = torch.from_numpy(g).int().reshape(1, -1), torch.from_numpy(r).int().reshape(1, -1)
            assert jsd_from_counts(*side) == got


def test_jsd_from_counts_exact_zero_and_one():
    from fpsg_amd.set_metrics import jsd_from_counts
    rng = np.random.default_rng(12)
    for _ in range(8):
        p = torch.from_numpy(_sparse_hist(rng, 4000, 0.2, 300))
        assert jsd_from_counts(p, p.clone()) == 0.0
        assert jsd_from_counts(p, 7 * p) == 0.0                    # c / sum and 7c / 7 sum round alike: M = P
        q = torch.from_numpy(_sparse_hist(rng, 4000, 0.2, 300))
        a, b = torch.cat([p, torch.zeros_like(q)]), torch.cat([torch.zeros_like(p), q])
        assert abs(jsd_from_counts(a, b) - 1.0) <= 1e-12           # disjoint supports
    assert jsd_from_counts(torch.tensor([3, 0]), torch.tensor([0, 5])) == pytest.approx(1.0, abs=1e-12)


def test_jsd_from_counts_refuses_bad_input():
    from fpsg_amd.set_metrics import jsd_from_counts
    with pytest.raises(ValueError):
        jsd_from_counts(torch.ones(8), torch.ones(9))
    with pytest.raises(ValueError):
        jsd_from_counts(torch.ones(2, 4), torch.ones(4, 2))
    with pytest.raises(ValueError):
        jsd_from_counts(torch.zeros(8), torch.ones(8))
    with pytest.raises(ValueError):
        jsd_from_counts(torch.ones(8), torch.zeros(8, dtype=torch.int32))


# ---- 3. the occupancy entropy ------------------------------------------------------------------------------------

def test_occupancy_entropy_from_counts_hand_built():
    from fpsg_amd.set_metrics import occupancy_entropy_from_counts, retained_nodes
    keep = retained_nodes(3)                                       # 7 nodes: the centre and its six neighbours
    hit = torch.zeros((3, 3, 3), dtype=torch.int32)
    assert occupancy_entropy_from_counts(hit, 10, keep) == 0.0     # no cloud hits anything
    hit[keep] = 10
    assert occupancy_entropy_from_counts(hit, 10, keep) == 0.0     # every cloud hits every node
    hit[keep] = 0
    hit[1, 1, 1] = 5
    assert occupancy_entropy_from_counts(hit, 10, keep) == pytest.approx(1.0 / 7, abs=1e-15)   # one bit at one of 7
    hit[0, 1, 1] = 5
    hit[0, 0, 0] = 5                                               # not retained: ignored
    assert occupancy_entropy_from_counts(hit, 10, keep) == pytest.approx(2.0 / 7, abs=1e-15)
    hit[1, 1, 2] = 1
    h = -(0.1 * np.log2(0.1) + 0.9 * np.log2(0.9))
    assert occupancy_entropy_from_counts(hit, 10, keep) == pytest.approx((2.0 + h) / 7, abs=1e-15)
    allk = retained_nodes(2, in_sphere=False)
    assert occupancy_entropy_from_counts(torch.tensor([2, 0, 0, 0, 4, 0, 0, 0]).reshape(2, 2, 2), 4, allk) == \
        pytest.approx(1.0 / 8, abs=1e-15)                          # mean over all 8 nodes
    with pytest.raises(ValueError):
        occupancy_entropy_from_counts(hit, 0, keep)
    with pytest.raises(ValueError):
        occupancy_entropy_from_counts(hit, 10, retained_nodes(4))


# ---- 4. the C entry's argument checks ----------------------------------------------------------------------------

def test_occupancy_entry_checks_its_arguments_on_the_host(lib):
    """Every refusal of fpsg_occupancy_grid comes before any HIP call (no GPU here), with its code and a message."""
    f = ctypes.c_float
    P, Q = 0x10000, 0x10002                                        # never dereferenced: aligned / misaligned fakes

    def call(xyz=P, S=4, N=100, res=28, E=1.0, sph=1, counts=P, hit=P, outside=P, cells=None):
        return lib.fpsg_occupancy_grid(xyz, S, N, res, f(E), sph, counts, hit, outside, cells, None, 0, None)

    null, shape, align, limit = -1, -2, -3, -4
    for kw in ({"xyz": None}, {"counts": None}, {"hit": None}, {"outside": None}):
        assert call(**kw) == null and b"null pointer" in lib.fpsg_last_error(), kw
    for kw in ({"xyz": Q}, {"counts": Q}, {"hit": Q}, {"outside": Q}, {"cells": Q}):
        assert call(**kw) == align and b"aligned" in lib.fpsg_last_error(), kw
    for kw in ({"S": 0}, {"N": 0}, {"S": -3}, {"N": -1}, {"E": 0.0}, {"E": -1.0}, {"E": float("inf")},
               {"E": float("nan")}, {"E": 1e-44}, {"res": 1}, {"res": 0}, {"res": -5}, {"res": 2}):
        assert call(**kw) == shape, kw
        assert b"fpsg_occupancy_grid" in lib.fpsg_last_error(), kw
    assert b"res" in lib.fpsg_last_error()
    for kw in ({"res": 65}, {"res": 1000}, {"res": 65, "sph": 0}):
        assert call(**kw) == limit and b"64" in lib.fpsg_last_error(), kw
    # shape and limit refusals do not need pointers at all
    assert lib.fpsg_occupancy_grid(None, 0, 8, 28, f(1), 1, None, None, None, None, None, 0, None) == shape
    assert lib.fpsg_occupancy_grid(None, 1, 8, 99, f(1), 1, None, None, None, None, None, 0, None) == limit
    assert lib.fpsg_occupancy_grid(None, 1, 8, 28, f(1), 1, None, None, None, None, None, 0, None) == null
    # the kernel keeps everything transient in LDS: no workspace, answered on the host
    for args in ((1, 1, 2), (370, 2048, 28), (300, 5000, 64)):
        assert lib.fpsg_occupancy_grid_workspace_bytes(*args) == 0


# ---- 5. the flag -------------------------------------------------------------------------------------------------

def test_jsd_flag_parses_and_changes_nothing_else():
    from fpsg_amd import cli
    p = cli.few_shot_parser(evaluation=True)
    base, on = vars(p.parse_args([])), vars(p.parse_args(["--jsd"]))
    assert base["jsd"] is False and on["jsd"] is True
    assert {k: v for k, v in on.items() if k != "jsd"} == {k: v for k, v in base.items() if k != "jsd"}
    both = p.parse_args(["--jsd", "--set_metrics", "--set_metrics_emd", "--exact_emd"])
    assert both.jsd and both.set_metrics and both.set_metrics_emd and both.exact_emd
    train = cli.few_shot_parser()
    assert "jsd" not in vars(train.parse_args([]))
    with pytest.raises(SystemExit):
        train.parse_args(["--jsd"])
    assert {k: v for k, v in base.items() if k in vars(train.parse_args([]))} == vars(train.parse_args([]))


# ---- 6. the mirror's errors --------------------------------------------------------------------------------------

def test_occupancy_grid_has_no_cpu_path_and_checks_first():
    from fpsg_amd._hip import FpsgHipError
    from fpsg_amd.metrics import occupancy_grid
    from fpsg_amd.set_metrics import jsd
    x = torch.rand(2, 16, 3)
    with pytest.raises(FpsgHipError):
        occupancy_grid(x)
    with pytest.raises(FpsgHipError):
        jsd(x, x)
    for bad in (torch.rand(16, 3), torch.rand(2, 16, 2), torch.rand(0, 16, 3), torch.rand(2, 0, 3)):
        with pytest.raises(ValueError):
            occupancy_grid(bad)
    for kw in ({"resolution": 1}, {"resolution": 65}, {"resolution": 2}, {"resolution": 28.5}, {"half_extent": 0.0},
               {"half_extent": -1.0}, {"half_extent": float("inf")}, {"half_extent": float("nan")}):
        with pytest.raises(ValueError):
            occupancy_grid(x, **kw)
    earlier = {"resolution": 28, "half_extent": 1.0, "in_sphere": True, "counts": torch.zeros(28, 28, 28, dtype=torch.int32)}
    for kw in ({"resolution": 27}, {"half_extent": 0.5}, {"in_sphere": False}):
        with pytest.raises(ValueError):                            # a parameter mismatch with out=
            occupancy_grid(x, out=earlier, **kw)
