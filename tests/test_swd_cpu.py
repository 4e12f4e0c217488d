"""The sliced Wasserstein distance (K22): what needs no GPU -- the numpy references against a brute force and
central differences, the direction lattice, the library's symbols and refusals, the option checks, the flags, and the
options on a CPU model."""
import ctypes
import os

import numpy as np
import pytest
import torch

from conftest import ROOT

import _swd_ref as ref

FLAGS = ("swd_n_proj", "swd_directions")


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    if not os.path.exists(os.path.join(ROOT, "fpsg_amd", "libfpsg_hip.so")):
        g.build()
    from fpsg_amd import _hip
    return _hip.load()


# ---- 1. the references -------------------------------------------------------------------------------------------------

def test_sorted_matching_is_the_optimal_one():
    """(a) N = 5, L = 3: the rank-by-rank matching costs what the cheapest of all 120 matchings costs, per direction."""
    rng = np.random.default_rng(0)
    x, y = rng.standard_normal((5, 3)), rng.standard_normal((5, 3)) + 0.5
    dirs = ref.lattice(3)
    value = ref.ref_f64(x, y, dirs)[0]
    brute = ref.brute_force(x, y, dirs)
    assert value > 0 and abs(value - brute) <= 1e-14 * brute
    assert abs(ref.value_f64(x, y, dirs) - value) <= 1e-14 * value
    # any other matching is dearer: the identity matching here
    kx, ky = ref.keys64(x, dirs), ref.keys64(y, dirs)
    assert float(((kx - ky) ** 2).sum()) / kx.size > value


def test_reference_gradient_agrees_with_central_differences():
    """(b) float64, a generic cloud (no ties: the matchings are constant in a neighbourhood)."""
    rng = np.random.default_rng(1)
    x, y = rng.standard_normal((12, 3)), rng.standard_normal((12, 3)) * 0.7 + 0.1
    dirs = ref.lattice(7)
    _, gx, gy, _, _ = ref.ref_f64(x, y, dirs)
    h = 1e-6
    for cloud, grad, first in ((x, gx, True), (y, gy, False)):
        num = np.zeros_like(cloud)
        for i in range(cloud.shape[0]):
            for c in range(3):
                up, dn = cloud.copy(), cloud.copy()
                up[i, c] += h
                dn[i, c] -= h
                f = (lambda q: ref.value_f64(q, y, dirs)) if first else (lambda q: ref.value_f64(x, q, dirs))
                num[i, c] = (f(up) - f(dn)) / (2 * h)
        assert np.abs(grad).max() > 0
        assert np.abs(num - grad).max() <= 1e-8 * np.abs(grad).max()


def test_fp32_keys_reference_orders_ties_by_index_and_stays_close_to_float64():
    x = np.zeros((6, 3), dtype=np.float32)
    x[:, 0] = [2, 1, 1, 0, 2, 1]
    y = x[::-1].copy()
    dirs = np.array([[1, 0, 0], [0, 1, 0], [-1, 0, 0]], dtype=np.float32)
    value, gx, gy, p1, p2 = ref.ref_keys32(x, y, dirs)
    assert p1.tolist() == [[3, 1, 2, 5, 0, 4], [0, 1, 2, 3, 4, 5], [0, 4, 1, 2, 5, 3]]
    assert p2.tolist() == [[2, 0, 3, 4, 1, 5], [0, 1, 2, 3, 4, 5], [1, 5, 0, 3, 4, 2]]
    assert value == 0.0 and not gx.any() and not gy.any()            # the same multiset of keys: distance 0
    # -0 keys (0 * -1) sort with +0 keys by index, not in front of them
    assert ref.keys32(x, dirs)[2, 3] == 0 and not np.signbit(ref.keys32(x, dirs)[2, 3])
    a, b = ref.clouds(1, 257, 3)
    d = ref.unit_directions(5, 4)
    v32, v64 = ref.ref_keys32(a[0], b[0], d)[0], ref.ref_f64(a[0], b[0], d)[0]
    assert abs(v32 - v64) <= 1e-6 * v64


# ---- 2. the lattice ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("L", [1, 2, 64, 128, 1024])
def test_lattice_is_unit_and_deterministic(L):
    from fpsg_amd.metrics import swd_directions
    d = swd_directions(L, "cpu")
    assert d.shape == (L, 3) and d.dtype == torch.float32 and d.device.type == "cpu"
    assert torch.equal(d, swd_directions(L))
    assert float((d.double().norm(dim=1) - 1).abs().max()) <= 2e-7
    assert np.abs(d.double().numpy() - ref.lattice(L)).max() <= 1e-7


def test_lattice_second_moment_is_isotropic_at_64():
    from fpsg_amd.metrics import swd_directions
    d = swd_directions(64).double().numpy()
    moment = 3.0 / 64 * d.T @ d
    assert np.abs(moment - np.eye(3)).max() <= 3e-3
    for bad in (0, -1, 1025, 2.0, "64", None, True):
        with pytest.raises(ValueError, match=r"\bL\b"):
            swd_directions(bad)


# ---- 3. the library --------------------------------------------------------------------------------------------------------

def test_library_exports_and_binding(lib):
    from fpsg_amd import _hip, metrics
    for name in ("fpsg_swd", "fpsg_swd_workspace_bytes"):
        assert name in _hip.SIGNATURES and getattr(lib, name).argtypes == _hip.SIGNATURES[name]
    assert lib.fpsg_swd_workspace_bytes.restype is ctypes.c_size_t and lib.fpsg_swd.restype is ctypes.c_int
    assert len(_hip.SIGNATURES["fpsg_swd"]) == 14
    header = open(os.path.join(ROOT, "include", "fpsg_hip.h")).read()
    assert f"#define FPSG_SWD_MAX_N {metrics.SWD_MAX_N}\n" in header
    assert f"#define FPSG_SWD_MAX_L {metrics.SWD_MAX_L}\n" in header
    assert metrics.SWD_MAX_N >= 2048 and metrics.SWD_MAX_L >= 1024


def test_entry_checks_its_arguments_on_the_host(lib):
    """Every refusal answers before any HIP call (there is no GPU here)."""
    P = 0x10000                                                      # never dereferenced

    def call(B=2, N=64, L=8, xyz1=P, xyz2=P, dirs=P, value=P, g1=None, g2=None, m1=None, m2=None, ws=P, ws_bytes=1 << 40):
        return lib.fpsg_swd(xyz1, xyz2, dirs, B, N, L, value, g1, g2, m1, m2, ws, ws_bytes, None)

    def refused(code, word, **kw):
        assert call(**kw) == code, kw
        msg = lib.fpsg_last_error()
        assert msg and b"fpsg_swd" in msg and word in msg, (kw, msg)

    for name in ("B", "N", "L"):
        for bad in (0, -1):
            refused(-2, name.encode(), **{name: bad})
    refused(-4, b"2048", N=2049)
    refused(-4, b"2048", N=1 << 30)
    refused(-4, b"1024", L=1025)
    refused(-4, b"65535", B=65536)
    for name in ("xyz1", "xyz2", "dirs", "value", "ws"):
        refused(-1, b"null pointer", **{name: None})
        refused(-3, b"aligned", **{name: P + 2})
    for name in ("g1", "g2", "m1", "m2"):
        refused(-3, b"aligned", **{name: P + 1})
    need = lib.fpsg_swd_workspace_bytes(2, 64, 8)
    refused(-2, b"workspace", ws_bytes=need - 1)
    refused(-2, b"workspace", ws_bytes=0)
    # shape and limit answer in front of the pointers
    refused(-2, b"N", N=0, xyz1=None)
    refused(-4, b"2048", N=4096, xyz1=None)


def test_workspace_size(lib):
    ws = lib.fpsg_swd_workspace_bytes
    for bad in ((0, 64, 8), (-1, 64, 8), (2, 0, 8), (2, 64, 0), (2, 2049, 8), (2, 64, 1025), (65536, 64, 8), (2, -5, 8)):
        assert ws(*bad) == 0, bad
    assert ws(1, 1, 1) == (1 + 6) * 4 and ws(1, 2048, 1024) > 0
    # G = min(ceil(L / 8), 16) groups per pair, each one partial value and two [N,3] partial gradients
    for L, G in ((1, 1), (8, 1), (9, 2), (64, 8), (128, 16), (129, 16), (1024, 16)):
        assert ws(37, 2048, L) == 37 * G * (1 + 6 * 2048) * 4, L
    assert ws(6, 100, 64) == 2 * ws(3, 100, 64)


# ---- 4. options, flags, model --------------------------------------------------------------------------------------------

def test_check_swd_options():
    from fpsg_amd.metrics import SWD_MAX_L, check_swd_options
    assert check_swd_options(64, "random") == (64, "random")
    n, d = check_swd_options(np.int64(1), "fixed")
    assert (n, d) == (1, "fixed") and type(n) is int
    assert check_swd_options(SWD_MAX_L, "fixed") == (SWD_MAX_L, "fixed")
    for bad in (0, -1, SWD_MAX_L + 1, 2.0, "64", None, True):
        with pytest.raises(ValueError, match="n_proj"):
            check_swd_options(bad, "fixed")
    for bad in ("Fixed", "lattice", "", None, 1, True):
        with pytest.raises(ValueError, match="directions"):
            check_swd_options(64, bad)


@pytest.mark.parametrize("evaluation", [False, True])
def test_flags_parse_and_change_nothing_else(evaluation):
    from fpsg_amd import cli
    p = cli.few_shot_parser(evaluation=evaluation)
    base = vars(p.parse_args([]))
    assert base["pc_dist"] == "cd" and base["swd_n_proj"] == 64 and base["swd_directions"] == "random"
    assert type(base["swd_n_proj"]) is int
    on = vars(p.parse_args(["--pc_dist", "swd", "--swd_n_proj", "128", "--swd_directions", "fixed"]))
    assert (on["pc_dist"], on["swd_n_proj"], on["swd_directions"]) == ("swd", 128, "fixed")
    skip = FLAGS + ("pc_dist",)
    assert {k: v for k, v in on.items() if k not in skip} == {k: v for k, v in base.items() if k not in skip}
    with pytest.raises(SystemExit):
        p.parse_args(["--pc_dist", "sliced"])
    with pytest.raises(SystemExit):
        p.parse_args(["--swd_n_proj", "many"])


@pytest.mark.parametrize("flag,bad", [("swd_n_proj", 0), ("swd_n_proj", -4), ("swd_n_proj", 1025), ("swd_n_proj", 2.5),
                                      ("swd_directions", "lattice"), ("swd_directions", "")])
def test_validate_refuses_bad_values_and_names_the_flag(flag, bad):
    from fpsg_amd import cli
    p = cli.few_shot_parser()
    cli.validate(p.parse_args(["--synthetic", "--pc_dist", "swd", "--swd_n_proj", "1024", "--swd_directions", "fixed"]))
    cli.validate(p.parse_args(["--synthetic"]))
    opt = p.parse_args(["--synthetic", "--pc_dist", "swd"])
    setattr(opt, flag, bad)
    with pytest.raises(SystemExit) as e:
        cli.validate(opt)
    assert f"--{flag}" in str(e.value)


def test_other_distances_ignore_the_flags():
    from fpsg_amd.engine import build_model, default_options
    for dist in ("cd", "dcd", "sinkhorn"):
        model = build_model(default_options(device="cpu", pc_dist=dist, swd_n_proj=7, swd_directions="fixed"))
        assert not hasattr(model, "swd_n_proj") and not hasattr(model, "_swd_lattice")
        assert model._batched_pairs == (dist != "cd")


def test_model_and_build_model_carry_the_options_on_cpu():
    from fpsg_amd.engine import build_model, default_options
    from fpsg_amd.few_shot import ImgPCProtoNet
    opt = default_options(device="cpu")
    assert (opt.pc_dist, opt.swd_n_proj, opt.swd_directions) == ("cd", 64, "random")
    model = build_model(default_options(device="cpu", pc_dist="swd"))
    assert (model.swd_n_proj, model.swd_directions) == (64, "random") and model._batched_pairs
    model = build_model(default_options(device="cpu", pc_dist="swd", swd_n_proj=128, swd_directions="fixed"))
    assert (model.swd_n_proj, model.swd_directions) == (128, "fixed")
    assert model.pc_metric == model._swd_metric
    direct = ImgPCProtoNet(model.img_encoder, model.pc_encoder, model.pc_decoder, metric="swd", swd_n_proj=3,
                           swd_directions="fixed")
    assert (direct.swd_n_proj, direct.swd_directions) == (3, "fixed")
    # an options namespace from before the flags existed builds the defaults
    old = default_options(device="cpu", pc_dist="swd")
    for f in FLAGS:
        delattr(old, f)
    assert build_model(old).swd_n_proj == 64
    for kw, word in (({"swd_n_proj": 0}, "n_proj"), ({"swd_n_proj": 1025}, "n_proj"), ({"swd_n_proj": 2.0}, "n_proj"),
                     ({"swd_directions": "lattice"}, "directions")):
        with pytest.raises(ValueError, match=word):
            ImgPCProtoNet(model.img_encoder, model.pc_encoder, model.pc_decoder, metric="swd", **kw)


# ---- 5. no CPU path ----------------------------------------------------------------------------------------------------------

def test_wrappers_refuse_what_the_kernel_does_not_serve():
    from fpsg_amd.metrics import swd, swd_directions, swd_loss
    d = swd_directions(4)
    ok = torch.rand(2, 16, 3)
    for p1, p2, dirs, word in ((ok, torch.rand(2, 17, 3), d, "same number"), (torch.rand(2, 16, 2), ok, d, "B,N,3"),
                               (ok, torch.rand(3, 16, 3), d, "batch"), (torch.rand(1, 2049, 3), torch.rand(1, 2049, 3), d, "2048"),
                               (ok.double(), ok.double(), d, "float32"), (ok, ok, d, "GPU"),
                               (ok, ok, torch.rand(4, 2), "L,3"), (ok, ok, torch.rand(1025, 3), "L,3"),
                               (torch.rand(0, 16, 3), torch.rand(0, 16, 3), d, "empty")):
        with pytest.raises(ValueError, match=word):
            swd_loss(p1, p2, dirs)
        with pytest.raises(ValueError, match=word):
            swd(p1, p2, directions=dirs)
    with pytest.raises(ValueError, match="n_proj"):
        swd(ok, ok, n_proj=0)
