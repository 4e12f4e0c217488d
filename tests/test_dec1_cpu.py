"""K9's float64 reference (tests/_dec1_ref.py) and its comparison are themselves checked here, without a GPU: the
reference against torch float64 autograd on the literal ``cat(x.repeat, pts)`` formulation, the comparison against
"kernel outputs" with one deliberate defect each, the kink-band cap of every GPU case and seed, and the LDS rule of
the entry points' argument check."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _dec1_ref as R
from conftest import ROOT


# ------------------------------------------------------------------------------------- the reference against autograd
@pytest.mark.parametrize("name", ["g2d70b7p32-train", "g2d70b7p32-eval", "g1d33b3p128-train", "g1d33b3p128-eval"])
def test_reference_equals_float64_autograd_of_the_literal_formulation(name):
    """conv1d of cat(x.repeat, pts) with the full [D, L+3] weight, F.batch_norm, relu, in torch float64 with autograd:
    every output and gradient of the NumPy statement agrees to 1e-12 of the quantity's maximum."""
    c = R.case(name, 0)
    G, D, B, P, L = c.G, c.D, c.B, c.P, c.L
    rng = np.random.default_rng(5)
    wfull = rng.standard_normal((G, D, L + 3)) / np.sqrt(L + 3)
    wfull[:, :, L:] = c.w[:, :, L:L + 3]
    bias, x = rng.standard_normal((G, D)), rng.standard_normal((B, L))
    pts, gamma, beta = c.pts.astype(np.float64), c.gamma.astype(np.float64), c.beta.astype(np.float64)
    rmean, rvar, dout = c.rmean.astype(np.float64), c.rvar.astype(np.float64), c.dout.astype(np.float64)

    hlat = np.einsum("gdl,bl->gdb", wfull[:, :, :L], x) + bias[:, :, None]
    fw = R.forward(hlat, wfull, L, pts, gamma, beta, B, P, R.EPS, c.training, rmean, rvar)
    bw = R.backward(fw, dout, fw["z"] > 0)
    mine = dict(out=fw["out"].reshape(G, D, B * P), dw=np.concatenate([np.einsum("gdb,bl->gdl", bw["dhlat"], x), bw["dw3"]], 2),
                db=bw["dhlat"].sum(2), dx=np.einsum("gdb,gdl->bl", bw["dhlat"], wfull[:, :, :L]), dpts=bw["dpts"],
                dgamma=bw["dgamma"], dbeta=bw["dbeta"])
    if c.training:
        mine["batch_mean"], mine["batch_var"] = fw["batch_mean"], fw["batch_var_unbiased"]

    t = lambda a: torch.tensor(a, dtype=torch.float64).requires_grad_()
    tw, tb, tx, tp, tg, tbe = t(wfull), t(bias), t(x), t(pts), t(gamma.reshape(G, D)), t(beta.reshape(G, D))
    outs, stats = [], []
    for g in range(G):
        xr = tx.unsqueeze(2).repeat(1, 1, P)                                           # [B, L, P]
        pg = tp[g].view(3, B, P).permute(1, 0, 2)                                      # [B, 3, P]
        hpre = F.conv1d(torch.cat((xr, pg), dim=1), tw[g].unsqueeze(2), tb[g])         # [B, D, P]
        rm, rv = torch.tensor(rmean.reshape(G, D)[g]).clone(), torch.tensor(rvar.reshape(G, D)[g]).clone()
        if c.training:
            rm, rv = torch.zeros(D, dtype=torch.float64), torch.zeros(D, dtype=torch.float64)
        y = F.batch_norm(hpre, rm, rv, tg[g], tbe[g], c.training, 1.0, R.EPS)
        stats.append((rm, rv))                                                        # momentum 1: the batch's statistics
        outs.append(torch.relu(y).permute(1, 0, 2).reshape(D, B * P))
    out = torch.stack(outs)
    out.backward(torch.tensor(dout))
    theirs = dict(out=out, dw=tw.grad, db=tb.grad, dx=tx.grad, dpts=tp.grad, dgamma=tg.grad, dbeta=tbe.grad)
    if c.training:
        theirs["batch_mean"], theirs["batch_var"] = torch.stack([s[0] for s in stats]), torch.stack([s[1] for s in stats])
    for k, v in theirs.items():
        v = v.detach().numpy()
        scale = np.abs(v).max()
        if k == "db" and c.training:        # cancelled by the batch statistics: round-off on both sides, on dhlat's scale
            scale = np.abs(bw["dhlat"]).max()
        err = np.abs(mine[k].reshape(v.shape) - v).max() / scale
        assert err <= 1e-12, (name, k, err)


# ----------------------------------------------------------------------------------------------- the checker has teeth
def _setup(name, seed=0):
    c = R.case(name, seed)
    fw = c.reference()
    return c, fw, R.yardstick(c)


@pytest.mark.parametrize("name", [c.name for c in R.CASES])
def test_comparison_accepts_the_rounded_reference(name):
    c, fw, yard = _setup(name)
    R.compare(c, fw, R.rounded_reference(c, fw), yard, R.FACTOR, show=lambda s: None)


def _rejected(c, fw, got, yard):
    with pytest.raises(AssertionError):
        R.compare(c, fw, got, yard, R.FACTOR, show=lambda s: None)


def test_comparison_rejects_dpts_without_the_last_channel_tile():
    c, fw, yard = _setup("g1d33b3p128-train")                       # D = 33: the last tile is channel 32 alone
    bw = R.backward(fw, c.dout, fw["z"] > 0)
    got = R.rounded_reference(c, fw, bw)
    got["dpts"] = np.einsum("gdc,gdbq->gcbq", fw["w3"][:, :32], bw["dh"][:, :32]).reshape(c.G, 3, -1).astype(np.float32)
    _rejected(c, fw, got, yard)


def test_comparison_rejects_dhlat_of_lane_groups_shifted_by_one_cloud():
    c, fw, yard = _setup("g2d70b7p32-train")
    got = R.rounded_reference(c, fw)
    got["dhlat"] = np.roll(got["dhlat"], 1, axis=2)
    _rejected(c, fw, got, yard)


def test_comparison_rejects_the_backward_without_its_hhat_term():
    c, fw, yard = _setup("g2d70b7p32-train")
    mask = fw["z"] > 0
    bw = R.backward(fw, c.dout, mask)
    dz = c.dout.astype(np.float64).reshape(mask.shape) * mask
    dh = fw["scale"][:, :, None, None] * (dz - dz.mean(axis=(2, 3), keepdims=True))       # - hhat mean(dz hhat): dropped
    bw.update(dh=dh, dhlat=dh.sum(3), dw3=np.einsum("gdbq,gcbq->gdc", dh, fw["p"]),
              dpts=np.einsum("gdc,gdbq->gcbq", fw["w3"], dh).reshape(c.G, 3, -1))
    _rejected(c, fw, R.rounded_reference(c, fw, bw), yard)


def test_comparison_rejects_the_cancelling_fp32_variance_on_one_offset_cloud():
    """Variance as fp32 E[h^2] - E[h]^2 on the raw h with |hlat| = 60 sigma and ONE cloud: what the kernel did before its
    sums ran over h - K."""
    c, fw, yard = _setup("g2d70b1p32-offset1")
    f = np.float32
    h = fw["h"].astype(f).reshape(c.G, c.D, -1)
    n = f(h.shape[2])
    s, ss = h.sum(axis=2, dtype=f), (h * h).sum(axis=2, dtype=f)
    mean = s / n
    var = np.maximum(ss / n - mean * mean, f(0.0))
    rstd = (1.0 / np.sqrt(var.astype(np.float64) + R.EPS))
    bad = dict(fw)
    bad["rstd"], bad["scale"] = rstd, c.gamma.reshape(c.G, c.D) * rstd
    bad["shift"] = c.beta.reshape(c.G, c.D) - fw["mean"] * bad["scale"]
    bad["z"] = fw["h"] * bad["scale"][:, :, None, None] + bad["shift"][:, :, None, None]
    bad["out"] = np.maximum(bad["z"], 0.0)
    bad["batch_var_unbiased"] = var.astype(np.float64) * (h.shape[2] / (h.shape[2] - 1.0))
    got = R.rounded_reference(c, bad, R.backward(fw, c.dout, fw["z"] > 0))
    _rejected(c, fw, got, yard)
    # and by the variance alone
    got = R.rounded_reference(c, fw)
    got["bvar"] = bad["batch_var_unbiased"].reshape(-1).astype(f)
    _rejected(c, fw, got, yard)


def test_comparison_rejects_the_biased_variance_as_batch_var():
    c, fw, yard = _setup("g2d70b7p32-train")
    got = R.rounded_reference(c, fw)
    BP = c.B * c.P
    got["bvar"] = (fw["batch_var_unbiased"] * (BP - 1.0) / BP).reshape(-1).astype(np.float32)
    _rejected(c, fw, got, yard)


def test_comparison_rejects_a_mask_of_z_greater_or_equal_zero_at_the_exact_kink():
    c, fw, yard = _setup("g2d70b7p32-kink_eval")
    assert (fw["z"][c.exact_kink] == 0).all()
    got = R.rounded_reference(c, fw, R.backward(fw, c.dout, fw["z"] >= 0))       # out itself is 0 either way
    _rejected(c, fw, got, yard)


def test_comparison_rejects_accumulate_that_overwrites():
    c, fw, yard = _setup("g2d70b7p32-train-accumulate")
    got = R.rounded_reference(c, fw)
    plain = R.backward(fw, c.dout, fw["z"] > 0)
    for k, v in (("dw3", plain["dw3"]), ("dgamma", plain["dgamma"].reshape(-1)), ("dbeta", plain["dbeta"].reshape(-1))):
        bad = dict(got)
        bad[k] = v.astype(np.float32)
        _rejected(c, fw, bad, yard)


# ------------------------------------------------------------------------------------------------- the kink-band cap
@pytest.mark.parametrize("name", [c.name for c in R.CASES])
def test_kink_band_cap_holds_for_every_case_and_seed(name):
    """A condition on the inputs, checked on the float64 side alone: at most 1e-3 of a case's elements lie where fp32 may
    round z across zero (the exactly-zero elements of the exact-kink case are that case's subject and do not count)."""
    for seed in R.SEEDS:
        c = R.case(name, seed)
        fw = c.reference()
        bd = R.band(fw) & ~c.exact_kink[:, :, None, None]
        assert bd.mean() <= R.BAND_CAP, (name, seed, int(bd.sum()), bd.size)
        if c.kind == "kink_eval":
            assert (fw["z"][c.exact_kink] == 0).all() and R.band(fw)[c.exact_kink].all()
        if c.kind == "zerovar":
            assert np.allclose(fw["rstd"][c.cancelled], 1.0 / np.sqrt(R.EPS), rtol=1e-12)
        if c.kind == "dead":
            assert (fw["out"][c.dead] == 0).all()


# --------------------------------------------------------------------------------------------------------- the LDS rule
@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    if not os.path.exists(os.path.join(ROOT, "fpsg_amd", "libfpsg_hip.so")):
        g.build()
    from fpsg_amd import _hip
    return _hip.load()


def _fwd(lib, B, P):
    return lib.fpsg_dec1_fwd_ld(None, B, None, 3, 0, None, B * P, None, None, None, None, 1, 32, B, P, 1, 1e-5, None, B * P,
                                None, None, None, None)


def _bwd(lib, B, P):
    return lib.fpsg_dec1_bwd_ld(None, B * P, None, B, None, 3, 0, None, B * P, None, 1, 32, B, P, 1, 0, None, None, None,
                                None, None, None)


def test_lds_rule_answers_on_the_host_at_its_thresholds(lib):
    """A workgroup's LDS is 4 (3 B P + 32 B [+ 6144 backward]) bytes; beyond the 163840 of a CU the entry points answer
    FPSG_E_LIMIT (-4) naming B, P and the bytes, before any pointer check (null pointers otherwise: -1), and the Python
    gate takes the library chain.  The thresholds are the formula's: P = 16 from B = 436 in the backward, P = 4 from
    B = 931 in the forward; (P 128, B 64), the largest production call, is 131072 bytes and passes.  (P 16, B 342) and
    (P 4, B 274), once put forward as those thresholds, need 134016 bytes in the backward and 48224 in the forward: they
    fit, launch and stay with K9 -- refusing them would send decodes that run today to the library chain.)"""
    from fpsg_amd.point_cloud_net import _layer1_sizes_ok
    assert R.lds_bytes(435, 16, True) <= R.LDS_LIMIT < R.lds_bytes(436, 16, True) == 164096
    assert R.lds_bytes(930, 4, False) <= R.LDS_LIMIT < R.lds_bytes(931, 4, False) == 163856
    assert R.lds_bytes(64, 128, True) == 128 * 1024
    assert _bwd(lib, 436, 16) == -4
    msg = lib.fpsg_last_error()
    assert b"B = 436" in msg and b"P = 16" in msg and b"164096" in msg, msg
    assert _fwd(lib, 436, 16) == -1 and _bwd(lib, 435, 16) == -1              # the forward's 139520 bytes fit
    assert _fwd(lib, 931, 4) == -4
    msg = lib.fpsg_last_error()
    assert b"B = 931" in msg and b"P = 4" in msg and b"163856" in msg, msg
    assert _bwd(lib, 931, 4) == -4 and _fwd(lib, 930, 4) == -1
    assert _fwd(lib, 64, 128) == -1 and _bwd(lib, 64, 128) == -1 and b"null pointer" in lib.fpsg_last_error()
    assert R.lds_bytes(342, 16, True) == 134016 and R.lds_bytes(274, 4, False) == 48224
    assert _bwd(lib, 342, 16) == -1 and _fwd(lib, 274, 4) == -1 and _bwd(lib, 274, 4) == -1
    for B, P, fwd_fits, bwd_fits in ((436, 16, 1, 0), (435, 16, 1, 1), (931, 4, 0, 0), (930, 4, 1, 0), (64, 128, 1, 1),
                                     (65, 128, 0, 0), (32, 128, 1, 1), (1, 4, 1, 1), (4, 12, 0, 0), (1, 512, 0, 0),
                                     (342, 16, 1, 1), (274, 4, 1, 1), (512, 16, 1, 0), (2048, 4, 0, 0)):      # (512, 16) forward: 163840 exactly
        assert (lib.fpsg_dec1_fits(B, P, 0), lib.fpsg_dec1_fits(B, P, 1)) == (fwd_fits, bwd_fits), (B, P)
        assert _layer1_sizes_ok(B, P) == bool(bwd_fits), (B, P)               # the gate goes by the backward's size
        assert bool(fwd_fits) == (R.lds_bytes(B, P, False) <= R.LDS_LIMIT and B * P <= 8192 and P in (4, 8, 16, 32, 64, 128, 256))
