"""The EdgeConv references of tests/_edgeconv_ref.py checked on their own, without a GPU: against the literal reference
chain (reference dgcnn/model.py:23-42,63-65) in float64, against each other, and the preconditions that
tests/test_edgeconv_gpu.py relies on for the inputs it fixes."""
import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import _edgeconv_ref as R


def _rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / np.abs(b).max())


def _dyadic_inputs(B, N, k, C, Co, seed):
    """x and W on the grid 2^-9 in [-1, 1]: every product is a multiple of 2^-18, |P| <= 8, |Q| <= 16 and |P + Q| <= 24
    take at most 23 bits, so the float64 GEMM, its rounding to fp32 and the fp32 addition P + Q are all exact and the
    literal chain sees the very numbers that layer64 works on."""
    rng = np.random.default_rng(seed)
    x = rng.integers(-512, 513, size=(B, C, N)) / 512.0
    W = rng.integers(-512, 513, size=(Co, 2 * C)) / 512.0
    idx = np.argsort(rng.random((B, N, N)), axis=2)[:, :, :k]              # no repeats: max(-1) then meets no tie
    wc = np.concatenate((W[:, :C], W[:, C:] - W[:, :C]), axis=0)              # [2Co, C]: rows of P, then of Q
    PQ64 = x.transpose(0, 2, 1) @ wc.T
    PQ = PQ64.astype(np.float32)
    assert np.array_equal(PQ.astype(np.float64), PQ64)
    exact = PQ64[..., :Co][np.arange(B)[:, None, None], idx] + PQ64[:, :, None, Co:]
    assert np.array_equal(R.edge_values(PQ, idx).astype(np.float64), exact)
    return x, W, wc, idx, PQ


@pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
def test_references_match_the_literal_chain(training):
    B, N, k, C, Co = 2, 24, 5, 8, 64
    x, W, wc, idx, PQ = _dyadic_inputs(B, N, k, C, Co, seed=11)
    rng = np.random.default_rng(12)
    gamma, beta = 0.7 * rng.standard_normal(Co), 0.3 * rng.standard_normal(Co)
    rm0, rv0 = 0.2 * rng.standard_normal(Co), 0.5 + rng.random(Co)
    w_out = rng.standard_normal((B, N, Co))
    assert (gamma > 0).any() and (gamma < 0).any()

    # the literal chain: torch-indexed cat(x_j - x_i, x_i), Conv2d, BatchNorm2d, LeakyReLU(0.2), max over k
    xt = torch.from_numpy(x).requires_grad_()
    Wt = torch.from_numpy(W).reshape(Co, 2 * C, 1, 1).requires_grad_()
    bn = nn.BatchNorm2d(Co).double()
    with torch.no_grad():
        bn.weight.copy_(torch.from_numpy(gamma)); bn.bias.copy_(torch.from_numpy(beta))
        bn.running_mean.copy_(torch.from_numpy(rm0)); bn.running_var.copy_(torch.from_numpy(rv0))
    bn.train(training)
    it = torch.from_numpy(idx)
    pm = xt.transpose(1, 2)                                                   # [B,N,C]
    nb = pm[torch.arange(B)[:, None, None], it]                               # [B,N,k,C]
    ctr = pm[:, :, None, :].expand_as(nb)
    feat = torch.cat((nb - ctr, ctr), dim=3).permute(0, 3, 1, 2)              # [B,2C,N,k]
    yc = F.conv2d(feat, Wt)
    yc.retain_grad()
    out = F.leaky_relu(bn(yc), 0.2).max(dim=-1)[0]                            # [B,Co,N]
    (out.transpose(1, 2) * torch.from_numpy(w_out)).sum().backward()
    dY = yc.grad.permute(0, 2, 3, 1)                                          # [B,N,k,Co]: the chain's per-edge gradient
    dPQ_chain = torch.zeros(B, N, 2 * Co, dtype=torch.float64)
    dPQ_chain[:, :, Co:] = dY.sum(dim=2)
    for b in range(B):
        dPQ_chain[b, :, :Co].index_add_(0, it[b].reshape(-1), dY[b].reshape(N * k, Co))

    ref = R.layer64(PQ, idx, gamma, beta, rm0, rv0, training, 0.1, 1e-5, 0.2, w_out)
    assert ref.inexact_ties == 0 and ref.gap_min > 0
    tol = 1e-9
    assert _rel(ref.out, out.detach().transpose(1, 2).numpy()) <= tol
    assert _rel(ref.running_mean, bn.running_mean.numpy()) <= tol
    assert _rel(ref.running_var, bn.running_var.numpy()) <= tol
    assert _rel(ref.dgamma, bn.weight.grad.numpy()) <= tol
    assert _rel(ref.dbeta, bn.bias.grad.numpy()) <= tol
    assert _rel(ref.dPQ, dPQ_chain.numpy()) <= tol
    # ... and through the GEMM in front, where the chain's autograd does the scatter itself
    dx = ref.dPQ @ wc                                                          # [B,N,C]
    assert _rel(dx.transpose(0, 2, 1), xt.grad.numpy()) <= tol
    dwc = np.einsum("bnc,bnd->cd", ref.dPQ, x.transpose(0, 2, 1))             # [2Co,C]
    dW = np.concatenate((dwc[:Co] - dwc[Co:], dwc[Co:]), axis=1)
    assert _rel(dW, Wt.grad.reshape(Co, 2 * C).numpy()) <= tol

    # backward_per_edge on the chain's own dz: dzs = w_out * LeakyReLU'(z) * scale, coef from the statistics
    dzs, coef = _bwd_inputs(ref, w_out, 0.2, training)
    dPQ_edge, T = R.backward_per_edge(dzs, ref.jsel, PQ, idx, coef)
    assert _rel(dPQ_edge, dPQ_chain.numpy()) <= tol
    assert (T >= np.abs(dPQ_edge) * (1 - 1e-12)).all()


def _bwd_inputs(ref, w_out, slope, training):
    Co = ref.scale.shape[0]
    dzs = np.asarray(w_out, dtype=np.float64) * np.where(ref.z > 0, 1.0, slope) * ref.scale
    coef = np.zeros((3, Co))
    if training:
        coef[0] = ref.scale * ref.dbeta / ref.count
        coef[1] = ref.scale * ref.rstd * ref.dgamma / ref.count
        coef[2] = ref.mean
    return dzs, coef


@pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("key", [(2, 48, 20, 64, 0.0), (9, 13, 5, 64, 0.0), (2, 24, 20, 256, 3.0)], ids=str)
def test_per_edge_backward_is_the_layer_gradient(key, training):
    """The identity behind the kernels' coefficients: with A = scale dbeta / count, Bc = scale rstd dgamma / count and
    mu = mean, the per-edge backward is autograd's dPQ of the whole layer."""
    case = R.layer_case(*key)
    ref = R.layer_ref(case, training)
    dzs, coef = _bwd_inputs(ref, case.w_out, R.SLOPE, training)
    dPQ, _ = R.backward_per_edge(dzs, ref.jsel, case.PQ, case.idx, coef)
    assert _rel(dPQ, ref.dPQ) <= 1e-12


def test_forward_exact_against_a_plain_loop():
    """Slot by slot in Python: strict comparison from slot 0 on, so the lowest slot keeps a tie; ``-0.0`` takes the max."""
    rng = np.random.default_rng(5)
    B, N, k, Co = 2, 6, 4, 64
    PQ = rng.standard_normal((B, N, 2 * Co)).astype(np.float32)
    PQ[:, :, 1:Co:4] = np.round(PQ[:, :, 1:Co:4] * 2) / 2                     # exact ties between different neighbours
    idx = rng.integers(0, N, size=(B, N, k))
    idx[0, :, 3] = idx[0, :, 1]
    sgn = rng.standard_normal(Co).astype(np.float32)
    sgn[5] = np.float32(-0.0)
    fwd = R.forward_exact(PQ, idx, sgn)
    ties = 0
    for b in range(B):
        for n in range(N):
            for c in range(Co):
                ys = [np.float32(PQ[b, idx[b, n, j], c] + PQ[b, n, Co + c]) for j in range(k)]
                best, bj = ys[0], 0
                for j in range(1, k):
                    if (ys[j] < best) if sgn[c] < 0 else (ys[j] > best):
                        best, bj = ys[j], j
                ties += sum(1 for v in ys if v == best) > 1
                assert fwd.jsel[b, n, c] == bj and fwd.ysel[b, n, c] == best
                assert abs(fwd.s1[b, n, c] - sum(float(v) for v in ys)) <= 1e-12
    assert ties > 20 and fwd.jsel.max() > 0
    assert np.allclose(fwd.sum_y, fwd.s1.sum(axis=(0, 1)), rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("key", R.LAYER_CASES, ids=str)
def test_fixed_layer_inputs_meet_the_preconditions(key):
    """What tests/test_edgeconv_gpu.py assumes of its end-to-end inputs, on the float64 reference alone: no selected
    activation within 1e-4 of the LeakyReLU kink (ten times the relative error that fp32 partial sums of up to 640 terms
    can put on scale and shift), ties only where the exact sums tie, gammas of both signs and none 0."""
    case = R.layer_case(*key)
    assert (case.gamma != 0).all() and (case.gamma > 0).any() and (case.gamma < 0).any()
    if key[4] > 0:
        assert 0.9 * key[4] <= case.ratio.max() <= key[4]
    for training in (True, False):
        ref = R.layer_ref(case, training)
        assert ref.kink_min >= 1e-4, (training, ref.kink_min)
        assert ref.gap_min > 0 or ref.inexact_ties == 0


@pytest.mark.parametrize("key", R.OFFSET12_CASES, ids=str)
def test_offset_inputs_reach_twelve_standard_deviations(key):
    case = R.layer_case(*key)
    assert 11.0 <= case.ratio.max() <= 12.0
    assert (case.gamma != 0).all()
