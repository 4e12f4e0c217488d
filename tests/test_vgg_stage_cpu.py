"""The kink-free VGG stages of ``tests/_vgg_stage_ref.py`` (the inputs of ``tests/test_vgg_stage_gpu.py``): the conditions
the construction promises are asserted here, on the CPU, before any kernel is compared with anything -- they are properties
of the inputs, not measurements -- and the F(4x4, 3x3) yardstick is held to float64 itself."""
import pytest
import torch
import torch.nn.functional as F

import _vgg_stage_ref as R

CASES = [("stem", "train"), ("stem", "eval"), ("stemw", "train"), ("s2", "train"), ("s2", "eval"), ("s3", "train"),
         ("s3", "eval"), ("s5", "train"), ("s5", "eval")]          # every (stage, mode) the GPU test uses


def _channel_stats(tr, bn, y):
    """Per channel of the BatchNorm input ``y``: mean, std, and |d z / d y| = |gamma| / sqrt(var + eps) of the chain."""
    mean, var = y.mean((0, 2, 3)), y.var((0, 2, 3), unbiased=False)
    used = var if tr.mode == "train" else tr.running[bn + ".running_var"].double()
    slope = tr.params[bn + ".weight"].double().abs() / (used + R.EPS).sqrt()
    return mean, var.sqrt(), slope


@pytest.mark.parametrize("name,mode", CASES)
def test_conditions_of_the_construction(name, mode):
    tr = R.truth(name, mode)
    i64 = tr.inner64
    for bn, y, z, step in (("1", i64["y1"], i64["z1"], 1.0), ("4", i64["y2"], i64["z2"], R.Q)):
        mean, std, slope = _channel_stats(tr, bn, y)
        # 1. margins: the distance of every pre-activation from its kink, in units of y, against 16 x the deviation the
        #    north-star tolerance would allow that tensor
        margin = float((z.abs() / slope.view(1, -1, 1, 1)).min())
        ymax = float(y.abs().max())
        print(f"{name}/{mode} BN {bn}: margin {margin:.4g} (lattice step {step:.4g}), max|y| {ymax:.4g}, "
              f"max |mean|/std {float((mean.abs() / std).max()):.3g}")
        assert margin >= 0.4999 * step
        assert margin >= R.MARGIN_FACTOR * R.NORTH_STAR * ymax, (margin, ymax)
        # 2. no offset channels (their cancellation is another test's subject)
        assert float((mean.abs() / std).max()) <= R.MAX_OFFSET
    kept = float(tr.kept.double().mean())
    print(f"{name}/{mode}: {100 * kept:.1f} % of the pool windows keep their cotangent")
    assert kept >= 0.5
    assert int(torch.count_nonzero(tr.g[~tr.kept.expand_as(tr.g)])) == 0
    gap = R.window_gap(i64["a2"])
    assert float(gap[tr.kept].min()) >= R.TIE * float(i64["a2"].max())
    # 3. the library's fp32 chain takes every ReLU and every kept pool window as float64 does
    for other in (tr.inner_lib, tr.inner_wino):
        for z in ("z1", "z2"):
            assert int(((other[z] > 0) != (i64[z] > 0)).sum()) == 0
        assert int(((other["sel"] != i64["sel"]) & tr.kept).sum()) == 0


@pytest.mark.parametrize("name,mode", CASES)
def test_yardsticks_against_float64(name, mode):
    """Both fp32 yardsticks within the north-star tolerance of float64 on every compared tensor (the Winograd chain in
    plain torch ops costs about a digit over the direct form); cancelled bias gradients hold round-off only."""
    tr = R.truth(name, mode)
    assert set(tr.lib) == set(tr.wino) == set(tr.t64)
    assert ("dx" in tr.t64) == (name not in ("stem", "stemw"))
    for k in sorted(tr.t64):
        if k.endswith("num_batches_tracked"):
            assert int(tr.lib[k]) == int(tr.wino[k]) == int(tr.t64[k]) == (1 if mode == "train" else 0)
            continue
        if R.cancelled(k, mode):
            beta = float(tr.t64["d 1.bias" if k == "d 0.bias" else "d 4.bias"].abs().max())
            assert float(tr.t64[k].abs().max()) <= 1e-10 * beta
            print(f"{name}/{mode} {k}: cancelled; max|lib| {float(tr.lib[k].abs().max()):.3g}, "
                  f"max|wino| {float(tr.wino[k].abs().max()):.3g}, allowed {R.cancelled_bound(tr, k):.3g}")
            assert max(float(tr.lib[k].abs().max()), float(tr.wino[k].abs().max())) <= R.NORTH_STAR * beta
            continue
        dl, dw = R.deviation(tr.lib[k], tr.t64[k]), R.deviation(tr.wino[k], tr.t64[k])
        print(f"{name}/{mode} {k}: lib {dl:.3g}, wino {dw:.3g}, bound for a path under test {R.bound(tr, k):.3g}")
        assert dl <= R.NORTH_STAR and dw <= R.NORTH_STAR, (k, dl, dw)


@pytest.mark.parametrize("shape", [(2, 5, 7, 8, 12), (1, 3, 4, 14, 14), (2, 4, 3, 6, 10)])
def test_winograd_yardstick_is_the_convolution(shape):
    """``wino_conv3x3`` in float64 equals ``conv2d`` to float64 round-off, value and both gradients, ragged planes too."""
    N, C, K, H, W = shape
    gen = torch.Generator().manual_seed(H)
    x = torch.randn(N, C, H, W, generator=gen, dtype=torch.float64)
    w = torch.randn(K, C, 3, 3, generator=gen, dtype=torch.float64)
    g = torch.randn(N, K, H, W, generator=gen, dtype=torch.float64)
    res = []
    for conv in (lambda a, b: F.conv2d(a, b, None, 1, 1), R.wino_conv3x3):
        xi, wi = x.clone().requires_grad_(), w.clone().requires_grad_()
        y = conv(xi, wi)
        y.backward(g)
        res.append((y.detach(), xi.grad, wi.grad))
    for a, b in zip(*res):
        assert R.deviation(b, a) <= 1e-12
