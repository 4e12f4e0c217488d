"""K9 (``dec1_fwd_kernel`` / ``dec1_bwd_kernel``, fpsg_amd/csrc/decoder.hip) through the C ABI against the NumPy float64
statement of tests/_dec1_ref.py.

Every output buffer is pre-filled with NaN and every input is surrounded by NaN: rows longer than the call's range
(``ld > B P``, hlat / dhlat ``ld > B``), the range one vector into the row, the weight's other columns, a stretch behind
every buffer and a whole spare tile behind ``dpts_part``.  After the call everything the kernel does not own is still NaN
and everything it owns is finite.  ``dpts`` is the sum of ``dpts_part`` over the channel tiles, as the caller forms it.

Shapes (G, D, B, P), each the smallest that reaches its path, in training and eval mode:
  3, 1, 1, 4      one channel, one cloud, one lane; a lane = a cloud; B = 1 so K = hlat
  2, 70, 7, 32    BP/4 = 56 < 64: idle lanes in the only block; last tile of 6 channels: one wave partly live, six dead
  1, 33, 3, 128   BP/4 = 96: the second half of the backward's two-block trip is out of range, second block partial;
                  a tile with one live channel
  1, 32, 5, 256   a cloud = a whole wave; odd number of 64-lane blocks
  2, 40, 130, 4   B > 64: two trips of the K sum; BP/4 = 130
  1, 64, 9, 8     P = 8, two full tiles
  1, 96, 16, 128  BP/4 = 512: no tails anywhere (through the contiguous entry points)
  1, 35, 48, 128  LDS above 64 KiB: the hipFuncSetAttribute path, forward (78 KiB) and backward (102 KiB)
plus accumulate = 1 onto random contents on two of them, and at (2, 70, 1 | 7, 32) channels with |hlat| = 60 sigma, dead
channels, gamma = 0 and < 0, zero variance and z exactly 0, side by side with ordinary channels in one launch.

Bound: deviation from float64 <= max(FACTOR x the deviation of the same split formulation in plain torch fp32, 16 fp32
ulps of the quantity's float64 maximum); FACTOR and the measurements it comes from: profiles/k9/dec1_deviation.txt.  The
gradients are compared with the float64 backward under the kernel's own ReLU mask, which must equal the float64 mask
outside the kink band (tests/_dec1_ref.py; the band holds at most 1e-3 of a case's elements:
tests/test_dec1_cpu.py)."""
import numpy as np
import pytest
import torch

import _dec1_ref as R

pytestmark = pytest.mark.gpu

NAN = float("nan")


@pytest.fixture(scope="module")
def lib():
    from fpsg_amd import _hip
    return _hip.load()


def _nan(gpu, *shape, behind=64):
    """A NaN-filled tensor of ``shape`` and the ``behind`` NaN floats after it."""
    n = int(np.prod(shape))
    flat = torch.full((n + behind,), NAN, device=gpu)
    return flat[:n].view(*shape), flat[n:]


def _framed(gpu, a, ld, off):
    """``a [.., .., n]`` at columns off .. off+n of NaN rows of length ld."""
    buf, guard = _nan(gpu, a.shape[0], a.shape[1], ld)
    buf[:, :, off:off + a.shape[2]] = torch.as_tensor(a, device=gpu)
    return buf, guard


def _only_nan_outside(buf, off, n):
    return bool(torch.isnan(buf[:, :, :off]).all() and torch.isnan(buf[:, :, off + n:]).all()
                and torch.isfinite(buf[:, :, off:off + n]).all())


def _run(c, lib, gpu):
    from fpsg_amd import _hip
    G, D, B, P, L, K = c.G, c.D, c.B, c.P, c.L, c.ldw
    BP, GD = B * P, G * D
    T = lib.fpsg_dec1_tiles(D)
    assert T == -(-D // 32)
    ld, off, ldh, offh = (BP, 0, B, 0) if c.contiguous else (BP + 8, 4, B + 3, 1)
    t = lambda a: torch.as_tensor(a, device=gpu).contiguous()
    pts, _ = _framed(gpu, c.pts, ld, off)
    hlat, _ = _framed(gpu, c.hlat, ldh, offh)
    dout, _ = _framed(gpu, c.dout, ld, off)
    w, gamma, beta, rmean, rvar = t(c.w), t(c.gamma), t(c.beta), t(c.rmean), t(c.rvar)
    out, g_out = _nan(gpu, G, D, ld)
    chan, g_chan = _nan(gpu, 4, GD)
    bmean, g_bm = _nan(gpu, GD)
    bvar, g_bv = _nan(gpu, GD)
    dhlat, g_dh = _nan(gpu, G, D, ldh)
    dw, g_dw = _nan(gpu, G, D, K)
    part, g_part = _nan(gpu, G, T, 3, BP, behind=max(64, 3 * BP))          # the rows of a tile after the last
    dgamma, g_dg = _nan(gpu, GD)
    dbeta, g_db = _nan(gpu, GD)
    if c.accumulate:
        dw[:, :, L:L + 3] = t(c.prior["dw3"])
        dgamma.copy_(t(c.prior["dgamma"]))
        dbeta.copy_(t(c.prior["dbeta"]))
    st = _hip.stream_of(w)
    p = _hip.ptr
    tr = 1 if c.training else 0
    stat = (p(bmean), p(bvar)) if c.training else (None, None)
    run = (None, None) if c.training else (p(rmean), p(rvar))
    if c.contiguous:
        rc = lib.fpsg_dec1_fwd(p(hlat), p(w), K, L, p(pts), p(gamma), p(beta), run[0], run[1], G, D, B, P, tr, R.EPS, p(out),
                               p(chan), stat[0], stat[1], st)
    else:
        rc = lib.fpsg_dec1_fwd_ld(p(hlat) + 4 * offh, ldh, p(w), K, L, p(pts) + 4 * off, ld, p(gamma), p(beta), run[0], run[1],
                                  G, D, B, P, tr, R.EPS, p(out) + 4 * off, ld, p(chan), stat[0], stat[1], st)
    _hip.check(rc, "fpsg_dec1_fwd")
    if c.contiguous:
        assert not c.accumulate
        rc = lib.fpsg_dec1_bwd(p(dout), p(hlat), p(w), K, L, p(pts), p(chan), G, D, B, P, tr, p(dhlat), p(dw), p(part),
                               p(dgamma), p(dbeta), st)
    else:
        rc = lib.fpsg_dec1_bwd_ld(p(dout) + 4 * off, ld, p(hlat) + 4 * offh, ldh, p(w), K, L, p(pts) + 4 * off, ld, p(chan),
                                  G, D, B, P, tr, 1 if c.accumulate else 0, p(dhlat) + 4 * offh, p(dw), p(part), p(dgamma),
                                  p(dbeta), st)
    _hip.check(rc, "fpsg_dec1_bwd")
    torch.cuda.synchronize()
    # what the kernel does not own is untouched, what it owns is written
    for name, g in (("out", g_out), ("chan", g_chan), ("batch_mean", g_bm), ("batch_var", g_bv), ("dhlat", g_dh),
                    ("dw", g_dw), ("dpts_part", g_part), ("dgamma", g_dg), ("dbeta", g_db)):
        assert bool(torch.isnan(g).all()), (c, name, "written behind the buffer")
    assert _only_nan_outside(out, off, BP), (c, "out: columns outside the call's range written, or inside it not")
    assert _only_nan_outside(dhlat, offh, B), (c, "dhlat")
    assert _only_nan_outside(dw, L, 3), (c, "dw: columns outside wofs .. wofs+2")
    assert bool(torch.isfinite(part).all() and torch.isfinite(chan).all() and torch.isfinite(dgamma).all()
                and torch.isfinite(dbeta).all()), c
    if c.training:
        assert bool(torch.isfinite(bmean).all() and torch.isfinite(bvar).all()), c
    else:
        assert bool(torch.isnan(bmean).all() and torch.isnan(bvar).all()), (c, "eval mode wrote batch statistics")
    n = lambda v: v.cpu().numpy()
    got = dict(out=n(out[:, :, off:off + BP]), chan=n(chan), dhlat=n(dhlat[:, :, offh:offh + B]), dw3=n(dw[:, :, L:L + 3]),
               dpts=n(part.sum(dim=1)), dgamma=n(dgamma), dbeta=n(dbeta), part=n(part))
    if c.training:
        got["bmean"], got["bvar"] = n(bmean), n(bvar)
    return got


@pytest.mark.parametrize("seed", R.SEEDS)
@pytest.mark.parametrize("name", [c.name for c in R.CASES])
def test_k9_against_float64(gpu, lib, name, seed):
    c = R.case(name, seed)
    fw = c.reference()
    got = _run(c, lib, gpu)
    yard = R.yardstick(c)                    # plain torch fp32 on the same inputs (CPU: no library heuristics in it)
    if c.kind == "dead":                     # channels 64..69 are a whole tile: its share of dpts is exactly zero
        assert not got["part"][:, 2].any()
    if c.kind == "zerovar":
        rstd = np.float32(1.0 / np.sqrt(np.float64(np.float32(R.EPS))))          # var is exactly 0: 1 / sqrt(eps)
        assert (got["chan"][3].reshape(c.G, c.D)[c.cancelled] == rstd).all()
        assert not got["bvar"].reshape(c.G, c.D)[c.cancelled].any()
    R.compare(c, fw, got, yard, R.FACTOR)     # profiles/k9/dec1_deviation.txt


def _to(inp, gpu, *keys):
    return [torch.tensor(inp[k], device=gpu).requires_grad_() for k in keys]


@pytest.mark.parametrize("batches", [(7,), (2, 5)])
def test_k9_autograd_functions_against_the_float64_literal_formulation(gpu, batches):
    """``_DecoderLayer1`` (one decode) and ``_DecoderLayer1Pair`` (two decodes side by side, each with its own statistics):
    output, batch statistics and the gradients of the full stacked weight, the bias, the latents, the points, gamma and
    beta against conv1d of cat(x.repeat, pts) + F.batch_norm + relu in float64, once per decode.  The seed's kink band is
    empty (asserted), so the masks agree and the yardstick rule applies as it stands."""
    from fpsg_amd.point_cloud_net import _DecoderLayer1, _DecoderLayer1Pair
    inp = R.layer1_inputs(R.LAYER1_SEEDS[batches], batches)
    assert R.layer1_band(inp) == 0
    truth, yard = R.layer1_torch(inp, torch.float64, split=False), R.layer1_torch(inp, torch.float32, split=True)
    w1, b1, x, pts, gamma, beta = _to(inp, gpu, "w1", "b1", "x", "pts", "gamma", "beta")
    if len(batches) == 1:
        out, bm, bv = _DecoderLayer1.apply(w1, b1, x, pts, gamma, beta, None, None, True, R.EPS, inp["P"])
        stats = torch.stack([bm, bv]).unsqueeze(0)
    else:
        out, stats = _DecoderLayer1Pair.apply(w1, b1, x, pts, gamma, beta, R.EPS, inp["P"], batches)
    (out * torch.tensor(inp["dout"], device=gpu)).sum().backward()
    n = lambda v: v.detach().cpu().numpy().astype(np.float64)
    got = dict(out=n(out), stats=n(stats), w1=n(w1.grad), b1=n(b1.grad), x=n(x.grad), pts=n(pts.grad), gamma=n(gamma.grad),
               beta=n(beta.grad))
    R.compare_layer1("layer1-b" + "+".join(map(str, batches)), got, truth, yard, R.FACTOR)
