"""K9 (the decoder's first layer, ``fpsg_dec1_fwd[_ld]`` / ``fpsg_dec1_bwd[_ld]``) stated in NumPy float64, the cases the
kernel tests run, the fp32 yardstick and the comparison both test files use.  Nothing here calls into ``fpsg_amd``.

The operation, per patch g, channel d, cloud b and point q of the cloud (e = b P + q):

    h[g,d,b,q] = hlat[g,d,b] + sum_c w[g,d,wofs+c] pts[g,c,e]
    training:  mean, var = mean and BIASED variance of h over (b, q);   eval: the running statistics
    rstd = 1 / sqrt(var + eps),  scale = gamma rstd,  shift = beta - mean scale,  hhat = (h - mean) rstd
    z = hhat gamma + beta,  out = max(z, 0),  batch_var_unbiased = var BP / (BP - 1)

    dz = dout mask,  dbeta = sum dz,  dgamma = sum dz hhat
    dh = scale (dz - mean(dz) - hhat mean(dz hhat))  in training,  scale dz  in eval
    dhlat[g,d,b] = sum_q dh,  dW[g,d,wofs+c] = sum_e dh pts[g,c,e],  dpts[g,c,e] = sum_d w[g,d,wofs+c] dh[g,d,e]

The ReLU mask is an argument of the backward: fp32 and float64 may disagree on it where z rounds across zero (`band`),
so a kernel's gradients are compared with the float64 backward under the KERNEL's mask, and the masks themselves
must agree everywhere outside the band.
"""
from __future__ import annotations

import numpy as np

ULP = 2.0 ** -23                 # of a value in [1, 2)
FLOOR = 16 * ULP                 # "16 fp32 ulps of the quantity's scale"
# kernel <= max(FACTOR x yardstick, FLOOR).  FACTOR: the smallest of {2, 4, 8} that leaves a factor 2 over the worst
# kernel / yardstick ratio recorded on the MI355X over all cases x 3 seeds (profiles/k9/dec1_deviation.txt: the kernel is
# inside the floor everywhere but in the two one-cloud cases, 0.90-1.20 x the yardstick with |hlat| = 60 sigma and
# 1.02-1.48 x on `out` of zero-variance channels; 2 x 1.48 needs 4).  A ratio above 4 on a quantity that is above the
# floor is a finding about the kernel, not a reason to raise this.
FACTOR = 4.0
BAND_CAP = 1e-3                 # at most this share of a case's elements may lie in the kink band
SEEDS = (0, 1, 2)
EPS = 1e-5
LDS_LIMIT = 160 * 1024


# --------------------------------------------------------------------------------------------- the operation, float64
def forward(hlat, w, wofs, pts, gamma, beta, B, P, eps, training, rmean=None, rvar=None):
    hlat, w, pts = (np.asarray(a, np.float64) for a in (hlat, w, pts))
    G, D, _ = hlat.shape
    BP = B * P
    w3 = w[:, :, wofs:wofs + 3]
    p = pts.reshape(G, 3, B, P)
    h = hlat[:, :, :, None] + np.einsum("gdc,gcbq->gdbq", w3, p)
    gamma, beta = np.asarray(gamma, np.float64).reshape(G, D), np.asarray(beta, np.float64).reshape(G, D)
    if training:
        mean = h.mean(axis=(2, 3))
        var = np.square(h - mean[:, :, None, None]).mean(axis=(2, 3))
    else:
        mean, var = np.asarray(rmean, np.float64).reshape(G, D), np.asarray(rvar, np.float64).reshape(G, D)
    rstd = 1.0 / np.sqrt(var + eps)
    scale = gamma * rstd
    shift = beta - mean * scale
    hhat = (h - mean[:, :, None, None]) * rstd[:, :, None, None]
    z = hhat * gamma[:, :, None, None] + beta[:, :, None, None]
    fw = dict(G=G, D=D, B=B, P=P, training=bool(training), h=h, hhat=hhat, z=z, out=np.maximum(z, 0.0), scale=scale,
              shift=shift, mean=mean, rstd=rstd, w3=w3, p=p)
    if training:
        fw["batch_mean"] = mean
        fw["batch_var_unbiased"] = var * (BP / (BP - 1.0)) if BP > 1 else var
    return fw


def backward(fw, dout, mask):
    G, D, B, P = fw["G"], fw["D"], fw["B"], fw["P"]
    hhat, scale = fw["hhat"], fw["scale"][:, :, None, None]
    dz = np.asarray(dout, np.float64).reshape(G, D, B, P) * mask.reshape(G, D, B, P)
    dbeta = dz.sum(axis=(2, 3))
    dgamma = (dz * hhat).sum(axis=(2, 3))
    if fw["training"]:
        dh = scale * (dz - dz.mean(axis=(2, 3), keepdims=True) - hhat * (dz * hhat).mean(axis=(2, 3), keepdims=True))
    else:
        dh = scale * dz
    return dict(dh=dh, dhlat=dh.sum(axis=3), dw3=np.einsum("gdbq,gcbq->gdc", dh, fw["p"]),
                dpts=np.einsum("gdc,gdbq->gcbq", fw["w3"], dh).reshape(G, 3, B * P), dgamma=dgamma, dbeta=dbeta)


def band(fw):
    """|z| <= tau_d, tau_d = 32 2^-24 (|scale_d| max|h_d| + |shift_d|): where the roundings of h, of the fma and of the fp32
    statistics can move z across zero."""
    tau = 32 * 2.0 ** -24 * (np.abs(fw["scale"]) * np.abs(fw["h"]).max(axis=(2, 3)) + np.abs(fw["shift"]))
    return np.abs(fw["z"]) <= tau[:, :, None, None]


def lds_bytes(B, P, bwd):
    """What a K9 workgroup asks of LDS: the patch's points [3][B P], 32 latent rows [32][B], and in the backward the
    [8][64][12] buffer of the channel-tile sum."""
    return 4 * (3 * B * P + 32 * B + (8 * 64 * 12 if bwd else 0))


# ----------------------------------------------------------------------------------------------------------- the cases
class Case:
    """One launch: fp32 inputs as the kernel gets them (``w`` holds NaN outside its three point columns)."""

    def __init__(self, name, G, D, B, P, L, ldw, training, kind="plain", accumulate=False, contiguous=False):
        self.name, self.G, self.D, self.B, self.P, self.L, self.ldw = name, G, D, B, P, L, ldw
        self.training, self.kind, self.accumulate, self.contiguous = training, kind, accumulate, contiguous

    def __repr__(self):
        return self.name

    def build(self, seed):
        G, D, B, P, L = self.G, self.D, self.B, self.P, self.L
        rng = np.random.default_rng([seed, G, D, B, P, L, int(self.training), sum(map(ord, self.kind))])
        f = np.float32
        self.seed = seed
        self.pts = np.tanh(rng.standard_normal((G, 3, B * P))).astype(f)
        w3 = (0.5 * rng.standard_normal((G, D, 3))).astype(f)
        self.hlat = rng.standard_normal((G, D, B)).astype(f)
        self.gamma = (0.5 * rng.standard_normal(G * D) + 1.0).astype(f)
        self.beta = (0.1 * rng.standard_normal(G * D)).astype(f)
        self.rmean = (0.3 * rng.standard_normal(G * D)).astype(f)
        self.rvar = (0.5 + rng.random(G * D)).astype(f)
        self.dout = rng.standard_normal((G, D, B * P)).astype(f)
        self.cancelled = np.zeros((G, D), bool)          # channels whose float64 gradients are zero by cancellation
        self.dead = np.zeros((G, D), bool)               # channels that must contribute exact zeros
        self.exact_kink = np.zeros((G, D), bool)         # channels with z == 0 exactly
        d = np.arange(D)
        gam, bet = self.gamma.reshape(G, D), self.beta.reshape(G, D)
        if self.kind in ("offset1", "offset7"):
            # |hlat| = 60 sigma of the point part: the 1-shot episode's conditioning (one cloud), and the same common
            # offset with a per-cloud variation of order sigma
            sel = d % 2 == 0
            sigma = np.einsum("gdc,gce->gde", w3.astype(np.float64), self.pts.astype(np.float64)).std(axis=2)
            sign = np.where(d % 4 == 0, 1.0, -1.0)
            vary = (0.01 if self.kind == "offset1" else 1.0) * rng.standard_normal((G, D, B))
            off = (60.0 * sign)[None, :, None] * sigma[:, :, None] + sigma[:, :, None] * vary
            self.hlat[:, sel] = off[:, sel].astype(f)
        elif self.kind == "dead":
            sel = (d % 3 == 0) | (d >= 64)               # the last channel tile (64..69) is dead as a whole
            gam[:, sel] = np.abs(gam[:, sel]) + f(0.1)
            bet[:, sel] = f(-10.0)
            self.dead[:, sel] = True
        elif self.kind == "gamma":
            gam[:, d % 4 == 0] = f(0.0)
            gam[:, d % 4 == 1] = -np.abs(gam[:, d % 4 == 1]) - f(0.1)
        elif self.kind == "zerovar":
            assert B == 1 and self.training
            w3[:, d % 2 == 0] = f(0.0)
            self.cancelled[:, d % 2 == 0] = True
        elif self.kind == "kink_eval":
            assert not self.training
            sel = d % 2 == 0
            w3[:, sel] = f(0.0)
            self.hlat[:, sel] = f(0.0)
            bet[:, sel] = f(0.0)
            self.rmean.reshape(G, D)[:, sel] = f(0.0)
            self.exact_kink[:, sel] = True
        else:
            assert self.kind == "plain", self.kind
        self.w = np.full((G, D, self.ldw), np.nan, f)
        self.w[:, :, L:L + 3] = w3
        if self.accumulate:
            self.prior = dict(dw3=rng.standard_normal((G, D, 3)).astype(f), dgamma=rng.standard_normal(G * D).astype(f),
                              dbeta=rng.standard_normal(G * D).astype(f))
        else:
            self.prior = None
        return self

    def reference(self):
        return forward(self.hlat, self.w, self.L, self.pts, self.gamma, self.beta, self.B, self.P, EPS, self.training,
                       self.rmean, self.rvar)


def _cases():
    shapes = [  # G, D, B, P, L, ldw -- each the smallest that reaches its path (see tests/test_dec1_gpu.py)
        (3, 1, 1, 4, 0, 3), (2, 70, 7, 32, 24, 27), (1, 33, 3, 128, 5, 40), (1, 32, 5, 256, 0, 3),
        (2, 40, 130, 4, 24, 27), (1, 64, 9, 8, 5, 40), (1, 96, 16, 128, 0, 3), (1, 35, 48, 128, 24, 27)]
    out = []
    for G, D, B, P, L, ldw in shapes:
        for training in (True, False):
            out.append(Case(f"g{G}d{D}b{B}p{P}-{'train' if training else 'eval'}", G, D, B, P, L, ldw, training,
                            contiguous=(D, B) == (96, 16)))
    out.append(Case("g2d70b7p32-train-accumulate", 2, 70, 7, 32, 24, 27, True, accumulate=True))
    out.append(Case("g1d33b3p128-train-accumulate", 1, 33, 3, 128, 5, 40, True, accumulate=True))
    for kind, B, training in (("offset1", 1, True), ("offset7", 7, True), ("dead", 7, True), ("gamma", 7, True),
                              ("zerovar", 1, True), ("kink_eval", 7, False)):
        out.append(Case(f"g2d70b{B}p32-{kind}", 2, 70, B, 32, 24, 27, training, kind=kind))
    return out


CASES = _cases()
CASE_BY_NAME = {c.name: c for c in CASES}


def case(name, seed):
    c = CASE_BY_NAME[name]
    return Case(c.name, c.G, c.D, c.B, c.P, c.L, c.ldw, c.training, c.kind, c.accumulate, c.contiguous).build(seed)


# ---------------------------------------------------------------------------------------------------- the fp32 yardstick
def yardstick(c, device="cpu"):
    """The same split formulation in plain torch fp32 on the same inputs: broadcast add of an einsum, ``F.batch_norm``,
    ``relu``, autograd; the per-channel constants from plain fp32 tensor ops."""
    import torch
    import torch.nn.functional as F
    G, D, B, P, L = c.G, c.D, c.B, c.P, c.L
    t = lambda a: torch.tensor(np.ascontiguousarray(a), device=device)
    hlat, w3, pts = t(c.hlat).requires_grad_(), t(c.w[:, :, L:L + 3]).requires_grad_(), t(c.pts).requires_grad_()
    gamma, beta = t(c.gamma).requires_grad_(), t(c.beta).requires_grad_()
    h = hlat[..., None] + torch.einsum("gdc,gcbq->gdbq", w3, pts.view(G, 3, B, P))
    x = h.reshape(1, G * D, B * P)
    if c.training:
        y = F.batch_norm(x, None, None, gamma, beta, True, 0.0, EPS)
    else:
        y = F.batch_norm(x, t(c.rmean), t(c.rvar), gamma, beta, False, 0.0, EPS)
    out = torch.relu(y).view(G, D, B * P)
    out.backward(t(c.dout))
    with torch.no_grad():
        xs = x[0]
        if c.training:
            mean, var = xs.mean(1), xs.var(1, unbiased=False)
        else:
            mean, var = t(c.rmean), t(c.rvar)
        rstd = 1.0 / torch.sqrt(var + EPS)
        scale = gamma * rstd
        chan = torch.stack([scale, beta - mean * scale, mean, rstd])
        res = dict(out=out, chan=chan, dhlat=hlat.grad, dw3=w3.grad, dpts=pts.grad, dgamma=gamma.grad, dbeta=beta.grad)
        if c.training:
            res["bmean"] = mean
            res["bvar"] = xs.var(1, unbiased=True) if B * P > 1 else var
    return {k: v.detach().cpu().numpy() for k, v in res.items()}


def rounded_reference(c, fw, bw=None):
    """What a faultless fp32 kernel would return: the float64 reference rounded to fp32 (``prior`` added where the case
    accumulates)."""
    f = np.float32
    bw = backward(fw, c.dout, fw["z"] > 0) if bw is None else bw
    got = dict(out=fw["out"].reshape(c.G, c.D, -1).astype(f),
               chan=np.stack([fw[k].reshape(-1) for k in ("scale", "shift", "mean", "rstd")]).astype(f),
               dhlat=bw["dhlat"].astype(f), dw3=bw["dw3"].astype(f), dpts=bw["dpts"].astype(f),
               dgamma=bw["dgamma"].reshape(-1).astype(f), dbeta=bw["dbeta"].reshape(-1).astype(f))
    if c.training:
        got["bmean"], got["bvar"] = fw["batch_mean"].reshape(-1).astype(f), fw["batch_var_unbiased"].reshape(-1).astype(f)
    if c.prior is not None:
        for k, v in c.prior.items():
            got[k] = (got[k].astype(np.float64) + v).astype(f)
    return got


# ------------------------------------------------------------------- the whole layer (the two autograd functions' subject)
LAYER1_SEEDS = {(7,): 0, (2, 5): 0}     # batches -> a seed whose kink band is empty (asserted where it is used)


def layer1_inputs(seed, batches, G=2, D=70, L=24, P=32):
    """fp32 inputs of ``relu(BN(conv1(cat(x.repeat, pts))))`` for G patch MLPs: the stacked [G,D,L+3] weight, biases, the
    latents of all decodes in order, their patch points side by side, and the upstream gradient."""
    B = sum(batches)
    rng = np.random.default_rng([seed, 91, B, len(batches)])
    f = np.float32
    w1 = (rng.standard_normal((G, D, L + 3)) / np.sqrt(L + 3.0)).astype(f)
    w1[:, :, L:] = (0.5 * rng.standard_normal((G, D, 3))).astype(f)
    return dict(w1=w1, b1=(0.1 * rng.standard_normal((G, D, 1))).astype(f), x=rng.standard_normal((B, L)).astype(f),
                pts=np.tanh(rng.standard_normal((G, 3, B * P))).astype(f),
                gamma=(0.5 * rng.standard_normal(G * D) + 1.0).astype(f), beta=(0.1 * rng.standard_normal(G * D)).astype(f),
                dout=rng.standard_normal((G, D, B * P)).astype(f), P=P, L=L, batches=tuple(batches))


def layer1_band(inp):
    """Elements of the float64 forward inside the kink band, over all decodes."""
    L, P, n, b0 = inp["L"], inp["P"], 0, 0
    w, x = inp["w1"].astype(np.float64), inp["x"].astype(np.float64)
    for Bi in inp["batches"]:
        hlat = np.einsum("gdl,bl->gdb", w[:, :, :L], x[b0:b0 + Bi]) + inp["b1"].astype(np.float64)
        fw = forward(hlat, w, L, inp["pts"][:, :, b0 * P:(b0 + Bi) * P], inp["gamma"], inp["beta"], Bi, P, EPS, True)
        n += int(band(fw).sum())
        b0 += Bi
    return n


def layer1_torch(inp, dtype, split):
    """Training mode, each decode with its own batch statistics.  ``split=False``: the literal formulation -- conv1d of
    cat(x.repeat, pts) with the full weight, F.batch_norm, relu, per patch and decode; ``split=True``: latent product plus
    an einsum over the three point columns.  Returns the output, the statistics [n, 2, G*D] (mean, unbiased variance),
    the gradients, and the uncancelled scale of the bias gradient (sum of |d loss / d conv1 output|)."""
    import torch
    import torch.nn.functional as F
    L, P, batches = inp["L"], inp["P"], inp["batches"]
    t = lambda k: torch.tensor(inp[k], dtype=dtype).requires_grad_()
    w1, b1, x, pts, gamma, beta = (t(k) for k in ("w1", "b1", "x", "pts", "gamma", "beta"))
    G, D, _ = w1.shape
    outs, stats, pre, b0 = [], [], [], 0
    for Bi in batches:
        cols = slice(b0 * P, (b0 + Bi) * P)
        if split:
            hlat = torch.baddbmm(b1, w1[..., :L], x[b0:b0 + Bi].t().unsqueeze(0).expand(G, L, Bi))
            h = hlat[..., None] + torch.einsum("gdc,gcbq->gdbq", w1[..., L:], pts[:, :, cols].reshape(G, 3, Bi, P))
            h = h.permute(2, 0, 1, 3).reshape(Bi, G * D, P)
        else:
            xr = x[b0:b0 + Bi].unsqueeze(2).repeat(1, 1, P)
            h = torch.cat([F.conv1d(torch.cat((xr, pts[g, :, cols].reshape(3, Bi, P).permute(1, 0, 2)), dim=1),
                                    w1[g].unsqueeze(2), b1[g, :, 0]) for g in range(G)], dim=1)          # [Bi, G*D, P]
        h.retain_grad()
        pre.append(h)
        rm, rv = torch.zeros(G * D, dtype=dtype), torch.zeros(G * D, dtype=dtype)
        y = torch.relu(F.batch_norm(h, rm, rv, gamma, beta, True, 1.0, EPS))
        stats.append(torch.stack([rm, rv]))
        outs.append(y.reshape(Bi, G, D, P).permute(1, 2, 0, 3).reshape(G, D, Bi * P))
        b0 += Bi
    out = torch.cat(outs, dim=2)
    out.backward(torch.tensor(inp["dout"], dtype=dtype))
    n = lambda v: v.detach().numpy().astype(np.float64)
    res = dict(out=n(out), stats=n(torch.stack(stats)), w1=n(w1.grad), b1=n(b1.grad), x=n(x.grad), pts=n(pts.grad),
               gamma=n(gamma.grad), beta=n(beta.grad))
    res["b1_scale"] = float(sum(h.grad.abs().sum(dim=(0, 2)) for h in pre).max())
    return res


def compare_layer1(what, got, truth, yard, factor, show=print):
    """The yardstick rule on the whole layer's outputs and gradients; ``b1``'s gradient cancels in training mode and is
    held against the sum of the magnitudes it is the sum of."""
    missed = []
    for k in ("out", "stats.mean", "stats.var", "w1", "b1", "x", "pts", "gamma", "beta"):
        if k.startswith("stats."):
            i = 0 if k == "stats.mean" else 1
            g, t, y = got["stats"][:, i], truth["stats"][:, i], yard["stats"][:, i]
        else:
            g, t, y = got[k], truth[k], yard[k]
        scale = truth["b1_scale"] if k == "b1" else float(np.abs(t).max())
        dk, dy = _dev(g.reshape(t.shape), t, scale), _dev(y.reshape(t.shape), t, scale)
        bound = max(factor * dy, FLOOR)
        show(f"DEVIATION {what} {k}: kernel {dk:.3e} yardstick {dy:.3e} ratio {_ratio(dk, dy)} bound {bound:.3e}")
        if not dk <= bound:
            missed.append((k, dk, bound))
    assert not missed, (what, "beyond factor x yardstick", missed)


# --------------------------------------------------------------------------------------------------------- comparison
def _dev(got, truth, scale):
    diff = np.abs(np.asarray(got, np.float64) - truth)
    if not np.all(np.isfinite(diff)):
        return float("inf")
    scale = np.broadcast_to(scale, diff.shape)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(diff == 0, 0.0, diff / scale)           # a non-zero difference on a zero scale: inf
    return float(r.max())


def _ratio(dk, dy):
    """kernel / yardstick as text; 'floor' where the kernel is within 16 ulps of the scale, whatever the yardstick is."""
    if dk <= FLOOR:
        return "floor" if dy == 0 else f"{dk / dy:.2f}(floor)"
    return f"{dk / dy:.2f}" if dy > 0 else "inf"


def deviations(c, fw, got, prior=None):
    """Maximum deviation of every compared quantity from float64, each scaled by the quantity's float64 maximum (channels
    whose gradients cancel to zero in float64: by |gamma| rstd max|dout|).  Asserts what is exact: the mask outside the
    kink band, zeros where z is exactly zero, zeros from dead channels."""
    G, D, B, P = c.G, c.D, c.B, c.P
    out = np.asarray(got["out"], np.float64).reshape(G, D, B, P)
    assert np.all(np.isfinite(out)), (c, "out holds non-finite values")
    mask, mask64, bd = out > 0, fw["z"] > 0, band(fw)
    wrong = (mask != mask64) & ~bd
    assert not wrong.any(), (c, "ReLU mask differs from float64 outside the kink band", int(wrong.sum()))
    zero = fw["z"] == 0
    assert not (out[zero] != 0).any(), (c, "out is not 0 where z is exactly 0")
    bw = backward(fw, c.dout, mask)
    gmax = lambda a: float(np.abs(a).max())
    res = {"out": _dev(out, fw["out"], gmax(fw["out"]))}
    chan = np.asarray(got["chan"], np.float64).reshape(4, G, D)
    for i, k in enumerate(("scale", "shift", "mean", "rstd")):
        res["chan." + k] = _dev(chan[i], fw[k], gmax(fw[k]))
    if c.training:
        res["batch_mean"] = _dev(np.reshape(got["bmean"], (G, D)), fw["batch_mean"], gmax(fw["batch_mean"]))
        res["batch_var"] = _dev(np.reshape(got["bvar"], (G, D)), fw["batch_var_unbiased"], gmax(fw["batch_var_unbiased"]))
    cs = np.where(c.cancelled, np.abs(fw["scale"]) * gmax(c.dout), 0.0)          # [G,D]
    truth = dict(dhlat=bw["dhlat"], dw3=bw["dw3"], dpts=bw["dpts"], dgamma=bw["dgamma"], dbeta=bw["dbeta"])
    if prior is not None:
        for k, v in prior.items():
            truth[k] = truth[k] + np.asarray(v, np.float64).reshape(truth[k].shape)
    # with ONE cloud in training mode dhlat is the sum of dh over the whole channel: zero in float64, in every channel
    ch = np.abs(fw["scale"]) * gmax(c.dout) if (B == 1 and c.training) else cs
    res["dhlat"] = _dev(got["dhlat"], truth["dhlat"], np.maximum(gmax(truth["dhlat"]), ch)[:, :, None])
    res["dW"] = _dev(got["dw3"], truth["dw3"], np.maximum(gmax(truth["dw3"]), cs)[:, :, None])
    res["dpts"] = _dev(got["dpts"], truth["dpts"], gmax(truth["dpts"]))
    res["dgamma"] = _dev(np.reshape(got["dgamma"], (G, D)), truth["dgamma"], gmax(truth["dgamma"]))
    res["dbeta"] = _dev(np.reshape(got["dbeta"], (G, D)), truth["dbeta"], gmax(truth["dbeta"]))
    for sel in (c.dead, c.exact_kink):               # out and every gradient of these channels: exactly zero
        if sel.any():
            for k in ("dhlat", "dw3"):
                assert not np.asarray(got[k])[sel].any(), (c, k, "not exactly zero in a dead / exact-kink channel")
            assert not out[sel].any() and not np.reshape(got["dgamma"], (G, D))[sel].any(), (c, "dead channel")
            assert not np.reshape(got["dbeta"], (G, D))[sel].any(), (c, "dbeta of a dead channel")
    return res


def compare(c, fw, got, yard, factor, show=print):
    """Raises unless every quantity of ``got`` is within ``max(factor x the yardstick's deviation, FLOOR)`` of float64.
    Prints one DEVIATION line per quantity before it asserts; returns the rows."""
    dk = deviations(c, fw, got, c.prior)
    dy = deviations(c, fw, yard)
    rows, missed = [], []
    for k in dk:
        bound = max(factor * dy[k], FLOOR)
        rows.append((k, dk[k], dy[k], bound))
        show(f"DEVIATION {c.name} seed={c.seed} {k}: kernel {dk[k]:.3e} yardstick {dy[k]:.3e} ratio {_ratio(dk[k], dy[k])} "
             f"bound {bound:.3e}")
        if not dk[k] <= bound:
            missed.append((k, dk[k], bound))
    assert not missed, (c, c.seed, "beyond factor x yardstick", missed)
    return rows
