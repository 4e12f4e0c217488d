"""The fused EdgeConv kernels (K4b, fpsg_amd/csrc/edgeconv.hip) against the exact and float64 references of
tests/_edgeconv_ref.py: every kernel through the C ABI on inputs made on the CPU, then ``_EdgeConvBNMax`` end to end
with ``PQ`` as the exact fp32 input.  With ``PQ`` exact an edge activation is one fp32 addition, so the selected value
and slot are compared bit for bit and every sum against float64 with a bound derived from its number of fp32 terms.

Every output buffer carries 64 guard elements behind it, filled (like the buffer) with a NaN bit pattern."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _edgeconv_ref as R

pytestmark = pytest.mark.gpu

EPS = R.EPS32
# "1 ulp" of a value v below is 2^-23 |v|: each fp32 rounding is at most 2^-24 relative, and the negative side of
# LeakyReLU takes two in a row (the fma, then the product with the slope).  In units of the fp32 spacing AT v the same
# two roundings reach 1.3 (z just above a power of two, 0.2 z just below the next binade), so that unit would refuse
# correctly rounded arithmetic.
ULP = 2.0 ** -23
GUARD = 64
FORMS = ["grouped", "one_edge"]


def _guarded(n, dtype, dev):
    if dtype == torch.uint8:
        return torch.full((n + GUARD,), 0xFF, dtype=torch.uint8, device=dev)
    return torch.full((n + GUARD,), float("nan"), dtype=dtype, device=dev)


def _take(buf, shape):
    """The payload of a guarded buffer as numpy; the guard must still hold its fill pattern."""
    n = int(np.prod(shape))
    tail = buf[n:].cpu()
    if buf.dtype == torch.uint8:
        assert bool((tail == 0xFF).all()), "guard bytes behind a uint8 output were written"
    else:
        fill = torch.full((GUARD,), float("nan"), dtype=buf.dtype).view(torch.int32)
        assert torch.equal(tail.view(torch.int32), fill), "guard elements behind a float output were written"
    return buf[:n].cpu().numpy().reshape(shape)


def _set_form(monkeypatch, form):
    if form == "one_edge":
        monkeypatch.setenv("FPSG_EDGECONV_BWD", "one_edge")
    else:
        monkeypatch.delenv("FPSG_EDGECONV_BWD", raising=False)


def _lib():
    from fpsg_amd import _hip
    return _hip.load()


def _ok(rc, what):
    from fpsg_amd import _hip
    _hip.check(rc, what)


def _stream():
    return torch.cuda.current_stream().cuda_stream


# ---- fpsg_edgeconv_fwd / fpsg_edgeconv_bwd -------------------------------------------------------------------------

SHAPES = [(1, 1, 1),        # one point
          (3, 7, 3),        # k below the group count
          (2, 33, 20),      # one point past a full forward workgroup at Co = 64
          (9, 13, 5),       # second lap of the cloud -> XCD mapping; 18 (cloud, slice) pairs in the Co = 256 backward
          (2, 40, 21),      # one neighbour past a round of 20
          (1, 50, 64),      # the largest k
          (2, 300, 20)]     # the size of the tests of the two forms against each other
KINDS = ["random", "hubs", "degrees", "same"]


def _graph(kind, B, N, k, rng):
    if kind == "random":                      # repeated entries: by chance, and slot k-1 repeats slot 0
        idx = rng.integers(0, N, size=(B, N, k))
        idx[:, :, k - 1] = idx[:, :, 0]
    elif kind == "hubs":                      # points 0..2 in every list: in-degree N
        idx = rng.integers(0, N, size=(B, N, k))
        for j in range(min(3, k, N)):
            idx[:, :, j] = j
    elif kind == "degrees":                   # in-degree exactly 64 at point 0, 65 at point 1, 0 at point 2
        idx = rng.integers(3, N, size=(B, N * k))
        for b in range(B):
            slots = rng.permutation(N * k)[:129]
            idx[b, slots[:64]] = 0
            idx[b, slots[64:]] = 1
        idx = idx.reshape(B, N, k)
    else:                                     # every slot of a list names one point: all candidates tie
        idx = np.repeat(rng.integers(0, N, size=(B, N, 1)), k, axis=2)
    return idx.astype(np.int32)


def _kernel_cases():
    cases = []
    for (B, N, k) in SHAPES:
        for kind in KINDS:
            if kind == "degrees" and (N < 4 or N * k < 2 * 129):
                continue
            for Co in (64, 128, 256):
                cases.append((B, N, k, Co, kind))
    return cases


@pytest.fixture(scope="module", params=_kernel_cases(), ids=lambda p: "B%d-N%d-k%d-Co%d-%s" % p)
def case(request, gpu):
    B, N, k, Co, kind = request.param
    rng = np.random.default_rng(1000 * N + 10 * k + Co + KINDS.index(kind))
    idx = _graph(kind, B, N, k, rng)
    deg = R.in_degree(idx, N)
    if kind == "hubs":
        assert (deg[:, :min(3, k, N)] >= N).all()
    if kind == "degrees":
        assert (deg[:, 0] == 64).all() and (deg[:, 1] == 65).all() and (deg[:, 2] == 0).all()
    PQ = rng.standard_normal((B, N, 2 * Co)).astype(np.float32)
    if kind == "random":                      # planted exact ties between DIFFERENT neighbours, in any pair of slots
        PQ[:, :, 1:Co:4] = np.round(PQ[:, :, 1:Co:4] * 2) / 2
    sgn = (rng.uniform(0.5, 1.5, size=Co) * rng.choice([-1.0, 1.0], size=Co)).astype(np.float32)   # only the sign counts
    sgn[5] = np.float32(-0.0)                 # not below zero: the maximum
    assert (sgn < 0).any() and (sgn > 0).any()
    fwd = R.forward_exact(PQ, idx, sgn)
    if kind == "same":
        assert (fwd.jsel == 0).all()
    if kind == "random" and k >= 5 and N >= 7:
        y = R.edge_values(PQ, idx)
        assert ((y == fwd.ysel[:, :, None, :]).sum(axis=2) > 1)[..., 1:Co:4].any() and (fwd.jsel[..., 1:Co:4] > 0).any()
    dev = lambda a: torch.from_numpy(a).to(gpu)
    c = R.SimpleNamespace(B=B, N=N, k=k, Co=Co, kind=kind, idx=idx, deg=deg, PQ=PQ, sgn=sgn, fwd=fwd, rng=rng,
                          d_idx=dev(idx), d_PQ=dev(PQ), d_sgn=dev(sgn), bwd={})
    return c


def _run_fwd(c, stats):
    lib = _lib()
    B, N, k, Co = c.B, c.N, c.k, c.Co
    dev = c.d_PQ.device
    blocks = lib.fpsg_edgeconv_blocks(B, N, Co)
    ysel, jsel = _guarded(B * N * Co, torch.float32, dev), _guarded(B * N * Co, torch.uint8, dev)
    s1 = _guarded(B * N * Co, torch.float32, dev) if stats else None
    part = _guarded(blocks * 2 * Co, torch.float32, dev) if stats else None
    _ok(lib.fpsg_edgeconv_fwd(c.d_PQ.data_ptr(), c.d_idx.data_ptr(), c.d_sgn.data_ptr(), B, N, k, Co, ysel.data_ptr(),
                              jsel.data_ptr(), s1.data_ptr() if stats else None, part.data_ptr() if stats else None,
                              _stream()), "fpsg_edgeconv_fwd")
    torch.cuda.synchronize()
    out = R.SimpleNamespace(ysel=_take(ysel, (B, N, Co)), jsel=_take(jsel, (B, N, Co)))
    if stats:
        out.s1 = _take(s1, (B, N, Co))
        out.part = _take(part, (blocks, 2, Co))
    return out


@pytest.mark.parametrize("form", FORMS)
def test_forward_kernel_is_exact_and_its_sums_are_within_fp32_bounds(case, form, monkeypatch):
    """fpsg_edgeconv_fwd: ysel and jsel bit for bit (ties: lowest slot, in both forms), s1 within (k + 2) 2^-24 sum_j |y|,
    the column sums of the per-workgroup partial rows within (n_b + 8) 2^-24 sum |y| resp. sum y^2, where
    n_b = 4 ppw k is the number of fp32 terms a workgroup adds; without s1 and part (eval mode) the same selection."""
    c, ref = case, case.fwd
    _set_form(monkeypatch, form)
    got = _run_fwd(c, stats=True)
    assert np.array_equal(got.ysel.view(np.int32), ref.ysel.view(np.int32))
    assert np.array_equal(got.jsel, ref.jsel)
    err = np.abs(got.s1.astype(np.float64) - ref.s1)
    bound = (c.k + 2) * EPS * ref.abs_s1
    assert (err <= bound).all(), float((err / np.maximum(bound, 1e-300)).max())
    n_b = 4 * {64: 8, 128: 4, 256: 2}[c.Co] * c.k
    tot = got.part.astype(np.float64).sum(axis=0)                             # [2, Co]
    assert np.isfinite(tot).all()
    assert (np.abs(tot[0] - ref.sum_y) <= (n_b + 8) * EPS * ref.sum_abs).all()
    assert (np.abs(tot[1] - ref.sum_y2) <= (n_b + 8) * EPS * ref.sum_y2).all()
    ev = _run_fwd(c, stats=False)
    assert np.array_equal(ev.ysel.view(np.int32), ref.ysel.view(np.int32)) and np.array_equal(ev.jsel, ref.jsel)


def _bwd_reference(c, stats):
    if stats not in c.bwd:
        rng = np.random.default_rng(c.N * 77 + c.k + c.Co)
        dzs = rng.standard_normal((c.B, c.N, c.Co)).astype(np.float32)
        coef = (0.1 * rng.standard_normal((3, c.Co))).astype(np.float32) if stats else np.zeros((3, c.Co), np.float32)
        dPQ, T = R.backward_per_edge(dzs, c.fwd.jsel, c.PQ, c.idx, coef)
        c.bwd[stats] = (dzs, coef, dPQ, T)
    return c.bwd[stats]


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("stats", [True, False], ids=["train", "eval"])
def test_backward_kernel_against_the_per_edge_definition(case, form, stats, monkeypatch, gpu):
    """fpsg_edgeconv_bwd on the jsel and s1 of the same case's (reference) forward, random dzs and coef, through
    _reverse_graph: every element of dPQ within (d + k + 8) 2^-24 T of the float64 per-edge sum -- d the in-degree of
    the element's point, T the sum of the absolute values of its terms -- and bit-identical from run to run.
    ``eval``: s1 = NULL and coef = 0."""
    from fpsg_amd.dgcnn import _reverse_graph
    c = case
    lib = _lib()
    B, N, k, Co = c.B, c.N, c.k, c.Co
    dzs, coef, ref, T = _bwd_reference(c, stats)
    rev, off = _reverse_graph(c.d_idx)
    order = np.stack([np.argsort(c.idx[b].ravel(), kind="stable") for b in range(B)])
    assert np.array_equal(rev.cpu().numpy(), order)
    assert np.array_equal(off.cpu().numpy()[:, 1:], np.cumsum(c.deg, axis=1))
    d_dzs, d_coef = torch.from_numpy(dzs).to(gpu), torch.from_numpy(coef).to(gpu)
    d_jsel = torch.from_numpy(c.fwd.jsel).to(gpu)
    d_s1 = torch.from_numpy(c.fwd.s1.astype(np.float32)).to(gpu) if stats else None
    _set_form(monkeypatch, form)

    def run():
        out = _guarded(B * N * 2 * Co, torch.float32, gpu)
        _ok(lib.fpsg_edgeconv_bwd(d_dzs.data_ptr(), d_jsel.data_ptr(), c.d_PQ.data_ptr(),
                                  d_s1.data_ptr() if stats else None, rev.data_ptr(), off.data_ptr(), d_coef.data_ptr(),
                                  B, N, k, Co, out.data_ptr(), _stream()), "fpsg_edgeconv_bwd")
        torch.cuda.synchronize()
        return _take(out, (B, N, 2 * Co))

    a, a2 = run(), run()
    assert np.array_equal(a.view(np.int32), a2.view(np.int32))
    assert np.isfinite(a).all()
    err = np.abs(a.astype(np.float64) - ref)
    bound = (c.deg[:, :, None] + k + 8) * EPS * T
    worst = float((err / np.maximum(bound, 1e-300)).max())
    assert (err <= bound).all(), worst


# ---- the elementwise kernels around them ---------------------------------------------------------------------------

def _epilogue_inputs(rows, Co):
    """ysel, g, scale (both signs, |scale| >= 0.3), shift; every ysel whose float64 z = ysel scale + shift has
    |z| < 1e-3 is moved by 0.01 (|dz| >= 3e-3), so that no element sits at the LeakyReLU kink and none is excluded."""
    rng = np.random.default_rng(rows * 7 + Co)
    ysel = rng.standard_normal((rows, Co)).astype(np.float32)
    g = rng.standard_normal((rows, Co)).astype(np.float32)
    scale = (rng.uniform(0.3, 1.5, size=Co) * rng.choice([-1.0, 1.0], size=Co)).astype(np.float32)
    shift = (0.5 * rng.standard_normal(Co)).astype(np.float32)
    z = ysel.astype(np.float64) * scale + shift
    ysel[np.abs(z) < 1e-3] += np.float32(0.01)
    z = ysel.astype(np.float64) * scale + shift
    assert np.abs(z).min() >= 1e-3
    return ysel, g, scale, shift, z


@pytest.mark.parametrize("Co", [64, 128, 256])
@pytest.mark.parametrize("rows", [1, 3, 255, 256, 257, 1000])
def test_activation_and_backward_prep_kernels(gpu, rows, Co):
    """fpsg_edgeconv_act: out within 1 ulp of the float64 LeakyReLU(ysel scale + shift) (an fma, then one product on the
    negative side: two roundings).  fpsg_edgeconv_bwd_prep: dzs within 2 ulp of g LeakyReLU'(z) scale, the column sums
    of its partial rows within (r + 8) 2^-24 sum |dz| resp. sum |dz ysel| of float64, r = 256 rows per workgroup."""
    lib = _lib()
    ysel, g, scale, shift, z = _epilogue_inputs(rows, Co)
    up = lambda a: torch.from_numpy(a).to(gpu)
    d_y, d_g, d_sc, d_sh = up(ysel), up(g), up(scale), up(shift)
    out = _guarded(rows * Co, torch.float32, gpu)
    _ok(lib.fpsg_edgeconv_act(d_y.data_ptr(), d_sc.data_ptr(), d_sh.data_ptr(), R.SLOPE, rows, Co, out.data_ptr(),
                              _stream()), "fpsg_edgeconv_act")
    torch.cuda.synchronize()
    ref = np.where(z > 0, z, z * R.SLOPE)
    err = np.abs(_take(out, (rows, Co)).astype(np.float64) - ref)
    assert (err <= ULP * np.abs(ref)).all(), float((err / np.abs(ref)).max() / ULP)

    blocks = lib.fpsg_edgeconv_prep_blocks(rows)
    assert blocks == (rows + 255) // 256
    dzs = _guarded(rows * Co, torch.float32, gpu)
    part = _guarded(blocks * 2 * Co, torch.float32, gpu)
    _ok(lib.fpsg_edgeconv_bwd_prep(d_g.data_ptr(), d_y.data_ptr(), d_sc.data_ptr(), d_sh.data_ptr(), R.SLOPE, rows, Co,
                                   dzs.data_ptr(), part.data_ptr(), _stream()), "fpsg_edgeconv_bwd_prep")
    torch.cuda.synchronize()
    dz = g.astype(np.float64) * np.where(z > 0, 1.0, R.SLOPE)
    ref = dz * scale
    err = np.abs(_take(dzs, (rows, Co)).astype(np.float64) - ref)
    assert (err <= 2 * ULP * np.abs(ref)).all(), float((err / np.abs(ref)).max() / ULP)
    tot = _take(part, (blocks, 2, Co)).astype(np.float64).sum(axis=0)
    dzy = dz * ysel
    assert (np.abs(tot[0] - dz.sum(axis=0)) <= (256 + 8) * EPS * np.abs(dz).sum(axis=0)).all()
    assert (np.abs(tot[1] - dzy.sum(axis=0)) <= (256 + 8) * EPS * np.abs(dzy).sum(axis=0)).all()


@pytest.mark.parametrize("Co", [64, 128, 256])
@pytest.mark.parametrize("blocks", [1, 3, 257, 600])
def test_backward_finalize_kernel(gpu, blocks, Co):
    """fpsg_edgeconv_bwd_finalize on synthetic partial rows against float64 sums of the same rows: dbeta to 2e-7 (one
    rounding after fp64 sums), dgamma and coef[1] to 2e-7 of |sum dz y| + |mean sum dz| (the difference cancels),
    coef[0] to 2e-7, coef[2] = mean; training = 0 gives coef that is exactly zero and the same dbeta, dgamma."""
    lib = _lib()
    rng = np.random.default_rng(blocks * 3 + Co)
    part = (256 * rng.standard_normal((blocks, 2, Co))).astype(np.float32)
    part[:, 1] += np.float32(0.4) * part[:, 0]                                # sum dz y correlated with sum dz: it cancels
    chan = np.stack([rng.uniform(0.3, 1.5, size=Co) * rng.choice([-1.0, 1.0], size=Co), rng.standard_normal(Co),
                     0.5 * rng.standard_normal(Co), rng.uniform(0.5, 2.0, size=Co)]).astype(np.float32)
    count = float(blocks * 256 * 20)
    d_part, d_chan = torch.from_numpy(part).to(gpu), torch.from_numpy(chan).to(gpu)
    scale, mean, rstd = (chan[i].astype(np.float64) for i in (0, 2, 3))
    s0, s1 = part[:, 0].astype(np.float64).sum(axis=0), part[:, 1].astype(np.float64).sum(axis=0)
    cancel = (np.abs(s1) + np.abs(mean * s0)) * rstd
    dg_ref = (s1 - mean * s0) * rstd
    for training in (1, 0):
        dgamma, dbeta = _guarded(Co, torch.float32, gpu), _guarded(Co, torch.float32, gpu)
        coef = _guarded(3 * Co, torch.float32, gpu)
        _ok(lib.fpsg_edgeconv_bwd_finalize(d_part.data_ptr(), blocks, d_chan.data_ptr(), count, Co, training,
                                           dgamma.data_ptr(), dbeta.data_ptr(), coef.data_ptr(), _stream()),
            "fpsg_edgeconv_bwd_finalize")
        torch.cuda.synchronize()
        dgamma, dbeta, coef = _take(dgamma, (Co,)), _take(dbeta, (Co,)), _take(coef, (3, Co))
        assert (np.abs(dbeta - s0) <= 2e-7 * np.abs(s0)).all()
        assert (np.abs(dgamma - dg_ref) <= 2e-7 * cancel).all()
        if training:
            c0 = scale * s0 / count
            assert (np.abs(coef[0] - c0) <= 2e-7 * np.abs(c0)).all()
            assert (np.abs(coef[1] - scale * rstd * dg_ref / count) <= 2e-7 * np.abs(scale * rstd / count) * cancel).all()
            assert np.array_equal(coef[2], chan[2])
        else:
            assert (coef == 0).all()


# ---- _EdgeConvBNMax end to end, PQ as the exact input --------------------------------------------------------------

TENSORS = ("out", "running_mean", "running_var", "dPQ", "dgamma", "dbeta")


def _run_layer(case, training, gpu, fused):
    """The fused layer, or the same chain in plain fp32 torch ops (index, add, F.batch_norm, leaky_relu, max)."""
    up = lambda a: torch.from_numpy(a).to(gpu)
    PQ, gamma, beta = up(case.PQ).requires_grad_(), up(case.gamma).requires_grad_(), up(case.beta).requires_grad_()
    rm, rv = up(case.running_mean.copy()), up(case.running_var.copy())
    idx, Co = up(case.idx), case.Co
    if fused:
        from fpsg_amd.dgcnn import _EdgeConvBNMax
        out = _EdgeConvBNMax.apply(PQ, idx, gamma, beta, rm, rv, training, R.MOMENTUM, R.BN_EPS, R.SLOPE)
    else:
        y = PQ[..., :Co][torch.arange(case.B, device=gpu)[:, None, None], idx.long()] + PQ[:, :, None, Co:]
        z = F.batch_norm(y.permute(0, 3, 1, 2), rm, rv, gamma, beta, training, R.MOMENTUM, R.BN_EPS)
        out = F.leaky_relu(z, R.SLOPE).max(dim=-1)[0].transpose(1, 2)
    (out * up(case.w_out)).sum().backward()
    res = dict(out=out.detach(), running_mean=rm, running_var=rv, dPQ=PQ.grad, dgamma=gamma.grad, dbeta=beta.grad)
    return {name: t.double().cpu().numpy() for name, t in res.items()}


def _errors(case, ref, training, gpu):
    fused, lit = _run_layer(case, training, gpu, True), _run_layer(case, training, gpu, False)
    table = {}
    print("\n(B, N, k, Co, offset) = %s, %s" % ((case.B, case.N, case.k, case.Co, case.offset), "train" if training else "eval"))
    for name in TENSORS:
        want = getattr(ref, name)
        e_fused = float(np.abs(fused[name] - want).max() / np.abs(want).max())
        e_lit = float(np.abs(lit[name] - want).max() / np.abs(want).max())
        print("%-12s e_fused %.3e  e_lit %.3e  ratio %.2f" % (name, e_fused, e_lit, e_fused / max(e_lit, 1e-300)))
        table[name] = (e_fused, e_lit)
    return table, fused, lit


@pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("key", R.LAYER_CASES, ids=str)
def test_layer_against_float64_with_the_fp32_chain_as_yardstick(gpu, key, training):
    """out, the running statistics and the gradients of PQ, gamma and beta against layer64.  For each tensor
    e = max |x - f64| / max |f64|; the fused layer must meet e_fused <= max(4 e_lit, 32 2^-24), e_lit being the error
    of the same chain in plain fp32 torch ops from the same PQ.  The factor 4 covers another association of the same
    sums (fp32 workgroup partials here, torch's accumulation there), the floor the cases where the fp32 chain happens to
    land on the float64 value.  The cases with an offset spread |mean| / std of the channels up to 3."""
    case = R.layer_case(*key)
    ref = R.layer_ref(case, training)
    assert ref.kink_min >= 1e-4 and (ref.gap_min > 0 or ref.inexact_ties == 0)
    table, _, _ = _errors(case, ref, training, gpu)
    bad = {n: e for n, e in table.items() if not e[0] <= max(4 * e[1], 32 * EPS)}
    assert not bad, bad


@pytest.mark.parametrize("key", R.OFFSET12_CASES, ids=str)
def test_layer_statistics_at_twelve_standard_deviations_of_offset(gpu, key):
    """|mean| / std up to 12, four times what the network shows: only the derived bound of the one-pass fp32 statistics
    is asserted, on running_var: |d var| <= (n_b + 8) 2^-24 (E[y^2] + 2 |mean| E|y|) with n_b = 4 ppw k terms per
    workgroup partial, carried into running_var by momentum * count / (count - 1), plus 4 * 2^-24 |running_var| for the
    fp32 roundings of the update itself (1 - m, its product, the unbiased variance, the fma)."""
    case = R.layer_case(*key)
    ref = R.layer_ref(case, True)
    table, fused, _ = _errors(case, ref, True, gpu)
    n_b = 4 * {64: 8, 128: 4, 256: 2}[case.Co] * case.k
    dvar = (n_b + 8) * EPS * (ref.mean_y2 + 2 * np.abs(ref.mean) * ref.mean_abs_y)
    bound = R.MOMENTUM * ref.count / (ref.count - 1) * dvar + 4 * EPS * np.abs(ref.running_var)
    err = np.abs(fused["running_var"] - ref.running_var)
    print("running_var: worst error / bound %.3f" % float((err / bound).max()))
    assert (err <= bound).all(), float((err / bound).max())
    assert np.isfinite(fused["out"]).all() and np.isfinite(fused["dPQ"]).all()
