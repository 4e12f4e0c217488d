"""The streaming (non-temporal) kernel forms, ``NT = true``, at small shapes.

The shipped library takes a pass's streaming form when its largest tensor is beyond 300 MiB (``beyond_cache()``,
fpsg_amd/csrc/fpsg_common.h): the forms the full-size training step launches, and the ones no small shape reaches.  The
second build ``fpsg_amd/csrc/build/libfpsg_hip_stream.so`` is the same library with the threshold compiled to 0
(tests/_stream_lib.py), so every pass of it streams.  ``NT`` only chooses ``__builtin_nontemporal_load / _store`` in
place of a plain access (``ld_stream`` / ``st_stream``, ``stream_load`` / ``stream_store``; read in all five sources: no
arithmetic and no order depends on it), so every case asserts

  1. every output of the streaming library is BIT-identical to the shipped library's on the same inputs -- activations,
     gradients, partial sums, statistics, index outputs -- and
  2. the streaming library passes the reference comparison of the sibling form's own test (float64, the torch module
     chain, the three-kernel form), called as it stands with the handle swapped: same helper, same tolerance.  So a
     failure of 1 alone says "only the streaming form is wrong", a failure of both "both forms are".

Shapes are those tests/_dispatch.py lists for each sibling row (same template arguments, ``NT = false``), the smallest
that meets the row's other conditions, ragged where the sibling has a ragged case.  The guarded-buffer procedure of
tests/test_memory_contract_gpu.py runs on the second build for every entry that can select a streaming form, and one
training episode runs with the streaming forms chained through the Python wrappers.  Nothing here is meant to fault: every
call is one the header documents as valid."""
import copy

import pytest
import torch
import torch.nn as nn

import _dec1_ref as R
import _memory_contract as T
import _stream_lib as S
import test_bnact_gpu as bnact_tests
import test_dec1_gpu as dec1_tests
import test_winograd_gpu as wino_tests

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def libs():
    """(shipped, streaming): two handles, the thresholds 300 MiB and 0."""
    return S.both()


@pytest.fixture
def use(monkeypatch, libs):
    """use("shipped" | "stream"): the handle every Python wrapper gets from ``_hip.load()`` from here on."""
    from fpsg_amd import _hip

    def swap(which):
        lib = libs[("shipped", "stream").index(which)]
        monkeypatch.setattr(_hip, "_lib", lib)
        assert _hip.load() is lib
        return lib
    return swap


def _same_bits(shipped, stream):
    assert shipped.keys() == stream.keys()
    for name in shipped:
        a, b = shipped[name], stream[name]
        assert a.shape == b.shape and a.dtype == b.dtype, name
        assert bool(torch.isfinite(a.float()).all()), f"'{name}' of the shipped library is not finite"
        assert torch.equal(a, b), (f"'{name}': the streaming form differs from its cached sibling in "
                                   f"{int((a != b).sum())} of {a.numel()} elements")


def _both(use, produce):
    out = {}
    for which in ("shipped", "stream"):
        use(which)
        out[which] = produce()
    torch.cuda.synchronize()
    _same_bits(out["shipped"], out["stream"])
    return out


def _affine(C, gpu, both_signs=False):
    gamma = torch.randn(C, device=gpu) * (1.0 if both_signs else 0.5) + (0.0 if both_signs else 1.0)
    return gamma.requires_grad_(), (torch.randn(C, device=gpu) * 0.3).requires_grad_()


# ---- bnact.hip: bn_reduce_kernel<MODE, ACT, true>, bn_apply_kernel<MODE, ACT, true> ----------------------------------
# N L > 16384 (the sliced path) and L % 4 == 0 (the vector accesses that carry the hint); 8196 = 2 x 4096 + 4: a last
# segment of one vector; 37 images; every activation; training (the statistics pass <0, 0, true>) and evaluation
BN_CASES = [((37, 16, 56, 56), "relu", "train"), ((5, 9, 4096 + 4100), ("leaky", 0.1), "train"),
            ((24, 32, 2048), None, "train"), ((37, 16, 56, 56), "relu", "eval")]


@pytest.mark.parametrize("shape,act,mode", BN_CASES, ids=["relu-37x16x56x56-train", "leaky-5x9x8196-train",
                                                         "none-24x32x2048-train", "relu-37x16x56x56-eval"])
def test_bn_reduce_and_apply(gpu, use, shape, act, mode):
    from fpsg_amd.fused_bn import bn_act
    assert shape[0] * (shape[2] * (shape[3] if len(shape) == 4 else 1)) > 16384

    def produce():
        torch.manual_seed(sum(shape))
        C = shape[1]
        bn = (nn.BatchNorm2d if len(shape) == 4 else nn.BatchNorm1d)(C).to(gpu).train(mode == "train")
        with torch.no_grad():
            bn.weight.copy_(torch.randn(C) * 0.5 + 1)
            bn.bias.copy_(torch.randn(C) * 0.3)
        x = (torch.randn(*shape, device=gpu) * 1.7 + 0.4).requires_grad_()
        pb = (torch.randn(C, device=gpu) * 0.3).requires_grad_()
        y = bn_act(bn, x, act, pre_bias=pb)
        y.backward(torch.randn_like(y))
        return dict(y=y.detach(), dx=x.grad, dpre_bias=pb.grad, dgamma=bn.weight.grad, dbeta=bn.bias.grad,
                    running_mean=bn.running_mean.clone(), running_var=bn.running_var.clone())

    _both(use, produce)
    use("stream")
    bnact_tests.test_matches_torch_modules(gpu, shape, act, mode)
    if shape == (37, 16, 56, 56):       # a case of that test's own list
        bnact_tests.test_pre_bias_is_the_broadcast_add(gpu, shape, act, mode)


# ---- bnact.hip: bn_reduce_ext_kernel<1, true>, bn_max_apply_kernel<true> ---------------------------------------------
# training mode (the statistics-and-extremes pass); L = 4096 + 640: a ragged second segment; a batch of 3; gamma of both
# signs (arg-max and arg-min rows), the index output through the C ABI
@pytest.mark.parametrize("shape,act", [((3, 16, 4096 + 640), ("leaky", 0.2)), ((6, 128, 2048), "relu")],
                         ids=["leaky-3x16x4736", "relu-6x128x2048"])
def test_bn_max_forward_and_backward(gpu, use, libs, shape, act):
    from fpsg_amd import _hip
    from fpsg_amd.fused_bn import _BNActMax, _parse_act
    N, C, L = shape
    code, slope = _parse_act(act)

    def produce():
        lib = _hip.load()
        torch.manual_seed(sum(shape) + 7)
        gamma, beta = _affine(C, gpu, both_signs=True)
        x = torch.randn(N, C, L, device=gpu).requires_grad_()
        pb = (torch.randn(C, device=gpu) * 0.3).requires_grad_()
        rm, rv = torch.zeros(C, device=gpu), torch.ones(C, device=gpu)
        out = _BNActMax.apply(x, gamma, beta, rm, rv, True, 1e-5, code, slope, pb, 0.1)
        out.backward(torch.randn_like(out))
        # the same forward through the C ABI: its index, coefficient and batch-statistics outputs
        o2, idx = torch.empty(N, C, device=gpu), torch.empty(N, C, dtype=torch.int32, device=gpu)
        chan, bm, bv = torch.empty(4, C, device=gpu), torch.empty(C, device=gpu), torch.empty(C, device=gpu)
        ws = torch.empty(lib.fpsg_bn_max_workspace_floats(N, C, L), device=gpu)
        p = _hip.ptr
        rc = lib.fpsg_bn_act_max_fwd(p(x), p(pb), p(gamma), p(beta), None, None, -1.0, N, C, L, 1, 1e-5, code, slope, p(o2),
                                     p(idx), p(chan), p(bm), p(bv), p(ws), _hip.stream_of(x))
        _hip.check(rc, "fpsg_bn_act_max_fwd")
        assert torch.equal(o2, out.detach())
        return dict(out=out.detach(), idx=idx, chan=chan, batch_mean=bm, batch_var=bv, dx=x.grad, dpre_bias=pb.grad,
                    dgamma=gamma.grad, dbeta=beta.grad, running_mean=rm, running_var=rv)

    got = _both(use, produce)["stream"]
    # the index output against the definition: the arg-max of x + pre_bias where gamma >= 0, the arg-min where gamma < 0
    # (continuous random values: the extreme of a row is unique)
    torch.manual_seed(sum(shape) + 7)
    gamma, _ = _affine(C, gpu, both_signs=True)
    x = torch.randn(N, C, L, device=gpu)
    xb = x + (torch.randn(C, device=gpu) * 0.3).view(1, C, 1)
    want = torch.where(gamma.detach().view(1, C) >= 0, xb.argmax(dim=2), xb.argmin(dim=2))
    assert torch.equal(got["idx"].long(), want)
    use("stream")
    bnact_tests.test_max_variant_matches_unfused_chain(gpu, shape, act, "train")
    if shape[1] == 16:
        bnact_tests.test_max_variant_selected_index(gpu)


# ---- bnact.hip: bn_pool_apply_kernel<0 | 2, 1, 2, true>, bn_pool_reduce_kernel<1, 2, true> ---------------------------
# W % 4 == 0 and ReLU; N H W > 16384; 37 images of 28 x 28: 7 vectors a pooled row, a plane of one partly filled item
@pytest.mark.parametrize("shape,mode", [((37, 16, 28, 28), "train"), ((37, 16, 28, 28), "eval"), ((8, 64, 56, 56), "train")],
                         ids=["37x16x28x28-train", "37x16x28x28-eval", "8x64x56x56-train"])
def test_bn_pooled_forward_and_backward(gpu, use, shape, mode):
    from fpsg_amd.fused_bn import _BNActPool
    N, C, H, W = shape
    assert W % 4 == 0 and N * H * W > 16384

    def produce():
        torch.manual_seed(sum(shape))
        gamma, beta = _affine(C, gpu)
        x = torch.randn(N, C, H, W, device=gpu).requires_grad_()
        pb = (torch.randn(C, device=gpu) * 0.3).requires_grad_()
        rm, rv = torch.randn(C, device=gpu) * 0.2, torch.rand(C, device=gpu) + 0.5
        yp = _BNActPool.apply(x, gamma, beta, rm, rv, mode == "train", 1e-5, 1, 0.0, pb, 0.1)
        yp.backward(torch.randn_like(yp))
        return dict(y_pooled=yp.detach(), dx=x.grad, dpre_bias=pb.grad, dgamma=gamma.grad, dbeta=beta.grad,
                    running_mean=rm, running_var=rv)

    _both(use, produce)
    use("stream")
    bnact_tests.test_pooled_variant_matches_unfused_chain(gpu, shape, mode)


# ---- winograd_fused.hip: wino4_fused_c64_kernel<false, true, true>, <true, false, true>, <true, true, true> ----------
# 64 input channels; with parts (_fused_stats) and without (_fused, _fused_act); 28 x 36 planes and the 4 x 4 minimum
@pytest.mark.parametrize("shape", [(2, 64, 128, 28, 36), (1, 64, 16, 4, 4), (37, 64, 32, 56, 56)],
                         ids=["2x64x128x28x36", "1x64x16x4x4", "37x64x32x56x56"])
@pytest.mark.parametrize("act", [False, True], ids=["plain", "activated"])
def test_fused_winograd_convolution(gpu, use, shape, act):
    from fpsg_amd import winograd as wg
    N, C, K, H, W = shape

    def produce():
        torch.manual_seed(K + H)
        x = torch.randn(N, C, H, W, device=gpu)
        U = wg._filter(4, torch.randn(K, C, 3, 3, device=gpu) * 0.05, False)
        ob = torch.randn(K, device=gpu)
        chan = torch.randn(4, C, device=gpu) * 0.5 + 1.0 if act else None
        pb = torch.randn(C, device=gpu) * 0.1 if act else None
        y = wg._fused_act(x, chan, pb, U) if act else wg._fused(x, U)
        ys, parts = wg._fused_stats(x, chan, pb, U, ob)
        yn, parts_nobias = wg._fused_stats(x, chan, pb, U, None)
        return dict(y=y, y_with_stats=ys, parts=parts, y_with_stats_nobias=yn, parts_nobias=parts_nobias)

    _both(use, produce)
    use("stream")
    wino_tests.test_fused_kernel_delivers_batchnorm_partial_sums(gpu, shape, act)


@pytest.mark.parametrize("shape", [(2, 64, 128, 28, 36), (1, 64, 64, 4, 4)], ids=["2x64x128x28x36", "1x64x64x4x4"])
def test_fused_winograd_convolution_against_the_three_kernel_form_and_float64(gpu, use, monkeypatch, shape):
    """conv3x3 with 64 input channels, forward and gradients, fused (<false, false, true>; the data gradient takes it
    again where the output has 64 channels) and as transform + GEMM + transform (the streaming transforms), against
    each other and float64."""
    use("stream")
    wino_tests.test_fused_kernel_matches_three_kernel_form(gpu, shape, monkeypatch)


# ---- winograd.hip: wino_input_kernel<4, true, true>, wino_output_kernel<4, true, false | true, true>,
#      wino_grad_output_kernel<4, true> --------------------------------------------------------------------------------
# m = 4 and whole tiles; 37 images of 28 x 28: 1813 tiles, a last workgroup of 21 of 256 lanes, rows padded to 1824
def test_winograd_activated_input_transform(gpu, use, monkeypatch):
    from fpsg_amd import winograd as wg
    N, C, H, W = 37, 40, 28, 28

    def produce():
        torch.manual_seed(C + H)
        x = torch.randn(N, C, H, W, device=gpu)
        chan = torch.randn(4, C, device=gpu) * 0.5 + 1.0
        pb = torch.randn(C, device=gpu) * 0.1
        V = wg._input_act(4, x, chan, pb)
        # a consistency check inside one build (under the second build ``_input`` is itself the streaming plain
        # transform): the plain transform of relu((x + pre_bias) scale + shift).  The independent reference of this
        # row is the sibling test below
        z = torch.relu(torch.addcmul(chan[1].view(1, C, 1, 1), x + pb.view(1, C, 1, 1), chan[0].view(1, C, 1, 1)))
        return dict(V=V, V_of_activated=wg._input(4, z))

    out = _both(use, produce)["stream"]
    # torch's addcmul may round the activation's product where the kernel's fma does not: one ulp (6e-8) of an
    # activation, through B^T d B whose rows sum to at most 10 in absolute value: 100 x 6e-8 of the largest activation,
    # below 1e-5 of the largest transformed value
    scale = float(out["V_of_activated"].abs().max())
    assert float((out["V"] - out["V_of_activated"]).abs().max()) <= 1e-5 * scale
    use("stream")
    wino_tests.test_bn_relu_folded_into_next_conv_equals_two_ops(gpu, monkeypatch, 128, 128, 56, 6, "train")


@pytest.mark.parametrize("shape", [(37, 32, 28, 28), (3, 8, 12, 20)], ids=["37x32x28x28", "3x8x12x20"])
def test_winograd_output_transform_with_statistics(gpu, use, shape):
    from fpsg_amd import winograd as wg
    N, K, H, W = shape

    def produce():
        torch.manual_seed(H + K)
        P = N * (H // 4) * (W // 4)
        Mt = torch.randn(36, K, P, device=gpu)
        b = torch.randn(K, device=gpu)
        y0 = wg._output(4, Mt, N, H, W)
        y1, parts = wg._output(4, Mt, N, H, W, b, True)
        y2, parts_nobias = wg._output(4, Mt, N, H, W, None, True)
        return dict(y=y0, y_with_stats=y1, parts=parts, y_with_stats_nobias=y2, parts_nobias=parts_nobias)

    _both(use, produce)
    use("stream")
    wino_tests.test_output_transform_delivers_batchnorm_partial_sums(gpu, 4, shape)


@pytest.mark.parametrize("shape", [(37, 32, 28, 28), (3, 7, 8, 12)], ids=["37x32x28x28", "3x7x8x12"])
def test_winograd_output_transform_with_backward_sums(gpu, use, shape):
    from fpsg_amd import winograd as wg
    N, K, H, W = shape

    def produce():
        torch.manual_seed(H + K)
        P = N * (H // 4) * (W // 4)
        M = torch.randn(36, K, P, device=gpu)
        xpre = torch.randn(N, K, H, W, device=gpu)
        pb = torch.randn(K, device=gpu) * 0.1
        chan = torch.stack([torch.randn(K, device=gpu) * 0.5 + 1, torch.randn(K, device=gpu) * 0.3,
                            torch.randn(K, device=gpu) * 0.1, torch.rand(K, device=gpu) + 0.5]).contiguous()
        y, parts = wg._output_bwd_stats(4, M, N, H, W, xpre, pb, chan)
        return dict(y=y, parts=parts)

    _both(use, produce)
    use("stream")
    wino_tests.test_output_transform_delivers_batchnorm_backward_sums(gpu, 4, shape)


@pytest.mark.parametrize("shape", [(37, 40, 28, 28), (1, 3, 4, 4)], ids=["37x40x28x28", "1x3x4x4"])
def test_winograd_gradient_transforms(gpu, use, monkeypatch, shape):
    """wino_grad_output_kernel<4, true> (A g A^T) beside the one-pass pair of both transforms, and conv3x3's gradients
    through them against float64."""
    import torch.nn.functional as F
    from fpsg_amd import winograd as wg
    N, K, H, W = shape

    def produce():
        torch.manual_seed(K + H)
        gy = torch.randn(*shape, device=gpu)
        V, dM = wg._grad_transforms(4, gy)
        return dict(dM=wg._grad_output(4, gy), V=wg._input(4, gy), V_one_pass=V, dM_one_pass=dM)

    out = _both(use, produce)["stream"]
    # A g A^T against float64: the tile (n, th, tw) of channel k, A = [[1,0,0,0],[1,1,1,1],[1,-1,1,-1],[1,2,4,8],[1,-2,4,-8],[0,0,0,1]]
    torch.manual_seed(K + H)
    gy = torch.randn(*shape, device=gpu).double().cpu()
    A = torch.tensor([[1, 0, 0, 0], [1, 1, 1, 1], [1, -1, 1, -1], [1, 2, 4, 8], [1, -2, 4, -8], [0, 0, 0, 1]], dtype=torch.float64)
    tiles = gy.view(N, K, H // 4, 4, W // 4, 4).permute(1, 0, 2, 4, 3, 5).reshape(K, -1, 4, 4)      # [K, P, 4, 4]
    want = torch.einsum("ia,kpab,jb->ijkp", A, tiles, A).reshape(36, K, -1)
    # every element is a sum of 16 terms formed in two passes of at most 4 roundings each (sums and fmas with exact
    # power-of-two coefficients): each term carries at most (1 + 2^-24)^8, so |error| <= 8 x 2^-24 x sum |terms|
    bound = 8 * 2.0 ** -24 * torch.einsum("ia,kpab,jb->ijkp", A.abs(), tiles.abs(), A.abs()).reshape(36, K, -1)
    P = want.shape[2]
    got = out["dM"].double().cpu()
    assert bool(((got[:, :, :P] - want).abs() <= bound).all()) and not got[:, :, P:].any()
    use("stream")
    wino_tests.test_both_transforms_of_an_output_gradient_from_one_pass(gpu, 4, shape, monkeypatch)


# ---- conv_first.hip: conv_first_fwd_kernel<true, true> (parts), <false, true> (no parts) -----------------------------
# 30 x 36: W no multiple of the 64-pixel row segment; 37 images of 56 x 100: a ragged segment in every row
@pytest.mark.parametrize("shape", [(3, 30, 36), (37, 56, 100)], ids=["3x30x36", "37x56x100"])
def test_first_layer_forward(gpu, use, shape):
    from fpsg_amd.conv_first import _forward
    N, H, W = shape

    def produce():
        torch.manual_seed(H * 7 + W)
        x = torch.randn(N, 3, H, W, device=gpu)
        w = torch.randn(64, 3, 3, 3, device=gpu) * 0.2
        b = torch.randn(64, device=gpu)
        y, none = _forward(x, w)
        y2, parts = _forward(x, w, b, True)
        assert none is None
        return dict(y=y, y_with_stats=y2, parts=parts)

    _both(use, produce)
    use("stream")
    wino_tests.test_first_layer_forward_and_its_batchnorm_partial_sums(gpu, shape)


# ---- decoder.hip: dec1_fwd_kernel<true>, dec1_bwd_kernel<true> -------------------------------------------------------
# through the C ABI in NaN frames (tests/test_dec1_gpu.py): idle lanes and a last tile of 6 channels; a partial second
# block in evaluation mode; B > 64; the contiguous entries; accumulate = 1
@pytest.mark.parametrize("name,seed", [("g2d70b7p32-train", 0), ("g1d33b3p128-eval", 1), ("g2d40b130p4-train", 1),
                                       ("g1d96b16p128-train", 2), ("g2d70b7p32-train-accumulate", 0)])
def test_decoder_first_layer(gpu, libs, name, seed):
    shipped, stream = libs
    c = R.case(name, seed)
    a, b = dec1_tests._run(c, shipped, gpu), dec1_tests._run(c, stream, gpu)
    assert a.keys() == b.keys()
    for key in a:
        assert (a[key] == b[key]).all(), f"'{key}': the streaming form differs from its cached sibling"
    dec1_tests.test_k9_against_float64(gpu, stream, name, seed)


# ---- the guarded-buffer rows on the second build ---------------------------------------------------------------------
# every entry of the table that can select a streaming form: K5's (bnact.hip); the table has no row of a Winograd
# transform, of fpsg_conv_first_fwd or of K9 (they take no workspace)
GUARDED = [c for c in T.CASES if c[1].startswith("fpsg_bn_")]


def _takes_vector_streaming_accesses(case):
    """The row's call executes v4f accesses that carry the hint on the second build: a sliced shape (N L > 16384) of whole
    vectors (L % 4 == 0), or a pooled shape with W % 4 == 0 (the builders' activation is ReLU).  Every other K5 row
    launches at most the scalar branch of a streaming instantiation, which is the cached form's text, or a kernel
    without a streaming form (the one-launch kernel, W % 4 != 0)."""
    entry, args = case[1], case[3]
    if "pool" in entry:
        return args[3] % 4 == 0
    N, C, L = args[:3]
    return N * L > 16384 and L % 4 == 0 and entry != "fpsg_bn_act_max_bwd_coef"


@pytest.mark.parametrize("case", GUARDED, ids=[c[0] for c in GUARDED])
def test_memory_contract_of_the_streaming_forms(gpu, libs, case):
    """The five runs of tests/test_memory_contract_gpu.py on the second build: guards and inputs intact, every output
    element written and bit-identical across fills, layouts and repeats -- and bit-identical to the shipped library's.
    Where the row takes vector accesses (``_takes_vector_streaming_accesses``: the ``vec`` rows of the table) this is
    the check of the vector non-temporal stores: one that left a tail element out would differ between the 0xFF and
    the zero fill, one that went past the buffer would break a guard.  The other rows check the second build's launches
    of the scalar branches and of the kernels without a streaming form."""
    import _guarded as G
    shipped, stream = libs
    got = T.five_runs(case, stream, gpu)
    row = T.build(case, shipped)
    want = T.run_once(row, G.Arena(row.bufs, G.PATTERNS[0], gpu, seed=17), 1, shipped)
    sizes = {b.name: torch.empty((), dtype=b.dtype).element_size() for b in row.bufs}
    assert got.keys() == want.keys()
    for buf in want:
        at = G.first_difference(want[buf], got[buf], sizes[buf])
        assert at is None, f"output '{buf}': the streaming form differs from its cached sibling, first at element {at}"


def test_guarded_rows_cover_the_entries_that_stream():
    streaming = {"fpsg_bn_act_fwd", "fpsg_bn_stats", "fpsg_bn_act_bwd", "fpsg_bn_act_bwd_coef", "fpsg_bn_act_bwd_parts",
                 "fpsg_bn_act_pool_fwd", "fpsg_bn_act_pool_bwd", "fpsg_bn_act_max_fwd", "fpsg_bn_act_max_bwd"}
    assert {c[1] for c in GUARDED} >= streaming
    vector = [c for c in GUARDED if _takes_vector_streaming_accesses(c)]
    for entry in streaming:     # two shapes each that execute the hinted vector accesses, a ragged last vector among them
        assert sum(c[1] == entry for c in vector) >= 2, entry
    assert {c[4].get("act", 1) for c in vector if c[1] == "fpsg_bn_act_bwd_parts"} == {0, 1, 2}
    assert not [c[1] for c in T.CASES if c[1].startswith(("fpsg_wino_input", "fpsg_wino_output", "fpsg_wino_grad",
                                                         "fpsg_wino_conv_fused", "fpsg_conv_first_fwd", "fpsg_dec1"))]


# ---- one training episode with the streaming forms chained -----------------------------------------------------------
class _Counting:
    """The streaming handle, counting the entries called through it."""

    def __init__(self, lib):
        self._lib, self.calls = lib, {}

    def __getattr__(self, name):
        self.calls[name] = self.calls.get(name, 0) + 1
        return getattr(self._lib, name)


def test_training_episode(gpu, libs, monkeypatch):
    """A 1-shot episode of the PointNet path (the model and options of smoke(); 1 support + 1 query item, clouds of 1024
    points, 96 x 96 images): every loss, the gradient of every parameter and every running statistic after the
    forward + backward.  The shipped library runs it twice; what reproduces bit for bit there must be bit-identical
    under the streaming library, producer to consumer on one stream through the Python wrappers.  Left out: nothing --
    with the generator seeded in front of every run (the decoder draws its template points in the forward) all 508
    tensors reproduce under the shipped library on the MI355X; that is asserted, so all 508 are compared."""
    from fpsg_amd import _hip
    from fpsg_amd.engine import build_model, default_options
    from fpsg_amd.episodes import synthetic_episode
    shipped, stream = libs
    torch.manual_seed(0)
    base = build_model(default_options(device="cuda", intra_recon=True)).to(gpu).train()
    ep = synthetic_episode(1, 1, n_pts=1024, img_size=96, seed=7, device=gpu)

    def run(lib):
        monkeypatch.setattr(_hip, "_lib", lib)
        torch.manual_seed(1)
        model = copy.deepcopy(base)
        out = model.loss({k: (v.clone() if torch.is_tensor(v) else v) for k, v in ep.items()})
        total = out["ttl_loss"]
        (total if total.dim() == 0 else total.sum()).backward()
        res = {f"loss:{k}": v.detach().clone() for k, v in out.items() if torch.is_tensor(v)}
        for name, p in model.named_parameters():
            if p.grad is not None:
                res[f"grad:{name}"] = p.grad.detach().clone()
        for name, b in model.named_buffers():
            if "running" in name:
                res[f"buffer:{name}"] = b.detach().clone()
        torch.cuda.synchronize()
        return res

    first, second = run(shipped), run(shipped)
    counting = _Counting(stream)
    third = run(counting)
    # the episode went through the second build, and through entries of each family that chooses a streaming form
    called = counting.calls
    print(f"training episode: entries called through the streaming library: {dict(sorted(called.items()))}")
    for family in ("fpsg_bn_act", "fpsg_dec1", ("fpsg_conv_first_fwd", "fpsg_wino_")):
        assert any(name.startswith(family) for name in called), (family, sorted(called))
    assert first.keys() == second.keys() == third.keys() and any(k.startswith("grad:") for k in first)
    stable = [k for k in first if torch.equal(first[k], second[k])]
    unstable = sorted(set(first) - set(stable))
    print(f"training episode: {len(stable)} of {len(first)} tensors reproduce under the shipped library; not reproducible: "
          f"{unstable[:40]}{' ...' if len(unstable) > 40 else ''}")
    assert not unstable, f"no longer reproducible under the shipped library itself: {unstable[:40]}"
    for k in first:
        assert bool(torch.isfinite(third[k].float()).all()), k
    differing = [k for k in stable if not torch.equal(first[k], third[k])]
    assert not differing, f"reproducible under the shipped library, different under the streaming one: {differing}"
