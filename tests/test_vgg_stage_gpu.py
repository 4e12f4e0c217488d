"""A VGG stage (``conv -> BN -> ReLU -> conv -> BN -> ReLU -> pool``; torchvision ``vgg16_bn.features`` as built at reference
``src/models/image_net.py:14``) through ``ImageEncoderWarpper.forward`` with every default fusion on TOGETHER, against the
literal ``nn.Sequential`` in float64: pooled output, input gradient, every parameter's gradient and both BatchNorms'
running statistics at fp32 round-off.  The other trunk tests compare the fused forms with each other; here every case --
the default environment in both modes, one switch off at a time, the split-operand products -- goes against float64 with
one bound, none against another case.

The inputs are the kink-free stages of ``tests/_vgg_stage_ref.py`` (no ReLU mask and no pool selection can differ between
fp32 and float64; ``tests/test_vgg_stage_cpu.py`` asserts the conditions), at the smallest shapes at which the fused forms
switch on (more than 16384 values per channel).  Bound per tensor: 4 x the worse of two fp32 yardsticks outside the code
under test (torch's own modules; F(4x4,3x3) in plain torch ops) + 2e-6, and never more than 1e-4; a convolution bias in
front of a training-mode BatchNorm (true gradient exactly cancelled) is bounded by 10 x the yardsticks' own round-off
+ 2e-6 of the gradient of the BatchNorm shift behind it.  No number measured on the project's kernels enters a bound.

Every case runs twice, each time inside a ``winograd.weights_frozen()`` block as a training step does, and the second run
is compared: it takes its transformed filters from the filter bank's one launch.  Every case also asserts which forms it
took, by counting calls -- a case that silently fell back to another form would test nothing.  ``stemw`` is the stem at
64 x 64 with ``winograd.MIN_DW_TILES`` (a speed threshold: below it K6w is slower, not wrong) lowered so that K6w serves
conv1_2's weight gradient.  (The issue's table lists K6w under ``stem``; at 56 x 56 K6w's width rule -- multiples of 16 --
keeps it out whatever the threshold, so ``stem`` asserts k6w = 0 and ``stemw`` carries K6w, in the stem function, plain
under ``FPSG_BN_FOLD=0`` and from the fold under ``FPSG_STEM_FOLD=0``.)

Measured deviations: ``profiles/vgg_stage/deviation.jsonl``.

Found by this test: under ``FPSG_GEMM_SPLIT=1`` the gradient of BN1's shift (a sum over 18816 pixels of conv2's masked data
gradient) missed its bound at s2 (1.27e-5 against 8.8e-6; default path 2.4e-6): every element of a K10 product was biased
towards -inf by 1e-8 of the product's rms, below every per-element bound but coherent in sums over a row of the product
(``profiles/vgg_stage/gemm_split_bias.txt``).  K10 now sums the low-order pieces from zero (``split_step`` in
``csrc/gemm_split.hip``): 5.3e-6."""
import collections
import inspect
import json

import pytest
import torch
import torch.nn as nn

import _vgg_stage_ref as R

pytestmark = pytest.mark.gpu

K6F = ("fpsg_wino_conv_fused", "fpsg_wino_conv_fused_act", "fpsg_wino_conv_fused_stats")

# What a stage takes in the default environment: calls during one forward + backward.  stem: _StemConvBNReluConv; fold:
# _BNReluConv3x3; fused_stats: K6f with the statistics epilogue; out_parts: _output(..., want_parts=True); bwd_stats:
# _output_bwd_stats; pool / pool_parts: the pooled K5 pass (given the convolution's partial sums); k6f / k6w: launches of
# K6f (any form) / K6w; k8f: K8f forwards; k8fold: K8 with the folded BatchNorm backward; gt: fpsg_wino_grad_transforms;
# split: K10 products; bank / filt: batched / single filter-transform launches.
_ZERO = dict(stem=0, fold=0, fused_stats=0, out_parts=0, bwd_stats=0, pool=1, pool_parts=0, k6f=0, k6w=0, k8f=0, k8fold=0,
             gt=0, split=0, bank=1, filt=0)
DEFAULT = {
    ("stem", "train"): dict(_ZERO, stem=1, fused_stats=1, pool_parts=1, k6f=2, k8f=1, k8fold=1),
    ("stem", "eval"): dict(_ZERO, fold=1, k6f=2, k8f=1),
    ("stemw", "train"): dict(_ZERO, stem=1, fused_stats=1, pool_parts=1, k6f=2, k6w=1, k8f=1, k8fold=1),
    ("s2", "train"): dict(_ZERO, fold=1, fused_stats=1, out_parts=1, bwd_stats=1, pool_parts=1, k6f=1, gt=2),
    ("s2", "eval"): dict(_ZERO, fold=1, bwd_stats=1, k6f=1, gt=2),
    ("s3", "train"): dict(_ZERO, fold=1, out_parts=2, bwd_stats=1, pool_parts=1, gt=2),
    ("s3", "eval"): dict(_ZERO, fold=1, bwd_stats=1, gt=2),
    ("s5", "train"): dict(_ZERO, fold=1, out_parts=2, bwd_stats=1, pool_parts=1, gt=2),
    ("s5", "eval"): dict(_ZERO, fold=1, bwd_stats=1, gt=2),
}
_FILTERS = {"stem": 2, "stemw": 2, "s2": 4, "s3": 4, "s5": 4}      # transformed filters of a stage (conv1_1 has none)

# (stage, mode, switch, what changes against DEFAULT)
CASES = [(n, m, None, {}) for (n, m) in DEFAULT] + [
    ("stem", "train", "FPSG_BN_FOLD=0", dict(stem=0, k8fold=0)),                   # K8f + K5, then conv1_2 as a plain K6f
    ("stemw", "train", "FPSG_BN_FOLD=0", dict(stem=0, k8fold=0)),                  # ... whose weight gradient is the plain K6w
    ("s2", "train", "FPSG_BN_FOLD=0", dict(fold=0, bwd_stats=0)),
    ("s3", "train", "FPSG_BN_FOLD=0", dict(fold=0, bwd_stats=0)),
    ("stem", "train", "FPSG_CONV_STATS=0", dict(stem=0, k8fold=0, fold=1, fused_stats=0, pool_parts=0)),
    ("s2", "train", "FPSG_CONV_STATS=0", dict(fused_stats=0, out_parts=0, pool_parts=0)),
    ("s3", "train", "FPSG_CONV_STATS=0", dict(out_parts=0, pool_parts=0)),
    ("s2", "train", "FPSG_CONV_BWD_STATS=0", dict(bwd_stats=0)),
    ("s3", "train", "FPSG_CONV_BWD_STATS=0", dict(bwd_stats=0)),
    ("s5", "train", "FPSG_CONV_BWD_STATS=0", dict(bwd_stats=0)),
    ("stem", "train", "FPSG_STEM_FOLD=0", dict(stem=0, k8fold=0, fold=1)),
    ("stemw", "train", "FPSG_STEM_FOLD=0", dict(stem=0, k8fold=0, fold=1)),        # K6w with the activating load, from the fold
    ("stem", "train", "FPSG_WINOGRAD_FUSED=0", dict(fused_stats=0, out_parts=1, k6f=0)),
    ("s2", "train", "FPSG_WINOGRAD_FUSED=0", dict(fused_stats=0, out_parts=2, k6f=0)),
    ("stemw", "train", "FPSG_WINOGRAD_DW=0", dict(k6w=0)),
    ("s2", "train", "FPSG_GRAD_TRANSFORMS=0", dict(gt=0)),
    ("s3", "train", "FPSG_GRAD_TRANSFORMS=0", dict(gt=0)),
    ("s5", "train", "FPSG_GRAD_TRANSFORMS=0", dict(gt=0)),
    ("s2", "train", "FPSG_FILTER_BANK=0", dict(bank=0, filt=4)),
    ("s3", "train", "FPSG_FILTER_BANK=0", dict(bank=0, filt=4)),
    ("s2", "train", "FPSG_GEMM_SPLIT=1", dict(split=3)),                           # conv2_2's three products (conv2_1 has 64 inputs)
    ("s3", "train", "FPSG_GEMM_SPLIT=1", dict(split=6)),
]


def _count_calls(monkeypatch):
    from fpsg_amd import conv_first, fused_bn, gemm_split, winograd
    n = collections.Counter()

    def function(cls, key):
        orig = cls.forward

        def counted(*a, **k):
            n[key] += 1
            return orig(*a, **k)

        monkeypatch.setattr(cls, "forward", staticmethod(counted))

    function(winograd._StemConvBNReluConv, "stem")
    function(winograd._BNReluConv3x3, "fold")
    orig_pool = fused_bn._BNActPool.forward
    pool_signature = inspect.signature(orig_pool)

    def pool(*a, **k):
        n["pool"] += 1
        n["pool_parts"] += 1 if pool_signature.bind(*a, **k).arguments.get("parts") is not None else 0
        return orig_pool(*a, **k)

    monkeypatch.setattr(fused_bn._BNActPool, "forward", staticmethod(pool))
    orig_out, orig_fused, orig_bwd = winograd._output, winograd._fused_stats, winograd._output_bwd_stats
    orig_call, orig_split, orig_first = winograd._call, gemm_split.bmm_split, conv_first._forward

    def out(m, M, N, H, W, stats_bias=None, want_parts=False):
        n["out_parts"] += 1 if want_parts else 0
        return orig_out(m, M, N, H, W, stats_bias, want_parts)

    def fused(*a):
        n["fused_stats"] += 1
        return orig_fused(*a)

    def bwd(*a):
        n["bwd_stats"] += 1
        return orig_bwd(*a)

    def call(name, *a):
        n[name] += 1
        return orig_call(name, *a)

    def split(*a, **k):
        n["split"] += 1
        return orig_split(*a, **k)

    def first(*a, **k):
        n["k8f"] += 1
        return orig_first(*a, **k)

    monkeypatch.setattr(winograd, "_output", out)
    monkeypatch.setattr(winograd, "_fused_stats", fused)
    monkeypatch.setattr(winograd, "_output_bwd_stats", bwd)
    monkeypatch.setattr(winograd, "_call", call)
    monkeypatch.setattr(gemm_split, "bmm_split", split)
    monkeypatch.setattr(conv_first, "_forward", first)
    return n


def _taken(n):
    return dict(stem=n["stem"], fold=n["fold"], fused_stats=n["fused_stats"], out_parts=n["out_parts"],
                bwd_stats=n["bwd_stats"], pool=n["pool"], pool_parts=n["pool_parts"], k6f=sum(n[k] for k in K6F),
                k6w=n["fpsg_wino_dw_fused"], k8f=n["k8f"], k8fold=n["fpsg_conv_first_dw_fold"],
                gt=n["fpsg_wino_grad_transforms"], split=n["split"], bank=n["fpsg_wino_filter_transform_batch"],
                filt=n["fpsg_wino_filter_transform"])


def _encoder(seq):
    """An ``ImageEncoderWarpper`` whose trunk is the stage and whose pool is the identity (built without the 15 M
    parameter VGG16-BN trunk its constructor would initialise only to have it replaced); a fresh one per case."""
    from fpsg_amd.image_net import ImageEncoderWarpper
    enc = ImageEncoderWarpper.__new__(ImageEncoderWarpper)
    nn.Module.__init__(enc)
    enc.finetune_layer = 0
    enc.img_feature_extractor, enc.img_feature_pool = seq, nn.Identity()
    return enc


def _run_project_path(gpu, monkeypatch, tr, name):
    """``ImageEncoderWarpper.forward`` on the stage: two runs, each in its own ``weights_frozen`` block; -> the second
    run's tensors (named as ``_vgg_stage_ref.run_chain`` names them) and the calls it made."""
    from fpsg_amd import winograd
    p, train = tr.p, tr.mode == "train"
    seq = R.make_stage(p, tr.params, running=tr.running).to(gpu)
    enc = _encoder(seq)
    enc.train(train)
    if name == "stemw":
        monkeypatch.setattr(winograd, "MIN_DW_TILES", 1024)
    n = _count_calls(monkeypatch)
    g = tr.g.to(gpu)
    winograd._bank.__init__()
    try:
        for _ in range(2):
            for prm in seq.parameters():
                prm.grad = None
            if train:
                seq[1].reset_running_stats()
                seq[4].reset_running_stats()
            n.clear()
            x = tr.x.to(gpu).requires_grad_(tr.need_dx)
            with winograd.weights_frozen():
                out = enc(x).view(p.N, p.C2, p.H // 2, p.W // 2)
                out.backward(g)
        torch.cuda.synchronize()
    finally:
        winograd._bank.__init__()
    got = {"out": out.detach()}
    if tr.need_dx:
        got["dx"] = x.grad
    for k, prm in seq.named_parameters():
        got["d " + k] = prm.grad
    for k, b in seq.named_buffers():
        got[k] = b.detach().clone()
    return got, _taken(n)


@pytest.mark.parametrize("name,mode,switch,change", CASES,
                         ids=[f"{n}-{m}-{s or 'default'}" for n, m, s, _ in CASES])
def test_stage_against_float64(gpu, monkeypatch, name, mode, switch, change):
    tr = R.truth(name, mode)
    if switch:
        monkeypatch.setenv(*switch.split("="))
    got, taken = _run_project_path(gpu, monkeypatch, tr, name)
    expect = dict(DEFAULT[(name, mode)], **change)
    if switch and switch.startswith("FPSG_FILTER_BANK"):
        assert expect["filt"] == _FILTERS[name]
    assert set(got) == set(tr.t64)
    record, bad = {"stage": name, "mode": mode, "switch": switch or "default", "deviation": {}}, []
    for k in sorted(tr.t64):
        if k.endswith("num_batches_tracked"):
            if int(got[k]) != int(tr.t64[k]):
                bad.append((k, int(got[k]), int(tr.t64[k])))
            continue
        if R.cancelled(k, mode):
            v, lim = float(got[k].abs().max()), R.cancelled_bound(tr, k)
            record["deviation"][k] = {"max_abs_ours": v, "max_abs_lib": float(tr.lib[k].abs().max()),
                                      "max_abs_wino": float(tr.wino[k].abs().max()), "allowed": lim}
            print(f"{name}/{mode}/{switch} {k}: cancelled, max|ours| {v:.3g}  lib {float(tr.lib[k].abs().max()):.3g}  "
                  f"wino {float(tr.wino[k].abs().max()):.3g}  allowed {lim:.3g}")
            if v > lim:
                bad.append((k, v, lim))
            continue
        d = R.deviation(got[k], tr.t64[k])
        dl, dw, lim = R.deviation(tr.lib[k], tr.t64[k]), R.deviation(tr.wino[k], tr.t64[k]), R.bound(tr, k)
        record["deviation"][k] = {"ours": d, "lib": dl, "wino": dw, "bound": lim}
        print(f"{name}/{mode}/{switch} {k}: ours {d:.3g}  lib {dl:.3g}  wino {dw:.3g}  bound {lim:.3g}")
        if not d <= lim:
            bad.append((k, d, lim))
    print("DEVIATION " + json.dumps(record))
    print(f"{name}/{mode}/{switch} forms taken: {taken}")
    assert taken == expect, {k: (taken[k], expect[k]) for k in expect if taken[k] != expect[k]}
    assert not bad, bad
