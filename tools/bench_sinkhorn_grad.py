"""K19 (fpsg_sinkhorn_divergence_grad) against the forward-only call, and what ``--pc_dist sinkhorn`` costs an episode.
On the GPU box:

    python tools/bench_sinkhorn_grad.py kernel [rounds]       # the three calls per configuration, alternating
    python tools/bench_sinkhorn_grad.py train [steps] [rounds]  # episodes/s of the training step, cd / sinkhorn

``kernel``: at B = 5 and 37 with N = M = 2048, and at B = 64 with N = M = 512, unit-ball clouds against tanh(0.4 randn)
clouds and the training schedule (diameter 2 sqrt(3), blur 0.05; its length is printed), it times
``fpsg_sinkhorn_divergence``, ``fpsg_sinkhorn_divergence_grad`` with both gradients and with gx alone -- whole calls,
CALLS back to back between two HIP events after WARM warm-ups, the three forms alternating within every round, in one
process.  It also reports the largest deviation of the gradients from the float64 reference of
``tests/_sinkhorn_grad_ref.py`` at B = 2, N = M = 512.  ``train`` is bench.py's c3 workload (32-shot 5-query,
``--intra_recon``, one episode per step, replayed as a graph) with ``pc_dist="cd"`` -- the parent's code path, which
this change does not touch -- against ``pc_dist="sinkhorn"``."""
import ctypes
import json
import math
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CONFIGS = [(5, 2048), (37, 2048), (64, 512)]                  # (B, N = M)
WARM, CALLS = 5, 30
DIAMETER, BLUR = 2.0 * math.sqrt(3.0), 0.05


def _clouds(B, N, dev, seed):
    g = torch.Generator().manual_seed(seed)
    v = torch.randn(B, N, 3, generator=g)
    x = v / v.norm(dim=-1, keepdim=True) * torch.rand(B, N, 1, generator=g) ** (1.0 / 3.0)
    y = torch.tanh(0.4 * torch.randn(B, N, 3, generator=g))
    return x.to(dev).contiguous(), y.to(dev).contiguous()


def kernel(rounds):
    from fpsg_amd import _hip
    from fpsg_amd.metrics import sinkhorn_epsilons, sinkhorn_loss
    dev = torch.device("cuda:0")
    lib = _hip.load()
    eps_s = sinkhorn_epsilons(DIAMETER, BLUR, 0.5)
    eps = (ctypes.c_float * len(eps_s))(*eps_s)
    res = {}
    for B, N in CONFIGS:
        x, y = _clouds(B, N, dev, B + N)
        out = torch.empty((B,), device=dev)
        gx, gy = torch.empty_like(x), torch.empty_like(y)
        ws = torch.empty((lib.fpsg_sinkhorn_grad_workspace_floats(B, N, N),), device=dev)
        stream = _hip.stream_of(x)

        def forward():
            _hip.check(lib.fpsg_sinkhorn_divergence(_hip.ptr(x), _hip.ptr(y), B, N, N, eps, len(eps_s), _hip.ptr(out),
                                                    _hip.ptr(ws), stream), "fpsg_sinkhorn_divergence")

        def grad(both):
            _hip.check(lib.fpsg_sinkhorn_divergence_grad(_hip.ptr(x), _hip.ptr(y), B, N, N, eps, len(eps_s),
                                                         _hip.ptr(out), _hip.ptr(gx), _hip.ptr(gy) if both else None,
                                                         _hip.ptr(ws), stream), "fpsg_sinkhorn_divergence_grad")

        forms = {"forward": forward, "grad_both": lambda: grad(True), "grad_gx": lambda: grad(False)}
        ms = {k: [] for k in forms}
        for _ in range(rounds):
            for name, fn in forms.items():
                for _ in range(WARM):
                    fn()
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(CALLS):
                    fn()
                e1.record()
                torch.cuda.synchronize()
                ms[name].append(e0.elapsed_time(e1) / CALLS)
        med = {k: statistics.median(v) for k, v in ms.items()}
        res[f"B{B}_N{N}"] = {"ms_per_call": ms, "median_ms": med,
                             "grad_both_over_forward": med["grad_both"] / med["forward"],
                             "grad_gx_over_forward": med["grad_gx"] / med["forward"]}
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import _sinkhorn_grad_ref as ref
    x, y = _clouds(2, 512, dev, 9)
    a, b = x.clone().requires_grad_(), y.clone().requires_grad_()
    g1, g2 = torch.autograd.grad(sinkhorn_loss(a, b, blur=BLUR, diameter=DIAMETER).sum(), [a, b])
    _, r1, r2 = ref.closed_form(x, y, blur=BLUR, diameter=DIAMETER)
    print(json.dumps({"kernel_mode": res, "n_eps": len(eps_s), "launches_forward": len(eps_s) + 3,
                      "yardstick_1_plus_2_over_n_eps_plus_3": 1 + 2 / (len(eps_s) + 3), "warm": WARM, "calls": CALLS, "rounds": rounds,
                      "gradient_row_error_vs_float64_B2_N512": [ref.row_error(g1, r1), ref.row_error(g2, r2)]}))


def training(steps, rounds):
    import bench
    from fpsg_amd import gemm_tuning
    from fpsg_amd.engine import TrainStep, build_model, build_optimizer, default_options
    dev = torch.device("cuda:0")
    gemm_tuning.enable()
    S, Q = 32, 5
    eps = bench.make_episodes(S, Q, 1, seed=1234, device=dev)
    res = {"cd": [], "sinkhorn": []}
    last = {}
    for _ in range(rounds):
        for dist in ("cd", "sinkhorn"):
            opt = default_options(device="cuda", intra_recon=True, pc_encoder="pointnet", n_shot=S, n_query=Q,
                                  pc_dist=dist)
            torch.manual_seed(0)
            model = build_model(opt).to(dev).train()
            optimizer, _ = build_optimizer(model, opt)
            step = TrainStep(model, optimizer, graph=True)
            for _ in range(4):                                 # two eager uses, the capture, one replay
                step(eps, n_episodes_global=1)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                out = step(eps, n_episodes_global=1)
            torch.cuda.synchronize()
            res[dist].append(steps / (time.perf_counter() - t0))
            last[dist] = float(out[0]["ttl_loss"].sum())
            del step, optimizer, model
            torch.cuda.empty_cache()
    print(json.dumps({"train_episodes_per_s": res, "steps": steps, "rounds": rounds, "last_loss": last,
                      "workload": "bench.py's c3 (32-shot 5-query, --intra_recon, pointnet, 1 episode per step, graph "
                                  "replay), B = 37 pairs of 2048 x 2048 per loss call; 'cd' is the parent's path"}))


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else "kernel"
    if mode == "kernel":
        kernel(int(sys.argv[2]) if len(sys.argv) > 2 else 5)
    elif mode == "train":
        training(int(sys.argv[2]) if len(sys.argv) > 2 else 20, int(sys.argv[3]) if len(sys.argv) > 3 else 2)
    else:
        sys.exit(__doc__)
