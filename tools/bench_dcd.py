"""K18 (fpsg_dcd), what ``evaluate_Network.py --dcd`` costs an item and what ``--pc_dist dcd`` costs an episode.  On the
GPU box:

    python tools/bench_dcd.py kernel                 # K18 per launch, back to back, HIP events around the C entry
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o k18 -- python tools/bench_dcd.py kernel
    python tools/bench_dcd.py summarise DIR          # K18's time per configuration from the kernel trace
    python tools/bench_dcd.py eval [items] [rounds]  # items/s of the evaluation loop, flag off / on, alternating
    python tools/bench_dcd.py train [steps] [rounds] # episodes/s of the training step, cd / dcd, alternating

``kernel`` launches K18 at B = 5 and 37, N = M = 2048, on unit-cube clouds and on the collapse case (every point of one
cloud choosing the same target), without and with the weight rows, LAUNCHES times each after WARM warm-ups, one
configuration after the other: ``summarise`` splits the trace's K18 dispatches in that order.  ``eval`` is bench.py's
evaluation leg (32-shot 5-query) with ``EvalItem(model)`` -- the parent's code path -- against ``EvalItem(model,
dcd=1000.0)``.  ``train`` is bench.py's c3 workload (32-shot 5-query, ``--intra_recon``, one episode per step, replayed
as a graph) with ``pc_dist="cd"`` -- the parent's code path, which this change does not touch -- against
``pc_dist="dcd"``."""
import csv
import glob
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CONFIGS = [(5, "cube", False), (5, "cube", True), (37, "cube", False), (37, "cube", True), (5, "collapse", True),
           (37, "collapse", True)]                            # (B, clouds, weight rows) at N = M = 2048
N = 2048
WARM, LAUNCHES = 20, 200
ALPHA = 1000.0


def _clouds(B, kind, dev, g):
    p1 = torch.rand((B, N, 3), generator=g, device=dev) * 2 - 1
    p2 = torch.rand((B, N, 3), generator=g, device=dev) * 2 - 1
    if kind == "collapse":
        p1 = p1 * 1e-3 + 0.5
        p2[:, 0] = 0.5
        p2[:, 1:, 0] = -p2[:, 1:, 0].abs() - 0.5
    return p1.contiguous(), p2.contiguous()


def kernel():
    from fpsg_amd import _hip
    from fpsg_amd.metrics import _sided_forward
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)
    lib = _hip.load()
    out = {}
    for B, kind, weights in CONFIGS:
        p1, p2 = _clouds(B, kind, dev, g)
        d1, d2, i1, i2 = _sided_forward(p1, p2)               # K1's rows, as the mirror hands them over
        res = torch.empty((B,), device=dev)
        sides = torch.empty((B, 2), device=dev)
        deg1 = torch.empty((B, N), dtype=torch.int32, device=dev)
        deg2 = torch.empty((B, N), dtype=torch.int32, device=dev)
        w1 = torch.empty((B, N), device=dev) if weights else None
        w2 = torch.empty((B, N), device=dev) if weights else None
        stream = _hip.stream_of(p1)

        def launch():
            rc = lib.fpsg_dcd(_hip.ptr(d1), _hip.ptr(i1), _hip.ptr(d2), _hip.ptr(i2), B, N, N, ALPHA, _hip.ptr(res),
                              _hip.ptr(sides), _hip.ptr(deg1), _hip.ptr(deg2), None if w1 is None else _hip.ptr(w1),
                              None if w2 is None else _hip.ptr(w2), stream)
            _hip.check(rc, "fpsg_dcd")

        for _ in range(WARM):
            launch()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(LAUNCHES):
            launch()
        e1.record()
        torch.cuda.synchronize()
        # back-to-back launches on one stream: the launch rate where the kernel is shorter than a launch, else its time
        out[f"B{B}_{kind}_{'w' if weights else 'now'}"] = {"back_to_back_us": e0.elapsed_time(e1) * 1e3 / LAUNCHES,
                                                           "max_deg": int(deg2.max())}
    print(json.dumps({"kernel_mode": out, "N": N, "M": N, "alpha": ALPHA, "launches": LAUNCHES, "warm": WARM}))


def summarise(d):
    files = glob.glob(d + "/**/*kernel_trace.csv", recursive=True)
    if not files:
        sys.exit("no *kernel_trace.csv under " + d)
    rows = []
    for f in files:
        for r in csv.DictReader(open(f)):
            if "dcd_kernel" in r["Kernel_Name"]:
                rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"])))
    rows.sort()
    per = WARM + LAUNCHES
    if len(rows) != per * len(CONFIGS):
        sys.exit(f"expected {per * len(CONFIGS)} K18 dispatches, found {len(rows)}")
    out = {}
    for k, (B, kind, weights) in enumerate(CONFIGS):
        ns = [e - s for s, e in rows[k * per + WARM:(k + 1) * per]]
        out[f"B{B}_{kind}_{'w' if weights else 'now'}"] = {
            "kernel_us_median": statistics.median(ns) / 1e3, "kernel_us_mean": statistics.mean(ns) / 1e3,
            "kernel_us_min": min(ns) / 1e3, "kernel_us_max": max(ns) / 1e3, "dispatches": len(ns)}
    print(json.dumps({"rocprofv3_kernel_trace": out, "N": N, "M": N}))


def evaluation(items, rounds):
    import bench
    from fpsg_amd import gemm_tuning, metrics
    from fpsg_amd.engine import EvalItem, build_model, default_options
    dev = torch.device("cuda:0")
    gemm_tuning.enable()
    S, Q = 32, 5
    torch.manual_seed(0)
    model = build_model(default_options(device="cuda", intra_recon=True, pc_encoder="pointnet", n_shot=S,
                                        n_query=Q)).to(dev).eval()
    eps = bench.make_episodes(S, Q, 4, seed=77, device=dev)
    probe = bench.EventProbe()
    probe.enabled = False
    metrics.set_launch_probe(probe)
    res = {"off": [], "on": []}
    extra = {"k1_second_forward_us": [], "k18_us": []}

    def loop(run_item, n, on):
        for i in range(n):
            out = run_item(eps[i % len(eps)])
            out["cd_loss"].item(), out["emd_loss"].item()
            if on:
                out["dcd"].item()

    for _ in range(rounds):
        for name in ("off", "on"):
            with (EvalItem(model) if name == "off" else EvalItem(model, dcd=ALPHA)) as item:
                loop(item, 4, name == "on")                    # two eager items, the capture, one replay
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                loop(item, items, name == "on")
                torch.cuda.synchronize()
                res[name].append(items / (time.perf_counter() - t0))
                assert item._graphs
                probe.records = []
                if name == "on":                               # the events in a pass of their own, not in the timed one
                    probe.enabled = True
                    loop(item, items, True)
                    torch.cuda.synchronize()
                    probe.enabled = False
            sec = {}
            for (k, B, n, m), e0, e1 in probe.records:
                sec[k] = sec.get(k, 0.0) + e0.elapsed_time(e1) * 1e-3
            if name == "on":                                   # (the first K1 forward sits inside the replayed graph)
                extra["k1_second_forward_us"].append(sec.get("chamfer_fwd", 0.0) / items * 1e6)
                extra["k18_us"].append(sec.get("dcd", 0.0) / items * 1e6)
    print(json.dumps({"eval_items_per_s": res, "items": items, "rounds": rounds, "alpha": ALPHA,
                      "ms_per_item": {k: [1e3 / v for v in vs] for k, vs in res.items()},
                      "per_item_event_us_with_flag": extra,
                      "workload": "bench.py's evaluation leg (32-shot 5-query, B = 5 x 2048 x 2048), EvalItem with the "
                                  "graph; 'off' is EvalItem(model), the parent's path"}))


def training(steps, rounds):
    import bench
    from fpsg_amd import gemm_tuning
    from fpsg_amd.engine import TrainStep, build_model, build_optimizer, default_options
    dev = torch.device("cuda:0")
    gemm_tuning.enable()
    S, Q = 32, 5
    eps = bench.make_episodes(S, Q, 1, seed=1234, device=dev)
    res = {"cd": [], "dcd": []}
    last = {}
    for _ in range(rounds):
        for dist in ("cd", "dcd"):
            opt = default_options(device="cuda", intra_recon=True, pc_encoder="pointnet", n_shot=S, n_query=Q,
                                  pc_dist=dist, dcd_alpha=ALPHA)
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
    print(json.dumps({"train_episodes_per_s": res, "steps": steps, "rounds": rounds, "alpha": ALPHA, "last_loss": last,
                      "workload": "bench.py's c3 (32-shot 5-query, --intra_recon, pointnet, 1 episode per step, graph "
                                  "replay), B = 37 pairs of 2048 x 2048 per K1 / K18 call; 'cd' is the parent's path"}))


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else "kernel"
    if mode == "kernel":
        kernel()
    elif mode == "summarise":
        summarise(sys.argv[2])
    elif mode == "eval":
        evaluation(int(sys.argv[2]) if len(sys.argv) > 2 else 40, int(sys.argv[3]) if len(sys.argv) > 3 else 3)
    elif mode == "train":
        training(int(sys.argv[2]) if len(sys.argv) > 2 else 20, int(sys.argv[3]) if len(sys.argv) > 3 else 2)
    else:
        sys.exit(__doc__)
