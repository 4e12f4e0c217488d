"""K17 (fpsg_dist_profile) and what ``evaluate_Network.py --fscore`` costs an item.  On the GPU box:

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o k17 -- python tools/bench_dist_profile.py kernel
    python tools/bench_dist_profile.py summarise DIR          # K17's time per configuration from the kernel trace
    python tools/bench_dist_profile.py eval [items] [rounds]  # items/s of the evaluation loop, flag off / on, alternating

``kernel`` launches K17 at B = 5 and 37, N = M = 2048, T = 1 and 16, LAUNCHES times each after WARM warm-ups, one
configuration after the other: ``summarise`` splits the trace's K17 dispatches in that order.  ``eval`` is bench.py's
evaluation leg (configs[2] episode: 32-shot 5-query) with ``EvalItem(model)`` -- the parent's code path -- against
``EvalItem(model, fscore=(0.01, 0.02, 0.05))``, and HIP events around the second K1 forward and K17."""
import csv
import glob
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CONFIGS = [(5, 1), (5, 16), (37, 1), (37, 16)]            # (B, T) at N = M = 2048
N = 2048
WARM, LAUNCHES = 20, 200
TAUS = (0.01, 0.02, 0.05)


def kernel():
    from fpsg_amd.metrics import distance_profile, sided_distances
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)
    out = {}
    for B, T in CONFIGS:
        p1 = torch.rand((B, N, 3), generator=g, device=dev) * 2 - 1
        p2 = torch.rand((B, N, 3), generator=g, device=dev) * 2 - 1
        d1, _, d2, _ = sided_distances(p1, p2)                # K1's rows, as the evaluation hands them over
        taus = [0.005 * (t + 1) for t in range(T)]
        for _ in range(WARM):
            distance_profile(d1, d2, taus)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(LAUNCHES):
            distance_profile(d1, d2, taus)
        e1.record()
        torch.cuda.synchronize()
        # (the mirror's call, threshold upload and output allocation included: a host-side figure, not the kernel's)
        out[f"B{B}_T{T}"] = {"mirror_call_us": e0.elapsed_time(e1) * 1e3 / LAUNCHES}
    print(json.dumps({"kernel_mode": out, "N": N, "M": N, "launches": LAUNCHES, "warm": WARM}))


def summarise(d):
    files = glob.glob(d + "/**/*kernel_trace.csv", recursive=True)
    if not files:
        sys.exit("no *kernel_trace.csv under " + d)
    rows = []
    for f in files:
        for r in csv.DictReader(open(f)):
            if "dist_profile" in r["Kernel_Name"]:
                rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"])))
    rows.sort()
    per = WARM + LAUNCHES
    if len(rows) != per * len(CONFIGS):
        sys.exit(f"expected {per * len(CONFIGS)} K17 dispatches, found {len(rows)}")
    out = {}
    for k, (B, T) in enumerate(CONFIGS):
        ns = [e - s for s, e in rows[k * per + WARM:(k + 1) * per]]
        out[f"B{B}_T{T}"] = {"kernel_us_median": statistics.median(ns) / 1e3, "kernel_us_mean": statistics.mean(ns) / 1e3,
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
    extra = {"k1_second_forward_us": [], "k17_us": []}

    def loop(run_item, n, on):
        out = None
        for i in range(n):
            out = run_item(eps[i % len(eps)])
            out["cd_loss"].item(), out["emd_loss"].item()
            if on:
                torch.stack([out["fscore"], out["precision"], out["recall"], out["hausdorff"].expand(len(TAUS))]).tolist()
        return out

    for _ in range(rounds):
        for name in ("off", "on"):
            with (EvalItem(model) if name == "off" else EvalItem(model, fscore=TAUS)) as item:
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
                extra["k17_us"].append(sec.get("dist_profile", 0.0) / items * 1e6)
    print(json.dumps({"eval_items_per_s": res, "items": items, "rounds": rounds, "thresholds": TAUS,
                      "ms_per_item": {k: [1e3 / v for v in vs] for k, vs in res.items()},
                      "per_item_event_us_with_flag": extra,
                      "workload": "bench.py's evaluation leg (32-shot 5-query, B = 5 x 2048 x 2048), EvalItem with the "
                                  "graph; 'off' is EvalItem(model), the parent's path"}))


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else "kernel"
    if mode == "kernel":
        kernel()
    elif mode == "summarise":
        summarise(sys.argv[2])
    elif mode == "eval":
        evaluation(int(sys.argv[2]) if len(sys.argv) > 2 else 40, int(sys.argv[3]) if len(sys.argv) > 3 else 3)
    else:
        sys.exit(__doc__)
