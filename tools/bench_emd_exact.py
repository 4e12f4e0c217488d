"""K12 (exact EMD, fpsg_emd_exact) timed on unit-ball cloud pairs of 2048 points: B = 5 (the evaluation shape: 5
query clouds per item at 32 shots / 5 queries) and B = 37.  Reports, per shape, the median time of a call, the auction
rounds each pair used and the certificate gap relative to N * eps and to the cost.

    python tools/bench_emd_exact.py [--reps 5] [--out profiles/k12_emd_exact.json]

Every shape is measured in a child process of its own under ``timeout -k 10 <s>``; a step that fails or runs out of
time ends the run (nothing after it is started)."""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(5, 2048), (37, 2048)]


def unit_ball(rng, B, N):
    import numpy as np
    v = rng.standard_normal((B, N, 3))
    v /= np.linalg.norm(v, axis=-1, keepdims=True)
    p = v * rng.random((B, N, 1)) ** (1.0 / 3.0)
    p = p - p.mean(axis=1, keepdims=True)
    return (p / np.sqrt((p ** 2).sum(-1)).max(axis=1)[:, None, None]).astype(np.float32)


def one(B: int, N: int, reps: int) -> dict:
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    from fpsg_amd.metrics import emd_exact, emd_exact_default_eps
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(B * 7919 + N)
    p1 = torch.from_numpy(unit_ball(rng, B, N)).to(dev)
    p2 = torch.from_numpy(unit_ball(rng, B, N)).to(dev)
    eps = emd_exact_default_eps(p1, p2)
    emd_exact(p1, p2, eps=eps)                              # warm-up (module load)
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        cost, info = emd_exact(p1, p2, eps=eps, return_info=True)
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b))
    cost = cost.cpu().numpy().astype(float)
    gap = info["gap"].cpu().numpy().astype(float)
    rounds = info["rounds"].cpu().numpy().tolist()
    return {"B": B, "N": N, "eps": eps, "reps": reps, "ms_median": float(np.median(times)),
            "ms_min": float(min(times)), "ms_max": float(max(times)),
            "rounds_min": int(min(rounds)), "rounds_median": float(np.median(rounds)), "rounds_max": int(max(rounds)),
            "status": info["status"].cpu().numpy().tolist(), "cost_mean": float(cost.mean()),
            "gap_over_N_eps_max": float((gap / (N * eps)).max()), "gap_over_cost_max": float((gap / cost).max())}


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--timeout", type=int, default=300, help="seconds per shape")
    ap.add_argument("--out", default="")
    ap.add_argument("--one", nargs=2, type=int, metavar=("B", "N"), help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.one:
        print(json.dumps(one(args.one[0], args.one[1], args.reps)))
        return 0
    results = []
    for B, N in SHAPES:
        cmd = ["timeout", "-k", "10", str(args.timeout), sys.executable, os.path.abspath(__file__), "--reps",
               str(args.reps), "--one", str(B), str(N)]
        r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True)
        if r.returncode != 0:
            print(f"B={B} N={N}: exit status {r.returncode}; stopping\n{r.stdout[-2000:]}{r.stderr[-2000:]}")
            return 1
        res = json.loads(r.stdout.strip().splitlines()[-1])
        print(json.dumps(res))
        results.append(res)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
