"""K13 (all-pairs Chamfer matrix, fpsg_chamfer_cross) against K1's forward in the same run, on unit-ball clouds of
2048 points:

* K13, full mode: 256 x 256 clouds (``chamfer_matrix(A, B)``);
* K13, symmetric mode: 256 clouds against themselves (``chamfer_matrix(A)``, 256 * 255 / 2 pairs evaluated);
* K1's forward (``metrics._sided_forward``, the one-pass tiled kernel and its finalize pass) on 2048 materialised pairs.

Reports the median time per call, distance evaluations per second (each d(i,j) counted once: N * M per pair) and that
rate's fraction of the 157.3 TFLOP/s fp32 peak at 8 flop per distance (K1's convention).

    python tools/bench_chamfer_cross.py [--reps 10] [--out profiles/k13/chamfer_cross_bench.json]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PEAK_FP32 = 157.3e12
FLOP_PER_DIST = 8


def unit_ball(rng, B, N):
    import numpy as np
    v = rng.standard_normal((B, N, 3))
    v /= np.linalg.norm(v, axis=-1, keepdims=True)
    p = v * rng.random((B, N, 1)) ** (1.0 / 3.0)
    p = p - p.mean(axis=1, keepdims=True)
    return (p / np.sqrt((p ** 2).sum(-1)).max(axis=1)[:, None, None]).astype(np.float32)


def timed(fn, reps):
    import numpy as np
    import torch
    fn()                                                    # warm-up (module load, first launch)
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b) * 1e-3)
    return float(np.median(times)), float(min(times)), float(max(times))


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--sets", type=int, default=256, help="clouds per set of K13")
    ap.add_argument("--pairs", type=int, default=2048, help="materialised cloud pairs of K1")
    ap.add_argument("--n", type=int, default=2048, help="points per cloud")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    from fpsg_amd import metrics
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(2024)
    S, P, N = args.sets, args.pairs, args.n
    A = torch.from_numpy(unit_ball(rng, S, N)).to(dev)
    B = torch.from_numpy(unit_ball(rng, S, N)).to(dev)
    p1 = torch.from_numpy(unit_ball(rng, P, N)).to(dev)
    p2 = torch.from_numpy(unit_ball(rng, P, N)).to(dev)
    cases = [
        ("k13_full", lambda: metrics.chamfer_matrix(A, B), S * S * N * N,
         {"Na": S, "Nb": S, "N": N, "M": N}),
        ("k13_symmetric", lambda: metrics.chamfer_matrix(A), S * (S - 1) // 2 * N * N,
         {"Na": S, "N": N, "pairs_evaluated": S * (S - 1) // 2}),
        ("k1_forward", lambda: metrics._sided_forward(p1, p2), P * N * N, {"B": P, "N": N, "M": N}),
    ]
    results = []
    with torch.no_grad():
        for name, fn, dists, shape in cases:
            med, lo, hi = timed(fn, args.reps)
            rate = dists / med
            res = {"case": name, **shape, "reps": args.reps, "s_median": med, "s_min": lo, "s_max": hi,
                   "distances": dists, "distances_per_s": rate, "fp32_peak_fraction": rate * FLOP_PER_DIST / PEAK_FP32}
            print(json.dumps(res))
            results.append(res)
    full, sym = results[0], results[1]
    summary = {"sym_over_full_time": sym["s_median"] / full["s_median"],
               "k13_over_k1_rate": full["distances_per_s"] / results[2]["distances_per_s"]}
    print(json.dumps(summary))
    if args.out:
        with open(args.out, "w") as f:
            json.dump({"results": results, "summary": summary}, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
