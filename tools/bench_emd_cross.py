"""K14 (all-pairs exact EMD matrix, fpsg_emd_cross) against a loop of K12 (fpsg_emd_exact) over batches of the same
pairs, in the same run, on unit-ball clouds of 2048 points:

* K14, full mode: S x S clouds (``emd_matrix(A, B)``, S * S pairs);
* K14, symmetric mode: S clouds against themselves (``emd_matrix(A)``, S * (S - 1) / 2 pairs solved);
* K12: ``emd_exact`` over batches of ``--batch`` materialised pairs of the full mode, the loop covering all S * S.

All three use one eps (``emd_exact_default_eps`` over both sets).  Reports the time of each and pairs per second,
and checks that K12's and K14's rounds agree on every pair.  Each step runs in a child process under its own
``timeout -k 10 <s>``; the steps run one after the other and the first failure ends the run.

    python tools/bench_emd_cross.py [--sets 64] [--n 2048] [--out profiles/k14/emd_cross_bench.json]
"""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def unit_ball(rng, B, N):
    import numpy as np
    v = rng.standard_normal((B, N, 3))
    v /= np.linalg.norm(v, axis=-1, keepdims=True)
    p = v * rng.random((B, N, 1)) ** (1.0 / 3.0)
    p = p - p.mean(axis=1, keepdims=True)
    return (p / np.sqrt((p ** 2).sum(-1)).max(axis=1)[:, None, None]).astype(np.float32)


def step(args) -> dict:
    """One measurement in this process: ``args.step`` in {full, sym, k12}."""
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    from fpsg_amd.metrics import emd_exact, emd_exact_default_eps, emd_matrix
    rng = np.random.default_rng(2024)
    S, N = args.sets, args.n
    dev = torch.device("cuda:0")
    A = torch.from_numpy(unit_ball(rng, S, N)).to(dev)
    B = torch.from_numpy(unit_ball(rng, S, N)).to(dev)
    eps = emd_exact_default_eps(A, B)
    emd_matrix(A[:2].contiguous(), B[:1].contiguous(), eps=eps)          # module load, first launch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    if args.step == "full":
        cost, info = emd_matrix(A, B, eps=eps, return_info=True)
        pairs = S * S
    elif args.step == "sym":
        cost, info = emd_matrix(A, eps=eps, return_info=True)
        pairs = S * (S - 1) // 2
    else:
        a_idx = torch.arange(S, device=dev).repeat_interleave(S)
        b_idx = torch.arange(S, device=dev).repeat(S)
        costs, rounds, status = [], [], []
        for s in range(0, S * S, args.batch):
            p1 = A[a_idx[s:s + args.batch]].contiguous()
            p2 = B[b_idx[s:s + args.batch]].contiguous()
            c, inf = emd_exact(p1, p2, eps=eps, return_info=True)
            costs.append(c)
            rounds.append(inf["rounds"].clone())
            status.append(inf["status"])
        cost = torch.cat(costs).reshape(S, S)
        info = {"rounds": torch.cat(rounds).reshape(S, S), "status": torch.cat(status).reshape(S, S)}
        pairs = S * S
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    r = info["rounds"].cpu().numpy()
    if args.step == "sym":
        r = r[np.triu_indices(S, 1)]
    res = {"step": args.step, "sets": S, "n": N, "eps": eps, "pairs": pairs, "seconds": dt, "pairs_per_s": pairs / dt,
           "rounds_min": int(r.min()), "rounds_median": float(np.median(r)), "rounds_max": int(r.max()),
           "capped": int((info["status"] != 0).sum().item()), "mean_cost": float(cost.double().mean())}
    if args.step != "sym":
        np.save(os.path.join(args.tmp, f"rounds_{args.step}.npy"), info["rounds"].cpu().numpy())
    return res


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--sets", type=int, default=64, help="clouds per set")
    ap.add_argument("--n", type=int, default=2048, help="points per cloud")
    ap.add_argument("--batch", type=int, default=256, help="pairs per emd_exact call of the K12 loop")
    ap.add_argument("--timeout", type=int, default=600, help="seconds per step")
    ap.add_argument("--out", default="")
    ap.add_argument("--step", default="", help=argparse.SUPPRESS)
    ap.add_argument("--tmp", default="", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.step:
        print(json.dumps(step(args)))
        return 0
    import tempfile
    import numpy as np
    results = {}
    with tempfile.TemporaryDirectory() as tmp:
        for name in ("full", "sym", "k12"):
            cmd = ["timeout", "-k", "10", str(args.timeout), sys.executable, os.path.abspath(__file__), "--step", name,
                   "--sets", str(args.sets), "--n", str(args.n), "--batch", str(args.batch), "--tmp", tmp]
            r = subprocess.run(cmd, capture_output=True, text=True)
            if r.returncode != 0:
                print(f"step {name} failed with exit status {r.returncode}:\n{r.stdout[-2000:]}{r.stderr[-2000:]}",
                      file=sys.stderr)
                return 1
            results[name] = json.loads(r.stdout.strip().splitlines()[-1])
            print(json.dumps(results[name]), flush=True)
        same = bool(np.array_equal(np.load(os.path.join(tmp, "rounds_full.npy")),
                                   np.load(os.path.join(tmp, "rounds_k12.npy"))))
    out = {"kernel": "K14 emd_cross vs K12 emd_exact loop", "results": results,
           "rounds_equal_k12": same,
           "speedup_full_vs_k12_loop": results["full"]["pairs_per_s"] / results["k12"]["pairs_per_s"],
           "speedup_sym_vs_k12_loop": results["sym"]["pairs_per_s"] / results["k12"]["pairs_per_s"]}
    print(json.dumps(out))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=2)
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
