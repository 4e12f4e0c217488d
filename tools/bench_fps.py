"""K16 (farthest point sampling, fpsg_fps) against the same selection written as a plain PyTorch loop (per round: the
distances to the last pick, ``minimum``, ``argmax``), on one card, in the same process, on unit-ball clouds.

Per shape (B, N, n): microseconds per launch and per round for K16 (HIP events around ``--reps`` launches after warm-up,
``--windows`` windows, median and minimum), the time of the PyTorch loop (one warm-up pass, then ``--loop_reps`` timed
passes), the ratio, the fraction of picks on which the two agree (the loop rounds its distances differently), and
the shader clock the card reported under the load.  Each shape runs in a child process under its own
``timeout -k 10 <s>``; the shapes run one after the other and the first failure ends the run.

    python tools/bench_fps.py [--out profiles/k16/fps_bench.txt]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(1, 2048, 2048), (64, 2048, 512), (256, 2048, 512), (5, 15000, 2048)]


def unit_ball(rng, B, N):
    import numpy as np
    v = rng.standard_normal((B, N, 3))
    v /= np.linalg.norm(v, axis=-1, keepdims=True)
    p = v * rng.random((B, N, 1)) ** (1.0 / 3.0)
    p = p - p.mean(axis=1, keepdims=True)
    return (p / np.sqrt((p ** 2).sum(-1)).max(axis=1)[:, None, None]).astype(np.float32)


def torch_loop(points, n):
    """The selection of K16's definition in PyTorch operators: three launches and more per round."""
    import torch
    B, N, _ = points.shape
    rows = torch.arange(B, device=points.device)
    idx = torch.zeros((B, n), dtype=torch.int64, device=points.device)
    D = torch.full((B, N), float("inf"), device=points.device)
    last = idx[:, 0]
    for t in range(1, n):
        D = torch.minimum(D, ((points - points[rows, last].unsqueeze(1)) ** 2).sum(-1))
        last = D.argmax(dim=1)
        idx[:, t] = last
    return idx


def step(args) -> dict:
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    from bench import gpu_clock_mhz
    from fpsg_amd.sampling import farthest_point_sample
    B, N, n = args.shape
    dev = torch.device("cuda:0")
    pts = torch.from_numpy(unit_ball(np.random.default_rng(2024), B, N)).to(dev)
    for _ in range(3):
        idx = farthest_point_sample(pts, n)
    torch.cuda.synchronize()
    windows = []
    clock = None
    for w in range(args.windows):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.reps):
            farthest_point_sample(pts, n)
        e1.record()
        if w == args.windows - 1:
            clock = gpu_clock_mhz(dev)                             # while the launches are still executing
        torch.cuda.synchronize()
        windows.append(e0.elapsed_time(e1) * 1e3 / args.reps)
    ref = torch_loop(pts, n)
    torch.cuda.synchronize()
    loops = []
    for _ in range(args.loop_reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        torch_loop(pts, n)
        e1.record()
        torch.cuda.synchronize()
        loops.append(e0.elapsed_time(e1) * 1e3)
    k16, loop = statistics.median(windows), statistics.median(loops)
    return {"B": B, "N": N, "n": n, "k16_us_per_launch_median": k16, "k16_us_per_launch_min": min(windows),
            "k16_us_per_round": k16 / max(n - 1, 1), "torch_loop_us_median": loop, "torch_loop_us_min": min(loops),
            "torch_loop_over_k16": loop / k16, "picks_equal_fraction": float((ref == idx).float().mean()),
            "sclk_mhz": clock, "reps": args.reps, "windows": args.windows, "loop_reps": args.loop_reps}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "k16", "fps_bench.txt"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--loop_reps", type=int, default=3)
    ap.add_argument("--timeout", type=int, default=240, help="seconds per shape")
    ap.add_argument("--shape", type=int, nargs=3, default=None, help=argparse.SUPPRESS)   # the child's one shape
    args = ap.parse_args()
    if args.shape is not None:
        print("RESULT " + json.dumps(step(args)))
        return
    lines = ["K16 fpsg_fps against a plain PyTorch loop, one MI355X, unit-ball clouds "
             f"(HIP events; {args.windows} windows of {args.reps} launches; loop: {args.loop_reps} passes)."]
    for shape in SHAPES:
        cmd = ["timeout", "-k", "10", str(args.timeout), sys.executable, os.path.abspath(__file__), "--shape",
               *map(str, shape), "--reps", str(args.reps), "--windows", str(args.windows), "--loop_reps",
               str(args.loop_reps)]
        r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True)
        got = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
        if r.returncode != 0 or not got:
            print(r.stdout[-2000:] + r.stderr[-2000:])
            raise SystemExit(f"shape {shape}: exit status {r.returncode}; nothing more is started")
        m = json.loads(got[-1][7:])
        lines.append(f"(B,N,n)=({m['B']},{m['N']},{m['n']}): K16 {m['k16_us_per_launch_median']:.1f} us/launch (min "
                     f"{m['k16_us_per_launch_min']:.1f}), {m['k16_us_per_round']:.3f} us/round; PyTorch loop "
                     f"{m['torch_loop_us_median']:.0f} us (min {m['torch_loop_us_min']:.0f}) = "
                     f"{m['torch_loop_over_k16']:.1f} x K16; picks equal {m['picks_equal_fraction']:.4f}; "
                     f"sclk {m['sclk_mhz']} MHz")
        print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
