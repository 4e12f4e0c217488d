"""K25 alone and in the step: HIP-event times of K16's seeds (farthest point sampling, 5 % of the cloud), of
fpsg_uniform_fwd / _bwd on given seeds and of the whole term, beside K21's forward and backward on the same clouds
(B = 37, N = 2048: one c5 episode's decoded clouds), alternating in one process, and episodes/s of a TrainStep loop with
uniform_weight 0 and 0.1.  Appends its figures to profiles/k25/uniform_notes.txt.

    python tools/bench_uniform.py [--B 37] [--N 2048] [--pairs 5] [--iters 20] [--steps 12] [--no-step]
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from fpsg_amd import metrics
from fpsg_amd.sampling import farthest_point_sample

NOTES = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "k25", "uniform_notes.txt")


def timed(fn, iters):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3          # us


def kernels(B, N, pairs, iters, out):
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)
    p = torch.tanh(torch.randn((B, N, 3), generator=g, device=dev)).contiguous()
    S = max(1, N // 20)
    seeds = farthest_point_sample(p, S)
    x = p.clone().requires_grad_()

    def uniform_both(seeds=None):
        metrics.uniform_loss(x, seeds=seeds).sum().backward()
        x.grad = None

    def repulsion_both():
        metrics.repulsion_loss(x, 4, 0.03).sum().backward()
        x.grad = None

    forms = {f"K16 seeds (n = {S})": lambda: farthest_point_sample(p, S),
             "K25 fwd, given seeds": lambda: metrics.uniform_loss(p, seeds=seeds),
             "K25 fwd + bwd, given seeds (with autograd)": lambda: uniform_both(seeds),
             "K16 + K25 fwd + bwd (with autograd)": uniform_both,
             "K21 fwd k=4": lambda: metrics.repulsion_loss(p, 4, 0.03),
             "K21 fwd + bwd k=4 (with autograd)": repulsion_both}
    times = {name: [] for name in forms}
    for _ in range(pairs):                              # alternating: every form once per round
        for name, fn in forms.items():
            times[name].append(timed(fn, iters))
    for name, ts in times.items():
        out.append(f"{name:>44}: {min(ts):8.1f} - {max(ts):8.1f} us per call (host-paced events) over {pairs} rounds of "
                   f"{iters} (B = {B}, N = {N})")


def step_loop(steps, pairs, out):
    from fpsg_amd.engine import TrainStep, build_model, build_optimizer, default_options
    from fpsg_amd.episodes import synthetic_episode
    dev = torch.device("cuda:0")
    ep = synthetic_episode(32, 5, n_pts=2048, img_size=224, seed=1, device=dev)
    runs = {}
    for weight in (0.0, 0.1):
        torch.manual_seed(0)
        opt = default_options(device="cuda", intra_recon=True, uniform_weight=weight)
        model = build_model(opt).to(dev).train()
        optimizer, _ = build_optimizer(model, opt)
        runs[weight] = TrainStep(model, optimizer, graph=True)
        for _ in range(4):
            runs[weight]([ep])
    rates = {weight: [] for weight in runs}
    for _ in range(pairs):
        for weight, step in runs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                step([ep])
            torch.cuda.synchronize()
            rates[weight].append(steps / (time.perf_counter() - t0))
    for weight, rs in rates.items():
        name = f"uniform_weight={weight}" if weight else "no uniform term"
        out.append(f"TrainStep, one 32-shot 5-query episode per step, {name:>20}: {min(rs):.2f} - {max(rs):.2f} episodes/s "
                   f"over {pairs} alternating rounds of {steps}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=37)
    ap.add_argument("--N", type=int, default=2048)
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--steps", type=int, default=12)
    ap.add_argument("--no-step", action="store_true")
    a = ap.parse_args()
    out = [f"# tools/bench_uniform.py on {torch.cuda.get_device_name(0)}, {time.strftime('%Y-%m-%d')}"]
    kernels(a.B, a.N, a.pairs, a.iters, out)
    if not a.no_step:
        step_loop(a.steps, a.pairs, out)
    print("\n".join(out))
    os.makedirs(os.path.dirname(NOTES), exist_ok=True)
    with open(NOTES, "a") as f:
        f.write("\n".join(out) + "\n")


if __name__ == "__main__":
    main()
