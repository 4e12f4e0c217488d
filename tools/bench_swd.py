"""K22 alone and in the step: HIP-event times of one fpsg_swd call (forward only; with both gradients) beside K1's forward
on the same clouds (B = 37, N = 2048: one c5 episode's decoded clouds) for L = 64 and 128, alternating in one process,
and episodes/s of a TrainStep loop with pc_dist cd and swd.  Appends its figures to profiles/k22/swd_notes.txt.

    python tools/bench_swd.py [--B 37] [--N 2048] [--pairs 3] [--iters 20] [--steps 10] [--no-step]
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from fpsg_amd import metrics

NOTES = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "k22", "swd_notes.txt")


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
    ref = (torch.rand((B, N, 3), generator=g, device=dev) * 2 - 1).contiguous()
    x, y = p.clone().requires_grad_(), ref.clone().requires_grad_()
    forms = {"K1 fwd (sided_distances)": lambda: metrics.sided_distances(p, ref)}
    for L in (64, 128):
        dirs = metrics.swd_directions(L, dev)
        forms[f"K22 value only L={L}"] = lambda dirs=dirs: metrics.swd_loss(p, ref, dirs)
        forms[f"K22 value + both gradients L={L}"] = lambda dirs=dirs: metrics.swd_loss(x, y, dirs)
    times = {name: [] for name in forms}
    for _ in range(pairs):                              # alternating: every form once per round
        for name, fn in forms.items():
            times[name].append(timed(fn, iters))
    for name, ts in times.items():
        out.append(f"{name:>36}: {min(ts):8.1f} - {max(ts):8.1f} us per call (host-paced events) over {pairs} rounds of "
                   f"{iters} (B = {B}, N = {N})")


def step_loop(steps, pairs, out):
    from fpsg_amd.engine import TrainStep, build_model, build_optimizer, default_options
    from fpsg_amd.episodes import synthetic_episode
    dev = torch.device("cuda:0")
    ep = synthetic_episode(32, 5, n_pts=2048, img_size=224, seed=1, device=dev)
    runs = {}
    for dist in ("cd", "swd"):
        torch.manual_seed(0)
        opt = default_options(device="cuda", intra_recon=True, pc_dist=dist)
        model = build_model(opt).to(dev).train()
        optimizer, _ = build_optimizer(model, opt)
        runs[dist] = TrainStep(model, optimizer, graph=True)
        for _ in range(4):
            runs[dist]([ep])
    rates = {dist: [] for dist in runs}
    for _ in range(pairs):
        for dist, step in runs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                step([ep])
            torch.cuda.synchronize()
            rates[dist].append(steps / (time.perf_counter() - t0))
    for dist, rs in rates.items():
        out.append(f"TrainStep, one 32-shot 5-query episode per step, pc_dist={dist:>4}: {min(rs):.2f} - {max(rs):.2f} episodes/s "
                   f"over {pairs} alternating rounds of {steps}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=37)
    ap.add_argument("--N", type=int, default=2048)
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--no-step", action="store_true")
    a = ap.parse_args()
    out = [f"# tools/bench_swd.py on {torch.cuda.get_device_name(0)}, {time.strftime('%Y-%m-%d')}"]
    kernels(a.B, a.N, a.pairs, a.iters, out)
    if not a.no_step:
        step_loop(a.steps, a.pairs, out)
    print("\n".join(out))
    os.makedirs(os.path.dirname(NOTES), exist_ok=True)
    with open(NOTES, "a") as f:
        f.write("\n".join(out) + "\n")


if __name__ == "__main__":
    main()
