"""K24 in the step: episodes/s of a TrainStep(graph=True) loop, one 32-shot 5-query episode per step, with
expansion_weight 0 and 0.1, alternating in one process (as tools/bench_repulsion.py does for K21).  Appends its figures
to profiles/k24/expansion_notes.txt.

    python tools/bench_expansion.py [--pairs 5] [--steps 12]
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

NOTES = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "k24", "expansion_notes.txt")


def step_loop(steps, pairs, out):
    from fpsg_amd.engine import TrainStep, build_model, build_optimizer, default_options
    from fpsg_amd.episodes import synthetic_episode
    dev = torch.device("cuda:0")
    ep = synthetic_episode(32, 5, n_pts=2048, img_size=224, seed=1, device=dev)
    runs = {}
    for weight in (0.0, 0.1):
        torch.manual_seed(0)
        opt = default_options(device="cuda", intra_recon=True, expansion_weight=weight)
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
        name = f"expansion_weight={weight}" if weight else "no expansion term"
        out.append(f"TrainStep, one 32-shot 5-query episode per step, {name:>22}: {min(rs):.2f} - {max(rs):.2f} episodes/s "
                   f"over {pairs} alternating rounds of {steps}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--steps", type=int, default=12)
    a = ap.parse_args()
    out = [f"# tools/bench_expansion.py on {torch.cuda.get_device_name(0)}, {time.strftime('%Y-%m-%d')}"]
    step_loop(a.steps, a.pairs, out)
    print("\n".join(out))
    os.makedirs(os.path.dirname(NOTES), exist_ok=True)
    with open(NOTES, "a") as f:
        f.write("\n".join(out) + "\n")


if __name__ == "__main__":
    main()
