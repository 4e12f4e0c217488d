"""K20 alone and in the step: HIP-event times of fpsg_grad_clip_scale (flat and pointer-table form) and of the _dscale
Adam entries against the plain ones at the model's 77.4 M parameters, alternating in one process, and episodes/s of a
TrainStep loop with and without max_grad_norm.  Appends its figures to profiles/k20/grad_clip_notes.txt.

    python tools/bench_grad_clip.py [--n 77445125] [--pairs 5] [--iters 20] [--steps 12] [--no-step]
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from fpsg_amd import _hip

NOTES = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "k20", "grad_clip_notes.txt")


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


def kernels(n, pairs, iters, out):
    lib = _hip.load()
    dev = torch.device("cuda:0")
    g = torch.randn(n, device=dev)
    p, m, v = torch.randn(n, device=dev), torch.zeros(n, device=dev), torch.zeros(n, device=dev)
    nseg = 600                                          # about the model's number of parameter tensors
    cuts = torch.linspace(0, n, nseg + 1).long()
    cuts[-1] = n
    seg_off = cuts.to(dev)
    table = torch.tensor([g.data_ptr() + 4 * int(c) for c in cuts[:-1]], dtype=torch.int64, device=dev)
    nbytes = lib.fpsg_grad_norm_workspace_bytes(n)
    ws = torch.empty(nbytes // 8, dtype=torch.float64, device=dev)
    out2 = torch.zeros(2, device=dev)
    stats = torch.zeros(4, dtype=torch.float64, device=dev)
    ptr = _hip.ptr
    hyper = (1e-3, 0.9, 0.999, 1e-8, 5)

    def check(rc):
        _hip.check(rc, "bench_grad_clip")

    forms = {
        "clip flat": lambda: check(lib.fpsg_grad_clip_scale(ptr(g), n, 1.0, 1.0, ptr(ws), nbytes, ptr(out2), ptr(stats), None)),
        "clip segments": lambda: check(lib.fpsg_grad_clip_scale_segments(ptr(table), ptr(seg_off), nseg, n, 1.0, 1.0, ptr(ws),
                                                                         nbytes, ptr(out2), ptr(stats), None)),
        "adam plain": lambda: check(lib.fpsg_adam_step(ptr(p), ptr(g), ptr(m), ptr(v), n, *hyper, 1.0, None)),
        "adam dscale": lambda: check(lib.fpsg_adam_step_dscale(ptr(p), ptr(g), ptr(m), ptr(v), n, *hyper, ptr(out2) + 4, None)),
        "adam segments plain": lambda: check(lib.fpsg_adam_step_segments(ptr(p), ptr(table), ptr(seg_off), nseg, ptr(m), ptr(v),
                                                                         n, *hyper, 1.0, None)),
        "adam segments dscale": lambda: check(lib.fpsg_adam_step_segments_dscale(ptr(p), ptr(table), ptr(seg_off), nseg, ptr(m),
                                                                                 ptr(v), n, *hyper, ptr(out2) + 4, None)),
    }
    times = {k: [] for k in forms}
    for _ in range(pairs):                              # alternating: every form once per round
        for k, fn in forms.items():
            times[k].append(timed(fn, iters))
    for k, ts in times.items():
        out.append(f"{k:>22}: {min(ts):8.1f} - {max(ts):8.1f} us over {pairs} rounds of {iters} (n = {n})")


def step_loop(steps, pairs, out):
    from fpsg_amd.engine import TrainStep, build_model, build_optimizer, default_options
    from fpsg_amd.episodes import synthetic_episode
    dev = torch.device("cuda:0")
    ep = synthetic_episode(32, 5, n_pts=2048, img_size=224, seed=1, device=dev)
    runs = {}
    for clip in (0.0, 1.0):
        torch.manual_seed(0)
        opt = default_options(device="cuda", intra_recon=True, clip_grad_norm=clip)
        model = build_model(opt).to(dev).train()
        optimizer, _ = build_optimizer(model, opt)
        runs[clip] = TrainStep(model, optimizer, graph=True)
        for _ in range(4):
            runs[clip]([ep])
    rates = {clip: [] for clip in runs}
    for _ in range(pairs):
        for clip, step in runs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                step([ep])
            torch.cuda.synchronize()
            rates[clip].append(steps / (time.perf_counter() - t0))
    for clip, rs in rates.items():
        name = "max_grad_norm=1.0" if clip else "no clipping"
        out.append(f"TrainStep, one 32-shot episode per step, {name:>18}: {min(rs):.2f} - {max(rs):.2f} episodes/s "
                   f"over {pairs} alternating rounds of {steps}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=77445125)
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--steps", type=int, default=12)
    ap.add_argument("--no-step", action="store_true")
    a = ap.parse_args()
    out = [f"# tools/bench_grad_clip.py on {torch.cuda.get_device_name(0)}, {time.strftime('%Y-%m-%d')}"]
    kernels(a.n, a.pairs, a.iters, out)
    if not a.no_step:
        step_loop(a.steps, a.pairs, out)
    print("\n".join(out))
    os.makedirs(os.path.dirname(NOTES), exist_ok=True)
    with open(NOTES, "a") as f:
        f.write("\n".join(out) + "\n")


if __name__ == "__main__":
    main()
