"""K22 beside K1 under the profiler: one fpsg_swd call with both gradients and K1's forward on the same clouds, B = 37
pairs of N = 2048 points -- one c5 episode's decoded clouds -- on the fixed lattice of L directions.  Run it under the
kernel trace and keep the statistics (DESIGN.md K22 cites profiles/k22/):

    rocprofv3 --kernel-trace --stats -d OUT -o swd -- python tools/profile_swd.py [--B 37] [--N 2048] [--L 64]
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from fpsg_amd import metrics


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=37)
    ap.add_argument("--N", type=int, default=2048)
    ap.add_argument("--L", type=int, default=64)
    ap.add_argument("--iters", type=int, default=20)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)
    p = torch.tanh(torch.randn((a.B, a.N, 3), generator=g, device=dev)).contiguous()       # the decoder's range
    ref = (torch.rand((a.B, a.N, 3), generator=g, device=dev) * 2 - 1).contiguous()
    dirs = metrics.swd_directions(a.L, dev)
    x, y = p.clone().requires_grad_(), ref.clone().requires_grad_()
    for _ in range(a.iters):
        metrics.sided_distances(p, ref)                                                  # K1 forward, no gradient
        out = metrics.swd_loss(x, y, dirs)                                               # K22: value and both gradients
    torch.cuda.synchronize()
    print(f"profile_swd: {a.iters} x (K1 fwd, K22 with both gradients) at B={a.B} N={a.N} L={a.L}; "
          f"mean SWD {float(out.mean()):.6g}")


if __name__ == "__main__":
    main()
