"""K21 beside K1 under the profiler: the forward and backward of the repulsion term and K1's forward on the same clouds,
B = 37 clouds of N = 2048 points, k = 4 -- one c5 episode's decoded clouds.  Run it under the kernel trace and keep the
statistics (DESIGN.md K21 cites profiles/k21/):

    rocprofv3 --kernel-trace --stats -d OUT -o repulsion -- python tools/profile_repulsion.py [--B 37] [--N 2048] [--k 4]
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
    ap.add_argument("--k", type=int, default=4)
    ap.add_argument("--h", type=float, default=0.03)
    ap.add_argument("--iters", type=int, default=20)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)
    p = torch.tanh(torch.randn((a.B, a.N, 3), generator=g, device=dev)).contiguous()       # the decoder's range
    ref = (torch.rand((a.B, a.N, 3), generator=g, device=dev) * 2 - 1).contiguous()
    x = p.clone().requires_grad_()
    for _ in range(a.iters):
        metrics.sided_distances(p, ref)                                                  # K1 forward, no gradient
        out = metrics.repulsion_loss(x, a.k, a.h)
        out.sum().backward()
        x.grad = None
    torch.cuda.synchronize()
    print(f"profile_repulsion: {a.iters} x (K1 fwd, K21 fwd, K21 bwd) at B={a.B} N={a.N} k={a.k} h={a.h}; "
          f"mean R {float(out.mean()):.6g}")


if __name__ == "__main__":
    main()
