"""K24 beside K21 and K1 under the profiler: the forward (trees, then the per-cloud sum) and backward of the expansion
penalty, the repulsion term's and K1's forward on the same clouds, B = 37 clouds of N = 2048 points in patches of
P = 128 -- one c5 episode's decoded clouds.  Run it under the kernel trace and keep the statistics (DESIGN.md K24 cites
profiles/k24/):

    rocprofv3 --kernel-trace --stats -d OUT -o expansion -- python tools/profile_expansion.py [--B 37] [--N 2048] [--P 128]
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
    ap.add_argument("--P", type=int, default=128)
    ap.add_argument("--lam", type=float, default=1.5)
    ap.add_argument("--iters", type=int, default=20)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)
    p = torch.tanh(torch.randn((a.B, a.N, 3), generator=g, device=dev)).contiguous()       # the decoder's range
    ref = (torch.rand((a.B, a.N, 3), generator=g, device=dev) * 2 - 1).contiguous()
    x = p.clone().requires_grad_()
    for _ in range(a.iters):
        metrics.sided_distances(p, ref)                                                  # K1 forward, no gradient
        metrics.repulsion_loss(x, 4, 0.03).sum().backward()                              # K21
        x.grad = None
        out = metrics.expansion_penalty(x, a.P, a.lam)                                   # K24
        out.sum().backward()
        x.grad = None
    torch.cuda.synchronize()
    print(f"profile_expansion: {a.iters} x (K1 fwd, K21 fwd + bwd, K24 fwd + bwd) at B={a.B} N={a.N} P={a.P} "
          f"lambda={a.lam}; mean E {float(out.mean()):.6g}")


if __name__ == "__main__":
    main()
