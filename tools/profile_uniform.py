"""K25 beside K16 and K21 under the profiler: the seeds (farthest point sampling, 5 % of the cloud), the forward and
backward of the uniform loss and of the repulsion term on the same clouds, B = 37 clouds of N = 2048 points -- one c5
episode's decoded clouds.  Run it under the kernel trace and keep the statistics (DESIGN.md K25 cites profiles/k25/):

    rocprofv3 --kernel-trace --stats -d OUT -o uniform -- python tools/profile_uniform.py [--B 37] [--N 2048]
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
    ap.add_argument("--iters", type=int, default=20)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)
    p = torch.tanh(torch.randn((a.B, a.N, 3), generator=g, device=dev)).contiguous()       # the decoder's range
    x = p.clone().requires_grad_()
    for _ in range(a.iters):
        rep = metrics.repulsion_loss(x, 4, 0.03)                                         # K21 forward and backward
        rep.sum().backward()
        x.grad = None
        out, info = metrics.uniform_loss(x, return_info=True)                            # K16, K25 forward and backward
        out.sum().backward()
        x.grad = None
    torch.cuda.synchronize()
    c = info["count"]
    print(f"profile_uniform: {a.iters} x (K21 fwd, bwd, K16, K25 fwd, bwd) at B={a.B} N={a.N} S={c.size(2)} T={c.size(1)} "
          f"cap={info['member'].size(3)}; mean U {float(out.mean()):.6g}; count median {int(c.median())} max {int(c.max())}")


if __name__ == "__main__":
    main()
