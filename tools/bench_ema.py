"""K23 alone: the flat Adam step over the model's 77.4 M parameters without a shadow (fpsg_adam_step, 28 B per
parameter), with the shadow in the same stream (fpsg_adam_step_ema, 36 B) and the un-fused alternative (fpsg_adam_step,
then flat_ema.lerp_(flat_param, w): a second launch, 28 + 12 B).  --lib times the entries another build of the library
has (an older one has only the first), for alternating two builds on one box:

    python tools/bench_ema.py [--lib other/libfpsg_hip.so] [--rounds 3]
"""
import argparse
import ctypes
import sys

import torch

sys.path.insert(0, ".")
from fpsg_amd import _hip  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=_hip.LIB_PATH)
    ap.add_argument("--n", type=int, default=77445125)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    lib = ctypes.CDLL(args.lib)
    names = [n for n in ("fpsg_adam_step", "fpsg_adam_step_ema") if hasattr(lib, n)]
    for name in names:
        getattr(lib, name).argtypes = _hip.SIGNATURES[name]
        getattr(lib, name).restype = ctypes.c_int
    n = args.n
    p, g, e = (torch.randn(n, device="cuda") for _ in range(3))
    m, v = torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")
    stream = _hip.stream_of(p)
    hyper = (1e-3, 0.9, 0.999, 1e-8)
    w = 0.001
    count = [0]

    def plain():
        count[0] += 1
        rc = lib.fpsg_adam_step(_hip.ptr(p), _hip.ptr(g), _hip.ptr(m), _hip.ptr(v), n, *hyper, count[0], 1.0, stream)
        assert rc == 0

    def fused():
        count[0] += 1
        rc = lib.fpsg_adam_step_ema(_hip.ptr(p), _hip.ptr(g), _hip.ptr(m), _hip.ptr(v), _hip.ptr(e), n, *hyper, count[0],
                                    1.0, None, w, stream)
        assert rc == 0

    def unfused():
        plain()
        e.lerp_(p, w)

    def lerp():
        e.lerp_(p, w)

    forms = [("adam_step", plain, 28.0), ("adam_step + lerp_", unfused, 40.0), ("lerp_ alone", lerp, 12.0)]
    if "fpsg_adam_step_ema" in names:
        forms.insert(1, ("adam_step_ema", fused, 36.0))

    def timed(fn):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / args.iters * 1e-3

    print(f"library {args.lib}, n = {n}, {args.iters} calls per figure")
    for r in range(args.rounds):
        for label, fn, nbytes in forms:
            t = timed(fn)
            print(f"round {r}: {label:18s} {t * 1e6:8.1f} us  {nbytes * n / t / 1e9:7.0f} GB/s of its {nbytes:.0f} B per parameter")


if __name__ == "__main__":
    main()
