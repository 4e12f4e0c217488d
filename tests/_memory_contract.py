"""The contract table of the memory-contract tests: one row builder per workspace-taking entry of include/fpsg_hip.h.

A row builds one valid call of its entry for one shape: the inputs (CPU tensors from a seeded generator), the outputs and
in/out buffers, the workspace sized by the entry's own size function, each buffer with the alignment the header documents
for it (4 bytes by the header's general rule unless the entry's text says 8 or 16).  tests/test_memory_contract_cpu.py
checks the table against the header and the size functions on the host; tests/test_memory_contract_gpu.py runs every
case in guarded arenas (tests/_guarded.py).

CASES lists (id, entry, builder, arguments).  Shapes are the smallest at which a kernel can still go wrong: (a) the
minimum the entry accepts, (b) one past the largest tile / segment / stage constant of the kernel in every dimension
that can be ragged (the constant is named beside the case), (c) a batch of 3 with both ragged dimensions.
"""
from __future__ import annotations

import ctypes
import math

import torch

from _guarded import inp, out, inout, ws as ws_buf

F32, I32, I64, U8, F64 = torch.float32, torch.int32, torch.int64, torch.uint8, torch.float64

# Workspace-taking entries that the table leaves out, each with its reason.
EXCLUDED = {
    "fpsg_max_bwd_scatter": "guard elements behind its in/out gradient and its workspace: tests/test_maxbwd_gpu.py",
}

# Entries of the table WITHOUT a caller workspace (the header scan does not turn them up): the backward halves of K21,
# K24 and K25, which read what the guarded forwards wrote.
NO_WORKSPACE = ("fpsg_repulsion_bwd", "fpsg_expansion_bwd", "fpsg_uniform_bwd")


class Row:
    """One call.  call(p, stream, wsn): p maps buffer names to addresses (None = NULL), wsn is the workspace size in the
    entry's own unit, passed where the entry has a size argument."""

    def __init__(self, bufs, call, ws_units=0, size_arg=False, refuses=False, needs_ws=True, late=None):
        self.bufs, self.call = bufs, call
        self.ws_units = int(ws_units)       # what the size function returned
        self.size_arg = size_arg            # the entry takes ws_bytes / workspace_bytes / ws_floats
        self.refuses = refuses              # header: a workspace too small is FPSG_E_SHAPE "before any launch"
        self.needs_ws = needs_ws            # False where the header says the entry needs no workspace (size 0)
        self.late = late                    # late(p) -> {name: CPU tensor}: inputs that hold addresses of other buffers


def _g(seed):
    return torch.Generator().manual_seed(seed)


def _randn(g, *shape):
    return torch.randn(*shape, generator=g, dtype=F32)


def _rand(g, *shape):
    return torch.rand(*shape, generator=g, dtype=F32)


def _randint(g, lo, hi, *shape):
    return torch.randint(lo, hi, shape, generator=g, dtype=I32)


def _cf(vals):
    return (ctypes.c_float * len(vals))(*[float(v) for v in vals])


def _f(v):
    return ctypes.c_float(v)


def _W(units, unit_bytes, align):
    return ws_buf("ws", int(units) * unit_bytes, align)


# ---- K1 -------------------------------------------------------------------------------------------------------------
def chamfer_tiled(lib, B, N, M, variant, losses=False):
    g = _g(1)
    nbytes = lib.fpsg_chamfer_workspace_bytes(B, N, M, variant)
    bufs = [inp("xyz1", _randn(g, B, N, 3)), inp("xyz2", _randn(g, B, M, 3)),
            out("dist1", F32, (B, N)), out("idx1", I32, (B, N)), out("dist2", F32, (B, M)), out("idx2", I32, (B, M)),
            _W(nbytes, 1, 8)]                                       # "ws: ... bytes, 8-byte aligned"
    if losses:
        bufs.append(out("out3", F32, (3,)))

        def call(p, s, wsn):
            return lib.fpsg_chamfer_fwd_tiled_losses(p["xyz1"], p["xyz2"], B, N, M, p["dist1"], p["idx1"], p["dist2"],
                                                     p["idx2"], p["ws"], wsn, variant, (B + 1) // 2, _f(0.75), _f(0.25),
                                                     p["out3"], s)
    else:
        def call(p, s, wsn):
            return lib.fpsg_chamfer_fwd_tiled(p["xyz1"], p["xyz2"], B, N, M, p["dist1"], p["idx1"], p["dist2"], p["idx2"],
                                              p["ws"], wsn, variant, s)
    return Row(bufs, call, nbytes, size_arg=True)


# ---- K3 -------------------------------------------------------------------------------------------------------------
def knn(lib, B, C, N, k, layout=0, flags=0, ex=False):
    g = _g(3)
    x = _randn(g, B, C, N) if layout == 0 else _randn(g, B, N, C)
    floats = lib.fpsg_knn_workspace_floats(B, C, N)
    bufs = [inp("x", x), out("idx", I32, (B, N, k)), _W(floats, 4, 16)]     # "floats, 16-byte aligned"
    if ex:
        def call(p, s, wsn):
            return lib.fpsg_knn_ex(p["x"], layout, B, C, N, k, p["idx"], p["ws"], flags, s)
    else:
        def call(p, s, wsn):
            return lib.fpsg_knn(p["x"], B, C, N, k, p["idx"], p["ws"], s)
    return Row(bufs, call, floats)


# ---- K2 / K2b / K19 ---------------------------------------------------------------------------------------------------
def emd_approx(lib, B, N, M, grads, variant=None):
    g = _g(2)
    floats = lib.fpsg_emd_workspace_floats(B, N, M)
    bufs = [inp("xyz1", _rand(g, B, N, 3)), inp("xyz2", _rand(g, B, M, 3)), out("cost", F32, (B,)),
            _W(floats, 4, 16)]                                      # "floats, 16-byte aligned"
    if grads:
        bufs += [out("gxyz1", F32, (B, N, 3)), out("gxyz2", F32, (B, M, 3))]

    def call(p, s, wsn):
        if variant is None:
            return lib.fpsg_emd_approx(p["xyz1"], p["xyz2"], B, N, M, p["cost"], p.get("gxyz1"), p.get("gxyz2"), p["ws"], s)
        return lib.fpsg_emd_approx_variant(p["xyz1"], p["xyz2"], B, N, M, p["cost"], p.get("gxyz1"), p.get("gxyz2"),
                                           p["ws"], variant, s)
    return Row(bufs, call, floats)


_EPS = (1.0, 0.25, 0.0625, 0.01, 0.01)       # a short geomloss-style schedule: diameter^2 down to blur^2, blur^2 again


def sinkhorn(lib, B, N, M, grad=False):
    g = _g(19)
    eps = _cf(_EPS)
    floats = (lib.fpsg_sinkhorn_grad_workspace_floats if grad else lib.fpsg_sinkhorn_workspace_floats)(B, N, M)
    bufs = [inp("x", _rand(g, B, N, 3)), inp("y", _rand(g, B, M, 3)), out("out", F32, (B,)), _W(floats, 4, 4)]
    if grad:
        bufs += [out("gx", F32, (B, N, 3)), out("gy", F32, (B, M, 3))]

        def call(p, s, wsn):
            return lib.fpsg_sinkhorn_divergence_grad(p["x"], p["y"], B, N, M, eps, len(_EPS), p["out"], p["gx"], p["gy"],
                                                     p["ws"], s)
    else:
        def call(p, s, wsn):
            return lib.fpsg_sinkhorn_divergence(p["x"], p["y"], B, N, M, eps, len(_EPS), p["out"], p["ws"], s)
    return Row(bufs, call, floats)


# ---- K12 / K14 --------------------------------------------------------------------------------------------------------
def emd_exact(lib, B, N, grads):
    g = _g(12)
    floats = lib.fpsg_emd_exact_workspace_floats(B, N)
    bufs = [inp("xyz1", _rand(g, B, N, 3)), inp("xyz2", _rand(g, B, N, 3)), out("cost", F32, (B,)), out("gap", F32, (B,)),
            out("assign", I32, (B, N)), out("status", I32, (B,)), _W(floats, 4, 4)]
    if grads:
        bufs += [out("gxyz1", F32, (B, N, 3)), out("gxyz2", F32, (B, N, 3))]

    def call(p, s, wsn):
        return lib.fpsg_emd_exact(p["xyz1"], p["xyz2"], B, N, _f(0.01), 100000, p["cost"], p["gap"], p["assign"],
                                  p["status"], p.get("gxyz1"), p.get("gxyz2"), p["ws"], s)
    return Row(bufs, call, floats)


def emd_cross(lib, Na, Nb, N, sym):
    g = _g(14)
    nbytes = lib.fpsg_emd_cross_workspace_bytes(Na, Nb, N)
    bufs = [inp("xyz1", _rand(g, Na, N, 3))]
    if not sym:
        bufs.append(inp("xyz2", _rand(g, Nb, N, 3)))
    bufs += [out("cost", F32, (Na, Nb)), out("gap", F32, (Na, Nb)), out("status", I32, (Na, Nb)),
             out("rounds", I32, (Na, Nb)), _W(nbytes, 1, 8)]        # "bytes, 8-byte aligned"

    def call(p, s, wsn):
        return lib.fpsg_emd_cross(p["xyz1"], p.get("xyz2"), Na, Nb, N, _f(0.01), 100000, p["cost"], p["gap"], p["status"],
                                  p["rounds"], p["ws"], wsn, s)
    return Row(bufs, call, nbytes, size_arg=True, refuses=True)


# ---- K15 / K16: "No workspace: ... returns 0 and ws may be NULL" -----------------------------------------------------
def occupancy(lib, S, N, res, in_sphere):
    g = _g(15)
    nbytes = lib.fpsg_occupancy_grid_workspace_bytes(S, N, res)
    why = "K15: 'Outputs, all int32 and all ACCUMULATED INTO'"
    bufs = [inp("xyz", _rand(g, S, N, 3) * 1.2 - 0.6),
            inout("counts", _randint(g, 0, 5, res ** 3), why=why), inout("clouds_hit", _randint(g, 0, 5, res ** 3), why=why),
            inout("outside", _randint(g, 0, 5, 3), why=why), out("cells", I32, (S, N)), _W(nbytes, 1, 4)]

    def call(p, s, wsn):
        return lib.fpsg_occupancy_grid(p["xyz"], S, N, res, _f(0.5), in_sphere, p["counts"], p["clouds_hit"], p["outside"],
                                       p["cells"], p["ws"], wsn, s)
    return Row(bufs, call, nbytes, size_arg=True, needs_ws=False)


def fps(lib, B, N, n):
    g = _g(16)
    nbytes = lib.fpsg_fps_workspace_bytes(B, N, n)
    bufs = [inp("xyz", _rand(g, B, N, 3)), inp("start", _randint(g, 0, N, B)), out("idx", I32, (B, n)),
            out("min_dist", F32, (B, n)), _W(nbytes, 1, 4)]

    def call(p, s, wsn):
        return lib.fpsg_fps(p["xyz"], B, N, n, p["start"], p["idx"], p["min_dist"], p["ws"], wsn, s)
    return Row(bufs, call, nbytes, size_arg=True, needs_ws=False)


# ---- K21 / K22 / K24 / K25 --------------------------------------------------------------------------------------------
def _self_knn_cpu(xyz, k):
    """Neighbour lists for the backward rows (any table is valid input there): nearest first, self skipped."""
    d = ((xyz[:, :, None, :] - xyz[:, None, :, :]) ** 2).sum(-1)
    n = xyz.shape[1]
    d[:, torch.arange(n), torch.arange(n)] = float("inf")
    d2, idx = torch.sort(d, dim=-1, stable=True)
    return idx[..., :k].to(I32).contiguous(), d2[..., :k].contiguous()


def repulsion_fwd(lib, B, N, k):
    g = _g(21)
    nbytes = lib.fpsg_repulsion_workspace_bytes(B, N, k)
    bufs = [inp("xyz", _rand(g, B, N, 3)), out("nbr_idx", I32, (B, N, k)), out("nbr_d2", F32, (B, N, k)),
            out("value", F32, (B,)), _W(nbytes, 1, 4)]

    def call(p, s, wsn):
        return lib.fpsg_repulsion_fwd(p["xyz"], B, N, k, _f(0.07), p["nbr_idx"], p["nbr_d2"], p["value"], p["ws"], wsn, s)
    return Row(bufs, call, nbytes, size_arg=True, refuses=True)


def repulsion_bwd(lib, B, N, k):
    g = _g(21)
    xyz = _rand(g, B, N, 3)
    idx, d2 = _self_knn_cpu(xyz, k)
    bufs = [inp("xyz", xyz), inp("nbr_idx", idx), inp("nbr_d2", d2), inp("gvalue", _randn(g, B)), out("gxyz", F32, (B, N, 3))]

    def call(p, s, wsn):
        return lib.fpsg_repulsion_bwd(p["xyz"], p["nbr_idx"], p["nbr_d2"], p["gvalue"], B, N, k, _f(0.07), p["gxyz"], s)
    return Row(bufs, call, needs_ws=False)


def swd(lib, B, N, L):
    g = _g(22)
    nbytes = lib.fpsg_swd_workspace_bytes(B, N, L)
    bufs = [inp("xyz1", _randn(g, B, N, 3)), inp("xyz2", _randn(g, B, N, 3)), inp("dirs", _randn(g, L, 3)),
            out("value", F32, (B,)), out("gxyz1", F32, (B, N, 3)), out("gxyz2", F32, (B, N, 3)),
            out("perm1", I32, (B, L, N)), out("perm2", I32, (B, L, N)), _W(nbytes, 1, 4)]   # "bytes, 4-byte aligned"

    def call(p, s, wsn):
        return lib.fpsg_swd(p["xyz1"], p["xyz2"], p["dirs"], B, N, L, p["value"], p["gxyz1"], p["gxyz2"], p["perm1"],
                            p["perm2"], p["ws"], wsn, s)
    return Row(bufs, call, nbytes, size_arg=True, refuses=True)


def expansion_fwd(lib, B, N, P):
    g = _g(24)
    nbytes = lib.fpsg_expansion_workspace_bytes(B, N, P)
    bufs = [inp("xyz", _rand(g, B, N, 3)), out("parent", I32, (B, N)), out("edge_d2", F32, (B, N)), out("order", I32, (B, N)),
            out("mean_len", F32, (B, N // P)), out("value", F32, (B,)), _W(nbytes, 1, 4)]

    def call(p, s, wsn):
        return lib.fpsg_expansion_fwd(p["xyz"], B, N, P, _f(1.5), p["parent"], p["edge_d2"], p["order"], p["mean_len"],
                                      p["value"], p["ws"], wsn, s)
    return Row(bufs, call, nbytes, size_arg=True, refuses=True)


def expansion_bwd(lib, B, N, P):
    g = _g(24)
    xyz = _rand(g, B, N, 3)
    # a star per patch: every vertex hangs on local vertex 0 (the backward is "safe on any int32 / fp32 arrays")
    parent = torch.zeros(B, N, dtype=I32)
    parent[:, ::P] = -1
    root = xyz.view(B, N // P, P, 3)[:, :, :1, :]
    d2 = ((xyz.view(B, N // P, P, 3) - root) ** 2).sum(-1).reshape(B, N).contiguous()
    mean_len = d2.sqrt().view(B, N // P, P).sum(-1) / (P - 1)
    bufs = [inp("xyz", xyz), inp("parent", parent), inp("edge_d2", d2), inp("mean_len", mean_len.contiguous()),
            inp("gvalue", _randn(g, B)), out("gxyz", F32, (B, N, 3))]

    def call(p, s, wsn):
        return lib.fpsg_expansion_bwd(p["xyz"], p["parent"], p["edge_d2"], p["mean_len"], p["gvalue"], B, N, P, _f(1.0),
                                      p["gxyz"], s)
    return Row(bufs, call, needs_ws=False)


def uniform_fwd(lib, B, N, S, T, cap):
    g = _g(25)
    percent = _cf([0.9, 0.3, 0.6, 0.1][:T])            # 0.9: more members than the cap of retained ones
    nbytes = lib.fpsg_uniform_workspace_bytes(B, N, S, T, cap)
    seeds = torch.stack([torch.randperm(N, generator=g)[:S] for _ in range(B)]).to(I32)
    bufs = [inp("xyz", _rand(g, B, N, 3)), inp("seeds", seeds), out("count", I32, (B, T, S)),
            out("member", I32, (B, T, S, cap)), out("nn", I32, (B, T, S, cap)), out("nn_d2", F32, (B, T, S, cap)),
            out("ball_value", F32, (B, T, S)), out("per_percent", F32, (B, T)), out("value", F32, (B,)), _W(nbytes, 1, 4)]

    def call(p, s, wsn):
        return lib.fpsg_uniform_fwd(p["xyz"], p["seeds"], B, N, S, percent, T, _f(1.0), cap, p["count"], p["member"],
                                    p["nn"], p["nn_d2"], p["ball_value"], p["per_percent"], p["value"], p["ws"], wsn, s)
    return Row(bufs, call, nbytes, size_arg=True, refuses=True)


def uniform_bwd(lib, B, N, S, T, cap):
    g = _g(25)
    percent_l = [0.9, 0.3, 0.6, 0.1][:T]
    percent = _cf(percent_l)
    xyz = _rand(g, B, N, 3)
    seeds = torch.stack([torch.randperm(N, generator=g)[:S] for _ in range(B)]).to(I32)
    # the forward's lists by its definition (fp32 sums in another order: the backward re-derives membership itself and is
    # "safe on any int32 / fp32 contents")
    count = torch.zeros(B, T, S, dtype=I32)
    member = torch.full((B, T, S, cap), -1, dtype=I32)
    nn = torch.full((B, T, S, cap), -1, dtype=I32)
    nn_d2 = torch.full((B, T, S, cap), float("inf"), dtype=F32)
    for b in range(B):
        d = ((xyz[b][:, None, :] - xyz[b][None, :, :]) ** 2).sum(-1)
        for t in range(T):
            for j in range(S):
                ins = torch.nonzero(d[:, int(seeds[b, j])] <= percent_l[t]).flatten()
                count[b, t, j] = ins.numel()
                m = ins[:cap]
                member[b, t, j, :m.numel()] = m.to(I32)
                if m.numel() > 1:
                    dd = d[m][:, m].clone()
                    dd.fill_diagonal_(float("inf"))
                    v, a = dd.min(dim=1)
                    nn[b, t, j, :m.numel()] = m[a].to(I32)
                    nn_d2[b, t, j, :m.numel()] = v
    bufs = [inp("xyz", xyz), inp("seeds", seeds), inp("count", count), inp("member", member), inp("nn", nn),
            inp("nn_d2", nn_d2), inp("gvalue", _randn(g, B)), out("gxyz", F32, (B, N, 3))]

    def call(p, s, wsn):
        return lib.fpsg_uniform_bwd(p["xyz"], p["seeds"], p["count"], p["member"], p["nn"], p["nn_d2"], p["gvalue"], B, N, S,
                                    T, percent, _f(1.0), cap, p["gxyz"], s)
    return Row(bufs, call, needs_ws=False)


# ---- K4b ------------------------------------------------------------------------------------------------------------
def edgeconv_stats_ws(lib, blocks, Co):
    g = _g(4)
    floats = lib.fpsg_edgeconv_stats_ws_floats(blocks, Co)
    part = _randn(g, blocks, 2, Co)
    part[:, 1] = part[:, 1].abs() * 8 + 4                      # sums of squares: a positive variance
    why = "K4b: 'updates the running statistics as nn.BatchNorm2d does'"
    # "Co must be 64, 128 or 256; float buffers 16-byte aligned"; ws "floats, 8-byte aligned"
    bufs = [inp("part", part, 16), inp("gamma", _randn(g, Co), 16), inp("beta", _randn(g, Co), 16),
            inout("running_mean", _randn(g, Co), 16, why), inout("running_var", _rand(g, Co) + 0.5, 16, why),
            out("chan", F32, (4, Co), 16), _W(floats, 4, 8)]

    def call(p, s, wsn):
        return lib.fpsg_edgeconv_stats_finalize_ws(p["part"], blocks, p["gamma"], p["beta"], p["running_mean"],
                                                   p["running_var"], _f(0.1), _f(1e-5), ctypes.c_double(blocks * 4.0), Co, 1,
                                                   p["chan"], p["ws"], s)
    return Row(bufs, call, floats)


# ---- K5 -------------------------------------------------------------------------------------------------------------
_RUN = "K5: 'running_mean / running_var [C] (optional) are then updated in place'"


def _bn_common(g, N, C, L):
    return [inp("x", _randn(g, N, C, L), 16), inp("pre_bias", _randn(g, C)), inp("gamma", _randn(g, C)),
            inp("beta", _randn(g, C)), inout("running_mean", _randn(g, C), why=_RUN),
            inout("running_var", _rand(g, C) + 0.5, why=_RUN)]


def _chan(g, C):
    c = _randn(g, 4, C)
    c[3] = c[3].abs() + 0.5                                     # rstd
    return c


def bn_act_fwd(lib, N, C, L, training):
    g = _g(5)
    floats = lib.fpsg_bn_workspace_floats(N, C, L)
    bufs = _bn_common(g, N, C, L) + [out("y", F32, (N, C, L), 16), out("chan", F32, (4, C)), _W(floats, 4, 4)]
    if training == 1:
        bufs += [out("batch_mean", F32, (C,)), out("batch_var", F32, (C,))]
    else:                                                       # evaluation: the running statistics are inputs
        bufs = [inp(b.name, b.data, b.align) if b.role == "inout" else b for b in bufs]
    if training == 2:                                           # "evaluation mode with chan ALREADY holding the coefficients"
        bufs = [inp("chan", _chan(g, C)) if b.name == "chan" else b for b in bufs]

    def call(p, s, wsn):
        return lib.fpsg_bn_act_fwd(p["x"], p["pre_bias"], p["gamma"], p["beta"], p["running_mean"], p["running_var"],
                                   _f(0.1), N, C, L, training, _f(1e-5), 2, _f(0.2), p["y"], p["chan"], p.get("batch_mean"),
                                   p.get("batch_var"), p["ws"], s)
    return Row(bufs, call, floats)


def _parts(g, C, n_parts, count):
    """[C][n_parts][2] partial sums (sum, sum of squares) of a positive variance."""
    parts = _randn(g, C, n_parts, 2) * 0.1
    parts[..., 1] = parts[..., 1].abs() + 2.0 * count / n_parts
    return parts


def bn_stats(lib, N, C, L, n_parts=0):
    g = _g(5)
    floats = lib.fpsg_bn_workspace_floats(N, C, L)
    bufs = _bn_common(g, N, C, L) + [out("chan", F32, (4, C)), out("batch_mean", F32, (C,)), out("batch_var", F32, (C,)),
                                     _W(floats, 4, 4)]
    if n_parts:                                                 # the producing convolution's sums: no pass over x
        bufs.append(inp("parts", _parts(g, C, n_parts, N * L)))

    def call(p, s, wsn):
        return lib.fpsg_bn_stats(p["x"], p["pre_bias"], p["gamma"], p["beta"], p["running_mean"], p["running_var"], _f(0.1),
                                 N, C, L, 1, _f(1e-5), p["chan"], p["batch_mean"], p["batch_var"], p["ws"], p.get("parts"), n_parts, s)
    return Row(bufs, call, floats)


def _bn_bwd_in(g, N, C, L):
    return [inp("x", _randn(g, N, C, L), 16), inp("pre_bias", _randn(g, C)), inp("dy", _randn(g, N, C, L), 16),
            inp("chan", _chan(g, C))]


def bn_act_bwd(lib, N, C, L):
    g = _g(6)
    floats = lib.fpsg_bn_workspace_floats(N, C, L)
    # "coef [3][C] scratch": contents unspecified, like the workspace (the one-launch path never writes it)
    bufs = _bn_bwd_in(g, N, C, L) + [out("dx", F32, (N, C, L), 16), out("dgamma", F32, (C,)), out("dbeta", F32, (C,)),
                                     out("dpre_bias", F32, (C,)), ws_buf("coef", 3 * C * 4, 4), _W(floats, 4, 4)]

    def call(p, s, wsn):
        return lib.fpsg_bn_act_bwd(p["x"], p["pre_bias"], p["dy"], p["chan"], N, C, L, 1, 1, _f(0.0), p["dx"], p["dgamma"],
                                   p["dbeta"], p["dpre_bias"], p["coef"], p["ws"], s)
    return Row(bufs, call, floats)


def bn_act_bwd_coef(lib, N, C, L):
    g = _g(6)
    floats = lib.fpsg_bn_workspace_floats(N, C, L)
    bufs = _bn_bwd_in(g, N, C, L) + [out("dgamma", F32, (C,)), out("dbeta", F32, (C,)), out("coef", F32, (3, C)),
                                     _W(floats, 4, 4)]

    def call(p, s, wsn):
        return lib.fpsg_bn_act_bwd_coef(p["x"], p["pre_bias"], p["dy"], p["chan"], N, C, L, 1, 1, _f(0.0), p["dgamma"],
                                        p["dbeta"], p["coef"], p["ws"], s)
    return Row(bufs, call, floats)


def bn_act_bwd_parts(lib, N, C, L, n_parts=3, act=1):
    g = _g(6)
    floats = lib.fpsg_bn_workspace_floats(N, C, L)
    bufs = _bn_bwd_in(g, N, C, L) + [inp("parts", _randn(g, C, n_parts, 2)), out("dx", F32, (N, C, L), 16),
                                     out("dgamma", F32, (C,)), out("dbeta", F32, (C,)), out("dpre_bias", F32, (C,)),
                                     out("coef", F32, (3, C)), _W(floats, 4, 4)]

    def call(p, s, wsn):
        return lib.fpsg_bn_act_bwd_parts(p["x"], p["pre_bias"], p["dy"], p["chan"], N, C, L, 1, act,
                                         _f(0.2 if act == 2 else 0.0), p["dx"], p["dgamma"], p["dbeta"], p["dpre_bias"],
                                         p["coef"], p["ws"], p["parts"], n_parts, s)
    return Row(bufs, call, floats)


def bn_pool_fwd(lib, N, C, H, W, n_parts=0):
    g = _g(7)
    floats = lib.fpsg_bn_pool_workspace_floats(N, C, H, W)
    bufs = _bn_common(g, N, C, H * W) + [out("y_pooled", F32, (N, C, H // 2, W // 2), 16), out("chan", F32, (4, C)),
                                         out("batch_mean", F32, (C,)), out("batch_var", F32, (C,)), _W(floats, 4, 4)]
    if n_parts:
        bufs.append(inp("parts", _parts(g, C, n_parts, N * H * W)))

    def call(p, s, wsn):
        return lib.fpsg_bn_act_pool_fwd(p["x"], p["pre_bias"], p["gamma"], p["beta"], p["running_mean"], p["running_var"],
                                        _f(0.1), N, C, H, W, 1, _f(1e-5), 1, _f(0.0), p["y_pooled"], p["chan"],
                                        p["batch_mean"], p["batch_var"], p["ws"], p.get("parts"), n_parts, s)
    return Row(bufs, call, floats)


def bn_pool_bwd(lib, N, C, H, W):
    g = _g(7)
    floats = lib.fpsg_bn_pool_workspace_floats(N, C, H, W)
    bufs = [inp("x", _randn(g, N, C, H, W), 16), inp("pre_bias", _randn(g, C)),
            inp("dy_pooled", _randn(g, N, C, H // 2, W // 2), 16), inp("chan", _chan(g, C)),
            out("dx", F32, (N, C, H, W), 16), out("dgamma", F32, (C,)), out("dbeta", F32, (C,)), out("dpre_bias", F32, (C,)),
            out("coef", F32, (3, C)), _W(floats, 4, 4)]

    def call(p, s, wsn):
        return lib.fpsg_bn_act_pool_bwd(p["x"], p["pre_bias"], p["dy_pooled"], p["chan"], N, C, H, W, 1, 1, _f(0.0), p["dx"],
                                        p["dgamma"], p["dbeta"], p["dpre_bias"], p["coef"], p["ws"], s)
    return Row(bufs, call, floats)


def bn_max_fwd(lib, N, C, L):
    g = _g(8)
    floats = lib.fpsg_bn_max_workspace_floats(N, C, L)
    bufs = _bn_common(g, N, C, L) + [out("out", F32, (N, C)), out("idx", I32, (N, C)), out("chan", F32, (4, C)),
                                     out("batch_mean", F32, (C,)), out("batch_var", F32, (C,)), _W(floats, 4, 4)]

    def call(p, s, wsn):
        return lib.fpsg_bn_act_max_fwd(p["x"], p["pre_bias"], p["gamma"], p["beta"], p["running_mean"], p["running_var"],
                                       _f(0.1), N, C, L, 1, _f(1e-5), 1, _f(0.0), p["out"], p["idx"], p["chan"],
                                       p["batch_mean"], p["batch_var"], p["ws"], s)
    return Row(bufs, call, floats)


def bn_max_bwd(lib, N, C, L, coef_only=False):
    g = _g(8)
    floats = lib.fpsg_bn_max_workspace_floats(N, C, L)
    bufs = [inp("x", _randn(g, N, C, L), 16), inp("pre_bias", _randn(g, C)), inp("gout", _randn(g, N, C)),
            inp("idx", _randint(g, 0, L, N, C)), inp("chan", _chan(g, C)), out("dgamma", F32, (C,)), out("dbeta", F32, (C,)),
            out("coef", F32, (3, C)), _W(floats, 4, 4)]
    if coef_only:
        def call(p, s, wsn):
            return lib.fpsg_bn_act_max_bwd_coef(p["x"], p["pre_bias"], p["gout"], p["idx"], p["chan"], N, C, L, 1, 1, _f(0.0),
                                                p["dgamma"], p["dbeta"], p["coef"], p["ws"], s)
    else:
        bufs += [out("dx", F32, (N, C, L), 16), out("dpre_bias", F32, (C,))]

        def call(p, s, wsn):
            return lib.fpsg_bn_act_max_bwd(p["x"], p["pre_bias"], p["gout"], p["idx"], p["chan"], N, C, L, 1, 1, _f(0.0),
                                           p["dx"], p["dgamma"], p["dbeta"], p["dpre_bias"], p["coef"], p["ws"], s)
    return Row(bufs, call, floats)


# ---- K6w / K8 -------------------------------------------------------------------------------------------------------
def wino_dw_fused(lib, N, K, H, W, act):
    g = _g(60)
    floats = lib.fpsg_wino_dw_fused_workspace_floats(N, K, H, W)
    bufs = [inp("x", _randn(g, N, 64, H, W), 16), inp("dy", _randn(g, N, K, H, W), 16), out("dU", F32, (36, K, 64)),
            _W(floats, 4, 4)]
    if act:
        bufs += [inp("chan", _chan(g, 64)), inp("pre_bias", _randn(g, 64))]

    def call(p, s, wsn):
        return lib.fpsg_wino_dw_fused(p["x"], p.get("chan"), p.get("pre_bias"), p["dy"], N, 64, K, H, W, p["dU"], p["ws"], s)
    return Row(bufs, call, floats)


def conv_first_dw(lib, N, H, W, fold):
    g = _g(80)
    floats = lib.fpsg_conv_first_dw_workspace_floats(N, H, W)
    bufs = [inp("x", _randn(g, N, 3, H, W)), out("dw", F32, (64, 3, 3, 3)), _W(floats, 4, 4)]
    if fold:
        bufs += [inp("y", _randn(g, N, 64, H, W), 16), inp("ga", _randn(g, N, 64, H, W), 16), inp("chan", _chan(g, 64)),
                 inp("coef", _randn(g, 3, 64)), inp("pre_bias", _randn(g, 64))]

        def call(p, s, wsn):
            return lib.fpsg_conv_first_dw_fold(p["x"], p["y"], p["ga"], p["chan"], p["coef"], p["pre_bias"], N, 3, 64, H, W,
                                               p["dw"], p["ws"], s)
    else:
        bufs.append(inp("dy", _randn(g, N, 64, H, W), 16))

        def call(p, s, wsn):
            return lib.fpsg_conv_first_dw(p["x"], p["dy"], N, 3, 64, H, W, p["dw"], p["ws"], s)
    return Row(bufs, call, floats)


# ---- K10 ------------------------------------------------------------------------------------------------------------
def gemm_split(lib, batch, M, N, K, transB, variant):
    g = _g(10)
    floats = lib.fpsg_gemm_split_workspace_floats(batch, M, N, K, transB, variant)
    Bm = _randn(g, batch, N, K) if transB else _randn(g, batch, K, N)
    bufs = [inp("A", _randn(g, batch, M, K)), inp("B", Bm), out("C", F32, (batch, M, N)), _W(floats, 4, 4)]

    def call(p, s, wsn):
        return lib.fpsg_gemm_split(p["A"], p["B"], p["C"], batch, M, N, K, K, K if transB else N, N, M * K, N * K, M * N,
                                   transB, variant, p["ws"], wsn, s)
    return Row(bufs, call, floats, size_arg=True, needs_ws=False)   # "0 when the reduction is not split; then ws may be NULL"


# ---- K20 ------------------------------------------------------------------------------------------------------------
_STATS = "K20: 'stats (optional, double[4], updated in place by plain loads and stores'"


def grad_clip(lib, n):
    g = _g(20)
    nbytes = lib.fpsg_grad_norm_workspace_bytes(n)
    bufs = [inp("grad", _randn(g, n), 16), out("out2", F32, (2,)),
            inout("stats", torch.tensor([3.0, 1.0, 0.0, 0.5], dtype=F64), 8, _STATS), _W(nbytes, 1, 8)]

    def call(p, s, wsn):
        return lib.fpsg_grad_clip_scale(p["grad"], n, _f(0.5), _f(1.0), p["ws"], wsn, p["out2"], p["stats"], s)
    return Row(bufs, call, nbytes, size_arg=True, refuses=True)


def grad_clip_segments(lib, sizes):
    """sizes: elements per segment, negative = a segment of that length without gradient (NULL = zeros).  The gradient tensors "may start at any
    4-byte address"."""
    g = _g(20)
    n = sum(abs(v) for v in sizes)
    nbytes = lib.fpsg_grad_norm_workspace_bytes(n)
    off = [0]
    for v in sizes:
        off.append(off[-1] + abs(v))
    bufs = [inp(f"g{i}", _randn(g, v)) for i, v in enumerate(sizes) if v > 0]
    bufs += [inp("grad_ptrs", torch.zeros(len(sizes), dtype=I64), 8), inp("seg_off", torch.tensor(off, dtype=I64), 8),
             out("out2", F32, (2,)), inout("stats", torch.tensor([3.0, 1.0, 0.0, 0.5], dtype=F64), 8, _STATS),
             _W(nbytes, 1, 8)]

    def late(p):
        return {"grad_ptrs": torch.tensor([p[f"g{i}"] if v > 0 else 0 for i, v in enumerate(sizes)], dtype=I64)}

    def call(p, s, wsn):
        return lib.fpsg_grad_clip_scale_segments(p["grad_ptrs"], p["seg_off"], len(sizes), n, _f(0.5), _f(1.0), p["ws"], wsn,
                                                 p["out2"], p["stats"], s)
    return Row(bufs, call, nbytes, size_arg=True, refuses=True, late=late)


# ---- K26 ------------------------------------------------------------------------------------------------------------
def mesh_cdf(lib, V, F):
    g = _g(26)
    nbytes = lib.fpsg_mesh_cdf_workspace_bytes(V, F)
    faces = _randint(g, 0, V, F, 3)
    if F > 2:
        faces[1, 2] = V + 5                                         # "a vertex index outside [0, V) has area 0"
    bufs = [inp("verts", _randn(g, V, 3)), inp("faces", faces), out("cdf", I64, (F,), 8), _W(nbytes, 1, 8)]

    def call(p, s, wsn):
        return lib.fpsg_mesh_cdf(p["verts"], V, p["faces"], F, p["cdf"], p["ws"], wsn, s)
    return Row(bufs, call, nbytes, size_arg=True, refuses=True)


# ---- K27 / K28 / K29 / K31 --------------------------------------------------------------------------------------------
def _views(g, n):
    """n cameras on the -z side, turned about the y axis: right, up, forward, position."""
    rows = []
    for i in range(n):
        a = 0.4 * i
        r, u, f = (math.cos(a), 0.0, -math.sin(a)), (0.0, 1.0, 0.0), (math.sin(a), 0.0, math.cos(a))
        rows.append([*r, *u, *f, *[-2.0 * v for v in f]])
    return torch.tensor(rows, dtype=F32)


_PARAMS = [0.1, 0.1, 0.1, 0.6, 0.5, 0.4, 0.3, 0.3, 0.3, 0.3, 0.4, -0.86, 0.2, 0.3, 0.4, 0.25, 0.75]


def _mesh(g, V, F):
    verts = _rand(g, V, 3) - 0.5
    faces = _randint(g, 0, V, F, 3)
    if F >= 3:
        verts[:3] = torch.tensor([[-0.7, -0.7, 0.1], [0.7, -0.7, 0.2], [0.0, 0.7, 0.3]])   # one triangle beyond the
        faces[0] = torch.tensor([0, 1, 2], dtype=I32)                                      # 64-pixel small box
        faces[F - 1, 1] = V                                                               # an index outside [0, V)
    return verts, faces


def _render_outs(lead, H, W, ssaa, id_name):
    return [out("image", U8, (*lead, H // ssaa, W // ssaa, 3)), out("radiance", F32, (*lead, H // ssaa, W // ssaa, 3)),
            out(id_name, I32, (*lead, H, W)), out("depth", F32, (*lead, H, W))]


def mesh_render(lib, V, F, nv, W, H, ssaa, form="plain", bg=False):
    g = _g(27)
    verts, faces = _mesh(g, V, F)
    M, T = (2, 1) if form != "plain" else (0, 0)
    tex_w, tex_h = 5, 3
    if form == "plain":
        nbytes = lib.fpsg_mesh_render_workspace_bytes(V, F, nv, W, H)
    elif form == "materials":
        nbytes = lib.fpsg_mesh_render_materials_workspace_bytes(V, F, nv, W, H, M, T)
    else:
        nbytes = lib.fpsg_mesh_render_smooth_workspace_bytes(V, F, nv, W, H, M, T)
    params = _cf(_PARAMS[:15] if form == "plain" else _PARAMS)
    bufs = [inp("verts", verts), inp("faces", faces), inp("views", _views(g, nv))]
    bufs += _render_outs((nv,), H, W, ssaa, "face_id") + [_W(nbytes, 1, 16)]            # "(16-byte aligned)"
    if bg:
        bufs.append(inp("bg_image", torch.randint(0, 256, (H // ssaa, W // ssaa, 3), generator=g, dtype=U8)))
    if form != "plain":
        materials = _cf([0.8, 0.2, 0.1, -1.0, 0.1, 0.9, 0.3, 0.0])                       # Kd + texture index per material
        tex_table = (ctypes.c_int32 * 3)(0, tex_w, tex_h)
        bufs += [inp("face_material", _randint(g, -1, M + 1, F)), inp("face_uv", _rand(g, F, 3, 2) * 3 - 1),
                 inp("texels", torch.randint(0, 256, (tex_w * tex_h, 3), generator=g, dtype=U8))]
    if form == "smooth":
        bufs.append(inp("face_normals", _randn(g, F, 3, 3)))

    def call(p, s, wsn):
        tail = (p["views"], nv, W, H, ssaa, _f(1.5), params, 3, p.get("bg_image"), p["image"], p["radiance"], p["face_id"],
                p["depth"], p["ws"], wsn, s)
        if form == "plain":
            return lib.fpsg_mesh_render(p["verts"], V, p["faces"], F, *tail)
        if form == "materials":
            return lib.fpsg_mesh_render_materials(p["verts"], V, p["faces"], F, p["face_material"], p["face_uv"], materials,
                                                  M, tex_table, T, p["texels"], tex_w * tex_h, *tail)
        return lib.fpsg_mesh_render_smooth(p["verts"], V, p["faces"], F, p["face_material"], p["face_uv"],
                                           p["face_normals"], materials, M, tex_table, T, p["texels"], tex_w * tex_h, *tail)
    return Row(bufs, call, nbytes, size_arg=True, refuses=True)


def points_render(lib, B, N, nv, W, H, ssaa, colors):
    g = _g(29)
    nbytes = lib.fpsg_points_render_workspace_bytes(B, N, nv, W, H)
    params = _cf(_PARAMS)
    bufs = [inp("points", _rand(g, B, N, 3) - 0.5), inp("views", _views(g, nv))]
    bufs += _render_outs((B, nv), H, W, ssaa, "point_id") + [_W(nbytes, 1, 16)]         # "(16-byte aligned)"
    if colors:
        bufs.append(inp("colors", torch.randint(0, 256, (B, N, 3), generator=g, dtype=U8)))
    radius = 1.5 * 3.0 / max(W, H)                                  # three samples: R = 768 snapped units

    def call(p, s, wsn):
        return lib.fpsg_points_render(p["points"], p.get("colors"), B, N, p["views"], nv, W, H, ssaa, _f(1.5), _f(radius),
                                      params, 3, None, p["image"], p["radiance"], p["point_id"], p["depth"], p["ws"], wsn, s)
    return Row(bufs, call, nbytes, size_arg=True, refuses=True)


# ---- K32 / K33 --------------------------------------------------------------------------------------------------------
def point_mesh(lib, B, N, V, F, per_mesh, chunks):
    g = _g(32)
    nbytes = lib.fpsg_point_mesh_workspace_bytes(B, N, F, chunks)
    verts = _rand(g, B, V, 3) if per_mesh else _rand(g, V, 3)
    faces = _randint(g, 0, V, F, 3)
    if F > 2:
        faces[F - 1, 0] = -1                                        # "a face with an index outside is skipped"
    bufs = [inp("points", _rand(g, B, N, 3)), inp("verts", verts), inp("faces", faces), out("dist2", F32, (B, N)),
            out("face", I32, (B, N)), out("closest", F32, (B, N, 3)), out("bary", F32, (B, N, 3)),
            _W(nbytes, 1, 8)]                                       # "bytes, 8-byte aligned"

    def call(p, s, wsn):
        return lib.fpsg_point_mesh_distance(p["points"], B, N, p["verts"], V, per_mesh, p["faces"], F, chunks, p["dist2"],
                                            p["face"], p["closest"], p["bary"], p["ws"], wsn, s)
    return Row(bufs, call, nbytes, size_arg=True, refuses=True)


def point_normals(lib, B, N, k, sign_mode, lists):
    g = _g(33)
    nbytes = lib.fpsg_point_normals_workspace_bytes(B, N, k)
    bufs = [inp("xyz", _rand(g, B, N, 3)), inp("ref", _randn(g, B, 3)), out("normals", F32, (B, N, 3)),
            out("variation", F32, (B, N)), _W(nbytes, 1, 4)]
    if lists:
        bufs.append(out("nbr_idx", I32, (B, N, k)))

    def call(p, s, wsn):
        return lib.fpsg_point_normals(p["xyz"], B, N, k, sign_mode, p["ref"], p["normals"], p["variation"], p.get("nbr_idx"),
                                      p["ws"], wsn, s)
    return Row(bufs, call, nbytes, size_arg=True, refuses=True)


def point_normals_orient(lib, B, N, k, axis):
    g = _g(34)
    nbytes = lib.fpsg_point_normals_orient_workspace_bytes(B, N, k)
    nbr = _randint(g, 0, N, B, N, k)                                 # "K33a's, or any table"
    nbr[:, 0, 0] = N + 3                                             # "an entry outside [0, N) ... is no edge"
    n_in = torch.nn.functional.normalize(_randn(g, B, N, 3), dim=-1)
    bufs = [inp("xyz", _rand(g, B, N, 3)), inp("normals_in", n_in), inp("nbr_idx", nbr), out("normals_out", F32, (B, N, 3)),
            out("parent", I32, (B, N)), _W(nbytes, 1, 4)]

    def call(p, s, wsn):
        return lib.fpsg_point_normals_orient(p["xyz"], p["normals_in"], p["nbr_idx"], B, N, k, axis, p["normals_out"],
                                             p["parent"], p["ws"], wsn, s)
    return Row(bufs, call, nbytes, size_arg=True, refuses=True)


def _cases():
    c = []

    def add(entry, tag, fn, *args, **kw):
        c.append((f"{entry[5:]}-{tag}", entry, fn, args, kw))

    # K1 (chamfer_tiled.hip): a tile is 64 R rows x 16 W cpw candidates; variant 11 = 256 x 16, 149 = 512 x 576 (the
    # largest); 4096 points a side is the form's limit
    for entry, losses in (("fpsg_chamfer_fwd_tiled", False), ("fpsg_chamfer_fwd_tiled_losses", True)):
        add(entry, "min", chamfer_tiled, 1, 1, 1, 11, losses=losses)
        add(entry, "tile+1", chamfer_tiled, 1, 513, 577, 149, losses=losses)
        add(entry, "limit", chamfer_tiled, 1, 4096, 4095, 149, losses=losses)
        add(entry, "batch3", chamfer_tiled, 3, 257, 33, 11, losses=losses)
        add(entry, "v125-ragged", chamfer_tiled, 2, 600, 170, 125, losses=losses)       # 512 x 160 tiles
        add(entry, "automatic", chamfer_tiled, 8, 2048, 2047, -1, losses=losses)        # the variant the mirror runs
    # K3: streaming kernel (C <= 128, k <= 24): 128 query rows per workgroup (kSRows); score-tile kernel: 16 queries
    # against 2048 candidates at a time
    add("fpsg_knn", "min", knn, 1, 1, 1, 1)
    add("fpsg_knn", "stream-rows+1", knn, 1, 3, 129, 5)
    add("fpsg_knn", "tile-2048+1", knn, 1, 130, 2049, 25)
    add("fpsg_knn", "batch3", knn, 3, 5, 131, 24)
    add("fpsg_knn", "stream-limits", knn, 2, 128, 200, 24)                           # the streaming kernel's largest C and k
    add("fpsg_knn", "tile-limits", knn, 1, 440, 100, 64)                             # the score-tile kernel's
    add("fpsg_knn_ex", "point-major", knn, 3, 6, 131, 7, layout=1, ex=True)
    add("fpsg_knn_ex", "force-tile-pm-copy", knn, 2, 48, 70, 3, flags=1, ex=True)     # C % 16 == 0, 32 < C <= 128
    add("fpsg_knn_ex", "force-slow", knn, 1, 3, 129, 24, flags=2, ex=True)
    # K2 (emd.hip): rows padded to 4 points; 2 owners per wave x 4 waves (4 owners in the forward-only sweeps)
    add("fpsg_emd_approx", "min", emd_approx, 1, 1, 1, True)
    add("fpsg_emd_approx", "wave+1", emd_approx, 1, 65, 257, True)
    add("fpsg_emd_approx", "batch3", emd_approx, 3, 67, 130, False)
    add("fpsg_emd_approx_variant", "separate-4-owners", emd_approx, 3, 67, 130, False, variant=2)
    add("fpsg_emd_approx_variant", "merged", emd_approx, 3, 67, 130, False, variant=1)
    add("fpsg_emd_approx_variant", "auto-grads", emd_approx, 1, 5, 3, True, variant=-1)
    # K2b / K19 (sinkhorn.hip): 64 owners per workgroup pass, kSmTile = 2048 staged points
    for entry, grad in (("fpsg_sinkhorn_divergence", False), ("fpsg_sinkhorn_divergence_grad", True)):
        add(entry, "min", sinkhorn, 1, 1, 1, grad=grad)
        add(entry, "stage-2048+1", sinkhorn, 1, 65, 2049, grad=grad)
        add(entry, "batch3", sinkhorn, 3, 130, 67, grad=grad)
    # K12 (emd_exact.hip): kExThreads = 1024 per pair
    add("fpsg_emd_exact", "min", emd_exact, 1, 1, True)
    add("fpsg_emd_exact", "threads+1", emd_exact, 1, 1025, False)
    add("fpsg_emd_exact", "batch3", emd_exact, 3, 67, True)
    # K14 (emd_cross.hip): the kernel instance changes above N = 256; both modes
    add("fpsg_emd_cross", "min", emd_cross, 1, 1, 1, False)
    add("fpsg_emd_cross", "pairs-257", emd_cross, 2, 3, 257, False)
    add("fpsg_emd_cross", "symmetric", emd_cross, 3, 3, 65, True)
    add("fpsg_emd_cross", "no-rounds", emd_cross, 2, 3, 65, False, drop=("rounds",))          # "when not NULL, rounds"
    # K15 / K16: no workspace (ws NULL, 0 bytes); 256 threads a workgroup
    add("fpsg_occupancy_grid", "min", occupancy, 1, 1, 2, 0)
    add("fpsg_occupancy_grid", "block+1", occupancy, 1, 257, 5, 1)
    add("fpsg_occupancy_grid", "batch3", occupancy, 3, 65, 8, 1)
    add("fpsg_fps", "min", fps, 1, 1, 1)
    add("fpsg_fps", "1024+1", fps, 1, 1025, 17)
    add("fpsg_fps", "batch3", fps, 3, 130, 130)
    add("fpsg_fps", "limit", fps, 1, 16384, 3)
    add("fpsg_fps", "null-start-min_dist", fps, 3, 130, 9, drop=("start", "min_dist"))       # "or NULL" for both
    # K21 (repulsion.hip, self_knn.h): kSelfKnnTile = 1024 candidates per LDS tile, 256 points per workgroup
    for entry, fn in (("fpsg_repulsion_fwd", repulsion_fwd), ("fpsg_repulsion_bwd", repulsion_bwd)):
        add(entry, "min", fn, 1, 2, 1)
        add(entry, "tile-1024+1", fn, 1, 1025, 8)
        add(entry, "batch3", fn, 3, 257, 3)
    # K22 (swd.hip): 8 directions per group, P = power of two >= max(N, 64) sort slots, 2048 points the limit
    add("fpsg_swd", "min", swd, 1, 1, 1)
    add("fpsg_swd", "slots+1", swd, 1, 1025, 9)
    add("fpsg_swd", "limit", swd, 1, 2048, 2)
    add("fpsg_swd", "batch3", swd, 3, 130, 17)
    add("fpsg_swd", "groups-cap", swd, 2, 70, 129)                                   # G = min(ceil(L / 8), 16) = 16
    # "either may be NULL, as may perm1 / perm2: the other outputs keep their bits"
    add("fpsg_swd", "no-perms", swd, 3, 130, 17, drop=("perm1", "perm2"))
    add("fpsg_swd", "value-only", swd, 3, 130, 17, drop=("gxyz1", "gxyz2", "perm1", "perm2"))
    # K24 (expansion.hip): one wave per patch, vertex v = lane + 64 slot
    for entry, fn in (("fpsg_expansion_fwd", expansion_fwd), ("fpsg_expansion_bwd", expansion_bwd)):
        add(entry, "min", fn, 1, 2, 2)
        add(entry, "wave+1", fn, 1, 130, 65)
        add(entry, "batch3", fn, 3, 201, 67)
    add("fpsg_expansion_fwd", "limit-1024", expansion_fwd, 1, 1024, 1024)
    add("fpsg_repulsion_fwd", "two-tiles+1", repulsion_fwd, 2, 2049, 8)
    add("fpsg_uniform_fwd", "cap-256", uniform_fwd, 1, 300, 3, 1, 256)
    # K25 (uniform.hip): 4 (cloud, seed) waves per workgroup, cap = retained members (64 / 128 / 256)
    for entry, fn in (("fpsg_uniform_fwd", uniform_fwd), ("fpsg_uniform_bwd", uniform_bwd)):
        add(entry, "min", fn, 1, 2, 1, 1, 64)
        add(entry, "cap+1", fn, 1, 257, 5, 2, 64)
        add(entry, "batch3", fn, 3, 130, 7, 3, 128)
    # K4b: the two-stage form starts at 256 partial rows; below it the one-launch form runs (ws given, unused)
    add("fpsg_edgeconv_stats_finalize_ws", "one-launch", edgeconv_stats_ws, 255, 64)
    add("fpsg_edgeconv_stats_finalize_ws", "two-stage-256", edgeconv_stats_ws, 256, 64)
    add("fpsg_edgeconv_stats_finalize_ws", "two-stage-ragged", edgeconv_stats_ws, 1027, 128)
    # K5 (bnact.hip): one launch up to kBnSmallMax = 16384 values per channel, slices above; kBnSeg = 4096 floats
    small, seg, over = (3, 5, 67), (5, 3, 4097), (1, 2, 16385)
    for shape, tag in (((1, 1, 1), "min"), (small, "one-launch"), (seg, "sliced-seg+1"), (over, "sliced-16384+1")):
        add("fpsg_bn_act_fwd", tag, bn_act_fwd, *shape, 1)
        add("fpsg_bn_stats", tag, bn_stats, *shape)
        add("fpsg_bn_act_bwd", tag, bn_act_bwd, *shape)
        add("fpsg_bn_act_bwd_parts", tag, bn_act_bwd_parts, *shape)
        add("fpsg_bn_act_max_fwd", tag, bn_max_fwd, *shape)
        add("fpsg_bn_act_max_bwd", tag, bn_max_bwd, *shape)
        add("fpsg_bn_act_max_bwd_coef", tag, bn_max_bwd, *shape, coef_only=True)
    # sliced rows of whole 16-byte vectors (L % 4 == 0): the branch that loads and stores v4f, and the only one whose
    # accesses carry the non-temporal hint in the streaming forms (tests/test_streaming_forms_gpu.py runs these rows on
    # the second build); 4100 = a last segment of ONE vector, 5464 = 1366 vectors: a last trip that fills 86 of 256 lanes
    vec, vec3 = (5, 3, 4100), (3, 2, 5464)
    for shape, tag in ((vec, "sliced-vec-seg+4"), (vec3, "sliced-vec-batch3")):
        add("fpsg_bn_act_fwd", tag, bn_act_fwd, *shape, 1)
        add("fpsg_bn_stats", tag, bn_stats, *shape)
        add("fpsg_bn_act_bwd", tag, bn_act_bwd, *shape)
        add("fpsg_bn_act_bwd_coef", tag, bn_act_bwd_coef, *shape)
        add("fpsg_bn_act_bwd_parts", tag, bn_act_bwd_parts, *shape)
        add("fpsg_bn_act_max_fwd", tag, bn_max_fwd, *shape)
        add("fpsg_bn_act_max_bwd", tag, bn_max_bwd, *shape)
    add("fpsg_bn_act_fwd", "eval-sliced-vec", bn_act_fwd, *vec, 0)
    add("fpsg_bn_act_bwd_parts", "sliced-vec-leaky", bn_act_bwd_parts, *vec, act=2)
    add("fpsg_bn_act_bwd_parts", "sliced-vec-none", bn_act_bwd_parts, *vec, act=0)
    # pooled rows with W % 4 == 0: two windows a lane (16-byte loads, 16-byte dx stores); 68 = 17 vectors a pooled row
    for shape, tag in (((2, 3, 130, 68), "vec-items+1"), ((3, 2, 6, 12), "vec-batch3")):
        add("fpsg_bn_act_pool_fwd", tag, bn_pool_fwd, *shape)
        add("fpsg_bn_act_pool_bwd", tag, bn_pool_bwd, *shape)
    add("fpsg_bn_act_fwd", "eval-one-launch", bn_act_fwd, *small, 0)
    add("fpsg_bn_act_fwd", "eval-sliced", bn_act_fwd, *seg, 0)
    add("fpsg_bn_act_fwd", "chan-given-one-launch", bn_act_fwd, *small, 2)
    add("fpsg_bn_act_fwd", "chan-given-sliced", bn_act_fwd, *seg, 2)
    add("fpsg_bn_stats", "parts", bn_stats, *seg, n_parts=3)
    # "pre_bias [C] (optional, NULL = none)", "dpre_bias ... (optional, NULL = skip)", optional batch statistics
    add("fpsg_bn_act_fwd", "no-pre_bias-one-launch", bn_act_fwd, *small, 1, drop=("pre_bias", "batch_mean", "batch_var"))
    add("fpsg_bn_act_fwd", "no-pre_bias-sliced", bn_act_fwd, *seg, 1, drop=("pre_bias", "batch_mean", "batch_var"))
    add("fpsg_bn_act_bwd", "no-dpre_bias-one-launch", bn_act_bwd, *small, drop=("pre_bias", "dpre_bias"))
    add("fpsg_bn_act_bwd", "no-dpre_bias-sliced", bn_act_bwd, *seg, drop=("pre_bias", "dpre_bias"))
    add("fpsg_bn_act_max_bwd", "no-dpre_bias", bn_max_bwd, *seg, drop=("pre_bias", "dpre_bias"))
    add("fpsg_bn_act_pool_fwd", "parts", bn_pool_fwd, 2, 3, 130, 66, n_parts=5)
    for shape, tag in ((seg, "sliced-seg+1"), (over, "sliced-16384+1"), ((3, 2, 5462), "batch3")):   # N L > 16384 only
        add("fpsg_bn_act_bwd_coef", tag, bn_act_bwd_coef, *shape)
    # pooled form: an item is max(1, 4096 // (2 W)) row pairs
    for shape, tag in (((1, 1, 2, 2), "min"), ((3, 2, 6, 10), "batch3"), ((2, 3, 130, 66), "items+1"),
                       ((1, 2, 4, 4098), "row-pair-over-item")):
        add("fpsg_bn_act_pool_fwd", tag, bn_pool_fwd, *shape)
        add("fpsg_bn_act_pool_bwd", tag, bn_pool_bwd, *shape)
    # K6w: four 4 x 4 tiles of one tile row per MFMA step (W % 16), ranges of >= 32 steps
    add("fpsg_wino_dw_fused", "min", wino_dw_fused, 1, 16, 4, 16, False)
    add("fpsg_wino_dw_fused", "ranges+1", wino_dw_fused, 2, 32, 36, 48, True)        # 2 * 9 * 12 / 4 = 54 steps
    add("fpsg_wino_dw_fused", "batch3", wino_dw_fused, 3, 16, 12, 16, False)
    # K8: row segments of 64 pixels, or 112 where W % 112 == 0
    for entry, fold in (("fpsg_conv_first_dw", False), ("fpsg_conv_first_dw_fold", True)):
        add(entry, "min", conv_first_dw, 1, 1, 4, fold)
        add(entry, "seg-64+4", conv_first_dw, 1, 3, 68, fold)
        add(entry, "seg-112", conv_first_dw, 1, 2, 224, fold)
        add(entry, "batch3", conv_first_dw, 3, 5, 8, fold)
    # K10: tile 5 = 128 x 128 x 16; variant 35 = tile 5, three ranges of the reduction asked for
    add("fpsg_gemm_split", "no-split-null-ws", gemm_split, 1, 1, 1, 1, 0, -1)
    add("fpsg_gemm_split", "split-tile+1", gemm_split, 2, 129, 130, 49, 1, 35)
    add("fpsg_gemm_split", "nn-tile+1", gemm_split, 3, 129, 131, 17, 0, 5)
    for tile in (0, 1, 3, 7):                                                         # the 256-wide tiles, two ranges
        add("fpsg_gemm_split", f"split-tile{tile}", gemm_split, 1, 257, 258, 70, 1, 20 + tile)
    # K20: vector slots of 4, 256 threads, at most 4096 workgroups
    add("fpsg_grad_clip_scale", "min", grad_clip, 1)
    add("fpsg_grad_clip_scale", "block+tail", grad_clip, 1025)
    add("fpsg_grad_clip_scale", "grid-cap+tail", grad_clip, 4 * 256 * 4096 + 5)
    add("fpsg_grad_clip_scale_segments", "min", grad_clip_segments, (1,))
    add("fpsg_grad_clip_scale_segments", "ragged-null", grad_clip_segments, (5, -7, 1025, 3))
    # K26: kScanB = 1024 faces per scan workgroup
    add("fpsg_mesh_cdf", "min", mesh_cdf, 1, 1)
    add("fpsg_mesh_cdf", "scan-1024+1", mesh_cdf, 40, 1025)
    add("fpsg_mesh_cdf", "scan-blocks", mesh_cdf, 300, 3 * 1024 + 7)
    # K27 / K28 / K31b: one thread draws a box of up to 64 pixel centres, 16 waves share a larger triangle
    for entry, form in (("fpsg_mesh_render", "plain"), ("fpsg_mesh_render_materials", "materials"),
                        ("fpsg_mesh_render_smooth", "smooth")):
        add(entry, "min", mesh_render, 3, 1, 1, 1, 1, 1, form=form)
        add(entry, "box-64+", mesh_render, 40, 70, 1, 132, 70, 2, form=form, bg=True)
        add(entry, "views3", mesh_render, 30, 65, 3, 20, 12, 4, form=form)
        # "Any output may be NULL, not all"
        add(entry, "image-only", mesh_render, 30, 65, 3, 20, 12, 4, form=form, drop=("radiance", "face_id", "depth"))
        add(entry, "ids-only", mesh_render, 30, 65, 3, 20, 12, 4, form=form, drop=("image", "radiance"))
    # K29: tiles of 32 x 32 samples, 256 threads
    add("fpsg_points_render", "min", points_render, 1, 1, 1, 1, 1, 1, False)
    add("fpsg_points_render", "tile+1", points_render, 1, 257, 1, 66, 34, 2, True)
    add("fpsg_points_render", "batch3", points_render, 3, 65, 2, 36, 20, 4, True)
    add("fpsg_points_render", "depth-only", points_render, 3, 65, 2, 36, 20, 4, True, drop=("image", "radiance", "point_id"))
    add("fpsg_points_render", "radiance-only", points_render, 3, 65, 2, 36, 20, 4, False, drop=("image", "depth", "point_id"))
    # K32: 512 points per workgroup, 256 faces per LDS tile, chunks of >= 64 faces
    add("fpsg_point_mesh_distance", "min", point_mesh, 1, 1, 3, 1, 0, 1)
    add("fpsg_point_mesh_distance", "tile+1-chunks3", point_mesh, 1, 513, 40, 771, 0, 3)
    add("fpsg_point_mesh_distance", "batch3-auto", point_mesh, 3, 67, 30, 70, 1, 0)
    add("fpsg_point_mesh_distance", "chunks-64", point_mesh, 2, 70, 20, 64 * 64 + 5, 0, 64)
    add("fpsg_point_mesh_distance", "dist-only", point_mesh, 3, 67, 30, 70, 1, 0, drop=("closest", "bary"))   # "or NULL"
    # K33: kSelfKnnTile = 1024 candidates, 128 list rows per tile of the reverse sweeps, 1024 threads in the forest
    add("fpsg_point_normals", "min", point_normals, 1, 4, 3, 0, True)
    add("fpsg_point_normals", "tile-1024+1-ws-lists", point_normals, 1, 1025, 8, 1, False)
    add("fpsg_point_normals", "batch3", point_normals, 3, 130, 5, 2, True)
    add("fpsg_point_normals", "k-32", point_normals, 2, 200, 32, 0, False)
    add("fpsg_point_normals", "null-ref-variation", point_normals, 3, 130, 5, 0, True, drop=("ref", "variation"))
    add("fpsg_point_normals_orient", "min", point_normals_orient, 1, 4, 3, 0)
    add("fpsg_point_normals_orient", "1024+1", point_normals_orient, 1, 1025, 4, 1)
    add("fpsg_point_normals_orient", "batch3", point_normals_orient, 3, 130, 5, 2)
    add("fpsg_point_normals_orient", "no-parent", point_normals_orient, 3, 130, 5, 2, drop=("parent",))
    return c


CASES = _cases()
ENTRIES = sorted({c[1] for c in CASES})


class _Optional(dict):
    """Addresses by name; a buffer the case left out is NULL."""

    def __missing__(self, name):
        return None


def build(case, lib) -> Row:
    """The case's row.  drop=(names): arguments the header lets a caller pass as NULL are left out of the call."""
    _, _, fn, args, kw = case
    kw = dict(kw)
    drop = kw.pop("drop", ())
    row = fn(lib, *args, **kw)
    if drop:
        assert set(drop) < {b.name for b in row.bufs} and "ws" not in drop
        row.bufs = [b for b in row.bufs if b.name not in drop]
        inner = row.call
        row.call = lambda p, s, wsn: inner(_Optional(p), s, wsn)
    return row


def run_once(row, layout, scale, lib):
    """One call of the row in `layout` (tests/_guarded.py): it returns 0, the guards and the pure inputs are unchanged;
    gives the output bits."""
    p = layout.ptrs()
    if row.late:
        for name, data in row.late(p).items():
            layout.poke(name, data)
    torch.cuda.synchronize()
    rc = row.call(p, torch.cuda.current_stream().cuda_stream, row.ws_units * scale)
    torch.cuda.synchronize()
    assert rc == 0, f"[{layout.pattern}] returned {rc}: {(lib.fpsg_last_error() or b'').decode()}"
    layout.check()
    return layout.outputs()


def five_runs(case, lib, gpu):
    """The procedure of tests/test_memory_contract_gpu.py for one case, on the library handle `lib`: guarded arenas under
    the three fills, the roomy layout, the first fill again; every output element bit-identical across the five."""
    import _guarded as G
    row = build(case, lib)
    runs = []
    for i, pattern in enumerate(G.PATTERNS):
        runs.append((pattern, run_once(row, G.Arena(row.bufs, pattern, gpu, seed=17 + i), 1, lib)))
    runs.append(("roomy", run_once(row, G.Roomy(row.bufs, gpu), 2, lib)))
    runs.append(("ff again", run_once(row, G.Arena(row.bufs, G.PATTERNS[0], gpu), 1, lib)))
    name0, ref = runs[0]
    sizes = {b.name: torch.empty((), dtype=b.dtype).element_size() for b in row.bufs}
    for name, outs in runs[1:]:
        for buf, bits in outs.items():
            at = G.first_difference(ref[buf], bits, sizes[buf])
            assert at is None, f"output '{buf}' differs between the '{name0}' and '{name}' runs, first at element {at}"
    return ref
