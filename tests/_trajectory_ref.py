"""What the multi-step trajectory tests share (tests/test_trajectory_cpu.py, tests/test_trajectory_gpu.py; DESIGN.md
section 5): the shape, the reference's pieces in float64, snapshots, one reference Adam step from a snapshot, and the
comparison rule of the teacher-forced steps.

Teacher-forced: after every step ``t`` of ONE continuing run a snapshot is taken (model, optimizer, scheduler, weight
average); step ``t + 1`` of the continuing run is compared with step ``t + 1`` taken from that snapshot by objects that
have no history.  Both start from identical state, so two free-running trajectories never have to be compared (that
amplifies round-off) and any difference is state that did not follow the weights from one step to the next."""
import collections
import copy
import json
import os

import torch

GROUPS = ("img_encoder", "pc_encoder", "pc_decoder")
LOSS_KEYS = ("query_rec_loss", "support_rec_loss", "ttl_loss")

# the smallest shape at which all of the cross-step state exists: Winograd trunk, decoder pack, training-mode BatchNorm
S, Q, N_PTS, IMG = 2, 1, 2048, 64
LR = 1e-3
MARGIN = 3.0                     # over a run-to-run yardstick, as tests/test_step_switches_gpu.py

# The conditions tests/test_trajectory_cpu.py asserts on the reference alone, and what they allow the GPU test's bounds.
# One stale weight tensor moves a reconstruction loss by at least SINGLE_TENSOR_FLOOR (relative), at every step and for
# every tensor of the set.  The floor is set by the first layer of a deformer (2 input channels; measured 3.6e-5 to 8.8e-4
# over the steps, the direction of one Adam step against the next episode's gradient being close to orthogonal at
# times); every other kind of tensor is at least SINGLE_TENSOR_FLOOR_WITHOUT_DEFORMER_INPUT (measured 1.2e-3).
SINGLE_TENSOR_FLOOR = 3e-5
SINGLE_TENSOR_FLOOR_WITHOUT_DEFORMER_INPUT = 1e-3
GROUP_FLOOR = 4e-3               # one stale module group moves ttl_loss by at least this (relative)
REFERENCE_DEVIATION_CAP = 3e-4   # fp32 CPU port against float64, every loss at every snapshot
RESTART_LOSS_BOUND_CAP = SINGLE_TENSOR_FLOOR / 10      # restart leg: a bound on a loss is valid only up to here
FLOAT64_LOSS_BOUND_CAP = GROUP_FLOOR / 4               # float64 leg: likewise


# ---- the shape ----------------------------------------------------------------------------------------------------------

def options(**overrides):
    from fpsg_amd.engine import default_options
    kw = dict(intra_recon=True, lr=LR, lr_decay=1)
    kw.update(overrides)
    return default_options(**kw)


def episode(k, device="cpu"):
    from fpsg_amd.episodes import synthetic_episode
    return synthetic_episode(S, Q, n_pts=N_PTS, img_size=IMG, seed=3 + k, device=device)


def episode_to(ep, device=None, dtype=None):
    out = {}
    for k, v in ep.items():
        if torch.is_tensor(v):
            v = v.to(device) if device is not None else v
            v = v.to(dtype) if dtype is not None and v.is_floating_point() else v
        out[k] = v
    return out


# ---- the reference's pieces (shared with tests/test_episode_parity_gpu.py) -------------------------------------------------

def chamfer64(p1, p2, w1=1.0, w2=1.0):
    """Kaolin's chamfer_distance semantics (few_shot.py:57,110) in torch, differentiable through the arg-min: in float64
    the 'truth' metric of the float64 run."""
    d = (p1.unsqueeze(2) - p2.unsqueeze(1)).square().sum(-1)          # [B,N,M]
    return w1 * d.min(dim=2)[0].mean(dim=1) + w2 * d.min(dim=1)[0].mean(dim=1)


def fixed_grids(model, sizes, device):
    return {b: model.pc_decoder.sample_grids(b, device, torch.Generator(device=device).manual_seed(100 + b))
            for b in sizes}


def grids_to(grids, device=None, dtype=None):
    return {b: [[t.to(device=device, dtype=dtype) for t in c] for c in g] for b, g in grids.items()}


def pin_grids(model, grids):
    orig = model.pc_decoder.forward
    model.pc_decoder.forward = lambda h, grid=None, generator=None, pack=None: orig(h, grid=grids[h.size(0)], pack=pack)
    pair = model.pc_decoder.forward_pair        # the episode's two decodes side by side (its fallback calls .forward)
    model.pc_decoder.forward_pair = lambda a, b, generator=None, pack=None, grids_=None: pair(
        a, b, pack=pack, grids=(grids[a.size(0)], grids[b.size(0)]))


# ---- snapshots ------------------------------------------------------------------------------------------------------------

def copy_state(obj):
    """A state dict with every tensor cloned where it is (``FlatAdam``'s entries are views of its flat buffers, the
    model's are the live parameters); containers keep their type, a module state dict its ``_metadata``."""
    if torch.is_tensor(obj):
        return obj.detach().clone()
    if isinstance(obj, dict):
        out = type(obj)((k, copy_state(v)) for k, v in obj.items())
        if hasattr(obj, "_metadata"):
            out._metadata = copy.deepcopy(obj._metadata)
        return out
    if isinstance(obj, (list, tuple)):
        return type(obj)(copy_state(v) for v in obj)
    return copy.deepcopy(obj)


def snapshot(model, optimizer, scheduler=None, ema=None):
    return {"model": copy_state(model.state_dict()), "optimizer": copy_state(optimizer.state_dict()),
            "scheduler": copy_state(scheduler.state_dict()) if scheduler is not None else None,
            "ema": copy_state(ema.state_dict()) if ema is not None else None}


def is_weight(name):
    return "running_" not in name and "num_batches_tracked" not in name


# ---- the reference model on the CPU ------------------------------------------------------------------------------------------

def cpu_reference(template, grids, dtype=torch.float32, metric=None):
    """A copy of the (unpinned, CPU, fp32) ``template`` in ``dtype`` with ``metric`` as its point-cloud distance
    (default: ``chamfer64``) and the patch grids pinned."""
    m = copy.deepcopy(template)
    if dtype != torch.float32:
        m = m.to(dtype)
    m.pc_metric = metric if metric is not None else chamfer64
    pin_grids(m, grids_to(grids, "cpu", dtype))
    return m.train()


def losses_of(out):
    return {k: float(out[k].detach().sum()) for k in LOSS_KEYS}


def adam_from_snapshot(model, opt_state):
    """``torch.optim.Adam`` over ``model``'s parameters (any dtype) holding the moments, step count, learning rate, betas
    and eps of ``opt_state`` (``torch.optim.Adam``'s format, which ``FlatAdam.state_dict()`` keeps; its param_groups lack
    Adam's other keys, so the state is placed by hand rather than through ``load_state_dict``)."""
    g = opt_state["param_groups"][0]
    optimizer = torch.optim.Adam(model.parameters(), lr=float(g["lr"]), betas=tuple(g["betas"]), eps=float(g["eps"]))
    params = list(model.parameters())
    assert len(g["params"]) == len(params)
    for slot, index in enumerate(g["params"]):
        st = opt_state["state"].get(index)
        if st is None:
            continue
        p = params[slot]
        optimizer.state[p] = {"step": torch.tensor(float(st["step"])),
                              "exp_avg": st["exp_avg"].detach().to(device=p.device, dtype=p.dtype).clone(),
                              "exp_avg_sq": st["exp_avg_sq"].detach().to(device=p.device, dtype=p.dtype).clone()}
    return optimizer


def reference_step(model, snap, episodes):
    """One optimizer step of the reference from ``snap``: ``model`` (CPU, any dtype, metric and grids in place) takes the
    snapshot's weights and buffers, runs ``episodes``, and steps ``torch.optim.Adam`` with the snapshot's moments and
    step count on the MEAN gradient.  -> (losses per episode, {group: flat update ``p_after - p_before`` in float64})."""
    p0 = next(model.parameters())
    model.load_state_dict({k: v.detach().to("cpu") for k, v in snap["model"].items()})
    model.train()
    optimizer = adam_from_snapshot(model, snap["optimizer"])
    before = {n: p.detach().clone() for n, p in model.named_parameters()}
    optimizer.zero_grad(set_to_none=True)
    losses = []
    for ep in episodes:
        out = model.loss(episode_to(ep, "cpu", p0.dtype))
        (out["ttl_loss"].sum() / len(episodes)).backward()
        losses.append(losses_of(out))
    optimizer.step()
    return losses, group_updates(before, dict(model.named_parameters()))


def group_updates(before, after):
    out = {}
    for g in GROUPS:
        out[g] = torch.cat([(after[n].detach().double().cpu() - before[n].detach().double().cpu()).reshape(-1)
                            for n in before if n.startswith(g) and after[n].requires_grad])
    return out


def rel_l2(a, b):
    """``||a - b|| / ||b||`` in float64 (the absolute distance where ``b`` is zero)."""
    a, b = a.detach().double().reshape(-1), b.detach().double().reshape(-1)
    d, n = float((a - b).norm()), float(b.norm())
    return d / n if n > 0 else d


# ---- what a step leaves behind, and the rule of the restart leg -----------------------------------------------------------------

def collect(model, optimizer, outs, ema=None, extra=None):
    """Everything of one finished step that the restart leg compares, as fresh tensors (nothing here aliases the side
    it was read from): the losses of every episode; per module group the step's gradient (the parameters' ``.grad``: views
    of the flat buffer behind a several-episode step, the backward's own tensors on the pointer-table path), the
    parameters and both moments; the shadow; the BatchNorm running statistics; and, compared exactly whatever the
    yardstick says, the counters (``num_batches_tracked``, the optimizer's step count, the average's update count)."""
    q = collections.OrderedDict()
    for e, out in enumerate(outs):
        for k in sorted(out):
            q[f"loss[{e}].{k}"] = out[k].detach().double().sum().reshape(1).cpu()
    named = [(n, p) for n, p in model.named_parameters() if p.requires_grad]
    for g in GROUPS:
        mine = [(n, p) for n, p in named if n.startswith(g)]
        q[f"grad[{g}]"] = torch.cat([(p.grad if p.grad is not None else torch.zeros_like(p)).detach().reshape(-1)
                                     for _, p in mine]).clone()
        q[f"param[{g}]"] = torch.cat([p.detach().reshape(-1) for _, p in mine]).clone()
        for key in ("exp_avg", "exp_avg_sq"):
            q[f"{key}[{g}]"] = torch.cat([optimizer.state[p][key].detach().reshape(-1) for _, p in mine]).clone()
    frozen = [p.detach().reshape(-1) for _, p in model.named_parameters() if not p.requires_grad]
    if frozen:
        q["param[frozen]"] = torch.cat(frozen).clone()
    if ema is not None:
        q["shadow"] = torch.cat([e.detach().reshape(-1) for e in ema.shadow]).clone()
    buffers = list(model.named_buffers())
    q["bn_running"] = torch.cat([b.detach().reshape(-1).float() for n, b in buffers if "running_" in n]).clone()
    counters = [b.detach().reshape(-1).double().cpu() for n, b in buffers if "num_batches_tracked" in n]
    counters.append(torch.tensor([float(getattr(optimizer, "_t", -1)), float(ema.updates) if ema is not None else -1.0,
                                  float(optimizer.param_groups[0]["lr"])], dtype=torch.float64))
    q["exact:counters"] = torch.cat(counters)
    for k, v in (extra or {}).items():
        q[k] = v
    return q


def compare(a, b, y1, y2, what=""):
    """The rule of the restart leg for every quantity of ``collect``: ``a`` (the continuing run) against ``b`` (a side
    without history), with the two history-free sides ``y1`` / ``y2`` as the yardstick.  Where the yardstick pair agrees
    bit for bit, so must ``a`` and ``b``; where it does not, ``rel_l2(a, b) <= MARGIN * rel_l2(y1, y2)`` -- and on a loss
    such a bound is valid only up to ``RESTART_LOSS_BOUND_CAP``.  Counters are always exact.
    -> (record, violations): the record holds per quantity ``[difference, yardstick]`` and what held."""
    assert list(a) == list(b) == list(y1) == list(y2), (what, [list(x) for x in (a, b, y1, y2)])
    quantities, violations = {}, []
    pair_equal = cont_equal = True
    for k in a:
        same_yard = torch.equal(y1[k], y2[k])
        same = torch.equal(a[k], b[k])
        diff, yard = rel_l2(a[k], b[k]), rel_l2(y1[k], y2[k])
        pair_equal, cont_equal = pair_equal and same_yard, cont_equal and same
        quantities[k] = [diff, yard]
        if k.startswith("exact:"):
            if not same:
                violations.append((what, k, "counters differ", a[k].tolist()[-3:], b[k].tolist()[-3:]))
            if not same_yard:
                violations.append((what, k, "the yardstick pair's counters differ"))
        elif same_yard:
            if not same:
                violations.append((what, k, "not bit-equal although two history-free sides are", diff))
        else:
            if k.startswith("loss[") and MARGIN * yard > RESTART_LOSS_BOUND_CAP:
                violations.append((what, k, "invalid bound: two history-free sides differ by more than the "
                                            "staleness sensitivity allows", yard))
            if not diff <= MARGIN * yard:
                violations.append((what, k, "beyond three times the difference of two history-free sides", diff, yard))
    record = {"what": what, "yardstick_bit_equal": pair_equal, "continuing_bit_equal": cont_equal,
              "max_difference": max(v[0] for v in quantities.values()),
              "max_yardstick": max(v[1] for v in quantities.values()),
              "quantities": {k: v for k, v in quantities.items() if v != [0.0, 0.0]}}
    return record, violations


def record(payload):
    """Measured values are printed; with ``FPSG_TRAJECTORY_RECORD=<file>`` they are appended there as well (how
    profiles/trajectory/deviation.jsonl was made)."""
    line = json.dumps(payload)
    print(line)
    path = os.environ.get("FPSG_TRAJECTORY_RECORD")
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")
