"""Several optimizer steps of the real model, each held to the same step taken from a snapshot by objects without history
(the method and the rule: tests/_trajectory_ref.py; the conditions on the inputs: tests/test_trajectory_cpu.py; the
measured values: profiles/trajectory/deviation.jsonl).

What follows the weights from one step to the next is host code -- the filter bank and the step-scoped cache of
``winograd``, captured graphs, the flat gradient buckets, ``FlatAdam``'s step count / pointer table / ``grad_scale``, the
deferred BatchNorm counters, the weight average, the scheduler, ``eval()`` / ``train()`` around an evaluation, the resume
files.  A stale entry in any of it gives finite, plausible losses; only a comparison from an identical start sees it.

Restart leg: the continuing run's step against the same step of a side built from the snapshot alone (new model, new
optimizer, eager, an empty filter bank with FPSG_FILTER_BANK=0); yardstick: a second such side.  float64 leg: the same
step by the CPU port in float64 with ``torch.optim.Adam``; yardstick: the fp32 CPU port."""
import collections
import contextlib
import copy
import gc
import os

import pytest
import torch

import _trajectory_ref as tr

pytestmark = pytest.mark.gpu

TERMS = dict(pc_dist="sinkhorn", n_shot=tr.S, n_query=tr.Q, repulsion_weight=0.25, expansion_weight=0.125,
             uniform_weight=0.5, uniform_percentages=(0.01, 0.03), uniform_radius=0.5)
# counts: episodes per step; graphs: captured graphs at the end (one per shape and first / later episode of a step);
# evaluate_after / resume_after: 0-based index of the step behind which the evaluation / the save to files happens
CONFIGS = {
    "direct": dict(counts=(1, 1, 1, 1)),                                   # pointer table: no flat gradient buffer
    "flat": dict(counts=(2, 2, 2, 2), evaluate_after=(1, 3)),              # lazy absorb, folded 1/E
    "graph-flat": dict(counts=(2,) * 6, graph=True, graphs=2),             # two eager uses, the capture, three replays
    "graph-direct": dict(counts=(1,) * 6, graph=True, graphs=1),           # gradients in the graph's pool
    "clip-ema": dict(counts=(2, 2, 2, 2), opts=dict(clip_grad_norm=0.5, ema_decay=0.9), evaluate_after=(1, 3),
                     resume_after=2),
    "dgcnn": dict(counts=(2, 2, 2), opts=dict(pc_encoder="dgcnn")),
    "terms": dict(counts=(2,) * 5, graph=True, graphs=2, opts=TERMS),
}
SCHEDULER_STEP_AFTER = 1        # scheduler.step() behind the second step: the learning rate is part of the moving state


@contextlib.contextmanager
def _no_history(bank_off=True, **env):
    """The block's filters come from an EMPTY filter bank (the continuing run's bank, whose pinned buffers its captured
    graphs read, is put back afterwards) and, with ``bank_off``, from one launch per filter (FPSG_FILTER_BANK=0)."""
    from fpsg_amd import winograd
    if bank_off:
        env["FPSG_FILTER_BANK"] = "0"
    saved_bank, winograd._bank = winograd._bank, winograd._FilterBank()
    saved_env = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        yield
    finally:
        winograd._bank = saved_bank
        for k, v in saved_env.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


class _Side:
    """Model, optimizer, scheduler, weight average and ``TrainStep`` in the order ``trainNetwork.main`` makes them;
    ``weights`` / ``state``: what a resumed run loads (a snapshot's entries, or the files' contents)."""

    def __init__(self, template, opt, gpu, grids, graph=False, weights=None, state=None):
        from fpsg_amd.engine import TrainStep, build_optimizer
        model = copy.deepcopy(template)
        if weights is not None:
            model.load_state_dict(weights)
        self.model = model.to(gpu).train()
        self.optimizer, self.scheduler = build_optimizer(self.model, opt)
        self.ema = getattr(self.optimizer, "ema", None)
        assert (self.ema is not None) == bool(opt.ema_decay)
        if state is not None:
            # (a copy: torch's own load_state_dict keeps tensors that already have the parameter's device and dtype, and
            # a step of this side must not move the snapshot the next side starts from)
            self.optimizer.load_state_dict(tr.copy_state(state["optimizer"]))
            self.scheduler.load_state_dict(state["scheduler"])
            if self.ema is not None:
                self.ema.load_state_dict(state["ema"])
        self.step = TrainStep(self.model, self.optimizer, graph=graph)
        self.clips = bool(opt.clip_grad_norm)
        tr.pin_grids(self.model, grids)

    def run(self, eps, seed):
        torch.manual_seed(seed)                 # whatever a loss term draws, every side draws the same
        outs = self.step(eps, n_episodes_global=len(eps))
        extra = {}
        if self.clips:
            s = self.step.clip_stats(reset=True)          # this step's alone, on a side with history as on one without
            extra["exact:clip_counts"] = torch.tensor([s["steps"], s["clipped"], s["nonfinite"]], dtype=torch.float64)
            extra["clip_norm"] = torch.tensor([s["max_norm_seen"], float(self.step.last_grad_norm)], dtype=torch.float64)
        return tr.collect(self.model, self.optimizer, outs, self.ema, extra)

    def snapshot(self):
        return tr.snapshot(self.model, self.optimizer, self.scheduler, self.ema)

    def aliases_flat_buffer(self):
        o = self.optimizer
        return all(p.data_ptr() == o.flat_param.data_ptr() + 4 * off and p.numel() == n for p, off, n in o._layout)


def _evaluate(model, items):
    """What ``trainNetwork.evaluate`` does to the model around its report."""
    from fpsg_amd import winograd
    model.eval()
    with torch.no_grad(), winograd.weights_frozen():
        outs = [model.loss(item) for item in items]
    model.train()
    return collections.OrderedDict((f"loss[eval {i}].{k}", out[k].detach().double().sum().reshape(1).cpu())
                                   for i, out in enumerate(outs) for k in tr.LOSS_KEYS)


def _evaluate_without_history(template, weights, gpu, grids, items):
    with _no_history(FPSG_EVAL_CHAN_CACHE="0", FPSG_EVAL_PACK_CACHE="0"):
        model = copy.deepcopy(template)
        model.load_state_dict(weights)
        model = model.to(gpu)
        tr.pin_grids(model, grids)
        out = _evaluate(model, items)
    del model
    gc.collect()
    return out


def _everything(side):
    state = tr.copy_state(side.model.state_dict())
    if side.ema is not None:
        state["shadow"] = torch.cat([e.detach().reshape(-1) for e in side.ema.shadow]).clone()
    return state


def _check_evaluation(side, template, gpu, grids, items, what, records, violations):
    before = _everything(side)
    passes = [("", contextlib.nullcontext)] + ([("[EMA]", side.ema.swapped)] if side.ema is not None else [])
    for tag, block in passes:
        with block():
            got = _evaluate(side.model, items)
            weights = tr.copy_state(side.model.state_dict())        # with EMA: the swapped state dict
        y1, y2 = (_evaluate_without_history(template, weights, gpu, grids, items) for _ in range(2))
        rec, bad = tr.compare(got, y1, y1, y2, f"{what} evaluation{tag}")
        records.append(rec)
        violations += bad
    after = _everything(side)
    changed = [k for k in before if not torch.equal(before[k], after[k])]
    if changed:
        violations.append((what, "the evaluation changed", changed[:5]))
    assert side.model.training and all(m.training for m in side.model.modules())


def _save_as_training_does(side, folder, epoch):
    """The three files of ``trainNetwork.main``'s save."""
    torch.save(side.model.state_dict(), os.path.join(folder, f"model_epoch_{epoch}.pt"))
    train_state = {"optimizer": side.optimizer.state_dict(), "scheduler": side.scheduler.state_dict(), "epoch": epoch}
    if side.ema is not None:
        with side.ema.swapped():
            torch.save(side.model.state_dict(), os.path.join(folder, f"model_epoch_{epoch}_ema.pt"))
        train_state["ema"] = side.ema.state_dict()
    torch.save(train_state, os.path.join(folder, f"train_state_epoch_{epoch}.pt"))


def _resume_as_training_does(template, opt, gpu, grids, folder, epoch):
    weights = torch.load(os.path.join(folder, f"model_epoch_{epoch}.pt"), map_location="cpu", weights_only=True)
    state = torch.load(os.path.join(folder, f"train_state_epoch_{epoch}.pt"), map_location=gpu, weights_only=True)
    assert int(state["epoch"]) == epoch
    side = _Side(template, opt, gpu, grids, weights=weights, state=state)
    assert side.aliases_flat_buffer()            # the three loads copied INTO the flat buffers: nothing was re-pointed
    if side.ema is not None:
        # the averaged weights' file is the shadow under the parameters' names, with the live buffers
        avg = torch.load(os.path.join(folder, f"model_epoch_{epoch}_ema.pt"), map_location=gpu, weights_only=True)
        shadow = {id(p): e for p, e in zip(side.ema.params, side.ema.shadow)}
        assert all(torch.equal(avg[n], shadow[id(p)]) for n, p in side.model.named_parameters() if id(p) in shadow)
        assert all(torch.equal(avg[n], b) for n, b in side.model.named_buffers())
    return side


class _NoDefect:
    name = None

    def on(self):
        return contextlib.nullcontext()

    resumed = on

    def after_step(self, side):
        pass


def _trajectory(gpu, name, cfg, **kw):
    """``_run_trajectory`` with a filter bank of the case's own.  The process-wide bank keeps every entry a captured graph
    has seen for the life of the process and takes no more than ``MAX_ENTRIES``: behind a few graph cases it is full of
    dead models' filters and a later case's continuing run would register nothing -- and test nothing of the bank."""
    from fpsg_amd import winograd
    saved, winograd._bank = winograd._bank, winograd._FilterBank()
    try:
        out = _run_trajectory(gpu, name, cfg, **kw)
        # the continuing run did go through the bank: its filters are registered (and pinned by its captures)
        assert winograd._bank.entries and winograd._bank.has_pinned() == bool(cfg.get("graph")) and not winograd._bank.valid
        return out
    finally:
        winograd._bank = saved


def _run_trajectory(gpu, name, cfg, tmp_path=None, oracle=None, restart=True, float64=False, defect=None, write=True):
    """The continuing run of configuration ``name``, every step compared as the legs say.  -> (violations, records);
    a violation is a tuple that starts with ``"<name> step <t>..."``."""
    from fpsg_amd.engine import build_model
    defect = defect or _NoDefect()
    counts = cfg["counts"]
    torch.manual_seed(0)
    opts = cfg.get("opts", {})
    template = build_model(tr.options(device="cpu", **opts))           # the one model build of the case
    opt = tr.options(device="cuda", **opts)
    grids_cpu = tr.fixed_grids(template, (tr.S, tr.Q), "cpu")
    grids = tr.grids_to(grids_cpu, gpu)
    held_out = [tr.episode(50 + i, gpu) for i in range(2)]
    violations, records = [], []
    if float64:
        ref64 = tr.cpu_reference(template, grids_cpu, torch.float64)
        ref32 = tr.cpu_reference(template, grids_cpu, torch.float32, oracle.make_torch_chamfer())
        dev_hip, dev_cpu = {}, {}

    cont = _Side(template, opt, gpu, grids, graph=cfg.get("graph", False))
    resumed = None
    k = 0
    for t, count in enumerate(counts):
        what = f"{name} step {t}"
        snap = cont.snapshot()
        eps = [tr.episode(k + i, gpu) for i in range(count)]
        k += count
        with defect.on():
            got = cont.run(eps, 1000 + t)
        defect.after_step(cont)
        if restart:
            fresh = []
            for _ in range(2):
                with _no_history():
                    side = _Side(template, opt, gpu, grids, weights=snap["model"], state=snap)
                    fresh.append(side.run(eps, 1000 + t))
                del side
                gc.collect()
            rec, bad = tr.compare(got, fresh[0], fresh[0], fresh[1], what)
            records.append(rec)
            violations += bad
            if resumed is not None:
                with _no_history(bank_off=False), defect.resumed():
                    res = resumed.run(eps, 1000 + t)
                rec, bad = tr.compare(got, res, fresh[0], fresh[1], what + " resumed from files")
                records.append(rec)
                violations += bad
                resumed = None
                gc.collect()
        if float64:
            l64, u64 = tr.reference_step(ref64, snap, eps)
            l32, u32 = tr.reference_step(ref32, snap, eps)
            uhip = tr.group_updates({n: snap["model"][n] for n, _ in cont.model.named_parameters()},
                                    dict(cont.model.named_parameters()))
            rec = {"what": what + " float64"}
            for e in range(count):
                for key in tr.LOSS_KEYS:
                    hip = float(got[f"loss[{e}].{key}"])
                    dev_hip[(t, e, key)] = abs(hip - l64[e][key]) / abs(l64[e][key])
                    dev_cpu[(t, e, key)] = abs(l32[e][key] - l64[e][key]) / abs(l64[e][key])
                    rec[f"loss[{e}].{key}"] = {"hip_vs_f64": dev_hip[(t, e, key)], "cpu32_vs_f64": dev_cpu[(t, e, key)]}
            for g in tr.GROUPS:
                a, b = tr.rel_l2(uhip[g], u64[g]), tr.rel_l2(u32[g], u64[g])
                rec[f"update[{g}]"] = {"hip_vs_f64": a, "cpu32_vs_f64": b}
                if not a <= tr.MARGIN * b:
                    violations.append((what, f"update[{g}]", "further from float64's update than three times the fp32 "
                                                             "CPU port's", a, b))
            records.append(rec)
        if t == SCHEDULER_STEP_AFTER:
            cont.scheduler.step()
        if restart and t in cfg.get("evaluate_after", ()):
            _check_evaluation(cont, template, gpu, grids, held_out, what, records, violations)
        if restart and t == cfg.get("resume_after") and t + 1 < len(counts):
            _save_as_training_does(cont, str(tmp_path), t + 1)
            with _no_history(bank_off=False), defect.resumed():
                resumed = _resume_as_training_does(template, opt, gpu, grids, str(tmp_path), t + 1)
        if violations and defect.name is not None:
            break                               # a seeded defect: the first step that shows it is what is asked
    if float64:
        # every loss of the HIP run within three times the reference arithmetic's own largest deviation from float64
        bound = tr.MARGIN * max(dev_cpu.values())
        records.append({"what": f"{name} float64 bound", "largest_cpu32_vs_f64": max(dev_cpu.values()),
                        "largest_hip_vs_f64": max(dev_hip.values()), "bound": bound})
        if bound > tr.FLOAT64_LOSS_BOUND_CAP:
            violations.append((name, "invalid bound: the fp32 CPU port is further from float64 than a quarter of the "
                                     "group sensitivity allows", bound))
        violations += [(f"{name} step {t}", f"loss[{e}].{key}", "further from float64 than three times the fp32 CPU "
                        "port ever is", v, bound) for (t, e, key), v in dev_hip.items() if not v <= bound]
    if "graphs" in cfg and defect.name is None:
        assert len(cont.step._graphs) == cfg["graphs"]
    if cfg.get("opts", {}).get("ema_decay") and defect.name is None:
        assert cont.ema.updates == len(counts)
    for rec in records:
        rec["config"] = name
        if write:
            tr.record(rec)
    return violations, records


@pytest.mark.parametrize("name", list(CONFIGS))
def test_every_step_equals_the_step_of_a_run_without_history(gpu, tmp_path, name):
    violations, records = _trajectory(gpu, name, CONFIGS[name], tmp_path=tmp_path)
    steps = [r for r in records if "yardstick_bit_equal" in r]
    print(f"{name}: {len(steps)} comparisons; two history-free sides bit-equal in {sum(r['yardstick_bit_equal'] for r in steps)}, "
          f"the continuing run bit-equal in {sum(r['continuing_bit_equal'] for r in steps)}; largest difference "
          f"{max(r['max_difference'] for r in steps):.3e}, largest yardstick {max(r['max_yardstick'] for r in steps):.3e}")
    assert not violations, violations


@pytest.mark.parametrize("name", ["direct", "flat"])
def test_every_step_follows_one_float64_step_from_its_snapshot(gpu, oracle, name):
    violations, _ = _trajectory(gpu, name, CONFIGS[name], oracle=oracle, restart=False, float64=True)
    assert not violations, violations


# ---- the comparison must be seen to catch staleness ----------------------------------------------------------------------------
# Each defect leaves every pointer valid and puts OLD VALUES into live buffers, on the continuing side only.

class _Defect(_NoDefect):
    def __init__(self, name, monkeypatch):
        self.name, self.flag, self.flag_resumed = name, {"on": False}, {"on": False}
        self.acted = 0                  # how often the defect put an old value somewhere
        getattr(self, "_patch_" + name)(monkeypatch)

    @contextlib.contextmanager
    def _raise(self, flag):
        flag["on"] = True
        try:
            yield
        finally:
            flag["on"] = False

    def on(self):
        return self._raise(self.flag)

    def resumed(self):
        return self._raise(self.flag_resumed)

    def _patch_bank(self, monkeypatch):
        """(a) ``_FilterBank.refresh`` leaves the last registered entry as it was."""
        from fpsg_amd import winograd
        orig, flag = winograd._FilterBank.refresh, self.flag

        def refresh(bank):
            if not flag["on"] or not bank.entries:
                return orig(bank)
            entry = list(bank.entries.values())[-1]
            old = entry[1].clone()
            orig(bank)
            entry[1].copy_(old)
            self.acted += 1

        monkeypatch.setattr(winograd._FilterBank, "refresh", refresh)

    def _patch_cache(self, monkeypatch):
        """(b) ``weights_frozen.__exit__`` keeps the step-scoped cache for the next block."""
        from fpsg_amd import winograd
        enter, leave, flag, kept = winograd.weights_frozen.__enter__, winograd.weights_frozen.__exit__, self.flag, {}

        def __enter__(block):
            out = enter(block)
            if flag["on"] and block._outer is None and "cache" in kept:
                winograd._frozen_cache = kept["cache"]
                self.acted += 1
            return out

        def __exit__(block, *exc):
            if flag["on"] and block._outer is None:
                kept["cache"] = winograd._frozen_cache
            return leave(block, *exc)

        monkeypatch.setattr(winograd.weights_frozen, "__enter__", __enter__)
        monkeypatch.setattr(winograd.weights_frozen, "__exit__", __exit__)

    def _patch_count(self, monkeypatch):
        """(c) ``FlatAdam.step`` does not advance ``_t`` after a ``load_state_dict`` (the resumed side)."""
        from fpsg_amd.optim import FlatAdam
        load, step, flag = FlatAdam.load_state_dict, FlatAdam.step, self.flag_resumed

        def load_state_dict(optimizer, state):
            load(optimizer, state)
            optimizer._count_stuck = flag["on"]

        def stuck_step(optimizer, closure=None):
            if getattr(optimizer, "_count_stuck", False):
                optimizer._t -= 1
                self.acted += 1
            return step(optimizer, closure)

        monkeypatch.setattr(FlatAdam, "load_state_dict", load_state_dict)
        monkeypatch.setattr(FlatAdam, "step", stuck_step)

    def _patch_lr(self, monkeypatch):
        """(d) ``scheduler.step()`` has no effect on the learning rate ``FlatAdam.step`` passes."""
        from fpsg_amd.optim import FlatAdam
        step, flag = FlatAdam.step, self.flag

        def deaf_step(optimizer, closure=None):
            group = optimizer.param_groups[0]
            lr = group["lr"]
            if flag["on"]:
                self.acted += group["lr"] != group["initial_lr"]
                group["lr"] = group["initial_lr"]
            try:
                return step(optimizer, closure)
            finally:
                group["lr"] = lr

        monkeypatch.setattr(FlatAdam, "step", deaf_step)

    def _patch_scale(self, monkeypatch):
        """(e) the ``grad_scale`` reset behind the step is skipped: the next step that does not set it (one episode:
        the pointer-table path) still multiplies its gradient by the last step's 1/E."""
        from fpsg_amd.optim import FlatAdam
        step = FlatAdam.step

        def remembering_step(optimizer, closure=None):
            optimizer._scale_used = optimizer.grad_scale
            return step(optimizer, closure)

        monkeypatch.setattr(FlatAdam, "step", remembering_step)

    def after_step(self, side):
        if self.name == "scale":
            self.acted += side.optimizer._scale_used != 1.0
            side.optimizer.grad_scale = side.optimizer._scale_used


# defect -> (configuration, overrides, the comparison that must report it first)
SEEDED = {
    "bank": ("flat", dict(counts=(2, 2), evaluate_after=()), "flat step 1"),
    "cache": ("flat", dict(counts=(2, 2), evaluate_after=()), "flat step 1"),
    "count": ("clip-ema", dict(counts=(2, 2), evaluate_after=(), resume_after=0), "clip-ema step 1 resumed from files"),
    "lr": ("flat", dict(counts=(2, 2, 2), evaluate_after=()), "flat step 2"),
    "scale": ("flat", dict(counts=(2, 1), evaluate_after=()), "flat step 1"),
}


@pytest.mark.parametrize("defect", list(SEEDED))
def test_trajectory_catches_seeded_staleness(gpu, tmp_path, monkeypatch, defect):
    name, overrides, first = SEEDED[defect]
    cfg = dict(CONFIGS[name], **overrides)
    seeded = _Defect(defect, monkeypatch)
    violations, records = _trajectory(gpu, name, cfg, tmp_path=tmp_path, defect=seeded, write=False)
    print(f"seeded defect {defect!r} acted {seeded.acted} time(s): {violations[:3]}")
    assert seeded.acted >= 1, "the defect never had a chance to act: the case does not exercise what it breaks"
    assert violations, f"the seeded defect {defect!r} went unnoticed"
    assert all(v[0] == first for v in violations), (first, violations)
    assert not any(str(v[2]).startswith("invalid bound") for v in violations)
    # every comparison in front of it was clean: the defect is seen where it first acts, not before
    assert [r["what"] for r in records][-1] == first
