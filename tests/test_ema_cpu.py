"""The weight average (K23): what needs no GPU -- the ``--ema_decay`` flag and its checks, the warm-up
schedule, ``WeightEma`` beside a CPU optimizer against the float64 recurrence, the swap and the state dict, the three C
entries' refusals, ``trainNetwork.py --device cpu --ema_decay`` end to end, and two gloo ranks keeping equal shadows."""
import contextlib
import ctypes
import io
import math
import os
import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp
import torch.nn as nn

from conftest import ROOT


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    if not os.path.exists(os.path.join(ROOT, "fpsg_amd", "libfpsg_hip.so")):
        g.build()
    from fpsg_amd import _hip
    return _hip.load()


# ---- 1. the flag and the checks ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("evaluation", [False, True])
def test_flag_parses_and_defaults_to_off(evaluation):
    from fpsg_amd import cli
    from fpsg_amd.engine import default_options
    p = cli.few_shot_parser(evaluation=evaluation)
    base = vars(p.parse_args([]))
    assert base["ema_decay"] == 0.0 and type(base["ema_decay"]) is float
    on = vars(p.parse_args(["--ema_decay", "0.999"]))
    assert on["ema_decay"] == 0.999
    assert {k: v for k, v in on.items() if k != "ema_decay"} == {k: v for k, v in base.items() if k != "ema_decay"}
    action = next(a for a in p._actions if a.dest == "ema_decay")
    assert action.metavar == "D" and action.option_strings == ["--ema_decay"]
    assert default_options().ema_decay == 0.0


@pytest.mark.parametrize("bad", [-0.1, 1, 1.5, math.nan])
def test_validate_refuses_bad_values_and_names_the_flag(bad):
    from fpsg_amd import cli
    p = cli.few_shot_parser()
    cli.validate(p.parse_args(["--synthetic"]))
    cli.validate(p.parse_args(["--synthetic", "--ema_decay", "0.9999"]))
    opt = p.parse_args(["--synthetic"])
    opt.ema_decay = bad
    with pytest.raises(SystemExit) as e:
        cli.validate(opt)
    assert "--ema_decay" in str(e.value)


def test_check_ema_decay():
    from fpsg_amd.ema import WeightEma, check_ema_decay
    assert check_ema_decay(None) is None and check_ema_decay(0) is None and check_ema_decay(0.0) is None
    assert check_ema_decay(0.5) == 0.5 and check_ema_decay(np.float32(0.5)) == 0.5 and type(check_ema_decay(np.float32(0.5))) is float
    assert check_ema_decay(1e-9) == 1e-9 and check_ema_decay(1 - 1e-9) == 1 - 1e-9
    for bad in (True, False, "0.9", [0.9], math.nan, -0.1, -1e-30, 1, 1.0, 1.5, math.inf, -math.inf):
        with pytest.raises(ValueError, match="ema_decay"):
            check_ema_decay(bad)
    with pytest.raises(ValueError, match="my_name"):
        check_ema_decay(2, "my_name")
    params = [nn.Parameter(torch.zeros(3))]
    for bad in (0, None, 1.0, -1, math.nan, True):
        with pytest.raises(ValueError, match="decay"):
            WeightEma(params, bad)
    with pytest.raises(ValueError, match="trainable"):
        WeightEma([nn.Parameter(torch.zeros(3), requires_grad=False)], 0.9)


def test_build_optimizer_makes_the_average_only_when_asked():
    from fpsg_amd.ema import WeightEma
    from fpsg_amd.engine import build_optimizer, default_options
    net = nn.Linear(3, 2)
    for sgd in (False, True):
        o, _ = build_optimizer(net, default_options(SGD=sgd))
        assert getattr(o, "ema", None) is None
        o, _ = build_optimizer(net, default_options(SGD=sgd, ema_decay=0.75))
        assert isinstance(o.ema, WeightEma) and o.ema.decay == 0.75 and not o.ema.fused and o.ema.updates == 0
        assert "ema" not in o.state_dict() and "ema" not in o.state_dict()["param_groups"][0]
    old = default_options()
    del old.ema_decay                       # an options namespace from before the flag existed
    assert getattr(build_optimizer(net, old)[0], "ema", None) is None
    with pytest.raises(ValueError, match="ema_decay"):
        build_optimizer(net, default_options(ema_decay=1.0))


# ---- 2. schedule and recurrence ------------------------------------------------------------------------------------------

def test_schedule_is_the_closed_form():
    from fpsg_amd.ema import WeightEma, decay_at, weight_at
    decay = 0.999
    ema = WeightEma([nn.Parameter(torch.zeros(2))], decay)
    for t in range(1, 41):
        d = min(decay, (1 + t) / (10 + t))
        assert decay_at(decay, t) == d
        w = weight_at(decay, t)
        assert w == float(np.float32(1.0 - d))                    # formed in double, rounded to fp32 once
        assert ema.next_weight() == w and ema.updates == t - 1
        ema.update()
    assert decay_at(decay, 1) == 2 / 11 and decay_at(decay, 40) == 41 / 50 and decay_at(0.5, 40) == 0.5
    assert decay_at(decay, 10 ** 6) == decay and weight_at(0.5, 8) == 0.5 and weight_at(0.5, 7) == float(np.float32(1 - 8 / 17))


class _Small(nn.Module):
    """Odd sizes, a frozen parameter and BatchNorm buffers; ``loss(sample)`` as ``TrainStep`` wants it."""

    def __init__(self):
        super().__init__()
        torch.manual_seed(2)
        self.a = nn.Linear(7, 13)
        self.bn = nn.BatchNorm1d(13)
        self.b = nn.Linear(13, 5)
        self.frozen = nn.Parameter(torch.randn(3), requires_grad=False)

    def forward(self, x):
        return self.b(torch.tanh(self.bn(self.a(x)))) + self.frozen.sum()

    def loss(self, sample):
        l = (self(sample["x"]) - sample["y"]).square().sum()
        return {"ttl_loss": l, "recon_loss": l, "query_rec_loss": l, "support_rec_loss": l * 0}


def _sample(i):
    g = torch.Generator().manual_seed(50 + i)
    return {"x": torch.randn(11, 7, generator=g), "y": torch.randn(11, 5, generator=g) * 3}


@pytest.mark.parametrize("decay", [0.5, 0.9, 0.9999])
def test_weight_ema_beside_sgd_follows_the_float64_recurrence(decay):
    """``TrainStep`` calls ``ema.update()`` after ``optimizer.step()``; the shadow against e <- e + w_t (p_t - e) in float64,
    driven by the module's own fp32 parameters after each step and the same fp32 w_t.  ``lerp`` rounds at most three
    times per step (difference, product, sum), half an ulp each of a value no larger than 2 max(|p|, |e|) in magnitude:
    at most 3 * 2^-24 * 2 max(|p|, |e|); every step multiplies the earlier error by d_t < 1, so after T steps the error
    is at most 6 * min(T, 1 / (1 - decay)) * 2^-24 * max(|p|, |e|)."""
    from fpsg_amd.ema import WeightEma, weight_at
    from fpsg_amd.engine import TrainStep
    T = 12
    model = _Small().train()
    optimizer = torch.optim.SGD(model.parameters(), lr=1e-2)
    optimizer.ema = ema = WeightEma(model.parameters(), decay)
    trainable = [p for p in model.parameters() if p.requires_grad]
    assert len(ema.params) == len(trainable) == 6 and {id(p) for p in ema.params} == {id(p) for p in trainable}
    assert all(torch.equal(e, p) and e.data_ptr() != p.data_ptr() for e, p in zip(ema.shadow, ema.params))
    step = TrainStep(model, optimizer)
    e64 = [p.detach().double().clone() for p in ema.params]
    peak = [p.detach().abs().double() for p in ema.params]
    for t in range(1, T + 1):
        step([_sample(t)])
        assert ema.updates == t
        w = weight_at(decay, t)
        for e, p, big in zip(e64, ema.params, peak):
            e += w * (p.detach().double() - e)
            torch.maximum(big, torch.maximum(p.detach().abs().double(), e.abs()), out=big)
    bound = 6 * min(T, 1 / (1 - decay)) * 2.0 ** -24
    moved = 0.0
    for e, got, p, big in zip(e64, ema.shadow, ema.params, peak):
        assert bool(((got.double() - e).abs() <= bound * big).all())
        moved = max(moved, float((got - p.detach()).abs().max()))
    assert moved > 0                                                  # the average lags the weights
    # the BatchNorm buffers are no part of it
    assert sum(e.numel() for e in ema.shadow) == sum(p.numel() for p in trainable)


# ---- 3. swap and state ---------------------------------------------------------------------------------------------------

def _trained_ema(decay=0.9, steps=3):
    from fpsg_amd.ema import WeightEma
    from fpsg_amd.engine import TrainStep
    model = _Small().train()
    optimizer = torch.optim.SGD(model.parameters(), lr=1e-2)
    optimizer.ema = ema = WeightEma(model.parameters(), decay)
    step = TrainStep(model, optimizer)
    for t in range(steps):
        step([_sample(t)])
    return model, ema


def test_swapped_round_trip_is_bit_exact():
    model, ema = _trained_ema()
    raw = [p.detach().clone() for p in ema.params]
    avg = [e.clone() for e in ema.shadow]
    ptrs = [p.data_ptr() for p in ema.params]
    buffers = {k: v.clone() for k, v in model.named_buffers()}
    assert any(not torch.equal(a, b) for a, b in zip(raw, avg))
    model.eval()
    x = _sample(9)["x"]
    with torch.no_grad():
        before = model(x)
        with ema.swapped() as inside:
            assert inside is ema
            assert all(torch.equal(p.detach(), a) for p, a in zip(ema.params, avg))
            assert all(torch.equal(e, r) for e, r in zip(ema.shadow, raw))
            assert [p.data_ptr() for p in ema.params] == ptrs         # contents move, addresses do not
            assert not torch.equal(model(x), before)
            with pytest.raises(RuntimeError, match="swapped"):
                with ema.swapped():
                    pass
            with pytest.raises(RuntimeError, match="swapped"):
                ema.update()
        assert torch.equal(model(x), before)
    assert all(torch.equal(p.detach(), r) for p, r in zip(ema.params, raw))
    assert all(torch.equal(e, a) for e, a in zip(ema.shadow, avg))
    assert all(torch.equal(v, buffers[k]) for k, v in model.named_buffers())
    assert torch.equal(model.frozen, _Small().frozen)
    # exchanged back when the block raises
    with pytest.raises(KeyError):
        with ema.swapped():
            raise KeyError("x")
    assert all(torch.equal(p.detach(), r) for p, r in zip(ema.params, raw))
    assert all(torch.equal(e, a) for e, a in zip(ema.shadow, avg))


def test_swapped_refuses_to_start_inside_weights_frozen():
    from fpsg_amd import winograd
    model, ema = _trained_ema()
    raw = [p.detach().clone() for p in ema.params]
    with winograd.weights_frozen():
        with pytest.raises(RuntimeError, match="weights_frozen"):
            with ema.swapped():
                pass
    assert all(torch.equal(p.detach(), r) for p, r in zip(ema.params, raw))      # nothing was exchanged
    with ema.swapped():                                                           # blocks are opened inside it instead
        with winograd.weights_frozen():
            assert winograd.frozen_cache_ro() is not None
    assert winograd.frozen_cache_ro() is None


def test_state_dict_round_trip(tmp_path):
    from fpsg_amd.ema import WeightEma
    model, ema = _trained_ema(decay=0.9, steps=4)
    sd = ema.state_dict()
    assert set(sd) == {"decay", "updates", "shadow"} and sd["decay"] == 0.9 and sd["updates"] == 4
    assert list(sd["shadow"]) == list(range(len(ema.params)))
    assert all(sd["shadow"][i].shape == p.shape for i, p in enumerate(ema.params))
    torch.save({"ema": sd}, tmp_path / "s.pt")
    loaded = torch.load(tmp_path / "s.pt", weights_only=True)["ema"]
    fresh = WeightEma(_Small().parameters(), 0.9)
    assert fresh.updates == 0 and any(not torch.equal(a, b) for a, b in zip(fresh.shadow, ema.shadow))
    fresh.load_state_dict(loaded)
    assert fresh.updates == 4 and fresh.next_weight() == ema.next_weight()
    assert all(torch.equal(a, b) for a, b in zip(fresh.shadow, ema.shadow))
    short = dict(loaded, shadow={0: loaded["shadow"][0]})
    with pytest.raises(ValueError, match="shadow"):
        fresh.load_state_dict(short)
    wrong = dict(loaded, shadow=dict(loaded["shadow"]))
    wrong["shadow"][0] = torch.zeros(2, 2)
    with pytest.raises(ValueError, match="shape"):
        fresh.load_state_dict(wrong)


# ---- 4. the C entries ------------------------------------------------------------------------------------------------------

def test_symbols_are_exported_and_bound(lib):
    from fpsg_amd import _hip
    header = open(os.path.join(ROOT, "include", "fpsg_hip.h")).read()
    for name, nargs in (("fpsg_adam_step_ema", 15), ("fpsg_adam_step_segments_ema", 17), ("fpsg_flat_swap", 4)):
        assert f"int {name}(" in header
        assert name in _hip.SIGNATURES and len(_hip.SIGNATURES[name]) == nargs
        fn = getattr(lib, name)
        assert fn.argtypes == _hip.SIGNATURES[name] and fn.restype is ctypes.c_int


def test_entries_check_their_arguments_on_the_host(lib):
    """Every refusal with its own code and a message that names the entry, before any HIP call (no GPU here)."""
    f = ctypes.c_float
    P, G, M, V, E = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000      # never dereferenced
    null, shape, align = -1, -2, -3
    hyper = (f(1e-3), f(0.9), f(0.999), f(1e-8))

    def flat(param=P, grad=G, m=M, v=V, ema=E, n=8, step=1, scale_dev=None, w=0.1):
        return lib.fpsg_adam_step_ema(param, grad, m, v, ema, n, *hyper, step, f(1.0), scale_dev, f(w), None)

    def seg(param=P, grad=G, m=M, v=V, ema=E, n=8, step=1, scale_dev=None, w=0.1, nseg=2):
        return lib.fpsg_adam_step_segments_ema(param, grad, G + 0x100, nseg, m, v, ema, n, *hyper, step, f(1.0), scale_dev,
                                               f(w), None)

    for call, name in ((flat, b"fpsg_adam_step_ema"), (seg, b"fpsg_adam_step_segments_ema")):
        def refused(code, word, **kw):
            assert call(**kw) == code, (name, kw)
            msg = lib.fpsg_last_error()
            assert msg and name in msg and word in msg, (name, kw, msg)
        # the step's own checks
        refused(shape, b"n", n=0)
        refused(shape, b"step", step=0)
        refused(null, b"param", param=None)
        refused(align, b"16-byte", param=P + 4)
        refused(null, b"", grad=None)
        # the shadow
        refused(null, b"ema", ema=None)
        refused(align, b"ema", ema=E + 2)
        refused(align, b"ema", ema=E + 4)
        refused(align, b"ema", ema=E + 8)
        refused(shape, b"ema", ema=P)
        refused(shape, b"ema", ema=M)
        refused(shape, b"ema", ema=V)
        for w in (0.0, -0.1, 1.5, math.nan, math.inf, -math.inf):
            refused(shape, b"ema_weight", w=w)
        # a weight of 1 and a tiny one pass: the call gets as far as the check behind them
        refused(align, b"grad_scale_dev", w=1.0, scale_dev=0x60002)
        refused(align, b"grad_scale_dev", w=1e-30, scale_dev=0x60002)
    assert flat(grad=G + 4) == align
    assert seg(nseg=0) == shape and seg(nseg=-1) == shape

    def swap(a=P, b=G, n=8):
        return lib.fpsg_flat_swap(a, b, n, None)

    for code, word, kw in ((shape, b"n must be positive", {"n": 0}), (null, b"'a'", {"a": None}), (null, b"'b'", {"b": None}),
                           (align, b"aligned", {"a": P + 4}), (align, b"aligned", {"b": G + 8}), (align, b"aligned", {"b": G + 2}),
                           (shape, b"same buffer", {"b": P})):
        assert swap(**kw) == code, kw
        msg = lib.fpsg_last_error()
        assert msg and b"fpsg_flat_swap" in msg and word in msg, (kw, msg)
    # the entries without a shadow answer as before
    assert lib.fpsg_adam_step(None, G, M, V, 8, *hyper, 1, f(1.0), None) == null
    assert b"fpsg_adam_step: null pointer 'param'" in lib.fpsg_last_error()


def test_flat_adam_attach_needs_its_own_parameters():
    """(``FlatAdam`` itself needs a GPU; what ``attach_ema`` refuses is checked on an object made without one.)"""
    from fpsg_amd.ema import WeightEma
    from fpsg_amd.optim import FlatAdam
    a, b = nn.Parameter(torch.zeros(3)), nn.Parameter(torch.zeros(3))
    o = FlatAdam.__new__(FlatAdam)
    o.ema, o._layout = None, [(a, 0, 3)]
    with pytest.raises(ValueError, match="trainable parameters"):
        o.attach_ema(WeightEma([b], 0.5))
    with pytest.raises(ValueError, match="trainable parameters"):
        o.attach_ema(WeightEma([a, b], 0.5))
    o.ema = object()
    with pytest.raises(RuntimeError, match="already"):
        o.attach_ema(WeightEma([a], 0.5))


# ---- 5. the entry point on the CPU ---------------------------------------------------------------------------------------

def _train(monkeypatch, oracle, ck, argv):
    """``trainNetwork.main`` in this process, the Chamfer loss through the CPU oracle (tests/test_entrypoints_cpu.py)."""
    import trainNetwork
    from fpsg_amd import cli
    build = trainNetwork.build_model

    def build_model(opt):
        model = build(opt)
        model.pc_metric = oracle.make_torch_chamfer()
        return model

    monkeypatch.setattr(trainNetwork, "build_model", build_model)
    opt = cli.few_shot_parser().parse_args(["--synthetic", "--device", "cpu", "--n_shot", "1", "--n_query", "1",
                                            "--n_episode", "2", "--model_path", ck] + argv)
    out = io.StringIO()
    threads = torch.get_num_threads()
    try:
        with contextlib.redirect_stdout(out):
            trainNetwork.main(opt)
    finally:
        torch.set_num_threads(threads)
    return out.getvalue()


def test_train_network_on_the_cpu_with_and_without_the_flag(monkeypatch, oracle, tmp_path):
    ck = str(tmp_path)
    out = _train(monkeypatch, oracle, ck, ["--epoch", "2", "--name", "on", "--ema_decay", "0.9"])
    files = os.listdir(os.path.join(ck, "on"))
    assert "model_epoch_2.pt" in files and "model_epoch_2_ema.pt" in files and "train_state_epoch_2.pt" in files
    raw = torch.load(os.path.join(ck, "on", "model_epoch_2.pt"), weights_only=True)
    avg = torch.load(os.path.join(ck, "on", "model_epoch_2_ema.pt"), weights_only=True)
    assert list(raw) == list(avg) and all(raw[k].shape == avg[k].shape for k in raw)
    differ = [k for k in raw if not torch.equal(raw[k], avg[k])]
    assert differ and not any("running_" in k or "num_batches" in k for k in differ)     # the live BatchNorm buffers
    state = torch.load(os.path.join(ck, "on", "train_state_epoch_2.pt"), weights_only=True)
    assert set(state) == {"optimizer", "scheduler", "epoch", "ema"}
    assert state["ema"]["decay"] == 0.9 and state["ema"]["updates"] == 4                 # 2 epochs of 2 one-episode steps
    lines = out.splitlines()
    plain = [l for l in lines if l.startswith("Class: ")]
    marked = [l for l in lines if l.startswith("[EMA] Class: ")]
    assert plain and len(marked) == len(plain)
    assert [l.split(" -- ")[0] for l in marked] == ["[EMA] " + l.split(" -- ")[0] for l in plain]     # the same test items
    assert sum(l.startswith("[EMA] Avg testing results across all classes Epoch -- 2 are: Query_rec:") for l in lines) == 1
    assert sum(l.startswith("Avg testing results across all classes Epoch -- 2 are: Query_rec:") for l in lines) == 1
    log = open(os.path.join(ck, "on", next(f for f in files if f.startswith("log_")))).read()
    assert "[EMA] Class: " in log and "[EMA] Avg testing results" in log
    del raw, avg

    # a resumed run restores the shadow and its count
    out3 = _train(monkeypatch, oracle, ck, ["--epoch", "3", "--resume", "2", "--name", "on", "--ema_decay", "0.9"])
    assert "EMA restored after 4 updates" in out3 and "EMA started from" not in out3
    state3 = torch.load(os.path.join(ck, "on", "train_state_epoch_3.pt"), weights_only=True)
    assert state3["ema"]["updates"] == 6
    before, after = state["ema"]["shadow"], state3["ema"]["shadow"]
    assert list(before) == list(after) and any(not torch.equal(before[i], after[i]) for i in before)
    del state, state3

    # without the flag: neither the file nor the key nor the prefix -- and a sidecar's entry is ignored
    off = _train(monkeypatch, oracle, ck, ["--epoch", "3", "--resume", "2", "--name", "on"])
    assert "[EMA]" not in off and "EMA" not in off
    state_off = torch.load(os.path.join(ck, "on", "train_state_epoch_3.pt"), weights_only=True)
    assert set(state_off) == {"optimizer", "scheduler", "epoch"}
    del state_off
    out_off = _train(monkeypatch, oracle, ck, ["--epoch", "1", "--name", "off"])
    files = os.listdir(os.path.join(ck, "off"))
    assert "model_epoch_1.pt" in files and not any("ema" in f for f in files)
    assert "EMA" not in out_off and "Class: " in out_off
    assert "ema" not in torch.load(os.path.join(ck, "off", "train_state_epoch_1.pt"), weights_only=True)
    # the flag on, a sidecar without an entry: the shadow starts from the loaded weights
    late = _train(monkeypatch, oracle, ck, ["--epoch", "2", "--resume", "1", "--name", "off", "--ema_decay", "0.9"])
    assert "EMA started from the resumed weights" in late
    assert torch.load(os.path.join(ck, "off", "train_state_epoch_2.pt"), weights_only=True)["ema"]["updates"] == 2


# ---- 6. two gloo ranks -------------------------------------------------------------------------------------------------------

def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _run_rank(rank, world, port, out_dir):
    os.environ.update(RANK=str(rank), LOCAL_RANK=str(rank), WORLD_SIZE=str(world),
                      MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    from fpsg_amd import dist as fdist
    from fpsg_amd.engine import TrainStep, build_optimizer, default_options
    fdist.init_distributed("cpu")
    model = _Small().train()
    if rank != 0:                              # ranks start different, the broadcast fixes it
        with torch.no_grad():
            for p in model.parameters():
                p.add_(1.0)
    fdist.broadcast_parameters(model, src=0)
    optimizer, _ = build_optimizer(model, default_options(device="cpu", SGD=True, lr=1e-2, ema_decay=0.9))
    step = TrainStep(model, optimizer, world=world)
    for t in range(3):                         # every rank its own episode, the gradients averaged
        step([_sample(10 * t + rank)], n_episodes_global=world)
    torch.save({"shadow": [e.clone() for e in optimizer.ema.shadow], "updates": optimizer.ema.updates,
                "params": [p.detach().clone() for p in optimizer.ema.params]}, os.path.join(out_dir, f"ema{rank}.pt"))
    fdist.shutdown()


def test_two_ranks_keep_equal_shadows(tmp_path):
    """Every rank keeps its own shadow and nothing is communicated: equal parameters and a deterministic update."""
    mp.spawn(_run_rank, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
    a = torch.load(tmp_path / "ema0.pt", weights_only=True)
    b = torch.load(tmp_path / "ema1.pt", weights_only=True)
    assert a["updates"] == b["updates"] == 3
    for x, y in zip(a["shadow"], b["shadow"]):
        assert torch.equal(x, y)
    assert any(not torch.equal(e, p) for e, p in zip(a["shadow"], a["params"]))
