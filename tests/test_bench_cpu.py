"""What a plain ``bench.py`` run executes and what only ``--full`` adds: ``bench.main`` with every measurement replaced
by a recorder, so the dispatch is checked without a device."""
import json
import sys

import pytest
import torch

import bench


@pytest.fixture
def fake_bench(monkeypatch, capsys):
    calls = []

    def run_workload(wl, args, rank, world, device, steps, warmup, probe=None, graph=None, epr=None, dump_dir=None,
                     full=False):
        calls.append(("run_workload", wl, full))
        return {"value": 40.0, "elapsed": steps / 5.0, "steps": steps, "warmup": warmup, "epr": 8, "graph": False,
                "loss": 1.0, "desc": wl, "params": 1, "step": None, "ranks_seen": 1, "clock": {}, "mfu": {"note": ""}}

    def recorder(name):
        return lambda *a, **k: calls.append((name,)) or {}

    monkeypatch.setattr(bench, "run_workload", run_workload)
    for name in ("cpu_baseline", "kernel_rooflines", "eval_leg", "allreduce_probe", "split_gemm_error"):
        monkeypatch.setattr(bench, name, recorder(name))
    monkeypatch.setattr(bench.fdist, "init_distributed", lambda *a: (0, 1, torch.device("cpu")))
    monkeypatch.setattr(bench.gemm_tuning, "enable", lambda **k: {})
    monkeypatch.setattr(bench.metrics, "set_launch_probe", lambda probe: None)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    monkeypatch.setattr(torch.cuda, "max_memory_allocated", lambda *a: 0)
    monkeypatch.setattr(torch.cuda, "empty_cache", lambda: None)
    monkeypatch.setattr(torch.backends.cudnn, "benchmark", torch.backends.cudnn.benchmark)
    monkeypatch.delenv("FPSG_FORCE_DIST", raising=False)
    monkeypatch.delenv("FPSG_GEMM_SPLIT", raising=False)

    def run(*argv, force_dist=False):
        calls.clear()
        if force_dist:
            monkeypatch.setenv("FPSG_FORCE_DIST", "1")
        else:
            monkeypatch.delenv("FPSG_FORCE_DIST", raising=False)
        monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "4", "--warmup", "2", *argv])
        bench.main()
        lines = [l for l in capsys.readouterr().out.splitlines() if l.startswith("{")]
        assert len(lines) == 1
        return json.loads(lines[0]), list(calls)

    return run


def test_plain_run_times_the_workload_and_nothing_else(fake_bench):
    line, calls = fake_bench()
    assert calls == [("run_workload", "c5", False)]
    assert line["value"] == 40.0 and line["unit"] == "episodes/s" and line["higher_is_better"] is True
    assert line["dtype"] == "f32" and line["ms_per_step"] == pytest.approx(200.0)
    assert "cpu_baseline" not in line and "configs" not in line and "allreduce" not in line
    # the skip switches of --full change nothing in a plain run
    assert fake_bench("--no-extra", "--no-cpu-baseline")[1] == calls
    assert fake_bench(force_dist=True)[1] == calls


def test_full_run_adds_every_leg(fake_bench):
    line, calls = fake_bench("--full")
    names = [c[0] for c in calls]
    assert calls[0] == ("run_workload", "c5", True)
    assert [c[1] for c in calls if c[0] == "run_workload"][1:] == ["c2", "c3", "c4", "c5"]
    assert {"split_gemm_error", "eval_leg", "kernel_rooflines", "cpu_baseline"} <= set(names)
    assert "cpu_baseline" in line and set(line["configs"]) == {"c2", "c3", "c4", "c5_split", "eval"}
    assert "allreduce_probe" not in names
    assert fake_bench("--full", "--no-extra", "--no-cpu-baseline")[1] == [("run_workload", "c5", True)]
    line, calls = fake_bench("--full", "--no-extra", "--no-cpu-baseline", force_dist=True)
    assert calls == [("run_workload", "c5", True), ("allreduce_probe",)] and "allreduce" in line
