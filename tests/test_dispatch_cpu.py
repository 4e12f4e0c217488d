"""Pins ``tests/_dispatch.py``, the inventory of launch-time kernel choices: every dispatch line still stands in its
source, every named GPU test exists, the shapes of the named cases satisfy the condition restated next to the row, and
(where the trace was kept) every instantiation was seen running under the named cases.  A threshold that moves, a test
that is renamed or a shape that leaves its branch turns this file red; nothing here needs a GPU."""
import os
import subprocess
import sys

import pytest

from conftest import ROOT

import _dispatch

CSRC = os.path.join(ROOT, "fpsg_amd", "csrc")
KERNELS = os.path.join(ROOT, "profiles", "dispatch", "kernels.txt")
IDS = [f"{r['file']}:{r['entry']}:{r['kernel']}" for r in _dispatch.ROWS]


@pytest.fixture(scope="module")
def sources():
    out = {}
    for name in {r["file"] for r in _dispatch.ROWS}:
        with open(os.path.join(CSRC, name)) as fh:
            out[name] = fh.read()
    return out


@pytest.fixture(scope="module")
def collected():
    """The node ids of the test files the inventory names, from one ``pytest --collect-only`` in a child process."""
    files = sorted({case[0].split("::")[0] for r in _dispatch.ROWS for case in r["cases"]})
    res = subprocess.run([sys.executable, "-m", "pytest", "--collect-only", "-q", "-p", "no:cacheprovider"] + files,
                         cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-3000:]
    return {ln.strip() for ln in res.stdout.splitlines() if "::" in ln}


def test_rows_are_complete_and_unique():
    assert len(set(IDS)) == len(IDS), "one row per entry and instantiation"
    for r in _dispatch.ROWS:
        assert r["entry"].startswith("fpsg_") and r["kernel"] and r["when"] and r["lines"], r
        if r["cases"]:
            assert "uncovered" not in r, f"{r['kernel']}: a covered row carries no excuse"
        else:       # only with the technical reason why no test of the suite can reach it
            assert len(r.get("uncovered", "")) > 40, \
                f"{r['entry']}: {r['kernel']} has no GPU test with a reference comparison"


def test_every_source_file_is_accounted_for():
    hip = {n for n in os.listdir(CSRC) if n.endswith(".hip")}
    groups = [{r["file"] for r in _dispatch.ROWS}, set(_dispatch.FILES_WITHOUT_A_CHOICE)]
    assert set().union(*groups) == hip, sorted(set().union(*groups) ^ hip)
    assert sum(len(g) for g in groups) == len(hip), "a file stands in one group only"


@pytest.mark.parametrize("r", _dispatch.ROWS, ids=IDS)
def test_dispatch_lines_stand_in_the_source(sources, r):
    for line in r["lines"]:
        assert line in sources[r["file"]], f"{r['file']}: no longer reads\n    {line}"


@pytest.mark.parametrize("r", _dispatch.ROWS, ids=IDS)
def test_named_tests_exist(collected, r):
    for test_id, _ in r["cases"]:
        assert test_id in collected, test_id


@pytest.mark.parametrize("r", [r for r in _dispatch.ROWS if r["cond"]], ids=[i for i, r in zip(IDS, _dispatch.ROWS) if r["cond"]])
def test_shapes_of_the_named_cases_take_the_branch(r):
    shaped = [(t, s) for t, s in r["cases"] if s is not None]
    assert shaped, "an arithmetic condition needs the shape of at least one case"
    for test_id, shape in shaped:
        assert eval(r["cond"], {"__builtins__": {}, "max": max}, dict(shape)), (r["kernel"], r["cond"], test_id, shape)


def test_conditions_of_one_dispatch_exclude_each_other():
    """The rows of one dispatch (one entry and one kernel template, or one ``group`` where an entry dispatches the same
    template at several places) partition the shapes: a case of one row fails every other row's condition.  Rows whose
    conditions read other names than the case's shape has (the byte thresholds next to the size ranges) are not
    compared."""
    rows = [r for r in _dispatch.ROWS if r["cond"]]
    group = lambda r: (r["entry"], r.get("group", r["kernel"].split("<")[0]))
    for a in rows:
        for b in rows:
            if a is b or group(a) != group(b):
                continue
            for test_id, shape in a["cases"]:
                if shape is None:
                    continue
                try:
                    other = eval(b["cond"], {"__builtins__": {}, "max": max}, dict(shape))
                except NameError:
                    continue
                assert not other, (a["kernel"], b["kernel"], shape)


def test_every_instantiation_ran_under_the_named_cases():
    """``kernels.txt`` is the set of kernel names of one trace of exactly the cases the rows name (not of their whole
    files): a row's instantiation occurs there only if one of the named cases of some row launched it.  It does not
    tell which case did; that is what ``cond`` and the shapes are for."""
    if not os.path.exists(KERNELS):
        pytest.skip("profiles/dispatch/kernels.txt was not recorded: no kernel trace of the named cases")
    with open(KERNELS) as fh:
        seen = [ln.split("::")[-1] for ln in fh.read().splitlines()]
    for r in _dispatch.ROWS:
        if r["cases"]:
            assert any(ln.startswith(r["kernel"]) for ln in seen), f"{r['kernel']} is not in the kernel trace"
