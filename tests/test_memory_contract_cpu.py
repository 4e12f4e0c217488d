"""Host half of the memory-contract tests: the guarded arena itself, the coverage of the contract
table against include/fpsg_hip.h, and what the size functions and the entries' own size checks answer.  No GPU: the
library loads without one and every call here is refused on the host before any launch."""
import os
import re

import pytest
import torch

import _guarded as G
import _memory_contract as T
from conftest import ROOT

FPSG_E_SHAPE = -2


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    if not os.path.exists(os.path.join(ROOT, "fpsg_amd", "libfpsg_hip.so")):
        g.build()
    from fpsg_amd import _hip
    return _hip.load()


# ---- the arena ------------------------------------------------------------------------------------------------------
def _bufs():
    g = torch.Generator().manual_seed(0)
    return [G.inp("a", torch.randn(7, 3, generator=g)),                         # 4-byte aligned by the general rule
            G.inp("tab", torch.arange(5, dtype=torch.int64), 8),
            G.out("y", torch.float32, (33,), 16),
            G.inout("acc", torch.arange(3, dtype=torch.int32)),
            G.out("img", torch.uint8, (5, 3)),
            G.ws("ws", 1001, 8),
            G.ws("none", 0, 4)]


@pytest.mark.parametrize("pattern", G.PATTERNS)
def test_arena_layout_is_exact(pattern):
    bufs = _bufs()
    a = G.Arena(bufs, pattern)
    spans = []
    for b in bufs:
        if b.nbytes == 0:
            assert a.ptr(b) is None                                  # a buffer of no bytes is passed as NULL
            continue
        p = a.ptr(b)
        assert p % b.align == 0 and p % (2 * b.align) != 0, (b.name, p)   # the documented alignment and no stricter one
        assert a.raw(b).numel() == b.nbytes                          # exactly the documented size
        spans.append((a.off[b.name], a.off[b.name] + b.nbytes))
    assert G.GUARD >= 64 * 1024
    spans.sort()
    assert spans[0][0] >= G.GUARD and a.mem.numel() - spans[-1][1] >= G.GUARD
    for (_, e0), (o1, _) in zip(spans, spans[1:]):
        assert o1 - e0 >= G.GUARD                                    # a guard zone between any two regions
    # the fill reached the payload too: outputs and the workspace hold the pattern, inputs their data
    want = {"ff": 0xFF, "zero": 0}.get(pattern)
    for b in bufs:
        if b.role in (G.OUT, G.WS) and b.nbytes:
            raw = a.raw(b)
            assert bool((raw == want).all()) if want is not None else raw.unique().numel() > 8
        if b.role in (G.IN, G.INOUT):
            assert torch.equal(a.region(b), b.data)
    a.check()                                                        # untouched: passes
    # writes where a call may write are no violation
    a.region(bufs[2]).fill_(1.0)
    a.region(bufs[3]).add_(1)
    a.raw(bufs[5]).fill_(7)
    a.check()
    outs = a.outputs()
    assert set(outs) == {"y", "acc", "img"} and outs["y"].numel() == 33 * 4


@pytest.mark.parametrize("pattern", G.PATTERNS)
@pytest.mark.parametrize("target, where, names", [
    ("y", "before", "in front of 'y'"), ("y", "after", "behind 'y'"),
    ("ws", "before", "in front of 'ws'"), ("ws", "after", "behind 'ws'"),
    ("img", "after", "behind 'img'"), ("acc", "before", "in front of 'acc'"),
    ("a", "inside", "input 'a'"), ("tab", "inside", "input 'tab'"),
])
def test_arena_reports_a_one_byte_write(pattern, target, where, names):
    bufs = _bufs()
    a = G.Arena(bufs, pattern)
    b = next(x for x in bufs if x.name == target)
    at = {"before": a.off[target] - 1, "after": a.off[target] + b.nbytes, "inside": a.off[target] + b.nbytes - 1}[where]
    a.mem[at] = a.mem[at] ^ 0x5A
    msg = a.violation()
    assert msg is not None and names in msg, msg
    if where == "inside":
        assert f"byte {b.nbytes - 1} of {b.nbytes}" in msg, msg
    else:
        assert ("1 bytes in front of" in msg) if where == "before" else ("0 bytes behind" in msg), msg
    with pytest.raises(AssertionError):
        a.check()


def test_arena_late_inputs_and_roomy_layout():
    bufs = _bufs()
    a = G.Arena(bufs, "ff")
    a.poke("tab", torch.full((5,), 9, dtype=torch.int64))
    a.check()                                                        # a late input becomes part of the image
    assert int(a.region(bufs[1])[4]) == 9
    r = G.Roomy(bufs)
    for b in bufs:
        if b.nbytes:
            assert r.ptr(b) % 256 == 0
            assert r.t[b.name][0].numel() - r.t[b.name][1] >= b.nbytes * (2 if b.role == G.WS else 1)
        else:
            assert r.ptr(b) is None
        if b.role == G.IN:
            assert torch.equal(r.region(b), b.data)
        elif b.nbytes and b.role != G.INOUT:
            assert not bool(r.region(b).any())                       # zeroed
    # an unspecified part is masked out of the comparison, and only with the header line that leaves it open
    m = torch.zeros(33, dtype=torch.bool)
    m[5] = True
    y = G.out("y", torch.float32, (33,), 16, unspecified=m, why="header: '...'")
    a1, a2 = G.Arena([y], "ff"), G.Arena([y], "zero")
    a1.region(y).fill_(2.0)
    a2.region(y).fill_(2.0)
    a2.region(y)[5] = 3.0
    assert G.first_difference(a1.outputs()["y"], a2.outputs()["y"], 4) is None
    a2.region(y)[6] = 3.0
    assert G.first_difference(a1.outputs()["y"], a2.outputs()["y"], 4) == 6


# ---- coverage cannot drift ------------------------------------------------------------------------------------------------
def _workspace_entries():
    """Every `int fpsg_*` entry of include/fpsg_hip.h with a parameter named ws or workspace."""
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fpsg_hip.h")).read(), flags=re.S)
    found = set()
    for name, params in re.findall(r"\bint\s+(fpsg_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", txt):
        names = [re.sub(r"\[.*", "", p).split()[-1].lstrip("*") for p in params.split(",") if p.strip() and p.strip() != "void"]
        if "ws" in names or "workspace" in names:
            found.add(name)
    return found


def test_contract_table_matches_header():
    scanned = _workspace_entries()
    assert "fpsg_knn" in scanned and "fpsg_repulsion_fwd" in scanned and "fpsg_chamfer_fwd" not in scanned
    assert len(scanned) >= 40
    queries = [n for n in scanned if re.search(r"_workspace_|_fits$|_blocks$|_parts$", n) and n != "fpsg_bn_act_bwd_parts"]
    assert not queries, queries                                      # pure queries take no workspace
    table = set(T.ENTRIES)
    assert set(T.NO_WORKSPACE) <= table and not (set(T.NO_WORKSPACE) & scanned)
    assert not (set(T.EXCLUDED) & table)
    assert all(reason.strip() for reason in T.EXCLUDED.values())
    assert scanned == (table - set(T.NO_WORKSPACE)) | set(T.EXCLUDED), (
        f"workspace-taking entries without a row or a commented exclusion: {sorted(scanned - table - set(T.EXCLUDED))}; "
        f"rows or exclusions without such an entry: {sorted(((table - set(T.NO_WORKSPACE)) | set(T.EXCLUDED)) - scanned)}")
    ids = [c[0] for c in T.CASES]
    assert len(ids) == len(set(ids))
    for entry in T.ENTRIES:
        assert sum(c[1] == entry for c in T.CASES) >= 2, entry      # two or three shapes per entry


# ---- size functions and refusals --------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", T.CASES, ids=[c[0] for c in T.CASES])
def test_size_function_and_refusal(lib, case):
    row = T.build(case, lib)
    wsb = [b for b in row.bufs if b.name == "ws"]
    if case[1] in T.NO_WORKSPACE:
        assert not wsb and row.ws_units == 0
        return
    assert len(wsb) == 1 and wsb[0].role == G.WS and wsb[0].nbytes % max(row.ws_units, 1) == 0
    if row.needs_ws:
        assert row.ws_units > 0, "the size function answers 0 for a shape of the table"
    else:
        assert row.ws_units >= 0                                      # the header says this entry may need none
    for b in row.bufs:
        if b.role in (G.IN, G.INOUT):
            assert b.data is not None and b.data.dtype == b.dtype and tuple(b.data.shape) == b.shape, b.name
        if b.role == G.INOUT:
            assert b.why, f"{b.name}: an in/out buffer cites its header line"
    if not (row.refuses and row.size_arg and row.ws_units > 0):
        return
    # one unit short: refused on the host with FPSG_E_SHAPE before any launch (fake non-null, well-aligned pointers;
    # host arrays such as K25's percentages are real)
    fake = {b.name: (0x100000 * (i + 1) if b.nbytes else None) for i, b in enumerate(row.bufs)}
    rc = row.call(fake, None, row.ws_units - 1)
    assert rc == FPSG_E_SHAPE, (rc, lib.fpsg_last_error())
