"""The memory contract of every workspace-taking entry of include/fpsg_hip.h, on the GPU.

Every case of tests/_memory_contract.py runs its entry five times: in a guarded arena (tests/_guarded.py: every buffer
at exactly its documented alignment and size, 64 KiB guard zones, the workspace exactly what the size function
returned) filled with 0xFF bytes, with zeros and with random bytes, once in a roomy layout (own zeroed allocations,
256-byte aligned, twice the workspace) and once more under the first fill.  Asserted, with no tolerance anywhere:
  1. every call returns 0 -- FPSG_E_ALIGN at the documented alignment would be a failure of the header or the check;
  2. every guard zone and every pure-input region is unchanged;
  3. every output element is bit-identical across the five runs: the result depends neither on what the workspace or
     the outputs held before, nor on the bytes beyond the inputs, nor on alignment or spare room; the call is
     repeatable; and every output element is written (an unwritten one would differ between the 0xFF and zero fills).
The workspace may end in any state (its contents are unspecified); only its guards are checked.
Every call is one the header documents as valid, with buffers of the documented size: nothing here is meant to fault.
"""
import pytest
import torch

import _guarded as G
import _memory_contract as T

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    from fpsg_amd import _hip
    return _hip.load()


def _run(row, layout, scale, lib):
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


@pytest.mark.parametrize("case", T.CASES, ids=[c[0] for c in T.CASES])
def test_memory_contract(gpu, lib, case):
    row = T.build(case, lib)
    runs = []
    for i, pattern in enumerate(G.PATTERNS):
        runs.append((pattern, _run(row, G.Arena(row.bufs, pattern, gpu, seed=17 + i), 1, lib)))
    runs.append(("roomy", _run(row, G.Roomy(row.bufs, gpu), 2, lib)))
    runs.append(("ff again", _run(row, G.Arena(row.bufs, G.PATTERNS[0], gpu), 1, lib)))
    name0, ref = runs[0]
    sizes = {b.name: torch.empty((), dtype=b.dtype).element_size() for b in row.bufs}
    for name, outs in runs[1:]:
        for buf, bits in outs.items():
            at = G.first_difference(ref[buf], bits, sizes[buf])
            assert at is None, f"output '{buf}' differs between the '{name0}' and '{name}' runs, first at element {at}"
