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

import _memory_contract as T

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    from fpsg_amd import _hip
    return _hip.load()


@pytest.mark.parametrize("case", T.CASES, ids=[c[0] for c in T.CASES])
def test_memory_contract(gpu, lib, case):
    T.five_runs(case, lib, gpu)     # the procedure above; tests/test_streaming_forms_gpu.py runs it on the second build
