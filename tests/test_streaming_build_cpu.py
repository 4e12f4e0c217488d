"""The second build of the HIP library (fpsg_amd/csrc/Makefile: build/libfpsg_hip_stream.so, every pass in its streaming
form) covers what it claims to cover: every source that reads the byte threshold is compiled twice, the threshold has one
home, and the second library has the whole C ABI.  Nothing here needs a GPU."""
import ctypes
import os
import re

from conftest import ROOT

import _stream_lib

CSRC = os.path.join(ROOT, "fpsg_amd", "csrc")
HOME = "fpsg_common.h"          # defines FPSG_NT_BYTES and beyond_cache()


def _sources():
    return {n: open(os.path.join(CSRC, n)).read() for n in sorted(os.listdir(CSRC)) if n.endswith((".hip", ".h"))}


def _make_list(name):
    text = open(os.path.join(CSRC, "Makefile")).read()
    m = re.search(rf"^{name}\s*:=\s*(.*)$", text, flags=re.M)
    assert m, f"the Makefile no longer defines {name}"
    return m.group(1).split()


def _code(text):
    """The source without its comments."""
    return re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", text, flags=re.S))


def test_every_source_that_reads_the_threshold_is_compiled_twice():
    twice = set(_make_list("STREAM_SRCS"))
    assert twice <= set(_make_list("SRCS"))
    readers = {n for n, text in _sources().items() if re.search(r"\bbeyond_cache\b|\bFPSG_NT_BYTES\b", _code(text))}
    assert HOME in readers, f"{HOME} no longer defines the threshold"
    assert readers - {HOME} == twice, (f"read the threshold but are compiled once: {sorted(readers - {HOME} - twice)}; "
                                       f"compiled twice without reading it: {sorted(twice - readers)}")
    make = open(os.path.join(CSRC, "Makefile")).read()
    assert "-DFPSG_NT_BYTES=0" in make and "-Wl,-Bsymbolic" in make
    assert re.search(r"^all:.*\$\(STREAM_OUT\)", make, flags=re.M), "`make` no longer builds the second library"


def test_no_source_keeps_a_byte_threshold_of_its_own():
    """The streaming forms are template arguments (``NT``, or a literal ``true`` in a launch) chosen by
    ``beyond_cache()`` alone: no MiB constant (``<< 20``) of any source but the header stands in a line that chooses
    or names such a form, and no source but the header defines or compares against a byte size of its own to choose one
    (the one other ``<< 20`` of the library, the swap kernel's grid cap in adam.hip, chooses nothing)."""
    for name, text in _sources().items():
        if name == HOME:
            assert re.search(r"#ifndef FPSG_NT_BYTES\s*\n#define FPSG_NT_BYTES \(\(size_t\)300 << 20\)\s*\n#endif", text), \
                "the shipped threshold is 300 MiB, overridable at compile time only"
            continue
        code = _code(text)
        consts = set(re.findall(r"constexpr\s+\w+\s+(\w+)\s*=[^;]*<<\s*20", code))
        for line in code.splitlines():
            chooses = re.search(r"\bNT\b|\bnt\b|beyond_cache|, true>|<true>|Stream|stream_(load|store)|[ls][dt]_stream", line)
            if not chooses:
                continue
            assert "<< 20" not in line, f"{name}: a MiB constant beside a streaming choice:\n    {line.strip()}"
            for c in consts:
                assert not re.search(rf"\b{c}\b", line) or re.match(r"\s*constexpr", line), \
                    f"{name}: {c} feeds a streaming choice:\n    {line.strip()}"
        assert "FPSG_NT_BYTES" not in code or name == "bnact.hip", f"{name}: reads the macro, not beyond_cache()"
        assert not re.search(r"#\s*(define|undef)\s+FPSG_NT_BYTES", code), f"{name} redefines the threshold"


def test_second_library_exports_the_whole_abi():
    from fpsg_amd import _hip
    assert os.path.exists(_stream_lib.PATH), \
        f"{_stream_lib.PATH} not found: build it with `make -C fpsg_amd/csrc build/libfpsg_hip_stream.so`"
    lib = ctypes.CDLL(_stream_lib.PATH)
    missing = [name for name in _hip.SIGNATURES if not hasattr(lib, name)]
    assert not missing, missing
    bound, shipped = _stream_lib.load(), _hip.load()
    assert bound.fpsg_stream_threshold_bytes() == 0 and shipped.fpsg_stream_threshold_bytes() == 300 << 20
    assert bound.fpsg_version() == shipped.fpsg_version()
    # each library answers with its own state: an argument error in one leaves the other's message alone
    assert shipped.fpsg_chamfer_fwd(None, None, 0, 8, 8, None, None, None, None, None) == -2
    assert bound.fpsg_chamfer_fwd(None, None, 1, 8, 8, None, None, None, None, None) == -1
    assert b"positive" in shipped.fpsg_last_error() and b"null pointer" in bound.fpsg_last_error()
