"""The tests' second build of the HIP library, ``fpsg_amd/csrc/build/libfpsg_hip_stream.so``: the sources that read the
byte threshold of the streaming (non-temporal) kernel forms compiled with ``-DFPSG_NT_BYTES=0``, so that every pass
takes its streaming form at any size (fpsg_amd/csrc/Makefile).  Same C ABI, bound with the package's own signature
table; both libraries live in one process.  There is no fallback: a missing file is an error that names the target."""
import os

from conftest import ROOT

PATH = os.path.join(ROOT, "fpsg_amd", "csrc", "build", "libfpsg_hip_stream.so")
SHIPPED_THRESHOLD = 300 << 20

_handle = None


def load():
    """The bound handle of the second library (one per process)."""
    global _handle
    if _handle is None:
        from fpsg_amd import _hip
        assert os.path.exists(PATH), (f"{PATH} not found: build it with `make -C fpsg_amd/csrc build/libfpsg_hip_stream.so` "
                                      "(part of `make -C fpsg_amd/csrc` and of build())")
        _handle = _hip.bind(PATH)
    return _handle


def both():
    """(shipped handle, streaming handle), after proving which build each one is."""
    from fpsg_amd import _hip
    shipped, stream = _hip.load(), load()
    assert shipped is not stream and shipped._handle != stream._handle, "one library loaded twice"
    assert shipped.fpsg_stream_threshold_bytes() == SHIPPED_THRESHOLD, shipped.fpsg_stream_threshold_bytes()
    assert stream.fpsg_stream_threshold_bytes() == 0, stream.fpsg_stream_threshold_bytes()
    return shipped, stream
