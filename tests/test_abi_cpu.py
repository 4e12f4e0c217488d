"""The C-ABI library loads without a GPU and exports every symbol include/*.h declares;
argument checks answer without touching a device."""
import ctypes
import glob
import os
import re

import pytest

from conftest import ROOT


def _declared():
    names = set()
    for h in glob.glob(os.path.join(ROOT, "include", "*.h")):
        txt = re.sub(r"/\*.*?\*/", "", open(h).read(), flags=re.S)
        names |= set(re.findall(r"\b(fpsg_[a-z0-9_]+)\s*\(", txt))
    return sorted(names)


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    so = os.path.join(ROOT, "fpsg_amd", "libfpsg_hip.so")
    if not os.path.exists(so):
        g.build()
    from fpsg_amd import _hip
    return _hip.load()


def test_exports_every_declared_symbol(lib):
    decl = _declared()
    assert "fpsg_chamfer_fwd" in decl and "fpsg_version" in decl
    for name in decl:
        assert hasattr(lib, name), f"{name} declared in include/ but not exported"


def test_binding_table_matches_header(lib):
    from fpsg_amd import _hip
    assert sorted(_hip.SIGNATURES) == _declared()


def test_version_and_argument_checks(lib):
    assert lib.fpsg_version() == 1
    assert lib.fpsg_stream_threshold_bytes() == 300 << 20       # the shipped build: streaming forms beyond 300 MiB
    # null pointers / bad shapes are refused on the host, before any HIP call
    rc = lib.fpsg_chamfer_fwd(None, None, 1, 8, 8, None, None, None, None, None)
    assert rc == -1 and b"null pointer" in lib.fpsg_last_error()
    rc = lib.fpsg_chamfer_fwd(None, None, 0, 8, 8, None, None, None, None, None)
    assert rc == -2 and b"positive" in lib.fpsg_last_error()
    rc = lib.fpsg_chamfer_bwd(None, None, None, None, None, None, 2, 0, 3, None, None, None)
    assert rc == -2


def test_round4_entry_points_check_their_arguments(lib):
    """The entry points added in round 4 refuse bad arguments on the host, before any HIP call (no GPU needed)."""
    f = ctypes.c_float
    # K1 + loss sums: null clouds, then a bad n_first (caught behind the pointer checks: give fake non-null pointers)
    assert lib.fpsg_chamfer_fwd_tiled_losses(None, None, 8, 2048, 2048, None, None, None, None, None, 0, -1, 1, f(1), f(1),
                                             None, None) == -1
    assert lib.fpsg_chamfer_fwd_tiled_losses(None, None, 0, 2048, 2048, None, None, None, None, None, 0, -1, 1, f(1), f(1),
                                             None, None) == -2
    assert lib.fpsg_chamfer_bwd_losses(None, None, None, None, None, None, None, 4, 100, 100, 9, f(1), f(1), None, None,
                                       None) == -2 and b"n_first" in lib.fpsg_last_error()
    assert lib.fpsg_chamfer_bwd_losses(None, None, None, None, None, None, None, 4, 5000, 100, 1, f(1), f(1), None, None,
                                       None) == -4                                   # beyond 4096 points: FPSG_E_LIMIT
    assert lib.fpsg_chamfer_workspace_bytes(37, 2048, 2048, -1) == 37 * (8 + 4) * 2048 * 4 + 37 * 16 * 4
    # K2 variants
    assert lib.fpsg_emd_approx_variant(None, None, 2, 64, 64, None, None, None, None, 7, None) == -2
    assert lib.fpsg_emd_approx_variant(None, None, 2, 64, 64, None, None, None, None, 3, None) == -1
    # K8 with the BatchNorm backward folded in, K5's sums-only backward
    assert lib.fpsg_conv_first_dw_fold(None, None, None, None, None, None, 2, 3, 64, 32, 32, None, None, None) == -1
    assert lib.fpsg_bn_act_bwd_coef(None, None, None, None, 2, 64, 100, 1, 1, f(0), None, None, None, None, None) in (-1, -4)
    assert lib.fpsg_edgeconv_stats_ws_floats(8192, 64) == 512 * 2 * 64 * 2 and lib.fpsg_edgeconv_stats_ws_floats(0, 64) == 0
    assert lib.fpsg_bn_max_dz_offset(64, 1024, 2048) + 64 * 1024 == lib.fpsg_bn_max_workspace_floats(64, 1024, 2048)


def test_batchnorm_workspace_sizes_and_offsets(lib):
    """K5's size functions and the entry points that slice the buffer read one layout.  The numbers are those the
    library returned before the layout had a single home (recorded from that build, not derived from this one), at
    shapes with L below, at and not a multiple of the 4096-float segment and with H / 2 a multiple of the pooled
    form's rows per item and not; the closed forms are that layout's (128 floats of channel sums per channel, then one
    word, or four in the max form, per row and item; include/fpsg_hip.h states the dz offset's)."""
    rows = {  # (N, C, L): (fpsg_bn_workspace_floats, fpsg_bn_max_workspace_floats, fpsg_bn_max_dz_offset)
        (64, 1024, 2048): (196608, 458752, 393216),
        (5, 9, 4096 + 4100): (1287, 1737, 1692),
        (37, 64, 224 * 224): (38976, 133696, 131328),
        (16, 769, 4736): (123040, 209168, 196864),
        (2, 3, 4096): (390, 414, 408),
        (1, 1, 1): (129, 133, 132),
        (3, 2, 2 ** 31 - 1): (3145984, 12583174, 12583168),
    }
    for (N, C, L), (plain, most, dz) in rows.items():
        segs = -(-L // 4096)
        assert lib.fpsg_bn_workspace_floats(N, C, L) == plain == C * 128 + N * C * segs, (N, C, L)
        assert lib.fpsg_bn_max_dz_offset(N, C, L) == dz == C * 128 + N * C * segs * 4, (N, C, L)
        assert lib.fpsg_bn_max_workspace_floats(N, C, L) == most == dz + N * C, (N, C, L)
    planes = {  # (N, C, H, W): fpsg_bn_pool_workspace_floats; rows per item = max(1, 4096 // (2 W))
        (37, 64, 224, 224): 38976,       # 112 row pairs in items of 9: 13 items
        (8, 64, 112, 112): 10240,        # 56 in items of 18: 4
        (2, 3, 6, 4098): 402,            # a row pair longer than an item: 3 items of 1
        (4, 16, 36, 56): 2112,           # 18 in one item of 36
        (2, 8, 64, 64): 1040,            # 32 in one item of 32
        (5, 7, 30, 6): 931,
        (1, 1, 2, 2): 129,
    }
    for (N, C, H, W), floats in planes.items():
        rp = max(1, 4096 // (2 * W))
        assert lib.fpsg_bn_pool_workspace_floats(N, C, H, W) == floats == C * 128 + N * C * -(-(H // 2) // rp), (N, C, H, W)
    for bad in ((0, 4, 4), (4, -1, 4), (4, 4, 0)):
        assert lib.fpsg_bn_workspace_floats(*bad) == 0 and lib.fpsg_bn_max_workspace_floats(*bad) == 0, bad
        assert lib.fpsg_bn_max_dz_offset(*bad) == 0, bad
    for bad in ((0, 1, 2, 2), (1, 0, 2, 2), (1, 1, 1, 2), (1, 1, 2, 1), (1, 1, 0, -2)):
        assert lib.fpsg_bn_pool_workspace_floats(*bad) == 0, bad


def test_gemm_variant_ids_outside_the_documented_lists_are_refused_on_the_host(lib):
    """K10's entry points take the variant ids include/fpsg_hip.h lists and nothing else: the ids that once selected
    measurement-only builds (kernels without their loads, stores or split, delayed starts, no wave priorities) get
    FPSG_E_SHAPE (-2) with the id in the message, before any HIP call and before the pointer checks -- never a launch, never
    an alias of a kept id.  The kept ids pass the variant check (and then stop at the null pointers: -1)."""
    def split(variant, transB=0):
        return lib.fpsg_gemm_split(None, None, None, 1, 256, 256, 4096, 4096, 4096 if transB else 256, 256, 256 * 4096,
                                   256 * 4096, 256 * 256, transB, variant, None, 0, None)

    def persistent(variant):
        return lib.fpsg_gemm_split_nn_persistent(None, None, None, 1, 256, 256, 64, 256, 256, 64 * 256, 256 * 256, variant, None)

    for v in (1000, 2000, 4002, 100010, 200052, 8, 9):
        for transB in (0, 1):
            assert split(v, transB) == -2, v
            msg = lib.fpsg_last_error()
            assert b"fpsg_gemm_split" in msg and b"variant %d" % v in msg, (v, msg)
            assert lib.fpsg_gemm_split_workspace_floats(1, 256, 256, 4096, transB, v) == 0, v
    for v in (2, 3, 4, 5, 7, 8, 9, 10, 11, 15):
        assert persistent(v) == -2, v
        msg = lib.fpsg_last_error()
        assert b"fpsg_gemm_split_nn_persistent" in msg and b"variant %d" % v in msg, (v, msg)
    # kept ids: -1 and one explicit id per entry point get past the variant check
    for v in (-1, 5, 73):
        assert split(v, 1) == -1 and b"null pointer" in lib.fpsg_last_error(), v
    assert lib.fpsg_gemm_split_workspace_floats(1, 256, 256, 4096, 1, -1) > 0      # (the shape does split its reduction)
    assert lib.fpsg_gemm_split_workspace_floats(1, 256, 256, 4096, 1, 70) == 7 * 256 * 256
    for v in (-1, 0, 1, 6, 12, 13, 14):
        assert persistent(v) == -1 and b"null pointer" in lib.fpsg_last_error(), v


def test_product_path_has_no_cpu_fallback():
    import torch
    from fpsg_amd._hip import FpsgHipError
    from fpsg_amd.metrics import chamfer_distance
    with pytest.raises(FpsgHipError):
        chamfer_distance(torch.rand(1, 4, 3), torch.rand(1, 4, 3))


def test_package_never_imports_oracle():
    """Only tests/, smoke() and bench.py's cpu_baseline leg may touch oracle/."""
    for path in glob.glob(os.path.join(ROOT, "fpsg_amd", "**", "*.py"), recursive=True):
        src = open(path).read()
        assert not re.search(r"^\s*(from|import)\s+oracle\b", src, flags=re.M), path
    for path in glob.glob(os.path.join(ROOT, "fpsg_amd", "csrc", "*")):
        if os.path.isfile(path):   # comments may cite the oracle as the specification; code may not use it
            src = re.sub(r"(?m)^\s*#(?!\s*include)[^\n]*", "", open(path, errors="ignore").read())
            assert not re.search(r"#\s*include[^\n]*oracle", src), path
            assert "fpsg_oracle" not in re.sub(r"//[^\n]*", "", src), path


def test_package_sets_the_runtime_default_without_overriding_the_caller():
    """``import fpsg_amd`` asks the HIP runtime for kernel arguments in device memory (HIP_FORCE_DEV_KERNARG=1, +2.2 % on
    the 350-launch episode) unless the caller already chose a value."""
    import subprocess
    import sys
    code = "import os, fpsg_amd; print(os.environ.get('HIP_FORCE_DEV_KERNARG'))"
    env = {k: v for k, v in os.environ.items() if k != "HIP_FORCE_DEV_KERNARG"}
    out = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, check=True)
    assert out.stdout.strip() == "1"
    env["HIP_FORCE_DEV_KERNARG"] = "0"
    out = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, check=True)
    assert out.stdout.strip() == "0"
