"""CPU-side checks of the exact scans' sidecar path: the counter entry point is exported and bound in the header, the ctypes table and the Rust
block, and hx_create_ex validates HX_CREATE_SCAN_SIDECAR before any device is touched."""
import ctypes
import os
import re

import pgvector_rx_amd as hx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_stats_entry_point_everywhere():
    L = hx.lib()
    assert hasattr(L, "hx_exact_sidecar_stats")
    a, b = ctypes.c_uint64(7), ctypes.c_uint64(7)
    assert L.hx_exact_sidecar_stats(None, ctypes.byref(a), ctypes.byref(b), 0) == -1       # HX_E_ARG
    assert (a.value, b.value) == (7, 7)
    hdr = open(os.path.join(ROOT, "include", "hnswrx.h")).read()
    assert re.search(r"int hx_exact_sidecar_stats\(hx_engine \*e, uint64_t \*rows_coded, uint64_t \*rows_fetched, int reset\);", hdr)
    assert "#define HX_CREATE_SCAN_SIDECAR 8" in hdr and "HX_EXACT_SIDECAR" in hdr
    ffi = open(os.path.join(ROOT, "integration", "rust", "src", "gpu", "ffi.rs")).read()
    assert "pub fn hx_exact_sidecar_stats(" in ffi and "pub const HX_CREATE_SCAN_SIDECAR: c_int = 8;" in ffi
    assert hx.CREATE_SCAN_SIDECAR == 8 and callable(hx.Engine.exact_sidecar_stats)


def test_scan_sidecar_flag_validation():
    L, h = hx.lib(), ctypes.c_void_p()
    SO, SS, NS = hx.CREATE_SCAN_ONLY, hx.CREATE_SCAN_SIDECAR, hx.CREATE_NO_SIDECAR
    assert L.hx_create_ex(0, hx.F32, hx.L2SQ, 3072, 16, SS, ctypes.byref(h)) == -1             # not scan-only
    assert b"HX_CREATE_SCAN_SIDECAR" in L.hx_last_error(None)
    assert L.hx_create_ex(0, hx.F32, hx.L2SQ, 768, 16, SS, ctypes.byref(h)) == -1
    assert L.hx_create_ex(0, hx.F16, hx.L2SQ, 3072, 16, SO | SS, ctypes.byref(h)) == -1        # halfvec
    assert L.hx_create_ex(0, hx.F32, hx.L2SQ, 128, 16, SO | SS, ctypes.byref(h)) == -1         # 128 dimensions: 8-lane rows
    assert L.hx_create_ex(0, hx.F32, hx.NEG_IP, 3072, 16, SO | SS, ctypes.byref(h)) == -1      # not L2
    assert L.hx_create_ex(0, hx.F32, hx.L1, 3072, 16, SO | SS, ctypes.byref(h)) == -1
    assert L.hx_create_ex(0, hx.F32, hx.L2SQ, 3072, 16, SO | SS | NS, ctypes.byref(h)) == -1   # with and without at once
    assert L.hx_create_ex(0, hx.F32, hx.L2SQ, 3072, 16, 2, ctypes.byref(h)) == -1              # 2 stays unknown
    assert L.hx_create_ex(0, hx.F32, hx.L2SQ, 3072, 16, 16, ctypes.byref(h)) == -1
    assert h.value is None


def test_scan_sidecar_gets_past_validation():
    import torch
    if torch.cuda.is_available():
        return                                  # the device case is tests/test_gpu_exact_sidecar.py's
    L, h = hx.lib(), ctypes.c_void_p()
    for dim in (129, 3072, 16000):
        assert L.hx_create_ex(0, hx.F32, hx.L2SQ, dim, 16, hx.CREATE_SCAN_ONLY | hx.CREATE_SCAN_SIDECAR, ctypes.byref(h)) == -5   # HX_E_NODEVICE
        assert b"no CPU fallback" in L.hx_last_error(None)
