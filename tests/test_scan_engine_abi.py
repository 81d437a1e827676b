"""CPU-side checks of the scan-only engines, the halfvec casts and the exact re-rank: hx_create_ex validates its arguments before any device is
touched, and the library exports the new entry points."""
import ctypes
import os

import pgvector_rx_amd as hx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_create_ex_flags_and_limits():
    L, h = hx.lib(), ctypes.c_void_p()
    assert L.hx_create_ex(0, hx.F32, hx.L2SQ, 8, 16, 2, ctypes.byref(h)) == -1                         # unknown flag
    assert L.hx_create_ex(0, hx.F32, hx.L2SQ, 8, 16, -1, ctypes.byref(h)) == -1
    assert L.hx_create_ex(0, hx.F32, hx.L2SQ, 16001, 16, hx.CREATE_SCAN_ONLY, ctypes.byref(h)) == -2    # VECTOR_MAX_DIM, vector.rs:30
    assert b"16000" in L.hx_last_error(None) and b"vector" in L.hx_last_error(None)
    assert L.hx_create_ex(0, hx.F16, hx.L2SQ, 16001, 16, hx.CREATE_SCAN_ONLY, ctypes.byref(h)) == -2    # HALFVEC_MAX_DIM, halfvec.rs:28
    assert b"halfvec cannot have more than 16000" in L.hx_last_error(None)
    assert L.hx_create_ex(0, hx.BIT, hx.HAMMING, 64001, 16, hx.CREATE_SCAN_ONLY, ctypes.byref(h)) == -2  # bit keeps its limit
    assert L.hx_create_ex(0, hx.F32, hx.L2SQ, 0, 16, hx.CREATE_SCAN_ONLY, ctypes.byref(h)) == -2
    # without the flag, hx_create's index limits
    assert L.hx_create_ex(0, hx.F32, hx.L2SQ, 2001, 16, 0, ctypes.byref(h)) == -2
    assert b"2000 dimensions" in L.hx_last_error(None)
    assert L.hx_create_ex(0, 7, hx.L2SQ, 8, 16, hx.CREATE_SCAN_ONLY, ctypes.byref(h)) == -1
    assert L.hx_create_ex(0, hx.F32, hx.L2SQ, 8, 16, 0, None) == -1


def test_scan_only_wide_gets_past_validation():
    import torch
    if torch.cuda.is_available():
        return                                  # the device case is tests/test_gpu_rerank.py's
    L, h = hx.lib(), ctypes.c_void_p()
    for dtype, dim in ((hx.F32, 3072), (hx.F32, 16000), (hx.F16, 16000)):
        assert L.hx_create_ex(0, dtype, hx.L2SQ, dim, 16, hx.CREATE_SCAN_ONLY, ctypes.byref(h)) == -5
        assert b"no CPU fallback" in L.hx_last_error(None)
    assert L.hx_create_ex(0, hx.F32, hx.L2SQ, 3072, 16, 0, ctypes.byref(h)) == -2                       # an index engine still stops at 2000


def test_new_names_exported_and_bound():
    L = hx.lib()
    for name in ("hx_create_ex", "hx_append_rows_halfvec", "hx_set_queries_halfvec", "hx_exact_rerank"):
        assert hasattr(L, name), name
    src = open(os.path.join(ROOT, "include", "hnswrx.h")).read()
    assert "#define HX_CREATE_SCAN_ONLY 1" in src and "HX_E_RANGE = -7" in src
    assert hx.CREATE_SCAN_ONLY == 1 and hx.E_RANGE == -7
    for m in ("append_halfvec_from", "set_queries_halfvec_from", "exact_rerank"):
        assert callable(getattr(hx.Engine, m))
