"""CPU-side checks of hx_index_search_filtered (per-query filters and distance predicates in iterative index scans): the entry point is exported
and declared in the header, the ctypes table and the Rust block, its constants agree everywhere, and a call without an index fails without
touching a device.  What needs an index (the argument errors included: an index needs an engine, an engine a device) is in
tests/test_gpu_scan_filtered.py."""
import ctypes
import inspect
import os
import re

import pgvector_rx_amd as hx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_entry_point_everywhere():
    L = hx.lib()
    assert hasattr(L, "hx_index_search_filtered")
    assert L.hx_index_search_filtered.restype is ctypes.c_int and len(L.hx_index_search_filtered.argtypes) == 17
    hdr = open(os.path.join(ROOT, "include", "hnswrx.h")).read()
    m = re.search(r"int hx_index_search_filtered\(([^;]*)\);", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S))
    assert m and len(m.group(1).split(",")) == 17                                  # the ctypes table binds what the header declares
    assert "#define HX_SCAN_MAX_FILTERS 64" in hdr and "#define HX_SCAN_STOP_PAST_RADIUS 1" in hdr
    assert hx.SCAN_MAX_FILTERS == 64 and hx.SCAN_STOP_PAST_RADIUS == 1
    ffi = open(os.path.join(ROOT, "integration", "rust", "src", "gpu", "ffi.rs")).read()
    assert "pub fn hx_index_search_filtered(" in ffi
    assert "pub const HX_SCAN_MAX_FILTERS: u32 = 64;" in ffi and "pub const HX_SCAN_STOP_PAST_RADIUS: c_int = 1;" in ffi
    decl = ffi[ffi.index("pub fn hx_index_search_filtered("):]
    assert len(decl[:decl.index(") -> c_int;")].split(",")) == 17
    graph = open(os.path.join(ROOT, "integration", "rust", "src", "gpu", "graph.rs")).read()
    assert "pub fn search_filtered_gpu(" in graph and "hx_index_search_filtered(" in graph


def test_old_entry_point_keeps_its_signature():
    hdr = open(os.path.join(ROOT, "include", "hnswrx.h")).read()
    assert re.search(r"int hx_index_search_iterative\(hx_index \*ix, uint32_t nq, uint32_t ef_search, int mode, int64_t max_scan_tuples,\s*"
                     r"uint32_t limit, const uint8_t \*filter_pass, uint64_t n_filter,\s*int64_t \*tids_out, float \*dist_out, uint32_t \*counts_out\);", hdr)
    assert len(hx.lib().hx_index_search_iterative.argtypes) == 11


def test_binding_signature():
    p = inspect.signature(hx.Index.search_filtered).parameters
    assert list(p) == ["self", "nq", "ef_search", "mode", "max_scan_tuples", "limit", "filters", "filter_of", "cmp", "radius", "stop_past_radius"]
    assert p["filters"].default is None and p["filter_of"].default is None and p["cmp"].default is None and p["radius"].default is None
    assert p["stop_past_radius"].default is False


def test_no_index_is_an_argument_error():
    L = hx.lib()
    out = (ctypes.c_int64 * 4)()
    cnt = (ctypes.c_uint32 * 1)(7)
    rc = L.hx_index_search_filtered(None, 1, 40, 2, 20000, 4, 0, None, None, None, -1, None, 0, out, None, None, cnt)
    assert rc == -1 and cnt[0] == 7                                     # HX_E_ARG, outputs untouched
