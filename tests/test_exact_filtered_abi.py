"""CPU-side checks of hx_exact_search_filtered (exact k-NN scans with a WHERE filter per query): the entry point is exported and declared in the
header, the ctypes table and the Rust block with the same 13 parameters, its constant agrees everywhere, hx_exact_search keeps its declaration, and
a call without an engine fails without touching a device or the outputs.  What needs an engine (the argument errors included) is in
tests/test_gpu_exact_filtered.py."""
import ctypes
import inspect
import os
import re

import pgvector_rx_amd as hx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_entry_point_everywhere():
    L = hx.lib()
    assert hasattr(L, "hx_exact_search_filtered")
    assert L.hx_exact_search_filtered.restype is ctypes.c_int and len(L.hx_exact_search_filtered.argtypes) == 13
    hdr = open(os.path.join(ROOT, "include", "hnswrx.h")).read()
    m = re.search(r"int hx_exact_search_filtered\(([^;]*)\);", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S))
    assert m and len(m.group(1).split(",")) == 13                                  # the ctypes table binds what the header declares
    assert re.sub(r"\s+", " ", m.group(1)) == ("hx_engine *e, int op, uint32_t first_query, uint32_t nq, uint64_t first_row, uint64_t n_rows, "
                                               "uint32_t n_filters, const uint64_t *const *filters, const int32_t *filter_of, "
                                               "uint32_t k, uint32_t *ids_out, double *dist_out, uint32_t *counts_out")
    assert "#define HX_EXACT_MAX_FILTERS 64" in hdr
    assert hx.EXACT_MAX_FILTERS == 64
    ffi = open(os.path.join(ROOT, "integration", "rust", "src", "gpu", "ffi.rs")).read()
    assert "pub fn hx_exact_search_filtered(" in ffi
    assert "pub const HX_EXACT_MAX_FILTERS: u32 = 64;" in ffi
    decl = ffi[ffi.index("pub fn hx_exact_search_filtered("):]
    assert len(decl[:decl.index(") -> c_int;")].split(",")) == 13
    wrapper = open(os.path.join(ROOT, "integration", "rust", "src", "gpu", "exact.rs")).read()
    assert "pub fn exact_search_filtered_gpu(" in wrapper and "hx_exact_search_filtered(" in wrapper
    assert "pub mod exact;" in open(os.path.join(ROOT, "integration", "rust", "src", "gpu", "mod.rs")).read()


def test_exact_search_keeps_its_signature():
    hdr = open(os.path.join(ROOT, "include", "hnswrx.h")).read()
    assert re.search(r"int hx_exact_search\(hx_engine \*e, int op, uint32_t first_query, uint32_t nq, uint64_t first_row, uint64_t n_rows,\s*"
                     r"const uint64_t \*row_pass, uint32_t k, uint32_t \*ids_out, double \*dist_out, uint32_t \*counts_out\);", hdr)
    assert len(hx.lib().hx_exact_search.argtypes) == 11


def test_binding_signature():
    p = inspect.signature(hx.Engine.exact_search_filtered).parameters
    assert list(p) == ["self", "op", "k", "filters", "filter_of", "first_query", "nq", "first_row", "n_rows", "packed"]
    assert p["first_query"].default == 0 and p["nq"].default is None and p["first_row"].default == 0 and p["n_rows"].default is None
    assert p["packed"].default is False


def test_no_engine_is_an_argument_error():
    L = hx.lib()
    ids = (ctypes.c_uint32 * 4)(*[7] * 4)
    dist = (ctypes.c_double * 4)(*[7.0] * 4)
    cnt = (ctypes.c_uint32 * 1)(7)
    words = (ctypes.c_uint64 * 1)(1)
    filters = (ctypes.c_void_p * 1)(ctypes.addressof(words))
    of = (ctypes.c_int32 * 1)(0)
    rc = L.hx_exact_search_filtered(None, hx.OP_L2, 0, 1, 0, 1, 1, filters, of, 4, ids, dist, cnt)
    assert rc == -1                                                     # HX_E_ARG, outputs untouched
    assert list(ids) == [7] * 4 and list(dist) == [7.0] * 4 and cnt[0] == 7
