"""CPU-side checks of hx_exact_range_filtered (exact range scans with a WHERE filter per query): the entry point is exported and declared in the
header, the ctypes table and the Rust block with the same 17 parameters, hx_exact_range keeps its declaration, the binding method has the
documented signature, and a call without an engine fails without touching a device or the outputs.  What needs an engine (the argument errors
included) is in tests/test_gpu_exact_range_filtered.py."""
import ctypes
import inspect
import os
import re

import pgvector_rx_amd as hx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_entry_point_everywhere():
    L = hx.lib()
    assert hasattr(L, "hx_exact_range_filtered")
    assert L.hx_exact_range_filtered.restype is ctypes.c_int and len(L.hx_exact_range_filtered.argtypes) == 17
    hdr = open(os.path.join(ROOT, "include", "hnswrx.h")).read()
    m = re.search(r"int hx_exact_range_filtered\(([^;]*)\);", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S))
    assert m and len(m.group(1).split(",")) == 17                                  # the ctypes table binds what the header declares
    assert re.sub(r"\s+", " ", m.group(1)) == ("hx_engine *e, int op, int cmp, const double *radius, uint32_t first_query, uint32_t nq, "
                                               "uint64_t first_row, uint64_t n_rows, "
                                               "uint32_t n_filters, const uint64_t *const *filters, const int32_t *filter_of, "
                                               "int order, uint64_t cap, "
                                               "uint64_t *offsets_out, uint32_t *ids_out, double *dist_out, uint64_t *total_out")
    ffi = open(os.path.join(ROOT, "integration", "rust", "src", "gpu", "ffi.rs")).read()
    assert "pub fn hx_exact_range_filtered(" in ffi
    decl = ffi[ffi.index("pub fn hx_exact_range_filtered("):]
    assert len(decl[:decl.index(") -> c_int;")].split(",")) == 17
    wrapper = open(os.path.join(ROOT, "integration", "rust", "src", "gpu", "exact.rs")).read()
    assert "pub fn exact_range_filtered_gpu(" in wrapper and "hx_exact_range_filtered(" in wrapper


def test_exact_range_keeps_its_signature():
    hdr = open(os.path.join(ROOT, "include", "hnswrx.h")).read()
    assert re.search(r"int hx_exact_range\(hx_engine \*e, int op, int cmp, const double \*radius, uint32_t first_query, uint32_t nq,\s*"
                     r"uint64_t first_row, uint64_t n_rows, const uint64_t \*row_pass, int order, uint64_t cap,\s*"
                     r"uint64_t \*offsets_out, uint32_t \*ids_out, double \*dist_out, uint64_t \*total_out\);", hdr)
    assert len(hx.lib().hx_exact_range.argtypes) == 15


def test_binding_signature():
    p = inspect.signature(hx.Engine.exact_range_filtered).parameters
    assert list(p) == ["self", "op", "radius", "filters", "filter_of", "cmp", "first_query", "nq", "first_row", "n_rows", "packed", "ordered",
                       "count_only", "cap"]
    assert p["cmp"].default == hx.CMP_LT and p["first_query"].default == 0 and p["nq"].default is None and p["first_row"].default == 0
    assert p["n_rows"].default is None and p["packed"].default is False and p["ordered"].default is False and p["count_only"].default is False
    assert p["cap"].default is None
    q = inspect.signature(hx.Engine.exact_range).parameters                        # the same names and defaults where they share them
    for name in ("cmp", "first_query", "nq", "first_row", "n_rows", "packed", "ordered", "count_only", "cap"):
        assert p[name].default == q[name].default


def test_no_engine_is_an_argument_error():
    L = hx.lib()
    off = (ctypes.c_uint64 * 2)(7, 7)
    ids = (ctypes.c_uint32 * 4)(*[7] * 4)
    dist = (ctypes.c_double * 4)(*[7.0] * 4)
    total = ctypes.c_uint64(7)
    radius = (ctypes.c_double * 1)(1.0)
    words = (ctypes.c_uint64 * 1)(1)
    filters = (ctypes.c_void_p * 1)(ctypes.addressof(words))
    of = (ctypes.c_int32 * 1)(0)
    rc = L.hx_exact_range_filtered(None, hx.OP_L2, hx.CMP_LT, radius, 0, 1, 0, 1, 1, filters, of, hx.RANGE_BY_ROW, 4, off, ids, dist,
                                   ctypes.byref(total))
    assert rc == -1                                                     # HX_E_ARG, outputs untouched
    assert list(off) == [7, 7] and list(ids) == [7] * 4 and list(dist) == [7.0] * 4 and total.value == 7
