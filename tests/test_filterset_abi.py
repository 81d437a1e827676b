"""CPU-side checks of the filter sets (hx_filterset_*, hx_exact_search_set, hx_exact_range_set): every new entry point is exported and declared
with the same parameter count in the header, the ctypes table and the Rust block; the constants agree in all three places; the two _filtered
scans keep their declarations; and a call without an engine or without a set fails without touching a device or its outputs.  What needs an
engine is in tests/test_gpu_filterset.py."""
import ctypes
import os
import re

import pytest

import pgvector_rx_amd as hx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"hx_filterset_create_labels": 6, "hx_filterset_create_labels_device": 6, "hx_filterset_create_bitmaps": 6, "hx_filterset_append_labels": 3,
       "hx_filterset_info": 5, "hx_filterset_counts": 4, "hx_filterset_read": 5, "hx_filterset_destroy": 1, "hx_exact_search_set": 10,
       "hx_exact_range_set": 14}


def header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "hnswrx.h")).read(), flags=re.S)


def rust():
    return open(os.path.join(ROOT, "integration", "rust", "src", "gpu", "ffi.rs")).read()


@pytest.mark.parametrize("name", sorted(NEW))
def test_entry_point_everywhere(name):
    L = hx.lib()
    assert hasattr(L, name)
    fn = getattr(L, name)
    assert fn.restype is ctypes.c_int and len(fn.argtypes) == NEW[name]
    m = re.search(r"int %s\(([^;]*)\);" % name, header())
    assert m and len(m.group(1).split(",")) == NEW[name]
    ffi = rust()
    assert "pub fn %s(" % name in ffi
    decl = ffi[ffi.index("pub fn %s(" % name):]
    assert len(decl[:decl.index(") -> c_int;")].split(",")) == NEW[name]


def test_rust_wrappers():
    wrapper = open(os.path.join(ROOT, "integration", "rust", "src", "gpu", "exact.rs")).read()
    for fn, sym in (("filterset_from_labels_gpu", "hx_filterset_create_labels("), ("filterset_append_gpu", "hx_filterset_append_labels("),
                    ("exact_search_set_gpu", "hx_exact_search_set("), ("exact_range_set_gpu", "hx_exact_range_set(")):
        assert "pub fn %s(" % fn in wrapper and sym in wrapper
    assert "pub struct hx_filterset" in rust()


def test_constants_agree():
    hdr, ffi = header(), rust()
    assert re.search(r"#define HX_FILTERSET_MAX_FILTERS \(1u << 20\)", hdr) and re.search(r"#define HX_NO_LABEL 0xFFFFFFFFu", hdr)
    assert re.search(r"pub const HX_FILTERSET_MAX_FILTERS: u32 = 1 << 20;", ffi) and re.search(r"pub const HX_NO_LABEL: u32 = 0xFFFF_FFFF;", ffi)
    assert hx.FILTERSET_MAX_FILTERS == 1 << 20 and hx.NO_LABEL == 0xFFFFFFFF
    assert re.search(r"#define HX_EXACT_MAX_FILTERS 64\b", hdr) and "pub const HX_EXACT_MAX_FILTERS: u32 = 64;" in ffi and hx.EXACT_MAX_FILTERS == 64


def test_filtered_scans_keep_their_declarations():
    hdr = re.sub(r"\s+", " ", header())
    assert ("int hx_exact_search_filtered(hx_engine *e, int op, uint32_t first_query, uint32_t nq, uint64_t first_row, uint64_t n_rows, "
            "uint32_t n_filters, const uint64_t *const *filters, const int32_t *filter_of, "
            "uint32_t k, uint32_t *ids_out, double *dist_out, uint32_t *counts_out);") in hdr
    assert ("int hx_exact_range_filtered(hx_engine *e, int op, int cmp, const double *radius, uint32_t first_query, uint32_t nq, "
            "uint64_t first_row, uint64_t n_rows, "
            "uint32_t n_filters, const uint64_t *const *filters, const int32_t *filter_of, "
            "int order, uint64_t cap, "
            "uint64_t *offsets_out, uint32_t *ids_out, double *dist_out, uint64_t *total_out);") in hdr
    assert len(hx.lib().hx_exact_search_filtered.argtypes) == 13 and len(hx.lib().hx_exact_range_filtered.argtypes) == 17
    assert ("int hx_exact_search(hx_engine *e, int op, uint32_t first_query, uint32_t nq, uint64_t first_row, uint64_t n_rows, "
            "const uint64_t *row_pass, uint32_t k, uint32_t *ids_out, double *dist_out, uint32_t *counts_out);") in hdr


def test_binding_surface():
    for name in ("from_labels", "from_bitmaps", "append_labels", "counts", "read", "close"):
        assert callable(getattr(hx.FilterSet, name))
    assert callable(hx.Engine.exact_search_set) and callable(hx.Engine.exact_range_set)


def test_creates_without_an_engine():
    L = hx.lib()
    labels = (ctypes.c_uint32 * 4)(0, 1, 0, 1)
    words = (ctypes.c_uint64 * 1)(5)
    filters = (ctypes.c_void_p * 1)(ctypes.addressof(words))
    for fn, src in ((L.hx_filterset_create_labels, labels), (L.hx_filterset_create_labels_device, labels), (L.hx_filterset_create_bitmaps, filters)):
        h = ctypes.c_void_p(0x77)
        assert fn(None, 0, 4, 2, src, ctypes.byref(h)) == -1             # HX_E_ARG, out untouched
        assert h.value == 0x77


def test_set_calls_without_a_set():
    L = hx.lib()
    labels = (ctypes.c_uint32 * 2)(0, 0)
    assert L.hx_filterset_append_labels(None, 2, labels) == -1
    a, b, c, d = ctypes.c_uint64(7), ctypes.c_uint64(7), ctypes.c_uint32(7), ctypes.c_uint64(7)
    assert L.hx_filterset_info(None, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c), ctypes.byref(d)) == -1
    assert (a.value, b.value, c.value, d.value) == (7, 7, 7, 7)
    counts = (ctypes.c_uint64 * 2)(7, 7)
    assert L.hx_filterset_counts(None, 0, 2, counts) == -1 and list(counts) == [7, 7]
    ids, n = (ctypes.c_uint32 * 2)(7, 7), ctypes.c_uint64(7)
    assert L.hx_filterset_read(None, 0, 2, ids, ctypes.byref(n)) == -1 and list(ids) == [7, 7] and n.value == 7
    assert L.hx_filterset_destroy(None) == -1


def test_scans_without_an_engine():
    L = hx.lib()
    of = (ctypes.c_int32 * 1)(0)
    ids, dist, cnt = (ctypes.c_uint32 * 4)(*[7] * 4), (ctypes.c_double * 4)(*[7.0] * 4), (ctypes.c_uint32 * 1)(7)
    assert L.hx_exact_search_set(None, hx.OP_L2, 0, 1, None, of, 4, ids, dist, cnt) == -1
    assert list(ids) == [7] * 4 and list(dist) == [7.0] * 4 and list(cnt) == [7]
    off, total, radius = (ctypes.c_uint64 * 2)(7, 7), ctypes.c_uint64(7), (ctypes.c_double * 1)(1.0)
    assert L.hx_exact_range_set(None, hx.OP_L2, hx.CMP_LT, radius, 0, 1, None, of, hx.RANGE_BY_ROW, 4, off, ids, dist, ctypes.byref(total)) == -1
    assert list(off) == [7, 7] and list(ids) == [7] * 4 and list(dist) == [7.0] * 4 and total.value == 7
