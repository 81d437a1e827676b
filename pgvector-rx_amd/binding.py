"""ctypes binding of include/hnswrx.h (no arithmetic here; every call lands in libhnswrx.so)."""
import ctypes as C
import os

import numpy as np

from . import build as _build

F32, F16, BIT, SPARSE = 0, 1, 2, 3
L2SQ, NEG_IP, L1, HAMMING, JACCARD = 0, 1, 2, 3, 4
OP_L2, OP_NEG_IP, OP_COSINE, OP_L1, OP_HAMMING, OP_JACCARD = 0, 1, 2, 3, 4, 5   # hx_op: the SQL operators <-> <#> <=> <+> <~> <%>
EXACT_MAX_K = 1024
EXACT_MAX_FILTERS = 64                                 # hx_exact_search_filtered
FILTERSET_MAX_FILTERS = 1 << 20                        # hx_filterset_create_*
NO_LABEL = 0xFFFFFFFF                                  # HX_NO_LABEL: a row in no filter of a filter set
CMP_LT, CMP_LE, CMP_GT, CMP_GE = 0, 1, 2, 3           # hx_cmp: v <op> q  <  <=  >  >=  radius
SCAN_MAX_FILTERS, SCAN_STOP_PAST_RADIUS = 64, 1       # hx_index_search_filtered
RANGE_BY_ROW, RANGE_BY_DISTANCE = 0, 1                 # hx_range_order: heap order, or the ORDER BY without LIMIT
E_ARG = -1
E_NOMEM = -3
E_STATE = -6
E_RANGE = -7                                           # a value out of range for the target type (the halfvec casts)
CREATE_SCAN_ONLY = 1                                   # hx_create_ex: no index; vector / halfvec up to 16000 dims
CREATE_NO_SIDECAR = 4                                  # hx_create_ex: no 8-bit row sidecar (f32 L2 engines keep one by default)
CREATE_SCAN_SIDECAR = 8                                # hx_create_ex: a scan-only f32 L2 engine (dim > 128) keeps the sidecar for the exact scans
QUERY_SLOT = 0x80000000
_NP = {F32: np.float32, F16: np.uint16, BIT: np.uint8, SPARSE: np.uint8}
SPARSE_MAX_NNZ = 1000


def sparse_record_bytes(dim):
    return (16 + 8 * min(dim, SPARSE_MAX_NNZ) + 15) & ~15


def pack_sparse(dim, rows):
    """rows: iterable of (indices, values) -- ascending 0-based indices, at most 1000 of them -> uint8[n, record] in the engine's HX_SPARSE
    record layout {int32 nnz; int32 pad[3]; int32 index[cap]; float32 value[cap]} (include/hnswrx.h), unused slots zero."""
    cap, rb = min(dim, SPARSE_MAX_NNZ), sparse_record_bytes(dim)
    rows = list(rows)
    out = np.zeros((len(rows), rb), np.uint8)
    for r, (idx, val) in enumerate(rows):
        idx, val = np.asarray(idx, np.int32), np.asarray(val, np.float32)
        k = len(idx)
        assert k == len(val) and k <= cap and (k < 2 or np.all(np.diff(idx) > 0)) and (k == 0 or (idx[0] >= 0 and idx[-1] < dim))
        out[r, 0:4] = np.array([k], np.int32).view(np.uint8)
        out[r, 16:16 + 4 * k] = idx.view(np.uint8)
        out[r, 16 + 4 * cap:16 + 4 * cap + 4 * k] = val.view(np.uint8)
    return out

_lib = None


class HxError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("hnswrx error %d: %s" % (code, msg))
        self.code = code


def lib_path():
    return _build.LIB


def lib():
    """Loads libhnswrx.so, (re)building it when hipcc is available and the sources are newer.
    There is no fallback: if the library cannot be built or loaded this raises."""
    global _lib
    if _lib is not None:
        return _lib
    if _build.stale():
        _build.build()
    L = C.CDLL(_build.LIB)
    vp, i32, u32, u64, i64 = C.c_void_p, C.c_int, C.c_uint32, C.c_uint64, C.c_int64
    sig = {
        "hx_abi_version": (i32, []),
        "hx_last_error": (C.c_char_p, [vp]),
        "hx_create": (i32, [i32, i32, i32, i32, u64, C.POINTER(vp)]),
        "hx_create_ex": (i32, [i32, i32, i32, i32, u64, i32, C.POINTER(vp)]),
        "hx_destroy": (i32, [vp]),
        "hx_dim": (i32, [vp]),
        "hx_row_bytes": (u64, [vp]),
        "hx_num_rows": (u64, [vp]),
        "hx_stream": (vp, [vp]),
        "hx_append_rows": (i32, [vp, vp, u64, C.POINTER(u64)]),
        "hx_append_rows_device": (i32, [vp, vp, u64, C.POINTER(u64)]),
        "hx_pop_rows": (i32, [vp, u64]),
        "hx_read_rows": (i32, [vp, u64, u64, vp]),
        "hx_sidecar_read": (i32, [vp, u64, u64, vp, vp]),
        "hx_sidecar_stats": (i32, [vp, C.POINTER(u64), C.POINTER(u64), i32]),
        "hx_sidecar_bounds": (i32, [vp, u32, vp, u32, vp]),
        "hx_exact_sidecar_stats": (i32, [vp, C.POINTER(u64), C.POINTER(u64), i32]),
        "hx_normalize_rows": (i32, [vp, u64, u64, vp]),
        "hx_set_queries": (i32, [vp, vp, u32, i32]),
        "hx_set_queries_device": (i32, [vp, vp, u32, i32]),
        "hx_append_rows_halfvec": (i32, [vp, vp, u64, u64, C.POINTER(u64)]),
        "hx_set_queries_halfvec": (i32, [vp, vp, i32]),
        "hx_distances": (i32, [vp, vp, vp, u32, vp]),
        "hx_distances_batch": (i32, [vp, u32, vp, vp, vp, vp]),
        "hx_pairwise": (i32, [vp, vp, u32, vp]),
        "hx_pairwise_many": (i32, [vp, u32, vp, vp, vp, vp, vp, vp]),
        "hx_pairwise_many_mfma": (i32, [vp, u32, vp, vp, vp, vp, vp, vp, vp]),
        "hx_rows_equal": (i32, [vp, u32, vp, vp, vp]),
        "hx_set_timing": (i32, [vp, i32]),
        "hx_last_kernel_ms": (i32, [vp, C.POINTER(C.c_float)]),
        "hx_kernel_stats": (i32, [vp, i32, C.POINTER(u64), C.POINTER(u64), C.POINTER(C.c_double), i32]),
        "hx_exact_search": (i32, [vp, i32, u32, u32, u64, u64, vp, u32, vp, vp, vp]),
        "hx_exact_search_filtered": (i32, [vp, i32, u32, u32, u64, u64, u32, vp, vp, u32, vp, vp, vp]),
        "hx_exact_range": (i32, [vp, i32, i32, vp, u32, u32, u64, u64, vp, i32, u64, vp, vp, vp, vp]),
        "hx_exact_range_filtered": (i32, [vp, i32, i32, vp, u32, u32, u64, u64, u32, vp, vp, i32, u64, vp, vp, vp, vp]),
        "hx_exact_rerank": (i32, [vp, i32, u32, u32, vp, vp, u32, vp, vp, vp]),
        "hx_filterset_create_labels": (i32, [vp, u64, u64, u32, vp, C.POINTER(vp)]),
        "hx_filterset_create_labels_device": (i32, [vp, u64, u64, u32, vp, C.POINTER(vp)]),
        "hx_filterset_create_bitmaps": (i32, [vp, u64, u64, u32, vp, C.POINTER(vp)]),
        "hx_filterset_append_labels": (i32, [vp, u64, vp]),
        "hx_filterset_info": (i32, [vp, C.POINTER(u64), C.POINTER(u64), C.POINTER(u32), C.POINTER(u64)]),
        "hx_filterset_counts": (i32, [vp, u32, u32, vp]),
        "hx_filterset_read": (i32, [vp, u32, u64, vp, C.POINTER(u64)]),
        "hx_filterset_destroy": (i32, [vp]),
        "hx_exact_search_set": (i32, [vp, i32, u32, u32, vp, vp, u32, vp, vp, vp]),
        "hx_exact_range_set": (i32, [vp, i32, i32, vp, u32, u32, vp, vp, i32, u64, vp, vp, vp, vp]),
        "hx_index_create": (i32, [vp, i32, i32, C.POINTER(vp)]),
        "hx_index_destroy": (i32, [vp]),
        "hx_index_last_error": (C.c_char_p, [vp]),
        "hx_index_set_threads": (i32, [vp, i32]),
        "hx_index_insert": (i32, [vp, u64, u32, vp, vp, u32, vp]),
        "hx_index_batch_begin": (i32, [vp, u64, u32, vp, vp]),
        "hx_index_batch_search": (i32, [vp, u32, u32]),
        "hx_index_batch_new_bytes": (u64, [vp, u32, u32]),
        "hx_index_batch_export_new": (i32, [vp, u32, u32, vp]),
        "hx_index_batch_import_new": (i32, [vp, u32, u32, vp]),
        "hx_index_batch_links": (i32, [vp, u32, u32]),
        "hx_index_batch_links_bytes": (u64, [vp]),
        "hx_index_batch_export_links": (i32, [vp, vp]),
        "hx_index_batch_import_links": (i32, [vp, vp, u64]),
        "hx_index_batch_end": (i32, [vp, vp]),
        "hx_index_insert_ondisk": (i32, [vp, u64, u32, vp, vp, u32, vp]),
        "hx_index_vacuum": (i32, [vp, vp, u64, u32, C.POINTER(u64), C.POINTER(u64)]),
        "hx_index_deleted": (i32, [vp, u32]),
        "hx_index_invalidate": (i32, [vp, u32, vp, vp, vp, C.POINTER(u32)]),
        "hx_index_dbatch_supported": (i32, [vp, vp, u32]),
        "hx_index_dbatch_record_bytes": (u64, [vp]),
        "hx_index_dbatch_list_record_bytes": (u64, [vp]),
        "hx_index_dbatch_begin": (i32, [vp, u64, u32, vp, vp]),
        "hx_index_dbatch_search": (i32, [vp, u32, u32, vp]),
        "hx_index_dbatch_links": (i32, [vp, u32, u32, vp, C.POINTER(u64)]),
        "hx_index_dbatch_export_links": (i32, [vp, vp]),
        "hx_index_dbatch_import_links": (i32, [vp, vp, u64]),
        "hx_index_dbatch_wtab_bytes": (u64, [vp]),
        "hx_index_dbatch_export_wtabs": (i32, [vp, u32, u32, vp]),
        "hx_index_dbatch_import_wtabs": (i32, [vp, u32, u32, vp]),
        "hx_index_dbatch_end": (i32, [vp, vp]),
        "hx_index_size": (u32, [vp]),
        "hx_index_entry": (i64, [vp]),
        "hx_index_level": (i32, [vp, u32]),
        "hx_index_neighbors": (i32, [vp, u32, i32, vp, vp]),
        "hx_index_heaptids": (i32, [vp, u32, vp]),
        "hx_index_export_levels": (i32, [vp, u32, u32, vp]),
        "hx_index_export_layer": (i32, [vp, i32, u32, u32, vp, vp, vp]),
        "hx_index_set_neighbors": (i32, [vp, u32, i32, u32, vp, vp]),
        "hx_index_counters": (i32, [vp, vp]),
        "hx_index_profile": (i32, [vp, vp, i32]),
        "hx_index_set_fused": (i32, [vp, i32]),
        "hx_index_set_mfma": (i32, [vp, i32]),
        "hx_index_mfma_stats": (i32, [vp, C.POINTER(u64), C.POINTER(u64)]),
        "hx_index_fused_stats": (i32, [vp, C.POINTER(u64), C.POINTER(u64)]),
        "hx_index_search": (i32, [vp, u32, u32, u32, vp, vp, vp, vp]),
        "hx_index_search_submit": (i32, [vp, u32, u32, u32, u32, u32]),
        "hx_index_search_wait": (i32, [vp, u32, vp, vp, vp, vp]),
        "hx_index_search_iterative": (i32, [vp, u32, u32, i32, i64, u32, vp, u64, vp, vp, vp]),
        "hx_index_search_filtered": (i32, [vp, u32, u32, i32, i64, u32, u32, vp, vp, vp, i32, vp, i32, vp, vp, vp, vp]),
        "hx_index_search_null": (i32, [vp, u32, i32, i64, u32, vp, u64, vp, vp, vp]),
        "hx_index_serialize_pages": (i32, [vp, vp, u64, C.POINTER(u64), vp, vp]),
        "hx_index_load_pages": (i32, [vp, vp, u64, vp, vp, u64, C.POINTER(u64)]),
    }
    for name, (res, args) in sig.items():
        if os.environ.get("HX_LIB") and not hasattr(L, name):
            continue                # an older variant library loaded for an A/B timing run (tools/qsweep.py) may lack newer entry points
        fn = getattr(L, name)       # AttributeError if the library lacks a declared symbol
        fn.restype, fn.argtypes = res, args
    _lib = L
    return L


ABI_SYMBOLS = None  # filled lazily by tests from include/hnswrx.h


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _u32(a):
    return np.ascontiguousarray(a, dtype=np.uint32)


def _row_words(row_pass, n_rows, packed):
    """A row filter as the C bitmap: None; a mask of n_rows entries (bool or any integer type: non-zero passes), packed here; or with
    packed=True the uint64 words as they are (ceil(n_rows / 64) of them)."""
    if row_pass is None:
        return None
    n_words = (n_rows + 63) // 64
    rp = np.asarray(row_pass)
    if packed:
        if rp.dtype != np.uint64 or rp.ndim != 1 or len(rp) < n_words:
            raise ValueError("packed row_pass needs ceil(n_rows / 64) uint64 words")
        return np.ascontiguousarray(rp)
    if rp.ndim != 1 or len(rp) != n_rows:
        raise ValueError("row_pass needs one entry per row")
    bits = np.zeros(n_words * 64, np.uint8)
    bits[:n_rows] = rp != 0
    return np.ascontiguousarray(np.packbits(bits, bitorder="little").view(np.uint64))


class Engine:
    """hx_engine: device row store + batched distance kernels (replaces graph::DistanceFn)."""

    def __init__(self, dtype, metric, dim, capacity, device=0, scan_only=False, sidecar=True, scan_sidecar=False):
        """scan_only: an engine for the scan plans and re-ranking (hx_create_ex HX_CREATE_SCAN_ONLY): vector / halfvec up to 16000 dims,
        never indexed.  sidecar=False: HX_CREATE_NO_SIDECAR (same results, no 8-bit row copy for the searches to skip rows with).
        scan_sidecar: HX_CREATE_SCAN_SIDECAR, a scan-only f32 L2 engine of more than 128 dims keeps the sidecar for the exact scans."""
        self.dtype, self.metric, self.dim = dtype, metric, dim
        h = C.c_void_p()
        flags = (CREATE_SCAN_ONLY if scan_only else 0) | (0 if sidecar else CREATE_NO_SIDECAR) | (CREATE_SCAN_SIDECAR if scan_sidecar else 0)
        rc = lib().hx_create_ex(device, dtype, metric, dim, int(capacity), flags, C.byref(h))
        if rc:
            raise HxError(rc, lib().hx_last_error(None).decode())
        self.h = h
        self.row_bytes = lib().hx_row_bytes(h)
        self._nq = 0

    def close(self):
        if getattr(self, "h", None):
            lib().hx_destroy(self.h)
            self.h = None

    __del__ = close

    def _ck(self, rc):
        if rc:
            raise HxError(rc, lib().hx_last_error(self.h).decode())

    def _rows(self, a):
        a = np.ascontiguousarray(a, dtype=_NP[self.dtype])
        if a.nbytes % self.row_bytes:
            raise ValueError("row payload size mismatch")
        return a, a.nbytes // self.row_bytes

    @property
    def num_rows(self):
        return lib().hx_num_rows(self.h)

    def append(self, rows):
        a, n = self._rows(rows)
        first = C.c_uint64()
        self._ck(lib().hx_append_rows(self.h, _p(a), n, C.byref(first)))
        return first.value

    def append_device(self, dev_ptr, n):
        first = C.c_uint64()
        self._ck(lib().hx_append_rows_device(self.h, C.c_void_p(dev_ptr), n, C.byref(first)))
        return first.value

    def pop(self, n):
        self._ck(lib().hx_pop_rows(self.h, n))

    def read_rows(self, first, n):
        out = np.empty((n, self.row_bytes // np.dtype(_NP[self.dtype]).itemsize), _NP[self.dtype])
        self._ck(lib().hx_read_rows(self.h, first, n, _p(out)))
        return out

    def sidecar_read(self, first, n):
        """(codes uint8 [n, dim], meta float32 [n, 3] = lo, step, e_x) of rows [first, first + n)"""
        codes = np.empty((n, self.dim), np.uint8)
        meta = np.empty((n, 3), np.float32)
        self._ck(lib().hx_sidecar_read(self.h, first, n, _p(codes), _p(meta)))
        return codes, meta

    def sidecar_stats(self, reset=False):
        """(f32 rows the index searches fetched, rows the sidecar bound let them skip) since the last reset"""
        a, b = C.c_uint64(), C.c_uint64()
        self._ck(lib().hx_sidecar_stats(self.h, C.byref(a), C.byref(b), int(reset)))
        return a.value, b.value

    def exact_sidecar_stats(self, reset=False):
        """(code rows read, f32 rows read) by the exact_search / exact_range calls that took the sidecar path since the last reset"""
        a, b = C.c_uint64(), C.c_uint64()
        self._ck(lib().hx_exact_sidecar_stats(self.h, C.byref(a), C.byref(b), int(reset)))
        return a.value, b.value

    def sidecar_bounds(self, query, row_ids):
        """the searches' lower bound of d(query, row) per row id (query: a row id, or QUERY_SLOT | slot)"""
        ids = _u32(row_ids)
        out = np.empty(len(ids), np.float32)
        self._ck(lib().hx_sidecar_bounds(self.h, query, _p(ids), len(ids), _p(out)))
        return out

    def normalize_rows(self, first, n):
        norms = np.empty(n, np.float64)
        self._ck(lib().hx_normalize_rows(self.h, first, n, _p(norms)))
        return norms

    def set_queries(self, q, normalize=False):
        a, n = self._rows(q)
        self._ck(lib().hx_set_queries(self.h, _p(a), n, int(normalize)))
        self._nq = n
        return n

    def set_queries_device(self, dev_ptr, n, normalize=False):
        self._ck(lib().hx_set_queries_device(self.h, C.c_void_p(dev_ptr), n, int(normalize)))
        self._nq = n

    def append_halfvec_from(self, src, first=0, n=None):
        """hx_append_rows_halfvec: appends `embedding::halfvec` of src's rows [first, first + n) (src: an F32 engine, self: F16), device to
        device, f32_to_half bit for bit.  Raises HxError E_RANGE (self unchanged) when a finite element does not fit a half."""
        n = src.num_rows - first if n is None else n
        out = C.c_uint64()
        self._ck(lib().hx_append_rows_halfvec(self.h, src.h, first, n, C.byref(out)))
        return out.value

    def set_queries_halfvec_from(self, src, normalize=False):
        """hx_set_queries_halfvec: self's query slots become the halfvec casts of all of src's uploaded query slots."""
        self._ck(lib().hx_set_queries_halfvec(self.h, src.h, int(normalize)))
        self._nq = src._nq
        return self._nq

    def distances(self, query, row_ids):
        q, _ = self._rows(query)
        ids = _u32(row_ids)
        out = np.empty(len(ids), np.float32)
        self._ck(lib().hx_distances(self.h, _p(q), _p(ids), len(ids), _p(out)))
        return out

    def distances_batch(self, group_query, group_offsets, row_ids):
        gq, go, ids = _u32(group_query), _u32(group_offsets), _u32(row_ids)
        out = np.empty(len(ids), np.float32)
        self._ck(lib().hx_distances_batch(self.h, len(gq), _p(gq), _p(go), _p(ids), _p(out)))
        return out

    def pairwise(self, ids):
        ids = _u32(ids)
        out = np.empty((len(ids), len(ids)), np.float32)
        self._ck(lib().hx_pairwise(self.h, _p(ids), len(ids), _p(out)))
        return out

    def pairwise_many(self, groups, mfma=False):
        """groups: list of (A_ids, B_ids or None).  Returns one array per group: packed lower triangle
        (B None) or an (na, nb) rectangle.  mfma: on the matrix cores (halfvec inner product; values in MFMA summation order);
        then also returns |row|^2 per id (concatenated A then B ids of every group)."""
        off, na, nb, ids, ooff, n_out = [0], [], [], [], [], 0
        for a, b in groups:
            b = [] if b is None else b
            ids.extend(a)
            ids.extend(b)
            na.append(len(a))
            nb.append(len(b))
            off.append(len(ids))
            ooff.append(n_out)
            n_out += len(a) * len(b) if len(b) else len(a) * (len(a) - 1) // 2
        off, ids = _u32(off), _u32(ids)
        na, nb = np.asarray(na, np.uint16), np.asarray(nb, np.uint16)
        ooff_a = np.asarray(ooff, np.uint64)
        out = np.empty(max(n_out, 1), np.float32)
        norm2 = np.empty(len(ids), np.float32) if mfma else None
        if mfma:
            self._ck(lib().hx_pairwise_many_mfma(self.h, len(groups), _p(off), _p(na), _p(nb), _p(ids), _p(ooff_a), _p(out), _p(norm2)))
        else:
            self._ck(lib().hx_pairwise_many(self.h, len(groups), _p(off), _p(na), _p(nb), _p(ids), _p(ooff_a), _p(out)))
        res = []
        for g, (a, b) in enumerate(groups):
            if b is None or len(b) == 0:
                res.append(out[ooff[g]:ooff[g] + len(a) * (len(a) - 1) // 2].copy())
            else:
                res.append(out[ooff[g]:ooff[g] + len(a) * len(b)].reshape(len(a), len(b)).copy())
        return (res, norm2) if mfma else res

    def rows_equal(self, a_ids, b_ids):
        a, b = _u32(a_ids), _u32(b_ids)
        out = np.empty(len(a), np.uint8)
        self._ck(lib().hx_rows_equal(self.h, len(a), _p(a), _p(b), _p(out)))
        return out.astype(bool)

    def set_timing(self, on=True):
        self._ck(lib().hx_set_timing(self.h, int(on)))

    def exact_search(self, op, k, first_query=0, nq=None, first_row=0, n_rows=None, row_pass=None, packed=False):
        """hx_exact_search: per query slot first_query.. (nq default: the rest of the uploaded slots), the k rows of [first_row, first_row + n_rows)
        nearest under the SQL operator `op` (OP_*), exact float8 values, ties by row id.  row_pass: None (every row), a mask of n_rows entries
        (bool or any integer type: non-zero passes; packed here), or with packed=True the uint64 words of the C bitmap as they are.
        Returns (ids uint32[nq, k], dist float64[nq, k], counts uint32[nq]); padding is id 0xFFFFFFFF, NaN."""
        nq = self._nq - first_query if nq is None else nq
        n_rows = self.num_rows - first_row if n_rows is None else n_rows
        words = _row_words(row_pass, n_rows, packed)
        ids = np.empty((nq, k), np.uint32)
        dist = np.empty((nq, k), np.float64)
        cnt = np.empty(nq, np.uint32)
        self._ck(lib().hx_exact_search(self.h, op, first_query, nq, first_row, n_rows, _p(words), k, _p(ids), _p(dist), _p(cnt)))
        return ids, dist, cnt

    def exact_search_filtered(self, op, k, filters, filter_of, first_query=0, nq=None, first_row=0, n_rows=None, packed=False):
        """hx_exact_search_filtered: exact_search with a row filter per query, in one call.  filters: a list of row_pass masks as exact_search
        takes them (packed=True: of uint64 word arrays); an entry that no query references may be None.  filter_of: per query the index of its
        filter, -1 for none (None: -1 for all).  Returns (ids, dist, counts) as exact_search does; row i is what exact_search would return for
        query i alone with row_pass = filters[filter_of[i]]."""
        nq = self._nq - first_query if nq is None else nq
        n_rows = self.num_rows - first_row if n_rows is None else n_rows
        words = [_row_words(f, n_rows, packed) for f in filters]
        ptrs = (C.c_void_p * max(1, len(words)))(*[None if w is None else w.ctypes.data for w in words])
        fo = None if filter_of is None else np.ascontiguousarray(filter_of, dtype=np.int32)
        if fo is not None and (fo.ndim != 1 or len(fo) != nq):
            raise ValueError("filter_of needs one entry per query")
        ids = np.empty((nq, k), np.uint32)
        dist = np.empty((nq, k), np.float64)
        cnt = np.empty(nq, np.uint32)
        self._ck(lib().hx_exact_search_filtered(self.h, op, first_query, nq, first_row, n_rows, len(words), ptrs if words else None, _p(fo), k,
                                                _p(ids), _p(dist), _p(cnt)))
        return ids, dist, cnt

    def exact_rerank(self, op, candidates, k, first_query=0):
        """hx_exact_rerank: per query slot first_query + i, the k rows of its candidate list nearest under the SQL operator `op` (OP_*), with
        exactly exact_search's values, order and padding.  candidates: a tuple (offsets, ids) in CSR form (offsets: nq + 1 entries from 0), or
        a list of per-query id arrays.  Returns (ids uint32[nq, k], dist float64[nq, k], counts uint32[nq])."""
        if isinstance(candidates, tuple):
            off, cand = np.ascontiguousarray(candidates[0], np.uint64), _u32(candidates[1])
        else:
            lists = [np.asarray(c, np.uint32).ravel() for c in candidates]
            off = np.zeros(len(lists) + 1, np.uint64)
            off[1:] = np.cumsum([len(c) for c in lists], dtype=np.uint64)
            cand = _u32(np.concatenate(lists) if lists else np.empty(0, np.uint32))
        nq = len(off) - 1
        ids = np.empty((nq, k), np.uint32)
        dist = np.empty((nq, k), np.float64)
        cnt = np.empty(nq, np.uint32)
        self._ck(lib().hx_exact_rerank(self.h, op, first_query, nq, _p(off), _p(cand), k, _p(ids), _p(dist), _p(cnt)))
        return ids, dist, cnt

    def exact_range(self, op, radius, cmp=CMP_LT, first_query=0, nq=None, first_row=0, n_rows=None, row_pass=None, packed=False,
                    ordered=False, count_only=False, cap=None):
        """hx_exact_range: per query slot first_query.. (nq default: the rest of the uploaded slots), every row of [first_row, first_row + n_rows)
        whose value under the SQL operator `op` (OP_*) satisfies `value <cmp> radius` (CMP_*, PostgreSQL's float8 comparison: -0.0 == +0.0,
        NaN above everything).  radius: a scalar or one value per query.  row_pass: as in exact_search.  ordered: by value, ties by row id
        (RANGE_BY_DISTANCE), else by row id (RANGE_BY_ROW).  Returns (offsets uint64[nq + 1], ids uint32[total], dist float64[total]), CSR:
        query i's rows are ids[offsets[i]:offsets[i + 1]]; count_only: the arrays are empty.  cap=None: one call with a default capacity,
        then, if the hits exceed it, one more sized to the total."""
        nq = self._nq - first_query if nq is None else nq
        n_rows = self.num_rows - first_row if n_rows is None else n_rows
        words = _row_words(row_pass, n_rows, packed)
        r = np.ascontiguousarray(np.broadcast_to(np.asarray(radius, np.float64), (nq,)))
        offsets = np.zeros(nq + 1, np.uint64)
        total = C.c_uint64()
        order = RANGE_BY_DISTANCE if ordered else RANGE_BY_ROW
        L = lib()
        if count_only:
            self._ck(L.hx_exact_range(self.h, op, cmp, _p(r), first_query, nq, first_row, n_rows, _p(words), order, 0, _p(offsets), None, None,
                                      C.byref(total)))
            return offsets, np.empty(0, np.uint32), np.empty(0, np.float64)
        n = max(1 << 16, 64 * nq) if cap is None else int(cap)
        for attempt in range(2):
            ids, dist = np.empty(max(n, 1), np.uint32), np.empty(max(n, 1), np.float64)
            rc = L.hx_exact_range(self.h, op, cmp, _p(r), first_query, nq, first_row, n_rows, _p(words), order, n, _p(offsets), _p(ids), _p(dist),
                                  C.byref(total))
            if rc == E_NOMEM and cap is None and attempt == 0 and total.value > n:
                n = total.value                              # sized to the total exactly: the second and last call
                continue
            self._ck(rc)
            break
        t = int(total.value)
        return offsets, ids[:t], dist[:t]

    def exact_range_filtered(self, op, radius, filters, filter_of, cmp=CMP_LT, first_query=0, nq=None, first_row=0, n_rows=None, packed=False,
                             ordered=False, count_only=False, cap=None):
        """hx_exact_range_filtered: exact_range with a row filter per query, in one call.  filters and filter_of as exact_search_filtered takes
        them; radius: a scalar or one value per query.  Returns what exact_range returns, (offsets, ids, dist) in CSR form: query i's part is
        what exact_range returns for query i alone with row_pass = filters[filter_of[i]].  cap=None: as in exact_range."""
        nq = self._nq - first_query if nq is None else nq
        n_rows = self.num_rows - first_row if n_rows is None else n_rows
        words = [_row_words(f, n_rows, packed) for f in filters]
        ptrs = (C.c_void_p * max(1, len(words)))(*[None if w is None else w.ctypes.data for w in words])
        fo = None if filter_of is None else np.ascontiguousarray(filter_of, dtype=np.int32)
        if fo is not None and (fo.ndim != 1 or len(fo) != nq):
            raise ValueError("filter_of needs one entry per query")
        r = np.ascontiguousarray(np.broadcast_to(np.asarray(radius, np.float64), (nq,)))
        offsets = np.zeros(nq + 1, np.uint64)
        total = C.c_uint64()
        order = RANGE_BY_DISTANCE if ordered else RANGE_BY_ROW
        L = lib()

        def call(n, ids, dist):
            return L.hx_exact_range_filtered(self.h, op, cmp, _p(r), first_query, nq, first_row, n_rows, len(words), ptrs if words else None, _p(fo),
                                             order, n, _p(offsets), _p(ids), _p(dist), C.byref(total))
        if count_only:
            self._ck(call(0, None, None))
            return offsets, np.empty(0, np.uint32), np.empty(0, np.float64)
        n = max(1 << 16, 64 * nq) if cap is None else int(cap)
        for attempt in range(2):
            ids, dist = np.empty(max(n, 1), np.uint32), np.empty(max(n, 1), np.float64)
            rc = call(n, ids, dist)
            if rc == E_NOMEM and cap is None and attempt == 0 and total.value > n:
                n = total.value                              # sized to the total exactly: the second and last call
                continue
            self._ck(rc)
            break
        t = int(total.value)
        return offsets, ids[:t], dist[:t]

    def exact_search_set(self, op, k, fset, filter_of, first_query=0, nq=None):
        """hx_exact_search_set: exact_search_filtered over the rows a FilterSet covers, with the set's resident lists in place of host bitmaps.
        filter_of: per query the index of its filter in the set, -1 for none (None: -1 for all); at most EXACT_MAX_FILTERS distinct ones per
        call.  Returns (ids, dist, counts): the bytes exact_search_filtered returns for the bitmaps the set represents."""
        nq = self._nq - first_query if nq is None else nq
        fo = None if filter_of is None else np.ascontiguousarray(filter_of, dtype=np.int32)
        if fo is not None and (fo.ndim != 1 or len(fo) != nq):
            raise ValueError("filter_of needs one entry per query")
        ids = np.empty((nq, k), np.uint32)
        dist = np.empty((nq, k), np.float64)
        cnt = np.empty(nq, np.uint32)
        self._ck(lib().hx_exact_search_set(self.h, op, first_query, nq, fset.h, _p(fo), k, _p(ids), _p(dist), _p(cnt)))
        return ids, dist, cnt

    def exact_range_set(self, op, radius, fset, filter_of, cmp=CMP_LT, first_query=0, nq=None, ordered=False, count_only=False, cap=None,
                        values=True):
        """hx_exact_range_set: exact_range_filtered over the rows a FilterSet covers, with the set's resident lists in place of host bitmaps.
        filter_of as in exact_search_set; radius: a scalar or one value per query; values=False: ids without values (dist comes back empty).
        Returns (offsets, ids, dist) in CSR form: the bytes exact_range_filtered returns for the bitmaps the set represents.  cap=None: as in
        exact_range."""
        nq = self._nq - first_query if nq is None else nq
        fo = None if filter_of is None else np.ascontiguousarray(filter_of, dtype=np.int32)
        if fo is not None and (fo.ndim != 1 or len(fo) != nq):
            raise ValueError("filter_of needs one entry per query")
        r = np.ascontiguousarray(np.broadcast_to(np.asarray(radius, np.float64), (nq,)))
        offsets = np.zeros(nq + 1, np.uint64)
        total = C.c_uint64()
        order = RANGE_BY_DISTANCE if ordered else RANGE_BY_ROW
        L = lib()

        def call(n, ids, dist):
            return L.hx_exact_range_set(self.h, op, cmp, _p(r), first_query, nq, fset.h, _p(fo), order, n, _p(offsets), _p(ids), _p(dist),
                                        C.byref(total))
        if count_only:
            self._ck(call(0, None, None))
            return offsets, np.empty(0, np.uint32), np.empty(0, np.float64)
        n = max(1 << 16, 64 * nq) if cap is None else int(cap)
        for attempt in range(2):
            ids, dist = np.empty(max(n, 1), np.uint32), (np.empty(max(n, 1), np.float64) if values else None)
            rc = call(n, ids, dist)
            if rc == E_NOMEM and cap is None and attempt == 0 and total.value > n:
                n = total.value                              # sized to the total exactly: the second and last call
                continue
            self._ck(rc)
            break
        t = int(total.value)
        return offsets, ids[:t], (dist[:t] if values else np.empty(0, np.float64))

    def kernel_stats(self, kind, reset=False):
        l, u, ms = C.c_uint64(), C.c_uint64(), C.c_double()
        self._ck(lib().hx_kernel_stats(self.h, kind, C.byref(l), C.byref(u), C.byref(ms), int(reset)))
        return {"launches": l.value, "units": u.value, "ms": ms.value}


class FilterSet:
    """hx_filterset: the filters of the exact scans as row-id lists resident on the device (one ascending list per filter), made once from a label
    column or from bitmaps and extended as rows are appended.  Engine.exact_search_set / exact_range_set take it in place of host bitmaps.  It
    borrows the engine (and keeps it alive)."""

    def __init__(self, engine, handle):
        self.engine, self.h = engine, handle

    @classmethod
    def from_labels(cls, engine, labels, n_filters, first_row=0, device_ptr=None, n_rows=None):
        """Row first_row + i is in filter labels[i]; NO_LABEL: in no filter.  device_ptr: the uint32 label column in device memory instead
        (n_rows entries; labels is ignored)."""
        h = C.c_void_p()
        if device_ptr is not None:
            rc = lib().hx_filterset_create_labels_device(engine.h, first_row, int(n_rows), n_filters, C.c_void_p(device_ptr), C.byref(h))
        else:
            lb = _u32(labels)
            rc = lib().hx_filterset_create_labels(engine.h, first_row, len(lb), n_filters, _p(lb), C.byref(h))
        engine._ck(rc)
        return cls(engine, h)

    @classmethod
    def from_bitmaps(cls, engine, filters, n_rows=None, first_row=0, packed=False):
        """filters: a list of row masks as Engine.exact_search_filtered takes them (packed=True: uint64 word arrays); None: an empty filter."""
        n_rows = engine.num_rows - first_row if n_rows is None else n_rows
        words = [_row_words(f, n_rows, packed) for f in filters]
        ptrs = (C.c_void_p * max(1, len(words)))(*[None if w is None else w.ctypes.data for w in words])
        h = C.c_void_p()
        engine._ck(lib().hx_filterset_create_bitmaps(engine.h, first_row, n_rows, len(words), ptrs, C.byref(h)))
        return cls(engine, h)

    def _ck(self, rc):
        self.engine._ck(rc)

    def append_labels(self, labels):
        """Extends the coverage by the next len(labels) rows, which must already be in the engine."""
        lb = _u32(labels)
        self._ck(lib().hx_filterset_append_labels(self.h, len(lb), _p(lb)))

    def info(self):
        a, b, c, d = C.c_uint64(), C.c_uint64(), C.c_uint32(), C.c_uint64()
        self._ck(lib().hx_filterset_info(self.h, C.byref(a), C.byref(b), C.byref(c), C.byref(d)))
        return {"first_row": a.value, "n_rows": b.value, "n_filters": c.value, "n_listed": d.value}

    def counts(self, first=0, n=None):
        n = self.info()["n_filters"] - first if n is None else n
        out = np.empty(n, np.uint64)
        self._ck(lib().hx_filterset_counts(self.h, first, n, _p(out)))
        return out

    def read(self, f):
        """The ascending row ids filter f passes."""
        n = int(self.counts(f, 1)[0])
        out = np.empty(n, np.uint32)
        got = C.c_uint64()
        self._ck(lib().hx_filterset_read(self.h, f, n, _p(out) if n else None, C.byref(got)))
        return out[:got.value]

    def close(self):
        if getattr(self, "h", None):
            lib().hx_filterset_destroy(self.h)
            self.h = None

    __del__ = close


class Index:
    """hx_index: host-side HNSW graph (graph/mod.rs + build.rs + scan.rs control flow) over an Engine."""

    def __init__(self, engine, m=16, ef_construction=64):
        self.engine, self.m, self.efc = engine, m, ef_construction
        h = C.c_void_p()
        rc = lib().hx_index_create(engine.h, m, ef_construction, C.byref(h))
        if rc:
            raise HxError(rc, lib().hx_last_error(engine.h).decode())
        self.h = h

    def close(self):
        if getattr(self, "h", None):
            lib().hx_index_destroy(self.h)
            self.h = None

    __del__ = close

    def _ck(self, rc):
        if rc:
            raise HxError(rc, lib().hx_index_last_error(self.h).decode())

    def set_threads(self, n):
        self._ck(lib().hx_index_set_threads(self.h, n))

    def insert(self, first_row, levels, tids=None, batch=1):
        levels = np.ascontiguousarray(levels, np.int32)
        n = len(levels)
        tids = np.arange(first_row, first_row + n, dtype=np.int64) if tids is None else np.ascontiguousarray(tids, np.int64)
        out = np.empty(n, np.uint32)
        self._ck(lib().hx_index_insert(self.h, first_row, n, _p(levels), _p(tids), batch, _p(out)))
        return out

    def insert_ondisk(self, first_row, levels, tids=None, batch=1):
        """aminsert (insert.rs:1227-1480) for rows already appended to the engine."""
        levels = np.ascontiguousarray(levels, np.int32)
        n = len(levels)
        tids = np.arange(first_row, first_row + n, dtype=np.int64) if tids is None else np.ascontiguousarray(tids, np.int64)
        out = np.empty(n, np.uint32)
        self._ck(lib().hx_index_insert_ondisk(self.h, first_row, n, _p(levels), _p(tids), batch, _p(out)))
        return out

    def vacuum(self, dead_tids, batch=1):
        """ambulkdelete + amvacuumcleanup (vacuum.rs); returns (elements marked deleted, elements repaired)."""
        d = np.ascontiguousarray(dead_tids, np.int64)
        nd, nr = C.c_uint64(0), C.c_uint64(0)
        self._ck(lib().hx_index_vacuum(self.h, _p(d), len(d), batch, C.byref(nd), C.byref(nr)))
        return nd.value, nr.value

    def deleted(self, e):
        return lib().hx_index_deleted(self.h, e)

    def invalidate(self, blkno, offno, versions=None):
        """Drops loaded elements whose tuple version changed (scan.rs:262-265); returns how many were dropped."""
        b = np.ascontiguousarray(blkno, np.uint32)
        o = np.ascontiguousarray(offno, np.uint16)
        v = None if versions is None else np.ascontiguousarray(versions, np.uint8)
        nd = C.c_uint32(0)
        self._ck(lib().hx_index_invalidate(self.h, len(b), _p(b), _p(o), _p(v), C.byref(nd)))
        return nd.value

    # ---- staged batch (multi-GPU build; see dist_build.py) ----
    def batch_begin(self, first_row, levels, tids):
        levels = np.ascontiguousarray(levels, np.int32)
        tids = np.ascontiguousarray(tids, np.int64)
        self._ck(lib().hx_index_batch_begin(self.h, first_row, len(levels), _p(levels), _p(tids)))

    def batch_search(self, lo, hi):
        self._ck(lib().hx_index_batch_search(self.h, lo, hi))

    def batch_new_bytes(self, lo, hi):
        return lib().hx_index_batch_new_bytes(self.h, lo, hi)

    def batch_export_new(self, lo, hi):
        buf = np.empty(self.batch_new_bytes(lo, hi), np.uint8)
        self._ck(lib().hx_index_batch_export_new(self.h, lo, hi, _p(buf)))
        return buf

    def batch_import_new(self, lo, hi, buf):
        buf = np.ascontiguousarray(buf, np.uint8)
        assert buf.nbytes == self.batch_new_bytes(lo, hi)
        self._ck(lib().hx_index_batch_import_new(self.h, lo, hi, _p(buf)))

    def batch_links(self, rank, world):
        self._ck(lib().hx_index_batch_links(self.h, rank, world))

    def batch_links_bytes(self):
        return lib().hx_index_batch_links_bytes(self.h)

    def batch_export_links(self):
        buf = np.empty(self.batch_links_bytes(), np.uint8)
        self._ck(lib().hx_index_batch_export_links(self.h, _p(buf)))
        return buf

    def batch_import_links(self, buf):
        buf = np.ascontiguousarray(buf, np.uint8)
        self._ck(lib().hx_index_batch_import_links(self.h, _p(buf), buf.nbytes))

    def batch_end(self, n):
        out = np.empty(n, np.uint32)
        self._ck(lib().hx_index_batch_end(self.h, _p(out)))
        return out

    # ---- device-resident staged batch: the buffers are DEVICE pointers (ints), e.g. torch tensors' data_ptr() ----
    def dbatch_supported(self, levels):
        levels = np.ascontiguousarray(levels, np.int32)
        return bool(lib().hx_index_dbatch_supported(self.h, _p(levels), len(levels)))

    @property
    def dbatch_record_bytes(self):
        return lib().hx_index_dbatch_record_bytes(self.h)

    @property
    def dbatch_list_record_bytes(self):
        return lib().hx_index_dbatch_list_record_bytes(self.h)

    def dbatch_begin(self, first_row, levels, tids):
        levels = np.ascontiguousarray(levels, np.int32)
        tids = np.ascontiguousarray(tids, np.int64)
        self._ck(lib().hx_index_dbatch_begin(self.h, first_row, len(levels), _p(levels), _p(tids)))

    def dbatch_search(self, lo, hi, d_records):
        self._ck(lib().hx_index_dbatch_search(self.h, lo, hi, C.c_void_p(d_records)))

    def dbatch_links(self, rank, world, d_records):
        n = C.c_uint64(0)
        self._ck(lib().hx_index_dbatch_links(self.h, rank, world, C.c_void_p(d_records), C.byref(n)))
        return n.value

    def dbatch_export_links(self, d_out):
        self._ck(lib().hx_index_dbatch_export_links(self.h, C.c_void_p(d_out)))

    def dbatch_import_links(self, d_list_records, n):
        self._ck(lib().hx_index_dbatch_import_links(self.h, C.c_void_p(d_list_records), n))

    @property
    def dbatch_wtab_bytes(self):
        """Bytes per member of the W-table exchange of the open device batch (0: tables off)."""
        return lib().hx_index_dbatch_wtab_bytes(self.h)

    def dbatch_export_wtabs(self, lo, hi, d_out):
        self._ck(lib().hx_index_dbatch_export_wtabs(self.h, lo, hi, C.c_void_p(d_out)))

    def dbatch_import_wtabs(self, lo, hi, d_in):
        self._ck(lib().hx_index_dbatch_import_wtabs(self.h, lo, hi, C.c_void_p(d_in)))

    def dbatch_end(self, n):
        out = np.empty(n, np.uint32)
        self._ck(lib().hx_index_dbatch_end(self.h, _p(out)))
        return out

    @property
    def size(self):
        return lib().hx_index_size(self.h)

    @property
    def entry(self):
        return lib().hx_index_entry(self.h)

    def level(self, e):
        return lib().hx_index_level(self.h, e)

    def neighbors(self, e, layer):
        ids = np.empty(2 * self.m, np.uint32)
        d = np.empty(2 * self.m, np.float32)
        n = lib().hx_index_neighbors(self.h, e, layer, _p(ids), _p(d))
        if n < 0:
            return None, None
        return ids[:n].copy(), d[:n].copy()

    def heaptids(self, e):
        t = np.empty(10, np.int64)
        n = lib().hx_index_heaptids(self.h, e, _p(t))
        return t[:n].tolist()

    def export_levels(self, first=0, n=None):
        n = self.size - first if n is None else n
        out = np.empty(n, np.int32)
        self._ck(lib().hx_index_export_levels(self.h, first, n, _p(out)))
        return out

    def export_layer(self, layer, first=0, n=None, with_dist=True):
        n = self.size - first if n is None else n
        lm = 2 * self.m if layer == 0 else self.m
        ids = np.zeros((n, lm), np.uint32)
        d = np.zeros((n, lm), np.float32) if with_dist else None
        cnt = np.zeros(n, np.uint16)
        self._ck(lib().hx_index_export_layer(self.h, layer, first, n, _p(ids), _p(d), _p(cnt)))
        return ids, d, cnt

    def set_neighbors(self, e, layer, ids, dist):
        ids, dist = _u32(ids), np.ascontiguousarray(dist, np.float32)
        self._ck(lib().hx_index_set_neighbors(self.h, e, layer, len(ids), _p(ids), _p(dist)))

    def counters(self):
        c = np.zeros(8, np.uint64)
        self._ck(lib().hx_index_counters(self.h, _p(c)))
        return c

    def profile(self, reset=False):
        p = np.zeros(16, np.float64)
        self._ck(lib().hx_index_profile(self.h, _p(p), int(reset)))
        return {"advance_s": p[0], "compact_s": p[1], "fill_s": p[2], "round_s": p[3], "rounds": int(p[5]), "fused_s": p[6],
                "mirror_sync_s": p[7], "links_setup_s": p[8], "links_lockstep_s": p[9], "insert_total_s": p[10],
                "batch_search_s": p[11], "batch_begin_s": p[12], "links_max_chain": int(p[13]), "links_ops": int(p[14])}

    def serialize_pages(self):
        """hx_index_serialize_pages: (pages uint8 [n_pages, 8192], elem_blkno[n], elem_offno[n])."""
        n = self.size
        npg = C.c_uint64()
        self._ck(lib().hx_index_serialize_pages(self.h, None, 0, C.byref(npg), None, None))
        pages = np.zeros((npg.value, 8192), np.uint8)
        blk = np.zeros(max(n, 1), np.uint32)
        off = np.zeros(max(n, 1), np.uint16)
        self._ck(lib().hx_index_serialize_pages(self.h, _p(pages), npg.value, C.byref(npg), _p(blk), _p(off)))
        return pages, blk[:n], off[:n]

    def load_pages(self, pages):
        """hx_index_load_pages: fills the (empty) index and engine from a page image; returns (elem_blkno, elem_offno)."""
        pages = np.ascontiguousarray(pages, np.uint8).reshape(-1, 8192)
        cap = len(pages) * 400          # an 8 KB page holds fewer than 400 element tuples
        blk = np.zeros(max(cap, 1), np.uint32)
        off = np.zeros(max(cap, 1), np.uint16)
        n = C.c_uint64()
        self._ck(lib().hx_index_load_pages(self.h, _p(pages), len(pages), _p(blk), _p(off), cap, C.byref(n)))
        return blk[:n.value], off[:n.value]

    def set_fused(self, on):
        self._ck(lib().hx_index_set_fused(self.h, int(on)))

    def set_mfma(self, on):
        self._ck(lib().hx_index_set_mfma(self.h, int(on)))

    def mfma_stats(self):
        a, b = C.c_uint64(), C.c_uint64()
        self._ck(lib().hx_index_mfma_stats(self.h, C.byref(a), C.byref(b)))
        return {"mfma_pairs": a.value, "exact_pairs": b.value}

    def fused_stats(self):
        a, b = C.c_uint64(), C.c_uint64()
        self._ck(lib().hx_index_fused_stats(self.h, C.byref(a), C.byref(b)))
        return {"tasks": a.value, "redone": b.value & 0xFFFFFFFF, "max_candidate_heap": b.value >> 32}

    @staticmethod
    def _pad(cnt, k, *arrays_and_fills):
        """The ABI defines the first counts_out[q] entries of a row; the rest is set here (-1 / inf / 0), and only for the rows that are short --
        pre-filling 1.6 MB per 10 000-query call cost 3 % of the bench's step time."""
        short = np.nonzero(cnt < k)[0]
        if short.size:
            tail = np.arange(k)[None, :] >= cnt[short, None]
            for a, fill in arrays_and_fills:
                sub = a[short]
                sub[tail] = fill
                a[short] = sub

    def search(self, nq, ef_search, k):
        tids = np.empty((nq, k), np.int64)
        d = np.empty((nq, k), np.float32)
        el = np.empty((nq, k), np.uint32)
        cnt = np.zeros(nq, np.uint32)
        self._ck(lib().hx_index_search(self.h, nq, ef_search, k, _p(tids), _p(d), _p(el), _p(cnt)))
        self._pad(cnt, k, (tids, -1), (d, np.inf), (el, 0))
        return tids, d, el, cnt

    def search_submit(self, slot, first_query, nq, ef_search, k):
        """Pipelined scan: launches the scan of engine query slots [first_query, first_query + nq) on `slot` and returns at once."""
        self._ck(lib().hx_index_search_submit(self.h, slot, first_query, nq, ef_search, k))
        self._scan_shape = getattr(self, "_scan_shape", {})
        self._scan_shape[slot] = (nq, k)

    def search_wait(self, slot):
        """Results of the scan submitted on `slot`: as search()."""
        if slot not in getattr(self, "_scan_shape", {}):
            raise HxError(-6, "nothing submitted on this scan slot")
        nq, k = self._scan_shape.pop(slot)
        tids = np.empty((nq, k), np.int64)
        d = np.empty((nq, k), np.float32)
        el = np.empty((nq, k), np.uint32)
        cnt = np.zeros(nq, np.uint32)
        self._ck(lib().hx_index_search_wait(self.h, slot, _p(tids), _p(d), _p(el), _p(cnt)))
        self._pad(cnt, k, (tids, -1), (d, np.inf), (el, 0))
        return tids, d, el, cnt

    def search_null(self, ef_search, limit, mode=0, max_scan_tuples=20000, filter_pass=None):
        """ORDER BY val <-> NULL (scan.rs:186-187): (tids, elems) of the traversal with every distance 0.0."""
        tids = np.full(limit, -1, np.int64)
        el = np.zeros(limit, np.uint32)
        cnt = C.c_uint32()
        f = None if filter_pass is None else np.ascontiguousarray(filter_pass, np.uint8)
        self._ck(lib().hx_index_search_null(self.h, ef_search, mode, max_scan_tuples, limit, _p(f), 0 if f is None else len(f), _p(tids), _p(el), C.byref(cnt)))
        return tids[:cnt.value], el[:cnt.value]

    def search_iterative(self, nq, ef_search, mode, max_scan_tuples, limit, filter_pass=None):
        tids = np.empty((nq, limit), np.int64)
        d = np.empty((nq, limit), np.float32)
        cnt = np.zeros(nq, np.uint32)
        f = None if filter_pass is None else np.ascontiguousarray(filter_pass, np.uint8)
        self._ck(lib().hx_index_search_iterative(self.h, nq, ef_search, mode, max_scan_tuples, limit, _p(f),
                                                 0 if f is None else len(f), _p(tids), _p(d), _p(cnt)))
        self._pad(cnt, limit, (tids, -1), (d, np.inf))
        return tids, d, cnt

    def search_filtered(self, nq, ef_search, mode, max_scan_tuples, limit, filters=None, filter_of=None, cmp=None, radius=None,
                        stop_past_radius=False):
        """Iterative scan with a WHERE clause per query (hx_index_search_filtered): query q is filtered by filters[filter_of[q]] (-1: none) and
        by `value <cmp> radius[q]` (cmp: one of CMP_LT / CMP_LE / CMP_GT / CMP_GE, None: no predicate).  Returns (tids, distances, elements, counts)."""
        tids = np.empty((nq, limit), np.int64)
        d = np.empty((nq, limit), np.float32)
        el = np.empty((nq, limit), np.uint32)
        cnt = np.zeros(nq, np.uint32)
        fl = [np.ascontiguousarray(f, np.uint8) for f in (filters or [])]
        ptrs = (C.c_void_p * max(len(fl), 1))(*[f.ctypes.data for f in fl])
        lens = np.array([len(f) for f in fl], np.uint64)
        fo = None if filter_of is None else np.ascontiguousarray(filter_of, np.int32)
        if fo is not None and len(fo) != nq:
            raise ValueError("filter_of needs one entry per query")
        r = None if radius is None else np.ascontiguousarray(np.broadcast_to(np.asarray(radius, np.float64), (nq,)))
        self._ck(lib().hx_index_search_filtered(self.h, nq, ef_search, mode, max_scan_tuples, limit, len(fl), C.cast(ptrs, C.c_void_p) if fl else None,
                                                _p(lens) if fl else None, _p(fo), -1 if cmp is None else int(cmp), _p(r),
                                                SCAN_STOP_PAST_RADIUS if stop_past_radius else 0, _p(tids), _p(d), _p(el), _p(cnt)))
        self._pad(cnt, limit, (tids, -1), (d, np.inf), (el, 0))
        return tids, d, el, cnt
