"""Reference model of hx_exact_search composed from the oracle (test infrastructure only): the operator functions' float8 values in the
device's canonical summation order (orc.W64), ordered under PostgreSQL's float8 comparison, ties by ascending row id."""
import numpy as np

import pgvector_rx_amd as hx
from oracle import orc

# SQL operator -> the support function whose W64 value it is built on
_SUPPORT = {hx.OP_L2: orc.L2SQ, hx.OP_NEG_IP: orc.NEG_IP, hx.OP_L1: orc.L1, hx.OP_HAMMING: orc.HAMMING, hx.OP_JACCARD: orc.JACCARD}


def self_ip(dtype, dim, rows):
    """W64 sum of x*x per row (the cosine norm accumulator): -NEG_IP(r, r)."""
    return np.array([-orc.distance(dtype, orc.NEG_IP, dim, r, r, orc.W64) for r in rows], np.float64)


def values(dtype, dim, op, q, rows, row_norms=None):
    """Operator values of query q against every row of `rows` (f64)."""
    if dtype == orc.SPARSE and op == hx.OP_COSINE:
        L, qa, ra = orc.lib(), orc.as_rows(dtype, q), orc.as_rows(dtype, rows)       # one record per row: addressed in place
        fn, qp, base, rb = L.orc_cosine_distance, orc._p(qa), ra.ctypes.data, ra.nbytes // max(len(ra), 1)
        return np.array([fn(dtype, dim, qp, base + i * rb) for i in range(len(ra))], np.float64)
    if op == hx.OP_COSINE:
        s = -orc.distances_many(dtype, orc.NEG_IP, dim, q, rows, order=orc.W64)
        na = self_ip(dtype, dim, rows) if row_norms is None else row_norms
        nb = self_ip(dtype, dim, [q])[0]
        with np.errstate(all="ignore"):
            sim = s / np.sqrt(na * nb)
        return 1.0 - np.clip(sim, -1.0, 1.0)           # np.clip keeps NaN, as f64::clamp
    v = orc.distances_many(dtype, _SUPPORT[op], dim, q, rows, order=orc.W64)
    if op == hx.OP_L2:
        with np.errstate(all="ignore"):
            v = np.sqrt(v)
    return v


def order(vals, ids):
    """Indices sorting (vals, ids) under float8 comparison: -0.0 == +0.0, +inf < NaN, NaNs equal, then id."""
    nan = np.isnan(vals)
    v = np.where(nan | (vals == 0), 0.0, vals)
    return np.lexsort((ids, v, nan))


def topk(dtype, dim, op, q, rows, k, ids=None, row_norms=None):
    """(ids, values) of the first k rows; `rows` are the candidate rows, `ids` their row ids (default 0..n-1)."""
    ids = np.arange(len(rows), dtype=np.int64) if ids is None else np.asarray(ids, np.int64)
    if len(ids) == 0:
        return ids, np.empty(0)
    v = values(dtype, dim, op, q, rows, row_norms)
    o = order(v, ids)[:k]
    return ids[o], v[o]


def same_bits(got, want):
    """f64 equality bit for bit, NaN matching NaN (its payload is the platform's)."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    both_nan = np.isnan(got) & np.isnan(want)
    return bool(np.all(both_nan | (got.view(np.uint64) == want.view(np.uint64))))
