"""hx_exact_rerank: the outer `ORDER BY v <op> q LIMIT k` over per-query candidate lists, checked bit for bit against the oracle composed in
tests/exact_ref.py and against hx_exact_search; scan-only engines up to 16000 dimensions; and the halfvec-expression-index plan end to end."""
import ctypes

import numpy as np
import pytest

import pgvector_rx_amd as hx
import exact_ref as ref
from oracle import orc
from test_gpu_exact import BOPS, FOPS, NOT_FOUND, engine, make

E_ARG, E_STATE = -1, -6


def same(a, b):
    return all((x.view(np.uint8) == y.view(np.uint8)).all() for x, y in zip(a, b))


def check(e, dtype, dim, op, rows, queries, lists, k, first_query=0, norms=None):
    """Re-ranks `lists` (one id array per query) and compares ids and value bits with the composed reference; returns the outputs."""
    ids, dist, cnt = e.exact_rerank(op, lists, k, first_query=first_query)
    for qi, cand in enumerate(lists):
        cand = np.asarray(cand, np.int64)
        want_ids, want_d = ref.topk(dtype, dim, op, queries[first_query + qi], rows[cand], k, ids=cand,
                                    row_norms=None if norms is None else norms[cand])
        c = int(cnt[qi])
        assert c == len(want_ids) == min(k, len(cand)), (qi, c, len(want_ids))
        assert ids[qi, :c].tolist() == want_ids.tolist(), (op, qi)
        assert ref.same_bits(dist[qi, :c], want_d), (op, qi)
        assert (ids[qi, c:] == NOT_FOUND).all() and np.isnan(dist[qi, c:]).all()
    return ids, dist, cnt


# ---- 1. parity: every dtype x operator, list lengths around k and around a chunk, duplicates ------------------------------------------------
CASES = [(hx.F32, 3), (hx.F32, 768), (hx.F16, 10), (hx.F16, 1000), (hx.BIT, 8), (hx.BIT, 1024), (hx.SPARSE, 100)]


@pytest.mark.gpu
@pytest.mark.parametrize("dtype,dim", CASES, ids=lambda v: str(v))
def test_parity_matrix(dtype, dim):
    rng = np.random.default_rng(31 + dim + 10 * dtype)
    n, k = 1200, 10
    rows, qs = make(dtype, n, dim, rng), make(dtype, 16, dim, rng)
    if dtype != hx.SPARSE:
        rows[7] = rows[3]                                               # equal rows: ties by id
    lens = [0, 1, k - 1, k, k + 1, 15, 16, 17, 255, 256, 257, 600]
    lists = [rng.integers(0, n, L) for L in lens]
    lists[-1][:50] = 3                                                  # an id listed many times, and its twin row 7
    lists[-1][50:60] = 7
    for op in (BOPS if dtype == hx.BIT else FOPS):
        e = engine(dtype, dim, op, rows, qs)
        norms = ref.self_ip(dtype, dim, rows) if op == hx.OP_COSINE and dtype != hx.SPARSE else None
        ids, _, cnt = check(e, dtype, dim, op, rows, qs, lists, k, norms=norms)
        assert cnt.tolist() == [min(k, L) for L in lens]
        check(e, dtype, dim, op, rows, qs, lists[:4], 300, first_query=12, norms=norms)   # k beyond the lists: padding
        e.close()


@pytest.mark.gpu
def test_long_lists_and_windows(monkeypatch):
    """70 000 candidates for one query (many chunks), k = HX_EXACT_MAX_K; then scratch so small that lists straddle windows: same result."""
    rng = np.random.default_rng(41)
    n, dim = 20000, 64
    rows, qs = make(hx.F32, n, dim, rng), make(hx.F32, 4, dim, rng)
    e = engine(hx.F32, dim, hx.OP_L2, rows, qs)
    lists = [rng.integers(0, n, 70000), rng.integers(0, n, 3000), np.empty(0, np.int64), rng.integers(0, n, 5)]
    full = check(e, hx.F32, dim, hx.OP_L2, rows, qs, lists, 1024)
    one = check(e, hx.F32, dim, hx.OP_L2, rows, qs, lists[:1], 10)
    monkeypatch.setenv("HX_EXACT_SCRATCH", str(1 << 20))
    assert same(full, e.exact_rerank(hx.OP_L2, lists, 1024))
    assert same(one, e.exact_rerank(hx.OP_L2, lists[:1], 10))
    monkeypatch.setenv("HX_EXACT_SCRATCH", "1")                         # one chunk and one query per window
    assert same(full, e.exact_rerank(hx.OP_L2, lists, 1024))
    e.close()


@pytest.mark.gpu
def test_special_values():
    rng = np.random.default_rng(43)
    rows = make(hx.F32, 200, 8, rng)
    rows[[5, 50, 77]] = 0
    qs = np.concatenate([np.zeros((1, 8), np.float32), make(hx.F32, 1, 8, rng)])
    e = engine(hx.F32, 8, hx.OP_COSINE, rows, qs)
    norms = ref.self_ip(hx.F32, 8, rows)
    lists = [np.arange(200), np.arange(200)[::-1]]
    ids, d, _ = check(e, hx.F32, 8, hx.OP_COSINE, rows, qs, lists, 200, norms=norms)   # NaN last, by id
    assert np.isnan(d[0]).all() and ids[0].tolist() == list(range(200)) and ids[1, -3:].tolist() == [5, 50, 77]
    rows = make(hx.F32, 100, 4, rng)
    rows[::3, 0] = 0
    e2 = engine(hx.F32, 4, hx.OP_NEG_IP, rows, np.array([[1, 0, 0, 0]], np.float32))
    ids, d, _ = e2.exact_rerank(hx.OP_NEG_IP, [np.arange(100)], 100)
    z = d[0] == 0
    assert z.sum() == 34 and np.signbit(d[0][z]).all() and ids[0][z].tolist() == list(range(0, 100, 3))
    e.close()
    e2.close()


@pytest.mark.gpu
def test_bitmap_list_equals_exact_search():
    rng = np.random.default_rng(47)
    n, dim = 5000, 200
    rows, qs = make(hx.F16, n, dim, rng), make(hx.F16, 20, dim, rng)
    e = engine(hx.F16, dim, hx.OP_L2, rows, qs)
    mask = rng.random(n) < 0.2
    passing = np.nonzero(mask)[0]
    for op, k in ((hx.OP_L2, 10), (hx.OP_COSINE, 100), (hx.OP_L1, 1024)):
        want = e.exact_search(op, k, row_pass=mask)
        got = e.exact_rerank(op, [passing] * 20, k)
        assert same(want, got), op
        got = e.exact_rerank(op, [rng.permutation(passing) for _ in range(20)], k)   # the list's order does not matter
        assert same(want, got), op
    e.close()


# ---- 2. argument errors, stats, concurrency --------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_argument_errors_and_stats():
    rng = np.random.default_rng(53)
    rows, qs = make(hx.F32, 100, 8, rng), make(hx.F32, 4, 8, rng)
    e = engine(hx.F32, 8, hx.OP_L2, rows, qs)
    L, P = hx.lib(), lambda a: a.ctypes.data_as(ctypes.c_void_p)
    off, cand = np.array([0, 3, 3, 5, 8], np.uint64), np.array([1, 2, 3, 4, 5, 6, 7, 99], np.uint32)
    ids, d, c = np.empty(4 * 1024, np.uint32), np.empty(4 * 1024, np.float64), np.empty(4, np.uint32)

    def call(op=hx.OP_L2, fq=0, nq=4, o=off, cd=cand, k=10, i=True, dd=True, cc=True):
        return L.hx_exact_rerank(e.h, op, fq, nq, None if o is None else P(o), None if cd is None else P(cd), k,
                                 P(ids) if i else None, P(d) if dd else None, P(c) if cc else None)
    assert call() == 0
    assert call(op=hx.OP_HAMMING) == E_ARG and call(op=hx.OP_JACCARD) == E_ARG and call(op=6) == E_ARG and call(op=-1) == E_ARG
    assert call(k=0) == E_ARG and call(k=1025) == E_ARG and call(k=1024) == 0
    assert call(cd=np.array([1, 2, 3, 4, 5, 6, 7, 100], np.uint32)) == E_ARG                    # id past hx_num_rows
    assert call(o=np.array([0, 3, 2, 5, 8], np.uint64)) == E_ARG                                # decreasing
    assert call(o=np.array([1, 3, 3, 5, 8], np.uint64)) == E_ARG                                # offsets[0] != 0
    assert call(o=None) == E_ARG and call(cd=None) == E_ARG and call(cd=None, o=np.zeros(5, np.uint64)) == 0
    assert call(fq=1) == E_ARG and call(nq=5, o=np.array([0, 3, 3, 5, 8, 8], np.uint64)) == E_ARG
    assert call(i=False) == E_ARG and call(dd=False) == E_ARG and call(cc=False) == E_ARG
    assert call(nq=0, o=np.zeros(1, np.uint64)) == 0
    eb = engine(hx.BIT, 64, hx.OP_HAMMING, make(hx.BIT, 10, 64, rng), make(hx.BIT, 1, 64, rng))
    for op in FOPS:
        with pytest.raises(hx.HxError):
            eb.exact_rerank(op, [[1]], 1)
    e.set_timing(True)
    e.exact_search(hx.OP_L2, 5)
    e.exact_range(hx.OP_L2, 3.0)
    k7, k8 = e.kernel_stats(7), e.kernel_stats(8)
    e.kernel_stats(9, reset=True)
    e.exact_rerank(hx.OP_L2, (off, cand[:-1].tolist() + [0]), 10)
    e.exact_rerank(hx.OP_L2, [np.arange(100)] * 4, 5)
    st = e.kernel_stats(9)
    assert st["units"] == 8 + 400 and st["launches"] >= 4 and st["ms"] > 0
    assert e.kernel_stats(7) == k7 and e.kernel_stats(8) == k8
    e.close()
    eb.close()


@pytest.mark.gpu
def test_while_index_scan_in_flight():
    rng = np.random.default_rng(59)
    n, dim = 4000, 32
    rows, qs = rng.random((n, dim), dtype=np.float32), rng.random((16, dim), dtype=np.float32)
    e = hx.Engine(hx.F32, hx.L2SQ, dim, n)
    e.append(rows)
    e.set_queries(qs)
    ix = hx.Index(e, 8, 32)
    ix.insert(0, hx.draw_levels(n, 8, seed=9), batch=256)
    lists = [rng.integers(0, n, 500) for _ in range(16)]
    alone = ix.search(16, 40, 10)
    rr = e.exact_rerank(hx.OP_L2, lists, 10)
    ix.search_submit(0, 0, 16, 40, 10)
    during = e.exact_rerank(hx.OP_L2, lists, 10)
    waited = ix.search_wait(0)
    assert same(rr, during)
    assert all((a == b).all() for a, b in zip(alone, waited))
    ix.close()
    e.close()


# ---- 3. scan-only engines at 16000 dimensions ------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [hx.F32, hx.F16], ids=["vector", "halfvec"])
def test_wide_scan_only(dtype):
    rng = np.random.default_rng(61 + dtype)
    n, dim = 300, 16000
    rows, qs = make(dtype, n, dim, rng), make(dtype, 3, dim, rng)
    e = hx.Engine(dtype, hx.L2SQ, dim, n, scan_only=True)
    assert e.append(rows[:250]) == 0 and e.append(rows[250:]) == 250
    assert (e.read_rows(0, n) == rows).all()
    e.pop(1)
    assert e.num_rows == n - 1
    e.append(rows[-1:])
    e.set_queries(qs)
    L = hx.lib()
    h = ctypes.c_void_p()
    assert L.hx_index_create(e.h, 16, 64, ctypes.byref(h)) == E_STATE
    u32 = np.array([0, 1], np.uint32)
    P = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    out = np.empty(4, np.float32)
    assert L.hx_distances_batch(e.h, 1, P(np.array([hx.QUERY_SLOT], np.uint32)), P(np.array([0, 2], np.uint32)), P(u32), P(out)) == E_STATE
    assert L.hx_pairwise(e.h, P(u32), 2, P(out)) == E_STATE
    assert L.hx_rows_equal(e.h, 1, P(u32[:1]), P(u32[1:]), P(np.empty(1, np.uint8))) == E_STATE
    assert L.hx_pairwise_many(e.h, 1, P(np.array([0, 2], np.uint32)), P(np.array([2], np.uint16)), P(np.array([0], np.uint16)), P(u32),
                              P(np.zeros(1, np.uint64)), P(out)) == E_STATE
    # hx_distances: the support function in the canonical order
    ids = rng.integers(0, n, 50).astype(np.uint32)
    want = orc.distances_many(dtype, orc.L2SQ, dim, qs[0], rows[ids], order=orc.W64).astype(np.float32)
    assert (e.distances(qs[0], ids).view(np.uint32) == want.view(np.uint32)).all()
    norms = ref.self_ip(dtype, dim, rows)
    for op, k in ((hx.OP_L2, 1024), (hx.OP_COSINE, 10)):               # k = 1024: the exact scan's LDS tile beyond 64 KiB
        nm = norms if op == hx.OP_COSINE else None
        got = e.exact_search(op, k, nq=2)
        for qi in range(2):
            wi, wd = ref.topk(dtype, dim, op, qs[qi], rows, k, row_norms=nm)
            c = int(got[2][qi])
            assert c == len(wi) and got[0][qi, :c].tolist() == wi.tolist() and ref.same_bits(got[1][qi, :c], wd)
        lists = [rng.integers(0, n, 400), np.arange(n)]
        check(e, dtype, dim, op, rows, qs, lists, k, norms=nm)
        assert same(e.exact_rerank(op, [np.arange(n)] * 3, k), e.exact_search(op, k))
    vals = ref.values(dtype, dim, hx.OP_L2, qs[0], rows)
    r = float(np.median(vals))
    off, rid, rd = e.exact_range(hx.OP_L2, r, nq=1)
    want = np.nonzero(vals < r)[0]
    assert rid.tolist() == want.tolist() and ref.same_bits(rd, vals[want])
    nrm = e.normalize_rows(0, 4)
    assert np.allclose(nrm, np.sqrt(norms[:4]), rtol=1e-5)
    e.close()


# ---- 4. end to end: a halfvec expression index on a vector(3072) column, re-ranked at full precision ------------------------------------------
@pytest.mark.gpu
def test_halfvec_index_rerank_end_to_end():
    rng = np.random.default_rng(67)
    n, dim, nq, kp, k = 20000, 3072, 50, 40, 10
    centres = rng.random((64, dim), dtype=np.float32)
    rows = (centres[rng.integers(0, 64, n)] + 0.1 * rng.standard_normal((n, dim))).astype(np.float32)
    qs = (centres[rng.integers(0, 64, nq)] + 0.1 * rng.standard_normal((nq, dim))).astype(np.float32)
    vec = hx.Engine(hx.F32, hx.L2SQ, dim, n, scan_only=True)            # the table's vector(3072) column
    vec.append(rows)
    vec.set_queries(qs)
    half = hx.Engine(hx.F16, hx.L2SQ, dim, n)                           # the expression index's halfvec(3072) values
    assert half.append_halfvec_from(vec) == 0
    ix = hx.Index(half, 16, 64)
    ix.insert(0, hx.draw_levels(n, 16, seed=5), batch=256)
    half.set_queries_halfvec_from(vec)
    tids, _, _, cnt = ix.search(nq, 100, kp)                            # ORDER BY embedding::halfvec(3072) <-> $1::halfvec(3072) LIMIT 40
    assert (cnt == kp).all()
    lists = [tids[q].astype(np.int64) for q in range(nq)]               # heap TIDs are row ids here
    got = check(vec, hx.F32, dim, hx.OP_L2, rows, qs, lists, k)         # ORDER BY c.embedding <-> $1 LIMIT 10
    truth = vec.exact_search(hx.OP_L2, k)[0]
    for q in range(nq):
        t = set(truth[q].tolist())
        assert len(t & set(got[0][q].tolist())) >= len(t & set(tids[q, :k].tolist())), q
    ix.close()
    half.close()
    vec.close()
