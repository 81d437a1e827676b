"""hx_exact_search: the exact (filtered) k-NN scan -- the sequential-scan plan of `ORDER BY v <op> q LIMIT k` -- on the device, checked bit for bit
against the oracle composed in tests/exact_ref.py, within the north-star tolerance of the reference's own (sequential) sums, and against the
reference's known answers."""
import ctypes
import json
import os

import numpy as np
import pytest

import pgvector_rx_amd as hx
from oracle import orc
import exact_ref as ref

G = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "reference_known_answers.json")))
FOPS = [hx.OP_L2, hx.OP_NEG_IP, hx.OP_COSINE, hx.OP_L1]
BOPS = [hx.OP_HAMMING, hx.OP_JACCARD]
METRIC_OF = {hx.OP_L2: hx.L2SQ, hx.OP_NEG_IP: hx.NEG_IP, hx.OP_COSINE: hx.NEG_IP, hx.OP_L1: hx.L1, hx.OP_HAMMING: hx.HAMMING, hx.OP_JACCARD: hx.JACCARD}
NOT_FOUND = 0xFFFFFFFF


def make(dtype, n, dim, rng):
    if dtype == hx.F32:
        return rng.standard_normal((n, dim)).astype(np.float32)
    if dtype == hx.F16:
        return rng.standard_normal((n, dim)).astype(np.float16).view(np.uint16)
    if dtype == hx.BIT:
        return rng.integers(0, 256, (n, (dim + 7) // 8), dtype=np.uint8)
    sp = []
    for _ in range(n):
        nnz = int(rng.integers(0, 12))
        idx = np.sort(rng.choice(dim, nnz, replace=False))
        sp.append((idx, rng.standard_normal(nnz).astype(np.float32)))
    return hx.pack_sparse(dim, sp)


def check(e, dtype, dim, op, rows, queries, k, first_query=0, nq=None, first_row=0, n_rows=None, mask=None, norms=None, seq=True):
    """Runs the scan and compares every query's ids and distance bits with the composed reference; returns the scan's outputs."""
    nq = len(queries) - first_query if nq is None else nq
    n_rows = len(rows) - first_row if n_rows is None else n_rows
    ids, dist, cnt = e.exact_search(op, k, first_query=first_query, nq=nq, first_row=first_row, n_rows=n_rows, row_pass=mask)
    cand = np.arange(first_row, first_row + n_rows)
    if mask is not None:
        cand = cand[np.asarray(mask, bool)]
    for qi in range(nq):
        q = queries[first_query + qi]
        want_ids, want_d = ref.topk(dtype, dim, op, q, rows[cand], k, ids=cand, row_norms=None if norms is None else norms[cand])
        c = int(cnt[qi])
        assert c == len(want_ids) == min(k, len(cand)), (qi, c, len(want_ids))
        assert ids[qi, :c].tolist() == want_ids.tolist(), (op, qi)
        assert ref.same_bits(dist[qi, :c], want_d), (op, qi)
        assert (ids[qi, c:] == NOT_FOUND).all() and np.isnan(dist[qi, c:]).all()
        if seq and c:
            north_star(dtype, dim, op, q, rows[ids[qi, :c].astype(np.int64)], dist[qi, :c])
    return ids, dist, cnt


def north_star(dtype, dim, op, q, rows, got):
    """Within the tolerance of the reference's own sequential sums (tests/test_gpu_engine.py: check_tolerance)."""
    L = orc.lib()
    qa = orc.as_rows(dtype, q)
    if op in (hx.OP_HAMMING, hx.OP_JACCARD):
        want = orc.distances_many(dtype, METRIC_OF[op], dim, q, rows, order=orc.SEQ)
        assert (want == got).all()
        return
    if op == hx.OP_L2:
        want = np.array([L.orc_l2_distance(dtype, dim, orc._p(qa), orc._p(orc.as_rows(dtype, r))) for r in rows])
        ok = np.abs(got - want) <= 1e-5 * np.abs(want) + 1e-30
    elif op == hx.OP_COSINE:
        want = np.array([L.orc_cosine_distance(dtype, dim, orc._p(qa), orc._p(orc.as_rows(dtype, r))) for r in rows])
        ok = np.abs(got - want) <= 1e-5
    else:
        want = orc.distances_many(dtype, METRIC_OF[op], dim, q, rows, order=orc.SEQ)
        if op == hx.OP_NEG_IP and dtype != hx.SPARSE:
            qf = q.astype(np.float64) if dtype == hx.F32 else q.view(np.float16).astype(np.float64)
            rf = rows.astype(np.float64) if dtype == hx.F32 else rows.view(np.float16).astype(np.float64)
            scale = np.abs(rf * qf[None, :]).sum(1)
        else:
            scale = np.abs(want)
        ok = np.abs(got - want) <= 1e-5 * scale + 1e-30
    assert (ok | (np.isnan(got) & np.isnan(want))).all()


def engine(dtype, dim, op, rows, queries):
    e = hx.Engine(dtype, METRIC_OF[op] if dtype == hx.BIT else hx.L2SQ, dim, len(rows))
    e.append(rows)
    e.set_queries(queries)
    return e


# ---- 1. parity matrix -----------------------------------------------------------------------------------------------------------------------
CASES = [(hx.F32, d) for d in (1, 3, 100, 768, 1536, 2000)] + [(hx.F16, 10), (hx.F16, 4000), (hx.BIT, 8), (hx.BIT, 1024), (hx.SPARSE, 100)]


@pytest.mark.gpu
@pytest.mark.parametrize("dtype,dim", CASES, ids=lambda v: str(v))
def test_parity_matrix(dtype, dim):
    rng = np.random.default_rng(7 + dim + 10 * dtype)
    n = 1500 if dim <= 1536 else 700
    rows, qs = make(dtype, n, dim, rng), make(dtype, 64, dim, rng)
    ops = BOPS if dtype == hx.BIT else FOPS
    norms = None
    for op in ops:
        e = engine(dtype, dim, op, rows, qs)            # the handle's metric does not restrict the operator (an L2 index, a <=> seq scan)
        if op == hx.OP_COSINE and dtype != hx.SPARSE and norms is None:
            norms = ref.self_ip(dtype, dim, rows)
        nm = norms if op == hx.OP_COSINE else None
        check(e, dtype, dim, op, rows, qs, 10, nq=1, norms=nm)                   # one query: many slices, Q = 1
        check(e, dtype, dim, op, rows, qs, 100, first_query=3, nq=7, norms=nm)   # Q = 4, a partial tile
        check(e, dtype, dim, op, rows, qs, 1, nq=64, norms=nm, seq=False)         # Q = 16
        if dim <= 768:
            check(e, dtype, dim, op, rows, qs, 1024, nq=2, norms=nm, seq=False)
        e.close()


@pytest.mark.gpu
def test_one_slice_and_scratch_blocks(monkeypatch):
    """Fewer rows than one slice's minimum; then the query-block regime (scratch smaller than all queries' buffers) gives the same lists."""
    rng = np.random.default_rng(3)
    rows, qs = make(hx.F32, 40, 16, rng), make(hx.F32, 64, 16, rng)
    e = engine(hx.F32, 16, hx.OP_L2, rows, qs)
    check(e, hx.F32, 16, hx.OP_L2, rows, qs, 100, nq=64)
    rows, qs = make(hx.F32, 5000, 64, rng), make(hx.F32, 64, 64, rng)
    e = engine(hx.F32, 64, hx.OP_L2, rows, qs)
    full = e.exact_search(hx.OP_L2, 100, nq=64)
    monkeypatch.setenv("HX_EXACT_SCRATCH", str(1 << 20))
    got = check(e, hx.F32, 64, hx.OP_L2, rows, qs, 100, nq=64, seq=False)
    assert all((a.view(np.uint8) == b.view(np.uint8)).all() for a, b in zip(full, got))


# ---- 2. ties and special values -------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_ties_and_special_values():
    rng = np.random.default_rng(11)
    # 64 copies of one row among others: equal distances come back by row id
    base = make(hx.F32, 300, 24, rng)
    rows = np.concatenate([base[:100], np.repeat(base[100:101], 64, 0), base[101:]])
    qs = make(hx.F32, 4, 24, rng)
    qs[1] = rows[120]
    e = engine(hx.F32, 24, hx.OP_L2, rows, qs)
    ids, d, _ = check(e, hx.F32, 24, hx.OP_L2, rows, qs, 100)
    assert ids[1, :64].tolist() == list(range(100, 164)) and (d[1, :64] == 0).all()
    # bit(1024) Hamming at k = 1024: ties everywhere
    rows, qs = make(hx.BIT, 3000, 1024, rng), make(hx.BIT, 2, 1024, rng)
    e = engine(hx.BIT, 1024, hx.OP_HAMMING, rows, qs)
    check(e, hx.BIT, 1024, hx.OP_HAMMING, rows, qs, 1024)
    # <=> with a zero query and zero rows: NaN, last, by id
    rows = make(hx.F32, 200, 8, rng)
    rows[[5, 50, 77]] = 0
    qs = np.concatenate([np.zeros((1, 8), np.float32), make(hx.F32, 1, 8, rng)])
    e = engine(hx.F32, 8, hx.OP_COSINE, rows, qs)
    ids, d, _ = check(e, hx.F32, 8, hx.OP_COSINE, rows, qs, 200)
    assert np.isnan(d[0]).all() and ids[0].tolist() == list(range(200))
    assert ids[1, -3:].tolist() == [5, 50, 77] and np.isnan(d[1, -3:]).all() and not np.isnan(d[1, :-3]).any()
    # <#> with a zero product: -0.0 comes back with its sign, and equals +0.0 in the order
    rows = make(hx.F32, 100, 4, rng)
    rows[::3, 0] = 0
    qs = np.array([[1, 0, 0, 0]], np.float32)
    e = engine(hx.F32, 4, hx.OP_NEG_IP, rows, qs)
    ids, d, cnt = check(e, hx.F32, 4, hx.OP_NEG_IP, rows, qs, 100)
    z = d[0] == 0
    assert z.sum() == 34 and (np.signbit(d[0][z])).all() and ids[0][z].tolist() == list(range(0, 100, 3))
    # magnitude 1e30: l2sq overflows to +inf (before NaN), ip becomes inf - inf = NaN
    rows = (rng.choice([-1.0, 1.0], (50, 8)) * 1e30).astype(np.float32)
    rows[:10] = rng.standard_normal((10, 8)).astype(np.float32)
    qs = (rng.choice([-1.0, 1.0], (1, 8)) * 1e30).astype(np.float32)
    for op in FOPS:
        e = engine(hx.F32, 8, op, rows, qs)
        ids, d, _ = check(e, hx.F32, 8, op, rows, qs, 50, seq=False)
        if op == hx.OP_L2:
            assert np.isinf(d[0, 10:]).all()
        if op == hx.OP_NEG_IP:
            assert np.isnan(d[0]).any()


# ---- 3. filter and range --------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_filter_and_range():
    rng = np.random.default_rng(17)
    n = 10000                                         # tests/t/017_hnsw_filtering.pl: c = i % 50, WHERE c = 7 ORDER BY v <-> q LIMIT 20
    rows, qs = rng.random((n, 3), dtype=np.float32), rng.random((8, 3), dtype=np.float32)
    e = engine(hx.F32, 3, hx.OP_L2, rows, qs)
    e.set_timing(True)
    e.kernel_stats(7, reset=True)
    mask = (np.arange(n) % 50) == 7
    ids, _, _ = check(e, hx.F32, 3, hx.OP_L2, rows, qs, 20, mask=mask)
    assert (ids % 50 == 7).all()
    st = e.kernel_stats(7, reset=True)
    assert st["units"] == mask.sum() * 8 and st["launches"] >= 3 and st["ms"] > 0
    few = np.zeros(n, bool)
    few[[3, 999, 5000, 9998, 9999]] = True                                       # fewer than k pass: counts and padding
    _, _, cnt = check(e, hx.F32, 3, hx.OP_L2, rows, qs, 20, mask=few)
    assert (cnt == 5).all()
    ids, d, cnt = e.exact_search(hx.OP_L2, 20, row_pass=np.zeros(n, bool))        # empty filter
    assert (cnt == 0).all() and (ids == NOT_FOUND).all() and np.isnan(d).all()
    check(e, hx.F32, 3, hx.OP_COSINE, rows, qs, 20, first_row=1234, n_rows=4321)  # a sub-range
    sub = rng.random(4321) < 0.3
    check(e, hx.F32, 3, hx.OP_L1, rows, qs, 20, first_row=1234, n_rows=4321, mask=sub)
    words = np.packbits(np.concatenate([sub, np.zeros(4352 - 4321, bool)]), bitorder="little").view(np.uint64)
    a = e.exact_search(hx.OP_L1, 20, first_row=1234, n_rows=4321, row_pass=sub)
    b = e.exact_search(hx.OP_L1, 20, first_row=1234, n_rows=4321, row_pass=words, packed=True)   # the packed form
    c = e.exact_search(hx.OP_L1, 20, first_row=1234, n_rows=4321, row_pass=sub.astype(np.uint64))  # a uint64 0/1 mask is a mask
    assert all((x == y).all() for x, y in zip(a[:1] + a[2:], c[:1] + c[2:]))
    d_ = e.exact_search(hx.OP_L1, 20, first_query=5)                             # nq defaults to the slots after first_query
    assert d_[0].shape == (3, 20) and (d_[0] == e.exact_search(hx.OP_L1, 20, first_query=5, nq=3)[0]).all()
    assert all((x == y).all() for x, y in zip(a[:1] + a[2:], b[:1] + b[2:]))


# ---- 4. argument errors ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_argument_errors():
    rng = np.random.default_rng(5)
    rows, qs = make(hx.F32, 100, 8, rng), make(hx.F32, 4, 8, rng)
    e = engine(hx.F32, 8, hx.OP_L2, rows, qs)
    L = hx.lib()
    ids, d, c = np.empty(4 * 1024, np.uint32), np.empty(4 * 1024, np.float64), np.empty(4, np.uint32)
    P = lambda a: a.ctypes.data_as(ctypes.c_void_p)

    def call(op=hx.OP_L2, fq=0, nq=4, fr=0, nr=100, k=10, outs=True):
        return L.hx_exact_search(e.h, op, fq, nq, fr, nr, None, k, P(ids) if outs else None, P(d), P(c))
    assert call() == 0
    assert call(op=hx.OP_HAMMING) == -1 and call(op=hx.OP_JACCARD) == -1 and call(op=6) == -1 and call(op=-1) == -1
    assert call(k=0) == -1 and call(k=1025) == -1 and call(k=1024) == 0
    assert call(fr=50, nr=51) == -1 and call(fr=101, nr=0) == -1 and call(fr=2 ** 32, nr=0) == -1
    assert call(fq=1, nq=4) == -1 and call(nq=5) == -1
    assert call(outs=False) == -1
    eb = engine(hx.BIT, 64, hx.OP_HAMMING, make(hx.BIT, 10, 64, rng), make(hx.BIT, 1, 64, rng))
    for op in FOPS:
        with pytest.raises(hx.HxError):
            eb.exact_search(op, 5)


# ---- 5. reference known answers -------------------------------------------------------------------------------------------------------------
TYPE = {"vector": hx.F32, "halfvec": hx.F16, "bit": hx.BIT, "sparsevec": hx.SPARSE}
OP = {"l2": hx.OP_L2, "ip": hx.OP_NEG_IP, "cosine": hx.OP_COSINE, "l1": hx.OP_L1, "hamming": hx.OP_HAMMING, "jaccard": hx.OP_JACCARD}


def enc(tname, v):
    if tname == "vector":
        return np.asarray(v, np.float32), len(v)
    if tname == "halfvec":
        return np.array([orc.lib().orc_f32_to_half(float(x)) for x in v], np.uint16), len(v)
    if tname == "sparsevec":
        return orc.sparse_from_dense(v), len(v)
    return orc.pack_bits(v), len(v)


@pytest.mark.gpu
@pytest.mark.parametrize("case", G["regress_order"], ids=lambda c: c["ref"].split("/")[-1])
def test_regress_orderings_exact(case):
    """The pg_regress expected orderings through the exact scan.  Under <=> the zero row, which the index skips, comes back last with NaN."""
    dt, op = TYPE[case["type"]], OP[case["metric"]]
    enc_rows = [enc(case["type"], r)[0] for r in case["rows"]]
    q, dim = enc(case["type"], case["query"])
    rows = np.stack(enc_rows)
    e = engine(dt, dim, op, rows, q[None, :])
    ids, d, cnt = e.exact_search(op, 10)
    got = [case["rows"][i] for i in ids[0, :cnt[0]]]
    zero = [r for r in case["rows"] if not any(r if not isinstance(r, str) else [ch == "1" for ch in r])]
    if op == hx.OP_COSINE and zero:
        assert got[:len(case["expect"])] == case["expect"] and got[len(case["expect"]):] == zero and np.isnan(d[0, cnt[0] - 1])
    else:
        assert got[:len(case["expect"])] == case["expect"]


@pytest.mark.gpu
@pytest.mark.parametrize("case", [c for c in G["distance"] if c["fn"] not in ("vector_norm", "inner_product")], ids=lambda c: c["fn"] + "@" + c["ref"].split("/")[-1])
def test_distance_known_answers_exact(case):
    fn = {"l2_distance": hx.OP_L2, "negative_inner_product": hx.OP_NEG_IP, "cosine_distance": hx.OP_COSINE, "l1_distance": hx.OP_L1,
          "hamming_distance": hx.OP_HAMMING, "jaccard_distance": hx.OP_JACCARD}[case["fn"]]
    a, dim = enc(case["type"], case["a"])
    b, _ = enc(case["type"], case["b"])
    e = engine(TYPE[case["type"]], dim, fn, a[None, :], b[None, :])
    _, d, cnt = e.exact_search(fn, 1)
    assert cnt[0] == 1
    want = case["expect"]
    assert (np.isnan(d[0, 0]) and want is None) or abs(d[0, 0] - want) < case["tol"], (case, d[0, 0])


# ---- 6. the reference's recall procedures, with the exact scan as ground truth ----------------------------------------------------------
@pytest.mark.gpu
def test_gate_012_with_exact_ground_truth():
    gate = G["recall_gates"][0]
    n, dim, k, nq = gate["rows"], gate["dim"], gate["k"], gate["queries"]
    rng = np.random.default_rng(12)
    rows = (rng.random((n, dim)) * rng.random((n, dim))).astype(np.float32)      # random() * random() per component (012:11)
    qs = rng.random((nq, dim)).astype(np.float32)
    levels = hx.draw_levels(n, gate["m"], seed=12)
    for name, op in (("l2", hx.OP_L2), ("ip", hx.OP_NEG_IP), ("cosine", hx.OP_COSINE), ("l1", hx.OP_L1)):
        metric = METRIC_OF[op]
        e = hx.Engine(hx.F32, metric, dim, n)
        e.append(rows)
        e.set_queries(qs)
        ids, d, _ = e.exact_search(op, 100)                 # 012:79-84: the expected rows come from a plain ORDER BY before the index exists
        if op == hx.OP_COSINE:
            e.normalize_rows(0, n)
            e.set_queries(qs, normalize=True)
        ix = hx.Index(e, gate["m"], gate["ef_construction"])
        ix.insert(0, levels, batch=128)
        tids, _, _, cnt = ix.search(nq, gate["ef_search"], k)
        want = [set(ids[q][d[q] <= d[q, k - 1]].tolist()) for q in range(nq)]   # ties with the k-th distance count (020:60-66)
        hit = sum(len(set(tids[q, :cnt[q]].tolist()) & want[q]) for q in range(nq))
        assert hit / (nq * k) >= gate["min_recall"][name], name
        ix.close()
        e.close()


@pytest.mark.gpu
def test_gate_044_with_exact_ground_truth():
    """tests/t/044_hnsw_iterative_scan_recall.pl:111-112 with the exact scan as its ground truth: for each metric the expected rows come from
    hx_exact_search with the filter before the index exists (044:97-107, enable_indexscan = off), tie-inclusive -- every passing row whose distance
    is <= the largest of the top `limit` (044:96-104) --; then the index is built and both iterative modes must reach the gate's recall."""
    gate = G["iterative_recall_gates"][0]
    n, dim, limit, nq = gate["rows"], gate["dim"], gate["limit"], gate["queries"]
    rng = np.random.default_rng(44)
    rows, qs = rng.random((n, dim)).astype(np.float32), rng.random((nq, dim)).astype(np.float32)
    r64 = rows.astype(np.float64)
    levels = hx.draw_levels(n, gate["m"], seed=44)
    for metric in gate["metrics"]:
        cosine = metric == "cosine"
        op = hx.OP_COSINE if cosine else hx.OP_L2
        e = hx.Engine(hx.F32, hx.NEG_IP if cosine else hx.L2SQ, dim, n)
        e.append(rows)
        e.set_queries(qs)
        expected = {}
        for c in gate["filter_mod"]:
            mask = (np.arange(1, n + 1) % c) == 0                              # i = 1..rows (044:66), WHERE i % c = 0
            _, top, _ = e.exact_search(op, limit, row_pass=mask)
            ids, d, cnt = e.exact_search(op, 1024, row_pass=mask)             # every passing row (<= 1000)
            assert (cnt == mask.sum()).all()
            expected[c] = [set((ids[q, :cnt[q]][d[q, :cnt[q]] <= top[q].max()] + 1).tolist()) for q in range(nq)]
            if not cosine:                                                      # the same sets as the f64 restatement of the SQL
                for q in range(nq):
                    dist = np.sqrt(((r64 - qs[q].astype(np.float64)) ** 2).sum(1))
                    t64 = np.sort(dist[mask])[limit - 1]
                    assert expected[c][q] == set((np.nonzero(mask & (dist <= t64))[0] + 1).tolist()), (c, q)
        if cosine:
            assert (e.normalize_rows(0, n) > 0).all()
        ix = hx.Index(e, gate["m"], gate["ef_construction"])
        ix.insert(0, levels, tids=np.arange(1, n + 1), batch=512)             # heap TID = i
        e.set_queries(qs, normalize=cosine)
        for c in gate["filter_mod"]:
            passes = (np.arange(n + 1) % c == 0).astype(np.uint8)               # indexed by TID
            for mode in gate["modes"]:
                tids, _, rc = ix.search_iterative(nq, gate["ef_search"], 2 if mode == "strict_order" else 1, 20000, limit, passes)
                hit = sum(t in expected[c][q] for q in range(nq) for t in tids[q, :rc[q]].tolist())
                assert hit / (nq * limit) >= gate["min_recall"], (metric, c, mode, hit)
        ix.close()
        e.close()


# ---- 7. at scale ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_at_scale_200k_768():
    rng = np.random.default_rng(200)
    n, dim = 200_000, 768
    rows, qs = rng.standard_normal((n, dim), dtype=np.float32), rng.standard_normal((4, dim), dtype=np.float32)
    e = engine(hx.F32, dim, hx.OP_L2, rows, qs)
    check(e, hx.F32, dim, hx.OP_L2, rows, qs, 100, seq=False)
