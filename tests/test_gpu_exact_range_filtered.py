"""hx_exact_range_filtered: exact range scans with a WHERE filter per query in one call.  The oracle is the definition: offsets, ids and distance
bits equal, byte for byte, the CSR concatenation of one hx_exact_range call per query with that query's filter and radius (on the same engine); a
handful of queries per case are also compared with the CPU model composed in tests/exact_ref.py (values + order + the float8 predicate).
Radii come per query from exact_search on that query's filter: the value of its 1st, 10th or 100th nearest passing row, so the hit counts are
known -- `<` the nearest row's value: none; `>=` it: every passing row; `<=` the p-th: at least p."""
import ctypes

import numpy as np
import pytest

import pgvector_rx_amd as hx
import exact_ref as ref
from test_gpu_exact_filtered import BOPS, FOPS, engine, interleaved, make
from test_gpu_range import CMPS, E_ARG, E_NOMEM, expected

PICKS = (0, 9, 99)


def same(a, b):
    return all(x.shape == y.shape and (x.view(np.uint8) == y.view(np.uint8)).all() for x, y in zip(a, b))


def radii_of(e, op, masks, fo, first_query=0, first_row=0, n_rows=None):
    """Per query the value of its PICKS[i % 3]-th nearest passing row (its last one if it has fewer; 0.0 if none) -> (radii, ranks, passing rows)"""
    _, d, cnt = e.exact_search_filtered(op, 100, masks, fo, first_query=first_query, nq=len(fo), first_row=first_row, n_rows=n_rows)
    rank = np.array([min(PICKS[i % 3], max(int(c), 1) - 1) for i, c in enumerate(cnt)])
    r = np.array([d[i, rank[i]] if cnt[i] else 0.0 for i in range(len(fo))])
    n = (e.num_rows - first_row) if n_rows is None else n_rows
    n_pass = np.array([n if f < 0 else int(np.asarray(masks[f], bool).sum()) for f in fo])
    return r, rank, n_pass


def one_by_one(e, op, radii, masks, fo, cmp=hx.CMP_LT, ordered=False, first_query=0, first_row=0, n_rows=None, count_only=False):
    """The definition: one hx_exact_range call per query with that query's filter and radius, concatenated."""
    out = [e.exact_range(op, radii[i], cmp=cmp, first_query=first_query + i, nq=1, first_row=first_row, n_rows=n_rows,
                         row_pass=None if f < 0 else masks[f], ordered=ordered, count_only=count_only) for i, f in enumerate(fo)]
    off = np.zeros(len(fo) + 1, np.uint64)
    off[1:] = np.cumsum([int(o[0][1]) for o in out], dtype=np.uint64)
    return off, np.concatenate([o[1] for o in out]), np.concatenate([o[2] for o in out])


def check(e, op, radii, masks, fo, cmp=hx.CMP_LT, ordered=False, first_query=0, first_row=0, n_rows=None, cpu=None, cache=None):
    """Runs the grouped call and requires the bytes of the per-query calls.  cpu = (dtype, dim, rows, queries, picks, norms): also the CPU model
    for the queries in `picks`; cache: a dict that keeps their reference values from one call to the next (same rows, queries and filters)."""
    radii = np.broadcast_to(np.asarray(radii, np.float64), (len(fo),))
    got = e.exact_range_filtered(op, radii, masks, fo, cmp=cmp, first_query=first_query, nq=len(fo), first_row=first_row, n_rows=n_rows, ordered=ordered)
    want = one_by_one(e, op, radii, masks, fo, cmp, ordered, first_query, first_row, n_rows)
    for j, name in enumerate(("offsets", "ids", "dist")):
        assert got[j].shape == want[j].shape and (got[j].view(np.uint8) == want[j].view(np.uint8)).all(), (op, cmp, ordered, name)
    if cpu:
        dtype, dim, rows, queries, picks, norms = cpu
        n = (len(rows) - first_row) if n_rows is None else n_rows
        for i in picks:
            cand = np.arange(first_row, first_row + n)
            if fo[i] >= 0:
                cand = cand[np.asarray(masks[fo[i]], bool)]
            key = (op, first_query + i, int(fo[i]), first_row, n)
            if cache is None or key not in cache:
                vals = ref.values(dtype, dim, op, queries[first_query + i], rows[cand], None if norms is None else norms[cand])
                if cache is not None:
                    cache[key] = vals
            else:
                vals = cache[key]
            w_ids, w_v = expected(vals, cand, radii[i], cmp, ordered)
            a, b = int(got[0][i]), int(got[0][i + 1])
            assert got[1][a:b].tolist() == w_ids.tolist() and ref.same_bits(got[2][a:b], w_v), (op, cmp, ordered, i)
    return got


# ---- 1. parity matrix -----------------------------------------------------------------------------------------------------------------------
CASES = [(hx.F32, d) for d in (3, 100, 768, 2000)] + [(hx.F16, 10), (hx.F16, 4000), (hx.BIT, 8), (hx.BIT, 1024), (hx.SPARSE, 100)]


@pytest.mark.gpu
@pytest.mark.parametrize("dtype,dim", CASES, ids=lambda v: str(v))
def test_parity_matrix(dtype, dim):
    """26 queries over 4 filters in groups of 1, 3, 5 and 17 (tiles of 16 + 1, 4 + 1, a partial tile of 4 and a tile of 1) and 3 unfiltered ones."""
    rng = np.random.default_rng(170 + dim + 10 * dtype)
    n = 1500 if dim <= 1536 else 700
    fo = interleaved([1, 3, 5, 17], 3, rng)
    rows, qs = make(dtype, n, dim, rng), make(dtype, len(fo), dim, rng)
    masks = [rng.random(n) < p for p in (0.5, 0.1, 0.3, 0.2)]
    picks = [int(np.nonzero(fo == f)[0][-1]) for f in (-1, 0, 3)]
    norms = None
    for op in (BOPS if dtype == hx.BIT else FOPS):
        e = engine(dtype, dim, op, rows, qs)
        if op == hx.OP_COSINE and dtype != hx.SPARSE and norms is None:
            norms = ref.self_ip(dtype, dim, rows)
        radii, rank, n_pass = radii_of(e, op, masks, fo)
        finite, cache = ~np.isnan(radii), {}
        cpu = (dtype, dim, rows, qs, picks, norms if op == hx.OP_COSINE else None)
        for cmp in CMPS:
            for ordered in (False, True):
                off, _, _ = check(e, op, radii, masks, fo, cmp, ordered, cpu=cpu, cache=cache)
                cnt = np.diff(off).astype(np.int64)
                if cmp == hx.CMP_LT:
                    assert (cnt[finite] <= rank[finite]).all() and (cnt[finite & (rank == 0)] == 0).all()    # nothing below the nearest row
                if cmp == hx.CMP_LE:
                    assert (cnt[finite] >= rank[finite] + 1).all()
                if cmp == hx.CMP_GE:
                    assert (cnt[rank == 0] == n_pass[rank == 0]).all()                                        # every passing row
        e.close()


# ---- 2. modes -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_modes():
    rng = np.random.default_rng(12)
    n, dim = 1500, 40
    fo = interleaved([2, 4, 7], 2, rng)
    rows, qs = make(hx.F32, n, dim, rng), make(hx.F32, len(fo), dim, rng)
    masks = [rng.random(n) < p for p in (0.5, 0.2, 0.7)]
    e = engine(hx.F32, dim, hx.OP_L2, rows, qs)
    radii, _, _ = radii_of(e, hx.OP_L2, masks, fo)
    L, P = hx.lib(), lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)
    words = [np.packbits(m, bitorder="little") for m in masks]
    words = [np.concatenate([w, np.zeros(-len(w) % 8, np.uint8)]).view(np.uint64) for w in words]
    ptrs = (ctypes.c_void_p * 3)(*[w.ctypes.data for w in words])
    r, of = np.ascontiguousarray(radii), np.ascontiguousarray(fo, np.int32)

    def call(order, cap, ids, dist):
        off, total = np.full(len(fo) + 1, 7, np.uint64), ctypes.c_uint64(7)
        rc = L.hx_exact_range_filtered(e.h, hx.OP_L2, hx.CMP_LE, P(r), 0, len(fo), 0, n, 3, ptrs, P(of), order, cap, P(off), P(ids), P(dist), ctypes.byref(total))
        return rc, off, total.value

    for ordered in (False, True):
        order = hx.RANGE_BY_DISTANCE if ordered else hx.RANGE_BY_ROW
        w_off, w_ids, w_d = one_by_one(e, hx.OP_L2, radii, masks, fo, hx.CMP_LE, ordered)
        t = int(w_off[-1])
        assert t > len(fo)
        rc, off, total = call(order, 0, None, None)                                  # count only
        assert rc == 0 and total == t and (off == w_off).all()
        assert same(e.exact_range_filtered(hx.OP_L2, radii, masks, fo, cmp=hx.CMP_LE, ordered=ordered, count_only=True)[:1], (w_off,))
        ids = np.full(t + 1, 7, np.uint32)
        rc, off, total = call(order, t + 1, ids, None)                               # ids without values
        assert rc == 0 and total == t and (off == w_off).all() and (ids[:t] == w_ids).all() and ids[t] == 7
        ids, d = np.full(t + 1, 7, np.uint32), np.full(t + 1, 7.0)
        rc, off, total = call(order, t, ids, d)                                      # cap equal to the total
        assert rc == 0 and total == t and same((off, ids[:t], d[:t]), (w_off, w_ids, w_d)) and ids[t] == 7 and d[t] == 7.0
        rc, off, total = call(order, t - 1, ids, d)                                  # one below: the true offsets and total
        assert rc == E_NOMEM and total == t and (off == w_off).all() and b"capacity exceeded" in L.hx_last_error(e.h)
        with pytest.raises(hx.HxError):
            e.exact_range_filtered(hx.OP_L2, radii, masks, fo, cmp=hx.CMP_LE, ordered=ordered, cap=t - 1)
        assert same(e.exact_range_filtered(hx.OP_L2, radii, masks, fo, cmp=hx.CMP_LE, ordered=ordered, cap=t), (w_off, w_ids, w_d))
    # cap=None: more hits than the default capacity, so the binding calls twice
    got = e.exact_range_filtered(hx.OP_L2, np.inf, masks, fo, cmp=hx.CMP_LE)
    want = one_by_one(e, hx.OP_L2, np.full(len(fo), np.inf), masks, fo, hx.CMP_LE)
    assert same(got, want) and len(got[1]) < (1 << 16)
    big = engine(hx.F32, 4, hx.OP_L2, make(hx.F32, 9000, 4, rng), make(hx.F32, 10, 4, rng))
    bm, bfo = [np.ones(9000, bool), np.arange(9000) % 2 == 0], np.arange(10) % 2
    got = big.exact_range_filtered(hx.OP_L2, np.inf, bm, bfo)
    assert len(got[1]) == 5 * 9000 + 5 * 4500 > (1 << 16) and same(got, one_by_one(big, hx.OP_L2, np.full(10, np.inf), bm, bfo))
    big.close()
    e.close()


# ---- 3. filter edge cases -------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("dim", [16, 768])
def test_filter_edge_cases(dim):
    rng = np.random.default_rng(300 + dim)
    n = 1003                                              # not a multiple of 64
    rows, qs = make(hx.F32, n + 40, dim, rng), make(hx.F32, 14, dim, rng)
    e = engine(hx.F32, dim, hx.OP_L2, rows, qs)
    empty, one, few, ones = np.zeros(n, bool), np.zeros(n, bool), np.zeros(n, bool), np.ones(n, bool)
    one[777] = True
    few[[0, 63, 64, 500, 1002]] = True
    a, b = rng.random(n) < 0.4, rng.random(n) < 0.4        # overlapping
    masks = [empty, one, few, ones, None, a, b]           # filter 4: referenced by no query, a NULL pointer
    fo = np.array([0, 1, 2, 3, 5, 6, -1, 0, 2, 5, 6, 3], np.int32)
    cpu = (hx.F32, dim, rows, qs, [1, 2, 3, 4, 6], None)
    radii, _, _ = radii_of(e, hx.OP_L2, masks, fo, 2, 17, n)
    cache = {}
    for cmp in CMPS:
        for ordered in (False, True):
            off, ids, _ = check(e, hx.OP_L2, radii, masks, fo, cmp, ordered, first_query=2, first_row=17, n_rows=n, cpu=cpu, cache=cache)
            assert off[1] == off[0] and off[8] == off[7]                                     # the empty filter
    off, ids, _ = check(e, hx.OP_L2, np.inf, masks, fo, hx.CMP_LT, False, first_query=2, first_row=17, n_rows=n)
    assert np.diff(off).tolist() == [0, 1, 5, n, int(a.sum()), int(b.sum()), n, 0, 5, int(a.sum()), int(b.sum()), n]
    assert ids[0] == 17 + 777 and ids[1:6].tolist() == [17, 80, 81, 517, 1019]
    # packed words with garbage bits past n_rows in the last word: ignored
    words = []
    for m in masks:
        if m is None:
            words.append(None)
            continue
        bits = np.ones(((n + 63) // 64) * 64, np.uint8)
        bits[:n] = m
        words.append(np.packbits(bits, bitorder="little").view(np.uint64))
    got = e.exact_range_filtered(hx.OP_L2, radii, words, fo, cmp=hx.CMP_GE, first_query=2, nq=len(fo), first_row=17, n_rows=n, packed=True)
    assert same(got, one_by_one(e, hx.OP_L2, radii, masks, fo, hx.CMP_GE, False, 2, 17, n))
    # every query's filter is empty, beside unreferenced ones: answered without a scan
    e.set_timing(True)
    e.kernel_stats(8, reset=True)
    off, ids, d = e.exact_range_filtered(hx.OP_L2, np.inf, [empty, None, np.zeros(n, bool)], [0, 2, 0], nq=3, n_rows=n, cmp=hx.CMP_LE)
    assert (off == 0).all() and len(ids) == 0 and len(d) == 0 and e.kernel_stats(8)["launches"] == 0
    e.close()


# ---- 4. slices ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_slices_of_very_unequal_groups():
    """One group whose list is shorter than one round beside one that spans many slices; 5 rows against 4000."""
    rng = np.random.default_rng(431)
    n = 5000
    rows, qs = make(hx.F32, n, 64, rng), make(hx.F32, 12, 64, rng)
    e = engine(hx.F32, 64, hx.OP_L2, rows, qs)
    tiny, big, mid = np.zeros(n, bool), np.zeros(n, bool), rng.random(n) < 0.2
    tiny[[4, 1000, 2500, 4001, 4999]] = True
    big[rng.permutation(n)[:4000]] = True
    fo = np.array([0, 1, 2, 1, 0, -1, 1, 1, 2, 1, 0, 1], np.int32)
    radii, _, _ = radii_of(e, hx.OP_L2, [tiny, big, mid], fo)
    cache = {}
    for cmp in (hx.CMP_LE, hx.CMP_GT):
        for ordered in (False, True):
            check(e, hx.OP_L2, radii, [tiny, big, mid], fo, cmp, ordered, cpu=(hx.F32, 64, rows, qs, [0, 1, 2, 5], None), cache=cache)
    check(e, hx.OP_L2, radii[:2], [tiny, big], np.array([0, 1], np.int32), hx.CMP_GE)
    e.close()


# ---- 5. windows, overflow and blocks --------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_windows_overflow_and_query_blocks(monkeypatch):
    """Small scratch budgets: segments overflow their staging, the output goes through several windows and the queries through several blocks;
    the bytes stay those of the default budget."""
    rng = np.random.default_rng(541)
    n = 3000
    fo = interleaved([20, 19, 14, 5], 6, rng)
    assert len(fo) == 64
    rows, qs = make(hx.F32, n, 64, rng), make(hx.F32, 64, 64, rng)
    e = engine(hx.F32, 64, hx.OP_L2, rows, qs)
    masks = [rng.random(n) < p for p in (0.6, 0.3, 0.9, 0.05)]
    _, _, d_all = e.exact_range(hx.OP_L2, np.inf, cmp=hx.CMP_LE, ordered=True)
    radii = d_all.reshape(64, n)[:, n // 2].copy()                                   # about half of the passing rows
    e.set_timing(True)
    full, cache = {}, {}
    for ordered in (False, True):
        full[ordered] = check(e, hx.OP_L2, radii, masks, fo, hx.CMP_LT, ordered, cpu=(hx.F32, 64, rows, qs, [0, 1, 2], None), cache=cache)
    hits = np.diff(full[False][0]).astype(np.int64)
    assert 0.3 * n * 64 * 0.5 < hits.sum() and hits.max() > 1000
    e.kernel_stats(8, reset=True)
    e.exact_range_filtered(hx.OP_L2, radii, masks, fo)
    base_launches = e.kernel_stats(8, reset=True)["launches"]
    assert base_launches <= 6                                                        # one compaction, at most three scans, a gather, the values
    counts = e.exact_range_filtered(hx.OP_L2, radii, masks, fo, count_only=True)[0]
    for budget, orders in ((64 << 10, (False,)), (256 << 10, (False, True)), (1 << 20, (False, True))):
        monkeypatch.setenv("HX_RANGE_SCRATCH", str(budget))
        for ordered in orders:
            e.kernel_stats(8, reset=True)
            got = e.exact_range_filtered(hx.OP_L2, radii, masks, fo, ordered=ordered)
            assert same(got, full[ordered]), (budget, ordered)
            assert e.kernel_stats(8)["launches"] > base_launches + 2, budget         # more windows or blocks, and re-scans
        assert same(e.exact_range_filtered(hx.OP_L2, radii, masks, fo, count_only=True)[:1], (counts,))
    # by distance, `< inf`: the largest queries (3000 hits x 24 B) cannot fit the window of a 64 KiB budget: HX_E_NOMEM with the counts filled
    monkeypatch.setenv("HX_RANGE_SCRATCH", str(64 << 10))
    r = np.full(64, np.inf)
    counts = e.exact_range_filtered(hx.OP_L2, r, masks, fo, count_only=True)[0]
    assert same((counts,), one_by_one(e, hx.OP_L2, r, masks, fo, count_only=True)[:1])
    L, P = hx.lib(), lambda a: a.ctypes.data_as(ctypes.c_void_p)
    words = [np.packbits(m, bitorder="little") for m in masks]
    words = [np.concatenate([w, np.zeros(-len(w) % 8, np.uint8)]).view(np.uint64) for w in words]
    ptrs = (ctypes.c_void_p * 4)(*[w.ctypes.data for w in words])
    t = int(counts[-1])
    off, ids, d, total = np.zeros(65, np.uint64), np.empty(t, np.uint32), np.empty(t), ctypes.c_uint64()
    of = np.ascontiguousarray(fo, np.int32)
    rc = L.hx_exact_range_filtered(e.h, hx.OP_L2, hx.CMP_LT, P(r), 0, 64, 0, n, 4, ptrs, P(of), hx.RANGE_BY_DISTANCE, t, P(off), P(ids), P(d), ctypes.byref(total))
    assert rc == E_NOMEM and b"ordered by distance" in L.hx_last_error(e.h)
    assert (off == counts).all() and total.value == t
    e.close()


# ---- 6. ties and special values -------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_ties_and_special_values():
    rng = np.random.default_rng(651)
    # 64 copies of one row spread over two overlapping filters: equal values come back by row id, under both orders
    base = make(hx.F32, 300, 24, rng)
    rows = np.concatenate([base[:100], np.repeat(base[100:101], 64, 0), base[101:]])
    n = len(rows)
    qs = make(hx.F32, 5, 24, rng)
    qs[1] = qs[3] = rows[120]
    a, b = np.zeros(n, bool), np.zeros(n, bool)
    a[:140], b[120:] = True, True
    fo = np.array([0, 0, 1, 1, -1], np.int32)
    e = engine(hx.F32, 24, hx.OP_L2, rows, qs)
    for ordered in (False, True):
        off, ids, d = check(e, hx.OP_L2, 0.0, [a, b], fo, hx.CMP_LE, ordered, cpu=(hx.F32, 24, rows, qs, [1, 3], None))
        assert np.diff(off).tolist() == [0, 40, 0, 44, 0] and ids.tolist() == list(range(100, 140)) + list(range(120, 164)) and (d == 0).all()
        radii, _, _ = radii_of(e, hx.OP_L2, [a, b], fo)
        for cmp in CMPS:
            check(e, hx.OP_L2, radii, [a, b], fo, cmp, ordered)
    e.close()
    # rows with NaN and +-inf elements; radii NaN, +-inf, +-0.0; > and >= include the NaN-valued rows
    rows = make(hx.F32, 400, 8, rng)
    rows[5, 3], rows[50, 0], rows[51, 0], rows[300, 7] = np.nan, np.inf, -np.inf, np.nan
    qs = make(hx.F32, 6, 8, rng)
    masks = [np.arange(400) % 2 == 0, np.arange(400) % 2 == 1, np.arange(400) < 100]
    fo = np.array([0, 1, 2, 0, 1, -1], np.int32)
    for op in FOPS:
        e = engine(hx.F32, 8, op, rows, qs)
        cache = {}
        for radii in ([np.nan, np.inf, -np.inf, 0.0, -0.0, 1.5], [1.0, np.nan, 2.0, np.inf, 3.0, np.nan]):
            for cmp in CMPS:
                for ordered in (False, True):
                    off, ids, d = check(e, op, radii, masks, fo, cmp, ordered, cpu=(hx.F32, 8, rows, qs, [0, 1, 3, 5], None), cache=cache)
        off, ids, d = check(e, op, 1e30, masks, fo, hx.CMP_GT, True)                  # above every finite value: the inf- and NaN-valued rows
        assert 5 in ids[off[1]:off[2]] and np.isnan(d[off[2] - 1]) and 300 in ids[off[0]:off[1]]
        e.close()
    # <#> with a zero product: -0.0 keeps its sign and equals +0.0 in the predicate; <=> with a zero vector: NaN
    rows = make(hx.F32, 100, 4, rng)
    rows[::3, 0] = 0
    qs = np.array([[1, 0, 0, 0], [1, 0, 0, 0], [0, 0, 0, 0]], np.float32)
    masks = [np.arange(100) < 50, np.arange(100) >= 30]
    fo = np.array([0, 1, 1], np.int32)
    e = engine(hx.F32, 4, hx.OP_NEG_IP, rows, qs)
    for rr in (0.0, -0.0):
        for cmp in CMPS:
            for ordered in (False, True):
                off, ids, d = check(e, hx.OP_NEG_IP, rr, masks, fo, cmp, ordered, cpu=(hx.F32, 4, rows, qs, [0, 1], None))
                z = d[:off[1]] == 0
                assert z.sum() == (17 if cmp in (hx.CMP_LE, hx.CMP_GE) else 0) and np.signbit(d[:off[1]][z]).all()
    for cmp in CMPS:
        off, ids, d = check(e, hx.OP_COSINE, 0.5, masks, fo, cmp, True)
        assert int(off[3] - off[2]) == (70 if cmp in (hx.CMP_GT, hx.CMP_GE) else 0)   # the zero query: every value NaN, above everything
    assert np.isnan(d[off[2]:]).all() and ids[off[2]:].tolist() == list(range(30, 100))
    e.close()


# ---- 7. sidecar engine ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("dim", [132, 768])
def test_sidecar_engine(dim, monkeypatch):
    """Groups of 1, 4, 5 and 8 queries: tiles of 1, 4, 4 + 1 and 4 + 4, the tiles hx_exact_range takes for each group alone."""
    rng = np.random.default_rng(761 + dim)
    n = 3000
    fo = interleaved([1, 4, 5, 8], 0, rng)
    rows, qs = make(hx.F32, n, dim, rng), make(hx.F32, len(fo), dim, rng)
    masks = [rng.random(n) < p for p in (0.5, 0.2, 0.7, 0.35)]
    e, plain = engine(hx.F32, dim, hx.OP_L2, rows, qs), engine(hx.F32, dim, hx.OP_L2, rows, qs, sidecar=False)
    radii, _, _ = radii_of(plain, hx.OP_L2, masks, fo)
    order = np.argsort(fo, kind="stable")                   # the per-group calls need their queries in adjacent slots
    grouped = engine(hx.F32, dim, hx.OP_L2, rows, qs[order])
    for cmp in (hx.CMP_LT, hx.CMP_LE, hx.CMP_GT):
        for ordered in (False, True):
            monkeypatch.delenv("HX_EXACT_SIDECAR", raising=False)
            want = plain.exact_range_filtered(hx.OP_L2, radii, masks, fo, cmp=cmp, ordered=ordered)
            assert same(want, one_by_one(plain, hx.OP_L2, radii, masks, fo, cmp, ordered))
            assert same(e.exact_range_filtered(hx.OP_L2, radii, masks, fo, cmp=cmp, ordered=ordered), want)         # unset: below the threshold, no sidecar
            monkeypatch.setenv("HX_EXACT_SIDECAR", "0")
            e.exact_sidecar_stats(reset=True)
            assert same(e.exact_range_filtered(hx.OP_L2, radii, masks, fo, cmp=cmp, ordered=ordered), want)
            assert e.exact_sidecar_stats() == (0, 0)
            monkeypatch.setenv("HX_EXACT_SIDECAR", "1")
            e.exact_sidecar_stats(reset=True)
            assert same(e.exact_range_filtered(hx.OP_L2, radii, masks, fo, cmp=cmp, ordered=ordered), want)
            coded, fetched = e.exact_sidecar_stats(reset=True)
            assert same(plain.exact_range_filtered(hx.OP_L2, radii, masks, fo, cmp=cmp, ordered=ordered), want)     # no sidecar to force
            if cmp == hx.CMP_GT:
                assert (coded, fetched) == (0, 0)
                continue
            # the per-group calls: hx_exact_range over each group's queries with its bitmap
            grouped.exact_sidecar_stats(reset=True)
            at = 0
            for f in range(4):
                m = int((fo == f).sum())
                grouped.exact_range(hx.OP_L2, radii[order][at:at + m], cmp=cmp, first_query=at, nq=m, row_pass=masks[f], ordered=ordered)
                at += m
            g_coded, g_fetched = grouped.exact_sidecar_stats(reset=True)
            assert coded == g_coded == sum(int(masks[f].sum()) * t for f, t in enumerate((1, 1, 2, 2)))
            assert 0 < fetched <= coded
    for x in (e, plain, grouped):
        x.close()


# ---- 8. launch count ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_launch_count_does_not_grow_with_the_filters():
    rng = np.random.default_rng(871)
    n = 1500
    rows, qs = make(hx.F32, n, 16, rng), make(hx.F32, 32, 16, rng)
    e = engine(hx.F32, 16, hx.OP_L2, rows, qs)
    masks = [rng.random(n) < 0.05 + 0.01 * f for f in range(32)]
    e.set_timing(True)
    counts, got = {}, {}
    for nf in (4, 32):
        fo = (np.arange(32) % nf).astype(np.int32)
        e.kernel_stats(8, reset=True)
        got[nf] = e.exact_range_filtered(hx.OP_L2, 5.0, masks[:nf], fo)
        st = e.kernel_stats(8, reset=True)
        counts[nf] = st["launches"]
        assert st["units"] == sum(int(masks[f].sum()) for f in fo) and st["ms"] > 0
        assert same(got[nf], one_by_one(e, hx.OP_L2, np.full(32, 5.0), masks, fo))
        assert e.kernel_stats(8, reset=True)["launches"] >= 3 * 32          # what the separate calls cost
    assert counts[4] == counts[32] == 4                                         # one compaction, one scan (one tile size), the gather, the values
    e.close()


# ---- 9. argument errors ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_argument_errors():
    rng = np.random.default_rng(981)
    rows, qs = make(hx.F32, 100, 8, rng), make(hx.F32, 4, 8, rng)
    e = engine(hx.F32, 8, hx.OP_L2, rows, qs)
    L = hx.lib()
    off, ids, d, total = np.full(6, 7, np.uint64), np.full(400, 7, np.uint32), np.full(400, 7.0, np.float64), ctypes.c_uint64(7)
    P = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    words = [np.full(2, 0x5555555555555555, np.uint64), np.full(2, 0x3333333333333333, np.uint64)]
    two = (ctypes.c_void_p * 2)(words[0].ctypes.data, words[1].ctypes.data)
    many = (ctypes.c_void_p * 65)(*[words[0].ctypes.data] * 65)
    holed = (ctypes.c_void_p * 2)(words[0].ctypes.data, None)
    radius = np.full(5, 3.0)

    def call(op=hx.OP_L2, cmp=hx.CMP_LT, r=True, fq=0, nq=4, fr=0, nr=100, nf=2, filters=two, fo=(0, 1, -1, 0), order=hx.RANGE_BY_ROW, offs=True, tot=True,
             outs=(True, True)):
        of = None if fo is None else np.array(fo, np.int32)
        return L.hx_exact_range_filtered(e.h, op, cmp, P(radius) if r else None, fq, nq, fr, nr, nf, filters, None if of is None else P(of), order, 400,
                                         P(off) if offs else None, P(ids) if outs[0] else None, P(d) if outs[1] else None, ctypes.byref(total) if tot else None)

    def is_error(**kw):
        """HX_E_ARG with a message and the outputs untouched -> the message"""
        off[:], ids[:], d[:], total.value = 7, 7, 7.0, 7
        rc = call(**kw)
        msg = L.hx_last_error(e.h)
        return rc == E_ARG and (off == 7).all() and (ids == 7).all() and (d == 7.0).all() and total.value == 7 and msg

    assert call() == 0 and call(fo=None) == 0 and call(nf=0, filters=None, fo=(-1, -1, -1, -1)) == 0
    assert call(filters=holed, fo=(0, 0, -1, 0)) == 0                            # an unreferenced NULL filter is accepted
    assert call(outs=(False, False)) == 0 and call(outs=(True, False)) == 0
    m65 = is_error(nf=65, filters=many)
    assert m65 and b"HX_EXACT_MAX_FILTERS" in m65
    assert call(nf=64, filters=many) == 0
    for kw in (dict(fo=(0, 2, -1, 0)), dict(fo=(0, -2, -1, 0)), dict(filters=None), dict(filters=holed), dict(nf=0, filters=None, fo=(0, -1, -1, -1))):
        r = is_error(**kw)
        assert r and b"filter" in r, kw
        # the same message as hx_exact_search_filtered
        k_ids, k_d, k_c = np.empty(40, np.uint32), np.empty(40), np.empty(4, np.uint32)
        of = np.array(kw.get("fo", (0, 1, -1, 0)), np.int32)
        rc = L.hx_exact_search_filtered(e.h, hx.OP_L2, 0, 4, 0, 100, kw.get("nf", 2), kw.get("filters", two), P(of), 10, P(k_ids), P(k_d), P(k_c))
        assert rc == E_ARG and L.hx_last_error(e.h) == r
    # everything hx_exact_range rejects, with its messages
    for kw, text in ((dict(op=hx.OP_HAMMING), b"operator"), (dict(op=6), b"operator"), (dict(op=-1), b"operator"), (dict(cmp=4), b"comparison"),
                     (dict(cmp=-1), b"comparison"), (dict(order=2), b"order"), (dict(fr=50, nr=51), b"row range"), (dict(fr=101, nr=0), b"row range"),
                     (dict(fr=2 ** 32, nr=0), b"row range"), (dict(fq=1, nq=4), b"query range"), (dict(nq=5, fo=(0, 1, -1, 0, 0)), b"query range"),
                     (dict(r=False), b"NULL radius"), (dict(offs=False), b"NULL offsets"), (dict(tot=False), b"NULL offsets"),
                     (dict(outs=(False, True)), b"values without ids")):
        r = is_error(**kw)
        assert r and text in r, kw
        off[:], ids[:], d[:], total.value = 7, 7, 7.0, 7
        g = lambda name, default: kw.get(name, default)
        rc = L.hx_exact_range(e.h, g("op", hx.OP_L2), g("cmp", hx.CMP_LT), P(radius) if g("r", True) else None, g("fq", 0), g("nq", 4), g("fr", 0), g("nr", 100),
                              None, g("order", hx.RANGE_BY_ROW), 400, P(off) if g("offs", True) else None, P(ids) if g("outs", (True, True))[0] else None,
                              P(d) if g("outs", (True, True))[1] else None, ctypes.byref(total) if g("tot", True) else None)
        assert rc == E_ARG and L.hx_last_error(e.h) == r                        # the same message
    with pytest.raises(hx.HxError):
        e.exact_range_filtered(hx.OP_L2, 1.0, [np.ones(100, bool)], [0, 1, 0, 0])
    e.close()


# ---- 10. scan-only wide engine --------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_scan_only_wide_engine():
    rng = np.random.default_rng(1091)
    n, dim = 700, 3072
    rows, qs = make(hx.F32, n, dim, rng), make(hx.F32, 6, dim, rng)
    e = engine(hx.F32, dim, hx.OP_L2, rows, qs, scan_only=True)
    masks = [rng.random(n) < p for p in (0.5, 0.3, 0.1)]
    fo = np.array([0, 1, 0, 2, 1, 0], np.int32)
    for op in FOPS:
        radii, _, _ = radii_of(e, op, masks, fo)
        for cmp, ordered in ((hx.CMP_LE, False), (hx.CMP_LE, True), (hx.CMP_GT, False)):
            check(e, op, radii, masks, fo, cmp, ordered, cpu=(hx.F32, dim, rows, qs, [0, 3], None) if op == hx.OP_L2 else None)
    e.close()


# ---- 11. one distinct filter ----------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_one_distinct_filter_is_exact_range(monkeypatch):
    rng = np.random.default_rng(1101)
    n, dim = 1500, 132
    rows, qs = make(hx.F32, n, dim, rng), make(hx.F32, 3, dim, rng)
    masks = [rng.random(n) < 0.5, None, np.zeros(n, bool)]
    masks[2][rng.permutation(n)[:60]] = True
    e = engine(hx.F32, dim, hx.OP_L2, rows, qs)
    monkeypatch.setenv("HX_EXACT_SIDECAR", "1")            # the sidecar decision is hx_exact_range's too
    e.set_timing(True)
    for f in (np.array([2, 2, 2], np.int32), np.array([-1, -1, -1], np.int32), None):
        mask = None if f is None or f[0] < 0 else masks[2]
        radii = e.exact_search(hx.OP_L2, 10, row_pass=mask)[1][:, 9].copy()
        for ordered in (False, True):
            e.exact_sidecar_stats(reset=True)
            e.kernel_stats(8, reset=True)
            want = e.exact_range(hx.OP_L2, radii, cmp=hx.CMP_LE, row_pass=mask, ordered=ordered)
            sc_want, ks_want = e.exact_sidecar_stats(reset=True), e.kernel_stats(8, reset=True)
            got = e.exact_range_filtered(hx.OP_L2, radii, masks, f, cmp=hx.CMP_LE, ordered=ordered)
            sc_got, ks_got = e.exact_sidecar_stats(reset=True), e.kernel_stats(8, reset=True)
            assert same(got, want) and (np.diff(got[0]) >= 10).all()
            assert sc_want[0] > 0 and sc_got[0] == sc_want[0]
            assert (ks_got["launches"], ks_got["units"]) == (ks_want["launches"], ks_want["units"])
    e.close()
