"""hx_exact_range: the distance-threshold scans -- the sequential-scan plans of `WHERE v <op> q < r` and `WHERE v <op> q < r ORDER BY v <op> q`
(tests/t/017_hnsw_filtering.pl:75-99) -- on the device, checked against the oracle composed in tests/exact_ref.py: the expected rows of a query
are the candidate rows whose value satisfies PostgreSQL's float8 comparison with its radius, in row order or in ref.order."""
import ctypes

import numpy as np
import pytest

import pgvector_rx_amd as hx
import exact_ref as ref
from test_gpu_exact import BOPS, FOPS, engine, make, north_star

CMPS = [hx.CMP_LT, hx.CMP_LE, hx.CMP_GT, hx.CMP_GE]
E_ARG, E_NOMEM = -1, -3


def f8cmp(v, r, cmp):
    """float8lt / le / gt / ge: -0.0 == +0.0, NaN equal to NaN and above everything."""
    nv, nr = np.isnan(v), bool(np.isnan(r))
    with np.errstate(invalid="ignore"):
        if cmp == hx.CMP_LT:
            return ~nv & (nr | (v < r))
        if cmp == hx.CMP_LE:
            return nr | (~nv & (v <= r))
        if cmp == hx.CMP_GT:
            return (nv & (not nr)) | (~nv & (not nr) & (v > r))
        return nv | ((not nr) & (v >= r))


def expected(vals, cand, r, cmp, ordered):
    keep = f8cmp(vals, r, cmp)
    ids, v = cand[keep], vals[keep]
    if ordered:
        o = ref.order(v, ids)
        ids, v = ids[o], v[o]
    return ids, v


def check(e, dtype, dim, op, rows, queries, radii, cmp, ordered, first_query=0, nq=None, first_row=0, n_rows=None, mask=None, norms=None,
          seq=False, vals=None):
    """Runs the range scan and compares every query's ids and value bits with the composed reference; returns (offsets, ids, dist, vals)."""
    nq = len(queries) - first_query if nq is None else nq
    n_rows = len(rows) - first_row if n_rows is None else n_rows
    radii = np.broadcast_to(np.asarray(radii, np.float64), (nq,))
    off, ids, dist = e.exact_range(op, radii, cmp=cmp, first_query=first_query, nq=nq, first_row=first_row, n_rows=n_rows, row_pass=mask,
                                   ordered=ordered)
    cand = np.arange(first_row, first_row + n_rows)
    if mask is not None:
        cand = cand[np.asarray(mask, bool)]
    if vals is None:
        vals = [ref.values(dtype, dim, op, queries[first_query + qi], rows[cand], None if norms is None else norms[cand]) for qi in range(nq)]
    assert off[0] == 0 and len(off) == nq + 1 and len(ids) == len(dist) == off[-1]
    for qi in range(nq):
        want_ids, want_v = expected(vals[qi], cand, radii[qi], cmp, ordered)
        a, b = int(off[qi]), int(off[qi + 1])
        assert ids[a:b].tolist() == want_ids.tolist(), (op, cmp, ordered, qi, b - a, len(want_ids))
        assert ref.same_bits(dist[a:b], want_v), (op, cmp, ordered, qi)
        if seq and b > a:
            north_star(dtype, dim, op, queries[first_query + qi], rows[ids[a:b].astype(np.int64)], dist[a:b])
    return off, ids, dist, vals


def quantile_radii(vals, qs):
    """Per query a radius equal to the value at quantile qs[i % len(qs)] of its finite values (a row's own value: the boundary case)."""
    out = []
    for i, v in enumerate(vals):
        f = np.sort(v[~np.isnan(v)])
        out.append(f[int(qs[i % len(qs)] * (len(f) - 1))] if len(f) else 0.0)
    return np.array(out)


# ---- 1. parity matrix -----------------------------------------------------------------------------------------------------------------------
CASES = [(hx.F32, d) for d in (3, 17, 300, 768, 2000)] + [(hx.F16, 10), (hx.F16, 4000), (hx.BIT, 8), (hx.BIT, 1024), (hx.BIT, 64000),
                                                           (hx.SPARSE, 100)]


@pytest.mark.gpu
@pytest.mark.parametrize("dtype,dim", CASES, ids=lambda v: str(v))
def test_parity_matrix(dtype, dim):
    rng = np.random.default_rng(70 + dim + 10 * dtype)
    n = 1200 if dim <= 768 else 400
    rows, qs = make(dtype, n, dim, rng), make(dtype, 20, dim, rng)
    norms = None
    for op in (BOPS if dtype == hx.BIT else FOPS):
        e = engine(dtype, dim, op, rows, qs)
        if op == hx.OP_COSINE and dtype != hx.SPARSE and norms is None:
            norms = ref.self_ip(dtype, dim, rows)
        nm = norms if op == hx.OP_COSINE else None
        vals = [ref.values(dtype, dim, op, qs[1 + i], rows, nm) for i in range(5)]
        radii = quantile_radii(vals, [0.02, 0.5, 0.97])                       # radii that differ within the call
        for cmp in CMPS:
            for ordered in (False, True):
                check(e, dtype, dim, op, rows, qs, radii, cmp, ordered, first_query=1, nq=5, norms=nm, vals=vals, seq=(cmp == hx.CMP_LT and not ordered))
        if dtype != hx.SPARSE:                                                   # 20 queries: a tile of 16 and a partial one
            vals20 = [ref.values(dtype, dim, op, qs[i], rows, nm) for i in range(20)]
            check(e, dtype, dim, op, rows, qs, quantile_radii(vals20, [0.1, 0.3]), hx.CMP_LE, True, vals=vals20)
            check(e, dtype, dim, op, rows, qs, quantile_radii(vals20, [0.1, 0.3]), hx.CMP_GT, False, vals=vals20)
        e.close()


# ---- 2. boundaries --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_boundaries():
    rng = np.random.default_rng(21)
    rows = make(hx.F32, 500, 12, rng)
    rows[100:110] = rows[7]                                                      # equal values: the radius is one of them
    qs = make(hx.F32, 2, 12, rng)
    e = engine(hx.F32, 12, hx.OP_L2, rows, qs)
    v = ref.values(hx.F32, 12, hx.OP_L2, qs[0], rows)
    r = v[7]
    _, lt, _, _ = check(e, hx.F32, 12, hx.OP_L2, rows, qs, r, hx.CMP_LT, False, nq=1)
    _, le, d, _ = check(e, hx.F32, 12, hx.OP_L2, rows, qs, r, hx.CMP_LE, True, nq=1)
    assert 7 not in lt and set(range(100, 110)) | {7} <= set(le.tolist()) and le[-11:].tolist() == [7] + list(range(100, 110))
    for rr in (np.inf, -np.inf, np.nan, 0.0, -0.0):
        for cmp in CMPS:
            for ordered in (False, True):
                check(e, hx.F32, 12, hx.OP_L2, rows, qs, rr, cmp, ordered)
    off, ids, _ = e.exact_range(hx.OP_L2, np.nan, cmp=hx.CMP_LT)                # < NaN: every non-NaN row; <= NaN: every row; > NaN: none
    assert (np.diff(off) == 500).all()
    assert (np.diff(e.exact_range(hx.OP_L2, np.nan, cmp=hx.CMP_GT)[0]) == 0).all()
    # <#> with zero products: -0.0 values against +-0.0 radii
    rows = make(hx.F32, 90, 4, rng)
    rows[::3, 0] = 0
    q = np.array([[1, 0, 0, 0]], np.float32)
    e = engine(hx.F32, 4, hx.OP_NEG_IP, rows, q)
    for rr in (0.0, -0.0):
        for cmp in CMPS:
            _, ids, d, _ = check(e, hx.F32, 4, hx.OP_NEG_IP, rows, q, rr, cmp, True)
            z = d == 0
            assert z.sum() == (30 if cmp in (hx.CMP_LE, hx.CMP_GE) else 0) and np.signbit(d[z]).all()
    # <=> with zero rows: NaN values are in > r and >= r, never in < r
    rows = make(hx.F32, 200, 8, rng)
    rows[[5, 50, 77]] = 0
    q = make(hx.F32, 1, 8, rng)
    e = engine(hx.F32, 8, hx.OP_COSINE, rows, q)
    norms = ref.self_ip(hx.F32, 8, rows)
    for rr in (0.5, np.inf, np.nan):
        for cmp in CMPS:
            for ordered in (False, True):
                _, ids, d, _ = check(e, hx.F32, 8, hx.OP_COSINE, rows, q, rr, cmp, ordered, norms=norms)
                has = {5, 50, 77} & set(ids.tolist())
                if cmp in (hx.CMP_GT, hx.CMP_GE) and not np.isnan(rr):
                    assert has == {5, 50, 77} and (not ordered or ids[-3:].tolist() == [5, 50, 77])
                if cmp == hx.CMP_LT:
                    assert not has and not np.isnan(d).any()


# ---- 3. shapes ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_shapes_and_filters():
    rng = np.random.default_rng(33)
    n = 6000
    rows, qs = rng.random((n, 3), dtype=np.float32), rng.random((9, 3), dtype=np.float32)
    e = engine(hx.F32, 3, hx.OP_L2, rows, qs)
    radii = np.linspace(0.05, 0.4, 6)
    check(e, hx.F32, 3, hx.OP_L2, rows, qs, radii, hx.CMP_LT, False, first_query=3, nq=6)
    check(e, hx.F32, 3, hx.OP_L1, rows, qs, radii, hx.CMP_GE, True, first_query=2, nq=6, first_row=1234, n_rows=2345)
    mask = (np.arange(n) % 50) == 7                                              # 017: c = i % 50, WHERE c = 7
    for ordered in (False, True):
        _, ids, _, _ = check(e, hx.F32, 3, hx.OP_L2, rows, qs, 0.5, hx.CMP_LT, ordered, mask=mask)
        assert (ids % 50 == 7).all()
    sub = rng.random(2345) < 0.3
    check(e, hx.F32, 3, hx.OP_L2, rows, qs, 0.3, hx.CMP_LE, False, first_row=1234, n_rows=2345, mask=sub)
    words = np.packbits(np.concatenate([sub, np.zeros(2368 - 2345, bool)]), bitorder="little").view(np.uint64)
    a = e.exact_range(hx.OP_L2, 0.3, cmp=hx.CMP_LE, first_row=1234, n_rows=2345, row_pass=sub)
    b = e.exact_range(hx.OP_L2, 0.3, cmp=hx.CMP_LE, first_row=1234, n_rows=2345, row_pass=words, packed=True)
    assert all((x == y).all() for x, y in zip(a, b))
    e.set_timing(True)
    e.kernel_stats(8, reset=True)
    off, ids, d = e.exact_range(hx.OP_L2, np.inf, cmp=hx.CMP_LE, row_pass=np.zeros(n, bool))     # all fail: empty, nothing launched
    assert (off == 0).all() and len(ids) == len(d) == 0 and e.kernel_stats(8)["launches"] == 0
    check(e, hx.F32, 3, hx.OP_L2, rows, qs, 0.2, hx.CMP_LT, True, mask=np.ones(n, bool))        # all pass
    off, ids, d = e.exact_range(hx.OP_L2, 0.1, nq=0)
    assert off.tolist() == [0] and len(ids) == 0


# ---- 4. count-only and capacity -------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_count_only_and_capacity():
    rng = np.random.default_rng(44)
    rows, qs = make(hx.F32, 3000, 32, rng), make(hx.F32, 7, 32, rng)
    e = engine(hx.F32, 32, hx.OP_L2, rows, qs)
    r = np.linspace(6.5, 8.0, 7)
    for ordered in (False, True):
        off, ids, d = e.exact_range(hx.OP_L2, r, ordered=ordered)
        c_off, c_ids, c_d = e.exact_range(hx.OP_L2, r, ordered=ordered, count_only=True)
        assert (c_off == off).all() and len(c_ids) == len(c_d) == 0
        total = int(off[-1])
        assert 0 < total < 3000 * 7
        L, P = hx.lib(), lambda a: a.ctypes.data_as(ctypes.c_void_p)
        rr = np.ascontiguousarray(r)
        o2, i2, d2, t = np.zeros(8, np.uint64), np.empty(total, np.uint32), np.empty(total, np.float64), ctypes.c_uint64()
        order = hx.RANGE_BY_DISTANCE if ordered else hx.RANGE_BY_ROW
        rc = L.hx_exact_range(e.h, hx.OP_L2, hx.CMP_LT, P(rr), 0, 7, 0, 3000, None, order, total - 1, P(o2), P(i2), P(d2), ctypes.byref(t))
        assert rc == E_NOMEM and t.value == total and (o2 == off).all()
        rc = L.hx_exact_range(e.h, hx.OP_L2, hx.CMP_LT, P(rr), 0, 7, 0, 3000, None, order, total, P(o2), P(i2), P(d2), ctypes.byref(t))
        assert rc == 0 and t.value == total and (o2 == off).all() and (i2 == ids).all() and ref.same_bits(d2, d)
        rc = L.hx_exact_range(e.h, hx.OP_L2, hx.CMP_LT, P(rr), 0, 7, 0, 3000, None, order, total, P(o2), P(i2), None, ctypes.byref(t))
        assert rc == 0 and (i2 == ids).all()                                                   # ids without values
        with pytest.raises(hx.HxError) as ei:
            e.exact_range(hx.OP_L2, r, ordered=ordered, cap=total - 1)
        assert ei.value.code == E_NOMEM
        o3, i3, d3 = e.exact_range(hx.OP_L2, r, ordered=ordered, cap=total)
        assert (i3 == ids).all()
    big = e.exact_range(hx.OP_L2, np.inf, cmp=hx.CMP_LE)                           # every row of every query, in row order
    assert big[0][-1] == 3000 * 7 and all((big[1][i * 3000:(i + 1) * 3000] == np.arange(3000)).all() for i in range(7))


# ---- 5. bounded scratch ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_bounded_scratch(monkeypatch):
    rng = np.random.default_rng(55)
    rows, qs = make(hx.F32, 5000, 64, rng), make(hx.F32, 300, 64, rng)
    e = engine(hx.F32, 64, hx.OP_L2, rows, qs)
    r = np.full(300, 11.0)
    r[::7] = 10.0
    runs = {}
    for env in (None, str(1 << 20)):
        if env:
            monkeypatch.setenv("HX_RANGE_SCRATCH", env)
        runs[env] = [e.exact_range(hx.OP_L2, r, cmp=cmp, ordered=o) for cmp, o in ((hx.CMP_LT, False), (hx.CMP_GE, True))] + \
                    [e.exact_range(hx.OP_L2, r, count_only=True)]
        monkeypatch.delenv("HX_RANGE_SCRATCH", raising=False)
    assert runs[None][0][0][-1] > 300 * 500                                       # many hits per query: staging overflows at 1 MiB
    for a, b in zip(runs[None], runs[str(1 << 20)]):
        assert all(x.shape == y.shape and (x.view(np.uint8) == y.view(np.uint8)).all() for x, y in zip(a, b))
    # check one block of the small-scratch run against the reference
    monkeypatch.setenv("HX_RANGE_SCRATCH", str(1 << 20))
    check(e, hx.F32, 64, hx.OP_L2, rows, qs, r[:40], hx.CMP_LT, False, nq=40)
    monkeypatch.delenv("HX_RANGE_SCRATCH")
    # radius +inf over 200 000 x 768: every row is a hit
    n, dim = 200_000, 768
    rows = rng.standard_normal((n, dim), dtype=np.float32)
    e = engine(hx.F32, dim, hx.OP_L2, rows, rows[:3].copy())
    full = e.exact_range(hx.OP_L2, np.inf, cmp=hx.CMP_LT)                        # more hits than the binding's first capacity: two calls
    assert (np.diff(full[0]) == n).all() and all((full[1][i * n:(i + 1) * n] == np.arange(n)).all() for i in range(3))
    fo = e.exact_range(hx.OP_L2, np.inf, cmp=hx.CMP_LT, ordered=True)
    assert fo[1][0] == 0 and fo[2][0] == 0.0 and (np.diff(fo[2][:n]) >= 0).all()
    monkeypatch.setenv("HX_RANGE_SCRATCH", str(1 << 20))
    small = e.exact_range(hx.OP_L2, np.inf, cmp=hx.CMP_LT)
    assert all((x.view(np.uint8) == y.view(np.uint8)).all() for x, y in zip(full, small))
    with pytest.raises(hx.HxError) as ei:                                         # by distance, one query's hits must fit the scratch
        e.exact_range(hx.OP_L2, np.inf, cmp=hx.CMP_LT, ordered=True)
    assert ei.value.code == E_NOMEM
    cnt = e.exact_range(hx.OP_L2, np.inf, cmp=hx.CMP_LT, ordered=True, count_only=True)[0]    # counting needs no window
    assert (cnt == full[0]).all()


# ---- 6. agreement with hx_exact_search ------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("dtype,dim", [(hx.F32, 40), (hx.F16, 300), (hx.BIT, 256), (hx.SPARSE, 60)], ids=lambda v: str(v))
def test_agrees_with_exact_search(dtype, dim):
    rng = np.random.default_rng(66 + dtype)
    rows, qs = make(dtype, 2000, dim, rng), make(dtype, 6, dim, rng)
    for op in (BOPS if dtype == hx.BIT else FOPS):
        e = engine(dtype, dim, op, rows, qs)
        for k in (1, 10, 100):
            ids, d, cnt = e.exact_search(op, k)
            off, rid, rd = e.exact_range(op, d[:, k - 1], cmp=hx.CMP_LE, ordered=True)
            for q in range(6):
                a = int(off[q])
                assert rid[a:a + k].tolist() == ids[q].tolist() and ref.same_bits(rd[a:a + k], d[q]), (op, k, q)
        e.close()


# ---- 7. size --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_at_scale_200k_768():
    rng = np.random.default_rng(77)
    n, dim = 200_000, 768
    rows, qs = rng.standard_normal((n, dim), dtype=np.float32), rng.standard_normal((64, dim), dtype=np.float32)
    e = engine(hx.F32, dim, hx.OP_L2, rows, qs)
    ids, d, _ = e.exact_search(hx.OP_L2, 1024)
    r = d[:, 199]                                                                 # the 0.1 % quantile: 200 rows per query
    off, rid, rd = e.exact_range(hx.OP_L2, r, cmp=hx.CMP_LE, ordered=True)
    assert (np.diff(off) >= 200).all()
    for q in range(64):
        a, b = int(off[q]), int(off[q + 1])
        keep = d[q] <= r[q]
        assert rid[a:b].tolist() == ids[q][keep].tolist() and ref.same_bits(rd[a:b], d[q][keep])
    off2, rid2, rd2 = e.exact_range(hx.OP_L2, r, cmp=hx.CMP_LE)
    assert (off2 == off).all()
    for q in range(64):
        a, b = int(off[q]), int(off[q + 1])
        o = np.argsort(rid[a:b])
        assert rid2[a:b].tolist() == rid[a:b][o].tolist() and ref.same_bits(rd2[a:b], rd[a:b][o])
    check(e, hx.F32, dim, hx.OP_L2, rows, qs, r[:2], hx.CMP_LE, False, nq=2)   # and two queries against the composed reference


# ---- 8. argument errors and stats -----------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_argument_errors_and_stats():
    rng = np.random.default_rng(88)
    rows, qs = make(hx.F32, 100, 8, rng), make(hx.F32, 4, 8, rng)
    e = engine(hx.F32, 8, hx.OP_L2, rows, qs)
    L, P = hx.lib(), lambda a: a.ctypes.data_as(ctypes.c_void_p)
    r, off, ids, d, t = np.full(4, 3.0), np.zeros(5, np.uint64), np.empty(400, np.uint32), np.empty(400, np.float64), ctypes.c_uint64()

    def call(op=hx.OP_L2, cmp=hx.CMP_LT, rad=True, fq=0, nq=4, fr=0, nr=100, order=0, o=True, i=True, dd=True, tt=True):
        return L.hx_exact_range(e.h, op, cmp, P(r) if rad else None, fq, nq, fr, nr, None, order, 400, P(off) if o else None,
                                P(ids) if i else None, P(d) if dd else None, ctypes.byref(t) if tt else None)
    assert call() == 0
    assert call(op=hx.OP_HAMMING) == E_ARG and call(op=hx.OP_JACCARD) == E_ARG and call(op=6) == E_ARG and call(op=-1) == E_ARG
    assert call(cmp=4) == E_ARG and call(cmp=-1) == E_ARG and call(order=2) == E_ARG and call(order=-1) == E_ARG
    assert call(rad=False) == E_ARG and call(rad=False, nq=0) == 0
    assert call(o=False) == E_ARG and call(tt=False) == E_ARG and call(i=False) == E_ARG and call(i=False, dd=False) == 0
    assert call(fr=50, nr=51) == E_ARG and call(fr=101, nr=0) == E_ARG and call(fr=2 ** 32, nr=0) == E_ARG
    assert call(fq=1, nq=4) == E_ARG and call(nq=5) == E_ARG
    eb = engine(hx.BIT, 64, hx.OP_HAMMING, make(hx.BIT, 10, 64, rng), make(hx.BIT, 1, 64, rng))
    for op in FOPS:
        with pytest.raises(hx.HxError):
            eb.exact_range(op, 1.0)
    e.set_timing(True)
    e.exact_search(hx.OP_L2, 5)
    k7 = e.kernel_stats(7)
    e.kernel_stats(8, reset=True)
    e.exact_range(hx.OP_L2, 3.0)
    e.exact_range(hx.OP_L2, 3.0, ordered=True)
    st = e.kernel_stats(8)
    assert st["units"] == 2 * 100 * 4 and st["launches"] >= 4 and st["ms"] > 0
    assert e.kernel_stats(7) == k7                                                # kind 7 is not touched by range calls


# ---- 9. concurrency with a pipelined index scan ---------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_while_index_scan_in_flight():
    rng = np.random.default_rng(99)
    n, dim = 4000, 32
    rows, qs = rng.random((n, dim), dtype=np.float32), rng.random((16, dim), dtype=np.float32)
    e = hx.Engine(hx.F32, hx.L2SQ, dim, n)
    e.append(rows)
    e.set_queries(qs)
    ix = hx.Index(e, 8, 32)
    ix.insert(0, hx.draw_levels(n, 8, seed=9), batch=256)
    alone = ix.search(16, 40, 10)
    rg = e.exact_range(hx.OP_L2, 1.2, cmp=hx.CMP_LT)
    rgo = e.exact_range(hx.OP_L2, 1.2, cmp=hx.CMP_LT, ordered=True)
    ix.search_submit(0, 0, 16, 40, 10)
    during = e.exact_range(hx.OP_L2, 1.2, cmp=hx.CMP_LT)
    during_o = e.exact_range(hx.OP_L2, 1.2, cmp=hx.CMP_LT, ordered=True)
    waited = ix.search_wait(0)
    assert all((a.view(np.uint8) == b.view(np.uint8)).all() for a, b in zip(rg + rgo, during + during_o))
    assert all((a == b).all() for a, b in zip(alone, waited))
    ix.close()
    e.close()
