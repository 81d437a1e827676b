"""hx_index_search_filtered: iterative index scans with a filter and a distance predicate PER QUERY of one launch
(`WHERE cond AND v <op> q <cmp> r ORDER BY v <op> q LIMIT k`, reference tests/t/017).

Expected values never come from the code under test: the oracle's amgettuple stream is filtered in Python the way the executor would
(PostgreSQL float8 comparison on the operator value of the oracle's distance), the existing entry point is given the equivalent single mask,
and the placements (traversal kernel, its roomier re-run, the lock-step driver) are compared with each other."""
import math
import os

import numpy as np
import pytest

import pgvector_rx_amd as hx
from oracle import orc

pytestmark = pytest.mark.gpu

NQ, EFS, LIMIT = 36, 20, 9
CMPS = {hx.CMP_LT: "<", hx.CMP_LE: "<=", hx.CMP_GT: ">", hx.CMP_GE: ">="}


def f8cmp(value, op, radius):
    """PostgreSQL's float8 comparison: NaN equals NaN and is above everything, -0.0 == +0.0."""
    a, b = float(value), float(radius)
    c = (0 if math.isnan(b) else 1) if math.isnan(a) else -1 if math.isnan(b) else (a > b) - (a < b)
    return {"<": c < 0, "<=": c <= 0, ">": c > 0, ">=": c >= 0}[op]


def op_value(metric, d):
    """The operator function's float8 result formed from the f32 distance: <-> takes the root, <#> <+> <~> widen."""
    d = np.float64(np.float32(d))
    with np.errstate(invalid="ignore"):
        return np.sqrt(d) if metric == hx.L2SQ else d


def random_sparse(rng, n, dim, max_nnz):
    rows = []
    for _ in range(n):
        k = int(rng.integers(1, max_nnz + 1))
        idx = np.sort(rng.choice(dim, k, replace=False)).astype(np.int32)
        val = rng.standard_normal(k).astype(np.float32)
        val[val == 0] = 1.0
        rows.append((idx, val))
    return rows


def make_rows(dt, n, dim, rng, data="uniform"):
    if data != "uniform":                                      # signed rows: N(0, 1); "scaled": times a per-row factor 10**U(-3, 3)
        x = rng.standard_normal((n, dim))
        if data == "scaled":
            x = x * 10.0 ** rng.uniform(-3.0, 3.0, (n, 1))
        x = x.astype(np.float32)
        return x if dt == hx.F32 else x.astype(np.float16).view(np.uint16)
    if dt == hx.F32:
        return rng.random((n, dim)).astype(np.float32)
    if dt == hx.F16:
        return rng.random((n, dim)).astype(np.float16).view(np.uint16)
    if dt == hx.SPARSE:
        return hx.pack_sparse(dim, random_sparse(rng, n, dim, 12))
    return np.packbits(rng.integers(0, 2, (n, dim)).astype(np.uint8), axis=1, bitorder="big")


class Setup:
    """A device index and the oracle's index on the same rows (heap TID == row id), NQ queries uploaded."""

    def __init__(self, dt, metric, dim, n, seed=7, data="uniform", precheck=None):
        rng = np.random.default_rng(seed)
        m, efc = 8, 32
        self.dt, self.metric, self.n = dt, metric, n
        rows = make_rows(dt, n, dim, rng, data)
        levels = hx.draw_levels(n, m, seed=seed)
        batch = 1 if dt == hx.SPARSE else 64
        # the summation order of the existing iterative parity tests (test_iterative_scan_on_device_equals_lockstep_and_oracle; sparsevec: test_gpu_sparse)
        self.o = orc.Index(dt, metric, dim, m=m, ef_construction=efc) if dt == hx.SPARSE else orc.Index(dt, metric, dim, m=m, ef_construction=efc, order=orc.W64)
        tids = np.arange(n, dtype=np.int64)
        i = 0
        for b in hx.batch_schedule(0, n, batch):
            self.o.insert_batch(rows[i:i + b], levels[i:i + b], tids[i:i + b])
            i += b
        self.qs = make_rows(dt, NQ, dim, rng, data)
        self._streams = {}
        self._near = [self.o.bruteforce_topk(self.qs[q], 500)[1] for q in range(NQ)]
        if precheck is not None:
            precheck(self)                                      # what the data is meant to do, on the oracle alone: no device call so far
        self.e = hx.Engine(dt, metric, dim, n)
        self.e.append(rows)
        self.ix = hx.Index(self.e, m, efc)
        self.ix.insert(0, levels, batch=batch)
        self.e.set_queries(self.qs)
        t = np.arange(n)
        self.filters = [(t % 100 == 0).astype(np.uint8), (t % 10 == 0).astype(np.uint8), (t % 2 == 0).astype(np.uint8), (t % 10 == 3).astype(np.uint8)]   # 1 %, 10 %, 50 %, 10 %
        self.filter_of = np.array([(q % 5) - 1 for q in range(NQ)], np.int32)                    # -1 (no filter), 0, 1, 2, 3

    def stream(self, q, mode, max_tuples=20000):
        key = (q, mode, max_tuples)
        if key not in self._streams:
            it = orc.ITER_RELAXED if mode == 1 else orc.ITER_STRICT
            self._streams[key] = self.o.scan(self.qs[q], ef_search=EFS, iterative=it, max_scan_tuples=max_tuples)
        return self._streams[key]

    def radii(self):
        """Per query: its own 5th / 50th / 500th-nearest operator value (a stored value: the tie decides between < and <=), NaN, below every value."""
        r = np.empty(NQ, np.float64)
        for q in range(NQ):
            kind = q % 6
            if kind == 3:
                r[q] = np.nan
            elif kind == 4:
                r[q] = -np.inf
            else:
                r[q] = op_value(self.metric, self._near[q][{0: 4, 1: 49, 2: 499, 5: 4}[kind]])
        return r

    def values(self, q, mode=2):
        """The distinct operator values of the query's stream, ascending (NaN left out)."""
        v = np.unique(np.array([op_value(self.metric, d) for _, d, _ in self.stream(q, mode)], np.float64))
        return v[~np.isnan(v)]

    def edge_radii(self):
        """Per query, radii that are NOT values of its stream: +0.0, -0.0, +inf; the float8 midpoint between its 5th and 6th distinct values (`<` and `<=`
        then select the same tuples); for <->, the float8 neighbours of sqrt(d5) on both sides; for <#>, radii of the sign opposite to most of the stream
        (the nearest tuples of an inner-product scan are negative); its own 5th value (the tie); NaN."""
        r = np.empty(NQ, np.float64)
        for q in range(NQ):
            v, kind = self.values(q), q % 9
            if kind == 0:
                r[q] = 0.0
            elif kind == 1:
                r[q] = -0.0
            elif kind == 2:
                r[q] = np.inf
            elif kind == 3:
                r[q] = (v[4] + v[5]) / 2
                assert v[4] < r[q] < v[5]
            elif kind in (4, 5):
                up = kind == 4
                if self.metric == hx.L2SQ:
                    r[q] = np.nextafter(v[4], np.inf if up else -np.inf)
                elif self.metric == hx.NEG_IP:
                    pos = v[v > 0]
                    r[q] = (pos[0] + pos[1]) / 2 if up else float(np.float32(pos[len(pos) // 2]))
                else:
                    r[q] = np.nextafter(v[4], np.inf if up else -np.inf)
            elif kind == 6:
                r[q] = v[4]
            elif kind == 7:
                r[q] = np.nan
            else:
                r[q] = -1.5 if self.metric != hx.NEG_IP else (v[9] + v[10]) / 2        # a negative radius
        return r

    def expected(self, q, mode, cmp, radius, limit=LIMIT, max_tuples=20000, filtered=True):
        out = []
        f = self.filter_of[q] if filtered else -1
        for tid, d, el in self.stream(q, mode, max_tuples):
            if len(out) >= limit:
                break
            if f >= 0 and not self.filters[f][tid]:
                continue
            if cmp is not None and not f8cmp(op_value(self.metric, d), CMPS[cmp], radius[q]):
                continue
            out.append((tid, np.float32(d)))
        return out

    def close(self):
        self.ix.close()
        self.e.close()


def same(a, b):
    return np.array_equal(a[3], b[3]) and np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32)) and np.array_equal(a[2], b[2])


SIGNED = [(hx.F32, hx.NEG_IP, 24, 4000, "normal"), (hx.F32, hx.L1, 12, 4000, "normal"), (hx.F16, hx.NEG_IP, 40, 4000, "normal"), (hx.F32, hx.L2SQ, 8, 4000, "scaled")]
SIGNED_IDS = ["vector-ip-normal", "vector-l1-normal", "halfvec-ip-normal", "vector-l2-scaled"]


def signed_precheck(s):
    """On the oracle's streams alone: <#> streams hold both signs for at least a quarter of the queries, and some query has a value of exactly +-0 or
    values on both sides of its zero radius; every kind of row has coordinates of both signs."""
    if s.metric != hx.NEG_IP:
        return
    both = zero = 0
    for q in range(NQ):
        for mode in (1, 2):
            v = s.values(q, mode)
            both += mode == 2 and (v < 0).any() and (v > 0).any()
            zero += (v == 0).any() or (q % 9 in (0, 1) and (v < 0).any() and (v > 0).any())
    print("streams with both signs", both, "of", NQ, "; zero values or crossings of a zero radius", zero)
    assert 4 * both >= NQ and zero > 0


SHAPES = [(hx.F32, hx.L2SQ, 8, 6000), (hx.F16, hx.NEG_IP, 24, 4000), (hx.BIT, hx.HAMMING, 64, 5000), (hx.SPARSE, hx.L2SQ, 300, 1200)]


@pytest.mark.parametrize("dt,metric,dim,n", SHAPES, ids=["vector-l2", "halfvec-ip", "bit-hamming", "sparsevec-l2"])
def test_filtered_scan_equals_the_oracle_stream_filtered_as_the_executor_would(dt, metric, dim, n):
    """36 queries per call mixing no filter and four filters of 1 / 10 / 50 / 10 %, radii at each query's own 5th / 50th / 500th-nearest
    value, NaN and -inf, for < <= > >= and for no predicate, in both modes: TIDs, counts and distance bits are those of the oracle's
    amgettuple stream filtered in Python; every query is served by the traversal kernel (redone == 0); the lock-step driver agrees."""
    s = Setup(dt, metric, dim, n)
    radius = s.radii()
    ties = 0
    for mode in (1, 2):
        for cmp in (None, hx.CMP_LT, hx.CMP_LE, hx.CMP_GT, hx.CMP_GE):
            before = s.ix.fused_stats()
            got = s.ix.search_filtered(NQ, EFS, mode, 20000, LIMIT, filters=s.filters, filter_of=s.filter_of, cmp=cmp, radius=None if cmp is None else radius)
            after = s.ix.fused_stats()
            assert after["tasks"] == before["tasks"] + NQ and after["redone"] == before["redone"]       # the kernel, not the fallback
            for q in range(NQ):
                want = s.expected(q, mode, cmp, radius)
                c = int(got[3][q])
                print("shape", dt, "mode", mode, "cmp", cmp, "q", q, "count", c, "want", len(want))
                assert c == len(want), (mode, cmp, q)
                assert got[0][q, :c].tolist() == [t for t, _ in want], (mode, cmp, q)
                assert np.array_equal(got[1][q, :c].view(np.uint32), np.array([d for _, d in want], np.float32).view(np.uint32)), (mode, cmp, q)
                if cmp in (hx.CMP_LT, hx.CMP_LE) and q % 6 == 4:
                    assert c == 0                                                                       # radius below every value
            if cmp is not None:                                                                         # placement: the lock-step driver evaluates the value itself
                s.ix.set_fused(False)
                try:
                    ls = s.ix.search_filtered(NQ, EFS, mode, 20000, LIMIT, filters=s.filters, filter_of=s.filter_of, cmp=cmp, radius=radius)
                finally:
                    s.ix.set_fused(True)
                assert same(got, ls), (mode, cmp)
        for q in range(NQ):                                                                             # the radius really is a value of the stream
            if q % 6 in (0, 1, 2, 5):
                ties += any(op_value(metric, d) == radius[q] for _, d, _ in s.stream(q, mode))
    assert ties > 0
    s.close()


@pytest.mark.parametrize("dt,metric,dim,n,data", SIGNED, ids=SIGNED_IDS)
def test_filtered_scan_on_signed_rows_equals_the_oracle_stream_filtered_as_the_executor_would(dt, metric, dim, n, data):
    """N(0, 1) rows and queries (<-> : rows scaled per row over six decades): distances of both signs, and radii that are no value of the stream (edge_radii)
    next to the stored-value, NaN and -inf kinds.  TIDs, counts and distance bits are the oracle's stream filtered in Python by f8cmp on op_value, on the
    traversal kernel (redone == 0), on the lock-step driver, and through one single-mask call of hx_index_search_iterative per query."""
    s = Setup(dt, metric, dim, n, seed=7, data=data, precheck=signed_precheck)
    all_rows = np.arange(n, dtype=np.uint32)
    for radius in (s.edge_radii(), s.radii()):
        for mode in (1, 2):
            res = {}
            for cmp in (hx.CMP_LT, hx.CMP_LE, hx.CMP_GT, hx.CMP_GE):
                s.e.set_queries(s.qs)
                before = s.ix.fused_stats()
                got = s.ix.search_filtered(NQ, EFS, mode, 20000, LIMIT, filters=s.filters, filter_of=s.filter_of, cmp=cmp, radius=radius)
                after = s.ix.fused_stats()
                assert after["tasks"] == before["tasks"] + NQ and after["redone"] == before["redone"]
                res[cmp] = got
                for q in range(NQ):
                    want = s.expected(q, mode, cmp, radius)
                    c = int(got[3][q])
                    print("shape", dt, metric, "mode", mode, "cmp", cmp, "q", q, "radius", radius[q], "count", c, "want", len(want))
                    assert c == len(want), (mode, cmp, q, radius[q])
                    assert got[0][q, :c].tolist() == [t for t, _ in want], (mode, cmp, q, radius[q])
                    assert np.array_equal(got[1][q, :c].view(np.uint32), np.array([d for _, d in want], np.float32).view(np.uint32)), (mode, cmp, q)
                s.ix.set_fused(False)
                try:
                    ls = s.ix.search_filtered(NQ, EFS, mode, 20000, LIMIT, filters=s.filters, filter_of=s.filter_of, cmp=cmp, radius=radius)
                finally:
                    s.ix.set_fused(True)
                assert same(got, ls), (mode, cmp)
                if (mode, cmp) in [(2, hx.CMP_LT), (1, hx.CMP_GE)]:                                        # the one-mask-per-query call of the existing entry point
                    for q in range(0, NQ, 2):
                        val = op_value(metric, s.e.distances(s.qs[q], all_rows))
                        mask = np.array([f8cmp(v, CMPS[cmp], radius[q]) for v in val], np.uint8)
                        if s.filter_of[q] >= 0:
                            mask &= s.filters[s.filter_of[q]]
                        s.e.set_queries(s.qs[q:q + 1])
                        t1, d1, c1 = s.ix.search_iterative(1, EFS, mode, 20000, LIMIT, mask)
                        assert int(got[3][q]) == int(c1[0]), (mode, cmp, q)
                        assert np.array_equal(got[0][q], t1[0]) and np.array_equal(got[1][q].view(np.uint32), d1[0].view(np.uint32)), (mode, cmp, q)
                    s.e.set_queries(s.qs)
            for q in range(NQ):                                                                            # a radius between two values: < and <= agree, > and >= agree
                if True:
                    if not any(op_value(metric, d) == radius[q] for _, d, _ in s.stream(q, mode)) and not np.isnan(radius[q]):
                        for a, b in ((hx.CMP_LT, hx.CMP_LE), (hx.CMP_GT, hx.CMP_GE)):
                            assert res[a][3][q] == res[b][3][q] and np.array_equal(res[a][0][q], res[b][0][q]), (mode, q, radius[q])
    s.close()


def test_stop_past_radius_on_a_signed_inner_product_stream():
    """HX_SCAN_STOP_PAST_RADIUS, strict order, `<` and `<=`, on N(0, 1) rows under <#>: radii that are negative (the 20th-nearest value), zero (+0.0 and -0.0)
    and positive (three quarters down the stream), every one inside the stream.  The tuples are those without the flag and the oracle's; the scan's distance
    evaluations (hx_index_counters()[4]) are strictly fewer with it."""
    s = Setup(hx.F32, hx.NEG_IP, 24, 4000, seed=7, data="normal", precheck=signed_precheck)
    n = s.n
    vals = [s.values(q) for q in range(NQ)]
    for name, radius, limit in [("negative", np.array([v[19] for v in vals]), 100), ("+0", np.zeros(NQ), n), ("-0", -np.zeros(NQ), n),
                                ("positive", np.array([v[3 * len(v) // 4] for v in vals]), n)]:
        for q in range(NQ):
            assert vals[q][0] < radius[q] < vals[q][-1] or (radius[q] == 0 and vals[q][0] < 0 < vals[q][-1])   # inside the stream
        assert (np.sign(radius) == {"negative": -1, "+0": 0, "-0": 0, "positive": 1}[name]).all()
        for cmp in (hx.CMP_LT, hx.CMP_LE):
            for fused in ((True, False) if limit == 100 else (True,)):                                     # the lock-step driver: the short scans
                s.ix.set_fused(fused)
                c0 = int(s.ix.counters()[4])
                plain = s.ix.search_filtered(NQ, EFS, 2, 20000, limit, cmp=cmp, radius=radius)
                c1 = int(s.ix.counters()[4])
                flag = s.ix.search_filtered(NQ, EFS, 2, 20000, limit, cmp=cmp, radius=radius, stop_past_radius=True)
                c2 = int(s.ix.counters()[4])
                print("radius", name, "cmp", cmp, "fused", fused, "distance evaluations without the flag", c1 - c0, "with", c2 - c1, "counts", plain[3][:6].tolist())
                assert same(plain, flag), (name, cmp, fused)
                assert (plain[3] < limit).all() and plain[3].sum() > 0
                assert 0 < c2 - c1 < c1 - c0, (name, cmp, fused)
                for q in range(0, NQ, 6):
                    want = s.expected(q, 2, cmp, radius, limit=limit, filtered=False)
                    assert plain[0][q, :plain[3][q]].tolist() == [t for t, _ in want], (name, cmp, q)
    s.ix.set_fused(True)
    s.close()


@pytest.mark.parametrize("dt,metric,dim,n", SHAPES[:3], ids=["vector-l2", "halfvec-ip", "bit-hamming"])
def test_filtered_scan_equals_one_call_of_the_existing_entry_point_per_query(dt, metric, dim, n):
    """Per query: the equivalent single mask built on the host -- its filter AND the predicate on hx_distances of that query against all rows --
    the query uploaded alone, hx_index_search_iterative(nq = 1).  Bit for bit; also pins `value = function of the returned f32`."""
    s = Setup(dt, metric, dim, n)
    radius = s.radii()
    all_rows = np.arange(n, dtype=np.uint32)
    for mode, cmp in [(2, hx.CMP_LT), (1, hx.CMP_LE), (2, hx.CMP_GE), (1, hx.CMP_GT)]:
        s.e.set_queries(s.qs)
        before = s.ix.fused_stats()
        got = s.ix.search_filtered(NQ, EFS, mode, 20000, LIMIT, filters=s.filters, filter_of=s.filter_of, cmp=cmp, radius=radius)
        assert s.ix.fused_stats()["redone"] == before["redone"]
        for q in range(NQ):
            val = op_value(metric, s.e.distances(s.qs[q], all_rows))
            mask = np.array([f8cmp(v, CMPS[cmp], radius[q]) for v in val], np.uint8)
            if s.filter_of[q] >= 0:
                mask &= s.filters[s.filter_of[q]]
            s.e.set_queries(s.qs[q:q + 1])
            t1, d1, c1 = s.ix.search_iterative(1, EFS, mode, 20000, LIMIT, mask)
            c = int(got[3][q])
            print("shape", dt, "mode", mode, "cmp", cmp, "q", q, "count", c, "single", int(c1[0]))
            assert c == int(c1[0]), (mode, cmp, q)
            assert np.array_equal(got[0][q], t1[0]) and np.array_equal(got[1][q].view(np.uint32), d1[0].view(np.uint32)), (mode, cmp, q)
    s.close()


def test_filtered_scan_that_outgrows_its_tables_is_redone_with_its_own_filter_and_predicate():
    """The "8x the room" re-run (HX_ITER_VIS_SHIFT=-5 makes the first tables 32x too small, as in
    test_iterative_scan_that_outgrows_its_tables_is_retried_on_the_device) keeps each redone query's filter row, predicate and stop rule."""
    s = Setup(hx.F32, hx.L2SQ, 8, 6000, seed=19)
    radius = s.radii()
    for mode, cmp, stop in [(1, hx.CMP_GT, False), (2, hx.CMP_LE, False), (2, hx.CMP_LT, True)]:
        ref = s.ix.search_filtered(NQ, EFS, mode, 20000, LIMIT, filters=s.filters, filter_of=s.filter_of, cmp=cmp, radius=radius, stop_past_radius=stop)
        os.environ["HX_ITER_VIS_SHIFT"] = "-5"
        try:
            before = s.ix.fused_stats()
            got = s.ix.search_filtered(NQ, EFS, mode, 20000, LIMIT, filters=s.filters, filter_of=s.filter_of, cmp=cmp, radius=radius, stop_past_radius=stop)
            after = s.ix.fused_stats()
        finally:
            del os.environ["HX_ITER_VIS_SHIFT"]
        assert after["redone"] == before["redone"]                       # nothing reached the lock-step driver
        assert same(ref, got), (mode, cmp, stop)
        for q in range(NQ):
            want = s.expected(q, mode, cmp, radius)
            assert got[0][q, :got[3][q]].tolist() == [t for t, _ in want], (mode, cmp, q)
    s.close()


def test_stop_past_radius_returns_the_same_tuples_for_less_work():
    """strict_order, `<` with the radius at the 20th-nearest value, limit 100, max_scan_tuples 20000: the same outputs with and without
    HX_SCAN_STOP_PAST_RADIUS (counts < limit), strictly fewer scan distance evaluations (hx_index_counters()[4]) with it -- on the
    traversal kernel and on the lock-step driver."""
    s = Setup(hx.F32, hx.L2SQ, 8, 6000, seed=23)
    radius = np.array([op_value(hx.L2SQ, s._near[q][19]) for q in range(NQ)])
    for fused in (True, False):
        s.ix.set_fused(fused)
        c0 = int(s.ix.counters()[4])
        plain = s.ix.search_filtered(NQ, EFS, 2, 20000, 100, cmp=hx.CMP_LT, radius=radius)
        c1 = int(s.ix.counters()[4])
        flag = s.ix.search_filtered(NQ, EFS, 2, 20000, 100, cmp=hx.CMP_LT, radius=radius, stop_past_radius=True)
        c2 = int(s.ix.counters()[4])
        print("fused", fused, "distance evaluations without the flag", c1 - c0, "with", c2 - c1, "counts", plain[3].tolist())
        assert same(plain, flag)
        assert (plain[3] < 100).all() and plain[3].sum() > 0
        assert 0 < c2 - c1 < c1 - c0
        for q in range(0, NQ, 4):
            want = s.expected(q, 2, hx.CMP_LT, radius, limit=100, filtered=False)
            assert plain[0][q, :plain[3][q]].tolist() == [t for t, _ in want], q
    s.ix.set_fused(True)
    for mode, cmp in [(1, hx.CMP_LT), (2, hx.CMP_GT), (2, hx.CMP_GE), (2, None)]:                # the flag needs strict_order and < / <=
        with pytest.raises(hx.HxError) as ei:
            s.ix.search_filtered(NQ, EFS, mode, 20000, 10, cmp=cmp, radius=radius, stop_past_radius=True)
        assert ei.value.code == -1 and "HX_SCAN_STOP_PAST_RADIUS" in str(ei.value)
    s.close()


def test_the_existing_entry_point_is_the_special_case():
    s = Setup(hx.BIT, hx.HAMMING, 64, 5000)
    for mode in (1, 2):
        for f in s.filters[:2]:
            a = s.ix.search_iterative(NQ, EFS, mode, 20000, LIMIT, filter_pass=f)
            b = s.ix.search_filtered(NQ, EFS, mode, 20000, LIMIT, filters=[f], filter_of=[0] * NQ)
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32)) and np.array_equal(a[2], b[3])
        a = s.ix.search_iterative(NQ, EFS, mode, 20000, LIMIT)
        b = s.ix.search_filtered(NQ, EFS, mode, 20000, LIMIT)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32)) and np.array_equal(a[2], b[3])
        c = s.ix.search_filtered(NQ, EFS, mode, 20000, LIMIT, filters=s.filters, filter_of=[-1] * NQ)      # filters nobody uses
        assert same(b, c)
    s.close()


def test_argument_errors():
    s = Setup(hx.F32, hx.L2SQ, 8, 800)
    r = np.ones(NQ)
    ok = dict(nq=NQ, ef_search=EFS, mode=2, max_scan_tuples=20000, limit=LIMIT)

    def bad(code=-1, **kw):
        a = dict(ok)
        a.update(kw)
        with pytest.raises(hx.HxError) as ei:
            s.ix.search_filtered(**a)
        assert ei.value.code == code, kw
        assert len(str(ei.value).split(": ", 1)[1]) > 0, kw                 # hx_index_last_error is set

    bad(mode=0)
    bad(mode=3)
    bad(max_scan_tuples=0)
    bad(filters=[s.filters[0]] * 65, filter_of=[0] * NQ)                       # > HX_SCAN_MAX_FILTERS
    bad(filters=s.filters, filter_of=[4] * NQ)
    bad(filters=s.filters, filter_of=[-2] * NQ)
    bad(filter_of=[0] * NQ)                                                    # no filters at all: 0 is outside [-1, 0)
    bad(cmp=4, radius=r)
    bad(cmp=-2, radius=r)
    bad(cmp=hx.CMP_LT)                                                         # radius == NULL
    bad(ef_search=0)
    bad(ef_search=1001)
    L = hx.lib()
    import ctypes as C
    tids, cnt = np.zeros((NQ, LIMIT), np.int64), np.zeros(NQ, np.uint32)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    assert L.hx_index_search_filtered(s.ix.h, NQ, EFS, 2, 20000, LIMIT, 0, None, None, None, -1, None, 2, vp(tids), None, None, vp(cnt)) == -1   # unknown flag
    assert b"flag" in L.hx_index_last_error(s.ix.h)
    assert L.hx_index_search_filtered(s.ix.h, NQ, EFS, 2, 20000, LIMIT, 0, None, None, None, -1, None, 0, None, None, None, vp(cnt)) == -1       # NULL outputs
    assert L.hx_index_search_filtered(s.ix.h, NQ, EFS, 2, 20000, LIMIT, 0, None, None, None, -1, None, 0, vp(tids), None, None, None) == -1
    assert len(L.hx_index_last_error(s.ix.h)) > 0
    s.e.set_queries(s.qs[:4])
    bad(code=-6)                                                               # HX_E_STATE: more queries than were uploaded, as hx_index_search_iterative
    s.close()
    rng = np.random.default_rng(3)
    rows = make_rows(hx.BIT, 300, 64, rng)
    e = hx.Engine(hx.BIT, hx.JACCARD, 64, 300)
    e.append(rows)
    ix = hx.Index(e, 8, 32)
    ix.insert(0, hx.draw_levels(300, 8, seed=3), batch=64)
    e.set_queries(rows[:4])
    with pytest.raises(hx.HxError) as ei:
        ix.search_filtered(4, EFS, 2, 20000, LIMIT, cmp=hx.CMP_LT, radius=0.5)
    assert ei.value.code == -1 and "Jaccard" in str(ei.value)
    assert ix.search_filtered(4, EFS, 2, 20000, LIMIT)[3].tolist() == ix.search_iterative(4, EFS, 2, 20000, LIMIT)[2].tolist()   # filters alone are fine
    ix.close()
    e.close()
