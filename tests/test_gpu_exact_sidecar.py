"""The exact scans' 8-bit sidecar path (hx_exact_search, hx_exact_range with `<` / `<=` on f32 L2 engines that keep a sidecar):
every output is bit for bit that of the scan without it -- an engine created with HX_CREATE_NO_SIDECAR, and the same engine under
HX_EXACT_SIDECAR=0 -- and that of the oracle-composed model (tests/exact_ref.py); the device counters are sound and the path really skips rows."""
import numpy as np
import pytest

import pgvector_rx_amd as hx
import exact_ref as ref

NOT_FOUND = 0xFFFFFFFF


def gmm(n, dim, rng, centres=16, spread=0.1):
    c = rng.standard_normal((centres, dim)).astype(np.float32)
    return (c[rng.integers(0, centres, n)] + spread * rng.standard_normal((n, dim))).astype(np.float32)


def adversarial(dim, rng):
    big = np.float32(np.finfo(np.float32).max / dim / 4)
    rows = [
        np.full(dim, 0.5, np.float32),                              # constant rows: step 0, e_x 0
        np.zeros(dim, np.float32),
        (rng.standard_normal(dim) * big).astype(np.float32),        # near FLT_MAX / dim
        (rng.random(dim) * np.float32(1e-40)).astype(np.float32),   # subnormals
        np.where(np.arange(dim) == dim // 2, np.float32(1e30), np.float32(0.25)).astype(np.float32),   # one huge coordinate
        (rng.random(dim) * 1e-20).astype(np.float32),
        np.full(dim, -3.0e38, np.float32),
        np.where(np.arange(dim) == 0, np.float32(np.inf), np.float32(0.5)).astype(np.float32),
        np.where(np.arange(dim) == dim - 1, np.float32(np.nan), np.float32(0.5)).astype(np.float32),
        np.where(np.arange(dim) == 3, np.float32(-np.inf), np.float32(0.1)).astype(np.float32),
    ]
    return np.stack(rows)


def engine(rows, qs, **kw):
    e = hx.Engine(kw.pop("dtype", hx.F32), kw.pop("metric", hx.L2SQ), rows.shape[1] if "dim" not in kw else kw.pop("dim"), len(rows), **kw)
    e.append(rows)
    e.set_queries(qs)
    return e


def same(a, b):
    return all(x.shape == y.shape and (np.ascontiguousarray(x).view(np.uint8) == np.ascontiguousarray(y).view(np.uint8)).all() for x, y in zip(a, b))


def wide_tile(dim):
    """16 queries of this width do not fit a query tile: 17 queries run in tiles of 4"""
    return 16 * ((dim * 4 + 15) // 16 * 16) > 65536


def three_ways(monkeypatch, e, e_no, call, expect_sidecar=True):
    """call(engine) on the sidecar engine (HX_EXACT_SIDECAR=1), on it with HX_EXACT_SIDECAR=0 and on the engine without a sidecar: all the
    same bits."""
    monkeypatch.setenv("HX_EXACT_SIDECAR", "1")                    # these inputs are below the sizes that take the path by default
    e.exact_sidecar_stats(reset=True)
    got = call(e)
    coded, _ = e.exact_sidecar_stats(reset=True)
    assert (coded > 0) == expect_sidecar
    monkeypatch.setenv("HX_EXACT_SIDECAR", "0")
    off = call(e)
    assert e.exact_sidecar_stats(reset=True) == (0, 0)
    monkeypatch.delenv("HX_EXACT_SIDECAR")
    e_no.exact_sidecar_stats(reset=True)
    plain = call(e_no)
    assert e_no.exact_sidecar_stats() == (0, 0)
    assert same(got, off) and same(got, plain)
    return got


def model_topk(rows, q, k, cand):
    return ref.topk(hx.F32, rows.shape[1], hx.OP_L2, q, rows[cand], k, ids=cand)


def check_topk(rows, qs, got, k, cand, first_query=0):
    ids, dist, cnt = got
    for qi in range(len(cnt)):
        want_ids, want_d = model_topk(rows, qs[first_query + qi], k, cand)
        c = int(cnt[qi])
        assert c == len(want_ids) == min(k, len(cand))
        assert ids[qi, :c].tolist() == want_ids.tolist(), qi
        assert ref.same_bits(dist[qi, :c], want_d), qi
        assert (ids[qi, c:] == NOT_FOUND).all() and np.isnan(dist[qi, c:]).all()


def model_range(rows, q, r, cmp, cand, ordered):
    v = ref.values(hx.F32, rows.shape[1], hx.OP_L2, q, rows[cand])
    nan = np.isnan(v)
    rn = np.isnan(r)
    with np.errstate(invalid="ignore"):                        # float8 comparison: NaN above everything, all NaNs equal
        lt = np.where(nan, False, True if rn else v < r)
        eq = np.where(nan, rn, False if rn else v == r)
    hit = {hx.CMP_LT: lt, hx.CMP_LE: lt | eq, hx.CMP_GT: ~(lt | eq), hx.CMP_GE: ~lt}[cmp]
    ids, v = cand[hit], v[hit]
    if ordered:
        o = ref.order(v, ids)
        ids, v = ids[o], v[o]
    return ids, v


def check_range(rows, qs, got, radius, cmp, cand, ordered=False, first_query=0):
    off, ids, dist = got
    radius = np.broadcast_to(np.asarray(radius, np.float64), (len(off) - 1,))
    for qi in range(len(off) - 1):
        want_ids, want_v = model_range(rows, qs[first_query + qi], radius[qi], cmp, cand, ordered)
        a, b = int(off[qi]), int(off[qi + 1])
        assert b - a == len(want_ids), (qi, b - a, len(want_ids))
        assert ids[a:b].tolist() == want_ids.tolist(), qi
        assert ref.same_bits(dist[a:b], want_v), qi


# ---- 1. parity with and without, 2. against the model ---------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("dim", [129, 130, 768, 1000, 2000])
def test_topk_parity_and_model(dim, monkeypatch):
    rng = np.random.default_rng(dim)
    n = 6000
    rows, qs = gmm(n, dim, rng), gmm(17, dim, rng)
    qs[2] = rows[4321]                                             # a duplicate of a row: distance 0
    e, e_no = engine(rows, qs), engine(rows, qs, sidecar=False)
    allr = np.arange(n)
    m10, m01 = rng.random(n) < 0.10, rng.random(n) < 0.001
    m01[17] = True
    sub = (1235, 3333)                                             # a sub-range with an odd first_row
    subm = rng.random(sub[1]) < 0.3
    for nq in (1, 3, 4, 5, 17):
        for k in (1, 10, 100, 1024):
            sc = nq < 16 or wide_tile(dim)                         # query tiles of 16 stay on the plain kernel
            for kw, cand in (({}, allr), ({"row_pass": m10}, allr[m10]), ({"row_pass": m01}, allr[m01]),
                             ({"first_row": sub[0], "n_rows": sub[1]}, allr[sub[0]:sub[0] + sub[1]]),
                             ({"first_row": sub[0], "n_rows": sub[1], "row_pass": subm}, allr[sub[0]:sub[0] + sub[1]][subm])):
                got = three_ways(monkeypatch, e, e_no, lambda en: en.exact_search(hx.OP_L2, k, first_query=17 - nq, nq=nq, **kw), sc)
                if dim in (129, 768) and nq in (1, 5) and k in (10, 1024):
                    check_topk(rows, qs, got, k, cand, first_query=17 - nq)
    assert same(got, e.exact_search(hx.OP_L2, 1024, nq=17, first_row=sub[0], n_rows=sub[1], row_pass=subm))
    assert e.exact_sidecar_stats() == (0, 0)                        # unset: a call of this size stays on the plain kernel
    monkeypatch.setenv("HX_EXACT_SIDECAR", "1")
    full = e.exact_search(hx.OP_L2, 100, nq=17)
    few = e.exact_search(hx.OP_L2, 100, nq=5)
    monkeypatch.setenv("HX_EXACT_SCRATCH", str(1 << 18))           # query blocks
    assert same(full, e.exact_search(hx.OP_L2, 100, nq=17)) and same(few, e.exact_search(hx.OP_L2, 100, nq=5))
    assert same(few, e_no.exact_search(hx.OP_L2, 100, nq=5))
    e.close()
    e_no.close()


@pytest.mark.gpu
@pytest.mark.parametrize("dim", [129, 130, 768, 1000, 2000])
def test_range_parity_and_model(dim, monkeypatch):
    rng = np.random.default_rng(1000 + dim)
    n = 6000
    rows, qs = gmm(n, dim, rng), gmm(17, dim, rng)
    qs[2] = rows[4321]
    e, e_no = engine(rows, qs), engine(rows, qs, sidecar=False)
    allr = np.arange(n)
    m10 = rng.random(n) < 0.10
    _, d, _ = e_no.exact_search(hx.OP_L2, 400, nq=17)
    for nq in (1, 3, 4, 5, 17):
        for hits in (1, 30, 400):
            r = d[17 - nq:, hits - 1].copy()                       # the hits-th value itself: `<` and `<=` differ by the ties
            for cmp in (hx.CMP_LT, hx.CMP_LE, hx.CMP_GT, hx.CMP_GE):
                sc = (nq < 16 or wide_tile(dim)) and cmp in (hx.CMP_LT, hx.CMP_LE)
                if cmp in (hx.CMP_GT, hx.CMP_GE) and (hits != 30 or nq not in (1, 4)):
                    continue                                       # the plain path: a sample only (its hits are nearly all rows)
                for kw, cand in (({}, allr), ({"row_pass": m10}, allr[m10]), ({"first_row": 1235, "n_rows": 3333}, allr[1235:1235 + 3333])):
                    for mode in ({}, {"ordered": True}, {"count_only": True}):
                        got = three_ways(monkeypatch, e, e_no, lambda en: en.exact_range(hx.OP_L2, r, cmp=cmp, first_query=17 - nq, nq=nq, **kw, **mode), sc)
                        if dim in (129, 768) and nq in (1, 5) and hits == 30 and "count_only" not in mode:
                            check_range(rows, qs, got, r, cmp, cand, ordered="ordered" in mode, first_query=17 - nq)
    r = d[:, 399].copy()
    monkeypatch.setenv("HX_EXACT_SIDECAR", "1")
    full = [e.exact_range(hx.OP_L2, r[:nq], cmp=hx.CMP_LE, nq=nq, ordered=o) for nq in (4, 17) for o in (False, True)]
    monkeypatch.setenv("HX_RANGE_SCRATCH", str(1 << 20))           # windows and the overflow re-scan
    e.exact_sidecar_stats(reset=True)
    small = [e.exact_range(hx.OP_L2, r[:nq], cmp=hx.CMP_LE, nq=nq, ordered=o) for nq in (4, 17) for o in (False, True)]
    assert e.exact_sidecar_stats()[0] > 0
    small_no = [e_no.exact_range(hx.OP_L2, r[:nq], cmp=hx.CMP_LE, nq=nq, ordered=o) for nq in (4, 17) for o in (False, True)]
    assert all(same(a, b) and same(a, c) for a, b, c in zip(full, small, small_no))
    big = e.exact_range(hx.OP_L2, np.inf, cmp=hx.CMP_LT, nq=3)    # every finite row of three queries through 1 MiB: overflowed segments
    assert same(big, e_no.exact_range(hx.OP_L2, np.inf, cmp=hx.CMP_LT, nq=3)) and int(big[0][-1]) == 3 * n
    e.close()
    e_no.close()


# ---- 3. adversarial rows --------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("dim", [129, 768, 2000])
def test_adversarial_rows(dim, monkeypatch):
    rng = np.random.default_rng(3000 + dim)
    base = gmm(1500, dim, rng)
    adv = adversarial(dim, rng)
    rows = np.concatenate([base[:700], adv, np.repeat(base[700:701], 64, 0), base[701:], adv])
    n = len(rows)
    qs = np.concatenate([rows[:2], adv[:7], rows[720:721], (rows[5:7] + 1e-3).astype(np.float32)])   # slot 9: 64 duplicates of the query
    nq = len(qs)
    e, e_no = engine(rows, qs), engine(rows, qs, sidecar=False)
    cand = np.arange(n)
    for k in (1, 10, 100, 1024):
        for q0, m in ((0, 1), (0, 4), (4, 4), (8, 4), (9, 1)):
            got = three_ways(monkeypatch, e, e_no, lambda en: en.exact_search(hx.OP_L2, k, first_query=q0, nq=m))
            if k in (10, 1024):
                check_topk(rows, qs, got, k, cand, first_query=q0)
    ids, d, _ = e.exact_search(hx.OP_L2, 100, first_query=9, nq=1)
    assert ids[0, :64].tolist() == list(range(710, 774)) and (d[0, :64] == 0).all()
    few = np.zeros(n, bool)
    few[[3, 705, 708, 1000, n - 1]] = True                          # k larger than the number of passing rows
    got = three_ways(monkeypatch, e, e_no, lambda en: en.exact_search(hx.OP_L2, 10, nq=4, row_pass=few))
    check_topk(rows, qs, got, 10, cand[few])
    assert (got[2] == 5).all()
    for r in (0.0, -0.0, np.inf, np.nan, -1.0, 1e-30, float(d[0, 70])):
        for cmp in (hx.CMP_LT, hx.CMP_LE, hx.CMP_GT, hx.CMP_GE):
            for q0, m in ((0, 4), (8, 4), (9, 1)):
                sc = cmp in (hx.CMP_LT, hx.CMP_LE)
                got = three_ways(monkeypatch, e, e_no, lambda en: en.exact_range(hx.OP_L2, r, cmp=cmp, first_query=q0, nq=m), sc)
                check_range(rows, qs, got, r, cmp, cand, first_query=q0)
                cnt = three_ways(monkeypatch, e, e_no, lambda en: en.exact_range(hx.OP_L2, r, cmp=cmp, first_query=q0, nq=m, count_only=True), sc)
                assert (cnt[0] == got[0]).all()
    e.close()
    e_no.close()
    # all rows identical: every distance ties, only the row id orders them
    rows = np.repeat(gmm(1, dim, rng), 3000, 0)
    qs = np.concatenate([rows[:1], gmm(3, dim, rng)])
    e, e_no = engine(rows, qs), engine(rows, qs, sidecar=False)
    for k in (1, 10, 1024):
        got = three_ways(monkeypatch, e, e_no, lambda en: en.exact_search(hx.OP_L2, k, nq=4))
        assert (got[0] == np.arange(k)[None, :]).all() and (got[1][0] == 0).all()
    got = three_ways(monkeypatch, e, e_no, lambda en: en.exact_range(hx.OP_L2, 0.0, cmp=hx.CMP_LE, nq=4))
    assert got[0].tolist() == [0, 3000, 3000, 3000, 3000] and got[1].tolist() == list(range(3000))
    e.close()
    e_no.close()


# ---- 4. the counters are sound and the feature is real --------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def clustered():
    rng = np.random.default_rng(2024)
    n, dim, nc = 200_000, 768, 100
    centres = rng.standard_normal((nc, dim)).astype(np.float32)   # centres about 39 apart, members about 3.9 from one another
    label = rng.permutation(np.arange(n) % nc)                     # rows shuffled
    rows = centres[label] + np.float32(0.1) * rng.standard_normal((n, dim), dtype=np.float32)
    qs = (centres[[7, 23, 51, 88]] + np.float32(0.1) * rng.standard_normal((4, dim), dtype=np.float32)).astype(np.float32)
    e = engine(rows, qs)
    yield e, rows, qs, n
    e.close()


def bounds(e, nq, n):
    ids = np.arange(n, dtype=np.uint32)
    return [e.sidecar_bounds(hx.QUERY_SLOT | q, ids) for q in range(nq)]


@pytest.mark.gpu
@pytest.mark.parametrize("nq", [1, 4])
def test_counters_topk(clustered, nq, monkeypatch):
    monkeypatch.delenv("HX_EXACT_SIDECAR", raising=False)
    e, rows, qs, n = clustered
    e.exact_sidecar_stats(reset=True)
    ids, d, cnt = e.exact_search(hx.OP_L2, 10, nq=nq)
    coded, fetched = e.exact_sidecar_stats(reset=True)
    must = np.zeros(n, bool)
    for q, lb in enumerate(bounds(e, nq, n)):
        kth = e.distances(qs[q], ids[q, 9:10])[0]                  # the final k-th squared distance, f32 bits
        must |= (lb == 0) | (lb <= kth)
    must = int(must.sum())
    print("top-k nq %d: rows_coded %d rows_fetched %d must %d" % (nq, coded, fetched, must))
    assert must <= n // 20                                          # precondition: the fixture leaves a tenfold margin
    assert coded == n                                               # one query tile
    assert must <= fetched                                          # by the rule none of these may be skipped
    assert fetched <= coded // 2
    check_topk(rows, qs, (ids, d, cnt), 10, np.arange(n))


@pytest.mark.gpu
def test_counters_range(clustered, monkeypatch):
    monkeypatch.delenv("HX_EXACT_SIDECAR", raising=False)
    e, rows, qs, n = clustered
    r = 8.0                                                         # admits only rows of the query's cluster
    e.exact_sidecar_stats(reset=True)
    off, ids, d = e.exact_range(hx.OP_L2, r, cmp=hx.CMP_LT, nq=1)
    coded, fetched = e.exact_sidecar_stats(reset=True)
    lb = bounds(e, 1, n)[0]
    must = int(((lb == 0) | (np.sqrt(lb.astype(np.float64)) < r)).sum())
    print("range: rows_coded %d rows_fetched %d must %d hits %d" % (coded, fetched, must, int(off[1])))
    assert must <= n // 20
    assert coded == n and must <= fetched <= coded // 2
    assert int(off[1]) == n // 100
    check_range(rows, qs, (off, ids, d), r, hx.CMP_LT, np.arange(n))


# ---- 5. engines and operators without a sidecar path ----------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_no_sidecar_cases_stay_plain(monkeypatch):
    monkeypatch.setenv("HX_EXACT_SIDECAR", "1")                    # even when asked for at every size
    rng = np.random.default_rng(55)
    n = 3000
    rows, qs = gmm(n, 128, rng), gmm(4, 128, rng)
    e = engine(rows, qs)                                            # 128 dimensions: no sidecar
    check_topk(rows, qs, e.exact_search(hx.OP_L2, 10), 10, np.arange(n))
    check_range(rows, qs, e.exact_range(hx.OP_L2, 3.0), 3.0, hx.CMP_LT, np.arange(n))
    assert e.exact_sidecar_stats() == (0, 0)
    e.close()
    rows, qs = gmm(n, 300, rng), gmm(4, 300, rng)
    e = engine(rows, qs)                                            # a sidecar engine, other operators
    for op in (hx.OP_COSINE, hx.OP_L1, hx.OP_NEG_IP):
        ids, d, cnt = e.exact_search(op, 10)
        off, rid, rd = e.exact_range(op, float(d[0, 5]), cmp=hx.CMP_LE, nq=1)
        for q in range(4):
            w_ids, w_d = ref.topk(hx.F32, 300, op, qs[q], rows, 10)
            assert ids[q].tolist() == w_ids.tolist() and ref.same_bits(d[q], w_d)
        v = ref.values(hx.F32, 300, op, qs[0], rows)
        assert rid.tolist() == np.nonzero(v <= d[0, 5])[0].tolist()
    assert e.exact_sidecar_stats() == (0, 0)
    e.close()
    h = rng.standard_normal((n, 300)).astype(np.float16).view(np.uint16)
    hq = rng.standard_normal((4, 300)).astype(np.float16).view(np.uint16)
    e = engine(h, hq, dtype=hx.F16)                                 # halfvec
    ids, d, _ = e.exact_search(hx.OP_L2, 10)
    for q in range(4):
        w_ids, w_d = ref.topk(hx.F16, 300, hx.OP_L2, hq[q], h, 10)
        assert ids[q].tolist() == w_ids.tolist() and ref.same_bits(d[q], w_d)
    assert e.exact_sidecar_stats() == (0, 0)
    e.close()
    rows, qs = gmm(500, 3072, rng), gmm(4, 3072, rng)
    e = engine(rows, qs, scan_only=True)                            # scan-only without the flag: what it is today
    check_topk(rows, qs, e.exact_search(hx.OP_L2, 10), 10, np.arange(500))
    assert e.exact_sidecar_stats() == (0, 0)
    with pytest.raises(hx.HxError):
        e.sidecar_read(0, 1)
    e.close()


# ---- 6. wide scan-only engines with HX_CREATE_SCAN_SIDECAR ----------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("dim", [3072, 16000])
def test_wide_scan_sidecar(dim, monkeypatch):
    rng = np.random.default_rng(dim)
    adv = adversarial(dim, rng)
    rows = np.concatenate([gmm(2500, dim, rng), adv])
    n = len(rows)
    qs = np.concatenate([gmm(3, dim, rng), adv[:4], (rows[3:5] + 1e-3).astype(np.float32)])
    nq = len(qs)
    e, e_no = engine(rows, qs, scan_only=True, scan_sidecar=True), engine(rows, qs, scan_only=True)
    ids = np.arange(n, dtype=np.uint32)
    useful = 0
    for q in range(nq):
        lb = e.sidecar_bounds(hx.QUERY_SLOT | q, ids)
        d = e.distances(qs[q], ids)
        assert np.all(np.isfinite(lb)) and np.all(lb >= 0)
        ok = (lb <= d) | np.isnan(d)
        assert ok.all(), (q, np.nonzero(~ok)[0][:5], lb[~ok][:5], d[~ok][:5])
        assert np.all(lb[np.isnan(d)] == 0)
        useful += int((lb[:2500] > 0.5 * d[:2500]).sum())
    assert useful > 2500
    codes, meta = e.sidecar_read(0, n)
    xh = (meta[:, 0:1].astype(np.float64) + meta[:, 1:2].astype(np.float64) * codes).astype(np.float32)
    with np.errstate(all="ignore"):
        err = np.sqrt(((rows.astype(np.float64) - xh.astype(np.float64)) ** 2).sum(1))
    fin = np.isfinite(meta[:, 2])
    assert np.all(meta[fin, 2] >= err[fin]) and fin[:2500].all()
    for k in (10, 1024):
        for q0, m in ((0, 1), (0, 3), (0, 4), (5, 4)):
            three_ways(monkeypatch, e, e_no, lambda en: en.exact_search(hx.OP_L2, k, first_query=q0, nq=m))
    check_topk(rows, qs, e.exact_search(hx.OP_L2, 10, nq=3), 10, np.arange(n))
    _, d, _ = e_no.exact_search(hx.OP_L2, 50, nq=nq)
    for cmp in (hx.CMP_LT, hx.CMP_LE, hx.CMP_GE):
        for m in (1, 3, 4):
            for mode in ({}, {"ordered": True}, {"count_only": True}):
                three_ways(monkeypatch, e, e_no, lambda en: en.exact_range(hx.OP_L2, d[:m, 49].copy(), cmp=cmp, nq=m, **mode), cmp != hx.CMP_GE)
    lists = [rng.integers(0, n, 300) for _ in range(nq)]            # the re-rank and the halfvec casts behave as before
    assert same(e.exact_rerank(hx.OP_L2, lists, 10), e_no.exact_rerank(hx.OP_L2, lists, 10))
    fine = np.concatenate([np.arange(2500), [2500, 2501]])          # rows a half can hold
    ha, hb = (hx.Engine(hx.F16, hx.L2SQ, dim, n, scan_only=True) for _ in range(2))
    for h, src in ((ha, e), (hb, e_no)):
        h.append_halfvec_from(src, 0, 2502)
        h.set_queries_halfvec_from(engine(rows[:1], qs[:3], scan_only=True))
    assert (ha.read_rows(0, 2502) == hb.read_rows(0, 2502)).all() and len(fine) == 2502
    assert same(ha.exact_search(hx.OP_L2, 10), hb.exact_search(hx.OP_L2, 10))
    e.pop(5)                                                        # row writers keep the sidecar in step
    e.append(rows[-5:])
    c2, m2 = e.sidecar_read(0, n)
    assert (c2 == codes).all() and (m2.view(np.uint32) == meta.view(np.uint32)).all()
    for x in (e, e_no, ha, hb):
        x.close()


# ---- 7. while an index scan is in flight ----------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_while_index_scan_in_flight(monkeypatch):
    monkeypatch.setenv("HX_EXACT_SIDECAR", "1")
    rng = np.random.default_rng(77)
    n, dim = 4000, 160
    rows, qs = gmm(n, dim, rng), gmm(16, dim, rng)
    e = engine(rows, qs)
    ix = hx.Index(e, 8, 32)
    ix.insert(0, hx.draw_levels(n, 8, seed=9), batch=256)
    alone = ix.search(16, 40, 10)
    e.exact_sidecar_stats(reset=True)
    ex = e.exact_search(hx.OP_L2, 10, nq=4)
    rg = e.exact_range(hx.OP_L2, 2.0, cmp=hx.CMP_LT, nq=4)
    rgo = e.exact_range(hx.OP_L2, 2.0, cmp=hx.CMP_LE, nq=4, ordered=True)
    assert e.exact_sidecar_stats()[0] == 3 * n
    ix.search_submit(0, 0, 16, 40, 10)
    during = e.exact_search(hx.OP_L2, 10, nq=4) + e.exact_range(hx.OP_L2, 2.0, cmp=hx.CMP_LT, nq=4) + e.exact_range(hx.OP_L2, 2.0, cmp=hx.CMP_LE, nq=4, ordered=True)
    waited = ix.search_wait(0)
    assert same(ex + rg + rgo, during)
    assert all((a == b).all() for a, b in zip(alone, waited))
    check_topk(rows, qs, ex, 10, np.arange(n))
    ix.close()
    e.close()
