"""hx_exact_search_filtered: exact k-NN scans with a WHERE filter per query in one call.  The oracle is the definition: for every query the ids,
distance bits and counts equal, byte for byte, what hx_exact_search returns for that query alone with its filter (on the same engine); a handful
of queries per case are also compared with the CPU oracle of tests/exact_ref.py."""
import ctypes

import numpy as np
import pytest

import pgvector_rx_amd as hx
import exact_ref as ref

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


def engine(dtype, dim, op, rows, queries, **kw):
    e = hx.Engine(dtype, METRIC_OF[op] if dtype == hx.BIT else hx.L2SQ, dim, len(rows), **kw)
    e.append(rows)
    e.set_queries(queries)
    return e


def same(a, b):
    return all(x.shape == y.shape and (x.view(np.uint8) == y.view(np.uint8)).all() for x, y in zip(a, b))


def one_by_one(e, op, k, masks, filter_of, first_query=0, first_row=0, n_rows=None):
    """The definition: one hx_exact_search call per query with that query's filter."""
    out = [e.exact_search(op, k, first_query=first_query + i, nq=1, first_row=first_row, n_rows=n_rows, row_pass=None if f < 0 else masks[f])
           for i, f in enumerate(filter_of)]
    return tuple(np.concatenate([o[j] for o in out]) for j in range(3))


def check(e, op, k, masks, filter_of, first_query=0, first_row=0, n_rows=None, cpu=None):
    """Runs the grouped call and requires the bytes of the per-query calls.  cpu = (dtype, dim, rows, queries, picks, norms): also the CPU oracle
    for the queries in `picks`."""
    got = e.exact_search_filtered(op, k, masks, filter_of, first_query=first_query, nq=len(filter_of), first_row=first_row, n_rows=n_rows)
    want = one_by_one(e, op, k, masks, filter_of, first_query, first_row, n_rows)
    for j, name in enumerate(("ids", "dist", "counts")):
        assert (got[j].view(np.uint8) == want[j].view(np.uint8)).all(), (op, name, np.nonzero((got[j].view(np.uint8) != want[j].view(np.uint8)).reshape(len(filter_of), -1).any(1))[0])
    if cpu:
        dtype, dim, rows, queries, picks, norms = cpu
        n = (len(rows) - first_row) if n_rows is None else n_rows
        for i in picks:
            cand = np.arange(first_row, first_row + n)
            if filter_of[i] >= 0:
                cand = cand[np.asarray(masks[filter_of[i]], bool)]
            w_ids, w_d = ref.topk(dtype, dim, op, queries[first_query + i], rows[cand], k, ids=cand, row_norms=None if norms is None else norms[cand])
            c = int(got[2][i])
            assert c == len(w_ids) == min(k, len(cand))
            assert got[0][i, :c].tolist() == w_ids.tolist() and ref.same_bits(got[1][i, :c], w_d), (op, i)
            assert (got[0][i, c:] == NOT_FOUND).all() and np.isnan(got[1][i, c:]).all()
    return got


def interleaved(sizes, n_unfiltered, rng):
    """filter_of with sizes[f] queries of filter f and n_unfiltered of -1, shuffled so that the queries of a group are not adjacent."""
    fo = np.concatenate([np.full(s, f, np.int32) for f, s in enumerate(sizes)] + [np.full(n_unfiltered, -1, np.int32)])
    return rng.permutation(fo)


# ---- 1. parity matrix -----------------------------------------------------------------------------------------------------------------------
CASES = [(hx.F32, d) for d in (3, 100, 768, 2000)] + [(hx.F16, 10), (hx.F16, 4000), (hx.BIT, 8), (hx.BIT, 1024), (hx.SPARSE, 100)]


@pytest.mark.gpu
@pytest.mark.parametrize("dtype,dim", CASES, ids=lambda v: str(v))
def test_parity_matrix(dtype, dim):
    """26 queries over 4 filters in groups of 1, 3, 5 and 17 (tiles of 16 + 1, 4 + 1, a partial tile of 4 and a tile of 1) and 3 unfiltered ones."""
    rng = np.random.default_rng(70 + dim + 10 * dtype)
    n = 1500 if dim <= 1536 else 700
    fo = interleaved([1, 3, 5, 17], 3, rng)
    rows, qs = make(dtype, n, dim, rng), make(dtype, len(fo), dim, rng)
    masks = [rng.random(n) < p for p in (0.5, 0.1, 0.3, 0.02)]
    picks = [int(np.nonzero(fo == f)[0][-1]) for f in (-1, 0, 3)]
    norms = None
    for op in (BOPS if dtype == hx.BIT else FOPS):
        e = engine(dtype, dim, op, rows, qs)
        if op == hx.OP_COSINE and dtype != hx.SPARSE:
            norms = ref.self_ip(dtype, dim, rows)
        check(e, op, 10, masks, fo, cpu=(dtype, dim, rows, qs, picks, norms if op == hx.OP_COSINE else None))
        e.close()


# ---- 2. filter edge cases -------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("dim", [16, 768])
def test_filter_edge_cases(dim):
    rng = np.random.default_rng(dim)
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
    for k in (1, 10, 1024):
        ids, d, cnt = check(e, hx.OP_L2, k, masks, fo, first_query=2, first_row=17, n_rows=n, cpu=cpu if k == 10 else None)
        assert cnt[0] == cnt[7] == 0 and (ids[0] == NOT_FOUND).all() and np.isnan(d[0]).all()
        assert cnt[1] == 1 and ids[1, 0] == 17 + 777 and cnt[2] == min(k, 5) and cnt[3] == min(k, n)
    # packed words with garbage bits past n_rows in the last word: ignored
    words = []
    for m in masks:
        if m is None:
            words.append(None)
            continue
        bits = np.ones(((n + 63) // 64) * 64, np.uint8)
        bits[:n] = m
        words.append(np.packbits(bits, bitorder="little").view(np.uint64))
    got = e.exact_search_filtered(hx.OP_L2, 10, words, fo, first_query=2, nq=len(fo), first_row=17, n_rows=n, packed=True)
    assert same(got, one_by_one(e, hx.OP_L2, 10, masks, fo, 2, 17, n))
    # every query's filter is empty, beside unreferenced ones: answered without a scan
    ids, d, cnt = e.exact_search_filtered(hx.OP_L2, 10, [empty, None, np.zeros(n, bool)], [0, 2, 0], nq=3, n_rows=n)
    assert (cnt == 0).all() and (ids == NOT_FOUND).all() and np.isnan(d).all()
    e.close()


# ---- 3. slices ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_slices_of_very_unequal_groups():
    """One group whose list is shorter than one round beside one that spans many slices; 5 rows against 4000."""
    rng = np.random.default_rng(31)
    n = 5000
    rows, qs = make(hx.F32, n, 64, rng), make(hx.F32, 12, 64, rng)
    e = engine(hx.F32, 64, hx.OP_L2, rows, qs)
    tiny, big, mid = np.zeros(n, bool), np.zeros(n, bool), rng.random(n) < 0.2
    tiny[[4, 1000, 2500, 4001, 4999]] = True
    big[rng.permutation(n)[:4000]] = True
    check(e, hx.OP_L2, 10, [tiny, big, mid], np.array([0, 1, 2, 1, 0, -1, 1, 1, 2, 1, 0, 1], np.int32), cpu=(hx.F32, 64, rows, qs, [0, 1, 2, 5], None))
    check(e, hx.OP_L2, 10, [tiny, big], np.array([0, 1], np.int32))
    e.close()


# ---- 4. query blocks ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_query_blocks(monkeypatch):
    """A scratch budget smaller than all queries' buffers: groups are split across query blocks, the bytes stay the same."""
    rng = np.random.default_rng(41)
    n = 3000
    fo = interleaved([20, 19, 14, 5], 6, rng)
    assert len(fo) == 64
    rows, qs = make(hx.F32, n, 64, rng), make(hx.F32, 64, 64, rng)
    e = engine(hx.F32, 64, hx.OP_L2, rows, qs)
    masks = [rng.random(n) < p for p in (0.6, 0.3, 0.9, 0.05)]
    full = check(e, hx.OP_L2, 100, masks, fo, cpu=(hx.F32, 64, rows, qs, [0, 1, 2], None))
    monkeypatch.setenv("HX_EXACT_SCRATCH", str(1 << 20))
    e.set_timing(True)
    e.kernel_stats(7, reset=True)
    got = e.exact_search_filtered(hx.OP_L2, 100, masks, fo)
    assert e.kernel_stats(7)["launches"] > 5               # more than one block ran
    assert same(full, got)
    e.close()


# ---- 5. ties and special values -------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_ties_and_special_values():
    rng = np.random.default_rng(51)
    # 64 copies of one row spread over two overlapping filters: equal distances come back by row id
    base = make(hx.F32, 300, 24, rng)
    rows = np.concatenate([base[:100], np.repeat(base[100:101], 64, 0), base[101:]])
    n = len(rows)
    qs = make(hx.F32, 5, 24, rng)
    qs[1] = qs[3] = rows[120]
    a, b = np.zeros(n, bool), np.zeros(n, bool)
    a[:140], b[120:] = True, True
    e = engine(hx.F32, 24, hx.OP_L2, rows, qs)
    ids, d, _ = check(e, hx.OP_L2, 100, [a, b], np.array([0, 0, 1, 1, -1], np.int32), cpu=(hx.F32, 24, rows, qs, [1, 3], None))
    assert ids[1, :40].tolist() == list(range(100, 140)) and ids[3, :44].tolist() == list(range(120, 164)) and (d[1, :40] == 0).all()
    e.close()
    # rows with NaN and +-inf elements
    rows = make(hx.F32, 400, 8, rng)
    rows[5, 3], rows[50, 0], rows[51, 0], rows[300, 7] = np.nan, np.inf, -np.inf, np.nan
    qs = make(hx.F32, 6, 8, rng)
    masks = [np.arange(400) % 2 == 0, np.arange(400) % 2 == 1, np.arange(400) < 100]
    fo = np.array([0, 1, 2, 0, 1, -1], np.int32)
    for op in FOPS:
        e = engine(hx.F32, 8, op, rows, qs)
        ids, d, cnt = check(e, op, 200, masks, fo)
        assert cnt[1] == 200 and np.isnan(d[1, 199]) and ids[1, 199] == (51 if op == hx.OP_COSINE else 5)   # NaN last (<=>: inf / inf too), by id
        e.close()
    # <#> with a zero product: -0.0 keeps its sign and ties with +0.0 by id; <=> with a zero vector: NaN, last, by id
    rows = make(hx.F32, 100, 4, rng)
    rows[::3, 0] = 0
    qs = np.array([[1, 0, 0, 0], [1, 0, 0, 0], [0, 0, 0, 0]], np.float32)
    masks = [np.arange(100) < 50, np.arange(100) >= 30]
    e = engine(hx.F32, 4, hx.OP_NEG_IP, rows, qs)
    ids, d, cnt = check(e, hx.OP_NEG_IP, 100, masks, np.array([0, 1, 1], np.int32), cpu=(hx.F32, 4, rows, qs, [0, 1], None))
    z = d[0, :cnt[0]] == 0
    assert z.sum() == 17 and np.signbit(d[0, :cnt[0]][z]).all() and ids[0, :cnt[0]][z].tolist() == list(range(0, 50, 3))
    ids, d, cnt = check(e, hx.OP_COSINE, 100, masks, np.array([0, 1, 1], np.int32))
    assert np.isnan(d[2, :70]).all() and ids[2, :70].tolist() == list(range(30, 100))
    e.close()


# ---- 6. sidecar engine ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_sidecar_engine(monkeypatch):
    rng = np.random.default_rng(61)
    n, dim = 1500, 768
    rows, qs = make(hx.F32, n, dim, rng), make(hx.F32, 6, dim, rng)
    masks = [rng.random(n) < 0.5, rng.random(n) < 0.2, np.zeros(n, bool)]
    masks[2][rng.permutation(n)[:60]] = True
    fo = np.array([0, 1, 0, -1, 1, 0], np.int32)
    e, plain = engine(hx.F32, dim, hx.OP_L2, rows, qs), engine(hx.F32, dim, hx.OP_L2, rows, qs, sidecar=False)
    monkeypatch.setenv("HX_EXACT_SIDECAR", "1")            # the scan with one filter would take the sidecar at every size
    e.exact_sidecar_stats(reset=True)
    got = e.exact_search_filtered(hx.OP_L2, 10, masks, fo)
    assert e.exact_sidecar_stats() == (0, 0)               # two or more distinct filters: the grouped path, no sidecar
    assert same(got, plain.exact_search_filtered(hx.OP_L2, 10, masks, fo))
    assert same(got, one_by_one(plain, hx.OP_L2, 10, masks, fo))
    # one distinct filter: the call is hx_exact_search with that bitmap, counters included (60 passing rows: one slice, so they are reproducible)
    e.set_timing(True)
    for m, f in ((masks, np.array([2, 2, 2], np.int32)), ([None, None], np.array([-1, -1, -1], np.int32))):
        e.exact_sidecar_stats(reset=True)
        e.kernel_stats(7, reset=True)
        want = e.exact_search(hx.OP_L2, 5, nq=3, n_rows=None if f[0] >= 0 else 60, row_pass=masks[2] if f[0] >= 0 else None)
        sc_want, ks_want = e.exact_sidecar_stats(reset=True), e.kernel_stats(7, reset=True)
        got = e.exact_search_filtered(hx.OP_L2, 5, m, f, nq=3, n_rows=None if f[0] >= 0 else 60)
        sc_got, ks_got = e.exact_sidecar_stats(reset=True), e.kernel_stats(7, reset=True)
        assert same(got, want)
        assert sc_want[0] > 0 and sc_got == sc_want
        assert (ks_got["launches"], ks_got["units"]) == (ks_want["launches"], ks_want["units"])
    e.close()
    plain.close()


# ---- 7. launch count ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_launch_count_does_not_grow_with_the_filters():
    rng = np.random.default_rng(71)
    n = 1500
    rows, qs = make(hx.F32, n, 16, rng), make(hx.F32, 64, 16, rng)
    e = engine(hx.F32, 16, hx.OP_L2, rows, qs)
    masks = [rng.random(n) < 0.05 + 0.01 * f for f in range(64)]
    e.set_timing(True)
    counts = {}
    for nf in (8, 64):
        e.kernel_stats(7, reset=True)
        got = e.exact_search_filtered(hx.OP_L2, 10, masks[:nf], np.arange(nf, dtype=np.int32), nq=nf)
        st = e.kernel_stats(7, reset=True)
        counts[nf] = st["launches"]
        assert st["units"] == sum(int(m.sum()) for m in masks[:nf]) and st["ms"] > 0
    assert counts[64] <= 5 and counts[8] == counts[64]     # one compaction, at most three scans, one merge
    want = one_by_one(e, hx.OP_L2, 10, masks, np.arange(64))
    assert e.kernel_stats(7)["launches"] == 192            # what the 64 separate calls cost
    assert same(got, want)
    e.close()


# ---- 8. argument errors ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_argument_errors():
    rng = np.random.default_rng(81)
    rows, qs = make(hx.F32, 100, 8, rng), make(hx.F32, 4, 8, rng)
    e = engine(hx.F32, 8, hx.OP_L2, rows, qs)
    L = hx.lib()
    ids, d, c = np.full(4 * 1024, 7, np.uint32), np.full(4 * 1024, 7.0, np.float64), np.full(4, 7, np.uint32)
    P = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    words = [np.full(2, 0x5555555555555555, np.uint64), np.full(2, 0x3333333333333333, np.uint64)]
    two = (ctypes.c_void_p * 2)(words[0].ctypes.data, words[1].ctypes.data)
    many = (ctypes.c_void_p * 65)(*[words[0].ctypes.data] * 65)
    holed = (ctypes.c_void_p * 2)(words[0].ctypes.data, None)

    def call(op=hx.OP_L2, fq=0, nq=4, fr=0, nr=100, nf=2, filters=two, fo=(0, 1, -1, 0), k=10, outs=True):
        of = None if fo is None else np.array(fo, np.int32)
        return L.hx_exact_search_filtered(e.h, op, fq, nq, fr, nr, nf, filters, None if of is None else P(of), k, P(ids) if outs else None, P(d), P(c))

    def is_error(**kw):
        """HX_E_ARG with a message and the outputs untouched -> the message"""
        ids[:], d[:], c[:] = 7, 7.0, 7
        rc = call(**kw)
        msg = L.hx_last_error(e.h)
        return rc == -1 and (ids == 7).all() and (d == 7.0).all() and (c == 7).all() and msg

    assert call() == 0 and call(fo=None) == 0 and call(nf=0, filters=None, fo=(-1, -1, -1, -1)) == 0
    assert call(filters=holed, fo=(0, 0, -1, 0)) == 0                            # an unreferenced NULL filter is accepted
    m65 = is_error(nf=65, filters=many)
    assert m65 and b"HX_EXACT_MAX_FILTERS" in m65
    assert call(nf=64, filters=many) == 0
    for kw in (dict(fo=(0, 2, -1, 0)), dict(fo=(0, -2, -1, 0)), dict(filters=None), dict(filters=holed), dict(nf=0, filters=None, fo=(0, -1, -1, -1))):
        r = is_error(**kw)
        assert r and b"filter" in r, kw
    # everything hx_exact_search rejects, with its messages
    for kw, text in ((dict(op=hx.OP_HAMMING), b"operator"), (dict(op=6), b"operator"), (dict(op=-1), b"operator"), (dict(k=0), b"k must"), (dict(k=1025), b"k must"),
                     (dict(fr=50, nr=51), b"row range"), (dict(fr=101, nr=0), b"row range"), (dict(fr=2 ** 32, nr=0), b"row range"),
                     (dict(fq=1, nq=4), b"query range"), (dict(nq=5, fo=(0, 1, -1, 0, 0)), b"query range"), (dict(outs=False), b"NULL output")):
        r = is_error(**kw)
        assert r and text in r, kw
        ids[:], d[:], c[:] = 7, 7.0, 7
        kw1 = {a: b for a, b in kw.items() if a != "fo"}
        rc = L.hx_exact_search(e.h, kw1.get("op", hx.OP_L2), kw1.get("fq", 0), kw1.get("nq", 4), kw1.get("fr", 0), kw1.get("nr", 100), None, kw1.get("k", 10),
                               P(ids) if kw1.get("outs", True) else None, P(d), P(c))
        assert rc == -1 and L.hx_last_error(e.h) == r                         # the same message
    assert call(k=1024) == 0
    with pytest.raises(hx.HxError):
        e.exact_search_filtered(hx.OP_L2, 5, [np.ones(100, bool)], [0, 1, 0, 0])
    e.close()


# ---- 9. scan-only wide engine ---------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_scan_only_wide_engine():
    rng = np.random.default_rng(91)
    n, dim = 300, 3072
    rows, qs = make(hx.F32, n, dim, rng), make(hx.F32, 6, dim, rng)
    e = engine(hx.F32, dim, hx.OP_L2, rows, qs, scan_only=True)
    masks = [rng.random(n) < p for p in (0.5, 0.3, 0.1)]
    fo = np.array([0, 1, 0, 2, 1, 0], np.int32)
    for op in FOPS:
        check(e, op, 10, masks, fo, cpu=(hx.F32, dim, rows, qs, [0, 3], None) if op == hx.OP_L2 else None)
    e.close()
