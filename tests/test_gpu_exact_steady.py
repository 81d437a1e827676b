"""The exact top-k scans in their steady state, per instantiation: hx_exact_search, hx_exact_search_filtered and hx_exact_search_set on the calls
of tests/exact_steady_cases.py -- long slices, where nearly every row is compared against a live threshold and the candidate buffers are cut back
to k inside the round loop, and merges that filter against their own threshold (tests/test_exact_steady_plan.py proves each call's regime with
the library's plan code).  Every query of every call is compared with the oracle composed in tests/exact_ref.py: ids equal, float8 bits equal,
counts equal, padding 0xFFFFFFFF / NaN; there is no tolerance.  The grouped calls also return the bytes of the per-query hx_exact_search calls,
and the filter-set call the bytes of the bitmap call; the sidecar kernel returns the bytes of an engine without a sidecar."""
import numpy as np
import pytest

import pgvector_rx_amd as hx
import exact_ref as ref
import exact_steady_cases as T

assert (T.F32, T.F16, T.BIT, T.SPARSE) == (hx.F32, hx.F16, hx.BIT, hx.SPARSE)
assert (T.L2, T.IP, T.COS, T.L1, T.HAM, T.JAC) == (hx.OP_L2, hx.OP_NEG_IP, hx.OP_COSINE, hx.OP_L1, hx.OP_HAMMING, hx.OP_JACCARD)
METRIC_OF = {hx.OP_HAMMING: hx.HAMMING, hx.OP_JACCARD: hx.JACCARD}
NOT_FOUND = 0xFFFFFFFF


# ---- data -----------------------------------------------------------------------------------------------------------------------------------
def random_rows(c, n, rng):
    dtype, dim = c["dtype"], c["dim"]
    if dtype == hx.F32:
        return rng.standard_normal((n, dim), dtype=np.float32)
    if dtype == hx.F16:
        return rng.standard_normal((n, dim), dtype=np.float32).astype(np.float16).view(np.uint16)
    if dtype == hx.BIT:
        return rng.integers(0, 256, (n, (dim + 7) // 8), dtype=np.uint8)
    sp = []
    for nnz in rng.integers(0, c["max_nnz"] + 1, n):
        idx = np.unique(rng.integers(0, dim, int(nnz)))
        sp.append((idx, rng.standard_normal(len(idx)).astype(np.float32)))
    return hx.pack_sparse(dim, sp)


def few_bits(c, n, rng):
    """bit rows with at most 3 of their first 16 bits set"""
    out = np.zeros((n, (c["dim"] + 7) // 8), np.uint8)
    bits = np.zeros(n, np.uint16)
    for _ in range(3):
        bits |= np.where(rng.random(n) < 0.7, np.uint16(1) << rng.integers(0, 16, n).astype(np.uint16), np.uint16(0)).astype(np.uint16)
    out[:, 0], out[:, 1] = bits & 0xFF, bits >> 8
    return out


def make_data(c, op, n, nq, seed):
    """(rows, queries, {query: its values over all rows, where making the data computed them})"""
    rng = np.random.default_rng(seed)
    kind, known = c["data"], {}
    if kind == "ties" and c["dtype"] == hx.BIT:
        return few_bits(c, n, rng), few_bits(c, nq, rng), known
    if kind == "ties":                                  # rows of {0, -1}; even queries of {0, 1}: <#> is -0.0 wherever the product vanishes, and nothing is smaller
        rows = np.where(rng.random((n, c["dim"])) < 0.03, -1.0, 0.0).astype(np.float32)
        qs = rng.integers(-1, 2, (nq, c["dim"])).astype(np.float32)
        qs[0::2] = (rng.random((len(qs[0::2]), c["dim"])) < 0.2).astype(np.float32)
        return rows, qs, known
    rows, qs = random_rows(c, n, rng), random_rows(c, nq, rng)
    if kind == "late":                                  # the nearest rows of every query: rows lo .. hi - 1
        lo, hi = c["late"]
        centre = 4 * rng.standard_normal(c["dim"], dtype=np.float32)
        qs = centre + np.float32(0.1) * qs
        rows[lo:hi] = centre + np.float32(0.5) * rows[lo:hi]
    if kind == "zeros":                                 # <=>: NaN for every row but seven
        keep = rng.permutation(min(n, 16384))[:7]
        z = np.zeros_like(rows)
        z[keep] = rows[keep]
        rows = z
    if kind in ("improving", "worsening"):
        v = ref.values(c["dtype"], c["dim"], op, qs[0], rows)
        perm = np.argsort(-v if kind == "improving" else v, kind="stable")
        rows, known[0] = np.ascontiguousarray(rows[perm]), v[perm]
        assert (np.diff(known[0]) <= 0).all() if kind == "improving" else (np.diff(known[0]) >= 0).all()
        if nq > 9:                                      # a second such query at another place of the tile
            qs[9] = qs[0]
            known[9] = known[0]
    return rows, qs, known


def engine(c, op, rows, queries, **kw):
    e = hx.Engine(c["dtype"], METRIC_OF.get(op, hx.L2SQ), c["dim"], len(rows), scan_only=c["scan_only"], **kw)
    assert (e.row_bytes + 15) // 16 * 16 == T.pitch(c["dtype"], c["dim"])    # the device row pitch: the row bytes in 16-byte fragments
    e.append(rows)
    e.set_queries(queries)
    return e


class Oracle:
    """The operator values of a query over the rows it is ever asked about, computed once."""

    def __init__(self, c, op, rows, queries, need, known):
        self.c, self.op, self.rows, self.queries, self.need, self.v = c, op, rows, queries, need, dict(known)
        self.norms = None
        if op == hx.OP_COSINE and c["dtype"] != hx.SPARSE:
            self.norms = ref.self_ip(c["dtype"], c["dim"], rows[:max(need.values())])

    def values(self, qi):
        if qi not in self.v or len(self.v[qi]) < self.need[qi]:
            m = self.need[qi]
            self.v[qi] = ref.values(self.c["dtype"], self.c["dim"], self.op, self.queries[qi], self.rows[:m], None if self.norms is None else self.norms[:m])
        return self.v[qi]

    def check(self, qi, cand, ks, got_of_k, what):
        """got_of_k[k] = (ids[k], dist[k], count) of query qi; cand: the ascending row ids it may return"""
        v = self.values(qi)[cand]
        o = ref.order(v, cand)[:max(ks)]
        for k in ks:
            ids, dist, cnt = got_of_k[k]
            want_ids, want_d = cand[o[:k]], v[o[:k]]
            n = int(cnt)
            assert n == len(want_ids) == min(k, len(cand)), (what, qi, k, n)
            assert ids[:n].tolist() == want_ids.tolist(), (what, qi, k)
            assert ref.same_bits(dist[:n], want_d), (what, qi, k)
            assert (ids[n:] == NOT_FOUND).all() and np.isnan(dist[n:]).all(), (what, qi, k)


def same(a, b):
    return all(x.shape == y.shape and (x.view(np.uint8) == y.view(np.uint8)).all() for x, y in zip(a, b))


def pick(n_rows, n_pass, rng):
    m = np.zeros(n_rows, bool)
    m[rng.permutation(n_rows)[:n_pass]] = True
    return m


# ---- the plain path: hx_exact_search -------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name,op", T.PLAIN, ids=T.case_id)
def test_plain(name, op, monkeypatch):
    c = T.BY_NAME[name]
    calls = c["plain"]
    n, nq = T.rows_needed(c, calls), T.queries_needed(c, calls)
    rows, qs, known = make_data(c, op, n, nq, seed=1000 + 17 * T.CASES.index(c) + op)
    need = {}
    for call in calls:
        for qi in range(call["first_query"], call["first_query"] + call["nq"]):
            need[qi] = max(need.get(qi, 0), call["first_row"] + call["n_rows"])
    oracle = Oracle(c, op, rows, qs, need, known)
    monkeypatch.delenv("HX_EXACT_SCRATCH", raising=False)
    if c["sidecar"]:
        monkeypatch.setenv("HX_EXACT_SIDECAR", "1")     # the pre-pass at any size
    else:
        monkeypatch.delenv("HX_EXACT_SIDECAR", raising=False)
    e = engine(c, op, rows, qs)
    e_no = engine(c, op, rows, qs, sidecar=False) if c["sidecar"] else None
    rng = np.random.default_rng(5)
    for call in calls:
        fr, nr, fq, cq = call["first_row"], call["n_rows"], call["first_query"], call["nq"]
        mask = None if call["n_pass"] is None else pick(nr, call["n_pass"], rng)
        cand = np.arange(fr, fr + nr) if mask is None else fr + np.nonzero(mask)[0]
        got = {}
        for k in call["ks"]:
            e.exact_sidecar_stats(reset=True)
            got[k] = e.exact_search(op, k, first_query=fq, nq=cq, first_row=fr, n_rows=nr, row_pass=mask)
            coded, fetched = e.exact_sidecar_stats()
            if c["sidecar"]:
                tiles = (cq + 3) // 4 if cq >= 4 else cq
                assert coded == tiles * len(cand), (coded, tiles, len(cand))          # every row of the call, once per query tile
                assert 0 < fetched <= coded
                assert same(got[k], e_no.exact_search(op, k, first_query=fq, nq=cq, first_row=fr, n_rows=nr, row_pass=mask))
                assert e_no.exact_sidecar_stats() == (0, 0)
            else:
                assert (coded, fetched) == (0, 0)
        for i in range(cq):
            oracle.check(fq + i, cand, list(call["ks"]), {k: (g[0][i], g[1][i], g[2][i]) for k, g in got.items()}, (name, "plain", cq, nr))
    if c["data"] == "ties" and op == hx.OP_NEG_IP:      # the threshold is the key of zero: -0.0 with its sign, by ascending id
        ids, d, _ = e.exact_search(op, 10, nq=16, n_rows=16384)
        assert (d[0] == 0).all() and np.signbit(d[0]).all() and (np.diff(ids[0].astype(np.int64)) > 0).all()
    if c["data"] == "late":
        ids, _, _ = e.exact_search(op, 10, nq=3, n_rows=16384 if c["lanes"] == 64 else 32768)
        assert ((ids >= c["late"][0]) & (ids < c["late"][1])).all()
    if c["data"] == "zeros":                            # a NaN threshold: the seven finite rows, then NaN by ascending id
        ids, d, _ = e.exact_search(op, 10, nq=16, n_rows=16384)
        assert (~np.isnan(d[:, :7])).all() and np.isnan(d[:, 7:]).all() and (np.diff(ids[:, 7:].astype(np.int64), axis=1) > 0).all()
    e.close()
    if e_no:
        e_no.close()


# ---- the grouped path: hx_exact_search_filtered and hx_exact_search_set ------------------------------------------------------------------
def n_tiles(m, qmax):
    """tiles of a group of m queries: of 16 while m >= 16, of 4 while m >= 2, then of 1 (hx_exact_plan.h)"""
    t = 0
    while m > 0:
        q = 16 if qmax >= 16 and m >= 16 else 4 if qmax >= 4 and m >= 2 else 1
        m -= min(m, q)
        t += 1
    return t


@pytest.mark.gpu
@pytest.mark.parametrize("name,op", T.GROUPED, ids=T.case_id)
def test_grouped(name, op, monkeypatch):
    c = T.BY_NAME[name]
    calls = c["grouped"]
    n, nq = T.rows_needed(c, calls), T.queries_needed(c, calls)
    rows, qs, known = make_data(c, op, n, nq, seed=2000 + 17 * T.CASES.index(c) + op)
    oracle = Oracle(c, op, rows, qs, {qi: n for qi in range(nq)}, known)
    monkeypatch.delenv("HX_EXACT_SIDECAR", raising=False)
    monkeypatch.setenv("HX_EXACT_SCRATCH", str(T.SCRATCH))   # one slice per tile; the plain per-query calls below do not plan their slices by it
    e = engine(c, op, rows, qs)
    e.set_timing(True)
    pitch = T.pitch(c["dtype"], c["dim"])
    qmax = 1 if c["dtype"] == hx.SPARSE else 16 if 16 * pitch <= 65536 else 4 if 4 * pitch <= 65536 else 1
    rng = np.random.default_rng(6)
    for call in calls:
        fr, nr, fq = call["first_row"], call["n_rows"], call["first_query"]
        masks = [pick(nr, n_pass, rng) for _, n_pass in call["groups"]]
        fo = rng.permutation(np.concatenate([np.full(m, f, np.int32) for f, (m, _) in enumerate(call["groups"])] + [np.full(call["unfiltered"], -1, np.int32)]))
        tiles = sum(n_tiles(m, qmax) for m, _ in call["groups"]) + n_tiles(call["unfiltered"], qmax)
        fset = hx.FilterSet.from_bitmaps(e, masks, n_rows=nr, first_row=fr)
        got = {}
        for k in call["ks"]:
            e.kernel_stats(7, reset=True)
            got[k] = e.exact_search_filtered(op, k, masks, fo, first_query=fq, nq=len(fo), first_row=fr, n_rows=nr)
            assert e.kernel_stats(7, reset=True)["launches"] == 1 + 2 * tiles            # the compaction, then a scan and a merge per tile: one slice each
            by_set = e.exact_search_set(op, k, fset, fo, first_query=fq, nq=len(fo))
            assert e.kernel_stats(7, reset=True)["launches"] == 2 * tiles
            assert same(got[k], by_set), (name, k, "filter set")
            one = [e.exact_search(op, k, first_query=fq + i, nq=1, first_row=fr, n_rows=nr, row_pass=None if f < 0 else masks[f]) for i, f in enumerate(fo)]
            assert same(got[k], tuple(np.concatenate([o[j] for o in one]) for j in range(3))), (name, k, "per-query calls")
        for i, f in enumerate(fo):
            cand = np.arange(fr, fr + nr) if f < 0 else fr + np.nonzero(masks[f])[0]
            oracle.check(fq + i, cand, list(call["ks"]), {k: (g[0][i], g[1][i], g[2][i]) for k, g in got.items()}, (name, "grouped", int(f)))
        fset.close()
    e.close()
