"""Every engine entry point that addresses rows, on a row table LARGER THAN 4 GiB: vector(2000) x 560 000 rows = 4.48 GB at a pitch of 8000 bytes,
so the rows from id 2^32 / pitch on start past byte 2^32.  A `rows + id * pitch` evaluated in 32 bits, or a 32-bit byte count on the host side of a
launch, wraps to an address inside ANOTHER row of the table: no fault, a plausible wrong value.  Every id list below therefore holds ids under the
boundary, the two ids on either side of it and ids among the last 100 rows, and every value is compared bit for bit with the oracle in the device's
canonical order (orc.W64; the exact scans: the model composed in tests/exact_ref.py) over the same rows materialised on the host.

The table is one block of 8192 N(0, 1) rows appended again and again with element 0 set to the block number: row(r) = base[r % 8192] with
element 0 = r // 8192.  Rows are distinct and the host can produce any subset without holding 4.5 GB.  No index is built here.

The tests share one engine and run in file order; the last one normalises rows in place."""
import time

import numpy as np
import pytest

import pgvector_rx_amd as hx
from oracle import orc
import exact_ref as ref
from test_gpu_halfcast import orc_half
from test_gpu_sidecar import sidecar_of

pytestmark = pytest.mark.gpu

N, DIM, BLOCK = 560_000, 2000, 8192
BAD_ELEMENT, BAD_VALUE = 7, np.float32(1e6)          # one element no half can hold, in a row of the last appended block
TAIL = 140_000                                       # >= 131 072 passing rows: hx_exact_search takes the 8-bit sidecar route
RANGE_TAIL = 70_000                                  # >= 65 536: so does hx_exact_range


def bits(a):
    return np.asarray(a, np.float32).view(np.uint32)


class Table:
    """The host's statement of the table: row(r) for any id list."""

    def __init__(self):
        self.base = np.random.default_rng(4096).standard_normal((BLOCK, DIM), dtype=np.float32)
        self.bad_row = N - 2500
        assert self.bad_row // BLOCK == (N - 1) // BLOCK

    def rows_of(self, ids):
        ids = np.asarray(ids, np.int64).reshape(-1)
        src = np.where(ids == N - 1, 5, ids)                     # the last row is row(5) once more: a pair of genuinely equal rows
        out = self.base[src % BLOCK]                             # fancy indexing: a copy
        out[:, 0] = src // BLOCK
        out[ids == self.bad_row, BAD_ELEMENT] = BAD_VALUE
        return out


@pytest.fixture(scope="module")
def big():
    t0 = time.time()
    s = Table()
    rows_of = s.rows_of
    rng = np.random.default_rng(4097)
    e = hx.Engine(hx.F32, hx.L2SQ, DIM, N)
    s.pitch = int(e.row_bytes)
    s.boundary = -(-(1 << 32) // s.pitch)                    # the first row that starts at or past byte 2^32
    assert N * s.pitch > (1 << 32) and N - TAIL < s.boundary < N - 4096     # the scanned windows straddle the boundary or lie past it
    block = s.base.copy()
    for j in range(-(-N // BLOCK)):
        first, cnt = j * BLOCK, min(BLOCK, N - j * BLOCK)
        block[:, 0] = j
        if first + cnt == N:
            block[:cnt] = rows_of(np.arange(first, N))
        assert e.append(block[:cnt]) == first
    assert e.num_rows == N
    src = np.array([5, 123_457, s.boundary - 3000, s.boundary - 1, s.boundary, s.boundary + 1, N - 60_000, N - 7])
    s.q_src = src
    s.qs = (rows_of(src) + 1e-3 * rng.standard_normal((8, DIM))).astype(np.float32)
    e.set_queries(s.qs)
    s.e = e
    t1 = time.time()
    # operator values of every query against the last TAIL rows, once, for the scans below (the reference materialises 1.1 GB of rows)
    tail = rows_of(np.arange(N - TAIL, N))
    s.tail_values = [ref.values(hx.F32, DIM, hx.OP_L2, s.qs[q], tail) for q in range(8)]
    del tail
    print("\n4.48 GB table filled in %.1f s; reference values of the last %d rows in %.1f s" % (t1 - t0, TAIL, time.time() - t1))
    yield s
    e.close()


def mixed_ids(s, k, seed):
    """k ids: under the boundary, the two on either side of it, and among the last 100 rows."""
    rng = np.random.default_rng(seed)
    b = s.boundary
    edge = [b - 2, b - 1, b, b + 1]
    n_low = (k - 4) // 3
    n_last = (k - 4) // 3
    low = rng.integers(0, b - 2, n_low)
    last = rng.choice(np.arange(N - 100, N), n_last, replace=False)
    high = rng.integers(b + 2, N - 100, k - 4 - n_low - n_last)
    ids = np.concatenate([low, edge, high, last]).astype(np.uint32)
    assert (ids >= b).sum() > 0 and (ids < b).sum() > 0 and (ids >= N - 100).sum() > 0
    return rng.permutation(ids)


def test_table_is_past_4gib_and_reads_back(big):
    s = big
    assert s.boundary == (1 << 32) // s.pitch + 1 and s.boundary * s.pitch >= 1 << 32 > (s.boundary - 1) * s.pitch
    for first, n in ((N - 3, 3), (s.boundary - 1, 2), (0, 2)):
        want = s.rows_of(np.arange(first, first + n))
        assert s.e.read_rows(first, n).tobytes() == want.tobytes(), first
    assert s.e.read_rows(N - 1, 1).tobytes() == s.e.read_rows(5, 1).tobytes()


def test_distances_by_slot_and_by_row(big):
    s = big
    ids = mixed_ids(s, 257, 1)
    rows = s.rows_of(ids)
    for q in (0, 5):
        got = s.e.distances(s.qs[q], ids)
        want = np.float32(orc.distances_many(hx.F32, hx.L2SQ, DIM, s.qs[q], rows, order=orc.W64))
        assert np.array_equal(bits(got), bits(want)), q
    # groups whose query is a slot, a row under the boundary, the rows on either side of it and a row among the last 100
    gq = [hx.QUERY_SLOT | 3, 17, s.boundary - 1, s.boundary, hx.QUERY_SLOT | 6, N - 2, s.boundary + 1]
    sizes = [64, 33, 1, 70, 0, 40, 49]
    off = np.concatenate([[0], np.cumsum(sizes)])
    assert off[-1] == len(ids)
    got = s.e.distances_batch(gq, off, ids)
    for g, query in enumerate(gq):
        q = s.qs[query & 0x7FFFFFFF] if query & hx.QUERY_SLOT else s.rows_of([query])[0]
        want = np.float32(orc.distances_many(hx.F32, hx.L2SQ, DIM, q, rows[off[g]:off[g + 1]], order=orc.W64))
        assert np.array_equal(bits(got[off[g]:off[g + 1]]), bits(want)), g


def test_pair_kernels(big):
    s = big
    ids = mixed_ids(s, 64, 2)
    rows = s.rows_of(ids)
    want = np.float32(orc.pairwise(hx.F32, hx.L2SQ, DIM, rows, np.arange(64), orc.W64))
    assert np.array_equal(bits(s.e.pairwise(ids)), bits(want))
    a, b, c = ids[:33], ids[:32], ids[33:64]
    assert (a >= s.boundary).any() and (a < s.boundary).any() and (c >= s.boundary).any() and (c < s.boundary).any()
    tri, rect = s.e.pairwise_many([(a.tolist(), None), (b.tolist(), c.tolist())])
    assert np.array_equal(bits(tri), bits(want[:33, :33][np.tril_indices(33, -1)]))
    assert np.array_equal(bits(rect), bits(want[:32, 33:64]))


def test_rows_equal(big):
    s = big
    b = s.boundary
    r = np.array([3, b - BLOCK - 1, b - BLOCK, b - 1, b, b + 1, N - 1 - BLOCK - 50], np.uint32)
    assert (r + BLOCK >= b).sum() >= 5 and (r + BLOCK < N).all()
    assert not s.e.rows_equal(r, r + BLOCK).any()                # differ in element 0 only
    assert s.e.rows_equal(r + BLOCK, r + BLOCK).all() and s.e.rows_equal(r, r).all()
    assert s.e.rows_equal([5, N - 1, N - 1, N - 1], [N - 1, 5, 5 + BLOCK, N - 2]).tolist() == [True, True, False, False]


def host_sidecar(rows):
    """k_sc_encode (hx_sidecar.hip; sequentially: `encode` in tests/test_sidecar_bound_host.py) in numpy, for finite rows: lo / hi, step = (hi - lo) / 255
    in f32, codes rint((x - lo) / step) clamped to [0, 255], x^ = fmaf(step, code, lo), e_x = sqrt(sum (x - x^)^2) (1 + 2^-40) rounded UP to f32.
    The f64 sum runs in the kernel's order -- lane l adds its elements l, l + 64, ... in turn, then the xor butterfly 32 .. 1 -- so e_x is the
    kernel's to the bit.  Returns (codes uint8 [n, dim], meta f32 [n, 3])."""
    x = np.ascontiguousarray(rows, np.float32)
    n, dim = x.shape
    assert np.isfinite(x).all()
    lo, hi = x.min(1, keepdims=True), x.max(1, keepdims=True)
    step = ((hi - lo) / np.float32(255.0)).astype(np.float32)
    assert (step > 0).all() and np.isfinite(step).all()
    t = np.rint(((x - lo) / step).astype(np.float32))
    code = np.clip(t, 0.0, 255.0).astype(np.uint32)
    xh = (step.astype(np.float64) * code + lo.astype(np.float64)).astype(np.float32)      # the product is exact in f64 and so is the sum here: one rounding, as fmaf
    dd = (x.astype(np.float64) - xh.astype(np.float64)) ** 2
    pad = np.zeros((n, -(-dim // 64) * 64))
    pad[:, :dim] = dd
    lanes = np.zeros((n, 64))
    for chunk in pad.reshape(n, -1, 64).transpose(1, 0, 2):
        lanes = lanes + chunk
    for off in (32, 16, 8, 4, 2, 1):
        lanes = lanes + lanes[:, np.arange(64) ^ off]
    e = np.sqrt(lanes[:, 0]) * (1.0 + 2.0 ** -40)
    ex = e.astype(np.float32)
    up = ex.astype(np.float64) < e
    ex[up] = np.nextafter(ex[up], np.float32(np.inf))
    return code.astype(np.uint8), np.stack([lo[:, 0], step[:, 0], ex], axis=1).astype(np.float32)


def test_sidecar_codes_and_bounds(big):
    """The 8-bit sidecar of rows past the boundary is the host's encoding of those rows (host_sidecar) and what a small engine, every row of it
    under 4 GiB, holds for them.  The searches' lower bound for them is that engine's bound, bit for bit (the kernel sums lane-parallel: the
    sequential hx_l2_lb of hx_ops.h bounds the same distance but is not its bit pattern), and never above the oracle's distance."""
    s = big
    for first, n in ((N - 3, 3), (s.boundary - 1, 2)):
        codes, meta = s.e.sidecar_read(first, n)
        rows = s.rows_of(np.arange(first, first + n))
        hc, hm = host_sidecar(rows)
        assert np.array_equal(codes, hc) and np.array_equal(meta.view(np.uint32), hm.view(np.uint32)), first
        c0, m0 = sidecar_of(rows)
        assert np.array_equal(codes, c0) and np.array_equal(meta.view(np.uint32), m0.view(np.uint32)), first
    ids = mixed_ids(s, 100, 3)
    ids = ids[ids != s.bad_row]
    rows = s.rows_of(ids)
    small = hx.Engine(hx.F32, hx.L2SQ, DIM, len(ids))
    try:
        small.append(rows)
        small.set_queries(s.qs)
        local = np.arange(len(ids), dtype=np.uint32)
        for q in (1, 6):
            lb = s.e.sidecar_bounds(hx.QUERY_SLOT | q, ids)
            assert np.array_equal(bits(lb), bits(small.sidecar_bounds(hx.QUERY_SLOT | q, local))), q
            d = np.float32(orc.distances_many(hx.F32, hx.L2SQ, DIM, s.qs[q], rows, order=orc.W64))
            assert (lb <= d).all() and (lb > 0).any(), q
        hi = int(s.boundary + 1)                                  # the query is a row past the boundary
        lb = s.e.sidecar_bounds(hi, ids)
        at = int(np.nonzero(ids == hi)[0][0])
        assert np.array_equal(bits(lb), bits(small.sidecar_bounds(at, local)))
    finally:
        small.close()


def check_topk(s, got, cand, values_of, k):
    ids, dist, cnt = got
    for q in range(8):
        v = values_of(q)
        o = ref.order(v, cand)[:k]
        c = int(cnt[q])
        assert c == len(o) == min(k, len(cand)), q
        assert ids[q, :c].tolist() == cand[o].tolist(), q
        assert ref.same_bits(dist[q, :c], v[o]), q


def test_exact_search_window_of_the_last_rows(big):
    s = big
    got = s.e.exact_search(hx.OP_L2, 10, first_row=N - 4096, n_rows=4096)
    check_topk(s, got, np.arange(N - 4096, N), lambda q: s.tail_values[q][TAIL - 4096:], 10)


def test_exact_search_whole_table_with_a_row_filter(big):
    s = big
    b = s.boundary
    cand = np.unique(np.concatenate([np.random.default_rng(4).choice(N, 3000, replace=False), [b - 2, b - 1, b, b + 1], s.q_src, np.arange(N - 100, N, 9)])).astype(np.int64)
    mask = np.zeros(N, np.uint8)
    mask[cand] = 1
    got = s.e.exact_search(hx.OP_L2, 100, row_pass=mask)
    rows = s.rows_of(cand)
    check_topk(s, got, cand, lambda q: ref.values(hx.F32, DIM, hx.OP_L2, s.qs[q], rows), 100)
    assert got[0][:, 0].tolist() == s.q_src.tolist()              # each query's own row, on either side of the boundary, is its nearest


def test_exact_search_through_the_sidecar(big, monkeypatch):
    s = big
    cand = np.arange(N - TAIL, N)
    s.e.exact_sidecar_stats(reset=True)
    got = s.e.exact_search(hx.OP_L2, 10, first_row=N - TAIL, n_rows=TAIL)
    coded, fetched = s.e.exact_sidecar_stats(reset=True)
    print("\nexact_search over %d rows: %d code rows read, %d f32 rows read" % (TAIL, coded, fetched))
    assert coded > 0                                             # the scan went through the 8-bit sidecar
    check_topk(s, got, cand, lambda q: s.tail_values[q], 10)
    monkeypatch.setenv("HX_EXACT_SIDECAR", "0")
    plain = s.e.exact_search(hx.OP_L2, 10, first_row=N - TAIL, n_rows=TAIL)
    assert s.e.exact_sidecar_stats(reset=True) == (0, 0)
    for a, b in zip(got, plain):
        assert a.tobytes() == b.tobytes()


def test_exact_range(big, monkeypatch):
    s = big
    first = N - RANGE_TAIL
    cand = np.arange(first, N)
    vals = [s.tail_values[q][TAIL - RANGE_TAIL:] for q in range(8)]
    radius = np.array([np.sort(vals[q])[5 + 6 * q] for q in range(8)])           # a stored value: `<` leaves the tie out
    want = [np.nonzero(vals[q] < radius[q])[0] for q in range(8)]
    assert all(not np.isnan(v).any() for v in vals) and all(5 <= len(w) <= 50 for w in want)
    s.e.exact_sidecar_stats(reset=True)
    off, ids, dist = s.e.exact_range(hx.OP_L2, radius, hx.CMP_LT, first_row=first, n_rows=RANGE_TAIL)
    assert s.e.exact_sidecar_stats(reset=True)[0] > 0            # through the sidecar
    for q in range(8):
        a, b = int(off[q]), int(off[q + 1])
        assert ids[a:b].tolist() == cand[want[q]].tolist(), q
        assert ref.same_bits(dist[a:b], vals[q][want[q]]), q
    coff, cids, _ = s.e.exact_range(hx.OP_L2, radius, hx.CMP_LT, first_row=first, n_rows=RANGE_TAIL, count_only=True)
    assert np.array_equal(coff, off) and len(cids) == 0
    assert s.e.exact_sidecar_stats(reset=True)[0] > 0
    monkeypatch.setenv("HX_EXACT_SIDECAR", "0")                  # the plain kernels: every f32 row past the boundary is read
    plain = s.e.exact_range(hx.OP_L2, radius, hx.CMP_LT, first_row=first, n_rows=RANGE_TAIL)
    assert s.e.exact_sidecar_stats(reset=True) == (0, 0)
    for a, b in zip((off, ids, dist), plain):
        assert a.tobytes() == b.tobytes()
    assert np.array_equal(s.e.exact_range(hx.OP_L2, radius, hx.CMP_LT, first_row=first, n_rows=RANGE_TAIL, count_only=True)[0], off)


def test_exact_rerank(big):
    s = big
    lists = [np.unique(np.concatenate([mixed_ids(s, 299, 10 + q), [s.q_src[q]]])).astype(np.uint32) for q in range(8)]
    ids, dist, cnt = s.e.exact_rerank(hx.OP_L2, lists, 10)
    for q in range(8):
        want_ids, want_d = ref.topk(hx.F32, DIM, hx.OP_L2, s.qs[q], s.rows_of(lists[q]), 10, ids=lists[q])
        assert cnt[q] == 10 and ids[q].tolist() == want_ids.tolist() and ref.same_bits(dist[q], want_d), q
        assert ids[q, 0] == s.q_src[q]                           # each query's own row is nearest


def test_halfvec_cast_of_rows_past_the_boundary(big):
    """hx_append_rows_halfvec reads its source rows past byte 2^32.  The range error names the source row and the element (the flat index
    row * dim + element is past 2^30, the row's byte offset past 2^32); the rows that are in range equal the oracle's f32_to_half, element by element."""
    s = big
    assert s.bad_row * DIM + BAD_ELEMENT > 1 << 30 and s.bad_row >= s.boundary
    dst = hx.Engine(hx.F16, hx.L2SQ, DIM, 2000)
    try:
        with pytest.raises(hx.HxError) as ei:
            dst.append_halfvec_from(s.e, N - 4000, 2000)
        msg = str(ei.value)
        assert ei.value.code == hx.E_RANGE and '"1000000" is out of range for type halfvec' in msg
        assert "row %d" % s.bad_row in msg and "element %d" % BAD_ELEMENT in msg
        assert dst.num_rows == 0
        assert dst.append_halfvec_from(s.e, N - 2000, 2000) == 0 and dst.num_rows == 2000
        got = dst.read_rows(0, 2000)
        rows = s.rows_of(np.arange(N - 2000, N))
        assert np.array_equal(got, orc_half(rows.view(np.uint32).ravel()).reshape(2000, DIM))
    finally:
        dst.close()


def test_normalize_rows_in_place_last(big):
    """hx_normalize_rows on the last 64 rows (in place: this test runs last), norms and rows equal to the oracle's l2_normalize; the sidecar follows."""
    s = big
    first = N - 64
    before = s.rows_of(np.arange(first, N))
    norms = s.e.normalize_rows(first, 64)
    got = s.e.read_rows(first, 64)
    for i in range(64):
        want, wn = orc.l2_normalize(hx.F32, DIM, before[i])
        assert norms[i] == wn and got[i].tobytes() == want.tobytes(), i
    codes, meta = s.e.sidecar_read(first, 64)
    c0, m0 = sidecar_of(got)
    assert np.array_equal(codes, c0) and np.array_equal(meta.view(np.uint32), m0.view(np.uint32))
    assert s.e.read_rows(first - 1, 1).tobytes() == s.rows_of([first - 1]).tobytes()              # the row before them is untouched
