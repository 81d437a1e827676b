"""Graph, scan, aminsert and vacuum parity with the oracle on SIGNED and WIDE-RANGE rows.

The other index tests draw rows uniform in [0, 1): every distance of a search has one sign, all lie within a factor of two and all rows have
about the same norm.  Here the rows are
  normal   N(0, 1): inner-product distances of both signs, L2 / L1 of rows on both sides of the origin;
  scaled   N(0, 1) times a per-row log-uniform factor (6 decades in f32, 3 in f16, finite in f16): one row dwarfs its neighbours;
  offset   N(0, 1e-3) around a common centre of norm 30: near-equal inner products, L2 / L1 between rows that agree in their leading bits --
           the order of summation (SEQ against the device's W64) changes the value, so only the canonical order reproduces the graph;
at dims on both sides of each lanes-per-row switch (pitch 128 B, 512 B) and of the 1 KiB chunk, for m = 8 (k_links), 20 (lists of 40) and 40
(hx_biglist.hip).  What the data is meant to do is asserted on the oracle alone before the device is touched.  Expected values are the oracle's."""
import numpy as np
import pytest

import pgvector_rx_amd as hx
from oracle import orc
from test_gpu_index import assert_same_graph, build_both

pytestmark = pytest.mark.gpu

KINDS = ["normal", "scaled", "offset"]
F32_DIMS = [31, 32, 33, 128, 129, 256, 257]
F16_DIMS = [64, 65, 256, 257, 513]
NQ = 8


def make_data(kind, dt, n, dim, rng):
    """n rows of the kind as f32; halfvec rows are their f16 roundings (checked finite)."""
    x = rng.standard_normal((n, dim))
    if kind == "scaled":
        decades = 6.0 if dt == hx.F32 else 3.0
        x = x * 10.0 ** rng.uniform(-decades / 2, decades / 2, (n, 1))
    elif kind == "offset":
        c = rng.standard_normal(dim)
        x = 30.0 * c / np.linalg.norm(c) + 1e-3 * x
    x = x.astype(np.float32)
    if dt == hx.F16:
        h = x.astype(np.float16)
        assert np.isfinite(h).all()
        return h.view(np.uint16)
    return x


def as_f64(dt, rows):
    return (rows.view(np.float16) if dt == hx.F16 else rows).astype(np.float64)


def offset_attainable(dt, metric, dim):
    """Where two summation orders of `offset` rows can differ by 1e-6 at all.  The operands of a difference agree in their leading bits, so a - b is exact
    (and every f16 product is exact in f32): what is left is the rounding of the running sum, about sqrt(dim) * 2^-24.  Measured on the oracle over all
    pairs of 400 rows (largest relative SEQ - W64 difference): f32 <-> / <#> 3.9e-7 at dim 33, 8.0e-7 at 128 / 129, 1.0e-6 to 1.1e-6 at 256 / 257; f32 <+>
    at most 3.4e-7 at any dim; halfvec <-> at most 2.0e-7; halfvec <#> 5.4e-7 at 64 / 65, 1.1e-6 to 1.5e-6 from 256 on.  The kind is drawn where the bound
    can be met; the other shapes get `normal` and `scaled` rows."""
    return dim >= 256 and (metric == hx.NEG_IP or (metric == hx.L2SQ and dt == hx.F32))


def _cases():
    """A seeded subset of the matrix: every (type, metric) with every kind, every dim, every m, both batch sizes, both placements."""
    rng = np.random.default_rng(2027)
    combos = [(hx.F32, mt, d) for mt in (hx.L2SQ, hx.NEG_IP, hx.L1) for d in F32_DIMS] + [(hx.F16, mt, d) for mt in (hx.L2SQ, hx.NEG_IP) for d in F16_DIMS]
    order = [int(i) for i in rng.permutation(len(combos))]
    order += [int(i) for i in rng.choice(len(combos), 40 - len(combos), replace=False)]
    seen, had_offset, cases = {}, set(), []
    for i, ci in enumerate(order):
        dt, metric, dim = combos[ci]
        if offset_attainable(dt, metric, dim) and (dt, metric, dim) not in had_offset:
            had_offset.add((dt, metric, dim))
            kind = 2
        else:
            k = seen.get((dt, metric), int(rng.integers(0, 2)))
            seen[(dt, metric)] = k + 1
            kind = k % 2
        m = [8, 20, 40][(i + int(rng.integers(0, 3))) % 3]
        efc = {8: 32, 20: 48, 40: 80}[m]
        batch = [1, 37][int(rng.integers(0, 2))]
        fused = 1 if m > 32 else int(rng.integers(0, 2))            # lists of more than 64 slots are served by the device kernels only
        # inner product on N(0, 1): the lists of a large graph hold the LARGEST products only, all of one sign (measured on the oracle: no list of
        # either sign mix from n = 250 on); a graph of a few lists' length keeps both, and its full lists are pruned across the signs
        n = 3 * m if (metric == hx.NEG_IP and kind == 0) else int(rng.integers(260, 420))
        dup = int(rng.choice([0, 7, 11]))
        cases.append((i, dt, metric, dim, kind, m, efc, n, batch, fused, dup))
    return cases


CASES = _cases()
assert {(c[1], c[2], c[4]) for c in CASES} == {(dt, mt, k) for dt, mts in ((hx.F32, (hx.L2SQ, hx.NEG_IP, hx.L1)), (hx.F16, (hx.L2SQ, hx.NEG_IP))) for mt in mts for k in range(3)
                                                  if k < 2 or offset_attainable(dt, mt, 256)}
assert {c[3] for c in CASES} == set(F32_DIMS + F16_DIMS) and {c[5] for c in CASES} == {8, 20, 40} and {c[8] for c in CASES} == {1, 37} and {c[9] for c in CASES} == {0, 1}
assert {(c[5], c[2] == hx.NEG_IP) for c in CASES} >= {(8, True), (20, True), (40, True)}           # k_links, the m > 16 path and the big-list kernels see <#>


SEEDS = {4: 7104, 5: 7305, 14: 7114, 30: 7630}                                                                                         # chosen on the CPU so that the preconditions hold


def case_data(case):
    i, dt, metric, dim, kind, m, efc, n, batch, fused, dup = case
    rng = np.random.default_rng(SEEDS.get(i, 5000 + i))
    data = make_data(KINDS[kind], dt, n + NQ, dim, rng)
    rows, qs = np.ascontiguousarray(data[:n]), np.ascontiguousarray(data[n:])
    if dup:
        for j in range(dup, n, 5 * dup):                                                           # a few duplicates per case
            rows[j] = rows[j - 1]
    return rows, qs, hx.draw_levels(n, m, seed=5000 + i)


def oracle_graph(dt, metric, dim, rows, levels, m, efc, batch):
    o = orc.Index(dt, metric, dim, m=m, ef_construction=efc, order=orc.W64)
    i = 0
    for b in hx.batch_schedule(0, len(levels), batch):
        o.insert_batch(rows[i:i + b], levels[i:i + b], np.arange(i, i + b, dtype=np.int64))
        i += b
    return o


def layer0_lists(o, n):
    return [(i,) + o.neighbors(i, 0) for i in range(n) if not o.merged(i)]


def check_both_signs(o, n):
    """<#> on N(0, 1): the layer-0 lists of the finished graph hold distances of both signs for more than half of the elements."""
    lists = layer0_lists(o, n)
    both = sum(1 for _, _, d in lists if (d < 0).any() and (d > 0).any())
    print("lists with distances of both signs: %d of %d" % (both, len(lists)))
    assert 2 * both > len(lists)


def check_cancellation(o, n, dt, metric, dim, rows):
    """offset: within every list the largest neighbour distance is less than twice the smallest, while the reference's sequential summation (SEQ) differs
    from the device's order (W64) by more than 1e-6 relative for some pair of rows -- the stored bits are the canonical order's alone."""
    tight, worst, r64, n_lists = 0, 0.0, as_f64(dt, rows), 0
    for i, ids, d in layer0_lists(o, n):
        a = np.abs(d.astype(np.float64))
        if len(a) >= 2 and a.min() > 0.0:                                                          # not duplicates of one another
            n_lists += 1
            tight += a.max() / a.min() < 2.0
        seq = orc.distances_many(dt, metric, dim, rows[i], rows, order=orc.SEQ)
        w64 = orc.distances_many(dt, metric, dim, rows[i], rows, order=orc.W64)
        assert np.array_equal(np.float32(w64[ids]).view(np.uint32), d.view(np.uint32))             # the lists hold W64 values
        ok = w64 != 0.0
        worst = max(worst, float(np.max(np.abs(seq[ok] - w64[ok]) / np.abs(w64[ok]))))
        diff = r64[i] - r64
        exact = {hx.L2SQ: (diff * diff).sum(1), hx.NEG_IP: -(r64[i] * r64).sum(1), hx.L1: np.abs(diff).sum(1)}[metric]
        assert np.allclose(w64, exact, rtol=1e-4, atol=0.0) and np.allclose(seq, exact, rtol=1e-4, atol=0.0)   # both orders are roundings of the same value
    print("lists with max / min < 2: %d of %d; largest relative SEQ - W64 difference %.3g" % (tight, n_lists, worst))
    assert n_lists > 0 and tight == n_lists
    assert worst > 1e-6


def preconditions(case, rows, levels):
    i, dt, metric, dim, kind, m, efc, n, batch, fused, dup = case
    if metric == hx.NEG_IP and KINDS[kind] == "normal":
        check_both_signs(oracle_graph(dt, metric, dim, rows, levels, m, efc, batch), n)
    if KINDS[kind] == "offset":
        check_cancellation(oracle_graph(dt, metric, dim, rows, levels, m, efc, batch), n, dt, metric, dim, rows)


def assert_scans(e, ix, o, qs, n, efs, k):
    """Top-k, then a relaxed and a strict iterative scan with a filter: TIDs and distance bits of the oracle's amgettuple stream."""
    nq = len(qs)
    e.set_queries(qs)
    tids, d, _, cnt = ix.search(nq, efs, k)
    passes = (np.arange(n) % 3 != 1).astype(np.uint8)
    for q in range(nq):
        want = o.scan(qs[q], ef_search=efs, limit=k)
        assert cnt[q] == len(want) and tids[q, :cnt[q]].tolist() == [t for t, _, _ in want], q
        assert np.array_equal(d[q, :cnt[q]].view(np.uint32), np.float32([x for _, x, _ in want]).view(np.uint32)), q
    for mode, it in ((1, orc.ITER_RELAXED), (2, orc.ITER_STRICT)):
        got = ix.search_iterative(nq, efs, mode, 500, 7, passes)
        for q in range(nq):
            want = [(t, x) for t, x, _ in o.scan(qs[q], ef_search=efs, iterative=it, max_scan_tuples=500) if passes[t]][:7]
            c = int(got[2][q])
            assert got[0][q, :c].tolist() == [t for t, _ in want], (mode, q)
            assert np.array_equal(got[1][q, :c].view(np.uint32), np.float32([x for _, x in want]).view(np.uint32)), (mode, q)


def _id(c):
    return "s%d-t%d-op%d-d%d-%s-M%d-e%d-n%d-b%d-%s-dup%d" % (c[0], c[1], c[2], c[3], KINDS[c[4]], c[5], c[6], c[7], c[8], "fused" if c[9] else "lockstep", c[10])


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_signed_and_wide_range_rows_match_oracle(case):
    i, dt, metric, dim, kind, m, efc, n, batch, fused, dup = case
    rows, qs, levels = case_data(case)
    preconditions(case, rows, levels)                                                              # on the oracle alone, before any device call
    e, ix, elem, o, oelem = build_both(dt, metric, dim, rows, levels, m, efc, batch, bool(fused))
    assert elem.tolist() == oelem.tolist()
    if fused:
        assert ix.fused_stats()["redone"] <= int((levels >= 8).sum())
    assert_same_graph(ix, o, n)
    ix.set_fused(True)
    assert_scans(e, ix, o, qs, n, max(10, m), 6)
    ix.close()
    e.close()


ONDISK = [(hx.F32, hx.NEG_IP, 33, 8, 32), (hx.F32, hx.L1, 129, 20, 48), (hx.F16, hx.NEG_IP, 65, 8, 32)]


@pytest.mark.parametrize("dt,metric,dim,m,efc", ONDISK, ids=["vector-ip", "vector-l1", "halfvec-ip"])
def test_signed_rows_through_aminsert_and_vacuum(dt, metric, dim, m, efc):
    """N(0, 1) rows: a batched build, 200 aminserts, a VACUUM of 10 % of the elements, aminserts again.  One insert at a time is the reference's schedule:
    graph, heap TIDs and deleted flags are the oracle's after every step.  The same steps in concurrent groups (which the oracle does not restate) leave the
    same graph on the traversal-kernel placement and on the lock-step driver."""
    rng = np.random.default_rng(900 + dim)
    n0, n1, n2 = 500, 200, 100
    n = n0 + n1 + n2
    data = make_data("normal", dt, n + NQ, dim, rng)
    rows, qs = np.ascontiguousarray(data[:n]), np.ascontiguousarray(data[n:])
    rows[n0 + 10] = rows[5]
    rows[n0 + n1 + 3] = rows[n0 + 20]
    levels = hx.draw_levels(n, m, seed=900 + dim)
    dead = np.sort(rng.choice(n0 + n1, (n0 + n1) // 10, replace=False)).astype(np.int64)
    if metric == hx.NEG_IP:                                                                        # on the oracle alone: this graph's search streams cross zero
        o0 = oracle_graph(dt, metric, dim, rows[:n0], levels[:n0], m, efc, 64)
        crossing = 0
        for q in range(NQ):
            s = np.array([x for _, x, _ in o0.scan(qs[q], ef_search=40, iterative=orc.ITER_RELAXED, max_scan_tuples=400)])
            crossing += (s < 0).any() and (s > 0).any()
        assert 4 * crossing >= NQ

    # one at a time, against the oracle
    e = hx.Engine(dt, metric, dim, n)                                                              # as build_both, with room for the rows to come
    e.append(rows)
    ix = hx.Index(e, m, efc)
    ix.insert(0, levels[:n0], batch=64)
    o = oracle_graph(dt, metric, dim, rows[:n0], levels[:n0], m, efc, 64)
    o.set_ondisk_tombstones(True)
    assert_same_graph(ix, o, n0)
    ix.insert_ondisk(n0, levels[n0:n0 + n1], batch=1)
    for i in range(n0, n0 + n1):
        o.insert_on_disk(rows[i], int(levels[i]), i)
    assert_same_graph(ix, o, n0 + n1)
    ix.vacuum(dead, batch=1)
    o.vacuum(dead)
    assert [ix.deleted(i) for i in range(n0 + n1)] == [o.deleted(i) for i in range(n0 + n1)]
    assert_same_graph(ix, o, n0 + n1)
    ix.insert_ondisk(n0 + n1, levels[n0 + n1:], batch=1)
    for i in range(n0 + n1, n):
        o.insert_on_disk(rows[i], int(levels[i]), i)
    assert_same_graph(ix, o, n)
    e.set_queries(qs)
    tids, d, _, cnt = ix.search(NQ, 40, 10)
    dead_set = set(dead.tolist())
    for q in range(NQ):
        want = o.scan(qs[q], ef_search=40, limit=10)
        assert tids[q, :cnt[q]].tolist() == [t for t, _, _ in want] and not (set(tids[q, :cnt[q]].tolist()) & dead_set)
        assert np.array_equal(d[q, :cnt[q]].view(np.uint32), np.float32([x for _, x, _ in want]).view(np.uint32))
    ix.close()
    e.close()

    # concurrent groups: both placements, step by step
    def snapshot(ix, size):
        lv = ix.export_levels()
        out = [lv.copy(), ix.entry, [ix.heaptids(i) for i in range(size)], [ix.deleted(i) for i in range(size)]]
        for l in range(int(max(lv.max(), 0)) + 1):
            ids, dd, c = ix.export_layer(l)
            valid = np.arange(ids.shape[1])[None, :] < c[:, None]
            out.append((c.copy(), np.where(valid, ids, 0), np.where(valid, dd.view(np.uint32), 0)))
        return out

    def same_snapshot(a, b):
        assert np.array_equal(a[0], b[0]) and a[1:4] == b[1:4] and len(a) == len(b)
        for x, y in zip(a[4:], b[4:]):
            assert all(np.array_equal(p, r) for p, r in zip(x, y))

    steps = {}
    for fused in (True, False):
        e = hx.Engine(dt, metric, dim, n)
        e.append(rows)
        ix = hx.Index(e, m, efc)
        ix.insert(0, levels[:n0], batch=64)
        ix.set_fused(fused)
        snaps = []
        ix.insert_ondisk(n0, levels[n0:n0 + 120], batch=16)
        ix.insert_ondisk(n0 + 120, levels[n0 + 120:n0 + n1], batch=10)
        snaps.append(snapshot(ix, n0 + n1))
        ix.vacuum(dead, batch=1)
        snaps.append(snapshot(ix, n0 + n1))
        ix.insert_ondisk(n0 + n1, levels[n0 + n1:], batch=25)
        snaps.append(snapshot(ix, n))
        steps[fused] = snaps
        ix.close()
        e.close()
    for a, b in zip(steps[True], steps[False]):
        same_snapshot(a, b)
