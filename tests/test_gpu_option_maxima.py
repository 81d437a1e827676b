"""Builds, scans, aminsert and vacuum at the LARGEST legal option values and on both sides of every size at which the code changes
its path between the sizes the rest of the suite runs and those maxima:

  ef_construction (4..1000, options.rs:203-225)
      256 | 257   the matrix-core select of halfvec inner-product builds serves W <= 256 (hx_index.cpp: hx_index_dbatch_search)
      512 | 513   the members' W tables (hx_batch.hip: db_begin_wtabs) exist up to 512 -- the fullest 1024-entry table -- and are off above:
                  the back-link kernels then stream rows instead of looking d(new, x) up
      600         8-chunk rows: the largest `clds` term of the traversal kernel's insert mode (hx_fused.inc.h: fused_launch)
      1000        the maximum: W[ef + 2] EP[ef + 2] in LDS, `+ 254` for repair searches, k_select_w at its last legal stride (hx_biglist.hip)
  ef_search (1..1000, options.rs:156-166)
      256 | 257   the limit of the HX_SORTED_ARRAY experiment (compiled out of the default build: only the setting's harmlessness is checked)
      512, 513, 1000 with k = ef_search tuples per query

Every expected value -- graphs, levels, heap TIDs, neighbour ids, distance bits, scan TIDs -- is the oracle's in the device's canonical
summation order (orc.W64); every comparison is equality.  What the data is meant to do (a result set W that really fills to
ef_construction) is asserted on the oracle alone before the device is touched."""
import time

import numpy as np
import pytest

import pgvector_rx_amd as hx
from oracle import orc
import test_gpu_scan_filtered as sf
from test_gpu_index import assert_same_graph, build_device, build_oracle, device_batches_two_rank_simulation, make_rows

pytestmark = pytest.mark.gpu


def w_fills(o, rows, efc):
    """On the oracle alone: the layer-0 search of the last inserted member, from the entry point, returns ef_construction candidates."""
    n = o.size
    member = next(i for i in range(n - 1, -1, -1) if not o.merged(i))
    ids, _ = o.search_layer_raw(rows[member], [o.entry], efc, 0)
    return len(ids) == efc


def same_scan(got, o, qs, ef, limit):
    tids, d, _, cnt = got
    for q in range(len(qs)):
        want = o.scan(qs[q], ef_search=ef, limit=limit)
        assert cnt[q] == len(want), (q, cnt[q], len(want))                       # the oracle's count: inner-product scans may return fewer than ef
        assert tids[q, :cnt[q]].tolist() == [t for t, _, _ in want], q
        assert np.array_equal(d[q, :cnt[q]].view(np.uint32), np.float32([x for _, x, _ in want]).view(np.uint32)), q


# ---- A1. builds across the W-table switch, the matrix-core select's limit and at the maximum ---------------------------------------------------
# (type, metric, dim, n, m, efc, batch, fused)
# Rows are uniform in [0, 1) as in test_gpu_index.py, but for halfvec(4000) inner product at m = 4: there the high-norm rows are everybody's
# neighbours, only 398 of the 700 elements can be reached from the entry point (measured on the oracle) and W never holds 600; N(0, 1) rows
# of near-equal norm keep the graph connected and W fills.
BUILDS = [
    (hx.F32, hx.L2SQ, 8, 700, 16, 512, 64, True),        # the fullest W table ...
    (hx.F32, hx.L2SQ, 8, 700, 16, 513, 64, True),        # ... and the first size without one: same rows, same levels.  That the tables are OFF here is not
                                                         # visible in a graph (both sizes equal their oracle either way): test_two_rank_device_batches_with_the_w_tables_off asserts it
    (hx.F32, hx.L2SQ, 8, 1200, 16, 1000, 64, True),
    (hx.F32, hx.L2SQ, 8, 1200, 16, 1000, 1, True),       # no device batch: the sequential schedule
    (hx.F32, hx.NEG_IP, 12, 1200, 32, 1000, 100, True),   # 64-slot lists, the largest the insert mode's select serves
    (hx.F32, hx.L2SQ, 8, 1180, 33, 1000, 128, True),      # k_select_w at a stride of 1000, its last legal value
    (hx.BIT, hx.HAMMING, 64, 1150, 100, 1000, 64, True),  # largest m, largest ef_construction, ties everywhere
    (hx.F32, hx.L1, 2000, 700, 4, 600, 37, True),        # 8-chunk rows, the largest `clds` term
    (hx.F16, hx.NEG_IP, 4000, 700, 4, 600, 37, True),
    (hx.F16, hx.NEG_IP, 300, 600, 16, 256, 64, True),     # the last size of the matrix-core select ...
    (hx.F16, hx.NEG_IP, 300, 600, 16, 257, 64, True),    # ... and the first that must take the exact select
    (hx.F32, hx.L2SQ, 6, 1150, 8, 1000, 37, False),      # the lock-step driver at the maximum
]


@pytest.mark.parametrize("dtype,metric,dim,n,m,efc,batch,fused", BUILDS,
                         ids=["t%d-%d-d%d-n%d-m%d-efc%d-b%d-%s" % (c[0], c[1], c[2], c[3], c[4], c[5], c[6], "fused" if c[7] else "lockstep") for c in BUILDS])
def test_builds_at_the_ef_construction_switches_and_maximum(dtype, metric, dim, n, m, efc, batch, fused):
    """Graph, levels, heap TIDs, neighbour ids and distance bits equal the oracle's; the searches were device tasks (tasks > 0) and at most a
    tenth of them was redone by the lock-step driver (the cap of test_graph_identical_to_oracle).  Measured on an MI355X: redone == 0 and
    rounds == 0 in every fused case."""
    rng = np.random.default_rng(dim + m)                        # not a function of efc: 512 / 513 and 256 / 257 share rows and levels
    rows = sf.make_rows(dtype, n, dim, rng, "normal") if (dtype, dim) == (hx.F16, 4000) else make_rows(dtype, n, dim, rng)
    levels = hx.draw_levels(n, m, seed=6)
    t0 = time.perf_counter()
    o, oelem = build_oracle(dtype, metric, dim, rows, levels, m, efc, batch)
    t_oracle = time.perf_counter() - t0
    assert n > efc and w_fills(o, rows, efc)                    # W fills to ef_construction: checked before the device is touched
    e, ix, elem = build_device(dtype, metric, dim, rows, levels, m, efc, batch, fused, mfma=True if (dtype, metric) == (hx.F16, hx.NEG_IP) else None)
    assert elem.tolist() == oelem.tolist()
    assert_same_graph(ix, o, n)
    st, rounds, mf = ix.fused_stats(), ix.profile()["rounds"], ix.mfma_stats()
    print("\nefc %d m %d batch %d: tasks %d redone %d lock-step rounds %d mfma_pairs %d; the oracle's build took %.2f s" % (
        efc, m, batch, st["tasks"], st["redone"], rounds, mf["mfma_pairs"], t_oracle))
    assert (st["tasks"] > 0) == fused and st["redone"] <= st["tasks"] // 10
    if fused:
        assert rounds == 0                                      # nothing fell back to lock-step rounds (the run on an MI355X showed 0 in every fused case)
    if dtype == hx.F16 and dim == 300:
        assert (mf["mfma_pairs"] > 0) == (efc <= 256)
    ix.close()
    e.close()


def test_two_rank_device_batches_with_the_w_tables_off():
    """The device-resident two-rank exchange at ef_construction 600: no W tables inside an open device batch (hx_index_dbatch_wtab_bytes == 0), the
    back-link kernels stream rows, and both replicas equal the oracle's graph."""
    n_dev, wtab_bytes = device_batches_two_rank_simulation(600, n=1500)
    assert n_dev >= 3
    assert len(wtab_bytes) == 2 * n_dev and all(b == 0 for b in wtab_bytes)


# ---- A2. scans at ef_search 256 | 257, 512 | 513 and 1000 with k = ef_search --------------------------------------------------------------------
NQ = 16
SCAN_SHAPES = [(hx.F32, hx.L2SQ, 8), (hx.F16, hx.NEG_IP, 40), (hx.BIT, hx.HAMMING, 64), (hx.SPARSE, hx.L2SQ, 300)]


class Scans(sf.Setup):
    """test_gpu_scan_filtered.Setup's reference (`expected`: the oracle's amgettuple stream filtered as the executor would) on a graph of this
    module's shape and at this module's ef_search."""

    def __init__(self, dt, metric, dim):
        rng = np.random.default_rng(dim + 1000)
        n, m, efc = 3000, 12, 48
        batch = 1 if dt == hx.SPARSE else 256                   # sparsevec builds: the schedule of tests/test_gpu_sparse.py
        self.dt, self.metric, self.n, self.ef = dt, metric, n, 1000
        rows = sf.make_rows(dt, n, dim, rng)
        levels = hx.draw_levels(n, m, seed=5)
        self.o, _ = build_oracle(dt, metric, dim, rows, levels, m, efc, batch)
        self.qs = sf.make_rows(dt, NQ, dim, rng)
        self._streams = {}
        self.e = hx.Engine(dt, metric, dim, n)
        self.e.append(rows)
        self.ix = hx.Index(self.e, m, efc)
        self.ix.insert(0, levels, batch=batch)
        assert_same_graph(self.ix, self.o, n)
        self.e.set_queries(self.qs)
        t = np.arange(n)
        self.filters = [(t % 7 == 0).astype(np.uint8), (t % 7 == 3).astype(np.uint8)]
        self.filter_of = np.array([(q % 3) - 1 for q in range(NQ)], np.int32)                 # none, the first, the second

    def stream(self, q, mode, max_tuples=20000):
        key = (q, mode, max_tuples)
        if key not in self._streams:
            it = orc.ITER_RELAXED if mode == 1 else orc.ITER_STRICT
            self._streams[key] = self.o.scan(self.qs[q], ef_search=self.ef, iterative=it, max_scan_tuples=max_tuples)
        return self._streams[key]


@pytest.fixture(scope="module", params=SCAN_SHAPES, ids=["vector-l2", "halfvec-ip", "bit-hamming", "sparsevec-l2"])
def scans(request):
    s = Scans(*request.param)
    yield s
    s.close()


@pytest.mark.parametrize("ef", [257, 512, 513, 1000])
def test_scan_returning_ef_search_tuples(scans, ef):
    s = scans
    before = s.ix.fused_stats()
    got = s.ix.search(NQ, ef, ef)
    after = s.ix.fused_stats()
    assert after["tasks"] == before["tasks"] + NQ and after["redone"] == before["redone"]     # served by the traversal kernel
    same_scan(got, s.o, s.qs, ef, ef)


@pytest.mark.parametrize("mode", [1, 2])
def test_iterative_scan_at_ef_search_1000(scans, mode):
    s, limit = scans, 50
    passes = s.filters[0]                                        # 1 in 7
    before = s.ix.fused_stats()
    tids, d, cnt = s.ix.search_iterative(NQ, 1000, mode, 20000, limit, passes)
    after = s.ix.fused_stats()
    assert after["tasks"] == before["tasks"] + NQ and after["redone"] == before["redone"]
    for q in range(NQ):
        want = [(t, x) for t, x, _ in s.stream(q, mode) if passes[t]][:limit]
        assert cnt[q] == len(want), q
        assert tids[q, :cnt[q]].tolist() == [t for t, _ in want], q
        assert np.array_equal(d[q, :cnt[q]].view(np.uint32), np.float32([x for _, x in want]).view(np.uint32)), q


def test_filtered_scan_at_ef_search_1000(scans):
    """Two filters and a `<` radius per query at about its median distance, strict order: the oracle's stream filtered as the executor would."""
    s, limit, mode = scans, 50, 2
    radius = np.empty(NQ, np.float64)
    for q in range(NQ):
        v = np.sort(np.array([sf.op_value(s.metric, x) for _, x, _ in s.stream(q, mode)], np.float64))
        radius[q] = v[len(v) // 2]
    before = s.ix.fused_stats()
    got = s.ix.search_filtered(NQ, 1000, mode, 20000, limit, filters=s.filters, filter_of=s.filter_of, cmp=hx.CMP_LT, radius=radius)
    after = s.ix.fused_stats()
    assert after["tasks"] == before["tasks"] + NQ and after["redone"] == before["redone"]
    hits = 0
    for q in range(NQ):
        want = s.expected(q, mode, hx.CMP_LT, radius, limit=limit)
        c = int(got[3][q])
        hits += c
        assert c == len(want), q
        assert got[0][q, :c].tolist() == [t for t, _ in want], q
        assert np.array_equal(got[1][q, :c].view(np.uint32), np.array([x for _, x in want], np.float32).view(np.uint32)), q
    assert hits > 0


def test_pipelined_and_null_scans_at_ef_search_1000(scans):
    s, h = scans, NQ // 2
    ref = s.ix.search(NQ, 1000, 1000)
    s.ix.search_submit(0, 0, h, 1000, 1000)
    s.ix.search_submit(1, h, NQ - h, 1000, 1000)
    got0, got1 = s.ix.search_wait(0), s.ix.search_wait(1)
    for a, b, r in zip(got0, got1, ref):
        assert np.array_equal(a, r[:h]) and np.array_equal(b, r[h:])
    tids, _ = s.ix.search_null(1000, 1000)
    assert tids.tolist() == [t for t, _, _ in s.o.scan(None, ef_search=1000, limit=1000)]


@pytest.mark.parametrize("ef", [256, 257])
def test_sorted_array_setting_changes_nothing_in_the_default_build(scans, ef, monkeypatch):
    """HX_SORTED_ARRAY=1 selects the sorted-array search (ef_search <= 256) only in a library compiled with HX_CFLAGS=-DHX_EXPERIMENTS
    (hx_fused.inc.h: sa_env_on); the build this suite runs compiles it out, so BOTH calls below are the heap kernel.  What is checked is only
    that the setting disturbs nothing at 256 and 257: the same outputs, the oracle's answers, nothing redone.  The `ef <= 256` limit of the
    experiment itself and its K = (ef + 63) >> 6 sizing are NOT covered here: no counter tells the two kernels apart, and a test cannot
    rebuild the library with the experiment in."""
    s = scans
    ref = s.ix.search(NQ, ef, ef)
    redone = s.ix.fused_stats()["redone"]
    monkeypatch.setenv("HX_SORTED_ARRAY", "1")
    got = s.ix.search(NQ, ef, ef)
    monkeypatch.delenv("HX_SORTED_ARRAY")
    assert s.ix.fused_stats()["redone"] == redone
    for a, b in zip(ref, got):
        assert np.array_equal(a, b)
    same_scan(got, s.o, s.qs, ef, ef)


def test_ef_search_outside_its_range_is_refused(scans):
    s = scans
    for ef in (0, 1001):
        for call in (lambda: s.ix.search(NQ, ef, 10),
                     lambda: s.ix.search_iterative(NQ, ef, 1, 20000, 10),
                     lambda: s.ix.search_iterative(NQ, ef, 2, 20000, 10, s.filters[0]),
                     lambda: s.ix.search_submit(0, 0, NQ, ef, 10),
                     lambda: s.ix.search_null(ef, 10)):
            with pytest.raises(hx.HxError) as ei:
                call()
            assert ei.value.code == -1, ef
    assert s.ix.search(NQ, 1000, 10)[3].tolist() == [10] * NQ                                 # nothing was left in flight or half done


# ---- A3. aminsert and vacuum at ef_construction 1000 ---------------------------------------------------------------------------------------------
def graph_of(ix, n):
    lv = ix.export_levels()
    layers = [ix.export_layer(l) for l in range(int(max(lv.max(), 0)) + 1)]
    out = [lv, np.int64(ix.entry), np.array([ix.deleted(i) for i in range(n)])]
    for ids, d, cnt in layers:
        valid = np.arange(ids.shape[1])[None, :] < cnt[:, None]
        out += [cnt, np.where(valid, ids, 0), np.where(valid, d.view(np.uint32), 0)]
    return out


def well_formed(ix, o, dtype, metric, dim, rows, n, n_vacuumed, m, dead, nd):
    """What holds for any schedule: deleted flags are the oracle's (an element dies with its last heap TID), no list of a live element names a
    deleted or merged element, itself or an element twice, lists respect 2m / m and their layer, and every stored distance is the oracle's
    distance of that pair, bit for bit."""
    flags = [ix.deleted(i) for i in range(n)]
    assert flags[:n_vacuumed] == [o.deleted(i) for i in range(n_vacuumed)] and not any(flags[n_vacuumed:]) and nd == sum(flags)
    dead = set(dead.tolist())
    lists = 0
    for i in range(n):
        lv = ix.level(i)
        assert (lv < 0) == bool(o.merged(i)), i
        if lv < 0 or flags[i]:
            continue
        assert ix.heaptids(i) and not (set(ix.heaptids(i)) & dead), i
        for layer in range(lv + 1):
            ids, d = ix.neighbors(i, layer)
            assert len(ids) <= (2 * m if layer == 0 else m) and len(set(ids.tolist())) == len(ids) and i not in ids, (i, layer)
            assert all(ix.level(int(j)) >= layer and not flags[int(j)] for j in ids), (i, layer)
            want = np.float32(orc.distances_many(dtype, metric, dim, rows[i], rows, ids.astype(np.int32), orc.W64))
            assert np.array_equal(d.view(np.uint32), want.view(np.uint32)), (i, layer)
            lists += 1
    assert lists >= n - len(dead) - 5


def live_scan(got, dtype, metric, dim, rows, qs, n, dead):
    """A scan of 1000 tuples on more than 1000 live ones: 1000 distinct live TIDs per query, ascending, each with the oracle's distance bits."""
    tids, d, _, cnt = got
    dead = set(dead.tolist())
    assert n - len(dead) > 1000
    for q in range(len(qs)):
        t = tids[q, :cnt[q]]
        assert cnt[q] == 1000 and len(set(t.tolist())) == 1000 and not (set(t.tolist()) & dead), q
        want = np.float32(orc.distances_many(dtype, metric, dim, qs[q], rows, t.astype(np.int32), orc.W64))
        assert np.array_equal(d[q, :cnt[q]].view(np.uint32), want.view(np.uint32)) and (np.diff(d[q, :cnt[q]]) >= 0).all(), q


@pytest.mark.parametrize("dtype,metric,dim,n0,m", [(hx.F32, hx.L2SQ, 4, 1200, 8), (hx.BIT, hx.HAMMING, 40, 1100, 40)], ids=["vector-m8", "bit-m40"])
def test_aminsert_and_vacuum_at_ef_construction_1000(dtype, metric, dim, n0, m):
    """The procedure of test_ondisk_insert_identical_to_oracle and test_vacuum_identical_to_oracle at the maximum: n0 rows built, 100 inserted through
    aminsert (k_update_runs; m = 40: k_update_runs_big), a tenth vacuumed (repair searches with the skip set: wcap = ef + 2 + 254), 50 more inserted.
    One at a time -- the reference's and the oracle's schedule -- graph, deleted flags and a scan of 1000 tuples equal the oracle's after every
    step.  With 37 concurrent aminserts and 64 concurrent repairs there is no oracle to follow (the members search one snapshot): there, on both
    shapes, the graph must be well formed with the oracle's value in every slot, deleted flags the oracle's and a scan of 1000 live tuples exact;
    on m = 8 the device placement must also leave the graph the lock-step placement leaves (lists of more than 64 slots have none)."""
    efc, n1, n2 = 1000, 100, 50
    n = n0 + n1 + n2
    rng = np.random.default_rng(dim + m)
    rows = make_rows(dtype, n, dim, rng)
    rows[n0 + 7] = rows[17]                                      # a duplicate through find_duplicate_on_disk
    levels = hx.draw_levels(n, m, seed=9)
    qs = make_rows(dtype, 16, dim, rng)
    dead = rng.choice(n0 + n1, (n0 + n1) // 10, replace=False).astype(np.int64)
    o, _ = build_oracle(dtype, metric, dim, rows[:n0], levels[:n0], m, efc, 64, tombstones=True)
    assert w_fills(o, rows, efc)

    def device(fused=True):
        e = hx.Engine(dtype, metric, dim, n)
        e.append(rows)
        ix = hx.Index(e, m, efc)
        ix.insert(0, levels[:n0], batch=64)
        ix.set_fused(fused)
        e.set_queries(qs)
        return e, ix

    def same_as_oracle(ix, e, size):
        assert [ix.deleted(i) for i in range(size)] == [o.deleted(i) for i in range(size)]
        assert_same_graph(ix, o, size)
        same_scan(ix.search(16, 1000, 1000), o, qs, 1000, 1000)

    e, ix = device()
    before = ix.fused_stats()
    elem = ix.insert_ondisk(n0, levels[n0:n0 + n1], batch=1)
    oelem = [o.insert_on_disk(rows[i], int(levels[i]), i) for i in range(n0, n0 + n1)]
    assert elem.tolist() == oelem
    after = ix.fused_stats()
    assert after["tasks"] - before["tasks"] >= n1 - 1 and after["redone"] <= after["tasks"] // 10
    same_as_oracle(ix, e, n0 + n1)
    tasks = after["tasks"]
    nd, nr = ix.vacuum(dead, batch=1)
    st = ix.fused_stats()
    print("\nrepair searches on the device: %d, redone by the lock-step driver so far: %d" % (st["tasks"] - tasks, st["redone"]))
    assert st["tasks"] > tasks and nr > 0
    o.vacuum(dead)
    assert nd == sum(o.deleted(i) for i in range(n0 + n1))
    same_as_oracle(ix, e, n0 + n1)
    elem = ix.insert_ondisk(n0 + n1, levels[n0 + n1:], batch=1)
    oelem = [o.insert_on_disk(rows[i], int(levels[i]), i) for i in range(n0 + n1, n)]
    assert elem.tolist() == oelem
    same_as_oracle(ix, e, n)
    ix.close()
    e.close()
    # 37 concurrent aminserts, 64 concurrent repairs: no oracle follows this schedule.  Checked on every shape: the graph is well formed and every
    # stored value is the oracle's; on m = 8 also: the lock-step placement leaves the same graph (lists of more than 64 slots have none).
    graphs = []
    for fused in ((True, False) if m <= 32 else (True,)):
        e, ix = device(fused)
        before = ix.fused_stats()
        el1 = ix.insert_ondisk(n0, levels[n0:n0 + n1], batch=37)
        nd, nr = ix.vacuum(dead, batch=64)
        el2 = ix.insert_ondisk(n0 + n1, levels[n0 + n1:], batch=37)
        st = ix.fused_stats()
        got = ix.search(16, 1000, 1000)
        if fused:
            print("batches of 37 / 64: device tasks %d, redone %d" % (st["tasks"] - before["tasks"], st["redone"]))
            assert st["tasks"] - before["tasks"] >= n1 + n2 - 2 and st["redone"] <= st["tasks"] // 10 and nr > 0
            well_formed(ix, o, dtype, metric, dim, rows, n, n0 + n1, m, dead, nd)
            live_scan(got, dtype, metric, dim, rows, qs, n, dead)
        graphs.append([el1, el2] + graph_of(ix, n) + list(got))
        ix.close()
        e.close()
    for a, b in zip(*graphs) if len(graphs) == 2 else ():
        assert np.array_equal(a, b)
