"""Filter sets (hx_filterset_*) and the two scans that take one (hx_exact_search_set, hx_exact_range_set).  A set's contents are checked against
numpy (filter f = the ascending row ids whose label is f); the scans against their definition: the bytes of hx_exact_search_filtered /
hx_exact_range_filtered called with the set's row range and the bitmaps the set represents."""
import ctypes

import numpy as np
import pytest

import pgvector_rx_amd as hx
from test_gpu_exact_filtered import engine, interleaved, make
from test_gpu_exact_range_filtered import radii_of

E_ARG, E_NOMEM, E_STATE = -1, -3, -6
NO = hx.NO_LABEL
P = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)   # noqa: E731


def draw_labels(n, L, rng, null=0.1):
    """n labels below L; label L // 2 never occurs (L >= 3) and about `null` of the rows are in no filter"""
    pool = np.array([f for f in range(L) if L < 3 or f != L // 2], np.uint32)
    lb = pool[rng.integers(0, len(pool), n)]
    lb[rng.random(n) < null] = NO
    return lb


def lists_of(labels, L, first_row):
    order = np.argsort(labels, kind="stable")
    cut = np.searchsorted(labels[order], np.arange(L + 1))
    return [(order[cut[f]:cut[f + 1]] + first_row).astype(np.uint32) for f in range(L)]


def check_set(fs, want, first_row, n_rows):
    info = fs.info()
    assert (info["first_row"], info["n_rows"], info["n_filters"]) == (first_row, n_rows, len(want))
    assert info["n_listed"] == sum(len(w) for w in want)
    assert fs.counts().tolist() == [len(w) for w in want]
    for f, w in enumerate(want):
        got = fs.read(f)
        assert got.dtype == np.uint32 and got.tolist() == w.tolist(), f


def masks_of(labels, L):
    return [labels == f for f in range(L)]


@pytest.fixture(scope="module")
def store():
    """70 100 rows of vector(3): the rows the content tests label"""
    e = hx.Engine(hx.F32, hx.L2SQ, 3, 80000)
    e.append(np.random.default_rng(5).standard_normal((70100, 3)).astype(np.float32))
    yield e
    e.close()


# ---- 1. contents ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("L", [1, 2, 64, 65, 300, 5000])
def test_contents_from_labels(store, L, device):
    """4 099 rows from row 37: no multiple of 64 or of a tile; 1 .. 300 filters take the histogram path, 5 000 the sort path, where most lists
    have no row or one; a label that never occurs; a tenth of the rows in no filter."""
    rng = np.random.default_rng(100 + L)
    n, first = 4099, 37
    lb = draw_labels(n, L, rng)
    if device:
        import torch
        t = torch.from_numpy(lb.view(np.int32)).cuda()
        torch.cuda.synchronize()
        fs = hx.FilterSet.from_labels(store, None, L, first_row=first, device_ptr=t.data_ptr(), n_rows=n)
    else:
        fs = hx.FilterSet.from_labels(store, lb, L, first_row=first)
    check_set(fs, lists_of(lb, L, first), first, n)
    fs.close()


@pytest.mark.gpu
@pytest.mark.parametrize("L", [3, 2000])
def test_contents_edge_shapes(store, L):
    one = np.full(4099, 1, np.uint32)                           # every row in one label
    fs = hx.FilterSet.from_labels(store, one, L, first_row=37)
    check_set(fs, lists_of(one, L, 37), 37, 4099)
    fs.close()
    fs = hx.FilterSet.from_labels(store, np.empty(0, np.uint32), L, first_row=5)   # no row
    check_set(fs, [np.empty(0, np.uint32)] * L, 5, 0)
    fs.close()
    none = np.full(200, NO, np.uint32)                          # every row in no filter
    fs = hx.FilterSet.from_labels(store, none, L)
    check_set(fs, [np.empty(0, np.uint32)] * L, 0, 200)
    fs.close()


@pytest.mark.gpu
@pytest.mark.parametrize("L", [7, 1500])
def test_contents_many_tiles(store, L):
    """70 000 rows: dozens of wave tiles in several workgroups contribute to one list"""
    lb = draw_labels(70000, L, np.random.default_rng(L))
    fs = hx.FilterSet.from_labels(store, lb, L)
    check_set(fs, lists_of(lb, L, 0), 0, 70000)
    fs.close()


@pytest.mark.gpu
def test_contents_from_bitmaps(store):
    """two overlapping 10 % filters, an all-zero one, a NULL one; stray bits past n_rows in the last word"""
    rng = np.random.default_rng(9)
    n, first = 4099, 37
    masks = [rng.random(n) < 0.1, rng.random(n) < 0.1, np.zeros(n, bool), None]
    masks[1][:50] = masks[0][:50]
    words = []
    for m in masks:
        if m is None:
            words.append(None)
            continue
        bits = np.ones((n + 63) // 64 * 64, np.uint8)           # every bit past n_rows is set
        bits[:n] = m
        words.append(np.packbits(bits, bitorder="little").view(np.uint64))
    fs = hx.FilterSet.from_bitmaps(store, words, n_rows=n, first_row=first, packed=True)
    want = [(np.flatnonzero(m) + first).astype(np.uint32) if m is not None else np.empty(0, np.uint32) for m in masks]
    check_set(fs, want, first, n)
    fs.close()
    fs = hx.FilterSet.from_bitmaps(store, masks, n_rows=n, first_row=first)
    check_set(fs, want, first, n)
    fs.close()


# ---- 2. append ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("L,from_bitmaps", [(65, False), (1500, False), (65, True)])
def test_append(store, L, from_bitmaps):
    rng = np.random.default_rng(L)
    n0, first = 1000, 37
    lb = draw_labels(n0 + 1 + 63 + 3000, L, rng)
    fs = hx.FilterSet.from_bitmaps(store, masks_of(lb[:n0], L), n_rows=n0, first_row=first) if from_bitmaps else \
        hx.FilterSet.from_labels(store, lb[:n0], L, first_row=first)
    n = n0
    for step in (0, 1, 63, 3000):
        fs.append_labels(lb[n:n + step])
        n += step
        check_set(fs, lists_of(lb[:n], L, first), first, n)
        whole = hx.FilterSet.from_labels(store, lb[:n], L, first_row=first)
        assert fs.counts().tolist() == whole.counts().tolist() and all((fs.read(f) == whole.read(f)).all() for f in range(L))
        whole.close()
    with pytest.raises(hx.HxError) as ei:                      # the rows must be in the engine
        fs.append_labels(np.zeros(store.num_rows - first - n + 1, np.uint32))
    assert ei.value.code == E_ARG
    fs.close()


# ---- 3. errors ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("L", [64, 5000])
def test_bad_label(store, L):
    rng = np.random.default_rng(3)
    lb = draw_labels(4099, L, rng)
    bad = lb.copy()
    bad[1234] = L
    bad[3000] = L + 7                                           # a later one: the first is named
    with pytest.raises(hx.HxError) as ei:
        hx.FilterSet.from_labels(store, bad, L)
    assert ei.value.code == E_ARG and "row 1234 " in str(ei.value)
    fs = hx.FilterSet.from_labels(store, lb[:1000], L)
    want = lists_of(lb[:1000], L, 0)
    with pytest.raises(hx.HxError) as ei:
        fs.append_labels(bad[1000:])
    assert ei.value.code == E_ARG and "row 1234 " in str(ei.value)
    check_set(fs, want, 0, 1000)                                # unchanged
    fs.append_labels(lb[1000:])
    check_set(fs, lists_of(lb, L, 0), 0, 4099)
    fs.close()


@pytest.mark.gpu
def test_create_argument_errors(store):
    L, h = hx.lib(), ctypes.c_void_p()
    lb = np.zeros(8, np.uint32)
    n = store.num_rows
    for args in ((0, 8, 0), (0, 8, hx.FILTERSET_MAX_FILTERS + 1), (n - 7, 8, 2), (n + 1, 0, 2)):
        assert L.hx_filterset_create_labels(store.h, args[0], args[1], args[2], P(lb), ctypes.byref(h)) == E_ARG and not h.value
    assert L.hx_filterset_create_labels(store.h, 0, 8, 2, None, ctypes.byref(h)) == E_ARG
    assert L.hx_filterset_create_labels(store.h, 0, 8, 2, P(lb), None) == E_ARG
    assert L.hx_filterset_create_bitmaps(store.h, 0, 8, 2, None, ctypes.byref(h)) == E_ARG and not h.value


@pytest.mark.gpu
def test_distinct_filter_limit_and_foreign_set():
    rng = np.random.default_rng(4)
    n, L = 3000, 5000
    rows, qs = make(hx.F32, n, 3, rng), make(hx.F32, 65, 3, rng)
    e = engine(hx.F32, 3, hx.OP_L2, rows, qs)
    lb = rng.integers(0, 200, n).astype(np.uint32) * 25          # 200 labels in use, spread over the 5 000
    fs = hx.FilterSet.from_labels(e, lb, L)
    with pytest.raises(hx.HxError) as ei:
        e.exact_search_set(hx.OP_L2, 3, fs, np.arange(65) * 25)
    assert ei.value.code == E_ARG and "distinct" in str(ei.value)
    with pytest.raises(hx.HxError) as ei:
        e.exact_range_set(hx.OP_L2, 1.0, fs, np.arange(65) * 25)
    assert ei.value.code == E_ARG and "distinct" in str(ei.value)
    fo = np.arange(65) % 64                                      # 65 queries over 64 distinct filters
    got = e.exact_search_set(hx.OP_L2, 3, fs, fo * 25)
    want = e.exact_search_filtered(hx.OP_L2, 3, [lb == f * 25 for f in range(64)], fo)
    assert all((a.view(np.uint8) == b.view(np.uint8)).all() for a, b in zip(got, want))
    for bad in (-2, L):
        with pytest.raises(hx.HxError) as ei:
            e.exact_search_set(hx.OP_L2, 3, fs, np.full(65, bad))
        assert ei.value.code == E_ARG and "filter_of" in str(ei.value)
    with pytest.raises(hx.HxError) as ei:                      # the twin's messages
        e.exact_search_set(hx.OP_L2, 0, fs, fo)
    assert ei.value.code == E_ARG and "k must be" in str(ei.value)
    with pytest.raises(hx.HxError) as ei:
        e.exact_search_set(hx.OP_HAMMING, 3, fs, fo)
    assert ei.value.code == E_ARG and "operator" in str(ei.value)
    other = engine(hx.F32, 3, hx.OP_L2, rows, qs)
    with pytest.raises(hx.HxError) as ei:
        other.exact_search_set(hx.OP_L2, 3, fs, fo)
    assert ei.value.code == E_ARG and "another engine" in str(ei.value)
    with pytest.raises(hx.HxError) as ei:
        other.exact_range_set(hx.OP_L2, 1.0, fs, fo)
    assert ei.value.code == E_ARG
    fs.close()
    other.close()
    e.close()


@pytest.mark.gpu
def test_pop_invalidates():
    rng = np.random.default_rng(6)
    rows, qs = make(hx.F32, 500, 3, rng), make(hx.F32, 4, 3, rng)
    e = engine(hx.F32, 3, hx.OP_L2, rows, qs)
    lb = draw_labels(500, 4, rng)
    fs = hx.FilterSet.from_labels(e, lb[:400], 4)                # covers rows 0 .. 399
    fo = np.array([0, 1, 3, -1])
    e.pop(50)                                                    # rows past the coverage: still valid
    e.append(rows[450:])
    e.pop(100)
    want = e.exact_search_filtered(hx.OP_L2, 5, masks_of(lb[:400], 4), fo, n_rows=400)
    got = e.exact_search_set(hx.OP_L2, 5, fs, fo)
    assert all((a.view(np.uint8) == b.view(np.uint8)).all() for a, b in zip(got, want))
    e.append(rows[400:])
    e.pop(101)                                                   # cuts row 399 off
    e.append(rows[399:400])                                      # and the row is back
    for call in (lambda: e.exact_search_set(hx.OP_L2, 5, fs, fo), lambda: e.exact_range_set(hx.OP_L2, 1.0, fs, fo), lambda: fs.counts(),
                 lambda: fs.read(0), lambda: fs.append_labels(np.zeros(0, np.uint32))):
        with pytest.raises(hx.HxError) as ei:
            call()
        assert ei.value.code == E_STATE
    assert fs.info()["n_rows"] == 400                            # info and destroy still work
    fs.close()
    e.close()


# ---- 4. top-k equality ----------------------------------------------------------------------------------------------------------------------
def tenant_labels(n, rng):
    """six filters: about 45 %, 20 % and 10 % of the rows, one of five rows, one that occurs nowhere, one of one row; the rest in no filter"""
    lb = np.full(n, NO, np.uint32)
    u = rng.random(n)
    lb[u < 0.45] = 0
    lb[(u >= 0.45) & (u < 0.65)] = 1
    lb[(u >= 0.65) & (u < 0.75)] = 2
    lb[rng.choice(np.flatnonzero(u >= 0.8), 6, replace=False)] = np.array([3, 3, 3, 3, 3, 5], np.uint32)
    return lb


def topk_case(dtype, dim, op, ks=(1, 10, 1024), n=1500, **kw):
    rng = np.random.default_rng(31 + dim + dtype)
    fo = interleaved([5, 3, 17, 2, 2, 1], 3, rng)                # filter 3 has fewer rows than k = 10, filter 4 none
    rows, qs = make(dtype, n, dim, rng), make(dtype, len(fo), dim, rng)
    rows[n // 2:n // 2 + 300] = rows[:300]                        # duplicated rows: ties
    qs[0] = rows[7]
    lb = tenant_labels(n, rng)
    e = engine(dtype, dim, op, rows, qs, **kw)
    fs = hx.FilterSet.from_labels(e, lb, 6)
    masks = masks_of(lb, 6)
    for k in ks:
        for f in (fo, None, np.full(len(fo), 2), np.full(len(fo), 4), np.where(fo == 4, 4, -1)):
            got = e.exact_search_set(op, k, fs, f)
            want = e.exact_search_filtered(op, k, masks, f)
            for j, name in enumerate(("ids", "dist", "counts")):
                assert got[j].shape == want[j].shape and (got[j].view(np.uint8) == want[j].view(np.uint8)).all(), (op, k, name)
    got = e.exact_search_set(op, 5, fs, fo[4:9], first_query=4, nq=5)
    want = e.exact_search_filtered(op, 5, masks, fo[4:9], first_query=4, nq=5)
    assert all((a.view(np.uint8) == b.view(np.uint8)).all() for a, b in zip(got, want))
    fs.close()
    e.close()


@pytest.mark.gpu
@pytest.mark.parametrize("dtype,dim,op", [(hx.F32, 3, hx.OP_L2), (hx.F32, 200, hx.OP_L2), (hx.F16, 16, hx.OP_L2), (hx.BIT, 70, hx.OP_HAMMING),
                                          (hx.SPARSE, 100, hx.OP_L2), (hx.F32, 3, hx.OP_NEG_IP), (hx.F32, 3, hx.OP_COSINE)], ids=str)
def test_topk_equals_the_filtered_call(dtype, dim, op):
    topk_case(dtype, dim, op, ks=(1, 10, 1024) if dim != 200 and dtype != hx.SPARSE else (10,))


@pytest.mark.gpu
def test_topk_row_range_and_bitmap_set():
    """a set over rows 37 .. from overlapping bitmaps"""
    rng = np.random.default_rng(8)
    n, first = 1200, 37
    fo = interleaved([4, 9], 2, rng)
    rows, qs = make(hx.F32, n + first + 10, 5, rng), make(hx.F32, len(fo), 5, rng)
    e = engine(hx.F32, 5, hx.OP_L2, rows, qs)
    masks = [rng.random(n) < 0.3, rng.random(n) < 0.3]
    fs = hx.FilterSet.from_bitmaps(e, masks, n_rows=n, first_row=first)
    got = e.exact_search_set(hx.OP_L2, 10, fs, fo)
    want = e.exact_search_filtered(hx.OP_L2, 10, masks, fo, first_row=first, n_rows=n)
    assert all((a.view(np.uint8) == b.view(np.uint8)).all() for a, b in zip(got, want))
    got = e.exact_range_set(hx.OP_L2, 2.0, fs, fo, ordered=True)
    want = e.exact_range_filtered(hx.OP_L2, 2.0, masks, fo, first_row=first, n_rows=n, ordered=True)
    assert int(got[0][-1]) > 0 and all(a.shape == b.shape and (a.view(np.uint8) == b.view(np.uint8)).all() for a, b in zip(got, want))
    fs.close()
    e.close()


@pytest.fixture(scope="module")
def wide():
    """a default engine of vector(200): it keeps the 8-bit sidecar"""
    rng = np.random.default_rng(21)
    n = 3000
    rows, qs = make(hx.F32, n, 200, rng), make(hx.F32, 12, 200, rng)
    qs[:6] = rows[:6] + 0.01 * qs[:6]                             # near some rows: a threshold the bound can skip against
    e = engine(hx.F32, 200, hx.OP_L2, rows, qs)
    lb = tenant_labels(n, rng)
    fs = hx.FilterSet.from_labels(e, lb, 6)
    yield e, fs, masks_of(lb, 6), lb
    fs.close()
    e.close()


@pytest.mark.gpu
def test_single_filter_takes_the_sidecar_path(wide, monkeypatch):
    """One distinct filter with HX_EXACT_SIDECAR=1: both calls take hx_exact_search's sidecar path.  The code rows read are a function of the plan
    (passing rows x query tiles) and must be equal; the f32 rows fetched depend on how fast the workgroups' shared threshold tightens, which is a
    race and differs from run to run of one and the same call, so they are only required to have moved."""
    e, fs, masks, lb = wide
    monkeypatch.setenv("HX_EXACT_SIDECAR", "1")
    fo = np.zeros(3, np.int32)
    e.exact_sidecar_stats(reset=True)
    want = e.exact_search_filtered(hx.OP_L2, 10, masks, fo, nq=3)
    coded_t, fetched_t = e.exact_sidecar_stats(reset=True)
    got = e.exact_search_set(hx.OP_L2, 10, fs, fo, nq=3)
    coded_s, fetched_s = e.exact_sidecar_stats(reset=True)
    assert all((a.view(np.uint8) == b.view(np.uint8)).all() for a, b in zip(got, want))
    assert coded_t == coded_s > 0 and fetched_t > 0 and fetched_s > 0
    r = float(want[1][0, 5])
    want = e.exact_range_filtered(hx.OP_L2, r, masks, fo, nq=3, cmp=hx.CMP_LE)
    coded_t, fetched_t = e.exact_sidecar_stats(reset=True)
    got = e.exact_range_set(hx.OP_L2, r, fs, fo, nq=3, cmp=hx.CMP_LE)
    coded_s, fetched_s = e.exact_sidecar_stats(reset=True)
    assert int(got[0][-1]) >= 6 and all(a.shape == b.shape and (a.view(np.uint8) == b.view(np.uint8)).all() for a, b in zip(got, want))
    assert coded_t == coded_s > 0 and fetched_t == fetched_s > 0   # a range scan's bound does not move: the fetches are determined


# ---- 5. range equality ----------------------------------------------------------------------------------------------------------------------
def range_raw(e, fs, masks, fo, radii, cmp, order, cap, want_ids=True, want_dist=True):
    """both calls through the C ABI -> (rc, offsets, ids, dist, total) each; ids / dist None: not asked for"""
    L, nq = hx.lib(), len(fo)
    n_rows, first = fs.info()["n_rows"], fs.info()["first_row"]
    words = [np.packbits(np.concatenate([m, np.zeros(-len(m) % 64, bool)]), bitorder="little").view(np.uint64) for m in masks]
    ptrs = (ctypes.c_void_p * len(words))(*[w.ctypes.data for w in words])
    r, of = np.ascontiguousarray(radii, np.float64), np.ascontiguousarray(fo, np.int32)
    out = []
    for twin in (True, False):
        off, total = np.full(nq + 1, 7, np.uint64), ctypes.c_uint64(7)
        ids = np.full(max(cap, 1), 7, np.uint32) if want_ids else None
        dist = np.full(max(cap, 1), 7.0) if want_dist else None
        if twin:
            rc = L.hx_exact_range_filtered(e.h, hx.OP_L2, cmp, P(r), 0, nq, first, n_rows, len(words), ptrs, P(of), order, cap, P(off), P(ids), P(dist),
                                           ctypes.byref(total))
        else:
            rc = L.hx_exact_range_set(e.h, hx.OP_L2, cmp, P(r), 0, nq, fs.h, P(of), order, cap, P(off), P(ids), P(dist), ctypes.byref(total))
        out.append((rc, off, ids, dist, total.value))
    return out


def same_range(a, b, written=True):
    assert a[0] == b[0] and (a[1] == b[1]).all() and a[4] == b[4]
    if written:
        t = int(a[4])
        for x, y in ((a[2], b[2]), (a[3], b[3])):
            assert (x is None) == (y is None) and (x is None or (x[:t].view(np.uint8) == y[:t].view(np.uint8)).all())


@pytest.mark.gpu
def test_range_equals_the_filtered_call():
    rng = np.random.default_rng(41)
    n, dim = 1500, 40
    fo = interleaved([5, 3, 17, 2, 2, 1], 3, rng)
    rows, qs = make(hx.F32, n, dim, rng), make(hx.F32, len(fo), dim, rng)
    rows[n // 2:n // 2 + 300] = rows[:300]
    lb = tenant_labels(n, rng)
    e = engine(hx.F32, dim, hx.OP_L2, rows, qs)
    fs = hx.FilterSet.from_labels(e, lb, 6)
    masks = masks_of(lb, 6)
    radii, _, _ = radii_of(e, hx.OP_L2, masks, fo)
    cap = n * len(fo)
    for cmp in (hx.CMP_LT, hx.CMP_LE, hx.CMP_GT, hx.CMP_GE):
        for order in (hx.RANGE_BY_ROW, hx.RANGE_BY_DISTANCE):
            t, s = range_raw(e, fs, masks, fo, radii, cmp, order, cap)
            assert t[0] == 0 and (cmp == hx.CMP_LT or t[4] > 0)
            same_range(t, s)
    t, s = range_raw(e, fs, masks, fo, radii, hx.CMP_LE, hx.RANGE_BY_ROW, 0, want_ids=False, want_dist=False)   # count only
    assert t[0] == 0 and t[4] > 0
    same_range(t, s)
    total = int(t[4])
    t, s = range_raw(e, fs, masks, fo, radii, hx.CMP_LE, hx.RANGE_BY_DISTANCE, cap, want_dist=False)            # ids without values
    assert t[0] == 0 and t[4] == total
    same_range(t, s)
    nan = np.where(np.arange(len(fo)) % 2 == 0, np.nan, radii)                                                  # `< NaN`: every row
    t, s = range_raw(e, fs, masks, fo, nan, hx.CMP_LT, hx.RANGE_BY_ROW, cap)
    assert t[0] == 0 and t[4] > total
    same_range(t, s)
    t, s = range_raw(e, fs, masks, fo, radii, hx.CMP_LE, hx.RANGE_BY_ROW, total - 1)                            # one short: the true counts
    assert t[0] == s[0] == E_NOMEM and t[4] == s[4] == total
    same_range(t, s, written=False)
    for f in (None, np.full(len(fo), 1), np.full(len(fo), 4)):                                                   # one distinct filter, or none
        got = e.exact_range_set(hx.OP_L2, radii, fs, f, cmp=hx.CMP_LE, ordered=True)
        want = e.exact_range_filtered(hx.OP_L2, radii, masks, f, cmp=hx.CMP_LE, ordered=True)
        assert all(a.shape == b.shape and (a.view(np.uint8) == b.view(np.uint8)).all() for a, b in zip(got, want))
    fs.close()
    e.close()


@pytest.mark.gpu
def test_range_sidecar_code_rows(wide, monkeypatch):
    e, fs, masks, lb = wide
    monkeypatch.setenv("HX_EXACT_SIDECAR", "1")
    fo = np.array([0, 1, 0, 2, 1, 0, -1, 0, 3, 1, 4, 0], np.int32)
    radii, _, _ = radii_of(e, hx.OP_L2, masks, fo)
    for cmp in (hx.CMP_LT, hx.CMP_LE):
        e.exact_sidecar_stats(reset=True)
        want = e.exact_range_filtered(hx.OP_L2, radii, masks, fo, cmp=cmp)
        coded_t, fetched_t = e.exact_sidecar_stats(reset=True)
        got = e.exact_range_set(hx.OP_L2, radii, fs, fo, cmp=cmp)
        coded_s, fetched_s = e.exact_sidecar_stats(reset=True)
        assert all(a.shape == b.shape and (a.view(np.uint8) == b.view(np.uint8)).all() for a, b in zip(got, want))
        assert coded_t == coded_s > 0 and fetched_t == fetched_s


# ---- 6. accounting and lifetime -------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_accounting():
    rng = np.random.default_rng(51)
    n = 2000
    rows, qs = make(hx.F32, n + 100, 8, rng), make(hx.F32, 6, 8, rng)
    e = engine(hx.F32, 8, hx.OP_L2, rows, qs)
    e.set_timing(True)
    lb = rng.integers(0, 2, n + 100).astype(np.uint32)
    before = e.kernel_stats(11)
    fs = hx.FilterSet.from_labels(e, lb[:n], 2)
    made = e.kernel_stats(11)
    assert made["launches"] > before["launches"] and made["units"] == before["units"] + n and made["ms"] > before["ms"]
    fs.append_labels(lb[n:])
    grown = e.kernel_stats(11)
    assert grown["launches"] > made["launches"] and grown["units"] == made["units"] + 100
    masks, fo = masks_of(lb, 2), np.array([0, 1, 0, 1, 1, 0])
    for kind, twin, mine in ((7, lambda: e.exact_search_filtered(hx.OP_L2, 5, masks, fo), lambda: e.exact_search_set(hx.OP_L2, 5, fs, fo)),
                             (8, lambda: e.exact_range_filtered(hx.OP_L2, 3.0, masks, fo), lambda: e.exact_range_set(hx.OP_L2, 3.0, fs, fo))):
        e.kernel_stats(kind, reset=True)
        want = twin()
        t = e.kernel_stats(kind, reset=True)
        got = mine()
        s = e.kernel_stats(kind, reset=True)
        assert all(a.shape == b.shape and (a.view(np.uint8) == b.view(np.uint8)).all() for a, b in zip(got, want))
        assert s["launches"] == t["launches"] - 1 and s["units"] == t["units"] == int((lb == 0).sum() + (lb == 1).sum()) * 3 and s["ms"] > 0
    assert e.kernel_stats(11) == grown                           # the scans do not move kind 11
    fs.close()
    e.close()


@pytest.mark.gpu
def test_two_sets_on_one_engine():
    rng = np.random.default_rng(61)
    n = 1000
    rows, qs = make(hx.F32, n, 4, rng), make(hx.F32, 5, 4, rng)
    e = engine(hx.F32, 4, hx.OP_L2, rows, qs)
    la, lb = draw_labels(n, 3, rng), draw_labels(n, 70, rng)
    a, b = hx.FilterSet.from_labels(e, la, 3), hx.FilterSet.from_labels(e, lb, 70)
    foa, fob = np.array([0, 2, 0, -1, 2]), np.array([5, 69, 5, 0, 12])
    wa = e.exact_search_filtered(hx.OP_L2, 7, masks_of(la, 3), foa)
    wb = e.exact_search_filtered(hx.OP_L2, 7, [lb == f for f in (0, 5, 12, 69)], np.array([1, 3, 1, 0, 2]))   # the same filters, numbered 0 .. 3
    for _ in range(2):
        assert all((x.view(np.uint8) == y.view(np.uint8)).all() for x, y in zip(e.exact_search_set(hx.OP_L2, 7, a, foa), wa))
        assert all((x.view(np.uint8) == y.view(np.uint8)).all() for x, y in zip(e.exact_search_set(hx.OP_L2, 7, b, fob), wb))
    a.close()
    assert all((x.view(np.uint8) == y.view(np.uint8)).all() for x, y in zip(e.exact_search_set(hx.OP_L2, 7, b, fob), wb))
    check_set(b, lists_of(lb, 70, 0), 0, n)
    b.close()
    e.close()
