"""The 8-bit row sidecar of f32 L2 engines: its bound never exceeds the canonical distance, it never changes a search or a
build, and every entry point that writes rows keeps it in step with them."""
import numpy as np
import pytest

import pgvector_rx_amd as hx

pytestmark = pytest.mark.gpu


def gmm(n, dim, rng, centres=32):
    c = rng.random((centres, dim)).astype(np.float32)
    return (c[rng.integers(0, centres, n)] + 0.1 * rng.standard_normal((n, dim))).astype(np.float32)


def adversarial(dim, rng):
    big = np.float32(np.finfo(np.float32).max / max(dim, 1) / 4)
    tiny = np.float32(1e-40)                                        # subnormal
    rows = [
        np.full(dim, 0.5, np.float32),                              # constant row: step 0, e_x 0
        np.zeros(dim, np.float32),
        (rng.standard_normal(dim) * big).astype(np.float32),        # near FLT_MAX / dim
        (rng.random(dim) * tiny).astype(np.float32),                # subnormals
        np.where(np.arange(dim) == dim // 2, np.float32(1e30), np.float32(0.25)).astype(np.float32),   # one huge coordinate
        rng.standard_normal(dim).astype(np.float32),
        (rng.random(dim) * 1e-20).astype(np.float32),
        np.full(dim, -3.0e38, np.float32),
    ]
    return np.stack(rows)


@pytest.mark.parametrize("dim", [129, 255, 256, 767, 768, 769, 1024, 2000])
def test_bound_below_canonical_distance(dim):
    rng = np.random.default_rng(dim)
    rows = np.concatenate([gmm(200, dim, rng), adversarial(dim, rng)])
    e = hx.Engine(hx.F32, hx.L2SQ, dim, len(rows))
    try:
        e.append(rows)
        ids = np.arange(len(rows), dtype=np.uint32)
        queries = np.concatenate([rows[:3], adversarial(dim, rng), (rows[3:6] + 1e-3).astype(np.float32)])
        e.set_queries(queries)
        for q in range(len(queries)):
            lb = e.sidecar_bounds(hx.QUERY_SLOT | q, ids)
            d = e.distances(queries[q], ids)
            assert np.all(np.isfinite(lb)) and np.all(lb >= 0)
            ok = (lb <= d) | np.isnan(d)
            assert ok.all(), (q, np.nonzero(~ok)[0][:5], lb[~ok][:5], d[~ok][:5])
            assert np.all(lb[np.isnan(d)] == 0)
        # the bound is useful on clustered data: most far rows are bounded above half their distance
        lb = e.sidecar_bounds(hx.QUERY_SLOT | 0, ids[:200])
        d = e.distances(queries[0], ids[:200])
        far = d > 1.0
        assert np.mean(lb[far] > 0.5 * d[far]) > 0.9
    finally:
        e.close()


def test_sidecar_meta_contract():
    rng = np.random.default_rng(5)
    dim = 300
    rows = np.concatenate([gmm(50, dim, rng), adversarial(dim, rng)])
    rows[-1, 7] = np.inf
    e = hx.Engine(hx.F32, hx.L2SQ, dim, len(rows))
    try:
        e.append(rows)
        codes, meta = e.sidecar_read(0, len(rows))
        lo, step, ex = meta[:, 0:1], meta[:, 1:2], meta[:, 2]
        xh = (lo.astype(np.float64) + step.astype(np.float64) * codes).astype(np.float32)    # exact product, one rounding: fmaf
        err = np.sqrt(((rows.astype(np.float64) - xh.astype(np.float64)) ** 2).sum(1))
        fin = np.isfinite(ex)
        assert np.all(ex[fin] >= err[fin])
        assert not np.isfinite(ex[-1])                              # a non-finite value: never rejected
        assert ex[len(rows) - 8] == 0.0                             # the constant row
    finally:
        e.close()


def sidecar_of(rows):
    e = hx.Engine(hx.F32, hx.L2SQ, rows.shape[1], len(rows))
    try:
        e.append(rows)
        return e.sidecar_read(0, len(rows))
    finally:
        e.close()


def test_sidecar_follows_row_writes():
    rng = np.random.default_rng(9)
    dim = 200
    a, b = gmm(100, dim, rng), gmm(40, dim, rng)
    e = hx.Engine(hx.F32, hx.L2SQ, dim, 200)
    try:
        e.append(a)
        e.append(b)
        e.pop(40)
        e.append(b[::-1].copy())                                    # popped slots rewritten
        e.normalize_rows(10, 30)
        now = e.read_rows(0, e.num_rows)
        c, m = e.sidecar_read(0, e.num_rows)
        c0, m0 = sidecar_of(now)
        assert np.array_equal(c, c0) and np.array_equal(m.view(np.uint32), m0.view(np.uint32))
    finally:
        e.close()


def test_no_sidecar_flag():
    e = hx.Engine(hx.F32, hx.L2SQ, 768, 16, sidecar=False)
    try:
        e.append(np.zeros((2, 768), np.float32))
        with pytest.raises(hx.HxError):
            e.sidecar_read(0, 1)
    finally:
        e.close()
    for dtype, metric, dim in ((hx.F32, hx.NEG_IP, 768), (hx.F32, hx.L2SQ, 64), (hx.F16, hx.L2SQ, 768)):
        e = hx.Engine(dtype, metric, dim, 16)
        try:
            with pytest.raises(hx.HxError):
                e.sidecar_read(0, 0)
        finally:
            e.close()


def build_and_search(rows, queries, sidecar, efs=40, batch=64):
    n, dim = rows.shape
    e = hx.Engine(hx.F32, hx.L2SQ, dim, n, sidecar=sidecar)
    try:
        e.append(rows)
        ix = hx.Index(e, 16, 64)
        levels = hx.draw_levels(n, 16, seed=3)
        ix.insert(0, levels, batch=batch)
        e.set_queries(queries)
        out = [ix.export_layer(0, 0, n)]
        out.append(ix.search(len(queries), efs, 10))
        filt = (np.arange(n) % 3 != 0).astype(np.uint8)
        out.append(ix.search_iterative(len(queries), efs, 1, 20000, 30, filter_pass=filt))
        out.append(ix.search_iterative(len(queries), efs, 2, 20000, 30))
        stats = e.sidecar_stats() if sidecar else None
        ix.close()
        return out, stats
    finally:
        e.close()


def flat(x):
    if isinstance(x, (tuple, list)):
        return [y for z in x for y in flat(z)]
    return [np.ascontiguousarray(x)]


def test_search_and_build_identical_with_and_without_sidecar():
    rng = np.random.default_rng(17)
    rows = gmm(6000, 768, rng)
    queries = (rows[rng.integers(0, 6000, 200)] + 0.05 * rng.standard_normal((200, 768))).astype(np.float32)
    on, (fetched, rejected) = build_and_search(rows, queries, True)
    off, _ = build_and_search(rows, queries, False)
    for a, b in zip(flat(on), flat(off)):
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()
    assert rejected > 0 and fetched > 0
