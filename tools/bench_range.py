#!/usr/bin/env python3
"""bench_range.py -- the exact range scan (hx_exact_range) on the device: one JSON line per shape.

    python tools/bench_range.py [--quick] [--n ROWS] [--reps R]

Shapes: N x vector(768) f32 <-> (default N = 1 000 000) for nq in {1, 16, 256}, radii chosen per query for about 10, 1 000 and 100 000 hits
(the values of hx_exact_search's k-th neighbour, or a quantile of a sample), each by row, by distance and count-only; then halfvec(4000) <#>
and bit(1024) <~> for one line each (nq 1, ~1 000 hits, by row).  --quick: nq {1, 16}, ~10 and ~1 000 hits.  Each line: kernel time
(hx_kernel_stats kind 8, one warm-up call, median of R calls) and wall time; algorithmic bytes = rows x row payload (each row read once per
query tile) plus 12 B per hit written; GB/s and fraction of the 8 TB/s HBM peak; hits per second.  Where the call took the 8-bit sidecar path
(DESIGN.md 3a), rows_fetched_frac = f32 rows read / code rows read, bytes_moved_model = code rows x (al16(dim) + 16) + f32 rows x row bytes
(+ the hits), and hbm_peak_frac is computed from that model (`bytes` stays the rows' payload); kernel_ms_min / _max: extremes of the R calls."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import pgvector_rx_amd as hx  # noqa: E402

HBM_PEAK = 8e12


def device_rows(torch, n, dim, dtype, seed):
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    if dtype == hx.BIT:
        return torch.randint(0, 256, (n, (dim + 7) // 8), generator=g, device="cuda", dtype=torch.uint8)
    x = torch.randn((n, dim), generator=g, device="cuda", dtype=torch.float32)
    return x.half() if dtype == hx.F16 else x


def radii_for(e, op, nq, hits, n):
    """Per query the value of its `hits`-th nearest row (hx_exact_search when hits <= 1024, else a quantile of a 1024-row sample scan)."""
    if hits <= hx.EXACT_MAX_K:
        _, d, _ = e.exact_search(op, hits, nq=nq)
        return d[:, hits - 1].copy()
    step = n // 8192
    _, d, _ = e.exact_search(op, hx.EXACT_MAX_K, nq=nq)        # the sample's order statistic: rows 0, step, 2 step, ...
    off, _, dist = e.exact_range(op, np.inf, cmp=hx.CMP_LE, nq=nq, row_pass=(np.arange(n) % step == 0), ordered=True)
    return np.array([dist[int(off[q]) + min(int(off[q + 1] - off[q]) - 1, hits // step)] for q in range(nq)])


def measure(e, op, r, nq, mode, reps):
    kw = {"ordered": mode == "by_distance", "count_only": mode == "count_only"}
    out = e.exact_range(op, r, nq=nq, **kw)                     # warm-up (scratch reservation, code objects)
    cap = max(1, int(out[0][-1]))
    ks, ws = [], []
    e.exact_sidecar_stats(reset=True)
    for _ in range(reps):
        e.kernel_stats(8, reset=True)
        t = time.perf_counter()
        e.exact_range(op, r, nq=nq, cap=None if kw["count_only"] else cap, **kw)
        ws.append((time.perf_counter() - t) * 1e3)
        ks.append(e.kernel_stats(8)["ms"])
    coded, fetched = e.exact_sidecar_stats(reset=True)
    return float(np.median(ks)), float(np.median(ws)), int(out[0][-1]), min(ks), max(ks), coded / reps, fetched / reps


def line(shape, e, dim, op, n, nq, hits, mode, r, reps, row_bytes):
    kms, wms, total, kmin, kmax, coded, fetched = measure(e, op, r, nq, mode, reps)
    tiles = (nq + 15) // 16 if nq >= 16 and 16 * row_bytes <= 65536 else (nq + 3) // 4 if nq >= 4 and 4 * row_bytes <= 65536 else nq
    nbytes = n * row_bytes * tiles + (0 if mode == "count_only" else total * 12)
    hit_bytes = 0 if mode == "count_only" else total * 12
    moved = coded * ((dim + 15) // 16 * 16 + 16) + fetched * row_bytes + hit_bytes if coded else nbytes
    return {"shape": shape, "rows": n, "dim": dim, "op": op, "nq": nq, "target_hits_per_query": hits, "mode": mode, "hits": total,
            "kernel_ms": round(kms, 4), "wall_ms": round(wms, 4), "bytes": nbytes, "gbps": round(nbytes / kms / 1e6, 1),
            "hbm_peak_frac": round(moved / kms / 1e-3 / HBM_PEAK, 3), "hits_per_s": float("%.4g" % (total / kms * 1e3)),
            "dist_per_s": float("%.4g" % (n * nq / kms * 1e3)), "kernel_ms_min": round(kmin, 4), "kernel_ms_max": round(kmax, 4),
            "rows_fetched_frac": round(fetched / coded, 4) if coded else None, "bytes_moved_model": int(moved)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    import torch
    n, dim = a.n, 768
    nqs, hitss = ([1, 16], [10, 1000]) if a.quick else ([1, 16, 256], [10, 1000, 100_000])
    rows = device_rows(torch, n, dim, hx.F32, 1)
    e = hx.Engine(hx.F32, hx.L2SQ, dim, n)
    e.append_device(rows.data_ptr(), n)
    qs = np.random.default_rng(0).standard_normal((max(nqs), dim)).astype(np.float32)
    e.set_queries(qs)
    e.set_timing(True)
    for nq in nqs:
        for hits in hitss:
            r = radii_for(e, hx.OP_L2, nq, hits, n)
            for mode in ("by_row", "by_distance", "count_only"):
                print(json.dumps(line("vector(768) <->", e, dim, hx.OP_L2, n, nq, hits, mode, r, a.reps, dim * 4)), flush=True)
    e.close()
    del rows
    torch.cuda.empty_cache()
    for shape, dtype, d2, op in (("halfvec(4000) <#>", hx.F16, 4000, hx.OP_NEG_IP), ("bit(1024) <~>", hx.BIT, 1024, hx.OP_HAMMING)):
        r = device_rows(torch, n, d2, dtype, 2)
        e = hx.Engine(dtype, hx.HAMMING if dtype == hx.BIT else hx.L2SQ, d2, n)
        e.append_device(r.data_ptr(), n)
        e.set_queries(r[:1].cpu().numpy().view(np.uint16 if dtype == hx.F16 else np.uint8))
        e.set_timing(True)
        rad = radii_for(e, op, 1, 1000, n)
        print(json.dumps(line(shape, e, d2, op, n, 1, 1000, "by_row", rad, a.reps, int(e.row_bytes))), flush=True)
        e.close()
        del r
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
