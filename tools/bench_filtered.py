#!/usr/bin/env python3
"""bench_filtered.py -- per-query filters and distance predicates in iterative index scans (hx_index_search_filtered) against the only
ways hx_index_search_iterative can serve the same queries.  One JSON line per measurement, wall time = median of --reps calls.

    python tools/bench_filtered.py [--rows 1000000 --dim 768 --queries 1000]

On a library without hx_index_search_filtered (the parent commit) only the hx_index_search_iterative lines are printed, so the same script
gives both sides of the comparison on one lease.  Wall times include what the host does per call (mask table, query upload); `kernel_ms`
is the traversal kernel alone (hx_kernel_stats kind 2), so the difference is the host's share."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import pgvector_rx_amd as hx  # noqa: E402
from bench import synth  # noqa: E402


def timed(reps, eng, ix, fn):
    fn()                                                    # first call: allocates the per-query tables
    wall, kern, dist = [], [], []
    for _ in range(reps):
        eng.kernel_stats(2, reset=True)
        c0 = int(ix.counters()[4])
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        wall.append(time.perf_counter() - t0)
        kern.append(eng.kernel_stats(2, reset=True)["ms"])
        dist.append(int(ix.counters()[4]) - c0)
    return out, statistics.median(wall), min(wall), max(wall), statistics.median(kern), statistics.median(dist)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--rows", type=int, default=1_000_000)
    p.add_argument("--dim", type=int, default=768)
    p.add_argument("--queries", type=int, default=1000)
    p.add_argument("--efs", type=int, default=40)
    p.add_argument("--limit", type=int, default=10)
    p.add_argument("--max-scan-tuples", type=int, default=20000)
    p.add_argument("--reps", type=int, default=5)
    p.add_argument("--single-queries", type=int, default=40, help="nq = 1 calls with host-built masks actually timed (scaled to --queries)")
    a = p.parse_args()
    dev = torch.device("cuda:0")
    n, nq, G = a.rows, a.queries, 8
    rows, centres = synth(n, a.dim, "gmm", 11, dev)
    qs, _ = synth(nq, a.dim, "gmm", 12, dev, centres)
    eng = hx.Engine(hx.F32, hx.L2SQ, a.dim, n)
    eng.append_device(rows.data_ptr(), n)
    ix = hx.Index(eng, 16, 200)
    eng.set_timing(True)
    t0 = time.perf_counter()
    ix.insert(0, hx.draw_levels(n, 16, seed=11), batch=32768)
    has_new = hasattr(hx.Index, "search_filtered")
    base = {"rows": n, "dim": a.dim, "queries": nq, "ef_search": a.efs, "limit": a.limit, "max_scan_tuples": a.max_scan_tuples, "mode": "strict_order",
            "build_sec": round(time.perf_counter() - t0, 1), "has_search_filtered": has_new}
    tid = np.arange(n)
    filters = [(tid % 10 == g).astype(np.uint8) for g in range(G)]            # 8 filters of 10 % selectivity
    filter_of = (np.arange(nq) * G // nq).astype(np.int32)                    # queries of one filter are contiguous: a group is one upload for the old entry point
    args = (a.efs, 2, a.max_scan_tuples, a.limit)

    def emit(name, r, extra=None):
        _, med, lo, hi, kern, dist = r
        o = dict(base, measurement=name, wall_ms=round(med * 1e3, 2), wall_ms_min=round(lo * 1e3, 2), wall_ms_max=round(hi * 1e3, 2), kernel_ms=round(kern, 2),
                 queries_per_s=round(nq / med, 1), scan_distances_per_query=round(dist / nq, 1))
        o.update(extra or {})
        print(json.dumps(o), flush=True)

    def per_group():                                                          # the parent's way: one hx_index_search_iterative call per filter group
        out = []
        for g in range(G):
            sel = np.nonzero(filter_of == g)[0]
            eng.set_queries_device(qs[int(sel[0]):].data_ptr(), len(sel))
            out.append(ix.search_iterative(len(sel), *args, filters[g]))
        return out

    emit("8 filters of 10 %: 8 hx_index_search_iterative calls, one per filter group", timed(a.reps, eng, ix, per_group))
    eng.set_queries_device(qs.data_ptr(), nq)
    if has_new:
        emit("8 filters of 10 %: one hx_index_search_filtered call", timed(a.reps, eng, ix, lambda: ix.search_filtered(nq, *args, filters=filters, filter_of=filter_of)))

    # radius at each query's 5th-nearest value among the rows its filter passes (f32 distance of the engine -> float8 operator value)
    radius = np.empty(nq)
    rn = (rows * rows).sum(1)
    for g in range(G):
        sub = torch.nonzero(torch.from_numpy(filters[g]).to(dev)).squeeze(1)
        sel = torch.from_numpy(np.nonzero(filter_of == g)[0]).to(dev)
        near = sub[torch.topk(rn[sub][None, :] - 2.0 * qs[sel] @ rows[sub].T, 5, dim=1, largest=False).indices[:, 4]].cpu().numpy()
        for q, r in zip(sel.cpu().numpy(), near):
            radius[q] = np.sqrt(np.float64(eng.distances(qs[q].cpu().numpy(), np.array([r], np.uint32))[0]))

    all_rows = np.arange(n, dtype=np.uint32)
    ns = min(a.single_queries, nq)

    def singles():                                                            # the parent's way: nq = 1 calls, the mask built on the host from hx_distances against all rows
        out = []
        for q in list(range(0, nq, max(1, nq // ns)))[:ns]:
            d = eng.distances(qs[q].cpu().numpy(), all_rows)
            mask = filters[filter_of[q]] & (np.sqrt(d.astype(np.float64)) <= radius[q]).astype(np.uint8)
            eng.set_queries_device(qs[q:].data_ptr(), 1)
            out.append(ix.search_iterative(1, *args, mask))
        return out

    r = timed(max(1, a.reps // 2), eng, ix, singles)
    scale = nq / ns
    emit("filters + radius at the 5th nearest: nq = 1 hx_index_search_iterative calls with host-built masks (timed on %d queries, scaled to %d)" % (ns, nq),
         (r[0], r[1] * scale, r[2] * scale, r[3] * scale, r[4] * scale, r[5] * scale))
    eng.set_queries_device(qs.data_ptr(), nq)
    if has_new:
        kw = dict(filters=filters, filter_of=filter_of, cmp=hx.CMP_LE, radius=radius)
        emit("filters + radius at the 5th nearest: one hx_index_search_filtered call", timed(a.reps, eng, ix, lambda: ix.search_filtered(nq, *args, **kw)))
        plain = timed(a.reps, eng, ix, lambda: ix.search_filtered(nq, *args, cmp=hx.CMP_LE, radius=radius))
        flag = timed(a.reps, eng, ix, lambda: ix.search_filtered(nq, *args, cmp=hx.CMP_LE, radius=radius, stop_past_radius=True))
        same = all(np.array_equal(x, y) for x, y in zip(plain[0], flag[0]))
        emit("radius at the 5th nearest of the filtered rows, no filter, without HX_SCAN_STOP_PAST_RADIUS", plain, {"mean_returned": float(plain[0][3].mean())})
        emit("the same with HX_SCAN_STOP_PAST_RADIUS", flag, {"mean_returned": float(flag[0][3].mean()), "outputs_equal": bool(same)})
    emit("no filter, no predicate: hx_index_search_iterative", timed(a.reps, eng, ix, lambda: ix.search_iterative(nq, *args)))
    print(json.dumps(dict(base, fused=ix.fused_stats())), flush=True)


if __name__ == "__main__":
    main()
