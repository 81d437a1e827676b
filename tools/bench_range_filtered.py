#!/usr/bin/env python3
"""bench_range_filtered.py -- exact range scans with a WHERE filter per query: hx_exact_range_filtered (one call) against the loop of
hx_exact_range calls, one per distinct filter, that a host has to make without it.  One JSON line per shape and engine.

    python tools/bench_range_filtered.py [--n ROWS] [--reps R] [--warmup W] [--out FILE]

Workload: N x vector(768) f32 (default N = 1 000 000, rows generated on the device), `v <-> q < r` by row, r = the value of the query's 100th
nearest passing row (so 99 hits per query, ties aside), on a default engine (8-bit sidecar) and on one created without it.  Shapes:
  a  64 queries, 64 disjoint tenant filters of 1/64 of the rows each
  b  64 queries over 8 disjoint tenants (1/8 of the rows each), 8 queries per tenant
  c  16 queries over 16 disjoint tenants of very unequal size: 1/2, 1/4, ... of the rows
  d  64 queries over 64 overlapping filters, each passing 10 % of the rows
Both sides run in this process on the same engine, take the filters as packed words (packing is not timed) and go through the same binding.
Per side: wall-clock per call (for the loop: per round of calls), uploads, launches, synchronisation and result copies included -- the median
of R calls after W warm-up calls, with min / quartiles / max as the run-to-run spread -- and the kernel time of hx_kernel_stats kind 8 (median).
The loop's queries of one filter are consecutive slots, so it needs one call per filter.  Before timing, the two sides' outputs are compared
byte for byte."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import pgvector_rx_amd as hx  # noqa: E402

K = 100                                                   # the radius is the value of the K-th nearest passing row


def pack(mask):
    bits = np.zeros((len(mask) + 63) // 64 * 64, np.uint8)
    bits[:len(mask)] = mask
    return np.ascontiguousarray(np.packbits(bits, bitorder="little").view(np.uint64))


def shapes(n, rng):
    tenant64 = rng.integers(0, 64, n)
    tenant8 = rng.integers(0, 8, n)
    p = np.array([2.0 ** -(i + 1) for i in range(15)] + [2.0 ** -15])
    tenant16 = rng.choice(16, n, p=p)
    yield "a: 64 queries, 64 disjoint tenants of 1/64", [tenant64 == f for f in range(64)], np.arange(64)
    yield "b: 64 queries, 8 disjoint tenants of 1/8, 8 queries each", [tenant8 == f for f in range(8)], np.repeat(np.arange(8), 8)
    yield "c: 16 queries, 16 disjoint tenants of 1/2, 1/4, ... of the rows", [tenant16 == f for f in range(16)], np.arange(16)
    yield "d: 64 queries, 64 overlapping filters of 10 %", [rng.random(n) < 0.10 for _ in range(64)], np.arange(64)


def grouped(e, words, fo, r):
    return e.exact_range_filtered(hx.OP_L2, r, words, fo, nq=len(fo), packed=True)


def loop(e, words, fo, r):
    out, at = [], 0
    for f in range(len(words)):                           # the queries of filter f are the consecutive slots where fo == f
        q = np.nonzero(fo == f)[0]
        out.append(e.exact_range(hx.OP_L2, r[q], first_query=int(q[0]), nq=len(q), row_pass=words[f], packed=True))
    off = np.zeros(len(fo) + 1, np.uint64)
    for o in out:                                         # the calls' CSR parts one after the other
        off[at + 1:at + len(o[0])] = off[at] + o[0][1:]
        at += len(o[0]) - 1
    return off, np.concatenate([o[1] for o in out]), np.concatenate([o[2] for o in out])


def measure(e, fn, words, fo, r, reps, warmup):
    for _ in range(warmup):
        fn(e, words, fo, r)
    wall, kern, launches = [], [], 0
    for _ in range(reps):
        e.kernel_stats(8, reset=True)
        t = time.perf_counter()
        fn(e, words, fo, r)
        wall.append((time.perf_counter() - t) * 1e3)
        st = e.kernel_stats(8)
        kern.append(st["ms"])
        launches = st["launches"]
    q = lambda a, p: round(float(np.percentile(a, p)), 4)
    return {"wall_ms": q(wall, 50), "wall_ms_min": q(wall, 0), "wall_ms_p25": q(wall, 25), "wall_ms_p75": q(wall, 75), "wall_ms_max": q(wall, 100),
            "kernel_ms": q(kern, 50), "kernel_ms_min": q(kern, 0), "kernel_ms_max": q(kern, 100), "launches": launches}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    a = ap.parse_args()
    import torch
    n, dim = a.n, 768
    g = torch.Generator(device="cuda")
    g.manual_seed(1)
    rows = torch.randn((n, dim), generator=g, device="cuda", dtype=torch.float32)
    queries = np.random.default_rng(0).standard_normal((64, dim)).astype(np.float32)
    for sidecar in (True, False):
        e = hx.Engine(hx.F32, hx.L2SQ, dim, n, sidecar=sidecar)
        e.append_device(rows.data_ptr(), n)
        e.set_queries(queries)
        e.set_timing(True)
        rng = np.random.default_rng(0)
        for name, masks, fo in shapes(n, rng):
            fo = fo.astype(np.int32)
            words = [pack(m) for m in masks]
            r = np.ascontiguousarray(e.exact_search_filtered(hx.OP_L2, K, words, fo, nq=len(fo), packed=True)[1][:, K - 1])
            got, want = grouped(e, words, fo, r), loop(e, words, fo, r)
            assert all(x.shape == y.shape and (x.view(np.uint8) == y.view(np.uint8)).all() for x, y in zip(got, want)), name
            e.exact_sidecar_stats(reset=True)
            one = measure(e, grouped, words, fo, r, a.reps, a.warmup)
            sc_one = e.exact_sidecar_stats(reset=True)
            many = measure(e, loop, words, fo, r, a.reps, a.warmup)
            sc_many = e.exact_sidecar_stats(reset=True)
            out = {"shape": name, "engine": "sidecar" if sidecar else "no sidecar", "rows": n, "dim": dim, "op": "<->", "cmp": "<", "order": "by row",
                   "nq": len(fo), "filters": len(words), "hits": int(got[0][-1]),
                   "passing_rows_per_query_sum": int(sum(int(masks[f].sum()) for f in fo)), "reps": a.reps, "warmup": a.warmup,
                   "grouped_call": one, "per_filter_loop": many,
                   "code_rows_per_call": {"grouped_call": sc_one[0] // (a.reps + a.warmup), "per_filter_loop": sc_many[0] // (a.reps + a.warmup)},
                   "wall_ratio_loop_over_grouped": round(many["wall_ms"] / one["wall_ms"], 2),
                   "kernel_ratio_loop_over_grouped": round(many["kernel_ms"] / one["kernel_ms"], 2),
                   "grouped_below_loop_min": {"wall": one["wall_ms"] < many["wall_ms_min"], "kernel": one["kernel_ms"] < many["kernel_ms_min"]}}
            s = json.dumps(out)
            print(s, flush=True)
            if a.out:
                with open(a.out, "a") as f:
                    f.write(s + "\n")
        e.close()


if __name__ == "__main__":
    main()
