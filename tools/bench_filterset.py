#!/usr/bin/env python3
"""bench_filterset.py -- filter sets: hx_exact_search_set / hx_exact_range_set (the filters resident on the device) against the
hx_exact_search_filtered / hx_exact_range_filtered calls they replace (the filters as host bitmaps, popcounted, uploaded and compacted per call).
One JSON line per shape and scan, then one per set build.

    python tools/bench_filterset.py [--n ROWS] [--reps R] [--warmup W] [--out FILE]

Workload: N x vector(768) f32 (default N = 1 000 000, rows generated on the device) on one default engine (8-bit sidecar), in one process.  The
four tenant shapes of tools/bench_exact_filtered.py and tools/bench_range_filtered.py:
  a  64 queries, 64 disjoint tenant filters of 1/64 of the rows each
  b  64 queries over 8 disjoint tenants (1/8 of the rows each), 8 queries per tenant
  c  16 queries over 16 disjoint tenants of very unequal size: 1/2, 1/4, ... of the rows
  d  64 queries over 64 overlapping filters, each passing 10 % of the rows
a, b and c are label columns (the set is made from the labels), d is bitmaps (the set is made from them).  top-k: `<->`, k = 10; range:
`v <-> q < r` by row, r = the value of the query's 100th nearest passing row.  Before anything is timed the two sides' outputs are compared
byte for byte.  Per side: wall-clock per call through the same binding (the twin takes packed words; packing is not timed) -- the median of R
calls after W warm-up calls with min and max -- and the kernel time of hx_kernel_stats kind 7 / 8 (median).
Set builds (hx_kernel_stats kind 11 for the kernel time): from a device label column and from a host one, for 64 and for 10 000 labels, and one
hx_filterset_append_labels of 10 000 rows; wall median of 5 builds after 1."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import pgvector_rx_amd as hx  # noqa: E402

K, KR = 10, 100


def pack(mask):
    bits = np.zeros((len(mask) + 63) // 64 * 64, np.uint8)
    bits[:len(mask)] = mask
    return np.ascontiguousarray(np.packbits(bits, bitorder="little").view(np.uint64))


def shapes(n, rng):
    tenant64 = rng.integers(0, 64, n).astype(np.uint32)
    tenant8 = rng.integers(0, 8, n).astype(np.uint32)
    p = np.array([2.0 ** -(i + 1) for i in range(15)] + [2.0 ** -15])
    tenant16 = rng.choice(16, n, p=p).astype(np.uint32)
    yield "a: 64 queries, 64 disjoint tenants of 1/64", tenant64, [tenant64 == f for f in range(64)], np.arange(64)
    yield "b: 64 queries, 8 disjoint tenants of 1/8, 8 queries each", tenant8, [tenant8 == f for f in range(8)], np.repeat(np.arange(8), 8)
    yield "c: 16 queries, 16 disjoint tenants of 1/2, 1/4, ... of the rows", tenant16, [tenant16 == f for f in range(16)], np.arange(16)
    yield "d: 64 queries, 64 overlapping filters of 10 %", None, [rng.random(n) < 0.10 for _ in range(64)], np.arange(64)


def spread(a):
    q = lambda p: round(float(np.percentile(a, p)), 4)   # noqa: E731
    return {"median": q(50), "min": q(0), "max": q(100)}


def measure(e, kind, fn, reps, warmup):
    for _ in range(warmup):
        fn()
    wall, kern, launches = [], [], 0
    for _ in range(reps):
        e.kernel_stats(kind, reset=True)
        t = time.perf_counter()
        fn()
        wall.append((time.perf_counter() - t) * 1e3)
        st = e.kernel_stats(kind)
        kern.append(st["ms"])
        launches = st["launches"]
    return {"wall_ms": spread(wall), "kernel_ms": spread(kern), "launches": launches}


def emit(out, path):
    s = json.dumps(out)
    print(s, flush=True)
    if path:
        with open(path, "a") as f:
            f.write(s + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    a = ap.parse_args()
    import torch
    n, dim, extra = a.n, 768, 10_000
    g = torch.Generator(device="cuda")
    g.manual_seed(1)
    rows = torch.randn((n, dim), generator=g, device="cuda", dtype=torch.float32)
    queries = np.random.default_rng(0).standard_normal((64, dim)).astype(np.float32)
    e = hx.Engine(hx.F32, hx.L2SQ, dim, n + extra)
    e.append_device(rows.data_ptr(), n)
    e.set_queries(queries)
    e.set_timing(True)
    rng = np.random.default_rng(0)
    same = lambda x, y: all(u.shape == v.shape and (u.view(np.uint8) == v.view(np.uint8)).all() for u, v in zip(x, y))   # noqa: E731
    for name, labels, masks, fo in shapes(n, rng):
        fo = fo.astype(np.int32)
        words = [pack(m) for m in masks]
        fs = hx.FilterSet.from_labels(e, labels, len(masks)) if labels is not None else hx.FilterSet.from_bitmaps(e, words, n_rows=n, packed=True)
        topk_twin = lambda: e.exact_search_filtered(hx.OP_L2, K, words, fo, nq=len(fo), n_rows=n, packed=True)   # noqa: E731
        topk_set = lambda: e.exact_search_set(hx.OP_L2, K, fs, fo, nq=len(fo))                                    # noqa: E731
        r = np.ascontiguousarray(e.exact_search_filtered(hx.OP_L2, KR, words, fo, nq=len(fo), n_rows=n, packed=True)[1][:, KR - 1])
        range_twin = lambda: e.exact_range_filtered(hx.OP_L2, r, words, fo, nq=len(fo), n_rows=n, packed=True)    # noqa: E731
        range_set = lambda: e.exact_range_set(hx.OP_L2, r, fs, fo, nq=len(fo))                                    # noqa: E731
        for scan, kind, twin, mine in (("top-k", 7, topk_twin, topk_set), ("range", 8, range_twin, range_set)):
            assert same(mine(), twin()), (name, scan)
            t = measure(e, kind, twin, a.reps, a.warmup)
            s = measure(e, kind, mine, a.reps, a.warmup)
            emit({"shape": name, "scan": scan, "rows": n, "dim": dim, "op": "<->", "nq": len(fo), "filters": len(words),
                  "set_from": "labels" if labels is not None else "bitmaps", "reps": a.reps, "warmup": a.warmup, "filtered_call": t, "set_call": s,
                  "wall_saved_ms": round(t["wall_ms"]["median"] - s["wall_ms"]["median"], 4),
                  "kernel_saved_ms": round(t["kernel_ms"]["median"] - s["kernel_ms"]["median"], 4),
                  "set_wall_median_below_filtered_min": s["wall_ms"]["median"] < t["wall_ms"]["min"],
                  "set_kernel_median_not_above_filtered": s["kernel_ms"]["median"] <= t["kernel_ms"]["median"]}, a.out)
        fs.close()

    # set builds: the label column in device memory and in host memory
    for L in (64, 10_000):
        lb = rng.integers(0, L, n + extra).astype(np.uint32)
        d_lb = torch.from_numpy(lb[:n].view(np.int32)).cuda()
        torch.cuda.synchronize()
        for src in ("device labels", "host labels"):
            wall, kern = [], []
            for i in range(6):
                e.kernel_stats(11, reset=True)
                t = time.perf_counter()
                fs = hx.FilterSet.from_labels(e, lb[:n], L) if src == "host labels" else hx.FilterSet.from_labels(e, None, L, device_ptr=d_lb.data_ptr(), n_rows=n)
                w = (time.perf_counter() - t) * 1e3
                st = e.kernel_stats(11)
                if i:
                    wall.append(w)
                    kern.append(st["ms"])
                fs.close()
            emit({"build": "create from " + src, "rows": n, "labels": L, "path": "histogram" if L <= 1024 else "sort", "wall_ms": spread(wall),
                  "kernel_ms": spread(kern), "launches": st["launches"]}, a.out)
        if L == 64:                                              # one append of 10 000 rows (each to a fresh set over the first n rows)
            e.append_device(rows.data_ptr(), extra)
            wall, kern = [], []
            for i in range(6):
                fs = hx.FilterSet.from_labels(e, lb[:n], L)
                e.kernel_stats(11, reset=True)
                t = time.perf_counter()
                fs.append_labels(lb[n:])
                w = (time.perf_counter() - t) * 1e3
                st = e.kernel_stats(11)
                if i:
                    wall.append(w)
                    kern.append(st["ms"])
                fs.close()
            emit({"build": "append_labels", "rows": n, "appended": extra, "labels": L, "wall_ms": spread(wall), "kernel_ms": spread(kern),
                  "launches": st["launches"]}, a.out)
    e.close()


if __name__ == "__main__":
    main()
