#!/usr/bin/env python3
"""bench_rerank.py -- the vector -> halfvec cast and the exact re-rank (hx_append_rows_halfvec, hx_exact_rerank): one JSON line per shape.

    python tools/bench_rerank.py [--n ROWS] [--reps R] [--legs cast,rerank,e2e] [--e2e-n ROWS] [--e2e-nq NQ]

cast    : N x vector(3072) -> halfvec(3072) rows, device to device (default N = 1 000 000).  Kernel time (hx_kernel_stats kind 10, median of R
          calls after one warm-up); bytes = 6 B per element (4 read, 2 written); fraction of the 8 TB/s HBM peak.
rerank  : N x vector(768) and vector(3072) rows; nq in {1, 100, 10 000} x candidates per query in {40, 100, 1 000}, ids drawn uniformly
          (random whole-row gathers), k = 10, <->.  Kernel time (kind 9); bytes = gathered row bytes (nq x candidates x row payload).
e2e     : the halfvec-expression-index plan on bench.py's 1 024-centre mixture (synth): E rows of vector(3072) in a scan-only engine (default
          E = N), the halfvec index (m 16, ef_construction 64) built on the device cast, ef_search 100, k' in {10, 40, 100} candidates, then
          hx_exact_rerank to k = 10 on the vector engine.  QPS (index scan + re-rank, wall) and recall@10 against hx_exact_search on the
          vector engine, next to the halfvec index's own first 10."""
import argparse
import importlib.util
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import pgvector_rx_amd as hx  # noqa: E402

HBM_PEAK = 8e12


def device_rows(torch, n, dim, seed):
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    return torch.randn((n, dim), generator=g, device="cuda", dtype=torch.float32)


def vector_engine(torch, n, dim, seed, rows=None):
    e = hx.Engine(hx.F32, hx.L2SQ, dim, n, scan_only=True)
    step = max(1, (1 << 30) // (dim * 4))                    # 1 GiB of rows at a time
    for i in range(0, n, step):
        b = min(step, n - i)
        x = device_rows(torch, b, dim, seed + i) if rows is None else rows[i:i + b]
        e.append_device(x.data_ptr(), b)
        del x
    torch.cuda.empty_cache()
    return e


def leg_cast(torch, n, reps):
    dim = 3072
    src = vector_engine(torch, n, dim, 1)
    dst = hx.Engine(hx.F16, hx.L2SQ, dim, n, scan_only=True)
    dst.set_timing(True)
    dst.append_halfvec_from(src)                              # warm-up
    ks, ws = [], []
    for _ in range(reps):
        dst.pop(n)
        dst.kernel_stats(10, reset=True)
        t = time.perf_counter()
        dst.append_halfvec_from(src)
        ws.append((time.perf_counter() - t) * 1e3)
        ks.append(dst.kernel_stats(10)["ms"])
    kms, nbytes = float(np.median(ks)), 6 * n * dim
    print(json.dumps({"leg": "cast", "shape": "vector(3072) -> halfvec(3072)", "rows": n, "elements": n * dim, "kernel_ms": round(kms, 4),
                      "wall_ms": round(float(np.median(ws)), 4), "bytes": nbytes, "gbps": round(nbytes / kms / 1e6, 1),
                      "hbm_peak_frac": round(nbytes / kms / 1e-3 / HBM_PEAK, 3)}), flush=True)
    src.close()
    dst.close()


def leg_rerank(torch, n, reps):
    rng = np.random.default_rng(0)
    for dim in (768, 3072):
        e = vector_engine(torch, n, dim, 2)
        e.set_queries(rng.standard_normal((10000, dim)).astype(np.float32))
        e.set_timing(True)
        for nq in (1, 100, 10000):
            for c in (40, 100, 1000):
                off = np.arange(nq + 1, dtype=np.uint64) * c
                ids = rng.integers(0, n, nq * c).astype(np.uint32)
                e.exact_rerank(hx.OP_L2, (off, ids), 10)      # warm-up (scratch reservation, code objects)
                ks, ws = [], []
                for _ in range(reps):
                    e.kernel_stats(9, reset=True)
                    t = time.perf_counter()
                    e.exact_rerank(hx.OP_L2, (off, ids), 10)
                    ws.append((time.perf_counter() - t) * 1e3)
                    ks.append(e.kernel_stats(9)["ms"])
                kms, nbytes = float(np.median(ks)), nq * c * dim * 4
                print(json.dumps({"leg": "rerank", "shape": "vector(%d) <->" % dim, "rows": n, "nq": nq, "candidates": c, "k": 10,
                                  "kernel_ms": round(kms, 4), "wall_ms": round(float(np.median(ws)), 4), "bytes": nbytes,
                                  "gbps": round(nbytes / kms / 1e6, 1), "hbm_peak_frac": round(nbytes / kms / 1e-3 / HBM_PEAK, 3),
                                  "dist_per_s": float("%.4g" % (nq * c / kms * 1e3))}), flush=True)
        e.close()


def leg_e2e(torch, n, nq, reps):
    spec = importlib.util.spec_from_file_location("bench_main", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    dim = 3072
    rows, centres = bench.synth(n, dim, "mixture", 1, "cuda")
    qs, _ = bench.synth(nq, dim, "mixture", 2, "cuda", centres)
    vec = vector_engine(torch, n, dim, 0, rows)
    del rows
    torch.cuda.empty_cache()
    vec.set_queries(qs.cpu().numpy())
    half = hx.Engine(hx.F16, hx.L2SQ, dim, n)
    t = time.perf_counter()
    half.append_halfvec_from(vec)
    ix = hx.Index(half, 16, 64)
    ix.insert(0, hx.draw_levels(n, 16, seed=5), batch=max(1, min(8192, n // 64)))
    build_s = time.perf_counter() - t
    half.set_queries_halfvec_from(vec)
    truth = vec.exact_search(hx.OP_L2, 10)[0]

    def recall(got):
        return float(np.mean([len(set(truth[q].tolist()) & set(got[q][:10].tolist())) / 10 for q in range(nq)]))
    for kp in (10, 40, 100):
        ix.search(nq, 100, kp)                                # warm-up
        ts, tr = [], []
        for _ in range(reps):
            t = time.perf_counter()
            tids, _, _, cnt = ix.search(nq, 100, kp)
            t1 = time.perf_counter()
            off = np.zeros(nq + 1, np.uint64)
            off[1:] = np.cumsum(cnt, dtype=np.uint64)
            cand = np.concatenate([tids[q, :cnt[q]] for q in range(nq)]).astype(np.uint32)
            ids, _, _ = vec.exact_rerank(hx.OP_L2, (off, cand), 10)
            ts.append(t1 - t)
            tr.append(time.perf_counter() - t1)
        s, r = float(np.median(ts)), float(np.median(tr))
        print(json.dumps({"leg": "e2e", "shape": "vector(3072) via halfvec(3072) hnsw", "rows": n, "nq": nq, "ef_search": 100, "k_prime": kp,
                          "k": 10, "build_s": round(build_s, 1), "index_qps": round(nq / s, 1), "qps": round(nq / (s + r), 1),
                          "recall_index_only": round(recall(tids), 4), "recall_reranked": round(recall(ids), 4)}), flush=True)
    ix.close()
    half.close()
    vec.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--legs", default="cast,rerank,e2e")
    ap.add_argument("--e2e-n", type=int, default=None)
    ap.add_argument("--e2e-nq", type=int, default=100)
    a = ap.parse_args()
    import torch
    legs = a.legs.split(",")
    if "cast" in legs:
        leg_cast(torch, a.n, a.reps)
    if "rerank" in legs:
        leg_rerank(torch, a.n, a.reps)
    if "e2e" in legs:
        leg_e2e(torch, a.e2e_n or a.n, a.e2e_nq, a.reps)


if __name__ == "__main__":
    main()
