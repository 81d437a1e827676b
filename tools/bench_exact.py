#!/usr/bin/env python3
"""bench_exact.py -- the exact k-NN scan (hx_exact_search) on the device: one JSON line per shape.

    python tools/bench_exact.py [--quick] [--n ROWS] [--reps R]

Shapes: N x vector(768) f32 <-> (default N = 1 000 000) for nq in {1, 4, 16, 64, 1024, 10000}, k in {10, 100, 1000}, filter none / 10 % / 1 %;
then one line each for halfvec(4000) <#>, vector(1536) <=> and bit(1024) <~> (nq 1, k 10).  --quick: nq {1, 16, 1024}, k {10, 100}, filter
none / 1 %.  Each line: kernel time (hx_kernel_stats kind 7, one warm-up call, median of R calls) and wall time; algorithmic bytes = passing
rows x row payload (each read once), GB/s and fraction of the 8 TB/s HBM peak; distance evaluations per second.  The nq = 1, k = 10, unfiltered
vector(768) line also times, for comparison, the oracle's brute force on one CPU core (sequential sums, over the first 100 000 rows, scaled to N)
and bench.py's torch ground_truth formula |r|^2 - 2 q.r on the same device rows -- different arithmetic from the operator's, labelled so.
Where the call took the 8-bit sidecar path, rows_fetched_frac = f32 rows read / code rows read, bytes_moved_model = code rows x
(al16(dim) + 16) + f32 rows x row bytes, and hbm_peak_frac is computed from that model (`bytes` stays the rows' payload); kernel_ms_min / _max
are the extremes of the R calls."""
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


def measure(e, op, k, nq, mask, reps):
    e.exact_search(op, k, nq=nq, row_pass=mask)                     # warm-up (scratch reservation, code objects)
    ks, ws = [], []
    e.exact_sidecar_stats(reset=True)
    for _ in range(reps):
        e.kernel_stats(7, reset=True)
        t = time.perf_counter()
        e.exact_search(op, k, nq=nq, row_pass=mask)
        ws.append((time.perf_counter() - t) * 1e3)
        ks.append(e.kernel_stats(7)["ms"])
    coded, fetched = e.exact_sidecar_stats(reset=True)
    return float(np.median(ks)), float(np.median(ws)), min(ks), max(ks), coded / reps, fetched / reps


def line(shape, e, dtype, dim, op, n, nq, k, filt, mask, reps, row_bytes):
    n_pass = int(mask.sum()) if mask is not None else n
    kms, wms, kmin, kmax, coded, fetched = measure(e, op, k, nq, mask, reps)
    nbytes = n_pass * row_bytes
    moved = coded * ((dim + 15) // 16 * 16 + 16) + fetched * row_bytes if coded else nbytes
    out = {"shape": shape, "rows": n, "dim": dim, "op": op, "nq": nq, "k": k, "filter": filt, "passing_rows": n_pass,
           "kernel_ms": round(kms, 4), "wall_ms": round(wms, 4), "bytes": nbytes, "gbps": round(nbytes / kms / 1e6, 1),
           "hbm_peak_frac": round(moved / kms / 1e-3 / HBM_PEAK, 3), "dist_per_s": float("%.4g" % (n_pass * nq / kms * 1e3)),
           "kernel_ms_min": round(kmin, 4), "kernel_ms_max": round(kmax, 4),
           "rows_fetched_frac": round(fetched / coded, 4) if coded else None, "bytes_moved_model": int(moved)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    import torch
    from oracle import orc
    n, dim = a.n, 768
    nqs, ks, filts = ([1, 16, 1024], [10, 100], ["none", "1%"]) if a.quick else ([1, 4, 16, 64, 1024, 10000], [10, 100, 1000], ["none", "10%", "1%"])
    rng = np.random.default_rng(0)
    masks = {"none": None, "10%": rng.random(n) < 0.10, "1%": rng.random(n) < 0.01}
    rows = device_rows(torch, n, dim, hx.F32, 1)
    e = hx.Engine(hx.F32, hx.L2SQ, dim, n)
    e.append_device(rows.data_ptr(), n)
    qs = rng.standard_normal((max(nqs), dim)).astype(np.float32)
    e.set_queries(qs)
    e.set_timing(True)
    for nq in nqs:
        for k in ks:
            for f in filts:
                out = line("vector(768) <->", e, hx.F32, dim, hx.OP_L2, n, nq, k, f, masks[f], a.reps, dim * 4)
                if nq == 1 and k == 10 and f == "none":
                    sub = min(n, 100_000)
                    host = rows[:sub].cpu().numpy()
                    t = time.perf_counter()
                    orc.distances_many(orc.F32, orc.L2SQ, dim, qs[0], host, order=orc.SEQ)
                    out["oracle_1core_ms_scaled"] = round((time.perf_counter() - t) * 1e3 * n / sub, 1)
                    qd = torch.from_numpy(qs[:1]).cuda()
                    rn = (rows * rows).sum(1)                  # bench.py ground_truth: |r|^2 - 2 q.r, then torch.topk (different arithmetic)
                    torch.cuda.synchronize()
                    tt = []
                    for _ in range(a.reps):
                        t = time.perf_counter()
                        torch.topk(rn[None, :] - 2.0 * (qd @ rows.T), k, dim=1, largest=False)
                        torch.cuda.synchronize()
                        tt.append((time.perf_counter() - t) * 1e3)
                    out["torch_ground_truth_ms_different_arithmetic"] = round(float(np.median(tt)), 3)
                print(json.dumps(out), flush=True)
    e.close()
    del rows
    torch.cuda.empty_cache()
    for shape, dtype, d2, op in (("halfvec(4000) <#>", hx.F16, 4000, hx.OP_NEG_IP), ("vector(1536) <=>", hx.F32, 1536, hx.OP_COSINE),
                                 ("bit(1024) <~>", hx.BIT, 1024, hx.OP_HAMMING)):
        r = device_rows(torch, n, d2, dtype, 2)
        e = hx.Engine(dtype, hx.HAMMING if dtype == hx.BIT else hx.L2SQ, d2, n)
        e.append_device(r.data_ptr(), n)
        e.set_queries(r[:1].cpu().numpy().view(np.uint16 if dtype == hx.F16 else np.float32 if dtype == hx.F32 else np.uint8))
        e.set_timing(True)
        print(json.dumps(line(shape, e, dtype, d2, op, n, 1, 10, "none", None, a.reps, int(e.row_bytes))), flush=True)
        e.close()
        del r
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
