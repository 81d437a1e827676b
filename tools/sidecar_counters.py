#!/usr/bin/env python3
"""sidecar_counters.py -- what the 8-bit row sidecar saves on bench.py's workload: the same 1M x vector(768) gmm rows, build and
ef_search 100 query batch, then per query the decided candidate distances, the f32 rows fetched (S) and the rows the bound skipped, from
hx_sidecar_stats; and the row bytes per query against the parent's (every decided row = one 3 072-byte f32 row).

    python tools/sidecar_counters.py [--rows 1000000] [--efs 100 40 200]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import pgvector_rx_amd as hx  # noqa: E402
from bench import synth  # noqa: E402


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--rows", type=int, default=1_000_000)
    p.add_argument("--dim", type=int, default=768)
    p.add_argument("--queries", type=int, default=10_000)
    p.add_argument("--efs", type=int, nargs="+", default=[100, 40, 200])
    a = p.parse_args()
    dev = torch.device("cuda:0")
    rows, centres = synth(a.rows, a.dim, "gmm", 11, dev)
    queries, _ = synth(a.queries, a.dim, "gmm", 12, dev, centres)
    torch.cuda.synchronize()
    eng = hx.Engine(hx.F32, hx.L2SQ, a.dim, a.rows)
    eng.append_device(rows.data_ptr(), a.rows)
    ix = hx.Index(eng, 16, 200)
    ix.insert(0, hx.draw_levels(a.rows, 16, seed=11), batch=32768)
    fb, rb = eng.sidecar_stats(reset=True)
    print(json.dumps({"phase": "build", "f32_rows_fetched": fb, "rows_skipped": rb, "skipped_frac": round(rb / max(1, fb + rb), 4)}))
    eng.set_queries_device(queries.data_ptr(), a.queries)
    row_b, code_b = a.dim * 4, (a.dim + 15) // 16 * 16 + 16
    for efs in a.efs:
        eng.sidecar_stats(reset=True)
        ix.search(a.queries, efs, 10)
        f, r = eng.sidecar_stats(reset=True)
        nq = a.queries
        decided = (f + r) / nq
        # every row decided after W's fill had its codes read; a row fetched while W fills did not: (decided - fill) codes, fill <= ef + entry rows
        print(json.dumps({"phase": "search", "ef_search": efs, "decided_per_query": round(decided, 1), "S_f32_rows_per_query": round(f / nq, 1),
                          "skipped_per_query": round(r / nq, 1), "skipped_frac_of_decided": round(r / max(1, f + r), 4),
                          "f32_bytes_per_query": round(f / nq * row_b), "parent_bytes_per_query": round(decided * row_b),
                          "upper_bound_bytes_per_query": round(f / nq * row_b + decided * code_b)}))
    ix.close()
    eng.close()


if __name__ == "__main__":
    main()
