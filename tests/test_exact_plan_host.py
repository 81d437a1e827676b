"""The host plan of hx_exact_search_filtered's grouped path (pgvector-rx_amd/csrc/hx_exact_plan.h) on its own, over a few thousand random inputs:
groups of 1 .. 40 queries (0: the group is not there) with 1 .. 10^6 passing rows, k 1 .. 1024, row pitches on both sides of every tile-size rule,
small scratch budgets.
  - every (query, position of its filter's list) is streamed by exactly one scan workgroup, from the list of that query's group;
  - the candidate buffers and the counts of different (query, slice) never overlap and lie inside the block's scratch;
  - the slice count, buffer and count places the merge reads per query are the ones the scan workgroups write;
  - a block's scratch stays within the budget unless it is a single tile with a single slice;
  - a tile has no more slices than one per four rounds of its rows, and the call about 1024 workgroups.
Compiled for the host only, with the address and undefined-behaviour sanitizers; needs hipcc, no GPU."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")

SRC = r"""
#include "hx_exact_plan.h"
#include <cstdio>
#include <map>
#include <random>

static long bad = 0;
#define CHECK(c, ...) do { if (!(c)) { if (bad < 20) { printf("BAD %s: ", #c); printf(__VA_ARGS__); printf("\n"); } bad++; } } while (0)

int main()
{
    std::mt19937_64 g(20250611);
    auto rnd = [&](uint64_t lo, uint64_t hi) { return lo + g() % (hi - lo + 1); };
    const uint32_t pitches[] = {16, 64, 128, 144, 3072, 4096, 4112, 8016, 16384, 16400, 64000};
    long plans = 0, wgs = 0, multi_block = 0, partial = 0, over_budget = 0, cls_seen[3] = {0, 0, 0};
    for (int it = 0; it < 3000; it++) {
        const uint32_t k = it % 7 == 0 ? 1024 : it % 5 == 0 ? 1 : (uint32_t)rnd(1, 1024);
        const uint32_t pitch = pitches[rnd(0, 10)];
        const bool sparse = pitch == 8016;
        const uint64_t budget = it % 3 == 0 ? rnd(1, 4u << 20) : it % 3 == 1 ? rnd(1u << 20, 64u << 20) : 256ull << 20;
        std::vector<ExGroup> groups;
        const int ng = (int)rnd(1, 9);
        uint64_t ids = 0;
        for (int i = 0; i < ng; i++) {
            const uint32_t nq = (uint32_t)rnd(0, 40);
            const uint64_t pw = rnd(0, 3), n = pw == 0 ? rnd(1, 10) : pw == 1 ? rnd(1, 1000) : pw == 2 ? rnd(1, 100000) : rnd(1, 1000000);
            if (!nq) continue;
            const bool plain = i == 0 && (it & 1);
            groups.push_back(ExGroup{nq, n, plain ? EX_NO_IDS : ids});
            if (!plain) ids += n;
        }
        if (groups.empty()) continue;
        const ExGPlan p = ex_plan(groups, k, pitch, sparse, budget);
        plans++; wgs += (long)p.wg.size();

        uint32_t total_q = 0;
        std::vector<uint32_t> group_of;
        for (size_t gi = 0; gi < groups.size(); gi++) for (uint32_t j = 0; j < groups[gi].nq; j++) { group_of.push_back((uint32_t)gi); total_q++; }
        CHECK(p.mq.size() == total_q, "mq %zu queries %u", p.mq.size(), total_q);
        CHECK(p.wg.size() <= EX_PLAN_WGS + p.tiles.size(), "%zu workgroups for %zu tiles", p.wg.size(), p.tiles.size());

        uint32_t next_q = 0; size_t next_wg = 0;
        for (const ExBlock &b : p.blocks) {
            CHECK(b.q0 == next_q && b.nq > 0, "block at %u, expected %u", b.q0, next_q);
            next_q = b.q0 + b.nq;
            std::map<uint64_t, uint64_t> regions;                 // tile-slice buffers [buf, buf + cap * Q)
            std::vector<uint8_t> cnt_used(b.counts, 0);
            // per query: its workgroups as (beg -> index)
            std::vector<std::map<uint32_t, size_t>> by_q(b.nq);
            uint32_t tiles_in_block = 0, max_S = 0;
            for (int c = 0; c < 3; c++) {
                CHECK(b.wg0[c] == next_wg, "class %d starts at %u, expected %zu", c, b.wg0[c], next_wg);
                next_wg += b.nwg[c];
                if (b.nwg[c]) cls_seen[c]++;
                const uint32_t Q = EX_CLS_Q[c];
                CHECK(!b.nwg[c] || Q == 1 || (!sparse && (uint64_t)Q * pitch <= 64 * 1024), "tile of %u at pitch %u", Q, pitch);
                for (uint32_t w = b.wg0[c]; w < b.wg0[c] + b.nwg[c]; w++) {
                    const ExWg &d = p.wg[w];
                    CHECK(d.nlive >= 1 && d.nlive <= Q, "nlive %u of %u", d.nlive, Q);
                    if (d.nlive < Q) partial++;
                    CHECK(d.qpos >= b.q0 && d.qpos + d.nlive <= b.q0 + b.nq, "queries %u+%u outside block %u+%u", d.qpos, d.nlive, b.q0, b.nq);
                    CHECK(d.beg < d.end, "empty slice %u..%u", d.beg, d.end);
                    const uint64_t len = (uint64_t)p.cap[c] * Q;
                    CHECK(d.buf + len <= b.entries, "buffer %llu+%llu past %llu", (unsigned long long)d.buf, (unsigned long long)len, (unsigned long long)b.entries);
                    CHECK(!regions.count(d.buf), "two workgroups share the buffer at %llu", (unsigned long long)d.buf);
                    regions[d.buf] = d.buf + len;
                    if (d.beg == 0) { tiles_in_block++; max_S = std::max(max_S, d.S); }
                    const uint64_t n = groups[group_of[d.qpos]].n_pass, rounds4 = (n + 4 * p.R[c] - 1) / (4 * p.R[c]);
                    CHECK(d.S <= std::max<uint64_t>(1, rounds4), "S %u for %llu rows at %u per round", d.S, (unsigned long long)n, p.R[c]);
                    for (uint32_t i = 0; i < d.nlive; i++) {
                        const uint64_t ci = (uint64_t)d.cnt + (uint64_t)i * d.S;
                        CHECK(ci < b.counts && !cnt_used[ci], "count place %llu of %llu reused or outside", (unsigned long long)ci, (unsigned long long)b.counts);
                        if (ci < b.counts) cnt_used[ci] = 1;
                        CHECK(group_of[d.qpos + i] == group_of[d.qpos] && d.ids == groups[group_of[d.qpos]].ids, "a tile across groups, or another group's list");
                        CHECK(!by_q[d.qpos + i - b.q0].count(d.beg), "query %u slice at %u twice", d.qpos + i, d.beg);
                        by_q[d.qpos + i - b.q0][d.beg] = w;
                    }
                }
            }
            uint64_t prev_end = 0;
            for (auto &r : regions) { CHECK(r.first >= prev_end, "buffers overlap at %llu", (unsigned long long)r.first); prev_end = r.second; }
            for (uint32_t j = 0; j < b.nq; j++) {
                const uint32_t qp = b.q0 + j;
                const ExMq &m = p.mq[qp];
                const uint64_t n = groups[group_of[qp]].n_pass;
                uint64_t at = 0; uint32_t s = 0;
                CHECK(m.S == by_q[j].size(), "query %u: merge reads %u slices, scan wrote %zu", qp, m.S, by_q[j].size());
                for (auto &kv : by_q[j]) {                       // ascending beg == ascending slice
                    const ExWg &d = p.wg[kv.second];
                    const uint32_t i = qp - d.qpos;
                    CHECK(d.beg == at, "query %u: gap or overlap at %llu (slice starts at %u)", qp, (unsigned long long)at, d.beg);
                    at = d.end;
                    const int c = kv.second >= b.wg0[2] ? 2 : kv.second >= b.wg0[1] ? 1 : 0;
                    CHECK(m.Q == EX_CLS_Q[c] && m.cap == p.cap[c] && m.S == d.S, "query %u: merge (Q %u cap %u S %u) against scan (Q %u cap %u S %u)", qp, m.Q, m.cap, m.S,
                          EX_CLS_Q[c], p.cap[c], d.S);
                    CHECK(m.buf + (uint64_t)s * m.cap * m.Q == d.buf + i, "query %u slice %u: merge reads another buffer", qp, s);
                    CHECK((uint64_t)m.cnt + s == (uint64_t)d.cnt + (uint64_t)i * d.S, "query %u slice %u: merge reads another count", qp, s);
                    s++;
                }
                CHECK(at == n, "query %u: covered %llu of %llu rows", qp, (unsigned long long)at, (unsigned long long)n);
            }
            const uint64_t bytes = p.scratch(b, k);
            if (bytes > budget) over_budget++;
            CHECK(bytes <= budget || (tiles_in_block == 1 && max_S == 1), "block of %u tiles (S <= %u): %llu B over the budget %llu", tiles_in_block, max_S,
                  (unsigned long long)bytes, (unsigned long long)budget);
            CHECK(b.entries <= p.max_entries && b.counts <= p.max_counts && b.nq <= p.max_nq, "the maxima miss a block");
        }
        CHECK(next_q == total_q && next_wg == p.wg.size(), "blocks end at query %u of %u, workgroup %zu of %zu", next_q, total_q, next_wg, p.wg.size());
        if (p.blocks.size() > 1) multi_block++;
    }
    printf("plans %ld bad %ld workgroups %ld multi_block %ld partial %ld over_budget %ld q16 %ld q4 %ld q1 %ld\n", plans, bad, wgs, multi_block, partial, over_budget,
           cls_seen[0], cls_seen[1], cls_seen[2]);
    return bad ? 1 : 0;
}
"""


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
def test_every_row_of_every_query_is_scanned_once_and_the_merge_reads_what_the_scan_wrote(tmp_path):
    src = tmp_path / "plan.hip"
    src.write_text(SRC)
    exe = tmp_path / "plan"
    subprocess.run([HIPCC, "--offload-arch=gfx950", "--offload-host-only", "-O1", "-g", "-std=c++17", "-Xarch_host", "-fsanitize=address,undefined",
                    "-Xarch_host", "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, "pgvector-rx_amd", "csrc"), "-x", "hip", str(src), "-o", str(exe)],
                   check=True, capture_output=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    f = out.stdout.split("\n")[-2].split()
    res = dict(zip(f[0::2], map(int, f[1::2])))
    assert res["bad"] == 0
    assert res["plans"] > 2500 and res["workgroups"] > 100000
    assert res["multi_block"] > 100 and res["partial"] > 100 and res["over_budget"] > 0     # query blocks, partial tiles and the single-tile floor all occur
    assert res["q16"] > 100 and res["q4"] > 100 and res["q1"] > 100
