"""The host plan of hx_exact_range_filtered's grouped path (pgvector-rx_amd/csrc/hx_range_plan.h) on its own, over a few thousand random inputs:
1 .. 9 groups of 0 .. 40 queries (0: the group is not there) with 1 .. 10^6 passing rows, the caller's order interleaved (with queries whose filter
passes nothing in between), row pitches on both sides of every tile-size rule (8016 as sparsevec), budgets from 64 KiB up.
  - every (query, position of its filter's list) is streamed by exactly one wave, from the list of that query's group;
  - a query's segments are numbered in ascending list order, and every segment place of the block has exactly one writer;
  - the count, staging and base places of different (query, segment) never overlap and lie inside the block's areas;
  - blocks are consecutive ranges of the caller's order that cover all queries once;
  - a block's metadata and staging stay within their quarters of the budget unless it is a single tile with a single slice;
  - a tile has no more slices than one per four rounds of its rows, and a block about 1024 workgroups;
  - only tiles of 4 and 1 of a group marked for the sidecar are in the sidecar classes.
Compiled for the host only, with the address and undefined-behaviour sanitizers; needs hipcc, no GPU."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")

SRC = r"""
#include "hx_range_plan.h"
#include <cstdio>
#include <map>
#include <random>

static long bad = 0;
#define CHECK(c, ...) do { if (!(c)) { if (bad < 20) { printf("BAD %s: ", #c); printf(__VA_ARGS__); printf("\n"); } bad++; } } while (0)

int main()
{
    std::mt19937_64 g(20250712);
    auto rnd = [&](uint64_t lo, uint64_t hi) { return lo + g() % (hi - lo + 1); };
    const uint32_t pitches[] = {16, 64, 128, 144, 3072, 4096, 4112, 8016, 16384, 16400, 64000};
    long plans = 0, wgs = 0, multi_block = 0, partial = 0, over_budget = 0, dead = 0, cls_seen[RG_CLASSES] = {0, 0, 0, 0, 0};
    for (int it = 0; it < 3000; it++) {
        const uint32_t pitch = pitches[rnd(0, 10)];
        const bool sparse = pitch == 8016;
        const uint64_t budget = it % 3 == 0 ? rnd(64u << 10, 1u << 20) : it % 3 == 1 ? rnd(1u << 20, 64u << 20) : 256ull << 20;
        std::vector<RgGroup> groups;
        std::vector<int32_t> group_of;
        const int ng = (int)rnd(1, 9);
        uint64_t ids = 0;
        for (int i = 0; i < ng; i++) {
            const uint32_t nq = (uint32_t)rnd(0, 40);
            const uint64_t pw = rnd(0, 3), n = pw == 0 ? rnd(1, 10) : pw == 1 ? rnd(1, 1000) : pw == 2 ? rnd(1, 100000) : rnd(1, 1000000);
            if (!nq) continue;
            const bool plain = i == 0 && (it & 1);
            for (uint32_t j = 0; j < nq; j++) group_of.push_back((int32_t)groups.size());
            groups.push_back(RgGroup{n, plain ? RG_NO_IDS : ids, rnd(0, 2) == 0});
            if (!plain) ids += n;
        }
        if (groups.empty()) continue;
        for (uint64_t j = rnd(0, 5); j > 0; j--) { group_of.push_back(-1); dead++; }   // queries whose filter passes no row
        std::shuffle(group_of.begin(), group_of.end(), g);
        const uint32_t nq = (uint32_t)group_of.size();
        const std::vector<RgBlock> blocks = rg_plan(group_of, groups, pitch, sparse, budget);
        plans++;

        uint32_t next_q = 0;
        for (const RgBlock &b : blocks) {
            CHECK(b.q0 == next_q && b.nq > 0, "block at %u, expected %u", b.q0, next_q);
            next_q = b.q0 + b.nq;
            wgs += (long)b.wg.size();
            CHECK(b.qseg.size() == (size_t)b.nq + 1 && b.qseg[0] == 0 && b.qseg[b.nq] == b.nseg, "segment table");
            uint32_t scanned = 0;
            for (uint32_t j = 0; j < b.nq; j++) {
                CHECK(b.qseg[j] <= b.qseg[j + 1], "segments of query %u", j);
                CHECK((group_of[b.q0 + j] < 0) == (b.qseg[j] == b.qseg[j + 1]), "query %u: segments and group disagree", j);
                scanned += group_of[b.q0 + j] >= 0;
            }
            CHECK(b.qlist.size() == scanned, "grouped list %zu, scanned %u", b.qlist.size(), scanned);
            std::vector<uint8_t> listed(b.nq, 0);
            for (uint32_t j : b.qlist) { CHECK(j < b.nq && !listed[j], "grouped list entry %u", j); if (j < b.nq) listed[j] = 1; }
            std::vector<uint8_t> seg_used(b.nseg, 0);
            std::vector<std::map<uint32_t, std::pair<uint32_t, uint32_t>>> by_q(b.nq);     // segment -> list range
            std::map<uint32_t, uint32_t> slices;                                          // tile (its place in the grouped list) -> slices
            size_t next_wg = 0;
            for (uint32_t c = 0; c < RG_CLASSES; c++) {
                CHECK(b.wg0[c] == next_wg, "class %u starts at %u, expected %zu", c, b.wg0[c], next_wg);
                next_wg += b.nwg[c];
                if (b.nwg[c]) cls_seen[c]++;
                const uint32_t Q = RG_CLS_Q[c];
                CHECK(!b.nwg[c] || Q == 1 || (!sparse && (uint64_t)Q * pitch <= 64 * 1024), "tile of %u at pitch %u", Q, pitch);
                for (uint32_t w = b.wg0[c]; w < b.wg0[c] + b.nwg[c]; w++) {
                    const RgWg &d = b.wg[w];
                    CHECK(d.nlive >= 1 && d.nlive <= Q && (size_t)d.qlist + d.nlive <= b.qlist.size(), "nlive %u of %u at %u", d.nlive, Q, d.qlist);
                    if (d.nlive < Q) partial++;
                    CHECK(d.beg < d.end && d.wper > 0 && d.seg % RG_WAVES == 0, "slice %u..%u, %u per wave, segment %u", d.beg, d.end, d.wper, d.seg);
                    CHECK((uint64_t)d.beg + (uint64_t)RG_WAVES * d.wper >= d.end, "slice %u..%u longer than %u waves of %u", d.beg, d.end, RG_WAVES, d.wper);
                    slices[d.qlist]++;
                    const int32_t grp = group_of[b.q0 + b.qlist[d.qlist]];
                    CHECK(grp >= 0 && d.ids == groups[grp].ids && d.end <= groups[grp].n_pass, "another group's list, or past its end");
                    CHECK((c >= 3) == (groups[grp].sc && Q <= 4), "class %u for a group with sidecar flag %d", c, (int)groups[grp].sc);
                    const uint64_t n = groups[grp].n_pass, R = rg_plan_rows_per_round(Q, pitch, sparse);
                    CHECK(slices[d.qlist] <= std::max<uint64_t>(1, (n + 4 * R - 1) / (4 * R)), "slice %u of a tile of %llu rows at %llu per round", slices[d.qlist],
                          (unsigned long long)n, (unsigned long long)R);
                    for (uint32_t i = 0; i < d.nlive; i++) {
                        const uint32_t j = b.qlist[d.qlist + i];
                        CHECK(group_of[b.q0 + j] == grp, "a tile across groups");
                        for (uint32_t wv = 0; wv < RG_WAVES; wv++) {
                            const uint64_t seg = (uint64_t)b.qseg[j] + d.seg + wv;
                            CHECK(seg < b.qseg[j + 1] && !seg_used[seg], "query %u: segment %llu outside its range or written twice", j, (unsigned long long)seg);
                            if (seg >= b.nseg) continue;
                            seg_used[seg] = 1;
                            const uint32_t sb = (uint32_t)std::min<uint64_t>((uint64_t)d.beg + (uint64_t)wv * d.wper, d.end);
                            const uint32_t se = (uint32_t)std::min<uint64_t>((uint64_t)sb + d.wper, d.end);
                            CHECK(se - sb <= b.max_wper, "segment longer than max_wper");
                            by_q[j][(uint32_t)seg] = {sb, se};
                        }
                    }
                }
            }
            CHECK(next_wg == b.wg.size(), "classes end at %zu of %zu", next_wg, b.wg.size());
            CHECK(b.wg.size() <= RG_PLAN_WGS + b.tiles.size(), "%zu workgroups for %zu tiles", b.wg.size(), b.tiles.size());
            for (uint64_t s = 0; s < b.nseg; s++) CHECK(seg_used[s], "segment %llu has no writer", (unsigned long long)s);
            for (uint32_t j = 0; j < b.nq; j++) {
                if (group_of[b.q0 + j] < 0) continue;
                uint64_t at = 0;
                for (auto &kv : by_q[j]) {                       // ascending segment number == ascending list order
                    CHECK(kv.second.first == at || kv.second.first == kv.second.second, "query %u: segment %u starts at %u, expected %llu", j, kv.first,
                          kv.second.first, (unsigned long long)at);
                    at = std::max<uint64_t>(at, kv.second.second);
                }
                CHECK(at == groups[group_of[b.q0 + j]].n_pass, "query %u: covered %llu rows", j, (unsigned long long)at);
            }
            uint32_t max_S = 0;
            for (auto &kv : slices) max_S = std::max(max_S, kv.second);
            const bool floor = slices.size() == 1 && max_S == 1;
            for (uint64_t ent : {12, 4}) {
                const uint64_t scap = b.scap(budget, ent);
                CHECK(scap <= b.max_wper && b.nseg * scap * ent <= budget / 4, "staging of %llu segments x %llu entries", (unsigned long long)b.nseg, (unsigned long long)scap);
            }
            if (b.meta_bytes() > budget / 4) over_budget++;
            CHECK(b.meta_bytes() <= budget / 4 || floor, "metadata %llu B over a quarter of %llu", (unsigned long long)b.meta_bytes(), (unsigned long long)budget);
        }
        CHECK(next_q == nq, "blocks end at query %u of %u", next_q, nq);
        if (blocks.size() > 1) multi_block++;
    }
    printf("plans %ld bad %ld workgroups %ld multi_block %ld partial %ld over_budget %ld dead %ld q16 %ld q4 %ld q1 %ld sc4 %ld sc1 %ld\n", plans, bad, wgs, multi_block,
           partial, over_budget, dead, cls_seen[0], cls_seen[1], cls_seen[2], cls_seen[3], cls_seen[4]);
    return bad ? 1 : 0;
}
"""


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
def test_every_row_of_every_query_has_one_wave_and_every_segment_one_writer(tmp_path):
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
    assert res["multi_block"] > 100 and res["partial"] > 100 and res["dead"] > 1000     # query blocks, partial tiles and unscanned queries all occur
    assert min(res[c] for c in ("q16", "q4", "q1", "sc4", "sc1")) > 100
