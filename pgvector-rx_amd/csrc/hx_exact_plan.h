// hx_exact_plan.h -- the host plans of the exact top-k scans (hx_exact.hip).  ex_plan: hx_exact_search_filtered's grouped path, queries grouped
// by their filter, every group cut into query tiles, every tile into row slices, one work descriptor per scan workgroup and one per query for
// the merge.  ex_plan_plain: hx_exact_search's tile size, slices and query blocks.
// Plain C++ with no device code: tests/test_exact_plan_host.py and tests/test_exact_steady_plan.py compile it into stand-alone programs.
//
// Input: the groups in the order their queries stand in the grouped query order (ex_plan's positions 0 .. sum of nq - 1), each with its
//   number of queries (> 0), its number of passing rows (> 0) and where its row-id list starts (EX_NO_IDS: the plain row range).
// Tiles: a group of m queries is cut into tiles of 16 while m >= 16, then of 4 while m >= 2 (the last one may hold 2 or 3 live queries), then
//   of 1 -- within what the LDS rule of hx_exact_search allows (Q * pitch <= 64 KiB; sparsevec: 1).
// Slices: a tile gets a share of about EX_PLAN_WGS workgroups proportional to its passing rows, at least one, at most one per four rounds of
//   its rows (a round is R(Q) rows), and no more than fit the scratch budget beside its outputs.
// Blocks: tiles are taken in order into a block while the block's scratch stays within the budget (a block holds at least one tile): per tile
//   Q * S buffers of cap(Q) entries (12 B each) and as many counts (4 B), per live query k outputs (12 B) and a count.  The scratch of a plan
//   exceeds the budget only where a single tile with one slice does.
// Descriptors of a block: its workgroups by tile size (16, 4, 1), each size contiguous -- one scan launch per size present.
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

namespace {

constexpr uint64_t EX_NO_IDS = ~0ull;
constexpr uint32_t EX_PLAN_WGS = 1024;

struct ExWg {                 // one scan workgroup
    uint64_t ids;             // start of its group's row-id list in the id buffer (entries), or EX_NO_IDS: rows row0 + [beg, end)
    uint64_t buf;             // its candidate buffers in the block's scratch (entries): entry pos of query i at [buf + pos * Q + i]
    uint32_t beg, end;        // the list positions it streams
    uint32_t qpos, nlive;     // its queries: grouped positions qpos .. qpos + nlive - 1 (nlive <= Q)
    uint32_t cnt, S;          // the count of query i goes to [cnt + i * S]
};
struct ExMq {                 // one query of the merge, by grouped position
    uint64_t buf;             // entry pos of its slice s at [buf + (s * cap + pos) * Q] (its place in the tile is folded into buf)
    uint32_t S, Q, cap, cnt;  // the count of slice s at [cnt + s]
};
struct ExGroup { uint32_t nq; uint64_t n_pass, ids; };
struct ExTile { uint32_t group, qpos, nlive, cls, S, per; };   // cls: 0 / 1 / 2 = tiles of 16 / 4 / 1
struct ExBlock {
    uint32_t q0, nq;          // grouped positions [q0, q0 + nq)
    uint32_t wg0[3], nwg[3];  // its workgroups in ExGPlan::wg, by tile size
    uint64_t entries, counts; // scratch: candidate entries and counts
};
struct ExGPlan {
    uint32_t cap[3], R[3], cap2;
    std::vector<ExTile> tiles;
    std::vector<ExBlock> blocks;
    std::vector<ExWg> wg;
    std::vector<ExMq> mq;
    uint64_t max_entries = 0, max_counts = 0; uint32_t max_nq = 0;
    uint64_t scratch(const ExBlock &b, uint32_t k) const { return b.entries * 12 + b.counts * 4 + (uint64_t)b.nq * ((uint64_t)k * 12 + 4); }
};

constexpr uint32_t EX_CLS_Q[3] = {16, 4, 1};

// rows per round of a scan workgroup (waves * row slots in flight * rows per slot), as hx_exact_search plans them
inline uint32_t ex_plan_rows_per_round(uint32_t Q, uint32_t pitch, bool sparse)
{
    if (sparse) return 4 * 64;
    return 4 * (Q == 16 ? 2 : 4) * (pitch > 128 ? 1 : 8);
}

// The plan of the plain call (hx_exact_search; one filter or none for all nq queries, n_pass passing rows): query tile Q (LDS budget), rows
// per round R, per-(query, slice) buffer cap, slices S (~1024 workgroups, at least four rounds each), queries per block nqb (scratch budget).
struct ExPlan { uint32_t Q, R, cap, S, per, nqb, cap2; };

inline ExPlan ex_plan_plain(uint32_t nq, uint32_t pitch, bool sparse, uint64_t n_pass, uint32_t k, uint64_t budget)
{
    ExPlan p{};
    p.Q = sparse ? 1 : nq >= 16 && 16ull * pitch <= 64 * 1024 ? 16 : nq >= 4 && 4ull * pitch <= 64 * 1024 ? 4 : 1;
    p.R = ex_plan_rows_per_round(p.Q, pitch, sparse);
    p.cap = 64; while (p.cap < 2 * k || p.cap < k + p.R) p.cap <<= 1;
    p.cap2 = 4096; while (p.cap2 < 4 * k) p.cap2 <<= 1;
    const uint32_t tiles_all = (nq + p.Q - 1) / p.Q;
    p.S = std::max<uint64_t>(1, std::min<uint64_t>((1024 + tiles_all - 1) / tiles_all, (n_pass + 4 * p.R - 1) / (4 * p.R)));
    p.per = (uint32_t)((n_pass + p.S - 1) / p.S);
    p.S = (uint32_t)((n_pass + p.per - 1) / p.per);
    // top-k scratch per query: S buffers of cap entries + S counts + the merged output
    const uint64_t per_q = (uint64_t)p.S * p.cap * 12 + (uint64_t)p.S * 4 + (uint64_t)k * 12 + 4;
    p.nqb = (uint32_t)std::min<uint64_t>(nq, std::max<uint64_t>(p.Q, budget / per_q / p.Q * p.Q));
    return p;
}

inline ExGPlan ex_plan(const std::vector<ExGroup> &groups, uint32_t k, uint32_t pitch, bool sparse, uint64_t budget)
{
    ExGPlan p;
    for (int c = 0; c < 3; c++) {
        p.R[c] = ex_plan_rows_per_round(EX_CLS_Q[c], pitch, sparse);
        p.cap[c] = 64; while (p.cap[c] < 2 * k || p.cap[c] < k + p.R[c]) p.cap[c] <<= 1;
    }
    p.cap2 = 4096; while (p.cap2 < 4 * k) p.cap2 <<= 1;
    const uint32_t qmax = sparse ? 1 : 16ull * pitch <= 64 * 1024 ? 16 : 4ull * pitch <= 64 * 1024 ? 4 : 1;

    uint32_t qpos = 0; uint64_t weight = 0;
    for (uint32_t g = 0; g < groups.size(); g++) {
        uint32_t m = groups[g].nq;
        while (m > 0) {
            const uint32_t cls = qmax >= 16 && m >= 16 ? 0 : qmax >= 4 && m >= 2 ? 1 : 2;
            const uint32_t live = std::min(m, EX_CLS_Q[cls]);
            p.tiles.push_back(ExTile{g, qpos, live, cls, 0, 0});
            qpos += live; m -= live; weight += groups[g].n_pass;
        }
    }
    const uint64_t out_q = (uint64_t)k * 12 + 4;
    for (ExTile &t : p.tiles) {
        const uint64_t n = groups[t.group].n_pass, Q = EX_CLS_Q[t.cls];
        const uint64_t rounds4 = (n + 4 * p.R[t.cls] - 1) / (4 * p.R[t.cls]);
        uint64_t S = (uint64_t)((double)EX_PLAN_WGS * (double)n / (double)weight + 0.5);
        S = std::max<uint64_t>(1, std::min(S, rounds4));
        const uint64_t per_slice = Q * ((uint64_t)p.cap[t.cls] * 12 + 4), outs = t.nlive * out_q;
        S = std::max<uint64_t>(1, std::min(S, budget > outs ? (budget - outs) / per_slice : 0));
        t.per = (uint32_t)((n + S - 1) / S);
        t.S = (uint32_t)((n + t.per - 1) / t.per);
    }

    p.mq.resize(qpos);
    for (size_t t0 = 0; t0 < p.tiles.size();) {
        ExBlock b{};
        b.q0 = p.tiles[t0].qpos;
        size_t t1 = t0; uint64_t bytes = 0;
        while (t1 < p.tiles.size()) {
            const ExTile &t = p.tiles[t1];
            const uint64_t Q = EX_CLS_Q[t.cls], add = Q * t.S * ((uint64_t)p.cap[t.cls] * 12 + 4) + t.nlive * out_q;
            if (t1 > t0 && (bytes + add > budget || b.counts + Q * t.S > 0x7FFFFFFFull)) break;
            bytes += add; b.counts += Q * t.S; b.nq += t.nlive; t1++;
        }
        b.counts = 0;
        for (int c = 0; c < 3; c++) {
            b.wg0[c] = (uint32_t)p.wg.size();
            for (size_t ti = t0; ti < t1; ti++) {
                const ExTile &t = p.tiles[ti];
                if (t.cls != (uint32_t)c) continue;
                const ExGroup &g = groups[t.group];
                const uint32_t Q = EX_CLS_Q[c];
                for (uint32_t i = 0; i < t.nlive; i++)
                    p.mq[t.qpos + i] = ExMq{b.entries + i, t.S, Q, p.cap[c], (uint32_t)b.counts + i * t.S};
                for (uint32_t s = 0; s < t.S; s++) {
                    const uint64_t beg = (uint64_t)s * t.per, end = std::min<uint64_t>(beg + t.per, g.n_pass);
                    p.wg.push_back(ExWg{g.ids, b.entries + (uint64_t)s * p.cap[c] * Q, (uint32_t)beg, (uint32_t)end, t.qpos, t.nlive,
                                        (uint32_t)b.counts + s, t.S});
                }
                b.entries += (uint64_t)Q * t.S * p.cap[c]; b.counts += (uint64_t)Q * t.S;
            }
            b.nwg[c] = (uint32_t)p.wg.size() - b.wg0[c];
        }
        p.max_entries = std::max(p.max_entries, b.entries); p.max_counts = std::max(p.max_counts, b.counts); p.max_nq = std::max(p.max_nq, b.nq);
        p.blocks.push_back(b);
        t0 = t1;
    }
    return p;
}

} // namespace
