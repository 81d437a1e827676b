// hx_range_plan.h -- the host plan of hx_exact_range_filtered's grouped path (hx_range_g.hip): query blocks in the caller's order, inside a block
// the queries grouped by their filter, every group cut into query tiles, every tile into row slices, one work descriptor per scan workgroup.
// Plain C++ with no device code: tests/test_range_plan_host.py compiles it into a stand-alone program.
//
// Input: per query in the caller's order its group (-1: its filter passes no row, so it has no hits and is not scanned), and per group its
//   number of passing rows (> 0), where its row-id list starts (RG_NO_IDS: the plain row range) and whether its tiles of 4 and 1 take the sidecar
//   kernel.
// Blocks: consecutive ranges of the caller's query order -- the CSR base of a block is known only when the blocks before it are counted.  A block
//   takes all remaining queries, halved until its metadata (16 B of interval keys and 4 B of sort offset per query, 12 B of count and CSR base per
//   (query, segment)) fits a quarter of the budget; a block of one query holds one tile, whose slices are capped to fit.
// Tiles (ex_plan's rule): a group's m queries of the block are cut into tiles of 16 while m >= 16, then of 4 while m >= 2 (the last one may hold
//   2 or 3 live queries), then of 1 -- within what the LDS rule of hx_exact_range allows (Q * pitch <= 64 KiB; sparsevec: 1).
// Slices: a tile gets a share of about RG_PLAN_WGS workgroups proportional to its passing rows, at least one, at most one per four rounds of its
//   rows.  A slice is one workgroup of RG_WAVES waves; wave w streams list positions [beg + w * wper, beg + (w + 1) * wper) below `end`: one
//   segment per (query of the tile, wave).  The segments of block query j are numbered qseg[j] + slice * RG_WAVES + w: ascending in the list, so
//   in row order, and query after query in the caller's order -- the exclusive scan of the segments' counts is the block's CSR.
// Descriptors of a block: its workgroups by launch class (tiles of 16 / 4 / 1, then sidecar tiles of 4 / 1), each class contiguous -- one scan
//   launch per class present.
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

namespace {

constexpr uint64_t RG_NO_IDS = ~0ull;
constexpr uint32_t RG_PLAN_WGS = 1024, RG_WAVES = 4, RG_CLASSES = 5;
constexpr uint32_t RG_CLS_Q[RG_CLASSES] = {16, 4, 1, 4, 1};   // classes 3 and 4: the sidecar kernel

struct RgWg {                 // one scan workgroup (32 B)
    uint64_t ids;             // start of its group's row-id list in the id buffer (entries), or RG_NO_IDS: rows row0 + list position
    uint32_t beg, end, wper;  // its list positions [beg, end); wave w takes wper of them from beg + w * wper
    uint32_t qlist, nlive;    // its queries: entries qlist .. qlist + nlive - 1 of the block's grouped list (nlive <= Q)
    uint32_t seg;             // wave w writes segment qseg[j] + seg + w of its query at block position j
};
struct RgGroup { uint64_t n_pass, ids; bool sc; };
struct RgTile { uint32_t group, qlist, nlive, cls, S, wper; };
struct RgBlock {
    uint32_t q0, nq;                            // the caller's queries [q0, q0 + nq)
    uint32_t wg0[RG_CLASSES], nwg[RG_CLASSES];  // its workgroups in `wg`, by launch class
    uint64_t nseg; uint32_t max_wper;           // (query, segment) pairs; the longest segment
    std::vector<RgTile> tiles;
    std::vector<RgWg> wg;
    std::vector<uint32_t> qlist;                // block positions of the scanned queries, grouped by filter, a group's in the caller's order
    std::vector<uint32_t> qseg;                 // nq + 1: first segment of block position j; qseg[nq] = nseg
    uint64_t meta_bytes() const { return (uint64_t)nq * 20 + 4 + nseg * 12; }
    // staging entries per segment: within a quarter of the budget, ent bytes each (12 with keys, 4 without)
    uint32_t scap(uint64_t budget, uint64_t ent) const { return nseg ? (uint32_t)std::min<uint64_t>(max_wper, budget / 4 / ent / nseg) : 0; }
};

// rows per round of a scan workgroup, as hx_exact_range plans them
inline uint32_t rg_plan_rows_per_round(uint32_t Q, uint32_t pitch, bool sparse)
{
    if (sparse) return RG_WAVES * 64;
    return RG_WAVES * (Q == 16 ? 2 : 4) * (pitch > 128 ? 1 : 8);
}

// the block of the caller's queries [q0, q0 + nb)
inline RgBlock rg_plan_block(const int32_t *group_of, uint32_t q0, uint32_t nb, const std::vector<RgGroup> &groups, uint32_t pitch, bool sparse,
                             uint64_t budget)
{
    RgBlock b{};
    b.q0 = q0; b.nq = nb;
    const uint32_t qmax = sparse ? 1 : 16ull * pitch <= 64 * 1024 ? 16 : 4ull * pitch <= 64 * 1024 ? 4 : 1;
    std::vector<uint32_t> g_n(groups.size() + 1, 0);            // counting sort of the block positions by group
    for (uint32_t j = 0; j < nb; j++) if (group_of[q0 + j] >= 0) g_n[group_of[q0 + j] + 1]++;
    for (size_t g = 0; g < groups.size(); g++) g_n[g + 1] += g_n[g];
    b.qlist.resize(g_n[groups.size()]);
    {
        std::vector<uint32_t> at(g_n.begin(), g_n.end() - 1);
        for (uint32_t j = 0; j < nb; j++) if (group_of[q0 + j] >= 0) b.qlist[at[group_of[q0 + j]]++] = j;
    }
    uint64_t weight = 0;
    for (uint32_t g = 0; g < groups.size(); g++) {
        uint32_t m = g_n[g + 1] - g_n[g], at = g_n[g];
        while (m > 0) {
            uint32_t cls = qmax >= 16 && m >= 16 ? 0 : qmax >= 4 && m >= 2 ? 1 : 2;
            const uint32_t live = std::min(m, RG_CLS_Q[cls]);
            if (groups[g].sc && cls > 0) cls += 2;
            b.tiles.push_back(RgTile{g, at, live, cls, 0, 0});
            at += live; m -= live; weight += groups[g].n_pass;
        }
    }
    std::vector<uint32_t> G(nb, 0);                               // segments per block position
    for (RgTile &t : b.tiles) {
        const uint64_t n = groups[t.group].n_pass, Q = RG_CLS_Q[t.cls], R = rg_plan_rows_per_round((uint32_t)Q, pitch, sparse);
        uint64_t S = (uint64_t)((double)RG_PLAN_WGS * (double)n / (double)weight + 0.5);
        S = std::max<uint64_t>(1, std::min(S, (n + 4 * R - 1) / (4 * R)));
        const uint64_t room = budget / 4 / Q;                    // a tile alone in its block still fits the metadata quarter where one slice does
        S = std::max<uint64_t>(1, std::min<uint64_t>(S, room > 64 ? (room - 64) / (RG_WAVES * 12ull) : 0));
        t.wper = (uint32_t)((n + S * RG_WAVES - 1) / (S * RG_WAVES));
        t.S = (uint32_t)(((n + t.wper - 1) / t.wper + RG_WAVES - 1) / RG_WAVES);
        b.max_wper = std::max(b.max_wper, t.wper);
        for (uint32_t i = 0; i < t.nlive; i++) G[b.qlist[t.qlist + i]] = t.S * RG_WAVES;
    }
    b.qseg.resize(nb + 1);
    for (uint32_t j = 0; j < nb; j++) { b.qseg[j] = (uint32_t)b.nseg; b.nseg += G[j]; }
    b.qseg[nb] = (uint32_t)b.nseg;
    return b;
}

// the descriptors of a block whose tiles are final
inline void rg_plan_descriptors(RgBlock &b, const std::vector<RgGroup> &groups)
{
    for (uint32_t c = 0; c < RG_CLASSES; c++) {
        b.wg0[c] = (uint32_t)b.wg.size();
        for (const RgTile &t : b.tiles) {
            if (t.cls != c) continue;
            const RgGroup &g = groups[t.group];
            for (uint32_t s = 0; s < t.S; s++) {
                const uint64_t beg = (uint64_t)s * RG_WAVES * t.wper, end = std::min<uint64_t>(beg + (uint64_t)RG_WAVES * t.wper, g.n_pass);
                b.wg.push_back(RgWg{g.ids, (uint32_t)beg, (uint32_t)end, t.wper, t.qlist, t.nlive, s * RG_WAVES});
            }
        }
        b.nwg[c] = (uint32_t)b.wg.size() - b.wg0[c];
    }
}

// group_of: nq entries in [-1, groups.size())
inline std::vector<RgBlock> rg_plan(const std::vector<int32_t> &group_of, const std::vector<RgGroup> &groups, uint32_t pitch, bool sparse, uint64_t budget)
{
    std::vector<RgBlock> blocks;
    const uint32_t nq = (uint32_t)group_of.size();
    for (uint32_t q0 = 0; q0 < nq;) {
        uint32_t nb = nq - q0;
        RgBlock b = rg_plan_block(group_of.data(), q0, nb, groups, pitch, sparse, budget);
        while (nb > 1 && (b.meta_bytes() > budget / 4 || b.nseg > 0x7FFFFFFFull)) {
            nb = (nb + 1) / 2;
            b = rg_plan_block(group_of.data(), q0, nb, groups, pitch, sparse, budget);
        }
        rg_plan_descriptors(b, groups);
        q0 += nb;
        blocks.push_back(std::move(b));
    }
    return blocks;
}

} // namespace
