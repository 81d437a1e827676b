// hx_range_g.hip -- exact distance-threshold scans with a filter per query (include/hnswrx.h: hx_exact_range_filtered): a batch of
// `WHERE tenant = $1 AND v <op> $2 < r` in one call.  The outputs are, byte for byte, the CSR concatenation of one hx_exact_range call per query.
//
// One distinct filter: the call is hx_exact_range (hx_range.hip).  Two or more: the grouped path below.
//   One launch compacts every referenced bitmap into a row-id list in row order (k_range_compact_g: per-word offsets from the host's popcount
//   pass, as k_range_compact).  The host plans query blocks, tiles, slices and segments (hx_range_plan.h).  Per block, pass 1 is one launch per
//   launch class present (query tiles of 16 / 4 / 1, and of 4 / 1 through the 8-bit sidecar): k_range_scan_g and k_range_scan_sc_g are
//   k_range_scan's and k_range_scan_sc's bodies with tile, slice, row list and segment places read from a work descriptor per workgroup
//   (hx_exact_core.h: ex_uni, ex_park_slots).  A (query, segment) pair has one writer; a query's segments follow each other in row order and the
//   queries stand in the caller's order, so the host's exclusive scan of the counts is the CSR.  Windows, the gather of the staged segments, the
//   re-scan of the overflowed ones, the segmented sort and the values are those of hx_exact_range (hx_range_core.h).
#include "hx_range_core.h"
#include "hx_range_plan.h"

#include <cstring>

namespace {

struct RgGArgs {
    const uint8_t *rows, *queries; uint32_t pitch, cap_sp;
    const uint32_t *ids; uint32_t row0, qslot0;               // ids: the id lists of all referenced filters; qslot0: slot of the block's first query
    const RgWg *wg;                                           // one per workgroup of this launch
    const uint32_t *slots, *qseg;                             // query slot by entry of the block's grouped list; first segment by block position
    const uint64_t *klo, *khi;                                // by block position: a hit iff klo <= key <= khi
    uint32_t *cnt;                                            // by segment: pass 1 writes them, a window pass reads them
    uint32_t scap;                                            // staging entries per segment (pass 1: segment s at s * scap)
    const uint64_t *seg_base; uint64_t w0, w1;                // window pass (seg_base != nullptr): CSR position of a segment's first hit, window
    uint64_t *okey; uint32_t *oid;                            // staging (pass 1) or window output; oid == nullptr: count only, okey may be
};

struct RgWgU { uint64_t ids; uint32_t beg, end, wper, qlist, nlive, seg; };
__device__ __forceinline__ RgWgU rg_desc(const RgWg *wg)     // a uniform address: into scalar registers
{
    const RgWg &w = wg[blockIdx.x];
    return RgWgU{ex_uni(w.ids), ex_uni(w.beg), ex_uni(w.end), ex_uni(w.wper), ex_uni(w.qlist), ex_uni(w.nlive), ex_uni(w.seg)};
}

// per (wave, query of the tile): the query's interval, its segment, and where hit number pos goes: at dbase + pos iff plo <= pos < phi
template <int Q>
__device__ __forceinline__ void rg_places(const RgGArgs &a, const RgWgU &d, uint32_t lane, uint32_t wave, uint64_t *klo, uint64_t *khi,
                                          uint64_t (*dbase)[Q], uint32_t (*plo)[Q], uint32_t (*phi)[Q], uint32_t (*sseg)[Q])
{
    if (lane < Q) {
        const bool live = lane < d.nlive;                      // a partial tile's extra queries: an empty interval, never a hit
        const uint32_t j = live ? a.slots[d.qlist + lane] - a.qslot0 : 0u;
        if (wave == 0) { klo[lane] = live ? a.klo[j] : ~0ull; khi[lane] = live ? a.khi[j] : 0ull; }
        const uint32_t seg = live ? a.qseg[j] + d.seg + wave : 0u;
        uint64_t db = 0; uint32_t lo = 0, hi = 0;
        if (live && a.oid) {
            if (!a.seg_base) { db = (uint64_t)seg * a.scap; hi = a.scap; }
            else if (a.cnt[seg] > a.scap) {                    // the segments that fit their staging come from k_range_gather
                const uint64_t sb = a.seg_base[seg], c = a.cnt[seg];
                db = sb - a.w0;                                // modulo 2^64: only positions inside the window are used
                lo = (uint32_t)(sb < a.w0 ? std::min<uint64_t>(c, a.w0 - sb) : 0);
                hi = (uint32_t)(sb < a.w1 ? std::min<uint64_t>(c, a.w1 - sb) : 0);
            }
        }
        dbase[wave][lane] = db; plo[wave][lane] = lo; phi[wave][lane] = hi; sseg[wave][lane] = seg;
    }
}

// k_range_scan with its tile, slice, row list and segments read from wg[blockIdx.x].  RPS = 64 / LPR rows per wave slot, RIF slots per wave round.
template <class OP, int HOP, int LPR, int RIF, int Q>
__global__ void __launch_bounds__(EX_THREADS)
k_range_scan_g(const RgGArgs a)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
    uint8_t *q_lds = lds;
    __shared__ float qn[Q];
    __shared__ uint64_t klo[Q], khi[Q], dbase[EX_WAVES][Q];
    __shared__ uint32_t plo[EX_WAVES][Q], phi[EX_WAVES][Q], sseg[EX_WAVES][Q];
    constexpr int RPS = 64 / LPR, RW = RIF * RPS;
    const RgWgU d = rg_desc(a.wg);
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6, sub = lane / LPR, sl = lane % LPR;
    const bool window = a.seg_base != nullptr;

    ex_park_slots<OP, HOP, Q>(a.queries, a.slots + d.qlist, d.nlive, a.pitch, a.cap_sp, q_lds, qn,
                              [&] { rg_places<Q>(a, d, lane, wave, klo, khi, dbase, plo, phi, sseg); });

    const uint32_t beg = (uint32_t)std::min<uint64_t>((uint64_t)d.beg + (uint64_t)wave * d.wper, d.end);
    const uint32_t end = (uint32_t)std::min<uint64_t>((uint64_t)beg + d.wper, d.end);
    const uint32_t *ids = d.ids != RG_NO_IDS ? a.ids + d.ids : nullptr;
    if (window) {                                              // nothing of this wave's in the window: no row is read
        bool any = false;
        for (int i = 0; i < Q; i++) any |= plo[wave][i] < phi[wave][i];
        if (!any) return;
    }
    uint32_t cnt[Q];
#pragma unroll
    for (int i = 0; i < Q; i++) cnt[i] = 0;
    for (uint32_t b = beg; b < end; b += RW) {
        uint32_t rid[RIF]; bool ok[RIF]; const uint8_t *rp[RIF];
#pragma unroll
        for (int j = 0; j < RIF; j++) {
            const uint32_t r = b + j * RPS + sub;
            ok[j] = r < end;
            rid[j] = ids ? ids[ok[j] ? r : beg] : a.row0 + (ok[j] ? r : beg);   // slots past the segment re-read its first row; never hits
            rp[j] = a.rows + (size_t)rid[j] * a.pitch;
        }
        auto emit = [&](int i, int j, double v) {              // rows of slot j ascend with the lane, and slot j + 1 follows slot j
            const uint64_t key = ex_key(v);
            const bool hit = sl == 0 && ok[j] && klo[i] <= key && key <= khi[i];
            const uint64_t m = __ballot(hit);
            if (hit) {
                const uint32_t pos = cnt[i] + rg_below(m);
                if (pos >= plo[wave][i] && pos < phi[wave][i]) {
                    const size_t o = (size_t)(dbase[wave][i] + pos);
                    a.oid[o] = rid[j];
                    if (a.okey) a.okey[o] = key;
                }
            }
            cnt[i] += (uint32_t)__popcll(m);
        };
        ex_eval<OP, HOP, LPR, RIF, Q>(q_lds, qn, rp, a.pitch, a.cap_sp, sl, emit);
    }
    if (!window && lane == 0) {
#pragma unroll
        for (int i = 0; i < Q; i++)
            if ((uint32_t)i < d.nlive) a.cnt[sseg[wave][i]] = cnt[i];
    }
}

// k_range_scan_sc in the same way: <-> `<` / `<=` on f32 rows through the 8-bit sidecar (64 lanes per row); the threshold key of query i is khi[i]
template <class OP, int HOP, int RIF, int Q>
__global__ void __launch_bounds__(EX_THREADS)
k_range_scan_sc_g(const RgGArgs a, const ScArgs c)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
    uint8_t *q_lds = lds;
    __shared__ float qn[Q];
    __shared__ uint64_t klo[Q], khi[Q], dbase[EX_WAVES][Q];
    __shared__ uint32_t plo[EX_WAVES][Q], phi[EX_WAVES][Q], sseg[EX_WAVES][Q], st_coded, st_fetched;
    const RgWgU d = rg_desc(a.wg);
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const bool window = a.seg_base != nullptr;
    const uint32_t live = (1u << d.nlive) - 1u;

    ex_park_slots<OP, HOP, Q>(a.queries, a.slots + d.qlist, d.nlive, a.pitch, a.cap_sp, q_lds, qn, [&] {
        if (threadIdx.x == 0) { st_coded = 0; st_fetched = 0; }
        rg_places<Q>(a, d, lane, wave, klo, khi, dbase, plo, phi, sseg);
    });

    const uint32_t beg = (uint32_t)std::min<uint64_t>((uint64_t)d.beg + (uint64_t)wave * d.wper, d.end);
    uint32_t end = (uint32_t)std::min<uint64_t>((uint64_t)beg + d.wper, d.end);
    const uint32_t *ids = d.ids != RG_NO_IDS ? a.ids + d.ids : nullptr;
    if (window) {                                              // nothing of this wave's in the window: no row is read
        bool any = false;
        for (int i = 0; i < Q; i++) any |= plo[wave][i] < phi[wave][i];
        if (!any) end = beg;
    }
    uint32_t cnt[Q], nf = 0;
#pragma unroll
    for (int i = 0; i < Q; i++) cnt[i] = 0;
    for (uint32_t b = beg; b < end; b += SC_ROWS) {
        uint32_t rid4[SC_P];
#pragma unroll
        for (int p = 0; p < SC_P; p++) {
            const uint32_t r = b + 4u * p + (lane >> 4);
            rid4[p] = ids ? ids[r < end ? r : beg] : a.row0 + (r < end ? r : beg);
        }
        uint32_t m = sc_survivors<Q>(c, q_lds, rid4, end - b < (uint32_t)SC_ROWS ? end - b : (uint32_t)SC_ROWS, khi, live, lane);
        nf += (uint32_t)__popc(m);
        while (m) {                                            // survivors in row order, RIF at a time
            uint32_t rid[RIF]; bool ok[RIF]; const uint8_t *rp[RIF];
#pragma unroll
            for (int j = 0; j < RIF; j++) {
                ok[j] = m != 0;
                const uint32_t r = ok[j] ? b + (uint32_t)__builtin_ctz(m) : beg;   // slots past the survivors re-read the segment's first row; never hits
                m &= m - 1u;
                rid[j] = ids ? ids[r] : a.row0 + r;
                rp[j] = a.rows + (size_t)rid[j] * a.pitch;
            }
            auto emit = [&](int i, int j, double v) {          // one row per slot: lane 0 holds its value
                const uint64_t key = ex_key(v);
                const bool hit = lane == 0 && ok[j] && klo[i] <= key && key <= khi[i];
                if (hit) {
                    const uint32_t pos = cnt[i];
                    if (pos >= plo[wave][i] && pos < phi[wave][i]) {
                        const size_t o = (size_t)(dbase[wave][i] + pos);
                        a.oid[o] = rid[j];
                        if (a.okey) a.okey[o] = key;
                    }
                }
                cnt[i] += (uint32_t)__popcll(__ballot(hit));
            };
            ex_eval<OP, HOP, 64, RIF, Q>(q_lds, qn, rp, a.pitch, a.cap_sp, lane, emit);
        }
    }
    if (lane == 0) {
        if (!window) {
#pragma unroll
            for (int i = 0; i < Q; i++)
                if ((uint32_t)i < d.nlive) a.cnt[sseg[wave][i]] = cnt[i];
        }
        atomicAdd(&st_coded, end - beg); atomicAdd(&st_fetched, nf);
    }
    __syncthreads();
    if (threadIdx.x == 0) { atomicAdd(c.stats, (unsigned long long)st_coded); atomicAdd(c.stats + 1, (unsigned long long)st_fetched); }
}

// k_range_compact for several bitmaps in one launch: bitmap blockIdx.y (n_words words and per-word offsets each, one after the other) -> the list
// at out + base[y], in row order
struct RgCompactBases { uint64_t base[HX_EXACT_MAX_FILTERS]; };
__global__ void k_range_compact_g(const uint64_t *__restrict__ words, const uint32_t *__restrict__ woff, uint64_t n_words, uint64_t n_rows, uint32_t row0,
                                  uint32_t *__restrict__ out, const RgCompactBases b)
{
    const uint64_t w = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= n_words) return;
    uint64_t bits = words[(uint64_t)blockIdx.y * n_words + w];
    if (w == n_words - 1 && (n_rows & 63)) bits &= (1ull << (n_rows & 63)) - 1;
    uint32_t *list = out + b.base[blockIdx.y];
    uint32_t pos = woff[(uint64_t)blockIdx.y * n_words + w];
    while (bits) { const int bi = __builtin_ctzll(bits); list[pos++] = row0 + (uint32_t)(w * 64 + bi); bits &= bits - 1; }
}

template <class OP, int HOP, int LPR, int RIF, int Q>
hipError_t rgg_launch(hx_engine *e, const RgGArgs &a, uint32_t n_wg)
{
    const size_t lds = (size_t)Q * a.pitch;
    static thread_local uint64_t attr_devices = 0;            // the attribute is per device: set it on each device this thread launches on
    const uint64_t bit = 1ull << (e->device & 63);
    if (lds > 60 * 1024 && !(attr_devices & bit)) {           // Q * pitch <= 64 KiB plus the static arrays
        hipError_t s = hipFuncSetAttribute((const void *)k_range_scan_g<OP, HOP, LPR, RIF, Q>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024 - 4096);
        if (s != hipSuccess) return s;
        attr_devices |= bit;
    }
    hipLaunchKernelGGL((k_range_scan_g<OP, HOP, LPR, RIF, Q>), dim3(n_wg), dim3(EX_THREADS), lds, e->stream, a);
    return hipGetLastError();
}
template <int RIF, int Q>
hipError_t rgg_launch_sc(hx_engine *e, const RgGArgs &a, const ScArgs &c, uint32_t n_wg)
{
    const size_t lds = (size_t)Q * a.pitch;
    static thread_local uint64_t attr_devices = 0;
    const uint64_t bit = 1ull << (e->device & 63);
    if (lds > 60 * 1024 && !(attr_devices & bit)) {
        hipError_t s = hipFuncSetAttribute((const void *)k_range_scan_sc_g<OpF32<K_L2>, HX_OP_L2, RIF, Q>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024 - 4096);
        if (s != hipSuccess) return s;
        attr_devices |= bit;
    }
    hipLaunchKernelGGL((k_range_scan_sc_g<OpF32<K_L2>, HX_OP_L2, RIF, Q>), dim3(n_wg), dim3(EX_THREADS), lds, e->stream, a, c);
    return hipGetLastError();
}
// the (LPR, RIF) of a tile size are those of hx_exact_range's kernels
template <class OP, int HOP>
hipError_t rgg_dispatch_q(hx_engine *e, const RgGArgs &a, uint32_t Q, uint32_t n_wg)
{
    if (a.pitch > 128) {
        if (Q == 16) return rgg_launch<OP, HOP, 64, 2, 16>(e, a, n_wg);
        if (Q == 4) return rgg_launch<OP, HOP, 64, 4, 4>(e, a, n_wg);
        return rgg_launch<OP, HOP, 64, 4, 1>(e, a, n_wg);
    }
    if (Q == 16) return rgg_launch<OP, HOP, 8, 2, 16>(e, a, n_wg);
    if (Q == 4) return rgg_launch<OP, HOP, 8, 4, 4>(e, a, n_wg);
    return rgg_launch<OP, HOP, 8, 4, 1>(e, a, n_wg);
}
template <template <int> class OPT>
hipError_t rgg_dispatch_float(hx_engine *e, int op, const RgGArgs &a, uint32_t Q, uint32_t n_wg)
{
    switch (op) {
    case HX_OP_L2: return rgg_dispatch_q<OPT<K_L2>, HX_OP_L2>(e, a, Q, n_wg);
    case HX_OP_NEG_IP: return rgg_dispatch_q<OPT<K_IP>, HX_OP_NEG_IP>(e, a, Q, n_wg);
    case HX_OP_COSINE: return rgg_dispatch_q<OPT<K_IP>, HX_OP_COSINE>(e, a, Q, n_wg);
    default: return rgg_dispatch_q<OPT<K_L1>, HX_OP_L1>(e, a, Q, n_wg);
    }
}
hipError_t rgg_scan(hx_engine *e, int op, const RgGArgs &a, uint32_t Q, uint32_t n_wg)
{
    if (e->dtype == HX_F32) return rgg_dispatch_float<OpF32>(e, op, a, Q, n_wg);
    if (e->dtype == HX_F16) return rgg_dispatch_float<OpF16>(e, op, a, Q, n_wg);
    if (e->dtype == HX_BIT) return op == HX_OP_HAMMING ? rgg_dispatch_q<OpHamming, HX_OP_HAMMING>(e, a, Q, n_wg)
                                                       : rgg_dispatch_q<OpJaccard, HX_OP_JACCARD>(e, a, Q, n_wg);
    switch (op) {                                             // sparsevec: one lane per pair
    case HX_OP_L2: return rgg_launch<OpSparse<K_L2>, HX_OP_L2, 1, 1, 1>(e, a, n_wg);
    case HX_OP_NEG_IP: return rgg_launch<OpSparse<K_L2>, HX_OP_NEG_IP, 1, 1, 1>(e, a, n_wg);
    case HX_OP_COSINE: return rgg_launch<OpSparse<K_L2>, HX_OP_COSINE, 1, 1, 1>(e, a, n_wg);
    default: return rgg_launch<OpSparse<K_L2>, HX_OP_L1, 1, 1, 1>(e, a, n_wg);
    }
}

// The body of hx_exact_range_filtered and hx_exact_range_set.  The filter source is host bitmaps (filters; set == nullptr) or the resident lists of a
// filter set (set; filters unused): then the counts are the set's offsets, nothing is uploaded or compacted and the set's id array is the id base.
int rgf_run(hx_engine *e, int op, int cmp, const double *radius, uint32_t first_query, uint32_t nq, uint64_t first_row, uint64_t n_rows,
            uint32_t n_filters, const uint64_t *const *filters, const hx_filterset *set, const int32_t *filter_of, int order, uint64_t cap,
            uint64_t *offsets_out, uint32_t *ids_out, double *dist_out, uint64_t *total_out)
{
    const bool bit = e->dtype == HX_BIT;
    if (op < HX_OP_L2 || op > HX_OP_JACCARD || bit != (op == HX_OP_HAMMING || op == HX_OP_JACCARD))
        return e->fail(HX_E_ARG, "operator is not defined for this column type");
    if (cmp < HX_CMP_LT || cmp > HX_CMP_GE) return e->fail(HX_E_ARG, "comparison must be one of HX_CMP_*");
    if (order != HX_RANGE_BY_ROW && order != HX_RANGE_BY_DISTANCE) return e->fail(HX_E_ARG, "order must be one of HX_RANGE_BY_*");
    if (first_row > e->n_rows || n_rows > e->n_rows - first_row) return e->fail(HX_E_ARG, "row range past the stored rows");
    if (first_row + n_rows > 0xFFFFFFFFull) return e->fail(HX_E_ARG, "row range past 2^32 - 1");
    if ((uint64_t)first_query + nq > e->n_queries) return e->fail(HX_E_ARG, "query range past the uploaded query slots");
    if (nq > 0 && !radius) return e->fail(HX_E_ARG, "NULL radius");
    if (!offsets_out || !total_out) return e->fail(HX_E_ARG, "NULL offsets or total output");
    if (!ids_out && dist_out) return e->fail(HX_E_ARG, "values without ids");
    std::vector<int32_t> local_of; uint32_t set_f[HX_EXACT_MAX_FILTERS];   // a set: the call's distinct filters stand for the bitmaps
    if (set) {
        const int rc = hx_filterset_localize(e, set, nq, filter_of, local_of, set_f, &n_filters);
        if (rc) return rc;
        if (filter_of) filter_of = local_of.data();
    } else {
        if (n_filters > HX_EXACT_MAX_FILTERS) return e->fail(HX_E_ARG, "more than HX_EXACT_MAX_FILTERS filters");
        if (n_filters > 0 && !filters) return e->fail(HX_E_ARG, "NULL filters with n_filters > 0");
    }
    auto set_off = [&](uint32_t v) { return set->off[set_f[v - 1]]; };
    auto set_cnt = [&](uint32_t v) { return set->off[(size_t)set_f[v - 1] + 1] - set->off[set_f[v - 1]]; };
    // group v + 1 holds the queries of filter v (v = -1: no filter)
    uint32_t g_nq[HX_EXACT_MAX_FILTERS + 1] = {};
    if (!filter_of) g_nq[0] = nq;
    else
        for (uint32_t i = 0; i < nq; i++) {
            const int32_t f = filter_of[i];
            if (f < -1 || f >= (int32_t)n_filters) return e->fail(HX_E_ARG, "filter_of entry outside [-1, n_filters)");
            if (f >= 0 && !set && !filters[f]) return e->fail(HX_E_ARG, "a query references a NULL filter");
            g_nq[f + 1]++;
        }
    for (uint32_t v = 0; v <= n_filters; v++)                  // one distinct filter (or no query): this is hx_exact_range with that bitmap
        if (g_nq[v] == nq) {
            const HxIdList one{set && v ? set->d_ids + set_off(v) : nullptr, set && v ? set_cnt(v) : 0};
            return hx_exact_range_src(e, op, cmp, radius, first_query, nq, first_row, n_rows, v && !set ? filters[v - 1] : nullptr, v && set ? &one : nullptr,
                                      order, cap, offsets_out, ids_out, dist_out, total_out);
        }
    const bool count_only = !ids_out, by_dist = order == HX_RANGE_BY_DISTANCE;
    const bool need_key = !count_only && (dist_out || by_dist);
    offsets_out[0] = 0; *total_out = 0;

    // the referenced filters' per-word offsets (popcounts, exclusive scan) and the groups: a referenced filter that passes a row, or no filter
    const uint64_t n_words = (n_rows + 63) / 64;
    const bool sc_legal = op == HX_OP_L2 && (cmp == HX_CMP_LT || cmp == HX_CMP_LE) && e->d_sc_codes;
    uint64_t g_pass[HX_EXACT_MAX_FILTERS + 1] = {}, total_ids = 0, units = 0;
    int32_t g_idx[HX_EXACT_MAX_FILTERS + 1];
    const uint64_t *ref_words[HX_EXACT_MAX_FILTERS]; uint32_t n_ref = 0;
    std::vector<uint32_t> woff;
    std::vector<RgGroup> groups;
    RgCompactBases bases{};
    g_pass[0] = n_rows;
    for (uint32_t v = 0; v <= n_filters; v++) {
        g_idx[v] = -1;
        if (!g_nq[v]) continue;
        if (v > 0 && set) g_pass[v] = set_cnt(v);
        else if (v > 0) {
            const uint64_t *words = filters[v - 1];
            woff.resize((size_t)(n_ref + 1) * n_words);
            uint32_t *wo = woff.data() + (size_t)n_ref * n_words;
            uint64_t n = 0;
            for (uint64_t w = 0; w < n_words; w++) {
                uint64_t b = words[w];
                if (w == n_words - 1 && (n_rows & 63)) b &= (1ull << (n_rows & 63)) - 1;
                wo[w] = (uint32_t)n;
                n += (uint64_t)__builtin_popcountll(b);
            }
            g_pass[v] = n;
            if (!n) continue;
            bases.base[n_ref] = total_ids; ref_words[n_ref++] = words;
        }
        if (!g_pass[v]) continue;
        g_idx[v] = (int32_t)groups.size();
        groups.push_back(RgGroup{g_pass[v], !v ? RG_NO_IDS : set ? set_off(v) : total_ids, sc_legal && sc_enabled(g_pass[v], SC_MIN_ROWS_RANGE)});
        if (v && !set) total_ids += g_pass[v];
    }
    std::vector<int32_t> group_of(nq);
    for (uint32_t i = 0; i < nq; i++) {
        const uint32_t v = filter_of ? (uint32_t)(filter_of[i] + 1) : 0;
        group_of[i] = g_idx[v]; units += g_pass[v];
    }
    if (groups.empty()) { for (uint32_t i = 0; i < nq; i++) offsets_out[i + 1] = 0; return HX_OK; }
    HX_HIP(e, hipSetDevice(e->device));

    // device memory: HX_RANGE_SCRATCH bytes as for hx_exact_range: a quarter for the per-block metadata, a quarter for staging, the rest for the
    // output window (and the sort's second buffer and temporary).  The id lists, bitmaps and per-word offsets are not in the budget.
    const uint32_t pitch = (uint32_t)e->pitch;
    uint64_t budget = 256ull << 20;
    if (const char *env = getenv("HX_RANGE_SCRATCH")) budget = std::max<uint64_t>(64 << 10, strtoull(env, nullptr, 10));
    const std::vector<RgBlock> blocks = rg_plan(group_of, groups, pitch, e->dtype == HX_SPARSE, budget);
    const uint64_t ent_stage = need_key ? 12 : 4;
    uint64_t max_nb = 0, max_seg = 0, max_list = 0, max_wg = 0, max_stage = 0;
    bool any_sc = false;
    for (const RgBlock &b : blocks) {
        max_nb = std::max<uint64_t>(max_nb, b.nq); max_seg = std::max(max_seg, b.nseg); max_list = std::max<uint64_t>(max_list, b.qlist.size());
        max_wg = std::max<uint64_t>(max_wg, b.wg.size());
        max_stage = std::max(max_stage, count_only ? 0 : b.nseg * b.scap(budget, ent_stage));
        any_sc |= b.nwg[3] || b.nwg[4];
    }
    // device: id lists | bitmaps | per-word offsets | first segments, slots and descriptors of a block || interval keys | counts | bases | sort offsets |
    // staging | window: what stands before || is for the whole call and outside the budget
    const size_t o_words = al16((size_t)total_ids * 4), o_woff = o_words + al16((size_t)n_ref * n_words * 8), o_qseg = o_woff + al16((size_t)n_ref * n_words * 4);
    const size_t o_slots = o_qseg + al16((max_nb + 1) * 4), o_wg = o_slots + al16(max_list * 4), o_klo = o_wg + al16(max_wg * sizeof(RgWg));
    const size_t o_khi = o_klo + al16(max_nb * 8), o_cnt = o_khi + al16(max_nb * 8), o_base = o_cnt + al16(max_seg * 4);
    const size_t o_qoff = o_base + al16(max_seg * 8), o_skey = o_qoff + al16((max_nb + 1) * 4);
    const size_t o_sid = o_skey + (need_key ? al16(max_stage * 8) : 0), o_out = o_sid + al16(max_stage * 4);
    const size_t filt = o_klo;
    const uint64_t ent_out = by_dist ? 24 : need_key ? 12 : 4;
    uint64_t W = 0; size_t tmp_bytes = 0;
    if (!count_only) {
        const uint64_t used = o_out - filt + 64, rest = budget > used ? budget - used : 0;
        W = rest / ent_out;
        if (by_dist && W > 0) {                                // the radix sort's temporary, sized for the largest window, shrinks the window
            HX_HIP(e, hipcub::DeviceSegmentedRadixSort::SortPairs(nullptr, tmp_bytes, (const unsigned long long *)nullptr, (unsigned long long *)nullptr,
                                                                  (const uint32_t *)nullptr, (uint32_t *)nullptr, (int)std::min<uint64_t>(W, 1ull << 30),
                                                                  (int)max_nb, (const int *)nullptr, (const int *)nullptr, 0, 64, e->stream));
            W = rest > tmp_bytes + 64 ? (rest - tmp_bytes - 64) / ent_out : 0;
        }
        W = std::min<uint64_t>(W, 1ull << 30);
        if (W == 0) return e->fail(HX_E_NOMEM, "HX_RANGE_SCRATCH leaves no room for the output window");
    }
    const size_t o_okey = o_out, o_oid = o_okey + (need_key ? al16(W * 8) : 0), o_okey2 = o_oid + al16(W * 4), o_oid2 = o_okey2 + (by_dist ? al16(W * 8) : 0);
    const size_t o_tmp = o_oid2 + (by_dist ? al16(W * 4) : 0), o_st = o_tmp + al16(tmp_bytes) + 16, need = o_st + (any_sc ? 16 : 0);
    if (need > e->cap_range) {
        if (e->d_range) (void)hipFree(e->d_range);
        e->d_range = nullptr; e->cap_range = 0;
        if (hipMalloc((void **)&e->d_range, need) != hipSuccess) return e->fail(HX_E_NOMEM, "cannot reserve range-scan scratch in HBM");
        e->cap_range = need;
    }
    uint8_t *d = e->d_range;

    uint64_t launches = 0; double ms = 0.0;
    auto t_begin = [&]() -> hipError_t { return e->timing ? hipEventRecord(e->ev0, e->stream) : hipSuccess; };
    auto t_end = [&]() -> hipError_t { return e->timing ? hipEventRecord(e->ev1, e->stream) : hipSuccess; };   // kind 8 = kernel time
    auto t_add = [&]() -> hipError_t {
        if (!e->timing) return hipSuccess;
        float t = 0.f; hipError_t s = hipEventElapsedTime(&t, e->ev0, e->ev1); ms += t; return s;
    };
    bool compact_timed = false;
    if (n_ref) {                                               // one launch for all referenced bitmaps; it is timed with the first block's pass 1
        for (uint32_t c = 0; c < n_ref; c++)
            HX_HIP(e, hipMemcpyAsync(d + o_words + (size_t)c * n_words * 8, ref_words[c], n_words * 8, hipMemcpyHostToDevice, e->stream));
        HX_HIP(e, hipMemcpyAsync(d + o_woff, woff.data(), (size_t)n_ref * n_words * 4, hipMemcpyHostToDevice, e->stream));
    }

    RgGArgs a{};
    a.rows = e->d_rows; a.queries = e->d_queries; a.pitch = pitch; a.cap_sp = (uint32_t)std::min(e->dim, HX_SPARSE_MAX_NNZ);
    a.ids = set ? set->d_ids : (const uint32_t *)d; a.row0 = (uint32_t)first_row;
    a.slots = (const uint32_t *)(d + o_slots); a.qseg = (const uint32_t *)(d + o_qseg);
    a.klo = (const uint64_t *)(d + o_klo); a.khi = (const uint64_t *)(d + o_khi); a.cnt = (uint32_t *)(d + o_cnt);
    uint64_t *d_base = (uint64_t *)(d + o_base);
    ScArgs c{};
    unsigned long long sc_stats[2] = {0, 0};
    if (any_sc) {
        c.codes = e->d_sc_codes; c.meta = e->d_sc_meta; c.cpitch = e->sc_pitch; c.dim = (uint32_t)e->dim; c.nterm = pitch >> 2;
        c.stats = (unsigned long long *)(d + o_st);
        HX_HIP(e, hipMemsetAsync(d + o_st, 0, 16, e->stream));
    }
    std::vector<uint8_t> meta(o_cnt - o_qseg);                 // first segments, slots, descriptors and interval keys of a block: one upload
    std::vector<uint64_t> base(max_seg);
    std::vector<uint32_t> cnt(max_seg);
    std::vector<int> qoff(max_nb + 1);
    bool writing = !count_only, nomem_sort = false;
    const int neg_zero = op == HX_OP_NEG_IP;
    for (const RgBlock &b : blocks) {
        const uint32_t q0 = b.q0, nb = b.nq;
        const uint32_t scap = count_only ? 0 : b.scap(budget, ent_stage);
        auto scan = [&](const RgGArgs &ra) -> hipError_t {     // one launch per class present
            for (uint32_t cl = 0; cl < RG_CLASSES; cl++) {
                if (!b.nwg[cl]) continue;
                RgGArgs r = ra;
                r.wg = (const RgWg *)(d + o_wg) + b.wg0[cl];
                hipError_t s = cl < 3 ? rgg_scan(e, op, r, RG_CLS_Q[cl], b.nwg[cl])
                                      : cl == 3 ? rgg_launch_sc<4, 4>(e, r, c, b.nwg[cl]) : rgg_launch_sc<4, 1>(e, r, c, b.nwg[cl]);
                if (s != hipSuccess) return s;
                launches++;
            }
            return hipSuccess;
        };
        if (b.nseg == 0) {                                     // no query of the block has a passing row
            for (uint32_t i = 0; i < nb; i++) offsets_out[q0 + i + 1] = offsets_out[q0];
            continue;
        }
        {
            uint64_t *klo = (uint64_t *)(meta.data() + (o_klo - o_qseg)), *khi = (uint64_t *)(meta.data() + (o_khi - o_qseg));
            for (uint32_t i = 0; i < nb; i++) hx_where_keys(cmp, radius[q0 + i], &klo[i], &khi[i]);
            memcpy(meta.data(), b.qseg.data(), ((size_t)nb + 1) * 4);
            uint32_t *slots = (uint32_t *)(meta.data() + (o_slots - o_qseg));
            for (size_t i = 0; i < b.qlist.size(); i++) slots[i] = first_query + q0 + b.qlist[i];
            memcpy(meta.data() + (o_wg - o_qseg), b.wg.data(), b.wg.size() * sizeof(RgWg));
            HX_HIP(e, hipMemcpyAsync(d + o_qseg, meta.data(), meta.size(), hipMemcpyHostToDevice, e->stream));
        }
        // pass 1: counts, and the hits that fit their segment's staging
        a.qslot0 = first_query + q0; a.scap = writing ? scap : 0; a.seg_base = nullptr; a.w0 = a.w1 = 0;
        a.okey = writing && need_key ? (uint64_t *)(d + o_skey) : nullptr; a.oid = writing ? (uint32_t *)(d + o_sid) : nullptr;
        HX_HIP(e, t_begin());
        if (n_ref && !compact_timed) {
            hipLaunchKernelGGL(k_range_compact_g, dim3((uint32_t)((n_words + 255) / 256), n_ref), dim3(256), 0, e->stream, (const uint64_t *)(d + o_words),
                               (const uint32_t *)(d + o_woff), n_words, n_rows, (uint32_t)first_row, (uint32_t *)d, bases);
            HX_HIP(e, hipGetLastError());
            launches++; compact_timed = true;
        }
        HX_HIP(e, scan(a));
        HX_HIP(e, t_end());
        HX_HIP(e, hipMemcpyAsync(cnt.data(), a.cnt, (size_t)b.nseg * 4, hipMemcpyDeviceToHost, e->stream));
        if (any_sc) HX_HIP(e, hipMemcpyAsync(sc_stats, d + o_st, 16, hipMemcpyDeviceToHost, e->stream));   // running totals of this call
        HX_HIP(e, hipStreamSynchronize(e->stream));
        HX_HIP(e, t_add());
        uint64_t pos = 0; bool overflow = false;                 // CSR positions relative to the block's first hit
        for (uint32_t i = 0; i < nb; i++) {
            for (uint32_t s = b.qseg[i]; s < b.qseg[i + 1]; s++) { base[s] = pos; pos += cnt[s]; overflow |= cnt[s] > scap; }
            offsets_out[q0 + i + 1] = offsets_out[q0] + pos;
        }
        const uint64_t blk0 = offsets_out[q0], blk_n = pos;
        if (writing && blk0 + blk_n > cap) writing = false;     // capacity exceeded: count the rest
        if (!writing || blk_n == 0) continue;
        HX_HIP(e, hipMemcpyAsync(d_base, base.data(), (size_t)b.nseg * 8, hipMemcpyHostToDevice, e->stream));
        // output windows [w0, w1) of the block's hits; by distance, whole queries [qa, qb)
        for (uint64_t w0 = 0, qa = 0; w0 < blk_n;) {
            uint64_t w1 = std::min(blk_n, w0 + W), qb = qa;
            if (by_dist) {
                while (qb < nb && offsets_out[q0 + qb + 1] - blk0 <= w0 + W) qb++;
                if (qb == qa) { nomem_sort = true; writing = false; break; }   // one query's hits exceed the window
                w1 = offsets_out[q0 + qb] - blk0;
                for (uint64_t i = qa; i <= qb; i++) qoff[i - qa] = (int)(offsets_out[q0 + i] - blk0 - w0);
                HX_HIP(e, hipMemcpyAsync(d + o_qoff, qoff.data(), (qb - qa + 1) * 4, hipMemcpyHostToDevice, e->stream));
            }
            bool rescan = false;
            if (overflow)
                for (size_t s = 0; s < (size_t)b.nseg && !rescan; s++) rescan = cnt[s] > scap && base[s] < w1 && base[s] + cnt[s] > w0;
            uint64_t *okey = need_key ? (uint64_t *)(d + o_okey) : nullptr;
            uint32_t *oid = (uint32_t *)(d + o_oid);
            HX_HIP(e, t_begin());
            hipLaunchKernelGGL(k_range_gather, dim3((uint32_t)std::min<uint64_t>(4096, (b.nseg + 3) / 4)), dim3(256), 0, e->stream,
                               (const uint64_t *)(d + o_skey), (const uint32_t *)(d + o_sid), (const uint32_t *)a.cnt, (const uint64_t *)d_base,
                               b.nseg, scap, w0, w1, okey, oid);
            HX_HIP(e, hipGetLastError());
            launches++;
            if (rescan) {                                        // the overflowed segments' hits in this window, straight to their positions
                RgGArgs r = a;
                r.scap = scap; r.seg_base = d_base; r.w0 = w0; r.w1 = w1; r.okey = okey; r.oid = oid;
                HX_HIP(e, scan(r));
            }
            const uint64_t wn = w1 - w0;
            if (by_dist) {                                       // stable: equal keys keep row order
                size_t tb = tmp_bytes;
                HX_HIP(e, hipcub::DeviceSegmentedRadixSort::SortPairs(d + o_tmp, tb, (const unsigned long long *)okey, (unsigned long long *)(d + o_okey2),
                                                                      (const uint32_t *)oid, (uint32_t *)(d + o_oid2), (int)wn, (int)(qb - qa),
                                                                      (const int *)(d + o_qoff), (const int *)(d + o_qoff) + 1, 0, 64, e->stream));
                okey = (uint64_t *)(d + o_okey2); oid = (uint32_t *)(d + o_oid2);
                launches++;
            }
            if (dist_out) {
                hipLaunchKernelGGL(k_range_values, dim3((uint32_t)((wn + 255) / 256)), dim3(256), 0, e->stream, okey, wn, neg_zero);
                HX_HIP(e, hipGetLastError());
                launches++;
            }
            HX_HIP(e, t_end());
            HX_HIP(e, hipMemcpyAsync(ids_out + blk0 + w0, oid, wn * 4, hipMemcpyDeviceToHost, e->stream));
            if (dist_out) HX_HIP(e, hipMemcpyAsync(dist_out + blk0 + w0, okey, wn * 8, hipMemcpyDeviceToHost, e->stream));
            if (any_sc && rescan) HX_HIP(e, hipMemcpyAsync(sc_stats, d + o_st, 16, hipMemcpyDeviceToHost, e->stream));
            HX_HIP(e, hipStreamSynchronize(e->stream));
            HX_HIP(e, t_add());
            w0 = w1; qa = qb;
        }
    }
    *total_out = offsets_out[nq];
    e->xs_coded += sc_stats[0]; e->xs_fetched += sc_stats[1];
    if (e->timing) {
        e->last_ms = (float)ms;
        e->stat_range.launches += launches; e->stat_range.units += units; e->stat_range.ms += ms;
    }
    if (nomem_sort) return e->fail(HX_E_NOMEM, "one query's hits exceed HX_RANGE_SCRATCH (ordered by distance)");
    if (!count_only && *total_out > cap) return e->fail(HX_E_NOMEM, "capacity exceeded");
    return HX_OK;
}

} // namespace

hipError_t hx_range_compact_lists(hx_engine *e, const uint64_t *d_words, const uint32_t *d_woff, uint64_t n_words, uint64_t n_rows, uint32_t row0,
                                  uint32_t *out, const uint64_t *base, uint32_t n)
{
    RgCompactBases b{};
    for (uint32_t i = 0; i < n && i < HX_EXACT_MAX_FILTERS; i++) b.base[i] = base[i];
    hipLaunchKernelGGL(k_range_compact_g, dim3((uint32_t)((n_words + 255) / 256), std::min<uint32_t>(n, HX_EXACT_MAX_FILTERS)), dim3(256), 0, e->stream, d_words, d_woff,
                       n_words, n_rows, row0, out, b);
    return hipGetLastError();
}

// =================================================================================================
// C ABI
// =================================================================================================
extern "C" int hx_exact_range_filtered(hx_engine *e, int op, int cmp, const double *radius, uint32_t first_query, uint32_t nq,
                                       uint64_t first_row, uint64_t n_rows,
                                       uint32_t n_filters, const uint64_t *const *filters, const int32_t *filter_of,
                                       int order, uint64_t cap,
                                       uint64_t *offsets_out, uint32_t *ids_out, double *dist_out, uint64_t *total_out)
{
    if (!e) return HX_E_ARG;
    return rgf_run(e, op, cmp, radius, first_query, nq, first_row, n_rows, n_filters, filters, nullptr, filter_of, order, cap, offsets_out, ids_out, dist_out,
                   total_out);
}

extern "C" int hx_exact_range_set(hx_engine *e, int op, int cmp, const double *radius, uint32_t first_query, uint32_t nq,
                                  const hx_filterset *s, const int32_t *filter_of, int order, uint64_t cap,
                                  uint64_t *offsets_out, uint32_t *ids_out, double *dist_out, uint64_t *total_out)
{
    if (!e) return HX_E_ARG;
    if (const int rc = hx_filterset_usable(e, s)) return rc;
    return rgf_run(e, op, cmp, radius, first_query, nq, s->first_row, s->n_rows, 0, nullptr, s, filter_of, order, cap, offsets_out, ids_out, dist_out, total_out);
}
