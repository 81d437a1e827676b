// hx_range.hip -- exact distance-threshold scans on the device: the sequential-scan plans of `WHERE v <op> q < r` (heap order) and
// `WHERE v <op> q < r ORDER BY v <op> q` (no LIMIT), i.e. the executor calling the operator function on every heap row and keeping the rows
// where the float8 comparison holds (include/hnswrx.h: hx_exact_range).
//
// Values and the row streaming are those of hx_exact_core.h, so a row's value is bit for bit the one hx_exact_search returns.  The four
// comparisons are one interval of order keys per query, [klo, khi] (ex_key makes float8 comparison the integer one), set on the host.
//
// Pass 1 (k_range_scan): workgroup (query tile of Q queries, row slice); its EX_WAVES waves each own a contiguous segment of the slice, so
//   a (query, segment) pair has one writer and hits are compacted in row order with a ballot and a lane prefix count, no atomics.  The
//   first `scap` hits of a segment go to its staging area; all are counted.  Count-only calls stage nothing.
// The host scans the counts into CSR offsets.  Output then goes through windows of the device buffer: k_range_gather copies the segments
//   that fit their staging, in segment (= row) order, and k_range_scan runs again over the tiles whose segments overflowed, now writing
//   each hit straight to its CSR position when that lies in the window (a wave with nothing in the window returns at once).
// HX_RANGE_BY_DISTANCE: each window holds whole queries, sorted by a stable segmented radix sort on the order key (hipcub), so equal
//   values keep row order.
// A filter bitmap is compacted into a row-id list in row order (per-word offsets: popcount + exclusive scan, then k_range_compact);
// rows that fail it are never read.
//
// <-> with `<` / `<=` on an f32 engine that keeps the 8-bit sidecar (k_range_scan_sc, query tiles of 1 and 4; hx_exact_sc.h): a wave
//   first reads the code rows of SC_ROWS rows and evaluates only those whose proven lower bound does not already lie past the radius, in row
//   order, through the same ex_eval and ballot + prefix count.  Count-only calls and the window pass take the same kernel.
#include "hx_range_core.h"

namespace {

struct RgArgs {
    const uint8_t *rows, *queries; uint32_t pitch, cap_sp;   // cap_sp: sparsevec record capacity
    uint32_t qslot0, nq;                                      // queries of this block: slots qslot0 .. qslot0 + nq - 1
    const uint32_t *ids; uint32_t row0, n, wper, G;           // rows ids[0..n) or row0 + [0..n); segment g = [g * wper, (g + 1) * wper), G per query
    const uint64_t *klo, *khi;                                // query of the block: a hit iff klo <= key <= khi
    uint32_t *cnt;                                            // [query][segment] hit counts: pass 1 writes them, a window pass reads them
    uint32_t scap;                                            // staging entries per segment (pass 1: segment s at s * scap)
    const uint64_t *seg_base; uint64_t w0, w1;                // window pass (seg_base != nullptr): CSR position of a segment's first hit, window
    uint64_t *okey; uint32_t *oid;                            // staging (pass 1) or window output; oid == nullptr: count only, okey may be
};

// Q queries x one row slice of EX_WAVES segments.  RPS = 64 / LPR rows per wave slot, RIF slots per wave round.
template <class OP, int HOP, int LPR, int RIF, int Q>
__global__ void __launch_bounds__(EX_THREADS)
k_range_scan(const RgArgs a)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
    uint8_t *q_lds = lds;
    __shared__ float qn[Q];
    __shared__ uint64_t klo[Q], khi[Q], dbase[EX_WAVES][Q];
    __shared__ uint32_t plo[EX_WAVES][Q], phi[EX_WAVES][Q];
    constexpr int RPS = 64 / LPR, RW = RIF * RPS;
    const uint32_t tile = blockIdx.x, lane = threadIdx.x & 63u, wave = threadIdx.x >> 6, sub = lane / LPR, sl = lane % LPR;
    const uint32_t g = blockIdx.y * EX_WAVES + wave;
    const bool window = a.seg_base != nullptr;

    ex_park<OP, HOP, Q>(a.queries, a.qslot0, a.nq, tile, a.pitch, a.cap_sp, q_lds, qn, [&] {
        if (lane < Q) {                                        // per (wave, query): hit number pos is written at dbase + pos iff plo <= pos < phi
            const uint32_t q = tile * Q + lane;
            const bool live = q < a.nq;                        // a partial tile's extra queries: an empty interval, never a hit
            if (wave == 0) { klo[lane] = live ? a.klo[q] : ~0ull; khi[lane] = live ? a.khi[q] : 0ull; }
            uint64_t db = 0; uint32_t lo = 0, hi = 0;
            if (live && a.oid) {
                const size_t seg = (size_t)q * a.G + g;
                if (!window) { db = seg * a.scap; hi = a.scap; }
                else if (a.cnt[seg] > a.scap) {                // the segments that fit their staging come from k_range_gather
                    const uint64_t sb = a.seg_base[seg], c = a.cnt[seg];
                    db = sb - a.w0;                            // modulo 2^64: only positions inside the window are used
                    lo = (uint32_t)(sb < a.w0 ? std::min<uint64_t>(c, a.w0 - sb) : 0);
                    hi = (uint32_t)(sb < a.w1 ? std::min<uint64_t>(c, a.w1 - sb) : 0);
                }
            }
            dbase[wave][lane] = db; plo[wave][lane] = lo; phi[wave][lane] = hi;
        }
    });

    const uint32_t beg = (uint32_t)std::min<uint64_t>((uint64_t)g * a.wper, a.n), end = (uint32_t)std::min<uint64_t>((uint64_t)beg + a.wper, a.n);
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
            rid[j] = a.ids ? a.ids[ok[j] ? r : beg] : a.row0 + (ok[j] ? r : beg);   // slots past the segment re-read its first row; never hits
            rp[j] = a.rows + (size_t)rid[j] * a.pitch;
        }
        auto emit = [&](int i, int j, double v) {              // rows of slot j ascend with the lane, and slot j + 1 follows slot j
            const uint64_t key = ex_key(v);
            const bool hit = sl == 0 && ok[j] && klo[i] <= key && key <= khi[i];
            const uint64_t m = __ballot(hit);
            if (hit) {
                const uint32_t pos = cnt[i] + rg_below(m);
                if (pos >= plo[wave][i] && pos < phi[wave][i]) {
                    const size_t d = (size_t)(dbase[wave][i] + pos);
                    a.oid[d] = rid[j];
                    if (a.okey) a.okey[d] = key;
                }
            }
            cnt[i] += (uint32_t)__popcll(m);
        };
        ex_eval<OP, HOP, LPR, RIF, Q>(q_lds, qn, rp, a.pitch, a.cap_sp, sl, emit);
    }
    if (!window && lane == 0) {
#pragma unroll
        for (int i = 0; i < Q; i++)
            if (tile * Q + i < a.nq) a.cnt[(size_t)(tile * Q + i) * a.G + g] = cnt[i];
    }
}

// The sidecar variant for <-> `<` / `<=` on f32 rows (64 lanes per row): the threshold key of query i is khi[i], nothing is shared.
template <class OP, int HOP, int RIF, int Q>
__global__ void __launch_bounds__(EX_THREADS)
k_range_scan_sc(const RgArgs a, const ScArgs c)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
    uint8_t *q_lds = lds;
    __shared__ float qn[Q];
    __shared__ uint64_t klo[Q], khi[Q], dbase[EX_WAVES][Q];
    __shared__ uint32_t plo[EX_WAVES][Q], phi[EX_WAVES][Q], st_coded, st_fetched;
    const uint32_t tile = blockIdx.x, lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t g = blockIdx.y * EX_WAVES + wave;
    const bool window = a.seg_base != nullptr;
    uint32_t live = 0;
#pragma unroll
    for (int i = 0; i < Q; i++) live |= (tile * Q + i < a.nq ? 1u : 0u) << i;

    ex_park<OP, HOP, Q>(a.queries, a.qslot0, a.nq, tile, a.pitch, a.cap_sp, q_lds, qn, [&] {
        if (threadIdx.x == 0) { st_coded = 0; st_fetched = 0; }
        if (lane < Q) {                                        // as k_range_scan
            const uint32_t q = tile * Q + lane;
            const bool lv = q < a.nq;
            if (wave == 0) { klo[lane] = lv ? a.klo[q] : ~0ull; khi[lane] = lv ? a.khi[q] : 0ull; }
            uint64_t db = 0; uint32_t lo = 0, hi = 0;
            if (lv && a.oid) {
                const size_t seg = (size_t)q * a.G + g;
                if (!window) { db = seg * a.scap; hi = a.scap; }
                else if (a.cnt[seg] > a.scap) {
                    const uint64_t sb = a.seg_base[seg], n = a.cnt[seg];
                    db = sb - a.w0;
                    lo = (uint32_t)(sb < a.w0 ? std::min<uint64_t>(n, a.w0 - sb) : 0);
                    hi = (uint32_t)(sb < a.w1 ? std::min<uint64_t>(n, a.w1 - sb) : 0);
                }
            }
            dbase[wave][lane] = db; plo[wave][lane] = lo; phi[wave][lane] = hi;
        }
    });

    const uint32_t beg = (uint32_t)std::min<uint64_t>((uint64_t)g * a.wper, a.n);
    uint32_t end = (uint32_t)std::min<uint64_t>((uint64_t)beg + a.wper, a.n);
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
            rid4[p] = a.ids ? a.ids[r < end ? r : beg] : a.row0 + (r < end ? r : beg);
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
                rid[j] = a.ids ? a.ids[r] : a.row0 + r;
                rp[j] = a.rows + (size_t)rid[j] * a.pitch;
            }
            auto emit = [&](int i, int j, double v) {          // one row per slot: lane 0 holds its value
                const uint64_t key = ex_key(v);
                const bool hit = lane == 0 && ok[j] && klo[i] <= key && key <= khi[i];
                if (hit) {
                    const uint32_t pos = cnt[i];
                    if (pos >= plo[wave][i] && pos < phi[wave][i]) {
                        const size_t d = (size_t)(dbase[wave][i] + pos);
                        a.oid[d] = rid[j];
                        if (a.okey) a.okey[d] = key;
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
                if (tile * Q + i < a.nq) a.cnt[(size_t)(tile * Q + i) * a.G + g] = cnt[i];
        }
        atomicAdd(&st_coded, end - beg); atomicAdd(&st_fetched, nf);
    }
    __syncthreads();
    if (threadIdx.x == 0) { atomicAdd(c.stats, (unsigned long long)st_coded); atomicAdd(c.stats + 1, (unsigned long long)st_fetched); }
}

// filter bitmap -> row-id list in row order: word w's passing rows go to out[woff[w] ..] (woff: exclusive scan of the words' popcounts)
__global__ void k_range_compact(const uint64_t *__restrict__ words, const uint32_t *__restrict__ woff, uint64_t n_words, uint64_t n_rows, uint32_t row0,
                                uint32_t *__restrict__ out)
{
    const uint64_t w = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= n_words) return;
    uint64_t bits = words[w];
    if (w == n_words - 1 && (n_rows & 63)) bits &= (1ull << (n_rows & 63)) - 1;
    uint32_t pos = woff[w];
    while (bits) { const int b = __builtin_ctzll(bits); out[pos++] = row0 + (uint32_t)(w * 64 + b); bits &= bits - 1; }
}

template <class OP, int HOP, int LPR, int RIF, int Q>
hipError_t rg_launch(hx_engine *e, const RgArgs &a, uint32_t tiles)
{
    const size_t lds = (size_t)Q * a.pitch;
    static thread_local uint64_t attr_devices = 0;            // the attribute is per device: set it on each device this thread launches on
    const uint64_t bit = 1ull << (e->device & 63);
    if (lds > 60 * 1024 && !(attr_devices & bit)) {           // Q * pitch <= 64 KiB plus the static arrays
        hipError_t s = hipFuncSetAttribute((const void *)k_range_scan<OP, HOP, LPR, RIF, Q>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024 - 4096);
        if (s != hipSuccess) return s;
        attr_devices |= bit;
    }
    hipLaunchKernelGGL((k_range_scan<OP, HOP, LPR, RIF, Q>), dim3(tiles, a.G / EX_WAVES), dim3(EX_THREADS), lds, e->stream, a);
    return hipGetLastError();
}
template <int RIF, int Q>
hipError_t rg_launch_sc(hx_engine *e, const RgArgs &a, const ScArgs &c, uint32_t tiles)
{
    const size_t lds = (size_t)Q * a.pitch;
    static thread_local uint64_t attr_devices = 0;
    const uint64_t bit = 1ull << (e->device & 63);
    if (lds > 60 * 1024 && !(attr_devices & bit)) {
        hipError_t s = hipFuncSetAttribute((const void *)k_range_scan_sc<OpF32<K_L2>, HX_OP_L2, RIF, Q>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024 - 4096);
        if (s != hipSuccess) return s;
        attr_devices |= bit;
    }
    hipLaunchKernelGGL((k_range_scan_sc<OpF32<K_L2>, HX_OP_L2, RIF, Q>), dim3(tiles, a.G / EX_WAVES), dim3(EX_THREADS), lds, e->stream, a, c);
    return hipGetLastError();
}
template <class OP, int HOP, int LPR>
hipError_t rg_dispatch_q(hx_engine *e, const RgArgs &a, uint32_t Q, uint32_t tiles)
{
    if (Q == 16) return rg_launch<OP, HOP, LPR, 2, 16>(e, a, tiles);
    if (Q == 4) return rg_launch<OP, HOP, LPR, 4, 4>(e, a, tiles);
    return rg_launch<OP, HOP, LPR, 4, 1>(e, a, tiles);
}
template <class OP, int HOP>
hipError_t rg_dispatch_lpr(hx_engine *e, const RgArgs &a, uint32_t Q, uint32_t tiles)
{
    return a.pitch > 128 ? rg_dispatch_q<OP, HOP, 64>(e, a, Q, tiles) : rg_dispatch_q<OP, HOP, 8>(e, a, Q, tiles);
}
template <template <int> class OPT>
hipError_t rg_dispatch_float(hx_engine *e, int op, const RgArgs &a, uint32_t Q, uint32_t tiles)
{
    switch (op) {
    case HX_OP_L2: return rg_dispatch_lpr<OPT<K_L2>, HX_OP_L2>(e, a, Q, tiles);
    case HX_OP_NEG_IP: return rg_dispatch_lpr<OPT<K_IP>, HX_OP_NEG_IP>(e, a, Q, tiles);
    case HX_OP_COSINE: return rg_dispatch_lpr<OPT<K_IP>, HX_OP_COSINE>(e, a, Q, tiles);
    default: return rg_dispatch_lpr<OPT<K_L1>, HX_OP_L1>(e, a, Q, tiles);
    }
}
hipError_t rg_scan(hx_engine *e, int op, const RgArgs &a, uint32_t Q, uint32_t tiles)
{
    if (e->dtype == HX_F32) return rg_dispatch_float<OpF32>(e, op, a, Q, tiles);
    if (e->dtype == HX_F16) return rg_dispatch_float<OpF16>(e, op, a, Q, tiles);
    if (e->dtype == HX_BIT) return op == HX_OP_HAMMING ? rg_dispatch_lpr<OpHamming, HX_OP_HAMMING>(e, a, Q, tiles)
                                                       : rg_dispatch_lpr<OpJaccard, HX_OP_JACCARD>(e, a, Q, tiles);
    switch (op) {                                             // sparsevec: one lane per pair
    case HX_OP_L2: return rg_launch<OpSparse<K_L2>, HX_OP_L2, 1, 1, 1>(e, a, tiles);
    case HX_OP_NEG_IP: return rg_launch<OpSparse<K_L2>, HX_OP_NEG_IP, 1, 1, 1>(e, a, tiles);
    case HX_OP_COSINE: return rg_launch<OpSparse<K_L2>, HX_OP_COSINE, 1, 1, 1>(e, a, tiles);
    default: return rg_launch<OpSparse<K_L2>, HX_OP_L1, 1, 1, 1>(e, a, tiles);
    }
}

} // namespace

// =================================================================================================
// C ABI
// =================================================================================================
// hx_exact_range with its filter source chosen: a host bitmap (row_pass: popcounted, uploaded and compacted here), a row-ordered id list already
// on the device (list: a filter set's; it stands where the compacted bitmap stands, and nothing is uploaded or compacted), or neither
int hx_exact_range_src(hx_engine *e, int op, int cmp, const double *radius, uint32_t first_query, uint32_t nq, uint64_t first_row, uint64_t n_rows,
                       const uint64_t *row_pass, const HxIdList *list, int order, uint64_t cap, uint64_t *offsets_out, uint32_t *ids_out,
                       double *dist_out, uint64_t *total_out)
{
    if (!e) return HX_E_ARG;
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
    const bool count_only = !ids_out, by_dist = order == HX_RANGE_BY_DISTANCE;
    const bool need_key = !count_only && (dist_out || by_dist);

    offsets_out[0] = 0; *total_out = 0;
    if (nq == 0) return HX_OK;
    const uint64_t n_words = (n_rows + 63) / 64;
    std::vector<uint32_t> woff;
    uint64_t n_pass = list ? list->n : n_rows;
    if (row_pass) {                                            // the filter's per-word offsets: popcounts, exclusive scan
        woff.resize(n_words);
        n_pass = 0;
        for (uint64_t w = 0; w < n_words; w++) {
            uint64_t b = row_pass[w];
            if (w == n_words - 1 && (n_rows & 63)) b &= (1ull << (n_rows & 63)) - 1;
            woff[w] = (uint32_t)n_pass;
            n_pass += (uint64_t)__builtin_popcountll(b);
        }
    }
    if (n_pass == 0) { for (uint32_t i = 0; i < nq; i++) offsets_out[i + 1] = 0; return HX_OK; }
    HX_HIP(e, hipSetDevice(e->device));

    // plan: query tile Q and rows per wave round RW (as the exact scan), segments of wper rows (~1024 workgroups over all tiles), query blocks
    const uint32_t pitch = (uint32_t)e->pitch;
    uint32_t Q = 1, RW = 64;
    if (e->dtype != HX_SPARSE) {
        Q = nq >= 16 && 16ull * pitch <= 64 * 1024 ? 16 : nq >= 4 && 4ull * pitch <= 64 * 1024 ? 4 : 1;
        RW = (Q == 16 ? 2 : 4) * (pitch > 128 ? 1 : 8);
    }
    // device memory: HX_RANGE_SCRATCH bytes (default 256 MiB, at least 64 KiB): a quarter for the per-block metadata (interval keys, counts,
    // CSR bases of the segments), a quarter for staging, the rest for the output window (and the sort's second buffer and temporary).
    uint64_t budget = 256ull << 20;
    if (const char *env = getenv("HX_RANGE_SCRATCH")) budget = std::max<uint64_t>(64 << 10, strtoull(env, nullptr, 10));
    const uint32_t tiles_all = (nq + Q - 1) / Q;
    uint64_t S = std::max<uint64_t>(1, std::min<uint64_t>((1024 + tiles_all - 1) / tiles_all, (n_pass + 4ull * EX_WAVES * RW - 1) / (4ull * EX_WAVES * RW)));
    S = std::max<uint64_t>(1, std::min<uint64_t>(S, (budget / 4 / Q - 64) / (EX_WAVES * 12ull)));
    const uint32_t wper = (uint32_t)((n_pass + S * EX_WAVES - 1) / (S * EX_WAVES));
    const uint32_t G = (uint32_t)((n_pass + wper - 1) / wper + EX_WAVES - 1) / EX_WAVES * EX_WAVES;
    const uint64_t meta_q = (uint64_t)G * 12 + 16 + 4;
    const uint32_t nqb = (uint32_t)std::min<uint64_t>(nq, std::max<uint64_t>(Q, budget / 4 / meta_q / Q * Q));
    const uint64_t nseg = (uint64_t)nqb * G, ent_stage = need_key ? 12 : 4;
    const uint32_t scap = count_only ? 0 : (uint32_t)std::min<uint64_t>(wper, budget / 4 / ent_stage / nseg);
    const size_t o_words = row_pass ? al16((size_t)n_pass * 4) : 0, o_woff = o_words + (row_pass ? al16(n_words * 8) : 0);
    const size_t o_klo = o_woff + (row_pass ? al16(n_words * 4) : 0), o_khi = o_klo + al16((size_t)nqb * 8), o_cnt = o_khi + al16((size_t)nqb * 8);
    const size_t o_base = o_cnt + al16(nseg * 4), o_qoff = o_base + al16(nseg * 8), o_skey = o_qoff + al16(((size_t)nqb + 1) * 4);
    const size_t o_sid = o_skey + (need_key ? al16(nseg * scap * 8) : 0), o_out = o_sid + al16(nseg * scap * 4);
    const size_t filt = o_klo;                                 // the filter's arrays are not in the budget (as for hx_exact_search)
    const uint64_t ent_out = by_dist ? 24 : need_key ? 12 : 4;
    uint64_t W = 0; size_t tmp_bytes = 0;
    if (!count_only) {
        const uint64_t used = o_out - filt + 64, rest = budget > used ? budget - used : 0;
        W = rest / ent_out;
        if (by_dist && W > 0) {                                // the radix sort's temporary, sized for the largest window, shrinks the window
            HX_HIP(e, hipcub::DeviceSegmentedRadixSort::SortPairs(nullptr, tmp_bytes, (const unsigned long long *)nullptr, (unsigned long long *)nullptr,
                                                                  (const uint32_t *)nullptr, (uint32_t *)nullptr, (int)std::min<uint64_t>(W, 1ull << 30),
                                                                  (int)nqb, (const int *)nullptr, (const int *)nullptr, 0, 64, e->stream));
            W = rest > tmp_bytes + 64 ? (rest - tmp_bytes - 64) / ent_out : 0;
        }
        W = std::min<uint64_t>(W, 1ull << 30);
        if (W == 0) return e->fail(HX_E_NOMEM, "HX_RANGE_SCRATCH leaves no room for the output window");
    }
    const size_t o_okey = o_out, o_oid = o_okey + (need_key ? al16(W * 8) : 0), o_okey2 = o_oid + al16(W * 4), o_oid2 = o_okey2 + (by_dist ? al16(W * 8) : 0);
    // the sidecar path (<-> with `<` / `<=` on an engine with a sidecar, query tiles of 1 and 4): two counters behind the scratch
    const bool sc = op == HX_OP_L2 && (cmp == HX_CMP_LT || cmp == HX_CMP_LE) && e->d_sc_codes && Q <= 4 && sc_enabled(n_pass, SC_MIN_ROWS_RANGE);
    const size_t o_tmp = o_oid2 + (by_dist ? al16(W * 4) : 0), o_st = o_tmp + al16(tmp_bytes) + 16, need = o_st + (sc ? 16 : 0);
    if (need > e->cap_range) {
        if (e->d_range) (void)hipFree(e->d_range);
        e->d_range = nullptr; e->cap_range = 0;
        if (hipMalloc((void **)&e->d_range, need) != hipSuccess) return e->fail(HX_E_NOMEM, "cannot reserve range-scan scratch in HBM");
        e->cap_range = need;
    }
    uint8_t *d = e->d_range;

    uint64_t launches = 0; double ms = 0.0;
    auto t_begin = [&]() -> hipError_t { return e->timing ? hipEventRecord(e->ev0, e->stream) : hipSuccess; };
    auto t_end = [&]() -> hipError_t {                         // kind 8 = kernel time; callers synchronise before reading it
        return e->timing ? hipEventRecord(e->ev1, e->stream) : hipSuccess;
    };
    auto t_add = [&]() -> hipError_t {
        if (!e->timing) return hipSuccess;
        float t = 0.f; hipError_t s = hipEventElapsedTime(&t, e->ev0, e->ev1); ms += t; return s;
    };
    if (row_pass) {
        HX_HIP(e, hipMemcpyAsync(d + o_words, row_pass, n_words * 8, hipMemcpyHostToDevice, e->stream));
        HX_HIP(e, hipMemcpyAsync(d + o_woff, woff.data(), n_words * 4, hipMemcpyHostToDevice, e->stream));
        HX_HIP(e, t_begin());
        hipLaunchKernelGGL(k_range_compact, dim3((uint32_t)((n_words + 255) / 256)), dim3(256), 0, e->stream, (const uint64_t *)(d + o_words),
                           (const uint32_t *)(d + o_woff), n_words, n_rows, (uint32_t)first_row, (uint32_t *)d);
        HX_HIP(e, hipGetLastError());
        HX_HIP(e, t_end());
        HX_HIP(e, hipStreamSynchronize(e->stream));
        HX_HIP(e, t_add());
        launches++;
    }

    RgArgs a{};
    a.rows = e->d_rows; a.queries = e->d_queries; a.pitch = pitch; a.cap_sp = (uint32_t)std::min(e->dim, HX_SPARSE_MAX_NNZ);
    a.ids = row_pass ? (const uint32_t *)d : list ? list->d : nullptr; a.row0 = (uint32_t)first_row; a.n = (uint32_t)n_pass; a.wper = wper; a.G = G;
    a.klo = (const uint64_t *)(d + o_klo); a.khi = (const uint64_t *)(d + o_khi); a.cnt = (uint32_t *)(d + o_cnt);
    uint64_t *d_base = (uint64_t *)(d + o_base);
    ScArgs c{};
    unsigned long long sc_stats[2] = {0, 0};
    if (sc) {
        c.codes = e->d_sc_codes; c.meta = e->d_sc_meta; c.cpitch = e->sc_pitch; c.dim = (uint32_t)e->dim; c.nterm = pitch >> 2;
        c.stats = (unsigned long long *)(d + o_st);
        HX_HIP(e, hipMemsetAsync(d + o_st, 0, 16, e->stream));
    }
    auto scan = [&](const RgArgs &ra, uint32_t tiles) -> hipError_t {
        if (!sc) return rg_scan(e, op, ra, Q, tiles);
        return Q == 4 ? rg_launch_sc<4, 4>(e, ra, c, tiles) : rg_launch_sc<4, 1>(e, ra, c, tiles);
    };
    std::vector<uint64_t> klo(nqb), khi(nqb), base(nseg);
    std::vector<uint32_t> cnt(nseg);
    std::vector<int> qoff(nqb + 1);
    bool writing = !count_only, nomem_sort = false;
    const int neg_zero = op == HX_OP_NEG_IP;
    for (uint32_t q0 = 0; q0 < nq; q0 += nqb) {
        const uint32_t nb = std::min(nqb, nq - q0), tiles = (nb + Q - 1) / Q;
        for (uint32_t i = 0; i < nb; i++) hx_where_keys(cmp, radius[q0 + i], &klo[i], &khi[i]);
        HX_HIP(e, hipMemcpyAsync(d + o_klo, klo.data(), (size_t)nb * 8, hipMemcpyHostToDevice, e->stream));
        HX_HIP(e, hipMemcpyAsync(d + o_khi, khi.data(), (size_t)nb * 8, hipMemcpyHostToDevice, e->stream));
        // pass 1: counts, and the hits that fit their segment's staging
        a.qslot0 = first_query + q0; a.nq = nb; a.scap = writing ? scap : 0; a.seg_base = nullptr; a.w0 = a.w1 = 0;
        a.okey = writing && need_key ? (uint64_t *)(d + o_skey) : nullptr; a.oid = writing ? (uint32_t *)(d + o_sid) : nullptr;
        HX_HIP(e, t_begin());
        HX_HIP(e, scan(a, tiles));
        HX_HIP(e, t_end());
        launches++;
        HX_HIP(e, hipMemcpyAsync(cnt.data(), a.cnt, (size_t)nb * G * 4, hipMemcpyDeviceToHost, e->stream));
        if (sc) HX_HIP(e, hipMemcpyAsync(sc_stats, d + o_st, 16, hipMemcpyDeviceToHost, e->stream));   // running totals of this call
        HX_HIP(e, hipStreamSynchronize(e->stream));
        HX_HIP(e, t_add());
        uint64_t pos = 0; bool overflow = false;                 // CSR positions relative to the block's first hit
        for (uint32_t i = 0; i < nb; i++) {
            for (uint32_t gi = 0; gi < G; gi++) {
                const size_t s = (size_t)i * G + gi;
                base[s] = pos; pos += cnt[s]; overflow |= cnt[s] > scap;
            }
            offsets_out[q0 + i + 1] = offsets_out[q0] + pos;
        }
        const uint64_t blk0 = offsets_out[q0], blk_n = pos;
        if (writing && blk0 + blk_n > cap) writing = false;     // capacity exceeded: count the rest
        if (!writing || blk_n == 0) continue;
        HX_HIP(e, hipMemcpyAsync(d_base, base.data(), (size_t)nb * G * 8, hipMemcpyHostToDevice, e->stream));
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
                for (size_t s = 0; s < (size_t)nb * G && !rescan; s++) rescan = cnt[s] > scap && base[s] < w1 && base[s] + cnt[s] > w0;
            uint64_t *okey = need_key ? (uint64_t *)(d + o_okey) : nullptr;
            uint32_t *oid = (uint32_t *)(d + o_oid);
            HX_HIP(e, t_begin());
            hipLaunchKernelGGL(k_range_gather, dim3((uint32_t)std::min<uint64_t>(4096, (nb * (uint64_t)G + 3) / 4)), dim3(256), 0, e->stream,
                               (const uint64_t *)(d + o_skey), (const uint32_t *)(d + o_sid), (const uint32_t *)a.cnt, (const uint64_t *)d_base,
                               (uint64_t)nb * G, scap, w0, w1, okey, oid);
            HX_HIP(e, hipGetLastError());
            launches++;
            if (rescan) {                                        // the overflowed segments' hits in this window, straight to their positions
                RgArgs b = a;
                b.scap = scap; b.seg_base = d_base; b.w0 = w0; b.w1 = w1; b.okey = okey; b.oid = oid;
                HX_HIP(e, scan(b, tiles));
                launches++;
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
            if (sc && rescan) HX_HIP(e, hipMemcpyAsync(sc_stats, d + o_st, 16, hipMemcpyDeviceToHost, e->stream));
            HX_HIP(e, hipStreamSynchronize(e->stream));
            HX_HIP(e, t_add());
            w0 = w1; qa = qb;
        }
    }
    *total_out = offsets_out[nq];
    e->xs_coded += sc_stats[0]; e->xs_fetched += sc_stats[1];
    if (e->timing) {
        e->last_ms = (float)ms;
        e->stat_range.launches += launches; e->stat_range.units += n_pass * nq; e->stat_range.ms += ms;
    }
    if (nomem_sort) return e->fail(HX_E_NOMEM, "one query's hits exceed HX_RANGE_SCRATCH (ordered by distance)");
    if (!count_only && *total_out > cap) return e->fail(HX_E_NOMEM, "capacity exceeded");
    return HX_OK;
}

extern "C" int hx_exact_range(hx_engine *e, int op, int cmp, const double *radius, uint32_t first_query, uint32_t nq, uint64_t first_row, uint64_t n_rows,
                              const uint64_t *row_pass, int order, uint64_t cap, uint64_t *offsets_out, uint32_t *ids_out, double *dist_out, uint64_t *total_out)
{
    return hx_exact_range_src(e, op, cmp, radius, first_query, nq, first_row, n_rows, row_pass, nullptr, order, cap, offsets_out, ids_out, dist_out, total_out);
}
