// hx_rerank.hip -- exact re-rank of per-query candidate lists on the device: the outer `ORDER BY v <op> q LIMIT k` of a query whose
// subquery returned candidate rows (an index scan on a halfvec expression index, re-ranked on the full-precision vector column;
// include/hnswrx.h: hx_exact_rerank).
//
// Values, the order key, the row streaming (ex_park / ex_eval) and the LDS sort are those of hx_exact_core.h, with hx_exact_search's
// lanes-per-row mapping (pitch > 128 ? 64 : 8): each value is bit for bit the one hx_exact_search returns for that (query, row).
//
// A query's list is cut into chunks of CH candidates (a power of two <= 256; smaller when there are too few chunks to fill the chip).
// Pass 1 (k_rerank_chunk): one workgroup per chunk parks the chunk's query in LDS (Q = 1); each wave gathers RIF candidate rows at a time
//   into registers (rp[j] = rows + id * pitch) and evaluates them.  The chunk's (key, id) entries are sorted in LDS and its best
//   min(k, CH) written to scratch.  Every chunk of a query but its last is full, so a query's entries are one contiguous run of scratch.
// Pass 2 (k_rerank_merge): one workgroup per query keeps the k best of that run through an LDS buffer, as k_exact_merge does.
// Windows: the candidates, chunk tables, entries and outputs of a run of consecutive chunks fit HX_EXACT_SCRATCH.  A query whose chunks
// straddle a window boundary carries its running top-k (keys and ids) into the next window, where pass 2 merges it with the new chunks.
#include "hx_exact_core.h"

namespace {

constexpr int RR_MERGE_THREADS = 512;

struct RrArgs {
    const uint8_t *rows, *queries; uint32_t pitch, cap_sp;   // cap_sp: sparsevec record capacity
    uint32_t qslot0;                                          // query slot of the window's query 0
    const uint32_t *cand;                                     // the window's candidate row ids
    const uint32_t *tab;                                      // per chunk: window query, first candidate, candidates (<= CH)
    uint32_t CH, kk;                                          // chunk length; entries kept per chunk = min(k, CH)
    uint64_t *gkey; uint32_t *gid;                            // [chunk][kk]
};

template <class OP, int HOP, int LPR, int RIF>
__global__ void __launch_bounds__(EX_THREADS)
k_rerank_chunk(const RrArgs a)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
    uint8_t *q_lds = lds;
    uint64_t *skey = (uint64_t *)(lds + a.pitch);
    uint32_t *sid = (uint32_t *)(skey + a.CH);
    __shared__ float qn[1];
    constexpr int RPS = 64 / LPR, R = EX_WAVES * RIF * RPS;
    const uint32_t c = blockIdx.x, q = a.tab[3 * c], beg = a.tab[3 * c + 1], n = a.tab[3 * c + 2];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6, sub = lane / LPR, sl = lane % LPR;

    ex_park<OP, HOP, 1>(a.queries, a.qslot0 + q, 1, 0, a.pitch, a.cap_sp, q_lds, qn, [] {});

    const uint32_t *cand = a.cand + beg;
    for (uint32_t b = 0; b < n; b += R) {
        uint32_t pos[RIF], rid[RIF]; bool ok[RIF]; const uint8_t *rp[RIF];
#pragma unroll
        for (int j = 0; j < RIF; j++) {
            pos[j] = b + (wave * RIF + j) * RPS + sub;
            ok[j] = pos[j] < n;
            rid[j] = cand[ok[j] ? pos[j] : 0];                 // slots past the chunk re-read its first row; never kept
            rp[j] = a.rows + (size_t)rid[j] * a.pitch;
        }
        auto put = [&](int, int j, double v) {                 // lanes sl == 0 hold the row's value
            if (sl == 0 && ok[j]) { skey[pos[j]] = ex_key(v); sid[pos[j]] = rid[j]; }
        };
        ex_eval<OP, HOP, LPR, RIF, 1>(q_lds, qn, rp, a.pitch, a.cap_sp, sl, put);
    }
    const uint32_t P = ex_pow2(n);                             // n <= CH, a power of two >= 16
    for (uint32_t i = n + threadIdx.x; i < P; i += blockDim.x) { skey[i] = ~0ull; sid[i] = ~0u; }
    __syncthreads();
    ex_sort(skey, sid, P);
    const uint32_t m = n < a.kk ? n : a.kk;
    for (uint32_t i = threadIdx.x; i < m; i += blockDim.x) { a.gkey[(size_t)c * a.kk + i] = skey[i]; a.gid[(size_t)c * a.kk + i] = sid[i]; }
}

// one workgroup per window query: the k best of its entries gkey/gid[qtab[2q] .. + qtab[2q+1]) and, for query 0, the carry (cn entries)
__global__ void __launch_bounds__(RR_MERGE_THREADS)
k_rerank_merge(const uint64_t *__restrict__ gkey, const uint32_t *__restrict__ gid, const uint32_t *__restrict__ qtab, const uint64_t *__restrict__ ckey,
               const uint32_t *__restrict__ cid, uint32_t cn, uint32_t k, uint32_t cap2, int neg_zero, uint64_t *__restrict__ okey,
               uint32_t *__restrict__ oid, double *__restrict__ odist, uint32_t *__restrict__ ocnt)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
    uint64_t *skey = (uint64_t *)lds;
    uint32_t *sid = (uint32_t *)(skey + cap2);
    __shared__ uint64_t thr_k; __shared__ uint32_t thr_i, cnt;
    const uint32_t q = blockIdx.x, C = cap2 / 2;
    const uint32_t base = qtab[2 * q], nc = q == 0 ? cn : 0, total = nc + qtab[2 * q + 1];
    if (threadIdx.x == 0) { thr_k = ~0ull; thr_i = ~0u; cnt = 0; }
    __syncthreads();
    for (uint32_t p0 = 0; p0 < total; p0 += C) {
        for (uint32_t t = threadIdx.x; t < C && p0 + t < total; t += RR_MERGE_THREADS) {
            const uint32_t p = p0 + t;
            const uint64_t key = p < nc ? ckey[p] : gkey[(size_t)base + p - nc];
            const uint32_t id = p < nc ? cid[p] : gid[(size_t)base + p - nc];
            if (ex_less(key, id, thr_k, thr_i)) { const uint32_t pos = atomicAdd(&cnt, 1u); skey[pos] = key; sid[pos] = id; }
        }
        __syncthreads();
        if (cnt > cap2 - C) ex_keep(skey, sid, cnt, k, &cnt, &thr_k, &thr_i);
        __syncthreads();                                       // every thread has read cnt before the next chunk appends
    }
    if (cnt > 0) ex_keep(skey, sid, cnt, k, &cnt, &thr_k, &thr_i);
    const uint32_t m = cnt;
    for (uint32_t j = threadIdx.x; j < k; j += RR_MERGE_THREADS) {
        const size_t o = (size_t)q * k + j;
        okey[o] = j < m ? skey[j] : ~0ull;
        oid[o] = j < m ? sid[j] : 0xFFFFFFFFu;
        odist[o] = j < m ? ex_val(skey[j], neg_zero != 0) : __builtin_bit_cast(double, 0x7ff8000000000000ull);
    }
    if (threadIdx.x == 0) ocnt[q] = m;
}

template <class OP, int HOP, int LPR, int RIF>
hipError_t rr_launch(hx_engine *e, const RrArgs &a, uint32_t nch)
{
    const size_t lds = (size_t)a.pitch + (size_t)a.CH * 12;
    static thread_local uint64_t attr_devices = 0;            // the attribute is per device: set it on each device this thread launches on
    const uint64_t bit = 1ull << (e->device & 63);
    if (lds > 60 * 1024 && !(attr_devices & bit)) {           // plus the static qn
        hipError_t s = hipFuncSetAttribute((const void *)k_rerank_chunk<OP, HOP, LPR, RIF>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024 - 4096);
        if (s != hipSuccess) return s;
        attr_devices |= bit;
    }
    hipLaunchKernelGGL((k_rerank_chunk<OP, HOP, LPR, RIF>), dim3(nch), dim3(EX_THREADS), lds, e->stream, a);
    return hipGetLastError();
}
// hx_exact_search's lanes per row as a function of the pitch (hx_exact.hip ex_dispatch_lpr): the summation order, hence the value bits
template <class OP, int HOP>
hipError_t rr_dispatch_lpr(hx_engine *e, const RrArgs &a, uint32_t nch)
{
    return a.pitch > 128 ? rr_launch<OP, HOP, 64, 4>(e, a, nch) : rr_launch<OP, HOP, 8, 4>(e, a, nch);
}
template <template <int> class OPT>
hipError_t rr_dispatch_float(hx_engine *e, int op, const RrArgs &a, uint32_t nch)
{
    switch (op) {
    case HX_OP_L2: return rr_dispatch_lpr<OPT<K_L2>, HX_OP_L2>(e, a, nch);
    case HX_OP_NEG_IP: return rr_dispatch_lpr<OPT<K_IP>, HX_OP_NEG_IP>(e, a, nch);
    case HX_OP_COSINE: return rr_dispatch_lpr<OPT<K_IP>, HX_OP_COSINE>(e, a, nch);
    default: return rr_dispatch_lpr<OPT<K_L1>, HX_OP_L1>(e, a, nch);
    }
}
hipError_t rr_scan(hx_engine *e, int op, const RrArgs &a, uint32_t nch)
{
    if (e->dtype == HX_F32) return rr_dispatch_float<OpF32>(e, op, a, nch);
    if (e->dtype == HX_F16) return rr_dispatch_float<OpF16>(e, op, a, nch);
    if (e->dtype == HX_BIT) return op == HX_OP_HAMMING ? rr_dispatch_lpr<OpHamming, HX_OP_HAMMING>(e, a, nch)
                                                       : rr_dispatch_lpr<OpJaccard, HX_OP_JACCARD>(e, a, nch);
    switch (op) {                                             // sparsevec: one lane per (query, row) pair
    case HX_OP_L2: return rr_launch<OpSparse<K_L2>, HX_OP_L2, 1, 1>(e, a, nch);
    case HX_OP_NEG_IP: return rr_launch<OpSparse<K_L2>, HX_OP_NEG_IP, 1, 1>(e, a, nch);
    case HX_OP_COSINE: return rr_launch<OpSparse<K_L2>, HX_OP_COSINE, 1, 1>(e, a, nch);
    default: return rr_launch<OpSparse<K_L2>, HX_OP_L1, 1, 1>(e, a, nch);
    }
}

} // namespace

// =================================================================================================
// C ABI
// =================================================================================================
extern "C" int hx_exact_rerank(hx_engine *e, int op, uint32_t first_query, uint32_t nq, const uint64_t *cand_offsets, const uint32_t *cand_ids,
                               uint32_t k, uint32_t *ids_out, double *dist_out, uint32_t *counts_out)
{
    if (!e) return HX_E_ARG;
    const bool bit = e->dtype == HX_BIT;
    if (op < HX_OP_L2 || op > HX_OP_JACCARD || bit != (op == HX_OP_HAMMING || op == HX_OP_JACCARD))
        return e->fail(HX_E_ARG, "operator is not defined for this column type");
    if (k == 0 || k > HX_EXACT_MAX_K) return e->fail(HX_E_ARG, "k must be in [1, HX_EXACT_MAX_K]");
    if ((uint64_t)first_query + nq > e->n_queries) return e->fail(HX_E_ARG, "query range past the uploaded query slots");
    if (!ids_out || !dist_out || !counts_out) return e->fail(HX_E_ARG, "NULL output");
    if (!cand_offsets) return e->fail(HX_E_ARG, "cand_offsets is NULL");
    if (cand_offsets[0] != 0) return e->fail(HX_E_ARG, "cand_offsets[0] must be 0");
    for (uint32_t i = 0; i < nq; i++)
        if (cand_offsets[i + 1] < cand_offsets[i]) return e->fail(HX_E_ARG, "candidate offsets must be non-decreasing");
    const uint64_t total = cand_offsets[nq];
    if (total && !cand_ids) return e->fail(HX_E_ARG, "cand_ids is NULL");
    for (uint64_t t = 0; t < total; t++)
        if (cand_ids[t] >= e->n_rows) return e->fail(HX_E_ARG, "candidate row id past the stored rows");
    if (nq == 0) return HX_OK;
    HX_HIP(e, hipSetDevice(e->device));

    // chunk length: 256 candidates, halved (down to 16) while the lists give fewer than 2048 chunks
    auto n_chunks = [&](uint32_t ch) { uint64_t c = 0; for (uint32_t i = 0; i < nq; i++) c += (cand_offsets[i + 1] - cand_offsets[i] + ch - 1) / ch; return c; };
    uint32_t CH = 256;
    while (CH > 16 && n_chunks(CH) < 2048) CH >>= 1;
    const uint32_t kk = std::min(k, CH);
    uint32_t cap2 = 1024; while (cap2 < 4 * k) cap2 <<= 1;

    // window bounds from HX_EXACT_SCRATCH (default 256 MiB): half for the chunks (candidates, table, kept entries), half for the queries' outputs
    uint64_t budget = 256ull << 20;
    if (const char *env = getenv("HX_EXACT_SCRATCH")) budget = std::max<uint64_t>(1, strtoull(env, nullptr, 10));
    const uint64_t per_chunk = (uint64_t)CH * 4 + 12 + (uint64_t)kk * 12, per_query = 8 + (uint64_t)k * 20 + 4;
    const uint64_t all_chunks = n_chunks(CH);
    const uint32_t max_ch = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>({budget / 2 / per_chunk, all_chunks, 1u << 22}));
    const uint32_t max_q = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>({budget / 2 / per_query, (uint64_t)nq, 1u << 22}));
    const uint64_t max_cand = std::min<uint64_t>(total, (uint64_t)max_ch * CH);

    const size_t o_tab = al16((size_t)max_cand * 4), o_qtab = o_tab + al16((size_t)max_ch * 12), o_gkey = o_qtab + al16((size_t)max_q * 8);
    const size_t o_gid = o_gkey + al16((size_t)max_ch * kk * 8), o_okey = o_gid + al16((size_t)max_ch * kk * 4);
    const size_t o_oid = o_okey + al16((size_t)max_q * k * 8), o_od = o_oid + al16((size_t)max_q * k * 4), o_oc = o_od + al16((size_t)max_q * k * 8);
    const size_t o_ckey = o_oc + al16((size_t)max_q * 4), o_cid = o_ckey + al16((size_t)k * 8), need = o_cid + al16((size_t)k * 4);
    if (need > e->cap_rerank) {
        if (e->d_rerank) (void)hipFree(e->d_rerank);
        e->d_rerank = nullptr; e->cap_rerank = 0;
        if (hipMalloc((void **)&e->d_rerank, need) != hipSuccess) return e->fail(HX_E_NOMEM, "cannot reserve re-rank scratch in HBM");
        e->cap_rerank = need;
    }
    uint8_t *d = e->d_rerank;
    std::vector<uint32_t> tab, qtab;
    tab.reserve((size_t)max_ch * 3); qtab.reserve((size_t)max_q * 2);

    RrArgs a{};
    a.rows = e->d_rows; a.queries = e->d_queries; a.pitch = (uint32_t)e->pitch; a.cap_sp = (uint32_t)std::min(e->dim, HX_SPARSE_MAX_NNZ);
    a.cand = (const uint32_t *)d; a.tab = (const uint32_t *)(d + o_tab); a.CH = CH; a.kk = kk;
    a.gkey = (uint64_t *)(d + o_gkey); a.gid = (uint32_t *)(d + o_gid);
    uint64_t launches = 0; double ms = 0.0;
    uint32_t qi = 0, cn = 0; uint64_t ci = 0;                 // next query, its next chunk; entries carried into the next window
    while (qi < nq) {
        const uint32_t q0 = qi;
        const uint64_t cand0 = cand_offsets[qi] + ci * CH;
        uint32_t nchw = 0, nqw = 0;
        uint64_t ncand = 0;
        bool split = false;
        tab.clear(); qtab.clear();
        while (qi < nq && nqw < max_q) {
            const uint64_t off = cand_offsets[qi], len = cand_offsets[qi + 1] - off, nch_q = (len + CH - 1) / CH;
            const uint64_t take = std::min<uint64_t>(nch_q - ci, max_ch - nchw);
            if (take == 0 && nch_q > ci) break;                // the window has no room for another chunk
            uint64_t ents = 0;
            for (uint64_t t = 0; t < take; t++) {
                const uint64_t b = (ci + t) * CH, n = std::min<uint64_t>(CH, len - b);
                tab.push_back(nqw); tab.push_back((uint32_t)(off + b - cand0)); tab.push_back((uint32_t)n);
                ents += std::min<uint64_t>(kk, n);
                ncand += n;
            }
            qtab.push_back(nchw * kk); qtab.push_back((uint32_t)ents);
            nchw += (uint32_t)take; nqw++; ci += take;
            if (ci < nch_q) { split = true; break; }           // this query continues in the next window
            qi++; ci = 0;
        }
        if (ncand) HX_HIP(e, hipMemcpyAsync(d, cand_ids + cand0, ncand * 4, hipMemcpyHostToDevice, e->stream));
        if (nchw) HX_HIP(e, hipMemcpyAsync(d + o_tab, tab.data(), tab.size() * 4, hipMemcpyHostToDevice, e->stream));
        HX_HIP(e, hipMemcpyAsync(d + o_qtab, qtab.data(), qtab.size() * 4, hipMemcpyHostToDevice, e->stream));
        if (e->timing) HX_HIP(e, hipEventRecord(e->ev0, e->stream));   // kind 9 = kernel time: the uploads are not in it
        a.qslot0 = first_query + q0;
        if (nchw) { HX_HIP(e, rr_scan(e, op, a, nchw)); launches++; }
        hipLaunchKernelGGL(k_rerank_merge, dim3(nqw), dim3(RR_MERGE_THREADS), (size_t)cap2 * 12, e->stream, a.gkey, a.gid, (const uint32_t *)(d + o_qtab),
                           (const uint64_t *)(d + o_ckey), (const uint32_t *)(d + o_cid), cn, k, cap2, (int)(op == HX_OP_NEG_IP),
                           (uint64_t *)(d + o_okey), (uint32_t *)(d + o_oid), (double *)(d + o_od), (uint32_t *)(d + o_oc));
        HX_HIP(e, hipGetLastError());
        launches++;
        if (e->timing) HX_HIP(e, hipEventRecord(e->ev1, e->stream));
        // a split query's partial list is copied out too; the window that finishes it overwrites it
        HX_HIP(e, hipMemcpyAsync(ids_out + (size_t)q0 * k, d + o_oid, (size_t)nqw * k * 4, hipMemcpyDeviceToHost, e->stream));
        HX_HIP(e, hipMemcpyAsync(dist_out + (size_t)q0 * k, d + o_od, (size_t)nqw * k * 8, hipMemcpyDeviceToHost, e->stream));
        HX_HIP(e, hipMemcpyAsync(counts_out + q0, d + o_oc, (size_t)nqw * 4, hipMemcpyDeviceToHost, e->stream));
        if (split) {
            HX_HIP(e, hipMemcpyAsync(d + o_ckey, d + o_okey + (size_t)(nqw - 1) * k * 8, (size_t)k * 8, hipMemcpyDeviceToDevice, e->stream));
            HX_HIP(e, hipMemcpyAsync(d + o_cid, d + o_oid + (size_t)(nqw - 1) * k * 4, (size_t)k * 4, hipMemcpyDeviceToDevice, e->stream));
        }
        HX_HIP(e, hipStreamSynchronize(e->stream));
        cn = split ? counts_out[q0 + nqw - 1] : 0;
        if (e->timing) { float t = 0.f; HX_HIP(e, hipEventElapsedTime(&t, e->ev0, e->ev1)); ms += t; }
    }
    if (e->timing) {
        e->last_ms = (float)ms;
        e->stat_rerank.launches += launches; e->stat_rerank.units += total; e->stat_rerank.ms += ms;
    }
    return HX_OK;
}
