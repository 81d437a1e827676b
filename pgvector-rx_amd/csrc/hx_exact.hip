// hx_exact.hip -- exact (filtered) k-NN scan on the device: the sequential-scan plan of `SELECT ... ORDER BY v <op> q LIMIT k`,
// i.e. the executor calling the operator function on every heap row and keeping the top k (include/hnswrx.h: hx_exact_search).
//
// Values, the order key, the row streaming (ex_park / ex_eval) and the LDS sort (ex_sort / ex_keep) are those of hx_exact_core.h, shared
// with the range scans and the re-rank.
//
// Order: ascending by the value under PostgreSQL's float8 comparison (-0.0 == +0.0, +inf < NaN, all NaNs equal), ties by ascending row id.
// Each (value, id) is carried as the 64-bit order key (ex_key) and the id.
//
// Pass 1 (k_exact_scan): workgroup (query tile of Q queries, row slice).  The Q queries are parked in LDS; each wave streams RIF row slots
//   at a time (LPR lanes per row, 16-byte fragments, as K1) and evaluates every row fragment against every parked query, one accumulator
//   per (row, query) -- a row is read from HBM once per tile.  Candidates that beat the running k-th entry of their query are appended to
//   that query's buffer (global scratch, `cap` entries); after a round the workgroup sorts any buffer that could overflow in the next round
//   and keeps its k best.  Pass 2 (k_exact_merge): one workgroup per query merges the slices' lists the same way in LDS.
// Sparsevec rows: one lane per (query, row) pair with the merge joins of hx_sparse.hip, feeding the same top-k stage.
// A filter bitmap is compacted into a row-id list on the device first (k_exact_compact); rows that fail it are never read.
//
// <-> on an f32 engine that keeps the 8-bit sidecar (k_exact_scan_sc, query tiles of 1 and 4; hx_exact_sc.h): a round first reads
//   the code rows, skips the rows whose proven lower bound already lies past the query's threshold key, and queues the survivors' ids in LDS;
//   the queue is drained through the same ex_eval + append, so the lists are those of k_exact_scan.  The threshold is the smaller of the
//   workgroup's own k-th key and one key per query shared by all workgroups (atomicMin after every prune), seeded on large inputs by a plain scan
//   of a prefix of the rows.  Any such key is the k-th key of a subset of the query's rows, hence >= the final k-th key: results do not depend on it.
//
// hx_exact_search_filtered (a filter per query): the host groups the queries by filter and plans tiles, slices and query blocks
//   (hx_exact_plan.h); one launch compacts every referenced bitmap (k_exact_compact_g), one scan launch per tile size present runs
//   k_exact_scan's body from a work descriptor per workgroup (k_exact_scan_g), and k_exact_merge_g merges each query's slices.
#include "hx_exact_sc.h"
#include "hx_exact_plan.h"

namespace {

constexpr int EX_MERGE_THREADS = 512;

// one query's candidate buffer in global scratch: sort through LDS, keep the k best
__device__ void ex_prune(uint64_t *gkey, uint32_t *gid, uint32_t stride, uint64_t *skey, uint32_t *sid, uint32_t k, uint32_t *cnt, uint64_t *thr_k, uint32_t *thr_i)
{
    const uint32_t n = *cnt;
    for (uint32_t i = threadIdx.x; i < n; i += blockDim.x) { skey[i] = gkey[(size_t)i * stride]; sid[i] = gid[(size_t)i * stride]; }
    ex_keep(skey, sid, n, k, cnt, thr_k, thr_i);
    const uint32_t m = *cnt;
    for (uint32_t i = threadIdx.x; i < m; i += blockDim.x) { gkey[(size_t)i * stride] = skey[i]; gid[(size_t)i * stride] = sid[i]; }
    __syncthreads();
}

struct ExArgs {
    const uint8_t *rows, *queries; uint32_t pitch, cap_sp;   // cap_sp: sparsevec record capacity
    uint32_t qslot0, nq;                                      // queries of this block: slots qslot0 .. qslot0 + nq - 1
    const uint32_t *ids; uint32_t row0; uint32_t n, per;      // rows: ids[0..n) or row0 + [0..n); slice s = [s * per, (s + 1) * per)
    uint32_t S, k, cap;
    uint64_t *gkey; uint32_t *gid, *gcnt;                     // [query tile][slice][cap][Q], [query][slice]
};

// Q queries x one row slice.  RPS = 64 / LPR rows per wave slot; a round is EX_WAVES * RIF slots.
template <class OP, int HOP, int LPR, int RIF, int Q>
__global__ void __launch_bounds__(EX_THREADS)
k_exact_scan(const ExArgs a)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
    uint8_t *q_lds = lds;
    uint64_t *skey = (uint64_t *)(lds + (size_t)Q * a.pitch);
    uint32_t *sid = (uint32_t *)(skey + a.cap);
    __shared__ uint64_t thr_k[Q];
    __shared__ uint32_t thr_i[Q], cnt[Q];
    __shared__ float qn[Q];
    constexpr int RPS = 64 / LPR, R = EX_WAVES * RIF * RPS;
    const uint32_t tile = blockIdx.x, s = blockIdx.y;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6, sub = lane / LPR, sl = lane % LPR;

    ex_park<OP, HOP, Q>(a.queries, a.qslot0, a.nq, tile, a.pitch, a.cap_sp, q_lds, qn, [&] {   // a partial tile's extra queries: never appended
        if (threadIdx.x < Q) {                                 // a query past the block gets a threshold nothing beats
            const bool live = tile * Q + threadIdx.x < a.nq;
            thr_k[threadIdx.x] = live ? ~0ull : 0ull; thr_i[threadIdx.x] = live ? ~0u : 0u; cnt[threadIdx.x] = 0;
        }
    });

    const uint32_t beg = s * a.per, end = beg + a.per < a.n ? beg + a.per : a.n;
    uint64_t *gkey = a.gkey + ((size_t)tile * a.S + s) * a.cap * Q;      // entry pos of query i at [pos * Q + i]
    uint32_t *gid = a.gid + ((size_t)tile * a.S + s) * a.cap * Q;
    for (uint32_t b = beg; b < end; b += R) {
        uint32_t rid[RIF]; bool ok[RIF]; const uint8_t *rp[RIF];
#pragma unroll
        for (int j = 0; j < RIF; j++) {
            const uint32_t r = b + (wave * RIF + j) * RPS + sub;
            ok[j] = r < end;
            rid[j] = a.ids ? a.ids[ok[j] ? r : beg] : a.row0 + (ok[j] ? r : beg);   // slots past the slice re-read its first row; never appended
            rp[j] = a.rows + (size_t)rid[j] * a.pitch;
        }
        auto append = [&](int i, int j, double v) {            // lanes sl == 0 hold the row's values
            const uint64_t key = ex_key(v);
            if (sl == 0 && ok[j] && ex_less(key, rid[j], thr_k[i], thr_i[i])) {
                const uint32_t pos = atomicAdd(&cnt[i], 1u);
                gkey[pos * Q + i] = key; gid[pos * Q + i] = rid[j];
            }
        };
        ex_eval<OP, HOP, LPR, RIF, Q>(q_lds, qn, rp, a.pitch, a.cap_sp, sl, append);
        __syncthreads();
        for (int i = 0; i < Q; i++)                            // a buffer that the next round could overflow is cut back to k
            if (cnt[i] > a.cap - R) ex_prune(gkey + i, gid + i, Q, skey, sid, a.k, &cnt[i], &thr_k[i], &thr_i[i]);
        __syncthreads();                                       // every thread has read the counts before the next round appends
    }
    for (int i = 0; i < Q; i++) {
        if (tile * Q + i >= a.nq) break;
        if (cnt[i] > a.k) ex_prune(gkey + i, gid + i, Q, skey, sid, a.k, &cnt[i], &thr_k[i], &thr_i[i]);
        if (threadIdx.x == 0) a.gcnt[(size_t)(tile * Q + i) * a.S + s] = cnt[i];
    }
}

// The sidecar variant for <-> on f32 rows (64 lanes per row).  A round is EX_WAVES * SC_NB wave steps of SC_ROWS code rows; survivors wait in
// sq[] until a batch of EX_WAVES * RIF is there (or the slice ends) and are then evaluated and appended exactly as in k_exact_scan.
constexpr int SC_NB = 2, SC_RR = EX_WAVES * SC_NB * SC_ROWS;
template <class OP, int HOP, int RIF, int Q>
__global__ void __launch_bounds__(EX_THREADS)
k_exact_scan_sc(const ExArgs a, const ScArgs c)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
    uint8_t *q_lds = lds;
    uint64_t *skey = (uint64_t *)(lds + (size_t)Q * a.pitch);
    uint32_t *sid = (uint32_t *)(skey + a.cap);
    constexpr int BATCH = EX_WAVES * RIF;
    __shared__ uint64_t thr_k[Q], T[Q];
    __shared__ uint32_t thr_i[Q], cnt[Q], sq[SC_RR + BATCH], sq_n;
    __shared__ float qn[Q];
    const uint32_t tile = blockIdx.x, s = blockIdx.y;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6, g = lane >> 4;
    uint32_t live = 0;
#pragma unroll
    for (int i = 0; i < Q; i++) live |= (tile * Q + i < a.nq ? 1u : 0u) << i;

    ex_park<OP, HOP, Q>(a.queries, a.qslot0, a.nq, tile, a.pitch, a.cap_sp, q_lds, qn, [&] {
        if (threadIdx.x < Q) {
            const bool lv = (live >> threadIdx.x) & 1u;
            thr_k[threadIdx.x] = lv ? ~0ull : 0ull; thr_i[threadIdx.x] = lv ? ~0u : 0u; cnt[threadIdx.x] = 0;
            T[threadIdx.x] = lv ? __hip_atomic_load(&c.shared[tile * Q + threadIdx.x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0ull;
        }
        if (threadIdx.x == 0) sq_n = 0;
    });

    const uint32_t beg = s * a.per, end = beg + a.per < a.n ? beg + a.per : a.n;
    uint64_t *gkey = a.gkey + ((size_t)tile * a.S + s) * a.cap * Q;
    uint32_t *gid = a.gid + ((size_t)tile * a.S + s) * a.cap * Q;
    uint32_t fetched = 0;                                      // thread 0's count of drained rows
    for (uint32_t b = beg; b < end; b += SC_RR) {
        for (int nb = 0; nb < SC_NB; nb++) {
            const uint32_t b0 = b + (wave * SC_NB + nb) * SC_ROWS;
            if (b0 >= end) break;                              // wave-uniform
            uint32_t rid[SC_P];
#pragma unroll
            for (int p = 0; p < SC_P; p++) {
                const uint32_t r = b0 + 4u * p + g;
                rid[p] = a.ids ? a.ids[r < end ? r : beg] : a.row0 + (r < end ? r : beg);   // slots past the slice re-read its first row; never kept
            }
            const uint32_t m = sc_survivors<Q>(c, q_lds, rid, end - b0 < (uint32_t)SC_ROWS ? end - b0 : (uint32_t)SC_ROWS, T, live, lane);
            if (m) {
                uint32_t base = 0;
                if (lane == 0) base = atomicAdd(&sq_n, (uint32_t)__popc(m));
                base = __shfl(base, 0, 64);
                if (lane < (uint32_t)SC_ROWS && ((m >> lane) & 1u))
                    sq[base + __popc(m & ((1u << lane) - 1u))] = a.ids ? a.ids[b0 + lane] : a.row0 + b0 + lane;
            }
        }
        __syncthreads();
        const uint32_t n = sq_n;
        if (n >= (uint32_t)BATCH || (b + SC_RR >= end && n > 0)) {
            for (uint32_t o = 0; o < n; o += BATCH) {
                uint32_t rid[RIF]; bool ok[RIF]; const uint8_t *rp[RIF];
#pragma unroll
                for (int j = 0; j < RIF; j++) {
                    const uint32_t x = o + wave * RIF + j;
                    ok[j] = x < n;
                    rid[j] = sq[ok[j] ? x : 0];                // slots past the queue re-read its first row; never appended
                    rp[j] = a.rows + (size_t)rid[j] * a.pitch;
                }
                auto append = [&](int i, int j, double v) {
                    const uint64_t key = ex_key(v);
                    if (lane == 0 && ok[j] && ex_less(key, rid[j], thr_k[i], thr_i[i])) {
                        const uint32_t pos = atomicAdd(&cnt[i], 1u);
                        gkey[pos * Q + i] = key; gid[pos * Q + i] = rid[j];
                    }
                };
                ex_eval<OP, HOP, 64, RIF, Q>(q_lds, qn, rp, a.pitch, a.cap_sp, lane, append);
                __syncthreads();
                for (int i = 0; i < Q; i++)
                    if (cnt[i] > a.cap - BATCH) {
                        ex_prune(gkey + i, gid + i, Q, skey, sid, a.k, &cnt[i], &thr_k[i], &thr_i[i]);
                        if (threadIdx.x == 0) atomicMin((unsigned long long *)&c.shared[tile * Q + i], (unsigned long long)thr_k[i]);   // ~0 until k entries
                    }
                __syncthreads();
            }
            if (threadIdx.x == 0) { fetched += n; sq_n = 0; }
        }
        if (threadIdx.x < Q && ((live >> threadIdx.x) & 1u)) {
            const uint64_t sh = __hip_atomic_load(&c.shared[tile * Q + threadIdx.x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            T[threadIdx.x] = sh < thr_k[threadIdx.x] ? sh : thr_k[threadIdx.x];
        }
        __syncthreads();
    }
    for (int i = 0; i < Q; i++) {
        if (tile * Q + i >= a.nq) break;
        if (cnt[i] > a.k) ex_prune(gkey + i, gid + i, Q, skey, sid, a.k, &cnt[i], &thr_k[i], &thr_i[i]);
        if (threadIdx.x == 0) {
            a.gcnt[(size_t)(tile * Q + i) * a.S + s] = cnt[i];
            atomicMin((unsigned long long *)&c.shared[tile * Q + i], (unsigned long long)thr_k[i]);
        }
    }
    if (threadIdx.x == 0) { atomicAdd(c.stats, (unsigned long long)(end - beg)); atomicAdd(c.stats + 1, (unsigned long long)fetched); }
}

// the seed of the shared thresholds: the k-th key of a finished top-k (of a prefix of the rows), where that has k entries
__global__ void k_exact_seed(const uint32_t *__restrict__ cnt, const double *__restrict__ dist, uint32_t k, uint32_t nq, uint64_t *__restrict__ shared)
{
    const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q < nq && cnt[q] == k) shared[q] = ex_key(dist[(size_t)q * k + k - 1]);
}

// one workgroup per query: the S slice lists (each <= k entries, at stride cap) in chunks of cap2 / 2 positions through an LDS buffer
__global__ void __launch_bounds__(EX_MERGE_THREADS)
k_exact_merge(const uint64_t *__restrict__ gkey, const uint32_t *__restrict__ gid, const uint32_t *__restrict__ gcnt, uint32_t S, uint32_t cap, uint32_t Q,
              uint32_t k, uint32_t cap2, int neg_zero, uint32_t *__restrict__ ids_out, double *__restrict__ dist_out, uint32_t *__restrict__ cnt_out)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
    uint64_t *skey = (uint64_t *)lds;
    uint32_t *sid = (uint32_t *)(skey + cap2);
    __shared__ uint64_t thr_k; __shared__ uint32_t thr_i, cnt;
    const uint32_t q = blockIdx.x, C = cap2 / 2;
    if (threadIdx.x == 0) { thr_k = ~0ull; thr_i = ~0u; cnt = 0; }
    __syncthreads();
    const uint64_t total = (uint64_t)S * k;
    for (uint64_t p0 = 0; p0 < total; p0 += C) {
        for (uint32_t t = threadIdx.x; t < C && p0 + t < total; t += EX_MERGE_THREADS) {
            const uint32_t s = (uint32_t)((p0 + t) / k), i = (uint32_t)((p0 + t) % k);
            if (i >= gcnt[(size_t)q * S + s]) continue;
            const size_t o = (((size_t)(q / Q) * S + s) * cap + i) * Q + q % Q;
            const uint64_t key = gkey[o]; const uint32_t id = gid[o];
            if (ex_less(key, id, thr_k, thr_i)) { const uint32_t pos = atomicAdd(&cnt, 1u); skey[pos] = key; sid[pos] = id; }
        }
        __syncthreads();
        if (cnt > cap2 - C) ex_keep(skey, sid, cnt, k, &cnt, &thr_k, &thr_i);
        __syncthreads();                                       // every thread has read cnt before the next chunk appends
    }
    if (cnt > 0) ex_keep(skey, sid, cnt, k, &cnt, &thr_k, &thr_i);
    const uint32_t m = cnt;
    for (uint32_t j = threadIdx.x; j < k; j += EX_MERGE_THREADS) {
        ids_out[(size_t)q * k + j] = j < m ? sid[j] : 0xFFFFFFFFu;
        dist_out[(size_t)q * k + j] = j < m ? ex_val(skey[j], neg_zero != 0) : __builtin_bit_cast(double, 0x7ff8000000000000ull);
    }
    if (threadIdx.x == 0) cnt_out[q] = m;
}

// filter bitmap -> row-id list (order free: the top-k order includes the id)
__global__ void k_exact_compact(const uint64_t *__restrict__ words, uint64_t n_words, uint64_t n_rows, uint32_t row0, uint32_t *__restrict__ out, uint32_t *__restrict__ ctr)
{
    const uint64_t w = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= n_words) return;
    uint64_t bits = words[w];
    if (w == n_words - 1 && (n_rows & 63)) bits &= (1ull << (n_rows & 63)) - 1;
    if (!bits) return;
    uint32_t pos = atomicAdd(ctr, (uint32_t)__popcll(bits));
    while (bits) { const int b = __builtin_ctzll(bits); out[pos++] = row0 + (uint32_t)(w * 64 + b); bits &= bits - 1; }
}

constexpr uint32_t EX_SEED_ROWS = 16384;                      // prefix of the rows whose top k seeds the sidecar path's shared thresholds

template <class OP, int HOP, int LPR, int RIF, int Q>
hipError_t ex_launch_scan(hx_engine *e, const ExArgs &a, uint32_t tiles)
{
    const size_t lds = (size_t)Q * a.pitch + (size_t)a.cap * 12;
    static thread_local uint64_t attr_devices = 0;            // the attribute is per device: set it on each device this thread launches on
    const uint64_t bit = 1ull << (e->device & 63);
    if (lds > 65536 && !(attr_devices & bit)) {
        hipError_t s = hipFuncSetAttribute((const void *)k_exact_scan<OP, HOP, LPR, RIF, Q>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024 - 4096);
        if (s != hipSuccess) return s;
        attr_devices |= bit;
    }
    hipLaunchKernelGGL((k_exact_scan<OP, HOP, LPR, RIF, Q>), dim3(tiles, a.S), dim3(EX_THREADS), lds, e->stream, a);
    return hipGetLastError();
}

template <int RIF, int Q>
hipError_t ex_launch_scan_sc(hx_engine *e, const ExArgs &a, const ScArgs &c, uint32_t tiles)
{
    const size_t lds = (size_t)Q * a.pitch + (size_t)a.cap * 12;
    static thread_local uint64_t attr_devices = 0;
    const uint64_t bit = 1ull << (e->device & 63);
    if (lds > 60 * 1024 && !(attr_devices & bit)) {
        hipError_t s = hipFuncSetAttribute((const void *)k_exact_scan_sc<OpF32<K_L2>, HX_OP_L2, RIF, Q>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024 - 4096);
        if (s != hipSuccess) return s;
        attr_devices |= bit;
    }
    hipLaunchKernelGGL((k_exact_scan_sc<OpF32<K_L2>, HX_OP_L2, RIF, Q>), dim3(tiles, a.S), dim3(EX_THREADS), lds, e->stream, a, c);
    return hipGetLastError();
}

// rows per round of a workgroup for (LPR, RIF): EX_WAVES * RIF * 64 / LPR
template <class OP, int HOP, int LPR>
hipError_t ex_dispatch_q(hx_engine *e, const ExArgs &a, uint32_t Q, uint32_t tiles)
{
    if (Q == 16) return ex_launch_scan<OP, HOP, LPR, 2, 16>(e, a, tiles);
    if (Q == 4) return ex_launch_scan<OP, HOP, LPR, 4, 4>(e, a, tiles);
    return ex_launch_scan<OP, HOP, LPR, 4, 1>(e, a, tiles);
}
template <class OP, int HOP>
hipError_t ex_dispatch_lpr(hx_engine *e, const ExArgs &a, uint32_t Q, uint32_t tiles)
{
    return a.pitch > 128 ? ex_dispatch_q<OP, HOP, 64>(e, a, Q, tiles) : ex_dispatch_q<OP, HOP, 8>(e, a, Q, tiles);
}
template <template <int> class OPT>
hipError_t ex_dispatch_float(hx_engine *e, int op, const ExArgs &a, uint32_t Q, uint32_t tiles)
{
    switch (op) {
    case HX_OP_L2: return ex_dispatch_lpr<OPT<K_L2>, HX_OP_L2>(e, a, Q, tiles);
    case HX_OP_NEG_IP: return ex_dispatch_lpr<OPT<K_IP>, HX_OP_NEG_IP>(e, a, Q, tiles);
    case HX_OP_COSINE: return ex_dispatch_lpr<OPT<K_IP>, HX_OP_COSINE>(e, a, Q, tiles);
    default: return ex_dispatch_lpr<OPT<K_L1>, HX_OP_L1>(e, a, Q, tiles);
    }
}
template <int HOP>
hipError_t ex_launch_sparse(hx_engine *e, const ExArgs &a, uint32_t tiles)
{
    hipLaunchKernelGGL((k_exact_scan<OpSparse<K_L2>, HOP, 1, 1, 1>), dim3(tiles, a.S), dim3(EX_THREADS), (size_t)a.pitch + (size_t)a.cap * 12, e->stream, a);
    return hipGetLastError();
}

hipError_t ex_scan(hx_engine *e, int op, const ExArgs &a, uint32_t Q, uint32_t tiles)
{
    if (e->dtype == HX_F32) return ex_dispatch_float<OpF32>(e, op, a, Q, tiles);
    if (e->dtype == HX_F16) return ex_dispatch_float<OpF16>(e, op, a, Q, tiles);
    if (e->dtype == HX_BIT) return op == HX_OP_HAMMING ? ex_dispatch_lpr<OpHamming, HX_OP_HAMMING>(e, a, Q, tiles)
                                                       : ex_dispatch_lpr<OpJaccard, HX_OP_JACCARD>(e, a, Q, tiles);
    switch (op) {
    case HX_OP_L2: return ex_launch_sparse<HX_OP_L2>(e, a, tiles);
    case HX_OP_NEG_IP: return ex_launch_sparse<HX_OP_NEG_IP>(e, a, tiles);
    case HX_OP_COSINE: return ex_launch_sparse<HX_OP_COSINE>(e, a, tiles);
    default: return ex_launch_sparse<HX_OP_L1>(e, a, tiles);
    }
}

// ---- per-query filters (hx_exact_search_filtered): the same scan and merge, driven by the descriptors of hx_exact_plan.h ----------------------
struct ExGArgs {
    const uint8_t *rows, *queries; uint32_t pitch, cap_sp;
    const uint32_t *ids; uint32_t row0, k, cap;               // ids: the id lists of all referenced filters; cap: of this launch's tile size
    uint64_t *gkey; uint32_t *gid, *gcnt;                     // the block's scratch; places from the descriptors
    const ExWg *wg;                                           // one per workgroup of this launch
    const uint32_t *slots;                                    // query slot by grouped position
};

// k_exact_scan with its tile, slice, row list and buffers read from wg[blockIdx.x]: a uniform address, loaded once into scalar registers
template <class OP, int HOP, int LPR, int RIF, int Q>
__global__ void __launch_bounds__(EX_THREADS)
k_exact_scan_g(const ExGArgs a)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
    uint8_t *q_lds = lds;
    uint64_t *skey = (uint64_t *)(lds + (size_t)Q * a.pitch);
    uint32_t *sid = (uint32_t *)(skey + a.cap);
    __shared__ uint64_t thr_k[Q];
    __shared__ uint32_t thr_i[Q], cnt[Q];
    __shared__ float qn[Q];
    constexpr int RPS = 64 / LPR, R = EX_WAVES * RIF * RPS;
    const ExWg &w = a.wg[blockIdx.x];
    const ExWg d{ex_uni(w.ids), ex_uni(w.buf), ex_uni(w.beg), ex_uni(w.end), ex_uni(w.qpos), ex_uni(w.nlive), ex_uni(w.cnt), ex_uni(w.S)};
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6, sub = lane / LPR, sl = lane % LPR;

    ex_park_slots<OP, HOP, Q>(a.queries, a.slots + d.qpos, d.nlive, a.pitch, a.cap_sp, q_lds, qn, [&] {   // a partial tile's extra queries: never appended
        if (threadIdx.x < Q) {
            const bool live = threadIdx.x < d.nlive;
            thr_k[threadIdx.x] = live ? ~0ull : 0ull; thr_i[threadIdx.x] = live ? ~0u : 0u; cnt[threadIdx.x] = 0;
        }
    });

    const uint32_t beg = d.beg, end = d.end;
    const uint32_t *ids = d.ids != EX_NO_IDS ? a.ids + d.ids : nullptr;
    uint64_t *gkey = a.gkey + d.buf;                          // entry pos of query i at [pos * Q + i]
    uint32_t *gid = a.gid + d.buf;
    for (uint32_t b = beg; b < end; b += R) {
        uint32_t rid[RIF]; bool ok[RIF]; const uint8_t *rp[RIF];
#pragma unroll
        for (int j = 0; j < RIF; j++) {
            const uint32_t r = b + (wave * RIF + j) * RPS + sub;
            ok[j] = r < end;
            rid[j] = ids ? ids[ok[j] ? r : beg] : a.row0 + (ok[j] ? r : beg);   // slots past the slice re-read its first row; never appended
            rp[j] = a.rows + (size_t)rid[j] * a.pitch;
        }
        auto append = [&](int i, int j, double v) {            // lanes sl == 0 hold the row's values
            const uint64_t key = ex_key(v);
            if (sl == 0 && ok[j] && ex_less(key, rid[j], thr_k[i], thr_i[i])) {
                const uint32_t pos = atomicAdd(&cnt[i], 1u);
                gkey[pos * Q + i] = key; gid[pos * Q + i] = rid[j];
            }
        };
        ex_eval<OP, HOP, LPR, RIF, Q>(q_lds, qn, rp, a.pitch, a.cap_sp, sl, append);
        __syncthreads();
        for (int i = 0; i < Q; i++)                            // a buffer that the next round could overflow is cut back to k
            if (cnt[i] > a.cap - R) ex_prune(gkey + i, gid + i, Q, skey, sid, a.k, &cnt[i], &thr_k[i], &thr_i[i]);
        __syncthreads();                                       // every thread has read the counts before the next round appends
    }
    for (int i = 0; i < Q; i++) {
        if ((uint32_t)i >= d.nlive) break;
        if (cnt[i] > a.k) ex_prune(gkey + i, gid + i, Q, skey, sid, a.k, &cnt[i], &thr_k[i], &thr_i[i]);
        if (threadIdx.x == 0) a.gcnt[d.cnt + (uint32_t)i * d.S] = cnt[i];
    }
}

// k_exact_merge with the query's slice count and buffers from mq[blockIdx.x]; outputs by grouped position
__global__ void __launch_bounds__(EX_MERGE_THREADS)
k_exact_merge_g(const uint64_t *__restrict__ gkey, const uint32_t *__restrict__ gid, const uint32_t *__restrict__ gcnt, const ExMq *__restrict__ mq,
                uint32_t k, uint32_t cap2, int neg_zero, uint32_t *__restrict__ ids_out, double *__restrict__ dist_out, uint32_t *__restrict__ cnt_out)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
    uint64_t *skey = (uint64_t *)lds;
    uint32_t *sid = (uint32_t *)(skey + cap2);
    __shared__ uint64_t thr_k; __shared__ uint32_t thr_i, cnt;
    const uint32_t q = blockIdx.x, C = cap2 / 2;
    const ExMq m = mq[q];
    if (threadIdx.x == 0) { thr_k = ~0ull; thr_i = ~0u; cnt = 0; }
    __syncthreads();
    const uint64_t total = (uint64_t)m.S * k;
    for (uint64_t p0 = 0; p0 < total; p0 += C) {
        for (uint32_t t = threadIdx.x; t < C && p0 + t < total; t += EX_MERGE_THREADS) {
            const uint32_t s = (uint32_t)((p0 + t) / k), i = (uint32_t)((p0 + t) % k);
            if (i >= gcnt[m.cnt + s]) continue;
            const size_t o = m.buf + ((size_t)s * m.cap + i) * m.Q;
            const uint64_t key = gkey[o]; const uint32_t id = gid[o];
            if (ex_less(key, id, thr_k, thr_i)) { const uint32_t pos = atomicAdd(&cnt, 1u); skey[pos] = key; sid[pos] = id; }
        }
        __syncthreads();
        if (cnt > cap2 - C) ex_keep(skey, sid, cnt, k, &cnt, &thr_k, &thr_i);
        __syncthreads();                                       // every thread has read cnt before the next chunk appends
    }
    if (cnt > 0) ex_keep(skey, sid, cnt, k, &cnt, &thr_k, &thr_i);
    const uint32_t n = cnt;
    for (uint32_t j = threadIdx.x; j < k; j += EX_MERGE_THREADS) {
        ids_out[(size_t)q * k + j] = j < n ? sid[j] : 0xFFFFFFFFu;
        dist_out[(size_t)q * k + j] = j < n ? ex_val(skey[j], neg_zero != 0) : __builtin_bit_cast(double, 0x7ff8000000000000ull);
    }
    if (threadIdx.x == 0) cnt_out[q] = n;
}

// k_exact_compact for several bitmaps in one launch: bitmap blockIdx.y (n_words words each, one after the other) -> the list at out + base[y]
struct ExCompactBases { uint64_t base[HX_EXACT_MAX_FILTERS]; };
__global__ void k_exact_compact_g(const uint64_t *__restrict__ words, uint64_t n_words, uint64_t n_rows, uint32_t row0, uint32_t *__restrict__ out,
                                  uint32_t *__restrict__ ctr, const ExCompactBases b)
{
    const uint64_t w = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= n_words) return;
    uint64_t bits = words[(uint64_t)blockIdx.y * n_words + w];
    if (w == n_words - 1 && (n_rows & 63)) bits &= (1ull << (n_rows & 63)) - 1;
    if (!bits) return;
    uint32_t *list = out + b.base[blockIdx.y];
    uint32_t pos = atomicAdd(ctr + blockIdx.y, (uint32_t)__popcll(bits));
    while (bits) { const int bi = __builtin_ctzll(bits); list[pos++] = row0 + (uint32_t)(w * 64 + bi); bits &= bits - 1; }
}

template <class OP, int HOP, int LPR, int RIF, int Q>
hipError_t exg_launch(hx_engine *e, const ExGArgs &a, uint32_t n_wg)
{
    const size_t lds = (size_t)Q * a.pitch + (size_t)a.cap * 12;
    static thread_local uint64_t attr_devices = 0;            // the attribute is per device: set it on each device this thread launches on
    const uint64_t bit = 1ull << (e->device & 63);
    if (lds > 65536 && !(attr_devices & bit)) {
        hipError_t s = hipFuncSetAttribute((const void *)k_exact_scan_g<OP, HOP, LPR, RIF, Q>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024 - 4096);
        if (s != hipSuccess) return s;
        attr_devices |= bit;
    }
    hipLaunchKernelGGL((k_exact_scan_g<OP, HOP, LPR, RIF, Q>), dim3(n_wg), dim3(EX_THREADS), lds, e->stream, a);
    return hipGetLastError();
}
// the (LPR, RIF) of a tile size are those of ex_dispatch_q / ex_dispatch_lpr
template <class OP, int HOP>
hipError_t exg_dispatch_q(hx_engine *e, const ExGArgs &a, uint32_t Q, uint32_t n_wg)
{
    if (a.pitch > 128) {
        if (Q == 16) return exg_launch<OP, HOP, 64, 2, 16>(e, a, n_wg);
        if (Q == 4) return exg_launch<OP, HOP, 64, 4, 4>(e, a, n_wg);
        return exg_launch<OP, HOP, 64, 4, 1>(e, a, n_wg);
    }
    if (Q == 16) return exg_launch<OP, HOP, 8, 2, 16>(e, a, n_wg);
    if (Q == 4) return exg_launch<OP, HOP, 8, 4, 4>(e, a, n_wg);
    return exg_launch<OP, HOP, 8, 4, 1>(e, a, n_wg);
}
template <template <int> class OPT>
hipError_t exg_dispatch_float(hx_engine *e, int op, const ExGArgs &a, uint32_t Q, uint32_t n_wg)
{
    switch (op) {
    case HX_OP_L2: return exg_dispatch_q<OPT<K_L2>, HX_OP_L2>(e, a, Q, n_wg);
    case HX_OP_NEG_IP: return exg_dispatch_q<OPT<K_IP>, HX_OP_NEG_IP>(e, a, Q, n_wg);
    case HX_OP_COSINE: return exg_dispatch_q<OPT<K_IP>, HX_OP_COSINE>(e, a, Q, n_wg);
    default: return exg_dispatch_q<OPT<K_L1>, HX_OP_L1>(e, a, Q, n_wg);
    }
}
hipError_t exg_scan(hx_engine *e, int op, const ExGArgs &a, uint32_t Q, uint32_t n_wg)
{
    if (e->dtype == HX_F32) return exg_dispatch_float<OpF32>(e, op, a, Q, n_wg);
    if (e->dtype == HX_F16) return exg_dispatch_float<OpF16>(e, op, a, Q, n_wg);
    if (e->dtype == HX_BIT) return op == HX_OP_HAMMING ? exg_dispatch_q<OpHamming, HX_OP_HAMMING>(e, a, Q, n_wg)
                                                       : exg_dispatch_q<OpJaccard, HX_OP_JACCARD>(e, a, Q, n_wg);
    switch (op) {
    case HX_OP_L2: return exg_launch<OpSparse<K_L2>, HX_OP_L2, 1, 1, 1>(e, a, n_wg);
    case HX_OP_NEG_IP: return exg_launch<OpSparse<K_L2>, HX_OP_NEG_IP, 1, 1, 1>(e, a, n_wg);
    case HX_OP_COSINE: return exg_launch<OpSparse<K_L2>, HX_OP_COSINE, 1, 1, 1>(e, a, n_wg);
    default: return exg_launch<OpSparse<K_L2>, HX_OP_L1, 1, 1, 1>(e, a, n_wg);
    }
}

// hx_exact_search with its filter source chosen: a host bitmap (row_pass: popcounted, uploaded and compacted here), an id list already on the
// device (list: a filter set's; it stands where the compacted bitmap stands, and nothing is uploaded or compacted), or neither
int ex_search(hx_engine *e, int op, uint32_t first_query, uint32_t nq, uint64_t first_row, uint64_t n_rows, const uint64_t *row_pass, const HxIdList *list,
              uint32_t k, uint32_t *ids_out, double *dist_out, uint32_t *counts_out)
{
    const bool bit = e->dtype == HX_BIT;
    if (op < HX_OP_L2 || op > HX_OP_JACCARD || bit != (op == HX_OP_HAMMING || op == HX_OP_JACCARD))
        return e->fail(HX_E_ARG, "operator is not defined for this column type");
    if (k == 0 || k > HX_EXACT_MAX_K) return e->fail(HX_E_ARG, "k must be in [1, HX_EXACT_MAX_K]");
    if (first_row > e->n_rows || n_rows > e->n_rows - first_row) return e->fail(HX_E_ARG, "row range past the stored rows");
    if (first_row + n_rows > 0xFFFFFFFFull) return e->fail(HX_E_ARG, "row range past 2^32 - 1");
    if ((uint64_t)first_query + nq > e->n_queries) return e->fail(HX_E_ARG, "query range past the uploaded query slots");
    if (!ids_out || !dist_out || !counts_out) return e->fail(HX_E_ARG, "NULL output");
    if (nq == 0) return HX_OK;

    const uint64_t n_words = (n_rows + 63) / 64;
    uint64_t n_pass = list ? list->n : n_rows;
    if (row_pass) {
        n_pass = 0;
        for (uint64_t w = 0; w < n_words; w++) {
            uint64_t b = row_pass[w];
            if (w == n_words - 1 && (n_rows & 63)) b &= (1ull << (n_rows & 63)) - 1;
            n_pass += (uint64_t)__builtin_popcountll(b);
        }
    }
    if (n_pass == 0) {
        for (size_t i = 0; i < (size_t)nq * k; i++) { ids_out[i] = 0xFFFFFFFFu; dist_out[i] = std::nan(""); }
        memset(counts_out, 0, nq * sizeof(uint32_t));
        return HX_OK;
    }
    HX_HIP(e, hipSetDevice(e->device));

    // plan (hx_exact_plan.h: ex_plan_plain): query tile Q, rows per round R, per-(query, slice) buffer cap, slices S, queries per block.
    // The top-k scratch is bounded by HX_EXACT_SCRATCH bytes (default 256 MiB).
    // A filtered call also holds its bitmap (n_rows / 8 B) and the compacted id list (4 B per passing row) on the device.
    const uint32_t pitch = (uint32_t)e->pitch;
    uint64_t budget = 256ull << 20;
    if (const char *env = getenv("HX_EXACT_SCRATCH")) budget = std::max<uint64_t>(1, strtoull(env, nullptr, 10));
    const ExPlan p = ex_plan_plain(nq, pitch, e->dtype == HX_SPARSE, n_pass, k, budget);

    const size_t ids_bytes = row_pass ? al16((size_t)n_pass * 4) : 0, words_bytes = row_pass ? al16((size_t)n_words * 8) : 0;
    const size_t o_words = ids_bytes, o_ctr = o_words + words_bytes, o_key = o_ctr + 16;
    const size_t nq_pad = (size_t)(p.nqb + p.Q - 1) / p.Q * p.Q;            // the buffers are laid out by whole query tiles
    const size_t o_id = o_key + al16(nq_pad * p.S * p.cap * 8), o_cnt = o_id + al16(nq_pad * p.S * p.cap * 4);
    const size_t o_oid = o_cnt + al16((size_t)p.nqb * p.S * 4), o_od = o_oid + al16((size_t)p.nqb * k * 4), o_oc = o_od + al16((size_t)p.nqb * k * 8);
    // the sidecar path (<-> on an engine with a sidecar, query tiles of 1 and 4): 8 B per query for the shared threshold key, and two counters
    const bool sc = op == HX_OP_L2 && e->d_sc_codes && p.Q <= 4 && sc_enabled(n_pass, SC_MIN_ROWS_TOPK);
    const size_t o_sh = o_oc + al16((size_t)p.nqb * 4), o_st = o_sh + (sc ? al16(nq_pad * 8) : 0);
    const size_t need = o_st + (sc ? 16 : 0);
    if (need > e->cap_exact) {
        if (e->d_exact) (void)hipFree(e->d_exact);
        e->d_exact = nullptr; e->cap_exact = 0;
        if (hipMalloc((void **)&e->d_exact, need) != hipSuccess) return e->fail(HX_E_NOMEM, "cannot reserve exact-scan scratch in HBM");
        e->cap_exact = need;
    }
    uint8_t *d = e->d_exact;
    const uint32_t *d_ids = row_pass ? (const uint32_t *)d : list ? list->d : nullptr;
    uint64_t launches = 0; double ms = 0.0;
    if (row_pass) {
        HX_HIP(e, hipMemsetAsync(d + o_ctr, 0, 4, e->stream));
        HX_HIP(e, hipMemcpyAsync(d + o_words, row_pass, n_words * 8, hipMemcpyHostToDevice, e->stream));
    }
    if (e->timing) HX_HIP(e, hipEventRecord(e->ev0, e->stream));   // kind 7 = kernel time: the bitmap upload is not in it
    if (row_pass) {
        hipLaunchKernelGGL(k_exact_compact, dim3((uint32_t)((n_words + 255) / 256)), dim3(256), 0, e->stream,
                           (const uint64_t *)(d + o_words), n_words, n_rows, (uint32_t)first_row, (uint32_t *)d, (uint32_t *)(d + o_ctr));
        HX_HIP(e, hipGetLastError());
        launches++;
    }
    ExArgs a{};
    a.rows = e->d_rows; a.queries = e->d_queries; a.pitch = pitch; a.cap_sp = (uint32_t)std::min(e->dim, HX_SPARSE_MAX_NNZ);
    a.ids = d_ids; a.row0 = (uint32_t)first_row; a.n = (uint32_t)n_pass; a.per = p.per; a.S = p.S; a.k = k; a.cap = p.cap;
    a.gkey = (uint64_t *)(d + o_key); a.gid = (uint32_t *)(d + o_id); a.gcnt = (uint32_t *)(d + o_cnt);
    ScArgs c{};
    unsigned long long sc_stats[2] = {0, 0}; uint64_t seed_rows = 0;
    // seed: large inputs first take the top k of a prefix with the plain kernel (no threshold is known yet, so every row of it would be fetched
    // anyway); its k-th key starts the shared thresholds, so the main scan skips from its first round on
    const uint32_t n_seed = sc && n_pass >= SC_MIN_ROWS_TOPK && k <= EX_SEED_ROWS / 8 ? EX_SEED_ROWS : 0;
    if (sc) {
        c.codes = e->d_sc_codes; c.meta = e->d_sc_meta; c.cpitch = e->sc_pitch; c.dim = (uint32_t)e->dim; c.nterm = pitch >> 2;
        c.shared = (uint64_t *)(d + o_sh); c.stats = (unsigned long long *)(d + o_st);
        HX_HIP(e, hipMemsetAsync(d + o_st, 0, 16, e->stream));
    }
    for (uint32_t q0 = 0; q0 < nq; q0 += p.nqb) {
        const uint32_t nb = std::min(p.nqb, nq - q0), tiles = (nb + p.Q - 1) / p.Q;
        if (q0 > 0 && e->timing) HX_HIP(e, hipEventRecord(e->ev0, e->stream));
        a.qslot0 = first_query + q0; a.nq = nb;
        if (sc) {
            HX_HIP(e, hipMemsetAsync(d + o_sh, 0xFF, nq_pad * 8, e->stream));
            if (n_seed) {
                ExArgs as = a;
                as.S = std::min<uint32_t>(p.S, n_seed / (4 * p.R)); as.per = (n_seed + as.S - 1) / as.S; as.S = (n_seed + as.per - 1) / as.per; as.n = n_seed;
                HX_HIP(e, ex_scan(e, op, as, p.Q, tiles));
                hipLaunchKernelGGL(k_exact_merge, dim3(nb), dim3(EX_MERGE_THREADS), (size_t)p.cap2 * 12, e->stream, as.gkey, as.gid, as.gcnt, as.S, p.cap, p.Q, k, p.cap2,
                                   0, (uint32_t *)(d + o_oid), (double *)(d + o_od), (uint32_t *)(d + o_oc));
                HX_HIP(e, hipGetLastError());
                hipLaunchKernelGGL(k_exact_seed, dim3((nb + 255) / 256), dim3(256), 0, e->stream, (const uint32_t *)(d + o_oc), (const double *)(d + o_od), k, nb, c.shared);
                HX_HIP(e, hipGetLastError());
                launches += 3; seed_rows += (uint64_t)n_seed * tiles;
            }
            HX_HIP(e, (p.Q == 4 ? ex_launch_scan_sc<4, 4>(e, a, c, tiles) : ex_launch_scan_sc<4, 1>(e, a, c, tiles)));
        } else {
            HX_HIP(e, ex_scan(e, op, a, p.Q, tiles));
        }
        hipLaunchKernelGGL(k_exact_merge, dim3(nb), dim3(EX_MERGE_THREADS), (size_t)p.cap2 * 12, e->stream, a.gkey, a.gid, a.gcnt, p.S, p.cap, p.Q, k, p.cap2,
                           (int)(op == HX_OP_NEG_IP), (uint32_t *)(d + o_oid), (double *)(d + o_od), (uint32_t *)(d + o_oc));
        HX_HIP(e, hipGetLastError());
        launches += 2;
        if (e->timing) HX_HIP(e, hipEventRecord(e->ev1, e->stream));
        HX_HIP(e, hipMemcpyAsync(ids_out + (size_t)q0 * k, d + o_oid, (size_t)nb * k * 4, hipMemcpyDeviceToHost, e->stream));
        HX_HIP(e, hipMemcpyAsync(dist_out + (size_t)q0 * k, d + o_od, (size_t)nb * k * 8, hipMemcpyDeviceToHost, e->stream));
        HX_HIP(e, hipMemcpyAsync(counts_out + q0, d + o_oc, (size_t)nb * 4, hipMemcpyDeviceToHost, e->stream));
        if (sc) HX_HIP(e, hipMemcpyAsync(sc_stats, d + o_st, 16, hipMemcpyDeviceToHost, e->stream));   // running totals of this call
        HX_HIP(e, hipStreamSynchronize(e->stream));
        if (e->timing) { float t = 0.f; HX_HIP(e, hipEventElapsedTime(&t, e->ev0, e->ev1)); ms += t; }
    }
    e->xs_coded += sc_stats[0]; e->xs_fetched += sc_stats[1] + seed_rows;
    if (e->timing) {
        e->last_ms = (float)ms;
        e->stat_exact.launches += launches; e->stat_exact.units += n_pass * nq; e->stat_exact.ms += ms;
    }
    return HX_OK;
}

// The body of hx_exact_search_filtered and hx_exact_search_set.  The filter source is host bitmaps (filters; set == nullptr) or the resident lists of
// a filter set (set; filters unused): then the counts are the set's offsets, nothing is uploaded or compacted and the set's id array is the id base.
int exf_run(hx_engine *e, int op, uint32_t first_query, uint32_t nq, uint64_t first_row, uint64_t n_rows, uint32_t n_filters,
            const uint64_t *const *filters, const hx_filterset *set, const int32_t *filter_of, uint32_t k, uint32_t *ids_out, double *dist_out,
            uint32_t *counts_out)
{
    const bool bit = e->dtype == HX_BIT;
    if (op < HX_OP_L2 || op > HX_OP_JACCARD || bit != (op == HX_OP_HAMMING || op == HX_OP_JACCARD))
        return e->fail(HX_E_ARG, "operator is not defined for this column type");
    if (k == 0 || k > HX_EXACT_MAX_K) return e->fail(HX_E_ARG, "k must be in [1, HX_EXACT_MAX_K]");
    if (first_row > e->n_rows || n_rows > e->n_rows - first_row) return e->fail(HX_E_ARG, "row range past the stored rows");
    if (first_row + n_rows > 0xFFFFFFFFull) return e->fail(HX_E_ARG, "row range past 2^32 - 1");
    if ((uint64_t)first_query + nq > e->n_queries) return e->fail(HX_E_ARG, "query range past the uploaded query slots");
    if (!ids_out || !dist_out || !counts_out) return e->fail(HX_E_ARG, "NULL output");
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
    if (nq == 0) return HX_OK;
    for (uint32_t v = 0; v <= n_filters; v++)                  // one distinct filter: this is hx_exact_search with that bitmap
        if (g_nq[v] == nq) {
            const HxIdList one{set && v ? set->d_ids + set_off(v) : nullptr, set && v ? set_cnt(v) : 0};
            return ex_search(e, op, first_query, nq, first_row, n_rows, v && !set ? filters[v - 1] : nullptr, v && set ? &one : nullptr, k, ids_out, dist_out,
                             counts_out);
        }

    const uint64_t n_words = (n_rows + 63) / 64;
    uint64_t g_pass[HX_EXACT_MAX_FILTERS + 1] = {}, g_ids[HX_EXACT_MAX_FILTERS + 1], total_ids = 0, units = 0;
    const uint64_t *ref_words[HX_EXACT_MAX_FILTERS]; uint32_t n_ref = 0;      // the referenced bitmaps that pass a row, in filter order
    ExCompactBases bases{};
    g_pass[0] = n_rows; g_ids[0] = EX_NO_IDS;
    for (uint32_t v = 1; v <= n_filters; v++) {
        if (!g_nq[v]) continue;
        if (set) { g_pass[v] = set_cnt(v); g_ids[v] = set_off(v); continue; }
        const uint64_t *words = filters[v - 1];
        uint64_t n = 0;
        for (uint64_t w = 0; w < n_words; w++) {
            uint64_t b = words[w];
            if (w == n_words - 1 && (n_rows & 63)) b &= (1ull << (n_rows & 63)) - 1;
            n += (uint64_t)__builtin_popcountll(b);
        }
        g_pass[v] = n;
        if (!n) continue;
        g_ids[v] = total_ids; bases.base[n_ref] = total_ids; ref_words[n_ref++] = words; total_ids += n;
    }
    // the grouped query order: by filter, queries of a filter in the caller's order; a query whose filter passes nothing is answered here
    std::vector<uint32_t> order; order.reserve(nq);
    std::vector<ExGroup> groups;
    {
        uint32_t start[HX_EXACT_MAX_FILTERS + 2]; uint32_t n_live = 0;
        for (uint32_t v = 0; v <= n_filters; v++) {
            start[v] = n_live;
            if (g_nq[v] && g_pass[v]) { groups.push_back(ExGroup{g_nq[v], g_pass[v], g_ids[v]}); n_live += g_nq[v]; }
        }
        order.resize(n_live);
        for (uint32_t i = 0; i < nq; i++) {
            const uint32_t v = filter_of ? (uint32_t)(filter_of[i] + 1) : 0;
            units += g_pass[v];
            if (g_pass[v]) { order[start[v]++] = i; continue; }
            for (uint32_t j = 0; j < k; j++) { ids_out[(size_t)i * k + j] = 0xFFFFFFFFu; dist_out[(size_t)i * k + j] = std::nan(""); }
            counts_out[i] = 0;
        }
    }
    if (order.empty()) return HX_OK;
    HX_HIP(e, hipSetDevice(e->device));

    const uint32_t pitch = (uint32_t)e->pitch;
    uint64_t budget = 256ull << 20;
    if (const char *env = getenv("HX_EXACT_SCRATCH")) budget = std::max<uint64_t>(1, strtoull(env, nullptr, 10));
    const ExGPlan p = ex_plan(groups, k, pitch, e->dtype == HX_SPARSE, budget);

    // device: id lists | bitmaps | list counters | slots, workgroup and merge descriptors | the largest block's buffers, counts and outputs
    const size_t nq_live = order.size();
    const size_t o_words = al16((size_t)total_ids * 4), o_ctr = o_words + al16((size_t)n_ref * n_words * 8), o_slots = o_ctr + HX_EXACT_MAX_FILTERS * 4;
    const size_t o_wg = o_slots + al16(nq_live * 4), o_mq = o_wg + al16(p.wg.size() * sizeof(ExWg)), o_key = o_mq + al16(p.mq.size() * sizeof(ExMq));
    const size_t o_id = o_key + al16((size_t)p.max_entries * 8), o_cnt = o_id + al16((size_t)p.max_entries * 4), o_oid = o_cnt + al16((size_t)p.max_counts * 4);
    const size_t o_od = o_oid + al16((size_t)p.max_nq * k * 4), o_oc = o_od + al16((size_t)p.max_nq * k * 8), need = o_oc + al16((size_t)p.max_nq * 4);
    if (need > e->cap_exact) {
        if (e->d_exact) (void)hipFree(e->d_exact);
        e->d_exact = nullptr; e->cap_exact = 0;
        if (hipMalloc((void **)&e->d_exact, need) != hipSuccess) return e->fail(HX_E_NOMEM, "cannot reserve exact-scan scratch in HBM");
        e->cap_exact = need;
    }
    uint8_t *d = e->d_exact;
    std::vector<uint8_t> meta(o_key - o_slots);
    for (size_t i = 0; i < nq_live; i++) ((uint32_t *)meta.data())[i] = first_query + order[i];
    memcpy(meta.data() + (o_wg - o_slots), p.wg.data(), p.wg.size() * sizeof(ExWg));
    memcpy(meta.data() + (o_mq - o_slots), p.mq.data(), p.mq.size() * sizeof(ExMq));
    HX_HIP(e, hipMemsetAsync(d + o_ctr, 0, HX_EXACT_MAX_FILTERS * 4, e->stream));
    HX_HIP(e, hipMemcpyAsync(d + o_slots, meta.data(), meta.size(), hipMemcpyHostToDevice, e->stream));
    for (uint32_t c = 0; c < n_ref; c++)
        HX_HIP(e, hipMemcpyAsync(d + o_words + (size_t)c * n_words * 8, ref_words[c], n_words * 8, hipMemcpyHostToDevice, e->stream));
    uint64_t launches = 0; double ms = 0.0;
    if (e->timing) HX_HIP(e, hipEventRecord(e->ev0, e->stream));   // kind 7 = kernel time: the uploads are not in it
    if (n_ref) {
        hipLaunchKernelGGL(k_exact_compact_g, dim3((uint32_t)((n_words + 255) / 256), n_ref), dim3(256), 0, e->stream,
                           (const uint64_t *)(d + o_words), n_words, n_rows, (uint32_t)first_row, (uint32_t *)d, (uint32_t *)(d + o_ctr), bases);
        HX_HIP(e, hipGetLastError());
        launches++;
    }
    ExGArgs a{};
    a.rows = e->d_rows; a.queries = e->d_queries; a.pitch = pitch; a.cap_sp = (uint32_t)std::min(e->dim, HX_SPARSE_MAX_NNZ);
    a.ids = set ? set->d_ids : (const uint32_t *)d; a.row0 = (uint32_t)first_row; a.k = k;
    a.gkey = (uint64_t *)(d + o_key); a.gid = (uint32_t *)(d + o_id); a.gcnt = (uint32_t *)(d + o_cnt);
    a.slots = (const uint32_t *)(d + o_slots);
    std::vector<uint32_t> h_ids((size_t)p.max_nq * k), h_cnt(p.max_nq);
    std::vector<double> h_dist((size_t)p.max_nq * k);
    for (size_t bi = 0; bi < p.blocks.size(); bi++) {
        const ExBlock &b = p.blocks[bi];
        if (bi > 0 && e->timing) HX_HIP(e, hipEventRecord(e->ev0, e->stream));
        for (int c = 0; c < 3; c++) {
            if (!b.nwg[c]) continue;
            a.cap = p.cap[c]; a.wg = (const ExWg *)(d + o_wg) + b.wg0[c];
            HX_HIP(e, exg_scan(e, op, a, EX_CLS_Q[c], b.nwg[c]));
            launches++;
        }
        hipLaunchKernelGGL(k_exact_merge_g, dim3(b.nq), dim3(EX_MERGE_THREADS), (size_t)p.cap2 * 12, e->stream, a.gkey, a.gid, a.gcnt,
                           (const ExMq *)(d + o_mq) + b.q0, k, p.cap2, (int)(op == HX_OP_NEG_IP), (uint32_t *)(d + o_oid), (double *)(d + o_od), (uint32_t *)(d + o_oc));
        HX_HIP(e, hipGetLastError());
        launches++;
        if (e->timing) HX_HIP(e, hipEventRecord(e->ev1, e->stream));
        HX_HIP(e, hipMemcpyAsync(h_ids.data(), d + o_oid, (size_t)b.nq * k * 4, hipMemcpyDeviceToHost, e->stream));
        HX_HIP(e, hipMemcpyAsync(h_dist.data(), d + o_od, (size_t)b.nq * k * 8, hipMemcpyDeviceToHost, e->stream));
        HX_HIP(e, hipMemcpyAsync(h_cnt.data(), d + o_oc, (size_t)b.nq * 4, hipMemcpyDeviceToHost, e->stream));
        HX_HIP(e, hipStreamSynchronize(e->stream));
        if (e->timing) { float t = 0.f; HX_HIP(e, hipEventElapsedTime(&t, e->ev0, e->ev1)); ms += t; }
        for (uint32_t j = 0; j < b.nq; j++) {                  // back into the caller's query order
            const size_t i = order[b.q0 + j];
            memcpy(ids_out + i * k, h_ids.data() + (size_t)j * k, (size_t)k * 4);
            memcpy(dist_out + i * k, h_dist.data() + (size_t)j * k, (size_t)k * 8);
            counts_out[i] = h_cnt[j];
        }
    }
    if (e->timing) {
        e->last_ms = (float)ms;
        e->stat_exact.launches += launches; e->stat_exact.units += units; e->stat_exact.ms += ms;
    }
    return HX_OK;
}

} // namespace

// =================================================================================================
// C ABI
// =================================================================================================
extern "C" int hx_exact_search(hx_engine *e, int op, uint32_t first_query, uint32_t nq, uint64_t first_row, uint64_t n_rows,
                               const uint64_t *row_pass, uint32_t k, uint32_t *ids_out, double *dist_out, uint32_t *counts_out)
{
    if (!e) return HX_E_ARG;
    return ex_search(e, op, first_query, nq, first_row, n_rows, row_pass, nullptr, k, ids_out, dist_out, counts_out);
}

extern "C" int hx_exact_search_filtered(hx_engine *e, int op, uint32_t first_query, uint32_t nq, uint64_t first_row, uint64_t n_rows,
                                        uint32_t n_filters, const uint64_t *const *filters, const int32_t *filter_of,
                                        uint32_t k, uint32_t *ids_out, double *dist_out, uint32_t *counts_out)
{
    if (!e) return HX_E_ARG;
    return exf_run(e, op, first_query, nq, first_row, n_rows, n_filters, filters, nullptr, filter_of, k, ids_out, dist_out, counts_out);
}

extern "C" int hx_exact_search_set(hx_engine *e, int op, uint32_t first_query, uint32_t nq, const hx_filterset *s, const int32_t *filter_of,
                                   uint32_t k, uint32_t *ids_out, double *dist_out, uint32_t *counts_out)
{
    if (!e) return HX_E_ARG;
    if (const int rc = hx_filterset_usable(e, s)) return rc;
    return exf_run(e, op, first_query, nq, s->first_row, s->n_rows, 0, nullptr, s, filter_of, k, ids_out, dist_out, counts_out);
}

extern "C" int hx_exact_sidecar_stats(hx_engine *e, uint64_t *rows_coded, uint64_t *rows_fetched, int reset)
{
    if (!e) return HX_E_ARG;
    if (rows_coded) *rows_coded = e->xs_coded;
    if (rows_fetched) *rows_fetched = e->xs_fetched;
    if (reset) e->xs_coded = e->xs_fetched = 0;
    return HX_OK;
}
