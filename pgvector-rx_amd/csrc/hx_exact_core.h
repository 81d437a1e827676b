// hx_exact_core.h -- the row streaming shared by the exact scans (hx_exact.hip: top-k, hx_range.hip: distance thresholds).
//
// Values are the operator functions' float8 results, in the canonical summation order of hx_engine.hip:
//   <->  sqrt((f64) l2sq)                                vector.rs:586-593, halfvec.rs:751-763, sparsevec <->
//   <#>  -(f64) ip                                       vector.rs:624-633
//   <=>  1 - clamp(s / sqrt((f64) na * (f64) nb), -1, 1) vector.rs:541-556,638-647 (three f32 accumulators; NaN stays NaN)
//   <+>  (f64) l1                                        vector.rs:652-659
//   <~>  (f64) popcount(a ^ b)                           bitvec.rs:144-153
//   <%>  jaccard, ab == 0 -> 1.0                         bitvec.rs:113-132,158-167
// The support-function parts (l2sq, ip, l1, popcounts) are the OpXxx operators of hx_ops.h with K1's lane mapping, so each is the very
// value hx_distances returns for that pair; the cosine norms are the same sums with both operands the row (or the query).
//
// Order: PostgreSQL's float8 comparison (-0.0 == +0.0, +inf < NaN, all NaNs equal).  A value is carried as a 64-bit order key (ex_key)
// under which that comparison is the integer one; the key is a bijection on values apart from the two zeros and the NaN payloads, and
// ex_val inverts it (a zero is -0.0 exactly for <#>: its f32 sum starts at +0.0 and can never become -0.0).
//
// A scan workgroup parks Q queries in LDS (ex_park); each wave streams RIF row slots at a time (LPR lanes per row, 16-byte fragments, as
// K1) and ex_eval evaluates every row fragment against every parked query, one accumulator per (row, query) -- a row is read from HBM once
// per query tile.  Sparsevec rows: one lane per (query, row) pair with the merge joins of hx_sparse.hip.
#pragma once
#include "hx_ops.h"

namespace {

constexpr int EX_WAVES = 4, EX_THREADS = EX_WAVES * 64;

__host__ __device__ __forceinline__ uint64_t ex_key(double d)
{
    if (d != d) return ~0ull;                                  // every NaN: last, equal to every other NaN
    if (d == 0.0) return 0x8000000000000000ull;                // -0.0 == +0.0
    const uint64_t b = __builtin_bit_cast(uint64_t, d);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
__device__ __forceinline__ double ex_val(uint64_t key, bool neg_zero)
{
    if (key == ~0ull) return __builtin_bit_cast(double, 0x7ff8000000000000ull);
    if (key == 0x8000000000000000ull) return neg_zero ? -0.0 : 0.0;
    return __builtin_bit_cast(double, (key >> 63) ? (key ^ 0x8000000000000000ull) : ~key);
}

// top-k in LDS: entries ordered by (key, id); shared by the exact scan, its merge and the re-rank
__device__ __forceinline__ bool ex_less(uint64_t ka, uint32_t ia, uint64_t kb, uint32_t ib) { return ka < kb || (ka == kb && ia < ib); }

// bitonic sort of P (a power of two) entries in LDS by (key, id), by the whole workgroup
__device__ void ex_sort(uint64_t *key, uint32_t *id, uint32_t P)
{
    for (uint32_t k2 = 2; k2 <= P; k2 <<= 1)
        for (uint32_t j = k2 >> 1; j > 0; j >>= 1) {
            for (uint32_t i = threadIdx.x; i < P; i += blockDim.x) {
                const uint32_t x = i ^ j;
                if (x > i) {
                    const uint64_t ka = key[i], kb = key[x];
                    const uint32_t ia = id[i], ib = id[x];
                    if (ex_less(kb, ib, ka, ia) == ((i & k2) == 0)) { key[i] = kb; key[x] = ka; id[i] = ib; id[x] = ia; }
                }
            }
            __syncthreads();
        }
}
__device__ __forceinline__ uint32_t ex_pow2(uint32_t n) { uint32_t p = 2; while (p < n) p <<= 1; return p; }

// sorts the n entries in skey/sid (LDS), keeps the best min(n, k); *cnt / *thr_k / *thr_i updated.  Whole workgroup, uniform arguments.
__device__ void ex_keep(uint64_t *skey, uint32_t *sid, uint32_t n, uint32_t k, uint32_t *cnt, uint64_t *thr_k, uint32_t *thr_i)
{
    const uint32_t P = ex_pow2(n);
    for (uint32_t i = n + threadIdx.x; i < P; i += blockDim.x) { skey[i] = ~0ull; sid[i] = ~0u; }
    __syncthreads();
    ex_sort(skey, sid, P);
    if (threadIdx.x == 0) {
        const uint32_t m = n < k ? n : k;
        *cnt = m;
        if (m == k) { *thr_k = skey[k - 1]; *thr_i = sid[k - 1]; }
    }
    __syncthreads();
}

// the f64 operator value from the lane partials (all lanes of the row's LPR-lane group get it)
template <class OP, int HOP, int LPR>
__device__ __forceinline__ double ex_value(const typename OP::acc_t &acc, float na, float nb)
{
    if constexpr (HOP == HX_OP_HAMMING) return (double)lanes_sum_i<LPR>(acc);
    else if constexpr (HOP == HX_OP_JACCARD) {
        const int ab = lanes_sum_i<LPR>(acc.ab), aa = lanes_sum_i<LPR>(acc.aa), bb = lanes_sum_i<LPR>(acc.bb);
        return ab == 0 ? 1.0 : 1.0 - ((double)ab / (double)(aa + bb - ab));
    } else {
        const float s = lanes_sum_f<LPR>(acc);
        if constexpr (HOP == HX_OP_L2) return sqrt((double)s);
        else if constexpr (HOP == HX_OP_NEG_IP) return -(double)s;
        else if constexpr (HOP == HX_OP_L1) return (double)s;
        else {
            double sim = (double)s / sqrt((double)na * (double)nb);
            if (sim < -1.0) sim = -1.0;
            if (sim > 1.0) sim = 1.0;                          // f64::clamp: NaN stays NaN
            return 1.0 - sim;
        }
    }
}

// Parks the Q queries of query tile `tile` (slots qslot0 + tile * Q ..; a partial tile re-reads the block's last query) in q_lds, 16-byte
// fragments interleaved by query, and for <=> their |q|^2 in the canonical order in qn[] (the row's is formed with its dot products).
// init() runs between the loads and the first barrier (the caller's own LDS state).  Whole workgroup; ends synchronised.
template <class OP, int HOP, int Q, class INIT>
__device__ __forceinline__ void ex_park(const uint8_t *queries, uint32_t qslot0, uint32_t nq, uint32_t tile, uint32_t pitch, uint32_t cap_sp,
                                        uint8_t *q_lds, float *qn, INIT &&init)
{
    constexpr bool kCos = HOP == HX_OP_COSINE, kSp = OP::kSparse;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    for (int i = 0; i < Q; i++) {
        const uint32_t qi = tile * Q + i < nq ? tile * Q + i : nq - 1;
        const uint8_t *src = queries + (size_t)(qslot0 + qi) * pitch;
        for (uint32_t o = threadIdx.x * 16u; o < pitch; o += EX_THREADS * 16u) *(u4 *)(q_lds + o * Q + i * 16) = *(const u4 *)(src + o);
    }
    init();
    __syncthreads();
    if constexpr (kCos) {
        for (int i = wave; i < Q; i += EX_WAVES) {
            float v = 0.0f;
            if constexpr (kSp) {
                if (lane == 0) { const SpRow r = sp_row((const uint8_t *)q_lds, cap_sp); for (int t = 0; t < r.nnz; t++) v += r.val[t] * r.val[t]; }
            } else {
                typename OP::acc_t acc; OP::init(acc);
                for (uint32_t c = lane * 16u; c < pitch; c += 1024u) { const u4 x = *(const u4 *)(q_lds + c * Q + i * 16); OP::add(acc, x, x); }
                v = lanes_sum_f<64>(acc);
            }
            if (lane == 0) qn[i] = v;
        }
        __syncthreads();
    }
}

// A value every lane of the workgroup holds, loaded from a table (a slot number, a work descriptor's field), as the scalar it is.  Beyond naming
// it uniform this ends the address chain the compiler's occupancy heuristic follows: it counts an access whose address derives from a loaded value
// as indirect, and a kernel with many of those is scheduled for 4 waves per SIMD at most -- 20 to 45 VGPRs more than the same loop needs when
// its tile and slice come from blockIdx.
__device__ __forceinline__ uint32_t ex_uni(uint32_t v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ uint64_t ex_uni(uint64_t v) { return ((uint64_t)ex_uni((uint32_t)(v >> 32)) << 32) | ex_uni((uint32_t)v); }

// ex_park for queries that are not consecutive slots: parks slots[0 .. nlive) (nlive <= Q; the rest of a partial tile re-reads the last one).
// slots and nlive are uniform over the workgroup.  Same LDS layout, qn[] and barriers as ex_park.
template <class OP, int HOP, int Q, class INIT>
__device__ __forceinline__ void ex_park_slots(const uint8_t *queries, const uint32_t *__restrict__ slots, uint32_t nlive, uint32_t pitch, uint32_t cap_sp,
                                              uint8_t *q_lds, float *qn, INIT &&init)
{
    constexpr bool kCos = HOP == HX_OP_COSINE, kSp = OP::kSparse;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    for (int i = 0; i < Q; i++) {
        const uint8_t *src = queries + (size_t)ex_uni(slots[(uint32_t)i < nlive ? (uint32_t)i : nlive - 1]) * pitch;
        for (uint32_t o = threadIdx.x * 16u; o < pitch; o += EX_THREADS * 16u) *(u4 *)(q_lds + o * Q + i * 16) = *(const u4 *)(src + o);
    }
    init();
    __syncthreads();
    if constexpr (kCos) {
        for (int i = wave; i < Q; i += EX_WAVES) {
            float v = 0.0f;
            if constexpr (kSp) {
                if (lane == 0) { const SpRow r = sp_row((const uint8_t *)q_lds, cap_sp); for (int t = 0; t < r.nnz; t++) v += r.val[t] * r.val[t]; }
            } else {
                typename OP::acc_t acc; OP::init(acc);
                for (uint32_t c = lane * 16u; c < pitch; c += 1024u) { const u4 x = *(const u4 *)(q_lds + c * Q + i * 16); OP::add(acc, x, x); }
                v = lanes_sum_f<64>(acc);
            }
            if (lane == 0) qn[i] = v;
        }
        __syncthreads();
    }
}

// Evaluates the RIF row slots rp[0..RIF) of this lane's LPR-lane group against the Q parked queries and calls emit(i, j, value) for query i
// and slot j, slot-major (j outer, i inner); every lane of the group holds the value.  Sparsevec: LPR == RIF == Q == 1.
template <class OP, int HOP, int LPR, int RIF, int Q, class EMIT>
__device__ __forceinline__ void ex_eval(const uint8_t *q_lds, const float *qn, const uint8_t *const *rp, uint32_t pitch, uint32_t cap_sp, uint32_t sl,
                                        EMIT &emit)
{
    constexpr bool kCos = HOP == HX_OP_COSINE, kSp = OP::kSparse;
    if constexpr (kSp) {
        static_assert(LPR == 1 && RIF == 1 && Q == 1, "sparsevec: one lane per pair");
        const SpRow q = sp_row((const uint8_t *)q_lds, cap_sp), r = sp_row(rp[0], cap_sp);
        constexpr int K = HOP == HX_OP_L2 ? K_L2 : HOP == HX_OP_L1 ? K_L1 : K_IP;
        const float v = sp_merge<K>(q, r);                     // -ip for K_IP
        double dv;
        if constexpr (HOP == HX_OP_L2) dv = sqrt((double)v);
        else if constexpr (HOP == HX_OP_NEG_IP || HOP == HX_OP_L1) dv = (double)v;
        else {                                                 // sparsevec_cosine_distance: f32 norms over the stored values
            float na = 0.0f;
            for (int t = 0; t < r.nnz; t++) na += r.val[t] * r.val[t];
            double sim = (double)(-v) / sqrt((double)qn[0] * (double)na);
            if (sim < -1.0) sim = -1.0;
            if (sim > 1.0) sim = 1.0;
            dv = 1.0 - sim;
        }
        emit(0, 0, dv);
    } else {
        typename OP::acc_t acc[RIF][Q];
        float nacc[RIF];
#pragma unroll
        for (int j = 0; j < RIF; j++) {
            nacc[j] = 0.0f;
#pragma unroll
            for (int i = 0; i < Q; i++) OP::init(acc[j][i]);
        }
        for (uint32_t c = sl * 16u; c < pitch; c += LPR * 16u) {
            u4 rv[RIF];
#pragma unroll
            for (int j = 0; j < RIF; j++) rv[j] = *(const u4 *)(rp[j] + c);
            if constexpr (kCos) {
#pragma unroll
                for (int j = 0; j < RIF; j++) OP::add(nacc[j], rv[j], rv[j]);
            }
#pragma unroll
            for (int i = 0; i < Q; i++) {
                const u4 qv = *(const u4 *)(q_lds + c * Q + i * 16);
#pragma unroll
                for (int j = 0; j < RIF; j++) OP::add(acc[j][i], qv, rv[j]);
            }
        }
#pragma unroll
        for (int j = 0; j < RIF; j++) {
            const float na = kCos ? lanes_sum_f<LPR>(nacc[j]) : 0.0f;
#pragma unroll
            for (int i = 0; i < Q; i++) emit(i, j, ex_value<OP, HOP, LPR>(acc[j][i], na, kCos ? qn[i] : 0.0f));
        }
    }
}

} // namespace
