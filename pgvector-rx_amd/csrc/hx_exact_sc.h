// hx_exact_sc.h -- the 8-bit sidecar pre-pass of the exact scans (hx_exact.hip: top-k, hx_range.hip: `<` / `<=` thresholds) on f32 L2 engines
// that keep a sidecar ("Exact and range scans").
//
// A row is decided from its code row (al16(dim) bytes) and 16 bytes of metadata where the proven bound LB <= d (hx_ops.h: hx_l2_lb_finish) already
// places its value past a threshold key T of the query: skipped iff LB > 0 and ex_key(sqrt((double)LB)) > T, strictly.  The f64 root is monotone,
// so ex_key(value) >= ex_key(sqrt(LB)) > T and the unchanged evaluation would not have kept the row.  LB = 0 (rows with inf / NaN, bounds lost to
// rounding) never skips.  Survivors go through ex_eval as before, so every output bit is that of the scan without the sidecar.
//
// Lane mapping: 16 lanes per row (16 codes = one 16-byte load per lane and 256-byte chunk), 4 rows per load instruction, SC_P such instructions x
// SC_CG chunks in flight: a wave step decides SC_ROWS = 16 rows with up to 12 KiB of loads outstanding.  D^ is summed per lane and then over the 16
// lanes, an order the bound allows.  The arithmetic is f_lb_reject's: fmaf(step, c, lo), fmaf(d, d, acc), hx_l2_lb_finish with nterm = pitch / 4.
#pragma once
#include "hx_exact_core.h"

#include <cstdlib>

namespace {

constexpr int SC_P = 4, SC_CG = 3, SC_ROWS = 4 * SC_P;

struct ScArgs {
    const uint8_t *codes; const float *meta; uint32_t cpitch, dim, nterm;
    uint64_t *shared;                                         // top-k: one threshold key per query of the block, lowered with atomicMin
    unsigned long long *stats;                                // {code rows read, f32 rows read}
};

// HX_EXACT_SIDECAR, read at each call: 0 forces the scans without the pre-pass, 1 forces it wherever it is defined; otherwise the calls whose
// shape measured faster with it take it: top-k from SC_MIN_ROWS_TOPK passing rows (the seeded calls), ranges from SC_MIN_ROWS_RANGE.
constexpr uint64_t SC_MIN_ROWS_TOPK = 131072, SC_MIN_ROWS_RANGE = 65536;
inline bool sc_enabled(uint64_t n_pass, uint64_t min_rows)
{
    const char *v = getenv("HX_EXACT_SIDECAR");
    if (v && v[0] == '0' && v[1] == '\0') return false;
    if (v && v[0] == '1' && v[1] == '\0') return true;
    return n_pass >= min_rows;
}

// Rows t = 4 * s + g (s < SC_P, g = lane / 16) of a wave step, ids rid[s] for this lane's group; rows t >= nvalid are padding.  T[i]: threshold
// key of parked query i (LDS or global), live: bit i set for the queries that count.  Returns the wave-uniform mask of the rows at least one
// live query does not skip.  q_lds: the Q parked f32 queries, 16-byte fragments interleaved by query (ex_park).
template <int Q>
__device__ __forceinline__ uint32_t sc_survivors(const ScArgs &c, const uint8_t *q_lds, const uint32_t (&rid)[SC_P], uint32_t nvalid, const uint64_t *T,
                                                 uint32_t live, uint32_t lane)
{
    static_assert(SC_P * Q <= 16, "one (row, query) pair per lane of a 16-lane group");
    const uint32_t g = lane >> 4, l16 = lane & 15u;
    const uint32_t nck = (c.cpitch + 255u) >> 8;
    const uint8_t *rb[SC_P]; float lo[SC_P], st[SC_P], ex[SC_P], acc[SC_P][Q];
#pragma unroll
    for (int s = 0; s < SC_P; s++) {
        rb[s] = c.codes + (size_t)rid[s] * c.cpitch;
        const float4 m = *(const float4 *)(c.meta + (size_t)rid[s] * HX_SC_META);
        lo[s] = m.x; st[s] = m.y; ex[s] = m.z;
#pragma unroll
        for (int i = 0; i < Q; i++) acc[s][i] = 0.0f;
    }
#pragma unroll 1
    for (uint32_t c0 = 0; c0 < nck; c0 += SC_CG) {
        u4 rv[SC_P][SC_CG];
#pragma unroll
        for (int k = 0; k < SC_CG; k++) {                      // chunks past the row re-read its first bytes; not used
            const uint32_t o = (c0 + (uint32_t)k) * 256u + l16 * 16u, off = o < c.cpitch ? o : 0u;
#pragma unroll
            for (int s = 0; s < SC_P; s++) rv[s][k] = *(const u4 *)(rb[s] + off);
        }
#pragma unroll
        for (int k = 0; k < SC_CG; k++) {
            const uint32_t i0 = (c0 + (uint32_t)k) * 256u + l16 * 16u;
            if (i0 < c.dim) {
                const uint32_t lim = c.dim - i0;              // >= 16 except in a row's last, partial chunk: its terms past dim are 0
#pragma unroll
                for (int w = 0; w < 4; w++) {
                    if ((uint32_t)(4 * w) < lim) {
                        float xh[SC_P][4];
#pragma unroll
                        for (int s = 0; s < SC_P; s++)
#pragma unroll
                            for (int t = 0; t < 4; t++) xh[s][t] = fmaf(st[s], (float)((rv[s][k][w] >> (8 * t)) & 0xffu), lo[s]);
#pragma unroll
                        for (int i = 0; i < Q; i++) {
                            const u4 qw = *(const u4 *)(q_lds + ((size_t)(i0 / 4u + (uint32_t)w) * Q + i) * 16u);
#pragma unroll
                            for (int s = 0; s < SC_P; s++)
#pragma unroll
                                for (int t = 0; t < 4; t++) {
                                    const float d = (uint32_t)(4 * w + t) < lim ? bits2f(qw[t]) - xh[s][t] : 0.0f;
                                    acc[s][i] = fmaf(d, d, acc[s][i]);
                                }
                        }
                    }
                }
            }
        }
    }
    // lane l16 of a group takes the pair (row slot s = l16 % 4, query i = l16 / 4): one f64 root per lane
    float my = 0.0f;
#pragma unroll
    for (int s = 0; s < SC_P; s++)
#pragma unroll
        for (int i = 0; i < Q; i++) {
            const float lb = hx_l2_lb_finish(lanes_sum_f<16>(acc[s][i]), ex[s], c.nterm);
            if (l16 == (uint32_t)(s + 4 * i)) my = lb;
        }
    const uint32_t qi = l16 >> 2, ps = l16 & 3u;
    bool keep = false;
    if (qi < (uint32_t)Q && ((live >> qi) & 1u) && 4u * ps + g < nvalid)
        keep = !(my > 0.0f && ex_key(sqrt((double)my)) > T[qi]);     // LB 0 never skips
    const unsigned long long b = __ballot(keep);
    uint32_t m = 0;
#pragma unroll
    for (int g2 = 0; g2 < 4; g2++)
#pragma unroll
        for (int s = 0; s < SC_P; s++)
            if ((b >> (16 * g2 + s)) & 0x1111ull) m |= 1u << (4 * s + g2);
    return m;
}

} // namespace
