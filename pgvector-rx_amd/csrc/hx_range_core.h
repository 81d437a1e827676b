// hx_range_core.h -- what the range scans share (hx_range.hip: hx_exact_range, hx_range_g.hip: hx_exact_range_filtered): the lane prefix count
// of the row-order compaction, the gather of the staged segments into an output window, and the order keys' way back to values.
#pragma once
#include "hx_exact_sc.h"

#include <hipcub/hipcub.hpp>
#include <vector>

namespace {

__device__ __forceinline__ uint32_t rg_below(uint64_t m)    // set bits of m below this lane
{
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
}

// the staged segments that did not overflow, each to its CSR position when that lies in [w0, w1); one wave per segment
__global__ void __launch_bounds__(256)
k_range_gather(const uint64_t *__restrict__ skey, const uint32_t *__restrict__ sid, const uint32_t *__restrict__ cnt, const uint64_t *__restrict__ seg_base,
               uint64_t nseg, uint32_t scap, uint64_t w0, uint64_t w1, uint64_t *__restrict__ okey, uint32_t *__restrict__ oid)
{
    const uint32_t lane = threadIdx.x & 63u;
    for (uint64_t seg = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6); seg < nseg; seg += (uint64_t)gridDim.x * 4) {
        const uint32_t c = cnt[seg];
        const uint64_t sb = seg_base[seg];
        if (c == 0 || c > scap || sb >= w1 || sb + c <= w0) continue;
        const uint32_t lo = sb < w0 ? (uint32_t)(w0 - sb) : 0u, hi = (uint32_t)std::min<uint64_t>(c, w1 - sb);
        for (uint32_t t = lo + lane; t < hi; t += 64) {
            const uint64_t d = sb + t - w0;
            oid[d] = sid[seg * scap + t];
            if (okey) okey[d] = skey[seg * scap + t];
        }
    }
}

// order keys -> the values hx_exact_search returns (in place: the key array becomes the f64 array)
__global__ void k_range_values(uint64_t *__restrict__ key, uint64_t n, int neg_zero)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) key[i] = __builtin_bit_cast(uint64_t, ex_val(key[i], neg_zero != 0));
}

} // namespace
