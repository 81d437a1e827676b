// hx_sidecar.hip -- the 8-bit row sidecar of f32 L2 engines: its encoder, which every entry point that writes rows calls, and
// the C ABI around it (read-back, counters, the bound of a query against listed rows).  The traversal kernel reads the sidecar through
// FusedParams::sc_codes / sc_meta (hx_fused_core.h: f_lb_reject).
#include "hx_fused_core.h"

// One wave per row: lo / hi over the row, codes c_i = rint((x_i - lo) / step) clamped to [0, 255], then e_x from x^_i = fmaf(step, c_i, lo) -- the
// kernels' own expression -- as an f64 sum of squares, widened by 2^-40 (the f64 rounding of <= 2000 squares, their sum and the root; by 2^-36 for
// the up to 16000 squares of a scan-only engine's rows past 2000 dimensions) and rounded up to f32.  A row with a non-finite value, range, step or x^_i gets e_x = +inf: its bound is always 0.  Codes past dim (up to the pitch) are 0.
__global__ void __launch_bounds__(256) k_sc_encode(const uint8_t *rows, uint32_t pitch, uint32_t dim, uint64_t first, uint64_t n, uint8_t *codes, uint32_t cpitch, float *meta)
{
    const uint64_t r = (uint64_t)blockIdx.x * 4u + (threadIdx.x >> 6);
    const uint32_t lane = threadIdx.x & 63u;
    if (r >= n) return;                                   // wave-uniform
    const float *x = (const float *)(rows + (first + r) * pitch);
    float lo = __builtin_inff(), hi = -__builtin_inff(); bool fin = true;
    for (uint32_t i = lane; i < dim; i += 64u) { const float v = x[i]; fin = fin && __builtin_isfinite(v); lo = fminf(lo, v); hi = fmaxf(hi, v); }
    for (int o = 32; o >= 1; o >>= 1) { lo = fminf(lo, __shfl_xor(lo, o, 64)); hi = fmaxf(hi, __shfl_xor(hi, o, 64)); }
    bool ok = __all(fin) != 0;
    const float step = ok ? (hi - lo) / 255.0f : 0.0f;
    ok = ok && __builtin_isfinite(step);
    uint8_t *cr = codes + (first + r) * cpitch;
    double err = 0.0; bool fx = true;
    for (uint32_t i = lane; i < cpitch; i += 64u) {
        uint32_t c = 0u;
        if (i < dim) {
            const float v = x[i];
            if (ok && step > 0.0f) { const float t = rintf((v - lo) / step); c = t >= 255.0f ? 255u : t > 0.0f ? (uint32_t)t : 0u; }
            const float xh = fmaf(step, (float)c, lo);
            fx = fx && __builtin_isfinite(xh);
            const double dd = (double)v - (double)xh;
            err += dd * dd;
        }
        cr[i] = (uint8_t)c;
    }
    for (int o = 32; o >= 1; o >>= 1) err += __shfl_xor(err, o, 64);
    ok = ok && __all(fx) != 0;
    const double e = sqrt(err) * (dim > 2000u ? 1.0 + 0x1p-36 : 1.0 + 0x1p-40);
    float ex = (float)e;
    if ((double)ex < e) ex = nextafterf(ex, __builtin_inff());
    if (!ok || !__builtin_isfinite(ex)) ex = __builtin_inff();
    if (lane == 0u) *(float4 *)(meta + (first + r) * HX_SC_META) = make_float4(ok ? lo : 0.0f, step, ex, 0.0f);
}

// LB of one query (row id, or HX_QUERY_SLOT | slot) against ids[0..n), 64 ids per wave, by the traversal kernel's own code (tests)
__global__ void __launch_bounds__(64) k_sc_bounds(FRows fr, const uint8_t *qsrc, FCodes c, const uint32_t *ids, uint32_t n, float *out)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
    const uint32_t lane = threadIdx.x, j0 = blockIdx.x * 64u;
    f_park_w(fr, qsrc, lane, (lds_u8 *)lds);
    (void)f_lb_reject<true>(c, (const lds_u8 *)lds, ids + j0, n - j0 < 64u ? n - j0 : 64u, lane, 0.0f, out + j0);
}

int hx_sidecar_encode(hx_engine *e, uint64_t first, uint64_t n)
{
    if (!e->d_sc_codes || !n) return HX_OK;
    hipLaunchKernelGGL(k_sc_encode, dim3((uint32_t)((n + 3) / 4)), dim3(256), 0, e->stream, e->d_rows, (uint32_t)e->pitch, (uint32_t)e->dim, first, n,
                       e->d_sc_codes, e->sc_pitch, e->d_sc_meta);
    HX_HIP(e, hipGetLastError());
    return HX_OK;
}

extern "C" {

int hx_sidecar_read(hx_engine *e, uint64_t first, uint64_t n, void *codes_host, float *meta_host)
{
    if (!e) return HX_E_ARG;
    if (!e->d_sc_codes) return e->fail(HX_E_STATE, "this engine keeps no row sidecar (f32 L2 engines of more than 128 dimensions, without HX_CREATE_NO_SIDECAR)");
    if (first + n > e->n_rows) return e->fail(HX_E_ARG, "row range out of bounds");
    if (!n) return HX_OK;
    if (!codes_host && !meta_host) return e->fail(HX_E_ARG, "NULL argument");
    HX_HIP(e, hipSetDevice(e->device));
    if (codes_host) HX_HIP(e, hipMemcpy2DAsync(codes_host, (size_t)e->dim, e->d_sc_codes + first * e->sc_pitch, e->sc_pitch, (size_t)e->dim, n, hipMemcpyDeviceToHost, e->stream));
    if (meta_host) HX_HIP(e, hipMemcpy2DAsync(meta_host, 3 * sizeof(float), e->d_sc_meta + first * HX_SC_META, HX_SC_META * sizeof(float), 3 * sizeof(float), n, hipMemcpyDeviceToHost, e->stream));
    HX_HIP(e, hipStreamSynchronize(e->stream));
    return HX_OK;
}

int hx_sidecar_stats(hx_engine *e, uint64_t *rows_fetched, uint64_t *rows_rejected, int reset)
{
    if (!e) return HX_E_ARG;
    if (rows_fetched) *rows_fetched = e->sc_rows;
    if (rows_rejected) *rows_rejected = e->sc_rej;
    if (reset) e->sc_rows = e->sc_rej = 0;
    return HX_OK;
}

int hx_sidecar_bounds(hx_engine *e, uint32_t query, const uint32_t *ids, uint32_t n, float *lb_host)
{
    if (!e) return HX_E_ARG;
    if (!e->d_sc_codes) return e->fail(HX_E_STATE, "this engine keeps no row sidecar (f32 L2 engines of more than 128 dimensions, without HX_CREATE_NO_SIDECAR)");
    if (!n) return HX_OK;
    if (!ids || !lb_host) return e->fail(HX_E_ARG, "NULL argument");
    for (uint32_t i = 0; i < n; i++) if (ids[i] >= e->n_rows) return e->fail(HX_E_ARG, "row id out of range");
    const uint8_t *qsrc;
    if (query & HX_QUERY_SLOT) { if ((query & 0x7fffffffu) >= e->n_queries) return e->fail(HX_E_ARG, "query slot out of range"); qsrc = e->d_queries + (size_t)(query & 0x7fffffffu) * e->pitch; }
    else { if (query >= e->n_rows) return e->fail(HX_E_ARG, "query row id out of range"); qsrc = e->d_rows + (size_t)query * e->pitch; }
    HX_HIP(e, hipSetDevice(e->device));
    uint8_t *buf = nullptr;
    HX_HIP(e, hipMalloc((void **)&buf, (size_t)n * 8));
    FRows fr; fr.rows = e->d_rows; fr.pitch = (uint32_t)e->pitch; fr.nch = (uint32_t)((e->pitch + 1023) / 1024); fr.dsc = nullptr;
    const FCodes c{e->d_sc_codes, e->d_sc_meta, e->sc_pitch, (uint32_t)e->dim, (uint32_t)(e->pitch >> 2)};
    hipError_t s = hipMemcpyAsync(buf, ids, (size_t)n * 4, hipMemcpyHostToDevice, e->stream);
    if (s == hipSuccess) {
        hipLaunchKernelGGL(k_sc_bounds, dim3((n + 63) / 64), dim3(64), (size_t)fr.nch * 1024, e->stream, fr, qsrc, c, (const uint32_t *)buf, n, (float *)(buf + (size_t)n * 4));
        s = hipGetLastError();
    }
    if (s == hipSuccess) s = hipMemcpyAsync(lb_host, buf + (size_t)n * 4, (size_t)n * 4, hipMemcpyDeviceToHost, e->stream);
    if (s == hipSuccess) s = hipStreamSynchronize(e->stream);
    (void)hipFree(buf);
    if (s != hipSuccess) return e->fail(HX_E_HIP, std::string("hx_sidecar_bounds: ") + hipGetErrorString(s));
    return HX_OK;
}

} // extern "C"
