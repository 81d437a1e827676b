// hx_filterset.hip -- filter sets (include/hnswrx.h: hx_filterset_*): the filters of the exact scans as row-ordered row-id lists resident on the
// device, CSR: one uint32 id array, uint64 offsets on the device and a copy of them on the host.  hx_exact_search_set / hx_exact_range_set
// (hx_exact.hip, hx_range_g.hip) hand the id array to the scan kernels as their id base and a list's offset as the group's list offset.
//
// From labels the lists are a STABLE PARTITION of the row ids by label.  Two paths:
//   up to FS_SMALL_MAX labels -- the tenant-column case -- no sort.  The rows are cut into wave tiles (a wavefront's consecutive rows, four per
//     workgroup).  k_fs_hist counts each tile's labels in LDS (one histogram per wavefront, LDS atomics) and writes them label-major, tile-minor;
//     one exclusive scan over that table gives every (label, tile) its place in the CSR -- tile-minor inside a label, so a list keeps row order
//     across tiles; k_fs_scatter reads the labels a second time, 64 rows per step, and ranks a row among the lanes of its label with one ballot
//     per label bit, a running base per label in LDS carrying the order from step to step.  No global atomic decides an output position.
//   above -- a stable radix sort (hipcub) of (label, row id) over ceil(log2(n_filters + 1)) key bits and one boundary-search kernel (k_fs_bounds).
// Every kernel bound-checks every label: one that is neither below n_filters nor HX_NO_LABEL is never used as an index, nothing is written for
// its row, and the smallest such row is reported (atomicMin), which fails the call.
// From bitmaps the lists come from hx_range_g.hip's row-ordered compaction, in chunks of at most HX_EXACT_MAX_FILTERS bitmaps.
// An append partitions the new rows alone and k_fs_concat writes, per label, the old list followed by the new segment into a fresh array.
#include "hx_internal.h"

#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <cstring>
#include <string>

namespace {

constexpr uint32_t FS_THREADS = 256, FS_WAVES = FS_THREADS / 64;
constexpr uint32_t FS_SMALL_MAX = 1024;                       // labels of the histogram path: 10 ballots per step, 4 x 4 KiB of LDS per workgroup
constexpr uint32_t FS_MIN_WROWS = 1024, FS_MAX_WTILES = 8192; // rows per wave tile: at least FS_MIN_WROWS, and so many that there are at most FS_MAX_WTILES
constexpr unsigned long long FS_NO_BAD = ~0ull;

// pass 1 of the histogram path: hist[label * n_wt + tile] = rows of that label in the wave tile.  lds: FS_WAVES x L counters.
__global__ void __launch_bounds__(FS_THREADS)
k_fs_hist(const uint32_t *__restrict__ labels, uint64_t n, uint32_t L, uint32_t wrows, uint32_t n_wt, uint32_t *__restrict__ hist,
          unsigned long long *__restrict__ bad)
{
    extern __shared__ uint32_t fs_lds[];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint32_t *h = fs_lds + (size_t)wave * L;
    for (uint32_t l = lane; l < L; l += 64) h[l] = 0;
    __syncthreads();
    const uint32_t wt = blockIdx.x * FS_WAVES + wave;
    const uint64_t r0 = (uint64_t)wt * wrows;
    if (wt < n_wt)
        for (uint32_t i = lane; i < wrows && r0 + i < n; i += 64) {
            const uint32_t lb = labels[r0 + i];
            if (lb < L) atomicAdd(&h[lb], 1u);
            else if (lb != HX_NO_LABEL) atomicMin(bad, (unsigned long long)(r0 + i));
        }
    __syncthreads();
    if (wt < n_wt)
        for (uint32_t l = lane; l < L; l += 64) hist[(size_t)l * n_wt + wt] = h[l];
}

// off[l] = where label l's first tile starts = the CSR offset; the table has one entry past the last label, whose scan is the total
__global__ void k_fs_offsets(const uint32_t *__restrict__ scan, uint32_t L, uint32_t n_wt, uint64_t *__restrict__ off)
{
    const uint32_t l = blockIdx.x * blockDim.x + threadIdx.x;
    if (l <= L) off[l] = scan[(size_t)l * n_wt];
}

// pass 2: row r0 + i of the wave tile goes to out[base[label] + its rank among the tile's earlier rows of that label].  The rank inside a step
// of 64 rows is the number of lower lanes with the same label: the lanes that agree with this one on every label bit (one ballot per bit).
__global__ void __launch_bounds__(FS_THREADS)
k_fs_scatter(const uint32_t *__restrict__ labels, uint64_t n, uint32_t L, uint32_t nbits, uint32_t wrows, uint32_t n_wt,
             const uint32_t *__restrict__ scan, uint32_t row0, uint32_t *__restrict__ out, uint64_t out_n)
{
    extern __shared__ uint32_t fs_lds[];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint32_t *base = fs_lds + (size_t)wave * L;
    const uint32_t wt = blockIdx.x * FS_WAVES + wave;
    if (wt < n_wt)
        for (uint32_t l = lane; l < L; l += 64) base[l] = scan[(size_t)l * n_wt + wt];
    __syncthreads();
    if (wt >= n_wt) return;
    const uint64_t r0 = (uint64_t)wt * wrows;
    for (uint32_t i0 = 0; i0 < wrows && r0 + i0 < n; i0 += 64) {   // the bounds are the same for all lanes: every ballot sees the whole wavefront
        const uint64_t r = r0 + i0 + lane;
        const uint32_t lb = r < n ? labels[r] : HX_NO_LABEL;
        const bool ok = lb < L;                                // a label out of range is never an index and its row is written nowhere
        unsigned long long peers = __ballot(ok);
        for (uint32_t b = 0; b < nbits; b++) {
            const bool bit = (lb >> b) & 1u;
            const unsigned long long m = __ballot(bit);
            peers &= bit ? m : ~m;
        }
        if (ok) {
            const uint32_t rank = (uint32_t)__popcll(peers & ((1ull << lane) - 1ull));
            const uint32_t pos = base[lb];                     // all lanes of the label read it before the last of them moves it on
            if ((uint64_t)pos + rank < out_n) out[pos + rank] = row0 + (uint32_t)r;
            if ((peers >> lane) == 1ull) base[lb] = pos + (uint32_t)__popcll(peers);
        }
    }
}

// the sort path: key = label, n_filters for a row in no filter (dropped: it sorts behind every list) and for a bad label (reported)
__global__ void k_fs_keys(const uint32_t *__restrict__ labels, uint64_t n, uint32_t L, uint32_t row0, uint32_t *__restrict__ keys, uint32_t *__restrict__ vals,
                          unsigned long long *__restrict__ bad)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint32_t lb = labels[i];
    if (lb >= L) {
        if (lb != HX_NO_LABEL) atomicMin(bad, (unsigned long long)i);
        lb = L;
    }
    keys[i] = lb; vals[i] = row0 + (uint32_t)i;
}

// off[l] = the first position of the sorted keys that is not below l, for l in [0, L]
__global__ void k_fs_bounds(const uint32_t *__restrict__ keys, uint64_t n, uint32_t L, uint64_t *__restrict__ off)
{
    const uint32_t l = blockIdx.x * blockDim.x + threadIdx.x;
    if (l > L) return;
    uint64_t a = 0, b = n;
    while (a < b) { const uint64_t m = (a + b) >> 1; if (keys[m] < l) a = m + 1; else b = m; }
    off[l] = a;
}

// an append's new CSR: position p of the new array lies in label l's list (new_off[l] <= p < new_off[l + 1]); the list is the old one, then
// the new rows' segment
__global__ void k_fs_concat(const uint32_t *__restrict__ old_ids, const uint64_t *__restrict__ old_off, const uint32_t *__restrict__ seg,
                            const uint64_t *__restrict__ seg_off, const uint64_t *__restrict__ new_off, uint32_t L, uint32_t *__restrict__ out, uint64_t total)
{
    const uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= total) return;
    uint32_t a = 0, b = L - 1;                                 // the last l in [0, L) with new_off[l] <= p (new_off[0] = 0)
    while (a < b) { const uint32_t m = (a + b + 1) >> 1; if (new_off[m] <= p) a = m; else b = m - 1; }
    const uint64_t j = p - new_off[a], old_n = old_off[a + 1] - old_off[a];
    out[p] = j < old_n ? old_ids[old_off[a] + j] : seg[seg_off[a] + (j - old_n)];
}

struct FsTmp {                                                // device temporaries of one build
    std::vector<void *> p;
    ~FsTmp() { for (void *q : p) (void)hipFree(q); }
    template <class T> hipError_t get(T **out, size_t bytes)
    {
        void *q = nullptr;
        hipError_t s = hipMalloc(&q, std::max<size_t>(bytes, 16));
        if (s == hipSuccess) { p.push_back(q); *out = (T *)q; }
        return s;
    }
};
struct FsClock {                                              // kind 11: the kernels between begin() and end(), when timing is on
    hx_engine *e; double ms = 0.0; uint64_t launches = 0;
    hipError_t begin() { return e->timing ? hipEventRecord(e->ev0, e->stream) : hipSuccess; }
    hipError_t end()                                           // synchronises the stream
    {
        hipError_t s = e->timing ? hipEventRecord(e->ev1, e->stream) : hipSuccess;
        if (s == hipSuccess) s = hipStreamSynchronize(e->stream);
        if (s == hipSuccess && e->timing) { float t = 0.f; s = hipEventElapsedTime(&t, e->ev0, e->ev1); ms += t; }
        return s;
    }
    void book(uint64_t units)
    {
        if (!e->timing) return;
        e->last_ms = (float)ms; e->stat_fset.launches += launches; e->stat_fset.units += units; e->stat_fset.ms += ms;
    }
};

#define FS_NOMEM(e, call)                                                                           \
    do {                                                                                            \
        if ((call) != hipSuccess) return (e)->fail(HX_E_NOMEM, "cannot reserve filter-set memory in HBM"); \
    } while (0)

// The stable partition of rows [row0, row0 + n) by d_labels (device): *seg (n_listed ids; owned by the caller), *d_off and off (L + 1 offsets from
// 0).  A bad label: HX_E_ARG with the message set and nothing returned.
int fs_partition(hx_engine *e, FsClock &clk, const uint32_t *d_labels, uint64_t n, uint32_t row0, uint32_t L, uint32_t **seg, uint64_t **d_off,
                 std::vector<uint64_t> &off)
{
    FsTmp tmp;
    uint64_t *doff = nullptr; unsigned long long *d_bad = nullptr;
    uint32_t *vals2 = nullptr;                                 // sort path: the sorted row ids
    unsigned long long bad = FS_NO_BAD;
    off.assign((size_t)L + 1, 0);
    if (hipMalloc((void **)&doff, ((size_t)L + 1) * 8) != hipSuccess) return e->fail(HX_E_NOMEM, "cannot reserve filter-set memory in HBM");
    auto drop = [&](int rc) { (void)hipFree(doff); return rc; };
#define FS_TRY(call) do { hipError_t _s = (call); if (_s != hipSuccess) return drop(e->fail(HX_E_HIP, std::string(#call) + ": " + hipGetErrorString(_s))); } while (0)
#define FS_MEM(call) do { if ((call) != hipSuccess) return drop(e->fail(HX_E_NOMEM, "cannot reserve filter-set memory in HBM")); } while (0)
    FS_MEM(tmp.get(&d_bad, 8));
    FS_TRY(hipMemsetAsync(d_bad, 0xFF, 8, e->stream));
    const uint32_t grid_l = (L + 1 + 255) / 256;
    uint32_t wrows = 0, n_wt = 0, nbits = 0; const uint32_t *scan = nullptr;
    const bool small = L <= FS_SMALL_MAX;
    if (n == 0) {
        FS_TRY(hipMemsetAsync(doff, 0, ((size_t)L + 1) * 8, e->stream));
        FS_TRY(hipStreamSynchronize(e->stream));
    } else if (small) {
        wrows = (uint32_t)std::max<uint64_t>(FS_MIN_WROWS, ((n + FS_MAX_WTILES - 1) / FS_MAX_WTILES + 63) / 64 * 64);
        n_wt = (uint32_t)((n + wrows - 1) / wrows);
        while ((1u << nbits) < L) nbits++;
        const size_t cells = (size_t)L * n_wt + 1;
        uint32_t *hist = nullptr, *sc = nullptr; void *cub = nullptr; size_t cub_bytes = 0;
        FS_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, cub_bytes, (const uint32_t *)nullptr, (uint32_t *)nullptr, cells, e->stream));
        FS_MEM(tmp.get(&hist, cells * 4)); FS_MEM(tmp.get(&sc, cells * 4)); FS_MEM(tmp.get(&cub, cub_bytes));
        FS_TRY(hipMemsetAsync(hist + (cells - 1), 0, 4, e->stream));
        FS_TRY(clk.begin());
        hipLaunchKernelGGL(k_fs_hist, dim3((n_wt + FS_WAVES - 1) / FS_WAVES), dim3(FS_THREADS), (size_t)FS_WAVES * L * 4, e->stream, d_labels, n, L, wrows, n_wt, hist, d_bad);
        FS_TRY(hipGetLastError());
        FS_TRY(hipcub::DeviceScan::ExclusiveSum(cub, cub_bytes, (const uint32_t *)hist, sc, cells, e->stream));
        hipLaunchKernelGGL(k_fs_offsets, dim3(grid_l), dim3(256), 0, e->stream, (const uint32_t *)sc, L, n_wt, doff);
        FS_TRY(hipGetLastError());
        clk.launches += 3;
        scan = sc;
    } else {
        nbits = 32 - (uint32_t)__builtin_clz(L);                // the keys are 0 .. L
        uint32_t *keys = nullptr, *keys2 = nullptr, *vals = nullptr; void *cub = nullptr; size_t cub_bytes = 0;
        FS_TRY(hipcub::DeviceRadixSort::SortPairs(nullptr, cub_bytes, (const uint32_t *)nullptr, (uint32_t *)nullptr, (const uint32_t *)nullptr, (uint32_t *)nullptr,
                                                  n, 0, (int)nbits, e->stream));
        FS_MEM(tmp.get(&keys, n * 4)); FS_MEM(tmp.get(&keys2, n * 4)); FS_MEM(tmp.get(&vals, n * 4)); FS_MEM(tmp.get(&vals2, n * 4)); FS_MEM(tmp.get(&cub, cub_bytes));
        FS_TRY(clk.begin());
        hipLaunchKernelGGL(k_fs_keys, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, e->stream, d_labels, n, L, row0, keys, vals, d_bad);
        FS_TRY(hipGetLastError());
        FS_TRY(hipcub::DeviceRadixSort::SortPairs(cub, cub_bytes, (const uint32_t *)keys, keys2, (const uint32_t *)vals, vals2, n, 0, (int)nbits, e->stream));
        hipLaunchKernelGGL(k_fs_bounds, dim3(grid_l), dim3(256), 0, e->stream, (const uint32_t *)keys2, n, L, doff);
        FS_TRY(hipGetLastError());
        clk.launches += 3;
    }
    if (n) {
        FS_TRY(hipMemcpyAsync(off.data(), doff, ((size_t)L + 1) * 8, hipMemcpyDeviceToHost, e->stream));
        FS_TRY(hipMemcpyAsync(&bad, d_bad, 8, hipMemcpyDeviceToHost, e->stream));
        FS_TRY(clk.end());
    }
    if (bad != FS_NO_BAD) {
        uint32_t lb = 0;
        FS_TRY(hipMemcpy(&lb, d_labels + bad, 4, hipMemcpyDeviceToHost));
        return drop(e->fail(HX_E_ARG, "label " + std::to_string(lb) + " of row " + std::to_string((uint64_t)row0 + bad) + " is neither below n_filters (" +
                                          std::to_string(L) + ") nor HX_NO_LABEL"));
    }
    const uint64_t n_listed = off[L];
    uint32_t *ids = nullptr;
    FS_MEM(hipMalloc((void **)&ids, std::max<uint64_t>(n_listed, 4) * 4));
    auto drop2 = [&](int rc) { (void)hipFree(ids); return drop(rc); };
#define FS_TRY2(call) do { hipError_t _s = (call); if (_s != hipSuccess) return drop2(e->fail(HX_E_HIP, std::string(#call) + ": " + hipGetErrorString(_s))); } while (0)
    if (n_listed && small) {
        FS_TRY2(clk.begin());
        hipLaunchKernelGGL(k_fs_scatter, dim3((n_wt + FS_WAVES - 1) / FS_WAVES), dim3(FS_THREADS), (size_t)FS_WAVES * L * 4, e->stream, d_labels, n, L, nbits, wrows, n_wt,
                           scan, row0, ids, n_listed);
        FS_TRY2(hipGetLastError());
        clk.launches++;
        FS_TRY2(clk.end());
    } else if (n_listed) {                                      // the listed rows stand first in the sorted values
        FS_TRY2(hipMemcpyAsync(ids, vals2, n_listed * 4, hipMemcpyDeviceToDevice, e->stream));
        FS_TRY2(hipStreamSynchronize(e->stream));
    }
#undef FS_TRY2
#undef FS_TRY
#undef FS_MEM
    *seg = ids; *d_off = doff;
    return HX_OK;
}

int fs_check_create(hx_engine *e, uint64_t first_row, uint64_t n_rows, uint32_t n_filters, const void *src, hx_filterset **out, const char *what)
{
    if (!e) return HX_E_ARG;
    if (!out) return e->fail(HX_E_ARG, "NULL out");
    if (!src && n_rows > 0) return e->fail(HX_E_ARG, std::string("NULL ") + what + " with n_rows > 0");
    if (n_filters == 0 || n_filters > HX_FILTERSET_MAX_FILTERS) return e->fail(HX_E_ARG, "n_filters must be in [1, HX_FILTERSET_MAX_FILTERS]");
    if (first_row > e->n_rows || n_rows > e->n_rows - first_row) return e->fail(HX_E_ARG, "row range past the stored rows");
    if (first_row + n_rows > 0xFFFFFFFFull) return e->fail(HX_E_ARG, "row range past 2^32 - 1");
    return HX_OK;
}

hx_filterset *fs_new(hx_engine *e, uint64_t first_row, uint64_t n_rows, uint32_t n_filters, uint32_t *d_ids, uint64_t *d_off, std::vector<uint64_t> &off)
{
    hx_filterset *s = new hx_filterset();
    s->e = e; s->first_row = first_row; s->n_rows = n_rows; s->n_filters = n_filters; s->d_ids = d_ids; s->d_off = d_off; s->off.swap(off);
    e->sets.push_back(s);
    return s;
}

int fs_create_labels(hx_engine *e, uint64_t first_row, uint64_t n_rows, uint32_t n_filters, const uint32_t *labels, bool on_device, hx_filterset **out)
{
    int rc = fs_check_create(e, first_row, n_rows, n_filters, labels, out, "labels");
    if (rc) return rc;
    HX_HIP(e, hipSetDevice(e->device));
    FsTmp tmp; FsClock clk{e};
    const uint32_t *d_labels = labels;
    if (n_rows && on_device) HX_HIP(e, hipDeviceSynchronize());   // the column was produced on a stream this library does not know
    if (n_rows && !on_device) {
        uint32_t *up = nullptr;
        FS_NOMEM(e, tmp.get(&up, n_rows * 4));
        HX_HIP(e, hipMemcpyAsync(up, labels, n_rows * 4, hipMemcpyHostToDevice, e->stream));
        d_labels = up;
    }
    uint32_t *ids = nullptr; uint64_t *d_off = nullptr; std::vector<uint64_t> off;
    if ((rc = fs_partition(e, clk, d_labels, n_rows, (uint32_t)first_row, n_filters, &ids, &d_off, off))) return rc;
    clk.book(n_rows);
    *out = fs_new(e, first_row, n_rows, n_filters, ids, d_off, off);
    return HX_OK;
}

int fs_live(const hx_filterset *s)                             // a set call's own checks of its set
{
    if (!s) return HX_E_ARG;
    if (!s->e) return HX_E_STATE;
    if (!s->valid) return s->e->fail(HX_E_STATE, "the filter set lost covered rows to hx_pop_rows");
    return HX_OK;
}

} // namespace

int hx_filterset_usable(hx_engine *e, const hx_filterset *s)
{
    if (!s) return e->fail(HX_E_ARG, "NULL filter set");
    if (s->e != e) return e->fail(HX_E_ARG, "the filter set belongs to another engine");
    if (!s->valid) return e->fail(HX_E_STATE, "the filter set lost covered rows to hx_pop_rows");
    return HX_OK;
}

int hx_filterset_localize(hx_engine *e, const hx_filterset *s, uint32_t nq, const int32_t *filter_of, std::vector<int32_t> &local_of,
                          uint32_t set_f[HX_EXACT_MAX_FILTERS], uint32_t *n_distinct)
{
    *n_distinct = 0; local_of.clear();
    if (!filter_of) return HX_OK;
    std::vector<uint32_t> seen;
    for (uint32_t i = 0; i < nq; i++) {
        const int32_t f = filter_of[i];
        if (f < -1 || (f >= 0 && (uint32_t)f >= s->n_filters)) return e->fail(HX_E_ARG, "filter_of entry outside [-1, n_filters)");
        if (f >= 0) seen.push_back((uint32_t)f);
    }
    std::sort(seen.begin(), seen.end());
    seen.erase(std::unique(seen.begin(), seen.end()), seen.end());
    if (seen.size() > HX_EXACT_MAX_FILTERS) return e->fail(HX_E_ARG, "more than HX_EXACT_MAX_FILTERS distinct filters in one call");
    std::copy(seen.begin(), seen.end(), set_f);
    *n_distinct = (uint32_t)seen.size();
    local_of.resize(nq);
    for (uint32_t i = 0; i < nq; i++)
        local_of[i] = filter_of[i] < 0 ? -1 : (int32_t)(std::lower_bound(seen.begin(), seen.end(), (uint32_t)filter_of[i]) - seen.begin());
    return HX_OK;
}

void hx_filterset_engine_gone(hx_engine *e)
{
    for (hx_filterset *s : e->sets) {
        if (s->d_ids) (void)hipFree(s->d_ids);
        if (s->d_off) (void)hipFree(s->d_off);
        s->d_ids = nullptr; s->d_off = nullptr; s->e = nullptr; s->valid = false;
    }
    e->sets.clear();
}

// =================================================================================================
// C ABI
// =================================================================================================
extern "C" int hx_filterset_create_labels(hx_engine *e, uint64_t first_row, uint64_t n_rows, uint32_t n_filters, const uint32_t *labels_host, hx_filterset **out)
{
    return fs_create_labels(e, first_row, n_rows, n_filters, labels_host, false, out);
}

extern "C" int hx_filterset_create_labels_device(hx_engine *e, uint64_t first_row, uint64_t n_rows, uint32_t n_filters, const uint32_t *labels_dev,
                                                 hx_filterset **out)
{
    return fs_create_labels(e, first_row, n_rows, n_filters, labels_dev, true, out);
}

extern "C" int hx_filterset_create_bitmaps(hx_engine *e, uint64_t first_row, uint64_t n_rows, uint32_t n_filters, const uint64_t *const *filters,
                                           hx_filterset **out)
{
    int rc = fs_check_create(e, first_row, n_rows, n_filters, filters, out, "filters");
    if (rc) return rc;
    const uint64_t n_words = (n_rows + 63) / 64;
    auto word = [&](const uint64_t *w, uint64_t i) { return i == n_words - 1 && (n_rows & 63) ? w[i] & ((1ull << (n_rows & 63)) - 1) : w[i]; };
    std::vector<uint64_t> off((size_t)n_filters + 1, 0);
    std::vector<uint32_t> live;                                // the bitmaps that pass a row
    for (uint32_t f = 0; f < n_filters; f++) {
        uint64_t c = 0;
        if (n_rows && filters[f])
            for (uint64_t w = 0; w < n_words; w++) c += (uint64_t)__builtin_popcountll(word(filters[f], w));
        off[f + 1] = off[f] + c;
        if (c) live.push_back(f);
    }
    const uint64_t n_listed = off[n_filters];
    HX_HIP(e, hipSetDevice(e->device));
    FsTmp tmp; FsClock clk{e};
    // staging of a chunk: its bitmaps and per-word offsets, at most HX_EXACT_MAX_FILTERS bitmaps and about 64 MiB
    const uint32_t chunk = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(HX_EXACT_MAX_FILTERS, (64ull << 20) / std::max<uint64_t>(1, n_words * 12)));
    uint64_t *d_words = nullptr; uint32_t *d_woff = nullptr;
    uint32_t *ids = nullptr; uint64_t *d_off = nullptr;
    if (!live.empty()) {
        FS_NOMEM(e, tmp.get(&d_words, (size_t)chunk * n_words * 8));
        FS_NOMEM(e, tmp.get(&d_woff, (size_t)chunk * n_words * 4));
    }
    FS_NOMEM(e, tmp.get(&ids, std::max<uint64_t>(n_listed, 4) * 4));
    FS_NOMEM(e, tmp.get(&d_off, ((size_t)n_filters + 1) * 8));
    HX_HIP(e, hipMemcpyAsync(d_off, off.data(), ((size_t)n_filters + 1) * 8, hipMemcpyHostToDevice, e->stream));
    std::vector<uint32_t> woff((size_t)std::min<size_t>(chunk, live.size()) * n_words);
    for (size_t c0 = 0; c0 < live.size(); c0 += chunk) {
        const uint32_t nc = (uint32_t)std::min<size_t>(chunk, live.size() - c0);
        uint64_t base[HX_EXACT_MAX_FILTERS];
        for (uint32_t c = 0; c < nc; c++) {
            const uint64_t *w = filters[live[c0 + c]];
            uint32_t *wo = woff.data() + (size_t)c * n_words; uint64_t at = 0;
            for (uint64_t i = 0; i < n_words; i++) { wo[i] = (uint32_t)at; at += (uint64_t)__builtin_popcountll(word(w, i)); }
            base[c] = off[live[c0 + c]];
            HX_HIP(e, hipMemcpyAsync(d_words + (size_t)c * n_words, w, n_words * 8, hipMemcpyHostToDevice, e->stream));
        }
        HX_HIP(e, hipMemcpyAsync(d_woff, woff.data(), (size_t)nc * n_words * 4, hipMemcpyHostToDevice, e->stream));
        HX_HIP(e, clk.begin());
        HX_HIP(e, hx_range_compact_lists(e, d_words, d_woff, n_words, n_rows, (uint32_t)first_row, ids, base, nc));
        clk.launches++;
        HX_HIP(e, clk.end());                                  // the staging and woff are free again
    }
    HX_HIP(e, hipStreamSynchronize(e->stream));
    clk.book(n_listed);
    tmp.p.erase(std::remove_if(tmp.p.begin(), tmp.p.end(), [&](void *q) { return q == ids || q == d_off; }), tmp.p.end());   // the set keeps them
    *out = fs_new(e, first_row, n_rows, n_filters, ids, d_off, off);
    return HX_OK;
}

extern "C" int hx_filterset_append_labels(hx_filterset *s, uint64_t n, const uint32_t *labels_host)
{
    int rc = fs_live(s);
    if (rc) return rc;
    hx_engine *e = s->e;
    if (!labels_host && n > 0) return e->fail(HX_E_ARG, "NULL labels with n > 0");
    const uint64_t at = s->first_row + s->n_rows;
    if (n > e->n_rows - at) return e->fail(HX_E_ARG, "row range past the stored rows");
    if (at + n > 0xFFFFFFFFull) return e->fail(HX_E_ARG, "row range past 2^32 - 1");
    if (n == 0) return HX_OK;
    HX_HIP(e, hipSetDevice(e->device));
    const uint32_t L = s->n_filters;
    FsTmp tmp; FsClock clk{e};
    uint32_t *up = nullptr;
    FS_NOMEM(e, tmp.get(&up, n * 4));
    HX_HIP(e, hipMemcpyAsync(up, labels_host, n * 4, hipMemcpyHostToDevice, e->stream));
    uint32_t *seg = nullptr; uint64_t *d_seg_off = nullptr; std::vector<uint64_t> seg_off;
    if ((rc = fs_partition(e, clk, up, n, (uint32_t)at, L, &seg, &d_seg_off, seg_off))) return rc;   // a bad label: the set is as it was
    tmp.p.push_back(seg); tmp.p.push_back(d_seg_off);
    std::vector<uint64_t> new_off((size_t)L + 1);
    for (uint32_t l = 0; l <= L; l++) new_off[l] = s->off[l] + seg_off[l];
    const uint64_t total = new_off[L];
    uint32_t *ids = nullptr; uint64_t *d_off = nullptr;
    FS_NOMEM(e, tmp.get(&ids, std::max<uint64_t>(total, 4) * 4));
    FS_NOMEM(e, tmp.get(&d_off, ((size_t)L + 1) * 8));
    HX_HIP(e, hipMemcpyAsync(d_off, new_off.data(), ((size_t)L + 1) * 8, hipMemcpyHostToDevice, e->stream));
    if (total) {
        HX_HIP(e, clk.begin());
        hipLaunchKernelGGL(k_fs_concat, dim3((uint32_t)((total + 255) / 256)), dim3(256), 0, e->stream, (const uint32_t *)s->d_ids, (const uint64_t *)s->d_off,
                           (const uint32_t *)seg, (const uint64_t *)d_seg_off, (const uint64_t *)d_off, L, ids, total);
        HX_HIP(e, hipGetLastError());
        clk.launches++;
        HX_HIP(e, clk.end());
    }
    HX_HIP(e, hipStreamSynchronize(e->stream));
    clk.book(n);
    for (void *&q : tmp.p) {                                   // the new arrays become the set's, the old ones go with the temporaries
        if (q == ids) q = s->d_ids;
        else if (q == d_off) q = s->d_off;
    }
    s->d_ids = ids; s->d_off = d_off; s->off.swap(new_off); s->n_rows += n;
    return HX_OK;
}

extern "C" int hx_filterset_info(const hx_filterset *s, uint64_t *first_row, uint64_t *n_rows, uint32_t *n_filters, uint64_t *n_listed)
{
    if (!s) return HX_E_ARG;
    if (first_row) *first_row = s->first_row;
    if (n_rows) *n_rows = s->n_rows;
    if (n_filters) *n_filters = s->n_filters;
    if (n_listed) *n_listed = s->off.empty() ? 0 : s->off.back();
    return HX_OK;
}

extern "C" int hx_filterset_counts(const hx_filterset *s, uint32_t first, uint32_t n, uint64_t *counts_out)
{
    int rc = fs_live(s);
    if (rc) return rc;
    if (first > s->n_filters || n > s->n_filters - first) return s->e->fail(HX_E_ARG, "filter range past n_filters");
    if (!counts_out && n > 0) return s->e->fail(HX_E_ARG, "NULL output");
    for (uint32_t i = 0; i < n; i++) counts_out[i] = s->off[(size_t)first + i + 1] - s->off[(size_t)first + i];
    return HX_OK;
}

extern "C" int hx_filterset_read(hx_filterset *s, uint32_t filter, uint64_t cap, uint32_t *ids_out, uint64_t *n_out)
{
    int rc = fs_live(s);
    if (rc) return rc;
    hx_engine *e = s->e;
    if (filter >= s->n_filters) return e->fail(HX_E_ARG, "filter past n_filters");
    if (!n_out || (!ids_out && cap > 0)) return e->fail(HX_E_ARG, "NULL output");
    const uint64_t n = s->off[(size_t)filter + 1] - s->off[filter];
    *n_out = n;
    if (n > cap) return e->fail(HX_E_NOMEM, "capacity exceeded");
    if (!n) return HX_OK;
    HX_HIP(e, hipSetDevice(e->device));
    HX_HIP(e, hipMemcpyAsync(ids_out, s->d_ids + s->off[filter], n * 4, hipMemcpyDeviceToHost, e->stream));
    HX_HIP(e, hipStreamSynchronize(e->stream));
    return HX_OK;
}

extern "C" int hx_filterset_destroy(hx_filterset *s)
{
    if (!s) return HX_E_ARG;
    if (hx_engine *e = s->e) {
        (void)hipSetDevice(e->device);
        (void)hipStreamSynchronize(e->stream);
        if (s->d_ids) (void)hipFree(s->d_ids);
        if (s->d_off) (void)hipFree(s->d_off);
        e->sets.erase(std::remove(e->sets.begin(), e->sets.end(), s), e->sets.end());
    }
    delete s;
    return HX_OK;
}
