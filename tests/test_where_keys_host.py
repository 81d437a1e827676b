"""The mapping of a distance predicate `value <cmp> radius` onto the returned f32 distance (hx_internal.h: hx_where_keys, hx_where_keys32 -- what
hx_index_search_filtered hands its traversal kernel, and hx_where_keys alone what hx_exact_range hands its scan), on the host: for every comparison,
both kinds of value ((double)d, and sqrt((double)d) of `<->` on an HX_L2SQ index) and radii at every edge of float8 and f32, the interval [k0, k1]
contains hx_order_key32(d, root) exactly when PostgreSQL's float8 comparison of the operator's value with the radius holds.  The model is written
from that comparison (float8_cmp_internal: NaN equals NaN and is above everything, -0.0 == +0.0) and never touches an order key.  Also: K(k), on whose
monotonicity the two binary searches rest, never decreases.  Compiled for the host only; needs hipcc, no GPU."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")

SRC = r"""
#include "hx_internal.h"
#include <algorithm>
#include <cfloat>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

static float f32_of(uint32_t b) { float f; memcpy(&f, &b, 4); return f; }
static uint32_t bits_of(float f) { uint32_t b; memcpy(&b, &f, 4); return b; }

// PostgreSQL float8_cmp_internal
static int f8cmp(double a, double b)
{
    if (std::isnan(a)) return std::isnan(b) ? 0 : 1;
    if (std::isnan(b)) return -1;
    return a > b ? 1 : a < b ? -1 : 0;
}
// the operator function's float8 result of the f32 distance d
static double value_of(float d, bool root)
{
    if (!root) return (double)d;
    if (d < 0.0f) return NAN;
    return std::sqrt((double)d);
}
static bool model(int cmp, bool root, double radius, float d)
{
    const int c = f8cmp(value_of(d, root), radius);
    return cmp == HX_CMP_LT ? c < 0 : cmp == HX_CMP_LE ? c <= 0 : cmp == HX_CMP_GT ? c > 0 : c >= 0;
}

// the f32 values around v: the rounding of v and `n` neighbours on each side
static void around(double v, int n, std::vector<float> &out)
{
    if (std::isnan(v)) return;
    const float c = (float)v;
    out.push_back(c);
    float a = c, b = c;
    for (int i = 0; i < n; i++) { a = nextafterf(a, -INFINITY); b = nextafterf(b, INFINITY); out.push_back(a); out.push_back(b); }
}

int main()
{
    std::mt19937_64 g(20240917);
    const double D_DENORM = 4.9406564584124654e-324, F_DENORM = (double)f32_of(1u);
    std::vector<double> radii = {0.0, -0.0, INFINITY, -INFINITY, NAN, -NAN, D_DENORM, -D_DENORM, 2 * D_DENORM, F_DENORM, -F_DENORM, F_DENORM / 2, F_DENORM * 1.5,
                                 (double)FLT_MIN, -(double)FLT_MIN, nextafter((double)FLT_MIN, 0.0), (double)FLT_MAX, -(double)FLT_MAX,
                                 nextafter((double)FLT_MAX, INFINITY), nextafter(-(double)FLT_MAX, -INFINITY), 0x1p128, -0x1p128, 1e39, -1e39, 1e300, -1e300, DBL_MAX, -DBL_MAX,
                                 std::sqrt((double)FLT_MAX), nextafter(std::sqrt((double)FLT_MAX), INFINITY), 0x1p64, nextafter(0x1p64, INFINITY), 1e200,
                                 -1.0, -0.5, -3.25, -1e-30, -1e30, -7.0, 1.0, 0.5, 2.0, 0.1, 1e-3, 1e3};
    std::vector<double> root_radii;                                // radii that matter for `root`: around the roots of f32 values
    for (int i = 0; i < 200; i++) {
        const uint32_t e = (uint32_t)(i * 255 / 200);              // every exponent from the subnormals to the largest finite one
        const uint32_t b = ((uint32_t)(g() & 1) << 31) | (e << 23) | (uint32_t)(g() & 0x7FFFFF);
        const float x = f32_of(b);
        const double dx = (double)x;
        radii.push_back(dx);
        const float dn = nextafterf(x, -INFINITY), up = nextafterf(x, INFINITY);
        if (std::isfinite(dn)) radii.push_back((dx + (double)dn) / 2);
        if (std::isfinite(up)) radii.push_back((dx + (double)up) / 2);
        radii.push_back(nextafter(dx, -INFINITY));
        radii.push_back(nextafter(dx, INFINITY));
        const double s = std::sqrt(std::fabs(dx));
        root_radii.push_back(s); root_radii.push_back(nextafter(s, -INFINITY)); root_radii.push_back(nextafter(s, INFINITY));
    }
    radii.insert(radii.end(), root_radii.begin(), root_radii.end());

    std::vector<float> common = {0.0f, -0.0f, INFINITY, -INFINITY, FLT_MIN, -FLT_MIN, nextafterf(FLT_MIN, 0.0f), -nextafterf(FLT_MIN, 0.0f),
                                 nextafterf(FLT_MIN, 1.0f), -nextafterf(FLT_MIN, 1.0f), f32_of(1u), f32_of(0x80000001u), f32_of(2u), f32_of(0x80000002u),
                                 FLT_MAX, -FLT_MAX, nextafterf(FLT_MAX, 0.0f), -nextafterf(FLT_MAX, 0.0f), 1.0f, -1.0f,
                                 f32_of(0x7FC00000u), f32_of(0xFFC00000u), f32_of(0x7F800001u), f32_of(0xFF800001u), f32_of(0x7FFFFFFFu), f32_of(0xFFFFFFFFu),
                                 f32_of(0x7FA55AA5u), f32_of(0xFFD12345u)};

    long cases = 0, bad = 0, passing = 0, empties = 0;
    std::vector<uint64_t> all_keys;                                // K's domain: the f32 order key without the NaN collapse
    auto raw_key = [](float d) -> uint64_t { const uint32_t b = bits_of(d); return (b >> 31) ? (uint32_t)~b : (b | 0x80000000u); };
    const int cmps[4] = {HX_CMP_LT, HX_CMP_LE, HX_CMP_GT, HX_CMP_GE};
    for (double r : radii) {
        std::vector<float> probes = common;
        around(r, 6, probes);
        around(r * r, 6, probes);
        around(-r, 1, probes);
        for (float d : probes) all_keys.push_back(raw_key(d));
        for (int root = 0; root < 2; root++)
            for (int cmp : cmps) {
                uint64_t lo, hi; uint32_t k[2];
                hx_where_keys(cmp, r, &lo, &hi);
                hx_where_keys32(lo, hi, root != 0, k);
                if (k[0] > k[1]) { empties++; if (k[0] != ~0u || k[1] != 0u) { if (bad < 20) printf("BAD empty cmp %d root %d r %a: {%08x, %08x}\n", cmp, root, r, k[0], k[1]); bad++; } }
                bool any = false;
                for (float d : probes) {
                    const uint32_t key = hx_order_key32(d, root != 0);
                    const bool got = k[0] <= key && key <= k[1], want = model(cmp, root != 0, r, d);
                    // the 64-bit interval is what hx_exact_range and the lock-step driver test against the value itself
                    const uint64_t vk = hx_order_key(value_of(d, root != 0));
                    const bool got64 = lo <= vk && vk <= hi;
                    cases++; passing += want; any = any || want;
                    if (got != want || got64 != want) {
                        if (bad < 20) printf("BAD cmp %d root %d r %a d %a (%08x): kernel %d scan %d model %d  [%08x, %08x]\n", cmp, root, r, (double)d, bits_of(d), got, got64, want, k[0], k[1]);
                        bad++;
                    }
                }
                // no f32 at all passes (the probes hold both ends of every order): the interval must be the empty one
                const bool none = (cmp == HX_CMP_GT && std::isnan(r)) || (cmp == HX_CMP_LT && !root && r == -INFINITY) || (cmp == HX_CMP_LT && root && f8cmp(r, 0.0) <= 0)
                                  || (cmp == HX_CMP_LE && root && f8cmp(r, 0.0) < 0);
                if (none && (any || k[0] != ~0u || k[1] != 0u)) { if (bad < 20) printf("BAD not empty cmp %d root %d r %a: {%08x, %08x}\n", cmp, root, r, k[0], k[1]); bad++; }
            }
    }
    // K never decreases over the keys the searches visit: [key of 0, NaN] with root, [key of -inf, NaN] without
    for (int i = 0; i < 4000; i++) all_keys.push_back(g() & 0xFFFFFFFFull);
    std::sort(all_keys.begin(), all_keys.end());
    all_keys.erase(std::unique(all_keys.begin(), all_keys.end()), all_keys.end());
    long mono = 0;
    for (int root = 0; root < 2; root++) {
        const uint64_t kmin = root ? 0x80000000ull : 0x007FFFFFull;
        uint64_t prev = 0; bool have = false;
        for (uint64_t k : all_keys) {
            if (k < kmin) continue;
            const uint64_t v = hx_where_value_key(k, root != 0);
            if (have && v < prev) { if (bad < 20) printf("BAD K decreases at key %08llx root %d\n", (unsigned long long)k, root); bad++; }
            prev = v; have = true; mono++;
        }
    }
    printf("cases %ld bad %ld passing %ld empties %ld radii %zu monotone_keys %ld\n", cases, bad, passing, empties, radii.size(), mono);
    return bad ? 1 : 0;
}
"""


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
def test_key_interval_contains_exactly_the_distances_whose_value_passes_the_float8_comparison(tmp_path):
    src = tmp_path / "wk.hip"
    src.write_text(SRC)
    exe = tmp_path / "wk"
    subprocess.run([HIPCC, "--offload-arch=gfx950", "--offload-host-only", "-O2", "-std=c++17", "-ffp-contract=off", "-fno-fast-math",
                    "-I", os.path.join(ROOT, "pgvector-rx_amd", "csrc"), "-x", "hip", str(src), "-o", str(exe)], check=True, capture_output=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    f = out.stdout.split("\n")[-2].split()
    res = dict(zip(f[0::2], map(int, f[1::2])))
    assert res["bad"] == 0
    assert res["cases"] > 100000                                    # (cmp, root, radius, probe)
    assert 0 < res["passing"] < res["cases"] and res["empties"] > 0   # both answers occur, and so does the empty interval
    assert res["radii"] > 1500 and res["monotone_keys"] > 4000
