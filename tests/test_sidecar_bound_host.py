"""The sidecar bound of include-free header code (hx_ops.h: hx_l2_lb, hx_l2_lb_finish) on the host: for every (query, row) pair, LB never exceeds
the canonical f32 squared L2 distance -- 64 lanes, each summing its 16-byte fragments of every 1 KiB chunk in order with rounded multiplies and
adds, then the xor butterfly 32, 16, 8, 4, 2, 1 (hx_fused_core.h: f_dist_batch) -- on clustered and adversarial rows.  Compiled for the host only;
needs hipcc, no GPU."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")

SRC = r"""
#include "hx_ops.h"
#include <cstdio>
#include <random>
#include <vector>

static float canon(const std::vector<float> &q, const std::vector<float> &x, uint32_t nw)   // nw: f32 words of the pitch (zeros past dim)
{
    float v[64];
    const uint32_t nch = (nw * 4 + 1023) / 1024;
    for (uint32_t l = 0; l < 64; l++) {
        float acc = 0.0f;
        for (uint32_t c = 0; c < nch; c++)
            for (uint32_t t = 0; t < 4; t++) {
                const uint32_t i = c * 256 + l * 4 + t;
                const float a = i < q.size() ? q[i] : 0.0f, b = i < x.size() ? x[i] : 0.0f;
                if (i < nw) { const float d = a - b; const float dd = d * d; acc = acc + dd; }
            }
        v[l] = acc;
    }
    for (uint32_t off = 32; off >= 1; off >>= 1) {
        float w[64];
        for (uint32_t l = 0; l < 64; l++) w[l] = v[l] + v[l ^ off];
        for (uint32_t l = 0; l < 64; l++) v[l] = w[l];
    }
    return v[0];
}

// the encoder of hx_sidecar.hip (k_sc_encode), sequentially
static void encode(const std::vector<float> &x, std::vector<uint8_t> &c, float meta[3])
{
    const uint32_t dim = (uint32_t)x.size();
    float lo = INFINITY, hi = -INFINITY; bool ok = true;
    for (float v : x) { ok = ok && std::isfinite(v); lo = fminf(lo, v); hi = fmaxf(hi, v); }
    const float step = ok ? (hi - lo) / 255.0f : 0.0f;
    ok = ok && std::isfinite(step);
    c.assign(dim, 0);
    double err = 0.0; bool fx = true;
    for (uint32_t i = 0; i < dim; i++) {
        uint32_t k = 0;
        if (ok && step > 0.0f) { const float t = rintf((x[i] - lo) / step); k = t >= 255.0f ? 255u : t > 0.0f ? (uint32_t)t : 0u; }
        c[i] = (uint8_t)k;
        const float xh = fmaf(step, (float)k, lo);
        fx = fx && std::isfinite(xh);
        const double dd = (double)x[i] - (double)xh; err += dd * dd;
    }
    ok = ok && fx;
    const double e = sqrt(err) * (1.0 + 0x1p-40);
    float ex = (float)e;
    if ((double)ex < e) ex = nextafterf(ex, INFINITY);
    if (!ok || !std::isfinite(ex)) ex = INFINITY;
    meta[0] = ok ? lo : 0.0f; meta[1] = step; meta[2] = ex;
}

static std::vector<std::vector<float>> rows_for(uint32_t dim, std::mt19937 &g)
{
    std::uniform_real_distribution<float> U(0.0f, 1.0f); std::normal_distribution<float> N(0.0f, 1.0f);
    std::vector<std::vector<float>> R;
    std::vector<float> centre(dim); for (auto &v : centre) v = U(g);
    for (int r = 0; r < 40; r++) { std::vector<float> x(dim); for (uint32_t i = 0; i < dim; i++) x[i] = centre[i] + 0.1f * N(g); R.push_back(x); }
    const float big = 3.402823466e+38f / (float)dim / 4.0f;
    auto fill = [&](auto f) { std::vector<float> x(dim); for (uint32_t i = 0; i < dim; i++) x[i] = f(i); R.push_back(x); };
    fill([&](uint32_t) { return 0.5f; });                                   // constant
    fill([&](uint32_t) { return 0.0f; });
    fill([&](uint32_t) { return N(g) * big; });                             // near FLT_MAX / dim
    fill([&](uint32_t) { return U(g) * 1e-40f; });                          // subnormals
    fill([&](uint32_t i) { return i == dim / 2 ? 1e30f : 0.25f; });         // one huge coordinate
    fill([&](uint32_t) { return U(g) * 1e-20f; });
    fill([&](uint32_t) { return -3.0e38f; });
    fill([&](uint32_t i) { return i == 0 ? INFINITY : 0.5f; });             // non-finite
    return R;
}

int main()
{
    const uint32_t dims[] = {1, 3, 100, 129, 255, 256, 767, 768, 769, 1024, 2000};
    std::mt19937 g(7);
    long pairs = 0, bad = 0, useful = 0;
    for (uint32_t dim : dims) {
        const uint32_t nw = (uint32_t)(((size_t)dim * 4 + 15) / 16 * 4);
        const auto R = rows_for(dim, g);
        std::vector<std::vector<uint8_t>> C(R.size()); std::vector<float> M(3 * R.size());
        for (size_t r = 0; r < R.size(); r++) encode(R[r], C[r], &M[3 * r]);
        std::vector<std::vector<float>> Q = R;
        for (size_t r = 0; r < 5; r++) { auto q = R[r]; for (auto &v : q) v += 1e-3f; Q.push_back(q); }
        for (const auto &q : Q)
            for (size_t r = 0; r < R.size(); r++) {
                const float lb = hx_l2_lb(q.data(), C[r].data(), &M[3 * r], dim, nw);
                const float d = canon(q, R[r], nw);
                pairs++;
                const bool ok = std::isfinite(lb) && lb >= 0.0f && (std::isnan(d) ? lb == 0.0f : lb <= d);
                if (!ok) { if (bad < 10) printf("BAD dim %u row %zu lb %.9g d %.9g\n", dim, r, lb, d); bad++; }
                if (r < 40 && d > 0.0f && lb > 0.9f * d) useful++;
            }
    }
    printf("pairs %ld bad %ld useful %ld\n", pairs, bad, useful);
    return bad ? 1 : 0;
}
"""


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
def test_lower_bound_never_exceeds_canonical_distance(tmp_path):
    src = tmp_path / "lb.hip"
    src.write_text(SRC)
    exe = tmp_path / "lb"
    subprocess.run([HIPCC, "--offload-arch=gfx950", "--offload-host-only", "-O2", "-std=c++17", "-ffp-contract=off", "-fno-fast-math",
                    "-I", os.path.join(ROOT, "pgvector-rx_amd", "csrc"), "-x", "hip", str(src), "-o", str(exe)], check=True, capture_output=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    _, pairs, _, bad, _, useful = out.stdout.split("\n")[-2].split()
    assert int(bad) == 0 and int(pairs) > 5000 and int(useful) > 0
