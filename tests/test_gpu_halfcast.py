"""hx_append_rows_halfvec / hx_set_queries_halfvec: `embedding::halfvec(n)` on the device, checked bit for bit against the oracle's restatement of
f32_to_half (halfvec.rs:92-143), and the reference's range error (halfvec.rs:665) leaving the destination untouched."""
import ctypes

import numpy as np
import pytest

import pgvector_rx_amd as hx
from oracle import orc

E_ARG, E_DIM, E_STATE, E_RANGE = -1, -2, -6, -7


def orc_half(bits):
    """orc_f32_to_half of each f32 bit pattern.  A NaN goes in as a ctypes float holding its bits: through a Python float its payload would be
    quieted on the way (f32 -> f64 -> f32)."""
    f = orc.lib().orc_f32_to_half
    bits = np.asarray(bits, np.uint32)
    vals = bits.view(np.float32)
    nan = np.isnan(vals)
    return np.fromiter((f(ctypes.c_float.from_buffer_copy(b.tobytes())) if isn else f(float(v)) for b, v, isn in zip(bits, vals, nan)),
                       np.uint16, len(vals))


def overflows(bits, half):
    """finite input whose half is +-inf: the reference's `rt.is_infinite() && !val.is_infinite()`"""
    return ((half & 0x7FFF) == 0x7C00) & ((np.asarray(bits, np.uint32) & 0x7FFFFFFF) != 0x7F800000)


def cast_rows(vals, dim):
    """device cast of a flat f32 array, as rows of `dim` (zero padded); returns the halves"""
    n = (len(vals) + dim - 1) // dim
    rows = np.zeros(n * dim, np.float32)
    rows[:len(vals)] = vals
    src = hx.Engine(hx.F32, hx.L2SQ, dim, n)
    src.append(rows.reshape(n, dim))
    dst = hx.Engine(hx.F16, hx.L2SQ, dim, n)
    assert dst.append_halfvec_from(src, 0, n) == 0 and dst.num_rows == n
    out = dst.read_rows(0, n).reshape(-1)[:len(vals)]
    src.close()
    dst.close()
    return out


@pytest.mark.gpu
def test_cast_bits_all_exponents():
    hi = np.arange(1 << 19, dtype=np.uint32) << 13                        # every sign / exponent / upper-mantissa pattern
    bits = np.concatenate([hi | low for low in (0, 1, 0xFFF, 0x1000, 0x1001, 0x1FFF)])
    want = orc_half(bits)
    keep = ~overflows(bits, want)
    bits, want = bits[keep], want[keep]
    got = cast_rows(bits.view(np.float32), 1024)
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, [(hex(int(bits[i])), hex(int(got[i])), hex(int(want[i]))) for i in bad[:8]]


@pytest.mark.gpu
def test_cast_special_values():
    f = np.float32
    band = np.linspace(2.0 ** -25, 2.0 ** -24, 37).astype(f)             # (2^-25, 2^-24): zero, not the smallest denormal
    vals = np.concatenate([np.array([0.0, -0.0, np.inf, -np.inf, 65504.0, 65519.996, -65519.996, 2.0 ** -24, 2.0 ** -25, 6.1e-5], f),
                           band, -band,
                           np.array([0x7FC00000, 0x7F800001, 0xFF800FFF, 0x7FFFE000, 0x7FA5A5A5, 0xFFC00001], np.uint32).view(f)])
    want = orc_half(vals.view(np.uint32))
    assert not overflows(vals.view(np.uint32), want).any()
    got = cast_rows(vals, 13)                                             # a pitch with padding
    assert (got == want).all(), [(v, hex(int(a)), hex(int(b))) for v, a, b in zip(vals, got, want) if a != b]
    assert got[2] == 0x7C00 and got[3] == 0xFC00 and ((got[10:10 + len(band)] & 0x7FFF) <= 1).all()


@pytest.mark.gpu
def test_queries_and_normalize():
    rng = np.random.default_rng(5)
    dim = 300
    rows = (rng.standard_normal((40, dim)) * 50).astype(np.float32)
    qs = (rng.standard_normal((7, dim)) * 50).astype(np.float32)
    src = hx.Engine(hx.F32, hx.L2SQ, dim, 40)
    src.append(rows)
    src.set_queries(qs)
    dst = hx.Engine(hx.F16, hx.L2SQ, dim, 40)
    dst.append_halfvec_from(src)
    host = orc_half(qs.view(np.uint32).ravel()).reshape(qs.shape)
    assert (dst.read_rows(0, 7) == orc_half(rows[:7].view(np.uint32).ravel()).reshape(7, dim)).all()
    # query casts: equal to the row casts (read back through a row store), and normalize equals hx_set_queries(normalize=True) of them
    assert dst.set_queries_halfvec_from(src) == 7
    ids = np.arange(40, dtype=np.uint32)
    a = dst.exact_search(hx.OP_L2, 5)
    dst2 = hx.Engine(hx.F16, hx.L2SQ, dim, 40)
    dst2.append_halfvec_from(src)
    dst2.set_queries(host)
    b = dst2.exact_search(hx.OP_L2, 5)
    assert all((x.view(np.uint8) == y.view(np.uint8)).all() for x, y in zip(a, b))
    dst.set_queries_halfvec_from(src, normalize=True)
    dst2.set_queries(host, normalize=True)
    a, b = dst.exact_search(hx.OP_NEG_IP, 40), dst2.exact_search(hx.OP_NEG_IP, 40)
    assert all((x.view(np.uint8) == y.view(np.uint8)).all() for x, y in zip(a, b))
    assert (dst.distances(host[0], ids) == dst2.distances(host[0], ids)).all()
    # a query set larger than the destination's slots grows them
    src.set_queries(np.tile(qs, (20, 1)))
    assert dst.set_queries_halfvec_from(src) == 140
    dst2.set_queries(host)
    a, b = dst.exact_search(hx.OP_L2, 3, first_query=133, nq=7), dst2.exact_search(hx.OP_L2, 3)
    assert all((x.view(np.uint8) == y.view(np.uint8)).all() for x, y in zip(a, b))
    for e in (src, dst, dst2):
        e.close()


@pytest.mark.gpu
def test_range_error_changes_nothing():
    dim = 20
    rows = np.ones((6, dim), np.float32)
    src = hx.Engine(hx.F32, hx.L2SQ, dim, 6)
    src.append(rows)
    src.set_queries(rows[:2])
    dst = hx.Engine(hx.F16, hx.L2SQ, dim, 16)
    dst.append_halfvec_from(src, 0, 2)
    dst.set_queries_halfvec_from(src)
    before_rows, before_q = dst.read_rows(0, 2), dst.exact_search(hx.OP_L1, 2)
    for bad, shown in ((65520.0, '"65520" is out of range for type halfvec'), (-1e6, '"-1000000" is out of range for type halfvec')):
        r = rows.copy()
        r[4, 7] = bad
        r[5, 3] = bad                                                      # the first offending row is named
        s2 = hx.Engine(hx.F32, hx.L2SQ, dim, 6)
        s2.append(r)
        with pytest.raises(hx.HxError) as ei:
            dst.append_halfvec_from(s2, 1, 5)
        assert ei.value.code == E_RANGE and shown in str(ei.value) and "row 4" in str(ei.value) and "element 7" in str(ei.value)
        assert dst.num_rows == 2 and (dst.read_rows(0, 2) == before_rows).all()
        s2.set_queries(r[3:6])
        with pytest.raises(hx.HxError) as ei:
            dst.set_queries_halfvec_from(s2)
        assert ei.value.code == E_RANGE and shown in str(ei.value) and "query slot 1" in str(ei.value)
        after = dst.exact_search(hx.OP_L1, 2, nq=2)
        assert all((x.view(np.uint8) == y.view(np.uint8)).all() for x, y in zip(before_q, after))
        s2.close()
    r = rows.copy()
    r[0, 0], r[1, 1] = np.inf, -np.inf                                     # infinities are not errors
    s3 = hx.Engine(hx.F32, hx.L2SQ, dim, 6)
    s3.append(r)
    assert dst.append_halfvec_from(s3, 0, 2) == 2
    got = dst.read_rows(2, 2)
    assert got[0, 0] == 0x7C00 and got[1, 1] == 0xFC00
    for e in (src, dst, s3):
        e.close()


@pytest.mark.gpu
def test_argument_errors_and_busy_slot():
    import torch
    rng = np.random.default_rng(8)
    n, dim = 2000, 16
    rows = rng.random((n, dim), dtype=np.float32)
    src = hx.Engine(hx.F32, hx.L2SQ, dim, n)
    src.append(rows)
    src.set_queries(rows[:4])
    L = hx.lib()
    other = hx.Engine(hx.F16, hx.L2SQ, dim + 1, 10)
    assert L.hx_append_rows_halfvec(other.h, src.h, 0, 1, None) == E_DIM and b"expected 17 dimensions, not 16" in L.hx_last_error(other.h)
    assert L.hx_set_queries_halfvec(other.h, src.h, 0) == E_DIM
    f32 = hx.Engine(hx.F32, hx.L2SQ, dim, 10)
    assert L.hx_append_rows_halfvec(f32.h, src.h, 0, 1, None) == E_ARG                                  # dst must be halfvec
    h16 = hx.Engine(hx.F16, hx.L2SQ, dim, n)
    assert L.hx_append_rows_halfvec(h16.h, h16.h, 0, 0, None) == E_ARG                                  # src must be vector
    assert L.hx_set_queries_halfvec(h16.h, None, 0) == E_ARG
    assert L.hx_append_rows_halfvec(h16.h, src.h, n - 1, 2, None) == E_ARG                              # past the source rows
    assert L.hx_append_rows_halfvec(f32.h, src.h, 0, 1, None) == E_ARG
    small = hx.Engine(hx.F16, hx.L2SQ, dim, 3)
    assert L.hx_append_rows_halfvec(small.h, src.h, 0, 4, None) == -3 and small.num_rows == 0
    if torch.cuda.device_count() > 1:                                                                  # device mismatch
        far = hx.Engine(hx.F16, hx.L2SQ, dim, 10, device=1)
        assert L.hx_append_rows_halfvec(far.h, src.h, 0, 1, None) == E_ARG
        far.close()
    # a busy pipelined scan slot of dst refuses both casts; afterwards they work
    h16.append_halfvec_from(src)
    h16.set_queries_halfvec_from(src)
    h16.set_timing(True)
    h16.kernel_stats(10, reset=True)
    ix = hx.Index(h16, 8, 32)
    ix.insert(0, hx.draw_levels(n, 8, seed=3), batch=256)
    alone = ix.search(4, 40, 10)
    ix.search_submit(0, 0, 4, 40, 10)
    assert L.hx_set_queries_halfvec(h16.h, src.h, 0) == E_STATE
    assert L.hx_append_rows_halfvec(h16.h, src.h, 0, 1, None) == E_STATE
    waited = ix.search_wait(0)
    assert all((a == b).all() for a, b in zip(alone, waited))
    assert h16.set_queries_halfvec_from(src) == 4
    st = h16.kernel_stats(10)
    assert st["units"] == 4 * dim and st["launches"] == 1 and st["ms"] > 0
    ix.close()
    for e in (src, other, f32, h16, small):
        e.close()
