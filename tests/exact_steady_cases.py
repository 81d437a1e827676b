"""The case table of the steady-state tests of the exact top-k scans: tests/test_exact_steady_plan.py proves on the CPU, with the plan code of
pgvector-rx_amd/csrc/hx_exact_plan.h itself, that every call is in the regime it claims, and tests/test_gpu_exact_steady.py runs the same calls on
the device against the oracle.  No GPU, no engine and no oracle is needed to import this module.

The regime.  A scan is *steady* when every slice but the last holds per >= 4 * cap rows (cap: the per-(query, slice) candidate buffer, the power
of two >= max(2k, k + R), R rows per round): the buffer is full after at most a quarter of the slice, so at least three quarters of the rows are
compared against a live threshold -- the running k-th (key, id) -- and the buffer is cut back to k again and again inside the round loop.  A merge
is *steady* when the slices are full (per >= k) and S * k >= 2 * cap2, so that it filters against its own threshold from the third chunk on.

Plain calls (hx_exact_search) reach the regime by many rows or many queries: S = min(1024 / tiles, n_pass / 4R), so per >= 4 * cap needs
nq * n_pass >= Q * 1024 * 4 * cap pairs whatever the shape.  Grouped calls (hx_exact_search_filtered / hx_exact_search_set with two or more
distinct filters) run under HX_EXACT_SCRATCH = SCRATCH bytes, where ex_plan gives every tile one slice: a filter with 4 * cap passing rows is steady.
"""
F32, F16, BIT, SPARSE = 0, 1, 2, 3                     # hx_dtype
L2, IP, COS, L1, HAM, JAC = 0, 1, 2, 3, 4, 5           # hx_op: <-> <#> <=> <+> <~> <%>
OP_NAME = {L2: "l2", IP: "ip", COS: "cos", L1: "l1", HAM: "hamming", JAC: "jaccard"}
FOPS, BOPS = (L2, IP, COS, L1), (HAM, JAC)
SCRATCH = 64                                           # HX_EXACT_SCRATCH of the grouped calls, bytes: one slice per tile, one tile per block
SPARSE_MAX_NNZ = 1000

SCAN, MERGE = "scan", "merge"


def pitch(dtype, dim):
    """bytes per stored row"""
    if dtype == SPARSE:
        return (16 + 8 * min(dim, SPARSE_MAX_NNZ) + 15) & ~15
    raw = {F32: 4 * dim, F16: 2 * dim, BIT: (dim + 7) // 8}[dtype]
    return (raw + 15) & ~15


def P(nq, n_rows, ks, first_row=0, first_query=0, n_pass=None):
    """A plain call: nq queries from slot first_query over rows [first_row, first_row + n_rows); n_pass: through a bitmap that passes that many
    of them (random), None: the plain range.  ks: {k: the stages claimed steady, a subset of (SCAN, MERGE)}."""
    return dict(nq=nq, n_rows=n_rows, ks=ks, first_row=first_row, first_query=first_query, n_pass=n_pass)


def G(n_rows, groups, ks, unfiltered=0, first_row=0, first_query=0):
    """A grouped call: groups = [(queries, passing rows)] -- one filter each --, `unfiltered` queries without a filter; the queries of the groups
    are interleaved.  ks: {k: the tile sizes (16, 4, 1) whose scans are claimed steady}."""
    return dict(n_rows=n_rows, groups=groups, ks=ks, unfiltered=unfiltered, first_row=first_row, first_query=first_query)


def case(name, dtype, dim, ops, plain=(), grouped=(), data="random", lanes=None, **flags):
    """data: "random"; "improving" / "worsening": the rows sorted so that the value to query 0 (and to query 9, its copy) falls / rises with the
    row id; "ties": rows of {0, -1} (bit: at most 3 bits of the first 16) so that thousands of rows share the k-th value; "zeros": all rows zero
    vectors but seven; "late": the queries near one far point and the rows late[0] .. late[1] - 1 around it.  lanes: lanes per row the case is
    about (64: pitch > 128, 8: pitch <= 128), checked by the plan test."""
    c = dict(name=name, dtype=dtype, dim=dim, ops=tuple(ops), plain=list(plain), grouped=list(grouped), data=data, lanes=lanes,
             sidecar=False, scan_only=False, max_nnz=0)
    c.update(flags)
    return c


K10 = {10: (SCAN,)}
ALL3 = {10: (16, 4, 1)}
# tiles of 16 | 4 | 1 on the plain path at 64 lanes per row (R = 8 | 16 | 16, cap = 64 at k <= 10) and at 8 lanes (R = 64 | 128 | 128, cap = 128 | 256 | 256)
P64_16, P64_4, P64_1 = P(256, 16384, K10), P(12, 90000, K10), P(3, 90000, K10)
P8_16, P8_4, P8_1 = P(256, 32768, K10), P(12, 360000, K10), P(3, 360000, K10)
# groups of 21 = 16 + 4 + 1 and 7 = 4 + 3 queries and two unfiltered ones (a partial tile of 4)
G64 = G(700, [(21, 400), (7, 300)], ALL3, unfiltered=2)
G8 = G(3000, [(21, 1500), (7, 1100)], ALL3, unfiltered=2)

CASES = [
    # ---- 1. operator x type at 64 lanes per row ------------------------------------------------------------------------------------------
    # <->: the k sweep (k = 100 on the plain path: tiles of 1 over 350 300 rows, 342 slices of 1025 rows -- its merge is steady too) and the
    # windows (first_row > 0, first_query > 0, a partial last tile)
    case("f32x33-l2", F32, 33, [L2], lanes=64,
         plain=[P(256, 16384, {10: (SCAN,), 1: (SCAN,)}), P64_4, P(3, 350300, {10: (SCAN,), 100: (SCAN, MERGE), 1: (SCAN,)}),
                P(250, 16384, K10, first_row=1000, first_query=5)],
         grouped=[G64, G(2600, [(21, 1500), (7, 1100)], {100: (16, 4, 1), 1: (16, 4, 1)}, unfiltered=2, first_row=37, first_query=3)]),
    case("f32x33", F32, 33, [IP, COS, L1], lanes=64, plain=[P64_16, P64_4, P64_1], grouped=[G64]),
    case("f16x72", F16, 72, FOPS, lanes=64, plain=[P64_16, P64_4, P64_1], grouped=[G64]),
    case("bit1100", BIT, 1100, BOPS, lanes=64, plain=[P64_16, P64_4, P64_1], grouped=[G64]),
    # 4096 < pitch <= 16384: at most 4 queries fit the LDS, a group of 64 is 16 tiles of 4.  A steady plain call needs nq * n * dim >= 10^9
    # oracle operations at this width, so the shape runs on the grouped path
    case("f32x1100", F32, 1100, FOPS, lanes=64, grouped=[G(600, [(64, 300), (3, 280), (1, 270)], {10: (4, 1)})]),
    # pitch > 16384: tiles of 1 only, and at k = 1024 (not steady: it would take 8192 rows of 41 200 B) more than 64 KiB of dynamic LDS
    case("f32x10300", F32, 10300, [L2], lanes=64, scan_only=True, grouped=[G(700, [(2, 400), (1, 300)], {10: (1,), 1024: ()})]),
    # ---- 2. the same at 8 lanes per row -------------------------------------------------------------------------------------------------
    case("f32x4", F32, 4, FOPS, lanes=8, plain=[P8_16], grouped=[G8]),
    case("f16x8", F16, 8, FOPS, lanes=8, plain=[P8_16], grouped=[G8]),
    case("bit128", BIT, 128, BOPS, lanes=8, plain=[P8_16], grouped=[G8]),
    # tiles of 4 and 1; <-> with the k sweep and, at k = 1024, the steady merge of 342 full slices (171 chunks)
    case("f32x4-long", F32, 4, [L2], lanes=8,
         plain=[P8_4, P(3, 360000, {10: (SCAN,), 100: (SCAN, MERGE), 1: (SCAN,), 1024: (MERGE,)})],
         grouped=[G(3000, [(21, 1500), (7, 1100)], {100: (16, 4, 1), 1: (16, 4, 1)}, unfiltered=2),
                  G(9000, [(5, 8300), (1, 8200)], {1024: (4, 1)})]),                        # k = 1024: cap = 2048, one slice of >= 8192 rows
    case("bit128-long", BIT, 128, [HAM], lanes=8, plain=[P8_4, P8_1]),
    # ---- 3. sparsevec: one lane per (query, row), R = 256, cap = 512 -------------------------------------------------------------------
    case("sparse100000", SPARSE, 100000, FOPS, max_nnz=40, plain=[P(256, 8200, K10)], grouped=[G(5000, [(3, 2600), (2, 2100)], {10: (1,)}, unfiltered=1)]),
    case("sparse1e9", SPARSE, 10 ** 9, FOPS, max_nnz=1000, grouped=[G(2600, [(2, 2300), (1, 2100)], {10: (1,)})]),
    # ---- 4. row orders --------------------------------------------------------------------------------------------------------------------
    case("f32x33-improving", F32, 33, [L2], lanes=64, data="improving", plain=[P64_16], grouped=[G64]),
    case("f32x33-worsening", F32, 33, [L2], lanes=64, data="worsening", plain=[P64_16], grouped=[G64]),
    case("f32x4-improving", F32, 4, [L2], lanes=8, data="improving", plain=[P8_16], grouped=[G8]),
    case("f32x4-worsening", F32, 4, [L2], lanes=8, data="worsening", plain=[P8_16], grouped=[G8]),
    case("bit1100-improving", BIT, 1100, [HAM], lanes=64, data="improving", plain=[P64_16], grouped=[G64]),
    case("bit1100-worsening", BIT, 1100, [HAM], lanes=64, data="worsening", plain=[P64_16], grouped=[G64]),
    # every query's k nearest rows stand together in the later half of one slice, in no order: each meets the threshold of the ones before it,
    # where a row that is exactly the k-th so far must still get in (with neighbours spread over many slices it is the best of its slice)
    case("f32x33-late", F32, 33, [L2], lanes=64, data="late", late=(16256, 16368), plain=[P64_16, P64_4, P64_1]),
    case("f32x4-late", F32, 4, [L2], lanes=8, data="late", late=(32512, 32768), plain=[P8_16]),
    # ---- 5. ties under a live threshold: the plain range and a bitmap, whose compacted id list is in no order ----------------------------
    case("f32x33-ties", F32, 33, [L2, IP], lanes=64, data="ties", plain=[P64_16, P(256, 20000, K10, n_pass=16384)], grouped=[G64]),
    # ... and in a steady merge: 342 full slices at k = 100, 17 chunks against a threshold that thousands of entries tie with, again through a
    # bitmap -- over the plain range a later slice holds larger ids only, and the id of a tying entry never decides
    case("bit128-ties", BIT, 128, BOPS, lanes=8, data="ties",
         plain=[P8_16, P(256, 40000, K10, n_pass=32768), P(3, 400000, {100: (SCAN, MERGE)}, n_pass=360000)], grouped=[G8]),
    case("f32x33-zeros", F32, 33, [COS], lanes=64, data="zeros", plain=[P64_16, P(256, 20000, K10, n_pass=16384)], grouped=[G64]),
    # ---- 7. the sidecar kernel (<-> on f32 rows that keep the 8-bit copy; tiles of 4 and 1), rows in improving order -------------------
    # dim 768 in tiles of 1 only: any steady call in tiles of 4 needs 4 * 262 144 * 768 = 8 * 10^8 oracle operations
    case("f32x132-sidecar", F32, 132, [L2], lanes=64, data="improving", sidecar=True, plain=[P64_4, P64_1]),
    case("f32x768-sidecar", F32, 768, [L2], lanes=64, data="improving", sidecar=True, plain=[P64_1]),
]

BY_NAME = {c["name"]: c for c in CASES}
PLAIN = [(c["name"], op) for c in CASES if c["plain"] for op in c["ops"]]
GROUPED = [(c["name"], op) for c in CASES if c["grouped"] for op in c["ops"]]


def case_id(v):
    return OP_NAME[v] if isinstance(v, int) else str(v)


def rows_needed(c, calls):
    return max(call["first_row"] + call["n_rows"] for call in calls)


def queries_needed(c, calls):
    return max(call["first_query"] + (call["nq"] if "nq" in call else sum(g[0] for g in call["groups"]) + call["unfiltered"]) for call in calls)
