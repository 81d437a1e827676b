"""pgvector-rx_amd: MI355X-native HNSW distance engine for pgvector-rx's hot path.

The product is the C-ABI shared library built from csrc/ (include/hnswrx.h).  This Python package is
thin ctypes plumbing over that ABI for tests, bench.py and the multi-GPU (torch.distributed / RCCL)
driver; it contains no arithmetic of its own and has no CPU fallback.
"""
from .binding import (  # noqa: F401
    BIT, F16, F32, HAMMING, JACCARD, L1, L2SQ, NEG_IP, QUERY_SLOT, SPARSE,
    EXACT_MAX_FILTERS, EXACT_MAX_K, OP_COSINE, OP_HAMMING, OP_JACCARD, OP_L1, OP_L2, OP_NEG_IP,
    CMP_GE, CMP_GT, CMP_LE, CMP_LT, RANGE_BY_DISTANCE, RANGE_BY_ROW, CREATE_SCAN_ONLY, CREATE_NO_SIDECAR, CREATE_SCAN_SIDECAR, E_RANGE, SCAN_MAX_FILTERS, SCAN_STOP_PAST_RADIUS,
    E_ARG, E_NOMEM, E_STATE, FILTERSET_MAX_FILTERS, NO_LABEL, FilterSet,
    Engine, HxError, Index, lib, lib_path, pack_sparse, sparse_record_bytes,
)
from .levels import batch_schedule, draw_levels, max_level  # noqa: F401
