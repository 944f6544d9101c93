"""ctypes binding of librdx.so (include/rdx.h). There is no CPU fallback: a missing or unloadable
library, or a machine without a gfx950 GPU, raises RdxUnavailable as soon as the hot path is used."""
from __future__ import annotations

import ctypes
import os

# torch bundles its own libamdhip64 (same soname as ROCm's): import it first so that librdx and
# torch.distributed/RCCL share ONE HIP runtime in the process.
import torch  # noqa: F401  (plumbing only: device tensors, streams, torch.distributed)

_HERE = os.path.dirname(os.path.abspath(__file__))
# RDX_LIB_PATH: developer override (tools/ab_bench.sh points a run at a variant build WITHOUT touching the product file)
LIB_PATH = os.environ.get("RDX_LIB_PATH") or os.path.join(_HERE, "librdx.so")

RDX_OK, RDX_ERR_INVALID, RDX_ERR_HIP, RDX_ERR_NOMEM, RDX_ERR_STATE = 0, 1, 2, 3, 4
RDX_HOST, RDX_DEVICE = 0, 1
ABI_VERSION = 3          # include/rdx.h RDX_ABI_VERSION
PACKED_FLAGS = 4         # include/rdx.h RDX_PACKED_FLAGS: int32 words behind the counts of a packed partial
RERANK_FEATURES = 8      # include/rdx.h RDX_RERANK_WORKSPACE_BYTES: output features per head workgroup
# the postfix filter programs of rdx_docs_set_query and rdx_meta_set_query (where_document.py and where_device.py compile them):
OP_NOT, OP_AND, OP_OR = -1, -2, -3   # include/rdx.h RDX_DOCS_OP_* = RDX_META_OP_*
MAX_OPS, MAX_STACK = 4096, 16        # include/rdx.h: at most 4096 ops and 16 stack entries
DOCS_OP_NOT, DOCS_OP_AND, DOCS_OP_OR = OP_NOT, OP_AND, OP_OR
DOCS_MAX_LEAVES = 1024   # include/rdx.h RDX_DOCS_MAX_LEAVES
META_MAX_COLUMNS = 4096   # include/rdx.h RDX_META_MAX_COLUMNS (leaf ops and the leaf limit: rag_dpo_amd/where_device.py)
SPACE_IP, SPACE_L2 = 0, 1   # include/rdx.h RDX_SPACE_*
SPACE_MAX_CAND, SPACE_MAX_PAGE_QUERIES = 4096, 64   # include/rdx.h rdx_space_rescore's / rdx_space_distances' limits
FUSE_MAX_LISTS, FUSE_MAX_LIST_ENTRIES, FUSE_MAX_ENTRIES = 16, 512, 1024   # include/rdx.h RDX_FUSE_MAX_*: rdx_fuse_rankings' limits
FUSE_DENSE, FUSE_BM25 = 0, 1   # include/rdx.h RDX_FUSE_DENSE / RDX_FUSE_BM25
GROUP_MAX_K, GROUP_MAX_GROUPS, GROUP_MAX_SIZE, GROUP_FILL_SPAN = 4096, 64, 16, 4096   # include/rdx.h RDX_GROUP_*: the grouped search's limits
MMR_MAX_FETCH, MMR_MAX_K = 1024, 64   # include/rdx.h RDX_MMR_MAX_*: rdx_index_mmr's limits
RANGE_MAX_RESULTS = 1024   # include/rdx.h RDX_RANGE_MAX_RESULTS: rdx_index_range's limit
KMEANS_MAX_CLUSTERS, KMEANS_MAX_ITER = 4096, 1000   # include/rdx.h RDX_KMEANS_MAX_*: rdx_index_kmeans' limits
FACET_MAX_LIMIT = 1024   # include/rdx.h RDX_FACET_MAX_LIMIT: rdx_index_range_facets' limit
TOPIC_MAX_N, TOPIC_MAX_TOPICS, TOPIC_MAX_TAGS, TOPIC_MAX_DIM = 1024, 32, 64, 4096   # include/rdx.h rdx_topic_boost's limits
# include/rdx.h RDX_RERANK_BATCH_MAX_ROWS / _MAX_QUESTIONS / RDX_RERANK_SELECT_WIDTHS: the batched reranker calls' limits, and the workgroup
# widths rdx_rerank_select_batch chooses among (the smallest that holds the call's longest segment)
RERANK_BATCH_MAX_ROWS, RERANK_BATCH_MAX_QUESTIONS, RERANK_SELECT_WIDTHS = 1 << 20, 65535, (64, 256, 1024)
# include/rdx.h RDX_MAXSIM_MAX_*: rdx_maxsim_f16's limits (token vectors per question and per slot, dim, pairs per call)
MAXSIM_MAX_Q_TOKENS, MAXSIM_MAX_SLOT_TOKENS, MAXSIM_MAX_DIM, MAXSIM_MAX_PAIRS = 256, 8192, 1024, 1 << 20
LEX_MAX_TOKENS, LEX_MAX_SKIP = 8192, 8   # include/rdx.h RDX_LEX_MAX_*: rdx_lex_reduce's limits (tokens per text, skip ids)


def topic_pair(topic: int, tag: int, exact: bool) -> int:
    """include/rdx.h RDX_TOPIC_PAIR"""
    return (tag << 8) | (128 if exact else 0) | (topic & 31)


class RdxUnavailable(RuntimeError):
    """The HIP library is not built/loadable or no gfx950 device is visible."""


class RdxError(RuntimeError):
    pass


class SearchStats(ctypes.Structure):
    _fields_ = [
        ("nq", ctypes.c_int64), ("k", ctypes.c_int64), ("rows", ctypes.c_int64),
        ("sample_rows", ctypes.c_int64), ("emitted", ctypes.c_int64), ("rescored", ctypes.c_int64),
        ("exact_queries", ctypes.c_int64), ("path", ctypes.c_int32), ("profiled", ctypes.c_int32),
        ("ms_normalize", ctypes.c_float), ("ms_scan_sample", ctypes.c_float), ("ms_tau", ctypes.c_float),
        ("ms_scan_main", ctypes.c_float), ("ms_refine", ctypes.c_float), ("ms_exact", ctypes.c_float),
        ("ms_total", ctypes.c_float),
        ("scan_main_launch_rows", ctypes.c_int64), ("scan_main_launch_queries", ctypes.c_int64),
        ("retried_queries", ctypes.c_int64),
        ("xcd_finish_spread_ms", ctypes.c_float), ("xcd_share_min", ctypes.c_float), ("xcd_share_max", ctypes.c_float),
        ("tau_rank", ctypes.c_float),
    ]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


_lib = None

# every symbol include/rdx.h declares: (restype, argtypes)
_vp, _i, _i64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64
SYMBOLS = {
    "rdx_version": (_i, []),
    "rdx_last_error": (ctypes.c_char_p, []),
    "rdx_device_count": (_i, [ctypes.POINTER(_i)]),
    "rdx_set_wait_policy": (_i, [_i, _i]),
    "rdx_index_create": (_i, [_i, _i, ctypes.POINTER(_vp)]),
    "rdx_index_destroy": (_i, [_vp]),
    "rdx_index_dim": (_i, [_vp, ctypes.POINTER(_i)]),
    "rdx_index_count": (_i, [_vp, ctypes.POINTER(_i64)]),
    "rdx_index_reserve": (_i, [_vp, _i64]),
    "rdx_index_add": (_i, [_vp, _vp, _i64, _i]),
    "rdx_index_add_bf16": (_i, [_vp, _vp, _i64, _i]),
    "rdx_index_add_stored": (_i, [_vp, _vp, _i64, _i]),
    "rdx_index_update": (_i, [_vp, _vp, _vp, _i64, _i]),
    "rdx_index_update_stored": (_i, [_vp, _vp, _vp, _i64, _i]),
    "rdx_index_get": (_i, [_vp, _vp, _i64, _vp, _i]),
    "rdx_index_compact": (_i, [_vp, _vp, _i64]),
    "rdx_index_set_row_ids": (_i, [_vp, _i64, _vp, _i64, _i]),
    "rdx_index_set_option": (_i, [_vp, ctypes.c_char_p, _i64]),
    "rdx_index_xcd_shares": (_i, [_vp, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double)]),
    "rdx_l2_normalize": (_i, [_i, _vp, _i64, _i, _vp, _i, _vp]),
    "rdx_enc_attention_f16": (_i, [_i, _vp, _vp, _vp, _i64, _i, _i, ctypes.c_float, _i, _vp, _vp]),
    "rdx_enc_attention_mfma_f16": (_i, [_i, _vp, _vp, _i, _i, _i, ctypes.c_float, _vp, _vp]),
    "rdx_enc_gelu_f16": (_i, [_i, _vp, ctypes.c_int64, _vp]),
    "rdx_enc_linear_small_f16": (_i, [_i, _vp, _vp, _vp, _i, _i, _i, _i, _vp, _vp]),
    "rdx_enc_add_layernorm_f16": (_i, [_i, _vp, _vp, _vp, _vp, ctypes.c_float, _i64, _i, _vp, _vp]),
    "rdx_enc_embed_f16": (_i, [_i, _vp, _vp, _vp, _vp, _vp, _i, _i, _vp, _vp]),
    "rdx_enc_stage_f16": (_i, [_i, _vp, _vp, _vp, _vp, ctypes.c_float, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _vp, _vp]),
    "rdx_enc_attention_small_f16": (_i, [_i, _vp, _vp, _i, _i, _i, ctypes.c_float, _vp, _vp]),
    "rdx_enc_layernorm_rows_f16": (_i, [_i, _vp, _vp, _vp, ctypes.c_float, _i, _i, _vp, _vp]),
    "rdx_enc_gemm_f16": (_i, [_i, _vp, _vp, _vp, _vp, _i64, _i, _i, _i, _vp, _vp]),
    "rdx_enc_layernorm_f16": (_i, [_i, _vp, _vp, _vp, ctypes.c_float, _i64, _i, _vp, _vp]),
    "rdx_rerank_head_f16": (_i, [_i, _vp, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "rdx_rerank_select": (_i, [_i, _vp, _vp, _i, _i, ctypes.c_double, _i, _vp, _vp, _vp, _vp]),
    "rdx_topic_boost": (_i, [_i, _vp, _i64, _i, _vp, _i, _vp, _i, _vp, _vp, _i64, _i, ctypes.c_double, ctypes.c_double, _vp, _vp, _vp, _vp]),
    "rdx_rerank_head_rows_f16": (_i, [_i, _vp, _i64, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "rdx_topic_boost_batch": (_i, [_i, _vp, _i64, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, ctypes.c_double, ctypes.c_double,
                                   _vp, _vp, _vp, _vp]),
    "rdx_rerank_select_batch": (_i, [_i, _vp, _vp, _i, _vp, _i, ctypes.c_double, _i, _vp, _vp, _vp, _vp, _vp]),
    "rdx_maxsim_f16": (_i, [_i, _vp, _vp, _i, _vp, _i64, _vp, _vp, _i64, _vp, _vp, _i64, _i, _vp, _vp]),
    "rdx_maxsim_quantize_i8": (_i, [_i, _vp, _i64, _i, _vp, _vp, _vp]),
    "rdx_maxsim_i8": (_i, [_i, _vp, _vp, _vp, _i, _vp, _vp, _i64, _vp, _vp, _i64, _vp, _vp, _i64, _i, _vp, _vp]),
    "rdx_search": (_i, [_vp, _vp, _i64, _i, _vp, _vp, _vp, _vp, _i, _vp]),
    "rdx_mask_create": (_i, [_vp, _vp, _i, ctypes.POINTER(_vp)]),
    "rdx_mask_destroy": (_i, [_vp]),
    "rdx_search_masked": (_i, [_vp, _vp, _i64, _i, _vp, _vp, _vp, _vp, _i, _vp]),
    "rdx_search_filtered": (_i, [_vp, _vp, _i64, _i, _vp, ctypes.c_int32, _vp, _vp, _vp, _vp, _i, _vp]),
    "rdx_search_async": (_i, [_vp, _vp, _i64, _i, _vp, _vp, _vp, _vp, _vp, _vp]),
    "rdx_search_wait": (_i, [_vp, ctypes.POINTER(_i)]),
    "rdx_merge_topk": (_i, [_i, _vp, _vp, _vp, _i, _i64, _i, _vp, _vp, _vp, _i, _vp]),
    "rdx_signal_create": (_i, [_i, ctypes.POINTER(_vp)]),
    "rdx_signal_destroy": (_i, [_vp]),
    "rdx_signal_wait": (_i, [_vp, _vp, ctypes.POINTER(ctypes.c_int32)]),
    "rdx_merge_topk_packed": (_i, [_i, _vp, _i64, _i, _i64, _i, _vp, _vp, _vp, _vp, _vp]),
    "rdx_search_last_stats": (_i, [_vp, ctypes.POINTER(SearchStats)]),
    "rdx_search_last_coarse_bits": (_i, [_vp, ctypes.POINTER(ctypes.c_int32)]),
    "rdx_bm25_create": (_i, [_i, _i64, _i64, _vp, _vp, _vp, _vp, _vp, _vp, ctypes.c_int32, ctypes.POINTER(_vp)]),
    "rdx_bm25_destroy": (_i, [_vp]),
    "rdx_bm25_search": (_i, [_vp, _vp, _vp, _i64, _i, _vp, _vp, _vp, _vp, _i, _vp]),
    "rdx_bm25_search_filtered": (_i, [_vp, _vp, _vp, _i64, _i, _vp, ctypes.c_int32, _vp, _vp, _vp, _vp, _i, _vp]),
    "rdx_lex_reduce": (_i, [_i, _vp, _vp, _i64, _vp, _i64, _i, _vp, _i, _vp, _vp, _vp, _vp]),
    "rdx_lex_create": (_i, [_i, _i64, _i64, _vp, _vp, _vp, _vp, ctypes.c_int32, ctypes.POINTER(_vp)]),
    "rdx_lex_destroy": (_i, [_vp]),
    "rdx_lex_search": (_i, [_vp, _vp, _vp, _vp, _i64, _i, _vp, ctypes.c_int32, _vp, _vp, _vp, _vp, _i, _vp]),
    "rdx_lex_score_pairs": (_i, [_vp, _vp, _vp, _vp, _i64, _vp, _vp, _i64, _vp, _vp]),
    "rdx_bm25_build_create": (_i, [_i, _i64, ctypes.c_uint64, ctypes.POINTER(_vp)]),
    "rdx_bm25_build_destroy": (_i, [_vp]),
    "rdx_bm25_build_tokenize": (_i, [_vp, _vp, _i64, _vp, _i64, _i64, _vp, _i64, _vp, _vp]),
    "rdx_bm25_build_stats": (_i, [_vp, ctypes.POINTER(_i64), ctypes.POINTER(_i64), ctypes.POINTER(ctypes.c_int32)]),
    "rdx_bm25_build_first_pos": (_i, [_vp, _vp, _i64, _vp]),
    "rdx_bm25_build_vocab": (_i, [_vp, _vp, _i64, _vp, _vp, _i64, _vp]),
    "rdx_docs_create": (_i, [_i, ctypes.POINTER(_vp)]),
    "rdx_docs_destroy": (_i, [_vp]),
    "rdx_docs_append": (_i, [_vp, _vp, _vp, _i64]),
    "rdx_docs_replace": (_i, [_vp, _vp, _vp, _vp, _i64]),
    "rdx_docs_compact": (_i, [_vp, _vp, _i64]),
    "rdx_docs_stats": (_i, [_vp, ctypes.POINTER(_i64), ctypes.POINTER(_i64), ctypes.POINTER(_i64)]),
    "rdx_docs_set_query": (_i, [_vp, _vp, _vp, _i, _vp, _i]),
    "rdx_docs_contains": (_i, [_vp, _vp, _i, _vp]),
    "rdx_docs_filter": (_i, [_vp, _vp, _vp, _i, _vp]),
    "rdx_meta_create": (_i, [_i, ctypes.POINTER(_vp)]),
    "rdx_meta_destroy": (_i, [_vp]),
    "rdx_meta_set_rows": (_i, [_vp, _i, _i64, _vp, _vp, _vp, _i64]),
    "rdx_meta_drop_column": (_i, [_vp, _i]),
    "rdx_meta_truncate": (_i, [_vp, _i64]),
    "rdx_meta_stats": (_i, [_vp, ctypes.POINTER(_i64), ctypes.POINTER(_i64)]),
    "rdx_meta_set_query": (_i, [_vp, _vp, _i, _vp, _i]),
    "rdx_meta_filter": (_i, [_vp, _i64, _vp, _vp, _i, _vp]),
    "rdx_space_measure": (_i, [_i, _i, _vp, _i64, _i, _vp, _vp, _vp]),
    "rdx_space_lift": (_i, [_i, _i, _i, _vp, _i64, _i, _i, _vp, _vp, _vp]),
    "rdx_space_rescore": (_i, [_i, _i, _vp, _i64, _i, _vp, _vp, _vp, _vp, _i, _i, _i, ctypes.c_double, _vp, _vp, _vp, _vp, _vp, _vp]),
    "rdx_space_distances": (_i, [_i, _i, _vp, _i, _i, _vp, _i64, _i, _vp, _i64, _vp, _i64, _vp]),
    "rdx_fuse_rankings": (_i, [_i, _i64, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _vp, _vp, _i, _i, _i, _i, _i,
                               _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _vp]),
    "rdx_group_select": (_i, [_i, _vp, _vp, _vp, _i64, _i, _vp, _i64, _vp, _i64, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "rdx_index_group_fill": (_i, [_vp, _vp, _i64, _vp, _vp, _vp, _vp, _i64, _vp, _i64, _i, _vp, _vp, _vp, _vp]),
    "rdx_index_mmr": (_i, [_vp, _vp, _vp, _vp, _i64, _i, _i, ctypes.c_double, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "rdx_index_range": (_i, [_vp, _vp, _i64, _vp, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "rdx_index_near_dup": (_i, [_vp, ctypes.c_float, _vp, _i, _i64, _vp, _vp, _vp, _vp]),
    "rdx_index_kmeans": (_i, [_vp, _vp, _i, _i, _vp, _vp, _vp, _vp, _vp, ctypes.POINTER(ctypes.c_int32), _vp]),
    "rdx_index_facet_count": (_i, [_vp, _vp, _vp, _i64, _vp, ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int64), _vp]),
    "rdx_index_range_facets": (_i, [_vp, _vp, _i64, _vp, _vp, _vp, _i64, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "rdx_index_score_pairs": (_i, [_vp, _vp, _i64, _vp, _vp, _i64, _vp, _vp]),
    "rdx_m3_combine": (_i, [_i, _vp, _vp, _vp, _i64, ctypes.c_double, ctypes.c_double, ctypes.c_double, _vp, _vp, _vp]),
}


def load(require_gpu: bool = True):
    """Load librdx.so. Raises RdxUnavailable (never falls back) when it cannot serve the hot path."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RdxUnavailable(
                f"{LIB_PATH} is missing: build it with `python -m rag_dpo_amd.build` "
                "(hipcc --offload-arch=gfx950). There is no CPU fallback for the retrieval hot path.")
        try:
            L = ctypes.CDLL(LIB_PATH)
        except OSError as e:
            raise RdxUnavailable(f"cannot load {LIB_PATH}: {e}") from e
        for name, (res, args) in SYMBOLS.items():
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        if L.rdx_version() != ABI_VERSION:
            raise RdxUnavailable(f"librdx ABI version {L.rdx_version()} != {ABI_VERSION}: rebuild the library")
        _lib = L
    if require_gpu:
        n = ctypes.c_int(0)
        rc = _lib.rdx_device_count(ctypes.byref(n))
        if rc != RDX_OK or n.value < 1:
            raise RdxUnavailable("no HIP device visible: the retrieval hot path needs an MI355X (gfx950) GPU; "
                                 "there is no CPU fallback. " + last_error())
    return _lib


def last_error() -> str:
    if _lib is None:
        return ""
    return (_lib.rdx_last_error() or b"").decode("utf-8", "replace")


def check(rc: int):
    if rc == RDX_OK:
        return
    msg = last_error()
    if rc == RDX_ERR_INVALID:
        raise ValueError(msg)
    if rc == RDX_ERR_NOMEM:
        raise MemoryError(msg)
    raise RdxError(f"librdx error {rc}: {msg}")
