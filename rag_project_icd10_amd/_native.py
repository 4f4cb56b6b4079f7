"""ctypes binding of libicdsearch.so (C ABI: include/icd_search.h).

This is the only place the product touches native code. There is NO CPU fallback: if the shared
library is missing or the device is not an MI355X (gfx950) the constructors raise.

`IcdIndex` is the MI355X replacement for the Milvus Lite collection the reference opens in
services/milvus_service.py:57-206 and searches at :280-285.
"""
from __future__ import annotations

import ctypes as C
import math
import os
import sys
from typing import Optional

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "csrc", "libicdsearch.so")

MODE_AUTO = 0   # fp16-MFMA coarse pass + certified exact rescoring (+ exact fallback); same results as EXACT
MODE_EXACT = 1  # fp32-MFMA kernel only
MAX_K = 128
ABI_VERSION = 6   # include/icd_search.h ICD_ABI_VERSION: a stale libicdsearch.so is refused with a clear message

EXPORTED_SYMBOLS = (
    "icd_abi_version", "icd_last_error", "icd_device_count", "icd_index_create", "icd_index_create_view", "icd_index_destroy",
    "icd_index_search", "icd_index_search_reweighted", "icd_merge_topk", "icd_index_lookup_levels",
    "icd_index_stats", "icd_index_cert_terms", "icd_index_set_chunks", "icd_index_debug_counters", "icd_index_set_profiling",
    "icd_index_last_profile", "icd_index_profile_summary", "icd_index_set_option", "icd_packed_attention",
    "icd_hier_rescore", "icd_hier_rescore_entities",
    "icd_score_stats",
    "icd_cosine_rows",
    "icd_term_first_match",
    "icd_index_set_second_pass",
    "icd_group_unique_id", "icd_group_create", "icd_group_prepare", "icd_group_connect", "icd_group_search", "icd_group_destroy",
    "icd_unpack_query_slices", "icd_split_bf16x3", "icd_encoder_create", "icd_encoder_encode", "icd_encoder_encode_many", "icd_encoder_destroy", "icd_pack_winners",
    "icd_grouping_create", "icd_grouping_destroy", "icd_grouping_stats", "icd_index_search_grouped",
    "icd_index_search_range",
    "icd_rowmask_create", "icd_rowmask_destroy", "icd_rowmask_stats", "icd_rowmask_pack", "icd_index_search_masked",
    "icd_fusion_create", "icd_fusion_destroy", "icd_fusion_stats", "icd_index_search_hybrid", "icd_fusion_fuse_lists",
    "icd_sparse_tile_rows", "icd_sparse_pack", "icd_sparse_create", "icd_sparse_destroy", "icd_sparse_stats", "icd_sparse_search",
    "icd_grouping_pair_sparse", "icd_sparse_search_grouped", "icd_index_search_hybrid_grouped", "icd_fusion_fuse_lists_grouped",
    "icd_sparse_search_range",
    "icd_sparse_match_rowmasks", "icd_rowmask_read",
    "icd_columns_create", "icd_columns_destroy", "icd_columns_stats", "icd_filter_program_check", "icd_filter_rowmasks",
    "icd_rowmask_select", "icd_rowmask_group_counts",
    "icd_mmr_create", "icd_mmr_destroy", "icd_mmr_stats", "icd_index_search_mmr",
    "icd_boost_create", "icd_boost_destroy", "icd_boost_stats", "icd_index_search_boosted",
    "icd_byrows_create", "icd_byrows_destroy", "icd_byrows_stats", "icd_index_search_by_rows",
    "icd_rankof_create", "icd_rankof_destroy", "icd_rankof_stats", "icd_index_rank_of",
    "icd_wide_create", "icd_wide_destroy", "icd_wide_stats", "icd_index_search_wide",
    "icd_recommend_create", "icd_recommend_destroy", "icd_recommend_stats", "icd_recommend_read_vectors", "icd_index_recommend",
    "icd_grouping_prepare_scorers", "icd_index_search_grouped_scored",
    "icd_grouping_prepare_maxsim", "icd_index_search_maxsim",
)
MAXSIM_SCORERS = {"sum": 1, "mean": 2}   # include/icd_search.h ICD_MAXSIM_*: how an embedding list's per-vector maxima combine
RANKOF_MAX_TARGETS = 16                  # ICD_RANKOF_MAX_TARGETS: targets of one query of a rank-of call
WIDE_MAX_K = 16384                       # ICD_WIDE_MAX_K: first + k of one wide search
RECOMMEND_MAX_EXAMPLES = 16              # ICD_RECOMMEND_MAX_EXAMPLES: positive + negative examples of one request
RECOMMEND_STRATEGIES = {"average_vector": 0, "best_score": 1, "sum_scores": 2}   # ICD_RECOMMEND_*
MAXSIM_MAX_T = 64                        # ICD_MAXSIM_MAX_T: vectors of one list
GROUP_SCORERS = {"max": 0, "sum": 1, "avg": 2}   # include/icd_search.h ICD_GROUP_SCORER_*: what a group of a grouped search ranks by
MAX_BOOSTS = 4   # include/icd_search.h ICD_MAX_BOOSTS: (row mask, weight) pairs per query of a boosted search
SELECT_MAX_LIMIT = 16384   # include/icd_search.h ICD_SELECT_MAX_LIMIT: rows per query of one select_rows call (Milvus's offset + limit window)
SELECT_SEGMENT_ROWS = 16384   # csrc/mask_select_plan.hpp MS_SEG_ROWS: rows of one work-group of the select's two passes
FACET_LDS_GROUPS = 8192   # csrc/facet_count_plan.hpp FC_LDS_GROUPS: groups up to which a facet count sums in LDS (above it: global adds)
SPARSE_MAX_QUERY_TERMS = 64  # include/icd_search.h ICD_SPARSE_MAX_QUERY_TERMS
MAX_REQUESTS = 8   # include/icd_search.h ICD_MAX_REQUESTS: requests per query of a hybrid search
RANKER_RRF, RANKER_WEIGHTED = 0, 1
NORMS = {"none": 0, "cosine": 1, "atan": 2}   # ICD_NORM_*
MAX_K = 128   # include/icd_search.h ICD_MAX_K: the slots of one query's hit list (a grouped search: k * group_size)
# include/icd_search.h: icd_index_create flags and icd_index_set_option ids (A/B and test options of ONE index)
CREATE_CORPUS_ON_DEVICE, CREATE_ROW_ORDER, CREATE_NO_PROBE, CREATE_NO_CENTER = 1, 2, 4, 8
OPTIONS = {"family_order": 1, "stream_one": 2, "host_one": 3, "pacing_shift": 4, "pacing_lead": 5, "exact_narrow": 6, "wide_from": 7}
GROUP_ROW_SHARD = 0
GROUP_QUERY_SHARD = 1
GROUP_ID_BYTES = 128
SPLIT_TAIL = 64   # csrc/attention_kernel.hpp: elements behind [hi | hi | lo] of icd_split_bf16x3's rows


class IcdError(RuntimeError):
    """A libicdsearch call returned a negative icd_status."""

    def __init__(self, code: int, text: str):
        super().__init__(f"libicdsearch error {code}: {text}")
        self.code = code


class _Stats(C.Structure):
    _fields_ = [("n", C.c_int64), ("dim", C.c_int32), ("device", C.c_int32), ("id_base", C.c_int64),
                ("bytes_corpus_f32", C.c_int64), ("bytes_corpus_f16", C.c_int64), ("bytes_workspace", C.c_int64),
                ("max_nq", C.c_int32), ("max_k", C.c_int32), ("fast_path", C.c_int32), ("rmax", C.c_float),
                ("last_nq", C.c_int64), ("last_fallback", C.c_int64), ("last_chunks", C.c_int32),
                ("last_mode", C.c_int32), ("last_second_pass", C.c_int64), ("last_second_pass_lists", C.c_int32),
                ("second_pass_armed", C.c_int32), ("wide_mode", C.c_int32), ("sparse_fallback_armed", C.c_int32),
                ("centered", C.c_int32), ("mean_share", C.c_float)]


_ENC_LAYER_FIELDS = ("w_qkv", "b_qkv", "w_ao", "b_ao", "ln1_g", "ln1_b", "w_up", "b_up", "w_down", "b_down", "ln2_g", "ln2_b")


class _EncoderDesc(C.Structure):   # include/icd_search.h icd_encoder_desc
    _fields_ = ([("layers", C.c_int32), ("hidden", C.c_int32), ("heads", C.c_int32), ("inter", C.c_int32), ("vocab", C.c_int32),
                 ("max_pos", C.c_int32), ("pos_offset", C.c_int32), ("ln_eps", C.c_float),
                 ("word_emb", C.c_void_p), ("pos_emb", C.c_void_p), ("type_emb0", C.c_void_p), ("emb_ln_g", C.c_void_p), ("emb_ln_b", C.c_void_p)]
                + [(name, C.POINTER(C.c_void_p)) for name in _ENC_LAYER_FIELDS] + [("arithmetic", C.c_int32)])


ENCODER_ARITH = {"fp32": 0, "bf16x3": 1}   # include/icd_search.h ICD_ENCODER_ARITH_*
ENCODER_MAX_TOKENS = 512   # include/icd_search.h ICD_ENCODER_MAX_TOKENS
ENCODER_MAX_SEQS = 64      # ... ICD_ENCODER_MAX_SEQS


class _Profile(C.Structure):
    _fields_ = [("ms_prep", C.c_float), ("ms_coarse", C.c_float), ("ms_finalize", C.c_float),
                ("ms_exact", C.c_float), ("ms_exact_finalize", C.c_float), ("ms_total", C.c_float)]


_lib = None


def load_library(path: Optional[str] = None) -> C.CDLL:
    """Load libicdsearch.so and declare the prototypes. Raises if the library is not built."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    p = path or os.environ.get("ICD_SEARCH_LIB", LIB_PATH)
    if not os.path.exists(p):
        raise ImportError(
            f"{p} not found: the HIP extension is not built. Run `python -c 'import __graft_entry__ as g; g.build()'` "
            f"or `make -C rag_project_icd10_amd/csrc`. There is no CPU fallback for the search path.")
    lib = C.CDLL(p)
    vp, i32, i64 = C.c_void_p, C.c_int32, C.c_int64
    lib.icd_abi_version.restype = C.c_int
    lib.icd_last_error.restype = C.c_char_p
    lib.icd_device_count.restype = C.c_int
    lib.icd_index_create.argtypes = [vp, i64, i32, vp, i64, i32, i32, i32, i32, C.POINTER(vp)]
    lib.icd_index_create_view.argtypes = [vp, vp, i64, i32, i32, i32, i32, C.POINTER(vp)]
    lib.icd_index_destroy.argtypes = [vp]
    lib.icd_index_search.argtypes = [vp, vp, i64, i32, i32, i32, vp, vp, i32, vp]
    lib.icd_index_search_reweighted.argtypes = [vp, vp, i64, i32, i32, i32, vp, vp, vp, vp, i32, vp]
    lib.icd_grouping_create.argtypes = [vp, vp, i64, i32, i32, C.POINTER(vp)]
    lib.icd_grouping_destroy.argtypes = [vp]
    lib.icd_grouping_stats.argtypes = [vp, C.POINTER(i64), C.POINTER(i64), C.POINTER(i64)]
    lib.icd_index_search_grouped.argtypes = [vp, vp, vp, i64, i32, i32, i32, i32, vp, vp, vp, vp, vp, i32, vp]
    lib.icd_grouping_prepare_scorers.argtypes = [vp, vp]
    lib.icd_index_search_grouped_scored.argtypes = [vp, vp, vp, i64, i32, i32, i32, i32, i32, vp, vp, vp, vp, vp, vp, vp, i32, vp]
    lib.icd_grouping_prepare_maxsim.argtypes = [vp, vp, i64, i64]
    lib.icd_index_search_maxsim.argtypes = [vp, vp, vp, vp, i64, i32, i32, i32, vp, vp, vp, vp, vp, i32, vp]
    lib.icd_index_search_range.argtypes = [vp, vp, i64, i32, i32, vp, vp, vp, vp, i32, i32, vp, vp, vp, vp, i32, vp]
    lib.icd_rowmask_create.argtypes = [vp, vp, i64, i32, C.POINTER(vp)]
    lib.icd_rowmask_destroy.argtypes = [vp]
    lib.icd_rowmask_stats.argtypes = [vp, C.POINTER(i64), C.POINTER(i64)]
    lib.icd_rowmask_pack.argtypes = [vp, i64, i64, vp, i64]
    lib.icd_index_search_masked.argtypes = [vp, vp, vp, i64, i32, i32, vp, vp, vp, vp, i32, i32, vp, vp, vp, vp, i32, vp]
    lib.icd_fusion_create.argtypes = [vp, i64, C.POINTER(vp)]
    lib.icd_fusion_destroy.argtypes = [vp]
    lib.icd_fusion_stats.argtypes = [vp, C.POINTER(i64), C.POINTER(i64)]
    lib.icd_index_search_hybrid.argtypes = [vp, vp, vp, i64, i32, i32, vp, vp, vp, vp, i32, i32, i32, C.c_double, vp, i32, i32, i32,
                                            vp, vp, vp, vp, vp, i32, vp]
    lib.icd_fusion_fuse_lists.argtypes = [vp, vp, vp, vp, i64, i32, i32, vp, i32, C.c_double, vp, i32, i32, i32, vp, vp, vp, vp, vp, i32, vp]
    lib.icd_sparse_tile_rows.restype = C.c_int
    lib.icd_sparse_pack.argtypes = [vp, vp, vp, i64, i64, vp, vp, vp]
    lib.icd_sparse_create.argtypes = [vp, vp, vp, vp, i64, i32, i32, C.POINTER(vp)]
    lib.icd_sparse_destroy.argtypes = [vp]
    lib.icd_sparse_stats.argtypes = [vp, C.POINTER(i64), C.POINTER(i64), C.POINTER(i64)]
    lib.icd_sparse_search.argtypes = [vp, vp, vp, vp, vp, i64, i32, i32, vp, i32, vp, vp, vp, vp, i32, vp]
    lib.icd_sparse_search_range.argtypes = [vp, vp, vp, vp, vp, i64, i32, i32, vp, vp, vp, vp, vp, i32, i32, vp, vp, vp, vp, i32, vp]
    lib.icd_grouping_pair_sparse.argtypes = [vp, vp, vp]
    lib.icd_sparse_match_rowmasks.argtypes = [vp, vp, vp, vp, vp, i64, i32, vp, vp, vp]
    lib.icd_rowmask_read.argtypes = [vp, vp, i64]
    lib.icd_columns_create.argtypes = [vp, vp, i32, C.POINTER(vp)]
    lib.icd_columns_destroy.argtypes = [vp]
    lib.icd_columns_stats.argtypes = [vp, C.POINTER(i32), C.POINTER(i64), C.POINTER(i64)]
    lib.icd_filter_program_check.argtypes = [vp, vp, i64, i32, i64, vp, i64]
    lib.icd_filter_rowmasks.argtypes = [vp, vp, vp, vp, vp, i64, vp, vp, vp]
    lib.icd_rowmask_select.argtypes = [vp, vp, i64, vp, i32, vp, vp, vp, i32, vp]
    lib.icd_rowmask_group_counts.argtypes = [vp, vp, vp, i64, vp, i32, vp]
    lib.icd_mmr_create.argtypes = [vp, i64, C.POINTER(vp)]
    lib.icd_mmr_destroy.argtypes = [vp]
    lib.icd_mmr_stats.argtypes = [vp, C.POINTER(i64), C.POINTER(i64)]
    lib.icd_index_search_mmr.argtypes = [vp, vp, vp, vp, i64, i32, i32, C.c_double, i32, vp, vp, i32, i32, vp, vp, vp, vp, vp, i32, vp]
    lib.icd_byrows_create.argtypes = [vp, i64, C.POINTER(vp)]
    lib.icd_byrows_destroy.argtypes = [vp]
    lib.icd_byrows_stats.argtypes = [vp, C.POINTER(i64), C.POINTER(i64)]
    lib.icd_index_search_by_rows.argtypes = [vp, vp, vp, vp, i64, i32, i32, i32, vp, vp, i32, i32, vp, vp, vp, vp, i32, vp]
    lib.icd_rankof_create.argtypes = [vp, i64, C.POINTER(vp)]
    lib.icd_rankof_destroy.argtypes = [vp]
    lib.icd_rankof_stats.argtypes = [vp, C.POINTER(i64), C.POINTER(i64)]
    lib.icd_index_rank_of.argtypes = [vp, vp, vp, i64, i32, vp, i32, vp, vp, vp, vp, vp, vp, vp]
    lib.icd_wide_create.argtypes = [vp, i64, i32, C.POINTER(vp)]
    lib.icd_wide_destroy.argtypes = [vp]
    lib.icd_wide_stats.argtypes = [vp, C.POINTER(i64), C.POINTER(i64), C.POINTER(i64)]
    lib.icd_index_search_wide.argtypes = [vp, vp, vp, vp, i64, i32, i32, i32, vp, vp, i32, i32, vp, vp, vp, vp, vp, vp, i32, vp]
    lib.icd_recommend_create.argtypes = [vp, i64, i64, i32, C.POINTER(vp)]
    lib.icd_recommend_destroy.argtypes = [vp]
    lib.icd_recommend_stats.argtypes = [vp, C.POINTER(i64), C.POINTER(i64), C.POINTER(i64), C.POINTER(i64)]
    lib.icd_recommend_read_vectors.argtypes = [vp, i64, vp]
    lib.icd_index_recommend.argtypes = [vp, vp, vp, vp, vp, vp, vp, i64, i32, i32, i32, vp, vp, i32, i32, vp, vp, vp, vp, vp, vp, i32, i32, vp]
    lib.icd_boost_create.argtypes = [vp, i64, C.POINTER(vp)]
    lib.icd_boost_destroy.argtypes = [vp]
    lib.icd_boost_stats.argtypes = [vp, C.POINTER(i64), C.POINTER(i64)]
    lib.icd_index_search_boosted.argtypes = [vp, vp, vp, vp, vp, vp, i64, i32, i32, vp, vp, vp, vp, i32, i32, vp, vp, vp, vp, i32, vp]
    lib.icd_index_search_hybrid_grouped.argtypes = [vp, vp, vp, vp, i64, i32, i32, vp, vp, vp, vp, i32, C.c_double, vp, i32, i32, i32, i32,
                                                    vp, vp, vp, vp, vp, vp, i32, vp]
    lib.icd_fusion_fuse_lists_grouped.argtypes = [vp, vp, vp, vp, vp, i64, i32, i32, vp, i32, C.c_double, vp, i32, i32, i32, i32,
                                                  vp, vp, vp, vp, vp, vp, i32, vp]
    lib.icd_sparse_search_grouped.argtypes = [vp, vp, vp, vp, vp, vp, i64, i32, i32, i32, vp, i32, vp, vp, vp, vp, vp, i32, vp]
    lib.icd_merge_topk.argtypes = [i32, vp, vp, vp, i32, i64, i32, vp, vp, vp, vp, vp]
    lib.icd_index_lookup_levels.argtypes = [vp, vp, i64, vp, vp]
    lib.icd_index_stats.argtypes = [vp, C.POINTER(_Stats)]
    lib.icd_index_cert_terms.argtypes = [vp, vp, vp, vp, vp, vp, i64]
    lib.icd_index_set_chunks.argtypes = [vp, i32]
    lib.icd_index_set_second_pass.argtypes = [vp, i32]
    lib.icd_index_set_option.argtypes = [vp, i32, i32]
    lib.icd_group_unique_id.argtypes = [vp]
    lib.icd_group_create.argtypes = [vp, vp, i32, i32, i32, i32, i32, C.POINTER(vp)]
    lib.icd_group_prepare.argtypes = [vp, i32, i32, i32, i32, i32, i32, C.POINTER(vp)]
    lib.icd_group_connect.argtypes = [vp, vp]
    lib.icd_group_search.argtypes = [vp, vp, i64, i32, i32, vp, vp, vp, vp, vp]
    lib.icd_group_destroy.argtypes = [vp]
    lib.icd_split_bf16x3.argtypes = [i32, vp, i64, i32, i64, i32, vp, vp]
    lib.icd_unpack_query_slices.argtypes = [i32, vp, i32, i64, i32, vp, vp, vp, vp, vp]
    lib.icd_packed_attention.argtypes = [i32, vp, i64, vp, i32, i32, i32, i32, vp, i64, vp]
    lib.icd_encoder_create.argtypes = [i32, C.POINTER(_EncoderDesc), C.POINTER(vp)]
    lib.icd_encoder_encode.argtypes = [vp, vp, vp, i32, i32, i32, vp, i32, vp, vp]
    lib.icd_encoder_encode_many.argtypes = [vp, vp, vp, i64, i32, i32, vp, i32, vp]
    lib.icd_encoder_destroy.argtypes = [vp]
    lib.icd_hier_rescore.argtypes = [i32, vp, vp, i64, i32, i64, i64, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    lib.icd_hier_rescore_entities.argtypes = lib.icd_hier_rescore.argtypes
    lib.icd_score_stats.argtypes = [i32, vp, vp, i64, i32, i32, vp, vp]
    lib.icd_pack_winners.argtypes = [i32, vp, vp, vp, vp, vp, vp, vp, vp, i64, i32, i32, vp, vp]
    lib.icd_cosine_rows.argtypes = [i32, vp, vp, i64, i64, i32, vp, vp]
    lib.icd_term_first_match.argtypes = [i32, vp, vp, i32, vp, vp, i32, vp, vp]
    lib.icd_index_debug_counters.argtypes = [vp, vp, i32]
    lib.icd_index_set_profiling.argtypes = [vp, i32]
    lib.icd_index_last_profile.argtypes = [vp, C.POINTER(_Profile)]
    lib.icd_index_profile_summary.argtypes = [vp, C.POINTER(_Profile), C.POINTER(C.c_int32)]
    have = lib.icd_abi_version()
    if have != ABI_VERSION:
        raise ImportError(f"{p} has ABI version {have}, this package needs {ABI_VERSION}: rebuild it (make -C rag_project_icd10_amd/csrc)")
    for name in EXPORTED_SYMBOLS:
        getattr(lib, name)  # AttributeError if the build is stale
    if path is None:
        _lib = lib
    return lib


def _check(lib, rc: int):
    if rc != 0:
        raise IcdError(rc, (lib.icd_last_error() or b"").decode("utf-8", "replace"))


def _check_inv(lib, rc: int):
    """_check, with ICD_ERR_INVALID (a bad argument) as a ValueError"""
    if rc == -1:
        raise ValueError(lib.icd_last_error().decode("utf-8", "replace"))
    _check(lib, rc)


def device_count() -> int:
    lib = load_library()
    n = lib.icd_device_count()
    if n < 0:
        _check(lib, n)
    return n


def _is_torch_tensor(x) -> bool:
    return type(x).__module__.startswith("torch") and hasattr(x, "data_ptr")


def _current_stream_ptr(device_index: int) -> int:
    import torch
    return int(torch.cuda.current_stream(device_index).cuda_stream)


# ---- what the search methods share ---------------------------------------------------------------------------------------------
def _host_ptr(a):
    return a.ctypes.data


def _dev_ptr(t):
    return t.data_ptr()


def _outputs(on_dev: bool, device: int, shape, dtypes):
    """The uninitialised outputs of one call (numpy dtypes; torch tensors on cuda:device when on_dev), how to take an array's
    pointer, the stream the call runs on and the C ABI's on_device flag"""
    if on_dev:
        import torch
        where = torch.device("cuda", device)
        return ([torch.empty(shape, dtype=getattr(torch, np.dtype(dt).name), device=where) for dt in dtypes], _dev_ptr,
                _current_stream_ptr(device), 1)
    return [np.empty(shape, dt) for dt in dtypes], _host_ptr, None, 0


def _chunked(q, step: int, on_dev: bool, call):
    """call(queries of the chunk, its first query) -> tuple of arrays, per chunk of at most `step` queries; the chunks joined"""
    nq = q.shape[0]
    if nq <= step:   # (the usual call: no slice, no list)
        return call(q, 0)
    outs = [call(q[s0:s0 + step], s0) for s0 in range(0, nq, step)]
    if on_dev:
        import torch
        return tuple(torch.cat([o[i] for o in outs]) for i in range(len(outs[0])))
    return tuple(np.concatenate([o[i] for o in outs]) for i in range(len(outs[0])))


def check_list_offsets(list_off, vectors: int) -> np.ndarray:
    """list_off of an embedding-list search as a contiguous int64 array: lists + 1 offsets from 0 to `vectors`, every list of
    1 .. MAXSIM_MAX_T vectors; anything else is a ValueError"""
    if _is_torch_tensor(list_off):
        list_off = list_off.detach().cpu().numpy()
    raw = np.asarray(list_off)
    if raw.ndim != 1 or raw.size < 1 or raw.dtype.kind not in "iu":
        raise ValueError("list_off: a one-dimensional integer array of lists + 1 offsets")
    off = np.ascontiguousarray(raw, dtype=np.int64)
    if off[0] != 0 or off[-1] != vectors:
        raise ValueError(f"list_off runs from {int(off[0])} to {int(off[-1])}: need 0 to the number of vectors, {vectors}")
    sizes = np.diff(off)
    if sizes.size and (sizes.min() < 1 or sizes.max() > MAXSIM_MAX_T):
        raise ValueError(f"list_off: every list holds 1 .. {MAXSIM_MAX_T} vectors (got {int(sizes.min())} .. {int(sizes.max())})")
    return off


def _bound(v, dtype, shape, on_dev: bool, device: int):
    """A bound (None, a scalar, or values that fill or broadcast to `shape`) as a flat contiguous array of numpy `dtype`, on
    cuda:device when on_dev. The one-dimensional form takes ONE value of any rank for every query."""
    if v is None:
        return None
    flat = len(shape) == 1
    count = shape[0] if flat else math.prod(shape)
    if on_dev:
        import torch
        t = torch.as_tensor(v).to(device=torch.device("cuda", device), dtype=getattr(torch, np.dtype(dtype).name))
        size = t.numel()
    else:
        if _is_torch_tensor(v):
            v = v.detach().cpu().numpy()
        t = np.asarray(v, dtype)
        size = t.size
    if size != count:
        if flat:
            if size != 1:
                raise ValueError(f"a bound holds {size} values for {count} queries")
            t = t.reshape(-1)
        t = t.expand(shape) if on_dev else np.broadcast_to(t, shape)
    return t.contiguous().reshape(-1) if on_dev else np.ascontiguousarray(t).reshape(-1)


class _Bands:
    """The mask table and the bounds of ONE banded call, held over its chunks. The table is made first (a bad mask is the call's first
    error), the bounds by `bound`; at(s0, m, ptr) -> (the mask-table pointer of the chunk of m queries from s0 on, or None; the
    pointers of its bounds, None for an absent one). A chunk's slices are views of the call's arrays, which this object keeps alive."""

    def __init__(self, masks, nq: int, what: str, per: str):
        self.nq = nq
        self.table = None if masks is None else _mask_table(masks, nq, what, per)
        self.bounds = ()

    def bound(self, values, on_dev: bool, device: int):
        """values: (None or a scalar or one value per query, numpy dtype) per bound, in the C call's order"""
        self.bounds = [None if v is None else _bound(v, dt, (self.nq,), on_dev, device) for v, dt in values]

    def at(self, s0: int, m: int, ptr):
        part = self.bounds if m == self.nq else [None if b is None else b[s0:s0 + m] for b in self.bounds]
        return None if self.table is None else self.table.ctypes.data + 8 * s0, [None if b is None else ptr(b) for b in part]


def _check_group_args(grouping, k, group_size) -> int:
    """group_size of a call that may carry a grouping, checked (ValueError / IcdError) before anything else happens"""
    group_size = int(group_size)
    if grouping is None:
        if group_size != 1:
            raise ValueError("group_size needs a grouping")
        return 1
    if grouping.closed:
        raise IcdError(-5, "grouping is closed")
    if int(k) < 1 or group_size < 1 or int(k) * group_size > MAX_K:
        raise ValueError(f"k={k}, group_size={group_size}: need k >= 1, group_size >= 1 and k * group_size <= {MAX_K}")
    return group_size


_SPARSE_OUTS = (np.float64, np.float32, np.int64, np.int32)   # search_sparse: adj, raw, ids, levels; grouped: the hits' groups behind them
_SPARSE_OUTS_GROUPED = _SPARSE_OUTS + (np.int32,)


def _fuse_params(limits, R: int, ranker: str, rrf_c, weights, norm: str):
    """What search_hybrid and fuse_lists hand the fuse: limits as R contiguous int32 (one int is broadcast), weights as R contiguous
    float64 (None unless the ranker is "weighted"), and the C ABI's (ranker, rrf_c, weights pointer, norm). ValueError on a bad one."""
    lim = np.ascontiguousarray(np.broadcast_to(np.asarray(limits, dtype=np.int32).reshape(-1), (R,)) if np.size(limits) == 1
                               else np.asarray(limits, dtype=np.int32).reshape(-1))
    if lim.size != R:
        raise ValueError(f"limits holds {lim.size} entries for {R} requests")
    if ranker not in ("rrf", "weighted"):
        raise ValueError(f"ranker={ranker!r}: 'rrf' or 'weighted'")
    if norm not in NORMS:
        raise ValueError(f"norm={norm!r}: one of {sorted(NORMS)}")
    wts = None
    if ranker == "weighted":
        wts = np.ascontiguousarray(np.asarray(weights, dtype=np.float64).reshape(-1))
        if wts.size != R:
            raise ValueError(f"weights holds {wts.size} entries for {R} requests")
    fuse = (RANKER_RRF if ranker == "rrf" else RANKER_WEIGHTED, float(rrf_c), None if wts is None else wts.ctypes.data, NORMS[norm])
    return lim, wts, fuse


def _mask_table(masks, count: int, what: str, per: str) -> np.ndarray:
    """[entry] -> row-mask handle as a uint64 array (0: unfiltered), for ONE IcdRowMask on every entry or a sequence of `count` of
    IcdRowMask or None. Built without a Python loop over the entries (10 000 of them cost milliseconds in front of the launch): the
    distinct mask objects are found by identity and checked once each."""
    if isinstance(masks, IcdRowMask):
        uniq, inverse = [masks], np.zeros(count, np.int64)
    else:
        masks = list(masks)
        if len(masks) != count:
            raise ValueError(f"masks holds {len(masks)} entries for {what}")
        ident = np.fromiter(map(id, masks), np.int64, count)
        _, first, inverse = np.unique(ident, return_index=True, return_inverse=True)
        uniq = [masks[i] for i in first]
    vals = np.zeros(max(len(uniq), 1), np.uint64)
    for j, m_ in enumerate(uniq):
        if m_ is None:
            continue
        if not isinstance(m_, IcdRowMask):
            raise TypeError(f"masks: IcdRowMask or None per {per}")
        if m_.closed:
            raise IcdError(-5, "a row mask is closed")
        vals[j] = m_._h.value
    return np.ascontiguousarray(vals[inverse.reshape(-1)]) if count else np.zeros(1, np.uint64)


def _boost_tables(boosts, nq: int):
    """[nq][MAX_BOOSTS] row-mask handles (uint64, 0: slot unused) and weights (float32) of a boosted search, from one list of
    (IcdRowMask, weight) pairs - or None - per query"""
    boosts = list(boosts)
    if len(boosts) != nq:
        raise ValueError(f"boosts holds {len(boosts)} entries for {nq} queries")
    handles = np.zeros((max(nq, 1), MAX_BOOSTS), np.uint64)
    weights = np.ones((max(nq, 1), MAX_BOOSTS), np.float32)
    done = {}
    for q, per in enumerate(boosts):
        key = id(per)
        if key in done:   # (the same list object on many queries: filled once)
            handles[q], weights[q] = handles[done[key]], weights[done[key]]
            continue
        done[key] = q
        per = [] if per is None else list(per)
        if len(per) > MAX_BOOSTS:
            raise ValueError(f"boosts[{q}] holds {len(per)} pairs: a query carries up to {MAX_BOOSTS}")
        for j, pair in enumerate(per):
            if pair is None:
                continue
            m_, w = pair
            if not isinstance(m_, IcdRowMask):
                raise TypeError("boosts: (IcdRowMask, weight) pairs")
            if m_.closed:
                raise IcdError(-5, "a row mask is closed")
            handles[q, j] = m_._h.value
            weights[q, j] = np.float32(w)
    return handles, weights


class BoostTable:
    """The boosts of a batch in the form the C ABI takes, built once: search_boosted accepts it in place of the per-query lists,
    which it would otherwise walk in Python on every call (a millisecond per thousand queries, in front of a launch of that
    length). Keeps the masks alive."""

    def __init__(self, boosts, nq: int):
        self._keep = boosts
        self.nq = int(nq)
        self.handles, self.weights = _boost_tables(boosts, self.nq)


class _Handle:
    """A native workspace handle of an index: `_h`, closed once through the entry point its class names in `_destroy`"""
    _destroy = ""

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            getattr(self._lib, self._destroy)(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def closed(self) -> bool:
        return not self._h.value


class IcdIndex:
    """Exact inner-product index over a dense fp32 corpus resident in one GPU's HBM.

    corpus : (n, dim) float32, C-contiguous numpy array, or a torch CUDA tensor on `device`.
    levels : (n,) ICD hierarchy level per row (1/2/3) or None (all level 1, the reference default
             services/milvus_service.py:247).
    id_base: id of row 0 (row-sharded corpora).
    """

    def __init__(self, corpus, levels=None, *, device: int = 0, max_nq: int = 16384, max_k: int = 100,
                 id_base: int = 0, permute: bool = True, probe: bool = True, center: bool = True):
        """permute / probe / center: A/B and test options of THIS index (icd_index_create flags ICD_CREATE_ROW_ORDER / _NO_PROBE /
        _NO_CENTER): performance decisions only, results are identical either way"""
        self._lib = load_library()
        self._h = C.c_void_p()
        on_dev = 0
        if _is_torch_tensor(corpus):
            if not corpus.is_cuda:
                corpus = corpus.detach().cpu().numpy()
            else:
                import torch
                if corpus.dtype != torch.float32 or not corpus.is_contiguous():
                    corpus = corpus.to(torch.float32).contiguous()
                if corpus.device.index != device:
                    raise ValueError(f"corpus is on cuda:{corpus.device.index}, index on device {device}")
                on_dev = 1
        if on_dev:
            import torch
            n, dim = int(corpus.shape[0]), int(corpus.shape[1])
            cptr = corpus.data_ptr()
            lv = None
            if levels is not None:
                lv = torch.as_tensor(levels).to(device=corpus.device, dtype=torch.int32).contiguous()
            lptr = lv.data_ptr() if lv is not None else None
            torch.cuda.synchronize(device)
        else:
            corpus = np.ascontiguousarray(corpus, dtype=np.float32)
            if corpus.ndim != 2:
                raise ValueError("corpus must be 2-D (n, dim)")
            n, dim = corpus.shape
            cptr = corpus.ctypes.data
            lv = None if levels is None else np.ascontiguousarray(levels, dtype=np.int32)
            if lv is not None and lv.shape != (n,):
                raise ValueError("levels must have shape (n,)")
            lptr = lv.ctypes.data if lv is not None else None
        self.n, self.dim, self.device, self.max_nq, self.max_k = int(n), int(dim), int(device), int(max_nq), int(max_k)
        self.id_base = int(id_base)
        self.rows = None   # a view's rows of its parent (view())
        self._ab_flags = (0 if permute else CREATE_ROW_ORDER) | (0 if probe else CREATE_NO_PROBE) | (0 if center else CREATE_NO_CENTER)
        flags = (CREATE_CORPUS_ON_DEVICE if on_dev else 0) | self._ab_flags
        _check(self._lib, self._lib.icd_index_create(cptr, n, dim, lptr, id_base, device, max_nq, max_k, flags,
                                                      C.byref(self._h)))

    def view(self, rows, *, max_nq: Optional[int] = None, max_k: Optional[int] = None) -> "IcdIndex":
        """An index over rows `rows` of this one (icd_index_create_view): built on the device from this index's rows and levels,
        then like any index (its own fp16 image, centring and probe); its hits carry THIS index's global ids. rows: strictly
        increasing row indices in [0, n), a numpy array or a torch CUDA tensor (int64). max_nq / max_k default to this index's.
        The view is independent: closing this index first leaves it valid."""
        if self.closed:
            raise IcdError(-5, "index is closed")
        if _is_torch_tensor(rows) and rows.is_cuda:
            import torch
            r = rows.to(torch.int64).contiguous().reshape(-1)
            if r.device.index != self.device:
                raise ValueError(f"rows on cuda:{r.device.index}, index on device {self.device}")
            torch.cuda.synchronize(self.device)
            ptr, on_dev, m = r.data_ptr(), 1, int(r.numel())
        else:
            if _is_torch_tensor(rows):
                rows = rows.detach().cpu().numpy()
            r = np.ascontiguousarray(rows, dtype=np.int64).reshape(-1)
            ptr, on_dev, m = r.ctypes.data, 0, int(r.size)
        v = IcdIndex.__new__(IcdIndex)
        v._lib = self._lib
        v._h = C.c_void_p()
        v.n, v.dim, v.device = m, self.dim, self.device
        v.max_nq = int(max_nq if max_nq is not None else self.max_nq)
        v.max_k = int(max_k if max_k is not None else self.max_k)
        v.id_base, v._ab_flags = self.id_base, self._ab_flags
        _check(self._lib, self._lib.icd_index_create_view(self._h, ptr if m else None, m, on_dev, v.max_nq, v.max_k, self._ab_flags,
                                                           C.byref(v._h)))
        v.rows = r.cpu().numpy() if on_dev else r.copy()
        return v

    # -- lifecycle -----------------------------------------------------------------------------------
    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            for ref in list(getattr(self, "_group_refs", [])):   # (an IcdGroup borrows this handle: it goes first, never dangles)
                grp = ref()
                if grp is not None:
                    grp.close()
            self._lib.icd_index_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def closed(self) -> bool:
        return not self._h.value

    # -- search --------------------------------------------------------------------------------------
    def _prep_queries(self, queries, rank: int = 2):
        """queries as contiguous float32 of `rank` dimensions (one dimension less: a single entry) -> (array, on_device)"""
        on_dev = type(queries) is not np.ndarray and _is_torch_tensor(queries) and queries.is_cuda
        if on_dev:
            import torch
            q = queries
            if q.dtype != torch.float32 or not q.is_contiguous():
                q = q.to(torch.float32).contiguous()
            if q.device.index != self.device:
                raise ValueError(f"queries on cuda:{q.device.index}, index on device {self.device}")
        else:
            if type(queries) is not np.ndarray and _is_torch_tensor(queries):
                queries = queries.detach().cpu().numpy()
            q = np.ascontiguousarray(queries, dtype=np.float32)
        if q.ndim == rank - 1:
            q = q[None]
        return q, on_dev

    def _validate(self, q, k):
        if self.closed:
            raise IcdError(-5, "index is closed")
        if q.shape[-1] != self.dim:
            raise ValueError(f"query dim {q.shape[-1]} != index dim {self.dim}")
        if not (1 <= k <= self.max_k):
            raise ValueError(f"k={k} outside 1..{self.max_k}")

    def search(self, queries, k: int = 10, mode: int = MODE_AUTO):
        """Raw top-k by inner product -> (scores float32 [nq,k], ids int64 [nq,k]), best first.
        Device tensors in -> device tensors out (enqueued on torch's current stream, no sync)."""
        q, on_dev = self._prep_queries(queries)
        self._validate(q, k)

        def call(qs, s0):
            m = qs.shape[0]
            (sc, ids), ptr, stream, dev = _outputs(on_dev, self.device, (m, k), (np.float32, np.int64))
            if m:
                _check(self._lib, self._lib.icd_index_search(self._h, ptr(qs), m, k, dev, mode, ptr(sc), ptr(ids), dev, stream))
            return sc, ids
        return _chunked(q, self.max_nq, on_dev, call)

    def search_reweighted(self, queries, k: int = 10, mode: int = MODE_AUTO):
        """Raw top-k, then adj = float64(score) * w[level] and a stable descending re-sort of the k hits
        (services/milvus_service.py:290-295,314). Returns (adj f64, raw f32, ids i64, levels i32), each [nq,k]."""
        q, on_dev = self._prep_queries(queries)
        self._validate(q, k)

        def call(qs, s0):
            m = qs.shape[0]
            (adj, raw, ids, lv), ptr, stream, dev = _outputs(on_dev, self.device, (m, k), (np.float64, np.float32, np.int64, np.int32))
            if m:
                _check(self._lib, self._lib.icd_index_search_reweighted(self._h, ptr(qs), m, k, dev, mode, ptr(adj), ptr(raw), ptr(ids),
                                                                         ptr(lv), dev, stream))
            return adj, raw, ids, lv
        return _chunked(q, self.max_nq, on_dev, call)

    # -- grouping search (Milvus group_by_field / group_size) ------------------------------------------
    def grouping(self, group_of, *, max_nq: Optional[int] = None) -> "IcdGrouping":
        """A grouping of this index's rows (icd_grouping_create): group_of holds one non-negative int32 id per row (of a view:
        per row of the view), a numpy array or a torch CUDA tensor. Created once per field; several may coexist. It holds the
        workspace of its searches (batches of up to max_nq queries, default this index's max_nq)."""
        if self.closed:
            raise IcdError(-5, "index is closed")
        return IcdGrouping(self, group_of, int(max_nq if max_nq is not None else self.max_nq))

    def search_grouped(self, queries, k: int, group_size: int, grouping: "IcdGrouping", reweighted: bool = True, *, scorer: str = "max",
                       group_scores: bool = False):
        """The k best groups of every query and the group_size best rows of each, exact (icd_index_search_grouped). Outputs are
        [nq, k * group_size]. reweighted=True: (adj f64, raw f32, ids i64, levels i32, groups i32) in search_reweighted's order
        (level weight, one stable re-sort of the query's hits); False: (raw, ids, levels, groups) group by group, best group
        first. Padding: -inf, id -1, level 0, group -1. Device tensors in -> device tensors out on torch's current stream.

        scorer "max" | "sum" | "avg" (icd_index_search_grouped_scored): what a group ranks by - its best row, or the fp32 sum /
        mean, best first, of its group_size best rows; the hits keep their own scores. group_scores=True appends two arrays
        [nq, k] in group-rank order: that score (f32, padding -inf) and the group's id (i32, padding -1). The defaults are the
        call above with its return tuple. The first scored call prepares the grouping (IcdGrouping.prepare_scorers)."""
        q, on_dev = self._prep_queries(queries)
        if self.closed or grouping is None or grouping.closed:
            raise IcdError(-5, "index or grouping is closed")
        if q.shape[-1] != self.dim:
            raise ValueError(f"query dim {q.shape[-1]} != index dim {self.dim}")
        k, group_size = int(k), int(group_size)
        if k < 1 or group_size < 1 or k * group_size > MAX_K:
            raise ValueError(f"k={k}, group_size={group_size}: need k >= 1, group_size >= 1 and k * group_size <= {MAX_K}")
        if scorer not in GROUP_SCORERS:
            raise ValueError(f"scorer={scorer!r}: one of {sorted(GROUP_SCORERS)}")
        scored = scorer != "max" or bool(group_scores)
        if scored:
            grouping.prepare_scorers(self)   # (behind every argument check of this layer: a refused call leaves the grouping as it was)

        def call(qs, s0):
            m = qs.shape[0]
            (adj, raw, ids, lv, grp), ptr, stream, dev = _outputs(on_dev, self.device, (m, k * group_size),
                                                                  (np.float64, np.float32, np.int64, np.int32, np.int32))
            if scored:
                (gsc, gid), _p, _s, _d = _outputs(on_dev, self.device, (m, k), (np.float32, np.int32))
                if m:
                    _check(self._lib, self._lib.icd_index_search_grouped_scored(
                        self._h, grouping._h, ptr(qs), m, k, group_size, dev, 1 if reweighted else 0, GROUP_SCORERS[scorer],
                        ptr(adj) if reweighted else None, ptr(raw), ptr(ids), ptr(lv), ptr(grp),
                        ptr(gsc) if group_scores else None, ptr(gid) if group_scores else None, dev, stream))
                return ((adj, raw, ids, lv, grp) if reweighted else (raw, ids, lv, grp)) + ((gsc, gid) if group_scores else ())
            if m:
                _check(self._lib, self._lib.icd_index_search_grouped(
                    self._h, grouping._h, ptr(qs), m, k, group_size, dev, 1 if reweighted else 0,
                    ptr(adj) if reweighted else None, ptr(raw), ptr(ids), ptr(lv), ptr(grp), dev, stream))
            return (adj, raw, ids, lv, grp) if reweighted else (raw, ids, lv, grp)
        return _chunked(q, grouping.max_nq, on_dev, call)

    # -- embedding-list search (Milvus embedding lists, metric MAX_SIM) ---------------------------------
    def search_lists(self, queries, list_off, k: int, grouping: "IcdGrouping", *, scorer: str = "sum", matches: bool = True):
        """The k best groups of every LIST of query vectors, exact (icd_index_search_maxsim): list L owns the vectors
        list_off[L] .. list_off[L + 1] of queries [vectors, dim] (1 .. 64 each; list_off a host array of lists + 1 offsets from
        0), and a group scores the fp32 sum - scorer "mean": the mean over the vectors that hit it - in list order, of its best
        row's inner product under every vector. Returns (group_scores f32 [lists, k], group_ids i32 [lists, k]) and, with
        matches=True, (match_scores f32, match_ids i64, match_levels i32), each [vectors, k]: slot j of vector t is the best row
        of its list's j-th group under t. Padding: -inf, group -1, id -1, level 0. Device tensors in -> device tensors out on
        torch's current stream. The first call prepares the grouping for its max_nq (IcdGrouping.prepare_maxsim); a batch above
        the preparation is split between lists into several calls."""
        q, on_dev = self._prep_queries(queries)
        if self.closed or grouping is None or grouping.closed:
            raise IcdError(-5, "index or grouping is closed")
        if q.ndim != 2 or q.shape[-1] != self.dim:
            raise ValueError(f"queries of shape {tuple(q.shape)}: need [vectors, {self.dim}]")
        off = check_list_offsets(list_off, q.shape[0])
        k = int(k)
        if not 1 <= k <= MAX_K:
            raise ValueError(f"k={k} outside 1..{MAX_K}")
        if scorer not in MAXSIM_SCORERS:
            raise ValueError(f"scorer={scorer!r}: one of {sorted(MAXSIM_SCORERS)}")
        if grouping.maxsim is None:   # (behind every argument check of this layer: a refused call leaves the grouping as it was)
            grouping.prepare_maxsim(self, grouping.max_nq, max(grouping.max_nq, MAXSIM_MAX_T))
        max_lists, max_vectors = grouping.maxsim
        nl, nv = len(off) - 1, q.shape[0]
        outs = []
        l0 = 0
        while l0 < nl:   # whole lists per call, within the preparation
            l1 = min(nl, l0 + max_lists, int(np.searchsorted(off, off[l0] + max_vectors, side="right")) - 1)
            v0, v1 = int(off[l0]), int(off[l1])
            (gsc, gid), ptr, stream, dev = _outputs(on_dev, self.device, (l1 - l0, k), (np.float32, np.int32))
            (msc, mid, mlv), _p, _s, _d = _outputs(on_dev, self.device, (v1 - v0, k) if matches else (0, k), (np.float32, np.int64, np.int32))
            local = np.ascontiguousarray(off[l0:l1 + 1] - v0)
            _check(self._lib, self._lib.icd_index_search_maxsim(
                self._h, grouping._h, ptr(q[v0:v1]), local.ctypes.data, l1 - l0, k, MAXSIM_SCORERS[scorer], dev, ptr(gsc), ptr(gid),
                ptr(msc) if matches else None, ptr(mid) if matches else None, ptr(mlv) if matches else None, dev, stream))
            outs.append((gsc, gid, msc, mid, mlv) if matches else (gsc, gid))
            l0 = l1
        if len(outs) == 1:
            return outs[0]
        if not outs:
            (gsc, gid), _p, _s, _d = _outputs(on_dev, self.device, (0, k), (np.float32, np.int32))
            (msc, mid, mlv), _p, _s, _d = _outputs(on_dev, self.device, (0, k), (np.float32, np.int64, np.int32))
            return (gsc, gid, msc, mid, mlv) if matches else (gsc, gid)
        if on_dev:
            import torch
            return tuple(torch.cat([o[i] for o in outs]) for i in range(len(outs[0])))
        return tuple(np.concatenate([o[i] for o in outs]) for i in range(len(outs[0])))

    # -- range search, offset, iterator pages (Milvus radius / range_filter, offset, search_iterator) ----
    def search_range(self, queries, k: int = 10, *, radius=None, range_filter=None, after=None, reweighted: bool = True):
        """The min(k, rows in the band) best rows strictly inside a band of every query's ranking, exact (icd_index_search_range):
        radius < score <= range_filter, and - after=(scores, ids), a hit an earlier search returned: its raw score and its id -
        ranked strictly behind that hit. Bounds are scalars (broadcast) or one value per query (arrays / CUDA tensors); the band
        is on the raw inner product. reweighted=True: (adj f64, raw f32, ids i64, levels i32) in search_reweighted's order;
        False: (raw, ids, levels) in raw order. Padding behind the band's last row: -inf, id -1, level 0. Device tensors in ->
        device tensors out on torch's current stream (the bounds are moved to the device if they are not there)."""
        return self._search_band(queries, k, radius, range_filter, after, reweighted, None)

    # -- masked search (a Milvus filter as a per-query bitset over the rows) ----------------------------
    def rowmask(self, rows) -> "IcdRowMask":
        """A row mask of this index (icd_rowmask_create): rows = strictly increasing row indices in [0, n), a numpy array or a
        torch CUDA tensor (int64); an empty list is the empty mask. A bitset of n / 8 bytes on the device; any number per index."""
        if self.closed:
            raise IcdError(-5, "index is closed")
        return IcdRowMask(self, rows)

    def search_masked(self, queries, k: int, masks, *, radius=None, range_filter=None, after=None, reweighted: bool = True):
        """search_range over, for every query, the ranking restricted to the rows of its mask (icd_index_search_masked): masks is
        ONE IcdRowMask for every query, or a sequence of length nq of IcdRowMask or None (None: that query is unfiltered). Same
        bounds, outputs and padding as search_range; ids are this index's own. With one mask on every query the outputs equal
        view(rows).search in MODE_EXACT bit for bit. Device tensors in -> device tensors out on torch's
        current stream, enqueued only; the call is not graph-capturable (the mask table is staged on the host at call time)."""
        return self._search_band(queries, k, radius, range_filter, after, reweighted, masks)

    def _search_band(self, queries, k, radius, range_filter, after, reweighted, masks, boost=None):
        q, on_dev = self._prep_queries(queries)
        self._validate(q, k)
        nq = int(q.shape[0])
        step = self.max_nq
        if boost is not None:   # (workspace, boosts): the [nq][MAX_BOOSTS] tables of the call, kept alive over the calls below
            step = min(step, boost[0].max_nq)
            table = boost[1] if isinstance(boost[1], BoostTable) else BoostTable(boost[1], nq)   # (kept alive over the calls below)
            if table.nq != nq:
                raise ValueError(f"the boost table holds {table.nq} entries for {nq} queries")
            boost_h, boost_w = table.handles, table.weights
        bands = _Bands(masks, nq, f"{nq} queries", "query")
        a_sc, a_id = (None, None) if after is None else after
        if (a_sc is None) != (a_id is None):
            raise ValueError("after = (scores, ids): both or neither")
        bands.bound(((radius, np.float32), (range_filter, np.float32), (a_sc, np.float32), (a_id, np.int64)), on_dev, self.device)

        def call(qs, s0):
            m = qs.shape[0]
            (adj, raw, ids, lv), ptr, stream, dev = _outputs(on_dev, self.device, (m, k), (np.float64, np.float32, np.int64, np.int32))
            if m:
                p_mask, p_bounds = bands.at(s0, m, ptr)
                tail = (ptr(qs), m, k, dev, *p_bounds, dev, 1 if reweighted else 0,
                        ptr(adj) if reweighted else None, ptr(raw), ptr(ids), ptr(lv), dev, stream)
                if boost is not None:
                    _check(self._lib, self._lib.icd_index_search_boosted(
                        self._h, boost[0]._h, p_mask,
                        boost_h.ctypes.data + 8 * MAX_BOOSTS * s0, boost_w.ctypes.data + 4 * MAX_BOOSTS * s0, *tail))
                elif p_mask is None:
                    _check(self._lib, self._lib.icd_index_search_range(self._h, *tail))
                else:
                    _check(self._lib, self._lib.icd_index_search_masked(self._h, p_mask, *tail))
            return (adj, raw, ids, lv) if reweighted else (raw, ids, lv)
        return _chunked(q, step, on_dev, call)

    def _workspace(self, cls, size):
        """a sized workspace of this index (IcdBoost, IcdMmr, IcdByRows, IcdFusion)"""
        if self.closed:
            raise IcdError(-5, "index is closed")
        return cls(self, int(size))

    # -- boosted search (Milvus 2.6's boost ranker: rows inside a mask count `weight` times as much, before the top-k is chosen) --
    def boost_workspace(self, max_nq: Optional[int] = None) -> "IcdBoost":
        """The workspace of this index's boosted searches (icd_boost_create) for calls of up to max_nq queries (default: the index's)."""
        return self._workspace(IcdBoost, max_nq if max_nq is not None else self.max_nq)

    def search_boosted(self, queries, k: int, boosts, masks=None, *, workspace: "IcdBoost", reweighted: bool = True, radius=None,
                       range_filter=None, after=None):
        """search_masked over the BOOSTED ranking (icd_index_search_boosted): boosts holds, per query, a list of up to MAX_BOOSTS
        (IcdRowMask, weight) pairs - None in a pair's place for an unused slot, None or [] for a query without boosts - or a
        BoostTable made of such lists once, for a batch that is searched again and again; the score
        of a row inside a pair's mask is multiplied by its weight (one fp32 multiply per pair, in list order) before anything is
        selected. masks, radius, range_filter and after=(scores, ids) are search_masked's and act on the boosted score; the raw
        output carries it. Weights are positive normal floats (IcdError -1 otherwise). Outputs as search_masked; with no pair at
        all they are search_masked's bit for bit. Not graph-capturable."""
        if self.closed or workspace is None or workspace.closed:
            raise IcdError(-5, "index or boost workspace is closed")
        return self._search_band(queries, k, radius, range_filter, after, reweighted, masks, (workspace, boosts))

    # -- MMR search (a diverse top-k: LangChain's max_marginal_relevance_search on the device) -------------
    def mmr(self, max_nq: Optional[int] = None) -> "IcdMmr":
        """The workspace of this index's MMR searches (icd_mmr_create) for calls of up to max_nq queries (default: the index's)."""
        return self._workspace(IcdMmr, max_nq if max_nq is not None else self.max_nq)

    def search_mmr(self, queries, k: int, fetch_k: int, lambda_mult: float, *, mmr: "IcdMmr", masks=None, radius=None, range_filter=None,
                   reweighted: bool = True, on_device: bool = False):
        """The k hits of every query picked greedily out of its fetch_k exact candidates by maximal marginal relevance
        (icd_index_search_mmr): value = lambda_mult * score - (1 - lambda_mult) * max similarity to a hit already picked, the
        similarity being the canonical inner product of the two stored rows. 1 <= k <= fetch_k <= 128 (and the index's max_k),
        lambda_mult in [0, 1]; masks, radius and range_filter as in search_masked (they shape the candidate list). Returns
        (adj f64, raw f32, ids i64, levels i32, mmr_values f64), each [nq, k]: reweighted=True in search_reweighted's order (level
        weight, one stable re-sort of the picked hits), False in pick order with adj None. Padding: -inf, id -1, level 0, mmr -inf.
        lambda_mult = 1 is search_masked at k, bit for bit. CUDA queries or on_device=True: device tensors out on torch's current
        stream. A batch longer than the workspace's max_nq runs in chunks."""
        if self.closed or mmr is None or mmr.closed:
            raise IcdError(-5, "index or mmr workspace is closed")
        q, q_dev = self._prep_queries(queries)
        if q.shape[-1] != self.dim:
            raise ValueError(f"query dim {q.shape[-1]} != index dim {self.dim}")
        k, fetch_k, lam = int(k), int(fetch_k), float(lambda_mult)
        if not (1 <= k <= fetch_k <= min(MAX_K, self.max_k)):
            raise ValueError(f"k={k}, fetch_k={fetch_k}: need 1 <= k <= fetch_k <= {min(MAX_K, self.max_k)}")
        if not (0.0 <= lam <= 1.0):
            raise ValueError(f"lambda_mult={lambda_mult}: the relevance weight lies in [0, 1]")
        out_dev = bool(on_device) or q_dev
        nq = int(q.shape[0])
        bands = _Bands(masks, nq, f"{nq} queries", "query")
        bands.bound(((radius, np.float32), (range_filter, np.float32)), q_dev, self.device)

        def call(qs, s0):
            m = qs.shape[0]
            (adj, raw, ids, lv, mv), ptr, stream, dev = _outputs(out_dev, self.device, (m, k), (np.float64, np.float32, np.int64, np.int32, np.float64))
            if m:
                if q_dev and stream is None:
                    stream = _current_stream_ptr(self.device)
                qptr = _dev_ptr if q_dev else _host_ptr
                p_mask, p_bounds = bands.at(s0, m, qptr)
                _check(self._lib, self._lib.icd_index_search_mmr(
                    self._h, mmr._h, p_mask, qptr(qs), m, k, fetch_k, lam, 1 if q_dev else 0,
                    *p_bounds, 1 if q_dev else 0, 1 if reweighted else 0,
                    ptr(adj) if reweighted else None, ptr(raw), ptr(ids), ptr(lv), ptr(mv), dev, stream))
            return (adj, raw, ids, lv, mv) if reweighted else (raw, ids, lv, mv)
        outs = _chunked(q, min(self.max_nq, mmr.max_nq), out_dev, call)
        return outs if reweighted else (None,) + tuple(outs)

    # -- search by stored rows (Milvus's search by primary key: a stored row is the query) ----------------
    def byrows(self, max_nq: Optional[int] = None) -> "IcdByRows":
        """The workspace of this index's searches by rows (icd_byrows_create) for calls of up to max_nq ids (default: the index's)."""
        return self._workspace(IcdByRows, max_nq if max_nq is not None else self.max_nq)

    def search_by_rows(self, ids, k: int, *, workspace: "IcdByRows", masks=None, radius=None, range_filter=None, include_self: bool = False,
                       reweighted: bool = True, on_device: bool = False):
        """search_masked with, for query q, the stored fp32 row of global id ids[q] as the query vector, ranked over every row but
        that row itself (icd_index_search_by_rows): the row is gathered on the device, the masked search runs at k + 1 and the
        row's own hit is cut out there - no vector crosses the bus. ids: int64 [nq], a numpy array / sequence (checked: IcdError -1
        for an id outside the index) or a torch CUDA tensor (not read on the host: an id outside the index yields padding); the
        same id may repeat. 1 <= k <= 127 and k + 1 <= the index's max_k; include_self=True is search_masked at k, bit for bit
        (k <= 128). masks, radius and range_filter as in search_masked. Returns (adj f64, raw f32, ids i64, levels i32), each
        [nq, k], in search_reweighted's order, or (raw, ids, levels) in raw order with reweighted=False. Padding: -inf, id -1,
        level 0. CUDA ids or on_device=True: device tensors out on torch's current stream. A batch longer than the workspace's
        max_nq runs in chunks."""
        if self.closed or workspace is None or workspace.closed:
            raise IcdError(-5, "index or by-rows workspace is closed")
        ids_dev = _is_torch_tensor(ids) and ids.is_cuda
        if ids_dev:
            import torch
            rows = ids.to(dtype=torch.int64).contiguous().reshape(-1)
        else:
            if _is_torch_tensor(ids):
                ids = ids.detach().cpu().numpy()
            rows = np.ascontiguousarray(np.asarray(ids, np.int64).reshape(-1))
        k = int(k)
        top = min(MAX_K, self.max_k) - (0 if include_self else 1)
        if not (1 <= k <= top):
            raise ValueError(f"k={k}: need 1 <= k <= {top} (the search runs at k + 1 unless include_self)")
        out_dev = bool(on_device) or ids_dev
        nq = int(rows.shape[0])
        bands = _Bands(masks, nq, f"{nq} ids", "id")
        bands.bound(((radius, np.float32), (range_filter, np.float32)), ids_dev, self.device)

        def call(rs, s0):
            m = rs.shape[0]
            (adj, raw, oid, lv), ptr, stream, dev = _outputs(out_dev, self.device, (m, k), (np.float64, np.float32, np.int64, np.int32))
            if m:
                if ids_dev and stream is None:
                    stream = _current_stream_ptr(self.device)
                iptr = _dev_ptr if ids_dev else _host_ptr
                p_mask, p_bounds = bands.at(s0, m, iptr)
                _check(self._lib, self._lib.icd_index_search_by_rows(
                    self._h, workspace._h, p_mask, iptr(rs), m, k, 1 if ids_dev else 0,
                    1 if include_self else 0, *p_bounds, 1 if ids_dev else 0,
                    1 if reweighted else 0, ptr(adj) if reweighted else None, ptr(raw), ptr(oid), ptr(lv), dev, stream))
            return (adj, raw, oid, lv) if reweighted else (raw, oid, lv)
        return _chunked(rows, min(self.max_nq, workspace.max_nq), out_dev, call)

    # -- hybrid search (Milvus hybrid_search over dense requests) -----------------------------------------
    def fusion(self, max_total: int) -> "IcdFusion":
        """The workspace of this index's hybrid searches (icd_fusion_create) for calls of up to max_total = nq * R sub-lists."""
        return self._workspace(IcdFusion, max_total)

    def search_hybrid(self, queries, limits, k: int, fusion: "IcdFusion", *, ranker: str = "rrf", rrf_c: float = 60.0, weights=None,
                      norm: str = "none", masks=None, radius=None, range_filter=None, mode: int = MODE_AUTO, reweighted: bool = True,
                      grouping: Optional["IcdGrouping"] = None, group_size: int = 1):
        """R dense requests per query fused into one hit list on the device (icd_index_search_hybrid). queries: [nq, R, dim] (a
        numpy array or a torch CUDA tensor); limits: R ints in 1 .. 128 (or one int for every request). ranker "rrf" (rrf_c) or
        "weighted" (weights: R floats in [0, 1]; norm "none" | "cosine" | "atan"). masks: None, or nq * R entries (nested [nq][R]
        or flat) of IcdRowMask or None; radius / range_filter: None, or arrays broadcastable to [nq, R] (-inf / +inf leave a
        sub-list unbounded). reweighted=True: (adj f64, fused f64, ids i64, levels i32, reqbits) in search_reweighted's
        order; False: (fused, ids, levels, reqbits) best fused score first. reqbits: bit r set iff request r's list held the id
        (uint32 in numpy; an int32 tensor on the device, the same bit patterns). Padding: -inf, id -1, level 0, bits 0. Device
        tensors in -> device tensors out on torch's current stream.
        grouping (an IcdGrouping of this index) / group_size: the grouped form (icd_index_search_hybrid_grouped) - limits then
        count GROUPS per request (limit * group_size <= 128), k the fused groups (k * group_size <= 128); every sub-list is the
        grouped search's, the fused hits are grouped again; outputs [nq, k * group_size] with the hits' group ids as one more
        array (padding -1). Masks and bounds cannot be combined with it (ValueError); `mode` does not apply."""
        if self.closed or fusion is None or fusion.closed:
            raise IcdError(-5, "index or fusion is closed")
        group_size = _check_group_args(grouping, k, group_size)
        if grouping is not None and (masks is not None or radius is not None or range_filter is not None):
            raise ValueError("masks and radius / range_filter cannot be combined with grouping")
        q, on_dev = self._prep_queries(queries, rank=3)
        if q.ndim != 3 or q.shape[-1] != self.dim:
            raise ValueError(f"queries must be [nq, R, {self.dim}], got {tuple(q.shape)}")
        nq, R = int(q.shape[0]), int(q.shape[1])
        lim, wts, fuse = _fuse_params(limits, R, ranker, rrf_c, weights, norm)   # (lim and wts kept alive over the call)
        k = int(k)
        mask_h = None
        if masks is not None:
            flat = []
            for m_ in masks:
                flat.extend(m_ if isinstance(m_, (list, tuple)) else [m_])
            mask_h = _mask_table(flat, nq * R, f"{nq} x {R} sub-searches", "(query, request)")
            if not mask_h.any():
                mask_h = None
        if grouping is not None:
            (adj, fused, ids, lv, bits, grp), ptr, stream, dev = _outputs(
                on_dev, self.device, (nq, k * group_size), (np.float64, np.float64, np.int64, np.int32, np.int32 if on_dev else np.uint32, np.int32))
            rc = self._lib.icd_index_search_hybrid_grouped(
                self._h, fusion._h, grouping._h, ptr(q) if nq else None, nq, R, dev, lim.ctypes.data, None, None, None,
                *fuse, k, group_size, 1 if reweighted else 0, ptr(adj) if reweighted else None, ptr(fused), ptr(ids), ptr(lv), ptr(bits), ptr(grp), dev, stream)
            _check_inv(self._lib, rc)
            return (adj, fused, ids, lv, bits, grp) if reweighted else (fused, ids, lv, bits, grp)
        lo, hi = (_bound(v, np.float32, (nq, R), on_dev, self.device) for v in (radius, range_filter))
        (adj, fused, ids, lv, bits), ptr, stream, dev = _outputs(
            on_dev, self.device, (nq, k), (np.float64, np.float64, np.int64, np.int32, np.int32 if on_dev else np.uint32))
        rc = self._lib.icd_index_search_hybrid(
            self._h, fusion._h, ptr(q) if nq else None, nq, R, dev, lim.ctypes.data,
            None if mask_h is None else mask_h.ctypes.data, None if lo is None else ptr(lo), None if hi is None else ptr(hi),
            dev, int(mode), *fuse, k, 1 if reweighted else 0,
            ptr(adj) if reweighted else None, ptr(fused), ptr(ids), ptr(lv), ptr(bits), dev, stream)
        _check(self._lib, rc)
        return (adj, fused, ids, lv, bits) if reweighted else (fused, ids, lv, bits)

    def fuse_lists(self, fusion: "IcdFusion", scores, ids, limits, k: int, *, ranker: str = "rrf", rrf_c: float = 60.0, weights=None,
                   norm: str = "none", reweighted: bool = True, to_host: bool = False, grouping: Optional["IcdGrouping"] = None,
                   group_size: int = 1):
        """Step 2 of search_hybrid on the caller's lists (icd_fusion_fuse_lists): scores [nq, R, lmax] float32 and ids
        [nq, R, lmax] int64 (this index's ids, -1 = padding), best first - numpy arrays (uploaded) or torch CUDA tensors. limits,
        rankers and outputs as search_hybrid; device tensors out unless to_host. grouping / group_size: the grouped form
        (icd_fusion_fuse_lists_grouped) as in search_hybrid - list r is cut in front of its (limit + 1)-th run of equal group ids,
        a hit's group is read from the grouping by row."""
        if self.closed or fusion is None or fusion.closed:
            raise IcdError(-5, "index or fusion is closed")
        group_size = _check_group_args(grouping, k, group_size)
        import torch
        where = torch.device("cuda", self.device)
        sc = torch.as_tensor(scores).to(device=where, dtype=torch.float32).contiguous()
        idt = torch.as_tensor(ids).to(device=where, dtype=torch.int64).contiguous()
        if sc.ndim != 3 or tuple(idt.shape) != tuple(sc.shape):
            raise ValueError(f"scores and ids must both be [nq, R, lmax], got {tuple(sc.shape)} and {tuple(idt.shape)}")
        nq, R, lmax = (int(v) for v in sc.shape)
        lim, wts, fuse = _fuse_params(limits, R, ranker, rrf_c, weights, norm)   # (lim and wts kept alive over the call)
        k = int(k)
        on_dev = not to_host
        dtypes = (np.float64, np.float64, np.int64, np.int32, np.int32 if on_dev else np.uint32) + ((np.int32,) if grouping is not None else ())
        outs, ptr, stream, dev = _outputs(on_dev, self.device, (nq, k * group_size), dtypes)
        adj, fused, out_ids, lv, bits = outs[:5]
        if stream is None:
            stream = _current_stream_ptr(self.device)   # (the lists are device tensors of torch's current stream)
        if grouping is not None:
            grp = outs[5]
            rc = self._lib.icd_fusion_fuse_lists_grouped(
                self._h, fusion._h, grouping._h, sc.data_ptr() if nq else None, idt.data_ptr() if nq else None, nq, R, lmax, lim.ctypes.data,
                *fuse, k, group_size, 1 if reweighted else 0, ptr(adj) if reweighted else None, ptr(fused), ptr(out_ids), ptr(lv), ptr(bits), ptr(grp),
                dev, stream)
            _check_inv(self._lib, rc)
            return (adj, fused, out_ids, lv, bits, grp) if reweighted else (fused, out_ids, lv, bits, grp)
        rc = self._lib.icd_fusion_fuse_lists(
            self._h, fusion._h, sc.data_ptr() if nq else None, idt.data_ptr() if nq else None, nq, R, lmax, lim.ctypes.data,
            *fuse, k, 1 if reweighted else 0, ptr(adj) if reweighted else None, ptr(fused), ptr(out_ids), ptr(lv), ptr(bits), dev, stream)
        _check(self._lib, rc)
        return (adj, fused, out_ids, lv, bits) if reweighted else (fused, out_ids, lv, bits)

    # -- sparse-vector search (Milvus SPARSE_FLOAT_VECTOR, metric IP) --------------------------------------
    def sparse(self, row_off, terms, vals, vocab: int, max_nq: int = 1024, max_k: int = MAX_K) -> "IcdSparse":
        """A sparse index over this index's rows (icd_sparse_create): CSR rows (row_off int64 [n + 1], terms uint32, vals
        float32; strictly increasing terms below vocab, finite non-zero values), with the workspace of searches of up to max_nq
        queries at k <= max_k."""
        if self.closed:
            raise IcdError(-5, "index is closed")
        return IcdSparse(self, row_off, terms, vals, int(vocab), int(max_nq), int(max_k))

    def search_sparse(self, sp: "IcdSparse", q_off, q_terms, q_vals, k: int, masks=None, reweighted: bool = False, validate: bool = True,
                      grouping: Optional["IcdGrouping"] = None, group_size: int = 1, radius=None, range_filter=None, after=None):
        """The best k rows by sparse inner product among the rows that share a term with the query (icd_sparse_search). Queries
        in CSR form (q_off int64 [nq + 1], q_terms uint32, q_vals float32; at most 64 strictly increasing terms each): numpy
        arrays - checked by the library, host outputs - or torch CUDA tensors (int64 / int32 holding the uint32 bit patterns /
        float32), device tensors out on torch's current stream. The library cannot read device queries, so with validate=True
        (the default) they are copied to the host and checked there first: that SYNCHRONISES, and the call is not
        graph-capturable. validate=False skips the copy for queries the caller has already checked (check_sparse_rows): the
        call then only enqueues and, without masks, can be captured; the kernel trusts strictly increasing terms. masks: None, ONE IcdRowMask for
        every query, or nq of IcdRowMask or None. reweighted: (adj f64, raw f32, ids i64, levels i32) in search_reweighted's
        order, else (raw, ids, levels) best first; padding -inf, -1, 0.
        grouping (an IcdGrouping of this index) / group_size: the grouped form (icd_sparse_search_grouped) - the k best GROUPS
        among the hits and the group_size best hit rows of each, outputs [nq, k * group_size] with the hits' group ids as one
        more array at the end, layout and padding (-inf, -1, 0, -1) as search_grouped. Masks are allowed. The first grouped call
        of a grouping pairs it with the sparse index (one launch, n * 4 bytes the grouping then owns).
        radius / range_filter / after=(scores, ids): search_range's band on the sparse ranking (icd_sparse_search_range) - only hits
        with radius < score <= range_filter ranked strictly behind the cursor hit; scalars (broadcast) or one value per query
        (arrays / CUDA tensors; with device queries the bounds are moved to the device). A row without a shared term is no hit
        under any band. Any bound next to `grouping` is a ValueError; with no bound the call above runs untouched."""
        if self.closed or sp is None or sp.closed:
            raise IcdError(-5, "index or sparse index is closed")
        group_size = _check_group_args(grouping, k, group_size)
        a_sc, a_id = (None, None) if after is None else after
        if (a_sc is None) != (a_id is None):
            raise ValueError("after = (scores, ids): both or neither")
        banded = radius is not None or range_filter is not None or a_sc is not None
        if banded and grouping is not None:
            raise ValueError("radius / range_filter / after cannot be combined with grouping")
        on_dev = _is_torch_tensor(q_off) and q_off.is_cuda
        if on_dev:
            import torch
            off = q_off.to(torch.int64).contiguous().reshape(-1)
            tr = q_terms.contiguous().reshape(-1)
            if tr.dtype not in (torch.int32, getattr(torch, "uint32", torch.int32)):
                tr = tr.to(torch.int64).to(torch.int32)   # (values up to 2^32 - 1 wrap into the same bit patterns)
            vl = q_vals.to(torch.float32).contiguous().reshape(-1)
            nq, n_terms = int(off.numel()) - 1, int(tr.numel())
            if nq < 0 or n_terms != int(vl.numel()):
                raise ValueError("q_off must hold nq + 1 offsets; q_terms and q_vals one entry per pair")
            if validate:   # (device -> host copies: a synchronisation)
                check_sparse_rows(off.cpu().numpy(), tr.cpu().numpy().view(np.uint32), vl.cpu().numpy(), sp.vocab, SPARSE_MAX_QUERY_TERMS, "query")
        else:   # (a host caller's queries are checked by icd_sparse_search itself)
            off = np.ascontiguousarray(np.asarray(q_off).reshape(-1), dtype=np.int64)
            tr = np.ascontiguousarray(np.asarray(q_terms).reshape(-1), dtype=np.uint32)
            vl = np.ascontiguousarray(np.asarray(q_vals).reshape(-1), dtype=np.float32)
            nq, n_terms = int(off.size) - 1, int(tr.size)
            if nq < 0 or n_terms != vl.size or (nq > 0 and int(off[-1]) != n_terms):
                raise ValueError("q_off must hold nq + 1 offsets that end at the number of terms and values")
        k = int(k)
        mask_h = None if masks is None else _mask_table(masks, nq, f"{nq} queries", "query")
        if grouping is not None:
            grouping.pair_sparse(self, sp)   # (behind every argument check of this layer: a refused call leaves the grouping as it was)
        outs, ptr, stream, dev = _outputs(on_dev, self.device, (nq, k * group_size), _SPARSE_OUTS if grouping is None else _SPARSE_OUTS_GROUPED)
        bounds = ()
        if banded:
            bounds = [None if v is None else _bound(v, dt, (nq,), on_dev, self.device)   # (kept alive over the call)
                      for v, dt in ((radius, np.float32), (range_filter, np.float32), (a_sc, np.float32), (a_id, np.int64))]
        if nq:   # what the three entry points share, once: the queries, the mask table, the outputs (no tuples: this is the nq = 1 path too)
            p_off = ptr(off)
            p_tr, p_vl = (ptr(tr), ptr(vl)) if n_terms else (p_off, p_off)
            p_mask, rw = None if mask_h is None else mask_h.ctypes.data, 1 if reweighted else 0
            p_adj, p_raw, p_ids, p_lv = ptr(outs[0]) if reweighted else None, ptr(outs[1]), ptr(outs[2]), ptr(outs[3])
            if grouping is not None:
                rc = self._lib.icd_sparse_search_grouped(self._h, sp._h, grouping._h, p_off, p_tr, p_vl, nq, k, group_size, dev, p_mask,
                                                         rw, p_adj, p_raw, p_ids, p_lv, ptr(outs[4]), dev, stream)
            elif banded:
                rc = self._lib.icd_sparse_search_range(self._h, sp._h, p_off, p_tr, p_vl, nq, k, dev, p_mask,
                                                       *[None if b is None else ptr(b) for b in bounds], dev, rw, p_adj, p_raw, p_ids, p_lv, dev, stream)
            else:
                rc = self._lib.icd_sparse_search(self._h, sp._h, p_off, p_tr, p_vl, nq, k, dev, p_mask, rw, p_adj, p_raw, p_ids, p_lv, dev, stream)
            _check_inv(self._lib, rc)
        return tuple(outs) if reweighted else tuple(outs[1:])

    def _produce_masks(self, nq, base_masks, call) -> list:
        """what match_masks and filter_masks share: the base table, the handles' out array, call(base, out) -> rc with ICD_ERR_INVALID
        as a ValueError, and the nq handles adopted as IcdRowMask"""
        base_h = None if base_masks is None else _mask_table(base_masks, nq, f"{nq} queries", "query")   # (kept alive over the call)
        if nq == 0:
            return []
        out = (C.c_void_p * nq)()
        rc = call(None if base_h is None else base_h.ctypes.data, C.cast(out, C.c_void_p))
        _check_inv(self._lib, rc)
        return [IcdRowMask._adopt(self, out[q]) for q in range(nq)]

    def match_masks(self, sp: "IcdSparse", q_off, q_terms, min_match, base_masks=None) -> list:
        """The row masks of a batch of keyword matches (icd_sparse_match_rowmasks), one IcdRowMask per query,
        built on the device from the sparse index's postings in one launch: row r is in mask q iff it holds at least
        min_match[q] (1 .. 64) of the terms q_terms[q_off[q] : q_off[q + 1]] (uint32, strictly increasing, below the vocabulary,
        at most 64) and lies in base_masks[q] (None, ONE IcdRowMask for every query, or nq of IcdRowMask or None). Host arrays,
        checked by the library (ValueError). The masks are ordinary row masks of this index: every masked search takes them;
        close() them (or drop them) when the search they were made for is done."""
        if self.closed or sp is None or sp.closed:
            raise IcdError(-5, "index or sparse index is closed")
        off = np.ascontiguousarray(np.asarray(q_off).reshape(-1), dtype=np.int64)
        tr = np.ascontiguousarray(np.asarray(q_terms).reshape(-1), dtype=np.uint32)
        mm = np.ascontiguousarray(np.asarray(min_match).reshape(-1), dtype=np.int32)
        nq = int(off.size) - 1
        if nq < 0 or mm.size != nq or (nq > 0 and int(off[-1]) != tr.size):
            raise ValueError("q_off must hold nq + 1 offsets that end at the number of terms; min_match one entry per query")
        return self._produce_masks(nq, base_masks, lambda base, out: self._lib.icd_sparse_match_rowmasks(
            self._h, sp._h, off.ctypes.data, tr.ctypes.data if tr.size else off.ctypes.data, mm.ctypes.data, nq, 0, base, out, None))

    def columns(self, cols) -> "IcdColumns":
        """int32 columns of this index's rows on the device (icd_columns_*): cols [ncols, n]"""
        return IcdColumns(self, cols)

    def filter_masks(self, columns: "IcdColumns", sparse, prog_off, prog, base_masks=None) -> list:
        """The row masks of a batch of filter programs (icd_filter_rowmasks), one IcdRowMask per query, built
        on the device in one launch: query q's program is the uint32 words prog[prog_off[q] : prog_off[q + 1]] in
        include/icd_search.h's layout (services/filter_expr.device_program writes them) over `columns` and - for TEXT leaves -
        the sparse index `sparse` (None: no program holds one). base_masks: None, ONE IcdRowMask for every query, or nq of
        IcdRowMask or None, ANDed in. Host arrays, checked by the library (ValueError). The masks are ordinary row masks of this
        index: every masked search takes them; close() them (or drop them) when the search they were made for is done."""
        if self.closed or columns is None or columns.closed or (sparse is not None and sparse.closed):
            raise IcdError(-5, "index, columns or sparse index is closed")
        off = np.ascontiguousarray(np.asarray(prog_off).reshape(-1), dtype=np.int64)
        pr = np.ascontiguousarray(np.asarray(prog).reshape(-1), dtype=np.uint32)
        nq = int(off.size) - 1
        if nq < 0 or (nq > 0 and int(off[-1]) != pr.size):
            raise ValueError("prog_off must hold nq + 1 offsets that end at the number of program words")
        return self._produce_masks(nq, base_masks, lambda base, out: self._lib.icd_filter_rowmasks(
            self._h, columns._h, None if sparse is None else sparse._h, off.ctypes.data, pr.ctypes.data if pr.size else off.ctypes.data, nq,
            base, out, None))

    def select_rows(self, masks, limit: int, offsets=None, *, on_device: bool = False):
        """The ordered select over a batch of row masks (icd_rowmask_select), a Milvus query / count(*) /
        query_iterator page per entry: masks is a sequence of IcdRowMask or None (None: every row of the index), offsets None (0),
        one int for every query or one per query (>= 0), limit 1 .. SELECT_MAX_LIMIT. Returns (ids int64 [nq, limit], total int64
        [nq], taken int32 [nq]): total[q] the rows of mask q, taken[q] = clamp(total - offset, 0, limit), ids[q] the rows of
        ranks offset .. offset + taken of the mask in ascending order, then -1. numpy arrays; on_device=True: torch tensors on
        the index's device, enqueued on torch's current stream, no synchronisation. Two launches whatever the batch holds; the same
        bytes on every run. At most max_nq masks per call. Bad arguments raise ValueError."""
        if self.closed:
            raise IcdError(-5, "index is closed")
        masks = list(masks)
        nq, limit = len(masks), int(limit)
        if not 1 <= limit <= SELECT_MAX_LIMIT:
            raise ValueError(f"limit={limit}: 1 .. {SELECT_MAX_LIMIT}")
        table = _mask_table(masks, nq, f"{nq} queries", "query")   # (kept alive over the call)
        off = None
        if offsets is not None:
            off = np.ascontiguousarray(np.asarray(offsets, dtype=np.int64).reshape(-1))
            if off.size == 1:
                off = np.full(nq, off[0], np.int64)
            if off.size != nq:
                raise ValueError(f"offsets holds {off.size} entries for {nq} queries")
        # host outputs go through the staging the index allocated (ms_host_slots); a larger call writes device tensors and copies them
        through = on_device or nq * limit > max(64 * self.max_nq, 4 * SELECT_MAX_LIMIT)
        (ids,), ptr, stream, dev = _outputs(through, self.device, (nq, limit), (np.int64,))
        (total,), _, _, _ = _outputs(through, self.device, (nq,), (np.int64,))
        (taken,), _, _, _ = _outputs(through, self.device, (nq,), (np.int32,))
        if nq:
            rc = self._lib.icd_rowmask_select(self._h, table.ctypes.data, nq, None if off is None else off.ctypes.data, limit, ptr(ids),
                                              ptr(total), ptr(taken), dev, stream)
            _check_inv(self._lib, rc)
        if through and not on_device:
            return ids.cpu().numpy(), total.cpu().numpy(), taken.cpu().numpy()
        return ids, total, taken

    def count_rows(self, masks, *, on_device: bool = False):
        """total of select_rows alone (int64 [nq]; numpy, or a torch tensor on the index's device when on_device): the count pass
        and the totals, no row is written"""
        if self.closed:
            raise IcdError(-5, "index is closed")
        masks = list(masks)
        nq = len(masks)
        table = _mask_table(masks, nq, f"{nq} queries", "query")
        (total,), ptr, stream, dev = _outputs(on_device, self.device, (nq,), (np.int64,))
        if nq:
            rc = self._lib.icd_rowmask_select(self._h, table.ctypes.data, nq, None, 1, None, ptr(total), None, dev, stream)
            _check_inv(self._lib, rc)
        return total

    def group_counts(self, masks, grouping: "IcdGrouping", *, on_device: bool = False):
        """Facet counts (icd_rowmask_group_counts): int32 [nq, G], counts[q][j] = the rows of masks[q] whose
        group is grouping.group_ids[j]. masks is a sequence of IcdRowMask or None (None: every row of the index, so the row of
        counts is the group sizes). A numpy array; on_device=True: a torch tensor on the index's device, enqueued on torch's
        current stream, no synchronisation. One launch whatever the batch holds; exact integers, the same bytes on every run; a
        row sums to count_rows of its mask. At most max_nq masks per call. Bad arguments raise ValueError."""
        if self.closed or grouping is None or grouping.closed:
            raise IcdError(-5, "index or grouping is closed")
        masks = list(masks)
        nq = len(masks)
        table = _mask_table(masks, nq, f"{nq} queries", "query")   # (kept alive over the call)
        (counts,), ptr, stream, dev = _outputs(on_device, self.device, (nq, grouping.groups), (np.int32,))
        if nq:
            rc = self._lib.icd_rowmask_group_counts(self._h, grouping._h, table.ctypes.data, nq, ptr(counts), dev, stream)
            _check_inv(self._lib, rc)
        return counts

    def lookup_levels(self, ids):
        """Levels of hit ids (torch CUDA int64 tensor) -> int32 tensor; ids < 0 give 0."""
        import torch
        ids = ids.contiguous()
        out = torch.empty(ids.shape, dtype=torch.int32, device=ids.device)
        _check(self._lib, self._lib.icd_index_lookup_levels(self._h, ids.data_ptr(), ids.numel(), out.data_ptr(),
                                                            _current_stream_ptr(self.device)))
        return out

    # -- introspection -------------------------------------------------------------------------------
    def stats(self) -> dict:
        st = _Stats()
        _check(self._lib, self._lib.icd_index_stats(self._h, C.byref(st)))
        return {f: getattr(st, f) for f, _ in _Stats._fields_}

    def cert_terms(self, count: int = 0) -> dict:
        """the measured terms of the certificate's error bound, in the fp16 image's scaled units: `cmax`
        and `dcmax` of the corpus, `cexp`, and `qnorm` / `qres` of the first `count` queries of the last AUTO batch search"""
        cmax, dcmax, cexp = C.c_float(), C.c_float(), C.c_int32()
        qnorm, qres = np.zeros(max(count, 1), np.float32), np.zeros(max(count, 1), np.float32)
        _check(self._lib, self._lib.icd_index_cert_terms(self._h, C.addressof(cmax), C.addressof(dcmax), C.addressof(cexp),
                                                        qnorm.ctypes.data, qres.ctypes.data, int(count)))
        return {"cmax": cmax.value, "dcmax": dcmax.value, "cexp": cexp.value, "qnorm": qnorm[:count], "qres": qres[:count]}

    def set_chunks(self, chunks: int):
        _check(self._lib, self._lib.icd_index_set_chunks(self._h, int(chunks)))

    def set_second_pass(self, enabled, adaptive: bool = True):
        """test / A-B switch: the second coarse pass over uncertified queries (default on), and the adaptive list count of
        large batches that follows from its counters"""
        _check(self._lib, self._lib.icd_index_set_second_pass(self._h, 0 if not enabled else (1 if adaptive else 2)))

    def set_option(self, name: str, value: int):
        """A/B and test options of this index (icd_index_set_option; `name` one of OPTIONS): family_order, stream_one, host_one,
        pacing_shift, pacing_lead, exact_narrow - performance decisions only, results are identical whatever they are set to"""
        _check(self._lib, self._lib.icd_index_set_option(self._h, OPTIONS[name], int(value)))

    def set_profiling(self, enabled, every: int = 1):
        """hipEvents around the kernels of every `every`-th search (read back by profile_summary / last_profile)"""
        _check(self._lib, self._lib.icd_index_set_profiling(self._h, max(1, int(every)) if enabled else 0))

    def last_profile(self) -> dict:
        p = _Profile()
        _check(self._lib, self._lib.icd_index_last_profile(self._h, C.byref(p)))
        return {f: float(getattr(p, f)) for f, _ in _Profile._fields_}


class IcdGrouping(_Handle):
    """Rows of one IcdIndex ordered by group, with the workspace of the grouped searches (icd_grouping_*). Independent of the
    index's lifetime: either may be closed first (a search with a closed partner raises)."""
    _destroy = "icd_grouping_destroy"

    def __init__(self, index: "IcdIndex", group_of, max_nq: int):
        self._lib = index._lib
        self._h = C.c_void_p()
        keep = None
        if _is_torch_tensor(group_of) and group_of.is_cuda:
            import torch
            keep = group_of.to(torch.int32).contiguous().reshape(-1)
            if keep.device.index != index.device:
                raise ValueError(f"group_of on cuda:{keep.device.index}, index on device {index.device}")
            torch.cuda.synchronize(index.device)
            ptr, on_dev, n = keep.data_ptr(), 1, int(keep.numel())
        else:
            if _is_torch_tensor(group_of):
                group_of = group_of.detach().cpu().numpy()
            g64 = np.asarray(group_of).reshape(-1)
            if g64.size and (g64.min() < 0 or g64.max() > 0x7FFFFFFF):
                raise ValueError("group ids must be integers in 0 .. 2^31 - 1")
            keep = np.ascontiguousarray(g64, dtype=np.int32)
            ptr, on_dev, n = keep.ctypes.data, 0, int(keep.size)
        if n != index.n:
            raise ValueError(f"group_of holds {n} ids, the index {index.n} rows")
        self.n, self.max_nq, self.device = n, int(max_nq), index.device
        _check(self._lib, self._lib.icd_grouping_create(index._h, ptr, n, on_dev, self.max_nq, C.byref(self._h)))
        self._paired = False
        self._scorers = False
        self.maxsim = None   # (max_lists, max_vectors) once prepare_maxsim has run
        self._group_of, self._group_ids = keep, None   # (kept until group_ids is first asked for)
        self.groups = int(self.stats()["groups"])

    @property
    def group_ids(self) -> np.ndarray:
        """the sorted distinct ids of group_of (int32 [groups]): entry j is the group of column j of IcdIndex.group_counts, the
        dense number icd_grouping_create assigns"""
        if self._group_ids is None:
            ids = self._group_of
            ids = ids.cpu().numpy() if _is_torch_tensor(ids) else ids
            self._group_ids = np.unique(ids).astype(np.int32)
            self._group_ids.setflags(write=False)
            self._group_of = None
        return self._group_ids

    def pair_sparse(self, index: "IcdIndex", sp: "IcdSparse"):
        """The one-time pairing with a sparse index of the same IcdIndex (icd_grouping_pair_sparse): the grouping's row ->
        position table. search_sparse issues it at a grouping's first grouped call; later calls return at once."""
        if self._paired:
            return
        if self.closed or index.closed or sp.closed:
            raise IcdError(-5, "index, grouping or sparse index is closed")
        _check(self._lib, self._lib.icd_grouping_pair_sparse(index._h, self._h, sp._h))
        self._paired = True

    def prepare_scorers(self, index: "IcdIndex"):
        """The one-time preparation for the group scorers (icd_grouping_prepare_scorers): the plan that cuts the grouping's rows
        into per-wave work along group boundaries, counted in stats()["bytes"] from then on. search_grouped issues it at a
        grouping's first scored call; later calls return at once. It allocates: refused while torch's current stream is being
        captured into a graph - prepare first, then capture."""
        if self._scorers:
            return
        if self.closed or index.closed:
            raise IcdError(-5, "index or grouping is closed")
        torch = sys.modules.get("torch")
        if torch is not None and torch.cuda.is_available() and torch.cuda.is_current_stream_capturing():
            raise IcdError(-1, "prepare_scorers allocates: it cannot run while a graph is being captured (prepare the grouping first)")
        _check(self._lib, self._lib.icd_grouping_prepare_scorers(index._h, self._h))
        self._scorers = True

    def prepare_maxsim(self, index: "IcdIndex", max_lists: int, max_vectors: int):
        """The one-time preparation for the embedding-list search (icd_grouping_prepare_maxsim): the block of the lists'
        aggregates and a host caller's staging for calls of up to max_lists lists holding max_vectors vectors in all (at least 64:
        one full list), counted in stats()["bytes"] from then on. search_lists issues it at a grouping's first call with the
        grouping's max_nq for both; a repeated call within the prepared sizes returns at once. It allocates: refused while
        torch's current stream is being captured into a graph - prepare first, then capture."""
        max_lists, max_vectors = int(max_lists), int(max_vectors)
        if max_lists < 1 or max_vectors < max(max_lists, MAXSIM_MAX_T):
            raise ValueError(f"max_lists={max_lists}, max_vectors={max_vectors}: need max_lists >= 1 and max_vectors >= max(max_lists, {MAXSIM_MAX_T})")
        if self.maxsim is not None and max_lists <= self.maxsim[0] and max_vectors <= self.maxsim[1]:
            return
        if self.closed or index.closed:
            raise IcdError(-5, "index or grouping is closed")
        torch = sys.modules.get("torch")
        if torch is not None and torch.cuda.is_available() and torch.cuda.is_current_stream_capturing():
            raise IcdError(-1, "prepare_maxsim allocates: it cannot run while a graph is being captured (prepare the grouping first)")
        _check(self._lib, self._lib.icd_grouping_prepare_maxsim(index._h, self._h, max_lists, max_vectors))
        self.maxsim = (max_lists, max_vectors)

    def stats(self) -> dict:
        if self.closed:
            raise IcdError(-5, "grouping is closed")
        g, m, b = C.c_int64(), C.c_int64(), C.c_int64()
        _check(self._lib, self._lib.icd_grouping_stats(self._h, C.byref(g), C.byref(m), C.byref(b)))
        return {"groups": g.value, "largest_group": m.value, "bytes": b.value}


class _Workspace(_Handle):
    """A sized workspace of one IcdIndex behind icd_<_prefix>_create / _stats / _destroy. A subclass names the prefix, the noun of
    its closed message and the key its size goes by - in stats() and as the attribute that holds it (max_nq or max_total)."""
    _prefix = _noun = _size_key = ""

    def __init__(self, index: "IcdIndex", size: int):
        self._lib = index._lib
        self._h = C.c_void_p()
        setattr(self, self._size_key, int(size))
        _check(self._lib, getattr(self._lib, f"icd_{self._prefix}_create")(index._h, int(size), C.byref(self._h)))

    def stats(self) -> dict:
        if self.closed:
            raise IcdError(-5, f"{self._noun} is closed")
        t, b = C.c_int64(), C.c_int64()
        _check(self._lib, getattr(self._lib, f"icd_{self._prefix}_stats")(self._h, C.byref(t), C.byref(b)))
        return {self._size_key: t.value, "bytes": b.value}


class IcdFusion(_Workspace):
    """The workspace of one IcdIndex's hybrid searches (icd_fusion_*): staging for max_total = nq * R sub-lists of 128 hits and
    for host callers. Independent of the index's lifetime: either may be closed first (a search with a closed partner raises)."""
    _prefix, _noun, _size_key, _destroy = "fusion", "fusion", "max_total", "icd_fusion_destroy"

    def __init__(self, index: "IcdIndex", max_total: int):
        super().__init__(index, max_total)
        self.device = index.device


class IcdMmr(_Workspace):
    """The workspace of one IcdIndex's MMR searches (icd_mmr_*): the staging of max_nq candidate lists of 128 hits and of a host
    caller's outputs."""
    _prefix, _noun, _size_key, _destroy = "mmr", "mmr workspace", "max_nq", "icd_mmr_destroy"


class IcdByRows(_Workspace):
    """The workspace of one IcdIndex's searches by rows (icd_byrows_*): the query block the rows are gathered into, the
    (k + 1)-wide lists of max_nq queries and a host caller's ids and outputs. Independent of the index's lifetime: either may be
    closed first (a search with a closed partner raises)."""
    _prefix, _noun, _size_key, _destroy = "byrows", "by-rows workspace", "max_nq", "icd_byrows_destroy"


class IcdRankOf(_Handle):
    """The workspace of one IcdIndex's rank-of calls (icd_rankof_*) and the call itself: IcdRankOf(index, max_nq).rank_of(...). It
    holds a host caller's queries, the targets of max_nq queries, their keys and the outputs. Independent of the index's lifetime:
    either may be closed first (a call with a closed partner raises). It is made and asked like every sized workspace -
    _Workspace's own constructor and stats(), not a copy of them."""
    _prefix, _noun, _size_key, _destroy = "rankof", "rank-of workspace", "max_nq", "icd_rankof_destroy"
    stats = _Workspace.stats

    def __init__(self, index: "IcdIndex", max_nq: Optional[int] = None):
        if index.closed:
            raise IcdError(-5, "index is closed")
        _Workspace.__init__(self, index, index.max_nq if max_nq is None else max_nq)
        self._index = index

    def rank_of(self, queries, targets, masks=None):
        """The exact rank of given ids in every query's ranking (icd_index_rank_of). queries: [nq, dim], a numpy array or a torch
        CUDA tensor; targets: int64 [nq, nt] global ids (or [nq]: one per query), 1 <= nt <= RANKOF_MAX_TARGETS, -1 = padding;
        masks: None, one IcdRowMask for every query, or nq entries of IcdRowMask or None. Returns numpy arrays (rank i64 [nq, nt],
        adj f64, raw f32, levels i32, selected i64 [nq]): rank = the rows of the query's mask that stand strictly ahead of the
        target in search_masked's raw order (score desc, id asc) - the position search_masked(reweighted=False) returns the id
        at, for any k and past it - adj / raw the bits the search reports for that row, selected the rows the mask admits. No
        rank (-1, NaN scores): padding, an id outside the index, a row outside its mask; a NaN-scored target has rank -1 too.
        A batch longer than the workspace's max_nq runs in chunks. The call synchronises."""
        index = self._index
        if index.closed or self.closed:
            raise IcdError(-5, "index or rank-of workspace is closed")
        q, q_dev = index._prep_queries(queries)
        if q.ndim != 2 or q.shape[-1] != index.dim:
            raise ValueError(f"queries must be [nq, {index.dim}], got {tuple(q.shape)}")
        nq = int(q.shape[0])
        if _is_torch_tensor(targets):
            targets = targets.detach().cpu().numpy()
        tg = np.asarray(targets)
        if tg.dtype.kind not in "iu":
            raise ValueError("targets: integer ids")
        if tg.ndim <= 1:
            tg = tg.reshape(nq, -1) if nq else tg.reshape(0, 1)
        tg = np.ascontiguousarray(tg, dtype=np.int64)
        if tg.ndim != 2 or tg.shape[0] != nq or not (1 <= tg.shape[1] <= RANKOF_MAX_TARGETS):
            raise ValueError(f"targets must be [{nq}, 1 .. {RANKOF_MAX_TARGETS}], got {tuple(tg.shape)}")
        nt = int(tg.shape[1])
        table = None if masks is None else _mask_table(masks, nq, f"{nq} queries", "query")
        qptr = _dev_ptr if q_dev else _host_ptr
        stream = _current_stream_ptr(index.device) if q_dev else None

        def call(qs, s0):
            m = qs.shape[0]
            rank, adj, raw, lv = (np.empty((m, nt), dt) for dt in (np.int64, np.float64, np.float32, np.int32))
            sel = np.empty(m, np.int64)
            if m:
                _check(self._lib, self._lib.icd_index_rank_of(
                    index._h, self._h, qptr(qs), m, 1 if q_dev else 0, tg[s0:s0 + m].ctypes.data, nt,
                    None if table is None else table.ctypes.data + 8 * s0,
                    rank.ctypes.data, adj.ctypes.data, raw.ctypes.data, lv.ctypes.data, sel.ctypes.data, stream))
            return rank, adj, raw, lv, sel
        return _chunked(q, self.max_nq if table is None else min(index.max_nq, self.max_nq), False, call)


class IcdWide(_Handle):
    """The workspace of one IcdIndex's wide searches (icd_wide_*) and the call itself: IcdWide(index, max_nq, max_k).search_wide(...).
    It holds the score block, the candidate block, the threshold records and a host caller's queries, bounds and outputs for calls
    of up to max_nq queries and first + k up to max_k. Independent of the index's lifetime: either may be closed first (a call
    with a closed partner raises). IcdIndex's public surface is recorded and stays as it is, so - as with IcdRankOf - workspace
    and call stand beside it."""
    _destroy = "icd_wide_destroy"

    def __init__(self, index: "IcdIndex", max_nq: Optional[int] = None, max_k: int = WIDE_MAX_K):
        if index.closed:
            raise IcdError(-5, "index is closed")
        self._lib = index._lib
        self._h = C.c_void_p()
        self.max_nq = int(index.max_nq if max_nq is None else max_nq)
        self.max_k = int(max_k)
        _check(self._lib, self._lib.icd_wide_create(index._h, self.max_nq, self.max_k, C.byref(self._h)))
        self._index = index

    def stats(self) -> dict:
        if self.closed:
            raise IcdError(-5, "wide-search workspace is closed")
        q, k, b = C.c_int64(), C.c_int64(), C.c_int64()
        _check(self._lib, self._lib.icd_wide_stats(self._h, C.byref(q), C.byref(k), C.byref(b)))
        return {"max_nq": q.value, "max_k": k.value, "bytes": b.value}

    def search_wide(self, queries, k: int, *, masks=None, radius=None, range_filter=None, first: int = 0, reweighted: bool = True):
        """Ranks first .. first + k - 1 of every query's exact ranking, first + k <= WIDE_MAX_K (icd_index_search_wide). queries:
        [nq, dim], a numpy array or a torch CUDA tensor; masks: None, one IcdRowMask for every query, or nq entries of IcdRowMask
        or None; radius / range_filter: None, a scalar or one value per query (radius < score <= range_filter). Returns
        (adj f64, raw f32, ids i64, levels i32) [nq, k], count i32 [nq] and selected i64 [nq]: reweighted=True in
        search_reweighted's order (level weight, one stable re-sort of the slice); False: adj is None and the rest is in raw order
        (score desc, id asc). Padding: -inf, id -1, level 0. count: the real hits of the slice; selected: the rows that rank
        (mask, band, no NaN) - the total behind the page. Numpy in -> numpy out; device tensors in -> device tensors out on
        torch's current stream. A batch longer than the workspace's max_nq runs in chunks."""
        index = self._index
        if index.closed or self.closed:
            raise IcdError(-5, "index or wide-search workspace is closed")
        q, on_dev = index._prep_queries(queries)
        if q.ndim != 2 or q.shape[-1] != index.dim:
            raise ValueError(f"queries must be [nq, {index.dim}], got {tuple(q.shape)}")
        k, first = int(k), int(first)
        if k < 1 or first < 0 or first + k > WIDE_MAX_K:
            raise ValueError(f"k={k}, first={first}: need k >= 1, first >= 0 and first + k <= {WIDE_MAX_K}")
        nq = int(q.shape[0])
        bands = _Bands(masks, nq, f"{nq} queries", "query")
        bands.bound(((radius, np.float32), (range_filter, np.float32)), on_dev, index.device)

        def call(qs, s0):
            m = qs.shape[0]
            (adj, raw, ids, lv), ptr, stream, dev = _outputs(on_dev, index.device, (m, k), (np.float64, np.float32, np.int64, np.int32))
            (count, sel), _p, _s, _d = _outputs(on_dev, index.device, (m,), (np.int32, np.int64))
            if m:
                p_mask, (p_lo, p_hi) = bands.at(s0, m, ptr)
                _check(self._lib, self._lib.icd_index_search_wide(
                    index._h, self._h, p_mask, ptr(qs), m, k, first, dev, p_lo, p_hi, dev, 1 if reweighted else 0,
                    ptr(adj) if reweighted else None, ptr(raw), ptr(ids), ptr(lv), ptr(count), ptr(sel), dev, stream))
            return (adj, raw, ids, lv, count, sel)
        out = _chunked(q, self.max_nq if bands.table is None else min(index.max_nq, self.max_nq), on_dev, call)
        return out if reweighted else (None,) + tuple(out[1:])


class IcdRecommend(_Handle):
    """The workspace of one IcdIndex's recommend searches (icd_recommend_*) and the call itself:
    IcdRecommend(index, max_requests, max_examples, max_k).recommend(...). It holds the example block and its scores, the request
    block, the candidate block, the request table and a host caller's vectors, bounds and outputs for calls of up to max_requests
    requests with up to max_examples examples in all (default: 16 per request) and first + k up to max_k. Independent of the
    index's lifetime: either may be closed first (a call with a closed partner raises). IcdIndex's public surface is recorded and
    stays as it is, so - as with IcdWide - workspace and call stand beside it."""
    _destroy = "icd_recommend_destroy"

    def __init__(self, index: "IcdIndex", max_requests: Optional[int] = None, max_examples: Optional[int] = None, max_k: int = 128):
        if index.closed:
            raise IcdError(-5, "index is closed")
        self._lib = index._lib
        self._h = C.c_void_p()
        self.max_requests = int(index.max_nq if max_requests is None else max_requests)
        self.max_examples = int(self.max_requests * RECOMMEND_MAX_EXAMPLES if max_examples is None else max_examples)
        self.max_k = int(max_k)
        _check(self._lib, self._lib.icd_recommend_create(index._h, self.max_requests, self.max_examples, self.max_k, C.byref(self._h)))
        self._index = index

    def stats(self) -> dict:
        if self.closed:
            raise IcdError(-5, "recommend workspace is closed")
        r, e, k, b = C.c_int64(), C.c_int64(), C.c_int64(), C.c_int64()
        _check(self._lib, self._lib.icd_recommend_stats(self._h, C.byref(r), C.byref(e), C.byref(k), C.byref(b)))
        return {"max_requests": r.value, "max_examples": e.value, "max_k": k.value, "bytes": b.value}

    def last_vectors(self, count: int) -> np.ndarray:
        """the first `count` vectors the last call's last block built on the device (icd_recommend_read_vectors): under
        "average_vector" the requests' targets, else the examples' vectors. float32 [count, dim]; synchronises. For tests."""
        if self.closed:
            raise IcdError(-5, "recommend workspace is closed")
        out = np.empty((int(count), self._index.dim), np.float32)
        _check(self._lib, self._lib.icd_recommend_read_vectors(self._h, int(count), out.ctypes.data))
        return out

    def _pack(self, positive, negative):
        """the requests of a call in the C ABI's form: rows int64 [ne] (a stored example's row, -1 for a vector), off int64
        [nr + 1], npos int32 [nr], the vector examples by their place in the example order, and whether they are CUDA tensors"""
        index = self._index
        positive = list(positive)
        negative = [()] * len(positive) if negative is None else list(negative)
        if len(negative) != len(positive):
            raise ValueError(f"negative holds {len(negative)} entries for {len(positive)} requests")
        rows, off, npos, vectors, on_dev = [], [0], [], {}, None
        for r, (pos, neg) in enumerate(zip(positive, negative)):
            pos, neg = list(pos), list(neg)
            if not 1 <= len(pos) + len(neg) <= RECOMMEND_MAX_EXAMPLES:
                raise ValueError(f"request {r} holds {len(pos) + len(neg)} examples: 1 .. {RECOMMEND_MAX_EXAMPLES}")
            for ex in pos + neg:
                if isinstance(ex, (int, np.integer)) and not isinstance(ex, bool):
                    row = int(ex) - index.id_base
                    if not 0 <= row < index.n:
                        raise ValueError(f"request {r}: id {int(ex)} is outside the index")
                    rows.append(row)
                    continue
                dev = _is_torch_tensor(ex) and ex.is_cuda
                if _is_torch_tensor(ex) and not dev:
                    ex = ex.detach().numpy()
                if not dev:
                    ex = np.asarray(ex, np.float32)
                if ex.ndim != 1 or ex.shape[0] != index.dim:
                    raise ValueError(f"request {r}: an example is an int id or a vector of {index.dim} floats, got shape {tuple(ex.shape)}")
                if on_dev is not None and on_dev != dev:
                    raise ValueError("example vectors: numpy arrays or CUDA tensors, not both")
                on_dev = dev
                vectors[len(rows)] = ex
                rows.append(-1)
            off.append(len(rows))
            npos.append(len(pos))
        return np.asarray(rows, np.int64), np.asarray(off, np.int64), np.asarray(npos, np.int32), vectors, bool(on_dev)

    def recommend(self, positive, negative, strategy: str, k: int, *, masks=None, radius=None, range_filter=None, first: int = 0,
                  reweighted: bool = True):
        """Ranks first .. first + k - 1 of every request's ranking by its examples, first + k <= WIDE_MAX_K (icd_index_recommend;
        DESIGN.md section 28). positive, negative: one sequence of examples per request (negative may be None: no negatives), 1 ..
        16 examples a request; an example is an int (a stored id) or a vector of dim floats (a numpy array or a torch CUDA
        tensor). strategy: "average_vector" (needs a positive), "best_score" or "sum_scores". masks: None, one IcdRowMask for every
        request, or one entry (IcdRowMask or None) per request; radius / range_filter: None, a scalar or one value per request
        (radius < combined score <= range_filter). A request's stored examples never rank. Returns (adj f64, raw f32, ids i64,
        levels i32) [nr, k], count i32 [nr] and selected i64 [nr] as search_wide does, raw being the combined score; reweighted=
        False: adj is None and the rest is in raw order. Numpy in -> numpy out; example vectors as CUDA tensors -> device tensors
        out on torch's current stream. A batch above the workspace's sizes runs in chunks of whole requests."""
        index = self._index
        if index.closed or self.closed:
            raise IcdError(-5, "index or recommend workspace is closed")
        if strategy not in RECOMMEND_STRATEGIES:
            raise ValueError(f"strategy={strategy!r}: one of {sorted(RECOMMEND_STRATEGIES)}")
        k, first = int(k), int(first)
        if k < 1 or first < 0 or first + k > WIDE_MAX_K:
            raise ValueError(f"k={k}, first={first}: need k >= 1, first >= 0 and first + k <= {WIDE_MAX_K}")
        rows, off, npos, vectors, on_dev = self._pack(positive, negative)
        nr = len(npos)
        if strategy == "average_vector" and nr and int(npos.min()) < 1:
            raise ValueError("average_vector needs a positive example in every request")
        bands = _Bands(masks, nr, f"{nr} requests", "request")
        bands.bound(((radius, np.float32), (range_filter, np.float32)), on_dev, index.device)
        vec = None
        if vectors:   # [ne, dim] in the example order; the entries of stored examples are not read
            if on_dev:
                import torch
                vec = torch.zeros((len(rows), index.dim), dtype=torch.float32, device=torch.device("cuda", index.device))
                at = torch.as_tensor(list(vectors), device=vec.device)
                vec[at] = torch.stack([v.to(device=vec.device, dtype=torch.float32) for v in vectors.values()])
            else:
                vec = np.zeros((len(rows), index.dim), np.float32)
                vec[list(vectors)] = np.stack(list(vectors.values()))
        step_r = self.max_requests if bands.table is None else min(index.max_nq, self.max_requests)
        code = RECOMMEND_STRATEGIES[strategy]

        def call(r0, m):
            (adj, raw, ids, lv), ptr, stream, dev = _outputs(on_dev, index.device, (m, k), (np.float64, np.float32, np.int64, np.int32))
            (count, sel), _p, _s, _d = _outputs(on_dev, index.device, (m,), (np.int32, np.int64))
            if m:
                e0, e1 = int(off[r0]), int(off[r0 + m])
                p_mask, (p_lo, p_hi) = bands.at(r0, m, ptr)
                c_off = np.ascontiguousarray(off[r0:r0 + m + 1] - e0)
                c_rows, c_npos = np.ascontiguousarray(rows[e0:e1]), np.ascontiguousarray(npos[r0:r0 + m])
                c_vec = None if vec is None else vec[e0:e1]
                _check(self._lib, self._lib.icd_index_recommend(
                    index._h, self._h, p_mask, c_rows.ctypes.data, None if c_vec is None else ptr(c_vec), c_off.ctypes.data, c_npos.ctypes.data, m,
                    code, k, first, p_lo, p_hi, dev, 1 if reweighted else 0,
                    ptr(adj) if reweighted else None, ptr(raw), ptr(ids), ptr(lv), ptr(count), ptr(sel), dev, dev, stream))
            return (adj, raw, ids, lv, count, sel)
        outs, r0 = [], 0
        while r0 < nr:   # chunks of whole requests inside the workspace's requests and examples
            m = 1
            while r0 + m < nr and m < step_r and off[r0 + m + 1] - off[r0] <= self.max_examples:
                m += 1
            outs.append(call(r0, m))
            r0 += m
        if not outs:
            outs = [call(0, 0)]
        if len(outs) == 1:
            out = outs[0]
        elif on_dev:
            import torch
            out = tuple(torch.cat([o[i] for o in outs]) for i in range(6))
        else:
            out = tuple(np.concatenate([o[i] for o in outs]) for i in range(6))
        return tuple(out) if reweighted else (None,) + tuple(out[1:])


class IcdBoost(_Workspace):
    """The workspace of one IcdIndex's boosted searches (icd_boost_*): the staging of a call's per-query boost table. The owning
    index must outlive its use; close() (or garbage collection) frees it."""
    _prefix, _noun, _size_key, _destroy = "boost", "boost workspace", "max_nq", "icd_boost_destroy"


def sparse_tile_rows() -> int:
    """Rows per tile of the sparse search kernel (icd_sparse_tile_rows: a constant of the build)"""
    return int(load_library().icd_sparse_tile_rows())


def check_sparse_rows(row_off, terms, vals, vocab: int, max_terms: int = 0, unit: str = "row"):
    """The rules of sparse rows / queries in CSR form, in numpy (what icd_sparse_pack and icd_sparse_search check on the host):
    offsets from 0 that never decrease, terms strictly increasing within a row and below vocab, values finite and non-zero, at
    most max_terms (> 0) pairs per row. Raises ValueError."""
    off = np.asarray(row_off, np.int64).reshape(-1)
    t = np.asarray(terms).reshape(-1).astype(np.int64)
    v = np.asarray(vals, np.float32).reshape(-1)
    if off.size < 1 or off[0] != 0 or (np.diff(off) < 0).any() or off[-1] != t.size or t.size != v.size:
        raise ValueError(f"{unit} offsets must start at 0, never decrease and end at the number of terms and values")
    if max_terms > 0 and off.size > 1 and int(np.diff(off).max()) > max_terms:
        raise ValueError(f"a {unit} carries at most {max_terms} terms")
    if t.size == 0:
        return
    if t.min() < 0 or t.max() >= vocab:
        raise ValueError(f"{unit}: a term lies outside the vocabulary's [0, {vocab})")
    inner = np.ones(t.size, bool)
    inner[off[:-1][off[:-1] < t.size]] = False   # the first pair of every row has no predecessor
    if (np.diff(t, prepend=t[0])[inner] <= 0).any():
        raise ValueError(f"{unit}: terms must be strictly increasing")
    if not np.isfinite(v).all() or (v == 0).any():
        raise ValueError(f"{unit}: values must be finite and non-zero")


def sparse_pack(row_off, terms, vals, n: int, vocab: int):
    """The inverted index CSR rows become (icd_sparse_pack, the packer icd_sparse_create runs; no device needed):
    (post_off int64 [vocab + 1], post_row uint32 [nnz], post_val float32 [nnz]), every term's postings by ascending row. Raises
    ValueError for rows the rules refuse."""
    lib = load_library()
    off = np.ascontiguousarray(np.asarray(row_off).reshape(-1), dtype=np.int64)
    t = np.ascontiguousarray(np.asarray(terms).reshape(-1), dtype=np.uint32)
    v = np.ascontiguousarray(np.asarray(vals).reshape(-1), dtype=np.float32)
    if off.size != int(n) + 1 or int(vocab) < 1:
        raise ValueError(f"row_off holds {off.size} offsets for {n} rows (vocab={vocab})")
    if off[0] != 0 or (np.diff(off) < 0).any() or off[-1] != t.size or t.size != v.size:
        raise ValueError("row offsets must start at 0, never decrease and end at the number of terms and values")
    post_off = np.empty(int(vocab) + 1, np.int64)
    post_row = np.empty(max(t.size, 1), np.uint32)
    post_val = np.empty(max(t.size, 1), np.float32)
    rc = lib.icd_sparse_pack(off.ctypes.data, t.ctypes.data if t.size else None, v.ctypes.data if t.size else None, int(n), int(vocab),
                             post_off.ctypes.data, post_row.ctypes.data, post_val.ctypes.data)
    _check_inv(lib, rc)
    return post_off, post_row[:t.size], post_val[:t.size]


class IcdSparse(_Handle):
    """A sparse index over the rows of one IcdIndex (icd_sparse_*): postings on the device and the workspace of its searches.
    Independent of the index's lifetime: either may be closed first (a search with a closed partner raises)."""
    _destroy = "icd_sparse_destroy"

    def __init__(self, index: "IcdIndex", row_off, terms, vals, vocab: int, max_nq: int, max_k: int):
        self._lib = index._lib
        self._h = C.c_void_p()
        off = np.ascontiguousarray(np.asarray(row_off).reshape(-1), dtype=np.int64)
        t = np.ascontiguousarray(np.asarray(terms).reshape(-1), dtype=np.uint32)
        v = np.ascontiguousarray(np.asarray(vals).reshape(-1), dtype=np.float32)
        if off.size != index.n + 1:
            raise ValueError(f"row_off holds {off.size} offsets, the index {index.n} rows")
        if off[0] != 0 or (np.diff(off) < 0).any() or off[-1] != t.size or t.size != v.size:
            raise ValueError("row offsets must start at 0, never decrease and end at the number of terms and values")
        self.n, self.vocab, self.max_nq, self.max_k, self.device = index.n, int(vocab), int(max_nq), int(max_k), index.device
        rc = self._lib.icd_sparse_create(index._h, off.ctypes.data, t.ctypes.data if t.size else None, v.ctypes.data if t.size else None,
                                         self.vocab, self.max_nq, self.max_k, C.byref(self._h))
        _check_inv(self._lib, rc)

    def stats(self) -> dict:
        if self.closed:
            raise IcdError(-5, "sparse index is closed")
        vv, nn, bb = C.c_int64(), C.c_int64(), C.c_int64()
        _check(self._lib, self._lib.icd_sparse_stats(self._h, C.byref(vv), C.byref(nn), C.byref(bb)))
        return {"vocab": vv.value, "nnz": nn.value, "bytes": bb.value}


class IcdColumns(_Handle):
    """int32 columns of the rows of one IcdIndex on the device (icd_columns_*): what the filter programs of IcdIndex.filter_masks
    read. Independent of the index's lifetime: either may be closed first (a call with a closed partner raises)."""
    _destroy = "icd_columns_destroy"

    def __init__(self, index: "IcdIndex", cols):
        self._lib = index._lib
        self._h = C.c_void_p()
        keep = np.ascontiguousarray(np.asarray(cols), dtype=np.int32)
        if keep.ndim != 2 or keep.shape[0] < 1 or keep.shape[1] != index.n:
            raise ValueError(f"cols of shape {keep.shape}: [ncols >= 1, n = {index.n}]")
        self.n, self.ncols, self.device = index.n, int(keep.shape[0]), index.device
        rc = self._lib.icd_columns_create(index._h, keep.ctypes.data, self.ncols, C.byref(self._h))
        _check_inv(self._lib, rc)

    def stats(self) -> dict:
        if self.closed:
            raise IcdError(-5, "columns are closed")
        c, r, b = C.c_int32(), C.c_int64(), C.c_int64()
        _check(self._lib, self._lib.icd_columns_stats(self._h, C.byref(c), C.byref(r), C.byref(b)))
        return {"ncols": c.value, "rows": r.value, "bytes": b.value}


def filter_program_check(prog_off, prog, ncols: int, vocab: int = 0):
    """icd_filter_program_check (host only): None when the nq programs are well-formed for `ncols` columns and a vocabulary of
    `vocab` terms (0: no sparse index), else the library's reason"""
    lib = load_library()
    off = np.ascontiguousarray(np.asarray(prog_off).reshape(-1), dtype=np.int64)
    pr = np.ascontiguousarray(np.asarray(prog).reshape(-1), dtype=np.uint32)
    msg = C.create_string_buffer(256)
    rc = lib.icd_filter_program_check(off.ctypes.data, pr.ctypes.data if pr.size else None, int(off.size) - 1, int(ncols), int(vocab),
                                      C.cast(msg, C.c_void_p), len(msg))
    return None if rc == 0 else msg.value.decode("utf-8", "replace")


def rowmask_words(n: int) -> int:
    """32-bit words of a row mask's bitset over n rows: whole 128-row tiles (include/icd_search.h, icd_rowmask_create)"""
    return (int(n) + 127) // 128 * 4


def pack_rowmask(rows, n: int) -> np.ndarray:
    """The bitset a host row list becomes (icd_rowmask_pack, the packer icd_rowmask_create runs on a host list; no device
    needed): uint32[rowmask_words(n)], row r = bit r & 31 of word r >> 5, zero-padded. rows: strictly increasing, in [0, n)."""
    lib = load_library()
    r = np.ascontiguousarray(np.asarray(rows).reshape(-1), dtype=np.int64)
    out = np.empty(rowmask_words(n), dtype=np.uint32)
    rc = lib.icd_rowmask_pack(r.ctypes.data if r.size else None, int(r.size), int(n), out.ctypes.data, int(out.size))
    _check_inv(lib, rc)
    return out


class IcdRowMask(_Handle):
    """A set of rows of one IcdIndex as a device bitset (icd_rowmask_*): what search_masked tests inside the scan. Independent
    of the index's lifetime: either may be closed first (a search with a closed partner raises)."""
    _destroy = "icd_rowmask_destroy"

    def __init__(self, index: "IcdIndex", rows):
        self._lib = index._lib
        self._h = C.c_void_p()
        if _is_torch_tensor(rows) and rows.is_cuda:
            import torch
            keep = rows.to(torch.int64).contiguous().reshape(-1)
            if keep.device.index != index.device:
                raise ValueError(f"rows on cuda:{keep.device.index}, index on device {index.device}")
            torch.cuda.synchronize(index.device)
            ptr, on_dev, m = keep.data_ptr(), 1, int(keep.numel())
        else:
            if _is_torch_tensor(rows):
                rows = rows.detach().cpu().numpy()
            keep = np.ascontiguousarray(np.asarray(rows).reshape(-1), dtype=np.int64)
            ptr, on_dev, m = keep.ctypes.data, 0, int(keep.size)
        self.n, self.rows, self.device = index.n, m, index.device
        rc = self._lib.icd_rowmask_create(index._h, ptr if m else None, m, on_dev, C.byref(self._h))
        _check_inv(self._lib, rc)

    @classmethod
    def _adopt(cls, index: "IcdIndex", handle: int) -> "IcdRowMask":
        """a mask the library created itself (IcdIndex.match_masks); `rows` is None until stats() reads the device's count"""
        m = cls.__new__(cls)
        m._lib, m._h = index._lib, C.c_void_p(handle)
        m.n, m.rows, m.device = index.n, None, index.device
        return m

    def stats(self) -> dict:
        if self.closed:
            raise IcdError(-5, "row mask is closed")
        r, b = C.c_int64(), C.c_int64()
        _check(self._lib, self._lib.icd_rowmask_stats(self._h, C.byref(r), C.byref(b)))
        if self.rows is None:
            self.rows = r.value
        return {"rows": r.value, "bytes": b.value}

    def words(self) -> np.ndarray:
        """The mask's bitset on the host (icd_rowmask_read; synchronises): uint32[rowmask_words(n)] in pack_rowmask's layout"""
        if self.closed:
            raise IcdError(-5, "row mask is closed")
        out = np.empty(rowmask_words(self.n), dtype=np.uint32)
        _check(self._lib, self._lib.icd_rowmask_read(self._h, out.ctypes.data, int(out.size)))
        return out


def group_unique_id() -> bytes:
    """rank 0: the RCCL unique id every rank passes to IcdGroup (icd_group_unique_id); hand the bytes over any side channel"""
    lib = load_library()
    buf = (C.c_uint8 * GROUP_ID_BYTES)()
    _check(lib, lib.icd_group_unique_id(C.cast(buf, C.c_void_p)))
    return bytes(buf)


class IcdGroup:
    """Multi-GPU search behind the C ABI (icd_group_*): one process per GPU, this rank's IcdIndex (a row shard created with
    id_base = its first global row, or a replica), an RCCL communicator owned by the group. `unique_id`: group_unique_id()
    of rank 0 (None for a single rank). search() takes the FULL query batch as a CUDA tensor on every rank."""

    def __init__(self, index: "IcdIndex", mode: int, rank: int = 0, world: int = 1, unique_id: Optional[bytes] = None,
                 max_nq: Optional[int] = None, max_k: Optional[int] = None, connect: bool = True, with_comm: Optional[bool] = None):
        """connect=True (default): prepare + connect in one go (`unique_id` required for world > 1). connect=False: only the
        LOCAL half (icd_group_prepare: argument checks, buffers, librccl) - the caller lets the ranks agree that every one of
        them got this far and then calls connect(unique_id) on all of them (collective) or close() on all of them."""
        self._lib = load_library()
        self._h = C.c_void_p()
        self.index, self.mode, self.rank, self.world = index, int(mode), int(rank), int(world)
        # (row-sharded: every rank searches the whole slice, so a slice is at most the index's max_nq; query-sharded: a
        #  slice of world x max_nq queries gives every rank max_nq of them)
        self.max_nq = int(max_nq or (index.max_nq if mode == GROUP_ROW_SHARD else index.max_nq * max(1, world)))
        self.max_k = int(max_k or min(index.max_k, 1024 // max(1, world) if mode == GROUP_ROW_SHARD else index.max_k))
        if connect and world > 1 and unique_id is None:
            raise ValueError(f"a group of {world} ranks needs rank 0's {GROUP_ID_BYTES}-byte unique id")
        if with_comm is None:   # (world = 1 with an id: a one-rank communicator, the collective path end to end)
            with_comm = world > 1 or unique_id is not None
        if index.closed:
            raise IcdError(-5, "index is closed")
        _check(self._lib, self._lib.icd_group_prepare(index._h, 1 if with_comm else 0, self.rank, self.world, self.mode, self.max_nq,
                                                       self.max_k, C.byref(self._h)))
        self.connected = not with_comm
        import weakref
        if not hasattr(index, "_group_refs"):
            index._group_refs = []
        index._group_refs.append(weakref.ref(self))   # the group borrows the index's handle: IcdIndex.close() closes it first
        if connect and with_comm:
            try:
                self.connect(unique_id)
            except Exception:
                self.close()
                raise

    def connect(self, unique_id: bytes):
        """COLLECTIVE (ncclCommInitRank): every rank of the group calls it, or none does"""
        if self.connected:
            return
        if unique_id is None or len(unique_id) != GROUP_ID_BYTES:
            raise ValueError(f"unique id must be {GROUP_ID_BYTES} bytes")
        idbuf = (C.c_uint8 * GROUP_ID_BYTES).from_buffer_copy(unique_id)
        _check(self._lib, self._lib.icd_group_connect(self._h, C.cast(idbuf, C.c_void_p)))
        self.connected = True

    def search(self, queries, k: int = 10, gather: bool = True):
        """-> (adj f64, raw f32, ids i64, levels i32), each [nq, k] CUDA tensors (query-sharded with gather=False: only
        this rank's rows). Batches larger than the group's max_nq go through in slices of that many queries."""
        import torch
        if not getattr(self, "_h", None) or not self._h.value:
            raise IcdError(-5, "group is closed")
        q, on_dev = self.index._prep_queries(queries)
        self.index._validate(q, k)   # (icd_group_search has no dim argument: a wrong width would be an out-of-bounds device read)
        if k > self.max_k:
            raise ValueError(f"k={k} outside 1..{self.max_k} (group)")
        if not on_dev:
            q = torch.from_numpy(q).to(torch.device("cuda", self.index.device))
        nq, dev = int(q.shape[0]), q.device
        local_only = self.mode == GROUP_QUERY_SHARD and not gather
        if local_only and nq > self.max_nq:
            # (slices of max_nq would each be split over the ranks: another set of rows than shard_bounds(nq) of the whole batch)
            raise ValueError(f"query-sharded search without gather takes at most the group's max_nq = {self.max_nq} queries per call (got {nq})")
        parts = []
        for s0 in range(0, max(nq, 1), self.max_nq):
            qs = q[s0:s0 + self.max_nq]
            m = int(qs.shape[0])
            outs = (torch.empty((m, k), dtype=torch.float64, device=dev), torch.empty((m, k), dtype=torch.float32, device=dev),
                    torch.empty((m, k), dtype=torch.int64, device=dev), torch.empty((m, k), dtype=torch.int32, device=dev))
            if m:
                _check(self._lib, self._lib.icd_group_search(self._h, qs.data_ptr(), m, k, 1 if gather else 0, *[o.data_ptr() for o in outs],
                                                              _current_stream_ptr(self.index.device)))
            keep = m
            if local_only:
                base, rem = divmod(m, self.world)
                keep = base + (1 if self.rank < rem else 0)
            parts.append(tuple(o[:keep] for o in outs))
        if len(parts) == 1:
            return parts[0]
        return tuple(torch.cat([p[i] for p in parts]) for i in range(4))

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self._lib.icd_group_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _profile_summary(self) -> dict:
    """Mean per-kernel ms over the profiled searches since the last summary (events on the search stream)."""
    p, n = _Profile(), C.c_int32(0)
    _check(self._lib, self._lib.icd_index_profile_summary(self._h, C.byref(p), C.byref(n)))
    out = {f: float(getattr(p, f)) for f, _ in _Profile._fields_}
    out["count"] = int(n.value)
    return out


IcdIndex.profile_summary = _profile_summary


def hier_rescore(adj, ids, row_tags, q_params, weights, id_base: int = 0):
    """Device-side hierarchical rescoring of a batch of hit lists (icd_hier_rescore). adj f64 [nq,k], ids i64 [nq,k],
    row_tags u8 [n_rows], q_params f64 [nq,12] are tensors on one GPU; weights: 7 Python floats. Returns
    (order i32, enhanced f64, score f64, vs f64, hb f64, boost f64), each [nq,k], in the final order.
    q_params of shape [nq,22] (queries with NER entities: HierarchicalSimilarityService.query_params_entities) take
    icd_hier_rescore_entities instead."""
    import torch
    lib = load_library()
    nq, k = adj.shape
    dev = adj.device
    adj = adj.to(torch.float64).contiguous()
    ids = ids.to(torch.int64).contiguous()
    row_tags = row_tags.to(torch.uint8).contiguous()
    q_params = q_params.to(device=dev, dtype=torch.float64).contiguous()
    assert q_params.shape in ((nq, 12), (nq, 22)) and row_tags.device == dev
    entry = lib.icd_hier_rescore if q_params.shape[1] == 12 else lib.icd_hier_rescore_entities
    w = (C.c_double * 7)(*[float(x) for x in weights])
    order = torch.empty((nq, k), dtype=torch.int32, device=dev)
    outs = [torch.empty((nq, k), dtype=torch.float64, device=dev) for _ in range(5)]
    _check(lib, entry(dev.index, adj.data_ptr(), ids.data_ptr(), nq, k, int(id_base), row_tags.numel(),
                      row_tags.data_ptr(), q_params.data_ptr(), C.cast(w, C.c_void_p), order.data_ptr(),
                      *[t.data_ptr() for t in outs], _current_stream_ptr(dev.index)))
    return (order, *outs)


def pack_winners(order, ids, raw, adj, enhanced, vs, hb, boost, kk: int):
    """The top kk rescored hits of every query as ONE float64 tensor [8, nq, kk] on the device (icd_pack_winners): id (plane 0
    holds the int64 ids' BIT PATTERNS: read it with .view(torch.int64)), raw score,
    level-reweighted score (of the hit order points at), order, enhanced, vector similarity, hierarchy boost, uncertainty boost."""
    import torch
    lib = load_library()
    nq, k = order.shape
    dev = order.device
    order = order.to(torch.int32).contiguous(); ids = ids.to(torch.int64).contiguous(); raw = raw.to(torch.float32).contiguous()
    f64 = [t.to(torch.float64).contiguous() for t in (adj, enhanced, vs, hb, boost)]
    out = torch.empty((8, nq, kk), dtype=torch.float64, device=dev)
    _check(lib, lib.icd_pack_winners(dev.index, order.data_ptr(), ids.data_ptr(), raw.data_ptr(), *[t.data_ptr() for t in f64],
                                     nq, k, kk, out.data_ptr(), _current_stream_ptr(dev.index)))
    return out


def score_stats(scores, order=None, use=None):
    """Row N3 (icd_score_stats): numpy-identical mean / std / var / max of every query's first `use` scores, plus the
    confidence service's model_uncertainty and prediction_variance. scores f64 [nq,k] on a GPU, order i32 [nq,k] or None
    (entries with order < 0 do not exist). Returns f64 [nq,6]."""
    import torch
    lib = load_library()
    nq, k = scores.shape
    dev = scores.device
    scores = scores.to(torch.float64).contiguous()
    if order is not None:
        order = order.to(device=dev, dtype=torch.int32).contiguous()
        assert order.shape == (nq, k)
    out = torch.empty((nq, 6), dtype=torch.float64, device=dev)
    _check(lib, lib.icd_score_stats(dev.index, scores.data_ptr(), order.data_ptr() if order is not None else None, nq, k,
                                    int(k if use is None else use), out.data_ptr(), _current_stream_ptr(dev.index)))
    return out


def cosine_rows(x, y):
    """Row N3 (icd_cosine_rows): sklearn-style cosine of every row of x (f32 [nq,dim] on a GPU) with the matching row of
    y ([nq,dim]) or with the single row y ([dim]); returns f64 [nq]."""
    import torch
    lib = load_library()
    nq, dim = x.shape
    dev = x.device
    x = x.to(torch.float32).contiguous()
    y = y.to(device=dev, dtype=torch.float32).contiguous()
    if y.dim() == 1:
        assert y.shape[0] == dim
        stride = 0
    else:
        assert y.shape == (nq, dim)
        stride = dim
    out = torch.empty((nq,), dtype=torch.float64, device=dev)
    _check(lib, lib.icd_cosine_rows(dev.index, x.data_ptr(), y.data_ptr(), stride, nq, dim, out.data_ptr(),
                                    _current_stream_ptr(dev.index)))
    return out


TERM_MAX_LEN = 32   # include/icd_search.h ICD_TERM_MAX_LEN


def pack_strings(strings):
    """strings -> (int32 code points back to back, int32 offsets [n + 1]) as numpy arrays: the layout icd_term_first_match reads"""
    cp = np.frombuffer("".join(strings).encode("utf-32-le"), dtype=np.int32)
    off = np.zeros(len(strings) + 1, dtype=np.int64)
    np.cumsum([len(s) for s in strings], out=off[1:])
    if off[-1] >= 2 ** 31:
        raise ValueError("more than 2^31 - 1 code points")
    return cp.copy(), off.astype(np.int32)


def term_first_match(key_cp, key_off, terms):
    """icd_term_first_match: for every term (a Python str of at most TERM_MAX_LEN code points), the index of the first key with
    `term in key or key in term` (both at least two code points long), else -1 - in ONE launch. key_cp / key_off: int32 tensors on
    a GPU (pack_strings of the keys). Returns a list of ints; raises IcdError (ICD_ERR_UNSUPPORTED) for a longer term."""
    import torch
    lib = load_library()
    dev = key_cp.device
    assert key_cp.dtype == torch.int32 and key_off.dtype == torch.int32 and key_off.device == dev
    terms = list(terms)
    if not terms:
        return []
    cp, off = pack_strings(terms)
    # (one upload: the offsets and the code points side by side; a lone empty code-point array still needs a valid pointer)
    buf = torch.from_numpy(np.concatenate([off, cp, np.zeros(1, np.int32)])).to(dev)
    out = torch.empty((len(terms),), dtype=torch.int32, device=dev)
    n_off = off.size
    _check(lib, lib.icd_term_first_match(dev.index, key_cp.data_ptr(), key_off.data_ptr(), key_off.numel() - 1,
                                         buf[n_off:].data_ptr(), buf[:n_off].data_ptr(), len(terms), out.data_ptr(),
                                         _current_stream_ptr(dev.index)))
    return out.tolist()


def packed_attention(qkv, starts, nseq: int, heads: int, max_len: int, out):
    """icd_packed_attention: softmax(Q K^T / 8) V per sequence and head over packed tokens. qkv f32 [T(+1), 3 * heads * 64]
    (row-contiguous), starts int32 [nseq + 1] on the same GPU, out f32 [T(+1), heads * 64]; sequences of at most 64 tokens.
    Enqueued on the current stream."""
    lib = load_library()
    dev = qkv.device
    assert qkv.is_cuda and qkv.stride(1) == 1 and out.stride(1) == 1 and starts.is_cuda
    _check(lib, lib.icd_packed_attention(dev.index, qkv.data_ptr(), qkv.stride(0), starts.data_ptr(), int(nseq), int(heads), 64,
                                         int(max_len), out.data_ptr(), out.stride(0), _current_stream_ptr(dev.index)))
    return out


class SmallEncoder:
    """The BERT-style sentence encoder for SMALL inputs (include/icd_search.h icd_encoder_*; csrc/encoder_small.hpp): up to
    ENCODER_MAX_SEQS sequences / ENCODER_MAX_TOKENS packed tokens per call, ONE graph launch per forward. Replaces the
    SentenceTransformer.encode call of EmbeddingService.encode_query / encode_single (reference
    services/embedding_service.py:97-102,117-120) for one string or a request's handful.

    Built from a transformers BertModel-like module on a CUDA device with fp32 parameters. The handle COPIES the four Linear
    weights of every layer at creation (into the order its GEMMs read them) and BORROWS embeddings, biases and LayerNorm
    parameters (this object keeps those tensors alive): rebuild it after changing the module's parameters."""

    @staticmethod
    def supported(bert) -> bool:
        try:
            cfg = bert.config
            p = bert.embeddings.word_embeddings.weight
            import torch
            return (type(bert).__name__ in ("BertModel", "XLMRobertaModel", "RobertaModel") and p.is_cuda and p.dtype == torch.float32
                    and getattr(cfg, "position_embedding_type", None) in (None, "absolute") and getattr(cfg, "hidden_act", "gelu") == "gelu"
                    and not getattr(cfg, "is_decoder", False) and int(cfg.hidden_size) in (768, 1024) and int(cfg.hidden_size) // int(cfg.num_attention_heads) == 64
                    and int(cfg.intermediate_size) == 4 * int(cfg.hidden_size))   # (icd_encoder_create refuses any other FFN width)
        except Exception:
            return False

    def __init__(self, bert, arithmetic: Optional[str] = None):
        """arithmetic: "bf16x3" (the default; env ICD_ENCODER_ARITH) = the split-bf16 GEMMs, "fp32" = fp32-input MFMAs - of BOTH
        forms (encode / encode_many) alike: whichever it is, a list's rows equal the one-string call's bit for bit"""
        import torch
        self._lib = load_library()
        self.arithmetic = (arithmetic or os.environ.get("ICD_ENCODER_ARITH", "bf16x3")).strip().lower()
        if self.arithmetic not in ENCODER_ARITH:
            raise ValueError(f"encoder arithmetic {self.arithmetic!r}: one of {sorted(ENCODER_ARITH)}")
        cfg = bert.config
        emb = bert.embeddings
        self.hidden = int(cfg.hidden_size)
        self.device = emb.word_embeddings.weight.device.index or 0
        keep = []   # every tensor the handle points at

        def ptr(t):
            t = t.detach()
            if not t.is_contiguous():
                t = t.contiguous()
            assert t.dtype == torch.float32 and t.is_cuda
            keep.append(t)
            return t.data_ptr()
        d = _EncoderDesc()
        d.layers, d.hidden, d.heads, d.inter = len(bert.encoder.layer), self.hidden, int(cfg.num_attention_heads), int(cfg.intermediate_size)
        d.vocab, d.max_pos = int(emb.word_embeddings.weight.shape[0]), int(emb.position_embeddings.weight.shape[0])
        d.pos_offset = int(emb.padding_idx) + 1 if type(bert).__name__ != "BertModel" else 0
        d.ln_eps = float(cfg.layer_norm_eps)
        d.arithmetic = ENCODER_ARITH[self.arithmetic]
        d.word_emb, d.pos_emb = ptr(emb.word_embeddings.weight), ptr(emb.position_embeddings.weight)
        d.type_emb0 = ptr(emb.token_type_embeddings.weight[0])
        d.emb_ln_g, d.emb_ln_b = ptr(emb.LayerNorm.weight), ptr(emb.LayerNorm.bias)
        per = {name: [] for name in _ENC_LAYER_FIELDS}
        scratch = []
        for l in bert.encoder.layer:
            a = l.attention.self
            wqkv = torch.cat([a.query.weight, a.key.weight, a.value.weight], 0).detach().contiguous()   # (copied by the handle at create: not kept)
            scratch.append(wqkv)
            per["w_qkv"].append(wqkv.data_ptr())
            per["b_qkv"].append(ptr(torch.cat([a.query.bias, a.key.bias, a.value.bias], 0)))
            per["w_ao"].append(ptr(l.attention.output.dense.weight)); per["b_ao"].append(ptr(l.attention.output.dense.bias))
            per["ln1_g"].append(ptr(l.attention.output.LayerNorm.weight)); per["ln1_b"].append(ptr(l.attention.output.LayerNorm.bias))
            per["w_up"].append(ptr(l.intermediate.dense.weight)); per["b_up"].append(ptr(l.intermediate.dense.bias))
            per["w_down"].append(ptr(l.output.dense.weight)); per["b_down"].append(ptr(l.output.dense.bias))
            per["ln2_g"].append(ptr(l.output.LayerNorm.weight)); per["ln2_b"].append(ptr(l.output.LayerNorm.bias))
        arrays = {}
        for name in _ENC_LAYER_FIELDS:
            arrays[name] = (C.c_void_p * d.layers)(*per[name])
            setattr(d, name, C.cast(arrays[name], C.POINTER(C.c_void_p)))
        self._keep = keep
        h = C.c_void_p()
        _check(self._lib, self._lib.icd_encoder_create(self.device, C.byref(d), C.byref(h)))   # (synchronises: the weight copies are done)
        del scratch
        self._h = h

    def fits(self, lengths) -> bool:
        return 0 < len(lengths) <= ENCODER_MAX_SEQS and sum(lengths) <= ENCODER_MAX_TOKENS and min(lengths) >= 1

    def encode(self, ids, pooling: str = "mean", normalize: bool = True, to_device: bool = False, hidden: bool = False):
        """ids: token id lists (special tokens included). -> float32 [n, hidden] (numpy, or a CUDA tensor with to_device=True:
        enqueued on torch's current stream); with hidden=True also the last hidden state of every token, packed [T, hidden]
        (a CUDA tensor)."""
        import torch
        if not getattr(self, "_h", None) or not self._h.value:
            raise IcdError(-5, "encoder is closed")
        lengths = np.fromiter((len(x) for x in ids), dtype=np.int32, count=len(ids))
        flat = np.fromiter((t for x in ids for t in x), dtype=np.int32, count=int(lengths.sum()))
        n = len(ids)
        dev = torch.device("cuda", self.device)
        hid = torch.empty((int(lengths.sum()), self.hidden), dtype=torch.float32, device=dev) if hidden else None
        if to_device:
            out = torch.empty((n, self.hidden), dtype=torch.float32, device=dev)
            optr = out.data_ptr()
        else:
            out = np.empty((n, self.hidden), dtype=np.float32)
            optr = out.ctypes.data
        _check(self._lib, self._lib.icd_encoder_encode(self._h, flat.ctypes.data, lengths.ctypes.data, n, 1 if pooling == "cls" else 0,
                                                      1 if normalize else 0, optr, 1 if to_device else 0,
                                                      hid.data_ptr() if hidden else None, _current_stream_ptr(self.device)))
        return (out, hid) if hidden else out

    def fits_each(self, lengths) -> bool:
        """every sequence fits a call of its own: encode_many takes the list whatever its size"""
        return len(lengths) > 0 and 1 <= min(lengths) and max(lengths) <= ENCODER_MAX_TOKENS

    def encode_many(self, ids, pooling: str = "mean", normalize: bool = True, to_device: bool = False):
        """ANY number of sequences (each of at most ENCODER_MAX_TOKENS tokens) through the same kernels, cut into calls by the
        library (icd_encoder_encode_many): row i equals encode([ids[i]]) BIT FOR BIT - the arithmetic of a sequence does not
        depend on what shares its call. -> float32 [n, hidden], numpy or (to_device) a CUDA tensor on the current stream."""
        import torch
        if not getattr(self, "_h", None) or not self._h.value:
            raise IcdError(-5, "encoder is closed")
        n = len(ids)
        lengths = np.fromiter((len(x) for x in ids), dtype=np.int32, count=n)
        flat = np.fromiter((t for x in ids for t in x), dtype=np.int32, count=int(lengths.sum()))
        out = torch.empty((n, self.hidden), dtype=torch.float32, device=torch.device("cuda", self.device))
        _check(self._lib, self._lib.icd_encoder_encode_many(self._h, flat.ctypes.data, lengths.ctypes.data, n, 1 if pooling == "cls" else 0,
                                                           1 if normalize else 0, out.data_ptr(), 1, _current_stream_ptr(self.device)))
        return out if to_device else out.cpu().numpy()

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self._lib.icd_encoder_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def split_bf16x3(x, gelu: bool = False):
    """icd_split_bf16x3: x f32 [rows, cols] on the GPU (row-contiguous) -> bf16 [rows, 3 * cols + 64] = [hi | hi | lo | 1 1 0 ...],
    the A operand of a split-bf16 GEMM (services/embedding_service.py _PackedBert); gelu: through erf-GELU first.
    Enqueued on the current stream."""
    import torch
    lib = load_library()
    assert x.is_cuda and x.dtype == torch.float32 and x.dim() == 2 and x.stride(1) == 1 and x.shape[1] % 8 == 0 and x.shape[1] >= 64
    out = torch.empty((x.shape[0], 3 * x.shape[1] + SPLIT_TAIL), dtype=torch.bfloat16, device=x.device)
    _check(lib, lib.icd_split_bf16x3(x.device.index, x.data_ptr(), int(x.shape[0]), int(x.shape[1]), int(x.stride(0)), 1 if gelu else 0,
                                     out.data_ptr(), _current_stream_ptr(x.device.index)))
    return out


def merge_topk(scores, ids, levels, k: int):
    """Row-sharded search, step 2 (device tensors): scores/ids/levels are [G, nq, k] gathered from G
    shards; returns (adj f64, raw f32, ids i64, levels i32), each [nq, k], reweighted and re-sorted."""
    import torch
    lib = load_library()
    G, nq, kk = scores.shape
    assert kk == k
    dev = scores.device
    scores = scores.to(torch.float32).contiguous()
    ids = ids.to(torch.int64).contiguous()
    levels = levels.to(torch.int32).contiguous()
    adj = torch.empty((nq, k), dtype=torch.float64, device=dev)
    raw = torch.empty((nq, k), dtype=torch.float32, device=dev)
    oid = torch.empty((nq, k), dtype=torch.int64, device=dev)
    olv = torch.empty((nq, k), dtype=torch.int32, device=dev)
    _check(lib, lib.icd_merge_topk(dev.index, scores.data_ptr(), ids.data_ptr(), levels.data_ptr(), G, nq, k,
                                   adj.data_ptr(), raw.data_ptr(), oid.data_ptr(), olv.data_ptr(),
                                   _current_stream_ptr(dev.index)))
    return adj, raw, oid, olv
