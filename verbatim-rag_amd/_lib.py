"""ctypes binding of libvrag_amd.so (include/vrag_amd.h). Fails loudly: there is no
Python/CPU fallback for any entry point."""
from __future__ import annotations

import ctypes as C
import os
import threading

_HERE = os.path.dirname(os.path.abspath(__file__))
_LOCK = threading.Lock()
_LIB = None

VRAG_OK = 0
ABI_VERSION = 6
PROF_CLASSES = (
    "embed", "layernorm", "gemm_qkv", "attn_global", "attn_local",
    "gemm_wo", "gemm_wi", "gemm_wo_mlp", "head", "qkv_attn_global", "qkv_attn_local",
)


class VragError(RuntimeError):
    """A libvrag_amd call returned a non-zero status."""

    def __init__(self, fn: str, status: int, message: str):
        super().__init__(f"{fn} failed (status {status}): {message}")
        self.status = status


class EncoderConfig(C.Structure):
    _fields_ = [
        ("vocab_size", C.c_int32), ("hidden_size", C.c_int32), ("num_layers", C.c_int32),
        ("num_heads", C.c_int32), ("intermediate_size", C.c_int32), ("global_every", C.c_int32),
        ("sliding_window", C.c_int32), ("rope_theta_global", C.c_float), ("rope_theta_local", C.c_float),
        ("norm_eps", C.c_float), ("pad_token_id", C.c_int32), ("max_seq_len", C.c_int32),
        ("max_tokens", C.c_int32), ("max_seqs", C.c_int32), ("max_ranges", C.c_int32),
        ("micro_batch_tokens", C.c_int32), ("device", C.c_int32), ("operand_dtype", C.c_int32),
    ]


OPERAND_DTYPES = {"bf16": 0, "f16": 1}
_FP = C.POINTER(C.c_float)
_FPP = C.POINTER(_FP)
_IP = C.POINTER(C.c_int32)
_LP = C.POINTER(C.c_int64)


class EncoderWeights(C.Structure):
    _fields_ = [
        ("tok_embeddings", _FP), ("emb_norm", _FP), ("attn_norm", _FPP), ("wqkv", _FPP), ("wo", _FPP),
        ("mlp_norm", _FPP), ("wi", _FPP), ("wo_mlp", _FPP), ("final_norm", _FP),
    ]


class BertConfig(C.Structure):
    _fields_ = [
        ("vocab_size", C.c_int32), ("hidden_size", C.c_int32), ("num_layers", C.c_int32), ("num_heads", C.c_int32),
        ("intermediate_size", C.c_int32), ("max_position_embeddings", C.c_int32), ("norm_eps", C.c_float),
        ("pad_token_id", C.c_int32), ("max_seq_len", C.c_int32), ("max_tokens", C.c_int32), ("max_seqs", C.c_int32),
        ("max_ranges", C.c_int32), ("micro_batch_tokens", C.c_int32), ("device", C.c_int32), ("operand_dtype", C.c_int32),
    ]


class BertWeights(C.Structure):
    _fields_ = [
        ("word_embeddings", _FP), ("position_embeddings", _FP), ("token_type_row", _FP), ("emb_norm_w", _FP),
        ("emb_norm_b", _FP), ("wqkv", _FPP), ("bqkv", _FPP), ("wo", _FPP), ("bo", _FPP), ("attn_norm_w", _FPP),
        ("attn_norm_b", _FPP), ("w1", _FPP), ("b1", _FPP), ("w2", _FPP), ("b2", _FPP), ("out_norm_w", _FPP),
        ("out_norm_b", _FPP),
    ]


class FilterLeaf(C.Structure):
    """vrag_filter_leaf (include/vrag_amd.h), field for field; tests/test_filter_program_host.py checks the layout against the host
    compiler's."""
    _fields_ = [("bound", C.c_double), ("table_off", C.c_int64), ("table_codes", C.c_int64), ("column", C.c_int32),
                ("num_op", C.c_uint8), ("str_mode", C.c_uint8), ("bool_bits", C.c_uint8), ("other_bit", C.c_uint8)]


FILTER_MAX_COLUMNS, FILTER_MAX_LEAVES, FILTER_MAX_OPS, FILTER_MAX_DEPTH = 16, 64, 256, 32   # VRAG_FILTER_MAX_*
FILTER_KINDS = {"other": 0, "number": 1, "string": 2, "bool": 3}                                # VRAG_FILTER_KIND_*
FILTER_NUM_OPS = {"never": 0, "always": 1, "==": 2, "!=": 3, "<": 4, "<=": 5, ">": 6, ">=": 7}  # VRAG_FILTER_NUM_*
FILTER_STR_MODES = {"never": 0, "always": 1, "table": 2}                                        # VRAG_FILTER_STR_*
FILTER_OPS = {"leaf": 0, "and": 1, "or": 2, "not": 3, "list_any": 4}                            # VRAG_FILTER_OP_* (leaf index << 8)
FILTER_MATCH_OPS = {"==": 0, "!=": 1, "<": 2, "<=": 3, ">": 4, ">=": 5, "like": 6}                  # VRAG_FILTER_MATCH_*
FILTER_MATCH_MAX_PATTERN, FILTER_MATCH_MAX_SEGMENTS = 256, 16                                   # VRAG_FILTER_MATCH_MAX_*


class FilterMatch(C.Structure):
    """vrag_filter_match (include/vrag_amd.h), field for field; tests/test_like_filter_host.py checks the layout against the host
    compiler's."""
    _fields_ = [("text_off", C.c_int64), ("text_len", C.c_int32), ("leaf", C.c_int32), ("op", C.c_int32), ("pad", C.c_int32)]


# name -> (restype, argtypes); every symbol include/vrag_amd.h declares.
_H = C.c_void_p
SIGNATURES = {
    "vrag_last_error": (C.c_char_p, []),
    "vrag_abi_version": (C.c_int, []),
    "vrag_device_count": (C.c_int, []),
    "vrag_encoder_create": (C.c_int, [C.POINTER(EncoderConfig), C.POINTER(EncoderWeights), C.POINTER(_H)]),
    "vrag_bert_encoder_create": (C.c_int, [C.POINTER(BertConfig), C.POINTER(BertWeights), C.POINTER(_H)]),
    "vrag_encoder_destroy": (None, [_H]),
    "vrag_encoder_set_qa_head": (C.c_int, [_H, _FP, _FP, C.c_int32]),
    "vrag_encoder_set_token_head": (C.c_int, [_H, _FP, _FP, _FP, _FP, C.c_int32]),
    "vrag_encoder_set_mlm_head": (C.c_int, [_H, _FP, _FP, _FP, _FP]),
    "vrag_encoder_set_mlm_head_ex": (C.c_int, [_H, _FP, _FP, _FP, _FP, _FP, _FP]),
    "vrag_encoder_set_head_precision": (C.c_int, [_H, C.c_int32]),
    "vrag_encoder_set_token_types": (C.c_int, [_H, _FP, C.c_int32]),
    "vrag_encoder_load_token_types": (C.c_int, [_H, _IP, C.c_void_p]),
    "vrag_encoder_set_pair_head": (C.c_int, [_H, _FP, _FP, _FP, _FP, C.c_int32]),
    "vrag_encoder_run_pair_head": (C.c_int, [_H, C.c_void_p]),
    "vrag_encoder_read_pair_logits": (C.c_int, [_H, _FP, C.c_void_p]),
    "vrag_encoder_set_seq_head": (C.c_int, [_H, _FP, _FP, _FP, _FP, _FP, _FP, C.c_int32, C.c_int32]),
    "vrag_encoder_run_seq_head": (C.c_int, [_H, C.c_void_p]),
    "vrag_encoder_read_seq_logits": (C.c_int, [_H, _FP, C.c_void_p]),
    "vrag_encoder_load_batch": (C.c_int, [_H, _IP, _IP, C.c_int32, C.c_void_p]),
    "vrag_encoder_run": (C.c_int, [_H, C.c_void_p]),
    "vrag_encoder_run_layers": (C.c_int, [_H, C.c_int32, C.c_void_p]),
    "vrag_encoder_load_ranges": (C.c_int, [_H, _IP, _IP, _IP, C.c_int32, C.c_void_p]),
    "vrag_encoder_run_qa_head": (C.c_int, [_H, C.c_void_p]),
    "vrag_encoder_read_qa_logits": (C.c_int, [_H, _FP, C.c_void_p]),
    "vrag_encoder_run_pool": (C.c_int, [_H, C.c_int32, C.c_void_p]),
    "vrag_encoder_read_pool": (C.c_int, [_H, _FP, C.c_void_p]),
    "vrag_encoder_run_token_head": (C.c_int, [_H, C.c_void_p]),
    "vrag_encoder_read_token_logits": (C.c_int, [_H, _FP, C.c_void_p]),
    "vrag_encoder_read_token_spans": (C.c_int, [_H, _IP, _IP, _IP, _IP, C.c_int32, _LP, _IP, C.c_int32, C.c_float, C.c_int32, C.c_int32,
                                                C.c_int32, _IP, _IP, C.c_void_p]),
    "vrag_encoder_run_splade": (C.c_int, [_H, C.c_void_p]),
    "vrag_encoder_read_splade": (C.c_int, [_H, _FP, C.c_void_p]),
    "vrag_encoder_read_splade_sparse": (C.c_int, [_H, C.c_float, C.c_int32, _IP, _IP, _FP, C.c_void_p]),
    "vrag_encoder_read_hidden": (C.c_int, [_H, C.c_int32, _FP, C.c_void_p]),
    "vrag_encoder_extract_qa": (C.c_int, [_H, _IP, _IP, C.c_int32, _IP, _IP, _IP, C.c_int32, _FP]),
    "vrag_encoder_graph_stats": (C.c_int, [_H, C.c_int32, _LP, _IP]),
    "vrag_encoder_f16_saturated": (C.c_int, [_H, C.c_int32, _IP]),
    "vrag_encoder_set_concurrency": (C.c_int, [_H, C.c_int32]),
    "vrag_encoder_set_profiling": (C.c_int, [_H, C.c_int32]),
    "vrag_encoder_read_profile": (C.c_int, [_H, _FP, _LP, C.c_int32]),
    "vrag_set_small_batch_rows": (C.c_int, [C.c_int32]),
    "vrag_dense_index_create": (C.c_int, [C.c_int32, C.c_int64, C.c_int32, C.c_int32, C.POINTER(_H)]),
    "vrag_dense_index_destroy": (None, [_H]),
    "vrag_dense_index_size": (C.c_int64, [_H]),
    "vrag_dense_index_add": (C.c_int, [_H, _FP, C.c_int64]),
    "vrag_dense_index_add_device": (C.c_int, [_H, C.c_void_p, C.c_int64, C.c_void_p]),
    "vrag_dense_index_search": (C.c_int, [_H, _FP, C.c_int32, C.c_int32, _FP, _LP, C.c_void_p]),
    "vrag_dense_index_search_filtered": (C.c_int, [_H, _FP, C.c_int32, C.c_int32, C.c_void_p, C.c_int64, _FP, _LP, C.c_void_p]),
    "vrag_dense_index_run_resident": (C.c_int, [_H, C.c_int32, C.c_int32, C.c_void_p]),
    "vrag_dense_index_compact": (C.c_int, [_H, C.c_void_p, C.c_int64, _LP]),
    "vrag_dense_index_read": (C.c_int, [_H, C.c_int64, C.c_int64, _FP]),
    "vrag_dense_index_search_device": (C.c_int, [_H, _FP, C.c_int32, C.c_int32, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p,
                                                 C.c_void_p, C.c_void_p]),
    "vrag_dense_index_search_grouped": (C.c_int, [_H, _FP, C.c_int32, C.c_int32, C.c_int32, _H, C.c_void_p, C.c_int64, _FP, _LP, _IP,
                                                  C.c_void_p]),
    "vrag_group_column_create": (C.c_int, [C.c_int32, C.POINTER(_H)]),
    "vrag_group_column_destroy": (None, [_H]),
    "vrag_group_column_append": (C.c_int, [_H, _IP, C.c_int64]),
    "vrag_group_column_size": (C.c_int64, [_H]),
    "vrag_ivf_index_create": (C.c_int, [_H, C.c_int32, C.POINTER(_H)]),
    "vrag_ivf_index_create_sq8": (C.c_int, [_H, C.c_int32, C.POINTER(_H)]),
    "vrag_ivf_index_destroy": (None, [_H]),
    "vrag_ivf_index_set_centroids": (C.c_int, [_H, _FP]),
    "vrag_ivf_index_train": (C.c_int, [_H, C.c_int32, C.c_int64]),
    "vrag_ivf_index_sync": (C.c_int, [_H]),
    "vrag_ivf_index_stats": (C.c_int, [_H, _IP, _LP, _LP]),
    "vrag_ivf_index_read": (C.c_int, [_H, _FP, C.c_void_p, C.c_void_p]),
    "vrag_ivf_index_remap": (C.c_int, [_H, C.c_void_p, C.c_int64]),
    "vrag_ivf_index_search": (C.c_int, [_H, _FP, C.c_int32, C.c_int32, C.c_int32, _FP, _LP, _LP, C.c_void_p]),
    "vrag_sq8_index_create": (C.c_int, [C.c_int32, C.c_int64, C.c_int32, C.POINTER(_H)]),
    "vrag_sq8_index_destroy": (None, [_H]),
    "vrag_sq8_index_size": (C.c_int64, [_H]),
    "vrag_sq8_index_add": (C.c_int, [_H, _FP, C.c_int64]),
    "vrag_sq8_index_add_device": (C.c_int, [_H, C.c_void_p, C.c_int64, C.c_void_p]),
    "vrag_sq8_index_read": (C.c_int, [_H, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p]),
    "vrag_sq8_index_compact": (C.c_int, [_H, C.c_void_p, C.c_int64, _LP]),
    "vrag_sq8_index_set_route": (C.c_int, [_H, C.c_int32]),
    "vrag_sq8_index_search": (C.c_int, [_H, _FP, C.c_int32, C.c_int32, _FP, _LP, C.c_void_p]),
    "vrag_sq8_index_search_filtered": (C.c_int, [_H, _FP, C.c_int32, C.c_int32, C.c_void_p, C.c_int64, _FP, _LP, C.c_void_p]),
    "vrag_pq_index_create": (C.c_int, [C.c_int32, C.c_int32, C.c_int64, C.c_int32, C.POINTER(_H)]),
    "vrag_pq_index_destroy": (None, [_H]),
    "vrag_pq_index_size": (C.c_int64, [_H]),
    "vrag_pq_index_set_codebooks": (C.c_int, [_H, _FP]),
    "vrag_pq_index_read_codebooks": (C.c_int, [_H, _FP]),
    "vrag_pq_index_train": (C.c_int, [_H, _FP, C.c_int64, C.c_int32]),
    "vrag_pq_index_add": (C.c_int, [_H, _FP, C.c_int64]),
    "vrag_pq_index_add_device": (C.c_int, [_H, C.c_void_p, C.c_int64, C.c_void_p]),
    "vrag_pq_index_read": (C.c_int, [_H, C.c_int64, C.c_int64, C.c_void_p]),
    "vrag_pq_index_compact": (C.c_int, [_H, C.c_void_p, C.c_int64, _LP]),
    "vrag_pq_index_search": (C.c_int, [_H, _FP, C.c_int32, C.c_int32, _FP, _LP, C.c_void_p]),
    "vrag_pq_index_search_filtered": (C.c_int, [_H, _FP, C.c_int32, C.c_int32, C.c_void_p, C.c_int64, _FP, _LP, C.c_void_p]),
    "vrag_row_filter_create": (C.c_int, [C.c_int32, C.POINTER(_H)]),
    "vrag_row_filter_destroy": (None, [_H]),
    "vrag_row_filter_add_column": (C.c_int, [_H, _IP]),
    "vrag_row_filter_append": (C.c_int, [_H, C.c_int32, C.c_void_p, C.c_void_p, C.c_int64]),
    "vrag_row_filter_rows": (C.c_int, [_H, C.c_int32, _LP]),
    "vrag_row_filter_compact": (C.c_int, [_H, C.c_void_p, C.c_int64]),
    "vrag_row_filter_eval": (C.c_int, [_H, C.POINTER(FilterLeaf), C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_int64, C.c_int64,
                                       C.c_void_p, C.c_void_p]),
    "vrag_row_filter_append_strings": (C.c_int, [_H, C.c_int32, C.c_void_p, C.c_void_p, C.c_int64]),
    "vrag_row_filter_strings": (C.c_int, [_H, C.c_int32, _LP, _LP]),
    "vrag_row_filter_match": (C.c_int, [_H, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_int64, C.c_void_p, C.c_void_p]),
    "vrag_row_filter_eval_matched": (C.c_int, [_H, C.POINTER(FilterLeaf), C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_int64,
                                               C.POINTER(FilterMatch), C.c_int32, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p,
                                               C.c_void_p]),
    "vrag_row_filter_append_lists": (C.c_int, [_H, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64]),
    "vrag_row_filter_list_rows": (C.c_int, [_H, C.c_int32, _LP, _LP]),
    "vrag_row_filter_eval_lists": (C.c_int, [_H, C.POINTER(FilterLeaf), C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_int64,
                                             C.POINTER(FilterMatch), C.c_int32, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p,
                                             C.c_void_p]),
    "vrag_sparse_index_search_device": (C.c_int, [_H, _LP, _IP, _FP, C.c_int32, C.c_int32, C.c_void_p, C.c_int64, C.c_int64,
                                                  C.c_void_p, C.c_void_p, C.c_void_p]),
    "vrag_pack_qa_pairs": (C.c_int, [_IP, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, _IP, C.c_int32, C.c_int32, _IP, C.c_int64,
                                      _LP, _LP, C.c_int64, _IP, _IP, _LP]),
    "vrag_split_sentences": (C.c_int, [C.c_void_p, _LP, C.c_int32, C.c_int32, _IP, _IP, _IP, C.c_int32]),
    "vrag_chunk_markdown": (C.c_int, [C.c_void_p, _LP, C.c_int32, C.c_uint32, C.c_int32, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p,
                                      _LP, _LP, _LP, C.c_int32]),
    "vrag_topk_fill_empty": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p]),
    "vrag_sparse_index_create": (C.c_int, [C.c_int32, C.c_int64, _LP, _IP, _FP, C.c_int32, C.POINTER(_H)]),
    "vrag_sparse_index_destroy": (None, [_H]),
    "vrag_sparse_index_stats": (C.c_int, [_H, _LP, _LP, _LP]),
    "vrag_sparse_index_search": (C.c_int, [_H, _LP, _IP, _FP, C.c_int32, C.c_int32, _FP, _LP, C.c_void_p]),
    "vrag_sparse_index_search_filtered": (C.c_int, [_H, _LP, _IP, _FP, C.c_int32, C.c_int32, C.c_void_p, C.c_int64, _FP, _LP,
                                                    C.c_void_p]),
    "vrag_sparse_index_run_resident": (C.c_int, [_H, C.c_int32, C.c_int32, C.c_void_p]),
    "vrag_text_tokenize": (C.c_int, [C.c_void_p, _LP, C.c_int32, C.c_int32, C.c_int64, _IP, C.c_void_p, _LP]),
    "vrag_text_index_create": (C.c_int, [C.c_float, C.c_float, C.c_int32, C.POINTER(_H)]),
    "vrag_text_index_destroy": (None, [_H]),
    "vrag_text_index_add": (C.c_int, [_H, C.c_void_p, _LP, C.c_int32, C.c_int32]),
    "vrag_text_index_set_live": (C.c_int, [_H, C.c_void_p, C.c_int64]),
    "vrag_text_index_stats": (C.c_int, [_H, _LP, _LP, _LP, _LP, _LP]),
    "vrag_text_index_set_corpus_stats": (C.c_int, [_H, C.c_int64, C.c_int64]),
    "vrag_text_index_query_terms": (C.c_int, [_H, C.c_void_p, _LP, C.c_int32, C.c_int64, _LP, C.c_void_p, _IP, _LP, _LP]),
    "vrag_text_index_search": (C.c_int, [_H, _LP, C.c_void_p, _FP, C.c_int32, C.c_int32, C.c_void_p, C.c_int64, _FP, _LP]),
    "vrag_text_index_search_device": (C.c_int, [_H, _LP, C.c_void_p, _FP, C.c_int32, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p,
                                                C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]),
    "vrag_wordpiece_create": (C.c_int, [C.c_void_p, _LP, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_char_p, C.c_int32, C.c_int32,
                                        C.c_int32, C.POINTER(_H)]),
    "vrag_wordpiece_destroy": (None, [_H]),
    "vrag_wordpiece_encode": (C.c_int, [_H, C.c_void_p, _LP, C.c_int32, C.c_int32, C.c_int32, C.c_int64, _IP, _IP, C.c_void_p, _LP]),
    "vrag_bpe_create": (C.c_int, [C.c_int32, _IP, _IP, _IP, C.c_int32, _IP, _IP, C.c_void_p, _LP, _IP, C.c_int32, C.c_int32, C.c_int32,
                                  C.c_int32, C.c_int32, C.POINTER(_H)]),
    "vrag_bpe_destroy": (None, [_H]),
    "vrag_bpe_encode": (C.c_int, [_H, C.c_void_p, _LP, C.c_int32, C.c_int32, C.c_int32, C.c_int64, _IP, _IP, C.c_void_p, _LP]),
    "vrag_bpe_encode_offsets": (C.c_int, [_H, C.c_void_p, _LP, C.c_int32, C.c_int32, C.c_int32, C.c_int64, _IP, _IP, _IP, C.c_void_p, _LP]),
    "vrag_comm_get_unique_id": (C.c_int, [C.c_void_p]),
    "vrag_comm_create": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.POINTER(_H)]),
    "vrag_comm_destroy": (None, [_H]),
    "vrag_comm_info": (C.c_int, [_H, _IP, _IP, _IP]),
    "vrag_comm_allgather": (C.c_int, [_H, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]),
    "vrag_topk_allgather_merge": (C.c_int, [_H, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p,
                                            C.c_void_p]),
    "vrag_topk_merge": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int64,
                                  C.c_int64, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]),
    "vrag_rrf_fuse": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32,
                                C.c_int32, C.c_void_p]),
}


# include/vrag_amd_debug.h: the tuning / unit-test harness, exported by libvrag_amd_dbg.so only (load_debug()).
DEBUG_SIGNATURES = {
    "vrag_debug_gemm_ms": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _FP]),
    "vrag_debug_attn_run": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p,
                                      C.c_void_p, C.c_void_p, C.c_int32]),
    "vrag_debug_attn_run_ex": (C.c_int, [C.c_void_p, C.c_int32]),
    "vrag_debug_attn_ms": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _FP]),
    "vrag_debug_qkv_attn_ms": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _FP]),
    "vrag_debug_gemm_run": (C.c_int, [C.c_void_p, C.c_int32]),
    "vrag_debug_qkv_attn_run": (C.c_int, [C.c_void_p, C.c_int32]),
    "vrag_debug_pack_groups": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]),
    "vrag_debug_rows_run": (C.c_int, [C.c_void_p, C.c_int32]),
    "vrag_debug_glue_run": (C.c_int, [C.c_void_p, C.c_int32]),
    "vrag_debug_topk_run": (C.c_int, [C.c_void_p, C.c_int32]),
    "vrag_debug_text_run": (C.c_int, [C.c_void_p, C.c_int32]),
    "vrag_debug_text_index_read": (C.c_int, [C.c_void_p, C.c_void_p]),
    "vrag_debug_token_spans": (C.c_int, [_FP, C.c_int64, _IP, _IP, _IP, _IP, C.c_int32, _LP, _IP, C.c_int32, C.c_float, C.c_int32, C.c_int32,
                                         C.c_int32, _IP, _IP, C.c_int32]),
    "vrag_debug_canary_selftest": (C.c_int, [C.c_int32, C.c_int32]),
    "vrag_debug_topk_launch_log_reset": (None, []),
    "vrag_debug_topk_launch_log_read": (C.c_int, [_IP, C.c_int32, _IP, _IP]),
}

# the enum of include/vrag_amd_debug.h behind vrag_debug_topk_launch_log_read (tests/test_capi_abi.py compares the two)
DEBUG_TOPK_LAUNCH_IDS = {name: i for i, name in enumerate((
    "DENSE_BF16", "DENSE_F32", "MFMA", "MFMA2", "EXACT", "EXACT2", "SEED_THRESHOLD", "PF_PREFIX", "PF_COLLECT", "PF_COLLECT_MULTI",
    "PF_RESCORE_LIST", "PF_RESCORE", "PF_COMBINE", "SPARSE", "SPARSE_SCATTER", "SPARSE_MULTI", "MERGE_LISTS", "MERGE_SCAN"))}


class DebugGemmArgs(C.Structure):
    """vrag_debug_gemm_args (include/vrag_amd_debug.h), field for field; tests/test_capi_abi.py checks the layout against the
    host compiler's."""
    _fields_ = [(n, C.c_void_p) for n in (
        "A", "W", "bias", "ln_s", "stats_in", "res_mu", "res_rstd", "res_g", "res_b", "rope_cos", "rope_sin", "pos", "tok_seq",
        "lo_in", "out_f32", "out_bf16", "q", "k", "vt", "ln_mu", "ln_rstd", "ln_shift", "ln_shift_prev", "resid_bf16",
        "stats_part", "lo_out", "splade_rows")] + [(n, C.c_int32) for n in (
        "epi", "M", "N", "K", "f16", "act_gelu", "row0", "rows", "hidden", "rope_rows", "n_seqs", "small_rows")] + [
        ("q_scale", C.c_float), ("fin_eps", C.c_float), ("config", C.c_int32 * 7), ("f16_saturated", C.c_int32)]


class DebugQkvAttnArgs(C.Structure):
    """vrag_debug_qkv_attn_args (include/vrag_amd_debug.h), field for field; tests/test_capi_abi.py checks the layout too."""
    _fields_ = [(n, C.c_void_p) for n in (
        "x", "w", "ln_s", "ln_mu", "ln_rstd", "rope_cos", "rope_sin", "o", "seq_row", "seq_len", "groups_out")] + [
        (n, C.c_int32) for n in ("rows", "H", "nh", "rope_rows", "n_seqs", "packer", "local", "window", "f16")] + [
        ("q_scale", C.c_float), ("n_groups", C.c_int32), ("f16_saturated", C.c_int32), ("debug_flags", C.c_int32)]


class DebugAttnArgs(C.Structure):
    """vrag_debug_attn_args (include/vrag_amd_debug.h), field for field; tests/test_capi_abi.py checks the layout too."""
    _fields_ = [(n, C.c_void_p) for n in ("q", "k", "vt", "o", "seq_row", "seq_len", "blocks_out")] + [
        (n, C.c_int32) for n in ("rows", "H", "n_seqs", "local", "window", "f16", "blocks_cap", "n_blocks", "f16_saturated")]


class DebugRowsArgs(C.Structure):
    """vrag_debug_rows_args (include/vrag_amd_debug.h), field for field; tests/test_capi_abi.py checks the layout too."""
    _fields_ = [(n, C.c_void_p) for n in (
        "h", "ids", "E", "P", "pos", "type_row", "type_ids", "w", "bias", "start", "end", "first_row", "seq_row", "seq_len", "Wp",
        "bp", "WdT", "bd", "wn", "bn", "Wc", "bc", "out_f32", "out16", "out_lo", "row_mean", "pooled")] + [
        (n, C.c_int32) for n in ("op", "H", "rows", "h_rows", "out_rows", "vocab", "n_pos", "n_types", "num_labels", "mode",
                                 "gelu_first", "split3", "alias_f32", "f16", "no_sat")] + [
        ("eps", C.c_float), ("launch_status", C.c_int32), ("f16_saturated", C.c_int32)]


DEBUG_ROWS_OPS = {"embed_ln": 0, "layernorm": 1, "range_pool": 2, "ln_classifier": 3, "pooler_classifier": 4, "seq_head": 5}


class DebugGlueArgs(C.Structure):
    """vrag_debug_glue_args (include/vrag_amd_debug.h), field for field; tests/test_capi_abi.py checks the layout too."""
    _fields_ = [(n, C.c_void_p) for n in (
        "src", "col_scale", "dst", "dst_lo", "row_sum", "part", "mu", "rstd", "shift_in", "shift_out", "shift_prev", "packed",
        "seq_row", "seq_src", "seq_len", "ids", "pos", "tok_seq", "counts", "idx", "val", "w", "s", "w_out", "s_out")] + [
        (n, C.c_int32) for n in ("op", "f16", "rows_dst", "rows_src", "cols", "interleave", "I", "out_rows", "rows", "ld", "row0",
                                 "H", "np", "nh", "alias_shift", "n_seqs", "n_packed", "pad_id", "V", "cap")] + [
        ("thr", C.c_float), ("eps", C.c_float), ("f16_saturated", C.c_int32)]


DEBUG_GLUE_OPS = {"cvt_rows": 0, "cvt_split3": 1, "ln_stats_finalize": 2, "pack_layout": 3, "splade_compact": 4,
                  "permute_qkv_heads": 5}



class DebugTopkArgs(C.Structure):
    """vrag_debug_topk_args (include/vrag_amd_debug.h), field for field; tests/test_capi_abi.py checks the layout too."""
    _fields_ = [(n, C.c_void_p) for n in (
        "corpus", "w", "queries", "eps", "src", "w_out", "buf", "cnt", "thr_key", "thr_score", "out", "ovf", "done")] + [
        (n, C.c_int32) for n in ("op", "M", "N", "K", "corpus_rows", "nq", "nq_buf", "k", "cap", "pairs", "direct", "tile")] + [
        ("row_base", C.c_uint32)] + [
        (n, C.c_int32) for n in ("tile_stride", "tile_skip", "tile0", "n", "src_stride", "slices", "small_rows")] + [
        ("config", C.c_int32 * 7)]


DEBUG_TOPK_OPS = {"score_stage": 0, "queries": 1, "select": 2, "select_direct": 3, "rescue": 4, "merge": 5, "tau": 6}



class DebugTextArgs(C.Structure):
    """vrag_debug_text_args (include/vrag_amd_debug.h), field for field; tests/test_capi_abi.py checks the layout too."""
    _fields_ = [(n, C.c_void_p) for n in ("in", "out", "key", "row", "tf", "ukeys", "pstart", "prow", "ptf", "pkey")] + [
        (n, C.c_void_p * 4) for n in ("seg_keys", "seg_pstart", "seg_prow", "seg_ptf", "seg_df")] + [
        (n, C.c_void_p) for n in ("dl", "live", "allow", "acc", "kd", "qkeys", "tu", "df_out", "q_indptr", "w", "bound", "cand")] + [
        (n, C.c_int64 * 4) for n in ("seg_n_keys", "seg_n_post", "seg_row_lo", "seg_n_rows")] + [
        (n, C.c_int64) for n in ("n", "n_buf", "post_buf", "keys_buf", "n_rows", "rows_buf", "allow_rows", "n_terms", "terms_buf",
                                 "cand_buf", "corpus_n", "corpus_sum_dl", "n_post", "n_keys")] + [
        (n, C.c_int32) for n in ("op", "by_row", "row_bits", "unit", "n_segs", "nq", "kk")] + [
        ("k1", C.c_float), ("b", C.c_float), ("k1p1", C.c_float)]


DEBUG_TEXT_OPS = {"scan": 0, "sort": 1, "rle": 2, "fold": 3, "stats": 4, "lookup": 5, "score": 6}


class DebugTextIndexState(C.Structure):
    """vrag_debug_text_index_state (include/vrag_amd_debug.h), field for field; tests/test_capi_abi.py checks the layout too."""
    _fields_ = [(n, C.c_void_p * 2) for n in ("keys", "pstart", "prow", "ptf", "df")] + [
        (n, C.c_void_p) for n in ("dl", "kd", "live")] + [
        (n, C.c_int64 * 2) for n in ("row_lo", "seg_rows", "n_keys", "n_post")] + [
        (n, C.c_int64) for n in ("n_rows", "n_live", "sum_dl")] + [("n_segs", C.c_int32), ("with_data", C.c_int32)]


_DBG = None


def library_path() -> str:
    return os.environ.get("VRAG_AMD_LIB", os.path.join(_HERE, "libvrag_amd.so"))


def _preload_torch_hip_runtime() -> None:
    """One HIP runtime per process.  PyTorch-ROCm wheels bundle their own `libamdhip64.so` and link it by that
    un-versioned name, so when libvrag_amd.so (linked against the system `libamdhip64.so.7`) is loaded BEFORE torch, the
    loader does not recognise the two as the same library and maps both: torch then finds no usable GPU, and stream
    handles could not cross between the two runtimes.  Mapping torch's copy first (without importing torch) makes
    libvrag_amd.so bind to it by SONAME -- the arrangement that `import torch` before this package produces anyway."""
    import importlib.util
    import sys

    if "torch" in sys.modules:
        return
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        spec = None
    if spec is None or not spec.origin:
        return
    cand = os.path.join(os.path.dirname(spec.origin), "lib", "libamdhip64.so")
    if os.path.exists(cand):
        try:
            C.CDLL(cand, mode=C.RTLD_GLOBAL)
        except OSError:
            pass


def load() -> C.CDLL:
    """Loads the shared library and binds every declared symbol (raises if anything is missing)."""
    global _LIB
    with _LOCK:
        if _LIB is not None:
            return _LIB
        path = library_path()
        if not os.path.exists(path):
            raise ImportError(
                f"{path} not found: build it with `python __graft_entry__.py build` "
                "(hipcc --offload-arch=gfx950). verbatim_rag_amd has no CPU fallback."
            )
        _preload_torch_hip_runtime()
        lib = C.CDLL(path)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(lib, name)  # AttributeError if the symbol is not exported
            fn.restype = res
            fn.argtypes = args
        if lib.vrag_abi_version() != ABI_VERSION:
            raise ImportError(f"{path}: ABI version {lib.vrag_abi_version()} != {ABI_VERSION}")
        _LIB = lib
        return lib


def debug_library_path() -> str:
    return os.environ.get("VRAG_AMD_DEBUG_LIB", os.path.join(_HERE, "libvrag_amd_dbg.so"))


def load_debug() -> C.CDLL:
    """The harness library (include/vrag_amd_debug.h; tools/ and the attention unit test): the product sources plus the
    synthetic-operand timing loops.  The product path never loads it."""
    global _DBG
    with _LOCK:
        if _DBG is not None:
            return _DBG
        path = debug_library_path()
        if not os.path.exists(path):
            raise ImportError(f"{path} not found: build it with `python __graft_entry__.py build`")
        _preload_torch_hip_runtime()
        lib = C.CDLL(path)
        for name, (res, args) in DEBUG_SIGNATURES.items():
            fn = getattr(lib, name)
            fn.restype = res
            fn.argtypes = args
        # the harness library is a full build: searches through ITS index entry points are the ones its launch log records
        for name, (res, args) in SIGNATURES.items():
            if name.startswith(("vrag_dense_index_", "vrag_sparse_index_")):
                fn = getattr(lib, name)
                fn.restype = res
                fn.argtypes = args
        lib.vrag_last_error.restype = C.c_char_p
        lib.vrag_set_small_batch_rows.restype = C.c_int     # the harness library is a full build: its own copy of the threshold
        lib.vrag_set_small_batch_rows.argtypes = [C.c_int32]
        _DBG = lib
        return lib


def check_debug(fn: str, status: int) -> None:
    if status != VRAG_OK:
        msg = load_debug().vrag_last_error()
        raise VragError(fn, status, msg.decode("utf-8", "replace") if msg else "")


def last_error() -> str:
    msg = load().vrag_last_error()
    return msg.decode("utf-8", "replace") if msg else ""


def check(fn: str, status: int) -> None:
    if status != VRAG_OK:
        raise VragError(fn, status, last_error())


def require_gpu() -> None:
    if load().vrag_device_count() <= 0:
        raise RuntimeError(
            "verbatim_rag_amd: no HIP device visible. The MI355X hot path has no CPU fallback; "
            "use the reference's own providers on machines without a GPU."
        )
