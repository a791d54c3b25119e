"""ctypes binding of libmi355_retrieval.so (include/mi355_retrieval.h).

The HIP library IS the product path: if it cannot be loaded this module raises — there is no
CPU or eager-torch fallback anywhere in the package.
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# MI355_LIB_PATH: another build of the same library (developer A/B runs of two kernel variants on one box)
LIB_PATH = os.environ.get("MI355_LIB_PATH") or os.path.join(_HERE, "libmi355_retrieval.so")

c_f32p = C.POINTER(C.c_float)
c_i64p = C.POINTER(C.c_int64)
vp = C.c_void_p


class GemmExArgs(C.Structure):
    """mi355_gemm_ex_args (include/mi355_retrieval.h), the operand block of the developer entry mi355_gemm_bf16_ex."""
    _fields_ = [("A", vp), ("lda", C.c_int), ("W", vp), ("ldw", C.c_int), ("bias", vp),
                ("res", vp), ("ldr", C.c_int), ("res_n", C.c_int),
                ("gate", vp), ("gate_ld", C.c_int), ("rows_per_img", C.c_int), ("a_relu6", C.c_int),
                ("out", vp), ("ldo", C.c_int), ("out_f32", C.c_int),
                ("M", C.c_int), ("N", C.c_int), ("K", C.c_int), ("act", C.c_int),
                ("M_sel", C.c_int64), ("splitk_ws", vp), ("splitk_ws_bytes", C.c_size_t),
                ("ln_stats", vp), ("ln_colsum", vp)]


class DwconvExArgs(C.Structure):
    """mi355_dwconv_ex_args (include/mi355_retrieval.h), the operand block of the developer entry mi355_dwconv_se_ex."""
    _fields_ = [("in_", vp), ("w", vp), ("bias", vp), ("out", vp),
                ("B", C.c_int), ("H", C.c_int), ("W", C.c_int), ("C", C.c_int), ("k", C.c_int), ("stride", C.c_int),
                ("act", C.c_int), ("choice", C.c_int),
                ("se_w1", vp), ("se_b1", vp), ("se_w2t", vp), ("se_b2", vp), ("rd", C.c_int), ("act1", C.c_int),
                ("gate", vp), ("squeeze", vp)]


class MbconvFrontArgs(C.Structure):
    """mi355_mbconv_front_args (include/mi355_retrieval.h), the operand block of the developer entry mi355_mbconv_front_ex."""
    _fields_ = [("X", vp), ("We", vp), ("be", vp), ("Wd", vp), ("bd", vp), ("D", vp), ("pool", vp),
                ("B", C.c_int), ("H", C.c_int), ("W", C.c_int), ("Cin", C.c_int), ("mid", C.c_int), ("k", C.c_int),
                ("stride", C.c_int), ("act_e", C.c_int), ("act_d", C.c_int),
                ("kernel", C.c_int), ("band_rows", C.c_int), ("sweep_variant", C.c_int), ("sweep_csplit", C.c_int)]


class MbconvBlockArgs(C.Structure):
    """mi355_mbconv_block_args (include/mi355_retrieval.h), the operand block of the developer entry mi355_mbconv_block_ex."""
    _fields_ = [("X", vp), ("We", vp), ("be", vp), ("Wd", vp), ("bd", vp), ("W1", vp), ("b1", vp), ("W2", vp), ("b2", vp),
                ("Wp", vp), ("bp", vp), ("D", vp), ("Y", vp),
                ("B", C.c_int), ("H", C.c_int), ("W", C.c_int), ("Cin", C.c_int), ("mid", C.c_int), ("Cout", C.c_int),
                ("k", C.c_int), ("stride", C.c_int), ("rd", C.c_int), ("act_e", C.c_int), ("act_d", C.c_int),
                ("se_act", C.c_int), ("a_relu6", C.c_int), ("has_res", C.c_int), ("res_n", C.c_int), ("norot", C.c_int)]


class StemExArgs(C.Structure):
    """mi355_stem_ex_args (include/mi355_retrieval.h), the operand block of the developer entry mi355_stem_ex."""
    _fields_ = [("x", vp), ("images", vp), ("images_bytes", C.c_int64), ("desc_host", vp), ("desc_dev", vp),
                ("B", C.c_int), ("H", C.c_int), ("W", C.c_int), ("fill", C.c_int), ("mean", c_f32p), ("stdv", c_f32p),
                ("conv_input_w", vp), ("w", vp), ("bias", vp), ("out", vp), ("Cout", C.c_int), ("act", C.c_int)]


DW_CHOICE_AUTO, DW_CHOICE_DIRECT, DW_CHOICE_TILED, DW_CHOICE_MFMA = 0, 1, 2, 3


class RankFilter(C.Structure):
    """mi355_rank_filter (include/mi355_retrieval.h): the eligibility filter of mi355_rank_topk_filtered / _f16_filtered."""
    _fields_ = [("query_labels", vp), ("gallery_labels", vp), ("label_mode", C.c_int), ("exclude", vp)]


class ScoreAdjust(C.Structure):
    """mi355_score_adjust (include/mi355_retrieval.h): the four nullable coefficient vectors of the adjusted searches."""
    _fields_ = [("aq", vp), ("bq", vp), ("ag", vp), ("bg", vp)]


LABEL_ANY, LABEL_SAME, LABEL_DIFFERENT = 0, 1, 2
DTYPE_F32, DTYPE_F16 = 0, 1

# name -> (restype, argtypes); must list every symbol include/mi355_retrieval.h declares
# (tests/test_abi.py cross-checks this table against the header).
PROTOTYPES = {
    "mi355_abi_version": (C.c_int, []),
    "mi355_last_error": (C.c_char_p, []),
    "mi355_device_count": (C.c_int, []),
    "mi355_synth_fill": (C.c_int, [vp, C.c_int64, C.c_uint64, C.c_int64, C.c_int, vp]),
    "mi355_l2_normalize_rows": (C.c_int, [vp, vp, C.c_int64, C.c_int, C.c_float, vp]),
    "mi355_rank_workspace_bytes": (C.c_size_t, [C.c_int64, C.c_int64, C.c_int, C.c_int]),
    "mi355_rank_topk": (C.c_int, [vp, C.c_int64, vp, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_float,
                                  C.c_int64, vp, vp, vp, C.c_size_t, vp]),
    "mi355_gallery_planes_bytes": (C.c_size_t, [C.c_int64, C.c_int]),
    "mi355_gallery_prepare": (C.c_int, [vp, C.c_int64, C.c_int, vp, C.c_size_t, vp]),
    "mi355_rank_topk_prepared": (C.c_int, [vp, C.c_int64, vp, C.c_int64, C.c_int, C.c_int, C.c_float, C.c_int64, vp, vp, vp,
                                           C.c_size_t, vp]),
    "mi355_gallery_f16_bytes": (C.c_size_t, [C.c_int64, C.c_int]),
    "mi355_gallery_to_f16": (C.c_int, [vp, C.c_int64, C.c_int, C.c_int, C.c_float, vp, C.c_size_t, vp]),
    "mi355_rank_f16_workspace_bytes": (C.c_size_t, [C.c_int64, C.c_int64, C.c_int, C.c_int]),
    "mi355_rank_topk_f16": (C.c_int, [vp, C.c_int64, vp, C.c_int64, C.c_int, C.c_int, C.c_float, C.c_int64, vp, vp, vp,
                                      C.c_size_t, vp]),
    "mi355_rank_topk_filtered": (C.c_int, [vp, C.c_int64, vp, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_float, C.c_int64,
                                           C.POINTER(RankFilter), vp, vp, vp, C.c_size_t, vp]),
    "mi355_rank_topk_f16_filtered": (C.c_int, [vp, C.c_int64, vp, C.c_int64, C.c_int, C.c_int, C.c_float, C.c_int64,
                                               C.POINTER(RankFilter), vp, vp, vp, C.c_size_t, vp]),
    "mi355_rank_adjusted_workspace_bytes": (C.c_size_t, [C.c_int64, C.c_int64, C.c_int, C.c_int]),
    "mi355_rank_adjusted_f16_workspace_bytes": (C.c_size_t, [C.c_int64, C.c_int64, C.c_int, C.c_int]),
    "mi355_rank_topk_adjusted": (C.c_int, [vp, C.c_int64, vp, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_float, C.c_int64,
                                           C.POINTER(ScoreAdjust), C.POINTER(RankFilter), C.c_int64, vp, vp, vp, C.c_size_t, vp]),
    "mi355_rank_topk_adjusted_f16": (C.c_int, [vp, C.c_int64, vp, C.c_int64, C.c_int, C.c_int, C.c_float, C.c_int64,
                                               C.POINTER(ScoreAdjust), C.POINTER(RankFilter), C.c_int64, vp, vp, vp, C.c_size_t, vp]),
    "mi355_cosine_scores_adjusted": (C.c_int, [vp, C.c_int64, vp, C.c_int64, C.c_int, C.c_int, C.c_float, C.POINTER(ScoreAdjust),
                                               C.c_int64, vp, vp, C.c_size_t, vp]),
    "mi355_cosine_scores_adjusted_f16": (C.c_int, [vp, C.c_int64, vp, C.c_int64, C.c_int, C.c_float, C.POINTER(ScoreAdjust),
                                                   C.c_int64, vp, vp, C.c_size_t, vp]),
    "mi355_topn_stats": (C.c_int, [vp, vp, C.c_int64, C.c_int, C.c_double, C.c_double, vp, vp, vp, vp, vp, vp]),
    "mi355_gallery_i8_bytes": (C.c_size_t, [C.c_int64, C.c_int]),
    "mi355_gallery_to_i8": (C.c_int, [vp, C.c_int64, C.c_int, C.c_int, C.c_float, vp, C.c_size_t, vp, vp]),
    "mi355_rank_i8_workspace_bytes": (C.c_size_t, [C.c_int64, C.c_int64, C.c_int, C.c_int]),
    "mi355_rank_topk_i8": (C.c_int, [vp, C.c_int64, vp, vp, C.c_int64, C.c_int, C.c_int, C.c_float, C.c_int64, vp, vp, vp,
                                     C.c_size_t, vp]),
    "mi355_rank_topk_i8_filtered": (C.c_int, [vp, C.c_int64, vp, vp, C.c_int64, C.c_int, C.c_int, C.c_float, C.c_int64,
                                              C.POINTER(RankFilter), vp, vp, vp, C.c_size_t, vp]),
    "mi355_range_i8_workspace_bytes": (C.c_size_t, [C.c_int64, C.c_int64, C.c_int]),
    "mi355_cosine_range_i8": (C.c_int, [vp, C.c_int64, vp, vp, C.c_int64, C.c_int, C.c_float, C.c_double, C.c_int64,
                                        C.POINTER(RankFilter), vp, C.c_int64, C.POINTER(C.c_int64), vp, C.c_size_t, vp]),
    "mi355_gallery_fp4_bytes": (C.c_size_t, [C.c_int64, C.c_int]),
    "mi355_gallery_to_fp4": (C.c_int, [vp, C.c_int64, C.c_int, C.c_int, C.c_float, vp, C.c_size_t, vp, vp]),
    "mi355_rank_fp4_workspace_bytes": (C.c_size_t, [C.c_int64, C.c_int64, C.c_int, C.c_int]),
    "mi355_rank_topk_fp4": (C.c_int, [vp, C.c_int64, vp, vp, C.c_int64, C.c_int, C.c_int, C.c_float, C.c_int64, vp, vp, vp,
                                      C.c_size_t, vp]),
    "mi355_rank_topk_fp4_filtered": (C.c_int, [vp, C.c_int64, vp, vp, C.c_int64, C.c_int, C.c_int, C.c_float, C.c_int64,
                                               C.POINTER(RankFilter), vp, vp, vp, C.c_size_t, vp]),
    "mi355_range_fp4_workspace_bytes": (C.c_size_t, [C.c_int64, C.c_int64, C.c_int]),
    "mi355_cosine_range_fp4": (C.c_int, [vp, C.c_int64, vp, vp, C.c_int64, C.c_int, C.c_float, C.c_double, C.c_int64,
                                         C.POINTER(RankFilter), vp, C.c_int64, C.POINTER(C.c_int64), vp, C.c_size_t, vp]),
    "mi355_rank_last_path": (C.c_int, []),
    "mi355_rank_round_split": (C.c_int, [C.c_int, C.c_int, C.c_int]),
    "mi355_rank_set_round_slots": (C.c_int, [C.c_int]),
    "mi355_rank_last_tiles": (C.c_int, [C.POINTER(C.c_int), C.c_int]),
    "mi355_expand_workspace_bytes": (C.c_size_t, [C.c_int64, C.c_int, C.c_int]),
    "mi355_expand_rows": (C.c_int, [vp, C.c_int, C.c_int64, C.c_int, vp, C.c_int, C.c_int64, C.c_int64, C.c_int, vp, vp,
                                    C.c_int64, C.c_int, C.c_int64, C.c_float, C.c_float, vp, C.c_int, C.c_int64, vp,
                                    C.c_size_t, vp]),
    "mi355_kr_sets": (C.c_int, [vp, vp, vp, C.c_int64, C.c_int, vp, C.c_int64, vp, vp, C.c_int64, vp]),
    "mi355_kr_weights": (C.c_int, [vp, C.c_int, C.c_int64, C.c_int64, vp, C.c_int, C.c_int64, C.c_int64, C.c_int, vp, vp,
                                   C.c_int64, vp, vp]),
    "mi355_kr_local_qe": (C.c_int, [vp, C.c_int64, C.c_int, C.c_int, vp, vp, vp, C.c_int64, vp, vp, vp, C.c_int64, C.c_int64,
                                    vp, vp, vp, C.c_int64, vp]),
    "mi355_kr_score": (C.c_int, [vp, vp, vp, C.c_int64, C.c_int64, vp, vp, vp, C.c_int64, C.c_int64, vp, vp, C.c_int,
                                 C.c_float, vp, vp]),
    "mi355_diffusion_graph": (C.c_int, [vp, vp, C.c_int64, C.c_int, C.c_int, vp, vp, vp, vp]),
    "mi355_diffusion_source": (C.c_int, [vp, vp, C.c_int64, C.c_int, C.c_int, C.c_int, vp, vp]),
    "mi355_diffusion_lds_bytes": (C.c_size_t, [C.c_int, C.c_int]),
    "mi355_diffusion_solve": (C.c_int, [vp, vp, C.c_int64, C.c_int, vp, vp, C.c_int64, C.c_int, C.c_float, C.c_int, vp, vp, vp]),
    "mi355_aggregate_workspace_bytes": (C.c_size_t, [C.c_int64, C.c_int, C.c_int]),
    "mi355_aggregate_regions": (C.c_int, [vp, C.c_int64, C.c_int, C.c_int, C.c_int, vp, C.c_int, C.c_int, C.c_float, vp, C.c_float,
                                          C.c_int, C.c_int, C.c_float, vp, vp, C.c_size_t, vp]),
    "mi355_aggregate_crow": (C.c_int, [vp, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, vp, vp, C.c_size_t, vp]),
    "mi355_aggregate_sum": (C.c_int, [vp, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_float, vp, vp]),
    "mi355_region_scores_lds_bytes": (C.c_size_t, [C.c_int, C.c_int]),
    "mi355_region_scores": (C.c_int, [vp, C.c_int64, C.c_int, vp, C.c_int64, C.c_int, C.c_int, C.c_int, vp, C.c_int64, vp, vp, vp, vp]),
    "mi355_shortlist_gram": (C.c_int, [vp, C.c_int, C.c_int64, C.c_int64, C.c_int, vp, C.c_int64, C.c_int, vp, vp]),
    "mi355_mmr_select": (C.c_int, [vp, vp, vp, C.c_int64, C.c_int, C.c_int, C.c_float, C.c_float, C.c_int64, vp, vp, vp, vp, vp]),
    "mi355_moments_workspace_bytes": (C.c_size_t, [C.c_int64, C.c_int]),
    "mi355_embedding_moments": (C.c_int, [vp, C.c_int, C.c_int64, C.c_int64, C.c_int, C.c_int, C.c_float, C.c_int, vp, vp, vp,
                                          C.c_size_t, vp]),
    "mi355_whiten_workspace_bytes": (C.c_size_t, [C.c_int64, C.c_int, C.c_int, C.c_int]),
    "mi355_whiten_rows": (C.c_int, [vp, C.c_int, C.c_int64, C.c_int64, C.c_int, C.c_int, C.c_float, vp, vp, C.c_int, C.c_int, vp,
                                    C.c_int, C.c_int64, vp, C.c_size_t, vp]),
    "mi355_clear_pads": (C.c_int, [vp, vp, C.c_int64, C.c_int64, C.c_int64, vp]),
    "mi355_range_workspace_bytes": (C.c_size_t, [C.c_int64, C.c_int64, C.c_int]),
    "mi355_cosine_range": (C.c_int, [vp, C.c_int64, vp, C.c_int64, C.c_int, C.c_int, C.c_float, C.c_double, C.c_int64,
                                     C.POINTER(RankFilter), vp, C.c_int64, C.POINTER(C.c_int64), vp, C.c_size_t, vp]),
    "mi355_range_f16_workspace_bytes": (C.c_size_t, [C.c_int64, C.c_int64, C.c_int]),
    "mi355_cosine_range_f16": (C.c_int, [vp, C.c_int64, vp, C.c_int64, C.c_int, C.c_float, C.c_double, C.c_int64,
                                         C.POINTER(RankFilter), vp, C.c_int64, C.POINTER(C.c_int64), vp, C.c_size_t, vp]),
    "mi355_range_compact": (C.c_int, [vp, C.c_int64, C.c_int64, C.c_int64, C.c_int64, vp, C.c_size_t, vp, vp, vp, vp]),
    "mi355_positives_range": (C.c_int, [vp, C.c_int64, vp, C.c_int64, C.c_int, C.c_int, C.c_float, C.c_int64,
                                        C.POINTER(RankFilter), vp, C.c_int64, C.POINTER(C.c_int64), vp, C.c_size_t, vp]),
    "mi355_positives_range_f16": (C.c_int, [vp, C.c_int64, vp, C.c_int64, C.c_int, C.c_float, C.c_int64,
                                            C.POINTER(RankFilter), vp, C.c_int64, C.POINTER(C.c_int64), vp, C.c_size_t, vp]),
    "mi355_rank_positives_keys": (C.c_int, [vp, vp, C.c_int64, C.c_int64, vp, vp]),
    "mi355_rank_positives_workspace_bytes": (C.c_size_t, [C.c_int64, C.c_int64, C.c_int]),
    "mi355_rank_positives": (C.c_int, [vp, C.c_int64, vp, C.c_int64, C.c_int, C.c_int, C.c_float, vp, vp, vp, C.c_int64, vp,
                                       C.POINTER(C.c_int64), vp, C.c_int64, vp, C.c_int64, vp, C.c_size_t, vp]),
    "mi355_rank_positives_f16_workspace_bytes": (C.c_size_t, [C.c_int64, C.c_int64, C.c_int]),
    "mi355_rank_positives_f16": (C.c_int, [vp, C.c_int64, vp, C.c_int64, C.c_int, C.c_float, vp, vp, vp, C.c_int64, vp,
                                           C.POINTER(C.c_int64), vp, C.c_int64, vp, C.c_int64, vp, C.c_size_t, vp]),
    "mi355_rank_positives_finalize": (C.c_int, [vp, vp, C.c_int64, C.c_int64, vp, vp, vp, vp]),
    "mi355_nearest_centroid_workspace_bytes": (C.c_size_t, [C.c_int64, C.c_int64, C.c_int]),
    "mi355_nearest_centroid": (C.c_int, [vp, C.c_int64, vp, C.c_int64, C.c_int, C.c_int, C.c_float, C.c_int64, vp, vp, vp,
                                         C.c_size_t, vp]),
    "mi355_nearest_centroid_f16_workspace_bytes": (C.c_size_t, [C.c_int64, C.c_int64, C.c_int]),
    "mi355_nearest_centroid_f16": (C.c_int, [vp, C.c_int64, vp, C.c_int64, C.c_int, C.c_float, C.c_int64, vp, vp, vp,
                                             C.c_size_t, vp]),
    "mi355_cluster_members_workspace_bytes": (C.c_size_t, [C.c_int64, C.c_int64]),
    "mi355_cluster_members": (C.c_int, [vp, C.c_int64, C.c_int64, vp, vp, vp, C.c_size_t, vp]),
    "mi355_centroid_update_workspace_bytes": (C.c_size_t, [C.c_int64, C.c_int64, C.c_int]),
    "mi355_centroid_update": (C.c_int, [vp, C.c_int64, C.c_int, vp, C.c_int64, vp, C.c_float, vp, vp, vp, vp, vp, C.c_size_t,
                                        vp]),
    "mi355_centroid_update_f16_workspace_bytes": (C.c_size_t, [C.c_int64, C.c_int64, C.c_int]),
    "mi355_centroid_update_f16": (C.c_int, [vp, C.c_int64, C.c_int, vp, C.c_int64, vp, C.c_float, vp, vp, vp, vp, vp,
                                            C.c_size_t, vp]),
    "mi355_contingency_workspace_bytes": (C.c_size_t, [C.c_int64, C.c_int64, C.c_int64]),
    "mi355_contingency": (C.c_int, [vp, vp, C.c_int64, C.c_int64, C.c_int64, vp, vp, C.c_size_t, vp]),
    "mi355_dbscan_workspace_bytes": (C.c_size_t, [C.c_int64, C.c_int64, C.c_int]),
    "mi355_dbscan_f16_workspace_bytes": (C.c_size_t, [C.c_int64, C.c_int64, C.c_int]),
    "mi355_dbscan_init": (C.c_int, [C.c_int64, vp, vp, vp, vp]),
    "mi355_dbscan_degree": (C.c_int, [vp, C.c_int64, C.c_int64, vp, C.c_int64, C.c_int, C.c_int, C.c_float, C.c_double, vp, vp,
                                      C.c_size_t, vp]),
    "mi355_dbscan_degree_f16": (C.c_int, [vp, C.c_int64, C.c_int64, vp, C.c_int64, C.c_int, C.c_float, C.c_double, vp, vp,
                                          C.c_size_t, vp]),
    "mi355_dbscan_link": (C.c_int, [vp, C.c_int64, C.c_int64, vp, C.c_int64, C.c_int, C.c_int, C.c_float, C.c_double, C.c_int, vp,
                                    vp, vp, vp, C.c_size_t, vp]),
    "mi355_dbscan_link_f16": (C.c_int, [vp, C.c_int64, C.c_int64, vp, C.c_int64, C.c_int, C.c_float, C.c_double, C.c_int, vp, vp,
                                        vp, vp, C.c_size_t, vp]),
    "mi355_dbscan_finish": (C.c_int, [C.c_int64, C.c_int, vp, vp, vp, vp, vp, vp]),
    "mi355_ivf_scan_workspace_bytes": (C.c_size_t, [C.c_int64, C.c_int, C.c_int64, C.c_int, C.c_int64]),
    "mi355_ivf_scan": (C.c_int, [vp, C.c_int64, C.c_int, C.c_float, vp, C.c_int, C.c_int64, C.c_int64, vp, vp, C.c_int64, vp,
                                 C.c_int, C.c_int64, C.c_int64, C.POINTER(RankFilter), vp, vp, vp, C.c_size_t, vp]),
    "mi355_ivf_scan_i8_workspace_bytes": (C.c_size_t, [C.c_int64, C.c_int, C.c_int64, C.c_int, C.c_int64]),
    "mi355_ivf_scan_i8": (C.c_int, [vp, C.c_int64, C.c_int, C.c_float, vp, vp, C.c_int64, C.c_int64, vp, vp, C.c_int64, vp,
                                    C.c_int, C.c_int64, C.c_int64, C.POINTER(RankFilter), vp, vp, vp, C.c_size_t, vp]),
    "mi355_pq_encode_workspace_bytes": (C.c_size_t, [C.c_int64, C.c_int, C.c_int]),
    "mi355_pq_encode": (C.c_int, [vp, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_float, vp, vp, C.c_size_t, vp, C.c_size_t, vp]),
    "mi355_pq_update_workspace_bytes": (C.c_size_t, [C.c_int64, C.c_int, C.c_int]),
    "mi355_pq_update": (C.c_int, [vp, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_float, vp, vp, vp, vp, vp, C.c_size_t, vp]),
    "mi355_pq_search_workspace_bytes": (C.c_size_t, [C.c_int64, C.c_int64, C.c_int, C.c_int, C.c_int]),
    "mi355_pq_scores": (C.c_int, [vp, C.c_int64, C.c_int, C.c_float, vp, C.c_int, vp, C.c_int64, vp, vp, C.c_size_t, vp]),
    "mi355_pq_search": (C.c_int, [vp, C.c_int64, C.c_int, C.c_float, vp, C.c_int, vp, C.c_int64, C.c_int, C.c_int64,
                                  C.POINTER(RankFilter), vp, vp, vp, C.c_size_t, vp]),
    "mi355_rescore_candidates_workspace_bytes": (C.c_size_t, [C.c_int64, C.c_int]),
    "mi355_rescore_candidates": (C.c_int, [vp, C.c_int64, C.c_int, C.c_float, vp, C.c_int, C.c_int64, C.c_int64, vp, C.c_int64,
                                           C.c_int64, vp, vp, C.c_size_t, vp]),
    "mi355_binary_bytes": (C.c_size_t, [C.c_int64, C.c_int]),
    "mi355_binary_encode": (C.c_int, [vp, C.c_int64, C.c_int, C.c_int, C.c_float, vp, vp, C.c_size_t, vp]),
    "mi355_binary_search_workspace_bytes": (C.c_size_t, [C.c_int64, C.c_int64, C.c_int, C.c_int]),
    "mi355_binary_distances": (C.c_int, [vp, C.c_int64, C.c_int, C.c_float, vp, vp, C.c_int64, vp, vp, C.c_size_t, vp]),
    "mi355_binary_search": (C.c_int, [vp, C.c_int64, C.c_int, C.c_float, vp, vp, C.c_int64, C.c_int, C.c_int64,
                                      C.POINTER(RankFilter), vp, vp, vp, C.c_size_t, vp]),
    "mi355_binary_asym_search_workspace_bytes": (C.c_size_t, [C.c_int64, C.c_int64, C.c_int, C.c_int]),
    "mi355_binary_asym_query_codes": (C.c_int, [vp, C.c_int64, C.c_int, C.c_float, vp, vp, vp, vp, vp]),
    "mi355_binary_asym_distances": (C.c_int, [vp, C.c_int64, C.c_int, C.c_float, vp, vp, C.c_int64, vp, vp, C.c_size_t, vp]),
    "mi355_binary_asym_search": (C.c_int, [vp, C.c_int64, C.c_int, C.c_float, vp, vp, C.c_int64, C.c_int, C.c_int64,
                                           C.POINTER(RankFilter), vp, vp, vp, C.c_size_t, vp]),
    "mi355_ivfpq_search_workspace_bytes": (C.c_size_t, [C.c_int64, C.c_int, C.c_int64, C.c_int, C.c_int, C.c_int64, C.c_int]),
    "mi355_ivfpq_search": (C.c_int, [vp, C.c_int64, C.c_int, C.c_float, vp, C.c_int, vp, C.c_int64, vp, vp, C.c_int64, vp, C.c_int,
                                     C.c_int64, C.c_int, C.c_int64, C.POINTER(RankFilter), vp, vp, vp, C.c_size_t, vp]),
    "mi355_ivfpq_residuals": (C.c_int, [vp, C.c_int64, C.c_int, C.c_int, C.c_float, vp, vp, C.c_int64, vp, vp, C.c_size_t, vp]),
    "mi355_ivfpq_residual_search_workspace_bytes": (C.c_size_t, [C.c_int64, C.c_int, C.c_int64, C.c_int, C.c_int, C.c_int64,
                                                                 C.c_int]),
    "mi355_ivfpq_residual_search": (C.c_int, [vp, C.c_int64, C.c_int, C.c_float, vp, C.c_int, vp, C.c_int64, vp, vp, C.c_int64, vp,
                                              C.c_int, C.c_int64, C.c_int, C.c_int64, C.POINTER(RankFilter), vp, vp, vp, vp,
                                              C.c_size_t, vp]),
    "mi355_graph_search_workspace_bytes": (C.c_size_t, [C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
    "mi355_graph_search": (C.c_int, [vp, C.c_int64, C.c_int, C.c_float, vp, C.c_int, C.c_int64, C.c_int64, vp, C.c_int, vp, C.c_int,
                                     C.c_int, C.c_int, C.c_int, C.c_int64, C.POINTER(RankFilter), vp, vp, vp, vp, vp, C.c_size_t,
                                     vp]),
    "mi355_roc_pairs_workspace_bytes": (C.c_size_t, [C.c_int64, C.c_int64, C.c_int]),
    "mi355_roc_pairs_hist": (C.c_int, [vp, C.c_int64, vp, C.c_int64, C.c_int, C.c_int, C.c_float, vp, vp, vp, C.c_int64,
                                       C.POINTER(C.c_double), vp, C.c_int, vp, vp, C.c_size_t, vp]),
    "mi355_roc_pairs_f16_workspace_bytes": (C.c_size_t, [C.c_int64, C.c_int64, C.c_int]),
    "mi355_roc_pairs_hist_f16": (C.c_int, [vp, C.c_int64, vp, C.c_int64, C.c_int, C.c_float, vp, vp, vp, C.c_int64,
                                           C.POINTER(C.c_double), vp, C.c_int, vp, vp, C.c_size_t, vp]),
    "mi355_roc_scores_hist": (C.c_int, [vp, C.c_int, C.c_int64, vp, C.POINTER(C.c_double), vp, C.c_int, vp, vp]),
    "mi355_roc_finalize": (C.c_int, [vp, C.c_int, vp, vp, vp, vp, vp]),
    "mi355_retrieval_metrics": (C.c_int, [vp, C.c_int64, C.c_int, vp, vp, C.c_int64, vp, vp, vp]),
    "mi355_cosine_scores": (C.c_int, [vp, C.c_int64, vp, C.c_int64, C.c_int, C.c_int, C.c_float, vp, vp,
                                      C.c_size_t, vp]),
    "mi355_topk_rows": (C.c_int, [vp, C.c_int64, C.c_int64, C.c_int, C.c_int64, vp, vp, vp, C.c_size_t, vp]),
    "mi355_merge_topk": (C.c_int, [vp, vp, C.c_int64, C.c_int, C.c_int, vp, vp, vp, C.c_size_t, vp]),
    "mi355_pack_candidates": (C.c_int, [vp, vp, C.c_int64, C.c_int, C.c_int, vp, vp]),
    "mi355_merge_packed_workspace_bytes": (C.c_size_t, [C.c_int64, C.c_int, C.c_int]),
    "mi355_merge_packed_topk": (C.c_int, [vp, vp, C.c_int, C.c_int64, C.c_int, vp, vp, vp, C.c_size_t, vp]),
    "mi355_pair_cosine": (C.c_int, [vp, vp, C.c_int64, C.c_int, C.c_float, vp, vp]),
    "mi355_contrastive_loss": (C.c_int, [vp, vp, C.c_int64, C.c_int, C.c_float, C.c_float, C.c_int, vp, vp, vp]),
    "mi355_cosine_embedding_loss": (C.c_int, [vp, vp, C.c_int64, C.c_int, C.c_float, C.c_float, C.c_int, vp, vp]),
    "mi355_hit_counts": (C.c_int, [vp, C.c_int64, C.c_int, vp, vp, C.c_int64, vp, vp]),
    "mi355_distinct_class_topn": (C.c_int, [vp, vp, C.c_int64, C.c_int, vp, C.c_int64, C.c_int, vp, vp, vp, vp]),
    "mi355_model_create": (C.c_int, [C.c_char_p, C.c_int, C.POINTER(vp)]),
    "mi355_model_destroy": (None, [vp]),
    "mi355_model_num_tensors": (C.c_int, [vp]),
    "mi355_model_tensor_info": (C.c_int, [vp, C.c_int, C.POINTER(C.c_char_p), C.POINTER(C.c_int),
                                          C.POINTER(C.c_int64), C.POINTER(C.c_int)]),
    "mi355_model_feature_dim": (C.c_int, [vp]),
    "mi355_model_num_classes": (C.c_int, [vp]),
    "mi355_model_set_tensor": (C.c_int, [vp, C.c_char_p, vp, C.c_int64]),
    "mi355_model_pack": (C.c_int, [vp, vp]),
    "mi355_model_forward_features": (C.c_int, [vp, vp, C.c_int, C.c_int, C.c_int, vp, vp, vp]),
    "mi355_model_forward": (C.c_int, [vp, vp, C.c_int, C.c_int, C.c_int, vp, vp, vp]),
    "mi355_model_forward_u8": (C.c_int, [vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_float), C.POINTER(C.c_float),
                                         vp, C.c_int, vp, vp, vp]),
    "mi355_model_enable_taps": (C.c_int, [vp, C.c_int]),
    "mi355_model_read_tap": (C.c_int, [vp, C.c_char_p, vp, C.c_int64, C.POINTER(C.c_int64), vp]),
    "mi355_model_run_between_taps": (C.c_int, [vp, C.c_char_p, C.c_char_p, vp, C.c_int, C.c_int, C.c_int, C.c_int, vp]),
    "mi355_model_traffic": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_double),
                                      C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "mi355_model_traffic_kinds": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_double),
                                            C.POINTER(C.c_double), C.c_int]),
    "mi355_model_set_option": (C.c_int, [vp, C.c_char_p, C.c_int64]),
    "mi355_model_profile_read": (C.c_int, [vp, C.POINTER(C.c_double), C.POINTER(C.c_int64), C.c_int]),
    "mi355_model_profile_ops": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_double),
                                          C.POINTER(C.c_double), C.POINTER(C.c_int), C.c_char_p, C.c_int]),
    "mi355_model_plan": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int),
                                   C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_size_t)]),
    "mi355_model_block_stamps": (C.c_int, [vp, C.POINTER(C.c_double), C.c_int]),
    "mi355_pool_linear": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, vp, vp, C.c_int, vp, vp, vp]),
    "mi355_gemm_bf16": (C.c_int, [vp, vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp]),
    "mi355_gemm_bf16_ex": (C.c_int, [vp, C.POINTER(C.c_int), vp]),
    "mi355_dwconv_se_ex": (C.c_int, [vp, C.POINTER(C.c_int), vp]),
    "mi355_mbconv_front_ex": (C.c_int, [vp, C.POINTER(C.c_int), C.POINTER(C.c_int), vp]),
    "mi355_mbconv_block_ex": (C.c_int, [vp, C.POINTER(C.c_int), vp]),
    "mi355_mbconv_block_how": (C.c_int, [C.c_int] * 10 + [C.POINTER(C.c_int)]),
    "mi355_stem_ex": (C.c_int, [vp, C.POINTER(C.c_int), vp]),
    "mi355_head_gap_ex": (C.c_int, [vp, C.c_int, vp, C.c_int, vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                    C.POINTER(C.c_int), vp]),
    "mi355_gap": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, vp, vp, vp]),
    "mi355_nhwc_to_nchw": (C.c_int, [vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, vp]),
    "mi355_nchw_to_nhwc": (C.c_int, [vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, vp]),
    "mi355_window_attention": (C.c_int, [vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp]),
    "mi355_window_attention_ws": (C.c_int, [vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp]),
    "mi355_swin_layernorm": (C.c_int, [vp, vp, vp, vp, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, vp]),
    "mi355_swin_patch_embed": (C.c_int, [vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_float),
                                         C.POINTER(C.c_float), vp, vp, vp, vp, C.c_int, C.c_float, vp, vp]),
    "mi355_swin_ln_token_mean": (C.c_int, [vp, vp, vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_float, vp]),
    "mi355_square_pad_normalize": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_float), C.POINTER(C.c_float), vp, vp]),
    "mi355_conv_input_silu": (C.c_int, [vp, vp, C.c_int, C.c_int, C.c_int, vp, vp]),
    "mi355_resize_bilinear_u8": (C.c_int, [vp, C.c_int, C.c_int, vp, C.c_int, C.c_int, vp, vp]),
    "mi355_resize_batch_workspace_bytes": (C.c_size_t, [vp, C.c_int, C.c_int, C.c_int, C.c_int]),
    "mi355_resize_batch_u8": (C.c_int, [vp, C.c_int64, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, C.c_size_t,
                                        vp]),
    "mi355_model_forward_images_workspace_bytes": (C.c_size_t, [vp, C.c_int, C.c_int, C.c_int]),
    "mi355_model_forward_images": (C.c_int, [vp, vp, C.c_int64, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_float),
                                             C.POINTER(C.c_float), vp, C.c_int, vp, vp, vp, C.c_size_t, vp]),
    "mi355_score_boost": (C.c_int, [vp, C.c_int64, C.c_float, C.c_float, C.c_float, C.c_int, vp, vp]),
}

_lib = None


class MI355Error(RuntimeError):
    """A libmi355_retrieval call returned nonzero; the message is mi355_last_error()."""


def lib() -> C.CDLL:
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(
                f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "(or `make -C imageretrievalresearch_amd/csrc`). There is no fallback path.")
        L = C.CDLL(LIB_PATH)
        for name, (res, args) in PROTOTYPES.items():
            fn = getattr(L, name)  # AttributeError here = header/library mismatch: fail loudly
            fn.restype = res
            fn.argtypes = args
        if L.mi355_abi_version() != 3:
            raise ImportError(f"ABI version mismatch: library {L.mi355_abi_version()} != binding 3")
        _lib = L
    return _lib


def check(status: int) -> None:
    if status != 0:
        raise MI355Error(lib().mi355_last_error().decode("utf-8", "replace"))


def stream_ptr(device=None) -> int:
    """Raw hipStream_t of torch's CURRENT stream, so results order correctly behind `.item()`."""
    import torch
    return torch.cuda.current_stream(device).cuda_stream


def require_cuda(t, name: str):
    if not t.is_cuda:
        raise MI355Error(f"{name} must live on the GPU (got device {t.device}); "
                         "the MI355X path has no CPU fallback")
