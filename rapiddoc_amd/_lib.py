"""ctypes binding of librapiddoc_mi355.so (include/rapiddoc_mi355.h).  No fallback: if the library is
missing or no MI355X is visible, importing callers get a loud error."""
from __future__ import annotations

import ctypes as C
from pathlib import Path

_PKG = Path(__file__).resolve().parent
LIB_PATH = _PKG / "librapiddoc_mi355.so"
_lib = None

SYMBOLS = {
    "rd_version": (C.c_char_p, []),
    "rd_create": (C.c_void_p, [C.c_int, C.c_char_p]),
    "rd_create_error": (C.c_char_p, []),
    "rd_destroy": (None, [C.c_void_p]),
    "rd_last_error": (C.c_char_p, [C.c_void_p]),
    "rd_load_weights": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t]),
    "rd_query_workspace": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_size_t)]),
    "rd_det_forward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "rd_det_forward_ex": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "rd_rec_forward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p]),
    "rd_rec_num_classes": (C.c_int, [C.c_void_p]),
    "rd_backbone_name": (C.c_char_p, [C.c_void_p]),
    "rd_rec_token_dim": (C.c_int, [C.c_void_p]),
    "rd_rec_backbone_forward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "rd_rec_backbone_forward_lines": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "rd_rec_tail_forward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                      C.c_void_p, C.c_size_t, C.c_void_p]),
    "rd_rec_seq_len": (C.c_int, [C.c_int]),
    "rd_backbone_forward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_void_p), C.c_void_p, C.c_size_t, C.c_void_p]),
    "rd_formula_encoder_forward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "rd_formula_decode": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.POINTER(C.c_int32), C.c_void_p]),
    "rd_formula_decode_stream": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "rd_formula_max_new_tokens": (C.c_int, [C.c_void_p]),
    "rd_preproc_resize_norm": (C.c_int, [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_float, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "rd_preproc_resize_norm_batch": (C.c_int, [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_float, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "rd_preproc_resize_norm_sources": (C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_float, C.c_int, C.c_int, C.c_void_p, C.c_int64, C.c_void_p]),
    "rd_preproc_resize_aa_norm": (C.c_int, [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "rd_formula_margin_boxes": (C.c_int, [C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "rd_formula_preproc_plan": (C.c_int, [C.c_int, C.c_int, C.c_void_p]),
    "rd_formula_preproc_batch": (C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "rd_crop_resize_norm_batch": (C.c_int, [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_float, C.c_int, C.c_void_p, C.c_void_p]),
    "rd_line_crops_batch": (C.c_int, [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int64, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "rd_line_warp_batch": (C.c_int, [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int64, C.c_void_p, C.c_void_p]),
    "rd_line_warp_sources": (C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int64, C.c_void_p]),
    "rd_line_resize_norm_batch": (C.c_int, [C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "rd_cls_forward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "rd_table_encoder_forward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "rd_table_decode": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "rd_table_decode_stream": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "rd_line_flip180_batch": (C.c_int, [C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p]),
    "rd_ctc_collapse": (C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p]),
    "rd_ctc_collapse_lines": (C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                                        C.c_void_p]),
    "rd_db_postprocess": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_float, C.c_float, C.c_float, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int]),
    "rd_db_boxes_workspace": (C.c_size_t, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
    "rd_db_boxes_device": (C.c_int, [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_float, C.c_float, C.c_float, C.c_int, C.c_int,
                                     C.c_int, C.c_void_p, C.c_size_t, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "rd_rec_chunk_cost": (C.c_double, [C.c_int, C.c_int, C.c_int]),
    "rd_rec_plan_chunks": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p]),
    "rd_rec_plan_lines": (C.c_int, [C.c_void_p, C.c_void_p] + [C.c_int] * 9 + [C.c_void_p] * 4 + [C.c_int, C.c_void_p]),
    "rd_text_boxes_order_merge": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "rd_ctc_rows_text": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "rd_layout_postprocess": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "rd_layout_postprocess_select": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "rd_find_external_contours": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "rd_find_external_contours_none": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "rd_checkbox_workspace": (C.c_size_t, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "rd_checkbox_detect_device": (C.c_int, [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p,
                                            C.c_void_p, C.c_void_p]),
    "rd_checkbox_finish": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p]),
    "rd_region_canvases_workspace": (C.c_size_t, [C.c_int, C.c_int, C.c_int]),
    "rd_region_canvases": (C.c_int, [C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t,
                                     C.c_void_p]),
    "rd_stage_pack": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int64, C.c_int]),
    "rd_stage_canvases": (C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "rd_contour_area": (C.c_double, [C.c_void_p, C.c_int]),
    "rd_arc_length": (C.c_double, [C.c_void_p, C.c_int, C.c_int]),
    "rd_approx_poly_dp": (C.c_int, [C.c_void_p, C.c_int, C.c_double, C.c_int, C.c_void_p, C.c_void_p]),
    "rd_min_area_rect_points": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p]),
    "rd_polygon_area": (C.c_double, [C.c_void_p, C.c_int]),
    "rd_polygon_intersection_area": (C.c_double, [C.c_void_p, C.c_int, C.c_void_p, C.c_int]),
    "rd_fill_poly": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int]),
    "rd_msdeform_attn": (C.c_int, [C.c_int] + [C.c_void_p] * 6 + [C.c_int] * 7 + [C.c_void_p]),
    "rd_topk_rows": (C.c_int, [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "rd_encoder_layer_workspace": (C.c_size_t, [C.c_int, C.c_int, C.c_int]),
    "rd_encoder_layer": (C.c_int, [C.c_int, C.c_void_p, C.c_void_p] + [C.c_int] * 6 + [C.c_void_p] * 12 + [C.c_float, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "rd_set_precision": (C.c_int, [C.c_void_p, C.c_char_p]),
    "rd_range_status": (C.c_int, [C.c_void_p, C.c_void_p]),
    "rd_plan_stats": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "rd_set_profiling": (C.c_int, [C.c_void_p, C.c_int]),
    "rd_profile_json": (C.c_char_p, [C.c_void_p]),
}

# The developer entries (csrc/api_debug.cpp; not in the public header), one row per exported rd_debug_* in the order of that file.
# tests/test_cabi.py holds both tables to the C prototypes.
_I, _P, _F = C.c_int, C.c_void_p, C.c_float
DEBUG_SYMBOLS = {
    "rd_debug_det_forward_stages": (_I, [_P, _P, _I, _I, _I, _P, _P, _P]),
    "rd_debug_cls_forward_stages": (_I, [_P, _P, _I, _I, _I, _P, _P, _P, _P]),
    "rd_debug_table_decode": (_I, [_P, _P, _I, _I, _I, _P] + [_P] * 7),
    "rd_debug_table_decode_stream": (_I, [_P, _P, _I, _I, _I, _I, _P, _P, _P, _P, _P, _P, _P, _P, _I]),
    "rd_debug_table_encoder_taps": (_I, [_P, _P, _I, _I, _I, _P, _P, _P]),
    "rd_debug_formula_decode": (_I, [_P, _P, _I, _I, _I, _P, C.POINTER(C.c_int32), _P, _P, _P]),
    "rd_debug_formula_decode_stream": (_I, [_P, _P, _I, _I, _I, _I, _P, _P, _P, _P, _P, _P, _P, _I]),
    "rd_debug_resize_aa_coeffs": (_I, [_I, _I, _P, _P, C.c_int64]),
    "rd_debug_resample_coeffs": (_I, [_I, _I, C.c_double, C.c_double, _I, _P, _P, C.c_int64]),
    "rd_debug_region_keep_mask": (_I, [_I, _I, _P, _I, _P]),
    "rd_debug_time_mixer": (_F, [_I] * 4 + [_P] * 6),
    "rd_debug_time_gemm": (_F, [_I] * 5 + [_P] * 6),
    "rd_debug_gemm_h1": (_F, [_I] * 5 + [_P, _I, _P, _P, _P, _I, _P, _I, _P]),
    "rd_debug_seqconv": (_F, [_I] * 8 + [_P, _I, _P, _I, _P, _P, _P, _P, _I, _P]),
    "rd_debug_det_local": (_F, [_I] * 5 + [_P] * 5 + [_F, _P, C.POINTER(C.c_int)]),
    "rd_debug_conv_route": (_I, [_I] * 17 + [_P, _I]),
    "rd_debug_conv_ex": (_F, [_I] * 22 + [_P] * 10 + [C.c_char_p, _P, _I, _P]),
    "rd_debug_conv3x3_wide": (_F, [_I] * 10 + [_P] * 5 + [_I, _P]),
    "rd_debug_conv": (_F, [_I] * 14 + [_P] * 8),
    "rd_debug_stem34": (_F, [_I] * 11 + [_P] * 7),
    "rd_debug_stem_front": (_F, [_I] * 8 + [_P] * 10),
    "rd_debug_dwconv_ex": (_F, [_I] * 17 + [_P] * 10 + [_I]),
    "rd_debug_dwconv": (_F, [_I] * 8 + [_P] * 8),
    "rd_debug_dw_route": (_I, [_I] * 9 + [_P, _I, _P]),
    "rd_debug_weight_split": (_I, [_P, _I, _I, _P, _P]),
    "rd_debug_lcv3_dw": (_F, [_I] * 9 + [_P] * 8),
    "rd_debug_dw5_strip": (_F, [_I] * 11 + [_P] * 7),
    "rd_debug_mv1e_pool": (_I, [_I] * 4 + [_P] * 3),
    "rd_debug_derived_tensor": (C.c_long, [C.c_char_p, C.c_char_p, C.c_size_t, C.c_char_p, _P, C.c_long]),
    "rd_debug_mbv3_dw": (_F, [_I] * 12 + [_P] * 4),
    "rd_debug_mbv3_block": (_F, [_I] * 14 + [_P] * 8),
    "rd_debug_mbv3_block_ok": (_I, [_I] * 12),
    "rd_debug_mbv3s_dw": (_F, [_I] * 13 + [_P] * 4),
    "rd_debug_mbv3s_block": (_F, [_I] * 15 + [_P] * 12),
    "rd_debug_lcv3_dw_det": (_F, [_I] * 10 + [_P] * 5),
    "rd_debug_lcv3_block": (_F, [_I] * 9 + [_P] * 9),
    "rd_debug_time_ctc": (_F, [_I] * 4 + [_P] * 7 + [_I, _P]),
    "rd_debug_time_checkbox_mask": (_F, [_I] * 4 + [_P, _P]),
    "rd_debug_attention": (_I, [_I] * 4 + [_F, _P, _P, _P, _I, _P]),
    "rd_debug_vit_attention": (_I, [_I] * 4 + [_F, _P, _P]),
    "rd_debug_attention_limits": (_I, [_I, _P, _P]),
    "rd_debug_layernorm": (_I, [_I, _I, _P, _I, _P, _I, _P, _P, _F]),
    "rd_debug_se_chain": (_I, [_I] * 7 + [_F] + [_I] * 3 + [_P] * 9),
    "rd_debug_ese": (_I, [_I] * 7 + [_P] * 8),
    "rd_debug_maxpool3x3s2": (_I, [_I] * 6 + [_P] * 2),
    "rd_debug_maxpool2x2s1": (_I, [_I] * 6 + [_P] * 2),
    "rd_debug_avgpool3x2": (_I, [_I] * 6 + [_P] * 3),
    "rd_debug_mask_cols": (_I, [_I] * 5 + [_P, _P, _I]),
    "rd_debug_upsample": (_I, [_I] * 8 + [_P] * 2),
    "rd_debug_add": (_I, [_I] * 5 + [_P] * 3),
    "rd_debug_det_head_tail": (_I, [_I] * 4 + [_P] * 6),
    "rd_debug_ctc_head": (_I, [_I] * 3 + [_P, _I] + [_P] * 6 + [_I, _P, _P]),
    "rd_debug_dec_gemv": (_I, [_I] * 4 + [_P] * 7),
    "rd_debug_dec_attention": (_I, [_I] * 4 + [_P, _P, _I, C.c_longlong] + [_P] * 5 + [_P, _I, _P, _P, _I, _P, _I]),
    "rd_debug_dec_select": (_I, [_I, _P, _I, _I, _I, _P, _I, _P, _I, _I] + [_P] * 6),
    "rd_debug_td_gemv": (_I, [_I] * 4 + [_P] * 5),
    "rd_debug_td_attention": (_I, [_I] * 4 + [_P, _P, _I, C.c_longlong, _P, _I, _P, _P, _I, _P, _I, _P, _P]),
    "rd_debug_td_select": (_I, [_I, _P, _I, _P, _I, _P, _I, _P, _P, _P, _I, _P, _P, _P, _P, _I] + [_P] * 6),
}


class NativeLibraryError(RuntimeError):
    pass


def load():
    """Load the HIP library (once).  Raises NativeLibraryError if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not LIB_PATH.exists():
        raise NativeLibraryError(
            f"{LIB_PATH} is missing - build it with `python -m rapiddoc_amd.build` (hipcc, gfx950). "
            "rapiddoc_amd has no CPU fallback.")
    # PyTorch-ROCm bundles its own HIP runtime; it must be in the process BEFORE this library is opened so that
    # both resolve to ONE libamdhip64 (shared streams / device memory).  Opening ours first would pull in
    # /opt/rocm's copy and leave the process with two runtimes.
    import torch  # noqa: F401
    lib = C.CDLL(str(LIB_PATH))
    for name, (res, args) in {**SYMBOLS, **DEBUG_SYMBOLS}.items():
        fn = getattr(lib, name)  # AttributeError = a symbol of include/rapiddoc_mi355.h or a developer entry is not exported
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib
