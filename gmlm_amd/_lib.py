"""ctypes binding of libgmlm_hip.so (C ABI: include/gmlm_hip.h, gmlm_hip_split.h, gmlm_hip_optim.h, gmlm_hip_d32.h,
gmlm_hip_wide.h, gmlm_hip_modernbert.h, gmlm_hip_relbias.h, gmlm_hip_disent.h, gmlm_hip_gqa.h, gmlm_hip_bidir.h, gmlm_hip_gqa_short.h, gmlm_hip_d32_short.h, gmlm_hip_gqa_wide.h, gmlm_hip_gqa_band.h and gmlm_hip_gqa_softcap.h): one signature table per header, positional argument types only.  Which attention entry point a head dim
takes, and where each ABI puts its arguments by name, is the family table of ops.py (``_ATTN_FAMILIES``).

The product path has NO fallback: if the shared library is missing or a call fails, a Python
exception is raised.  Build with ``python -c "import __graft_entry__ as g; g.build()"`` or
``make -C gmlm_amd/csrc``.
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libgmlm_hip.so")

F32, BF16 = 0, 1
_p, _i64, _i32, _f32, _u64, _sz = C.c_void_p, C.c_int64, C.c_int, C.c_float, C.c_uint64, C.c_size_t

# name -> (restype, argtypes); mirrors include/gmlm_hip.h line by line
SIGNATURES = {
    "gmlm_version": (C.c_int, []),
    "gmlm_last_error": (C.c_char_p, []),
    "gmlm_device_check": (C.c_int, [_p, _p, C.c_char_p, _i32]),
    "gmlm_degree_i32": (C.c_int, [_p, _i64, _i64, _p, _p]),
    "gmlm_degree_f32": (C.c_int, [_p, _i64, _i64, _p, _p]),
    "gmlm_edge_bucket": (C.c_int, [_p, _p, _i64, _i64, _p, _p]),
    "gmlm_relation_histogram": (C.c_int, [_p, _i64, _i32, _p, _p]),
    "gmlm_segment_sort_workspace_bytes": (_sz, [_i64]),
    "gmlm_segment_sort": (C.c_int, [_p, _p, _p, _i32, _i64, _i64, _p, _p, _p, _p, _p, _sz, _p]),
    "gmlm_gather_i64_to_i32": (C.c_int, [_p, _p, _i64, _p, _p]),
    "gmlm_gather_i32": (C.c_int, [_p, _p, _i64, _p, _p]),
    "gmlm_segment_inv_count": (C.c_int, [_p, _i64, _p, _p]),
    "gmlm_split_plan_capacity": (C.c_int, [_i64, _i64, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "gmlm_split_plan_build": (C.c_int, [_p, _i64, _i64, _i64, _p, _p, _p, _p]),
    "gmlm_rgcn_mean_spmm": (C.c_int, [_p, _i64, _i64, _p, _p, _p, _i32, _i64, _i64, _p, _i64, _i32, _i64, _p, _p, _p, _i64, _i64,
                                      _p, _p]),
    "gmlm_basis_compose_fwd": (C.c_int, [_p, _p, _i32, _i32, _i64, _p, _p]),
    "gmlm_basis_compose_bwd_workspace_bytes": (_sz, [_i32, _i32, _i64]),
    "gmlm_basis_compose_bwd": (C.c_int, [_p, _p, _p, _i32, _i32, _i64, _p, _p, _p, _sz, _p]),
    "gmlm_colstats_workspace_bytes": (_sz, [_i64, _i64]),
    "gmlm_colstats": (C.c_int, [_p, _i32, _p, _i64, _i64, _p, _p, _p, _sz, _p]),
    "gmlm_graphnorm_finalize": (C.c_int, [_p, _p, _p, _p, _i64, _i64, _f32, _p, _p, _p]),
    "gmlm_graphnorm_apply": (C.c_int, [_p, _p, _p, _p, _p, _p, _i64, _i64, _i32, _f32, _u64, _p, _p, _i32, _p]),
    "gmlm_graphnorm_bwd_stats": (C.c_int, [_p, _i32, _p, _p, _p, _p, _p, _p, _i64, _i64, _i32, _f32, _u64, _p, _p, _p, _sz, _p]),
    "gmlm_graphnorm_bwd_apply": (C.c_int, [_p, _i32, _p, _p, _p, _p, _p, _p, _p, _i64, _i64, _i64, _i32, _f32, _u64, _p,
                                           _p, _p, _p, _p, _p]),
    "gmlm_bias_res_layernorm_fwd": (C.c_int, [_p, _p, _p, _p, _p, _i64, _i64, _f32, _i32, _f32, _u64, _p, _p, _p, _p, _i32, _p]),
    "gmlm_layernorm_bwd_workspace_bytes": (_sz, [_i64, _i64]),
    "gmlm_bias_res_layernorm_bwd": (C.c_int, [_p, _p, _p, _p, _p, _p, _p, _p, _i64, _i64, _i32, _f32, _u64, _p, _p, _p, _p, _p,
                                              _p, _i32, _p, _sz, _p]),
    "gmlm_attention_fwd": (C.c_int, [_p, _p, _p, _p, _i64, _i64, _i64, _i64, _i64, _i64, _i64, _i64, _f32, _f32, _u64, _p,
                                     _p, _p, _p, _i32, _p, _i64, _p, _i64, _p]),
    "gmlm_attention_bwd_workspace_bytes": (_sz, [_i64, _i64, _i64, _i64, _i64]),
    "gmlm_attention_bwd": (C.c_int, [_p, _p, _p, _p, _p, _p, _p, _i64, _i64, _i64, _i64, _i64, _i64, _i64, _i64, _f32,
                                     _f32, _u64, _p, _p, _p, _p, _i64, _i64, _i64, _i32, _p, _i64, _p, _sz, _p, _p, _p, _p, _i64, _p]),
    "gmlm_attention_d128_fwd": (C.c_int, [_p, _p, _p, _p, _i64, _i64, _i64, _i64, _i64, _i64, _i64, _i64, _f32, _f32, _u64, _p,
                                          _p, _p, _p, _i32, _p]),
    "gmlm_attention_d128_workspace_bytes": (_sz, [_i64, _i64, _i64]),
    "gmlm_attention_d128_bwd": (C.c_int, [_p, _p, _p, _p, _p, _p, _p, _p, _i64, _i64, _i64, _i64, _i64, _i64, _i64, _i64, _f32,
                                          _f32, _u64, _p, _p, _p, _p, _i64, _i64, _i64, _i32, _p, _sz, _p]),
    "gmlm_attention_causal_d128_fwd": (C.c_int, [_p, _p, _p, _p, _i64, _i64, _i64, _i64, _i64, _i64, _i64, _i64, _i64, _f32, _f32,
                                                 _p, _p, _p, _i32, _p]),
    "gmlm_attention_causal_d128_workspace_bytes": (_sz, [_i64, _i64, _i64]),
    "gmlm_attention_causal_d128_bwd": (C.c_int, [_p, _p, _p, _p, _p, _p, _p, _p, _i64, _i64, _i64, _i64, _i64, _i64, _i64, _i64,
                                                 _i64, _f32, _f32, _p, _p, _p, _i64, _i64, _i64, _i32, _p, _sz, _p]),
    "gmlm_attention_causal_d128_varlen_fwd": (C.c_int, [_p, _p, _p, _p, _i64, _i64, _i64, _i64, _i64, _i64, _i64, _i64, _i64, _f32,
                                                        _f32, _p, _p, _p, _i32, _p]),
    "gmlm_attention_causal_d128_varlen_workspace_bytes": (_sz, [_i64, _i64]),
    "gmlm_attention_causal_d128_varlen_bwd": (C.c_int, [_p, _p, _p, _p, _p, _p, _p, _p, _i64, _i64, _i64, _i64, _i64, _i64, _i64,
                                                        _i64, _i64, _f32, _f32, _p, _p, _p, _i64, _i64, _i64, _i32, _p, _sz, _p]),
    "gmlm_add_rmsnorm_fwd": (C.c_int, [_p, _p, _p, _i64, _i64, _f32, _p, _p, _p, _i32, _p]),
    "gmlm_add_rmsnorm_bwd_workspace_bytes": (_sz, [_i64, _i64]),
    "gmlm_add_rmsnorm_bwd": (C.c_int, [_p, _p, _p, _p, _p, _i64, _i64, _p, _p, _i32, _p, _sz, _p]),
    "gmlm_qknorm_rope_fwd": (C.c_int, [_p, _i64, _p, _p, _p, _i64, _i64, _i64, _i64, _i64, _i64, _f32, _p, _i64, _p, _i32, _p]),
    "gmlm_qknorm_rope_bwd_workspace_bytes": (_sz, [_i64, _i64, _i64, _i32]),
    "gmlm_qknorm_rope_bwd": (C.c_int, [_p, _i64, _p, _i64, _p, _p, _p, _i64, _p, _i64, _i64, _i64, _i64, _i64, _p, _p, _i32, _p,
                                       _sz, _p]),
    "gmlm_qknorm_rope_pos_fwd": (C.c_int, [_p, _i64, _p, _p, _p, _i64, _i64, _p, _i64, _i64, _i64, _f32, _p, _i64, _p, _i32, _p]),
    "gmlm_qknorm_rope_pos_bwd": (C.c_int, [_p, _i64, _p, _i64, _p, _p, _p, _i64, _p, _i64, _p, _i64, _i64, _i64, _p, _p, _i32, _p,
                                           _sz, _p]),
    "gmlm_swiglu_fwd": (C.c_int, [_p, _i64, _i64, _p, _i32, _p]),
    "gmlm_swiglu_bwd": (C.c_int, [_p, _p, _i64, _i64, _p, _i32, _p]),
    "gmlm_embed_sum_fwd": (C.c_int, [_p, _p, _p, _p, _p, _i64, _i64, _i64, _i64, _p, _i32, _p, _p]),
    "gmlm_meanpool_scatter_fwd": (C.c_int, [_p, _p, _p, _i64, _i64, _i64, _p, _i32, _p, _p]),
    "gmlm_meanpool_scatter_bwd": (C.c_int, [_p, _p, _p, _i64, _i64, _i64, _p, _i32, _p, _p]),
    "gmlm_softmask_blend_fwd": (C.c_int, [_p, _p, _p, _f32, _i64, _i64, _p, _i64, _i32, _p]),
    "gmlm_softmask_blend_bwd_workspace_bytes": (_sz, [_i64, _i64]),
    "gmlm_softmask_blend_bwd": (C.c_int, [_p, _i64, _p, _f32, _i64, _i64, _p, _p, _sz, _p]),
    "gmlm_bias_gelu_fwd": (C.c_int, [_p, _p, _i64, _i64, _f32, _u64, _p, _p, _i32, _p]),
    "gmlm_bias_gelu_bwd_workspace_bytes": (_sz, [_i64, _i64, _i32]),
    "gmlm_bias_gelu_bwd": (C.c_int, [_p, _p, _p, _i64, _i64, _f32, _u64, _p, _p, _p, _i32, _p, _sz, _p]),
    "gmlm_wgrad_workspace_bytes": (_sz, [_i64, _i64, _i64, _i32]),
    "gmlm_wgrad_bf16": (C.c_int, [_p, _i64, _p, _i64, _i64, _i64, _i64, _i32, _p, _i64, _i32, _p, _sz, _p]),
}

# second header, include/gmlm_hip_split.h (the bf16x3 operand split); same conventions, bound next to the first table
SIGNATURES_SPLIT = {
    "gmlm_split_bf16x3": (C.c_int, [_p, _i64, _i64, _i64, _i64, _p, _i64, _i64, _i32, _p]),
}

# third header, include/gmlm_hip_optim.h (gradient clipping + AdamW as one multi-tensor step)
SIGNATURES_OPTIM = {
    "gmlm_adamw_chunk_elems": (_i64, []),
    "gmlm_adamw_sumsq": (C.c_int, [_p, _p, _p, _i64, _p, _p, _p]),
    "gmlm_adamw_finalize": (C.c_int, [_p, _p, _i64, _f32, _p, _p, _i64, _p, _i64, _p, _i64, _p, _p, _p]),
    "gmlm_adamw_update": (C.c_int, [_p, _p, _p, _p, _i64, _p, _i64, _p, _p, _p]),
}

# fourth header, include/gmlm_hip_d32.h (attention at head dim 32: padded and packed, 1-D grids)
SIGNATURES_D32 = {
    "gmlm_attention_d32_fwd": (C.c_int, [_p, _p, _p, _p, _i64, _i64, _i64, _i64, _i64, _i64, _i64, _i64, _f32, _f32, _u64, _p,
                                         _p, _p, _p, _i32, _p, _i64, _p]),
    "gmlm_attention_d32_bwd_workspace_bytes": (_sz, [_i64, _i64, _i64]),
    "gmlm_attention_d32_bwd": (C.c_int, [_p, _p, _p, _p, _p, _p, _p, _i64, _i64, _i64, _i64, _i64, _i64, _i64, _i64, _f32,
                                         _f32, _u64, _p, _p, _p, _p, _i64, _i64, _i64, _i32, _p, _i64, _p, _sz, _p, _p]),
}

# fifth header, include/gmlm_hip_wide.h (encoders wider than 1,024: attention at head dims 256 / 384 / 512, LayerNorm rows to 4,096)
SIGNATURES_WIDE = {
    "gmlm_attention_wide_fwd": (C.c_int, [_p, _p, _p, _p, _i64, _i64, _i64, _i64, _i64, _i64, _i64, _i64, _f32, _f32, _u64, _p,
                                          _p, _p, _p, _i32, _p]),
    "gmlm_attention_wide_bwd_workspace_bytes": (_sz, [_i64, _i64, _i64]),
    "gmlm_attention_wide_bwd": (C.c_int, [_p, _p, _p, _p, _p, _p, _p, _p, _i64, _i64, _i64, _i64, _i64, _i64, _i64, _i64, _f32,
                                          _f32, _u64, _p, _p, _p, _p, _i64, _i64, _i64, _i32, _p, _sz, _p]),
    "gmlm_bias_res_layernorm_wide_fwd": (C.c_int, [_p, _p, _p, _p, _p, _i64, _i64, _f32, _i32, _f32, _u64, _p, _p, _p, _p, _i32,
                                                   _p]),
    "gmlm_bias_res_layernorm_wide_bwd_workspace_bytes": (_sz, [_i64, _i64]),
    "gmlm_bias_res_layernorm_wide_bwd": (C.c_int, [_p, _p, _p, _p, _p, _p, _p, _p, _i64, _i64, _i32, _f32, _u64, _p, _p, _p, _p,
                                                   _p, _p, _i32, _p, _sz, _p]),
}

# sixth header, include/gmlm_hip_modernbert.h (ModernBERT encoder: add + LayerNorm, rotary embedding at d = 64, GeGLU, band-limited attention)
SIGNATURES_MODERNBERT = {
    "gmlm_add_layernorm_fwd": (C.c_int, [_p, _p, _p, _p, _i64, _i64, _f32, _p, _p, _p, _p, _i32, _p]),
    "gmlm_add_layernorm_bwd_workspace_bytes": (_sz, [_i64, _i64]),
    "gmlm_add_layernorm_bwd": (C.c_int, [_p, _p, _p, _p, _p, _p, _i64, _i64, _p, _p, _p, _i32, _p, _sz, _p]),
    "gmlm_rope64_fwd": (C.c_int, [_p, _i64, _p, _i64, _i64, _i64, _p, _i64, _i64, _i32, _p]),
    "gmlm_rope64_bwd": (C.c_int, [_p, _i64, _p, _i64, _i64, _i64, _p, _i64, _i64, _i32, _p]),
    "gmlm_geglu_fwd": (C.c_int, [_p, _i64, _i64, _p, _i32, _p]),
    "gmlm_geglu_bwd": (C.c_int, [_p, _p, _i64, _i64, _p, _i32, _p]),
    "gmlm_attention_window_fwd": (C.c_int, [_p, _p, _p, _p, _i64, _i64, _i64, _i64, _i64, _i64, _i64, _i64, _f32, _f32, _i64, _p,
                                            _p, _p, _i32, _p, _i64, _p]),
    "gmlm_attention_window_workspace_bytes": (_sz, [_i64, _i64, _i64]),
    "gmlm_attention_window_bwd": (C.c_int, [_p, _p, _p, _p, _p, _p, _p, _p, _i64, _i64, _i64, _i64, _i64, _i64, _i64, _i64, _f32,
                                            _f32, _i64, _p, _p, _p, _i64, _i64, _i64, _i32, _p, _i64, _p, _sz, _p]),
}

SIGNATURE_TABLES = (SIGNATURES, SIGNATURES_SPLIT, SIGNATURES_OPTIM, SIGNATURES_D32, SIGNATURES_WIDE,
                    SIGNATURES_MODERNBERT)   # one per header, all bound by lib()

# seventh header, include/gmlm_hip_relbias.h (self-attention with a learned relative-position bias at d = 64: MPNet encoders)
SIGNATURES_RELBIAS = {
    "gmlm_attention_relbias_fwd": (C.c_int, [_p, _p, _p, _p, _i64, _i64, _i64, _i64, _i64, _i64, _i64, _i64, _f32, _f32, _u64, _p,
                                             _p, _i64, _p, _p, _p, _i32, _p, _i64, _p]),
    "gmlm_attention_relbias_workspace_bytes": (_sz, [_i64, _i64, _i64, _i64, _i64]),
    "gmlm_attention_relbias_bwd": (C.c_int, [_p, _p, _p, _p, _p, _p, _p, _p, _i64, _i64, _i64, _i64, _i64, _i64, _i64, _i64, _f32,
                                             _f32, _u64, _p, _p, _i64, _p, _p, _p, _p, _i64, _i64, _i64, _i32, _p, _i64, _p, _sz,
                                             _p]),
}

# the headers added after the sixth: SIGNATURE_TABLES keeps the six that came with ABI version 1, lib() binds both tuples
# eighth header, include/gmlm_hip_disent.h (disentangled self-attention at d = 64: DeBERTa-v2 / v3 encoders)
SIGNATURES_DISENT = {
    "gmlm_attention_disent_fwd": (C.c_int, [_p, _p, _p, _p, _i64, _i64, _i64, _i64, _i64, _i64, _i64, _i64, _f32, _f32, _u64, _p,
                                            _p, _p, _p, _i64, _i64, _p, _p, _p, _i32, _p, _i64, _p]),
    "gmlm_attention_disent_workspace_bytes": (_sz, [_i64, _i64, _i64, _i64]),
    "gmlm_attention_disent_bwd": (C.c_int, [_p, _p, _p, _p, _p, _p, _p, _p, _i64, _i64, _i64, _i64, _i64, _i64, _i64, _i64, _f32,
                                            _f32, _u64, _p, _p, _p, _p, _i64, _i64, _p, _p, _p, _p, _p, _i64, _i64, _i64, _i32, _p,
                                            _i64, _p, _sz, _p]),
}

# ninth header, include/gmlm_hip_gqa.h (Llama / Qwen2 / Mistral encoders: rotary embedding over head rows at d = 64 / 128, causal
# GQA attention at d = 64); the attention six take the argument lists of their gmlm_attention_causal_d128_* namesakes
_D128 = "gmlm_attention_causal_d128"
SIGNATURES_GQA = {
    "gmlm_rope_heads_fwd": (C.c_int, [_p, _i64, _p, _i64, _i64, _i64, _p, _i64, _i64, _i32, _p]),
    "gmlm_rope_heads_bwd": (C.c_int, [_p, _i64, _p, _i64, _i64, _i64, _p, _i64, _i64, _i32, _p]),
    **{"gmlm_attention_causal_d64" + tail: SIGNATURES[_D128 + tail]
       for tail in ("_fwd", "_workspace_bytes", "_bwd", "_varlen_fwd", "_varlen_workspace_bytes", "_varlen_bwd")},
}

# tenth header, include/gmlm_hip_bidir.h (EuroBERT encoders: bidirectional GQA attention at d = 64 / 128); the argument lists of
# the gmlm_attention_causal_d64_* namesakes
SIGNATURES_BIDIR = {"gmlm_attention_bidir_gqa" + tail: SIGNATURES[_D128 + tail]
                    for tail in ("_fwd", "_workspace_bytes", "_bwd", "_varlen_fwd", "_varlen_workspace_bytes", "_varlen_bwd")}

# eleventh header, include/gmlm_hip_gqa_short.h (LDS-resident short-sequence form of the two grouped families at d = 64, packed
# layout with seq_groups; `causal` is an argument, there is no out_lo and no workspace)
SIGNATURES_GQA_SHORT = {
    "gmlm_attention_gqa_short_fwd": (C.c_int, [_p, _p, _p, _p, _i64, _i64, _i64, _i64, _i64, _i64, _i64, _i64, _i64, _f32, _f32, _i32,
                                               _p, _i64, _p, _p, _i32, _p]),
    "gmlm_attention_gqa_short_bwd": (C.c_int, [_p, _p, _p, _p, _p, _p, _i64, _i64, _i64, _i64, _i64, _i64, _i64, _i64, _i64, _f32,
                                               _f32, _i32, _p, _i64, _p, _p, _p, _i64, _i64, _i64, _i32, _p]),
}

# twelfth header, include/gmlm_hip_d32_short.h (LDS-resident short-sequence attention at head dim 32, packed layout with seq_groups:
# one h, dropout seed arguments, optional fused bias sums; no out_lo and no workspace)
SIGNATURES_D32_SHORT = {
    "gmlm_attention_d32_short_fwd": (C.c_int, [_p, _p, _p, _p, _i64, _i64, _i64, _i64, _i64, _i64, _i64, _i64, _f32, _f32, _u64, _p,
                                               _p, _i64, _p, _p, _i32, _p]),
    "gmlm_attention_d32_short_bwd": (C.c_int, [_p, _p, _p, _p, _p, _p, _i64, _i64, _i64, _i64, _i64, _i64, _i64, _i64, _f32, _f32,
                                               _u64, _p, _p, _i64, _p, _p, _p, _i64, _i64, _i64, _p, _p, _i32, _p]),
}

# thirteenth header, include/gmlm_hip_gqa_wide.h (Gemma3 text encoders: grouped-KV attention at head dim 256, causal or not, the
# sandwich RMSNorm pair, Q / K head norm + rotary embedding at head dim 256, tanh-GELU gated unit).  The attention entry points
# take the argument lists of their gmlm_attention_bidir_gqa_* namesakes with `causal` (int) after dropout_p, the rotary ones
# those of gmlm_qknorm_rope_* with `w_offset` (float) after d
_GQAW_FWD = (C.c_int, [_p, _p, _p, _p] + [_i64] * 9 + [_f32, _f32, _i32, _p, _p, _p, _i32, _p])
_GQAW_BWD = (C.c_int, [_p] * 8 + [_i64] * 9 + [_f32, _f32, _i32, _p, _p, _p, _i64, _i64, _i64, _i32, _p, _sz, _p])
SIGNATURES_GQA_WIDE = {
    "gmlm_attention_gqa_d256_fwd": _GQAW_FWD,
    "gmlm_attention_gqa_d256_bwd_workspace_bytes": (_sz, [_i64, _i64, _i64]),
    "gmlm_attention_gqa_d256_bwd": _GQAW_BWD,
    "gmlm_attention_gqa_d256_varlen_fwd": _GQAW_FWD,
    "gmlm_attention_gqa_d256_varlen_bwd_workspace_bytes": (_sz, [_i64, _i64]),
    "gmlm_attention_gqa_d256_varlen_bwd": _GQAW_BWD,
    "gmlm_sandwich_rmsnorm_fwd": (C.c_int, [_p, _p, _p, _p, _i64, _i64, _f32, _f32, _p, _p, _p, _p, _i32, _p]),
    "gmlm_sandwich_rmsnorm_bwd_workspace_bytes": (_sz, [_i64, _i64]),
    "gmlm_sandwich_rmsnorm_bwd": (C.c_int, [_p, _p, _p, _p, _p, _p, _p, _p, _i64, _i64, _f32, _p, _p, _p, _p, _i32, _p, _sz, _p]),
    "gmlm_qknorm_rope_d256_fwd": (C.c_int, [_p, _i64, _p, _p, _p, _i64, _i64, _i64, _i64, _i64, _i64, _f32, _f32, _p, _i64, _p, _i32, _p]),
    "gmlm_qknorm_rope_d256_pos_fwd": (C.c_int, [_p, _i64, _p, _p, _p, _i64, _i64, _p, _i64, _i64, _i64, _f32, _f32, _p, _i64, _p, _i32, _p]),
    "gmlm_qknorm_rope_d256_bwd_workspace_bytes": (_sz, [_i64, _i64, _i64, _i32]),
    "gmlm_qknorm_rope_d256_bwd": (C.c_int, [_p, _i64, _p, _i64, _p, _p, _p, _i64, _p, _i64, _i64, _i64, _i64, _i64, _f32, _p, _p, _i32, _p,
                                            _sz, _p]),
    "gmlm_qknorm_rope_d256_pos_bwd": (C.c_int, [_p, _i64, _p, _i64, _p, _p, _p, _i64, _p, _i64, _p, _i64, _i64, _i64, _f32, _p, _p, _i32, _p,
                                                _sz, _p]),
    "gmlm_geglu_tanh_fwd": (C.c_int, [_p, _i64, _i64, _p, _i32, _p]),
    "gmlm_geglu_tanh_bwd": (C.c_int, [_p, _p, _i64, _i64, _p, _i32, _p]),
}

# fourteenth header, include/gmlm_hip_gqa_band.h (band-limited form of the grouped-KV attention at head dim 256: the sliding layers
# of a Gemma3 encoder past the window).  The argument lists of the gmlm_attention_gqa_d256_* namesakes with `window` (int64_t) after
# `causal`; the workspace queries are the namesakes'
_GQAB_FWD = (C.c_int, [_p, _p, _p, _p] + [_i64] * 9 + [_f32, _f32, _i32, _i64, _p, _p, _p, _i32, _p])
_GQAB_BWD = (C.c_int, [_p] * 8 + [_i64] * 9 + [_f32, _f32, _i32, _i64, _p, _p, _p, _i64, _i64, _i64, _i32, _p, _sz, _p])
SIGNATURES_GQA_BAND = {
    "gmlm_attention_gqa_d256_band_fwd": _GQAB_FWD,
    "gmlm_attention_gqa_d256_band_bwd_workspace_bytes": (_sz, [_i64, _i64, _i64]),
    "gmlm_attention_gqa_d256_band_bwd": _GQAB_BWD,
    "gmlm_attention_gqa_d256_band_varlen_fwd": _GQAB_FWD,
    "gmlm_attention_gqa_d256_band_varlen_bwd_workspace_bytes": (_sz, [_i64, _i64]),
    "gmlm_attention_gqa_d256_band_varlen_bwd": _GQAB_BWD,
}

# fifteenth header, include/gmlm_hip_gqa_softcap.h (Gemma2 text encoders: the grouped-KV attention at head dim 256 with attention-logit
# soft-capping, with or without a band, and the rotary embedding on head rows at d = 256).  The argument lists of the
# gmlm_attention_gqa_d256_band_* namesakes with `softcap` (float) after `window` (0 = no band); the rotary pair takes the lists of
# gmlm_rope_heads_*
_GQAC_FWD = (C.c_int, [_p, _p, _p, _p] + [_i64] * 9 + [_f32, _f32, _i32, _i64, _f32, _p, _p, _p, _i32, _p])
_GQAC_BWD = (C.c_int, [_p] * 8 + [_i64] * 9 + [_f32, _f32, _i32, _i64, _f32, _p, _p, _p, _i64, _i64, _i64, _i32, _p, _sz, _p])
SIGNATURES_GQA_SOFTCAP = {
    "gmlm_attention_gqa_d256_softcap_fwd": _GQAC_FWD,
    "gmlm_attention_gqa_d256_softcap_bwd_workspace_bytes": (_sz, [_i64, _i64, _i64]),
    "gmlm_attention_gqa_d256_softcap_bwd": _GQAC_BWD,
    "gmlm_attention_gqa_d256_softcap_varlen_fwd": _GQAC_FWD,
    "gmlm_attention_gqa_d256_softcap_varlen_bwd_workspace_bytes": (_sz, [_i64, _i64]),
    "gmlm_attention_gqa_d256_softcap_varlen_bwd": _GQAC_BWD,
    "gmlm_rope_heads_d256_fwd": SIGNATURES_GQA["gmlm_rope_heads_fwd"],
    "gmlm_rope_heads_d256_bwd": SIGNATURES_GQA["gmlm_rope_heads_bwd"],
}

SIGNATURE_TABLES_LATER = (SIGNATURES_RELBIAS, SIGNATURES_GQA, SIGNATURES_BIDIR, SIGNATURES_GQA_SHORT, SIGNATURES_D32_SHORT,
                          SIGNATURES_GQA_WIDE, SIGNATURES_GQA_BAND, SIGNATURES_GQA_SOFTCAP, SIGNATURES_DISENT)


class GmlmHipError(RuntimeError):
    pass


_lib = None


def lib() -> C.CDLL:
    """Load libgmlm_hip.so once; raise loudly when it is not built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise GmlmHipError(
            f"{LIB_PATH} not found: the HIP extension is not built. Run `make -C gmlm_amd/csrc` "
            "(or __graft_entry__.build()). gmlm_amd has no CPU / eager fallback.")
    handle = C.CDLL(LIB_PATH)
    for table in SIGNATURE_TABLES + SIGNATURE_TABLES_LATER:
        for name, (res, args) in table.items():
            fn = getattr(handle, name)  # AttributeError here = header / library mismatch
            fn.restype, fn.argtypes = res, args
    if handle.gmlm_version() != 1:
        raise GmlmHipError(f"ABI version mismatch: library {handle.gmlm_version()} != binding 1")
    _lib = handle
    return handle


def check(rc: int, what: str = "") -> None:
    if rc != 0:
        msg = lib().gmlm_last_error().decode(errors="replace")
        raise GmlmHipError(f"{what or 'gmlm call'} failed (code {rc}): {msg}")


_device_ok = {}


def require_gfx950(device_index: int) -> None:
    """One-time check per device that we are on a gfx950 part."""
    if _device_ok.get(device_index):
        return
    import torch
    with torch.cuda.device(device_index):
        arch = C.create_string_buffer(64)
        cu, wave = C.c_int(0), C.c_int(0)
        check(lib().gmlm_device_check(C.byref(cu), C.byref(wave), arch, 64), "gmlm_device_check")
    _device_ok[device_index] = (cu.value, wave.value, arch.value.decode())


def device_info(device_index: int = 0):
    require_gfx950(device_index)
    return _device_ok[device_index]
