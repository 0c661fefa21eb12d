"""EuroBERT text encoders on the gfx950 kernels.

Replaces the forward of HuggingFace ``EuroBertModel`` (hf:modeling_eurobert.py: the Llama decoder layer with ``is_causal =
False`` and ``create_bidirectional_mask``; EuroBERT-210m / -610m / -2.1B), while keeping the HF module as the *parameter
container*: its module names are ``LlamaModel``'s, so state-dict keys stay ``plm_encoder.layers.N.self_attn.q_proj.weight`` etc.

The layer is the Llama layer of llama.py (add + RMSNorm, fused Q|K|V GEMM with its bias under ``attention_bias``, rotary
embedding in place, attention, O GEMM, add + RMSNorm, fused gate|up GEMM, SwiGLU, down GEMM) with the attention swapped: a query
sees every key of its own sequence.  Which kernels run it:

* one KV head per query head at head dim 64 (EuroBERT-210m): ``ops.rope_attention`` / ``_varlen``, the rotary kernel of the
  ModernBERT encoder followed by the bidirectional attention family of the BERT encoder (K5 / K7), as nomic_bert.py does;
* grouped KV heads, or head dim 128: ``ops.rope_bidir_gqa`` / ``_varlen``, the rotary kernel of llama.py followed by the
  bidirectional grouped-KV kernels (attn_bidir.hip, include/gmlm_hip_bidir.h).

Weights, rotary table (rope types default, linear and llama3) and head dim are llama.py's.  Two layouts: padded
(``eurobert_encode``) and packed / varlen (``eurobert_encode_packed``; with ``groups`` the grouped route at head dim 64 takes the
short-sequence kernels of attn_gqa_short.hip).  There is no hipGraph, bucketed or ring form of this encoder (DESIGN.md section 4 "EuroBERT and NomicBERT encoders").
"""
from __future__ import annotations

import torch

from . import encoder, llama, ops
from .dense import _mm
from .llama import head_dim, prepare_weights, rope_table  # noqa: F401  (a EuroBERT layer's weights and table are a Llama layer's)

MODEL_TYPES = ("eurobert",)


def check_supported(plm) -> None:
    llama.check_config(plm.config, MODEL_TYPES, "EuroBERT", "grouped")


def _layer(lw, stream, branch, lens, cs, hq, hkv, d, scale, eps, packed=None):
    """``llama._layer`` with bidirectional attention; ``packed`` = (pos_ids, cu_seqlens, max_len[, groups]); ``groups`` reaches
    the grouped route only."""
    s1, y1 = ops.add_rmsnorm(stream, branch, lw.ln1, eps)
    qkv = _mm(y1, lw.wqkv, lw.bqkv, lw.m_qkv)
    if hq == hkv and d == 64:
        ctx = ops.rope_attention_varlen(qkv, cs, *packed[:3], hq, scale) if packed is not None else \
            ops.rope_attention(qkv, cs, lens, hq, scale)
    elif packed is not None:
        ctx = ops.rope_bidir_gqa_varlen(qkv, cs, *packed[:3], hq, hkv, d, scale, groups=packed[3] if len(packed) > 3 else None)
    else:
        ctx = ops.rope_bidir_gqa(qkv, cs, lens, hq, hkv, d, scale)
    s2, y2 = ops.add_rmsnorm(s1, _mm(ctx, lw.wo, lw.bo, lw.m_wo), lw.ln2, eps)
    m = ops.swiglu(_mm(y2, lw.wgu, None, lw.m_gu))
    return s2, _mm(m, lw.wdown, None, lw.m_down)


def eurobert_encode(plm, input_ids: torch.Tensor, lens: torch.Tensor, cd: torch.dtype, training: bool = False,
                    gradient_checkpointing: bool = False, weights=None) -> torch.Tensor:
    """input_ids int [B, L] (left-aligned: padding anywhere past ``lens[b]`` is ignored), lens int32 [B] -> [B, L, P] in ``cd``.

    Positions are 0..L-1 per row; a query sees the keys below ``lens[b]``.  Rows at or past ``lens[b]`` are computed but never
    read by the pooling.  ``weights``: optional ``prepare_weights(plm, cd)`` result."""
    b, l = input_ids.shape
    encoder.check_length(plm.config, l)
    x = torch.nn.functional.embedding(input_ids.long(), plm.embed_tokens.weight).to(cd)   # bit-exact row gather
    return llama._encode_rows(plm, x, lens, rope_table(plm, l, x.device), cd, training, gradient_checkpointing, weights, layer=_layer)


def eurobert_encode_packed(plm, tok: torch.Tensor, pos: torch.Tensor, cu_seqlens: torch.Tensor, max_len: int, cd: torch.dtype,
                           training: bool = False, gradient_checkpointing: bool = False, weights=None, groups=None) -> torch.Tensor:
    """Packed (varlen) pass: tok / pos int [T] (token id and position of every row, the sequences back to back), cu_seqlens
    int32 [S + 1] (sequence i = rows [cu[i], cu[i+1]), covering all T rows), max_len >= the longest sequence -> [T, P] in ``cd``.
    ``groups``: optional ``ops.pack_sequence_groups`` of the sequence lengths; with grouped KV heads at head dim 64, bf16,
    max_len <= 128 and >= 512 (sequence, query head) pairs the attention runs on the short-sequence kernels."""
    max_len = int(max_len)
    encoder.check_length(plm.config, max_len)
    encoder.check_packed(tok, pos)
    x = torch.nn.functional.embedding(tok.long(), plm.embed_tokens.weight).to(cd)   # bit-exact row gather
    cs = rope_table(plm, max_len, x.device)
    return llama._encode_rows(plm, x, None, cs, cd, training, gradient_checkpointing, weights,
                              (pos.to(torch.int32), cu_seqlens, max_len, groups), layer=_layer)
