"""NomicBERT text encoder forward on the gfx950 kernels.

Replaces the forward of HuggingFace ``NomicBertModel`` (hf:modeling_nomic_bert.py: NomicBertEmbeddings, NomicBertAttention,
NomicBertMLP, NomicBertLayer; nomic-embed-text-v1 / v1.5), while keeping the HF module as the *parameter container*: state-dict
keys stay ``plm_encoder.layers.N.self_attn.q_proj.weight``, ``plm_encoder.embeddings.LayerNorm.weight`` etc.

A NomicBERT layer has the BERT geometry (post-LayerNorm, 12 heads x 64) with a rotary embedding instead of a position table, a
SwiGLU MLP and no projection biases:

    x = LayerNorm(word[ids] + token_type[0])
    per layer:  fused Q|K|V GEMM -> rotary embedding in place + bidirectional attention (``ops.rope_attention``: the rotary
                kernel of the ModernBERT encoder, then K5 / K7) -> O GEMM -> K6 dropout + residual + LayerNorm
                -> fused gate|up GEMM -> SwiGLU -> down GEMM -> K6

There are no kernels of its own.  The rotary table is built from the model's own ``rotary_emb`` (``llama.rope_table``: its
``inv_freq`` and ``attention_scaling``; the default theta of this family is 1000).  Two layouts: padded (``nomic_bert_encode``)
and packed / varlen (``nomic_bert_encode_packed``).  The pooler and the MLM head are not run.  There is no hipGraph, bucketed,
short-sequence-group or ring form of this encoder (DESIGN.md section 4 "EuroBERT and NomicBERT encoders").
"""
from __future__ import annotations

import torch

from . import encoder, ops
from .dense import _mm, encoder_operands
from .llama import ROPE_TYPES, rope_table
from .qwen3 import _rope_type, head_dim

HEAD_DIM = 64


def check_supported(plm) -> None:
    """Every way in which ``plm`` is not a NomicBERT encoder that the kernels cover, at once."""
    cfg = plm.config
    problems = []
    if getattr(cfg, "model_type", None) != "nomic_bert":
        problems.append(f"model_type={getattr(cfg, 'model_type', None)!r} (this module takes NomicBERT encoders)")
    if not getattr(cfg, "num_attention_heads", 0) or head_dim(cfg) != HEAD_DIM:
        problems.append(f"head_dim={head_dim(cfg) if getattr(cfg, 'num_attention_heads', 0) else None} (the rotary attention path takes {HEAD_DIM})")
    if getattr(cfg, "hidden_act", "silu") != "silu":
        problems.append(f"hidden_act={cfg.hidden_act!r}")
    if float(getattr(cfg, "attention_probs_dropout_prob", 0.0) or 0.0) != 0.0:
        problems.append(f"attention_probs_dropout_prob={cfg.attention_probs_dropout_prob} (no probability dropout behind the rotary embedding)")
    if _rope_type(cfg) not in ROPE_TYPES:
        problems.append(f"rope type {_rope_type(cfg)!r} (default, linear and llama3 only: the table must not depend on the length)")
    if problems:
        raise NotImplementedError("gmlm_amd text-encoder kernels do not cover this PLM: " + "; ".join(problems))


class LayerWeights:
    """Per-forward view of one layer: the GEMM operands in the compute dtype (fused ``wqkv`` [q|k|v], ``wo``, fused ``wgu``
    [gate|up], ``wdown``; no autograd history, no biases) next to the fp32 masters their gradients go to, and the two
    LayerNorms."""
    __slots__ = ("wqkv", "wo", "wgu", "wdown", "m_qkv", "m_wo", "m_gu", "m_down", "ln1", "ln2")


def prepare_weights(plm, cd, gemm_precision="native"):
    """One flat buffer in the compute dtype for all layers' GEMM weights, filled by ONE multi-tensor copy (Q/K/V rows land
    directly in the fused [3P, P] operand, gate / up rows in the fused [2 I, P] one).  ``gemm_precision`` "bf16x3" (fp32 only):
    the four operands become ``dense.SplitWeight`` objects."""
    out, specs = [], []
    for i, layer in enumerate(plm.layers):
        sa, mlp = layer.self_attn, layer.mlp
        wq, wgu = [sa.q_proj.weight, sa.k_proj.weight, sa.v_proj.weight], [mlp.gate_proj.weight, mlp.up_proj.weight]
        specs += [((i, "wqkv"), wq, 0), ((i, "wo"), [sa.o_proj.weight], 0), ((i, "wgu"), wgu, 0), ((i, "wdown"), [mlp.down_proj.weight], 0)]
        lw = LayerWeights()
        lw.m_qkv, lw.m_wo, lw.m_gu, lw.m_down = tuple(wq), (sa.o_proj.weight,), tuple(wgu), (mlp.down_proj.weight,)
        lw.ln1, lw.ln2 = layer.post_attention_layernorm, layer.post_mlp_layernorm
        out.append(lw)
    operands = encoder_operands(specs, cd, gemm_precision)
    for i, lw in enumerate(out):
        lw.wqkv, lw.wo, lw.wgu, lw.wdown = (operands[(i, k)] for k in ("wqkv", "wo", "wgu", "wdown"))
    return out


def _layer(lw, h, lens, cs, heads, scale, training, p_hidden, eps, packed=None):
    """``packed`` = (pos_ids, cu_seqlens, max_len): the rows are [T, .] packed sequences."""
    qkv, h_res = _mm(h, lw.wqkv, None, lw.m_qkv, residual=True)
    if packed is not None:
        ctx = ops.rope_attention_varlen(qkv, cs, *packed, heads, scale)
    else:
        ctx = ops.rope_attention(qkv, cs, lens, heads, scale)
    a = ops.bias_res_layernorm(_mm(ctx, lw.wo, None, lw.m_wo), None, h_res, lw.ln1.weight, lw.ln1.bias, eps, False, p_hidden, training)
    gu, a_res = _mm(a, lw.wgu, None, lw.m_gu, residual=True)
    m = ops.swiglu(gu)
    return ops.bias_res_layernorm(_mm(m, lw.wdown, None, lw.m_down), None, a_res, lw.ln2.weight, lw.ln2.bias, eps, False, p_hidden, training)


def _encode_rows(plm, x, lens, cs, cd, training, gradient_checkpointing, weights, *packed):
    """Embedding LayerNorm + dropout and the layers over the embedding rows ``x`` in ``cd`` ([B, L, P] with ``lens``, or [T, P]
    with ``packed`` = the one trailing argument of ``_layer``)."""
    cfg = plm.config
    emb = plm.embeddings
    eps, p_hidden = cfg.layer_norm_eps, cfg.hidden_dropout_prob
    h = ops.bias_res_layernorm(x, None, None, emb.LayerNorm.weight, emb.LayerNorm.bias, eps, False, p_hidden, training)
    if weights is None:
        weights = prepare_weights(plm, cd)
    args = (lens, cs, cfg.num_attention_heads, HEAD_DIM ** -0.5, training, p_hidden, eps, *packed)
    return encoder.run_layers(_layer, weights, h, args, training, gradient_checkpointing)


def _embed(plm, ids, cd):
    emb = plm.embeddings
    x = torch.nn.functional.embedding(ids.long(), emb.word_embeddings.weight)      # bit-exact row gather
    return (x + emb.token_type_embeddings.weight[0]).to(cd)


def nomic_bert_encode(plm, input_ids: torch.Tensor, lens: torch.Tensor, cd: torch.dtype, training: bool = False,
                      gradient_checkpointing: bool = False, weights=None) -> torch.Tensor:
    """input_ids int [B, L] (left-aligned: padding anywhere past ``lens[b]`` is ignored), lens int32 [B] -> [B, L, P] in ``cd``.

    Positions are 0..L-1 per row; padded key positions get probability 0 in every layer; rows at or past ``lens[b]`` are
    computed but never read by the pooling.  ``weights``: optional ``prepare_weights`` result shared across micro-batches."""
    b, l = input_ids.shape
    encoder.check_length(plm.config, l)
    x = _embed(plm, input_ids, cd)
    return _encode_rows(plm, x, lens, rope_table(plm, l, x.device), cd, training, gradient_checkpointing, weights)


def nomic_bert_encode_packed(plm, tok: torch.Tensor, pos: torch.Tensor, cu_seqlens: torch.Tensor, max_len: int, cd: torch.dtype,
                             training: bool = False, gradient_checkpointing: bool = False, weights=None) -> torch.Tensor:
    """Packed (varlen) pass: tok / pos int [T] (token id and position of every row, the sequences back to back), cu_seqlens
    int32 [S + 1] (sequence i = rows [cu[i], cu[i+1]), covering all T rows), max_len >= the longest sequence -> [T, P] in ``cd``."""
    max_len = int(max_len)
    encoder.check_length(plm.config, max_len)
    encoder.check_packed(tok, pos)
    x = _embed(plm, tok, cd)
    cs = rope_table(plm, max_len, x.device)
    return _encode_rows(plm, x, None, cs, cd, training, gradient_checkpointing, weights, (pos.to(torch.int32), cu_seqlens, max_len))
