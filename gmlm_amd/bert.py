"""BERT-geometry text encoder forward on the gfx950 kernels.

Replaces the forward of HuggingFace ``BertModel`` as the reference runs it (main.py:349; classes at
hf:modeling_bert.py:53-108 embeddings, 139-203 self-attention, 282-293 / 325-351 dense epilogues,
354-416 layer) while keeping the HF module as the *parameter container*, so state-dict keys
(``plm_encoder.*``), ``config.hidden_size`` and ``base_model_prefix`` stay what callers expect
(main.py:222, 328, 380, 409).

Per layer:  fused QKV GEMM (hipBLASLt) -> K5 masked attention (MFMA, per-sequence key length)
            -> out-proj GEMM -> K6 bias+dropout+residual+LayerNorm
            -> FFN-in GEMM -> bias+GELU(+dropout) kernel -> FFN-out GEMM -> K6.
Also registers the attention core under HF's AttentionInterface as ``"gmlm_hip"`` so an unmodified
HF BertModel can call K5 through ``config._attn_implementation``.
"""
from __future__ import annotations

from typing import Optional

import torch

from . import encoder, ops
from .dense import _mm, _splitk_wgrad  # noqa: F401  (_splitk_wgrad: tests/test_gpu_model.py imports it from here)
from .encoder import LayerWeights  # noqa: F401  (the post-LayerNorm layer's weights, shared with mpnet.py)
from .nn import attention_any_dim

# Head dims the encoder runs on attention kernels of their own, with the fused QKV buffer, the packed pass, the bucketed
# layout and the recorded encoder / whole step (32: attn_d32.hip; 64 / 96: attn_kernels.hip and its siblings).  Every gate
# reads this tuple at call time; any other head dim takes the padded pass through ``attention_any_dim`` (zero-padded heads).
# Set back to (64, 96), a d = 32 encoder takes that route again, bit for bit.
NATIVE_HEAD_DIMS = (32, 64, 96)


def check_supported(plm) -> None:
    cfg = plm.config
    problems = []
    if getattr(cfg, "model_type", None) != "bert":
        problems.append(f"model_type={getattr(cfg, 'model_type', None)!r} (only BERT-geometry encoders are on the kernel path)")
    if getattr(cfg, "position_embedding_type", "absolute") not in ("absolute", None):
        problems.append("non-absolute position embeddings")
    if getattr(cfg, "hidden_act", "gelu") != "gelu":
        problems.append(f"hidden_act={cfg.hidden_act!r}")
    if getattr(cfg, "is_decoder", False) or getattr(cfg, "add_cross_attention", False):
        problems.append("decoder / cross-attention BERT")
    if problems:
        raise NotImplementedError("gmlm_amd text-encoder kernels do not cover this PLM: " + "; ".join(problems))


def _layer_masters(layer):
    sa, so = layer.attention.self, layer.attention.output
    return [sa.query.weight, sa.key.weight, sa.value.weight], [sa.query.bias, sa.key.bias, sa.value.bias], so.dense, so.LayerNorm


def prepare_weights(plm, cd, gemm_precision="native"):
    """``encoder.prepare_weights`` over the BertLayers."""
    return encoder.prepare_weights(plm.encoder.layer, _layer_masters, cd, gemm_precision)


def _layer(lw, h, lens, heads, training, p_hidden, p_attn, eps, cu=None, max_len=0, pair_count=None, groups=None):
    pdim = h.shape[-1]
    d = pdim // heads
    scale = d ** -0.5
    if d in NATIVE_HEAD_DIMS:
        # the fused projection adds the Q|K|V biases; their GRADIENT (the column sums of dqkv) is returned by the attention
        # operator, which can form it inside its backward kernel (ops.AttentionQKV): an explicit autograd edge
        # bias master -> attention op, no side channel between the two backward functions
        qkv, h_res = _mm(h, lw.wqkv, lw.bqkv, lw.m_qkv[:3], residual=True, bias_grad=False)   # [B, L, 3P] or packed [T, 3P]
        ctx = ops.attention_qkv(qkv, None if cu is not None else lens, heads, scale, p_attn, training, cu, max_len, pair_count,
                                bias_masters=lw.m_qkv[3:], groups=groups)
    else:
        qkv, h_res = _mm(h, lw.wqkv, lw.bqkv, lw.m_qkv, residual=True)
        ctx = attention_any_dim(qkv[..., :pdim], qkv[..., pdim:2 * pdim], qkv[..., 2 * pdim:], lens, heads, scale, p_attn,
                                training)
    return encoder.post_ln_tail(lw, ctx, h_res, training, p_hidden, eps)


def bert_encode(plm, input_ids: torch.Tensor, lens: torch.Tensor, cd: torch.dtype, training: bool = False,
                gradient_checkpointing: bool = False, weights=None) -> torch.Tensor:
    """input_ids int [B, L] (padding anywhere past ``lens[b]`` is ignored), lens int32 [B] -> [B, L, P] in ``cd``.

    Token / position / type gathers are plain index gathers (bit-exact); padded key positions get
    probability 0 in every layer, padded query rows are computed but never read by the pooling.
    ``weights``: optional ``prepare_weights(plm, cd)`` result shared across micro-batches.
    """
    emb = plm.embeddings
    b, l = input_ids.shape
    x = torch.nn.functional.embedding(input_ids.long(), emb.word_embeddings.weight)   # bit-exact row gather
    x = x + (emb.token_type_embeddings.weight[0] + emb.position_embeddings.weight[:l]).unsqueeze(0)
    return _encode_rows(plm, x.to(cd), lens, cd, training, gradient_checkpointing, weights)


def _encode_rows(plm, x, lens, cd, training, gradient_checkpointing, weights, *packed):
    """Embedding LayerNorm and the layers over the embedding rows ``x`` in ``cd`` ([B, L, P] with ``lens``, or [T, P] with
    ``packed`` = the (cu_seqlens, max_len, pair_count, groups) of ``_layer``)."""
    cfg = plm.config
    emb = plm.embeddings
    eps, p_hidden, p_attn = cfg.layer_norm_eps, cfg.hidden_dropout_prob, cfg.attention_probs_dropout_prob
    h = ops.bias_res_layernorm(x, None, None, emb.LayerNorm.weight, emb.LayerNorm.bias, eps, False, p_hidden, training)
    heads = cfg.num_attention_heads
    if weights is None:
        weights = prepare_weights(plm, cd)
    args = (lens, heads, training, p_hidden, p_attn, eps, *packed)
    return encoder.run_layers(_layer, weights, h, args, training, gradient_checkpointing)


def bert_encode_packed(plm, token_ids: torch.Tensor, pos_ids: torch.Tensor, cu_seqlens: torch.Tensor, max_len: int,
                       cd: torch.dtype, training: bool = False, gradient_checkpointing: bool = False, weights=None,
                       pair_count=None, groups=None):
    """Variable-length (packed) encoder pass: ``token_ids`` int [T] = the valid tokens of all sequences back to
    back, ``pos_ids`` int [T] = position of each token inside its sequence, ``cu_seqlens`` int32 [B+1].
    Returns [T, P].  Every GEMM / LayerNorm / GELU row is a real token and attention never sees padding
    (same result per token as the padded form: padded keys have probability exactly 0 there).
    ``groups``: optional ``ops.pack_sequence_groups`` boundaries (device int32) for the short-sequence attention kernels."""
    cfg = plm.config
    emb = plm.embeddings
    heads = cfg.num_attention_heads
    if cfg.hidden_size // heads not in NATIVE_HEAD_DIMS:
        raise NotImplementedError("packed encoder pass needs head dim 32, 64 or 96 (use the padded path otherwise)")
    # word + type-0 + position rows in one pass (fp32 sums in torch's order, stored as cd); backward = segment sums by id
    x = ops.embed_sum(token_ids, pos_ids, emb.word_embeddings.weight, emb.position_embeddings.weight,
                      emb.token_type_embeddings.weight, cd)
    return _encode_rows(plm, x, None, cd, training, gradient_checkpointing, weights, cu_seqlens, max_len, pair_count, groups)


# ---------------------------------------------------------------------------------------------
# HF AttentionInterface registration (operator-level drop-in for K5)
# ---------------------------------------------------------------------------------------------
def gmlm_hip_attention_forward(module, query, key, value, attention_mask, dropout: float = 0.0,
                               scaling: Optional[float] = None, **kwargs):
    """Signature of transformers' attention functions (hf:modeling_bert.py:111-136,
    integrations/sdpa_attention.py:79).  query/key/value: [B, h, L, d].  ``attention_mask`` must be a
    key-padding mask (bool or additive [B,1,1|Lq,Lk]) whose valid keys form a prefix, which is what
    tokenizer right-padding produces; returns ([B, Lq, h, d], None)."""
    b, h, lq, d = query.shape
    lk = key.shape[2]
    if scaling is None:
        scaling = d ** -0.5
    kv_len = None
    if attention_mask is not None:
        m = attention_mask
        keep = m if m.dtype == torch.bool else (m > -1.0)
        keep = keep.reshape(b, -1, lk)[:, 0, :]
        kv_len = keep.sum(-1).to(torch.int32)
        # prefix check is cheap and guards against silently mis-handling arbitrary masks
        if not bool((keep == (torch.arange(lk, device=keep.device)[None] < kv_len[:, None])).all()):
            raise NotImplementedError("gmlm_hip attention supports right-padded key masks only")
    to_rows = lambda t: t.transpose(1, 2).reshape(b, t.shape[2], h * d).contiguous()
    q2, k2, v2 = to_rows(query), to_rows(key), to_rows(value)
    if q2.dtype not in (torch.float32, torch.bfloat16):
        q2, k2, v2 = q2.bfloat16(), k2.bfloat16(), v2.bfloat16()
    out = attention_any_dim(q2, k2, v2, kv_len, h, scaling, dropout, dropout > 0)
    return out.reshape(b, lq, h, d).to(query.dtype), None


def register_hf_attention(name: str = "gmlm_hip") -> str:
    from transformers import AttentionInterface
    AttentionInterface.register(name, gmlm_hip_attention_forward)
    try:  # same mask builder as sdpa (boolean / additive key-padding mask)
        from transformers.masking_utils import AttentionMaskInterface, sdpa_mask
        AttentionMaskInterface.register(name, sdpa_mask)
    except Exception:  # older/newer transformers without the mask registry: eager mask is used
        pass
    return name
