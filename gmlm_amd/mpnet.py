"""MPNet text encoder forward on the gfx950 kernels.

Replaces the forward of HuggingFace ``MPNetModel`` (hf:modeling_mpnet.py: MPNetEmbeddings, MPNetSelfAttention, MPNetAttention,
MPNetLayer, MPNetEncoder) as the reference would run ``sentence-transformers/all-mpnet-base-v2`` and its siblings
(main.py:213, 349), while keeping the HF module as the *parameter container*: state-dict keys stay
``plm_encoder.encoder.layer.N.attention.attn.q.weight``, ``plm_encoder.encoder.relative_attention_bias.weight`` etc.

An MPNet layer is a BERT layer (post-LayerNorm, biased Q / K / V / O, erf-GELU FFN) whose attention scores get one learned
term, the same in every layer:

    s_ij = q_i . k_j / sqrt(d) + B[h, bucket(j - i)],    B = encoder.relative_attention_bias.weight  (32 buckets x heads)

    x = LayerNorm(word[ids] + position[padding_idx + 1 + i])            (no token-type table)
    per layer:  fused QKV GEMM -> attention with the bias table (attn_relbias.hip, head dim 64) -> O GEMM
                -> K6 bias + dropout + residual + LayerNorm -> FFN-in GEMM -> bias + GELU -> FFN-out GEMM -> K6

The bias reaches the kernels as ONE fp32 table [h, 2M - 1] per forward, ``weight[bucket(rel)]`` for rel = -(M - 1) .. M - 1 with
M = the longest sequence of the call, bucketed by ``MPNetEncoder.relative_position_bucket`` itself; its gradient is folded back
onto the 32 x h parameter by fixed-order segment sums (``fold_bias_grad``).  Two layouts: padded ([B, L, .] with ``lens``,
``mpnet_encode``) and packed ([T, .] rows with ``cu_seqlens``, ``mpnet_encode_packed``).  There is no hipGraph, bucketed or ring
form of this encoder (DESIGN.md section 4 "MPNet encoder").
"""
from __future__ import annotations

import torch

from . import encoder, ops
from .dense import _mm
from .encoder import LayerWeights  # noqa: F401  (an MPNet layer's weights are a BERT layer's)

HEAD_DIM = 64
NUM_BUCKETS = 32      # hf: compute_position_bias always buckets with 32, whatever relative_attention_num_buckets says


def check_supported(plm) -> None:
    """Every way in which ``plm`` is not an MPNet encoder that the kernels cover, at once."""
    cfg = plm.config
    problems = []
    if getattr(cfg, "model_type", None) != "mpnet":
        problems.append(f"model_type={getattr(cfg, 'model_type', None)!r} (this module takes MPNet encoders)")
    heads = getattr(cfg, "num_attention_heads", 0)
    hidden = getattr(cfg, "hidden_size", 0)
    if not heads or hidden % heads or hidden // heads != HEAD_DIM:
        problems.append(f"head_dim={hidden // heads if heads else None} (the relative-position-bias attention kernels take {HEAD_DIM})")
    if getattr(cfg, "hidden_act", "gelu") != "gelu":
        problems.append(f"hidden_act={cfg.hidden_act!r} (the erf GELU only)")
    buckets = getattr(cfg, "relative_attention_num_buckets", NUM_BUCKETS)
    if buckets < NUM_BUCKETS:
        problems.append(f"relative_attention_num_buckets={buckets} (MPNetEncoder.compute_position_bias indexes {NUM_BUCKETS} rows)")
    if problems:
        raise NotImplementedError("gmlm_amd text-encoder kernels do not cover this PLM: " + "; ".join(problems))


def max_sequence(cfg) -> int:
    """Longest sequence the encoder takes: the position table less its two reserved rows, and the kernels' table bound."""
    return min(ops.RELBIAS_MAX_LEN, int(cfg.max_position_embeddings) - 2)


def _check_length(cfg, n: int) -> None:
    if n > max_sequence(cfg):
        raise ValueError(f"sequence length {n} exceeds {max_sequence(cfg)} = min({ops.RELBIAS_MAX_LEN}, max_position_embeddings "
                         f"{cfg.max_position_embeddings} - 2)")


# ---------------------------------------------------------------------------------------------
# the bias table and the fold of its gradient
# ---------------------------------------------------------------------------------------------
_BUCKETS = {}


def bucket_index(m: int, device="cpu"):
    """(bucket [2m - 1] long, gather [32, longest bucket] long) for rel = -(m - 1) .. m - 1, built once per (m, device).
    ``bucket`` is ``MPNetEncoder.relative_position_bucket(rel)`` with its defaults.  ``gather`` lists, per bucket, the table
    entries that read it, in ascending order, padded with 2m - 1 (the index of a zero column the fold appends)."""
    from transformers.models.mpnet.modeling_mpnet import MPNetEncoder
    device = torch.device(device)
    key = (int(m), device.type, device.index)
    hit = _BUCKETS.get(key)
    if hit is None:
        rel = torch.arange(-(m - 1), m, dtype=torch.long)
        bucket = MPNetEncoder.relative_position_bucket(rel)
        members = [torch.nonzero(bucket == k).flatten() for k in range(NUM_BUCKETS)]
        gather = torch.full((NUM_BUCKETS, max(1, max(t.numel() for t in members))), 2 * m - 1, dtype=torch.long)
        for k, t in enumerate(members):
            gather[k, :t.numel()] = t
        hit = _BUCKETS[key] = (bucket.to(device), gather.to(device))
    return hit


def fold_bias_grad(d_rel: torch.Tensor, gather: torch.Tensor) -> torch.Tensor:
    """d_rel [h, 2m - 1] -> the gradient [32, h] of the bucket rows: each bucket's entries gathered side by side and summed
    along the last dim (one reduction per output, fixed order, no atomics; not ``index_add_``)."""
    ext = torch.cat([d_rel, d_rel.new_zeros(d_rel.shape[0], 1)], 1)
    return ext[:, gather].sum(-1).t()


class _BiasTable(torch.autograd.Function):
    """weight [>= 32, h] -> fp32 table [h, 2m - 1] = weight[bucket(rel)]; the backward is ``fold_bias_grad``."""

    @staticmethod
    def forward(ctx, weight, bucket, gather):
        ctx.save_for_backward(gather)
        ctx.rows, ctx.dtype = weight.shape[0], weight.dtype
        return weight.detach().float()[bucket].t().contiguous()

    @staticmethod
    def backward(ctx, d_rel):
        (gather,) = ctx.saved_tensors
        dw = d_rel.new_zeros(ctx.rows, d_rel.shape[0])
        dw[:NUM_BUCKETS] = fold_bias_grad(d_rel, gather)
        return dw.to(ctx.dtype), None, None


def bias_table(weight: torch.Tensor, m: int) -> torch.Tensor:
    """The kernels' bias operand for sequences of at most ``m`` tokens: fp32 [h, 2m - 1], entry m - 1 + (j - i) = the bias of
    query i and key j, i.e. ``MPNetEncoder.compute_position_bias`` without its [L, L] expansion."""
    bucket, gather = bucket_index(m, weight.device)
    return _BiasTable.apply(weight, bucket, gather)


# ---------------------------------------------------------------------------------------------
# weights and layers
# ---------------------------------------------------------------------------------------------
def _layer_masters(layer):
    sa = layer.attention.attn
    return [sa.q.weight, sa.k.weight, sa.v.weight], [sa.q.bias, sa.k.bias, sa.v.bias], sa.o, layer.attention.LayerNorm


def prepare_weights(plm, cd, gemm_precision="native"):
    """``encoder.prepare_weights`` over the MPNetLayers."""
    return encoder.prepare_weights(plm.encoder.layer, _layer_masters, cd, gemm_precision)


def _layer(lw, h, table, lens, heads, training, p_hidden, p_attn, eps, cu=None, max_len=0):
    scale = HEAD_DIM ** -0.5
    qkv, h_res = _mm(h, lw.wqkv, lw.bqkv, lw.m_qkv, residual=True)    # [B, L, 3P] or packed [T, 3P]; the bias sum is _mm's own
    if cu is not None:
        ctx = ops.attention_relbias_qkv_varlen(qkv, table, cu, max_len, heads, scale, p_attn, training)
    else:
        ctx = ops.attention_relbias_qkv(qkv, table, lens, heads, scale, p_attn, training)
    return encoder.post_ln_tail(lw, ctx, h_res, training, p_hidden, eps)


def _encode_rows(plm, x, lens, max_len, cd, training, gradient_checkpointing, weights, *packed):
    """Embedding LayerNorm + dropout and the layers over the embedding rows ``x`` in ``cd`` ([B, L, P] with ``lens``, or [T, P]
    with ``packed`` = (cu_seqlens, max_len)); all layers read ONE bias table, so its gradient is the sum over the layers."""
    cfg = plm.config
    emb = plm.embeddings
    eps, p_hidden, p_attn = cfg.layer_norm_eps, cfg.hidden_dropout_prob, cfg.attention_probs_dropout_prob
    h = ops.bias_res_layernorm(x, None, None, emb.LayerNorm.weight, emb.LayerNorm.bias, eps, False, p_hidden, training)
    heads = cfg.num_attention_heads
    if weights is None:
        weights = prepare_weights(plm, cd)
    table = bias_table(plm.encoder.relative_attention_bias.weight, max(int(max_len), 1))
    args = (table, lens, heads, training, p_hidden, p_attn, eps, *packed)
    return encoder.run_layers(_layer, weights, h, args, training, gradient_checkpointing)


def position_ids(l: int, padding_idx: int, device=None) -> torch.Tensor:
    """Rows of the position table for tokens 0 .. l - 1 of a right-padded text: padding_idx + 1 + i, what
    ``create_position_ids_from_input_ids`` yields for every non-pad token."""
    return torch.arange(padding_idx + 1, padding_idx + 1 + l, dtype=torch.long, device=device)


def mpnet_encode(plm, input_ids: torch.Tensor, lens: torch.Tensor, cd: torch.dtype, training: bool = False,
                 gradient_checkpointing: bool = False, weights=None) -> torch.Tensor:
    """input_ids int [B, L] (left-aligned: padding anywhere past ``lens[b]`` is ignored), lens int32 [B] -> [B, L, P] in ``cd``.

    Padded key positions get probability 0 in every layer; rows at or past ``lens[b]`` are computed but never read by the
    pooling.  ``weights``: optional ``prepare_weights`` result shared across micro-batches."""
    emb = plm.embeddings
    b, l = input_ids.shape
    _check_length(plm.config, l)
    x = torch.nn.functional.embedding(input_ids.long(), emb.word_embeddings.weight)   # bit-exact row gather
    x = x + emb.position_embeddings.weight[emb.padding_idx + 1:emb.padding_idx + 1 + l].unsqueeze(0)
    return _encode_rows(plm, x.to(cd), lens, l, cd, training, gradient_checkpointing, weights)


def mpnet_encode_packed(plm, tok: torch.Tensor, pos: torch.Tensor, cu_seqlens: torch.Tensor, max_len: int, cd: torch.dtype,
                        training: bool = False, gradient_checkpointing: bool = False, weights=None) -> torch.Tensor:
    """Packed (varlen) pass: tok / pos int [T] (token id and position inside its sequence of every row, the sequences back to
    back), cu_seqlens int32 [S + 1], max_len >= the longest sequence -> [T, P] in ``cd``.  Every GEMM / LayerNorm / GELU row is
    a real token; the attention resolves its rows, and the relative positions, through ``cu_seqlens``."""
    emb = plm.embeddings
    max_len = int(max_len)
    _check_length(plm.config, max_len)
    encoder.check_packed(tok, pos)
    word = emb.word_embeddings.weight
    # word + position rows in one pass (fp32 sum, stored as cd); the kernel's type-0 row is a zero row here
    x = ops.embed_sum(tok, pos.long() + (emb.padding_idx + 1), word, emb.position_embeddings.weight, word.new_zeros(1, word.shape[1]), cd)
    return _encode_rows(plm, x, None, max_len, cd, training, gradient_checkpointing, weights, cu_seqlens, max_len)
