"""DeBERTa-v2 / v3 text encoder forward on the gfx950 kernels.

Replaces the forward of HuggingFace ``DebertaV2Model`` (hf:modeling_deberta_v2.py: DebertaV2Embeddings, DisentangledSelfAttention,
DebertaV2Layer, DebertaV2Encoder) as the reference would run ``microsoft/deberta-v3-base`` and its siblings (main.py:213, 349),
while keeping the HF module as the *parameter container*: state-dict keys stay
``plm_encoder.encoder.layer.N.attention.self.query_proj.weight``, ``plm_encoder.encoder.rel_embeddings.weight`` etc.

A DeBERTa-v3 layer is a BERT layer (post-LayerNorm, biased Q / K / V / O, erf-GELU FFN) whose attention scores get two terms
that depend on the query row, the key row and their bucketed distance (``pos_att_type`` c2p + p2c, ``share_att_key``):

    R    = LayerNorm_enc(rel_embeddings.weight[0 : 2k])           once per forward; dropout per layer in training
    Qr   = query_proj(R),  Kr = key_proj(R)                       this layer's own projections, bias included
    s_ij = (q_i . k_j + q_i . Kr[c(i - j)] + k_j . Qr[c(i - j)]) / sqrt(3 d)
    c(r) = clamp(bucket(r) + k, 0, 2k - 1),  bucket = make_log_bucket_position(r, k, max_relative_positions)

    x = LayerNorm(word[ids])                                       (v3: no position table, no token types)
    per layer:  fused QKV GEMM -> Qr | Kr GEMM over the W reachable rows of R -> the tables C = Q Kr^T and Pt = K Qr^T (GEMMs
                batched over the heads, fp32 results) -> disentangled attention (attn_disent.hip, head dim 64) -> O GEMM
                -> K6 bias + dropout + residual + LayerNorm -> FFN-in GEMM -> bias + GELU -> FFN-out GEMM -> K6

``bucket`` is odd, so HF's separately built p2c index ``clamp(-bucket(j - i) + k)`` is ``c(i - j)`` too: both terms read ONE
column, which the kernels take from an int32 table ``col[2M - 1]`` (``bucket_columns``; M = the longest sequence of the call)
restricted to the W = c(M - 1) - c(1 - M) + 1 columns the call can reach.  The backward of the two tables is a kernel of its
own; from there autograd runs through the table GEMMs (dQ += dC Kr, dK += dPt Qr, dKr, dQr), the projections, the LayerNorm of
the relative embeddings and ``rel_embeddings.weight``.  The table GEMMs and the Qr | Kr GEMM are the library's, in the compute
dtype; under ``gemm_precision="bf16x3"`` (fp32 storage) they stay native fp32 GEMMs and do not go through ``dense._mm``.
Two layouts: padded ([B, L, .] with ``lens``, ``deberta_encode``) and packed ([T, .] rows with ``cu_seqlens``,
``deberta_encode_packed``).  There is no hipGraph, bucketed or ring form of this encoder (DESIGN.md section 4 "DeBERTa encoder").
"""
from __future__ import annotations

from typing import NamedTuple

import torch
import torch.nn.functional as F

from . import encoder, ops
from .dense import _f32_out, _mm
from .encoder import LayerWeights  # noqa: F401  (a DeBERTa layer's weights are a BERT layer's)

HEAD_DIM = 64


def check_supported(plm) -> None:
    """Every way in which ``plm`` is not a DeBERTa-v2 / v3 encoder that the kernels cover, at once."""
    cfg = plm.config
    problems = []
    if getattr(cfg, "model_type", None) != "deberta-v2":
        problems.append(f"model_type={getattr(cfg, 'model_type', None)!r} (this module takes DeBERTa-v2 / v3 encoders)")
    heads = getattr(cfg, "num_attention_heads", 0)
    hidden = getattr(cfg, "hidden_size", 0)
    head_dim = getattr(cfg, "attention_head_size", hidden // heads if heads else None)
    if not heads or hidden % heads or head_dim != HEAD_DIM:
        problems.append(f"head_dim={head_dim} (the disentangled attention kernels take {HEAD_DIM})")
    if not getattr(cfg, "relative_attention", False):
        problems.append("relative_attention=False (the encoder path is the disentangled attention)")
    pos_att = sorted(x.strip() for x in (getattr(cfg, "pos_att_type", None) or []))
    if pos_att != ["c2p", "p2c"]:
        problems.append(f"pos_att_type={getattr(cfg, 'pos_att_type', None)!r} (both terms, c2p and p2c)")
    if not getattr(cfg, "share_att_key", False):
        problems.append("share_att_key=False (the position projections are the layer's query_proj / key_proj)")
    norm = [x.strip() for x in str(getattr(cfg, "norm_rel_ebd", "none")).lower().split("|")]
    if norm != ["layer_norm"]:
        problems.append(f"norm_rel_ebd={getattr(cfg, 'norm_rel_ebd', 'none')!r} ('layer_norm' only)")
    if getattr(cfg, "position_buckets", -1) <= 0:
        problems.append(f"position_buckets={getattr(cfg, 'position_buckets', -1)} (log buckets, > 0)")
    if getattr(cfg, "position_biased_input", True):
        problems.append("position_biased_input=True (no absolute position table)")
    if getattr(cfg, "type_vocab_size", 0) > 0:
        problems.append(f"type_vocab_size={cfg.type_vocab_size} (no token-type table)")
    if getattr(cfg, "embedding_size", hidden) != hidden:
        problems.append(f"embedding_size={cfg.embedding_size} != hidden_size={hidden} (no embedding projection)")
    if getattr(cfg, "conv_kernel_size", 0) > 0:
        problems.append(f"conv_kernel_size={cfg.conv_kernel_size} (no convolution layer)")
    if getattr(cfg, "hidden_act", "gelu") != "gelu":
        problems.append(f"hidden_act={cfg.hidden_act!r} (the erf GELU only)")
    if problems:
        raise NotImplementedError("gmlm_amd text-encoder kernels do not cover this PLM: " + "; ".join(problems))


def max_sequence(cfg) -> int:
    """Longest sequence the encoder takes: the kernels' table bound (a v3 encoder has no position table to run out of)."""
    return ops.DISENT_MAX_LEN


def _check_length(cfg, n: int) -> None:
    if n > max_sequence(cfg):
        raise ValueError(f"sequence length {n} exceeds {max_sequence(cfg)} (the column-table bound of the disentangled attention kernels)")


def max_relative(cfg) -> int:
    """``max_relative_positions`` as DisentangledSelfAttention resolves it."""
    m = int(getattr(cfg, "max_relative_positions", -1))
    return m if m >= 1 else int(cfg.max_position_embeddings)


# ---------------------------------------------------------------------------------------------
# the column table
# ---------------------------------------------------------------------------------------------
class Columns(NamedTuple):
    col: torch.Tensor     # int32 [2m - 1]: col[m - 1 + (i - j)] = c(i - j) - first, in [0, width), non-decreasing
    first: int            # c(-(m - 1)): the row of the relative embeddings that column 0 stands for
    width: int            # W = c(m - 1) - first + 1 <= 2k


_COLUMNS = {}


def bucket_columns(m: int, k: int, max_rel: int, device="cpu") -> Columns:
    """The columns of query - key = -(m - 1) .. m - 1, built once per (m, k, max_rel, device) by HF's own
    ``make_log_bucket_position`` (what ``build_relative_position`` applies to i - j): ``col + first`` is
    ``clamp(build_relative_position(...) + k, 0, 2k - 1)`` read along i - j."""
    from transformers.models.deberta_v2.modeling_deberta_v2 import make_log_bucket_position
    device = torch.device(device)
    key = (int(m), int(k), int(max_rel), device.type, device.index)
    hit = _COLUMNS.get(key)
    if hit is None:
        rel = torch.arange(-(m - 1), m, dtype=torch.long)
        c = torch.clamp(make_log_bucket_position(rel, int(k), int(max_rel)).to(torch.long) + k, 0, 2 * k - 1)
        first = int(c[0])
        hit = _COLUMNS[key] = Columns((c - first).to(torch.int32).to(device), first, int(c[-1]) - first + 1)
    return hit


# ---------------------------------------------------------------------------------------------
# the two tables
# ---------------------------------------------------------------------------------------------
def _bmm_f32(a, b):
    """Batched a @ b with an fp32 result straight out of the GEMM when the operands are 16-bit."""
    if a.dtype not in (torch.bfloat16, torch.float16):
        return torch.bmm(a, b)
    out = _f32_out("bmm", a, b)
    return torch.bmm(a, b).float() if out is None else out


class _Tables(torch.autograd.Function):
    """qkv [..., 3 * h * d] (fused Q | K | V rows), qkr [W, 2 * h * d] (Qr | Kr rows) -> the fp32 tables C = Q Kr^T and
    Pt = K Qr^T, [h, rows, W] each: two GEMMs batched over the heads that read the fused buffers through strides.  The backward
    is four more: dQ = dC Kr, dK = dPt Qr (into a buffer of qkv's layout whose V third is zero), dKr = dC^T Q, dQr = dPt^T K."""

    @staticmethod
    def forward(ctx, qkv, qkr, heads):
        d = qkv.shape[-1] // (3 * heads)
        q3 = qkv.reshape(-1, 3, heads, d)
        r3 = qkr.reshape(-1, 2, heads, d)
        c2p = _bmm_f32(q3[:, 0].permute(1, 0, 2), r3[:, 1].permute(1, 2, 0))
        p2c = _bmm_f32(q3[:, 1].permute(1, 0, 2), r3[:, 0].permute(1, 2, 0))
        ctx.save_for_backward(qkv, qkr)
        ctx.heads = heads
        return c2p, p2c

    @staticmethod
    def backward(ctx, g_c2p, g_p2c):
        qkv, qkr = ctx.saved_tensors
        heads = ctx.heads
        d = qkv.shape[-1] // (3 * heads)
        q3 = qkv.reshape(-1, 3, heads, d)
        r3 = qkr.reshape(-1, 2, heads, d)
        gc, gp = g_c2p.to(qkv.dtype), g_p2c.to(qkv.dtype)
        dqkv = torch.zeros_like(q3)
        dqkv[:, 0] = torch.bmm(gc, r3[:, 1].permute(1, 0, 2)).permute(1, 0, 2)
        dqkv[:, 1] = torch.bmm(gp, r3[:, 0].permute(1, 0, 2)).permute(1, 0, 2)
        dqkr = torch.empty_like(r3)
        dqkr[:, 1] = _bmm_f32(gc.transpose(1, 2), q3[:, 0].permute(1, 0, 2)).permute(1, 0, 2)
        dqkr[:, 0] = _bmm_f32(gp.transpose(1, 2), q3[:, 1].permute(1, 0, 2)).permute(1, 0, 2)
        return dqkv.view(qkv.shape), dqkr.view(qkr.shape), None


def position_tables(qkv: torch.Tensor, qkr: torch.Tensor, heads: int):
    """(C, Pt) fp32 [h, rows, W] for the fused rows ``qkv`` and the projected relative embeddings ``qkr`` = Qr | Kr [W, 2 * h * d]."""
    return _Tables.apply(qkv, qkr, heads)


# ---------------------------------------------------------------------------------------------
# weights and layers
# ---------------------------------------------------------------------------------------------
def _layer_masters(layer):
    sa = layer.attention.self
    return ([sa.query_proj.weight, sa.key_proj.weight, sa.value_proj.weight], [sa.query_proj.bias, sa.key_proj.bias, sa.value_proj.bias],
            layer.attention.output.dense, layer.attention.output.LayerNorm)


def prepare_weights(plm, cd, gemm_precision="native"):
    """``encoder.prepare_weights`` over the DebertaV2Layers: Q / K / V in one fused operand, the masters kept."""
    return encoder.prepare_weights(plm.encoder.layer, _layer_masters, cd, gemm_precision)


def _layer(lw, h, rel, col, lens, heads, training, p_hidden, p_attn, eps, cu=None, max_len=0):
    scale = (3 * HEAD_DIM) ** -0.5
    qkv, h_res = _mm(h, lw.wqkv, lw.bqkv, lw.m_qkv, residual=True)    # [B, L, 3P] or packed [T, 3P]; the bias sum is _mm's own
    wq, wk, _, bq, bk, _ = lw.m_qkv
    with torch.autocast("cuda", enabled=False):
        r = F.dropout(rel, p_hidden, training)                       # torch's own mask: a checkpoint replays it with the RNG state
        qkr = F.linear(r, torch.cat([wq, wk]).to(r.dtype), torch.cat([bq, bk]).to(r.dtype))    # Qr | Kr [W, 2P]
        c2p, p2c = position_tables(qkv, qkr, heads)
    if cu is not None:
        ctx = ops.attention_disent_qkv_varlen(qkv, c2p, p2c, col, cu, max_len, heads, scale, p_attn, training)
    else:
        ctx = ops.attention_disent_qkv(qkv, c2p, p2c, col, lens, heads, scale, p_attn, training)
    return encoder.post_ln_tail(lw, ctx, h_res, training, p_hidden, eps)


def relative_rows(plm, cols: Columns, cd) -> torch.Tensor:
    """The ``cols.width`` rows of LayerNorm(rel_embeddings.weight[0 : 2k]) that the call can reach, in ``cd``."""
    enc, cfg = plm.encoder, plm.config
    w = enc.rel_embeddings.weight[cols.first:cols.first + cols.width]
    return F.layer_norm(w, (w.shape[-1],), enc.LayerNorm.weight, enc.LayerNorm.bias, cfg.layer_norm_eps).to(cd)


def _encode_rows(plm, x, lens, max_len, cd, training, gradient_checkpointing, weights, *packed):
    """Embedding LayerNorm + dropout and the layers over the embedding rows ``x`` in ``cd`` ([B, L, P] with ``lens``, or [T, P]
    with ``packed`` = (cu_seqlens, max_len)); all layers read ONE normalised slice of the relative embeddings."""
    cfg = plm.config
    emb = plm.embeddings
    eps, p_hidden, p_attn = cfg.layer_norm_eps, cfg.hidden_dropout_prob, cfg.attention_probs_dropout_prob
    h = ops.bias_res_layernorm(x, None, None, emb.LayerNorm.weight, emb.LayerNorm.bias, eps, False, p_hidden, training)
    heads = cfg.num_attention_heads
    if weights is None:
        weights = prepare_weights(plm, cd)
    cols = bucket_columns(max(int(max_len), 1), int(cfg.position_buckets), max_relative(cfg), x.device)
    rel = relative_rows(plm, cols, cd)
    args = (rel, cols.col, lens, heads, training, p_hidden, p_attn, eps, *packed)
    return encoder.run_layers(_layer, weights, h, args, training, gradient_checkpointing)


def deberta_encode(plm, input_ids: torch.Tensor, lens: torch.Tensor, cd: torch.dtype, training: bool = False,
                   gradient_checkpointing: bool = False, weights=None) -> torch.Tensor:
    """input_ids int [B, L] (left-aligned: padding anywhere past ``lens[b]`` is ignored), lens int32 [B] -> [B, L, P] in ``cd``.

    Padded key positions get probability 0 in every layer; rows at or past ``lens[b]`` are computed but never read by the
    pooling.  ``weights``: optional ``prepare_weights`` result shared across micro-batches."""
    b, l = input_ids.shape
    _check_length(plm.config, l)
    x = F.embedding(input_ids.long(), plm.embeddings.word_embeddings.weight)   # bit-exact row gather
    return _encode_rows(plm, x.to(cd), lens, l, cd, training, gradient_checkpointing, weights)


def deberta_encode_packed(plm, tok: torch.Tensor, pos: torch.Tensor, cu_seqlens: torch.Tensor, max_len: int, cd: torch.dtype,
                          training: bool = False, gradient_checkpointing: bool = False, weights=None) -> torch.Tensor:
    """Packed (varlen) pass: tok / pos int [T] (token id and position inside its sequence of every row, the sequences back to
    back; the positions are not read: the attention resolves them through ``cu_seqlens``), cu_seqlens int32 [S + 1], max_len >=
    the longest sequence -> [T, P] in ``cd``.  Every GEMM / LayerNorm / GELU row is a real token."""
    max_len = int(max_len)
    _check_length(plm.config, max_len)
    encoder.check_packed(tok, pos)
    x = F.embedding(tok.long(), plm.embeddings.word_embeddings.weight)
    return _encode_rows(plm, x.to(cd), None, max_len, cd, training, gradient_checkpointing, weights, cu_seqlens, max_len)
