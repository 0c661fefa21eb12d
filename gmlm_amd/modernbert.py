"""ModernBERT text encoder forward on the gfx950 kernels.

Replaces the forward of HuggingFace ``ModernBertModel`` (hf:modeling_modernbert.py: ModernBertEmbeddings, ModernBertAttention,
ModernBertMLP, ModernBertEncoderLayer) as the reference would run ``answerdotai/ModernBERT-base`` and its embedding
fine-tunes (main.py:213, 349), while keeping the HF module as the *parameter container*: state-dict keys stay
``plm_encoder.layers.N.attn.Wqkv.weight`` etc.

    x = LayerNorm(tok_embeddings[ids])
    per layer:  add + LayerNorm (one kernel, also yields the residual stream; layer 0 has no attention norm)
                -> fused Wqkv GEMM (hipBLASLt) -> rotary embedding at head dim 64, in place (theta by layer type)
                -> attention: bidirectional, in a "sliding_attention" layer limited to |i - j| <= config.sliding_window
                -> Wo GEMM -> add + LayerNorm -> Wi GEMM -> GeGLU (erf GELU) -> mlp.Wo GEMM
    out = LayerNorm(x)

Two layouts: padded ([B, L, .] with ``lens``, ``modernbert_encode``) and packed / varlen ([T, .] rows of the sequences back to
back with ``cu_seqlens`` and per-row positions, ``modernbert_encode_packed``: no padded token is computed).  A full-attention
layer, and a sliding layer whose band hides no key of the batch (longest sequence <= window + 1), run the attention kernels
of the BERT path on the rotated buffer; only a sliding layer that the window actually cuts runs the band-limited kernels
(``ops.window_cuts``).  There is no hipGraph, bucketed or ring form of this encoder (DESIGN.md section 4 "ModernBERT encoder").
"""
from __future__ import annotations

import torch

from . import encoder, ops
from .dense import _mm, encoder_operands

HEAD_DIM = 64
LAYER_TYPES = ("full_attention", "sliding_attention")


def head_dim(cfg) -> int:
    hd = getattr(cfg, "head_dim", None)
    return int(hd) if hd else cfg.hidden_size // cfg.num_attention_heads


def _rope_params(cfg, layer_type: str) -> dict:
    rp = getattr(cfg, "rope_parameters", None)
    sub = rp.get(layer_type) if isinstance(rp, dict) else None
    return sub if isinstance(sub, dict) else {}


def rope_theta(cfg, layer_type: str) -> float:
    return float(_rope_params(cfg, layer_type).get("rope_theta", 10000.0))


def check_supported(plm) -> None:
    """Every way in which ``plm`` is not a ModernBERT encoder that the kernels cover, at once."""
    cfg = plm.config
    problems = []
    if getattr(cfg, "model_type", None) != "modernbert":
        problems.append(f"model_type={getattr(cfg, 'model_type', None)!r} (this module takes ModernBERT encoders)")
    heads = getattr(cfg, "num_attention_heads", 0)
    if not heads or getattr(cfg, "hidden_size", 0) % heads or head_dim(cfg) != HEAD_DIM:
        problems.append(f"head_dim={head_dim(cfg) if heads else None} (the rotary and band-limited attention kernels take {HEAD_DIM})")
    if getattr(cfg, "hidden_activation", "gelu") != "gelu":
        problems.append(f"hidden_activation={cfg.hidden_activation!r} (GeGLU with the erf GELU only)")
    for name in ("attention_bias", "mlp_bias", "norm_bias"):
        if getattr(cfg, name, False):
            problems.append(name)
    for name in ("attention_dropout", "embedding_dropout", "mlp_dropout"):
        if float(getattr(cfg, name, 0.0) or 0.0) != 0.0:
            problems.append(f"{name}={getattr(cfg, name)}")
    types = tuple(getattr(cfg, "layer_types", None) or ())
    other = sorted(set(types) - set(LAYER_TYPES))
    if other:
        problems.append(f"layer types {other} (full_attention / sliding_attention only)")
    for lt in LAYER_TYPES:
        rt = _rope_params(cfg, lt).get("rope_type", _rope_params(cfg, lt).get("type", "default"))
        if rt != "default":
            problems.append(f"rope type {rt!r} for {lt} (default rotary embedding only)")
    if getattr(cfg, "hidden_size", 0) > ops.ADD_LAYERNORM_MAX_F:
        problems.append(f"hidden_size={cfg.hidden_size} (the add + LayerNorm kernel takes rows of at most {ops.ADD_LAYERNORM_MAX_F})")
    if problems:
        raise NotImplementedError("gmlm_amd text-encoder kernels do not cover this PLM: " + "; ".join(problems))


def rope_table(cfg, layer_type: str, max_len: int, device) -> torch.Tensor:
    """fp32 [>= max_len, 2, 32]: ``encoder.rope_table`` for ModernBertRotaryEmbedding's theta of the layer type."""
    return encoder.rope_table(rope_theta(cfg, layer_type), HEAD_DIM, encoder.table_rows(cfg, max_len), device)


class LayerWeights:
    """Per-forward view of one ModernBertEncoderLayer: the GEMM operands in the compute dtype (``wqkv``, ``wo``, ``wi``,
    ``wmo``; no autograd history) next to the fp32 masters their gradients go to (``dense._mm``), the two norm weights
    (``ln1`` None: layer 0 has no attention norm) and the layer's attention type."""
    __slots__ = ("wqkv", "wo", "wi", "wmo", "m_qkv", "m_wo", "m_wi", "m_mo", "ln1", "ln2", "kind")


def prepare_weights(plm, cd, gemm_precision="native"):
    """One flat buffer in the compute dtype for all layers' GEMM weights, filled by ONE multi-tensor copy.
    ``gemm_precision`` "bf16x3" (fp32 only): the four operands become ``dense.SplitWeight`` objects (see bert.prepare_weights)."""
    out, specs = [], []
    for i, layer in enumerate(plm.layers):
        lw = LayerWeights()
        lw.m_qkv, lw.m_wo = (layer.attn.Wqkv.weight,), (layer.attn.Wo.weight,)
        lw.m_wi, lw.m_mo = (layer.mlp.Wi.weight,), (layer.mlp.Wo.weight,)
        specs += [((i, "wqkv"), list(lw.m_qkv), 0), ((i, "wo"), list(lw.m_wo), 0), ((i, "wi"), list(lw.m_wi), 0),
                  ((i, "wmo"), list(lw.m_mo), 0)]
        lw.ln1 = getattr(layer.attn_norm, "weight", None)           # nn.Identity in layer 0
        lw.ln2 = layer.mlp_norm.weight
        lw.kind = plm.config.layer_types[i]
        out.append(lw)
    operands = encoder_operands(specs, cd, gemm_precision)
    for i, lw in enumerate(out):
        lw.wqkv, lw.wo, lw.wi, lw.wmo = (operands[(i, k)] for k in ("wqkv", "wo", "wi", "wmo"))
    return out


def _layer(lw, stream, branch, lens, tables, heads, scale, eps, window, packed=None):
    """(residual stream, last branch output) of the previous layer -> the same pair after this layer; the add that joins them
    is fused into the next LayerNorm.  ``packed`` = (pos_ids, cu_seqlens, max_len): the rows are [T, .] packed sequences."""
    if lw.ln1 is None:
        s1, y1 = stream, stream                                     # layer 0: the embedding norm's output feeds Wqkv directly
    else:
        s1, y1 = ops.add_layernorm(stream, branch, lw.ln1, None, eps)
    qkv = _mm(y1, lw.wqkv, None, lw.m_qkv)
    if packed is not None:
        ctx = ops.rope_attention_varlen(qkv, tables[lw.kind], *packed, heads, scale, lw.kind, window)
    else:
        ctx = ops.rope_attention(qkv, tables[lw.kind], lens, heads, scale, lw.kind, window)
    s2, y2 = ops.add_layernorm(s1, _mm(ctx, lw.wo, None, lw.m_wo), lw.ln2, None, eps)
    m = ops.geglu(_mm(y2, lw.wi, None, lw.m_wi))
    return s2, _mm(m, lw.wmo, None, lw.m_mo)


def _embed(plm, ids, cd):
    emb = plm.embeddings.tok_embeddings
    x = torch.nn.functional.embedding(ids.long(), emb.weight, emb.padding_idx).to(cd)   # bit-exact row gather
    return ops.add_layernorm(x, None, plm.embeddings.norm.weight, None, plm.config.norm_eps)[1]


def _encode_rows(plm, x, lens, max_len, cd, training, gradient_checkpointing, weights, *packed):
    """The layers and the final norm over the normalised embedding rows ``x`` ([B, L, P] with ``lens``, or [T, P] with
    ``packed`` = the one trailing argument of ``_layer``)."""
    cfg = plm.config
    heads, eps, scale, window = cfg.num_attention_heads, cfg.norm_eps, HEAD_DIM ** -0.5, int(cfg.sliding_window)
    if weights is None:
        weights = prepare_weights(plm, cd)
    tables = {lt: rope_table(cfg, lt, max_len, x.device) for lt in set(cfg.layer_types)}
    stream, branch = encoder.run_layers(_layer, weights, (x, None), (lens, tables, heads, scale, eps, window, *packed), training,
                                        gradient_checkpointing)
    return ops.add_layernorm(stream, branch, plm.final_norm.weight, None, eps)[1]


def modernbert_encode(plm, input_ids: torch.Tensor, lens: torch.Tensor, cd: torch.dtype, training: bool = False,
                      gradient_checkpointing: bool = False, weights=None) -> torch.Tensor:
    """input_ids int [B, L] (left-aligned: padding anywhere past ``lens[b]`` is ignored), lens int32 [B] -> [B, L, P] in ``cd``.

    Positions are 0..L-1 per row; a query sees the keys below ``lens[b]`` (in a sliding layer: those within the window).
    Rows at or past ``lens[b]`` are computed but never read by the pooling.  ``weights``: optional ``prepare_weights`` result."""
    cfg = plm.config
    b, l = input_ids.shape
    encoder.check_length(cfg, l)
    return _encode_rows(plm, _embed(plm, input_ids, cd), lens, l, cd, training, gradient_checkpointing, weights)


def modernbert_encode_packed(plm, tok: torch.Tensor, pos: torch.Tensor, cu_seqlens: torch.Tensor, max_len: int, cd: torch.dtype,
                             training: bool = False, gradient_checkpointing: bool = False, weights=None) -> torch.Tensor:
    """Packed (varlen) pass: tok / pos int [T] (token id and position of every row, the sequences back to back), cu_seqlens
    int32 [S + 1] (sequence i = rows [cu[i], cu[i+1]), covering all T rows), max_len >= the longest sequence -> [T, P] in ``cd``.

    The same layer chain as ``modernbert_encode`` on [T, .] rows: the norms, GeGLU and the GEMMs are row-wise, the rotary
    embedding reads its table row by ``pos`` and the attention resolves its rows through ``cu_seqlens``."""
    cfg = plm.config
    max_len = int(max_len)
    encoder.check_length(cfg, max_len)
    encoder.check_packed(tok, pos)
    x = _embed(plm, tok, cd)
    return _encode_rows(plm, x, None, max_len, cd, training, gradient_checkpointing, weights, (pos.to(torch.int32), cu_seqlens, max_len))
