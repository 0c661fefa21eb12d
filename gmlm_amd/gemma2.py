"""Gemma2 text encoders on the gfx950 kernels: ``google/gemma-2-2b`` and ``-9b`` and the embedders built on them
(``BAAI/bge-multilingual-gemma2``).

Replaces the forward of HuggingFace ``Gemma2Model`` (hf:modeling_gemma2.py: Gemma2TextScaledWordEmbedding, Gemma2RMSNorm,
Gemma2RotaryEmbedding, Gemma2Attention, Gemma2MLP, Gemma2DecoderLayer) while keeping the HF module as the *parameter container*:
state-dict keys stay ``plm_encoder.layers.N.*`` etc.

A Gemma2 layer is a Gemma3 layer (gemma3.py: the sandwich norms with weight ``1 + w``, the tanh-GELU gated unit, grouped KV heads
at head dim 256, scale ``query_pre_attn_scalar ** -0.5``) with two differences: the attention scores are soft-capped,
``z = c * tanh(q.k * scale / c)`` with ``c = config.attn_logit_softcapping`` BEFORE the mask and the softmax (HF applies the cap
on its eager and flex paths only), and there is no Q / K head norm: the rotary embedding is applied to the head rows directly.
Per layer, given (residual stream s, y = input norm of s):
    fused Q|K|V GEMM of y (hipBLASLt) -> rotary embedding + soft-capped causal attention (``ops.rope_softcap_gqa_d256``:
    gmlm_rope_heads_d256_*, gmlm_attention_gqa_d256_softcap_*) -> O GEMM -> sandwich norm pair (post-attention, pre-feed-forward:
    ``ops.sandwich_rmsnorm``) -> fused gate|up GEMM -> ``ops.geglu_tanh`` -> down GEMM -> sandwich norm pair (post-feed-forward,
    the NEXT layer's input norm or the model's final ``norm``).
The first layer's input norm is ``ops.add_rmsnorm`` without a branch, fed ``1 + w``.  ONE rotary table serves all layers, built
from the model's own ``rotary_emb`` (rope types default and linear).  Sliding layers: when the call's longest sequence exceeds
``config.sliding_window`` they run with ``window = sliding_window`` (query i sees key j iff 0 <= i - j < window, HF's exclusive
window), otherwise, like the full layers, without a band.  ``attn_logit_softcapping = None`` runs uncapped, on the kernels of the
Gemma3 encoder behind the same rotation.  ``final_logit_softcapping`` belongs to the LM head and is not read.  Two layouts: padded
(``gemma2_encode``) and packed / varlen (``gemma2_encode_packed``).  There is no hipGraph, bucketed, short-sequence or ring form
of this encoder (DESIGN.md section 4 "Gemma2 encoder").
"""
from __future__ import annotations

import weakref

import torch

from . import encoder, ops
from .dense import _mm
from .gemma3 import HEAD_DIM, LAYER_TYPES, MAX_HIDDEN, ROPE_TYPES, W_OFFSET, _embed, _layer_types, _rope_type, prepare_weights  # noqa: F401

MODEL_TYPES = ("gemma2",)


def check_supported(plm) -> None:
    """Every way in which ``plm.config`` is not a Gemma2 text encoder that the kernels cover, at once."""
    cfg = plm.config
    problems = []
    if getattr(cfg, "model_type", None) not in MODEL_TYPES:
        problems.append(f"model_type={getattr(cfg, 'model_type', None)!r} (this module takes Gemma2 text encoders)")
    hd = getattr(cfg, "head_dim", None)
    if hd != HEAD_DIM:
        problems.append(f"head_dim={hd} (the rotary and soft-capped grouped-KV attention kernels of this encoder take 256)")
    act = getattr(cfg, "hidden_activation", None)
    if act != "gelu_pytorch_tanh":
        problems.append(f"hidden_activation={act!r}")
    cap = getattr(cfg, "attn_logit_softcapping", None)
    if cap is not None and not (float(cap) > 0.0 and float(cap) != float("inf")):
        problems.append(f"attn_logit_softcapping={cap} (must be finite and > 0, or None)")
    if float(getattr(cfg, "attention_dropout", 0.0) or 0.0) != 0.0:
        problems.append(f"attention_dropout={cfg.attention_dropout} (no probability dropout in the grouped kernels)")
    if getattr(cfg, "attention_bias", False):
        problems.append("attention_bias")
    heads, kv = getattr(cfg, "num_attention_heads", 0), getattr(cfg, "num_key_value_heads", 0)
    if not heads or not kv or heads % kv:
        problems.append(f"{heads} query heads / {kv} KV heads")
    if int(getattr(cfg, "hidden_size", 0) or 0) > MAX_HIDDEN:
        problems.append(f"hidden_size={cfg.hidden_size} (the RMSNorm kernels take rows up to {MAX_HIDDEN})")
    for lt in dict.fromkeys(_layer_types(cfg)):
        if lt not in LAYER_TYPES:
            problems.append(f"layer type {lt!r}")
    rp = getattr(cfg, "rope_parameters", None) or getattr(cfg, "rope_scaling", None)      # one dict for all layers
    rt = _rope_type(rp if isinstance(rp, dict) else None)
    if rt not in ROPE_TYPES:
        problems.append(f"rope type {rt!r} (default and linear only: the table must not depend on the length)")
    if problems:
        raise NotImplementedError("gmlm_amd text-encoder kernels do not cover this PLM: " + "; ".join(problems))


def sliding_window(cfg, longest: int) -> int:
    """The ``window`` of the call's sliding layers: ``config.sliding_window`` when the longest sequence exceeds it (a sequence of
    L tokens is covered whole iff L <= w: the causal mask is i - j < w), else 0, the kernels without a band."""
    w = getattr(cfg, "sliding_window", None)
    return int(w) if w and "sliding_attention" in _layer_types(cfg) and int(longest) > int(w) else 0


_TABLES = weakref.WeakKeyDictionary()      # rotary module -> {(device type, index): table}


def rope_tables(plm, max_len: int, device) -> torch.Tensor:
    """fp32 [>= max_len, 2, 128], the one table of all layers: cos and sin as the model's own rotary embedding gives them
    (hf:Gemma2RotaryEmbedding.forward: position * ``inv_freq`` in fp32, cos / sin in fp32, times ``attention_scaling``).  Built on
    the host, kept per rotary module and device, and rebuilt only for a longer sequence: a row depends on its position only."""
    rot = plm.rotary_emb
    if getattr(rot, "rope_type", "default") not in ROPE_TYPES:
        raise NotImplementedError(f"rope type {rot.rope_type!r}: its frequencies depend on the sequence length")
    device = torch.device(device)
    per = _TABLES.setdefault(rot, {})
    key = (device.type, device.index)
    hit = per.get(key)
    if hit is None or hit.shape[0] < max_len:
        rows = max(512, 1 << (int(max_len) - 1).bit_length())
        inv_freq = rot.inv_freq.detach().to(device="cpu", dtype=torch.float32)
        freqs = torch.arange(rows, dtype=torch.float32)[:, None] * inv_freq[None, :]
        hit = per[key] = torch.stack([freqs.cos() * rot.attention_scaling, freqs.sin() * rot.attention_scaling], 1).contiguous().to(device)
    return hit


def _layer(lw, stream, y, lens, cs, hq, hkv, scale, softcap, eps, window, packed=None):
    """(residual stream, its input norm) -> the same pair for the next layer (after the last: the model's output is the second).
    ``window``: 0, or the band of the sliding layers.  ``packed`` = (pos_ids, cu_seqlens, max_len): the rows are [T, .] packed
    sequences."""
    qkv = _mm(y, lw.wqkv, None, lw.m_qkv)
    w = window if lw.layer_type == "sliding_attention" else 0
    if packed is not None:
        ctx = ops.rope_softcap_gqa_d256_varlen(qkv, cs, *packed, hq, hkv, scale, True, softcap, window=w)
    else:
        ctx = ops.rope_softcap_gqa_d256(qkv, cs, lens, hq, hkv, scale, True, softcap, window=w)
    s1, y1 = ops.sandwich_rmsnorm(stream, _mm(ctx, lw.wo, None, lw.m_wo), lw.ln_post_attn, lw.ln_pre_ff, W_OFFSET, eps)
    m = ops.geglu_tanh(_mm(y1, lw.wgu, None, lw.m_gu))
    return ops.sandwich_rmsnorm(s1, _mm(m, lw.wdown, None, lw.m_down), lw.ln_post_ff, lw.ln_next, W_OFFSET, eps)


def _encode_rows(plm, x, lens, cs, cd, training, gradient_checkpointing, weights, window, *packed):
    cfg = plm.config
    hq, hkv = cfg.num_attention_heads, cfg.num_key_value_heads
    eps, scale = cfg.rms_norm_eps, float(cfg.query_pre_attn_scalar) ** -0.5
    cap = getattr(cfg, "attn_logit_softcapping", None)
    softcap = None if cap is None else float(cap)
    if weights is None:
        weights = prepare_weights(plm, cd)
    if not weights:
        return ops.add_rmsnorm(x, None, W_OFFSET + plm.norm.weight, eps)[1]
    y = ops.add_rmsnorm(x, None, W_OFFSET + plm.layers[0].input_layernorm.weight, eps)[1]   # the one norm without a branch before it
    return encoder.run_layers(_layer, weights, (x, y), (lens, cs, hq, hkv, scale, softcap, eps, window, *packed), training,
                              gradient_checkpointing)[1]


def gemma2_encode(plm, input_ids: torch.Tensor, lens: torch.Tensor, cd: torch.dtype, training: bool = False,
                  gradient_checkpointing: bool = False, weights=None) -> torch.Tensor:
    """input_ids int [B, L] (left-aligned: padding anywhere past ``lens[b]`` is ignored), lens int32 [B] -> [B, L, P] in ``cd``.

    Positions are 0..L-1 per row; a query sees the keys below ``lens[b]`` at or before it.  Rows at or past ``lens[b]`` are
    computed but never read by the pooling.  ``weights``: optional ``prepare_weights(plm, cd)`` result.  The longest sequence of
    a padded call is its width L: no device value is read to decide the window."""
    cfg = plm.config
    b, l = input_ids.shape
    encoder.check_length(cfg, l)
    x = _embed(plm, input_ids, cd)
    return _encode_rows(plm, x, lens, rope_tables(plm, l, x.device), cd, training, gradient_checkpointing, weights, sliding_window(cfg, l))


def gemma2_encode_packed(plm, tok: torch.Tensor, pos: torch.Tensor, cu_seqlens: torch.Tensor, max_len: int, cd: torch.dtype,
                         training: bool = False, gradient_checkpointing: bool = False, weights=None) -> torch.Tensor:
    """Packed (varlen) pass: tok / pos int [T] (token id and position of every row, the sequences back to back), cu_seqlens
    int32 [S + 1] (sequence i = rows [cu[i], cu[i+1]), covering all T rows), max_len >= the longest sequence -> [T, P] in ``cd``.
    The window of the sliding layers is decided by ``max_len``."""
    cfg = plm.config
    max_len = int(max_len)
    encoder.check_length(cfg, max_len)
    encoder.check_packed(tok, pos)
    x = _embed(plm, tok, cd)
    return _encode_rows(plm, x, None, rope_tables(plm, max_len, x.device), cd, training, gradient_checkpointing, weights,
                        sliding_window(cfg, max_len), (pos.to(torch.int32), cu_seqlens, max_len))
