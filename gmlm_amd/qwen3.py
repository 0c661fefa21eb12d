"""Qwen3-geometry text encoder forward on the gfx950 kernels.

Replaces the forward of HuggingFace ``Qwen3Model`` (hf:modeling_qwen3.py: Qwen3RMSNorm, Qwen3RotaryEmbedding,
Qwen3Attention, Qwen3MLP, Qwen3DecoderLayer) as the reference runs it on ``Qwen/Qwen3-Embedding-0.6B`` (main.py:1007, 349),
while keeping the HF module as the *parameter container*: state-dict keys stay ``plm_encoder.layers.N.*`` etc.

Per layer:  add + RMSNorm (one kernel, also yields the residual stream) -> fused Q|K|V GEMM (hipBLASLt)
            -> per-head RMSNorm of Q / K + rotary embedding -> causal attention, grouped KV heads (MFMA, per-sequence length)
            -> O GEMM -> add + RMSNorm -> fused gate|up GEMM -> SwiGLU -> down GEMM.
Two layouts: padded ([B, L, .] with ``lens``, ``qwen3_encode``) and packed / varlen ([T, .] rows of the sequences back to back
with ``cu_seqlens`` and per-row positions, ``qwen3_encode_packed``: no padded token is computed).  There is no hipGraph,
bucketed, short-sequence or ring form of this encoder (DESIGN.md section 4 "Qwen3 encoder").
"""
from __future__ import annotations

import torch

from . import encoder, ops
from .dense import _mm, encoder_operands


def _sliding_window_in_use(cfg) -> bool:
    if getattr(cfg, "use_sliding_window", False) and getattr(cfg, "sliding_window", None):
        return True
    return any(t != "full_attention" for t in (getattr(cfg, "layer_types", None) or ()))


def _rope_type(cfg) -> str:
    for name in ("rope_parameters", "rope_scaling"):
        rp = getattr(cfg, name, None)
        if isinstance(rp, dict):
            t = rp.get("rope_type", rp.get("type"))
            if t is not None:
                return t
    return "default"


def rope_theta(cfg) -> float:
    rp = getattr(cfg, "rope_parameters", None)
    if isinstance(rp, dict) and rp.get("rope_theta") is not None:
        return float(rp["rope_theta"])
    return float(getattr(cfg, "rope_theta", 10000.0))


def head_dim(cfg) -> int:
    """``config.head_dim`` where the config has one (Qwen3: 128 with hidden 1024 and 16 heads), else hidden_size // heads."""
    hd = getattr(cfg, "head_dim", None)
    return int(hd) if hd else cfg.hidden_size // cfg.num_attention_heads


def check_supported(plm) -> None:
    cfg = plm.config
    problems = []
    if getattr(cfg, "model_type", None) != "qwen3":
        problems.append(f"model_type={getattr(cfg, 'model_type', None)!r} (this module takes Qwen3 encoders)")
    if getattr(cfg, "hidden_act", "silu") != "silu":
        problems.append(f"hidden_act={cfg.hidden_act!r}")
    if head_dim(cfg) != 128:
        problems.append(f"head_dim={head_dim(cfg)} (the causal attention kernels take 128)")
    if getattr(cfg, "attention_bias", False):
        problems.append("attention_bias")
    if _sliding_window_in_use(cfg):
        problems.append("sliding-window attention")
    if _rope_type(cfg) != "default":
        problems.append(f"rope type {_rope_type(cfg)!r} (default rotary embedding only)")
    if float(getattr(cfg, "attention_dropout", 0.0) or 0.0) != 0.0:
        problems.append(f"attention_dropout={cfg.attention_dropout} (no probability dropout in the causal kernels)")
    for name in ("hidden_dropout", "hidden_dropout_prob", "resid_pdrop"):
        if float(getattr(cfg, name, 0.0) or 0.0) != 0.0:
            problems.append(f"{name}={getattr(cfg, name)}")
    heads, kv = getattr(cfg, "num_attention_heads", 0), getattr(cfg, "num_key_value_heads", 0)
    if not heads or not kv or heads % kv:
        problems.append(f"{heads} query heads / {kv} KV heads")
    if problems:
        raise NotImplementedError("gmlm_amd text-encoder kernels do not cover this PLM: " + "; ".join(problems))


def rope_table(cfg, max_len: int, device) -> torch.Tensor:
    """fp32 [>= max_len, 2, 64]: ``encoder.rope_table`` for Qwen3RotaryEmbedding's theta and head dim."""
    return encoder.rope_table(rope_theta(cfg), head_dim(cfg), encoder.table_rows(cfg, max_len), device)


class LayerWeights:
    """Per-forward view of one Qwen3DecoderLayer: the GEMM operands in the compute dtype (fused ``wqkv`` [q|k|v] and ``wgu``
    [gate|up], ``wo``, ``wdown``; no autograd history) next to the fp32 masters their gradients go to (``dense._mm``)."""
    __slots__ = ("wqkv", "wo", "wgu", "wdown", "m_qkv", "m_wo", "m_gu", "m_down", "ln1", "ln2", "qn", "kn")


def _layer_masters(layer):
    sa, mlp = layer.self_attn, layer.mlp
    return ([sa.q_proj.weight, sa.k_proj.weight, sa.v_proj.weight], sa.o_proj.weight, [mlp.gate_proj.weight, mlp.up_proj.weight],
            mlp.down_proj.weight)


def prepare_weights(plm, cd, gemm_precision="native"):
    """One flat buffer in the compute dtype for all layers' GEMM weights, filled by ONE multi-tensor copy (Q/K/V rows land
    directly in the fused [(hq + 2 hkv) * 128, P] operand, gate / up rows in the fused [2 I, P] one).
    ``gemm_precision`` "bf16x3" (fp32 only): the four operands become ``dense.SplitWeight`` objects (see bert.prepare_weights)."""
    out, specs = [], []
    for i, layer in enumerate(plm.layers):
        wq, wo, wgu, wd = _layer_masters(layer)
        specs += [((i, "wqkv"), wq, 0), ((i, "wo"), [wo], 0), ((i, "wgu"), wgu, 0), ((i, "wdown"), [wd], 0)]
        lw = LayerWeights()
        lw.m_qkv, lw.m_wo, lw.m_gu, lw.m_down = tuple(wq), (wo,), tuple(wgu), (wd,)
        lw.ln1, lw.ln2 = layer.input_layernorm.weight, layer.post_attention_layernorm.weight
        lw.qn, lw.kn = layer.self_attn.q_norm.weight, layer.self_attn.k_norm.weight
        out.append(lw)
    operands = encoder_operands(specs, cd, gemm_precision)
    for i, lw in enumerate(out):
        lw.wqkv, lw.wo, lw.wgu, lw.wdown = (operands[(i, k)] for k in ("wqkv", "wo", "wgu", "wdown"))
    return out


def _layer(lw, stream, branch, lens, cs, hq, hkv, scale, eps, packed=None):
    """(residual stream, last branch output) of the previous layer -> the same pair after this layer; the add that joins them
    is fused into the next RMSNorm.  ``packed`` = (pos_ids, cu_seqlens, max_len): the rows are [T, .] packed sequences."""
    s1, y1 = ops.add_rmsnorm(stream, branch, lw.ln1, eps)
    qkv = _mm(y1, lw.wqkv, None, lw.m_qkv)
    if packed is not None:
        ctx = ops.rope_causal_attention_varlen(qkv, lw.qn, lw.kn, cs, *packed, hq, hkv, scale, eps)
    else:
        ctx = ops.rope_causal_attention(qkv, lw.qn, lw.kn, cs, lens, hq, hkv, scale, eps)
    s2, y2 = ops.add_rmsnorm(s1, _mm(ctx, lw.wo, None, lw.m_wo), lw.ln2, eps)
    m = ops.swiglu(_mm(y2, lw.wgu, None, lw.m_gu))
    return s2, _mm(m, lw.wdown, None, lw.m_down)


def qwen3_encode(plm, input_ids: torch.Tensor, lens: torch.Tensor, cd: torch.dtype, training: bool = False,
                 gradient_checkpointing: bool = False, weights=None) -> torch.Tensor:
    """input_ids int [B, L] (left-aligned: padding anywhere past ``lens[b]`` is ignored), lens int32 [B] -> [B, L, P] in ``cd``.

    Positions are 0..L-1 per row; a query sees the keys at or before it that lie below ``lens[b]``.  Rows at or past
    ``lens[b]`` are computed but never read by the pooling.  ``weights``: optional ``prepare_weights(plm, cd)`` result."""
    cfg = plm.config
    b, l = input_ids.shape
    encoder.check_length(cfg, l)
    x = torch.nn.functional.embedding(input_ids.long(), plm.embed_tokens.weight).to(cd)   # bit-exact row gather
    return _encode_rows(plm, x, lens, rope_table(cfg, l, x.device), cd, training, gradient_checkpointing, weights)


def _encode_rows(plm, x, lens, cs, cd, training, gradient_checkpointing, weights, *packed):
    """The layers and the final norm over the embedding rows ``x`` ([B, L, P] with ``lens``, or [T, P] with ``packed`` = the one
    trailing argument of ``_layer``)."""
    cfg = plm.config
    hq, hkv = cfg.num_attention_heads, cfg.num_key_value_heads
    eps, scale = cfg.rms_norm_eps, head_dim(cfg) ** -0.5
    if weights is None:
        weights = prepare_weights(plm, cd)
    stream, branch = encoder.run_layers(_layer, weights, (x, None), (lens, cs, hq, hkv, scale, eps, *packed), training,
                                        gradient_checkpointing)
    return ops.add_rmsnorm(stream, branch, plm.norm.weight, eps)[1]


def qwen3_encode_packed(plm, tok: torch.Tensor, pos: torch.Tensor, cu_seqlens: torch.Tensor, max_len: int, cd: torch.dtype,
                        training: bool = False, gradient_checkpointing: bool = False, weights=None) -> torch.Tensor:
    """Packed (varlen) pass: tok / pos int [T] (token id and position of every row, the sequences back to back), cu_seqlens
    int32 [S + 1] (sequence i = rows [cu[i], cu[i+1]), covering all T rows), max_len >= the longest sequence -> [T, P] in ``cd``.

    The same layer chain as ``qwen3_encode`` on [T, .] rows: the norms, SwiGLU and the GEMMs are row-wise, the rotary
    embedding reads its table row by ``pos`` and the attention resolves its rows through ``cu_seqlens``."""
    cfg = plm.config
    max_len = int(max_len)
    encoder.check_length(cfg, max_len)
    encoder.check_packed(tok, pos)
    x = torch.nn.functional.embedding(tok.long(), plm.embed_tokens.weight).to(cd)   # bit-exact row gather
    cs = rope_table(cfg, max_len, x.device)
    return _encode_rows(plm, x, None, cs, cd, training, gradient_checkpointing, weights, (pos.to(torch.int32), cu_seqlens, max_len))
