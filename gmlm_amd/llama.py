"""Llama-architecture text encoders without the Q / K head norm on the gfx950 kernels: Llama, Qwen2 / Qwen2.5 and Mistral.

Replaces the forward of HuggingFace ``LlamaModel`` / ``Qwen2Model`` / ``MistralModel`` (hf:modeling_llama.py, modeling_qwen2.py,
modeling_mistral.py: RMSNorm, rotary embedding, attention with grouped KV heads, gated MLP, decoder layer), the siblings of
the ``Qwen/Qwen3-Embedding-0.6B`` the reference runs (main.py:213, 1007), while keeping the HF module as the *parameter
container*: state-dict keys stay ``plm_encoder.layers.N.*`` etc.

Per layer:  add + RMSNorm (one kernel, also yields the residual stream) -> fused Q|K|V GEMM (hipBLASLt; with its bias where the
            model has one: Qwen2 always, Llama with ``attention_bias``) -> rotary embedding IN PLACE on the Q | K head rows
            -> causal attention, grouped KV heads, head dim 64 or 128 (MFMA, per-sequence length) -> O GEMM (+ bias)
            -> add + RMSNorm -> fused gate|up GEMM -> SwiGLU -> down GEMM.
It is the Qwen3 layer (qwen3.py) without the per-head RMSNorm of Q and K; the rotary table is built from the model's own
``rotary_emb`` (rope types default, linear and llama3).  Two layouts: padded (``llama_encode``) and packed / varlen
(``llama_encode_packed``).  A sliding window (Mistral; Qwen2 with ``use_sliding_window``) is accepted as long as no sequence of
the call is longer than the window: there is no causal band kernel.  There is no hipGraph, bucketed, short-sequence or ring
form of this encoder (DESIGN.md section 4 "Llama, Qwen2 and Mistral encoders").
"""
from __future__ import annotations

import weakref

import torch

from . import encoder, ops
from .dense import _mm, encoder_operands
from .qwen3 import _rope_type, head_dim

MODEL_TYPES = ("llama", "qwen2", "mistral")
ROPE_TYPES = ("default", "linear", "llama3")     # inv_freq and attention_scaling do not depend on the sequence length


def sliding_window(cfg):
    """The window of the model's attention (a query sees the ``window`` keys ending at itself), or None: Mistral's
    ``sliding_window``; Qwen2's when ``use_sliding_window`` is set (its upper layers then use it)."""
    w = getattr(cfg, "sliding_window", None)
    if not w:
        return None
    if cfg.model_type == "qwen2" and not getattr(cfg, "use_sliding_window", False):
        return None
    return int(w)


def check_window(cfg, longest: int) -> None:
    w = sliding_window(cfg)
    if w is not None and int(longest) > w:
        raise ValueError(f"sequence length {int(longest)} exceeds sliding_window {w}: the causal kernels have no band form")


def check_supported(plm) -> None:
    check_config(plm.config, MODEL_TYPES, "Llama, Qwen2 and Mistral", "causal")


def check_config(cfg, model_types, names: str, mask: str) -> None:
    """Every way in which ``cfg`` is not a Llama-layer encoder that the kernels cover, at once.  ``model_types`` / ``names``: what
    the calling module takes; ``mask``: how it names its attention kernels ("causal"; eurobert.py: "grouped")."""
    problems = []
    if getattr(cfg, "model_type", None) not in model_types:
        problems.append(f"model_type={getattr(cfg, 'model_type', None)!r} (this module takes {names} encoders)")
    if getattr(cfg, "hidden_act", "silu") != "silu":
        problems.append(f"hidden_act={cfg.hidden_act!r}")
    if head_dim(cfg) not in ops.GQA_HEAD_DIMS:
        problems.append(f"head_dim={head_dim(cfg)} (the rotary and {mask} attention kernels take 64 or 128)")
    if getattr(cfg, "mlp_bias", False):
        problems.append("mlp_bias")
    if float(getattr(cfg, "attention_dropout", 0.0) or 0.0) != 0.0:
        problems.append(f"attention_dropout={cfg.attention_dropout} (no probability dropout in the {mask} kernels)")
    if int(getattr(cfg, "pretraining_tp", 1) or 1) > 1:
        problems.append(f"pretraining_tp={cfg.pretraining_tp}")
    heads, kv = getattr(cfg, "num_attention_heads", 0), getattr(cfg, "num_key_value_heads", 0)
    if not heads or not kv or heads % kv:
        problems.append(f"{heads} query heads / {kv} KV heads")
    if _rope_type(cfg) not in ROPE_TYPES:
        problems.append(f"rope type {_rope_type(cfg)!r} (default, linear and llama3 only: the table must not depend on the length)")
    if problems:
        raise NotImplementedError("gmlm_amd text-encoder kernels do not cover this PLM: " + "; ".join(problems))


_TABLES = weakref.WeakKeyDictionary()      # rotary module -> {(device type, index): table}


def rope_table(plm, max_len: int, device) -> torch.Tensor:
    """fp32 [>= max_len, 2, d / 2]: cos and sin as the model's own rotary embedding gives them (hf:LlamaRotaryEmbedding.forward:
    position * ``inv_freq`` in fp32, cos / sin in fp32, times ``attention_scaling``), so that the rope types ``ROPE_TYPES`` get
    the exact floats HF uses.  Built on the host, kept per rotary module (= configuration) and device, and rebuilt only for a
    longer sequence: a row depends on its position only."""
    rot = plm.rotary_emb
    if getattr(rot, "rope_type", "default") not in ROPE_TYPES:
        raise NotImplementedError(f"rope type {rot.rope_type!r}: its frequencies depend on the sequence length")
    device = torch.device(device)
    per_dev = _TABLES.setdefault(rot, {})
    key = (device.type, device.index)
    hit = per_dev.get(key)
    if hit is None or hit.shape[0] < max_len:
        rows = max(512, 1 << (int(max_len) - 1).bit_length())
        inv_freq = rot.inv_freq.detach().to(device="cpu", dtype=torch.float32)
        freqs = torch.arange(rows, dtype=torch.float32)[:, None] * inv_freq[None, :]
        scaling = rot.attention_scaling
        hit = per_dev[key] = torch.stack([freqs.cos() * scaling, freqs.sin() * scaling], 1).contiguous().to(device)
    return hit


class LayerWeights:
    """Per-forward view of one decoder layer: the GEMM operands in the compute dtype (fused ``wqkv`` [q|k|v] with ``bqkv``, ``wo``
    with ``bo``, fused ``wgu`` [gate|up], ``wdown``; no autograd history; a bias the model lacks is None) next to the fp32
    masters their gradients go to (``dense._mm``: weights, then biases)."""
    __slots__ = ("wqkv", "bqkv", "wo", "bo", "wgu", "wdown", "m_qkv", "m_wo", "m_gu", "m_down", "ln1", "ln2")


def prepare_weights(plm, cd, gemm_precision="native"):
    """One flat buffer in the compute dtype for all layers' GEMM weights and projection biases, filled by ONE multi-tensor copy
    (Q/K/V rows land directly in the fused [(hq + 2 hkv) * d, P] operand, gate / up rows in the fused [2 I, P] one).
    ``gemm_precision`` "bf16x3" (fp32 only): the four weight operands become ``dense.SplitWeight`` objects."""
    out, specs = [], []
    for i, layer in enumerate(plm.layers):
        sa, mlp = layer.self_attn, layer.mlp
        qkv = [sa.q_proj, sa.k_proj, sa.v_proj]
        wq, wgu = [m.weight for m in qkv], [mlp.gate_proj.weight, mlp.up_proj.weight]
        bq = [m.bias for m in qkv] if sa.q_proj.bias is not None else []
        bo = [sa.o_proj.bias] if sa.o_proj.bias is not None else []
        specs += [((i, "wqkv"), wq, 0), ((i, "wo"), [sa.o_proj.weight], 0), ((i, "wgu"), wgu, 0), ((i, "wdown"), [mlp.down_proj.weight], 0)]
        specs += [((i, "bqkv"), bq, 0)] if bq else []
        specs += [((i, "bo"), bo, 0)] if bo else []
        lw = LayerWeights()
        lw.m_qkv, lw.m_wo, lw.m_gu, lw.m_down = tuple(wq + bq), tuple([sa.o_proj.weight] + bo), tuple(wgu), (mlp.down_proj.weight,)
        lw.ln1, lw.ln2 = layer.input_layernorm.weight, layer.post_attention_layernorm.weight
        out.append(lw)
    operands = encoder_operands(specs, cd, gemm_precision)
    for i, lw in enumerate(out):
        lw.wqkv, lw.wo, lw.wgu, lw.wdown = (operands[(i, k)] for k in ("wqkv", "wo", "wgu", "wdown"))
        lw.bqkv, lw.bo = operands.get((i, "bqkv")), operands.get((i, "bo"))
    return out


def _layer(lw, stream, branch, lens, cs, hq, hkv, d, scale, eps, packed=None):
    """(residual stream, last branch output) of the previous layer -> the same pair after this layer; the add that joins them
    is fused into the next RMSNorm.  ``packed`` = (pos_ids, cu_seqlens, max_len[, groups]): the rows are [T, .] packed sequences;
    ``groups`` (``ops.pack_sequence_groups``, optional) lets the attention take the short-sequence kernels."""
    s1, y1 = ops.add_rmsnorm(stream, branch, lw.ln1, eps)
    qkv = _mm(y1, lw.wqkv, lw.bqkv, lw.m_qkv)
    if packed is not None:
        ctx = ops.rope_causal_gqa_varlen(qkv, cs, *packed[:3], hq, hkv, d, scale, groups=packed[3] if len(packed) > 3 else None)
    else:
        ctx = ops.rope_causal_gqa(qkv, cs, lens, hq, hkv, d, scale)
    s2, y2 = ops.add_rmsnorm(s1, _mm(ctx, lw.wo, lw.bo, lw.m_wo), lw.ln2, eps)
    m = ops.swiglu(_mm(y2, lw.wgu, None, lw.m_gu))
    return s2, _mm(m, lw.wdown, None, lw.m_down)


def _encode_rows(plm, x, lens, cs, cd, training, gradient_checkpointing, weights, *packed, layer=None):
    """The layers and the final norm over the embedding rows ``x`` ([B, L, P] with ``lens``, or [T, P] with ``packed`` = the one
    trailing argument of ``_layer``).  ``layer``: a layer function with ``_layer``'s arguments (eurobert.py: another attention)."""
    cfg = plm.config
    hq, hkv, d = cfg.num_attention_heads, cfg.num_key_value_heads, head_dim(cfg)
    eps, scale = cfg.rms_norm_eps, d ** -0.5
    if weights is None:
        weights = prepare_weights(plm, cd)
    stream, branch = encoder.run_layers(layer or _layer, weights, (x, None), (lens, cs, hq, hkv, d, scale, eps, *packed), training,
                                        gradient_checkpointing)
    return ops.add_rmsnorm(stream, branch, plm.norm.weight, eps)[1]


def llama_encode(plm, input_ids: torch.Tensor, lens: torch.Tensor, cd: torch.dtype, training: bool = False,
                 gradient_checkpointing: bool = False, weights=None) -> torch.Tensor:
    """input_ids int [B, L] (left-aligned: padding anywhere past ``lens[b]`` is ignored), lens int32 [B] -> [B, L, P] in ``cd``.

    Positions are 0..L-1 per row; a query sees the keys at or before it that lie below ``lens[b]``.  Rows at or past
    ``lens[b]`` are computed but never read by the pooling.  ``weights``: optional ``prepare_weights(plm, cd)`` result."""
    cfg = plm.config
    b, l = input_ids.shape
    encoder.check_length(cfg, l)
    check_window(cfg, l)
    x = torch.nn.functional.embedding(input_ids.long(), plm.embed_tokens.weight).to(cd)   # bit-exact row gather
    return _encode_rows(plm, x, lens, rope_table(plm, l, x.device), cd, training, gradient_checkpointing, weights)


def llama_encode_packed(plm, tok: torch.Tensor, pos: torch.Tensor, cu_seqlens: torch.Tensor, max_len: int, cd: torch.dtype,
                        training: bool = False, gradient_checkpointing: bool = False, weights=None, groups=None) -> torch.Tensor:
    """Packed (varlen) pass: tok / pos int [T] (token id and position of every row, the sequences back to back), cu_seqlens
    int32 [S + 1] (sequence i = rows [cu[i], cu[i+1]), covering all T rows), max_len >= the longest sequence -> [T, P] in ``cd``.
    ``groups``: optional ``ops.pack_sequence_groups`` of the sequence lengths (int32 [G + 1] on the device): at head dim 64, bf16,
    max_len <= 128 and >= 512 (sequence, query head) pairs the attention runs on the short-sequence kernels."""
    cfg = plm.config
    max_len = int(max_len)
    encoder.check_length(cfg, max_len)
    check_window(cfg, max_len)
    encoder.check_packed(tok, pos)
    x = torch.nn.functional.embedding(tok.long(), plm.embed_tokens.weight).to(cd)   # bit-exact row gather
    cs = rope_table(plm, max_len, x.device)
    return _encode_rows(plm, x, None, cs, cd, training, gradient_checkpointing, weights, (pos.to(torch.int32), cu_seqlens, max_len, groups))
