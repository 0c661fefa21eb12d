"""Gemma3 text encoders on the gfx950 kernels: ``google/embeddinggemma-300m`` (bidirectional), gemma-3-270m / -1b and the text
towers of gemma-3-4b / -12b (causal).

Replaces the forward of HuggingFace ``Gemma3TextModel`` (hf:modeling_gemma3.py: Gemma3TextScaledWordEmbedding, Gemma3RMSNorm,
Gemma3RotaryEmbedding, Gemma3Attention, Gemma3MLP, Gemma3DecoderLayer) while keeping the HF module as the *parameter container*:
state-dict keys stay ``plm_encoder.layers.N.*`` etc.

Every block output is normed before it joins the residual stream and the sum is normed again for the next block, all four
norms with weight ``1 + w``.  Per layer, given (residual stream s, y = input norm of s):
    fused Q|K|V GEMM of y (hipBLASLt) -> per-head RMSNorm of Q / K + rotary embedding + attention with grouped KV heads at head
    dim 256, causal or bidirectional, scale ``query_pre_attn_scalar ** -0.5`` (``ops.rope_gqa_d256``) -> O GEMM
    -> sandwich norm pair (post-attention, pre-feed-forward: ``ops.sandwich_rmsnorm``) -> fused gate|up GEMM -> tanh-GELU gated
    unit (``ops.geglu_tanh``) -> down GEMM -> sandwich norm pair (post-feed-forward, the NEXT layer's input norm or the model's
    final ``norm``).
The first layer's input norm is ``ops.add_rmsnorm`` without a branch, fed ``1 + w``.  The rotary table is built per layer type
(``sliding_attention``: local base frequency; ``full_attention``: global, rope types default and linear) from the model's own
``rotary_emb``.  Sliding layers: by default (``band=False``) a call is accepted as long as no sequence reaches past the window
(``check_window``; the message still says what this default path lacks).  With ``band=True`` a call whose longest sequence exceeds
``config.sliding_window`` runs its sliding layers on the band-limited kernels (``ops.rope_gqa_d256(..., window=sliding_window)``,
gmlm_attention_gqa_d256_band_*: query i sees key j iff |i - j| < window, causal 0 <= i - j < window, HF's exclusive window); its
full layers, and every layer of a call that fits under the window, run the kernels of the default path, so a short batch
launches exactly the same kernel set either way.  Two layouts: padded (``gemma3_encode``) and packed / varlen
(``gemma3_encode_packed``).  There is no hipGraph, bucketed, short-sequence or ring form of this encoder (DESIGN.md section 4
"Gemma3 encoder").
"""
from __future__ import annotations

import weakref

import torch

from . import encoder, ops
from .dense import _mm, encoder_operands

MODEL_TYPES = ("gemma3_text",)
HEAD_DIM = ops.GQA_WIDE_HEAD_DIM
ROPE_TYPES = ("default", "linear")     # inv_freq and attention_scaling do not depend on the sequence length
LAYER_TYPES = ("sliding_attention", "full_attention")
MAX_HIDDEN = 4096                      # widest row of the RMSNorm kernels
W_OFFSET = 1.0                         # Gemma3RMSNorm: x_hat * (1 + w)


def _layer_types(cfg):
    return list(getattr(cfg, "layer_types", None) or ["full_attention"] * cfg.num_hidden_layers)


def _rope_type(sub) -> str:
    """The rope type of one ``rope_parameters`` dict (absent or empty: default)."""
    return (sub or {}).get("rope_type", (sub or {}).get("type", "default"))


def _rope_types(cfg):
    """{layer type in use: its rope type}, read from ``rope_parameters[layer type]`` (absent: default)."""
    rp = getattr(cfg, "rope_parameters", None) or {}
    out = {}
    for lt in dict.fromkeys(_layer_types(cfg)):
        sub = rp.get(lt) if isinstance(rp, dict) else None
        out[lt] = _rope_type(sub)
    return out


def check_supported(plm) -> None:
    """Every way in which ``plm.config`` is not a Gemma3 text encoder that the kernels cover, at once."""
    cfg = plm.config
    problems = []
    if getattr(cfg, "model_type", None) not in MODEL_TYPES:
        problems.append(f"model_type={getattr(cfg, 'model_type', None)!r} (this module takes Gemma3 text encoders)")
    hd = getattr(cfg, "head_dim", None)
    if hd != HEAD_DIM:
        problems.append(f"head_dim={hd} (the head-norm, rotary and grouped-KV attention kernels of this encoder take 256)")
    act = getattr(cfg, "hidden_activation", None)
    if act != "gelu_pytorch_tanh":
        problems.append(f"hidden_activation={act!r}")
    if getattr(cfg, "attn_logit_softcapping", None) is not None:
        problems.append(f"attn_logit_softcapping={cfg.attn_logit_softcapping}")
    if float(getattr(cfg, "attention_dropout", 0.0) or 0.0) != 0.0:
        problems.append(f"attention_dropout={cfg.attention_dropout} (no probability dropout in the grouped kernels)")
    if getattr(cfg, "attention_bias", False):
        problems.append("attention_bias")
    heads, kv = getattr(cfg, "num_attention_heads", 0), getattr(cfg, "num_key_value_heads", 0)
    if not heads or not kv or heads % kv:
        problems.append(f"{heads} query heads / {kv} KV heads")
    for lt, rt in _rope_types(cfg).items():
        if lt not in LAYER_TYPES:
            problems.append(f"layer type {lt!r}")
        elif rt not in ROPE_TYPES:
            problems.append(f"rope type {rt!r} of {lt} layers (default and linear only: the table must not depend on the length)")
    if int(getattr(cfg, "hidden_size", 0) or 0) > MAX_HIDDEN:
        problems.append(f"hidden_size={cfg.hidden_size} (the RMSNorm kernels take rows up to {MAX_HIDDEN})")
    if problems:
        raise NotImplementedError("gmlm_amd text-encoder kernels do not cover this PLM: " + "; ".join(problems))


def check_window(cfg, longest: int) -> None:
    """A sliding layer sees the whole sequence iff no distance i - j reaches ``sliding_window``.  Causal: the mask is
    i - j < w.  Bidirectional: the config has already turned the checkpoint's window into w // 2 + 1 and the mask is |i - j| < w.
    Either way a sequence of L tokens is covered iff L <= w."""
    w = getattr(cfg, "sliding_window", None)
    if w and "sliding_attention" in _layer_types(cfg) and int(longest) > int(w):
        raise ValueError(f"sequence length {int(longest)} exceeds sliding_window {int(w)}: there is no band kernel at head dim 256")


def band_window(cfg, longest: int, band: bool) -> int:
    """The ``window`` of the call's sliding layers: ``config.sliding_window`` when ``band`` is set and the longest sequence
    exceeds it, else 0 (the kernels without a band; ``band`` False: after ``check_window``)."""
    if not band:
        check_window(cfg, longest)
        return 0
    w = getattr(cfg, "sliding_window", None)
    return int(w) if w and "sliding_attention" in _layer_types(cfg) and int(longest) > int(w) else 0


_TABLES = weakref.WeakKeyDictionary()      # rotary module -> {(layer type, device type, index): table}


def rope_tables(plm, max_len: int, device) -> dict:
    """{layer type: fp32 [>= max_len, 2, 128]}: cos and sin as the model's own rotary embedding gives them for that layer type
    (hf:Gemma3RotaryEmbedding.forward: position * ``<layer type>_inv_freq`` in fp32, cos / sin in fp32, times
    ``<layer type>_attention_scaling``).  Built on the host, kept per rotary module and device, and rebuilt only for a longer
    sequence: a row depends on its position only."""
    rot = plm.rotary_emb
    device = torch.device(device)
    per = _TABLES.setdefault(rot, {})
    out = {}
    for lt in dict.fromkeys(_layer_types(plm.config)):
        if getattr(rot, "rope_type", {}).get(lt, "default") not in ROPE_TYPES:
            raise NotImplementedError(f"rope type {rot.rope_type[lt]!r}: its frequencies depend on the sequence length")
        key = (lt, device.type, device.index)
        hit = per.get(key)
        if hit is None or hit.shape[0] < max_len:
            rows = max(512, 1 << (int(max_len) - 1).bit_length())
            inv_freq = getattr(rot, f"{lt}_inv_freq").detach().to(device="cpu", dtype=torch.float32)
            scaling = getattr(rot, f"{lt}_attention_scaling")
            freqs = torch.arange(rows, dtype=torch.float32)[:, None] * inv_freq[None, :]
            hit = per[key] = torch.stack([freqs.cos() * scaling, freqs.sin() * scaling], 1).contiguous().to(device)
        out[lt] = hit
    return out


class LayerWeights:
    """Per-forward view of one Gemma3DecoderLayer (or Gemma2DecoderLayer: ``qn`` and ``kn`` None): the GEMM operands in the compute dtype (fused ``wqkv`` [q|k|v] and ``wgu``
    [gate|up], ``wo``, ``wdown``; no autograd history) next to the fp32 masters their gradients go to (``dense._mm``), the norm
    weights (``ln_next``: the next layer's input norm, or the model's final norm) and the layer type."""
    __slots__ = ("wqkv", "wo", "wgu", "wdown", "m_qkv", "m_wo", "m_gu", "m_down", "ln_post_attn", "ln_pre_ff", "ln_post_ff", "ln_next",
                 "qn", "kn", "layer_type")


def prepare_weights(plm, cd, gemm_precision="native"):
    """One flat buffer in the compute dtype for all layers' GEMM weights, filled by ONE multi-tensor copy (Q/K/V rows land
    directly in the fused [(hq + 2 hkv) * 256, P] operand, gate / up rows in the fused [2 I, P] one).
    ``gemm_precision`` "bf16x3" (fp32 only): the four operands become ``dense.SplitWeight`` objects."""
    out, specs = [], []
    types = _layer_types(plm.config)
    n = len(plm.layers)
    for i, layer in enumerate(plm.layers):
        sa, mlp = layer.self_attn, layer.mlp
        wq, wgu = [sa.q_proj.weight, sa.k_proj.weight, sa.v_proj.weight], [mlp.gate_proj.weight, mlp.up_proj.weight]
        specs += [((i, "wqkv"), wq, 0), ((i, "wo"), [sa.o_proj.weight], 0), ((i, "wgu"), wgu, 0), ((i, "wdown"), [mlp.down_proj.weight], 0)]
        lw = LayerWeights()
        lw.m_qkv, lw.m_wo, lw.m_gu, lw.m_down = tuple(wq), (sa.o_proj.weight,), tuple(wgu), (mlp.down_proj.weight,)
        lw.ln_post_attn, lw.ln_pre_ff = layer.post_attention_layernorm.weight, layer.pre_feedforward_layernorm.weight
        lw.ln_post_ff = layer.post_feedforward_layernorm.weight
        lw.ln_next = plm.layers[i + 1].input_layernorm.weight if i + 1 < n else plm.norm.weight
        # a Gemma2 layer (gemma2.py shares this function) has no Q / K head norm
        lw.qn, lw.kn = (sa.q_norm.weight, sa.k_norm.weight) if hasattr(sa, "q_norm") else (None, None)
        lw.layer_type = types[i]
        out.append(lw)
    operands = encoder_operands(specs, cd, gemm_precision)
    for i, lw in enumerate(out):
        lw.wqkv, lw.wo, lw.wgu, lw.wdown = (operands[(i, k)] for k in ("wqkv", "wo", "wgu", "wdown"))
    return out


def _layer(lw, stream, y, lens, tables, hq, hkv, scale, causal, eps, window, packed=None):
    """(residual stream, its input norm) -> the same pair for the next layer (after the last: the model's output is the second).
    ``window``: 0, or the band of the sliding layers.  ``packed`` = (pos_ids, cu_seqlens, max_len): the rows are [T, .] packed
    sequences."""
    cs = tables[lw.layer_type]
    qkv = _mm(y, lw.wqkv, None, lw.m_qkv)
    w = window if lw.layer_type == "sliding_attention" else 0
    if packed is not None:
        ctx = ops.rope_gqa_d256_varlen(qkv, lw.qn, lw.kn, cs, *packed, hq, hkv, scale, causal, W_OFFSET, eps, window=w)
    else:
        ctx = ops.rope_gqa_d256(qkv, lw.qn, lw.kn, cs, lens, hq, hkv, scale, causal, W_OFFSET, eps, window=w)
    s1, y1 = ops.sandwich_rmsnorm(stream, _mm(ctx, lw.wo, None, lw.m_wo), lw.ln_post_attn, lw.ln_pre_ff, W_OFFSET, eps)
    m = ops.geglu_tanh(_mm(y1, lw.wgu, None, lw.m_gu))
    return ops.sandwich_rmsnorm(s1, _mm(m, lw.wdown, None, lw.m_down), lw.ln_post_ff, lw.ln_next, W_OFFSET, eps)


def _embed(plm, ids, cd):
    """hf:Gemma3TextScaledWordEmbedding: the row gather times ``embed_scale`` cast to the weight dtype; the padding row gets no
    gradient, as ``nn.Embedding`` has it."""
    emb = plm.embed_tokens
    x = torch.nn.functional.embedding(ids.long(), emb.weight, padding_idx=emb.padding_idx)
    return (x * emb.embed_scale.to(device=x.device, dtype=emb.weight.dtype)).to(cd)


def _encode_rows(plm, x, lens, tables, cd, training, gradient_checkpointing, weights, window, *packed):
    cfg = plm.config
    hq, hkv = cfg.num_attention_heads, cfg.num_key_value_heads
    eps, scale = cfg.rms_norm_eps, float(cfg.query_pre_attn_scalar) ** -0.5
    causal = not getattr(cfg, "use_bidirectional_attention", False)
    if weights is None:
        weights = prepare_weights(plm, cd)
    if not weights:
        return ops.add_rmsnorm(x, None, W_OFFSET + plm.norm.weight, eps)[1]
    y = ops.add_rmsnorm(x, None, W_OFFSET + plm.layers[0].input_layernorm.weight, eps)[1]   # the one norm without a branch before it
    return encoder.run_layers(_layer, weights, (x, y), (lens, tables, hq, hkv, scale, causal, eps, window, *packed), training,
                              gradient_checkpointing)[1]


def gemma3_encode(plm, input_ids: torch.Tensor, lens: torch.Tensor, cd: torch.dtype, training: bool = False,
                  gradient_checkpointing: bool = False, weights=None, band: bool = False) -> torch.Tensor:
    """input_ids int [B, L] (left-aligned: padding anywhere past ``lens[b]`` is ignored), lens int32 [B] -> [B, L, P] in ``cd``.

    Positions are 0..L-1 per row; a query sees the keys below ``lens[b]`` (a causal model: those at or before it).  Rows at or
    past ``lens[b]`` are computed but never read by the pooling.  ``weights``: optional ``prepare_weights(plm, cd)`` result.
    ``band``: False refuses L > ``sliding_window``; True runs the sliding layers of such a call on the band-limited kernels (the
    longest sequence of a padded call is its width L: no device value is read)."""
    cfg = plm.config
    b, l = input_ids.shape
    encoder.check_length(cfg, l)
    window = band_window(cfg, l, band)
    x = _embed(plm, input_ids, cd)
    return _encode_rows(plm, x, lens, rope_tables(plm, l, x.device), cd, training, gradient_checkpointing, weights, window)


def gemma3_encode_packed(plm, tok: torch.Tensor, pos: torch.Tensor, cu_seqlens: torch.Tensor, max_len: int, cd: torch.dtype,
                         training: bool = False, gradient_checkpointing: bool = False, weights=None, band: bool = False) -> torch.Tensor:
    """Packed (varlen) pass: tok / pos int [T] (token id and position of every row, the sequences back to back), cu_seqlens
    int32 [S + 1] (sequence i = rows [cu[i], cu[i+1]), covering all T rows), max_len >= the longest sequence -> [T, P] in ``cd``.
    ``band`` as in ``gemma3_encode``, decided by ``max_len``."""
    cfg = plm.config
    max_len = int(max_len)
    encoder.check_length(cfg, max_len)
    window = band_window(cfg, max_len, band)
    encoder.check_packed(tok, pos)
    x = _embed(plm, tok, cd)
    tables = rope_tables(plm, max_len, x.device)
    return _encode_rows(plm, x, None, tables, cd, training, gradient_checkpointing, weights, window,
                        (pos.to(torch.int32), cu_seqlens, max_len))
