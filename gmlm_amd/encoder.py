"""What the text encoders (bert.py, mpnet.py, qwen3.py, modernbert.py, deberta.py, llama.py, eurobert.py, nomic_bert.py, gemma3.py) share: the loop over the layers with its checkpoint
rule, the rotary cos / sin table, the argument checks, and the post-LayerNorm layer of the BERT geometry (its weights and
everything after the attention)."""
from __future__ import annotations

import torch
from torch.utils.checkpoint import checkpoint

from . import ops
from .dense import _mm, encoder_operands


def run_layers(layer_fn, weights, state, args, training, gradient_checkpointing):
    """``state = layer_fn(lw, *state, *args)`` over the layers.  ``state`` is the hidden rows (post-LayerNorm encoders) or the
    pair (residual stream, last branch output) of a pre-norm encoder.  A checkpointed layer is recomputed with the very
    arguments it ran with."""
    pair = isinstance(state, tuple)
    for lw in weights:
        s = state if pair else (state,)
        if gradient_checkpointing and training and torch.is_grad_enabled():
            state = checkpoint(layer_fn, lw, *s, *args, use_reentrant=False)
        else:
            state = layer_fn(lw, *s, *args)
    return state


def check_length(cfg, n: int) -> None:
    if n > cfg.max_position_embeddings:
        raise ValueError(f"sequence length {n} exceeds max_position_embeddings {cfg.max_position_embeddings}")


def check_packed(tok: torch.Tensor, pos: torch.Tensor) -> None:
    if tok.dim() != 1 or pos.shape != tok.shape:
        raise ValueError("packed token ids and positions must be [T] tensors of one size")


_ROPE_TABLES = {}


def rope_table(theta: float, d: int, rows: int, device) -> torch.Tensor:
    """fp32 [>= rows, 2, d / 2]: cos and sin of position * inv_freq, computed as the HF rotary embeddings do (default rope type:
    inv_freq = theta^(-2i/d) in fp32, the products and cos / sin in fp32).  Built ONCE per (device, theta, head dim) and kept (a
    row depends on its position only, so every shorter sequence reads a prefix): no host work and no host-to-device copy per
    encoder call.  The callers ask for ``max_position_embeddings`` rows at least."""
    device = torch.device(device)
    key = (device.type, device.index, theta, d)
    hit = _ROPE_TABLES.get(key)
    if hit is None or hit.shape[0] < rows:
        # through int64, as Qwen3RotaryEmbedding spells it (ModernBertRotaryEmbedding's fp32 arange gives the same floats)
        inv_freq = 1.0 / (theta ** (torch.arange(0, d, 2, dtype=torch.int64).to(dtype=torch.float) / d))
        freqs = torch.arange(rows, dtype=torch.float32)[:, None] * inv_freq[None, :]
        hit = _ROPE_TABLES[key] = torch.stack([freqs.cos(), freqs.sin()], 1).contiguous().to(device)
    return hit


def table_rows(cfg, max_len: int) -> int:
    return max(int(max_len), int(getattr(cfg, "max_position_embeddings", 0) or 0))


# ---------------------------------------------------------------------------------------------
# the post-LayerNorm layer (BERT, MPNet): biased Q / K / V / O, erf-GELU FFN
# ---------------------------------------------------------------------------------------------
class LayerWeights:
    """Per-forward view of one post-LayerNorm layer's parameters: the GEMM operands in the compute dtype (``w*`` / ``bqkv``,
    no autograd history) next to the fp32 master parameters they were cast from.  Built ONCE per forward and
    shared by all micro-batches.  The GEMM wrappers compute with the cached copy and hand the weight /
    bias gradients straight to the MASTERS in fp32 (the split-K partial sums are fp32 already), so neither the
    per-weight cast kernels nor their backward casts exist."""
    __slots__ = ("wqkv", "bqkv", "wo", "wi", "wo2", "m_qkv", "m_wo", "m_wi", "m_wo2", "bo", "bi", "bo2", "ln1w", "ln1b",
                 "ln2w", "ln2b")


def prepare_weights(layers, masters_of, cd, gemm_precision="native"):
    """One flat buffer in the compute dtype for all layers' GEMM weights, filled by ONE multi-tensor copy
    (Q/K/V rows land directly in the fused [3P, P] operand, so there is no concatenation either).
    ``masters_of(layer)`` -> ([wq, wk, wv], [bq, bk, bv], the attention output's dense and its LayerNorm).
    ``gemm_precision`` "bf16x3" (fp32 only): ``lw.w*`` then hold ``dense.SplitWeight`` objects, the two bf16 three-part forms of
    the fused fp32 operand, split once here for all micro-batches; ``dense._mm`` picks the GEMM by the operand's type."""
    out, specs = [], []
    for i, layer in enumerate(layers):
        wq, bq, o, ln1 = masters_of(layer)
        wo, wi, wo2 = o.weight, layer.intermediate.dense.weight, layer.output.dense.weight
        specs += [((i, "wqkv"), wq, 0), ((i, "bqkv"), bq, 0), ((i, "wo"), [wo], 0), ((i, "wi"), [wi], 0), ((i, "wo2"), [wo2], 0)]
        lw = LayerWeights()
        lw.m_qkv, lw.m_wo, lw.m_wi, lw.m_wo2 = tuple(wq) + tuple(bq), (wo,), (wi,), (wo2,)
        lw.bo, lw.bi, lw.bo2 = o.bias, layer.intermediate.dense.bias, layer.output.dense.bias
        lw.ln1w, lw.ln1b = ln1.weight, ln1.bias
        lw.ln2w, lw.ln2b = layer.output.LayerNorm.weight, layer.output.LayerNorm.bias
        out.append(lw)
    operands = encoder_operands(specs, cd, gemm_precision)
    for i, lw in enumerate(out):
        lw.wqkv, lw.bqkv, lw.wo, lw.wi, lw.wo2 = (operands[(i, k)] for k in ("wqkv", "bqkv", "wo", "wi", "wo2"))
    return out


def post_ln_tail(lw, ctx, h_res, training, p_hidden, eps):
    """The layer after its attention: O GEMM -> K6 bias + dropout + residual + LayerNorm -> FFN-in GEMM -> bias + GELU ->
    FFN-out GEMM -> K6."""
    a = ops.bias_res_layernorm(_mm(ctx, lw.wo, None, lw.m_wo), lw.bo, h_res, lw.ln1w, lw.ln1b, eps, False, p_hidden, training)
    m_pre, a_res = _mm(a, lw.wi, None, lw.m_wi, residual=True)
    m = ops.bias_gelu(m_pre, lw.bi)
    return ops.bias_res_layernorm(_mm(m, lw.wo2, None, lw.m_wo2), lw.bo2, a_res, lw.ln2w, lw.ln2b, eps, False, p_hidden, training)
