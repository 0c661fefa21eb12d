"""The operators of the Gemma2 text encoder that are autograd nodes of their own (include/gmlm_hip_gqa_softcap.h), re-exported by
ops.py: grouped-KV attention at head dim 256 with attention-logit soft-capping, ``SoftcapAttention256``
(``ops.gqa_d256_softcap_attention`` / ``_varlen``; gmlm_attention_gqa_d256_softcap_*), the rotary embedding on head rows at head
dim 256 without a head norm, ``ops.rope_heads_d256_`` (gmlm_rope_heads_d256_*), and the two in one node, ``RopeSoftcapGQA256``
(``ops.rope_softcap_gqa_d256`` / ``_varlen``).  The calls themselves are ``ops_gemma._band_fwd`` / ``_band_bwd`` with a
``softcap``.  The nodes stand in a module of their own because tests/test_gqa_band_cpu.py pins the set of nodes ops_gemma.py defines.

Every node returns one gradient entry per input whatever is frozen, like the nodes of ops.py; their frozen-input tests are
tests/test_gqa_softcap_cpu.py and tests/test_gpu_gqa_softcap_kernels.py.
"""
from __future__ import annotations

import torch

from . import ops as _o
from ._lib import check, lib
from .ops_gemma import D, _band_bwd, _band_fwd, _table, _window_arg


def _cap_args(softcap, window):
    softcap, window = float(softcap), int(window)
    if not (softcap > 0.0 and softcap != float("inf")):
        raise ValueError(f"softcap must be finite and > 0, got {softcap}")
    if not 0 <= window < 1 << 30:
        raise ValueError(f"window must be 0 (no band) or in [1, 2^30), got {window}")
    return softcap, window


class SoftcapAttention256(torch.autograd.Function):
    """Grouped-KV attention at head dim 256 with attention-logit soft-capping (gmlm_attention_gqa_d256_softcap_*): the scores enter
    the softmax as ``softcap * tanh(q.k * scale / softcap)``, capped before the mask of ``BandAttention256`` (``window`` 0: of
    ``gqa_d256_attention``).  The layouts, the zero rows, the single fused gradient buffer and the frozen-input contract of
    ``BandAttention256``."""

    @staticmethod
    def forward(ctx, q, k, v, kv_len, cu_seqlens, max_len, hq, hkv, scale, causal, softcap, window):
        softcap, window = _cap_args(softcap, window)
        _o._cuda(q, k, v)
        if cu_seqlens is not None:
            _, max_len = _o._varlen_args(q, cu_seqlens, max_len)
        want_lo = q.dtype == torch.bfloat16 and any(t.requires_grad for t in (q, k, v))
        out, out_lo, lse = _band_fwd(q, k, v, kv_len, cu_seqlens, max_len, hq, hkv, scale, causal, window, want_lo, softcap)
        ctx.save_for_backward(q, k, v, out, lse, kv_len, cu_seqlens, out_lo)
        ctx.cfg = (int(max_len), hq, hkv, float(scale), bool(causal), window, softcap)
        return out

    @staticmethod
    def backward(ctx, gout):
        q, k, v, out, lse, kv_len, cu, out_lo = ctx.saved_tensors
        max_len, hq, hkv, scale, causal, window, softcap = ctx.cfg
        nq, nk = hq * D, hkv * D
        dqkv = torch.empty(*q.shape[:-1], nq + 2 * nk, dtype=q.dtype, device=q.device)
        dq, dk, dv = dqkv[..., :nq], dqkv[..., nq:nq + nk], dqkv[..., nq + nk:]
        _band_bwd(q, k, v, out, out_lo, gout, lse, kv_len, cu, max_len, hq, hkv, scale, causal, window, dq, dk, dv, softcap)
        return (dq, dk, dv) + (None,) * 9


def gqa_d256_softcap_attention(q, k, v, kv_len, hq, hkv, scale, causal, softcap, window=0):
    """``gqa_d256_attention`` (``window`` > 0: ``gqa_d256_band_attention``) on the scores ``softcap * tanh(q.k * scale / softcap)``."""
    return SoftcapAttention256.apply(q, k, v, kv_len, None, 0, hq, hkv, scale, causal, softcap, window)


def gqa_d256_softcap_attention_varlen(q, k, v, cu_seqlens, max_len, hq, hkv, scale, causal, softcap, window=0):
    """The same on packed rows: sequence i = rows [cu_seqlens[i], cu_seqlens[i + 1])."""
    return SoftcapAttention256.apply(q, k, v, None, cu_seqlens, int(max_len), hq, hkv, scale, causal, softcap, window)


# ---- rotary embedding without a head norm (Gemma2), include/gmlm_hip_gqa_softcap.h ----------------------------------------------
def rope_heads_d256_(t, cos_sin, heads, seq_len, pos_ids=None, inverse=False):
    """Rotate (``inverse``: rotate back) the first ``heads`` = hq + hkv head rows of 256 elements of every fused [.., >= heads * 256]
    row of ``t`` IN PLACE; what follows them (V, padding columns) is not touched.  Positions are row % ``seq_len``, or ``pos_ids``
    (int32 [tokens]) when given.  Outside autograd: the building block of ``RopeSoftcapGQA256``."""
    _o._cuda(t)
    _table(cos_sin)
    tokens, stride = _o._qkv_rows(t, heads * D)
    name = "gmlm_rope_heads_d256_bwd" if inverse else "gmlm_rope_heads_d256_fwd"
    check(getattr(lib(), name)(_o._ptr(t), stride, _o._ptr(cos_sin), cos_sin.shape[0], tokens, int(seq_len), _o._ptr(pos_ids), heads, D,
                               _o._dt(t), _o._stream()), name)
    return t


class RopeSoftcapGQA256(torch.autograd.Function):
    """Rotary embedding (no head norm) and grouped-KV attention at head dim 256 of a fused [.., (hq + 2 hkv) * 256] projection
    output in one autograd node: the rotation runs in place on a COPY of the Q | K columns, V is read from the fused rows where
    it lies.  ``softcap`` given: the soft-capped kernels (``window`` 0 or a band); None: the kernels of ``RopeGQA256`` or, with a
    ``window``, of ``RopeGQABand256`` behind the same rotation.  Padded ([b, l, .] with ``kv_len``) or packed ([T, .] with
    ``pos_ids``, ``cu_seqlens``, ``max_len``).  The backward lets the attention kernels write dq | dk | dv into ONE fused buffer
    and rotates its Q | K columns back in place: a single data-gradient GEMM follows."""

    @staticmethod
    def forward(ctx, qkv, cs, kv_len, hq, hkv, scale, pos_ids, cu_seqlens, max_len, causal, softcap, window):
        window = int(window)
        if softcap is not None:
            softcap, window = _cap_args(softcap, window)
        elif window:
            window = _window_arg(window)
        _o._cuda(qkv)
        _table(cs)
        packed = cu_seqlens is not None
        if qkv.dim() != (2 if packed else 3) or qkv.shape[-1] != (hq + 2 * hkv) * D:
            raise ValueError("fused projection output must be [b, l, (hq + 2 hkv) * 256], or [tokens, (hq + 2 hkv) * 256] when packed")
        pos = _o._pos_arg(qkv, pos_ids) if packed else None
        seq_len = 0 if packed else qkv.shape[1]
        nq, nk = hq * D, hkv * D
        qk = rope_heads_d256_(qkv[..., :nq + nk].contiguous(), cs, hq + hkv, seq_len, pos)
        want_lo = qkv.dtype == torch.bfloat16 and qkv.requires_grad
        q, k, v = qk[..., :nq], qk[..., nq:], qkv[..., nq + nk:]
        if packed:
            s, max_len = _o._varlen_args(qkv, cu_seqlens, max_len)
        if softcap is not None or window:
            out, out_lo, lse = _band_fwd(q, k, v, kv_len, cu_seqlens, max_len, hq, hkv, scale, causal, window, want_lo, softcap)
        elif packed:
            out, out_lo, lse = _o._causal_varlen_fwd(q, k, v, cu_seqlens, s, max_len, hq, hkv, scale, want_lo, D, not causal)
        else:
            out, out_lo, lse = _o._causal_fwd(q, k, v, kv_len, hq, hkv, scale, want_lo, D, not causal)
        ctx.save_for_backward(qkv, qk, cs, out, lse, kv_len, cu_seqlens, pos, out_lo)
        ctx.cfg = (hq, hkv, float(scale), seq_len, int(max_len), bool(causal), softcap, window)
        return out

    @staticmethod
    def backward(ctx, gout):
        qkv, qk, cs, out, lse, kv_len, cu, pos, out_lo = ctx.saved_tensors
        hq, hkv, scale, seq_len, max_len, causal, softcap, window = ctx.cfg
        nq, nk = hq * D, hkv * D
        q, k, v = qk[..., :nq], qk[..., nq:], qkv[..., nq + nk:]
        dqkv = torch.empty_like(qkv, memory_format=torch.contiguous_format)
        dq, dk, dv = dqkv[..., :nq], dqkv[..., nq:nq + nk], dqkv[..., nq + nk:]
        if softcap is not None or window:
            _band_bwd(q, k, v, out, out_lo, gout, lse, kv_len, cu, max_len, hq, hkv, scale, causal, window, dq, dk, dv, softcap)
        elif cu is not None:
            _o._causal_varlen_bwd(q, k, v, out, out_lo, gout, lse, cu, cu.numel() - 1, max_len, hq, hkv, scale, dq, dk, dv, D, not causal)
        else:
            _o._causal_bwd(q, k, v, out, out_lo, gout, lse, kv_len, hq, hkv, scale, dq, dk, dv, D, not causal)
        rope_heads_d256_(dqkv, cs, hq + hkv, seq_len, pos, inverse=True)
        return (dqkv,) + (None,) * 11


def rope_softcap_gqa_d256(qkv, cos_sin, kv_len, hq, hkv, scale, causal, softcap, *, window=0):
    """Padded layout: ``qkv`` [b, l, (hq + 2 hkv) * 256] (positions 0..l-1), ``kv_len`` int32 [b] or None -> [b, l, hq * 256].
    ``softcap`` None: no cap.  ``window`` > 0: query i sees key j iff |i - j| < window (causal: 0 <= i - j < window)."""
    return RopeSoftcapGQA256.apply(qkv, cos_sin, kv_len, hq, hkv, scale, None, None, 0, causal, softcap, window)


def rope_softcap_gqa_d256_varlen(qkv, cos_sin, pos_ids, cu_seqlens, max_len, hq, hkv, scale, causal, softcap, *, window=0):
    """Packed layout: ``qkv`` [T, (hq + 2 hkv) * 256] rows at positions ``pos_ids``, sequences by ``cu_seqlens`` (none longer than
    ``max_len``) -> [T, hq * 256].  ``softcap`` and ``window`` as in ``rope_softcap_gqa_d256``."""
    return RopeSoftcapGQA256.apply(qkv, cos_sin, None, hq, hkv, scale, pos_ids, cu_seqlens, int(max_len), causal, softcap, window)
