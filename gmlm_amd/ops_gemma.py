"""The operators of the Gemma3 text encoder that are autograd nodes of their own (include/gmlm_hip_gqa_wide.h), re-exported by
ops.py as ``ops.sandwich_rmsnorm`` and ``ops.rope_gqa_d256`` / ``_varlen``: the sandwich RMSNorm pair (gmlm_sandwich_rmsnorm_*) and
head norm + rotary embedding + grouped-KV attention at head dim 256 (gmlm_qknorm_rope_d256_*, gmlm_attention_gqa_d256_*).  The
tanh-GELU gated unit is ``ops.geglu_tanh`` (the ``_GLU`` node) and attention alone is ``ops.CausalAttention`` /
``CausalAttentionVarlen`` at d = 256 (``gqa_d256_attention`` / ``_varlen`` below name the mask instead of its negation).
The band-limited (sliding-window) form of that attention (include/gmlm_hip_gqa_band.h, gmlm_attention_gqa_d256_band_*) has two
nodes of its own here: ``BandAttention256`` (``ops.gqa_d256_band_attention`` / ``_varlen``) and ``RopeGQABand256``, which
``rope_gqa_d256`` / ``_varlen`` run when their ``window`` keyword is not 0.
The soft-capped form (include/gmlm_hip_gqa_softcap.h) has its nodes in ops_softcap.py; ``_band_fwd`` / ``_band_bwd`` here make
its calls when given a ``softcap``.

Every node returns one gradient entry per input whatever is frozen, like the nodes of ops.py; their frozen-input tests are
tests/test_gpu_gemma_rowops.py, tests/test_gpu_gqa_wide_kernels.py and tests/test_gqa_band_cpu.py
(tests/test_autograd_contract_cpu.py files a builder for every node that ops.py itself defines).
"""
from __future__ import annotations

import torch

from . import ops as _o
from ._lib import check, lib

D = 256


class SandwichNorm(torch.autograd.Function):
    """(s', y):  s' = s + RMSNorm(b) * (w_offset + w_post) in the compute dtype (``s`` None: no residual),
    y = RMSNorm(s') * (w_offset + w_pre), the second statistic taken from the stored s'.  ``s'`` is the residual stream handed
    to the next pair; its gradient and y's meet in ONE backward kernel, which also yields both weight gradients."""

    @staticmethod
    def forward(ctx, s, b, w_post, w_pre, w_offset, eps):
        _o._cuda(b)
        shape = b.shape
        f = shape[-1]
        b2 = b.contiguous().view(-1, f)
        s2 = None if s is None else s.to(b.dtype).contiguous().view(-1, f)
        rows = b2.shape[0]
        wpo, wpr = _o._f32c(w_post), _o._f32c(w_pre)
        sp, y = torch.empty_like(b2), torch.empty_like(b2)
        stats = torch.empty(2, rows, dtype=torch.float32, device=b.device)              # rstd_b | rstd_s
        check(lib().gmlm_sandwich_rmsnorm_fwd(_o._ptr(s2), _o._ptr(b2), _o._ptr(wpo), _o._ptr(wpr), rows, f, float(w_offset), float(eps),
                                              _o._ptr(sp), _o._ptr(y), _o._ptr(stats[0]), _o._ptr(stats[1]), _o._dt(b2), _o._stream()),
              "gmlm_sandwich_rmsnorm_fwd")
        ctx.save_for_backward(b2, sp, wpo, wpr, stats)
        ctx.cfg = (shape, s is not None, float(w_offset))
        return sp.view(shape), y.view(shape)

    @staticmethod
    def backward(ctx, gs, gy):
        b2, sp, wpo, wpr, stats = ctx.saved_tensors
        shape, has_s, w_offset = ctx.cfg
        rows, f = b2.shape
        if gy is None:
            gy = torch.zeros_like(sp)
        gy2 = gy.contiguous().view(rows, f).to(sp.dtype)
        gs2 = None if gs is None else gs.contiguous().view(rows, f).to(sp.dtype)
        ds = torch.empty_like(sp) if has_s else None
        db = torch.empty_like(sp)
        dw = torch.empty(2, f, dtype=torch.float32, device=sp.device)                   # dw_post | dw_pre: one buffer
        ws = _o._ws(lib().gmlm_sandwich_rmsnorm_bwd_workspace_bytes(rows, f), sp.device)
        check(lib().gmlm_sandwich_rmsnorm_bwd(_o._ptr(gy2), _o._ptr(gs2), _o._ptr(b2), _o._ptr(sp), _o._ptr(wpo), _o._ptr(wpr),
                                              _o._ptr(stats[0]), _o._ptr(stats[1]), rows, f, w_offset, _o._ptr(ds), _o._ptr(db),
                                              _o._ptr(dw[0]), _o._ptr(dw[1]), _o._dt(sp), _o._ptr(ws), ws.numel(), _o._stream()),
              "gmlm_sandwich_rmsnorm_bwd")
        return (ds.view(shape) if has_s else None), db.view(shape), dw[0], dw[1], None, None


def sandwich_rmsnorm(s, b, w_post, w_pre, w_offset=1.0, eps=1e-6):
    """-> (s + RMSNorm(b) * (w_offset + w_post), RMSNorm(of that sum) * (w_offset + w_pre)); ``s`` may be None."""
    return SandwichNorm.apply(s, b, w_post, w_pre, w_offset, eps)


def gqa_d256_attention(q, k, v, kv_len, hq, hkv, scale, causal):
    """Grouped-KV attention at head dim 256, padded: q [b, l, hq * 256], k / v [b, l, hkv * 256] (strided slices of a fused buffer
    are fine), ``kv_len`` int32 [b] or None; ``scale`` multiplies the scores."""
    return _o.CausalAttention.apply(q, k, v, kv_len, hq, hkv, scale, D, not causal)


def gqa_d256_attention_varlen(q, k, v, cu_seqlens, max_len, hq, hkv, scale, causal):
    """The same on packed rows: q [T, hq * 256], k / v [T, hkv * 256], sequence i = rows [cu_seqlens[i], cu_seqlens[i + 1])."""
    return _o.CausalAttentionVarlen.apply(q, k, v, cu_seqlens, max_len, hq, hkv, scale, D, not causal, None)


# ---- the band-limited (sliding-window) form, include/gmlm_hip_gqa_band.h -------------------------------------------------------
# visible(i, j) = j < kv_len and (0 <= i - j < window if causal else |i - j| < window): HF's exclusive window, window >= 1
_BAND = "gmlm_attention_gqa_d256_band"
_CAP = "gmlm_attention_gqa_d256_softcap"      # include/gmlm_hip_gqa_softcap.h: the same with ``softcap`` after ``window`` (0: no band)


def _band_fwd(q, k, v, kv_len, cu, max_len, hq, hkv, scale, causal, window, want_lo, softcap=None):
    """Padded ([b, l, .] with ``kv_len``) or, with ``cu`` (int32 [S + 1]), packed ([T, .]) -> (out, out_lo, lse).  ``softcap``
    given: the soft-capped kernels, for which ``window`` may be 0."""
    base, cap = (_CAP, (float(softcap),)) if softcap is not None else (_BAND, ())
    if cu is not None:
        t = q.shape[0]
        qs, ks, vs = _o._packed_stride(q, hq, D), _o._packed_stride(k, hkv, D), _o._packed_stride(v, hkv, D)
        if k.shape[0] != t or v.shape[0] != t:
            raise ValueError("packed q, k and v must have the same number of rows")
        out = torch.empty(t, hq * D, dtype=q.dtype, device=q.device)
        lse = torch.empty(hq, t, dtype=torch.float32, device=q.device)
        head, name = (_o._ptr(cu), cu.numel() - 1, max_len, t), base + "_varlen_fwd"
    else:
        b, l = q.shape[0], q.shape[1]
        qs, ks, vs = _o._rows_view(q, hq, D), _o._rows_view(k, hkv, D), _o._rows_view(v, hkv, D)
        out = torch.empty(b, l, hq * D, dtype=q.dtype, device=q.device)
        lse = torch.empty(b, hq, l, dtype=torch.float32, device=q.device)
        head, name = (_o._ptr(kv_len), b), base + "_fwd"
    out_lo = torch.empty_like(out) if want_lo else None
    mid = () if cu is not None else (l, k.shape[1])
    check(getattr(lib(), name)(_o._ptr(q), _o._ptr(k), _o._ptr(v), *head, hq, hkv, *mid, D, qs, ks, vs, float(scale), 0.0, 1 if causal else 0,
                               int(window), *cap, _o._ptr(out), _o._ptr(out_lo), _o._ptr(lse), _o._dt(q), _o._stream()), name)
    return out, out_lo, lse


def _band_bwd(q, k, v, out, out_lo, gout, lse, kv_len, cu, max_len, hq, hkv, scale, causal, window, dq, dk, dv, softcap=None):
    base, cap = (_CAP, (float(softcap),)) if softcap is not None else (_BAND, ())
    gout = gout.contiguous().to(q.dtype)
    if cu is not None:
        t = q.shape[0]
        ws = _o._ws(getattr(lib(), base + "_varlen_bwd_workspace_bytes")(t, hq), q.device)
        head, mid, name, r = (_o._ptr(cu), cu.numel() - 1, max_len, t), (), base + "_varlen_bwd", 0
    else:
        b, l = q.shape[0], q.shape[1]
        ws = _o._ws(getattr(lib(), base + "_bwd_workspace_bytes")(b, hq, l), q.device)
        head, mid, name, r = (_o._ptr(kv_len), b), (l, k.shape[1]), base + "_bwd", 1
    check(getattr(lib(), name)(_o._ptr(q), _o._ptr(k), _o._ptr(v), _o._ptr(out), _o._ptr(out_lo), _o._ptr(gout), _o._ptr(lse), *head, hq, hkv,
                               *mid, D, q.stride(r), k.stride(r), v.stride(r), float(scale), 0.0, 1 if causal else 0, int(window),
                               *cap, _o._ptr(dq), _o._ptr(dk), _o._ptr(dv), dq.stride(r), dk.stride(r), dv.stride(r), _o._dt(q), _o._ptr(ws),
                               ws.numel(), _o._stream()), name)


def _window_arg(window):
    window = int(window)
    if not 1 <= window < 1 << 30:
        raise ValueError(f"window must be in [1, 2^30), got {window}")
    return window


class BandAttention256(torch.autograd.Function):
    """Band-limited grouped-KV attention at head dim 256 (gmlm_attention_gqa_d256_band_*): query i sees key j of its sequence iff
    j < kv_len and 0 <= i - j < ``window`` (``causal``) or |i - j| < ``window``.  Padded (q [b, l, hq * 256], k / v [b, l, hkv * 256],
    ``kv_len``) or, with ``cu_seqlens``, packed ([T, .]); strided slices of a fused buffer are fine.  A query without a visible
    key gives a zero row (``lse``, the node's fifth saved tensor, is -inf there).  The three gradients are views of ONE fused buffer;
    one entry per input whatever is frozen."""

    @staticmethod
    def forward(ctx, q, k, v, kv_len, cu_seqlens, max_len, hq, hkv, scale, causal, window):
        window = _window_arg(window)
        _o._cuda(q, k, v)
        if cu_seqlens is not None:
            _, max_len = _o._varlen_args(q, cu_seqlens, max_len)
        want_lo = q.dtype == torch.bfloat16 and any(t.requires_grad for t in (q, k, v))
        out, out_lo, lse = _band_fwd(q, k, v, kv_len, cu_seqlens, max_len, hq, hkv, scale, causal, window, want_lo)
        ctx.save_for_backward(q, k, v, out, lse, kv_len, cu_seqlens, out_lo)
        ctx.cfg = (int(max_len), hq, hkv, float(scale), bool(causal), window)
        return out

    @staticmethod
    def backward(ctx, gout):
        q, k, v, out, lse, kv_len, cu, out_lo = ctx.saved_tensors
        max_len, hq, hkv, scale, causal, window = ctx.cfg
        nq, nk = hq * D, hkv * D
        dqkv = torch.empty(*q.shape[:-1], nq + 2 * nk, dtype=q.dtype, device=q.device)
        dq, dk, dv = dqkv[..., :nq], dqkv[..., nq:nq + nk], dqkv[..., nq + nk:]
        _band_bwd(q, k, v, out, out_lo, gout, lse, kv_len, cu, max_len, hq, hkv, scale, causal, window, dq, dk, dv)
        return (dq, dk, dv) + (None,) * 8


def gqa_d256_band_attention(q, k, v, kv_len, hq, hkv, scale, causal, window):
    """``gqa_d256_attention`` with the band |i - j| < ``window`` (causal: 0 <= i - j < ``window``) added to the mask."""
    return BandAttention256.apply(q, k, v, kv_len, None, 0, hq, hkv, scale, causal, window)


def gqa_d256_band_attention_varlen(q, k, v, cu_seqlens, max_len, hq, hkv, scale, causal, window):
    """The same on packed rows: sequence i = rows [cu_seqlens[i], cu_seqlens[i + 1])."""
    return BandAttention256.apply(q, k, v, None, cu_seqlens, int(max_len), hq, hkv, scale, causal, window)


def _table(cs):
    if cs.dtype != torch.float32 or cs.dim() != 3 or tuple(cs.shape[1:]) != (2, D // 2) or not cs.is_contiguous():
        raise ValueError(f"cos / sin table must be a contiguous fp32 [max_len, 2, {D // 2}] tensor")


def qknorm_rope_d256(qkv, qw, kw, cs, hq, hkv, w_offset, eps, pos_ids=None, out=None):
    """Outside autograd: head norm + rotation of the Q | K head rows of fused [.., >= (hq + 2 hkv) * 256] rows -> (out, rstd).
    ``out`` None: a new [.., (hq + hkv) * 256] buffer; ``out`` = ``qkv``: in place, the V columns are not written.  Positions are
    row % (rows per sequence), or ``pos_ids`` (int32 [tokens]) when given."""
    _table(cs)
    n = (hq + hkv) * D
    tokens, stride = _o._qkv_rows(qkv, (hq + 2 * hkv) * D)
    if out is None:
        out = torch.empty(*qkv.shape[:-1], n, dtype=qkv.dtype, device=qkv.device)
    _, ostride = _o._qkv_rows(out, n)
    rstd = torch.empty(tokens, hq + hkv, dtype=torch.float32, device=qkv.device)
    head = (_o._ptr(qkv), stride, _o._ptr(qw), _o._ptr(kw), _o._ptr(cs), cs.shape[0], tokens)
    tail = (hq, hkv, D, float(w_offset), float(eps), _o._ptr(out), ostride, _o._ptr(rstd), _o._dt(qkv), _o._stream())
    if pos_ids is not None:
        check(lib().gmlm_qknorm_rope_d256_pos_fwd(*head, _o._ptr(pos_ids), *tail), "gmlm_qknorm_rope_d256_pos_fwd")
    else:
        check(lib().gmlm_qknorm_rope_d256_fwd(*head, qkv.shape[-2], *tail), "gmlm_qknorm_rope_d256_fwd")
    return out, rstd


def qknorm_rope_d256_bwd_(dqkv, qkv, qw, kw, cs, rstd, hq, hkv, w_offset, pos_ids=None):
    """In place on the Q | K columns of ``dqkv``; ``qkv`` is what the forward read; returns the fp32 [2, 256] weight gradients."""
    tokens, stride = _o._qkv_rows(qkv, (hq + 2 * hkv) * D)
    _, dstride = _o._qkv_rows(dqkv, (hq + hkv) * D)
    dwt = torch.empty(2, D, dtype=torch.float32, device=qkv.device)
    ws = _o._ws(lib().gmlm_qknorm_rope_d256_bwd_workspace_bytes(tokens, hq, hkv, _o._dt(qkv)), qkv.device)
    head = (_o._ptr(dqkv), dstride, _o._ptr(qkv), stride, _o._ptr(qw), _o._ptr(kw), _o._ptr(cs), cs.shape[0], _o._ptr(rstd), tokens)
    tail = (hq, hkv, D, float(w_offset), _o._ptr(dwt), _o._ptr(dwt[1]), _o._dt(qkv), _o._ptr(ws), ws.numel(), _o._stream())
    if pos_ids is not None:
        check(lib().gmlm_qknorm_rope_d256_pos_bwd(*head, _o._ptr(pos_ids), *tail), "gmlm_qknorm_rope_d256_pos_bwd")
    else:
        check(lib().gmlm_qknorm_rope_d256_bwd(*head, qkv.shape[-2], *tail), "gmlm_qknorm_rope_d256_bwd")
    return dwt


class RopeGQA256(torch.autograd.Function):
    """Per-head RMSNorm of Q / K with weight ``w_offset + w``, rotary embedding and grouped-KV attention at head dim 256 of a
    fused [.., (hq + 2 hkv) * 256] projection output in one autograd node, ``causal`` or bidirectional.  Padded ([b, l, .] with
    ``kv_len``) or packed ([T, .] with ``pos_ids``, ``cu_seqlens``, ``max_len``).  V is read from the fused rows in place; the
    backward lets the attention kernels write dq | dk | dv into ONE fused buffer, which the head-norm backward then finishes
    in place: a single data-gradient GEMM follows."""

    @staticmethod
    def forward(ctx, qkv, qw, kw, cs, kv_len, hq, hkv, scale, w_offset, eps, pos_ids, cu_seqlens, max_len, causal):
        _o._cuda(qkv)
        _table(cs)
        packed = cu_seqlens is not None
        if qkv.dim() != (2 if packed else 3) or qkv.shape[-1] != (hq + 2 * hkv) * D:
            raise ValueError("fused projection output must be [b, l, (hq + 2 hkv) * 256], or [tokens, (hq + 2 hkv) * 256] when packed")
        qwf, kwf = _o._f32c(qw), _o._f32c(kw)
        pos = _o._pos_arg(qkv, pos_ids) if packed else None
        nq, nk = hq * D, hkv * D
        qk, rstd = qknorm_rope_d256(qkv, qwf, kwf, cs, hq, hkv, w_offset, eps, pos)
        want_lo = qkv.dtype == torch.bfloat16 and (qkv.requires_grad or qw.requires_grad or kw.requires_grad)
        q, k, v = qk[..., :nq], qk[..., nq:], qkv[..., nq + nk:]
        if packed:
            s, max_len = _o._varlen_args(qkv, cu_seqlens, max_len)
            out, out_lo, lse = _o._causal_varlen_fwd(q, k, v, cu_seqlens, s, max_len, hq, hkv, scale, want_lo, D, not causal)
        else:
            out, out_lo, lse = _o._causal_fwd(q, k, v, kv_len, hq, hkv, scale, want_lo, D, not causal)
        ctx.save_for_backward(qkv, qk, qwf, kwf, cs, rstd, out, lse, kv_len, cu_seqlens, pos, out_lo)
        ctx.cfg = (hq, hkv, float(scale), float(w_offset), int(max_len), bool(causal))
        return out

    @staticmethod
    def backward(ctx, gout):
        qkv, qk, qwf, kwf, cs, rstd, out, lse, kv_len, cu, pos, out_lo = ctx.saved_tensors
        hq, hkv, scale, w_offset, max_len, causal = ctx.cfg
        nq, nk = hq * D, hkv * D
        q, k, v = qk[..., :nq], qk[..., nq:], qkv[..., nq + nk:]
        dqkv = torch.empty_like(qkv, memory_format=torch.contiguous_format)
        dq, dk, dv = dqkv[..., :nq], dqkv[..., nq:nq + nk], dqkv[..., nq + nk:]
        if cu is not None:
            _o._causal_varlen_bwd(q, k, v, out, out_lo, gout, lse, cu, cu.numel() - 1, max_len, hq, hkv, scale, dq, dk, dv, D, not causal)
        else:
            _o._causal_bwd(q, k, v, out, out_lo, gout, lse, kv_len, hq, hkv, scale, dq, dk, dv, D, not causal)
        dwt = qknorm_rope_d256_bwd_(dqkv, qkv, qwf, kwf, cs, rstd, hq, hkv, w_offset, pos)
        return (dqkv, dwt[0], dwt[1]) + (None,) * 11


class RopeGQABand256(torch.autograd.Function):
    """``RopeGQA256`` with the band-limited attention kernels: the same head norm, rotation, layouts and single fused ``dqkv``,
    and a trailing ``window`` (>= 1)."""

    @staticmethod
    def forward(ctx, qkv, qw, kw, cs, kv_len, hq, hkv, scale, w_offset, eps, pos_ids, cu_seqlens, max_len, causal, window):
        window = _window_arg(window)
        _o._cuda(qkv)
        _table(cs)
        packed = cu_seqlens is not None
        if qkv.dim() != (2 if packed else 3) or qkv.shape[-1] != (hq + 2 * hkv) * D:
            raise ValueError("fused projection output must be [b, l, (hq + 2 hkv) * 256], or [tokens, (hq + 2 hkv) * 256] when packed")
        qwf, kwf = _o._f32c(qw), _o._f32c(kw)
        pos = _o._pos_arg(qkv, pos_ids) if packed else None
        nq, nk = hq * D, hkv * D
        qk, rstd = qknorm_rope_d256(qkv, qwf, kwf, cs, hq, hkv, w_offset, eps, pos)
        want_lo = qkv.dtype == torch.bfloat16 and (qkv.requires_grad or qw.requires_grad or kw.requires_grad)
        if packed:
            _, max_len = _o._varlen_args(qkv, cu_seqlens, max_len)
        out, out_lo, lse = _band_fwd(qk[..., :nq], qk[..., nq:], qkv[..., nq + nk:], kv_len, cu_seqlens, max_len, hq, hkv, scale, causal,
                                     window, want_lo)
        ctx.save_for_backward(qkv, qk, qwf, kwf, cs, rstd, out, lse, kv_len, cu_seqlens, pos, out_lo)
        ctx.cfg = (hq, hkv, float(scale), float(w_offset), int(max_len), bool(causal), window)
        return out

    @staticmethod
    def backward(ctx, gout):
        qkv, qk, qwf, kwf, cs, rstd, out, lse, kv_len, cu, pos, out_lo = ctx.saved_tensors
        hq, hkv, scale, w_offset, max_len, causal, window = ctx.cfg
        nq, nk = hq * D, hkv * D
        dqkv = torch.empty_like(qkv, memory_format=torch.contiguous_format)
        _band_bwd(qk[..., :nq], qk[..., nq:], qkv[..., nq + nk:], out, out_lo, gout, lse, kv_len, cu, max_len, hq, hkv, scale, causal, window,
                  dqkv[..., :nq], dqkv[..., nq:nq + nk], dqkv[..., nq + nk:])
        dwt = qknorm_rope_d256_bwd_(dqkv, qkv, qwf, kwf, cs, rstd, hq, hkv, w_offset, pos)
        return (dqkv, dwt[0], dwt[1]) + (None,) * 12


def rope_gqa_d256(qkv, q_weight, k_weight, cos_sin, kv_len, hq, hkv, scale, causal, w_offset=1.0, eps=1e-6, *, window=0):
    """Padded layout: ``qkv`` [b, l, (hq + 2 hkv) * 256] (positions 0..l-1), ``kv_len`` int32 [b] or None -> [b, l, hq * 256].
    ``window`` > 0: the band-limited kernels (query i sees key j iff |i - j| < window, causal: 0 <= i - j < window)."""
    if window:
        return RopeGQABand256.apply(qkv, q_weight, k_weight, cos_sin, kv_len, hq, hkv, scale, w_offset, eps, None, None, 0, causal, window)
    return RopeGQA256.apply(qkv, q_weight, k_weight, cos_sin, kv_len, hq, hkv, scale, w_offset, eps, None, None, 0, causal)


def rope_gqa_d256_varlen(qkv, q_weight, k_weight, cos_sin, pos_ids, cu_seqlens, max_len, hq, hkv, scale, causal, w_offset=1.0, eps=1e-6, *,
                         window=0):
    """Packed layout: ``qkv`` [T, (hq + 2 hkv) * 256] rows at positions ``pos_ids``, sequences by ``cu_seqlens`` (none longer than
    ``max_len``) -> [T, hq * 256].  ``window`` as in ``rope_gqa_d256``."""
    if window:
        return RopeGQABand256.apply(qkv, q_weight, k_weight, cos_sin, None, hq, hkv, scale, w_offset, eps, pos_ids, cu_seqlens, int(max_len),
                                    causal, window)
    return RopeGQA256.apply(qkv, q_weight, k_weight, cos_sin, None, hq, hkv, scale, w_offset, eps, pos_ids, cu_seqlens, int(max_len),
                            causal)
