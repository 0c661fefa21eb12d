"""The dense-layer path: compute-dtype GEMM operands packed into one flat buffer, the GEMMs themselves (hipBLASLt through
torch, or the three-product bf16 form of gemm_precision "bf16x3"), the split-K weight gradient, and the routing of fp32 weight /
bias gradients to the master parameters.  The kernels it calls are wrapped in gmlm_amd.ops (``split_bf16x3``, ``wgrad_bf16``,
``column_sum``); nn.py, bert.py, qwen3.py and model.py build their layers on what is here.
"""
from __future__ import annotations

import math

import torch
import torch.nn.functional as F

from . import ops
from ._lib import GmlmHipError

GEMM_PRECISIONS = ("native", "bf16x3")


def check_gemm_precision(gemm_precision, cd=None) -> None:
    """ValueError for an unknown mode, or for "bf16x3" with a compute dtype ``cd`` other than float32."""
    if gemm_precision not in GEMM_PRECISIONS:
        raise ValueError(f"gemm_precision must be one of {GEMM_PRECISIONS}, got {gemm_precision!r}")
    if gemm_precision == "bf16x3" and cd is not None and cd != torch.float32:
        raise ValueError("gemm_precision='bf16x3' keeps fp32 storage: the compute dtype must be float32")


# ---------------------------------------------------------------------------------------------
# fp32 result straight out of a GEMM with 16-bit operands
# ---------------------------------------------------------------------------------------------
_F32_OUT_REFUSED = set()   # (op, device type) for which this torch refused out_dtype=float32 (found on first use, then kept)


def _f32_out(op, *args, **kw):
    """``torch.<op>(*args, out_dtype=torch.float32)`` for op "mm" | "bmm" | "addmm", or None where this torch refuses it."""
    key = (op, args[-1].device.type)
    if key not in _F32_OUT_REFUSED:
        try:
            return getattr(torch, op)(*args, out_dtype=torch.float32, **kw)
        except (RuntimeError, TypeError):
            _F32_OUT_REFUSED.add(key)
    return None


def _mm_f32(a, b):
    """a [N, K] @ b [P, K]^T with an fp32 result straight out of the GEMM when the operands are 16-bit."""
    out = _f32_out("mm", a, b.t()) if a.dtype != torch.float32 else None
    return (a @ b.t()).float() if out is None else out


# ---------------------------------------------------------------------------------------------
# split-K weight gradient
# ---------------------------------------------------------------------------------------------
_SLICES_MEASURED = {(2304, 768): 14, (3072, 768): 14, (768, 3072): 14}
SPLITK_ROW_QUANTUM = 112   # lcm(14, 16): a token count that is a multiple of it leaves no tail rows for either slice count
# bf16 -> fp32 weight gradients at T >= NATIVE_WGRAD_MIN_T with N, K multiples of 256 and at least NATIVE_WGRAD_MIN_TILES
# 256 x 256 output tiles run on the split-K kernel of libgmlm_hip.so (wgrad_kernels.hip) instead of the batched hipBLASLt
# GEMM + ATen slice sum (MI355X, T = 91,712, tools/ubench/wgrad_native.py: 1.2-1.4x on every BERT-base weight).  The
# BERT-mini weights (1-4 tiles) stay on the library path: alone 1.3x except 256 x 256 (90 vs 50 us), but the chameleon
# whole-step graph, where they share the chip with the GNN branch, measured 6.41-6.44 vs 6.33 ms.  False = library path (A/B).
# These three are read here at call time: set them as dense.NATIVE_WGRAD*, a copy imported elsewhere switches nothing.
NATIVE_WGRAD = True
NATIVE_WGRAD_MIN_T = 16384
NATIVE_WGRAD_MIN_TILES = 9


def _native_wgrad_ok(dy2: torch.Tensor, x2: torch.Tensor, keep_fp32: bool) -> bool:
    t, n = dy2.shape
    k = x2.shape[1]
    return (NATIVE_WGRAD and keep_fp32 and dy2.is_cuda and dy2.dtype == torch.bfloat16 and x2.dtype == torch.bfloat16
            and t >= NATIVE_WGRAD_MIN_T and n % ops.WGRAD_TILE == 0 and k % ops.WGRAD_TILE == 0
            and (n // ops.WGRAD_TILE) * (k // ops.WGRAD_TILE) >= NATIVE_WGRAD_MIN_TILES
            and dy2.stride(1) == 1 and x2.stride(1) == 1 and dy2.stride(0) % 8 == 0 and x2.stride(0) % 8 == 0
            and dy2.data_ptr() % 16 == 0 and x2.data_ptr() % 16 == 0)


def _splitk_wgrad(dy2: torch.Tensor, x2: torch.Tensor, keep_fp32: bool = False) -> torch.Tensor:
    """dW [N, K] = dy2^T [N, T] @ x2 [T, K] (returned in fp32 when ``keep_fp32``, else in dy2's dtype).  The reduction dim is the token count (10^4..10^5) while the
    output is only a few 256x256 tiles, so one hipBLASLt call leaves most CUs idle; cutting T into S
    slices (batched GEMM, fp32 partials) and adding them fills the chip (measured 1.5-2.7x on MI355X)."""
    if _native_wgrad_ok(dy2, x2, keep_fp32):
        return ops.wgrad_bf16(dy2, x2)
    t, n = dy2.shape
    k = x2.shape[1]
    tiles = ((n + 255) // 256) * ((k + 255) // 256)
    s = 1
    if tiles < 128 and t >= 16384:                    # (node-level layers, t = a few thousand rows: one GEMM; slicing them left a tail GEMM + an add per weight)
        # measured on MI355X (tools/ubench/wgrad_shapes.py, T = 91,712): 16 slices is within 5 % of the best power of two for every
        # BERT shape once T >= 64k; 14 fills the chip better for three of the four BERT-base weights (QKV 322 vs 415 us, FFN
        # 440 vs 455 and 444 vs 447 us; the 768 x 768 output projection stays at 16: 128 vs 161 us)
        s = _SLICES_MEASURED.get((n, k), 16) if t >= 65536 else min(16, max(1, 2 ** round(math.log2(200.0 / tiles))))
    f32_out = dy2.dtype != torch.float32                  # 16-bit operands: ask the GEMM for the fp32 result, no cast pass over dW
    if s == 1:
        dw = _f32_out("mm", dy2.t(), x2) if keep_fp32 and f32_out else None
        if dw is not None:
            return dw
        dw = dy2.t() @ x2
        return dw.float() if keep_fp32 else dw
    # a packed batch has an arbitrary token count: S equal slices of floor(T/S) rows + a tail of < S rows
    q = t // s
    a = dy2[:s * q].view(s, q, n).transpose(1, 2)
    b = x2[:s * q].view(s, q, k)
    dw = _f32_out("bmm", a, b) if f32_out else None
    dw = (torch.bmm(a, b).float() if dw is None else dw).sum(0)
    if s * q < t:
        dw += dy2[s * q:].t() @ x2[s * q:]         # < S rows: one tiny GEMM, added in fp32
    return dw if keep_fp32 else dw.to(dy2.dtype)


# ---------------------------------------------------------------------------------------------
# the GEMMs, with fp32 gradients to the master parameters
# ---------------------------------------------------------------------------------------------
def _note_masters(ctx, masters, bc, bias_grad) -> None:
    """``masters`` = the weight(s) whose rows stack up to the operand, then (``bias_grad`` and a bias operand) the bias(es)
    stacking up to ``bc``."""
    ctx.masters = masters
    ctx.has_bias = bc is not None and bias_grad
    ctx.n_w = len(masters) // 2 if ctx.has_bias else len(masters)


def _master_grads(ctx, dw, db, need):
    """The stacked fp32 gradients ``dw`` [rows, K] / ``db`` [rows] (None = not formed) cut by master rows and cast to each
    master's dtype; ``need`` = ``ctx.needs_input_grad`` of the masters."""
    masters, n_w = ctx.masters, ctx.n_w
    grads = [None] * len(masters)
    for lo, hi, stacked in ((0, n_w, dw), (n_w, len(masters), db)):
        if stacked is not None:
            for i, g in zip(range(lo, hi), stacked.split([m.shape[0] for m in masters[lo:hi]], 0)):
                if need[i]:
                    grads[i] = g if g.dtype == masters[i].dtype else g.to(masters[i].dtype)
    return grads


class _Linear(torch.autograd.Function):
    """y = x @ wc^T (+ bc) on hipBLASLt with the cached compute-dtype operands ``wc`` / ``bc``; the gradients go
    to the fp32 MASTER parameters (``masters`` = the weight(s) whose rows stack up to ``wc``, then the bias(es)
    stacking up to ``bc``): split-K weight gradient and the bias column sum stay in fp32 end to end.
    With ``residual`` the input is also returned as a second output for the residual branch, so that the two
    gradients of ``x`` meet HERE and the data-gradient GEMM accumulates onto the residual one (beta = 1 in the
    GEMM epilogue) instead of autograd running a separate add kernel."""

    @staticmethod
    def forward(ctx, x, wc, bc, residual, bias_grad, *masters):
        """``bias_grad`` False: ``bc`` is added but its masters are not among ``masters`` (their gradient is produced
        elsewhere: ops.AttentionQKV returns the fused QKV bias gradient itself, from inside its backward kernel)."""
        ctx.save_for_backward(x, wc)
        _note_masters(ctx, masters, bc, bias_grad)
        y = F.linear(x, wc, bc)
        return (y, x.view_as(x)) if residual else y

    @staticmethod
    def backward(ctx, dy, dxres=None):
        x, wc = ctx.saved_tensors
        dy2 = dy.reshape(-1, dy.shape[-1])
        x2 = x.reshape(-1, x.shape[-1])
        dx = None
        if ctx.needs_input_grad[0]:
            if dxres is None:
                dx = (dy2 @ wc).view(x.shape)
            else:
                # the residual gradient buffer is ours alone (it was produced for this node): accumulate in place
                dres2 = dxres.reshape(-1, x.shape[-1])
                dx = (dres2.addmm_(dy2, wc) if dres2.is_contiguous() else torch.addmm(dres2, dy2, wc)).view(x.shape)
        need = ctx.needs_input_grad[5:]
        dw = db = None
        if any(need[:ctx.n_w]):
            dw = _splitk_wgrad(dy2, x2, keep_fp32=True)
        if ctx.has_bias and any(need[ctx.n_w:]):
            db = ops.column_sum(dy2) if dy2.is_cuda and dy2.dtype in (torch.float32, torch.bfloat16) else dy2.sum(0, dtype=torch.float32)
        return (dx, None, None, None, None, *_master_grads(ctx, dw, db, need))


class SplitWeight:
    """The two bf16x3 forms of one fp32 weight ``w`` [N, K], split once and used by every call of a step: ``w0`` [N, 3 K'] =
    (hi, lo, hi) side by side for the forward GEMM, ``w1s`` [3 N', K'] = (hi, hi, lo) stacked for the data-gradient GEMM
    (K', N' = K, N rounded up to 8; the pad rows and columns are zeros)."""
    __slots__ = ("w0", "w1s", "n", "k")

    def __init__(self, w: torch.Tensor):
        with torch.no_grad():
            w = w.detach()
            self.n, self.k = w.shape
            self.w0 = ops.split_bf16x3(w, 0)
            self.w1s = ops.split_bf16x3(w, 1, stacked=True, part_rows=ops._up8(self.n))

    @property
    def shape(self):
        return (self.n, self.k)


def _mm_bf16_f32(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """bf16 a @ b with the fp32 result straight out of the GEMM.  No fallback: a bf16 GEMM output would round away everything
    the three-product form gains."""
    out = _f32_out("mm", a, b)
    if out is None:
        raise GmlmHipError("gemm_precision='bf16x3' needs torch.mm(..., out_dtype=torch.float32) (bf16 operands, fp32 "
                           "result); this PyTorch does not have it")
    return out


class LinearBf16x3(torch.autograd.Function):
    """y = x @ w^T (+ bc) for fp32 ``x`` [..., K] and a ``SplitWeight`` of the fp32 weight [N, K], every GEMM on the bf16 matrix
    pipe with fp32 accumulation and an fp32 result; the interface and the gradient routing are those of ``_Linear``
    (``masters``, ``residual``, ``bias_grad``).
      forward          X1 = split(x, hi hi lo) [T, 3K'];  y = X1 @ w0^T
      data gradient    DY0 = split(dy, hi lo hi) [T, 3N'];  dx = DY0 @ w1s
      weight gradient  no further split: the contiguous [T, 3N'] / [T, 3K'] buffers viewed as [3T, N'] / [3T, K'] pair their
                       rows (hi, lo, hi) against (hi, hi, lo);  dW = DY0.view(3T, N')^T @ X1.view(3T, K') (split-K kernel K11
                       when 3T >= 16,384 and N', K' are multiples of 256, else the library)
    X1 (6 bytes per element) is what is saved for backward, not x."""

    @staticmethod
    def forward(ctx, x, sw, bc, residual, bias_grad, *masters):
        if x.dtype != torch.float32:
            raise TypeError(f"bf16x3 dense layers take float32 activations, got {x.dtype}")
        x2 = x.reshape(-1, x.shape[-1])
        if x2.shape[1] != sw.k:
            raise ValueError(f"bf16x3 linear: input width {x2.shape[1]} != weight width {sw.k}")
        x1 = ops.split_bf16x3(x2, 1)
        y = _mm_bf16_f32(x1, sw.w0.t())
        if bc is not None:
            y.add_(bc)
        ctx.save_for_backward(x1, sw.w1s)
        ctx.n, ctx.k, ctx.xshape = sw.n, sw.k, x.shape
        _note_masters(ctx, masters, bc, bias_grad)
        y = y.view(*x.shape[:-1], sw.n)
        return (y, x.view_as(x)) if residual else y

    @staticmethod
    def backward(ctx, dy, dxres=None):
        x1, w1s = ctx.saved_tensors
        n_w, n, k = ctx.n_w, ctx.n, ctx.k
        dy2 = dy.reshape(-1, n)
        need = ctx.needs_input_grad[5:]
        dy0 = ops.split_bf16x3(dy2, 0) if (ctx.needs_input_grad[0] or any(need[:n_w])) else None
        dx = None
        if ctx.needs_input_grad[0]:
            dres2 = None if dxres is None else dxres.reshape(-1, k)
            if dres2 is not None and dres2.is_contiguous() and w1s.shape[1] == k:
                # the residual gradient buffer is ours alone (it was produced for this node): accumulate in the GEMM epilogue
                dx = _f32_out("addmm", dres2, dy0, w1s, out=dres2)
            if dx is None:
                dx = _mm_bf16_f32(dy0, w1s)
                if dx.shape[1] != k:
                    dx = dx[:, :k]
                if dres2 is not None:
                    dx = dres2.add_(dx) if dres2.is_contiguous() else dres2 + dx
            dx = dx.reshape(ctx.xshape)
        dw = db = None
        if any(need[:n_w]):
            t = x1.shape[0]
            dw = _splitk_wgrad(dy0.view(3 * t, -1), x1.view(3 * t, -1), keep_fp32=True)     # [N', K']
            if not _F32_OUT_REFUSED.isdisjoint({("mm", dy0.device.type), ("bmm", dy0.device.type)}):
                # that function falls back to a bf16 GEMM output where the library refuses the fp32 one: fine for bf16 operands
                # of the bf16 path, but here it would round away what the three-product form gains
                raise GmlmHipError("gemm_precision='bf16x3': the GEMM library refused an fp32 result from bf16 operands")
            if dw.shape != (n, k):
                dw = dw[:n, :k]
        if ctx.has_bias and any(need[n_w:]):
            db = ops.column_sum(dy2)
        return (dx, None, None, None, None, *_master_grads(ctx, dw, db, need))


def _mm(x, wc, bc, masters, residual=False, bias_grad=True):
    """``wc``: the compute-dtype copy of the weight, or its ``SplitWeight`` (gemm_precision "bf16x3": the operand itself says
    which GEMM runs, so a checkpoint recompute that is handed the same operands takes the same path)."""
    with torch.autocast("cuda", enabled=False):
        fn = LinearBf16x3 if isinstance(wc, SplitWeight) else _Linear
        return fn.apply(x, wc, bc, residual, bias_grad, *masters)


def mm_bf16x3(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """a [M, K] @ b [N, K]^T in fp32 from two fp32 matrices on the bf16 matrix pipe (three-product form: relative error
    ~ 3 * 2^-16 per entry against 2^-8.5 for plain bf16 operands); differentiable in both."""
    with torch.autocast("cuda", enabled=False):
        return LinearBf16x3.apply(a, SplitWeight(b), None, False, True, b)


# ---------------------------------------------------------------------------------------------
# Compute-dtype copies of fp32 master parameters: ONE flat buffer, ONE multi-tensor copy
# ---------------------------------------------------------------------------------------------
def pack_operands(specs, dtype, device, zero_fill=False):
    """``specs``: list of (key, [master tensors stacked along dim 0], pad_rows).  Each entry becomes one contiguous
    [sum(rows) + pad_rows, ...] view, in the order given, of ONE flat buffer in ``dtype`` with every operand 256-byte aligned
    (its slot rounded up to 128 elements), filled by ONE ``_foreach_copy_`` instead of a cast kernel per parameter.
    ``zero_fill``: the pad rows (and the slack between slots) read zero; otherwise ``pad_rows`` must be 0.
    Returns (flat buffer, {key: view}); the views carry no autograd history."""
    total, plan = 0, []
    for key, masters, pad in specs:
        shape = (sum(m.shape[0] for m in masters) + pad,) + tuple(masters[0].shape[1:])
        numel = math.prod(shape)
        plan.append((key, masters, shape, total, numel))
        total += (numel + 127) // 128 * 128
    with torch.no_grad():
        flat = (torch.zeros if zero_fill else torch.empty)(total, dtype=dtype, device=device)
        views, dsts, srcs = {}, [], []
        for key, masters, shape, off, numel in plan:
            v = views[key] = flat[off:off + numel].view(shape)
            r0 = 0
            for m in masters:
                dsts.append(v if m.shape[0] == shape[0] else v[r0:r0 + m.shape[0]])
                srcs.append(m.detach())
                r0 += m.shape[0]
        if dsts:
            torch._foreach_copy_(dsts, srcs)
    return flat, views


def encoder_operands(specs, cd, gemm_precision="native"):
    """{key: GEMM operand} of a text encoder's layers for one forward (bert / qwen3 ``prepare_weights``): ``pack_operands``
    in the compute dtype on the masters' device; with ``gemm_precision`` "bf16x3" (fp32 only) every 2-D entry is then split
    once, for all micro-batches, into its ``SplitWeight``, and ``_mm`` picks the GEMM by the operand's type."""
    check_gemm_precision(gemm_precision, cd)
    views = pack_operands(specs, cd, specs[0][1][0].device if specs else None)[1]
    if gemm_precision == "bf16x3":
        for key, v in views.items():
            if v.dim() == 2:
                views[key] = SplitWeight(v)
    return views


class ParamShadow:
    """bf16 operands of a region's dense layers: ``pack_operands(specs, ...)`` with a zero-initialised buffer (the pad
    rows stay zero: the first RGCN layer's root is padded to the 16-byte-aligned input width).  The layers hand their weight /
    bias gradients straight to the fp32 masters (``_Linear``), so no cast kernels run in backward either."""

    def __init__(self, specs, dtype, device):
        self.dtype = dtype
        self.flat, self.views = pack_operands(specs, dtype, device, zero_fill=True)

    def get(self, key):
        return self.views.get(key)

    def record_stream(self, stream) -> None:
        """The operands are also read by kernels on ``stream`` (a branch of a recorded step): keep the allocator from recycling
        the buffer on its own stream while that branch still runs."""
        if self.flat.is_cuda:
            self.flat.record_stream(stream)


class SplitShadow:
    """The shadow of an fp32 region in gemm_precision "bf16x3": every 2-D entry of ``specs`` (a weight, or several stacked along
    dim 0) as a ``SplitWeight``, split ONCE per region call; every 1-D entry (a bias) as its fp32 values.  Looked up by the
    same keys as ``ParamShadow`` and re-entered by a checkpoint recompute through ``use_shadow``.  The caller lists only the
    parameters of layers that go through ``_linear`` / ``_mm``: what is not listed stays on the native fp32 path."""
    dtype = torch.float32

    def __init__(self, specs, device):
        self.views = {}
        with torch.no_grad():
            for key, masters, pad in specs:
                if pad:
                    raise ValueError("bf16x3 shadow entries take no pad rows")
                w = masters[0].detach() if len(masters) == 1 else torch.cat([m.detach() for m in masters], 0)
                self.views[key] = SplitWeight(w) if w.dim() == 2 else w

    def get(self, key):
        return self.views.get(key)

    def record_stream(self, stream) -> None:
        for v in self.views.values():
            for t in ((v.w0, v.w1s) if isinstance(v, SplitWeight) else (v,)):
                if t.is_cuda:
                    t.record_stream(stream)


_SHADOW = None             # the ParamShadow / SplitShadow of the region that is running


def active_shadow(dtype):
    """The shadow of the region that is running if it holds operands for activations of ``dtype``, else None."""
    sh = _SHADOW
    return sh if sh is not None and sh.dtype == dtype else None


class shadow_params:
    """``with shadow_params(specs, dtype, device):`` - the dense layers called inside find their compute-dtype operands in the
    shadow (``_linear`` by ``id(weight)``); no-op for fp32 (the masters ARE the operands) unless ``gemm_precision`` is "bf16x3":
    then the shadow holds the split weights (``SplitShadow``)."""

    def __init__(self, specs, dtype, device, gemm_precision="native"):
        self.args = (specs, dtype, device)
        self.x3 = gemm_precision == "bf16x3"
        self.prev = None

    def __enter__(self):
        global _SHADOW
        self.prev = _SHADOW
        specs, dtype, device = self.args
        if self.x3 and dtype == torch.float32 and device.type == "cuda":
            _SHADOW = SplitShadow(specs, device)
        else:
            _SHADOW = ParamShadow(specs, dtype, device) if (dtype != torch.float32 and device.type == "cuda") else None
        return _SHADOW

    def __exit__(self, *exc):
        global _SHADOW
        _SHADOW = self.prev
        return False


class use_shadow:
    """Re-enter an existing shadow (a checkpoint recompute runs a block in backward, outside the region's ``with``)."""

    def __init__(self, sh):
        self.sh, self.prev = sh, None

    def __enter__(self):
        global _SHADOW
        self.prev = _SHADOW
        if _SHADOW is None:
            _SHADOW = self.sh
        return _SHADOW

    def __exit__(self, *exc):
        global _SHADOW
        _SHADOW = self.prev
        return False


def linear_specs(*mods):
    """Shadow entries of plain ``nn.Linear`` modules: weight under id(weight), bias under id(bias)."""
    out = []
    for m in mods:
        out.append((id(m.weight), [m.weight], 0))
        if m.bias is not None:
            out.append((id(m.bias), [m.bias], 0))
    return out


def _linear(x, weight, bias=None, gemm_precision="native"):
    """x @ weight^T (+ bias) in x's dtype with autocast off (explicit precision policy).  Inside ``shadow_params`` the operands
    come from the region's shadow and the gradients go to the fp32 masters directly; otherwise per-call casts.
    ``gemm_precision`` "bf16x3" (fp32 ``x`` on the GPU): outside a shadow the weight is split for this call (``SplitWeight``);
    a shadow built for that mode already holds the split weights, whatever is passed here."""
    sh = active_shadow(x.dtype)
    if sh is not None:
        wc = sh.get(id(weight))
        bc = sh.get(id(bias)) if bias is not None else None
        if wc is not None and (bias is None or bc is not None):
            return _mm(x, wc, bc, (weight,) + ((bias,) if bias is not None else ()))
    if gemm_precision != "native":
        check_gemm_precision(gemm_precision)
        if x.dtype != torch.float32:
            raise TypeError(f"gemm_precision='bf16x3' keeps fp32 storage; got {x.dtype} activations")
        return _mm(x, SplitWeight(weight), None if bias is None else bias.detach(),
                   (weight,) + ((bias,) if bias is not None else ()))
    with torch.autocast("cuda", enabled=False):
        w = weight.to(x.dtype)
        b = None if bias is None else bias.to(x.dtype)
        return F.linear(x, w, b)
