"""Autograd operators over libgmlm_hip.so.  Every op is the HIP path; there is no eager fallback.

Tensors are PyTorch-owned device memory handed to the C ABI as raw pointers together with
``torch.cuda.current_stream()``; the library never allocates, frees or synchronises.
"""
from __future__ import annotations

from collections import namedtuple
from operator import itemgetter
from typing import Optional

import torch

from . import _lib
from ._lib import BF16, F32, check, lib


# ---------------------------------------------------------------------------------------------
# small helpers
# ---------------------------------------------------------------------------------------------
def _ptr(t: Optional[torch.Tensor]):
    return None if t is None else t.data_ptr()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _dt(t: torch.Tensor) -> int:
    if t.dtype == torch.float32:
        return F32
    if t.dtype == torch.bfloat16:
        return BF16
    raise TypeError(f"gmlm_amd kernels take float32 or bfloat16 tensors, got {t.dtype}")


def _cuda(*ts):
    for t in ts:
        if t is not None and not t.is_cuda:
            raise _lib.GmlmHipError("gmlm_amd ops run on the GPU only (tensor on %s); there is no CPU path" % t.device)
    dev = next(t for t in ts if t is not None).device
    _lib.require_gfx950(dev.index if dev.index is not None else torch.cuda.current_device())


def _ws(nbytes: int, device) -> torch.Tensor:
    return torch.empty(max(int(nbytes), 16), dtype=torch.uint8, device=device)


def _f32c(t: torch.Tensor) -> torch.Tensor:
    return t.detach().float().contiguous()


class KernelTimer:
    """Optional per-launch timing with HIP events recorded on the launch stream (bench.py roofline).
    Off by default (TIMER is None): the product path records nothing."""

    def __init__(self):
        self.records = []            # (name, start_event, end_event, meta)

    def span(self, name, **meta):
        return _Span(self, name, meta)

    def summary(self):
        torch.cuda.synchronize()
        out = {}
        for name, e0, e1, meta in self.records:
            d = out.setdefault(name, dict(launches=0, ms=0.0, bytes=0.0, flops=0.0))
            d["launches"] += 1
            d["ms"] += e0.elapsed_time(e1)
            d["bytes"] += meta.get("bytes", 0.0)
            d["flops"] += meta.get("flops", 0.0)
        return out


class _Span:
    def __init__(self, timer, name, meta):
        self.timer, self.name, self.meta = timer, name, meta

    def __enter__(self):
        self.e0 = torch.cuda.Event(enable_timing=True)
        self.e1 = torch.cuda.Event(enable_timing=True)
        self.e0.record()
        return self

    def __exit__(self, *exc):
        self.e1.record()
        self.timer.records.append((self.name, self.e0, self.e1, self.meta))
        return False


class _NoSpan:
    def __enter__(self):
        return self

    def __exit__(self, *exc):
        return False


TIMER: Optional[KernelTimer] = None
_NOSPAN = _NoSpan()


def _span(name, **meta):
    return TIMER.span(name, **meta) if TIMER is not None else _NOSPAN


def spmm_algorithmic_bytes(num_edges, num_segments, out_rows, f, elem, edge_w=False):
    """every edge reads its source row once (no cache credit) + a 4-byte index,
    per-segment row pointers, one output row per segment (+ a 4-byte 1/cnt lookup per edge backward)."""
    return float(num_edges * (f * elem + 4 + (4 if edge_w else 0)) + (num_segments + 1) * 4 + out_rows * f * elem)


SEED_DEVICE: Optional[torch.Tensor] = None   # optional int64[1] device counter added to every dropout seed (see graphs.py)


def _sd():
    """Device pointer of the seed counter (None = plain host seeds).  Kernels add *ptr to the host seed when they run, so a
    captured hipGraph draws fresh dropout masks on every replay (the counter is bumped inside the graph)."""
    return None if SEED_DEVICE is None else SEED_DEVICE.data_ptr()


def draw_seed() -> int:
    """Dropout seed from torch's CPU generator: replayed by torch.utils.checkpoint (RNG state is
    preserved there), costs no device sync."""
    return int(torch.randint(0, 2 ** 62, (1,), device="cpu").item())


# ---------------------------------------------------------------------------------------------
# K1: degree / edge types (integer)
# ---------------------------------------------------------------------------------------------
def degree(index: torch.Tensor, num_nodes: Optional[int] = None, dtype=torch.float32) -> torch.Tensor:
    """Drop-in for ``torch_geometric.utils.degree`` (main.py:65, 256): float32 occurrence counts."""
    _cuda(index)
    index = index.to(torch.long).contiguous()
    if num_nodes is None:
        num_nodes = int(index.max().item()) + 1 if index.numel() else 0
    if dtype == torch.float32:
        out = torch.empty(num_nodes, dtype=torch.float32, device=index.device)
        check(lib().gmlm_degree_f32(_ptr(index), index.numel(), num_nodes, _ptr(out), _stream()), "gmlm_degree_f32")
        return out
    out = torch.empty(num_nodes, dtype=torch.int32, device=index.device)
    check(lib().gmlm_degree_i32(_ptr(index), index.numel(), num_nodes, _ptr(out), _stream()), "gmlm_degree_i32")
    return out.to(dtype)


def edge_types_from_degree(edge_index: torch.Tensor, num_nodes: int) -> torch.Tensor:
    """main.py:253-267 as two kernels (degree histogram + bucketing); int64 [E], bit-exact."""
    _cuda(edge_index)
    src = edge_index[0].to(torch.long).contiguous()
    e = src.numel()
    deg = torch.empty(num_nodes, dtype=torch.int32, device=src.device)
    check(lib().gmlm_degree_i32(_ptr(src), e, num_nodes, _ptr(deg), _stream()), "gmlm_degree_i32")
    et = torch.empty(e, dtype=torch.long, device=src.device)
    check(lib().gmlm_edge_bucket(_ptr(src), _ptr(deg), e, num_nodes, _ptr(et), _stream()), "gmlm_edge_bucket")
    return et


# ---------------------------------------------------------------------------------------------
# K2/K3: relation-segmented mean aggregation
# ---------------------------------------------------------------------------------------------
def _spmm(src, rowptr, idx, edge_w, mean, num_segments, f, out, split=None):
    """split: optional graph.SplitPlan (long segments of a skewed graph are reduced chunk-wise)."""
    if split is not None and split.n_long > 0:
        partial = torch.empty(split.n_chunks, f, dtype=torch.float32, device=src.device)
        extra = (split.thresh, _ptr(split.long_seg), _ptr(split.chunk_ptr), _ptr(split.chunk_owner), split.n_long,
                 split.n_chunks, _ptr(partial))
    else:
        extra = (0, None, None, None, 0, 0, None)
    check(lib().gmlm_rgcn_mean_spmm(_ptr(src), src.shape[0], src.stride(0), _ptr(rowptr), _ptr(idx), _ptr(edge_w),
                                    1 if mean else 0, num_segments, f, _ptr(out), f, _dt(src), *extra, _stream()),
          "gmlm_rgcn_mean_spmm")


def column_sum(x: torch.Tensor) -> torch.Tensor:
    """fp32 column sums of a 2-D fp32 / bf16 tensor on the K4 statistics kernel (fixed-order partials, deterministic): the bias
    gradients of the dense layers.  (``x.sum(0, dtype=float32)`` - ATen's reduction, on shapes that take its cross-block path
    with a semaphore buffer - goes wrong from the second replay on inside a recorded hipGraph on this PyTorch / ROCm stack:
    tools/dev/aten_sum_graph_repro.py; this kernel needs no zero-initialised scratch.)"""
    _cuda(x)
    x = x.contiguous()
    n, f = x.shape
    out = torch.empty(2, f, dtype=torch.float32, device=x.device)
    if n == 0:
        return out[0].zero_()
    ws = _ws(lib().gmlm_colstats_workspace_bytes(n, f), x.device)
    check(lib().gmlm_colstats(_ptr(x), _dt(x), None, n, f, _ptr(out[0]), _ptr(out[1]), _ptr(ws), ws.numel(), _stream()), "gmlm_colstats")
    return out[0]


WGRAD_TILE = 256           # N and K granularity of gmlm_wgrad_bf16
WGRAD_NO_REMAP = 1         # gmlm_wgrad_bf16 flag: plain workgroup order
WGRAD_ONE_PHASE = 2        # gmlm_wgrad_bf16 flag: the one-barrier main loop (default: two wave groups a phase apart)


def wgrad_bf16(dy: torch.Tensor, x: torch.Tensor, splits: int = 0, flags: int = 0) -> torch.Tensor:
    """fp32 dW [N, K] = dy^T [N, T] @ x [T, K] for bf16 ``dy`` [T, N] / ``x`` [T, K] with unit column stride (a column slice
    of a wider tensor is fine): the split-K weight-gradient kernel, slice partials added in fixed order (deterministic).
    N and K multiples of WGRAD_TILE, T >= 32.  ``splits`` 0 = the kernel's default plan."""
    _cuda(dy, x)
    t, n = dy.shape
    k = x.shape[1]
    out = torch.empty(n, k, dtype=torch.float32, device=dy.device)
    ws = _ws(lib().gmlm_wgrad_workspace_bytes(t, n, k, splits), dy.device)
    check(lib().gmlm_wgrad_bf16(_ptr(dy), dy.stride(0), _ptr(x), x.stride(0), t, n, k, splits, _ptr(out), k, flags, _ptr(ws),
                                ws.numel(), _stream()), "gmlm_wgrad_bf16")
    return out


# ---------------------------------------------------------------------------------------------
# bf16x3: fp32-grade dense layers as ONE bf16 GEMM of three times the contraction depth (DESIGN.md section 4 "bf16x3")
# ---------------------------------------------------------------------------------------------
def _up8(n: int) -> int:
    return (n + 7) // 8 * 8


def split_bf16x3(x: torch.Tensor, order: int, stacked: bool = False, part_rows: Optional[int] = None) -> torch.Tensor:
    """bf16 operand of the three-product GEMM from an fp32 matrix ``x`` [rows, cols] (gmlm_split_bf16x3): x ~ hi + lo with
    hi = bf16(x), lo = bf16(x - hi); ``order`` 0 = the parts (hi, lo, hi), 1 = (hi, hi, lo).  Side by side along the contraction
    dimension: [rows, 3 * cols_out]; ``stacked``: [3 * rows, cols_out] (``part_rows`` > rows leaves zero rows behind every part).
    cols_out = cols rounded up to 8, the pad columns are zeros."""
    _cuda(x)
    if x.dim() != 2 or x.dtype != torch.float32:
        raise TypeError(f"split_bf16x3 takes a 2-D float32 tensor, got {tuple(x.shape)} {x.dtype}")
    rows, cols = x.shape
    if rows > 1 and x.stride(0) % 4 or (cols > 1 and x.stride(1) != 1) or x.data_ptr() % 16:
        x = x.contiguous()
        if rows > 1 and cols % 4:                                  # 16-byte aligned rows for the vector loads
            x = torch.nn.functional.pad(x, (0, (-cols) % 4))
        elif x.data_ptr() % 16:
            x = x.clone()
    ld_x = x.stride(0) if rows > 1 else _up8(cols)
    co = _up8(cols)
    if stacked:
        pr = rows if part_rows is None else int(part_rows)
        if pr < rows:
            raise ValueError(f"part_rows {pr} < rows {rows}")
        out = (torch.empty if pr == rows else torch.zeros)(3 * pr, co, dtype=torch.bfloat16, device=x.device)
        ld_out, part_stride = co, pr * co
    else:
        out = torch.empty(rows, 3 * co, dtype=torch.bfloat16, device=x.device)
        ld_out, part_stride = 3 * co, co
    check(lib().gmlm_split_bf16x3(_ptr(x), ld_x, rows, cols, co, _ptr(out), ld_out, part_stride, int(order), _stream()),
          "gmlm_split_bf16x3")
    return out


# ---------------------------------------------------------------------------------------------
# gradient clipping + AdamW as one multi-tensor step (include/gmlm_hip_optim.h; the tables are built by optim.FusedAdamW)
# ---------------------------------------------------------------------------------------------
def adamw_step(addr, numel, group, slot, chunks, num_chunks, num_tensors, hyper, num_groups, steps, num_slots, partial, nonfinite,
               bias_corr, status, max_norm: float) -> None:
    """The three launches of one step on the current stream: sum of squares per chunk -> norm, clip coefficient, skip, step
    counters and bias corrections -> update of p, m, v.  Every table is a raw device address laid out as the header says."""
    st = _stream()
    with _span("adamw_sumsq"):
        check(lib().gmlm_adamw_sumsq(addr, numel, chunks, num_chunks, partial, nonfinite, st), "gmlm_adamw_sumsq")
    with _span("adamw_finalize"):
        check(lib().gmlm_adamw_finalize(partial, nonfinite, num_chunks, float(max_norm), group, slot, num_tensors, hyper,
                                        num_groups, steps, num_slots, bias_corr, status, st), "gmlm_adamw_finalize")
    with _span("adamw_update"):
        check(lib().gmlm_adamw_update(addr, numel, group, chunks, num_chunks, hyper, num_groups, bias_corr, status, st),
              "gmlm_adamw_update")


def device_split_plan(rowptr: torch.Tensor, num_items: int, thresh: int = 64):
    """``graph.SplitPlan`` for segments known only on the device (they change every step): capacity-sized arrays filled by ONE
    kernel, no host round trip; unused slots are -1 and skipped by the aggregation kernels (gmlm_split_plan_build)."""
    import ctypes
    from .graph import SplitPlan
    cl, cc = ctypes.c_int64(), ctypes.c_int64()
    check(lib().gmlm_split_plan_capacity(int(num_items), int(thresh), ctypes.byref(cl), ctypes.byref(cc)), "gmlm_split_plan_capacity")
    dev = rowptr.device
    long_seg = torch.empty(cl.value, dtype=torch.int32, device=dev)
    chunk_ptr = torch.empty(cl.value + 1, dtype=torch.int32, device=dev)
    chunk_owner = torch.empty(cc.value, dtype=torch.int32, device=dev)
    check(lib().gmlm_split_plan_build(_ptr(rowptr), rowptr.numel() - 1, int(num_items), int(thresh), _ptr(long_seg), _ptr(chunk_ptr),
                                      _ptr(chunk_owner), _stream()), "gmlm_split_plan_build")
    return SplitPlan(int(thresh), long_seg, chunk_ptr, chunk_owner, int(cl.value), int(cc.value))


class RGCNAggregate(torch.autograd.Function):
    """H[i, r*F:(r+1)*F] = mean_{j->i, type r} x[j]  (K2); backward = same kernel on the transposed CSR (K3)."""

    @staticmethod
    def forward(ctx, x: torch.Tensor, csr) -> torch.Tensor:
        _cuda(x)
        x = x.contiguous()
        n_src, f = x.shape
        n = csr.num_nodes
        if n_src != csr.num_src:
            raise ValueError(f"x has {n_src} rows but the graph expects {csr.num_src} source rows")
        out = torch.empty(n, csr.r_active * f, dtype=x.dtype, device=x.device)
        with _span("spmm_fwd", bytes=spmm_algorithmic_bytes(csr.num_edges, n * csr.r_active, n * csr.r_active, f,
                                                           x.element_size()), f=f):
            _spmm(x, csr.rowptr, csr.col, None, True, n * csr.r_active, f, out, csr.split)
        ctx.csr, ctx.n_src = csr, x.shape[0]
        return out

    @staticmethod
    def backward(ctx, gh: torch.Tensor):
        csr = ctx.csr
        gh = gh.contiguous()
        n, rf = gh.shape
        f = rf // csr.r_active
        gx = torch.empty(csr.num_src, f, dtype=gh.dtype, device=gh.device)
        with _span("spmm_bwd", bytes=spmm_algorithmic_bytes(csr.num_edges, csr.num_src, csr.num_src, f, gh.element_size(),
                                                           True), f=f):
            _spmm(gh.view(n * csr.r_active, f), csr.t_rowptr, csr.t_seg, csr.inv_cnt, False, csr.num_src, f, gx, csr.t_split)
        return gx, None


# ---------------------------------------------------------------------------------------------
# K4: GraphNorm + GELU + dropout
# ---------------------------------------------------------------------------------------------
GN_ONE_PASS_MAX_RATIO = 64.0   # R above which a GraphNorm column takes the second statistics pass (row 0 beyond ~8 sigma)


class GraphNormAct(torch.autograd.Function):
    """y = dropout(act(GraphNorm(z))).  z [n, f] in the compute dtype (the GEMM output feeds the kernels
    directly: no fp32 staging copy); y and dz in the same dtype; statistics fp32.

    ``reducer``: optional callable(tensor) summing a small fp32 tensor over all ranks in place (the
    1-D node partition makes GraphNorm's column statistics global: SURVEY.md §8e); ``n_total`` is the
    global row count.
    """

    @staticmethod
    def forward(ctx, z, weight, bias, mean_scale, eps, act, p, seed, out_dtype, reducer, n_total):
        _cuda(z)
        z = z.to(out_dtype).contiguous()
        n, f = z.shape
        n_total = int(n_total) if n_total else n
        dev = z.device
        w, b, ms = _f32c(weight), _f32c(bias), _f32c(mean_scale)
        st = _stream()
        dt = _dt(z)
        stats = torch.empty(2, f, dtype=torch.float32, device=dev)
        shift = None
        if reducer is None and n > 0:
            shift = z[0].float().contiguous()          # shifted sums: no cancellation in E[o^2] unless row 0 lies far out (below)
        ws = _ws(lib().gmlm_colstats_workspace_bytes(n, f), dev)
        check(lib().gmlm_colstats(_ptr(z), dt, _ptr(shift), n, f, _ptr(stats[0]), _ptr(stats[1]), _ptr(ws), ws.numel(), st),
              "gmlm_colstats")
        if reducer is not None:
            # exact two-pass in the distributed case: all-reduce sum(x) -> mean, then sum((x - mean*ms)^2)
            reducer(stats)
            mu = stats[0] / n_total
            shift = (mu * ms).contiguous()
            check(lib().gmlm_colstats(_ptr(z), dt, _ptr(shift), n, f, _ptr(stats[0]), _ptr(stats[1]), _ptr(ws), ws.numel(),
                                      st), "gmlm_colstats")
            reducer(stats)
            mean = mu.contiguous()
            rstd = torch.rsqrt(stats[1] / n_total + eps).contiguous()
        else:
            mr = torch.empty(2, f, dtype=torch.float32, device=dev)          # [mean; rstd]
            check(lib().gmlm_graphnorm_finalize(_ptr(stats[0]), _ptr(stats[1]), _ptr(shift), _ptr(ms), n_total, f, eps,
                                                _ptr(mr[0]), _ptr(mr[1]), st), "gmlm_graphnorm_finalize")
            # finalize forms E[o^2] = (s2 - 2 d s1) / n + d^2 with d = mean*ms - z[0]: when row 0 lies far from the column mean
            # this cancels and loses ~log2(R) bits, R = (s2 / n) / var.  A second pass shifted by that mean (s1 ~ 0: E[o^2] is
            # the sum of s2 / n and d^2, nothing cancels) replaces the columns with R > GN_ONE_PASS_MAX_RATIO; the others keep
            # the one-pass values ('GraphNorm statistics').  No host sync: both passes always run, the
            # choice is per column on the device.
            stats2 = torch.empty_like(stats)
            check(lib().gmlm_colstats(_ptr(z), dt, _ptr(mr[0]), n, f, _ptr(stats2[0]), _ptr(stats2[1]), _ptr(ws), ws.numel(),
                                      st), "gmlm_colstats")
            mr2 = torch.empty_like(mr)
            check(lib().gmlm_graphnorm_finalize(_ptr(stats2[0]), _ptr(stats2[1]), _ptr(mr[0]), _ptr(ms), n_total, f, eps,
                                                _ptr(mr2[0]), _ptr(mr2[1]), st), "gmlm_graphnorm_finalize")
            mr = torch.where(stats[1] * mr[1] * mr[1] > GN_ONE_PASS_MAX_RATIO * n_total, mr2, mr)
            mean, rstd = mr[0], mr[1]
        y = torch.empty(n, f, dtype=out_dtype, device=dev)
        sd = ctx.sd = _sd()
        check(lib().gmlm_graphnorm_apply(_ptr(z), _ptr(mean), _ptr(rstd), _ptr(w), _ptr(b), _ptr(ms), n, f, int(act),
                                         float(p), seed, sd, _ptr(y), dt, st), "gmlm_graphnorm_apply")
        ctx.save_for_backward(z, mean, rstd, w, b, ms)
        ctx.cfg = (int(act), float(p), seed, reducer, n_total)
        return y

    @staticmethod
    def backward(ctx, gy):
        z, mean, rstd, w, b, ms = ctx.saved_tensors
        act, p, seed, reducer, n_total = ctx.cfg
        gy = gy.contiguous().to(z.dtype)
        n, f = z.shape
        dev = z.device
        st = _stream()
        dt = _dt(z)
        gs = torch.empty(2, f, dtype=torch.float32, device=dev)
        ws = _ws(lib().gmlm_colstats_workspace_bytes(n, f), dev)
        sd = ctx.sd
        check(lib().gmlm_graphnorm_bwd_stats(_ptr(gy), dt, _ptr(z), _ptr(mean), _ptr(rstd), _ptr(w), _ptr(b), _ptr(ms),
                                             n, f, act, p, seed, sd, _ptr(gs), _ptr(ws), ws.numel(), st),
              "gmlm_graphnorm_bwd_stats")
        gs_local = gs
        if reducer is not None:
            gs_local = gs.clone()
            reducer(gs)
        dz = torch.empty(n, f, dtype=z.dtype, device=dev)
        if reducer is None:
            dw = torch.empty(f, dtype=torch.float32, device=dev)
            db = torch.empty_like(dw)
            dms = torch.empty_like(dw)
            check(lib().gmlm_graphnorm_bwd_apply(_ptr(gy), dt, _ptr(z), _ptr(mean), _ptr(rstd), _ptr(w), _ptr(b),
                                                 _ptr(ms), _ptr(gs), n, n_total, f, act, p, seed, sd, _ptr(dz), _ptr(dw),
                                                 _ptr(db), _ptr(dms), st), "gmlm_graphnorm_bwd_apply")
        else:
            check(lib().gmlm_graphnorm_bwd_apply(_ptr(gy), dt, _ptr(z), _ptr(mean), _ptr(rstd), _ptr(w), _ptr(b),
                                                 _ptr(ms), _ptr(gs), n, n_total, f, act, p, seed, sd, _ptr(dz), None, None,
                                                 None, st), "gmlm_graphnorm_bwd_apply")
            # parameter grads: LOCAL contributions only (the gradient all-reduce sums them over ranks)
            dw, db = gs_local[1].clone(), gs_local[0].clone()
            m2 = gs[1] / n_total
            # sum over LOCAL rows of do_j = w*rstd*(sum_local gz - m2 * sum_local ohat)
            sum_oh_local = (z.float().sum(0) - n * mean * ms) * rstd
            dms = -mean * (w * rstd * (gs_local[0] - m2 * sum_oh_local))
        return dz, dw, db, dms, None, None, None, None, None, None, None


# ---------------------------------------------------------------------------------------------
# K6: bias + dropout + residual + LayerNorm (+GELU)
# ---------------------------------------------------------------------------------------------
LN_WIDE_ABOVE = 1024            # widest row of gmlm_bias_res_layernorm_*; wider rows (to 4,096) go to gmlm_bias_res_layernorm_wide_*
ATTN_WIDE_DIMS = (256, 384, 512)   # head dims of gmlm_attention_wide_* (attn_wide.hip)


def _ln_entries(f: int):   # (forward, backward, workspace size); rows wider than 1,024: norm_wide.hip (a workgroup per row), same arguments
    if f > LN_WIDE_ABOVE:
        return "gmlm_bias_res_layernorm_wide_fwd", "gmlm_bias_res_layernorm_wide_bwd", "gmlm_bias_res_layernorm_wide_bwd_workspace_bytes"
    return "gmlm_bias_res_layernorm_fwd", "gmlm_bias_res_layernorm_bwd", "gmlm_layernorm_bwd_workspace_bytes"


class BiasResLayerNorm(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, bias, residual, gamma, beta, eps, act, p, seed):
        _cuda(x)
        shape = x.shape
        f = shape[-1]
        x2 = x.contiguous().view(-1, f)
        rows = x2.shape[0]
        res2 = None if residual is None else residual.to(x.dtype).contiguous().view(-1, f)
        bf = None if bias is None else _f32c(bias)
        g, b = _f32c(gamma), _f32c(beta)
        y = torch.empty_like(x2)
        mean = torch.empty(rows, dtype=torch.float32, device=x.device)
        rstd = torch.empty_like(mean)
        sd = ctx.sd = _sd()
        name = _ln_entries(f)[0]
        check(getattr(lib(), name)(_ptr(x2), _ptr(bf), _ptr(res2), _ptr(g), _ptr(b), rows, f, float(eps),
                                   int(act), float(p), seed, sd, _ptr(y), _ptr(mean), _ptr(rstd), _dt(x2), _stream()), name)
        ctx.save_for_backward(x2, res2, bf, g, b, mean, rstd)
        ctx.cfg = (int(act), float(p), seed, shape, bias is not None, residual is not None)
        return y.view(shape)

    @staticmethod
    def backward(ctx, gy):
        x2, res2, bf, g, b, mean, rstd = ctx.saved_tensors
        act, p, seed, shape, has_bias, has_res = ctx.cfg
        rows, f = x2.shape
        gy2 = gy.contiguous().view(rows, f).to(x2.dtype)
        dx = torch.empty_like(x2)
        dres = torch.empty_like(x2) if has_res else None
        dg = torch.empty(f, dtype=torch.float32, device=x2.device)
        dbeta = torch.empty_like(dg)
        dbias = torch.empty_like(dg) if has_bias else None
        _, name, ws_name = _ln_entries(f)
        ws = _ws(getattr(lib(), ws_name)(rows, f), x2.device)
        sd = ctx.sd
        check(getattr(lib(), name)(_ptr(gy2), _ptr(x2), _ptr(bf), _ptr(res2), _ptr(g), _ptr(b), _ptr(mean),
                                   _ptr(rstd), rows, f, act, p, seed, sd, _ptr(dx), _ptr(dres), _ptr(dg),
                                   _ptr(dbeta), _ptr(dbias), _dt(x2), _ptr(ws), ws.numel(), _stream()), name)
        return (dx.view(shape), dbias, None if dres is None else dres.view(shape), dg, dbeta, None, None, None, None)


def bias_res_layernorm(x, bias, residual, gamma, beta, eps=1e-5, act=False, p=0.0, training=False):
    p = float(p) if training else 0.0
    return BiasResLayerNorm.apply(x, bias, residual, gamma, beta, eps, act, p, draw_seed() if p > 0 else 0)


# ---------------------------------------------------------------------------------------------
# K5/K7: attention core
# ---------------------------------------------------------------------------------------------
def _rows_view(t: torch.Tensor, h: int, d: int):
    """[b, l, h*d-wide slice] view -> (tensor, row stride in elements); last dim must be contiguous."""
    if t.stride(-1) != 1 or t.shape[-1] != h * d:
        raise ValueError("attention operands must be [b, l, h*d] with a contiguous last dim")
    if t.stride(0) != t.shape[1] * t.stride(1) and t.shape[0] > 1 and t.shape[1] > 0:
        raise ValueError("attention operands must have batch stride = l * row stride")
    return t.stride(1)


def _short_path(dtype, d: int, rows: int, pairs: int) -> bool:
    """Same condition as the C entries: bf16, d = 64, every sequence <= 128 rows, >= 512 (sequence, head) pairs -> the
    LDS-resident short-sequence kernels (their backward forms delta itself and needs neither ``out`` nor ``out_lo``; the C
    backward takes that path only when ``out_lo`` is NULL, which ``Attention`` / ``AttentionQKV`` pass there)."""
    return dtype == torch.bfloat16 and d == 64 and rows <= 128 and pairs >= 512


def _gqa_short_path(groups, dtype, d: int, max_len: int, seqs: int, hq: int) -> bool:
    """The one rule for the grouped-KV families (causal d = 64, bidirectional): the LDS-resident short-sequence entry points
    (gmlm_attention_gqa_short_*, include/gmlm_hip_gqa_short.h) run iff the caller gave ``groups`` (packed layout only) and
    ``_short_path`` holds for (sequences x query heads) pairs.  The 512 is the threshold measured for the K5 short kernels;
    whether it is the right one for the grouped kernels has not been measured."""
    return groups is not None and _short_path(dtype, d, max_len, seqs * hq)


D32_SHORT_MIN_PAIRS = 96     # measured: the new route is not slower from the smallest count probed on (8 sequences x 12 heads)


def _d32_short_path(groups, dtype, d: int, max_len: int, seqs: int, h: int) -> bool:
    """The one rule for head dim 32: the LDS-resident short-sequence entry points (gmlm_attention_d32_short_*,
    include/gmlm_hip_d32_short.h) run iff the caller gave ``groups`` (packed layout only), the dtype is bf16, ``d == 32``, no
    sequence is longer than 128 rows, ``h`` is even (a work item is a pair of adjacent heads; the entry points refuse an odd
    ``h``, which stays on the streaming ``gmlm_attention_d32_*`` kernels) and there are at least ``D32_SHORT_MIN_PAIRS``
    (sequence, head) pairs: 96, the smallest count measured, where the one-launch backward already wins on launches alone (DESIGN.md
    section 5 "Head dim 32, short sequences" has the table).  ``GraphTextLM`` builds ``groups`` from 512 pairs on, as at head dim 64."""
    return groups is not None and dtype == torch.bfloat16 and d == 32 and max_len <= 128 and h % 2 == 0 \
        and seqs * h >= D32_SHORT_MIN_PAIRS


def _d32_short_common(q, k, v, cu_seqlens, b, max_len, l, h, hd3, scale, p, seed, sd, groups):
    """Arguments both gmlm_attention_d32_short_* calls share, in header order: (head ..., seq_groups, num_groups)."""
    return ((_ptr(cu_seqlens), b, int(max_len), l, h, 32, hd3, hd3, hd3, float(scale), float(p), seed, sd),
            (_ptr(groups), _groups_arg(groups, cu_seqlens)))


def _groups_arg(groups, cu_seqlens):
    """``groups``: int32 [G + 1] on the device of ``cu_seqlens`` (``pack_sequence_groups``); -> G."""
    if groups.dtype != torch.int32 or groups.dim() != 1 or groups.numel() < 1 or not groups.is_contiguous() \
            or groups.device != cu_seqlens.device:
        raise ValueError("groups must be a contiguous int32 [groups + 1] tensor on the device of cu_seqlens")
    return groups.numel() - 1


# A head-dim family of non-causal attention entry points: names, and getters that put arguments named as in the headers in ABI
# order.  The orders are where families differ: out_lo last or after `out`, packed mode, seq_groups and dbias (`short`) or not.
_AttnFamily = namedtuple("_AttnFamily", "fwd bwd ws fwd_args bwd_args ws_args packed short")
_ATTN_FWD_ARGS = "q k v kv_len b h lq lk d q_stride k_stride v_stride scale dropout_p seed seed_dev out out_lo lse dtype "
_ATTN_BWD_ARGS = "kv_len b h lq lk d q_stride k_stride v_stride scale dropout_p seed seed_dev dq dk dv dq_stride dk_stride dv_stride dtype "
_ATTN_OPTIONAL = dict(cu_seqlens=None, max_len=0, seq_groups=None, num_groups=0, dbias_partial=None, dbias=None)


def _attn_family(stem, ws, ws_args, fwd_tail, bwd_head, bwd_tail):
    return _AttnFamily(stem + "_fwd", stem + "_bwd", stem + ws, itemgetter(*(_ATTN_FWD_ARGS + fwd_tail).split()),
                       itemgetter(*(bwd_head + _ATTN_BWD_ARGS + bwd_tail).split()), itemgetter(*ws_args.split()),
                       "cu_seqlens" in fwd_tail, "seq_groups" in fwd_tail)


_ATTN_D64 = _attn_family("gmlm_attention", "_bwd_workspace_bytes", "h lq lk d", "cu_seqlens max_len seq_groups num_groups stream",
                         "q k v out dout lse ", "cu_seqlens max_len workspace workspace_bytes dbias_partial dbias out_lo seq_groups "
                         "num_groups stream")                                                    # d = 64 / 96: attn_kernels.hip
_ATTN_D32 = _attn_family("gmlm_attention_d32", "_bwd_workspace_bytes", "h lq", "cu_seqlens max_len stream", "q k v out dout lse ",
                         "cu_seqlens max_len workspace workspace_bytes out_lo stream")            # attn_d32.hip: no bound on b * h
_ATTN_D128, _ATTN_WIDE = (_attn_family(stem_, ws_, "h lq", "stream", "q k v out out_lo dout lse ", "workspace workspace_bytes stream")
                          for stem_, ws_ in (("gmlm_attention_d128", "_workspace_bytes"), ("gmlm_attention_wide", "_bwd_workspace_bytes")))
_ATTN_FAMILIES = {64: _ATTN_D64, 96: _ATTN_D64, 32: _ATTN_D32, 128: _ATTN_D128, **{d_: _ATTN_WIDE for d_ in ATTN_WIDE_DIMS}}


def _attn_family_of(a, fused_qkv):
    """One lookup per call.  A head dim without a family goes to the d = 64 / 96 entries, whose own check refuses it by name;
    so does a fused-QKV call (AttentionQKV) at a head dim whose family has no packed mode.  An argument the ABI lacks is an error."""
    fam = _ATTN_FAMILIES.get(a["d"], _ATTN_D64)
    if fused_qkv and not fam.packed:
        fam = _ATTN_D64
    if (a["cu_seqlens"] is not None and not fam.packed) or ((a["seq_groups"] is not None or a["dbias"] is not None) and not fam.short):
        raise _lib.GmlmHipError(f"{fam.fwd[:-4]}_*: no packed mode / seq_groups / fused bias sums at head dim {a['d']}")
    return fam


def _attention_fwd(fused_qkv=False, **a):
    """The one forward call: every argument by its header name (pointers as pointers), placed by the family's order."""
    a = {**_ATTN_OPTIONAL, **a, "stream": _stream()}
    fam = _attn_family_of(a, fused_qkv)
    check(getattr(lib(), fam.fwd)(*fam.fwd_args(a)), fam.fwd)


def _attention_bwd(device, fused_qkv=False, **a):
    """The one backward call, same conventions; allocates the family's workspace (delta: a packed batch is one sequence)."""
    a = {**_ATTN_OPTIONAL, **a, "stream": _stream()}
    fam = _attn_family_of(a, fused_qkv)
    ws = _ws(getattr(lib(), fam.ws)(a["b"] if a["cu_seqlens"] is None else 1, *fam.ws_args(a)), device)
    a.update(workspace=ws.data_ptr(), workspace_bytes=ws.numel())
    check(getattr(lib(), fam.bwd)(*fam.bwd_args(a)), fam.bwd)


class Attention(torch.autograd.Function):
    """out[b, lq, h*d] = softmax(q k^T * scale + key-padding mask) v with streaming softmax.

    q: [b, lq, h*d], k/v: [b, lk, h*d] (may be strided slices of a fused QKV buffer);
    kv_len: int32 [b] or None.
    """

    @staticmethod
    def forward(ctx, q, k, v, kv_len, h, scale, p, seed):
        _cuda(q, k, v)
        b, lq, hd = q.shape
        lk = k.shape[1]
        d = hd // h
        qs, ks, vs = _rows_view(q, h, d), _rows_view(k, h, d), _rows_view(v, h, d)
        out = torch.empty(b, lq, hd, dtype=q.dtype, device=q.device)
        lse = torch.empty(b, h, lq, dtype=torch.float32, device=q.device)
        # bf16 streaming path: keep the rounding residual of the output for the backward's delta (gmlm_hip.h, out_lo)
        want_lo = q.dtype == torch.bfloat16 and not _short_path(q.dtype, d, max(lq, lk), b * h) and \
            any(t.requires_grad for t in (q, k, v))
        out_lo = torch.empty_like(out) if want_lo else None
        with _span("attn_fwd_d%d" % d, flops=4.0 * b * h * lq * lk * d):
            sd = ctx.sd = _sd()
            _attention_fwd(q=_ptr(q), k=_ptr(k), v=_ptr(v), kv_len=_ptr(kv_len), b=b, h=h, lq=lq, lk=lk, d=d, q_stride=qs, k_stride=ks,
                           v_stride=vs, scale=float(scale), dropout_p=float(p), seed=seed, seed_dev=sd, out=_ptr(out),
                           out_lo=_ptr(out_lo), lse=_ptr(lse), dtype=_dt(q))
        ctx.save_for_backward(q, k, v, out, lse, kv_len, out_lo)
        ctx.cfg = (h, float(scale), float(p), seed)
        return out

    @staticmethod
    def backward(ctx, gout):
        q, k, v, out, lse, kv_len, out_lo = ctx.saved_tensors
        h, scale, p, seed = ctx.cfg
        b, lq, hd = q.shape
        lk = k.shape[1]
        d = hd // h
        gout = gout.contiguous().to(q.dtype)
        dq = torch.empty(b, lq, hd, dtype=q.dtype, device=q.device)
        dk = torch.empty(b, lk, hd, dtype=q.dtype, device=q.device)
        dv = torch.empty(b, lk, hd, dtype=q.dtype, device=q.device)
        with _span("attn_bwd_d%d" % d, flops=10.0 * b * h * lq * lk * d):
            _attention_bwd(q.device, q=_ptr(q), k=_ptr(k), v=_ptr(v), out=_ptr(out), out_lo=_ptr(out_lo), dout=_ptr(gout), lse=_ptr(lse),
                           kv_len=_ptr(kv_len), b=b, h=h, lq=lq, lk=lk, d=d, q_stride=q.stride(1), k_stride=k.stride(1),
                           v_stride=v.stride(1), scale=scale, dropout_p=p, seed=seed, seed_dev=ctx.sd, dq=_ptr(dq), dk=_ptr(dk),
                           dv=_ptr(dv), dq_stride=hd, dk_stride=hd, dv_stride=hd, dtype=_dt(q))
        return dq, dk, dv, None, None, None, None, None


class AttentionQKV(torch.autograd.Function):
    """Self-attention on a fused QKV buffer (BERT layout).  Forward reads q/k/v in place through row
    strides; backward writes dq|dk|dv straight into ONE gradient buffer of the same layout, so no
    slice-gradient accumulation passes are needed.

    padded mode: qkv [b, l, 3*h*d], kv_len int32 [b] or None.
    packed mode: qkv [total_rows, 3*h*d], cu_seqlens int32 [b+1], max_len = longest sequence: sequence i owns
    rows [cu[i], cu[i+1]) and attends only to itself; no padded token exists anywhere.
    """

    @staticmethod
    def forward(ctx, qkv, kv_len, h, scale, p, seed, cu_seqlens, max_len, pair_count=None, groups=None, *bias_masters):
        """``bias_masters``: optional (q, k, v) bias parameters of the fused projection that produced ``qkv``.  Their values
        are not read (the projection has added them); they are inputs so that backward can RETURN their gradient, the
        column sums of dqkv, which the short-sequence kernel forms in-kernel (otherwise one reduction pass here).
        ``groups`` (packed mode): int32 [G + 1] device tensor; work item g of the short-sequence kernels = sequences
        [groups[g], groups[g+1]) - at most 13 sequences / 128 rows (``pack_sequence_groups``)."""
        _cuda(qkv)
        qkv = qkv.contiguous()
        packed = cu_seqlens is not None
        if packed:
            l, hd3 = qkv.shape
            b = cu_seqlens.numel() - 1
        else:
            b, l, hd3 = qkv.shape
        hd = hd3 // 3
        d = hd // h
        q, k, v = qkv[..., :hd], qkv[..., hd:2 * hd], qkv[..., 2 * hd:]
        out = torch.empty(qkv.shape[:-1] + (hd,), dtype=qkv.dtype, device=qkv.device)
        lse = torch.empty((h, l) if packed else (b, h, l), dtype=torch.float32, device=qkv.device)
        # packed: exact sum of len^2 when the caller knows it (host copy of the lengths), else the bound max_len * rows
        flops = 4.0 * h * d * ((float(pair_count) if pair_count else float(max_len) * l) if packed else float(b) * l * l)
        rows = int(max_len) if packed else l
        d32s = packed and _d32_short_path(groups, qkv.dtype, d, rows, b, h)     # head dim 32: its own short-sequence entry points
        short = _short_path(qkv.dtype, d, rows, b * h) or d32s
        if groups is not None and not (packed and short):
            groups = None                                       # only the short-sequence kernels pack sequences into work items
        n_groups = 0 if groups is None else groups.numel() - 1
        # (a backward runs when ANY input needs a gradient: trainable bias masters behind a frozen qkv get the same delta)
        out_lo = torch.empty_like(out) if (qkv.dtype == torch.bfloat16 and not short and any(ctx.needs_input_grad)) else None
        nb = out.numel() * out.element_size()                   # one of q, k, v, o
        with _span("attn_fwd_d%d" % d, flops=flops, bytes=(4 + (1 if out_lo is not None else 0)) * nb):
            sd = ctx.sd = _sd()
            if d32s:
                head, tail = _d32_short_common(q, k, v, cu_seqlens, b, max_len, l, h, hd3, scale, p, seed, sd, groups)
                name = "gmlm_attention_d32_short_fwd"
                check(getattr(lib(), name)(_ptr(q), _ptr(k), _ptr(v), *head, *tail, _ptr(out), _ptr(lse), _dt(qkv), _stream()), name)
            else:
                _attention_fwd(True, q=_ptr(q), k=_ptr(k), v=_ptr(v), kv_len=_ptr(kv_len), b=b, h=h, lq=l, lk=l, d=d, q_stride=hd3,
                               k_stride=hd3, v_stride=hd3, scale=float(scale), dropout_p=float(p), seed=seed, seed_dev=sd, out=_ptr(out),
                               out_lo=_ptr(out_lo), lse=_ptr(lse), dtype=_dt(qkv), cu_seqlens=_ptr(cu_seqlens), max_len=int(max_len),
                               seq_groups=_ptr(groups), num_groups=n_groups)
        if short:
            ctx.save_for_backward(qkv, lse, kv_len, cu_seqlens, groups)        # the fused backward never reads the forward output
        else:
            ctx.save_for_backward(qkv, lse, kv_len, cu_seqlens, groups, out, out_lo)
        ctx.short, ctx.d32s = short, d32s
        ctx.cfg = (h, float(scale), float(p), seed, int(max_len), b, l, flops)
        ctx.bias_shapes = [(m.shape[0], m.dtype) for m in bias_masters]
        return out

    @staticmethod
    def backward(ctx, gout):
        if ctx.short:
            qkv, lse, kv_len, cu_seqlens, groups = ctx.saved_tensors
            out, out_lo = gout, None                            # placeholder pointer: not read on this path
        else:
            qkv, lse, kv_len, cu_seqlens, groups, out, out_lo = ctx.saved_tensors
        h, scale, p, seed, max_len, b, l, flops = ctx.cfg
        # per master; a frozen one gets None, never a missing entry (cut to the masters: _RopeAttention runs this with its own ctx)
        need_db = ctx.needs_input_grad[10:10 + len(ctx.bias_shapes)] if ctx.bias_shapes else ()
        want_db = any(need_db)
        hd3 = qkv.shape[-1]
        hd = hd3 // 3
        d = hd // h
        gout = gout.contiguous().to(qkv.dtype)
        q, k, v = qkv[..., :hd], qkv[..., hd:2 * hd], qkv[..., 2 * hd:]
        dqkv = torch.empty_like(qkv)
        dq, dk, dv = dqkv[..., :hd], dqkv[..., hd:2 * hd], dqkv[..., 2 * hd:]
        # short-sequence path (one launch per (sequence, head): same condition as the C entry): the column sums of dqkv --
        # the bias gradient of the fused QKV projection that produced qkv -- come out of the kernel as well
        fused_db = want_db and ctx.short
        n_groups = 0 if groups is None else groups.numel() - 1
        part = db = None
        if fused_db:
            part = _ws(4 * (n_groups or b) * hd3, qkv.device).view(torch.float32)
            db = torch.empty(hd3, dtype=torch.float32, device=qkv.device)
        # q, k, v, dO in; dq, dk, dv out (+ o, o_lo on the streaming path, which forms delta from them)
        with _span("attn_bwd_d%d" % d, flops=2.5 * flops, bytes=(7 + (0 if ctx.short else 2)) * qkv.numel() // 3 * qkv.element_size()):
            if ctx.d32s:
                head, tail = _d32_short_common(q, k, v, cu_seqlens, b, max_len, l, h, hd3, scale, p, seed, ctx.sd, groups)
                name = "gmlm_attention_d32_short_bwd"
                check(getattr(lib(), name)(_ptr(q), _ptr(k), _ptr(v), _ptr(gout), _ptr(lse), *head, *tail, _ptr(dq), _ptr(dk), _ptr(dv),
                                           hd3, hd3, hd3, _ptr(part), _ptr(db), _dt(qkv), _stream()), name)
            else:
                _attention_bwd(qkv.device, True, q=_ptr(q), k=_ptr(k), v=_ptr(v), out=_ptr(out), out_lo=_ptr(out_lo), dout=_ptr(gout),
                               lse=_ptr(lse), kv_len=_ptr(kv_len), b=b, h=h, lq=l, lk=l, d=d, q_stride=hd3, k_stride=hd3, v_stride=hd3,
                               scale=scale, dropout_p=p, seed=seed, seed_dev=ctx.sd, dq=_ptr(dq), dk=_ptr(dk), dv=_ptr(dv),
                               dq_stride=hd3, dk_stride=hd3, dv_stride=hd3, dtype=_dt(qkv), cu_seqlens=_ptr(cu_seqlens), max_len=max_len,
                               dbias_partial=_ptr(part), dbias=_ptr(db), seq_groups=_ptr(groups), num_groups=n_groups)
        dbs = (None,) * len(ctx.bias_shapes)
        if want_db:
            if db is None:
                db = column_sum(dqkv.reshape(-1, hd3))
            dbs = tuple((g if g.dtype == dt_ else g.to(dt_)) if need else None
                        for g, (_, dt_), need in zip(db.split([n_ for n_, _ in ctx.bias_shapes], 0), ctx.bias_shapes, need_db))
        return (dqkv, None, None, None, None, None, None, None, None, None, *dbs)


class AttentionBlock:
    """Per-block arithmetic of the ring K|V exchange (gmlm_amd.dist._RingAttention) on the HIP kernels, outside
    autograd: ``fwd`` returns the block's normalised output and its log-sum-exp; ``bwd`` evaluates the block's share of
    dQ / dK / dV from the GLOBAL output and log-sum-exp (P is recomputed as exp(S - lse_global), delta = rowsum(dO * O)).

    Contract of ``bwd`` (gmlm_hip.h, "Foreign lse / out"): every path that forms delta from ``out`` accepts an ``lse`` and an
    ``out`` that are not its own forward's - ``lse`` >= the block's own, ``out`` the output of all keys.  The short-sequence
    path (bf16, d = 64, <= 128 rows, b*h >= 512) sums delta over the block's own keys and ASSUMES the block's own ``lse``; it
    is selected only without ``out_lo``.  A bf16 ring block therefore always passes ``out_lo`` (``_RingAttention`` does);
    without it the call is the plain backward of ``fwd``'s own ``out`` and ``lse``."""

    def __init__(self, num_heads: int, scale: float, dropout_p: float = 0.0):
        self.h, self.scale, self.p = num_heads, float(scale), float(dropout_p)

    def fwd(self, q, k, v, kv_len, seed):
        b, lq, hd = q.shape
        lk, d = k.shape[1], hd // self.h
        if d > 128:
            raise NotImplementedError(f"ring attention has no block form at head dim {d}: the wide-head kernels "
                                      "(gmlm_attention_wide_*) run on one GPU only")
        _cuda(q, k, v)
        if d not in (64, 96):
            raise NotImplementedError(f"ring attention needs a native head dim (64 or 96), got {d}: the head-dim-128 kernels "
                                      "(gmlm_attention_d128_*) have no ring-block form")
        out = torch.empty(b, lq, hd, dtype=q.dtype, device=q.device)
        lse = torch.empty(b, self.h, lq, dtype=torch.float32, device=q.device)
        with _span("attn_fwd_d%d" % d, flops=4.0 * b * self.h * lq * lk * d):
            _attention_fwd(q=_ptr(q), k=_ptr(k), v=_ptr(v), kv_len=_ptr(kv_len), b=b, h=self.h, lq=lq, lk=lk, d=d,
                           q_stride=_rows_view(q, self.h, d), k_stride=_rows_view(k, self.h, d), v_stride=_rows_view(v, self.h, d),
                           scale=self.scale, dropout_p=self.p, seed=int(seed), seed_dev=_sd(), out=_ptr(out), out_lo=None,
                           lse=_ptr(lse), dtype=_dt(q))
        return out, lse

    def bwd(self, q, k, v, out, dout, lse, kv_len, seed, out_lo=None):
        """``out_lo``: optional bf16 residual of the (global) output, O = out + out_lo (the ring merges its blocks in fp32 and
        knows it): delta then has fp32-like accuracy."""
        b, lq, hd = q.shape
        lk, d = k.shape[1], hd // self.h
        dq = torch.empty(b, lq, hd, dtype=q.dtype, device=q.device)
        dk = torch.empty(b, lk, hd, dtype=q.dtype, device=q.device)
        dv = torch.empty(b, lk, hd, dtype=q.dtype, device=q.device)
        out, dout, lse = out.contiguous(), dout.contiguous(), lse.contiguous()
        with _span("attn_bwd_d%d" % d, flops=10.0 * b * self.h * lq * lk * d):
            _attention_bwd(q.device, q=_ptr(q), k=_ptr(k), v=_ptr(v), out=_ptr(out), out_lo=_ptr(out_lo), dout=_ptr(dout),
                           lse=_ptr(lse), kv_len=_ptr(kv_len), b=b, h=self.h, lq=lq, lk=lk, d=d, q_stride=_rows_view(q, self.h, d),
                           k_stride=_rows_view(k, self.h, d), v_stride=_rows_view(v, self.h, d), scale=self.scale, dropout_p=self.p,
                           seed=int(seed), seed_dev=_sd(), dq=_ptr(dq), dk=_ptr(dk), dv=_ptr(dv), dq_stride=hd, dk_stride=hd,
                           dv_stride=hd, dtype=_dt(q))
        return dq, dk, dv


def attention_qkv(qkv, kv_len, num_heads, scale, dropout_p=0.0, training=False, cu_seqlens=None, max_len=0, pair_count=None,
                  bias_masters=(), groups=None):
    p = float(dropout_p) if training else 0.0
    return AttentionQKV.apply(qkv, kv_len, num_heads, scale, p, draw_seed() if p > 0 else 0, cu_seqlens, max_len, pair_count,
                              groups, *bias_masters)


SHORT_GROUP_ROWS, SHORT_GROUP_SEQS = 128, 13


def pack_sequence_groups(lens) -> torch.Tensor:
    """Greedy packing of CONSECUTIVE sequences into work items of the short-sequence attention kernels: a group takes
    sequences while its rows stay <= 128 and its count <= 13 (gmlm_hip.h, seq_groups).  ``lens``: host sequence of ints
    (every length <= 128).  Returns the int32 [G + 1] boundaries (host tensor)."""
    bounds, rows, cnt = [0], 0, 0
    for i, n in enumerate(lens):
        n = int(n)
        if n > SHORT_GROUP_ROWS:
            raise ValueError(f"sequence {i} has {n} rows: the short-sequence kernels take <= {SHORT_GROUP_ROWS}")
        if cnt and (rows + n > SHORT_GROUP_ROWS or cnt == SHORT_GROUP_SEQS):
            bounds.append(i)
            rows = cnt = 0
        rows += n
        cnt += 1
    bounds.append(len(lens))
    return torch.tensor(bounds, dtype=torch.int32)


def attention(q, k, v, kv_len, num_heads, scale, dropout_p=0.0, training=False):
    p = float(dropout_p) if training else 0.0
    return Attention.apply(q, k, v, kv_len, num_heads, scale, p, draw_seed() if p > 0 else 0)



# ---------------------------------------------------------------------------------------------
# K8: masked mean pool + row scatter
# ---------------------------------------------------------------------------------------------
class MeanPoolScatter(torch.autograd.Function):
    """plm_embeds[node_idx[b]] = sum_t hs[b,t]*[t<len[b]] / max(len[b],1e-9)  (main.py:351-358), in place.
    hs is [b, l, p] (padded, ``lens``) or [total_rows, p] (packed, ``cu_seqlens``)."""

    @staticmethod
    def forward(ctx, plm_embeds, hs, lens, node_idx, cu_seqlens=None, valid_rows=None):
        """``valid_rows`` (packed): rows of ``hs`` covered by ``cu_seqlens``; rows behind them (padding the token count to a
        friendlier multiple) get a zero gradient."""
        _cuda(hs, plm_embeds)
        hs = hs.contiguous()
        if cu_seqlens is not None:
            b, l, p = cu_seqlens.numel() - 1, 0, hs.shape[-1]
        else:
            b, l, p = hs.shape
        check(lib().gmlm_meanpool_scatter_fwd(_ptr(hs), _ptr(lens), _ptr(node_idx), b, l, p, _ptr(plm_embeds), _dt(hs),
                                              _ptr(cu_seqlens), _stream()), "gmlm_meanpool_scatter_fwd")
        ctx.mark_dirty(plm_embeds)
        ctx.save_for_backward(lens, node_idx, cu_seqlens)
        ctx.cfg = (b, l, p, hs.dtype, tuple(hs.shape), valid_rows)
        return plm_embeds

    @staticmethod
    def backward(ctx, g):
        lens, node_idx, cu_seqlens = ctx.saved_tensors
        b, l, p, dtype, shape, valid_rows = ctx.cfg
        g = g.contiguous().float()
        dhs = torch.empty(shape, dtype=dtype, device=g.device)
        if valid_rows is not None and valid_rows < shape[0]:
            dhs[valid_rows:].zero_()
        check(lib().gmlm_meanpool_scatter_bwd(_ptr(g), _ptr(lens), _ptr(node_idx), b, l, p, _ptr(dhs), _dt(dhs),
                                              _ptr(cu_seqlens), _stream()), "gmlm_meanpool_scatter_bwd")
        # rows written by this micro-batch were overwritten: no gradient flows to their previous value (out of place: g may
        # be the caller's tensor).  The first micro-batch's buffer is a constant and gets nothing.
        dprev = g.index_fill(0, node_idx[:b].long(), 0.0) if ctx.needs_input_grad[0] else None
        return dprev, dhs, None, None, None, None


# ---------------------------------------------------------------------------------------------
# BERT embedding sum (word + token type 0 + position) and its segment-sum backward
# ---------------------------------------------------------------------------------------------
class EmbedSum(torch.autograd.Function):
    """out[t] = word[tok[t]] + type[0] + pos[pos_ids[t]]  (hf:modeling_bert.py:53-108 ahead of the LayerNorm) stored as
    ``out_dtype``: one pass instead of two gathers, two adds and a cast.  Backward: the output gradient is summed per token id
    and per position id with the aggregation kernel over a stable segment sort of the ids (K1 + K2: deterministic, no atomics);
    the type-0 row's gradient is the sum of the position rows' gradients (every token has exactly one position)."""

    @staticmethod
    def forward(ctx, tok, pos_ids, word_w, pos_w, type_w, out_dtype, bad_flag=None):
        """``bad_flag``: optional int32[1] device tensor the kernel sets to 1 when an id lies outside its table (the ids are
        then clamped, never read out of bounds); ``check_embed_ids`` is the raising, synchronising form."""
        _cuda(word_w, pos_w, type_w)
        tok, pos_ids = tok.long().contiguous(), pos_ids.long().contiguous()
        word, pos, typ = _f32c(word_w), _f32c(pos_w), _f32c(type_w)
        rows, p = tok.numel(), word.shape[1]
        out = torch.empty(rows, p, dtype=out_dtype, device=word.device)
        check(lib().gmlm_embed_sum_fwd(_ptr(word), _ptr(pos), _ptr(typ), _ptr(tok), _ptr(pos_ids), rows, p, word.shape[0],
                                       pos.shape[0], _ptr(out), _dt(out), _ptr(bad_flag), _stream()), "gmlm_embed_sum_fwd")
        ctx.save_for_backward(tok, pos_ids)
        ctx.cfg = (word.shape[0], pos.shape[0], type_w.shape[0], p)
        return out

    @staticmethod
    def backward(ctx, g):
        from .graph import _segment_sort
        tok, pos_ids = ctx.saved_tensors
        vocab, npos, ntype, p = ctx.cfg
        g = g.contiguous()
        grads = []
        # The segment sums feed fp32 master tables and a position row sums ~10^3 sequences: they are accumulated AND stored in
        # fp32.  The aggregation kernel keeps one storage dtype for source and result, so a bf16 gradient is widened once
        # ([T, P] fp32 transient: one pass, 1-2 % of the encoder backward) instead of rounding every sum to 8 bits.
        g32 = g if g.dtype == torch.float32 else g.float()
        # Real text makes a few segments very long ([CLS] / [SEP] once per sequence, every position id once per sequence that is
        # long enough, frequent words): segments of more than 64 rows are reduced chunk-wise through a split plan built on the
        # device from this step's rowptr (one lane group walking a 1,257-row - or, at arxiv size, 40,000-row - segment alone was
        # the whole duration of this kernel)
        for ids, nseg in ((tok, vocab), (pos_ids, npos)):
            _, perm, rowptr, _ = _segment_sort(ids, None, None, 1, nseg)
            acc = torch.empty(nseg, p, dtype=torch.float32, device=g.device)
            _spmm(g32, rowptr, perm, None, False, nseg, p, acc, device_split_plan(rowptr, ids.numel()))
            grads.append(acc)
        d_type = torch.zeros(ntype, p, dtype=torch.float32, device=g.device)
        d_type[0] = column_sum(grads[1])                   # (not ATen's global reduction: see column_sum)
        return None, None, grads[0], grads[1], d_type, None, None


def embed_sum(tok, pos_ids, word_w, pos_w, type_w, out_dtype, bad_flag=None):
    return EmbedSum.apply(tok, pos_ids, word_w, pos_w, type_w, out_dtype, bad_flag)


def check_embed_ids(input_ids: torch.Tensor, lens: torch.Tensor, vocab: int, npos: int) -> None:
    """What F.embedding / HF BERT enforce per call (an id outside the table raises), done ONCE for a static id tensor:
    token ids in [0, vocab), sequence lengths <= max_position_embeddings.  One device sync; ``TokenizedTexts`` remembers
    the tables it was checked against."""
    if input_ids.numel() == 0:
        return
    lo, hi, lmax = int(input_ids.min()), int(input_ids.max()), int(lens.max()) if lens.numel() else 0
    if lo < 0 or hi >= vocab:
        raise IndexError(f"token id out of range: ids span [{lo}, {hi}], the word embedding table has {vocab} rows")
    if lmax > npos:
        raise IndexError(f"sequence of {lmax} tokens exceeds max_position_embeddings = {npos}")


# ---------------------------------------------------------------------------------------------
# K9: soft-mask blend
# ---------------------------------------------------------------------------------------------
class SoftMask(torch.autograd.Function):
    """x~[i] = mask[i] ? (1-beta) x[i] + beta*token : x[i]  (main.py:92-99); output dtype / column
    padding (zeros) chosen by the caller so the first RGCN layer gets 16-byte aligned rows."""

    @staticmethod
    def forward(ctx, x, mask, token, beta, out_dtype, out_cols):
        _cuda(x)
        x = x.float().contiguous()
        n, f = x.shape
        out_cols = int(out_cols) if out_cols else f
        m8 = mask.to(torch.uint8).contiguous()
        tok = _f32c(token).view(-1)
        out = torch.empty(n, out_cols, dtype=out_dtype, device=x.device)
        check(lib().gmlm_softmask_blend_fwd(_ptr(x), _ptr(m8), _ptr(tok), float(beta), n, f, _ptr(out), out_cols, _dt(out),
                                            _stream()), "gmlm_softmask_blend_fwd")
        ctx.save_for_backward(m8)
        ctx.cfg = (float(beta), n, f, token.shape)
        return out

    @staticmethod
    def backward(ctx, g):
        (m8,) = ctx.saved_tensors
        beta, n, f, tshape = ctx.cfg
        g = g.float().contiguous()
        dtok = torch.empty(f, dtype=torch.float32, device=g.device)
        ws = _ws(lib().gmlm_softmask_blend_bwd_workspace_bytes(n, f), g.device)
        check(lib().gmlm_softmask_blend_bwd(_ptr(g), g.stride(0), _ptr(m8), beta, n, f, _ptr(dtok), _ptr(ws), ws.numel(),
                                            _stream()), "gmlm_softmask_blend_bwd")
        return None, None, dtok.view(tshape), None, None, None


def soft_masking_gnn_input(x, gnn_perturb_mask, mask_token_embed, beta=0.7, out_dtype=torch.float32, out_cols=None):
    """Drop-in for main.py:92-99 (same name / argument order); gradient flows to ``mask_token_embed``."""
    return SoftMask.apply(x, gnn_perturb_mask.to(x.device), mask_token_embed.to(x.device), beta, out_dtype, out_cols)


# ---------------------------------------------------------------------------------------------
# bias + GELU (+dropout)
# ---------------------------------------------------------------------------------------------
class BiasGelu(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, bias, p, seed):
        _cuda(x)
        shape = x.shape
        f = shape[-1]
        x2 = x.contiguous().view(-1, f)
        bf = None if bias is None else _f32c(bias)
        y = torch.empty_like(x2)
        sd = ctx.sd = _sd()
        check(lib().gmlm_bias_gelu_fwd(_ptr(x2), _ptr(bf), x2.shape[0], f, float(p), seed, sd, _ptr(y), _dt(x2), _stream()),
              "gmlm_bias_gelu_fwd")
        ctx.save_for_backward(x2, bf)
        ctx.cfg = (float(p), seed, shape, bias is not None)
        return y.view(shape)

    @staticmethod
    def backward(ctx, gy):
        x2, bf = ctx.saved_tensors
        p, seed, shape, has_bias = ctx.cfg
        rows, f = x2.shape
        gy2 = gy.contiguous().view(rows, f).to(x2.dtype)
        dx = torch.empty_like(x2)
        dbias = torch.empty(f, dtype=torch.float32, device=x2.device) if has_bias else None
        ws = _ws(lib().gmlm_bias_gelu_bwd_workspace_bytes(rows, f, _dt(x2)), x2.device)
        sd = ctx.sd
        check(lib().gmlm_bias_gelu_bwd(_ptr(gy2), _ptr(x2), _ptr(bf), rows, f, p, seed, sd, _ptr(dx), _ptr(dbias), _dt(x2),
                                       _ptr(ws), ws.numel(), _stream()), "gmlm_bias_gelu_bwd")
        return dx.view(shape), dbias, None, None


def bias_gelu(x, bias, p=0.0, training=False):
    p = float(p) if training else 0.0
    return BiasGelu.apply(x, bias, p, draw_seed() if p > 0 else 0)


# ---------------------------------------------------------------------------------------------
# Pre-norm decoder-style encoder (Qwen3 geometry): add + RMSNorm, Q/K head norm + RoPE, SwiGLU, causal GQA attention
# ---------------------------------------------------------------------------------------------
class _AddNorm(torch.autograd.Function):
    """(s, y) with s = a + b in the compute dtype (``b`` None: s is ``a``) and y = norm(s) * w (+ ``beta``, may be None).
    ``s`` is the residual stream handed to the next add; its gradient and y's meet in ONE backward kernel.
    ``ln``: LayerNorm (gmlm_add_layernorm_*: a row mean is saved beside rstd, ``beta`` is taken), else RMSNorm (gmlm_add_rmsnorm_*)."""

    @staticmethod
    def forward(ctx, ln, a, b, w, beta, eps):
        _cuda(a)
        shape = a.shape
        f = shape[-1]
        a2 = a.contiguous().view(-1, f)
        b2 = None if b is None else b.to(a.dtype).contiguous().view(-1, f)
        rows = a2.shape[0]
        wf = _f32c(w)
        s2 = torch.empty_like(a2) if b2 is not None else None
        y = torch.empty_like(a2)
        if ln:
            bf = None if beta is None else _f32c(beta)
            stats = torch.empty(2, rows, dtype=torch.float32, device=a.device)          # mean | rstd
            check(lib().gmlm_add_layernorm_fwd(_ptr(a2), _ptr(b2), _ptr(wf), _ptr(bf), rows, f, float(eps), _ptr(s2), _ptr(y),
                                               _ptr(stats[0]), _ptr(stats[1]), _dt(a2), _stream()), "gmlm_add_layernorm_fwd")
        else:
            stats = torch.empty(rows, dtype=torch.float32, device=a.device)             # rstd
            check(lib().gmlm_add_rmsnorm_fwd(_ptr(a2), _ptr(b2), _ptr(wf), rows, f, float(eps), _ptr(s2), _ptr(y), _ptr(stats),
                                             _dt(a2), _stream()), "gmlm_add_rmsnorm_fwd")
        if s2 is None:
            s2 = a2
        ctx.save_for_backward(s2, wf, stats)
        ctx.cfg = (ln, shape, b is not None, beta is not None)
        return (s2.view(shape) if b is not None else a.view_as(a)), y.view(shape)

    @staticmethod
    def backward(ctx, gs, gy):
        s2, wf, stats = ctx.saved_tensors
        ln, shape, has_b, has_beta = ctx.cfg
        rows, f = s2.shape
        if gy is None:
            gy = torch.zeros_like(s2)
        gy2 = gy.contiguous().view(rows, f).to(s2.dtype)
        gs2 = None if gs is None else gs.contiguous().view(rows, f).to(s2.dtype)
        ds = torch.empty_like(s2)
        dw = torch.empty(2 if has_beta else 1, f, dtype=torch.float32, device=s2.device)   # dw (| dbeta): one buffer
        if ln:
            ws = _ws(lib().gmlm_add_layernorm_bwd_workspace_bytes(rows, f), s2.device)
            check(lib().gmlm_add_layernorm_bwd(_ptr(gy2), _ptr(gs2), _ptr(s2), _ptr(wf), _ptr(stats[0]), _ptr(stats[1]), rows, f, _ptr(ds),
                                               _ptr(dw), _ptr(dw[1]) if has_beta else None, _dt(s2), _ptr(ws), ws.numel(), _stream()),
                  "gmlm_add_layernorm_bwd")
        else:
            ws = _ws(lib().gmlm_add_rmsnorm_bwd_workspace_bytes(rows, f), s2.device)
            check(lib().gmlm_add_rmsnorm_bwd(_ptr(gy2), _ptr(gs2), _ptr(s2), _ptr(wf), _ptr(stats), rows, f, _ptr(ds), _ptr(dw),
                                             _dt(s2), _ptr(ws), ws.numel(), _stream()), "gmlm_add_rmsnorm_bwd")
        ds = ds.view(shape)
        return None, ds, (ds if has_b else None), dw[0], (dw[1] if has_beta else None), None


def add_rmsnorm(a, b, w, eps=1e-6):
    """-> (a + b, RMSNorm(a + b) * w); ``b`` may be None."""
    return _AddNorm.apply(False, a, b, w, None, eps)


def _qkv_rows(qkv: torch.Tensor, width: int):
    """[..., >= width] rows with a contiguous last dim and one row stride -> (tokens, row stride in elements)."""
    if qkv.stride(-1) != 1 or qkv.shape[-1] < width:
        raise ValueError(f"fused projection rows must be contiguous and at least {width} wide")
    tokens = qkv.numel() // qkv.shape[-1]
    stride = qkv.stride(-2)
    if qkv.dim() == 3 and qkv.shape[0] > 1 and tokens > 0 and qkv.stride(0) != qkv.shape[1] * stride:
        raise ValueError("fused projection rows must have batch stride = l * row stride")
    return tokens, stride


def _rope_fwd(qkv, qw, kw, cs, seq_len, hq, hkv, eps, pos_ids=None):
    """``pos_ids`` (int32 [tokens]) given: the position of row t is pos_ids[t] and ``seq_len`` is not used."""
    tokens, stride = _qkv_rows(qkv, (hq + 2 * hkv) * 128)
    qk = torch.empty(*qkv.shape[:-1], (hq + hkv) * 128, dtype=qkv.dtype, device=qkv.device)
    rstd = torch.empty(tokens, hq + hkv, dtype=torch.float32, device=qkv.device)
    if pos_ids is not None:
        check(lib().gmlm_qknorm_rope_pos_fwd(_ptr(qkv), stride, _ptr(qw), _ptr(kw), _ptr(cs), cs.shape[0], tokens, _ptr(pos_ids), hq,
                                             hkv, 128, float(eps), _ptr(qk), (hq + hkv) * 128, _ptr(rstd), _dt(qkv), _stream()),
              "gmlm_qknorm_rope_pos_fwd")
        return qk, rstd
    check(lib().gmlm_qknorm_rope_fwd(_ptr(qkv), stride, _ptr(qw), _ptr(kw), _ptr(cs), cs.shape[0], tokens, seq_len, hq, hkv, 128,
                                     float(eps), _ptr(qk), (hq + hkv) * 128, _ptr(rstd), _dt(qkv), _stream()),
          "gmlm_qknorm_rope_fwd")
    return qk, rstd


def _rope_bwd_(dqkv, qkv, qw, kw, cs, rstd, seq_len, hq, hkv, pos_ids=None):
    """In place on the Q | K columns of ``dqkv``; returns the fp32 [2, 128] weight gradients."""
    tokens, stride = _qkv_rows(qkv, (hq + 2 * hkv) * 128)
    _, dstride = _qkv_rows(dqkv, (hq + hkv) * 128)
    dwt = torch.empty(2, 128, dtype=torch.float32, device=qkv.device)
    ws = _ws(lib().gmlm_qknorm_rope_bwd_workspace_bytes(tokens, hq, hkv, _dt(qkv)), qkv.device)
    if pos_ids is not None:
        check(lib().gmlm_qknorm_rope_pos_bwd(_ptr(dqkv), dstride, _ptr(qkv), stride, _ptr(qw), _ptr(kw), _ptr(cs), cs.shape[0],
                                             _ptr(rstd), tokens, _ptr(pos_ids), hq, hkv, 128, _ptr(dwt), _ptr(dwt[1]), _dt(qkv),
                                             _ptr(ws), ws.numel(), _stream()), "gmlm_qknorm_rope_pos_bwd")
        return dwt
    check(lib().gmlm_qknorm_rope_bwd(_ptr(dqkv), dstride, _ptr(qkv), stride, _ptr(qw), _ptr(kw), _ptr(cs), cs.shape[0], _ptr(rstd),
                                     tokens, seq_len, hq, hkv, 128, _ptr(dwt), _ptr(dwt[1]), _dt(qkv), _ptr(ws), ws.numel(),
                                     _stream()), "gmlm_qknorm_rope_bwd")
    return dwt


def _pos_arg(qkv, pos_ids):
    """Positions of packed rows: int32 [tokens] on the rows' device."""
    if qkv.dim() != 2:
        raise ValueError("packed fused projection output must be [tokens, (hq + 2 hkv) * 128]")
    if pos_ids.dim() != 1 or pos_ids.numel() != qkv.shape[0] or pos_ids.device != qkv.device or pos_ids.is_floating_point() \
            or pos_ids.dtype == torch.bool:
        raise ValueError("pos_ids must be an integer [tokens] tensor on the device of the rows")
    return pos_ids.to(torch.int32).contiguous()


def _rope_args(qkv, qw, kw, cs, packed=False):
    if not packed and qkv.dim() != 3:
        raise ValueError("fused projection output must be [b, l, (hq + 2 hkv) * 128]")
    if cs.dtype != torch.float32 or cs.dim() != 3 or tuple(cs.shape[1:]) != (2, 64) or not cs.is_contiguous():
        raise ValueError("cos / sin table must be a contiguous fp32 [max_len, 2, 64] tensor")
    return _f32c(qw), _f32c(kw)


class QKNormRope(torch.autograd.Function):
    """Rotated, head-normalised [q | k] of a fused [b, l, (hq + 2 hkv) * 128] projection output (positions 0..l-1), or, with
    ``pos_ids`` (integer [tokens]), of packed [tokens, (hq + 2 hkv) * 128] rows at the positions given."""

    @staticmethod
    def forward(ctx, qkv, qw, kw, cs, hq, hkv, eps, pos_ids=None):
        _cuda(qkv)
        qwf, kwf = _rope_args(qkv, qw, kw, cs, pos_ids is not None)
        pos = None if pos_ids is None else _pos_arg(qkv, pos_ids)
        qk, rstd = _rope_fwd(qkv, qwf, kwf, cs, qkv.shape[-2], hq, hkv, eps, pos)
        ctx.save_for_backward(qkv, qwf, kwf, cs, rstd, pos)
        ctx.cfg = (hq, hkv)
        return qk

    @staticmethod
    def backward(ctx, g):
        qkv, qwf, kwf, cs, rstd, pos = ctx.saved_tensors
        hq, hkv = ctx.cfg
        n = (hq + hkv) * 128
        dqkv = torch.zeros(*qkv.shape[:-1], (hq + 2 * hkv) * 128, dtype=qkv.dtype, device=qkv.device)   # V columns: no gradient from here
        dqkv[..., :n].copy_(g)
        dwt = _rope_bwd_(dqkv, qkv, qwf, kwf, cs, rstd, qkv.shape[-2], hq, hkv, pos)
        if dqkv.shape[-1] != qkv.shape[-1]:
            dqkv = torch.nn.functional.pad(dqkv, (0, qkv.shape[-1] - dqkv.shape[-1]))
        return dqkv, dwt[0], dwt[1], None, None, None, None, None


def qknorm_rope(qkv, q_weight, k_weight, cos_sin, hq, hkv, eps=1e-6, pos_ids=None):
    return QKNormRope.apply(qkv, q_weight, k_weight, cos_sin, hq, hkv, eps, pos_ids)


def _gqa_entry(d, bidir):
    """(entry-point stem, span stem) of a grouped-KV attention family: causal at d = 128 (gmlm_attention_causal_d128_*) or 64
    (gmlm_attention_causal_d64_*, include/gmlm_hip_gqa.h), or ``bidir``: no causal mask, d = 64 / 128 (gmlm_attention_bidir_gqa_*,
    include/gmlm_hip_bidir.h).  One argument list for all of them.  d = 256 (gmlm_attention_gqa_d256_*, include/gmlm_hip_gqa_wide.h):
    one family for both masks, whose argument list has ``causal`` after the dropout rate (``_gqa_causal_arg``) and whose workspace
    queries are named ``*_bwd_workspace_bytes`` (``_gqa_ws``)."""
    if d == GQA_WIDE_HEAD_DIM:
        return "gmlm_attention_gqa_d256", "attn_gqaw"
    return ("gmlm_attention_bidir_gqa", "attn_bidir") if bidir else (f"gmlm_attention_causal_d{d}", "attn_causal")


def _gqa_causal_arg(d, bidir):
    return (0 if bidir else 1,) if d == GQA_WIDE_HEAD_DIM else ()


def _gqa_ws(stem, d, varlen=""):
    return stem + varlen + ("_bwd_workspace_bytes" if d == GQA_WIDE_HEAD_DIM else "_workspace_bytes")


def _causal_fwd(q, k, v, kv_len, hq, hkv, scale, want_lo, d=128, bidir=False):
    stem, tag = _gqa_entry(d, bidir)
    b, l = q.shape[0], q.shape[1]
    qs, ks, vs = _rows_view(q, hq, d), _rows_view(k, hkv, d), _rows_view(v, hkv, d)
    out = torch.empty(b, l, hq * d, dtype=q.dtype, device=q.device)
    lse = torch.empty(b, hq, l, dtype=torch.float32, device=q.device)
    out_lo = torch.empty_like(out) if want_lo else None
    name = stem + "_fwd"
    with _span(f"{tag}_fwd_d{d}", flops=(4.0 if bidir else 2.0) * b * hq * l * l * d):
        check(getattr(lib(), name)(_ptr(q), _ptr(k), _ptr(v), _ptr(kv_len), b, hq, hkv, l, k.shape[1], d, qs, ks, vs, float(scale), 0.0,
                                   *_gqa_causal_arg(d, bidir), _ptr(out), _ptr(out_lo), _ptr(lse), _dt(q), _stream()), name)
    return out, out_lo, lse


def _causal_bwd(q, k, v, out, out_lo, gout, lse, kv_len, hq, hkv, scale, dq, dk, dv, d=128, bidir=False):
    stem, tag = _gqa_entry(d, bidir)
    b, l = q.shape[0], q.shape[1]
    gout = gout.contiguous().to(q.dtype)
    ws = _ws(getattr(lib(), _gqa_ws(stem, d))(b, hq, l), q.device)
    name = stem + "_bwd"
    with _span(f"{tag}_bwd_d{d}", flops=(10.0 if bidir else 5.0) * b * hq * l * l * d):
        check(getattr(lib(), name)(_ptr(q), _ptr(k), _ptr(v), _ptr(out), _ptr(out_lo), _ptr(gout), _ptr(lse), _ptr(kv_len), b, hq, hkv, l,
                                   k.shape[1], d, q.stride(1), k.stride(1), v.stride(1), float(scale), 0.0, *_gqa_causal_arg(d, bidir),
                                   _ptr(dq), _ptr(dk), _ptr(dv), dq.stride(1), dk.stride(1), dv.stride(1), _dt(q), _ptr(ws), ws.numel(),
                                   _stream()), name)


class CausalAttention(torch.autograd.Function):
    """out[b, l, hq*d] = softmax(causal + key-padding mask(q k^T * scale)) v with hq query heads sharing hkv KV heads, head dim
    d = 128 (or 64: the gmlm_attention_causal_d64_* family).  q [b, l, hq*d], k / v [b, l, hkv*d] (strided slices of a fused
    buffer are fine); kv_len int32 [b] or None.  The three gradients are views of ONE fused [b, l, (hq + 2 hkv) * d] buffer.
    ``bidir``: the key-padding mask alone (gmlm_attention_bidir_gqa_*, d = 64 or 128)."""

    @staticmethod
    def forward(ctx, q, k, v, kv_len, hq, hkv, scale, d=128, bidir=False):
        _cuda(q, k, v)
        want_lo = q.dtype == torch.bfloat16 and any(t.requires_grad for t in (q, k, v))
        out, out_lo, lse = _causal_fwd(q, k, v, kv_len, hq, hkv, scale, want_lo, d, bidir)
        ctx.save_for_backward(q, k, v, out, lse, kv_len, out_lo)
        ctx.cfg = (hq, hkv, float(scale), d, bidir)
        return out

    @staticmethod
    def backward(ctx, gout):
        q, k, v, out, lse, kv_len, out_lo = ctx.saved_tensors
        hq, hkv, scale, d, bidir = ctx.cfg
        b, l = q.shape[0], q.shape[1]
        nq, nk = hq * d, hkv * d
        dqkv = torch.empty(b, l, nq + 2 * nk, dtype=q.dtype, device=q.device)
        dq, dk, dv = dqkv[..., :nq], dqkv[..., nq:nq + nk], dqkv[..., nq + nk:]
        _causal_bwd(q, k, v, out, out_lo, gout, lse, kv_len, hq, hkv, scale, dq, dk, dv, d, bidir)
        return dq, dk, dv, None, None, None, None, None, None


def causal_attention(q, k, v, kv_len, hq, hkv, scale, d=128):
    return CausalAttention.apply(q, k, v, kv_len, hq, hkv, scale, d, False)


class RopeCausalAttention(torch.autograd.Function):
    """Head norm + RoPE + causal GQA attention of a fused [b, l, (hq + 2 hkv) * 128] projection output in one autograd node:
    V is read from the fused rows in place, and the backward lets the attention kernels write dq | dk | dv into ONE fused
    buffer that the head-norm backward then finishes in place, so a single data-gradient GEMM follows."""

    @staticmethod
    def forward(ctx, qkv, qw, kw, cs, kv_len, hq, hkv, scale, eps):
        _cuda(qkv)
        qwf, kwf = _rope_args(qkv, qw, kw, cs)
        if qkv.shape[-1] != (hq + 2 * hkv) * 128:
            raise ValueError("fused projection output must be [b, l, (hq + 2 hkv) * 128]")
        nq, nk = hq * 128, hkv * 128
        qk, rstd = _rope_fwd(qkv, qwf, kwf, cs, qkv.shape[1], hq, hkv, eps)
        want_lo = qkv.dtype == torch.bfloat16 and (qkv.requires_grad or qw.requires_grad or kw.requires_grad)
        out, out_lo, lse = _causal_fwd(qk[..., :nq], qk[..., nq:], qkv[..., nq + nk:], kv_len, hq, hkv, scale, want_lo)
        ctx.save_for_backward(qkv, qk, qwf, kwf, cs, rstd, out, lse, kv_len, out_lo)
        ctx.cfg = (hq, hkv, float(scale))
        return out

    @staticmethod
    def backward(ctx, gout):
        qkv, qk, qwf, kwf, cs, rstd, out, lse, kv_len, out_lo = ctx.saved_tensors
        hq, hkv, scale = ctx.cfg
        nq, nk = hq * 128, hkv * 128
        dqkv = torch.empty_like(qkv, memory_format=torch.contiguous_format)
        _causal_bwd(qk[..., :nq], qk[..., nq:], qkv[..., nq + nk:], out, out_lo, gout, lse, kv_len, hq, hkv, scale,
                    dqkv[..., :nq], dqkv[..., nq:nq + nk], dqkv[..., nq + nk:])
        dwt = _rope_bwd_(dqkv, qkv, qwf, kwf, cs, rstd, qkv.shape[1], hq, hkv)
        return dqkv, dwt[0], dwt[1], None, None, None, None, None, None


def rope_causal_attention(qkv, q_weight, k_weight, cos_sin, kv_len, hq, hkv, scale, eps=1e-6):
    return RopeCausalAttention.apply(qkv, q_weight, k_weight, cos_sin, kv_len, hq, hkv, scale, eps)


def _varlen_args(rows, cu_seqlens, max_len):
    """cu_seqlens int32 [S + 1] on the rows' device; -> (S, max_len)."""
    if cu_seqlens is None or cu_seqlens.dtype != torch.int32 or cu_seqlens.dim() != 1 or cu_seqlens.numel() < 1 \
            or not cu_seqlens.is_contiguous() or cu_seqlens.device != rows.device:
        raise ValueError("cu_seqlens must be a contiguous int32 [sequences + 1] tensor on the device of the rows")
    if int(max_len) <= 0:
        raise ValueError(f"max_len must be positive, got {max_len}")
    return cu_seqlens.numel() - 1, int(max_len)


def _packed_stride(t: torch.Tensor, h: int, d: int = 128):
    if t.dim() != 2 or t.stride(-1) != 1 or t.shape[-1] != h * d:
        raise ValueError(f"packed attention operands must be [tokens, heads * {d}] with a contiguous last dim")
    return t.stride(0)


def _causal_varlen_fwd(q, k, v, cu, s, max_len, hq, hkv, scale, want_lo, d=128, bidir=False, groups=None):
    """``groups`` set = the caller decided for the short-sequence route (``_gqa_short_path``): no out_lo comes back."""
    stem, tag = _gqa_entry(d, bidir)
    t = q.shape[0]
    qs, ks, vs = _packed_stride(q, hq, d), _packed_stride(k, hkv, d), _packed_stride(v, hkv, d)
    if k.shape[0] != t or v.shape[0] != t:
        raise ValueError("packed q, k and v must have the same number of rows")
    out = torch.empty(t, hq * d, dtype=q.dtype, device=q.device)
    lse = torch.empty(hq, t, dtype=torch.float32, device=q.device)
    if groups is not None:
        name = "gmlm_attention_gqa_short_fwd"
        with _span(f"{tag}_short_fwd_d{d}", flops=(4.0 if bidir else 2.0) * s * hq * max_len * max_len * d):
            check(getattr(lib(), name)(_ptr(q), _ptr(k), _ptr(v), _ptr(cu), s, max_len, t, hq, hkv, d, qs, ks, vs, float(scale), 0.0,
                                       0 if bidir else 1, _ptr(groups), _groups_arg(groups, cu), _ptr(out), _ptr(lse), _dt(q),
                                       _stream()), name)
        return out, None, lse
    out_lo = torch.empty_like(out) if want_lo else None
    name = stem + "_varlen_fwd"
    with _span(f"{tag}_varlen_fwd_d{d}", flops=(4.0 if bidir else 2.0) * s * hq * max_len * max_len * d):
        check(getattr(lib(), name)(_ptr(q), _ptr(k), _ptr(v), _ptr(cu), s, max_len, t, hq, hkv, d, qs, ks, vs, float(scale), 0.0,
                                   *_gqa_causal_arg(d, bidir), _ptr(out), _ptr(out_lo), _ptr(lse), _dt(q), _stream()), name)
    return out, out_lo, lse


def _causal_varlen_bwd(q, k, v, out, out_lo, gout, lse, cu, s, max_len, hq, hkv, scale, dq, dk, dv, d=128, bidir=False, groups=None):
    stem, tag = _gqa_entry(d, bidir)
    t = q.shape[0]
    gout = gout.contiguous().to(q.dtype)
    if groups is not None:                  # the short-sequence route: delta is formed in the kernel, no out / out_lo / workspace
        name = "gmlm_attention_gqa_short_bwd"
        with _span(f"{tag}_short_bwd_d{d}", flops=(10.0 if bidir else 5.0) * s * hq * max_len * max_len * d):
            check(getattr(lib(), name)(_ptr(q), _ptr(k), _ptr(v), _ptr(gout), _ptr(lse), _ptr(cu), s, max_len, t, hq, hkv, d,
                                       q.stride(0), k.stride(0), v.stride(0), float(scale), 0.0, 0 if bidir else 1, _ptr(groups),
                                       _groups_arg(groups, cu), _ptr(dq), _ptr(dk), _ptr(dv), dq.stride(0), dk.stride(0),
                                       dv.stride(0), _dt(q), _stream()), name)
        return
    ws = _ws(getattr(lib(), _gqa_ws(stem, d, "_varlen"))(t, hq), q.device)
    name = stem + "_varlen_bwd"
    with _span(f"{tag}_varlen_bwd_d{d}", flops=(10.0 if bidir else 5.0) * s * hq * max_len * max_len * d):
        check(getattr(lib(), name)(_ptr(q), _ptr(k), _ptr(v), _ptr(out), _ptr(out_lo), _ptr(gout), _ptr(lse), _ptr(cu), s, max_len, t, hq,
                                   hkv, d, q.stride(0), k.stride(0), v.stride(0), float(scale), 0.0, *_gqa_causal_arg(d, bidir), _ptr(dq), _ptr(dk),
                                   _ptr(dv), dq.stride(0), dk.stride(0), dv.stride(0), _dt(q), _ptr(ws), ws.numel(), _stream()), name)


class CausalAttentionVarlen(torch.autograd.Function):
    """``CausalAttention`` on a packed batch: q [T, hq*d], k / v [T, hkv*d] (strided slices of a fused buffer are fine),
    sequence i = rows [cu_seqlens[i], cu_seqlens[i+1]) (int32 [S + 1]; a sequence may be empty, none is longer than
    ``max_len``), query i of a sequence sees its keys 0..i.  The sequences cover all T rows: a row that belongs to none is
    neither read nor written, so its output and gradient rows would be uninitialised.  The three gradients are views of ONE fused [T, (hq + 2 hkv) * d] buffer.
    ``groups`` (int32 [G + 1], ``pack_sequence_groups``): where ``_gqa_short_path`` holds, the short-sequence kernels run, work
    item g = sequences [groups[g], groups[g+1]); the node then saves neither ``out`` nor ``out_lo``.  Otherwise it is ignored."""

    @staticmethod
    def forward(ctx, q, k, v, cu_seqlens, max_len, hq, hkv, scale, d=128, bidir=False, groups=None):
        _cuda(q, k, v)
        s, max_len = _varlen_args(q, cu_seqlens, max_len)
        if not _gqa_short_path(groups, q.dtype, d, max_len, s, hq):
            groups = None
        want_lo = groups is None and q.dtype == torch.bfloat16 and any(t.requires_grad for t in (q, k, v))
        out, out_lo, lse = _causal_varlen_fwd(q, k, v, cu_seqlens, s, max_len, hq, hkv, scale, want_lo, d, bidir, groups)
        ctx.save_for_backward(q, k, v, out if groups is None else None, lse, cu_seqlens, out_lo, groups)
        ctx.cfg = (s, max_len, hq, hkv, float(scale), d, bidir)
        return out

    @staticmethod
    def backward(ctx, gout):
        q, k, v, out, lse, cu, out_lo, groups = ctx.saved_tensors
        s, max_len, hq, hkv, scale, d, bidir = ctx.cfg
        nq, nk = hq * d, hkv * d
        dqkv = torch.empty(q.shape[0], nq + 2 * nk, dtype=q.dtype, device=q.device)
        dq, dk, dv = dqkv[:, :nq], dqkv[:, nq:nq + nk], dqkv[:, nq + nk:]
        _causal_varlen_bwd(q, k, v, out, out_lo, gout, lse, cu, s, max_len, hq, hkv, scale, dq, dk, dv, d, bidir, groups)
        return dq, dk, dv, None, None, None, None, None, None, None, None


def causal_attention_varlen(q, k, v, cu_seqlens, max_len, hq, hkv, scale, d=128, groups=None):
    return CausalAttentionVarlen.apply(q, k, v, cu_seqlens, max_len, hq, hkv, scale, d, False, groups)


class RopeCausalAttentionVarlen(torch.autograd.Function):
    """``RopeCausalAttention`` on packed [T, (hq + 2 hkv) * 128] rows: head norm + RoPE at ``pos_ids`` (integer [T]) + causal GQA
    attention per sequence of ``cu_seqlens`` in one autograd node.  V is read from the fused rows in place; the backward
    writes dq | dk | dv into ONE fused buffer that the head-norm backward finishes in place."""

    @staticmethod
    def forward(ctx, qkv, qw, kw, cs, pos_ids, cu_seqlens, max_len, hq, hkv, scale, eps):
        _cuda(qkv)
        qwf, kwf = _rope_args(qkv, qw, kw, cs, True)
        pos = _pos_arg(qkv, pos_ids)
        if qkv.shape[-1] != (hq + 2 * hkv) * 128:
            raise ValueError("fused projection output must be [tokens, (hq + 2 hkv) * 128]")
        s, max_len = _varlen_args(qkv, cu_seqlens, max_len)
        nq, nk = hq * 128, hkv * 128
        qk, rstd = _rope_fwd(qkv, qwf, kwf, cs, 0, hq, hkv, eps, pos)
        want_lo = qkv.dtype == torch.bfloat16 and (qkv.requires_grad or qw.requires_grad or kw.requires_grad)
        out, out_lo, lse = _causal_varlen_fwd(qk[:, :nq], qk[:, nq:], qkv[:, nq + nk:], cu_seqlens, s, max_len, hq, hkv, scale, want_lo)
        ctx.save_for_backward(qkv, qk, qwf, kwf, cs, rstd, out, lse, cu_seqlens, pos, out_lo)
        ctx.cfg = (s, max_len, hq, hkv, float(scale))
        return out

    @staticmethod
    def backward(ctx, gout):
        qkv, qk, qwf, kwf, cs, rstd, out, lse, cu, pos, out_lo = ctx.saved_tensors
        s, max_len, hq, hkv, scale = ctx.cfg
        nq, nk = hq * 128, hkv * 128
        dqkv = torch.empty_like(qkv, memory_format=torch.contiguous_format)
        _causal_varlen_bwd(qk[:, :nq], qk[:, nq:], qkv[:, nq + nk:], out, out_lo, gout, lse, cu, s, max_len, hq, hkv, scale,
                           dqkv[:, :nq], dqkv[:, nq:nq + nk], dqkv[:, nq + nk:])
        dwt = _rope_bwd_(dqkv, qkv, qwf, kwf, cs, rstd, 0, hq, hkv, pos)
        return dqkv, dwt[0], dwt[1], None, None, None, None, None, None, None, None


def rope_causal_attention_varlen(qkv, q_weight, k_weight, cos_sin, pos_ids, cu_seqlens, max_len, hq, hkv, scale, eps=1e-6):
    return RopeCausalAttentionVarlen.apply(qkv, q_weight, k_weight, cos_sin, pos_ids, cu_seqlens, max_len, hq, hkv, scale, eps)


class _GLU(torch.autograd.Function):
    """[..., 2 I] = [gate | up] -> act(gate) * up [..., I]; ``stem``: gmlm_<stem>_fwd / _bwd (swiglu: SiLU, geglu: erf GELU)."""

    @staticmethod
    def forward(ctx, stem, gu):
        _cuda(gu)
        shape = gu.shape
        inter = shape[-1] // 2
        g2 = gu.contiguous().view(-1, 2 * inter)
        y = torch.empty(g2.shape[0], inter, dtype=gu.dtype, device=gu.device)
        name = f"gmlm_{stem}_fwd"
        check(getattr(lib(), name)(_ptr(g2), g2.shape[0], inter, _ptr(y), _dt(g2), _stream()), name)
        ctx.save_for_backward(g2)
        ctx.cfg = (stem, shape)
        return y.view(*shape[:-1], inter)

    @staticmethod
    def backward(ctx, gy):
        (g2,) = ctx.saved_tensors
        stem, shape = ctx.cfg
        rows, inter = g2.shape[0], g2.shape[1] // 2
        gy2 = gy.contiguous().view(rows, inter).to(g2.dtype)
        dgu = torch.empty_like(g2)
        name = f"gmlm_{stem}_bwd"
        check(getattr(lib(), name)(_ptr(gy2), _ptr(g2), rows, inter, _ptr(dgu), _dt(g2), _stream()), name)
        return None, dgu.view(shape)


def swiglu(gate_up):
    return _GLU.apply("swiglu", gate_up)


# ---------------------------------------------------------------------------------------------
# ModernBERT encoder: add + LayerNorm, GeGLU, rotary embedding at d = 64 in place + (band-limited) attention
# ---------------------------------------------------------------------------------------------
ADD_LAYERNORM_MAX_F = 4096       # GMLM_ADD_LAYERNORM_MAX_F (include/gmlm_hip_modernbert.h)


def add_layernorm(a, b, gamma, beta=None, eps=1e-5):
    """-> (a + b, LayerNorm(a + b) * gamma + beta); ``b`` and ``beta`` may be None."""
    return _AddNorm.apply(True, a, b, gamma, beta, eps)


def geglu(u):
    return _GLU.apply("geglu", u)


def geglu_tanh(u):
    """[..., 2 I] = [gate | up] -> gelu_tanh(gate) * up, the tanh form of GELU (Gemma3: ``gelu_pytorch_tanh``; gmlm_geglu_tanh_*)."""
    return _GLU.apply("geglu_tanh", u)


def rope64_(qkv, cos_sin, h, seq_len=0, pos_ids=None, inverse=False):
    """Rotate (``inverse``: rotate back) the Q | K columns of fused [.., 3 * h * 64] rows IN PLACE; positions are row % seq_len,
    or ``pos_ids`` (int32 [tokens]) when given.  Outside autograd: the building block of ``RopeWindowAttention``."""
    tokens, stride = _qkv_rows(qkv, 3 * h * 64)
    if cos_sin.dtype != torch.float32 or cos_sin.dim() != 3 or tuple(cos_sin.shape[1:]) != (2, 32) or not cos_sin.is_contiguous():
        raise ValueError("cos / sin table must be a contiguous fp32 [max_len, 2, 32] tensor")
    name = "gmlm_rope64_bwd" if inverse else "gmlm_rope64_fwd"
    check(getattr(lib(), name)(_ptr(qkv), stride, _ptr(cos_sin), cos_sin.shape[0], tokens, int(seq_len), _ptr(pos_ids), h, 64, _dt(qkv),
                               _stream()), name)
    return qkv


def window_cuts(layer_type: str, window: int, max_len: int) -> bool:
    """The routing rule of a ModernBERT layer's attention: only a ``sliding_attention`` layer whose band |i - j| <= window
    actually hides a key of the call's longest sequence (max_len > window + 1) runs the band-limited kernels; a full-attention
    layer, and a sliding layer on sequences of at most window + 1 tokens (the band is vacuous), take the ``attention_qkv`` path."""
    return layer_type == "sliding_attention" and int(max_len) > int(window) + 1


def _window_fwd(qkv, kv_len, h, scale, window, cu, max_len, want_lo):
    packed = cu is not None
    l, hd3 = (qkv.shape[0] if packed else qkv.shape[1]), qkv.shape[-1]
    b = cu.numel() - 1 if packed else qkv.shape[0]
    hd = hd3 // 3
    out = torch.empty(qkv.shape[:-1] + (hd,), dtype=qkv.dtype, device=qkv.device)
    lse = torch.empty((h, l) if packed else (b, h, l), dtype=torch.float32, device=qkv.device)
    out_lo = torch.empty_like(out) if want_lo else None
    q, k, v = qkv[..., :hd], qkv[..., hd:2 * hd], qkv[..., 2 * hd:]
    rows = int(max_len) if packed else l
    span = min(rows, 2 * int(window) + 1)
    with _span("attn_window_fwd_d64", flops=4.0 * h * 64 * b * rows * span):
        check(lib().gmlm_attention_window_fwd(_ptr(q), _ptr(k), _ptr(v), _ptr(kv_len), b, h, l, l, 64, hd3, hd3, hd3, float(scale), 0.0,
                                              int(window), _ptr(out), _ptr(out_lo), _ptr(lse), _dt(qkv), _ptr(cu), int(max_len),
                                              _stream()), "gmlm_attention_window_fwd")
    return out, out_lo, lse


def _window_bwd(qkv, out, out_lo, gout, lse, kv_len, h, scale, window, cu, max_len, dqkv):
    packed = cu is not None
    l, hd3 = (qkv.shape[0] if packed else qkv.shape[1]), qkv.shape[-1]
    b = cu.numel() - 1 if packed else qkv.shape[0]
    hd = hd3 // 3
    gout = gout.contiguous().to(qkv.dtype)
    q, k, v = qkv[..., :hd], qkv[..., hd:2 * hd], qkv[..., 2 * hd:]
    dq, dk, dv = dqkv[..., :hd], dqkv[..., hd:2 * hd], dqkv[..., 2 * hd:]
    ws = _ws(lib().gmlm_attention_window_workspace_bytes(1 if packed else b, h, l), qkv.device)
    rows = int(max_len) if packed else l
    span = min(rows, 2 * int(window) + 1)
    with _span("attn_window_bwd_d64", flops=10.0 * h * 64 * b * rows * span):
        check(lib().gmlm_attention_window_bwd(_ptr(q), _ptr(k), _ptr(v), _ptr(out), _ptr(out_lo), _ptr(gout), _ptr(lse), _ptr(kv_len),
                                              b, h, l, l, 64, hd3, hd3, hd3, float(scale), 0.0, int(window), _ptr(dq), _ptr(dk),
                                              _ptr(dv), hd3, hd3, hd3, _dt(qkv), _ptr(cu), int(max_len), _ptr(ws), ws.numel(),
                                              _stream()), "gmlm_attention_window_bwd")


class _RopeAttention(torch.autograd.Function):
    """Rotary embedding at d = 64 IN PLACE on the Q | K columns of a fused [.., 3 * h * 64] projection output (marked dirty and
    returned beside the context), then attention on the rotated buffer, in one autograd node.  ``window`` None: the
    ``AttentionQKV`` path (padded, packed and short-sequence kernels, ``groups``); an int: the band-limited kernels.  The
    backward runs the attention backward into ONE dqkv buffer, then the inverse rotation in place on it."""

    @staticmethod
    def forward(ctx, qkv, cs, kv_len, h, scale, window, pos_ids, cu_seqlens, max_len, pair_count, groups):
        _cuda(qkv)
        if not qkv.is_contiguous() or qkv.shape[-1] != 3 * h * 64:
            raise ValueError("fused projection output must be contiguous [.., 3 * h * 64] rows")
        packed = cu_seqlens is not None
        if packed:
            pos_ids = _pos_arg(qkv, pos_ids)
            _varlen_args(qkv, cu_seqlens, max_len)
        elif qkv.dim() != 3:
            raise ValueError("padded fused projection output must be [b, l, 3 * h * 64]")
        seq_len = 0 if packed else qkv.shape[1]
        rope64_(qkv, cs, h, seq_len, pos_ids if packed else None)
        ctx.mark_dirty(qkv)
        ctx.rope = (cs, h, seq_len, pos_ids if packed else None)
        ctx.window = window
        if window is None:
            out = AttentionQKV.forward(ctx, qkv, kv_len, h, scale, 0.0, 0, cu_seqlens, max_len, pair_count, groups)
        else:
            out, out_lo, lse = _window_fwd(qkv, kv_len, h, scale, window, cu_seqlens, max_len,
                                           qkv.dtype == torch.bfloat16 and qkv.requires_grad)
            ctx.save_for_backward(qkv, out, out_lo, lse, kv_len, cu_seqlens)
            ctx.wcfg = (float(scale), int(max_len))
        return out, qkv

    @staticmethod
    def backward(ctx, gout, _gqkv):
        cs, h, seq_len, pos = ctx.rope
        if ctx.window is None:
            dqkv = AttentionQKV.backward(ctx, gout)[0]
        else:
            qkv, out, out_lo, lse, kv_len, cu = ctx.saved_tensors
            scale, max_len = ctx.wcfg
            dqkv = torch.empty_like(qkv)
            _window_bwd(qkv, out, out_lo, gout, lse, kv_len, h, scale, ctx.window, cu, max_len, dqkv)
        rope64_(dqkv, cs, h, seq_len, pos, inverse=True)
        return (dqkv,) + (None,) * 10


def _own_rows(qkv):
    """Autograd cannot rebase a VIEW that a node with more than one output modifies in place (``dense.LinearBf16x3`` returns its
    [T, N] product viewed as [b, l, N]): such a buffer is copied once; the native GEMM's output is rotated where it lies."""
    return qkv.clone() if qkv._is_view() else qkv


def rope_attention(qkv, cos_sin, kv_len, num_heads, scale, layer_type="full_attention", window=0):
    """Padded layout: rotary embedding in place on ``qkv`` [b, l, 3 * h * 64] (positions 0..l-1), then full or band-limited
    attention by ``window_cuts``; ``kv_len`` int32 [b] or None.  ``qkv`` is overwritten with its rotated form (a view is copied first: ``_own_rows``)."""
    w = int(window) if window_cuts(layer_type, window, qkv.shape[1]) else None
    return _RopeAttention.apply(_own_rows(qkv), cos_sin, kv_len, num_heads, scale, w, None, None, 0, None, None)[0]


def rope_attention_varlen(qkv, cos_sin, pos_ids, cu_seqlens, max_len, num_heads, scale, layer_type="full_attention", window=0,
                          pair_count=None, groups=None):
    """Packed layout: ``qkv`` [T, 3 * h * 64] rows at positions ``pos_ids``, sequences by ``cu_seqlens`` (none longer than
    ``max_len``, which also decides whether the band cuts).  ``qkv`` is overwritten with its rotated form."""
    w = int(window) if window_cuts(layer_type, window, max_len) else None
    return _RopeAttention.apply(_own_rows(qkv), cos_sin, None, num_heads, scale, w, pos_ids, cu_seqlens, int(max_len), pair_count, groups)[0]


# ---------------------------------------------------------------------------------------------
# Llama / Qwen2 / Mistral encoders: rotary embedding over the Q | K head rows in place + causal GQA attention at d = 64 / 128
# (include/gmlm_hip_gqa.h); EuroBERT encoders: the same with bidirectional GQA attention (include/gmlm_hip_bidir.h)
# ---------------------------------------------------------------------------------------------
GQA_HEAD_DIMS = (64, 128)        # gmlm_rope_heads_*; causal attention: gmlm_attention_causal_d64_* / _d128_*
GQA_WIDE_HEAD_DIM = 256          # gmlm_attention_gqa_d256_*, gmlm_qknorm_rope_d256_* (Gemma3 encoders, include/gmlm_hip_gqa_wide.h)


def rope_heads_(qkv, cos_sin, heads, d, seq_len=0, pos_ids=None, inverse=False):
    """Rotate (``inverse``: rotate back) the first ``heads`` = hq + hkv head rows of ``d`` (64 or 128) elements of every fused
    [.., >= heads * d] row IN PLACE; what follows them (V) is not touched.  Positions are row % seq_len, or ``pos_ids`` (int32
    [tokens]) when given.  Outside autograd: the building block of ``_RopeCausalGQA``."""
    tokens, stride = _qkv_rows(qkv, heads * d)
    if cos_sin.dtype != torch.float32 or cos_sin.dim() != 3 or tuple(cos_sin.shape[1:]) != (2, d // 2) or not cos_sin.is_contiguous():
        raise ValueError(f"cos / sin table must be a contiguous fp32 [max_len, 2, {d // 2}] tensor")
    name = "gmlm_rope_heads_bwd" if inverse else "gmlm_rope_heads_fwd"
    check(getattr(lib(), name)(_ptr(qkv), stride, _ptr(cos_sin), cos_sin.shape[0], tokens, int(seq_len), _ptr(pos_ids), heads, d,
                               _dt(qkv), _stream()), name)
    return qkv


class _RopeCausalGQA(torch.autograd.Function):
    """Rotary embedding IN PLACE on the Q | K columns of a fused [.., (hq + 2 hkv) * d] projection output (marked dirty and
    returned beside the context), then causal attention with grouped KV heads on the rotated buffer (d = 64:
    gmlm_attention_causal_d64_*, d = 128: gmlm_attention_causal_d128_*; ``bidir``: without the causal mask,
    gmlm_attention_bidir_gqa_* at either head dim), in one autograd node.  Padded ([b, l, .] with
    ``kv_len``) or packed ([T, .] with ``pos_ids``, ``cu_seqlens``, ``max_len``).  The backward runs the attention backward into
    ONE dqkv buffer, then the inverse rotation in place on it: a single data-gradient GEMM follows."""

    @staticmethod
    def forward(ctx, qkv, cs, kv_len, hq, hkv, d, scale, pos_ids, cu_seqlens, max_len, bidir, groups=None):
        _cuda(qkv)
        if d not in GQA_HEAD_DIMS:
            raise ValueError(f"head dim {d}: the rotary / grouped-KV attention kernels take {GQA_HEAD_DIMS}")
        if not qkv.is_contiguous() or qkv.shape[-1] != (hq + 2 * hkv) * d:
            raise ValueError("fused projection output must be contiguous [.., (hq + 2 hkv) * d] rows")
        packed = cu_seqlens is not None
        if packed:
            pos_ids = _pos_arg(qkv, pos_ids)
            s, max_len = _varlen_args(qkv, cu_seqlens, max_len)
        elif qkv.dim() != 3:
            raise ValueError("padded fused projection output must be [b, l, (hq + 2 hkv) * d]")
        seq_len = 0 if packed else qkv.shape[1]
        pos = pos_ids if packed else None
        rope_heads_(qkv, cs, hq + hkv, d, seq_len, pos)
        ctx.mark_dirty(qkv)
        nq, nk = hq * d, hkv * d
        q, k, v = qkv[..., :nq], qkv[..., nq:nq + nk], qkv[..., nq + nk:]
        if not (packed and _gqa_short_path(groups, qkv.dtype, d, max_len, s, hq)):
            groups = None                                       # only the packed short-sequence kernels take groups
        want_lo = groups is None and qkv.dtype == torch.bfloat16 and qkv.requires_grad
        if packed:
            out, out_lo, lse = _causal_varlen_fwd(q, k, v, cu_seqlens, s, max_len, hq, hkv, scale, want_lo, d, bidir, groups)
        else:
            out, out_lo, lse = _causal_fwd(q, k, v, kv_len, hq, hkv, scale, want_lo, d, bidir)
        # the short-sequence backward reads neither the forward output nor its residual
        ctx.save_for_backward(qkv, cs, out if groups is None else None, out_lo, lse, kv_len, cu_seqlens, pos, groups)
        ctx.cfg = (hq, hkv, d, float(scale), seq_len, int(max_len), bidir)
        return out, qkv

    @staticmethod
    def backward(ctx, gout, _gqkv):
        qkv, cs, out, out_lo, lse, kv_len, cu, pos, groups = ctx.saved_tensors
        hq, hkv, d, scale, seq_len, max_len, bidir = ctx.cfg
        nq, nk = hq * d, hkv * d
        q, k, v = qkv[..., :nq], qkv[..., nq:nq + nk], qkv[..., nq + nk:]
        dqkv = torch.empty_like(qkv)
        dq, dk, dv = dqkv[..., :nq], dqkv[..., nq:nq + nk], dqkv[..., nq + nk:]
        if cu is not None:
            _causal_varlen_bwd(q, k, v, out, out_lo, gout, lse, cu, cu.numel() - 1, max_len, hq, hkv, scale, dq, dk, dv, d, bidir, groups)
        else:
            _causal_bwd(q, k, v, out, out_lo, gout, lse, kv_len, hq, hkv, scale, dq, dk, dv, d, bidir)
        rope_heads_(dqkv, cs, hq + hkv, d, seq_len, pos, inverse=True)
        return (dqkv,) + (None,) * 11


def rope_causal_gqa(qkv, cos_sin, kv_len, hq, hkv, d, scale):
    """Padded layout: rotary embedding in place on ``qkv`` [b, l, (hq + 2 hkv) * d] (positions 0..l-1), then causal GQA
    attention; ``kv_len`` int32 [b] or None.  ``qkv`` is overwritten with its rotated form (a view is copied first: ``_own_rows``)."""
    return _RopeCausalGQA.apply(_own_rows(qkv), cos_sin, kv_len, hq, hkv, d, scale, None, None, 0, False)[0]


def rope_causal_gqa_varlen(qkv, cos_sin, pos_ids, cu_seqlens, max_len, hq, hkv, d, scale, groups=None):
    """Packed layout: ``qkv`` [T, (hq + 2 hkv) * d] rows at positions ``pos_ids``, sequences by ``cu_seqlens`` (none longer than
    ``max_len``).  ``qkv`` is overwritten with its rotated form.  ``groups`` (``pack_sequence_groups``): the short-sequence
    kernels where ``_gqa_short_path`` holds."""
    return _RopeCausalGQA.apply(_own_rows(qkv), cos_sin, None, hq, hkv, d, scale, pos_ids, cu_seqlens, int(max_len), False, groups)[0]


# EuroBERT encoders: the same node and the same two attention nodes without the causal mask (include/gmlm_hip_bidir.h)
def bidir_gqa_attention(q, k, v, kv_len, hq, hkv, scale, d):
    """``causal_attention`` without the causal mask: query i sees every key of its sequence below ``kv_len``; d = 64 or 128."""
    return CausalAttention.apply(q, k, v, kv_len, hq, hkv, scale, d, True)


def bidir_gqa_attention_varlen(q, k, v, cu_seqlens, max_len, hq, hkv, scale, d, groups=None):
    return CausalAttentionVarlen.apply(q, k, v, cu_seqlens, max_len, hq, hkv, scale, d, True, groups)


def rope_bidir_gqa(qkv, cos_sin, kv_len, hq, hkv, d, scale):
    """``rope_causal_gqa`` with bidirectional attention: rotary embedding in place on ``qkv`` [b, l, (hq + 2 hkv) * d], then
    grouped-KV attention over all keys below ``kv_len`` (int32 [b] or None).  ``qkv`` is overwritten with its rotated form."""
    return _RopeCausalGQA.apply(_own_rows(qkv), cos_sin, kv_len, hq, hkv, d, scale, None, None, 0, True)[0]


def rope_bidir_gqa_varlen(qkv, cos_sin, pos_ids, cu_seqlens, max_len, hq, hkv, d, scale, groups=None):
    """``rope_causal_gqa_varlen`` with bidirectional attention on packed ``qkv`` [T, (hq + 2 hkv) * d] rows."""
    return _RopeCausalGQA.apply(_own_rows(qkv), cos_sin, None, hq, hkv, d, scale, pos_ids, cu_seqlens, int(max_len), True, groups)[0]


# ---------------------------------------------------------------------------------------------
# attention with a learned relative-position bias at head dim 64 (MPNet encoders; include/gmlm_hip_relbias.h)
# ---------------------------------------------------------------------------------------------
RELBIAS_MAX_LEN = 512      # GMLM_RELBIAS_MAX_LEN


class AttentionRelBiasQKV(torch.autograd.Function):
    """Self-attention on a fused QKV buffer whose scores get ``rel_bias[h, M - 1 + (j - i)]`` (fp32 [h, 2M - 1], M >= the
    longest sequence), at head dim 64.  Called like ``AttentionQKV``:

    padded mode: qkv [b, l, 3*h*64], kv_len int32 [b] or None.
    packed mode: qkv [total_rows, 3*h*64], cu_seqlens int32 [b+1], max_len = longest sequence; positions count from the start
    of each sequence.

    Returns the context; the backward writes dq|dk|dv into ONE buffer of qkv's layout and returns the gradient of ``rel_bias``
    (fp32, every entry written, fixed summation order).  Dropout is the replayable mask of every other attention kernel."""

    @staticmethod
    def forward(ctx, qkv, rel_bias, kv_len, h, scale, p, seed, cu_seqlens, max_len):
        _cuda(qkv, rel_bias)
        qkv = qkv.contiguous()
        packed = cu_seqlens is not None
        if packed:
            _varlen_args(qkv, cu_seqlens, max_len)
            l, hd3 = qkv.shape
            b = cu_seqlens.numel() - 1
        else:
            b, l, hd3 = qkv.shape
        hd = hd3 // 3
        d = hd // h
        if rel_bias.dtype != torch.float32 or rel_bias.dim() != 2 or rel_bias.shape[0] != h or rel_bias.shape[1] % 2 != 1:
            raise ValueError("rel_bias must be an fp32 [heads, 2M - 1] tensor")
        m = (rel_bias.shape[1] + 1) // 2
        bias = rel_bias.detach().contiguous()
        q, k, v = qkv[..., :hd], qkv[..., hd:2 * hd], qkv[..., 2 * hd:]
        out = torch.empty(qkv.shape[:-1] + (hd,), dtype=qkv.dtype, device=qkv.device)
        lse = torch.empty((h, l) if packed else (b, h, l), dtype=torch.float32, device=qkv.device)
        out_lo = torch.empty_like(out) if (qkv.dtype == torch.bfloat16 and (qkv.requires_grad or rel_bias.requires_grad)) else None
        flops = 4.0 * h * d * (float(max_len) * l if packed else float(b) * l * l)
        with _span("attn_relbias_fwd_d%d" % d, flops=flops):
            sd = ctx.sd = _sd()
            check(lib().gmlm_attention_relbias_fwd(_ptr(q), _ptr(k), _ptr(v), _ptr(kv_len), b, h, l, l, d, hd3, hd3, hd3, float(scale),
                                                   float(p), seed, sd, _ptr(bias), m, _ptr(out), _ptr(out_lo), _ptr(lse), _dt(qkv),
                                                   _ptr(cu_seqlens), int(max_len), _stream()), "gmlm_attention_relbias_fwd")
        ctx.save_for_backward(qkv, bias, lse, kv_len, cu_seqlens, out, out_lo)
        ctx.cfg = (h, float(scale), float(p), seed, int(max_len), b, l, m, flops)
        return out

    @staticmethod
    def backward(ctx, gout):
        qkv, bias, lse, kv_len, cu_seqlens, out, out_lo = ctx.saved_tensors
        h, scale, p, seed, max_len, b, l, m, flops = ctx.cfg
        hd3 = qkv.shape[-1]
        hd = hd3 // 3
        d = hd // h
        gout = gout.contiguous().to(qkv.dtype)
        q, k, v = qkv[..., :hd], qkv[..., hd:2 * hd], qkv[..., 2 * hd:]
        dqkv = torch.empty_like(qkv)
        dq, dk, dv = dqkv[..., :hd], dqkv[..., hd:2 * hd], dqkv[..., 2 * hd:]
        dbias = torch.empty_like(bias)
        ws = _ws(lib().gmlm_attention_relbias_workspace_bytes(b, h, l, max_len if cu_seqlens is not None else 0, m), qkv.device)
        with _span("attn_relbias_bwd_d%d" % d, flops=3.5 * flops):          # the backward's five GEMMs + two of them again
            check(lib().gmlm_attention_relbias_bwd(_ptr(q), _ptr(k), _ptr(v), _ptr(out), _ptr(out_lo), _ptr(gout), _ptr(lse),
                                                   _ptr(kv_len), b, h, l, l, d, hd3, hd3, hd3, scale, p, seed, ctx.sd, _ptr(bias), m,
                                                   _ptr(dq), _ptr(dk), _ptr(dv), _ptr(dbias), hd3, hd3, hd3, _dt(qkv),
                                                   _ptr(cu_seqlens), max_len, ws.data_ptr(), ws.numel(), _stream()),
                  "gmlm_attention_relbias_bwd")
        if b == 0 or l == 0:
            dbias.zero_()                                                    # a call with nothing to do launches nothing
        return dqkv, dbias, None, None, None, None, None, None, None


def attention_relbias_qkv(qkv, rel_bias, kv_len, num_heads, scale, dropout_p=0.0, training=False):
    """Padded form: qkv [b, l, 3 * h * 64], kv_len int32 [b] or None, rel_bias fp32 [h, 2M - 1] with M >= l."""
    p = float(dropout_p) if training else 0.0
    return AttentionRelBiasQKV.apply(qkv, rel_bias, kv_len, num_heads, scale, p, draw_seed() if p > 0 else 0, None, 0)


def attention_relbias_qkv_varlen(qkv, rel_bias, cu_seqlens, max_len, num_heads, scale, dropout_p=0.0, training=False):
    """Packed form: qkv [T, 3 * h * 64], sequences by ``cu_seqlens`` (none longer than ``max_len``), rel_bias fp32 [h, 2M - 1]
    with M >= max_len."""
    p = float(dropout_p) if training else 0.0
    return AttentionRelBiasQKV.apply(qkv, rel_bias, None, num_heads, scale, p, draw_seed() if p > 0 else 0, cu_seqlens, int(max_len))


# ---------------------------------------------------------------------------------------------
# disentangled self-attention at head dim 64 (DeBERTa-v2 / v3 encoders; include/gmlm_hip_disent.h)
# ---------------------------------------------------------------------------------------------
DISENT_MAX_LEN = 512      # GMLM_DISENT_MAX_LEN


class AttentionDisentQKV(torch.autograd.Function):
    """Self-attention on a fused QKV buffer whose scores are ``(q_i . k_j + c2p[i, h, c] + p2c[j, h, c]) * scale`` with
    ``c = col[M - 1 + (i - j)]``, at head dim 64: c2p / p2c fp32 [h, rows of qkv, W], col int32 [2M - 1] with values in [0, W),
    monotone, M >= the longest sequence.  Called like ``AttentionRelBiasQKV``:

    padded mode: qkv [b, l, 3*h*64], tables [h, b * l, W], kv_len int32 [b] or None.
    packed mode: qkv [total_rows, 3*h*64], tables [h, total_rows, W], cu_seqlens int32 [b+1], max_len = longest sequence.

    Returns the context; the backward writes dq|dk|dv (the content-content parts) into ONE buffer of qkv's layout and returns the
    gradients of the two tables (fp32, every entry written, fixed summation order)."""

    @staticmethod
    def forward(ctx, qkv, c2p, p2c, col, kv_len, h, scale, p, seed, cu_seqlens, max_len):
        _cuda(qkv, c2p, p2c, col)
        qkv = qkv.contiguous()
        packed = cu_seqlens is not None
        if packed:
            _varlen_args(qkv, cu_seqlens, max_len)
            l, hd3 = qkv.shape
            b = cu_seqlens.numel() - 1
        else:
            b, l, hd3 = qkv.shape
        hd = hd3 // 3
        d = hd // h
        if col.dtype != torch.int32 or col.dim() != 1 or col.numel() % 2 != 1:
            raise ValueError("col must be an int32 [2M - 1] tensor")
        m = (col.numel() + 1) // 2
        want = (h, qkv.numel() // hd3 if hd3 else 0)
        for name, t in (("c2p", c2p), ("p2c", p2c)):
            if t.dtype != torch.float32 or t.dim() != 3 or tuple(t.shape[:2]) != want or t.shape != c2p.shape:
                raise ValueError(f"{name} must be an fp32 [heads, rows, W] = {list(want)} + [W] tensor, one shape for both tables")
        wcols = c2p.shape[-1]
        c2p, p2c, col = c2p.detach().contiguous(), p2c.detach().contiguous(), col.contiguous()
        q, k, v = qkv[..., :hd], qkv[..., hd:2 * hd], qkv[..., 2 * hd:]
        out = torch.empty(qkv.shape[:-1] + (hd,), dtype=qkv.dtype, device=qkv.device)
        lse = torch.empty((h, l) if packed else (b, h, l), dtype=torch.float32, device=qkv.device)
        need_grad = any(ctx.needs_input_grad[:3])
        out_lo = torch.empty_like(out) if (qkv.dtype == torch.bfloat16 and need_grad) else None
        flops = 4.0 * h * d * (float(max_len) * l if packed else float(b) * l * l)
        with _span("attn_disent_fwd_d%d" % d, flops=flops):
            sd = ctx.sd = _sd()
            check(lib().gmlm_attention_disent_fwd(_ptr(q), _ptr(k), _ptr(v), _ptr(kv_len), b, h, l, l, d, hd3, hd3, hd3, float(scale),
                                                  float(p), seed, sd, _ptr(c2p), _ptr(p2c), _ptr(col), m, wcols, _ptr(out),
                                                  _ptr(out_lo), _ptr(lse), _dt(qkv), _ptr(cu_seqlens), int(max_len), _stream()),
                  "gmlm_attention_disent_fwd")
        ctx.save_for_backward(qkv, c2p, p2c, col, lse, kv_len, cu_seqlens, out, out_lo)
        ctx.cfg = (h, float(scale), float(p), seed, int(max_len), b, l, m, wcols, flops)
        return out

    @staticmethod
    def backward(ctx, gout):
        qkv, c2p, p2c, col, lse, kv_len, cu_seqlens, out, out_lo = ctx.saved_tensors
        h, scale, p, seed, max_len, b, l, m, wcols, flops = ctx.cfg
        hd3 = qkv.shape[-1]
        hd = hd3 // 3
        d = hd // h
        gout = gout.contiguous().to(qkv.dtype)
        q, k, v = qkv[..., :hd], qkv[..., hd:2 * hd], qkv[..., 2 * hd:]
        dqkv = torch.empty_like(qkv)
        dq, dk, dv = dqkv[..., :hd], dqkv[..., hd:2 * hd], dqkv[..., 2 * hd:]
        dc2p, dp2c = torch.empty_like(c2p), torch.empty_like(p2c)
        ws = _ws(lib().gmlm_attention_disent_workspace_bytes(b, h, l, max_len if cu_seqlens is not None else 0), qkv.device)
        with _span("attn_disent_bwd_d%d" % d, flops=4.5 * flops):          # the backward's five GEMMs + two of them twice again
            check(lib().gmlm_attention_disent_bwd(_ptr(q), _ptr(k), _ptr(v), _ptr(out), _ptr(out_lo), _ptr(gout), _ptr(lse),
                                                  _ptr(kv_len), b, h, l, l, d, hd3, hd3, hd3, scale, p, seed, ctx.sd, _ptr(c2p),
                                                  _ptr(p2c), _ptr(col), m, wcols, _ptr(dq), _ptr(dk), _ptr(dv), _ptr(dc2p),
                                                  _ptr(dp2c), hd3, hd3, hd3, _dt(qkv), _ptr(cu_seqlens), max_len, ws.data_ptr(),
                                                  ws.numel(), _stream()), "gmlm_attention_disent_bwd")
        if b == 0 or l == 0:
            dc2p.zero_()                                                     # a call with nothing to do launches nothing
            dp2c.zero_()
        return dqkv, dc2p, dp2c, None, None, None, None, None, None, None, None


def attention_disent_qkv(qkv, c2p, p2c, col, kv_len, num_heads, scale, dropout_p=0.0, training=False):
    """Padded form: qkv [b, l, 3 * h * 64], c2p / p2c fp32 [h, b * l, W], col int32 [2M - 1] with M >= l, kv_len int32 [b] or None."""
    p = float(dropout_p) if training else 0.0
    return AttentionDisentQKV.apply(qkv, c2p, p2c, col, kv_len, num_heads, scale, p, draw_seed() if p > 0 else 0, None, 0)


def attention_disent_qkv_varlen(qkv, c2p, p2c, col, cu_seqlens, max_len, num_heads, scale, dropout_p=0.0, training=False):
    """Packed form: qkv [T, 3 * h * 64], c2p / p2c fp32 [h, T, W], sequences by ``cu_seqlens`` (none longer than ``max_len``),
    col int32 [2M - 1] with M >= max_len."""
    p = float(dropout_p) if training else 0.0
    return AttentionDisentQKV.apply(qkv, c2p, p2c, col, None, num_heads, scale, p, draw_seed() if p > 0 else 0, cu_seqlens, int(max_len))


# ---------------------------------------------------------------------------------------------
# Gemma3 encoders (include/gmlm_hip_gqa_wide.h): the sandwich RMSNorm pair and head norm + rotary embedding + grouped-KV attention
# at head dim 256; ``geglu_tanh`` is above, the plain attention nodes are CausalAttention / CausalAttentionVarlen with d = 256
# ---------------------------------------------------------------------------------------------
from .ops_gemma import gqa_d256_attention, gqa_d256_attention_varlen, rope_gqa_d256, rope_gqa_d256_varlen, sandwich_rmsnorm  # noqa: E402,F401
from .ops_gemma import gqa_d256_band_attention, gqa_d256_band_attention_varlen  # noqa: E402,F401
from .ops_softcap import gqa_d256_softcap_attention, gqa_d256_softcap_attention_varlen, rope_heads_d256_  # noqa: E402,F401
from .ops_softcap import rope_softcap_gqa_d256, rope_softcap_gqa_d256_varlen  # noqa: E402,F401
