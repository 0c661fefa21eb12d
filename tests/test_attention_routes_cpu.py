"""Which entry point the ops layer calls, and with which argument in which position (no GPU needed).

``ops.lib`` is replaced by a recorder whose attributes log ``(name, args)`` and return 0 (64 for a ``*_workspace_bytes``);
``ops._cuda``, ``ops._stream`` and ``ops.check`` are made inert, so ``Attention``, ``AttentionQKV``, ``AttentionBlock`` and
``BiasResLayerNorm`` run forward and backward on small CPU tensors.  Every recorded call is mapped onto the parameter names of
the parsed headers and compared, name by name, with one expectation dict per case: the entry point chosen, each pointer
against the ``data_ptr()`` of the tensor it must be, each stride / size / dtype code / max_len / num_groups, which optional
pointers are NULL, and that the workspace size came from the chosen family's function.  A pointer of a buffer the op
allocates and keeps to itself (the workspace, the bias-sum partials) is only required to be non-NULL."""
import os

import pytest
import torch

from conftest import ROOT
from gmlm_amd import _lib, nn as gnn, ops
from test_abi_contract_cpu import parse_header

PROTOS = {}
for _h in ("gmlm_hip.h", "gmlm_hip_d32.h", "gmlm_hip_wide.h"):
    PROTOS.update(parse_header(open(os.path.join(ROOT, "include", _h)).read()))

STREAM = 0x57EA0
WS_BYTES = 64
SOME = object()          # "any non-NULL pointer"
CODE = {torch.float32: _lib.F32, torch.bfloat16: _lib.BF16}
DTYPES = [torch.bfloat16, torch.float32]

# head dim -> (forward entry, backward entry, workspace entry and the names of its arguments)
FAMILY = {32: ("gmlm_attention_d32_fwd", "gmlm_attention_d32_bwd", "gmlm_attention_d32_bwd_workspace_bytes", "b h lq"),
          64: ("gmlm_attention_fwd", "gmlm_attention_bwd", "gmlm_attention_bwd_workspace_bytes", "b h lq lk d"),
          128: ("gmlm_attention_d128_fwd", "gmlm_attention_d128_bwd", "gmlm_attention_d128_workspace_bytes", "b h lq"),
          256: ("gmlm_attention_wide_fwd", "gmlm_attention_wide_bwd", "gmlm_attention_wide_bwd_workspace_bytes", "b h lq")}
FAMILY[96] = FAMILY[64]
FAMILY[384] = FAMILY[512] = FAMILY[256]


class Recorder:
    def __init__(self):
        self.calls, self.checked = [], []

    def __getattr__(self, name):
        def fn(*args):
            self.calls.append((name, args))
            return WS_BYTES if name.endswith("workspace_bytes") else 0
        return fn

    def take(self):
        """The calls since the last take, each launching one followed by the name `check` was given for it."""
        calls, checked = self.calls[:], self.checked[:]
        del self.calls[:], self.checked[:]
        assert [n for n, _ in calls if not n.endswith("workspace_bytes")] == checked
        return calls


@pytest.fixture
def rec(monkeypatch):
    r = Recorder()
    monkeypatch.setattr(ops, "lib", lambda: r)
    monkeypatch.setattr(ops, "_cuda", lambda *ts: None)
    monkeypatch.setattr(ops, "_stream", lambda: STREAM)
    monkeypatch.setattr(ops, "check", lambda rc, what="": r.checked.append(what))
    monkeypatch.setattr(ops, "SEED_DEVICE", None)
    return r


def ptr(t, elems=0):
    return None if t is None else t.data_ptr() + elems * t.element_size()


def assert_call(call, name, want):
    """`call` is entry point `name`, and each of its arguments, by the header's parameter name, is what `want` says."""
    got_name, args = call
    assert got_name == name
    names = [n for _, n in PROTOS[name][1]]
    assert len(args) == len(names), f"{name}: {len(args)} arguments for {len(names)} parameters"
    for n, a in zip(names, args):
        w = want[n]                                     # KeyError: the expectation does not cover this parameter
        if w is SOME:
            assert isinstance(a, int) and a != 0, f"{name}({n}) must be a non-NULL pointer, got {a!r}"
        else:
            assert type(a) is type(w) and a == w, f"{name}({n}) = {a!r}, expected {w!r}"


def assert_ws_call(call, head_dim, **sizes):
    name, names = FAMILY[head_dim][2], FAMILY[head_dim][3].split()
    assert call == (name, tuple(sizes[n] for n in names))
    assert names == [n for _, n in PROTOS[name][1]]


# what every non-causal attention call has in common; entries of ABI positions a family lacks are simply not looked at
def common(q, k, v, kv_len, b, h, lq, lk, d, strides, scale, p, seed, dtype, **more):
    want = dict(q=ptr(q), k=ptr(k), v=ptr(v), kv_len=ptr(kv_len), b=b, h=h, lq=lq, lk=lk, d=d, q_stride=strides[0],
                k_stride=strides[1], v_stride=strides[2], scale=float(scale), dropout_p=float(p), seed=seed, seed_dev=None,
                dtype=CODE[dtype], cu_seqlens=None, max_len=0, seq_groups=None, num_groups=0, dbias_partial=None, dbias=None,
                workspace=SOME, workspace_bytes=WS_BYTES, stream=STREAM)
    want.update(more)
    return want


# ------------------------------------------------------------------------------------------------------------ Attention
@pytest.mark.parametrize("fused", [False, True], ids=["contiguous", "slices"])
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp32"])
@pytest.mark.parametrize("d", [32, 64, 96, 128, 256, 384, 512])
def test_attention(rec, d, dtype, fused):
    b, h, hd = 2, 2, 2 * d
    if fused:
        lq = lk = 2
        buf = torch.zeros(b, lq, 3 * hd, dtype=dtype, requires_grad=True)
        q, k, v = buf[..., :hd], buf[..., hd:2 * hd], buf[..., 2 * hd:]
        strides = (3 * hd,) * 3
    else:
        lq, lk = 2, 3
        q = torch.zeros(b, lq, hd, dtype=dtype, requires_grad=True)
        k, v = (torch.zeros(b, lk, hd, dtype=dtype, requires_grad=True) for _ in range(2))
        strides = (hd,) * 3
    kv_len = torch.tensor([3, 1], dtype=torch.int32)
    scale, p, seed = 0.375, 0.25, 1234
    out = ops.Attention.apply(q, k, v, kv_len, h, scale, p, seed)
    saved = out.grad_fn.saved_tensors
    assert len(saved) == 7 and [ptr(t) for t in saved[:3]] == [ptr(q), ptr(k), ptr(v)] and ptr(saved[3]) == ptr(out)
    lse, out_lo = saved[4], saved[6]
    assert tuple(lse.shape) == (b, h, lq) and lse.dtype == torch.float32 and tuple(out.shape) == (b, lq, hd)
    assert (out_lo is not None) == (dtype == torch.bfloat16)      # b*h = 4 pairs: never the short-sequence path
    want = common(q, k, v, kv_len, b, h, lq, lk, d, strides, scale, p, seed, dtype, out=ptr(out), out_lo=ptr(out_lo), lse=ptr(lse))
    fwd, = rec.take()
    assert_call(fwd, FAMILY[d][0], want)

    gout = torch.ones_like(out)
    dq, dk, dv = torch.autograd.grad(out, (q, k, v), gout)
    assert tuple(dq.shape) == (b, lq, hd) and tuple(dk.shape) == tuple(dv.shape) == (b, lk, hd)
    want.update(dout=ptr(gout), dq=ptr(dq), dk=ptr(dk), dv=ptr(dv), dq_stride=hd, dk_stride=hd, dv_stride=hd)
    ws, bwd = rec.take()
    assert_ws_call(ws, d, b=b, h=h, lq=lq, lk=lk, d=d)
    assert_call(bwd, FAMILY[d][1], want)


def test_attention_without_grad_or_kv_len_keeps_no_residual(rec):
    q = torch.zeros(1, 2, 64, dtype=torch.bfloat16)
    out = ops.Attention.apply(q, q, q, None, 1, 1.0, 0.0, 0)
    (name, args), = rec.take()
    want = common(q, q, q, None, 1, 1, 2, 2, 64, (64,) * 3, 1.0, 0.0, 0, torch.bfloat16, out=ptr(out), out_lo=None, lse=SOME)
    assert_call((name, args), "gmlm_attention_fwd", want)


# --------------------------------------------------------------------------------------------------------- AttentionQKV
def _qkv_case(rec, d, dtype, mode, masters, b, h, seq):
    """One forward + backward of AttentionQKV.  mode: padded / packed / groups; `seq` rows per sequence."""
    hd, hd3 = h * d, 3 * h * d
    packed = mode != "padded"
    if packed:
        l = b * seq
        qkv = torch.zeros(l, hd3, dtype=dtype, requires_grad=True)
        cu = torch.arange(0, l + 1, seq, dtype=torch.int32)
        kv_len, max_len = None, seq
    else:
        l = seq
        qkv = torch.zeros(b, l, hd3, dtype=dtype, requires_grad=True)
        cu, kv_len, max_len = None, torch.full((b,), seq, dtype=torch.int32), 0
    groups = torch.tensor([0, b // 2, b], dtype=torch.int32) if mode == "groups" else None
    bias = tuple(torch.zeros(hd, requires_grad=True) for _ in range(3)) if masters else ()
    scale, p, seed = 0.5, 0.125, 77
    short = dtype == torch.bfloat16 and d == 64 and seq <= 128 and b * h >= 512
    out = ops.AttentionQKV.apply(qkv, kv_len, h, scale, p, seed, cu, max_len, None, groups, *bias)
    saved = out.grad_fn.saved_tensors
    assert len(saved) == (5 if short else 7)
    assert [ptr(t) for t in saved[:5]] == [ptr(qkv), ptr(saved[1]), ptr(kv_len), ptr(cu), ptr(groups if short else None)]
    lse = saved[1]
    assert tuple(lse.shape) == ((h, l) if packed else (b, h, l)) and tuple(out.shape) == tuple(qkv.shape[:-1]) + (hd,)
    out_lo = None if short else saved[6]
    assert short or ptr(saved[5]) == ptr(out)
    assert (out_lo is not None) == (dtype == torch.bfloat16 and not short)
    grouped = groups is not None and short                      # only the short-sequence kernels take groups
    want = common(qkv, None, None, kv_len, b, h, l, l, d, (hd3,) * 3, scale, p, seed, dtype, out=ptr(out), out_lo=ptr(out_lo),
                  lse=ptr(lse), cu_seqlens=ptr(cu), max_len=max_len, seq_groups=ptr(groups) if grouped else None,
                  num_groups=2 if grouped else 0)
    want.update(k=ptr(qkv, hd), v=ptr(qkv, 2 * hd))             # q | k | v are column blocks of the one buffer
    fwd, = rec.take()
    assert_call(fwd, FAMILY[d][0], want)

    gout = torch.ones_like(out)
    grads = torch.autograd.grad(out, (qkv,) + bias, gout)
    dqkv = grads[0]
    assert tuple(dqkv.shape) == tuple(qkv.shape) and all(tuple(g.shape) == (hd,) for g in grads[1:])
    fused_db = masters and short
    want.update(out=ptr(gout) if short else ptr(out), dout=ptr(gout), dq=ptr(dqkv), dk=ptr(dqkv, hd), dv=ptr(dqkv, 2 * hd),
                dq_stride=hd3, dk_stride=hd3, dv_stride=hd3, dbias_partial=SOME if fused_db else None,
                dbias=SOME if fused_db else None)
    calls = rec.take()
    assert_ws_call(calls[0], d, b=1 if packed else b, h=h, lq=l, lk=l, d=d)
    assert_call(calls[1], FAMILY[d][1], want)
    # the bias gradient: in-kernel on the short-sequence path, else one column-sum pass over dqkv
    tail = [n for n, _ in calls[2:]]
    assert tail == (["gmlm_colstats_workspace_bytes", "gmlm_colstats"] if masters and not short else [])
    if tail:
        assert calls[3][1][0] == ptr(dqkv) and calls[3][1][3:5] == (dqkv.numel() // hd3, hd3)


@pytest.mark.parametrize("masters", [False, True], ids=["nobias", "bias_masters"])
@pytest.mark.parametrize("mode", ["padded", "packed", "groups"])
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp32"])
@pytest.mark.parametrize("d", [32, 64])
def test_attention_qkv(rec, d, dtype, mode, masters):
    _qkv_case(rec, d, dtype, mode, masters, b=2, h=2, seq=3)


@pytest.mark.parametrize("masters", [False, True], ids=["nobias", "bias_masters"])
@pytest.mark.parametrize("mode", ["padded", "packed", "groups"])
@pytest.mark.parametrize("d", [32, 64])
def test_attention_qkv_with_512_pairs(rec, d, mode, masters):
    """b * h = 512 sequences of one row: d = 64 takes the short-sequence route (groups and bias sums reach the kernel), d = 32 not."""
    _qkv_case(rec, d, torch.bfloat16, mode, masters, b=512, h=1, seq=1)


@pytest.mark.parametrize("b,h,short", [(73, 7, False), (64, 8, True)], ids=["511_pairs", "512_pairs"])
def test_short_path_edge_at_128_rows(rec, b, h, short):
    """bf16, d = 64, 128 rows: out_lo and the saved output exist below 512 (sequence, head) pairs and not from 512 on."""
    l, hd = 128, h * 64
    qkv = torch.zeros(b, l, 3 * hd, dtype=torch.bfloat16, requires_grad=True)
    out = ops.AttentionQKV.apply(qkv, None, h, 0.125, 0.0, 0, None, 0)
    assert len(out.grad_fn.saved_tensors) == (5 if short else 7)
    (name, args), = rec.take()
    named = dict(zip([n for _, n in PROTOS[name][1]], args))
    assert name == "gmlm_attention_fwd" and (named["out_lo"] is None) == short
    assert short or named["out_lo"] == ptr(out.grad_fn.saved_tensors[6])
    q = torch.zeros(b, l, hd, dtype=torch.bfloat16, requires_grad=True)
    out = ops.Attention.apply(q, q, q, None, h, 0.125, 0.0, 0)
    (name, args), = rec.take()
    named = dict(zip([n for _, n in PROTOS[name][1]], args))
    assert name == "gmlm_attention_fwd" and (named["out_lo"] is None) == short
    assert (out.grad_fn.saved_tensors[6] is None) == short
    # one row more is no short sequence at any pair count
    q = torch.zeros(b, l + 1, hd, dtype=torch.bfloat16, requires_grad=True)
    out = ops.Attention.apply(q, q, q, None, h, 0.125, 0.0, 0)
    assert out.grad_fn.saved_tensors[6] is not None
    rec.take()


def test_attention_qkv_refuses_nothing_itself_at_other_head_dims(rec):
    """Any head dim but 32 goes to gmlm_attention_fwd, whose own check refuses what it does not serve."""
    qkv = torch.zeros(1, 2, 3 * 128)
    ops.AttentionQKV.apply(qkv, None, 1, 1.0, 0.0, 0, None, 0)
    assert [n for n, _ in rec.take()] == ["gmlm_attention_fwd"]


# ------------------------------------------------------------------------------------------------------- AttentionBlock
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp32"])
@pytest.mark.parametrize("d", [64, 96])
def test_attention_block(rec, d, dtype):
    b, h, lq, lk, hd = 2, 2, 2, 3, 2 * d
    kvbuf = torch.zeros(b, lk, 2 * hd, dtype=dtype)
    q, k, v = torch.zeros(b, lq, hd, dtype=dtype), kvbuf[..., :hd], kvbuf[..., hd:]
    kv_len = torch.tensor([2, 3], dtype=torch.int32)
    blk = ops.AttentionBlock(h, 0.25, 0.5)
    out, lse = blk.fwd(q, k, v, kv_len, 99)
    assert tuple(out.shape) == (b, lq, hd) and tuple(lse.shape) == (b, h, lq)
    want = common(q, k, v, kv_len, b, h, lq, lk, d, (hd, 2 * hd, 2 * hd), 0.25, 0.5, 99, dtype, out=ptr(out), out_lo=None, lse=ptr(lse))
    fwd, = rec.take()
    assert_call(fwd, "gmlm_attention_fwd", want)
    dout = torch.ones_like(out)
    for out_lo in (None, torch.zeros_like(out)):
        dq, dk, dv = blk.bwd(q, k, v, out, dout, lse, kv_len, 99, out_lo)
        want.update(dout=ptr(dout), dq=ptr(dq), dk=ptr(dk), dv=ptr(dv), dq_stride=hd, dk_stride=hd, dv_stride=hd, out_lo=ptr(out_lo))
        ws, bwd = rec.take()
        assert_ws_call(ws, d, b=b, h=h, lq=lq, lk=lk, d=d)
        assert_call(bwd, "gmlm_attention_bwd", want)


def test_attention_block_forwards_out_lo_at_the_short_geometry(rec):
    """bf16, d = 64, 64 rows, b * h = 512: the shape of the short-sequence kernels.  AttentionBlock decides nothing itself: the
    caller's out_lo reaches gmlm_attention_bwd untouched (its presence is what keeps a ring block, whose lse and out are those of
    all keys, off the short-sequence backward), and no out_lo stays NULL (the plain backward of the block's own forward)."""
    b, h, l, hd = 64, 8, 64, 8 * 64
    kvbuf = torch.zeros(b, l, 2 * hd, dtype=torch.bfloat16)
    q, k, v = torch.zeros(b, l, hd, dtype=torch.bfloat16), kvbuf[..., :hd], kvbuf[..., hd:]
    assert ops._short_path(q.dtype, 64, l, b * h)
    kv_len = torch.full((b,), 33, dtype=torch.int32)
    blk = ops.AttentionBlock(h, 0.125, 0.1)
    out, lse = blk.fwd(q, k, v, kv_len, 7)
    want = common(q, k, v, kv_len, b, h, l, l, 64, (hd, 2 * hd, 2 * hd), 0.125, 0.1, 7, torch.bfloat16, out=ptr(out), out_lo=None,
                  lse=ptr(lse))
    fwd, = rec.take()
    assert_call(fwd, "gmlm_attention_fwd", want)
    dout, out_lo = torch.ones_like(out), torch.zeros_like(out)
    for lo in (out_lo, None):
        dq, dk, dv = blk.bwd(q, k, v, out, dout, lse, kv_len, 7, out_lo=lo) if lo is not None else blk.bwd(q, k, v, out, dout, lse, kv_len, 7)
        want.update(dout=ptr(dout), dq=ptr(dq), dk=ptr(dk), dv=ptr(dv), dq_stride=hd, dk_stride=hd, dv_stride=hd, out_lo=ptr(lo))
        ws, bwd = rec.take()
        assert_ws_call(ws, 64, b=b, h=h, lq=l, lk=l, d=64)
        assert_call(bwd, "gmlm_attention_bwd", want)


def test_attention_block_refusals(rec):
    blk = ops.AttentionBlock(2, 1.0)
    for d in (32, 128):
        q = torch.zeros(1, 2, 2 * d)
        with pytest.raises(NotImplementedError, match=rf"native head dim \(64 or 96\), got {d}: the head-dim-128 kernels"):
            blk.fwd(q, q, q, None, 0)
    q = torch.zeros(1, 2, 2 * 256)
    with pytest.raises(NotImplementedError, match="no block form at head dim 256: the wide-head kernels"):
        blk.fwd(q, q, q, None, 0)
    assert not rec.take()


# ----------------------------------------------------------------------------------------------------- BiasResLayerNorm
@pytest.mark.parametrize("f,wide", [(1024, False), (1028, True)])
def test_bias_res_layernorm(rec, f, wide):
    rows = 3
    x = torch.zeros(rows, f, requires_grad=True)
    res = torch.zeros(rows, f, requires_grad=True)
    bias, gamma, beta = (torch.zeros(f, requires_grad=True) for _ in range(3))
    y = ops.BiasResLayerNorm.apply(x, bias, res, gamma, beta, 1e-5, True, 0.25, 5)
    sx, sres, sb, sg, sbeta, mean, rstd = y.grad_fn.saved_tensors
    want = dict(x=ptr(x), bias=ptr(bias), residual=ptr(res), gamma=ptr(gamma), beta=ptr(beta), rows=rows, f=f, eps=1e-5, act=1,
                dropout_p=0.25, seed=5, seed_dev=None, y=ptr(y), mean=ptr(mean), rstd=ptr(rstd), dtype=_lib.F32, stream=STREAM)
    fwd, = rec.take()
    assert_call(fwd, "gmlm_bias_res_layernorm_wide_fwd" if wide else "gmlm_bias_res_layernorm_fwd", want)
    gy = torch.ones_like(y)
    dx, dbias, dres, dg, dbeta = torch.autograd.grad(y, (x, bias, res, gamma, beta), gy)
    want.update(dy=ptr(gy), dx=ptr(dx), dresidual=ptr(dres), dgamma=ptr(dg), dbeta=ptr(dbeta), dbias=ptr(dbias), workspace=SOME,
                workspace_bytes=WS_BYTES)
    ws, bwd = rec.take()
    assert ws == ("gmlm_bias_res_layernorm_wide_bwd_workspace_bytes" if wide else "gmlm_layernorm_bwd_workspace_bytes", (rows, f))
    assert_call(bwd, "gmlm_bias_res_layernorm_wide_bwd" if wide else "gmlm_bias_res_layernorm_bwd", want)


def test_bias_res_layernorm_optional_operands_are_null(rec):
    x = torch.zeros(2, 64, dtype=torch.bfloat16, requires_grad=True)
    gamma, beta = torch.zeros(64), torch.zeros(64)
    y = ops.BiasResLayerNorm.apply(x, None, None, gamma, beta, 1e-5, False, 0.0, 0)
    (name, args), = rec.take()
    named = dict(zip([n for _, n in PROTOS[name][1]], args))
    assert name == "gmlm_bias_res_layernorm_fwd" and named["bias"] is None and named["residual"] is None and named["act"] == 0
    assert named["dtype"] == _lib.BF16
    torch.autograd.grad(y, x, torch.ones_like(y))
    _, (name, args) = rec.take()
    named = dict(zip([n for _, n in PROTOS[name][1]], args))
    assert named["dresidual"] is None and named["dbias"] is None and named["residual"] is None and named["dgamma"] is not None


# ------------------------------------------------------------------------------------------- nn: pad, call, cut back
@pytest.mark.parametrize("d,dp", [(32, 64), (48, 64), (64, 64), (100, 128), (200, 256), (256, 256), (400, 512)])
def test_any_dim_and_wide_dim_round_the_head_dim_up(rec, d, dp):
    attend = gnn.attention_any_dim if d <= 128 else gnn.attention_wide_dim
    h, lq, lk = 2, 2, 3
    q, k, v = torch.zeros(1, lq, h * d), torch.zeros(1, lk, h * d), torch.zeros(1, lk, h * d)
    out = attend(q, k, v, None, h, d ** -0.5, 0.5, False)
    assert tuple(out.shape) == (1, lq, h * d)
    (name, args), = rec.take()
    named = dict(zip([n for _, n in PROTOS[name][1]], args))
    assert name == FAMILY[dp][0]
    assert (named["d"], named["h"], named["lq"], named["lk"]) == (dp, h, lq, lk)
    assert (named["q_stride"], named["k_stride"], named["v_stride"]) == (h * dp,) * 3
    assert named["scale"] == d ** -0.5 and named["dropout_p"] == 0.0 and named["seed"] == 0     # not training: no dropout
    if d == dp:
        assert (named["q"], named["k"], named["v"]) == (ptr(q), ptr(k), ptr(v))


def test_any_dim_and_wide_dim_errors(rec):
    q = torch.zeros(1, 2, 2 * 160)
    with pytest.raises(NotImplementedError, match="attention head dim 160 > 128 is not supported by the gfx950 kernels"):
        gnn.attention_any_dim(q, q, q, None, 2, 1.0, 0.0, False)
    q = torch.zeros(1, 2, 2 * 520)
    with pytest.raises(NotImplementedError, match="attention head dim 520 > 512 is not supported by the gfx950 kernels"):
        gnn.attention_wide_dim(q, q, q, None, 2, 1.0, 0.0, False)
    q = torch.zeros(1, 2, 2 * 100)
    with pytest.raises(ValueError, match=r"attention_wide_dim takes head dims 129 \.\.\. 512, got 100: use attention_any_dim"):
        gnn.attention_wide_dim(q, q, q, None, 2, 1.0, 0.0, False)
    assert not rec.take()
