"""The packed (variable-length) causal grouped-KV attention at d = 128 and the rotary embedding by position against float64
torch on the same rounded inputs, bf16 and fp32, forward and backward.

Sequences: the LENS of test_gpu_decoder_ops.py (both sides of every wave, key-tile and workgroup edge, and one sequence of
length 0) packed back to back with the 257-row one last: T = 835 rows.  The kernels are the ones of the padded entry
points, so the budgets are test_gpu_decoder_ops.py's.  Every attention case also runs the C entry points once more on
buffers of its own, with 128 sentinel rows behind row T of everything written and NaN rows behind row T of everything read:
the results must be the bits the operator gave, the sentinels untouched."""
import pytest
import torch

from helpers import _close, kernels_run
from test_gpu_decoder_ops import (LENS as PADDED_LENS, TN, U, _budget, _elem_check, _rel_l2, _rope_table, _rot, _rot_mag, _same_bits,
                                  _stat)

pytestmark = pytest.mark.gpu

DT = [torch.bfloat16, torch.float32]
SEQS = [1, 31, 33, 64, 0, 65, 127, 128, 129, 257]         # the empty sequence in the middle, the longest one last
T = sum(SEQS)
MAX_LEN = max(SEQS)
GUARD = 128


def test_sequence_set_is_the_padded_tests():
    assert sorted(SEQS) == sorted(PADDED_LENS) and T == 835 and SEQS[-1] == 257 and 0 in SEQS


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _cu(dev):
    return torch.tensor([0] + SEQS, dtype=torch.int64).cumsum(0).to(dev, torch.int32)


def _positions(dev):
    return torch.cat([torch.arange(n) for n in SEQS]).to(dev)


def _reference(q, k, v, go, hq, hkv, scale):
    """Dense float64 causal attention, one sequence at a time, autograd backward.  q, go [T, hq*128]; k, v [T, hkv*128]."""
    rep = hq // hkv
    qd, kd, vd = (t.detach().double().requires_grad_(True) for t in (q, k, v))
    outs, r0 = [], 0
    for n in SEQS:
        if n == 0:
            continue
        qh = qd[r0:r0 + n].view(n, hq, 128).transpose(0, 1)
        kh = kd[r0:r0 + n].view(n, hkv, 128).transpose(0, 1).repeat_interleave(rep, 0)
        vh = vd[r0:r0 + n].view(n, hkv, 128).transpose(0, 1).repeat_interleave(rep, 0)
        s = (qh @ kh.transpose(-1, -2)) * scale
        s = s.masked_fill(~torch.ones(n, n, dtype=torch.bool, device=q.device).tril(), float("-inf"))
        outs.append((torch.softmax(s, -1) @ vh).transpose(0, 1).reshape(n, hq * 128))
        r0 += n
    o = torch.cat(outs)
    o.backward(go.double())
    return o.detach(), qd.grad, kd.grad, vd.grad


def _guarded(src, fill):
    """``src`` [T, w] as the leading rows of a [T + GUARD, w] buffer whose other rows hold ``fill``."""
    buf = torch.full((T + GUARD, src.shape[1]), fill, dtype=src.dtype, device=src.device)
    buf[:T] = src
    return buf


def _raw_run(ops, qkv, go, cu, hq, hkv, scale, fused):
    """The C entry points on buffers of this test: reads end exactly at row T of NaN-backed buffers, writes have sentinel rows."""
    dtype, dev = qkv.dtype, qkv.device
    nq, nk = hq * 128, hkv * 128
    lib, ptr = ops.lib(), ops._ptr
    if fused:
        x = _guarded(qkv, float("nan"))
        q, k, v = x[:T, :nq], x[:T, nq:nq + nk], x[:T, nq + nk:]
    else:
        q, k, v = (_guarded(t.contiguous(), float("nan"))[:T] for t in (qkv[:, :nq], qkv[:, nq:nq + nk], qkv[:, nq + nk:]))
    gb = _guarded(go, float("nan"))
    sent = 7.0
    out = torch.full((T + GUARD, nq), sent, dtype=dtype, device=dev)
    out_lo = torch.full((T + GUARD, nq), sent, dtype=dtype, device=dev) if dtype == torch.bfloat16 else None
    lse = torch.full((hq * T + GUARD * hq,), sent, dtype=torch.float32, device=dev)
    dqkv = torch.full((T + GUARD, nq + 2 * nk), sent, dtype=dtype, device=dev)
    s = cu.numel() - 1
    ops.check(lib.gmlm_attention_causal_d128_varlen_fwd(ptr(q), ptr(k), ptr(v), ptr(cu), s, MAX_LEN, T, hq, hkv, 128, q.stride(0),
                                                        k.stride(0), v.stride(0), scale, 0.0, ptr(out), ptr(out_lo), ptr(lse),
                                                        ops._dt(q), ops._stream()), "varlen_fwd")
    ws = ops._ws(lib.gmlm_attention_causal_d128_varlen_workspace_bytes(T, hq), dev)
    dq, dk, dv = dqkv[:T, :nq], dqkv[:T, nq:nq + nk], dqkv[:T, nq + nk:]
    ops.check(lib.gmlm_attention_causal_d128_varlen_bwd(ptr(q), ptr(k), ptr(v), ptr(out), ptr(out_lo), ptr(gb), ptr(lse), ptr(cu), s,
                                                        MAX_LEN, T, hq, hkv, 128, q.stride(0), k.stride(0), v.stride(0), scale, 0.0,
                                                        ptr(dq), ptr(dk), ptr(dv), dqkv.stride(0), dqkv.stride(0), dqkv.stride(0),
                                                        ops._dt(q), ptr(ws), ws.numel(), ops._stream()), "varlen_bwd")
    torch.cuda.synchronize()
    for name, buf in (("out", out), ("out_lo", out_lo), ("dqkv", dqkv)):
        if buf is not None:
            assert bool((buf[T:] == sent).all()), f"{name}: rows behind row T were written"
    assert bool((lse[hq * T:] == sent).all()), "lse: written behind [hq, T]"
    assert bool(torch.isfinite(lse[:hq * T]).all())
    return out[:T], dq.contiguous(), dk.contiguous(), dv.contiguous()


def _varlen_case(dev, dtype, hq, hkv, fused, seed):
    from gmlm_amd import ops
    g = torch.Generator().manual_seed(seed)
    scale = 128 ** -0.5
    nq, nk = hq * 128, hkv * 128
    cu = _cu(dev)
    qkv = torch.randn(T, nq + 2 * nk, generator=g).to(dev, dtype)
    go = torch.randn(T, nq, generator=g).to(dev, dtype)

    def run():
        if fused:
            x = qkv.clone().requires_grad_(True)
            q, k, v = x[:, :nq], x[:, nq:nq + nk], x[:, nq + nk:]
            leaves = None
        else:
            q, k, v = (t.clone().contiguous().requires_grad_(True) for t in (qkv[:, :nq], qkv[:, nq:nq + nk], qkv[:, nq + nk:]))
            leaves = (q, k, v)
        out = ops.causal_attention_varlen(q, k, v, cu, MAX_LEN, hq, hkv, scale)
        out.backward(go)
        grads = (x.grad[:, :nq], x.grad[:, nq:nq + nk], x.grad[:, nq + nk:]) if fused else tuple(t.grad for t in leaves)
        return (out.detach(),) + tuple(t.contiguous() for t in grads)

    box = {}
    ran = kernels_run(lambda: box.setdefault("r", run()))
    tn = TN[dtype]
    assert {n for n in ran if n.startswith("causal128::")} == {f"causal128::{k}<{tn}>" for k in
                                                               ("fwd_kernel", "delta_kernel", "dq_kernel", "dkv_kernel")}, ran
    assert not any(n.startswith(("attn_", "d128::")) for n in ran), ran
    assert _same_bits(run(), box["r"])
    ref = _reference(qkv[:, :nq], qkv[:, nq:nq + nk], qkv[:, nq + nk:], go, hq, hkv, scale)
    for name, got, r_ in zip(("out", "dq", "dk", "dv"), box["r"], ref):
        assert got.shape == r_.shape and bool(torch.isfinite(got).all()), name
        _close(name, got, r_, *_budget(dtype, name))
    raw = _raw_run(ops, qkv, go, cu, hq, hkv, scale, fused)
    for name, got, r_ in zip(("out", "dq", "dk", "dv"), raw, box["r"]):
        assert bool(torch.isfinite(got).all()), name               # nothing read from the NaN rows behind row T
        assert _same_bits([got.contiguous()], [r_]), name


@pytest.mark.parametrize("dtype", DT, ids=["bf16", "fp32"])
@pytest.mark.parametrize("fused", [False, True], ids=["contiguous", "fused_qkv"])
@pytest.mark.parametrize("hkv", [4, 2, 1])
def test_varlen_causal_attention_vs_dense_float64(dev, hkv, fused, dtype):
    _varlen_case(dev, dtype, 4, hkv, fused, 31 + hkv)


@pytest.mark.parametrize("dtype", DT, ids=["bf16", "fp32"])
def test_varlen_equals_the_padded_kernels_on_one_full_sequence(dev, dtype):
    """One sequence of 257 rows is the padded layout with b = 1: the same kernels on the same tiles give the same bits."""
    from gmlm_amd import ops
    hq, hkv, n, scale = 4, 2, 257, 128 ** -0.5
    nq, nk = hq * 128, hkv * 128
    g = torch.Generator().manual_seed(3)
    qkv = torch.randn(n, nq + 2 * nk, generator=g).to(dev, dtype)
    go = torch.randn(n, nq, generator=g).to(dev, dtype)
    cu = torch.tensor([0, n], dtype=torch.int32, device=dev)
    a = qkv.clone().requires_grad_(True)
    ops.causal_attention_varlen(a[:, :nq], a[:, nq:nq + nk], a[:, nq + nk:], cu, n, hq, hkv, scale).backward(go)
    b = qkv.clone()[None].requires_grad_(True)
    ops.causal_attention(b[..., :nq], b[..., nq:nq + nk], b[..., nq + nk:], None, hq, hkv, scale).backward(go[None])
    assert float(a.grad.abs().max()) > 0 and _same_bits([a.grad], [b.grad[0]])


# ---------------------------------------------------------------------------------------------
# rotary embedding by position
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DT, ids=["bf16", "fp32"])
def test_qknorm_rope_by_position_vs_float64(dev, dtype):
    """The packed rows' positions (0..len-1 per sequence, so 0, 1, 63 and 256 all occur) plus two positions outside the
    table, which must read its first / last row; budgets and formulas of test_qknorm_rope."""
    from gmlm_amd import ops
    hq, hkv, eps, table = 4, 2, 1e-6, 300
    g = torch.Generator().manual_seed(41)
    wid, nqk = (hq + 2 * hkv) * 128, (hq + hkv) * 128
    buf = torch.randn(T, wid + 64, generator=g).to(dev, dtype)
    qw, kw = (torch.empty(128).uniform_(0.5, 1.5, generator=g).to(dev) for _ in range(2))
    cs = _rope_table(table, 1e6, dev)
    go = torch.randn(T, nqk, generator=g).to(dev, dtype)
    pos = _positions(dev)
    pos[5], pos[700] = -3, table + 9
    read = pos.clamp(0, table - 1)

    def run():
        bv, qv, kv = buf.clone().requires_grad_(True), qw.clone().requires_grad_(True), kw.clone().requires_grad_(True)
        out = ops.qknorm_rope(bv[:, :wid], qv, kv, cs, hq, hkv, eps, pos_ids=pos)
        out.backward(go)
        assert float(bv.grad[:, wid:].abs().max()) == 0.0
        return out.detach(), bv.grad[:, :wid].contiguous(), qv.grad, kv.grad

    box = {}
    ran = kernels_run(lambda: box.setdefault("r", run()))
    out, dx, dqw, dkw = box["r"]
    tn = TN[dtype]
    assert f"qknorm_rope_fwd_kernel<{tn}>" in ran and f"qknorm_rope_bwd_kernel<{tn}>" in ran, ran
    assert _same_bits(run(), box["r"])

    x = buf[:, :wid].double().view(T, hq + 2 * hkv, 128)[:, :hq + hkv]
    wd = torch.cat([qw.double().expand(hq, 128), kw.double().expand(hkv, 128)])[None]
    cos, sin = cs[read, 0].double()[:, None, :], cs[read, 1].double()[:, None, :]
    st = _stat(128, 16 if dtype == torch.bfloat16 else 32)
    rstd = (x.pow(2).mean(-1, keepdim=True) + eps).rsqrt()
    xh = x * rstd
    n = xh * wd
    ref, mag = _rot(n, cos, sin), _rot_mag(n, cos, sin)
    got = out.view(T, hq + hkv, 128)
    for p_ in (0, 1, 63, 256):
        rows = read == p_
        assert int(rows.sum()) > 0
        _elem_check(f"out @ position {p_}", got[rows], ref[rows], mag[rows] * (0.5 * st + 5 * U))
    _elem_check("out", got, ref, mag * (0.5 * st + 5 * U))
    gd = go.double().view(T, hq + hkv, 128)
    dn, dn_mag = _rot(gd, cos, -sin), _rot_mag(gd, cos, sin)
    gr = dn * wd
    m = (gr * xh).mean(-1, keepdim=True)
    m_abs = (dn_mag * wd * xh.abs()).mean(-1, keepdim=True)
    dxr = rstd * (gr - xh * m)
    extra = rstd * ((4 * U + 0.5 * st) * (dn_mag * wd + (xh * m).abs()) + xh.abs() * (st + 4 * U) * m_abs)
    dxg = dx.view(T, hq + 2 * hkv, 128)
    _elem_check("dx (q | k)", dxg[:, :hq + hkv], dxr, extra)
    assert float(dxg[:, hq + hkv:].abs().max()) == 0.0
    _rel_l2("dq_weight", dqw, (dn * xh)[:, :hq].sum((0, 1)), dtype)
    _rel_l2("dk_weight", dkw, (dn * xh)[:, hq:].sum((0, 1)), dtype)


@pytest.mark.parametrize("dtype", DT, ids=["bf16", "fp32"])
def test_qknorm_rope_by_position_equals_the_padded_form(dev, dtype):
    """[3, 40, .] rows with pos_ids = arange % 40: the same arithmetic, so output, input gradient and both weight gradients
    are bit for bit those of the padded entry points."""
    from gmlm_amd import ops
    hq, hkv, eps, b, l = 4, 2, 1e-6, 3, 40
    g = torch.Generator().manual_seed(43)
    wid, nqk = (hq + 2 * hkv) * 128, (hq + hkv) * 128
    qkv = torch.randn(b, l, wid, generator=g).to(dev, dtype)
    qw, kw = (torch.empty(128).uniform_(0.5, 1.5, generator=g).to(dev) for _ in range(2))
    cs = _rope_table(64, 1e6, dev)
    go = torch.randn(b, l, nqk, generator=g).to(dev, dtype)
    pos = (torch.arange(b * l, device=dev) % l).to(torch.int32)

    def run(by_pos):
        x, qv, kv = qkv.clone().requires_grad_(True), qw.clone().requires_grad_(True), kw.clone().requires_grad_(True)
        if by_pos:
            out = ops.qknorm_rope(x.view(b * l, wid), qv, kv, cs, hq, hkv, eps, pos_ids=pos).view(b, l, nqk)
        else:
            out = ops.qknorm_rope(x, qv, kv, cs, hq, hkv, eps)
        out.backward(go)
        return out.detach(), x.grad, qv.grad, kv.grad

    for name, a, r_ in zip(("out", "dqkv", "dq_weight", "dk_weight"), run(True), run(False)):
        assert float(a.abs().max()) > 0, name
        assert _same_bits([a], [r_]), name


@pytest.mark.parametrize("dtype", DT, ids=["bf16", "fp32"])
def test_fused_varlen_node_equals_the_two_ops(dev, dtype):
    """ops.rope_causal_attention_varlen (the node the packed encoder uses) against ops.qknorm_rope by position followed by
    ops.causal_attention_varlen, which the cases above check against float64: equal element for element (torch.equal, as
    in test_fused_rope_attention_node_equals_the_two_ops)."""
    from gmlm_amd import ops
    hq, hkv, scale, eps = 4, 2, 128 ** -0.5, 1e-6
    g = torch.Generator().manual_seed(47)
    nq, nk = hq * 128, hkv * 128
    cu, pos = _cu(dev), _positions(dev)
    qkv = torch.randn(T, nq + 2 * nk, generator=g).to(dev, dtype)
    qw, kw = (torch.empty(128).uniform_(0.5, 1.5, generator=g).to(dev) for _ in range(2))
    cs = _rope_table(MAX_LEN + 7, 1e6, dev)
    go = torch.randn(T, nq, generator=g).to(dev, dtype)

    def run(fused):
        x, qv, kv = qkv.clone().requires_grad_(True), qw.clone().requires_grad_(True), kw.clone().requires_grad_(True)
        if fused:
            out = ops.rope_causal_attention_varlen(x, qv, kv, cs, pos, cu, MAX_LEN, hq, hkv, scale, eps)
        else:
            qk = ops.qknorm_rope(x, qv, kv, cs, hq, hkv, eps, pos_ids=pos)
            out = ops.causal_attention_varlen(qk[:, :nq], qk[:, nq:], x[:, nq + nk:], cu, MAX_LEN, hq, hkv, scale)
        out.backward(go)
        return out.detach(), x.grad, qv.grad, kv.grad

    box = {}
    ran = kernels_run(lambda: box.setdefault("r", run(True)))
    tn = TN[dtype]
    for k in ("qknorm_rope_fwd_kernel", "qknorm_rope_bwd_kernel", "causal128::fwd_kernel", "causal128::dq_kernel", "causal128::dkv_kernel"):
        assert f"{k}<{tn}>" in ran, (k, ran)
    for name, a, r_ in zip(("out", "dqkv", "dq_weight", "dk_weight"), box["r"], run(False)):
        assert bool(torch.isfinite(a).all()) and float(a.abs().max()) > 0, name
        assert torch.equal(a, r_), name
