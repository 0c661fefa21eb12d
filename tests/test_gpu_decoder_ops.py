"""The decoder row kernels (add + RMSNorm, Q/K head norm + RoPE, SwiGLU) and the causal grouped-KV attention at d = 128
against float64 torch on the same rounded inputs, bf16 and fp32, forward and backward; every case asserts by name which
kernels ran and that a second identical call gives identical bits.

Budgets of the row kernels (the rule of test_gpu_norm_matrix.py).  Per element, |got - ref| <= one ulp of the storage type
at ref (bf16: one bf16 ulp; fp32: 4 fp32 ulps, "a few") plus an absolute term for the fp32 arithmetic behind it, written out
where it is used:
 * statistics: a row sum of n terms, taken as n / lanes serial fp32 additions per lane and log2(lanes) butterfly steps, has
   relative error <= (n / lanes + log2(lanes) + 2) 2^-24 of the sum of the terms' magnitudes (worst case of sequential
   summation); rstd = (mean + eps)^-1/2 carries half of it;
 * every product / sum that forms the result contributes 2^-24 of its operands' magnitudes, which matters only where two
   terms nearly cancel (rotation, the norm backward, 1 + g (1 - sigmoid g)) and the result's own ulp is smaller than that.
A value that is a function of a tensor the kernel itself stored (y of the stored sum s, the backward of the stored s) is
checked against float64 of the STORED tensor, since that is what every later kernel reads.
Weight gradients: rel-L2 1e-5 (fp32) / 8e-3 (bf16) and the attention budgets are the tree's (test_gpu_attention_d128.py)."""
import pytest
import torch

from helpers import _close, kernels_run

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
DT = [torch.bfloat16, torch.float32]
TN = {torch.bfloat16: "unsigned short", torch.float32: "float"}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _ulp(ref, dtype):
    bits = 7 if dtype == torch.bfloat16 else 23
    return torch.exp2(torch.floor(torch.log2(ref.abs().clamp_min(2.0 ** -126))) - bits)


def _elem_check(name, got, ref, extra):
    assert got.dtype in (torch.bfloat16, torch.float32)
    assert bool(torch.isfinite(got).all()), name
    bound = _ulp(ref, got.dtype) * (1 if got.dtype == torch.bfloat16 else 4) + extra
    ratio = (got.double() - ref).abs() / bound
    worst, nbad = float(ratio.max()), int((ratio > 1).sum())
    print(f"  {name}: max err / bound = {worst:.2f}, {nbad} of {ratio.numel()} outside")
    assert nbad == 0, (name, worst, nbad)


def _rel_l2(name, got, ref, dtype):
    e = float((got.double() - ref).norm()) / float(ref.norm())
    print(f"  {name}: rel l2 = {e:.2e}")
    assert e <= (1e-5 if dtype == torch.float32 else 8e-3), (name, e)


def _stat(n, lanes):
    import math
    return (n / lanes + math.log2(lanes) + 2) * U


def _same_bits(a, b):
    return all(torch.equal(x.view(torch.int16 if x.dtype == torch.bfloat16 else torch.int32),
                           y.view(torch.int16 if y.dtype == torch.bfloat16 else torch.int32)) for x, y in zip(a, b))


# ---------------------------------------------------------------------------------------------
# add + RMSNorm
# ---------------------------------------------------------------------------------------------
def _ch(f, dtype):
    need = -(-(f // (8 if dtype == torch.bfloat16 else 4)) // 64)
    return next(c for c in (2, 4, 8, 16) if need <= c)


@pytest.mark.parametrize("dtype", DT, ids=["bf16", "fp32"])
@pytest.mark.parametrize("with_b", [True, False], ids=["add", "plain"])
@pytest.mark.parametrize("f", [256, 1024, 2048, 2560, 4096])     # 2048: the <bf16, 4> and <fp32, 8> instantiations
@pytest.mark.parametrize("rows", [1, 7, 4096])
def test_add_rmsnorm(dev, rows, f, with_b, dtype):
    from gmlm_amd import ops
    g = torch.Generator().manual_seed(rows * 7 + f)
    eps = 1e-6
    a = torch.randn(rows, f, generator=g).to(dev, dtype)
    b = (0.5 * torch.randn(rows, f, generator=g)).to(dev, dtype) if with_b else None
    w = torch.empty(f).uniform_(0.5, 1.5, generator=g).to(dev)
    gy, gs = (torch.randn(rows, f, generator=g).to(dev, dtype) for _ in range(2))

    def run():
        av, wv = a.clone().requires_grad_(True), w.clone().requires_grad_(True)
        bv = b.clone().requires_grad_(True) if with_b else None
        s, y = ops.add_rmsnorm(av, bv, wv, eps)
        torch.autograd.backward([s, y], [gs, gy])
        return s.detach(), y.detach(), av.grad, (bv.grad if with_b else av.grad), wv.grad

    box = {}
    ran = kernels_run(lambda: box.setdefault("r", run()))
    s, y, da, db, dw = box["r"]
    tn, ch = TN[dtype], _ch(f, dtype)
    assert f"rmsnorm_fwd_kernel<{tn}, {ch}>" in ran and f"rmsnorm_bwd_kernel<{tn}, {ch}>" in ran, ran
    assert not any(n.startswith(("ln_", "graphnorm_")) for n in ran), ran
    assert _same_bits(run(), box["r"])

    ad = a.double()
    if with_b:
        _elem_check("s", s, ad + b.double(), 0.0)
    else:
        assert torch.equal(s, a)
    sd = s.double()                                               # the stored sum: what y and the backward are functions of
    st = _stat(f, 64)
    rstd = (sd.pow(2).mean(-1, keepdim=True) + eps).rsqrt()
    wd = w.double()
    yr = sd * rstd * wd
    _elem_check("y", y, yr, yr.abs() * (0.5 * st + 4 * U))
    gr = gy.double() * wd
    xh = sd * rstd
    m = (gr * xh).mean(-1, keepdim=True)
    m_abs = (gr * xh).abs().mean(-1, keepdim=True)
    dsr = gs.double() + rstd * (gr - xh * m)
    # dres + rstd (g - xhat m): the three terms can cancel; m is a row statistic (relative st of mean|g xhat|), rstd is one
    extra = 4 * U * (gs.double().abs() + rstd * (gr.abs() + (xh * m).abs())) + rstd * xh.abs() * st * m_abs \
        + 0.5 * st * rstd * (gr.abs() + (xh * m).abs())
    _elem_check("da", da, dsr, extra)
    assert torch.equal(da, db)
    _rel_l2("dw", dw, (gy.double() * xh).sum(0), dtype)


# ---------------------------------------------------------------------------------------------
# Q / K head norm + RoPE
# ---------------------------------------------------------------------------------------------
def _rope_table(max_len, theta, dev):
    inv = 1.0 / (theta ** (torch.arange(0, 128, 2, dtype=torch.float) / 128))
    fr = torch.arange(max_len, dtype=torch.float32)[:, None] * inv[None]
    return torch.stack([fr.cos(), fr.sin()], 1).contiguous().to(dev)


def _rot_mag(n, cos, sin):
    """the same with every product taken in magnitude: what can cancel in the rotation"""
    lo, hi = n[..., :64].abs(), n[..., 64:].abs()
    return torch.cat([lo * cos.abs() + hi * sin.abs(), hi * cos.abs() + lo * sin.abs()], -1)


def _rot(n, cos, sin):
    """rotate-half rotation of [..., 128] rows; cos / sin [..., 64]"""
    lo, hi = n[..., :64], n[..., 64:]
    return torch.cat([lo * cos - hi * sin, hi * cos + lo * sin], -1)


@pytest.mark.parametrize("dtype", DT, ids=["bf16", "fp32"])
@pytest.mark.parametrize("hq,hkv", [(4, 4), (4, 2), (16, 8)])
def test_qknorm_rope(dev, hq, hkv, dtype):
    """[2, 512] tokens, so positions 0, 1, 63 and 511 all occur (checked per position below); the input is a strided
    slice of a wider buffer, as a fused projection output with extra columns would be."""
    from gmlm_amd import ops
    g = torch.Generator().manual_seed(hq * 10 + hkv)
    b, l, eps = 2, 512, 1e-6
    wid, nqk = (hq + 2 * hkv) * 128, (hq + hkv) * 128
    buf = torch.randn(b, l, wid + 64, generator=g).to(dev, dtype)
    qkv = buf[..., :wid]
    assert qkv.stride(1) == wid + 64
    qw, kw = (torch.empty(128).uniform_(0.5, 1.5, generator=g).to(dev) for _ in range(2))
    cs = _rope_table(l, 1e6, dev)
    go = torch.randn(b, l, nqk, generator=g).to(dev, dtype)

    def run():
        bv, qv, kv = buf.clone().requires_grad_(True), qw.clone().requires_grad_(True), kw.clone().requires_grad_(True)
        out = ops.qknorm_rope(bv[..., :wid], qv, kv, cs, hq, hkv, eps)
        out.backward(go)
        assert float(bv.grad[..., wid:].abs().max()) == 0.0        # the columns outside the fused rows
        return out.detach(), bv.grad[..., :wid].contiguous(), qv.grad, kv.grad

    box = {}
    ran = kernels_run(lambda: box.setdefault("r", run()))
    out, dx, dqw, dkw = box["r"]
    tn = TN[dtype]
    assert f"qknorm_rope_fwd_kernel<{tn}>" in ran and f"qknorm_rope_bwd_kernel<{tn}>" in ran, ran
    assert _same_bits(run(), box["r"])

    x = qkv.double().view(b, l, hq + 2 * hkv, 128)[:, :, :hq + hkv]
    wd = torch.cat([qw.double().expand(hq, 128), kw.double().expand(hkv, 128)])[None, None]
    cos, sin = cs[:, 0].double()[None, :, None, :], cs[:, 1].double()[None, :, None, :]
    st = _stat(128, 16 if dtype == torch.bfloat16 else 32)
    rstd = (x.pow(2).mean(-1, keepdim=True) + eps).rsqrt()
    xh = x * rstd
    n = xh * wd
    ref = _rot(n, cos, sin)
    mag = _rot_mag(n, cos, sin)
    got = out.view(b, l, hq + hkv, 128)
    for pos in (0, 1, 63, 511):
        _elem_check(f"out @ position {pos}", got[:, pos], ref[:, pos], mag[:, pos] * (0.5 * st + 5 * U))
    _elem_check("out", got, ref, mag * (0.5 * st + 5 * U))
    # backward: dn = R^T go, g = dn w, dx = rstd (g - xhat mean(g xhat))
    gd = go.double().view(b, l, hq + hkv, 128)
    dn = _rot(gd, cos, -sin)
    dn_mag = _rot_mag(gd, cos, sin)
    gr = dn * wd
    m = (gr * xh).mean(-1, keepdim=True)
    m_abs = (dn_mag * wd * xh.abs()).mean(-1, keepdim=True)
    dxr = rstd * (gr - xh * m)
    extra = rstd * ((4 * U + 0.5 * st) * (dn_mag * wd + (xh * m).abs()) + xh.abs() * (st + 4 * U) * m_abs)
    dxg = dx.view(b, l, hq + 2 * hkv, 128)
    _elem_check("dx (q | k)", dxg[:, :, :hq + hkv], dxr, extra)
    assert float(dxg[:, :, hq + hkv:].abs().max()) == 0.0          # V columns: no gradient from this op
    _rel_l2("dq_weight", dqw, (dn * xh)[:, :, :hq].sum((0, 1, 2)), dtype)
    _rel_l2("dk_weight", dkw, (dn * xh)[:, :, hq:].sum((0, 1, 2)), dtype)


# ---------------------------------------------------------------------------------------------
# SwiGLU
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DT, ids=["bf16", "fp32"])
@pytest.mark.parametrize("inter", [384, 3072])
@pytest.mark.parametrize("rows", [1, 130])
def test_swiglu(dev, rows, inter, dtype):
    from gmlm_amd import ops
    g = torch.Generator().manual_seed(rows + inter)
    gu = (2.0 * torch.randn(rows, 2 * inter, generator=g)).to(dev, dtype)
    gy = torch.randn(rows, inter, generator=g).to(dev, dtype)

    def run():
        v = gu.clone().requires_grad_(True)
        y = ops.swiglu(v)
        y.backward(gy)
        return y.detach(), v.grad

    box = {}
    ran = kernels_run(lambda: box.setdefault("r", run()))
    y, dgu = box["r"]
    assert f"swiglu_fwd_kernel<{TN[dtype]}>" in ran and f"swiglu_bwd_kernel<{TN[dtype]}>" in ran, ran
    assert not any(n.startswith("bias_gelu_") for n in ran), ran
    assert _same_bits(run(), box["r"])
    gt, up, d = gu[:, :inter].double(), gu[:, inter:].double(), gy.double()
    sig = torch.sigmoid(gt)
    yr = gt * sig * up
    # exp, 1 + e, the quotient and two products: a few fp32 ulps of the result; exp(-g) itself is good to 2 ulps of ITS value,
    # which reaches sigmoid as |g|-independent relative error <= 2^-22
    _elem_check("y", y, yr, yr.abs() * 12 * U)
    dup = d * gt * sig
    t = gt * (1 - sig)
    dgate = d * up * sig * (1 + t)
    _elem_check("d up", dgu[:, inter:], dup, dup.abs() * 12 * U)
    _elem_check("d gate", dgu[:, :inter], dgate, (d * up * sig).abs() * (1 + t.abs()) * 16 * U)     # 1 + g (1 - sig) cancels near g = -1.28


# ---------------------------------------------------------------------------------------------
# causal attention, grouped KV heads
# ---------------------------------------------------------------------------------------------
LENS = [1, 31, 33, 64, 65, 127, 128, 129, 257, 0]      # both sides of every wave (32), key-tile (32 / 64) and workgroup (128) edge;
L = 257                                                # 257: the diagonal reaches the third query tile; 0: a sequence with no key


def _budget(dtype, name):
    if dtype == torch.float32:
        return 1e-4, 1e-5
    return 2e-2, (6e-3 if name == "out" else 8e-3)


def _causal_reference(q, k, v, go, kv_len, hq, hkv, scale):
    """Dense float64 attention with the tril mask combined with the key-padding mask, autograd backward.
    q, go [b, l, hq*128]; k, v [b, l, hkv*128]; a row with no visible key (kv_len = 0) has zero output and gradients."""
    b, l = q.shape[0], q.shape[1]
    rep = hq // hkv
    qd, kd, vd = (t.detach().double().requires_grad_(True) for t in (q, k, v))
    qh = qd.view(b, l, hq, 128).transpose(1, 2)
    kh = kd.view(b, l, hkv, 128).transpose(1, 2).repeat_interleave(rep, 1)
    vh = vd.view(b, l, hkv, 128).transpose(1, 2).repeat_interleave(rep, 1)
    idx = torch.arange(l, device=q.device)
    keep = (idx[None, :] <= idx[:, None])[None] & (idx[None, None, :] < kv_len.long()[:, None, None])      # [b, l, l]
    s = (qh @ kh.transpose(-1, -2)) * scale
    none = ~keep.any(-1, keepdim=True)                             # rows with no visible key (kv_len = 0): zero output, zero gradients
    s = s.masked_fill(~(keep | none)[:, None], float("-inf"))
    p = torch.softmax(s, -1) * (~none)[:, None]
    o = (p @ vh).transpose(1, 2).reshape(b, l, hq * 128)
    o.backward(go.double())
    return o.detach(), qd.grad, kd.grad, vd.grad


def _causal_case(dev, dtype, hq, hkv, fused, seed):
    from gmlm_amd import ops
    g = torch.Generator().manual_seed(seed)
    b, scale = len(LENS), 128 ** -0.5
    nq, nk = hq * 128, hkv * 128
    kv_len = torch.tensor(LENS, dtype=torch.int32, device=dev)
    valid = (torch.arange(L, device=dev)[None, :] < kv_len[:, None])[..., None]                # [b, l, 1]
    qkv = torch.randn(b, L, nq + 2 * nk, generator=g).to(dev, dtype)
    go = torch.randn(b, L, nq, generator=g).to(dev, dtype) * valid                             # nothing is pooled from padded rows

    def run():
        if fused:
            x = qkv.clone().requires_grad_(True)
            q, k, v = x[..., :nq], x[..., nq:nq + nk], x[..., nq + nk:]
            leaves = None
        else:
            q, k, v = (t.clone().contiguous().requires_grad_(True) for t in (qkv[..., :nq], qkv[..., nq:nq + nk], qkv[..., nq + nk:]))
            leaves = (q, k, v)
        out = ops.causal_attention(q, k, v, kv_len, hq, hkv, scale)
        out.backward(go)
        grads = (x.grad[..., :nq], x.grad[..., nq:nq + nk], x.grad[..., nq + nk:]) if fused else tuple(t.grad for t in leaves)
        return (out.detach(),) + tuple(t.contiguous() for t in grads)

    box = {}
    ran = kernels_run(lambda: box.setdefault("r", run()))
    tn = TN[dtype]
    assert {n for n in ran if n.startswith("causal128::")} == {f"causal128::{k}<{tn}>" for k in
                                                               ("fwd_kernel", "delta_kernel", "dq_kernel", "dkv_kernel")}, ran
    assert not any(n.startswith(("attn_", "d128::")) for n in ran), ran
    assert _same_bits(run(), box["r"])
    ref = _causal_reference(qkv[..., :nq], qkv[..., nq:nq + nk], qkv[..., nq + nk:], go, kv_len, hq, hkv, scale)
    for name, got, r_ in zip(("out", "dq", "dk", "dv"), box["r"], ref):
        assert bool(torch.isfinite(got).all()), name               # rows at or past kv_len included
        _close(name, got * valid, r_ * valid, *_budget(dtype, name))
    empty = LENS.index(0)
    assert all(float(t[empty].abs().max()) == 0.0 for t in box["r"])


@pytest.mark.parametrize("dtype", DT, ids=["bf16", "fp32"])
@pytest.mark.parametrize("fused", [False, True], ids=["contiguous", "fused_qkv"])
@pytest.mark.parametrize("hkv", [4, 2, 1])
def test_causal_attention_vs_dense_float64(dev, hkv, fused, dtype):
    _causal_case(dev, dtype, 4, hkv, fused, 11 + hkv)


@pytest.mark.parametrize("dtype", DT, ids=["bf16", "fp32"])
def test_causal_attention_full_size_head_ratio(dev, dtype):
    _causal_case(dev, dtype, 16, 8, True, 5)


@pytest.mark.parametrize("dtype", DT, ids=["bf16", "fp32"])
def test_causal_attention_online_softmax_spikes_below_the_diagonal(dev, dtype):
    """The spiked keys of test_gpu_kernels.py's rescale test, each placed just below the diagonal of the query it is aligned
    with: key 70 (second 64-key tile) for query 72, a key of a middle tile for the query two rows on, and the last key but
    one for the last query, which also sees the first two spikes (its running max jumps three times).  Spike sizes as
    there: large for fp32, s ~ 10 / 12 / 20 for bf16, whose score rounding (~|s| 2^-9) must stay inside the budget."""
    from gmlm_amd import ops
    h, l, scale = 2, 400, 128 ** -0.5
    g = torch.Generator().manual_seed(17 + 128)
    q, go, k, v = (torch.randn(1, l, h * 128, generator=g) for _ in range(4))
    a1, a2, a3 = (6.0, 9.0, 12.0) if dtype == torch.float32 else tuple(x * 8.0 / 128 ** 0.5 for x in (1.25, 1.5, 2.5))
    mid = l // 2 + 33
    k[0, 70] = q[0, 72] * a1
    k[0, mid] = q[0, mid + 2] * a2
    k[0, l - 2] = q[0, l - 1] * a3
    q, k, v, go = (t.to(dev, dtype) for t in (q, k, v, go))
    qd, kd, vd = (t.clone().requires_grad_(True) for t in (q, k, v))
    box = {}
    ran = kernels_run(lambda: box.setdefault("y", ops.causal_attention(qd, kd, vd, None, h, h, scale)))
    assert f"causal128::fwd_kernel<{TN[dtype]}>" in ran, ran
    box["y"].backward(go)
    ref = _causal_reference(q, k, v, go, torch.tensor([l], device=dev), h, h, scale)
    for name, got, r_ in zip(("out", "dq", "dk", "dv"), (box["y"].detach(), qd.grad, kd.grad, vd.grad), ref):
        _close(name, got, r_, *_budget(dtype, name))


@pytest.mark.parametrize("dtype", DT, ids=["bf16", "fp32"])
def test_fused_rope_attention_node_equals_the_two_ops(dev, dtype):
    """ops.rope_causal_attention (the node the encoder uses: V read from the fused rows, dq | dk finished in place on the
    attention's fused gradient buffer) against ops.qknorm_rope followed by ops.causal_attention, which the cases above check
    against float64: same kernels on the same values, so output, fused input gradient and both weight gradients are equal
    element for element (torch.equal: autograd's sum of the two ops' input gradients turns a -0 into +0, nothing else)."""
    from gmlm_amd import ops
    hq, hkv, scale, eps = 4, 2, 128 ** -0.5, 1e-6
    g = torch.Generator().manual_seed(23)
    nq, nk = hq * 128, hkv * 128
    lens = [n for n in LENS if n <= 129]
    b, l = len(lens), 129
    kv_len = torch.tensor(lens, dtype=torch.int32, device=dev)
    qkv = torch.randn(b, l, nq + 2 * nk, generator=g).to(dev, dtype)
    qw, kw = (torch.empty(128).uniform_(0.5, 1.5, generator=g).to(dev) for _ in range(2))
    cs = _rope_table(l + 7, 1e6, dev)                              # a table longer than the sequence: a prefix is read
    go = torch.randn(b, l, nq, generator=g).to(dev, dtype)

    def run(fused):
        x, qv, kv = qkv.clone().requires_grad_(True), qw.clone().requires_grad_(True), kw.clone().requires_grad_(True)
        if fused:
            out = ops.rope_causal_attention(x, qv, kv, cs, kv_len, hq, hkv, scale, eps)
        else:
            qk = ops.qknorm_rope(x, qv, kv, cs, hq, hkv, eps)
            out = ops.causal_attention(qk[..., :nq], qk[..., nq:], x[..., nq + nk:], kv_len, hq, hkv, scale)
        out.backward(go)
        return out.detach(), x.grad, qv.grad, kv.grad

    box = {}
    ran = kernels_run(lambda: box.setdefault("r", run(True)))
    tn = TN[dtype]
    for k in ("qknorm_rope_fwd_kernel", "qknorm_rope_bwd_kernel", "causal128::fwd_kernel", "causal128::dq_kernel", "causal128::dkv_kernel"):
        assert f"{k}<{tn}>" in ran, (k, ran)
    two = run(False)
    for name, a, r_ in zip(("out", "dqkv", "dq_weight", "dk_weight"), box["r"], two):
        assert bool(torch.isfinite(a).all()) and float(a.abs().max()) > 0, name
        assert torch.equal(a, r_), name
