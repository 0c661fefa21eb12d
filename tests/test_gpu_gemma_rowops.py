"""The row kernels of the Gemma3 encoder (csrc/gemma_kernels.hip: sandwich RMSNorm pair, Q / K head norm + rotary embedding at
head dim 256, tanh-GELU gated unit) against float64 torch on the same rounded inputs, bf16 and fp32, forward and backward;
every case asserts by name which kernels ran and that a second identical call gives identical bits.

Formulas and budgets are those of tests/test_gpu_decoder_ops.py (its docstring derives them): per element one ulp of the storage
type at the reference (bf16) or four (fp32), plus an absolute term for the fp32 arithmetic behind it, written out where it is
used; a value that is a function of a tensor the kernel itself stored (y and the backward of the stored s') is checked against
float64 of the STORED tensor.  What the new kernels add to those terms:
 * sandwich norm: TWO row statistics.  s' carries the first (half of ``_stat`` through rstd_b) on its branch term only; y and
   ds' carry the second exactly as add_rmsnorm's y and da do; db carries both: the first as a norm backward of its own, and the
   error of ds' (which the kernel keeps in fp32: no storage rounding in between) propagated through that backward;
 * tanh-GELU: the argument 2u of the exponential is a cubic of the gate formed with 3 roundings, so exp(-2|u|) has relative
   error 3 * 2^-24 * 2|u| beside its own 2 ulps; it reaches the result at full weight where sigmoid(2u) = e / (1 + e) (u < 0).
Weight gradients: rel-L2 1e-5 (fp32) / 8e-3 (bf16), the tree's.

The input builders and float64 references are module-level functions without a device argument of their own, so that
tests/test_gemma3_cpu.py can evaluate the kernels' expressions in fp32 on the CPU on the very same inputs."""
import math

import pytest
import torch

from helpers import kernels_run
from test_gpu_decoder_matrix import SAT_GATES
from test_gpu_decoder_ops import TN, U, _elem_check, _rel_l2, _same_bits, _stat

pytestmark = pytest.mark.gpu

DT = [torch.bfloat16, torch.float32]
EPS = 1e-6
SAND_WIDTHS = (8, 640, 768, 1152, 4096)          # 8: one chunk of one lane; 640 / 768 / 1152: the Gemma3 widths; 4096: the widest
SAND_ROWS = (1, 3, 257)                          # less than a block of 4 rows, and 64 blocks + 1 row
KA, KB = 0.7978845608028654, 0.044715


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _ch(f, dtype):
    need = -(-(f // (8 if dtype == torch.bfloat16 else 4)) // 64)
    return next(c for c in (2, 4, 8, 16) if need <= c)


# ---------------------------------------------------------------------------------------------
# sandwich RMSNorm
# ---------------------------------------------------------------------------------------------
def sandwich_inputs(rows, f, dtype, device="cpu"):
    """s, b, gy, gs in the storage type; w_post, w_pre fp32 drawn from U(-0.5, 0.5): with w_offset = 1 the weights are
    U(0.5, 1.5).  With 3 rows, row 1 is all zero in s AND b."""
    g = torch.Generator().manual_seed(rows * 7 + f)
    s = torch.randn(rows, f, generator=g)
    b = 3.0 * torch.randn(rows, f, generator=g)                    # a block output is not unit-scale: the post norm matters
    if rows == 3:
        s[1], b[1] = 0.0, 0.0
    wpo, wpr = (torch.empty(f).uniform_(-0.5, 0.5, generator=g) for _ in range(2))
    gy, gs = (torch.randn(rows, f, generator=g) for _ in range(2))
    return tuple(t.to(device, dtype) for t in (s, b, gy, gs)) + (wpo.to(device), wpr.to(device))


def sandwich_reference(s, b, sp, wpo, wpr, off, gy, gs, lanes=64):
    """float64 values and their absolute extras: s' (of s, b), then y, ds', db of the STORED s' (``sp``).  ``s`` / ``gs`` may be None."""
    f = b.shape[-1]
    st = _stat(f, lanes)
    bd, spd, gyd = b.double(), sp.double(), gy.double()
    sd = torch.zeros_like(bd) if s is None else s.double()
    gsd = torch.zeros_like(bd) if gs is None else gs.double()
    wo, wr = off + wpo.double(), off + wpr.double()
    rb = (bd.pow(2).mean(-1, keepdim=True) + EPS).rsqrt()
    n = bd * rb * wo
    # n: half the statistic through rstd_b and six roundings ((off + w); / f and + eps, half each through the root; the root;
    # 1 / x; two products).  The fp32 add s + n in front of the store rounds |s| + |n| once more, and that rounding is not the
    # store's own when the store is bf16: counted on both sides of it
    out = {"sp": (sd + n, n.abs() * (0.5 * st + 6 * U) + 2 * U * (sd.abs() + n.abs()))}
    rs = (spd.pow(2).mean(-1, keepdim=True) + EPS).rsqrt()
    yr = spd * rs * wr
    out["y"] = (yr, yr.abs() * (0.5 * st + 5 * U))                   # add_rmsnorm's 4 u and one for off + w, formed in the kernel
    g = gyd * wr
    xh = spd * rs
    m = (g * xh).mean(-1, keepdim=True)
    m_abs = (g * xh).abs().mean(-1, keepdim=True)
    dsp = gsd + rs * (g - xh * m)
    e_ds = 4 * U * (gsd.abs() + rs * (g.abs() + (xh * m).abs())) + rs * xh.abs() * st * m_abs + 0.5 * st * rs * (g.abs() + (xh * m).abs()) \
        + U * rs * g.abs()                                            # add_rmsnorm's da, and one rounding for off + w inside g
    out["ds"] = (dsp, e_ds)
    h = dsp * wo
    bh = bd * rb
    m1 = (h * bh).mean(-1, keepdim=True)
    m1_abs = (h * bh).abs().mean(-1, keepdim=True)
    eh = e_ds * wo.abs()
    e_db = 4 * U * rb * (h.abs() + (bh * m1).abs()) + rb * bh.abs() * st * m1_abs + 0.5 * st * rb * (h.abs() + (bh * m1).abs()) \
        + rb * (eh + bh.abs() * (eh * bh.abs()).mean(-1, keepdim=True))
    out["db"] = (rb * (h - bh * m1), e_db)
    out["dw_post"], out["dw_pre"] = (dsp * bh).sum(0), (gyd * xh).sum(0)
    out["rstd"] = (rb[:, 0], rs[:, 0])
    return out


@pytest.mark.parametrize("dtype", DT, ids=["bf16", "fp32"])
@pytest.mark.parametrize("off", [1.0, 0.0], ids=["offset1", "offset0"])
@pytest.mark.parametrize("with_s", [True, False], ids=["residual", "plain"])
@pytest.mark.parametrize("f", SAND_WIDTHS)
def test_sandwich_rmsnorm(dev, f, with_s, off, dtype):
    from gmlm_amd import ops
    for rows in SAND_ROWS:
        s, b, gy, gs, wpo, wpr = sandwich_inputs(rows, f, dtype, dev)
        if off == 0.0:
            wpo, wpr = wpo + 1.0, wpr + 1.0                           # plain weights around 1
        if not with_s:
            s = None

        def run():
            sv = s.clone().requires_grad_(True) if with_s else None
            bv, w1, w2 = b.clone().requires_grad_(True), wpo.clone().requires_grad_(True), wpr.clone().requires_grad_(True)
            sp, y = ops.sandwich_rmsnorm(sv, bv, w1, w2, off, EPS)
            stats = y.grad_fn.saved_tensors[4]
            torch.autograd.backward([sp, y], [gs, gy])
            return sp.detach(), y.detach(), (sv.grad if with_s else bv.grad), bv.grad, w1.grad, w2.grad, stats[0], stats[1]

        box = {}
        ran = kernels_run(lambda: box.setdefault("r", run()))
        sp, y, ds, db, dw1, dw2, rstd_b, rstd_s = box["r"]
        tn, ch = TN[dtype], _ch(f, dtype)
        assert f"gemma_kernels::sandwich_fwd_kernel<{tn}, {ch}>" in ran and f"gemma_kernels::sandwich_bwd_kernel<{tn}, {ch}>" in ran, ran
        assert any(n.startswith(f"col_reduce_partial_kernel<2, gmlm::gemma_kernels::SandwichDwFn<{tn}>") for n in ran), ran
        assert not any(n.startswith(("rmsnorm_", "ln_", "add_ln_")) for n in ran), ran
        assert _same_bits(run(), box["r"])                            # column sums included: fixed order, no atomics
        ref = sandwich_reference(s, b, sp, wpo, wpr, off, gy, gs)
        print(f"\nsandwich rows={rows} f={f} residual={with_s} offset={off} {dtype}:")
        _elem_check("s'", sp, *ref["sp"])
        _elem_check("y", y, *ref["y"])
        if with_s:
            _elem_check("ds", ds, *ref["ds"])
        _elem_check("db", db, *ref["db"])
        if rows > 1:                                                  # one row: the "sum" is a single product
            _rel_l2("dw_post", dw1, ref["dw_post"], dtype)
            _rel_l2("dw_pre", dw2, ref["dw_pre"], dtype)
        for name, got, want in (("rstd_b", rstd_b, ref["rstd"][0]), ("rstd_s", rstd_s, ref["rstd"][1])):
            assert float(((got.double() - want).abs() / want).max()) <= 0.5 * _stat(f, 64) + 4 * U, name
        if rows == 3:                                                 # the all-zero row: rstd = eps^-1/2, everything finite
            assert abs(float(rstd_b[1]) - EPS ** -0.5) <= 1e-6 * EPS ** -0.5 and abs(float(rstd_s[1]) - EPS ** -0.5) <= 1e-6 * EPS ** -0.5
            assert float(sp[1].abs().max()) == 0.0 and float(y[1].abs().max()) == 0.0
            assert all(bool(torch.isfinite(t).all()) for t in (ds, db, dw1, dw2))


def test_sandwich_statistics_come_from_the_stored_sum(dev):
    """bf16: the second statistic is taken from the ROUNDED s' (what every later kernel reads), not from the fp32 sum.  With
    s = 256 and a branch term of 0.5 the stored sum is 256 (the bf16 spacing there is 2) and rstd_s is 1 / 256 to fp32 rounding;
    from the unrounded 256.5 it would be 2e-3 smaller, relatively."""
    from gmlm_amd import ops
    f = 64
    s = torch.full((1, f), 256.0, device=dev, dtype=torch.bfloat16)
    b = torch.full((1, f), 0.5, device=dev, dtype=torch.bfloat16).requires_grad_(True)
    z = torch.zeros(f, device=dev)
    sp, y = ops.sandwich_rmsnorm(s, b, z - 0.5, z, 1.0, EPS)          # b * rstd_b * (1 - 0.5) = 0.5
    rstd_s = y.grad_fn.saved_tensors[4][1]
    assert float(sp.float().min()) == 256.0 and float(sp.float().max()) == 256.0
    assert abs(float(rstd_s[0]) * 256.0 - 1.0) <= 1e-6
    assert float((y.float() - 1.0).abs().max()) == 0.0


def test_sandwich_node_under_frozen_inputs(dev):
    """One gradient entry per input whatever is frozen; the unfrozen ones have the bits of the all-trainable run; either output
    used alone works."""
    from gmlm_amd import ops
    s, b, gy, gs, wpo, wpr = sandwich_inputs(5, 640, torch.float32, dev)

    def run(train, use=(True, True)):
        leaves = [t.clone().requires_grad_(i in train) for i, t in enumerate((s, b, wpo, wpr))]
        sp, y = ops.sandwich_rmsnorm(*leaves, 1.0, EPS)
        outs = [(o, g) for o, g, u in ((sp, gs, use[0]), (y, gy, use[1])) if u]
        torch.autograd.backward([o for o, _ in outs], [g for _, g in outs])
        return [t.grad for t in leaves]

    full = run({0, 1, 2, 3})
    for train in ({0}, {1}, {2, 3}, {0, 3}, {1, 2}):
        got = run(train)
        for i in range(4):
            assert (got[i] is not None) == (i in train) and (got[i] is None or torch.equal(got[i], full[i])), (train, i)
    only_s = run({0, 1, 2, 3}, use=(True, False))                     # y unused: ds = gs, dw_pre = 0
    assert torch.equal(only_s[0], gs) and float(only_s[3].abs().max()) == 0.0
    assert all(bool(torch.isfinite(t).all()) for t in run({0, 1, 2, 3}, use=(False, True)))
    with torch.no_grad():
        sp, y = ops.sandwich_rmsnorm(s, b, wpo, wpr, 1.0, EPS)
    assert not sp.requires_grad and not y.requires_grad


# ---------------------------------------------------------------------------------------------
# Q / K head norm + RoPE at head dim 256
# ---------------------------------------------------------------------------------------------
def _rope_table(max_len, theta, dev):
    inv = 1.0 / (theta ** (torch.arange(0, 256, 2, dtype=torch.float) / 256))
    fr = torch.arange(max_len, dtype=torch.float32)[:, None] * inv[None]
    return torch.stack([fr.cos(), fr.sin()], 1).contiguous().to(dev)


def _rot(n, cos, sin):
    lo, hi = n[..., :128], n[..., 128:]
    return torch.cat([lo * cos - hi * sin, hi * cos + lo * sin], -1)


def _rot_mag(n, cos, sin):
    lo, hi = n[..., :128].abs(), n[..., 128:].abs()
    return torch.cat([lo * cos.abs() + hi * sin.abs(), hi * cos.abs() + lo * sin.abs()], -1)


@pytest.mark.parametrize("dtype", DT, ids=["bf16", "fp32"])
@pytest.mark.parametrize("by_pos", [False, True], ids=["seq_len", "pos_ids"])
@pytest.mark.parametrize("hq,hkv", [(3, 1), (4, 2)])
def test_qknorm_rope_d256(dev, hq, hkv, by_pos, dtype):
    """[2, 300] tokens at positions 0..299 (``seq_len``), or 600 packed rows at scattered positions up to 511 (``pos_ids``); the
    input is a strided slice of a wider buffer; q and k weights differ; weight offset 1.  Forward out of place and in place
    (same bits, V bytes untouched), backward in place on dqkv (V columns untouched)."""
    from gmlm_amd import ops_gemma as og
    g = torch.Generator().manual_seed(hq * 10 + hkv)
    b, l, off = 2, 300, 1.0
    wid, nqk = (hq + 2 * hkv) * 256, (hq + hkv) * 256
    buf = torch.randn(b, l, wid + 64, generator=g).to(dev, dtype)
    qw, kw = (torch.empty(256).uniform_(-0.5, 0.5, generator=g).to(dev) for _ in range(2))
    cs = _rope_table(512, 1e4, dev)
    go = torch.randn(b, l, nqk, generator=g).to(dev, dtype)
    if by_pos:
        buf, go = buf.reshape(b * l, -1), go.reshape(b * l, -1)
        pos = torch.randint(0, 512, (b * l,), generator=g)
        pos[:4] = torch.tensor([0, 1, 127, 511])
        pos_d = pos.to(dev, torch.int32)
    else:
        pos, pos_d = torch.arange(l).repeat(b), None
    qkv = buf[..., :wid]
    assert qkv.stride(-2) == wid + 64

    def run():
        out, rstd = og.qknorm_rope_d256(qkv, qw, kw, cs, hq, hkv, off, EPS, pos_d)
        dqkv = torch.full_like(buf, 7.0)[..., :wid]
        dqkv[..., :nqk] = go
        dwt = og.qknorm_rope_d256_bwd_(dqkv, qkv, qw, kw, cs, rstd, hq, hkv, off, pos_d)
        return out, dqkv.clone(), dwt[0].clone(), dwt[1].clone()

    box = {}
    ran = kernels_run(lambda: box.setdefault("r", run()))
    out, dx, dqw, dkw = box["r"]
    tn = TN[dtype]
    assert f"gemma_kernels::qknorm_rope_fwd_kernel<{tn}>" in ran and f"gemma_kernels::qknorm_rope_bwd_kernel<{tn}>" in ran, ran
    assert not any(n.startswith("qknorm_rope_") for n in ran), ran                     # the d = 128 kernels stay out of it
    assert _same_bits(run(), box["r"])
    assert float((dx[..., nqk:] - 7.0).abs().max()) == 0.0                              # backward in place: V columns untouched
    own = buf.clone()
    og.qknorm_rope_d256(own[..., :wid], qw, kw, cs, hq, hkv, off, EPS, pos_d, out=own[..., :wid])
    assert torch.equal(own[..., :nqk], out) and torch.equal(own[..., nqk:], buf[..., nqk:])   # in place: same bits, V bytes unchanged

    rows = b * l
    x = qkv.double().reshape(rows, hq + 2 * hkv, 256)[:, :hq + hkv]
    wd = off + torch.cat([qw.double().expand(hq, 256), kw.double().expand(hkv, 256)])[None]
    cos, sin = cs[pos.to(dev), 0].double()[:, None, :], cs[pos.to(dev), 1].double()[:, None, :]
    st = _stat(256, 32 if dtype == torch.bfloat16 else 64)
    rstd = (x.pow(2).mean(-1, keepdim=True) + EPS).rsqrt()
    xh = x * rstd
    n = xh * wd
    ref, mag = _rot(n, cos, sin), _rot_mag(n, cos, sin)
    print(f"\nqknorm_rope_d256 {hq}/{hkv} by_pos={by_pos} {dtype}:")
    _elem_check("out", out.reshape(rows, hq + hkv, 256), ref, mag * (0.5 * st + 5 * U))
    gd = go.double().reshape(rows, hq + hkv, 256)
    dn, dn_mag = _rot(gd, cos, -sin), _rot_mag(gd, cos, sin)
    gr = dn * wd
    m = (gr * xh).mean(-1, keepdim=True)
    m_abs = (dn_mag * wd * xh.abs()).mean(-1, keepdim=True)
    dxr = rstd * (gr - xh * m)
    extra = rstd * ((4 * U + 0.5 * st) * (dn_mag * wd + (xh * m).abs()) + xh.abs() * (st + 4 * U) * m_abs)
    _elem_check("dx (q | k)", dx.reshape(rows, hq + 2 * hkv, 256)[:, :hq + hkv], dxr, extra)
    _rel_l2("dq_weight", dqw, (dn * xh)[:, :hq].sum((0, 1)), dtype)
    _rel_l2("dk_weight", dkw, (dn * xh)[:, hq:].sum((0, 1)), dtype)
    assert float((dqw - dkw).abs().max()) > 0


def test_rope_gqa_node_under_frozen_inputs(dev):
    """``ops.rope_gqa_d256``: one gradient entry per input; frozen norm weights or a frozen qkv leave the other gradients' bits
    unchanged; the packed form of the same rows gives the padded bits."""
    from gmlm_amd import ops
    hq, hkv, l = 3, 1, 40
    g = torch.Generator().manual_seed(3)
    qkv = torch.randn(2, l, (hq + 2 * hkv) * 256, generator=g).to(dev)
    qw, kw = (torch.empty(256).uniform_(-0.5, 0.5, generator=g).to(dev) for _ in range(2))
    cs = _rope_table(64, 1e4, dev)
    go = torch.randn(2, l, hq * 256, generator=g).to(dev)

    def run(train, packed=False):
        leaves = [t.clone().requires_grad_(i in train) for i, t in enumerate((qkv, qw, kw))]
        if packed:
            pos = torch.arange(l, device=dev).repeat(2)
            cu = torch.tensor([0, l, 2 * l], dtype=torch.int32, device=dev)
            out = ops.rope_gqa_d256_varlen(leaves[0].reshape(2 * l, -1), leaves[1], leaves[2], cs, pos, cu, l, hq, hkv, 0.07, True)
            out.backward(go.reshape(2 * l, -1))
        else:
            out = ops.rope_gqa_d256(*leaves, cs, None, hq, hkv, 0.07, True)
            out.backward(go)
        return out.detach(), [t.grad for t in leaves]

    orig = qkv.clone()
    out, full = run({0, 1, 2})
    for train in ({0}, {1, 2}, {0, 2}):
        o, got = run(train)
        assert torch.equal(o, out)
        for i in range(3):
            assert (got[i] is not None) == (i in train) and (got[i] is None or torch.equal(got[i], full[i])), (train, i)
    o, got = run({0, 1, 2}, packed=True)
    assert torch.equal(o.reshape(out.shape), out) and torch.equal(got[0], full[0])
    assert torch.equal(qkv, orig)                                                       # the node does not rewrite its input
    with torch.no_grad():
        assert torch.equal(ops.rope_gqa_d256(qkv, qw, kw, cs, None, hq, hkv, 0.07, True), out)


# ---------------------------------------------------------------------------------------------
# tanh-GELU gated unit
# ---------------------------------------------------------------------------------------------
GLU_SHAPES = ((1, 384), (130, 1152), (3, 10 * 8))       # Gemma3-270m's intermediate has 2,048; 1,152 is EmbeddingGemma's; 80: SAT_GATES


def geglu_inputs(rows, inter, dtype, device="cpu"):
    """(gate_up, dy) in the storage type; at inter = 80 gate column j is fixed at SAT_GATES[j % 10]."""
    g = torch.Generator().manual_seed(rows + inter)
    gu = 2.0 * torch.randn(rows, 2 * inter, generator=g)
    gy = torch.randn(rows, inter, generator=g)
    if inter == 80:
        gu[:, :inter] = torch.tensor(SAT_GATES)[torch.arange(inter) % len(SAT_GATES)]
    return gu.to(device, dtype), gy.to(device, dtype)


def geglu_reference(gu, gy):
    """float64 y, d up, d gate with their absolute extras (see the module docstring)."""
    inter = gu.shape[-1] // 2
    gt, up, d = gu[:, :inter].double(), gu[:, inter:].double(), gy.double()
    u = KA * (gt + KB * gt ** 3)
    sig = torch.sigmoid(2 * u)
    rel = (12 + 6 * 2 * u.abs()) * U                                  # e's argument: 3 roundings of 2|u|, twice for safety
    yr = gt * sig * up
    dup = d * gt * sig
    t = gt * (1 - sig) * 2 * KA * (1 + 3 * KB * gt ** 2)
    dgate = d * up * sig * (1 + t)
    return (yr, yr.abs() * rel), (dup, dup.abs() * rel), (dgate, (d * up * sig).abs() * (1 + t.abs()) * (rel + 4 * U))


@pytest.mark.parametrize("dtype", DT, ids=["bf16", "fp32"])
@pytest.mark.parametrize("rows,inter", GLU_SHAPES)
def test_geglu_tanh(dev, rows, inter, dtype):
    from gmlm_amd import ops
    gu, gy = geglu_inputs(rows, inter, dtype, dev)

    def run():
        v = gu.clone().requires_grad_(True)
        y = ops.geglu_tanh(v)
        y.backward(gy)
        return y.detach(), v.grad

    box = {}
    ran = kernels_run(lambda: box.setdefault("r", run()))
    y, dgu = box["r"]
    assert f"gemma_kernels::geglu_tanh_fwd_kernel<{TN[dtype]}>" in ran and f"gemma_kernels::geglu_tanh_bwd_kernel<{TN[dtype]}>" in ran, ran
    assert not any(n.startswith(("swiglu_", "mbert::", "bias_gelu_")) for n in ran), ran
    assert _same_bits(run(), box["r"])
    (yr, ey), (dup, eu), (dgate, eg) = geglu_reference(gu, gy)
    print(f"\ngeglu_tanh rows={rows} inter={inter} {dtype}:")
    _elem_check("y", y, yr, ey)
    _elem_check("d up", dgu[:, inter:], dup, eu)
    _elem_check("d gate", dgu[:, :inter], dgate, eg)
    ref = torch.nn.functional.gelu(gu[:, :inter].double(), approximate="tanh") * gu[:, inter:].double()
    assert float((yr - ref).abs().max()) <= 1e-12 * max(1.0, float(ref.abs().max()))       # the reference IS torch's tanh GELU
    if inter == 80:
        gates = gu[0, :10].double().tolist()
        assert max(abs(x) for x in gates) == 60.0 and math.copysign(1.0, gates[1]) == -1.0
        up, d = gu[:, inter:].float(), gy.float()
        cols = torch.arange(inter, device=dev) % 10
        hi, lo = (cols == 2) | (cols == 4) | (cols == 6), (cols == 3) | (cols == 5) | (cols == 7)
        gcol = gu[:, :inter].float()
        # saturated gates: exactly g * up and d * up (one rounding each), exactly 0 on the other side; nothing is NaN
        assert torch.equal(y[:, hi].float(), (gcol[:, hi] * up[:, hi]).to(dtype).float())
        assert torch.equal(dgu[:, :inter][:, hi].float(), (d[:, hi] * up[:, hi]).to(dtype).float())
        assert float(y[:, lo].abs().max()) == 0.0 and float(dgu[:, :inter][:, lo].abs().max()) == 0.0
        assert float(dgu[:, inter:][:, lo].abs().max()) == 0.0
        assert bool(torch.isfinite(y).all()) and bool(torch.isfinite(dgu).all())
