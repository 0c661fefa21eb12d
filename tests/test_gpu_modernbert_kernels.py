"""The ModernBERT kernels (modernbert_kernels.hip, attn_window.hip: ``mbert::*``) at the edges of their loops, against float64
torch on the CPU on the same rounded inputs.  Every case rounds its inputs to the storage type first, asserts the kernels it
launched by name, and asserts that a second identical call gives identical bits.

1. Band-limited attention (``mbert::window_*``), h = 2, d = 64, both dtypes, the fused [q | k | v] buffer.
   Padded: l in ``PAD_LS`` = 1, 32, 33, 129, 257, one sequence per key count in {0, 1, 31, 33, l - 1, l} (those <= l), every
   window of ``WINDOWS`` = 0, 1, 16, 31, 32, 33, 64, 300: both sides of a 32-key block and of a 128-row workgroup, and a window
   >= l.  Packed: sequences of ``PACKED_LENS`` tokens plus one of length 0.  EVERY row carries an output gradient and is
   compared, the rows at or past the key count included (they see the keys below it that lie within the window).  A row
   with no visible key must be exactly 0 in out and dq, with lse = -inf; keys at or past the key count have dk = dv = 0.
   Error measure and budgets: ``_close`` with ``test_gpu_attention_matrix._budget`` over the whole tensor.  Where the
   reference gradient is identically 0 (window 0 or l = 1: every visible row has ONE key, probability 1, so dq = dk = 0) a
   relative measure has nothing to divide by and the absolute bound of ``_one_key_bounds`` holds instead (its docstring).
2. add + LayerNorm: the rows and widths of test_gpu_decoder_matrix.RMS_CASES (both sides of every chunk boundary, 4096) plus
   768 and 1024, a zero row; budgets of its RMSNorm cases.  The statistic bound is ``rms_stat``'s, taken twice: a lane adds
   its elements in sequence before the 6 butterfly steps, once for the mean (error <= st mean|s|) and once for the squared
   deviations (relative error st of their sum, of which rstd = (.)^-1/2 takes half; st is kept whole).  The error of the
   mean and the subtraction's own rounding enter xhat = (s - mean) rstd, and through xhat both y and the backward's
   rstd (g - mean(g) - xhat mean(g xhat)).
3. Rotary embedding at d = 64 in place: padded and by position (clamped), a table of one row, a tail block; the rotation's
   budget of the Qwen3 rope cases without the norm terms: each output is two products and one add, 3 u of the magnitude sum
   on top of the storage rounding; forward then backward on the same buffer restores the input to 2 roundings of the
   storage type + 8 u (R^T R = I only to the fp32 rounding of the table's cos and sin, and each rotation adds its 3 u).
4. GeGLU: the shapes of SWIGLU_CASES (second trips included); budget of the SwiGLU cases with the activation's own error:
   erff (fp32) is taken within 4 ulp at 1 and the bf16 kernels' polynomial erf within 1.5e-7 absolute (common.hpp), so
   |gelu err| <= |g| (8 u + 1.5e-7 bf) / 2 + 8 u |gelu|, likewise for the derivative."""
import math
import zlib

import pytest
import torch

from helpers import _close, kernels_run
from test_gpu_attention_matrix import _budget
from test_gpu_decoder_matrix import RMS_CASES, RmsCase, SWIGLU_CASES, rms_stat, swiglu_inputs
from test_gpu_decoder_ops import TN, U, _elem_check, _rel_l2, _same_bits

pytestmark = pytest.mark.gpu

BF, FP = torch.bfloat16, torch.float32
DTYPES = (BF, FP)
H, D, HD = 2, 64, 128
SCALE = D ** -0.5
WINDOWS = (0, 1, 16, 31, 32, 33, 64, 300)
PAD_LS = (1, 32, 33, 129, 257)
PACKED_LENS = (1, 31, 33, 64, 65, 127, 128, 129, 257, 0)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def _mbert(ran):
    return {n for n in ran if n.startswith("mbert::")}


# ---------------------------------------------------------------------------------------------- 1. band-limited attention
def _band_reference(qkv, go, n_keys, window):
    """float64 band-limited attention of ONE sequence on the CPU: qkv [l, 3 * HD], go [l, HD], ``n_keys`` visible key count ->
    (out, dq, dk, dv, lse [H, l], alive [l]).  A row without a visible key: zero output, zero gradients, lse = -inf."""
    l = qkv.shape[0]
    heads = lambda t: t.double().reshape(l, H, D).transpose(0, 1).contiguous()
    q, k, v = (heads(qkv[:, i * HD:(i + 1) * HD]).requires_grad_(True) for i in range(3))
    i, j = torch.arange(l)[:, None], torch.arange(l)[None, :]
    mask = ((i - j).abs() <= window) & (j < n_keys)
    alive = mask.any(1)
    s = (q @ k.transpose(1, 2)) * SCALE
    s = s.masked_fill(~(mask | ~alive[:, None]), float("-inf"))       # a dead row keeps all its scores: no NaN, zeroed below
    p = torch.softmax(s, -1) * alive[:, None]
    o = p @ v
    o.backward(heads(go))
    lse = torch.logsumexp(s.detach(), -1).masked_fill(~alive[None, :], float("-inf"))
    back = lambda t: t.detach().transpose(0, 1).reshape(l, HD)
    return back(o), back(q.grad), back(k.grad), back(v.grad), lse, alive


def _one_key_bounds(qkv, go, dtype):
    """Every visible row has ONE key (itself, or key 0): its probability is 1 whatever q and k are, so dq and dk are exactly 0.
    The kernels form dS = P (dP - delta) with dP = dO . v and delta = dO . O (O = v): two fp32 evaluations of ONE 64-term
    dot product, each within (64 + 2) u sum |dO_i v_i| of it, so |dS| <= 2 (64 + 2) u P sum |dO_i| |v_i|.  The bf16 kernels
    carry delta into the MFMA as two bf16 numbers (hi + lo), which leaves up to 64 u |delta| behind, round dS and the result
    to bf16 (1 + 2^-7), and form P = exp2(s' - lse) from a score whose q (or k) operand was rounded to bf16 once more: s' is
    within 2^-8 sum |q_i k_i| scale log2 e of s, so P <= exp2 of that.  Then dq = scale dS k, dk = scale dS q (row sums over
    the at most 2 w + 1 = 1 or l = 1 partners: one term)."""
    bf = dtype == BF
    l = qkv.shape[0]
    q, k, v = (qkv[:, i * HD:(i + 1) * HD].double().reshape(l, H, D) for i in range(3))
    pmax = torch.exp2((q.abs() * k.abs()).sum(-1) * SCALE * 1.4427 * 2.0 ** -8) if bf else 1.0
    ds = (2 * (D + 2) + 64 * bf) * U * (1 + 2.0 ** -7 * bf) * pmax * (go.double().reshape(l, H, D).abs() * v.abs()).sum(-1)
    return (SCALE * ds[..., None] * k.abs()).reshape(l, HD), (SCALE * ds[..., None] * q.abs()).reshape(l, HD)


def _window_run(dev, qkv, go, kv_len, window, cu, max_len):
    from gmlm_amd import ops
    want_lo = qkv.dtype == BF

    def run():
        out, out_lo, lse = ops._window_fwd(qkv, kv_len, H, SCALE, window, cu, max_len, want_lo)
        dqkv = torch.full_like(qkv, float("nan"))
        ops._window_bwd(qkv, out, out_lo, go, lse, kv_len, H, SCALE, window, cu, max_len, dqkv)
        return out, dqkv, lse

    box = {}
    ran = kernels_run(lambda: box.setdefault("r", run()))
    tn = TN[qkv.dtype]
    assert _mbert(ran) == {f"mbert::window_{k}_kernel<{tn}>" for k in ("fwd", "delta", "dq", "dkv")}, sorted(ran)
    assert not any(n.startswith(("attn_", "d128::", "d32::", "causal128::")) for n in ran), sorted(ran)
    again = run()
    assert _same_bits(again[:2], box["r"][:2]) and torch.equal(again[2], box["r"][2])
    return box["r"]


def _check_sequences(dtype, window, seqs, one_key):
    """``seqs``: [(qkv, go, n_keys, out, dqkv, lse)] per sequence, all on the CPU; whole-tensor ``_close`` over their concatenation."""
    got, ref, bounds = [[] for _ in range(4)], [[] for _ in range(4)], [[], []]
    for qkv, go, n_keys, out, dqkv, lse in seqs:
        l = qkv.shape[0]
        r_out, r_dq, r_dk, r_dv, r_lse, alive = _band_reference(qkv, go, n_keys, window)
        for i, (g_, r_) in enumerate(zip((out, dqkv[:, :HD], dqkv[:, HD:2 * HD], dqkv[:, 2 * HD:]), (r_out, r_dq, r_dk, r_dv))):
            assert bool(torch.isfinite(g_).all())
            got[i].append(g_.double())
            ref[i].append(r_)
        dead = ~alive
        assert float(out[dead].abs().sum()) == 0.0 and float(dqkv[dead, :HD].abs().sum()) == 0.0        # exactly zero
        assert bool((lse[:, dead] == float("-inf")).all()) and bool(torch.isfinite(lse[:, alive]).all())
        e = (lse[:, alive].double() - r_lse[:, alive]).abs().max() if bool(alive.any()) else 0.0
        assert float(e) <= (1e-4 if dtype == FP else 2e-2), float(e)
        past = torch.arange(l) >= n_keys
        assert float(dqkv[past, HD:].abs().sum()) == 0.0                                               # keys past the count: no gradient
        if one_key:
            bq, bk = _one_key_bounds(qkv, go, dtype)
            bounds[0].append(bq)
            bounds[1].append(bk)
    got, ref = [torch.cat(x) for x in got], [torch.cat(x) for x in ref]
    for i, name in enumerate(("out", "dq", "dk", "dv")):
        if one_key and name in ("dq", "dk"):
            assert float(ref[i].abs().max()) == 0.0
            bound = torch.cat(bounds[i - 1])
            worst = float((got[i].abs() / bound.clamp_min(1e-300)).max())
            print(f"  {name}: reference exactly 0, max |got| / bound = {worst:.3f}")
            assert bool((got[i].abs() <= bound).all()), (name, worst)
        elif float(ref[i].abs().max()) == 0.0:                     # nothing visible anywhere (all key counts 0)
            assert float(got[i].abs().max()) == 0.0, name
        else:
            _close(name, got[i], ref[i], *_budget(dtype, name))


def _kv_lens(l):
    return sorted({n for n in (0, 1, 31, 33, l - 1, l) if 0 <= n <= l})


@pytest.mark.parametrize("window", WINDOWS)
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp32"])
def test_window_attention_padded_vs_float64(dev, dtype, window):
    for l in PAD_LS:
        lens = _kv_lens(l)
        b = len(lens)
        g = torch.Generator().manual_seed(zlib.crc32(f"pad{l}w{window}".encode()))
        qkv = torch.randn(b, l, 3 * HD, generator=g)
        qkv[..., HD:2 * HD] *= 1.5                                  # scores ~ N(0, 1.5): neither flat nor one-hot
        qkv, go = qkv.to(dtype), torch.randn(b, l, HD, generator=g).to(dtype)
        kv_len = torch.tensor(lens, dtype=torch.int32, device=dev)
        out, dqkv, lse = (t.cpu() for t in _window_run(dev, qkv.to(dev), go.to(dev), kv_len, window, None, 0))
        print(f"\nl = {l}, window = {window}, key counts {lens}")
        seqs = [(qkv[i], go[i], lens[i], out[i], dqkv[i], lse[i]) for i in range(b)]
        _check_sequences(dtype, window, seqs, one_key=(window == 0 or l == 1))


@pytest.mark.parametrize("window", WINDOWS)
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp32"])
def test_window_attention_packed_vs_float64(dev, dtype, window):
    lens = list(PACKED_LENS)
    total = sum(lens)
    g = torch.Generator().manual_seed(zlib.crc32(f"packed w{window}".encode()))
    qkv = torch.randn(total, 3 * HD, generator=g)
    qkv[:, HD:2 * HD] *= 1.5
    qkv, go = qkv.to(dtype), torch.randn(total, HD, generator=g).to(dtype)
    cu_h = [0]
    for n in lens:
        cu_h.append(cu_h[-1] + n)
    cu = torch.tensor(cu_h, dtype=torch.int32, device=dev)
    out, dqkv, lse = (t.cpu() for t in _window_run(dev, qkv.to(dev), go.to(dev), None, window, cu, max(lens)))
    assert lse.shape == (H, total)
    seqs = [(qkv[a:e], go[a:e], e - a, out[a:e], dqkv[a:e], lse[:, a:e]) for a, e in zip(cu_h[:-1], cu_h[1:]) if e > a]
    _check_sequences(dtype, window, seqs, one_key=(window == 0))


# ---------------------------------------------------------------------------------------------------- 2. add + LayerNorm
EPS = 1e-5
LN_EXTRA = {BF: ((768, 2), (1024, 2)), FP: ((768, 4), (1024, 4))}
LN_CASES = RMS_CASES + [RmsCase(dt, f, 3, ch) for dt in DTYPES for f, ch in LN_EXTRA[dt] if not any(c.dtype == dt and c.f == f for c in RMS_CASES)]


def ln_stat(f, dtype):
    """Relative error of a row sum of the LayerNorm kernels: the lanes add as the RMSNorm kernels do (module docstring, 2)."""
    return rms_stat(f, dtype)


def _ln_inputs(c, with_b):
    g = torch.Generator().manual_seed(c.rows * 11 + c.f + 100_000 * c.zero_row)
    a = (torch.randn(c.rows, c.f, generator=g) + 0.5).to(c.dtype)            # a mean that matters
    b = (0.5 * torch.randn(c.rows, c.f, generator=g)).to(c.dtype) if with_b else None
    if c.zero_row:
        a[1] = 0
        if with_b:
            b[1] = 0
    w = torch.empty(c.f).uniform_(0.5, 1.5, generator=g)
    gy, gs = (torch.randn(c.rows, c.f, generator=g).to(c.dtype) for _ in range(2))
    return a, b, w, gy, gs


@pytest.mark.parametrize("with_b", [True, False], ids=["add", "plain"])
@pytest.mark.parametrize("c", LN_CASES, ids=[c.id for c in LN_CASES])
def test_add_layernorm_matrix(dev, c, with_b):
    from gmlm_amd import ops
    a, b, w, gy, gs = _ln_inputs(c, with_b)
    ad, bd, wd_, gyd, gsd = (None if t is None else t.to(dev) for t in (a, b, w, gy, gs))

    def run():
        av, wv = ad.clone().requires_grad_(True), wd_.clone().requires_grad_(True)
        bv = bd.clone().requires_grad_(True) if with_b else None
        s, y = ops.add_layernorm(av, bv, wv, None, EPS)
        stats = y.grad_fn.saved_tensors[2].clone()
        torch.autograd.backward([s, y], [gsd, gyd])
        return s.detach(), y.detach(), av.grad, (bv.grad if with_b else av.grad), wv.grad, stats

    box = {}
    ran = kernels_run(lambda: box.setdefault("r", run()))
    tn = TN[c.dtype]
    want = {f"mbert::add_ln_{k}_kernel<{tn}, {c.ch}>" for k in ("fwd", "bwd")}
    assert _mbert(ran) == want, (sorted(_mbert(ran)), sorted(want))
    assert any(n.startswith(f"col_reduce_partial_kernel<1, gmlm::mbert::LnDwFn<{tn}, 1>") for n in ran), sorted(ran)
    assert not any(n.startswith(("ln_", "graphnorm_", "rmsnorm_")) for n in ran), sorted(ran)
    assert _same_bits(run(), box["r"])
    s, y, da, db, dw, stats = (t.cpu() for t in box["r"])
    assert stats.shape == (2, c.rows) and stats.dtype == torch.float32

    if with_b:
        _elem_check("s", s, a.double() + b.double(), 0.0)
    else:
        assert torch.equal(s, a)
    sd, wd = s.double(), w.double()
    st = ln_stat(c.f, c.dtype)
    mean = sd.mean(-1, keepdim=True)
    dev_ = sd - mean
    dev_mag = sd.abs().mean(-1, keepdim=True) * st + 2 * U * (sd.abs() + mean.abs())      # error of (s - mean): the mean's, and the subtraction
    rstd = (dev_.pow(2).mean(-1, keepdim=True) + EPS).rsqrt()
    xh = dev_ * rstd
    yr = xh * wd
    xh_err = rstd * dev_mag + xh.abs() * (st + 4 * U)                                      # |error of xhat|
    _elem_check("y", y, yr, xh_err * wd + yr.abs() * 4 * U)
    gr = gy.double() * wd
    m1, m2 = gr.mean(-1, keepdim=True), (gr * xh).mean(-1, keepdim=True)
    m1_abs, m2_abs = gr.abs().mean(-1, keepdim=True), (gr * xh).abs().mean(-1, keepdim=True)
    dsr = gs.double() + rstd * (gr - m1 - xh * m2)
    terms = gr.abs() + m1.abs() + (xh * m2).abs()
    extra = 4 * U * (gs.double().abs() + rstd * terms) + rstd * (st * m1_abs + xh.abs() * st * m2_abs + xh_err * (m2.abs() + m2_abs)) \
        + (st + 4 * U) * rstd * terms
    _elem_check("da", da, dsr, extra)
    assert torch.equal(da, db)
    if not (c.zero_row and c.rows == 1):
        _rel_l2("dgamma", dw, (gy.double() * xh).sum(0), c.dtype)
    for name, got, ref in (("mean", stats[0], mean[:, 0]), ("rstd", stats[1], rstd[:, 0])):
        err = float(((got.double() - ref).abs() / (ref.abs() + sd.abs().mean(-1) * (name == "mean") + 1e-300)).max())
        print(f"  {name}: rel err {err / U:.1f} u (bound {(st + 4 * U) / U:.1f} u)")
        assert err <= st + 4 * U, (name, err)
    if c.zero_row:
        assert float(s[1].abs().max()) == 0.0 and float(y[1].abs().max()) == 0.0
        assert float(stats[0, 1]) == 0.0
        want_r = float(torch.tensor(EPS, dtype=torch.float32).double().rsqrt())
        assert abs(float(stats[1, 1]) - want_r) / want_r <= 4 * U


def test_add_layernorm_with_beta_matches_torch(dev):
    """The nullable beta and its gradient (ModernBERT has none; the entry point takes one): against float64 layer_norm."""
    from gmlm_amd import ops
    g = torch.Generator().manual_seed(5)
    a, b = (torch.randn(9, 768, generator=g).to(dev) for _ in range(2))
    w, beta = torch.empty(768).uniform_(0.5, 1.5, generator=g).to(dev), torch.randn(768, generator=g).to(dev)
    gy = torch.randn(9, 768, generator=g).to(dev)
    av, bv, wv, be = (t.clone().requires_grad_(True) for t in (a, b, w, beta))
    box = {}
    ran = kernels_run(lambda: box.setdefault("r", ops.add_layernorm(av, bv, wv, be, EPS)))
    s, y = box["r"]
    y.backward(gy)
    assert "mbert::add_ln_fwd_kernel<float, 4>" in ran
    ad, bd, wd, bed = (t.detach().double().cpu().requires_grad_(True) for t in (a, b, w, beta))
    yr = torch.nn.functional.layer_norm(ad + bd, (768,), wd, bed, EPS)
    yr.backward(gy.double().cpu())
    for name, got, ref in (("y", y, yr), ("da", av.grad, ad.grad), ("db", bv.grad, bd.grad), ("dgamma", wv.grad, wd.grad),
                           ("dbeta", be.grad, bed.grad)):
        _rel_l2(name, got.detach().cpu(), ref.detach(), FP)


# -------------------------------------------------------------------------------------------------- 3. rotary embedding
def _table32(rows, theta, dev):
    inv = 1.0 / (theta ** (torch.arange(0, D, 2, dtype=torch.float) / D))
    fr = torch.arange(rows, dtype=torch.float32)[:, None] * inv[None]
    return torch.stack([fr.cos(), fr.sin()], 1).contiguous().to(dev)


def _rot64(x, cos, sin):
    lo, hi = x[..., :32], x[..., 32:]
    return torch.cat([lo * cos - hi * sin, hi * cos + lo * sin], -1)


def _rot64_mag(x, cos, sin):
    lo, hi = x[..., :32].abs(), x[..., 32:].abs()
    return torch.cat([lo * cos.abs() + hi * sin.abs(), hi * cos.abs() + lo * sin.abs()], -1)


ROPE_CASES = [                                 # (id, lead, heads, table rows, positions or None, position modulus)
    ("b1_l1", (1, 1), 1, 2, None, 0),          # 2 head rows: the other lane groups of the one block dead
    ("b2_l3", (2, 3), 3, 3, None, 0),
    ("b3_l1", (3, 1), 2, 4, None, 0),          # seq_len = 1: every token at position 0
    ("pos_len1", (3,), 2, 1, (-2, 0, 7), 0),   # a table of ONE row: all three clamp to row 0
    ("tail", (1367,), 2, 300, None, 300),      # 5468 head rows: 171 (bf16) / 342 (fp32) blocks, the last one partly live
]


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp32"])
@pytest.mark.parametrize("case", ROPE_CASES, ids=[c[0] for c in ROPE_CASES])
def test_rope64_matrix(dev, case, dtype):
    from gmlm_amd import ops
    name, lead, h, rows, positions, mod = case
    g = torch.Generator().manual_seed(zlib.crc32(name.encode()))
    tok, wid = math.prod(lead), 3 * h * D
    x = torch.randn(*lead, wid, generator=g).to(dtype)
    cs = _table32(rows, 1e4, dev)
    by_pos = len(lead) == 1
    if by_pos:
        pos = torch.tensor(positions) if positions else torch.arange(tok) % mod
        read, pos_d, seq_len = pos.clamp(0, rows - 1), pos.to(dev, torch.int32), 0
    else:
        read, pos_d, seq_len = torch.arange(tok) % lead[1], None, lead[1]

    def run(inverse):
        buf = x.to(dev).clone()
        ops.rope64_(buf, cs, h, seq_len, pos_d, inverse=inverse)
        return buf

    box = {}
    ran = kernels_run(lambda: box.setdefault("f", run(False)))
    assert _mbert(ran) == {f"mbert::rope64_kernel<{TN[dtype]}, false>"}, sorted(ran)
    ran = kernels_run(lambda: box.setdefault("b", run(True)))
    assert _mbert(ran) == {f"mbert::rope64_kernel<{TN[dtype]}, true>"}, sorted(ran)
    assert _same_bits((run(False), run(True)), (box["f"], box["b"]))
    fwd, bwd = box["f"].cpu().view(tok, 3 * h, D), box["b"].cpu().view(tok, 3 * h, D)
    xd = x.double().view(tok, 3 * h, D)
    cos, sin = cs.cpu()[read, 0].double()[:, None, :], cs.cpu()[read, 1].double()[:, None, :]
    assert torch.equal(fwd[:, 2 * h:], x.view(tok, 3 * h, D)[:, 2 * h:]) and torch.equal(bwd[:, 2 * h:], fwd[:, 2 * h:])   # V untouched
    _elem_check("forward", fwd[:, :2 * h], _rot64(xd[:, :2 * h], cos, sin), _rot64_mag(xd[:, :2 * h], cos, sin) * 3 * U)
    _elem_check("inverse", bwd[:, :2 * h], _rot64(xd[:, :2 * h], cos, -sin), _rot64_mag(xd[:, :2 * h], cos, sin) * 3 * U)
    # forward, then backward on the SAME buffer: the input to rounding
    buf = x.to(dev).clone()
    ops.rope64_(buf, cs, h, seq_len, pos_d)
    mid = buf.clone()
    ops.rope64_(buf, cs, h, seq_len, pos_d, inverse=True)
    back = buf.cpu().view(tok, 3 * h, D)[:, :2 * h]
    mag = _rot64_mag(_rot64_mag(xd[:, :2 * h], cos, sin), cos, sin)
    ulp = 2.0 ** -8 if dtype == BF else 2.0 ** -24
    err = (back.double() - xd[:, :2 * h]).abs() / (mag * (2 * ulp + 8 * U) + 1e-300)
    print(f"  round trip: max err / bound = {float(err.max()):.3f}")
    assert float(err.max()) <= 1.0 and bool(torch.isfinite(mid).all())


# ----------------------------------------------------------------------------------------------------------------- 4. GeGLU
def _gelu_ref(g):
    cdf = 0.5 * (1 + torch.erf(g / math.sqrt(2)))
    return g * cdf, cdf + g * torch.exp(-0.5 * g * g) / math.sqrt(2 * math.pi)


GEGLU_CASES = [c for c in SWIGLU_CASES if not c.saturated]


@pytest.mark.parametrize("c", GEGLU_CASES, ids=[c.id for c in GEGLU_CASES])
def test_geglu_matrix(dev, c):
    from gmlm_amd import ops
    u, gy = swiglu_inputs(c, dev)
    inter = c.inter

    def run():
        v = u.clone().requires_grad_(True)
        y = ops.geglu(v)
        y.backward(gy)
        return y.detach(), v.grad

    box = {}
    ran = kernels_run(lambda: box.setdefault("r", run()))
    assert _mbert(ran) == {f"mbert::geglu_{k}_kernel<{TN[c.dtype]}>" for k in ("fwd", "bwd")}, sorted(ran)
    assert not any(n.startswith(("swiglu_", "bias_gelu_")) for n in ran), sorted(ran)
    assert _same_bits(run(), box["r"])
    y, du = box["r"]
    assert y.shape == (c.rows, inter) and du.shape == u.shape
    erf_abs = 8 * U + (1.5e-7 if c.dtype == BF else 0.0)           # error of erf: 4 ulp of erff at <= 1 (fp32) / the polynomial's (bf16)
    slab = 256
    for r0 in range(0, c.rows, slab):
        r1 = min(c.rows, r0 + slab)
        gt, up, d = u[r0:r1, :inter].double(), u[r0:r1, inter:].double(), gy[r0:r1].double()
        act, grad = _gelu_ref(gt)
        act_err = 0.5 * gt.abs() * erf_abs + 8 * U * act.abs()
        grad_err = 0.5 * erf_abs + 8 * U * grad.abs() + gt.abs() * torch.exp(-0.5 * gt * gt) * 0.4 * 8 * U
        tag = f" rows {r0}..{r1 - 1}" if c.rows > slab else ""
        _elem_check("y" + tag, y[r0:r1], act * up, act_err * up.abs() + 4 * U * (act * up).abs())
        _elem_check("d up" + tag, du[r0:r1, inter:], d * act, act_err * d.abs() + 4 * U * (d * act).abs())
        _elem_check("d gate" + tag, du[r0:r1, :inter], d * up * grad, grad_err * (d * up).abs() + 6 * U * (d * up * grad).abs())


def test_nothing_to_do_through_the_operators(dev):
    from gmlm_amd import ops
    for dtype in DTYPES:
        z = torch.zeros(0, 768, device=dev, dtype=dtype, requires_grad=True)
        w = torch.ones(768, device=dev, requires_grad=True)
        s, y = ops.add_layernorm(z, None, w, None, EPS)
        y.sum().backward()
        assert y.shape == (0, 768) and float(w.grad.abs().max()) == 0.0
        assert ops.geglu(torch.zeros(0, 16, device=dev, dtype=dtype)).shape == (0, 8)
        buf = torch.zeros(0, 3 * HD, device=dev, dtype=dtype)
        ops.rope64_(buf, _table32(4, 1e4, dev), H, 0, torch.zeros(0, dtype=torch.int32, device=dev))
        out, _, lse = ops._window_fwd(torch.zeros(2, 0, 3 * HD, device=dev, dtype=dtype), None, H, SCALE, 4, None, 0, False)
        assert out.shape == (2, 0, HD)
