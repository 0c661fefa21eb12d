"""The soft-capped grouped-KV attention kernels at head dim 256 (gmlm_attention_gqa_d256_softcap_*, csrc/attn_gqa_softcap.hip,
namespace gqac::) through ``ops.gqa_d256_softcap_attention`` / ``_varlen`` on slices of a fused buffer, against dense float64
attention on the same rounded inputs, forward and backward; and the rotary embedding on head rows at head dim 256
(``ops.rope_heads_d256_``) with the node that joins the two (``ops.rope_softcap_gqa_d256`` / ``_varlen``).

The scores enter the softmax as z = c tanh(q.k scale / c), capped BEFORE the mask
visible(i, j) = j < kv_len and (window == 0 or (0 <= i - j < w if causal else |i - j| < w)) and (not causal or j <= i).

The checker is tests/test_gqa_softcap_cpu.softcap_reference, which that file ties to transformers' own eager_attention_forward
of modeling_gemma2 to 1e-12.  The input builders and the budgets are those of tests/test_gpu_gqa_band_kernels.py, imported
unchanged (same head dim, same rounding points; a tanh whose error is relative to |z| adds nothing above them): fp32 1e-4 max /
1e-5 relative L2; bf16 2e-2 max, 6e-3 relative L2 for out and dv, 8e-3 for dq and dk; lse as there.  Every case prints the
measured value beside its budget.  Scale 1 / 12 and K scaled 1.5 as there: scores reach +-7.5.

Cases.  Heads (3, 1) and (4, 2); fp32 and bf16; causal and bidirectional; caps 50 (Gemma2's), 4 and 1; windows 0 (no band), 2,
33 and 100; lengths 1, 33, 65 and 129; kv_len = L, 1, 0 and L // 2; packed: the four lengths and an empty sequence in one call,
max_len exact and larger, equal to the padded pass bit for bit.

Not vacuous: at caps <= 4 and kv_len = L >= 65 the float64 capped and uncapped outputs differ by >= 0.1 in relative L2 (a
condition on the inputs, asserted).  At c = 50 the difference is 4e-3 to 8e-3: above the fp32 budget, below the bf16 one, so the bf16
cases at 50 prove only that the cap does no harm.

Every test here calls an operator that the tree before this kernel family does not have."""
import math

import pytest
import torch

import test_gpu_gqa_wide_kernels as GW
from helpers import kernels_run
from test_gpu_attention_wide import _budget
from test_gpu_gqa_band_kernels import _assert_blind_rows, _bits, _bound, _pad_batch, _rel_l2, _same, _unpad
from test_gpu_gqa_wide_kernels import D, PAD, SCALE, TN, _check, _flat, _fused, _slices
from test_gqa_softcap_cpu import softcap_reference, visible

pytestmark = pytest.mark.gpu

HEADS = ((3, 1), (4, 2))
CAPS = (50.0, 4.0, 1.0)
WINDOWS = (0, 2, 33, 100)
LENS = (1, 33, 65, 129)
DTYPES = (torch.float32, torch.bfloat16)
NEG = float("-inf")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _kernel_sets(dtype, causal, band):
    t, c, b = TN[dtype], "true" if causal else "false", "true" if band else "false"
    return ({f"gqac::fwd_kernel<{t}, {c}, {b}>"},
            {f"gqac::delta_kernel<{t}>", f"gqac::dq_kernel<{t}, {c}, {b}>", f"gqac::dkv_kernel<{t}, {c}, {b}>"})


def _run(buf, go, hq, hkv, causal, cap, window, kv_len=None, cu=None, max_len=0, kernels=False):
    """Through the operator on slices of the fused buffer -> out, lse, dq, dk, dv (the gradients as slices of buf.grad)."""
    from gmlm_amd import ops
    leaf = buf.clone().requires_grad_(True)
    q, k, v = _slices(leaf, hq, hkv)
    assert q.stride(-2) == (hq + 2 * hkv) * D + PAD
    if cu is None:
        fwd = lambda: ops.gqa_d256_softcap_attention(q, k, v, kv_len, hq, hkv, SCALE, causal, cap, window)
    else:
        fwd = lambda: ops.gqa_d256_softcap_attention_varlen(q, k, v, cu, max_len, hq, hkv, SCALE, causal, cap, window)
    if kernels:
        box = {}
        fwd_k = kernels_run(lambda: box.setdefault("o", fwd()))
        out = box["o"]
        lse = out.grad_fn.saved_tensors[4]                            # before the backward frees what the node saved
        bwd_k = kernels_run(lambda: out.backward(go))
        assert (fwd_k, bwd_k) == _kernel_sets(buf.dtype, causal, window > 0), (sorted(fwd_k), sorted(bwd_k))   # no gqaw:: / gqab:: kernel
    else:
        out = fwd()
        lse = out.grad_fn.saved_tensors[4]
        out.backward(go)
    assert float(leaf.grad[..., (hq + 2 * hkv) * D:].abs().max()) == 0.0           # the padding columns get no gradient
    return (out.detach(), lse) + tuple(t.clone() for t in _slices(leaf.grad, hq, hkv))


def _check_lse(tag, dtype, got_lse, ref_lse):
    seen = torch.isfinite(ref_lse)
    lerr = float((got_lse.double() - ref_lse)[seen].abs().max()) / float(ref_lse[seen].abs().max()) if bool(seen.any()) else 0.0
    print(f"  lse: max|err| / max|ref| = {lerr:.2e} (budget {_budget(dtype, False)[0]:.0e})")
    assert lerr <= _budget(dtype, False)[0], tag


@pytest.mark.parametrize("dtype", DTYPES, ids=("fp32", "bf16"))
@pytest.mark.parametrize("causal", [False, True], ids=("bidir", "causal"))
@pytest.mark.parametrize("hq,hkv", HEADS)
def test_padded_caps_windows_lengths_and_kv_len_vs_dense_fp64(dev, hq, hkv, causal, dtype):
    """Per cap, window and length L: four sequences with kv_len L, 1, 0 and L // 2."""
    blind_total = 0
    for L in LENS:
        buf, go = _fused(dev, dtype, (4, L), hq, hkv, 100 * L + hq + hkv)
        kv = torch.tensor([L, 1, 0, L // 2], device=dev)
        kv_len = kv.to(torch.int32)
        q, k, v = _slices(buf, hq, hkv)
        for w in WINDOWS:
            plain = softcap_reference(q, k, v, go, kv, hq, hkv, SCALE, causal, None, w)[0]
            for cap in CAPS:
                tag = f"padded L={L} c={cap} w={w} {hq}/{hkv} causal={causal} {dtype}"
                got = _run(buf, go, hq, hkv, causal, cap, w, kv_len=kv_len, kernels=(L, cap, w) in ((129, 50.0, 0), (129, 4.0, 33)))
                ref = softcap_reference(q, k, v, go, kv, hq, hkv, SCALE, causal, cap, w)
                _check(tag, dtype, [None if i == 1 else _flat(t) for i, t in enumerate(got)], [_flat(t) for t in ref[:4]], _bound(q, k, v, go))
                blind_total += _assert_blind_rows(tag, got, kv, w if w else 1 << 29, causal, L)
                _check_lse(tag, dtype, got[1], ref[4])
                # the cap must matter: a condition on the case, not a measurement.  Not asked of window 2, where a row has two or
                # three keys (float64: 0.04 at c = 4); at windows 0, 33 and 100 the smallest over these cases is 0.37 (c = 4), 0.72 (c = 1)
                if cap <= 4 and L >= 65 and w != 2:
                    differs = _rel_l2(ref[0][0], plain[0])
                    print(f"  float64 capped vs uncapped out, kv_len = L: rel l2 = {differs:.2f} (must be >= 0.1)")
                    assert differs >= 0.1, tag
    assert blind_total > 0


@pytest.mark.parametrize("dtype", DTYPES, ids=("fp32", "bf16"))
@pytest.mark.parametrize("causal", [False, True], ids=("bidir", "causal"))
@pytest.mark.parametrize("hq,hkv", HEADS)
def test_packed_vs_dense_fp64_and_vs_the_padded_pass(dev, hq, hkv, causal, dtype):
    """The four lengths and an empty sequence back to back in one packed call per cap and window, max_len exact (129); max_len
    larger (200) gives the same bytes; each sequence alone in the padded layout gives the same bytes, so the packed pass meets
    the padded pass's budgets."""
    lens = [1, 33, 0, 65, 129]
    cu_l = [0] + torch.tensor(lens).cumsum(0).tolist()
    cu = torch.tensor(cu_l, dtype=torch.int32, device=dev)
    total = sum(lens)
    buf, go = _fused(dev, dtype, (total,), hq, hkv, 31 + hq + hkv)
    q, k, v = _slices(buf, hq, hkv)
    width = max(lens)
    qb, kb, vb, gb = (_pad_batch(t, cu_l, width) for t in (q, k, v, go))
    kv = torch.tensor(lens, device=dev)
    for w in WINDOWS:
        for cap in CAPS:
            tag = f"packed c={cap} w={w} {hq}/{hkv} causal={causal} {dtype}"
            got = _run(buf, go, hq, hkv, causal, cap, w, cu=cu, max_len=width, kernels=(cap, w) in ((50.0, 0), (4.0, 33)))
            ref_b = softcap_reference(qb, kb, vb, gb, kv, hq, hkv, SCALE, causal, cap, w)
            _check(tag, dtype, got, [_unpad(t, cu_l) for t in ref_b[:4]], _bound(q, k, v, go))
            assert tuple(got[1].shape) == (hq, total) and bool(torch.isfinite(got[1]).all())       # every row sees itself
            _same(tag + " max_len 200", got, _run(buf, go, hq, hkv, causal, cap, w, cu=cu, max_len=200))
            for i, n in enumerate(lens):
                if n == 0:
                    continue
                r0 = cu_l[i]
                one = _run(buf[r0:r0 + n][None], go[r0:r0 + n][None], hq, hkv, causal, cap, w)
                _same(f"{tag} sequence of {n} padded", (got[0][r0:r0 + n], got[1][:, r0:r0 + n], got[2][r0:r0 + n], got[3][r0:r0 + n],
                                                        got[4][r0:r0 + n]), tuple(t[0] for t in one))


def _spiked(buf, hq, hkv, i, j, sign):
    """Head 0 of query i all 20, KV head 0 of key j all +-24: q.k * scale = +-256 * 480 / 12 = +-10,240 (exact in bf16)."""
    out = buf.clone()
    out[0, i, :D] = 20.0
    out[0, j, hq * D:hq * D + D] = 24.0 * sign
    return out


@pytest.mark.parametrize("dtype", DTYPES, ids=("fp32", "bf16"))
@pytest.mark.parametrize("cap", CAPS)
def test_a_spiked_score_saturates_to_exactly_the_cap(dev, cap, dtype):
    """One (query, key) pair with q.k * scale = +-10,240, i.e. |x| = |s| scale / c >= 204: tanh is 1 in every precision.
    Everything finite and within budget against float64.  That z is exactly +-c is not read off directly (no output is z) but
    shown by two weaker observations that together leave no room for another value: (a) query 0 of a causal sequence sees
    key 0 alone, so its lse is z passed through log2 e and ln 2, (c log2 e) ln 2 in fp32, asserted within 2 ulp of c, not bit
    for bit; (b) a spike twice as large (on that query, which has no other key) gives the same bytes everywhere, which an
    unsaturated z would not.  The dS factor of the pair is exactly 0: dq of that query, which has no other key, is exactly 0
    (without the cap it is rounding noise of P (dP - delta))."""
    hq, hkv, L = 3, 1, 65
    base, go = _fused(dev, dtype, (1, L), hq, hkv, 17)
    kv_len = torch.tensor([L], dtype=torch.int32, device=dev)
    for sign in (1.0, -1.0):
        for i, j in ((0, 0), (40, 7)):
            buf = _spiked(base, hq, hkv, i, j, sign)
            q, k, v = _slices(buf, hq, hkv)
            assert abs(float(q[0, i, :D].double() @ k[0, j].double()) * SCALE) == 10240.0
            tag = f"spike {sign:+.0f} ({i}, {j}) c={cap} {dtype}"
            got = _run(buf, go, hq, hkv, True, cap, 0, kv_len=kv_len)
            ref = softcap_reference(q, k, v, go, kv_len.long(), hq, hkv, SCALE, True, cap)
            for t in got:
                assert bool(torch.isfinite(t).all()), tag
            _check(tag, dtype, [None if n == 1 else _flat(t) for n, t in enumerate(got)], [_flat(t) for t in ref[:4]], _bound(q, k, v, go))
            _check_lse(tag, dtype, got[1], ref[4])
            if (i, j) == (0, 0):
                twice = buf.clone()
                twice[0, i, :D] = 40.0                                                    # q.k * scale = +-20,480; query 0 has no other key
                _same(tag + " twice the spike", got, _run(twice, go, hq, hkv, True, cap, 0, kv_len=kv_len))
                z = float(got[1][0, 0, 0])
                print(f"  lse of the one-key row = {z!r} (z = {sign * cap})")
                assert abs(z - sign * cap) <= 2 * cap * 2.0 ** -23, tag
                assert float(got[2][0, 0, :D].abs().max()) == 0.0, tag                  # dS = P (dP - delta) * 0


@pytest.mark.parametrize("dtype", DTYPES, ids=("fp32", "bf16"))
@pytest.mark.parametrize("cap", (50.0, 1.0))
def test_a_spiked_score_on_a_masked_key_has_probability_exactly_zero(dev, cap, dtype):
    """The same spike (+10,240: after the cap the largest score of its row) on a key (a) at or past kv_len, (b) above the
    causal diagonal, (c) outside the band.  The queries that do not see the key give the bytes of the run with that key's row of
    K zeroed: out, lse and dq (for (a), where no query sees it, dk and dv too): the spiked row of K reaches nothing.  That
    comparison alone would not catch a cap applied AFTER the mask (both runs would turn the key's -inf into -c and agree), so
    the spiked run is also held to float64, outputs, gradients and lse, within the budgets: there the masked key has probability
    0, and with a misplaced cap it would have that of a score of -c."""
    hq, hkv, L = 3, 1, 65
    base, go = _fused(dev, dtype, (1, L), hq, hkv, 23)
    for name, causal, w, kvl, i, j in (("past kv_len", False, 0, 40, 5, 50), ("at kv_len", True, 0, 40, 45, 40),
                                       ("above the diagonal", True, 0, L, 20, 21), ("outside the band", False, 4, L, 20, 24),
                                       ("outside the causal band", True, 33, L, 64, 31)):
        buf = _spiked(base, hq, hkv, i, j, 1.0)
        zeroed = buf.clone()
        zeroed[0, j, hq * D:(hq + hkv) * D] = 0.0
        kv_len = torch.tensor([kvl], dtype=torch.int32, device=dev)
        sees = visible(L, kvl, w, causal, dev)[:, j]                        # the queries that see key j
        assert not bool(sees[i])
        a = _run(buf, go, hq, hkv, causal, cap, w, kv_len=kv_len)
        b = _run(zeroed, go, hq, hkv, causal, cap, w, kv_len=kv_len)
        rows = ~sees
        tag = f"{name} c={cap} {dtype}"
        _same(tag, (a[0][0, rows], a[1][0][:, rows], a[2][0, rows]), (b[0][0, rows], b[1][0][:, rows], b[2][0, rows]))   # out, lse, dq
        q, k, v = _slices(buf, hq, hkv)
        ref = softcap_reference(q, k, v, go, kv_len.long(), hq, hkv, SCALE, causal, cap, w)
        _check(tag, dtype, [None if n == 1 else _flat(t) for n, t in enumerate(a)], [_flat(t) for t in ref[:4]], _bound(q, k, v, go))
        _check_lse(tag, dtype, a[1], ref[4])
        if not bool(sees.any()):
            _same(tag + " (every gradient)", a, b)
            assert float(a[3][0, j].abs().max()) == 0.0 and float(a[4][0, j].abs().max()) == 0.0


@pytest.mark.parametrize("dtype", DTYPES, ids=("fp32", "bf16"))
@pytest.mark.parametrize("causal", [False, True], ids=("bidir", "causal"))
def test_a_huge_cap_is_the_uncapped_family(dev, causal, dtype):
    """c = 1e6: z = c tanh(s / c) = s (1 - (s / c)^2 / 3 ...), 2e-11 relative at |s| = 7.5, below fp32 rounding; the fp32 outputs
    agree with ``ops.gqa_d256_attention`` to the fp32 budget.  In bf16 a score that differs in its last fp32 bit can flip the
    rounding of a stored element, one bf16 ulp, so there the budget is the bf16 one."""
    hq, hkv = 4, 2
    for L in (33, 129):
        buf, go = _fused(dev, dtype, (3, L), hq, hkv, 60 + L)
        kv_len = torch.tensor([L, 1, L // 2], dtype=torch.int32, device=dev)
        plain = GW._run(buf, go, hq, hkv, causal, kv_len=kv_len)
        got = _run(buf, go, hq, hkv, causal, 1e6, 0, kv_len=kv_len)
        q, k, v = _slices(buf, hq, hkv)
        _check(f"huge cap L={L} causal={causal} {dtype}", dtype, [None if i == 1 else _flat(t) for i, t in enumerate(got)],
               [_flat(plain[i]).double() for i in (0, 2, 3, 4)], _bound(q, k, v, go))
        seen = torch.isfinite(plain[1])
        assert float((got[1] - plain[1])[seen].abs().max()) <= 1e-4 * float(plain[1][seen].abs().max())


@pytest.mark.parametrize("dtype", DTYPES, ids=("fp32", "bf16"))
@pytest.mark.parametrize("causal", [False, True], ids=("bidir", "causal"))
def test_repeated_call_gives_identical_bytes(dev, causal, dtype):
    hq, hkv, L = 4, 2, 129
    buf, go = _fused(dev, dtype, (3, L), hq, hkv, 11)
    kv_len = torch.tensor([L, 40, 97], dtype=torch.int32, device=dev)
    for cap, w in ((50.0, 0), (4.0, 33), (1.0, 2)):
        _same(f"c={cap} w={w}", _run(buf, go, hq, hkv, causal, cap, w, kv_len=kv_len), _run(buf, go, hq, hkv, causal, cap, w, kv_len=kv_len))


@pytest.mark.parametrize("dtype", DTYPES, ids=("fp32", "bf16"))
@pytest.mark.parametrize("cap", (50.0, 1.0))
def test_rows_that_see_nothing_at_129_33_40(dev, cap, dtype):
    """L = 129, w = 33, kv_len = 40, causal, with a cap: the 57 queries from row 72 = kv_len + w - 1 on see no key: zeros,
    lse = -inf, dq = 0, nothing in dk / dv (the key gradients of the first 72 rows alone, bit for bit)."""
    hq, hkv, L, w = 3, 1, 129, 33
    buf, go = _fused(dev, dtype, (2, L), hq, hkv, 4)
    kv = torch.tensor([40, 129], device=dev)
    blind = ~visible(L, kv, w, True, dev).any(-1)
    assert int(blind[0].sum()) == 57 and int(blind[0].nonzero()[0]) == 72 and int(blind[1].sum()) == 0
    got = _run(buf, go, hq, hkv, True, cap, w, kv_len=kv.to(torch.int32))
    assert _assert_blind_rows("129/33/40", got, kv, w, True, L) == 57
    q, k, v = _slices(buf, hq, hkv)
    ref = softcap_reference(q, k, v, go, kv, hq, hkv, SCALE, True, cap, w)
    _check(f"129/33/40 c={cap} {dtype}", dtype, [None if i == 1 else _flat(t) for i, t in enumerate(got)], [_flat(t) for t in ref[:4]], 0.0)
    cut = _run(buf[:1, :72].contiguous(), go[:1, :72].contiguous(), hq, hkv, True, cap, w, kv_len=kv[:1].to(torch.int32))
    assert torch.equal(_bits(got[3][0, :72]), _bits(cut[3][0])) and torch.equal(_bits(got[4][0, :72]), _bits(cut[4][0]))


def test_nothing_to_do_and_refused_arguments(dev):
    from gmlm_amd import _lib, ops
    hq, hkv = 3, 1
    for shape in ((0, 5), (2, 0)):
        q = torch.zeros(*shape, hq * D, device=dev, requires_grad=True)
        k, v = (torch.zeros(*shape, hkv * D, device=dev, requires_grad=True) for _ in range(2))
        out = ops.gqa_d256_softcap_attention(q, k, v, None, hq, hkv, SCALE, True, 50.0, 4)
        out.sum().backward()
        assert tuple(out.shape) == (*shape, hq * D) and tuple(k.grad.shape) == tuple(k.shape)
    q = torch.zeros(1, 8, hq * D, device=dev)
    k, v = (torch.zeros(1, 8, hkv * D, device=dev) for _ in range(2))
    lib = _lib.lib()
    out, lse = torch.zeros(1, 8, hq * D, device=dev), torch.zeros(1, hq, 8, device=dev)

    def calls():
        for w, c, word in ((-1, 50.0, b": window"), (1 << 30, 50.0, b": window"), (0, 0.0, b": softcap"), (4, -1.0, b": softcap"),
                           (0, math.inf, b": softcap"), (0, math.nan, b": softcap")):
            rc = lib.gmlm_attention_gqa_d256_softcap_fwd(q.data_ptr(), k.data_ptr(), v.data_ptr(), None, 1, hq, hkv, 8, 8, D, hq * D, hkv * D,
                                                         hkv * D, SCALE, 0.0, 1, w, c, out.data_ptr(), None, lse.data_ptr(), _lib.F32, None)
            assert rc == -1 and word in lib.gmlm_last_error(), (w, c, lib.gmlm_last_error())
        torch.zeros(4, device=dev).add_(1)

    assert kernels_run(calls) == set()


# ---- the rotary embedding on head rows at d = 256 ---------------------------------------------------------------------
def _table(n, dev):
    """fp32 [n, 2, 128] of the default rotary frequencies (base 10,000)"""
    inv = 1.0 / (10000.0 ** (torch.arange(0, D, 2, dtype=torch.float32) / D))
    f = torch.arange(n, dtype=torch.float32)[:, None] * inv[None, :]
    return torch.stack([f.cos(), f.sin()], 1).contiguous().to(dev)


def _rotate_fp64(rows, cs, pos, heads):
    """rows [T, >= heads * D], pos [T]: float64 rotate-half of the first ``heads`` head rows; the rest unchanged"""
    out = rows.double().clone()
    x = out[:, :heads * D].reshape(-1, heads, D)
    c, s = cs[pos, 0].double()[:, None, :], cs[pos, 1].double()[:, None, :]
    x1, x2 = x[..., :D // 2], x[..., D // 2:]
    out[:, :heads * D] = torch.cat([x1 * c - x2 * s, x2 * c + x1 * s], -1).reshape(-1, heads * D)
    return out


@pytest.mark.parametrize("dtype", DTYPES, ids=("fp32", "bf16"))
@pytest.mark.parametrize("hq,hkv", HEADS)
def test_rope_heads_d256_in_place_vs_float64(dev, hq, hkv, dtype):
    """Padded [3, 37, .] (positions row % 37) and packed rows with pos_ids, on the fused buffer with V and 8 padding columns:
    one rounding of the float64 rotate-half: a product and a fused multiply-add in fp32 and the store, three roundings of
    eps / 2 each at most, bound 2 eps max|result| (eps = 2^-7 in bf16, 2^-23 in fp32); V and padding bit for bit; forward then
    inverse gives the input back to one rounding each way (the inverse turns the first error by the same angle and adds its own:
    2 eps max|x|); the kernels are the gqac:: rotary ones."""
    from gmlm_amd import ops
    heads, eps = hq + hkv, torch.finfo(dtype).eps
    cs = _table(64, dev)
    buf, _ = _fused(dev, dtype, (3, 37), hq, hkv, 3)
    lens = [1, 33, 0, 40]
    pos = torch.cat([torch.arange(n) for n in lens]).to(dev, torch.int32)
    pbuf, _ = _fused(dev, dtype, (sum(lens),), hq, hkv, 4)
    for name, rows, kw, p in (("padded", buf, dict(seq_len=37), torch.arange(3 * 37, device=dev) % 37),
                              ("packed", pbuf, dict(seq_len=0, pos_ids=pos), pos.long())):
        work = rows.clone()
        names = kernels_run(lambda: ops.rope_heads_d256_(work, cs, heads, **kw))
        assert names == {f"gqac::rope_heads_d256_kernel<{TN[dtype]}, false>"}, names
        ref = _rotate_fp64(_flat(rows), cs, p, heads)
        err = float((_flat(work).double() - ref).abs().max())
        bound = 2 * eps * float(ref.abs().max())
        print(f"  {name} {dtype}: max|err| = {err:.2e} (bound {bound:.2e})")
        assert err <= bound
        assert torch.equal(_bits(work[..., heads * D:]), _bits(rows[..., heads * D:]))          # V and the padding columns
        names = kernels_run(lambda: ops.rope_heads_d256_(work, cs, heads, inverse=True, **kw))
        assert names == {f"gqac::rope_heads_d256_kernel<{TN[dtype]}, true>"}, names
        back = float((work.double() - rows.double()).abs().max())
        print(f"  {name} {dtype}: forward then inverse max|x' - x| = {back:.2e} (bound {2 * eps * float(rows.double().abs().max()):.2e})")
        assert back <= 2 * eps * float(rows.double().abs().max())
        assert torch.equal(_bits(work[..., heads * D:]), _bits(rows[..., heads * D:]))


@pytest.mark.parametrize("dtype", DTYPES, ids=("fp32", "bf16"))
@pytest.mark.parametrize("packed", [False, True], ids=("padded", "packed"))
@pytest.mark.parametrize("cap,window", [(50.0, 0), (4.0, 33), (None, 0), (None, 33)], ids=("cap50", "cap4-w33", "nocap", "nocap-w33"))
def test_the_fused_node_is_rope_then_attention_then_inverse_rope(dev, cap, window, packed, dtype):
    """``ops.rope_softcap_gqa_d256`` / ``_varlen`` against the three steps on views of one buffer, bit for bit, output and dqkv;
    and the kernels it launches: the gqac:: rotary pair around gqac:: attention (capped) or gqaw:: / gqab:: (``softcap`` None)."""
    from gmlm_amd import ops
    hq, hkv = 4, 2
    heads, W = hq + hkv, (hq + 2 * hkv) * D
    cs = _table(256, dev)
    if packed:
        lens = [1, 33, 0, 65]
        cu = torch.tensor([0] + torch.tensor(lens).cumsum(0).tolist(), dtype=torch.int32, device=dev)
        pos = torch.cat([torch.arange(n) for n in lens]).to(dev, torch.int32)
        buf, go = _fused(dev, dtype, (sum(lens),), hq, hkv, 8)
        rope_kw, kv_len = dict(seq_len=0, pos_ids=pos), None
    else:
        buf, go = _fused(dev, dtype, (2, 65), hq, hkv, 9)
        kv_len = torch.tensor([65, 30], dtype=torch.int32, device=dev)
        rope_kw = dict(seq_len=65)
    qkv = buf[..., :W].contiguous().requires_grad_(True)
    if packed:
        fused = lambda: ops.rope_softcap_gqa_d256_varlen(qkv, cs, pos, cu, 65, hq, hkv, SCALE, True, cap, window=window)
    else:
        fused = lambda: ops.rope_softcap_gqa_d256(qkv, cs, kv_len, hq, hkv, SCALE, True, cap, window=window)
    box = {}
    fwd_k = kernels_run(lambda: box.setdefault("o", fused()))
    out = box["o"]
    bwd_k = kernels_run(lambda: out.backward(go))
    t = TN[dtype]
    fam = "gqac" if cap is not None else ("gqab" if window else "gqaw")
    targs = f"{t}, true" + (f", {'true' if window else 'false'}" if cap is not None else "")
    assert fwd_k == {f"gqac::rope_heads_d256_kernel<{t}, false>", f"{fam}::fwd_kernel<{targs}>"}, sorted(fwd_k)
    assert bwd_k == {f"gqac::rope_heads_d256_kernel<{t}, true>", f"{fam}::delta_kernel<{t}>", f"{fam}::dq_kernel<{targs}>",
                     f"{fam}::dkv_kernel<{targs}>"}, sorted(bwd_k)
    # the three steps by hand
    leaf = ops.rope_heads_d256_(buf[..., :W].contiguous(), cs, heads, **rope_kw).requires_grad_(True)
    q, k, v = _slices(leaf, hq, hkv)
    if cap is not None:
        step = (ops.gqa_d256_softcap_attention_varlen(q, k, v, cu, 65, hq, hkv, SCALE, True, cap, window) if packed else
                ops.gqa_d256_softcap_attention(q, k, v, kv_len, hq, hkv, SCALE, True, cap, window))
    elif window:
        step = (ops.gqa_d256_band_attention_varlen(q, k, v, cu, 65, hq, hkv, SCALE, True, window) if packed else
                ops.gqa_d256_band_attention(q, k, v, kv_len, hq, hkv, SCALE, True, window))
    else:
        step = (ops.gqa_d256_attention_varlen(q, k, v, cu, 65, hq, hkv, SCALE, True) if packed else
                ops.gqa_d256_attention(q, k, v, kv_len, hq, hkv, SCALE, True))
    step.backward(go)
    grad = ops.rope_heads_d256_(leaf.grad.clone(), cs, heads, inverse=True, **rope_kw)
    assert torch.equal(_bits(out.detach()), _bits(step.detach()))
    assert torch.equal(qkv.grad, grad)               # values: the sum of the three slice gradients turns a -0 into +0
    assert bool(torch.isfinite(qkv.grad).all()) and float(qkv.grad.abs().max()) > 0
