"""The band-limited grouped-KV attention kernels at head dim 256 (gmlm_attention_gqa_d256_band_*, csrc/attn_gqa_band.hip, namespace
gqab::) through ``ops.gqa_d256_band_attention`` / ``_varlen`` on slices of a fused buffer, against dense float64 attention on the
same rounded inputs, forward and backward.

The mask:  visible(i, j) = j < kv_len and (0 <= i - j < w if causal else |i - j| < w), an EXCLUSIVE window w >= 1.

The checker (``_reference``) is the computation of test_gpu_gqa_wide_kernels._reference (scores of the query head against its KV
head, softmax, K / V repeated over the group under autograd) with the band added to its mask and a row without a visible key
giving zeros; ``test_window_past_the_length_is_the_unbanded_family_bit_for_bit`` ties it to that function with w >= L.  The
budgets are those of tests/test_gpu_attention_wide.py, imported unchanged (same head dim, same rounding points): fp32 1e-4 max /
1e-5 relative L2; bf16 2e-2 max, 6e-3 relative L2 for out and dv, 8e-3 for dq and dk.  Every case prints the measured value beside
its budget.  Scale 1 / 12 and K scaled 1.5 as there.

Edges.  One tile height (32 query rows, 32 keys).  Windows 1 (self only), 2 (the smallest band), 31, 32, 33, 64, 65 (the tile
edge inside, on and one past the first and the second tile) and 100; with w < 32 a row can see no key in the first tile of its
loop.  Lengths 1, 33, 65, 129, 257.  Padded: kv_len = L, 1, 0 and L // 2 per length; with a small window the last leaves queries
at or past kv_len + w - 1 that see no key at all: exact zeros in out and dq, lse = -inf, nothing added to dk / dv.  Packed: the
five lengths and an empty sequence in one call, max_len once exact and once larger.

Not vacuous: wherever 2 w <= L and kv_len = L the float64 banded and un-banded outputs differ by >= 0.1 in relative L2.

Every test here calls one of the two operators, which the tree before this kernel family does not have."""
import pytest
import torch

import test_gpu_gqa_wide_kernels as GW
from helpers import kernels_run
from test_gpu_attention_wide import _budget
from test_gpu_gqa_wide_kernels import D, PAD, SCALE, TN, _check, _flat, _fused, _slices

pytestmark = pytest.mark.gpu

HEADS = ((3, 1), (4, 2))
WINDOWS = (1, 2, 31, 32, 33, 64, 65, 100)
LENS = (1, 33, 65, 129, 257)
DTYPES = (torch.float32, torch.bfloat16)
NEG = float("-inf")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def visible(n, kv, window, causal, device):
    """bool [.., n, n]: the stated rule, element by element; ``kv`` a number or a [b] tensor"""
    i, j = torch.arange(n, device=device)[:, None], torch.arange(n, device=device)[None, :]
    band = (i - j >= 0) & (i - j < window) if causal else (i - j).abs() < window
    if torch.is_tensor(kv):
        return band[None] & (j[None] < kv[:, None, None])
    return band & (j < kv)


def _reference(q, k, v, go, kv, hq, hkv, scale, causal, window):
    """q, go [b, L, hq * D], k, v [b, L, hkv * D], kv int [b] (already clamped) -> out, dq, dk, dv, lse in float64; a query
    without a visible key gives a zero row (and takes no part in the backward), its lse is -inf"""
    b, L = q.shape[:2]
    g = hq // hkv
    heads = lambda t, h: t.double().reshape(b, L, h, D).transpose(1, 2).contiguous().requires_grad_(True)
    qq, kk, vv = heads(q, hq), heads(k, hkv), heads(v, hkv)
    mask = visible(L, kv, window, causal, q.device)[:, None]                 # [b, 1, L, L]
    some = mask.any(-1, keepdim=True)
    s = (qq @ kk.repeat_interleave(g, 1).transpose(2, 3)) * scale
    p = torch.softmax(s.masked_fill(~(mask | ~some), NEG), -1) * some       # a row that sees nothing: uniform, then times 0
    o = p @ vv.repeat_interleave(g, 1)
    o.backward(go.double().reshape(b, L, hq, D).transpose(1, 2))
    lse = torch.logsumexp(s.detach().masked_fill(~mask, NEG), -1)           # [b, hq, L]; -inf where nothing is visible
    back = lambda t: t.transpose(1, 2).reshape(b, L, -1)
    return back(o.detach()), back(qq.grad), back(kk.grad), back(vv.grad), lse


def _pad_batch(t, cu, width):
    """packed rows [T, f] -> [S, width, f] (zero padded)"""
    out = t.new_zeros(len(cu) - 1, width, t.shape[-1])
    for i in range(len(cu) - 1):
        out[i, :cu[i + 1] - cu[i]] = t[cu[i]:cu[i + 1]]
    return out


def _unpad(t, cu):
    return torch.cat([t[i, :cu[i + 1] - cu[i]] for i in range(len(cu) - 1)])


def _kernel_sets(dtype, causal):
    t, c = TN[dtype], "true" if causal else "false"
    return ({f"gqab::fwd_kernel<{t}, {c}>"}, {f"gqab::delta_kernel<{t}>", f"gqab::dq_kernel<{t}, {c}>", f"gqab::dkv_kernel<{t}, {c}>"})


def _run(buf, go, hq, hkv, causal, window, kv_len=None, cu=None, max_len=0, kernels=False):
    """Through the operator on slices of the fused buffer -> out, lse, dq, dk, dv (the gradients as slices of buf.grad)."""
    from gmlm_amd import ops
    leaf = buf.clone().requires_grad_(True)
    q, k, v = _slices(leaf, hq, hkv)
    assert q.stride(-2) == (hq + 2 * hkv) * D + PAD
    if cu is None:
        fwd = lambda: ops.gqa_d256_band_attention(q, k, v, kv_len, hq, hkv, SCALE, causal, window)
    else:
        fwd = lambda: ops.gqa_d256_band_attention_varlen(q, k, v, cu, max_len, hq, hkv, SCALE, causal, window)
    if kernels:
        box = {}
        fwd_k = kernels_run(lambda: box.setdefault("o", fwd()))
        out = box["o"]
        lse = out.grad_fn.saved_tensors[4]                            # before the backward frees what the node saved
        bwd_k = kernels_run(lambda: out.backward(go))
        assert (fwd_k, bwd_k) == _kernel_sets(buf.dtype, causal), (sorted(fwd_k), sorted(bwd_k))   # and so no gqaw:: kernel
    else:
        out = fwd()
        lse = out.grad_fn.saved_tensors[4]
        out.backward(go)
    assert float(leaf.grad[..., (hq + 2 * hkv) * D:].abs().max()) == 0.0           # the padding columns get no gradient
    return (out.detach(), lse) + tuple(t.clone() for t in _slices(leaf.grad, hq, hkv))


def _bound(q, k, v, go):
    return float(v.double().abs().max()) * float(go.double().abs().max()) * float(k.double().abs().max() + q.double().abs().max())


def _rel_l2(a, b):
    return float((a - b).norm()) / float(b.norm())


def _bits(t):
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32)


def _same(tag, a, b):
    for name, x, y in zip(("out", "lse", "dq", "dk", "dv"), a, b):
        assert torch.equal(_bits(x), _bits(y)), (tag, name, float((x.double() - y.double()).abs().nan_to_num(1e30).max()))


def _assert_blind_rows(tag, got, kv, window, causal, L):
    """queries that see no key: exact zeros in out and dq, lse = -inf; every other lse finite; keys at or past kv_len: dk = dv = 0"""
    out, lse, dq, dk, dv = got
    blind = ~visible(L, kv, window, causal, out.device).any(-1)             # [b, L]
    for name, t in (("out", out), ("dq", dq), ("dk", dk), ("dv", dv)):
        assert bool(torch.isfinite(t).all()), (tag, name)
    if bool(blind.any()):
        assert float(out[blind].abs().max()) == 0.0 and float(dq[blind].abs().max()) == 0.0, tag
    hq = lse.shape[1]
    assert bool((lse[blind[:, None].expand(-1, hq, -1)] == NEG).all()) and bool(torch.isfinite(lse[~blind[:, None].expand(-1, hq, -1)]).all()), tag
    dead = torch.arange(L, device=out.device)[None, :] >= kv[:, None]
    if bool(dead.any()):
        assert float(dk[dead].abs().max()) == 0.0 and float(dv[dead].abs().max()) == 0.0, tag
    return int(blind.sum())


@pytest.mark.parametrize("dtype", DTYPES, ids=("fp32", "bf16"))
@pytest.mark.parametrize("causal", [False, True], ids=("bidir", "causal"))
@pytest.mark.parametrize("hq,hkv", HEADS)
def test_padded_windows_lengths_and_kv_len_vs_dense_fp64(dev, hq, hkv, causal, dtype):
    """Per window and length L: four sequences with kv_len L, 1, 0 and L // 2."""
    blind_total = 0
    for L in LENS:
        buf, go = _fused(dev, dtype, (4, L), hq, hkv, 100 * L + hq + hkv)
        kv = torch.tensor([L, 1, 0, L // 2], device=dev)
        kv_len = kv.to(torch.int32)
        q, k, v = _slices(buf, hq, hkv)
        full = _reference(q, k, v, go, kv, hq, hkv, SCALE, causal, 1 << 29)[0]
        for w in WINDOWS:
            tag = f"padded L={L} w={w} {hq}/{hkv} causal={causal} {dtype}"
            got = _run(buf, go, hq, hkv, causal, w, kv_len=kv_len, kernels=(L, w) == (129, 33))
            ref = _reference(q, k, v, go, kv, hq, hkv, SCALE, causal, w)
            _check(tag, dtype, [None if i == 1 else _flat(t) for i, t in enumerate(got)], [_flat(t) for t in ref[:4]], _bound(q, k, v, go))
            blind_total += _assert_blind_rows(tag, got, kv, w, causal, L)
            seen = torch.isfinite(ref[4])
            lerr = float((got[1].double() - ref[4])[seen].abs().max()) / float(ref[4][seen].abs().max()) if bool(seen.any()) else 0.0
            print(f"  lse: max|err| / max|ref| = {lerr:.2e} (budget {_budget(dtype, False)[0]:.0e})")
            assert lerr <= _budget(dtype, False)[0], tag
            if 2 * w <= L:                                               # the band must matter: a condition on the case, not a measurement
                differs = _rel_l2(ref[0][0], full[0])
                print(f"  float64 banded vs un-banded out, kv_len = L: rel l2 = {differs:.2f} (must be >= 0.1)")
                assert differs >= 0.1, tag
    assert blind_total > 0


@pytest.mark.parametrize("dtype", DTYPES, ids=("fp32", "bf16"))
def test_rows_that_see_nothing_at_129_33_40(dev, dtype):
    """L = 129, w = 33, kv_len = 40, causal: the 57 queries from row 72 = kv_len + w - 1 on see no key."""
    hq, hkv, L, w = 3, 1, 129, 33
    buf, go = _fused(dev, dtype, (2, L), hq, hkv, 4)
    kv = torch.tensor([40, 129], device=dev)
    blind = ~visible(L, kv, w, True, dev).any(-1)
    assert int(blind[0].sum()) == 57 and int(blind[0].nonzero()[0]) == 72 and int(blind[1].sum()) == 0
    got = _run(buf, go, hq, hkv, True, w, kv_len=kv.to(torch.int32))
    assert _assert_blind_rows("129/33/40", got, kv, w, True, L) == 57
    q, k, v = _slices(buf, hq, hkv)
    ref = _reference(q, k, v, go, kv, hq, hkv, SCALE, True, w)
    _check(f"129/33/40 {dtype}", dtype, [None if i == 1 else _flat(t) for i, t in enumerate(got)], [_flat(t) for t in ref[:4]], 0.0)
    # the blind rows add nothing to dk / dv: the same call on the first 72 rows alone gives the same key gradients to rounding of
    # nothing at all, i.e. bit for bit (the query loop of dK/dV walks the same tiles up to row 71, and the rest multiply by P = 0)
    cut = _run(buf[:1, :72].contiguous(), go[:1, :72].contiguous(), hq, hkv, True, w, kv_len=kv[:1].to(torch.int32))
    assert torch.equal(_bits(got[3][0, :72]), _bits(cut[3][0])) and torch.equal(_bits(got[4][0, :72]), _bits(cut[4][0]))


@pytest.mark.parametrize("dtype", DTYPES, ids=("fp32", "bf16"))
@pytest.mark.parametrize("causal", [False, True], ids=("bidir", "causal"))
@pytest.mark.parametrize("hq,hkv", HEADS)
def test_packed_windows_vs_dense_fp64_and_vs_the_padded_pass(dev, hq, hkv, causal, dtype):
    """The five lengths and an empty sequence back to back in one packed call per window, max_len exact (257); max_len larger
    (300) gives the same bytes; each sequence alone in the padded layout gives the same bytes."""
    lens = [1, 33, 0, 65, 129, 257]
    cu_l = [0] + torch.tensor(lens).cumsum(0).tolist()
    cu = torch.tensor(cu_l, dtype=torch.int32, device=dev)
    total = sum(lens)
    buf, go = _fused(dev, dtype, (total,), hq, hkv, 31 + hq + hkv)
    q, k, v = _slices(buf, hq, hkv)
    width = max(lens)
    qb, kb, vb, gb = (_pad_batch(t, cu_l, width) for t in (q, k, v, go))
    kv = torch.tensor(lens, device=dev)
    full = _reference(qb, kb, vb, gb, kv, hq, hkv, SCALE, causal, 1 << 29)[0]
    for w in WINDOWS:
        tag = f"packed w={w} {hq}/{hkv} causal={causal} {dtype}"
        got = _run(buf, go, hq, hkv, causal, w, cu=cu, max_len=width, kernels=w == 33)
        ref_b = _reference(qb, kb, vb, gb, kv, hq, hkv, SCALE, causal, w)
        ref = [_unpad(t, cu_l) for t in ref_b[:4]]
        _check(tag, dtype, got, ref, _bound(q, k, v, go))
        assert tuple(got[1].shape) == (hq, total) and bool(torch.isfinite(got[1]).all())       # every row sees itself
        _same(tag + " max_len 300", got, _run(buf, go, hq, hkv, causal, w, cu=cu, max_len=300))
        for i, n in enumerate(lens):
            if n == 0:
                continue
            r0 = cu_l[i]
            one = _run(buf[r0:r0 + n][None], go[r0:r0 + n][None], hq, hkv, causal, w)
            _same(f"{tag} sequence of {n} padded", (got[0][r0:r0 + n], got[1][:, r0:r0 + n], got[2][r0:r0 + n], got[3][r0:r0 + n],
                                                    got[4][r0:r0 + n]), tuple(t[0] for t in one))
            if 2 * w <= n:
                differs = _rel_l2(ref_b[0][i, :n], full[i, :n])
                print(f"  n={n} float64 banded vs un-banded out: rel l2 = {differs:.2f} (must be >= 0.1)")
                assert differs >= 0.1, (tag, n)


@pytest.mark.parametrize("dtype", DTYPES, ids=("fp32", "bf16"))
@pytest.mark.parametrize("causal", [False, True], ids=("bidir", "causal"))
def test_window_past_the_length_is_the_unbanded_family_bit_for_bit(dev, causal, dtype):
    """w = L and L + 7: the loops visit the same tiles in the same order and no guard changes a finite value, so out, lse, dq, dk
    and dv are the bytes of ``ops.gqa_d256_attention`` / ``_varlen``; and the float64 checker of this file is then that file's."""
    hq, hkv = 4, 2
    for L in LENS:
        buf, go = _fused(dev, dtype, (4, L), hq, hkv, 50 + L)
        kv_len = torch.tensor([L, 1, 0, L // 2], dtype=torch.int32, device=dev)
        plain = GW._run(buf, go, hq, hkv, causal, kv_len=kv_len)
        for w in (L, L + 7):
            _same(f"padded L={L} w={w}", _run(buf, go, hq, hkv, causal, w, kv_len=kv_len), plain)
        q, k, v = _slices(buf, hq, hkv)
        mine = _reference(q, k, v, go, kv_len.long(), hq, hkv, SCALE, causal, L)
        theirs = GW._reference(_flat(q), _flat(k), _flat(v), _flat(go), [(i * L, L, int(n)) for i, n in enumerate(kv_len)], hq, hkv, SCALE, causal)
        for a, r in zip(mine, theirs):
            assert float((_flat(a) - r).abs().max()) <= 1e-12 * max(1.0, float(r.abs().max()))
    lens = [1, 33, 0, 65, 129, 257]
    cu = torch.tensor([0] + torch.tensor(lens).cumsum(0).tolist(), dtype=torch.int32, device=dev)
    buf, go = _fused(dev, dtype, (sum(lens),), hq, hkv, 77)
    plain = GW._run(buf, go, hq, hkv, causal, cu=cu, max_len=257)
    for w in (257, 264):
        _same(f"packed w={w}", _run(buf, go, hq, hkv, causal, w, cu=cu, max_len=257), plain)


@pytest.mark.parametrize("dtype", DTYPES, ids=("fp32", "bf16"))
@pytest.mark.parametrize("causal", [False, True], ids=("bidir", "causal"))
def test_repeated_call_gives_identical_bytes(dev, causal, dtype):
    hq, hkv, L = 4, 2, 129
    buf, go = _fused(dev, dtype, (3, L), hq, hkv, 11)
    kv_len = torch.tensor([L, 40, 97], dtype=torch.int32, device=dev)
    for w in (2, 33):
        _same(f"w={w}", _run(buf, go, hq, hkv, causal, w, kv_len=kv_len), _run(buf, go, hq, hkv, causal, w, kv_len=kv_len))


def test_nothing_to_do_and_refused_windows(dev):
    """0 sequences / 0 rows through the operator; a window outside [1, 2^30) is refused by the operator and by the entry point,
    without a launch."""
    from gmlm_amd import _lib, ops
    hq, hkv = 3, 1
    for shape in ((0, 5), (2, 0)):
        q = torch.zeros(*shape, hq * D, device=dev, requires_grad=True)
        k, v = (torch.zeros(*shape, hkv * D, device=dev, requires_grad=True) for _ in range(2))
        out = ops.gqa_d256_band_attention(q, k, v, None, hq, hkv, SCALE, True, 4)
        out.sum().backward()
        assert tuple(out.shape) == (*shape, hq * D) and tuple(k.grad.shape) == tuple(k.shape)
    q = torch.zeros(1, 8, hq * D, device=dev)
    k, v = (torch.zeros(1, 8, hkv * D, device=dev) for _ in range(2))
    for w in (0, -1, 1 << 30):
        with pytest.raises(ValueError, match="window"):
            ops.gqa_d256_band_attention(q, k, v, None, hq, hkv, SCALE, False, w)
    lib = _lib.lib()
    out, lse = torch.zeros(1, 8, hq * D, device=dev), torch.zeros(1, hq, 8, device=dev)

    def calls():
        for w in (0, -1, 1 << 30):
            rc = lib.gmlm_attention_gqa_d256_band_fwd(q.data_ptr(), k.data_ptr(), v.data_ptr(), None, 1, hq, hkv, 8, 8, D, hq * D, hkv * D,
                                                      hkv * D, SCALE, 0.0, 1, w, out.data_ptr(), None, lse.data_ptr(), _lib.F32, None)
            assert rc == -1 and b"window" in lib.gmlm_last_error()
        torch.zeros(4, device=dev).add_(1)

    assert kernels_run(calls) == set()
