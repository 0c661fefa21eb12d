"""The ``gqa::`` kernels (include/gmlm_hip_gqa.h: rotary embedding over head rows in place at d = 64 / 128, causal grouped-KV
attention at d = 64, padded and packed) against float64 torch on inputs rounded to storage, bf16 and fp32, forward and
backward.  Every case asserts the exact set of ``gqa::`` kernels it launched, that a second identical call gives identical
bits, and prints its worst error-to-bound ratio.  tests/test_llama_cpu.py holds the kernels compiled into the library against
the ones named here: there is no unreachable instantiation.

Budgets: those of tests/test_gpu_decoder_ops.py.  Rotary embedding, per element: one ulp of the storage type at the reference
(bf16: one bf16 ulp; fp32: 4 fp32 ulps, ``_elem_check``) plus 3 u of the rotation taken in magnitudes (u = 2^-24): the kernel
forms fma(+-other, sin, x * cos) in fp32, i.e. x * cos rounded once (u |x cos|) and the fma rounded once (u |result|, at most u
of the magnitudes), both bounded by the magnitude sum |x cos| + |other sin|, one u to spare; the table is the same fp32 table
on both sides, so it adds nothing.  Attention: ``_budget`` (fp32: max 1e-4 / l2 1e-5; bf16: max 2e-2 / l2 6e-3 for out and 8e-3
for the gradients), the tree's attention budgets, here with a contraction of 64 instead of 128 terms (no wider)."""
from dataclasses import dataclass
from functools import lru_cache

import pytest
import torch

from helpers import _close, kernels_run
from test_gpu_decoder_ops import TN, U, _budget, _elem_check, _same_bits

pytestmark = pytest.mark.gpu

BF, FP = torch.bfloat16, torch.float32
DTYPES = (BF, FP)
VEC = {BF: 8, FP: 4}
HEAD_DIMS = (64, 128)
UNREACHABLE = {}                      # every compiled gqa:: instantiation is run below


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _family(ran):
    return {n for n in ran if n.startswith("gqa::")}


# ------------------------------------------------------------------------------------------------------- 1. rotary embedding
ROPE_MAX_BLOCKS = 2048                # kRopeMaxBlocks of attn_gqa.hip


def rope_kernels(dtype, d):
    return frozenset(f"gqa::rope_heads_kernel<{TN[dtype]}, {d}, {inv}>" for inv in ("false", "true"))


def rope_rows_per_block(dtype, d):
    """head rows per 256-thread block: a head row is d / V lanes of 16 bytes"""
    return 256 // (d // VEC[dtype])


def tail_tokens(dtype, d, heads):
    """The fewest tokens for which the capped grid takes a second, partly filled trip of its stride loop."""
    return ROPE_MAX_BLOCKS * rope_rows_per_block(dtype, d) // heads + 1


@dataclass(frozen=True)
class RopeCase:
    id: str
    lead: tuple          # leading shape: (b, l) padded, (tokens,) packed; () = sized by tail_tokens
    hq: int
    hkv: int
    table: int
    positions: tuple = None

    def shape(self, dtype, d):
        return self.lead or (tail_tokens(dtype, d, self.hq + self.hkv),)

    @property
    def by_pos(self):
        return len(self.lead) != 2


ROPE_CASES = (RopeCase("b1_l1", (1, 1), 1, 1, 2), RopeCase("b2_l3_odd_heads", (2, 3), 3, 1, 3), RopeCase("seq_len1", (3, 1), 2, 1, 4),
              RopeCase("pos_one_row_table", (3,), 2, 1, 1, (-2, 0, 7)), RopeCase("tail", (), 2, 1, 300))


def _rope_table(rows, d, dev):
    inv = 1.0 / (1e6 ** (torch.arange(0, d, 2, dtype=torch.float) / d))
    fr = torch.arange(rows, dtype=torch.float32)[:, None] * inv[None]
    return torch.stack([fr.cos(), fr.sin()], 1).contiguous().to(dev)


def _rot(n, cos, sin):
    """rotate-half rotation of [..., d] rows; cos / sin [..., d / 2] (test_gpu_decoder_ops._rot at any d)"""
    half = n.shape[-1] // 2
    lo, hi = n[..., :half], n[..., half:]
    return torch.cat([lo * cos - hi * sin, hi * cos + lo * sin], -1)


def _rot_mag(n, cos, sin):
    """the same with every product taken in magnitude: what can cancel in the rotation"""
    half = n.shape[-1] // 2
    lo, hi = n[..., :half].abs(), n[..., half:].abs()
    return torch.cat([lo * cos.abs() + hi * sin.abs(), hi * cos.abs() + lo * sin.abs()], -1)


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp32"])
@pytest.mark.parametrize("d", HEAD_DIMS)
@pytest.mark.parametrize("case", ROPE_CASES, ids=[c.id for c in ROPE_CASES])
def test_rope_heads_in_place(dev, case, d, dtype):
    from gmlm_amd import ops
    shape = case.shape(dtype, d)
    heads, wid = case.hq + case.hkv, (case.hq + 2 * case.hkv) * d
    tokens = shape[0] * (shape[1] if len(shape) == 2 else 1)
    g = torch.Generator().manual_seed(tokens * 3 + d)
    x = torch.randn(*shape, wid, generator=g).to(dev, dtype)
    gr = torch.randn(*shape, wid, generator=g).to(dev, dtype)
    cs = _rope_table(case.table, d, dev)
    if case.by_pos:
        pos = torch.tensor(case.positions, dtype=torch.int32, device=dev) if case.positions else \
            (torch.arange(tokens, device=dev) * 7 % case.table).to(torch.int32)
        seq_len, row = 0, pos.long().clamp(0, case.table - 1)
    else:
        pos, seq_len = None, shape[1]
        row = (torch.arange(tokens, device=dev) % seq_len)
    if case.id == "tail":
        items = tokens * heads
        per_trip = ROPE_MAX_BLOCKS * rope_rows_per_block(dtype, d)
        assert per_trip < items < per_trip + rope_rows_per_block(dtype, d)      # a second trip, and only part of one block of it

    def run():
        y, dy = x.clone(), gr.clone()
        ops.rope_heads_(y, cs, heads, d, seq_len, pos)
        ops.rope_heads_(dy, cs, heads, d, seq_len, pos, inverse=True)
        return y, dy

    box = {}
    ran = kernels_run(lambda: box.setdefault("r", run()))
    assert _family(ran) == set(rope_kernels(dtype, d)), sorted(ran)
    assert not any(n.startswith(("qknorm_rope_", "mbert::")) for n in ran), ran
    assert _same_bits(run(), box["r"])
    y, dy = box["r"]
    cos, sin = (cs[row, i].double().view(tokens, 1, d // 2) for i in (0, 1))
    for name, got, src, sgn in (("y", y, x, 1.0), ("dx", dy, gr, -1.0)):
        got2, src2 = got.view(tokens, wid), src.view(tokens, wid)
        assert torch.equal(got2[:, heads * d:], src2[:, heads * d:]), f"{name}: V columns changed"
        n = src2[:, :heads * d].double().view(tokens, heads, d)
        _elem_check(f"{case.id} {name}", got2[:, :heads * d].view(tokens, heads, d), _rot(n, cos, sgn * sin), 3 * U * _rot_mag(n, cos, sin))
    if case.positions:
        assert int(row.max()) == 0                                  # -2, 0 and 7 all clamp to the one row


# ------------------------------------------------------------------------------------------------ 2. causal attention, d = 64
D = 64
SCALE = D ** -0.5
HEADS = ((6, 2), (7, 1))
PAST_L = 257
PAST_LENS = (1, 31, 33, 64, 65, 127, 128, 129, 200, 257)
CLAMP_L = 129
CLAMP_LENS = (CLAMP_L + 5, CLAMP_L, -3, 0)
SHORT_LS = (1, 5, 33)
SHORT_B = 3
SEQS = (1, 31, 33, 64, 65, 127, 128, 129, 257, 0)
GUARD = 128
CAUSAL_CASES = ("past_kv_len", "clamp", "short", "packed")


def causal_kernels(dtype):
    return frozenset(f"gqa::causal64_{k}_kernel<{TN[dtype]}>" for k in ("fwd", "delta", "dq", "dkv"))


def expected_kernels():
    return set().union(*(rope_kernels(dt, d) for dt in DTYPES for d in HEAD_DIMS), *(causal_kernels(dt) for dt in DTYPES))


def _split(t, hq, hkv):
    nq, nk = hq * D, hkv * D
    return t[..., :nq], t[..., nq:nq + nk], t[..., nq + nk:]


def _reference(qkv, go, kv_len, hq, hkv):
    """test_gpu_decoder_ops._causal_reference at head dim 64: dense float64 attention with the tril mask combined with the
    key-padding mask, autograd backward; a row with no visible key (kv_len = 0) has zero output and gradients."""
    b, l = qkv.shape[0], qkv.shape[1]
    rep = hq // hkv
    qd, kd, vd = (t.detach().double().requires_grad_(True) for t in _split(qkv, hq, hkv))
    qh = qd.view(b, l, hq, D).transpose(1, 2)
    kh = kd.view(b, l, hkv, D).transpose(1, 2).repeat_interleave(rep, 1)
    vh = vd.view(b, l, hkv, D).transpose(1, 2).repeat_interleave(rep, 1)
    idx = torch.arange(l, device=qkv.device)
    keep = (idx[None, :] <= idx[:, None])[None] & (idx[None, None, :] < kv_len.long()[:, None, None])      # [b, l, l]
    s = (qh @ kh.transpose(-1, -2)) * SCALE
    none = ~keep.any(-1, keepdim=True)
    s = s.masked_fill(~(keep | none)[:, None], float("-inf"))
    p = torch.softmax(s, -1) * (~none)[:, None]
    o = (p @ vh).transpose(1, 2).reshape(b, l, hq * D)
    o.backward(go.double())
    return o.detach(), qd.grad, kd.grad, vd.grad


def _op_run(qkv, go, hq, hkv, fused, call):
    """out, dq, dk, dv of ``call(q, k, v)`` on fused or contiguous operands; asserts the kernels and the repeat."""
    def run():
        if fused:
            x = qkv.clone().requires_grad_(True)
            q, k, v = _split(x, hq, hkv)
        else:
            q, k, v = (t.clone().contiguous().requires_grad_(True) for t in _split(qkv, hq, hkv))
        out = call(q, k, v)
        out.backward(go)
        grads = _split(x.grad, hq, hkv) if fused else (q.grad, k.grad, v.grad)
        return (out.detach(),) + tuple(t.contiguous() for t in grads)

    box = {}
    ran = kernels_run(lambda: box.setdefault("r", run()))
    assert _family(ran) == set(causal_kernels(qkv.dtype)), sorted(ran)
    assert not any(n.startswith(("attn_", "d128::", "causal128::")) for n in ran), ran
    assert _same_bits(run(), box["r"])
    assert all(bool(torch.isfinite(t).all()) for t in box["r"])
    return box["r"]


def _causal_run(qkv, go, kv_len, hq, hkv, fused):
    from gmlm_amd import ops
    return _op_run(qkv, go, hq, hkv, fused, lambda q, k, v: ops.causal_attention(q, k, v, kv_len, hq, hkv, SCALE, D))


def _qkv_go(dev, dtype, lead, hq, hkv, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*lead, (hq + 2 * hkv) * D, generator=g).to(dev, dtype), torch.randn(*lead, hq * D, generator=g).to(dev, dtype))


@lru_cache(maxsize=None)
def _past_problem(dev, dtype, hq, hkv):
    """Inputs and the float64 reference of the past_kv_len case, computed once for the fused and the contiguous run."""
    qkv, go = _qkv_go(dev, dtype, (len(PAST_LENS), PAST_L), hq, hkv, 71 + hq)
    kv_len = torch.tensor(PAST_LENS, dtype=torch.int32, device=dev)
    valid = (torch.arange(PAST_L, device=dev)[None, :] < kv_len[:, None])[..., None]            # [b, l, 1]
    ref = _reference(qkv, go, kv_len, hq, hkv)
    dk_valid_only = _reference(qkv, go * valid, kv_len, hq, hkv)[2]      # the reference is linear in go
    i31 = PAST_LENS.index(31)
    share = float((ref[2][i31] - dk_valid_only[i31]).norm()) / float(ref[2][i31].norm())
    return qkv, go, kv_len, valid, ref, share


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp32"])
@pytest.mark.parametrize("fused", [False, True], ids=["contiguous", "fused_qkv"])
@pytest.mark.parametrize("hq,hkv", HEADS)
def test_causal64_rows_at_and_past_kv_len(dev, hq, hkv, fused, dtype):
    qkv, go, kv_len, valid, ref, share = _past_problem(dev, dtype, hq, hkv)
    print(f"\n  share of |dk| of the kv_len = 31 sequence that comes from queries >= kv_len: {share:.2f}")
    assert share >= 0.10, share
    got = _causal_run(qkv, go, kv_len, hq, hkv, fused)
    for name, g_, r_ in zip(("out", "dq", "dk", "dv"), got, ref):
        _close(name, g_, r_, *_budget(dtype, name))
    for name, g_, r_ in zip(("out", "dq"), got, ref):              # the two halves apart: neither hides behind the other
        _close(name + " of rows < kv_len", g_ * valid, r_ * valid, *_budget(dtype, name))
        _close(name + " of rows >= kv_len", g_ * ~valid, r_ * ~valid, *_budget(dtype, name))
    for name, g_, r_ in zip(("dk", "dv"), got[2:], ref[2:]):
        assert float((r_ * ~valid).abs().max()) == 0.0
        assert float((g_ * ~valid).abs().max()) == 0.0, f"{name} of a key at or past kv_len is not zero"


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp32"])
@pytest.mark.parametrize("fused", [False, True], ids=["contiguous", "fused_qkv"])
@pytest.mark.parametrize("hq,hkv", HEADS)
def test_causal64_kv_len_is_clamped(dev, hq, hkv, fused, dtype):
    """Sequences 0 / 1 and 2 / 3 hold the same data: kv_len = l + 5 must give the bits of kv_len = l, kv_len = -3 those of 0."""
    qkv, go = _qkv_go(dev, dtype, (4, CLAMP_L), hq, hkv, 73 + hq)
    qkv[1], qkv[3], go[1], go[3] = qkv[0], qkv[2], go[0], go[2]
    kv_len = torch.tensor(CLAMP_LENS, dtype=torch.int32, device=dev)
    got = _causal_run(qkv, go, kv_len, hq, hkv, fused)
    ref = _reference(qkv, go, kv_len.clamp(0, CLAMP_L), hq, hkv)
    for name, g_, r_ in zip(("out", "dq", "dk", "dv"), got, ref):
        _close(name, g_, r_, *_budget(dtype, name))
        assert float(g_[0].abs().max()) > 0 and _same_bits([g_[0]], [g_[1]]), f"{name}: kv_len = l + 5 differs from kv_len = l"
        assert float(g_[2].abs().max()) == 0.0 and _same_bits([g_[2]], [g_[3]]), f"{name}: a sequence without keys is not zero"


def _one_key_bounds(qkv, go, hq, hkv):
    """l = 1 (test_gpu_decoder_matrix._one_key_bounds with the contraction length set to 64): the one probability is 1, so dq
    and dk are exactly 0 in the reference.  The kernels form dS = P (dP - delta) with dP = dO . v and delta = dO . O, O = v: two
    fp32 evaluations of ONE 64-term dot product, each within (64 + 2) u sum |dO_i v_i| of it, so |dS| <= 2 (64 + 2) u sum |dO_i|
    |v_i|.  The bf16 kernels carry delta into the MFMA as two bf16 numbers (hi + lo), which leaves up to 2^-18 |delta| = 64 u
    |delta| behind, and round dS and the result to bf16 (1 + 2^-7 covers both).  Then dq = scale dS k and dk = scale sum over the
    query heads of the group of dS q."""
    b, bf = qkv.shape[0], qkv.dtype == BF
    q, k, v = (t.double().reshape(b, -1, D) for t in _split(qkv, hq, hkv))
    rep = hq // hkv
    ds = (2 * (D + 2) + 64 * bf) * U * (1 + 2.0 ** -7 * bf) * (go.double().reshape(b, hq, D).abs() * v.abs().repeat_interleave(rep, 1)).sum(-1)
    dq = SCALE * ds[..., None] * k.abs().repeat_interleave(rep, 1)
    dk = SCALE * (ds[..., None] * q.abs()).view(b, hkv, rep, D).sum(2)
    return {"dq": dq.view(b, 1, hq * D), "dk": dk.view(b, 1, hkv * D)}


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp32"])
@pytest.mark.parametrize("fused", [False, True], ids=["contiguous", "fused_qkv"])
@pytest.mark.parametrize("hq,hkv", HEADS)
@pytest.mark.parametrize("l", SHORT_LS)
def test_causal64_short_padded_sequences(dev, l, hq, hkv, fused, dtype):
    qkv, go = _qkv_go(dev, dtype, (SHORT_B, l), hq, hkv, 79 + l + hq)
    got = _causal_run(qkv, go, None, hq, hkv, fused)
    ref = _reference(qkv, go, torch.full((SHORT_B,), l, device=dev), hq, hkv)
    zero = _one_key_bounds(qkv, go, hq, hkv) if l == 1 else {}
    for name, g_, r_ in zip(("out", "dq", "dk", "dv"), got, ref):
        assert g_.shape == r_.shape
        if name in zero:
            assert float(r_.abs().max()) == 0.0
            ratio = g_.double().abs() / zero[name]
            print(f"  {name} (reference 0): max |got| / bound = {float(ratio.max()):.3f}")
            assert bool((ratio <= 1).all()), (name, float(ratio.max()))
        else:
            _close(name, g_, r_, *_budget(dtype, name))


# ---- packed
T = sum(SEQS)
MAX_LEN = max(SEQS)


def _packed_reference(qkv, go, hq, hkv):
    """One sequence at a time through the padded reference; [T, .] results."""
    outs, r0 = [[], [], [], []], 0
    for n in SEQS:
        if n:
            r = _reference(qkv[None, r0:r0 + n], go[None, r0:r0 + n], torch.tensor([n], device=qkv.device), hq, hkv)
            for acc, t in zip(outs, r):
                acc.append(t[0])
        r0 += n
    return tuple(torch.cat(a) for a in outs)


def _guarded(src, fill):
    """``src`` [T, w] as the leading rows of a [T + GUARD, w] buffer whose other rows hold ``fill``."""
    buf = torch.full((T + GUARD, src.shape[1]), fill, dtype=src.dtype, device=src.device)
    buf[:T] = src
    return buf


def _raw_packed_run(qkv, go, cu, hq, hkv, fused):
    """The C entry points on buffers of this test whose cu_seqlens own rows [0, T) only: the GUARD rows behind them are owned by
    no sequence, hold NaN where they could be read and a sentinel where they could be written."""
    from gmlm_amd import ops
    dtype, dev = qkv.dtype, qkv.device
    nq, nk = hq * D, hkv * D
    lib, ptr = ops.lib(), ops._ptr
    if fused:
        q, k, v = _split(_guarded(qkv, float("nan")), hq, hkv)
    else:
        q, k, v = (_guarded(t.contiguous(), float("nan")) for t in _split(qkv, hq, hkv))
    rows = T + GUARD
    gb = _guarded(go, float("nan"))
    sent = 7.0
    out = torch.full((rows, nq), sent, dtype=dtype, device=dev)
    out_lo = torch.full((rows, nq), sent, dtype=dtype, device=dev) if dtype == BF else None
    lse = torch.full((hq, rows), sent, dtype=torch.float32, device=dev)
    dqkv = torch.full((rows, nq + 2 * nk), sent, dtype=dtype, device=dev)
    dq, dk, dv = _split(dqkv, hq, hkv)
    s = cu.numel() - 1
    ops.check(lib.gmlm_attention_causal_d64_varlen_fwd(ptr(q), ptr(k), ptr(v), ptr(cu), s, MAX_LEN, rows, hq, hkv, D, q.stride(0), k.stride(0),
                                                       v.stride(0), SCALE, 0.0, ptr(out), ptr(out_lo), ptr(lse), ops._dt(q), ops._stream()),
              "varlen_fwd")
    ws = ops._ws(lib.gmlm_attention_causal_d64_varlen_workspace_bytes(rows, hq), dev)
    ops.check(lib.gmlm_attention_causal_d64_varlen_bwd(ptr(q), ptr(k), ptr(v), ptr(out), ptr(out_lo), ptr(gb), ptr(lse), ptr(cu), s, MAX_LEN,
                                                       rows, hq, hkv, D, q.stride(0), k.stride(0), v.stride(0), SCALE, 0.0, ptr(dq), ptr(dk),
                                                       ptr(dv), dqkv.stride(0), dqkv.stride(0), dqkv.stride(0), ops._dt(q), ptr(ws),
                                                       ws.numel(), ops._stream()), "varlen_bwd")
    torch.cuda.synchronize()
    for name, buf in (("out", out), ("out_lo", out_lo), ("dqkv", dqkv)):
        if buf is not None:
            assert bool((buf[T:] == sent).all()), f"{name}: rows owned by no sequence were written"
    assert bool((lse[:, T:] == sent).all()), "lse: written for rows owned by no sequence"
    assert bool(torch.isfinite(lse[:, :T]).all())
    return out[:T], dq[:T].contiguous(), dk[:T].contiguous(), dv[:T].contiguous()


@lru_cache(maxsize=None)
def _packed_problem(dev, dtype, hq, hkv):
    qkv, go = _qkv_go(dev, dtype, (T,), hq, hkv, 83 + hq)
    return qkv, go, _packed_reference(qkv, go, hq, hkv)


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp32"])
@pytest.mark.parametrize("fused", [False, True], ids=["contiguous", "fused_qkv"])
@pytest.mark.parametrize("hq,hkv", HEADS)
def test_causal64_packed_sequences(dev, hq, hkv, fused, dtype):
    from gmlm_amd import ops
    qkv, go, ref = _packed_problem(dev, dtype, hq, hkv)
    cu = torch.tensor((0,) + SEQS, dtype=torch.int64).cumsum(0).to(dev, torch.int32)
    got = _op_run(qkv, go, hq, hkv, fused, lambda q, k, v: ops.causal_attention_varlen(q, k, v, cu, MAX_LEN, hq, hkv, SCALE, D))
    for name, g_, r_ in zip(("out", "dq", "dk", "dv"), got, ref):
        assert g_.shape == r_.shape
        _close(name, g_, r_, *_budget(dtype, name))
    raw = _raw_packed_run(qkv, go, cu, hq, hkv, fused)
    for name, g_, r_ in zip(("out", "dq", "dk", "dv"), raw, got):
        assert bool(torch.isfinite(g_).all()), name                # nothing read from the NaN rows owned by no sequence
        assert _same_bits([g_.contiguous()], [r_]), name


# ------------------------------------------------------------------------------------------ 3. the node the encoder uses
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp32"])
@pytest.mark.parametrize("d", HEAD_DIMS)
@pytest.mark.parametrize("packed", [False, True], ids=["padded", "packed"])
def test_fused_rope_gqa_node_equals_the_two_ops(dev, packed, d, dtype):
    """ops.rope_causal_gqa / _varlen (rotation in place, attention, inverse rotation in place on the fused gradient) against
    ops.rope_heads_ followed by ops.causal_attention(_varlen), which the cases above hold to float64: the same kernels on the
    same values, so the context and the fused input gradient are equal bit for bit.  d = 128 runs causal128::."""
    from gmlm_amd import ops
    hq, hkv, scale = 4, 2, d ** -0.5
    nq, nk = hq * d, hkv * d
    lens = (1, 33, 129, 64)
    g = torch.Generator().manual_seed(29 + d)
    cs = _rope_table(140, d, dev)
    if packed:
        cu = torch.tensor((0,) + lens, dtype=torch.int64).cumsum(0).to(dev, torch.int32)
        pos = torch.cat([torch.arange(n) for n in lens]).to(dev)
        lead = (sum(lens),)
    else:
        kv_len = torch.tensor(lens, dtype=torch.int32, device=dev)
        lead = (len(lens), max(lens))
    qkv = torch.randn(*lead, nq + 2 * nk, generator=g).to(dev, dtype)
    go = torch.randn(*lead, nq, generator=g).to(dev, dtype)

    def run(fused):
        x = qkv.clone().requires_grad_(True)
        if fused:
            y = x * 1.0                                             # a non-leaf buffer of this graph, as the QKV GEMM's output is
            out = ops.rope_causal_gqa_varlen(y, cs, pos, cu, max(lens), hq, hkv, d, scale) if packed else \
                ops.rope_causal_gqa(y, cs, kv_len, hq, hkv, d, scale)
            out.backward(go)
            return out.detach(), x.grad
        r = ops.rope_heads_(qkv.clone(), cs, hq + hkv, d, 0 if packed else lead[1], pos.to(torch.int32) if packed else None)
        r.requires_grad_(True)
        q, k, v = r[..., :nq], r[..., nq:nq + nk], r[..., nq + nk:]
        out = ops.causal_attention_varlen(q, k, v, cu, max(lens), hq, hkv, scale, d) if packed else \
            ops.causal_attention(q, k, v, kv_len, hq, hkv, scale, d)
        out.backward(go)
        dx = ops.rope_heads_(r.grad.clone(), cs, hq + hkv, d, 0 if packed else lead[1], pos.to(torch.int32) if packed else None, inverse=True)
        return out.detach(), dx

    box = {}
    ran = kernels_run(lambda: box.setdefault("r", run(True)))
    tn = TN[dtype]
    attn = causal_kernels(dtype) if d == 64 else {f"causal128::{k}<{tn}>" for k in ("fwd_kernel", "delta_kernel", "dq_kernel", "dkv_kernel")}
    assert {n for n in ran if n.startswith(("gqa::", "causal128::"))} == set(rope_kernels(dtype, d)) | set(attn), sorted(ran)
    assert not any(n.startswith(("qknorm_rope_", "attn_", "d128::")) for n in ran), ran
    assert _same_bits(run(True), box["r"])
    for name, a, r_ in zip(("out", "dqkv"), box["r"], run(False)):
        assert bool(torch.isfinite(a).all()) and float(a.abs().max()) > 0, name
        assert torch.equal(a, r_), name
