"""The head-dim-32 attention kernels (attn_d32.hip, gmlm_attention_d32_*): every compiled instantiation run at least once
through the ops layer against dense float64 attention on the same rounded inputs, with the kernels that really ran read back
by name from the profiler.  The table has the form of tests/test_gpu_attention_matrix.py: ``CASES`` names the exact set of
``d32::`` kernels the forward and the backward of a case launch, ``UNREACHABLE`` would list compiled instantiations the host
rule cannot select (there is none); tests/test_attention_d32_cpu.py holds their union to the code objects.

The host picks the workgroup height from the longest sequence of a call, rows = max(lq, lk) padded / max_len packed
(attn_d32.hip): rows <= 32 -> 1 wave, rows <= 128 -> 2 waves, else 4.  Cases sit on both sides of both thresholds (32 / 33,
128 / 129), in both layouts.  Budgets are ``_budget`` of the matrix, unchanged.

One valid key and dropout in bf16.  With kv_len = 1 the probability is exactly 1, the forward feeds bf16(P * keep) to the
PV product, and keep = 256 / 230 at p = 0.1 is not a bf16 number (1.1130 -> 1.1094, 0.33 % off), while the backward forms
dP * keep in fp32: dS = P (dP keep - delta), exactly 0 in float64, becomes 0.33 % of dO.V, and a whole batch of such rows lifts
the l2 error of dQ / dK over the budget although no other batch is off (gmlm_hip.h states the same for dK without dropout).
It is a property of the shared bodies, not of the head dim: the d = 64 kernels give the same figures to three digits on these
inputs zero-padded to 64 (lq = lk = 32, kv_len (32, 1, 17, 0, 39), p = 0.1: dq l2 8.4e-3 from either, 3.3e-3 at p = 0, 4.5e-3
with every key valid).  As the matrix does for its d = 96 case, the bf16 dropout cases therefore take ``_kv2``, the lengths
of ``_kv`` with 2 in the place of 1; the kv_len = 1 edge itself runs in bf16 without dropout and in fp32 with it.

Dropout masks come only from helpers.attn_dropout_scale; the slab of a (batch, head) is (b*h + head) * lq when padded and
head * total_rows + cu[seq] when packed, as for every other head dim."""
import zlib

import pytest
import torch

from helpers import _close, _dense_reference, attn_dropout_scale, kernels_run
from test_gpu_attention_matrix import BF, DEVICE_COUNTER, F32, HOST_SEED, Case, _b, _budget, _case, _kv, _packed

pytestmark = pytest.mark.gpu

D = 32


def kern(kind, t, nw, dr):
    return f"d32::{kind}_kernel<{t}, {nw}, {_b(dr)}>"


def delta(t):
    return f"d32::delta_kernel<{t}>"


def sets(t, nw, dr):
    """forward / backward kernel sets of one call: one height for its three streaming launches"""
    return {kern("fwd", t, nw, dr)}, {delta(t), kern("dq", t, nw, dr), kern("dkv", t, nw, dr)}


def _kv2(b, lk, tile):
    """``_kv`` with two valid keys where it has one (bf16 dropout cases: module docstring)"""
    return tuple(2 if n == 1 else n for n in _kv(b, lk, tile))


_LONG_LENS = (1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 200)          # max_len 200: 4 waves
_MID_LENS = (1, 31, 32, 33, 63, 64, 65, 127, 128)                     # max_len 128: 2 waves
_TINY_LENS = (1, 31, 32, 5, 17)                                       # max_len 32: 1 wave
_MID33_LENS = (33, 1, 20)                                             # max_len 33: 2 waves
# 5,462 sequences x 12 heads = 65,544 (sequence, head) pairs: past the 65,535 of a two-dimensional grid's y
_MANY_LENS = tuple(1 + i % 3 for i in range(5462))

bf, f32 = torch.bfloat16, torch.float32
CASES = [
    # ---- fp32 ----
    _case("f32_w1_L32_kvlen", f32, D, *sets(F32, 1, False), b=5, h=2, lq=32, lk=32, mode="kvlen", lens=_kv(5, 32, 16)),
    _case("f32_w1_cross_drop", f32, D, *sets(F32, 1, True), b=2, h=3, lq=20, lk=32, mode="pad", p=0.1),
    _case("f32_w2_L33_fused", f32, D, *sets(F32, 2, False), b=2, h=3, lq=33, lk=33, mode="pad", layout="fused"),
    _case("f32_w2_L128_drop_seeddev", f32, D, *sets(F32, 2, True), b=5, h=2, lq=100, lk=128, mode="kvlen", lens=_kv(5, 128, 32),
          p=0.1, seed_dev=True),
    _case("f32_w4_L129", f32, D, *sets(F32, 4, False), b=2, h=2, lq=129, lk=129, mode="pad"),
    _case("f32_w4_cross_kvlen_drop", f32, D, *sets(F32, 4, True), b=5, h=2, lq=70, lk=200, mode="kvlen", lens=_kv(5, 200, 32),
          p=0.1),
    _case("f32_packed_w4", f32, D, *sets(F32, 4, False), mode="packed", **_packed(_LONG_LENS, 2)),
    _case("f32_packed_w2", f32, D, *sets(F32, 2, False), mode="packed", **_packed(_MID_LENS, 2)),
    _case("f32_packed_w1_drop", f32, D, *sets(F32, 1, True), mode="packed", p=0.1, **_packed(_TINY_LENS, 3)),
    # ---- bf16 ----
    _case("bf16_w1_L32_kvlen_drop", bf, D, *sets(BF, 1, True), b=5, h=2, lq=32, lk=32, mode="kvlen", lens=_kv2(5, 32, 16), p=0.1),
    _case("bf16_w1_cross", bf, D, *sets(BF, 1, False), b=2, h=3, lq=20, lk=32, mode="pad"),
    _case("bf16_w2_L33_fused_drop", bf, D, *sets(BF, 2, True), b=2, h=3, lq=33, lk=33, mode="pad", layout="fused", p=0.1),
    _case("bf16_w2_L128_kvlen", bf, D, *sets(BF, 2, False), b=5, h=2, lq=128, lk=128, mode="kvlen", lens=_kv(5, 128, 64)),
    _case("bf16_w4_L129_drop_seeddev", bf, D, *sets(BF, 4, True), b=2, h=2, lq=129, lk=129, mode="pad", p=0.1, seed_dev=True),
    _case("bf16_w4_cross_kvlen", bf, D, *sets(BF, 4, False), b=5, h=2, lq=70, lk=200, mode="kvlen", lens=_kv(5, 200, 64)),
    _case("bf16_w4_cross_kvlen_drop", bf, D, *sets(BF, 4, True), b=5, h=2, lq=70, lk=200, mode="kvlen", lens=_kv2(5, 200, 64),
          p=0.1),
    _case("bf16_w4_fused_kvlen", bf, D, *sets(BF, 4, False), b=5, h=2, lq=200, lk=200, mode="kvlen", lens=_kv(5, 200, 64),
          layout="fused"),
    _case("bf16_packed_w4_drop", bf, D, *sets(BF, 4, True), mode="packed", p=0.1, **_packed(_LONG_LENS, 2)),
    _case("bf16_packed_w2_drop_seeddev", bf, D, *sets(BF, 2, True), mode="packed", p=0.1, seed_dev=True, **_packed(_MID_LENS, 2)),
    _case("bf16_packed_w2_L33", bf, D, *sets(BF, 2, False), mode="packed", **_packed(_MID33_LENS, 2)),
    _case("bf16_packed_w1", bf, D, *sets(BF, 1, False), mode="packed", **_packed(_TINY_LENS, 3)),
    _case("bf16_packed_65544_pairs", bf, D, *sets(BF, 1, False), mode="packed", **_packed(_MANY_LENS, 12)),
]

UNREACHABLE = {}        # every compiled height of every kernel is selected by some `rows` (attn_d32.hip, pick_waves)


def _is_d32(name):
    return name.startswith("d32::")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _inputs(c: Case, dev):
    hd = c.h * c.d
    packed = c.mode == "packed"
    g = torch.Generator().manual_seed(zlib.crc32(c.id.encode()))
    nb = 1 if packed else c.b
    q = torch.randn(nb, c.lq, hd, generator=g).to(dev, c.dtype)
    k = (torch.randn(nb, c.lk, hd, generator=g) * 1.5).to(dev, c.dtype)   # scores ~ N(0, 1.5): neither flat nor one-hot
    v = torch.randn(nb, c.lk, hd, generator=g).to(dev, c.dtype)
    go = torch.randn(nb, c.lq, hd, generator=g).to(dev, c.dtype)
    return q, k, v, go


def _run(c: Case, dev, q, k, v, go, seed):
    """One forward + backward through the ops layer -> (outputs [out, dq, dk, dv], forward kernels, backward kernels)."""
    from gmlm_amd import ops
    h, hd, scale = c.h, c.h * c.d, c.d ** -0.5
    box = {}
    if c.mode == "packed":
        qkv = torch.cat([q, k, v], -1)[0].requires_grad_(True)            # [total_rows, 3hd]
        cu = torch.tensor([0] + torch.tensor(c.lens).cumsum(0).tolist(), dtype=torch.int32, device=dev)
        fwd_k = kernels_run(lambda: box.setdefault("out", ops.AttentionQKV.apply(qkv, None, h, scale, c.p, seed, cu, max(c.lens))))
        out = box["out"]
        bwd_k = kernels_run(lambda: out.backward(go[0]))
        return [out.detach(), qkv.grad[:, :hd], qkv.grad[:, hd:2 * hd], qkv.grad[:, 2 * hd:]], fwd_k, bwd_k
    kv_len = torch.tensor(c.lens, dtype=torch.int32, device=dev) if c.mode == "kvlen" else None
    if c.layout == "fused":
        qkv = torch.cat([q, k, v], -1)
        qi, ki, vi = (qkv[..., i * hd:(i + 1) * hd].requires_grad_(True) for i in range(3))
        assert qi.stride(1) == 3 * hd
    else:
        qi, ki, vi = (t_.clone().requires_grad_(True) for t_ in (q, k, v))
    fwd_k = kernels_run(lambda: box.setdefault("out", ops.Attention.apply(qi, ki, vi, kv_len, h, scale, c.p, seed)))
    out = box["out"]
    bwd_k = kernels_run(lambda: out.backward(go))
    return [out.detach(), qi.grad, ki.grad, vi.grad], fwd_k, bwd_k


def _packed_reference_by_length(c: Case, q, k, v, go):
    """Dense float64 attention of a packed batch without dropout, all sequences of one length in one batched evaluation
    (thousands of sequences: helpers._dense_reference walks them one by one)."""
    h, d, scale = c.h, c.d, c.d ** -0.5
    lens = torch.tensor(c.lens)
    start = torch.cumsum(lens, 0) - lens
    ref = [torch.zeros(c.lq, h * d, dtype=torch.float64, device=q.device) for _ in range(4)]
    for n in sorted(set(c.lens)):
        rows = (start[lens == n][:, None] + torch.arange(n)[None, :]).to(q.device)          # [s, n] row numbers
        heads = lambda t_: t_[0][rows].double().reshape(-1, n, h, d).transpose(1, 2)        # [s, h, n, d]
        qq, kk, vv = (heads(t_).requires_grad_(True) for t_ in (q, k, v))
        o = torch.softmax((qq @ kk.transpose(-1, -2)) * scale, -1) @ vv
        o.backward(heads(go))
        for dst, src in zip(ref, (o.detach(), qq.grad, kk.grad, vv.grad)):
            dst[rows] = src.transpose(1, 2).reshape(-1, n, h * d)
    return ref


def _reference(c: Case, dev, q, k, v, go, mask_seed):
    h, lq, lk = c.h, c.lq, c.lk
    if c.mode == "packed" and len(c.lens) > 64:
        assert not c.p
        return _packed_reference_by_length(c, q, k, v, go), None
    if c.mode == "packed":
        ref = [torch.zeros(lq, h * c.d, dtype=torch.float64, device=dev) for _ in range(4)]
        r0 = 0
        for n in c.lens:
            drop = None
            if c.p:
                drop = lambda bi, hi, r0=r0, n=n: attn_dropout_scale(mask_seed, hi * lq + r0, n, n, c.p, dev)
            rs = _dense_reference(q[:, r0:r0 + n], k[:, r0:r0 + n], v[:, r0:r0 + n], go[:, r0:r0 + n], h, c.d ** -0.5, None, drop)
            for i in range(4):
                ref[i][r0:r0 + n] = rs[i][0]
            r0 += n
        return ref, None
    kv_len = torch.tensor(c.lens, dtype=torch.int32) if c.mode == "kvlen" else None
    drop = None
    if c.p:
        drop = lambda bi, hi: attn_dropout_scale(mask_seed, (bi * h + hi) * lq, lq, lk, c.p, dev)
    ref = _dense_reference(q, k, v, go, h, c.d ** -0.5, kv_len, drop)
    valid = None if kv_len is None else torch.arange(lk)[None, :] < kv_len[:, None]
    return ref, valid


def _seeds(c: Case, dev, monkeypatch):
    from gmlm_amd import ops
    if not c.seed_dev:
        return 0x1234_5678_9ABC, 0x1234_5678_9ABC
    monkeypatch.setattr(ops, "SEED_DEVICE", torch.tensor([DEVICE_COUNTER], dtype=torch.int64, device=dev))
    assert (HOST_SEED + DEVICE_COUNTER) >> 32 == 1                        # the 64-bit sum carries into the high word
    return HOST_SEED, HOST_SEED + DEVICE_COUNTER


@pytest.mark.parametrize("c", CASES, ids=[c.id for c in CASES])
def test_d32_instantiation_vs_dense_fp64(dev, monkeypatch, c):
    seed, mask_seed = _seeds(c, dev, monkeypatch)
    q, k, v, go = _inputs(c, dev)
    outs, fwd_k, bwd_k = _run(c, dev, q, k, v, go, seed)
    ref, valid = _reference(c, dev, q, k, v, go, mask_seed)
    print(f"\n{c.id}: forward {sorted(fwd_k)}, backward {sorted(bwd_k)}")
    assert {n for n in fwd_k if _is_d32(n)} == set(c.fwd), (sorted(fwd_k), sorted(c.fwd))
    assert {n for n in bwd_k if _is_d32(n)} == set(c.bwd), (sorted(bwd_k), sorted(c.bwd))
    assert not [n for n in fwd_k | bwd_k if n.startswith("attn_") or n.startswith("d128::")], sorted(fwd_k | bwd_k)
    for name, got in zip(("out", "dq", "dk", "dv"), outs):
        assert bool(torch.isfinite(got).all()), name
    for name, got, r_ in zip(("out", "dq", "dk", "dv"), outs, ref):
        _close(name, got, r_, *_budget(c.dtype, name))
    if valid is not None:                                  # keys at or past kv_len: no gradient at all
        valid = valid.to(dev)
        assert float(outs[2][~valid].abs().sum()) == 0.0 and float(outs[3][~valid].abs().sum()) == 0.0
        for bi in [i for i, n in enumerate(c.lens) if n == 0]:     # no valid key: zero output, zero dq
            assert float(outs[0][bi].abs().max()) == 0.0 and float(outs[1][bi].abs().max()) == 0.0


_REPEAT = ("f32_w4_cross_kvlen_drop", "bf16_packed_w2_drop_seeddev", "bf16_w1_L32_kvlen_drop", "bf16_packed_w4_drop")


@pytest.mark.parametrize("cid", _REPEAT)
def test_d32_repeat_run_is_bit_identical(dev, monkeypatch, cid):
    """No atomics, fixed summation orders: the same call twice gives the same bits, output and gradients."""
    c = next(c_ for c_ in CASES if c_.id == cid)
    seed, _ = _seeds(c, dev, monkeypatch)
    q, k, v, go = _inputs(c, dev)
    first, _, _ = _run(c, dev, q, k, v, go, seed)
    again, _, _ = _run(c, dev, q, k, v, go, seed)
    for name, a, b_ in zip(("out", "dq", "dk", "dv"), first, again):
        assert torch.equal(a, b_), name


@pytest.mark.parametrize("dtype", [f32, bf], ids=["f32", "bf16"])
def test_dropout_mask_does_not_depend_on_the_head_dim(dev, dtype):
    """The same inputs through the d = 32 kernels and, zero-padded to 64 per head, through the d = 64 kernels, p = 0.1 and one
    seed: both land within budget of ONE float64 reference that uses one mask (helpers.attn_dropout_scale)."""
    from gmlm_amd import ops
    b, h, lq, lk, p, seed = 2, 3, 70, 200, 0.1, 0x1234_5678_9ABC
    c = _case("mask", dtype, D, (), (), b=b, h=h, lq=lq, lk=lk, mode="pad", p=p)
    q, k, v, go = _inputs(c, dev)
    scale = D ** -0.5
    ref = _dense_reference(q, k, v, go, h, scale, None, lambda bi, hi: attn_dropout_scale(seed, (bi * h + hi) * lq, lq, lk, p, dev))
    native, fwd_k, bwd_k = _run(c, dev, q, k, v, go, seed)
    assert fwd_k | bwd_k == set().union(*sets(BF if dtype == bf else F32, 4, True)), sorted(fwd_k | bwd_k)

    def widen(t_):                                                         # [b, l, h*32] -> [b, l, h*64], zeros in the upper half
        return torch.nn.functional.pad(t_.reshape(*t_.shape[:2], h, D), (0, D)).reshape(*t_.shape[:2], h * 2 * D)

    def narrow(t_):
        return t_.reshape(*t_.shape[:2], h, 2 * D)[..., :D].reshape(*t_.shape[:2], h * D)

    qi, ki, vi = (widen(t_).requires_grad_(True) for t_ in (q, k, v))
    box = {}
    wide_k = kernels_run(lambda: box.setdefault("out", ops.Attention.apply(qi, ki, vi, None, h, scale, p, seed)))
    assert any(n.startswith("attn_") for n in wide_k) and not any(_is_d32(n) for n in wide_k), sorted(wide_k)
    box["out"].backward(widen(go))
    padded = [narrow(t_) for t_ in (box["out"].detach(), qi.grad, ki.grad, vi.grad)]
    for tag, outs in (("d32", native), ("d64 zero-padded", padded)):
        print(f"\n{tag}:")
        for name, got, r_ in zip(("out", "dq", "dk", "dv"), outs, ref):
            _close(name, got, r_, *_budget(dtype, name))
