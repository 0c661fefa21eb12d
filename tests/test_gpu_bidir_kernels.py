"""The ``bidir::`` kernels (include/gmlm_hip_bidir.h: bidirectional attention with grouped KV heads at d = 64 / 128, padded and
packed) against float64 torch full attention with ``repeat_interleave``d K / V on inputs rounded to storage, bf16 and fp32,
forward, dq, dk and dv.  Every case asserts the exact set of ``bidir::`` kernels it launched, that a second identical call
gives identical bits, and prints its worst error-to-bound ratio.  tests/test_bidir_cpu.py holds the kernels compiled into the
library against the ones named here: there is no unreachable instantiation.

Budgets: ``_budget`` of tests/test_gpu_decoder_ops.py, the tree's attention budgets (fp32: max 1e-4 / l2 1e-5; bf16: max 2e-2 /
l2 6e-3 for out and 8e-3 for the gradients), here at contractions of 64 and 128 terms.  Where the reference is exactly zero (one
key: P = 1, dS = 0) the bound is that of tests/test_gpu_gqa_kernels.py ``_one_key_bounds`` at the case's head dim.

The shapes are the smallest that cross each loop edge: one row; one past a wave (33); one past a workgroup (129); a key-tile
edge (64, 65: the bf16 tile is 64 keys, the fp32 one 32); kv_len inside a tile with query rows past it; an empty sequence; query
groups of 1, 2, 3 and 7 heads per KV head."""
from functools import lru_cache

import pytest
import torch

from helpers import _close, kernels_run
from test_gpu_decoder_ops import TN, U, _budget, _same_bits

pytestmark = pytest.mark.gpu

BF, FP = torch.bfloat16, torch.float32
DTYPES = (BF, FP)
HEAD_DIMS = (64, 128)
UNREACHABLE = {}                      # every compiled bidir:: instantiation is run below
NAMES = ("out", "dq", "dk", "dv")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def bidir_kernels(dtype, d):
    return frozenset(f"bidir::gqa_{k}_kernel<{TN[dtype]}, {d}>" for k in ("fwd", "delta", "dq", "dkv"))


def expected_kernels():
    return set().union(*(bidir_kernels(dt, d) for dt in DTYPES for d in HEAD_DIMS))


def _family(ran):
    return {n for n in ran if n.startswith("bidir::")}


def _split(t, hq, hkv, d):
    nq, nk = hq * d, hkv * d
    return t[..., :nq], t[..., nq:nq + nk], t[..., nq + nk:]


def _reference(qkv, go, kv_len, hq, hkv, d):
    """Dense float64 attention under the key-padding mask alone, K / V heads repeated per group, autograd backward; a
    sequence with kv_len = 0 has zero output and gradients.  -> out, dq, dk, dv"""
    b, l = qkv.shape[0], qkv.shape[1]
    rep = hq // hkv
    qd, kd, vd = (t.detach().double().requires_grad_(True) for t in _split(qkv, hq, hkv, d))
    qh = qd.view(b, l, hq, d).transpose(1, 2)
    kh = kd.view(b, l, hkv, d).transpose(1, 2).repeat_interleave(rep, 1)
    vh = vd.view(b, l, hkv, d).transpose(1, 2).repeat_interleave(rep, 1)
    keep = (torch.arange(l, device=qkv.device)[None, :] < kv_len.long()[:, None])[:, None, None, :]      # [b, 1, 1, l]
    none = ~keep.any(-1, keepdim=True)
    s = (qh @ kh.transpose(-1, -2)) * d ** -0.5
    s = s.masked_fill(~(keep | none), float("-inf"))
    p = torch.softmax(s, -1) * ~none
    o = (p @ vh).transpose(1, 2).reshape(b, l, hq * d)
    o.backward(go.double())
    return o.detach(), qd.grad, kd.grad, vd.grad


def _qkv_go(dev, dtype, lead, hq, hkv, d, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*lead, (hq + 2 * hkv) * d, generator=g).to(dev, dtype), torch.randn(*lead, hq * d, generator=g).to(dev, dtype))


def _op_run(qkv, go, hq, hkv, d, call):
    """out, dq, dk, dv of ``call(q, k, v)`` on contiguous operands; asserts the kernels and the repeat."""
    def run():
        q, k, v = (t.clone().contiguous().requires_grad_(True) for t in _split(qkv, hq, hkv, d))
        out = call(q, k, v)
        out.backward(go)
        return out.detach(), q.grad, k.grad, v.grad

    box = {}
    ran = kernels_run(lambda: box.setdefault("r", run()))
    assert _family(ran) == set(bidir_kernels(qkv.dtype, d)), sorted(ran)
    assert not any(n.startswith(("attn_", "d128::", "causal128::", "gqa::")) for n in ran), ran
    assert _same_bits(run(), box["r"])
    assert all(bool(torch.isfinite(t).all()) for t in box["r"])
    return box["r"]


def _check(dtype, got, ref):
    worst = 0.0
    for name, g_, r_ in zip(NAMES, got, ref):
        assert g_.shape == r_.shape
        _close(name, g_, r_, *_budget(dtype, name))
        e = g_.double() - r_
        mx, l2 = _budget(dtype, name)
        worst = max(worst, float(e.abs().max()) / float(r_.abs().max()) / mx, float(e.norm()) / float(r_.norm()) / l2)
    print(f"  worst error / bound = {worst:.3f}")


# ---------------------------------------------------------------------------------------------------------------- padded
# (b, hq, hkv, l, kv_len)
PADDED = ((1, 1, 1, 1, None), (2, 6, 2, 33, (33, 1)), (3, 3, 1, 129, (129, 64, 0)), (2, 4, 4, 65, None), (1, 14, 2, 200, (150,)))


def _one_key_bounds(qkv, go, hq, hkv, d):
    """l = 1 (test_gpu_gqa_kernels._one_key_bounds at head dim d): the one probability is 1, so dq and dk are exactly 0 in the
    reference.  The kernels form dS = P (dP - delta) with dP = dO . v and delta = dO . O, O = v: two fp32 evaluations of ONE
    d-term dot product, each within (d + 2) u sum |dO_i v_i| of it.  The bf16 kernels carry delta into the MFMA as two bf16
    numbers (hi + lo), which leaves up to 2^-18 |delta| = 64 u |delta| behind, and round dS and the result to bf16 (1 + 2^-7
    covers both).  Then dq = scale dS k and dk = scale sum over the query heads of the group of dS q."""
    b, bf = qkv.shape[0], qkv.dtype == BF
    q, k, v = (t.double().reshape(b, -1, d) for t in _split(qkv, hq, hkv, d))
    rep, scale = hq // hkv, d ** -0.5
    ds = (2 * (d + 2) + 64 * bf) * U * (1 + 2.0 ** -7 * bf) * (go.double().reshape(b, hq, d).abs() * v.abs().repeat_interleave(rep, 1)).sum(-1)
    dq = scale * ds[..., None] * k.abs().repeat_interleave(rep, 1)
    dk = scale * (ds[..., None] * q.abs()).view(b, hkv, rep, d).sum(2)
    return {"dq": dq.view(b, 1, hq * d), "dk": dk.view(b, 1, hkv * d)}


@lru_cache(maxsize=None)
def _padded_problem(dev, dtype, d, case):
    b, hq, hkv, l, kv = case
    qkv, go = _qkv_go(dev, dtype, (b, l), hq, hkv, d, 101 + 7 * l + hq + d)
    kv_len = None if kv is None else torch.tensor(kv, dtype=torch.int32, device=dev)
    ref = _reference(qkv, go, torch.full((b,), l, device=dev) if kv is None else kv_len, hq, hkv, d)
    return qkv, go, kv_len, ref


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp32"])
@pytest.mark.parametrize("d", HEAD_DIMS)
@pytest.mark.parametrize("case", PADDED, ids=["one_row", "group3_l33", "l129_kv_edges_empty", "mha_l65", "group7_l200_kv150"])
def test_bidir_gqa_padded(dev, case, d, dtype):
    from gmlm_amd import ops
    b, hq, hkv, l, kv = case
    qkv, go, kv_len, ref = _padded_problem(dev, dtype, d, case)
    got = _op_run(qkv, go, hq, hkv, d, lambda q, k, v: ops.bidir_gqa_attention(q, k, v, kv_len, hq, hkv, d ** -0.5, d))
    if l == 1:
        zero = _one_key_bounds(qkv, go, hq, hkv, d)
        for name, g_, r_ in zip(NAMES, got, ref):
            if name in zero:
                assert float(r_.abs().max()) == 0.0
                ratio = g_.double().abs() / zero[name]
                print(f"  {name} (reference 0): max |got| / bound = {float(ratio.max()):.3f}")
                assert bool((ratio <= 1).all()), (name, float(ratio.max()))
            else:
                _close(name, g_, r_, *_budget(dtype, name))
        return
    _check(dtype, got, ref)
    if kv is None:
        return
    valid = (torch.arange(l, device=dev)[None, :] < kv_len[:, None])[..., None]             # [b, l, 1]
    for name, g_, r_ in zip(("dk", "dv"), got[2:], ref[2:]):
        assert float((r_ * ~valid).abs().max()) == 0.0
        assert float((g_ * ~valid).abs().max()) == 0.0, f"{name} of a key at or past kv_len is not zero"
    if any(0 < n < l for n in kv):                     # query rows past kv_len are still computed: held to the reference apart
        assert float((ref[0] * ~valid).abs().max()) > 0
        for name, g_, r_ in zip(("out", "dq"), got, ref):
            if float((r_ * ~valid).abs().max()) > 0:   # (kv_len = 1: one key, dq = 0; the whole-tensor check above holds it)
                _close(name + " of rows >= kv_len", g_ * ~valid, r_ * ~valid, *_budget(dtype, name))
    if 0 in kv:                                        # an empty sequence: zeros, lse = -inf, zero gradients
        e = kv.index(0)
        for name, g_ in zip(NAMES, got):
            assert float(g_[e].abs().max()) == 0.0, f"{name}: a sequence without keys is not zero"
        q, k, v = _split(qkv, hq, hkv, d)
        lse = ops._causal_fwd(q, k, v, kv_len, hq, hkv, d ** -0.5, False, d, True)[2]
        assert bool((lse[e] == float("-inf")).all()) and bool(torch.isfinite(lse[[i for i in range(b) if i != e]]).all())


# ---------------------------------------------------------------------------------------------------------------- packed
PACKED = (((1, 31, 0, 33, 64, 65, 127, 128, 129), 6, 2), ((5, 130), 2, 1))


def _packed_reference(qkv, go, lens, hq, hkv, d):
    """One sequence at a time through the padded reference; [T, .] results."""
    outs, r0 = [[], [], [], []], 0
    for n in lens:
        if n:
            r = _reference(qkv[None, r0:r0 + n], go[None, r0:r0 + n], torch.tensor([n], device=qkv.device), hq, hkv, d)
            for acc, t in zip(outs, r):
                acc.append(t[0])
        r0 += n
    return tuple(torch.cat(a) for a in outs)


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp32"])
@pytest.mark.parametrize("d", HEAD_DIMS)
@pytest.mark.parametrize("lens,hq,hkv", PACKED, ids=["nine_seqs_group3", "two_seqs_group2"])
def test_bidir_gqa_packed(dev, lens, hq, hkv, d, dtype):
    from gmlm_amd import ops
    qkv, go = _qkv_go(dev, dtype, (sum(lens),), hq, hkv, d, 211 + len(lens) + d)
    cu = torch.tensor((0,) + lens, dtype=torch.int64).cumsum(0).to(dev, torch.int32)
    got = _op_run(qkv, go, hq, hkv, d,
                  lambda q, k, v: ops.bidir_gqa_attention_varlen(q, k, v, cu, max(lens), hq, hkv, d ** -0.5, d))
    _check(dtype, got, _packed_reference(qkv, go, lens, hq, hkv, d))


# ------------------------------------------------------------------------------------------- the node the encoder uses
def _rope_table(rows, d, dev):
    inv = 1.0 / (1e4 ** (torch.arange(0, d, 2, dtype=torch.float) / d))
    fr = torch.arange(rows, dtype=torch.float32)[:, None] * inv[None]
    return torch.stack([fr.cos(), fr.sin()], 1).contiguous().to(dev)


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp32"])
@pytest.mark.parametrize("d", HEAD_DIMS)
@pytest.mark.parametrize("packed", [False, True], ids=["padded", "packed"])
def test_fused_rope_bidir_node(dev, packed, d, dtype):
    """ops.rope_bidir_gqa / _varlen: q, k and v are views of ONE fused [.., (hq + 2 hkv) d] buffer, the gradients land in ONE
    dqkv.  The rotation leaves the V columns alone; the context is held to float64 attention on the rotated buffer; context and
    fused input gradient equal, bit for bit, ops.rope_heads_ followed by ops.bidir_gqa_attention(_varlen) on views of the same
    buffer and the inverse rotation, which the cases above hold to float64."""
    from gmlm_amd import ops
    hq, hkv, scale = 4, 2, d ** -0.5
    nq, nk = hq * d, hkv * d
    lens = (1, 33, 129, 64)
    cs = _rope_table(140, d, dev)
    if packed:
        cu = torch.tensor((0,) + lens, dtype=torch.int64).cumsum(0).to(dev, torch.int32)
        pos = torch.cat([torch.arange(n) for n in lens]).to(dev)
        lead = (sum(lens),)
    else:
        kv_len = torch.tensor(lens, dtype=torch.int32, device=dev)
        lead = (len(lens), max(lens))
    qkv, go = _qkv_go(dev, dtype, lead, hq, hkv, d, 29 + d)
    rope = lambda t, inverse=False: ops.rope_heads_(t, cs, hq + hkv, d, 0 if packed else lead[1], pos.to(torch.int32) if packed else None,
                                                    inverse=inverse)

    def run(fused):
        x = qkv.clone().requires_grad_(True)
        if fused:
            y = x * 1.0                                             # a non-leaf buffer of this graph, as the QKV GEMM's output is
            out = ops.rope_bidir_gqa_varlen(y, cs, pos, cu, max(lens), hq, hkv, d, scale) if packed else \
                ops.rope_bidir_gqa(y, cs, kv_len, hq, hkv, d, scale)
            out.backward(go)
            return out.detach(), x.grad, y.detach()
        r = rope(qkv.clone()).requires_grad_(True)
        q, k, v = _split(r, hq, hkv, d)
        out = ops.bidir_gqa_attention_varlen(q, k, v, cu, max(lens), hq, hkv, scale, d) if packed else \
            ops.bidir_gqa_attention(q, k, v, kv_len, hq, hkv, scale, d)
        out.backward(go)
        return out.detach(), rope(r.grad.clone(), inverse=True), r.detach()

    box = {}
    ran = kernels_run(lambda: box.setdefault("r", run(True)))
    rope_k = {f"gqa::rope_heads_kernel<{TN[dtype]}, {d}, {inv}>" for inv in ("false", "true")}
    assert {n for n in ran if n.startswith(("gqa::", "bidir::", "causal128::"))} == rope_k | set(bidir_kernels(dtype, d)), sorted(ran)
    assert not any(n.startswith(("qknorm_rope_", "attn_", "d128::", "mbert::")) for n in ran), ran
    assert _same_bits(run(True), box["r"])
    out, dqkv, rotated = box["r"]
    assert torch.equal(rotated[..., nq + nk:], qkv[..., nq + nk:]), "V columns changed by the rotation"
    assert not torch.equal(rotated[..., :nq + nk], qkv[..., :nq + nk])
    for name, a, r_ in zip(("out", "dqkv", "rotated qkv"), box["r"], run(False)):
        assert bool(torch.isfinite(a).all()) and float(a.abs().max()) > 0, name
        assert torch.equal(a, r_), name
    if packed:
        ref = _packed_reference(rotated, go, lens, hq, hkv, d)[0]
    else:
        ref = _reference(rotated, go, kv_len, hq, hkv, d)[0]
    _close("out", out, ref, *_budget(dtype, "out"))
