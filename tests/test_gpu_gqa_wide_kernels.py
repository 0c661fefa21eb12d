"""The grouped-KV attention kernels at head dim 256 (gmlm_attention_gqa_d256_*, csrc/attn_gqa_wide.hip, namespace gqaw::) through
``ops.gqa_d256_attention`` / ``_varlen`` against dense float64 attention on the same rounded inputs, forward and backward.

The checker is helpers._dense_reference's computation with two additions the helper lacks, the causal mask and the KV head of a
query head (``_reference``: K / V repeated over the group under autograd, so dK / dV are the sums over the group's query
heads); ``test_the_reference_is_the_dense_reference_on_expanded_kv`` ties it to the helper itself.  The budgets are those of
tests/test_gpu_attention_wide.py, imported unchanged (the same head dim, the same rounding points): fp32 1e-4 max / 1e-5
relative L2; bf16 2e-2 max, 6e-3 relative L2 for out and dv, 8e-3 for dq and dk.  Every case prints measured error beside its
budget.

Edges.  The kernels have ONE tile height: 32 query rows per workgroup and 32 keys per tile (R = KT = 32), every wave of a
workgroup on the same rows, so there is no wave boundary inside a tile; key tile t is the diagonal tile of query tile t.
Sequence lengths 1, 31, 32, 33 (one row; one short of, exactly and one past the first tile / workgroup: the causal loop is the
diagonal tile alone, then one tile below it), 63, 64, 65 (the second tile edge: two workgroups per (sequence, head), the dK/dV
query loop starts at tile 1 for the second key workgroup), 127, 128, 129 (the 128-row edge of the other grouped families,
which this one must NOT have) and 257 (nine tiles, one row in the last).  kv_len 0, 1 and L per length; kv_len = L + 5 and -3
clamp."""
import pytest
import torch

from helpers import _dense_reference, kernels_run
from test_gpu_attention_wide import _budget

pytestmark = pytest.mark.gpu

D = 256
HEADS = ((3, 1), (4, 1), (4, 2))
LENS = (1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 257)
DTYPES = (torch.float32, torch.bfloat16)
TN = {torch.bfloat16: "unsigned short", torch.float32: "float"}
PAD = 8                                   # the fused rows are 8 elements wider than [q | k | v]
SCALE = 1.0 / 12.0                        # not d ** -0.5 = 1 / 16: the scale is an argument


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _close(name, got, ref, max_rel, l2_rel):
    e = got.double() - ref
    mx, l2 = float(e.abs().max()) / float(ref.abs().max()), float(e.norm()) / float(ref.norm())
    print(f"  {name}: max|err| / max|ref| = {mx:.2e} (budget {max_rel:.0e}), l2 rel = {l2:.2e} (budget {l2_rel:.0e})")
    assert mx <= max_rel and l2 <= l2_rel, (name, mx, l2)


def _reference(q, k, v, go, seqs, hq, hkv, scale, causal):
    """q, go [R, hq * D], k, v [R, hkv * D] flattened rows; seqs = [(first row, rows, valid keys)] -> out, dq, dk, dv in float64.
    Query i of a sequence sees the keys below ``valid`` (causal: at or before i); no valid key: zeros."""
    outs = [torch.zeros(t.shape, dtype=torch.float64, device=q.device) for t in (q, q, k, v)]
    g = hq // hkv
    for r0, n, kv in seqs:
        if n == 0 or kv == 0:
            continue
        qq = q[r0:r0 + n].double().reshape(n, hq, D).transpose(0, 1).contiguous().requires_grad_(True)
        kk = k[r0:r0 + kv].double().reshape(kv, hkv, D).transpose(0, 1).contiguous().requires_grad_(True)
        vv = v[r0:r0 + kv].double().reshape(kv, hkv, D).transpose(0, 1).contiguous().requires_grad_(True)
        s = (qq @ kk.repeat_interleave(g, 0).transpose(1, 2)) * scale
        if causal:
            s = s.masked_fill(torch.arange(kv, device=q.device)[None, :] > torch.arange(n, device=q.device)[:, None], float("-inf"))
        o = torch.softmax(s, -1) @ vv.repeat_interleave(g, 0)
        o.backward(go[r0:r0 + n].double().reshape(n, hq, D).transpose(0, 1))
        back = lambda t: t.transpose(0, 1).reshape(t.shape[1], -1)
        outs[0][r0:r0 + n], outs[1][r0:r0 + n] = back(o.detach()), back(qq.grad)
        outs[2][r0:r0 + kv], outs[3][r0:r0 + kv] = back(kk.grad), back(vv.grad)
    return outs


def _fused(dev, dtype, rows_shape, hq, hkv, seed):
    """One fused [.., (hq + 2 hkv) * D + PAD] buffer (K scaled so that scores are neither flat nor one-hot) and dO."""
    g = torch.Generator().manual_seed(seed)
    w = (hq + 2 * hkv) * D
    buf = torch.randn(*rows_shape, w + PAD, generator=g)
    buf[..., hq * D:(hq + hkv) * D] *= 1.5
    go = torch.randn(*rows_shape, hq * D, generator=g)
    return buf.to(dev, dtype), go.to(dev, dtype)


def _slices(buf, hq, hkv):
    nq, nk = hq * D, hkv * D
    return buf[..., :nq], buf[..., nq:nq + nk], buf[..., nq + nk:nq + 2 * nk]


def _kernel_sets(dtype, causal):
    t, c = TN[dtype], "true" if causal else "false"
    return ({f"gqaw::fwd_kernel<{t}, {c}>"}, {f"gqaw::delta_kernel<{t}>", f"gqaw::dq_kernel<{t}, {c}>", f"gqaw::dkv_kernel<{t}, {c}>"})


def _run(buf, go, hq, hkv, causal, kv_len=None, cu=None, max_len=0, kernels=False):
    """Through the operator on slices of the fused buffer -> out, lse, dq, dk, dv (the three gradients as slices of buf.grad)."""
    from gmlm_amd import ops
    leaf = buf.clone().requires_grad_(True)
    q, k, v = _slices(leaf, hq, hkv)
    assert q.stride(-2) == (hq + 2 * hkv) * D + PAD
    if cu is None:
        fwd = lambda: ops.gqa_d256_attention(q, k, v, kv_len, hq, hkv, SCALE, causal)
    else:
        fwd = lambda: ops.gqa_d256_attention_varlen(q, k, v, cu, max_len, hq, hkv, SCALE, causal)
    if kernels:
        box = {}
        fwd_k = kernels_run(lambda: box.setdefault("o", fwd()))
        out = box["o"]
        lse = out.grad_fn.saved_tensors[4]                            # before the backward frees what the node saved
        bwd_k = kernels_run(lambda: out.backward(go))
        assert (fwd_k, bwd_k) == _kernel_sets(buf.dtype, causal), (sorted(fwd_k), sorted(bwd_k))
    else:
        out = fwd()
        lse = out.grad_fn.saved_tensors[4]
        out.backward(go)
    assert float(leaf.grad[..., (hq + 2 * hkv) * D:].abs().max()) == 0.0           # the padding columns get no gradient
    return (out.detach(), lse) + tuple(t.clone() for t in _slices(leaf.grad, hq, hkv))


def _check(tag, dtype, got, ref, one_key_bound):
    print(f"\n{tag}:")
    for name, a, r, grad in (("out", got[0], ref[0], False), ("dq", got[2], ref[1], True), ("dk", got[3], ref[2], True),
                             ("dv", got[4], ref[3], False)):
        assert bool(torch.isfinite(a).all()), name
        if float(r.abs().max()) == 0.0:
            # one key everywhere: P = 1 and dS = P (dP - delta) = 0 in exact arithmetic; delta = rowsum(dO * O) and dP agree to
            # rounding only (the rule of tests/test_gpu_attention_wide.py); no key at all: exact zeros
            bound = one_key_bound * _budget(dtype, grad)[0]
            print(f"  {name}: max|got| = {float(a.abs().max()):.2e} (true value 0, bound {bound:.1e})")
            assert float(a.abs().max()) <= bound, name
            continue
        _close(name, a, r, *_budget(dtype, grad))


def _flat(t):
    return t.reshape(-1, t.shape[-1])


@pytest.mark.parametrize("dtype", DTYPES, ids=("fp32", "bf16"))
@pytest.mark.parametrize("causal", [False, True], ids=("bidir", "causal"))
@pytest.mark.parametrize("hq,hkv", HEADS)
def test_padded_lengths_and_kv_len_vs_dense_fp64(dev, hq, hkv, causal, dtype):
    """Per length L of ``LENS``: four sequences with kv_len L, 1, 0 and L + 5 (clamped to L).  Rows at or past kv_len are
    computed as queries; keys there get exactly zero gradients; kv_len 0 gives zeros and lse = -inf."""
    for L in LENS:
        buf, go = _fused(dev, dtype, (4, L), hq, hkv, 100 * L + hq + hkv)
        kv = [L, 1, 0, L + 5]
        kv_len = torch.tensor(kv, dtype=torch.int32, device=dev)
        got = _run(buf, go, hq, hkv, causal, kv_len=kv_len, kernels=L in (33, 257))
        q, k, v = (_flat(t) for t in _slices(buf, hq, hkv))
        seqs = [(i * L, L, min(max(n, 0), L)) for i, n in enumerate(kv)]
        ref = _reference(q, k, v, _flat(go), seqs, hq, hkv, SCALE, causal)
        bound = float(v.double().abs().max()) * float(go.double().abs().max()) * float(k.double().abs().max() + q.double().abs().max())
        _check(f"padded L={L} {hq}/{hkv} causal={causal} {dtype}", dtype, [None if t is None else _flat(t) for t in got], ref, bound)
        out, lse, dq, dk, dv = got
        valid = torch.arange(L, device=dev)[None, :] < kv_len.clamp(0, L)[:, None]
        assert float(dk[~valid].abs().max() if (~valid).any() else 0.0) == 0.0 and float(dv[~valid].abs().max() if (~valid).any() else 0.0) == 0.0
        assert float(out[2].abs().max()) == 0.0 and float(dq[2].abs().max()) == 0.0 and bool((lse[2] == float("-inf")).all())
        assert bool(torch.isfinite(lse[[0, 1, 3]]).all())
    # kv_len = L + 5 gives the bits of kv_len = L on the same data; kv_len = -3 those of 0
    L = 65
    buf, go = _fused(dev, dtype, (1, L), hq, hkv, 7)
    two, gtwo = buf.expand(4, L, -1).contiguous(), go.expand(4, L, -1).contiguous()
    got = _run(two, gtwo, hq, hkv, causal, kv_len=torch.tensor([L, L + 5, 0, -3], dtype=torch.int32, device=dev))
    for t in (got[0], got[2], got[3], got[4]):
        assert torch.equal(t[0], t[1]) and torch.equal(t[2], t[3]) and float(t[0].abs().max()) > 0


@pytest.mark.parametrize("dtype", DTYPES, ids=("fp32", "bf16"))
@pytest.mark.parametrize("causal", [False, True], ids=("bidir", "causal"))
@pytest.mark.parametrize("hq,hkv", HEADS)
def test_packed_lengths_vs_dense_fp64(dev, hq, hkv, causal, dtype):
    """All of ``LENS`` (and an empty sequence between them) back to back in one packed call, max_len = 257; then the same rows
    as the padded call of one sequence each give the same bytes."""
    lens = list(LENS[:4]) + [0] + list(LENS[4:])
    cu = torch.tensor([0] + lens).cumsum(0).to(dev, torch.int32)
    total = sum(lens)
    buf, go = _fused(dev, dtype, (total,), hq, hkv, 31 + hq + hkv)
    got = _run(buf, go, hq, hkv, causal, cu=cu, max_len=max(lens), kernels=True)
    q, k, v = _slices(buf, hq, hkv)
    seqs = [(int(cu[i]), n, n) for i, n in enumerate(lens)]
    ref = _reference(q, k, v, go, seqs, hq, hkv, SCALE, causal)
    _check(f"packed {hq}/{hkv} causal={causal} {dtype}", dtype, got, ref, 0.0)
    assert tuple(got[1].shape) == (hq, total) and bool(torch.isfinite(got[1]).all())
    for i in (0, 3, 7):                                              # lengths 1, 33 and 65 alone, padded layout
        r0, n = int(cu[i]), lens[i]
        one = _run(buf[r0:r0 + n][None], go[r0:r0 + n][None], hq, hkv, causal)
        for name, a, b_ in zip(("out", "dq", "dk", "dv"), (got[0], got[2], got[3], got[4]), (one[0], one[2], one[3], one[4])):
            assert torch.equal(a[r0:r0 + n], b_[0]), (name, n)
        assert torch.equal(got[1][:, r0:r0 + n], one[1][0])


@pytest.mark.parametrize("dtype", DTYPES, ids=("fp32", "bf16"))
def test_the_reference_is_the_dense_reference_on_expanded_kv(dev, dtype):
    """``_reference`` without the causal mask against helpers._dense_reference fed K / V expanded to hq heads, its dK / dV
    folded over the group; and a causal row i of ``_reference`` is the bidirectional row of the sequence cut after key i."""
    hq, hkv, L, b = 4, 2, 45, 3
    buf, go = _fused(dev, dtype, (b, L), hq, hkv, 5)
    q, k, v = _slices(buf, hq, hkv)
    kv = [L, 13, 0]
    mine = _reference(_flat(q), _flat(k), _flat(v), _flat(go), [(i * L, L, n) for i, n in enumerate(kv)], hq, hkv, SCALE, False)
    expand = lambda t: t.reshape(b, L, hkv, 1, D).expand(b, L, hkv, hq // hkv, D).reshape(b, L, hq * D)
    theirs = _dense_reference(q, expand(k), expand(v), go, hq, SCALE, torch.tensor(kv))
    fold = lambda t: t.reshape(b, L, hkv, hq // hkv, D).sum(3).reshape(b * L, hkv * D)
    for a, r in zip(mine, (_flat(theirs[0]), _flat(theirs[1]), fold(theirs[2]), fold(theirs[3]))):
        assert float((a - r).abs().max()) <= 1e-12 * max(1.0, float(r.abs().max()))
    i = 20
    cz = _reference(_flat(q), _flat(k), _flat(v), _flat(go), [(0, L, L)], hq, hkv, SCALE, True)[0][i]
    bz = _reference(_flat(q), _flat(k), _flat(v), _flat(go), [(0, i + 1, i + 1)], hq, hkv, SCALE, False)[0][i]
    assert float((cz - bz).abs().max()) <= 1e-12


@pytest.mark.parametrize("dtype", DTYPES, ids=("fp32", "bf16"))
@pytest.mark.parametrize("causal", [False, True], ids=("bidir", "causal"))
def test_repeated_call_gives_identical_bytes(dev, causal, dtype):
    hq, hkv, L = 4, 2, 129
    buf, go = _fused(dev, dtype, (3, L), hq, hkv, 11)
    kv_len = torch.tensor([L, 40, 97], dtype=torch.int32, device=dev)
    a = _run(buf, go, hq, hkv, causal, kv_len=kv_len)
    c = _run(buf, go, hq, hkv, causal, kv_len=kv_len)
    for name, x, y in zip(("out", "lse", "dq", "dk", "dv"), a, c):
        assert torch.equal(x.view(torch.int16 if x.element_size() == 2 else torch.int32),
                           y.view(torch.int16 if y.element_size() == 2 else torch.int32)), name


@pytest.mark.parametrize("dtype", DTYPES, ids=("fp32", "bf16"))
def test_group_of_one_bidirectional_padded_is_the_plain_body(dev, dtype):
    """gqaw:: and wide:: are one body (csrc/attn_wide.hpp).  With one query head per KV head, no causal mask, the padded layout
    and p = 0, what GROUPED adds is h / 1, a group loop of one turn and an early return no tile takes: the same expressions in
    the same order as wide:: at d = 256, so ``ops.gqa_d256_attention`` and ``ops.Attention`` give the same bytes on the same
    contiguous q, k, v, dO.  L = 31, 33, 65 (one short of and one past a tile, two tiles and a row); per L three sequences with
    kv_len L, 1 and 0."""
    from gmlm_amd import ops
    h = 2
    for L in (31, 33, 65):
        g = torch.Generator().manual_seed(900 + L)
        q, k, v, go = (torch.randn(3, L, h * D, generator=g).to(dev, dtype) for _ in range(4))
        kv_len = torch.tensor([L, 1, 0], dtype=torch.int32, device=dev)
        got = []
        for fwd in (lambda a, b_, c: ops.gqa_d256_attention(a, b_, c, kv_len, h, h, SCALE, False),
                    lambda a, b_, c: ops.Attention.apply(a, b_, c, kv_len, h, SCALE, 0.0, 0)):
            qd, kd, vd = (t.clone().requires_grad_(True) for t in (q, k, v))
            out = fwd(qd, kd, vd)
            lse = out.grad_fn.saved_tensors[4]
            out.backward(go)
            got.append((out.detach(), lse, qd.grad, kd.grad, vd.grad))
        assert float(got[0][0][0].abs().max()) > 0 and float(got[0][3][0].abs().max()) > 0
        for name, a, b_ in zip(("out", "lse", "dq", "dk", "dv"), *got):
            assert torch.equal(a, b_), (L, name, float((a.double() - b_.double()).abs().max()))


def test_every_column_slice_reaches_the_scores_exactly_once(dev):
    """fp32, 4 / 2 heads.  q is non-zero only in the columns of wave 1 of every head and k only in those of wave 2: every score is
    exactly 0, so a bidirectional output row is the mean of v, and dq is exactly zero wherever k is, dk wherever q is.  A partial
    that leaked into another wave's columns breaks the zeros."""
    from gmlm_amd import ops
    hq, hkv, n, ds = 4, 2, 70, D // 4
    g = torch.Generator().manual_seed(1)
    q, go = (torch.randn(1, n, hq, 4, ds, generator=g) for _ in range(2))
    k, v = (torch.randn(1, n, hkv, 4, ds, generator=g) for _ in range(2))
    qm, km = torch.zeros(4), torch.zeros(4)
    qm[1], km[2] = 1.0, 1.0
    qd = (q * qm[:, None]).reshape(1, n, hq * D).to(dev).requires_grad_(True)
    kd = (k * km[:, None]).reshape(1, n, hkv * D).to(dev).requires_grad_(True)
    vd = v.reshape(1, n, hkv * D).to(dev).requires_grad_(True)
    out = ops.gqa_d256_attention(qd, kd, vd, None, hq, hkv, SCALE, False)
    out.backward(go.reshape(1, n, hq * D).to(dev))
    mean_v = vd.detach().double().mean(1, keepdim=True).reshape(1, 1, hkv, 1, D).expand(1, n, hkv, hq // hkv, D).reshape(1, n, hq * D)
    _close("out vs mean(v)", out.detach(), mean_v, 1e-4, 1e-5)
    dq5, dk5 = qd.grad.reshape(1, n, hq, 4, ds), kd.grad.reshape(1, n, hkv, 4, ds)
    assert float(dq5[:, :, :, [0, 1, 3]].abs().max()) == 0.0 and float(dk5[:, :, :, [0, 2, 3]].abs().max()) == 0.0


def test_nothing_to_do_forms(dev):
    """0 sequences and 0 rows, through the operator (forward and backward) and through the C entry points with no pointer."""
    from gmlm_amd import _lib, ops
    hq, hkv = 3, 1
    for shape in ((0, 5), (2, 0)):
        q = torch.zeros(*shape, hq * D, device=dev, requires_grad=True)
        k, v = (torch.zeros(*shape, hkv * D, device=dev, requires_grad=True) for _ in range(2))
        out = ops.gqa_d256_attention(q, k, v, None, hq, hkv, SCALE, True)
        assert tuple(out.shape) == (*shape, hq * D)
        out.sum().backward()
        assert tuple(q.grad.shape) == tuple(q.shape) and tuple(k.grad.shape) == tuple(k.shape)
    for cu in ([0], [0, 0, 0]):
        q = torch.zeros(0, hq * D, device=dev, requires_grad=True)
        k, v = (torch.zeros(0, hkv * D, device=dev, requires_grad=True) for _ in range(2))
        out = ops.gqa_d256_attention_varlen(q, k, v, torch.tensor(cu, dtype=torch.int32, device=dev), 4, hq, hkv, SCALE, False)
        out.sum().backward()
        assert tuple(out.shape) == (0, hq * D) and tuple(v.grad.shape) == (0, hkv * D)
    lib = _lib.lib()
    cu = torch.zeros(3, dtype=torch.int32, device=dev)
    fwd_tail = (hq, hkv, D, 768, 256, 256, SCALE, 0.0, 1, None, None, None, _lib.F32, None)
    bwd_tail = (hq, hkv, D, 768, 256, 256, SCALE, 0.0, 1, None, None, None, 768, 256, 256, _lib.F32, None, 0, None)

    def calls():
        assert lib.gmlm_attention_gqa_d256_fwd(None, None, None, None, 0, hq, hkv, 7, 7, D, 768, 256, 256, SCALE, 0.0, 1, None, None, None,
                                               _lib.F32, None) == 0
        assert lib.gmlm_attention_gqa_d256_fwd(None, None, None, None, 2, hq, hkv, 0, 0, D, 768, 256, 256, SCALE, 0.0, 0, None, None, None,
                                               _lib.BF16, None) == 0
        assert lib.gmlm_attention_gqa_d256_bwd(None, None, None, None, None, None, None, None, 0, hq, hkv, 7, 7, D, 768, 256, 256, SCALE,
                                               0.0, 1, None, None, None, 768, 256, 256, _lib.F32, None, 0, None) == 0
        assert lib.gmlm_attention_gqa_d256_varlen_fwd(None, None, None, cu.data_ptr(), 0, 4, 0, *fwd_tail) == 0
        assert lib.gmlm_attention_gqa_d256_varlen_fwd(None, None, None, cu.data_ptr(), 2, 4, 0, *fwd_tail) == 0
        assert lib.gmlm_attention_gqa_d256_varlen_bwd(None, None, None, None, None, None, None, cu.data_ptr(), 2, 4, 0, *bwd_tail) == 0
        torch.zeros(4, device=dev).add_(1)                          # so that the profiler sees a device kernel at all

    assert kernels_run(calls) == set()


def test_refusals_return_their_status_without_a_launch(dev):
    from gmlm_amd import _lib
    lib = _lib.lib()
    hq, hkv, L = 4, 2, 8
    w = (hq + 2 * hkv) * D
    buf = torch.zeros(1, L, w, device=dev)
    out, lse, go, ws = torch.zeros(1, L, hq * D, device=dev), torch.zeros(1, hq, L, device=dev), torch.zeros(1, L, hq * D, device=dev), \
        torch.zeros(hq * L, device=dev)
    dbuf = torch.zeros_like(buf)
    base = dict(q=buf.data_ptr(), k=buf.data_ptr() + 4 * hq * D, v=buf.data_ptr() + 4 * (hq + hkv) * D, hq=hq, hkv=hkv, d=D, dropout_p=0.0)

    def call(bwd, **mut):
        a = dict(base, **mut)
        if bwd:
            rc = lib.gmlm_attention_gqa_d256_bwd(a["q"], a["k"], a["v"], out.data_ptr(), None, go.data_ptr(), lse.data_ptr(), None, 1,
                                                 a["hq"], a["hkv"], L, L, a["d"], w, w, w, SCALE, a["dropout_p"], 1, dbuf.data_ptr(),
                                                 dbuf.data_ptr() + 4 * hq * D, dbuf.data_ptr() + 4 * (hq + hkv) * D, w, w, w, _lib.F32,
                                                 ws.data_ptr(), ws.numel() * 4, None)
        else:
            rc = lib.gmlm_attention_gqa_d256_fwd(a["q"], a["k"], a["v"], None, 1, a["hq"], a["hkv"], L, L, a["d"], w, w, w, SCALE,
                                                 a["dropout_p"], 1, out.data_ptr(), None, lse.data_ptr(), _lib.F32, None)
        return rc, lib.gmlm_last_error()

    def calls():
        for bwd in (False, True):
            for mut, msg in ((dict(dropout_p=0.1), b"dropout"), (dict(d=128), b"head dim"), (dict(d=512), b"head dim"),
                             (dict(hq=3, hkv=2), b"multiple of"), (dict(q=base["q"] + 4), b"aligned"), (dict(v=base["v"] + 8), b"aligned")):
                rc, err = call(bwd, **mut)
                assert rc == -1 and msg in err, (bwd, mut, rc, err)
        rc = lib.gmlm_attention_gqa_d256_bwd(base["q"], base["k"], base["v"], out.data_ptr(), None, go.data_ptr(), lse.data_ptr(), None, 1, hq,
                                             hkv, L, L, D, w, w, w, SCALE, 0.0, 1, dbuf.data_ptr(), dbuf.data_ptr() + 4 * hq * D,
                                             dbuf.data_ptr() + 4 * (hq + hkv) * D, w, w, w, _lib.F32, ws.data_ptr(), ws.numel() * 4 - 1, None)
        assert rc == -2 and b"workspace" in lib.gmlm_last_error()
        torch.zeros(4, device=dev).add_(1)

    assert kernels_run(calls) == set()
    assert float(out.abs().max()) == 0.0 and float(dbuf.abs().max()) == 0.0
