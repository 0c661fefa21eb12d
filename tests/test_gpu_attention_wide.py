"""Oracle parity of the wide-head attention kernels (gmlm_attention_wide_*, csrc/attn_wide.hip: head dims 256 / 384 / 512, the
head dim split over the four waves of a workgroup), through ``ops.Attention`` and ``nn.attention_wide_dim``.

The checker is dense softmax attention in float64 on the same rounded inputs, forward and autograd backward
(helpers._dense_reference), with the kernels' replayable dropout hash restated in helpers.attn_dropout_scale.  The budgets
are those of test_gpu_attention_d128.py, unchanged: fp32 1e-4 max / 1e-5 relative L2; bf16 2e-2 max, 6e-3 relative L2 for
out and dv, 8e-3 for dq and dk (P and dS are rounded to bf16 before the second product, as in every streaming kernel; the
longer first contraction is accumulated in fp32).  Every case prints measured error beside its budget.

R = 32 rows per workgroup and KT = 32 rows per tile of the other operand; the shapes sit on both sides of those edges."""
import pytest
import torch

from helpers import _dense_reference, attn_dropout_scale, kernels_run

pytestmark = pytest.mark.gpu

R, KT = 32, 32
DIMS = (256, 384, 512)
DTYPES = (torch.float32, torch.bfloat16)
SEED = 0x1234_5678_9ABC


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _budget(dtype, grad):
    if dtype == torch.float32:
        return 1e-4, 1e-5
    return 2e-2, 8e-3 if grad else 6e-3


def _tn(dtype):
    return "float" if dtype == torch.float32 else "unsigned short"


def _close(name, got, ref, max_rel, l2_rel):
    e = got.double() - ref
    mx, l2 = float(e.abs().max()) / float(ref.abs().max()), float(e.norm()) / float(ref.norm())
    print(f"  {name}: max|err| / max|ref| = {mx:.2e} (budget {max_rel:.0e}), l2 rel = {l2:.2e} (budget {l2_rel:.0e})")
    assert mx <= max_rel and l2 <= l2_rel, (name, mx, l2)


def _inputs(dev, dtype, b, h, d, lq, lk, seed, fused_kv=False):
    g = torch.Generator().manual_seed(seed)
    q, go = (torch.randn(b, lq, h * d, generator=g).to(dev, dtype) for _ in range(2))
    kv = torch.randn(b, lk, 2 * h * d, generator=g)
    kv[..., :h * d] *= 1.5                                          # scores ~ N(0, 1.5): neither flat nor one-hot
    kv = kv.to(dev, dtype)
    if fused_kv:
        return q, kv, go
    return q, kv[..., :h * d].contiguous(), kv[..., h * d:].contiguous(), go


def _kernel_sets(dtype, d, p):
    t, dr = _tn(dtype), "true" if p else "false"
    return ({f"wide::fwd_kernel<{t}, {d}, {dr}>"},
            {f"wide::delta_kernel<{t}>", f"wide::dq_kernel<{t}, {d}, {dr}>", f"wide::dkv_kernel<{t}, {d}, {dr}>"})


def _run(q, k, v, go, kv_len, h, scale, p, kernels=False):
    """``kernels``: also assert the exact set of the project's kernels the forward and the backward launched"""
    from gmlm_amd import ops
    qd, kd, vd = (t.clone().requires_grad_(True) for t in (q, k, v))
    box = {}
    fwd = lambda: box.setdefault("out", ops.Attention.apply(qd, kd, vd, kv_len, h, scale, p, SEED))
    if kernels:
        fwd_k = kernels_run(fwd)
        out = box["out"]
        lse = out.grad_fn.saved_tensors[4]
        bwd_k = kernels_run(lambda: out.backward(go))
        want = _kernel_sets(q.dtype, q.shape[-1] // h, p)
        assert (fwd_k, bwd_k) == want, (sorted(fwd_k), sorted(bwd_k))
    else:
        out = fwd()
        lse = out.grad_fn.saved_tensors[4]
        out.backward(go)
    return out.detach(), lse, qd.grad, kd.grad, vd.grad


def _check(tag, dtype, got, q, k, v, go, kv_len, h, scale, p):
    b, lq, lk = q.shape[0], q.shape[1], k.shape[1]
    drop = (lambda bi, hi: attn_dropout_scale(SEED, (bi * h + hi) * lq, lq, lk, p, q.device)) if p else None
    ref = _dense_reference(q, k, v, go, h, scale, kv_len, drop)
    print(f"\n{tag}:")
    for name, a, r, grad in (("out", got[0], ref[0], False), ("dq", got[2], ref[1], True), ("dk", got[3], ref[2], True),
                             ("dv", got[4], ref[3], False)):
        if float(r.abs().max()) == 0.0:
            if lk == 1 and name in ("dq", "dk"):
                # one key: P = 1 and dS = P (dP - delta) = 0 in exact arithmetic; the kernel's delta = rowsum(dO * O) and its dP
                # agree to rounding only, so dS is the budget's fraction of |dP| ~ |dO| |V| and not a bit-exact zero
                bound = _budget(dtype, grad)[0] * float(ref[3].abs().max()) * float(k.double().abs().max() + q.double().abs().max())
                print(f"  {name}: max|got| = {float(a.abs().max()):.2e} (true value 0, bound {bound:.1e})")
                assert float(a.abs().max()) <= bound, name
            else:
                assert float(a.abs().max()) == 0.0, name
            continue
        _close(name, a, r, *_budget(dtype, grad))


@pytest.mark.parametrize("dtype", DTYPES, ids=("fp32", "bf16"))
@pytest.mark.parametrize("d", DIMS)
def test_one_sequence_at_the_row_edges_vs_dense_fp64(dev, d, dtype):
    """lq = lk in {1, R - 1, R + 1, 2R + 5}: one row, a partial workgroup, one row into the second, a ragged third."""
    h = 2
    for n in (1, R - 1, R + 1, 2 * R + 5):
        for p in (0.0, 0.3):
            q, k, v, go = _inputs(dev, dtype, 1, h, d, n, n, 1000 + n + d)
            got = _run(q, k, v, go, None, h, d ** -0.5, p, kernels=True)
            _check(f"one sequence n={n} h={h} d={d} {dtype} dropout {p}", dtype, got, q, k, v, go, None, h, d ** -0.5, p)


@pytest.mark.parametrize("dtype", DTYPES, ids=("fp32", "bf16"))
@pytest.mark.parametrize("d", DIMS)
def test_lq_differs_from_lk_at_the_tile_edges_vs_dense_fp64(dev, d, dtype):
    """lk in {KT - 1, KT, KT + 1, 3 KT + 7} with lq = 45: the key loop of the forward / dQ and the key workgroups of dK/dV end
    inside, at and behind a tile; the query loop of dK/dV ends inside its second tile."""
    h, lq = 2, R + 13
    for lk in (KT - 1, KT, KT + 1, 3 * KT + 7):
        for p in (0.0, 0.3):
            q, k, v, go = _inputs(dev, dtype, 1, h, d, lq, lk, 2000 + lk + d)
            got = _run(q, k, v, go, None, h, d ** -0.5, p, kernels=True)
            _check(f"lq={lq} lk={lk} h={h} d={d} {dtype} dropout {p}", dtype, got, q, k, v, go, None, h, d ** -0.5, p)


@pytest.mark.parametrize("dtype", DTYPES, ids=("fp32", "bf16"))
@pytest.mark.parametrize("d", DIMS)
@pytest.mark.parametrize("p", [0.0, 0.3])
def test_batch_kv_len_and_fused_kv_buffer_vs_dense_fp64(dev, d, dtype, p):
    """b = 5, h = 3; valid keys per sequence: all, none, inside the first tile, one past a tile edge, lk + 9 (counts as lk).
    K and V are the two halves of ONE [b, l, 2 h d] buffer, read in place through the row strides (what CrossAttention
    passes).  Keys past kv_len get probability 0 and a zero gradient; a sequence without a valid key gives zero output, lse =
    -inf and zero gradients."""
    from gmlm_amd import ops
    b, h, L = 5, 3, 2 * KT + 6
    kv_len = torch.tensor([L, 0, 13, KT + 1, L + 9], dtype=torch.int32)
    q, kv, go = _inputs(dev, dtype, b, h, d, L, L, 3000 + d, fused_kv=True)
    hd = h * d
    qd, kvd = q.clone().requires_grad_(True), kv.clone().requires_grad_(True)
    box = {}
    fwd_k = kernels_run(lambda: box.setdefault("out", ops.Attention.apply(qd, kvd[..., :hd], kvd[..., hd:], kv_len.to(dev), h,
                                                                          d ** -0.5, p, SEED)))
    out = box["out"]
    lse = out.grad_fn.saved_tensors[4]
    bwd_k = kernels_run(lambda: out.backward(go))
    assert (fwd_k, bwd_k) == _kernel_sets(dtype, d, p), (sorted(fwd_k), sorted(bwd_k))
    got = (out.detach(), lse, qd.grad, kvd.grad[..., :hd], kvd.grad[..., hd:])
    _check(f"b={b} L={L} h={h} d={d} {dtype} kv_len {kv_len.tolist()} dropout {p}, fused K|V", dtype, got, q, kv[..., :hd],
           kv[..., hd:], go, kv_len, h, d ** -0.5, p)
    valid = torch.arange(L, device=dev)[None, :] < kv_len.to(dev)[:, None]
    assert float(kvd.grad[~valid].abs().max()) == 0.0
    assert float(out[1].abs().max()) == 0.0 and float(qd.grad[1].abs().max()) == 0.0
    assert bool((lse[1] == float("-inf")).all()) and bool(torch.isfinite(lse[[0, 2, 3, 4]]).all())
    # lse against float64 (sequence 3: KT + 1 valid keys)
    n = KT + 1
    for hi in range(h):
        s = (q[3, :, hi * d:(hi + 1) * d].double() @ kv[3, :n, hi * d:(hi + 1) * d].double().t()) * d ** -0.5
        # fp32 scores of |value| < 10 through v_exp_f32 / v_log_f32 (1 ulp each) and a 33-term sum: a few 1e-6; 1e-4 is generous
        assert float((lse[3, hi].double() - torch.logsumexp(s, -1)).abs().max()) <= 1e-4


@pytest.mark.parametrize("dtype", DTYPES, ids=("fp32", "bf16"))
@pytest.mark.parametrize("d", DIMS)
def test_keep_rate_of_the_in_kernel_dropout(dev, d, dtype):
    """The kernel's own keep rate (test_gpu_attention_d128._check_keep_rate at this head dim): with q = 0 every probability is
    1/n, and with v = 1 each output element is the kept fraction of its row times the keep scale.  Compared row by row with
    the restated mask (which does not depend on the head dim) and on average with 1 - p."""
    from gmlm_amd import ops
    n, h, p_drop = 640, 2, 0.3
    th = round(p_drop * 256)
    ks = 256.0 / (256 - th)
    q = torch.zeros(1, n, h * d, device=dev, dtype=dtype)
    k = torch.randn(1, n, h * d, device=dev).to(dtype)
    v = torch.ones(1, n, h * d, device=dev, dtype=dtype)
    out = ops.Attention.apply(q, k, v, None, h, d ** -0.5, p_drop, SEED)
    kept_all = out[0].double().reshape(n, h, d) / ks
    assert float((kept_all - kept_all[..., :1]).abs().max()) == 0.0     # every column (all four waves' slices) saw the same mask
    kept = kept_all[..., 0]                                             # [n, h]: kept fraction of each row
    want = torch.stack([(attn_dropout_scale(SEED, hi * n, n, n, p_drop, dev) > 0).double().mean(1) for hi in range(h)], 1)
    tol = 1e-5 if dtype == torch.float32 else 4e-3
    worst = float((kept - want).abs().max())
    print(f"\nkeep rate d={d} {dtype}: rows differ from the restated mask by {worst:.2e} (budget {tol:.0e}), mean {float(kept.mean()):.4f}"
          f" vs {1 - th / 256:.4f}")
    assert worst <= tol
    assert abs(float(kept.mean()) - (1 - th / 256)) < 2e-3


@pytest.mark.parametrize("d", DIMS)
def test_every_column_slice_reaches_the_scores_exactly_once(dev, d):
    """fp32.  (1) q is non-zero only in the columns of slice 1 of every head and k only in those of slice 2: every score is
    exactly 0, so the output is uniform attention (the mean of v) and lse = log lk; dq is exactly zero wherever k is (its own
    support included) and dk wherever q is.  A partial that leaked into another wave's columns breaks the zeros.
    (2) all four slices non-zero with magnitudes 1, 2, 3, 4 against float64: a dropped or doubled partial changes the scores
    by a whole slice's contribution."""
    h, n, ds = 2, 2 * R + 5, d // 4
    g = torch.Generator().manual_seed(d)
    q, k, v, go = (torch.randn(1, n, h, 4, ds, generator=g) for _ in range(4))
    qm, km = torch.zeros(4), torch.zeros(4)
    qm[1], km[2] = 1.0, 1.0
    q1, k1 = q * qm[:, None], k * km[:, None]
    flat = lambda t: t.reshape(1, n, h * d).to(dev)
    out, lse, dq, dk, dv = _run(flat(q1), flat(k1), flat(v), flat(go), None, h, d ** -0.5, 0.0)
    mean_v = flat(v).double().mean(1, keepdim=True).expand(1, n, h * d)
    print(f"\nslice test d={d}:")
    _close("out vs mean(v)", out, mean_v, 1e-4, 1e-5)
    assert float((lse.double() - torch.log(torch.tensor(float(n)))).abs().max()) <= 1e-5
    dq5, dk5 = dq.reshape(1, n, h, 4, ds), dk.reshape(1, n, h, 4, ds)
    assert float(dq5[:, :, :, [0, 1, 3]].abs().max()) == 0.0 and float(dk5[:, :, :, [0, 2, 3]].abs().max()) == 0.0
    _check(f"disjoint slices d={d}", torch.float32, (out, lse, dq, dk, dv), flat(q1), flat(k1), flat(v), flat(go), None, h, d ** -0.5, 0.0)
    mag = torch.tensor([1.0, 2.0, 3.0, 4.0])[:, None]
    q2, k2 = flat(q * mag), flat(k * mag / 4)
    got = _run(q2, k2, flat(v), flat(go), None, h, d ** -0.5, 0.0)
    _check(f"slice magnitudes 1..4 d={d}", torch.float32, got, q2, k2, flat(v), flat(go), None, h, d ** -0.5, 0.0)


@pytest.mark.parametrize("dtype", DTYPES, ids=("fp32", "bf16"))
@pytest.mark.parametrize("d", DIMS)
def test_repeated_call_gives_identical_bytes(dev, d, dtype):
    b, h, lq, lk = 2, 3, 2 * R + 5, 3 * KT + 7
    q, k, v, go = _inputs(dev, dtype, b, h, d, lq, lk, 4000 + d)
    kv_len = torch.tensor([lk, KT + 3], dtype=torch.int32, device=dev)
    a = _run(q, k, v, go, kv_len, h, d ** -0.5, 0.3)
    c = _run(q, k, v, go, kv_len, h, d ** -0.5, 0.3)
    for name, x, y in zip(("out", "lse", "dq", "dk", "dv"), a, c):
        assert torch.equal(x.view(torch.int16 if x.element_size() == 2 else torch.int32),
                           y.view(torch.int16 if y.element_size() == 2 else torch.int32)), name


@pytest.mark.parametrize("dtype", DTYPES, ids=("fp32", "bf16"))
def test_attention_wide_dim_at_320_is_the_384_run_on_zero_padded_heads(dev, dtype):
    """Head dim 320 (Qwen3-Embedding-4B: 2,560 / 8) runs on the d = 384 kernels through zero padding: bit for bit the run on
    explicitly padded operands, and within the budgets of float64 attention at the true head dim."""
    import torch.nn.functional as F
    from gmlm_amd import nn as gnn, ops
    h, d, dp, n = 2, 320, 384, 2 * R + 5
    q, k, v, go = _inputs(dev, dtype, 1, h, d, n, n, 320)
    scale = d ** -0.5
    qd, kd, vd = (t.clone().requires_grad_(True) for t in (q, k, v))
    ran = kernels_run(lambda: gnn.attention_wide_dim(qd, kd, vd, None, h, scale, 0.3, True).backward(go))
    assert any(x.startswith("wide::fwd_kernel") and ", 384, true>" in x for x in ran), sorted(ran)
    for t in (qd, kd, vd):
        t.grad = None
    seeds = iter([SEED, SEED])
    orig = ops.draw_seed
    ops.draw_seed = lambda: next(seeds)
    try:
        out = gnn.attention_wide_dim(qd, kd, vd, None, h, scale, 0.3, True)
        out.backward(go)
        pad = lambda t: F.pad(t.reshape(1, n, h, d), (0, dp - d)).reshape(1, n, h * dp)
        cut = lambda t: t.reshape(1, n, h, dp)[..., :d].reshape(1, n, h * d)
        qp, kp, vp = (pad(t).clone().requires_grad_(True) for t in (q, k, v))
        outp = ops.attention(qp, kp, vp, None, h, scale, 0.3, True)
        outp.backward(pad(go))
    finally:
        ops.draw_seed = orig
    for name, a, bb in (("out", out.detach(), cut(outp.detach())), ("dq", qd.grad, cut(qp.grad)), ("dk", kd.grad, cut(kp.grad)),
                        ("dv", vd.grad, cut(vp.grad))):
        assert torch.equal(a, bb), name
    for t in (qp, kp, vp):                                        # the padding columns receive no gradient
        assert float(t.grad.reshape(1, n, h, dp)[..., d:].abs().max()) == 0.0
    _check(f"d=320 padded to 384 {dtype} dropout 0.3", dtype, (out.detach(), None, qd.grad, kd.grad, vd.grad), q, k, v, go, None, h,
           scale, 0.3)
