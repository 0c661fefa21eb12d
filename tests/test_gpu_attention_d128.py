"""Oracle parity of the head-dim-128 attention kernels (gmlm_attention_d128_*, csrc/attn_d128.hip), through ``ops.Attention``
(the dispatch every d = 128 caller takes):

* CrossAttention geometry over a 1024-wide text encoder (main.py:159-163 with 8 heads x 128): one sequence of N nodes, with
  and without probability dropout (the kernels' replayable hash, restated in tests/helpers.py);
* padded self-attention with a per-sequence key length (the BERT padded path and the HF attention-interface drop-in at head
  dims 97-128), kv_len = 0 and ragged tails included, with and without dropout.

The checker is dense softmax attention in float64 on the same rounded inputs, forward and autograd backward.  bf16 budgets
are those of test_gpu_attention_shapes.py (the kernels round P and dS to bf16 before the second product); fp32 runs the
exact-fp32 MFMA path and must agree to 1e-5 (relative L2)."""
import pytest
import torch

from helpers import attn_dropout_scale

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _close(name, got, ref, max_rel, l2_rel):
    got = got.double()
    e = got - ref
    mx, l2 = float(e.abs().max()) / float(ref.abs().max()), float(e.norm()) / float(ref.norm())
    print(f"  {name}: max|err| / max|ref| = {mx:.2e}, l2 rel = {l2:.2e}")
    assert mx <= max_rel and l2 <= l2_rel, (name, mx, l2)


def _budget(dtype, grad):
    if dtype == torch.float32:
        return 1e-4, 1e-5
    return 2e-2, 8e-3 if grad else 6e-3


@pytest.mark.parametrize("dtype,n", [(torch.bfloat16, 183), (torch.bfloat16, 2277), (torch.bfloat16, 5201),
                                     (torch.float32, 183), (torch.float32, 2277)])
@pytest.mark.parametrize("p_drop", [0.0, 0.3])
def test_cross_attention_d128_vs_dense_fp64(dev, dtype, n, p_drop):
    from gmlm_amd import ops
    h, d = 8, 128
    g = torch.Generator().manual_seed(128 + n)
    q, k, v, go = (torch.randn(1, n, h * d, generator=g).to(dev, dtype) for _ in range(4))
    k = (k.float() * 1.5).to(dtype)                               # scores ~ N(0, 1.5): neither flat nor one-hot
    seed = 0x1234_5678_9ABC
    scale = d ** -0.5
    qd, kd, vd = (t.clone().requires_grad_(True) for t in (q, k, v))
    out = ops.Attention.apply(qd, kd, vd, None, h, scale, p_drop, seed)
    out.backward(go)
    outs = [torch.zeros(n, h * d, dtype=torch.float64, device=dev) for _ in range(4)]
    for hi in range(h):
        sl = slice(hi * d, (hi + 1) * d)
        qq, kk, vv = (t[0, :, sl].double().requires_grad_(True) for t in (q, k, v))
        pr = torch.softmax((qq @ kk.t()) * scale, -1)
        if p_drop:
            pr = pr * attn_dropout_scale(seed, hi * n, n, n, p_drop, dev)     # slab = (batch * heads + head) * lq
        o = pr @ vv
        o.backward(go[0, :, sl].double())
        outs[0][:, sl], outs[1][:, sl], outs[2][:, sl], outs[3][:, sl] = o.detach(), qq.grad, kk.grad, vv.grad
        del pr, o
    print(f"\ncross-attention h=8 d=128 N={n} {dtype}, dropout {p_drop}:")
    _close("out", out.detach()[0], outs[0], *_budget(dtype, False))
    _close("dq", qd.grad[0], outs[1], *_budget(dtype, True))
    _close("dk", kd.grad[0], outs[2], *_budget(dtype, True))
    _close("dv", vd.grad[0], outs[3], *_budget(dtype, False))
    if p_drop:
        _check_keep_rate(dev, dtype, n, h, p_drop, seed)


def _check_keep_rate(dev, dtype, n, h, p_drop, seed):
    """The kernel's own keep rate: with q = 0 every probability is 1/n, and with v = 1 each output element is the kept
    fraction of its row times the keep scale.  Compared row by row with the restated mask and on average with 1 - p."""
    from gmlm_amd import ops
    th = round(p_drop * 256)
    ks = 256.0 / (256 - th)
    q = torch.zeros(1, n, h * 128, device=dev, dtype=dtype)
    k = torch.randn(1, n, h * 128, device=dev).to(dtype)
    v = torch.ones(1, n, h * 128, device=dev, dtype=dtype)
    out = ops.Attention.apply(q, k, v, None, h, 128 ** -0.5, p_drop, seed)
    kept = out[0].double().reshape(n, h, 128)[..., 0] / ks                      # [n, h]: kept fraction of each row
    want = torch.stack([(attn_dropout_scale(seed, hi * n, n, n, p_drop, dev) > 0).double().mean(1) for hi in range(h)], 1)
    # fp32: a few ulps of rounding, far below the 1/n = 4.4e-4 (n <= 2277) that one kept element more or fewer would move a
    # row, so the rows match the mask exactly; bf16: the probabilities and the output carry 2^-9 relative rounding
    tol = 1e-5 if dtype == torch.float32 else 4e-3
    assert float((kept - want).abs().max()) <= tol
    assert abs(float(kept.mean()) - (1 - th / 256)) < 2e-3


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("p_drop", [0.0, 0.3])
def test_padded_kv_len_d128_vs_dense_fp64(dev, dtype, p_drop):
    """b = 5 sequences of L = 300 rows, h = 8; valid keys per sequence: all, none, a ragged tail inside the first 64-key tile,
    one past a tile boundary, and one short of the end.  Keys past kv_len get probability 0 and no gradient; a sequence with
    no valid key gives zero output and zero gradients."""
    from gmlm_amd import ops
    b, L, h, d = 5, 300, 8, 128
    kv_len = torch.tensor([300, 0, 37, 193, 299], dtype=torch.int32)
    g = torch.Generator().manual_seed(300)
    q, k, v, go = (torch.randn(b, L, h * d, generator=g).to(dev, dtype) for _ in range(4))
    seed = 0x0BAD_5EED
    scale = d ** -0.5
    qd, kd, vd = (t.clone().requires_grad_(True) for t in (q, k, v))
    out = ops.Attention.apply(qd, kd, vd, kv_len.to(dev), h, scale, p_drop, seed)
    out.backward(go)
    ref = [torch.zeros(b, L, h * d, dtype=torch.float64, device=dev) for _ in range(4)]
    for bi in range(b):
        n = int(kv_len[bi])
        if n == 0:
            continue                                              # no valid key: zero output, zero gradients
        for hi in range(h):
            sl = slice(hi * d, (hi + 1) * d)
            qq = q[bi, :, sl].double().requires_grad_(True)
            kk, vv = (t[bi, :n, sl].double().requires_grad_(True) for t in (k, v))
            pr = torch.softmax((qq @ kk.t()) * scale, -1)
            if p_drop:
                pr = pr * attn_dropout_scale(seed, (bi * h + hi) * L, L, L, p_drop, dev)[:, :n]
            o = pr @ vv
            o.backward(go[bi, :, sl].double())
            ref[0][bi, :, sl], ref[1][bi, :, sl] = o.detach(), qq.grad
            ref[2][bi, :n, sl], ref[3][bi, :n, sl] = kk.grad, vv.grad
    print(f"\npadded self-attention b={b} L={L} h={h} d=128 {dtype}, kv_len {kv_len.tolist()}, dropout {p_drop}:")
    _close("out", out.detach(), ref[0], *_budget(dtype, False))
    _close("dq", qd.grad, ref[1], *_budget(dtype, True))
    _close("dk", kd.grad, ref[2], *_budget(dtype, True))
    _close("dv", vd.grad, ref[3], *_budget(dtype, False))
    valid = torch.arange(L, device=dev)[None, :] < kv_len.to(dev)[:, None]
    assert float(kd.grad[~valid].abs().max()) == 0.0 and float(vd.grad[~valid].abs().max()) == 0.0
    assert float(out[1].abs().max()) == 0.0 and float(qd.grad[1].abs().max()) == 0.0


def test_attention_any_dim_pads_97_to_127_up_to_128(dev):
    """Head dims between 96 and 128 run on the d = 128 kernels through zero padding (exact)."""
    from gmlm_amd import nn as gnn
    h, d, n = 2, 112, 300
    g = torch.Generator().manual_seed(112)
    q, k, v, go = (torch.randn(1, n, h * d, generator=g).to(dev) for _ in range(4))
    qd, kd, vd = (t.clone().requires_grad_(True) for t in (q, k, v))
    out = gnn.attention_any_dim(qd, kd, vd, None, h, d ** -0.5, 0.0, False)
    out.backward(go)
    qr, kr, vr = (t.double().reshape(n, h, d).transpose(0, 1).requires_grad_(True) for t in (q, k, v))
    o = torch.softmax(qr @ kr.transpose(1, 2) * d ** -0.5, -1) @ vr
    o.backward(go.double().reshape(n, h, d).transpose(0, 1))
    _close("out", out.detach()[0], o.detach().transpose(0, 1).reshape(n, h * d), 1e-4, 1e-5)
    _close("dq", qd.grad[0], qr.grad.transpose(0, 1).reshape(n, h * d), 1e-4, 1e-5)
    _close("dk", kd.grad[0], kr.grad.transpose(0, 1).reshape(n, h * d), 1e-4, 1e-5)
    _close("dv", vd.grad[0], vr.grad.transpose(0, 1).reshape(n, h * d), 1e-4, 1e-5)
