"""GPU parity tests: every kernel of libgmlm_hip.so, called through the C ABI (via gmlm_amd.ops),
against the CPU oracle / plain fp32 torch on the same seeded inputs.  Index work is bit-exact;
floating point tolerances are written next to each check."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import gmlm_oracle as O
from helpers import load_golden, t

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import gmlm_amd
    gmlm_amd.lib()
    from gmlm_amd._lib import device_info
    cu, wave, arch = device_info(0)
    assert wave == 64 and arch.startswith("gfx950"), (cu, wave, arch)
    return torch.device("cuda:0")


# ------------------------------------------------------------------------------------------- K1
def test_edge_types_and_degree_golden(dev):
    import gmlm_amd
    g = load_golden("g3_int")
    for ci in range(int(g["num_cases"])):
        n = int(g[f"c{ci}_n"])
        ei = t(g[f"c{ci}_edge_index"]).to(dev)
        deg = gmlm_amd.degree(ei[0], n)
        assert deg.dtype == torch.float32 and np.array_equal(deg.cpu().numpy(), g[f"c{ci}_degree"])
        et = gmlm_amd.edge_types_from_degree(ei, n)
        assert et.dtype == torch.long and np.array_equal(et.cpu().numpy(), g[f"c{ci}_edge_type"])


@pytest.mark.parametrize("n,e,r", [(1, 0, 5), (7, 3, 5), (100, 1000, 5), (5201, 217073, 5), (300, 5000, 3)])
def test_relation_csr_bit_exact(dev, n, e, r):
    import gmlm_amd
    g = torch.Generator().manual_seed(n + e)
    ei = torch.randint(0, n, (2, e), generator=g)
    et = torch.randint(0, r, (e,), generator=g) if r == 3 else None
    csr = gmlm_amd.build_rel_csr(ei.to(dev), n, r, None if et is None else et.to(dev))
    et_ref = et if et is not None else O.edge_types_from_degree(ei, n)
    assert np.array_equal(csr.edge_type.cpu().numpy(), et_ref.numpy())
    active = sorted(set(et_ref.tolist())) or [0]
    assert csr.active_relations == active
    remap = {rr: s for s, rr in enumerate(active)}
    et_slot = torch.tensor([remap[int(v)] for v in et_ref.tolist()], dtype=torch.long)
    rowptr, col, eid = O.relation_csr(ei, et_slot, n, len(active))
    assert np.array_equal(csr.rowptr.cpu().numpy(), rowptr)
    assert np.array_equal(csr.col.cpu().numpy(), col)
    assert np.array_equal(csr.perm.cpu().numpy(), eid)
    # transpose: sorted by source, stable; t_seg = forward segment of each edge
    order = np.argsort(ei[0].numpy(), kind="stable")
    key = (ei[1] * len(active) + et_slot).numpy()
    assert np.array_equal(csr.t_seg.cpu().numpy(), key[order].astype(np.int32))
    assert np.array_equal(csr.t_rowptr.cpu().numpy(), np.concatenate([[0], np.cumsum(np.bincount(ei[0].numpy(), minlength=n))]).astype(np.int32))


def test_csr_rejects_bad_ids(dev):
    import gmlm_amd
    ei = torch.tensor([[0, 5], [1, 0]], device=dev)
    with pytest.raises(ValueError):
        gmlm_amd.build_rel_csr(ei, 3, 5)
    with pytest.raises(ValueError):
        gmlm_amd.build_rel_csr(torch.tensor([[0, 1], [1, 0]], device=dev), 3, 5, torch.tensor([0, 7], device=dev))


# ------------------------------------------------------------------------------------------- K2/K3
@pytest.mark.parametrize("n,e,f", [(64, 256, 32), (183, 298, 1703), (500, 6000, 768), (500, 6000, 96), (300, 3000, 2089),
                                   (40, 0, 16), (2000, 40000, 1536), (128, 4000, 3072)])
def test_spmm_forward_backward_fp32(dev, n, e, f):
    from gmlm_amd import build_rel_csr
    from gmlm_amd.ops import RGCNAggregate
    g = torch.Generator().manual_seed(f + n)
    ei = torch.randint(0, n, (2, e), generator=g)
    x = torch.randn(n, f, generator=g)
    et = O.edge_types_from_degree(ei, n)
    csr = build_rel_csr(ei.to(dev), n, 5)
    xg = x.to(dev).requires_grad_(True)
    h = RGCNAggregate.apply(xg, csr)
    xr = x.clone().requires_grad_(True)
    href = O.rgcn_mean_aggregate(xr, ei, et, 5)[csr.active_relations]           # [R_a, n, f]
    href2 = href.permute(1, 0, 2).reshape(n, -1)
    # fp32 sums of <= a few hundred terms in a different order: 1e-5 relative to the row scale
    np.testing.assert_allclose(h.detach().cpu().numpy(), href2.detach().numpy(), rtol=1e-5, atol=1e-5)
    go = torch.randn(h.shape, generator=g)
    h.backward(go.to(dev))
    href2.backward(go)
    np.testing.assert_allclose(xg.grad.cpu().numpy(), xr.grad.numpy(), rtol=1e-5, atol=2e-5)


def test_spmm_bf16(dev):
    from gmlm_amd import build_rel_csr
    from gmlm_amd.ops import RGCNAggregate
    n, e, f = 700, 9000, 768
    g = torch.Generator().manual_seed(5)
    ei = torch.randint(0, n, (2, e), generator=g)
    x = torch.randn(n, f, generator=g).bfloat16()
    csr = build_rel_csr(ei.to(dev), n, 5)
    h = RGCNAggregate.apply(x.to(dev), csr)
    et = O.edge_types_from_degree(ei, n)
    href = O.rgcn_mean_aggregate(x.float(), ei, et, 5)[csr.active_relations].permute(1, 0, 2).reshape(n, -1)
    # inputs identical bf16 values, fp32 accumulation, one bf16 rounding at the end: <= 2^-8 relative
    np.testing.assert_allclose(h.float().cpu().numpy(), href.numpy(), rtol=8e-3, atol=1e-3)


def test_spmm_linearity_and_determinism_full_size(dev):
    """Squirrel-size (BASELINE headline): A(ax + by) = aA(x) + bA(y); two launches bit-identical."""
    from gmlm_amd import build_rel_csr
    from gmlm_amd.ops import RGCNAggregate
    n, e, f = 5201, 217073, 768
    g = torch.Generator().manual_seed(1002)
    ei = torch.randint(0, n, (2, e), generator=g).to(dev)
    x, y = torch.randn(n, f, generator=g).to(dev), torch.randn(n, f, generator=g).to(dev)
    csr = build_rel_csr(ei, n, 5)
    hx, hy = RGCNAggregate.apply(x, csr), RGCNAggregate.apply(y, csr)
    hxy = RGCNAggregate.apply(2.0 * x - 0.5 * y, csr)
    assert torch.allclose(hxy, 2.0 * hx - 0.5 * hy, rtol=1e-4, atol=1e-4)
    assert torch.equal(hx, RGCNAggregate.apply(x, csr))
    # mean of a constant field is that constant wherever a node has neighbours of that relation
    ones = RGCNAggregate.apply(torch.ones(n, 8, device=dev), csr).view(n, csr.r_active, 8)
    cnt = (csr.rowptr[1:] - csr.rowptr[:-1]).view(n, csr.r_active)
    assert torch.allclose(ones[..., 0], (cnt > 0).float(), rtol=0, atol=1e-6)


# ------------------------------------------------------------------------------------------- K4
@pytest.mark.parametrize("n,f,act", [(2, 16, True), (183, 64, True), (1000, 768, False), (777, 100, True)])
def test_graphnorm_fwd_bwd(dev, n, f, act):
    from gmlm_amd.ops import GraphNormAct
    g = torch.Generator().manual_seed(n * f)
    z = torch.randn(n, f, generator=g) * 2 + 0.7
    w, b, ms = (1 + 0.1 * torch.randn(f, generator=g)), 0.1 * torch.randn(f, generator=g), 1 + 0.1 * torch.randn(f, generator=g)
    go = torch.randn(n, f, generator=g)
    ref_in = [v.clone().requires_grad_(True) for v in (z, w, b, ms)]
    yr = O.graph_norm(*ref_in)
    if act:
        yr = F.gelu(yr)
    yr.backward(go)
    dev_in = [v.to(dev).requires_grad_(True) for v in (z, w, b, ms)]
    y = GraphNormAct.apply(dev_in[0], dev_in[1], dev_in[2], dev_in[3], 1e-5, act, 0.0, 0, torch.float32, None, None)
    y.backward(go.to(dev))
    np.testing.assert_allclose(y.detach().cpu().numpy(), yr.detach().numpy(), rtol=2e-5, atol=2e-5)
    for a, r, name in zip(dev_in, ref_in, "z w b ms".split()):
        scale = float(r.grad.abs().max()) + 1e-6
        np.testing.assert_allclose(a.grad.cpu().numpy(), r.grad.numpy(), rtol=2e-4, atol=2e-5 * scale, err_msg=name)


def test_graphnorm_dropout_replay_and_rate(dev):
    from gmlm_amd.ops import GraphNormAct
    n, f = 2000, 256
    z = torch.randn(n, f, device=dev, requires_grad=True)
    one, zero = torch.ones(f, device=dev), torch.zeros(f, device=dev)
    y0 = GraphNormAct.apply(z, one, zero, one, 1e-5, False, 0.0, 0, torch.float32, None, None)
    y1 = GraphNormAct.apply(z, one, zero, one, 1e-5, False, 0.3, 1234, torch.float32, None, None)
    y2 = GraphNormAct.apply(z, one, zero, one, 1e-5, False, 0.3, 1234, torch.float32, None, None)
    assert torch.equal(y1, y2)                                  # same seed -> same mask (checkpoint replay)
    kept = (y1 != 0)
    assert abs(kept.float().mean().item() - 0.7) < 0.01
    assert torch.allclose(y1[kept], y0[kept] / 0.7, rtol=1e-5, atol=1e-6)
    y1.sum().backward()                                          # backward regenerates the same mask
    g1 = z.grad.clone()
    assert torch.isfinite(g1).all()


# ------------------------------------------------------------------------------------------- K6
@pytest.mark.parametrize("rows,f,act,dt", [(5, 64, False, torch.float32), (300, 768, False, torch.float32),
                                           (300, 768, True, torch.float32), (257, 256, False, torch.bfloat16),
                                           (64, 1024, True, torch.float32)])
def test_bias_res_layernorm(dev, rows, f, act, dt):
    from gmlm_amd.ops import bias_res_layernorm
    g = torch.Generator().manual_seed(rows + f)
    x, res = torch.randn(rows, f, generator=g), torch.randn(rows, f, generator=g)
    bias, gamma, beta = 0.1 * torch.randn(f, generator=g), 1 + 0.1 * torch.randn(f, generator=g), 0.1 * torch.randn(f, generator=g)
    go = torch.randn(rows, f, generator=g)
    eps = 1e-12
    xq, rq = x.to(dt).float(), res.to(dt).float()
    ref_in = [v.clone().requires_grad_(True) for v in (xq, bias, rq, gamma, beta)]
    yr = F.layer_norm(ref_in[0] + ref_in[1] + ref_in[2], (f,), ref_in[3], ref_in[4], eps)
    if act:
        yr = F.gelu(yr)
    yr.backward(go)
    dev_in = [x.to(dev, dt).requires_grad_(True), bias.to(dev).requires_grad_(True), res.to(dev, dt).requires_grad_(True),
              gamma.to(dev).requires_grad_(True), beta.to(dev).requires_grad_(True)]
    y = bias_res_layernorm(dev_in[0], dev_in[1], dev_in[2], dev_in[3], dev_in[4], eps, act)
    y.backward(go.to(dev, dt))
    tol = dict(rtol=2e-5, atol=2e-5) if dt == torch.float32 else dict(rtol=2e-2, atol=2e-2)
    np.testing.assert_allclose(y.float().detach().cpu().numpy(), yr.detach().numpy(), **tol)
    for a, r, name in zip(dev_in, ref_in, "x bias res gamma beta".split()):
        scale = float(r.grad.abs().max()) + 1e-6
        gt = dict(rtol=2e-4, atol=3e-5 * scale) if dt == torch.float32 else dict(rtol=3e-2, atol=2e-2 * scale)
        np.testing.assert_allclose(a.grad.float().cpu().numpy(), r.grad.numpy(), err_msg=name, **gt)


# ------------------------------------------------------------------------------------------- K5/K7
def _attn_ref(q, k, v, kv_len, h, scale):
    b, lq, hd = q.shape
    d = hd // h
    qh, kh, vh = (x.view(b, -1, h, d).transpose(1, 2) for x in (q, k, v))
    s = (qh @ kh.transpose(-1, -2)) * scale
    if kv_len is not None:
        m = torch.arange(k.shape[1])[None, :] >= kv_len[:, None]
        s = s.masked_fill(m[:, None, None, :], torch.finfo(s.dtype).min)
    return (s.softmax(-1) @ vh).transpose(1, 2).reshape(b, lq, hd)


@pytest.mark.parametrize("b,h,lq,lk,d,masked", [(1, 8, 150, 150, 96, False), (3, 4, 24, 24, 64, True), (2, 12, 130, 130, 64, True),
                                                (1, 8, 5201, 5201, 96, False), (1, 2, 1, 1, 64, False), (2, 3, 70, 200, 96, True)])
def test_attention_fwd_bwd_fp32(dev, b, h, lq, lk, d, masked):
    from gmlm_amd.ops import attention
    g = torch.Generator().manual_seed(lq * 7 + d)
    q, k, v = (torch.randn(b, l, h * d, generator=g) for l in (lq, lk, lk))
    kv_len = None
    if masked:
        kv_len = torch.randint(1, lk + 1, (b,), generator=g)
        kv_len[0] = lk
        if b > 1:
            kv_len[1] = 1
    scale = d ** -0.5
    go = torch.randn(b, lq, h * d, generator=g)
    ref_in = [x.clone().requires_grad_(True) for x in (q, k, v)]
    big = lq * lk > 4_000_000
    if big:   # keep the CPU reference affordable: forward only on a row subset
        with torch.no_grad():
            rows = torch.arange(0, lq, 37)
            yr = _attn_ref(q[:, rows], k, v, kv_len, h, scale)
    else:
        yr = _attn_ref(*ref_in, kv_len, h, scale)
        yr.backward(go)
    dev_in = [x.to(dev).requires_grad_(True) for x in (q, k, v)]
    y = attention(dev_in[0], dev_in[1], dev_in[2], None if kv_len is None else kv_len.to(dev, torch.int32), h, scale)
    y.backward(go.to(dev))
    if big:
        np.testing.assert_allclose(y.detach().cpu()[:, rows].numpy(), yr.numpy(), rtol=1e-4, atol=2e-5)
        assert all(torch.isfinite(x.grad).all() for x in dev_in)
        return
    # exact-f32 MFMA (fmaf chain) + fast exp: 1e-5 absolute on O(1) outputs
    np.testing.assert_allclose(y.detach().cpu().numpy(), yr.detach().numpy(), rtol=1e-4, atol=1e-5)
    for a, r, name in zip(dev_in, ref_in, "q k v".split()):
        gr = r.grad
        if masked and name in ("k", "v"):   # masked keys get exactly zero gradient
            for bi in range(b):
                assert float(a.grad[bi, int(kv_len[bi]):].abs().max() if int(kv_len[bi]) < lk else 0.0) == 0.0
        scale_g = float(gr.abs().max()) + 1e-6
        np.testing.assert_allclose(a.grad.cpu().numpy(), gr.numpy(), rtol=1e-3, atol=2e-5 * scale_g + 1e-6, err_msg=name)


@pytest.mark.parametrize("b,h,l,d", [(4, 12, 128, 64), (1, 8, 700, 96)])
def test_attention_bf16(dev, b, h, l, d):
    from gmlm_amd.ops import attention
    g = torch.Generator().manual_seed(l + d)
    q, k, v = (torch.randn(b, l, h * d, generator=g).bfloat16() for _ in range(3))
    kv_len = torch.randint(1, l + 1, (b,), generator=g)
    go = torch.randn(b, l, h * d, generator=g).bfloat16()
    ref_in = [x.float().requires_grad_(True) for x in (q, k, v)]
    yr = _attn_ref(*ref_in, kv_len, h, d ** -0.5)
    yr.backward(go.float())
    dev_in = [x.to(dev).requires_grad_(True) for x in (q, k, v)]
    y = attention(dev_in[0], dev_in[1], dev_in[2], kv_len.to(dev, torch.int32), h, d ** -0.5)
    y.backward(go.to(dev))
    # bf16 operands (8-bit mantissa) for P and V with fp32 accumulation: 2e-2 on O(1) outputs
    np.testing.assert_allclose(y.float().detach().cpu().numpy(), yr.detach().numpy(), rtol=3e-2, atol=2e-2)
    for a, r, name in zip(dev_in, ref_in, "q k v".split()):
        s = float(r.grad.abs().max())
        np.testing.assert_allclose(a.grad.float().cpu().numpy(), r.grad.numpy(), rtol=5e-2, atol=3e-2 * s, err_msg=name)


def test_attention_fused_qkv_strides_and_small_heads(dev):
    """q/k/v as strided slices of one [b, l, 3*h*d] buffer (BERT layout); head dim 16 via zero padding."""
    from gmlm_amd.nn import attention_any_dim
    b, l, h, d = 2, 40, 4, 16
    g = torch.Generator().manual_seed(3)
    qkv = torch.randn(b, l, 3 * h * d, generator=g)
    kv_len = torch.tensor([40, 7])
    p = h * d
    yr = _attn_ref(qkv[..., :p], qkv[..., p:2 * p], qkv[..., 2 * p:], kv_len, h, d ** -0.5)
    qg = qkv.to(dev)
    y = attention_any_dim(qg[..., :p], qg[..., p:2 * p], qg[..., 2 * p:], kv_len.to(dev, torch.int32), h, d ** -0.5, 0.0, False)
    np.testing.assert_allclose(y.cpu().numpy(), yr.numpy(), rtol=1e-4, atol=1e-5)
    b, l, h, d = 2, 50, 12, 64
    qkv = torch.randn(b, l, 3 * h * d, generator=g).to(dev)
    p = h * d
    from gmlm_amd.ops import attention
    y1 = attention(qkv[..., :p], qkv[..., p:2 * p], qkv[..., 2 * p:], None, h, 0.125)
    y2 = attention(qkv[..., :p].contiguous(), qkv[..., p:2 * p].contiguous(), qkv[..., 2 * p:].contiguous(), None, h, 0.125)
    assert torch.equal(y1, y2)


def test_attention_dropout(dev):
    from gmlm_amd.ops import Attention
    b, h, l, d = 1, 8, 300, 96
    g = torch.Generator().manual_seed(9)
    q, k = (torch.randn(b, l, h * d, generator=g).to(dev) for _ in range(2))
    v = torch.ones(b, l, h * d, device=dev)
    # with V = 1 the output is sum_k drop(P)_k: mean 1, and exactly 1 without dropout
    y0 = Attention.apply(q, k, v, None, h, d ** -0.5, 0.0, 0)
    assert torch.allclose(y0, torch.ones_like(y0), atol=1e-5)
    y1 = Attention.apply(q, k, v, None, h, d ** -0.5, 0.3, 77)
    y2 = Attention.apply(q, k, v, None, h, d ** -0.5, 0.3, 77)
    assert torch.equal(y1, y2) and not torch.equal(y1, y0)
    assert abs(y1.mean().item() - 1.0) < 0.02
    # gradient check of the dropped attention against autograd on the same (recovered) mask
    qs, ks, vs = (torch.randn(1, 64, 2 * 64, generator=g).to(dev).requires_grad_(True) for _ in range(3))
    eye_v = torch.zeros(1, 64, 2 * 64, device=dev)
    eye_v[0, :, :64] = torch.eye(64, device=dev)
    eye_v[0, :, 64:] = torch.eye(64, device=dev)
    pd = Attention.apply(qs.detach(), ks.detach(), eye_v, None, 2, 0.125, 0.25, 5).view(1, 64, 2, 64).permute(0, 2, 1, 3)  # dropped P
    p_full = ((qs.view(1, 64, 2, 64).transpose(1, 2) @ ks.view(1, 64, 2, 64).transpose(1, 2).transpose(-1, -2)) * 0.125).softmax(-1)
    mask = (pd != 0).float() / 0.75
    assert torch.allclose(pd, p_full.detach() * mask, atol=1e-5)
    yr = ((p_full * mask) @ vs.view(1, 64, 2, 64).transpose(1, 2)).transpose(1, 2).reshape(1, 64, 128)
    go = torch.randn(1, 64, 128, generator=g).to(dev)
    gr = torch.autograd.grad(yr, (qs, ks, vs), go)
    y = Attention.apply(qs, ks, vs, None, 2, 0.125, 0.25, 5)
    gk = torch.autograd.grad(y, (qs, ks, vs), go)
    for a, r in zip(gk, gr):
        assert torch.allclose(a, r, rtol=1e-3, atol=2e-5)


# ------------------------------------------------------------------------------------------- K8 / K9 / gelu
def test_meanpool_scatter(dev):
    from gmlm_amd.ops import MeanPoolScatter
    b, l, p, n = 5, 17, 768, 40
    g = torch.Generator().manual_seed(8)
    hs = torch.randn(b, l, p, generator=g)
    lens = torch.tensor([17, 1, 5, 9, 2])
    idx = torch.tensor([3, 39, 0, 11, 12])
    am = (torch.arange(l)[None] < lens[:, None]).long()
    hr = hs.clone().requires_grad_(True)
    ref = torch.zeros(n, p).index_put((idx,), O.masked_mean_pool(hr, am))
    go = torch.randn(n, p, generator=g)
    ref.backward(go)
    hg = hs.to(dev).requires_grad_(True)
    out = MeanPoolScatter.apply(torch.zeros(n, p, device=dev), hg, lens.to(dev, torch.int32), idx.to(dev))
    out.backward(go.to(dev))
    np.testing.assert_allclose(out.detach().cpu().numpy(), ref.detach().numpy(), rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(hg.grad.cpu().numpy(), hr.grad.numpy(), rtol=1e-6, atol=1e-7)


def test_softmask_golden_and_grad(dev):
    import gmlm_amd
    g = load_golden("g5_funcs")
    x, m, tok = t(g["sm_x"]).to(dev), t(g["sm_mask"]).to(dev), t(g["sm_tok"]).to(dev).requires_grad_(True)
    out = gmlm_amd.soft_masking_gnn_input(x, m, tok, 0.7)
    # the kernel forms (1-beta)*x + (beta*token) with one fma: <= 1 ulp from the reference's two roundings
    np.testing.assert_allclose(out.detach().cpu().numpy(), g["sm_out"], rtol=2e-7, atol=2e-7)
    out2 = gmlm_amd.soft_masking_gnn_input(x, torch.zeros(40, dtype=torch.bool, device=dev), tok, 0.7)
    assert np.array_equal(out2.detach().cpu().numpy(), g["sm_out_empty"])
    go = torch.randn(out.shape, device=dev)
    out.backward(go)
    ref = 0.7 * go[m].sum(0, keepdim=True)
    assert torch.allclose(tok.grad, ref, rtol=1e-5, atol=1e-6)
    # padded, bf16 output used by the model's first layer
    o3 = gmlm_amd.soft_masking_gnn_input(x, m, tok, 0.7, torch.bfloat16, 16)
    assert o3.shape == (40, 16) and float(o3[:, 12:].abs().max()) == 0.0
    assert torch.allclose(o3[:, :12].float(), out.detach(), rtol=1e-2, atol=1e-2)


def test_bias_gelu(dev):
    from gmlm_amd.ops import bias_gelu
    g = torch.Generator().manual_seed(4)
    x, bias, go = torch.randn(333, 3072, generator=g), torch.randn(3072, generator=g), torch.randn(333, 3072, generator=g)
    xr, br = x.clone().requires_grad_(True), bias.clone().requires_grad_(True)
    F.gelu(xr + br).backward(go)
    xg, bg = x.to(dev).requires_grad_(True), bias.to(dev).requires_grad_(True)
    y = bias_gelu(xg, bg)
    y.backward(go.to(dev))
    np.testing.assert_allclose(y.detach().cpu().numpy(), F.gelu(x + bias).numpy(), rtol=1e-5, atol=3e-6)
    np.testing.assert_allclose(xg.grad.cpu().numpy(), xr.grad.numpy(), rtol=1e-4, atol=1e-6)
    np.testing.assert_allclose(bg.grad.cpu().numpy(), br.grad.numpy(), rtol=1e-4, atol=1e-4)


def test_ops_refuse_cpu_tensors():
    import gmlm_amd
    from gmlm_amd.ops import RGCNAggregate
    with pytest.raises(gmlm_amd.GmlmHipError):
        gmlm_amd.degree(torch.zeros(3, dtype=torch.long), 3)


def test_spmm_power_law_long_segments(dev):
    """Skewed graph: a few targets/sources own thousands of edges -> chunked reduction path (split plan)."""
    from gmlm_amd import build_rel_csr
    from gmlm_amd.ops import RGCNAggregate
    n, e, f = 3000, 60000, 64
    g = torch.Generator().manual_seed(21)
    w = (torch.arange(n, dtype=torch.float32) + 1).pow(-0.9)
    ei = torch.stack([torch.multinomial(w, e, True, generator=g), torch.multinomial(w, e, True, generator=g)])
    x = torch.randn(n, f, generator=g)
    csr = build_rel_csr(ei.to(dev), n, 5)
    assert csr.split is not None and csr.t_split is not None and csr.split.n_long > 0
    et = O.edge_types_from_degree(ei, n)
    xr = x.clone().requires_grad_(True)
    href = O.rgcn_mean_aggregate(xr, ei, et, 5)[csr.active_relations].permute(1, 0, 2).reshape(n, -1)
    xg = x.to(dev).requires_grad_(True)
    h = RGCNAggregate.apply(xg, csr)
    # up to ~10^4 terms per row summed in a different order: 1e-4 relative to the accumulated magnitude
    np.testing.assert_allclose(h.detach().cpu().numpy(), href.detach().numpy(), rtol=1e-4, atol=1e-4)
    go = torch.randn(h.shape, generator=g)
    h.backward(go.to(dev))
    href.backward(go)
    np.testing.assert_allclose(xg.grad.cpu().numpy(), xr.grad.numpy(), rtol=1e-4, atol=1e-4)
    assert torch.equal(h, RGCNAggregate.apply(xg, csr))          # deterministic


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
def test_attention_online_softmax_rescale_branch(dev, dt):
    """The kernel skips the running-max rescale while the max grows by < 2^6 and rescales otherwise.  Random
    data almost never takes the rescale branch after the first tile, so force it: a few keys far down the
    sequence score 40+ above everything before them for some queries (and not for others).

    fp32: against the fp32 torch reference at 2e-5.  bf16: the forced scores reach 50-100 (natural units) and the pipelined
    forward rounds q * scale * log2(e) once more to bf16, i.e. a score error of ~|s| 2^-9 ~ 0.1-0.2 in the worst element:
    against plain fp32 that is a few % on a probability that is not saturated (bar 5e-2: precision, not the kernel).  The
    real check is therefore against the oracle's bf16-emulating attention (oracle/bf16_emulation.py: same pre-scaling, same
    reference-max schedule per 32-query wave and 32-key block, same split lse / delta terms in the backward): forward AND
    all three gradients within 5e-2 relative, elementwise."""
    from gmlm_amd.ops import attention
    from helpers import kernels_run
    b, h, l, d = 1, 2, 400, 64
    g = torch.Generator().manual_seed(17)
    q, k, v = (torch.randn(b, l, h * d, generator=g) for _ in range(3))
    k[0, 70] = q[0, 5] * 6.0          # tile 1: huge score for query 5 (and a few correlated ones)
    k[0, 333] = q[0, 200] * 9.0       # tile 5: another jump for query 200
    k[0, 399] = q[0, 5] * 12.0        # last (partial) tile: second jump for query 5
    q, k, v = q.to(dt), k.to(dt), v.to(dt)
    go = torch.randn(b, l, h * d, generator=g).to(dt)
    qd, kd, vd = (x.to(dev).requires_grad_(True) for x in (q, k, v))
    box = {}
    ran = kernels_run(lambda: box.setdefault("y", attention(qd, kd, vd, None, h, d ** -0.5)))
    y = box["y"]
    want = "attn_fwd_kernel<float, 64, 2, false>" if dt == torch.float32 else "attn_fwd_pipe_kernel<64, 4, false, 2>"
    assert {n for n in ran if n.startswith("attn_")} == {want}, ran
    y.backward(go.to(dev))
    qr, kr, vr = (x.float().clone().requires_grad_(True) for x in (q, k, v))
    ref = _attn_ref(qr, kr, vr, None, h, d ** -0.5)
    ref.backward(go.float())
    if dt == torch.float32:
        np.testing.assert_allclose(y.detach().cpu().numpy(), ref.detach().numpy(), rtol=2e-5, atol=2e-5)
        for a, r_ in ((qd, qr), (kd, kr), (vd, vr)):
            sc = float(r_.grad.abs().max())
            np.testing.assert_allclose(a.grad.cpu().numpy(), r_.grad.numpy(), rtol=1e-3, atol=4e-5 * sc)
        return
    np.testing.assert_allclose(y.float().detach().cpu().numpy(), ref.detach().numpy(), rtol=5e-2, atol=5e-2)
    import bf16_emulation as E
    heads = lambda t_: t_[0].float().view(l, h, d).transpose(0, 1).contiguous()                  # [h, L, d]
    qe, ke, ve = (heads(x).requires_grad_(True) for x in (q, k, v))
    ye = E._LongAttention.apply(qe, ke, ve, d ** -0.5)
    ye.backward(heads(go))
    back = lambda t_: t_.transpose(0, 1).reshape(1, l, h * d)
    for name, a, r_ in (("out", y.detach(), back(ye.detach())), ("dq", qd.grad, back(qe.grad)), ("dk", kd.grad, back(ke.grad)),
                        ("dv", vd.grad, back(ve.grad))):
        a = a.float().cpu()
        sc = float(r_.abs().max())
        bad = ((a - r_).abs() > 5e-2 * r_.abs() + 4e-3 * sc)                # one bf16 ulp of the largest element absolute
        print(f"  rescale branch bf16 {name}: max|err|/max = {float((a - r_).abs().max()) / sc:.2e}, elements off = {int(bad.sum())}")
        assert int(bad.sum()) == 0, name



# one spiked input per copy of the deferred online-softmax rescale (kDefer in attn_fwd_kernel and attn_d128.hip, kSumDefer /
# settle() in attn_fwd_pipe.hip): id -> (dtype, d, b, h, lq, lk, forward kernel that must run, checker)
_RESCALE_FAMILIES = {
    "f32_d64_w8": (torch.float32, 64, 8, 8, 2100, 2100, "attn_fwd_kernel<float, 64, 8, false>", "fp64"),
    "f32_d96_w2": (torch.float32, 96, 1, 2, 400, 400, "attn_fwd_kernel<float, 96, 2, false>", "fp64"),
    "f32_d96_w8": (torch.float32, 96, 8, 8, 2100, 2100, "attn_fwd_kernel<float, 96, 8, false>", "fp64"),
    "bf16_d64_w2": (torch.bfloat16, 64, 1, 2, 100, 400, "attn_fwd_kernel<unsigned short, 64, 2, false>", "fp64"),
    "pipe_d96_w4": (torch.bfloat16, 96, 1, 2, 400, 400, "attn_fwd_pipe_kernel<96, 4, false, 2>", "emulation"),
    "pipe_d96_w8": (torch.bfloat16, 96, 8, 8, 2100, 2100, "attn_fwd_pipe_kernel<96, 8, false, 2>", "emulation"),
    "d128_bf16": (torch.bfloat16, 128, 1, 2, 400, 400, "d128::fwd_kernel<unsigned short, false>", "fp64"),
    "d128_f32": (torch.float32, 128, 1, 2, 400, 400, "d128::fwd_kernel<float, false>", "fp64"),
}


@pytest.mark.parametrize("family", list(_RESCALE_FAMILIES))
def test_attention_online_softmax_rescale_branch_every_family(dev, family):
    """The test above for every other copy of the deferred rescale.  Batch 0 gets three spiked keys: one in the second
    64-key tile and one in a middle tile, each far above every earlier score of one query, and one in the last (partial)
    tile that jumps again for the first of those queries.  The forward kernel that ran is asserted by name.

    Spike sizes (natural score units, s = a |q|^2 / sqrt(d) ~ a sqrt(d)): the rescale runs when the running max grows by
    more than kDefer = 6 in log2 units (4.2 natural) or, in the pipelined forward, when a block sum exceeds kSumDefer = 256
    (a jump of ~5.5).  fp32 and the pipelined forward take the large spikes of the test above (s ~ 50-120): fp32 is checked
    against float64 at the fp32 budget, the pipelined forward against its bf16 emulation (its pre-scaled query carries an
    extra ~|s| 2^-9 rounding that float64 does not model).  The other bf16 kernels do not pre-scale q and are checked
    against float64 at the bf16 budget, so their spikes stay small: s ~ 10 and 12 after N(0, 1) scores (jumps of ~6-8
    natural units, above both thresholds) and s ~ 20 for the second jump, where the bf16 rounding of a score (~|s| 2^-9 =
    0.04) is still inside the budget."""
    from gmlm_amd.ops import attention
    from helpers import _close, _dense_reference, kernels_run
    dt, d, b, h, lq, lk, want, checker = _RESCALE_FAMILIES[family]
    g = torch.Generator().manual_seed(17 + d)
    q, go = (torch.randn(b, lq, h * d, generator=g) for _ in range(2))
    k, v = (torch.randn(b, lk, h * d, generator=g) for _ in range(2))
    big = dt == torch.float32 or checker == "emulation"
    a1, a2, a3 = (6.0, 9.0, 12.0) if big else tuple(x * 8.0 / d ** 0.5 for x in (1.25, 1.5, 2.5))
    mid = lk // 2 + 33                                         # a middle tile, not on a tile boundary
    k[0, 70] = q[0, 5] * a1                                    # second tile: first jump for query 5
    k[0, mid] = q[0, min(lq - 1, 60)] * a2                     # middle tile: a jump for another query
    k[0, lk - 1] = q[0, 5] * a3                                # last (partial) tile: second jump for query 5
    q, k, v, go = (x.to(dev, dt) for x in (q, k, v, go))
    qd, kd, vd = (x.clone().requires_grad_(True) for x in (q, k, v))
    box = {}
    ran = kernels_run(lambda: box.setdefault("y", attention(qd, kd, vd, None, h, d ** -0.5)))
    y = box["y"]
    assert {n for n in ran if n.startswith(("attn_fwd", "d128::fwd"))} == {want}, ran
    y.backward(go)
    got = (y.detach(), qd.grad, kd.grad, vd.grad)
    if checker == "fp64":
        ref = _dense_reference(q, k, v, go, h, d ** -0.5)
        for name, a, r_ in zip(("out", "dq", "dk", "dv"), got, ref):
            if dt == torch.float32:
                _close(name, a, r_, 1e-4, 1e-5)
            else:
                _close(name, a, r_, 2e-2, 6e-3 if name == "out" else 8e-3)
        return
    import bf16_emulation as E
    heads = lambda t_: t_[0].float().cpu().view(-1, h, d).transpose(0, 1).contiguous()           # batch 0 (spiked): [h, L, d]
    qe, ke, ve = (heads(x).requires_grad_(True) for x in (q, k, v))
    ye = E._LongAttention.apply(qe, ke, ve, d ** -0.5)
    ye.backward(heads(go))
    back = lambda t_: t_.transpose(0, 1).reshape(-1, h * d)
    for name, a, r_ in (("out", got[0], back(ye.detach())), ("dq", got[1], back(qe.grad)), ("dk", got[2], back(ke.grad)),
                        ("dv", got[3], back(ve.grad))):
        a = a[0].float().cpu()
        sc = float(r_.abs().max())
        bad = ((a - r_).abs() > 5e-2 * r_.abs() + 4e-3 * sc)
        print(f"  rescale branch {family} {name}: max|err|/max = {float((a - r_).abs().max()) / sc:.2e}, elements off = {int(bad.sum())}")
        assert int(bad.sum()) == 0, name

@pytest.mark.parametrize("ra,nb,cols", [(1, 30, 768 * 1536), (4, 30, 64 * 128), (5, 32, 1000), (3, 7, 2096 * 16)])
def test_basis_compose_fwd_bwd(dev, ra, nb, cols):
    """K10: W_r = sum_b comp[r,b] weight[b] and the fused backward (dweight, dcomp) vs autograd."""
    from gmlm_amd.nn import _BasisCompose
    g = torch.Generator().manual_seed(ra * 100 + nb)
    comp, weight, gw = torch.randn(ra, nb, generator=g), torch.randn(nb, cols, generator=g), torch.randn(ra, cols, generator=g)
    cr, wr = comp.clone().requires_grad_(True), weight.clone().requires_grad_(True)
    (cr @ wr).backward(gw)
    cd_, wd = comp.to(dev).requires_grad_(True), weight.to(dev).requires_grad_(True)
    w = _BasisCompose.apply(cd_, wd, None)
    np.testing.assert_allclose(w.detach().cpu().numpy(), (comp @ weight).numpy(), rtol=1e-5, atol=1e-5)
    w.backward(gw.to(dev))
    np.testing.assert_allclose(wd.grad.cpu().numpy(), wr.grad.numpy(), rtol=1e-5, atol=1e-5)
    sc = float(cr.grad.abs().max())
    np.testing.assert_allclose(cd_.grad.cpu().numpy(), cr.grad.numpy(), rtol=1e-4, atol=1e-5 * sc)


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
def test_attention_packed_varlen_matches_padded(dev, dt):
    """Packed (cu_seqlens) self-attention == padded attention with key lengths, forward and backward, incl.
    sequences of length 1, exactly one tile and many tiles."""
    from gmlm_amd.ops import attention_qkv
    h, d = 12, 64
    lens = torch.tensor([1, 64, 130, 7, 128, 300, 65])
    b, lmax, tot = lens.numel(), int(lens.max()), int(lens.sum())
    g = torch.Generator().manual_seed(12)
    qkv_pad = torch.randn(b, lmax, 3 * h * d, generator=g).to(dt)
    go_pad = torch.randn(b, lmax, h * d, generator=g).to(dt)
    valid = torch.arange(lmax)[None] < lens[:, None]
    cu = torch.zeros(b + 1, dtype=torch.int32)
    cu[1:] = torch.cumsum(lens, 0)
    qp = qkv_pad.to(dev).requires_grad_(True)
    yp = attention_qkv(qp, lens.to(dev, torch.int32), h, d ** -0.5)
    (yp * go_pad.to(dev) * valid.to(dev)[..., None]).sum().backward()
    qk = qkv_pad[valid].to(dev).requires_grad_(True)                 # [tot, 3hd]
    yk = attention_qkv(qk, None, h, d ** -0.5, 0.0, False, cu.to(dev), lmax)
    (yk * go_pad[valid].to(dev)).sum().backward()
    assert yk.shape == (tot, h * d)
    tol = 1e-5 if dt == torch.float32 else 2e-2
    np.testing.assert_allclose(yk.float().detach().cpu().numpy(), yp.float().detach().cpu()[valid].numpy(), rtol=tol, atol=tol)
    gsc = float(qp.grad.float().abs().max())
    np.testing.assert_allclose(qk.grad.float().cpu().numpy(), qp.grad.float().cpu()[valid].numpy(), rtol=10 * tol, atol=2 * tol * gsc)


def test_split_plan_index_arrays_bit_exact(dev):
    """The long-segment chunk tables (index data of K2/K3) equal the numpy restatement exactly."""
    from gmlm_amd import build_rel_csr
    n, e = 2000, 80000
    g = torch.Generator().manual_seed(33)
    w = (torch.arange(n, dtype=torch.float32) + 1).pow(-1.0)
    ei = torch.stack([torch.multinomial(w, e, True, generator=g), torch.multinomial(w, e, True, generator=g)])
    csr = build_rel_csr(ei.to(dev), n, 5)
    for plan, rowptr in ((csr.split, csr.rowptr), (csr.t_split, csr.t_rowptr)):
        assert plan is not None
        ls, cp, ow = O.split_plan(rowptr.cpu().numpy(), plan.thresh)
        assert plan.n_long == ls.size and plan.n_chunks == ow.size
        assert np.array_equal(plan.long_seg.cpu().numpy(), ls)
        assert np.array_equal(plan.chunk_ptr.cpu().numpy(), cp)
        assert np.array_equal(plan.chunk_owner.cpu().numpy(), ow)


def _packed_ref_grads(qkv, go, lens, h, d, scale, masks=None):
    """fp32 torch reference of packed self-attention backward, one sequence at a time."""
    tot = qkv.shape[0]
    gq = torch.zeros(tot, 3 * h * d, device=qkv.device)
    out = torch.zeros(tot, h * d, device=qkv.device)
    o = 0
    for i, l in enumerate(lens.tolist()):
        x = qkv[o:o + l].float().detach().requires_grad_(True)
        q, k, v = (x[:, j * h * d:(j + 1) * h * d].view(l, h, d).transpose(0, 1) for j in range(3))
        p = ((q @ k.transpose(-1, -2)) * scale).softmax(-1)
        if masks is not None:
            p = p * masks[i]
        y = (p @ v).transpose(0, 1).reshape(l, h * d)
        y.backward(go[o:o + l].float())
        gq[o:o + l], out[o:o + l] = x.grad, y.detach()
        o += l
    return out, gq


def test_attention_fused_short_sequence_backward(dev):
    """Sequences of <= 128 tokens in bf16 take the single-launch backward (delta + dQ + dK/dV from one LDS image):
    checked against an fp32 torch reference per sequence, without dropout and — through the dropped
    probabilities recovered from a forward with V = I — with dropout."""
    from gmlm_amd.ops import attention_qkv
    h, d = 12, 64
    g = torch.Generator().manual_seed(21)
    lens = torch.cat([torch.tensor([1, 31, 32, 33, 64, 65, 96, 127, 128, 2]), torch.randint(1, 129, (50,), generator=g)])
    assert lens.numel() * h >= 512
    cu = torch.zeros(lens.numel() + 1, dtype=torch.int32)
    cu[1:] = torch.cumsum(lens, 0)
    tot = int(cu[-1])
    qkv = (torch.randn(tot, 3 * h * d, generator=g) * 0.7).to(dev, torch.bfloat16).requires_grad_(True)
    go = torch.randn(tot, h * d, generator=g).to(dev, torch.bfloat16)
    # the Q / K / V biases of the fused projection that produced qkv enter as inputs whose GRADIENT the operator returns
    # (an explicit autograd edge; different dtypes to check the cast)
    bq, bk, bv = (torch.zeros(h * d, device=dev, dtype=dt_, requires_grad=True) for dt_ in (torch.float32, torch.float32, torch.bfloat16))
    y = attention_qkv(qkv, None, h, d ** -0.5, 0.0, False, cu.to(dev), 128, bias_masters=(bq, bk, bv))
    y.backward(go)
    yr, gr = _packed_ref_grads(qkv.detach(), go, lens, h, d, d ** -0.5)
    assert float((y.detach().float() - yr).abs().max()) <= 2e-2 * float(yr.abs().max())
    for j, name in enumerate("qkv"):
        a, r = qkv.grad[:, j * h * d:(j + 1) * h * d].float(), gr[:, j * h * d:(j + 1) * h * d]
        assert float((a - r).abs().max()) <= 2e-2 * float(r.abs().max()), name
    # the same launch also returns the column sums of dqkv (the fused QKV projection's bias gradient), formed from the
    # LDS tiles by three matrix-vector MFMAs per (sequence, head): against the fp32 reference's column sums
    assert bq.grad.dtype == torch.float32 and bv.grad.dtype == torch.bfloat16
    db = torch.cat([bq.grad.float(), bk.grad.float(), bv.grad.float()])
    db_ref = gr.sum(0)
    assert float((db.cpu() - db_ref.cpu()).abs().max()) <= 1e-2 * float(db_ref.abs().max()) + 1e-3
    assert float((db - qkv.grad.float().sum(0)).abs().max()) <= 1e-2 * float(db_ref.abs().max()) + 1e-3
    # the same batch with consecutive sequences PACKED into work items of <= 128 rows / <= 13 sequences (block-diagonal mask in
    # the MFMA chain): same numbers as one sequence per work item up to the bf16 summation order of the bias sums
    from gmlm_amd.ops import pack_sequence_groups
    grp = pack_sequence_groups(lens.tolist())
    gl = (grp[1:] - grp[:-1]).tolist()
    rows_per = [int(lens[grp[i]:grp[i + 1]].sum()) for i in range(len(gl))]
    assert max(gl) > 1 and max(gl) <= 13 and max(rows_per) <= 128 and int(grp[-1]) == lens.numel()
    qkv_g = qkv.detach().clone().requires_grad_(True)
    bg = [torch.zeros(h * d, device=dev, requires_grad=True) for _ in range(3)]
    yg = attention_qkv(qkv_g, None, h, d ** -0.5, 0.0, False, cu.to(dev), 128, bias_masters=bg, groups=grp.to(dev))
    yg.backward(go)
    # a row's scores and maximum do not depend on the packing; its keys fall into other 32-key blocks, so fp32 sums run in
    # another order: at most an occasional bf16 ulp
    assert float((yg.float() - y.float()).abs().max()) <= 2 ** -7 * float(y.float().abs().max())
    for j, name in enumerate("qkv"):
        a, r = qkv_g.grad[:, j * h * d:(j + 1) * h * d].float(), gr[:, j * h * d:(j + 1) * h * d]
        assert float((a - r).abs().max()) <= 2e-2 * float(r.abs().max()), name
    assert float((qkv_g.grad.float() - qkv.grad.float()).abs().max()) <= 2 ** -6 * float(qkv.grad.float().abs().max())
    dbg = torch.cat([t_.grad for t_ in bg])
    assert float((dbg.cpu() - db_ref.cpu()).abs().max()) <= 1e-2 * float(db_ref.abs().max()) + 1e-3
    # 14 sequences of one token + short ones: more sequences than a group may hold (13) must split, ids stay distinct
    lens4 = torch.tensor([1] * 30 + [3, 2, 5] * 20)
    cu4 = torch.zeros(lens4.numel() + 1, dtype=torch.int32)
    cu4[1:] = torch.cumsum(lens4, 0)
    grp4 = pack_sequence_groups(lens4.tolist())
    assert int((grp4[1:] - grp4[:-1]).max()) == 13
    qkv4 = (torch.randn(int(cu4[-1]), 3 * h * d, generator=g) * 0.7).to(dev, torch.bfloat16).requires_grad_(True)
    go4 = torch.randn(int(cu4[-1]), h * d, generator=g).to(dev, torch.bfloat16)
    y4 = attention_qkv(qkv4, None, h, d ** -0.5, 0.0, False, cu4.to(dev), 5, groups=grp4.to(dev))
    y4.backward(go4)
    yr4, gr4 = _packed_ref_grads(qkv4.detach(), go4, lens4, h, d, d ** -0.5)
    assert float((y4.detach().float() - yr4).abs().max()) <= 2e-2 * float(yr4.abs().max())
    assert float((qkv4.grad.float() - gr4).abs().max()) <= 2e-2 * float(gr4.abs().max())
    # long sequences / few pairs: no in-kernel sums; the operator still returns the bias gradient (one reduction pass)
    lens3 = torch.tensor([200, 40])
    cu3 = torch.tensor([0, 200, 240], dtype=torch.int32)
    qkv3 = (torch.randn(240, 3 * h * d, generator=g) * 0.7).to(dev, torch.bfloat16).requires_grad_(True)
    b3 = [torch.zeros(h * d, device=dev, requires_grad=True) for _ in range(3)]
    attention_qkv(qkv3, None, h, d ** -0.5, 0.0, False, cu3.to(dev), 200, bias_masters=b3).backward(go[:240])
    assert torch.allclose(torch.cat([t.grad for t in b3]), qkv3.grad.float().sum(0), rtol=1e-5, atol=1e-4)
    # dropout: sequences of <= 64 tokens so that V = I (L x 64) exposes the dropped probabilities
    lens2 = torch.cat([torch.tensor([1, 2, 33, 64]), torch.randint(1, 65, (44,), generator=g)])
    cu2 = torch.zeros(lens2.numel() + 1, dtype=torch.int32)
    cu2[1:] = torch.cumsum(lens2, 0)
    tot2 = int(cu2[-1])
    qkv2 = (torch.randn(tot2, 3 * h * d, generator=g) * 0.7).to(dev, torch.bfloat16)
    eye = torch.cat([torch.eye(int(l), d) for l in lens2.tolist()]).to(dev, torch.bfloat16)       # [tot2, 64]
    qkv_eye = qkv2.clone()
    qkv_eye[:, 2 * h * d:] = eye.repeat(1, h)
    torch.manual_seed(5)
    pd = attention_qkv(qkv_eye, None, h, d ** -0.5, 0.25, True, cu2.to(dev), 64)                    # dropped P rows
    masks, o = [], 0
    for l in lens2.tolist():
        m = (pd[o:o + l].float().view(l, h, d)[:, :, :l].permute(1, 0, 2) != 0).float() / 0.75        # [h, l, l]
        masks.append(m)
        o += l
    frac = 1.0 - sum(float(m.sum()) * 0.75 for m in masks) / sum(h * l * l for l in lens2.tolist())
    assert 0.2 < frac < 0.3                                  # P underflow to 0 in bf16 is rare at this scale
    q2 = qkv2.clone().requires_grad_(True)
    go2 = torch.randn(tot2, h * d, generator=g).to(dev, torch.bfloat16)
    torch.manual_seed(5)                                     # same seed -> same mask as the V = I forward
    y2 = attention_qkv(q2, None, h, d ** -0.5, 0.25, True, cu2.to(dev), 64)
    y2.backward(go2)
    yr2, gr2 = _packed_ref_grads(qkv2, go2, lens2, h, d, d ** -0.5, masks)
    assert float((y2.detach().float() - yr2).abs().max()) <= 3e-2 * float(yr2.abs().max())
    for j, name in enumerate("qkv"):
        a, r = q2.grad[:, j * h * d:(j + 1) * h * d].float(), gr2[:, j * h * d:(j + 1) * h * d]
        assert float((a - r).abs().max()) <= 3e-2 * float(r.abs().max()), name


def test_csr_and_spmm_random_shapes_property(dev):
    """Seeded sweep over ragged shapes (hypothesis-style, fixed seeds so the run is reproducible): for every drawn
    (N, E, R, F) the CSR build is bit-exact against the numpy restatement and the aggregation matches the oracle,
    including N = 1, E = 0, F not a multiple of the vector width and graphs with self loops / repeated edges."""
    from gmlm_amd import build_rel_csr
    from gmlm_amd.ops import RGCNAggregate
    rng = np.random.default_rng(2024)
    for case in range(24):
        n = int(rng.choice([1, 2, 3, 17, 64, 255, 1000]))
        e = int(rng.choice([0, 1, 5, n, 7 * n, 40 * n]))
        r = int(rng.choice([1, 2, 5]))
        f = int(rng.choice([1, 3, 8, 20, 96, 257]))
        g = torch.Generator().manual_seed(1000 + case)
        ei = torch.randint(0, n, (2, e), generator=g)
        et = torch.randint(0, r, (e,), generator=g)
        csr = build_rel_csr(ei.to(dev), n, r, et.to(dev))
        act = sorted(set(et.tolist())) or [0]
        assert list(csr.active_relations) == act, (case, csr.active_relations, act)
        slot = {rel: i for i, rel in enumerate(act)}
        et_slot = torch.tensor([slot[int(v)] for v in et.tolist()], dtype=torch.long)
        rowptr, col, eid = O.relation_csr(ei, et_slot, n, len(act))
        assert np.array_equal(csr.rowptr.cpu().numpy(), rowptr), case
        assert np.array_equal(csr.col.cpu().numpy(), col), case
        x = torch.randn(n, f, generator=g)
        xd = x.to(dev).requires_grad_(True)
        h = RGCNAggregate.apply(xd, csr)                                        # [n, R_a * f]
        ref = O.rgcn_mean_aggregate(x, ei, et_slot, len(act))                   # [R_a, n, f]
        ref2 = ref.permute(1, 0, 2).reshape(n, len(act) * f)
        np.testing.assert_allclose(h.detach().cpu().numpy(), ref2.numpy(), rtol=1e-5, atol=1e-6, err_msg=str(case))
        gout = torch.randn(n, len(act) * f, generator=g)
        h.backward(gout.to(dev))
        xr = x.clone().requires_grad_(True)
        (O.rgcn_mean_aggregate(xr, ei, et_slot, len(act)).permute(1, 0, 2).reshape(n, -1) * gout).sum().backward()
        np.testing.assert_allclose(xd.grad.cpu().numpy(), xr.grad.numpy(), rtol=1e-5, atol=1e-5, err_msg=str(case))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_embed_sum_matches_torch_gathers(dev, dtype):
    """BERT embedding sum (hf:modeling_bert.py:53-108): one pass = F.embedding(tok, word) + type[0] + F.embedding(pos, position),
    bit-exact in the forward (fp32 sums in the same order, one rounding to the storage dtype); the backward's segment sums by token /
    position id against torch's embedding backward."""
    from gmlm_amd import ops
    g = torch.Generator().manual_seed(31)
    vocab, npos, p, rows = 997, 128, 768, 20011
    word = torch.randn(vocab, p, generator=g).to(dev).requires_grad_(True)
    pos = torch.randn(npos, p, generator=g).to(dev).requires_grad_(True)
    typ = torch.randn(2, p, generator=g).to(dev).requires_grad_(True)
    tok = torch.randint(0, vocab, (rows,), generator=g)
    tok[:3000] = 7                                              # a hot token: one long segment
    pid = torch.randint(0, npos, (rows,), generator=g)
    tok, pid = tok.to(dev), pid.to(dev)
    go = torch.randn(rows, p, generator=g).to(dev, dtype)
    out = ops.embed_sum(tok, pid, word, pos, typ, dtype)
    ref = (F.embedding(tok, word) + typ[0] + F.embedding(pid, pos))
    assert torch.equal(out, ref.to(dtype))
    out.backward(go)
    gw, gp, gt = word.grad.clone(), pos.grad.clone(), typ.grad.clone()
    word.grad = pos.grad = typ.grad = None
    ref.backward(go.float())
    # the segment sums are accumulated and stored in fp32 for bf16 gradients too (the 3,000-row hot token included)
    for a, r in ((gw, word.grad), (gp, pos.grad), (gt, typ.grad)):
        assert a.dtype == torch.float32
        assert float((a - r).abs().max()) <= 1e-5 * float(r.abs().max()) + 1e-6
    # ids outside the tables: F.embedding raises; the kernel clamps (no out-of-bounds read) and reports through the flag,
    # the host-side check raises like the reference
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    ops.embed_sum(tok, pid, word, pos, typ, dtype, flag)
    assert int(flag) == 0
    bad_tok = tok.clone()
    bad_tok[17] = vocab
    ops.embed_sum(bad_tok, pid, word, pos, typ, dtype, flag)
    assert int(flag) == 1
    flag.zero_()
    bad_pid = pid.clone()
    bad_pid[5] = -1
    ops.embed_sum(tok, bad_pid, word, pos, typ, dtype, flag)
    assert int(flag) == 1
    with pytest.raises(IndexError):
        ops.check_embed_ids(bad_tok.view(1, -1), torch.tensor([4], device=dev), vocab, npos)
    with pytest.raises(IndexError):
        ops.check_embed_ids(tok.view(1, -1), torch.tensor([npos + 1], device=dev), vocab, npos)
    ops.check_embed_ids(tok.view(1, -1), torch.tensor([npos], device=dev), vocab, npos)
    assert float(gt[1].abs().max()) == 0.0


@pytest.mark.parametrize("case", ["mixed", "none_long", "one_segment", "exactly_thresh", "many_long"])
def test_device_split_plan_matches_host_plan(dev, case):
    """gmlm_split_plan_build (one kernel, capacity-sized arrays, -1 in unused slots) against the host-built plan of
    graph.make_split_plan (its counts go through the host): same long segments in ascending order, same chunk table; and the
    chunked segment sum it drives equals the unsplit one up to fp32 summation order and is bit-deterministic."""
    from gmlm_amd import ops
    from gmlm_amd.graph import make_split_plan, _segment_sort
    g = torch.Generator().manual_seed({"mixed": 1, "none_long": 2, "one_segment": 3, "exactly_thresh": 4, "many_long": 5}[case])
    thresh, nseg, f = 64, 3001, 256
    if case == "mixed":
        ids = torch.randint(0, nseg, (20000,), generator=g)
        ids[:5000] = 11; ids[5000:5100] = 2999; ids[5100:5165] = 0
    elif case == "none_long":
        ids = torch.randint(0, nseg, (4000,), generator=g)
    elif case == "one_segment":
        ids = torch.full((7777,), 1234)
    elif case == "exactly_thresh":
        ids = torch.cat([torch.full((64,), 5), torch.full((65,), 6), torch.full((128,), 7), torch.full((129,), 8)])
    else:
        ids = torch.randint(0, 40, (30000,), generator=g)            # every segment ~750 rows
    ids = ids.to(dev)
    _, perm, rowptr, _ = _segment_sort(ids, None, None, 1, nseg)
    plan = ops.device_split_plan(rowptr, ids.numel(), thresh)
    host = make_split_plan(rowptr, thresh)
    nl = 0 if host is None else host.n_long
    nc = 0 if host is None else host.n_chunks
    assert plan.n_long >= nl + 0 and plan.n_chunks >= nc
    assert bool((plan.long_seg[nl:] == -1).all()) and bool((plan.chunk_owner[nc:] == -1).all())
    assert bool((plan.chunk_ptr[nl:] == nc).all())
    if host is not None:
        assert torch.equal(plan.long_seg[:nl], host.long_seg) and torch.equal(plan.chunk_ptr[:nl + 1], host.chunk_ptr)
        assert torch.equal(plan.chunk_owner[:nc], host.chunk_owner)
    src = torch.randn(ids.numel(), f, generator=g).to(dev)
    a = torch.empty(nseg, f, device=dev)
    b = torch.empty(nseg, f, device=dev)
    c = torch.empty(nseg, f, device=dev)
    ops._spmm(src, rowptr, perm, None, False, nseg, f, a, plan)
    ops._spmm(src, rowptr, perm, None, False, nseg, f, b, ops.device_split_plan(rowptr, ids.numel(), thresh))
    ops._spmm(src, rowptr, perm, None, False, nseg, f, c)
    ref = torch.zeros(nseg, f, device=dev, dtype=torch.float64).index_add_(0, ids, src.double())
    assert torch.equal(a, b)
    assert float((a.double() - ref).abs().max()) <= 1e-5 * float(ref.abs().max()) + 1e-6
    assert float((c.double() - ref).abs().max()) <= 1e-5 * float(ref.abs().max()) + 1e-6


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("n,f", [(1, 5), (7, 33), (2277, 256), (8192, 768), (8193, 96), (40960, 256)])
def test_column_sum_paths(dev, dtype, n, f):
    """ops.column_sum (bias gradients): the fixed-order two-pass column reduction against fp64; bit-deterministic.  (A one-launch
    kernel for short matrices - 32 columns x 8 row lanes per block - was measured and removed: 8 blocks walking 2,277 rows
    take longer than the two launches they replace.)"""
    from gmlm_amd import ops
    g = torch.Generator().manual_seed(n * 131 + f)
    x = torch.randn(n, f, generator=g).to(dev, dtype)
    a, b = ops.column_sum(x), ops.column_sum(x)
    ref = x.double().sum(0)
    assert a.dtype == torch.float32 and torch.equal(a, b)
    assert float((a.double() - ref).abs().max()) <= 2e-6 * float(x.double().abs().sum(0).max()) + 1e-9
