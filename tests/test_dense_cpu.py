"""Host side of the dense-layer path on the CPU, bit for bit against plain torch: the flat operand buffer of the two text
encoders (one slot per fused operand, every slot rounded up to 128 elements), the routing of fp32 weight / bias gradients to
the master parameters, the lookup of a region's shadow operands, and the slicing of the split-K weight gradient.  No library
and no GPU; every name is reached as gmlm_amd.nn / gmlm_amd.bert / gmlm_amd.qwen3 expose it."""
import itertools

import pytest
import torch
import torch.nn.functional as F

import gmlm_amd.nn as gnn
from gmlm_amd import bert, qwen3

BF16, F32 = torch.bfloat16, torch.float32


# ----------------------------------------------------------------------------------------------- the operand buffer
def _bert(hidden, inter):
    from transformers import BertConfig, BertModel
    torch.manual_seed(0)
    return BertModel(BertConfig(vocab_size=50, hidden_size=hidden, num_hidden_layers=2, num_attention_heads=2,
                                intermediate_size=inter, max_position_embeddings=16))


def _qwen3(hidden, inter):
    from transformers import Qwen3Config, Qwen3Model
    torch.manual_seed(0)
    return Qwen3Model(Qwen3Config(vocab_size=50, hidden_size=hidden, intermediate_size=inter, num_hidden_layers=2,
                                  num_attention_heads=2, num_key_value_heads=1, head_dim=16, max_position_embeddings=16,
                                  tie_word_embeddings=False))


def _bert_slots(plm):
    """Per layer, in buffer order: (operand name, masters stacked along dim 0, name of the tuple of masters or None, that tuple)."""
    out = []
    for layer in plm.encoder.layer:
        sa, so = layer.attention.self, layer.attention.output
        wq = (sa.query.weight, sa.key.weight, sa.value.weight)
        bq = (sa.query.bias, sa.key.bias, sa.value.bias)
        out.append([("wqkv", wq, "m_qkv", wq + bq), ("bqkv", bq, None, None), ("wo", (so.dense.weight,), "m_wo", (so.dense.weight,)),
                    ("wi", (layer.intermediate.dense.weight,), "m_wi", (layer.intermediate.dense.weight,)),
                    ("wo2", (layer.output.dense.weight,), "m_wo2", (layer.output.dense.weight,))])
    return out


def _qwen3_slots(plm):
    out = []
    for layer in plm.layers:
        sa, mlp = layer.self_attn, layer.mlp
        wq = (sa.q_proj.weight, sa.k_proj.weight, sa.v_proj.weight)
        wgu = (mlp.gate_proj.weight, mlp.up_proj.weight)
        out.append([("wqkv", wq, "m_qkv", wq), ("wo", (sa.o_proj.weight,), "m_wo", (sa.o_proj.weight,)), ("wgu", wgu, "m_gu", wgu),
                    ("wdown", (mlp.down_proj.weight,), "m_down", (mlp.down_proj.weight,))])
    return out


# the geometry of each family that the dense-path refactor names, and an odd one where no slot is a multiple of 128 elements
PACK_CASES = [("bert", 32, 64), ("bert", 24, 40), ("qwen3", 32, 48), ("qwen3", 25, 40)]


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("family,hidden,inter", PACK_CASES)
def test_prepare_weights_packs_one_buffer(family, hidden, inter, dtype):
    if family == "bert":
        plm, mod, slots = _bert(hidden, inter), bert, _bert_slots
    else:
        plm, mod, slots = _qwen3(hidden, inter), qwen3, _qwen3_slots
    weights = mod.prepare_weights(plm, dtype)
    layers = slots(plm)
    assert len(weights) == len(layers) == 2
    first = getattr(weights[0], layers[0][0][0])
    off, unaligned = 0, 0
    for lw, layer in zip(weights, layers):
        for name, masters, m_name, m_tuple in layer:
            v = getattr(lw, name)
            want = torch.cat([m.detach().to(dtype) for m in masters], 0)
            assert v.dtype == dtype and not v.requires_grad and v.is_contiguous()
            assert torch.equal(v, want), (family, name)
            assert v.untyped_storage().data_ptr() == first.untyped_storage().data_ptr(), (family, name)
            assert v.storage_offset() - first.storage_offset() == off, (family, name)
            off += (want.numel() + 127) // 128 * 128
            unaligned += want.numel() % 128 != 0
            if m_name is not None:
                got = getattr(lw, m_name)
                assert isinstance(got, tuple) and len(got) == len(m_tuple) and all(a is b for a, b in zip(got, m_tuple)), (family, m_name)
    if hidden != 32:
        assert unaligned == 2 * len(layers[0])                      # the odd geometry: the rounding moved every offset
    assert first.untyped_storage().nbytes() >= off * first.element_size()


# ----------------------------------------------------------------------------------------------- gradient routing
def _routing_case(dtype, residual, bias_grad):
    g = torch.Generator().manual_seed(11)
    x = torch.randn(2, 3, 8, generator=g).to(dtype).requires_grad_(True)
    w1 = torch.randn(6, 8, generator=g, dtype=torch.float64).requires_grad_(True)     # an fp64 master: the gradient is cast to it
    w2 = torch.randn(4, 8, generator=g).requires_grad_(False)                         # a frozen master: no gradient
    b1 = torch.randn(6, generator=g).requires_grad_(True)
    b2 = torch.randn(4, generator=g, dtype=torch.float64).requires_grad_(True)
    wc = torch.cat([w1.detach().to(dtype), w2.detach().to(dtype)], 0)
    bc = torch.cat([b1.detach().to(dtype), b2.detach().to(dtype)], 0)
    dy = torch.randn(2, 3, 10, generator=g).to(dtype)
    dres = torch.randn(2, 3, 8, generator=g).to(dtype)
    return x, (w1, w2), (b1, b2), wc, bc, dy, dres


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("residual,bias_grad", list(itertools.product([False, True], [False, True])))
def test_mm_routes_gradients_to_the_masters(dtype, residual, bias_grad):
    x, ws, bs, wc, bc, dy, dres = _routing_case(dtype, residual, bias_grad)
    masters = ws + bs if bias_grad else ws
    out = gnn._mm(x, wc, bc, masters, residual=residual, bias_grad=bias_grad)
    dres_in = dres.clone()
    if residual:
        y, xres = out
        assert xres._base is x and xres.data_ptr() == x.data_ptr() and xres.shape == x.shape     # a view of x, not a copy
        torch.autograd.backward([y, xres], [dy, dres_in])
    else:
        y = out
        torch.autograd.backward([y], [dy])
    assert y.dtype == dtype and torch.equal(y, F.linear(x.detach(), wc, bc))

    dy2, x2 = dy.reshape(-1, 10), x.detach().reshape(-1, 8)
    dx = torch.addmm(dres.reshape(-1, 8), dy2, wc) if residual else dy2 @ wc            # the residual gradient is accumulated into dx
    assert x.grad.dtype == dtype and torch.equal(x.grad, dx.view(2, 3, 8))
    dw = (dy2.t() @ x2).float()                                                          # fp32 before it is cut by master rows
    assert ws[0].grad.dtype == torch.float64 and torch.equal(ws[0].grad, dw[:6].to(torch.float64))
    assert ws[1].grad is None
    if bias_grad:
        db = dy2.sum(0, dtype=torch.float32)
        assert bs[0].grad.dtype == torch.float32 and torch.equal(bs[0].grad, db[:6])
        assert bs[1].grad.dtype == torch.float64 and torch.equal(bs[1].grad, db[6:].to(torch.float64))
    else:
        assert bs[0].grad is None and bs[1].grad is None


# ----------------------------------------------------------------------------------------------- shadow lookup
def _shadow_case():
    g = torch.Generator().manual_seed(5)
    w = torch.randn(6, 8, generator=g).requires_grad_(True)
    b = torch.randn(6, generator=g).requires_grad_(True)
    x = torch.randn(5, 8, generator=g)
    dy = torch.randn(5, 6, generator=g)
    return w, b, x, dy


def _doctored_shadow(w, b, factor):
    """A bf16 shadow of (w, b) whose weight operand is then scaled: a result formed from it cannot be mistaken for one formed
    from the masters."""
    sh = gnn.ParamShadow([(id(w), [w], 0), (id(b), [b], 0)], BF16, torch.device("cpu"))
    assert torch.equal(sh.get(id(w)), w.detach().to(BF16)) and torch.equal(sh.get(id(b)), b.detach().to(BF16))
    sh.get(id(w)).mul_(factor)
    return sh


def test_linear_takes_shadow_operands_by_dtype():
    w, b, x, dy = _shadow_case()
    sh = _doctored_shadow(w, b, -1.0)
    xb, dyb = x.to(BF16).requires_grad_(True), dy.to(BF16)
    with gnn.use_shadow(sh) as active:
        assert active is sh
        y = gnn._linear(xb, w, b)                                   # bf16 activations: the shadow's operands
        y32 = gnn._linear(x, w, b)                                  # fp32 activations: not this shadow's dtype, the masters
    assert y.dtype == BF16 and torch.equal(y, F.linear(xb.detach(), -w.detach().to(BF16), b.detach().to(BF16)))
    assert y32.dtype == F32 and torch.equal(y32, F.linear(x, w.detach(), b.detach()))
    y.backward(dyb)
    # fp32 gradients straight to the fp32 masters: the bias gradient is an fp32 sum, not a bf16 sum cast up
    assert w.grad.dtype == F32 and torch.equal(w.grad, (dyb.t() @ xb.detach()).float())
    assert b.grad.dtype == F32 and torch.equal(b.grad, dyb.sum(0, dtype=F32))
    assert not torch.equal(b.grad, dyb.sum(0).float())
    assert torch.equal(xb.grad, dyb @ -w.detach().to(BF16))
    w.grad = b.grad = None
    y32.backward(dy)
    assert torch.equal(w.grad, dy.t() @ x) and torch.equal(b.grad, dy.sum(0))


def test_use_shadow_nests_and_restores():
    w, b, x, _ = _shadow_case()
    xb = x.to(BF16)
    outer, inner = _doctored_shadow(w, b, -1.0), _doctored_shadow(w, b, 2.0)
    bb = b.detach().to(BF16)
    plain = F.linear(xb, w.detach().to(BF16), bb)
    from_outer = F.linear(xb, -w.detach().to(BF16), bb)
    from_inner = F.linear(xb, 2.0 * w.detach().to(BF16), bb)
    assert not torch.equal(plain, from_outer) and not torch.equal(from_inner, from_outer)
    with torch.no_grad():
        assert torch.equal(gnn._linear(xb, w, b), plain)
        with gnn.use_shadow(outer):
            assert torch.equal(gnn._linear(xb, w, b), from_outer)
            with gnn.use_shadow(inner) as active:                   # a region that is running keeps its own shadow
                assert active is outer
                assert torch.equal(gnn._linear(xb, w, b), from_outer)
            assert torch.equal(gnn._linear(xb, w, b), from_outer)
        assert torch.equal(gnn._linear(xb, w, b), plain)
        with gnn.use_shadow(None) as active:
            assert active is None
            with gnn.use_shadow(inner):
                assert torch.equal(gnn._linear(xb, w, b), from_inner)
            assert torch.equal(gnn._linear(xb, w, b), plain)
        with pytest.raises(KeyError):
            with gnn.use_shadow(outer):
                raise KeyError("left by an exception")
        assert torch.equal(gnn._linear(xb, w, b), plain)


# ----------------------------------------------------------------------------------------------- split-K slicing
_WGRAD_INPUTS = {}


def _wgrad_inputs(t, dtype):
    if (t, dtype) not in _WGRAD_INPUTS:
        g = torch.Generator().manual_seed(t)
        _WGRAD_INPUTS[(t, dtype)] = (torch.randn(t, 8, generator=g).to(dtype), torch.randn(t, 8, generator=g).to(dtype))
    return _WGRAD_INPUTS[(t, dtype)]


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("keep_fp32", [True, False])
@pytest.mark.parametrize("t", [16384 + 5, 40])
def test_splitk_wgrad_slices(t, keep_fp32, dtype):
    dy, x = _wgrad_inputs(t, dtype)
    got = gnn._splitk_wgrad(dy, x, keep_fp32=keep_fp32)
    if t == 40:                                                     # below 16,384 rows: one GEMM
        want = dy.t() @ x
        want = want.float() if keep_fp32 else want
    else:                                                           # one 8 x 8 tile at 16,389 rows: 16 slices of 1,024 rows + 5 rows
        s, q = 16, 1024
        want = torch.bmm(dy[:s * q].view(s, q, 8).transpose(1, 2), x[:s * q].view(s, q, 8)).float().sum(0)
        want += dy[s * q:].t() @ x[s * q:]
        want = want if keep_fp32 else want.to(dtype)
    assert got.dtype == (F32 if keep_fp32 else dtype) and got.shape == (8, 8)
    assert torch.equal(got, want)
