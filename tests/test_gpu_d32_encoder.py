"""A 384-wide BERT encoder (12 heads x 32: the MiniLM / bge-small / e5-small geometry) on the head-dim-32 kernels: the padded
and the packed encoder pass against the same HuggingFace model run in float64 on the CPU, a GraphTextLM on it through its
three routes, and the recorded encoder / whole step against the eager bucketed step.

Model: BertModel(hidden 384, 12 heads, 2 layers, intermediate 1536, vocab 200), recipe weights; eight sequences of 1..129
tokens (1, 33, 128 and 129 among them: both sides of the 32- and 128-row height thresholds of attn_d32.hip), train mode with
dropout 0, loss = a fixed random weighting of the masked mean pool.
fp32 bars are those of test_bert_block_vs_hf_golden: hidden states rtol = atol = 1e-4, pooled atol 5e-5, gradient norms 2e-3
(HF's own fp32 run on the CPU stays inside them: hidden 3e-6, pooled 2e-6, norms within 6e-4 of the float64 values).
bf16 follows tests/test_gpu_qwen3.py: every tensor within 2x the error of HF's own bf16 run against float64."""
import copy

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from helpers import bert_state_template, kernels_run
from param_recipe import recipe_state_dict

pytestmark = pytest.mark.gpu

PLM = dict(hidden=384, layers=2, heads=12, inter=1536, max_pos=160, vocab=200)
LENS = [1, 33, 128, 129, 16, 64, 65, 100]
L = max(LENS)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def make_plm(plm=PLM, seed=5):
    from test_gpu_model import hf_bert
    m = hf_bert(plm)
    m.load_state_dict(recipe_state_dict(bert_state_template(plm["hidden"], plm["layers"], plm["inter"], plm["vocab"], plm["max_pos"]),
                                        seed))
    m.config._attn_implementation = "eager"
    return m.train()


def make_tokens(seed=3):
    g = torch.Generator().manual_seed(seed)
    lens = torch.tensor(LENS)
    am = (torch.arange(L)[None, :] < lens[:, None]).long()
    ids = torch.randint(1, PLM["vocab"], (len(LENS), L), generator=g) * am
    gp = torch.randn(len(LENS), PLM["hidden"], generator=g, dtype=torch.float64)
    return ids, am, lens, gp


def hf_run(plm, dtype, ids, am, gp):
    """HF forward + backward in ``dtype`` on the CPU -> (valid hidden states, pooled, {name: grad}) as float64."""
    m = copy.deepcopy(plm).to(dtype).train()
    m.zero_grad()
    hs = m(input_ids=ids, attention_mask=am).last_hidden_state
    amf = am.unsqueeze(-1).to(hs.dtype)
    pooled = (hs * amf).sum(1) / amf.sum(1)
    (pooled.double() * gp).sum().backward()
    grads = {n: p.grad.detach().double() for n, p in m.named_parameters() if p.grad is not None}
    return hs[am.bool()].detach().double(), pooled.detach().double(), grads


def rel(a, b):
    return float((a - b).norm() / b.norm())


@pytest.fixture(scope="module")
def hf():
    """The float64 reference and the error of HF's own bf16 run, computed once for the module."""
    plm = make_plm()
    ids, am, lens, gp = make_tokens()
    ref = hf_run(plm, torch.float64, ids, am, gp)
    low = hf_run(plm, torch.bfloat16, ids, am, gp)
    floor = {"hidden": rel(low[0], ref[0]), "pooled": rel(low[1], ref[1])}
    floor.update({n: rel(low[2][n], ref[2][n]) for n in ref[2] if float(ref[2][n].norm()) > 0})
    return dict(plm=plm, ids=ids, am=am, lens=lens, gp=gp, ref=ref, floor=floor)


def ours(hf, dev, cd, packed):
    """bert_encode / bert_encode_packed + the masked mean pool -> (valid hidden states, pooled, grads) as float64 on the CPU"""
    from gmlm_amd import bert, ops
    m = copy.deepcopy(hf["plm"]).to(dev).train()
    m.zero_grad()
    ids, lens = hf["ids"].to(dev), hf["lens"].to(dev, torch.int32)
    b = len(LENS)
    pooled0 = torch.zeros(b, PLM["hidden"], device=dev)
    if packed:
        cu = torch.zeros(b + 1, dtype=torch.int32, device=dev)
        cu[1:] = torch.cumsum(lens, 0)
        keep = hf["am"].bool().to(dev)
        tok = ids[keep]
        pos = torch.arange(L, device=dev)[None, :].expand(b, L)[keep]
        hs = bert.bert_encode_packed(m, tok, pos, cu, L, cd, training=True)
        valid = hs
        pooled = ops.MeanPoolScatter.apply(pooled0, hs, None, torch.arange(b, device=dev), cu, int(sum(LENS)))
    else:
        hs = bert.bert_encode(m, ids, lens, cd, training=True)
        valid = hs[hf["am"].bool().to(dev)]
        pooled = ops.MeanPoolScatter.apply(pooled0, hs, lens, torch.arange(b, device=dev))
    (pooled.double() * hf["gp"].to(dev)).sum().backward()
    grads = {n: p.grad.detach().double().cpu() for n, p in m.named_parameters() if p.grad is not None}
    return valid.detach().double().cpu(), pooled.detach().double().cpu(), grads


def _assert_d32_only(ran, tn):
    for k in ("d32::fwd_kernel", "d32::delta_kernel", "d32::dq_kernel", "d32::dkv_kernel"):
        assert any(n.startswith(k + "<" + tn) for n in ran), (k, sorted(ran))
    assert not any(n.startswith(("attn_", "d128::")) for n in ran), sorted(ran)


@pytest.mark.parametrize("packed", [False, True], ids=["padded", "packed"])
def test_encoder_fp32_vs_hf_float64(dev, hf, packed):
    box = {}
    ran = kernels_run(lambda: box.setdefault("r", ours(hf, dev, torch.float32, packed)))
    _assert_d32_only(ran, "float")
    valid, pooled, grads = box["r"]
    ref_h, ref_p, ref_g = hf["ref"]
    print(f"  hidden max|err| = {float((valid - ref_h).abs().max()):.2e}, pooled max|err| = {float((pooled - ref_p).abs().max()):.2e}")
    np.testing.assert_allclose(valid.numpy(), ref_h.numpy(), rtol=1e-4, atol=1e-4)
    np.testing.assert_allclose(pooled.numpy(), ref_p.numpy(), rtol=1e-4, atol=5e-5)
    assert set(grads) == set(ref_g)                        # every parameter HF reaches (the pooler is unused on both sides)
    for n, r in ref_g.items():
        nrm, want = float(grads[n].norm()), float(r.norm())
        assert abs(nrm - want) <= 2e-3 * max(want, 1e-3) + 1e-6, (n, nrm, want)


@pytest.mark.parametrize("packed", [False, True], ids=["padded", "packed"])
def test_encoder_bf16_within_twice_the_hf_bf16_error(dev, hf, packed):
    """Hidden states, pooled rows and every parameter gradient within 2x the error of HF's own bf16 run against float64.  The
    key biases are left out: their gradient is mathematically zero (a constant added to every score of a row), so the float64
    value is rounding noise and no relative error exists on either side."""
    box = {}
    ran = kernels_run(lambda: box.setdefault("r", ours(hf, dev, torch.bfloat16, packed)))
    _assert_d32_only(ran, "unsigned short")
    valid, pooled, grads = box["r"]
    ref_h, ref_p, ref_g = hf["ref"]
    fl = hf["floor"]
    got = {"hidden": rel(valid, ref_h), "pooled": rel(pooled, ref_p)}
    got.update({n: rel(grads[n], ref_g[n]) for n in ref_g if n in fl and not n.endswith("key.bias")})
    bad = []
    for n, e in got.items():
        print(f"  {n}: rel l2 = {e:.2e}, HF bf16 {fl[n]:.2e}, ratio {e / fl[n]:.2f}")
        if not e <= 2 * fl[n]:
            bad.append((n, e, fl[n]))
    assert not bad, bad


# ------------------------------------------------------------------------------------------------ GraphTextLM on this encoder
def _cfg():
    return dict(n=183, e=298, f_in=40, hc=32, c=5, plm=dict(PLM, max_pos=64), seed=91, max_len=40)


def _data(cfg, dev, steps=3):
    import gmlm_amd
    g = torch.Generator().manual_seed(9)
    n = cfg["n"]
    x = torch.randn(n, cfg["f_in"], generator=g).to(dev)
    ei = torch.randint(0, n, (2, cfg["e"]), generator=g).to(dev)
    y = torch.randint(0, cfg["c"], (n,), generator=g).to(dev)
    lens = 1 + torch.randint(0, cfg["max_len"], (n,), generator=g)
    lens[:4] = torch.tensor([1, 32, 33, cfg["max_len"]])
    am = (torch.arange(cfg["max_len"])[None, :] < lens[:, None]).long()
    ids = torch.randint(1, cfg["plm"]["vocab"], (n, cfg["max_len"]), generator=g) * am
    tokens = gmlm_amd.TokenizedTexts.from_mask(ids.to(dev), am.to(dev))
    masks = [(torch.rand(n, generator=g) < 0.5).to(dev) for _ in range(steps)]
    return x, ei, y, tokens, masks


def test_graphtextlm_routes_agree(dev, monkeypatch):
    """The default (packed) route, the padded route and the restored old route (head dim 32 out of the native set: unfused
    Q / K / V zero-padded to 64 through attention_any_dim) give the same text embeddings within the fp32 bars; the first two
    run d32:: kernels only, the third none."""
    from gmlm_amd import bert
    from test_gpu_model import build_model
    cfg = _cfg()
    x, ei, y, tokens, masks = _data(cfg, dev)
    m = build_model(cfg, dev).eval()
    assert m._has_packed_pass() and m.plm_packed and m._packed_head_dim() == 32
    box = {}
    with torch.no_grad():
        ran = kernels_run(lambda: box.setdefault("packed", m.encode_texts(tokens, masks[0], plm_batch_size=512)))
        assert any(n.startswith("d32::fwd_kernel<float") for n in ran) and not any(n.startswith("attn_") for n in ran), sorted(ran)
        m.plm_packed = False
        ran = kernels_run(lambda: box.setdefault("padded", m.encode_texts(tokens, masks[0], plm_batch_size=64)))
        assert any(n.startswith("d32::fwd_kernel<float") for n in ran) and not any(n.startswith("attn_") for n in ran), sorted(ran)
        m.plm_packed = True
        monkeypatch.setattr(bert, "NATIVE_HEAD_DIMS", (64, 96))
        assert not m._has_packed_pass()
        ran = kernels_run(lambda: box.setdefault("old", m.encode_texts(tokens, masks[0], plm_batch_size=64)))
        assert any(n.startswith("attn_fwd_kernel<float, 64") for n in ran) and not any(n.startswith("d32::") for n in ran), sorted(ran)
    assert float(box["old"].abs().max()) > 0.1
    for tag in ("packed", "padded"):
        print(f"  {tag} vs old route: max|diff| = {float((box[tag] - box['old']).abs().max()):.2e}")
        np.testing.assert_allclose(box[tag].cpu().numpy(), box["old"].cpu().numpy(), rtol=1e-4, atol=5e-5)


def _step(m, x, ei, y, tokens, mask, plm_batch):
    m.zero_grad(set_to_none=True)
    logits = m(m.soft_mask_input(x, mask, 0.7), ei, tokens, mask, plm_batch_size=plm_batch)
    loss = F.cross_entropy(logits[mask], y[mask], label_smoothing=0.2)
    loss.backward()
    return logits.detach().clone(), {k: p.grad.detach().clone() for k, p in m.named_parameters() if p.grad is not None}


@pytest.mark.parametrize("cd", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("mode", ["encoder", "whole"])
def test_replay_equals_eager_at_head_dim_32(dev, cd, mode):
    """The recorded encoder and the whole-step graph of a head-dim-32 model against the eager bucketed step, bit for bit, over
    four steps with a changing active set (the pattern of test_replay_equals_eager_without_dropout)."""
    from test_gpu_model import build_model
    cfg = _cfg()
    x, ei, y, tokens, masks = _data(cfg, dev)
    eager = build_model(cfg, dev, compute_dtype=cd).train()
    eager.plm_bucketed = True
    graphed = build_model(cfg, dev, compute_dtype=cd).train()
    g = graphed.capture_hip_graphs(graphed.soft_mask_input(x, masks[0], 0.7), ei, encoder=True, whole_step=mode == "whole")
    for mask in masks + [masks[0]]:
        l0, g0 = _step(eager, x, ei, y, tokens, mask, 512)
        l1, g1 = _step(graphed, x, ei, y, tokens, mask, 512)
        assert torch.equal(l0, l1)
        assert set(g0) == set(g1)
        for k in g0:
            assert torch.equal(g0[k], g1[k]), k
    assert (len(g._steps) >= 1) == (mode == "whole") and (len(g._encoders) >= 1) == (mode == "encoder")
