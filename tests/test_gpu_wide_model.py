"""GraphTextLM on text encoders wider than 1,024: the model's two CrossAttention modules (8 heads over the PLM width: head
dims 256, 320 -> 384 and 512, gmlm_attention_wide_*) and the LayerNorms of MultiScaleFusion, of the fusion MLP and of the
encoder's own layers at rows of 2,048 ... 4,096 (gmlm_bias_res_layernorm_wide_*), inside the whole model.

(a) the construction of test_gpu_wide_encoder.py (Cornell-size graph, fp32, CPU oracle) with a one-layer BertModel at hidden
    2,048 / 2,560 / 4,096, at that file's bars: logits 1e-4, loss 1e-4, every gradient norm and tensor 2e-3;
(b) the same model at hidden 2,048 in bf16: every gradient tensor's cosine against the fp32 HIP run of (a) >= 0.99 (the bar
    test_gpu_workloads.py holds bf16 to against its emulation);
(c) a one-layer Qwen3 at the widths of Qwen3-Embedding-4B / -8B (2,560 and 4,096; 32 heads x 128, 8 KV heads) in the form of
    test_gpu_qwen3.py::test_graph_text_lm_with_a_qwen3_encoder.
Before the wide kernels existed all three raised in nn.attention_any_dim or in gmlm_bias_res_layernorm_fwd."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import gmlm_oracle as O
from helpers import kernels_run, model_state_template, oracle_model_from_config
from param_recipe import recipe_state_dict

pytestmark = pytest.mark.gpu

NAME, HC, MAX_LEN, BS = "cornell", 256, 24, 32
_FP32_RUN = {}                 # hidden -> ({parameter name: fp32 gradient (CPU, float64)} of the HIP run of (a), its state dict)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _cfg(hidden, heads):
    plm = dict(hidden=hidden, layers=1, heads=heads, inter=256, max_pos=64, vocab=200)
    n, e, f_in, c = O.WORKLOADS[NAME]
    return dict(n=n, e=e, f_in=f_in, hc=HC, c=c, plm=plm, seed=hidden + n, max_len=MAX_LEN)


def _hip_run(dev, cfg, dtype, sd):
    """forward + CE + backward of gmlm_amd.GraphTextLM with the recipe's parameters ``sd`` -> (logits, loss, {name: grad}, kernels)"""
    import gmlm_amd
    from transformers import BertConfig, BertModel
    plm, n = cfg["plm"], cfg["n"]
    data = O.synthetic_graph(NAME)
    ids, am = O.synthetic_tokens(n, MAX_LEN, plm["vocab"], seed=n, min_len=4)
    enc = BertModel(BertConfig(vocab_size=plm["vocab"], hidden_size=plm["hidden"], num_hidden_layers=plm["layers"],
                               num_attention_heads=plm["heads"], intermediate_size=plm["inter"],
                               max_position_embeddings=plm["max_pos"], hidden_dropout_prob=0.0,
                               attention_probs_dropout_prob=0.0))
    m = gmlm_amd.GraphTextLM(cfg["f_in"], HC, cfg["c"], dropout_rate=0.0, plm_encoder=enc, plm_max_length=MAX_LEN,
                             compute_dtype=dtype)
    m.load_state_dict(sd, strict=True)
    m = m.to(dev).train()
    assert m.graph_to_text_attn.num_heads == 8
    mask = data["active_mask"]
    x, ei, mk = data["x"].to(dev), data["edge_index"].to(dev), mask.to(dev)
    tokens = gmlm_amd.TokenizedTexts.from_mask(ids.to(dev), am.to(dev))
    box = {}

    def step():
        logits = m(m.soft_mask_input(x, mk, 0.7), ei, tokens, mk, plm_batch_size=BS)
        loss = F.cross_entropy(logits[mk].float(), data["y"].to(dev)[mk], label_smoothing=0.2)
        loss.backward()
        box["r"] = (logits.detach(), loss.detach())

    ran = kernels_run(step)
    grads = {k: (None if p.grad is None else p.grad.detach().double().cpu()) for k, p in m.named_parameters()}
    return box["r"][0].float().cpu(), float(box["r"][1]), grads, ran


def _assert_wide_kernels(ran, t, dp):
    for k in (f"wide::fwd_kernel<{t}, {dp}, false>", f"wide::delta_kernel<{t}>", f"wide::dq_kernel<{t}, {dp}, false>",
              f"wide::dkv_kernel<{t}, {dp}, false>"):
        assert k in ran, (k, sorted(ran))
    assert any(k.startswith(f"lnw::fwd_kernel<{t}") for k in ran) and any(k.startswith(f"lnw::bwd_kernel<{t}") for k in ran), sorted(ran)
    assert not any(k.startswith("d128::") for k in ran), sorted(ran)


@pytest.mark.parametrize("hidden,heads,head_dim,padded", [(2048, 32, 256, 256), (2560, 40, 320, 384), (4096, 64, 512, 512)])
def test_cornell_size_wide_bert_fp32_vs_oracle(dev, hidden, heads, head_dim, padded):
    cfg = _cfg(hidden, heads)
    assert hidden // 8 == head_dim
    data = O.synthetic_graph(NAME)
    ids, am = O.synthetic_tokens(cfg["n"], MAX_LEN, cfg["plm"]["vocab"], seed=cfg["n"], min_len=4)
    om, sd = oracle_model_from_config(cfg)                        # sd: the recipe's state dict, shared with the HIP model
    mask = data["active_mask"]
    ref = om(O.soft_masking_gnn_input(data["x"], mask, om.gnn_mask_token_embed, 0.7), data["edge_index"], ids, am, mask,
             plm_batch_size=BS)
    loss_ref = F.cross_entropy(ref[mask], data["y"][mask], label_smoothing=0.2)
    loss_ref.backward()

    logits, loss, grads, ran = _hip_run(dev, cfg, torch.float32, sd)
    _assert_wide_kernels(ran, "float", padded)
    if hidden == 2048:
        _FP32_RUN[hidden] = (grads, sd)
    print(f"\nhidden {hidden}: max|dlogit| = {float((logits - ref.detach()).abs().max()):.2e}, |dloss| = {abs(loss - float(loss_ref)):.2e}")
    np.testing.assert_allclose(logits.numpy(), ref.detach().numpy(), rtol=0, atol=1e-4)
    assert abs(loss - float(loss_ref)) < 1e-4
    og = {k: p.grad for k, p in om.named_parameters()}
    checked, worst = 0, (0.0, None)
    for k, g in grads.items():
        ok = "plm_params." + k[len("plm_encoder."):].replace(".", "/") if k.startswith("plm_encoder.") else k
        r = og.get(ok)
        if r is None or g is None:
            assert (r is None or float(r.abs().max()) == 0) and (g is None or float(g.abs().max()) == 0), k
            continue
        rn, gn = float(r.double().norm()), float(g.norm())
        assert abs(rn - gn) <= 2e-3 * max(rn, 1e-4) + 1e-6, (k, gn, rn)
        if rn > 1e-3:
            a, b = g.reshape(-1), r.double().reshape(-1)
            rel = float((a - b).norm()) / float(b.norm())
            worst = max(worst, (rel, k))
            assert float((a - b).norm()) <= 2e-3 * float(b.norm()) + 1e-7, (k, rel)
        checked += 1
    print(f"  {checked} gradient tensors, worst relative l2 error {worst[0]:.2e} at {worst[1]}")
    assert checked > 20


def test_cornell_size_wide_bert_2048_bf16_vs_the_fp32_run(dev):
    cfg = _cfg(2048, 32)
    if 2048 not in _FP32_RUN:                                     # run on its own: the fp32 HIP run of (a) is the reference
        sd = recipe_state_dict(model_state_template(cfg["f_in"], HC, cfg["c"], cfg["plm"]), cfg["seed"])
        _FP32_RUN[2048] = (_hip_run(dev, cfg, torch.float32, sd)[2], sd)
    g32, sd = _FP32_RUN.pop(2048)
    logits, loss, gbf, ran = _hip_run(dev, cfg, torch.bfloat16, sd)
    _assert_wide_kernels(ran, "unsigned short", 256)
    assert np.isfinite(loss) and bool(torch.isfinite(logits).all())
    gmax = max(float(g.norm()) for g in g32.values() if g is not None)
    rows = []
    for k, g in gbf.items():
        r = g32[k]
        if r is None or g is None:
            assert r is None and g is None, k
            continue
        assert bool(torch.isfinite(g).all()), k
        rn, gn = float(r.norm()), float(g.norm())
        if rn <= 1e-6 * gmax:                                     # a gradient that is zero in fp32 (nothing to take a cosine of)
            assert gn <= 1e-4 * gmax, (k, gn)
            continue
        rows.append((k, rn, gn, float((g.reshape(-1) @ r.reshape(-1)) / (rn * max(gn, 1e-300)))))
    print(f"\nhidden 2048 bf16 vs fp32 (HIP): {len(rows)} gradient tensors, lowest cosines:")
    for r_ in sorted(rows, key=lambda r_: r_[3])[:8]:
        print(f"    {r_[0]:62s} |g_fp32| {r_[1]:.3e} |g_bf16| {r_[2]:.3e} cos {r_[3]:.5f}")
    worst = min(rows, key=lambda r_: r_[3])
    assert worst[3] >= 0.99, worst


@pytest.mark.parametrize("hidden", [2560, 4096])
def test_graph_text_lm_with_a_wide_qwen3_encoder(dev, hidden):
    """One Qwen3 layer at the width of Qwen3-Embedding-4B / -8B (32 heads x 128, 8 KV heads, intermediate 256): plm_embeds
    against HF float64 + the reference's mean pooling to 1e-5, forward + CE + backward finite with non-zero gradients on the
    encoder and both CrossAttention modules, and a strict state-dict round trip."""
    import copy
    import gmlm_amd
    from transformers import Qwen3Config, Qwen3Model
    kw = dict(vocab_size=96, hidden_size=hidden, intermediate_size=256, num_hidden_layers=1, num_attention_heads=32,
              num_key_value_heads=8, head_dim=128, max_position_embeddings=64, tie_word_embeddings=False, attention_dropout=0.0)
    if hasattr(Qwen3Config(), "rope_parameters"):
        kw["rope_parameters"] = {"rope_type": "default", "rope_theta": 1e6}
    else:
        kw["rope_theta"] = 1e6
    qcfg = Qwen3Config(**kw)
    qcfg._attn_implementation = "eager"

    def make(seed):
        torch.manual_seed(seed)
        plm = Qwen3Model(qcfg)
        g = torch.Generator().manual_seed(seed + 1)
        with torch.no_grad():
            for n_, p in plm.named_parameters():
                if n_.endswith("norm.weight") or "layernorm" in n_:
                    p.copy_(torch.empty_like(p).uniform_(0.5, 1.5, generator=g))
                elif n_ == "embed_tokens.weight":
                    p.copy_(torch.randn(p.shape, generator=g))
                else:
                    p.copy_(torch.randn(p.shape, generator=g) * p.shape[1] ** -0.5)
        return plm.train()

    def graph_model(plm):
        n, e, f_in, c = O.WORKLOADS[NAME]
        torch.manual_seed(5)
        m = gmlm_amd.GraphTextLM(f_in, 64, c, dropout_rate=0.0, plm_encoder=plm, plm_max_length=MAX_LEN, compute_dtype=torch.float32)
        return m.to(dev).train(), n

    plm = make(0)
    m, n = graph_model(copy.deepcopy(plm))
    data = O.synthetic_graph(NAME)
    g = torch.Generator().manual_seed(6)
    lens = torch.randint(4, MAX_LEN + 1, (n,), generator=g)
    am = (torch.arange(MAX_LEN)[None, :] < lens[:, None]).long()
    ids = torch.randint(1, 96, (n, MAX_LEN), generator=g) * am
    mask = data["active_mask"]
    x, ei, mk = data["x"].to(dev), data["edge_index"].to(dev), mask.to(dev)
    tokens = gmlm_amd.TokenizedTexts.from_mask(ids.to(dev), am.to(dev))

    ref = copy.deepcopy(plm).double().eval()
    with torch.no_grad():
        hs = ref(input_ids=ids[mask], attention_mask=am[mask]).last_hidden_state
        amf = am[mask].unsqueeze(-1).double()
        pooled = (hs * amf).sum(1) / amf.sum(1).clamp(min=1e-9)
        got = m.encode_texts(tokens, mk, plm_batch_size=32).double().cpu()
    e = float((got[mask] - pooled).norm() / pooled.norm())
    print(f"\nQwen3 hidden {hidden}: plm_embeds rel l2 = {e:.2e}")
    assert e <= 1e-5 and float(got[~mask].abs().max()) == 0.0

    box = {}

    def step():
        logits = m(m.soft_mask_input(x, mk, 0.7), ei, tokens, mk, plm_batch_size=32)
        box["loss"] = F.cross_entropy(logits[mk], data["y"].to(dev)[mk], label_smoothing=0.2)
        box["loss"].backward()

    ran = kernels_run(step)
    _assert_wide_kernels(ran, "float", 384 if hidden == 2560 else 512)
    assert bool(torch.isfinite(box["loss"]))
    for k, p in m.named_parameters():
        if k.startswith(("plm_encoder.", "graph_to_text_attn.", "text_to_graph_attn.")):
            assert p.grad is not None and bool(torch.isfinite(p.grad).all()) and float(p.grad.abs().max()) > 0, k
    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    m2, _ = graph_model(make(7))
    m2.load_state_dict(sd, strict=True)
    assert all(torch.equal(v, sd[k]) for k, v in m2.state_dict().items())
    assert "plm_encoder.layers.0.self_attn.k_norm.weight" in sd
