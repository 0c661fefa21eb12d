"""GraphTextLM with a 1024-wide text encoder (BERT-large width: hidden 1024, 16 heads) against the CPU oracle, fp32.

The encoder's own attention stays at head dim 64; what is new is the model's two CrossAttention modules, which run 8 heads
over the PLM width (main.py:159-163): head dim 128, i.e. the gmlm_attention_d128_* kernels, forward and backward, inside the
whole model.  Before those kernels existed this configuration raised NotImplementedError in nn.attention_any_dim."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import gmlm_oracle as O
from helpers import model_state_template, oracle_model_from_config
from param_recipe import recipe_state_dict

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def test_cornell_size_bert_1024_fp32_vs_oracle(dev):
    import gmlm_amd
    from transformers import BertConfig, BertModel
    name, hc, max_len, bs = "cornell", 256, 24, 32
    plm = dict(hidden=1024, layers=2, heads=16, inter=2048, max_pos=64, vocab=200)
    n, e, f_in, c = O.WORKLOADS[name]
    cfg = dict(n=n, e=e, f_in=f_in, hc=hc, c=c, plm=plm, seed=1024 + n, max_len=max_len)
    data = O.synthetic_graph(name)
    ids, am = O.synthetic_tokens(n, max_len, plm["vocab"], seed=n, min_len=4)
    om, _ = oracle_model_from_config(cfg)
    mask = data["active_mask"]
    ref = om(O.soft_masking_gnn_input(data["x"], mask, om.gnn_mask_token_embed, 0.7), data["edge_index"], ids, am, mask,
             plm_batch_size=bs)
    loss_ref = F.cross_entropy(ref[mask], data["y"][mask], label_smoothing=0.2)
    loss_ref.backward()

    enc = BertModel(BertConfig(vocab_size=plm["vocab"], hidden_size=plm["hidden"], num_hidden_layers=plm["layers"],
                               num_attention_heads=plm["heads"], intermediate_size=plm["inter"],
                               max_position_embeddings=plm["max_pos"], hidden_dropout_prob=0.0,
                               attention_probs_dropout_prob=0.0))
    m = gmlm_amd.GraphTextLM(f_in, hc, c, dropout_rate=0.0, plm_encoder=enc, plm_max_length=max_len,
                             compute_dtype=torch.float32)
    m.load_state_dict(recipe_state_dict(model_state_template(f_in, hc, c, plm), cfg["seed"]), strict=True)
    m = m.to(dev).train()
    assert m.graph_to_text_attn.num_heads == 8 and m.graph_to_text_attn.q_proj.out_features // 8 == 128
    x, ei, mk = data["x"].to(dev), data["edge_index"].to(dev), mask.to(dev)
    tokens = gmlm_amd.TokenizedTexts.from_mask(ids.to(dev), am.to(dev))
    logits = m(m.soft_mask_input(x, mk, 0.7), ei, tokens, mk, plm_batch_size=bs)
    loss = F.cross_entropy(logits[mk], data["y"].to(dev)[mk], label_smoothing=0.2)
    loss.backward()
    np.testing.assert_allclose(logits.detach().cpu().numpy(), ref.detach().numpy(), rtol=0, atol=1e-4)
    assert abs(float(loss) - float(loss_ref)) < 1e-4
    og = {k: p.grad for k, p in om.named_parameters()}
    checked = 0
    for k, p in m.named_parameters():
        ok = "plm_params." + k[len("plm_encoder."):].replace(".", "/") if k.startswith("plm_encoder.") else k
        r = og.get(ok)
        if r is None or p.grad is None:
            assert (r is None or float(r.abs().max()) == 0) and (p.grad is None or float(p.grad.abs().max()) == 0), k
            continue
        rn, gn = float(r.double().norm()), float(p.grad.double().norm())
        assert abs(rn - gn) <= 2e-3 * max(rn, 1e-4) + 1e-6, (k, gn, rn)
        if rn > 1e-3:
            a, b = p.grad.detach().double().cpu().reshape(-1), r.double().reshape(-1)
            assert float((a - b).norm()) <= 2e-3 * float(b.norm()) + 1e-7, (k, float((a - b).norm()) / float(b.norm()))
        checked += 1
    assert checked > 20
