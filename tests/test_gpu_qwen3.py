"""The Qwen3 encoder pass (gmlm_amd.qwen3) and a GraphTextLM built on it against the installed transformers.Qwen3Model in
float64 on the CPU (eager attention), seeded random weights, norm weights drawn from U(0.5, 1.5) so that they matter.

Tiny model: 2 layers, hidden 256, 4 query / 2 KV heads x 128, intermediate 384, vocab 96, rope_theta 1e6; nine sequences of
1..257 tokens padded to 257 (both sides of every wave, key-tile and workgroup edge of the causal attention), train mode,
loss = a fixed random projection of the valid hidden states.
fp32 budgets are the tree's model budgets (hidden states rel-L2 1e-5, every parameter gradient within 2e-3 of its norm).
The bf16 bound is measured, not fixed: HF's own model in bf16 on the CPU against float64 gives each tensor's bf16 floor, and
each tensor of this path must be within 2x that floor (it rounds at the same places or fewer: statistics, SiLU and the
softmax stay in fp32; 2x covers a different summation order)."""
import pytest
import torch
import torch.nn.functional as F

from helpers import kernels_run

pytestmark = pytest.mark.gpu

LENS = [1, 31, 33, 64, 65, 127, 128, 129, 257]
L = 257


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _config(max_pos=512):
    from transformers import Qwen3Config
    kw = dict(vocab_size=96, hidden_size=256, intermediate_size=384, num_hidden_layers=2, num_attention_heads=4,
              num_key_value_heads=2, head_dim=128, max_position_embeddings=max_pos, tie_word_embeddings=False,
              attention_dropout=0.0)
    if hasattr(Qwen3Config(), "rope_parameters"):
        kw["rope_parameters"] = {"rope_type": "default", "rope_theta": 1e6}
    else:
        kw["rope_theta"] = 1e6
    cfg = Qwen3Config(**kw)
    cfg._attn_implementation = "eager"
    return cfg


def _make_plm(seed=0, max_pos=512):
    from transformers import Qwen3Model
    torch.manual_seed(seed)
    plm = Qwen3Model(_config(max_pos))
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for n, p in plm.named_parameters():
            if n.endswith("norm.weight") or "layernorm" in n:
                p.copy_(torch.empty_like(p).uniform_(0.5, 1.5, generator=g))
            elif n == "embed_tokens.weight":
                p.copy_(torch.randn(p.shape, generator=g))
            else:
                p.copy_(torch.randn(p.shape, generator=g) * p.shape[1] ** -0.5)
    return plm.train()


def _tokens(seed=3):
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(1, 96, (len(LENS), L), generator=g)
    lens = torch.tensor(LENS)
    am = (torch.arange(L)[None, :] < lens[:, None]).long()
    return ids * am, am, lens


def _hf_run(plm, dtype, ids, am, proj):
    """HF forward + backward in ``dtype`` on the CPU -> (valid hidden states [T, P], {name: grad}) as float64."""
    import copy
    m = copy.deepcopy(plm).to(dtype).train()
    m.zero_grad()
    hs = m(input_ids=ids, attention_mask=am).last_hidden_state
    valid = hs[am.bool()]
    (valid.double() * proj).sum().backward()
    return valid.detach().double(), {n: p.grad.detach().double() for n, p in m.named_parameters()}


@pytest.fixture(scope="module")
def hf():
    """The float64 reference and the bf16 / fp32 floors of HF's own model, computed once."""
    plm = _make_plm()
    ids, am, lens = _tokens()
    proj = torch.randn(int(am.sum()), 256, generator=torch.Generator().manual_seed(9), dtype=torch.float64) / 16
    ref = _hf_run(plm, torch.float64, ids, am, proj)
    floors = {}
    for dt in (torch.bfloat16, torch.float32):
        hs, gr = _hf_run(plm, dt, ids, am, proj)
        fl = {"hidden": float((hs - ref[0]).norm() / ref[0].norm())}
        fl.update({n: float((gr[n] - ref[1][n]).norm() / ref[1][n].norm()) for n in gr})
        floors[dt] = fl
    return dict(plm=plm, ids=ids, am=am, lens=lens, proj=proj, ref=ref, floors=floors)


def _ours(plm, dev, cd, ids, lens, proj, checkpointing=False):
    import copy
    from gmlm_amd import qwen3
    m = copy.deepcopy(plm).to(dev).train()
    m.zero_grad()
    lens_d = lens.to(dev, torch.int32)
    hs = qwen3.qwen3_encode(m, ids.to(dev), lens_d, cd, True, checkpointing)
    valid = hs[(torch.arange(L, device=dev)[None, :] < lens_d[:, None])]
    (valid.double() * proj.to(dev)).sum().backward()
    return hs.detach(), valid.detach().double().cpu(), {n: p.grad.detach().double().cpu() for n, p in m.named_parameters()}


QWEN3_KERNELS = ("rmsnorm_fwd_kernel", "rmsnorm_bwd_kernel", "qknorm_rope_fwd_kernel", "qknorm_rope_bwd_kernel",
                 "swiglu_fwd_kernel", "swiglu_bwd_kernel", "causal128::fwd_kernel", "causal128::delta_kernel",
                 "causal128::dq_kernel", "causal128::dkv_kernel")


def _assert_qwen3_kernels(ran, tn):
    for k in QWEN3_KERNELS:
        assert any(n.startswith(k + "<" + tn) for n in ran), (k, sorted(ran))
    assert not any(n.startswith(("ln_", "bias_gelu_", "attn_", "d128::")) for n in ran), sorted(ran)


def test_encoder_fp32_vs_hf_float64(dev, hf):
    box = {}
    ran = kernels_run(lambda: box.setdefault("r", _ours(hf["plm"], dev, torch.float32, hf["ids"], hf["lens"], hf["proj"])))
    _assert_qwen3_kernels(ran, "float")
    hs, valid, grads = box["r"]
    assert bool(torch.isfinite(hs).all())                         # padded rows included
    ref_h, ref_g = hf["ref"]
    e = float((valid - ref_h).norm() / ref_h.norm())
    print(f"  hidden: rel l2 = {e:.2e} (HF fp32 floor {hf['floors'][torch.float32]['hidden']:.2e})")
    assert e <= 1e-5
    assert set(grads) == set(ref_g)
    for n, r in ref_g.items():
        e = float((grads[n] - r).norm() / r.norm())
        print(f"  {n}: rel l2 = {e:.2e} (HF fp32 floor {hf['floors'][torch.float32][n]:.2e})")
        assert float(r.norm()) > 0 and e <= 2e-3, (n, e)


def test_encoder_bf16_within_twice_the_hf_bf16_floor(dev, hf):
    """Every tensor (valid hidden states, each parameter gradient) within 2x the error of HF's own bf16 run; the ratios are
    printed per tensor (DESIGN.md section 4 "Qwen3 encoder")."""
    box = {}
    ran = kernels_run(lambda: box.setdefault("r", _ours(hf["plm"], dev, torch.bfloat16, hf["ids"], hf["lens"], hf["proj"])))
    _assert_qwen3_kernels(ran, "unsigned short")
    hs, valid, grads = box["r"]
    assert hs.dtype == torch.bfloat16 and bool(torch.isfinite(hs).all())
    ref_h, ref_g = hf["ref"]
    fl = hf["floors"][torch.bfloat16]
    bad = []
    e = float((valid - ref_h).norm() / ref_h.norm())
    print(f"  hidden: rel l2 = {e:.2e}, HF bf16 floor {fl['hidden']:.2e}, ratio {e / fl['hidden']:.2f}")
    if e > 2 * fl["hidden"]:
        bad.append(("hidden", e, fl["hidden"]))
    for n, r in ref_g.items():
        e = float((grads[n] - r).norm() / r.norm())
        print(f"  {n}: rel l2 = {e:.2e}, HF bf16 floor {fl[n]:.2e}, ratio {e / fl[n]:.2f}")
        if e > 2 * fl[n]:
            bad.append((n, e, fl[n]))
    assert not bad, bad


@pytest.mark.parametrize("cd", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_gradient_checkpointing_is_bit_identical(dev, hf, cd):
    a = _ours(hf["plm"], dev, cd, hf["ids"], hf["lens"], hf["proj"], checkpointing=False)
    b = _ours(hf["plm"], dev, cd, hf["ids"], hf["lens"], hf["proj"], checkpointing=True)
    assert torch.equal(a[0], b[0])
    for n in a[2]:
        assert torch.equal(a[2][n], b[2][n]), n


def _graph_model(plm, dev, cd, max_len):
    import gmlm_amd
    import gmlm_oracle as O
    name, hc = "cornell", 64
    n, e, f_in, c = O.WORKLOADS[name]
    data = O.synthetic_graph(name)
    torch.manual_seed(5)
    m = gmlm_amd.GraphTextLM(f_in, hc, c, dropout_rate=0.0, plm_encoder=plm, plm_max_length=max_len, compute_dtype=cd)
    return m.to(dev).train(), data, n


def test_left_and_right_padded_token_tables_pool_identically(dev, hf):
    import copy
    import gmlm_amd
    m, data, n = _graph_model(copy.deepcopy(hf["plm"]), dev, torch.float32, 24)
    g = torch.Generator().manual_seed(4)
    width = 24
    lens = torch.randint(1, width + 1, (n,), generator=g)
    lens[0], lens[1] = width, 1
    toks = torch.randint(1, 96, (n, width), generator=g)
    cols = torch.arange(width)[None, :]
    am_r = (cols < lens[:, None]).long()
    am_l = (cols >= (width - lens)[:, None]).long()
    ids_r = toks * am_r
    ids_l = torch.zeros_like(toks)
    for i in range(n):
        ids_l[i, width - int(lens[i]):] = toks[i, :int(lens[i])]
    mask = torch.ones(n, dtype=torch.bool, device=dev)
    with torch.no_grad():
        pr = m.encode_texts(gmlm_amd.TokenizedTexts.from_mask(ids_r.to(dev), am_r.to(dev)), mask, plm_batch_size=32)
        pl = m.encode_texts(gmlm_amd.TokenizedTexts.from_mask(ids_l.to(dev), am_l.to(dev)), mask, plm_batch_size=32)
    assert float(pr.abs().max()) > 0 and torch.equal(pr, pl)


def test_graph_text_lm_with_a_qwen3_encoder(dev, hf):
    """Cornell-size graph (the construction of test_gpu_wide_encoder.py): plm_embeds against HF float64 + the reference's mean
    pooling (main.py:351-358), then forward + CE loss + backward, and a strict state-dict round trip."""
    import copy
    import gmlm_amd
    plm = copy.deepcopy(hf["plm"])
    m, data, n = _graph_model(plm, dev, torch.float32, 24)
    g = torch.Generator().manual_seed(6)
    width = 24
    lens = torch.randint(4, width + 1, (n,), generator=g)
    am = (torch.arange(width)[None, :] < lens[:, None]).long()
    ids = torch.randint(1, 96, (n, width), generator=g) * am
    mask = data["active_mask"]
    x, ei, mk = data["x"].to(dev), data["edge_index"].to(dev), mask.to(dev)
    tokens = gmlm_amd.TokenizedTexts.from_mask(ids.to(dev), am.to(dev))

    ref = copy.deepcopy(hf["plm"]).double().eval()
    with torch.no_grad():
        hs = ref(input_ids=ids[mask], attention_mask=am[mask]).last_hidden_state
        amf = am[mask].unsqueeze(-1).double()
        pooled = (hs * amf).sum(1) / amf.sum(1).clamp(min=1e-9)
    box = {}
    with torch.no_grad():
        ran = kernels_run(lambda: box.setdefault("p", m.encode_texts(tokens, mk, plm_batch_size=32)))
    assert any(k.startswith("causal128::fwd_kernel<float>") for k in ran) and any(k.startswith("meanpool_fwd_kernel") for k in ran), ran
    assert not any(k.startswith(("attn_", "embed_sum_")) for k in ran), ran          # not the packed BERT route
    got = box["p"].double().cpu()
    e = float((got[mask] - pooled).norm() / pooled.norm())
    print(f"  plm_embeds: rel l2 = {e:.2e}")
    assert e <= 1e-5 and float(got[~mask].abs().max()) == 0.0

    logits = m(m.soft_mask_input(x, mk, 0.7), ei, tokens, mk, plm_batch_size=32)
    loss = F.cross_entropy(logits[mk], data["y"].to(dev)[mk], label_smoothing=0.2)
    loss.backward()
    assert bool(torch.isfinite(loss))
    for k, p in m.named_parameters():
        if k.startswith(("plm_encoder.", "graph_to_text_attn.", "text_to_graph_attn.")):
            assert p.grad is not None and bool(torch.isfinite(p.grad).all()) and float(p.grad.abs().max()) > 0, k
    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    m2, _, _ = _graph_model(_make_plm(seed=7), dev, torch.float32, 24)
    m2.load_state_dict(sd, strict=True)
    assert all(torch.equal(v, sd[k]) for k, v in m2.state_dict().items())
    assert "plm_encoder.layers.1.self_attn.k_norm.weight" in sd
