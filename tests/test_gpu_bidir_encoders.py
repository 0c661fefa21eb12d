"""The EuroBERT and NomicBERT encoder passes (gmlm_amd.eurobert, gmlm_amd.nomic_bert), padded and packed, and a GraphTextLM
built on the first against the installed transformers models in float64 on the CPU (eager attention), seeded random weights,
norm weights drawn from U(0.5, 1.5) so that they matter, biases non-zero where the model has them.

Four two-layer models: EuroBertModel 384 wide, 6 query / 2 KV heads x 64 (``bidir::`` at d = 64); EuroBertModel 256 wide, 2 / 1 x
128 with attention_bias (``bidir::`` at d = 128, Q/K/V and O biases); EuroBertModel 128 wide, 2 / 2 x 64 (the MHA route: the rotary
kernel of the ModernBERT encoder and the bidirectional ``attn_`` family, no ``bidir::`` kernel); NomicBertModel 128 wide, 2 x 64
(the same route between LayerNorms, theta 1000).  Nine sequences of 1..257 tokens (both sides of every wave, key-tile and
workgroup edge), train mode, loss = a fixed random projection of the valid hidden states.  fp32 budgets are the tree's model
budgets (hidden states rel-L2 1e-5, every parameter gradient within 2e-3 of its norm).  The bf16 bound is measured, not fixed:
HF's own model in bf16 on the CPU against float64 gives each tensor's bf16 floor, and each tensor of this path must be within
2x that floor (the rule and the factor of tests/test_gpu_qwen3.py and tests/test_gpu_llama.py)."""
import copy

import pytest
import torch
import torch.nn.functional as F

from helpers import kernels_run

pytestmark = pytest.mark.gpu

LENS = [1, 31, 33, 64, 65, 127, 128, 129, 257]
L = 257
MODELS = ("euro_gqa64", "euro_gqa128", "euro_mha64", "nomic")
TN = {torch.bfloat16: "unsigned short", torch.float32: "float"}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _config(kind, **kw):
    from transformers import EuroBertConfig, NomicBertConfig
    base = dict(vocab_size=96, num_hidden_layers=2, max_position_embeddings=512, pad_token_id=0)
    euro = dict(bos_token_id=1, eos_token_id=2, mask_token_id=3, tie_word_embeddings=False, attention_dropout=0.0)
    if kind == "euro_gqa64":
        cls, own = EuroBertConfig, dict(euro, hidden_size=384, intermediate_size=512, num_attention_heads=6, num_key_value_heads=2)
    elif kind == "euro_gqa128":
        cls, own = EuroBertConfig, dict(euro, hidden_size=256, intermediate_size=384, num_attention_heads=2, num_key_value_heads=1,
                                        head_dim=128, attention_bias=True)
    elif kind == "euro_mha64":
        cls, own = EuroBertConfig, dict(euro, hidden_size=128, intermediate_size=256, num_attention_heads=2, num_key_value_heads=2)
    else:
        cls, own = NomicBertConfig, dict(hidden_size=128, intermediate_size=256, num_attention_heads=2, hidden_dropout_prob=0.0,
                                         attention_probs_dropout_prob=0.0)
    cfg = cls(**{**base, **own, **kw})
    cfg._attn_implementation = "eager"
    return cfg


def _make_plm(kind, seed=0, **kw):
    from transformers import EuroBertModel, NomicBertModel
    torch.manual_seed(seed)
    plm = (NomicBertModel if kind == "nomic" else EuroBertModel)(_config(kind, **kw))
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for n, p in plm.named_parameters():
            if n.lower().endswith("norm.weight"):
                p.copy_(torch.empty_like(p).uniform_(0.5, 1.5, generator=g))
            elif "embed" in n and p.dim() == 2:
                p.copy_(torch.randn(p.shape, generator=g))
            elif p.dim() == 1:
                p.copy_(torch.randn(p.shape, generator=g) * 0.5)        # projection and LayerNorm biases
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
    m = copy.deepcopy(plm).to(dtype).train()
    m.zero_grad()
    hs = m(input_ids=ids, attention_mask=am).last_hidden_state
    valid = hs[am.bool()]
    (valid.double() * proj).sum().backward()
    return valid.detach().double(), {n: p.grad.detach().double() for n, p in m.named_parameters()}


_HF = {}


def _hf(kind):
    """The float64 reference and the bf16 floor of HF's own model, computed once per model and left unchanged."""
    if kind not in _HF:
        plm = _make_plm(kind)
        ids, am, lens = _tokens()
        width = plm.config.hidden_size
        proj = torch.randn(int(am.sum()), width, generator=torch.Generator().manual_seed(9), dtype=torch.float64) / 16
        ref = _hf_run(plm, torch.float64, ids, am, proj)
        hs, gr = _hf_run(plm, torch.bfloat16, ids, am, proj)
        floor = {"hidden": float((hs - ref[0]).norm() / ref[0].norm())}
        floor.update({n: float((gr[n] - ref[1][n]).norm() / ref[1][n].norm()) for n in gr})
        _HF[kind] = dict(kind=kind, plm=plm, ids=ids, am=am, lens=lens, proj=proj, ref=ref, floor=floor)
    return _HF[kind]


def _passes(kind):
    from gmlm_amd import eurobert, nomic_bert
    if kind == "nomic":
        return nomic_bert, nomic_bert.nomic_bert_encode, nomic_bert.nomic_bert_encode_packed
    return eurobert, eurobert.eurobert_encode, eurobert.eurobert_encode_packed


def _ours(h, dev, cd, packed, checkpointing=False, weights=None, backward=True):
    _, encode, encode_packed = _passes(h["kind"])
    m = copy.deepcopy(h["plm"]).to(dev).train()
    m.zero_grad()
    if callable(weights):
        weights = weights(m)
    lens_d = h["lens"].to(dev, torch.int32)
    if packed:
        keep = h["am"].bool()
        tok = h["ids"][keep].to(dev)
        pos = torch.cat([torch.arange(n) for n in LENS]).to(dev)
        cu = torch.tensor([0] + LENS).cumsum(0).to(dev, torch.int32)
        hs = valid = encode_packed(m, tok, pos, cu, L, cd, True, checkpointing, weights)
    else:
        hs = encode(m, h["ids"].to(dev), lens_d, cd, True, checkpointing, weights)
        valid = hs[(torch.arange(L, device=dev)[None, :] < lens_d[:, None])]
    if not backward:
        return hs.detach(), valid.detach().double().cpu(), {}
    (valid.double() * h["proj"].to(dev)).sum().backward()
    return hs.detach(), valid.detach().double().cpu(), {n: p.grad.detach().double().cpu() for n, p in m.named_parameters()}


def _assert_kernels(ran, kind, dtype):
    tn = TN[dtype]
    has = lambda stem: any(n.startswith(stem + "<" + tn) for n in ran)
    if kind in ("euro_gqa64", "euro_gqa128"):
        d = 64 if kind == "euro_gqa64" else 128
        want = {f"gqa::rope_heads_kernel<{tn}, {d}, false>", f"gqa::rope_heads_kernel<{tn}, {d}, true>"}
        want |= {f"bidir::gqa_{k}_kernel<{tn}, {d}>" for k in ("fwd", "delta", "dq", "dkv")}
        assert {n for n in ran if n.startswith(("gqa::", "bidir::", "causal128::"))} == want, sorted(ran)
        assert not any(n.startswith(("attn_", "mbert::", "d128::")) for n in ran), sorted(ran)
    else:                                                            # the MHA route: rope64 + the bidirectional attn_ family
        assert any(n.startswith(f"mbert::rope64_kernel<{tn}, false>") for n in ran), sorted(ran)
        assert any(n.startswith(f"mbert::rope64_kernel<{tn}, true>") for n in ran), sorted(ran)
        assert any(n.startswith("attn_") for n in ran), sorted(ran)
        assert not any(n.startswith(("bidir::", "gqa::", "causal128::", "d128::")) for n in ran), sorted(ran)
    for k in ("swiglu_fwd_kernel", "swiglu_bwd_kernel"):
        assert has(k), (k, sorted(ran))
    if kind == "nomic":
        assert has("ln_fwd_kernel") and has("ln_bwd_kernel"), sorted(ran)
        assert not any(n.startswith("rmsnorm_") for n in ran), sorted(ran)
    else:
        assert has("rmsnorm_fwd_kernel") and has("rmsnorm_bwd_kernel"), sorted(ran)
        assert not any(n.startswith("ln_") for n in ran), sorted(ran)
    assert not any(n.startswith(("qknorm_rope_", "bias_gelu_", "relb::", "disent::")) for n in ran), sorted(ran)


@pytest.mark.parametrize("packed", [False, True], ids=["padded", "packed"])
@pytest.mark.parametrize("kind", MODELS)
def test_encoder_fp32_vs_hf_float64(dev, kind, packed):
    h = _hf(kind)
    box = {}
    ran = kernels_run(lambda: box.setdefault("r", _ours(h, dev, torch.float32, packed)))
    _assert_kernels(ran, kind, torch.float32)
    hs, valid, grads = box["r"]
    assert bool(torch.isfinite(hs).all())                         # padded rows included
    ref_h, ref_g = h["ref"]
    e = float((valid - ref_h).norm() / ref_h.norm())
    print(f"  hidden: rel l2 = {e:.2e}")
    assert e <= 1e-5
    assert set(grads) == set(ref_g)
    for n, r in ref_g.items():
        e = float((grads[n] - r).norm() / r.norm())
        print(f"  {n}: rel l2 = {e:.2e}")
        assert float(r.norm()) > 0 and e <= 2e-3, (n, e)
    assert any(n.endswith("q_proj.bias") for n in ref_g) == any(n.endswith("o_proj.bias") for n in ref_g) == (kind == "euro_gqa128")


@pytest.mark.parametrize("packed", [False, True], ids=["padded", "packed"])
@pytest.mark.parametrize("kind", MODELS)
def test_encoder_bf16_within_twice_the_hf_bf16_floor(dev, kind, packed):
    """Every tensor (valid hidden states, each parameter gradient) within 2x the error of HF's own bf16 run; the ratios are
    printed per tensor."""
    h = _hf(kind)
    box = {}
    ran = kernels_run(lambda: box.setdefault("r", _ours(h, dev, torch.bfloat16, packed)))
    _assert_kernels(ran, kind, torch.bfloat16)
    hs, valid, grads = box["r"]
    assert hs.dtype == torch.bfloat16 and bool(torch.isfinite(hs).all())
    ref_h, ref_g = h["ref"]
    fl = h["floor"]
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


@pytest.mark.parametrize("packed", [False, True], ids=["padded", "packed"])
@pytest.mark.parametrize("kind", ["euro_gqa64", "nomic"])
def test_gradient_checkpointing_is_bit_identical(dev, kind, packed):
    h = _hf(kind)
    a = _ours(h, dev, torch.bfloat16, packed, checkpointing=False)
    b = _ours(h, dev, torch.bfloat16, packed, checkpointing=True)
    assert torch.equal(a[0], b[0])
    for n in a[2]:
        assert torch.equal(a[2][n], b[2][n]), n


def test_bf16x3_gemm_precision_runs_the_fp32_kernels(dev):
    """gemm_precision "bf16x3": the GEMM operands become SplitWeight objects (fp32 rows in and out); the result stays within the
    bf16x3 form's reach of the float64 reference (3 * 2^-16 per product, far below 1e-3 here: the bound of
    tests/test_gpu_llama.py)."""
    from gmlm_amd import eurobert
    h = _hf("euro_gqa64")
    box = {}
    ran = kernels_run(lambda: box.setdefault("r", _ours(h, dev, torch.float32, False, backward=False,
                                                        weights=lambda m: eurobert.prepare_weights(m, torch.float32, "bf16x3"))))
    assert any(n.startswith("bidir::gqa_fwd_kernel<float, 64>") for n in ran), sorted(ran)
    e = float((box["r"][1] - h["ref"][0]).norm() / h["ref"][0].norm())
    print(f"  hidden (bf16x3): rel l2 = {e:.2e}")
    assert e <= 1e-3


def test_graph_text_lm_with_a_eurobert_encoder(dev):
    """Cornell-size graph (the construction of tests/test_gpu_llama.py): plm_embeds against HF float64 + the reference's mean
    pooling (main.py:351-358), then a forward + CE loss + backward step."""
    import gmlm_amd
    import gmlm_oracle as O
    h = _hf("euro_gqa64")
    n, e, f_in, c = O.WORKLOADS["cornell"]
    data = O.synthetic_graph("cornell")
    torch.manual_seed(5)
    m = gmlm_amd.GraphTextLM(f_in, 64, c, dropout_rate=0.0, plm_encoder=copy.deepcopy(h["plm"]), plm_max_length=24,
                             compute_dtype=torch.float32).to(dev).train()
    g = torch.Generator().manual_seed(6)
    width = 24
    lens = torch.randint(4, width + 1, (n,), generator=g)
    am = (torch.arange(width)[None, :] < lens[:, None]).long()
    ids = torch.randint(1, 96, (n, width), generator=g) * am
    mask = data["active_mask"]
    x, ei, mk = data["x"].to(dev), data["edge_index"].to(dev), mask.to(dev)
    tokens = gmlm_amd.TokenizedTexts.from_mask(ids.to(dev), am.to(dev))

    ref = copy.deepcopy(h["plm"]).double().eval()
    with torch.no_grad():
        hs = ref(input_ids=ids[mask], attention_mask=am[mask]).last_hidden_state
        amf = am[mask].unsqueeze(-1).double()
        pooled = (hs * amf).sum(1) / amf.sum(1).clamp(min=1e-9)
    box = {}
    with torch.no_grad():
        ran = kernels_run(lambda: box.setdefault("p", m.encode_texts(tokens, mk, plm_batch_size=32)))
    assert any(k.startswith("bidir::gqa_fwd_kernel<float, 64>") for k in ran) and any(k.startswith("gqa::rope_heads_kernel<float, 64, false>") for k in ran), ran
    assert not any(k.startswith(("attn_", "embed_sum_", "qknorm_rope_", "causal128::", "gqa::causal64")) for k in ran), ran
    got = box["p"].double().cpu()
    err = float((got[mask] - pooled).norm() / pooled.norm())
    print(f"  plm_embeds: rel l2 = {err:.2e}")
    assert err <= 1e-5 and float(got[~mask].abs().max()) == 0.0

    logits = m(m.soft_mask_input(x, mk, 0.7), ei, tokens, mk, plm_batch_size=32)
    loss = F.cross_entropy(logits[mk], data["y"].to(dev)[mk], label_smoothing=0.2)
    loss.backward()
    assert bool(torch.isfinite(logits).all()) and bool(torch.isfinite(loss))
    for k, p in m.named_parameters():
        if k.startswith("residual_proj3."):                         # dead branch of the reference model (kept for the state dict)
            continue
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), k
        if k.startswith(("plm_encoder.", "graph_to_text_attn.", "text_to_graph_attn.")):
            assert float(p.grad.abs().max()) > 0, k
    assert "plm_encoder.layers.1.self_attn.k_proj.weight" in m.state_dict()
