"""The Gemma3 text encoder pass (gmlm_amd.gemma3), padded and packed, and a GraphTextLM built on it against the installed
transformers ``Gemma3TextModel`` in float64 on the CPU (eager attention), seeded random weights, every norm weight drawn from
U(-0.5, 0.5) so that the ``1 + w`` of Gemma3RMSNorm matters (HF initialises them to 0).

Two three-layer models: "bidir", 384 wide, 3 query / 1 KV heads x 256, ``use_bidirectional_attention``, sliding_window 512 (which
the config turns into 257) with pattern 3: two sliding layers on the local rope table and one full layer on the global one;
"causal", 512 wide, 4 / 2 x 256, causal.  Nine sequences of 1..257 tokens (both sides of every 32-row tile edge of gqaw::, and
the longest the bidirectional window admits), train mode, loss = a fixed random projection of the valid hidden states.
fp32 budgets are the tree's model budgets (hidden states rel-L2 1e-5, every parameter gradient within 2e-3 of its norm).
The bf16 bound is measured, not fixed: HF's own model in bf16 on the CPU against float64 gives each tensor's bf16 floor, and
each tensor of this path must be within 2x that floor (the rule and the factor of tests/test_gpu_qwen3.py)."""
import copy

import pytest
import torch
import torch.nn.functional as F

from helpers import kernels_run

pytestmark = pytest.mark.gpu

LENS = [1, 31, 33, 64, 65, 127, 128, 129, 257]
L = 257
MODELS = ("bidir", "causal")
TN = {torch.bfloat16: "unsigned short", torch.float32: "float"}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _config(kind, **kw):
    from transformers import Gemma3TextConfig
    base = dict(vocab_size=96, num_hidden_layers=3, max_position_embeddings=512, head_dim=256, attention_dropout=0.0, pad_token_id=0,
                sliding_window=512, sliding_window_pattern=3)
    if kind == "bidir":
        own = dict(hidden_size=384, intermediate_size=512, num_attention_heads=3, num_key_value_heads=1, use_bidirectional_attention=True)
    else:
        own = dict(hidden_size=512, intermediate_size=640, num_attention_heads=4, num_key_value_heads=2, query_pre_attn_scalar=144)
    cfg = Gemma3TextConfig(**{**base, **own, **kw})
    cfg._attn_implementation = "eager"
    return cfg


def _make_plm(kind, seed=0, **kw):
    from transformers import Gemma3TextModel
    torch.manual_seed(seed)
    plm = Gemma3TextModel(_config(kind, **kw))
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for n, p in plm.named_parameters():
            if p.dim() == 1:                                          # the six norms of a layer and the final norm
                p.copy_(torch.empty_like(p).uniform_(-0.5, 0.5, generator=g))
            elif n == "embed_tokens.weight":
                p.copy_(torch.randn(p.shape, generator=g) * p.shape[1] ** -0.5)      # times embed_scale = sqrt(P): unit rows
            else:
                p.copy_(torch.randn(p.shape, generator=g) * p.shape[1] ** -0.5)
    return plm.train()


def _tokens(seed=3):
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(1, 96, (len(LENS), L), generator=g)
    lens = torch.tensor(LENS)
    am = (torch.arange(L)[None, :] < lens[:, None]).long()
    ids = ids * am
    ids[8, 5] = 0                                                     # the padding id inside a sequence: its embedding row gets no gradient
    return ids, am, lens


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
        _HF[kind] = dict(plm=plm, ids=ids, am=am, lens=lens, proj=proj, ref=ref, floor=floor)
    return _HF[kind]


def _ours(h, dev, cd, packed, checkpointing=False):
    from gmlm_amd import gemma3
    m = copy.deepcopy(h["plm"]).to(dev).train()
    m.zero_grad()
    lens_d = h["lens"].to(dev, torch.int32)
    if packed:
        keep = h["am"].bool()
        tok = h["ids"][keep].to(dev)
        pos = torch.cat([torch.arange(n) for n in LENS]).to(dev)
        cu = torch.tensor([0] + LENS).cumsum(0).to(dev, torch.int32)
        hs = valid = gemma3.gemma3_encode_packed(m, tok, pos, cu, L, cd, True, checkpointing)
    else:
        hs = gemma3.gemma3_encode(m, h["ids"].to(dev), lens_d, cd, True, checkpointing)
        valid = hs[(torch.arange(L, device=dev)[None, :] < lens_d[:, None])]
    (valid.double() * h["proj"].to(dev)).sum().backward()
    return hs.detach(), valid.detach().double().cpu(), {n: p.grad.detach().double().cpu() for n, p in m.named_parameters()}


def _assert_kernels(ran, kind, dtype):
    """Exactly the gqaw:: and gemma_kernels kernels of this (mask, dtype); no wide::, causal128::, bidir:: or ln_ kernel."""
    tn, c = TN[dtype], "true" if kind == "causal" else "false"
    want = {f"gqaw::fwd_kernel<{tn}, {c}>", f"gqaw::delta_kernel<{tn}>", f"gqaw::dq_kernel<{tn}, {c}>", f"gqaw::dkv_kernel<{tn}, {c}>"}
    assert {n for n in ran if n.startswith("gqaw::")} == want, sorted(ran)
    ch = 2                                                            # 384 / 512 columns: at most 128 chunks of 4 fp32 = 2 per lane
    gk = {f"gemma_kernels::{k}<{tn}>" for k in ("qknorm_rope_fwd_kernel", "qknorm_rope_bwd_kernel", "geglu_tanh_fwd_kernel", "geglu_tanh_bwd_kernel")}
    gk |= {f"gemma_kernels::sandwich_fwd_kernel<{tn}, {ch}>", f"gemma_kernels::sandwich_bwd_kernel<{tn}, {ch}>"}
    assert {n for n in ran if n.startswith("gemma_kernels::")} == gk, sorted(ran)
    assert any(n.startswith(f"col_reduce_partial_kernel<2, gmlm::gemma_kernels::SandwichDwFn<{tn}>") for n in ran), sorted(ran)
    assert any(n.startswith(f"rmsnorm_fwd_kernel<{tn}") for n in ran)                  # the first layer's input norm
    assert not any(n.startswith(("wide::", "causal128::", "bidir::", "gqa::", "ln_", "attn_", "qknorm_rope_", "swiglu_", "mbert::", "d128::"))
                   for n in ran), sorted(ran)


@pytest.mark.parametrize("packed", [False, True], ids=["padded", "packed"])
@pytest.mark.parametrize("kind", MODELS)
def test_encoder_fp32_vs_hf_float64(dev, kind, packed):
    h = _hf(kind)
    assert sorted(set(h["plm"].config.layer_types)) == ["full_attention", "sliding_attention"]      # both rope tables are in play
    box = {}
    ran = kernels_run(lambda: box.setdefault("r", _ours(h, dev, torch.float32, packed)))
    _assert_kernels(ran, kind, torch.float32)
    hs, valid, grads = box["r"]
    assert bool(torch.isfinite(hs).all())                         # padded rows included
    ref_h, ref_g = h["ref"]
    e = float((valid - ref_h).norm() / ref_h.norm())
    print(f"  hidden: rel l2 = {e:.2e} (budget 1e-05)")
    assert e <= 1e-5
    assert set(grads) == set(ref_g)
    for n, r in ref_g.items():
        e = float((grads[n] - r).norm() / r.norm())
        print(f"  {n}: rel l2 = {e:.2e} (budget 2e-03)")
        assert float(r.norm()) > 0 and e <= 2e-3, (n, e)
    assert float(grads["embed_tokens.weight"][0].abs().max()) == 0.0 and float(ref_g["embed_tokens.weight"][0].abs().max()) == 0.0
    assert any(n.endswith("q_norm.weight") for n in ref_g) and any(n.endswith("pre_feedforward_layernorm.weight") for n in ref_g)


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
    assert float(grads["embed_tokens.weight"][0].abs().max()) == 0.0


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("kind", MODELS)
def test_packed_pass_is_the_padded_pass(dev, kind, dtype):
    """The same rows through both layouts: the valid hidden states and every gradient agree to the budgets above (fp32: 1e-5 /
    2e-3; bf16: twice the HF floor of the tensor), measured against each other."""
    h = _hf(kind)
    a, b = _ours(h, dev, dtype, False), _ours(h, dev, dtype, True)
    fl = h["floor"]
    e = float((a[1] - b[1]).norm() / a[1].norm())
    print(f"  hidden: padded vs packed rel l2 = {e:.2e}")
    assert e <= (1e-5 if dtype == torch.float32 else 2 * fl["hidden"])
    for n in a[2]:
        e = float((a[2][n] - b[2][n]).norm() / a[2][n].norm())
        assert e <= (2e-3 if dtype == torch.float32 else 2 * fl[n]), (n, e)


@pytest.mark.parametrize("packed", [False, True], ids=["padded", "packed"])
def test_gradient_checkpointing_is_bit_identical(dev, packed):
    h = _hf("bidir")
    a = _ours(h, dev, torch.bfloat16, packed, checkpointing=False)
    b = _ours(h, dev, torch.bfloat16, packed, checkpointing=True)
    assert torch.equal(a[0], b[0])
    for n in a[2]:
        assert torch.equal(a[2][n], b[2][n]), n


def test_bf16x3_gemm_precision_runs_the_fp32_kernels(dev):
    from gmlm_amd import gemma3
    h = _hf("causal")
    m = copy.deepcopy(h["plm"]).to(dev).train()
    lens_d = h["lens"].to(dev, torch.int32)
    w = gemma3.prepare_weights(m, torch.float32, "bf16x3")
    box = {}
    ran = kernels_run(lambda: box.setdefault("h", gemma3.gemma3_encode(m, h["ids"].to(dev), lens_d, torch.float32, True, False, w)))
    assert any(n.startswith("gqaw::fwd_kernel<float, true>") for n in ran), sorted(ran)
    valid = box["h"].detach()[(torch.arange(L, device=dev)[None, :] < lens_d[:, None])].double().cpu()
    e = float((valid - h["ref"][0]).norm() / h["ref"][0].norm())
    print(f"  hidden (bf16x3): rel l2 = {e:.2e}")
    assert e <= 1e-3


def test_a_sequence_past_the_window_is_refused(dev):
    from gmlm_amd import gemma3
    plm = copy.deepcopy(_hf("bidir")["plm"]).to(dev)
    assert plm.config.sliding_window == 257
    ids = torch.ones(2, 258, dtype=torch.long, device=dev)
    with pytest.raises(ValueError, match="sequence length 258 exceeds sliding_window 257"):
        gemma3.gemma3_encode(plm, ids, torch.tensor([258, 3], dtype=torch.int32, device=dev), torch.float32)
    tok = torch.ones(258, dtype=torch.long, device=dev)
    with pytest.raises(ValueError, match="sequence length 258 exceeds sliding_window 257"):
        gemma3.gemma3_encode_packed(plm, tok, torch.arange(258, device=dev), torch.tensor([0, 258], dtype=torch.int32, device=dev), 258,
                                    torch.float32)


def test_graph_text_lm_with_a_gemma3_encoder(dev):
    """Cornell-size graph (the construction of tests/test_gpu_llama.py) on the bidirectional model: logits and every gradient
    against the SAME model with HF's encoder in float64 substituted for the kernel path (the pooled states of HF float64 + the
    reference's mean pooling, main.py:351-358, fed to the model's own head in float64-cast fp32), fp32 budgets."""
    import gmlm_amd
    import gmlm_oracle as O
    h = _hf("bidir")
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
    y = data["y"].to(dev)

    # ours: the kernel path end to end
    box = {}
    ran = kernels_run(lambda: box.setdefault("logits", m(m.soft_mask_input(x, mk, 0.7), ei, tokens, mk, plm_batch_size=32)))
    assert any(k.startswith("gqaw::fwd_kernel<float, false>") for k in ran) and any(k.startswith("gemma_kernels::sandwich_fwd_kernel<float") for k in ran), ran
    assert not any(k.startswith(("causal128::", "bidir::", "gqa::", "qknorm_rope_", "embed_sum_")) for k in ran), ran
    logits = box["logits"]
    F.cross_entropy(logits[mk], y[mk], label_smoothing=0.2).backward()
    ours = {k: p.grad.detach().double().cpu() for k, p in m.named_parameters() if p.grad is not None}

    # the same model with HF's encoder in float64 substituted: plm_embeds from HF + mean pooling, through the model's own head
    ref_plm = copy.deepcopy(h["plm"]).double().train()
    ref_plm.zero_grad()
    hs = ref_plm(input_ids=ids[mask], attention_mask=am[mask]).last_hidden_state
    amf = am[mask].unsqueeze(-1).double()
    pooled = (hs * amf).sum(1) / amf.sum(1).clamp(min=1e-9)
    with torch.no_grad():
        got = m.encode_texts(tokens, mk, plm_batch_size=32).double().cpu()
    err = float((got[mask] - pooled.detach()).norm() / pooled.detach().norm())
    print(f"  plm_embeds: rel l2 = {err:.2e} (budget 1e-05)")
    assert err <= 1e-5 and float(got[~mask].abs().max()) == 0.0
    m.zero_grad()
    sub = torch.zeros(n, pooled.shape[1], device=dev)
    sub[mk] = pooled.detach().float().to(dev)
    sub.requires_grad_(True)
    orig = m.encode_texts
    m.encode_texts = lambda *a, **k: sub
    try:
        ref_logits = m(m.soft_mask_input(x, mk, 0.7), ei, tokens, mk, plm_batch_size=32)
    finally:
        m.encode_texts = orig
    F.cross_entropy(ref_logits[mk], y[mk], label_smoothing=0.2).backward()
    e = float((logits.detach().double() - ref_logits.detach().double()).norm() / ref_logits.detach().double().norm())
    print(f"  logits: rel l2 = {e:.2e} (budget 1e-05)")
    assert e <= 1e-5
    pooled.backward(sub.grad[mk].double().cpu())                     # the head's gradient through HF's float64 encoder
    ref = {k: p.grad.detach().double().cpu() for k, p in m.named_parameters() if p.grad is not None and not k.startswith("plm_encoder.")}
    ref.update({"plm_encoder." + k: p.grad.detach() for k, p in ref_plm.named_parameters()})
    assert {k for k in ours if not k.startswith("residual_proj3.")} == {k for k in ref if not k.startswith("residual_proj3.")}
    # a bias in front of a GraphNorm has a gradient of exactly zero (the norm removes the column mean): both runs hold fp32
    # rounding noise there, to which no relative bound applies; such a tensor is held to that noise level instead
    noise = 1e-6 * max(float(r.norm()) for r in ref.values())
    bad = []
    for k, r in ref.items():
        if k.startswith("residual_proj3."):                         # dead branch of the reference model (kept for the state dict)
            continue
        if float(r.norm()) <= noise:
            print(f"  {k}: |ref| = {float(r.norm()):.1e}, |ours| = {float(ours[k].norm()):.1e} (zero in exact arithmetic; noise level {noise:.1e})")
            assert k.endswith(".bias") and float(ours[k].norm()) <= noise, k
            continue
        e = float((ours[k] - r).norm() / r.norm())
        print(f"  {k}: rel l2 = {e:.2e} (budget 2e-03)")
        if e > 2e-3:
            bad.append((k, e))
    assert not bad, bad
    assert "plm_encoder.layers.1.self_attn.q_norm.weight" in m.state_dict()
