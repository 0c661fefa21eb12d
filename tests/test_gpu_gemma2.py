"""The Gemma2 text encoder pass (gmlm_amd.gemma2), padded and packed, and a GraphTextLM built on it against the installed
transformers ``Gemma2Model`` in float64 on the CPU with eager attention (the HF path that applies the cap), seeded random
weights, every norm weight drawn from U(-0.5, 0.5) so that the ``1 + w`` of Gemma2RMSNorm matters (HF initialises them to 0):
the initialisation, the loss and the fp32 budgets of tests/test_gpu_gemma3.py.

Three four-layer causal models with ``query_pre_attn_scalar`` 144, layer types sliding, full, sliding, full:
  "cap4"   512 wide, 4 / 2 heads x 256, attn_logit_softcapping 4.0,  sliding_window 64;
  "cap50"  384 wide, 3 / 1 heads x 256, attn_logit_softcapping 50.0, sliding_window 512;
  "nocap"  "cap4" with attn_logit_softcapping None: the kernels of the Gemma3 encoder behind the rotation without a head norm.
Eight sequences of 1..129 tokens (both sides of the 32-row tile edges), so "cap4" and "nocap" run their sliding layers on the
band kernels and "cap50" runs on none.  HF runs one unpadded sequence at a time (tests/test_gpu_gemma3_band._hf_run: HF's eager
path makes a padded query without a visible key NaN).  Train mode, loss = a fixed random projection of the valid hidden states.
fp32: hidden states rel-L2 1e-5, every parameter gradient within 2e-3 of its norm.  bf16: HF's own model in bf16 on the CPU
against float64 gives each tensor's bf16 floor, and each tensor of this path must be within 2x that floor (the rule and the
factor of tests/test_gpu_gemma3.py and tests/test_gpu_qwen3.py); the ratios are printed.

Not vacuous (conditions on the cases, HF float64 at L = 129): the hidden states with cap 4 against no cap, and with window 64
against window 512, differ by >= 0.1 in relative L2 (0.27 and 0.29 when this file was written; cap 50 against no cap: 3.2e-3,
320x the fp32 budget)."""
import copy

import pytest
import torch
import torch.nn.functional as F

from helpers import kernels_run
from test_gpu_gemma3_band import _hf_run

pytestmark = pytest.mark.gpu

LENS = [1, 31, 33, 64, 65, 127, 128, 129]
L = 129
MODELS = ("cap4", "cap50", "nocap")
TN = {torch.bfloat16: "unsigned short", torch.float32: "float"}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _config(kind, **kw):
    from transformers import Gemma2Config
    base = dict(vocab_size=96, num_hidden_layers=4, max_position_embeddings=512, head_dim=256, attention_dropout=0.0, pad_token_id=0,
                query_pre_attn_scalar=144)
    if kind == "cap50":
        own = dict(hidden_size=384, intermediate_size=512, num_attention_heads=3, num_key_value_heads=1, attn_logit_softcapping=50.0,
                   sliding_window=512)
    else:
        own = dict(hidden_size=512, intermediate_size=640, num_attention_heads=4, num_key_value_heads=2, sliding_window=64,
                   attn_logit_softcapping=4.0 if kind == "cap4" else None)
    cfg = Gemma2Config(**{**base, **own, **kw})
    cfg._attn_implementation = "eager"
    return cfg


def _make_plm(kind, seed=0, **kw):
    from transformers import Gemma2Model
    torch.manual_seed(seed)
    plm = Gemma2Model(_config(kind, **kw))
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for n, p in plm.named_parameters():
            if p.dim() == 1:                                          # the four norms of a layer and the final norm
                p.copy_(torch.empty_like(p).uniform_(-0.5, 0.5, generator=g))
            else:                                                     # the embedding times embed_scale = sqrt(P): unit rows
                p.copy_(torch.randn(p.shape, generator=g) * p.shape[1] ** -0.5)
    return plm.train()


def _tokens(seed=3):
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(1, 96, (len(LENS), L), generator=g)
    lens = torch.tensor(LENS)
    am = (torch.arange(L)[None, :] < lens[:, None]).long()
    ids = ids * am
    ids[7, 5] = 0                                                     # the padding id inside a sequence: its embedding row gets no gradient
    return ids, am, lens


_HF = {}


def _hf(kind):
    """The float64 reference and the bf16 floor of HF's own model, computed once per model and left unchanged."""
    if kind not in _HF:
        plm = _make_plm(kind)
        assert list(plm.config.layer_types) == ["sliding_attention", "full_attention"] * 2
        ids, am, lens = _tokens()
        proj = torch.randn(int(am.sum()), plm.config.hidden_size, generator=torch.Generator().manual_seed(9), dtype=torch.float64) / 16
        ref = _hf_run(plm, torch.float64, ids, lens, proj)
        hs, gr = _hf_run(plm, torch.bfloat16, ids, lens, proj)
        assert bool(torch.isfinite(ref[0]).all()) and all(bool(torch.isfinite(t).all()) for t in ref[1].values())
        floor = {"hidden": float((hs - ref[0]).norm() / ref[0].norm())}
        floor.update({n: float((gr[n] - ref[1][n]).norm() / ref[1][n].norm()) for n in gr})
        _HF[kind] = dict(plm=plm, ids=ids, am=am, lens=lens, proj=proj, ref=ref, floor=floor)
    return _HF[kind]


def _ours(h, dev, cd, packed, checkpointing=False):
    from gmlm_amd import gemma2
    m = copy.deepcopy(h["plm"]).to(dev).train()
    m.zero_grad()
    lens_d = h["lens"].to(dev, torch.int32)
    if packed:
        keep = h["am"].bool()
        tok = h["ids"][keep].to(dev)
        pos = torch.cat([torch.arange(n) for n in LENS]).to(dev)
        cu = torch.tensor([0] + LENS).cumsum(0).to(dev, torch.int32)
        hs = valid = gemma2.gemma2_encode_packed(m, tok, pos, cu, L, cd, True, checkpointing)
    else:
        hs = gemma2.gemma2_encode(m, h["ids"].to(dev), lens_d, cd, True, checkpointing)
        valid = hs[(torch.arange(L, device=dev)[None, :] < lens_d[:, None])]
    (valid.double() * h["proj"].to(dev)).sum().backward()
    return hs.detach(), valid.detach().double().cpu(), {n: p.grad.detach().double().cpu() for n, p in m.named_parameters()}


def _assert_kernels(ran, kind, dtype):
    """Exactly the attention kernels of this model and dtype, the d = 256 rotary pair and the Gemma row kernels; no head norm."""
    tn = TN[dtype]
    attn = lambda fam, targs: {f"{fam}::fwd_kernel<{targs}>", f"{fam}::delta_kernel<{tn}>", f"{fam}::dq_kernel<{targs}>", f"{fam}::dkv_kernel<{targs}>"}
    want = {"gqac": set(), "gqaw": set(), "gqab": set()}
    if kind == "cap50":
        want["gqac"] = attn("gqac", f"{tn}, true, false")                       # window 512 >= 129: no band anywhere
    elif kind == "cap4":
        want["gqac"] = attn("gqac", f"{tn}, true, false") | attn("gqac", f"{tn}, true, true")
    else:
        want["gqaw"], want["gqab"] = attn("gqaw", f"{tn}, true"), attn("gqab", f"{tn}, true")
    for fam, names in want.items():
        assert {n for n in ran if n.startswith(fam + "::") and "rope" not in n} == names, (fam, sorted(ran))
    assert {n for n in ran if "rope" in n} == {f"gqac::rope_heads_d256_kernel<{tn}, false>", f"gqac::rope_heads_d256_kernel<{tn}, true>"}, sorted(ran)
    ch = 2                                                            # 384 / 512 columns: at most 128 chunks of 4 fp32 = 2 per lane
    gk = {f"gemma_kernels::{k}<{tn}>" for k in ("geglu_tanh_fwd_kernel", "geglu_tanh_bwd_kernel")}
    gk |= {f"gemma_kernels::sandwich_fwd_kernel<{tn}, {ch}>", f"gemma_kernels::sandwich_bwd_kernel<{tn}, {ch}>"}
    assert {n for n in ran if n.startswith("gemma_kernels::")} == gk, sorted(ran)                    # and so no qknorm_rope kernel
    assert any(n.startswith(f"rmsnorm_fwd_kernel<{tn}") for n in ran)                  # the first layer's input norm
    assert not any(n.startswith(("wide::", "causal128::", "bidir::", "gqa::", "ln_", "attn_", "qknorm_rope_", "swiglu_", "mbert::", "d128::"))
                   for n in ran), sorted(ran)


def test_the_cases_are_not_vacuous():
    """HF float64 at L = 129 (one sequence): cap 4 against no cap and window 64 against window 512 change the hidden states."""
    ids = _tokens()[0][7:8]
    am = torch.ones(1, L, dtype=torch.long)

    def hidden(**kw):
        with torch.no_grad():
            return _make_plm("cap4", **kw).double().eval()(input_ids=ids, attention_mask=am).last_hidden_state
    base = hidden()
    for what, other in (("cap 4 vs no cap", hidden(attn_logit_softcapping=None)), ("window 64 vs 512", hidden(sliding_window=512))):
        d = float((base - other).norm() / other.norm())
        print(f"  {what}: rel l2 = {d:.2f} (must be >= 0.1)")
        assert d >= 0.1, what
    with torch.no_grad():
        fifty = _make_plm("cap50").double().eval()(input_ids=ids, attention_mask=am).last_hidden_state
        plain = _make_plm("cap50", attn_logit_softcapping=None).double().eval()(input_ids=ids, attention_mask=am).last_hidden_state
    print(f"  cap 50 vs no cap: rel l2 = {float((fifty - plain).norm() / plain.norm()):.1e} (fp32 budget 1e-05)")


@pytest.mark.parametrize("packed", [False, True], ids=["padded", "packed"])
@pytest.mark.parametrize("kind", MODELS)
def test_encoder_fp32_vs_hf_float64(dev, kind, packed):
    h = _hf(kind)
    box = {}
    ran = kernels_run(lambda: box.setdefault("r", _ours(h, dev, torch.float32, packed)))
    _assert_kernels(ran, kind, torch.float32)
    hs, valid, grads = box["r"]
    assert bool(torch.isfinite(hs).all())                         # padded rows included (those without a visible key: zeros)
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
    assert not any("q_norm" in n for n in ref_g) and any(n.endswith("pre_feedforward_layernorm.weight") for n in ref_g)


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
@pytest.mark.parametrize("kind", ("cap4", "cap50"))
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
    h = _hf("cap4")
    a = _ours(h, dev, torch.bfloat16, packed, checkpointing=False)
    b = _ours(h, dev, torch.bfloat16, packed, checkpointing=True)
    assert torch.equal(a[0], b[0])
    for n in a[2]:
        assert torch.equal(a[2][n], b[2][n]), n


def test_graph_text_lm_with_a_gemma2_encoder(dev):
    """Cornell-size graph (the construction of tests/test_gpu_gemma3.py) on the "cap50" model: one forward and backward through
    the packed pass, finite, the encoder's parameter gradients present, the soft-capped kernels and no other attention family;
    hipGraph capture of the encoder and the bucketed layout are refused as for every encoder outside BERT geometry."""
    import gmlm_amd
    import gmlm_oracle as O
    from gmlm_amd import gemma2
    h = _hf("cap50")
    n, e, f_in, c = O.WORKLOADS["cornell"]
    data = O.synthetic_graph("cornell")
    torch.manual_seed(5)
    m = gmlm_amd.GraphTextLM(f_in, 64, c, dropout_rate=0.0, plm_encoder=copy.deepcopy(h["plm"]), plm_max_length=24,
                             compute_dtype=torch.float32).to(dev).train()
    assert m._enc is gemma2 and m._has_packed_pass()
    g = torch.Generator().manual_seed(6)
    width = 24
    lens = torch.randint(4, width + 1, (n,), generator=g)
    am = (torch.arange(width)[None, :] < lens[:, None]).long()
    ids = torch.randint(1, 96, (n, width), generator=g) * am
    mask = data["active_mask"]
    x, ei, mk = data["x"].to(dev), data["edge_index"].to(dev), mask.to(dev)
    tokens = gmlm_amd.TokenizedTexts.from_mask(ids.to(dev), am.to(dev))
    y = data["y"].to(dev)
    box = {}
    ran = kernels_run(lambda: box.setdefault("logits", m(m.soft_mask_input(x, mk, 0.7), ei, tokens, mk, plm_batch_size=32)))
    assert any(k.startswith("gqac::fwd_kernel<float, true, false>") for k in ran) and any(k.startswith("gqac::rope_heads_d256_kernel<float, false>") for k in ran), ran
    assert not any(k.startswith(("gqaw::", "gqab::", "causal128::", "bidir::", "gqa::", "qknorm_rope_", "embed_sum_")) or "qknorm" in k for k in ran), ran
    logits = box["logits"]
    assert bool(torch.isfinite(logits).all())
    F.cross_entropy(logits[mk], y[mk], label_smoothing=0.2).backward()
    enc = {k: p.grad for k, p in m.named_parameters() if k.startswith("plm_encoder.")}
    assert enc and all(gr is not None and bool(torch.isfinite(gr).all()) for gr in enc.values())
    assert all(float(gr.abs().max()) > 0 for k, gr in enc.items()), [k for k, gr in enc.items() if float(gr.abs().max()) == 0]
    assert "plm_encoder.layers.1.self_attn.q_proj.weight" in m.state_dict() and not any("q_norm" in k for k in m.state_dict())
    # the pooled states are HF's: float64, eager attention, the reference's mean pooling
    with torch.no_grad():
        got = m.encode_texts(tokens, mk, plm_batch_size=32).double().cpu()
        hs = copy.deepcopy(h["plm"]).double().eval()(input_ids=ids[mask], attention_mask=am[mask]).last_hidden_state
    amf = am[mask].unsqueeze(-1).double()
    pooled = (hs * amf).sum(1) / amf.sum(1).clamp(min=1e-9)
    err = float((got[mask] - pooled).norm() / pooled.norm())
    print(f"  plm_embeds: rel l2 = {err:.2e} (budget 1e-05)")
    assert err <= 1e-5 and float(got[~mask].abs().max()) == 0.0
    with pytest.raises(NotImplementedError, match="BERT"):
        m.capture_hip_graphs(x, ei, encoder=True)
    m.plm_bucketed = True                                            # a BERT form: this encoder takes its plain packed pass instead
    with torch.no_grad():
        again = m.encode_texts(tokens, mk, plm_batch_size=32).double().cpu()
    assert torch.equal(again, got)
