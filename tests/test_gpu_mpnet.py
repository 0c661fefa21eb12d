"""The MPNet encoder pass (gmlm_amd.mpnet) and a GraphTextLM built on it against the installed transformers.MPNetModel in float64
on the CPU, seeded random weights, LayerNorm weights drawn from U(0.5, 1.5) and ``encoder.relative_attention_bias`` from N(0, 1)
so that both matter.

Tiny model: 3 layers, hidden 128 = 2 heads x 64, intermediate 192, vocab 96, max_position_embeddings 514, dropouts 0; nine
sequences of 1..257 tokens (both sides of every wave, key-tile and workgroup edge, and of the bucket saturation at |rel| = 91),
token ids >= 2 (1 is MPNet's pad id), train mode, loss = a fixed random projection of the valid hidden states.  The float64
reference runs every sequence ALONE, unpadded, and adds the gradients up, as tests/test_gpu_modernbert.py does (for this model
HF's padded float64 run equals it exactly; either form is finite).
fp32 budgets are the tree's model budgets: hidden states rel-L2 1e-5, every parameter gradient within 2e-3 of its norm,
``encoder.relative_attention_bias.weight`` and the position rows included.  The bf16 bound is measured, not fixed: HF's own model
in bf16 on the CPU (the same per-sequence run) against float64 gives each tensor's bf16 floor, and each tensor of this path must
be within 2x that floor.
The key biases (``attention.attn.k.bias``) have a gradient that is mathematically zero (a constant added to every score of a
row leaves the softmax as it is), so the float64 value is rounding noise (1e-15) and no relative error exists: in fp32 their
gradient must stay within 2e-3 of the norm of the same layer's q.bias gradient (the same sums of dS against q instead of k), and
the bf16 comparison leaves them out, as tests/test_gpu_d32_encoder.py does.
One GraphTextLM step on a Cornell-size graph: logits and the gradient of the bias parameter against the SAME model with its
text embeddings taken from HF's encoder in float64 (autograd through HF into that parameter).  Budgets: the bias gradient the
2e-3 of the encoder test; the logits 1e-4 rel-L2, ten times the 1e-5 of the text embeddings that enter the head (two
cross-attentions, a LayerNorm and two small MLPs in fp32 behind them).  With the config's dropouts at 0.1 / 0.1 the step is
finite and two steps from the same seeds are bit-equal."""
import copy

import pytest
import torch
import torch.nn.functional as F

from helpers import kernels_run

pytestmark = pytest.mark.gpu

LENS = [1, 31, 33, 64, 65, 127, 128, 129, 257]
L = 257
P = 128
PAD = 1
BIAS = "encoder.relative_attention_bias.weight"


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _config(**kw):
    from transformers import MPNetConfig
    base = dict(vocab_size=96, hidden_size=P, intermediate_size=192, num_hidden_layers=3, num_attention_heads=2,
                max_position_embeddings=514, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)
    base.update(kw)
    return MPNetConfig(**base)


def _make_plm(seed=0, **kw):
    from transformers import MPNetModel
    torch.manual_seed(seed)
    plm = MPNetModel(_config(**kw), add_pooling_layer=False)
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for n, p in plm.named_parameters():
            if "LayerNorm.weight" in n:
                p.copy_(torch.empty_like(p).uniform_(0.5, 1.5, generator=g))
            elif "embeddings" in n or n == BIAS or p.dim() == 1:
                p.copy_(torch.randn(p.shape, generator=g) * (1.0 if p.dim() == 2 else 0.1))
            else:
                p.copy_(torch.randn(p.shape, generator=g) * p.shape[1] ** -0.5)
    return plm.train()


def _tokens(seed=3):
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(2, 96, (len(LENS), L), generator=g)
    lens = torch.tensor(LENS)
    am = torch.arange(L)[None, :] < lens[:, None]
    return torch.where(am, ids, torch.full_like(ids, PAD)), am.long(), lens


def _hf_run(plm, dtype, ids, lens, proj):
    """HF forward + backward in ``dtype`` on the CPU, one unpadded sequence at a time, gradients accumulated ->
    (valid hidden states [T, P], {name: grad}) as float64."""
    m = copy.deepcopy(plm).to(dtype).train()
    m.zero_grad()
    rows, t0 = [], 0
    for i, n in enumerate(lens.tolist()):
        hs = m(input_ids=ids[i:i + 1, :n]).last_hidden_state[0]
        (hs.double() * proj[t0:t0 + n]).sum().backward()
        rows.append(hs.detach().double())
        t0 += n
    return torch.cat(rows), {n: p.grad.detach().double() for n, p in m.named_parameters()}


@pytest.fixture(scope="module")
def hf():
    """The float64 reference and the bf16 / fp32 floors of HF's own model, computed once."""
    plm = _make_plm()
    ids, am, lens = _tokens()
    proj = torch.randn(int(am.sum()), P, generator=torch.Generator().manual_seed(9), dtype=torch.float64) / 16
    ref = _hf_run(plm, torch.float64, ids, lens, proj)
    assert bool(torch.isfinite(ref[0]).all()) and all(bool(torch.isfinite(g).all()) for g in ref[1].values())
    floors = {}
    for dt in (torch.bfloat16, torch.float32):
        hs, gr = _hf_run(plm, dt, ids, lens, proj)
        fl = {"hidden": float((hs - ref[0]).norm() / ref[0].norm())}
        fl.update({n: float((gr[n] - ref[1][n]).norm() / ref[1][n].norm()) for n in gr})
        floors[dt] = fl
    return dict(plm=plm, ids=ids, am=am, lens=lens, proj=proj, ref=ref, floors=floors)


def _ours(plm, dev, cd, ids, lens, proj, checkpointing=False, packed=False):
    from gmlm_amd import mpnet
    m = copy.deepcopy(plm).to(dev).train()
    m.zero_grad()
    lens_d = lens.to(dev, torch.int32)
    if packed:
        am = torch.arange(ids.shape[1])[None, :] < lens[:, None]
        tok = ids[am].to(dev)
        pos = torch.cat([torch.arange(n) for n in lens.tolist()]).to(dev)
        cu = torch.tensor([0] + lens.cumsum(0).tolist(), dtype=torch.int32, device=dev)
        hs = valid_rows = mpnet.mpnet_encode_packed(m, tok, pos, cu, int(lens.max()), cd, True, checkpointing)
    else:
        hs = mpnet.mpnet_encode(m, ids.to(dev), lens_d, cd, True, checkpointing)
        valid_rows = hs[(torch.arange(ids.shape[1], device=dev)[None, :] < lens_d[:, None])]
    (valid_rows.double() * proj.to(dev)).sum().backward()
    return hs.detach(), valid_rows.detach().double().cpu(), {n: p.grad.detach().double().cpu() for n, p in m.named_parameters()}


def _assert_kernels(ran, tn, packed):
    want = {f"relb::{k}_kernel<{tn}, false>" for k in ("fwd", "dq", "dkv", "dbias")} | {f"relb::delta_kernel<{tn}>", "relb::dbias_sum_kernel"}
    assert {n for n in ran if n.startswith("relb::")} == want, sorted(ran)
    assert not any(n.startswith(("attn_", "d32::", "d128::", "mbert::", "causal128::", "rmsnorm_", "swiglu_")) for n in ran), sorted(ran)
    assert any(n.startswith("embed_sum_") for n in ran) == packed, sorted(ran)


@pytest.mark.parametrize("packed", [False, True], ids=["padded", "packed"])
def test_encoder_fp32_vs_hf_float64(dev, hf, packed):
    box = {}
    ran = kernels_run(lambda: box.setdefault("r", _ours(hf["plm"], dev, torch.float32, hf["ids"], hf["lens"], hf["proj"], packed=packed)))
    _assert_kernels(ran, "float", packed)
    hs, valid, grads = box["r"]
    assert bool(torch.isfinite(hs).all())                         # padded rows included
    assert hs.shape == ((sum(LENS), P) if packed else (len(LENS), L, P))
    ref_h, ref_g = hf["ref"]
    e = float((valid - ref_h).norm() / ref_h.norm())
    print(f"  hidden: rel l2 = {e:.2e} (HF fp32 floor {hf['floors'][torch.float32]['hidden']:.2e})")
    assert e <= 1e-5
    assert set(grads) == set(ref_g) and BIAS in ref_g and "embeddings.position_embeddings.weight" in ref_g
    for n, r in ref_g.items():
        if n.endswith("attn.k.bias"):                             # mathematically zero (module docstring): absolute, against q.bias
            yard = float(ref_g[n.replace("attn.k.bias", "attn.q.bias")].norm())
            print(f"  {n}: |grad| = {float(grads[n].norm()):.2e} (float64 {float(r.norm()):.2e}; q.bias gradient {yard:.2e})")
            assert float(r.norm()) <= 1e-12 * yard and float(grads[n].norm()) <= 2e-3 * yard, n
            continue
        e = float((grads[n] - r).norm() / r.norm())
        print(f"  {n}: rel l2 = {e:.2e} (HF fp32 floor {hf['floors'][torch.float32][n]:.2e})")
        assert float(r.norm()) > 0 and e <= 2e-3, (n, e)
    pos_g = grads["embeddings.position_embeddings.weight"]
    assert float(pos_g[:PAD + 1].abs().sum()) == 0.0 and float(pos_g[PAD + 1 + L:].abs().sum()) == 0.0 and float(pos_g[PAD + 1 + L - 1].abs().max()) > 0


@pytest.mark.parametrize("packed", [False, True], ids=["padded", "packed"])
def test_encoder_bf16_within_twice_the_hf_bf16_floor(dev, hf, packed):
    """Every tensor (valid hidden states, each parameter gradient) within 2x the error of HF's own bf16 run; the ratios are
    printed per tensor (DESIGN.md section 4 "MPNet encoder")."""
    box = {}
    ran = kernels_run(lambda: box.setdefault("r", _ours(hf["plm"], dev, torch.bfloat16, hf["ids"], hf["lens"], hf["proj"], packed=packed)))
    _assert_kernels(ran, "unsigned short", packed)
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
        if n.endswith("attn.k.bias"):                             # mathematically zero: no relative error on either side
            continue
        e = float((grads[n] - r).norm() / r.norm())
        print(f"  {n}: rel l2 = {e:.2e}, HF bf16 floor {fl[n]:.2e}, ratio {e / fl[n]:.2f}")
        if e > 2 * fl[n]:
            bad.append((n, e, fl[n]))
    assert not bad, bad


@pytest.mark.parametrize("packed", [False, True], ids=["padded", "packed"])
@pytest.mark.parametrize("cd", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_gradient_checkpointing_is_bit_identical(dev, hf, cd, packed):
    a = _ours(hf["plm"], dev, cd, hf["ids"], hf["lens"], hf["proj"], checkpointing=False, packed=packed)
    b = _ours(hf["plm"], dev, cd, hf["ids"], hf["lens"], hf["proj"], checkpointing=True, packed=packed)
    assert torch.equal(a[0], b[0])
    for n in a[2]:
        assert torch.equal(a[2][n], b[2][n]), n


def _graph_model(plm, dev, cd, max_len, dropout_rate=0.0):
    import gmlm_amd
    import gmlm_oracle as O
    name, hc = "cornell", 64
    n, e, f_in, c = O.WORKLOADS[name]
    data = O.synthetic_graph(name)
    torch.manual_seed(5)
    m = gmlm_amd.GraphTextLM(f_in, hc, c, dropout_rate=dropout_rate, plm_encoder=plm, plm_max_length=max_len, compute_dtype=cd)
    return m.to(dev).train(), data, n


def _graph_inputs(data, n, dev, width=40):
    import gmlm_amd
    g = torch.Generator().manual_seed(6)
    lens = torch.randint(4, width + 1, (n,), generator=g)
    lens[0] = width
    am = torch.arange(width)[None, :] < lens[:, None]
    ids = torch.where(am, torch.randint(2, 96, (n, width), generator=g), torch.full((n, width), PAD))
    tokens = gmlm_amd.TokenizedTexts.from_mask(ids.to(dev), am.long().to(dev))
    return ids, lens, tokens


def test_graph_text_lm_step_vs_the_same_model_on_hf_float64(dev, hf):
    plm = copy.deepcopy(hf["plm"])
    m, data, n = _graph_model(plm, dev, torch.float32, 40)
    ids, lens, tokens = _graph_inputs(data, n, dev)
    mask = data["active_mask"]
    x, ei, mk, y = data["x"].to(dev), data["edge_index"].to(dev), mask.to(dev), data["y"].to(dev)

    box = {}
    ran = kernels_run(lambda: box.setdefault("l", m(m.soft_mask_input(x, mk, 0.7), ei, tokens, mk, plm_batch_size=32)))
    assert "relb::fwd_kernel<float, false>" in ran and any(k.startswith("embed_sum_") for k in ran), sorted(ran)
    logits = box["l"]
    F.cross_entropy(logits[mk], y[mk], label_smoothing=0.2).backward()
    got_g = m.plm_encoder.encoder.relative_attention_bias.weight.grad.detach().double().cpu()

    # the same model, its text embeddings from HF's encoder in float64 on the CPU (mean pooling of main.py:351-358)
    ref_plm = copy.deepcopy(hf["plm"]).double().train()
    active = mask.nonzero().flatten().tolist()
    pooled = torch.stack([ref_plm(input_ids=ids[i:i + 1, :int(lens[i])]).last_hidden_state[0].mean(0) for i in active])
    embeds = torch.zeros(n, P, dtype=torch.float64).index_put((mask.nonzero().flatten(),), pooled)
    m.zero_grad()
    ref_logits = m.head(m.get_graph_embeddings(m.soft_mask_input(x, mk, 0.7), ei), embeds.to(dev).float())
    F.cross_entropy(ref_logits[mk], y[mk], label_smoothing=0.2).backward()
    ref_g = ref_plm.encoder.relative_attention_bias.weight.grad

    e_l = float((logits.detach().double() - ref_logits.detach().double()).norm() / ref_logits.detach().double().norm())
    e_g = float((got_g - ref_g).norm() / ref_g.norm())
    print(f"  logits: rel l2 = {e_l:.2e}; {BIAS} gradient: rel l2 = {e_g:.2e}")
    assert float(ref_g.norm()) > 0 and e_l <= 1e-4 and e_g <= 2e-3
    sd = m.state_dict()
    assert "plm_encoder." + BIAS in sd and "plm_encoder.encoder.layer.2.attention.attn.q.weight" in sd


def test_graph_text_lm_step_with_dropout_is_finite_and_replayable(dev):
    """hidden_dropout_prob = attention_probs_dropout_prob = 0.1 (MPNet's defaults): finite, and bit-equal from equal seeds."""
    plm = _make_plm(hidden_dropout_prob=0.1, attention_probs_dropout_prob=0.1)
    m, data, n = _graph_model(plm, dev, torch.float32, 40)
    _, _, tokens = _graph_inputs(data, n, dev)
    mk = data["active_mask"].to(dev)
    x, ei, y = data["x"].to(dev), data["edge_index"].to(dev), data["y"].to(dev)
    runs = []
    for _ in range(2):
        torch.manual_seed(11)
        m.zero_grad()
        box = {}
        ran = kernels_run(lambda: box.setdefault("l", m(m.soft_mask_input(x, mk, 0.7), ei, tokens, mk, plm_batch_size=32)))
        assert "relb::fwd_kernel<float, true>" in ran, sorted(ran)
        logits = box["l"]
        loss = F.cross_entropy(logits[mk], y[mk], label_smoothing=0.2)
        loss.backward()
        grads = {k: p.grad.detach().clone() for k, p in m.plm_encoder.named_parameters()}
        assert bool(torch.isfinite(loss)) and all(bool(torch.isfinite(g).all()) for g in grads.values())
        assert float(grads[BIAS].abs().max()) > 0
        runs.append((logits.detach().clone(), grads))
    assert torch.equal(runs[0][0], runs[1][0])
    for k in runs[0][1]:
        assert torch.equal(runs[0][1][k], runs[1][1][k]), k
    torch.manual_seed(12)
    other = m(m.soft_mask_input(x, mk, 0.7), ei, tokens, mk, plm_batch_size=32)
    assert not torch.equal(other, runs[0][0])                      # another seed, another mask
