"""The ModernBERT encoder pass (gmlm_amd.modernbert) and a GraphTextLM built on it against the installed
transformers.ModernBertModel in float64 on the CPU (eager attention), seeded random weights, norm weights drawn from
U(0.5, 1.5) so that they matter.

Tiny model: 4 layers (full, sliding, sliding, full: global_attn_every_n_layers = 3), hidden 128 = 2 heads x 64, intermediate
192, vocab 96; once with local_attention = 32 (|i - j| <= 16) and once with 128 (<= 64); nine sequences of 1..257 tokens (both
sides of every wave, key-tile and workgroup edge, and of both windows), train mode, loss = a fixed random projection of the
valid hidden states.  The float64 reference runs every sequence ALONE, unpadded, and adds the gradients up: HF's padded float64
run returns NaN on the valid rows of every padded sequence of this construction, the per-sequence run is finite.
fp32 budgets are the tree's model budgets (hidden states rel-L2 1e-5, every parameter gradient within 2e-3 of its norm).
The bf16 bound is measured, not fixed: HF's own model in bf16 on the CPU (the same per-sequence run) against float64 gives each
tensor's bf16 floor, and each tensor of this path must be within 2x that floor, exactly as for Qwen3 (test_gpu_qwen3.py)."""
import copy

import pytest
import torch
import torch.nn.functional as F

from helpers import kernels_run

pytestmark = pytest.mark.gpu

LENS = [1, 31, 33, 64, 65, 127, 128, 129, 257]
L = 257
P = 128


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _config(local_attention, max_pos=512):
    from transformers import ModernBertConfig
    cfg = ModernBertConfig(vocab_size=96, hidden_size=P, intermediate_size=192, num_hidden_layers=4, num_attention_heads=2,
                           max_position_embeddings=max_pos, local_attention=local_attention, global_attn_every_n_layers=3,
                           pad_token_id=None, bos_token_id=None, eos_token_id=None, cls_token_id=None, sep_token_id=None)
    cfg._attn_implementation = "eager"
    assert cfg.layer_types == ["full_attention", "sliding_attention", "sliding_attention", "full_attention"]
    assert cfg.sliding_window == local_attention // 2
    return cfg


def _make_plm(local_attention, seed=0):
    from transformers import ModernBertModel
    torch.manual_seed(seed)
    plm = ModernBertModel(_config(local_attention))
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for n, p in plm.named_parameters():
            if "norm" in n:
                p.copy_(torch.empty_like(p).uniform_(0.5, 1.5, generator=g))
            elif n == "embeddings.tok_embeddings.weight":
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


def _reference(local_attention):
    plm = _make_plm(local_attention)
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
    return dict(plm=plm, ids=ids, am=am, lens=lens, proj=proj, ref=ref, floors=floors, window=local_attention // 2)


@pytest.fixture(scope="module", params=[32, 128], ids=["w16", "w64"])
def hf(request):
    """The float64 reference and the bf16 / fp32 floors of HF's own model, computed once per window."""
    return _reference(request.param)


def _ours(plm, dev, cd, ids, lens, proj, checkpointing=False, packed=False):
    from gmlm_amd import modernbert
    m = copy.deepcopy(plm).to(dev).train()
    m.zero_grad()
    lens_d = lens.to(dev, torch.int32)
    if packed:
        am = torch.arange(ids.shape[1])[None, :] < lens[:, None]
        tok = ids[am].to(dev)
        pos = torch.cat([torch.arange(n) for n in lens.tolist()]).to(dev)
        cu = torch.tensor([0] + lens.cumsum(0).tolist(), dtype=torch.int32, device=dev)
        hs = valid_rows = modernbert.modernbert_encode_packed(m, tok, pos, cu, int(lens.max()), cd, True, checkpointing)
    else:
        hs = modernbert.modernbert_encode(m, ids.to(dev), lens_d, cd, True, checkpointing)
        valid_rows = hs[(torch.arange(ids.shape[1], device=dev)[None, :] < lens_d[:, None])]
    (valid_rows.double() * proj.to(dev)).sum().backward()
    return hs.detach(), valid_rows.detach().double().cpu(), {n: p.grad.detach().double().cpu() for n, p in m.named_parameters()}


def _assert_kernels(ran, tn, window_cuts=True):
    for k in ("mbert::add_ln_fwd_kernel", "mbert::add_ln_bwd_kernel", "mbert::geglu_fwd_kernel", "mbert::geglu_bwd_kernel"):
        assert any(n.startswith(k + "<" + tn) for n in ran), (k, sorted(ran))
    for inv in ("false", "true"):
        assert f"mbert::rope64_kernel<{tn}, {inv}>" in ran, sorted(ran)
    assert any(n.startswith("attn_") for n in ran), sorted(ran)                     # the full-attention layers: the BERT path's kernels
    windowed = {n for n in ran if n.startswith("mbert::window_")}
    if window_cuts:
        assert windowed == {f"mbert::window_{k}_kernel<{tn}>" for k in ("fwd", "delta", "dq", "dkv")}, sorted(ran)
    else:
        assert not windowed, sorted(windowed)
    assert not any(n.startswith(("rmsnorm_", "swiglu_", "causal128::", "qknorm_rope_", "ln_", "bias_gelu_")) for n in ran), sorted(ran)


def test_encoder_fp32_vs_hf_float64(dev, hf):
    box = {}
    ran = kernels_run(lambda: box.setdefault("r", _ours(hf["plm"], dev, torch.float32, hf["ids"], hf["lens"], hf["proj"])))
    _assert_kernels(ran, "float")
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
    printed per tensor (DESIGN.md section 4 "ModernBERT encoder")."""
    box = {}
    ran = kernels_run(lambda: box.setdefault("r", _ours(hf["plm"], dev, torch.bfloat16, hf["ids"], hf["lens"], hf["proj"])))
    _assert_kernels(ran, "unsigned short")
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


def test_short_batch_launches_no_band_limited_kernel(dev, hf):
    """Longest sequence <= window + 1: the band is vacuous, every layer takes the ``attention_qkv`` path, and the result is
    still HF's (which applies its sliding mask all the same)."""
    w = hf["window"]
    lens = torch.tensor([1, w, w + 1, w - 3])
    lmax = w + 1
    ids = hf["ids"][-4:, :lmax] * (torch.arange(lmax)[None, :] < lens[:, None])       # rows of >= 128 tokens, cut to the new lengths
    proj = torch.randn(int(lens.sum()), P, generator=torch.Generator().manual_seed(10), dtype=torch.float64) / 16
    ref_h, ref_g = _hf_run(hf["plm"], torch.float64, ids, lens, proj)
    for packed in (False, True):
        box = {}
        ran = kernels_run(lambda: box.setdefault("r", _ours(hf["plm"], dev, torch.float32, ids, lens, proj, packed=packed)))
        _assert_kernels(ran, "float", window_cuts=False)
        _, valid, grads = box["r"]
        assert float((valid - ref_h).norm() / ref_h.norm()) <= 1e-5
        for n, r in ref_g.items():
            assert float((grads[n] - r).norm() / r.norm()) <= 2e-3, n


def test_packed_and_padded_passes_agree(dev, hf):
    a = _ours(hf["plm"], dev, torch.float32, hf["ids"], hf["lens"], hf["proj"])
    box = {}
    ran = kernels_run(lambda: box.setdefault("r", _ours(hf["plm"], dev, torch.float32, hf["ids"], hf["lens"], hf["proj"], packed=True)))
    _assert_kernels(ran, "float")
    b = box["r"]
    assert b[0].shape == (sum(LENS), P)
    ref_h, ref_g = hf["ref"]
    e_pair, e_ref = float((a[1] - b[1]).norm() / a[1].norm()), float((b[1] - ref_h).norm() / ref_h.norm())
    per_token = float(((a[1] - b[1]).norm(dim=-1) / a[1].norm(dim=-1)).max())
    print(f"  packed vs padded: rel l2 = {e_pair:.2e}, worst token {per_token:.2e}; packed vs float64: {e_ref:.2e}")
    assert e_pair <= 1e-5 and per_token <= 1e-5 and e_ref <= 1e-5
    for n, r in ref_g.items():
        assert float((b[2][n] - r).norm() / r.norm()) <= 2e-3, n


@pytest.mark.parametrize("packed", [False, True], ids=["padded", "packed"])
@pytest.mark.parametrize("cd", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_gradient_checkpointing_is_bit_identical(dev, hf, cd, packed):
    a = _ours(hf["plm"], dev, cd, hf["ids"], hf["lens"], hf["proj"], checkpointing=False, packed=packed)
    b = _ours(hf["plm"], dev, cd, hf["ids"], hf["lens"], hf["proj"], checkpointing=True, packed=packed)
    assert torch.equal(a[0], b[0])
    for n in a[2]:
        assert torch.equal(a[2][n], b[2][n]), n


def test_bf16x3_gemms_run_the_same_chain(dev, hf):
    """gemm_precision "bf16x3" through ``prepare_weights``: fp32 storage, the four GEMMs of a layer on the bf16 matrix pipe."""
    from gmlm_amd import modernbert
    from gmlm_amd.dense import SplitWeight
    m = copy.deepcopy(hf["plm"]).to(dev).train()
    lws = modernbert.prepare_weights(m, torch.float32, "bf16x3")
    assert all(isinstance(getattr(lw, k), SplitWeight) for lw in lws for k in ("wqkv", "wo", "wi", "wmo"))
    lens_d = hf["lens"].to(dev, torch.int32)
    hs = modernbert.modernbert_encode(m, hf["ids"].to(dev), lens_d, torch.float32, True, False, lws)
    valid = hs[(torch.arange(L, device=dev)[None, :] < lens_d[:, None])].double().cpu()
    e = float((valid - hf["ref"][0]).norm() / hf["ref"][0].norm())
    print(f"  bf16x3 hidden: rel l2 = {e:.2e}")
    assert e <= 1e-4                                              # 3 * 2^-16 per product (dense.mm_bf16x3), four GEMMs x four layers


def _graph_model(plm, dev, cd, max_len):
    import gmlm_amd
    import gmlm_oracle as O
    name, hc = "cornell", 64
    n, e, f_in, c = O.WORKLOADS[name]
    data = O.synthetic_graph(name)
    torch.manual_seed(5)
    m = gmlm_amd.GraphTextLM(f_in, hc, c, dropout_rate=0.0, plm_encoder=plm, plm_max_length=max_len, compute_dtype=cd)
    return m.to(dev).train(), data, n


def test_graph_text_lm_with_a_modernbert_encoder(dev, hf):
    """Cornell-size graph (the construction of test_gpu_qwen3.py): plm_embeds against HF float64 (one unpadded sequence at a
    time) + the reference's mean pooling (main.py:351-358), inactive rows exactly 0, then forward + CE loss + backward with a
    finite gradient for every parameter, and a strict state-dict round trip."""
    import gmlm_amd
    plm = copy.deepcopy(hf["plm"])
    m, data, n = _graph_model(plm, dev, torch.float32, 40)
    g = torch.Generator().manual_seed(6)
    width = 40                                                    # past both 16 + 1 and (for w = 64) below 64 + 1: both routes over the two fixtures
    lens = torch.randint(4, width + 1, (n,), generator=g)
    lens[0] = width
    am = (torch.arange(width)[None, :] < lens[:, None]).long()
    ids = torch.randint(1, 96, (n, width), generator=g) * am
    mask = data["active_mask"]
    x, ei, mk = data["x"].to(dev), data["edge_index"].to(dev), mask.to(dev)
    tokens = gmlm_amd.TokenizedTexts.from_mask(ids.to(dev), am.to(dev))

    ref = copy.deepcopy(hf["plm"]).double().eval()
    with torch.no_grad():
        pooled = torch.stack([ref(input_ids=ids[i:i + 1, :int(lens[i])]).last_hidden_state[0].mean(0)
                              for i in mask.nonzero().flatten().tolist()])
    box = {}
    with torch.no_grad():
        ran = kernels_run(lambda: box.setdefault("p", m.encode_texts(tokens, mk, plm_batch_size=32)))
    assert any(k.startswith("mbert::add_ln_fwd_kernel<float") for k in ran) and any(k.startswith("meanpool_fwd_kernel") for k in ran), ran
    assert any(k.startswith("mbert::window_fwd_kernel<float>") for k in ran) == (width > hf["window"] + 1), sorted(ran)
    assert not any(k.startswith(("embed_sum_", "causal128::", "rmsnorm_")) for k in ran), ran
    got = box["p"].double().cpu()
    e = float((got[mask] - pooled).norm() / pooled.norm())
    print(f"  plm_embeds: rel l2 = {e:.2e}")
    assert e <= 1e-5 and float(got[~mask].abs().max()) == 0.0

    logits = m(m.soft_mask_input(x, mk, 0.7), ei, tokens, mk, plm_batch_size=32)
    loss = F.cross_entropy(logits[mk], data["y"].to(dev)[mk], label_smoothing=0.2)
    loss.backward()
    assert bool(torch.isfinite(loss))
    for k, p in m.named_parameters():
        if p.grad is not None:
            assert bool(torch.isfinite(p.grad).all()), k
        if k.startswith(("plm_encoder.", "graph_to_text_attn.", "text_to_graph_attn.")):
            assert p.grad is not None and float(p.grad.abs().max()) > 0, k
    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    m2, _, _ = _graph_model(_make_plm(2 * hf["window"], seed=7), dev, torch.float32, 40)
    m2.load_state_dict(sd, strict=True)
    assert all(torch.equal(v, sd[k]) for k, v in m2.state_dict().items())
    assert "plm_encoder.layers.1.attn.Wqkv.weight" in sd and "plm_encoder.final_norm.weight" in sd
