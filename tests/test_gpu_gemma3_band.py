"""The Gemma3 text encoder with ``band=True`` on sequences PAST ``sliding_window`` (gmlm_amd.gemma3, the gqab:: kernels of
csrc/attn_gqa_band.hip on the sliding layers, gqaw:: on the full layer), padded and packed, and a GraphTextLM with
``plm_band_attention``, against the installed transformers ``Gemma3TextModel`` in float64 on the CPU (eager attention).

The two three-layer models of tests/test_gpu_gemma3.py (its ``_config`` / ``_make_plm``) with ``sliding_window=40``: the causal
model keeps 40, the bidirectional config turns it into 21.  Layer pattern 3: two sliding layers and one full layer.  Eight
sequences of 1, 21, 22, 40, 41, 64, 65 and 77 tokens in a width of 80: below, on and past each window and across the 32- and 64-row
tile edges.  Train mode, loss = a fixed random projection of the valid hidden states.  fp32 budgets are that file's (hidden
states rel-L2 1e-5, every parameter gradient within 2e-3 of its norm); the bf16 bound is twice the floor of HF's own bf16 run on
the same batch, as there."""
import copy

import pytest
import torch

from helpers import kernels_run
from test_gpu_gemma3 import TN, _config, _make_plm

pytestmark = pytest.mark.gpu

LENS = [1, 21, 22, 40, 41, 64, 65, 77]
L = 80
WINDOW = {"causal": 40, "bidir": 21}
MODELS = ("bidir", "causal")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _tokens(lens, width, seed=3):
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(1, 96, (len(lens), width), generator=g)
    lens = torch.tensor(lens)
    am = (torch.arange(width)[None, :] < lens[:, None]).long()
    return ids * am, am, lens


def _hf_run(plm, dtype, ids, lens, proj):
    """HF forward + backward in ``dtype`` on the CPU, one sequence per call and without padding, the gradients summed over the
    calls -> (valid hidden states [T, P], {name: grad}) as float64: test_gpu_gemma3._hf_run's computation.  Not one padded batch as
    there: HF's eager attention takes the softmax in float32, where the float64 mask value is -inf, so a padded query past
    kv_len + window - 1 (no visible key; that file has none) becomes NaN and reaches the valid rows of the next layer as 0 * NaN."""
    m = copy.deepcopy(plm).to(dtype).train()
    m.zero_grad()
    rows, r0 = [], 0
    for b, n in enumerate(int(x) for x in lens):
        hs = m(input_ids=ids[b:b + 1, :n], attention_mask=torch.ones(1, n, dtype=torch.long)).last_hidden_state[0]
        (hs.double() * proj[r0:r0 + n]).sum().backward()
        rows.append(hs.detach().double())
        r0 += n
    return torch.cat(rows), {n: p.grad.detach().double() for n, p in m.named_parameters()}


_HF = {}


def _hf(kind):
    """The float64 reference and the bf16 floor of HF's own model on the long batch, computed once per model and left unchanged."""
    if kind not in _HF:
        plm = _make_plm(kind, sliding_window=40)
        assert plm.config.sliding_window == WINDOW[kind] and _config(kind, sliding_window=40).sliding_window == WINDOW[kind]
        assert list(plm.config.layer_types) == ["sliding_attention", "sliding_attention", "full_attention"]
        ids, am, lens = _tokens(LENS, L)
        proj = torch.randn(int(am.sum()), plm.config.hidden_size, generator=torch.Generator().manual_seed(9), dtype=torch.float64) / 16
        ref = _hf_run(plm, torch.float64, ids, lens, proj)
        hs, gr = _hf_run(plm, torch.bfloat16, ids, lens, proj)
        assert bool(torch.isfinite(ref[0]).all()) and all(bool(torch.isfinite(t).all()) for t in ref[1].values())
        floor = {"hidden": float((hs - ref[0]).norm() / ref[0].norm())}
        floor.update({n: float((gr[n] - ref[1][n]).norm() / ref[1][n].norm()) for n in gr})
        _HF[kind] = dict(plm=plm, ids=ids, am=am, lens=lens, proj=proj, ref=ref, floor=floor)
    return _HF[kind]


def _ours(plm, ids, am, lens, proj, dev, cd, packed, band, checkpointing=False):
    from gmlm_amd import gemma3
    m = copy.deepcopy(plm).to(dev).train()
    m.zero_grad()
    width = ids.shape[1]
    lens_d = lens.to(dev, torch.int32)
    if packed:
        tok = ids[am.bool()].to(dev)
        pos = torch.cat([torch.arange(int(n)) for n in lens]).to(dev)
        cu = torch.tensor([0] + lens.tolist()).cumsum(0).to(dev, torch.int32)
        hs = valid = gemma3.gemma3_encode_packed(m, tok, pos, cu, int(lens.max()), cd, True, checkpointing, band=band)
    else:
        hs = gemma3.gemma3_encode(m, ids.to(dev), lens_d, cd, True, checkpointing, band=band)
        valid = hs[(torch.arange(width, device=dev)[None, :] < lens_d[:, None])]
    (valid.double() * proj.to(dev)).sum().backward()
    return hs.detach(), valid.detach().double().cpu(), {n: p.grad.detach().double().cpu() for n, p in m.named_parameters()}


def _long(h, dev, cd, packed, checkpointing=False):
    return _ours(h["plm"], h["ids"], h["am"], h["lens"], h["proj"], dev, cd, packed, True, checkpointing)


def _assert_kernels(ran, kind, dtype):
    """the four gqab:: kernels of this (mask, dtype) for the sliding layers and the four gqaw:: ones for the full layer"""
    tn, c = TN[dtype], "true" if kind == "causal" else "false"
    for ns in ("gqab", "gqaw"):
        want = {f"{ns}::fwd_kernel<{tn}, {c}>", f"{ns}::delta_kernel<{tn}>", f"{ns}::dq_kernel<{tn}, {c}>", f"{ns}::dkv_kernel<{tn}, {c}>"}
        assert {n for n in ran if n.startswith(ns + "::")} == want, sorted(ran)


@pytest.mark.parametrize("packed", [False, True], ids=["padded", "packed"])
@pytest.mark.parametrize("kind", MODELS)
def test_banded_encoder_fp32_vs_hf_float64(dev, kind, packed):
    h = _hf(kind)
    box = {}
    ran = kernels_run(lambda: box.setdefault("r", _long(h, dev, torch.float32, packed)))
    _assert_kernels(ran, kind, torch.float32)
    hs, valid, grads = box["r"]
    assert bool(torch.isfinite(hs).all())                         # padded rows included: some see no key in the sliding layers
    ref_h, ref_g = h["ref"]
    e = float((valid - ref_h).norm() / ref_h.norm())
    print(f"  hidden: rel l2 = {e:.2e} (budget 1e-05)")
    assert e <= 1e-5
    assert set(grads) == set(ref_g)
    for n, r in ref_g.items():
        e = float((grads[n] - r).norm() / r.norm())
        print(f"  {n}: rel l2 = {e:.2e} (budget 2e-03)")
        assert float(r.norm()) > 0 and e <= 2e-3, (n, e)


def test_the_band_matters_on_this_batch():
    """HF float64 with the window against HF float64 with a window that covers the batch: the hidden states differ by far more
    than any budget above, so a pass that ignored the window could not meet them."""
    for kind in MODELS:
        h = _hf(kind)
        wide = _make_plm(kind, sliding_window=512)
        got = _hf_run(wide, torch.float64, h["ids"], h["lens"], h["proj"])[0]
        e = float((got - h["ref"][0]).norm() / h["ref"][0].norm())
        print(f"  {kind}: un-banded vs banded HF float64 hidden states rel l2 = {e:.2e}")
        assert e >= 1e-2


@pytest.mark.parametrize("packed", [False, True], ids=["padded", "packed"])
@pytest.mark.parametrize("kind", MODELS)
def test_banded_encoder_bf16_within_twice_the_hf_bf16_floor(dev, kind, packed):
    h = _hf(kind)
    box = {}
    ran = kernels_run(lambda: box.setdefault("r", _long(h, dev, torch.bfloat16, packed)))
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
@pytest.mark.parametrize("kind", MODELS)
def test_a_batch_under_the_window_is_todays_pass_bit_for_bit(dev, kind, packed):
    """Longest sequence = the window: ``band=True`` launches no gqab:: kernel and gives the bytes of ``band=False``."""
    h = _hf(kind)
    w = WINDOW[kind]
    ids, am, lens = _tokens([1, w, w // 2, w - 1], w, seed=4)
    proj = torch.randn(int(am.sum()), h["plm"].config.hidden_size, generator=torch.Generator().manual_seed(2), dtype=torch.float64) / 16
    box = {}
    ran = kernels_run(lambda: box.setdefault("r", _ours(h["plm"], ids, am, lens, proj, dev, torch.bfloat16, packed, True)))
    assert not any(n.startswith("gqab::") for n in ran) and any(n.startswith("gqaw::fwd_kernel") for n in ran), sorted(ran)
    a, b = box["r"], _ours(h["plm"], ids, am, lens, proj, dev, torch.bfloat16, packed, False)
    assert torch.equal(a[0], b[0])
    for n in a[2]:
        assert torch.equal(a[2][n], b[2][n]), n


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("kind", MODELS)
def test_banded_packed_pass_is_the_padded_pass(dev, kind, dtype):
    """The same rows through both layouts agree to the budgets above (fp32: 1e-5 / 2e-3; bf16: twice the HF floor of the tensor)."""
    h = _hf(kind)
    a, b = _long(h, dev, dtype, False), _long(h, dev, dtype, True)
    fl = h["floor"]
    e = float((a[1] - b[1]).norm() / a[1].norm())
    print(f"  hidden: padded vs packed rel l2 = {e:.2e}")
    assert e <= (1e-5 if dtype == torch.float32 else 2 * fl["hidden"])
    for n in a[2]:
        e = float((a[2][n] - b[2][n]).norm() / a[2][n].norm())
        assert e <= (2e-3 if dtype == torch.float32 else 2 * fl[n]), (n, e)


@pytest.mark.parametrize("packed", [False, True], ids=["padded", "packed"])
def test_banded_gradient_checkpointing_is_bit_identical(dev, packed):
    h = _hf("bidir")
    a = _long(h, dev, torch.bfloat16, packed, checkpointing=False)
    b = _long(h, dev, torch.bfloat16, packed, checkpointing=True)
    assert torch.equal(a[0], b[0])
    for n in a[2]:
        assert torch.equal(a[2][n], b[2][n]), n


def test_graph_text_lm_with_band_attention(dev):
    """Cornell-size graph on the bidirectional model (window 21), texts of up to 48 tokens: with ``plm_band_attention`` the
    forward runs on gqab::fwd_kernel<float, false> and the pooled text states are HF's in float64; with the attribute off (the
    default) the same call raises the refusal."""
    import gmlm_amd
    import gmlm_oracle as O
    h = _hf("bidir")
    n, e, f_in, c = O.WORKLOADS["cornell"]
    data = O.synthetic_graph("cornell")
    torch.manual_seed(5)
    m = gmlm_amd.GraphTextLM(f_in, 64, c, dropout_rate=0.0, plm_encoder=copy.deepcopy(h["plm"]), plm_max_length=48,
                             compute_dtype=torch.float32).to(dev).train()
    assert m.plm_band_attention is False
    g = torch.Generator().manual_seed(6)
    width = 48
    lens = torch.randint(4, width + 1, (n,), generator=g)
    lens[0] = width
    am = (torch.arange(width)[None, :] < lens[:, None]).long()
    ids = torch.randint(1, 96, (n, width), generator=g) * am
    mask = data["active_mask"].clone()
    mask[0] = True                                                   # the longest text is encoded
    x, ei, mk = data["x"].to(dev), data["edge_index"].to(dev), mask.to(dev)
    tokens = gmlm_amd.TokenizedTexts.from_mask(ids.to(dev), am.to(dev))
    with pytest.raises(ValueError, match="exceeds sliding_window 21: there is no band kernel at head dim 256"):
        m(m.soft_mask_input(x, mk, 0.7), ei, tokens, mk, plm_batch_size=n)
    m.plm_band_attention = True
    box = {}
    ran = kernels_run(lambda: box.setdefault("logits", m(m.soft_mask_input(x, mk, 0.7), ei, tokens, mk, plm_batch_size=n)))
    assert any(k.startswith("gqab::fwd_kernel<float, false>") for k in ran) and any(k.startswith("gqaw::fwd_kernel<float, false>") for k in ran), ran
    logits = box["logits"]
    assert bool(torch.isfinite(logits).all())
    logits.float().sum().backward()
    assert all(bool(torch.isfinite(p.grad).all()) for p in m.parameters() if p.grad is not None)
    assert m.plm_encoder.layers[0].self_attn.q_proj.weight.grad is not None
    ref_plm = copy.deepcopy(h["plm"]).double().eval()
    with torch.no_grad():                                            # one text per call, unpadded (see _hf_run); the reference's mean pooling
        pooled = torch.stack([ref_plm(input_ids=ids[i:i + 1, :int(lens[i])]).last_hidden_state[0].mean(0) for i in mask.nonzero()[:, 0]])
        got = m.encode_texts(tokens, mk, plm_batch_size=n).double().cpu()
    err = float((got[mask] - pooled).norm() / pooled.norm())
    print(f"  plm_embeds: rel l2 = {err:.2e} (budget 1e-05)")
    assert err <= 1e-5 and float(got[~mask].abs().max()) == 0.0
