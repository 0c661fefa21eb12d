"""The packed (variable-length) Qwen3 encoder pass (qwen3.qwen3_encode_packed) and the GraphTextLM route built on it, against
the installed transformers.Qwen3Model in float64 on the CPU.  Tiny model, token set, float64 reference and bf16 / fp32
floors are those of test_gpu_qwen3.py (2 layers, hidden 256, 4 / 2 heads x 128; nine sequences of 1..257 tokens); the bars
are the padded tests': fp32 rel-L2 <= 1e-5 on the hidden states and <= 2e-3 per gradient, bf16 within 2x HF's own bf16 error."""
import copy

import pytest
import torch
import torch.nn.functional as F

from helpers import kernels_run
from test_gpu_qwen3 import LENS, _assert_qwen3_kernels, _graph_model, hf  # noqa: F401  (hf: the module-scoped fixture)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _packed_inputs(ids, am, lens, dev):
    tok = ids[am.bool()].to(dev)                                  # row-major: the sequences back to back
    pos = torch.cat([torch.arange(int(n)) for n in lens]).to(dev)
    cu = torch.cat([torch.zeros(1, dtype=torch.long), lens.long().cumsum(0)]).to(dev, torch.int32)
    return tok, pos, cu, int(lens.max())


def _ours(plm, dev, cd, h, checkpointing=False):
    from gmlm_amd import qwen3
    m = copy.deepcopy(plm).to(dev).train()
    m.zero_grad()
    tok, pos, cu, max_len = _packed_inputs(h["ids"], h["am"], h["lens"], dev)
    hs = qwen3.qwen3_encode_packed(m, tok, pos, cu, max_len, cd, True, checkpointing)
    assert tuple(hs.shape) == (sum(LENS), 256) and hs.dtype == cd
    (hs.double() * h["proj"].to(dev)).sum().backward()
    return hs.detach(), hs.detach().double().cpu(), {n: p.grad.detach().double().cpu() for n, p in m.named_parameters()}


def test_packed_encoder_fp32_vs_hf_float64(dev, hf):
    box = {}
    ran = kernels_run(lambda: box.setdefault("r", _ours(hf["plm"], dev, torch.float32, hf)))
    _assert_qwen3_kernels(ran, "float")
    hs, valid, grads = box["r"]
    assert bool(torch.isfinite(hs).all())
    ref_h, ref_g = hf["ref"]
    e = float((valid - ref_h).norm() / ref_h.norm())
    print(f"  hidden: rel l2 = {e:.2e} (HF fp32 floor {hf['floors'][torch.float32]['hidden']:.2e})")
    assert e <= 1e-5
    assert set(grads) == set(ref_g)
    for n, r in ref_g.items():
        e = float((grads[n] - r).norm() / r.norm())
        print(f"  {n}: rel l2 = {e:.2e} (HF fp32 floor {hf['floors'][torch.float32][n]:.2e})")
        assert float(r.norm()) > 0 and e <= 2e-3, (n, e)


def test_packed_encoder_bf16_within_twice_the_hf_bf16_floor(dev, hf):
    box = {}
    ran = kernels_run(lambda: box.setdefault("r", _ours(hf["plm"], dev, torch.bfloat16, hf)))
    _assert_qwen3_kernels(ran, "unsigned short")
    hs, valid, grads = box["r"]
    assert bool(torch.isfinite(hs).all())
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
def test_packed_gradient_checkpointing_is_bit_identical(dev, hf, cd):
    a = _ours(hf["plm"], dev, cd, hf, checkpointing=False)
    b = _ours(hf["plm"], dev, cd, hf, checkpointing=True)
    assert torch.equal(a[0], b[0])
    for n in a[2]:
        assert torch.equal(a[2][n], b[2][n]), n


def test_graph_text_lm_takes_the_packed_qwen3_route(dev, hf, monkeypatch):
    """Cornell-size graph, one micro-batch for all active nodes: plm_embeds against HF float64 + the reference's mean pooling,
    forward + CE + backward, the route taken (kernel names and a spy on the encoder functions), and plm_packed = False."""
    import gmlm_amd
    from gmlm_amd import qwen3
    m, data, n = _graph_model(copy.deepcopy(hf["plm"]), dev, torch.float32, 24)
    assert m.plm_packed and m._has_packed_pass() and m._packed_head_dim() == 0
    g = torch.Generator().manual_seed(6)
    width = 24
    lens = torch.randint(4, width + 1, (n,), generator=g)
    am = (torch.arange(width)[None, :] < lens[:, None]).long()
    ids = torch.randint(1, 96, (n, width), generator=g) * am
    mask = data["active_mask"]
    active = int(mask.sum())
    batch = 256
    assert batch >= active
    x, ei, mk = data["x"].to(dev), data["edge_index"].to(dev), mask.to(dev)
    tokens = gmlm_amd.TokenizedTexts.from_mask(ids.to(dev), am.to(dev))

    ref = copy.deepcopy(hf["plm"]).double().eval()
    with torch.no_grad():
        hs = ref(input_ids=ids[mask], attention_mask=am[mask]).last_hidden_state
        amf = am[mask].unsqueeze(-1).double()
        pooled = (hs * amf).sum(1) / amf.sum(1).clamp(min=1e-9)

    calls = {"packed": [], "padded": 0}
    real_packed, real_padded = qwen3.qwen3_encode_packed, qwen3.qwen3_encode

    def spy_packed(plm, tok, pos, cu, max_len, *a, **k):
        calls["packed"].append((tok.numel(), cu.numel() - 1, int(max_len)))
        return real_packed(plm, tok, pos, cu, max_len, *a, **k)

    def spy_padded(*a, **k):
        calls["padded"] += 1
        return real_padded(*a, **k)

    monkeypatch.setattr(qwen3, "qwen3_encode_packed", spy_packed)
    monkeypatch.setattr(qwen3, "qwen3_encode", spy_padded)

    box = {}
    with torch.no_grad():
        ran = kernels_run(lambda: box.setdefault("p", m.encode_texts(tokens, mk, plm_batch_size=batch)))
    assert any(k.startswith("causal128::fwd_kernel<float>") for k in ran) and any(k.startswith("meanpool_fwd_kernel") for k in ran), ran
    assert not any(k.startswith(("attn_", "embed_sum_")) for k in ran), ran
    total = int(lens[mask].sum())
    assert calls["padded"] == 0 and calls["packed"] == [(total, active, int(lens[mask].max()))], calls   # ONE batch, no padded row
    got = box["p"].double().cpu()
    e = float((got[mask] - pooled).norm() / pooled.norm())
    print(f"  plm_embeds (packed): rel l2 = {e:.2e}")
    assert e <= 1e-5 and float(got[~mask].abs().max()) == 0.0

    logits = m(m.soft_mask_input(x, mk, 0.7), ei, tokens, mk, plm_batch_size=batch)
    loss = F.cross_entropy(logits[mk], data["y"].to(dev)[mk], label_smoothing=0.2)
    loss.backward()
    assert bool(torch.isfinite(loss)) and len(calls["packed"]) == 2 and calls["padded"] == 0
    seen = 0
    for k, p in m.named_parameters():
        if k.startswith("plm_encoder."):
            seen += 1
            assert p.grad is not None and bool(torch.isfinite(p.grad).all()) and float(p.grad.abs().max()) > 0, k
    assert seen == len(list(hf["plm"].parameters()))

    m.plm_packed = False
    with torch.no_grad():
        padded = m.encode_texts(tokens, mk, plm_batch_size=batch).double().cpu()
    assert calls["padded"] == 1 and len(calls["packed"]) == 2
    e = float((padded - got).norm() / got.norm())
    print(f"  padded vs packed plm_embeds: rel l2 = {e:.2e}")
    assert e <= 1e-5 and float(padded[~mask].abs().max()) == 0.0


def test_packed_route_with_the_dummy_pad_sequence(dev, hf, monkeypatch):
    """All 183 nodes active with 17..48 tokens each: more than 4,096 rows, so the batch is brought to a multiple of 16 rows
    by one dummy sequence behind the real ones.  It is encoded, never pooled, and the result agrees with the padded pass."""
    import gmlm_amd
    from gmlm_amd import qwen3
    m, data, n = _graph_model(copy.deepcopy(hf["plm"]), dev, torch.float32, 48)
    g = torch.Generator().manual_seed(8)
    width = 48
    lens = torch.randint(17, width + 1, (n,), generator=g)
    if int(lens.sum()) % 16 == 0:
        lens[0] -= 1                                              # rows must be missing from the quantum
    total = int(lens.sum())
    assert total >= 4096 and total % 16
    am = (torch.arange(width)[None, :] < lens[:, None]).long()
    ids = torch.randint(1, 96, (n, width), generator=g) * am
    mk = torch.ones(n, dtype=torch.bool, device=dev)
    tokens = gmlm_amd.TokenizedTexts.from_mask(ids.to(dev), am.to(dev))
    seen = []
    real = qwen3.qwen3_encode_packed

    def spy(plm, tok, pos, cu, max_len, *a, **k):
        seen.append((tok.numel(), cu.numel() - 1, cu.tolist()[-2:]))
        return real(plm, tok, pos, cu, max_len, *a, **k)

    monkeypatch.setattr(qwen3, "qwen3_encode_packed", spy)
    with torch.no_grad():
        packed = m.encode_texts(tokens, mk, plm_batch_size=256)
        m.plm_packed = False
        padded = m.encode_texts(tokens, mk, plm_batch_size=256)
    rows = (total + 15) // 16 * 16
    assert seen == [(rows, n + 1, [total, rows])], seen
    e = float((packed.double() - padded.double()).norm() / padded.double().norm())
    print(f"  packed (with pad sequence) vs padded plm_embeds: rel l2 = {e:.2e}")
    assert bool(torch.isfinite(packed).all()) and float(padded.abs().max()) > 0 and e <= 1e-5
