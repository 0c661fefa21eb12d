"""The EuroBERT and Llama encoder passes on the short-sequence grouped kernels (``groups`` given to ``eurobert_encode_packed`` /
``llama_encode_packed``), and a GraphTextLM on each, against the installed transformers models in float64 on the CPU (eager
attention): the method, the models (two layers, 384 wide, 6 query / 2 KV heads x 64: ``euro_gqa64`` of
tests/test_gpu_bidir_encoders.py and ``llama`` of tests/test_gpu_llama.py, the latter with projection biases and the llama3 rope) and
the bounds of those two files.  86 sequences of 1..40 tokens: 516 (sequence, head) pairs, the first count at which the short route
runs.  The bf16 bound is measured, not fixed: HF's own model in bf16 on the CPU against float64 gives each tensor's bf16 floor, and
each tensor of this path must be within 2x that floor."""
import copy

import pytest
import torch

import test_gpu_bidir_encoders as E
import test_gpu_llama as Q
from helpers import kernels_run

pytestmark = pytest.mark.gpu

N_SEQ = 86
LENS = [1 + i % 40 for i in range(N_SEQ)]
WIDTH = 40
KINDS = ("eurobert", "llama")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _make_plm(kind):
    return E._make_plm("euro_gqa64") if kind == "eurobert" else Q._make_plm("llama")


def _encode_packed(kind):
    from gmlm_amd import eurobert, llama
    return eurobert.eurobert_encode_packed if kind == "eurobert" else llama.llama_encode_packed


def gqas_pair(kind):
    c = "false" if kind == "eurobert" else "true"
    return {f"gqas::fwd_kernel<{c}, 128>", f"gqas::bwd_kernel<{c}, 128>"}


def _attention_kernels(ran):
    return {n for n in ran if n.startswith(("gqas::", "bidir::", "gqa::causal64_", "attn_", "causal128::"))}


_HF = {}


def _hf(kind):
    """The float64 reference and the bf16 floor of HF's own model, computed once per model and left unchanged."""
    if kind not in _HF:
        plm = _make_plm(kind)
        g = torch.Generator().manual_seed(3)
        lens = torch.tensor(LENS)
        am = (torch.arange(WIDTH)[None, :] < lens[:, None]).long()
        ids = torch.randint(1, 96, (N_SEQ, WIDTH), generator=g) * am
        proj = torch.randn(int(am.sum()), plm.config.hidden_size, generator=torch.Generator().manual_seed(9), dtype=torch.float64) / 16
        ref = E._hf_run(plm, torch.float64, ids, am, proj)
        hs, gr = E._hf_run(plm, torch.bfloat16, ids, am, proj)
        floor = {"hidden": float((hs - ref[0]).norm() / ref[0].norm())}
        floor.update({n: float((gr[n] - ref[1][n]).norm() / ref[1][n].norm()) for n in gr})
        _HF[kind] = dict(kind=kind, plm=plm, ids=ids, am=am, lens=lens, proj=proj, ref=ref, floor=floor)
    return _HF[kind]


def _ours(h, dev, with_groups=True, checkpointing=False):
    from gmlm_amd import ops
    m = copy.deepcopy(h["plm"]).to(dev).train()
    m.zero_grad()
    tok = h["ids"][h["am"].bool()].to(dev)
    pos = torch.cat([torch.arange(n) for n in LENS]).to(dev)
    cu = torch.tensor([0] + LENS).cumsum(0).to(dev, torch.int32)
    groups = ops.pack_sequence_groups(LENS).to(dev) if with_groups else None
    hs = _encode_packed(h["kind"])(m, tok, pos, cu, WIDTH, torch.bfloat16, True, checkpointing, None, groups=groups)
    (hs.double() * h["proj"].to(dev)).sum().backward()
    return hs.detach(), hs.detach().double().cpu(), {n: p.grad.detach().double().cpu() for n, p in m.named_parameters()}


def _within_twice_the_floor(h, valid, grads):
    ref_h, ref_g = h["ref"]
    fl, bad = h["floor"], []
    e = float((valid - ref_h).norm() / ref_h.norm())
    print(f"  hidden: rel l2 = {e:.2e}, HF bf16 floor {fl['hidden']:.2e}, ratio {e / fl['hidden']:.2f}")
    if e > 2 * fl["hidden"]:
        bad.append(("hidden", e, fl["hidden"]))
    assert set(grads) == set(ref_g)
    for n, r in ref_g.items():
        e = float((grads[n] - r).norm() / r.norm())
        print(f"  {n}: rel l2 = {e:.2e}, HF bf16 floor {fl[n]:.2e}, ratio {e / fl[n]:.2f}")
        if e > 2 * fl[n]:
            bad.append((n, e, fl[n]))
    assert not bad, bad


@pytest.mark.parametrize("kind", KINDS)
def test_packed_pass_with_groups_within_twice_the_hf_bf16_floor(dev, kind):
    """Fails on the commit before the short-sequence grouped kernels: the packed passes take no ``groups``."""
    h = _hf(kind)
    box = {}
    ran = kernels_run(lambda: box.setdefault("r", _ours(h, dev)))
    assert _attention_kernels(ran) == gqas_pair(kind), sorted(ran)
    assert {n for n in ran if n.startswith("gqa::rope_heads_kernel")} == {f"gqa::rope_heads_kernel<unsigned short, 64, {i}>" for i in ("false", "true")}
    hs, valid, grads = box["r"]
    assert hs.dtype == torch.bfloat16 and bool(torch.isfinite(hs).all())
    _within_twice_the_floor(h, valid, grads)


@pytest.mark.parametrize("kind", KINDS)
def test_without_groups_the_streaming_kernels_run(dev, kind):
    h = _hf(kind)
    ran = kernels_run(lambda: _ours(h, dev, with_groups=False))
    attn = _attention_kernels(ran)
    assert attn and all(n.startswith("bidir::" if kind == "eurobert" else "gqa::causal64_") for n in attn), sorted(ran)


@pytest.mark.parametrize("kind", KINDS)
def test_gradient_checkpointing_is_bit_identical(dev, kind):
    h = _hf(kind)
    a = _ours(h, dev, checkpointing=False)
    b = _ours(h, dev, checkpointing=True)
    assert torch.equal(a[0], b[0])
    for n in a[2]:
        assert torch.equal(a[2][n], b[2][n]), n


@pytest.mark.parametrize("kind", KINDS)
def test_graph_text_lm_builds_the_groups_itself(dev, kind):
    """GraphTextLM.encode_texts on 86 active nodes in one micro-batch (516 pairs, bf16): it launches the ``gqas::`` pair, and its
    pooled rows and the encoder's parameter gradients stay within 2x HF's bf16 floor against HF float64 + the reference's mean
    pooling, the bound of the packed pass; with a micro-batch of 85 nodes (510 pairs) it runs the streaming family."""
    import gmlm_amd
    h = _hf(kind)
    ids, am = h["ids"], h["am"]
    pp = torch.randn(N_SEQ, h["plm"].config.hidden_size, generator=torch.Generator().manual_seed(12), dtype=torch.float64) / 4

    def hf_pooled(dtype):
        m = copy.deepcopy(h["plm"]).to(dtype).train()
        m.zero_grad()
        hs = m(input_ids=ids, attention_mask=am).last_hidden_state
        hs = hs.double() if dtype == torch.float64 else hs.float()     # the pooling itself is not what the floor measures
        amf = am.unsqueeze(-1).to(hs.dtype)
        pooled = (hs * amf).sum(1) / amf.sum(1).clamp(min=1e-9)
        (pooled.double() * pp).sum().backward()
        return pooled.detach().double(), {n: p.grad.detach().double() for n, p in m.named_parameters()}

    ref_p, ref_g = hf_pooled(torch.float64)
    low_p, low_g = hf_pooled(torch.bfloat16)
    rel = lambda a, b: float((a - b).norm() / b.norm())
    floor = {"pooled": rel(low_p, ref_p), **{n: rel(low_g[n], ref_g[n]) for n in ref_g}}

    torch.manual_seed(5)
    m = gmlm_amd.GraphTextLM(12, 16, 3, dropout_rate=0.0, plm_encoder=copy.deepcopy(h["plm"]), plm_max_length=WIDTH,
                             compute_dtype=torch.bfloat16).to(dev).train()
    tokens = gmlm_amd.TokenizedTexts.from_mask(ids.to(dev), am.to(dev))
    mask = torch.ones(N_SEQ, dtype=torch.bool, device=dev)

    def run(batch):
        m.zero_grad()
        pooled = m.encode_texts(tokens, mask, plm_batch_size=batch)
        (pooled.double() * pp.to(dev)).sum().backward()
        return pooled.detach().double().cpu(), {n[len("plm_encoder."):]: p.grad.detach().double().cpu()
                                                for n, p in m.named_parameters() if n.startswith("plm_encoder.")}

    box = {}
    ran = kernels_run(lambda: box.setdefault("r", run(N_SEQ)))
    assert _attention_kernels(ran) == gqas_pair(kind), sorted(ran)
    pooled, grads = box["r"]
    bad = []
    for n, got, ref in [("pooled", pooled, ref_p)] + [(n, grads[n], ref_g[n]) for n in ref_g]:
        e = rel(got, ref)
        print(f"  {n}: rel l2 = {e:.2e}, HF bf16 floor {floor[n]:.2e}, ratio {e / floor[n]:.2f}")
        if e > 2 * floor[n]:
            bad.append((n, e, floor[n]))
    assert not bad, bad
    ran = kernels_run(lambda: run(N_SEQ - 1))                  # 85 + 1 sequences: 510 and 6 pairs
    attn = _attention_kernels(ran)
    assert attn and all(n.startswith("bidir::" if kind == "eurobert" else "gqa::causal64_") for n in attn), sorted(ran)
