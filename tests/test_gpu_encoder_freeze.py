"""Text encoders and GraphTextLM with parameters frozen by name, on the device.

Freezing a parameter changes neither the hidden states nor the gradient of any other parameter, so the all-trainable float64
HF run of each family's own test module (its two-layer model, tokens and projection) is the reference of every recipe:

  (a) every bias frozen                       (b) the embeddings and layer 0 frozen
  (c) only the norm parameters trainable       (d) only the last layer's attention output projection trainable

Per (family, recipe, layout): the hidden states equal, bit for bit, those of the all-trainable run; every trainable
parameter's gradient is within the family module's budget of the HF float64 gradient (fp32: 2e-3 of its norm; bf16: 2x the
error of HF's own bf16 run); every frozen parameter has no gradient.  A gradient that is zero in exact arithmetic (a key bias
under softmax) has no relative error: fp32 holds it to 2e-3 of the query bias's gradient, as test_gpu_mpnet.py does, bf16
leaves it out, as the family modules do.  Every recipe runs in fp32, (b) also in bf16 (layer 0 runs without ``out_lo``, layer 1
with it) and, in every module that calls ``encoder.run_layers`` (EuroBERT runs llama.py's), with gradient checkpointing.

GraphTextLM: the pre-training freeze of the reference driver by name (PLM, fusion_network, classifier, gnn_proj frozen) and
its inverse (GNN layers and the mask token frozen) through forward + loss + backward against the CPU oracle with the same
flags, under test_gpu_model._oracle_vs_hip's fp32 tolerances, then one optimizer step of ``harness.setup_optimizer`` with
torch.optim.AdamW and with FusedAdamW: a frozen parameter keeps its bits."""
import copy
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import gmlm_oracle as O
import test_gpu_bidir_encoders as TB
import test_gpu_deberta as TD
import test_gpu_llama as TL
import test_gpu_modernbert as TM
import test_gpu_mpnet as TP
import test_gpu_qwen3 as TQ
from helpers import oracle_model_from_config
from test_gpu_model import build_model, hf_bert

pytestmark = pytest.mark.gpu

BF, FP = torch.bfloat16, torch.float32


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


# ---------------------------------------------------------------------------------------------------------------- the families
def _pack(plm, ids, lens, proj, run):
    """-> the family record: ``run(plm, dtype)`` is the module's HF run -> (valid hidden states, {name: grad}) in float64"""
    ref = run(plm, torch.float64)
    hs, gr = run(plm, BF)
    floor = {n: float((gr[n] - ref[1][n]).norm() / ref[1][n].norm()) for n in gr if float(ref[1][n].norm()) > 0}
    return dict(plm=plm, ids=ids, lens=lens, proj=proj, ref=ref, floor=floor)


def _bert():
    """The HF float64 run the other families' modules have, for BERT (test_gpu_model.hf_bert's configuration, two layers)"""
    from transformers import BertModel
    from gmlm_amd import bert
    torch.manual_seed(0)
    plm = BertModel(hf_bert(dict(vocab=96, hidden=128, layers=2, heads=2, inter=192, max_pos=512)).config, add_pooling_layer=False)
    g = torch.Generator().manual_seed(1)
    with torch.no_grad():
        for n, p in plm.named_parameters():
            if "LayerNorm.weight" in n:
                p.copy_(torch.empty_like(p).uniform_(0.5, 1.5, generator=g))
            elif "embeddings" in n or p.dim() == 1:
                p.copy_(torch.randn(p.shape, generator=g) * (1.0 if p.dim() == 2 else 0.1))
            else:
                p.copy_(torch.randn(p.shape, generator=g) * p.shape[1] ** -0.5)
    plm = plm.train()
    ids, am, lens = TL._tokens()
    proj = torch.randn(int(am.sum()), 128, generator=torch.Generator().manual_seed(9), dtype=torch.float64) / 16
    rec = _pack(plm, ids, lens, proj, lambda m, dt: TL._hf_run(m, dt, ids, am, proj))
    return dict(rec, encode=bert.bert_encode, packed=bert.bert_encode_packed)


def _mpnet():
    from gmlm_amd import mpnet
    plm = TP._make_plm(num_hidden_layers=2)
    ids, am, lens = TP._tokens()
    proj = torch.randn(int(am.sum()), TP.P, generator=torch.Generator().manual_seed(9), dtype=torch.float64) / 16
    return dict(_pack(plm, ids, lens, proj, lambda m, dt: TP._hf_run(m, dt, ids, lens, proj)), encode=mpnet.mpnet_encode,
                packed=mpnet.mpnet_encode_packed)


def _deberta():
    from gmlm_amd import deberta
    plm = TD._make_plm()
    ids, lens = TD._tokens(TD.BATCHES["short"])
    proj = torch.randn(int(lens.sum()), TD.P, generator=torch.Generator().manual_seed(9), dtype=torch.float64) / 16
    return dict(_pack(plm, ids, lens, proj, lambda m, dt: TD._hf_run(m, dt, ids, lens, proj)), encode=deberta.deberta_encode,
                packed=deberta.deberta_encode_packed)


def _modernbert():
    from gmlm_amd import modernbert
    h = TM._reference(32)                                   # four layers: the smallest with both layer types
    return dict(plm=h["plm"], ids=h["ids"], lens=h["lens"], proj=h["proj"], ref=h["ref"], floor=h["floors"][BF],
                encode=modernbert.modernbert_encode, packed=modernbert.modernbert_encode_packed)


def _qwen3():
    from gmlm_amd import qwen3
    plm = TQ._make_plm()
    ids, am, lens = TQ._tokens()
    proj = torch.randn(int(am.sum()), 256, generator=torch.Generator().manual_seed(9), dtype=torch.float64) / 16
    return dict(_pack(plm, ids, lens, proj, lambda m, dt: TQ._hf_run(m, dt, ids, am, proj)), encode=qwen3.qwen3_encode,
                packed=qwen3.qwen3_encode_packed)


def _llama():
    from gmlm_amd import llama
    h = TL._hf("llama")                                     # the kind with projection biases
    return dict(plm=h["plm"], ids=h["ids"], lens=h["lens"], proj=h["proj"], ref=h["ref"], floor=h["floor"],
                encode=llama.llama_encode, packed=llama.llama_encode_packed)


def _bidir(kind):
    def make():
        h = TB._hf(kind)
        _, encode, packed = TB._passes(kind)
        return dict(plm=h["plm"], ids=h["ids"], lens=h["lens"], proj=h["proj"], ref=h["ref"], floor=h["floor"], encode=encode, packed=packed)
    return make


FAMILIES = {"bert": _bert, "mpnet": _mpnet, "deberta": _deberta, "modernbert": _modernbert, "qwen3": _qwen3, "llama": _llama,
            "eurobert": _bidir("euro_gqa128"), "nomic_bert": _bidir("nomic")}     # euro_gqa128: the EuroBERT kind with projection biases
HAS_BIAS = ("bert", "mpnet", "deberta", "llama", "eurobert", "nomic_bert")      # recipe (a) freezes something there
_FAM = {}


def family(name):
    if name not in _FAM:
        _FAM[name] = FAMILIES[name]()
    return _FAM[name]


# ----------------------------------------------------------------------------------------------------------------- the recipes
_LAYER = re.compile(r"(?:^|\.)layers?\.(\d+)\.")
_OUT_PROJ = ("attention.output.dense.", "attention.attn.o.", "attn.Wo.", "self_attn.o_proj.")


def trainable(recipe, names):
    """-> the set of names that keep requires_grad"""
    layer = {n: int(_LAYER.search(n).group(1)) for n in names if _LAYER.search(n)}
    last = max(layer.values())
    if recipe == "all":
        keep = set(names)
    elif recipe == "a":
        keep = {n for n in names if not n.endswith("bias")}
    elif recipe == "b":
        keep = {n for n in names if layer.get(n, -1) >= 1 or (n not in layer and "embed" not in n.lower())}
    elif recipe == "c":
        keep = {n for n in names if "norm" in n.lower() or re.search(r"(^|[._])ln([._]|$)", n.lower())}      # ... or an emb_ln / ln_f
    else:
        keep = {n for n in names if layer.get(n) == last and any(s in n for s in _OUT_PROJ)}
    assert keep and (recipe == "all" or keep != set(names)), (recipe, sorted(keep))
    return keep


def test_recipes_by_name():
    names = ["embeddings.word_embeddings.weight", "embeddings.LayerNorm.weight", "embeddings.LayerNorm.bias",
             "encoder.layer.0.attention.self.query.bias", "encoder.layer.0.attention.output.dense.weight",
             "encoder.layer.1.attention.self.query.bias", "encoder.layer.1.attention.output.dense.weight",
             "encoder.layer.1.output.LayerNorm.weight", "encoder.rel_embeddings.weight", "final_norm.weight"]
    assert trainable("a", names) == {n for n in names if n.endswith("weight")}
    assert trainable("b", names) == {n for n in names if "layer.1." in n} | {"final_norm.weight"}
    assert trainable("c", names) == {"embeddings.LayerNorm.weight", "embeddings.LayerNorm.bias", "encoder.layer.1.output.LayerNorm.weight",
                                     "final_norm.weight"}
    assert trainable("d", names) == {"encoder.layer.1.attention.output.dense.weight"}


_ZERO_PARTNER = ((".key.", ".query."), (".key_proj.", ".query_proj."), ("attn.k.", "attn.q."), ("k_proj", "q_proj"))


def _run(fam, keep, dev, cd, packed, ckpt=False):
    """-> (valid hidden states, {name: grad or None})"""
    m = copy.deepcopy(fam["plm"])
    for n, p in m.named_parameters():
        p.requires_grad_(n in keep)
    m = m.to(dev).train()
    m.zero_grad()
    ids, lens = fam["ids"], fam["lens"]
    lens_d = lens.to(dev, torch.int32)
    am = torch.arange(ids.shape[1])[None, :] < lens[:, None]
    if packed:
        tok = ids[am].to(dev)
        pos = torch.cat([torch.arange(n) for n in lens.tolist()]).to(dev)
        cu = torch.tensor([0] + lens.cumsum(0).tolist(), dtype=torch.int32, device=dev)
        valid = fam["packed"](m, tok, pos, cu, int(lens.max()), cd, True, ckpt)
    else:
        valid = fam["encode"](m, ids.to(dev), lens_d, cd, True, ckpt)[am.to(dev)]
    (valid.double() * fam["proj"].to(dev)).sum().backward()
    return valid.detach(), {n: p.grad for n, p in m.named_parameters()}


_BASE = {}


def _base(name, dev, cd, packed):
    """The all-trainable run of (family, dtype, layout), once"""
    key = (name, cd, packed)
    if key not in _BASE:
        fam = family(name)
        _BASE[key] = _run(fam, trainable("all", [n for n, _ in fam["plm"].named_parameters()]), dev, cd, packed)
    return _BASE[key]


def _check(name, recipe, dev, cd, packed, ckpt=False):
    fam = family(name)
    names = [n for n, _ in fam["plm"].named_parameters()]
    keep = trainable(recipe, names)
    base_hs, base_g = _base(name, dev, cd, packed)
    hs, grads = _run(fam, keep, dev, cd, packed, ckpt)
    assert torch.equal(hs, base_hs), "freezing parameters changed the hidden states"
    ref_g = fam["ref"][1]
    bad = []
    for n in names:
        if n not in keep:
            assert grads[n] is None, f"frozen {n} got a gradient"
            continue
        g, r = grads[n], ref_g[n]
        assert g is not None and g.shape == r.shape and bool(torch.isfinite(g).all()), n
        g = g.detach().double().cpu()
        partner = next((n.replace(a, b) for a, b in _ZERO_PARTNER if a in n and n.endswith("bias")), None)
        if partner is not None and float(r.norm()) <= 1e-9 * float(ref_g[partner].norm()):
            if cd == FP:                                     # zero in exact arithmetic (module docstring)
                assert float(g.norm()) <= 2e-3 * float(ref_g[partner].norm()), n
            continue
        e = float((g - r).norm() / r.norm())
        lim = 2e-3 if cd == FP else 2 * fam["floor"][n]
        print(f"  {n}: rel l2 = {e:.2e} (limit {lim:.2e})")
        if e > lim:
            bad.append((n, e, lim))
    assert not bad, bad


LAYOUTS = [False, True]
FP32 = [(f, r, p) for f in FAMILIES for r in "abcd" if r != "a" or f in HAS_BIAS for p in LAYOUTS]


@pytest.mark.parametrize("name,recipe,packed", FP32, ids=[f"{f}-{r}-{'packed' if p else 'padded'}" for f, r, p in FP32])
def test_encoder_fp32_frozen_by_name(dev, name, recipe, packed):
    _check(name, recipe, dev, FP, packed)


BF16 = [(f, p) for f in FAMILIES for p in LAYOUTS]


@pytest.mark.parametrize("name,packed", BF16, ids=[f"{f}-{'packed' if p else 'padded'}" for f, p in BF16])
def test_encoder_bf16_with_embeddings_and_layer_0_frozen(dev, name, packed):
    _check(name, "b", dev, BF, packed)


@pytest.mark.parametrize("packed", LAYOUTS, ids=["padded", "packed"])
@pytest.mark.parametrize("cd", [FP, BF], ids=["fp32", "bf16"])
@pytest.mark.parametrize("name", ["bert", "mpnet", "deberta", "modernbert", "qwen3", "llama", "nomic_bert"])      # every run_layers user
def test_encoder_checkpointed_with_embeddings_and_layer_0_frozen(dev, name, cd, packed):
    _check(name, "b", dev, cd, packed, ckpt=True)


# ----------------------------------------------------------------------------------------------------------------- GraphTextLM
def _pretrain_frozen(name):
    return name.startswith(("plm_encoder.", "fusion_network", "classifier", "gnn_proj"))


def _gnn_frozen(name):
    from gmlm_amd.harness import GNN_PARAM_NAMES
    return any(g in name for g in (*GNN_PARAM_NAMES, "gnn_mask_token_embed"))


def _oracle_name(k):
    return "plm_params." + k[len("plm_encoder."):].replace(".", "/") if k.startswith("plm_encoder.") else k


@pytest.mark.parametrize("frozen", [_pretrain_frozen, _gnn_frozen], ids=["pretraining", "inverse"])
def test_graph_text_lm_frozen_by_name_vs_oracle(dev, frozen):
    """test_gpu_model._oracle_vs_hip on the toy workload with the same requires_grad flags on both sides; fp32: logits to 1e-4,
    gradient norms to 2e-3 (floor 1e-4)."""
    import gmlm_amd
    from gmlm_amd import harness
    plm = dict(hidden=64, layers=2, heads=2, inter=128, max_pos=64, vocab=200)
    n, e, f_in, c = O.WORKLOADS["toy"]
    cfg = dict(n=n, e=e, f_in=f_in, hc=16, c=c, plm=plm, seed=500 + n % 97, max_len=24)
    data = O.synthetic_graph("toy")
    ids, am = O.synthetic_tokens(n, 24, plm["vocab"], seed=n, min_len=4)
    om, _ = oracle_model_from_config(cfg)
    m = build_model(cfg, dev, compute_dtype=FP).train()
    names = [k for k, _ in m.named_parameters()]
    og_params = dict(om.named_parameters())
    assert any(frozen(k) for k in names) and not all(frozen(k) for k in names)
    for k, p in m.named_parameters():
        p.requires_grad_(not frozen(k))
        if _oracle_name(k) in og_params:
            og_params[_oracle_name(k)].requires_grad_(not frozen(k))
    mask = data["active_mask"]
    ref = om(O.soft_masking_gnn_input(data["x"], mask, om.gnn_mask_token_embed, 0.7), data["edge_index"], ids, am, mask, plm_batch_size=32)
    F.cross_entropy(ref[mask], data["y"][mask], label_smoothing=0.2).backward()
    x, ei, mk = data["x"].to(dev), data["edge_index"].to(dev), mask.to(dev)
    tokens = gmlm_amd.TokenizedTexts.from_mask(ids.to(dev), am.to(dev))
    logits = m(m.soft_mask_input(x, mk, 0.7), ei, tokens, mk, plm_batch_size=32)
    F.cross_entropy(logits[mk], data["y"].to(dev)[mk], label_smoothing=0.2).backward()
    np.testing.assert_allclose(logits.detach().cpu().numpy(), ref.detach().numpy(), rtol=0, atol=1e-4)
    checked = 0
    for k, p in m.named_parameters():
        r = og_params.get(_oracle_name(k))
        if frozen(k):
            assert p.grad is None, f"frozen {k} got a gradient"
            continue
        if r is None or r.grad is None or p.grad is None:
            assert (r is None or r.grad is None or float(r.grad.abs().max()) == 0) and (p.grad is None or float(p.grad.abs().max()) == 0), k
            continue
        rn, gn = float(r.grad.double().norm()), float(p.grad.double().norm())
        assert abs(rn - gn) <= 2e-3 * max(rn, 1e-4) + 1e-6, (k, gn, rn)
        checked += 1
    assert checked > 4
    # one optimizer step: a frozen parameter keeps its bits, a trainable one with a gradient moves
    before = {k: p.detach().clone() for k, p in m.named_parameters()}
    grads = {k: None if p.grad is None else p.grad.clone() for k, p in m.named_parameters()}
    for fused in (False, True):
        with torch.no_grad():
            for k, p in m.named_parameters():
                p.copy_(before[k])
                p.grad = None if grads[k] is None else grads[k].clone()
        opt = harness.setup_optimizer(m, 1e-3, 1e-4, 1e-3, 0.01, fused=fused)
        opt.step()
        torch.cuda.synchronize()
        moved = 0
        for k, p in m.named_parameters():
            if frozen(k):
                assert torch.equal(p.detach(), before[k]), f"{'FusedAdamW' if fused else 'AdamW'} changed frozen {k}"
            elif grads[k] is not None and float(grads[k].abs().max()) > 0:
                moved += int(not torch.equal(p.detach(), before[k]))
        assert moved > 4
