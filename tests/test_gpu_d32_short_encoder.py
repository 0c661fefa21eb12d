"""A 384-wide BERT encoder (12 heads x 32) on the short-sequence head-dim-32 kernels (``d32s::``, include/gmlm_hip_d32_short.h):
the packed pass with ``groups`` against the same HuggingFace model in float64, and a GraphTextLM on it through the eager bucketed
step with and without the new route.

Encoder: the 2-layer model of tests/test_gpu_d32_encoder.py (hidden 384, 12 heads, vocab 200, recipe weights), bf16, 48 sequences
of 1..40 tokens (1, 32 and 33 among them) = 576 (sequence, head) pairs, train mode with dropout 0, loss = a fixed random weighting
of the masked mean pool.  The bar is that of ``test_encoder_bf16_within_twice_the_hf_bf16_error``: hidden states, pooled rows and
every parameter gradient within 2x the error of HF's own bf16 run against float64, the key biases left out for the reason given
there.  Both tests fail on the commit before these kernels: ``groups`` is dropped at head dim 32 and ``d32::`` kernels run."""
import copy

import pytest
import torch

from helpers import kernels_run
from test_gpu_d32_encoder import PLM, _cfg, _data, _step, hf_run, make_plm, rel

pytestmark = pytest.mark.gpu

LENS = [1, 32, 33, 40] + [1 + (11 * i) % 40 for i in range(44)]
L = max(LENS)
PAIR = {"d32s::fwd_kernel<false, 128>", "d32s::bwd_kernel<false, 128>"}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _attention_kernels(ran):
    return {n for n in ran if n.startswith(("d32s::", "d32::", "attn_", "d128::"))}


@pytest.fixture(scope="module")
def hf():
    """The float64 reference and the error of HF's own bf16 run, computed once for the module."""
    assert len(LENS) == 48 and {1, 32, 33} <= set(LENS) and max(LENS) == 40 and min(LENS) == 1
    plm = make_plm()
    g = torch.Generator().manual_seed(3)
    lens = torch.tensor(LENS)
    am = (torch.arange(L)[None, :] < lens[:, None]).long()
    ids = torch.randint(1, PLM["vocab"], (len(LENS), L), generator=g) * am
    gp = torch.randn(len(LENS), PLM["hidden"], generator=g, dtype=torch.float64)
    ref = hf_run(plm, torch.float64, ids, am, gp)
    low = hf_run(plm, torch.bfloat16, ids, am, gp)
    floor = {"hidden": rel(low[0], ref[0]), "pooled": rel(low[1], ref[1])}
    floor.update({n: rel(low[2][n], ref[2][n]) for n in ref[2] if float(ref[2][n].norm()) > 0})
    return dict(plm=plm, ids=ids, am=am, lens=lens, gp=gp, ref=ref, floor=floor)


def _ours(hf, dev):
    from gmlm_amd import bert, ops
    m = copy.deepcopy(hf["plm"]).to(dev).train()
    m.zero_grad()
    ids, lens = hf["ids"].to(dev), hf["lens"].to(dev, torch.int32)
    b = len(LENS)
    cu = torch.zeros(b + 1, dtype=torch.int32, device=dev)
    cu[1:] = torch.cumsum(lens, 0)
    keep = hf["am"].bool().to(dev)
    tok = ids[keep]
    pos = torch.arange(L, device=dev)[None, :].expand(b, L)[keep]
    groups = ops.pack_sequence_groups(LENS).to(dev)
    hs = bert.bert_encode_packed(m, tok, pos, cu, L, torch.bfloat16, training=True, groups=groups)
    pooled = ops.MeanPoolScatter.apply(torch.zeros(b, PLM["hidden"], device=dev), hs, None, torch.arange(b, device=dev), cu, int(sum(LENS)))
    (pooled.double() * hf["gp"].to(dev)).sum().backward()
    grads = {n: p.grad.detach().double().cpu() for n, p in m.named_parameters() if p.grad is not None}
    return hs.detach().double().cpu(), pooled.detach().double().cpu(), grads


def test_packed_pass_with_groups_within_twice_the_hf_bf16_error(dev, hf):
    box = {}
    ran = kernels_run(lambda: box.setdefault("r", _ours(hf, dev)))
    assert _attention_kernels(ran) == PAIR, sorted(ran)        # forward and backward of the new pair, no d32:: attention kernel
    valid, pooled, grads = box["r"]
    ref_h, ref_p, ref_g = hf["ref"]
    fl = hf["floor"]
    assert set(grads) == set(ref_g)
    qkv_bias = [n for n in grads if n.endswith(("query.bias", "key.bias", "value.bias"))]
    assert len(qkv_bias) == 3 * PLM["layers"] and all(bool(torch.isfinite(grads[n]).all()) for n in qkv_bias)
    assert all(float(grads[n].norm()) > 0 for n in qkv_bias if not n.endswith("key.bias"))
    got = {"hidden": rel(valid, ref_h), "pooled": rel(pooled, ref_p)}
    got.update({n: rel(grads[n], ref_g[n]) for n in ref_g if n in fl and not n.endswith("key.bias")})
    bad = []
    for n, e in got.items():
        print(f"  {n}: rel l2 = {e:.2e}, HF bf16 {fl[n]:.2e}, ratio {e / fl[n]:.2f}")
        if not e <= 2 * fl[n]:
            bad.append((n, e, fl[n]))
    assert not bad, bad


def test_graphtextlm_eager_bucketed_step_takes_the_new_route(dev, monkeypatch):
    """One eager step with ``plm_bucketed`` at the geometry of tests/test_gpu_d32_encoder.py, bf16: the ``d32s::`` pair runs and no
    ``d32::`` attention kernel; with the dispatch rule forced to false the streaming ``d32::`` kernels run; the logits of the two
    agree within the bf16 bar tests/test_gpu_model.py uses between two routes (2e-2 of the largest value)."""
    from gmlm_amd import ops
    from test_gpu_model import build_model
    cfg = _cfg()
    x, ei, y, tokens, masks = _data(cfg, dev)
    m = build_model(cfg, dev, compute_dtype=torch.bfloat16).train()
    m.plm_bucketed = True
    box = {}
    # (the step's cross-attention between graph and text embeddings runs attn_ kernels at its own head dim: not the encoder's)
    d32_any = lambda ran: {n for n in ran if n.startswith(("d32s::", "d32::"))}
    ran = kernels_run(lambda: box.setdefault("new", _step(m, x, ei, y, tokens, masks[0], 512)))
    attn = d32_any(ran)
    assert attn and all(n.startswith("d32s::") for n in attn) and any("fwd" in n for n in attn) and any("bwd" in n for n in attn), sorted(ran)
    monkeypatch.setattr(ops, "_d32_short_path", lambda *a: False)
    m._active_seen = None                                      # the bucket tables are cached per mask: build them again
    ran = kernels_run(lambda: box.setdefault("old", _step(m, x, ei, y, tokens, masks[0], 512)))
    attn = d32_any(ran)
    assert attn and all(n.startswith("d32::") for n in attn), sorted(ran)
    l_new, l_old = box["new"][0].float(), box["old"][0].float()
    d = float((l_new - l_old).abs().max())
    print(f"  logits: max |d32s route - d32 route| = {d:.3e} of max |logit| {float(l_old.abs().max()):.3e}")
    assert bool(torch.isfinite(l_new).all()) and d <= 2e-2 * float(l_old.abs().max())
