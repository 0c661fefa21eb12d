"""gemm_precision="bf16x3" at model level, held to the fp32 bars of tests/test_gpu_model.py and tests/test_gpu_qwen3.py.

Every case of those files that compares the fp32 path against the oracle, a golden file or HF float64 is restated here and run
twice, once native fp32 and once bf16x3 (fp32 storage, the dense layers on the three-product bf16 GEMM), each with dropout 0
and each against the SAME bars and the SAME reference values; the native run is asserted alongside, so a broken reference
shows as a native failure.  Every check prints its measured maximum as a fraction of its bar.

One bar is missed, at BERT-base depth only (12 layers, golden g4_bert_base): the mean-pooled rows, atol 5e-5 + rtol 1e-4.
Measured on MI355X: bf16x3 7.03e-5 = 1.01 of the bar in the padded pass and 6.83e-5 = 1.18 of it in the packed pass, where the
native fp32 run is at 1.22e-5 = 0.16 and 7.87e-6 = 0.11 of the bar (DESIGN.md section 4 "bf16x3").  The hidden states of the
same runs hold their (wider) bar at 0.53 / 0.61 of it, and so does every gradient.  That assertion has a test of its own,
test_bert_base_depth_pooled_bar, which is marked xfail(strict=True) for bf16x3; the bar is not widened."""
import copy

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import gmlm_oracle as O
from helpers import bert_state_template, kernels_run, load_golden, oracle_model_from_config, t
from param_recipe import recipe_state_dict
from test_gpu_model import build_model, hf_bert
from test_gpu_qwen3 import L, LENS, hf  # noqa: F401  (hf: the module-scoped fixture)
from test_gpu_qwen3_packed import _packed_inputs

pytestmark = pytest.mark.gpu

MODES = ["native", "bf16x3"]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


class Bars:
    """Collects `measured / allowed` of every check of one run; the run passes when none exceeds 1."""

    def __init__(self, tag):
        self.tag, self.rows = tag, []

    def close(self, name, got, ref, rtol, atol):
        """numpy.testing.assert_allclose's criterion |got - ref| <= atol + rtol |ref|, as a ratio."""
        got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
        assert got.shape == ref.shape and np.isfinite(got).all(), name
        self.rows.append((name, float((np.abs(got - ref) / (atol + rtol * np.abs(ref))).max()), float(np.abs(got - ref).max())))

    def scalar(self, name, err, allowed):
        self.rows.append((name, float(err) / allowed, float(err)))

    def finish(self, only=None, apart=()):
        """Assert every row (``only``: just the rows of these names; ``apart``: every row but these, which have a test of their own)."""
        rows = [r for r in self.rows if (only is None or r[0] in only) and r[0] not in apart]
        worst = sorted(rows, key=lambda r: -r[1])[:4]
        print(f"\n  [{self.tag}] " + "; ".join(f"{n}: {e:.2e} = {r:.3f} of its bar" for n, r, e in worst))
        bad = [(n, r, e) for n, r, e in rows if not r <= 1.0]
        assert rows and not bad, (self.tag, bad)


def split_kernels_ran(ran, expected):
    assert any(k.startswith("split3::split_rows_kernel") for k in ran) is expected, sorted(ran)


# ------------------------------------------------------------------------------------------------- BERT blocks vs HF goldens
def _golden_bert(name, dev):
    g = load_golden(name)
    c = g["config"]
    plm = hf_bert(dict(vocab=c["vocab"], hidden=c["hidden"], layers=c["layers"], heads=c["heads"], inter=c["inter"], max_pos=c["max_pos"]))
    plm.load_state_dict(recipe_state_dict(bert_state_template(c["hidden"], c["layers"], c["inter"], c["vocab"], c["max_pos"]), c["seed"]))
    return g, c, plm.to(dev).train()


_RUNS = {}                 # (layout, golden, mode) -> Bars: every run is made once and shared by the tests that read it


def apart(name, mode):
    """The one bar with a test of its own (test_bert_base_depth_pooled_bar)."""
    return ("pooled",) if (name, mode) == ("g4_bert_base", "bf16x3") else ()


def _padded_run(dev, name, mode):
    """test_gpu_model.test_bert_block_vs_hf_golden (padded pass), its bars unchanged; g4_bert_base is BERT-base depth."""
    if ("padded", name, mode) in _RUNS:
        return _RUNS["padded", name, mode]
    from gmlm_amd import bert, ops
    g, c, plm = _golden_bert(name, dev)
    ids, am = t(g["input_ids"]).to(dev), t(g["attention_mask"]).to(dev)
    lens = am.sum(-1).to(torch.int32)
    box = {}

    def run():
        weights = bert.prepare_weights(plm, torch.float32, mode)
        hs = bert.bert_encode(plm, ids, lens, torch.float32, training=True, weights=weights)
        b, p = ids.shape[0], c["hidden"]
        pooled = ops.MeanPoolScatter.apply(torch.zeros(b, p, device=dev), hs, lens, torch.arange(b, device=dev))
        (pooled * t(g["grad_pooled"]).to(dev)).sum().backward()
        box.update(hs=hs.detach(), pooled=pooled.detach())

    split_kernels_ran(kernels_run(run), mode == "bf16x3")
    bars = Bars(f"{name} padded {mode}")
    valid = am.bool().cpu()
    bars.close("last_hidden_state", box["hs"].cpu()[valid].numpy(), t(g["last_hidden_state"])[valid].numpy(), 1e-4, 1e-4)
    bars.close("pooled", box["pooled"].cpu().numpy(), g["pooled"], 1e-4, 5e-5)
    grads = {k: v.grad for k, v in plm.named_parameters()}
    for k, ref in g["grad_norms"].items():
        bars.scalar("|grad| " + k, abs(float(grads[k].double().norm()) - ref), 2e-3 * max(ref, 1e-3) + 1e-6)
    for k in ("embeddings.LayerNorm.weight", "encoder.layer.0.attention.self.query.bias"):
        bars.close("grad " + k, grads[k].cpu().numpy(), g["grad:" + k], 5e-3, 1e-4 * g["grad_norms"][k])
    _RUNS["padded", name, mode] = bars
    return bars


def _packed_run(dev, mode):
    """test_gpu_model.test_packed_bert_matches_hf_golden (variable-length pass, BERT-base geometry), its bars unchanged."""
    if ("packed", "g4_bert_base", mode) in _RUNS:
        return _RUNS["packed", "g4_bert_base", mode]
    from gmlm_amd import bert, ops
    g, c, plm = _golden_bert("g4_bert_base", dev)
    ids, am = t(g["input_ids"]).to(dev), t(g["attention_mask"]).to(dev).bool()
    lens = am.sum(-1)
    b, l = ids.shape
    cu = torch.zeros(b + 1, dtype=torch.int32, device=dev)
    cu[1:] = torch.cumsum(lens, 0)
    pos = torch.arange(l, device=dev)[None].expand(b, l)[am]
    weights = bert.prepare_weights(plm, torch.float32, mode)
    hs = bert.bert_encode_packed(plm, ids[am], pos, cu, int(lens.max()), torch.float32, training=True, weights=weights)
    bars = Bars(f"g4_bert_base packed {mode}")
    bars.close("last_hidden_state", hs.detach().cpu().numpy(), t(g["last_hidden_state"])[am.cpu()].numpy(), 1e-4, 1e-4)
    pooled = ops.MeanPoolScatter.apply(torch.zeros(b, c["hidden"], device=dev), hs, None, torch.arange(b, device=dev), cu)
    bars.close("pooled", pooled.detach().cpu().numpy(), g["pooled"], 1e-4, 5e-5)
    (pooled * t(g["grad_pooled"]).to(dev)).sum().backward()
    grads = {k: v.grad for k, v in plm.named_parameters()}
    for k, ref in g["grad_norms"].items():
        bars.scalar("|grad| " + k, abs(float(grads[k].double().norm()) - ref), 2e-3 * max(ref, 1e-3) + 1e-6)
    _RUNS["packed", "g4_bert_base", mode] = bars
    return bars


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", ["g4_bert_tiny", "g4_bert_base"])
def test_bert_block_vs_hf_golden(dev, name, mode):
    _padded_run(dev, name, mode).finish(apart=apart(name, mode))


@pytest.mark.parametrize("mode", MODES)
def test_packed_bert_matches_hf_golden(dev, mode):
    _packed_run(dev, mode).finish(apart=apart("g4_bert_base", mode))


POOLED_MISS = ("bf16x3 misses the pooled-rows bar (atol 5e-5 + rtol 1e-4) at BERT-base depth: measured 7.03e-5 = 1.01 of the bar "
               "(padded) and 6.83e-5 = 1.18 of it (packed) on MI355X, native fp32 1.22e-5 = 0.16 and 7.87e-6 = 0.11 of it; the bar is not widened "
               "(DESIGN.md section 4 'bf16x3')")


@pytest.mark.parametrize("mode", ["native", pytest.param("bf16x3", marks=pytest.mark.xfail(strict=True, reason=POOLED_MISS))])
def test_bert_base_depth_pooled_bar(dev, mode):
    """The mean-pooled rows of the 12-layer golden, padded and packed pass, against test_gpu_model's bar for them."""
    a, b = _padded_run(dev, "g4_bert_base", mode), _packed_run(dev, mode)
    rows = [r for r in a.rows + b.rows if r[0] == "pooled"]
    print(f"\n  [g4_bert_base pooled {mode}] padded {rows[0][2]:.2e} = {rows[0][1]:.3f} of its bar; packed {rows[1][2]:.2e} = {rows[1][1]:.3f} of its bar")
    assert len(rows) == 2 and all(r[1] <= 1.0 for r in rows), rows


# ----------------------------------------------------------------------------------------------- full model vs the goldens
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", ["g1_toy", "g2_cornell"])
def test_golden_forward_backward(dev, name, mode):
    """test_gpu_model.test_golden_forward_backward: the reference's own outputs, bars unchanged (logits 1e-4 absolute)."""
    import gmlm_amd
    g = load_golden(name)
    cfg = g["config"]
    m = build_model(cfg, dev, gemm_precision=mode).train()
    x, ei, mask = t(g["x"]).to(dev), t(g["edge_index"]).to(dev), t(g["node_mask"]).to(dev)
    tokens = gmlm_amd.TokenizedTexts.from_mask(t(g["input_ids"]).to(dev), t(g["attention_mask"]).to(dev))
    bars = Bars(f"{name} {mode}")
    xm = gmlm_amd.soft_masking_gnn_input(x, mask, m.gnn_mask_token_embed, cfg["beta"])
    bars.close("x_soft_masked", xm.detach().cpu().numpy(), g["x_soft_masked"], 0, 1e-6)
    bars.close("gnn_embeds", m.get_graph_embeddings(xm, ei).detach().cpu().numpy(), g["gnn_embeds"], 1e-4, 1e-4)
    bars.close("plm_embeds", m.encode_texts(tokens, mask, cfg["plm_batch_size"]).detach().cpu().numpy(), g["plm_embeds"], 1e-4, 1e-4)
    logits = m(xm, ei, tokens, mask, plm_batch_size=cfg["plm_batch_size"])
    assert logits.dtype == torch.float32
    bars.close("logits", logits.detach().cpu().numpy(), g["logits"], 0, 1e-4)
    loss = F.cross_entropy(logits[mask], t(g["y"]).to(dev)[mask], label_smoothing=0.2)
    bars.scalar("loss", abs(loss.item() - float(g["loss"])), 1e-4)
    loss.backward()
    grads = {k: p.grad for k, p in m.named_parameters()}
    for k, ref in g["grad_norms"].items():
        gr = grads[k]
        if ref < 0:
            assert gr is None or float(gr.abs().max()) == 0.0, k
            continue
        assert gr is not None, k
        bars.scalar("|grad| " + k, abs(float(gr.double().norm()) - ref), 1e-3 * max(ref, 1e-3) + 1e-6)
        if "grad:" + k in g:
            bars.close("grad " + k, gr.cpu().numpy(), g["grad:" + k], 5e-3, 2e-5 * max(1.0, ref))
    with torch.no_grad():
        bars.close("gge_only", m.get_graph_embeddings(x, ei).cpu().numpy(), g["gge_only"], 1e-4, 1e-4)
    bars.finish()


# ------------------------------------------------------------------------------------------ full model vs the CPU oracle
PLM_MINI = dict(hidden=256, layers=4, heads=4, inter=1024, max_pos=64, vocab=200)


@pytest.fixture(scope="module")
def chameleon():
    """The oracle's forward + backward at BASELINE configs[1] geometry, computed once for both modes."""
    name, hc, max_len, bs = "chameleon", 256, 24, 32
    n, e, f_in, c = O.WORKLOADS[name]
    cfg = dict(n=n, e=e, f_in=f_in, hc=hc, c=c, plm=PLM_MINI, seed=500 + n % 97, max_len=max_len)
    data = O.synthetic_graph(name)
    ids, am = O.synthetic_tokens(n, max_len, PLM_MINI["vocab"], seed=n, min_len=4)
    om, _ = oracle_model_from_config(cfg)
    mask = data["active_mask"]
    ref = om(O.soft_masking_gnn_input(data["x"], mask, om.gnn_mask_token_embed, 0.7), data["edge_index"], ids, am, mask, plm_batch_size=bs)
    loss_ref = F.cross_entropy(ref[mask], data["y"][mask], label_smoothing=0.2)
    loss_ref.backward()
    return dict(cfg=cfg, data=data, ids=ids, am=am, bs=bs, ref=ref.detach(), loss=float(loss_ref),
                grads={k: p.grad for k, p in om.named_parameters()})


@pytest.mark.parametrize("mode", MODES)
def test_chameleon_size_fp32_vs_oracle(dev, chameleon, mode):
    """test_gpu_model.test_chameleon_size_fp32_vs_oracle: N = 2,277, E = 36,101, hc = 256, BERT-mini; logits within 1e-4 of the
    oracle, the loss within 1e-4, every gradient norm within 2e-3 (floor 1e-4)."""
    import gmlm_amd
    ch = chameleon
    data, mask = ch["data"], ch["data"]["active_mask"]
    m = build_model(ch["cfg"], dev, compute_dtype=torch.float32, gemm_precision=mode).train()
    x, ei, mk = data["x"].to(dev), data["edge_index"].to(dev), mask.to(dev)
    tokens = gmlm_amd.TokenizedTexts.from_mask(ch["ids"].to(dev), ch["am"].to(dev))
    xm = m.soft_mask_input(x, mk, 0.7)
    logits = m(xm, ei, tokens, mk, plm_batch_size=ch["bs"])
    loss = F.cross_entropy(logits[mk], data["y"].to(dev)[mk], label_smoothing=0.2)
    loss.backward()
    bars = Bars(f"chameleon {mode}")
    bars.close("logits", logits.detach().cpu().numpy(), ch["ref"].numpy(), 0, 1e-4)
    bars.scalar("loss", abs(float(loss) - ch["loss"]), 1e-4)
    for k, p in m.named_parameters():
        ok = "plm_params." + k[len("plm_encoder."):].replace(".", "/") if k.startswith("plm_encoder.") else k
        r = ch["grads"].get(ok)
        if r is None or p.grad is None:
            assert (r is None or float(r.abs().max()) == 0) and (p.grad is None or float(p.grad.abs().max()) == 0), k
            continue
        rn, gn = float(r.double().norm()), float(p.grad.double().norm())
        bars.scalar("|grad| " + k, abs(rn - gn), 2e-3 * max(rn, 1e-4) + 1e-6)
    bars.finish()


# ------------------------------------------------------------------------------------------------------ Qwen3 vs HF float64
def _qwen3_run(plm, dev, cd, mode, h, packed):
    from gmlm_amd import qwen3
    m = copy.deepcopy(plm).to(dev).train()
    m.zero_grad()
    weights = qwen3.prepare_weights(m, cd, mode)
    if packed:
        tok, pos, cu, max_len = _packed_inputs(h["ids"], h["am"], h["lens"], dev)
        valid = qwen3.qwen3_encode_packed(m, tok, pos, cu, max_len, cd, True, False, weights)
    else:
        lens_d = h["lens"].to(dev, torch.int32)
        hs = qwen3.qwen3_encode(m, h["ids"].to(dev), lens_d, cd, True, False, weights)
        valid = hs[(torch.arange(L, device=dev)[None, :] < lens_d[:, None])]
    assert valid.dtype == cd and tuple(valid.shape) == (sum(LENS), 256)
    (valid.double() * h["proj"].to(dev)).sum().backward()
    return valid.detach().double().cpu(), {n: p.grad.detach().double().cpu() for n, p in m.named_parameters()}


@pytest.mark.parametrize("packed", [False, True], ids=["padded", "packed"])
def test_qwen3_bf16x3_vs_hf_float64(dev, hf, packed):  # noqa: F811
    """The tiny Qwen3 model of test_gpu_qwen3.py against HF float64: the fp32-storage bf16x3 run must have at most 1/32 of the
    relative L2 error of this project's bf16 run on the hidden states and on every parameter gradient, and must hold the fp32
    bars of that file (hidden states 1e-5, every gradient 2e-3 of its norm), which the native fp32 run is held to alongside."""
    ref_h, ref_g = hf["ref"]
    runs = {}
    for tag, cd, mode in (("bf16", torch.bfloat16, "native"), ("fp32", torch.float32, "native"), ("bf16x3", torch.float32, "bf16x3")):
        valid, grads = _qwen3_run(hf["plm"], dev, cd, mode, hf, packed)
        assert set(grads) == set(ref_g)
        err = {"hidden": float((valid - ref_h).norm() / ref_h.norm())}
        err.update({n: float((grads[n] - r).norm() / r.norm()) for n, r in ref_g.items()})
        runs[tag] = err
    bad = []
    for n in runs["bf16"]:
        e16, e32, e3 = runs["bf16"][n], runs["fp32"][n], runs["bf16x3"][n]
        bar = 1e-5 if n == "hidden" else 2e-3
        print(f"  {n}: rel l2 bf16 {e16:.2e}, bf16x3 {e3:.2e} ({e16 / e3:.0f}x), native fp32 {e32:.2e}; fp32 bar {bar:.0e}")
        if e32 > bar:
            bad.append(("native fp32 over the fp32 bar", n, e32))
        if e3 > bar:
            bad.append(("bf16x3 over the fp32 bar", n, e3))
        if e3 > e16 / 32:
            bad.append(("bf16x3 not 32x below bf16", n, e3, e16))
    assert not bad, bad


# ------------------------------------------------------------------------------------------------------- routing and surface
def _small_step(dev, **kw):
    """One forward + backward of a small full model (BERT head dim 64: the packed text pass): logits and every gradient."""
    import gmlm_amd
    plm = dict(hidden=128, layers=2, heads=2, inter=256, max_pos=64, vocab=200)
    cfg = dict(n=183, e=298, f_in=61, hc=32, c=5, plm=plm, seed=7)
    g = torch.Generator().manual_seed(0)
    x = torch.randn(cfg["n"], cfg["f_in"], generator=g).to(dev)
    ei = torch.randint(0, cfg["n"], (2, cfg["e"]), generator=g).to(dev)
    y = torch.randint(0, 5, (cfg["n"],), generator=g).to(dev)
    mask = (torch.rand(cfg["n"], generator=g) < 0.4).to(dev)
    ids, am = O.synthetic_tokens(cfg["n"], 16, 200, 1, 2)
    m = build_model(cfg, dev, **kw).train()
    tokens = gmlm_amd.TokenizedTexts.from_mask(ids.to(dev), am.to(dev))
    box = {}

    def run():
        logits = m(m.soft_mask_input(x, mask, 0.7), ei, tokens, mask, plm_batch_size=64)
        F.cross_entropy(logits[mask], y[mask], label_smoothing=0.2).backward()
        box["logits"] = logits.detach()

    ran = kernels_run(run)
    return m, box["logits"], {k: p.grad for k, p in m.named_parameters() if p.grad is not None}, ran


def test_recompute_takes_the_same_gemms(dev):
    """activation_checkpointing + plm_gradient_checkpointing on a bf16x3 model: bit-identical logits and gradients to the same
    step without recomputation, i.e. the recomputed blocks found the split weights again (a recompute that fell back to the
    native fp32 GEMM would differ in the last bits of every dense layer)."""
    _, l0, g0, ran0 = _small_step(dev, gemm_precision="bf16x3")
    _, l1, g1, ran1 = _small_step(dev, gemm_precision="bf16x3", activation_checkpointing=True, plm_gradient_checkpointing=True)
    split_kernels_ran(ran0, True)
    split_kernels_ran(ran1, True)
    assert torch.equal(l0, l1) and g0.keys() == g1.keys() and len(g0) > 40
    for k in g0:
        assert torch.equal(g0[k], g1[k]), k
    _, ln, _, rann = _small_step(dev)
    split_kernels_ran(rann, False)
    d = float((l0 - ln).abs().max())
    print(f"\n  small model: bf16x3 vs native fp32 logits differ by {d:.2e}")
    assert d > 0.0                                                         # the mode is really on


def test_native_is_the_default_bit_for_bit(dev):
    _, la, ga, ran = _small_step(dev, gemm_precision="native")
    _, lb, gb, _ = _small_step(dev)
    split_kernels_ran(ran, False)
    assert torch.equal(la, lb) and ga.keys() == gb.keys()
    for k in ga:
        assert torch.equal(ga[k], gb[k]), k


def test_capture_refuses_a_bf16x3_model(dev):
    plm = dict(hidden=128, layers=1, heads=2, inter=256, max_pos=64, vocab=200)
    cfg = dict(n=64, e=200, f_in=32, hc=16, c=3, plm=plm, seed=3)
    m = build_model(cfg, dev, gemm_precision="bf16x3").train()
    with pytest.raises(NotImplementedError, match="bf16x3"):
        m.capture_hip_graphs(torch.zeros(64, 32, device=dev), torch.zeros(2, 10, dtype=torch.long, device=dev))
    assert m._graphed is None
