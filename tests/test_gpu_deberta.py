"""The DeBERTa-v2 / v3 encoder pass (gmlm_amd.deberta) and a GraphTextLM built on it against the installed
transformers.DebertaV2Model in float64 on the CPU, seeded random weights, LayerNorm weights drawn from U(0.5, 1.5) and
``encoder.rel_embeddings`` from N(0, 1) so that both matter.

Tiny model: 2 layers, hidden 128 = 2 heads x 64, intermediate 192, vocab 96, position_buckets 16, max_relative_positions 40
(the identity region ends at 9, log runs reach 8), dropouts 0; two batches: eight sequences of 1..40 tokens, and four of up to
100 tokens (past max_relative_positions: the clamped columns), token ids >= 1, train mode, loss = a fixed random projection of
the valid hidden states.  The float64 reference runs every sequence ALONE, unpadded, and adds the gradients up, as
tests/test_gpu_mpnet.py does (HF's padded float64 run equals it exactly per token).
fp32 budgets are the tree's model budgets: hidden states rel-L2 1e-5, every parameter gradient within 2e-3 of its norm,
``encoder.rel_embeddings.weight``, ``encoder.LayerNorm.*`` and every ``query_proj`` / ``key_proj`` bias included (in this encoder
the key bias has a gradient: it enters k_j . Qr[c]).  The bf16 bound is measured, not fixed: HF's own model in bf16 on the CPU
(the same per-sequence run) against float64 gives each tensor's bf16 floor, and each tensor of this path must be within 2x that
floor.
One GraphTextLM step on a Cornell-size graph: logits and the gradient of the relative embeddings against the SAME model with
its text embeddings taken from HF's encoder in float64.  Budgets: the gradient 2e-3; the logits 1e-4 rel-L2.  With the config's
dropouts at 0.1 / 0.1 the step is finite and two steps from the same seeds are bit-equal."""
import copy

import pytest
import torch
import torch.nn.functional as F

from helpers import kernels_run

pytestmark = pytest.mark.gpu

BATCHES = {"short": [1, 5, 9, 10, 17, 32, 33, 40], "long": [100, 41, 64, 7]}
P = 128
PAD = 0
REL = "encoder.rel_embeddings.weight"


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _config(**kw):
    from transformers import DebertaV2Config
    base = dict(vocab_size=96, hidden_size=P, intermediate_size=192, num_hidden_layers=2, num_attention_heads=2,
                max_position_embeddings=128, relative_attention=True, pos_att_type=["p2c", "c2p"], share_att_key=True,
                norm_rel_ebd="layer_norm", position_buckets=16, max_relative_positions=40, position_biased_input=False,
                type_vocab_size=0, layer_norm_eps=1e-7, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)
    base.update(kw)
    return DebertaV2Config(**base)


def _make_plm(seed=0, **kw):
    from transformers import DebertaV2Model
    torch.manual_seed(seed)
    plm = DebertaV2Model(_config(**kw))
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for n, p in plm.named_parameters():
            if "LayerNorm.weight" in n:
                p.copy_(torch.empty_like(p).uniform_(0.5, 1.5, generator=g))
            elif "embeddings" in n or p.dim() == 1:
                p.copy_(torch.randn(p.shape, generator=g) * (1.0 if p.dim() == 2 else 0.1))
            else:
                p.copy_(torch.randn(p.shape, generator=g) * p.shape[1] ** -0.5)
    return plm.train()


def _tokens(lens, seed=3):
    g = torch.Generator().manual_seed(seed)
    l = max(lens)
    ids = torch.randint(1, 96, (len(lens), l), generator=g)
    lens = torch.tensor(lens)
    am = torch.arange(l)[None, :] < lens[:, None]
    return torch.where(am, ids, torch.full_like(ids, PAD)), lens


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
    """The float64 references and the bf16 / fp32 floors of HF's own model, computed once per batch."""
    plm = _make_plm()
    out = dict(plm=plm)
    for name, lens_l in BATCHES.items():
        ids, lens = _tokens(lens_l)
        proj = torch.randn(int(lens.sum()), P, generator=torch.Generator().manual_seed(9), dtype=torch.float64) / 16
        ref = _hf_run(plm, torch.float64, ids, lens, proj)
        assert bool(torch.isfinite(ref[0]).all()) and all(bool(torch.isfinite(g).all()) for g in ref[1].values())
        floors = {}
        for dt in (torch.bfloat16, torch.float32):
            hs, gr = _hf_run(plm, dt, ids, lens, proj)
            fl = {"hidden": float((hs - ref[0]).norm() / ref[0].norm())}
            fl.update({n: float((gr[n] - ref[1][n]).norm() / ref[1][n].norm()) for n in gr})
            floors[dt] = fl
        out[name] = dict(ids=ids, lens=lens, proj=proj, ref=ref, floors=floors)
    return out


def test_hf_padded_run_equals_the_per_sequence_run():
    """What makes the unpadded per-sequence run a fair reference: HF's own padded forward gives the same valid rows."""
    plm = _make_plm().double().eval()
    ids, lens = _tokens(BATCHES["long"])
    am = torch.arange(ids.shape[1])[None, :] < lens[:, None]
    with torch.no_grad():
        padded = plm(input_ids=ids, attention_mask=am.long()).last_hidden_state
        for i, n in enumerate(lens.tolist()):
            alone = plm(input_ids=ids[i:i + 1, :n]).last_hidden_state[0]
            assert float((padded[i, :n] - alone).abs().max()) <= 1e-12


def _ours(plm, dev, cd, ids, lens, proj, checkpointing=False, packed=False):
    from gmlm_amd import deberta
    m = copy.deepcopy(plm).to(dev).train()
    m.zero_grad()
    lens_d = lens.to(dev, torch.int32)
    if packed:
        am = torch.arange(ids.shape[1])[None, :] < lens[:, None]
        tok = ids[am].to(dev)
        pos = torch.cat([torch.arange(n) for n in lens.tolist()]).to(dev)
        cu = torch.tensor([0] + lens.cumsum(0).tolist(), dtype=torch.int32, device=dev)
        hs = valid_rows = deberta.deberta_encode_packed(m, tok, pos, cu, int(lens.max()), cd, True, checkpointing)
    else:
        hs = deberta.deberta_encode(m, ids.to(dev), lens_d, cd, True, checkpointing)
        valid_rows = hs[(torch.arange(ids.shape[1], device=dev)[None, :] < lens_d[:, None])]
    (valid_rows.double() * proj.to(dev)).sum().backward()
    return hs.detach(), valid_rows.detach().double().cpu(), {n: p.grad.detach().double().cpu() for n, p in m.named_parameters()}


def _assert_kernels(ran, tn, drop=False):
    dr = "true" if drop else "false"
    want = {f"disent::{k}_kernel<{tn}, {dr}>" for k in ("fwd", "dq", "dkv", "dc", "dpt")} | {f"disent::delta_kernel<{tn}>"}
    assert {n for n in ran if n.startswith("disent::")} == want, sorted(ran)
    assert not any(n.startswith(("attn_", "d32::", "d128::", "mbert::", "relb::", "causal128::", "rmsnorm_", "swiglu_")) for n in ran), sorted(ran)


CASES = [(b, p) for b in BATCHES for p in (False, True)]
IDS = [f"{b}-{'packed' if p else 'padded'}" for b, p in CASES]


@pytest.mark.parametrize("batch,packed", CASES, ids=IDS)
def test_encoder_fp32_vs_hf_float64(dev, hf, batch, packed):
    t = hf[batch]
    box = {}
    ran = kernels_run(lambda: box.setdefault("r", _ours(hf["plm"], dev, torch.float32, t["ids"], t["lens"], t["proj"], packed=packed)))
    _assert_kernels(ran, "float")
    hs, valid, grads = box["r"]
    assert bool(torch.isfinite(hs).all())                         # padded rows included
    assert hs.shape == ((int(t["lens"].sum()), P) if packed else (len(t["lens"]), int(t["lens"].max()), P))
    ref_h, ref_g = t["ref"]
    fl = t["floors"][torch.float32]
    e = float((valid - ref_h).norm() / ref_h.norm())
    print(f"  hidden: rel l2 = {e:.2e} (HF fp32 floor {fl['hidden']:.2e})")
    assert e <= 1e-5
    assert set(grads) == set(ref_g) and {REL, "encoder.LayerNorm.weight", "encoder.LayerNorm.bias"} <= set(ref_g)
    assert sum(n.endswith(("query_proj.bias", "key_proj.bias")) for n in ref_g) == 4
    for n, r in ref_g.items():
        e = float((grads[n] - r).norm() / r.norm())
        print(f"  {n}: rel l2 = {e:.2e} (HF fp32 floor {fl[n]:.2e})")
        assert float(r.norm()) > 0 and e <= 2e-3, (n, e)
    # rows of the relative embeddings that no pair of the batch reaches take no gradient
    from gmlm_amd import deberta
    cols = deberta.bucket_columns(int(t["lens"].max()), 16, 40)
    rel_g = grads[REL]
    assert float(rel_g[:cols.first].abs().sum()) == 0.0 and float(rel_g[cols.first + cols.width:].abs().sum()) == 0.0
    assert float(rel_g[cols.first].abs().max()) > 0 and float(rel_g[cols.first + cols.width - 1].abs().max()) > 0


@pytest.mark.parametrize("batch,packed", CASES, ids=IDS)
def test_encoder_bf16_within_twice_the_hf_bf16_floor(dev, hf, batch, packed):
    """Every tensor (valid hidden states, each parameter gradient) within 2x the error of HF's own bf16 run; the ratios are
    printed per tensor (DESIGN.md section 4 "DeBERTa encoder")."""
    t = hf[batch]
    box = {}
    ran = kernels_run(lambda: box.setdefault("r", _ours(hf["plm"], dev, torch.bfloat16, t["ids"], t["lens"], t["proj"], packed=packed)))
    _assert_kernels(ran, "unsigned short")
    hs, valid, grads = box["r"]
    assert hs.dtype == torch.bfloat16 and bool(torch.isfinite(hs).all())
    ref_h, ref_g = t["ref"]
    fl = t["floors"][torch.bfloat16]
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
@pytest.mark.parametrize("cd", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_gradient_checkpointing_is_bit_identical_with_dropout(dev, cd, packed):
    """Dropout on (hidden, attention probabilities and the relative embeddings of every layer): the checkpointed layers replay
    the kernels' seeds and torch's mask of the relative embeddings."""
    plm = _make_plm(hidden_dropout_prob=0.1, attention_probs_dropout_prob=0.1)
    ids, lens = _tokens(BATCHES["long"])
    proj = torch.randn(int(lens.sum()), P, generator=torch.Generator().manual_seed(9), dtype=torch.float64) / 16
    runs = []
    for ck in (False, True, False):
        torch.manual_seed(21)
        runs.append(_ours(plm, dev, cd, ids, lens, proj, checkpointing=ck, packed=packed))
    a, b, c = runs
    assert torch.equal(a[0], b[0]) and torch.equal(a[0], c[0])
    for n in a[2]:
        assert torch.equal(a[2][n], b[2][n]), n
    torch.manual_seed(22)
    other = _ours(plm, dev, cd, ids, lens, proj, packed=packed)
    assert not torch.equal(other[0], a[0])                          # another seed, another mask
    plain = _ours(_make_plm(), dev, cd, ids, lens, proj, packed=packed)
    assert not torch.equal(plain[2][REL], a[2][REL])


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
    ids = torch.where(am, torch.randint(1, 96, (n, width), generator=g), torch.full((n, width), PAD))
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
    assert "disent::fwd_kernel<float, false>" in ran, sorted(ran)
    logits = box["l"]
    F.cross_entropy(logits[mk], y[mk], label_smoothing=0.2).backward()
    names = (REL, "encoder.LayerNorm.weight", "encoder.layer.1.attention.self.key_proj.bias", "embeddings.word_embeddings.weight")
    got = {k: dict(m.plm_encoder.named_parameters())[k].grad.detach().double().cpu() for k in names}

    # the same model, its text embeddings from HF's encoder in float64 on the CPU (mean pooling of main.py:351-358)
    ref_plm = copy.deepcopy(hf["plm"]).double().train()
    active = mask.nonzero().flatten().tolist()
    pooled = torch.stack([ref_plm(input_ids=ids[i:i + 1, :int(lens[i])]).last_hidden_state[0].mean(0) for i in active])
    embeds = torch.zeros(n, P, dtype=torch.float64).index_put((mask.nonzero().flatten(),), pooled)
    m.zero_grad()
    ref_logits = m.head(m.get_graph_embeddings(m.soft_mask_input(x, mk, 0.7), ei), embeds.to(dev).float())
    F.cross_entropy(ref_logits[mk], y[mk], label_smoothing=0.2).backward()
    ref = {k: dict(ref_plm.named_parameters())[k].grad for k in names}

    e_l = float((logits.detach().double() - ref_logits.detach().double()).norm() / ref_logits.detach().double().norm())
    print(f"  logits: rel l2 = {e_l:.2e}")
    assert e_l <= 1e-4
    for k in names:
        e_g = float((got[k] - ref[k]).norm() / ref[k].norm())
        print(f"  {k} gradient: rel l2 = {e_g:.2e}")
        assert float(ref[k].norm()) > 0 and e_g <= 2e-3, (k, e_g)
    sd = m.state_dict()
    assert "plm_encoder." + REL in sd and "plm_encoder.encoder.layer.1.attention.self.query_proj.weight" in sd


def test_graph_text_lm_step_with_dropout_is_finite_and_replayable(dev):
    """hidden_dropout_prob = attention_probs_dropout_prob = 0.1 (DeBERTa's defaults): finite, and bit-equal from equal seeds."""
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
        assert "disent::fwd_kernel<float, true>" in ran, sorted(ran)
        logits = box["l"]
        loss = F.cross_entropy(logits[mk], y[mk], label_smoothing=0.2)
        loss.backward()
        grads = {k: p.grad.detach().clone() for k, p in m.plm_encoder.named_parameters()}
        assert bool(torch.isfinite(loss)) and all(bool(torch.isfinite(g).all()) for g in grads.values())
        assert float(grads[REL].abs().max()) > 0
        runs.append((logits.detach().clone(), grads))
    assert torch.equal(runs[0][0], runs[1][0])
    for k in runs[0][1]:
        assert torch.equal(runs[0][1][k], runs[1][1][k]), k
    torch.manual_seed(12)
    other = m(m.soft_mask_input(x, mk, 0.7), ei, tokens, mk, plm_batch_size=32)
    assert not torch.equal(other, runs[0][0])                      # another seed, another mask
