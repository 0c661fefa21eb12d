"""Probe: what the native head-dim-32 route (attn_d32.hip, packed pass, whole-step graph) changes for a 384-wide BERT encoder
(12 heads x 32: the MiniLM-L6 geometry), against the route such an encoder took before (``bert.NATIVE_HEAD_DIMS`` set back to
(64, 96): the padded pass with unfused Q / K / V zero-padded to head dim 64 through ``nn.attention_any_dim``).

One process.  Every shape is warmed up first, then five rounds alternate the two sides; each figure is the median with
[min, max] over the rounds.
 (a) attention alone (device events): 1,257 sequences of 16-128 tokens, forward and backward, native packed against the
     padded batch zero-padded to 64;
 (b) the encoder pass, forward + backward (host clock around a synchronise): 6 layers x 384, the same sequences in one
     micro-batch, native packed against the old route;
 (c) a Cornell-size model (183 nodes, 298 edges, 1,703 features) on that encoder: eager step against the whole-step graph.

    python tools/attn_d32_probe.py profiles/attn_d32_probe.json"""
import json
import statistics
import sys
import time

import torch
import torch.nn.functional as F

sys.path.insert(0, ".")
import gmlm_amd  # noqa: E402
from gmlm_amd import bert, nn as gnn, ops  # noqa: E402

dev = torch.device("cuda")
H, D, P = 12, 32, 384
ROUNDS = 5


def lengths(n, seed=1):
    return torch.randint(16, 129, (n,), generator=torch.Generator().manual_seed(seed))


def events(fn, n=10):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(n):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / n * 1e3                     # us


def host(fn, n=5):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n * 1e3            # ms


def alternate(sides, timer):
    """{name: fn} -> {name: [median, min, max]}: one warm-up of every side, then ROUNDS rounds that visit the sides in turn."""
    for fn in sides.values():
        for _ in range(3):
            fn()
    got = {k: [] for k in sides}
    for _ in range(ROUNDS):
        for k, fn in sides.items():
            got[k].append(timer(fn))
    return {k: [round(statistics.median(v), 2), round(min(v), 2), round(max(v), 2)] for k, v in got.items()}


def attention_alone(dtype, p=0.0):
    lens = lengths(1257)
    t, l, b = int(lens.sum()), int(lens.max()), lens.numel()
    g = torch.Generator().manual_seed(2)
    qkv = torch.randn(t, 3 * P, generator=g).to(dev, dtype).requires_grad_(True)
    go = torch.randn(t, P, generator=g).to(dev, dtype)
    cu = torch.zeros(b + 1, dtype=torch.int32)
    cu[1:] = torch.cumsum(lens, 0)
    cu = cu.to(dev)
    scale = D ** -0.5
    pairs = float((lens.double() ** 2).sum())
    # today's route: the padded batch [b, l, 384], three unfused operands, heads zero-padded to 64 inside attention_any_dim
    keep = (torch.arange(l)[None, :] < lens[:, None]).to(dev)
    pad = torch.zeros(b, l, 3 * P, device=dev, dtype=dtype)
    pad[keep] = qkv.detach()
    q, k, v = (pad[..., i * P:(i + 1) * P].clone().requires_grad_(True) for i in range(3))
    gop = torch.zeros(b, l, P, device=dev, dtype=dtype)
    gop[keep] = go
    kv_len = lens.to(dev, torch.int32)

    def nat_f():
        return ops.AttentionQKV.apply(qkv, None, H, scale, p, 7, cu, l, pairs)

    def nat_fb():
        qkv.grad = None
        nat_f().backward(go)

    def old_f():
        return gnn.attention_any_dim(q, k, v, kv_len, H, scale, p, p > 0)

    def old_fb():
        q.grad = k.grad = v.grad = None
        old_f().backward(gop)

    r = alternate({"native_fwd": nat_f, "old_fwd": old_f, "native_fwd_bwd": nat_fb, "old_fwd_bwd": old_fb}, events)
    return dict(case=f"attention alone, {b} sequences 16-128 tokens ({t} rows real, {b * l} padded), {str(dtype)[6:]}, p={p}", unit="us",
                **r, native_bwd=round(r["native_fwd_bwd"][0] - r["native_fwd"][0], 2), old_bwd=round(r["old_fwd_bwd"][0] - r["old_fwd"][0], 2),
                speedup_fwd_bwd=round(r["old_fwd_bwd"][0] / r["native_fwd_bwd"][0], 2))


def encoder(layers=6, max_pos=512, vocab=30522):
    from transformers import BertConfig, BertModel
    torch.manual_seed(0)
    return BertModel(BertConfig(vocab_size=vocab, hidden_size=P, num_hidden_layers=layers, num_attention_heads=H,
                                intermediate_size=4 * P, max_position_embeddings=max_pos, hidden_dropout_prob=0.0,
                                attention_probs_dropout_prob=0.0))


def encoder_pass(dtype):
    plm = encoder().to(dev).train()
    lens = lengths(1257)
    t, l, b = int(lens.sum()), int(lens.max()), lens.numel()
    g = torch.Generator().manual_seed(3)
    am = torch.arange(l)[None, :] < lens[:, None]
    ids = (torch.randint(5, 30522, (b, l), generator=g) * am).to(dev)
    keep = am.to(dev)
    tok, pos = ids[keep], torch.arange(l, device=dev)[None, :].expand(b, l)[keep]
    cu = torch.zeros(b + 1, dtype=torch.int32)
    cu[1:] = torch.cumsum(lens, 0)
    cu = cu.to(dev)
    lens_d = lens.to(dev, torch.int32)
    gp = torch.randn(b, P, generator=g).to(dev)
    rows = torch.arange(b, device=dev)
    pairs = float((lens.double() ** 2).sum())

    def native():
        plm.zero_grad(set_to_none=True)
        hs = bert.bert_encode_packed(plm, tok, pos, cu, l, dtype, training=True, pair_count=pairs)
        (ops.MeanPoolScatter.apply(torch.zeros(b, P, device=dev), hs, None, rows, cu, t) * gp).sum().backward()

    def old():
        plm.zero_grad(set_to_none=True)
        saved, bert.NATIVE_HEAD_DIMS = bert.NATIVE_HEAD_DIMS, (64, 96)
        try:
            hs = bert.bert_encode(plm, ids, lens_d, dtype, training=True)
            (ops.MeanPoolScatter.apply(torch.zeros(b, P, device=dev), hs, lens_d, rows) * gp).sum().backward()
        finally:
            bert.NATIVE_HEAD_DIMS = saved

    r = alternate({"native_packed": native, "old_route": old}, host)
    return dict(case=f"encoder pass fwd+bwd, 6 layers x 384, {b} sequences in one micro-batch, {str(dtype)[6:]}", unit="ms", **r,
                row_ratio=round(t / (b * l), 3), speedup=round(r["old_route"][0] / r["native_packed"][0], 2))


def cornell(dtype):
    n, e, f_in, c = 183, 298, 1703, 5
    g = torch.Generator().manual_seed(1003)
    x = torch.randn(n, f_in, generator=g).to(dev)
    ei = torch.randint(0, n, (2, e), generator=g).to(dev)
    y = torch.randint(0, c, (n,), generator=g).to(dev)
    active = (torch.rand(n, generator=g) < 0.24).to(dev)
    lens = lengths(n, 4)
    am = (torch.arange(128)[None, :] < lens[:, None]).long()
    ids = torch.randint(5, 30522, (n, 128), generator=g) * am
    tokens = gmlm_amd.TokenizedTexts.from_mask(ids.to(dev), am.to(dev))

    def model():
        return gmlm_amd.GraphTextLM(f_in, 512, c, dropout_rate=0.3, plm_encoder=encoder(), plm_max_length=128,
                                    compute_dtype=dtype).to(dev).train()

    eager, graphed = model(), model()
    graphed.capture_hip_graphs(graphed.soft_mask_input(x, active, 0.7), ei, encoder=True, whole_step=True)

    def step(m):
        def run():
            m.zero_grad(set_to_none=True)
            logits = m(m.soft_mask_input(x, active, 0.7), ei, tokens, active, plm_batch_size=512)
            F.cross_entropy(logits[active], y[active], label_smoothing=0.2).backward()
        return run

    r = alternate({"eager": step(eager), "whole_step_graph": step(graphed)}, lambda fn: host(fn, 10))
    return dict(case=f"Cornell-size step (183 nodes, {int(active.sum())} active texts), 6 x 384 encoder, {str(dtype)[6:]}", unit="ms", **r,
                speedup=round(r["eager"][0] / r["whole_step_graph"][0], 2))


if __name__ == "__main__":
    rows = []
    for fn, args in ((attention_alone, (torch.bfloat16,)), (attention_alone, (torch.bfloat16, 0.1)), (attention_alone, (torch.float32,)),
                     (encoder_pass, (torch.bfloat16,)), (encoder_pass, (torch.float32,)), (cornell, (torch.bfloat16,))):
        rows.append(fn(*args))
        print(json.dumps(rows[-1]), flush=True)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            what = "tools/attn_d32_probe.py: median [median, min, max] over 5 alternating rounds"
            f.write('{"what": %s,\n "rows": [\n' % json.dumps(what) + ",\n".join("  " + json.dumps(r) for r in rows) + "\n ]}\n")
