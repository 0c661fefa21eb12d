"""Probe: the LDS-resident short-sequence attention at head dim 32 (attn_d32_short.hip, ``d32s::`` kernels, ``groups`` given) against
the route a 384-wide BERT encoder (12 heads x 32: the MiniLM-L6 geometry) took before it: the streaming ``d32::`` kernels, i.e. the
same call with ``groups=None`` and, for the QKV bias gradient, ``ops.column_sum`` over dqkv charged to it.

One process.  Every shape is warmed up first, then five rounds alternate the sides; each figure is [median, min, max] over the rounds.
 (a) attention alone (device events): 1,257 sequences of 16-128 tokens, forward and forward + backward at p = 0 and p = 0.1, without
     and with the bias sums; achieved TB/s over the tensors each route reads and writes (q, k, v, o forward, + out_lo on the streaming
     route; q, k, v, dO, dq, dk, dv backward, + o, out_lo on the streaming route);
 (b) the encoder pass, forward + backward (host clock around a synchronise): 6 layers x 384, the same sequences in one micro-batch;
 (c) the threshold: the same length mix at 8, 16, 32, 43, 64 and 128 sequences (96 to 1,536 (sequence, head) pairs), forward +
     backward with the bias sums, both routes (the new one forced below its threshold by setting ``ops.D32_SHORT_MIN_PAIRS = 0``).

    python tools/attn_d32_short_probe.py profiles/attn_d32_short_probe.json"""
import json
import statistics
import sys
import time

import torch

sys.path.insert(0, ".")
from gmlm_amd import bert, ops  # noqa: E402

dev = torch.device("cuda")
H, D, P = 12, 32, 384
ROUNDS = 5
BF = torch.bfloat16


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
    """{name: fn} -> {name: [median, min, max]}: three warm-up calls of every side, then ROUNDS rounds that visit the sides in turn."""
    for fn in sides.values():
        for _ in range(3):
            fn()
    got = {k: [] for k in sides}
    for _ in range(ROUNDS):
        for k, fn in sides.items():
            got[k].append(timer(fn))
    return {k: [round(statistics.median(v), 2), round(min(v), 2), round(max(v), 2)] for k, v in got.items()}


def problem(n_seq):
    lens = lengths(n_seq)
    t, l = int(lens.sum()), int(lens.max())
    g = torch.Generator().manual_seed(2)
    qkv = torch.randn(t, 3 * P, generator=g).to(dev, BF).requires_grad_(True)
    go = torch.randn(t, P, generator=g).to(dev, BF)
    cu = torch.zeros(n_seq + 1, dtype=torch.int32)
    cu[1:] = torch.cumsum(lens, 0)
    masters = tuple(torch.zeros(P, device=dev, requires_grad=True) for _ in range(3))
    return dict(lens=lens, t=t, l=l, qkv=qkv, go=go, cu=cu.to(dev), groups=ops.pack_sequence_groups(lens.tolist()).to(dev),
                pairs=float((lens.double() ** 2).sum()), masters=masters)


def sides(pr, p, bias):
    """forward and forward + backward of both routes on one problem"""
    qkv, go, masters = pr["qkv"], pr["go"], pr["masters"] if bias else ()

    def fwd(groups):
        return lambda: ops.AttentionQKV.apply(qkv, None, H, D ** -0.5, p, 7, pr["cu"], pr["l"], pr["pairs"], groups, *masters)

    def fb(groups):
        f = fwd(groups)

        def run():
            qkv.grad = None
            for m in masters:
                m.grad = None
            f().backward(go)
        return run

    return {"stream_fwd": fwd(None), "short_fwd": fwd(pr["groups"]), "stream_fwd_bwd": fb(None), "short_fwd_bwd": fb(pr["groups"])}


def attention_alone(p, bias):
    pr = problem(1257)
    assert ops._d32_short_path(pr["groups"], BF, D, pr["l"], 1257, H)
    r = alternate(sides(pr, p, bias), events)
    nb = pr["t"] * P * 2                                       # bytes of one of q, k, v, o
    tb = lambda n, us: round(n * nb / (us * 1e-6) / 1e12, 2)
    bwd = {k: round(r[k + "_fwd_bwd"][0] - r[k + "_fwd"][0], 2) for k in ("stream", "short")}
    return dict(case=f"attention alone, 1257 sequences 16-128 tokens ({pr['t']} rows, {pr['groups'].numel() - 1} groups), bf16, p={p}, "
                     f"bias sums {'on (stream: + ops.column_sum)' if bias else 'off'}", unit="us", **r,
                stream_bwd=bwd["stream"], short_bwd=bwd["short"],
                tb_per_s=dict(stream_fwd=tb(5, r["stream_fwd"][0]), short_fwd=tb(4, r["short_fwd"][0]),
                              stream_bwd=tb(9, bwd["stream"]), short_bwd=tb(7, bwd["short"])),
                speedup_fwd=round(r["stream_fwd"][0] / r["short_fwd"][0], 2),
                speedup_fwd_bwd=round(r["stream_fwd_bwd"][0] / r["short_fwd_bwd"][0], 2))


def encoder_pass():
    from transformers import BertConfig, BertModel
    torch.manual_seed(0)
    plm = BertModel(BertConfig(vocab_size=30522, hidden_size=P, num_hidden_layers=6, num_attention_heads=H, intermediate_size=4 * P,
                               max_position_embeddings=512, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)).to(dev).train()
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
    gp = torch.randn(b, P, generator=g).to(dev)
    rows = torch.arange(b, device=dev)
    pairs = float((lens.double() ** 2).sum())
    groups = ops.pack_sequence_groups(lens.tolist()).to(dev)

    def step(gr):
        def run():
            plm.zero_grad(set_to_none=True)
            hs = bert.bert_encode_packed(plm, tok, pos, cu, l, BF, training=True, pair_count=pairs, groups=gr)
            (ops.MeanPoolScatter.apply(torch.zeros(b, P, device=dev), hs, None, rows, cu, t) * gp).sum().backward()
        return run

    r = alternate({"stream": step(None), "short": step(groups)}, host)
    return dict(case=f"encoder pass fwd+bwd, 6 layers x 384, {b} sequences in one micro-batch, bf16", unit="ms", **r,
                speedup=round(r["stream"][0] / r["short"][0], 3))


def threshold():
    saved, ops.D32_SHORT_MIN_PAIRS = ops.D32_SHORT_MIN_PAIRS, 0
    try:
        rows = []
        for n in (8, 16, 32, 43, 64, 128):
            pr = problem(n)
            s = sides(pr, 0.0, True)
            r = alternate({k: s[k] for k in ("stream_fwd_bwd", "short_fwd_bwd")}, lambda fn: events(fn, 50))
            rows.append(dict(sequences=n, pairs=n * H, rows=pr["t"], groups=pr["groups"].numel() - 1, **r,
                             short_over_stream=round(r["short_fwd_bwd"][0] / r["stream_fwd_bwd"][0], 3)))
        return dict(case="threshold: fwd+bwd with bias sums, 12 x 32, bf16, p=0, both routes (the new one forced)", unit="us", rows=rows)
    finally:
        ops.D32_SHORT_MIN_PAIRS = saved


if __name__ == "__main__":
    out = []
    for fn, args in ((attention_alone, (0.0, False)), (attention_alone, (0.1, False)), (attention_alone, (0.0, True)),
                     (attention_alone, (0.1, True)), (threshold, ()), (encoder_pass, ())):
        out.append(fn(*args))
        print(json.dumps(out[-1]), flush=True)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            what = ("tools/attn_d32_short_probe.py: [median, min, max] over 5 alternating rounds on " + torch.cuda.get_device_name(0) +
                    "; stream = the parent route (d32:: streaming kernels, groups=None, column_sum for the bias gradient), short = d32s::")
            f.write('{"what": %s,\n "rows": [\n' % json.dumps(what) + ",\n".join("  " + json.dumps(r) for r in out) + "\n ]}\n")
