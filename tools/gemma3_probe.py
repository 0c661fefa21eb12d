"""EmbeddingGemma-geometry text encoder, forward + backward in bf16: this project's kernel path (gmlm_amd.gemma3, packed pass,
which is what GraphTextLM runs) against HF's Gemma3TextModel under bf16 autocast with sdpa attention, on the same device,
alternating; the attention of one layer alone on the grouped-KV kernels at head dim 256 (gmlm_attention_gqa_d256_varlen_*)
against the only route the tree had before them, the wide-head family (gmlm_attention_wide_*) on the padded layout with K / V
expanded to one KV head per query head, the padding, the expansion copies and the fold of dK / dV CHARGED to that route; and the
sandwich RMSNorm kernel against the two add_rmsnorm launches it replaces, as bytes moved per second.

Workload: 24 layers, hidden 768, 3 query / 1 KV heads x 256, intermediate 1,152, bidirectional, sliding_window 512 (the geometry
used here for google/embeddinggemma-300m; it was stated from memory and not read from a model card), random weights, a cut vocabulary;
  short   1,257 sequences of 16-128 tokens (the headline workload's text batch), micro-batches of 419 sequences;
  long    256 sequences of 256-257 tokens (the longest the bidirectional window admits), micro-batches of 64.
Times: host clock around a device synchronise, ``--rounds`` alternating rounds after two warm-up rounds of each path, medians.
Writes one JSON file (``--out``) and prints it.  Needs a GPU.

    python tools/gemma3_probe.py --out profiles/gemma3_probe.json
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from qwen3_probe import batches, emit, kernel_table, pack, step_hf, step_packed, timed  # noqa: E402  (tools/ is the script dir)

HIDDEN, HQ, HKV, D, INTER = 768, 3, 1, 256, 1152


def build(layers, vocab, dev):
    from transformers import Gemma3TextConfig, Gemma3TextModel
    cfg = Gemma3TextConfig(vocab_size=vocab, hidden_size=HIDDEN, intermediate_size=INTER, num_hidden_layers=layers, num_attention_heads=HQ,
                           num_key_value_heads=HKV, head_dim=D, max_position_embeddings=2048, sliding_window=512,
                           use_bidirectional_attention=True, pad_token_id=0)
    cfg._attn_implementation = "sdpa"
    torch.manual_seed(0)
    with torch.device(dev):
        plm = Gemma3TextModel(cfg)
    with torch.no_grad():
        for n, p in plm.named_parameters():                          # HF's zero norm weights would hide the 1 + w path
            if p.dim() == 1:
                p.uniform_(-0.5, 0.5)
    return plm.train()


def med(v):
    return sorted(v)[len(v) // 2]


def run_encoder(plm, name, n_seq, lo, hi, vocab, batch, rounds, dev):
    from gmlm_amd import gemma3
    data, tokens = batches(n_seq, lo, hi, vocab, batch, dev)
    pdata = pack(data)
    paths = dict(packed=lambda: step_packed(plm, pdata, gemma3.prepare_weights, gemma3.gemma3_encode_packed), hf=lambda: step_hf(plm, data))
    grads = {}
    for k, fn in paths.items():                                  # first warm-up round; the gradients agree to bf16 accuracy
        fn()
        grads[k] = plm.layers[0].mlp.down_proj.weight.grad.double().clone()
    for fn in paths.values():                                   # second warm-up round
        fn()
    t = {k: [] for k in paths}
    for _ in range(rounds):
        for k, fn in paths.items():
            t[k].append(timed(fn))
    return dict(batch=name, sequences=n_seq, tokens=tokens, padded_tokens=int(sum(i.numel() for i, _, _ in data)), micro_batch=batch,
                micro_batches=len(data), rounds=rounds, **{k + "_ms": v for k, v in t.items()},
                **{k + "_median_ms": med(v) for k, v in t.items()}, **{k + "_range_ms": [min(v), max(v)] for k, v in t.items()},
                speedup_packed_vs_hf_median=med(t["hf"]) / med(t["packed"]),
                grad_rel_diff_layer0_down_proj=float((grads["packed"] - grads["hf"]).norm() / grads["hf"].norm()),
                packed_kernels=kernel_table(paths["packed"]), hf_kernels=kernel_table(paths["hf"]))


def run_attention(name, n_seq, lo, hi, reps, rounds, dev):
    """The attention of ONE layer over the whole batch: the packed grouped-KV call against wide:: on the padded, expanded layout."""
    from gmlm_amd import ops
    g = torch.Generator().manual_seed(2)
    lens = torch.randint(lo, hi + 1, (n_seq,), generator=g)
    cu = torch.zeros(n_seq + 1, dtype=torch.int32)
    cu[1:] = lens.cumsum(0)
    cu, rows, longest = cu.to(dev), int(lens.sum()), int(lens.max())
    lens_d = lens.to(dev, torch.int32)
    scale, rep = D ** -0.5, HQ // HKV
    nq, nk = HQ * D, HKV * D
    x = torch.randn(rows, (HQ + 2 * HKV) * D, generator=g).to(dev, torch.bfloat16)
    go = torch.randn(rows, nq, generator=g).to(dev, torch.bfloat16)
    seq = torch.repeat_interleave(torch.arange(n_seq, device=dev), lens_d.long(), output_size=rows)
    pos = torch.arange(rows, device=dev) - cu[seq].long()

    def native():
        """forward + backward through the C entry points (ops._causal_varlen_fwd / _bwd), reading the fused rows in place"""
        q, k, v = x[:, :nq], x[:, nq:nq + nk], x[:, nq + nk:]
        out, out_lo, lse = ops._causal_varlen_fwd(q, k, v, cu, n_seq, longest, HQ, HKV, scale, True, D, True)
        dx = torch.empty_like(x)
        ops._causal_varlen_bwd(q, k, v, out, out_lo, go, lse, cu, n_seq, longest, HQ, HKV, scale, dx[:, :nq], dx[:, nq:nq + nk],
                               dx[:, nq + nk:], D, True)
        return out, dx

    def expanded():
        """what the tree offered before: pad to [b, longest, .], expand K / V to HQ heads, wide:: attention, fold, unpad"""
        xp = x.new_zeros(n_seq, longest, (HQ + 2 * HKV) * D)
        xp[seq, pos] = x
        gp = go.new_zeros(n_seq, longest, nq)
        gp[seq, pos] = go
        q = xp[..., :nq].contiguous().requires_grad_(True)
        k = xp[..., nq:nq + nk].reshape(n_seq, longest, HKV, 1, D).expand(-1, -1, -1, rep, -1).reshape(n_seq, longest, nq).contiguous().requires_grad_(True)
        v = xp[..., nq + nk:].reshape(n_seq, longest, HKV, 1, D).expand(-1, -1, -1, rep, -1).reshape(n_seq, longest, nq).contiguous().requires_grad_(True)
        out = ops.attention(q, k, v, lens_d, HQ, scale, 0.0, True)
        out.backward(gp)
        fold = lambda t: t.view(n_seq, longest, HKV, rep, D).sum(3).reshape(n_seq, longest, nk)
        dx = torch.cat([q.grad, fold(k.grad), fold(v.grad)], -1)[seq, pos]
        return out.detach()[seq, pos], dx

    o_n, g_n = native()
    o_e, g_e = expanded()
    same = float((o_e.double() - o_n.double()).norm() / o_n.double().norm())
    same_g = float((g_e.double() - g_n.double()).norm() / g_n.double().norm())
    many = lambda fn: (lambda: [fn() for _ in range(reps)])
    many(native)(), many(expanded)()
    tn, te = [], []
    for _ in range(rounds):
        tn.append(timed(many(native)) / reps)
        te.append(timed(many(expanded)) / reps)
    return dict(batch=name, sequences=n_seq, rows=rows, longest=longest, hq=HQ, hkv=HKV, calls_per_round=reps, rounds=rounds,
                native_ms=tn, expanded_ms=te, native_median_ms=med(tn), expanded_median_ms=med(te),
                native_range_ms=[min(tn), max(tn)], expanded_range_ms=[min(te), max(te)],
                speedup_native_median=med(te) / med(tn), out_rel_diff=same, grad_rel_diff=same_g,
                native_kernels=kernel_table(native, top=8), expanded_kernels=kernel_table(expanded, top=8))


def run_rows(rows, f, reps, rounds, dev):
    """Forward of one norm pair on [rows, f] bf16: one sandwich launch against two add_rmsnorm launches.  Bytes counted once per
    tensor the PAIR must move at least: read s and b, write s' and y = 4 rows f 2 bytes; the two-launch form moves 7."""
    from gmlm_amd import ops
    g = torch.Generator().manual_seed(3)
    s, b = (torch.randn(rows, f, generator=g).to(dev, torch.bfloat16) for _ in range(2))
    w1, w2 = (torch.rand(f, generator=g).to(dev) for _ in range(2))
    one = lambda: [ops.sandwich_rmsnorm(s, b, w1, w2, 1.0, 1e-6) for _ in range(reps)]

    def two():
        for _ in range(reps):
            n = ops.add_rmsnorm(b, None, 1.0 + w1, 1e-6)[1]
            ops.add_rmsnorm(s, n, 1.0 + w2, 1e-6)

    with torch.no_grad():
        one(), two()
        t1, t2 = [], []
        for _ in range(rounds):
            t1.append(timed(one) / reps)
            t2.append(timed(two) / reps)
    need = 4 * rows * f * 2
    return dict(rows=rows, f=f, calls_per_round=reps, rounds=rounds, sandwich_ms=t1, two_add_rmsnorm_ms=t2, sandwich_median_ms=med(t1),
                two_add_rmsnorm_median_ms=med(t2), min_bytes=need, sandwich_tb_per_s=need / med(t1) / 1e9,
                two_add_rmsnorm_tb_per_s_of_the_same_bytes=need / med(t2) / 1e9, speedup_median=med(t2) / med(t1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", type=int, default=24)
    ap.add_argument("--vocab", type=int, default=4096)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--attn-reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("gemma3_probe needs a GPU (a CPU run measures nothing)")
    dev = torch.device("cuda:0")
    from gmlm_amd import gemma3
    plm = build(a.layers, a.vocab, dev)
    gemma3.check_supported(plm)
    res = dict(what="EmbeddingGemma geometry text encoder, bf16 forward + backward: packed kernel path vs HF bf16 autocast (sdpa), "
                    "alternating rounds in one process; grouped-KV attention at head dim 256 alone, gqaw:: on packed rows vs wide:: on "
                    "padded rows with K / V expanded (padding, expansion and fold charged); sandwich RMSNorm vs two add_rmsnorm launches",
               geometry_source="stated from memory for google/embeddinggemma-300m, not read from a model card",
               device=torch.cuda.get_device_name(0), layers=a.layers, hidden=HIDDEN, hq=HQ, hkv=HKV, head_dim=D, intermediate=INTER,
               vocab=a.vocab, attn_implementation_hf=str(getattr(plm.config, "_attn_implementation", None)),
               kernel_figures_source="torch.profiler device events, one pass per path after the timed rounds",
               encoder=[run_encoder(plm, "short", 1257, 16, 128, a.vocab, 419, a.rounds, dev),
                        run_encoder(plm, "long", 256, 256, 257, a.vocab, 64, a.rounds, dev)],
               attention=[run_attention("short", 1257, 16, 128, a.attn_reps, a.rounds, dev),
                          run_attention("long", 256, 256, 257, a.attn_reps, a.rounds, dev)],
               rows=[run_rows(100_000, 768, 10, a.rounds, dev), run_rows(65_792, 1152, 10, a.rounds, dev)])
    emit(res, a.out)


if __name__ == "__main__":
    main()
