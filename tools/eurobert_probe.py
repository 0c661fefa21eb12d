"""EuroBERT-610m-geometry text encoder, forward + backward in bf16: this project's kernel path (gmlm_amd.eurobert, packed pass,
which is what GraphTextLM runs, and padded pass) against HF's EuroBertModel under bf16 autocast with sdpa attention, on the same
device, alternating; and the attention of one layer alone on the native grouped kernels (gmlm_attention_bidir_gqa_varlen_*)
against the same heads with K / V expanded to one KV head per query head and run through ``ops.attention_qkv`` (the
bidirectional family of the BERT encoder, with its short-sequence work items where they apply), alternating.

Workload: 26 layers, hidden 1,152, 18 query / 6 KV heads x 64, intermediate 4,096 (the geometry used here for EuroBERT-610m; it
was not read from a model card), no biases, random weights, a cut vocabulary;
  short   1,257 sequences of 16-128 tokens (the headline workload's text batch), micro-batches of 419 sequences;
  long    256 sequences of 256-512 tokens, micro-batches of 32.
Length-sorted micro-batches; HF and the padded pass see each padded to its longest sequence, the packed pass sees [T, .] rows.
Times: host clock around a device synchronise, ``--rounds`` alternating rounds after two warm-up rounds of each path.  The
attention comparison times forward + backward on prebuilt operands, ``--attn-reps`` calls per round: the native route through
the C entry points, the expanded route through its autograd node (one node, no slice gradients); the expansion is built here
only, and its copies (and the sum over each group that would fold dK / dV back) are NOT charged to the expanded route.  Device
kernel time of one further pass per route is reported beside the host clock (``*_kernels.total_kernel_ms``), so that host
overhead cannot decide the comparison.  Kernel tables: torch.profiler device events, after the timed rounds.  Writes one JSON
file (``--out``) and prints it.  Needs a GPU.

    python tools/eurobert_probe.py --out profiles/eurobert_probe.json
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from qwen3_probe import batches, emit, kernel_table, pack, step_hf, step_ours, step_packed, timed  # noqa: E402  (tools/ is the script dir)

HIDDEN, HQ, HKV, D, INTER = 1152, 18, 6, 64, 4096


def build(layers, vocab, dev):
    from transformers import EuroBertConfig, EuroBertModel
    cfg = EuroBertConfig(vocab_size=vocab, hidden_size=HIDDEN, intermediate_size=INTER, num_hidden_layers=layers, num_attention_heads=HQ,
                         num_key_value_heads=HKV, max_position_embeddings=512, tie_word_embeddings=False, pad_token_id=0, bos_token_id=1,
                         eos_token_id=2, mask_token_id=3)
    cfg._attn_implementation = "sdpa"
    torch.manual_seed(0)
    with torch.device(dev):
        plm = EuroBertModel(cfg)
    return plm.train()


def med(v):
    return sorted(v)[len(v) // 2]


def run_encoder(plm, name, n_seq, lo, hi, vocab, batch, rounds, dev):
    from gmlm_amd import eurobert
    data, tokens = batches(n_seq, lo, hi, vocab, batch, dev)
    pdata = pack(data)
    paths = dict(packed=lambda: step_packed(plm, pdata, eurobert.prepare_weights, eurobert.eurobert_encode_packed),
                 padded=lambda: step_ours(plm, data, eurobert.prepare_weights, eurobert.eurobert_encode),
                 hf=lambda: step_hf(plm, data))
    grads = {}
    for k, fn in paths.items():                                  # first warm-up round; the three gradients agree to bf16 accuracy
        fn()
        grads[k] = plm.layers[0].mlp.down_proj.weight.grad.double().clone()
    for fn in paths.values():                                   # second warm-up round
        fn()
    t = {k: [] for k in paths}
    for _ in range(rounds):
        for k, fn in paths.items():
            t[k].append(timed(fn))
    rel = lambda a, b: float((grads[a] - grads[b]).norm() / grads[b].norm())
    return dict(batch=name, sequences=n_seq, tokens=tokens, padded_tokens=int(sum(i.numel() for i, _, _ in data)), micro_batch=batch,
                micro_batches=len(data), rounds=rounds, **{k + "_ms": v for k, v in t.items()},
                **{k + "_median_ms": med(v) for k, v in t.items()}, **{k + "_range_ms": [min(v), max(v)] for k, v in t.items()},
                speedup_packed_vs_hf_median=med(t["hf"]) / med(t["packed"]), speedup_padded_vs_hf_median=med(t["hf"]) / med(t["padded"]),
                grad_rel_diff_layer0_down_proj=dict(packed_vs_hf=rel("packed", "hf"), padded_vs_hf=rel("padded", "hf")),
                packed_kernels=kernel_table(paths["packed"]), hf_kernels=kernel_table(paths["hf"]))


def run_attention(name, n_seq, lo, hi, reps, rounds, dev):
    """The attention of ONE layer over the whole batch as one packed call: native grouped kernels against K / V expanded to HQ heads."""
    from gmlm_amd import ops
    g = torch.Generator().manual_seed(2)
    lens = torch.randint(lo, hi + 1, (n_seq,), generator=g)
    cu = torch.zeros(n_seq + 1, dtype=torch.int32)
    cu[1:] = lens.cumsum(0)
    cu, rows, longest = cu.to(dev), int(lens.sum()), int(lens.max())
    scale, rep = D ** -0.5, HQ // HKV
    nq, nk = HQ * D, HKV * D
    x = torch.randn(rows, HQ + 2 * HKV, D, generator=g).to(dev, torch.bfloat16)
    go = torch.randn(rows, nq, generator=g).to(dev, torch.bfloat16)
    xe = torch.cat([x[:, :HQ], x[:, HQ:HQ + HKV].repeat_interleave(rep, 1), x[:, HQ + HKV:].repeat_interleave(rep, 1)], 1)
    xe = xe.reshape(rows, 3 * nq).contiguous().requires_grad_(True)          # [q | k expanded | v expanded], the BERT layout
    x = x.view(rows, -1)
    groups = ops.pack_sequence_groups(lens.tolist()).to(dev) if longest <= ops.SHORT_GROUP_ROWS else None
    pairs = float((lens.double() ** 2).sum())

    def native():
        """forward + backward through the C entry points (ops._causal_varlen_fwd / _bwd), no autograd bookkeeping in the timing"""
        q, k, v = x[:, :nq], x[:, nq:nq + nk], x[:, nq + nk:]
        out, out_lo, lse = ops._causal_varlen_fwd(q, k, v, cu, n_seq, longest, HQ, HKV, scale, True, D, True)
        dx = torch.empty_like(x)
        ops._causal_varlen_bwd(q, k, v, out, out_lo, go, lse, cu, n_seq, longest, HQ, HKV, scale, dx[:, :nq], dx[:, nq:nq + nk],
                               dx[:, nq + nk:], D, True)
        return out, dx

    def expanded():
        xe.grad = None
        out = ops.attention_qkv(xe, None, HQ, scale, cu_seqlens=cu, max_len=longest, pair_count=pairs, groups=groups)
        out.backward(go)
        return out.detach(), xe.grad

    o_n, g_n = native()
    o_e, g_e = expanded()
    fold = lambda t: t.view(rows, HKV, rep, D).double().sum(2).reshape(rows, nk)     # dK / dV of a KV head = the sum over its group
    g_fold = torch.cat([g_e[:, :nq].double(), fold(g_e[:, nq:2 * nq]), fold(g_e[:, 2 * nq:])], 1)
    same = float((o_e.double() - o_n.double()).norm() / o_n.double().norm())
    same_g = float((g_fold - g_n.double()).norm() / g_n.double().norm())
    many = lambda fn: (lambda: [fn() for _ in range(reps)])
    many(native)(), many(expanded)()
    tn, te = [], []
    for _ in range(rounds):
        tn.append(timed(many(native)) / reps)
        te.append(timed(many(expanded)) / reps)
    return dict(batch=name, sequences=n_seq, rows=rows, longest=longest, hq=HQ, hkv=HKV, calls_per_round=reps, rounds=rounds,
                short_sequence_groups=None if groups is None else int(groups.numel() - 1),
                native_ms=tn, expanded_ms=te, native_median_ms=med(tn), expanded_median_ms=med(te),
                native_range_ms=[min(tn), max(tn)], expanded_range_ms=[min(te), max(te)],
                speedup_native_median=med(te) / med(tn), out_rel_diff=same, grad_rel_diff=same_g,
                native_kernels=kernel_table(native, top=8), expanded_kernels=kernel_table(expanded, top=8))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", type=int, default=26)
    ap.add_argument("--vocab", type=int, default=4096)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--attn-reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("eurobert_probe needs a GPU (a CPU run measures nothing)")
    dev = torch.device("cuda:0")
    from gmlm_amd import eurobert
    plm = build(a.layers, a.vocab, dev)
    eurobert.check_supported(plm)
    res = dict(what="EuroBERT-610m geometry text encoder, bf16 forward + backward: packed and padded kernel paths vs HF bf16 autocast "
                    "(sdpa), alternating rounds in one process; bidirectional grouped-KV attention alone, native kernels vs K / V "
                    "expanded to one KV head per query head on the bidirectional attention family (expansion not charged)",
               geometry_source="as recalled for EuroBERT-610m, not read from a model card",
               device=torch.cuda.get_device_name(0), layers=a.layers, hidden=HIDDEN, hq=HQ, hkv=HKV, head_dim=D, intermediate=INTER,
               vocab=a.vocab, attn_implementation_hf=str(getattr(plm.config, "_attn_implementation", None)),
               kernel_figures_source="torch.profiler device events, one pass per path after the timed rounds",
               encoder=[run_encoder(plm, "short", 1257, 16, 128, a.vocab, 419, a.rounds, dev),
                        run_encoder(plm, "long", 256, 256, 512, a.vocab, 32, a.rounds, dev)],
               attention=[run_attention("short", 1257, 16, 128, a.attn_reps, a.rounds, dev),
                          run_attention("long", 256, 256, 512, a.attn_reps, a.rounds, dev)])
    emit(res, a.out)


if __name__ == "__main__":
    main()
