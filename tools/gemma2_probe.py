"""gemma-2-2b-geometry text encoder, forward + backward in bf16.  Nothing is fixed in advance; the parent of this encoder refuses
the model, so HF stands in for it:
  (a) the attention of one layer alone over the whole batch, the soft-capped kernels (gqac::, cap 50) against the uncapped ones
      (gqaw::) on the same packed rows: what the cap costs.  The uncapped kernels compute another function: the cost yardstick;
  (b) the same with a window (``--window``, default 256): gqac:: with the band against gqab::;
  (c) the packed encoder pass (gmlm_amd.gemma2) against HF's Gemma2Model under bf16 autocast with EAGER attention, the HF path
      that applies the cap (its sdpa path cannot express it), on the same device, alternating.

Workload: the geometry of google/gemma-2-2b STATED FROM MEMORY, not read from a config: hidden 2,304, 8 query / 4 KV heads x
256, intermediate 9,216, query_pre_attn_scalar 256, attn_logit_softcapping 50, sliding_window 4,096, layer types alternating sliding / full; ``--layers`` of its 26 layers (default 8: the per-layer cost is
what is compared), random weights, a cut vocabulary; 64 sequences of 512-1,024 tokens, micro-batches of 8.  No sequence reaches
the model's window, so (c) runs no band kernel; (b) covers them.  Times: host clock around a device synchronise, ``--rounds``
alternating rounds after two warm-up rounds of each path, medians and ranges.  Writes one JSON file (``--out``) and prints it.
Needs a GPU.

    python tools/gemma2_probe.py --out profiles/gemma2_probe.json
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gemma3_probe import med  # noqa: E402  (tools/ is the script dir)
from qwen3_probe import batches, emit, kernel_table, pack, step_hf, step_packed, timed  # noqa: E402

HQ, HKV, D, CAP = 8, 4, 256, 50.0


def build(layers, vocab, dev):
    from transformers import Gemma2Config, Gemma2Model
    torch.manual_seed(0)
    cfg = Gemma2Config(vocab_size=vocab, hidden_size=2304, intermediate_size=9216, num_hidden_layers=layers, num_attention_heads=HQ,
                       num_key_value_heads=HKV, head_dim=D, query_pre_attn_scalar=256, attn_logit_softcapping=CAP, sliding_window=4096,
                       max_position_embeddings=8192, pad_token_id=0, attention_dropout=0.0)
    cfg._attn_implementation = "eager"
    return Gemma2Model(cfg).to(dev).train()


def run_attention(n_seq, lo, hi, window, reps, rounds, dev):
    """One layer's attention over the whole batch through the operators on slices of the fused rows, causal: gqac:: against
    gqaw:: (no band) and, at ``window``, against gqab::, alternating."""
    from gmlm_amd import ops
    g = torch.Generator().manual_seed(2)
    lens = torch.randint(lo, hi + 1, (n_seq,), generator=g)
    cu = torch.zeros(n_seq + 1, dtype=torch.int32)
    cu[1:] = lens.cumsum(0)
    cu, rows, longest = cu.to(dev), int(lens.sum()), int(lens.max())
    scale = D ** -0.5
    nq, nk = HQ * D, HKV * D
    x = torch.randn(rows, (HQ + 2 * HKV) * D, generator=g).to(dev, torch.bfloat16).requires_grad_(True)
    go = torch.randn(rows, nq, generator=g).to(dev, torch.bfloat16)

    def step(cap, w):
        x.grad = None
        q, k, v = x[:, :nq], x[:, nq:nq + nk], x[:, nq + nk:]
        if cap:
            out = ops.gqa_d256_softcap_attention_varlen(q, k, v, cu, longest, HQ, HKV, scale, True, cap, w)
        elif w:
            out = ops.gqa_d256_band_attention_varlen(q, k, v, cu, longest, HQ, HKV, scale, True, w)
        else:
            out = ops.gqa_d256_attention_varlen(q, k, v, cu, longest, HQ, HKV, scale, True)
        out.backward(go)
        return out.detach(), x.grad

    paths = dict(cap=lambda: step(CAP, 0), plain=lambda: step(None, 0), cap_band=lambda: step(CAP, window), band=lambda: step(None, window))
    many = lambda fn: (lambda: [fn() for _ in range(reps)])
    for fn in paths.values():
        many(fn)()
    t = {k: [] for k in paths}
    for _ in range(rounds):
        for k, fn in paths.items():
            t[k].append(timed(many(fn)) / reps)
    return dict(sequences=n_seq, rows=rows, longest=longest, shortest=int(lens.min()), hq=HQ, hkv=HKV, softcap=CAP, window=window,
                causal=True, calls_per_round=reps, rounds=rounds, **{k + "_ms": v for k, v in t.items()},
                **{k + "_median_ms": med(v) for k, v in t.items()}, **{k + "_range_ms": [min(v), max(v)] for k, v in t.items()},
                cap_over_plain_median=med(t["cap"]) / med(t["plain"]), cap_band_over_band_median=med(t["cap_band"]) / med(t["band"]),
                cap_kernels=kernel_table(paths["cap"], top=6), plain_kernels=kernel_table(paths["plain"], top=6),
                cap_band_kernels=kernel_table(paths["cap_band"], top=6), band_kernels=kernel_table(paths["band"], top=6))


def run_encoder(plm, n_seq, lo, hi, vocab, batch, rounds, dev):
    from gmlm_amd import gemma2
    data, tokens = batches(n_seq, lo, hi, vocab, batch, dev)
    pdata = pack(data)
    paths = dict(packed=lambda: step_packed(plm, pdata, gemma2.prepare_weights, gemma2.gemma2_encode_packed), hf=lambda: step_hf(plm, data))
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
    return dict(sequences=n_seq, tokens=tokens, padded_tokens=int(sum(i.numel() for i, _, _ in data)), micro_batch=batch,
                micro_batches=len(data), rounds=rounds, sliding_window=int(plm.config.sliding_window), hf_attention="eager",
                **{k + "_ms": v for k, v in t.items()}, **{k + "_median_ms": med(v) for k, v in t.items()},
                **{k + "_range_ms": [min(v), max(v)] for k, v in t.items()},
                speedup_packed_vs_hf_median=med(t["hf"]) / med(t["packed"]),
                grad_rel_diff_layer0_down_proj=float((grads["packed"] - grads["hf"]).norm() / grads["hf"].norm()),
                packed_kernels=kernel_table(paths["packed"]), hf_kernels=kernel_table(paths["hf"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", type=int, default=8)
    ap.add_argument("--vocab", type=int, default=4096)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--attn-reps", type=int, default=3)
    ap.add_argument("--sequences", type=int, default=64)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--window", type=int, default=256)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("gemma2_probe needs a GPU (a CPU run measures nothing)")
    dev = torch.device("cuda:0")
    from gmlm_amd import gemma2
    plm = build(a.layers, a.vocab, dev)
    gemma2.check_supported(plm)
    res = dict(what="gemma-2-2b geometry (stated from memory, not read from a config), texts of 512-1,024 tokens, bf16 forward + backward: "
                    "(a) one layer's causal attention, gqac:: at cap 50 against gqaw:: (another function: the cost yardstick); (b) the same "
                    "with a window, against gqab::; (c) the packed encoder pass against HF Gemma2Model under bf16 autocast with eager "
                    "attention (the HF path that applies the cap); alternating rounds in one process, medians",
               device=torch.cuda.get_device_name(0), layers=a.layers, layers_of_the_model=26, hq=HQ, hkv=HKV, head_dim=D, vocab=a.vocab,
               geometry_source="stated from memory", kernel_figures_source="torch.profiler device events, one pass per path after the timed rounds",
               attention=run_attention(a.sequences, 512, 1024, a.window, a.attn_reps, a.rounds, dev),
               encoder=run_encoder(plm, a.sequences, 512, 1024, a.vocab, a.batch, a.rounds, dev))
    emit(res, a.out)


if __name__ == "__main__":
    main()
