"""EmbeddingGemma-geometry text encoder on texts PAST the sliding window, forward + backward in bf16:
  (a) the attention of one layer alone over the whole batch, the band-limited kernels (gqab::, window 257, and window >= the
      longest sequence) against the un-banded ones (gqaw::) on the same packed rows.  The un-banded kernels compute another
      function: they are the cost yardstick only;
  (b) the packed encoder pass with ``band=True`` (gmlm_amd.gemma3) against HF's Gemma3TextModel under bf16 autocast with sdpa
      attention, on the same device, alternating.

Workload: 24 layers, hidden 768, 3 query / 1 KV heads x 256, intermediate 1,152, bidirectional, sliding_window 512 (which the
config turns into 257; the geometry of tools/gemma3_probe.py), random weights, a cut vocabulary; 64 sequences of 1,024-2,048
tokens, micro-batches of 8.  Times: host clock around a device synchronise, ``--rounds`` alternating rounds after two warm-up
rounds of each path, medians and ranges.  Writes one JSON file (``--out``) and prints it.  Needs a GPU.

    python tools/gemma3_band_probe.py --out profiles/gemma3_band_probe.json
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gemma3_probe import D, HKV, HQ, build, med  # noqa: E402  (tools/ is the script dir)
from qwen3_probe import batches, emit, kernel_table, pack, step_hf, step_packed, timed  # noqa: E402


def run_attention(n_seq, lo, hi, window, reps, rounds, dev):
    """One layer's attention over the whole batch through the operators on slices of the fused rows: gqab:: at ``window``, gqab::
    at window = the longest sequence (the band covers everything: the same tiles as gqaw::) and gqaw::, alternating."""
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

    def step(w):
        x.grad = None
        q, k, v = x[:, :nq], x[:, nq:nq + nk], x[:, nq + nk:]
        if w:
            out = ops.gqa_d256_band_attention_varlen(q, k, v, cu, longest, HQ, HKV, scale, False, w)
        else:
            out = ops.gqa_d256_attention_varlen(q, k, v, cu, longest, HQ, HKV, scale, False)
        out.backward(go)
        return out.detach(), x.grad

    paths = dict(band=lambda: step(window), band_whole=lambda: step(longest), plain=lambda: step(0))
    whole, plain = paths["band_whole"](), paths["plain"]()
    same = all(torch.equal(a, b) for a, b in zip(whole, plain))      # window >= l: the bytes of the un-banded kernels
    many = lambda fn: (lambda: [fn() for _ in range(reps)])
    for fn in paths.values():
        many(fn)()
    t = {k: [] for k in paths}
    for _ in range(rounds):
        for k, fn in paths.items():
            t[k].append(timed(many(fn)) / reps)
    tiles = lambda w: float(sum(min(-(-int(n) // 32), (2 * (w - 1) + 31) // 32 + 1) * -(-int(n) // 32) for n in lens))
    return dict(sequences=n_seq, rows=rows, longest=longest, shortest=int(lens.min()), hq=HQ, hkv=HKV, window=window, calls_per_round=reps,
                rounds=rounds, **{k + "_ms": v for k, v in t.items()}, **{k + "_median_ms": med(v) for k, v in t.items()},
                **{k + "_range_ms": [min(v), max(v)] for k, v in t.items()},
                speedup_band_vs_plain_median=med(t["plain"]) / med(t["band"]),
                band_whole_vs_plain_median=med(t["band_whole"]) / med(t["plain"]),
                key_tiles_upper_bound_band_over_plain=tiles(window) / tiles(1 << 29), window_past_length_bit_identical=bool(same),
                band_kernels=kernel_table(paths["band"], top=6), plain_kernels=kernel_table(paths["plain"], top=6))


def run_encoder(plm, n_seq, lo, hi, vocab, batch, rounds, dev):
    from gmlm_amd import gemma3
    data, tokens = batches(n_seq, lo, hi, vocab, batch, dev)
    pdata = pack(data)
    encode = lambda *a: gemma3.gemma3_encode_packed(*a, band=True)
    paths = dict(packed_band=lambda: step_packed(plm, pdata, gemma3.prepare_weights, encode), hf=lambda: step_hf(plm, data))
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
                micro_batches=len(data), rounds=rounds, sliding_window=int(plm.config.sliding_window),
                **{k + "_ms": v for k, v in t.items()}, **{k + "_median_ms": med(v) for k, v in t.items()},
                **{k + "_range_ms": [min(v), max(v)] for k, v in t.items()},
                speedup_packed_band_vs_hf_median=med(t["hf"]) / med(t["packed_band"]),
                grad_rel_diff_layer0_down_proj=float((grads["packed_band"] - grads["hf"]).norm() / grads["hf"].norm()),
                packed_band_kernels=kernel_table(paths["packed_band"]), hf_kernels=kernel_table(paths["hf"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", type=int, default=24)
    ap.add_argument("--vocab", type=int, default=4096)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--attn-reps", type=int, default=3)
    ap.add_argument("--sequences", type=int, default=64)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("gemma3_band_probe needs a GPU (a CPU run measures nothing)")
    dev = torch.device("cuda:0")
    from gmlm_amd import gemma3
    plm = build(a.layers, a.vocab, dev)
    gemma3.check_supported(plm)
    window = int(plm.config.sliding_window)
    res = dict(what="EmbeddingGemma geometry, texts of 1,024-2,048 tokens, bf16 forward + backward: (a) one layer's attention, gqab:: at "
                    "the window and at window >= l against gqaw:: (another function: the cost yardstick); (b) the packed encoder pass with "
                    "band=True against HF bf16 autocast (sdpa); alternating rounds in one process, medians",
               device=torch.cuda.get_device_name(0), layers=a.layers, hq=HQ, hkv=HKV, head_dim=D, vocab=a.vocab, window=window,
               kernel_figures_source="torch.profiler device events, one pass per path after the timed rounds",
               attention=run_attention(a.sequences, 1024, 2048, window, a.attn_reps, a.rounds, dev),
               encoder=run_encoder(plm, a.sequences, 1024, 2048, a.vocab, a.batch, a.rounds, dev))
    emit(res, a.out)


if __name__ == "__main__":
    main()
