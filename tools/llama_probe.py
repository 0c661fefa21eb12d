"""Qwen2.5-0.5B-geometry text encoder, forward + backward in bf16: this project's kernel path (gmlm_amd.llama, packed pass, which
is what GraphTextLM runs, and padded pass) against HF's Qwen2Model under bf16 autocast with sdpa attention, on the same device,
alternating; and the causal attention alone at head dim 64 on the native kernels (gmlm_attention_causal_d64_varlen_*) against
the same heads zero-padded to 128 on causal128 (what a caller could do before the d = 64 family existed), alternating.

Workload: 24 layers, hidden 896, 14 query / 2 KV heads x 64, intermediate 4,864, Q/K/V biases, random weights, a cut vocabulary;
  short   1,257 sequences of 16-128 tokens (the headline workload's text batch), micro-batches of 419 sequences;
  long    256 sequences of 256-512 tokens, micro-batches of 32.
Length-sorted micro-batches; HF and the padded pass see each padded to its longest sequence, the packed pass sees [T, .] rows.
Times: host clock around a device synchronise, ``--rounds`` alternating rounds after two warm-up rounds of each path.  The
attention comparison times forward + backward through the C entry points on prebuilt operands, ``--attn-reps`` calls per round; the
copies that would build the zero-padded operands are NOT charged to the padded route.  Kernel tables: torch.profiler device
events of one further pass, after the timed rounds.  Writes one JSON file (``--out``) and prints it.  Needs a GPU.

    python tools/llama_probe.py --out profiles/llama_probe.json
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from qwen3_probe import batches, emit, kernel_table, pack, step_hf, step_ours, step_packed, timed  # noqa: E402  (tools/ is the script dir)

HIDDEN, HQ, HKV, D, INTER = 896, 14, 2, 64, 4864


def build(layers, vocab, dev):
    from transformers import Qwen2Config, Qwen2Model
    cfg = Qwen2Config(vocab_size=vocab, hidden_size=HIDDEN, intermediate_size=INTER, num_hidden_layers=layers, num_attention_heads=HQ,
                      num_key_value_heads=HKV, max_position_embeddings=512, tie_word_embeddings=False,
                      rope_parameters={"rope_type": "default", "rope_theta": 1e6})
    cfg._attn_implementation = "sdpa"
    torch.manual_seed(0)
    with torch.device(dev):
        plm = Qwen2Model(cfg)
    return plm.train()


def med(v):
    return sorted(v)[len(v) // 2]


def run_encoder(plm, name, n_seq, lo, hi, vocab, batch, rounds, dev):
    from gmlm_amd import llama
    data, tokens = batches(n_seq, lo, hi, vocab, batch, dev)
    pdata = pack(data)
    paths = dict(packed=lambda: step_packed(plm, pdata, llama.prepare_weights, llama.llama_encode_packed),
                 padded=lambda: step_ours(plm, data, llama.prepare_weights, llama.llama_encode),
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
    """The attention of ONE layer over the whole batch as one packed call: native d = 64 against heads zero-padded to 128."""
    from gmlm_amd import ops
    g = torch.Generator().manual_seed(2)
    lens = torch.randint(lo, hi + 1, (n_seq,), generator=g)
    cu = torch.zeros(n_seq + 1, dtype=torch.int32)
    cu[1:] = lens.cumsum(0)
    cu, rows, longest = cu.to(dev), int(lens.sum()), int(lens.max())
    scale = D ** -0.5
    x64 = torch.randn(rows, HQ + 2 * HKV, D, generator=g).to(dev, torch.bfloat16)
    x128 = torch.zeros(rows, HQ + 2 * HKV, 128, dtype=torch.bfloat16, device=dev)
    x128[..., :D] = x64
    go64 = torch.randn(rows, HQ, D, generator=g).to(dev, torch.bfloat16)
    go128 = torch.zeros(rows, HQ, 128, dtype=torch.bfloat16, device=dev)
    go128[..., :D] = go64

    def call(x, go, d):
        """forward + backward through the C entry points (ops._causal_varlen_fwd / _bwd), no autograd bookkeeping in the timing"""
        x, go = x.view(rows, -1), go.view(rows, -1)
        nq, nk = HQ * d, HKV * d
        q, k, v = x[:, :nq], x[:, nq:nq + nk], x[:, nq + nk:]
        out, out_lo, lse = ops._causal_varlen_fwd(q, k, v, cu, n_seq, longest, HQ, HKV, scale, True, d)
        dx = torch.empty_like(x)
        ops._causal_varlen_bwd(q, k, v, out, out_lo, go, lse, cu, n_seq, longest, HQ, HKV, scale, dx[:, :nq], dx[:, nq:nq + nk],
                               dx[:, nq + nk:], d)
        return out, dx

    native, padded = lambda: call(x64, go64, 64), lambda: call(x128, go128, 128)
    o64, g64 = native()
    o128, g128 = padded()
    same = float((o128.view(rows, HQ, 128)[..., :D].double() - o64.view(rows, HQ, D).double()).norm() / o64.double().norm())
    same_g = float((g128.view(rows, -1, 128)[..., :D].double() - g64.view(rows, -1, D).double()).norm() / g64.double().norm())
    many = lambda fn: (lambda: [fn() for _ in range(reps)])
    many(native)(), many(padded)()
    t64, t128 = [], []
    for _ in range(rounds):
        t64.append(timed(many(native)) / reps)
        t128.append(timed(many(padded)) / reps)
    return dict(batch=name, sequences=n_seq, rows=rows, longest=longest, hq=HQ, hkv=HKV, calls_per_round=reps, rounds=rounds,
                native_d64_ms=t64, padded_to_128_ms=t128, native_d64_median_ms=med(t64), padded_to_128_median_ms=med(t128),
                native_d64_range_ms=[min(t64), max(t64)], padded_to_128_range_ms=[min(t128), max(t128)],
                speedup_native_median=med(t128) / med(t64), out_rel_diff=same, grad_rel_diff=same_g,
                native_kernels=kernel_table(native, top=8), padded_kernels=kernel_table(padded, top=8))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", type=int, default=24)
    ap.add_argument("--vocab", type=int, default=4096)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--attn-reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("llama_probe needs a GPU (a CPU run measures nothing)")
    dev = torch.device("cuda:0")
    from gmlm_amd import llama
    plm = build(a.layers, a.vocab, dev)
    llama.check_supported(plm)
    res = dict(what="Qwen2.5-0.5B geometry text encoder, bf16 forward + backward: packed and padded kernel paths vs HF bf16 autocast "
                    "(sdpa), alternating rounds in one process; causal attention alone at d = 64, native kernels vs heads zero-padded "
                    "to 128 on causal128",
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
