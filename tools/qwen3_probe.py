"""Qwen3-0.6B-geometry text encoder, forward + backward in bf16: this project's kernel path (gmlm_amd.qwen3) against HF's
Qwen3Model under bf16 autocast with its default attention, on the same device, alternating.

Workload: 28 layers, hidden 1024, 16 query / 8 KV heads x 128, intermediate 3072, random weights, a cut vocabulary; 1,257
sequences of 16-128 tokens (the headline workload's text batch), length-sorted micro-batches of ``--batch`` sequences padded
to the longest of each.  Both paths see the same micro-batches and the same loss (sum of the mean-pooled rows).
Times: host clock around a device synchronise, ``--rounds`` alternating rounds after two warm-up rounds of each path (every
micro-batch shape is warm).  The per-kernel breakdown is torch.profiler's device-kernel table of one further pass per path,
taken after the timed rounds in the same process (the profiler slows the host, so it never overlaps a timed round); it is
not a rocprofv3 trace.
Writes one JSON file (``--out``) and prints it.  Needs a GPU: there is no CPU fallback.

    python tools/qwen3_probe.py --out profiles/qwen3_probe.json
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def build(layers, vocab, dev):
    from transformers import Qwen3Config, Qwen3Model
    kw = dict(vocab_size=vocab, hidden_size=1024, intermediate_size=3072, num_hidden_layers=layers, num_attention_heads=16,
              num_key_value_heads=8, head_dim=128, max_position_embeddings=512, tie_word_embeddings=False)
    if hasattr(Qwen3Config(), "rope_parameters"):
        kw["rope_parameters"] = {"rope_type": "default", "rope_theta": 1e6}
    else:
        kw["rope_theta"] = 1e6
    torch.manual_seed(0)
    with torch.device(dev):
        plm = Qwen3Model(Qwen3Config(**kw))
    return plm.train()


def batches(n_seq, lo, hi, vocab, batch, dev):
    g = torch.Generator().manual_seed(1)
    lens = torch.randint(lo, hi + 1, (n_seq,), generator=g).sort(descending=True).values
    out = []
    for s in range(0, n_seq, batch):
        ln = lens[s:s + batch]
        width = int(ln.max())
        am = (torch.arange(width)[None, :] < ln[:, None]).long()
        ids = torch.randint(1, vocab, (ln.numel(), width), generator=g) * am
        out.append((ids.to(dev), am.to(dev), ln.to(dev, torch.int32)))
    return out, int(lens.sum())


def step_ours(plm, data, weights_fn, encode):
    plm.zero_grad(set_to_none=True)
    weights = weights_fn(plm, torch.bfloat16)
    for ids, am, lens in data:
        hs = encode(plm, ids, lens, torch.bfloat16, True, False, weights)
        m = am.unsqueeze(-1).to(hs.dtype)
        ((hs * m).sum(1).float() / lens[:, None].float()).sum().backward()


def step_hf(plm, data):
    plm.zero_grad(set_to_none=True)
    for ids, am, lens in data:
        with torch.autocast("cuda", dtype=torch.bfloat16):
            hs = plm(input_ids=ids, attention_mask=am).last_hidden_state
        m = am.unsqueeze(-1).to(hs.dtype)
        ((hs * m).sum(1).float() / lens[:, None].float()).sum().backward()


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def kernel_table(fn, top=14):
    from torch.autograd import DeviceType
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    acc = {}
    for e in prof.events():
        if e.device_type == DeviceType.CUDA:
            name = e.name if len(e.name) <= 90 else e.name[:87] + "..."
            d = acc.setdefault(name, [0, 0.0])
            d[0] += 1
            d[1] += e.device_time_total if hasattr(e, "device_time_total") else e.cuda_time_total
    total = sum(v[1] for v in acc.values())
    rows = sorted(acc.items(), key=lambda kv: -kv[1][1])[:top]
    return dict(total_kernel_ms=total / 1e3, kernels=[dict(name=k, launches=v[0], ms=v[1] / 1e3, share=v[1] / max(total, 1e-9))
                                                       for k, v in rows])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", type=int, default=28)
    ap.add_argument("--vocab", type=int, default=4096)
    ap.add_argument("--sequences", type=int, default=1257)
    ap.add_argument("--min-len", type=int, default=16)
    ap.add_argument("--max-len", type=int, default=128)
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("qwen3_probe needs a GPU (a CPU run measures nothing)")
    dev = torch.device("cuda:0")
    from gmlm_amd import qwen3
    plm = build(a.layers, a.vocab, dev)
    qwen3.check_supported(plm)
    data, tokens = batches(a.sequences, a.min_len, a.max_len, a.vocab, a.batch, dev)
    ours = lambda: step_ours(plm, data, qwen3.prepare_weights, qwen3.qwen3_encode)
    hf = lambda: step_hf(plm, data)
    # same weights, same batches: the two losses' gradients agree to bf16 accuracy (printed, not a test: tests/test_gpu_qwen3.py)
    ours()
    g_ours = plm.layers[0].mlp.down_proj.weight.grad.double().clone()
    hf()
    g_hf = plm.layers[0].mlp.down_proj.weight.grad.double()
    agree = float((g_ours - g_hf).norm() / g_hf.norm())
    ours()                                                      # second warm-up round of each path
    hf()
    t_ours, t_hf = [], []
    for _ in range(a.rounds):
        t_ours.append(timed(ours))
        t_hf.append(timed(hf))
    med = lambda v: sorted(v)[len(v) // 2]
    res = dict(what="Qwen3-0.6B geometry text encoder, bf16 forward + backward, kernel path vs HF bf16 autocast (default attention), alternating",
               device=torch.cuda.get_device_name(0), layers=a.layers, sequences=a.sequences, tokens=tokens,
               padded_tokens=int(sum(i.numel() for i, _, _ in data)), micro_batch=a.batch, rounds=a.rounds,
               attn_implementation_hf=str(getattr(plm.config, "_attn_implementation", None)),
               ours_ms=t_ours, hf_ms=t_hf, ours_median_ms=med(t_ours), hf_median_ms=med(t_hf),
               speedup_median=med(t_hf) / med(t_ours), grad_rel_diff_layer0_down_proj=agree,
               kernel_table_source="torch.profiler device events, one pass per path after the timed rounds",
               ours_kernels=kernel_table(ours), hf_kernels=kernel_table(hf))
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
