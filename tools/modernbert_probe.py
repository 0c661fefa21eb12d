"""ModernBERT-base-geometry text encoder, forward + backward in bf16: this project's kernel path (gmlm_amd.modernbert, the
packed pass GraphTextLM runs) against HF's ModernBertModel under bf16 autocast with sdpa attention, on the same device, in the
same process, in alternating rounds.  The parent of this encoder path refused the model, so HF's module is what a user had.

Workload: 22 layers, hidden 768, 12 heads x 64, intermediate 1,152, local_attention 128 (|i - j| <= 64 in two of every three
layers), random weights, a cut vocabulary; two text batches:
  short   1,257 sequences of 16-128 tokens (the headline workload's text batch);
  long    256 sequences of 256-512 tokens (the reference's plm_max_length; the window cuts most of every score matrix).
Length-sorted micro-batches; HF sees each padded to its longest sequence with an attention mask, this project the same
sequences packed.  Both compute the same loss: the mean-pooled rows against a fixed random direction (their plain sum is
identically 0 behind a LayerNorm without bias, and so would every gradient be).
Times: host clock around a device synchronise, ``--rounds`` alternating rounds after two warm-up rounds of each path.  The
per-kernel figures are torch.profiler's device-kernel events of one further pass of this project's path, taken after the timed
rounds (the profiler slows the host, so it never overlaps a timed round), next to the algorithmic bytes (row kernels) or flops
(band-limited attention: 4 / 10 flops per visible (query, key) pair and head-dim element, forward / backward) of that pass.
Writes one JSON file (``--out``) and prints it.  Needs a GPU: there is no CPU fallback.

    python tools/modernbert_probe.py --out profiles/modernbert_probe.json
"""
import argparse
import json
import math
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HIDDEN, HEADS, INTER, WINDOW = 768, 12, 1152, 64
_DIRECTION = {}


def direction(dev):
    if dev not in _DIRECTION:
        _DIRECTION[dev] = torch.randn(HIDDEN, generator=torch.Generator().manual_seed(7)).to(dev)
    return _DIRECTION[dev]


def build(layers, vocab, dev):
    from transformers import ModernBertConfig, ModernBertModel
    cfg = ModernBertConfig(vocab_size=vocab, hidden_size=HIDDEN, intermediate_size=INTER, num_hidden_layers=layers,
                           num_attention_heads=HEADS, max_position_embeddings=8192, local_attention=2 * WINDOW,
                           global_attn_every_n_layers=3, pad_token_id=0, bos_token_id=1, eos_token_id=2, cls_token_id=1, sep_token_id=2)
    cfg._attn_implementation = "sdpa"
    torch.manual_seed(0)
    with torch.device(dev):
        plm = ModernBertModel(cfg)
    return plm.train()


def batches(n_seq, lo, hi, vocab, batch, dev, seed):
    """[(padded ids, attention mask, lens, packed tok, pos, cu_seqlens, longest, sequence of row)] and the host lengths."""
    g = torch.Generator().manual_seed(seed)
    lens = torch.randint(lo, hi + 1, (n_seq,), generator=g).sort(descending=True).values
    out = []
    for s in range(0, n_seq, batch):
        ln = lens[s:s + batch]
        width = int(ln.max())
        am = (torch.arange(width)[None, :] < ln[:, None])
        ids = (torch.randint(3, vocab, (ln.numel(), width), generator=g) * am).to(dev)
        am = am.to(dev)
        pos = torch.arange(width, device=dev).expand(ln.numel(), width)[am]
        seq = torch.arange(ln.numel(), device=dev)[:, None].expand(ln.numel(), width)[am]
        cu = torch.zeros(ln.numel() + 1, dtype=torch.int32)
        cu[1:] = ln.cumsum(0)
        out.append((ids, am.long(), ln.to(dev, torch.int32), ids[am], pos, cu.to(dev), width, seq))
    return out, lens.tolist()


def step_ours(plm, data):
    from gmlm_amd import modernbert
    plm.zero_grad(set_to_none=True)
    weights = modernbert.prepare_weights(plm, torch.bfloat16)
    for _, _, lens, tok, pos, cu, width, seq in data:
        hs = modernbert.modernbert_encode_packed(plm, tok, pos, cu, width, torch.bfloat16, True, False, weights)
        pooled = torch.zeros(lens.numel(), hs.shape[1], dtype=hs.dtype, device=hs.device).index_add_(0, seq, hs)
        (pooled.float() / lens[:, None].float() * direction(hs.device)).sum().backward()


def step_hf(plm, data):
    plm.zero_grad(set_to_none=True)
    for ids, am, lens, *_ in data:
        with torch.autocast("cuda", dtype=torch.bfloat16):
            hs = plm(input_ids=ids, attention_mask=am).last_hidden_state
        m = am.unsqueeze(-1).to(hs.dtype)
        ((hs * m).sum(1).float() / lens[:, None].float() * direction(hs.device)).sum().backward()


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def kernel_events(fn):
    """{device kernel name: [launches, microseconds]} of one pass."""
    from torch.autograd import DeviceType
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    acc = {}
    for e in prof.events():
        if e.device_type == DeviceType.CUDA:
            d = acc.setdefault(e.name, [0, 0.0])
            d[0] += 1
            d[1] += e.device_time_total if hasattr(e, "device_time_total") else e.cuda_time_total
    return acc


def band_pairs(lens, window):
    """Visible (query, key) pairs of the band |i - j| <= window over sequences of ``lens`` tokens."""
    total = 0
    for n in lens:
        w = min(window, n - 1)
        total += n * (2 * w + 1) - w * (w + 1)
    return total


def algorithmic(layers, lens, widths):
    """Algorithmic work of one forward + backward pass per kernel group: ('bytes' | 'flops', amount).  ``widths``: the longest
    sequence of every micro-batch with that micro-batch's lengths (a sliding layer runs the band-limited kernels only where
    the window cuts: longest > window + 1)."""
    t, e = sum(lens), 2
    sliding = sum(1 for i in range(layers) if i % 3)
    calls_b = 2 * layers                                           # (layers - 1) attention norms + layers MLP norms + the final norm
    cut_pairs = sum(band_pairs(ln, WINDOW) for width, ln in widths if width > WINDOW + 1)
    return {
        "mbert::add_ln_fwd_kernel": ("bytes", t * HIDDEN * e * (4 * calls_b + 2)),      # a, b, s, y; the embedding norm: x, y
        "mbert::add_ln_bwd_kernel": ("bytes", t * HIDDEN * e * (4 * calls_b + 3)),      # dy, dres, s, ds
        "mbert::LnDwFn": ("bytes", t * HIDDEN * e * 2 * (calls_b + 1)),                 # dgamma: dy, s once more
        "mbert::rope64_kernel<unsigned short, false>": ("bytes", layers * t * 2 * HIDDEN * e * 2),   # q | k columns read and written
        "mbert::rope64_kernel<unsigned short, true>": ("bytes", layers * t * 2 * HIDDEN * e * 2),
        "mbert::geglu_fwd_kernel": ("bytes", layers * t * 3 * INTER * e),
        "mbert::geglu_bwd_kernel": ("bytes", layers * t * 5 * INTER * e),
        "mbert::window_fwd_kernel": ("flops", 4.0 * 64 * HEADS * sliding * cut_pairs),
        "mbert::window_bwd (delta + dq + dkv)": ("flops", 10.0 * 64 * HEADS * sliding * cut_pairs),
    }


def per_kernel(events, work):
    rows = {}
    for group, (unit, amount) in work.items():
        keys = ("mbert::window_delta_kernel", "mbert::window_dq_kernel", "mbert::window_dkv_kernel") if "window_bwd" in group else (group,)
        hit = [(k, v) for k, v in events.items() if any(key in k for key in keys)]
        us = sum(v[1] for _, v in hit)
        rows[group] = dict(launches=sum(v[0] for _, v in hit), device_ms=us / 1e3, **{unit: amount},
                           **({"GB_per_s": amount / us / 1e3} if unit == "bytes" and us else {}),
                           **({"TFLOP_per_s": amount / us / 1e6} if unit == "flops" and us else {}))
    return rows


def run(plm, name, n_seq, lo, hi, vocab, batch, rounds, dev, seed):
    data, lens = batches(n_seq, lo, hi, vocab, batch, dev, seed)
    ours, hf = (lambda: step_ours(plm, data)), (lambda: step_hf(plm, data))
    ours()
    g_ours = plm.layers[1].mlp.Wo.weight.grad.double().clone()
    hf()
    g_hf = plm.layers[1].mlp.Wo.weight.grad.double()
    agree = float((g_ours - g_hf).norm() / g_hf.norm())
    ours()                                                      # second warm-up round of each path
    hf()
    t_ours, t_hf = [], []
    for _ in range(rounds):
        t_ours.append(timed(ours))
        t_hf.append(timed(hf))
    med = lambda v: sorted(v)[len(v) // 2]
    events = kernel_events(ours)
    total_us = sum(v[1] for v in events.values())
    widths = [(d[6], d[2].tolist()) for d in data]
    top = sorted(events.items(), key=lambda kv: -kv[1][1])[:12]
    return dict(batch=name, sequences=n_seq, min_len=lo, max_len=hi, tokens=sum(lens), padded_tokens=int(sum(d[0].numel() for d in data)),
                micro_batch=batch, micro_batches=len(data), rounds=rounds, ours_ms=t_ours, hf_ms=t_hf, ours_median_ms=med(t_ours),
                hf_median_ms=med(t_hf), ours_range_ms=[min(t_ours), max(t_ours)], hf_range_ms=[min(t_hf), max(t_hf)],
                speedup_median=med(t_hf) / med(t_ours),
                grad_rel_diff_layer1_mlp_Wo=agree if math.isfinite(agree) else None,
                ours_total_kernel_ms=total_us / 1e3, new_kernels=per_kernel(events, algorithmic(len(plm.layers), lens, widths)),
                ours_top_kernels=[dict(name=k if len(k) <= 90 else k[:87] + "...", launches=v[0], ms=v[1] / 1e3, share=v[1] / max(total_us, 1e-9))
                                  for k, v in top])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", type=int, default=22)
    ap.add_argument("--vocab", type=int, default=4096)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("modernbert_probe needs a GPU (a CPU run measures nothing)")
    dev = torch.device("cuda:0")
    from gmlm_amd import modernbert
    plm = build(a.layers, a.vocab, dev)
    modernbert.check_supported(plm)
    res = dict(what="ModernBERT-base geometry text encoder, bf16 forward + backward, packed kernel path vs HF bf16 autocast (sdpa), "
                    "alternating rounds in one process",
               device=torch.cuda.get_device_name(0), layers=a.layers, hidden=HIDDEN, heads=HEADS, intermediate=INTER, window=WINDOW,
               attn_implementation_hf=str(getattr(plm.config, "_attn_implementation", None)),
               kernel_figures_source="torch.profiler device events, one pass of the kernel path after the timed rounds",
               batches=[run(plm, "short", 1257, 16, 128, a.vocab, 419, a.rounds, dev, 1),
                        run(plm, "long", 256, 256, 512, a.vocab, 32, a.rounds, dev, 2)])
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
