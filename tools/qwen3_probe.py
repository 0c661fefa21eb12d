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

``--packed``: this project's two passes against each other instead of against HF, alternating in the same way: the padded
pass (``qwen3_encode``, every micro-batch padded to its longest sequence) and the packed / varlen pass
(``qwen3_encode_packed``, the same micro-batches as [T, .] rows with no padded token).  The result also says whether the
packed pass reached the split-K weight-gradient kernel (``wgrad_bf16_kernel``, T >= 16,384 rows in one micro-batch).

    python tools/qwen3_probe.py --packed --batch 1257 --out profiles/qwen3_packed_probe.json
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


def pack(data):
    """The padded micro-batches as packed ones: (token ids [T], positions [T], cu_seqlens [S + 1], longest, sequence of row, lens)."""
    out = []
    for ids, am, lens in data:
        keep = am.bool()
        s, width = ids.shape
        pos = torch.arange(width, device=ids.device).expand(s, width)[keep]
        seq = torch.arange(s, device=ids.device)[:, None].expand(s, width)[keep]
        cu = torch.zeros(s + 1, dtype=torch.int32, device=ids.device)
        cu[1:] = lens.cumsum(0)
        out.append((ids[keep], pos, cu, width, seq, lens))
    return out


def step_packed(plm, data, weights_fn, encode):
    plm.zero_grad(set_to_none=True)
    weights = weights_fn(plm, torch.bfloat16)
    for tok, pos, cu, width, seq, lens in data:
        hs = encode(plm, tok, pos, cu, width, torch.bfloat16, True, False, weights)
        pooled = torch.zeros(lens.numel(), hs.shape[1], dtype=hs.dtype, device=hs.device).index_add_(0, seq, hs)
        (pooled.float() / lens[:, None].float()).sum().backward()


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
    ap.add_argument("--packed", action="store_true", help="padded pass against packed pass of this project (no HF run)")
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
    if a.packed:
        return packed_main(a, plm, data, tokens, ours)
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
    emit(res, a.out)


def packed_main(a, plm, data, tokens, padded):
    from gmlm_amd import qwen3
    pdata = pack(data)
    packed = lambda: step_packed(plm, pdata, qwen3.prepare_weights, qwen3.qwen3_encode_packed)
    padded()
    g_pad = plm.layers[0].mlp.down_proj.weight.grad.double().clone()
    packed()
    g_pack = plm.layers[0].mlp.down_proj.weight.grad.double()
    agree = float((g_pack - g_pad).norm() / g_pad.norm())
    padded()                                                    # second warm-up round of each path
    packed()
    t_pad, t_pack = [], []
    for _ in range(a.rounds):
        t_pad.append(timed(padded))
        t_pack.append(timed(packed))
    med = lambda v: sorted(v)[len(v) // 2]
    padded_tokens = int(sum(i.numel() for i, _, _ in data))
    k_pad, k_pack = kernel_table(padded, top=10 ** 6), kernel_table(packed, top=10 ** 6)
    wgrad = lambda tab: any("wgrad_bf16_kernel" in k["name"] for k in tab["kernels"])
    res = dict(what="Qwen3-0.6B geometry text encoder, bf16 forward + backward, padded pass vs packed (varlen) pass of this project, alternating",
               device=torch.cuda.get_device_name(0), layers=a.layers, sequences=a.sequences, tokens=tokens,
               padded_tokens=padded_tokens, real_to_padded_rows=tokens / padded_tokens, micro_batch=a.batch,
               micro_batches=len(data), largest_packed_micro_batch_rows=max(int(t[0].numel()) for t in pdata), rounds=a.rounds,
               padded_ms=t_pad, packed_ms=t_pack, padded_median_ms=med(t_pad), packed_median_ms=med(t_pack),
               padded_range_ms=[min(t_pad), max(t_pad)], packed_range_ms=[min(t_pack), max(t_pack)],
               speedup_median=med(t_pad) / med(t_pack), grad_rel_diff_layer0_down_proj=agree,
               native_splitk_wgrad_reached=dict(padded=wgrad(k_pad), packed=wgrad(k_pack)),
               kernel_table_source="torch.profiler device events, one pass per path after the timed rounds",
               padded_kernels=dict(k_pad, kernels=k_pad["kernels"][:14]), packed_kernels=dict(k_pack, kernels=k_pack["kernels"][:14]))
    emit(res, a.out)


def emit(res, out):
    text = json.dumps(res, indent=1)
    print(text)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
