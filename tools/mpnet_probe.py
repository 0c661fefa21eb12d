"""all-mpnet-base-v2-geometry text encoder, forward + backward in bf16, three models in one process in alternating rounds:
  ours   this project's kernel path (gmlm_amd.mpnet, the packed pass GraphTextLM runs);
  hf     HF's MPNetModel under bf16 autocast on the same device (eager attention: MPNet has no sdpa path);
  bert   this tree's BERT path (gmlm_amd.bert, packed) at the same geometry: what the relative-position bias costs.
The parent of this encoder path refused the model, so HF's module is what a user had.

Workload: 12 layers, hidden 768, 12 heads x 64, intermediate 3,072, random weights, a cut vocabulary, dropouts 0; two text batches:
  short   1,257 sequences of 16-128 tokens (the headline workload's text batch);
  long    256 sequences of 256-512 tokens.
Length-sorted micro-batches; HF sees each padded to its longest sequence with an attention mask, the two kernel paths the same
sequences packed.  All compute the same loss: the mean-pooled rows against a fixed random direction.  The BERT path at d = 64,
bf16, sequences <= 128 and >= 512 (sequence, head) pairs runs its LDS-resident short-sequence attention kernels (with
``ops.pack_sequence_groups``, as GraphTextLM does); the MPNet path has no such form, so on the short batch the difference to BERT
is the bias AND the streaming kernels.
Times: host clock around a device synchronise, ``--rounds`` alternating rounds after two warm-up rounds of each path.  The
per-kernel figures are torch.profiler's device-kernel events of one further pass of the MPNet and of the BERT path, taken after
the timed rounds; ``bias_gradient_share_of_difference`` = device time of relb::dbias_kernel + relb::dbias_sum_kernel over the
difference of the two paths' total device-kernel times.
Writes one JSON file (``--out``) and prints it.  Needs a GPU: there is no CPU fallback.

    python tools/mpnet_probe.py --out profiles/mpnet_probe.json
"""
import argparse
import json
import math
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HIDDEN, HEADS, INTER = 768, 12, 3072
_DIRECTION = {}


def direction(dev):
    if dev not in _DIRECTION:
        _DIRECTION[dev] = torch.randn(HIDDEN, generator=torch.Generator().manual_seed(7)).to(dev)
    return _DIRECTION[dev]


def build(layers, vocab, dev):
    from transformers import BertConfig, BertModel, MPNetConfig, MPNetModel
    common = dict(vocab_size=vocab, hidden_size=HIDDEN, intermediate_size=INTER, num_hidden_layers=layers, num_attention_heads=HEADS,
                  hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)
    torch.manual_seed(0)
    with torch.device(dev):
        plm = MPNetModel(MPNetConfig(max_position_embeddings=514, **common), add_pooling_layer=False)
        ref = BertModel(BertConfig(max_position_embeddings=512, **common), add_pooling_layer=False)
    with torch.no_grad():
        plm.encoder.relative_attention_bias.weight.normal_()
    return plm.train(), ref.train()


def batches(n_seq, lo, hi, vocab, batch, dev, seed):
    """[(padded ids, attention mask, lens, packed tok, pos, cu_seqlens, longest, sequence of row, groups)] and the host lengths."""
    from gmlm_amd import ops
    g = torch.Generator().manual_seed(seed)
    lens = torch.randint(lo, hi + 1, (n_seq,), generator=g).sort(descending=True).values
    out = []
    for s in range(0, n_seq, batch):
        ln = lens[s:s + batch]
        width = int(ln.max())
        am = (torch.arange(width)[None, :] < ln[:, None])
        ids = torch.where(am, torch.randint(3, vocab, (ln.numel(), width), generator=g), torch.ones(ln.numel(), width, dtype=torch.long)).to(dev)
        am = am.to(dev)
        pos = torch.arange(width, device=dev).expand(ln.numel(), width)[am]
        seq = torch.arange(ln.numel(), device=dev)[:, None].expand(ln.numel(), width)[am]
        cu = torch.zeros(ln.numel() + 1, dtype=torch.int32)
        cu[1:] = ln.cumsum(0)
        groups = ops.pack_sequence_groups(ln.tolist()).to(dev) if (width <= 128 and ln.numel() * HEADS >= 512) else None
        out.append((ids, am.long(), ln.to(dev, torch.int32), ids[am], pos, cu.to(dev), width, seq, groups))
    return out, lens.tolist()


def _loss(hs, lens, seq):
    pooled = torch.zeros(lens.numel(), hs.shape[1], dtype=hs.dtype, device=hs.device).index_add_(0, seq, hs)
    return (pooled.float() / lens[:, None].float() * direction(hs.device)).sum()


def step_ours(plm, data):
    from gmlm_amd import mpnet
    plm.zero_grad(set_to_none=True)
    weights = mpnet.prepare_weights(plm, torch.bfloat16)
    for _, _, lens, tok, pos, cu, width, seq, _ in data:
        _loss(mpnet.mpnet_encode_packed(plm, tok, pos, cu, width, torch.bfloat16, True, False, weights), lens, seq).backward()


def step_bert(ref, data):
    from gmlm_amd import bert
    ref.zero_grad(set_to_none=True)
    weights = bert.prepare_weights(ref, torch.bfloat16)
    for _, _, lens, tok, pos, cu, width, seq, groups in data:
        pairs = float((lens.double() ** 2).sum())
        _loss(bert.bert_encode_packed(ref, tok, pos, cu, width, torch.bfloat16, True, False, weights, pair_count=pairs, groups=groups),
              lens, seq).backward()


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


def _group(events, *keys):
    hit = [v for k, v in events.items() if any(key in k for key in keys)]
    return dict(launches=sum(v[0] for v in hit), device_ms=sum(v[1] for v in hit) / 1e3)


def run(plm, ref, name, n_seq, lo, hi, vocab, batch, rounds, dev, seed):
    data, lens = batches(n_seq, lo, hi, vocab, batch, dev, seed)
    ours, hf, brt = (lambda: step_ours(plm, data)), (lambda: step_hf(plm, data)), (lambda: step_bert(ref, data))
    name_g = "encoder.layer.1.output.dense.weight"
    ours()
    g_ours = dict(plm.named_parameters())[name_g].grad.double().clone()
    b_ours = plm.encoder.relative_attention_bias.weight.grad.double().clone()
    hf()
    g_hf = dict(plm.named_parameters())[name_g].grad.double()
    b_hf = plm.encoder.relative_attention_bias.weight.grad.double()
    agree, agree_b = float((g_ours - g_hf).norm() / g_hf.norm()), float((b_ours - b_hf).norm() / b_hf.norm())
    brt()
    ours(); hf(); brt()                                          # second warm-up round of each path
    t = dict(ours=[], hf=[], bert=[])
    for _ in range(rounds):
        t["ours"].append(timed(ours))
        t["hf"].append(timed(hf))
        t["bert"].append(timed(brt))
    med = lambda v: sorted(v)[len(v) // 2]
    ev_o, ev_b = kernel_events(ours), kernel_events(brt)
    tot_o, tot_b = sum(v[1] for v in ev_o.values()) / 1e3, sum(v[1] for v in ev_b.values()) / 1e3
    pairs = sum(n * n for n in lens)
    layers = len(plm.encoder.layer)
    groups = {"relb::fwd_kernel": _group(ev_o, "relb::fwd_kernel"),
              "relb::bwd (delta + dq + dkv)": _group(ev_o, "relb::delta_kernel", "relb::dq_kernel", "relb::dkv_kernel"),
              "relb::dbias (dbias + dbias_sum)": _group(ev_o, "relb::dbias_kernel", "relb::dbias_sum_kernel"),
              "bert attention fwd": _group(ev_b, "attn_fwd", "attn_short_fwd", "short_fwd"),
              "bert attention (all attn_ kernels)": _group(ev_b, "attn_")}
    for key, fl in (("relb::fwd_kernel", 4.0), ("relb::bwd (delta + dq + dkv)", 10.0), ("relb::dbias (dbias + dbias_sum)", 4.0)):
        g = groups[key]
        g["flops"] = fl * 64 * HEADS * layers * pairs
        if g["device_ms"]:
            g["TFLOP_per_s"] = g["flops"] / g["device_ms"] / 1e9
    dbias_ms = groups["relb::dbias (dbias + dbias_sum)"]["device_ms"]
    top = lambda ev, tot: [dict(name=k if len(k) <= 90 else k[:87] + "...", launches=v[0], ms=v[1] / 1e3, share=v[1] / 1e3 / max(tot, 1e-9))
                           for k, v in sorted(ev.items(), key=lambda kv: -kv[1][1])[:10]]
    return dict(batch=name, sequences=n_seq, min_len=lo, max_len=hi, tokens=sum(lens), padded_tokens=int(sum(d[0].numel() for d in data)),
                micro_batch=batch, micro_batches=len(data), rounds=rounds, ours_ms=t["ours"], hf_ms=t["hf"], bert_ms=t["bert"],
                ours_median_ms=med(t["ours"]), hf_median_ms=med(t["hf"]), bert_median_ms=med(t["bert"]),
                ours_range_ms=[min(t["ours"]), max(t["ours"])], hf_range_ms=[min(t["hf"]), max(t["hf"])],
                bert_range_ms=[min(t["bert"]), max(t["bert"])],
                speedup_vs_hf_median=med(t["hf"]) / med(t["ours"]), ours_over_bert_median=med(t["ours"]) / med(t["bert"]),
                grad_rel_diff_layer1_ffn_out=agree if math.isfinite(agree) else None,
                grad_rel_diff_relative_attention_bias=agree_b if math.isfinite(agree_b) else None,
                ours_total_kernel_ms=tot_o, bert_total_kernel_ms=tot_b, kernel_ms_difference_to_bert=tot_o - tot_b,
                bias_gradient_kernel_ms=dbias_ms,
                bias_gradient_share_of_difference=(dbias_ms / (tot_o - tot_b)) if tot_o > tot_b else None,
                kernel_groups=groups, ours_top_kernels=top(ev_o, tot_o), bert_top_kernels=top(ev_b, tot_b))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", type=int, default=12)
    ap.add_argument("--vocab", type=int, default=4096)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mpnet_probe needs a GPU (a CPU run measures nothing)")
    dev = torch.device("cuda:0")
    from gmlm_amd import bert, mpnet
    plm, ref = build(a.layers, a.vocab, dev)
    mpnet.check_supported(plm)
    bert.check_supported(ref)
    res = dict(what="all-mpnet-base-v2 geometry text encoder, bf16 forward + backward: packed kernel path vs HF bf16 autocast (eager "
                    "attention) vs this tree's BERT path at the same geometry, alternating rounds in one process",
               device=torch.cuda.get_device_name(0), layers=a.layers, hidden=HIDDEN, heads=HEADS, intermediate=INTER,
               kernel_figures_source="torch.profiler device events, one pass of each kernel path after the timed rounds",
               batches=[run(plm, ref, "short", 1257, 16, 128, a.vocab, 419, a.rounds, dev, 1),
                        run(plm, ref, "long", 256, 256, 512, a.vocab, 32, a.rounds, dev, 2)])
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
