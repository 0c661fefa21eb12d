"""deberta-v3-base-geometry text encoder, forward + backward in bf16, three models in one process in alternating rounds:
  ours   this project's kernel path (gmlm_amd.deberta, the packed pass GraphTextLM runs);
  hf     HF's DebertaV2Model under bf16 autocast on the same device (its own eager disentangled attention);
  bert   this tree's BERT path (gmlm_amd.bert, packed) at the same geometry: what the two position terms cost.
The parent of this encoder path refused the model, so HF's module is what a user had.

Workload: 12 layers, hidden 768, 12 heads x 64, intermediate 3,072, position_buckets 256, vocabulary 128,100, random weights,
nothing downloaded, dropouts 0; two text batches:
  short   1,257 sequences of 16-128 tokens (the headline workload's text batch);
  long    256 sequences of 256-512 tokens.
Length-sorted micro-batches; HF sees each padded to its longest sequence with an attention mask, the two kernel paths the same
sequences packed.  All compute the same loss: the mean-pooled rows against a fixed random direction.  The BERT path at d = 64,
bf16, sequences <= 128 and >= 512 (sequence, head) pairs runs its LDS-resident short-sequence attention kernels; the DeBERTa
path has no such form, so on the short batch the difference to BERT is the two terms AND the streaming kernels.
Times: host clock around a device synchronise, ``--rounds`` alternating rounds after two warm-up rounds of each path.  The
per-kernel figures are torch.profiler's device-kernel events of one further pass of the DeBERTa and of the BERT path, taken
after the timed rounds.  The difference of the two paths' total device-kernel times is split into
  table_gradient   disent::dc_kernel + disent::dpt_kernel;
  attention        disent::fwd / delta / dq / dkv less all of the BERT path's attention kernels (the table reads);
  library_gemm     every GEMM-library kernel of the DeBERTa pass less those of the BERT pass (the table GEMMs, their backward,
                   and the Qr | Kr projection);
  other            the rest (zero fills, strided copies and casts around the table GEMMs, the relative-embedding LayerNorm).
Writes one JSON file (``--out``) and prints it.  Needs a GPU: there is no CPU fallback.

    python tools/deberta_probe.py --out profiles/deberta_probe.json
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
    from transformers import BertConfig, BertModel, DebertaV2Config, DebertaV2Model
    common = dict(vocab_size=vocab, hidden_size=HIDDEN, intermediate_size=INTER, num_hidden_layers=layers, num_attention_heads=HEADS,
                  hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)
    torch.manual_seed(0)
    with torch.device(dev):
        plm = DebertaV2Model(DebertaV2Config(max_position_embeddings=512, relative_attention=True, pos_att_type=["p2c", "c2p"],
                                             share_att_key=True, norm_rel_ebd="layer_norm", position_buckets=256,
                                             max_relative_positions=-1, position_biased_input=False, type_vocab_size=0,
                                             layer_norm_eps=1e-7, **common))
        ref = BertModel(BertConfig(max_position_embeddings=512, **common), add_pooling_layer=False)
    with torch.no_grad():
        plm.encoder.rel_embeddings.weight.normal_()
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
    from gmlm_amd import deberta
    plm.zero_grad(set_to_none=True)
    weights = deberta.prepare_weights(plm, torch.bfloat16)
    for _, _, lens, tok, pos, cu, width, seq, _ in data:
        _loss(deberta.deberta_encode_packed(plm, tok, pos, cu, width, torch.bfloat16, True, False, weights), lens, seq).backward()


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
    b_ours = plm.encoder.rel_embeddings.weight.grad.double().clone()
    hf()
    g_hf = dict(plm.named_parameters())[name_g].grad.double()
    b_hf = plm.encoder.rel_embeddings.weight.grad.double()
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
    gemm = ("Cijk_", "gemm", "Gemm", "GEMM")
    groups = {"disent::fwd_kernel": _group(ev_o, "disent::fwd_kernel"),
              "disent::bwd (delta + dq + dkv)": _group(ev_o, "disent::delta_kernel", "disent::dq_kernel", "disent::dkv_kernel"),
              "disent::dtab (dc + dpt)": _group(ev_o, "disent::dc_kernel", "disent::dpt_kernel"),
              "library GEMMs (deberta pass)": _group(ev_o, *gemm),
              "library GEMMs (bert pass)": _group(ev_b, *gemm),
              "bert attention (all attn_ kernels)": _group(ev_b, "attn_")}
    for key, fl in (("disent::fwd_kernel", 4.0), ("disent::bwd (delta + dq + dkv)", 10.0), ("disent::dtab (dc + dpt)", 8.0)):
        g = groups[key]
        g["flops"] = fl * 64 * HEADS * layers * pairs
        if g["device_ms"]:
            g["TFLOP_per_s"] = g["flops"] / g["device_ms"] / 1e9
    dtab_ms = groups["disent::dtab (dc + dpt)"]["device_ms"]
    attn_ms = groups["disent::fwd_kernel"]["device_ms"] + groups["disent::bwd (delta + dq + dkv)"]["device_ms"] - groups["bert attention (all attn_ kernels)"]["device_ms"]
    gemm_ms = groups["library GEMMs (deberta pass)"]["device_ms"] - groups["library GEMMs (bert pass)"]["device_ms"]
    diff = tot_o - tot_b
    split = dict(table_gradient=dtab_ms, attention=attn_ms, library_gemm=gemm_ms, other=diff - dtab_ms - attn_ms - gemm_ms)
    from gmlm_amd import deberta
    tab_bytes = sum(2 * 4 * HEADS * int(d[3].numel()) * deberta.bucket_columns(d[6], 256, 512).width for d in data)
    top = lambda ev, tot: [dict(name=k if len(k) <= 90 else k[:87] + "...", launches=v[0], ms=v[1] / 1e3, share=v[1] / 1e3 / max(tot, 1e-9))
                           for k, v in sorted(ev.items(), key=lambda kv: -kv[1][1])[:10]]
    return dict(batch=name, sequences=n_seq, min_len=lo, max_len=hi, tokens=sum(lens), padded_tokens=int(sum(d[0].numel() for d in data)),
                micro_batch=batch, micro_batches=len(data), rounds=rounds, ours_ms=t["ours"], hf_ms=t["hf"], bert_ms=t["bert"],
                ours_median_ms=med(t["ours"]), hf_median_ms=med(t["hf"]), bert_median_ms=med(t["bert"]),
                ours_range_ms=[min(t["ours"]), max(t["ours"])], hf_range_ms=[min(t["hf"]), max(t["hf"])],
                bert_range_ms=[min(t["bert"]), max(t["bert"])],
                speedup_vs_hf_median=med(t["hf"]) / med(t["ours"]), ours_over_bert_median=med(t["ours"]) / med(t["bert"]),
                grad_rel_diff_layer1_ffn_out=agree if math.isfinite(agree) else None,
                grad_rel_diff_rel_embeddings=agree_b if math.isfinite(agree_b) else None,
                ours_total_kernel_ms=tot_o, bert_total_kernel_ms=tot_b, kernel_ms_difference_to_bert=diff,
                difference_split_ms=split, difference_split_share={k: v / diff for k, v in split.items()} if diff > 0 else None,
                table_bytes_per_layer=tab_bytes, table_gib_per_layer=tab_bytes / 2 ** 30,
                kernel_groups=groups, ours_top_kernels=top(ev_o, tot_o), bert_top_kernels=top(ev_b, tot_b))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", type=int, default=12)
    ap.add_argument("--vocab", type=int, default=128100)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("deberta_probe needs a GPU (a CPU run measures nothing)")
    dev = torch.device("cuda:0")
    from gmlm_amd import bert, deberta
    plm, ref = build(a.layers, a.vocab, dev)
    deberta.check_supported(plm)
    bert.check_supported(ref)
    res = dict(what="deberta-v3-base geometry text encoder, bf16 forward + backward: packed kernel path vs HF bf16 autocast (eager "
                    "disentangled attention) vs this tree's BERT path at the same geometry, alternating rounds in one process",
               device=torch.cuda.get_device_name(0), layers=a.layers, hidden=HIDDEN, heads=HEADS, intermediate=INTER, position_buckets=256, vocab=a.vocab,
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
