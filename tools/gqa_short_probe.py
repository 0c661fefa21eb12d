"""Short-sequence grouped attention (gmlm_attention_gqa_short_*, attn_gqa_short.hip) against the streaming grouped kernels of the
same build, bf16, forward + backward, in ONE process with alternating rounds.

Geometries: EuroBERT-610m as tools/eurobert_probe.py has it (18 query / 6 KV heads x 64, bidirectional) and Qwen2.5-0.5B as
tools/llama_probe.py has it (14 / 2 x 64, causal).  Batches: ``short`` 1,257 sequences of 16-128 tokens (the headline workload's text
batch) and ``long`` 256 sequences of 256-512 tokens, on which the short route does not apply (max_len > 128): there the probe only
records that ``groups`` is not built and times the streaming route.

  (a) attention alone, forward + backward of one layer over the whole batch as one packed call on prebuilt operands, through
      ops._causal_varlen_fwd / _bwd (the C entry points, no autograd bookkeeping): ``short`` = with groups, ``stream`` = without;
  (b) bidirectional only: the same heads with K / V expanded to one KV head per query head on the K5 short kernels
      (ops.attention_qkv with groups), WITH the expansion copies (the [q | k x rep | v x rep] buffer is built inside the timed call)
      and the fold of dK / dV over each group charged;
  (c) the whole packed encoder pass (micro-batches of 419 sequences, forward + backward) with ``groups`` given against groups=None.

Times: host clock around a device synchronise, two warm-up rounds then ``--rounds`` alternating rounds, medians with ranges; the device
kernel time of one further pass per route is reported beside them, so that host overhead cannot decide a comparison.  Writes one JSON
file (``--out``) and prints it.  Needs a GPU.

    python tools/gqa_short_probe.py --out profiles/gqa_short_probe.json
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import eurobert_probe  # noqa: E402  (tools/ is the script dir)
import llama_probe  # noqa: E402
from qwen3_probe import batches, emit, kernel_table, pack, timed  # noqa: E402

D = 64
FAMILIES = dict(eurobert=dict(mod=eurobert_probe, hq=eurobert_probe.HQ, hkv=eurobert_probe.HKV, bidir=True, layers=26),
                qwen2=dict(mod=llama_probe, hq=llama_probe.HQ, hkv=llama_probe.HKV, bidir=False, layers=24))
BATCHES = (("short", 1257, 16, 128, 419), ("long", 256, 256, 512, 32))


def med(v):
    return sorted(v)[len(v) // 2]


def stats(t):
    return {k + "_ms": v for k, v in t.items()} | {k + "_median_ms": med(v) for k, v in t.items()} | \
        {k + "_range_ms": [min(v), max(v)] for k, v in t.items()}


def alternate(paths, rounds):
    for _ in range(2):                                           # two warm-up rounds of each path
        for fn in paths.values():
            fn()
    t = {k: [] for k in paths}
    for _ in range(rounds):
        for k, fn in paths.items():
            t[k].append(timed(fn))
    return t


def run_attention(fam, name, n_seq, lo, hi, reps, rounds, dev):
    from gmlm_amd import ops
    hq, hkv, bidir = fam["hq"], fam["hkv"], fam["bidir"]
    g = torch.Generator().manual_seed(2)
    lens = torch.randint(lo, hi + 1, (n_seq,), generator=g)
    cu = torch.zeros(n_seq + 1, dtype=torch.int32)
    cu[1:] = lens.cumsum(0)
    cu, rows, longest = cu.to(dev), int(lens.sum()), int(lens.max())
    scale, rep = D ** -0.5, hq // hkv
    nq, nk = hq * D, hkv * D
    x = torch.randn(rows, (hq + 2 * hkv) * D, generator=g).to(dev, torch.bfloat16)
    go = torch.randn(rows, nq, generator=g).to(dev, torch.bfloat16)
    short_ok = ops._gqa_short_path(True, x.dtype, D, longest, n_seq, hq)
    groups = ops.pack_sequence_groups(lens.tolist()).to(dev) if short_ok else None
    q, k, v = x[:, :nq], x[:, nq:nq + nk], x[:, nq + nk:]

    def route(gr):
        def fn():
            out, out_lo, lse = ops._causal_varlen_fwd(q, k, v, cu, n_seq, longest, hq, hkv, scale, gr is None, D, bidir, gr)
            dx = torch.empty_like(x)
            ops._causal_varlen_bwd(q, k, v, out, out_lo, go, lse, cu, n_seq, longest, hq, hkv, scale, dx[:, :nq], dx[:, nq:nq + nk],
                                   dx[:, nq + nk:], D, bidir, gr)
            return out, dx
        return fn

    def expanded():
        """K / V copied out to hq heads, the K5 short kernels, dK / dV folded back over each group: everything charged"""
        x3 = x.view(rows, hq + 2 * hkv, D)
        xe = torch.cat([x3[:, :hq], x3[:, hq:hq + hkv].repeat_interleave(rep, 1), x3[:, hq + hkv:].repeat_interleave(rep, 1)], 1)
        xe = xe.reshape(rows, 3 * nq).requires_grad_(True)
        out = ops.attention_qkv(xe, None, hq, scale, cu_seqlens=cu, max_len=longest, pair_count=float((lens.double() ** 2).sum()),
                                groups=groups)
        out.backward(go)
        ge = xe.grad
        fold = lambda t: t.view(rows, hkv, rep, D).float().sum(2).to(torch.bfloat16).reshape(rows, nk)
        return out.detach(), torch.cat([ge[:, :nq], fold(ge[:, nq:2 * nq]), fold(ge[:, 2 * nq:])], 1)

    paths = dict(stream=route(None))
    if short_ok:
        paths["short"] = route(groups)
        if bidir:
            paths["expanded"] = expanded
    many = lambda fn: (lambda: [fn() for _ in range(reps)])
    res = dict(batch=name, sequences=n_seq, rows=rows, longest=longest, hq=hq, hkv=hkv, causal=not bidir, calls_per_round=reps, rounds=rounds,
               short_route_applies=short_ok, work_items=None if groups is None else int(groups.numel() - 1))
    ref = paths["stream"]()
    for kname, fn in paths.items():
        if kname != "stream":
            o, gx = fn()
            res[kname + "_vs_stream_rel_diff"] = dict(out=float((o.double() - ref[0].double()).norm() / ref[0].double().norm()),
                                                      grad=float((gx.double() - ref[1].double()).norm() / ref[1].double().norm()))
    t = alternate({kname: many(fn) for kname, fn in paths.items()}, rounds)
    t = {kname: [ms / reps for ms in v] for kname, v in t.items()}
    res.update(stats(t))
    for kname in paths:
        if kname != "stream":
            res[f"speedup_{kname}_vs_stream_median"] = med(t["stream"]) / med(t[kname])
    res["kernels"] = {kname: kernel_table(fn, top=6) for kname, fn in paths.items()}
    return res


def run_encoder(fam, plm, name, n_seq, lo, hi, vocab, batch, rounds, dev):
    from gmlm_amd import eurobert, llama, ops
    mod, encode = (eurobert, eurobert.eurobert_encode_packed) if fam["bidir"] else (llama, llama.llama_encode_packed)
    data, tokens = batches(n_seq, lo, hi, vocab, batch, dev)
    pdata = pack(data)
    short_ok = all(ops._gqa_short_path(True, torch.bfloat16, D, width, lens.numel(), fam["hq"]) for _, _, _, width, _, lens in pdata)
    groups = [ops.pack_sequence_groups(lens.tolist()).to(dev) if short_ok else None for *_, lens in pdata]

    def step(use_groups):
        def fn():
            plm.zero_grad(set_to_none=True)
            weights = mod.prepare_weights(plm, torch.bfloat16)
            for (tok, pos, cu, width, seq, lens), gr in zip(pdata, groups):
                hs = encode(plm, tok, pos, cu, width, torch.bfloat16, True, False, weights, groups=gr if use_groups else None)
                pooled = torch.zeros(lens.numel(), hs.shape[1], dtype=hs.dtype, device=hs.device).index_add_(0, seq, hs)
                (pooled.float() / lens[:, None].float()).sum().backward()
        return fn

    paths = dict(stream=step(False))
    if short_ok:
        paths["short"] = step(True)
    grads = {}
    for kname, fn in paths.items():
        fn()
        grads[kname] = plm.layers[0].mlp.down_proj.weight.grad.double().clone()
    t = alternate(paths, rounds)
    res = dict(batch=name, sequences=n_seq, tokens=tokens, micro_batch=batch, micro_batches=len(pdata), rounds=rounds,
               short_route_applies=short_ok, **stats(t))
    if short_ok:
        res["speedup_short_vs_stream_median"] = med(t["stream"]) / med(t["short"])
        res["grad_rel_diff_layer0_down_proj_short_vs_stream"] = float((grads["short"] - grads["stream"]).norm() / grads["stream"].norm())
    res["kernels"] = {kname: kernel_table(fn, top=6) for kname, fn in paths.items()}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--vocab", type=int, default=4096)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--attn-reps", type=int, default=10)
    ap.add_argument("--skip-encoder", action="store_true", help="(a) and (b) only: no model is built")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("gqa_short_probe needs a GPU (a CPU run measures nothing)")
    dev = torch.device("cuda:0")
    res = dict(what="short-sequence grouped attention (gqas:: kernels) vs the streaming grouped kernels of the same build, bf16 forward + "
                    "backward, alternating rounds in one process after two warm-up rounds: (a) attention of one layer alone, (b) "
                    "bidirectional: vs K / V expanded to hq heads on the K5 short kernels with the copies and the dK / dV fold "
                    "charged, (c) the whole packed encoder pass with groups vs without",
               device=torch.cuda.get_device_name(0), head_dim=D,
               kernel_figures_source="torch.profiler device events, one pass per route after the timed rounds", families={})
    for fname, fam in FAMILIES.items():
        plm = None if a.skip_encoder else fam["mod"].build(fam["layers"], a.vocab, dev)
        res["families"][fname] = dict(
            hq=fam["hq"], hkv=fam["hkv"], causal=not fam["bidir"], layers=fam["layers"],
            attention=[run_attention(fam, n, s, lo, hi, a.attn_reps, a.rounds, dev) for n, s, lo, hi, _ in BATCHES],
            encoder=[] if plm is None else [run_encoder(fam, plm, n, s, lo, hi, a.vocab, b, a.rounds, dev) for n, s, lo, hi, b in BATCHES])
        del plm
        torch.cuda.empty_cache()
    emit(res, a.out)


if __name__ == "__main__":
    main()
