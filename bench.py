#!/usr/bin/env python3
"""bench.py — nodes/sec of one full-batch GraphTextLM forward+backward (BASELINE.json metric) on MI355X.

    python bench.py [--gpus N] [--steps K] [--warmup W] [--dump-outputs DIR] [--full]   # N>1: launched by torch.distributed.run

Workload (SURVEY.md §8d "S3", BASELINE configs[2], the config the metric is quoted on): synthetic
Squirrel-size graph (5,201 nodes, 217,073 edges, F_in=2089, 5 classes), hidden_channels=768,
BERT-base-geometry text encoder (768 x 12 layers x 12 heads, random init), dropout as in the reference
(0.3 model / 0.1 encoder), ~1,250 active text nodes of 16..128 tokens, bf16 GEMM/attention operands with
fp32 accumulation and statistics.  A "step" = soft-mask -> forward -> CE(label_smoothing=0.2) -> backward
(the optimiser is outside the metric: SURVEY.md §8d).  With N > 1 every rank owns a Squirrel-size
partition of an N x 5,201-node graph (1-D node partition, halo exchange + RCCL collectives): weak scaling.

Prints ONE JSON line (rank 0).  A plain run sets up, warms up, times the K steps and prints the headline ("value" nodes/s,
"ms_per_step" = wall time of one timed step); nothing else runs.  ``--dump-outputs DIR`` then writes what the last timed
step computed (see dump_outputs).  ``--full`` adds the extra objects (N = 1):
  "roofline"      the RGCN aggregation kernel in the regime where HBM is the binding roof: a 1.25M-node / 12.5M-edge
                  power-law shard (one GPU's share of the 10M-node S5 config), F = 768 bf16, X = 1.9 GB >> the 256 MiB
                  Infinity Cache; algorithmic bytes (SURVEY section 8d formula) / HIP-event launch time; "traffic" = HBM
                  bytes per launch from the committed rocprofv3 PMC passes (profiles/)
  "attention"     the MFMA-bound kernels: CrossAttention geometry (h=8, d=96, N=20,804) and masked MHA (B=32, h=12, L=512,
                  d=64), padded AND executed flops, HIP-event time, PMC MFMA-busy fraction from profiles/
  "kernels"       every hand-written kernel of the step (HIP events on the launch stream, K more steps after the timed ones);
                  the in-step aggregation launches run on a cache-resident X (8-32 MB) and are reported against the
                  L2 / Infinity-Cache gather rates of the guide, not against 8 TB/s
  "fp32"          the same step with fp32 operands (the north_star parity dtype), 3 timed steps
  "reference_recompute"  the same step with the reference's activation + PLM gradient checkpointing, 3 timed steps
  "power_law_variant"  the same step on a heavy-tailed graph of the same size (R_a = 4 instead of the headline's 1)
  "cpu_baseline"  the CPU oracle timed on this box's host cores on a bounded sample (1 warm-up + median of 3)

Other workloads (not the metric's config; each prints its own line):
  --workload arxiv   ogbn-arxiv-size full model (N=169,343, E=1,166,243, F_in=128, C=40), 1..N GPUs (node partition)
  --workload s5      10M-node / 100M-edge Chung-Lu graph, get_graph_embeddings forward+backward, STRONG scaling over the
                     node partition (the full model is bounded by the reference's own dense N x N attention at this size:
                     6e17 flop per forward)
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

HBM_PEAK_GBS = 8000.0        # MI355X spec (MI355X_MICROARCH.md): 8.0 TB/s
MFMA_BF16_PEAK_TF = 2500.0   # dense bf16
MFMA_F32_PEAK_TF = 157.3

WORKLOADS = {  # name: (N, E, F_in, C)
    "cornell": (183, 298, 1703, 5),
    "chameleon": (2277, 36101, 2325, 5),
    "squirrel": (5201, 217073, 2089, 5),
    "arxiv": (169343, 1166243, 128, 40),
}


def synthetic(name, n_parts=1):
    """Seeded synthetic graph of the named size; with n_parts > 1 the node/edge counts scale by n_parts."""
    n, e, f_in, c = WORKLOADS[name]
    n, e = n * n_parts, e * n_parts
    g = torch.Generator().manual_seed(1000 + list(WORKLOADS).index(name) + 2)
    x = torch.randn(n, f_in, generator=g)
    ei = torch.randint(0, n, (2, e), generator=g, dtype=torch.long)
    y = torch.randint(0, c, (n,), generator=g)
    perm = torch.randperm(n, generator=g)
    train = torch.zeros(n, dtype=torch.bool)
    train[perm[: int(0.48 * n)]] = True
    active = train & (torch.rand(n, generator=g) < 0.5)
    return dict(n=n, e=e, f_in=f_in, c=c, x=x, edge_index=ei, y=y, active=active)


def synthetic_tokens(n, max_len, vocab, seed, min_len=16):
    g = torch.Generator().manual_seed(seed)
    lens = torch.randint(min(min_len, max_len), max_len + 1, (n,), generator=g)
    ids = torch.randint(5, vocab, (n, max_len), generator=g)
    am = (torch.arange(max_len)[None, :] < lens[:, None]).long()
    return ids * am, am


def build_model(args, data, dev):
    from transformers import BertConfig, BertModel
    import gmlm_amd
    cfg = BertConfig(vocab_size=args.vocab, hidden_size=args.plm_hidden, num_hidden_layers=args.plm_layers,
                     num_attention_heads=args.plm_hidden // 64, intermediate_size=4 * args.plm_hidden,
                     max_position_embeddings=max(512, args.max_len))
    torch.manual_seed(0)
    enc = BertModel(cfg)
    cd = torch.bfloat16 if args.dtype == "bf16" else torch.float32
    m = gmlm_amd.GraphTextLM(data["f_in"], args.hc, data["c"], dropout_rate=0.3, plm_encoder=enc,
                             plm_max_length=args.max_len, compute_dtype=cd,
                             plm_gradient_checkpointing=recompute_flags(args)[1],    # reference: ON (main.py:217-218)
                             activation_checkpointing=recompute_flags(args)[0])      # reference: ON (main.py:278-314)
    m.overlap_streams = bool(getattr(args, "overlap_streams", False))
    return m.to(dev).train()


def recompute_flags(args):
    """(activation_checkpointing, plm_gradient_checkpointing).  The reference recomputes every RGCN block
    (torch.utils.checkpoint, main.py:278-314) and every BertLayer (HF gradient checkpointing, main.py:217-219) in backward: same
    results, more time, less memory.  The headline step runs WITHOUT recomputation (its activations fit easily) and says so in
    ``config``; ``--reference-recompute`` / the ``reference_recompute`` leg run with both ON; arxiv always does."""
    on = args.reference_recompute or args.workload == "arxiv"
    return on, (on or args.plm_ckpt)


def cpu_baseline(args, data, ids, am):
    """Oracle (oracle/gmlm_oracle.py, CPU fp32) forward+backward on the same graph; the PLM leg runs on a
    bounded sample of active nodes and is scaled linearly to all of them (it is row-wise independent)."""
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import gmlm_oracle as O
    from helpers import bert_state_template, model_state_template
    try:
        avail = len(os.sched_getaffinity(0))
    except AttributeError:
        avail = os.cpu_count() or 1
    threads = max(1, min(avail, 16))                  # the 1-GPU box's CPU share is 16 cores
    torch.set_num_threads(threads)
    say = lambda msg: print(f"[cpu_baseline] {msg}", file=sys.stderr, flush=True)
    hc = min(args.hc, args.cpu_hc)
    plm = dict(hidden=args.plm_hidden, layers=args.plm_layers, heads=args.plm_hidden // 64, inter=4 * args.plm_hidden,
               vocab=args.vocab, max_pos=max(512, args.max_len))
    tmpl = model_state_template(data["f_in"], hc, data["c"], plm)
    g = torch.Generator().manual_seed(1)

    def init(k, shape):
        if len(shape) > 1:
            return torch.randn(*shape, generator=g) * 0.02
        norm_gain = k.endswith("mean_scale") or (k.endswith("weight") and any(t in k for t in ("LayerNorm", "layer_norm", "gnorm", "fusion_network.1")))
        return torch.ones(*shape) if norm_gain else torch.zeros(*shape)

    say(f"building the oracle model (hidden_channels={hc}, {threads} threads)")
    sd = {k: init(k, s) for k, s in tmpl.items()}
    plm_sd = {k[len("plm_encoder."):]: v for k, v in sd.items() if k.startswith("plm_encoder.")}
    om = O.OracleGraphTextLM(data["f_in"], hc, data["c"], plm_sd, plm["heads"])
    om.load_reference_state(sd)
    del sd, plm_sd
    mask = data["active"]
    idx = mask.nonzero(as_tuple=True)[0]
    sample = idx[: args.cpu_plm_sample]
    smask = torch.zeros_like(mask)
    smask[sample] = True
    # leg 1: everything except the text encoder, on the full graph (empty text mask => plm_embeds = 0):
    # 1 warm-up + median of 3
    def leg1():
        om.zero_grad(set_to_none=True)
        t0 = time.time()
        xm = O.soft_masking_gnn_input(data["x"], mask, om.gnn_mask_token_embed, 0.7)
        logits = om(xm, data["edge_index"], ids, am, torch.zeros_like(mask), plm_batch_size=32)
        loss = F.cross_entropy(logits[mask], data["y"][mask], label_smoothing=0.2)
        loss.backward()
        return time.time() - t0

    t_all = time.time()
    warm = leg1()
    say(f"GNN + cross-attention + head fwd+bwd warm-up done ({warm:.1f}s)")
    runs = sorted(leg1() for _ in range(args.cpu_repeats))
    t_rest = runs[len(runs) // 2]
    say(f"... median of {len(runs)}: {t_rest:.1f}s ({', '.join('%.1f' % r for r in runs)})")
    # leg 2: BERT + pooling on a bounded sample of the active nodes, scaled linearly (row-wise independent)
    def leg2():
        om.zero_grad(set_to_none=True)
        t1 = time.time()
        pe = om.encode_texts(ids, am, smask, 32)
        pe.sum().backward()
        return time.time() - t1

    leg2()
    pl = sorted(leg2() for _ in range(args.cpu_repeats))
    t_plm = pl[len(pl) // 2]
    say(f"BERT leg on {sample.numel()} nodes: median {t_plm:.1f}s")
    est = t_rest + t_plm * (idx.numel() / max(sample.numel(), 1))
    # the reference's per-edge Python loop for edge typing (main.py:257-267), timed on a bounded sample of edges and
    # scaled linearly: the "faithful" variant of SURVEY.md section 8d
    t2 = time.time()
    ne = min(data["e"], 20000)
    O.edge_types_loop(data["edge_index"][:, :ne], data["n"])
    t_loop = (time.time() - t2) * (data["e"] / ne)
    say(f"per-edge typing loop: {t_loop:.1f}s for all edges (scaled from {ne})")
    return dict(value=round(data["n"] / est, 3), unit="nodes/s", cores=threads, kind="port",
                faithful_value=round(data["n"] / (est + t_loop), 3),
                sample=(f"oracle (CPU fp32 restatement) fwd+bwd on the same {data['n']}-node graph, vectorised edge typing, "
                        f"hidden_channels={hc}{'' if hc == args.hc else ' (bench uses %d)' % args.hc}: GNN + cross-attention + head "
                        f"on the full graph measured (1 warm-up + median of {len(runs)}: {t_rest:.1f}s); BERT leg measured on "
                        f"{sample.numel()} of {idx.numel()} active nodes (median {t_plm:.1f}s) and scaled linearly"),
                runs_s=dict(gnn_head=[round(r, 2) for r in runs], bert_sample=[round(r, 2) for r in pl]),
                seconds_measured=round(time.time() - t_all, 1))


def device_names(dev, world):
    """What every rank runs on, gathered over the process group: lets the reader of the JSON line see that RCCL saw N ranks on
    N different GPUs ("rank: name (cuda:i, pci bus id)")."""
    props = torch.cuda.get_device_properties(dev)
    mine = f"{props.name} (cuda:{dev.index}, uuid {str(getattr(props, 'uuid', ''))[-12:]})"
    if world == 1:
        return [mine]
    out = [None] * world
    torch.distributed.all_gather_object(out, mine)
    return out


def _time_events(fn, iters, warm=2):
    for _ in range(warm):
        fn()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
    for e0, e1 in ev:
        e0.record()
        fn()
        e1.record()
    torch.cuda.synchronize()
    ts = sorted(e0.elapsed_time(e1) for e0, e1 in ev)
    return sum(ts) / len(ts), ts[len(ts) // 2]


def _time_batch(fn, iters=20, warm=3):
    """ONE event bracket around ``iters`` back-to-back launches (per-launch event pairs add 3-5 us of their own, visible
    on 35 us kernels)."""
    for _ in range(warm):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def micro(dev, args):
    """Kernel micro-benchmarks at sizes where the named roofline is the binding one:
    * aggregation on a power-law graph whose feature matrix is far larger than the 256 MiB Infinity Cache
      (a per-GPU shard of the 10M-node S5 config), F=768;
    * BERT-geometry masked MHA at L=512 (B=32, h=12, d=64) and CrossAttention geometry (h=8, d=96)."""
    import gmlm_amd
    from gmlm_amd import ops
    out = {}
    groups = set(args.micro_select.split(","))
    if "spmm" in groups:
        _micro_spmm(dev, args, out)
    if "attn" in groups:
        _micro_attn(dev, args, out)
    return out


def _micro_spmm(dev, args, out):
    import gmlm_amd
    from gmlm_amd import ops
    g = torch.Generator(device=dev).manual_seed(5)
    n, e, f = args.micro_nodes, args.micro_edges, 768
    w = (torch.arange(n, device=dev, dtype=torch.float32) + 1.0).pow(-1.0 / 1.2)          # Chung-Lu, alpha = 2.2
    perm = torch.randperm(n, device=dev, generator=g)
    src = perm[torch.multinomial(w, e, replacement=True, generator=g)]
    dst = perm[torch.multinomial(w, e, replacement=True, generator=g)]
    ei = torch.stack([src, dst])
    del w, perm, src, dst
    csr = gmlm_amd.build_rel_csr(ei, n, 5)
    for dt, name in ((torch.bfloat16, "bf16"), (torch.float32, "f32")):
        x = torch.randn(n, f, device=dev, dtype=dt)
        s_fwd = n * csr.r_active
        a_fwd = ops.spmm_algorithmic_bytes(e, s_fwd, s_fwd, f, x.element_size())
        avg, med = _time_events(lambda: ops.RGCNAggregate.apply(x, csr), 5)
        out[f"spmm_fwd_{name}"] = {"nodes": n, "edges": e, "f": f, "r_active": csr.r_active, "avg_ms": round(avg, 3),
                                   "algorithmic_GB": round(a_fwd / 1e9, 2), "GBps": round(a_fwd / avg / 1e6, 1),
                                   "frac_hbm_peak": round(a_fwd / avg / 1e6 / HBM_PEAK_GBS, 4)}
        gh = torch.randn(n, csr.r_active * f, device=dev, dtype=dt)
        gx = torch.empty(n, f, device=dev, dtype=dt)
        a_bwd = ops.spmm_algorithmic_bytes(e, n, n, f, x.element_size(), True)
        avg, med = _time_events(lambda: ops._spmm(gh.view(n * csr.r_active, f), csr.t_rowptr, csr.t_seg, csr.inv_cnt, False, n, f, gx, csr.t_split), 5)
        out[f"spmm_bwd_{name}"] = {"avg_ms": round(avg, 3), "algorithmic_GB": round(a_bwd / 1e9, 2),
                                   "GBps": round(a_bwd / avg / 1e6, 1), "frac_hbm_peak": round(a_bwd / avg / 1e6 / HBM_PEAK_GBS, 4)}
        del x, gh, gx
    del csr, ei
    torch.cuda.empty_cache()


def _micro_attn(dev, args, out):
    from gmlm_amd import ops
    for tag, b, h, l, d, masked in (("mha_L512", 32, 12, 512, 64, True), ("mha_L128", 256, 12, 128, 64, True),
                                    ("mha_L2048", 16, 12, 2048, 64, True),
                                    ("xattn_N5201", 1, 8, 5201, 96, False), ("xattn_N20804", 1, 8, 20804, 96, False)):
        q, k, v = (torch.randn(b, l, h * d, device=dev, dtype=torch.bfloat16, requires_grad=True) for _ in range(3))
        kv_len = torch.randint(l // 2, l + 1, (b,), device=dev, dtype=torch.int32) if masked else None
        go = torch.randn(b, l, h * d, device=dev, dtype=torch.bfloat16)
        fl = 4.0 * b * h * l * l * d
        fl_exec = 4.0 * h * l * d * float(kv_len.sum()) if masked else fl
        # the C-ABI entries directly (ops.AttentionBlock: two allocations + one ctypes call): through the autograd Function a
        # call costs the host more than these 35-50 us launches take, and the event bracket would time the host
        qd, kd, vd = q.detach(), k.detach(), v.detach()
        blk = ops.AttentionBlock(h, d ** -0.5)
        avg = _time_batch(lambda: blk.fwd(qd, kd, vd, kv_len, 0))
        y, lse = blk.fwd(qd, kd, vd, kv_len, 0)
        avg_b = _time_batch(lambda: blk.bwd(qd, kd, vd, y, go, lse, kv_len, 0))
        out[tag] = {"b": b, "h": h, "l": l, "d": d, "fwd_ms": round(avg, 3), "fwd_TFLOPs": round(fl / avg / 1e9, 1),
                    "fwd_frac_mfma_peak": round(fl / avg / 1e9 / MFMA_BF16_PEAK_TF, 4),
                    "fwd_TFLOPs_executed": round(fl_exec / avg / 1e9, 1), "bwd_ms": round(avg_b, 3),
                    "bwd_TFLOPs": round(2.5 * fl / avg_b / 1e9, 1),
                    "bwd_frac_mfma_peak": round(2.5 * fl / avg_b / 1e9 / MFMA_BF16_PEAK_TF, 4),
                    "note": "padded flops (masked keys counted)" if masked else "no mask"}
        del q, k, v, go, y, lse


def gnn_large(dev, args):
    """get_graph_embeddings forward+backward on one GPU's share of the 10M-node S5 config (SURVEY.md §8d:
    reported separately because the N x N cross-attention, not the GNN, bounds the full model at that size):
    power-law graph, F_in = 768, hidden_channels = args.hc, bf16, reference dropout, activation checkpointing
    like the reference (main.py:278-314)."""
    import gmlm_amd
    from transformers import BertConfig, BertModel
    n, e, f_in = args.micro_nodes, args.micro_edges, 768
    g = torch.Generator(device=dev).manual_seed(6)
    w = (torch.arange(n, device=dev, dtype=torch.float32) + 1.0).pow(-1.0 / 1.2)
    perm = torch.randperm(n, device=dev, generator=g)
    ei = torch.stack([perm[torch.multinomial(w, e, replacement=True, generator=g)],
                      perm[torch.multinomial(w, e, replacement=True, generator=g)]])
    del w, perm
    x = torch.randn(n, f_in, device=dev)
    mask = torch.rand(n, device=dev) < 0.3
    enc = BertModel(BertConfig(vocab_size=64, hidden_size=args.plm_hidden, num_hidden_layers=1,
                               num_attention_heads=args.plm_hidden // 64, intermediate_size=64, max_position_embeddings=16))
    torch.manual_seed(0)
    m = gmlm_amd.GraphTextLM(f_in, args.hc, 16, dropout_rate=0.3, plm_encoder=enc, compute_dtype=torch.bfloat16,
                             activation_checkpointing=True).to(dev).train()

    def step():
        m.zero_grad(set_to_none=True)
        out = m.get_graph_embeddings(m.soft_mask_input(x, mask, 0.7), ei)
        out.float().square().mean().backward()

    torch.cuda.reset_peak_memory_stats()
    step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        step()
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / args.steps
    csr = m.graph(ei, n)
    return {"workload": f"get_graph_embeddings fwd+bwd, power-law graph N={n} E={e} F_in={f_in} hidden_channels={args.hc} bf16, "
                        f"activation checkpointing, R_a={csr.r_active}",
            "nodes_per_s": round(n / dt, 1), "ms_per_step": round(dt * 1e3, 2),
            "peak_mem_GB": round(torch.cuda.max_memory_allocated() / 1e9, 1)}


def _profile_json(names):
    for name in names:
        try:
            with open(os.path.join(ROOT, "profiles", name)) as f:
                return json.load(f), name
        except (OSError, ValueError):
            continue
    return {}, None


def _pmc_traffic(key):
    """HBM bytes per launch from the committed rocprofv3 PMC passes (profiles/rNN_spmm_traffic.json); None if absent."""
    d, _ = _profile_json(["r03_spmm_traffic.json", "r02_spmm_traffic.json", "r01_spmm_traffic.json"])
    return d.get(key, {}).get("hbm_bytes_per_launch")


def _pmc_attn(kernel_prefix, grid=None):
    """PMC MFMA-busy fraction (SQ_VALU_MFMA_BUSY_CYCLES / (GRBM_GUI_ACTIVE/8 * 1024 SIMDs)) of an attention kernel from the
    committed profile (profiles/rNN_attn_pmc.json, made by tools/pmc_attn.py); None if absent.  ``grid``: total threads of the
    launch (several shapes run the same kernel in the profile)."""
    d, name = _profile_json(["r03_attn_pmc.json", "r02_attn_pmc.json"])
    for k, v in d.items():
        if k.startswith(kernel_prefix) and (grid is None or k.endswith("grid=%d" % grid)):
            return {"mfma_busy": v.get("mfma_util"), "mfma_busy_useful_flops": v.get("mfma_util_useful"), "valu_per_mfma": v.get("valu_per_mfma"),
                    "profile": "profiles/" + name}
    return None


def s5_strong(dev, args, world, rank):
    """BASELINE configs[4]: 10M-node / 100M-edge Chung-Lu power-law graph (alpha = 2.2, ids randomly permuted so that
    the contiguous 1-D split is a random partition), F_in = 768, get_graph_embeddings forward+backward (GNN + multi-scale
    fusion; reference dropout; activation checkpointing like main.py:278-314), STRONG scaling: the same graph on 1..N
    GPUs, value = N_total / step time.  Every rank derives the same graph from the seeded generator on its own GPU and
    plans its partition from it (or reads its shard from --partition-dir); edge types use GLOBAL out-degrees."""
    import gmlm_amd
    from gmlm_amd.dist import attach_partition, partition_file, write_partition_files
    from transformers import BertConfig, BertModel
    n, e, f_in = args.s5_nodes, args.s5_edges, 768

    def make_graph():
        g = torch.Generator(device=dev).manual_seed(1005)
        w = (torch.arange(n, device=dev, dtype=torch.float32) + 1.0).pow(-1.0 / 1.2)
        perm = torch.randperm(n, device=dev, generator=g)
        # multinomial with replacement caps the category count at 2^24: sample through the CDF instead
        cdf = torch.cumsum(w.double(), 0)
        cdf /= cdf[-1].clone()
        src = perm[torch.searchsorted(cdf, torch.rand(e, device=dev, generator=g, dtype=torch.float64)).clamp_(max=n - 1)]
        dst = perm[torch.searchsorted(cdf, torch.rand(e, device=dev, generator=g, dtype=torch.float64)).clamp_(max=n - 1)]
        return torch.stack([src, dst])

    ei, pdir, t_part = None, args.partition_dir, 0.0
    if world == 1:
        ei = make_graph()
    elif pdir is None or not os.path.exists(partition_file(pdir, rank, world)):
        # Default for N > 1: the graph is partitioned ONCE - rank 0 builds it, plans every rank's shard and writes
        # part-RRRRR-of-WWWWW.npz - and each rank then reads only its own shard (1/N of the edges, its halo and send lists)
        # instead of holding the 100M-edge list and running the planning (degree histogram, unique, sort) N times over.
        import tempfile
        pdir = pdir or os.path.join(tempfile.gettempdir(), f"gmlm_s5_parts_n{n}_e{e}_w{world}")
        t0 = time.perf_counter()
        if rank == 0 and not all(os.path.exists(partition_file(pdir, r, world)) for r in range(world)):
            full = make_graph()
            write_partition_files(full, n, world, pdir)
            del full
            torch.cuda.empty_cache()
        torch.distributed.barrier()
        t_part = time.perf_counter() - t0
    enc = BertModel(BertConfig(vocab_size=64, hidden_size=768, num_hidden_layers=1, num_attention_heads=12,
                               intermediate_size=64, max_position_embeddings=16))       # not executed: P = 768 only
    torch.manual_seed(0)
    m = gmlm_amd.GraphTextLM(f_in, args.s5_hc, 16, dropout_rate=0.3, plm_encoder=enc, compute_dtype=torch.bfloat16,
                             activation_checkpointing=True).to(dev).train()
    if world > 1:
        part = attach_partition(m, None, n, dev, partition_dir=pdir)
        lo, hi = part.plan.lo, part.plan.hi
        halo = part.plan.n_halo
    else:
        part, lo, hi, halo = None, 0, n, 0
    # pre-flight: this rank's peak is the widest block's recompute + backward.  Its input buffer holds owned + halo rows at
    # 4 * hc columns and exists together with its gradient; next to it the aggregation output H [n_local, R_a * 4 hc], its
    # gradient, the block output [n_local, 8 hc] (+ gradient, + GraphNorm's bf16 input) and the fp32 fusion accumulator.
    hc = args.s5_hc
    rows_in, rows_out = (hi - lo) + halo, hi - lo
    est = (2 * rows_in * 4 * hc * 2 + 2 * rows_out * 4 * 4 * hc * 2 + 3 * rows_out * 8 * hc * 2 + rows_out * 768 * 4 * 3
           + rows_out * f_in * 2 * 2 + 30 * 4 * hc * 8 * hc * 4 * 3)
    total_mem = torch.cuda.get_device_properties(dev).total_memory
    fits = torch.tensor([1.0 if est < 0.9 * total_mem else 0.0])
    if world > 1:
        part.all_reduce_min(fits)                                   # the same decision on every rank, taken BEFORE the first collective of a step
    if float(fits) < 0.5:
        return {"metric": "nodes/sec fwd+bwd (get_graph_embeddings, 10M-node power-law graph)", "value": None, "unit": "nodes/s",
                "n_gpus": world, "steps": 0, "warmup": 0, "ms_per_step": None, "higher_is_better": True, "scaling": "strong",
                "vs_baseline": None, "dtype": "bf16", "data": "synthetic",
                "config": {"workload": f"s5 hidden_channels={hc}: NOT RUN, pre-flight memory estimate {est / 1e9:.0f} GB per rank "
                                       f"(rows {rows_out} + halo {halo}) exceeds 90 % of {total_mem / 1e9:.0f} GB on some rank; use more GPUs or a smaller --s5-hc",
                           "world": world}}
    gx = torch.Generator(device=dev).manual_seed(77)                  # same stream on every rank: row i is the same wherever it lives
    x = torch.empty(hi - lo, f_in, device=dev, dtype=torch.bfloat16)
    chunk = 1 << 20
    for c0 in range(0, n, chunk):                                      # global rows in chunks; keep only the owned ones
        c1 = min(n, c0 + chunk)
        blk = torch.randn(c1 - c0, f_in, device=dev, generator=gx, dtype=torch.float32)
        a, b_ = max(c0, lo), min(c1, hi)
        if a < b_:
            x[a - lo:b_ - lo] = blk[a - c0:b_ - c0].to(torch.bfloat16)
    del blk
    mask = (torch.rand(n, device=dev, generator=gx) < 0.3)[lo:hi]
    r_a = m.graph(ei, n).r_active if part is None else part.csr.r_active

    def step():
        m.zero_grad(set_to_none=True)
        out = m.get_graph_embeddings(m.soft_mask_input(x, mask, 0.7), ei)
        if part is not None:
            part.grad_buckets(m).prepare()
        (out.float().square().sum() / n).backward()
        if part is not None:
            part.grad_buckets(m).finish()

    def fence():
        if world > 1:
            torch.distributed.barrier()
        torch.cuda.synchronize()

    torch.cuda.reset_peak_memory_stats()
    for _ in range(max(args.warmup, 1)):
        step()
    fence()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        step()
    fence()
    dt = time.perf_counter() - t0
    if world > 1:
        tt = torch.tensor([dt], device=dev, dtype=torch.float64)
        torch.distributed.all_reduce(tt, op=torch.distributed.ReduceOp.MAX)
        dt = float(tt.item())
    return {
        "metric": "nodes/sec fwd+bwd (get_graph_embeddings, 10M-node power-law graph)", "value": round(n * args.steps / dt, 1),
        "unit": "nodes/s", "n_gpus": world, "steps": args.steps, "warmup": max(args.warmup, 1),
        "ms_per_step": round(dt / args.steps * 1e3, 2), "higher_is_better": True, "scaling": "strong", "vs_baseline": None,
        "dtype": "bf16", "data": "synthetic",
        "config": {"workload": f"s5: Chung-Lu power-law graph N={n} E={e} F_in={f_in}, hidden_channels={args.s5_hc}, P=768, R_a={r_a}, "
                               f"get_graph_embeddings forward+backward with activation checkpointing and reference dropout",
                   "global_nodes": n, "parallelism": f"1-D node partition x{world}" if world > 1 else "single GPU",
                   "rows_per_rank": hi - lo, "halo_rows_rank0": halo, "activation_checkpointing": True,
                   "partition": (f"shard files ({pdir}): rank 0 plans and writes once ({t_part:.1f} s incl. barrier), every rank loads its own" if world > 1 else None),
                   "preflight_mem_estimate_GB": round(est / 1e9, 1),
                   "world": world, "backend": (torch.distributed.get_backend() if world > 1 else None), "devices": device_names(dev, world),
                   "peak_mem_GB": round(torch.cuda.max_memory_allocated() / 1e9, 1)}}


DUMP_SAMPLE = 32768              # elements kept per gradient tensor (seeded, fixed positions); 269 tensors -> < 35 MB in all


def dump_outputs(out_dir, loss, logits, model):
    """What the last timed step hands its caller, as float32 .npy files: ``loss`` (0-d), ``logits`` [local nodes, C] and one
    ``grad.<parameter name>.npy`` per parameter that has a gradient: the whole gradient up to DUMP_SAMPLE elements, else
    DUMP_SAMPLE elements of the flattened gradient at sorted positions drawn from a generator seeded with crc32(name), i.e.
    the same positions in every run and every build."""
    import zlib

    import numpy as np
    os.makedirs(out_dir, exist_ok=True)
    files = {"loss": loss.detach().float().reshape(()), "logits": logits.detach().float()}
    for name, p in model.named_parameters():
        if p.grad is None:
            continue
        g = p.grad.detach().reshape(-1)
        if g.numel() > DUMP_SAMPLE:
            gen = torch.Generator().manual_seed(zlib.crc32(name.encode()))
            idx = torch.randint(0, g.numel(), (DUMP_SAMPLE,), generator=gen).sort().values
            g = g[idx.to(g.device)]
        files["grad." + name] = g.float()
    for name, t in files.items():
        np.save(os.path.join(out_dir, name + ".npy"), t.cpu().numpy())
    return len(files)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--workload", default="squirrel", choices=list(WORKLOADS) + ["s5"])
    ap.add_argument("--s5-nodes", type=int, default=10_000_000)
    ap.add_argument("--s5-edges", type=int, default=100_000_000)
    ap.add_argument("--s5-hc", type=int, default=96, help="hidden_channels of the s5 GNN run (F_in = P = 768; 96 keeps the 10M-node activations on ONE GPU for the N=1 point; "
                    "768 = BASELINE's h is meant for >= 8 GPUs: a pre-flight per-rank memory estimate decides collectively whether the step is run)")
    ap.add_argument("--partition-dir", default=None, help="s5: read this rank's shard (gmlm_amd.dist.write_partition_files) instead of planning from the edge list")
    ap.add_argument("--plm-ckpt", action="store_true", help="HF-style gradient checkpointing of the text encoder (reference: main.py:217-218)")
    ap.add_argument("--reference-recompute", action="store_true", help="activation checkpointing of the RGCN blocks AND of the BertLayers, as the reference runs (main.py:217-219, 278-314)")
    ap.add_argument("--no-fp32-leg", action="store_true")
    ap.add_argument("--no-gemm-tuning", action="store_true", help="library default GEMM algorithms instead of the looked-up picks (gmlm_amd/tuning.py)")
    ap.add_argument("--gemm-tune", default=None, metavar="CSV", help="time the library's GEMM candidates for every shape of this run and write the picks to CSV (offline step)")
    ap.add_argument("--gemm-tune-rotate", type=int, default=None, metavar="MB", help="with --gemm-tune: rotate the operands through a buffer of this size (cold-cache timing)")
    ap.add_argument("--gemm-picks", default=None, metavar="CSV", help="look up this results file instead of gmlm_amd/tunable/gfx950.csv")
    ap.add_argument("--no-hip-graph", action="store_true", help="cornell / chameleon: run eagerly (they replay hipGraphs by default)")
    ap.add_argument("--hip-graph", action="store_true", help="replay the static-shape regions (GNN blocks, cross-attention + head) from hipGraphs: for the launch-bound small workloads")
    ap.add_argument("--ring", action="store_true", help="N > 1: CrossAttention through the ring K|V exchange instead of the K|V all-gather")
    ap.add_argument("--no-ring", action="store_true")
    ap.add_argument("--cpu-repeats", type=int, default=3)
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "f32"])
    ap.add_argument("--hc", type=int, default=None, help="hidden_channels (default per workload: 768; chameleon 256, cornell 512)")
    ap.add_argument("--plm-hidden", type=int, default=None, help="text encoder width (default 768 = BERT-base; chameleon 256 = BERT-mini)")
    ap.add_argument("--plm-layers", type=int, default=None, help="text encoder depth (default 12; chameleon 4)")
    ap.add_argument("--vocab", type=int, default=30522)
    ap.add_argument("--max-len", type=int, default=128)
    ap.add_argument("--plm-batch", type=int, default=4096, help="text micro-batch (nodes); default = all active nodes in ONE packed batch")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--cpu-plm-sample", type=int, default=64)
    ap.add_argument("--cpu-hc", type=int, default=768)
    ap.add_argument("--no-encoder-graph", action="store_true", help="with hipGraphs: leave the text encoder eager (GNN + head regions only)")
    ap.add_argument("--overlap-streams", action="store_true", help="text encoder on a second HIP stream beside the GNN (model.overlap_streams)")
    ap.add_argument("--concurrent-graphs", action="store_true", help="with hipGraphs: replay the (linear) GNN and encoder recordings on two streams at once")
    ap.add_argument("--whole-step-graph", action="store_true", help="(default with hipGraphs) ONE graph per step with the encoder and GNN branches side by side")
    ap.add_argument("--linear-graphs", action="store_true", help="with hipGraphs: three linear recordings (GNN, encoder per size bucket, head) instead of the whole-step graph")
    ap.add_argument("--host-profile", default=None, metavar="FILE", help="cProfile the timed steps (host side) and write the top entries to FILE")
    ap.add_argument("--no-kernel-timers", action="store_true")
    ap.add_argument("--no-micro", action="store_true", help="skip the kernel micro-benchmarks (rank 0, N=1 only)")
    ap.add_argument("--backend", default="nccl", help="torch.distributed backend (gloo = 1-GPU rehearsal of the N>1 path)")
    ap.add_argument("--micro-only", action="store_true")
    ap.add_argument("--gnn-large", action="store_true", help="GNN-only step on a 1.25M-node S5 shard (single GPU)")
    ap.add_argument("--micro-select", default="spmm,attn", help="comma list of micro-benchmark groups: spmm, attn")
    ap.add_argument("--micro-nodes", type=int, default=1_250_000)
    ap.add_argument("--micro-edges", type=int, default=12_500_000)
    ap.add_argument("--full", action="store_true", help="also the per-kernel, micro-benchmark / roofline, fp32, reference_recompute, "
                    "power_law_variant and cpu_baseline legs (a plain run times the headline step only)")
    ap.add_argument("--dump-outputs", default=None, metavar="DIR", help="after the timed steps, write the last step's loss, logits and "
                    "(sampled) parameter gradients to DIR/<name>.npy (float32)")
    args = ap.parse_args()
    if args.dump_outputs and (args.gnn_large or args.micro_only or args.workload == "s5"):
        raise SystemExit("--dump-outputs writes the GraphTextLM step's outputs: not with --gnn-large, --micro-only or --workload s5")

    import gmlm_amd
    from gmlm_amd import ops, tuning

    gemm_tuning = False
    if args.gemm_tune:
        gemm_tuning = tuning.enable_gemm_tuning(args.gemm_tune, tune=True, rotating_buffer_mb=args.gemm_tune_rotate)
    elif not args.no_gemm_tuning:
        try:
            gemm_tuning = tuning.enable_gemm_tuning(args.gemm_picks)
        except Exception as exc:        # the look-up is an optimisation: never a reason to lose the bench line
            print(f"[bench] GEMM pick look-up unavailable ({exc!r}): library default algorithms", file=sys.stderr)
            tuning.disable_gemm_tuning()
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if args.gpus > 1 and world != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} needs torch.distributed.run with --nproc-per-node {args.gpus} (WORLD_SIZE={world})")
    local_rank = local_rank % max(torch.cuda.device_count(), 1)     # gloo rehearsal: several ranks on one GPU
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    distributed = world > 1
    if distributed:
        import torch.distributed as dist
        if args.backend == "nccl":
            dist.init_process_group("nccl", device_id=dev)
        else:
            dist.init_process_group(args.backend)

    # per-workload geometry (BASELINE.json configs): Chameleon-size is quoted with BERT-mini (256 x 4, 4 heads) and hc 256,
    # Cornell-size with BERT-base and hc 512, everything else with BERT-base and hc 768
    preset = {"chameleon": (256, 256, 4), "cornell": (512, 768, 12)}.get(args.workload, (768, 768, 12))
    args.hc = preset[0] if args.hc is None else args.hc
    args.plm_hidden = preset[1] if args.plm_hidden is None else args.plm_hidden
    args.plm_layers = preset[2] if args.plm_layers is None else args.plm_layers
    if args.gnn_large:
        print(json.dumps({"gnn_large": gnn_large(dev, args)}))
        return
    if args.micro_only:
        print(json.dumps({"micro": micro(dev, args)}))
        return
    if args.workload == "s5":
        line = s5_strong(dev, args, world, rank)
        if rank == 0:
            print(json.dumps(line))
        if distributed:
            torch.distributed.destroy_process_group()
        return
    # arxiv is one fixed graph that the ranks share (node partition of the SAME graph: strong scaling); the small
    # graphs keep one Squirrel-size partition per rank (weak scaling, as the contract's default N > 1 run)
    strong = args.workload == "arxiv"
    data = synthetic(args.workload, n_parts=1 if strong else world)
    ids, am = synthetic_tokens(data["n"], args.max_len, args.vocab, seed=data["n"])
    model = build_model(args, data, dev)
    if distributed:
        from gmlm_amd.dist import attach_partition
        part = attach_partition(model, data["edge_index"], data["n"], dev)
        part.use_ring = args.ring or (args.workload == "arxiv" and not args.no_ring)   # K|V stays distributed (ring) on the large graph
        lo, hi = part.plan.lo, part.plan.hi
    else:
        part, lo, hi = None, 0, data["n"]
    devices = device_names(dev, world)
    x = data["x"][lo:hi].to(dev)
    y = data["y"][lo:hi].to(dev)
    active = data["active"][lo:hi].to(dev)
    ei = data["edge_index"].to(dev)
    tokens = gmlm_amd.TokenizedTexts.from_mask(ids[lo:hi].to(dev), am[lo:hi].to(dev))
    n_active_total = int(data["active"].sum())
    if args.workload in ("cornell", "chameleon") and not distributed and not args.no_hip_graph:
        args.hip_graph = True                        # the launch-bound small workloads replay their static regions by default
    if args.hip_graph:
        if distributed:
            raise SystemExit("--hip-graph is single-GPU")
        args.whole_step_graph = not (args.linear_graphs or args.concurrent_graphs or args.no_encoder_graph)
        model.capture_hip_graphs(model.soft_mask_input(x, active, 0.7), ei, encoder=not args.no_encoder_graph,
                                 whole_step=args.whole_step_graph, concurrent=args.concurrent_graphs)

    def step():
        model.zero_grad(set_to_none=True)
        xm = model.soft_mask_input(x, active, 0.7)
        logits = model(xm, ei, tokens, active, plm_batch_size=args.plm_batch)
        idx = model.active_index                     # the forward's own active-node index (no second mask -> index sync)
        if idx is None:                              # a rank without a local active node still runs backward (its peers wait in the collectives)
            loss = logits.sum() * 0.0
        else:
            loss = F.cross_entropy(logits.index_select(0, idx), y.index_select(0, idx), label_smoothing=0.2,
                                   reduction="sum") / n_active_total
        if part is not None:
            part.grad_buckets(model).prepare()       # gradients as views of flat buckets: all-reduced under backward, no copies
        loss.backward()
        if part is not None:
            part.grad_buckets(model).finish()
        return loss, logits

    def fence():
        if distributed:
            torch.distributed.barrier()
        torch.cuda.synchronize()

    for _ in range(args.warmup):
        step()
    fence()
    prof = None
    if args.host_profile:                                # where a launch-bound step spends its HOST time (not a bench number)
        import cProfile
        prof = cProfile.Profile()
        prof.enable()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        loss, logits = step()
    fence()
    dt = time.perf_counter() - t0
    if prof is not None:
        import io
        import pstats
        prof.disable()
        buf = io.StringIO()
        pstats.Stats(prof, stream=buf).sort_stats("tottime").print_stats(45)
        with open(args.host_profile, "w") as f:
            f.write(f"{args.steps} steps, {dt / args.steps * 1e3:.3f} ms/step under cProfile\n" + buf.getvalue())
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, loss, logits, model)
    del logits
    timer = None
    if args.full and not args.no_kernel_timers:
        # per-kernel figures: K more steps with HIP events around every hand-written launch (the events cost host time, so
        # they stay out of the timed steps above)
        timer = ops.KernelTimer()
        ops.TIMER = timer
        for _ in range(args.steps):
            step()
        fence()
        ops.TIMER = None
    if distributed:
        tt = torch.tensor([dt], device=dev, dtype=torch.float64)
        torch.distributed.all_reduce(tt, op=torch.distributed.ReduceOp.MAX)
        dt = float(tt.item())
    ms_per_step = dt / args.steps * 1e3
    value = data["n"] * args.steps / dt

    out = {
        "metric": "nodes/sec fwd+bwd (full-batch GraphTextLM step)", "value": round(value, 2), "unit": "nodes/s",
        "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(ms_per_step, 3),
        "higher_is_better": True, "scaling": "strong" if strong else "weak", "vs_baseline": None, "dtype": args.dtype, "data": "synthetic",
        "config": {"workload": f"{args.workload}-size synthetic graph x{1 if strong else world} (N={data['n']}, E={data['e']}, F_in={data['f_in']}), "
                               f"hidden_channels={args.hc}, BERT geometry {args.plm_hidden}x{args.plm_layers}, "
                               f"{n_active_total} active text nodes, 16..{args.max_len} tokens, plm_batch_size={args.plm_batch}",
                   "global_nodes": data["n"], "parallelism": f"1-D node partition x{world}" if distributed else "single GPU",
                   "activation_checkpointing": bool(recompute_flags(args)[0]), "plm_gradient_checkpointing": bool(recompute_flags(args)[1]),
                   "recompute_note": "the reference recomputes RGCN blocks and BertLayers in backward (main.py:217-219, 278-314); this line runs "
                                     + ("WITH both, like the reference" if all(recompute_flags(args)) else "WITHOUT recomputation (same results; the reference-mode time is in reference_recompute)"),
                   "world": world, "backend": (torch.distributed.get_backend() if distributed else None), "devices": devices,
                   "hip_graph": ("whole-step graph with parallel branches" if args.whole_step_graph else "three linear recordings (GNN, text encoder per size bucket, head)"
                                 + (", GNN and encoder replayed on two streams at once" if args.concurrent_graphs else "")) if args.hip_graph else False,
                   "gemm_algorithms": ("library picks from gmlm_amd/tunable/gfx950.csv (TunableOp lookup)" if gemm_tuning and not args.gemm_tune
                                       else "tuned in this run" if gemm_tuning else "library default heuristic"),
                   "loss": round(float(loss.detach()), 5)},
    }
    if rank == 0 and timer is not None:
        summ = timer.summary()
        kern = {}
        for name, d in summ.items():
            ms = d["ms"] / max(d["launches"], 1)
            k = {"launches_per_step": d["launches"] / args.steps, "avg_ms": round(ms, 4)}
            if d["bytes"]:
                k["algorithmic_GBps"] = round(d["bytes"] / d["ms"] / 1e6, 1)
                k["frac_hbm_peak"] = round(d["bytes"] / d["ms"] / 1e6 / HBM_PEAK_GBS, 4)
            if d["flops"]:
                peak = MFMA_BF16_PEAK_TF if args.dtype == "bf16" else MFMA_F32_PEAK_TF
                k["TFLOPs"] = round(d["flops"] / d["ms"] / 1e9, 2)
                k["frac_mfma_peak"] = round(d["flops"] / d["ms"] / 1e9 / peak, 4)
            kern[name] = k
        sp_in = kern.get("spmm_fwd")
        if sp_in is not None and world == 1:
            # in-step aggregation: X is 8-32 MB, i.e. L2 / Infinity-Cache resident, so the algorithmic-byte rate is not
            # an HBM fraction.  Bound: the guide's gather rates for rows served from L2 (16.8-18.8 TB/s chip-wide) and
            # from the Infinity Cache (8.6 TB/s); counter traffic = what actually left L2 (profiles/).
            sp_in.pop("frac_hbm_peak", None)
            sp_in.update({"regime": "cache-resident X (8-32 MB): reported against the L2 / Infinity-Cache gather rate, not HBM",
                          "bound": "l2/mall", "peak_GBps": 17000.0, "frac_l2_gather_rate": round(sp_in["algorithmic_GBps"] / 17000.0, 4),
                          "pmc_hbm_side_bytes_per_launch": _pmc_traffic("spmm_fwd_in_step")})
        sp_bw = kern.get("spmm_bwd")
        if sp_bw is not None and world == 1:
            sp_bw.pop("frac_hbm_peak", None)
            sp_bw.update({"regime": "cache-resident dH (8-32 MB): reported against the L2 / Infinity-Cache gather rate, not HBM",
                          "bound": "l2/mall", "peak_GBps": 17000.0, "frac_l2_gather_rate": round(sp_bw["algorithmic_GBps"] / 17000.0, 4)})
        for nm in ("attn_fwd_d64", "attn_bwd_d64"):
            k = kern.get(nm)
            if k is not None and "algorithmic_GBps" in k and args.max_len <= 128:
                # sequences of <= 128 tokens: 4 L d flops per 8 d bytes of q, k, v, o = L / 2 <= 64 flop/B, far below the ridge
                # (2.5 PF / 8 TB/s = 312): these launches are priced against HBM, not MFMA
                k["bound"] = "hbm"
                k["note"] = ("text-encoder attention at <= 128 tokens per sequence: <= 64 flop per byte of q/k/v/o, a fifth of the MFMA/HBM "
                             "ridge (312): HBM-side kernel; frac_mfma_peak is reported for completeness only")
        out["kernels"] = kern
    if args.full and rank == 0 and world == 1 and not args.no_micro and args.workload == "squirrel":
        del model
        torch.cuda.empty_cache()
        out["micro"] = mi = micro(dev, args)
        # the HBM roofline binds only when the feature matrix is far larger than the 256 MiB Infinity Cache: that
        # launch IS the roofline object
        sp = mi.get("spmm_fwd_bf16")
        if sp:
            out["roofline"] = {
                "kernel": "seg_reduce_vec_kernel (RGCN mean aggregation, forward) on a %d-node / %d-edge power-law shard, F=768 bf16, R_a=%d"
                          % (sp["nodes"], sp["edges"], sp["r_active"]),
                "bound": "hbm", "achieved": sp["GBps"], "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": sp["frac_hbm_peak"],
                "traffic": _pmc_traffic("spmm_fwd_bf16"), "algorithmic_bytes_per_launch": int(sp["algorithmic_GB"] * 1e9),
                "avg_launch_ms": sp["avg_ms"],
                "backward": {k: mi["spmm_bwd_bf16"][k] for k in ("avg_ms", "algorithmic_GB", "GBps", "frac_hbm_peak")} if "spmm_bwd_bf16" in mi else None}
        xa, mh = mi.get("xattn_N20804"), mi.get("mha_L512")
        if xa and mh:
            out["attention"] = {
                "bound": "mfma", "peak": MFMA_BF16_PEAK_TF, "unit": "TFLOP/s",
                "cross_attention_fwd": {"kernel": "attn_fwd_pipe_kernel<96, 8> (h=8, d=96, N=20,804, no mask: padded = executed flops)",
                                        "achieved": xa["fwd_TFLOPs"], "frac": xa["fwd_frac_mfma_peak"], "avg_launch_ms": xa["fwd_ms"],
                                        "pmc": _pmc_attn("attn_fwd_pipe_kernel<96, 8", 82 * 8 * 512)},
                "cross_attention_bwd": {"kernel": "attn_delta + attn_bwd_dq_pipe<96, 8> + attn_bwd_dkv_pipe<96, 8> (10 B h L^2 d convention; 14 executed: S is recomputed in both)",
                                        "achieved": xa["bwd_TFLOPs"], "frac": xa["bwd_frac_mfma_peak"], "avg_launch_ms": xa["bwd_ms"],
                                        "executed_TFLOPs": round(xa["bwd_TFLOPs"] * 1.4, 1),
                                        "pmc_dq": _pmc_attn("attn_bwd_dq_pipe_kernel<96, 8", 82 * 8 * 512),
                                        "pmc_dkv": _pmc_attn("attn_bwd_dkv_pipe_kernel<96, 8", 82 * 8 * 512)},
                "masked_mha_fwd": {"kernel": "attn_fwd_pipe_kernel<64, 4> (B=32, h=12, L=512, d=64, kv_len ~ U[256,512])",
                                   "achieved_padded": mh["fwd_TFLOPs"], "frac_padded": mh["fwd_frac_mfma_peak"],
                                   "achieved_executed": mh.get("fwd_TFLOPs_executed"), "avg_launch_ms": mh["fwd_ms"],
                                   "note": "100 MB of q/k/v/o for 18 GF executed: this shape sits at the HBM/MFMA ridge (257 flop/B vs 312)",
                                   "pmc": _pmc_attn("attn_fwd_pipe_kernel<64, 4", 4 * 384 * 256)}}
            ml = mi.get("mha_L2048")
            if ml:
                # the same kernel where masked attention at h = 768 is MFMA-bound: L / 2 = 1,024 flop per byte of q/k/v/o
                out["attention"]["masked_mha_fwd_L2048"] = {
                    "kernel": "attn_fwd_pipe_kernel<64, 4> (B=16, h=12, L=2048, d=64, kv_len ~ U[1024,2048])",
                    "achieved_padded": ml["fwd_TFLOPs"], "frac_padded": ml["fwd_frac_mfma_peak"],
                    "achieved_executed": ml.get("fwd_TFLOPs_executed"), "avg_launch_ms": ml["fwd_ms"],
                    "pmc": _pmc_attn("attn_fwd_pipe_kernel<64, 4", 16 * 12 * 16 * 256)}
    if args.full and rank == 0 and world == 1 and not args.no_fp32_leg and args.dtype == "bf16" and args.workload == "squirrel":
        # the same step with fp32 operands (the dtype the 1e-4 parity bar is stated in)
        args32 = argparse.Namespace(**{**vars(args), "dtype": "f32"})
        m32 = build_model(args32, data, dev)

        def step32():
            m32.zero_grad(set_to_none=True)
            lg = m32(m32.soft_mask_input(x, active, 0.7), ei, tokens, active, plm_batch_size=args.plm_batch)
            idx = m32.active_index
            (F.cross_entropy(lg.index_select(0, idx), y.index_select(0, idx), label_smoothing=0.2, reduction="sum") / n_active_total).backward()

        step32()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(3):
            step32()
        torch.cuda.synchronize()
        d32 = (time.perf_counter() - t0) / 3
        out["fp32"] = {"ms_per_step": round(d32 * 1e3, 2), "value": round(data["n"] / d32, 1), "unit": "nodes/s", "steps": 3,
                       "note": "same workload, fp32 operands (exact-f32 MFMA attention, fp32 GEMMs)"}
        del m32
        torch.cuda.empty_cache()
    if args.full and rank == 0 and world == 1 and not args.no_fp32_leg and args.dtype == "bf16" and args.workload == "squirrel" and not args.reference_recompute:
        # the same step the way the reference runs it: every RGCN block and every BertLayer recomputed in backward
        argsr = argparse.Namespace(**{**vars(args), "reference_recompute": True})
        mr = build_model(argsr, data, dev)

        def step_r():
            mr.zero_grad(set_to_none=True)
            lg = mr(mr.soft_mask_input(x, active, 0.7), ei, tokens, active, plm_batch_size=args.plm_batch)
            idx = mr.active_index
            (F.cross_entropy(lg.index_select(0, idx), y.index_select(0, idx), label_smoothing=0.2, reduction="sum") / n_active_total).backward()

        torch.cuda.reset_peak_memory_stats()
        step_r()
        step_r()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(3):
            step_r()
        torch.cuda.synchronize()
        dr = (time.perf_counter() - t0) / 3
        out["reference_recompute"] = {"ms_per_step": round(dr * 1e3, 2), "value": round(data["n"] / dr, 1), "unit": "nodes/s", "steps": 3,
                                      "activation_checkpointing": True, "plm_gradient_checkpointing": True,
                                      "peak_mem_GB": round(torch.cuda.max_memory_allocated() / 1e9, 2),
                                      "note": "same workload with the reference's recomputation (main.py:217-219, 278-314): identical results, forward of every block runs twice"}
        del mr
        torch.cuda.empty_cache()
    if args.full and rank == 0 and world == 1 and not args.no_fp32_leg and args.dtype == "bf16" and args.workload == "squirrel":
        # the headline graph's uniform edges put every edge in degree bucket 3 (R_a = 1); real Squirrel is heavy-tailed.  Same
        # sizes with Chung-Lu power-law out-degrees (alpha = 2.2): all four degree buckets occur, the relation-segmented
        # aggregation and the one-GEMM H W_cat path run with R_a = 4
        g = torch.Generator().manual_seed(2024)
        w = (torch.arange(data["n"], dtype=torch.float32) + 1.0).pow(-1.0 / 1.2)
        perm = torch.randperm(data["n"], generator=g)
        ei_pl = torch.stack([perm[torch.multinomial(w, data["e"], replacement=True, generator=g)],
                             torch.randint(0, data["n"], (data["e"],), generator=g)]).to(dev)
        mpl = build_model(args, data, dev)

        def step_pl():
            mpl.zero_grad(set_to_none=True)
            lg = mpl(mpl.soft_mask_input(x, active, 0.7), ei_pl, tokens, active, plm_batch_size=args.plm_batch)
            idx = mpl.active_index
            (F.cross_entropy(lg.index_select(0, idx), y.index_select(0, idx), label_smoothing=0.2, reduction="sum") / n_active_total).backward()

        step_pl()
        step_pl()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(3):
            step_pl()
        torch.cuda.synchronize()
        dpl = (time.perf_counter() - t0) / 3
        out["power_law_variant"] = {"ms_per_step": round(dpl * 1e3, 2), "value": round(data["n"] / dpl, 1), "unit": "nodes/s", "steps": 3,
                                    "r_active": int(mpl.graph(ei_pl, data["n"]).r_active),
                                    "note": "same sizes, Chung-Lu power-law out-degrees: all degree buckets occur (the headline graph has R_a = 1)"}
        del mpl, ei_pl
        torch.cuda.empty_cache()
    if args.full and rank == 0 and world == 1 and not args.no_cpu_baseline and data["n"] > 16384:
        # the oracle follows the reference and materialises the [1, 8, N, N] scores of both cross-attentions (main.py:159-160):
        # 918 GB at ogbn-arxiv size - the reference cannot run this workload at all, so there is no CPU leg
        out["cpu_baseline"] = {"value": None, "unit": "nodes/s", "cores": os.cpu_count(), "kind": "port",
                               "sample": f"not run: the dense N x N cross-attention of the reference needs {8 * data['n'] ** 2 * 4 / 1e9:.0f} GB of host memory per module at N = {data['n']}"}
    elif args.full and rank == 0 and world == 1 and not args.no_cpu_baseline:
        try:
            out["cpu_baseline"] = cpu_baseline(args, data, ids, am)
        except Exception as exc:  # the baseline is a reported number, never a reason to lose the bench line
            out["cpu_baseline"] = {"value": None, "unit": "nodes/s", "cores": os.cpu_count(), "kind": "port", "sample": f"failed: {exc!r}"}
    if rank == 0:
        if args.full:
            out["child_processes_at_exit"] = child_processes()
        print(json.dumps(out))
    if distributed:
        torch.distributed.destroy_process_group()


def child_processes():
    """Names of the processes this one has started and not reaped (the bench starts none: [] expected)."""
    try:
        import psutil
        return [c.name() for c in psutil.Process().children(recursive=True)]
    except Exception as exc:          # psutil is part of the image; never a reason to lose the line
        return [f"unknown: {exc!r}"]


if __name__ == "__main__":
    main()
