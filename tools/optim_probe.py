"""The tail of a training iteration, gradient clipping + AdamW, three ways on one device, in one process.

The headline Squirrel model is built with bench.py's own builders (BERT-base encoder, hc 768; fp32 masters), every parameter's
.grad is filled with seeded noise, and three tails run on three builds of it, each with harness.setup_optimizer's three groups:
      stock        clip_grad_norm_ + torch.optim.AdamW (for-each), what harness.train_step runs by default
      torch_fused  clip_grad_norm_ + torch.optim.AdamW(fused=True)
      gmlm_fused   gmlm_amd.FusedAdamW.step(max_grad_norm=1.0): three launches, one pass over the gradients for the norm
Warm-up, then rounds that run the three one after the other, ``--steps`` tails each, host clock around a synchronise; every figure
is a median with its range.  The three kernels of gmlm_fused are also timed by device events (ops.KernelTimer), and their
algorithmic bytes (32 B per parameter + tables) are set beside a device-to-device copy of the same volume in this process and
the project's recorded granule_copy figure.  Writes one JSON file (``--out``) and prints it.  Needs a GPU.

    python tools/optim_probe.py --out profiles/fused_adamw_probe.json
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

GRANULE_COPY_TBS = 5.5      # tools/ubench/granule_copy.hip on MI355X, as recorded in DESIGN.md section 5
LRS = dict(lr_graph=1e-3, lr_bert=1e-5, lr_other=1e-4, weight_decay=0.01)        # harness.train_model's defaults


def stat(xs, digits=4):
    return {"median": round(statistics.median(xs), digits), "min": round(min(xs), digits), "max": round(max(xs), digits)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this probe needs a GPU"
    dev = torch.device("cuda:0")
    import bench
    import gmlm_amd
    from gmlm_amd import harness, ops

    args = argparse.Namespace(vocab=30522, plm_hidden=768, plm_layers=12, max_len=128, hc=768, dtype="bf16", workload="squirrel",
                              reference_recompute=False, plm_ckpt=False, overlap_streams=False, plm_batch=4096)
    data = bench.synthetic("squirrel")
    models = {k: bench.build_model(args, data, dev) for k in ("stock", "torch_fused", "gmlm_fused")}      # same seed, same weights
    base = models["stock"]
    gen = torch.Generator(device=dev).manual_seed(0)
    noise = [torch.randn(p.shape, device=dev, generator=gen) * 1e-2 for p in base.parameters()]      # global norm >> 1: clipped
    for m in models.values():
        for p, g in zip(m.parameters(), noise):
            p.grad = g.clone()
    n_params = sum(p.numel() for p in base.parameters())
    n_tensors = len(noise)
    del noise

    opts = {"stock": harness.setup_optimizer(models["stock"], **LRS),
            "gmlm_fused": harness.setup_optimizer(models["gmlm_fused"], fused=True, **LRS)}
    tf = harness.setup_optimizer(models["torch_fused"], **LRS)
    opts["torch_fused"] = torch.optim.AdamW([dict(params=g["params"], lr=g["lr"], weight_decay=g["weight_decay"]) for g in tf.param_groups],
                                            fused=True)

    def tail(name):
        m, o = models[name], opts[name]
        if name == "gmlm_fused":
            o.step(max_grad_norm=1.0)
        else:
            torch.nn.utils.clip_grad_norm_(m.parameters(), max_norm=1.0)
            o.step()

    order = ["stock", "torch_fused", "gmlm_fused"]
    for name in order:
        for _ in range(a.warmup):
            tail(name)
    torch.cuda.synchronize()
    times = {k: [] for k in order}
    for _ in range(a.rounds):
        for name in order:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.steps):
                tail(name)
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) / a.steps * 1e3)
    ms = {k: stat(v) for k, v in times.items()}

    # the three kernels by device events, one timer per round of `steps` tails
    fo = opts["gmlm_fused"]
    plan = next(iter(fo._plans.values()))
    table_bytes = plan.static.numel() + plan.work.numel() + plan.addr_bytes + 64 * len(fo.param_groups) + 32
    algo_bytes = 32.0 * n_params + table_bytes
    per_kernel = {"adamw_sumsq": [], "adamw_finalize": [], "adamw_update": []}
    for _ in range(a.rounds):
        ops.TIMER = ops.KernelTimer()
        for _ in range(a.steps):
            tail("gmlm_fused")
        summ = ops.TIMER.summary()
        ops.TIMER = None
        for k in per_kernel:
            per_kernel[k].append(summ[k]["ms"] / summ[k]["launches"])
    kernel_ms = {k: stat(v) for k, v in per_kernel.items()}
    three = sum(v["median"] for v in kernel_ms.values())

    # a device-to-device copy of the same volume (half read, half written), same process
    src = torch.empty(int(algo_bytes // 2), dtype=torch.uint8, device=dev)
    dst = torch.empty_like(src)
    copy_ms = []
    for _ in range(a.rounds + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.steps):
            dst.copy_(src)
        e1.record()
        e1.synchronize()
        copy_ms.append(e0.elapsed_time(e1) / a.steps)
    copy_ms = copy_ms[1:]

    out = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__,
           "method": f"one process; {a.warmup} warm-up tails per side, then {a.rounds} alternating rounds of {a.steps} tails, host clock "
                     "around a synchronise; median [min, max]; kernels by device events around every launch; gradients: seeded "
                     "noise, global norm far above max_norm = 1 (the clipped branch)",
           "model": "squirrel headline (bench.py builders): BERT-base encoder, hc 768, fp32 masters, harness.setup_optimizer's three groups",
           "parameters": n_params, "tensors": n_tensors, "chunks": plan.num_chunks, "chunk_elems": gmlm_amd.optim.chunk_elems(),
           "tail_ms": ms,
           "stock_over_gmlm_fused": round(ms["stock"]["median"] / ms["gmlm_fused"]["median"], 2),
           "torch_fused_over_gmlm_fused": round(ms["torch_fused"]["median"] / ms["gmlm_fused"]["median"], 2),
           "gmlm_fused_kernels_ms": kernel_ms, "gmlm_fused_three_kernels_ms": round(three, 4),
           "algorithmic_bytes": algo_bytes, "table_bytes": table_bytes,
           "gmlm_fused_TBs_over_three_kernels": round(algo_bytes / three / 1e9, 2),
           "update_kernel_TBs_28B_per_parameter": round(28.0 * n_params / kernel_ms["adamw_update"]["median"] / 1e9, 2),
           "sumsq_kernel_TBs_4B_per_parameter": round(4.0 * n_params / kernel_ms["adamw_sumsq"]["median"] / 1e9, 2),
           "copy_same_volume_ms": stat(copy_ms), "copy_same_volume_TBs": round(algo_bytes / statistics.median(copy_ms) / 1e9, 2),
           "granule_copy_TBs_recorded": GRANULE_COPY_TBS,
           "grad_norm_last_step": float(fo.last_grad_norm), "skipped_steps": fo.skipped_steps()}
    text = json.dumps(out, indent=1)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
