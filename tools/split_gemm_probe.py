"""gemm_precision="bf16x3" against native fp32 (and plain bf16, for scale) on one device, in one process.

(a) per shape: the four BERT-base dense layers at T = 91,712 tokens, forward / data gradient / weight gradient each:
      native fp32   torch.mm on fp32 operands (weight gradient: dense._splitk_wgrad, what the fp32 path runs)
      bf16x3        the split of the activation or incoming gradient (gmlm::split3) + ONE depth-3K bf16 GEMM with an fp32 result;
                    the weight gradient reuses the two split buffers as [3T, .] views (no further split).  The weight's own split
                    happens once per step and is listed on its own line
      bf16          the plain bf16 GEMM of the bf16 path
    and the split kernel alone: device events around 20 launches, achieved bytes/s (4 B in + 6 B out per element) beside a
    device-to-device copy_ of the same volume in the same process and the project's recorded granule_copy figure.
(b) the headline Squirrel step, built with bench.py's own builders: ms/step native fp32 against the same model with
    gemm_precision="bf16x3", and the largest logit difference between the two (eval mode, same inputs).
Rounds alternate the sides after warm-up; every figure is a median with its range.  GEMM times: device events around 5
launches; steps: host clock around a synchronise.  Writes one JSON file (``--out``) and prints it.  Needs a GPU.

    python tools/split_gemm_probe.py --out profiles/bf16x3_probe.json
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

GRANULE_COPY_TBS = 5.5      # tools/ubench/granule_copy.hip on MI355X, as recorded in DESIGN.md section 5


def ev_ms(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def stat(xs, digits=4):
    return {"median": round(statistics.median(xs), digits), "min": round(min(xs), digits), "max": round(max(xs), digits)}


def alternate(sides, rounds, reps):
    """sides: {name: fn}.  One warm-up pass of every side, then ``rounds`` rounds that run the sides one after the other."""
    for fn in sides.values():
        ev_ms(fn, 2)
    out = {k: [] for k in sides}
    for _ in range(rounds):
        for k, fn in sides.items():
            out[k].append(ev_ms(fn, reps))
    return {k: stat(v) for k, v in out.items()}


def per_shape(dev, t, rounds):
    from gmlm_amd import dense, ops
    shapes = {"qkv": (2304, 768), "attn_out": (768, 768), "ffn_in": (3072, 768), "ffn_out": (768, 3072)}
    g = torch.Generator(device=dev).manual_seed(0)
    res = {}
    for name, (n, k) in shapes.items():
        x = torch.randn(t, k, device=dev, generator=g)
        w = torch.randn(n, k, device=dev, generator=g) * k ** -0.5
        dy = torch.randn(t, n, device=dev, generator=g)
        xb, wb, dyb = x.bfloat16(), w.bfloat16(), dy.bfloat16()
        sw = dense.SplitWeight(w)
        x1, dy0 = ops.split_bf16x3(x, 1), ops.split_bf16x3(dy, 0)
        f32 = dict(out_dtype=torch.float32)
        r = {"N": n, "K": k, "T": t, "GFLOP": round(2.0 * t * n * k / 1e9, 1)}
        r["forward_ms"] = alternate({"fp32": lambda: torch.mm(x, w.t()),
                                     "bf16x3": lambda: torch.mm(ops.split_bf16x3(x, 1), sw.w0.t(), **f32),
                                     "bf16x3_gemm_only": lambda: torch.mm(x1, sw.w0.t(), **f32),
                                     "bf16": lambda: torch.mm(xb, wb.t())}, rounds, 5)
        r["data_gradient_ms"] = alternate({"fp32": lambda: torch.mm(dy, w),
                                           "bf16x3": lambda: torch.mm(ops.split_bf16x3(dy, 0), sw.w1s, **f32),
                                           "bf16x3_gemm_only": lambda: torch.mm(dy0, sw.w1s, **f32),
                                           "bf16": lambda: torch.mm(dyb, wb)}, rounds, 5)
        v_dy, v_x = dy0.view(3 * t, n), x1.view(3 * t, k)
        r["weight_gradient_ms"] = alternate({"fp32": lambda: dense._splitk_wgrad(dy, x, keep_fp32=True),
                                             "bf16x3": lambda: dense._splitk_wgrad(v_dy, v_x, keep_fp32=True),
                                             "bf16": lambda: dense._splitk_wgrad(dyb, xb, keep_fp32=True)}, rounds, 5)
        r["weight_gradient_on_split_k_kernel"] = bool(dense._native_wgrad_ok(v_dy, v_x, True))
        r["weight_split_both_forms_ms"] = stat([ev_ms(lambda: dense.SplitWeight(w), 5) for _ in range(rounds)])
        tot = {s: sum(r[p][s]["median"] for p in ("forward_ms", "data_gradient_ms", "weight_gradient_ms")) for s in ("fp32", "bf16x3", "bf16")}
        r["three_gemms_ms"] = {s: round(v, 3) for s, v in tot.items()}
        r["fp32_over_bf16x3"] = round(tot["fp32"] / tot["bf16x3"], 2)
        r["bf16x3_over_bf16"] = round(tot["bf16x3"] / tot["bf16"], 2)
        # accuracy on these very operands (relative L2 against float64 of a 2,048-row slice)
        s = slice(0, 2048)
        ref = x[s].double() @ w.double().t()
        rel = lambda a: float((a.double() - ref).norm() / ref.norm())
        r["forward_rel_l2"] = {"fp32": rel(torch.mm(x[s], w.t())), "bf16x3": rel(torch.mm(ops.split_bf16x3(x[s], 1), sw.w0.t(), **f32)),
                               "bf16": rel(torch.mm(xb[s], wb.t(), **f32))}
        res[name] = r
        del x, w, dy, xb, wb, dyb, sw, x1, dy0, v_dy, v_x
        torch.cuda.empty_cache()
    return res


def split_alone(dev, t, rounds):
    from gmlm_amd import ops
    out = {}
    for cols in (768, 3072):
        x = torch.randn(t, cols, device=dev)
        dst = torch.empty(t, 3 * cols, dtype=torch.bfloat16, device=dev)
        nbytes = t * cols * 10.0

        def launch(order=1):
            ops.check(ops.lib().gmlm_split_bf16x3(x.data_ptr(), cols, t, cols, cols, dst.data_ptr(), 3 * cols, cols, order,
                                                  ops._stream()), "gmlm_split_bf16x3")

        # a copy of the same volume: 5 bytes read and 5 bytes written per element
        src8 = torch.empty(int(nbytes // 2), dtype=torch.uint8, device=dev)
        dst8 = torch.empty_like(src8)
        ms = alternate({"split": launch, "copy": lambda: dst8.copy_(src8)}, rounds, 20)
        out[f"{t}x{cols}"] = {"bytes": nbytes, "split_us": {k: round(v * 1e3, 1) for k, v in ms["split"].items()},
                              "split_TBs": round(nbytes / ms["split"]["median"] / 1e9, 2),
                              "copy_same_volume_TBs": round(nbytes / ms["copy"]["median"] / 1e9, 2),
                              "granule_copy_TBs_recorded": GRANULE_COPY_TBS}
        del x, dst, src8, dst8
    return out


def headline(dev, rounds, steps):
    import bench
    import gmlm_amd
    from gmlm_amd import tuning
    args = argparse.Namespace(vocab=30522, plm_hidden=768, plm_layers=12, max_len=128, hc=768, dtype="f32", workload="squirrel",
                              reference_recompute=False, plm_ckpt=False, overlap_streams=False, plm_batch=4096)
    tuned = tuning.enable_gemm_tuning()
    data = bench.synthetic("squirrel")
    ids, am = bench.synthetic_tokens(data["n"], args.max_len, args.vocab, seed=data["n"])
    x, y, active, ei = data["x"].to(dev), data["y"].to(dev), data["active"].to(dev), data["edge_index"].to(dev)
    tokens = gmlm_amd.TokenizedTexts.from_mask(ids.to(dev), am.to(dev))
    n_active = int(data["active"].sum())
    models = {"fp32_native": bench.build_model(args, data, dev), "fp32_bf16x3": bench.build_model(args, data, dev)}
    models["fp32_bf16x3"].gemm_precision = "bf16x3"           # same seed, same weights: only the option differs
    assert all(torch.equal(a, b) for a, b in zip(models["fp32_native"].state_dict().values(), models["fp32_bf16x3"].state_dict().values()))

    def step(m):
        m.zero_grad(set_to_none=True)
        lg = m(m.soft_mask_input(x, active, 0.7), ei, tokens, active, plm_batch_size=args.plm_batch)
        idx = m.active_index
        (F.cross_entropy(lg.index_select(0, idx), y.index_select(0, idx), label_smoothing=0.2, reduction="sum") / n_active).backward()

    logits = {}
    for k, m in models.items():
        m.eval()
        with torch.no_grad():
            logits[k] = m(m.soft_mask_input(x, active, 0.7), ei, tokens, active, plm_batch_size=args.plm_batch).float()
        m.train()
    times = {k: [] for k in models}
    for m in models.values():
        step(m)
        step(m)
    torch.cuda.synchronize()
    for _ in range(rounds):
        for k, m in models.items():
            t0 = time.perf_counter()
            for _ in range(steps):
                step(m)
            torch.cuda.synchronize()
            times[k].append((time.perf_counter() - t0) / steps * 1e3)
    ms = {k: stat(v, 2) for k, v in times.items()}
    tokens_total = int(tokens.lens_host[data["active"]].sum())
    return {"workload": "squirrel, BERT-base, hc 768, fp32 storage, no recomputation, dropout 0.3 (bench.py builders)",
            "active_nodes": n_active, "tokens": tokens_total, "gemm_algorithms": "library picks (TunableOp lookup)" if tuned else "library default",
            "ms_per_step": ms, "steps_per_round": steps, "rounds": rounds,
            "native_over_bf16x3": round(ms["fp32_native"]["median"] / ms["fp32_bf16x3"]["median"], 2),
            "max_abs_logit_difference_eval": float((logits["fp32_native"] - logits["fp32_bf16x3"]).abs().max()),
            "max_abs_logit": float(logits["fp32_native"].abs().max())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--tokens", type=int, default=91712)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--skip", default="", help="comma list of parts to leave out: shapes, split, headline")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this probe needs a GPU"
    dev = torch.device("cuda:0")
    skip = set(a.skip.split(",")) - {""}
    out = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__,
           "method": "one process, warm-up then alternating rounds; median [min, max]; GEMMs and the split kernel by device events "
                     "around 5 / 20 launches, steps by a host clock around a synchronise"}
    if "split" not in skip:
        out["split_kernel"] = split_alone(dev, a.tokens, a.rounds)
    if "shapes" not in skip:
        out["per_shape"] = per_shape(dev, a.tokens, a.rounds)
    if "headline" not in skip:
        out["headline"] = headline(dev, a.rounds, a.steps)
    text = json.dumps(out, indent=1)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
