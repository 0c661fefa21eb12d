"""Probe: what the wide-encoder kernels cost (attn_wide.hip, norm_wide.hip).  Throughput was not their target; this records it.

One process.  Every shape is warmed up first, then five rounds alternate the sides; each figure is the median with
[min, max] over the rounds, by device events.
 (a) CrossAttention geometry, h = 8, one sequence of N = 5,201 nodes: forward and forward + backward, bf16 and fp32, head dims
     256 / 384 / 512, dropout 0 and 0.1; beside them the d = 128 kernels (attn_d128.hip) at the same N in the same process, and
     their time scaled by D / 128 as the reference line (the arithmetic grows with D, nothing else does).
 (b) wide LayerNorm forward and backward at 5,201 x 2,560 and 5,201 x 4,096 through the C entry points on preallocated
     buffers, as TB/s of the bytes the kernel must move (x, y / dy, x, dx), beside a ``copy_`` of the same byte volume.

    python tools/attn_wide_probe.py profiles/attn_wide_probe.json"""
import ctypes as C
import json
import statistics
import sys

import torch

sys.path.insert(0, ".")
from gmlm_amd import ops  # noqa: E402
from gmlm_amd._lib import BF16, F32, check, lib  # noqa: E402

dev = torch.device("cuda")
N, H, ROUNDS = 5201, 8, 5


def events(fn, n=3):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(n):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / n * 1e3                     # us


def alternate(sides, n=3):
    """{name: fn} -> {name: [median, min, max]} in us: a warm-up of every side, then ROUNDS rounds that visit the sides in turn."""
    for fn in sides.values():
        for _ in range(2):
            fn()
    got = {k: [] for k in sides}
    for _ in range(ROUNDS):
        for k, fn in sides.items():
            got[k].append(events(fn, n))
    return {k: [round(statistics.median(v), 1), round(min(v), 1), round(max(v), 1)] for k, v in got.items()}


def attention_sides(dtype, p):
    sides = {}
    for d in (128, 256, 384, 512):
        g = torch.Generator().manual_seed(d)
        q, k, v, go = (torch.randn(1, N, H * d, generator=g).to(dev, dtype) for _ in range(4))
        q.requires_grad_(True), k.requires_grad_(True), v.requires_grad_(True)

        def fwd(q=q, k=k, v=v, d=d):
            with torch.no_grad():
                return ops.Attention.apply(q, k, v, None, H, d ** -0.5, p, 1234)

        def both(q=q, k=k, v=v, go=go, d=d):
            out = ops.Attention.apply(q, k, v, None, H, d ** -0.5, p, 1234)
            torch.autograd.grad(out, (q, k, v), go)

        sides[f"d{d}_fwd"], sides[f"d{d}_fwd_bwd"] = fwd, both
    return sides


def attention():
    res = {}
    for dtype, tn in ((torch.bfloat16, "bf16"), (torch.float32, "fp32")):
        for p in (0.0, 0.1):
            t = alternate(attention_sides(dtype, p))
            row = {}
            for d in (256, 384, 512):
                for what in ("fwd", "fwd_bwd"):
                    base = t[f"d128_{what}"][0]
                    row[f"d{d}_{what}"] = dict(us=t[f"d{d}_{what}"], d128_us=t[f"d128_{what}"], d128_scaled_us=round(base * d / 128, 1),
                                               ratio_to_scaled=round(t[f"d{d}_{what}"][0] / (base * d / 128), 2))
            res[f"{tn}_p{p}"] = row
            print(tn, p, json.dumps(row), flush=True)
    return res


def layernorm():
    res = {}
    ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    for f in (2560, 4096):
        for dtype, code, tn in ((torch.bfloat16, BF16, "bf16"), (torch.float32, F32, "fp32")):
            x, gy = (torch.randn(N, f, device=dev).to(dtype) for _ in range(2))
            y, dx = torch.empty_like(x), torch.empty_like(x)
            gamma, beta = torch.ones(f, device=dev), torch.zeros(f, device=dev)
            mean, rstd = torch.empty(N, device=dev), torch.empty(N, device=dev)
            dg, db = torch.empty(f, device=dev), torch.empty(f, device=dev)
            ws = torch.empty(lib().gmlm_bias_res_layernorm_wide_bwd_workspace_bytes(N, f), dtype=torch.uint8, device=dev)
            stream = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)
            fwd = lambda: check(lib().gmlm_bias_res_layernorm_wide_fwd(ptr(x), None, None, ptr(gamma), ptr(beta), N, f, 1e-5, 0, 0.0, 0,
                                                                       None, ptr(y), ptr(mean), ptr(rstd), code, stream()), "fwd")
            bwd = lambda: check(lib().gmlm_bias_res_layernorm_wide_bwd(ptr(gy), ptr(x), None, None, ptr(gamma), ptr(beta), ptr(mean),
                                                                       ptr(rstd), N, f, 0, 0.0, 0, None, ptr(dx), None, ptr(dg), ptr(db),
                                                                       None, code, ptr(ws), ws.numel(), stream()), "bwd")
            nb = x.numel() * x.element_size()
            c2 = torch.empty(nb, dtype=torch.uint8, device=dev), torch.empty(nb, dtype=torch.uint8, device=dev)           # moves 2 nb
            c3 = torch.empty(nb * 3 // 2, dtype=torch.uint8, device=dev), torch.empty(nb * 3 // 2, dtype=torch.uint8, device=dev)   # 3 nb
            t = alternate(dict(fwd=fwd, bwd=bwd, copy2=lambda: c2[0].copy_(c2[1]), copy3=lambda: c3[0].copy_(c3[1])), n=10)
            tb = lambda nbytes, us: round(nbytes / (us * 1e-6) / 1e12, 2)
            res[f"{N}x{f}_{tn}"] = dict(fwd_us=t["fwd"], fwd_TBps=tb(2 * nb, t["fwd"][0]), copy_same_bytes_TBps=tb(2 * nb, t["copy2"][0]),
                                        bwd_us=t["bwd"], bwd_TBps=tb(3 * nb, t["bwd"][0]), copy_same_bytes_bwd_TBps=tb(3 * nb, t["copy3"][0]))
            print(f, tn, json.dumps(res[f"{N}x{f}_{tn}"]), flush=True)
    return res


def main():
    out = dict(what="wide-encoder kernels: median [min, max] us over five alternating rounds, device events, one process",
               device=torch.cuda.get_device_name(0), N=N, heads=H, attention=attention(), layernorm=layernorm())
    with open(sys.argv[1], "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
