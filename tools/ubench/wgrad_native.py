"""Weight-gradient GEMM of the BERT shapes: the native split-K kernel (ops.wgrad_bf16, dense.NATIVE_WGRAD = True) against the
library path (batched hipBLASLt GEMM with fp32 output + slice sum, dense.NATIVE_WGRAD = False), random bf16 operands, through
dense._splitk_wgrad.  usage: [T=tokens] [GEOMETRY=base|mini] [SPLITS=s,s,...] [NO_REMAP=1] [ONE_PHASE=1] [AB=rounds]
python tools/ubench/wgrad_native.py
SPLITS / NO_REMAP / ONE_PHASE time the native kernel alone at other slice counts / without the XCD grouping / with the
one-barrier main loop (ops.wgrad_bf16 direct).  AB=r skips the library comparison and alternates the two main-loop schedules
instead, r rounds of ONE_PHASE / default per shape in this one process at the default plan, every run printed."""
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
from gmlm_amd import dense, ops  # noqa: E402

dev = torch.device("cuda")
T = int(os.environ.get("T", "91712"))
SPLITS = [int(v) for v in os.environ.get("SPLITS", "").split(",") if v]
FLAGS = (ops.WGRAD_NO_REMAP if os.environ.get("NO_REMAP") else 0) | (ops.WGRAD_ONE_PHASE if os.environ.get("ONE_PHASE") else 0)
AB = int(os.environ.get("AB", "0"))
SHAPES = {"base": (("qkv", 2304, 768), ("o", 768, 768), ("ffn1", 3072, 768), ("ffn2", 768, 3072)),
          "mini": (("qkv", 768, 256), ("o", 256, 256), ("ffn1", 1024, 256), ("ffn2", 256, 1024))}[os.environ.get("GEOMETRY", "base")]


def timeit(f, n=20):
    for _ in range(3):
        f()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        f()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n * 1e3


def run(native):
    dense.NATIVE_WGRAD = native
    return timeit(lambda: dense._splitk_wgrad(dy, x, keep_fp32=True))


for name, n, k in SHAPES:
    g = torch.Generator(device=dev).manual_seed(n + k)
    dy = torch.randn(T, n, device=dev, generator=g).bfloat16()
    x = torch.randn(T, k, device=dev, generator=g).bfloat16()
    fl = 2.0 * T * n * k
    if AB:
        base = FLAGS & ~ops.WGRAD_ONE_PHASE
        assert torch.equal(ops.wgrad_bf16(dy, x, flags=base), ops.wgrad_bf16(dy, x, flags=base | ops.WGRAD_ONE_PHASE))
        one, two = [], []
        timeit(lambda: ops.wgrad_bf16(dy, x, flags=base | ops.WGRAD_ONE_PHASE), 100)    # untimed: clocks and caches settle
        timeit(lambda: ops.wgrad_bf16(dy, x, flags=base), 100)
        for _ in range(AB):
            one.append(timeit(lambda: ops.wgrad_bf16(dy, x, flags=base | ops.WGRAD_ONE_PHASE), 100))
            two.append(timeit(lambda: ops.wgrad_bf16(dy, x, flags=base), 100))
        print(f"{name:5s} {n:5d}x{k:<5d} T={T} flags={base}  one-phase " + " ".join(f"{v:6.1f}" for v in one) + "   default "
              + " ".join(f"{v:6.1f}" for v in two) + f" us   means {sum(one) / AB:6.1f} / {sum(two) / AB:6.1f}"
              f"  x{sum(one) / sum(two):4.2f}  every default run faster: {max(two) < min(one)}", flush=True)
        continue
    dense.NATIVE_WGRAD = True
    out = dense._splitk_wgrad(dy, x, keep_fp32=True)
    exact = dy.double().t() @ x.double()
    bound = (dy.double().abs().t() @ x.double().abs())
    rel = float(((out.double() - exact).abs() / bound).max())
    t_lib, t_nat, t_lib2, t_nat2 = run(False), run(True), run(False), run(True)
    tl, tn = min(t_lib, t_lib2), min(t_nat, t_nat2)
    line = (f"{name:5s} {n:5d}x{k:<5d} T={T}  library {tl:7.1f} us ({fl / tl / 1e6:6.1f} TF/s)   native {tn:7.1f} us "
            f"({fl / tn / 1e6:6.1f} TF/s)  x{tl / tn:4.2f}   max err / sum|dy||x| {rel:.1e}")
    for s in SPLITS:
        ts = timeit(lambda: ops.wgrad_bf16(dy, x, splits=s, flags=FLAGS))
        line += f"\n      S={s:2d} flags={FLAGS}: {ts:7.1f} us ({fl / ts / 1e6:6.1f} TF/s)"
    print(line, flush=True)
dense.NATIVE_WGRAD = True
