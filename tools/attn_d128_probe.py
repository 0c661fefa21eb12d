"""Probe: the head-dim-128 attention kernels (gmlm_attention_d128_*) at the CrossAttention shape of a 1024-wide text encoder
(one sequence of N nodes, 8 heads x 128), bf16, with and without dropout.

Prints one line per case: forward time, backward time (a forward + backward call minus the forward) and the matrix rate."""
import json
import sys

import torch

sys.path.insert(0, ".")
from gmlm_amd import ops  # noqa: E402

dev = torch.device("cuda")


def ev(fn, n=10):
    for _ in range(3):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(n):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / n * 1e3                     # us


def cross(n, p, h=8, d=128):
    g = torch.Generator().manual_seed(n)
    q, k, v = (torch.randn(1, n, h * d, generator=g).to(dev, torch.bfloat16).requires_grad_(True) for _ in range(3))
    go = torch.randn(1, n, h * d, generator=g).to(dev, torch.bfloat16)
    fwd = lambda: ops.Attention.apply(q, k, v, None, h, d ** -0.5, p, 7)

    def fb():
        q.grad = k.grad = v.grad = None
        fwd().backward(go)
    tf = ev(fwd)
    tb = ev(fb) - tf
    fl = 4.0 * h * n * n * d
    return dict(case=f"cross N={n} h={h} d={d} p={p}", fwd_us=round(tf, 1), bwd_us=round(tb, 1),
                fwd_tflops=round(fl / tf / 1e6, 1), bwd_tflops=round(2.5 * fl / tb / 1e6, 1))


if __name__ == "__main__":
    rows = [cross(n, p) for n in (2277, 5201, 20804) for p in (0.0, 0.1)]
    for r in rows:
        print(json.dumps(r), flush=True)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            json.dump(rows, f, indent=1)
