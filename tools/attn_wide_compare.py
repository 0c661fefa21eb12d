"""Byte comparison of the two wide-head attention families (csrc/attn_wide.hpp: wide::, gqaw::) between two builds of
libgmlm_hip.so, through the operators, on seeded inputs.  One fresh child process per library: the child points
``gmlm_amd._lib.LIB_PATH`` at its library before the first load, runs every case and hands back the sha256 of out, lse, dq, dk
and dv (and, for the grouped family, the tensors themselves in a temporary directory, for the max |difference|).

 wide::  d in (256, 384, 512) x {fp32, bf16} x dropout (0, 0.3; seed 1234) x (lq, lk) in ((33, 33), (45, 39), (69, 103)) x
         kv_len (None, lk - 3); b = 2, h = 2.  Every digest must be equal: exit status 1 otherwise.
 gqaw::  heads (3, 1) and (4, 2) x {bidirectional, causal} x {padded b = 2, L = 65; packed lengths (1, 33, 64)} x {fp32, bf16}.
         Equal or not and the max |difference| are recorded; no threshold here (the float64 budgets of
         tests/test_gpu_gqa_wide_kernels.py judge these kernels).

    python tools/attn_wide_compare.py --parent-lib PARENT/libgmlm_hip.so [--out profiles/attn_wide_refactor_bytes.json]
"""
import argparse
import hashlib
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("out", "lse", "dq", "dk", "dv")
SEED = 1234


def _sha(t):
    import torch
    return hashlib.sha256(t.detach().contiguous().cpu().view(torch.uint8).numpy().tobytes()).hexdigest()


def child(lib_path, keep):
    sys.path.insert(0, ROOT)
    from gmlm_amd import _lib
    _lib.LIB_PATH = lib_path                                          # before the first load
    import torch
    from gmlm_amd import ops
    dev = torch.device("cuda:0")
    res = {}

    def record(case, out, leaves, go, save):
        lse = out.grad_fn.saved_tensors[4]
        out.backward(go)
        got = (out.detach(), lse) + tuple(t.grad for t in leaves)
        res[case] = {n: _sha(t) for n, t in zip(NAMES, got)}
        if save:
            torch.save({n: t.detach().float().cpu() for n, t in zip(NAMES, got)}, os.path.join(keep, case + ".pt"))

    b, h = 2, 2
    for d in (256, 384, 512):
        for dtype, tn in ((torch.float32, "fp32"), (torch.bfloat16, "bf16")):
            for p in (0.0, 0.3):
                for lq, lk in ((33, 33), (45, 39), (69, 103)):
                    for kv in (None, lk - 3):
                        g = torch.Generator().manual_seed(d + 7 * lq + lk)
                        q, go = (torch.randn(b, lq, h * d, generator=g).to(dev, dtype) for _ in range(2))
                        k, v = (torch.randn(b, lk, h * d, generator=g).to(dev, dtype) for _ in range(2))
                        leaves = [t.requires_grad_(True) for t in (q, k, v)]
                        kv_len = None if kv is None else torch.full((b,), kv, dtype=torch.int32, device=dev)
                        out = ops.Attention.apply(*leaves, kv_len, h, d ** -0.5, p, SEED)
                        record(f"wide d{d} {tn} p{p} lq{lq} lk{lk} kv_len {kv}", out, leaves, go, False)
    D = 256
    for hq, hkv in ((3, 1), (4, 2)):
        for causal in (False, True):
            for dtype, tn in ((torch.float32, "fp32"), (torch.bfloat16, "bf16")):
                for layout, shape in (("padded L65", (2, 65)), ("packed 1+33+64", (98,))):
                    g = torch.Generator().manual_seed(10 * hq + hkv)
                    q, go = (torch.randn(*shape, hq * D, generator=g).to(dev, dtype) for _ in range(2))
                    k, v = (torch.randn(*shape, hkv * D, generator=g).to(dev, dtype) for _ in range(2))
                    leaves = [t.requires_grad_(True) for t in (q, k, v)]
                    if len(shape) == 2:
                        out = ops.gqa_d256_attention(*leaves, None, hq, hkv, D ** -0.5, causal)
                    else:
                        cu = torch.tensor([0, 1, 34, 98], dtype=torch.int32, device=dev)
                        out = ops.gqa_d256_attention_varlen(*leaves, cu, 64, hq, hkv, D ** -0.5, causal)
                    record(f"gqaw {hq}-{hkv} {'causal' if causal else 'bidir'} {tn} {layout}", out, leaves, go, True)
    torch.cuda.synchronize()
    print("DIGESTS " + json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib")
    ap.add_argument("--new-lib", default=os.path.join(ROOT, "gmlm_amd", "libgmlm_hip.so"))
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", nargs=2, metavar=("LIB", "DIR"), help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(*a.child)
    if not a.parent_lib:
        ap.error("--parent-lib is required")
    import torch
    sides = {}
    with tempfile.TemporaryDirectory() as tmp:
        for side, path in (("parent", a.parent_lib), ("new", a.new_lib)):
            keep = os.path.join(tmp, side)
            os.makedirs(keep)
            run = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", os.path.abspath(path), keep],
                                 capture_output=True, text=True)
            if run.returncode != 0:
                sys.exit(f"{side} child failed ({run.returncode}):\n{run.stdout[-2000:]}\n{run.stderr[-4000:]}")
            sides[side] = json.loads(next(ln for ln in run.stdout.splitlines() if ln.startswith("DIGESTS "))[len("DIGESTS "):])
        wide, gqaw = [], []
        for case, old in sides["parent"].items():
            new = sides["new"][case]
            differs = [n for n in NAMES if old[n] != new[n]]
            if case.startswith("wide"):
                wide.append(dict(case=case, equal=not differs, differs=differs))
            else:
                a_, b_ = (torch.load(os.path.join(tmp, s, case + ".pt")) for s in ("parent", "new"))
                diff = {}
                for n in NAMES:
                    both_inf = torch.isinf(a_[n]) & (a_[n] == b_[n])                 # lse = -inf on both sides is no difference
                    diff[n] = float(torch.where(both_inf, torch.zeros_like(a_[n]), (a_[n] - b_[n]).abs()).max()) if a_[n].numel() else 0.0
                gqaw.append(dict(case=case, equal=not differs, differs=differs, max_abs_diff=diff,
                                 max_abs_parent={n: float(a_[n][torch.isfinite(a_[n])].abs().max()) for n in NAMES}))
    bad = [r["case"] for r in wide if not r["equal"]]
    res = dict(what="sha256 of out, lse, dq, dk, dv per case, parent build against new build, one fresh process per library; wide:: must "
                    "be equal, gqaw:: is recorded with its max |difference| (fp32 values of both sides)",
               device=torch.cuda.get_device_name(0) if torch.cuda.is_available() else None,
               wide_cases=len(wide), wide_equal=len(wide) - len(bad), wide_not_equal=bad,
               gqaw_cases=len(gqaw), gqaw_equal=sum(r["equal"] for r in gqaw), gqaw=gqaw)
    text = json.dumps(res, indent=1)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text + "\n")
    print(f"wide:: {res['wide_equal']} of {res['wide_cases']} cases equal; gqaw:: {res['gqaw_equal']} of {res['gqaw_cases']} equal")
    for r in gqaw:
        if not r["equal"]:
            print("  ", r["case"], {n: f"{r['max_abs_diff'][n]:.2e}" for n in r["differs"]})
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
