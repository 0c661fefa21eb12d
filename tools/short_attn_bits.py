"""sha256 of every output buffer of the LDS-resident short-sequence attention entry points (K5 through gmlm_attention_fwd / _bwd,
gmlm_attention_gqa_short_*, gmlm_attention_d32_short_*) for a library given by path: two builds of libgmlm_hip.so that compute
the same bits write the same ``digests`` block.  These kernels have fixed summation orders and no atomics.

    python tools/short_attn_bits.py --lib gmlm_amd/libgmlm_hip.so --out profiles/short_attn_bits.json

Inputs are drawn on the CPU from ``torch.Generator().manual_seed(case index)``; the entry points are called directly, with the
``_lib`` signature tables, so the Python layers above them take no part.  The cases are the smallest that reach every
instantiation (R = 32 / 64 / 96 / 128 x flag, forward and backward) and every loop edge: a sequence starting at an odd tile row, a
second wave holding one row, a 13-sequence group, a full single-sequence group, a two-sequence full group.  Needs a GPU.

``--time`` measures instead: 1,257 sequences of 16-128 tokens (the workload of tools/gqa_short_probe.py and
tools/attn_d32_short_probe.py), K5 at h = 12, gqas at 18 / 6 bidirectional and 14 / 2 causal, d32s at h = 12; forward, backward and
backward with the bias sums, at dropout 0 and 0.1 where the family has it; per figure the median of ``--reps`` device-event
timings after a warm-up.  One process measures one library once: a comparison runs parent and new alternately, three rounds, and

    python tools/short_attn_bits.py --merge DIR --out profiles/attn_short_refactor.json

reads DIR/time_{parent,new}_{1,2,3}.json and writes, per figure, both libraries' medians, the parent's spread (max - min of its
round medians) and the verdict: the new median may exceed the parent's by no more than that spread.
"""
import argparse
import hashlib
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from gmlm_amd import _lib, ops  # noqa: E402

BF = torch.bfloat16
SEED = 1234
R128 = [3] * 13 + [2, 128, 65, 63, 127, 1]     # a 13-sequence group, a full single-sequence group, a two-sequence full group
GROUPED = {"r32": [1, 7, 24], "r64": [33], "r96": [31, 34, 5], "r128": R128}


def digest(t):
    t = t.detach().cpu().contiguous()
    return hashlib.sha256(t.view(torch.int16 if t.dtype == BF else torch.int32).numpy().tobytes()).hexdigest()


class Runner:
    def __init__(self, dev):
        self.dev, self.lib, self.cases = dev, _lib.lib(), {}

    def call(self, name, *args):
        _lib.check(getattr(self.lib, name)(*[ops._ptr(a) if isinstance(a, torch.Tensor) else a for a in args]), name)

    def case(self, name, fn):
        """fn(randn) -> {buffer name: tensor}; randn(*shape) draws from this case's generator on the CPU"""
        g = torch.Generator().manual_seed(len(self.cases))
        out = fn(lambda *shape: torch.randn(*shape, generator=g), g)
        torch.cuda.synchronize()
        self.cases[name] = {k: digest(v) for k, v in out.items()}


def packing(lens, dev):
    cu = torch.zeros(len(lens) + 1, dtype=torch.int32)
    cu[1:] = torch.tensor(lens).cumsum(0)
    return cu.to(dev), ops.pack_sequence_groups(lens).to(dev), int(sum(lens)), max(lens)


class K5:
    """gmlm_attention_fwd / _bwd at d = 64 on a fused [rows, 3 h d] buffer; padded (b, l, kv_len) or packed with groups (lens)"""

    def __init__(self, r, h, qkv, dout, lens=None, b=0, l=0, kv_len=None):
        self.r, self.h, self.qkv, self.dout, self.hd = r, h, qkv, dout, h * 64
        hd = self.hd
        self.q, self.k, self.v = qkv[..., :hd], qkv[..., hd:2 * hd], qkv[..., 2 * hd:]
        if lens is None:
            self.b, self.l, self.kv_len, self.cu, self.groups, self.ng, self.max_len, self.items = b, l, kv_len, None, None, 0, 0, b
            self.lse_shape = (b, h, l)
        else:
            self.cu, self.groups, self.l, self.max_len = packing(lens, r.dev)
            self.b, self.kv_len, self.ng = len(lens), None, self.groups.numel() - 1
            self.items, self.lse_shape = self.ng, (h, self.l)
        self.out = torch.zeros(qkv.shape[:-1] + (hd,), dtype=BF, device=r.dev)
        self.lse = torch.zeros(self.lse_shape, device=r.dev)
        self.dqkv = torch.zeros_like(qkv)
        self.part = torch.zeros(self.items * 3 * hd, device=r.dev)
        self.db = torch.zeros(3 * hd, device=r.dev)
        n = r.lib.gmlm_attention_bwd_workspace_bytes(self.b, h, self.l, self.l, 64)
        self.ws, self.ws_bytes = torch.empty(max(n, 1), dtype=torch.uint8, device=r.dev), n

    def fwd(self, p):
        hd3 = 3 * self.hd
        self.r.call("gmlm_attention_fwd", self.q, self.k, self.v, self.kv_len, self.b, self.h, self.l, self.l, 64, hd3, hd3, hd3,
                    0.125, p, SEED, None, self.out, None, self.lse, _lib.BF16, self.cu, self.max_len, self.groups, self.ng, ops._stream())

    def bwd(self, p, bias):
        hd, hd3, g = self.hd, 3 * self.hd, self.dqkv
        self.r.call("gmlm_attention_bwd", self.q, self.k, self.v, self.out, self.dout, self.lse, self.kv_len, self.b, self.h, self.l, self.l,
                    64, hd3, hd3, hd3, 0.125, p, SEED, None, g[..., :hd], g[..., hd:2 * hd], g[..., 2 * hd:], hd3, hd3, hd3, _lib.BF16,
                    self.cu, self.max_len, self.ws, self.ws_bytes, self.part if bias else None, self.db if bias else None, None,
                    self.groups, self.ng, ops._stream())


class D32:
    """gmlm_attention_d32_short_* on a fused [rows, 3 h 32] buffer, packed with groups"""

    def __init__(self, r, h, qkv, dout, lens):
        self.r, self.h, self.qkv, self.dout, self.hd = r, h, qkv, dout, h * 32
        hd = self.hd
        self.q, self.k, self.v = qkv[:, :hd], qkv[:, hd:2 * hd], qkv[:, 2 * hd:]
        self.cu, self.groups, self.rows, self.max_len = packing(lens, r.dev)
        self.b, self.ng = len(lens), self.groups.numel() - 1
        self.out = torch.zeros(self.rows, hd, dtype=BF, device=r.dev)
        self.lse = torch.zeros(h, self.rows, device=r.dev)
        self.dqkv = torch.zeros_like(qkv)
        self.part = torch.zeros(self.ng * 3 * hd, device=r.dev)
        self.db = torch.zeros(3 * hd, device=r.dev)

    def common(self, p):
        hd3 = 3 * self.hd
        return (self.cu, self.b, self.max_len, self.rows, self.h, 32, hd3, hd3, hd3, 32 ** -0.5, p, SEED, None, self.groups, self.ng)

    def fwd(self, p):
        self.r.call("gmlm_attention_d32_short_fwd", self.q, self.k, self.v, *self.common(p), self.out, self.lse, _lib.BF16, ops._stream())

    def bwd(self, p, bias):
        hd, hd3, g = self.hd, 3 * self.hd, self.dqkv
        self.r.call("gmlm_attention_d32_short_bwd", self.q, self.k, self.v, self.dout, self.lse, *self.common(p), g[:, :hd], g[:, hd:2 * hd],
                    g[:, 2 * hd:], hd3, hd3, hd3, self.part if bias else None, self.db if bias else None, _lib.BF16, ops._stream())


class Gqa:
    """gmlm_attention_gqa_short_* on a fused [rows, (hq + 2 hkv) 64] buffer, packed with groups"""

    def __init__(self, r, hq, hkv, causal, x, dout, lens):
        self.r, self.hq, self.hkv, self.causal, self.x, self.dout = r, hq, hkv, causal, x, dout
        self.nq, self.nk = hq * 64, hkv * 64
        self.cu, self.groups, self.rows, self.max_len = packing(lens, r.dev)
        self.b, self.ng = len(lens), self.groups.numel() - 1
        self.out = torch.zeros(self.rows, self.nq, dtype=BF, device=r.dev)
        self.lse = torch.zeros(hq, self.rows, device=r.dev)
        self.dx = torch.zeros_like(x)

    def split(self, t):
        return t[:, :self.nq], t[:, self.nq:self.nq + self.nk], t[:, self.nq + self.nk:]

    def common(self):
        w = self.x.shape[1]
        return (self.cu, self.b, self.max_len, self.rows, self.hq, self.hkv, 64, w, w, w, 0.125, 0.0, self.causal, self.groups, self.ng)

    def fwd(self, p=0.0):
        self.r.call("gmlm_attention_gqa_short_fwd", *self.split(self.x), *self.common(), self.out, self.lse, _lib.BF16, ops._stream())

    def bwd(self, p=0.0, bias=False):
        w = self.x.shape[1]
        self.r.call("gmlm_attention_gqa_short_bwd", *self.split(self.x), self.dout, self.lse, *self.common(), *self.split(self.dx), w, w, w,
                    _lib.BF16, ops._stream())


def fwd_bwd(make, p, biases):
    """make(randn, g) -> K5 / D32 / Gqa; one forward, then one backward per entry of ``biases``: every output buffer of each"""
    def fn(randn, g):
        a = make(randn, g)
        a.fwd(p)
        res = dict(out=a.out, lse=a.lse)
        for bias in biases:
            grad = a.dqkv if hasattr(a, "dqkv") else a.dx
            grad.zero_()
            a.bwd(p, bias)
            names, tag = ("dq", "dk", "dv"), "_bias" if bias else ""
            parts = a.split(grad) if hasattr(a, "split") else (grad[..., :a.hd], grad[..., a.hd:2 * a.hd], grad[..., 2 * a.hd:])
            res.update({n + tag: t.clone() for n, t in zip(names, parts)})
            if bias:
                res["dbias"] = a.db.clone()
        return res
    return fn


def bits(r):
    dev = r.dev
    for geo, lens in GROUPED.items():
        rows = sum(lens)
        for causal in (0, 1):
            for hq, hkv in ((4, 2), (3, 1), (2, 2)):
                r.case(f"gqas/{geo}/causal{causal}/hq{hq}_hkv{hkv}", fwd_bwd(
                    lambda randn, g: Gqa(r, hq, hkv, causal, randn(rows, (hq + 2 * hkv) * 64).to(dev, BF), randn(rows, hq * 64).to(dev, BF), lens),
                    0.0, (False,)))
        for h in (2, 6):
            for p in (0.0, 0.1):
                r.case(f"d32s/{geo}/h{h}/p{p}", fwd_bwd(
                    lambda randn, g: D32(r, h, randn(rows, 3 * h * 32).to(dev, BF), randn(rows, h * 32).to(dev, BF), lens), p, (False, True)))
    h, b = 8, 64
    for l in (17, 33, 70, 128):
        for p in (0.0, 0.1):
            def make(randn, g):
                kv_len = torch.randint(1, l + 1, (b,), generator=g).to(dev, torch.int32)
                return K5(r, h, randn(b, l, 3 * h * 64).to(dev, BF), randn(b, l, h * 64).to(dev, BF), b=b, l=l, kv_len=kv_len)
            r.case(f"k5/padded/b{b}_l{l}/p{p}", fwd_bwd(make, p, (False, True)))
    lens = R128 * 4                                     # 72 sequences x 8 heads = 576 pairs >= 512: the short path of gmlm_attention_*
    rows = sum(lens)
    for p in (0.0, 0.1):
        r.case(f"k5/packed/r128x4/p{p}", fwd_bwd(
            lambda randn, g: K5(r, h, randn(rows, 3 * h * 64).to(dev, BF), randn(rows, h * 64).to(dev, BF), lens=lens), p, (False, True)))
    whole = hashlib.sha256(json.dumps(r.cases, sort_keys=True).encode()).hexdigest()
    print(f"{len(r.cases)} cases, all = {whole}")
    return dict(what="sha256 of every output buffer (out, lse, dq, dk, dv; with the bias sums: dq_bias, dk_bias, dv_bias, dbias) of the "
                     "short-sequence attention entry points (tools/short_attn_bits.py)", cases=len(r.cases), all=whole, digests=r.cases)


def event_median(fn, reps, warm=10):
    for _ in range(warm):
        fn()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    torch.cuda.synchronize()
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return round(statistics.median(a.elapsed_time(b) for a, b in ev) * 1e3, 2)          # us


def timing(r, reps):
    dev, g = r.dev, torch.Generator().manual_seed(2)
    lens = torch.randint(16, 129, (1257,), generator=torch.Generator().manual_seed(1)).tolist()
    rows, randn = sum(lens), lambda *shape: torch.randn(*shape, generator=g)
    fams = {"k5_h12": (K5(r, 12, randn(rows, 3 * 768).to(dev, BF), randn(rows, 768).to(dev, BF), lens=lens), True),
            "d32s_h12": (D32(r, 12, randn(rows, 3 * 384).to(dev, BF), randn(rows, 384).to(dev, BF), lens), True),
            "gqas_18_6_bidir": (Gqa(r, 18, 6, 0, randn(rows, 30 * 64).to(dev, BF), randn(rows, 18 * 64).to(dev, BF), lens), False),
            "gqas_14_2_causal": (Gqa(r, 14, 2, 1, randn(rows, 18 * 64).to(dev, BF), randn(rows, 14 * 64).to(dev, BF), lens), False)}
    res = {}
    for name, (a, rich) in fams.items():
        for p in (0.0, 0.1) if rich else (0.0,):
            a.fwd(p)                                                    # the lse of this p, for the backwards below
            res[f"{name}/fwd/p{p}"] = event_median(lambda: a.fwd(p), reps)
            res[f"{name}/bwd/p{p}"] = event_median(lambda: a.bwd(p, False), reps)
            if rich:
                res[f"{name}/bwd_bias/p{p}"] = event_median(lambda: a.bwd(p, True), reps)
    for k, v in res.items():
        print(f"{k:36s} {v:9.2f} us")
    return dict(what=f"median of {reps} device-event timings per figure after 10 warm-up calls, us; 1257 sequences of 16-128 tokens "
                     f"({rows} rows), bf16 (tools/short_attn_bits.py --time)", device=torch.cuda.get_device_name(0), reps=reps, us=res)


def merge(d):
    load = lambda side: [json.load(open(os.path.join(d, f"time_{side}_{i}.json"))) for i in (1, 2, 3)]
    par, new = load("parent"), load("new")
    rows, ok = {}, True
    for k in par[0]["us"]:
        pm, nm = [x["us"][k] for x in par], [x["us"][k] for x in new]
        spread = round(max(pm) - min(pm), 2)
        over = round(statistics.median(nm) - statistics.median(pm), 2)
        rows[k] = dict(parent_rounds=pm, new_rounds=nm, parent_median=statistics.median(pm), new_median=statistics.median(nm),
                       parent_spread=spread, new_minus_parent=over, verdict="pass" if over <= spread else "fail")
        ok &= over <= spread
    return dict(what="short-sequence attention kernels, parent build against this build: three alternating rounds (parent, new, parent, "
                     "...), one process per library and round; per figure each round's median in us, the parent's spread (max - min of "
                     "its round medians) and the verdict: new median - parent median <= parent spread.  " + par[0]["what"],
                device=par[0]["device"], all_pass=ok, figures=rows)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=None, help="the libgmlm_hip.so to load (default: the tree's own)")
    ap.add_argument("--time", action="store_true", help="measure instead of hashing")
    ap.add_argument("--reps", type=int, default=60)
    ap.add_argument("--merge", default=None, metavar="DIR", help="no GPU: DIR/time_{parent,new}_{1,2,3}.json -> the comparison")
    ap.add_argument("--out", required=True)
    a = ap.parse_args()
    if a.merge:
        res = merge(a.merge)
        print("\n".join(f"{k:36s} parent {v['parent_median']:9.2f}  new {v['new_median']:9.2f}  spread {v['parent_spread']:6.2f}  {v['verdict']}"
                        for k, v in res["figures"].items()))
    else:
        if a.lib:
            _lib.LIB_PATH = os.path.abspath(a.lib)                    # before the first lib(): the one place the path is read
        assert torch.cuda.is_available(), "short_attn_bits.py needs a GPU"
        assert a.reps >= 50 or not a.time, "at least 50 repetitions per figure"
        r = Runner(torch.device("cuda:0"))
        res = timing(r, a.reps) if a.time else bits(r)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    if a.merge and not res["all_pass"]:
        sys.exit(1)


if __name__ == "__main__":
    main()
