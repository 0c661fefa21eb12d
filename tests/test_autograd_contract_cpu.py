"""The autograd contract of every custom node under frozen inputs (no GPU needed).

``NODES`` holds one or more builders per ``torch.autograd.Function`` subclass defined in gmlm_amd.ops, .nn, .dense, .mpnet and
.deberta; ``test_every_node_has_a_builder`` walks those modules, so a new node without an entry fails here.  A builder makes
small inputs on the device asked for and returns a ``Case``: the differentiable inputs by name and a function that runs the node
on them.  Here the nodes run on the CPU through the recorder lib of test_attention_routes_cpu.py (every entry point returns 0
and writes nothing); tests/test_gpu_autograd_freeze.py runs the same builders on the device and looks at the values.

Per (builder, freeze pattern): forward + backward complete, every input that requires grad ends with a ``.grad`` of its own
shape and dtype, every frozen input with ``.grad is None``.  Patterns: every non-empty subset of up to 4 inputs; beyond that
each input alone, all but each input, and all.  A variadic node's masters are inputs of their own.  Nodes with two outputs
also run with each output used alone."""
import inspect
import itertools
from dataclasses import dataclass
from types import SimpleNamespace
from typing import Callable
from unittest import mock

import pytest
import torch

from gmlm_amd import deberta, dense, graph, mpnet, nn as gnn, ops
from test_attention_routes_cpu import Recorder, STREAM

MODULES = (ops, gnn, dense, mpnet, deberta)

# gmlm_amd.dist's nodes run collectives on a process group; tests/test_dist_cpu.py runs them on gloo
EXEMPT = {"dist._HaloExchange": "needs a process group: test_dist_cpu.py", "dist._HaloReady": "needs a process group: test_dist_cpu.py",
          "dist._AllGatherRows": "needs a process group: test_dist_cpu.py", "dist._RingAttention": "needs a process group: test_dist_cpu.py"}


@dataclass
class Case:
    inputs: dict                  # name -> value of a differentiable input, in the node's argument order
    call: Callable                # {name: leaf} -> output or tuple of outputs
    outputs: int = 1
    meta: dict = None             # what a value check needs beyond the inputs (lengths, seeds, index tensors)


def _gen(seed=0):
    return torch.Generator().manual_seed(seed)


def _r(g, *shape, dev, dt=torch.float32, s=1.0, add=0.0):
    return (torch.randn(*shape, generator=g) * s + add).to(dev, dt)


def _cu(lens, dev):
    return torch.tensor([0] + torch.tensor(lens).cumsum(0).tolist(), dtype=torch.int32, device=dev)


def _pos(lens, dev):
    return torch.cat([torch.arange(n) for n in lens]).to(dev, torch.int32)


def rope_table(max_len, half, dev):
    """fp32 [max_len, 2, half]: cos | sin of position * 10000^(-i / half)"""
    ang = torch.arange(max_len, dtype=torch.float64)[:, None] * (10000.0 ** (-torch.arange(half, dtype=torch.float64) / half))[None, :]
    return torch.stack([ang.cos(), ang.sin()], 1).float().contiguous().to(dev)


# ------------------------------------------------------------------------------------------------------------- attention
def b_attention(dev="cpu", dt=torch.float32, b=2, h=2, lq=2, lk=3, d=64, kv_len=None, p=0.0, seed=0):
    g = _gen(1)
    hd = h * d
    inputs = dict(q=_r(g, b, lq, hd, dev=dev, dt=dt), k=_r(g, b, lk, hd, dev=dev, dt=dt, s=1.5), v=_r(g, b, lk, hd, dev=dev, dt=dt))
    kl = None if kv_len is None else torch.tensor(kv_len, dtype=torch.int32, device=dev)
    return Case(inputs, lambda t: ops.Attention.apply(t["q"], t["k"], t["v"], kl, h, d ** -0.5, p, seed),
                meta=dict(h=h, d=d, kv_len=kv_len, p=p, seed=seed))


def b_attention_qkv(dev="cpu", dt=torch.float32, h=2, d=64, lens=(3, 2), mode="padded", masters=True, p=0.0, seed=0):
    """padded: len(lens) sequences padded to max(lens) rows with kv_len = lens; packed / groups: the rows of lens back to back"""
    g = _gen(2)
    hd = h * d
    packed = mode != "padded"
    shape = (sum(lens),) if packed else (len(lens), max(lens))
    inputs = dict(qkv=torch.cat([_r(g, *shape, hd, dev=dev, dt=dt), _r(g, *shape, hd, dev=dev, dt=dt, s=1.5),
                                 _r(g, *shape, hd, dev=dev, dt=dt)], -1))
    if masters:
        inputs.update({n: _r(g, hd, dev=dev) for n in ("bq", "bk", "bv")})
    cu = _cu(lens, dev) if packed else None
    kl = None if packed else torch.tensor(lens, dtype=torch.int32, device=dev)
    groups = ops.pack_sequence_groups(lens).to(dev) if mode == "groups" else None

    def call(t):
        bias = (t["bq"], t["bk"], t["bv"]) if masters else ()
        return ops.AttentionQKV.apply(t["qkv"], kl, h, d ** -0.5, p, seed, cu, max(lens) if packed else 0, None, groups, *bias)
    return Case(inputs, call, meta=dict(h=h, d=d, lens=lens, packed=packed, p=p, seed=seed, grouped=groups is not None))


def b_relbias(dev="cpu", dt=torch.float32, h=2, lens=(3, 2), packed=False, p=0.0, seed=0, scale=0.125):
    g = _gen(3)
    hd, m = h * 64, max(lens) + 2
    shape = (sum(lens),) if packed else (len(lens), max(lens))
    inputs = dict(qkv=_r(g, *shape, 3 * hd, dev=dev, dt=dt), rel_bias=_r(g, h, 2 * m - 1, dev=dev))
    cu = _cu(lens, dev) if packed else None
    kl = None if packed else torch.tensor(lens, dtype=torch.int32, device=dev)
    return Case(inputs, lambda t: ops.AttentionRelBiasQKV.apply(t["qkv"], t["rel_bias"], kl, h, scale, p, seed, cu,
                                                                max(lens) if packed else 0),
                meta=dict(h=h, d=64, lens=lens, packed=packed, p=p, seed=seed, m=m, scale=scale))


def b_disent(dev="cpu", dt=torch.float32, h=2, lens=(3, 2), packed=False, w=4, p=0.0, seed=0, scale=0.125):
    g = _gen(4)
    hd, m = h * 64, max(lens) + 1
    shape = (sum(lens),) if packed else (len(lens), max(lens))
    rows = sum(lens) if packed else len(lens) * max(lens)
    inputs = dict(qkv=_r(g, *shape, 3 * hd, dev=dev, dt=dt), c2p=_r(g, h, rows, w, dev=dev), p2c=_r(g, h, rows, w, dev=dev))
    col = torch.div(torch.arange(2 * m - 1) * w, 2 * m - 1, rounding_mode="floor").to(dev, torch.int32)
    cu = _cu(lens, dev) if packed else None
    kl = None if packed else torch.tensor(lens, dtype=torch.int32, device=dev)
    return Case(inputs, lambda t: ops.AttentionDisentQKV.apply(t["qkv"], t["c2p"], t["p2c"], col, kl, h, scale, p, seed, cu,
                                                               max(lens) if packed else 0),
                meta=dict(h=h, d=64, lens=lens, packed=packed, p=p, seed=seed, m=m, col=col, scale=scale))


def b_causal(dev="cpu", dt=torch.float32, hq=4, hkv=2, d=64, lens=(3, 2), bidir=False, packed=False, groups=False):
    g = _gen(5)
    shape = (sum(lens),) if packed else (len(lens), max(lens))
    inputs = dict(q=_r(g, *shape, hq * d, dev=dev, dt=dt), k=_r(g, *shape, hkv * d, dev=dev, dt=dt, s=1.5),
                  v=_r(g, *shape, hkv * d, dev=dev, dt=dt))
    meta = dict(hq=hq, hkv=hkv, d=d, lens=lens, packed=packed, bidir=bidir)
    if packed:
        cu = _cu(lens, dev)
        gr = ops.pack_sequence_groups(lens).to(dev) if groups else None
        return Case(inputs, lambda t: ops.CausalAttentionVarlen.apply(t["q"], t["k"], t["v"], cu, max(lens), hq, hkv, d ** -0.5, d,
                                                                      bidir, gr), meta=meta)
    kl = torch.tensor(lens, dtype=torch.int32, device=dev)
    return Case(inputs, lambda t: ops.CausalAttention.apply(t["q"], t["k"], t["v"], kl, hq, hkv, d ** -0.5, d, bidir), meta=meta)


def b_rope_causal(dev="cpu", dt=torch.float32, hq=2, hkv=1, lens=(3, 2), packed=False, attend=True):
    """RopeCausalAttention(Varlen), or with ``attend`` False QKNormRope alone; head dim 128"""
    g = _gen(6)
    shape = (sum(lens),) if packed else (len(lens), max(lens))
    inputs = dict(qkv=_r(g, *shape, (hq + 2 * hkv) * 128, dev=dev, dt=dt), qw=_r(g, 128, dev=dev, s=0.1, add=1.0),
                  kw=_r(g, 128, dev=dev, s=0.1, add=1.0))
    cs = rope_table(max(lens) + 3, 64, dev)
    scale, eps = 128 ** -0.5, 1e-6
    meta = dict(hq=hq, hkv=hkv, d=128, lens=lens, packed=packed, cs=cs, eps=eps, bidir=False)
    if packed:
        cu, pos = _cu(lens, dev), _pos(lens, dev)
        if attend:
            return Case(inputs, lambda t: ops.RopeCausalAttentionVarlen.apply(t["qkv"], t["qw"], t["kw"], cs, pos, cu, max(lens), hq, hkv,
                                                                              scale, eps), meta=meta)
        return Case(inputs, lambda t: ops.QKNormRope.apply(t["qkv"], t["qw"], t["kw"], cs, hq, hkv, eps, pos), meta=meta)
    kl = torch.tensor(lens, dtype=torch.int32, device=dev)
    if attend:
        return Case(inputs, lambda t: ops.RopeCausalAttention.apply(t["qkv"], t["qw"], t["kw"], cs, kl, hq, hkv, scale, eps), meta=meta)
    return Case(inputs, lambda t: ops.QKNormRope.apply(t["qkv"], t["qw"], t["kw"], cs, hq, hkv, eps), meta=meta)


def b_rope_attention(dev="cpu", dt=torch.float32, h=2, lens=(3, 2), packed=False, window=None, groups=False):
    """_RopeAttention rewrites its input: the node gets a copy of the leaf (the fused projection's output in the encoders)"""
    g = _gen(7)
    shape = (sum(lens),) if packed else (len(lens), max(lens))
    inputs = dict(qkv=_r(g, *shape, 3 * h * 64, dev=dev, dt=dt))
    cs = rope_table(max(lens) + 3, 32, dev)
    meta = dict(h=h, d=64, lens=lens, packed=packed, cs=cs, window=window)
    if packed:
        cu, pos = _cu(lens, dev), _pos(lens, dev)
        gr = ops.pack_sequence_groups(lens).to(dev) if groups else None
        return Case(inputs, lambda t: ops._RopeAttention.apply(t["qkv"].clone(), cs, None, h, 0.125, window, pos, cu, max(lens), None, gr),
                    2, meta)
    kl = torch.tensor(lens, dtype=torch.int32, device=dev)
    return Case(inputs, lambda t: ops._RopeAttention.apply(t["qkv"].clone(), cs, kl, h, 0.125, window, None, None, 0, None, None), 2, meta)


def b_rope_gqa(dev="cpu", dt=torch.float32, hq=4, hkv=2, d=64, lens=(3, 2), packed=False, bidir=False, groups=False):
    g = _gen(8)
    shape = (sum(lens),) if packed else (len(lens), max(lens))
    inputs = dict(qkv=_r(g, *shape, (hq + 2 * hkv) * d, dev=dev, dt=dt))
    cs = rope_table(max(lens) + 3, d // 2, dev)
    meta = dict(hq=hq, hkv=hkv, d=d, lens=lens, packed=packed, cs=cs, bidir=bidir)
    if packed:
        cu, pos = _cu(lens, dev), _pos(lens, dev)
        gr = ops.pack_sequence_groups(lens).to(dev) if groups else None
        return Case(inputs, lambda t: ops._RopeCausalGQA.apply(t["qkv"].clone(), cs, None, hq, hkv, d, d ** -0.5, pos, cu, max(lens),
                                                               bidir, gr), 2, meta)
    kl = torch.tensor(lens, dtype=torch.int32, device=dev)
    return Case(inputs, lambda t: ops._RopeCausalGQA.apply(t["qkv"].clone(), cs, kl, hq, hkv, d, d ** -0.5, None, None, 0, bidir), 2, meta)


# ------------------------------------------------------------------------------------------------------------- row kernels
def b_bias_res_ln(dev="cpu", dt=torch.float32, rows=3, f=64, act=False, p=0.0, seed=0):
    g = _gen(9)
    inputs = dict(x=_r(g, rows, f, dev=dev, dt=dt), bias=_r(g, f, dev=dev, s=0.1), res=_r(g, rows, f, dev=dev, dt=dt),
                  gamma=_r(g, f, dev=dev, s=0.1, add=1.0), beta=_r(g, f, dev=dev, s=0.1))
    return Case(inputs, lambda t: ops.BiasResLayerNorm.apply(t["x"], t["bias"], t["res"], t["gamma"], t["beta"], 1e-12, act, p, seed),
                meta=dict(act=act, p=p, seed=seed, eps=1e-12))


def b_add_norm(dev="cpu", dt=torch.float32, rows=3, f=64, ln=True, has_b=True, has_beta=True):
    g = _gen(10)
    inputs = dict(a=_r(g, rows, f, dev=dev, dt=dt))
    if has_b:
        inputs["b"] = _r(g, rows, f, dev=dev, dt=dt)
    inputs["w"] = _r(g, f, dev=dev, s=0.1, add=1.0)
    if ln and has_beta:
        inputs["beta"] = _r(g, f, dev=dev, s=0.1)
    return Case(inputs, lambda t: ops._AddNorm.apply(ln, t["a"], t.get("b"), t["w"], t.get("beta"), 1e-6), 2, dict(ln=ln, eps=1e-6))


def b_graphnorm(dev="cpu", dt=torch.float32, n=5, f=8, act=True, p=0.0, seed=0):
    g = _gen(11)
    inputs = dict(z=_r(g, n, f, dev=dev, dt=dt), weight=_r(g, f, dev=dev, s=0.1, add=1.0), bias=_r(g, f, dev=dev, s=0.1),
                  mean_scale=_r(g, f, dev=dev, s=0.1, add=1.0))
    return Case(inputs, lambda t: ops.GraphNormAct.apply(t["z"], t["weight"], t["bias"], t["mean_scale"], 1e-5, act, p, seed, dt, None, 0),
                meta=dict(act=act, p=p, seed=seed, eps=1e-5))


def b_bias_gelu(dev="cpu", dt=torch.float32, rows=3, f=64, p=0.0, seed=0):
    g = _gen(12)
    inputs = dict(x=_r(g, rows, f, dev=dev, dt=dt), bias=_r(g, f, dev=dev, s=0.1))
    return Case(inputs, lambda t: ops.BiasGelu.apply(t["x"], t["bias"], p, seed), meta=dict(p=p, seed=seed))


def b_glu(dev="cpu", dt=torch.float32, rows=3, inter=8, stem="swiglu"):
    g = _gen(13)
    return Case(dict(gu=_r(g, rows, 2 * inter, dev=dev, dt=dt)), lambda t: ops._GLU.apply(stem, t["gu"]), meta=dict(stem=stem))


def b_embed_sum(dev="cpu", dt=torch.float32, rows=6, p=8, vocab=11, npos=7):
    g = _gen(14)
    tok = torch.randint(0, vocab, (rows,), generator=g).to(dev)
    pos = torch.randint(0, npos, (rows,), generator=g).to(dev)
    inputs = dict(word=_r(g, vocab, p, dev=dev), pos=_r(g, npos, p, dev=dev), type=_r(g, 2, p, dev=dev))
    return Case(inputs, lambda t: ops.EmbedSum.apply(tok, pos, t["word"], t["pos"], t["type"], dt, None), meta=dict(tok=tok, pos_ids=pos))


def b_softmask(dev="cpu", dt=torch.float32, n=5, f=6, out_cols=8):
    """x (node features) and the mask get no gradient by design: the mask token is the node's one differentiable input"""
    g = _gen(15)
    x = _r(g, n, f, dev=dev)
    mask = (torch.arange(n) % 2 == 0).to(dev)
    return Case(dict(token=_r(g, 1, f, dev=dev)), lambda t: ops.SoftMask.apply(x, mask, t["token"], 0.7, dt, out_cols),
                meta=dict(x=x, mask=mask, beta=0.7, out_cols=out_cols))


def b_meanpool(dev="cpu", dt=torch.float32, lens=(3, 2), p=8, nodes=4, packed=False):
    """MeanPoolScatter writes into its first input: the node gets a copy of the leaf (a zero buffer in the model)"""
    g = _gen(16)
    shape = (sum(lens),) if packed else (len(lens), max(lens))
    inputs = dict(plm_embeds=_r(g, nodes, p, dev=dev), hs=_r(g, *shape, p, dev=dev, dt=dt))
    ln = torch.tensor(lens, dtype=torch.int32, device=dev)
    idx = torch.arange(len(lens), dtype=torch.int64, device=dev) * 2 % nodes
    cu = _cu(lens, dev) if packed else None
    return Case(inputs, lambda t: ops.MeanPoolScatter.apply(t["plm_embeds"].clone(), t["hs"], ln, idx, cu, None),
                meta=dict(lens=lens, idx=idx, packed=packed))


def _toy_csr(dev, n):
    """a ring with both directions and two relations; on the CPU the index arrays are placeholders of the right shape"""
    src = torch.arange(n).repeat(2)
    dst = torch.cat([(torch.arange(n) + 1) % n, (torch.arange(n) + 2) % n])
    et = torch.cat([torch.zeros(n, dtype=torch.long), torch.ones(n, dtype=torch.long)])
    if torch.device(dev).type == "cuda":
        return graph.build_rel_csr(torch.stack([src, dst]).to(dev), n, 2, edge_type=et.to(dev)), (src, dst, et)
    e, z = 2 * n, lambda k: torch.zeros(k, dtype=torch.int32)
    return SimpleNamespace(num_nodes=n, num_src=n, num_edges=e, r_active=2, rowptr=z(2 * n + 1), col=z(e), inv_cnt=torch.ones(2 * n),
                           t_rowptr=z(n + 1), t_seg=z(e), split=None, t_split=None), (src, dst, et)


def b_rgcn(dev="cpu", dt=torch.float32, n=5, f=8):
    g = _gen(17)
    csr, edges = _toy_csr(dev, n)
    return Case(dict(x=_r(g, n, f, dev=dev, dt=dt)), lambda t: ops.RGCNAggregate.apply(t["x"], csr), meta=dict(edges=edges, n=n))


# ------------------------------------------------------------------------------------------------------------------- nn
def b_root_addmm(dev="cpu", dt=torch.float32, n=5, fi=6, fo=8, pad=2):
    g = _gen(18)
    inputs = dict(x=_r(g, n, fi + pad, dev=dev, dt=dt), root=_r(g, fi, fo, dev=dev), bias=_r(g, fo, dev=dev))

    def call(t):
        rootc = torch.cat([t["root"].detach(), t["root"].new_zeros(pad, fo)]).to(dt)
        return gnn._RootAddmm.apply(t["x"], rootc, t["bias"].detach().to(dt), t["root"], t["bias"])
    return Case(inputs, call, meta=dict(pad=pad))


def b_select_rows(dev="cpu", dt=torch.float32):
    g = _gen(19)
    idx = torch.tensor([3, 0, 2], device=dev)
    return Case(dict(x=_r(g, 5, 4, dev=dev, dt=dt)), lambda t: gnn._SelectRows.apply(t["x"], idx), meta=dict(idx=idx))


def b_basis(dev="cpu", dt=torch.float32, ra=3, nb=4, cols=8):
    """nb <= 32, ra <= 5 and cols % 4 == 0: the HIP kernels; otherwise the library GEMM.  The node refuses host tensors by
    ``is_cuda``, which has no hook to make inert: on the CPU the attribute reads True while the forward runs."""
    g = _gen(20)
    inputs = dict(comp=_r(g, ra, nb, dev=dev), weight=_r(g, nb, cols, dev=dev))

    def call(t):
        if torch.device(dev).type == "cuda":
            return gnn._BasisCompose.apply(t["comp"], t["weight"], None)
        with mock.patch.object(torch.Tensor, "is_cuda", True):
            return gnn._BasisCompose.apply(t["comp"], t["weight"], None)
    return Case(inputs, call)


def b_split_last(dev="cpu", dt=torch.float32):
    g = _gen(21)
    return Case(dict(x=_r(g, 3, 10, dev=dev, dt=dt)), lambda t: gnn._SplitLast.apply(t["x"], 4), 2, dict(c=4))


def b_scaled_projection(dev="cpu", dt=torch.float32, n=5, dims=(4, 8), p=8, cat=False):
    g = _gen(22)
    k = len(dims)
    inputs = dict(weights=torch.softmax(_r(g, k, dev=dev), 0))
    inputs.update({f"emb{i}": _r(g, n, dims[i], dev=dev, dt=dt) for i in range(k)})
    inputs.update({f"w{i}": _r(g, p, dims[i], dev=dev, s=0.3) for i in range(k)})
    inputs.update({f"b{i}": _r(g, p, dev=dev, s=0.3) for i in range(k)})
    seg = torch.repeat_interleave(torch.arange(k), torch.tensor(dims)).to(dev)
    onehot = torch.zeros(k, seg.numel(), device=dev).scatter_(0, seg.view(1, -1), 1.0)

    def call(t):
        args = [t[f"{s}{i}"] for s in ("emb", "w", "b") for i in range(k)]
        if cat:
            return gnn._ScaledProjectionCat.apply(t["weights"], dt, seg, onehot, *args)
        return gnn._ScaledProjectionSum.apply(t["weights"], dt, *args)
    return Case(inputs, call, meta=dict(k=k))


# ---------------------------------------------------------------------------------------------------------------- dense
def b_linear(dev="cpu", dt=torch.float32, rows=(2, 3), k=8, ns=(8, 8, 8), residual=False, bias_grad=True, x3=False):
    """``ns``: rows of the masters stacked to one operand (three: the fused Q | K | V projection); x3: LinearBf16x3"""
    g = _gen(23)
    inputs = dict(x=_r(g, *rows, k, dev=dev, dt=dt))
    inputs.update({f"w{i}": _r(g, n, k, dev=dev, s=0.3) for i, n in enumerate(ns)})
    if bias_grad:
        inputs.update({f"b{i}": _r(g, n, dev=dev, s=0.3) for i, n in enumerate(ns)})
    bfix = [_r(g, n, dev=dev, s=0.3) for n in ns]              # bias_grad False: the bias is added, its masters are not inputs

    def call(t):
        ws = [t[f"w{i}"] for i in range(len(ns))]
        bs = [t[f"b{i}"] for i in range(len(ns))] if bias_grad else []
        wc = torch.cat([w.detach() for w in ws]).to(dt)
        bc = torch.cat([b.detach() for b in (bs or bfix)]).to(dt)
        if x3:
            return dense.LinearBf16x3.apply(t["x"], dense.SplitWeight(wc), bc, residual, bias_grad, *ws, *bs)
        return dense._Linear.apply(t["x"], wc, bc, residual, bias_grad, *ws, *bs)
    return Case(inputs, call, 2 if residual else 1, dict(ns=ns, bfix=bfix, bias_grad=bias_grad, residual=residual))


# ------------------------------------------------------------------------------------------------------- mpnet / deberta
def b_bias_table(dev="cpu", dt=torch.float32, h=2, m=5):
    g = _gen(24)
    bucket, gather = mpnet.bucket_index(m, dev)
    return Case(dict(weight=_r(g, mpnet.NUM_BUCKETS + 1, h, dev=dev)), lambda t: mpnet._BiasTable.apply(t["weight"], bucket, gather),
                meta=dict(bucket=bucket))


def b_tables(dev="cpu", dt=torch.float32, h=2, d=8, rows=5, w=4):
    g = _gen(25)
    inputs = dict(qkv=_r(g, rows, 3 * h * d, dev=dev, dt=dt), qkr=_r(g, w, 2 * h * d, dev=dev, dt=dt))
    return Case(inputs, lambda t: deberta._Tables.apply(t["qkv"], t["qkr"], h), 2, dict(h=h, d=d))


def _v(fn, **kw):
    return lambda dev="cpu", dt=torch.float32, **more: fn(dev, dt, **{**kw, **more})


# node -> {variant id: builder}
NODES = {
    "ops.Attention": {"plain": b_attention, "kv_len": _v(b_attention, kv_len=(2, 3))},
    "ops.AttentionQKV": {f"{m}_{'masters' if ms else 'nobias'}": _v(b_attention_qkv, mode=m, masters=ms)
                         for m in ("padded", "packed", "groups") for ms in (True, False)},
    "ops.AttentionRelBiasQKV": {"padded": b_relbias, "packed": _v(b_relbias, packed=True)},
    "ops.AttentionDisentQKV": {"padded": b_disent, "packed": _v(b_disent, packed=True)},
    "ops.CausalAttention": {"causal_d64": b_causal, "bidir_d128": _v(b_causal, d=128, bidir=True)},
    "ops.CausalAttentionVarlen": {"causal_d64": _v(b_causal, packed=True), "bidir_d128_groups": _v(b_causal, d=128, bidir=True, packed=True,
                                                                                                 groups=True)},
    "ops.RopeCausalAttention": {"padded": b_rope_causal},
    "ops.RopeCausalAttentionVarlen": {"packed": _v(b_rope_causal, packed=True)},
    "ops.QKNormRope": {"padded": _v(b_rope_causal, attend=False), "packed": _v(b_rope_causal, attend=False, packed=True)},
    "ops._RopeAttention": {"full": b_rope_attention, "band": _v(b_rope_attention, window=1),
                           "packed_groups": _v(b_rope_attention, packed=True, groups=True), "packed_band": _v(b_rope_attention, packed=True,
                                                                                                             window=1)},
    "ops._RopeCausalGQA": {"causal_d64": b_rope_gqa, "bidir_d128": _v(b_rope_gqa, d=128, bidir=True),
                           "packed_groups": _v(b_rope_gqa, packed=True, groups=True)},
    "ops.BiasResLayerNorm": {"narrow": b_bias_res_ln, "wide_act": _v(b_bias_res_ln, f=1032, act=True)},
    "ops._AddNorm": {f"{'ln' if ln else 'rms'}{'_b' if hb else ''}{'_beta' if hbeta else ''}": _v(b_add_norm, ln=ln, has_b=hb, has_beta=hbeta)
                     for ln, hb, hbeta in ((True, True, True), (True, False, False), (True, True, False), (True, False, True),
                                           (False, True, False), (False, False, False))},
    "ops.GraphNormAct": {"act": b_graphnorm, "drop": _v(b_graphnorm, p=0.1, seed=5)},
    "ops.BiasGelu": {"plain": b_bias_gelu},
    "ops._GLU": {"swiglu": b_glu, "geglu": _v(b_glu, stem="geglu")},
    "ops.EmbedSum": {"plain": b_embed_sum},
    "ops.SoftMask": {"plain": b_softmask},
    "ops.MeanPoolScatter": {"padded": b_meanpool, "packed": _v(b_meanpool, packed=True)},
    "ops.RGCNAggregate": {"ring": b_rgcn},
    "nn._RootAddmm": {"pad2": b_root_addmm},
    "nn._SelectRows": {"plain": b_select_rows},
    "nn._BasisCompose": {"hip": b_basis, "fallback": _v(b_basis, ra=6, cols=6)},
    "nn._SplitLast": {"plain": b_split_last},
    "nn._ScaledProjectionSum": {"k2": b_scaled_projection},
    "nn._ScaledProjectionCat": {"k2": _v(b_scaled_projection, cat=True)},
    "dense._Linear": {"one": _v(b_linear, ns=(8,)), "one_res": _v(b_linear, ns=(8,), residual=True), "qkv": b_linear,
                      "qkv_res": _v(b_linear, residual=True), "qkv_res_nobiasgrad": _v(b_linear, residual=True, bias_grad=False)},
    "dense.LinearBf16x3": {"one": _v(b_linear, ns=(8,), x3=True), "one_res": _v(b_linear, ns=(8,), residual=True, x3=True),
                           "qkv": _v(b_linear, x3=True), "qkv_res": _v(b_linear, residual=True, x3=True),
                           "qkv_res_nobiasgrad": _v(b_linear, residual=True, bias_grad=False, x3=True)},
    "mpnet._BiasTable": {"plain": b_bias_table},
    "deberta._Tables": {"plain": b_tables},
}


def patterns(names):
    """Freeze patterns as tuples of the names that require grad"""
    names = list(names)
    if len(names) <= 4:
        return [c for k in range(1, len(names) + 1) for c in itertools.combinations(names, k)]
    out = [(n,) for n in names] + [tuple(m for m in names if m != n) for n in names] + [tuple(names)]
    return list(dict.fromkeys(out))


def run_pattern(case, pattern, use=None, gouts=None):
    """One forward + backward with exactly ``pattern`` requiring grad; ``use``: index of the one output that is used.
    -> (leaves, outputs)"""
    leaves = {n: v.clone().requires_grad_(n in pattern) for n, v in case.inputs.items()}
    outs = case.call(leaves)
    outs = outs if isinstance(outs, tuple) else (outs,)
    assert len(outs) == case.outputs
    idx = range(len(outs)) if use is None else (use,)
    used = [i for i in idx if outs[i].requires_grad]
    assert used, "no used output requires grad"
    torch.autograd.backward([outs[i] for i in used], [torch.ones_like(outs[i]) if gouts is None else gouts[i] for i in used])
    return leaves, outs


def assert_contract(case, pattern, leaves):
    for n, leaf in leaves.items():
        if n in pattern:
            assert leaf.grad is not None, f"{n} requires grad and got none"
            assert leaf.grad.shape == leaf.shape and leaf.grad.dtype == leaf.dtype, (n, leaf.grad.shape, leaf.grad.dtype)
        else:
            assert leaf.grad is None, f"{n} is frozen and got a gradient"


def defined_nodes():
    found = {}
    for mod in MODULES:
        for name, cls in inspect.getmembers(mod, inspect.isclass):
            if issubclass(cls, torch.autograd.Function) and cls.__module__ == mod.__name__:
                found[f"{mod.__name__.rsplit('.', 1)[1]}.{name}"] = cls
    return found


@pytest.fixture
def rec(monkeypatch):
    """The recorder lib of test_attention_routes_cpu.py, with what else needs a device made inert: the graph module's own
    handle on the library, and the GEMMs that ask the library for an fp32 result from 16-bit operands."""
    r = Recorder()
    for mod in (ops, graph):
        monkeypatch.setattr(mod, "lib", lambda: r)
        monkeypatch.setattr(mod, "_stream", lambda: STREAM)
        monkeypatch.setattr(mod, "check", lambda rc, what="": r.checked.append(what))
    monkeypatch.setattr(ops, "_cuda", lambda *ts: None)
    monkeypatch.setattr(ops, "SEED_DEVICE", None)

    def f32_out(op, *args, out=None, **kw):
        res = getattr(torch, op)(*[a.float() for a in args])
        return res if out is None else out.copy_(res)
    monkeypatch.setattr(dense, "_f32_out", f32_out)
    return r


CASES = [(node, var, dt) for node, variants in NODES.items() for var in variants for dt in (torch.float32, torch.bfloat16)
         if not (node == "dense.LinearBf16x3" and dt == torch.bfloat16)]          # bf16x3 takes fp32 activations only


def test_every_node_has_a_builder():
    found = defined_nodes()
    missing, stale = sorted(set(found) - set(NODES)), sorted(set(NODES) - set(found))
    assert not missing, f"autograd nodes without a builder in NODES: {missing}"
    assert not stale, f"NODES names nodes that no longer exist: {stale}"
    assert all(variants for variants in NODES.values())
    from gmlm_amd import dist
    dist_nodes = {f"dist.{n}" for n, c in inspect.getmembers(dist, inspect.isclass)
                  if issubclass(c, torch.autograd.Function) and c.__module__ == dist.__name__}
    assert dist_nodes == set(EXEMPT), (sorted(dist_nodes), sorted(EXEMPT))


def test_builders_run_the_node_they_are_filed_under(rec):
    found = defined_nodes()
    for node, variants in NODES.items():
        for var, build in variants.items():
            case = build()
            leaves = {n: v.clone().requires_grad_(True) for n, v in case.inputs.items()}
            outs = case.call(leaves)
            out = outs[0] if isinstance(outs, tuple) else outs
            assert out.grad_fn.name().startswith(found[node].__name__ + "Backward"), (node, var, out.grad_fn.name())


@pytest.mark.parametrize("node,var,dt", CASES, ids=[f"{n}-{v}-{'bf16' if d == torch.bfloat16 else 'fp32'}" for n, v, d in CASES])
def test_freeze_patterns(rec, node, var, dt):
    """every pattern runs even when an earlier one failed: the failure names each (pattern, output used) that broke"""
    case = NODES[node][var]("cpu", dt)
    failed = []
    for pattern in patterns(case.inputs):
        for use in [None] + (list(range(case.outputs)) if case.outputs > 1 else []):
            try:
                leaves, _ = run_pattern(case, pattern, use)
                assert_contract(case, pattern, leaves)
            except Exception as e:
                failed.append(f"trainable {pattern}, output used {use}: {type(e).__name__}: {e}")
    assert not failed, f"{node}[{var}]: {len(failed)} patterns failed:\n  " + "\n  ".join(failed)


def test_pattern_rule():
    assert len(patterns("abcd")) == 15 and len(patterns("abc")) == 7
    assert len(patterns("abcde")) == 11 and ("a",) in patterns("abcde") and tuple("bcde") in patterns("abcde")


@pytest.mark.parametrize("mode,h,lens", [("padded", 2, (3, 2)), ("groups", 8, (1,) * 64)], ids=["streaming", "short"])
def test_attention_qkv_forms_no_bias_sum_nobody_asked_for(rec, mode, h, lens):
    """No master needs a gradient: neither the fused bias sums of the short-sequence backward nor the column-sum pass; one
    master does: the sums are formed and the frozen masters' entries are None."""
    for pattern, wants in ((("qkv",), False), (("qkv", "bk"), True), (("bv",), True)):
        case = b_attention_qkv("cpu", torch.bfloat16, h=h, lens=lens, mode=mode)
        rec.take()
        leaves, _ = run_pattern(case, pattern)
        assert_contract(case, pattern, leaves)
        calls = rec.take()
        bwd = next(args for name, args in calls if name == "gmlm_attention_bwd")
        fused = mode == "groups" and wants                    # 64 sequences x 8 heads: the short-sequence kernels form the sums
        assert (bwd[-6] is not None) == fused and (bwd[-5] is not None) == fused, "dbias_partial / dbias of gmlm_attention_bwd"
        assert ("gmlm_colstats" in [n for n, _ in calls]) == (wants and not fused)
