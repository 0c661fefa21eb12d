"""sha256 of every output buffer of the pre-norm encoders' row-kernel entry points (add + RMSNorm / LayerNorm, SwiGLU / GeGLU,
rope64, qknorm_rope and its _pos form), forward and backward once each, for a library given by path: two builds of
libgmlm_hip.so that compute the same bits write the same file.

    python tools/row_kernel_bits.py --lib gmlm_amd/libgmlm_hip.so --out profiles/row_kernel_bits.json

Inputs are drawn on the CPU from ``torch.Generator().manual_seed(case index)``; the entry points are called directly, with the
``_lib`` signature tables, so the Python layers above them take no part.  Needs a GPU.

``--models`` adds a ``model_level`` block: sha256 of the hidden states and of all parameter gradients of every ``*_encode`` and
``*_encode_packed`` (fp32 and bf16, with and without checkpointing) on a two-layer BERT and on the tiny Qwen3 / ModernBERT /
MPNet models that tests/test_gpu_{qwen3,modernbert,mpnet}.py build.  ``--tree DIR`` takes ``gmlm_amd`` (its Python, and its
library unless ``--lib`` is given) and those test helpers from another checkout, e.g. a worktree of the parent commit:

    python tools/row_kernel_bits.py --models --tree ../parent --out profiles/row_kernel_bits_parent.json
"""
import argparse
import hashlib
import json
import os
import sys

import torch

_lib = ops = None            # gmlm_amd._lib, gmlm_amd.ops of the tree under test: main() imports them

BF, FP = torch.bfloat16, torch.float32
NAME = {BF: "bf16", FP: "fp32"}
VEC = {BF: 8, FP: 4}
# one width per instantiated CH (2, 4, 8, and 16 in fp32) plus the two ends
WIDTHS = {BF: (8, 520, 1032, 2056, 4096), FP: (4, 260, 516, 1028, 2052, 4096)}
ROWS = (1, 5, 33)            # 33 rows: col_reduce_plan (colreduce.hpp) gives cdiv(33, 16) = 3 chunks at every width
# tests/test_gpu_modernbert_kernels.py ROPE_CASES: (id, lead, heads, table rows, positions or None, position modulus)
ROPE_CASES = [("b1_l1", (1, 1), 1, 2, None, 0), ("b2_l3", (2, 3), 3, 3, None, 0), ("b3_l1", (3, 1), 2, 4, None, 0),
              ("pos_len1", (3,), 2, 1, (-2, 0, 7), 0), ("tail", (1367,), 2, 300, None, 300)]


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
        out = fn(lambda *shape: torch.randn(*shape, generator=g))
        torch.cuda.synchronize()
        self.cases[name] = {k: digest(v) for k, v in out.items()}

    def ws(self, name, *args):
        n = getattr(self.lib, name)(*args)
        return torch.empty(max(n, 1), dtype=torch.uint8, device=self.dev), n


def add_norm(r, dt, ln, rows, f, with_b, with_beta):
    def fn(randn):
        dev, code, st = r.dev, ops._dt(torch.empty(0, dtype=dt)), ops._stream()
        a, b = randn(rows, f).to(dt).to(dev), (randn(rows, f).to(dt).to(dev) if with_b else None)
        w, beta = (1 + 0.1 * randn(f)).to(dev), (randn(f).to(dev) if with_beta else None)
        dy, dres = randn(rows, f).to(dt).to(dev), (randn(rows, f).to(dt).to(dev) if with_b else None)
        s, y = (torch.empty_like(a) if with_b else None), torch.empty_like(a)
        mean, rstd = torch.empty(rows, device=dev), torch.empty(rows, device=dev)
        ds, dw = torch.empty_like(a), torch.empty(2, f, device=dev)
        if ln:
            r.call("gmlm_add_layernorm_fwd", a, b, w, beta, rows, f, 1e-5, s, y, mean, rstd, code, st)
            ws, n = r.ws("gmlm_add_layernorm_bwd_workspace_bytes", rows, f)
            r.call("gmlm_add_layernorm_bwd", dy, dres, s if with_b else a, w, mean, rstd, rows, f, ds, dw, dw[1] if with_beta else None,
                   code, ws, n, st)
        else:
            r.call("gmlm_add_rmsnorm_fwd", a, b, w, rows, f, 1e-6, s, y, rstd, code, st)
            ws, n = r.ws("gmlm_add_rmsnorm_bwd_workspace_bytes", rows, f)
            r.call("gmlm_add_rmsnorm_bwd", dy, dres, s if with_b else a, w, rstd, rows, f, ds, dw, code, ws, n, st)
        out = dict(y=y, rstd=rstd, ds=ds, dw=dw[0])
        if with_b:
            out["s"] = s
        if ln:
            out["mean"] = mean
        if with_beta:
            out["dbeta"] = dw[1]
        return out
    return fn


def glu(r, dt, stem, rows, inter):
    def fn(randn):
        dev, code, st = r.dev, ops._dt(torch.empty(0, dtype=dt)), ops._stream()
        gu, dy = (3 * randn(rows, 2 * inter)).to(dt).to(dev), randn(rows, inter).to(dt).to(dev)
        y, dgu = torch.empty_like(dy), torch.empty_like(gu)
        r.call(f"gmlm_{stem}_fwd", gu, rows, inter, y, code, st)
        r.call(f"gmlm_{stem}_bwd", dy, gu, rows, inter, dgu, code, st)
        return dict(y=y, dgu=dgu)
    return fn


def table(rows, half, theta=1e4):
    inv = 1.0 / (theta ** (torch.arange(0, 2 * half, 2, dtype=torch.float32) / (2 * half)))
    fr = torch.arange(rows, dtype=torch.float32)[:, None] * inv[None]
    return torch.stack([fr.cos(), fr.sin()], 1).contiguous()


def rope64(r, dt, case):
    _, lead, h, rows, positions, mod = case

    def fn(randn):
        dev, code, st = r.dev, ops._dt(torch.empty(0, dtype=dt)), ops._stream()
        tok = 1
        for n in lead:
            tok *= n
        x, cs = randn(tok, 3 * h * 64).to(dt), table(rows, 32).to(dev)
        pos, seq_len = None, lead[-1]
        if len(lead) == 1:
            pos = (torch.tensor(positions) if positions else torch.arange(tok) % mod).to(dev, torch.int32)
            seq_len = 0
        out = {}
        for name in ("fwd", "bwd"):
            buf = x.to(dev).clone()
            r.call(f"gmlm_rope64_{name}", buf, 3 * h * 64, cs, rows, tok, seq_len, pos, h, 64, code, st)
            out[name] = buf
        return out
    return fn


def qknorm_rope(r, dt, lead, hq, hkv, by_pos):
    def fn(randn):
        dev, code, st = r.dev, ops._dt(torch.empty(0, dtype=dt)), ops._stream()
        tok, max_len = lead[0] * lead[1], 700
        wid, ow = (hq + 2 * hkv) * 128, (hq + hkv) * 128
        qkv, dqkv = randn(tok, wid).to(dt).to(dev), randn(tok, wid).to(dt).to(dev)
        qw, dw = (1 + 0.1 * randn(2, 128)).to(dev), torch.empty(2, 128, device=dev)
        cs = table(max_len, 64, 1e6).to(dev)
        out, rstd = torch.empty(tok, ow, dtype=dt, device=dev), torch.empty(tok * (hq + hkv), device=dev)
        ws, n = r.ws("gmlm_qknorm_rope_bwd_workspace_bytes", tok, hq, hkv, code)
        if by_pos:
            pos = torch.arange(tok) % lead[1]
            pos[0], pos[-1] = -3, 10_000 + tok             # a negative and a too-large position: both are clamped into the table
            pos = pos.to(dev, torch.int32)
            r.call("gmlm_qknorm_rope_pos_fwd", qkv, wid, qw[0], qw[1], cs, max_len, tok, pos, hq, hkv, 128, 1e-6, out, ow, rstd, code, st)
            r.call("gmlm_qknorm_rope_pos_bwd", dqkv, wid, qkv, wid, qw[0], qw[1], cs, max_len, rstd, tok, pos, hq, hkv, 128, dw[0],
                   dw[1], code, ws, n, st)
        else:
            r.call("gmlm_qknorm_rope_fwd", qkv, wid, qw[0], qw[1], cs, max_len, tok, lead[1], hq, hkv, 128, 1e-6, out, ow, rstd, code, st)
            r.call("gmlm_qknorm_rope_bwd", dqkv, wid, qkv, wid, qw[0], qw[1], cs, max_len, rstd, tok, lead[1], hq, hkv, 128, dw[0],
                   dw[1], code, ws, n, st)
        return dict(out=out, rstd=rstd, dqkv=dqkv, dw=dw)
    return fn


MODEL_LENS = [7, 12, 1, 5, 9]


def model_level(dev):
    """{encoder/form/dtype/ckpt: digests} at the tiny geometries of the GPU tests: five sequences of MODEL_LENS tokens."""
    import test_gpu_modernbert as tm
    import test_gpu_mpnet as tp
    import test_gpu_qwen3 as tq
    from gmlm_amd import bert, modernbert, mpnet, qwen3
    from transformers import BertConfig, BertModel
    torch.manual_seed(0)
    bert_plm = BertModel(BertConfig(vocab_size=96, hidden_size=128, num_hidden_layers=2, num_attention_heads=2,
                                    intermediate_size=256, max_position_embeddings=64, hidden_dropout_prob=0.0,
                                    attention_probs_dropout_prob=0.0), add_pooling_layer=False)
    plms = [("bert", bert_plm, bert.bert_encode, bert.bert_encode_packed),
            ("qwen3", tq._make_plm(), qwen3.qwen3_encode, qwen3.qwen3_encode_packed),
            ("modernbert", tm._make_plm(8), modernbert.modernbert_encode, modernbert.modernbert_encode_packed),
            ("mpnet", tp._make_plm(), mpnet.mpnet_encode, mpnet.mpnet_encode_packed)]
    l, out = max(MODEL_LENS), {}
    ids = torch.randint(2, 96, (len(MODEL_LENS), l), generator=torch.Generator().manual_seed(3))
    lens = torch.tensor(MODEL_LENS, dtype=torch.int32)
    tok = torch.cat([ids[i, :n] for i, n in enumerate(MODEL_LENS)])
    pos = torch.cat([torch.arange(n) for n in MODEL_LENS])
    cu = torch.tensor([0] + torch.tensor(MODEL_LENS).cumsum(0).tolist(), dtype=torch.int32)
    keep = (torch.arange(l)[None] < lens[:, None]).to(dev)
    for name, plm, enc, enc_packed in plms:
        plm = plm.to(dev).train()
        for cd in (FP, BF):
            for ckpt in (False, True):
                for form in ("padded", "packed"):
                    plm.zero_grad(set_to_none=True)
                    if form == "padded":
                        hs = enc(plm, ids.to(dev), lens.to(dev), cd, True, ckpt)[keep]
                    else:
                        hs = enc_packed(plm, tok.to(dev), pos.to(dev), cu.to(dev), l, cd, True, ckpt)
                    w = torch.randn(hs.shape, generator=torch.Generator().manual_seed(5)).to(dev)
                    (hs.float() * w).sum().backward()
                    torch.cuda.synchronize()
                    grads = {n: digest(p.grad.float()) for n, p in plm.named_parameters() if p.grad is not None}
                    out[f"{name}/{form}/{NAME[cd]}/ckpt{int(ckpt)}"] = dict(
                        hidden=digest(hs.float()), grads=hashlib.sha256(json.dumps(grads, sort_keys=True).encode()).hexdigest(),
                        params_with_grad=len(grads))
    return out


def main():
    global _lib, ops
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=None, help="the libgmlm_hip.so to load (default: the tree's own)")
    ap.add_argument("--tree", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."),
                    help="checkout whose gmlm_amd (and tests/ helpers) are used")
    ap.add_argument("--models", action="store_true", help="add the model-level digests")
    ap.add_argument("--out", required=True)
    a = ap.parse_args()
    root = os.path.abspath(a.tree)
    sys.path[:0] = [root, os.path.join(root, "tests")]
    from gmlm_amd import _lib, ops
    assert os.path.abspath(_lib.__file__).startswith(root), _lib.__file__
    if a.lib:
        _lib.LIB_PATH = os.path.abspath(a.lib)                    # before the first lib(): the one place the path is read
    assert torch.cuda.is_available(), "row_kernel_bits.py needs a GPU"
    r = Runner(torch.device("cuda:0"))
    for dt in (BF, FP):
        for f in WIDTHS[dt]:
            for rows in ROWS:
                for with_b in (False, True):
                    r.case(f"add_rmsnorm/{NAME[dt]}/f{f}/r{rows}/b{int(with_b)}", add_norm(r, dt, False, rows, f, with_b, False))
                    for with_beta in (False, True):
                        r.case(f"add_layernorm/{NAME[dt]}/f{f}/r{rows}/b{int(with_b)}/beta{int(with_beta)}",
                               add_norm(r, dt, True, rows, f, with_b, with_beta))
    for stem in ("swiglu", "geglu"):
        for dt in (BF, FP):
            for inter in (VEC[dt], 65 * VEC[dt]):
                r.case(f"{stem}/{NAME[dt]}/r3/i{inter}", glu(r, dt, stem, 3, inter))
        # rows * inter / 8 = 2,098,176 chunks > 8192 * 256 threads: the grid is capped and some threads take a second trip
        r.case(f"{stem}/bf16/r2049/i8192", glu(r, BF, stem, 2049, 8192))
    for dt in (BF, FP):
        for case in ROPE_CASES:
            r.case(f"rope64/{NAME[dt]}/{case[0]}", rope64(r, dt, case))
        # 2049 tokens x 8 heads = 16,392 head rows: more than one pass of the 1,024-block backward (16 / 8 rows a block)
        for lead, hq, hkv in (((1, 1), 2, 1), ((1, 3), 2, 1), ((3, 683), 6, 2)):
            for by_pos in (False, True):
                r.case(f"qknorm_rope{'_pos' if by_pos else ''}/{NAME[dt]}/t{lead[0] * lead[1]}/hq{hq}_hkv{hkv}",
                       qknorm_rope(r, dt, lead, hq, hkv, by_pos))
    whole = hashlib.sha256(json.dumps(r.cases, sort_keys=True).encode()).hexdigest()
    res = dict(what="sha256 of every output buffer of the row-kernel entry points (tools/row_kernel_bits.py)",
               cases=len(r.cases), all=whole, digests=r.cases)
    if a.models:
        res["model_level"] = dict(what="sha256 of the valid hidden rows and of all parameter gradients (as fp32) of each *_encode / "
                                       "*_encode_packed, training mode (tools/row_kernel_bits.py --models)", cases=model_level(r.dev))
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(f"{len(r.cases)} cases, all = {whole}" + (f", {len(res['model_level']['cases'])} model cases" if a.models else ""))


if __name__ == "__main__":
    main()
