"""The disentangled attention kernels (attn_disent.hip: ``disent::*``) through ``ops.AttentionDisentQKV`` against dense float64
attention restated here, independent of HF: scores (q_i . k_j + C[h, i, col[i - j]] + Pt[h, j, col[i - j]]) * scale, autograd
giving all five gradients (q, k, v and the two tables).

Shapes: heads 1 and 3, d = 64, the fused [q | k | v] buffer, two bucket geometries:
  v3    (k = 256, max = 512), lengths 1, 33, 130, 200: one row, a tile edge, the end of the identity region (131), log runs.
  tiny  (k = 16, max = 40), lengths 5, 40, 100: runs of 8 and the clamp past max_relative_positions.
  padded  one sequence per length in [b, l, .] with l = M = the longest, one key count per sequence.  EVERY row carries an
          output gradient and is compared, the query rows at or past the key count included (they see the keys below it).
  packed  the same lengths back to back, M = the longest.
Dtypes fp32 and bf16, p = 0 and p = 0.1 (masks from ``helpers.attn_dropout_scale`` only).  Both tables are drawn from N(0, 8^2):
after the scale 1 / sqrt(3 d) they weigh as much as q . k, so a wrong row, column or factor is off by orders of magnitude.
The inputs are rounded to bf16 ONCE for both dtypes, so one float64 reference per (geometry, heads, mode, p) serves both.

Budgets.  out, dq, dk, dv: ``test_gpu_attention_matrix._budget`` (fp32 1e-4 max / 1e-5 l2; bf16 2e-2 max, l2 6e-3 out and
8e-3 gradients).  d_c2p and d_p2c: the error relative to the norm of the whole tensor; fp32 1e-5 (the gradient l2 budget of the
same function).  bf16 has no fixed number: the table-gradient kernel keeps S, P, dP and dS in fp32 (its q, k, v, dO are the
stored bf16 values), and what it inherits is delta = rowsum(dO * O) of an output whose forward fed bf16(P) times the 0 / 1 mask
to the P V product (the keep scale multiplies the output afterwards).  ``_dense(round_p=True)`` evaluates the dense formula in
float64 with exactly that rounding; its error against the unrounded float64 result is the floor, the kernel must be within 2x
of it, and both figures are printed.
Measured (MI355X, all 32 cases): fp32 out <= 1.0e-7, dq / dk / dv <= 1.6e-6 (max) and 5.2e-7 (l2), d_c2p / d_p2c <= 4.4e-7;
bf16 dq / dk / dv <= 5.4e-3 (max) and 4.1e-3 (l2), d_c2p / d_p2c 2.6e-4 .. 2.0e-3 of the tensor norm against floors of
3.4e-4 .. 3.4e-3: 0.55 .. 1.22 of the floor.

Every case asserts the ``disent::`` kernels it launched by name, that a second forward + backward on the same inputs gives
identical bits everywhere, and that table entries no pair reaches have exactly zero gradients."""
import zlib

import pytest
import torch

from helpers import _close, attn_dropout_scale, kernels_run
from test_gpu_attention_matrix import _budget
from test_gpu_decoder_ops import TN, _same_bits

pytestmark = pytest.mark.gpu

BF, FP = torch.bfloat16, torch.float32
D = 64
SCALE = (3 * D) ** -0.5
GEOMETRIES = {"v3": (256, 512, (1, 33, 130, 200)), "tiny": (16, 40, (5, 40, 100))}
SEED = 0x1234_5678_9ABC
TABLE_STD = 8.0


def expected_kernels(dtype, drop):
    """Bare names of the kernels one forward + backward launches."""
    tn, dr = TN[dtype], "true" if drop else "false"
    return {f"disent::{k}_kernel<{tn}, {dr}>" for k in ("fwd", "dq", "dkv", "dc", "dpt")} | {f"disent::delta_kernel<{tn}>"}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def _layout(mode, lens):
    """-> (sequences as (first row, query rows, key count), l or total rows, b, M, packed)"""
    if mode == "padded":
        l = max(lens)
        return [(i * l, l, n) for i, n in enumerate(lens)], l, len(lens), l, False
    starts = [sum(lens[:i]) for i in range(len(lens))]
    return [(s, n, n) for s, n in zip(starts, lens)], sum(lens), len(lens), max(lens), True


def _columns(geo, m):
    from gmlm_amd import deberta
    k, mx, _ = GEOMETRIES[geo]
    return deberta.bucket_columns(m, k, mx)


def _inputs(geo, h, mode):
    lens = GEOMETRIES[geo][2]
    seqs, rows, b, m, packed = _layout(mode, lens)
    g = torch.Generator().manual_seed(zlib.crc32(f"{geo}{h}{mode}".encode()))
    total = rows if packed else b * rows
    w = _columns(geo, m).width
    qkv = torch.randn(total, 3 * h * D, generator=g).bfloat16().float()
    go = torch.randn(total, h * D, generator=g).bfloat16().float()
    c2p = torch.randn(h, total, w, generator=g) * TABLE_STD
    p2c = torch.randn(h, total, w, generator=g) * TABLE_STD
    return qkv, go, c2p, p2c


def _dense(h, qkv, go, c2p, p2c, col, n_keys, drop, round_p=False):
    """float64 disentangled attention of ONE sequence: qkv [lq, 3 h D], go [lq, h D], c2p / p2c [h, lq, W], col long [2M - 1],
    ``n_keys`` visible keys, ``drop`` [h, lq, n] multiplier or None -> (out, dq, dk, dv [lq, h D], d_c2p, d_p2c [h, lq, W]).
    ``round_p``: the bf16 floor (module docstring): the output that enters delta comes from bf16(P) * D; the tables' gradients
    are then formed by hand from dS = scale * P (D dP - delta)."""
    lq, m, hd = qkv.shape[0], (col.numel() + 1) // 2, h * D
    heads = lambda t, rows: t[:rows].double().reshape(rows, h, D).transpose(0, 1).contiguous()
    q, k, v = heads(qkv[:, :hd], lq), heads(qkv[:, hd:2 * hd], n_keys), heads(qkv[:, 2 * hd:], n_keys)
    idx = col[(m - 1) + torch.arange(lq)[:, None] - torch.arange(n_keys)[None, :]]          # [lq, n]: column of (i, j)
    ci, pi = idx.expand(h, lq, n_keys), idx.t().expand(h, n_keys, lq)
    g = heads(go, lq)
    c, pt = c2p.double().clone(), p2c.double().clone()
    if not round_p:
        q, k, v, c, pt = (t.requires_grad_(True) for t in (q, k, v, c, pt))
    s = (q @ k.transpose(1, 2) + torch.gather(c, 2, ci) + torch.gather(pt[:, :n_keys], 2, pi).transpose(1, 2)) * SCALE
    p = torch.softmax(s, -1)
    if round_p:
        pb = p.bfloat16().double()
        o = (pb if drop is None else pb * drop) @ v
        delta = (g * o).sum(-1, keepdim=True)
        dp = g @ v.transpose(1, 2)
        ds = p * ((dp if drop is None else dp * drop) - delta) * SCALE
        dc, dpt = torch.zeros_like(c), torch.zeros_like(pt)
        dc.scatter_add_(2, ci, ds)
        dpt[:, :n_keys].scatter_add_(2, pi, ds.transpose(1, 2).contiguous())
        return dc, dpt
    if drop is not None:
        p = p * drop
    o = p @ v
    o.backward(g)
    back = lambda t, rows: torch.cat([t.detach().transpose(0, 1).reshape(rows, hd), torch.zeros(lq - rows, hd, dtype=torch.float64)])
    reach_c = torch.zeros(lq, c.shape[2], dtype=torch.bool).scatter_(1, idx, True) if n_keys else torch.zeros(lq, c.shape[2], dtype=torch.bool)
    reach_p = torch.zeros(lq, c.shape[2], dtype=torch.bool)
    if n_keys:
        reach_p[:n_keys].scatter_(1, idx.t().contiguous(), True)
    return back(o, lq), back(q.grad, lq), back(k.grad, n_keys), back(v.grad, n_keys), c.grad, pt.grad, reach_c, reach_p


def _slab(packed, h, seq_index, first_row, hi, rows, total):
    return hi * total + first_row if packed else (seq_index * h + hi) * rows


_REFS = {}


def _reference(geo, h, mode, p):
    """One float64 reference (and bf16 floor of the tables' gradients) per (geometry, heads, mode, p), shared by both dtypes."""
    key = (geo, h, mode, p)
    if key not in _REFS:
        qkv, go, c2p, p2c = _inputs(geo, h, mode)
        seqs, rows, b, m, packed = _layout(mode, GEOMETRIES[geo][2])
        col = _columns(geo, m).col.long()
        total = qkv.shape[0]
        rowwise, tabs = [[] for _ in range(4)], [[] for _ in range(6)]
        for si, (r0, lq, n) in enumerate(seqs):
            drop = None
            if p > 0:
                drop = torch.stack([attn_dropout_scale(SEED, _slab(packed, h, si, r0, hi, rows, total), lq, n, p) for hi in range(h)])
            args = (h, qkv[r0:r0 + lq], go[r0:r0 + lq], c2p[:, r0:r0 + lq], p2c[:, r0:r0 + lq], col, n, drop)
            res = _dense(*args)
            for acc, t in zip(rowwise, res[:4]):
                acc.append(t)
            for acc, t in zip(tabs, res[4:6] + _dense(*args, round_p=True) + res[6:8]):
                acc.append(t)
        _REFS[key] = [torch.cat(x) for x in rowwise] + [torch.cat(x, 1) for x in tabs[:4]] + [torch.cat(x, 0) for x in tabs[4:]]
    return _REFS[key]


CASES = [(geo, h, mode, dtype, p) for geo in GEOMETRIES for h in (1, 3) for mode in ("padded", "packed") for dtype in (FP, BF)
         for p in (0.0, 0.1)]


@pytest.mark.parametrize("geo,h,mode,dtype,p", CASES,
                         ids=[f"{g}-h{h}-{m}-{'bf16' if t == BF else 'fp32'}-p{p}" for g, h, m, t, p in CASES])
def test_disent_attention_vs_dense_fp64(dev, geo, h, mode, dtype, p):
    from gmlm_amd import ops
    hd = h * D
    seqs, rows, b, m, packed = _layout(mode, GEOMETRIES[geo][2])
    qkv_h, go_h, c2p_h, p2c_h = _inputs(geo, h, mode)
    ref = _reference(geo, h, mode, p)
    cols = _columns(geo, m)
    shape = (qkv_h.shape[0],) if packed else (b, rows)
    qkv = qkv_h.to(dev, dtype).reshape(*shape, 3 * hd).requires_grad_(True)
    go = go_h.to(dev, dtype).reshape(*shape, hd)
    c2p, p2c = c2p_h.to(dev).requires_grad_(True), p2c_h.to(dev).requires_grad_(True)
    col = cols.col.to(dev)
    kv_len = None if packed else torch.tensor([n for _, _, n in seqs], dtype=torch.int32, device=dev)
    cu = torch.tensor([0] + [r0 + n for r0, _, n in seqs], dtype=torch.int32, device=dev) if packed else None
    max_len = max(n for _, _, n in seqs) if packed else 0

    def run():
        out = ops.AttentionDisentQKV.apply(qkv, c2p, p2c, col, kv_len, h, SCALE, p, SEED, cu, max_len)
        return (out.detach(),) + torch.autograd.grad(out, (qkv, c2p, p2c), go)

    box = {}
    ran = kernels_run(lambda: box.setdefault("r", run()))
    assert {n for n in ran if n.startswith("disent::")} == expected_kernels(dtype, p > 0), sorted(ran)
    assert not any(n.startswith(("attn_", "d128::", "d32::", "mbert::", "relb::")) for n in ran), sorted(ran)
    out, dqkv, dc, dpt = box["r"]
    again = run()
    assert _same_bits(again[:2], (out, dqkv)) and torch.equal(again[2], dc) and torch.equal(again[3], dpt)

    got = [t.detach().cpu().reshape(-1, t.shape[-1]) for t in (out, dqkv[..., :hd], dqkv[..., hd:2 * hd], dqkv[..., 2 * hd:])]
    for name, g_, r_ in zip(("out", "dq", "dk", "dv"), got, ref[:4]):
        assert bool(torch.isfinite(g_).all()), name
        _close(name, g_, r_, *_budget(dtype, name))
    if not packed:                                                 # keys past the count: no gradient, exactly
        for (r0, lq, n) in seqs:
            assert float(got[2][r0 + n:r0 + lq].abs().sum()) == 0.0 and float(got[3][r0 + n:r0 + lq].abs().sum()) == 0.0

    r_dc, r_dpt, f_dc, f_dpt, reach_c, reach_p = ref[4:]
    for name, g_, r_, f_, reach in (("d_c2p", dc.cpu(), r_dc, f_dc, reach_c), ("d_p2c", dpt.cpu(), r_dpt, f_dpt, reach_p)):
        assert g_.dtype == torch.float32 and g_.shape == r_.shape and bool(torch.isfinite(g_).all()), name
        norm = float(r_.norm())
        err = float((g_.double() - r_).norm()) / norm
        floor = float((f_ - r_).norm()) / norm
        print(f"  {name}: err / |ref| = {err:.2e}, bf16 floor = {floor:.2e}")
        if dtype == FP:
            assert err <= _budget(FP, "dq")[1], (name, err)
        else:
            assert err <= 2 * floor, (name, err, floor)
        assert float(g_[:, ~reach].abs().sum()) == 0.0, name        # entries no pair reaches: exact zeros, written by the kernel
        assert int((~reach).sum()) > 0


def test_disent_operator_refuses_what_the_kernels_do_not_take(dev):
    from gmlm_amd import _lib, ops
    h, l = 2, 40
    qkv = torch.zeros(1, l, 3 * h * D, device=dev)
    tab = lambda heads, w: torch.zeros(heads, l, w, device=dev)
    col = lambda m_: torch.zeros(2 * m_ - 1, dtype=torch.int32, device=dev)
    with pytest.raises(_lib.GmlmHipError, match="col_m"):
        ops.attention_disent_qkv(qkv, tab(h, 8), tab(h, 8), col(39), None, h, SCALE)             # col shorter than the sequence
    with pytest.raises(_lib.GmlmHipError, match="col_m"):
        ops.attention_disent_qkv(qkv, tab(h, 8), tab(h, 8), col(513), None, h, SCALE)
    with pytest.raises(_lib.GmlmHipError, match="tab_w"):
        ops.attention_disent_qkv(qkv, tab(h, 80), tab(h, 80), col(40), None, h, SCALE)           # more columns than distances
    with pytest.raises(_lib.GmlmHipError, match="head dim"):
        ops.attention_disent_qkv(qkv, tab(4, 8), tab(4, 8), col(40), None, 4, SCALE)             # d = 32
    with pytest.raises(ValueError):
        ops.attention_disent_qkv(qkv, tab(h, 8), tab(h, 9), col(40), None, h, SCALE)             # two widths
    with pytest.raises(ValueError):
        ops.attention_disent_qkv(qkv, tab(h, 8).transpose(0, 1), tab(h, 8).transpose(0, 1), col(40), None, h, SCALE)   # [rows, h, W]
    with pytest.raises(ValueError):
        ops.attention_disent_qkv(qkv, tab(h, 8), tab(h, 8), col(40).long(), None, h, SCALE)      # int64 columns
