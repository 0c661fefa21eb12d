"""The relative-position-bias attention kernels (attn_relbias.hip: ``relb::*``) through ``ops.AttentionRelBiasQKV`` against dense
float64 attention with the bias added, autograd giving all four gradients (q, k, v and the bias table).

Shapes: h = 2, d = 64, the fused [q | k | v] buffer.  ``LENS`` = 1, 31, 33, 64, 65, 127, 128, 129, 257: both sides of a wave
(32), of a bf16 key tile (64) and of a workgroup (128), with |rel| = 91 (where MPNet's bucket saturates) inside the longer ones.
  padded  b = 9, l = 257, one key count of ``LENS`` per sequence, M = 257.  EVERY row carries an output gradient and is compared,
          the query rows at or past the key count included (they see the keys below it).
  packed  the same lengths back to back, M = 257.
  long    one sequence of 512 with M = 512 = GMLM_RELBIAS_MAX_LEN: both ends of the table are read.
  bigm    two packed sequences (33, 65) with M = 200: entries outside [-(L - 1), L - 1] = [-64, 64] must be exactly 0.
Dtypes fp32 and bf16, p = 0 and p = 0.1 (masks from ``helpers.attn_dropout_scale`` only).  With dropout in bf16 the length 1 is
replaced by 2, for the reason given in test_gpu_attention_d32.py (one key: P = 1 exactly, and the bf16 rounding of P * keep
alone exceeds the budget).  The table is drawn from N(0, 1): a wrong index or a dropped log2 e factor is off by orders of
magnitude.  The inputs are rounded to bf16 ONCE for both dtypes, so one float64 reference per (mode, p, lengths) serves both.

Budgets.  out, dq, dk, dv: ``test_gpu_attention_matrix._budget`` (fp32 1e-4 max / 1e-5 l2; bf16 2e-2 max, l2 6e-3 out and
8e-3 gradients).  d_rel_bias: the rows of dS sum to zero, so its entries cancel and the error is measured against the norm of
the whole tensor: fp32 1e-5 of it.  bf16 has no fixed number: the bias-gradient kernel itself keeps S, P, dP and dS in fp32
(its q, k, v, dO are the stored bf16 values), and what it inherits is delta = rowsum(dO * O) of an output whose forward fed
bf16 probabilities to the P V product.  ``_dense(..., round_p=True)`` evaluates the dense formula in float64 with bf16(P * D); its error
against the unrounded float64 result is the floor, the kernel must be within 2x of it (as the encoder tests do with HF's bf16
run), and both figures are printed.

Every case asserts the ``relb::`` kernels it launched by name (and that no ``attn_`` kernel ran) and that a second backward on
the same inputs gives identical bits in dq, dk, dv and d_rel_bias."""
import zlib

import pytest
import torch

from helpers import _close, attn_dropout_scale, kernels_run
from test_gpu_attention_matrix import _budget
from test_gpu_decoder_ops import TN, _same_bits

pytestmark = pytest.mark.gpu

BF, FP = torch.bfloat16, torch.float32
H, D, HD = 2, 64, 128
SCALE = D ** -0.5
LENS = (1, 31, 33, 64, 65, 127, 128, 129, 257)
SEED = 0x1234_5678_9ABC
MODES = ("padded", "packed", "long", "bigm")


def expected_kernels(dtype, drop):
    """Bare names of the kernels one forward + backward launches."""
    tn, dr = TN[dtype], "true" if drop else "false"
    return {f"relb::{k}_kernel<{tn}, {dr}>" for k in ("fwd", "dq", "dkv", "dbias")} | {f"relb::delta_kernel<{tn}>", "relb::dbias_sum_kernel"}


ALL_KERNELS = set().union(*(expected_kernels(t, dr) for t in (BF, FP) for dr in (False, True)))


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def _layout(mode, lens):
    """-> (sequences as (first row, query rows, key count), total rows or l, b, M, packed)"""
    if mode == "padded":
        l = max(lens)
        return [(i * l, l, n) for i, n in enumerate(lens)], l, len(lens), l, False
    if mode == "long":
        return [(0, 512, 512)], 512, 1, 512, False
    if mode == "bigm":
        lens = (33, 65)
    starts = [sum(lens[:i]) for i in range(len(lens))]
    return [(s, n, n) for s, n in zip(starts, lens)], sum(lens), len(lens), (200 if mode == "bigm" else max(lens)), True


def _inputs(mode, lens):
    seqs, rows, b, m, packed = _layout(mode, lens)
    g = torch.Generator().manual_seed(zlib.crc32(f"{mode}{lens}".encode()))
    total = rows if packed else b * rows
    qkv = torch.randn(total, 3 * HD, generator=g).bfloat16().float()
    go = torch.randn(total, HD, generator=g).bfloat16().float()
    table = torch.randn(H, 2 * m - 1, generator=g)
    return qkv, go, table


def _slab(mode, seq_index, first_row, hi, rows, total):
    packed = mode in ("packed", "bigm")
    return hi * total + first_row if packed else (seq_index * H + hi) * rows


def _dense(qkv, go, table, n_keys, drop, round_p=False):
    """float64 attention with the bias of ONE sequence: qkv [lq, 3 HD], go [lq, HD], ``n_keys`` visible keys, ``drop`` [H, lq, n]
    multiplier or None -> (out, dq, dk, dv [lq, HD], d_table [H, 2M - 1]).  ``round_p``: the bf16 floor (module docstring): the
    output that enters delta comes from bf16(P * D); the table's gradient is then formed by hand from dS = P (D dP - delta)."""
    lq, m = qkv.shape[0], (table.shape[1] + 1) // 2
    heads = lambda t, rows: t[:rows].double().reshape(rows, H, D).transpose(0, 1).contiguous()
    q, k, v = heads(qkv[:, :HD], lq), heads(qkv[:, HD:2 * HD], n_keys), heads(qkv[:, 2 * HD:], n_keys)
    idx = (m - 1) + torch.arange(n_keys)[None, :] - torch.arange(lq)[:, None]
    g = heads(go, lq)
    if round_p:
        p = torch.softmax((q @ k.transpose(1, 2)) * SCALE + table.double()[:, idx], -1)
        pd = p if drop is None else p * drop
        o = pd.bfloat16().double() @ v
        delta = (g * o).sum(-1, keepdim=True)
        dp = g @ v.transpose(1, 2)
        ds = p * ((dp if drop is None else dp * drop) - delta)
        dt = torch.zeros(H, 2 * m - 1, dtype=torch.float64)
        dt.index_add_(1, idx.flatten(), ds.reshape(H, -1))
        return dt
    q, k, v = (t.requires_grad_(True) for t in (q, k, v))
    tb = table.double().clone().requires_grad_(True)
    p = torch.softmax((q @ k.transpose(1, 2)) * SCALE + tb[:, idx], -1)
    if drop is not None:
        p = p * drop
    o = p @ v
    o.backward(g)
    back = lambda t, rows: torch.cat([t.detach().transpose(0, 1).reshape(rows, HD), torch.zeros(lq - rows, HD, dtype=torch.float64)])
    return back(o, lq), back(q.grad, lq), back(k.grad, n_keys), back(v.grad, n_keys), tb.grad


_REFS = {}


def _reference(mode, lens, p):
    """One float64 reference (and bf16 floor of the table's gradient) per (mode, lengths, p), shared by both dtypes."""
    key = (mode, lens, p)
    if key not in _REFS:
        qkv, go, table = _inputs(mode, lens)
        seqs, rows, b, m, packed = _layout(mode, lens)
        total = qkv.shape[0]
        parts, dt, dt_floor = [[] for _ in range(4)], 0, 0
        for si, (r0, lq, n) in enumerate(seqs):
            drop = None
            if p > 0:
                drop = torch.stack([attn_dropout_scale(SEED, _slab(mode, si, r0, hi, rows, total), lq, n, p) for hi in range(H)])
            res = _dense(qkv[r0:r0 + lq], go[r0:r0 + lq], table, n, drop)
            for acc, t in zip(parts, res[:4]):
                acc.append(t)
            dt = dt + res[4]
            dt_floor = dt_floor + _dense(qkv[r0:r0 + lq], go[r0:r0 + lq], table, n, drop, round_p=True)
        _REFS[key] = [torch.cat(x) for x in parts] + [dt, dt_floor]
    return _REFS[key]


CASES = [(mode, dtype, p) for mode in MODES for dtype in (FP, BF) for p in (0.0, 0.1)]


@pytest.mark.parametrize("mode,dtype,p", CASES, ids=[f"{m}-{'bf16' if t == BF else 'fp32'}-p{p}" for m, t, p in CASES])
def test_relbias_attention_vs_dense_fp64(dev, mode, dtype, p):
    from gmlm_amd import ops
    lens = tuple(2 if (n == 1 and dtype == BF and p > 0) else n for n in LENS)
    seqs, rows, b, m, packed = _layout(mode, lens)
    qkv_h, go_h, table_h = _inputs(mode, lens)
    ref = _reference(mode, lens, p)
    shape = (qkv_h.shape[0],) if packed else (b, rows)
    qkv = qkv_h.to(dev, dtype).reshape(*shape, 3 * HD).requires_grad_(True)
    go = go_h.to(dev, dtype).reshape(*shape, HD)
    table = table_h.to(dev).requires_grad_(True)
    kv_len = torch.tensor([n for _, _, n in seqs], dtype=torch.int32, device=dev) if mode == "padded" else None
    cu = torch.tensor([0] + [r0 + n for r0, _, n in seqs], dtype=torch.int32, device=dev) if packed else None
    max_len = max(n for _, _, n in seqs) if packed else 0

    def run():
        out = ops.AttentionRelBiasQKV.apply(qkv, table, kv_len, H, SCALE, p, SEED, cu, max_len)
        dqkv, dtab = torch.autograd.grad(out, (qkv, table), go)
        return out.detach(), dqkv, dtab

    box = {}
    ran = kernels_run(lambda: box.setdefault("r", run()))
    assert {n for n in ran if n.startswith("relb::")} == expected_kernels(dtype, p > 0), sorted(ran)
    assert not any(n.startswith(("attn_", "d128::", "d32::", "mbert::")) for n in ran), sorted(ran)
    out, dqkv, dtab = box["r"]
    again = run()
    assert _same_bits((again[1],), (dqkv,)) and torch.equal(again[2], dtab) and _same_bits((again[0],), (out,))

    got = [t.detach().cpu().reshape(-1, t.shape[-1]) for t in (out, dqkv[..., :HD], dqkv[..., HD:2 * HD], dqkv[..., 2 * HD:])]
    for name, g_, r_ in zip(("out", "dq", "dk", "dv"), got, ref[:4]):
        assert bool(torch.isfinite(g_).all()), name
        _close(name, g_, r_, *_budget(dtype, name))
    if mode == "padded":                                           # keys past the count: no gradient, exactly
        for (r0, lq, n) in seqs:
            assert float(got[2][r0 + n:r0 + lq].abs().sum()) == 0.0 and float(got[3][r0 + n:r0 + lq].abs().sum()) == 0.0

    dtab = dtab.cpu()
    assert dtab.dtype == torch.float32 and tuple(dtab.shape) == (H, 2 * m - 1) and bool(torch.isfinite(dtab).all())
    r_dt, r_floor = ref[4], ref[5]
    norm = float(r_dt.norm())
    err = float((dtab.double() - r_dt).norm()) / norm
    floor = float((r_floor - r_dt).norm()) / norm
    print(f"  d_rel_bias: err / |ref| = {err:.2e}, bf16 floor = {floor:.2e}")
    if dtype == FP:
        assert err <= 1e-5, err
    else:
        assert err <= 2 * floor, (err, floor)
    longest = max(lq for _, lq, _ in seqs)
    outside = torch.ones(2 * m - 1, dtype=torch.bool)
    outside[m - 1 - (longest - 1):m - 1 + longest] = False
    assert float(dtab[:, outside].abs().sum()) == 0.0 and (mode != "bigm" or int(outside.sum()) == 2 * (200 - 65))
    # both ends of the table are reached by exactly one pair each when a sequence fills it
    if mode == "long":
        assert float(r_dt[:, 0].abs().min()) > 0 and float(dtab[:, 0].abs().min()) > 0 and float(dtab[:, -1].abs().min()) > 0


def test_relbias_operator_refuses_what_the_kernels_do_not_take(dev):
    from gmlm_amd import _lib, ops
    qkv = torch.zeros(1, 40, 3 * HD, device=dev)
    with pytest.raises(_lib.GmlmHipError, match="rel_m"):
        ops.attention_relbias_qkv(qkv, torch.zeros(H, 2 * 39 - 1, device=dev), None, H, SCALE)          # table shorter than the sequence
    with pytest.raises(_lib.GmlmHipError, match="rel_m"):
        ops.attention_relbias_qkv(qkv, torch.zeros(H, 2 * 513 - 1, device=dev), None, H, SCALE)
    with pytest.raises(_lib.GmlmHipError, match="head dim"):
        ops.attention_relbias_qkv(qkv, torch.zeros(4, 2 * 40 - 1, device=dev), None, 4, SCALE)           # d = 32
    with pytest.raises(ValueError):
        ops.attention_relbias_qkv(qkv, torch.zeros(H, 2 * 40, device=dev), None, H, SCALE)               # even width
