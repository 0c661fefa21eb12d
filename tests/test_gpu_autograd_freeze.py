"""Every autograd node under frozen inputs, on the device, against float64.

The builders are those of tests/test_autograd_contract_cpu.py at the smallest shapes that still take each kernel path.  The
float64 gradient of an input does not depend on which other inputs are frozen, so one float64 reference per (spec, dtype,
incoming gradient) serves every freeze pattern.  Per pattern: the gradients of the unfrozen inputs are within the node's
budget of float64 and bit-identical to the all-trainable run's; the set of the project's kernels the pattern launched
(helpers.kernels_run) is the all-trainable run's set, less at most the bias column-sum kernels when no bias master needs a
gradient (they feed no other gradient); frozen inputs have no gradient.  Per spec also: the forward under
``torch.no_grad()`` and in grad mode with nothing requiring grad (every bf16 forward without its ``out_lo``), a non-contiguous,
an expanded and (bf16) an fp32 incoming gradient, and for nodes with two outputs each output used alone.

Budgets are the tree's own: test_gpu_attention_matrix._budget for attention outputs and gradients (the bias masters of
AttentionQKV, column sums of dqkv, included), the 2x bf16 floor of test_gpu_mpnet_kernels / test_gpu_deberta_kernels for the
table gradients (``_dense(..., round_p=True)`` of those modules gives the floor), test_gpu_norm_matrix's FP32_BUDGET and bf16
ulp checks with its stated extras for the norm-family nodes, test_gpu_decoder_ops._rel_l2 for the decoder-family nodes and the
fp32 GEMMs, and test_gpu_split_gemm's rule for bf16x3 (at most 1/32 of the plain bf16 error).  The bf16 GEMM nodes have no
budget in the tree at these shapes (K = 8, a gradient of ones: sums that cancel); ``c_gemm`` and ``c_scaled`` derive theirs from
the number format and say how.  A gradient whose float64 value is exactly zero (an output nobody used) must be exactly zero.

One place is not value-checked, by the nodes' design: the second output of _RopeAttention / _RopeCausalGQA (the rewritten
input, returned only because autograd wants a dirty input back: its incoming gradient is ignored) is never used alone.  The
"fp32 gradient" form hands fp32 ``grad_tensors`` to a bf16 output: the engine casts them to the output's dtype before the node
runs, so it checks that route, not the nodes' own ``.to(dtype)``."""
from dataclasses import dataclass
from typing import Callable

import pytest
import torch
import torch.nn.functional as F

import test_autograd_contract_cpu as T
import test_gpu_deberta_kernels as DK
import test_gpu_mpnet_kernels as MK
from helpers import _close, attn_dropout_scale, elem_dropout_scale, kernels_run
from test_gpu_attention_matrix import _budget
from test_gpu_decoder_ops import _rel_l2, _same_bits
from test_gpu_norm_matrix import FP32_BUDGET, _col_rms, _erf_floor, _erf_grad_floor, _row_rms, _ulp_check

pytestmark = pytest.mark.gpu

BF, FP = torch.bfloat16, torch.float32
SEED = 0x1234_5678_9ABC
# the only kernels a freeze pattern may leave out without any gradient changing: the bias column sums nobody asked for
BIAS_SUM_KERNELS = ("col_reduce_partial_kernel<2, gmlm::ColStatsFn<", "rows_sum_kernel")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


# ------------------------------------------------------------------------------------------------------ float64 references
def _rot(x, cs, pos):
    """rotate-half rotation of x [rows, heads, d] at positions pos [rows]; cs fp32 [max_len, 2, d / 2]"""
    half = x.shape[-1] // 2
    c, s = cs[pos.long(), 0].double()[:, None, :], cs[pos.long(), 1].double()[:, None, :]
    lo, hi = x[..., :half], x[..., half:]
    return torch.cat([lo * c - hi * s, hi * c + lo * s], -1)


def _seqs(meta):
    lens = meta["lens"]
    if meta["packed"]:
        starts = [sum(lens[:i]) for i in range(len(lens))]
        return [(s, n, n) for s, n in zip(starts, lens)], sum(lens)
    l = max(lens)
    return [(i * l, l, n) for i, n in enumerate(lens)], l * len(lens)


def _positions(meta):
    seqs, total = _seqs(meta)
    pos = torch.zeros(total, dtype=torch.long)
    for r0, lq, _ in seqs:
        pos[r0:r0 + lq] = torch.arange(lq)
    return pos


def _attend(q, k, v, seqs, hq, hkv, d, scale, causal=False, window=None, bias=None, drop=None):
    """float64 attention of flattened rows, one sequence at a time: q [R, hq d], k / v [R, hkv d]; a sequence is (first row,
    query rows, visible keys).  ``bias(si, lq, n)`` -> [hq, lq, n] added to the scaled scores, ``drop(si, hi, lq, n)`` -> the
    [lq, n] multiplier of the probabilities."""
    parts = []
    for si, (r0, lq, n) in enumerate(seqs):
        qh = q[r0:r0 + lq].reshape(lq, hq, d).transpose(0, 1)
        kh = k[r0:r0 + n].reshape(n, hkv, d).transpose(0, 1).repeat_interleave(hq // hkv, 0)
        vh = v[r0:r0 + n].reshape(n, hkv, d).transpose(0, 1).repeat_interleave(hq // hkv, 0)
        s = qh @ kh.transpose(1, 2) * scale
        if bias is not None:
            s = s + bias(si, lq, n)
        i, j = torch.arange(lq)[:, None], torch.arange(n)[None, :]
        keep = torch.ones(lq, n, dtype=torch.bool)
        if causal:
            keep &= j <= i
        if window is not None:
            keep &= (i - j).abs() <= window
        alive = keep.any(-1, keepdim=True)                     # a row without a visible key: zero output, zero gradients
        s = torch.where(alive, s.masked_fill(~keep, float("-inf")), torch.zeros_like(s))
        p = torch.softmax(s, -1) * alive
        if drop is not None:
            p = p * torch.stack([drop(si, hi, lq, n) for hi in range(hq)])
        parts.append((p @ vh).transpose(0, 1).reshape(lq, hq * d))
    assert [r0 for r0, _, _ in seqs] == [sum(x[1] for x in seqs[:i_]) for i_ in range(len(seqs))]      # the sequences tile the rows
    return torch.cat(parts)


def r_attention(L, m):
    b, lq, hd = L["q"].shape
    lk, h, d = L["k"].shape[1], m["h"], m["d"]
    kv = m["kv_len"] or (lk,) * b
    outs = []
    for bi in range(b):
        drop = None
        if m["p"]:
            drop = lambda si, hi, lq_, n, bi=bi: attn_dropout_scale(m["seed"], (bi * h + hi) * lq, lq, lk, m["p"])[:, :n]
        outs.append(_attend(L["q"][bi], L["k"][bi], L["v"][bi], [(0, lq, kv[bi])], h, h, d, d ** -0.5, drop=drop))
    return (torch.stack(outs),)


def r_attention_qkv(L, m):
    qkv, h, d = L["qkv"], m["h"], m["d"]
    hd = h * d
    if "bq" in L:                                       # the masters' gradient: the column sums of dqkv; their values are not read
        bcat = torch.cat([L["bq"], L["bk"], L["bv"]])
        qkv = qkv + (bcat - bcat.detach())
    flat = qkv.reshape(-1, 3 * hd)
    seqs, total = _seqs(m)
    drop = None
    if m["p"]:
        if m["packed"]:
            drop = lambda si, hi, lq, n: attn_dropout_scale(m["seed"], hi * total + seqs[si][0], n, n, m["p"])
        else:
            drop = lambda si, hi, lq, n: attn_dropout_scale(m["seed"], (si * h + hi) * lq, lq, lq, m["p"])[:, :n]
    out = _attend(flat[:, :hd], flat[:, hd:2 * hd], flat[:, 2 * hd:], seqs, h, h, d, m.get("scale", d ** -0.5), drop=drop)
    return (out.reshape(*L["qkv"].shape[:-1], hd),)


def _qkv_drop(m):
    """the mask of AttentionQKV's relatives: slab (sequence * h + head) * l padded, head * total rows + first row packed"""
    if not m["p"]:
        return None
    seqs, total = _seqs(m)
    h = m["h"]
    if m["packed"]:
        return lambda si, hi, lq, n: attn_dropout_scale(m["seed"], hi * total + seqs[si][0], lq, n, m["p"])
    return lambda si, hi, lq, n: attn_dropout_scale(m["seed"], (si * h + hi) * lq, lq, n, m["p"])


def _drop_stack(m, si, lq, n):
    d = _qkv_drop(m)
    return None if d is None else torch.stack([d(si, hi, lq, n) for hi in range(m["h"])])


def r_relbias(L, m):
    h, hd, mm = m["h"], m["h"] * 64, m["m"]
    flat = L["qkv"].reshape(-1, 3 * hd)
    seqs, total = _seqs(m)

    def bias(si, lq, n):
        idx = (mm - 1) + torch.arange(n)[None, :] - torch.arange(lq)[:, None]
        return L["rel_bias"][:, idx]
    out = _attend(flat[:, :hd], flat[:, hd:2 * hd], flat[:, 2 * hd:], seqs, h, h, 64, m["scale"], bias=bias, drop=_qkv_drop(m))
    return (out.reshape(*L["qkv"].shape[:-1], hd),)


def r_disent(L, m):
    h, hd, mm, col = m["h"], m["h"] * 64, m["m"], m["col"].cpu().long()
    flat = L["qkv"].reshape(-1, 3 * hd)
    seqs, total = _seqs(m)

    def bias(si, lq, n):
        r0 = seqs[si][0]
        idx = col[(mm - 1) + torch.arange(lq)[:, None] - torch.arange(n)[None, :]]
        c = torch.gather(L["c2p"][:, r0:r0 + lq], 2, idx.expand(h, lq, n))
        pt = torch.gather(L["p2c"][:, r0:r0 + n], 2, idx.t().expand(h, n, lq)).transpose(1, 2)
        return (c + pt) * m["scale"]
    out = _attend(flat[:, :hd], flat[:, hd:2 * hd], flat[:, 2 * hd:], seqs, h, h, 64, m["scale"], bias=bias, drop=_qkv_drop(m))
    return (out.reshape(*L["qkv"].shape[:-1], hd),)


def r_causal(L, m):
    hq, hkv, d = m["hq"], m["hkv"], m["d"]
    seqs, _ = _seqs(m)
    out = _attend(L["q"].reshape(-1, hq * d), L["k"].reshape(-1, hkv * d), L["v"].reshape(-1, hkv * d), seqs, hq, hkv, d, d ** -0.5,
                  causal=not m["bidir"])
    return (out.reshape(*L["q"].shape[:-1], hq * d),)


def _headnorm_rope(L, m):
    """-> (q, k) rotated and head-normalised [R, heads * 128], v [R, hkv * 128]"""
    hq, hkv = m["hq"], m["hkv"]
    flat = L["qkv"].reshape(-1, (hq + 2 * hkv) * 128)
    pos = _positions(m)
    res = []
    for x, w, heads in ((flat[:, :hq * 128], L["qw"], hq), (flat[:, hq * 128:(hq + hkv) * 128], L["kw"], hkv)):
        xh = x.reshape(-1, heads, 128)
        xh = xh * (xh.pow(2).mean(-1, keepdim=True) + m["eps"]).rsqrt() * w
        res.append(_rot(xh, m["cs"].cpu(), pos).reshape(-1, heads * 128))
    return res[0], res[1], flat[:, (hq + hkv) * 128:]


def r_rope_causal(L, m):
    q, k, v = _headnorm_rope(L, m)
    seqs, _ = _seqs(m)
    out = _attend(q, k, v, seqs, m["hq"], m["hkv"], 128, 128 ** -0.5, causal=True)
    return (out.reshape(*L["qkv"].shape[:-1], m["hq"] * 128),)


def r_qknorm_rope(L, m):
    q, k, _ = _headnorm_rope(L, m)
    return (torch.cat([q, k], -1).reshape(*L["qkv"].shape[:-1], -1),)


def _rope_qk(L, m, hq, hkv, d):
    flat = L["qkv"].reshape(-1, (hq + 2 * hkv) * d)
    qk = _rot(flat[:, :(hq + hkv) * d].reshape(-1, hq + hkv, d), m["cs"].cpu(), _positions(m)).reshape(-1, (hq + hkv) * d)
    return torch.cat([qk, flat[:, (hq + hkv) * d:]], -1)


def r_rope_attention(L, m):
    h = m["h"]
    rot = _rope_qk(L, m, h, h, 64)
    seqs, _ = _seqs(m)
    out = _attend(rot[:, :h * 64], rot[:, h * 64:2 * h * 64], rot[:, 2 * h * 64:], seqs, h, h, 64, 0.125, window=m["window"])
    return out.reshape(*L["qkv"].shape[:-1], h * 64), rot.reshape(L["qkv"].shape)


def r_rope_gqa(L, m):
    hq, hkv, d = m["hq"], m["hkv"], m["d"]
    rot = _rope_qk(L, m, hq, hkv, d)
    seqs, _ = _seqs(m)
    out = _attend(rot[:, :hq * d], rot[:, hq * d:(hq + hkv) * d], rot[:, (hq + hkv) * d:], seqs, hq, hkv, d, d ** -0.5,
                  causal=not m["bidir"])
    return out.reshape(*L["qkv"].shape[:-1], hq * d), rot.reshape(L["qkv"].shape)


def _elem_mask(m, shape):
    if not m["p"]:
        return None
    n = shape[0] * shape[1]
    return elem_dropout_scale(m["seed"], torch.arange(n, dtype=torch.int64), m["p"]).view(shape).double()


def r_bias_res_ln(L, m):
    z = L["x"] + L["bias"]
    mask = _elem_mask(m, z.shape)
    if mask is not None:
        z = z * mask
    z = z + L["res"]
    mu = z.mean(-1, keepdim=True)
    rs = ((z - mu).pow(2).mean(-1, keepdim=True) + m["eps"]).rsqrt()
    t = (z - mu) * rs * L["gamma"] + L["beta"]
    m["aux"] = dict(t=t.detach(), rs=rs.detach(), gamma=L["gamma"].detach(), mask=mask)
    return (F.gelu(t) if m["act"] else t,)


def r_add_norm(L, m):
    s = L["a"] + L["b"] if "b" in L else L["a"] * 1
    if m["ln"]:
        y = F.layer_norm(s, s.shape[-1:], L["w"], L.get("beta"), m["eps"])
    else:
        y = s * (s.pow(2).mean(-1, keepdim=True) + m["eps"]).rsqrt() * L["w"]
    return s, y


def r_graphnorm(L, m):
    z = L["z"]
    o = z - z.mean(0) * L["mean_scale"]
    t = L["weight"] * o * (o.pow(2).mean(0) + m["eps"]).rsqrt() + L["bias"]
    y = F.gelu(t) if m["act"] else t
    mask = _elem_mask(m, z.shape)
    m["aux"] = dict(t=t.detach(), mask=mask)
    return (y if mask is None else y * mask,)


def r_bias_gelu(L, m):
    t = L["x"] + L["bias"]
    m["aux"] = dict(t=t.detach())
    return (F.gelu(t),)


def r_glu(L, m):
    gate, up = L["gu"].chunk(2, -1)
    return ((F.silu(gate) if m["stem"] == "swiglu" else F.gelu(gate)) * up,)


def r_embed_sum(L, m):
    return (L["word"][m["tok"].cpu()] + L["type"][0] + L["pos"][m["pos_ids"].cpu()],)


def r_softmask(L, m):
    x, mask, beta = m["x"].cpu().double(), m["mask"].cpu(), m["beta"]
    out = torch.where(mask[:, None], (1 - beta) * x + beta * L["token"], x)
    return (F.pad(out, (0, m["out_cols"] - out.shape[1])),)


def r_meanpool(L, m):
    seqs, _ = _seqs(m)
    flat = L["hs"].reshape(-1, L["hs"].shape[-1])
    means = torch.stack([flat[r0:r0 + n].sum(0) / n for r0, _, n in seqs])
    return (L["plm_embeds"].index_copy(0, m["idx"].cpu(), means),)


def r_rgcn(L, m):
    src, dst, et = m["edges"]
    n, x = m["n"], L["x"]
    blocks = []
    for r in range(2):
        a = torch.zeros(n, n, dtype=torch.float64)
        a.index_put_((dst[et == r], src[et == r]), torch.ones(int((et == r).sum()), dtype=torch.float64), accumulate=True)
        blocks.append((a / a.sum(1, keepdim=True).clamp_min(1)) @ x)
    return (torch.cat(blocks, 1),)


def r_root_addmm(L, m):
    return (L["bias"] + L["x"][:, :L["root"].shape[0]] @ L["root"],)


def r_select_rows(L, m):
    return (L["x"][m["idx"].cpu()],)


def r_basis(L, m):
    return (L["comp"] @ L["weight"],)


def r_split_last(L, m):
    return L["x"][..., :m["c"]], L["x"][..., m["c"]:]


def r_scaled_projection(L, m):
    return (sum(L["weights"][i] * (L[f"emb{i}"] @ L[f"w{i}"].t() + L[f"b{i}"]) for i in range(m["k"])),)


def r_linear(L, m):
    k = len(m["ns"])
    w = torch.cat([L[f"w{i}"] for i in range(k)])
    b = torch.cat([L[f"b{i}"] for i in range(k)]) if m["bias_grad"] else torch.cat(m["bfix"]).cpu().double()
    y = L["x"] @ w.t() + b
    return (y, L["x"] * 1) if m["residual"] else (y,)


def r_bias_table(L, m):
    return (L["weight"][m["bucket"].cpu()].t(),)


def r_tables(L, m):
    h, d = m["h"], m["d"]
    q3, r3 = L["qkv"].reshape(-1, 3, h, d), L["qkr"].reshape(-1, 2, h, d)
    return (q3[:, 0].permute(1, 0, 2) @ r3[:, 1].permute(1, 2, 0), q3[:, 1].permute(1, 0, 2) @ r3[:, 0].permute(1, 2, 0))


# ------------------------------------------------------------------------------------------------------------- budget classes
def c_attn(name, got, ref, dt, spec, env):
    if name == "dbk":
        # the key bias shifts every score of a query row alike: its gradient, the column sums of dk, is zero in exact arithmetic
        # and has no relative error.  The sum over R rows of a dk within the l2 budget is off by at most sqrt(R) * budget * |dk|.
        dk = env["ref"]["dqkv"].reshape(-1, 3 * ref.numel())[:, ref.numel():2 * ref.numel()]
        err, lim = float((got.double().cpu() - ref).norm()), dk.shape[0] ** 0.5 * _budget(dt, "dq")[1] * float(dk.norm())
        print(f"  dbk: |err| = {err:.2e}, bound {lim:.2e} (|float64 dbk| = {float(ref.norm()):.2e})")
        assert float(ref.norm()) <= 1e-9 * float(dk.norm()) and err <= lim, (err, lim)
        return
    _close(name, got.cpu(), ref, *_budget(dt, "out" if name.startswith("out") else "dq"))


def c_table(name, got, ref, dt, spec, env):
    """fp32: the modules' 1e-5 of the tensor norm; bf16: within 2x of the floor ``_dense(..., round_p=True)`` gives"""
    err = float((got.double().cpu() - ref).norm()) / float(ref.norm())
    if dt == FP:
        print(f"  {name}: err / |ref| = {err:.2e}")
        assert err <= 1e-5, (name, err)
        return
    floor = float((env["floor"][name] - ref).norm()) / float(ref.norm())
    print(f"  {name}: err / |ref| = {err:.2e}, bf16 floor = {floor:.2e}")
    assert err <= 2 * floor, (name, err, floor)


def c_f32(name, got, ref, dt, spec, env):
    _close(name, got.cpu(), ref, *FP32_BUDGET)


def c_l2(name, got, ref, dt, spec, env):
    _rel_l2(name, got.cpu(), ref, dt)


def c_x3(name, got, ref, dt, spec, env):
    """test_gpu_split_gemm: at most 1/32 of the relative L2 error of the plain bf16 GEMM (here: of float64 on operands rounded to bf16)"""
    e3 = float((got.double().cpu() - ref).norm() / ref.norm())
    e1 = float((env["plain"][name] - ref).norm() / ref.norm())
    print(f"  {name}: rel L2 bf16x3 {e3:.2e}, plain bf16 {e1:.2e}")
    assert e3 <= e1 / 32, (name, e3, e1)


def c_gemm(name, got, ref, dt, spec, env):
    """fp32: _rel_l2.  bf16: the operands of the GEMMs are the fp32 masters rounded to bf16 and the result is rounded to bf16
    once: within 2x the error float64 makes on leaves rounded to bf16 (the floor of the format, as the encoder tests take HF's
    bf16 run) plus 2^-8 of the tensor norm (twice the half-ulp of the stored result).  At these shapes (K = 8, a gradient of
    ones) sums cancel, so a bound relative to the result alone does not follow from the format."""
    if dt == FP:
        return _rel_l2(name, got.cpu(), ref, dt)
    err, floor, norm = float((got.double().cpu() - ref).norm()), float((env["plain"][name] - ref).norm()), float(ref.norm())
    print(f"  {name}: |err| / |ref| = {err / norm:.2e}, bf16 floor {floor / norm:.2e}")
    assert err <= 2 * floor + 2.0 ** -8 * norm, (name, err, floor, norm)


def c_scaled(name, got, ref, dt, spec, env):
    """_ScaledProjectionSum / Cat.  The scalar weights' gradient in bf16: d_weights[i] = sum(dW_i * W_i) + sum(gsum * b_i), a sum
    with cancellation of products whose factor dW_i = g^T e_i left its GEMM rounded to bf16 (relative 2^-9 per entry, 2^-8 with
    the products' own rounding): |err| <= 2^-8 * (sum |dW_i| |W_i| + sum |gsum| |b_i|)."""
    if name != "dweights" or dt == FP:
        return c_gemm(name, got, ref, dt, spec, env)
    l, g = env["leaves64"], env["gouts"][0]
    k = env["meta"]["k"]
    mag = torch.stack([((g.t() @ l[f"emb{i}"]).abs() * l[f"w{i}"].abs()).sum() + (g.sum(0).abs() * l[f"b{i}"].abs()).sum() for i in range(k)])
    err = (got.double().cpu() - ref).abs()
    print(f"  dweights: max err / bound = {float((err / (2.0 ** -8 * mag)).max()):.2f}")
    assert bool((err <= 2.0 ** -8 * mag).all()), (err, mag)


def _norm_family(extra):
    """fp32: FP32_BUDGET; bf16: fp32 parameter gradients FP32_BUDGET, bf16 tensors one ulp + ``extra(name, env)`` (None: plain ulp)"""
    def check(name, got, ref, dt, spec, env):
        if got.dtype == FP:
            return _close(name, got.cpu(), ref, *FP32_BUDGET)
        _ulp_check(name, got.cpu(), ref, extra(name, env) if extra else None)
    return check


def _ln_extra(name, env):
    a, g = env["aux"], env["gouts"][0]
    act = env["meta"]["act"]
    if name == "out0":
        return 2.0 ** -16 * _row_rms(a["t"]) + (_erf_floor(a["t"]) if act else 0.0)
    dyn = g * (torch.autograd.functional.vjp(F.gelu, a["t"], torch.ones_like(a["t"]))[1] if act else 1.0)
    return 2.0 ** -15 * a["rs"] * _row_rms(dyn * a["gamma"])


def _gn_extra(name, env):
    a = env["aux"]
    if name == "out0":
        ks = a["mask"] if a["mask"] is not None else 1.0
        return 2.0 ** -16 * _col_rms(a["t"]) + (_erf_floor(a["t"]) * ks if env["meta"]["act"] else 0.0)
    return 2.0 ** -15 * _col_rms(env["ref"]["dz"])


def _bg_extra(name, env):
    t = env["aux"]["t"]
    return _erf_floor(t) if name == "out0" else _erf_grad_floor(t, env["gouts"][0])


def _softmask_extra(name, env):
    m = env["meta"]
    x = m["x"].cpu().double()
    e = 2.0 ** -22 * ((1 - m["beta"]) * x.abs() + m["beta"] * env["leaves64"]["token"].abs())
    return F.pad(e, (0, m["out_cols"] - e.shape[1]))


def _embed_extra(name, env):
    m, l = env["meta"], env["leaves64"]
    return 2.0 ** -23 * (l["word"][m["tok"].cpu()].abs() + l["type"][0].abs() + l["pos"][m["pos_ids"].cpu()].abs())


# ---------------------------------------------------------------------------------------------------------------------- specs
@dataclass
class Spec:
    id: str
    build: Callable               # (dev, dtype) -> T.Case
    ref: Callable                 # ({name: float64 leaf}, meta) -> tuple of float64 outputs
    check: Callable
    dtypes: tuple = (BF, FP)
    kernels: tuple = ()           # substrings of kernel names that must have run (bf16)
    use_alone: tuple = ()         # outputs of a two-output node that are also used alone
    floor: Callable = None        # bf16 floor of the table gradients
    cls: str = ""
    primary: int = None           # the one output whose gradient the node takes (the in-place nodes ignore the other's)


L33, L65 = (33, 20), (65, 33)
SHORT64 = tuple(8 for _ in range(64))                   # 64 sequences x 8 heads = 512 pairs: the _short_path threshold
SHORT32 = tuple(8 for _ in range(8))                    # 8 sequences x 12 heads = D32_SHORT_MIN_PAIRS
GQA_SHORT = tuple(8 for _ in range(128))                # 128 sequences x 4 query heads = 512 pairs


def _mk_floor(L, m, gouts):
    """test_gpu_mpnet_kernels._dense(round_p=True), one sequence at a time (its H, D and SCALE are this spec's)"""
    seqs, _ = _seqs(m)
    flat, go = L["qkv"].reshape(-1, 3 * MK.HD), gouts[0].reshape(-1, MK.HD)
    return {"drel_bias": sum(MK._dense(flat[r0:r0 + lq], go[r0:r0 + lq], L["rel_bias"], n, _drop_stack(m, si, lq, n), round_p=True)
                             for si, (r0, lq, n) in enumerate(seqs))}


def _dk_floor(L, m, gouts):
    h = m["h"]
    seqs, _ = _seqs(m)
    flat, go = L["qkv"].reshape(-1, 3 * h * 64), gouts[0].reshape(-1, h * 64)
    dc, dpt = torch.zeros_like(L["c2p"]), torch.zeros_like(L["p2c"])
    for si, (r0, lq, n) in enumerate(seqs):
        a, b = DK._dense(h, flat[r0:r0 + lq], go[r0:r0 + lq], L["c2p"][:, r0:r0 + lq], L["p2c"][:, r0:r0 + lq], m["col"].cpu().long(), n,
                         _drop_stack(m, si, lq, n), round_p=True)
        dc[:, r0:r0 + lq], dpt[:, r0:r0 + lq] = a, b
    return {"dc2p": dc, "dp2c": dpt}


def _table_or_attn(name, got, ref, dt, spec, env):
    (c_table if name in ("drel_bias", "dc2p", "dp2c") else c_attn)(name, got, ref, dt, spec, env)


def _rope_causal_check(name, got, ref, dt, spec, env):
    (c_l2 if name in ("dqw", "dkw") else c_attn)(name, got, ref, dt, spec, env)


def _rope_check(name, got, ref, dt, spec, env):
    (c_l2 if name == "out1" else c_attn)(name, got, ref, dt, spec, env)


def _A(id_, build, ref, check=c_attn, **kw):
    return Spec(id_, build, ref, check, cls="attention", **kw)


SPECS = [
    # streaming attention families: b = 2, h = 2, one key-tile edge, at every head-dim family
    *[_A(f"Attention-d{d}-L{ln[0]}", T._v(T.b_attention, b=2, h=2, lq=ln[0], lk=ln[0], d=d, kv_len=ln), r_attention)
      for d in (32, 64, 128, 256) for ln in (L33, L65)],
    _A("Attention-d64-cross-drop", T._v(T.b_attention, b=2, h=2, lq=33, lk=65, d=64, p=0.3, seed=SEED), r_attention),
    *[_A(f"AttentionQKV-d{d}-L{ln[0]}", T._v(T.b_attention_qkv, h=2, d=d, lens=ln, mode="padded"), r_attention_qkv)
      for d in (32, 64) for ln in (L33, L65)],
    _A("AttentionQKV-d64-packed-drop", T._v(T.b_attention_qkv, h=2, d=64, lens=L65, mode="packed", p=0.3, seed=SEED), r_attention_qkv),
    _A("AttentionQKV-d64-short-groups", T._v(T.b_attention_qkv, h=8, d=64, lens=SHORT64, mode="groups"), r_attention_qkv, dtypes=(BF,),
       kernels=("attn_fwd_short_kernel", "attn_bwd_short_kernel")),
    _A("AttentionQKV-d32-short-groups", T._v(T.b_attention_qkv, h=12, d=32, lens=SHORT32, mode="groups"), r_attention_qkv, dtypes=(BF,),
       kernels=("d32s::fwd_kernel", "d32s::bwd_kernel")),
    _A("AttentionRelBiasQKV-padded", T._v(T.b_relbias, h=MK.H, lens=L65, scale=MK.SCALE), r_relbias, _table_or_attn, floor=_mk_floor),
    _A("AttentionRelBiasQKV-packed", T._v(T.b_relbias, h=MK.H, lens=L65, packed=True, scale=MK.SCALE), r_relbias, _table_or_attn,
       floor=_mk_floor),
    _A("AttentionRelBiasQKV-padded-drop", T._v(T.b_relbias, h=MK.H, lens=L65, scale=MK.SCALE, p=0.1, seed=SEED), r_relbias, _table_or_attn,
       floor=_mk_floor),
    _A("AttentionDisentQKV-packed-drop", T._v(T.b_disent, h=2, lens=L65, w=8, packed=True, scale=DK.SCALE, p=0.1, seed=SEED), r_disent,
       _table_or_attn, floor=_dk_floor),
    _A("AttentionDisentQKV-padded", T._v(T.b_disent, h=2, lens=L65, w=8, scale=DK.SCALE), r_disent, _table_or_attn, floor=_dk_floor),
    _A("AttentionDisentQKV-packed", T._v(T.b_disent, h=2, lens=L65, w=8, packed=True, scale=DK.SCALE), r_disent, _table_or_attn,
       floor=_dk_floor),
    # grouped KV heads: hq = 4, hkv = 2 at d = 64 and 128, causal and bidirectional, padded and packed, and the short route
    *[_A(f"CausalAttention{'Varlen' if pk else ''}-d{d}-{'bidir' if bd else 'causal'}", T._v(T.b_causal, d=d, lens=L65, bidir=bd, packed=pk),
         r_causal) for d in (64, 128) for bd in (False, True) for pk in (False, True)],
    *[_A(f"CausalAttentionVarlen-d64-short-{'bidir' if bd else 'causal'}", T._v(T.b_causal, d=64, lens=GQA_SHORT, bidir=bd, packed=True,
                                                                              groups=True), r_causal, dtypes=(BF,), kernels=("gqas::fwd_kernel", "gqas::bwd_kernel"))
      for bd in (False, True)],
    _A("RopeCausalAttention", T._v(T.b_rope_causal, lens=L65), r_rope_causal, _rope_causal_check),
    _A("RopeCausalAttentionVarlen", T._v(T.b_rope_causal, lens=L65, packed=True), r_rope_causal, _rope_causal_check),
    Spec("QKNormRope", T._v(T.b_rope_causal, lens=L33, attend=False), r_qknorm_rope, c_l2, cls="decoder rows and GEMMs"),
    Spec("QKNormRope-packed", T._v(T.b_rope_causal, lens=L33, attend=False, packed=True), r_qknorm_rope, c_l2, cls="decoder rows and GEMMs"),
    _A("_RopeAttention-full", T._v(T.b_rope_attention, lens=L65), r_rope_attention, _rope_check, primary=0),
    _A("_RopeAttention-band", T._v(T.b_rope_attention, lens=L65, window=16), r_rope_attention, _rope_check, primary=0),
    _A("_RopeAttention-packed-band", T._v(T.b_rope_attention, lens=L65, window=16, packed=True), r_rope_attention, _rope_check, primary=0),
    _A("_RopeAttention-short-groups", T._v(T.b_rope_attention, h=8, lens=SHORT64, packed=True, groups=True), r_rope_attention, _rope_check,
       dtypes=(BF,), kernels=("attn_fwd_short_kernel", "attn_bwd_short_kernel"), primary=0),
    *[_A(f"_RopeCausalGQA-d{d}-{'bidir' if bd else 'causal'}{'-packed' if pk else ''}", T._v(T.b_rope_gqa, d=d, lens=L65, bidir=bd, packed=pk),
         r_rope_gqa, _rope_check, primary=0) for d, bd, pk in ((64, False, False), (128, True, False), (128, False, True), (64, True, True))],
    _A("_RopeCausalGQA-d64-short-groups", T._v(T.b_rope_gqa, d=64, lens=GQA_SHORT, packed=True, groups=True), r_rope_gqa, _rope_check,
       dtypes=(BF,), kernels=("gqas::fwd_kernel", "gqas::bwd_kernel"), primary=0),
    # norm family: one width on each side of LN_WIDE_ABOVE, 5 rows
    Spec("BiasResLayerNorm-1024", T._v(T.b_bias_res_ln, rows=5, f=1024), r_bias_res_ln, _norm_family(_ln_extra), cls="norm family"),
    Spec("BiasResLayerNorm-1032-act", T._v(T.b_bias_res_ln, rows=5, f=1032, act=True), r_bias_res_ln, _norm_family(_ln_extra),
         cls="norm family"),
    Spec("GraphNormAct", T._v(T.b_graphnorm, n=37, f=24), r_graphnorm, _norm_family(_gn_extra), cls="norm family"),
    Spec("GraphNormAct-drop", T._v(T.b_graphnorm, n=37, f=24, p=0.1, seed=SEED), r_graphnorm, _norm_family(_gn_extra), cls="norm family"),
    Spec("BiasGelu", T._v(T.b_bias_gelu, rows=5, f=72), r_bias_gelu, _norm_family(_bg_extra), cls="norm family"),
    Spec("EmbedSum", T._v(T.b_embed_sum, rows=40, p=24), r_embed_sum, _norm_family(_embed_extra), cls="norm family"),
    Spec("SoftMask", T._v(T.b_softmask, n=9, f=20, out_cols=32), r_softmask, _norm_family(_softmask_extra), cls="norm family"),
    Spec("MeanPoolScatter", T._v(T.b_meanpool, lens=(5, 1, 33), p=24, nodes=7), r_meanpool, _norm_family(None), cls="norm family"),
    Spec("MeanPoolScatter-packed", T._v(T.b_meanpool, lens=(5, 1, 33), p=24, nodes=7, packed=True), r_meanpool, _norm_family(None), cls="norm family"),
    # decoder family and everything that is a GEMM
    *[Spec(f"_AddNorm-{k}", T.NODES["ops._AddNorm"][k], r_add_norm, c_l2, use_alone=(0, 1), cls="decoder rows and GEMMs")
      for k in T.NODES["ops._AddNorm"]],
    Spec("_GLU-swiglu", T._v(T.b_glu, rows=5, inter=72), r_glu, c_l2, cls="decoder rows and GEMMs"),
    Spec("_GLU-geglu", T._v(T.b_glu, rows=5, inter=72, stem="geglu"), r_glu, c_l2, cls="decoder rows and GEMMs"),
    Spec("RGCNAggregate", T._v(T.b_rgcn, n=9, f=24), r_rgcn, c_l2, cls="decoder rows and GEMMs"),
    Spec("_RootAddmm", T.b_root_addmm, r_root_addmm, c_gemm, cls="decoder rows and GEMMs"),
    Spec("_SelectRows", T.b_select_rows, r_select_rows, c_l2, cls="decoder rows and GEMMs"),
    Spec("_BasisCompose-hip", T.b_basis, r_basis, c_l2, dtypes=(FP,), kernels=(), cls="decoder rows and GEMMs"),
    Spec("_BasisCompose-fallback", T._v(T.b_basis, ra=6, cols=6), r_basis, c_l2, dtypes=(FP,), cls="decoder rows and GEMMs"),
    Spec("_SplitLast", T.b_split_last, r_split_last, c_l2, use_alone=(0, 1), cls="decoder rows and GEMMs"),
    Spec("_ScaledProjectionSum", T.b_scaled_projection, r_scaled_projection, c_scaled, cls="decoder rows and GEMMs"),
    Spec("_ScaledProjectionCat", T._v(T.b_scaled_projection, cat=True), r_scaled_projection, c_scaled, cls="decoder rows and GEMMs"),
    *[Spec(f"_Linear-{k}", T.NODES["dense._Linear"][k], r_linear, c_gemm, use_alone=(0, 1) if "res" in k else (), cls="decoder rows and GEMMs")
      for k in T.NODES["dense._Linear"]],
    *[Spec(f"LinearBf16x3-{k}", T.NODES["dense.LinearBf16x3"][k], r_linear, c_x3, dtypes=(FP,), use_alone=(0, 1) if "res" in k else (),
           cls="bf16x3") for k in T.NODES["dense.LinearBf16x3"]],
    Spec("_BiasTable", T.b_bias_table, r_bias_table, c_l2, dtypes=(FP,), cls="decoder rows and GEMMs"),
    Spec("_Tables", T._v(T.b_tables, d=64, rows=33, w=8), r_tables, c_gemm, use_alone=(0, 1), cls="decoder rows and GEMMs"),
]
RUNS = [(s, dt) for s in SPECS for dt in s.dtypes]


# --------------------------------------------------------------------------------------------------------------------- runner
def _gouts(case, outs, dt):
    g = torch.Generator().manual_seed(99)
    return [torch.randn(o.shape, generator=g).to(o.device, o.dtype) for o in outs]


def _reference(spec, case, gouts, use=None, rounded=False):
    """float64 outputs and gradients of every differentiable input: {'out0': .., 'd<name>': ..}, the aux of the run"""
    rnd = (lambda t: t.bfloat16()) if rounded else (lambda t: t)
    leaves = {n: rnd(v.detach().cpu()).double().requires_grad_(True) for n, v in case.inputs.items()}
    meta = dict(case.meta or {})
    outs = spec.ref(leaves, meta)
    idx = range(len(outs)) if use is None else (use,)
    torch.autograd.backward([outs[i] for i in idx], [rnd(gouts[i].detach().cpu()).double() for i in idx])
    ref = {f"out{i}": o.detach() for i, o in enumerate(outs)}
    ref.update({f"d{n}": (v.grad if v.grad is not None else torch.zeros_like(v)) for n, v in leaves.items()})
    return ref, meta, {n: v.detach() for n, v in leaves.items()}


def _run(case, pattern, gouts, use=None, profile=True):
    """-> (leaves, outputs, kernels of forward + backward).  The node may accumulate into a contiguous incoming gradient in
    place (dense._Linear's residual output): every run gets its own copy."""
    box = {}
    gouts = [g.clone() if g.is_contiguous() else g for g in gouts]

    def go():
        leaves = {n: v.clone().requires_grad_(n in pattern) for n, v in case.inputs.items()}
        outs = case.call(leaves)
        outs = outs if isinstance(outs, tuple) else (outs,)
        idx = [i for i in (range(len(outs)) if use is None else (use,)) if outs[i].requires_grad]
        torch.autograd.backward([outs[i] for i in idx], [gouts[i] for i in idx])
        box.update(leaves=leaves, outs=outs)
    ks = kernels_run(go) if profile else go()
    return box["leaves"], box["outs"], ks


def _forward(case, grad_mode, trainable):
    box = {}

    def go():
        leaves = {n: v.clone().requires_grad_(trainable) for n, v in case.inputs.items()}
        with torch.set_grad_enabled(grad_mode):
            outs = case.call(leaves)
        box["outs"] = tuple(o.detach() for o in (outs if isinstance(outs, tuple) else (outs,)))
    return box, kernels_run(go)


def _env(spec, case, gouts, use, dt):
    ref, meta, leaves64 = _reference(spec, case, gouts, use)
    env = dict(ref=ref, meta=meta, aux=meta.get("aux"), leaves64=leaves64, gouts=[g.detach().cpu().double() for g in gouts])
    if spec.floor is not None and dt == BF:
        env["floor"] = spec.floor(leaves64, meta, env["gouts"])
    if spec.check is c_x3 or (spec.check in (c_gemm, c_scaled) and dt == BF):
        env["plain"] = _reference(spec, case, gouts, use, rounded=True)[0]
    return env


def _check_grads(spec, dt, pattern, leaves, env, tag):
    for n, leaf in leaves.items():
        if n not in pattern:
            assert leaf.grad is None, f"{spec.id} {tag}: frozen {n} got a gradient"
            continue
        assert leaf.grad is not None and leaf.grad.shape == leaf.shape and leaf.grad.dtype == leaf.dtype, (spec.id, tag, n)
        assert bool(torch.isfinite(leaf.grad).all()), (spec.id, tag, n)
        if float(env["ref"][f"d{n}"].abs().max()) == 0.0:          # no used output depends on it: exact zeros, nothing relative
            assert float(leaf.grad.abs().max()) == 0.0, (spec.id, tag, n)
            continue
        spec.check(f"d{n}", leaf.grad, env["ref"][f"d{n}"], dt, spec, env)


def _check_outs(spec, dt, outs, env, tag, which=None):
    for i, o in enumerate(outs):
        if which is None or i in which:
            spec.check(f"out{i}", o.detach(), env["ref"][f"out{i}"], dt, spec, env)


def _bits(a, b):
    return _same_bits((a.contiguous(),), (b.contiguous(),))


@pytest.mark.parametrize("spec,dt", RUNS, ids=[f"{s.id}-{'bf16' if d == BF else 'fp32'}" for s, d in RUNS])
def test_freeze_patterns_vs_float64(dev, spec, dt):
    case = spec.build(dev, dt)
    names = list(case.inputs)
    outs0 = case.call({n: v.clone() for n, v in case.inputs.items()})
    outs0 = outs0 if isinstance(outs0, tuple) else (outs0,)
    gouts = _gouts(case, outs0, dt)
    env = _env(spec, case, gouts, spec.primary, dt)
    base_leaves, base_outs, base_k = _run(case, tuple(names), gouts, spec.primary)
    print(f"\n{spec.id}: all trainable: {sorted(base_k)}")
    if dt == BF or len(spec.dtypes) == 1:
        for part in spec.kernels:
            assert any(part in k for k in base_k), (part, sorted(base_k))
    _check_outs(spec, dt, base_outs, env, "all")
    _check_grads(spec, dt, tuple(names), base_leaves, env, "all")
    for pattern in T.patterns(names):
        if set(pattern) == set(names):
            continue
        leaves, outs, ks = _run(case, pattern, gouts, spec.primary)
        tag = "trainable " + ",".join(pattern)
        print(f" {tag}")
        _check_grads(spec, dt, pattern, leaves, env, tag)
        # the same kernels on the same inputs in the same order give the same bits.  A pattern may only leave out the bias
        # column sums (no bias master needs one): they feed no other gradient, so the bits still hold
        assert ks <= base_k and all(k.startswith(BIAS_SUM_KERNELS) for k in base_k - ks), (tag, sorted(ks ^ base_k))
        for n in pattern:
            assert _bits(leaves[n].grad, base_leaves[n].grad), f"{spec.id} {tag}: d{n} differs in bits from the all-trainable run"
        for o, b in zip(outs, base_outs):
            assert _bits(o.detach(), b.detach()), f"{spec.id} {tag}: the output differs in bits from the all-trainable run"


@pytest.mark.parametrize("spec,dt", RUNS, ids=[f"{s.id}-{'bf16' if d == BF else 'fp32'}" for s, d in RUNS])
def test_forward_without_grad(dev, spec, dt):
    """under no_grad, and in grad mode with nothing requiring grad: within the forward budget, and the training forward's bits
    whenever the same forward kernels ran (the rewritten input of the in-place nodes included)"""
    case = spec.build(dev, dt)
    train, train_k = _forward(case, True, True)
    gouts = _gouts(case, train["outs"], dt)
    env = _env(spec, case, gouts, spec.primary, dt)
    _check_outs(spec, dt, train["outs"], env, "training forward")
    for tag, grad_mode in (("no_grad", False), ("nothing requires grad", True)):
        box, ks = _forward(case, grad_mode, False)
        _check_outs(spec, dt, box["outs"], env, tag)
        assert ks == train_k, (tag, sorted(ks ^ train_k))          # out_lo is an argument, not another kernel
        for o, b in zip(box["outs"], train["outs"]):
            assert _bits(o, b), f"{spec.id} {tag}: the output differs in bits from the training forward"


@pytest.mark.parametrize("spec,dt", RUNS, ids=[f"{s.id}-{'bf16' if d == BF else 'fp32'}" for s, d in RUNS])
def test_incoming_gradient_forms(dev, spec, dt):
    case = spec.build(dev, dt)
    names = tuple(case.inputs)
    outs0 = case.call({n: v.clone() for n, v in case.inputs.items()})
    outs0 = outs0 if isinstance(outs0, tuple) else (outs0,)
    gouts = _gouts(case, outs0, dt)
    env = _env(spec, case, gouts, spec.primary, dt)
    # a column slice of a wider buffer
    wide = [torch.cat([g, torch.full_like(g, 7.0)], -1)[..., :g.shape[-1]] for g in gouts]
    assert all(not w.is_contiguous() or w.numel() <= w.shape[-1] for w in wide)
    leaves, _, _ = _run(case, names, wide, spec.primary, profile=False)
    _check_grads(spec, dt, names, leaves, env, "non-contiguous gradient")
    # an expanded, zero-stride gradient of ones: out.sum().backward()
    ones = [torch.ones((), device=dev, dtype=o.dtype).expand(o.shape) for o in outs0]
    env1 = _env(spec, case, ones, spec.primary, dt)
    leaves = {n: v.clone().requires_grad_(True) for n, v in case.inputs.items()}
    outs = case.call(leaves)
    outs = outs if isinstance(outs, tuple) else (outs,)
    sum(o.sum() for i, o in enumerate(outs) if spec.primary in (None, i)).backward()
    _check_grads(spec, dt, names, leaves, env1, "expanded gradient")
    if dt == BF:
        leaves, _, _ = _run(case, names, [g.float() for g in gouts], spec.primary, profile=False)
        _check_grads(spec, dt, names, leaves, env, "fp32 gradient")
    for use in spec.use_alone:
        envu = _env(spec, case, gouts, use, dt)
        leaves, _, _ = _run(case, names, gouts, use, profile=False)
        _check_grads(spec, dt, names, leaves, envu, f"only output {use} used")
