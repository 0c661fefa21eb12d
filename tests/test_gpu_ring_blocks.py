"""The ring K|V exchange's contract of the attention kernels, in one process: ``ops.AttentionBlock`` driven exactly as
``dist._RingAttention`` drives it, against dense float64 attention over all keys.

The keys of one attention problem are split into W consecutive blocks; every block is zero-padded to the largest one and
masked by ``kv_len`` = its size, and block j draws its dropout mask with ``seed + j``.  Forward: ``AttentionBlock.fwd`` per
block, the blocks merged with the project's own ``dist._merge_partial`` in fp32, ``out = o_acc.to(dtype)`` and, for bf16,
``out_lo = (o_acc - out).to(dtype)``.  Backward: ``AttentionBlock.bwd`` per block with the MERGED ``out``, ``lse`` and
``out_lo`` - an ``lse`` and an ``out`` that are not the block's own - the dQ shares summed in fp32, every block's dK / dV placed
at its rows.  The inputs are rounded to bf16 once for both dtypes, so one float64 reference serves a geometry in either.

References: ``helpers._dense_reference`` over all keys (out, dQ, dK, dV), and ``_block_reference`` here, the arithmetic of
tests/test_dist_cpu.py's ``_TorchBlock`` in float64 with dropout: block output, block log-sum-exp, and the block's dQ share
given the global log-sum-exp and the global delta.  The shares must add up to the dense dQ (asserted to 1e-9).

Asserted per case:
  * every block's ``lse_j`` and the merged ``lse`` against float64 logsumexp: fp32 within 1e-4 (the figure of
    test_gpu_attention_wide.py); bf16 within max_j 2^-9 scale sum_d |q_id| |k_jd| + 1e-4 per row (the pipelined forward rounds
    q scale log2(e) to bf16, and lse is 1-Lipschitz in the scores under the max norm).  An empty block gives out = 0 and
    lse = -inf exactly.
  * every block's ``out_j``, the merged ``out``, the summed dQ, dK and dV within ``test_gpu_attention_matrix._budget``; every dQ
    share against its float64 share, the error measured against the max and the norm of the FULL dQ (the quantity the ring
    accumulates into in fp32; a one-key block's share has almost no norm of its own).
  * a bf16 quantity that misses its budget is not given a wider one: the same ring is run in fp32, which must meet the fp32
    budget, and ``_floor`` evaluates the dense formula in float64 with the roundings the kernels apply (bf16 block outputs,
    bf16(P D) into the P V products); the kernel must be within 2x of that floor, and both figures are printed.
  * dK and dV rows of every block at or past its ``kv_len`` (the padding) are exactly 0.
  * the attention kernels the forward and the backward launched, by name.
  * a second identical forward + backward gives identical bits.

Measured (MI355X, all cases; max|err| / max|ref| and l2 rel):
  fp32  lse <= 9.1e-7 abs (blocks and merged); out_j 5.8e-7 / 2.9e-7, out 6.0e-7 / 3.8e-7, dq 1.0e-6 / 4.8e-7,
        dq shares 9.3e-7 / 3.7e-7 of the full dQ, dk 1.1e-6 / 4.8e-7, dv 9.3e-7 / 4.9e-7.
  bf16  lse <= 4.8e-3 abs (pipelined forward; 1.3e-6 for the register-staged and the short-sequence forward) against bounds of
        1.2e-2 .. 3.1e-2; out_j 6.3e-3 / 3.3e-3, out 7.5e-3 / 3.9e-3, dq 8.0e-3 / 4.4e-3, dq shares 9.4e-3 / 3.3e-3 of the
        full dQ, dk 1.0e-2 / 4.0e-3, dv 1.0e-2 / 3.8e-3.
  No bf16 quantity missed its budget, so no floor was needed (the floors of dq in the short geometry: 3.2e-3 / 1.0e-3 at
  p = 0, 8.6e-3 / 1.1e-3 at p = 0.1).

Before the short-sequence dispatch of gmlm_attention_bwd looked at ``out_lo``, the two ``short_geom`` cases ran
attn_bwd_short_kernel, which forms delta from the block's own keys: dq 3.0e-1 / 1.8e-1 (p = 0) and 2.7e-1 / 1.8e-1 (p = 0.1),
dk 3.0e-1 / 1.6e-1 in both, against budgets of 2e-2 / 8e-3; out, dv and every lse were within budget, and the fp32 twin of
the same ring met the fp32 budget."""
from dataclasses import dataclass

import pytest
import torch

from helpers import _close, _dense_reference, attn_dropout_scale, kernels_run
from test_gpu_attention_matrix import BF, F32, _budget, _is_attention, delta, dkv, dq, fwd, pdkv, pdq, pfwd, sbwd, sfwd
from test_gpu_decoder_ops import _same_bits

pytestmark = pytest.mark.gpu

bf, f32 = torch.bfloat16, torch.float32
SEED = 0x1234_5678_9ABC
LSE_ABS = 1e-4


@dataclass(frozen=True)
class Case:
    id: str
    dtype: torch.dtype
    d: int
    b: int
    h: int
    lq: int
    sizes: tuple               # keys per block, in merge order
    p: float
    fwd: frozenset             # the attention kernels of all forward calls / of all backward calls (every block has one shape)
    bwd: frozenset


def _case(id_, dtype, d, b, h, lq, sizes, p, fwd_set, bwd_set):
    return Case(id_, dtype, d, b, h, lq, tuple(sizes), p, frozenset(fwd_set), frozenset(bwd_set))


def _staged(t, d, nw, dr, qt=32):
    """register-staged forward and backward (attn_kernels.hip) at `nw` waves"""
    return {fwd(t, d, nw, dr)}, {delta(t), dq(t, d, nw, dr), dkv(t, d, nw, dr, qt)}


# The expected sets are read off gmlm_attention_fwd / gmlm_attention_bwd (attn_kernels.hip) for b, h, lq and lk = max(sizes):
# pick_waves gives 2 everywhere here (ceil(rows / 128) * b*h < 1024).
CASES = [
    # fp32: register-staged, 2 waves (the geometry of test_gpu_dist's ring)
    _case("f32_d64", f32, 64, 1, 8, 150, (151, 150), 0.0, *_staged(F32, 64, 2, False)),
    # an empty block (not the first: dist._merge_partial of two empty states is NaN) and a one-key block
    _case("f32_d96_uneven", f32, 96, 2, 3, 150, (97, 64, 0, 1), 0.0, *_staged(F32, 96, 2, False)),
    _case("f32_d64_drop", f32, 64, 1, 8, 150, (151, 150), 0.1, *_staged(F32, 64, 2, True)),
    # bf16 d = 96, the production CrossAttention geometry: LDS-DMA forward and backward, 4 waves
    _case("bf16_d96_pipe", bf, 96, 1, 8, 200, (130, 129, 70), 0.0, {pfwd(96, 4, False)}, {delta(BF), pdq(96, 4, False), pdkv(96, 4, False)}),
    _case("bf16_d96_pipe_drop", bf, 96, 1, 8, 200, (130, 129, 70), 0.1, {pfwd(96, 4, True)}, {delta(BF), pdq(96, 4, True), pdkv(96, 4, True)}),
    # bf16 d = 64 beyond 128 query rows: pipelined forward, folded register-staged backward staging 64 query rows
    _case("bf16_d64_long", bf, 64, 2, 4, 200, (129, 128, 0), 0.0, {pfwd(64, 4, False)}, {delta(BF), dq(BF, 64, 2, False), dkv(BF, 64, 2, False, 64)}),
    # bf16 d = 64, <= 128 rows, b*h < 512: register-staged forward
    _case("bf16_d64_rows100", bf, 64, 3, 4, 100, (100, 37), 0.0, *_staged(BF, 64, 2, False)),
    # the short geometry (<= 128 rows, b*h = 512): LDS-resident forward; the backward is handed out_lo and a foreign lse, so it
    # must NOT be attn_bwd_short_kernel (that kernel forms delta from its own keys) but the streaming kernels
    _case("bf16_d64_short_geom", bf, 64, 64, 8, 64, (64, 33), 0.0, {sfwd(64, False)}, _staged(BF, 64, 2, False)[1]),
    # the dropout slab (b*h + head) * lq uses the absolute batch index: a batch split below 512 pairs would draw another mask
    _case("bf16_d64_short_geom_drop", bf, 64, 64, 8, 64, (64, 33), 0.1, {sfwd(64, True)}, _staged(BF, 64, 2, True)[1]),
]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _heads(t, h):
    b, l, c = t.shape
    return t.reshape(b, l, h, c // h).transpose(1, 2)                                # [b, h, l, d]


def _rows(t):
    return t.transpose(1, 2).reshape(t.shape[0], t.shape[2], t.shape[1] * t.shape[3])   # [b, h, l, d] -> [b, l, h*d]


def _inputs(c):
    """q, go [b, lq, hd], k, v [b, sum(sizes), hd] as float32 holding bf16 values (exact in either dtype), on the host"""
    g = torch.Generator().manual_seed(sum(c.sizes) * 1000 + c.lq * 10 + c.d + c.b * c.h)
    hd, n = c.h * c.d, sum(c.sizes)
    r = lambda *s, f=1.0: (torch.randn(*s, generator=g) * f).bfloat16().float()
    return r(c.b, c.lq, hd), r(c.b, n, hd, f=1.5), r(c.b, n, hd), r(c.b, c.lq, hd)  # scores ~ N(0, 1.5)


def _offsets(sizes):
    return [sum(sizes[:j]) for j in range(len(sizes))]


def _drop_masks(c, dev):
    """[b, h, lq, n_j] float64 multiplier per block (None without dropout): block j of the ring draws seed + j over its padded
    width mx with the slab of the padded layout, (batch * heads + head) * lq."""
    if not c.p:
        return [None] * len(c.sizes)
    mx = max(c.sizes)
    return [torch.stack([torch.stack([attn_dropout_scale(SEED + j, (bi * c.h + hi) * c.lq, c.lq, mx, c.p, dev)[:, :n]
                                      for hi in range(c.h)]) for bi in range(c.b)]) for j, n in enumerate(c.sizes)]


def _block_reference(c, q, k, v, go, out, drops):
    """float64, per block j: (out_j [b, lq, hd], lse_j [b, h, lq], dq share [b, lq, hd]) and the global lse; the arithmetic of
    test_dist_cpu._TorchBlock with dropout.  ``out`` is the dense output of all keys (delta = rowsum(dO * O))."""
    scale = c.d ** -0.5
    qh, gh, oh = _heads(q.double(), c.h), _heads(go.double(), c.h), _heads(out, c.h)
    s = [qh @ _heads(k[:, o:o + n].double(), c.h).transpose(-1, -2) * scale for o, n in zip(_offsets(c.sizes), c.sizes)]
    lse = torch.logsumexp(torch.cat(s, -1), -1)
    dlt = (gh * oh).sum(-1, keepdim=True)
    blocks = []
    for s_j, o, n, drop in zip(s, _offsets(c.sizes), c.sizes, drops):
        kh, vh = _heads(k[:, o:o + n].double(), c.h), _heads(v[:, o:o + n].double(), c.h)
        lse_j = torch.logsumexp(s_j, -1) if n else torch.full_like(lse, float("-inf"))
        p_loc = torch.exp(s_j - lse_j.unsqueeze(-1)) if n else s_j
        p_glob = torch.exp(s_j - lse.unsqueeze(-1))                                # the global softmax restricted to the block
        dp = gh @ vh.transpose(-1, -2)
        if drop is not None:
            p_loc, dp = p_loc * drop, dp * drop
        ds = p_glob * (dp - dlt) * scale
        blocks.append((_rows(p_loc @ vh), lse_j, _rows(ds @ kh)))
    return blocks, lse


def _floor(c, q, k, v, go, drops):
    """The dense formula in float64 with the roundings the bf16 kernels apply: the probabilities enter the P V products as
    bf16(P D), every block output is stored in bf16; the merge, out + out_lo and delta are as exact as the ring's fp32 keeps
    them.  -> dict of out_j / dq_j lists and out, dq, dk, dv."""
    scale = c.d ** -0.5
    rb = lambda t: t.bfloat16().double()
    qh, gh = _heads(q.double(), c.h), _heads(go.double(), c.h)
    offs = _offsets(c.sizes)
    s = [qh @ _heads(k[:, o:o + n].double(), c.h).transpose(-1, -2) * scale for o, n in zip(offs, c.sizes)]
    lse = torch.logsumexp(torch.cat(s, -1), -1)
    res = dict(out_j=[], dq_j=[], dk=[], dv=[])
    o_acc = torch.zeros_like(qh)
    for s_j, o, n, drop in zip(s, offs, c.sizes, drops):
        vh = _heads(v[:, o:o + n].double(), c.h)
        lse_j = torch.logsumexp(s_j, -1) if n else torch.full_like(lse, float("-inf"))
        p_loc = torch.exp(s_j - lse_j.unsqueeze(-1)) if n else s_j
        o_j = rb((rb(p_loc) if drop is None else rb(p_loc * drop)) @ vh)
        res["out_j"].append(_rows(o_j))
        o_acc = o_acc + o_j * torch.exp(lse_j - lse).unsqueeze(-1)
    res["out"] = _rows(rb(o_acc))
    o_hi = rb(o_acc)
    dlt = (gh * (o_hi + rb(o_acc - o_hi))).sum(-1, keepdim=True)
    for s_j, o, n, drop in zip(s, offs, c.sizes, drops):
        kh, vh = _heads(k[:, o:o + n].double(), c.h), _heads(v[:, o:o + n].double(), c.h)
        p_glob = torch.exp(s_j - lse.unsqueeze(-1))
        dp = gh @ vh.transpose(-1, -2)
        pd = p_glob if drop is None else p_glob * drop
        ds = p_glob * ((dp if drop is None else dp * drop) - dlt) * scale
        res["dq_j"].append(_rows(ds @ kh))
        res["dk"].append(_rows(ds.transpose(-1, -2) @ qh))
        res["dv"].append(_rows(pd.transpose(-1, -2) @ gh))
    res["dq"] = sum(res["dq_j"])
    res["dk"], res["dv"] = torch.cat(res["dk"], 1), torch.cat(res["dv"], 1)
    return res


_REFS = {}


def _reference(c, dev):
    """One float64 reference per (geometry, p), left unchanged: dense out / dq / dk / dv, the per-block figures, the lse bounds."""
    key = (c.d, c.b, c.h, c.lq, c.sizes, c.p)
    if key not in _REFS:
        q, k, v, go = (t.to(dev) for t in _inputs(c))
        drops = _drop_masks(c, dev)
        full = None if not c.p else torch.cat(drops, -1)
        dense = _dense_reference(q, k, v, go, c.h, c.d ** -0.5, None, None if full is None else (lambda bi, hi: full[bi, hi]))
        blocks, lse = _block_reference(c, q, k, v, go, dense[0], drops)
        share_sum = sum(bl[2] for bl in blocks)
        assert float((share_sum - dense[1]).abs().max()) <= 1e-9 * float(dense[1].abs().max())     # the references agree
        # bf16 lse bound per row: 2^-9 * scale * max over the keys in scope of sum_d |q_id| |k_jd|
        qa = _heads(q.double().abs(), c.h)
        reach = [(qa @ _heads(k[:, o:o + n].double().abs(), c.h).transpose(-1, -2)).amax(-1) if n else torch.zeros_like(lse)
                 for o, n in zip(_offsets(c.sizes), c.sizes)]
        bound = [2.0 ** -9 * c.d ** -0.5 * r_ + LSE_ABS for r_ in reach]
        _REFS[key] = dict(dense=dense, blocks=blocks, lse=lse, bound=bound, bound_all=torch.stack(bound).amax(0), drops=drops)
    return _REFS[key]


def _ring(c, dtype, dev, q, k, v, go):
    """forward + backward of the ring on the kernels, as dist._RingAttention runs them (rank-local, no exchange)"""
    from gmlm_amd import ops
    from gmlm_amd.dist import _merge_partial
    b, lq, hd, h, mx = c.b, c.lq, c.h * c.d, c.h, max(c.sizes)
    blk = ops.AttentionBlock(h, c.d ** -0.5, c.p)
    bufs, lens = [], []
    for o, n in zip(_offsets(c.sizes), c.sizes):
        cur = torch.zeros(b, mx, 2 * hd, dtype=dtype, device=dev)                  # K | V of one block, zero-padded to mx
        cur[:, :n, :hd], cur[:, :n, hd:] = k[:, o:o + n], v[:, o:o + n]
        bufs.append(cur)
        lens.append(torch.full((b,), n, dtype=torch.int32, device=dev))
    r = dict(out_j=[], lse_j=[], dq_j=[], dk_j=[], dv_j=[])

    def forward():
        o_acc = torch.zeros(b, lq, h, c.d, dtype=torch.float32, device=dev)
        lse_acc = torch.full((b, h, lq), float("-inf"), dtype=torch.float32, device=dev)
        for j, (cur, kv_len) in enumerate(zip(bufs, lens)):
            o_j, lse_j = blk.fwd(q, cur[..., :hd], cur[..., hd:], kv_len, SEED + j)
            r["out_j"].append(o_j)
            r["lse_j"].append(lse_j)
            o_acc, lse_acc = _merge_partial(o_acc, lse_acc, o_j.float().view(b, lq, h, c.d), lse_j.float())
        r["out"] = o_acc.view(b, lq, hd).to(dtype)
        r["out_lo"] = (o_acc.view(b, lq, hd) - r["out"].float()).to(dtype) if dtype != torch.float32 else None
        r["lse"] = lse_acc

    def backward():
        lo_kw = {"out_lo": r["out_lo"]} if r["out_lo"] is not None else {}
        dq_acc = torch.zeros(b, lq, hd, dtype=torch.float32, device=dev)
        for j, (cur, kv_len) in enumerate(zip(bufs, lens)):
            dq_j, dk_j, dv_j = blk.bwd(q, cur[..., :hd], cur[..., hd:], r["out"], go, r["lse"], kv_len, SEED + j, **lo_kw)
            dq_acc += dq_j.float()
            for name, t in (("dq_j", dq_j), ("dk_j", dk_j), ("dv_j", dv_j)):
                r[name].append(t)
        r["dq"] = dq_acc.to(dtype)

    r["fwd_kernels"] = {n for n in kernels_run(forward) if _is_attention(n)}
    r["bwd_kernels"] = {n for n in kernels_run(backward) if _is_attention(n)}
    r["dk"] = torch.cat([t[:, :n] for t, n in zip(r["dk_j"], c.sizes)], 1)
    r["dv"] = torch.cat([t[:, :n] for t, n in zip(r["dv_j"], c.sizes)], 1)
    return r


def _flat(r):
    return [r["out"], r["lse"], r["dq"]] + r["out_j"] + r["lse_j"] + r["dq_j"] + r["dk_j"] + r["dv_j"]


def _measure(name, got, ref, whole=None):
    """max |got - ref| / max |whole| and ||got - ref|| / ||whole|| (whole = ref unless the error is measured against a larger
    quantity), printed"""
    whole = ref if whole is None else whole
    e = got.double() - ref
    mx, l2 = float(e.abs().max()) / float(whole.abs().max()), float(e.norm()) / float(whole.norm())
    print(f"  {name}: max|err| / max|ref| = {mx:.2e}, l2 rel = {l2:.2e}")
    return mx, l2


def _compare(c, dtype, r, ref):
    """-> list of (name, mx, l2, block index or None) of the quantities over their budget; every figure is printed first"""
    dense, missed = ref["dense"], []
    for name, got in (("out", r["out"]), ("dq", r["dq"]), ("dk", r["dk"]), ("dv", r["dv"])):
        assert bool(torch.isfinite(got).all()), name
    # log-sum-exp: blocks and merged
    for j, (n, got, (_, lse_j, _), bound) in enumerate(zip(c.sizes, r["lse_j"], ref["blocks"], ref["bound"])):
        if n == 0:
            assert bool((got == float("-inf")).all()) and float(r["out_j"][j].abs().max()) == 0.0, f"empty block {j}"
            continue
        err = (got.double() - lse_j).abs()
        lim = bound if dtype == bf else torch.full_like(bound, LSE_ABS)
        print(f"  lse_{j}: max|err| = {float(err.max()):.2e} (bound {float(lim.min()):.2e} .. {float(lim.max()):.2e})")
        assert bool((err <= lim).all()), (f"lse_{j}", float(err.max()), float((err - lim).max()))
    err = (r["lse"].double() - ref["lse"]).abs()
    lim = ref["bound_all"] if dtype == bf else torch.full_like(ref["bound_all"], LSE_ABS)
    print(f"  lse: max|err| = {float(err.max()):.2e} (bound {float(lim.min()):.2e} .. {float(lim.max()):.2e})")
    assert bool((err <= lim).all()), ("lse", float(err.max()))
    # outputs and gradients
    checks = [(f"out_{j}", r["out_j"][j], bl[0], None, "out", j) for j, (n, bl) in enumerate(zip(c.sizes, ref["blocks"])) if n]
    checks += [("out", r["out"], dense[0], None, "out", None), ("dq", r["dq"], dense[1], None, "dq", None)]
    checks += [(f"dq_{j}", r["dq_j"][j], bl[2], dense[1], "dq", j) for j, bl in enumerate(ref["blocks"])]
    checks += [("dk", r["dk"], dense[2], None, "dk", None), ("dv", r["dv"], dense[3], None, "dv", None)]
    for name, got, want, whole, what, j in checks:
        if whole is None:
            try:
                _close(name, got, want, *_budget(dtype, what))
            except AssertionError as e:                                           # _close printed the figures and carries them
                missed.append(e.args[0] + (j,))
        else:
            mx, l2 = _measure(name, got, want, whole)
            if mx > _budget(dtype, what)[0] or l2 > _budget(dtype, what)[1]:
                missed.append((name, mx, l2, j))
    # the padding of every block: no gradient at all
    for j, n in enumerate(c.sizes):
        assert float(r["dk_j"][j][:, n:].abs().sum()) == 0.0 and float(r["dv_j"][j][:, n:].abs().sum()) == 0.0, f"padding of block {j}"
    return missed


@pytest.mark.parametrize("c", CASES, ids=[c.id for c in CASES])
def test_ring_blocks_vs_dense_fp64(dev, c):
    ref = _reference(c, dev)
    q, k, v, go = (t.to(dev, c.dtype) for t in _inputs(c))
    r = _ring(c, c.dtype, dev, q, k, v, go)
    print(f"\n{c.id}: forward {sorted(r['fwd_kernels'])}, backward {sorted(r['bwd_kernels'])}")
    missed = _compare(c, c.dtype, r, ref)
    if missed and c.dtype == bf:
        # no wider budget: the fp32 twin must meet its own, and the bf16 figures must be within 2x of the rounding floor
        twin = _ring(c, f32, dev, *(t.float() for t in (q, k, v, go)))
        assert not _compare(c, f32, twin, ref), "the fp32 twin misses its budget as well"
        fl = _floor(c, q, k, v, go, ref["drops"])
        for name, mx, l2, j in missed:
            stem = name.split("_")[0]
            got_f, want = (fl[stem], ref["dense"][("out", "dq", "dk", "dv").index(stem)]) if j is None else \
                (fl[stem + "_j"][j], ref["blocks"][j][0 if stem == "out" else 2])
            fmx, fl2 = _measure(name + " (bf16 floor)", got_f, want, ref["dense"][1] if (j is not None and stem == "dq") else None)
            print(f"  {name}: {mx:.2e} / {l2:.2e} against the floor {fmx:.2e} / {fl2:.2e}")
            lim = _budget(bf, stem)
            assert mx <= max(lim[0], 2 * fmx) and l2 <= max(lim[1], 2 * fl2), (name, mx, l2, fmx, fl2)
    else:
        assert not missed, missed
    assert r["fwd_kernels"] == set(c.fwd), (sorted(r["fwd_kernels"]), sorted(c.fwd))
    assert r["bwd_kernels"] == set(c.bwd), (sorted(r["bwd_kernels"]), sorted(c.bwd))
    again = _ring(c, c.dtype, dev, q, k, v, go)
    assert again["out_lo"] is None or _same_bits([again["out_lo"]], [r["out_lo"]])
    assert _same_bits(_flat(again), _flat(r))


def test_short_path_backward_with_its_own_lse(dev):
    """The non-ring use of AttentionBlock (the attention micro-benchmark): the short geometry, no out_lo, the block's OWN lse and
    out.  That call stays on attn_bwd_short_kernel and matches float64."""
    from gmlm_amd import ops
    c = next(x for x in CASES if x.id == "bf16_d64_short_geom")
    b, h, l, hd = c.b, c.h, c.lq, c.h * c.d
    q, k, v, go = (t.to(dev, bf) for t in _inputs(c))
    k, v = k[:, :l].contiguous(), v[:, :l].contiguous()
    kv_len = torch.full((b,), l, dtype=torch.int32, device=dev)
    blk = ops.AttentionBlock(h, c.d ** -0.5)
    box = {}
    fwd_k = kernels_run(lambda: box.setdefault("f", blk.fwd(q, k, v, kv_len, 0)))
    out, lse = box["f"]
    bwd_k = kernels_run(lambda: box.setdefault("b", blk.bwd(q, k, v, out, go, lse, kv_len, 0)))
    assert {n for n in fwd_k if _is_attention(n)} == {sfwd(64, False)}, sorted(fwd_k)
    assert {n for n in bwd_k if _is_attention(n)} == {sbwd(64, False)}, sorted(bwd_k)
    ref = _dense_reference(q, k, v, go, h, c.d ** -0.5)
    for name, got, r_ in zip(("out", "dq", "dk", "dv"), (out,) + box["b"], ref):
        assert bool(torch.isfinite(got).all()), name
        _close(name, got, r_, *_budget(bf, name))
    lse_ref = torch.logsumexp(_heads(q.double(), h) @ _heads(k.double(), h).transpose(-1, -2) * c.d ** -0.5, -1)
    bound = 2.0 ** -9 * c.d ** -0.5 * (_heads(q.double().abs(), h) @ _heads(k.double().abs(), h).transpose(-1, -2)).amax(-1) + LSE_ABS
    assert bool(((lse.double() - lse_ref).abs() <= bound).all())
