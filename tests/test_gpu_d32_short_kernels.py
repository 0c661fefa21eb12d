"""The ``d32s::`` kernels (include/gmlm_hip_d32_short.h: LDS-resident short-sequence attention at head dim 32, bf16, packed layout
with seq_groups, one work item per (group, pair of adjacent heads)) against float64 per-sequence attention on inputs rounded to
bf16 with an autograd backward: out, dq, dk, dv and the fused QKV bias sums.  The C entry points are called directly on slices of
ONE fused [T, 3 * h * 32] buffer with gradients into ONE dqkv pre-filled with a sentinel, and through ``ops.attention_qkv(...,
groups=...)``.  Every case asserts the exact ``d32s::`` kernel pair it launched and that no ``d32::`` / ``attn_`` kernel ran, that
a second identical call gives identical bits, finiteness, and prints its worst error-to-bound ratio.
tests/test_d32_short_cpu.py holds the kernels compiled into the library against the ones named here (``expected_kernels``).

Budgets: ``_budget`` of tests/test_gpu_decoder_ops.py (bf16: max 2e-2, l2 6e-3 for out and 8e-3 for the gradients).  Where the
reference is exactly zero (one key: P = 1, dS = 0) the bound is ``_one_key_bounds`` of tests/test_gpu_gqa_kernels.py, applied to a
PAIR of heads as one 64-wide head: that function bounds a 64-term dot product, |dS| <= (2 * 66 + 64) u sum_64 |dO_i| |v_i|, times
its own scale 64^-1/2; a d = 32 head has (2 * 34 + 64) u sum_32 |dO_i| |v_i| times 32^-1/2, and 196 / 132 = 1.48 > 2^1/2 while the
64-term sum contains the 32-term one, so the pair's bound holds for each of its heads.

Dropout (p = 0.1): float64 with the explicit mask of ``helpers.attn_dropout_scale`` and the slab of the packed layout, (head *
total_rows + first row of the SEQUENCE), query and key counted inside the sequence.  The same inputs and seed run through the
streaming ``d32::`` kernels and are held to the same reference: one mask for both routes.

Every test here fails on the commit before these kernels: the library has no gmlm_attention_d32_short_* and the ops layer drops
``groups`` at head dim 32.

The shapes are the smallest that cross each edge: one row (R = 32); one past a wave (R = 64); R = 96; exactly 128 rows whose
sequences straddle the 32-row blocks; a full-tile sequence and three groups; the 13-sequence cap; empty sequences inside a group;
a whole group without rows; trailing rows owned by no sequence; 12 heads x 43 sequences = 516 pairs (past the 512 from which
``GraphTextLM`` builds groups) through the ops layer."""
from functools import lru_cache

import pytest
import torch

from helpers import _close, attn_dropout_scale, kernels_run
from test_gpu_decoder_ops import _budget, _same_bits
from test_gpu_gqa_kernels import _one_key_bounds

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
D, SCALE = 32, 32 ** -0.5
NAMES = ("out", "dq", "dk", "dv")
TILES = (32, 64, 96, 128)
SENTINEL = 7.0
P_DROP, SEED = 0.1, 0x1234_5678_9ABC


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def d32s_kernels(drop, r):
    c = "true" if drop else "false"
    return frozenset((f"d32s::fwd_kernel<{c}, {r}>", f"d32s::bwd_kernel<{c}, {r}>"))


def tile_rows(total_rows):
    """The tile height the host picks: no group holds more rows than the batch has, nor more than 128."""
    return (min(total_rows, 128) + 31) // 32 * 32


def _split(t, h):
    n = h * D
    return t[..., :n], t[..., n:2 * n], t[..., 2 * n:]


def _reference(qkv, go, lens, h, p=0.0, seed=0):
    """float64 attention, one sequence at a time, autograd backward; with ``p`` the explicit dropout mask of the packed layout
    (the normaliser is that of the un-dropped probabilities).  Rows past sum(lens) are left out.  -> out, dq, dk, dv."""
    total, r0, outs = qkv.shape[0], 0, [[], [], [], []]
    for n in lens:
        if n:
            qd, kd, vd = (t[r0:r0 + n].detach().double().requires_grad_(True) for t in _split(qkv, h))
            qh, kh, vh = (t.view(n, h, D).transpose(0, 1) for t in (qd, kd, vd))
            pr = torch.softmax((qh @ kh.transpose(-1, -2)) * SCALE, -1)
            if p:
                pr = pr * torch.stack([attn_dropout_scale(seed, hi * total + r0, n, n, p, qkv.device) for hi in range(h)])
            o = (pr @ vh).transpose(0, 1).reshape(n, h * D)
            o.backward(go[r0:r0 + n].double())
            for acc, t in zip(outs, (o.detach(), qd.grad, kd.grad, vd.grad)):
                acc.append(t)
        r0 += n
    return tuple(torch.cat(a) for a in outs)


def _qkv_go(dev, rows, h, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(rows, 3 * h * D, generator=g).to(dev, BF), torch.randn(rows, h * D, generator=g).to(dev, BF)


def _cu(lens, dev):
    return torch.tensor((0,) + tuple(lens), dtype=torch.int64).cumsum(0).to(dev, torch.int32)


def _c_call(qkv, go, cu, groups, max_len, h, p=0.0, seed=0, bias=False):
    """One forward and one backward through the C entry points on slices of the fused buffers; outputs pre-filled with a sentinel.
    -> out, dq, dk, dv, lse (dq | dk | dv are views of one dqkv) and, with ``bias``, dbias fp32 [3 * h * 32]."""
    from gmlm_amd import _lib
    lib = _lib.lib()
    t, w = qkv.shape
    q, k, v = _split(qkv, h)
    out = torch.full((t, h * D), SENTINEL, dtype=BF, device=qkv.device)
    lse = torch.full((h, t), SENTINEL, dtype=torch.float32, device=qkv.device)
    dqkv = torch.full_like(qkv, SENTINEL)
    dq, dk, dv = _split(dqkv, h)
    st = torch.cuda.current_stream().cuda_stream
    ns, ng = cu.numel() - 1, groups.numel() - 1
    part = torch.full((max(ng, 1), w), SENTINEL, dtype=torch.float32, device=qkv.device) if bias else None
    db = torch.full((w,), SENTINEL, dtype=torch.float32, device=qkv.device) if bias else None
    _lib.check(lib.gmlm_attention_d32_short_fwd(q.data_ptr(), k.data_ptr(), v.data_ptr(), cu.data_ptr(), ns, max_len, t, h, D, w, w, w,
                                                SCALE, p, seed, None, groups.data_ptr(), ng, out.data_ptr(), lse.data_ptr(), _lib.BF16,
                                                st), "d32_short_fwd")
    _lib.check(lib.gmlm_attention_d32_short_bwd(q.data_ptr(), k.data_ptr(), v.data_ptr(), go.data_ptr(), lse.data_ptr(), cu.data_ptr(),
                                                ns, max_len, t, h, D, w, w, w, SCALE, p, seed, None, groups.data_ptr(), ng,
                                                dq.data_ptr(), dk.data_ptr(), dv.data_ptr(), w, w, w,
                                                None if part is None else part.data_ptr(), None if db is None else db.data_ptr(),
                                                _lib.BF16, st), "d32_short_bwd")
    return (out, dq, dk, dv, lse) + ((db,) if bias else ())


def _run(qkv, go, cu, groups, max_len, h, p=0.0, seed=0, bias=False):
    """``_c_call`` with the kernel-pair, repeat and finiteness assertions of every case."""
    box = {}
    ran = kernels_run(lambda: box.setdefault("r", _c_call(qkv, go, cu, groups, max_len, h, p, seed, bias)))
    assert {n for n in ran if n.startswith("d32s::")} == set(d32s_kernels(p > 0, tile_rows(qkv.shape[0]))), sorted(ran)
    assert not any(n.startswith(("d32::", "attn_")) for n in ran), sorted(ran)
    assert ("rows_sum_kernel" in ran) == bias, sorted(ran)
    assert _same_bits(_c_call(qkv, go, cu, groups, max_len, h, p, seed, bias), box["r"])
    assert all(bool(torch.isfinite(t).all()) for t in box["r"])
    return box["r"]


def _check(got, ref, rows=None):
    worst = 0.0
    for name, g_, r_ in zip(NAMES, got, ref):
        g_ = g_ if rows is None else g_[:rows]
        assert g_.shape == r_.shape
        _close(name, g_, r_, *_budget(BF, name))
        e = g_.double() - r_
        mx, l2 = _budget(BF, name)
        worst = max(worst, float(e.abs().max()) / float(r_.abs().max()) / mx, float(e.norm()) / float(r_.norm()) / l2)
    print(f"  worst error / bound = {worst:.3f}")


# (lens, h, expected group boundaries, tile rows)
CASES = {
    "one_row": ((1,), 2, (0, 1), 32),
    "l33": ((33,), 2, (0, 1), 64),
    "rows96": ((64, 1, 31), 2, (0, 3), 96),
    "rows128_straddling": ((31, 33, 1, 63), 2, (0, 4), 128),
    "full_tile_three_groups": ((128, 127, 1, 128), 2, (0, 1, 3, 4), 128),
    "cap13_then_one": ((1,) * 14, 2, (0, 13, 14), 32),
    "empties_inside": ((3, 0, 5, 0, 0, 7), 4, (0, 6), 32),
    "empty_group": ((0,) * 13 + (5,), 2, (0, 13, 14), 32),
}
# the cases that also run with probability dropout: every tile height (one-key sequences are left to p = 0)
DROP_CASES = ("l33", "rows96", "rows128_straddling", "full_tile_three_groups", "empties_inside")
H12_LENS = tuple(1 + (7 * i) % 40 for i in range(43))            # 43 sequences x 12 heads = 516 pairs; 1, 32 and 33 among them


def expected_kernels():
    """Every ``d32s::`` instantiation a test of this file launches (and asserts by name)."""
    return set().union(*(d32s_kernels(p, CASES[n][3]) for n in CASES for p in (False, True) if not p or n in DROP_CASES))


@lru_cache(maxsize=None)
def _problem(dev, name):
    lens, h, _, _ = CASES[name]
    return _qkv_go(dev, sum(lens), h, 307 + 11 * len(lens) + sum(lens) + h)


@lru_cache(maxsize=None)
def _ref(dev, name, p):
    lens, h, _, _ = CASES[name]
    qkv, go = _problem(dev, name)
    return _reference(qkv, go, lens, h, p, SEED)


@pytest.mark.parametrize("name,p", [(n, 0.0) for n in CASES] + [(n, P_DROP) for n in DROP_CASES],
                         ids=list(CASES) + [n + "_drop" for n in DROP_CASES])
def test_d32_short_cases(dev, name, p):
    from gmlm_amd import ops
    lens, h, bounds, tile = CASES[name]
    qkv, go = _problem(dev, name)
    groups = ops.pack_sequence_groups(lens)
    assert tuple(groups.tolist()) == bounds and tile_rows(sum(lens)) == tile
    got = _run(qkv, go, _cu(lens, dev), groups.to(dev), max(lens), h, p, SEED)
    ref = _ref(dev, name, p)
    lse = got[4]
    assert bool(torch.isfinite(lse).all()) and not bool((lse == SENTINEL).any())
    if max(lens) == 1 and min(lens) == 1:                      # every sequence is one key: P = 1, dq = dk = 0 in the reference
        assert h == 2
        zero = _one_key_bounds(qkv[:, None], go[:, None], 1, 1)             # the pair as one 64-wide head (module docstring)
        for nm, g_, r_ in zip(NAMES, got, ref):
            if nm in zero:
                assert float(r_.abs().max()) == 0.0
                ratio = g_.double().abs() / zero[nm][:, 0]
                print(f"  {nm} (reference 0): max |got| / bound = {float(ratio.max()):.3f}")
                assert bool((ratio <= 1).all()), (nm, float(ratio.max()))
            else:
                _close(nm, g_, r_, *_budget(BF, nm))
        if name == "one_row":
            assert torch.equal(ref[3], go.double())            # dv = the sum of the group's dO rows: the one row
        return
    _check(got, ref)


def test_rows_owned_by_no_sequence_keep_their_sentinels(dev):
    """(20, 9) in a batch of 32 rows: the three trailing rows belong to no sequence and are neither read nor written."""
    lens, h, rows = (20, 9), 2, 32
    qkv, go = _qkv_go(dev, rows, h, 911)
    qkv[29:] = float("nan")                                    # reading them would poison the owned rows
    go[29:] = float("nan")
    groups = torch.tensor([0, 2], dtype=torch.int32, device=dev)
    for p in (0.0, P_DROP):
        box = {}
        ran = kernels_run(lambda: box.setdefault("r", _c_call(qkv, go, _cu(lens, dev), groups, 20, h, p, SEED, True)))
        assert {n for n in ran if n.startswith("d32s::")} == set(d32s_kernels(p > 0, 32)), sorted(ran)
        got = box["r"]
        for nm, t in zip(NAMES, got):
            assert bool((t[29:] == SENTINEL).all()), f"{nm}: a row owned by no sequence was written"
            assert bool(torch.isfinite(t[:29]).all()), nm
        assert bool((got[4][:, 29:] == SENTINEL).all()) and bool(torch.isfinite(got[4][:, :29]).all())
        assert bool(torch.isfinite(got[5]).all())              # the bias sums saw no row past the sequences either
        _check(got, _reference(qkv, go, lens, h, p, SEED), rows=29)


def test_explicit_boundaries_agree_with_one_group_to_rounding(dev):
    """(31, 33 | 1, 63): the same 128 rows as two work items, against float64 and against the one-group result within the same
    budgets (another grouping runs a row's sums over other 32-row blocks: agreement to rounding, not to bits)."""
    name = "rows128_straddling"
    lens, h, _, _ = CASES[name]
    qkv, go = _problem(dev, name)
    cu = _cu(lens, dev)
    for p in (0.0, P_DROP):
        two = _run(qkv, go, cu, torch.tensor([0, 2, 4], dtype=torch.int32, device=dev), max(lens), h, p, SEED)
        one = _c_call(qkv, go, cu, torch.tensor([0, 4], dtype=torch.int32, device=dev), max(lens), h, p, SEED)
        _check(two, _ref(dev, name, p))
        _check(two, [t.double() for t in one[:4]])


def _stream_route(qkv, go, cu, max_len, h, p, seed, bias=False):
    """The parent route on the same inputs: ``ops.AttentionQKV`` without ``groups`` (streaming ``d32::`` kernels with out_lo);
    with ``bias`` the QKV bias gradient the way it is formed there, ``ops.column_sum`` over the bf16 dqkv."""
    from gmlm_amd import ops
    box = {}

    def fn():
        x = qkv.clone().requires_grad_(True)
        masters = tuple(torch.zeros(h * D, device=qkv.device, requires_grad=True) for _ in range(3)) if bias else ()
        out = ops.AttentionQKV.apply(x, None, h, SCALE, p, seed, cu, max_len, None, None, *masters)
        out.backward(go)
        box["r"] = (out.detach(),) + _split(x.grad, h) + ((torch.cat([m.grad for m in masters]),) if bias else ())

    ran = kernels_run(fn)
    attn = {n for n in ran if n.startswith(("d32::", "d32s::", "attn_"))}
    assert attn and all(n.startswith("d32::") for n in attn), sorted(ran)
    return box["r"]


def test_dropout_mask_is_the_streaming_route_s(dev):
    """p = 0.1, the 128-row straddling case: the streaming ``d32::`` kernels on the same inputs and seed meet the reference the
    ``d32s::`` kernels met in ``test_d32_short_cases``: one mask for both routes.  (A reference without the mask, or with the mask
    of another slab, is far outside the budget: a tenth of the probabilities differ by a factor.)"""
    name = "rows128_straddling"
    lens, h, _, _ = CASES[name]
    qkv, go = _problem(dev, name)
    _check(_stream_route(qkv, go, _cu(lens, dev), max(lens), h, P_DROP, SEED), _ref(dev, name, P_DROP))
    got = _c_call(qkv, go, _cu(lens, dev), torch.tensor([0, 4], dtype=torch.int32, device=dev), max(lens), h, P_DROP, SEED)
    e = (got[0].double() - _ref(dev, name, 0.0)[0]).norm() / _ref(dev, name, 0.0)[0].norm()
    assert float(e) > 10 * _budget(BF, "out")[1]               # the mask really was applied


@lru_cache(maxsize=None)
def _h12(dev):
    qkv, go = _qkv_go(dev, sum(H12_LENS), 12, 4242)
    return qkv, go, {p: _reference(qkv, go, H12_LENS, 12, p, SEED) for p in (0.0, P_DROP)}


@pytest.mark.parametrize("p", [0.0, P_DROP], ids=["p0", "drop"])
def test_twelve_heads_through_the_ops_layer(dev, p):
    """12 heads x 43 sequences of 1..40 rows = 516 (sequence, head) pairs with ``groups``: ``ops.AttentionQKV`` runs the ``d32s::``
    pair alone, gives the bits of the direct C call (bias sums included), saves neither out nor out_lo, and returns the bias
    gradients; the streaming route with the same seed meets the same float64 reference."""
    from gmlm_amd import ops
    h = 12
    assert {1, 32, 33} <= set(H12_LENS) and len(H12_LENS) * h >= 512 > (len(H12_LENS) - 1) * h >= ops.D32_SHORT_MIN_PAIRS
    qkv, go, refs = _h12(dev)
    cu, groups = _cu(H12_LENS, dev), ops.pack_sequence_groups(H12_LENS).to(dev)
    assert ops._d32_short_path(groups, BF, D, max(H12_LENS), len(H12_LENS), h)
    box = {}

    def fn():
        x = qkv.clone().requires_grad_(True)
        masters = tuple(torch.zeros(h * D, device=dev, requires_grad=True) for _ in range(3))
        if p:
            out = ops.AttentionQKV.apply(x, None, h, SCALE, p, SEED, cu, max(H12_LENS), None, groups, *masters)
        else:
            out = ops.attention_qkv(x, None, h, SCALE, cu_seqlens=cu, max_len=max(H12_LENS), bias_masters=masters, groups=groups)
        saved = [s for s in out.grad_fn.saved_tensors if s is not None]
        assert not any(s.data_ptr() == out.data_ptr() for s in saved) and sum(s.dtype == BF for s in saved) == 1     # qkv alone
        out.backward(go)
        box["r"] = (out.detach(),) + _split(x.grad, h) + (torch.cat([m.grad for m in masters]),)

    ran = kernels_run(fn)
    assert {n for n in ran if n.startswith(("d32s::", "d32::", "attn_"))} == set(d32s_kernels(p > 0, 128)), sorted(ran)
    assert "rows_sum_kernel" in ran, sorted(ran)               # the fixed-order combination of the per-item bias sums
    got = box["r"]
    assert all(bool(torch.isfinite(t).all()) for t in got)
    _check(got, refs[p])
    direct = _run(qkv, go, cu, groups, max(H12_LENS), h, p, SEED, True)
    assert _same_bits(got[:4], direct[:4]) and torch.equal(got[4], direct[5])
    _check(_stream_route(qkv, go, cu, max(H12_LENS), h, p, SEED), refs[p])


def test_odd_head_count_stays_on_the_streaming_kernels(dev):
    """The entry points refuse an odd ``h`` (a work item is a pair of heads) and the dispatch rule carries ``h % 2 == 0``: 3 heads
    x 171 sequences = 513 pairs with ``groups`` give the right result on the ``d32::`` kernels, and no ``d32s::`` kernel runs."""
    from gmlm_amd import _lib, ops
    h, lens = 3, tuple(1 + i % 6 for i in range(171))
    qkv, go = _qkv_go(dev, sum(lens), h, 333)
    cu, groups = _cu(lens, dev), ops.pack_sequence_groups(lens).to(dev)
    assert len(lens) * h >= ops.D32_SHORT_MIN_PAIRS and not ops._d32_short_path(groups, BF, D, max(lens), len(lens), h)
    box = {}

    def fn():
        x = qkv.clone().requires_grad_(True)
        out = ops.attention_qkv(x, None, h, SCALE, cu_seqlens=cu, max_len=max(lens), groups=groups)
        out.backward(go)
        box["r"] = (out.detach(),) + _split(x.grad, h)

    ran = kernels_run(fn)
    assert any(n.startswith("d32::") for n in ran) and not any(n.startswith("d32s::") for n in ran), sorted(ran)
    _check(box["r"], _reference(qkv, go, lens, h))
    with pytest.raises(_lib.GmlmHipError, match="even"):
        _c_call(qkv, go, cu, groups, max(lens), h)


def _rel(got, ref):
    return float((got.double() - ref).norm()) / float(ref.norm())


def test_delta_is_no_worse_than_the_streaming_route_with_out_lo(dev):
    """rowsum(dS) = 0 is not observable; dQ on a case with large |dO| |O| is: V and dO carry a common offset, so delta = dO . O is
    large against dP - delta.  dQ of the new route (delta = sum_k P dP in fp32) is no further from float64 than dQ of the streaming
    route with its out + out_lo delta: new <= 2 x streaming + the l2 budget of ``_budget``."""
    lens, h = (31, 33, 1, 63), 2
    qkv, go = _qkv_go(dev, sum(lens), h, 777)
    qkv = qkv.clone()
    qkv[:, 2 * h * D:] += 6.0                                  # V: |O| ~ 6
    go = (go + 3.0).to(BF)                                     # dO . O ~ 32 * 18 per row
    cu = _cu(lens, dev)
    ref = _reference(qkv, go, lens, h)
    new = _run(qkv, go, cu, torch.tensor([0, 4], dtype=torch.int32, device=dev), max(lens), h)
    old = _stream_route(qkv, go, cu, max(lens), h, 0.0, 0)
    e_new, e_old = _rel(new[1], ref[1]), _rel(old[1], ref[1])
    print(f"  dq l2 rel error: d32s {e_new:.3e}, streaming with out_lo {e_old:.3e}")
    assert e_new <= 2 * e_old + _budget(BF, "dq")[1], (e_new, e_old)


@pytest.mark.parametrize("p", [0.0, P_DROP], ids=["p0", "drop"])
def test_bias_sums_against_float64_and_the_parent_route(dev, p):
    """dbias = column sums of dQ | dK | dV: against the float64 sums of the reference gradients, and no worse than twice the error
    of the parent route (``ops.column_sum`` over the streaming kernels' bf16 dqkv) on the same inputs.  The key-bias third is
    mathematically zero (the rows of dS sum to zero): it is compared in absolute terms with the parent's absolute error."""
    name = "full_tile_three_groups"
    lens, h, _, _ = CASES[name]
    qkv, go = _problem(dev, name)
    from gmlm_amd import ops
    cu, groups = _cu(lens, dev), ops.pack_sequence_groups(lens).to(dev)
    ref = _ref(dev, name, p)
    want = [r.sum(0) for r in ref[1:]]                         # float64 [h * 32] each: dq, dk, dv
    new = _split(_run(qkv, go, cu, groups, max(lens), h, p, SEED, True)[5].double(), h)
    old = _split(_stream_route(qkv, go, cu, max(lens), h, p, SEED, True)[4].double(), h)
    for i, nm in ((0, "q"), (2, "v")):
        e_new, e_old = float((new[i] - want[i]).norm()), float((old[i] - want[i]).norm())
        print(f"  d bias_{nm}: |error| d32s {e_new:.3e}, column_sum over the streaming dqkv {e_old:.3e}, |sums| {float(want[i].norm()):.3e}")
        assert e_new <= 2 * e_old, (nm, e_new, e_old)
    scale_k = float(ref[2].abs().max())
    assert float(want[1].abs().max()) <= 1e-9 * scale_k * sum(lens)         # the reference's key-bias sums: rounding noise of float64
    a_new, a_old = float((new[1] - want[1]).abs().max()), float((old[1] - want[1]).abs().max())
    print(f"  d bias_k (mathematically 0): max |error| d32s {a_new:.3e}, parent {a_old:.3e}")
    assert a_new <= 2 * a_old, (a_new, a_old)
