"""The ``gqas::`` kernels (include/gmlm_hip_gqa_short.h: LDS-resident short-sequence attention with grouped KV heads at d = 64,
bf16, packed layout with seq_groups; bidirectional and causal) against float64 per-sequence attention with
``repeat_interleave``d K / V on inputs rounded to bf16: forward, dq, dk and dv.  The C entry points are called directly (operands
are slices of ONE fused [T, (hq + 2 hkv) * 64] buffer, gradients slices of ONE dqkv) and through the ops layer.  Every case asserts
the exact ``gqas::`` kernel pair it launched and that no ``bidir::`` / ``gqa::`` kernel ran, that a second identical call gives
identical bits, finiteness, and prints its worst error-to-bound ratio.  tests/test_gqa_short_cpu.py holds the kernels compiled
into the library against the ones named here: there is no unreachable instantiation.

Budgets: ``_budget`` of tests/test_gpu_decoder_ops.py (bf16: max 2e-2, l2 6e-3 for out and 8e-3 for the gradients).  Where the
reference is exactly zero (one key: P = 1, dS = 0) the bound is ``_one_key_bounds`` of tests/test_gpu_gqa_kernels.py.

The shapes are the smallest that cross each edge: one row (R = 32); one past a wave (R = 64); R = 96; exactly 128 rows whose
sequences straddle the 32-row blocks; a full-tile sequence and three groups; the 13-sequence cap; empty sequences inside a group;
a whole group without rows; trailing rows owned by no sequence."""
from functools import lru_cache

import pytest
import torch

from helpers import _close, kernels_run
from test_gpu_decoder_ops import _budget, _same_bits
from test_gpu_gqa_kernels import _one_key_bounds

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
D, SCALE = 64, 64 ** -0.5
NAMES = ("out", "dq", "dk", "dv")
TILES = (32, 64, 96, 128)
SENTINEL = 7.0


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def gqas_kernels(causal, r):
    c = "true" if causal else "false"
    return frozenset((f"gqas::fwd_kernel<{c}, {r}>", f"gqas::bwd_kernel<{c}, {r}>"))


def expected_kernels():
    return set().union(*(gqas_kernels(c, r) for c in (False, True) for r in TILES))


def tile_rows(total_rows):
    """The tile height the host picks: no group holds more rows than the batch has, nor more than 128."""
    return (min(total_rows, 128) + 31) // 32 * 32


def _split(t, hq, hkv):
    nq, nk = hq * D, hkv * D
    return t[..., :nq], t[..., nq:nq + nk], t[..., nq + nk:]


def _reference(qkv, go, lens, hq, hkv, causal):
    """float64 attention, one sequence at a time, K / V heads repeated per group, autograd backward.  Rows past sum(lens) are
    left out.  -> out, dq, dk, dv over the owned rows."""
    rep, r0, outs = hq // hkv, 0, [[], [], [], []]
    for n in lens:
        if n:
            qd, kd, vd = (t[r0:r0 + n].detach().double().requires_grad_(True) for t in _split(qkv, hq, hkv))
            qh = qd.view(n, hq, D).transpose(0, 1)
            kh = kd.view(n, hkv, D).transpose(0, 1).repeat_interleave(rep, 0)
            vh = vd.view(n, hkv, D).transpose(0, 1).repeat_interleave(rep, 0)
            s = (qh @ kh.transpose(-1, -2)) * SCALE
            if causal:
                s = s.masked_fill(~torch.ones(n, n, dtype=torch.bool, device=qkv.device).tril(), float("-inf"))
            o = (torch.softmax(s, -1) @ vh).transpose(0, 1).reshape(n, hq * D)
            o.backward(go[r0:r0 + n].double())
            for acc, t in zip(outs, (o.detach(), qd.grad, kd.grad, vd.grad)):
                acc.append(t)
        r0 += n
    return tuple(torch.cat(a) for a in outs)


def _qkv_go(dev, rows, hq, hkv, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(rows, (hq + 2 * hkv) * D, generator=g).to(dev, BF), torch.randn(rows, hq * D, generator=g).to(dev, BF))


def _cu(lens, dev):
    return torch.tensor((0,) + tuple(lens), dtype=torch.int64).cumsum(0).to(dev, torch.int32)


def _c_call(qkv, go, cu, groups, max_len, hq, hkv, causal):
    """One forward and one backward through the C entry points on slices of the fused buffers; outputs pre-filled with a sentinel.
    -> out, dq, dk, dv, lse (dq | dk | dv are views of one dqkv)."""
    from gmlm_amd import _lib
    lib = _lib.lib()
    t, w = qkv.shape
    q, k, v = _split(qkv, hq, hkv)
    out = torch.full((t, hq * D), SENTINEL, dtype=BF, device=qkv.device)
    lse = torch.full((hq, t), SENTINEL, dtype=torch.float32, device=qkv.device)
    dqkv = torch.full_like(qkv, SENTINEL)
    dq, dk, dv = _split(dqkv, hq, hkv)
    st = torch.cuda.current_stream().cuda_stream
    ns, ng = cu.numel() - 1, groups.numel() - 1
    _lib.check(lib.gmlm_attention_gqa_short_fwd(q.data_ptr(), k.data_ptr(), v.data_ptr(), cu.data_ptr(), ns, max_len, t, hq, hkv, D, w, w,
                                                w, SCALE, 0.0, int(causal), groups.data_ptr(), ng, out.data_ptr(), lse.data_ptr(),
                                                _lib.BF16, st), "gqa_short_fwd")
    _lib.check(lib.gmlm_attention_gqa_short_bwd(q.data_ptr(), k.data_ptr(), v.data_ptr(), go.data_ptr(), lse.data_ptr(), cu.data_ptr(),
                                                ns, max_len, t, hq, hkv, D, w, w, w, SCALE, 0.0, int(causal), groups.data_ptr(), ng,
                                                dq.data_ptr(), dk.data_ptr(), dv.data_ptr(), w, w, w, _lib.BF16, st), "gqa_short_bwd")
    return out, dq, dk, dv, lse


def _run(qkv, go, cu, groups, max_len, hq, hkv, causal):
    """``_c_call`` with the kernel-pair, repeat and finiteness assertions of every case."""
    box = {}
    ran = kernels_run(lambda: box.setdefault("r", _c_call(qkv, go, cu, groups, max_len, hq, hkv, causal)))
    assert {n for n in ran if n.startswith("gqas::")} == set(gqas_kernels(causal, tile_rows(qkv.shape[0]))), sorted(ran)
    assert not any(n.startswith(("bidir::", "gqa::", "attn_", "causal128::")) for n in ran), sorted(ran)
    assert _same_bits(_c_call(qkv, go, cu, groups, max_len, hq, hkv, causal), box["r"])
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


# (lens, hq, hkv, expected group boundaries, tile rows)
CASES = {
    "one_row": ((1,), 1, 1, (0, 1), 32),
    "l33_group3": ((33,), 6, 2, (0, 1), 64),
    "l64_l1_group7": ((64, 1), 7, 1, (0, 2), 96),
    "rows128_straddling": ((31, 2, 33, 30, 32), 3, 1, (0, 5), 128),
    "full_tile_three_groups": ((128, 127, 1, 128), 2, 1, (0, 1, 3, 4), 128),
    "cap13_then_one": ((1,) * 14, 4, 2, (0, 13, 14), 32),
    "empties_inside": ((3, 0, 5, 0, 0, 7), 4, 2, (0, 6), 32),
    "empty_group": ((0,) * 13 + (5,), 2, 2, (0, 13, 14), 32),
}


@lru_cache(maxsize=None)
def _problem(dev, name):
    lens, hq, hkv, _, _ = CASES[name]
    qkv, go = _qkv_go(dev, sum(lens), hq, hkv, 307 + 11 * len(lens) + sum(lens) + hq)
    return qkv, go, {c: _reference(qkv, go, lens, hq, hkv, c) for c in (False, True)}


@pytest.mark.parametrize("causal", [False, True], ids=["bidir", "causal"])
@pytest.mark.parametrize("name", list(CASES))
def test_gqa_short_cases(dev, name, causal):
    from gmlm_amd import ops
    lens, hq, hkv, bounds, tile = CASES[name]
    qkv, go, refs = _problem(dev, name)
    groups = ops.pack_sequence_groups(lens)
    assert tuple(groups.tolist()) == bounds and tile_rows(sum(lens)) == tile
    got = _run(qkv, go, _cu(lens, dev), groups.to(dev), max(lens), hq, hkv, causal)
    ref = refs[causal]
    if max(lens) == 1 and min(lens) == 1:                      # every sequence is one key: P = 1, dq = dk = 0 in the reference
        zero = _one_key_bounds(qkv[:, None], go[:, None], hq, hkv)
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
    lse = got[4]
    assert bool(torch.isfinite(lse).all()) and not bool((lse == SENTINEL).any())


def test_rows_owned_by_no_sequence_keep_their_sentinels(dev):
    """(20, 9) in a batch of 32 rows: the three trailing rows belong to no sequence and are neither read nor written."""
    lens, hq, hkv, rows = (20, 9), 2, 1, 32
    qkv, go = _qkv_go(dev, rows, hq, hkv, 911)
    qkv[29:] = float("nan")                                    # reading them would poison the owned rows
    go[29:] = float("nan")
    groups = torch.tensor([0, 2], dtype=torch.int32, device=dev)
    for causal in (False, True):
        box = {}
        ran = kernels_run(lambda: box.setdefault("r", _c_call(qkv, go, _cu(lens, dev), groups, 20, hq, hkv, causal)))
        assert {n for n in ran if n.startswith("gqas::")} == set(gqas_kernels(causal, 32)), sorted(ran)
        got = box["r"]
        assert _same_bits([t[:29] for t in _c_call(qkv, go, _cu(lens, dev), groups, 20, hq, hkv, causal)[:4]], [t[:29] for t in got[:4]])
        for nm, t in zip(NAMES, got):
            assert bool((t[29:] == SENTINEL).all()), f"{nm}: a row owned by no sequence was written"
            assert bool(torch.isfinite(t[:29]).all()), nm
        assert bool((got[4][:, 29:] == SENTINEL).all()) and bool(torch.isfinite(got[4][:, :29]).all())
        _check(got, _reference(qkv, go, lens, hq, hkv, causal), rows=29)


@pytest.mark.parametrize("causal", [False, True], ids=["bidir", "causal"])
def test_explicit_boundaries_agree_with_one_group_to_rounding(dev, causal):
    """(31, 2, 33 | 30, 32): the same 128 rows as two work items, against float64 and against the one-group result within the
    same budgets (another grouping runs a row's sums over other 32-row blocks: agreement to rounding, not to bits)."""
    name = "rows128_straddling"
    lens, hq, hkv, _, _ = CASES[name]
    qkv, go, refs = _problem(dev, name)
    cu = _cu(lens, dev)
    two = _run(qkv, go, cu, torch.tensor([0, 3, 5], dtype=torch.int32, device=dev), max(lens), hq, hkv, causal)
    one = _c_call(qkv, go, cu, torch.tensor([0, 5], dtype=torch.int32, device=dev), max(lens), hq, hkv, causal)
    _check(two, refs[causal])
    _check(two, [t.double() for t in one[:4]])


@pytest.mark.parametrize("causal", [False, True], ids=["bidir", "causal"])
def test_short_route_against_the_streaming_kernels(dev, causal):
    """The same problem on the streaming family of the same build (``bidir::`` / ``gqa::causal64_*``): within the bf16 budgets."""
    from gmlm_amd import ops
    name = "full_tile_three_groups"
    lens, hq, hkv, _, _ = CASES[name]
    qkv, go, _ = _problem(dev, name)
    cu = _cu(lens, dev)
    short = _c_call(qkv, go, cu, ops.pack_sequence_groups(lens).to(dev), max(lens), hq, hkv, causal)

    def stream():
        x = qkv.clone().requires_grad_(True)
        q, k, v = _split(x, hq, hkv)
        fn = ops.causal_attention_varlen if causal else ops.bidir_gqa_attention_varlen
        out = fn(q, k, v, cu, max(lens), hq, hkv, SCALE, D)
        out.backward(go)
        return (out.detach(),) + _split(x.grad, hq, hkv)

    box = {}
    ran = kernels_run(lambda: box.setdefault("r", stream()))
    assert any(n.startswith("gqa::causal64_" if causal else "bidir::") for n in ran) and not any(n.startswith("gqas::") for n in ran), sorted(ran)
    _check(short, [t.double() for t in box["r"]])


def test_ops_call_path_gives_the_bits_of_the_c_call(dev):
    """ops._causal_varlen_fwd / _bwd with ``groups``: the argument marshalling of the ops layer, bit for bit the direct call."""
    from gmlm_amd import ops
    name = "empties_inside"
    lens, hq, hkv, _, _ = CASES[name]
    qkv, go, _ = _problem(dev, name)
    cu, groups = _cu(lens, dev), ops.pack_sequence_groups(lens).to(dev)
    for causal in (False, True):
        q, k, v = _split(qkv, hq, hkv)
        out, out_lo, lse = ops._causal_varlen_fwd(q, k, v, cu, len(lens), max(lens), hq, hkv, SCALE, False, D, not causal, groups)
        dqkv = torch.empty_like(qkv)
        ops._causal_varlen_bwd(q, k, v, None, None, go, lse, cu, len(lens), max(lens), hq, hkv, SCALE, *_split(dqkv, hq, hkv), D, not causal,
                               groups)
        assert out_lo is None
        want = _c_call(qkv, go, cu, groups, max(lens), hq, hkv, causal)
        assert _same_bits((out,) + _split(dqkv, hq, hkv) + (lse,), want)


# ------------------------------------------------------------------------------------------- the nodes the encoders use
def _rope_table(rows, dev):
    inv = 1.0 / (1e4 ** (torch.arange(0, D, 2, dtype=torch.float) / D))
    fr = torch.arange(rows, dtype=torch.float32)[:, None] * inv[None]
    return torch.stack([fr.cos(), fr.sin()], 1).contiguous().to(dev)


@pytest.mark.parametrize("causal", [False, True], ids=["bidir", "causal"])
def test_rope_nodes_take_the_short_kernels_from_512_pairs_on(dev, causal):
    """ops.rope_bidir_gqa_varlen / rope_causal_gqa_varlen with ``groups`` at 6 / 2 heads: 86 sequences (516 pairs) run only
    ``gqas::`` attention kernels and match float64 attention on the rotated buffer; 85 sequences (510 pairs) run the streaming
    family.  Fails on the commit before the short-sequence grouped kernels (the wrappers take no ``groups``)."""
    from gmlm_amd import ops
    hq, hkv = 6, 2
    node = ops.rope_causal_gqa_varlen if causal else ops.rope_bidir_gqa_varlen
    stream_prefix = "gqa::causal64_" if causal else "bidir::"
    cs = _rope_table(48, dev)
    for n_seq, short in ((86, True), (85, False)):
        lens = tuple(1 + i % 40 for i in range(n_seq))
        qkv, go = _qkv_go(dev, sum(lens), hq, hkv, 53 + n_seq)
        cu, groups = _cu(lens, dev), ops.pack_sequence_groups(lens).to(dev)
        pos = torch.cat([torch.arange(n) for n in lens]).to(dev)

        def run():
            x = qkv.clone().requires_grad_(True)
            y = x * 1.0                                         # a non-leaf buffer, as the QKV GEMM's output is
            out = node(y, cs, pos, cu, max(lens), hq, hkv, D, SCALE, groups=groups)
            out.backward(go)
            return out.detach(), x.grad, y.detach()

        box = {}
        ran = kernels_run(lambda: box.setdefault("r", run()))
        attn = {n for n in ran if n.startswith(("gqas::", "bidir::", "gqa::causal64_", "attn_", "causal128::"))}
        if short:
            assert attn == set(gqas_kernels(causal, 128)), sorted(ran)
        else:
            assert attn and all(n.startswith(stream_prefix) for n in attn), sorted(ran)
        assert _same_bits(run(), box["r"])
        out, dqkv, rotated = box["r"]
        assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(dqkv).all())
        ref = _reference(rotated, go, lens, hq, hkv, causal)
        _close("out", out, ref[0], *_budget(BF, "out"))
        if not short:
            continue
        # the node = rotation, the C entry points on views of the rotated buffer, inverse rotation on ONE dqkv: bit for bit; and
        # the gradients before the inverse rotation are held to float64
        direct = _c_call(rotated, go, cu, groups, max(lens), hq, hkv, causal)
        assert torch.equal(out, direct[0])
        assert torch.equal(dqkv, ops.rope_heads_(torch.cat(direct[1:4], -1), cs, hq + hkv, D, 0, pos.to(torch.int32), inverse=True))
        _check(direct, ref)
