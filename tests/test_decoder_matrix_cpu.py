"""Coverage guard of the decoder matrix (no GPU needed): the rmsnorm_*, qknorm_rope_*, swiglu_* and causal128::* kernels compiled
into the library's gfx950 code objects must be exactly the kernels that tests/test_gpu_decoder_matrix.py names in its case
tables (plus ``UNREACHABLE``, empty); the launch arithmetic of decoder_kernels.hip and attn_causal.hip (the CH dispatch,
rope_bwd_blocks and the passes of the RoPE backward, the SwiGLU grid, the causal grids), restated here and tied to the
constants in the sources, must give every case the chunk count, blocks, passes, live groups, grid and trips it claims; the
budgets used on the saturated SwiGLU gates and on the all-zero RMSNorm row are held against the kernels' own expressions
evaluated in fp32; and everything the entry points decide before any launch (zero-size acceptances, refusals) is repeated on
the host with stand-in pointers."""
import math
import os
import re

import pytest
import torch

from gmlm_amd import _lib
from test_attention_matrix_cpu import _compiled_kernels
from test_gpu_decoder_matrix import (BF, CAUSAL_CASES, CLAMP_L, CLAMP_LENS, DTYPES, EPS, FP, HKV, HQ, PAST_L, PAST_LENS, RMS_CASES, RMS_ROWS,
                                     RMS_WIDTHS, ROPE_CASES, ROPE_MAX_BLOCKS, RPB, SAT_GATES, SHORT_B, SHORT_LS, SWIGLU_CASES,
                                     SWIGLU_GRID_CAP, U, UNREACHABLE, VEC, _is_decoder, causal_kernels, rms_inputs, rms_reference,
                                     rms_stat, rope_dw_depth, rows_sum_depth, swiglu_inputs, swiglu_reference)
from test_gpu_decoder_ops import TN, _stat

A = 16           # a non-null, 16-byte aligned stand-in pointer: the calls that get it are refused before it is dereferenced
CSRC = os.path.join(os.path.dirname(os.path.abspath(_lib.__file__)), "csrc")


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    import gmlm_amd
    return gmlm_amd.lib()


def cdiv(a, b):
    return (a + b - 1) // b


def _named():
    run = set().union(*(c.kernels for c in RMS_CASES), *(c.kernels(dt) for c in ROPE_CASES for dt in DTYPES),
                      *(c.kernels for c in SWIGLU_CASES), *(causal_kernels(dt) for dt in DTYPES))
    assert all(_is_decoder(n) for n in run)
    return run


# ------------------------------------------------------------------------------------------------ 1. compiled == named
def test_every_decoder_kernel_has_a_case_or_a_reason():
    compiled = _compiled_kernels(_is_decoder)
    run = _named()
    listed = run | set(UNREACHABLE)
    assert compiled, "no decoder row kernel or causal attention kernel found in the code objects"
    assert not sorted(compiled - listed), f"compiled but neither in the case tables nor in UNREACHABLE: {sorted(compiled - listed)}"
    assert not sorted(listed - compiled), f"listed but not compiled: {sorted(listed - compiled)}"
    assert not sorted(run & set(UNREACHABLE)), f"both run by a case and listed as unreachable: {sorted(run & set(UNREACHABLE))}"
    assert not UNREACHABLE
    count = lambda prefix: len({n for n in compiled if n.startswith(prefix)})
    # bf16 CH 2 / 4 / 8 and fp32 CH 2 / 4 / 8 / 16; two storage types of everything else; four causal kernels in each
    assert (count("rmsnorm_fwd_kernel<"), count("rmsnorm_bwd_kernel<")) == (7, 7)
    assert (count("qknorm_rope_fwd_kernel<"), count("qknorm_rope_bwd_kernel<")) == (2, 2)
    assert (count("swiglu_fwd_kernel<"), count("swiglu_bwd_kernel<")) == (2, 2)
    assert count("causal128::") == 8 and len(compiled) == 30
    for dt, chs in ((BF, (2, 4, 8)), (FP, (2, 4, 8, 16))):
        assert {n for n in compiled if n.startswith("rmsnorm_fwd_kernel<" + TN[dt])} == {f"rmsnorm_fwd_kernel<{TN[dt]}, {c}>" for c in chs}


def test_case_tables_are_complete():
    """The cases the matrix consists of, by name: dropping one fails here even where another case names the same kernels."""
    assert RMS_ROWS == (1, 3, 4, 5, 9)
    assert [f for f, _ in RMS_WIDTHS[BF]] == [8, 504, 512, 520, 1024, 1032, 2048, 2056, 4088, 4096]
    assert [f for f, _ in RMS_WIDTHS[FP]] == [4, 252, 256, 260, 512, 516, 1024, 1028, 2048, 2052, 4092, 4096]
    assert len(RMS_CASES) == 10 + 12 + 2 and len({c.id for c in RMS_CASES}) == len(RMS_CASES)
    assert [(c.dtype, c.f, c.rows) for c in RMS_CASES if c.zero_row] == [(BF, 520, 5), (FP, 260, 5)]
    assert [c.id for c in ROPE_CASES] == ["b1_l1", "b2_l3", "b3_l1", "pos_len1", "tail"]
    assert [(c.lead, c.hq, c.hkv, c.table) for c in ROPE_CASES] == [((1, 1), 1, 1, 2), ((2, 3), 2, 1, 3), ((3, 1), 2, 1, 4),
                                                                   ((3,), 2, 1, 1), ((5463,), 2, 1, 300)]
    assert ROPE_CASES[3].positions == (-2, 0, 7) and ROPE_CASES[4].pos_mod == 300 and [c.boost for c in ROPE_CASES] == [False] * 4 + [True]
    want = [f"{n}_r{r}_i{i * v if i < 1000 else i}" for n, v in (("bf16", 8), ("fp32", 4)) for r in (1, 3) for i in (1, 3, 1000)]
    want = want[:6] + ["bf16_saturated"] + want[6:] + ["fp32_saturated", "bf16_second_trip", "fp32_second_trip"]
    assert [c.id for c in SWIGLU_CASES] == want
    assert SAT_GATES == (0.0, -0.0, 20.0, -20.0, 30.0, -30.0, 60.0, -60.0, -1.25, -1.3) and math.copysign(1, SAT_GATES[1]) == -1
    assert (HQ, HKV) == (4, 2) and CAUSAL_CASES == ("past_kv_len", "clamp", "short")
    assert PAST_L == 257 and PAST_LENS == (1, 31, 33, 64, 65, 127, 128, 129, 200, 257)
    assert CLAMP_LENS == (CLAMP_L + 5, CLAMP_L, -3, 0) and SHORT_LS == (1, 5, 33) and SHORT_B == 3


# ------------------------------------------------------------------------------------------------- 2. restated dispatch
def grid_cap(blocks, cap=2048):
    return 1 if blocks < 1 else min(blocks, cap)


def rms_ch(f, dtype):
    """GMLM_RMS_DISPATCH"""
    need = cdiv(f // VEC[dtype], 64)
    return 2 if need <= 2 else 4 if need <= 4 else 8 if need <= 8 else {BF: 8, FP: 16}[dtype]


def rope_bwd_blocks(items, dtype):
    return max(1, min(ROPE_MAX_BLOCKS, cdiv(items, RPB[dtype])))


def _src(name):
    with open(os.path.join(CSRC, name)) as fh:
        return fh.read()


def test_the_sources_still_hold_the_restated_constants():
    """The arithmetic below is a restatement; these are the lines of the .hip files it restates.  A change to one of them fails
    here, and the cases have to be re-derived for the new launch arithmetic."""
    dec, cau = _src("decoder_kernels.hip"), _src("attn_causal.hip")
    assert "const int need_ = (int)cdiv(f / Store<T>::kVec, 64);" in dec
    assert re.findall(r"need_ <= (\d+)\) KERNEL<T, (\d+)>", dec) == [("2", "2"), ("4", "4"), ("8", "8")]
    assert "else KERNEL<T, WIDEST>" in dec and "const unsigned grid_ = (unsigned)cdiv(rows, 4);" in dec
    assert len(re.findall(r"GMLM_RMS_DISPATCH\(bf16_t, 8,", dec)) == 2 and len(re.findall(r"GMLM_RMS_DISPATCH\(float, 16,", dec)) == 2
    assert "f > 0 && f <= 4096 && f % v == 0" in dec
    assert f"constexpr int kRopeBwdMaxBlocks = {ROPE_MAX_BLOCKS};" in dec
    assert f"const int64_t rpb = dtype == GMLM_F32 ? {RPB[FP]} : {RPB[BF]};" in dec
    assert "const int64_t item = (it * gridDim.x + blockIdx.x) * RPB + grp;" in dec
    assert "cdiv(items * 16, 256), 256, 0, st>>>((const bf16_t*)qkv" in dec and "cdiv(items * 32, 256), 256, 0, st>>>((const float*)qkv" in dec
    assert "rows_sum_kernel<<<8, 256, 0, st>>>(partial, nb, 256, dq_weight);" in dec
    assert dec.count(f"const int grid = grid_cap(cdiv(rows * (inter / v), 256), {SWIGLU_GRID_CAP});") == 2
    grp, com = _src("attn_grouped.hpp"), _src("attn_common.hpp")      # the host side and the tile constants of causal128 / clamp_kvlen
    assert "constexpr int D = 128;" in cau and "using grouped::Params, grouped::NW, grouped::NT;" in cau
    assert "constexpr int NW = 4, NT = NW * 64, BQ = NW * 32;" in grp
    assert "cdiv(s.len, BQ) * s.n * hq < ((int64_t)1 << 31)" in grp                             # the size check
    assert grp.count("const int64_t tiles = cdiv(s.len, BQ)") == 2 and grp.count(", x, tiles, s.n, ") == 4   # fwd, bwd; x dtype
    assert grp.count("<<<(unsigned)(tiles * seqs * hq), NT, 0, st>>>(x);") == 2                 # fwd, dq
    assert grp.count("<<<(unsigned)(tiles * seqs * hkv), NT, 0, st>>>(x);") == 1                # dkv
    assert "padded(const int32_t* kv_len, int64_t b, int64_t lq, int64_t lk) { return {kv_len, nullptr, b, lq, lk, lq, false}; }" in grp
    assert cau.count("grouped::padded(kv_len, b, lq, lk)") == 2
    assert "if (kvlen > lk_) kvlen = lk_; if (kvlen < 0) kvlen = 0;" in com
    assert "clamp_kvlen(x.a, it.b, it.l));" in cau
    col = _src("colreduce.hpp")
    assert "for (; r + 24 < nrows; r += 32)" in col and "for (; r < nrows; r += 8)" in col      # rows_sum_depth


def test_rmsnorm_cases_select_the_chunk_counts_they_claim():
    for c in RMS_CASES:
        v = VEC[c.dtype]
        assert c.f % v == 0 and 0 < c.f <= 4096 and rms_ch(c.f, c.dtype) == c.ch, (c.id, rms_ch(c.f, c.dtype))
        assert cdiv(c.f // v, 64) <= c.ch                          # the kernel holds the row
        assert c.kernels == {f"rmsnorm_fwd_kernel<{TN[c.dtype]}, {c.ch}>", f"rmsnorm_bwd_kernel<{TN[c.dtype]}, {c.ch}>"}
    for dt, top in ((BF, 8), (FP, 16)):
        v = VEC[dt]
        fs = [c.f for c in RMS_CASES if c.dtype == dt and not c.zero_row]
        need = {f: cdiv(f // v, 64) for f in fs}
        assert {v, 63 * v, 64 * v, 65 * v, 4096 - v, 4096} <= set(fs)
        # either side of every boundary of the dispatch: the last width of CH = k and the first of the next, which has one
        # chunk (lane 0 alone) in its top row of chunks
        for k in (2, 4, 8):
            if k < top:
                lo, hi = 64 * k * v, 64 * k * v + v
                assert lo in fs and hi in fs and need[lo] == k and need[hi] == k + 1 and (hi // v) % 64 == 1
                assert rms_ch(lo, dt) == k and rms_ch(hi, dt) == 2 * k
        assert need[65 * v] == 2 and (65 * v // v) % 64 == 1 and need[64 * v] == 1 and need[63 * v] == 1 and need[v] == 1
        assert {rms_ch(f, dt) for f in fs} == ({2, 4, 8} if dt == BF else {2, 4, 8, 16})
        assert need[4096] == top and need[4096 - v] == top
        # rows: a partly filled block, a full one, one row in a second and in a third block
        rows = {c.rows for c in RMS_CASES if c.dtype == dt}
        assert rows == set(RMS_ROWS) and {(cdiv(r, 4), r % 4) for r in rows} == {(1, 1), (1, 3), (1, 0), (2, 1), (3, 1)}
        for f in fs:                                               # the statistic term is the tree's at every multiple of 64 V
            assert rms_stat(f, dt) >= _stat(f, 64) and (rms_stat(f, dt) == _stat(f, 64)) == (f % (64 * v) == 0), f
    assert rms_stat(520, BF) == (16 + 6 + 2) * U and rms_stat(8, BF) == (8 + 6 + 2) * U and rms_stat(4092, FP) == (64 + 6 + 2) * U


def test_rope_cases_run_the_blocks_passes_and_live_groups_they_claim(lib):
    for c in ROPE_CASES:
        items = c.tokens * (c.hq + c.hkv)
        for i, dt in enumerate(DTYPES):
            rpb, lpr = RPB[dt], 128 // VEC[dt]
            assert rpb * lpr == 256
            blocks = rope_bwd_blocks(items, dt)
            passes = cdiv(items, blocks * rpb)
            left = items - (passes - 1) * blocks * rpb             # head rows of the last pass
            live_last = left - (cdiv(left, rpb) - 1) * rpb         # in the last block that has any
            assert (blocks, passes, live_last) == (c.blocks[i], c.passes[i], c.live_last[i]), (c.id, dt, blocks, passes, live_last)
            assert 0 < live_last <= rpb and cdiv(items * lpr, 256) == cdiv(items, rpb)          # the forward grid
            assert lib.gmlm_qknorm_rope_bwd_workspace_bytes(c.tokens, c.hq, c.hkv, _dt(dt)) == blocks * 256 * 4
            if not c.by_pos:
                assert c.lead[1] <= c.table
    by = {c.id: c for c in ROPE_CASES}
    assert all(by[k].live_last[i] < RPB[dt] for k in ("b1_l1", "b2_l3") for i, dt in enumerate(DTYPES))   # a partly live last block
    assert by["b3_l1"].lead[1] == 1 and by["pos_len1"].table == 1
    tail = by["tail"]
    items = tail.tokens * 3
    assert items == 16389 and all(cdiv(items, RPB[dt]) > ROPE_MAX_BLOCKS for dt in DTYPES)                # the grid is capped
    for i, dt in enumerate(DTYPES):
        per_pass = ROPE_MAX_BLOCKS * RPB[dt]
        assert items - (tail.passes[i] - 1) * per_pass == 5 == tail.live_last[i]                            # block 0 alone, 5 groups
        assert tail.passes[i] * per_pass - items == {BF: 16379, FP: 8187}[dt]                              # dead groups, last pass
    assert tail.passes == (2, 3) and tail.pos_mod == tail.table
    assert rows_sum_depth(1024) == 32 + 2 + 3 + 3 and rope_dw_depth(tail, BF) == 2 + 16 + 40 and rope_dw_depth(tail, FP) == 3 + 8 + 40


def test_swiglu_cases_run_the_grids_and_trips_they_claim():
    for c in SWIGLU_CASES:
        v = VEC[c.dtype]
        assert c.inter % v == 0
        chunks = c.rows * (c.inter // v)
        grid = grid_cap(cdiv(chunks, 256), SWIGLU_GRID_CAP)
        threads = grid * 256
        trips = {cdiv(chunks, threads), cdiv(chunks - (min(chunks, threads) - 1), threads)}
        if c.saturated:
            assert grid == 1 and c.inter % len(SAT_GATES) == 0 and max(abs(g) for g in SAT_GATES) <= 60
            continue
        assert grid == c.grid and trips == set(c.trips) and max(chunks - threads, 0) == c.tail, (c.id, grid, trips, chunks - threads)
    by = {c.id: c for c in SWIGLU_CASES}
    assert (by["bf16_second_trip"].rows * 8200 // 8, by["fp32_second_trip"].rows * 8200 // 4) == (2_100_225, 2_101_250)
    assert SWIGLU_GRID_CAP * 256 == 2_097_152
    for n, v in (("bf16", 8), ("fp32", 4)):
        assert (1000 // v) % 64 != 0 and {(c.rows, c.inter) for c in SWIGLU_CASES if c.id.startswith(n + "_r")} == \
            {(r, i) for r in (1, 3) for i in (v, 3 * v, 1000)}


def test_causal_cases_sit_on_the_edges_they_name():
    bq = 128
    assert cdiv(PAST_L, bq) == 3 and cdiv(CLAMP_L, bq) == 2 and all(cdiv(l, bq) == 1 for l in SHORT_LS)
    for edge in (32, 64, 128):                                     # wave, key tile, workgroup: a length on either side
        assert any(n <= edge for n in PAST_LENS if n >= edge - 1) and edge + 1 in PAST_LENS
    assert 1 in PAST_LENS and PAST_L in PAST_LENS and all(0 < n <= PAST_L for n in PAST_LENS) and sum(n < PAST_L for n in PAST_LENS) == 9
    assert min(SHORT_LS) == 1 and sorted(SHORT_LS)[1] < 32 < max(SHORT_LS) < 64 and SHORT_B > 1
    assert CLAMP_LENS[0] > CLAMP_L and CLAMP_LENS[2] < 0


# ------------------------------------------------------------------------------------------- 3. the budgets, in fp32
def test_swiglu_budgets_hold_on_the_saturated_gates_in_fp32():
    """swiglu_fwd_kernel's and swiglu_bwd_kernel's expressions, operation for operation in torch fp32 on the inputs of the
    saturated case: at most HALF the budget the GPU file applies (before the rounding to the storage type, which has the
    budget's ulp term to itself).  If this fails the gates are at fault, not the budget."""
    for c in (c for c in SWIGLU_CASES if c.saturated):
        gu, gy = swiglu_inputs(c)
        assert gu.dtype == c.dtype
        g, u, d = gu[:, :c.inter].float(), gu[:, c.inter:].float(), gy.float()
        assert {float(x) for x in g[0, :8]} == {0.0, 20.0, -20.0, 30.0, -30.0, 60.0, -60.0}
        one = torch.ones((), dtype=torch.float32)
        y = g / (one + torch.exp(-g)) * u
        sig = one / (one + torch.exp(-g))
        du = d * g * sig
        dg = d * u * sig * (one + g * (one - sig))
        assert all(t_.dtype == torch.float32 for t_ in (y, sig, du, dg))
        assert bool((sig[:, 2] == 1).all()) and bool(((one - sig)[:, 3] == 1).all()) and bool((sig[:, 7] < 1e-25).all())   # saturated
        t = g.double() * (1 - torch.sigmoid(g.double()))
        assert bool((1 + t[:, 8] > 0).all()) and bool((1 + t[:, 9] < 0).all())                  # either side of the zero
        ref = swiglu_reference(gu, gy, c.inter)
        for name, got in (("y", y), ("d up", du), ("d gate", dg)):
            r_, extra = ref[name]
            err = (got.double() - r_).abs()
            assert bool(torch.isfinite(got).all()) and bool((err <= 0.5 * extra).all()), (c.id, name, float((err / extra.clamp_min(1e-300)).max()))


def test_rmsnorm_budgets_hold_on_the_zero_row_in_fp32():
    """rmsnorm_fwd_kernel's and rmsnorm_bwd_kernel's expressions in torch fp32 on the inputs of the zero-row cases: at most half
    the budgets of the GPU file; on the zero row y is exactly 0, rstd is eps^-1/2 within 2 u and da is gs + rstd gy w."""
    eps = torch.tensor(EPS, dtype=torch.float32)
    for c in (c for c in RMS_CASES if c.zero_row):
        for with_b in (True, False):
            a, b, w, gy, gs = rms_inputs(c, with_b)
            s = (a.float() + b.float()).to(c.dtype) if with_b else a     # the stored sum
            z = s.float()
            assert float(z[1].abs().max()) == 0.0 and float(z[0].abs().max()) > 0
            rs = 1.0 / torch.sqrt((z * z).sum(-1, keepdim=True) / c.f + eps)
            y = z * rs * w
            g, xh = gy.float() * w, z * rs
            m = (g * xh).sum(-1, keepdim=True) / c.f
            ds = rs * (g - xh * m) + gs.float()
            assert all(t_.dtype == torch.float32 for t_ in (rs, y, ds))
            rstd_r, yr, y_extra, dsr, ds_extra, _ = rms_reference(s, w, gy, gs, c.f, c.dtype)
            assert bool(((y.double() - yr).abs() <= 0.5 * y_extra).all()), (c.id, with_b)
            assert bool(((ds.double() - dsr).abs() <= 0.5 * ds_extra).all()), (c.id, with_b)
            want = float(eps.double().rsqrt())
            assert float(y[1].abs().max()) == 0.0 and abs(float(rs[1]) - want) <= 2 * U * want
            assert abs(float(rstd_r[1]) - want) <= 1e-6 * want     # the float64 reference takes eps as a double
            zr = gs[1].double() + float(rstd_r[1]) * gy[1].double() * w.double()
            assert bool(((ds[1].double() - zr).abs() <= 0.5 * ds_extra[1]).all())


# ------------------------------------------------------------------------------------------------- 4. host-side decisions
def _dt(dtype):
    return _lib.BF16 if dtype == BF else _lib.F32


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp32"])
def test_calls_with_nothing_to_do_are_accepted_before_any_pointer_is_examined(lib, dtype):
    """Every forward and the causal backward launch nothing for an empty problem: GMLM_OK with NULL everywhere.  (The row
    kernels' backward entry points still zero-fill their weight gradients; the GPU file runs those.)"""
    dt, v = _dt(dtype), VEC[dtype]
    wid, nqk = (HQ + 2 * HKV) * 128, (HQ + HKV) * 128
    assert lib.gmlm_add_rmsnorm_fwd(None, None, None, 0, 520, EPS, None, None, None, dt, None) == 0
    assert lib.gmlm_swiglu_fwd(None, 0, 40, None, dt, None) == 0
    assert lib.gmlm_swiglu_bwd(None, None, 0, 40, None, dt, None) == 0
    assert lib.gmlm_qknorm_rope_fwd(None, wid, None, None, None, 4, 0, 0, HQ, HKV, 128, EPS, None, nqk, None, dt, None) == 0     # [b, 0, w]
    assert lib.gmlm_qknorm_rope_fwd(None, wid, None, None, None, 4, 0, 3, HQ, HKV, 128, EPS, None, nqk, None, dt, None) == 0     # [0, 3, w]
    assert lib.gmlm_qknorm_rope_pos_fwd(None, wid, None, None, None, 4, 0, None, HQ, HKV, 128, EPS, None, nqk, None, dt, None) == 0
    for b in (2, 0):
        assert lib.gmlm_attention_causal_d128_fwd(None, None, None, None, b, HQ, HKV, 0, 0, 128, wid, wid, wid, 0.088, 0.0, None, None,
                                                  None, dt, None) == 0
        assert lib.gmlm_attention_causal_d128_bwd(None, None, None, None, None, None, None, None, b, HQ, HKV, 0, 0, 128, wid, wid, wid,
                                                  0.088, 0.0, None, None, None, wid, wid, wid, dt, None, 0, None) == 0
    # the workspace queries of the empty problems (the operators ask before they call): no division by the zero rows
    assert 0 < lib.gmlm_add_rmsnorm_bwd_workspace_bytes(0, 520) <= lib.gmlm_add_rmsnorm_bwd_workspace_bytes(1, 520)
    assert 0 < lib.gmlm_colstats_workspace_bytes(0, 520) <= lib.gmlm_colstats_workspace_bytes(1, 520)
    assert lib.gmlm_qknorm_rope_bwd_workspace_bytes(0, HQ, HKV, dt) == 256 * 4
    assert lib.gmlm_attention_causal_d128_workspace_bytes(2, HQ, 0) == 4
    # sizes are validated first: an empty problem with a bad size is still refused
    err = lib.gmlm_last_error
    assert lib.gmlm_add_rmsnorm_fwd(None, None, None, 0, 520 + v // 2, EPS, None, None, None, dt, None) == -1 and b"multiple of" in err()
    assert lib.gmlm_add_rmsnorm_fwd(None, None, None, 0, 8192, EPS, None, None, None, dt, None) == -1 and b"4096" in err()
    assert lib.gmlm_add_rmsnorm_bwd(None, None, None, None, None, 0, 0, None, A, dt, None, 0, None) == -1
    assert lib.gmlm_add_rmsnorm_bwd(None, None, None, None, None, 0, 520, None, None, dt, None, 0, None) == -1 and b"null dw" in err()
    assert lib.gmlm_swiglu_fwd(None, 0, 41, None, dt, None) == -1 and b"multiple of" in err()
    assert lib.gmlm_swiglu_bwd(None, None, -1, 40, None, dt, None) == -1
    rope = lambda **k: lib.gmlm_qknorm_rope_fwd(None, k.get("stride", wid), None, None, None, k.get("max_len", 4), k.get("tokens", 0),
                                                k.get("l", 0), HQ, HKV, k.get("d", 128), EPS, None, k.get("out_stride", nqk), None, dt, None)
    assert rope() == 0
    assert rope(d=64) == -1 and b"head dim" in err()
    assert rope(stride=wid - v) == -1 and b"stride" in err()
    assert rope(out_stride=nqk + 1) == -1 and b"stride" in err()
    assert rope(l=5) == -1 and b"table" in err()
    assert rope(max_len=0) == -1 and b"empty" in err()
    assert rope(l=-1) == -1
    assert rope(tokens=-1) == -1 and b"bad sizes" in err()
    assert rope(tokens=6, l=0) == -1 and b"length 0" in err()      # tokens in sequences of length 0: ``t % seq_len``
    assert rope(tokens=6, l=3) == -1 and b"null" in err()          # something to do: now the pointers count
    assert lib.gmlm_qknorm_rope_bwd(None, wid, None, wid, None, None, None, 4, None, 0, 0, HQ, HKV, 128, None, None, dt, None, 0,
                                    None) == -1 and b"dq_weight" in err()
    assert lib.gmlm_qknorm_rope_bwd(None, wid, None, wid, None, None, None, 4, None, 0, 0, HQ, HKV, 128, 1024, 1024 + 256, dt, None, 0,
                                    None) == -1 and b"dq_weight" in err()
    assert lib.gmlm_attention_causal_d128_fwd(None, None, None, None, 2, HQ, 3, 0, 0, 128, wid, wid, wid, 0.088, 0.0, None, None, None, dt,
                                              None) == -1 and b"multiple of" in err()
    assert lib.gmlm_attention_causal_d128_fwd(None, None, None, None, 2, HQ, HKV, 0, 0, 128, wid, wid, wid, 0.088, 0.1, None, None, None, dt,
                                              None) == -1 and b"dropout" in err()
    assert lib.gmlm_attention_causal_d128_bwd(None, None, None, None, None, None, None, None, 2, HQ, HKV, 0, 1, 128, wid, wid, wid, 0.088,
                                              0.0, None, None, None, wid, wid, wid, dt, None, 0, None) == -1 and b"lq == lk" in err()


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp32"])
def test_rope_entry_points_examine_pointers_once_there_is_a_token(lib, dtype):
    """With tokens > 0 every refusal the entry points had before the reordering is still made, in an order that never reaches
    a launch: pointers, pos_ids, rstd, the weight-gradient buffer, the workspace."""
    dt = _dt(dtype)
    wid, nqk = (HQ + 2 * HKV) * 128, (HQ + HKV) * 128
    err = lib.gmlm_last_error
    fwd = lambda qkv=A, out=A, qw=A, cs=A, rstd=A: lib.gmlm_qknorm_rope_fwd(qkv, wid, qw, A, cs, 8, 16, 8, HQ, HKV, 128, EPS, out, nqk,
                                                                          rstd, dt, None)
    assert fwd(qkv=None) == -1 and b"null or not 16-byte aligned" in err()
    assert fwd(out=A + 4) == -1 and b"null or not 16-byte aligned" in err()
    assert fwd(qw=None) == -1 and b"weight / table" in err()
    assert fwd(cs=A + 8) == -1 and b"weight / table" in err()
    assert fwd(rstd=None) == -1 and b"rstd" in err()
    assert lib.gmlm_qknorm_rope_pos_fwd(A, wid, A, A, A, 8, 16, None, HQ, HKV, 128, EPS, A, nqk, A, dt, None) == -1 and b"pos_ids" in err()
    bwd = lambda rstd=A, dq=1024, dk=1024 + 512, ws=A, nbytes=1 << 30: lib.gmlm_qknorm_rope_bwd(
        A, wid, A, wid, A, A, A, 8, rstd, 16, 8, HQ, HKV, 128, dq, dk, dt, ws, nbytes, None)
    assert bwd(rstd=None) == -1 and b"rstd" in err()
    assert bwd(dk=1024 + 256) == -1 and b"dq_weight" in err()
    assert bwd(nbytes=8) == -2 and b"workspace" in err()
    assert bwd(ws=None) == -2 and b"workspace" in err()
    assert lib.gmlm_qknorm_rope_pos_bwd(A, wid, A, wid, A, A, A, 8, A, 16, None, HQ, HKV, 128, 1024, 1024 + 512, dt, A, 1 << 30,
                                        None) == -1 and b"pos_ids" in err()


def test_operators_take_empty_batches_of_padded_rows():
    """ops._rows_view / ops._qkv_rows (host logic): torch gives [b, 0, w] a batch stride of w, which is not 0 * row stride; an
    empty tensor has no rows to be misplaced.  With rows, the batch-stride rule is unchanged."""
    from gmlm_amd import ops
    x = torch.empty(2, 0, 1024)
    assert x.stride(0) != x.shape[1] * x.stride(1)
    assert ops._rows_view(x[..., :512], 4, 128) == 1024 and ops._qkv_rows(x, 1024) == (0, 1024)
    assert ops._qkv_rows(torch.empty(0, 1024), 1024) == (0, 1024)
    y = torch.empty(2, 6, 1024)[:, :3]                             # rows of each batch entry apart: still refused
    with pytest.raises(ValueError, match="batch stride"):
        ops._rows_view(y[..., :512], 4, 128)
    with pytest.raises(ValueError, match="batch stride"):
        ops._qkv_rows(y, 1024)
