"""The Qwen3 row kernels (decoder_kernels.hip: add + RMSNorm, Q/K head norm + RoPE, SwiGLU) and the causal grouped-KV attention
(attn_causal.hip, ``causal128::*``) at the edges of their loops, against float64 torch on the same rounded inputs.  Every case
rounds its inputs to the storage type first, asserts the EXACT set of the family's kernels it launched (read back by name from
the profiler), asserts that a second identical call gives identical bits, and prints its worst error-to-bound ratio.  The union
of the kernels named by the case tables must equal the family's kernels in the built library, and every claim below about
chunk counts, blocks, passes, live groups, grids and trips is recomputed from the restated launch arithmetic
(tests/test_decoder_matrix_cpu.py).  Budgets are those of test_gpu_decoder_ops.py (its docstring derives them); the two places
where this file departs from them are written out under (1) and (2).

1. add + RMSNorm (``RMS_CASES``; each with and without ``b``).  One wave per row, lane j holds the 16-byte chunks j, j + 64, ...
   of the row, CH of them (GMLM_RMS_DISPATCH: the smallest of 2 / 4 / 8 / 16 that covers ceil((f / V) / 64)); ``ch < nch``
   masks the rest.  Widths: V (lane 0 only); 63 V, 64 V, 65 V (the last lane idle, every lane one chunk, lane 0 alone in the
   second chunk); both sides of every CH boundary of the dispatch, the largest width below 4096 and 4096.  Rows 1, 3, 4, 5, 9:
   a partly filled block of four waves, a full one, one row in a second and in a third block.  ``zero_row``: row 1 of 5 is zero
   in ``a`` and ``b``: y is exactly 0 there, rstd is eps^-1/2 (sqrtf and the reciprocal: at most one fp32 ulp = 2 u each, so
   4 u) and da = gs + rstd gy w.
   Budget: test_add_rmsnorm's, with the statistic term counted as the kernel adds: a lane adds ceil((f / V) / 64) V squares in
   sequence before the 6 butterfly steps, so st = (ceil((f / V) / 64) V + log2(64) + 2) u.  That is f / 64 at every multiple of
   64 V and more elsewhere (the lanes that hold the extra chunk).
2. Q/K head norm + RoPE (``ROPE_CASES``).  A head row is LPR = 16 (bf16) / 32 (fp32) lanes, a block holds RPB = 16 / 8 head
   rows; the forward launches cdiv(items, RPB) blocks, the backward min(that, 1024) blocks that stride over the head rows
   (``item = (it * gridDim.x + blockIdx.x) * RPB + grp``); a lane group without a head row reads token 0 / head 0 and must
   neither store nor add to the weight-gradient sums.
     * b1_l1: [1, 1, .] with hq = hkv = 1: 2 head rows, the other 14 / 6 groups of the one block dead.
     * b2_l3: [2, 3, .] with (hq, hkv) = (2, 1): 18 head rows: 2 blocks (bf16) / 3 blocks (fp32), the last with 2 live groups.
     * b3_l1: [3, 1, .]: seq_len = 1, every token at position 0 (``t % 1``) of a table of 4 rows.
     * pos_len1: packed rows at positions -2, 0, 7 against a table of ONE row: all three read row 0.
     * tail: 5463 packed rows, (hq, hkv) = (2, 1): 16,389 head rows; bf16: 2 passes of 1024 x 16, fp32: 3 passes of 1024 x 8, the
       last pass with 5 live groups, all in block 0.  Positions arange % 300 against a table of 300 rows.  dq_weight and
       dk_weight are also compared element for element: a column is a sum of 10,926 / 5,463 terms dn xhat added in a fixed
       order, so |got - ref| <= (depth + 2) u sum |term| with depth the longest chain of additions a term goes through:
       ``passes`` (a thread adds one term per pass) + RPB (the block adds its groups in sequence) + the depth of
       rows_sum_kernel over the 1024 block partials: 8 row lanes of 128 partials each, taken four at a time (a two-level tree
       and one add into the accumulator per 32 rows: ceil(1024 / 32) + 2), up to 3 leftover rows added in sequence, and a
       three-level tree over the lanes.  The 2 are the product's own rounding and the rounding of its factors; |term| is taken
       with the rotation's two products in magnitude (_rot_mag), since dn is itself a difference of two products.
       A dead group that leaked would add (dn xhat)[token 0, head 0] to the q sums; the gradient row of token 0 / head 0 is
       scaled by 16 so that ONE such row is at least 100 times the bound in some column (asserted), and there are 16,379 /
       8,187 dead groups in the last pass.
3. SwiGLU (``SWIGLU_CASES``).  A thread owns 16-byte chunks ``i = block * 256 + thread; i < rows * inter / V; i += grid * 256``
   with grid = min(cdiv(chunks, 256), 8192).  inter = V, 3 V, 1000 (125 / 250 chunks per row: no multiple of a wave) at 1 and 3
   rows; ``second_trip``: 2049 x 8200 (bf16) / 1025 x 8200 (fp32) = 2,100,225 / 2,101,250 chunks against 2,097,152 threads:
   3073 / 4098 threads take a second trip.  ``saturated``: gate columns fixed at ``SAT_GATES``: 0, -0.0, +-20, +-30, +-60, where
   ``1 / (1 + expf(-g))`` is 1 or ~0 and ``1 - sig`` is 0 or 1 in fp32, and -1.25, -1.3, either side of the zero of
   1 + g (1 - sig) (g = -1.278).  |g| <= 60: past ~87 expf overflows and the kernel returns a signed zero where float64 has a
   tiny normal number.  That the budgets of test_swiglu hold at these gates is not assumed: the CPU file evaluates the kernel's
   expressions in fp32 on the same inputs and holds them to half the budget.
4. Causal attention, padded layout, (hq, hkv) = (4, 2), fused and contiguous operands.
     * past_kv_len: l = 257, kv_len = ``PAST_LENS``, a gradient on EVERY output row: out, dq, dk, dv against _causal_reference
       with no mask on the rows at or past kv_len ("query i sees the keys <= i that lie below kv_len[b]", gmlm_hip.h); dk and
       dv of keys at or past kv_len exactly 0.  The case needs the padded queries to carry weight: in the reference the part
       of dk that comes from queries >= kv_len is at least 10% of |dk| for the kv_len = 31 sequence (asserted), so a dkv_kernel
       that stopped its query loop at kv_len fails.
     * clamp: kv_len = l + 5 gives the bits of kv_len = l; kv_len = -3 gives the all-zero sequence of kv_len = 0.
     * short: l = 1, 5, 33 with b = 3 and no kv_len: less than a wave / a tile per sequence through ``item % (b h)``.  At l = 1
       dq and dk are exactly 0 in the reference; they are held to an absolute bound (_one_key_bounds).
5. Calls with nothing to do ([0, f], [0, 2 I], packed [0, w], padded [b, 0, w]) through the operators and through the C entry
   points with NULL data pointers: GMLM_OK, no kernel of the family launched, weight gradients exactly zero."""
import math
import zlib
from dataclasses import dataclass
from functools import lru_cache

import pytest
import torch

from helpers import _close, kernels_run
from test_gpu_decoder_ops import TN, U, _budget, _causal_reference, _elem_check, _rel_l2, _rope_table, _rot, _rot_mag, _same_bits

pytestmark = pytest.mark.gpu

BF, FP = torch.bfloat16, torch.float32
DTYPES = (BF, FP)
VEC = {BF: 8, FP: 4}
DT_ID = {BF: "bf16", FP: "fp32"}
EPS = 1e-6
FAMILY = ("rmsnorm_", "qknorm_rope_", "swiglu_", "causal128::")
UNREACHABLE = {}


def _is_decoder(name):
    """The kernels the CPU guard holds to the case tables below."""
    return name.startswith(FAMILY)


def _seed(name):
    return zlib.crc32(name.encode())


def _family(ran):
    return {n for n in ran if _is_decoder(n)}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


# ------------------------------------------------------------------------------------------------------- 1. add + RMSNorm
@dataclass(frozen=True)
class RmsCase:
    dtype: torch.dtype
    f: int
    rows: int
    ch: int                    # the CH the dispatch must select (asserted through the kernel name)
    zero_row: bool = False

    @property
    def id(self):
        return f"{DT_ID[self.dtype]}_f{self.f}_r{self.rows}" + ("_zero_row" if self.zero_row else "")

    @property
    def kernels(self):
        return frozenset(f"rmsnorm_{k}_kernel<{TN[self.dtype]}, {self.ch}>" for k in ("fwd", "bwd"))


RMS_ROWS = (1, 3, 4, 5, 9)
RMS_WIDTHS = {                 # (f, CH): V; 63 V, 64 V, 65 V; both sides of every CH boundary; the widest below 4096; 4096
    BF: ((8, 2), (504, 2), (512, 2), (520, 2), (1024, 2), (1032, 4), (2048, 4), (2056, 8), (4088, 8), (4096, 8)),
    FP: ((4, 2), (252, 2), (256, 2), (260, 2), (512, 2), (516, 4), (1024, 4), (1028, 8), (2048, 8), (2052, 16), (4092, 16),
         (4096, 16)),
}
RMS_CASES = [RmsCase(dt, f, RMS_ROWS[(i + (dt == FP)) % 5], ch) for dt in DTYPES for i, (f, ch) in enumerate(RMS_WIDTHS[dt])] + \
    [RmsCase(dt, 65 * VEC[dt], 5, 2, zero_row=True) for dt in DTYPES]


def rms_stat(f, dtype):
    """Relative error of the row sum: serial additions per lane + the 6 butterfly steps + 2 (module docstring, 1)."""
    per_lane = -(-(f // VEC[dtype]) // 64) * VEC[dtype]
    return (per_lane + math.log2(64) + 2) * U


def rms_inputs(c, with_b):
    """CPU tensors in the storage type (shared with the fp32 formula check of the CPU file)."""
    g = torch.Generator().manual_seed(c.rows * 7 + c.f + 100_000 * c.zero_row)
    a = torch.randn(c.rows, c.f, generator=g).to(c.dtype)
    b = (0.5 * torch.randn(c.rows, c.f, generator=g)).to(c.dtype) if with_b else None
    if c.zero_row:
        a[1] = 0
        if with_b:
            b[1] = 0
    w = torch.empty(c.f).uniform_(0.5, 1.5, generator=g)
    gy, gs = (torch.randn(c.rows, c.f, generator=g).to(c.dtype) for _ in range(2))
    return a, b, w, gy, gs


def rms_reference(s, w, gy, gs, f, dtype):
    """float64 results of the STORED sum ``s`` and the budgets of test_add_rmsnorm with ``rms_stat``:
    (rstd, y, y extra, ds, ds extra, dw)."""
    sd, wd = s.double(), w.double()
    st = rms_stat(f, dtype)
    rstd = (sd.pow(2).mean(-1, keepdim=True) + EPS).rsqrt()
    yr = sd * rstd * wd
    gr = gy.double() * wd
    xh = sd * rstd
    m = (gr * xh).mean(-1, keepdim=True)
    m_abs = (gr * xh).abs().mean(-1, keepdim=True)
    dsr = gs.double() + rstd * (gr - xh * m)
    extra = 4 * U * (gs.double().abs() + rstd * (gr.abs() + (xh * m).abs())) + rstd * xh.abs() * st * m_abs \
        + 0.5 * st * rstd * (gr.abs() + (xh * m).abs())
    return rstd, yr, yr.abs() * (0.5 * st + 4 * U), dsr, extra, (gy.double() * xh).sum(0)


@pytest.mark.parametrize("with_b", [True, False], ids=["add", "plain"])
@pytest.mark.parametrize("c", RMS_CASES, ids=[c.id for c in RMS_CASES])
def test_add_rmsnorm_matrix(dev, c, with_b):
    from gmlm_amd import ops
    a, b, w, gy, gs = (None if t is None else t.to(dev) for t in rms_inputs(c, with_b))

    def run():
        av, wv = a.clone().requires_grad_(True), w.clone().requires_grad_(True)
        bv = b.clone().requires_grad_(True) if with_b else None
        s, y = ops.add_rmsnorm(av, bv, wv, EPS)
        rstd = y.grad_fn.saved_tensors[2].clone()
        torch.autograd.backward([s, y], [gs, gy])
        return s.detach(), y.detach(), av.grad, (bv.grad if with_b else av.grad), wv.grad, rstd

    box = {}
    ran = kernels_run(lambda: box.setdefault("r", run()))
    print(f"\n{c.id}: {sorted(_family(ran))}")
    assert _family(ran) == set(c.kernels), (sorted(_family(ran)), sorted(c.kernels))
    assert not any(n.startswith(("ln_", "graphnorm_")) for n in ran), ran
    assert _same_bits(run(), box["r"])
    s, y, da, db, dw, rstd = box["r"]
    assert rstd.shape == (c.rows,) and rstd.dtype == torch.float32

    if with_b:
        _elem_check("s", s, a.double() + b.double(), 0.0)
    else:
        assert torch.equal(s, a)
    rstd_r, yr, y_extra, dsr, ds_extra, dwr = rms_reference(s, w, gy, gs, c.f, c.dtype)
    _elem_check("y", y, yr, y_extra)
    _elem_check("da", da, dsr, ds_extra)
    assert torch.equal(da, db)
    _rel_l2("dw", dw, dwr, c.dtype)
    if c.zero_row:
        assert float(s[1].abs().max()) == 0.0 and float(y[1].abs().max()) == 0.0
        want = float(torch.tensor(EPS, dtype=torch.float32).double().rsqrt())       # the kernel's eps is the fp32 1e-6
        err = abs(float(rstd[1]) - want) / want
        print(f"  rstd of the zero row: {float(rstd[1]):.4f}, rel err {err / U:.2f} u")
        assert err <= 4 * U, (float(rstd[1]), want)
        zr = gs[1].double() + float(rstd_r[1]) * gy[1].double() * w.double()        # xhat = 0: no mean term
        _elem_check("da of the zero row", da[1], zr, ds_extra[1])


# -------------------------------------------------------------------------------------------------- 2. Q/K head norm + RoPE
ROPE_MAX_BLOCKS = 1024
RPB = {BF: 16, FP: 8}          # head rows (lane groups) per block of 256 threads


@dataclass(frozen=True)
class RopeCase:
    id: str
    lead: tuple                # (b, l): padded form; (tokens,): by position
    hq: int
    hkv: int
    table: int                 # rows of the cos / sin table
    positions: tuple = ()      # by position: the pos_ids (empty: ``arange % pos_mod``)
    pos_mod: int = 0
    # claims, per dtype (bf16, fp32), held to the restated launch arithmetic by the CPU file
    blocks: tuple = (1, 1)     # blocks of the backward grid
    passes: tuple = (1, 1)     # passes of its grid-stride loop
    live_last: tuple = (0, 0)  # live lane groups of the last block that has any, in the last pass
    boost: bool = False        # token 0 / head 0 gradient row x 16, element-wise weight-gradient bounds

    @property
    def tokens(self):
        return math.prod(self.lead)

    @property
    def by_pos(self):
        return len(self.lead) == 1

    def kernels(self, dtype):
        return frozenset(f"qknorm_rope_{k}_kernel<{TN[dtype]}>" for k in ("fwd", "bwd"))


ROPE_CASES = [
    RopeCase("b1_l1", (1, 1), 1, 1, 2, live_last=(2, 2)),
    RopeCase("b2_l3", (2, 3), 2, 1, 3, blocks=(2, 3), live_last=(2, 2)),
    RopeCase("b3_l1", (3, 1), 2, 1, 4, blocks=(1, 2), live_last=(9, 1)),
    RopeCase("pos_len1", (3,), 2, 1, 1, positions=(-2, 0, 7), blocks=(1, 2), live_last=(9, 1)),
    RopeCase("tail", (5463,), 2, 1, 300, pos_mod=300, blocks=(1024, 1024), passes=(2, 3), live_last=(5, 5), boost=True),
]


def rows_sum_depth(nrows):
    """Longest chain of additions a partial row goes through in rows_sum_kernel (module docstring, 2)."""
    return -(-nrows // 32) + 2 + 3 + 3


def rope_dw_depth(c, dtype):
    i = DTYPES.index(dtype)
    return c.passes[i] + RPB[dtype] + rows_sum_depth(c.blocks[i])


def _sum_check(name, got, ref, bound):
    ratio = (got.double() - ref).abs() / bound
    worst, nbad = float(ratio.max()), int((ratio > 1).sum())
    print(f"  {name}: max err / bound = {worst:.3f}, {nbad} of {ratio.numel()} outside")
    assert bool(torch.isfinite(got).all()) and nbad == 0, (name, worst, nbad)


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp32"])
@pytest.mark.parametrize("c", ROPE_CASES, ids=[c.id for c in ROPE_CASES])
def test_qknorm_rope_matrix(dev, c, dtype):
    """Formulas and budgets of test_qknorm_rope; different q and k weights, input rows 64 elements wider than the fused width."""
    from gmlm_amd import ops
    g = torch.Generator().manual_seed(_seed(c.id))
    hq, hkv, nh, tok = c.hq, c.hkv, c.hq + c.hkv, c.tokens
    wid, nqk = (hq + 2 * hkv) * 128, nh * 128
    buf = torch.randn(*c.lead, wid + 64, generator=g).to(dev, dtype)
    assert buf[..., :wid].stride(-2) == wid + 64
    qw, kw = (torch.empty(128).uniform_(0.5, 1.5, generator=g).to(dev) for _ in range(2))
    cs = _rope_table(c.table, 1e6, dev)
    go = torch.randn(tok, nqk, generator=g)
    if c.boost:
        go[0, :128] *= 16
    go = go.view(*c.lead, nqk).to(dev, dtype)
    if c.by_pos:
        pos = torch.tensor(c.positions, device=dev) if c.positions else torch.arange(tok, device=dev) % c.pos_mod
        read = pos.clamp(0, c.table - 1)
    else:
        pos, read = None, torch.arange(tok, device=dev) % c.lead[1]
    assert int(read.max()) < c.table

    def run():
        bv, qv, kv = buf.clone().requires_grad_(True), qw.clone().requires_grad_(True), kw.clone().requires_grad_(True)
        out = ops.qknorm_rope(bv[..., :wid], qv, kv, cs, hq, hkv, EPS, pos_ids=pos)
        out.backward(go)
        assert float(bv.grad[..., wid:].abs().max()) == 0.0        # the columns outside the fused rows
        return out.detach(), bv.grad[..., :wid].contiguous(), qv.grad, kv.grad

    box = {}
    ran = kernels_run(lambda: box.setdefault("r", run()))
    print(f"\n{c.id}: {sorted(_family(ran))}")
    assert _family(ran) == set(c.kernels(dtype)), sorted(_family(ran))
    assert _same_bits(run(), box["r"])
    out, dx, dqw, dkw = box["r"]

    x = buf[..., :wid].double().reshape(tok, hq + 2 * hkv, 128)[:, :nh]
    wd = torch.cat([qw.double().expand(hq, 128), kw.double().expand(hkv, 128)])[None]
    cos, sin = cs[read, 0].double()[:, None, :], cs[read, 1].double()[:, None, :]
    st = (128 / (128 // VEC[dtype]) + math.log2(128 // VEC[dtype]) + 2) * U         # _stat(128, lanes per head row)
    rstd = (x.pow(2).mean(-1, keepdim=True) + EPS).rsqrt()
    xh = x * rstd
    n = xh * wd
    _elem_check("out", out.view(tok, nh, 128), _rot(n, cos, sin), _rot_mag(n, cos, sin) * (0.5 * st + 5 * U))
    gd = go.double().view(tok, nh, 128)
    dn, dn_mag = _rot(gd, cos, -sin), _rot_mag(gd, cos, sin)
    gr = dn * wd
    m = (gr * xh).mean(-1, keepdim=True)
    m_abs = (dn_mag * wd * xh.abs()).mean(-1, keepdim=True)
    dxr = rstd * (gr - xh * m)
    extra = rstd * ((4 * U + 0.5 * st) * (dn_mag * wd + (xh * m).abs()) + xh.abs() * (st + 4 * U) * m_abs)
    dxg = dx.view(tok, hq + 2 * hkv, 128)
    _elem_check("dx (q | k)", dxg[:, :nh], dxr, extra)
    assert float(dxg[:, nh:].abs().max()) == 0.0                   # V columns: no gradient from this op
    terms = dn * xh
    ref_q, ref_k = terms[:, :hq].sum((0, 1)), terms[:, hq:].sum((0, 1))
    _rel_l2("dq_weight", dqw, ref_q, dtype)
    _rel_l2("dk_weight", dkw, ref_k, dtype)
    if c.boost:
        depth = rope_dw_depth(c, dtype)
        mag = dn_mag * xh.abs()
        bound_q, bound_k = ((depth + 2) * U * t_.sum((0, 1)) for t_ in (mag[:, :hq], mag[:, hq:]))
        _sum_check(f"dq_weight by element (depth {depth})", dqw, ref_q, bound_q)
        _sum_check(f"dk_weight by element (depth {depth})", dkw, ref_k, bound_k)
        seen = float((terms[0, 0].abs() / bound_q).max())
        print(f"  one leaked copy of token 0 / head 0: {seen:.0f} x the bound in its largest column")
        assert seen >= 100, seen


# ----------------------------------------------------------------------------------------------------------------- 3. SwiGLU
SWIGLU_GRID_CAP = 8192
SAT_GATES = (0.0, -0.0, 20.0, -20.0, 30.0, -30.0, 60.0, -60.0, -1.25, -1.3)


@dataclass(frozen=True)
class SwigluCase:
    id: str
    dtype: torch.dtype
    rows: int
    inter: int
    grid: int = 1              # claims, held to the restated launch arithmetic by the CPU file
    trips: tuple = (1,)        # passes of the grid-stride loop that threads with a chunk make
    tail: int = 0              # threads that make the second trip
    saturated: bool = False

    @property
    def kernels(self):
        return frozenset(f"swiglu_{k}_kernel<{TN[self.dtype]}>" for k in ("fwd", "bwd"))


def _swiglu_cases():
    out = []
    for dt in DTYPES:
        v, n = VEC[dt], DT_ID[dt]
        for rows in (1, 3):
            for inter in (v, 3 * v, 1000):
                out.append(SwigluCase(f"{n}_r{rows}_i{inter}", dt, rows, inter, grid=-(-(rows * inter // v) // 256)))
        out.append(SwigluCase(f"{n}_saturated", dt, 3, 40, saturated=True))
    out.append(SwigluCase("bf16_second_trip", BF, 2049, 8200, grid=8192, trips=(1, 2), tail=3073))
    out.append(SwigluCase("fp32_second_trip", FP, 1025, 8200, grid=8192, trips=(1, 2), tail=4098))
    return out


SWIGLU_CASES = _swiglu_cases()


def swiglu_inputs(c, device="cpu"):
    """(gate_up, dy) in the storage type; the saturated case fixes gate column j at SAT_GATES[j % 10] (shared with the fp32
    formula check of the CPU file, which is why the generator runs on the CPU for every case but the large ones)."""
    big = c.rows * c.inter > 1 << 20
    g = torch.Generator(device=device if big else "cpu").manual_seed(_seed(c.id))
    where = device if big else "cpu"
    gu = 2.0 * torch.randn(c.rows, 2 * c.inter, generator=g, device=where)
    gy = torch.randn(c.rows, c.inter, generator=g, device=where)
    if c.saturated:
        gu[:, :c.inter] = torch.tensor(SAT_GATES)[torch.arange(c.inter) % len(SAT_GATES)]
    return gu.to(device, c.dtype), gy.to(device, c.dtype)


def swiglu_reference(gu, gy, inter):
    """float64 results and the absolute budget terms of test_swiglu: {name: (ref, extra)}."""
    gt, up, d = gu[:, :inter].double(), gu[:, inter:].double(), gy.double()
    sig = torch.sigmoid(gt)
    yr = gt * sig * up
    dup = d * gt * sig
    t = gt * (1 - sig)
    dgate = d * up * sig * (1 + t)
    return {"y": (yr, yr.abs() * 12 * U), "d up": (dup, dup.abs() * 12 * U),
            "d gate": (dgate, (d * up * sig).abs() * (1 + t.abs()) * 16 * U)}


@pytest.mark.parametrize("c", SWIGLU_CASES, ids=[c.id for c in SWIGLU_CASES])
def test_swiglu_matrix(dev, c):
    from gmlm_amd import ops
    gu, gy = swiglu_inputs(c, dev)
    inter = c.inter
    if c.saturated:
        gates = gu[0, :len(SAT_GATES)].double().tolist()
        assert max(abs(x) for x in gates) == 60.0 and gates[8] == -1.25 and -1.31 < gates[9] < -1.28
        assert math.copysign(1.0, gates[1]) == -1.0                # -0.0 survives the rounding to the storage type

    def run():
        v = gu.clone().requires_grad_(True)
        y = ops.swiglu(v)
        y.backward(gy)
        return y.detach(), v.grad

    box = {}
    ran = kernels_run(lambda: box.setdefault("r", run()))
    print(f"\n{c.id}: {sorted(_family(ran))}")
    assert _family(ran) == set(c.kernels), sorted(_family(ran))
    assert not any(n.startswith("bias_gelu_") for n in ran), ran
    assert _same_bits(run(), box["r"])
    y, dgu = box["r"]
    assert y.shape == (c.rows, inter) and dgu.shape == gu.shape
    slab = 256                                                     # rows per comparison: the float64 temporaries stay small
    for r0 in range(0, c.rows, slab):
        r1 = min(c.rows, r0 + slab)
        ref = swiglu_reference(gu[r0:r1], gy[r0:r1], inter)
        tag = f" rows {r0}..{r1 - 1}" if c.rows > slab else ""
        _elem_check("y" + tag, y[r0:r1], *ref["y"])
        _elem_check("d up" + tag, dgu[r0:r1, inter:], *ref["d up"])
        _elem_check("d gate" + tag, dgu[r0:r1, :inter], *ref["d gate"])


# ---------------------------------------------------------------------------------------------------- 4. causal attention
HQ, HKV = 4, 2
NQ, NK = HQ * 128, HKV * 128
SCALE = 128 ** -0.5
PAST_L = 257
PAST_LENS = (1, 31, 33, 64, 65, 127, 128, 129, 200, 257)
CLAMP_L = 129
CLAMP_LENS = (CLAMP_L + 5, CLAMP_L, -3, 0)
SHORT_LS = (1, 5, 33)
SHORT_B = 3
CAUSAL_CASES = ("past_kv_len", "clamp", "short")


def causal_kernels(dtype):
    return frozenset(f"causal128::{k}<{TN[dtype]}>" for k in ("fwd_kernel", "delta_kernel", "dq_kernel", "dkv_kernel"))


def _causal_run(qkv, go, kv_len, fused):
    """out, dq, dk, dv of ops.causal_attention on fused or contiguous operands; asserts the kernels and the repeat."""
    from gmlm_amd import ops

    def run():
        if fused:
            x = qkv.clone().requires_grad_(True)
            q, k, v = x[..., :NQ], x[..., NQ:NQ + NK], x[..., NQ + NK:]
        else:
            q, k, v = (t.clone().contiguous().requires_grad_(True) for t in (qkv[..., :NQ], qkv[..., NQ:NQ + NK], qkv[..., NQ + NK:]))
        out = ops.causal_attention(q, k, v, kv_len, HQ, HKV, SCALE)
        out.backward(go)
        grads = (x.grad[..., :NQ], x.grad[..., NQ:NQ + NK], x.grad[..., NQ + NK:]) if fused else (q.grad, k.grad, v.grad)
        return (out.detach(),) + tuple(t.contiguous() for t in grads)

    box = {}
    ran = kernels_run(lambda: box.setdefault("r", run()))
    assert _family(ran) == set(causal_kernels(qkv.dtype)), sorted(_family(ran))
    assert not any(n.startswith(("attn_", "d128::")) for n in ran), ran
    assert _same_bits(run(), box["r"])
    assert all(bool(torch.isfinite(t).all()) for t in box["r"])
    return box["r"]


def _qkv_go(dev, dtype, b, l, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(b, l, NQ + 2 * NK, generator=g).to(dev, dtype), torch.randn(b, l, NQ, generator=g).to(dev, dtype))


def _reference(qkv, go, kv_len):
    return _causal_reference(qkv[..., :NQ], qkv[..., NQ:NQ + NK], qkv[..., NQ + NK:], go, kv_len, HQ, HKV, SCALE)


@lru_cache(maxsize=None)
def _past_problem(dev, dtype):
    """Inputs and the float64 reference of the past_kv_len case, computed once for the fused and the contiguous run."""
    qkv, go = _qkv_go(dev, dtype, len(PAST_LENS), PAST_L, 71)
    kv_len = torch.tensor(PAST_LENS, dtype=torch.int32, device=dev)
    valid = (torch.arange(PAST_L, device=dev)[None, :] < kv_len[:, None])[..., None]            # [b, l, 1]
    ref = _reference(qkv, go, kv_len)
    # the reference is linear in go: what the queries at or past kv_len add to dk
    dk_valid_only = _reference(qkv, go * valid, kv_len)[2]
    i31 = PAST_LENS.index(31)
    share = float((ref[2][i31] - dk_valid_only[i31]).norm()) / float(ref[2][i31].norm())
    return qkv, go, kv_len, valid, ref, share


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp32"])
@pytest.mark.parametrize("fused", [False, True], ids=["contiguous", "fused_qkv"])
def test_causal_rows_at_and_past_kv_len(dev, fused, dtype):
    qkv, go, kv_len, valid, ref, share = _past_problem(dev, dtype)
    print(f"\n  share of |dk| of the kv_len = 31 sequence that comes from queries >= kv_len: {share:.2f}")
    assert share >= 0.10, share
    got = _causal_run(qkv, go, kv_len, fused)
    for name, g_, r_ in zip(("out", "dq", "dk", "dv"), got, ref):
        _close(name, g_, r_, *_budget(dtype, name))
    for name, g_, r_ in zip(("out", "dq"), got, ref):              # the two halves apart: neither hides behind the other
        _close(name + " of rows < kv_len", g_ * valid, r_ * valid, *_budget(dtype, name))
        _close(name + " of rows >= kv_len", g_ * ~valid, r_ * ~valid, *_budget(dtype, name))
    for name, g_, r_ in zip(("dk", "dv"), got[2:], ref[2:]):
        assert float((r_ * ~valid).abs().max()) == 0.0
        assert float((g_ * ~valid).abs().max()) == 0.0, f"{name} of a key at or past kv_len is not zero"


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp32"])
@pytest.mark.parametrize("fused", [False, True], ids=["contiguous", "fused_qkv"])
def test_causal_kv_len_is_clamped(dev, fused, dtype):
    """Sequences 0 / 1 and 2 / 3 hold the same data: kv_len = l + 5 must give the bits of kv_len = l, kv_len = -3 those of 0."""
    qkv, go = _qkv_go(dev, dtype, 4, CLAMP_L, 73)
    qkv[1], qkv[3], go[1], go[3] = qkv[0], qkv[2], go[0], go[2]
    kv_len = torch.tensor(CLAMP_LENS, dtype=torch.int32, device=dev)
    got = _causal_run(qkv, go, kv_len, fused)
    ref = _reference(qkv, go, kv_len.clamp(0, CLAMP_L))
    for name, g_, r_ in zip(("out", "dq", "dk", "dv"), got, ref):
        _close(name, g_, r_, *_budget(dtype, name))
        assert float(g_[0].abs().max()) > 0 and _same_bits([g_[0]], [g_[1]]), f"{name}: kv_len = l + 5 differs from kv_len = l"
        assert float(g_[2].abs().max()) == 0.0 and float(g_[3].abs().max()) == 0.0, f"{name}: a sequence without keys is not zero"


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp32"])
@pytest.mark.parametrize("fused", [False, True], ids=["contiguous", "fused_qkv"])
@pytest.mark.parametrize("l", SHORT_LS)
def test_causal_short_padded_sequences(dev, l, fused, dtype):
    qkv, go = _qkv_go(dev, dtype, SHORT_B, l, 79 + l)
    got = _causal_run(qkv, go, None, fused)
    ref = _reference(qkv, go, torch.full((SHORT_B,), l, device=dev))
    zero = _one_key_bounds(qkv, go) if l == 1 else {}
    for name, g_, r_ in zip(("out", "dq", "dk", "dv"), got, ref):
        assert g_.shape == r_.shape
        if name in zero:
            assert float(r_.abs().max()) == 0.0
            ratio = g_.double().abs() / zero[name]
            print(f"  {name} (reference 0): max |got| / bound = {float(ratio.max()):.3f}")
            assert bool((ratio <= 1).all()), (name, float(ratio.max()))
        else:
            _close(name, g_, r_, *_budget(dtype, name))


def _one_key_bounds(qkv, go):
    """l = 1: the one probability is 1 whatever q and k are, so dq and dk are exactly 0 and a relative measure has nothing to
    divide by.  The kernels form dS = P (dP - delta) with dP = dO . v (dq / dkv kernels) and delta = dO . O (delta kernel,
    O = v): two fp32 evaluations of ONE 128-term dot product, each within (128 + 2) u sum |dO_i v_i| of it in any order of
    summation, so |dS| <= 2 (128 + 2) u sum |dO_i| |v_i|.  The bf16 kernels carry delta into the MFMA as two bf16 numbers
    (hi + lo), which leaves up to 2^-18 |delta| = 64 u |delta| behind, and round dS and the result to bf16 (1 + 2^-7 covers
    both).  Then dq = scale dS k and dk = scale sum over the query heads of the group of dS q."""
    b = qkv.shape[0]
    bf = qkv.dtype == BF
    q, k, v = (t.double().reshape(b, -1, 128) for t in (qkv[..., :NQ], qkv[..., NQ:NQ + NK], qkv[..., NQ + NK:]))
    rep = HQ // HKV
    ds = (2 * (128 + 2) + 64 * bf) * U * (1 + 2.0 ** -7 * bf) * (go.double().reshape(b, HQ, 128).abs() * v.abs().repeat_interleave(rep, 1)).sum(-1)
    dq = SCALE * ds[..., None] * k.abs().repeat_interleave(rep, 1)
    dk = SCALE * (ds[..., None] * q.abs()).view(b, HKV, rep, 128).sum(2)
    return {"dq": dq.view(b, 1, NQ), "dk": dk.view(b, 1, NK)}


# ------------------------------------------------------------------------------------------------- 5. nothing-to-do calls
ZERO = "zero_words_kernel"


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp32"])
def test_nothing_to_do_through_the_operators(dev, dtype):
    from gmlm_amd import ops
    f, inter, b = 520, 40, 2
    wid, nqk = (HQ + 2 * HKV) * 128, (HQ + HKV) * 128
    cs = _rope_table(4, 1e6, dev)
    res = {}

    def leaf(*shape):
        return torch.zeros(*shape, device=dev, dtype=dtype).requires_grad_(True)

    def weight(n):
        return torch.ones(n, device=dev).requires_grad_(True)

    def calls():
        for with_b in (True, False):
            a, bb, w = leaf(0, f), (leaf(0, f) if with_b else None), weight(f)
            s, y = ops.add_rmsnorm(a, bb, w, EPS)
            assert s.shape == y.shape == (0, f) and y.dtype == dtype
            torch.autograd.backward([s, y], [torch.zeros_like(s), torch.zeros_like(y)])
            assert a.grad.shape == (0, f) and (bb is None or bb.grad.shape == (0, f))
            res[f"rmsnorm dw (b: {with_b})"] = w.grad
        gu = leaf(0, 2 * inter)
        y = ops.swiglu(gu)
        assert y.shape == (0, inter)
        y.backward(torch.zeros_like(y))
        assert gu.grad.shape == (0, 2 * inter)
        for lead, pos in (((0,), torch.zeros(0, dtype=torch.int64, device=dev)), ((b, 0), None)):
            x, qw, kw = leaf(*lead, wid), weight(128), weight(128)
            out = ops.qknorm_rope(x, qw, kw, cs, HQ, HKV, EPS, pos_ids=pos)
            assert out.shape == (*lead, nqk) and out.dtype == dtype
            out.backward(torch.zeros_like(out))
            assert x.grad.shape == x.shape
            res[f"rope dq_weight {lead}"], res[f"rope dk_weight {lead}"] = qw.grad, kw.grad
        for fused in (True, False):
            x = leaf(b, 0, wid)
            q, k, v = x[..., :NQ], x[..., NQ:NQ + NK], x[..., NQ + NK:]
            if not fused:
                q, k, v = (t.detach().contiguous().requires_grad_(True) for t in (q, k, v))
            out = ops.causal_attention(q, k, v, None, HQ, HKV, SCALE)
            assert out.shape == (b, 0, NQ)
            out.backward(torch.zeros_like(out))
            assert (x.grad if fused else q.grad).shape[:2] == (b, 0)

    ran = kernels_run(calls)
    print(f"\n  {sorted(ran)}")
    assert not _family(ran), sorted(_family(ran))
    assert ZERO in ran, ran                                         # the weight gradients are filled by the library
    assert len(res) == 6
    for name, t_ in res.items():
        assert t_.dtype == torch.float32 and float(t_.abs().max()) == 0.0 and bool((t_ == 0).all()), name


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp32"])
def test_nothing_to_do_through_the_c_entry_points(dev, dtype):
    """Sizes are validated, then a call with nothing to do returns GMLM_OK before any pointer is examined: every data pointer is
    NULL here.  The weight gradients a backward still owes are required, and come back exactly zero."""
    from gmlm_amd import ops
    lib, p = ops.lib(), ops._ptr
    dt = 1 if dtype == BF else 0
    assert dt == ops._dt(torch.zeros(1, dtype=dtype))
    f, inter, v = 520, 40, VEC[dtype]
    wid, nqk = (HQ + 2 * HKV) * 128, (HQ + HKV) * 128
    sent = -77.0
    dw = torch.full((f + 64,), sent, device=dev)
    dwt = [torch.full((256 + 64,), sent, device=dev) for _ in range(2)]

    def calls():
        st = ops._stream()
        assert lib.gmlm_add_rmsnorm_fwd(None, None, None, 0, f, EPS, None, None, None, dt, st) == 0
        assert lib.gmlm_add_rmsnorm_bwd(None, None, None, None, None, 0, f, None, p(dw), dt, None, 0, st) == 0
        assert lib.gmlm_swiglu_fwd(None, 0, inter, None, dt, st) == 0
        assert lib.gmlm_swiglu_bwd(None, None, 0, inter, None, dt, st) == 0
        # padded [b, 0, w]: tokens = 0 and seq_len = 0; packed [0, w] by position
        assert lib.gmlm_qknorm_rope_fwd(None, wid, None, None, None, 4, 0, 0, HQ, HKV, 128, EPS, None, nqk, None, dt, st) == 0
        assert lib.gmlm_qknorm_rope_pos_fwd(None, wid, None, None, None, 4, 0, None, HQ, HKV, 128, EPS, None, nqk, None, dt, st) == 0
        assert lib.gmlm_qknorm_rope_bwd(None, wid, None, wid, None, None, None, 4, None, 0, 0, HQ, HKV, 128, p(dwt[0]), p(dwt[0][128:]),
                                        dt, None, 0, st) == 0
        assert lib.gmlm_qknorm_rope_pos_bwd(None, wid, None, wid, None, None, None, 4, None, 0, None, HQ, HKV, 128, p(dwt[1]),
                                            p(dwt[1][128:]), dt, None, 0, st) == 0
        assert lib.gmlm_attention_causal_d128_fwd(None, None, None, None, 2, HQ, HKV, 0, 0, 128, wid, wid, wid, SCALE, 0.0, None, None,
                                                  None, dt, st) == 0
        assert lib.gmlm_attention_causal_d128_bwd(None, None, None, None, None, None, None, None, 2, HQ, HKV, 0, 0, 128, wid, wid, wid,
                                                  SCALE, 0.0, None, None, None, wid, wid, wid, dt, None, 0, st) == 0
        # sizes come first: the same calls with a bad size are refused
        assert lib.gmlm_add_rmsnorm_fwd(None, None, None, 0, f + v // 2, EPS, None, None, None, dt, st) == -1
        assert lib.gmlm_swiglu_fwd(None, 0, inter + 1, None, dt, st) == -1
        assert lib.gmlm_qknorm_rope_fwd(None, wid - v, None, None, None, 4, 0, 0, HQ, HKV, 128, EPS, None, nqk, None, dt, st) == -1
        assert lib.gmlm_qknorm_rope_bwd(None, wid, None, wid, None, None, None, 4, None, 0, 0, HQ, HKV, 128, None, None, dt, None, 0,
                                        st) == -1 and b"dq_weight" in lib.gmlm_last_error()
        assert lib.gmlm_attention_causal_d128_fwd(None, None, None, None, 2, HQ, 3, 0, 0, 128, wid, wid, wid, SCALE, 0.0, None, None,
                                                  None, dt, st) == -1

    ran = kernels_run(calls)
    assert not _family(ran) and ZERO in ran, sorted(ran)
    torch.cuda.synchronize()
    assert bool((dw[:f] == 0).all()) and bool((dw[f:] == sent).all())
    for t_ in dwt:
        assert bool((t_[:256] == 0).all()) and bool((t_[256:] == sent).all())
