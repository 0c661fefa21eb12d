"""Spiked and masked-spike scores for every streaming attention family ("Spiked and masked-spike scores").

Every streaming forward keeps a running max per query row and defers the rescale of O and l: while no row of a 32-query wave
sees its max grow by more than kDefer = 6 log2 units in a key tile, the old reference is kept; otherwise every row of the wave
moves to its own new max and multiplies O and l by alpha = exp2(m - m_new).  N(0, 1) scores never reach 0 < alpha < 1 after a
wave's first tile (tests/test_softmax_spikes_cpu.py replays the schedule and counts zero such steps), so random inputs run the
rescale only with alpha = 0 on zero accumulators.  The cases here force it, with keys aligned to single queries
(k[j] = a q[i]), and put large finite scores where a mask must hide them.

``softmax_trace`` replays the kernels' schedule in float64 on the CPU (32-query waves, key tiles of ``kt`` keys: 32 for fp32 and
for wide:: / gqaw::, 64 for the bf16 streaming kernels).  It places the deferred spikes, proves on the CPU that every planned
spike does what its case claims (tests/test_softmax_spikes_cpu.py), and evaluates the schedule with the rescale left out
(alpha = 1 in O and l), which must miss the budget by 10x or the inputs would not discriminate.

Spike kinds of a ``Case`` (``_plan``): sequence 0 carries the visible ones,
  jump    a key of the second tile for query n - 10 (causal: n - 1), a key of a middle tile (off the tile boundary) for a query
          of another wave, and a key of the last, partial tile that jumps again for the first query: each >= 7 log2 units;
  defer   for query n - 60, a key 4 - 5 log2 units above the reference its wave keeps (no row of the wave rescales in that
          tile), then a key of a later tile >= 3 units further up: the total against the KEPT reference passes 7, against the
          true max it would not;
  late    (window) query 126 sees no key in its wave's first tile; it meets its band in the tile in which wave-mate 100 jumps;
  table   the jump comes from the added term: relb:: one relative offset of head 0 (every query meets it at key i + 45),
          disent:: one c2p entry and one p2c entry (single (query, key) pairs);
and the other sequences the masked ones, each aligned with a query that sees other keys, >= 20 natural units above its row:
  a  at index kv_len inside a partial tile and in a whole tile past kv_len (padded layouts), V rows = 2^13;
  b  at i + 1 and at the first key of the next tile for query i = 40, and at key 32 for query 31, the last row of its wave: the
     bf16 kernels hold that key in wave 0's diagonal tile although no row of the wave sees it (causal);
  c  at i - window - 1 for the first row of a wave (64) and at i + window + 1 for the last row of the wave before (63): each in a
     tile its wave computes, seen by no row of that wave (window);
  d  the last key of the previous and the first key of the next packed sequence, V rows = 2^13;
  e  a neighbouring sequence of the same work item (LDS-resident short kernels: ``seq_groups``), V rows = 2^13.
The call is repeated with the K and V rows of the masked spikes zeroed, (a, d, e) together and (b, c) key by key: every wave
none of whose queries sees them must keep every bit of out, lse and dq (a row that sees a key moves the rescale decision, and
so the rounding, of its whole wave), and a sequence in which no query sees them every bit of dk / dv, which are
exactly 0 at the keys of (a).  In a packed layout every row is a key of its own sequence, so for (d) and (e) the rows of the
neighbouring sequences themselves are left out.  (A forward that took the row max before the mask select would still give
the right values at these sizes, exp2(-43) being an ordinary fp32 number; it cannot keep the bits.)

Checked per case and per sequence against the family's own float64 reference (imported from its test file) within the family's
own budget (imported): out, dq, dk, dv, the table gradients of relb:: / disent::, and lse (fp32 1e-4 abs; bf16 the per-row bound
of tests/test_gpu_ring_blocks.py).  A bf16 quantity that misses is not given a wider budget: the fp32 twin must meet the fp32
budget and the kernel must be within 2x of ``_floor``, the dense formula in float64 with the kernels' roundings.  The kernels
that ran are asserted by name; a second identical run gives identical bits.

Measured on an MI355X (worst sequence over the cases of a family; max|err| / max|ref|, l2 rel; DESIGN.md section 4 has the full table):
  fp32  out <= 3.9e-6 / 4.3e-7, dq <= 2.9e-6 / 2.2e-6, dk <= 3.2e-6 / 2.2e-6, dv <= 3.4e-6 / 2.2e-6, table gradients <= 1.7e-6 of the
        tensor norm, lse <= 4e-5 abs.
  bf16  out <= 5.6e-3 / 3.7e-3; dq, dk, dv <= 1.2e-2 / 7.8e-3 for wide, gqaw, causal64, bidir and window; table gradients <= 4.0e-4;
        lse <= 4.0e-3 against bounds of 6e-3 .. 5e-2.  Six cases miss the l2 gradient budget in one sequence and pass by the
        floor: d32_bf16_w4_drop in the spiked sequence (dq 1.15e-2 / 1.0e-2, dk 1.4e-2 / 9.0e-3, dv 1.35e-2 / 1.03e-2; floor 1.13e-2 /
        7.7e-3, 1.9e-2 / 9.2e-3, 1.35e-2 / 1.03e-2) and the 8-row neighbour sequences of d32_bf16_w4_packed and the four packed
        bf16 relb / disent cases (dk or dq up to 2.0e-2 / 1.3e-2 against floors of the same size).  Their fp32 twins meet 1e-4 / 1e-5."""
import math
import zlib
from dataclasses import dataclass

import pytest
import torch

import test_gpu_attention_d32 as D32
import test_gpu_attention_matrix as AM
import test_gpu_attention_wide as WD
import test_gpu_bidir_kernels as BD
import test_gpu_deberta_kernels as DB
import test_gpu_d32_short_kernels as D32S
import test_gpu_gqa_kernels as G64
import test_gpu_gqa_short_kernels as GQS
import test_gpu_gqa_wide_kernels as GW
import test_gpu_modernbert_kernels as MB
import test_gpu_mpnet_kernels as MP
from helpers import _close, attn_dropout_scale, kernels_run
from test_gpu_decoder_ops import TN, _causal_reference, _same_bits
from test_gpu_decoder_ops import _budget as _decoder_budget
from test_gpu_ring_blocks import LSE_ABS

pytestmark = pytest.mark.gpu

bf, f32 = torch.bfloat16, torch.float32
INF = float("inf")
LOG2E = 1.0 / math.log(2.0)
SEED = 0x1234_5678_9ABC
K_DEFER = 6.0                      # kDefer of attn_stream.hpp / attn_wide.hpp, log2 units
JUMP_MIN = 7.0                     # a planned jump: the threshold plus one unit of margin
MASK_MARGIN = 20.0                 # natural units a masked spike would top its row by
VBIG = 2.0 ** 13


# ------------------------------------------------------------------------------------------------ 1. the schedule in float64
@dataclass
class Trace:
    kt: int
    jump: torch.Tensor             # [H, lq, nt] growth of the row max against the reference the kernel holds before tile t, log2
                                   # units; +inf for the first key a row sees, 0 while it has seen none
    rescale: torch.Tensor          # [H, nw, nt] bool: wave w multiplies O and l by alpha in tile t
    after_first: torch.Tensor      # [H, nw, nt] bool: ... while some row of the wave already holds a finite reference
    alpha: torch.Tensor            # [H, lq, nt] the factor each row applies (1 where the wave keeps its reference)
    held: torch.Tensor             # [H, lq, nt] bool: the row held a finite reference before tile t
    weights: torch.Tensor          # [H, lq, lk] normalised probabilities of the schedule as the kernels run it
    weights_no_rescale: torch.Tensor   # the same with alpha = 1 in O and l whenever a wave rescales


def softmax_trace(scores_log2, kt):
    """``scores_log2`` [heads, lq, lk] float64: the masked scores in the log2 domain (score * scale * log2 e, added terms
    included), -inf where masked.  Replays attn_fwd_body / widehead::fwd_body: per 32-query wave and tile of ``kt`` keys,
    m_new = max(m, row max); the wave keeps m while every row has m_new - m <= 6 (a row that has seen no key and sees none
    counts as 0), else every row takes m = m_new and alpha = exp2(m_old - m_new) (0 for a row without a reference)."""
    s = scores_log2.double()
    nh, lq, lk = s.shape
    nw, nt = -(-lq // 32), -(-lk // kt)
    rows = nw * 32
    if rows > lq:                                                  # rows past the sequence: they see nothing and never vote
        s = torch.cat([s, s.new_full((nh, rows - lq, lk), -INF)], 1)
    m = s.new_full((nh, rows), -INF)
    jump, alpha, ref, held = (s.new_zeros(nh, rows, nt) for _ in range(4))
    rescale = torch.zeros(nh, nw, nt, dtype=torch.bool)
    after_first = torch.zeros(nh, nw, nt, dtype=torch.bool)
    for t in range(nt):
        rmax = s[:, :, t * kt:(t + 1) * kt].amax(-1)
        m_new = torch.maximum(m, rmax)
        j = torch.where(m_new == -INF, torch.zeros_like(m), torch.where(m == -INF, torch.full_like(m, INF), m_new - m))
        j = torch.nan_to_num(j, nan=0.0, posinf=INF)
        res = (j > K_DEFER).view(nh, nw, 32).any(-1)                                       # [H, nw]
        had = (m > -INF)
        res_r = res.repeat_interleave(32, 1)
        a = torch.where(res_r, torch.where(had, torch.exp2(torch.where(had, m - m_new, torch.zeros_like(m))), torch.zeros_like(m)),
                        torch.ones_like(m))
        m = torch.where(res_r, m_new, m)
        jump[:, :, t], alpha[:, :, t], held[:, :, t] = j, a, had.double()
        ref[:, :, t] = torch.where(m == -INF, torch.zeros_like(m), m)
        rescale[:, :, t] = res
        after_first[:, :, t] = res & had.view(nh, nw, 32).any(-1)
    tile_of = torch.arange(lk) // kt
    p = torch.exp2(s - ref[:, :, tile_of])                                                 # exp2(-inf) = 0
    later = torch.flip(torch.cumprod(torch.flip(alpha, [2]), 2), [2])                      # prod of alpha over tiles >= t
    later = torch.cat([later[:, :, 1:], torch.ones_like(later[:, :, :1])], 2)              # ... over tiles > t
    w = p * later[:, :, tile_of]
    norm = lambda x: torch.where(x.sum(-1, keepdim=True) > 0, x / x.sum(-1, keepdim=True).clamp_min(1e-300), torch.zeros_like(x))
    return Trace(kt, jump[:, :lq], rescale, after_first, alpha[:, :lq], held[:, :lq].bool(), norm(w)[:, :lq], norm(p)[:, :lq])


# ------------------------------------------------------------------------------------------------ 2. the case table
@dataclass(frozen=True)
class Case:
    id: str
    family: str                    # "dense" (ops.Attention / AttentionQKV), "grouped", "window", "relb", "disent"
    dtype: torch.dtype
    d: int
    hq: int
    hkv: int
    layout: str                    # "padded": b sequences of l rows, kv_len per sequence; "packed": cu_seqlens
    lens: tuple                    # kv_len per sequence (padded) or sequence lengths (packed)
    kind: str                      # "jump" (jump + defer [+ late] spikes in sequence 0), "table" (the added term jumps), "masked"
    kt: int                        # keys per tile of the forward kernel
    fwd: frozenset
    bwd: frozenset
    l: int = 0                     # rows per sequence (padded)
    scale: float = 0.0
    causal: bool = False
    window: int = 0                # 0: no band
    p: float = 0.0
    groups: bool = False           # packed: pass pack_sequence_groups (the LDS-resident short kernels)

    @property
    def seqs(self):
        """(first row, rows, visible keys) per sequence"""
        if self.layout == "padded":
            return [(i * self.l, self.l, n) for i, n in enumerate(self.lens)]
        starts = [sum(self.lens[:i]) for i in range(len(self.lens))]
        return [(s, n, n) for s, n in zip(starts, self.lens)]

    @property
    def rows(self):
        return self.l * len(self.lens) if self.layout == "padded" else sum(self.lens)


PAD_L, PAD_KV = 200, (200, 70)                 # 200 = 6 * 32 + 8 = 3 * 64 + 8: >= 4 key tiles, the last one partial
PACKED_LENS = (200, 8, 136, 8)                 # the spiked sequence, then a victim (136 rows) between two 8-row neighbours
GROUP_LENS = (8, 8, 100, 8) + (30,) * 60       # pack_sequence_groups: the first four (124 rows) share one work item; 64 sequences
WINDOW = 60                                    # (96 - 60) % 32 = 4 and % 64 = 36: rows 124 .. 127 of wave 3 meet their band one tile late


def _fam(names):
    names = set(names)
    f = {n for n in names if "fwd" in n}
    return frozenset(f), frozenset(names - f)


def _mk(id_, family, dtype, d, hq, hkv, layout, kind, kt, names, **kw):
    lens = kw.pop("lens", PAD_KV if layout == "padded" else PACKED_LENS)
    l = kw.pop("l", PAD_L if layout == "padded" else 0)
    fwd_, bwd_ = names if isinstance(names, tuple) else _fam(names)
    return Case(id=id_, family=family, dtype=dtype, d=d, hq=hq, hkv=hkv, layout=layout, lens=tuple(lens), kind=kind, kt=kt,
                fwd=frozenset(fwd_), bwd=frozenset(bwd_), l=l, scale=kw.pop("scale", d ** -0.5), **kw)


def _dn(dtype):
    return "bf16" if dtype == bf else "f32"


def _kt(dtype):
    return 64 if dtype == bf else 32


CASES = []
# ---- wide:: (d = 256 / 384 / 512; one 32-row workgroup, 32-key tiles in both dtypes), one dropout instantiation per dtype
for _dt in (f32, bf):
    for _d in WD.DIMS:
        CASES.append(_mk(f"wide_{_dn(_dt)}_d{_d}", "dense", _dt, _d, 2, 2, "padded", "jump", 32, WD._kernel_sets(_dt, _d, 0.0)))
    CASES.append(_mk(f"wide_{_dn(_dt)}_d256_drop", "dense", _dt, 256, 2, 2, "padded", "jump", 32, WD._kernel_sets(_dt, 256, 0.1), p=0.1))
# ---- gqaw:: (d = 256, hq = 4 / hkv = 2): causal and not, padded and packed
for _dt in (f32, bf):
    for _causal in (False, True):
        for _layout in ("padded", "packed"):
            CASES.append(_mk(f"gqaw_{_dn(_dt)}_{'causal' if _causal else 'bidir'}_{_layout}", "grouped", _dt, 256, 4, 2, _layout, "jump",
                             32, GW._kernel_sets(_dt, _causal), causal=_causal, scale=GW.SCALE))
# ---- d32::  rows <= 32: 1 wave, <= 128: 2 waves, else 4.  fp32 (32-key tiles) reaches 3 tiles at 2 and 4 waves, bf16 (64-key
# tiles) only at 4 waves (128 rows are 2 tiles); 1 wave never has a second tile.  NOT_SPIKED (the CPU file) lists the rest.
CASES += [
    _mk("d32_f32_w2", "dense", f32, 32, 2, 2, "padded", "jump", 32, D32.sets(AM.F32, 2, False), l=104, lens=(104, 40)),
    _mk("d32_f32_w4", "dense", f32, 32, 2, 2, "padded", "jump", 32, D32.sets(AM.F32, 4, False)),
    _mk("d32_f32_w4_drop", "dense", f32, 32, 2, 2, "padded", "jump", 32, D32.sets(AM.F32, 4, True), p=0.1),
    _mk("d32_f32_w4_packed", "dense", f32, 32, 2, 2, "packed", "jump", 32, D32.sets(AM.F32, 4, False)),
    _mk("d32_bf16_w4", "dense", bf, 32, 2, 2, "padded", "jump", 64, D32.sets(AM.BF, 4, False)),
    _mk("d32_bf16_w4_drop", "dense", bf, 32, 2, 2, "padded", "jump", 64, D32.sets(AM.BF, 4, True), p=0.1),
    _mk("d32_bf16_w4_packed", "dense", bf, 32, 2, 2, "packed", "jump", 64, D32.sets(AM.BF, 4, False)),
]
# ---- gqa::causal64 and bidir::gqa (d = 64 / 128), hq = 4 / hkv = 2
for _dt in (f32, bf):
    for _layout in ("padded", "packed"):
        CASES.append(_mk(f"causal64_{_dn(_dt)}_{_layout}", "grouped", _dt, 64, 4, 2, _layout, "jump", _kt(_dt), set(G64.causal_kernels(_dt)),
                         causal=True))
        for _d in BD.HEAD_DIMS:
            CASES.append(_mk(f"bidir_{_dn(_dt)}_d{_d}_{_layout}", "grouped", _dt, _d, 4, 2, _layout, "jump", _kt(_dt),
                             set(BD.bidir_kernels(_dt, _d))))
# ---- mbert::window (h = 2, d = 64): a third padded sequence with every key valid carries the band spikes
for _dt in (f32, bf):
    _names = {f"mbert::window_{k}_kernel<{TN[_dt]}>" for k in ("fwd", "delta", "dq", "dkv")}
    CASES.append(_mk(f"window_{_dn(_dt)}_padded", "window", _dt, 64, 2, 2, "padded", "jump", _kt(_dt), _names, window=WINDOW, lens=(200, 70, 200)))
    CASES.append(_mk(f"window_{_dn(_dt)}_packed", "window", _dt, 64, 2, 2, "packed", "jump", _kt(_dt), _names, window=WINDOW))
# ---- relb:: and disent:: (h = 2, d = 64): the jump once from q . k and once from the added term
for _dt in (f32, bf):
    for _kind in ("jump", "table"):
        for _layout in ("padded", "packed"):
            CASES.append(_mk(f"relb_{_dn(_dt)}_{_kind}_{_layout}", "relb", _dt, 64, 2, 2, _layout, _kind, _kt(_dt), MP.expected_kernels(_dt, False)))
            CASES.append(_mk(f"disent_{_dn(_dt)}_{_kind}_{_layout}", "disent", _dt, 64, 2, 2, _layout, _kind, _kt(_dt),
                             DB.expected_kernels(_dt, False), scale=DB.SCALE))
    CASES.append(_mk(f"relb_{_dn(_dt)}_jump_drop", "relb", _dt, 64, 2, 2, "padded", "jump", _kt(_dt), MP.expected_kernels(_dt, True), p=0.1))
    CASES.append(_mk(f"disent_{_dn(_dt)}_table_drop", "disent", _dt, 64, 2, 2, "padded", "table", _kt(_dt), DB.expected_kernels(_dt, True),
                     scale=DB.SCALE, p=0.1))
# ---- masked spikes only, the older families (their rescale branch: test_gpu_kernels.py, test_gpu_decoder_ops.py)
_c128 = lambda t: {f"causal128::{k}<{t}>" for k in ("fwd_kernel", "delta_kernel", "dq_kernel", "dkv_kernel")}
CASES += [
    _mk("attn_f32_d64_masked", "dense", f32, 64, 2, 2, "padded", "masked", 64, AM._generic(AM.F32, 64, 2, 2, False)),
    _mk("attn_f32_d64_masked_packed", "dense", f32, 64, 2, 2, "packed", "masked", 64, AM._generic(AM.F32, 64, 2, 2, False)),
    _mk("attn_bf16_d64_masked", "dense", bf, 64, 2, 2, "padded", "masked", 64, AM._generic(AM.BF, 64, 2, 2, False), l=128, lens=(128, 40)),
    _mk("pipe_d64_masked", "dense", bf, 64, 2, 2, "padded", "masked", 64,
        ({AM.pfwd(64, 4, False)}, {AM.delta(AM.BF), AM.dq(AM.BF, 64, 2, False), AM.dkv(AM.BF, 64, 2, False, 64)})),
    _mk("pipe_d96_masked", "dense", bf, 96, 2, 2, "padded", "masked", 64,
        ({AM.pfwd(96, 4, False)}, {AM.delta(AM.BF), AM.pdq(96, 4, False), AM.pdkv(96, 4, False)})),
    _mk("pipe_d96_masked_packed", "dense", bf, 96, 2, 2, "packed", "masked", 64,
        ({AM.pfwd(96, 4, False)}, {AM.delta(AM.BF), AM.pdq(96, 4, False), AM.pdkv(96, 4, False)})),
    _mk("d128_f32_masked", "dense", f32, 128, 2, 2, "padded", "masked", 32, ({AM.d128("fwd", AM.F32, False)}, AM.d128_bwd(AM.F32, False))),
    _mk("d128_bf16_masked", "dense", bf, 128, 2, 2, "padded", "masked", 64, ({AM.d128("fwd", AM.BF, False)}, AM.d128_bwd(AM.BF, False))),
    _mk("causal128_f32_masked", "grouped", f32, 128, 4, 2, "padded", "masked", 32, _c128(AM.F32), causal=True),
    _mk("causal128_bf16_masked", "grouped", bf, 128, 4, 2, "padded", "masked", 64, _c128(AM.BF), causal=True),
    # the LDS-resident short kernels (bf16, d = 64, <= 128 rows, >= 512 (sequence, head) pairs): padded with kv_len, and packed
    # with seq_groups, where the spiked neighbours share the victim's work item
    _mk("short_masked", "dense", bf, 64, 8, 8, "padded", "masked", 64, ({AM.sfwd(128, False)}, {AM.sbwd(128, False)}), l=128,
        lens=(128, 40) + (128,) * 62),
    _mk("short_groups_masked", "dense", bf, 64, 8, 8, "packed", "masked", 64, ({AM.sfwd(128, False)}, {AM.sbwd(128, False)}),
        lens=GROUP_LENS, groups=True),
    # d32s:: (bf16, d = 32, an even head count, >= 96 pairs) and gqas:: (bf16, d = 64, >= 512 (sequence, query head) pairs)
    _mk("d32s_groups_masked", "dense", bf, 32, 2, 2, "packed", "masked", 64, set(D32S.d32s_kernels(False, 128)), lens=GROUP_LENS, groups=True),
    _mk("gqas_causal_groups_masked", "grouped", bf, 64, 8, 4, "packed", "masked", 64, set(GQS.gqas_kernels(True, 128)), lens=GROUP_LENS,
        groups=True, causal=True),
    _mk("gqas_bidir_groups_masked", "grouped", bf, 64, 8, 4, "packed", "masked", 64, set(GQS.gqas_kernels(False, 128)), lens=GROUP_LENS,
        groups=True),
]
BY_ID = {c.id: c for c in CASES}


def _plan(c):
    """The spikes of a case, as dicts: kind, seq / i (the query), kseq / j (the key, row of ITS sequence), and per kind ``n``
    (which of the three jumps), ``step`` (1: the deferred key, 2: the later one), ``pos`` (masked: a1 a2 b1 b2 c1 c2 d1 d2 e1
    e2) and ``vbig``."""
    out = []
    sp = lambda kind, seq, i, j, kseq=None, **kw: out.append(dict(kind=kind, seq=seq, i=i, kseq=seq if kseq is None else kseq, j=j, **kw))
    n0 = c.seqs[0][1]
    nt = -(-n0 // c.kt)
    if c.kind == "jump":
        # fp32 spikes are k = 6 / 9 / 12 q: every other row scores N(0, a^2) against such a key, so its tile makes waves rescale at
        # random.  The two deferred keys therefore sit in adjacent tiles that hold no jump key (bf16, four 64-key tiles: the
        # spikes are small multiples of q and share the tiles).
        if c.window:
            sp("jump", 0, 150, 170, n=0), sp("jump", 0, 40, 77, n=1), sp("jump", 0, 150, 198, n=2)
            sp("defer", 0, 80, 110, step=1), sp("defer", 0, 80, 131, step=2)
            sp("late", 0, 100, 70, late_row=126)
        else:
            if nt >= 7:
                t1, td1, td2, t2 = 1, 2, 3, 4
            elif c.dtype == f32:
                t1, t2, td1, td2 = 1, 1, 2, 3                       # 104 rows, four 32-key tiles: the second deferred key shares the last
            else:
                t1, td1, t2, td2 = 1, 1, 2, 2
            # three waves: the twice-spiked query in a full one (causal: the last row, which alone sees the partial tile)
            i1, i2 = (n0 - 1, n0 - 35) if c.causal else (n0 - 10, n0 - 100 if n0 >= 150 else 20)
            sp("jump", 0, i1, t1 * c.kt + 6, n=0), sp("jump", 0, i2, t2 * c.kt + 13, n=1), sp("jump", 0, i1, n0 - 2, n=2)
            sp("defer", 0, n0 - 60, td1 * c.kt + 20, step=1), sp("defer", 0, n0 - 60, td2 * c.kt + 3, step=2)
    elif c.kind == "table":
        if c.family == "relb":
            sp("table", 0, 0, 45, rel=45)                           # query i meets it at key i + 45, every i < n0 - 45
        else:
            # distances 72 / 40 and 61 / 29: inside the identity region of the buckets, so each entry meets ONE (query, key) pair
            sp("c2p", 0, n0 - 90, c.kt + 6), sp("p2c", 0, n0 - 30, (nt // 2) * c.kt + 13)
    if c.layout == "padded":
        kvl, l = c.lens[1], c.l
        far = 140 if l == 200 else 100                              # a whole tile past kv_len
        qa = (150, 160) if c.causal else ((75, 100) if l == 200 else (50, 60))
        if l == 104:
            far, qa = 90, (50, 60)
        sp("masked", 1, qa[0], kvl, pos="a1", vbig=True), sp("masked", 1, qa[1], far, pos="a2", vbig=True)
        if c.causal:
            sp("masked", 1, 40, 41, pos="b1", vbig=False), sp("masked", 1, 40, 64, pos="b2", vbig=False)
            sp("masked", 1, 31, 32, pos="b3", vbig=False)
        if c.window:
            sp("masked", 2, 64, 64 - c.window - 1, pos="c1", vbig=False), sp("masked", 2, 63, 63 + c.window + 1, pos="c2", vbig=False)
    else:
        tag = "e" if c.groups else "d"
        sp("masked", 2, 10, c.lens[1] - 1, kseq=1, pos=tag + "1", vbig=True), sp("masked", 2, 50, 0, kseq=3, pos=tag + "2", vbig=True)
        if c.causal:
            sp("masked", 2, 40, 41, pos="b1", vbig=False), sp("masked", 2, 40, 64, pos="b2", vbig=False)
            sp("masked", 2, 31, 32, pos="b3", vbig=False)
        if c.window:
            sp("masked", 2, 64, 64 - c.window - 1, pos="c1", vbig=False), sp("masked", 2, 63, 63 + c.window + 1, pos="c2", vbig=False)
    return out


def _unseen_rows(c):
    """Absolute K / V rows of the masked spikes of kinds a / d / e: zeroing them must not move a bit of the rows compared."""
    return [c.seqs[s["kseq"]][0] + s["j"] for s in _plan(c) if s["kind"] == "masked" and s["vbig"]]


def _hidden_rows(c):
    """Absolute K / V rows of the masked spikes of kinds b / c: other queries of the sequence see these keys."""
    return [c.seqs[s["kseq"]][0] + s["j"] for s in _plan(c) if s["kind"] == "masked" and not s["vbig"]]


def _unaffected(c, keys):
    """For absolute key rows ``keys``: (rows of the 32-query waves in which no query sees any of them, rows of the sequences in
    which no query does).  The wave and not the row: whether a wave rescales is decided by all its rows, so a key that one row
    sees moves the rounding, not the value, of its wave-mates."""
    rows_ok, seq_ok = torch.ones(c.rows, dtype=torch.bool), torch.ones(c.rows, dtype=torch.bool)
    for si, (r0, n, nk) in enumerate(c.seqs):
        own = [k_ - r0 for k_ in keys if r0 <= k_ < r0 + n]
        if own:
            sees = _mask(c, n, nk)[:, own].any(1)
            wave = torch.arange(n) // 32
            hit = torch.zeros(int(wave.max()) + 1, dtype=torch.bool).index_put_((wave,), sees, accumulate=True)
            rows_ok[r0:r0 + n] = ~hit[wave]
            seq_ok[r0:r0 + n] = not bool(sees.any())
    return rows_ok, seq_ok


# ------------------------------------------------------------------------------------------------ 3. inputs
class Data:
    pass


def _qhead(c, kh):
    """the query head a spiked key of KV head ``kh`` is aligned with: one head of the group, not the same one in every group"""
    rep = c.hq // c.hkv
    return kh * rep + kh % rep


def _align(c, dat, qrow, krow, size, literal):
    """k[krow] = a q[qrow] per KV head; ``literal``: a = size, else a so that the score is ``size`` natural units"""
    d = c.d
    for kh in range(c.hkv):
        qv = dat.q[qrow, _qhead(c, kh) * d:(_qhead(c, kh) + 1) * d]
        a = size if literal else size / (c.scale * float(qv.double().pow(2).sum()))
        dat.k[krow, kh * d:(kh + 1) * d] = a * qv


def _mask(c, n, nk):
    i, j = torch.arange(n)[:, None], torch.arange(n)[None, :]
    m = (j < nk) & torch.ones(n, 1, dtype=torch.bool)
    if c.causal:
        m = m & (j <= i)
    if c.window:
        m = m & ((i - j).abs() <= c.window)
    return m


def seq_scores(c, dat, si, extra=()):
    """float64 natural-unit scores [hq, n, n + len(extra)] of sequence ``si`` against its own rows and the absolute key rows
    ``extra`` (foreign keys: q . k alone), the mask [n, n + e] (foreign keys masked) and V [hq, n + e, d]."""
    r0, n, nk = c.seqs[si]
    d, rep = c.d, c.hq // c.hkv
    rows = list(range(r0, r0 + n)) + list(extra)
    q = dat.q[r0:r0 + n].double().view(n, c.hq, d).transpose(0, 1)
    k = dat.k[rows].double().view(len(rows), c.hkv, d).transpose(0, 1).repeat_interleave(rep, 0)
    v = dat.v[rows].double().view(len(rows), c.hkv, d).transpose(0, 1).repeat_interleave(rep, 0)
    s = q @ k.transpose(1, 2)
    i, j = torch.arange(n)[:, None], torch.arange(n)[None, :]
    if c.family == "relb":
        s = s * c.scale
        s[:, :, :n] += dat.table.double()[:, (dat.m - 1) + j - i]
    elif c.family == "disent":
        idx = dat.col[(dat.m - 1) + i - j]                                               # [n, n] column of (i, j)
        cc = torch.gather(dat.c2p[:, r0:r0 + n].double(), 2, idx.expand(c.hq, n, n))
        pt = torch.gather(dat.p2c[:, r0:r0 + n].double(), 2, idx.t().expand(c.hq, n, n)).transpose(1, 2)
        s[:, :, :n] += cc + pt
        s = s * c.scale
    else:
        s = s * c.scale
    mask = torch.cat([_mask(c, n, nk), torch.zeros(n, len(extra), dtype=torch.bool)], 1)
    return s, mask, v


def drop_mask(c, si):
    """[hq, n, n] float64 multiplier of the probabilities (None without dropout), helpers.attn_dropout_scale with the slab of
    the layout: (sequence * heads + head) * l padded, head * total_rows + first row packed"""
    if not c.p:
        return None
    r0, n, nk = c.seqs[si]
    slab = (lambda hi: hi * c.rows + r0) if c.layout == "packed" else (lambda hi: (si * c.hq + hi) * c.l)
    return torch.stack([attn_dropout_scale(SEED, slab(hi), n, n, c.p) for hi in range(c.hq)])


def seq_trace(c, dat, si):
    s, mask, _ = seq_scores(c, dat, si)
    return softmax_trace((s * LOG2E).masked_fill(~mask, -INF), c.kt)


_DATA = {}


def inputs(c):
    """q, go [rows, hq d], k, v [rows, hkv d] (+ the tables) as float32 holding values of the case's dtype, on the host.  The
    deferred spikes are sized with the trace of the data that holds every other spike."""
    if c.id in _DATA:
        return _DATA[c.id]
    g = torch.Generator().manual_seed(zlib.crc32(c.id.encode()))
    dat = Data()
    rows, d = c.rows, c.d
    dat.q, dat.go = torch.randn(rows, c.hq * d, generator=g), torch.randn(rows, c.hq * d, generator=g)
    dat.k, dat.v = torch.randn(rows, c.hkv * d, generator=g), torch.randn(rows, c.hkv * d, generator=g)
    rnd = lambda t: t.to(c.dtype).float()
    dat.q = rnd(dat.q)                                             # the spikes are multiples of the stored q
    dat.m = max(n for _, n, _ in c.seqs)
    if c.family == "relb":
        dat.table = torch.randn(c.hq, 2 * dat.m - 1, generator=g)  # the unit-variance score term of the family's own test
    if c.family == "disent":
        cols = DB._columns("v3", dat.m)
        dat.col, width = cols.col.long(), cols.width
        dat.c2p = torch.randn(c.hq, rows, width, generator=g) * DB.TABLE_STD
        dat.p2c = torch.randn(c.hq, rows, width, generator=g) * DB.TABLE_STD
    big = c.dtype == f32
    plan = _plan(c)
    row = lambda s, key=False: c.seqs[s["kseq" if key else "seq"]][0] + s["j" if key else "i"]
    for s in plan:
        if s["kind"] in ("jump", "late"):
            n = s.get("n", 0)
            _align(c, dat, row(s), row(s, True), (6.0, 9.0, 12.0)[n] if big else (10.0, 12.0, 20.0)[n], big)
        elif s["kind"] == "masked":
            # 30 natural units (relb "table": above the entry of 40 / 12 that the aligned query also meets)
            _align(c, dat, row(s), row(s, True), 30.0 + ((40.0 if big else 12.0) if (c.kind, c.family) == ("table", "relb") else 0.0), False)
            if s["vbig"]:
                dat.v[row(s, True)] = VBIG
        elif s["kind"] == "table":
            dat.table[0, dat.m - 1 + s["rel"]] = 40.0 if big else 12.0
        elif s["kind"] in ("c2p", "p2c"):
            size = (40.0 if big else 12.0) / c.scale
            colj = int(dat.col[dat.m - 1 + s["i"] - s["j"]])
            if s["kind"] == "c2p":
                dat.c2p[0, row(s), colj] = size
            else:
                dat.p2c[1 % c.hq, row(s, True), colj] = size
    dat.k = rnd(dat.k)
    # deferred spikes: 4.5 log2 units above the reference the wave keeps before the key's tile, then 8.5 above the same reference
    for step, up in ((1, 4.5), (2, 8.5)):
        for s in (s for s in plan if s["kind"] == "defer" and s["step"] == step):
            tr = seq_trace(c, dat, s["seq"])
            first = next(x for x in plan if x["kind"] == "defer" and x["step"] == 1)
            t1 = first["j"] // c.kt
            sc, mask, _ = seq_scores(c, dat, s["seq"])
            sc = (sc * LOG2E).masked_fill(~mask, -INF)
            for kh in range(c.hkv):
                h = _qhead(c, kh)
                # the kept reference before tile t1: the row max over the tiles up to the wave's last rescale before t1
                last = max(t for t in range(t1) if bool(tr.rescale[h, s["i"] // 32, t]))
                kept = float(sc[h, s["i"], :(last + 1) * c.kt].max())
                qv = dat.q[row(s), h * d:(h + 1) * d]
                base = 0.0
                if c.family == "relb":
                    base = float(dat.table[h, dat.m - 1 + s["j"] - s["i"]])
                elif c.family == "disent":
                    colj = int(dat.col[dat.m - 1 + s["i"] - s["j"]])
                    base = float(dat.c2p[h, row(s), colj] + dat.p2c[h, row(s, True), colj]) * c.scale
                target = (kept + up) / LOG2E - base                # natural units q . k * scale must contribute
                dat.k[row(s, True), kh * d:(kh + 1) * d] = target / (c.scale * float(qv.double().pow(2).sum())) * qv
            dat.k = rnd(dat.k)
    dat.v, dat.go = rnd(dat.v), rnd(dat.go)
    _DATA[c.id] = dat
    return dat


# ------------------------------------------------------------------------------------------------ 4. float64 results
def dense_out(c, dat, weights=None, unmask=None):
    """out [rows, hq d] in float64 from this file's own scores: softmax under the case's mask (``weights(si)`` replaces it;
    ``unmask`` {sequence: absolute key rows}: keys every query of that sequence sees as if no mask hid them, rows of another
    sequence included), dropout applied."""
    out = torch.zeros(c.rows, c.hq * c.d, dtype=torch.float64)
    for si, (r0, n, nk) in enumerate(c.seqs):
        if n == 0:
            continue
        asked = (unmask or {}).get(si, [])
        foreign = [r for r in asked if not r0 <= r < r0 + n]
        s, mask, v = seq_scores(c, dat, si, foreign)
        if weights is not None:
            w = weights(si)
        else:
            mask = mask.clone()
            for r in (r for r in asked if r0 <= r < r0 + n):
                mask[:, r - r0] = True
            mask[:, n:] = True                                     # the foreign keys asked for
            w = torch.softmax(s.masked_fill(~mask, -INF), -1).nan_to_num(0.0)
        drop = drop_mask(c, si)
        if drop is not None:
            w = w.clone()
            w[:, :, :n] = w[:, :, :n] * drop
        out[r0:r0 + n] = (w @ v).transpose(0, 1).reshape(n, -1)
    return out


def lse_reference(c, dat):
    """[rows, hq] float64, -inf for a row without a visible key; and the bf16 bound of tests/test_gpu_ring_blocks.py per row:
    2^-9 scale max_j sum_d |q_id| |k_jd| + 1e-4"""
    lse, bound = torch.zeros(c.rows, c.hq, dtype=torch.float64), torch.zeros(c.rows, c.hq, dtype=torch.float64)
    rep = c.hq // c.hkv
    for si, (r0, n, nk) in enumerate(c.seqs):
        if n == 0:
            continue
        s, mask, _ = seq_scores(c, dat, si)
        lse[r0:r0 + n] = torch.logsumexp(s.masked_fill(~mask, -INF), -1).t()
        qa = dat.q[r0:r0 + n].double().abs().view(n, c.hq, c.d).transpose(0, 1)
        ka = dat.k[r0:r0 + n].double().abs().view(n, c.hkv, c.d).transpose(0, 1).repeat_interleave(rep, 0)
        reach = (qa @ ka.transpose(1, 2)).masked_fill(~mask, 0.0).amax(-1)
        bound[r0:r0 + n] = (2.0 ** -9 * c.scale * reach + LSE_ABS).t()
    return lse, bound


def _fused(c, dat):
    return torch.cat([dat.q, dat.k, dat.v], -1)


_REFS = {}


def reference(c):
    """The family's own float64 reference (imported from its test file), on the host, once per case: dict of out, dq, dk, dv
    [rows, .] and the table gradients of relb:: (dtab) / disent:: (dc, dpt)."""
    if c.id in _REFS:
        return _REFS[c.id]
    dat = inputs(c)
    names = ("out", "dq", "dk", "dv")
    ref = {}
    padded = c.layout == "padded"
    b = len(c.lens)
    kv_len = torch.tensor(c.lens, dtype=torch.int32)
    if c.family == "dense":
        mc = AM.Case(id=c.id, dtype=c.dtype, d=c.d, b=b, h=c.hq, lq=c.l if padded else c.rows, lk=c.l if padded else c.rows,
                     mode="kvlen" if padded else "packed", fwd=c.fwd, bwd=c.bwd, lens=c.lens, p=c.p)
        shape = (b, c.l, -1) if padded else (1, c.rows, -1)
        res, _ = D32._reference(mc, torch.device("cpu"), *(t.view(*shape) for t in (dat.q, dat.k, dat.v, dat.go)), SEED)
        ref = {n_: t.reshape(c.rows, -1) for n_, t in zip(names, res)}
    elif c.family == "grouped":
        if c.d == 256:
            res = GW._reference(dat.q, dat.k, dat.v, dat.go, c.seqs, c.hq, c.hkv, c.scale, c.causal)
            ref = dict(zip(names, res))
        else:
            qkv = _fused(c, dat)

            def one(x, g_, kv):
                if c.d == 128 and c.causal:
                    nq, nk_ = c.hq * 128, c.hkv * 128
                    return _causal_reference(x[..., :nq], x[..., nq:nq + nk_], x[..., nq + nk_:], g_, kv, c.hq, c.hkv, c.scale)
                if c.causal:
                    return G64._reference(x, g_, kv, c.hq, c.hkv)
                return BD._reference(x, g_, kv, c.hq, c.hkv, c.d)
            if padded:
                res = one(qkv.view(b, c.l, -1), dat.go.view(b, c.l, -1), kv_len)
                ref = {n_: t.reshape(c.rows, -1) for n_, t in zip(names, res)}
            else:
                parts = [one(qkv[None, r0:r0 + n], dat.go[None, r0:r0 + n], torch.tensor([n])) for r0, n, _ in c.seqs]
                ref = {n_: torch.cat([p_[i][0] for p_ in parts]) for i, n_ in enumerate(names)}
    else:
        qkv = _fused(c, dat)
        parts, tabs = [], []
        for si, (r0, n, nk) in enumerate(c.seqs):
            drop = drop_mask(c, si)
            drop = None if drop is None else drop[:, :, :nk]
            if c.family == "window":
                res = MB._band_reference(qkv[r0:r0 + n], dat.go[r0:r0 + n], nk, c.window)
            elif c.family == "relb":
                res = MP._dense(qkv[r0:r0 + n], dat.go[r0:r0 + n], dat.table, nk, drop)
                tabs.append(res[4:5])
            else:
                res = DB._dense(c.hq, qkv[r0:r0 + n], dat.go[r0:r0 + n], dat.c2p[:, r0:r0 + n], dat.p2c[:, r0:r0 + n], dat.col, nk, drop)
                tabs.append(res[4:6])
            parts.append(res[:4])
        ref = {n_: torch.cat([p_[i] for p_ in parts]) for i, n_ in enumerate(names)}
        if c.family == "relb":
            ref["dtab"] = sum(t[0] for t in tabs)
        if c.family == "disent":
            ref["dc"], ref["dpt"] = torch.cat([t[0] for t in tabs], 1), torch.cat([t[1] for t in tabs], 1)
    ref["lse"], ref["lse_bound"] = lse_reference(c, dat)
    _REFS[c.id] = ref
    return ref


def family_budget(c, dtype, name):
    """(max rel, l2 rel) of ``name`` from the family's own test file"""
    if c.d >= 256:
        return WD._budget(dtype, name in ("dq", "dk"))              # test_gpu_attention_wide / test_gpu_gqa_wide_kernels
    if c.family == "grouped":
        return _decoder_budget(dtype, name)                         # test_gpu_gqa_kernels / test_gpu_bidir_kernels
    return AM._budget(dtype, name)                                  # the matrix, d32, window, relb, disent


def _floor(c, dat):
    """The dense formula in float64 with the roundings the bf16 kernels apply (attn_stream.hpp): the forward feeds bf16(P [* D])
    to the P V product and stores a bf16 output (delta reads out + out_lo, i.e. the unrounded one); the dQ chain recomputes the
    scores from Q' = bf16(Q scale log2 e) and the dK / dV chain from K' = bf16(K scale log2 e), both against the forward's lse;
    bf16(dS) and bf16(P [* D]) enter the second products; the results are stored in bf16."""
    rb = lambda t: t.bfloat16().double()
    res = {n_: torch.zeros_like(t, dtype=torch.float64) for n_, t in (("out", dat.q), ("dq", dat.q), ("dk", dat.k), ("dv", dat.v))}
    rep, d, sl2 = c.hq // c.hkv, c.d, c.scale * LOG2E
    for si, (r0, n, nk) in enumerate(c.seqs):
        if n == 0:
            continue
        s, mask, v = seq_scores(c, dat, si)
        p = torch.softmax(s.masked_fill(~mask, -INF), -1).nan_to_num(0.0)
        drop = drop_mask(c, si)
        pd = p if drop is None else p * drop
        g = dat.go[r0:r0 + n].double().view(n, c.hq, d).transpose(0, 1)
        q = dat.q[r0:r0 + n].double().view(n, c.hq, d).transpose(0, 1)
        k = dat.k[r0:r0 + n].double().view(n, c.hkv, d).transpose(0, 1).repeat_interleave(rep, 0)
        o = rb(pd) @ v
        added = s * LOG2E - (q @ k.transpose(1, 2)) * sl2                              # the bias / disentangled terms, log2 domain
        lse2 = torch.logsumexp(s.masked_fill(~mask, -INF), -1, keepdim=True) * LOG2E
        again = lambda s2: torch.exp2((s2 + added - lse2).masked_fill(~mask, -INF)).nan_to_num(0.0)
        p_q, p_k = again(rb(q * sl2) @ k.transpose(1, 2)), again(q @ rb(k * sl2).transpose(1, 2))
        dp = g @ v.transpose(1, 2)
        dpd = (dp if drop is None else dp * drop) - (g * o).sum(-1, keepdim=True)
        back = lambda t: t.transpose(0, 1).reshape(n, -1)
        group = lambda t: t.view(c.hkv, rep, n, d).sum(1)
        res["out"][r0:r0 + n], res["dq"][r0:r0 + n] = back(rb(o)), back(rb(rb(p_q * dpd) @ k * c.scale))
        res["dk"][r0:r0 + n] = back(rb(group(rb(p_k * dpd).transpose(1, 2) @ q * c.scale)))
        res["dv"][r0:r0 + n] = back(rb(group(rb(p_k if drop is None else p_k * drop).transpose(1, 2) @ g)))
    return res


# ------------------------------------------------------------------------------------------------ 5. the kernels
_ATTN_PREFIXES = ("attn_", "d128::", "d32::", "d32s::", "wide::", "gqaw::", "gqa::", "gqas::", "causal128::", "bidir::", "mbert::",
                  "relb::", "disent::")


def _attn(names):
    return {n for n in names if n.startswith(_ATTN_PREFIXES)}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def run(c, dev, dtype=None, zero_rows=()):
    """One forward + backward of the case through the family's lowest public call -> dict of out, dq, dk, dv [rows, .] in the
    kernels' dtype, lse [rows, hq] fp32, the table gradients, and the attention kernels the two passes launched."""
    from gmlm_amd import ops
    dat = inputs(c)
    dtype = dtype or c.dtype
    padded, b, l, rows = c.layout == "padded", len(c.lens), c.l, c.rows
    k, v = dat.k.clone(), dat.v.clone()
    for r in zero_rows:
        k[r], v[r] = 0.0, 0.0
    up = lambda t: t.to(dev, dtype)
    q, k, v, go = up(dat.q), up(k), up(v), up(dat.go)
    shape = (b, l, -1) if padded else (rows, -1)
    kv_len = torch.tensor(c.lens, dtype=torch.int32, device=dev) if padded else None
    cu = None if padded else torch.tensor([0] + [r0 + n for r0, n, _ in c.seqs], dtype=torch.int32, device=dev)
    max_len = 0 if padded else max(c.lens)
    flat = lambda t: t.reshape(rows, -1)
    lse_rows = lambda t: (t.permute(0, 2, 1).reshape(rows, -1) if padded else t.t()).contiguous()
    r, box = {}, {}
    nq, nk = c.hq * c.d, c.hkv * c.d
    if c.family == "dense" or (c.family == "grouped" and c.d != 256):
        if c.family == "dense" and not padded:
            qkv = torch.cat([q, k, v], -1).requires_grad_(True)
            groups = torch.tensor(ops.pack_sequence_groups(c.lens).tolist(), dtype=torch.int32, device=dev) if c.groups else None
            call = lambda: ops.AttentionQKV.apply(qkv, None, c.hq, c.scale, c.p, SEED, cu, max_len, None, groups)
            lse_at, leaves = 1, None
        else:
            leaves = tuple(t.view(*shape).clone().requires_grad_(True) for t in (q, k, v))
            lse_at = 4
            if c.family == "dense":
                call = lambda: ops.Attention.apply(*leaves, kv_len, c.hq, c.scale, c.p, SEED)
            elif padded:
                fn = ops.causal_attention if c.causal else ops.bidir_gqa_attention
                call = lambda: fn(*leaves, kv_len, c.hq, c.hkv, c.scale, c.d)
            else:
                fn = ops.causal_attention_varlen if c.causal else ops.bidir_gqa_attention_varlen
                groups = torch.tensor(ops.pack_sequence_groups(c.lens).tolist(), dtype=torch.int32, device=dev) if c.groups else None
                call = lambda: fn(*leaves, cu, max_len, c.hq, c.hkv, c.scale, c.d, groups)
        r["fwd_k"] = _attn(kernels_run(lambda: box.setdefault("o", call())))
        out = box["o"]
        r["lse"] = lse_rows(out.grad_fn.saved_tensors[lse_at].clone())
        r["bwd_k"] = _attn(kernels_run(lambda: out.backward(go.view(*shape))))
        grads = (qkv.grad[:, :nq], qkv.grad[:, nq:2 * nq], qkv.grad[:, 2 * nq:]) if leaves is None else tuple(t.grad for t in leaves)
        r.update(out=flat(out.detach()), dq=flat(grads[0]).contiguous(), dk=flat(grads[1]).contiguous(), dv=flat(grads[2]).contiguous())
    elif c.family == "grouped":
        buf = torch.zeros(rows, nq + 2 * nk + GW.PAD, dtype=dtype, device=dev)
        buf[:, :nq], buf[:, nq:nq + nk], buf[:, nq + nk:nq + 2 * nk] = q, k, v
        got = GW._run(buf.view(*shape), go.view(*shape), c.hq, c.hkv, c.causal, kv_len=kv_len, cu=cu, max_len=max_len, kernels=True)
        r["fwd_k"], r["bwd_k"] = (set(s_) for s_ in GW._kernel_sets(dtype, c.causal))      # asserted inside GW._run
        r.update(out=flat(got[0]), lse=lse_rows(got[1]), dq=flat(got[2]), dk=flat(got[3]), dv=flat(got[4]))
    elif c.family == "window":
        qkv = torch.cat([q, k, v], -1).view(*shape)
        out, dqkv, lse = MB._window_run(dev, qkv, go.view(*shape), kv_len, c.window, cu, max_len)    # asserts the kernels and the repeat
        r["fwd_k"], r["bwd_k"] = _fam({f"mbert::window_{k_}_kernel<{TN[dtype]}>" for k_ in ("fwd", "delta", "dq", "dkv")})
        dqkv = flat(dqkv)
        r.update(out=flat(out), lse=lse_rows(lse), dq=dqkv[:, :nq].contiguous(), dk=dqkv[:, nq:2 * nq].contiguous(), dv=dqkv[:, 2 * nq:].contiguous())
    else:
        qkv = torch.cat([q, k, v], -1).view(*shape).requires_grad_(True)
        if c.family == "relb":
            tabs = (dat.table.to(dev).requires_grad_(True),)
            call = lambda: ops.AttentionRelBiasQKV.apply(qkv, tabs[0], kv_len, c.hq, c.scale, c.p, SEED, cu, max_len)
            lse_at = 2
        else:
            tabs = (dat.c2p.to(dev).requires_grad_(True), dat.p2c.to(dev).requires_grad_(True))
            col = dat.col.to(dev, torch.int32)
            call = lambda: ops.AttentionDisentQKV.apply(qkv, tabs[0], tabs[1], col, kv_len, c.hq, c.scale, c.p, SEED, cu, max_len)
            lse_at = 4
        r["fwd_k"] = _attn(kernels_run(lambda: box.setdefault("o", call())))
        out = box["o"]
        r["lse"] = lse_rows(out.grad_fn.saved_tensors[lse_at].clone())
        r["bwd_k"] = _attn(kernels_run(lambda: box.setdefault("g", torch.autograd.grad(out, (qkv,) + tabs, go.view(*shape)))))
        dqkv = flat(box["g"][0])
        r.update(out=flat(out.detach()), dq=dqkv[:, :nq].contiguous(), dk=dqkv[:, nq:2 * nq].contiguous(), dv=dqkv[:, 2 * nq:].contiguous())
        r.update(dict(zip(("dtab",) if c.family == "relb" else ("dc", "dpt"), box["g"][1:])))
    torch.cuda.synchronize()
    return r


QUANTITIES = ("out", "dq", "dk", "dv")
TABLES = ("dtab", "dc", "dpt")


def _measure(got, ref):
    e = got.double().cpu() - ref
    scale = float(ref.abs().max())
    return (float(e.abs().max()) / scale, float(e.norm()) / float(ref.norm())) if scale > 0 else (float(e.abs().max()), 0.0)


def compare(c, dtype, r, ref, floor=None):
    """Per sequence and quantity against the family's budget -> the list of (quantity, sequence, max rel, l2 rel) that miss;
    every figure is printed first.  lse and the fp32 table gradients are asserted here."""
    missed, worst = [], {}
    for name in QUANTITIES:
        assert bool(torch.isfinite(r[name]).all()), name
        lim = family_budget(c, dtype, name)
        for si, (r0, n, nk) in enumerate(c.seqs):
            if n == 0:
                continue
            want = ref[name][r0:r0 + n]
            mx, l2 = _measure(r[name][r0:r0 + n], want)
            if float(want.abs().max()) == 0.0:
                assert mx == 0.0, (name, si)
                continue
            worst[name] = tuple(max(a, b_) for a, b_ in zip(worst.get(name, (0.0, 0.0)), (mx, l2)))
            if mx > lim[0] or l2 > lim[1]:
                if floor is not None:
                    fmx, fl2 = _measure(floor[name][r0:r0 + n], want)
                    print(f"  {name} of sequence {si}: {mx:.2e} / {l2:.2e} against the floor {fmx:.2e} / {fl2:.2e}")
                    if mx <= max(lim[0], 2 * fmx) and l2 <= max(lim[1], 2 * fl2):
                        continue
                missed.append((name, si, mx, l2))
    print("  " + ", ".join(f"{n_} {mx:.2e} / {l2:.2e}" for n_, (mx, l2) in worst.items()) + "  (worst sequence: max|err| / max|ref|, l2 rel)")
    lse, want = r["lse"].double().cpu(), ref["lse"]
    dead = want == -INF
    assert bool((lse[dead] == -INF).all()), "lse of a row without a visible key"
    err = (lse - want).abs().masked_fill(dead, 0.0)
    lim = ref["lse_bound"] if dtype == bf else torch.full_like(want, LSE_ABS)
    print(f"  lse: max|err| = {float(err.max()):.2e} (bound {float(lim.min()):.2e} .. {float(lim.max()):.2e})")
    assert bool((err <= lim).all()), ("lse", float(err.max()), float((err - lim).max()))
    for name in (n_ for n_ in TABLES if n_ in ref):
        got = r[name].double().cpu()
        e = float((got - ref[name]).norm()) / float(ref[name].norm())
        print(f"  {name}: err / |ref| = {e:.2e}")
        worst[name] = (e, e)
        if dtype == f32:
            assert e <= AM._budget(f32, "dq")[1], (name, e)            # the figure of the families' own tests: 1e-5 of the tensor norm
    return missed, worst


def _table_floor(c, dat):
    """bf16 floor of the table gradients, the families' own ``_dense(round_p=True)`` summed over the sequences"""
    qkv = _fused(c, dat)
    acc = None
    for si, (r0, n, nk) in enumerate(c.seqs):
        drop = drop_mask(c, si)
        drop = None if drop is None else drop[:, :, :nk]
        if c.family == "relb":
            res = (MP._dense(qkv[r0:r0 + n], dat.go[r0:r0 + n], dat.table, nk, drop, round_p=True),)
        else:
            res = DB._dense(c.hq, qkv[r0:r0 + n], dat.go[r0:r0 + n], dat.c2p[:, r0:r0 + n], dat.p2c[:, r0:r0 + n], dat.col, nk, drop, round_p=True)
        acc = [list(res)] if acc is None else acc + [list(res)]
    if c.family == "relb":
        return {"dtab": sum(a[0] for a in acc)}
    return {"dc": torch.cat([a[0] for a in acc], 1), "dpt": torch.cat([a[1] for a in acc], 1)}


def _outputs(r):
    return [r[n_] for n_ in QUANTITIES + ("lse",) + tuple(t for t in TABLES if t in r)]


WORST = {}


@pytest.mark.parametrize("c", CASES, ids=[c.id for c in CASES])
def test_spiked_scores_vs_float64(dev, c):
    dat, ref = inputs(c), reference(c)
    r = run(c, dev)
    print(f"\n{c.id}: forward {sorted(r['fwd_k'])}, backward {sorted(r['bwd_k'])}")
    missed, worst = compare(c, c.dtype, r, ref)
    if missed and c.dtype == bf:
        # no wider budget: the fp32 twin must meet its own, and the bf16 figures must be within 2x of the rounding floor
        twin_missed, _ = compare(c, f32, run(c, dev, dtype=f32), ref)
        assert not twin_missed, ("the fp32 twin misses its budget as well", twin_missed)
        missed, _ = compare(c, c.dtype, r, ref, floor=_floor(c, dat))
    assert not missed, missed
    if c.dtype == bf:
        for name, fl in (_table_floor(c, dat).items() if c.family in ("relb", "disent") else ()):
            norm = float(ref[name].norm())
            err, floor = float((r[name].double().cpu() - ref[name]).norm()) / norm, float((fl - ref[name]).norm()) / norm
            print(f"  {name}: err / |ref| = {err:.2e}, bf16 floor = {floor:.2e}")
            assert err <= 2 * floor, (name, err, floor)
    assert r["fwd_k"] == set(c.fwd), (sorted(r["fwd_k"]), sorted(c.fwd))
    assert r["bwd_k"] == set(c.bwd), (sorted(r["bwd_k"]), sorted(c.bwd))
    # masked keys zeroed, K and V: a wave none of whose queries sees them keeps every bit of out, lse and dq; where no query of
    # a sequence sees them, dk / dv keep theirs too, and are exactly 0 at those keys.  First the keys no query at all should see
    # (a; d / e: only their own sequence does), then one by one the keys that the diagonal or the band hides (b, c).
    for hidden in [_unseen_rows(c)] + [[k_] for k_ in _hidden_rows(c)]:
        if not hidden:
            continue
        z = run(c, dev, zero_rows=hidden)
        rows_ok, seq_ok = _unaffected(c, hidden)
        assert int(rows_ok.sum()) >= 32
        for name in ("out", "lse", "dq"):
            assert _same_bits([z[name][rows_ok.to(dev)]], [r[name][rows_ok.to(dev)]]), f"{name} moved when masked keys were zeroed"
        for name in ("dk", "dv"):
            assert _same_bits([z[name][seq_ok.to(dev)]], [r[name][seq_ok.to(dev)]]), f"{name} moved when masked keys were zeroed"
        if bool(seq_ok[hidden].all()):                              # no query sees them
            for name in ("dk", "dv"):
                assert float(r[name][hidden].abs().max()) == 0.0 and float(z[name][hidden].abs().max()) == 0.0, f"{name} of a key no query sees"
            if c.layout == "padded":
                assert all(torch.equal(z[t], r[t]) for t in TABLES if t in r), "a table gradient moved with keys no query sees"
    again = run(c, dev)
    assert _same_bits(_outputs(again), _outputs(r)), "a second identical run differs"
    WORST[c.id] = worst


def test_print_worst_errors_per_family(dev):
    """Not a check: the table that DESIGN.md section 4 records, from the cases that ran before this one."""
    fam = {}
    for cid, worst in WORST.items():
        key = (cid.split("_")[0], _dn(BY_ID[cid].dtype))
        for name, (mx, l2) in worst.items():
            old = fam.setdefault(key, {}).get(name, (0.0, 0.0))
            fam[key][name] = (max(old[0], mx), max(old[1], l2))
    for key, w in sorted(fam.items()):
        print(f"  {key[0]:9s} {key[1]:5s} " + ", ".join(f"{n_} {mx:.1e} / {l2:.1e}" for n_, (mx, l2) in w.items()))
