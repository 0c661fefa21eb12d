"""The segment-reduction ("SpMM") dispatch matrix: every instantiation of seg_reduce_vec_kernel<T, CH, EDGE_W, MODE>,
seg_reduce_combine_kernel<T> and seg_reduce_scalar_kernel<T, EDGE_W> (spmm_kernels.hip) run at least once through
ops._spmm (or the C ABI, where the output rows are padded) against a float64 reference built from the same rounded inputs
the kernels read, with the kernels that really ran read back by name from the profiler.

``CASES`` names, per case, the EXACT set of seg_reduce_* kernels the call launches; ``UNREACHABLE`` lists compiled
instantiations that launch_spmm cannot select (none).  Their union must equal the family's kernels in the built library
(tests/test_spmm_matrix_cpu.py, which also restates launch_spmm's choice and holds every case's shape to the kernel it names).

Segment layout, the same for every case with edges (``_layout``): lengths 0, 1, 2, 3, 4, 5, 7, 8, 9 (the 4-edge main loop of
accumulate_rows with every tail), then thresh - 1, thresh, thresh + 1, 2 thresh, 2 thresh + 1 and 10 thresh with
thresh = 64 (the ``end - beg > sp.thresh`` skip of MODE 0 on both sides, whole and ragged last chunks of MODE 1), short
random segments up to the case's segment count, and an empty last segment (the final rowptr entries are equal).  ``idx`` is
drawn with replacement (repeats) and every segment's first edge points at the segment's own row number (self-reference).

Geometry bands and the line of launch_spmm each one exercises (V = 4 fp32 / 8 bf16 elements per 16-byte chunk):
  * f / V = 1, 2, 63 -> ``ntile = ... f_chunks >= 64 ? 8 : 1`` false: one tile, ``while ((1 << log2_l) < cpt ...)`` gives
    L = 1, 2, 64 (63 chunks: the last lane of the group idles), CH 1;
  * f / V = 64, 512 -> ntile = 8 with cpt = 8 (L = 8) and 64 (L = 64): both ends of CH 1 under column tiling;
  * f / V = 65 -> cpt = 9, ``ntile = cdiv(f_chunks, cpt)`` = 8 and the last tile holds 2 chunks (``nch < chunks_per_tile``);
  * f / V = 513, 1024 / 1025, 1536 / 1537, 2048 -> ``ch = cdiv(cpt, L)`` = 2 / 3 / 4 at both ends of each band, ntile = 8;
  * f / V = 2049 -> ``while (cpt > 256) ntile *= 2``: 16 tiles of 129 chunks, CH 3;
  * f / V = 264 with 2100 segments -> ``grid = min(seg_blocks, cap) * ntile`` with seg_blocks = 525 > cap = 512 at L = 64
    (4 groups per block): the grid-stride loop of MODE 0 runs twice;
  * sources above 24 MiB -> ``src_bytes <= (24ll << 20)`` false, ntile = 1: fp32 f = 768 (192 chunks, CH 3: the kernel of the
    full-size backward), bf16 f = 768 (96 chunks, CH 2), fp32 f = 1024 (256 chunks, CH 4), fp32 f = 1028 (257 chunks: tile
    doubling from ONE tile, two tiles of 129 and 128 chunks, CH 3);
  * ``vec_ok`` false -> the scalar kernel: f % V != 0 (6; 513 = two 512-column tiles, one live column in the second; 1703),
    a source pointer that is not 16-byte aligned (column slice at an odd element offset), ``src_stride % V != 0``; with a split
    plan the scalar path sets ``sp.thresh = 0`` and sums the long segments itself;
  * ``src_stride > f`` (aligned column slice of a wider tensor) and ``out_stride > f`` (padded output rows, C ABI) on the
    vector path.
Within each CH x dtype all four EDGE_W x MODE kernels run: the forward (mean, no edge weights), the backward (sum, edge
weights 1 / count), and the embedding gradient (sum, no edge weights, capacity-sized device plan whose -1 slots take the skip
branches of MODE 1 and of the combine kernel), with host plans (graph.make_split_plan) and device plans
(ops.device_split_plan).

Budgets, per element, derived from the arithmetic and not tuned.  With n the segment length, u = 2^-24 the fp32 unit
roundoff and A = scale * sum_t |w_t x_t| in float64 (scale = 1 / max(n, 1) for the mean, else 1):
  * fp32 output: |got - ref| <= (n + 3) u A.  The n accumulations (an fp32 add, or one FMA whose product is not rounded) are
    n roundings in any order - also when they are split into chunk partials that the combine kernel adds - so the sum is
    within about n u sum|w x| of the exact one; the mean adds the rounding of 1 / n and of the multiply by it (or of one
    division in the combine kernel): n + 2 roundings at most, n + 3 covers the second-order terms.
  * bf16 output: that bound, d, plus one round-to-nearest-even store of the fp32 value v: half a bf16 ulp of v.  bf16 keeps 8
    significant bits, so half an ulp in the binade [2^e, 2^(e+1)) is 2^(e-8): between 2^-9 |v| (top of the binade) and
    2^-8 |v| (bottom).  A flat 2^-9 |ref| is therefore NOT a bound of a correctly rounded store - 1 + 2^-8 lies 2^-8 from both
    neighbours - and fp32 arithmetic emulated on the host with one rounding misses it on a fifth of the elements at up to
    1.99 x; the store is budgeted at what it is, half an ulp, which equals 2^-9 |v| only at the top of a binade.  With
    |v| <= |ref| + d and the spacing monotone: |got - ref| <= d + 2^(floor(log2(|ref| + d)) - 8).
An empty segment has A = 0 and must be exactly zero.  The output is pre-filled with NaN, so an element that no kernel wrote
fails.  The exactness cases (integer data in [-8, 8], sum, no edge weights) allow nothing: every partial sum is an integer
below 2^24, so the fp32 result is the float64 sum bit for bit and the bf16 result is that sum rounded once; a dropped or
double-counted edge cannot hide there."""
import zlib
from dataclasses import dataclass

import pytest
import torch

from helpers import kernels_run

pytestmark = pytest.mark.gpu

BF, F32 = "unsigned short", "float"          # bf16 is an unsigned short in the kernels' template ids
bf, f32 = torch.bfloat16, torch.float32
THRESH = 64
U = 2.0 ** -24
_HEAD = (0, 1, 2, 3, 4, 5, 7, 8, 9, THRESH - 1, THRESH, THRESH + 1, 2 * THRESH, 2 * THRESH + 1, 10 * THRESH)


def _b(v):
    return "true" if v else "false"


def _tn(dtype):
    return BF if dtype == bf else F32


def vec(t, ch, edge_w, mode):
    return f"seg_reduce_vec_kernel<{t}, {ch}, {_b(edge_w)}, {mode}>"


def combine(t):
    return f"seg_reduce_combine_kernel<{t}>"


def scalar(t, edge_w):
    return f"seg_reduce_scalar_kernel<{t}, {_b(edge_w)}>"


def _is_spmm_family(name):
    """The kernels the CPU guard holds to CASES / UNREACHABLE."""
    return name.startswith("seg_reduce_")


@dataclass(frozen=True)
class Case:
    id: str
    dtype: torch.dtype
    f: int
    path: str                  # "vec", "scalar" or "none" (no launch)
    kernels: frozenset         # the seg_reduce_* kernels the call launches
    ch: int = 0                # vector path: 16-byte chunks per lane (the CH of the kernels named)
    ntile: int = 0             # vector path: column tiles
    lanes: int = 0             # vector path: lanes per (segment, tile) group, L
    mean: bool = False
    edge_w: bool = False
    plan: str = ""             # "", "host" (graph.make_split_plan) or "device" (ops.device_split_plan)
    nseg: int = 120
    src_rows: int = 211
    layout: str = "contig"     # "contig"; src = wide[:, off:off + f]: "slice" (off = 2 V), "odd" (off = 1); "stride" (width f + 1)
    out_pad: int = 0           # extra columns per output row (out_stride = f + out_pad, through the C ABI)
    ints: bool = False         # integer data in [-8, 8]: the result must be exact
    twice: bool = False        # launched twice, bit-identical
    edges: bool = True         # False: every segment empty, no idx


def _kernels(t, path, ch, edge_w, split):
    if path == "none":
        return frozenset()
    if path == "scalar":
        return frozenset({scalar(t, edge_w)})
    k = {vec(t, ch, edge_w, 0)}
    if split:
        k |= {vec(t, ch, edge_w, 1), combine(t)}
    return frozenset(k)


# the three uses of the kernel: (mean, edge weights)
_FWD, _BWD, _EMB = (True, False), (False, True), (False, False)


def _mk(tag, dtype, f, path, use, plan="", ch=0, ntile=0, lanes=0, **kw):
    mean, edge_w = use
    name = f"{'bf16' if dtype == bf else 'f32'}_f{f}_{tag}_" + {_FWD: "fwd", _BWD: "bwd", _EMB: "emb"}[use] + (f"_{plan}" if plan else "")
    split = bool(plan) and path == "vec"
    return Case(id=name, dtype=dtype, f=f, path=path, kernels=_kernels(_tn(dtype), path, ch, edge_w, split), ch=ch, ntile=ntile,
                lanes=lanes, mean=mean, edge_w=edge_w, plan=plan, **kw)


# (tag, fp32 width, CH, ntile, L, [(use, plan), ...]); the bf16 width is twice the fp32 one (same chunk count)
_FULL_LO = [(_FWD, ""), (_BWD, "host"), (_EMB, "device")]
_FULL_HI = [(_FWD, "device"), (_BWD, "")]
_VEC = [
    ("c1_t1_L1", 4, 1, 1, 1, [(_FWD, "")]),
    ("c1_t1_L2", 8, 1, 1, 2, [(_BWD, "host")]),
    ("c1_t1_L64", 252, 1, 1, 64, _FULL_HI),
    ("c1_t8_L8", 256, 1, 8, 8, _FULL_LO),
    ("c1_t8_L64", 2048, 1, 8, 64, _FULL_HI),
    ("c1_ragged", 260, 1, 8, 16, [(_FWD, "device"), (_BWD, "host")]),
    ("c2_lo", 2052, 2, 8, 64, _FULL_LO),
    ("c2_hi", 4096, 2, 8, 64, _FULL_HI),
    ("c3_lo", 4100, 3, 8, 64, _FULL_LO),
    ("c3_hi", 6144, 3, 8, 64, _FULL_HI),
    ("c4_lo", 6148, 4, 8, 64, _FULL_LO),
    ("c4_hi", 8192, 4, 8, 64, _FULL_HI),
    ("t16", 8196, 3, 16, 64, [(_FWD, "device"), (_BWD, "host")]),
]


def _vec_cases():
    out = []
    for dtype, mul in ((f32, 1), (bf, 2)):
        for tag, f, ch, ntile, lanes, uses in _VEC:
            for use, plan in uses:
                # the ragged-tile backward is the determinism case: chunk partials, combine and a partial last tile
                out.append(_mk(tag, dtype, f * mul, "vec", use, plan, ch, ntile, lanes, twice=(tag == "c1_ragged" and use == _BWD)))
        # 525 blocks of 4 segments against a cap of 512
        out.append(_mk("gridcap", dtype, 1056 * mul, "vec", _FWD, "device", 1, 8, 64, nseg=2100))
        # src_stride > f and out_stride > f on the vector path
        out.append(_mk("c1_srcslice", dtype, 256 * mul, "vec", _BWD, "host", 1, 8, 8, layout="slice"))
        out.append(_mk("c1_outpad", dtype, 256 * mul, "vec", _FWD, "device", 1, 8, 8, out_pad=4 * mul))
        # exactness, MODE 0 alone (the long segments too) and MODE 0 + MODE 1 + combine
        out.append(_mk("exact_c1", dtype, 260 * mul, "vec", _EMB, "", 1, 8, 16, ints=True))
        out.append(_mk("exact_c3", dtype, 4100 * mul, "vec", _EMB, "host", 3, 8, 64, ints=True))
    # more than 24 MiB of source: one tile whatever the width
    out.append(_mk("big_c3", f32, 768, "vec", _BWD, "host", 3, 1, 64, nseg=300, src_rows=8200))
    out.append(_mk("big_c2", bf, 768, "vec", _BWD, "host", 2, 1, 64, nseg=300, src_rows=16400))
    out.append(_mk("big_c4", f32, 1024, "vec", _FWD, "device", 4, 1, 64, nseg=300, src_rows=6200))
    out.append(_mk("big_t2", f32, 1028, "vec", _EMB, "device", 3, 2, 64, nseg=300, src_rows=6200))
    # no edges at all: zeros from MODE 0; no segments: no launch
    out.append(_mk("noedges", f32, 256, "vec", _FWD, "", 1, 8, 8, edges=False))
    out.append(_mk("noedges", bf, 512, "vec", _EMB, "", 1, 8, 8, edges=False))
    out.append(_mk("nosegments", f32, 256, "none", _FWD, "", nseg=0))
    out.append(_mk("nosegments", bf, 6, "none", _EMB, "", nseg=0))
    return out


def _scalar_cases():
    out = []
    for dtype, mul in ((f32, 1), (bf, 2)):
        out.append(_mk("scalar", dtype, 6, "scalar", _BWD))
        out.append(_mk("scalar", dtype, 513, "scalar", _FWD))
        out.append(_mk("scalar", dtype, 1703, "scalar", _BWD))
        out.append(_mk("scalar", dtype, 1703, "scalar", _EMB, ints=True))
        out.append(_mk("scalar_oddslice", dtype, 64 * mul, "scalar", _FWD, layout="odd"))
        out.append(_mk("scalar_oddstride", dtype, 64 * mul, "scalar", _BWD, layout="stride"))
        # a split plan with long segments handed to the scalar path: it must sum them itself
        out.append(_mk("scalar_plan", dtype, 6, "scalar", _FWD, "host"))
        out.append(_mk("scalar_plan", dtype, 6, "scalar", _BWD, "device"))
    return out


CASES = _vec_cases() + _scalar_cases()
UNREACHABLE = {}


# ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _vec_width(dtype):
    return 8 if dtype == bf else 4


def _layout(c, g):
    """rowptr (int32 [nseg + 1]), idx (int32 [E]) and the segment lengths (int64 [nseg]) of a case, on the CPU."""
    if not c.edges or c.nseg == 0:
        lens = torch.zeros(c.nseg, dtype=torch.int64)
    else:
        pad = torch.randint(0, 7, (c.nseg - len(_HEAD) - 1,), generator=g)
        lens = torch.cat([torch.tensor(_HEAD), pad, torch.zeros(1, dtype=torch.int64)])
    rowptr = torch.zeros(c.nseg + 1, dtype=torch.int64)
    rowptr[1:] = torch.cumsum(lens, 0)
    e = int(rowptr[-1])
    idx = torch.randint(0, c.src_rows, (e,), generator=g)
    seg = torch.arange(c.nseg)
    first = rowptr[:-1]
    has1 = lens >= 1
    idx[first[has1]] = seg[has1] % c.src_rows                       # self-reference
    has2 = (lens >= 2) & (seg % 3 == 0)
    idx[first[has2] + 1] = idx[first[has2]]                         # an immediate repeat
    return rowptr.to(torch.int32), idx.to(torch.int32), lens


def _source(c, g, dev):
    """The source operand as the case lays it out: [src_rows, f] view, contiguous or a column slice of a wider tensor."""
    v = _vec_width(c.dtype)
    off, width = {"contig": (0, c.f), "slice": (2 * v, c.f + 3 * v), "odd": (1, c.f + v), "stride": (0, c.f + 1)}[c.layout]
    if c.ints:
        wide = torch.randint(-8, 9, (c.src_rows, width), generator=g).to(c.dtype)
    else:
        wide = torch.randn(c.src_rows, width, generator=g).to(c.dtype)
    src = wide.to(dev)[:, off:off + c.f]
    assert src.stride(0) == width and src.shape == (c.src_rows, c.f)
    return src


def _plan(c, rowptr, num_items):
    from gmlm_amd import graph, ops
    if c.plan == "host":
        plan = graph.make_split_plan(rowptr, THRESH)
        assert plan is not None and plan.n_long == 4 and plan.n_chunks == 2 + 2 + 3 + 10
        return plan
    if c.plan == "device":
        plan = ops.device_split_plan(rowptr, num_items, THRESH)
        assert plan.n_long > 4 and plan.n_chunks > 17                # capacity-sized: -1 slots behind the real entries
        return plan
    return None


def _launch(c, src, rowptr, idx, edge_w, out, plan):
    """ops._spmm, or the same C call with out_stride = out.stride(0) where the output rows are padded."""
    from gmlm_amd import ops
    from gmlm_amd._lib import check, lib
    if not c.out_pad:
        assert out.stride(0) == c.f
        return ops._spmm(src, rowptr, idx, edge_w, c.mean, c.nseg, c.f, out, plan)
    p = ops._ptr
    if plan is not None and plan.n_long > 0:
        partial = torch.empty(plan.n_chunks, c.f, dtype=torch.float32, device=src.device)
        extra = (plan.thresh, p(plan.long_seg), p(plan.chunk_ptr), p(plan.chunk_owner), plan.n_long, plan.n_chunks, p(partial))
    else:
        extra = (0, None, None, None, 0, 0, None)
    check(lib().gmlm_rgcn_mean_spmm(p(src), src.shape[0], src.stride(0), p(rowptr), p(idx), p(edge_w), 1 if c.mean else 0, c.nseg,
                                    c.f, p(out), out.stride(0), ops._dt(src), *extra, ops._stream()), "gmlm_rgcn_mean_spmm")


def _reference(c, src, idx, edge_w, lens, dev):
    """float64 out[s] = scale_s * sum_t w_t src[idx[t]] and the magnitude A = scale_s * sum_t |w_t src[idx[t]]| from the rounded
    inputs; [nseg, f] each."""
    seg = torch.repeat_interleave(torch.arange(c.nseg, device=dev), lens.to(dev))
    j = idx.long()
    ref = torch.zeros(c.nseg, c.f, dtype=torch.float64, device=dev)
    mag = torch.zeros_like(ref)
    step = max(1, (1 << 25) // c.f)                                   # edges per pass: 256 MiB of float64 rows at most
    for e0 in range(0, j.numel(), step):
        rows = src[j[e0:e0 + step]].double()
        if edge_w is not None:
            rows = rows * edge_w[j[e0:e0 + step]].double()[:, None]
        ref.index_add_(0, seg[e0:e0 + step], rows)
        mag.index_add_(0, seg[e0:e0 + step], rows.abs())
    if c.mean:
        scale = 1.0 / lens.to(dev).clamp_min(1).double()[:, None]
        ref, mag = ref * scale, mag * scale
    return ref, mag


def _budget_check(c, got, ref, mag, lens):
    bound = (lens.to(ref.device).double()[:, None] + 3) * U * mag
    if c.dtype == bf:
        v = ref.abs() + bound                                         # the fp32 value that is rounded is no larger than this
        half_ulp = torch.exp2(torch.floor(torch.log2(v.clamp_min(2.0 ** -126))) - 8)
        bound = bound + torch.where(v > 0, half_ulp, torch.zeros_like(v))
    err = (got.double() - ref).abs()
    ok = err <= bound                                                 # False for NaN: an element nobody wrote
    pos = bound > 0
    worst = float((err[pos] / bound[pos]).max()) if bool(pos.any()) else 0.0
    nbad = int((~ok).sum())
    print(f"  {c.id}: max err / bound = {worst:.3f}, {nbad} of {ok.numel()} outside")
    assert nbad == 0, (c.id, worst, nbad)


@pytest.mark.parametrize("c", CASES, ids=[c.id for c in CASES])
def test_spmm_instantiation_vs_fp64(dev, c):
    g = torch.Generator().manual_seed(zlib.crc32(c.id.encode()))
    rowptr_c, idx_c, lens = _layout(c, g)
    src = _source(c, g, dev)
    rowptr, idx = rowptr_c.to(dev), idx_c.to(dev)
    edge_w = None
    if c.edge_w:                                                      # 1 / count of the source row's own segment, as inv_cnt
        edge_w = (1.0 / torch.randint(1, 10, (c.src_rows,), generator=g).float()).to(dev)
    plan = _plan(c, rowptr, idx.numel()) if c.plan else None
    sentinel = -77.0
    wide_out = torch.full((c.nseg, c.f + c.out_pad), float("nan"), dtype=c.dtype, device=dev)
    if c.out_pad:
        wide_out[:, c.f:] = sentinel
    out = wide_out[:, :c.f]

    def run():
        _launch(c, src, rowptr, idx, edge_w, out, plan)
        if c.path == "none":
            torch.zeros(1, device=dev)                                # a device kernel for the profiler to see; not the project's

    ran = {k for k in kernels_run(run) if _is_spmm_family(k)}
    print(f"\n{c.id}: {sorted(ran)}")
    assert ran == set(c.kernels), (sorted(ran), sorted(c.kernels))
    if c.nseg == 0:
        return
    if c.out_pad:
        assert bool((wide_out[:, c.f:] == sentinel).all()), "the padding columns of the output rows were written"

    ref, mag = _reference(c, src, idx, edge_w, lens, dev)
    if not c.edges:
        assert float(ref.abs().max()) == 0.0
        assert bool((out == 0).all())
    _budget_check(c, out, ref, mag, lens)
    if c.ints:
        assert not c.mean and not c.edge_w
        assert float(ref.abs().max()) < 2 ** 24
        assert torch.equal(out, ref.float().to(c.dtype)), "an integer sum is not exact"
    if c.twice:
        again = torch.full_like(out, float("nan"))
        _launch(c, src, rowptr, idx, edge_w, again, plan)
        assert torch.equal(out, again), "two launches differ"
