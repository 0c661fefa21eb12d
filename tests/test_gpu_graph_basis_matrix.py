"""The graph-build kernels (graph_kernels.hip) and the basis-composition kernels (basis_kernels.hip) at their loop edges: every
case names the EXACT set of ``gmlm::`` kernels each of its calls launches (read back by name from the profiler; rocPRIM's sort
kernels are outside the namespace and are not listed), integer outputs are compared bit for bit with numpy, fp32 outputs with a
float64 reference under derived budgets.  The union of the kernels named here must equal the two families' kernels in the
built library (tests/test_graph_basis_matrix_cpu.py, which also restates grid_cap / basis_blocks / the radix ``end_bit`` and
holds every claim below about trips, groups and blocks to the case's numbers).

Part A - graph build (``GRAPH_CASES``).  The family is the nine kernels of graph_kernels.hip (gather_kernel in two
instantiations) and zero_words_kernel (common.hpp), which the entry points use in place of a memset.  Every graph kernel is a
grid-stride loop ``for (i = block * 256 + thread; i < n; i += gridDim.x * 256)`` launched with ``grid_cap(cdiv(n, 256))``
blocks, capped at 2048 (rel_hist_kernel: 1024).
  * second_trip: E = 2048 * 256 + 300 edges, three active relations, N = 180,000 (N * R_a = 540,000 > 524,288), a float32
    degree over 524,288 + 5 nodes: the ``i += gridDim.x * blockDim.x`` step of every graph kernel is taken (rel_hist_kernel:
    twice), and split_plan_kernel walks 528 segments per thread.
  * hot_node: every edge has the same source and the same target: one address for the atomicAdd of degree_kernel (the degree
    is exactly E), one segment holds every edge, ``perm`` is arange(E) (the sort is stable).
  * bucket_boundaries: node k has out-degree k, k = 0 .. 12: both sides of every ``d <= 2 / d <= 5 / d <= 10`` of
    edge_bucket_kernel, through edge_types_from_degree and through build_rel_csr(src_degree_for_types=...), whose degree vector
    is NOT the local histogram (it is reversed), so that the supplied vector is what must have been read.
  * hist_r64 / hist_r1: ``num_relations`` = 64 (every entry of rel_hist_kernel's ``local[64]``, ``threadIdx.x < r`` for the
    whole first wave) and 1.  hist_rejects: relation ids -1 and 64 are not counted (``t >= 0 && t < r``), build_rel_csr raises
    on the count and make_keys_kernel - whose ``remap[rel[i]]`` is unguarded - is never launched.
  * end_bit: ``while ((1ll << end_bit) < num_segments) ++end_bit`` on both sides of 2, 2^10 and 2^16, and num_segments = 1;
    the ids contain 0 and num_segments - 1 and nothing near them, so that thread 0 and thread e of rowptr_fill_kernel fill
    thousands of entries each (``for (s = lo + 1; s <= hi; ++s)``).
  * null_keys: gmlm_segment_sort with ``keys == NULL`` (``ukeys = ws + 2 * slot``) gives the perm and rowptr of the call with
    a keys buffer; a workspace one byte short is refused.
  * flagged_ids: targets -1 and num_nodes, a relation whose remap entry is -1, sources -1 and num_src: ``*bad`` is set, the
    keys are clamped to segment 0 (never out of range), edge_bucket_kernel reads degree 0 for the foreign sources.
  * no_edges: E = 0 with N = 1 and N = 1000: only the zero fills and inv_count_kernel run.
  * split_plan: split_plan_kernel with thresh = 64 at ``per = (nseg + 1023) / 1024`` = 1 (nseg = 1, 1023, 1024: 1023, 1 and
    0 threads without a segment), 2 (1025: the last owning thread has one segment) and 196 (200,000), over the length layouts
    of ``split_layout``; a refused capacity.
Raw-ABI cases (null_keys, flagged_ids) put ``GUARD`` sentinel elements behind the logical end of every array they hand out.

Part B - basis composition (``BASIS_CASES``), nn._BasisCompose forward and backward.  kGroup = 6 rows are loaded per group
with the row index clamped to nb - 1 (``b0 + j < nb ? b0 + j : nb - 1``); a thread owns chunks of 4 columns, a block 256
chunks, the grid is basis_blocks(cols) = min(cdiv(cols / 4, 256), 2048) blocks and strides (``ch += gridDim.x * 256``).
  * ra1..ra5 at nb = 30, cols = 8192: every ``case RA`` of the backward's switch at the model's number of bases (5 full groups).
  * ra2_nb1_c4: one chunk - 255 threads of the block never enter the loop and feed zeros into wave_sum / red[][]; the first
    group holds one row, five lanes of ``x[j]`` are clamped loads.
  * ra3_nb5_c1020: nb < kGroup (one ragged group); 255 chunks: the block's last thread idles.
  * ra4_nb6_c1024: exactly one full group, exactly one full block.
  * ra5_nb7_c1028: the second group holds one row; the second block holds one chunk.
  * ra5_nb31_c4096: six groups, the last ragged at nb - 1 (one row).
  * ra5_nb32_stride: cols = 2,097,152 + 1036: kMaxRB = 160 coefficients fill ``cs``; 2050 blocks are capped to 2048 and 259
    chunks take a second trip.
  * ra2_nb12_stride3: cols = 2 * 2,097,152 + 1036: 259 threads make three trips, the others two.
  * exact_*: comp, weight and dW drawn from {-1, 0, 1}: every partial sum is an integer below 2^24 (at most 4.2 M terms), so
    w, dweight and dcomp equal the float64 result exactly - a dropped or double-counted chunk cannot hide.
  * fallback_nb33 / fallback_c6: geometries the kernels refuse take ``comp @ weight``: no basis_compose_* kernel runs.

Budgets, per element, derived from the arithmetic and not tuned; u = 2^-24, magnitudes in float64 from the fp32 inputs:
  * w:       (nb + 1) u sum_b |comp[r, b] weight[b, c]|: nb FMAs in sequence, one rounding each.
  * dweight: (ra + 1) u sum_r |comp[r, b] dW[r, c]|: ra FMAs in sequence.
  * dcomp:   D u sum_c |dW[r, c] weight[b, c]| with D the longest chain of roundings a term goes through,
             D = 5 trips + 6 + 2 + ceil(blocks / 8) + 3, trips = ceil(nch / (blocks * 256)): per trip a 4-term dot (4 products
             and 3 adds, at most 4 roundings on the longest path) and the add into dc[r][b]; the 6 steps of wave_sum; two adds
             over the four waves' red[][]; rows_sum_kernel adds the ``blocks`` partials in 8 lanes (ceil(blocks / 8) serial
             adds at most) and joins the lanes with a 3-level tree."""
import ctypes
import zlib
from dataclasses import dataclass, field

import numpy as np
import pytest
import torch

import gmlm_oracle as O
from helpers import kernels_run

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
THRESH = 64
GUARD = 64

ZERO, DEG, I2F, BUCKET, HIST = "zero_words_kernel", "degree_kernel", "i32_to_f32_kernel", "edge_bucket_kernel", "rel_hist_kernel"
KEYS, ROWPTR, INV, SPLIT = "make_keys_kernel", "rowptr_fill_kernel", "inv_count_kernel", "split_plan_kernel"
G64, G32 = "gather_kernel<long>", "gather_kernel<int>"
GRAPH_KERNEL_NAMES = (ZERO, DEG, I2F, BUCKET, HIST, KEYS, ROWPTR, "gather_kernel", INV, SPLIT)

_SORT = {ZERO, KEYS, ROWPTR}                                   # gmlm_segment_sort with edges
_CSR = _SORT | {HIST, G64, G32, INV}                           # build_rel_csr with edges and a given edge_type
_TYPES = {ZERO, DEG, BUCKET}                                   # edge_types_from_degree with edges


def _is_graph_or_basis(name):
    """The kernels the CPU guard holds to GRAPH_CASES / BASIS_CASES / UNREACHABLE."""
    return name.split("<")[0] in GRAPH_KERNEL_NAMES or name.startswith("basis_compose_")


@dataclass(frozen=True)
class Stride:
    """A claim of the docstring: ``kernel`` runs over ``n`` elements with its grid capped at ``cap`` blocks and makes ``trips``
    passes of its grid-stride loop (held to grid_cap by the CPU guard)."""
    kernel: str
    n: int
    cap: int
    trips: int


@dataclass(frozen=True)
class GraphCase:
    id: str
    calls: tuple               # ((what, frozenset of the gmlm:: kernels that call launches), ...)
    strides: tuple = ()

    @property
    def kernels(self):
        return frozenset().union(*(k for _, k in self.calls))

    def call(self, what):
        return set(dict(self.calls)[what])


E2, N2, RA2, NDEG2 = 2048 * 256 + 300, 180_000, 3, 524_288 + 5
END_BIT_NSEG = (1, 2, 1024, 1025, 65536, 65537)
SPLIT_NSEG = (1, 1023, 1024, 1025, 200_000)
SPLIT_LAYOUTS = ("none_long", "one_segment", "exact_lengths", "all_65", "clustered")


def _gc(id_, calls, strides=()):
    return GraphCase(id_, tuple((w, frozenset(k)) for w, k in calls), tuple(strides))


GRAPH_CASES = {c.id: c for c in [
    _gc("second_trip",
        [("edge_types", _TYPES), ("degree_f32", {ZERO, DEG, I2F}), ("build", _CSR), ("split_plan", {SPLIT})],
        [Stride(DEG, E2, 2048, 2), Stride(BUCKET, E2, 2048, 2), Stride(HIST, E2, 1024, 3), Stride(KEYS, E2, 2048, 2),
         Stride(ROWPTR, E2 + 1, 2048, 2), Stride(G64, E2, 2048, 2), Stride(G32, E2, 2048, 2), Stride(INV, N2 * RA2, 2048, 2),
         Stride(I2F, NDEG2, 2048, 2)]),
    _gc("hot_node", [("degree_f32", {ZERO, DEG, I2F}), ("build", _TYPES | _CSR)]),
    _gc("bucket_boundaries", [("edge_types", _TYPES), ("build", {BUCKET} | _CSR)]),
    _gc("hist_r64", [("build", _CSR)]),
    _gc("hist_r1", [("build", _CSR)]),
    _gc("hist_rejects", [("build", {ZERO, HIST})]),
    _gc("end_bit", [("sort", _SORT)]),
    _gc("null_keys", [("with_keys", _SORT | {G64, G32, INV}), ("null_keys", _SORT | {G64, INV}), ("short_workspace", set())]),
    _gc("flagged_ids", [("raw_build", _SORT | {BUCKET, G64, G32, INV})]),
    _gc("no_edges", [("build", {ZERO, INV})]),
    _gc("split_plan", [("plan", {SPLIT}), ("refused", set())]),
]}


@dataclass(frozen=True)
class BasisCase:
    id: str
    ra: int
    nb: int
    cols: int
    nb_mod: int = -1           # nb mod kGroup, as the docstring says (hip cases)
    nch_mod: int = -1          # (cols / 4) mod 256
    blocks: int = 0            # basis_blocks(cols)
    trips: tuple = (1,)        # the numbers of passes of ``ch += gridDim.x * 256`` that threads with a chunk make
    ints: bool = False         # data in {-1, 0, 1}: exact
    hip: bool = True           # False: the geometry takes comp @ weight
    fwd: frozenset = field(default=frozenset(), compare=False)
    bwd: frozenset = field(default=frozenset(), compare=False)


FWD = "basis_compose_fwd_kernel"
ROWS_SUM = "rows_sum_kernel"


def bwd(ra):
    return f"basis_compose_bwd_kernel<{ra}>"


def _bc(id_, ra, nb, cols, **kw):
    hip = kw.get("hip", True)
    return BasisCase(id_, ra, nb, cols, fwd=frozenset({FWD} if hip else ()), bwd=frozenset({bwd(ra), ROWS_SUM} if hip else ()), **kw)


C_STRIDE2, C_STRIDE3 = 2_097_152 + 1036, 2 * 2_097_152 + 1036
BASIS_CASES = [_bc(f"ra{ra}_nb30_c8192", ra, 30, 8192, nb_mod=0, nch_mod=0, blocks=8) for ra in (1, 2, 3, 4, 5)] + [
    _bc("ra2_nb1_c4", 2, 1, 4, nb_mod=1, nch_mod=1, blocks=1),
    _bc("ra3_nb5_c1020", 3, 5, 1020, nb_mod=5, nch_mod=255, blocks=1),
    _bc("ra4_nb6_c1024", 4, 6, 1024, nb_mod=0, nch_mod=0, blocks=1),
    _bc("ra5_nb7_c1028", 5, 7, 1028, nb_mod=1, nch_mod=1, blocks=2),
    _bc("ra5_nb31_c4096", 5, 31, 4096, nb_mod=1, nch_mod=0, blocks=4),
    _bc("ra5_nb32_stride", 5, 32, C_STRIDE2, nb_mod=2, nch_mod=3, blocks=2048, trips=(1, 2)),
    _bc("ra2_nb12_stride3", 2, 12, C_STRIDE3, nb_mod=0, nch_mod=3, blocks=2048, trips=(2, 3)),
    _bc("exact_ra5_nb32_stride", 5, 32, C_STRIDE2, nb_mod=2, nch_mod=3, blocks=2048, trips=(1, 2), ints=True),
    _bc("exact_ra2_nb12_stride3", 2, 12, C_STRIDE3, nb_mod=0, nch_mod=3, blocks=2048, trips=(2, 3), ints=True),
    _bc("exact_ra5_nb7_c1028", 5, 7, 1028, nb_mod=1, nch_mod=1, blocks=2, ints=True),
    _bc("fallback_nb33", 3, 33, 1024, blocks=1, hip=False),
    _bc("fallback_c6", 2, 5, 6, blocks=1, hip=False),
]
UNREACHABLE = {}


def split_layout(name, nseg, thresh=THRESH):
    """Segment lengths (int64 [nseg]) of a split-plan layout; shared with the capacity check of the CPU guard."""
    t = thresh
    lens = np.zeros(nseg, dtype=np.int64)
    per = (nseg + 1023) // 1024
    if name == "none_long":                          # lengths up to thresh: ``len > thresh`` is false at len == thresh
        lens[:] = np.random.default_rng(nseg).integers(0, t + 1, nseg) if nseg <= 2048 else np.arange(nseg) % 4
        lens[nseg // 2] = t
    elif name == "one_segment":
        lens[nseg // 2] = 120 * t + 17
    elif name == "exact_lengths":                    # thresh, thresh + 1, 2 thresh, 2 thresh + 1 (one, two, two, three chunks)
        for j, n in enumerate((t, t + 1, 2 * t, 2 * t + 1)):
            lens[j * (nseg - 1) // 3] = n
    elif name == "all_65":                           # the most long segments an item count can hold
        if nseg <= 2048:
            lens[:] = t + 1
        else:                                        # 60,000 long segments: below the 65535 gmlm_split_plan_build accepts
            lens[:180_000:3] = t + 1
    elif name == "clustered":                        # several long segments in one thread's range; first and last range
        base = (nseg // 2 // per) * per
        for off, n in ((0, t + 6), (1, 3 * t + 8), (2, t + 1), (per - 1, 15 * t + 40)):
            lens[min(base + off, nseg - 1)] = n
        lens[0] = 2 * t + 2
        lens[nseg - 1] = 4 * t
        lens[1:nseg - 1:7] += 3
    else:
        raise KeyError(name)
    return lens


# ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import gmlm_amd
    gmlm_amd.lib()
    return torch.device("cuda:0")


def _seed(name):
    return zlib.crc32(name.encode())


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def _np_csr(src, keys, nseg, num_src, t_keys=None):
    """numpy build from the segment key of every edge (dst * R_a + slot): stable argsort, bincount, cumsum; the transpose is
    sorted by ``t_keys`` (the source ids unless given)."""
    keys = np.asarray(keys, dtype=np.int64)
    t_keys = np.asarray(src if t_keys is None else t_keys, dtype=np.int64)
    perm = np.argsort(keys, kind="stable")
    cnt = np.bincount(keys, minlength=nseg)
    t_perm = np.argsort(t_keys, kind="stable")
    return dict(keys=keys.astype(np.int32), perm=perm.astype(np.int32),
                rowptr=np.concatenate([[0], np.cumsum(cnt)]).astype(np.int32), col=src[perm].astype(np.int32),
                inv_cnt=np.float32(1) / np.maximum(cnt, 1).astype(np.float32),
                t_rowptr=np.concatenate([[0], np.cumsum(np.bincount(t_keys, minlength=num_src))]).astype(np.int32),
                t_seg=keys[t_perm].astype(np.int32))


def _check_csr(csr, ei, et, num_nodes, num_src=None):
    """A RelCSR against numpy, every array and every element; ``ei`` int64 [2, E] and ``et`` int64 [E] on the CPU."""
    num_src = num_src or num_nodes
    src, dst, rel = ei[0].numpy(), ei[1].numpy(), et.numpy()
    active = sorted(set(rel.tolist())) or [0]
    assert csr.active_relations == active
    slot = np.searchsorted(np.asarray(active), rel)
    r_a = len(active)
    want = _np_csr(src, dst * r_a + slot, num_nodes * r_a, num_src)
    # gmlm_oracle.relation_csr is the project's own checker of the same build: the two references must agree
    o_rowptr, o_col, o_eid = O.relation_csr(ei, torch.from_numpy(slot), num_nodes, r_a)
    assert np.array_equal(o_rowptr, want["rowptr"]) and np.array_equal(o_col, want["col"]) and np.array_equal(o_eid, want["perm"])
    assert csr.edge_type.dtype == torch.long and np.array_equal(csr.edge_type.cpu().numpy(), rel)
    for name in ("rowptr", "col", "perm", "t_rowptr", "t_seg"):
        got = getattr(csr, name)
        assert got.dtype == torch.int32 and np.array_equal(got.cpu().numpy(), want[name]), name
    assert csr.inv_cnt.dtype == torch.float32 and np.array_equal(_bits(csr.inv_cnt.cpu().numpy()), _bits(want["inv_cnt"])), "inv_cnt"
    assert int(want["rowptr"][-1]) == src.size == csr.num_edges
    return want


def _run(case, what, fn):
    """Runs ``fn`` under the profiler and holds the gmlm:: kernels it launched to the case's table entry."""
    box = []
    ran = kernels_run(lambda: box.append(fn()))
    print(f"\n{case.id}/{what}: {sorted(ran)}")
    assert ran == case.call(what), (case.id, what, sorted(ran), sorted(case.call(what)))
    return box[0]


def _check_plan(plan, rowptr_np, thresh):
    long_seg, chunk_ptr, owner = O.split_plan(rowptr_np, thresh)
    nl, nc = long_seg.size, owner.size
    assert plan.n_long >= nl and plan.n_chunks >= nc and plan.long_seg.numel() == plan.n_long
    assert plan.chunk_ptr.numel() == plan.n_long + 1 and plan.chunk_owner.numel() == plan.n_chunks
    got_l, got_p, got_o = plan.long_seg.cpu().numpy(), plan.chunk_ptr.cpu().numpy(), plan.chunk_owner.cpu().numpy()
    assert np.array_equal(got_l[:nl], long_seg) and np.array_equal(got_p[:nl + 1], chunk_ptr) and np.array_equal(got_o[:nc], owner)
    assert (got_l[nl:] == -1).all() and (got_o[nc:] == -1).all() and (got_p[nl:] == nc).all()
    return nl, nc


# ------------------------------------------------------------------------------------------------------- Part A: python layer
def test_second_trip_of_every_grid_stride_loop(dev):
    import gmlm_amd
    from gmlm_amd import ops
    case = GRAPH_CASES["second_trip"]
    g = torch.Generator().manual_seed(_seed(case.id))
    ei = torch.randint(0, N2, (2, E2), generator=g)
    ei[1, :5000] = 7                                                   # long segments for the split plan
    ei[0, -300:] = 11                                                  # the second trip's edges meet one counter
    ei[1, -300:] = N2 - 1                                              # and land in the last node's segments
    et = torch.tensor([0, 2, 4])[torch.randint(0, 3, (E2,), generator=g)]
    d_ei = ei.to(dev)

    types = _run(case, "edge_types", lambda: gmlm_amd.edge_types_from_degree(d_ei, N2))
    assert types.dtype == torch.long and np.array_equal(types.cpu().numpy(), O.edge_types_from_degree(ei, N2).numpy())

    degf = _run(case, "degree_f32", lambda: gmlm_amd.degree(d_ei[0], NDEG2, dtype=torch.float32))
    assert degf.dtype == torch.float32 and degf.shape == (NDEG2,)
    assert np.array_equal(_bits(degf.cpu().numpy()), _bits(np.bincount(ei[0].numpy(), minlength=NDEG2).astype(np.float32)))

    csr = _run(case, "build", lambda: gmlm_amd.build_rel_csr(d_ei, N2, 5, et.to(dev)))
    assert csr.active_relations == [0, 2, 4] and csr.r_active == RA2
    want = _check_csr(csr, ei, et, N2)

    plan = _run(case, "split_plan", lambda: ops.device_split_plan(csr.rowptr, E2, THRESH))
    nl, _ = _check_plan(plan, want["rowptr"], THRESH)
    assert nl >= 3


def test_one_hot_node(dev):
    import gmlm_amd
    case = GRAPH_CASES["hot_node"]
    e, n = 70_001, 9
    ei = torch.stack([torch.full((e,), 3), torch.full((e,), 5)])
    d_ei = ei.to(dev)
    degf = _run(case, "degree_f32", lambda: gmlm_amd.degree(d_ei[0], n))
    want_deg = np.zeros(n, dtype=np.float32)
    want_deg[3] = e                                                    # exact: e < 2^24
    assert np.array_equal(_bits(degf.cpu().numpy()), _bits(want_deg))
    csr = _run(case, "build", lambda: gmlm_amd.build_rel_csr(d_ei, n, 5))
    _check_csr(csr, ei, torch.full((e,), 3), n)
    assert csr.active_relations == [3]
    assert np.array_equal(csr.perm.cpu().numpy(), np.arange(e, dtype=np.int32)), "equal keys must keep their order"
    rowptr = csr.rowptr.cpu().numpy()
    assert (rowptr[:6] == 0).all() and (rowptr[6:] == e).all()


def test_degree_bucket_boundaries(dev):
    import gmlm_amd
    case = GRAPH_CASES["bucket_boundaries"]
    n = 13
    src = np.repeat(np.arange(n), np.arange(n))                        # node k is the source of k edges
    g = np.random.default_rng(_seed(case.id))
    order = g.permutation(src.size)
    ei = torch.from_numpy(np.stack([src[order], g.integers(0, n, src.size)]))
    d_ei = ei.to(dev)
    bucket = lambda d: np.where(d <= 2, 0, np.where(d <= 5, 1, np.where(d <= 10, 2, 3))).astype(np.int64)
    assert bucket(np.arange(n)).tolist() == [0, 0, 0, 1, 1, 1, 2, 2, 2, 2, 2, 3, 3]

    types = _run(case, "edge_types", lambda: gmlm_amd.edge_types_from_degree(d_ei, n))
    local = np.bincount(ei[0].numpy(), minlength=n)
    assert local.tolist() == list(range(n))
    assert np.array_equal(types.cpu().numpy(), bucket(local[ei[0].numpy()]))
    assert np.array_equal(types.cpu().numpy(), O.edge_types_from_degree(ei, n).numpy())

    given = torch.arange(n - 1, -1, -1, dtype=torch.int32)             # the partition path: degrees that are not the local ones
    csr = _run(case, "build", lambda: gmlm_amd.build_rel_csr(d_ei, n, 5, src_degree_for_types=given.to(dev)))
    want_types = bucket(given.numpy()[ei[0].numpy()])
    assert sorted(set(want_types.tolist())) == [0, 1, 2, 3]
    _check_csr(csr, ei, torch.from_numpy(want_types), n)


@pytest.mark.parametrize("r", [64, 1])
def test_histogram_relation_counts(dev, r):
    import gmlm_amd
    case = GRAPH_CASES[f"hist_r{r}"]
    g = torch.Generator().manual_seed(_seed(case.id))
    e, n = 5000, 50
    ei = torch.randint(0, n, (2, e), generator=g)
    et = (torch.arange(e) % r)[torch.randperm(e, generator=g)]
    csr = _run(case, "build", lambda: gmlm_amd.build_rel_csr(ei.to(dev), n, r, et.to(dev)))
    assert csr.active_relations == list(range(r))
    _check_csr(csr, ei, et, n)


def test_histogram_rejects_foreign_relations_before_the_remap_read(dev):
    import gmlm_amd
    case = GRAPH_CASES["hist_rejects"]
    ei = torch.randint(0, 20, (2, 300), generator=torch.Generator().manual_seed(_seed(case.id))).to(dev)
    for bad in (-1, 64):
        et = (torch.arange(300) % 64)
        et[137] = bad
        d_et = et.to(dev)

        def build():
            with pytest.raises(ValueError, match="outside"):
                gmlm_amd.build_rel_csr(ei, 20, 64, d_et)
        _run(case, "build", build)


@pytest.mark.parametrize("nseg", END_BIT_NSEG)
def test_radix_end_bit_boundaries(dev, nseg):
    from gmlm_amd import graph
    case = GRAPH_CASES["end_bit"]
    g = torch.Generator().manual_seed(_seed(case.id) + nseg)
    vals = torch.tensor(sorted({0, nseg - 1, nseg // 2, min(3, nseg - 1)}))
    ids = vals[torch.randint(0, vals.numel(), (50,), generator=g)]
    ids[0], ids[1] = nseg - 1, 0
    keys, perm, rowptr, bad = _run(case, "sort", lambda: graph._segment_sort(ids.to(dev), None, None, 1, nseg))
    want = _np_csr(ids.numpy(), ids.numpy(), nseg, nseg)
    assert int(bad) == 0
    assert np.array_equal(keys.cpu().numpy(), want["keys"]) and np.array_equal(perm.cpu().numpy(), want["perm"])
    assert rowptr.shape == (nseg + 1,) and np.array_equal(rowptr.cpu().numpy(), want["rowptr"])


@pytest.mark.parametrize("n", [1, 1000])
def test_graph_without_edges(dev, n):
    import gmlm_amd
    case = GRAPH_CASES["no_edges"]
    ei = torch.zeros(2, 0, dtype=torch.long)
    csr = _run(case, "build", lambda: gmlm_amd.build_rel_csr(ei.to(dev), n, 5))
    assert csr.active_relations == [0] and csr.num_edges == 0
    _check_csr(csr, ei, torch.zeros(0, dtype=torch.long), n)
    assert csr.rowptr.shape == (n + 1,) and not bool(csr.rowptr.any()) and not bool(csr.t_rowptr.any())
    assert bool((csr.inv_cnt == 1).all()) and csr.split is None and csr.t_split is None


# ----------------------------------------------------------------------------------------------------------- Part A: raw ABI
_SENT = {torch.int32: -777, torch.int64: -777, torch.float32: -77.0}


def _guarded(n, dtype, dev):
    return torch.full((n + GUARD,), _SENT[dtype], dtype=dtype, device=dev)


def _raw_build(dev, src, dst, num_nodes, num_src, r_active, remap, rel=None, deg=None, null_keys=False):
    """build_rel_csr's sequence of C calls on buffers of this test: GUARD sentinel elements behind the logical end of every
    array handed out, checked after the last call.  ``deg``: edge types come from gmlm_edge_bucket; else ``rel`` is given."""
    from gmlm_amd import ops
    lib, p, st = ops.lib(), ops._ptr, ops._stream()
    e, nseg = src.numel(), num_nodes * r_active
    buf = dict(keys=_guarded(e, torch.int32, dev), perm=_guarded(e, torch.int32, dev), rowptr=_guarded(nseg + 1, torch.int32, dev),
               col=_guarded(e, torch.int32, dev), inv_cnt=_guarded(nseg, torch.float32, dev), t_keys=_guarded(e, torch.int32, dev),
               t_perm=_guarded(e, torch.int32, dev), t_rowptr=_guarded(num_src + 1, torch.int32, dev),
               t_seg=_guarded(e, torch.int32, dev), edge_type=_guarded(e, torch.int64, dev), bad=_guarded(1, torch.int32, dev),
               bad2=_guarded(1, torch.int32, dev))
    size = dict(keys=e, perm=e, rowptr=nseg + 1, col=e, inv_cnt=nseg, t_keys=e, t_perm=e, t_rowptr=num_src + 1, t_seg=e, edge_type=e,
                bad=1, bad2=1)
    if deg is not None:
        ops.check(lib.gmlm_edge_bucket(p(src), p(deg), e, deg.numel(), p(buf["edge_type"]), st), "gmlm_edge_bucket")
    else:
        buf["edge_type"][:e] = rel
    nbytes = lib.gmlm_segment_sort_workspace_bytes(e)
    ws = ops._ws(nbytes, dev)
    ops.check(lib.gmlm_segment_sort(p(dst), p(buf["edge_type"]), p(remap), r_active, e, nseg, None if null_keys else p(buf["keys"]),
                                    p(buf["perm"]), p(buf["rowptr"]), p(buf["bad"]), p(ws), nbytes, st), "gmlm_segment_sort")
    ops.check(lib.gmlm_gather_i64_to_i32(p(src), p(buf["perm"]), e, p(buf["col"]), st), "gmlm_gather_i64_to_i32")
    ops.check(lib.gmlm_segment_inv_count(p(buf["rowptr"]), nseg, p(buf["inv_cnt"]), st), "gmlm_segment_inv_count")
    ops.check(lib.gmlm_segment_sort(p(src), None, None, 1, e, num_src, p(buf["t_keys"]), p(buf["t_perm"]), p(buf["t_rowptr"]),
                                    p(buf["bad2"]), p(ws), nbytes, st), "gmlm_segment_sort")
    written = set(size)
    if null_keys:                                                     # no keys to carry over to the transpose
        written -= {"keys", "t_seg"}
    else:
        ops.check(lib.gmlm_gather_i32(p(buf["keys"]), p(buf["t_perm"]), e, p(buf["t_seg"]), st), "gmlm_gather_i32")
    torch.cuda.synchronize()
    out = {}
    for name, t_ in buf.items():
        n = size[name] if name in written else 0
        assert bool((t_[n:] == _SENT[t_.dtype]).all()), f"{name}: written behind its logical end ({n} elements)"
        out[name] = t_[:size[name]].cpu().numpy()
    return out


def _raw_compare(got, want, names):
    for name in names:
        if name == "inv_cnt":
            assert np.array_equal(_bits(got[name]), _bits(want[name])), name
        else:
            assert np.array_equal(got[name], want[name]), name


def test_segment_sort_without_a_keys_buffer(dev):
    from gmlm_amd import ops
    case = GRAPH_CASES["null_keys"]
    g = torch.Generator().manual_seed(_seed(case.id))
    e, n, r = 3001, 40, 5
    src, dst = torch.randint(0, n, (e,), generator=g), torch.randint(0, n, (e,), generator=g)
    rel = torch.tensor([0, 2, 4])[torch.randint(0, 3, (e,), generator=g)]
    remap = torch.tensor([0, -1, 1, -1, 2], dtype=torch.int32)
    args = (dev, src.to(dev), dst.to(dev), n, n, 3, remap.to(dev))
    with_keys = _run(case, "with_keys", lambda: _raw_build(*args, rel=rel.to(dev)))
    no_keys = _run(case, "null_keys", lambda: _raw_build(*args, rel=rel.to(dev), null_keys=True))
    want = _np_csr(src.numpy(), dst.numpy() * 3 + remap.numpy()[rel.numpy()], n * 3, n)
    assert int(with_keys["bad"][0]) == 0 and int(with_keys["bad2"][0]) == 0 and int(no_keys["bad"][0]) == 0
    _raw_compare(with_keys, want, ("keys", "perm", "rowptr", "col", "inv_cnt", "t_rowptr", "t_seg"))
    _raw_compare(no_keys, want, ("perm", "rowptr", "col", "inv_cnt", "t_rowptr"))
    assert np.array_equal(with_keys["t_keys"], src.numpy().astype(np.int32))

    lib, p = ops.lib(), ops._ptr
    nbytes = lib.gmlm_segment_sort_workspace_bytes(e)
    ws, perm, rowptr, bad = ops._ws(nbytes, dev), _guarded(e, torch.int32, dev), _guarded(n * 3 + 1, torch.int32, dev), _guarded(1, torch.int32, dev)

    def short():
        rc = lib.gmlm_segment_sort(p(args[2]), None, None, 1, e, n, None, p(perm), p(rowptr), p(bad), p(ws), nbytes - 1, ops._stream())
        assert rc == -2 and b"workspace too small" in lib.gmlm_last_error()
        torch.zeros(1, device=dev)                                    # a device kernel for the profiler to see; not the project's
    _run(case, "short_workspace", short)
    for t_ in (perm, rowptr, bad):
        assert bool((t_ == _SENT[torch.int32]).all()), "a refused call wrote"


def test_flagged_ids_are_clamped_not_written_out_of_range(dev):
    case = GRAPH_CASES["flagged_ids"]
    g = torch.Generator().manual_seed(_seed(case.id))
    e, n, num_src, r_a = 2000, 30, 37, 3
    src, dst = torch.randint(0, num_src, (e,), generator=g), torch.randint(0, n, (e,), generator=g)
    deg = torch.randint(0, 14, (num_src,), generator=g).to(torch.int32)
    remap = torch.tensor([0, 1, -1, 2, -1], dtype=torch.int32)        # relation 2 (degrees 6 .. 10) occurs and has no slot
    dst[5], dst[6], dst[1999] = n, -1, n                              # targets outside the graph
    src[7], src[8] = -1, num_src                                      # sources outside: degree 0, transposed key 0
    got = _run(case, "raw_build", lambda: _raw_build(dev, src.to(dev), dst.to(dev), n, num_src, r_a, remap.to(dev), deg=deg.to(dev)))

    s, d = src.numpy(), dst.numpy()
    dd = np.where((s >= 0) & (s < num_src), deg.numpy()[np.clip(s, 0, num_src - 1)], 0)
    rel = np.where(dd <= 2, 0, np.where(dd <= 5, 1, np.where(dd <= 10, 2, 3))).astype(np.int64)
    assert (rel == 2).any()
    m = remap.numpy()[rel]
    keys = np.where(m < 0, 0, d * r_a + m)
    keys = np.where((keys < 0) | (keys >= n * r_a), 0, keys)
    t_keys = np.where((s < 0) | (s >= num_src), 0, s)
    want = _np_csr(s, keys, n * r_a, num_src, t_keys=t_keys)
    assert np.array_equal(got["edge_type"], rel)
    assert int(got["bad"][0]) != 0 and int(got["bad2"][0]) != 0
    assert got["keys"].min() >= 0 and got["keys"].max() < n * r_a
    assert int(got["rowptr"][-1]) == e and int(got["t_rowptr"][-1]) == e
    _raw_compare(got, want, ("keys", "perm", "rowptr", "col", "inv_cnt", "t_rowptr", "t_seg"))
    assert np.array_equal(got["t_keys"], t_keys.astype(np.int32))


# -------------------------------------------------------------------------------------------------------- Part A: split plan
@pytest.mark.parametrize("layout", SPLIT_LAYOUTS)
@pytest.mark.parametrize("nseg", SPLIT_NSEG)
def test_device_split_plan(dev, nseg, layout):
    from gmlm_amd import ops
    case = GRAPH_CASES["split_plan"]
    lens = split_layout(layout, nseg)
    rowptr_np = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    rowptr = torch.from_numpy(rowptr_np).to(dev)
    items = int(rowptr_np[-1])
    plan = _run(case, "plan", lambda: ops.device_split_plan(rowptr, items, THRESH))
    nl, nc = _check_plan(plan, rowptr_np, THRESH)
    print(f"  nseg {nseg} {layout}: {items} items, {nl} long of {plan.n_long}, {nc} chunks of {plan.n_chunks}")
    assert (nl == 0) == (layout == "none_long")
    again = ops.device_split_plan(rowptr, items, THRESH)
    for a, b in ((plan.long_seg, again.long_seg), (plan.chunk_ptr, again.chunk_ptr), (plan.chunk_owner, again.chunk_owner)):
        assert torch.equal(a, b), "two builds differ"


def test_split_plan_refuses_more_than_65535_possible_long_segments(dev):
    from gmlm_amd import ops
    case = GRAPH_CASES["split_plan"]
    lib, p = ops.lib(), ops._ptr
    items = 65535 * THRESH                                            # items / thresh + 1 = 65536
    rowptr = torch.tensor([0, items], dtype=torch.int32, device=dev)
    # capacity-sized, so that a build which does NOT refuse fails the assertion below and writes nothing out of bounds
    cap = items // THRESH + 1
    arrays = [_guarded(n, torch.int32, dev) for n in (cap, cap + 1, cap + items // THRESH)]

    def refused():
        rc = lib.gmlm_split_plan_build(p(rowptr), 1, items, THRESH, *(p(a) for a in arrays), ops._stream())
        assert rc == -1 and b"long_threshold" in lib.gmlm_last_error()
        torch.zeros(1, device=dev)                                    # a device kernel for the profiler to see; not the project's
    _run(case, "refused", refused)
    assert all(bool((a == _SENT[torch.int32]).all()) for a in arrays), "a refused call wrote"
    # one item fewer is accepted by the same check
    cl, cc = ctypes.c_int64(), ctypes.c_int64()
    assert lib.gmlm_split_plan_capacity(items - 1, THRESH, ctypes.byref(cl), ctypes.byref(cc)) == 0 and cl.value == 65535


# ---------------------------------------------------------------------------------------------------------------- Part B
def dcomp_depth(cols, blocks):
    """D of the dcomp budget, written out from basis_compose_bwd_kernel and rows_sum_kernel (module docstring)."""
    nch = cols // 4
    trips = -(-nch // (blocks * 256))
    return 5 * trips + 6 + 2 + -(-blocks // 8) + 3


def _basis_inputs(c, dev):
    g = torch.Generator(device=dev).manual_seed(_seed(c.id))
    if c.ints:
        draw = lambda *s: torch.randint(-1, 2, s, generator=g, device=dev).float()
    else:
        draw = lambda *s: torch.randn(*s, generator=g, device=dev)
    return draw(c.ra, c.nb), draw(c.nb, c.cols), draw(c.ra, c.cols)


def _basis_run(comp, weight, dw):
    from gmlm_amd import nn as gnn
    comp, weight = comp.clone().requires_grad_(True), weight.detach().requires_grad_(True)
    out = {}

    def fwd():
        out["w"] = gnn._BasisCompose.apply(comp, weight, None)

    def back():
        out["dcomp"], out["dweight"] = torch.autograd.grad(out["w"], (comp, weight), dw)
    return out, fwd, back


def _row_dots(a, b):
    """a [ra, cols] and b [nb, cols] -> [ra, nb] of float64 dot products over the columns: full-width reductions (a GEMM with
    cols as its inner dimension and 160 outputs would run in a handful of blocks)."""
    return torch.stack([(b * a[r]).sum(1) for r in range(a.shape[0])])


def _budget(name, got, ref, bound):
    err = (got.double() - ref).abs()
    ok = err <= bound                                                 # False for NaN
    pos = bound > 0
    worst = float((err[pos] / bound[pos]).max()) if bool(pos.any()) else 0.0
    nbad = int((~ok).sum())
    print(f"  {name}: max err / bound = {worst:.3f}, {nbad} of {ok.numel()} outside")
    return nbad, worst


@pytest.mark.parametrize("c", BASIS_CASES, ids=[c.id for c in BASIS_CASES])
def test_basis_compose_vs_fp64(dev, c):
    comp, weight, dw = _basis_inputs(c, dev)
    out, fwd, back = _basis_run(comp, weight, dw)
    ran_f, ran_b = kernels_run(fwd), kernels_run(back)
    print(f"\n{c.id}: {sorted(ran_f)} / {sorted(ran_b)}")
    assert ran_f == set(c.fwd) and ran_b == set(c.bwd), (sorted(ran_f), sorted(ran_b))
    w, dcomp, dweight = out["w"].detach(), out["dcomp"], out["dweight"]
    assert w.shape == (c.ra, c.cols) and dcomp.shape == (c.ra, c.nb) and dweight.shape == (c.nb, c.cols)
    assert w.dtype == dcomp.dtype == dweight.dtype == torch.float32

    depth = dcomp_depth(c.cols, c.blocks)
    comp64, dw64 = comp.double(), dw.double()
    bad = []
    w64 = weight.double()
    bad.append(_budget("w", w, comp64 @ w64, (c.nb + 1) * U * (comp64.abs() @ w64.abs())))
    ref_w = (comp64 @ w64) if c.ints else None
    ref_dc = _row_dots(dw64, w64)
    bad.append(_budget("dcomp", dcomp, ref_dc, depth * U * _row_dots(dw64.abs(), w64.abs())))
    del w64
    ref_dwt = comp64.t() @ dw64
    bad.append(_budget("dweight", dweight, ref_dwt, (c.ra + 1) * U * (comp64.abs().t() @ dw64.abs())))
    assert not any(n for n, _ in bad), (c.id, bad)
    if c.ints:
        assert float(ref_dc.abs().max()) < 2 ** 24
        assert torch.equal(w.double(), ref_w) and torch.equal(dweight.double(), ref_dwt) and torch.equal(dcomp.double(), ref_dc), \
            "an integer sum is not exact"
    del ref_dwt, ref_w

    out2, fwd2, back2 = _basis_run(comp, weight, dw)
    fwd2()
    back2()
    assert torch.equal(out2["w"].detach(), w) and torch.equal(out2["dcomp"], dcomp) and torch.equal(out2["dweight"], dweight), \
        "two runs differ"


_REFUSALS = [  # (ra, nb, cols, weight offset in bytes, workspace shortfall in bytes, message)
    (0, 30, 1024, 0, 0, b"active relations"), (6, 30, 1024, 0, 0, b"active relations"),
    (3, 0, 1024, 0, 0, b"bases supported"), (3, 33, 1024, 0, 0, b"bases supported"),
    (3, 30, 0, 0, 0, b"positive multiple of 4"), (3, 30, 6, 0, 0, b"positive multiple of 4"),
    (3, 30, 1024, 4, 0, b"misaligned pointer"), (3, 30, 1024, 0, 4, b"workspace too small"),
]


def test_basis_raw_abi_refusals(dev):
    """Status -1 and the message of every refusal of gmlm_basis_compose_fwd / _bwd, on real device buffers that must come back
    untouched; the workspace refusal is the backward's alone."""
    from gmlm_amd import ops
    lib, p, st = ops.lib(), ops._ptr, ops._stream()
    comp = torch.ones(5, 33, device=dev)
    weight = torch.ones(33 * 1024 + 4, device=dev)
    dw = torch.ones(6 * 1024, device=dev)
    sent = _SENT[torch.float32]
    for ra, nb, cols, off, short, msg in _REFUSALS:
        w, dweight, dcomp = (torch.full((n,), sent, device=dev) for n in (6 * 1024, 33 * 1024, 6 * 33))
        wp = p(weight) + off
        nbytes = lib.gmlm_basis_compose_bwd_workspace_bytes(max(ra, 1), max(nb, 1), max(cols, 4))
        ws = ops._ws(nbytes, dev)
        if not short:
            rc = lib.gmlm_basis_compose_fwd(p(comp), wp, ra, nb, cols, p(w), st)
            assert rc == -1 and msg in lib.gmlm_last_error(), (ra, nb, cols, off, lib.gmlm_last_error())
        rc = lib.gmlm_basis_compose_bwd(p(comp), wp, p(dw), ra, nb, cols, p(dweight), p(dcomp), p(ws), nbytes - short, st)
        assert rc == (-2 if short else -1) and msg in lib.gmlm_last_error(), (ra, nb, cols, off, short, lib.gmlm_last_error())
        torch.cuda.synchronize()
        assert all(bool((t_ == sent).all()) for t_ in (w, dweight, dcomp)), "a refused call wrote"
