"""Coverage guard of the graph-build and basis-composition matrix (no GPU needed): the graph kernels and basis_compose_*
kernels compiled into the library's gfx950 code objects must be exactly the kernels that tests/test_gpu_graph_basis_matrix.py
names in ``GRAPH_CASES`` and ``BASIS_CASES`` (plus ``UNREACHABLE``, empty); grid_cap, basis_blocks and the radix sort's
``end_bit`` (graph_kernels.hip, basis_kernels.hip, common.hpp), restated here, must give every case the trips, groups and
blocks its docstring claims; gmlm_split_plan_capacity (host only) must hold every plan of the split-plan layouts and of a
random sweep; and the refusals that are decided before any launch are repeated on the host."""
import ctypes
import os
import shutil
import subprocess
import tempfile

import numpy as np
import pytest
import torch

import gmlm_oracle as O
from gmlm_amd import _lib
from test_attention_matrix_cpu import _compiled_kernels
from test_wgrad_cpu import LLVM, _code_objects
from test_gpu_graph_basis_matrix import (BASIS_CASES, BUCKET, DEG, END_BIT_NSEG, FWD, G32, G64, GRAPH_CASES, GRAPH_KERNEL_NAMES, HIST,
                                         I2F, INV, KEYS, ROWPTR, ROWS_SUM, SPLIT, SPLIT_LAYOUTS, SPLIT_NSEG, THRESH, UNREACHABLE, ZERO,
                                         _REFUSALS, _is_graph_or_basis, bwd, dcomp_depth, split_layout)


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    import gmlm_amd
    return gmlm_amd.lib()


def _named():
    run = set().union(*(c.kernels for c in GRAPH_CASES.values()), *(c.fwd | c.bwd for c in BASIS_CASES))
    return {n for n in run if _is_graph_or_basis(n)}


# ------------------------------------------------------------------------------------------------ 1. compiled == named
def test_every_graph_and_basis_kernel_has_a_case_or_a_reason():
    compiled = _compiled_kernels(_is_graph_or_basis)
    run = _named()
    listed = run | set(UNREACHABLE)
    assert compiled, "no graph or basis kernel found in the code objects"
    assert not sorted(compiled - listed), f"compiled but neither in the case tables nor in UNREACHABLE: {sorted(compiled - listed)}"
    assert not sorted(listed - compiled), f"listed but not compiled: {sorted(listed - compiled)}"
    assert not sorted(run & set(UNREACHABLE)), f"both run by a case and listed as unreachable: {sorted(run & set(UNREACHABLE))}"
    graph = {n for n in compiled if not n.startswith("basis_compose_")}
    # ten graph kernels, gather_kernel<long> and <int>; basis_compose_fwd_kernel and basis_compose_bwd_kernel<1..5>
    assert len(GRAPH_KERNEL_NAMES) == 10 and len(graph) == 11 and len(compiled - graph) == 6 and not UNREACHABLE
    assert compiled - graph == {FWD} | {bwd(ra) for ra in (1, 2, 3, 4, 5)}


def test_no_project_kernel_lives_outside_the_namespace():
    """helpers.kernels_run and _compiled_kernels see ``gmlm::`` kernels only: a kernel defined after the namespace is closed
    (split_plan_kernel was) is invisible to every name assertion and to every coverage guard.  Every kernel descriptor of the
    code objects must be the project's, in ``gmlm::``, or rocPRIM's."""
    _compiled_kernels(lambda n: True)                            # skips where the library or the llvm tools are missing
    tmp = tempfile.mkdtemp()
    try:
        foreign = set()
        for co in _code_objects(_lib.LIB_PATH, tmp):
            syms = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--syms", "--wide", co], check=True, capture_output=True,
                                  text=True).stdout
            for line in syms.splitlines():
                f = line.split()
                if f and f[-1].endswith(".kd") and not f[-1].startswith("_ZN4gmlm"):
                    foreign.add(torch._C._demangle(f[-1][:-3]))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    strays = sorted(n for n in foreign if "rocprim::" not in n.split("(")[0])
    assert not strays, f"kernels outside gmlm:: (kernels_run cannot see them): {strays}"


def test_case_tables_are_complete():
    """The cases the matrix consists of, by name: dropping one fails here even where another case names the same kernels."""
    assert list(GRAPH_CASES) == ["second_trip", "hot_node", "bucket_boundaries", "hist_r64", "hist_r1", "hist_rejects", "end_bit",
                                 "null_keys", "flagged_ids", "no_edges", "split_plan"]
    assert [c.id for c in BASIS_CASES] == [
        "ra1_nb30_c8192", "ra2_nb30_c8192", "ra3_nb30_c8192", "ra4_nb30_c8192", "ra5_nb30_c8192", "ra2_nb1_c4", "ra3_nb5_c1020",
        "ra4_nb6_c1024", "ra5_nb7_c1028", "ra5_nb31_c4096", "ra5_nb32_stride", "ra2_nb12_stride3", "exact_ra5_nb32_stride",
        "exact_ra2_nb12_stride3", "exact_ra5_nb7_c1028", "fallback_nb33", "fallback_c6"]
    assert END_BIT_NSEG == (1, 2, 1024, 1025, 65536, 65537) and SPLIT_NSEG == (1, 1023, 1024, 1025, 200_000)
    assert SPLIT_LAYOUTS == ("none_long", "one_segment", "exact_lengths", "all_65", "clustered") and THRESH == 64
    assert [(ra, nb, cols, off, short) for ra, nb, cols, off, short, _ in _REFUSALS] == [
        (0, 30, 1024, 0, 0), (6, 30, 1024, 0, 0), (3, 0, 1024, 0, 0), (3, 33, 1024, 0, 0), (3, 30, 0, 0, 0), (3, 30, 6, 0, 0),
        (3, 30, 1024, 4, 0), (3, 30, 1024, 0, 4)]
    second = GRAPH_CASES["second_trip"]
    assert second.kernels == {ZERO, DEG, I2F, BUCKET, HIST, KEYS, ROWPTR, G64, G32, INV, SPLIT}, "not every graph kernel is named"
    assert KEYS not in GRAPH_CASES["hist_rejects"].kernels and HIST in GRAPH_CASES["hist_rejects"].kernels
    assert GRAPH_CASES["no_edges"].kernels == {ZERO, INV}
    assert G32 not in GRAPH_CASES["null_keys"].call("null_keys") and G32 in GRAPH_CASES["null_keys"].call("with_keys")
    assert DEG not in GRAPH_CASES["bucket_boundaries"].call("build") and BUCKET in GRAPH_CASES["bucket_boundaries"].call("build")
    for c in GRAPH_CASES.values():
        assert c.kernels and all(_is_graph_or_basis(n) for n in c.kernels), c.id


# ------------------------------------------------------------------------------------------------- 2. restated dispatch
def cdiv(a, b):
    return (a + b - 1) // b


def grid_cap(blocks, cap=2048):
    return 1 if blocks < 1 else min(blocks, cap)


def basis_blocks(cols):
    return max(1, min(2048, cdiv(cols // 4, 256)))


def end_bit(num_segments):
    b = 1
    while b < 32 and (1 << b) < num_segments:
        b += 1
    return b


def test_graph_cases_stride_as_claimed():
    c = GRAPH_CASES["second_trip"]
    strided = {s.kernel for s in c.strides}
    # every graph kernel with a grid-stride loop: all but the zero fill (not the family's subject) and the one-block plan kernel
    assert strided == c.kernels - {ZERO, SPLIT}
    caps = {HIST: 1024}
    for s in c.strides:
        assert s.cap == caps.get(s.kernel, 2048), s
        blocks = grid_cap(cdiv(s.n, 256), s.cap)
        assert blocks == s.cap and cdiv(s.n, 256) > s.cap, (s, "the grid is not capped")
        assert cdiv(s.n, blocks * 256) == s.trips and s.trips >= 2, (s, cdiv(s.n, blocks * 256))
    assert {s.kernel: s.trips for s in c.strides}[HIST] == 3


def test_end_bit_and_split_ranges_sit_on_their_boundaries():
    assert [end_bit(n) for n in END_BIT_NSEG] == [1, 1, 10, 11, 16, 17]
    for n in END_BIT_NSEG:                                       # the keys 0 .. n - 1 fit, and one bit fewer would not (n > 2)
        assert (1 << end_bit(n)) >= n and (n <= 2 or (1 << (end_bit(n) - 1)) < n)
    per = [cdiv(n, 1024) for n in SPLIT_NSEG]
    assert per == [1, 1, 1, 2, 196]
    idle = [1024 - cdiv(n, p) for n, p in zip(SPLIT_NSEG, per)]  # threads that own no segment
    assert idle == [1023, 1, 0, 511, 3]
    assert 1025 - 512 * 2 == 1                                   # nseg = 1025: the last owning thread has one segment


def test_basis_cases_meet_their_geometry():
    for c in BASIS_CASES:
        nch = c.cols // 4
        assert basis_blocks(c.cols) == c.blocks, (c.id, basis_blocks(c.cols))
        if not c.hip:
            assert c.nb > 32 or c.ra > 5 or c.cols % 4, c.id      # nn._BasisCompose's own condition
            assert not c.fwd and not c.bwd, c.id
            continue
        assert 1 <= c.ra <= 5 and 1 <= c.nb <= 32 and c.cols % 4 == 0 and c.cols > 0, c.id
        assert (c.nb % 6, nch % 256) == (c.nb_mod, c.nch_mod), (c.id, c.nb % 6, nch % 256)
        threads = c.blocks * 256
        # thread 0 makes the most passes, the last thread with a chunk the fewest
        trips = {cdiv(nch, threads), cdiv(nch - (min(nch, threads) - 1), threads)}
        assert trips == set(c.trips), (c.id, trips)
        assert (max(c.trips) > 1) == (cdiv(nch, 256) > 2048), c.id
        assert c.fwd == {FWD} and c.bwd == {bwd(c.ra), ROWS_SUM}, c.id
        assert dcomp_depth(c.cols, c.blocks) == 5 * max(c.trips) + 6 + 2 + cdiv(c.blocks, 8) + 3, c.id
    hip = [c for c in BASIS_CASES if c.hip]
    assert {c.ra for c in hip if c.nb == 30 and c.cols == 8192} == {1, 2, 3, 4, 5}
    assert {c.nb_mod for c in hip} >= {0, 1, 2, 5} and any(c.nb < 6 for c in hip) and any(c.nb == 6 for c in hip)
    assert any(c.nb == 32 and c.ra == 5 for c in hip), "kMaxRB never full"
    assert any(c.cols == 4 for c in hip) and any(c.nch_mod == 255 for c in hip) and any(c.cols == 1024 for c in hip)
    shape = lambda c: (c.ra, c.nb, c.cols)
    strided = {shape(c) for c in hip if max(c.trips) > 1 and not c.ints}
    assert {c.trips for c in hip if max(c.trips) > 1} == {(1, 2), (2, 3)}
    assert {shape(c) for c in hip if c.ints} == strided | {(5, 7, 1028)}
    for c in hip:
        if c.ints:                                                # every partial sum stays an exact fp32 integer
            assert c.cols < 2 ** 24 and c.nb < 2 ** 24
    assert {shape(c) for c in BASIS_CASES if not c.hip} == {(3, 33, 1024), (2, 5, 6)}
    # 259 chunks of the strided rows lie behind the first pass of the capped grid
    assert all(c.cols // 4 % (2048 * 256) == 259 for c in hip if max(c.trips) > 1)


# ------------------------------------------------------------------------------------------------- 3. capacity formula
def _capacity(lib, items, thresh):
    cl, cc = ctypes.c_int64(), ctypes.c_int64()
    assert lib.gmlm_split_plan_capacity(int(items), int(thresh), ctypes.byref(cl), ctypes.byref(cc)) == 0
    return cl.value, cc.value


def _plan_counts(lens, thresh):
    rowptr = np.concatenate([[0], np.cumsum(lens)])
    long_seg, chunk_ptr, owner = O.split_plan(rowptr, thresh)
    assert int(chunk_ptr[-1]) == owner.size
    return int(rowptr[-1]), long_seg.size, owner.size


def test_split_plan_capacity_holds_every_plan(lib):
    """``always true for capacities from gmlm_split_plan_capacity`` (split_plan_kernel): n_long <= cap_long and
    n_chunks <= cap_chunks for the GPU test's layouts and for 200 random length multisets at thresh 1, 2, 64 and 256.  Both
    capacities are at least 1: ops.device_split_plan allocates them with torch, whose empty tensor has a NULL pointer, which
    gmlm_split_plan_build refuses."""
    seen = 0
    for nseg in SPLIT_NSEG:
        for layout in SPLIT_LAYOUTS:
            items, nl, nc = _plan_counts(split_layout(layout, nseg), THRESH)
            cl, cc = _capacity(lib, items, THRESH)
            assert nl <= cl and nc <= cc and cl >= 1 and cc >= 1, (nseg, layout, items, nl, cl, nc, cc)
            assert cl <= 65535, (nseg, layout, "gmlm_split_plan_build would refuse this layout")
            seen += nl > 0
    assert seen == len(SPLIT_NSEG) * (len(SPLIT_LAYOUTS) - 1)
    rng = np.random.default_rng(20240611)
    for i in range(200):
        t = (1, 2, 64, 256)[i % 4]
        nseg = int(rng.integers(1, 400))
        edge = np.array([0, 1, t - 1, t, t + 1, 2 * t - 1, 2 * t, 2 * t + 1, 3 * t + 1, 7 * t, 7 * t + 1])
        lens = np.where(rng.random(nseg) < 0.5, edge[rng.integers(0, edge.size, nseg)], rng.integers(0, 5 * t + 2, nseg))
        if i % 10 == 0:
            lens[:] = t + 1
        if i % 10 == 1:
            lens[:] = 0
        items, nl, nc = _plan_counts(lens, t)
        cl, cc = _capacity(lib, items, t)
        assert nl <= cl and nc <= cc and cl >= 1 and cc >= 1, (i, t, items, nl, cl, nc, cc)


@pytest.mark.parametrize("thresh", [1, 2, 64, 256])
def test_split_plan_capacity_is_tight(lib, thresh):
    """All segments of length thresh + 1 hold the most long segments (and two chunks each) an item count allows.  With k such
    segments cap_long = k + k / thresh + 1 and cap_chunks = 2 k + 2 (k / thresh) + 1: both within one of what is needed for
    k < thresh; beyond that the slack is the k / thresh of dividing the item count by thresh and not by thresh + 1, which is
    exactly what the formula is held to here - a capacity that over-allocates by a factor fails."""
    for k in (0, 1, thresh - 1, thresh, 3 * thresh + 1, 1000):
        items, nl, nc = _plan_counts(np.full(k, thresh + 1, dtype=np.int64), thresh)
        assert (items, nl, nc) == (k * (thresh + 1), k, 2 * k)
        cl, cc = _capacity(lib, items, thresh)
        assert 0 <= cl - nl - k // thresh <= 1 and 0 <= cc - nc - 2 * (k // thresh) <= 1, (thresh, k, nl, cl, nc, cc)
        if k < thresh:
            assert 0 <= cl - nl <= 1 and 0 <= cc - nc <= 1 and cl >= 1, (thresh, k, nl, cl, nc, cc)


# ------------------------------------------------------------------------------------------------- 4. host-side refusals
def _host(nbytes):
    """A 16-byte aligned address inside a host buffer (kept alive by the caller): the calls below are refused before any launch
    and never read or write through it."""
    raw = ctypes.create_string_buffer(nbytes + 32)
    return raw, (ctypes.addressof(raw) + 15) & ~15


def test_refusals_decided_before_any_launch(lib):
    """Every refusal of the GPU file that the entry points decide from their arguments alone.  The geometry checks of the basis
    entry points come before their pointer checks, so those calls pass NULL; the alignment, workspace and capacity refusals come
    after a null check and get addresses of host memory, which a refused call never touches."""
    for ra, nb, cols, off, short, msg in _REFUSALS:
        if off or short:
            continue
        rc = lib.gmlm_basis_compose_fwd(None, None, ra, nb, cols, None, None)
        assert rc == -1 and msg in lib.gmlm_last_error(), (ra, nb, cols, lib.gmlm_last_error())
        rc = lib.gmlm_basis_compose_bwd(None, None, None, ra, nb, cols, None, None, None, 0, None)
        assert rc == -1 and msg in lib.gmlm_last_error(), (ra, nb, cols, lib.gmlm_last_error())
    keep, a = _host(256)
    ra, nb, cols = 3, 30, 1024
    msgs = {(off, short): msg for r, n, c, off, short, msg in _REFUSALS if off or short}
    rc = lib.gmlm_basis_compose_fwd(a, a + 4, ra, nb, cols, a, None)
    assert rc == -1 and msgs[(4, 0)] in lib.gmlm_last_error()
    rc = lib.gmlm_basis_compose_bwd(a, a + 4, a, ra, nb, cols, a, a, a, 1 << 20, None)
    assert rc == -1 and msgs[(4, 0)] in lib.gmlm_last_error()
    need = lib.gmlm_basis_compose_bwd_workspace_bytes(ra, nb, cols)
    assert need == basis_blocks(cols) * ra * nb * 4
    rc = lib.gmlm_basis_compose_bwd(a, a, a, ra, nb, cols, a, a, a, need - 4, None)
    assert rc == -2 and msgs[(0, 4)] in lib.gmlm_last_error()

    e = 3001
    need = lib.gmlm_segment_sort_workspace_bytes(e)
    assert need >= 3 * 4 * e
    rc = lib.gmlm_segment_sort(a, None, None, 1, e, 40, None, a, a, a, a, need - 1, None)
    assert rc == -2 and b"workspace too small" in lib.gmlm_last_error()

    items = 65535 * THRESH
    rc = lib.gmlm_split_plan_build(a, 1, items, THRESH, a, a, a, None)
    assert rc == -1 and b"long_threshold" in lib.gmlm_last_error()
    assert _capacity(lib, items, THRESH)[0] == 65536 and _capacity(lib, items - 1, THRESH)[0] == 65535
    del keep
