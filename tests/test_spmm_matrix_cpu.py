"""Coverage guard of the segment-reduction dispatch matrix (no GPU needed): the seg_reduce_* kernels compiled into the
library's gfx950 code objects must be exactly the kernels that tests/test_gpu_spmm_matrix.py runs against float64 (``CASES``)
plus those it lists as unreachable (``UNREACHABLE``), and every case's shape must lead launch_spmm (spmm_kernels.hip), restated
here, to the kernels the case names."""
import torch

from test_attention_matrix_cpu import _compiled_kernels
from test_gpu_spmm_matrix import CASES, THRESH, UNREACHABLE, _is_spmm_family, _kernels, _tn, _vec_width


def _named():
    return {n for c in CASES for n in c.kernels}


def test_every_spmm_instantiation_has_a_parity_case_or_a_reason():
    compiled = _compiled_kernels(_is_spmm_family)
    run = _named()
    listed = run | set(UNREACHABLE)
    assert compiled, "no seg_reduce_* kernel found in the code objects"
    assert not sorted(compiled - listed), f"compiled but neither in CASES nor in UNREACHABLE: {sorted(compiled - listed)}"
    assert not sorted(listed - compiled), f"listed but not compiled: {sorted(listed - compiled)}"
    assert not sorted(run & set(UNREACHABLE)), f"both run by a case and listed as unreachable: {sorted(run & set(UNREACHABLE))}"
    assert len(compiled) == 2 * 4 * 2 * 2 + 2 + 4 and not UNREACHABLE      # vec <T, CH, EDGE_W, MODE>, combine <T>, scalar <T, EDGE_W>


def test_every_edge_weight_and_mode_variant_runs_both_ways():
    """Each vector kernel <T, CH, EDGE_W, MODE> named in CASES has its other EDGE_W and its other MODE variant there too, and
    each scalar kernel <T, EDGE_W> its other EDGE_W variant."""
    run = _named()
    flip = {"true": "false", "false": "true", "0": "1", "1": "0"}
    seen = 0
    for n in run:
        if n.startswith("seg_reduce_combine_kernel<"):
            continue
        args = n[n.index("<") + 1:-1].split(", ")
        for i in ((2, 3) if n.startswith("seg_reduce_vec_kernel<") else (1,)):
            other = args[:i] + [flip[args[i]]] + args[i + 1:]
            assert n[:n.index("<") + 1] + ", ".join(other) + ">" in run, (n, f"its other variant of template argument {i} has no case")
            seen += 1
    assert seen


def _launch_spmm_choice(c):
    """launch_spmm restated: (path, ntile, chunks per tile, L, CH) for the case's dtype, width, source size and layout."""
    v, esize = _vec_width(c.dtype), 2 if c.dtype == torch.bfloat16 else 4
    off, stride = {"contig": (0, c.f), "slice": (2 * v, c.f + 3 * v), "odd": (1, c.f + v), "stride": (0, c.f + 1)}[c.layout]
    out_stride = c.f + c.out_pad
    # torch allocations are 16-byte aligned (and far beyond): the pointers' alignment is that of the column offset
    vec_ok = c.f % v == 0 and stride % v == 0 and out_stride % v == 0 and (off * esize) % 16 == 0
    if not vec_ok:
        return "scalar", -(-c.f // 512), 0, 0, 0
    f_chunks = c.f // v
    ntile = 8 if c.src_rows * c.f * esize <= (24 << 20) and f_chunks >= 64 else 1
    cpt = -(-f_chunks // ntile)
    while cpt > 256:
        ntile *= 2
        cpt = -(-f_chunks // ntile)
    ntile = -(-f_chunks // cpt)
    log2_l = 0
    while (1 << log2_l) < cpt and log2_l < 6:
        log2_l += 1
    lanes = 1 << log2_l
    ch = -(-cpt // lanes)
    return "vec", ntile, cpt, lanes, (ch if ch <= 3 else 4)


def test_case_table_is_consistent():
    ids = [c.id for c in CASES]
    assert len(ids) == len(set(ids))
    for c in CASES:
        assert all(_is_spmm_family(n) for n in c.kernels), c.id
        assert c.plan in ("", "host", "device") and c.layout in ("contig", "slice", "odd", "stride"), c.id
        if c.nseg == 0:
            assert c.path == "none" and not c.kernels, c.id
            continue
        assert c.nseg >= 17, c.id                                       # the fixed part of the segment layout and the empty tail
        path, ntile, cpt, lanes, ch = _launch_spmm_choice(c)
        assert path == c.path, (c.id, path)
        split = bool(c.plan) and path == "vec"
        if path == "vec":
            assert (ntile, lanes, ch) == (c.ntile, c.lanes, c.ch), (c.id, ntile, cpt, lanes, ch)
            assert cpt <= 256 and ch * lanes >= cpt, c.id
        assert c.kernels == _kernels(_tn(c.dtype), path, ch, c.edge_w, split), c.id
        mode1 = {n for n in c.kernels if n.endswith(", 1>") or n.startswith("seg_reduce_combine_kernel<")}
        if path == "scalar":
            assert not mode1 and all(n.startswith("seg_reduce_scalar_kernel<") for n in c.kernels), c.id
        elif split:
            assert len(mode1) == 2 and len(c.kernels) == 3, c.id
        else:
            assert not mode1 and len(c.kernels) == 1, c.id
        if c.ints:
            assert not c.mean and not c.edge_w, c.id
        if c.twice:
            assert split, c.id


def test_named_geometries_are_met():
    """The properties the table is there for, from the restated dispatch: a ragged last column tile, tile doubling from 8 and
    from 1 tile, the grid cap crossed at L = 64, sources above 24 MiB, the scalar path handed a split plan, strided operands,
    an exactness case per dtype with and without MODE 1, and a twice-launched split case per dtype."""
    for dtype in (torch.float32, torch.bfloat16):
        mine = [c for c in CASES if c.dtype == dtype and c.nseg]
        geo = {c.id: _launch_spmm_choice(c) for c in mine}
        vecs = [c for c in mine if c.path == "vec"]
        assert any(c.f // _vec_width(dtype) % geo[c.id][2] for c in vecs if geo[c.id][1] == 8), "no ragged last tile"
        assert any(geo[c.id][1] == 16 for c in vecs), "no tile doubling"
        # cap = 256 * 16 / ntile blocks of 256 / L groups
        assert any(geo[c.id][3] == 64 and -(-c.nseg // 4) > 256 * 16 // geo[c.id][1] for c in vecs), "grid cap not crossed at L = 64"
        assert {geo[c.id][4] for c in vecs} == {1, 2, 3, 4}
        assert {geo[c.id][3] for c in vecs} >= {1, 2, 8, 16, 64}
        assert any(c.path == "scalar" and c.plan for c in mine), "scalar path never handed a split plan"
        assert any(c.path == "scalar" and c.f > 512 and c.f % 512 for c in mine)
        assert {c.layout for c in mine if c.path == "scalar"} >= {"contig", "odd", "stride"}
        assert any(c.layout == "slice" for c in vecs) and any(c.out_pad for c in vecs)
        assert any(c.ints and c.plan for c in vecs) and any(c.ints and not c.plan for c in vecs)
        assert any(c.twice for c in vecs)
        assert {c.plan for c in vecs} == {"", "host", "device"}
        assert any(not c.edges for c in mine)
    big = [c for c in CASES if c.src_rows * c.f * (2 if c.dtype == torch.bfloat16 else 4) > (24 << 20)]
    assert {(c.dtype, c.f, _launch_spmm_choice(c)[1], _launch_spmm_choice(c)[4]) for c in big} == {
        (torch.float32, 768, 1, 3), (torch.bfloat16, 768, 1, 2), (torch.float32, 1024, 1, 4), (torch.float32, 1028, 2, 3)}
    assert THRESH == 64
