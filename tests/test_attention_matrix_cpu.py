"""Coverage guard of the attention dispatch matrix (no GPU needed): the attention kernels compiled into the library's gfx950
code objects must be exactly the kernels that tests/test_gpu_attention_matrix.py runs against float64 (``CASES``) plus
those it lists as unreachable (``UNREACHABLE``).  A new instantiation without a parity case, or a stale table entry, fails
here, by name."""
import os
import re
import shutil
import subprocess
import tempfile

import pytest
import torch

from gmlm_amd import _lib
from helpers import _bare_kernel_name
from test_gpu_attention_matrix import CASES, UNREACHABLE, _is_attention
from test_wgrad_cpu import LLVM, _code_objects


def _compiled_kernels(keep):
    """Bare template ids of the project's kernels for which ``keep(name)`` holds and that have a kernel descriptor (.kd) in a
    device code object of the built library; the host part of the .so (launch stubs) is not read."""
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libgmlm_hip.so not built")
    if not all(os.path.exists(os.path.join(LLVM, t)) for t in ("llvm-readelf", "llvm-objcopy")):
        pytest.skip("ROCm llvm tools not found")
    tmp = tempfile.mkdtemp()
    try:
        names = set()
        for co in _code_objects(_lib.LIB_PATH, tmp):
            syms = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--syms", "--wide", co], check=True, capture_output=True,
                                  text=True).stdout
            for line in syms.splitlines():
                f = line.split()
                if f and f[-1].endswith(".kd") and f[-1].startswith("_ZN4gmlm"):
                    names.add(_bare_kernel_name(torch._C._demangle(f[-1][:-3])))
        return {n for n in names if keep(n)}
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def test_every_attention_instantiation_has_a_parity_case_or_a_reason():
    compiled = _compiled_kernels(_is_attention)
    run = set().union(*(c.fwd | c.bwd for c in CASES))
    listed = run | set(UNREACHABLE)
    assert compiled, "no attention kernel found in the code objects"
    assert not sorted(compiled - listed), f"compiled but neither in CASES nor in UNREACHABLE: {sorted(compiled - listed)}"
    assert not sorted(listed - compiled), f"listed but not compiled: {sorted(listed - compiled)}"
    assert not sorted(run & set(UNREACHABLE)), f"both run by a case and listed as unreachable: {sorted(run & set(UNREACHABLE))}"


def test_every_dropout_template_runs_both_ways():
    """Each reachable kernel with a DROP template parameter runs in CASES with dropout and without."""
    run = set().union(*(c.fwd | c.bwd for c in CASES))
    for n in run:
        for a, b in ((", true", ", false"), (", false", ", true")):
            if a in n:
                assert n.replace(a, b) in run, (n, "its other dropout variant has no case")


def test_case_table_is_consistent():
    ids = [c.id for c in CASES]
    assert len(ids) == len(set(ids))
    for c in CASES:
        assert c.mode in ("pad", "kvlen", "packed", "groups") and c.layout in ("contig", "fused"), c.id
        assert all(_is_attention(n) for n in c.fwd | c.bwd), c.id
        assert (c.p > 0) == any(", true" in n for n in c.fwd | c.bwd), c.id
        if c.mode == "kvlen":
            assert len(c.lens) == c.b, c.id
        if c.mode in ("packed", "groups"):
            assert len(c.lens) == c.b and sum(c.lens) == c.lq == c.lk, c.id
        if c.layout == "fused":
            assert c.lq == c.lk and c.mode in ("pad", "kvlen"), c.id


def test_streaming_dq_mfma_chains_stay_per_key_block():
    """attn_dq_body (attn_stream.hpp) runs, per 32-key block of a tile, one extra contraction step for the scores, one for dP
    (without dropout), D/16 steps each for S^T and dP^T and 2 * D/32 for dQ^T.  The bf16 d = 64 / 96 dQ kernels must hold
    exactly that many v_mfma: one fewer means the key blocks were fused into one scheduling region (the dP start step is then
    shared), which costs the d = 64 kernels a wave per SIMD.  (d128::dq_kernel is its own text and not counted here.)"""
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libgmlm_hip.so not built")
    if not all(os.path.exists(os.path.join(LLVM, t)) for t in ("llvm-objdump", "llvm-objcopy")):
        pytest.skip("ROCm llvm tools not found")
    tmp = tempfile.mkdtemp()
    try:
        seen = 0
        for co in _code_objects(_lib.LIB_PATH, tmp):
            dis = subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-d", "--mcpu=gfx950", co], check=True, capture_output=True,
                                 text=True).stdout
            for m in re.finditer(r"^[0-9a-f]+ <_ZN4gmlm18attn_bwd_dq_kernelItLi(\d+)ELi(\d)ELb([01])EEEvNS_10AttnParamsE>:\n(.*?)(?=^[0-9a-f]+ <|\Z)",
                                 dis, re.S | re.M):
                d, nw, drop = int(m.group(1)), int(m.group(2)), m.group(3) == "1"
                kb = 4 if nw == 8 else 2                                   # 128-key tiles at 8 waves, else 64
                want = kb * ((1 if drop else 2) + 2 * (d // 16) + 2 * (d // 32))
                assert m.group(4).count("v_mfma_") == want, (d, nw, drop, m.group(4).count("v_mfma_"), want)
                seen += 1
        assert seen == 12, seen                                            # {64, 96} x {2, 4, 8 waves} x {plain, dropout}
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
