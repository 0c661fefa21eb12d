"""Coverage guard of the norm / row-op dispatch matrix (no GPU needed): the GraphNorm, LayerNorm, bias+GELU, mean-pool,
soft-mask and embedding-sum kernels compiled into the library's gfx950 code objects (with the column reductions over
ColStatsFn, GraphNormBwdStatsFn and SoftmaskBwdFn) must be exactly the kernels that tests/test_gpu_norm_matrix.py runs against
float64 (``CASES``) plus those it lists as unreachable (``UNREACHABLE``)."""
import torch

from helpers import elem_dropout_scale
from test_attention_matrix_cpu import _compiled_kernels
from test_gpu_norm_matrix import CASES, UNREACHABLE, _is_norm_family


def test_every_norm_instantiation_has_a_parity_case_or_a_reason():
    compiled = _compiled_kernels(_is_norm_family)
    run = {n for c in CASES for n in c.fwd | c.bwd if _is_norm_family(n)}
    listed = run | set(UNREACHABLE)
    assert compiled, "no norm / row-op kernel found in the code objects"
    assert not sorted(compiled - listed), f"compiled but neither in CASES nor in UNREACHABLE: {sorted(compiled - listed)}"
    assert not sorted(listed - compiled), f"listed but not compiled: {sorted(listed - compiled)}"
    assert not sorted(run & set(UNREACHABLE)), f"both run by a case and listed as unreachable: {sorted(run & set(UNREACHABLE))}"
    ln_fwd = [n for n in UNREACHABLE if n.startswith("ln_fwd_kernel<")]
    ln_bwd = [n for n in UNREACHABLE if n.startswith("ln_bwd_kernel<")]
    assert (len(ln_fwd), len(ln_bwd), len(UNREACHABLE)) == (8, 40, 48)


def test_every_dropout_template_runs_both_ways():
    """Each reachable kernel with a DROP template parameter runs in CASES with dropout and without: LayerNorm backward
    <T, CH, LPR, ACT, DROP, RES>, bias+GELU <T, DROP>."""
    run = set().union(*(c.fwd | c.bwd for c in CASES))
    drop = [n for n in run if n.startswith(("ln_bwd_kernel<", "bias_gelu_"))]
    assert drop
    for n in drop:
        args = n[n.index("<") + 1:-1].split(", ")
        i = 4 if n.startswith("ln_bwd") else 1
        other = args[:i] + [{"true": "false", "false": "true"}[args[i]]] + args[i + 1:]
        assert n[:n.index("<") + 1] + ", ".join(other) + ">" in run, (n, "its other dropout variant has no case")


def test_case_table_is_consistent():
    ids = [c.id for c in CASES]
    assert len(ids) == len(set(ids))
    for c in CASES:
        assert c.op in ("ln", "gn", "bg", "pool", "softmask", "embed"), c.id
        assert all(_is_norm_family(n) or n in ("rows_sum_kernel", "zero_words_kernel") for n in c.fwd | c.bwd), c.id
        drop = [n for n in c.fwd | c.bwd if n.startswith(("ln_bwd_kernel<", "bias_gelu_"))]
        for n in drop:
            args = n[n.index("<") + 1:-1].split(", ")
            assert (c.p > 0) == (args[4 if n.startswith("ln_bwd") else 1] == "true"), c.id
        if c.op == "ln" and c.rows:
            assert c.f % (4 if c.dtype == torch.float32 else 8) == 0 and c.f <= 1024, c.id


def test_elem_dropout_scale_rules():
    """The restated mask: one hash word per element pair (idx >> 1), the half picked by idx & 1, 16-bit threshold
    lround(p * 65536) clamped to 65535, fp32 keep scale; the high words of the offset and of the seed both take part."""
    idx = torch.arange(1 << 16, dtype=torch.int64)
    m = elem_dropout_scale(12345, idx, 0.25)
    assert m.dtype == torch.float32 and set(m.unique().tolist()) == {0.0, float(torch.tensor(65536.0 / 49152.0))}
    assert abs(float((m > 0).float().mean()) - 0.75) < 0.01
    assert not torch.equal(elem_dropout_scale(12345, idx + (1 << 33), 0.25), m)
    assert not torch.equal(elem_dropout_scale(12345 + (0x12345678 << 32), idx, 0.25), m)
    assert bool((elem_dropout_scale(1, idx, 0.0) == 1).all())
    big = torch.arange(1 << 20, dtype=torch.int64)
    assert float(elem_dropout_scale(1, big, 0.99999).max()) == 65536.0           # th clamped to 65535: keep scale 65536

    def field(seed, i):                                   # common.hpp hash_u32 in plain Python integers, element i's half
        w, x = i >> 1, 0
        x = ((w & 0xFFFFFFFF) * 0x9E3779B1 + (w >> 32) * 0x85EBCA77 + (seed & 0xFFFFFFFF)) & 0xFFFFFFFF
        x ^= x >> 16
        x = (x * 0x7FEB352D) & 0xFFFFFFFF
        x ^= x >> 15
        x = (x * 0x846CA68B) & 0xFFFFFFFF
        x ^= x >> 16
        return ((x ^ (seed >> 32)) >> (16 * (i & 1))) & 0xFFFF

    offs = [0, 1, 2, 3, 2 ** 32 - 2, 2 ** 32 - 1, 2 ** 32, 2 ** 32 + 1, 7_700_000_001] + [(k * 2654435761) % 2 ** 40 for k in range(300)]
    for seed in (0x1234_5678_9ABC, 2 ** 32 + 2, 3):
        got = elem_dropout_scale(seed, torch.tensor(offs), 0.1).tolist()
        assert got == [float(torch.tensor(65536.0 / (65536 - 6554))) if field(seed, i) >= 6554 else 0.0 for i in offs], seed
