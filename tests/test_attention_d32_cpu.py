"""Host side of the head-dim-32 attention (no GPU needed): the fourth header (include/gmlm_hip_d32.h), its ctypes table and
the exported symbols agree type by type; the entry points decide every documented refusal, the workspace boundary and the
nothing-to-do cases before any launch; the ``d32::`` kernels of the built code objects are exactly those that
tests/test_gpu_attention_d32.py runs against float64, none of them with a private segment (spill) or packed-fp32 VALU; and
the model layer routes a head-dim-32 encoder to the packed pass while other head dims below 64 keep the padded one."""
import os
import re
import shutil
import subprocess
import tempfile

import pytest
import torch

from conftest import ROOT
from gmlm_amd import _lib
from test_abi_contract_cpu import parse_header, signature_mismatches
from test_attention_matrix_cpu import _compiled_kernels
from test_gpu_attention_d32 import CASES, UNREACHABLE, _is_d32
from test_wgrad_cpu import LLVM, _code_objects

OK, EINVAL, EWORKSPACE, ELAUNCH = 0, -1, -2, -3
F32, BF16 = 0, 1
A = 0x10000000        # fabricated, non-null, 16-byte aligned: every call below ends before or at the launch

no_device = pytest.mark.skipif(torch.cuda.device_count() > 0,
                               reason="fabricated addresses: only meaningful (and only safe) without a device")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libgmlm_hip.so not built")
    return _lib.lib()


# ------------------------------------------------------------------------------------------------------------------ ABI
def test_header_ctypes_table_and_exports_agree(lib):
    protos = parse_header(open(os.path.join(ROOT, "include", "gmlm_hip_d32.h")).read())
    assert sorted(protos) == ["gmlm_attention_d32_bwd", "gmlm_attention_d32_bwd_workspace_bytes", "gmlm_attention_d32_fwd"]
    assert not signature_mismatches(protos, _lib.SIGNATURES_D32)
    for name in protos:
        assert hasattr(lib, name), f"{name} declared in include/gmlm_hip_d32.h but not exported"
    assert not set(_lib.SIGNATURES_D32) & (set(_lib.SIGNATURES) | set(_lib.SIGNATURES_SPLIT) | set(_lib.SIGNATURES_OPTIM))


_BASE = dict(q=A, k=A, v=A, kv_len=None, b=1, h=12, lq=64, lk=64, d=32, q_stride=384, k_stride=384, v_stride=384, scale=0.177,
             dropout_p=0.0, seed=1, seed_dev=None, out=A, out_lo=None, lse=A, dtype=BF16, cu_seqlens=None, max_len=0, stream=None,
             dout=A, dq=A, dk=A, dv=A, dq_stride=384, dk_stride=384, dv_stride=384, workspace=A, workspace_bytes=1 << 40)
_FWD = ("q k v kv_len b h lq lk d q_stride k_stride v_stride scale dropout_p seed seed_dev out out_lo lse dtype cu_seqlens max_len "
        "stream").split()
_BWD = ("q k v out dout lse kv_len b h lq lk d q_stride k_stride v_stride scale dropout_p seed seed_dev dq dk dv dq_stride dk_stride "
        "dv_stride dtype cu_seqlens max_len workspace workspace_bytes out_lo stream").split()


def _call(lib, which, **mut):
    a = dict(_BASE, **mut)
    fn, names = (lib.gmlm_attention_d32_fwd, _FWD) if which == "fwd" else (lib.gmlm_attention_d32_bwd, _BWD)
    return fn(*[a[n] for n in names]), lib.gmlm_last_error()


def test_argument_lists_follow_the_header():
    protos = parse_header(open(os.path.join(ROOT, "include", "gmlm_hip_d32.h")).read())
    assert [n for _, n in protos["gmlm_attention_d32_fwd"][1]] == _FWD
    assert [n for _, n in protos["gmlm_attention_d32_bwd"][1]] == _BWD


_REFUSALS = [
    (dict(d=64), b"head dim"), (dict(d=96), b"head dim"), (dict(d=128), b"head dim"), (dict(d=16), b"head dim"),
    (dict(dtype=2), b"dtype"), (dict(dtype=-1), b"dtype"),
    (dict(dropout_p=1.0), b"[0,1)"), (dict(dropout_p=-0.1), b"[0,1)"),
    (dict(scale=0.0), b"scale"), (dict(scale=-1.0), b"scale"),
    (dict(b=-1), b"bad sizes"), (dict(h=0), b"bad sizes"), (dict(lq=-1), b"bad sizes"),
    (dict(q_stride=380), b"stride"),                                    # below h * 32
    (dict(q_stride=388), b"stride"),                                    # bf16: not a multiple of 8 elements
    (dict(dtype=F32, k_stride=386), b"stride"),                         # fp32: not a multiple of 4 elements
    (dict(v_stride=1 << 24), b"stride"),
    (dict(q=A + 8), b"aligned"), (dict(k=None), b"null"), (dict(v=A + 4, dtype=F32), b"aligned"),
    (dict(cu_seqlens=A, max_len=64, lk=65), b"packed mode"),            # lq != lk
    (dict(cu_seqlens=A, max_len=0), b"packed mode"),
    (dict(cu_seqlens=A, max_len=64, kv_len=A), b"packed mode"),
    (dict(out_lo=A, dtype=F32), b"out_lo"), (dict(out_lo=A + 8), b"out_lo"),
    (dict(b=1 << 27, h=16, lq=1, lk=1), b"too many work items"),        # 2^31 work items of one 32-row tile
    (dict(b=(1 << 31) // 12 + 1, lq=1, lk=1), b"too many work items"),
]


@no_device
@pytest.mark.parametrize("which", ["fwd", "bwd"])
@pytest.mark.parametrize("mut,msg", _REFUSALS, ids=[",".join(f"{k}={v}" for k, v in m.items()) for m, _ in _REFUSALS])
def test_refusals_are_decided_on_the_host(lib, which, mut, msg):
    rc, err = _call(lib, which, **mut)
    assert rc == EINVAL and msg in err, (mut, rc, err)


@no_device
def test_valid_calls_reach_the_launch(lib):
    """Without a device a call that passes validation ends in GMLM_ELAUNCH: the baseline, both layouts, both dtypes, the
    largest admissible grid, and a gradient stride of a fused buffer."""
    for which in ("fwd", "bwd"):
        for mut in (dict(), dict(dtype=F32), dict(cu_seqlens=A, max_len=64), dict(kv_len=A), dict(out_lo=A), dict(lq=70, lk=200),
                    dict(b=(1 << 31) // 12 - 1, lq=1, lk=1), dict(q_stride=1152, k_stride=1152, v_stride=1152, dq_stride=1152)):
            rc, err = _call(lib, which, **mut)
            assert rc == ELAUNCH, (which, mut, rc, err)


@no_device
def test_backward_only_refusals(lib):
    for mut, msg in ((dict(dq_stride=380), b"dq"), (dict(dk=A + 8), b"dk"), (dict(dv=None), b"dv"), (dict(dout=None), b"out/dout/lse"),
                     (dict(lse=None), b"out/dout/lse"), (dict(lq=0), b"empty query or key set"), (dict(lk=0), b"empty query or key set")):
        rc, err = _call(lib, "bwd", **mut)
        assert rc == EINVAL and msg in err, (mut, rc, err)


@no_device
def test_workspace_boundary(lib):
    need = lib.gmlm_attention_d32_bwd_workspace_bytes(2, 12, 300)
    assert need == 2 * 12 * 300 * 4
    assert lib.gmlm_attention_d32_bwd_workspace_bytes(0, 12, 0) > 0                      # an empty problem still has a size
    shape = dict(b=2, lq=300, lk=300)
    assert _call(lib, "bwd", workspace_bytes=need, **shape)[0] == ELAUNCH
    rc, err = _call(lib, "bwd", workspace_bytes=need - 1, **shape)
    assert rc == EWORKSPACE and b"workspace" in err
    assert _call(lib, "bwd", workspace=None, **shape)[0] == EWORKSPACE
    # packed: delta is [h, total_rows] whatever the number of sequences
    packed = dict(b=7, lq=300, lk=300, cu_seqlens=A, max_len=100)
    need = lib.gmlm_attention_d32_bwd_workspace_bytes(1, 12, 300)
    assert _call(lib, "bwd", workspace_bytes=need, **packed)[0] == ELAUNCH
    assert _call(lib, "bwd", workspace_bytes=need - 1, **packed)[0] == EWORKSPACE


@no_device
def test_nothing_to_do_needs_no_pointer_but_sizes_are_still_checked(lib):
    nothing = dict(q=None, k=None, v=None, out=None, lse=None, dout=None, dq=None, dk=None, dv=None, workspace=None, workspace_bytes=0)
    for empty in (dict(b=0), dict(lq=0, lk=0), dict(lq=0, lk=0, cu_seqlens=A, max_len=1)):
        for which in ("fwd", "bwd"):
            assert _call(lib, which, **nothing, **empty)[0] == OK, (which, empty)
            rc, err = _call(lib, which, **nothing, **empty, d=64)
            assert rc == EINVAL and b"head dim" in err
    assert _call(lib, "fwd", **nothing, lq=0)[0] == OK                                   # the forward has no query row to write


@no_device
def test_existing_entry_points_keep_refusing_head_dim_32(lib):
    rc = lib.gmlm_attention_fwd(None, None, None, None, 1, 12, 16, 16, 32, 384, 384, 384, 1.0, 0.0, 0, None, None, None, None, 0,
                                None, 0, None, 0, None)
    assert rc == EINVAL and b"head dim" in lib.gmlm_last_error()
    rc = lib.gmlm_attention_d128_fwd(A, A, A, None, 1, 12, 16, 16, 32, 384, 384, 384, 1.0, 0.0, 0, None, A, None, A, 1, None)
    assert rc == EINVAL and b"head dim" in lib.gmlm_last_error()


# --------------------------------------------------------------------------------------------------------- code objects
def test_every_d32_instantiation_has_a_parity_case_or_a_reason():
    compiled = _compiled_kernels(_is_d32)
    run = set().union(*(c.fwd | c.bwd for c in CASES))
    listed = run | set(UNREACHABLE)
    assert len(compiled) == 38, sorted(compiled)           # {fwd, dq, dkv} x {bf16, fp32} x {1, 2, 4 waves} x {plain, dropout} + 2 delta
    assert not sorted(compiled - listed), f"compiled but neither in CASES nor in UNREACHABLE: {sorted(compiled - listed)}"
    assert not sorted(listed - compiled), f"listed but not compiled: {sorted(listed - compiled)}"
    assert not run & set(UNREACHABLE)
    for c in CASES:
        assert (c.p > 0) == any(", true>" in n for n in c.fwd | c.bwd), c.id
        if c.mode == "packed":
            assert len(c.lens) == c.b and sum(c.lens) == c.lq == c.lk, c.id


def test_case_table_sits_on_both_sides_of_the_height_thresholds():
    """rows = max(lq, lk) padded / max_len packed: 32 and 33, 128 and 129, in both layouts, with the height the rule gives."""
    seen = set()
    for c in CASES:
        rows = max(c.lens) if c.mode == "packed" else max(c.lq, c.lk)
        nw = 1 if rows <= 32 else (2 if rows <= 128 else 4)
        assert all(f", {nw}, " in n for n in c.fwd | c.bwd if "delta" not in n), c.id
        seen.add((c.mode == "packed", rows))
    for packed in (False, True):
        assert {(packed, r) for r in (32, 33, 128)} <= seen, sorted(seen)
    assert (False, 129) in seen and any(p and r > 128 for p, r in seen)


def test_d32_kernels_have_no_private_segment_and_no_packed_fp32():
    """No spill (a zero private segment in every kernel's metadata) and no packed-fp32 VALU (DESIGN.md section 5 b)."""
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libgmlm_hip.so not built")
    if not all(os.path.exists(os.path.join(LLVM, t)) for t in ("llvm-readelf", "llvm-objdump", "llvm-objcopy")):
        pytest.skip("ROCm llvm tools not found")
    tmp = tempfile.mkdtemp()
    try:
        private, bodies = {}, {}
        for co in _code_objects(_lib.LIB_PATH, tmp):
            notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", co], check=True, capture_output=True, text=True).stdout
            for m in re.finditer(r"\.name:\s+(_ZN4gmlm3d32\w+)\s+\.private_segment_fixed_size:\s+(\d+)", notes):
                private[m.group(1)] = int(m.group(2))
            dis = subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-d", "--mcpu=gfx950", co], check=True, capture_output=True,
                                 text=True).stdout
            for m in re.finditer(r"^[0-9a-f]+ <(_ZN4gmlm3d32\w+)>:\n(.*?)(?=^[0-9a-f]+ <|\Z)", dis, re.S | re.M):
                bodies[m.group(1)] = m.group(2)
        assert len(private) == 38 and set(private) == set(bodies), (sorted(private), sorted(bodies))
        assert not {n: v for n, v in private.items() if v}, private
        for name, body in bodies.items():
            assert "v_mfma" in body or "delta_kernel" in name, name
            for op in ("v_pk_fma_f32", "v_pk_mul_f32", "v_pk_add_f32"):
                assert op not in body, (name, op)
            assert "scratch_" not in body, name
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


# --------------------------------------------------------------------------------------------------------- host routing
def _model(hidden, heads):
    import gmlm_amd
    from transformers import BertConfig, BertModel
    enc = BertModel(BertConfig(vocab_size=50, hidden_size=hidden, num_hidden_layers=1, num_attention_heads=heads,
                               intermediate_size=2 * hidden, max_position_embeddings=32))
    return gmlm_amd.GraphTextLM(8, 8, 3, plm_encoder=enc)


def test_model_routes_head_dim_32_to_the_packed_pass(monkeypatch):
    from gmlm_amd import bert
    assert bert.NATIVE_HEAD_DIMS == (32, 64, 96)
    m32, m16 = _model(384, 12), _model(64, 4)
    assert m32._packed_head_dim() == 32 and m32.plm_packed and m32._has_packed_pass()
    assert m16._packed_head_dim() == 16 and not m16._has_packed_pass()
    monkeypatch.setattr(bert, "NATIVE_HEAD_DIMS", (64, 96))              # the old route
    assert not m32._has_packed_pass()


def test_packed_pass_refuses_other_small_head_dims():
    from gmlm_amd import bert
    m16 = _model(64, 4)
    z = torch.zeros(4, dtype=torch.long)
    with pytest.raises(NotImplementedError, match="head dim"):
        bert.bert_encode_packed(m16.plm_encoder, z, z, torch.tensor([0, 4], dtype=torch.int32), 4, torch.float32)


def test_ops_fail_loudly_at_head_dim_32_without_a_gpu(lib):
    """No eager fallback: on CPU tensors the d = 32 route raises the library's error, not a head-dim refusal."""
    from gmlm_amd import ops
    q = torch.zeros(1, 4, 2 * 32)
    with pytest.raises((_lib.GmlmHipError, ValueError, RuntimeError)) as e:
        ops.Attention.apply(q, q, q, None, 2, 32 ** -0.5, 0.0, 0)
    assert "head dim" not in str(e.value)
