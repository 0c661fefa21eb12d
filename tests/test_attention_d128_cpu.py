"""Host side of the head-dim-128 attention (no GPU needed): the entry points reject bad arguments before any launch, the
existing entry points still refuse d = 128, the Python layer routes d = 128 and its neighbours to the new kernels, and a
disassembly screen of the built gfx950 code objects (no scratch traffic, no packed-fp32 VALU)."""
import os
import re
import shutil
import subprocess
import tempfile

import pytest
import torch

from gmlm_amd import _lib

LLVM = "/opt/rocm/llvm/bin"
A = 16           # a non-null, 16-byte aligned stand-in pointer: every case below is refused before it is dereferenced


def _lib_or_skip():
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libgmlm_hip.so not built")
    return _lib.lib()


def _fwd(lib, b=1, h=8, lq=64, lk=64, d=128, qs=1024, ks=1024, vs=1024, p=0.0, q=A, dtype=1):
    return lib.gmlm_attention_d128_fwd(q, A, A, None, b, h, lq, lk, d, qs, ks, vs, 0.088, p, 0, None, A, None, A, dtype, None)


def _bwd(lib, b=1, h=8, lq=64, lk=64, d=128, qs=1024, ks=1024, vs=1024, p=0.0, dqs=1024, ws_bytes=1 << 30, dtype=1):
    return lib.gmlm_attention_d128_bwd(A, A, A, A, None, A, A, None, b, h, lq, lk, d, qs, ks, vs, 0.088, p, 0, None, A, A, A, dqs,
                                       ks, vs, dtype, A, ws_bytes, None)


@pytest.mark.parametrize("call", [_fwd, _bwd])
@pytest.mark.parametrize("kw,msg", [
    (dict(d=96), b"head dim"),
    (dict(d=64), b"head dim"),
    (dict(p=1.0), b"dropout_p"),
    (dict(p=-0.1), b"dropout_p"),
    (dict(qs=1000), b"stride"),                                         # not a multiple of 8 bf16 elements
    (dict(qs=512), b"stride"),                                          # narrower than h * 128
    (dict(ks=1028), b"stride"),                                         # k: not a multiple of 8 bf16 elements
])
def test_entry_points_reject_bad_arguments_on_the_host(call, kw, msg):
    lib = _lib_or_skip()
    rc = call(lib, **kw)
    assert rc == -1, kw
    assert msg in lib.gmlm_last_error(), (kw, lib.gmlm_last_error())


def test_backward_rejects_a_bad_gradient_stride():
    lib = _lib_or_skip()
    assert _bwd(lib, dqs=1020) == -1 and b"dq" in lib.gmlm_last_error()


def test_backward_workspace_is_checked():
    lib = _lib_or_skip()
    need = lib.gmlm_attention_d128_workspace_bytes(2, 8, 300)
    assert need == 2 * 8 * 300 * 4
    assert _bwd(lib, b=2, lq=300, lk=300, ws_bytes=need - 1) == -2       # GMLM_EWORKSPACE
    assert b"workspace" in lib.gmlm_last_error()


def test_existing_entry_points_still_refuse_head_dim_128():
    lib = _lib_or_skip()
    rc = lib.gmlm_attention_fwd(None, None, None, None, 1, 8, 16, 16, 128, 1024, 1024, 1024, 1.0, 0.0, 0, None, None, None, None, 0,
                                None, 0, None, 0, None)
    assert rc == -1 and b"head dim" in lib.gmlm_last_error()


def test_python_dispatch_covers_head_dims_up_to_128():
    """attention_any_dim takes every head dim up to 128 (it used to raise above 96) and refuses wider ones; on CPU tensors
    the op fails loudly (no eager fallback) instead of raising NotImplementedError."""
    _lib_or_skip()
    from gmlm_amd import nn as gnn
    for d in (100, 128):
        q = torch.zeros(1, 4, 2 * d)
        with pytest.raises(_lib.GmlmHipError):
            gnn.attention_any_dim(q, q, q, None, 2, d ** -0.5, 0.0, False)
    q = torch.zeros(1, 4, 2 * 160)
    with pytest.raises(NotImplementedError):
        gnn.attention_any_dim(q, q, q, None, 2, 160 ** -0.5, 0.0, False)


def test_misaligned_pointer_is_refused():
    lib = _lib_or_skip()
    assert _fwd(lib, dtype=0, q=A + 4) == -1 and b"aligned" in lib.gmlm_last_error()


def test_ring_block_refuses_head_dim_128(monkeypatch):
    """The ring cross-attention (multi-GPU) has no d = 128 block: it says so instead of running something else.
    AttentionBlock.fwd checks the device first; the head-dim refusal is the next check, reached with that check stubbed."""
    from gmlm_amd import ops
    monkeypatch.setattr(ops, "_cuda", lambda *ts: None)
    q = torch.zeros(1, 4, 8 * 128)
    with pytest.raises(NotImplementedError, match="ring"):
        ops.AttentionBlock(8, 128 ** -0.5).fwd(q, q, q, None, 0)


def _code_objects(so, into):
    from test_wgrad_cpu import _code_objects as co
    return co(so, into)


def test_d128_kernels_disassembly():
    """No scratch (spill) traffic and no packed-fp32 VALU (DESIGN.md section 5 b) in any of attn_d128.hip's kernels."""
    _lib_or_skip()
    if not (os.path.exists(os.path.join(LLVM, "llvm-objdump")) and os.path.exists(os.path.join(LLVM, "llvm-objcopy"))):
        pytest.skip("ROCm llvm tools not found")
    tmp = tempfile.mkdtemp()
    try:
        bodies = {}
        for co in _code_objects(_lib.LIB_PATH, tmp):
            dis = subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-d", "--mcpu=gfx950", co], check=True, capture_output=True,
                                 text=True).stdout
            for m in re.finditer(r"^[0-9a-f]+ <(_ZN4gmlm4d128\w+)>:\n(.*?)(?=^[0-9a-f]+ <|\Z)", dis, re.S | re.M):
                bodies[m.group(1)] = m.group(2)
        names = sorted(bodies)
        for kern in ("fwd_kernel", "dq_kernel", "dkv_kernel"):
            assert sum(kern in n for n in names) == 4, (kern, names)    # {bf16, fp32} x {plain, dropout}
        assert sum("delta_kernel" in n for n in names) == 2, names
        for name, body in bodies.items():
            assert "v_mfma" in body or "delta_kernel" in name, name
            for op in ("v_pk_fma_f32", "v_pk_mul_f32", "v_pk_add_f32"):
                assert op not in body, (name, op)
            assert "scratch_" not in body and "buffer_store" not in body, name
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
