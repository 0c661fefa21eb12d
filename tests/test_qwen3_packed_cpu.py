"""Host side of the packed (variable-length) Qwen3 pass (no GPU needed): the argument checks of the varlen causal attention and
the rotary-embedding-by-position entry points, the new operators on CPU tensors, the cu / pos tables the model hands to
``qwen3.qwen3_encode_packed``, and a disassembly screen of the rotary kernels that carry the position form."""
import os
import re
import shutil
import subprocess
import tempfile

import pytest
import torch

from gmlm_amd import _lib
from test_qwen3_cpu import LLVM, A, _bare, _code_objects, _lib_or_skip, _tiny_model

CU = 32          # stand-in cu_seqlens pointer; refused calls never read it


# ---- varlen causal attention entry points ----------------------------------------------------------
def _fwd(lib, cu=CU, seqs=3, max_len=64, rows=100, hq=4, hkv=2, d=128, qs=512, ks=256, vs=256, p=0.0, q=A, dtype=1):
    return lib.gmlm_attention_causal_d128_varlen_fwd(q, A, A, cu, seqs, max_len, rows, hq, hkv, d, qs, ks, vs, 0.088, p, A, None, A,
                                                     dtype, None)


def _bwd(lib, cu=CU, seqs=3, max_len=64, rows=100, hq=4, hkv=2, d=128, qs=512, ks=256, vs=256, p=0.0, q=A, dqs=512, dks=256,
         ws_bytes=1 << 30, dtype=1):
    return lib.gmlm_attention_causal_d128_varlen_bwd(q, A, A, A, None, A, A, cu, seqs, max_len, rows, hq, hkv, d, qs, ks, vs, 0.088, p,
                                                     A, A, A, dqs, dks, vs, dtype, A, ws_bytes, None)


@pytest.mark.parametrize("call", [_fwd, _bwd])
@pytest.mark.parametrize("kw,msg", [
    (dict(cu=None), b"cu_seqlens"),
    (dict(max_len=0), b"max_len"),
    (dict(max_len=-5), b"max_len"),
    (dict(d=64), b"head dim"),
    (dict(d=96), b"head dim"),
    (dict(hq=4, hkv=3, ks=384, vs=384), b"multiple of"),
    (dict(p=0.1), b"dropout"),
    (dict(rows=1 << 30), b"2^30"),
    (dict(seqs=1 << 20, max_len=1 << 20), b"work items"),
    (dict(q=A + 4, dtype=0), b"aligned"),
    (dict(qs=504), b"stride"),                                          # narrower than hq * 128
    (dict(qs=516), b"stride"),                                          # not a multiple of 8 bf16 elements
    (dict(ks=128), b"stride"),                                          # narrower than hkv * 128
])
def test_varlen_entry_points_reject_bad_arguments_on_the_host(call, kw, msg):
    lib = _lib_or_skip()
    rc = call(lib, **kw)
    assert rc == -1, kw
    assert msg in lib.gmlm_last_error(), (kw, lib.gmlm_last_error())


def test_varlen_backward_rejects_bad_gradient_strides_and_a_short_workspace():
    lib = _lib_or_skip()
    assert _bwd(lib, dqs=500) == -1 and b"dq" in lib.gmlm_last_error()
    assert _bwd(lib, dks=128) == -1 and b"dk" in lib.gmlm_last_error()
    need = lib.gmlm_attention_causal_d128_varlen_workspace_bytes(835, 4)
    assert need == 4 * 835 * 4                                           # delta: fp32 [hq, T]
    assert _bwd(lib, rows=835, ws_bytes=need - 1) == -2                  # GMLM_EWORKSPACE
    assert b"workspace" in lib.gmlm_last_error()


def test_varlen_signatures_have_no_kv_len():
    """A packed sequence's length is its row count: the varlen entry points take cu_seqlens and no kv_len."""
    header = open(os.path.join(os.path.dirname(_lib.__file__), "..", "include", "gmlm_hip.h")).read()
    for name in ("gmlm_attention_causal_d128_varlen_fwd", "gmlm_attention_causal_d128_varlen_bwd"):
        decl = re.search(r"int " + name + r"\(([^;]*)\);", header).group(1)
        assert "cu_seqlens" in decl and "max_len" in decl and "kv_len" not in decl, decl


# ---- rotary embedding by position ------------------------------------------------------------------
def test_rope_by_position_entry_points_reject_bad_arguments_on_the_host():
    lib = _lib_or_skip()

    def fwd(pos=A, stride=1024, max_len=64, d=128):
        return lib.gmlm_qknorm_rope_pos_fwd(A, stride, A, A, A, max_len, 8, pos, 4, 2, d, 1e-6, A, 768, A, 1, None)

    def bwd(pos=A, stride=1024, max_len=64, d=128, ws=1 << 20):
        return lib.gmlm_qknorm_rope_pos_bwd(A, 1024, A, stride, A, A, A, max_len, A, 8, pos, 4, 2, d, 1024, 1024 + 512, 1, A, ws, None)

    for call in (fwd, bwd):
        assert call(pos=None) == -1 and b"pos_ids" in lib.gmlm_last_error()
        assert call(d=64) == -1 and b"head dim" in lib.gmlm_last_error()
        assert call(stride=768) == -1 and b"stride" in lib.gmlm_last_error()
        assert call(max_len=0) == -1 and b"table" in lib.gmlm_last_error()
    assert bwd(ws=8) == -2 and b"workspace" in lib.gmlm_last_error()


# ---- operators -------------------------------------------------------------------------------------
def test_new_varlen_ops_fail_loudly_without_a_gpu():
    _lib_or_skip()
    from gmlm_amd import ops
    x = torch.zeros(6, 1024)
    cu = torch.tensor([0, 2, 6], dtype=torch.int32)
    pos = torch.tensor([0, 1, 0, 1, 2, 3])
    with pytest.raises(_lib.GmlmHipError):
        ops.causal_attention_varlen(x[:, :512], x[:, 512:768], x[:, 768:], cu, 4, 4, 2, 0.088)
    with pytest.raises(_lib.GmlmHipError):
        ops.rope_causal_attention_varlen(x, torch.ones(128), torch.ones(128), torch.zeros(4, 2, 64), pos, cu, 4, 4, 2, 0.088)
    with pytest.raises(_lib.GmlmHipError):
        ops.qknorm_rope(x, torch.ones(128), torch.ones(128), torch.zeros(4, 2, 64), 4, 2, pos_ids=pos)


# ---- model wiring ----------------------------------------------------------------------------------
class _Stop(Exception):
    pass


def _drive(model, tokens, mask, batch, monkeypatch):
    from gmlm_amd import qwen3
    seen = []

    def stub(plm, tok, pos, cu, max_len, cd, training, checkpointing, weights):
        seen.append((tok.clone(), pos.clone(), cu.clone(), max_len))
        raise _Stop

    monkeypatch.setattr(qwen3, "qwen3_encode_packed", stub)
    with pytest.raises(_Stop):
        model.encode_texts(tokens, mask, plm_batch_size=batch)
    return seen


def test_packed_route_hands_the_encoder_the_expected_tables(monkeypatch):
    """Five nodes, four active with 3, 1, 4 and 2 tokens: one batch, sequences sorted by length (longest first), tokens back
    to back, positions restarting at every sequence, cu their running sum; no dummy sequence below 4,096 rows."""
    from gmlm_amd import qwen3
    from gmlm_amd.model import TokenizedTexts
    model, _ = _tiny_model()
    assert model.plm_packed and model._has_packed_pass() and model._packed_head_dim() == 0
    ids = torch.tensor([[11, 12, 13, 0], [21, 0, 0, 0], [31, 32, 0, 0], [41, 42, 43, 44], [51, 52, 0, 0]])
    am = (ids > 0).long()
    mask = torch.tensor([True, True, False, True, True])
    tokens = TokenizedTexts.from_mask(ids, am)
    seen = _drive(model, tokens, mask, 8, monkeypatch)
    assert len(seen) == 1
    tok, pos, cu, max_len = seen[0]
    assert tok.tolist() == [41, 42, 43, 44, 11, 12, 13, 51, 52, 21]
    assert pos.tolist() == [0, 1, 2, 3, 0, 1, 2, 0, 1, 0]
    assert cu.dtype == torch.int32 and cu.tolist() == [0, 4, 7, 9, 10] and max_len == 4

    # micro-batches of two: each batch its own tables
    calls = []

    def stub(plm, tok, pos, cu, max_len, *a):
        calls.append((tok.tolist(), pos.tolist(), cu.tolist(), max_len))
        return torch.zeros(tok.numel(), plm.config.hidden_size)

    monkeypatch.setattr(qwen3, "qwen3_encode_packed", stub)
    from gmlm_amd import ops
    monkeypatch.setattr(ops.MeanPoolScatter, "apply", staticmethod(lambda out, hs, lens, idx, cu=None, rows=None: out))
    model.encode_texts(tokens, mask, plm_batch_size=2)
    assert calls == [([41, 42, 43, 44, 11, 12, 13], [0, 1, 2, 3, 0, 1, 2], [0, 4, 7], 4), ([51, 52, 21], [0, 1, 0], [0, 2, 3], 2)]


def test_plm_packed_false_keeps_the_padded_pass(monkeypatch):
    from gmlm_amd import qwen3
    from gmlm_amd.model import TokenizedTexts
    model, _ = _tiny_model()
    model.plm_packed = False
    ids = torch.tensor([[11, 12, 13], [21, 0, 0]])
    tokens = TokenizedTexts.from_mask(ids, (ids > 0).long())

    def padded(plm, input_ids, lens, *a):
        assert tuple(input_ids.shape) == (2, 3) and lens.tolist() == [3, 1]
        raise _Stop

    monkeypatch.setattr(qwen3, "qwen3_encode", padded)
    monkeypatch.setattr(qwen3, "qwen3_encode_packed", lambda *a, **k: pytest.fail("packed route taken"))
    with pytest.raises(_Stop):
        model.encode_texts(tokens, torch.tensor([True, True]), plm_batch_size=8)


def test_bert_only_forms_still_exclude_qwen3(monkeypatch):
    """plm_bucketed (the bucketed static layout) is a BERT form: a Qwen3 model takes its plain packed pass instead; the
    encoder cannot be recorded."""
    from gmlm_amd.model import TokenizedTexts
    model, _ = _tiny_model()
    model.plm_bucketed = True
    ids = torch.tensor([[11, 12, 13], [21, 0, 0]])
    tokens = TokenizedTexts.from_mask(ids, (ids > 0).long())
    seen = _drive(model, tokens, torch.tensor([True, True]), 8, monkeypatch)
    assert seen[0][2].tolist() == [0, 3, 4]
    with pytest.raises(NotImplementedError, match="BERT"):
        model.capture_hip_graphs(torch.zeros(4, 12), torch.zeros(2, 4, dtype=torch.long), encoder=True)


def test_packed_encoder_refuses_a_sequence_past_max_position_embeddings():
    from gmlm_amd import qwen3
    _, plm = _tiny_model(max_position_embeddings=16)
    t = torch.zeros(17, dtype=torch.long)
    with pytest.raises(ValueError, match="max_position_embeddings"):
        qwen3.qwen3_encode_packed(plm, t, torch.arange(17), torch.tensor([0, 17], dtype=torch.int32), 17, torch.float32)


# ---- code objects ----------------------------------------------------------------------------------
def test_rope_kernels_with_the_position_form_disassembly():
    """The qknorm_rope_* kernels now read their table row either by row % seq_len or by pos_ids: both element types of both
    kernels exist, and none has scratch (spill) traffic or packed-fp32 VALU (DESIGN.md section 5 b)."""
    _lib_or_skip()
    if not (os.path.exists(os.path.join(LLVM, "llvm-objdump")) and os.path.exists(os.path.join(LLVM, "llvm-objcopy"))):
        pytest.skip("ROCm llvm tools not found")
    tmp = tempfile.mkdtemp()
    try:
        bodies = {}
        for co in _code_objects(_lib.LIB_PATH, tmp):
            dis = subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-d", "--mcpu=gfx950", co], check=True, capture_output=True,
                                 text=True).stdout
            for m in re.finditer(r"^[0-9a-f]+ <(_ZN4gmlm\w+)>:\n(.*?)(?=^[0-9a-f]+ <|\Z)", dis, re.S | re.M):
                name = _bare(m.group(1))
                if name.startswith("qknorm_rope_"):
                    bodies[name] = m.group(2)
        assert set(bodies) == {f"qknorm_rope_{k}_kernel<{t}>" for k in ("fwd", "bwd") for t in ("unsigned short", "float")}, sorted(bodies)
        for name, body in bodies.items():
            assert not re.search(r"v_pk_\w+_f32", body), (name, re.findall(r"v_pk_\w+_f32", body)[:3])
            assert "scratch_" not in body, name
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
