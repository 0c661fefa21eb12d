"""Host side of the Qwen3 text encoder (no GPU needed): which configs ``qwen3.check_supported`` takes, the host-side argument
checks of the causal attention and row-kernel entry points, left- / right-padded token tables, the head dim the model reads
from the config, and a disassembly screen of the new gfx950 kernels (no scratch traffic, no packed-fp32 VALU)."""
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


def _cfg(**kw):
    from transformers import Qwen3Config
    base = dict(vocab_size=96, hidden_size=256, intermediate_size=384, num_hidden_layers=2, num_attention_heads=4,
                num_key_value_heads=2, head_dim=128, max_position_embeddings=512, tie_word_embeddings=False)
    base.update(kw)
    return Qwen3Config(**base)


class _Holder:
    def __init__(self, config):
        self.config = config


# ---- check_supported ---------------------------------------------------------------------------
def test_check_supported_accepts_a_qwen3_config():
    from gmlm_amd import qwen3
    qwen3.check_supported(_Holder(_cfg()))
    assert qwen3.head_dim(_cfg()) == 128


def _rope_kw(rope_type):
    """A non-default rope type in the spelling the installed transformers takes: ``rope_parameters`` where the config class
    has that field, else ``rope_scaling``.  The config must then carry the type where HF's rotary embedding reads it."""
    if hasattr(_cfg(), "rope_parameters"):
        kw, read = dict(rope_parameters={"rope_type": rope_type, "factor": 2.0, "rope_theta": 1e6}), "rope_parameters"
    else:
        kw, read = dict(rope_scaling={"rope_type": rope_type, "factor": 2.0}), "rope_scaling"
    assert getattr(_cfg(**kw), read)["rope_type"] == rope_type
    return kw


@pytest.mark.parametrize("kw,word", [
    (dict(use_sliding_window=True, sliding_window=64, max_window_layers=1), "sliding"),
    (dict(attention_dropout=0.1), "attention_dropout"),
    ("rope", "rope type"),
    (dict(head_dim=64), "head_dim=64"),
    (dict(hidden_act="gelu"), "hidden_act='gelu'"),
    (dict(attention_bias=True), "attention_bias"),
])
def test_check_supported_lists_each_problem(kw, word):
    from gmlm_amd import qwen3
    if kw == "rope":
        kw = _rope_kw("linear")
    with pytest.raises(NotImplementedError) as e:
        qwen3.check_supported(_Holder(_cfg(**kw)))
    assert word in str(e.value), str(e.value)


def test_check_supported_lists_every_problem_at_once():
    from gmlm_amd import qwen3
    with pytest.raises(NotImplementedError) as e:
        qwen3.check_supported(_Holder(_cfg(head_dim=64, hidden_act="gelu", attention_dropout=0.2)))
    for word in ("head_dim=64", "hidden_act", "attention_dropout"):
        assert word in str(e.value)


def test_bert_module_still_refuses_qwen3():
    from gmlm_amd import bert
    with pytest.raises(NotImplementedError):
        bert.check_supported(_Holder(_cfg()))


# ---- causal attention entry points ---------------------------------------------------------------
def _fwd(lib, b=1, hq=4, hkv=2, lq=64, lk=64, d=128, qs=512, ks=256, vs=256, p=0.0, q=A, dtype=1):
    return lib.gmlm_attention_causal_d128_fwd(q, A, A, None, b, hq, hkv, lq, lk, d, qs, ks, vs, 0.088, p, A, None, A, dtype, None)


def _bwd(lib, b=1, hq=4, hkv=2, lq=64, lk=64, d=128, qs=512, ks=256, vs=256, p=0.0, q=A, dqs=512, dks=256, ws_bytes=1 << 30, dtype=1):
    return lib.gmlm_attention_causal_d128_bwd(q, A, A, A, None, A, A, None, b, hq, hkv, lq, lk, d, qs, ks, vs, 0.088, p, A, A, A, dqs,
                                              dks, vs, dtype, A, ws_bytes, None)


@pytest.mark.parametrize("call", [_fwd, _bwd])
@pytest.mark.parametrize("kw,msg", [
    (dict(lk=65), b"lq == lk"),
    (dict(hq=4, hkv=3, ks=384, vs=384), b"multiple of"),
    (dict(d=64), b"head dim"),
    (dict(d=96), b"head dim"),
    (dict(p=0.1), b"dropout"),
    (dict(q=A + 4, dtype=0), b"aligned"),
    (dict(qs=504), b"stride"),                                          # narrower than hq * 128
    (dict(qs=516), b"stride"),                                          # not a multiple of 8 bf16 elements
    (dict(ks=128), b"stride"),                                          # narrower than hkv * 128
])
def test_causal_entry_points_reject_bad_arguments_on_the_host(call, kw, msg):
    lib = _lib_or_skip()
    rc = call(lib, **kw)
    assert rc == -1, kw
    assert msg in lib.gmlm_last_error(), (kw, lib.gmlm_last_error())


def test_causal_backward_rejects_bad_gradient_strides():
    lib = _lib_or_skip()
    assert _bwd(lib, dqs=500) == -1 and b"dq" in lib.gmlm_last_error()
    assert _bwd(lib, dks=128) == -1 and b"dk" in lib.gmlm_last_error()


def test_causal_backward_workspace_is_checked():
    lib = _lib_or_skip()
    need = lib.gmlm_attention_causal_d128_workspace_bytes(2, 4, 300)
    assert need == 2 * 4 * 300 * 4
    assert _bwd(lib, b=2, lq=300, lk=300, ws_bytes=need - 1) == -2       # GMLM_EWORKSPACE
    assert b"workspace" in lib.gmlm_last_error()


def test_existing_attention_entry_points_keep_their_refusals():
    lib = _lib_or_skip()
    rc = lib.gmlm_attention_fwd(None, None, None, None, 1, 8, 16, 16, 128, 1024, 1024, 1024, 1.0, 0.0, 0, None, None, None, None, 0,
                                None, 0, None, 0, None)
    assert rc == -1 and b"head dim" in lib.gmlm_last_error()
    rc = lib.gmlm_attention_d128_fwd(A, A, A, None, 1, 8, 64, 64, 64, 1024, 1024, 1024, 0.088, 0.0, 0, None, A, None, A, 1, None)
    assert rc == -1 and b"head dim" in lib.gmlm_last_error()


# ---- row-kernel entry points ---------------------------------------------------------------------
def test_row_kernel_entry_points_reject_bad_arguments_on_the_host():
    lib = _lib_or_skip()
    assert lib.gmlm_add_rmsnorm_fwd(A, None, A, 4, 1028, 1e-6, None, A, A, 1, None) == -1 and b"multiple of 8" in lib.gmlm_last_error()
    assert lib.gmlm_add_rmsnorm_fwd(A, None, A, 4, 8192, 1e-6, None, A, A, 1, None) == -1 and b"4096" in lib.gmlm_last_error()
    assert lib.gmlm_add_rmsnorm_fwd(A, A, A, 4, 1024, 1e-6, None, A, A, 1, None) == -1      # b without s
    assert lib.gmlm_add_rmsnorm_fwd(A + 2, None, A, 4, 1024, 1e-6, None, A, A, 1, None) == -1 and b"aligned" in lib.gmlm_last_error()
    assert lib.gmlm_add_rmsnorm_bwd(A, None, A, A, A, 64, 1024, A, A, 1, A, 8, None) == -2   # workspace
    rope = lambda **k: lib.gmlm_qknorm_rope_fwd(A, k.get("stride", 1024), A, A, A, k.get("max_len", 64), 8, k.get("l", 8), 4, 2,
                                                k.get("d", 128), 1e-6, A, 768, A, 1, None)
    assert rope(d=64) == -1 and b"head dim" in lib.gmlm_last_error()
    assert rope(stride=768) == -1 and b"stride" in lib.gmlm_last_error()
    assert rope(l=128) == -1 and b"table" in lib.gmlm_last_error()
    assert lib.gmlm_qknorm_rope_bwd(A, 1024, A, 1024, A, A, A, 64, A, 8, 8, 4, 2, 128, 1024, 1024 + 512, 1, A, 8, None) == -2
    assert lib.gmlm_swiglu_fwd(A, 4, 100, A, 1, None) == -1 and b"multiple of 8" in lib.gmlm_last_error()
    assert lib.gmlm_swiglu_bwd(A, A + 8, 4, 384, A, 1, None) == -1 and b"aligned" in lib.gmlm_last_error()


def test_new_ops_fail_loudly_without_a_gpu():
    """CPU tensors raise the library's error: no eager fallback behind the new operators."""
    _lib_or_skip()
    from gmlm_amd import ops
    x = torch.zeros(1, 4, 1024)
    with pytest.raises(_lib.GmlmHipError):
        ops.add_rmsnorm(x, None, torch.ones(1024))
    with pytest.raises(_lib.GmlmHipError):
        ops.swiglu(x)
    with pytest.raises(_lib.GmlmHipError):
        ops.causal_attention(x[..., :512], x[..., :256], x[..., :256], None, 4, 2, 0.088)
    with pytest.raises(_lib.GmlmHipError):
        ops.qknorm_rope(x, torch.ones(128), torch.ones(128), torch.zeros(4, 2, 64), 4, 2)


# ---- token tables ----------------------------------------------------------------------------------
def test_from_mask_left_right_and_unpadded_rows_agree():
    from gmlm_amd.model import TokenizedTexts
    g = torch.Generator().manual_seed(0)
    lens = [1, 3, 7, 5, 7]
    width = 7
    rows = [torch.randint(1, 90, (n,), generator=g) for n in lens]
    right = torch.zeros(len(lens), width, dtype=torch.long)
    left = torch.full((len(lens), width), 95, dtype=torch.long)             # a pad id that is not 0: it must not survive
    mixed = torch.zeros(len(lens), width, dtype=torch.long)
    am_r, am_l, am_m = (torch.zeros(len(lens), width, dtype=torch.long) for _ in range(3))
    for i, (r, n) in enumerate(zip(rows, lens)):
        right[i, :n], am_r[i, :n] = r, 1
        left[i, width - n:], am_l[i, width - n:] = r, 1
        if i % 2:
            mixed[i, :n], am_m[i, :n] = r, 1
        else:
            mixed[i, width - n:], am_m[i, width - n:] = r, 1
    want = TokenizedTexts.from_mask(right, am_r)
    assert want.lens.tolist() == lens
    for ids, am in ((left, am_l), (mixed, am_m)):
        got = TokenizedTexts.from_mask(ids, am)
        assert torch.equal(got.lens, want.lens)
        assert torch.equal(got.input_ids, want.input_ids)
    unpadded = TokenizedTexts.from_mask(right[2:3], am_r[2:3])              # a full row: nothing to move
    assert torch.equal(unpadded.input_ids, want.input_ids[2:3]) and unpadded.lens.tolist() == [7]


# ---- model wiring --------------------------------------------------------------------------------
def _tiny_model(**kw):
    import gmlm_amd
    from transformers import Qwen3Model
    torch.manual_seed(0)
    plm = Qwen3Model(_cfg(**kw))
    return gmlm_amd.GraphTextLM(12, 16, 3, plm_encoder=plm, plm_tokenizer=None), plm


def test_head_dim_comes_from_the_config_not_from_hidden_over_heads():
    """hidden 256 / 4 heads = 64 would be the packed d = 64 route of the BERT encoder; the config says head_dim 128."""
    from gmlm_amd import bert, qwen3
    model, plm = _tiny_model()
    assert plm.config.hidden_size // plm.config.num_attention_heads == 64
    assert qwen3.head_dim(plm.config) == 128
    assert model._enc is qwen3 and model._packed_head_dim() == 0         # no packed / short-sequence / whole-step route
    with pytest.raises(NotImplementedError, match="BERT"):
        model.capture_hip_graphs(torch.zeros(4, 12), torch.zeros(2, 4, dtype=torch.long))
    lws = qwen3.prepare_weights(plm, torch.float32)
    assert tuple(lws[0].wqkv.shape) == ((4 + 2 * 2) * 128, 256) and tuple(lws[0].wgu.shape) == (2 * 384, 256)
    assert tuple(lws[0].wo.shape) == (256, 512) and tuple(lws[0].wdown.shape) == (256, 384)
    sa = plm.layers[0].self_attn
    assert torch.equal(lws[0].wqkv, torch.cat([sa.q_proj.weight, sa.k_proj.weight, sa.v_proj.weight]))
    assert torch.equal(lws[1].wgu, torch.cat([plm.layers[1].mlp.gate_proj.weight, plm.layers[1].mlp.up_proj.weight]))
    assert model._enc is not bert


def test_state_dict_keys_are_those_of_the_hf_module():
    model, plm = _tiny_model()
    keys = {k[len("plm_encoder."):] for k in model.state_dict() if k.startswith("plm_encoder.")}
    assert keys == set(plm.state_dict())
    assert "layers.0.self_attn.q_norm.weight" in keys and "embed_tokens.weight" in keys


def test_rope_table_matches_the_hf_rotary_embedding():
    from gmlm_amd import qwen3
    from transformers.models.qwen3.modeling_qwen3 import Qwen3RotaryEmbedding
    cfg = _cfg(rope_parameters={"rope_type": "default", "rope_theta": 1e6}) if hasattr(_cfg(), "rope_parameters") else _cfg(rope_theta=1e6)
    cs = qwen3.rope_table(cfg, 40, "cpu")
    cos, sin = Qwen3RotaryEmbedding(cfg)(torch.zeros(1, 40, 8), torch.arange(40)[None])
    assert cs.shape[0] >= 40 and tuple(cs.shape[1:]) == (2, 64) and cs.dtype == torch.float32
    assert qwen3.rope_table(cfg, 17, "cpu") is cs                  # built once, shorter sequences read a prefix
    cs = cs[:40]
    assert torch.equal(cs[:, 0], cos[0, :, :64]) and torch.equal(cs[:, 0], cos[0, :, 64:])
    assert torch.equal(cs[:, 1], sin[0, :, :64]) and torch.equal(cs[:, 1], sin[0, :, 64:])


def test_encoder_refuses_a_sequence_past_max_position_embeddings():
    from gmlm_amd import qwen3
    _, plm = _tiny_model(max_position_embeddings=16)
    with pytest.raises(ValueError, match="max_position_embeddings"):
        qwen3.qwen3_encode(plm, torch.zeros(1, 17, dtype=torch.long), torch.tensor([17], dtype=torch.int32), torch.float32)


# ---- code objects ----------------------------------------------------------------------------------
def _code_objects(so, into):
    from test_wgrad_cpu import _code_objects as co
    return co(so, into)


CAUSAL_KERNELS = {f"causal128::{k}<{t}>" for k in ("fwd_kernel", "dq_kernel", "dkv_kernel", "delta_kernel")
                  for t in ("unsigned short", "float")}
ROW_PREFIXES = ("rmsnorm_fwd_kernel<", "rmsnorm_bwd_kernel<", "qknorm_rope_fwd_kernel<", "qknorm_rope_bwd_kernel<",
                "swiglu_fwd_kernel<", "swiglu_bwd_kernel<")


def _bare(mangled):
    name = torch._C._demangle(mangled)
    name = name[5:] if name.startswith("void ") else name
    depth = 0
    for i, c in enumerate(name):
        depth += (c == "<") - (c == ">")
        if c == "(" and depth == 0:
            name = name[:i]
            break
    return name[len("gmlm::"):] if name.startswith("gmlm::") else name


def test_new_kernels_disassembly():
    """The causal attention kernels are exactly fwd / dq / dkv / delta x {bf16, fp32} (each named by a case of
    test_gpu_decoder_ops.py); they and the row kernels have no scratch (spill) traffic and no packed-fp32 VALU
    (DESIGN.md section 5 b); the attention kernels run on the matrix pipe."""
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
                if name.startswith("causal128::") or name.startswith(ROW_PREFIXES):
                    bodies[name] = m.group(2)
        assert {n for n in bodies if n.startswith("causal128::")} == CAUSAL_KERNELS, sorted(bodies)
        for prefix in ROW_PREFIXES:
            got = {n for n in bodies if n.startswith(prefix)}
            assert {n.split("<")[1].split(",")[0].rstrip(">") for n in got} == {"unsigned short", "float"}, (prefix, got)
        for name, body in bodies.items():
            if name.startswith("causal128::") and "delta_kernel" not in name:
                assert "v_mfma" in body, name
            assert not re.search(r"v_pk_\w+_f32", body), (name, re.findall(r"v_pk_\w+_f32", body)[:3])
            assert "scratch_" not in body and "buffer_store" not in body, name
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
