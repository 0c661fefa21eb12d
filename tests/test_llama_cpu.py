"""Host side of the Llama / Qwen2 / Mistral text encoder (no GPU needed): the ninth header (include/gmlm_hip_gqa.h), its ctypes
table ``_lib.SIGNATURES_GQA`` and the exported symbols agree type by type, the table sitting between SIGNATURES_RELBIAS and
SIGNATURES_DISENT in ``SIGNATURE_TABLES_LATER`` and sharing no name with any other; the entry points decide every documented
refusal and the nothing-to-do cases before any launch; ``llama.check_supported`` names each problem, and all of them at once;
the model layer routes the three model types to ``gmlm_amd.llama``; ``llama.rope_table`` holds the floats of HF's rotary
embedding; and the ``gqa::`` kernels of the built code objects are the ones tests/test_gpu_gqa_kernels.py runs, none with a
private segment (spill) or packed-fp32 VALU."""
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
from test_wgrad_cpu import LLVM, _code_objects

OK, EINVAL, EWORKSPACE, ELAUNCH = 0, -1, -2, -3
F32, BF16 = 0, 1
A = 0x10000000        # fabricated, non-null, 16-byte aligned: every call below ends before or at the launch
HEADER = os.path.join(ROOT, "include", "gmlm_hip_gqa.h")

no_device = pytest.mark.skipif(torch.cuda.device_count() > 0,
                               reason="fabricated addresses: only meaningful (and only safe) without a device")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libgmlm_hip.so not built")
    return _lib.lib()


# ------------------------------------------------------------------------------------------------------------------ ABI
ATTN = ["gmlm_attention_causal_d64" + t for t in ("_bwd", "_fwd", "_varlen_bwd", "_varlen_fwd", "_varlen_workspace_bytes", "_workspace_bytes")]
ENTRY_POINTS = ATTN + ["gmlm_rope_heads_bwd", "gmlm_rope_heads_fwd"]


def test_header_ctypes_table_and_exports_agree(lib):
    protos = parse_header(open(HEADER).read())
    assert sorted(protos) == ENTRY_POINTS and len(protos) == 8
    assert not signature_mismatches(protos, _lib.SIGNATURES_GQA)
    for name in protos:
        assert hasattr(lib, name), f"{name} declared in include/gmlm_hip_gqa.h but not exported"
        assert getattr(lib, name).argtypes == _lib.SIGNATURES_GQA[name][1]                     # lib() bound the new table
    later = _lib.SIGNATURE_TABLES_LATER
    assert len(_lib.SIGNATURE_TABLES) == 6 and later[0] is _lib.SIGNATURES_RELBIAS and later[-1] is _lib.SIGNATURES_DISENT
    assert any(t is _lib.SIGNATURES_GQA for t in later[1:-1]) and not any(t is _lib.SIGNATURES_GQA for t in _lib.SIGNATURE_TABLES)
    others = set().union(*(set(t) for t in _lib.SIGNATURE_TABLES + later if t is not _lib.SIGNATURES_GQA))
    assert not set(_lib.SIGNATURES_GQA) & others
    assert lib.gmlm_version() == 1


def test_the_attention_six_take_the_argument_lists_of_their_d128_namesakes():
    main = parse_header(open(os.path.join(ROOT, "include", "gmlm_hip.h")).read())
    protos = parse_header(open(HEADER).read())
    for name in ATTN:
        assert protos[name] == main[name.replace("_d64", "_d128")], name
    rope = "qkv qkv_stride cos_sin max_len tokens seq_len pos_ids heads d dtype stream".split()
    assert [n for _, n in protos["gmlm_rope_heads_fwd"][1]] == rope
    assert [n for _, n in protos["gmlm_rope_heads_bwd"][1]] == ["d" + rope[0], "d" + rope[1]] + rope[2:]


_BASE = dict(q=A, k=A, v=A, kv_len=None, b=2, hq=6, hkv=2, lq=64, lk=64, d=64, q_stride=640, k_stride=640, v_stride=640, scale=0.125,
             dropout_p=0.0, out=A, out_lo=None, lse=A, dtype=BF16, stream=None, dout=A, dq=A, dk=A, dv=A, dq_stride=640, dk_stride=640,
             dv_stride=640, workspace=A, workspace_bytes=1 << 40, cu_seqlens=A, num_seqs=2, max_len=64, total_rows=100)
_FWD = "q k v kv_len b hq hkv lq lk d q_stride k_stride v_stride scale dropout_p out out_lo lse dtype stream".split()
_BWD = ("q k v out out_lo dout lse kv_len b hq hkv lq lk d q_stride k_stride v_stride scale dropout_p dq dk dv dq_stride dk_stride "
        "dv_stride dtype workspace workspace_bytes stream").split()
_VFWD = ("q k v cu_seqlens num_seqs max_len total_rows hq hkv d q_stride k_stride v_stride scale dropout_p out out_lo lse dtype "
         "stream").split()
_VBWD = ("q k v out out_lo dout lse cu_seqlens num_seqs max_len total_rows hq hkv d q_stride k_stride v_stride scale dropout_p dq dk dv "
         "dq_stride dk_stride dv_stride dtype workspace workspace_bytes stream").split()
_LISTS = {"fwd": _FWD, "bwd": _BWD, "varlen_fwd": _VFWD, "varlen_bwd": _VBWD}


def _call(lib, which, **mut):
    a = dict(_BASE, **mut)
    return getattr(lib, "gmlm_attention_causal_d64_" + which)(*[a[n] for n in _LISTS[which]]), lib.gmlm_last_error()


def test_argument_lists_follow_the_header():
    protos = parse_header(open(HEADER).read())
    for which, names in _LISTS.items():
        assert [n for _, n in protos["gmlm_attention_causal_d64_" + which][1]] == names, which
    assert [n for _, n in protos["gmlm_attention_causal_d64_workspace_bytes"][1]] == "b hq lq".split()
    assert [n for _, n in protos["gmlm_attention_causal_d64_varlen_workspace_bytes"][1]] == "total_rows hq".split()


_REFUSALS = [
    (dict(d=128), b"head dim"), (dict(d=96), b"head dim"), (dict(d=32), b"head dim"),
    (dict(dtype=2), b"dtype"),
    (dict(hq=7), b"multiple of"), (dict(hkv=4), b"multiple of"),
    (dict(dropout_p=0.1), b"dropout"),
    (dict(scale=0.0), b"scale"),
    (dict(hq=0), b"bad sizes"), (dict(hkv=-1), b"bad sizes"),
    (dict(q_stride=376), b"stride"),                                    # below hq * 64
    (dict(k_stride=120), b"stride"),                                    # below hkv * 64
    (dict(q_stride=644), b"stride"),                                    # bf16: not a multiple of 8 elements
    (dict(dtype=F32, v_stride=642), b"stride"),                         # fp32: not a multiple of 4 elements
    (dict(v_stride=1 << 24), b"stride"),
    (dict(q=A + 8), b"aligned"), (dict(k=None), b"null"), (dict(out=None), b"out"), (dict(out=A + 4), b"out"),
    (dict(out_lo=A, dtype=F32), b"out_lo"), (dict(out_lo=A + 8), b"out_lo"),
]
_PADDED_ONLY = [(dict(lk=65), b"lq == lk"), (dict(lq=63), b"lq == lk"), (dict(b=-1), b"bad sizes"),
                (dict(b=(1 << 31) // 6 + 1, lq=1, lk=1), b"too many work items")]
_PACKED_ONLY = [(dict(cu_seqlens=None), b"cu_seqlens"), (dict(max_len=0), b"max_len"), (dict(total_rows=-1), b"packed rows"),
                (dict(total_rows=1 << 30), b"packed rows"), (dict(num_seqs=(1 << 31) // 6 + 1, max_len=1), b"too many work items")]
_ids = lambda cases: [",".join(f"{k}={v}" for k, v in m.items()) for m, _ in cases]


@no_device
@pytest.mark.parametrize("which", ["fwd", "bwd", "varlen_fwd", "varlen_bwd"])
@pytest.mark.parametrize("mut,msg", _REFUSALS, ids=_ids(_REFUSALS))
def test_causal_d64_refusals_are_decided_on_the_host(lib, which, mut, msg):
    if "out" in mut and "out_lo" not in mut and which.endswith("bwd"):
        msg = b"out/dout/lse"                                           # the backward reads out
    rc, err = _call(lib, which, **mut)
    assert rc == EINVAL and msg in err, (mut, rc, err)


@no_device
@pytest.mark.parametrize("which", ["fwd", "bwd"])
@pytest.mark.parametrize("mut,msg", _PADDED_ONLY, ids=_ids(_PADDED_ONLY))
def test_padded_refusals(lib, which, mut, msg):
    rc, err = _call(lib, which, **mut)
    assert rc == EINVAL and msg in err, (mut, rc, err)


@no_device
@pytest.mark.parametrize("which", ["varlen_fwd", "varlen_bwd"])
@pytest.mark.parametrize("mut,msg", _PACKED_ONLY, ids=_ids(_PACKED_ONLY))
def test_packed_refusals(lib, which, mut, msg):
    rc, err = _call(lib, which, **mut)
    assert rc == EINVAL and msg in err, (mut, rc, err)


@no_device
def test_backward_refuses_bad_gradient_operands(lib):
    for which in ("bwd", "varlen_bwd"):
        for mut, msg in ((dict(dq=None), b"dq"), (dict(dk=A + 4), b"dk"), (dict(dv_stride=120), b"dv"), (dict(dq_stride=644), b"dq"),
                         (dict(dout=None), b"out/dout/lse"), (dict(lse=None), b"out/dout/lse")):
            rc, err = _call(lib, which, **mut)
            assert rc == EINVAL and msg in err, (which, mut, rc, err)


@no_device
def test_valid_causal_d64_calls_reach_the_launch(lib):
    for which in _LISTS:
        for mut in (dict(), dict(dtype=F32), dict(out_lo=A), dict(hq=7, hkv=1, q_stride=576, dq_stride=576), dict(hq=2, hkv=2),
                    dict(lq=1, lk=1, max_len=1), dict(q_stride=384, k_stride=128, v_stride=128)):
            rc, err = _call(lib, which, **mut)
            assert rc == ELAUNCH, (which, mut, rc, err)
    assert _call(lib, "fwd", kv_len=A)[0] == ELAUNCH and _call(lib, "bwd", kv_len=A)[0] == ELAUNCH
    assert _call(lib, "fwd", b=(1 << 31) // 6 - 1, lq=1, lk=1)[0] == ELAUNCH            # just below the work-item bound


@no_device
def test_backward_workspace_boundary(lib):
    need = lib.gmlm_attention_causal_d64_workspace_bytes(2, 6, 300)          # delta [b, hq, l]
    assert need == 2 * 6 * 300 * 4 and lib.gmlm_attention_causal_d64_workspace_bytes(0, 6, 0) > 0
    shape = dict(lq=300, lk=300)
    assert _call(lib, "bwd", workspace_bytes=need, **shape)[0] == ELAUNCH
    rc, err = _call(lib, "bwd", workspace_bytes=need - 1, **shape)
    assert rc == EWORKSPACE and b"workspace" in err
    assert _call(lib, "bwd", workspace=None, **shape)[0] == EWORKSPACE
    need = lib.gmlm_attention_causal_d64_varlen_workspace_bytes(100, 6)      # delta [hq, total_rows]
    assert need == 6 * 100 * 4 and lib.gmlm_attention_causal_d64_varlen_workspace_bytes(0, 6) > 0
    assert _call(lib, "varlen_bwd", workspace_bytes=need)[0] == ELAUNCH
    assert _call(lib, "varlen_bwd", workspace_bytes=need - 1)[0] == EWORKSPACE
    assert _call(lib, "varlen_bwd", workspace=None)[0] == EWORKSPACE


@no_device
def test_nothing_to_do_needs_no_pointer_but_sizes_are_still_checked(lib):
    nothing = dict(q=None, k=None, v=None, out=None, lse=None, dout=None, dq=None, dk=None, dv=None, workspace=None, workspace_bytes=0)
    for which, empties in (("fwd", (dict(b=0), dict(lq=0, lk=0))), ("bwd", (dict(b=0), dict(lq=0, lk=0))),
                           ("varlen_fwd", (dict(num_seqs=0), dict(total_rows=0))), ("varlen_bwd", (dict(num_seqs=0), dict(total_rows=0)))):
        for empty in empties:
            assert _call(lib, which, **nothing, **empty)[0] == OK, (which, empty)
            rc, err = _call(lib, which, **nothing, **empty, d=128)
            assert rc == EINVAL and b"head dim" in err
            rc, err = _call(lib, which, **nothing, **empty, dropout_p=0.5)
            assert rc == EINVAL and b"dropout" in err


# ---- rope_heads
_ROPE = dict(qkv=A, qkv_stride=640, cos_sin=A, max_len=128, tokens=256, seq_len=128, pos_ids=None, heads=8, d=64, dtype=BF16, stream=None)
_ROPE_ARGS = "qkv qkv_stride cos_sin max_len tokens seq_len pos_ids heads d dtype stream".split()


def _rope(lib, which="fwd", **mut):
    a = dict(_ROPE, **mut)
    return getattr(lib, "gmlm_rope_heads_" + which)(*[a[n] for n in _ROPE_ARGS]), lib.gmlm_last_error()


_ROPE_REFUSALS = [
    (dict(d=96), b"head dim"), (dict(d=32), b"head dim"), (dict(d=256), b"head dim"),
    (dict(heads=0), b"bad sizes"), (dict(heads=-3), b"bad sizes"), (dict(heads=4096), b"bad sizes"), (dict(tokens=-1), b"bad sizes"),
    (dict(cos_sin=None), b"table"), (dict(cos_sin=A + 4), b"table"),
    (dict(max_len=0), b"empty"), (dict(max_len=-1), b"empty"),
    (dict(seq_len=129), b"exceeds"), (dict(seq_len=0), b"length 0"), (dict(seq_len=-1), b"sequence length"),
    (dict(qkv_stride=504), b"stride"), (dict(qkv_stride=516), b"stride"), (dict(dtype=F32, qkv_stride=514), b"stride"),
    (dict(dtype=3), b"dtype"),
    (dict(qkv=None), b"null"), (dict(qkv=A + 8), b"aligned"),
    (dict(tokens=1 << 32, seq_len=1), b"too many head rows"),
]


@no_device
@pytest.mark.parametrize("which", ["fwd", "bwd"])
@pytest.mark.parametrize("mut,msg", _ROPE_REFUSALS, ids=_ids(_ROPE_REFUSALS))
def test_rope_heads_refusals_are_decided_on_the_host(lib, which, mut, msg):
    rc, err = _rope(lib, which, **mut)
    assert rc == EINVAL and msg in err, (mut, rc, err)


@no_device
def test_valid_rope_heads_calls_reach_the_launch(lib):
    for which in ("fwd", "bwd"):
        for mut in (dict(), dict(dtype=F32), dict(d=128, qkv_stride=1024), dict(heads=7, qkv_stride=448), dict(pos_ids=A, seq_len=0),
                    dict(pos_ids=A, seq_len=10 ** 9), dict(heads=1, qkv_stride=64, tokens=1, seq_len=1)):
            rc, err = _rope(lib, which, **mut)
            assert rc == ELAUNCH, (which, mut, rc, err)


def test_rope_heads_with_no_token_returns_ok_after_the_size_checks(lib):
    none = dict(qkv=None, cos_sin=None, tokens=0)
    for which in ("fwd", "bwd"):
        assert _rope(lib, which, **none)[0] == OK and _rope(lib, which, **none, seq_len=0)[0] == OK
        assert _rope(lib, which, **none, pos_ids=None, d=128, qkv_stride=1024)[0] == OK
        for mut, msg in ((dict(d=96), b"head dim"), (dict(heads=0), b"bad sizes"), (dict(max_len=0), b"empty"), (dict(qkv_stride=8), b"stride")):
            rc, err = _rope(lib, which, **none, **mut)
            assert rc == EINVAL and msg in err, (which, mut, rc, err)


def test_new_ops_fail_loudly_without_a_gpu(lib):
    """CPU tensors raise the library's error: no eager fallback behind the new operators."""
    from gmlm_amd import ops
    cs = torch.zeros(8, 2, 32)
    with pytest.raises(_lib.GmlmHipError):
        ops.rope_causal_gqa(torch.zeros(1, 4, 256), cs, None, 2, 1, 64, 0.125)
    with pytest.raises(_lib.GmlmHipError):
        ops.rope_causal_gqa_varlen(torch.zeros(4, 256), cs, torch.arange(4), torch.tensor([0, 4], dtype=torch.int32), 4, 2, 1, 64, 0.125)
    with pytest.raises(_lib.GmlmHipError):
        ops.causal_attention(torch.zeros(1, 4, 128), torch.zeros(1, 4, 64), torch.zeros(1, 4, 64), None, 2, 1, 0.125, 64)


# --------------------------------------------------------------------------------------------------------- check_supported
def _cfg(kind="llama", **kw):
    from transformers import LlamaConfig, MistralConfig, Qwen2Config
    base = dict(vocab_size=96, hidden_size=128, intermediate_size=192, num_hidden_layers=2, num_attention_heads=2, num_key_value_heads=1,
                max_position_embeddings=512)
    if kind == "mistral":
        base["sliding_window"] = None
    base.update(kw)
    return {"llama": LlamaConfig, "qwen2": Qwen2Config, "mistral": MistralConfig}[kind](**base)


class _Holder:
    def __init__(self, config):
        self.config = config


LLAMA3 = dict(rope_type="llama3", rope_theta=10000.0, factor=8.0, low_freq_factor=1.0, high_freq_factor=4.0,
              original_max_position_embeddings=64)


def test_check_supported_accepts_tiny_llama_qwen2_and_mistral_configs():
    from gmlm_amd import llama
    for kind in ("llama", "qwen2", "mistral"):
        cfg = _cfg(kind)
        llama.check_supported(_Holder(cfg))
        assert cfg.model_type == kind and llama.sliding_window(cfg) is None
    llama.check_supported(_Holder(_cfg("llama", attention_bias=True, rope_parameters=LLAMA3)))
    llama.check_supported(_Holder(_cfg("llama", rope_parameters=dict(rope_type="linear", rope_theta=10000.0, factor=2.0))))
    llama.check_supported(_Holder(_cfg("mistral", hidden_size=256, head_dim=128)))                     # config.head_dim where present
    llama.check_supported(_Holder(_cfg("qwen2", hidden_size=896, num_attention_heads=14, num_key_value_heads=2)))   # Qwen2.5-0.5B
    # a window is accepted; the encode functions hold the call's longest sequence against it
    win = _cfg("mistral", sliding_window=64)
    llama.check_supported(_Holder(win))
    assert llama.sliding_window(win) == 64
    qwin = _cfg("qwen2", sliding_window=32, use_sliding_window=True, max_window_layers=1)
    llama.check_supported(_Holder(qwin))
    assert llama.sliding_window(qwin) == 32 and llama.sliding_window(_cfg("qwen2", sliding_window=32, use_sliding_window=False)) is None
    llama.check_window(win, 64)
    with pytest.raises(ValueError, match="sequence length 65 exceeds sliding_window 64"):
        llama.check_window(win, 65)


_PROBLEMS = [
    (dict(hidden_act="gelu"), "hidden_act='gelu'"),
    (dict(head_dim=32), "head_dim=32"),
    (dict(mlp_bias=True), "mlp_bias"),
    (dict(attention_dropout=0.1), "attention_dropout=0.1"),
    (dict(pretraining_tp=2), "pretraining_tp=2"),
    (dict(num_attention_heads=3, num_key_value_heads=2), "3 query heads / 2 KV heads"),
    (dict(rope_parameters=dict(rope_type="dynamic", rope_theta=10000.0, factor=2.0)), "rope type 'dynamic'"),
]


@pytest.mark.parametrize("kw,word", _PROBLEMS, ids=[w for _, w in _PROBLEMS])
def test_check_supported_names_each_problem(kw, word):
    from gmlm_amd import llama
    cfg = _cfg()
    for k, v in kw.items():
        setattr(cfg, k, v)
    if "head_dim" not in kw:
        cfg.head_dim = 64                                               # 3 heads: keep the head dim out of the message
    with pytest.raises(NotImplementedError) as e:
        llama.check_supported(_Holder(cfg))
    assert word in str(e.value) and str(e.value).count(";") == 0, str(e.value)


def test_check_supported_names_every_problem_at_once():
    from gmlm_amd import llama
    cfg = _cfg()
    for kw, _ in _PROBLEMS:
        for k, v in kw.items():
            setattr(cfg, k, v)
    cfg.model_type = "gemma"
    with pytest.raises(NotImplementedError) as e:
        llama.check_supported(_Holder(cfg))
    for word in ["model_type='gemma'"] + [w for _, w in _PROBLEMS]:
        assert word in str(e.value), (word, str(e.value))
    for rope_type in ("yarn", "longrope"):                              # any type but default / linear / llama3
        cfg = _cfg()
        cfg.rope_parameters = dict(rope_type=rope_type, rope_theta=10000.0, factor=2.0)
        with pytest.raises(NotImplementedError, match=f"rope type '{rope_type}'"):
            llama.check_supported(_Holder(cfg))


def test_other_encoder_modules_refuse_llama_configs_and_it_refuses_theirs():
    from gmlm_amd import bert, deberta, llama, modernbert, mpnet, qwen3
    from transformers import BertConfig, Qwen3Config
    for kind in ("llama", "qwen2", "mistral"):
        for mod in (bert, qwen3, modernbert, mpnet, deberta):
            with pytest.raises(NotImplementedError, match=f"model_type='{kind}'"):
                mod.check_supported(_Holder(_cfg(kind)))
    for other, kind in ((BertConfig(hidden_size=128, num_attention_heads=2), "bert"),
                        (Qwen3Config(hidden_size=256, num_attention_heads=4, num_key_value_heads=2, head_dim=128, intermediate_size=384,
                                     num_hidden_layers=2, vocab_size=96), "qwen3")):
        with pytest.raises(NotImplementedError, match=f"model_type='{kind}'"):
            llama.check_supported(_Holder(other))


# ---------------------------------------------------------------------------------------------------------- model wiring
def _tiny(kind="llama", **kw):
    from transformers import LlamaModel, MistralModel, Qwen2Model
    torch.manual_seed(0)
    return {"llama": LlamaModel, "qwen2": Qwen2Model, "mistral": MistralModel}[kind](_cfg(kind, **kw))


def test_model_dispatches_a_llama_encoder():
    """Fails on the commit before this encoder: ``bert.check_supported`` raises NotImplementedError for model_type 'llama'."""
    import gmlm_amd
    plm = _tiny("llama")
    model = gmlm_amd.GraphTextLM(12, 16, 3, plm_encoder=plm)
    from gmlm_amd import bert, llama, qwen3
    assert model._enc is llama and model._enc is not bert and model._enc is not qwen3 and model._plm_kind == "llama"
    assert model._has_packed_pass() and model._packed_head_dim() == 0      # its own packed pass; no bucketed / recorded form
    with pytest.raises(NotImplementedError, match="BERT-geometry encoders only"):
        model.capture_hip_graphs(torch.zeros(4, 12), torch.zeros(2, 4, dtype=torch.long))
    keys = {k[len("plm_encoder."):] for k in model.state_dict() if k.startswith("plm_encoder.")}
    assert keys == set(plm.state_dict())
    assert {"embed_tokens.weight", "norm.weight", "layers.0.self_attn.q_proj.weight", "layers.1.self_attn.o_proj.weight",
            "layers.0.mlp.gate_proj.weight", "layers.1.post_attention_layernorm.weight"} <= keys


@pytest.mark.parametrize("kind", ["qwen2", "mistral"])
def test_model_dispatches_qwen2_and_mistral_encoders(kind):
    import gmlm_amd
    from gmlm_amd import llama, model as model_mod
    plm = _tiny(kind)
    model = gmlm_amd.GraphTextLM(12, 16, 3, plm_encoder=plm)
    assert model._enc is llama and model._plm_kind == kind
    assert model_mod._ENCODERS[kind] == (llama, "llama_encode", "llama_encode_packed")
    assert {k[len("plm_encoder."):] for k in model.state_dict() if k.startswith("plm_encoder.")} == set(plm.state_dict())


def test_prepare_weights_fuses_the_projections_and_carries_the_biases_the_model_has():
    from gmlm_amd import llama
    for kind, kw, qkv_bias, o_bias in (("llama", {}, False, False), ("llama", dict(attention_bias=True), True, True),
                                       ("qwen2", {}, True, False), ("mistral", {}, False, False)):
        plm = _tiny(kind, **kw)
        with torch.no_grad():
            for p in plm.parameters():
                if p.dim() == 1:
                    p.normal_()
        lws = llama.prepare_weights(plm, torch.float32)
        assert len(lws) == 2
        for lw, layer in zip(lws, plm.layers):
            sa, mlp = layer.self_attn, layer.mlp
            assert tuple(lw.wqkv.shape) == (256, 128) and not lw.wqkv.requires_grad       # (2 + 2 * 1) heads of 64
            assert torch.equal(lw.wqkv, torch.cat([sa.q_proj.weight, sa.k_proj.weight, sa.v_proj.weight]))
            assert torch.equal(lw.wgu, torch.cat([mlp.gate_proj.weight, mlp.up_proj.weight]))
            assert torch.equal(lw.wo, sa.o_proj.weight) and torch.equal(lw.wdown, mlp.down_proj.weight)
            assert (lw.bqkv is not None) == qkv_bias and (lw.bo is not None) == o_bias
            if qkv_bias:
                assert torch.equal(lw.bqkv, torch.cat([sa.q_proj.bias, sa.k_proj.bias, sa.v_proj.bias]))
                assert lw.m_qkv == (sa.q_proj.weight, sa.k_proj.weight, sa.v_proj.weight, sa.q_proj.bias, sa.k_proj.bias, sa.v_proj.bias)
            else:
                assert lw.m_qkv == (sa.q_proj.weight, sa.k_proj.weight, sa.v_proj.weight)
            assert lw.m_wo == ((sa.o_proj.weight, sa.o_proj.bias) if o_bias else (sa.o_proj.weight,))
            assert lw.ln1 is layer.input_layernorm.weight and lw.ln2 is layer.post_attention_layernorm.weight
    with pytest.raises(ValueError):
        llama.prepare_weights(_tiny(), torch.bfloat16, "bf16x3")           # gemm_precision is passed through and checked


@pytest.mark.parametrize("rope", [None, LLAMA3], ids=["default", "llama3"])
def test_rope_table_is_the_hf_rotary_embedding(rope):
    from gmlm_amd import llama
    plm = _tiny("llama", **({} if rope is None else dict(rope_parameters=rope)))
    n = 300
    table = llama.rope_table(plm, n, "cpu")
    assert table.dtype == torch.float32 and table.shape[0] >= n and tuple(table.shape[1:]) == (2, 32) and table.is_contiguous()
    assert table is llama.rope_table(plm, n, "cpu") and table is llama.rope_table(plm, 17, "cpu")          # cached
    cos, sin = plm.rotary_emb(torch.zeros(1, 1), torch.arange(n)[None])                                   # [1, n, 64]: (freqs, freqs)
    assert torch.equal(cos[0, :, :32], cos[0, :, 32:])
    assert torch.equal(table[:n, 0], cos[0, :, :32]) and torch.equal(table[:n, 1], sin[0, :, :32])
    if rope is not None:
        plain = llama.rope_table(_tiny("llama"), n, "cpu")
        assert not torch.equal(plain[:n], table[:n]) and plm.rotary_emb.rope_type == "llama3"               # the scaling acts inside 300 positions
        assert torch.equal(plain[:n, :, 0], table[:n, :, 0])                                                # the highest frequency is kept
    longer = llama.rope_table(plm, 700, "cpu")
    assert longer.shape[0] >= 700 and torch.equal(longer[:n], table[:n])


def test_encoder_refuses_a_sequence_past_the_window_or_the_position_table():
    from gmlm_amd import llama
    plm = _tiny("mistral", sliding_window=64)
    ids = torch.zeros(1, 65, dtype=torch.long)
    with pytest.raises(ValueError, match="sequence length 65 exceeds sliding_window 64"):
        llama.llama_encode(plm, ids, torch.tensor([65], dtype=torch.int32), torch.float32)
    z = torch.zeros(70, dtype=torch.long)
    with pytest.raises(ValueError, match="sequence length 70 exceeds sliding_window 64"):
        llama.llama_encode_packed(plm, z, z, torch.tensor([0, 70], dtype=torch.int32), 70, torch.float32)
    with pytest.raises(ValueError, match="sequence length 513 exceeds max_position_embeddings 512"):
        llama.llama_encode(_tiny(), torch.zeros(1, 513, dtype=torch.long), torch.tensor([513], dtype=torch.int32), torch.float32)
    with pytest.raises(ValueError):
        llama.llama_encode_packed(_tiny(), z[:8], z[:7], torch.tensor([0, 8], dtype=torch.int32), 8, torch.float32)


# --------------------------------------------------------------------------------------------------------- code objects
def test_gqa_kernels_are_the_ones_the_gpu_tests_run():
    from test_gpu_gqa_kernels import UNREACHABLE, expected_kernels
    want = expected_kernels()
    got = _compiled_kernels(lambda name: name.startswith("gqa::"))
    assert len(want) == 2 * 2 * 2 + 2 * 4 and not UNREACHABLE             # rope: dtype x head dim x direction; causal64: dtype x four
    assert got == want, (sorted(got - want), sorted(want - got))


def test_gpu_rope_cases_follow_the_kernel_s_grid_arithmetic():
    """The tail case of the GPU file is sized from kRopeMaxBlocks and the head rows per block; these are the lines it restates."""
    from test_gpu_gqa_kernels import BF, FP, ROPE_CASES, ROPE_MAX_BLOCKS, rope_rows_per_block, tail_tokens
    src = open(os.path.join(ROOT, "gmlm_amd", "csrc", "attn_gqa.hip")).read()
    assert f"constexpr int kRopeMaxBlocks = {ROPE_MAX_BLOCKS};" in src
    assert "gpb = 256 / (d / v);" in src and "const int grid = grid_cap(cdiv(items, gpb), kRopeMaxBlocks);" in src
    assert "first += (int64_t)gridDim.x * GPB" in src and "constexpr int V = Store<T>::kVec, LPR = D / V, GPB = 256 / LPR;" in src
    assert [(rope_rows_per_block(dt, d)) for dt in (BF, FP) for d in (64, 128)] == [32, 16, 16, 8]
    assert [c.id for c in ROPE_CASES] == ["b1_l1", "b2_l3_odd_heads", "seq_len1", "pos_one_row_table", "tail"]
    assert [(c.lead, c.hq, c.hkv, c.table) for c in ROPE_CASES] == [((1, 1), 1, 1, 2), ((2, 3), 3, 1, 3), ((3, 1), 2, 1, 4), ((3,), 2, 1, 1),
                                                                   ((), 2, 1, 300)]
    assert ROPE_CASES[3].positions == (-2, 0, 7)
    for dt in (BF, FP):
        for d in (64, 128):
            per_trip = ROPE_MAX_BLOCKS * rope_rows_per_block(dt, d)
            items = tail_tokens(dt, d, 3) * 3
            assert per_trip < items <= per_trip + 3                        # the second trip holds one to three head rows


def test_gqa_kernels_have_no_private_segment_and_no_packed_fp32():
    """No spill (a zero private segment in every kernel's metadata), no scratch traffic and no packed-fp32 VALU (DESIGN.md
    section 5 b); the attention kernels run on the matrix pipe."""
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libgmlm_hip.so not built")
    if not all(os.path.exists(os.path.join(LLVM, t)) for t in ("llvm-readelf", "llvm-objdump", "llvm-objcopy")):
        pytest.skip("ROCm llvm tools not found")
    tmp = tempfile.mkdtemp()
    try:
        private, bodies = {}, {}
        for co in _code_objects(_lib.LIB_PATH, tmp):
            notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", co], check=True, capture_output=True, text=True).stdout
            for m in re.finditer(r"\.name:\s+(_ZN4gmlm3gqa\w+)\s+\.private_segment_fixed_size:\s+(\d+)", notes):
                private[m.group(1)] = int(m.group(2))
            dis = subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-d", "--mcpu=gfx950", co], check=True, capture_output=True,
                                 text=True).stdout
            for m in re.finditer(r"^[0-9a-f]+ <(_ZN4gmlm3gqa\w+)>:\n(.*?)(?=^[0-9a-f]+ <|\Z)", dis, re.S | re.M):
                bodies[m.group(1)] = m.group(2)
        assert len(private) == 16 and set(private) == set(bodies), (sorted(private), sorted(bodies))
        assert not {n: v for n, v in private.items() if v}, private
        for name, body in bodies.items():
            if "causal64" in name and "delta" not in name:
                assert "v_mfma" in body, name
            assert not re.search(r"v_pk_\w+_f32", body), name
            assert "scratch_" not in body, name
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
