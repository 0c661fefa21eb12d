"""Host side of the EuroBERT and NomicBERT text encoders (no GPU needed): the tenth header (include/gmlm_hip_bidir.h), its ctypes
table ``_lib.SIGNATURES_BIDIR`` and the exported symbols agree type by type, the table sitting strictly inside
``SIGNATURE_TABLES_LATER`` and sharing no name with any other; the six argument lists are those of their
``gmlm_attention_causal_d64_*`` namesakes; the entry points decide every documented refusal and the nothing-to-do cases before
any launch; ``eurobert.check_supported`` and ``nomic_bert.check_supported`` name each problem, and all of them at once; the
model layer routes the two model types to their modules; ``prepare_weights`` fuses the projections row-exactly; the NomicBERT
rope table holds the floats of HF's rotary embedding at theta 1000; and the ``bidir::`` kernels of the built code objects are
the ones tests/test_gpu_bidir_kernels.py runs, none with a private segment (spill)."""
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
from test_llama_cpu import _BASE, _LISTS, _Holder, _ids, no_device
from test_wgrad_cpu import LLVM, _code_objects

OK, EINVAL, EWORKSPACE, ELAUNCH = 0, -1, -2, -3
F32, BF16 = 0, 1
A = 0x10000000        # fabricated, non-null, 16-byte aligned: every call below ends before or at the launch
HEADER = os.path.join(ROOT, "include", "gmlm_hip_bidir.h")
STEM = "gmlm_attention_bidir_gqa"
TAILS = ("_bwd", "_fwd", "_varlen_bwd", "_varlen_fwd", "_varlen_workspace_bytes", "_workspace_bytes")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libgmlm_hip.so not built")
    return _lib.lib()


# ------------------------------------------------------------------------------------------------------------------ ABI
def test_header_ctypes_table_and_exports_agree(lib):
    protos = parse_header(open(HEADER).read())
    assert sorted(protos) == [STEM + t for t in TAILS] and len(protos) == 6
    assert not signature_mismatches(protos, _lib.SIGNATURES_BIDIR)
    for name in protos:
        assert hasattr(lib, name), f"{name} declared in include/gmlm_hip_bidir.h but not exported"
        assert getattr(lib, name).argtypes == _lib.SIGNATURES_BIDIR[name][1]                     # lib() bound the new table
    later = _lib.SIGNATURE_TABLES_LATER
    assert any(t is _lib.SIGNATURES_BIDIR for t in later[1:-1])                                  # strictly inside
    assert later[0] is not _lib.SIGNATURES_BIDIR and later[-1] is not _lib.SIGNATURES_BIDIR
    assert not any(t is _lib.SIGNATURES_BIDIR for t in _lib.SIGNATURE_TABLES)
    others = set().union(*(set(t) for t in _lib.SIGNATURE_TABLES + later if t is not _lib.SIGNATURES_BIDIR))
    assert not set(_lib.SIGNATURES_BIDIR) & others
    assert lib.gmlm_version() == 1
    text = open(HEADER).read()
    assert '#include "gmlm_hip.h"' in text and 'extern "C"' in text


def test_the_six_take_the_argument_lists_of_their_causal_d64_namesakes():
    gqa = parse_header(open(os.path.join(ROOT, "include", "gmlm_hip_gqa.h")).read())
    protos = parse_header(open(HEADER).read())
    for tail in TAILS:
        assert protos[STEM + tail] == gqa["gmlm_attention_causal_d64" + tail], tail
        assert _lib.SIGNATURES_BIDIR[STEM + tail] == _lib.SIGNATURES_GQA["gmlm_attention_causal_d64" + tail], tail
    for which, names in _LISTS.items():
        assert [n for _, n in protos[f"{STEM}_{which}"][1]] == names, which


def test_the_makefile_names_the_new_source_and_header():
    mk = open(os.path.join(ROOT, "gmlm_amd", "csrc", "Makefile")).read()
    srcs = re.search(r"^SRCS\s*=(.*)$", mk, re.M).group(1).split()
    assert "attn_bidir.hip" in srcs and os.path.exists(os.path.join(ROOT, "gmlm_amd", "csrc", "attn_bidir.hip"))
    assert "../../include/gmlm_hip_bidir.h" in re.search(r"^\$\(BUILD\)/%\.o:(.*)$", mk, re.M).group(1).split()


# ------------------------------------------------------------------------------------------------- entry-point refusals
def _call(lib, which, **mut):
    a = dict(_BASE, **mut)
    return getattr(lib, f"{STEM}_{which}")(*[a[n] for n in _LISTS[which]]), lib.gmlm_last_error()


_D128 = dict(d=128, q_stride=1280, k_stride=1280, v_stride=1280, dq_stride=1280, dk_stride=1280, dv_stride=1280)
_REFUSALS = [
    (dict(d=32), b"head dim"), (dict(d=96), b"head dim"), (dict(d=256), b"head dim"),
    (dict(dtype=2), b"dtype"),
    (dict(hq=7), b"multiple of"), (dict(hkv=4), b"multiple of"),
    (dict(dropout_p=0.1), b"dropout"),
    (dict(scale=0.0), b"scale"), (dict(scale=-1.0), b"scale"),
    (dict(hq=0), b"bad sizes"), (dict(hkv=-1), b"bad sizes"),
    (dict(q_stride=376), b"stride"),                                    # below hq * 64
    (dict(k_stride=120), b"stride"),                                    # below hkv * 64
    (dict(_D128, q_stride=640), b"stride"),                             # d = 128: below hq * 128
    (dict(_D128, v_stride=192), b"stride"),                             # d = 128: below hkv * 128
    (dict(q_stride=644), b"stride"),                                    # bf16: not a multiple of 8 elements
    (dict(dtype=F32, v_stride=642), b"stride"),                         # fp32: not a multiple of 4 elements
    (dict(v_stride=1 << 24), b"stride"),
    (dict(q=A + 8), b"aligned"), (dict(k=None), b"null"), (dict(v=None), b"null"), (dict(out=None), b"out"), (dict(out=A + 4), b"out"),
    (dict(out_lo=A, dtype=F32), b"out_lo"), (dict(out_lo=A + 8), b"out_lo"),
]
_PADDED_ONLY = [(dict(lk=65), b"lq == lk"), (dict(lq=63), b"lq == lk"), (dict(b=-1), b"bad sizes"),
                (dict(b=(1 << 31) // 6 + 1, lq=1, lk=1), b"too many work items")]
_PACKED_ONLY = [(dict(cu_seqlens=None), b"cu_seqlens"), (dict(max_len=0), b"max_len"), (dict(total_rows=-1), b"packed rows"),
                (dict(total_rows=1 << 30), b"packed rows"), (dict(num_seqs=(1 << 31) // 6 + 1, max_len=1), b"too many work items")]


@no_device
@pytest.mark.parametrize("which", ["fwd", "bwd", "varlen_fwd", "varlen_bwd"])
@pytest.mark.parametrize("mut,msg", _REFUSALS, ids=_ids(_REFUSALS))
def test_bidir_refusals_are_decided_on_the_host(lib, which, mut, msg):
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
                         (dict(_D128, dk_stride=192), b"dk"), (dict(dout=None), b"out/dout/lse"), (dict(lse=None), b"out/dout/lse")):
            rc, err = _call(lib, which, **mut)
            assert rc == EINVAL and msg in err, (which, mut, rc, err)


@no_device
def test_valid_bidir_calls_reach_the_launch(lib):
    for which in _LISTS:
        for mut in (dict(), dict(dtype=F32), dict(out_lo=A), dict(hq=7, hkv=1, q_stride=576, dq_stride=576), dict(hq=2, hkv=2),
                    dict(lq=1, lk=1, max_len=1), dict(q_stride=384, k_stride=128, v_stride=128), _D128, dict(_D128, dtype=F32),
                    dict(_D128, q_stride=768, k_stride=256, v_stride=256)):
            rc, err = _call(lib, which, **mut)
            assert rc == ELAUNCH, (which, mut, rc, err)
    assert _call(lib, "fwd", kv_len=A)[0] == ELAUNCH and _call(lib, "bwd", kv_len=A)[0] == ELAUNCH
    assert _call(lib, "fwd", b=(1 << 31) // 6 - 1, lq=1, lk=1)[0] == ELAUNCH            # just below the work-item bound


@no_device
def test_backward_workspace_boundary(lib):
    need = lib.gmlm_attention_bidir_gqa_workspace_bytes(2, 6, 300)          # delta [b, hq, l]
    assert need == 2 * 6 * 300 * 4 and lib.gmlm_attention_bidir_gqa_workspace_bytes(0, 6, 0) > 0
    shape = dict(lq=300, lk=300)
    assert _call(lib, "bwd", workspace_bytes=need, **shape)[0] == ELAUNCH
    rc, err = _call(lib, "bwd", workspace_bytes=need - 1, **shape)
    assert rc == EWORKSPACE and b"workspace" in err
    assert _call(lib, "bwd", workspace=None, **shape)[0] == EWORKSPACE
    need = lib.gmlm_attention_bidir_gqa_varlen_workspace_bytes(100, 6)      # delta [hq, total_rows]
    assert need == 6 * 100 * 4 and lib.gmlm_attention_bidir_gqa_varlen_workspace_bytes(0, 6) > 0
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
            assert _call(lib, which, **nothing, **empty, d=128)[0] == OK, (which, empty)
            for mut, msg in ((dict(d=96), b"head dim"), (dict(dropout_p=0.5), b"dropout"), (dict(hq=7), b"multiple of"), (dict(dtype=5), b"dtype")):
                rc, err = _call(lib, which, **nothing, **empty, **mut)
                assert rc == EINVAL and msg in err, (which, empty, mut, rc, err)


def test_new_ops_fail_loudly_without_a_gpu(lib):
    """CPU tensors raise the library's error: no eager fallback behind the new operators."""
    from gmlm_amd import ops
    cs = torch.zeros(8, 2, 32)
    with pytest.raises(_lib.GmlmHipError):
        ops.rope_bidir_gqa(torch.zeros(1, 4, 256), cs, None, 2, 1, 64, 0.125)
    with pytest.raises(_lib.GmlmHipError):
        ops.rope_bidir_gqa_varlen(torch.zeros(4, 256), cs, torch.arange(4), torch.tensor([0, 4], dtype=torch.int32), 4, 2, 1, 64, 0.125)
    with pytest.raises(_lib.GmlmHipError):
        ops.bidir_gqa_attention(torch.zeros(1, 4, 128), torch.zeros(1, 4, 64), torch.zeros(1, 4, 64), None, 2, 1, 0.125, 64)


# --------------------------------------------------------------------------------------------------------- check_supported
def _euro_cfg(**kw):
    from transformers import EuroBertConfig
    base = dict(vocab_size=96, hidden_size=128, intermediate_size=192, num_hidden_layers=2, num_attention_heads=2, num_key_value_heads=1,
                max_position_embeddings=512, pad_token_id=0, bos_token_id=1, eos_token_id=2, mask_token_id=3)
    return EuroBertConfig(**{**base, **kw})


def _nomic_cfg(**kw):
    from transformers import NomicBertConfig
    base = dict(vocab_size=96, hidden_size=128, intermediate_size=192, num_hidden_layers=2, num_attention_heads=2, max_position_embeddings=512)
    return NomicBertConfig(**{**base, **kw})


LLAMA3 = dict(rope_type="llama3", rope_theta=10000.0, factor=8.0, low_freq_factor=1.0, high_freq_factor=4.0,
              original_max_position_embeddings=64)


def test_check_supported_accepts_plain_configs():
    from gmlm_amd import eurobert, nomic_bert
    cfg = _euro_cfg()
    eurobert.check_supported(_Holder(cfg))
    assert cfg.model_type == "eurobert" and eurobert.head_dim(cfg) == 64
    eurobert.check_supported(_Holder(_euro_cfg(attention_bias=True, rope_parameters=LLAMA3)))
    eurobert.check_supported(_Holder(_euro_cfg(rope_parameters=dict(rope_type="linear", rope_theta=10000.0, factor=2.0))))
    eurobert.check_supported(_Holder(_euro_cfg(hidden_size=256, head_dim=128)))
    eurobert.check_supported(_Holder(_euro_cfg(num_key_value_heads=2)))                                       # MHA
    eurobert.check_supported(_Holder(_euro_cfg(hidden_size=1152, num_attention_heads=18, num_key_value_heads=6)))
    cfg = _nomic_cfg()
    nomic_bert.check_supported(_Holder(cfg))
    assert cfg.model_type == "nomic_bert" and cfg.rope_parameters["rope_theta"] == 1000.0
    nomic_bert.check_supported(_Holder(_nomic_cfg(hidden_size=768, num_attention_heads=12, hidden_dropout_prob=0.1)))


_EURO_PROBLEMS = [
    (dict(hidden_act="gelu"), "hidden_act='gelu'"),
    (dict(head_dim=32), "head_dim=32"),
    (dict(mlp_bias=True), "mlp_bias"),
    (dict(attention_dropout=0.1), "attention_dropout=0.1"),
    (dict(pretraining_tp=2), "pretraining_tp=2"),
    (dict(num_attention_heads=3, num_key_value_heads=2), "3 query heads / 2 KV heads"),
    (dict(rope_parameters=dict(rope_type="dynamic", rope_theta=10000.0, factor=2.0)), "rope type 'dynamic'"),
]
_NOMIC_PROBLEMS = [
    (dict(head_dim=32), "head_dim=32"),
    (dict(hidden_act="gelu"), "hidden_act='gelu'"),
    (dict(attention_probs_dropout_prob=0.1), "attention_probs_dropout_prob=0.1"),
    (dict(rope_parameters=dict(rope_type="dynamic", rope_theta=1000.0, factor=2.0)), "rope type 'dynamic'"),
]


def _broken(cfg, kws):
    for kw in kws:
        for k, v in kw.items():
            setattr(cfg, k, v)
    return cfg


@pytest.mark.parametrize("kw,word", _EURO_PROBLEMS, ids=[w for _, w in _EURO_PROBLEMS])
def test_eurobert_check_supported_names_each_problem(kw, word):
    from gmlm_amd import eurobert
    cfg = _broken(_euro_cfg(), [kw])
    if "head_dim" not in kw:
        cfg.head_dim = 64                                               # 3 heads: keep the head dim out of the message
    with pytest.raises(NotImplementedError) as e:
        eurobert.check_supported(_Holder(cfg))
    assert word in str(e.value) and str(e.value).count(";") == 0, str(e.value)


@pytest.mark.parametrize("kw,word", _NOMIC_PROBLEMS, ids=[w for _, w in _NOMIC_PROBLEMS])
def test_nomic_bert_check_supported_names_each_problem(kw, word):
    from gmlm_amd import nomic_bert
    with pytest.raises(NotImplementedError) as e:
        nomic_bert.check_supported(_Holder(_broken(_nomic_cfg(), [kw])))
    assert word in str(e.value) and str(e.value).count(";") == 0, str(e.value)


def test_check_supported_names_every_problem_at_once():
    from gmlm_amd import eurobert, nomic_bert
    for mod, cfg, problems in ((eurobert, _euro_cfg(), _EURO_PROBLEMS), (nomic_bert, _nomic_cfg(), _NOMIC_PROBLEMS)):
        cfg = _broken(cfg, [kw for kw, _ in problems])
        cfg.model_type = "gemma"
        with pytest.raises(NotImplementedError) as e:
            mod.check_supported(_Holder(cfg))
        for word in ["model_type='gemma'"] + [w for _, w in problems]:
            assert word in str(e.value), (word, str(e.value))
    for rope_type in ("yarn", "longrope"):                              # any type but default / linear / llama3
        for mod, cfg in ((eurobert, _euro_cfg()), (nomic_bert, _nomic_cfg())):
            cfg.rope_parameters = dict(rope_type=rope_type, rope_theta=10000.0, factor=2.0)
            with pytest.raises(NotImplementedError, match=f"rope type '{rope_type}'"):
                mod.check_supported(_Holder(cfg))


def test_other_encoder_modules_refuse_the_new_configs_and_they_refuse_theirs():
    from gmlm_amd import bert, deberta, eurobert, llama, modernbert, mpnet, nomic_bert, qwen3
    from transformers import BertConfig, LlamaConfig, ModernBertConfig, Qwen3Config
    for cfg, own in ((_euro_cfg(), eurobert), (_nomic_cfg(), nomic_bert)):
        for mod in (bert, qwen3, modernbert, mpnet, deberta, llama, eurobert, nomic_bert):
            if mod is own:
                continue
            with pytest.raises(NotImplementedError, match=f"model_type='{cfg.model_type}'"):
                mod.check_supported(_Holder(cfg))
    small = dict(hidden_size=128, num_attention_heads=2, intermediate_size=192, num_hidden_layers=2, vocab_size=96)
    for other in (BertConfig(**small), LlamaConfig(**small, num_key_value_heads=1), ModernBertConfig(**small),
                  Qwen3Config(**dict(small, hidden_size=256, num_attention_heads=4), num_key_value_heads=2, head_dim=128)):
        for mod in (eurobert, nomic_bert):
            with pytest.raises(NotImplementedError, match=f"model_type='{other.model_type}'"):
                mod.check_supported(_Holder(other))
    with pytest.raises(NotImplementedError, match="model_type='nomic_bert'"):
        eurobert.check_supported(_Holder(_nomic_cfg()))
    with pytest.raises(NotImplementedError, match="model_type='eurobert'"):
        nomic_bert.check_supported(_Holder(_euro_cfg()))


# ---------------------------------------------------------------------------------------------------------- model wiring
def _tiny(kind, **kw):
    from transformers import EuroBertModel, NomicBertModel
    torch.manual_seed(0)
    return EuroBertModel(_euro_cfg(**kw)) if kind == "eurobert" else NomicBertModel(_nomic_cfg(**kw))


@pytest.mark.parametrize("kind", ["eurobert", "nomic_bert"])
def test_model_dispatches_the_new_encoders(kind):
    """Fails on the commit before these encoders: ``bert.check_supported`` raises NotImplementedError for both model types."""
    import gmlm_amd
    from gmlm_amd import bert, eurobert, llama, model as model_mod, nomic_bert
    plm = _tiny(kind)
    model = gmlm_amd.GraphTextLM(12, 16, 3, plm_encoder=plm)
    mod = eurobert if kind == "eurobert" else nomic_bert
    assert model._enc is mod and model._enc is not bert and model._enc is not llama and model._plm_kind == kind
    assert model_mod._ENCODERS[kind] == (mod, f"{kind}_encode", f"{kind}_encode_packed")
    assert callable(getattr(mod, f"{kind}_encode")) and callable(getattr(mod, f"{kind}_encode_packed"))
    assert model._has_packed_pass() and model._packed_head_dim() == 0      # its own packed pass; no bucketed / recorded form
    with pytest.raises(NotImplementedError, match="BERT-geometry encoders only"):
        model.capture_hip_graphs(torch.zeros(4, 12), torch.zeros(2, 4, dtype=torch.long))
    keys = {k[len("plm_encoder."):] for k in model.state_dict() if k.startswith("plm_encoder.")}
    assert keys == set(plm.state_dict())
    if kind == "eurobert":
        assert {"embed_tokens.weight", "norm.weight", "layers.0.self_attn.q_proj.weight", "layers.1.self_attn.o_proj.weight",
                "layers.0.mlp.gate_proj.weight", "layers.1.post_attention_layernorm.weight"} <= keys
    else:
        assert {"embeddings.word_embeddings.weight", "embeddings.token_type_embeddings.weight", "embeddings.LayerNorm.bias",
                "layers.0.self_attn.q_proj.weight", "layers.1.mlp.down_proj.weight", "layers.1.post_mlp_layernorm.weight"} <= keys


def test_prepare_weights_fuses_the_projections_and_carries_the_biases_the_model_has():
    from gmlm_amd import eurobert, nomic_bert
    for kw, has_bias in (({}, False), (dict(attention_bias=True), True)):
        plm = _tiny("eurobert", **kw)
        with torch.no_grad():
            for p in plm.parameters():
                if p.dim() == 1:
                    p.normal_()
        lws = eurobert.prepare_weights(plm, torch.float32)
        assert len(lws) == 2
        for lw, layer in zip(lws, plm.layers):
            sa, mlp = layer.self_attn, layer.mlp
            assert tuple(lw.wqkv.shape) == (256, 128) and not lw.wqkv.requires_grad       # (2 + 2 * 1) heads of 64
            assert torch.equal(lw.wqkv, torch.cat([sa.q_proj.weight, sa.k_proj.weight, sa.v_proj.weight]))
            assert torch.equal(lw.wgu, torch.cat([mlp.gate_proj.weight, mlp.up_proj.weight]))
            assert torch.equal(lw.wo, sa.o_proj.weight) and torch.equal(lw.wdown, mlp.down_proj.weight)
            assert (lw.bqkv is not None) == has_bias and (lw.bo is not None) == has_bias
            if has_bias:
                assert torch.equal(lw.bqkv, torch.cat([sa.q_proj.bias, sa.k_proj.bias, sa.v_proj.bias])) and torch.equal(lw.bo, sa.o_proj.bias)
                assert lw.m_qkv == (sa.q_proj.weight, sa.k_proj.weight, sa.v_proj.weight, sa.q_proj.bias, sa.k_proj.bias, sa.v_proj.bias)
            else:
                assert lw.m_qkv == (sa.q_proj.weight, sa.k_proj.weight, sa.v_proj.weight)
            assert lw.m_wo == ((sa.o_proj.weight, sa.o_proj.bias) if has_bias else (sa.o_proj.weight,))
            assert lw.ln1 is layer.input_layernorm.weight and lw.ln2 is layer.post_attention_layernorm.weight
    plm = _tiny("nomic_bert")
    lws = nomic_bert.prepare_weights(plm, torch.float32)
    assert len(lws) == 2
    for lw, layer in zip(lws, plm.layers):
        sa, mlp = layer.self_attn, layer.mlp
        assert tuple(lw.wqkv.shape) == (384, 128) and not lw.wqkv.requires_grad
        assert torch.equal(lw.wqkv, torch.cat([sa.q_proj.weight, sa.k_proj.weight, sa.v_proj.weight]))
        assert tuple(lw.wgu.shape) == (384, 128) and torch.equal(lw.wgu, torch.cat([mlp.gate_proj.weight, mlp.up_proj.weight]))
        assert torch.equal(lw.wo, sa.o_proj.weight) and torch.equal(lw.wdown, mlp.down_proj.weight)
        assert lw.m_qkv == (sa.q_proj.weight, sa.k_proj.weight, sa.v_proj.weight) and lw.m_wo == (sa.o_proj.weight,)
        assert lw.m_gu == (mlp.gate_proj.weight, mlp.up_proj.weight) and lw.m_down == (mlp.down_proj.weight,)
        assert lw.ln1 is layer.post_attention_layernorm and lw.ln2 is layer.post_mlp_layernorm
        assert not any(hasattr(lw, b) for b in ("bqkv", "bo"))              # the model has no projection bias
    for mod, kind in ((eurobert, "eurobert"), (nomic_bert, "nomic_bert")):
        with pytest.raises(ValueError):
            mod.prepare_weights(_tiny(kind), torch.bfloat16, "bf16x3")      # gemm_precision is passed through and checked


def test_nomic_bert_rope_table_is_the_hf_rotary_embedding_at_theta_1000():
    from gmlm_amd import nomic_bert, ops
    import inspect
    plm = _tiny("nomic_bert")
    assert plm.config.rope_parameters["rope_theta"] == 1000.0
    n = 300
    table = nomic_bert.rope_table(plm, n, "cpu")
    assert table.dtype == torch.float32 and table.shape[0] >= n and tuple(table.shape[1:]) == (2, 32) and table.is_contiguous()
    assert "(2, 32)" in inspect.getsource(ops.rope64_)                      # the layout ops.rope64_ checks for
    cos, sin = plm.rotary_emb(torch.zeros(1, 1), torch.arange(n)[None])                                   # [1, n, 64]: (freqs, freqs)
    assert torch.equal(cos[0, :, :32], cos[0, :, 32:])
    assert torch.equal(table[:n, 0], cos[0, :, :32]) and torch.equal(table[:n, 1], sin[0, :, :32])
    inv = 1.0 / (10000.0 ** (torch.arange(0, 64, 2, dtype=torch.float) / 64))
    assert not torch.equal(table[:n, 0], (torch.arange(n, dtype=torch.float32)[:, None] * inv[None]).cos())   # not the usual theta
    other = _tiny("nomic_bert", rope_parameters=dict(rope_type="default", rope_theta=500.0))
    assert not torch.equal(nomic_bert.rope_table(other, n, "cpu")[:n], table[:n])                          # the model's own theta is read


def test_encoders_refuse_a_sequence_past_the_position_table():
    from gmlm_amd import eurobert, nomic_bert
    z = torch.zeros(8, dtype=torch.long)
    for mod, kind in ((eurobert, "eurobert"), (nomic_bert, "nomic_bert")):
        plm = _tiny(kind)
        with pytest.raises(ValueError, match="sequence length 513 exceeds max_position_embeddings 512"):
            getattr(mod, f"{kind}_encode")(plm, torch.zeros(1, 513, dtype=torch.long), torch.tensor([513], dtype=torch.int32), torch.float32)
        with pytest.raises(ValueError):
            getattr(mod, f"{kind}_encode_packed")(plm, z, z[:7], torch.tensor([0, 8], dtype=torch.int32), 8, torch.float32)


# --------------------------------------------------------------------------------------------------------- code objects
def test_bidir_kernels_are_the_ones_the_gpu_tests_run():
    from test_gpu_bidir_kernels import UNREACHABLE, expected_kernels
    want = expected_kernels()
    got = _compiled_kernels(lambda name: name.startswith("bidir::"))
    assert len(want) == 2 * 2 * 4 and not UNREACHABLE                     # dtype x head dim x (fwd, delta, dq, dkv)
    assert got == want, (sorted(got - want), sorted(want - got))


def test_bidir_kernels_have_no_private_segment():
    """No spill (a zero private segment in every kernel's metadata) and no scratch traffic; the attention kernels run on the
    matrix pipe."""
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libgmlm_hip.so not built")
    if not all(os.path.exists(os.path.join(LLVM, t)) for t in ("llvm-readelf", "llvm-objdump", "llvm-objcopy")):
        pytest.skip("ROCm llvm tools not found")
    tmp = tempfile.mkdtemp()
    try:
        private, bodies = {}, {}
        for co in _code_objects(_lib.LIB_PATH, tmp):
            notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", co], check=True, capture_output=True, text=True).stdout
            for m in re.finditer(r"\.name:\s+(_ZN4gmlm5bidir\w+)\s+\.private_segment_fixed_size:\s+(\d+)", notes):
                private[m.group(1)] = int(m.group(2))
            dis = subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-d", "--mcpu=gfx950", co], check=True, capture_output=True,
                                 text=True).stdout
            for m in re.finditer(r"^[0-9a-f]+ <(_ZN4gmlm5bidir\w+)>:\n(.*?)(?=^[0-9a-f]+ <|\Z)", dis, re.S | re.M):
                bodies[m.group(1)] = m.group(2)
        assert len(private) == 16 and set(private) == set(bodies), (sorted(private), sorted(bodies))
        assert not {n: v for n, v in private.items() if v}, private
        for name, body in bodies.items():
            if "delta" not in name:
                assert "v_mfma" in body, name
            assert not re.search(r"v_pk_\w+_f32", body), name
            assert "scratch_" not in body, name
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
