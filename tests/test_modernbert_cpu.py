"""Host side of the ModernBERT text encoder (no GPU needed): the sixth header (include/gmlm_hip_modernbert.h), its ctypes table
and the exported symbols agree type by type and share no name with the other five tables; the entry points decide every
documented refusal and the nothing-to-do cases before any launch; ``modernbert.check_supported`` names each problem, and all
of them at once; the rope tables of both layer types are those of ``ModernBertRotaryEmbedding``; the model layer routes a
ModernBERT encoder to ``gmlm_amd.modernbert``; the routing rule of the attention is the pure function ``ops.window_cuts``;
and the ``mbert::`` kernels of the built code objects are the ones tests/test_gpu_modernbert_kernels.py runs, none with a
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
HEADER = os.path.join(ROOT, "include", "gmlm_hip_modernbert.h")

no_device = pytest.mark.skipif(torch.cuda.device_count() > 0,
                               reason="fabricated addresses: only meaningful (and only safe) without a device")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libgmlm_hip.so not built")
    return _lib.lib()


# ------------------------------------------------------------------------------------------------------------------ ABI
ENTRY_POINTS = ["gmlm_add_layernorm_bwd", "gmlm_add_layernorm_bwd_workspace_bytes", "gmlm_add_layernorm_fwd",
                "gmlm_attention_window_bwd", "gmlm_attention_window_fwd", "gmlm_attention_window_workspace_bytes",
                "gmlm_geglu_bwd", "gmlm_geglu_fwd", "gmlm_rope64_bwd", "gmlm_rope64_fwd"]


def test_header_ctypes_table_and_exports_agree(lib):
    protos = parse_header(open(HEADER).read())
    assert sorted(protos) == ENTRY_POINTS
    assert not signature_mismatches(protos, _lib.SIGNATURES_MODERNBERT)
    for name in protos:
        assert hasattr(lib, name), f"{name} declared in include/gmlm_hip_modernbert.h but not exported"
    assert _lib.SIGNATURE_TABLES[-1] is _lib.SIGNATURES_MODERNBERT and len(_lib.SIGNATURE_TABLES) == 6
    others = set().union(*(set(t) for t in _lib.SIGNATURE_TABLES[:-1]))
    assert not set(_lib.SIGNATURES_MODERNBERT) & others


def test_layernorm_bound_is_stated_once():
    from gmlm_amd import ops
    m = re.search(r"#define GMLM_ADD_LAYERNORM_MAX_F (\d+)", open(HEADER).read())
    assert m and int(m.group(1)) == ops.ADD_LAYERNORM_MAX_F >= 1024


_BASE = dict(q=A, k=A, v=A, kv_len=None, b=1, h=12, lq=64, lk=64, d=64, q_stride=2304, k_stride=2304, v_stride=2304, scale=0.125,
             dropout_p=0.0, window=16, out=A, out_lo=None, lse=A, dtype=BF16, cu_seqlens=None, max_len=0, stream=None,
             dout=A, dq=A, dk=A, dv=A, dq_stride=2304, dk_stride=2304, dv_stride=2304, workspace=A, workspace_bytes=1 << 40)
_FWD = ("q k v kv_len b h lq lk d q_stride k_stride v_stride scale dropout_p window out out_lo lse dtype cu_seqlens max_len "
        "stream").split()
_BWD = ("q k v out out_lo dout lse kv_len b h lq lk d q_stride k_stride v_stride scale dropout_p window dq dk dv dq_stride dk_stride "
        "dv_stride dtype cu_seqlens max_len workspace workspace_bytes stream").split()


def _call(lib, which, **mut):
    a = dict(_BASE, **mut)
    fn, names = (lib.gmlm_attention_window_fwd, _FWD) if which == "fwd" else (lib.gmlm_attention_window_bwd, _BWD)
    return fn(*[a[n] for n in names]), lib.gmlm_last_error()


def test_argument_lists_follow_the_header():
    protos = parse_header(open(HEADER).read())
    assert [n for _, n in protos["gmlm_attention_window_fwd"][1]] == _FWD
    assert [n for _, n in protos["gmlm_attention_window_bwd"][1]] == _BWD


_REFUSALS = [
    (dict(d=32), b"head dim"), (dict(d=96), b"head dim"), (dict(d=128), b"head dim"),
    (dict(dtype=2), b"dtype"),
    (dict(lk=65), b"lq == lk"), (dict(lq=63), b"lq == lk"),
    (dict(window=-1), b"window"), (dict(window=1 << 30), b"window"),
    (dict(dropout_p=0.1), b"dropout"),
    (dict(scale=0.0), b"scale"),
    (dict(b=-1), b"bad sizes"), (dict(h=0), b"bad sizes"),
    (dict(q_stride=760), b"stride"),                                    # below h * 64
    (dict(q_stride=2308), b"stride"),                                   # bf16: not a multiple of 8 elements
    (dict(dtype=F32, k_stride=2306), b"stride"),                        # fp32: not a multiple of 4 elements
    (dict(v_stride=1 << 24), b"stride"),
    (dict(q=A + 8), b"aligned"), (dict(k=None), b"null"),
    (dict(cu_seqlens=A, max_len=0), b"packed mode"),
    (dict(cu_seqlens=A, max_len=64, kv_len=A), b"packed mode"),
    (dict(out_lo=A, dtype=F32), b"out_lo"), (dict(out_lo=A + 8), b"out_lo"),
    (dict(b=(1 << 31) // 12 + 1, lq=1, lk=1), b"too many work items"),
]


@no_device
@pytest.mark.parametrize("which", ["fwd", "bwd"])
@pytest.mark.parametrize("mut,msg", _REFUSALS, ids=[",".join(f"{k}={v}" for k, v in m.items()) for m, _ in _REFUSALS])
def test_window_attention_refusals_are_decided_on_the_host(lib, which, mut, msg):
    rc, err = _call(lib, which, **mut)
    assert rc == EINVAL and msg in err, (mut, rc, err)


@no_device
def test_valid_window_calls_reach_the_launch(lib):
    for which in ("fwd", "bwd"):
        for mut in (dict(), dict(dtype=F32), dict(cu_seqlens=A, max_len=64), dict(kv_len=A), dict(out_lo=A), dict(window=0),
                    dict(window=(1 << 30) - 1), dict(b=(1 << 31) // 12 - 1, lq=1, lk=1)):
            rc, err = _call(lib, which, **mut)
            assert rc == ELAUNCH, (which, mut, rc, err)


@no_device
def test_window_backward_workspace_boundary(lib):
    need = lib.gmlm_attention_window_workspace_bytes(2, 12, 300)
    assert need == 2 * 12 * 300 * 4 and lib.gmlm_attention_window_workspace_bytes(0, 12, 0) > 0
    shape = dict(b=2, lq=300, lk=300)
    assert _call(lib, "bwd", workspace_bytes=need, **shape)[0] == ELAUNCH
    rc, err = _call(lib, "bwd", workspace_bytes=need - 1, **shape)
    assert rc == EWORKSPACE and b"workspace" in err
    assert _call(lib, "bwd", workspace=None, **shape)[0] == EWORKSPACE
    packed = dict(b=7, lq=300, lk=300, cu_seqlens=A, max_len=100)        # delta is [h, total_rows] whatever the number of sequences
    need = lib.gmlm_attention_window_workspace_bytes(1, 12, 300)
    assert _call(lib, "bwd", workspace_bytes=need, **packed)[0] == ELAUNCH
    assert _call(lib, "bwd", workspace_bytes=need - 1, **packed)[0] == EWORKSPACE


@no_device
def test_nothing_to_do_needs_no_pointer_but_sizes_are_still_checked(lib):
    nothing = dict(q=None, k=None, v=None, out=None, lse=None, dout=None, dq=None, dk=None, dv=None, workspace=None, workspace_bytes=0)
    for empty in (dict(b=0), dict(lq=0, lk=0), dict(lq=0, lk=0, cu_seqlens=A, max_len=1)):
        for which in ("fwd", "bwd"):
            assert _call(lib, which, **nothing, **empty)[0] == OK, (which, empty)
            rc, err = _call(lib, which, **nothing, **empty, d=128)
            assert rc == EINVAL and b"head dim" in err
    # the row kernels: zero rows / tokens return GMLM_OK before any pointer is examined, sizes and dtype first
    assert lib.gmlm_add_layernorm_fwd(None, None, None, None, 0, 768, 1e-5, None, None, None, None, BF16, None) == OK
    assert lib.gmlm_add_layernorm_fwd(None, None, None, None, 0, 772, 1e-5, None, None, None, None, BF16, None) == EINVAL
    assert lib.gmlm_geglu_fwd(None, 0, 1152, None, BF16, None) == OK and lib.gmlm_geglu_bwd(None, None, 0, 1152, None, F32, None) == OK
    assert lib.gmlm_geglu_fwd(None, 0, 1150, None, F32, None) == EINVAL
    for fn in (lib.gmlm_rope64_fwd, lib.gmlm_rope64_bwd):
        assert fn(None, 2304, None, 8192, 0, 0, None, 12, 64, BF16, None) == OK           # padded [b, 0]
        assert fn(None, 2304, None, 8192, 0, 0, A, 12, 64, F32, None) == OK               # packed, no row
        assert fn(None, 2304, None, 8192, 0, 0, None, 12, 128, BF16, None) == EINVAL and b"head dim" in lib.gmlm_last_error()


@no_device
def test_row_kernel_refusals_are_decided_on_the_host(lib):
    ln = lambda f=768, dtype=BF16, a=A, b=None, s=None: lib.gmlm_add_layernorm_fwd(a, b, A, None, 4, f, 1e-5, s, A, A, A, dtype, None)
    assert ln() == ELAUNCH and ln(f=1024) == ELAUNCH and ln(f=4096, dtype=F32) == ELAUNCH and ln(b=A, s=A) == ELAUNCH
    assert ln(f=772) == EINVAL and b"multiple of 8" in lib.gmlm_last_error()
    assert ln(f=770, dtype=F32) == EINVAL and b"multiple of 4" in lib.gmlm_last_error()
    assert ln(f=4104) == EINVAL and b"4096" in lib.gmlm_last_error()
    assert ln(f=8192, dtype=F32) == EINVAL and b"4096" in lib.gmlm_last_error()
    assert ln(b=A) == EINVAL and b"exactly when" in lib.gmlm_last_error()                # b without s
    assert ln(a=A + 2) == EINVAL and b"aligned" in lib.gmlm_last_error()
    assert ln(dtype=3) == EINVAL and b"dtype" in lib.gmlm_last_error()
    bwd = lambda ws=1 << 30, dbeta=None, f=768: lib.gmlm_add_layernorm_bwd(A, None, A, A, A, A, 64, f, A, A, dbeta, BF16, A, ws, None)
    assert bwd() == ELAUNCH and bwd(dbeta=A + 4 * 768) == ELAUNCH
    assert bwd(ws=8) == EWORKSPACE
    assert bwd(dbeta=A + 16) == EINVAL and b"[2, f]" in lib.gmlm_last_error()
    assert bwd(f=4104) == EINVAL
    assert lib.gmlm_add_layernorm_bwd_workspace_bytes(64, 768) <= 1 << 30

    rope = lambda **k: lib.gmlm_rope64_fwd(k.get("qkv", A), k.get("stride", 2304), A, k.get("max_len", 64), 16, k.get("l", 8),
                                           k.get("pos", None), 12, k.get("d", 64), k.get("dtype", BF16), None)
    assert rope() == ELAUNCH and rope(pos=A, l=0) == ELAUNCH
    assert rope(d=128) == EINVAL and b"head dim" in lib.gmlm_last_error()
    assert rope(stride=1536) == EINVAL and b"stride" in lib.gmlm_last_error()              # narrower than 3 * h * 64
    assert rope(stride=2308) == EINVAL and b"stride" in lib.gmlm_last_error()
    assert rope(l=128) == EINVAL and b"table" in lib.gmlm_last_error()
    assert rope(l=0) == EINVAL and b"length 0" in lib.gmlm_last_error()
    assert rope(max_len=0) == EINVAL and b"table" in lib.gmlm_last_error()
    assert rope(qkv=A + 8) == EINVAL and b"aligned" in lib.gmlm_last_error()

    assert lib.gmlm_geglu_fwd(A, 4, 1152, A, BF16, None) == ELAUNCH
    assert lib.gmlm_geglu_fwd(A, 4, 100, A, BF16, None) == EINVAL and b"multiple of 8" in lib.gmlm_last_error()
    assert lib.gmlm_geglu_bwd(A, A + 8, 4, 384, A, BF16, None) == EINVAL and b"aligned" in lib.gmlm_last_error()
    assert lib.gmlm_geglu_bwd(A, A, 4, 384, None, F32, None) == EINVAL


def test_new_ops_fail_loudly_without_a_gpu(lib):
    """CPU tensors raise the library's error: no eager fallback behind the new operators."""
    from gmlm_amd import ops
    x = torch.zeros(1, 4, 768)
    with pytest.raises(_lib.GmlmHipError):
        ops.add_layernorm(x, None, torch.ones(768))
    with pytest.raises(_lib.GmlmHipError):
        ops.geglu(x)
    with pytest.raises(_lib.GmlmHipError):
        ops.rope_attention(torch.zeros(1, 4, 384) * 1.0, torch.zeros(8, 2, 32), None, 2, 0.125, "sliding_attention", 1)
    with pytest.raises(_lib.GmlmHipError):
        ops.rope_attention_varlen(torch.zeros(4, 384) * 1.0, torch.zeros(8, 2, 32), torch.arange(4), torch.tensor([0, 4], dtype=torch.int32),
                                  4, 2, 0.125, "sliding_attention", 1)


# --------------------------------------------------------------------------------------------------------- check_supported
def _cfg(**kw):
    from transformers import ModernBertConfig
    base = dict(vocab_size=96, hidden_size=128, intermediate_size=192, num_hidden_layers=4, num_attention_heads=2,
                max_position_embeddings=512, local_attention=32, global_attn_every_n_layers=3, pad_token_id=None, bos_token_id=None,
                eos_token_id=None, cls_token_id=None, sep_token_id=None)
    base.update(kw)
    return ModernBertConfig(**base)


class _Holder:
    def __init__(self, config):
        self.config = config


def test_check_supported_accepts_a_modernbert_config():
    from gmlm_amd import modernbert
    cfg = _cfg()
    modernbert.check_supported(_Holder(cfg))
    assert cfg.layer_types == ["full_attention", "sliding_attention", "sliding_attention", "full_attention"]
    assert cfg.sliding_window == 16 and modernbert.head_dim(cfg) == 64


def _rope(layer_type):
    rp = {lt: {"rope_type": "default", "rope_theta": 10000.0} for lt in ("full_attention", "sliding_attention")}
    rp[layer_type] = {"rope_type": "linear", "factor": 2.0, "rope_theta": 10000.0}
    return dict(rope_parameters=rp)


_PROBLEMS = [
    (dict(num_attention_heads=4), "head_dim=32"),
    (dict(hidden_activation="silu"), "hidden_activation='silu'"),
    (dict(attention_bias=True), "attention_bias"), (dict(mlp_bias=True), "mlp_bias"), (dict(norm_bias=True), "norm_bias"),
    (dict(attention_dropout=0.1), "attention_dropout=0.1"), (dict(embedding_dropout=0.1), "embedding_dropout=0.1"),
    (dict(mlp_dropout=0.2), "mlp_dropout=0.2"),
    (_rope("full_attention"), "rope type 'linear' for full_attention"),
    (_rope("sliding_attention"), "rope type 'linear' for sliding_attention"),
    (dict(layer_types=["full_attention", "chunked_attention", "sliding_attention", "full_attention"]), "chunked_attention"),
    (dict(hidden_size=8192, num_attention_heads=128), "hidden_size=8192"),
]


@pytest.mark.parametrize("kw,word", _PROBLEMS, ids=[w for _, w in _PROBLEMS])
def test_check_supported_names_each_problem(kw, word):
    from gmlm_amd import modernbert
    cfg = _cfg()
    for k, v in kw.items():                      # set on the config: its constructor validates some of these away
        setattr(cfg, k, v)
    with pytest.raises(NotImplementedError) as e:
        modernbert.check_supported(_Holder(cfg))
    assert word in str(e.value), str(e.value)


def test_check_supported_names_every_problem_at_once():
    from gmlm_amd import modernbert
    cfg = _cfg()
    for kw, _ in _PROBLEMS[:9] + _PROBLEMS[10:11]:
        for k, v in kw.items():
            setattr(cfg, k, v)
    cfg.model_type = "bert"
    with pytest.raises(NotImplementedError) as e:
        modernbert.check_supported(_Holder(cfg))
    for word in ["model_type='bert'"] + [w for _, w in _PROBLEMS[:9] + _PROBLEMS[10:11]]:
        assert word in str(e.value), (word, str(e.value))


def test_other_encoder_modules_refuse_modernbert_and_it_refuses_them():
    from gmlm_amd import bert, modernbert, qwen3
    from transformers import BertConfig
    for mod in (bert, qwen3):
        with pytest.raises(NotImplementedError):
            mod.check_supported(_Holder(_cfg()))
    with pytest.raises(NotImplementedError, match="model_type='bert'"):
        modernbert.check_supported(_Holder(BertConfig(hidden_size=128, num_attention_heads=2)))


# ------------------------------------------------------------------------------------------------------------ rope tables
def test_rope_tables_match_the_hf_rotary_embedding_for_both_thetas():
    from gmlm_amd import modernbert
    from transformers.models.modernbert.modeling_modernbert import ModernBertRotaryEmbedding
    cfg = _cfg()
    thetas = {lt: modernbert.rope_theta(cfg, lt) for lt in modernbert.LAYER_TYPES}
    assert thetas["full_attention"] != thetas["sliding_attention"] and set(thetas.values()) == {160000.0, 10000.0}
    emb = ModernBertRotaryEmbedding(cfg)
    for lt in modernbert.LAYER_TYPES:
        cs = modernbert.rope_table(cfg, lt, 40, "cpu")
        assert cs.shape[0] >= 40 and tuple(cs.shape[1:]) == (2, 32) and cs.dtype == torch.float32 and cs.is_contiguous()
        assert modernbert.rope_table(cfg, lt, 17, "cpu") is cs                  # built once, shorter sequences read a prefix
        cos, sin = emb(torch.zeros(1, 40, 8), torch.arange(40)[None], lt)
        assert cos.dtype == torch.float32
        cs = cs[:40]
        assert torch.equal(cs[:, 0], cos[0, :, :32]) and torch.equal(cs[:, 0], cos[0, :, 32:])
        assert torch.equal(cs[:, 1], sin[0, :, :32]) and torch.equal(cs[:, 1], sin[0, :, 32:])
    assert modernbert.rope_table(cfg, "full_attention", 8, "cpu") is not modernbert.rope_table(cfg, "sliding_attention", 8, "cpu")


# ---------------------------------------------------------------------------------------------------------- model wiring
def _tiny_model(**kw):
    import gmlm_amd
    from transformers import ModernBertModel
    torch.manual_seed(0)
    plm = ModernBertModel(_cfg(**kw))
    return gmlm_amd.GraphTextLM(12, 16, 3, plm_encoder=plm, plm_tokenizer=None), plm


def test_model_dispatches_a_modernbert_encoder():
    from gmlm_amd import bert, modernbert
    model, plm = _tiny_model()
    assert model._enc is modernbert and model._enc is not bert
    assert model._has_packed_pass() and model._packed_head_dim() == 0      # its own packed pass; no bucketed / recorded form
    with pytest.raises(NotImplementedError, match="BERT"):
        model.capture_hip_graphs(torch.zeros(4, 12), torch.zeros(2, 4, dtype=torch.long))
    keys = {k[len("plm_encoder."):] for k in model.state_dict() if k.startswith("plm_encoder.")}
    assert keys == set(plm.state_dict())
    assert {"embeddings.tok_embeddings.weight", "layers.1.attn_norm.weight", "layers.0.attn.Wqkv.weight", "layers.3.mlp.Wi.weight",
            "final_norm.weight"} <= keys and "layers.0.attn_norm.weight" not in keys


def test_prepare_weights_packs_the_four_operands_of_each_layer():
    from gmlm_amd import modernbert
    _, plm = _tiny_model()
    lws = modernbert.prepare_weights(plm, torch.float32)
    assert [lw.kind for lw in lws] == plm.config.layer_types and lws[0].ln1 is None and lws[1].ln1 is plm.layers[1].attn_norm.weight
    for lw, layer in zip(lws, plm.layers):
        assert torch.equal(lw.wqkv, layer.attn.Wqkv.weight) and tuple(lw.wqkv.shape) == (384, 128)
        assert torch.equal(lw.wo, layer.attn.Wo.weight) and torch.equal(lw.wi, layer.mlp.Wi.weight) and tuple(lw.wi.shape) == (384, 128)
        assert torch.equal(lw.wmo, layer.mlp.Wo.weight) and not lw.wqkv.requires_grad
        assert lw.m_qkv == (layer.attn.Wqkv.weight,) and lw.m_mo == (layer.mlp.Wo.weight,)
    with pytest.raises(ValueError):
        modernbert.prepare_weights(plm, torch.bfloat16, "bf16x3")           # gemm_precision is passed through and checked


def test_encoder_refuses_a_sequence_past_max_position_embeddings():
    from gmlm_amd import modernbert
    _, plm = _tiny_model(max_position_embeddings=16)
    with pytest.raises(ValueError, match="max_position_embeddings"):
        modernbert.modernbert_encode(plm, torch.zeros(1, 17, dtype=torch.long), torch.tensor([17], dtype=torch.int32), torch.float32)
    z = torch.zeros(17, dtype=torch.long)
    with pytest.raises(ValueError, match="max_position_embeddings"):
        modernbert.modernbert_encode_packed(plm, z, z, torch.tensor([0, 17], dtype=torch.int32), 17, torch.float32)


# --------------------------------------------------------------------------------------------------------- routing rule
@pytest.mark.parametrize("layer_type,window,max_len,cuts", [
    ("full_attention", 64, 8192, False), ("full_attention", 0, 2, False),
    ("sliding_attention", 64, 64, False), ("sliding_attention", 64, 65, False),     # |i - j| <= 64 spans 65 tokens: vacuous
    ("sliding_attention", 64, 66, True), ("sliding_attention", 64, 512, True),
    ("sliding_attention", 16, 17, False), ("sliding_attention", 16, 18, True),
    ("sliding_attention", 0, 1, False), ("sliding_attention", 0, 2, True),
])
def test_routing_rule_is_a_pure_function(layer_type, window, max_len, cuts):
    from gmlm_amd import ops
    assert ops.window_cuts(layer_type, window, max_len) is cuts
    if not cuts and layer_type == "sliding_attention":                               # vacuous: no pair of the longest sequence is hidden
        i = torch.arange(max_len)
        assert bool(((i[:, None] - i[None, :]).abs() <= window).all())


# --------------------------------------------------------------------------------------------------------- code objects
def _is_mbert(name):
    return name.startswith("mbert::") or "mbert::LnDwFn" in name


def test_mbert_kernels_are_the_ones_the_gpu_tests_run():
    tn = ("unsigned short", "float")
    want = {f"mbert::window_{k}_kernel<{t}>" for k in ("fwd", "delta", "dq", "dkv") for t in tn}
    want |= {f"mbert::add_ln_{k}_kernel<{t}, {ch}>" for k in ("fwd", "bwd") for t, chs in zip(tn, ((2, 4, 8), (2, 4, 8, 16))) for ch in chs}
    want |= {f"mbert::rope64_kernel<{t}, {inv}>" for t in tn for inv in ("false", "true")}
    want |= {f"mbert::geglu_{k}_kernel<{t}>" for k in ("fwd", "bwd") for t in tn}
    want |= {f"col_reduce_partial_kernel<{k}, gmlm::mbert::LnDwFn<{t}, {k}> >" for k in (1, 2) for t in tn}
    got = _compiled_kernels(_is_mbert)
    norm = lambda s: {n.replace(" >", ">") for n in s}
    assert norm(got) == norm(want), (sorted(norm(got) - norm(want)), sorted(norm(want) - norm(got)))


def test_mbert_kernels_have_no_private_segment_and_no_packed_fp32():
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
            for m in re.finditer(r"\.name:\s+(_ZN4gmlm5mbert\w+)\s+\.private_segment_fixed_size:\s+(\d+)", notes):
                private[m.group(1)] = int(m.group(2))
            dis = subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-d", "--mcpu=gfx950", co], check=True, capture_output=True,
                                 text=True).stdout
            for m in re.finditer(r"^[0-9a-f]+ <(_ZN4gmlm5mbert\w+)>:\n(.*?)(?=^[0-9a-f]+ <|\Z)", dis, re.S | re.M):
                bodies[m.group(1)] = m.group(2)
        assert len(private) == 8 + 14 + 4 + 4 and set(private) == set(bodies), (sorted(private), sorted(bodies))
        assert not {n: v for n, v in private.items() if v}, private
        for name, body in bodies.items():
            if "window_" in name and "delta" not in name:
                assert "v_mfma" in body, name
            assert not re.search(r"v_pk_(fma|mul|add)_f32", body), name
            assert "scratch_" not in body, name
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
