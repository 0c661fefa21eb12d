"""Host side of the DeBERTa-v2 / v3 text encoder (no GPU needed): the eighth header (include/gmlm_hip_disent.h), its ctypes table
``_lib.SIGNATURES_DISENT`` and the exported symbols agree type by type and share no name with any other table, the six of
``SIGNATURE_TABLES`` staying as they are; the entry points decide every documented refusal and the nothing-to-do cases before
any launch; ``deberta.bucket_columns`` is HF's ``build_relative_position`` read along i - j (for the p2c index as well);
``deberta.check_supported`` names each problem, and all of them at once; the model layer routes a DeBERTa encoder to
``gmlm_amd.deberta``; the prepared weights fuse Q / K / V and keep the masters; and the ``disent::`` kernels of the built code
objects are the ones tests/test_gpu_deberta_kernels.py runs, none with a private segment (spill) or packed-fp32 VALU."""
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
HEADER = os.path.join(ROOT, "include", "gmlm_hip_disent.h")

no_device = pytest.mark.skipif(torch.cuda.device_count() > 0,
                               reason="fabricated addresses: only meaningful (and only safe) without a device")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libgmlm_hip.so not built")
    return _lib.lib()


# ------------------------------------------------------------------------------------------------------------------ ABI
ENTRY_POINTS = ["gmlm_attention_disent_bwd", "gmlm_attention_disent_fwd", "gmlm_attention_disent_workspace_bytes"]


def test_header_ctypes_table_and_exports_agree(lib):
    protos = parse_header(open(HEADER).read())
    assert sorted(protos) == ENTRY_POINTS
    assert not signature_mismatches(protos, _lib.SIGNATURES_DISENT)
    for name in protos:
        assert hasattr(lib, name), f"{name} declared in include/gmlm_hip_disent.h but not exported"
        assert getattr(lib, name).argtypes == _lib.SIGNATURES_DISENT[name][1]                     # lib() bound the new table
    assert len(_lib.SIGNATURE_TABLES) == 6 and _lib.SIGNATURE_TABLES[-1] is _lib.SIGNATURES_MODERNBERT
    assert _lib.SIGNATURE_TABLES_LATER[-1] is _lib.SIGNATURES_DISENT and _lib.SIGNATURE_TABLES_LATER[0] is _lib.SIGNATURES_RELBIAS
    assert not any(t is _lib.SIGNATURES_DISENT for t in _lib.SIGNATURE_TABLES)
    others = set().union(*(set(t) for t in _lib.SIGNATURE_TABLES + _lib.SIGNATURE_TABLES_LATER if t is not _lib.SIGNATURES_DISENT))
    assert not set(_lib.SIGNATURES_DISENT) & others
    assert lib.gmlm_version() == 1


def test_table_bound_is_stated_once():
    from gmlm_amd import ops
    m = re.search(r"#define GMLM_DISENT_MAX_LEN (\d+)", open(HEADER).read())
    assert m and int(m.group(1)) == ops.DISENT_MAX_LEN == ops.RELBIAS_MAX_LEN == 512


_BASE = dict(q=A, k=A, v=A, kv_len=None, b=1, h=12, lq=64, lk=64, d=64, q_stride=2304, k_stride=2304, v_stride=2304, scale=0.0722,
             dropout_p=0.0, seed=0, seed_dev=None, c2p=A, p2c=A, col=A, col_m=64, tab_w=127, out=A, out_lo=None, lse=A, dtype=BF16,
             cu_seqlens=None, max_len=0, stream=None, dout=A, dq=A, dk=A, dv=A, d_c2p=A, d_p2c=A, dq_stride=2304, dk_stride=2304,
             dv_stride=2304, workspace=A, workspace_bytes=1 << 40)
_FWD = ("q k v kv_len b h lq lk d q_stride k_stride v_stride scale dropout_p seed seed_dev c2p p2c col col_m tab_w out out_lo lse dtype "
        "cu_seqlens max_len stream").split()
_BWD = ("q k v out out_lo dout lse kv_len b h lq lk d q_stride k_stride v_stride scale dropout_p seed seed_dev c2p p2c col col_m tab_w "
        "dq dk dv d_c2p d_p2c dq_stride dk_stride dv_stride dtype cu_seqlens max_len workspace workspace_bytes stream").split()


def _call(lib, which, **mut):
    a = dict(_BASE, **mut)
    fn, names = (lib.gmlm_attention_disent_fwd, _FWD) if which == "fwd" else (lib.gmlm_attention_disent_bwd, _BWD)
    return fn(*[a[n] for n in names]), lib.gmlm_last_error()


def test_argument_lists_follow_the_header():
    protos = parse_header(open(HEADER).read())
    assert [n for _, n in protos["gmlm_attention_disent_fwd"][1]] == _FWD
    assert [n for _, n in protos["gmlm_attention_disent_bwd"][1]] == _BWD
    assert [n for _, n in protos["gmlm_attention_disent_workspace_bytes"][1]] == "b h lq max_len".split()


_REFUSALS = [
    (dict(d=32), b"head dim"), (dict(d=96), b"head dim"), (dict(d=128), b"head dim"),
    (dict(dtype=2), b"dtype"),
    (dict(lk=65), b"lq == lk"), (dict(lq=63), b"lq == lk"),
    (dict(col_m=63), b"col_m"), (dict(col_m=0, tab_w=1), b"col_m"), (dict(col_m=513), b"col_m"),      # below the sequence, above 512
    (dict(lq=513, lk=513, col_m=513), b"col_m"), (dict(lq=600, lk=600, col_m=512), b"col_m"),
    (dict(cu_seqlens=A, lq=900, lk=900, max_len=65, col_m=64), b"col_m"),                             # packed: the longest sequence counts
    (dict(tab_w=0), b"tab_w"), (dict(tab_w=128), b"tab_w"), (dict(col_m=512, tab_w=1024), b"tab_w"),  # W outside [1, 2 col_m - 1]
    (dict(c2p=None), b"c2p"), (dict(p2c=A + 4), b"p2c"), (dict(col=None), b"col"), (dict(col=A + 4), b"col"),
    (dict(dropout_p=1.0), b"dropout"), (dict(dropout_p=-0.1), b"dropout"),
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
    (dict(b=(1 << 31) // 12 + 1, lq=1, lk=1, tab_w=1), b"too many work items"),
]


@no_device
@pytest.mark.parametrize("which", ["fwd", "bwd"])
@pytest.mark.parametrize("mut,msg", _REFUSALS, ids=[",".join(f"{k}={v}" for k, v in m.items()) for m, _ in _REFUSALS])
def test_disent_attention_refusals_are_decided_on_the_host(lib, which, mut, msg):
    rc, err = _call(lib, which, **mut)
    assert rc == EINVAL and msg in err, (mut, rc, err)


@no_device
def test_backward_refuses_a_null_or_misaligned_gradient_table(lib):
    for name in ("d_c2p", "d_p2c"):
        for bad in (None, A + 4):
            rc, err = _call(lib, "bwd", **{name: bad})
            assert rc == EINVAL and b"d_c2p / d_p2c" in err


@no_device
def test_valid_disent_calls_reach_the_launch(lib):
    for which in ("fwd", "bwd"):
        for mut in (dict(), dict(dtype=F32), dict(cu_seqlens=A, max_len=64), dict(cu_seqlens=A, lq=900, lk=900, max_len=64), dict(kv_len=A),
                    dict(out_lo=A), dict(dropout_p=0.1, seed=7, seed_dev=A), dict(col_m=512, tab_w=512), dict(lq=512, lk=512, col_m=512),
                    dict(tab_w=1), dict(lq=1, lk=1, col_m=1, tab_w=1), dict(b=(1 << 31) // 12 - 1, lq=1, lk=1, tab_w=1)):
            rc, err = _call(lib, which, **mut)
            assert rc == ELAUNCH, (which, mut, rc, err)


@no_device
def test_disent_backward_workspace_boundary(lib):
    need = lib.gmlm_attention_disent_workspace_bytes(2, 12, 300, 0)          # delta [b, h, l]
    assert need == 2 * 12 * 300 * 4 and lib.gmlm_attention_disent_workspace_bytes(0, 12, 0, 0) > 0
    shape = dict(b=2, lq=300, lk=300, col_m=320)
    assert _call(lib, "bwd", workspace_bytes=need, **shape)[0] == ELAUNCH
    rc, err = _call(lib, "bwd", workspace_bytes=need - 1, **shape)
    assert rc == EWORKSPACE and b"workspace" in err
    assert _call(lib, "bwd", workspace=None, **shape)[0] == EWORKSPACE
    packed = dict(b=7, lq=300, lk=300, cu_seqlens=A, max_len=100, col_m=100)     # delta [h, total_rows]
    need = lib.gmlm_attention_disent_workspace_bytes(7, 12, 300, 100)
    assert need == 12 * 300 * 4
    assert _call(lib, "bwd", workspace_bytes=need, **packed)[0] == ELAUNCH
    assert _call(lib, "bwd", workspace_bytes=need - 1, **packed)[0] == EWORKSPACE


@no_device
def test_nothing_to_do_needs_no_pointer_but_sizes_are_still_checked(lib):
    nothing = dict(q=None, k=None, v=None, out=None, lse=None, dout=None, dq=None, dk=None, dv=None, c2p=None, p2c=None, col=None,
                   d_c2p=None, d_p2c=None, workspace=None, workspace_bytes=0)
    for empty in (dict(b=0), dict(lq=0, lk=0), dict(lq=0, lk=0, cu_seqlens=A, max_len=1)):
        for which in ("fwd", "bwd"):
            assert _call(lib, which, **nothing, **empty)[0] == OK, (which, empty)
            rc, err = _call(lib, which, **nothing, **empty, d=128)
            assert rc == EINVAL and b"head dim" in err
            rc, err = _call(lib, which, **nothing, **empty, col_m=600)
            assert rc == EINVAL and b"col_m" in err


def test_new_op_fails_loudly_without_a_gpu(lib):
    """CPU tensors raise the library's error: no eager fallback behind the new operator."""
    from gmlm_amd import ops
    col = torch.zeros(7, dtype=torch.int32)
    with pytest.raises(_lib.GmlmHipError):
        ops.attention_disent_qkv(torch.zeros(1, 4, 384), torch.zeros(2, 4, 7), torch.zeros(2, 4, 7), col, None, 2, 0.07)
    with pytest.raises(_lib.GmlmHipError):
        ops.attention_disent_qkv_varlen(torch.zeros(4, 384), torch.zeros(2, 4, 7), torch.zeros(2, 4, 7), col,
                                        torch.tensor([0, 4], dtype=torch.int32), 4, 2, 0.07)


# ---------------------------------------------------------------------------------------------------------- bucket columns
@pytest.mark.parametrize("k,mx,m", [(256, 512, 512), (256, 512, 130), (16, 40, 40), (16, 40, 100), (8, 24, 24)])
def test_bucket_columns_are_hf_relative_positions_read_along_the_distance(k, mx, m):
    from gmlm_amd import deberta
    from transformers.models.deberta_v2.modeling_deberta_v2 import build_relative_position
    cols = deberta.bucket_columns(m, k, mx)
    assert cols.col.dtype == torch.int32 and cols.col.numel() == 2 * m - 1 and cols is deberta.bucket_columns(m, k, mx)   # cached
    x = torch.zeros(1, m, 4)
    rel = build_relative_position(x, x, bucket_size=k, max_position=mx)[0]                  # [m, m]: bucket of i - j
    i = torch.arange(m)
    ours = (cols.col.long() + cols.first)[(m - 1) + i[:, None] - i[None, :]]
    assert torch.equal(ours, torch.clamp(rel + k, 0, 2 * k - 1))                            # the c2p index
    assert torch.equal(ours, torch.clamp(-rel + k, 0, 2 * k - 1).t())                       # the p2c index, transposed as HF transposes it
    step = cols.col[1:] - cols.col[:-1]
    assert int(cols.col[0]) == 0 and int(cols.col[-1]) == cols.width - 1 and int(step.min()) >= 0 and int(step.max()) <= 1
    assert 1 <= cols.width <= min(2 * k, 2 * m - 1) and 0 <= cols.first and cols.first + cols.width <= 2 * k


def test_bucket_columns_clamp_past_max_relative_positions():
    from gmlm_amd import deberta
    cols = deberta.bucket_columns(100, 16, 40)
    assert cols.first == 0 and cols.width == 32
    rel = torch.arange(-99, 100)
    assert bool((cols.col[rel >= 39] == 31).all()) and bool((cols.col[rel <= -40] == 0).all())
    runs = torch.unique_consecutive(deberta.bucket_columns(40, 16, 40).col, return_counts=True)[1]
    assert int(runs.max()) == 8                                                               # the longest run below the clamp


# --------------------------------------------------------------------------------------------------------- check_supported
def _cfg(**kw):
    from transformers import DebertaV2Config
    base = dict(vocab_size=96, hidden_size=128, intermediate_size=192, num_hidden_layers=3, num_attention_heads=2,
                max_position_embeddings=128, relative_attention=True, pos_att_type=["p2c", "c2p"], share_att_key=True,
                norm_rel_ebd="layer_norm", position_buckets=16, max_relative_positions=40, position_biased_input=False,
                type_vocab_size=0, layer_norm_eps=1e-7)
    base.update(kw)
    return DebertaV2Config(**base)


class _Holder:
    def __init__(self, config):
        self.config = config


def test_check_supported_accepts_a_v3_config():
    from gmlm_amd import deberta
    cfg = _cfg()
    deberta.check_supported(_Holder(cfg))
    assert cfg.model_type == "deberta-v2" and cfg.hidden_act == "gelu"
    deberta.check_supported(_Holder(_cfg(hidden_size=768, num_attention_heads=12, position_buckets=256, max_relative_positions=-1,
                                         max_position_embeddings=512)))                       # deberta-v3-base
    assert deberta.max_sequence(cfg) == 512 and deberta.max_relative(cfg) == 40
    assert deberta.max_relative(_cfg(max_relative_positions=-1)) == 128


_PROBLEMS = [
    (dict(num_attention_heads=4), "head_dim=32"),
    (dict(relative_attention=False), "relative_attention=False"),
    (dict(pos_att_type=["c2p"]), "pos_att_type=['c2p']"),
    (dict(share_att_key=False), "share_att_key=False"),
    (dict(norm_rel_ebd="none"), "norm_rel_ebd='none'"),
    (dict(position_buckets=-1), "position_buckets=-1"),
    (dict(position_biased_input=True), "position_biased_input=True"),
    (dict(type_vocab_size=2), "type_vocab_size=2"),
    (dict(embedding_size=64), "embedding_size=64"),
    (dict(conv_kernel_size=3), "conv_kernel_size=3"),
    (dict(hidden_act="relu"), "hidden_act='relu'"),
]


@pytest.mark.parametrize("kw,word", _PROBLEMS, ids=[w for _, w in _PROBLEMS])
def test_check_supported_names_each_problem(kw, word):
    from gmlm_amd import deberta
    cfg = _cfg()
    for k, v in kw.items():
        setattr(cfg, k, v)
    with pytest.raises(NotImplementedError) as e:
        deberta.check_supported(_Holder(cfg))
    assert word in str(e.value) and str(e.value).count(";") == 0, str(e.value)


def test_check_supported_names_every_problem_at_once():
    from gmlm_amd import deberta
    cfg = _cfg()
    for kw, _ in _PROBLEMS:
        for k, v in kw.items():
            setattr(cfg, k, v)
    cfg.model_type = "deberta"
    with pytest.raises(NotImplementedError) as e:
        deberta.check_supported(_Holder(cfg))
    for word in ["model_type='deberta'"] + [w for _, w in _PROBLEMS]:
        assert word in str(e.value), (word, str(e.value))


def test_other_encoder_modules_refuse_deberta_and_it_refuses_them():
    from gmlm_amd import bert, deberta, modernbert, mpnet, qwen3
    from transformers import BertConfig, DebertaConfig, ModernBertConfig, MPNetConfig, Qwen3Config
    for mod in (bert, qwen3, modernbert, mpnet):
        with pytest.raises(NotImplementedError, match="model_type='deberta-v2'"):
            mod.check_supported(_Holder(_cfg()))
    with pytest.raises(NotImplementedError, match="model_type='deberta'"):                   # v1 stays refused
        bert.check_supported(_Holder(DebertaConfig(hidden_size=128, num_attention_heads=2)))
    for other, kind in ((BertConfig(hidden_size=128, num_attention_heads=2), "bert"),
                        (MPNetConfig(hidden_size=128, num_attention_heads=2), "mpnet"),
                        (DebertaConfig(hidden_size=128, num_attention_heads=2), "deberta"),
                        (ModernBertConfig(hidden_size=128, num_attention_heads=2, intermediate_size=192, num_hidden_layers=2), "modernbert"),
                        (Qwen3Config(hidden_size=256, num_attention_heads=4, num_key_value_heads=2, head_dim=128, intermediate_size=384,
                                     num_hidden_layers=2, vocab_size=96), "qwen3")):
        with pytest.raises(NotImplementedError, match=f"model_type='{kind}'"):
            deberta.check_supported(_Holder(other))


# ---------------------------------------------------------------------------------------------------------- model wiring
def _tiny_model(**kw):
    import gmlm_amd
    from transformers import DebertaV2Model
    torch.manual_seed(0)
    plm = DebertaV2Model(_cfg(**kw))
    return gmlm_amd.GraphTextLM(12, 16, 3, plm_encoder=plm, plm_tokenizer=None), plm


def test_model_dispatches_a_deberta_encoder():
    """Fails on the commit before this encoder: ``bert.check_supported`` raises NotImplementedError for model_type 'deberta-v2'."""
    from gmlm_amd import bert, deberta
    model, plm = _tiny_model()
    assert model._enc is deberta and model._enc is not bert and model._plm_kind == "deberta-v2"
    assert model._has_packed_pass() and model._packed_head_dim() == 0      # its own packed pass; no bucketed / recorded form
    with pytest.raises(NotImplementedError, match="BERT-geometry encoders only"):
        model.capture_hip_graphs(torch.zeros(4, 12), torch.zeros(2, 4, dtype=torch.long))
    keys = {k[len("plm_encoder."):] for k in model.state_dict() if k.startswith("plm_encoder.")}
    assert keys == set(plm.state_dict())
    assert {"embeddings.word_embeddings.weight", "embeddings.LayerNorm.weight", "encoder.rel_embeddings.weight", "encoder.LayerNorm.bias",
            "encoder.layer.0.attention.self.query_proj.weight", "encoder.layer.2.attention.self.value_proj.bias",
            "encoder.layer.1.attention.output.LayerNorm.weight", "encoder.layer.2.output.dense.weight"} <= keys
    assert not any("token_type" in k or "position_embeddings" in k for k in keys)


def test_prepare_weights_fuses_q_k_v_and_keeps_the_masters():
    from gmlm_amd import deberta
    _, plm = _tiny_model()
    lws = deberta.prepare_weights(plm, torch.float32)
    assert len(lws) == 3
    for lw, layer in zip(lws, plm.encoder.layer):
        sa, so = layer.attention.self, layer.attention.output
        q, k, v = sa.query_proj, sa.key_proj, sa.value_proj
        assert tuple(lw.wqkv.shape) == (384, 128) and torch.equal(lw.wqkv, torch.cat([q.weight, k.weight, v.weight]))
        assert torch.equal(lw.bqkv, torch.cat([q.bias, k.bias, v.bias])) and not lw.wqkv.requires_grad
        assert torch.equal(lw.wo, so.dense.weight) and torch.equal(lw.wi, layer.intermediate.dense.weight)
        assert torch.equal(lw.wo2, layer.output.dense.weight)
        assert lw.m_qkv == (q.weight, k.weight, v.weight, q.bias, k.bias, v.bias) and lw.bo is so.dense.bias
        assert lw.ln1w is so.LayerNorm.weight and lw.ln2b is layer.output.LayerNorm.bias
    with pytest.raises(ValueError):
        deberta.prepare_weights(plm, torch.bfloat16, "bf16x3")         # gemm_precision is passed through and checked


def test_relative_rows_are_the_reachable_slice_of_hf_rel_embeddings():
    from gmlm_amd import deberta
    _, plm = _tiny_model()
    with torch.no_grad():
        plm.encoder.LayerNorm.weight.normal_()
        plm.encoder.LayerNorm.bias.normal_()
    ref = plm.encoder.get_rel_embedding()                                                     # [2k, P]
    for m in (5, 40, 100):
        cols = deberta.bucket_columns(m, 16, 40)
        got = deberta.relative_rows(plm, cols, torch.float32)
        assert tuple(got.shape) == (cols.width, 128) and torch.equal(got, ref[cols.first:cols.first + cols.width])


def test_position_tables_are_the_gathered_hf_terms_and_differentiable():
    """``position_tables`` on the CPU in float64 against the two bmm + gather terms of ``disentangled_attention_bias``."""
    from gmlm_amd import deberta
    g = torch.Generator().manual_seed(3)
    h, d, t, w = 2, 64, 9, 15
    qkv = torch.randn(t, 3 * h * d, generator=g, dtype=torch.float64, requires_grad=True)
    qkr = torch.randn(w, 2 * h * d, generator=g, dtype=torch.float64, requires_grad=True)
    c2p, p2c = deberta.position_tables(qkv, qkr, h)
    q, k = (qkv[:, i * h * d:(i + 1) * h * d].reshape(t, h, d).transpose(0, 1) for i in (0, 1))
    qr, kr = (qkr[:, i * h * d:(i + 1) * h * d].reshape(w, h, d).transpose(0, 1) for i in (0, 1))
    r_c2p, r_p2c = q @ kr.transpose(1, 2), k @ qr.transpose(1, 2)
    assert tuple(c2p.shape) == (h, t, w) and float((c2p - r_c2p).abs().max()) < 1e-12 and float((p2c - r_p2c).abs().max()) < 1e-12
    wc, wp = torch.randn(h, t, w, generator=g, dtype=torch.float64), torch.randn(h, t, w, generator=g, dtype=torch.float64)
    ours = torch.autograd.grad((c2p * wc).sum() + (p2c * wp).sum(), (qkv, qkr))
    ref = torch.autograd.grad((r_c2p * wc).sum() + (r_p2c * wp).sum(), (qkv, qkr))
    for a, b in zip(ours, ref):
        assert float((a - b).abs().max()) < 1e-11
    assert float(ours[0][:, 2 * h * d:].abs().sum()) == 0.0                                   # V takes no part


def test_encoder_refuses_a_sequence_past_the_kernel_table():
    from gmlm_amd import deberta
    _, plm = _tiny_model()
    with pytest.raises(ValueError, match="sequence length 513 exceeds 512"):
        deberta.deberta_encode(plm, torch.zeros(1, 513, dtype=torch.long), torch.tensor([513], dtype=torch.int32), torch.float32)
    z = torch.zeros(600, dtype=torch.long)
    with pytest.raises(ValueError, match="sequence length 600 exceeds 512"):
        deberta.deberta_encode_packed(plm, z, z, torch.tensor([0, 600], dtype=torch.int32), 600, torch.float32)
    with pytest.raises(ValueError):
        deberta.deberta_encode_packed(plm, z[:8], z[:7], torch.tensor([0, 8], dtype=torch.int32), 8, torch.float32)


# --------------------------------------------------------------------------------------------------------- code objects
def test_disent_kernels_are_the_ones_the_gpu_tests_run():
    from test_gpu_deberta_kernels import BF, FP, expected_kernels
    want = set().union(*(expected_kernels(t, dr) for t in (BF, FP) for dr in (False, True)))
    got = _compiled_kernels(lambda name: name.startswith("disent::"))
    assert len(want) == 4 * 5 + 2
    assert got == want, (sorted(got - want), sorted(want - got))


def test_disent_kernels_have_no_private_segment_and_no_packed_fp32():
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
            for m in re.finditer(r"\.name:\s+(_ZN4gmlm6disent\w+)\s+\.private_segment_fixed_size:\s+(\d+)", notes):
                private[m.group(1)] = int(m.group(2))
            dis = subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-d", "--mcpu=gfx950", co], check=True, capture_output=True,
                                 text=True).stdout
            for m in re.finditer(r"^[0-9a-f]+ <(_ZN4gmlm6disent\w+)>:\n(.*?)(?=^[0-9a-f]+ <|\Z)", dis, re.S | re.M):
                bodies[m.group(1)] = m.group(2)
        assert len(private) == 22 and set(private) == set(bodies), (sorted(private), sorted(bodies))
        assert not {n: v for n, v in private.items() if v}, private
        for name, body in bodies.items():
            if "delta" not in name:
                assert "v_mfma" in body, name
            assert not re.search(r"v_pk_\w+_f32", body), name
            assert "scratch_" not in body, name
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
