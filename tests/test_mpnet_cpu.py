"""Host side of the MPNet text encoder (no GPU needed): the seventh header (include/gmlm_hip_relbias.h), its ctypes table
``_lib.SIGNATURES_RELBIAS`` and the exported symbols agree type by type and share no name with the six tables of
``SIGNATURE_TABLES``, which stay as they are; the entry points decide every documented refusal and the nothing-to-do cases
before any launch; ``mpnet.check_supported`` names each problem, and all of them at once; the model layer routes an MPNet
encoder to ``gmlm_amd.mpnet``; the bias table is bit-equal to ``MPNetEncoder.compute_position_bias``, the fold of its gradient
sums as ``index_add`` does, the position rows are those of ``create_position_ids_from_input_ids``; and the ``relb::`` kernels
of the built code objects are the ones tests/test_gpu_mpnet_kernels.py runs, none with a private segment (spill) or packed-fp32
VALU."""
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
HEADER = os.path.join(ROOT, "include", "gmlm_hip_relbias.h")

no_device = pytest.mark.skipif(torch.cuda.device_count() > 0,
                               reason="fabricated addresses: only meaningful (and only safe) without a device")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libgmlm_hip.so not built")
    return _lib.lib()


# ------------------------------------------------------------------------------------------------------------------ ABI
ENTRY_POINTS = ["gmlm_attention_relbias_bwd", "gmlm_attention_relbias_fwd", "gmlm_attention_relbias_workspace_bytes"]


def test_header_ctypes_table_and_exports_agree(lib):
    protos = parse_header(open(HEADER).read())
    assert sorted(protos) == ENTRY_POINTS
    assert not signature_mismatches(protos, _lib.SIGNATURES_RELBIAS)
    for name in protos:
        assert hasattr(lib, name), f"{name} declared in include/gmlm_hip_relbias.h but not exported"
        assert getattr(lib, name).argtypes == _lib.SIGNATURES_RELBIAS[name][1]                    # lib() bound the new table
    assert len(_lib.SIGNATURE_TABLES) == 6 and _lib.SIGNATURE_TABLES[-1] is _lib.SIGNATURES_MODERNBERT
    assert _lib.SIGNATURES_RELBIAS in _lib.SIGNATURE_TABLES_LATER
    assert not any(t is _lib.SIGNATURES_RELBIAS for t in _lib.SIGNATURE_TABLES)
    others = set().union(*(set(t) for t in _lib.SIGNATURE_TABLES))
    assert not set(_lib.SIGNATURES_RELBIAS) & others
    assert lib.gmlm_version() == 1


def test_table_bound_is_stated_once():
    from gmlm_amd import ops
    m = re.search(r"#define GMLM_RELBIAS_MAX_LEN (\d+)", open(HEADER).read())
    assert m and int(m.group(1)) == ops.RELBIAS_MAX_LEN == 512


_BASE = dict(q=A, k=A, v=A, kv_len=None, b=1, h=12, lq=64, lk=64, d=64, q_stride=2304, k_stride=2304, v_stride=2304, scale=0.125,
             dropout_p=0.0, seed=0, seed_dev=None, rel_bias=A, rel_m=64, out=A, out_lo=None, lse=A, dtype=BF16, cu_seqlens=None,
             max_len=0, stream=None, dout=A, dq=A, dk=A, dv=A, d_rel_bias=A, dq_stride=2304, dk_stride=2304, dv_stride=2304,
             workspace=A, workspace_bytes=1 << 40)
_FWD = ("q k v kv_len b h lq lk d q_stride k_stride v_stride scale dropout_p seed seed_dev rel_bias rel_m out out_lo lse dtype "
        "cu_seqlens max_len stream").split()
_BWD = ("q k v out out_lo dout lse kv_len b h lq lk d q_stride k_stride v_stride scale dropout_p seed seed_dev rel_bias rel_m dq dk dv "
        "d_rel_bias dq_stride dk_stride dv_stride dtype cu_seqlens max_len workspace workspace_bytes stream").split()


def _call(lib, which, **mut):
    a = dict(_BASE, **mut)
    fn, names = (lib.gmlm_attention_relbias_fwd, _FWD) if which == "fwd" else (lib.gmlm_attention_relbias_bwd, _BWD)
    return fn(*[a[n] for n in names]), lib.gmlm_last_error()


def test_argument_lists_follow_the_header():
    protos = parse_header(open(HEADER).read())
    assert [n for _, n in protos["gmlm_attention_relbias_fwd"][1]] == _FWD
    assert [n for _, n in protos["gmlm_attention_relbias_bwd"][1]] == _BWD
    assert [n for _, n in protos["gmlm_attention_relbias_workspace_bytes"][1]] == "b h lq max_len rel_m".split()


_REFUSALS = [
    (dict(d=32), b"head dim"), (dict(d=96), b"head dim"), (dict(d=128), b"head dim"),
    (dict(dtype=2), b"dtype"),
    (dict(lk=65), b"lq == lk"), (dict(lq=63), b"lq == lk"),
    (dict(rel_m=63), b"rel_m"), (dict(rel_m=0), b"rel_m"), (dict(rel_m=513), b"rel_m"),             # below the sequence, above 512
    (dict(lq=513, lk=513, rel_m=513), b"rel_m"), (dict(lq=600, lk=600, rel_m=512), b"rel_m"),
    (dict(cu_seqlens=A, lq=900, lk=900, max_len=65, rel_m=64), b"rel_m"),                           # packed: the longest sequence counts
    (dict(rel_bias=None), b"rel_bias"), (dict(rel_bias=A + 4), b"rel_bias"),
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
    (dict(b=(1 << 31) // 12 + 1, lq=1, lk=1), b"too many work items"),
]


@no_device
@pytest.mark.parametrize("which", ["fwd", "bwd"])
@pytest.mark.parametrize("mut,msg", _REFUSALS, ids=[",".join(f"{k}={v}" for k, v in m.items()) for m, _ in _REFUSALS])
def test_relbias_attention_refusals_are_decided_on_the_host(lib, which, mut, msg):
    rc, err = _call(lib, which, **mut)
    assert rc == EINVAL and msg in err, (mut, rc, err)


@no_device
def test_backward_refuses_a_null_or_misaligned_gradient_table(lib):
    for bad in (None, A + 4):
        rc, err = _call(lib, "bwd", d_rel_bias=bad)
        assert rc == EINVAL and b"d_rel_bias" in err


@no_device
def test_valid_relbias_calls_reach_the_launch(lib):
    for which in ("fwd", "bwd"):
        for mut in (dict(), dict(dtype=F32), dict(cu_seqlens=A, max_len=64), dict(cu_seqlens=A, lq=900, lk=900, max_len=64), dict(kv_len=A),
                    dict(out_lo=A), dict(dropout_p=0.1, seed=7, seed_dev=A), dict(rel_m=512), dict(lq=512, lk=512, rel_m=512),
                    dict(lq=1, lk=1, rel_m=1), dict(b=(1 << 31) // 12 - 1, lq=1, lk=1)):
            rc, err = _call(lib, which, **mut)
            assert rc == ELAUNCH, (which, mut, rc, err)


@no_device
def test_relbias_backward_workspace_boundary(lib):
    # delta [b, h, l] (a multiple of 16 bytes here) + one partial row [2M - 1] per (128-query tile, sequence, head)
    need = lib.gmlm_attention_relbias_workspace_bytes(2, 12, 300, 0, 320)
    assert need == 2 * 12 * 300 * 4 + 3 * 2 * 12 * 639 * 4 and lib.gmlm_attention_relbias_workspace_bytes(0, 12, 0, 0, 1) > 0
    shape = dict(b=2, lq=300, lk=300, rel_m=320)
    assert _call(lib, "bwd", workspace_bytes=need, **shape)[0] == ELAUNCH
    rc, err = _call(lib, "bwd", workspace_bytes=need - 1, **shape)
    assert rc == EWORKSPACE and b"workspace" in err
    assert _call(lib, "bwd", workspace=None, **shape)[0] == EWORKSPACE
    packed = dict(b=7, lq=300, lk=300, cu_seqlens=A, max_len=100, rel_m=100)     # delta [h, total_rows]; one tile per sequence
    need = lib.gmlm_attention_relbias_workspace_bytes(7, 12, 300, 100, 100)
    assert need == 12 * 300 * 4 + 7 * 12 * 199 * 4
    assert _call(lib, "bwd", workspace_bytes=need, **packed)[0] == ELAUNCH
    assert _call(lib, "bwd", workspace_bytes=need - 1, **packed)[0] == EWORKSPACE


@no_device
def test_nothing_to_do_needs_no_pointer_but_sizes_are_still_checked(lib):
    nothing = dict(q=None, k=None, v=None, out=None, lse=None, dout=None, dq=None, dk=None, dv=None, rel_bias=None, d_rel_bias=None,
                   workspace=None, workspace_bytes=0)
    for empty in (dict(b=0), dict(lq=0, lk=0), dict(lq=0, lk=0, cu_seqlens=A, max_len=1)):
        for which in ("fwd", "bwd"):
            assert _call(lib, which, **nothing, **empty)[0] == OK, (which, empty)
            rc, err = _call(lib, which, **nothing, **empty, d=128)
            assert rc == EINVAL and b"head dim" in err
            rc, err = _call(lib, which, **nothing, **empty, rel_m=600)
            assert rc == EINVAL and b"rel_m" in err


def test_new_op_fails_loudly_without_a_gpu(lib):
    """CPU tensors raise the library's error: no eager fallback behind the new operator."""
    from gmlm_amd import ops
    with pytest.raises(_lib.GmlmHipError):
        ops.attention_relbias_qkv(torch.zeros(1, 4, 384), torch.zeros(2, 7), None, 2, 0.125)
    with pytest.raises(_lib.GmlmHipError):
        ops.attention_relbias_qkv_varlen(torch.zeros(4, 384), torch.zeros(2, 7), torch.tensor([0, 4], dtype=torch.int32), 4, 2, 0.125)


# --------------------------------------------------------------------------------------------------------- check_supported
def _cfg(**kw):
    from transformers import MPNetConfig
    base = dict(vocab_size=96, hidden_size=128, intermediate_size=192, num_hidden_layers=3, num_attention_heads=2,
                max_position_embeddings=514)
    base.update(kw)
    return MPNetConfig(**base)


class _Holder:
    def __init__(self, config):
        self.config = config


def test_check_supported_accepts_an_mpnet_config():
    from gmlm_amd import mpnet
    cfg = _cfg()
    mpnet.check_supported(_Holder(cfg))
    assert cfg.model_type == "mpnet" and cfg.relative_attention_num_buckets == 32 and cfg.hidden_act == "gelu"
    mpnet.check_supported(_Holder(_cfg(relative_attention_num_buckets=48)))       # more rows than HF reads: fine
    assert mpnet.max_sequence(cfg) == 512 and mpnet.max_sequence(_cfg(max_position_embeddings=130)) == 128
    assert mpnet.max_sequence(_cfg(max_position_embeddings=2050)) == 512


_PROBLEMS = [
    (dict(num_attention_heads=4), "head_dim=32"),
    (dict(hidden_act="relu"), "hidden_act='relu'"),
    (dict(relative_attention_num_buckets=16), "relative_attention_num_buckets=16"),
]


@pytest.mark.parametrize("kw,word", _PROBLEMS, ids=[w for _, w in _PROBLEMS])
def test_check_supported_names_each_problem(kw, word):
    from gmlm_amd import mpnet
    cfg = _cfg()
    for k, v in kw.items():
        setattr(cfg, k, v)
    with pytest.raises(NotImplementedError) as e:
        mpnet.check_supported(_Holder(cfg))
    assert word in str(e.value), str(e.value)


def test_check_supported_names_every_problem_at_once():
    from gmlm_amd import mpnet
    cfg = _cfg()
    for kw, _ in _PROBLEMS:
        for k, v in kw.items():
            setattr(cfg, k, v)
    cfg.model_type = "bert"
    with pytest.raises(NotImplementedError) as e:
        mpnet.check_supported(_Holder(cfg))
    for word in ["model_type='bert'"] + [w for _, w in _PROBLEMS]:
        assert word in str(e.value), (word, str(e.value))


def test_other_encoder_modules_refuse_mpnet_and_it_refuses_them():
    from gmlm_amd import bert, modernbert, mpnet, qwen3
    from transformers import BertConfig, ModernBertConfig, Qwen3Config
    for mod in (bert, qwen3, modernbert):
        with pytest.raises(NotImplementedError, match="model_type='mpnet'"):
            mod.check_supported(_Holder(_cfg()))
    for other, kind in ((BertConfig(hidden_size=128, num_attention_heads=2), "bert"),
                        (ModernBertConfig(hidden_size=128, num_attention_heads=2, intermediate_size=192, num_hidden_layers=2), "modernbert"),
                        (Qwen3Config(hidden_size=256, num_attention_heads=4, num_key_value_heads=2, head_dim=128, intermediate_size=384,
                                     num_hidden_layers=2, vocab_size=96), "qwen3")):
        with pytest.raises(NotImplementedError, match=f"model_type='{kind}'"):
            mpnet.check_supported(_Holder(other))


# ---------------------------------------------------------------------------------------------------------- model wiring
def _tiny_model(**kw):
    import gmlm_amd
    from transformers import MPNetModel
    torch.manual_seed(0)
    plm = MPNetModel(_cfg(**kw))
    return gmlm_amd.GraphTextLM(12, 16, 3, plm_encoder=plm, plm_tokenizer=None), plm


def test_model_dispatches_an_mpnet_encoder():
    from gmlm_amd import bert, mpnet
    model, plm = _tiny_model()
    assert model._enc is mpnet and model._enc is not bert and model._plm_kind == "mpnet"
    assert model._has_packed_pass() and model._packed_head_dim() == 0      # its own packed pass; no bucketed / recorded form
    with pytest.raises(NotImplementedError, match="BERT-geometry encoders only"):
        model.capture_hip_graphs(torch.zeros(4, 12), torch.zeros(2, 4, dtype=torch.long))
    keys = {k[len("plm_encoder."):] for k in model.state_dict() if k.startswith("plm_encoder.")}
    assert keys == set(plm.state_dict())
    assert {"embeddings.word_embeddings.weight", "embeddings.position_embeddings.weight", "encoder.relative_attention_bias.weight",
            "encoder.layer.0.attention.attn.q.weight", "encoder.layer.2.attention.attn.o.bias", "encoder.layer.1.attention.LayerNorm.weight",
            "encoder.layer.2.output.dense.weight"} <= keys and not any("token_type" in k for k in keys)


def test_prepare_weights_fuses_q_k_v_and_keeps_the_masters():
    from gmlm_amd import mpnet
    _, plm = _tiny_model()
    lws = mpnet.prepare_weights(plm, torch.float32)
    assert len(lws) == 3
    for lw, layer in zip(lws, plm.encoder.layer):
        sa = layer.attention.attn
        assert tuple(lw.wqkv.shape) == (384, 128) and torch.equal(lw.wqkv, torch.cat([sa.q.weight, sa.k.weight, sa.v.weight]))
        assert torch.equal(lw.bqkv, torch.cat([sa.q.bias, sa.k.bias, sa.v.bias])) and not lw.wqkv.requires_grad
        assert torch.equal(lw.wo, sa.o.weight) and torch.equal(lw.wi, layer.intermediate.dense.weight)
        assert torch.equal(lw.wo2, layer.output.dense.weight)
        assert lw.m_qkv == (sa.q.weight, sa.k.weight, sa.v.weight, sa.q.bias, sa.k.bias, sa.v.bias) and lw.bo is sa.o.bias
        assert lw.ln1w is layer.attention.LayerNorm.weight and lw.ln2b is layer.output.LayerNorm.bias
    with pytest.raises(ValueError):
        mpnet.prepare_weights(plm, torch.bfloat16, "bf16x3")           # gemm_precision is passed through and checked


# ---------------------------------------------------------------------------------------------------------- host functions
@pytest.mark.parametrize("l", [1, 8, 91, 92, 512])
def test_bias_table_is_bit_equal_to_compute_position_bias(l):
    from gmlm_amd import mpnet
    _, plm = _tiny_model()
    with torch.no_grad():
        plm.encoder.relative_attention_bias.weight.normal_()
    table = mpnet.bias_table(plm.encoder.relative_attention_bias.weight, l)
    assert table.dtype == torch.float32 and tuple(table.shape) == (2, 2 * l - 1) and table.is_contiguous()
    ref = plm.encoder.compute_position_bias(torch.zeros(1, l, 8))[0]          # [h, l, l]: query i, key j
    i, j = torch.arange(l)[:, None], torch.arange(l)[None, :]
    assert torch.equal(table[:, (l - 1) + (j - i)], ref)
    # a longer table read by a shorter sequence gives the same biases
    big = mpnet.bias_table(plm.encoder.relative_attention_bias.weight, 512)
    assert torch.equal(big[:, 511 + (j - i)], ref)


def test_buckets_are_contiguous_ranges_and_saturate_at_91():
    from gmlm_amd import mpnet
    bucket, gather = mpnet.bucket_index(512)
    assert bucket.numel() == 1023 and int(bucket.unique().numel()) == 31 and int((bucket[1:] != bucket[:-1]).sum()) == 30
    rel = torch.arange(-511, 512)
    assert bool((bucket[rel >= 91] == bucket[-1]).all()) and bool((bucket[rel <= -91] == bucket[0]).all())
    assert int(bucket[rel == 90]) != int(bucket[-1]) and int(bucket[rel == -90]) != int(bucket[0])
    assert tuple(gather.shape) == (32, 421)                                   # the saturated bucket: rel 91 .. 511


@pytest.mark.parametrize("m", [1, 8, 92, 512])
def test_bucket_fold_sums_as_index_add_does(m):
    from gmlm_amd import mpnet
    g = torch.Generator().manual_seed(m)
    d_rel = torch.randn(3, 2 * m - 1, generator=g, dtype=torch.float64)
    bucket, gather = mpnet.bucket_index(m)
    ref = torch.zeros(32, 3, dtype=torch.float64).index_add_(0, bucket, d_rel.t().contiguous())
    got = mpnet.fold_bias_grad(d_rel, gather)
    assert tuple(got.shape) == (32, 3) and float((got - ref).abs().max()) <= 1e-12 * max(1.0, float(ref.abs().max()))
    got32 = mpnet.fold_bias_grad(d_rel.float(), gather)
    assert got32.dtype == torch.float32 and float((got32.double() - ref).abs().max()) <= 2.0 ** -20 * float(d_rel.abs().sum(1).max())
    # through autograd: the table's backward is the fold, onto a parameter with more rows than HF reads as well
    for rows in (32, 40):
        w = torch.randn(rows, 3, generator=g).requires_grad_(True)
        mpnet.bias_table(w, m).backward(d_rel.float())
        assert tuple(w.grad.shape) == (rows, 3) and torch.equal(w.grad[:32], got32) and float(w.grad[32:].abs().sum()) == 0.0


def test_position_rows_are_those_of_right_padded_input_ids():
    from gmlm_amd import mpnet
    from transformers.models.mpnet.modeling_mpnet import create_position_ids_from_input_ids
    pad = 1
    ids = torch.full((3, 9), pad, dtype=torch.long)
    for b, n in enumerate((9, 4, 1)):
        ids[b, :n] = torch.randint(2, 96, (n,))
    ref = create_position_ids_from_input_ids(ids, pad)
    ours = mpnet.position_ids(9, pad)
    for b, n in enumerate((9, 4, 1)):
        assert torch.equal(ref[b, :n], ours[:n]) and bool((ref[b, n:] == pad).all())
    assert int(ours[0]) == 2 and int(ours[-1]) == 10


def test_encoder_refuses_a_sequence_past_the_position_table_or_the_kernel_table():
    from gmlm_amd import mpnet
    _, plm = _tiny_model(max_position_embeddings=18)
    with pytest.raises(ValueError, match="max_position_embeddings"):
        mpnet.mpnet_encode(plm, torch.zeros(1, 17, dtype=torch.long), torch.tensor([17], dtype=torch.int32), torch.float32)
    z = torch.zeros(17, dtype=torch.long)
    with pytest.raises(ValueError, match="max_position_embeddings"):
        mpnet.mpnet_encode_packed(plm, z, z, torch.tensor([0, 17], dtype=torch.int32), 17, torch.float32)
    _, plm = _tiny_model(max_position_embeddings=1026)
    with pytest.raises(ValueError, match="max_position_embeddings"):
        mpnet.mpnet_encode(plm, torch.zeros(1, 513, dtype=torch.long), torch.tensor([513], dtype=torch.int32), torch.float32)


# --------------------------------------------------------------------------------------------------------- code objects
def test_relb_kernels_are_the_ones_the_gpu_tests_run():
    from test_gpu_mpnet_kernels import ALL_KERNELS
    got = _compiled_kernels(lambda name: name.startswith("relb::"))
    assert len(ALL_KERNELS) == 4 * 4 + 2 + 1
    assert got == ALL_KERNELS, (sorted(got - ALL_KERNELS), sorted(ALL_KERNELS - got))


def test_relb_kernels_have_no_private_segment_and_no_packed_fp32():
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
            for m in re.finditer(r"\.name:\s+(_ZN4gmlm4relb\w+)\s+\.private_segment_fixed_size:\s+(\d+)", notes):
                private[m.group(1)] = int(m.group(2))
            dis = subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-d", "--mcpu=gfx950", co], check=True, capture_output=True,
                                 text=True).stdout
            for m in re.finditer(r"^[0-9a-f]+ <(_ZN4gmlm4relb\w+)>:\n(.*?)(?=^[0-9a-f]+ <|\Z)", dis, re.S | re.M):
                bodies[m.group(1)] = m.group(2)
        assert len(private) == 19 and set(private) == set(bodies), (sorted(private), sorted(bodies))
        assert not {n: v for n, v in private.items() if v}, private
        for name, body in bodies.items():
            if "delta" not in name and "dbias_sum" not in name:
                assert "v_mfma" in body, name
            assert not re.search(r"v_pk_\w+_f32", body), name
            assert "scratch_" not in body, name
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
