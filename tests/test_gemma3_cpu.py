"""Host side of the Gemma3 text encoder (no GPU needed): the thirteenth header (include/gmlm_hip_gqa_wide.h), its ctypes table
``_lib.SIGNATURES_GQA_WIDE`` and the exported symbols agree type by type, the table sitting strictly inside
``SIGNATURE_TABLES_LATER`` and sharing no name with any other; the attention argument lists are those of their
``gmlm_attention_bidir_gqa_*`` namesakes plus ``causal``; the entry points decide every documented refusal and the nothing-to-do
cases before any launch; ``gemma3.check_supported`` accepts the released geometries and names each problem, and all of them at
once; ``gemma3.rope_tables`` holds the floats of HF's Gemma3RotaryEmbedding for both layer types; ``check_window`` at the window
and one past it for both masks; the model layer routes ``gemma3_text`` to the module; the kernels' tanh-GeGLU and sandwich-norm
expressions in fp32 hold HALF the budgets of tests/test_gpu_gemma_rowops.py on that file's inputs; the compiled kernels are
the ones the static profile lists, none with scratch."""
import json
import os
import re

import pytest
import torch

from conftest import ROOT
from gmlm_amd import _lib
from test_abi_contract_cpu import parse_header, signature_mismatches
from test_attention_matrix_cpu import _compiled_kernels
from test_gpu_decoder_ops import U
from test_gpu_gemma_rowops import EPS, GLU_SHAPES, KA, KB, SAND_ROWS, SAND_WIDTHS, geglu_inputs, geglu_reference, sandwich_inputs, \
    sandwich_reference

OK, EINVAL, EWORKSPACE, ELAUNCH = 0, -1, -2, -3
F32, BF16 = 0, 1
A = 0x10000000        # fabricated, non-null, 16-byte aligned: every call below ends before or at the launch
HEADER = os.path.join(ROOT, "include", "gmlm_hip_gqa_wide.h")
STEM = "gmlm_attention_gqa_d256"
TABLE = _lib.SIGNATURES_GQA_WIDE

no_device = pytest.mark.skipif(torch.cuda.device_count() > 0,
                               reason="fabricated addresses: only meaningful (and only safe) without a device")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libgmlm_hip.so not built")
    return _lib.lib()


class _Holder:
    def __init__(self, config):
        self.config = config


# ------------------------------------------------------------------------------------------------------------------ ABI
ENTRY_POINTS = sorted([STEM + t for t in ("_fwd", "_bwd", "_bwd_workspace_bytes", "_varlen_fwd", "_varlen_bwd", "_varlen_bwd_workspace_bytes")]
                      + ["gmlm_sandwich_rmsnorm_fwd", "gmlm_sandwich_rmsnorm_bwd", "gmlm_sandwich_rmsnorm_bwd_workspace_bytes",
                         "gmlm_qknorm_rope_d256_fwd", "gmlm_qknorm_rope_d256_pos_fwd", "gmlm_qknorm_rope_d256_bwd",
                         "gmlm_qknorm_rope_d256_pos_bwd", "gmlm_qknorm_rope_d256_bwd_workspace_bytes", "gmlm_geglu_tanh_fwd",
                         "gmlm_geglu_tanh_bwd"])


def test_header_ctypes_table_and_exports_agree(lib):
    protos = parse_header(open(HEADER).read())
    assert sorted(protos) == ENTRY_POINTS and len(protos) == 16
    assert not signature_mismatches(protos, TABLE)
    for name in protos:
        assert hasattr(lib, name), f"{name} declared in include/gmlm_hip_gqa_wide.h but not exported"
        assert getattr(lib, name).argtypes == TABLE[name][1]                                  # lib() bound the new table
    later = _lib.SIGNATURE_TABLES_LATER
    assert any(t is TABLE for t in later[1:-1]) and later[0] is not TABLE and later[-1] is not TABLE      # strictly inside
    assert not any(t is TABLE for t in _lib.SIGNATURE_TABLES)
    others = set().union(*(set(t) for t in _lib.SIGNATURE_TABLES + later if t is not TABLE))
    assert not set(TABLE) & others
    assert lib.gmlm_version() == 1
    text = open(HEADER).read()
    assert '#include "gmlm_hip.h"' in text and 'extern "C"' in text


def _names(protos, name):
    return [n for _, n in protos[name][1]]


def test_argument_lists_are_the_namesakes_plus_one_argument():
    bidir = parse_header(open(os.path.join(ROOT, "include", "gmlm_hip_bidir.h")).read())
    main = parse_header(open(os.path.join(ROOT, "include", "gmlm_hip.h")).read())
    protos = parse_header(open(HEADER).read())
    for tail in ("_fwd", "_bwd", "_varlen_fwd", "_varlen_bwd"):
        old, new = bidir["gmlm_attention_bidir_gqa" + tail], protos[STEM + tail]
        i = _names(bidir, "gmlm_attention_bidir_gqa" + tail).index("dropout_p") + 1
        assert new[0] == old[0] and new[1] == old[1][:i] + [("int", "causal")] + old[1][i:], tail
    assert protos[STEM + "_bwd_workspace_bytes"] == bidir["gmlm_attention_bidir_gqa_workspace_bytes"]
    assert protos[STEM + "_varlen_bwd_workspace_bytes"] == bidir["gmlm_attention_bidir_gqa_varlen_workspace_bytes"]
    for tail in ("_fwd", "_pos_fwd", "_bwd", "_pos_bwd"):
        old, new = main["gmlm_qknorm_rope" + tail], protos["gmlm_qknorm_rope_d256" + tail]
        i = _names(main, "gmlm_qknorm_rope" + tail).index("d") + 1
        assert new[0] == old[0] and new[1] == old[1][:i] + [("float", "w_offset")] + old[1][i:], tail
    assert protos["gmlm_qknorm_rope_d256_bwd_workspace_bytes"] == main["gmlm_qknorm_rope_bwd_workspace_bytes"]
    for tail in ("_fwd", "_bwd"):
        assert protos["gmlm_geglu_tanh" + tail] == main["gmlm_swiglu" + tail]


def test_the_makefile_names_the_new_sources_and_header():
    mk = open(os.path.join(ROOT, "gmlm_amd", "csrc", "Makefile")).read()
    srcs = re.search(r"^SRCS\s*=(.*)$", mk, re.M).group(1).split()
    for src in ("attn_gqa_wide.hip", "gemma_kernels.hip"):
        assert src in srcs and os.path.exists(os.path.join(ROOT, "gmlm_amd", "csrc", src))
    assert "../../include/gmlm_hip_gqa_wide.h" in re.search(r"^\$\(BUILD\)/%\.o:(.*)$", mk, re.M).group(1).split()


# ------------------------------------------------------------------------------------------------- entry-point refusals
W = 1280 + 8        # (3 + 2) heads of 256 and 8 more: the fused rows are wider than [q | k | v]
_BASE = dict(q=A, k=A, v=A, kv_len=None, b=2, hq=3, hkv=1, lq=64, lk=64, d=256, q_stride=W, k_stride=W, v_stride=W, scale=0.0625,
             dropout_p=0.0, causal=1, out=A, out_lo=None, lse=A, dtype=BF16, stream=None, dout=A, dq=A, dk=A, dv=A, dq_stride=W,
             dk_stride=W, dv_stride=W, workspace=A, workspace_bytes=1 << 40, cu_seqlens=A, num_seqs=2, max_len=64, total_rows=100)


def _lists():
    protos = parse_header(open(HEADER).read())
    return {w: _names(protos, f"{STEM}_{w}") for w in ("fwd", "bwd", "varlen_fwd", "varlen_bwd")}


_LISTS = _lists()


def _call(lib, which, **mut):
    a = dict(_BASE, **mut)
    return getattr(lib, f"{STEM}_{which}")(*[a[n] for n in _LISTS[which]]), lib.gmlm_last_error()


def _ids(cases):
    return ["-".join(f"{k}={v}" for k, v in m.items()) for m, _ in cases]


_REFUSALS = [
    (dict(d=128), b"head dim"), (dict(d=64), b"head dim"), (dict(d=512), b"head dim"),
    (dict(dtype=2), b"dtype"),
    (dict(hq=3, hkv=2), b"multiple of"), (dict(hq=4, hkv=3), b"multiple of"),
    (dict(dropout_p=0.1), b"dropout"),
    (dict(scale=0.0), b"scale"), (dict(scale=-1.0), b"scale"),
    (dict(hq=0), b"bad sizes"), (dict(hkv=-1), b"bad sizes"),
    (dict(q_stride=760), b"stride"),                                    # below hq * 256
    (dict(k_stride=248), b"stride"),                                    # below hkv * 256
    (dict(q_stride=W + 4), b"stride"),                                  # bf16: not a multiple of 8 elements
    (dict(dtype=F32, v_stride=W + 2), b"stride"),                       # fp32: not a multiple of 4 elements
    (dict(v_stride=1 << 24), b"stride"),
    (dict(q=A + 8), b"aligned"), (dict(k=None), b"null"), (dict(v=None), b"null"), (dict(out=None), b"out"), (dict(out=A + 4), b"out"),
    (dict(out_lo=A, dtype=F32), b"out_lo"), (dict(out_lo=A + 8), b"out_lo"),
]
_PADDED_ONLY = [(dict(lk=65), b"lq == lk"), (dict(lq=63), b"lq == lk"), (dict(b=-1), b"bad sizes"),
                (dict(b=(1 << 31) // 3 + 1, lq=1, lk=1), b"too many work items")]
_PACKED_ONLY = [(dict(cu_seqlens=None), b"cu_seqlens"), (dict(max_len=0), b"max_len"), (dict(total_rows=-1), b"packed rows"),
                (dict(total_rows=1 << 30), b"packed rows"), (dict(num_seqs=(1 << 31) // 3 + 1, max_len=1), b"too many work items")]


@no_device
@pytest.mark.parametrize("which", ["fwd", "bwd", "varlen_fwd", "varlen_bwd"])
@pytest.mark.parametrize("mut,msg", _REFUSALS, ids=_ids(_REFUSALS))
def test_attention_refusals_are_decided_on_the_host(lib, which, mut, msg):
    if "out" in mut and "out_lo" not in mut and which.endswith("bwd"):
        msg = b"out/dout/lse"                                           # the backward reads out
    rc, err = _call(lib, which, **mut)
    assert rc == EINVAL and msg in err, (mut, rc, err)


@no_device
def test_layout_refusals_and_valid_calls(lib):
    for which in ("fwd", "bwd"):
        for mut, msg in _PADDED_ONLY:
            rc, err = _call(lib, which, **mut)
            assert rc == EINVAL and msg in err, (which, mut, rc, err)
    for which in ("varlen_fwd", "varlen_bwd"):
        for mut, msg in _PACKED_ONLY:
            rc, err = _call(lib, which, **mut)
            assert rc == EINVAL and msg in err, (which, mut, rc, err)
    for which in _LISTS:                                                 # valid: both masks, both dtypes, the three groupings
        for mut in (dict(), dict(causal=0), dict(dtype=F32), dict(out_lo=A), dict(hq=4, hkv=1), dict(hq=4, hkv=2, q_stride=2048, k_stride=2048,
                    v_stride=2048, dq_stride=2048, dk_stride=2048, dv_stride=2048), dict(hq=2, hkv=2), dict(lq=1, lk=1, max_len=1),
                    dict(q_stride=768, k_stride=256, v_stride=256)):
            rc, err = _call(lib, which, **mut)
            assert rc == ELAUNCH, (which, mut, rc, err)
    assert _call(lib, "fwd", b=(1 << 31) // 3 - 1, lq=1, lk=1)[0] == ELAUNCH              # just below the work-item bound
    for which in ("bwd", "varlen_bwd"):
        for mut, msg in ((dict(dq=None), b"dq"), (dict(dk=A + 4), b"dk"), (dict(dv_stride=248), b"dv"), (dict(dout=None), b"out/dout/lse")):
            rc, err = _call(lib, which, **mut)
            assert rc == EINVAL and msg in err, (which, mut, rc, err)
    need = lib.gmlm_attention_gqa_d256_bwd_workspace_bytes(2, 3, 300)
    assert need == 2 * 3 * 300 * 4 and lib.gmlm_attention_gqa_d256_bwd_workspace_bytes(0, 3, 0) > 0
    assert _call(lib, "bwd", lq=300, lk=300, workspace_bytes=need)[0] == ELAUNCH
    assert _call(lib, "bwd", lq=300, lk=300, workspace_bytes=need - 1)[0] == EWORKSPACE
    need = lib.gmlm_attention_gqa_d256_varlen_bwd_workspace_bytes(100, 3)
    assert need == 3 * 100 * 4
    assert _call(lib, "varlen_bwd", workspace_bytes=need)[0] == ELAUNCH and _call(lib, "varlen_bwd", workspace=None)[0] == EWORKSPACE


@no_device
def test_nothing_to_do_needs_no_pointer_but_sizes_are_still_checked(lib):
    nothing = dict(q=None, k=None, v=None, out=None, lse=None, dout=None, dq=None, dk=None, dv=None, workspace=None, workspace_bytes=0)
    for which, empties in (("fwd", (dict(b=0), dict(lq=0, lk=0))), ("bwd", (dict(b=0), dict(lq=0, lk=0))),
                           ("varlen_fwd", (dict(num_seqs=0), dict(total_rows=0))), ("varlen_bwd", (dict(num_seqs=0), dict(total_rows=0)))):
        for empty in empties:
            assert _call(lib, which, **nothing, **empty)[0] == OK, (which, empty)
            for mut, msg in ((dict(d=128), b"head dim"), (dict(dropout_p=0.5), b"dropout"), (dict(hq=3, hkv=2), b"multiple of"), (dict(dtype=5), b"dtype")):
                rc, err = _call(lib, which, **nothing, **empty, **mut)
                assert rc == EINVAL and msg in err, (which, empty, mut, rc, err)


@no_device
def test_row_kernel_entry_points_decide_on_the_host(lib):
    sf, sb = lib.gmlm_sandwich_rmsnorm_fwd, lib.gmlm_sandwich_rmsnorm_bwd
    assert sf(A, A, A, A, 4, 768, 1.0, 1e-6, A, A, A, A, BF16, None) == ELAUNCH
    assert sf(None, A, A, A, 4, 768, 1.0, 1e-6, A, A, A, A, F32, None) == ELAUNCH              # s is optional
    assert sf(None, None, None, None, 0, 768, 1.0, 1e-6, None, None, None, None, BF16, None) == OK
    for args, msg in (((A, A, A, A, 4, 4104, 1.0, 1e-6, A, A, A, A, BF16, None), b"at most 4096"),
                      ((A, A, A, A, 4, 772, 1.0, 1e-6, A, A, A, A, BF16, None), b"multiple of 8"),
                      ((A, A, A, A, 4, 768, 1.0, 1e-6, A, A, A, A, 3, None), b"dtype"),
                      ((A, None, A, A, 4, 768, 1.0, 1e-6, A, A, A, A, BF16, None), b"null"),
                      ((A + 4, A, A, A, 4, 768, 1.0, 1e-6, A, A, A, A, BF16, None), b"aligned")):
        assert sf(*args) == EINVAL and msg in lib.gmlm_last_error(), args
    f = 768
    need = lib.gmlm_sandwich_rmsnorm_bwd_workspace_bytes(100, f)
    assert need >= 100 * 4 + 2 * f * 4 and need % 16 == 0
    base = dict(dy=A, ds_in=A, b=A, s_out=A, w_post=A, w_pre=A, rstd_b=A, rstd_s=A, rows=100, f=f, off=1.0, ds=A, db=A, dw_post=A,
                dw_pre=A + 4 * f, dtype=BF16, ws=A, ws_bytes=need, stream=None)
    bwd = lambda **m: sb(*dict(base, **m).values())                     # the header's argument order
    assert bwd() == ELAUNCH and bwd(ds_in=None, ds=None) == ELAUNCH
    assert bwd(ws_bytes=need - 1) == EWORKSPACE and bwd(ws=None) == EWORKSPACE
    assert bwd(dw_pre=A) == EINVAL and b"one fp32 [2, f] buffer" in lib.gmlm_last_error()
    assert bwd(db=None) == EINVAL
    rf = lib.gmlm_qknorm_rope_d256_fwd
    ok = (A, W, A, A, A, 512, 128, 64, 3, 1, 256, 1.0, 1e-6, A, 1024, A, BF16, None)
    assert rf(*ok) == ELAUNCH
    for i, v, msg in ((10, 128, b"head dim"), (1, 1272, b"stride"), (14, 1016, b"stride"), (7, 600, b"exceeds"), (2, None, b"weight")):
        args = list(ok)
        args[i] = v
        assert rf(*args) == EINVAL and msg in lib.gmlm_last_error(), (i, v, lib.gmlm_last_error())
    assert rf(None, W, None, None, None, 512, 0, 64, 3, 1, 256, 1.0, 1e-6, None, 1024, None, BF16, None) == OK
    assert lib.gmlm_qknorm_rope_d256_bwd_workspace_bytes(128, 3, 1, BF16) == min(1024, -(-128 * 4 // 8)) * 512 * 4
    rb = lib.gmlm_qknorm_rope_d256_pos_bwd
    okb = (A, W, A, W, A, A, A, 512, A, 128, A, 3, 1, 256, 1.0, A, A + 1024, BF16, A, 1 << 30, None)
    assert rb(*okb) == ELAUNCH
    bad = list(okb)
    bad[16] = A + 512
    assert rb(*bad) == EINVAL and b"[2, 256]" in lib.gmlm_last_error()
    bad = list(okb)
    bad[19] = 16
    assert rb(*bad) == EWORKSPACE
    gf, gb = lib.gmlm_geglu_tanh_fwd, lib.gmlm_geglu_tanh_bwd
    assert gf(A, 4, 1152, A, BF16, None) == ELAUNCH and gb(A, A, 4, 1152, A, F32, None) == ELAUNCH
    assert gf(A, 4, 1156, A, BF16, None) == EINVAL and gf(None, 0, 1152, None, BF16, None) == OK and gb(A, None, 4, 1152, A, F32, None) == EINVAL


def test_new_ops_fail_loudly_without_a_gpu(lib):
    """CPU tensors raise the library's error: no eager fallback behind the new operators."""
    from gmlm_amd import ops
    cs = torch.zeros(8, 2, 128)
    w = torch.zeros(256)
    with pytest.raises(_lib.GmlmHipError):
        ops.rope_gqa_d256(torch.zeros(1, 4, 1280), w, w, cs, None, 3, 1, 0.0625, True)
    with pytest.raises(_lib.GmlmHipError):
        ops.rope_gqa_d256_varlen(torch.zeros(4, 1280), w, w, cs, torch.arange(4), torch.tensor([0, 4], dtype=torch.int32), 4, 3, 1, 0.0625, False)
    with pytest.raises(_lib.GmlmHipError):
        ops.gqa_d256_attention(torch.zeros(1, 4, 768), torch.zeros(1, 4, 256), torch.zeros(1, 4, 256), None, 3, 1, 0.0625, True)
    with pytest.raises(_lib.GmlmHipError):
        ops.sandwich_rmsnorm(torch.zeros(2, 8), torch.zeros(2, 8), torch.zeros(8), torch.zeros(8))
    with pytest.raises(_lib.GmlmHipError):
        ops.geglu_tanh(torch.zeros(2, 16))


# --------------------------------------------------------------------------------------------------------- check_supported
def _cfg(**kw):
    from transformers import Gemma3TextConfig
    base = dict(vocab_size=96, hidden_size=384, intermediate_size=512, num_hidden_layers=3, num_attention_heads=3, num_key_value_heads=1,
                head_dim=256, max_position_embeddings=1024, sliding_window=512, sliding_window_pattern=3, pad_token_id=0)
    return Gemma3TextConfig(**{**base, **kw})


def test_check_supported_accepts_the_released_geometries():
    from gmlm_amd import gemma3
    # EmbeddingGemma-300m (bidirectional), gemma-3-270m, gemma-3-1b, and the 4b / 12b text towers (8 / 4 and 16 / 8 heads)
    for kw in (dict(hidden_size=768, intermediate_size=1152, num_hidden_layers=24, use_bidirectional_attention=True),
               dict(hidden_size=640, intermediate_size=2048, num_hidden_layers=18, num_attention_heads=4),
               dict(hidden_size=1152, intermediate_size=6912, num_hidden_layers=26, num_attention_heads=4),
               dict(hidden_size=2560, num_attention_heads=8, num_key_value_heads=4),
               dict(hidden_size=3840, num_attention_heads=16, num_key_value_heads=8,
                    rope_parameters={"full_attention": dict(rope_type="linear", factor=8.0, rope_theta=1e6),
                                     "sliding_attention": dict(rope_type="default", rope_theta=1e4)})):
        cfg = _cfg(**kw)
        assert cfg.model_type == "gemma3_text" and cfg.head_dim == 256
        gemma3.check_supported(_Holder(cfg))


_PROBLEMS = [
    (dict(head_dim=128), "head_dim=128"),
    (dict(hidden_activation="gelu"), "hidden_activation='gelu'"),
    (dict(attn_logit_softcapping=50.0), "attn_logit_softcapping=50.0"),
    (dict(attention_dropout=0.1), "attention_dropout=0.1"),
    (dict(attention_bias=True), "attention_bias"),
    (dict(num_attention_heads=3, num_key_value_heads=2), "3 query heads / 2 KV heads"),
    (dict(rope_parameters={"full_attention": dict(rope_type="yarn", factor=2.0, rope_theta=1e6),
                           "sliding_attention": dict(rope_type="default", rope_theta=1e4)}), "rope type 'yarn' of full_attention layers"),
    (dict(hidden_size=4608), "hidden_size=4608"),
]


def _broken(cfg, kws):
    for kw in kws:
        for k, v in kw.items():
            setattr(cfg, k, v)
    return cfg


@pytest.mark.parametrize("kw,word", _PROBLEMS, ids=[w for _, w in _PROBLEMS])
def test_check_supported_names_each_problem(kw, word):
    from gmlm_amd import gemma3
    with pytest.raises(NotImplementedError) as e:
        gemma3.check_supported(_Holder(_broken(_cfg(), [kw])))
    assert word in str(e.value) and str(e.value).count(";") == 0, str(e.value)


def test_check_supported_names_every_problem_at_once_and_the_modules_refuse_each_others_configs():
    from gmlm_amd import bert, deberta, eurobert, gemma3, llama, modernbert, mpnet, nomic_bert, qwen3
    from transformers import BertConfig, LlamaConfig
    cfg = _broken(_cfg(), [kw for kw, _ in _PROBLEMS])
    cfg.model_type = "gemma2"
    with pytest.raises(NotImplementedError) as e:
        gemma3.check_supported(_Holder(cfg))
    for word in ["model_type='gemma2'"] + [w for _, w in _PROBLEMS]:
        assert word in str(e.value), (word, str(e.value))
    for mod in (bert, qwen3, modernbert, mpnet, deberta, llama, eurobert, nomic_bert):
        with pytest.raises(NotImplementedError, match="model_type='gemma3_text'"):
            mod.check_supported(_Holder(_cfg()))
    small = dict(hidden_size=128, num_attention_heads=2, intermediate_size=192, num_hidden_layers=2, vocab_size=96)
    for other in (BertConfig(**small), LlamaConfig(**small, num_key_value_heads=1)):
        with pytest.raises(NotImplementedError, match=f"model_type='{other.model_type}'"):
            gemma3.check_supported(_Holder(other))


# -------------------------------------------------------------------------------------------------- rope tables, window
def _tiny(**kw):
    from transformers import Gemma3TextModel
    torch.manual_seed(0)
    return Gemma3TextModel(_cfg(**kw))


def test_rope_tables_are_the_hf_rotary_embedding_bit_for_bit():
    from gmlm_amd import gemma3
    n = 300
    linear = {"full_attention": dict(rope_type="linear", factor=8.0, rope_theta=1e6), "sliding_attention": dict(rope_type="default", rope_theta=1e4)}
    for kw in ({}, dict(rope_parameters=linear)):
        plm = _tiny(**kw)
        tables = gemma3.rope_tables(plm, n, "cpu")
        assert set(tables) == {"sliding_attention", "full_attention"}
        for lt, table in tables.items():
            assert table.dtype == torch.float32 and table.shape[0] >= n and tuple(table.shape[1:]) == (2, 128) and table.is_contiguous()
            cos, sin = plm.rotary_emb(torch.zeros(1, 1), torch.arange(n)[None], lt)             # [1, n, 256]: (freqs, freqs)
            assert cos.dtype == torch.float32 and torch.equal(cos[0, :, :128], cos[0, :, 128:])
            assert torch.equal(table[:n, 0], cos[0, :, :128]) and torch.equal(table[:n, 1], sin[0, :, :128]), lt
        assert not torch.equal(tables["sliding_attention"][:n], tables["full_attention"][:n])      # local and global base frequency
        assert gemma3.rope_tables(plm, 10, "cpu")["full_attention"] is tables["full_attention"]    # cached; a prefix serves
        if kw:
            plain = gemma3.rope_tables(_tiny(), n, "cpu")["full_attention"]
            assert not torch.equal(plain[:n], tables["full_attention"][:n])                        # the linear factor is in the table


def test_check_window_at_the_window_and_one_past_it_for_both_masks():
    from gmlm_amd import gemma3
    causal = _cfg(sliding_window=64)
    assert causal.sliding_window == 64
    gemma3.check_window(causal, 64)
    with pytest.raises(ValueError, match="sequence length 65 exceeds sliding_window 64"):
        gemma3.check_window(causal, 65)
    bidir = _cfg(sliding_window=512, use_bidirectional_attention=True)
    assert bidir.sliding_window == 257                                   # the config has turned 512 into 512 // 2 + 1
    gemma3.check_window(bidir, 257)
    with pytest.raises(ValueError, match="sequence length 258 exceeds sliding_window 257"):
        gemma3.check_window(bidir, 258)
    gemma3.check_window(_cfg(sliding_window=8, layer_types=["full_attention"] * 3), 500)      # no sliding layer: no limit
    # the rule restated on HF's own mask functions: every pair (i, j) of a sequence of L tokens is inside the window iff L <= w
    from transformers.masking_utils import sliding_window_overlay
    from transformers.models.gemma3.modeling_gemma3 import _bidirectional_window_overlay
    w = 5
    for L in (w, w + 1):
        inside_c = all(bool(sliding_window_overlay(w)(0, 0, i, j)) for i in range(L) for j in range(i + 1))
        inside_b = all(bool(_bidirectional_window_overlay(w)(0, 0, i, j)) for i in range(L) for j in range(L))
        assert inside_c == (L <= w) and inside_b == (L <= w)
    z = torch.zeros(8, dtype=torch.long)
    plm = _tiny()
    with pytest.raises(ValueError, match="exceeds max_position_embeddings 1024"):
        gemma3.gemma3_encode(plm, torch.zeros(1, 1025, dtype=torch.long), torch.tensor([1025], dtype=torch.int32), torch.float32)
    with pytest.raises(ValueError, match="exceeds sliding_window 512"):
        gemma3.gemma3_encode(plm, torch.zeros(1, 513, dtype=torch.long), torch.tensor([513], dtype=torch.int32), torch.float32)
    with pytest.raises(ValueError):
        gemma3.gemma3_encode_packed(plm, z, z[:7], torch.tensor([0, 8], dtype=torch.int32), 8, torch.float32)


# ---------------------------------------------------------------------------------------------------------- model wiring
def test_model_dispatches_gemma3_text():
    """Fails on the commit before this encoder: ``bert.check_supported`` raises NotImplementedError for the model type."""
    import gmlm_amd
    from gmlm_amd import bert, gemma3, model as model_mod
    plm = _tiny()
    model = gmlm_amd.GraphTextLM(12, 16, 3, plm_encoder=plm)
    assert model._enc is gemma3 and model._enc is not bert and model._plm_kind == "gemma3_text"
    assert model_mod._ENCODERS["gemma3_text"] == (gemma3, "gemma3_encode", "gemma3_encode_packed")
    assert gmlm_amd.gemma3_encode is gemma3.gemma3_encode and gmlm_amd.gemma3_encode_packed is gemma3.gemma3_encode_packed
    assert model._has_packed_pass() and model._packed_head_dim() == 0 and model._gqa_short_head_dim() == 0
    with pytest.raises(NotImplementedError, match="BERT-geometry encoders only"):
        model.capture_hip_graphs(torch.zeros(4, 12), torch.zeros(2, 4, dtype=torch.long))
    keys = {k[len("plm_encoder."):] for k in model.state_dict() if k.startswith("plm_encoder.")}
    assert keys == set(plm.state_dict())
    assert {"embed_tokens.weight", "norm.weight", "layers.0.self_attn.q_norm.weight", "layers.2.pre_feedforward_layernorm.weight",
            "layers.1.post_feedforward_layernorm.weight", "layers.0.mlp.gate_proj.weight"} <= keys


def test_prepare_weights_fuses_the_projections_and_chains_the_norms():
    from gmlm_amd import gemma3
    plm = _tiny()
    lws = gemma3.prepare_weights(plm, torch.float32)
    assert len(lws) == 3 and [lw.layer_type for lw in lws] == ["sliding_attention", "sliding_attention", "full_attention"]
    for i, (lw, layer) in enumerate(zip(lws, plm.layers)):
        sa, mlp = layer.self_attn, layer.mlp
        assert tuple(lw.wqkv.shape) == (1280, 384) and not lw.wqkv.requires_grad              # (3 + 2 * 1) heads of 256
        assert torch.equal(lw.wqkv, torch.cat([sa.q_proj.weight, sa.k_proj.weight, sa.v_proj.weight]))
        assert torch.equal(lw.wgu, torch.cat([mlp.gate_proj.weight, mlp.up_proj.weight]))
        assert torch.equal(lw.wo, sa.o_proj.weight) and torch.equal(lw.wdown, mlp.down_proj.weight)
        assert lw.m_qkv == (sa.q_proj.weight, sa.k_proj.weight, sa.v_proj.weight) and lw.m_gu == (mlp.gate_proj.weight, mlp.up_proj.weight)
        assert lw.qn is sa.q_norm.weight and lw.kn is sa.k_norm.weight
        assert lw.ln_post_attn is layer.post_attention_layernorm.weight and lw.ln_pre_ff is layer.pre_feedforward_layernorm.weight
        assert lw.ln_post_ff is layer.post_feedforward_layernorm.weight
        assert lw.ln_next is (plm.layers[i + 1].input_layernorm.weight if i < 2 else plm.norm.weight)
    with pytest.raises(ValueError):
        gemma3.prepare_weights(plm, torch.bfloat16, "bf16x3")               # gemm_precision is passed through and checked


# ------------------------------------------------------------------------------------------------ the budgets, in fp32
def _tanh_glu_fp32(gu, gy):
    """TanhGeluAct of csrc/gemma_kernels.hip, operation for operation in torch fp32."""
    inter = gu.shape[-1] // 2
    g, up, d = gu[:, :inter].float(), gu[:, inter:].float(), gy.float()
    ka, kb = torch.tensor(KA, dtype=torch.float32), torch.tensor(KB, dtype=torch.float32)
    g2 = g * g
    u = ka * g * (kb * g2 + 1.0)
    e = torch.exp(-2.0 * u.abs())
    big = 1.0 / (1.0 + e)
    small = e * big
    sig, co = torch.where(u >= 0, big, small), torch.where(u >= 0, small, big)
    du2 = 2.0 * ka * (3.0 * kb * g2 + 1.0)
    return g * sig * up, d * g * sig, d * up * sig * (g * co * du2 + 1.0)


def test_geglu_tanh_budgets_hold_in_fp32_saturated_gates_included():
    """At most HALF the absolute extras the GPU file applies (the rounding to the storage type has the budget's ulp term to
    itself); saturated gates give exactly g * up / 0 and nothing is NaN."""
    for rows, inter in GLU_SHAPES:
        for dtype in (torch.bfloat16, torch.float32):
            gu, gy = geglu_inputs(rows, inter, dtype)
            got = _tanh_glu_fp32(gu, gy)
            assert all(t.dtype == torch.float32 and bool(torch.isfinite(t).all()) for t in got)
            for name, a, (r, extra) in zip(("y", "d up", "d gate"), got, geglu_reference(gu, gy)):
                err = (a.double() - r).abs()
                floor = 2.0 ** -149                                   # fp32 flushes what float64 still holds (the GPU file's ulp clamp)
                assert bool((err <= 0.5 * extra + floor).all()), (rows, inter, dtype, name, float((err / extra.clamp_min(1e-300)).max()))
            if inter == 80:
                cols = torch.arange(inter) % 10
                hi, lo = (cols == 2) | (cols == 4) | (cols == 6), (cols == 3) | (cols == 5) | (cols == 7)
                g, up = gu[:, :inter].float(), gu[:, inter:].float()
                assert torch.equal(got[0][:, hi], g[:, hi] * up[:, hi]) and float(got[0][:, lo].abs().max()) == 0.0
                assert torch.equal(got[2][:, hi], gy.float()[:, hi] * up[:, hi]) and float(got[2][:, lo].abs().max()) == 0.0


def test_sandwich_budgets_hold_in_fp32():
    """sandwich_fwd_kernel's and sandwich_bwd_kernel's expressions in torch fp32 on the GPU file's inputs: at most half its
    absolute extras; on the all-zero row rstd is eps^-1/2 within 2 u and s', y are exactly 0."""
    eps = torch.tensor(EPS, dtype=torch.float32)
    for f in SAND_WIDTHS:
        for rows in SAND_ROWS:
            for dtype in (torch.bfloat16, torch.float32):
                s, b, gy, gs, wpo, wpr = sandwich_inputs(rows, f, dtype)
                off = 1.0
                sf, bf = s.float(), b.float()
                rb = 1.0 / torch.sqrt(bf.pow(2).mean(-1, keepdim=True) + eps)
                sp32 = sf + bf * rb * (off + wpo)
                sp = sp32.to(dtype)                                   # the stored sum
                spf = sp.float()
                rs = 1.0 / torch.sqrt(spf.pow(2).mean(-1, keepdim=True) + eps)
                y = spf * rs * (off + wpr)
                g = gy.float() * (off + wpr)
                xh = spf * rs
                ds = rs * (g - xh * (g * xh).mean(-1, keepdim=True)) + gs.float()
                h = ds * (off + wpo)
                bh = bf * rb
                db = rb * (h - bh * (h * bh).mean(-1, keepdim=True))
                ref = sandwich_reference(s, b, sp, wpo, wpr, off, gy, gs)
                for name, a in (("sp", sp32), ("y", y), ("ds", ds), ("db", db)):
                    r, extra = ref[name]
                    assert a.dtype == torch.float32
                    err = (a.double() - r).abs()
                    assert bool((err <= 0.5 * extra).all()), (f, rows, dtype, name, float((err / extra.clamp_min(1e-300)).max()))
                if rows == 3:
                    want = float(eps.double().rsqrt())
                    assert abs(float(rb[1]) - want) <= 2 * U * want and abs(float(rs[1]) - want) <= 2 * U * want
                    assert float(sp32[1].abs().max()) == 0.0 and float(y[1].abs().max()) == 0.0


# --------------------------------------------------------------------------------------------------------- code objects
def test_compiled_kernels_are_the_ones_the_static_profile_lists_without_scratch():
    """profiles/gqa_wide_static.json (tools/gqa_wide_static.py: the compiler's resource-usage remarks) names every gqaw:: and
    gemma_kernels kernel of the built library, and none of them uses scratch or spills."""
    prof = json.load(open(os.path.join(ROOT, "profiles", "gqa_wide_static.json")))
    listed = {r["kernel"][len("gmlm::"):] for r in prof["kernels"]}
    got = _compiled_kernels(lambda name: name.startswith("gqaw::") or "gemma_kernels" in name)
    assert got == listed, (sorted(got - listed), sorted(listed - got))
    assert len([n for n in got if n.startswith("gqaw::")]) == 2 * 2 * 3 + 2                # dtype x mask x (fwd, dq, dkv) + delta
    for r in prof["kernels"]:
        assert r["scratch_bytes_per_lane"] == 0 and r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0, r
        if "dynamic_lds_bytes" in r:
            assert r["dynamic_lds_bytes"] == (83200 if "<float" in r["kernel"] else 50432) and r["static_lds_bytes"] == 0
