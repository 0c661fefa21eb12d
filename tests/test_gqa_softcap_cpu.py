"""Host side of the soft-capped grouped-KV attention at head dim 256 and of the Gemma2 encoder (no GPU needed): the fifteenth
header (include/gmlm_hip_gqa_softcap.h), its ctypes table ``_lib.SIGNATURES_GQA_SOFTCAP`` and the exported symbols agree type by
type; the attention argument lists are those of their ``gmlm_attention_gqa_d256_band_*`` namesakes plus ``softcap`` after
``window``, the rotary pair's those of ``gmlm_rope_heads_*``; the entry points decide every documented refusal on the host, in
order (window: 0 and [1, 2^30) accepted; softcap: finite and > 0, checked after the window), and return GMLM_OK for an empty call
without pointers; ``gemma2.check_supported`` names every problem; the encoder routes its layers to the soft-capped entry points
with the window only on sliding layers of a call past it; the new autograd nodes keep the frozen-input contract; and
``softcap_reference``, the float64 restatement the GPU tests check the kernels against, is transformers' own
``eager_attention_forward`` of modeling_gemma2 (scores, cap, then mask; K and V repeated over the group)."""
import math
import os
import re

import pytest
import torch

from conftest import ROOT
from gmlm_amd import _lib, dense, gemma2, gemma3, model, ops, ops_gemma, ops_softcap
from test_abi_contract_cpu import parse_header, signature_mismatches
from test_attention_routes_cpu import Recorder, STREAM
from test_autograd_contract_cpu import Case, _cu, _gen, _pos, _r, assert_contract, patterns, rope_table, run_pattern

OK, EINVAL, EWORKSPACE, ELAUNCH = 0, -1, -2, -3
F32, BF16 = 0, 1
A = 0x10000000        # fabricated, non-null, 16-byte aligned: every call below ends before or at the launch
D = 256
NEG = float("-inf")
HEADER = os.path.join(ROOT, "include", "gmlm_hip_gqa_softcap.h")
STEM, BAND, PLAIN = "gmlm_attention_gqa_d256_softcap", "gmlm_attention_gqa_d256_band", "gmlm_attention_gqa_d256"
TAILS = ("_fwd", "_bwd", "_bwd_workspace_bytes", "_varlen_fwd", "_varlen_bwd", "_varlen_bwd_workspace_bytes")
ROPE = ("gmlm_rope_heads_d256_fwd", "gmlm_rope_heads_d256_bwd")

no_device = pytest.mark.skipif(torch.cuda.device_count() > 0,
                               reason="fabricated addresses: only meaningful (and only safe) without a device")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libgmlm_hip.so not built")
    return _lib.lib()


# ------------------------------------------------------------------------------------------- the float64 restatement
def visible(n, kv, window, causal, device=None):
    """bool [.., n, n]: j < kv and (0 <= i - j < window if causal else |i - j| < window); ``window`` 0: no band; ``kv`` a number
    or a [b] tensor"""
    i, j = torch.arange(n, device=device)[:, None], torch.arange(n, device=device)[None, :]
    band = (i >= j) if causal else torch.ones(n, n, dtype=torch.bool, device=device)
    if window:
        band = band & ((i - j).abs() < window)
    if torch.is_tensor(kv):
        return band[None] & (j[None] < kv[:, None, None])
    return band & (j < kv)


def softcap_reference(q, k, v, go, kv, hq, hkv, scale, causal, softcap, window=0):
    """q, go [b, L, hq * D], k, v [b, L, hkv * D], kv int [b] -> out, dq, dk, dv, lse in float64.  Scores of the query head
    against its KV head times ``scale``, then ``softcap * tanh(. / softcap)`` (``softcap`` None: no cap), then the mask, softmax,
    K / V repeated over the group under autograd.  A query without a visible key gives a zero row (and takes no part in the
    backward); its lse is -inf.  The computation of tests/test_gpu_gqa_band_kernels._reference with the cap before its mask."""
    b, L = q.shape[:2]
    g = hq // hkv
    heads = lambda t, h: t.double().reshape(b, L, h, D).transpose(1, 2).contiguous().requires_grad_(True)
    qq, kk, vv = heads(q, hq), heads(k, hkv), heads(v, hkv)
    mask = visible(L, kv, window, causal, q.device)[:, None]                 # [b, 1, L, L]
    some = mask.any(-1, keepdim=True)
    s = (qq @ kk.repeat_interleave(g, 1).transpose(2, 3)) * scale
    if softcap is not None:
        s = torch.tanh(s / softcap) * softcap
    p = torch.softmax(s.masked_fill(~(mask | ~some), NEG), -1) * some       # a row that sees nothing: uniform, then times 0
    o = p @ vv.repeat_interleave(g, 1)
    o.backward(go.double().reshape(b, L, hq, D).transpose(1, 2))
    lse = torch.logsumexp(s.detach().masked_fill(~mask, NEG), -1)           # [b, hq, L]; -inf where nothing is visible
    back = lambda t: t.transpose(1, 2).reshape(b, L, -1)
    return back(o.detach()), back(qq.grad), back(kk.grad), back(vv.grad), lse


@pytest.mark.parametrize("window", [0, 8], ids=("full", "window8"))
@pytest.mark.parametrize("cap", [50.0, 4.0, 1.0])
def test_the_float64_restatement_is_hf_eager_attention_forward(cap, window, monkeypatch):
    """Seeded inputs at L = 33, heads 4 / 2, kv_len 33 and 20: transformers' ``eager_attention_forward`` of modeling_gemma2 with
    ``softcap = cap`` and an additive 0 / -inf mask of the stated rule, forward and (through autograd) backward, to 1e-12.  The
    queries at or past kv_len + window - 1 see no key: HF gives NaN there, the restatement zeros, so they are left out.
    HF asks its softmax for ``dtype=torch.float32`` (an UPcast for the half-precision models it is written for), which would
    round these float64 scores to fp32 (measured: 1e-7); the softmax it calls is given the dtype of its input here, nothing else
    of the function is touched."""
    from transformers.models.gemma2 import modeling_gemma2
    from transformers.models.gemma2.modeling_gemma2 import eager_attention_forward
    real = torch.nn.functional.softmax
    monkeypatch.setattr(modeling_gemma2.nn.functional, "softmax", lambda x, dim=None, dtype=None: real(x, dim=dim, dtype=x.dtype))
    hq, hkv, L, b, scale = 4, 2, 33, 2, 1.0 / 12.0
    g = torch.Generator().manual_seed(7)
    q = torch.randn(b, L, hq * D, generator=g, dtype=torch.float64)
    k = 1.5 * torch.randn(b, L, hkv * D, generator=g, dtype=torch.float64)
    v = torch.randn(b, L, hkv * D, generator=g, dtype=torch.float64)
    go = torch.randn(b, L, hq * D, generator=g, dtype=torch.float64)
    kv = torch.tensor([L, 20])
    mask = visible(L, kv, window, True)[:, None]
    some = mask.any(-1)[:, 0]                                                # [b, L]
    assert bool(some[0].all()) and (bool(some[1].all()) if not window else int((~some[1]).sum()) == L - 27)
    go = go * some[..., None]
    mine = softcap_reference(q, k, v, go, kv, hq, hkv, scale, True, cap, window)

    class Module(torch.nn.Module):
        num_key_value_groups, head_dim, training = hq // hkv, D, False
    heads = lambda t, h: t.reshape(b, L, h, D).transpose(1, 2).contiguous().requires_grad_(True)
    qq, kk, vv = heads(q, hq), heads(k, hkv), heads(v, hkv)
    add = torch.zeros(b, 1, L, L, dtype=torch.float64).masked_fill(~(mask | ~some[:, None, :, None]), NEG)
    out, probs = eager_attention_forward(Module(), qq, kk, vv, add, dropout=0.0, scaling=scale, softcap=cap)   # [b, L, hq, D]
    (out * go.reshape(b, L, hq, D)).sum().backward()
    back = lambda t: t.transpose(1, 2).reshape(b, L, -1)
    theirs = (out.detach().reshape(b, L, -1) * some[..., None], back(qq.grad), back(kk.grad), back(vv.grad))
    for name, a, r in zip(("out", "dq", "dk", "dv"), mine, theirs):
        err = float((a - r).abs().max()) / max(1.0, float(r.abs().max()))
        assert err <= 1e-12, (name, err)
    # the cap matters at 4 and 1 (scores reach several units) and the order matters: capping after the mask un-masks
    plain = softcap_reference(q, k, v, go, kv, hq, hkv, scale, True, None, window)[0]
    differs = float((mine[0] - plain).norm() / plain.norm())
    assert differs >= 0.1 if cap <= 4 else differs > 0, differs
    s = torch.full((3,), NEG, dtype=torch.float64)
    assert torch.equal(torch.tanh(s / cap) * cap, torch.full((3,), -cap, dtype=torch.float64))


# ------------------------------------------------------------------------------------------------------------------ ABI
def _names(protos, name):
    return [n for _, n in protos[name][1]]


def test_header_ctypes_table_and_exports_agree(lib):
    table = _lib.SIGNATURES_GQA_SOFTCAP
    text = open(HEADER).read()
    protos = parse_header(text)
    assert sorted(protos) == sorted([STEM + t for t in TAILS] + list(ROPE)) and len(protos) == 8
    assert not signature_mismatches(protos, table)
    for name in protos:
        assert hasattr(lib, name), f"{name} declared in include/gmlm_hip_gqa_softcap.h but not exported"
        assert getattr(lib, name).argtypes == table[name][1]                                  # lib() bound the new table
    later = _lib.SIGNATURE_TABLES_LATER
    assert later[0] is _lib.SIGNATURES_RELBIAS and later[-1] is _lib.SIGNATURES_DISENT
    assert any(t is table for t in later[1:-1]) and not any(t is table for t in _lib.SIGNATURE_TABLES)
    others = set().union(*(set(t) for t in _lib.SIGNATURE_TABLES + later if t is not table))
    assert not set(table) & others
    assert lib.gmlm_version() == 1
    assert '#include "gmlm_hip.h"' in text and 'extern "C"' in text
    band = parse_header(open(os.path.join(ROOT, "include", "gmlm_hip_gqa_band.h")).read())
    assert not set(band) & set(protos) and len(band) == 6                                      # the fourteenth header is as it was


def test_argument_lists_are_the_band_namesakes_plus_softcap_after_window():
    band = parse_header(open(os.path.join(ROOT, "include", "gmlm_hip_gqa_band.h")).read())
    gqa = parse_header(open(os.path.join(ROOT, "include", "gmlm_hip_gqa.h")).read())
    protos = parse_header(open(HEADER).read())
    for tail in ("_fwd", "_bwd", "_varlen_fwd", "_varlen_bwd"):
        old, new = band[BAND + tail], protos[STEM + tail]
        i = _names(band, BAND + tail).index("window") + 1
        assert new[0] == old[0] and new[1] == old[1][:i] + [("float", "softcap")] + old[1][i:], tail
    for tail in ("_bwd_workspace_bytes", "_varlen_bwd_workspace_bytes"):
        assert protos[STEM + tail] == band[BAND + tail]
    for tail in ("_fwd", "_bwd"):
        assert protos["gmlm_rope_heads_d256" + tail] == gqa["gmlm_rope_heads" + tail]


def test_the_makefile_names_the_new_source_and_header():
    mk = open(os.path.join(ROOT, "gmlm_amd", "csrc", "Makefile")).read()
    srcs = re.search(r"^SRCS\s*=(.*)$", mk, re.M).group(1).split()
    assert "attn_gqa_softcap.hip" in srcs and os.path.exists(os.path.join(ROOT, "gmlm_amd", "csrc", "attn_gqa_softcap.hip"))
    deps = re.search(r"^\$\(BUILD\)/%\.o:(.*)$", mk, re.M).group(1).split()
    assert "../../include/gmlm_hip_gqa_softcap.h" in deps


# ------------------------------------------------------------------------------------------------- entry-point refusals
W = 1280 + 8        # (3 + 2) heads of 256 and 8 more: the fused rows are wider than [q | k | v]
_BASE = dict(q=A, k=A, v=A, kv_len=None, b=2, hq=3, hkv=1, lq=64, lk=64, d=256, q_stride=W, k_stride=W, v_stride=W, scale=0.0625,
             dropout_p=0.0, causal=1, window=40, softcap=50.0, out=A, out_lo=None, lse=A, dtype=BF16, stream=None, dout=A, dq=A, dk=A,
             dv=A, dq_stride=W, dk_stride=W, dv_stride=W, workspace=A, workspace_bytes=1 << 40, cu_seqlens=A, num_seqs=2, max_len=64,
             total_rows=100)
_LISTS = {w: _names(parse_header(open(HEADER).read()), f"{STEM}_{w}") for w in ("fwd", "bwd", "varlen_fwd", "varlen_bwd")}
WHICH = tuple(_LISTS)
BAD_WINDOWS = (-1, 1 << 30)
BAD_CAPS = (0.0, -1.0, math.inf, -math.inf, math.nan)


def _call(lib, which, **mut):
    a = dict(_BASE, **mut)
    return getattr(lib, f"{STEM}_{which}")(*[a[n] for n in _LISTS[which]]), lib.gmlm_last_error()


# the family's refusals documented before the window check, in that order, and those after the cap check
_BEFORE = [(dict(hq=0), b"bad sizes"), (dict(d=128), b"head dim"), (dict(dtype=2), b"dtype"), (dict(out_lo=A, dtype=F32), b"out_lo"),
           (dict(lq=63), b"lq == lk"), (dict(hq=3, hkv=2), b"multiple of"), (dict(dropout_p=0.1), b"dropout"), (dict(scale=0.0), b"scale")]
_AFTER = [(dict(q_stride=760), b"stride"), (dict(q=A + 8), b"aligned"), (dict(k=None), b"null")]
_PACKED_FIRST = [(dict(cu_seqlens=None), b"cu_seqlens"), (dict(max_len=0), b"max_len"), (dict(total_rows=-1), b"packed rows")]


@no_device
@pytest.mark.parametrize("which", WHICH)
def test_window_and_softcap_refusals_and_their_place_in_the_order(lib, which):
    packed = which.startswith("varlen")
    for w in BAD_WINDOWS:
        rc, err = _call(lib, which, window=w)
        assert rc == EINVAL and b": window" in err, (w, rc, err)
        rc, err = _call(lib, which, window=w, softcap=0.0)                                    # the window is checked first
        assert rc == EINVAL and b": window" in err and b": softcap" not in err, (w, rc, err)
    for w in (0, 1, 2, 257, (1 << 30) - 1):
        assert _call(lib, which, window=w)[0] == ELAUNCH, w                                   # valid: ends at the launch (no device)
    for c in BAD_CAPS:
        for w in (0, 40):
            rc, err = _call(lib, which, softcap=c, window=w)
            assert rc == EINVAL and b": softcap" in err, (c, w, rc, err)
    for c in (1e-3, 1.0, 50.0, 1e6):
        assert _call(lib, which, softcap=c)[0] == ELAUNCH, c
    before = [(m, msg) for m, msg in _BEFORE if not (packed and "lq" in m)] + (_PACKED_FIRST if packed else [])
    for mut, msg in before:                                             # each is decided before a bad window and a bad cap
        for bad in (dict(), dict(window=-1), dict(softcap=0.0), dict(window=-1, softcap=math.nan)):
            rc, err = _call(lib, which, **bad, **mut)
            assert rc == EINVAL and msg in err, (mut, bad, rc, err)
    for i, (mut, msg) in enumerate(_BEFORE):                            # the documented order among the family's own refusals
        if packed and "lq" in mut:
            continue
        later = {}
        for m, _ in _BEFORE[i + 1:]:
            if not (packed and "lq" in m) and not set(m) & set(mut):
                later.update(m)
        rc, err = _call(lib, which, **later, **mut)
        assert rc == EINVAL and msg in err, (mut, later, rc, err)
    for mut, msg in _AFTER:                                             # the operand checks come after both
        rc, err = _call(lib, which, **mut)
        assert rc == EINVAL and msg in err, (mut, rc, err)
        rc, err = _call(lib, which, softcap=-2.0, **mut)
        assert rc == EINVAL and b": softcap" in err, (mut, rc, err)
        rc, err = _call(lib, which, window=-1, **mut)
        assert rc == EINVAL and b": window" in err, (mut, rc, err)
    if which.endswith("bwd"):
        assert _call(lib, which, workspace=None)[0] == EWORKSPACE and _call(lib, which, workspace=None, softcap=0.0)[0] == EINVAL
        assert _call(lib, which, workspace_bytes=8)[0] == EWORKSPACE


@no_device
def test_nothing_to_do_needs_no_pointer_but_sizes_window_and_softcap_are_still_checked(lib):
    nothing = dict(q=None, k=None, v=None, out=None, lse=None, dout=None, dq=None, dk=None, dv=None, workspace=None, workspace_bytes=0)
    for which, empties in (("fwd", (dict(b=0), dict(lq=0, lk=0))), ("bwd", (dict(b=0), dict(lq=0, lk=0))),
                           ("varlen_fwd", (dict(num_seqs=0), dict(total_rows=0))), ("varlen_bwd", (dict(num_seqs=0), dict(total_rows=0)))):
        for empty in empties:
            for w in (0, 40):
                assert _call(lib, which, window=w, **nothing, **empty)[0] == OK, (which, empty, w)
            for mut, msg in ((dict(d=128), b"head dim"), (dict(dropout_p=0.5), b"dropout"), (dict(dtype=5), b"dtype"), (dict(window=-1), b"window"),
                             (dict(window=1 << 30), b"window"), (dict(softcap=0.0), b": softcap"), (dict(softcap=math.nan), b": softcap")):
                rc, err = _call(lib, which, **nothing, **empty, **mut)
                assert rc == EINVAL and msg in err, (which, empty, mut, rc, err)
    assert lib.gmlm_attention_gqa_d256_softcap_bwd_workspace_bytes(2, 3, 300) == lib.gmlm_attention_gqa_d256_bwd_workspace_bytes(2, 3, 300)
    assert lib.gmlm_attention_gqa_d256_softcap_varlen_bwd_workspace_bytes(100, 3) == 3 * 100 * 4


_ROPE_BASE = dict(qkv=A, dqkv=A, qkv_stride=W, dqkv_stride=W, cos_sin=A, max_len=64, tokens=128, seq_len=64, pos_ids=None, heads=4, d=256,
                  dtype=BF16, stream=None)


def _rope(lib, name, **mut):
    a = dict(_ROPE_BASE, **mut)
    names = _names(parse_header(open(HEADER).read()), name)
    return getattr(lib, name)(*[a[n] for n in names]), lib.gmlm_last_error()


@no_device
@pytest.mark.parametrize("name", ROPE)
def test_rope_heads_d256_takes_256_only_and_keeps_the_family_checks(lib, name):
    assert _rope(lib, name)[0] == ELAUNCH
    assert _rope(lib, name, pos_ids=A, seq_len=0)[0] == ELAUNCH
    for d in (64, 128, 512):
        rc, err = _rope(lib, name, d=d)
        assert rc == EINVAL and b"head dim" in err and b"takes 256" in err, (d, rc, err)
    old = name.replace("_d256", "")
    a = dict(_ROPE_BASE, d=256)
    rc = getattr(lib, old)(*[a[n] for n in _names(parse_header(open(os.path.join(ROOT, "include", "gmlm_hip_gqa.h")).read()), old)])
    assert rc == EINVAL and b"takes 64 or 128" in lib.gmlm_last_error()                   # and gmlm_rope_heads_* still refuses 256
    for mut, msg in ((dict(dtype=2), b"dtype"), (dict(heads=0), b"bad sizes"), (dict(max_len=0), b"empty cos / sin"),
                     (dict(seq_len=65), b"exceeds"), (dict(seq_len=0), b"length 0"), (dict(qkv_stride=1000, dqkv_stride=1000), b"stride"),
                     (dict(qkv_stride=W + 4, dqkv_stride=W + 4), b"stride"), (dict(qkv=None, dqkv=None), b"null"),
                     (dict(qkv=A + 8, dqkv=A + 8), b"aligned"), (dict(cos_sin=None), b"cos / sin")):
        rc, err = _rope(lib, name, **mut)
        assert rc == EINVAL and msg in err, (mut, rc, err)
    assert _rope(lib, name, tokens=0, qkv=None, dqkv=None, cos_sin=None)[0] == OK
    assert _rope(lib, name, tokens=0, seq_len=0, qkv=None, dqkv=None, cos_sin=None)[0] == OK
    rc, err = _rope(lib, name, tokens=0, qkv=None, dqkv=None, d=128)
    assert rc == EINVAL and b"head dim" in err


def test_new_ops_fail_loudly_without_a_gpu(lib):
    """CPU tensors raise the library's error: no eager fallback behind the new operators."""
    q, k = torch.zeros(1, 4, 768), torch.zeros(1, 4, 256)
    cu = torch.tensor([0, 4], dtype=torch.int32)
    cs = torch.zeros(8, 2, 128)
    with pytest.raises(_lib.GmlmHipError):
        ops.gqa_d256_softcap_attention(q, k, k, None, 3, 1, 0.0625, True, 50.0)
    with pytest.raises(_lib.GmlmHipError):
        ops.gqa_d256_softcap_attention_varlen(q[0], k[0], k[0], cu, 4, 3, 1, 0.0625, False, 50.0, window=2)
    with pytest.raises(_lib.GmlmHipError):
        ops.rope_heads_d256_(torch.zeros(1, 4, 1280), cs, 4, 4)
    for cap in (50.0, None):
        with pytest.raises(_lib.GmlmHipError):
            ops.rope_softcap_gqa_d256(torch.zeros(1, 4, 1280), cs, None, 3, 1, 0.0625, True, cap)
    for c in BAD_CAPS:
        with pytest.raises(ValueError, match="softcap"):
            ops.gqa_d256_softcap_attention(q, k, k, None, 3, 1, 0.0625, True, c)
    for w in BAD_WINDOWS:
        with pytest.raises(ValueError, match="window"):
            ops.gqa_d256_softcap_attention(q, k, k, None, 3, 1, 0.0625, True, 4.0, w)


# ---------------------------------------------------------------------------------------------------- check_supported
def _config(**kw):
    from transformers import Gemma2Config
    base = dict(vocab_size=96, hidden_size=96, intermediate_size=64, num_hidden_layers=3, num_attention_heads=3, num_key_value_heads=1,
                head_dim=256, max_position_embeddings=64, sliding_window=8, pad_token_id=0, query_pre_attn_scalar=144,
                attn_logit_softcapping=50.0)
    base.update(kw)
    return Gemma2Config(**base)


class _Plm:
    def __init__(self, cfg):
        self.config = cfg


_PROBLEMS = [
    (dict(head_dim=128), "head_dim=128"),
    (dict(hidden_activation="gelu"), "hidden_activation='gelu'"),
    (dict(attention_dropout=0.1), "attention_dropout=0.1"),
    (dict(attention_bias=True), "attention_bias"),
    (dict(num_attention_heads=3, num_key_value_heads=2), "3 query heads / 2 KV heads"),
    (dict(hidden_size=4608), "hidden_size=4608"),
    (dict(layer_types=["sliding_attention", "chunked_attention", "full_attention"]), "layer type 'chunked_attention'"),
    (dict(rope_parameters=dict(rope_type="dynamic", factor=2.0, rope_theta=10000.0)), "rope type 'dynamic'"),
]


def test_check_supported_accepts_gemma2_and_names_each_problem_alone_and_all_at_once():
    gemma2.check_supported(_Plm(_config()))
    gemma2.check_supported(_Plm(_config(attn_logit_softcapping=None)))                    # runs uncapped
    gemma2.check_supported(_Plm(_config(final_logit_softcapping=30.0)))                   # the LM head's: ignored
    gemma2.check_supported(_Plm(_config(rope_parameters=dict(rope_type="linear", factor=2.0, rope_theta=10000.0))))
    for kw, word in _PROBLEMS:
        try:
            cfg = _config(**kw)
        except Exception as e:                                          # a config this transformers refuses to build: set it after
            cfg = _config()
            for k_, v_ in kw.items():
                setattr(cfg, k_, v_)
            assert cfg is not None, e
        with pytest.raises(NotImplementedError) as e:
            gemma2.check_supported(_Plm(cfg))
        msg = str(e.value)
        assert word in msg, (kw, msg)
        assert sum(w in msg for _, w in _PROBLEMS if w != word and not (w == "attention_bias" and "attention_bias" in word)) == 0, msg
    cfg = _config()
    for kw, _ in _PROBLEMS:
        for k_, v_ in kw.items():
            setattr(cfg, k_, v_)
    cfg.num_attention_heads, cfg.num_key_value_heads = 3, 2
    cfg.model_type = "gemma"
    with pytest.raises(NotImplementedError) as e:
        gemma2.check_supported(_Plm(cfg))
    for word in ["model_type='gemma'"] + [w for _, w in _PROBLEMS]:
        assert word in str(e.value), (word, str(e.value))


def test_other_encoders_configs_are_refused_by_model_type_and_the_dispatch_resolves():
    from transformers import BertConfig, Gemma3TextConfig, LlamaConfig, Qwen3Config
    for cfg in (Gemma3TextConfig(head_dim=256), LlamaConfig(), Qwen3Config(), BertConfig()):
        with pytest.raises(NotImplementedError, match="model_type=" + repr(cfg.model_type)):
            gemma2.check_supported(_Plm(cfg))
    with pytest.raises(NotImplementedError, match="model_type='gemma2'"):
        gemma3.check_supported(_Plm(_config()))                             # and the Gemma3 module still refuses a Gemma2
    mod, padded, packed = model._ENCODERS["gemma2"]
    assert mod is gemma2 and getattr(mod, padded) is gemma2.gemma2_encode and getattr(mod, packed) is gemma2.gemma2_encode_packed
    for name in ("prepare_weights", "rope_tables", "check_supported"):
        assert callable(getattr(gemma2, name))
    import gmlm_amd
    assert gmlm_amd.gemma2_encode is gemma2.gemma2_encode and gmlm_amd.gemma2_encode_packed is gemma2.gemma2_encode_packed


# -------------------------------------------------------------------------------------------------------- host routing
@pytest.fixture
def rec(monkeypatch):
    """The recorder lib of test_attention_routes_cpu.py behind ops.py, ops_gemma.py and ops_softcap.py; GEMMs run in fp32 on the
    host."""
    r = Recorder()
    for mod in (ops, ops_gemma, ops_softcap):
        monkeypatch.setattr(mod, "lib", lambda: r)
        monkeypatch.setattr(mod, "check", lambda rc, what="": r.checked.append(what))
    monkeypatch.setattr(ops, "_cuda", lambda *ts: None)
    monkeypatch.setattr(ops, "_stream", lambda: STREAM)
    monkeypatch.setattr(ops, "SEED_DEVICE", None)

    def f32_out(op, *args, out=None, **kw):
        res = getattr(torch, op)(*[a.float() for a in args])
        return res if out is None else out.copy_(res)
    monkeypatch.setattr(dense, "_f32_out", f32_out)
    return r


def _tiny(cap=50.0, window=8):
    from transformers import Gemma2Model
    torch.manual_seed(0)
    return Gemma2Model(_config(attn_logit_softcapping=cap, sliding_window=window))


def _calls(rec):
    protos = parse_header(open(HEADER).read())
    for h in ("gmlm_hip_gqa_wide.h", "gmlm_hip_gqa_band.h"):
        protos.update(parse_header(open(os.path.join(ROOT, "include", h)).read()))
    out = []
    for name, args in rec.take():
        if (name.startswith("gmlm_attention") or "rope" in name) and not name.endswith("workspace_bytes"):
            out.append((name, dict(zip(_names(protos, name), args))))
    return out


@pytest.mark.parametrize("packed", [False, True], ids=("padded", "packed"))
@pytest.mark.parametrize("cap", [50.0, None], ids=("cap50", "nocap"))
def test_the_encoder_routes_its_layers(rec, cap, packed):
    """Layer types sliding, full, sliding.  Capped: every layer calls the soft-capped entry point, causal, scale 1 / 12, with
    ``softcap`` = the config's; window = sliding_window on the sliding layers of a call past it, else 0.  Uncapped: the entry
    points of the Gemma3 encoder (band on those sliding layers).  Every layer rotates with gmlm_rope_heads_d256_* and none calls
    a head norm."""
    plm = _tiny(cap)
    w = plm.config.sliding_window
    assert w == 8 and gemma3._layer_types(plm.config) == ["sliding_attention", "full_attention", "sliding_attention"]
    tail = "_varlen" if packed else ""

    def run(longest, train=False):
        lens = [longest, 2]
        if packed:
            tok = torch.ones(sum(lens), dtype=torch.long)
            pos = torch.cat([torch.arange(n) for n in lens])
            cu = torch.tensor([0, lens[0], sum(lens)], dtype=torch.int32)
            out = gemma2.gemma2_encode_packed(plm, tok, pos, cu, longest, torch.float32, training=train)
        else:
            out = gemma2.gemma2_encode(plm, torch.ones(2, longest, dtype=torch.long), torch.tensor(lens, dtype=torch.int32), torch.float32,
                                       training=train)
        return out, _calls(rec)

    for longest in (w - 1, w, w + 1):
        _, calls = run(longest)
        windows = [w if longest > w else 0, 0, w if longest > w else 0]
        assert [n for n, _ in calls[0::2]] == ["gmlm_rope_heads_d256_fwd"] * 3
        for (name, a), win in zip(calls[1::2], windows):
            if cap is not None:
                assert name == STEM + tail + "_fwd" and a["softcap"] == cap and type(a["window"]) is int and a["window"] == win
            elif win:
                assert name == BAND + tail + "_fwd" and a["window"] == win and "softcap" not in a
            else:
                assert name == PLAIN + tail + "_fwd" and "window" not in a and "softcap" not in a
            assert a["causal"] == 1 and a["d"] == 256 and a["hq"] == 3 and a["hkv"] == 1 and a["dropout_p"] == 0.0
            assert a["scale"] == 144 ** -0.5
        for _, a in calls[0::2]:
            assert a["heads"] == 4 and a["d"] == 256 and a["max_len"] >= longest
            assert (a["pos_ids"] is not None and a["seq_len"] == 0) if packed else (a["pos_ids"] is None and a["seq_len"] == longest)
    out, _ = run(w + 1, train=True)
    out.sum().backward()
    names = [n for n, _ in _calls(rec)]
    first = STEM if cap is not None else BAND
    mid = STEM if cap is not None else PLAIN
    assert names == [first + tail + "_bwd", "gmlm_rope_heads_d256_bwd", mid + tail + "_bwd", "gmlm_rope_heads_d256_bwd",
                     first + tail + "_bwd", "gmlm_rope_heads_d256_bwd"]


def test_one_rope_table_from_the_models_own_rotary_module():
    plm = _tiny()
    t = gemma2.rope_tables(plm, 40, "cpu")
    assert t.dtype == torch.float32 and t.shape[1:] == (2, 128) and t.shape[0] >= 40 and gemma2.rope_tables(plm, 33, "cpu") is t
    cos, sin = plm.rotary_emb(torch.zeros(1, 40, 8), torch.arange(40)[None])
    assert torch.equal(t[:40, 0], cos[0, :, :128]) and torch.equal(t[:40, 1], sin[0, :, :128])


# ------------------------------------------------------------------------------------------------- the autograd contract
def b_cap(dev="cpu", dt=torch.float32, hq=4, hkv=2, lens=(3, 2), packed=False, causal=True, window=2):
    g = _gen(41)
    shape = (sum(lens),) if packed else (len(lens), max(lens))
    inputs = dict(q=_r(g, *shape, hq * 256, dev=dev, dt=dt), k=_r(g, *shape, hkv * 256, dev=dev, dt=dt, s=1.5),
                  v=_r(g, *shape, hkv * 256, dev=dev, dt=dt))
    if packed:
        cu = _cu(lens, dev)
        return Case(inputs, lambda t: ops.gqa_d256_softcap_attention_varlen(t["q"], t["k"], t["v"], cu, max(lens), hq, hkv, 0.07, causal, 4.0,
                                                                            window))
    kl = torch.tensor(lens, dtype=torch.int32, device=dev)
    return Case(inputs, lambda t: ops.gqa_d256_softcap_attention(t["q"], t["k"], t["v"], kl, hq, hkv, 0.07, causal, 4.0, window))


def b_rope_cap(dev="cpu", dt=torch.float32, hq=2, hkv=1, lens=(3, 2), packed=False, causal=True, window=2, cap=4.0):
    g = _gen(42)
    shape = (sum(lens),) if packed else (len(lens), max(lens))
    inputs = dict(qkv=_r(g, *shape, (hq + 2 * hkv) * 256, dev=dev, dt=dt))
    cs = rope_table(max(lens) + 3, 128, dev)
    if packed:
        cu, pos = _cu(lens, dev), _pos(lens, dev)
        return Case(inputs, lambda t: ops.rope_softcap_gqa_d256_varlen(t["qkv"], cs, pos, cu, max(lens), hq, hkv, 0.07, causal, cap, window=window))
    kl = torch.tensor(lens, dtype=torch.int32, device=dev)
    return Case(inputs, lambda t: ops.rope_softcap_gqa_d256(t["qkv"], cs, kl, hq, hkv, 0.07, causal, cap, window=window))


NODES = {"SoftcapAttention256": b_cap, "RopeSoftcapGQA256": b_rope_cap}


def test_these_are_the_new_nodes():
    import inspect
    mine = {n for n, c in inspect.getmembers(ops_softcap, inspect.isclass)
            if issubclass(c, torch.autograd.Function) and c.__module__ == ops_softcap.__name__}
    assert mine == set(NODES)


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=("fp32", "bf16"))
@pytest.mark.parametrize("window", [0, 2], ids=("full", "band"))
@pytest.mark.parametrize("packed", [False, True], ids=("padded", "packed"))
@pytest.mark.parametrize("node", sorted(NODES))
def test_freeze_patterns_of_the_new_nodes(rec, node, packed, window, dt):
    case = NODES[node]("cpu", dt, packed=packed, window=window)
    failed = []
    for pattern in patterns(case.inputs):
        try:
            rec.take()
            leaves, outs = run_pattern(case, pattern)
            assert outs[0].grad_fn.name().startswith(node + "Backward")
            assert_contract(case, pattern, leaves)
            names = [n for n, _ in rec.take() if n.startswith("gmlm_attention") and not n.endswith("workspace_bytes")]
            tail = "_varlen" if packed else ""
            assert names == [STEM + tail + "_fwd", STEM + tail + "_bwd"], names
        except Exception as e:
            failed.append(f"trainable {pattern}: {type(e).__name__}: {e}")
    assert not failed, f"{node}: {len(failed)} patterns failed:\n  " + "\n  ".join(failed)


@pytest.mark.parametrize("window", [0, 2], ids=("full", "band"))
def test_no_cap_runs_the_existing_attention_entry_points_behind_the_same_rope(rec, window):
    case = b_rope_cap(window=window, cap=None)
    leaves = {n: v.clone().requires_grad_(True) for n, v in case.inputs.items()}
    out = case.call(leaves)
    assert out.grad_fn.name().startswith("RopeSoftcapGQA256Backward")
    names = [n for n, _ in rec.take() if not n.endswith("workspace_bytes")]
    assert names == ["gmlm_rope_heads_d256_fwd", (BAND if window else PLAIN) + "_fwd"]
    out.sum().backward()
    names = [n for n, _ in rec.take() if not n.endswith("workspace_bytes")]
    assert names == [(BAND if window else PLAIN) + "_bwd", "gmlm_rope_heads_d256_bwd"]
