"""Host side of the short-sequence attention at head dim 32 (no GPU needed): the twelfth header (include/gmlm_hip_d32_short.h),
its ctypes table ``_lib.SIGNATURES_D32_SHORT`` and the exported symbols agree type by type; the Makefile names the source and the
header; the two entry points decide every documented refusal on the host, naming the argument, and the nothing-to-do cases before
any launch; the ops layer's one rule (``ops._d32_short_path``) sends a bf16 d = 32 call with ``groups`` and >= 96 pairs to the new
entry points (no out_lo, fused bias sums) and everything else to ``gmlm_attention_d32_*`` with today's arguments; ``GraphTextLM``
builds ``groups`` at head dim 32 where it builds them at 64; and the ``d32s::`` kernels of the built code objects are the sixteen
tests/test_gpu_d32_short_kernels.py runs, none with a private segment or packed-fp32 VALU code.

On the commit before these kernels the header, the table and the rule do not exist (this module does not import), the entry
points are not exported (the signature and refusal tests), ``AttentionQKV`` drops ``groups`` at head dim 32 (the routing tests)
and ``GraphTextLM`` builds no groups at head dim 32 (the two model tests)."""
import os
import re
import shutil
import subprocess
import tempfile

import pytest
import torch

from conftest import ROOT
from gmlm_amd import _lib, ops
from test_abi_contract_cpu import parse_header, signature_mismatches
from test_attention_matrix_cpu import _compiled_kernels
from test_attention_routes_cpu import STREAM, WS_BYTES, ptr, rec  # noqa: F401  (rec: the recording stub of the library)
from test_llama_cpu import _ids, no_device
from test_wgrad_cpu import LLVM, _code_objects

OK, EINVAL, ELAUNCH = 0, -1, -3
F32, BF16 = 0, 1
A = 0x10000000        # fabricated, non-null, 16-byte aligned: every call below ends before or at the launch
HEADER = os.path.join(ROOT, "include", "gmlm_hip_d32_short.h")
FWD, BWD = "gmlm_attention_d32_short_fwd", "gmlm_attention_d32_short_bwd"
PROTOS = parse_header(open(HEADER).read())
PROTOS.update(parse_header(open(os.path.join(ROOT, "include", "gmlm_hip_d32.h")).read()))
_FWD = ("q k v cu_seqlens num_seqs max_len total_rows h d q_stride k_stride v_stride scale dropout_p seed seed_dev seq_groups num_groups "
        "out lse dtype stream").split()
_BWD = ("q k v dout lse cu_seqlens num_seqs max_len total_rows h d q_stride k_stride v_stride scale dropout_p seed seed_dev seq_groups "
        "num_groups dq dk dv dq_stride dk_stride dv_stride dbias_partial dbias dtype stream").split()
_LISTS = {FWD: _FWD, BWD: _BWD}
_BASE = dict(q=A, k=A, v=A, cu_seqlens=A, num_seqs=9, max_len=64, total_rows=300, h=12, d=32, q_stride=1152, k_stride=1152,
             v_stride=1152, scale=0.125, dropout_p=0.0, seed=5, seed_dev=None, seq_groups=A, num_groups=3, out=A, lse=A, dtype=BF16,
             stream=None, dout=A, dq=A, dk=A, dv=A, dq_stride=1152, dk_stride=1152, dv_stride=1152, dbias_partial=None, dbias=None)


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libgmlm_hip.so not built")
    return _lib.lib()


# ------------------------------------------------------------------------------------------------------------------ ABI
def test_header_ctypes_table_and_exports_agree(lib):
    """Fails on the commit before these kernels: no such header, table or exported symbol."""
    protos = parse_header(open(HEADER).read())
    assert sorted(protos) == [BWD, FWD]
    assert not signature_mismatches(protos, _lib.SIGNATURES_D32_SHORT)
    table = _lib.SIGNATURES_D32_SHORT
    for name in protos:
        assert hasattr(lib, name), f"{name} declared in include/gmlm_hip_d32_short.h but not exported"
        assert getattr(lib, name).argtypes == table[name][1]                                  # lib() bound the new table
        assert [n for _, n in protos[name][1]] == _LISTS[name], name
    assert any(t is table for t in _lib.SIGNATURE_TABLES_LATER) and not any(t is table for t in _lib.SIGNATURE_TABLES)
    others = set().union(*(set(t) for t in _lib.SIGNATURE_TABLES + _lib.SIGNATURE_TABLES_LATER if t is not table))
    assert not set(table) & others
    assert lib.gmlm_version() == 1
    text = open(HEADER).read()
    assert '#include "gmlm_hip.h"' in text and 'extern "C"' in text and "Conventions: those of gmlm_hip.h" in text
    assert "h must be EVEN" in text                            # what the entry points do with an odd h is stated
    assert "gmlm_hip_d32_short.h" in open(os.path.join(ROOT, "include", "gmlm_hip_d32.h")).read()


def test_the_makefile_names_the_new_source_and_header():
    mk = open(os.path.join(ROOT, "gmlm_amd", "csrc", "Makefile")).read()
    srcs = re.search(r"^SRCS\s*=(.*)$", mk, re.M).group(1).split()
    assert "attn_d32_short.hip" in srcs and os.path.exists(os.path.join(ROOT, "gmlm_amd", "csrc", "attn_d32_short.hip"))
    deps = re.search(r"^\$\(BUILD\)/%\.o:(.*)$", mk, re.M).group(1).split()
    assert "../../include/gmlm_hip_d32_short.h" in deps and "attn_short.hpp" in deps
    assert "-fno-slp-vectorize" in re.search(r"^CXXFLAGS\s*=(.*)$", mk, re.M).group(1)         # every file, this one included
    text = open(os.path.join(ROOT, "gmlm_amd", "csrc", "attn_d32_short.hip")).read()
    assert '#include "attn_short.hpp"' in text and "onehot_frag(int" not in text and "struct ShortMeta" not in text
    assert text.count("__global__") == 2 and "namespace d32s" in text
    # the launcher, the tile height and the meta carving are the shared ones (attn_short_host.hpp, ShortMeta::carve)
    assert "attn_short_host.hpp" in deps and "hipFuncAttributeMaxDynamicSharedMemorySize" not in text
    assert not re.search(r"\btile_rows\b", text) and "meta_carve" not in text


# ------------------------------------------------------------------------------------------------- entry-point refusals
def _call(lib, name, **mut):
    a = dict(_BASE, **mut)
    return getattr(lib, name)(*[a[n] for n in _LISTS[name]]), lib.gmlm_last_error()


# every refusal the header lists, with the argument its message names
_REFUSED = [
    (dict(h=0), b"bad sizes"), (dict(num_seqs=-1), b"bad sizes"),
    (dict(d=64), b"head dim d = 64"), (dict(d=16), b"head dim d"),
    (dict(dtype=F32), b"dtype"), (dict(dtype=2), b"dtype"),
    (dict(h=3, q_stride=288, k_stride=288, v_stride=288), b"h = 3"),
    (dict(dropout_p=1.0), b"dropout_p"), (dict(dropout_p=-0.1), b"dropout_p"),
    (dict(scale=0.0), b"scale"), (dict(scale=-1.0), b"scale"),
    (dict(cu_seqlens=None), b"cu_seqlens"),
    (dict(seq_groups=None), b"seq_groups"),
    (dict(num_groups=-1), b"num_groups"),
    (dict(max_len=129), b"max_len"), (dict(max_len=0), b"max_len"), (dict(max_len=-3), b"max_len"),
    (dict(total_rows=-1), b"total_rows"), (dict(total_rows=1 << 30), b"total_rows"),
    (dict(num_groups=0), b"num_groups"),                                    # rows present, no group
    (dict(num_seqs=40), b"seq_groups"),                                     # 40 sequences in 3 groups: one holds more than 13
    (dict(total_rows=385), b"seq_groups"),                                  # 385 rows in 3 groups: one holds more than 128
    (dict(num_groups=(1 << 31) // 12 + 1), b"too many work items"),
    (dict(q_stride=376), b"(q)"), (dict(k_stride=120), b"(k)"), (dict(q_stride=1156), b"(q)"), (dict(v_stride=1 << 24), b"(v)"),
    (dict(q=A + 8), b"aligned"), (dict(k=None), b"(k)"), (dict(v=None), b"(v)"),
]


@no_device
@pytest.mark.parametrize("name", [FWD, BWD])
@pytest.mark.parametrize("mut,msg", _REFUSED, ids=_ids(_REFUSED))
def test_refusals_are_decided_on_the_host(lib, name, mut, msg):
    """Fails on the commit before these kernels: the entry points do not exist."""
    rc, err = _call(lib, name, **mut)
    assert rc == EINVAL and msg in err and name[len("gmlm_"):].encode() in err, (mut, rc, err)


@no_device
def test_outputs_gradient_operands_and_bias_sums(lib):
    for mut, msg in ((dict(out=None), b"out"), (dict(out=A + 4), b"out"), (dict(lse=None), b"lse")):
        rc, err = _call(lib, FWD, **mut)
        assert rc == EINVAL and msg in err, (mut, rc, err)
    for mut, msg in ((dict(dq=None), b"dq"), (dict(dk=A + 4), b"dk"), (dict(dv_stride=120), b"dv"), (dict(dq_stride=1156), b"dq"),
                     (dict(dout=None), b"dout/lse"), (dict(dout=A + 2), b"dout/lse"), (dict(lse=None), b"dout/lse"),
                     (dict(dbias=A), b"dbias_partial"), (dict(dbias_partial=A), b"dbias")):
        rc, err = _call(lib, BWD, **mut)
        assert rc == EINVAL and msg in err, (mut, rc, err)


@no_device
def test_valid_calls_reach_the_launch(lib):
    for name in (FWD, BWD):
        for mut in (dict(), dict(h=2, q_stride=64, k_stride=64, v_stride=64), dict(max_len=1), dict(max_len=128), dict(dropout_p=0.5),
                    dict(seed_dev=A), dict(total_rows=1), dict(total_rows=384), dict(num_seqs=39), dict(num_groups=20, num_seqs=2)):
            rc, err = _call(lib, name, **mut)
            assert rc == ELAUNCH, (name, mut, rc, err)
    rc, err = _call(lib, BWD, dbias=A, dbias_partial=A)
    assert rc == ELAUNCH, (rc, err)


@no_device
def test_nothing_to_do_needs_no_data_pointer_but_sizes_are_still_checked(lib):
    nothing = dict(q=None, k=None, v=None, out=None, lse=None, dout=None, dq=None, dk=None, dv=None)
    for name in (FWD, BWD):
        for empty in (dict(num_groups=0, total_rows=0), dict(num_groups=0, num_seqs=0), dict(num_seqs=0), dict(total_rows=0)):
            assert _call(lib, name, **nothing, **empty)[0] == OK, (name, empty)
            for mut, msg in ((dict(d=64), b"head dim"), (dict(dropout_p=1.5), b"dropout_p"), (dict(h=5), b"h = 5"),
                             (dict(dtype=F32), b"dtype"), (dict(max_len=200), b"max_len"), (dict(cu_seqlens=None), b"cu_seqlens"),
                             (dict(seq_groups=None), b"seq_groups"), (dict(scale=0.0), b"scale")):
                rc, err = _call(lib, name, **nothing, **empty, **mut)
                assert rc == EINVAL and msg in err, (name, empty, mut, rc, err)
    rc, err = _call(lib, BWD, **nothing, total_rows=0, dbias=A)
    assert rc == EINVAL and b"dbias" in err


def test_the_streaming_family_keeps_its_refusal_of_groups():
    """gmlm_attention_d32_* has no seq_groups argument; the ops family table still says so."""
    assert not ops._ATTN_D32.short and ops._ATTN_D32.packed


# ------------------------------------------------------------------------------------------------------ the dispatch rule
def test_the_rule_truth_table():
    """Fails on the commit before these kernels: ``ops._d32_short_path`` does not exist."""
    g = object()
    assert ops.D32_SHORT_MIN_PAIRS == 96                       # the smallest count measured
    assert ops._d32_short_path(g, torch.bfloat16, 32, 128, 43, 12)
    for args in ((None, torch.bfloat16, 32, 128, 43, 12),              # no groups
                 (g, torch.float32, 32, 128, 43, 12),                  # fp32
                 (g, torch.float16, 32, 128, 43, 12),
                 (g, torch.bfloat16, 64, 128, 43, 12),                 # another head dim
                 (g, torch.bfloat16, 16, 128, 43, 12),
                 (g, torch.bfloat16, 32, 129, 43, 12),                 # a sequence longer than a tile
                 (g, torch.bfloat16, 32, 128, 7, 12),                  # 84 pairs
                 (g, torch.bfloat16, 32, 128, 171, 3)):                # an odd head count (513 pairs)
        assert not ops._d32_short_path(*args), args
    assert ops._d32_short_path(g, torch.bfloat16, 32, 1, 48, 2) and ops._d32_short_path(g, torch.bfloat16, 32, 128, 8, 12)
    src = open(os.path.join(ROOT, "gmlm_amd", "ops.py")).read()
    assert src.count('"gmlm_attention_d32_short_fwd"') == 1 and src.count('"gmlm_attention_d32_short_bwd"') == 1
    assert "even" in ops._d32_short_path.__doc__


def _named(call):
    name, args = call
    names = [n for _, n in PROTOS[name][1]]
    assert len(args) == len(names), f"{name}: {len(args)} arguments for {len(names)} parameters"
    return dict(zip(names, args))


def _route(rec, n_seq=43, h=12, d=32, dtype=torch.bfloat16, max_len=128, with_groups=True, p=0.0, masters=True):
    hd = h * d
    qkv = torch.zeros(n_seq, 3 * hd, dtype=dtype, requires_grad=True)
    cu = torch.arange(n_seq + 1, dtype=torch.int32)
    groups = ops.pack_sequence_groups([1] * n_seq) if with_groups else None
    bias = tuple(torch.zeros(hd, requires_grad=True) for _ in range(3)) if masters else ()
    out = ops.AttentionQKV.apply(qkv, None, h, 0.25, p, 77, cu, max_len, None, groups, *bias)
    fwd, = rec.take()
    saved = out.grad_fn.saved_tensors
    gout = torch.ones_like(out)
    grads = torch.autograd.grad(out, (qkv,) + bias, gout, allow_unused=True)
    return fwd, rec.take(), dict(qkv=qkv, cu=cu, groups=groups, out=out, gout=gout, saved=saved, grads=grads, hd=hd)


@pytest.mark.parametrize("p", [0.0, 0.1])
def test_516_pairs_with_groups_take_the_short_entry_points(rec, p):
    """Fails on the commit before these kernels: ``groups`` is dropped at head dim 32 and gmlm_attention_d32_* is called."""
    n_seq, h = 43, 12
    fwd, bwd, t = _route(rec, p=p)
    qkv, hd, w = t["qkv"], t["hd"], 3 * t["hd"]
    saved = [s for s in t["saved"] if s is not None]
    assert not any(ptr(s) == ptr(t["out"]) for s in saved)                  # the node saves neither out nor out_lo
    assert sorted(str(s.dtype) for s in saved) == ["torch.bfloat16", "torch.float32", "torch.int32", "torch.int32"]      # qkv, lse, cu, groups
    lse = next(s for s in saved if s.dtype == torch.float32)
    assert tuple(lse.shape) == (h, n_seq)
    assert fwd[0] == FWD
    want = dict(q=ptr(qkv), k=ptr(qkv, hd), v=ptr(qkv, 2 * hd), cu_seqlens=ptr(t["cu"]), num_seqs=n_seq, max_len=128, total_rows=n_seq,
                h=h, d=32, q_stride=w, k_stride=w, v_stride=w, scale=0.25, dropout_p=p, seed=77, seed_dev=None,
                seq_groups=ptr(t["groups"]), num_groups=t["groups"].numel() - 1, out=ptr(t["out"]), lse=ptr(lse), dtype=_lib.BF16,
                stream=STREAM)
    assert _named(fwd) == want
    (name, args), = bwd                                                     # no workspace query, one call, no column_sum
    assert name == BWD
    b = _named((name, args))
    for key in ("q", "k", "v", "cu_seqlens", "num_seqs", "max_len", "total_rows", "h", "d", "q_stride", "k_stride", "v_stride", "scale",
                "dropout_p", "seed", "seed_dev", "seq_groups", "num_groups", "lse", "dtype", "stream"):
        assert b[key] == want[key], key
    assert b["dout"] == ptr(t["gout"]) and b["dq_stride"] == b["dk_stride"] == b["dv_stride"] == w
    assert b["dk"] - b["dq"] == 2 * hd and b["dv"] - b["dk"] == 2 * hd      # views of ONE dqkv (bf16: 2 bytes)
    assert b["dbias_partial"] and b["dbias"]                                # the fused bias sums are requested
    assert all(g is not None and tuple(g.shape) == (hd,) for g in t["grads"][1:])
    # without bias masters nothing is requested
    _, bwd2, _ = _route(rec, p=p, masters=False)
    (name2, args2), = bwd2
    b2 = _named((name2, args2))
    assert name2 == BWD and b2["dbias_partial"] is None and b2["dbias"] is None


_OLD = [
    ("84_pairs", dict(n_seq=7)),
    ("no_groups", dict(with_groups=False)),
    ("fp32", dict(dtype=torch.float32)),
    ("max_len_129", dict(max_len=129)),
    ("odd_heads", dict(n_seq=171, h=3)),
]


@pytest.mark.parametrize("tag,kw", _OLD, ids=[t for t, _ in _OLD])
def test_everything_else_takes_the_streaming_entry_points_unchanged(rec, tag, kw):
    cfg = dict(n_seq=43, h=12, dtype=torch.bfloat16, max_len=128, with_groups=True)
    cfg.update(kw)
    fwd, bwd, t = _route(rec, masters=False, **cfg)
    n_seq, h, dtype = cfg["n_seq"], cfg["h"], cfg["dtype"]
    qkv, hd, w = t["qkv"], t["hd"], 3 * t["hd"]
    bf = dtype == torch.bfloat16
    assert any(s is not None and ptr(s) == ptr(t["out"]) for s in t["saved"])        # the streaming backward reads out
    assert fwd[0] == "gmlm_attention_d32_fwd"
    a = _named(fwd)
    want = dict(q=ptr(qkv), k=ptr(qkv, hd), v=ptr(qkv, 2 * hd), kv_len=None, b=n_seq, h=h, lq=n_seq, lk=n_seq, d=32, q_stride=w,
                k_stride=w, v_stride=w, scale=0.25, dropout_p=0.0, seed=77, seed_dev=None, out=ptr(t["out"]),
                dtype=_lib.BF16 if bf else _lib.F32, cu_seqlens=ptr(t["cu"]), max_len=cfg["max_len"], stream=STREAM)
    assert {k: a[k] for k in want} == want and set(a) == set(want) | {"out_lo", "lse"}
    assert (a["out_lo"] is not None) == bf and a["lse"]
    ws, (name, args) = bwd
    assert ws == ("gmlm_attention_d32_bwd_workspace_bytes", (1, h, n_seq))
    b = _named((name, args))
    assert name == "gmlm_attention_d32_bwd" and b["out"] == ptr(t["out"]) and b["out_lo"] == a["out_lo"] and b["workspace_bytes"] == WS_BYTES
    assert "seq_groups" not in a and "seq_groups" not in b and "dbias" not in b


# --------------------------------------------------------------------------------------------------------- GraphTextLM
def _model(hidden, heads, cd):
    import gmlm_amd
    from transformers import BertConfig, BertModel
    plm = BertModel(BertConfig(vocab_size=50, hidden_size=hidden, num_hidden_layers=1, num_attention_heads=heads, intermediate_size=2 * hidden,
                               max_position_embeddings=160, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0))
    return gmlm_amd.GraphTextLM(8, 8, 3, dropout_rate=0.0, plm_encoder=plm, plm_max_length=160, compute_dtype=cd)


def _tokens(n, longest):
    import gmlm_amd
    lens = torch.tensor([longest] + [1 + i % 7 for i in range(n - 1)])
    am = (torch.arange(longest)[None, :] < lens[:, None]).long()
    return gmlm_amd.TokenizedTexts.from_mask(am.clone(), am)


# (hidden, heads, compute dtype, sequences, longest) -> groups built
_MODEL_CASES = [
    ("d32", (384, 12, torch.bfloat16, 60, 40), True),
    ("d64", (128, 2, torch.bfloat16, 300, 40), True),
    ("d32_fp32", (384, 12, torch.float32, 60, 40), False),
    ("d32_long", (384, 12, torch.bfloat16, 60, 129), False),
    ("d32_few_pairs", (64, 2, torch.bfloat16, 8, 40), False),
    ("d96", (192, 2, torch.bfloat16, 300, 40), False),
]


@pytest.mark.parametrize("tag,geo,want", _MODEL_CASES, ids=[t for t, _, _ in _MODEL_CASES])
def test_bucket_tables_build_groups_at_head_dim_32_as_at_64(tag, geo, want):
    """Host only.  Fails on the commit before these kernels at ``d32``: no groups at head dim 32."""
    hidden, heads, cd, n, longest = geo
    m = _model(hidden, heads, cd)
    tokens = _tokens(n, longest)
    seen = dict(bucket=None, idx_h=torch.arange(n), mask_h=torch.ones(n, dtype=torch.bool))
    key, args, short = m._bucket_tables(tokens, seen, cd)
    assert short == want and len(args) == (4 if want else 3) and (key[3] > 0) == want
    if want:
        groups = args[3].tolist()
        lens_all = args[0].tolist()
        assert groups[0] == 0 and groups[-1] == len(lens_all)
        for g0, g1 in zip(groups[:-1], groups[1:]):
            assert g1 - g0 <= 13 and sum(lens_all[g0:g1]) <= 128


@pytest.mark.parametrize("tag,geo,want", _MODEL_CASES, ids=[t for t, _, _ in _MODEL_CASES])
def test_eager_packed_micro_batch_builds_groups_at_head_dim_32_as_at_64(monkeypatch, tag, geo, want):
    """Host only, with a stub encoder.  Fails on the commit before these kernels at ``d32``."""
    from gmlm_amd import bert
    hidden, heads, cd, n, longest = geo
    m = _model(hidden, heads, cd).train()
    tokens = _tokens(n, longest)
    seen = []

    def stub(plm, tok, pos, cu, max_len, cd_, training, ckpt, weights, pair_count=None, groups=None):
        seen.append((groups, cu))
        return torch.zeros(tok.numel(), hidden)

    monkeypatch.setattr(bert, "bert_encode_packed", stub)
    monkeypatch.setattr(ops.MeanPoolScatter, "apply", staticmethod(lambda emb, hs, lens, bi, *a: emb))
    m.encode_texts(tokens, torch.ones(n, dtype=torch.bool), plm_batch_size=512, _weights=object())
    (groups, cu), = seen
    assert (groups is not None) == want
    if want:
        assert groups.dtype == torch.int32 and int(groups[0]) == 0 and int(groups[-1]) == cu.numel() - 1
    # the zero-padded route of a head dim outside the native set takes no packed pass at all
    if tag == "d32":
        monkeypatch.setattr(bert, "NATIVE_HEAD_DIMS", (64, 96))
        assert not m._has_packed_pass()


# --------------------------------------------------------------------------------------------------------- code objects
def test_d32s_kernels_are_the_ones_the_gpu_tests_run():
    from test_gpu_d32_short_kernels import expected_kernels
    want = expected_kernels()
    got = _compiled_kernels(lambda name: name.startswith("d32s::"))
    assert len(want) == 16                                     # (fwd, bwd) x (plain, dropout) x R in 32, 64, 96, 128
    assert got == want, (sorted(got - want), sorted(want - got))


def test_d32s_kernels_have_no_private_segment_and_no_packed_fp32():
    """No spill (a zero private segment in every kernel's metadata), no scratch traffic, no v_pk_*_f32; all run on the matrix pipe."""
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libgmlm_hip.so not built")
    if not all(os.path.exists(os.path.join(LLVM, t)) for t in ("llvm-readelf", "llvm-objdump", "llvm-objcopy")):
        pytest.skip("ROCm llvm tools not found")
    tmp = tempfile.mkdtemp()
    try:
        private, bodies = {}, {}
        for co in _code_objects(_lib.LIB_PATH, tmp):
            notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", co], check=True, capture_output=True, text=True).stdout
            for m in re.finditer(r"\.name:\s+(_ZN4gmlm4d32s\w+)\s+\.private_segment_fixed_size:\s+(\d+)", notes):
                private[m.group(1)] = int(m.group(2))
            dis = subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-d", "--mcpu=gfx950", co], check=True, capture_output=True,
                                 text=True).stdout
            for m in re.finditer(r"^[0-9a-f]+ <(_ZN4gmlm4d32s\w+)>:\n(.*?)(?=^[0-9a-f]+ <|\Z)", dis, re.S | re.M):
                bodies[m.group(1)] = m.group(2)
        assert len(private) == 16 and set(private) == set(bodies), (sorted(private), sorted(bodies))
        assert not {n: v for n, v in private.items() if v}, private
        for name, body in bodies.items():
            assert "v_mfma" in body, name
            assert not re.search(r"v_pk_\w+_f32", body), name
            assert "scratch_" not in body, name
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
