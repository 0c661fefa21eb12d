"""Host side of the short-sequence grouped attention (no GPU needed): the eleventh header (include/gmlm_hip_gqa_short.h), its
ctypes table ``_lib.SIGNATURES_GQA_SHORT`` and the exported symbols agree type by type, the table sitting strictly inside
``SIGNATURE_TABLES_LATER`` and sharing no name with any other; the Makefile names the source and the headers; the two entry points
decide every documented refusal, in the documented order, and the nothing-to-do cases before any launch; the ops layer's one
dispatch rule (``ops._gqa_short_path``) sends 516 (sequence, head) pairs with ``groups`` to the new entry points and everything
else to the old ones with their argument lists unchanged; and the ``gqas::`` kernels of the built code objects are the sixteen
tests/test_gpu_gqa_short_kernels.py runs, none with a private segment (spill)."""
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
from test_attention_routes_cpu import SOME, STREAM, WS_BYTES, ptr, rec  # noqa: F401  (rec: the recording stub of the library)
from test_llama_cpu import _ids, no_device
from test_wgrad_cpu import LLVM, _code_objects

OK, EINVAL, ELAUNCH = 0, -1, -3
F32, BF16 = 0, 1
A = 0x10000000        # fabricated, non-null, 16-byte aligned: every call below ends before or at the launch
HEADER = os.path.join(ROOT, "include", "gmlm_hip_gqa_short.h")
FWD, BWD = "gmlm_attention_gqa_short_fwd", "gmlm_attention_gqa_short_bwd"
PROTOS = parse_header(open(HEADER).read())
for _h in ("gmlm_hip.h", "gmlm_hip_gqa.h", "gmlm_hip_bidir.h"):
    PROTOS.update(parse_header(open(os.path.join(ROOT, "include", _h)).read()))
_FWD = ("q k v cu_seqlens num_seqs max_len total_rows hq hkv d q_stride k_stride v_stride scale dropout_p causal seq_groups num_groups "
        "out lse dtype stream").split()
_BWD = ("q k v dout lse cu_seqlens num_seqs max_len total_rows hq hkv d q_stride k_stride v_stride scale dropout_p causal seq_groups "
        "num_groups dq dk dv dq_stride dk_stride dv_stride dtype stream").split()
_LISTS = {FWD: _FWD, BWD: _BWD}
_BASE = dict(q=A, k=A, v=A, cu_seqlens=A, num_seqs=9, max_len=64, total_rows=300, hq=6, hkv=2, d=64, q_stride=640, k_stride=640,
             v_stride=640, scale=0.125, dropout_p=0.0, causal=0, seq_groups=A, num_groups=3, out=A, lse=A, dtype=BF16, stream=None,
             dout=A, dq=A, dk=A, dv=A, dq_stride=640, dk_stride=640, dv_stride=640)


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libgmlm_hip.so not built")
    return _lib.lib()


# ------------------------------------------------------------------------------------------------------------------ ABI
def test_header_ctypes_table_and_exports_agree(lib):
    protos = parse_header(open(HEADER).read())
    assert sorted(protos) == [BWD, FWD]
    assert not signature_mismatches(protos, _lib.SIGNATURES_GQA_SHORT)
    table = _lib.SIGNATURES_GQA_SHORT
    for name in protos:
        assert hasattr(lib, name), f"{name} declared in include/gmlm_hip_gqa_short.h but not exported"
        assert getattr(lib, name).argtypes == table[name][1]                                  # lib() bound the new table
        assert [n for _, n in protos[name][1]] == _LISTS[name], name
    later = _lib.SIGNATURE_TABLES_LATER
    assert any(t is table for t in later[1:-1])                                               # strictly inside
    assert later[0] is not table and later[-1] is not table
    assert not any(t is table for t in _lib.SIGNATURE_TABLES)
    others = set().union(*(set(t) for t in _lib.SIGNATURE_TABLES + later if t is not table))
    assert not set(table) & others
    assert lib.gmlm_version() == 1
    text = open(HEADER).read()
    assert '#include "gmlm_hip.h"' in text and 'extern "C"' in text and "Conventions: those of gmlm_hip.h" in text


def test_the_makefile_names_the_new_source_and_headers():
    mk = open(os.path.join(ROOT, "gmlm_amd", "csrc", "Makefile")).read()
    srcs = re.search(r"^SRCS\s*=(.*)$", mk, re.M).group(1).split()
    assert "attn_gqa_short.hip" in srcs and os.path.exists(os.path.join(ROOT, "gmlm_amd", "csrc", "attn_gqa_short.hip"))
    deps = re.search(r"^\$\(BUILD\)/%\.o:(.*)$", mk, re.M).group(1).split()
    assert "../../include/gmlm_hip_gqa_short.h" in deps and "attn_short.hpp" in deps
    for src in ("attn_short.hip", "attn_gqa_short.hip"):                    # the shared helpers live in the header alone
        text = open(os.path.join(ROOT, "gmlm_amd", "csrc", src)).read()
        assert '#include "attn_short.hpp"' in text and "onehot_frag(int" not in text and "struct ShortMeta" not in text
    assert "attn_short_host.hpp" in deps
    for src in ("attn_short.hip", "attn_gqa_short.hip", "attn_d32_short.hip"):   # one launcher, one tile height: attn_short_host.hpp
        text = open(os.path.join(ROOT, "gmlm_amd", "csrc", src)).read()
        assert "hipFuncAttributeMaxDynamicSharedMemorySize" not in text and not re.search(r"\btile_rows\b", text), src


# ------------------------------------------------------------------------------------------------- entry-point refusals
def _call(lib, name, **mut):
    a = dict(_BASE, **mut)
    return getattr(lib, name)(*[a[n] for n in _LISTS[name]]), lib.gmlm_last_error()


# the documented order: each entry's mutation is refused with its message even when every LATER one is broken as well
_ORDER = [
    (dict(hq=0), b"bad sizes"),
    (dict(d=128), b"head dim"),
    (dict(dtype=F32), b"dtype"),
    (dict(hq=7), b"multiple of"),
    (dict(dropout_p=0.1), b"dropout"),
    (dict(scale=0.0), b"scale"),
    (dict(causal=2), b"causal"),
    (dict(cu_seqlens=None), b"cu_seqlens"),
    (dict(seq_groups=None), b"seq_groups"),
    (dict(num_groups=-1), b"num_groups"),
    (dict(max_len=129), b"max_len"),
    (dict(total_rows=1 << 30), b"packed rows"),
]
_MORE = [
    (dict(num_seqs=-1), b"bad sizes"), (dict(hkv=-1), b"bad sizes"), (dict(hkv=0), b"bad sizes"),
    (dict(d=32), b"head dim"), (dict(d=96), b"head dim"), (dict(dtype=2), b"dtype"), (dict(hkv=4), b"multiple of"),
    (dict(scale=-1.0), b"scale"), (dict(causal=-1), b"causal"), (dict(max_len=0), b"max_len"), (dict(max_len=-3), b"max_len"),
    (dict(total_rows=-1), b"packed rows"),
    (dict(num_groups=(1 << 31) // 6 + 1), b"too many work items"), (dict(num_groups=1 << 62), b"too many work items"),
    (dict(q_stride=376), b"stride"), (dict(k_stride=120), b"stride"), (dict(q_stride=644), b"stride"), (dict(v_stride=1 << 24), b"stride"),
    (dict(q=A + 8), b"aligned"), (dict(k=None), b"null"), (dict(v=None), b"null"),
]


@no_device
@pytest.mark.parametrize("name", [FWD, BWD])
@pytest.mark.parametrize("mut,msg", _ORDER + _MORE, ids=_ids(_ORDER + _MORE))
def test_refusals_are_decided_on_the_host(lib, name, mut, msg):
    rc, err = _call(lib, name, **mut)
    assert rc == EINVAL and msg in err and name[len("gmlm_"):].encode() in err, (mut, rc, err)


@no_device
@pytest.mark.parametrize("name", [FWD, BWD])
def test_refusals_come_in_the_documented_order(lib, name):
    for i, (mut, msg) in enumerate(_ORDER):
        broken = dict(mut)
        for later, _ in _ORDER[i + 1:]:
            broken.update({k: v for k, v in later.items() if k not in mut})
        rc, err = _call(lib, name, **broken)
        assert rc == EINVAL and msg in err, (i, broken, rc, err)
    # all of them before the work-item bound, and that before the operands
    rc, err = _call(lib, name, total_rows=1 << 30, num_groups=1 << 40)
    assert rc == EINVAL and b"packed rows" in err
    rc, err = _call(lib, name, num_groups=1 << 40, q=None)
    assert rc == EINVAL and b"too many work items" in err


@no_device
def test_outputs_and_gradient_operands(lib):
    for mut, msg in ((dict(out=None), b"out"), (dict(out=A + 4), b"out"), (dict(lse=None), b"lse")):
        rc, err = _call(lib, FWD, **mut)
        assert rc == EINVAL and msg in err, (mut, rc, err)
    for mut, msg in ((dict(dq=None), b"dq"), (dict(dk=A + 4), b"dk"), (dict(dv_stride=120), b"dv"), (dict(dq_stride=644), b"dq"),
                     (dict(dout=None), b"dout/lse"), (dict(dout=A + 2), b"dout/lse"), (dict(lse=None), b"dout/lse")):
        rc, err = _call(lib, BWD, **mut)
        assert rc == EINVAL and msg in err, (mut, rc, err)


@no_device
def test_valid_calls_reach_the_launch(lib):
    for name in (FWD, BWD):
        for mut in (dict(), dict(causal=1), dict(hq=7, hkv=1, q_stride=576, dq_stride=576), dict(hq=2, hkv=2), dict(max_len=1),
                    dict(max_len=128), dict(q_stride=384, k_stride=128, v_stride=128), dict(total_rows=1), dict(total_rows=(1 << 30) - 1),
                    dict(num_groups=(1 << 31) // 6 - 1), dict(num_groups=20, num_seqs=2)):
            rc, err = _call(lib, name, **mut)
            assert rc == ELAUNCH, (name, mut, rc, err)


@no_device
def test_nothing_to_do_needs_no_pointer_but_sizes_are_still_checked(lib):
    nothing = dict(q=None, k=None, v=None, out=None, lse=None, dout=None, dq=None, dk=None, dv=None)
    for name in (FWD, BWD):
        for empty in (dict(num_groups=0), dict(num_seqs=0), dict(total_rows=0)):
            assert _call(lib, name, **nothing, **empty)[0] == OK, (name, empty)
            for mut, msg in ((dict(d=96), b"head dim"), (dict(dropout_p=0.5), b"dropout"), (dict(hq=7), b"multiple of"),
                             (dict(dtype=F32), b"dtype"), (dict(causal=3), b"causal"), (dict(max_len=200), b"max_len"),
                             (dict(cu_seqlens=None), b"cu_seqlens"), (dict(seq_groups=None), b"seq_groups")):
                rc, err = _call(lib, name, **nothing, **empty, **mut)
                assert rc == EINVAL and msg in err, (name, empty, mut, rc, err)


# ------------------------------------------------------------------------------------------------------ the dispatch rule
def _named(call):
    name, args = call
    names = [n for _, n in PROTOS[name][1]]
    assert len(args) == len(names), f"{name}: {len(args)} arguments for {len(names)} parameters"
    return dict(zip(names, args))


def _route(rec, bidir, n_seq, hq, hkv, d, dtype, max_len, with_groups):
    """One forward + backward of the packed attention node on one-row sequences; -> (forward call, backward calls, tensors)."""
    nq, nk = hq * d, hkv * d
    qkv = torch.zeros(n_seq, nq + 2 * nk, dtype=dtype, requires_grad=True)
    q, k, v = qkv[:, :nq], qkv[:, nq:nq + nk], qkv[:, nq + nk:]
    cu = torch.arange(n_seq + 1, dtype=torch.int32)
    groups = ops.pack_sequence_groups([1] * n_seq) if with_groups else None
    fn = ops.bidir_gqa_attention_varlen if bidir else ops.causal_attention_varlen
    out = fn(q, k, v, cu, max_len, hq, hkv, 0.125, d, groups=groups)
    fwd, = rec.take()
    saved = out.grad_fn.saved_tensors
    gout = torch.ones_like(out)
    dqkv, = torch.autograd.grad(out, qkv, gout)
    return fwd, rec.take(), dict(qkv=qkv, cu=cu, groups=groups, out=out, gout=gout, saved=saved, w=nq + 2 * nk, nq=nq, nk=nk)


@pytest.mark.parametrize("bidir", [True, False], ids=["bidir", "causal"])
def test_516_pairs_with_groups_take_the_short_entry_points(rec, bidir):
    """Fails on the commit before the short-sequence grouped kernels: the wrappers take no ``groups``."""
    n_seq, hq, hkv = 86, 6, 2
    fwd, bwd, t = _route(rec, bidir, n_seq, hq, hkv, 64, torch.bfloat16, 128, True)
    qkv, w, nq, nk = t["qkv"], t["w"], t["nq"], t["nk"]
    assert t["groups"].dtype == torch.int32                                 # pack_sequence_groups output accepted as is
    saved = t["saved"]
    assert all(s is None or ptr(s) != ptr(t["out"]) for s in saved)         # the node saves neither out nor out_lo
    assert sum(s is None for s in saved) == 2
    a = _named(fwd)
    assert fwd[0] == FWD
    lse = next(s for s in saved if s is not None and s.dtype == torch.float32)
    assert tuple(lse.shape) == (hq, n_seq)
    want = dict(q=ptr(qkv), k=ptr(qkv, nq), v=ptr(qkv, nq + nk), cu_seqlens=ptr(t["cu"]), num_seqs=n_seq, max_len=128, total_rows=n_seq,
                hq=hq, hkv=hkv, d=64, q_stride=w, k_stride=w, v_stride=w, scale=0.125, dropout_p=0.0, causal=0 if bidir else 1,
                seq_groups=ptr(t["groups"]), num_groups=t["groups"].numel() - 1, out=ptr(t["out"]), lse=ptr(lse), dtype=_lib.BF16,
                stream=STREAM)
    assert a == want
    (name, args), = bwd                                                     # no workspace query, one launch
    assert name == BWD
    b = _named((name, args))
    for key in ("q", "k", "v", "cu_seqlens", "num_seqs", "max_len", "total_rows", "hq", "hkv", "d", "q_stride", "k_stride", "v_stride",
                "scale", "dropout_p", "causal", "seq_groups", "num_groups", "lse", "dtype", "stream"):
        assert b[key] == want[key], key
    assert b["dout"] == ptr(t["gout"]) and b["dq_stride"] == b["dk_stride"] == b["dv_stride"] == w
    assert b["dk"] - b["dq"] == 2 * nq and b["dv"] - b["dk"] == 2 * nk      # views of ONE dqkv (bf16: 2 bytes)


_OLD = [
    ("510_pairs", dict(n_seq=85)),
    ("no_groups", dict(with_groups=False)),
    ("fp32", dict(dtype=torch.float32)),
    ("max_len_129", dict(max_len=129)),
    ("d128", dict(d=128)),
]


@pytest.mark.parametrize("bidir", [True, False], ids=["bidir", "causal"])
@pytest.mark.parametrize("tag,kw", _OLD, ids=[t for t, _ in _OLD])
def test_everything_else_takes_the_streaming_entry_points_unchanged(rec, tag, kw, bidir):
    cfg = dict(n_seq=86, hq=6, hkv=2, d=64, dtype=torch.bfloat16, max_len=128, with_groups=True)
    cfg.update(kw)
    fwd, bwd, t = _route(rec, bidir, **cfg)
    n_seq, hq, hkv, d, dtype = cfg["n_seq"], cfg["hq"], cfg["hkv"], cfg["d"], cfg["dtype"]
    stem = "gmlm_attention_bidir_gqa" if bidir else f"gmlm_attention_causal_d{d}"
    qkv, w, nq, nk = t["qkv"], t["w"], t["nq"], t["nk"]
    saved = t["saved"]
    assert any(s is not None and ptr(s) == ptr(t["out"]) for s in saved)    # the streaming backward reads out
    bf = dtype == torch.bfloat16
    a = _named(fwd)
    assert fwd[0] == stem + "_varlen_fwd"
    want = dict(q=ptr(qkv), k=ptr(qkv, nq), v=ptr(qkv, nq + nk), cu_seqlens=ptr(t["cu"]), num_seqs=n_seq, max_len=cfg["max_len"],
                total_rows=n_seq, hq=hq, hkv=hkv, d=d, q_stride=w, k_stride=w, v_stride=w, scale=0.125, dropout_p=0.0, out=ptr(t["out"]),
                dtype=_lib.BF16 if bf else _lib.F32, stream=STREAM)
    assert {k: a[k] for k in want} == want and set(a) == set(want) | {"out_lo", "lse"}
    assert (a["out_lo"] is not None) == bf and a["lse"]
    ws, (name, args) = bwd
    assert ws == (stem + "_varlen_workspace_bytes", (n_seq, hq))
    b = _named((name, args))
    assert name == stem + "_varlen_bwd" and b["out"] == ptr(t["out"]) and b["out_lo"] == a["out_lo"] and b["workspace_bytes"] == WS_BYTES
    assert b["workspace"] and b["dout"] == ptr(t["gout"]) and b["lse"] == a["lse"]
    for key in ("q", "k", "v", "cu_seqlens", "num_seqs", "max_len", "total_rows", "hq", "hkv", "d", "q_stride", "k_stride", "v_stride",
                "scale", "dropout_p", "dtype", "stream"):
        assert b[key] == want[key], key
    assert "seq_groups" not in a and "seq_groups" not in b and "causal" not in a


def test_the_rule_is_written_once():
    assert ops._gqa_short_path(object(), torch.bfloat16, 64, 128, 86, 6)
    for args in ((None, torch.bfloat16, 64, 128, 86, 6), (object(), torch.float32, 64, 128, 86, 6), (object(), torch.bfloat16, 128, 128, 86, 6),
                 (object(), torch.bfloat16, 64, 129, 86, 6), (object(), torch.bfloat16, 64, 128, 85, 6)):
        assert not ops._gqa_short_path(*args), args
    src = open(os.path.join(ROOT, "gmlm_amd", "ops.py")).read()
    assert src.count("gmlm_attention_gqa_short_fwd") == 1 and src.count("gmlm_attention_gqa_short_bwd") == 1
    assert "not been measured" in ops._gqa_short_path.__doc__


def test_encoders_hand_groups_to_their_layer(monkeypatch):
    """llama_encode_packed / eurobert_encode_packed pass ``groups`` down to the attention node; the EuroBERT route with one KV head
    per query head at head dim 64 keeps its own attention family and sees no groups."""
    from gmlm_amd import eurobert, llama
    seen = []
    sentinel = torch.tensor([0, 1], dtype=torch.int32)

    def fake_node(qkv, cs, pos, cu, max_len, hq, hkv, d, scale, groups=None):
        seen.append(groups)
        return qkv[:, :hq * d]

    monkeypatch.setattr(ops, "rope_causal_gqa_varlen", fake_node)
    monkeypatch.setattr(ops, "rope_bidir_gqa_varlen", fake_node)
    monkeypatch.setattr(ops, "rope_attention_varlen", lambda qkv, cs, pos, cu, max_len, h, scale: seen.append("mha") or qkv[:, :h * 64])
    monkeypatch.setattr(ops, "add_rmsnorm", lambda a, b, w, eps: (a, a))
    monkeypatch.setattr(ops, "swiglu", lambda gu: gu[:, :gu.shape[1] // 2])
    for mod in (llama, eurobert):
        monkeypatch.setattr(mod, "_mm", lambda x, w, b, m: x.new_zeros(x.shape[0], w))
    lw = type("LW", (), dict(ln1=None, ln2=None, wqkv=(2 + 2) * 64, bqkv=None, m_qkv=(), wo=8, bo=None, m_wo=(), wgu=16, m_gu=(), wdown=8,
                             m_down=()))()
    x = torch.zeros(3, 8)
    for mod in (llama, eurobert):
        del seen[:]
        mod._layer(lw, x, None, None, None, 2, 1, 64, 0.125, 1e-6, (None, None, 3, sentinel))
        mod._layer(lw, x, None, None, None, 2, 1, 64, 0.125, 1e-6, (None, None, 3))
        assert seen[0] is sentinel and seen[1] is None, mod.__name__
    del seen[:]
    lw.wqkv = (2 + 4) * 64
    eurobert._layer(lw, x, None, None, None, 2, 2, 64, 0.125, 1e-6, (None, None, 3, sentinel))
    assert seen == ["mha"]


# --------------------------------------------------------------------------------------------------------- code objects
def test_gqas_kernels_are_the_ones_the_gpu_tests_run():
    from test_gpu_gqa_short_kernels import expected_kernels
    want = expected_kernels()
    got = _compiled_kernels(lambda name: name.startswith("gqas::"))
    assert len(want) == 16                                                 # (fwd, bwd) x (bidirectional, causal) x R in 32, 64, 96, 128
    assert got == want, (sorted(got - want), sorted(want - got))


def test_gqas_kernels_have_no_private_segment():
    """No spill (a zero private segment in every kernel's metadata) and no scratch traffic; all run on the matrix pipe."""
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libgmlm_hip.so not built")
    if not all(os.path.exists(os.path.join(LLVM, t)) for t in ("llvm-readelf", "llvm-objdump", "llvm-objcopy")):
        pytest.skip("ROCm llvm tools not found")
    tmp = tempfile.mkdtemp()
    try:
        private, bodies = {}, {}
        for co in _code_objects(_lib.LIB_PATH, tmp):
            notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", co], check=True, capture_output=True, text=True).stdout
            for m in re.finditer(r"\.name:\s+(_ZN4gmlm4gqas\w+)\s+\.private_segment_fixed_size:\s+(\d+)", notes):
                private[m.group(1)] = int(m.group(2))
            dis = subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-d", "--mcpu=gfx950", co], check=True, capture_output=True,
                                 text=True).stdout
            for m in re.finditer(r"^[0-9a-f]+ <(_ZN4gmlm4gqas\w+)>:\n(.*?)(?=^[0-9a-f]+ <|\Z)", dis, re.S | re.M):
                bodies[m.group(1)] = m.group(2)
        assert len(private) == 16 and set(private) == set(bodies), (sorted(private), sorted(bodies))
        assert not {n: v for n, v in private.items() if v}, private
        for name, body in bodies.items():
            assert "v_mfma" in body, name
            assert not re.search(r"v_pk_\w+_f32", body), name
            assert "scratch_" not in body, name
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
