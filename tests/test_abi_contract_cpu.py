"""The argument contract of include/gmlm_hip.h, entry point by entry point, decided on the host.

One table (ROWS) has a row for every launching `int gmlm_*` function the header declares.  A row gives one valid call built from
fabricated addresses, the class of each pointer (required / nullable / required under a condition) and the refusals the header
promises.  Without a device a call that passes validation ends in GMLM_ELAUNCH (-3, "no ROCm-capable device"), a refused one
in GMLM_EINVAL (-1) or GMLM_EWORKSPACE (-2), and a call with nothing to do in GMLM_OK: the return code shows exactly which
check decided.  With a device a missed check would launch on the fabricated addresses, so the module skips itself there.

The ctypes signatures of gmlm_amd/_lib.py are compared with the parsed prototypes type by type as well."""
import ctypes as C
import os
import re

import pytest
import torch

from conftest import ROOT

pytestmark = pytest.mark.skipif(torch.cuda.device_count() > 0,
                                reason="fabricated addresses: only meaningful (and only safe) without a device")

OK, EINVAL, EWORKSPACE, ELAUNCH = 0, -1, -2, -3
F32, BF16 = 0, 1
HOST_ONLY = {"gmlm_version", "gmlm_device_check", "gmlm_split_plan_capacity"}     # return int, never launch
ALWAYS_NULLABLE = {"stream", "seed_dev"}                                          # stated once in the header's conventions


# ------------------------------------------------------------------------------------------------------- header parsing
def parse_header(text=None):
    """{name: (return type, [(type, name), ...])} of every gmlm_* prototype, comments and preprocessor lines stripped."""
    if text is None:
        text = open(os.path.join(ROOT, "include", "gmlm_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    text = "\n".join(l for l in text.splitlines() if not l.lstrip().startswith("#"))
    protos = {}
    for ret, name, params in re.findall(r"([A-Za-z_][\w\s\*]*?)\b(gmlm_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", text):
        ret = " ".join(ret.replace("*", " * ").split())
        plist = []
        if params.strip() not in ("", "void"):
            for prm in params.split(","):
                m = re.fullmatch(r"\s*(.*?)([A-Za-z_]\w*)\s*", prm, flags=re.S)
                plist.append((" ".join(m.group(1).replace("*", " * ").split()), m.group(2)))
        protos[name] = (ret, plist)
    return protos


def is_pointer(ctype):
    return "*" in ctype or ctype == "gmlm_stream_t"


_SCALARS = {"int64_t": C.c_int64, "int": C.c_int, "float": C.c_float, "uint64_t": C.c_uint64, "size_t": C.c_size_t}


def _is_ctypes_pointer(t):
    return t in (C.c_void_p, C.c_char_p) or (isinstance(t, type) and issubclass(t, C._Pointer))


def _type_matches(ctype, t):
    return _is_ctypes_pointer(t) if is_pointer(ctype) else _SCALARS.get(ctype) is t


def signature_mismatches(protos, signatures):
    """Every disagreement between the parsed prototypes and a SIGNATURES-style dict, as readable strings."""
    bad = [f"{n}: only in the header" for n in protos if n not in signatures]
    bad += [f"{n}: only in SIGNATURES" for n in signatures if n not in protos]
    for name, (ret, params) in protos.items():
        if name not in signatures:
            continue
        res, args = signatures[name]
        if not _type_matches(ret, res):
            bad.append(f"{name}: returns {ret}, bound as {res}")
        if len(args) != len(params):
            bad.append(f"{name}: {len(params)} parameters in the header, {len(args)} in SIGNATURES")
            continue
        bad += [f"{name}: parameter {i} `{ct} {pn}` bound as {t}" for i, ((ct, pn), t) in enumerate(zip(params, args))
                if not _type_matches(ct, t)]
    return bad


PROTOS = parse_header()


# ------------------------------------------------------------------------------------------------------------ the table
def ADDR(i):
    """Fabricated, distinct, 16-byte aligned, non-null: never dereferenced, every call here ends before or at the launch."""
    return 0x10000000 + 0x1000000 * i


class Off:
    """Mutation value: the baseline address of this pointer moved by `n` bytes."""
    def __init__(self, n):
        self.n = n

    def __repr__(self):
        return f"+{self.n}B"


def nul(names, rc, msg=None, **mut):
    """One case per name: that pointer NULL (plus `mut`), expected code and message."""
    return [(dict(mut, **{n: None}), rc, msg) for n in names.split()]


def each(key, values, rc, msg=None, **mut):
    return [(dict({key: v}, **mut), rc, msg) for v in values]


DROPOUT = each("dropout_p", (-0.1, 1.0), EINVAL, b"[0,1)") + each("dropout_p", (0.5,), ELAUNCH)
DTYPE = each("dtype", (2, -1), EINVAL, b"dtype")

ROWS = {}


def row(name, base, ptr, *, null_at_base=(), fixed=None, null_msg=None, align=None, align_msg=None, accepts_misaligned=(),
        cases=(), ws=None, empty=()):
    """base: non-pointer arguments of the valid call.  ptr: class of every pointer ('req' | 'null' | 'cond').
    null_at_base: pointers that are NULL in the valid call.  fixed: explicit baseline addresses (two pointers into one buffer).
    align: pointers under the 16-byte rule.  accepts_misaligned: pointers the header calls scalar (a 2- / 4-byte shift passes).
    cases: (mutation, code, message substring).  ws: (companion, its argument names, mutation under which the workspace is
    needed).  empty: (mutation, pointers kept, code): every other pointer NULL."""
    assert name not in ROWS
    ROWS[name] = dict(base=base, ptr=ptr, null_at_base=set(null_at_base), fixed=fixed or {}, null_msg=null_msg,
                      align=(align or "").split(), align_msg=align_msg, accepts_misaligned=list(accepts_misaligned),
                      cases=list(cases), ws=ws, empty=list(empty))


# ---- K1 graph preprocessing
for _n in ("gmlm_degree_i32", "gmlm_degree_f32"):
    row(_n, dict(e=1, n=1), dict(index="cond", deg="cond"),
        cases=nul("index deg", EINVAL, b"bad arguments") + nul("index", ELAUNCH, e=0) + [(dict(deg=None, index=None, e=0, n=0), OK, None)]
        + each("n", (-1,), EINVAL, b"bad arguments") + each("e", (-1,), EINVAL, b"bad arguments")
        + each("n", (1 << 31,), EINVAL, b"int32 range") + each("n", ((1 << 31) - 1,), ELAUNCH),
        empty=[(dict(e=0, n=0), (), OK), (dict(e=0), ("deg",), ELAUNCH)])
row("gmlm_edge_bucket", dict(e=1, n=1), dict(src="cond", deg="cond", edge_type="cond"),
    cases=nul("src deg edge_type", EINVAL, b"bad arguments") + nul("src deg edge_type", OK, e=0) + each("e", (-1,), EINVAL, b"bad arguments")
    + each("n", (-1,), EINVAL, b"bad arguments"),
    empty=[(dict(e=0), (), OK)])
row("gmlm_relation_histogram", dict(e=1, num_relations=1), dict(edge_type="cond", rel_count="req"), null_msg=b"bad arguments",
    cases=nul("edge_type", EINVAL, b"bad arguments") + nul("edge_type", ELAUNCH, e=0) + each("num_relations", (0, 65), EINVAL, b"[1, 64]")
    + each("num_relations", (64,), ELAUNCH) + each("e", (-1,), EINVAL, b"bad arguments"),
    empty=[(dict(e=0), ("rel_count",), ELAUNCH), (dict(e=0, num_relations=0), ("rel_count",), EINVAL)])
row("gmlm_segment_sort", dict(r_active=1, e=1, num_segments=1, workspace_bytes=1 << 30),
    dict(node="cond", rel="null", rel_remap="cond", keys="null", perm="cond", rowptr="req", bad_flag="req", workspace="ws"),
    null_msg=b"bad arguments",
    cases=nul("node perm", EINVAL, b"null pointer") + nul("node perm", ELAUNCH, e=0) + nul("rel_remap", EINVAL, b"without rel_remap")
    + [(dict(rel=None, rel_remap=None), ELAUNCH, None)] + each("r_active", (0,), EINVAL, b"bad arguments")
    + each("e", (-1,), EINVAL, b"bad arguments") + each("num_segments", (-1,), EINVAL, b"bad arguments")
    + each("num_segments", ((1 << 31) - 1,), EINVAL, b"int32 index range") + each("e", ((1 << 31) - 1,), EINVAL, b"int32 index range"),
    ws=("gmlm_segment_sort_workspace_bytes", "e", {}),
    empty=[(dict(e=0), ("rowptr", "bad_flag"), ELAUNCH), (dict(e=0, r_active=0), ("rowptr", "bad_flag"), EINVAL)])
for _n in ("gmlm_gather_i64_to_i32", "gmlm_gather_i32"):
    row(_n, dict(e=1), dict(src="cond", perm="cond", out="cond"),
        cases=nul("src perm out", EINVAL, b"bad arguments") + nul("src perm out", OK, e=0) + each("e", (-1,), EINVAL, b"bad arguments"),
        empty=[(dict(e=0), (), OK)])
row("gmlm_segment_inv_count", dict(num_segments=1), dict(rowptr="cond", inv_cnt="cond"),
    cases=nul("rowptr inv_cnt", EINVAL, b"bad arguments") + nul("rowptr inv_cnt", OK, num_segments=0)
    + each("num_segments", (-1,), EINVAL, b"bad arguments"),
    empty=[(dict(num_segments=0), (), OK)])
row("gmlm_split_plan_build", dict(num_segments=1, num_items=1, long_threshold=1),
    dict(rowptr="req", long_seg="req", chunk_ptr="req", chunk_owner="req"), null_msg=b"bad arguments",
    cases=each("num_segments", (0,), EINVAL, b"bad arguments") + each("num_items", (-1, 1 << 31), EINVAL, b"bad arguments")
    + each("long_threshold", (0, 1 << 30), EINVAL, b"bad arguments")
    + [(dict(num_items=65535 * 4, long_threshold=4), EINVAL, b"long_threshold"), (dict(num_items=65535 * 4 - 1, long_threshold=4), ELAUNCH, None)])

# ---- K2/K3 SpMM.  idx is required when a segment has an edge, which only the caller's rowptr knows: NULL passes the host.
_PLAN = dict(long_threshold=4, n_long=1, n_chunks=1, long_seg=ADDR(40), chunk_ptr=ADDR(41), chunk_owner=ADDR(42), partial=ADDR(43))
row("gmlm_rgcn_mean_spmm",
    dict(src_rows=1, src_stride=8, mean=1, num_segments=1, f=8, out_stride=8, dtype=BF16, long_threshold=0, n_long=0, n_chunks=0),
    dict(src="cond", rowptr="req", idx="null", edge_w="null", out="req", long_seg="cond", chunk_ptr="cond", chunk_owner="cond",
         partial="cond"),
    null_at_base=("long_seg", "chunk_ptr", "chunk_owner", "partial"), null_msg=b"null pointer",
    accepts_misaligned=("src", "out"),                               # misaligned rows take the scalar path
    cases=nul("src", EINVAL, b"null pointer") + nul("src", ELAUNCH, src_rows=0) + [(_PLAN, ELAUNCH, None)]
    + nul("long_seg chunk_ptr chunk_owner partial", EINVAL, b"incomplete split plan", **{k: v for k, v in _PLAN.items()})
    + [(dict(_PLAN, n_chunks=0), EINVAL, b"incomplete split plan"), (dict(_PLAN, n_long=65536), EINVAL, b"65535 long segments"),
       (dict(_PLAN, n_long=65535), ELAUNCH, None)]
    + each("f", (0,), EINVAL, b"bad sizes") + each("num_segments", (-1,), EINVAL, b"bad sizes") + each("src_rows", (-1,), EINVAL, b"bad sizes")
    + each("src_stride", (7,), EINVAL, b"stride") + each("out_stride", (7,), EINVAL, b"stride") + each("f", (7,), ELAUNCH) + DTYPE,
    empty=[(dict(num_segments=0), (), OK), (dict(num_segments=0, dtype=2), (), EINVAL), (dict(num_segments=0, src_stride=4), (), EINVAL)])

# ---- K10 basis composition
_BASIS = (each("r_active", (0, 6), EINVAL, b"active relations") + each("r_active", (5,), ELAUNCH) + each("num_bases", (0, 33), EINVAL, b"bases supported")
          + each("num_bases", (32,), ELAUNCH) + each("cols", (0, 6, -4), EINVAL, b"multiple of 4"))
row("gmlm_basis_compose_fwd", dict(r_active=1, num_bases=1, cols=4), dict(comp="req", weight="req", w="req"),
    null_msg=b"null or misaligned", align="weight w", align_msg=b"null or misaligned", accepts_misaligned=("comp",), cases=_BASIS)
row("gmlm_basis_compose_bwd", dict(r_active=1, num_bases=1, cols=4, workspace_bytes=1 << 30),
    dict(comp="req", weight="req", dw="req", dweight="req", dcomp="req", workspace="ws"),
    null_msg=b"null or misaligned", align="weight dw dweight", align_msg=b"null or misaligned", accepts_misaligned=("comp", "dcomp"),
    cases=_BASIS, ws=("gmlm_basis_compose_bwd_workspace_bytes", "r_active num_bases cols", {}))

# ---- K4 GraphNorm
row("gmlm_colstats", dict(dtype=BF16, n=1, f=8, workspace_bytes=1 << 30),
    dict(x="cond", shift="null", s1="req", s2="req", workspace="ws"), fixed=dict(s1=ADDR(50), s2=ADDR(50) + 32), null_msg=b"bad arguments",
    accepts_misaligned=("x",),
    cases=nul("x", EINVAL, b"bad arguments") + nul("x", ELAUNCH, n=0) + each("f", (0,), EINVAL, b"bad arguments")
    + each("n", (-1,), EINVAL, b"bad arguments") + DTYPE + [(dict(s2=ADDR(50) + 16), EINVAL, b"two rows"), (dict(s2=ADDR(51)), EINVAL, b"two rows")],
    ws=("gmlm_colstats_workspace_bytes", "n f", {}),
    empty=[(dict(n=0), ("s1", "s2"), ELAUNCH), (dict(n=0, dtype=2), ("s1", "s2"), EINVAL)])
row("gmlm_graphnorm_finalize", dict(n_total=1, f=8, eps=1e-5),
    dict(s1="req", s2="req", shift="null", mean_scale="req", mean="req", rstd="req"), null_msg=b"bad arguments",
    cases=each("n_total", (0,), EINVAL, b"bad arguments") + each("f", (0,), EINVAL, b"bad arguments"))
row("gmlm_graphnorm_apply", dict(n=1, f=8, act=1, dropout_p=0.0, seed=1, dtype=BF16),
    dict(x="req", mean="req", rstd="req", weight="req", bias="req", mean_scale="req", y="req"), null_msg=b"null pointer",
    accepts_misaligned=("x", "y"),
    cases=DROPOUT + DTYPE + each("f", (0,), EINVAL, b"bad sizes") + each("n", (-1,), EINVAL, b"bad sizes"),
    empty=[(dict(n=0), (), OK), (dict(n=0, dtype=2), (), EINVAL), (dict(n=0, dropout_p=1.0), (), EINVAL)])
_GN = "g x mean rstd weight bias mean_scale"
row("gmlm_graphnorm_bwd_stats", dict(dtype=BF16, n=1, f=8, act=1, dropout_p=0.0, seed=1, workspace_bytes=1 << 30),
    dict({k: "cond" for k in _GN.split()}, gs="req", workspace="ws"), null_msg=b"bad arguments", accepts_misaligned=("g", "x"),
    cases=nul(_GN, EINVAL, b"null pointer") + nul(_GN, ELAUNCH, n=0) + DROPOUT + DTYPE + each("f", (0,), EINVAL, b"bad arguments")
    + each("n", (-1,), EINVAL, b"bad arguments"),
    ws=("gmlm_colstats_workspace_bytes", "n f", {}),
    empty=[(dict(n=0), ("gs",), ELAUNCH), (dict(n=0, dropout_p=1.0), ("gs",), EINVAL), (dict(n=0, dtype=2), ("gs",), EINVAL)])
row("gmlm_graphnorm_bwd_apply", dict(dtype=BF16, n=1, n_total=1, f=8, act=1, dropout_p=0.0, seed=1),
    dict(g="cond", x="cond", dx="cond", mean="req", rstd="req", weight="req", bias="req", mean_scale="req", gs="req",
         dweight="null", dbias="null", dmean_scale="null"), null_msg=b"graphnorm_bwd_apply", accepts_misaligned=("g", "x", "dx"),
    cases=nul("g x dx", EINVAL, b"null pointer") + nul("g x dx", ELAUNCH, n=0) + DROPOUT + DTYPE + each("n_total", (0,), EINVAL, b"bad arguments")
    + [(dict(n=2, n_total=1), EINVAL, b"bad arguments"), (dict(n=1, n_total=2), ELAUNCH, None)] + each("f", (0,), EINVAL, b"bad arguments"),
    empty=[(dict(n=0), ("mean", "rstd", "weight", "bias", "mean_scale", "gs", "dweight", "dbias", "dmean_scale"), ELAUNCH),
           (dict(n=0, dtype=2), ("mean", "rstd", "weight", "bias", "mean_scale", "gs"), EINVAL)])

# ---- K6 LayerNorm
_LN_SIZES = (each("f", (12, 1032, 2048), EINVAL, b"multiple") + each("f", (1024,), ELAUNCH) + each("f", (0,), EINVAL, b"bad sizes")
             + each("rows", (-1,), EINVAL, b"bad sizes") + [(dict(dtype=F32, f=4), ELAUNCH, None), (dict(dtype=F32, f=6), EINVAL, b"multiple")]
             + DROPOUT + DTYPE)
row("gmlm_bias_res_layernorm_fwd", dict(rows=1, f=8, eps=1e-5, act=1, dropout_p=0.0, seed=1, dtype=BF16),
    dict(x="req", bias="null", residual="null", gamma="req", beta="req", y="req", mean="null", rstd="null"),
    null_msg=b"null pointer", align="x y residual bias gamma beta", align_msg=b"16-byte alignment", cases=_LN_SIZES,
    empty=[(dict(rows=0), (), OK), (dict(rows=0, f=12), (), EINVAL), (dict(rows=0, dtype=2), (), EINVAL)])
row("gmlm_bias_res_layernorm_bwd", dict(rows=1, f=8, act=1, dropout_p=0.0, seed=1, dtype=BF16, workspace_bytes=1 << 30),
    dict(dy="req", x="req", bias="null", residual="null", gamma="req", beta="req", mean="req", rstd="req", dx="req", dresidual="null",
         dgamma="null", dbeta="null", dbias="null", workspace="ws"),
    null_msg=b"null pointer", align="dy x dx residual dresidual bias gamma beta", align_msg=b"16-byte alignment", cases=_LN_SIZES,
    ws=("gmlm_layernorm_bwd_workspace_bytes", "rows f", {}),
    empty=[(dict(rows=0), (), OK), (dict(rows=0), ("dgamma", "dbeta", "dbias"), ELAUNCH), (dict(rows=0, f=12), ("dgamma",), EINVAL)])

# ---- attention, d = 64 / 96
_PACKED = dict(cu_seqlens=ADDR(60), kv_len=None, max_len=1)
_SHORT = dict(b=512, lq=16, lk=16)                                    # bf16, d = 64, <= 128 rows, b*h >= 512: the LDS-resident kernels
_SHORT_RING = dict(b=64, h=8, lq=64, lk=64, **{k + "_stride": 512 for k in ("q", "k", "v", "dq", "dk", "dv")})   # a ring block's shape


def _strides(names, width, big=1 << 24):
    out = []
    for n in names.split():
        out += each(n, (width - 8, width + 4, big), EINVAL, b"row stride") + each(n, (width + 8,), ELAUNCH)
    return out


_ATT_COMMON = (each("d", (128, 32, 0), EINVAL, b"head dim")
               + each("h", (0,), EINVAL, b"bad sizes") + each("b", (-1,), EINVAL, b"bad sizes") + each("b", (65536,), EINVAL, b"65535")
               + each("b", (65535,), ELAUNCH) + DTYPE + DROPOUT + each("scale", (0.0, -1.0), EINVAL, b"scale must be positive")
               + [(_PACKED, ELAUNCH, None), (dict(_PACKED, kv_len=ADDR(61)), EINVAL, b"packed mode"), (dict(_PACKED, max_len=0), EINVAL, b"packed mode"),
                  (dict(_PACKED, lk=2), EINVAL, b"packed mode"),
                  (dict(_PACKED, seq_groups=ADDR(62), num_groups=1), ELAUNCH, None), (dict(seq_groups=ADDR(62), num_groups=1), EINVAL, b"seq_groups"),
                  (dict(_PACKED, seq_groups=ADDR(62), num_groups=2), EINVAL, b"seq_groups"),
                  (dict(_PACKED, seq_groups=ADDR(62), num_groups=0), EINVAL, b"seq_groups"),
                  (dict(kv_len=None), ELAUNCH, None), (_SHORT, ELAUNCH, None),
                  (dict(dtype=F32, out_lo=None), ELAUNCH, None), (dict(dtype=F32), EINVAL, b"out_lo"), (dict(out_lo=Off(4)), EINVAL, b"out_lo"),
                  (dict(out_lo=Off(2)), EINVAL, b"out_lo")])
_ATT_BASE = dict(b=1, h=1, lq=1, lk=1, d=64, q_stride=64, k_stride=64, v_stride=64, scale=0.125, dropout_p=0.0, seed=1, dtype=BF16,
                 max_len=0, num_groups=0)
row("gmlm_attention_fwd", _ATT_BASE,
    dict(q="req", k="cond", v="cond", kv_len="cond", out="req", out_lo="cond", lse="null", cu_seqlens="cond", seq_groups="cond"),
    null_at_base=("cu_seqlens", "seq_groups"), null_msg=b"null or", align="q k v out", align_msg=b"aligned",
    cases=_ATT_COMMON + _strides("q_stride k_stride v_stride", 64) + nul("k v", EINVAL, b"null or not 16-byte")
    + [(dict(k=None, v=None, lk=0), ELAUNCH, None), (dict(d=96, q_stride=96, k_stride=96, v_stride=96), ELAUNCH, None), (dict(d=96), EINVAL, b"row stride")],
    empty=[(dict(b=0), (), OK), (dict(lq=0), (), OK), (dict(b=0, d=128), (), EINVAL), (dict(lq=0, dtype=2), (), EINVAL)])
row("gmlm_attention_bwd", dict(_ATT_BASE, dq_stride=64, dk_stride=64, dv_stride=64, workspace_bytes=1 << 30),
    dict(q="req", k="req", v="req", out="req", dout="req", lse="req", kv_len="cond", dq="req", dk="req", dv="req", cu_seqlens="cond",
         workspace="ws", dbias_partial="cond", dbias="cond", out_lo="cond", seq_groups="cond"),
    null_at_base=("cu_seqlens", "seq_groups", "dbias_partial", "dbias"), null_msg=b"null or", align="q k v dq dk dv out dout", align_msg=b"aligned",
    cases=_ATT_COMMON + _strides("q_stride k_stride v_stride dq_stride dk_stride dv_stride", 64)
    + [(dict(dbias=ADDR(63)), EINVAL, b"come together"), (dict(dbias_partial=ADDR(64)), EINVAL, b"come together"),
       (dict(dbias=ADDR(63), dbias_partial=ADDR(64)), EINVAL, b"short-sequence path"),
       # the short-sequence backward sums delta over its own keys (it assumes its own lse), so it is selected only without out_lo:
       # out_lo with the bias sums is refused with the streaming path's message, which shows that path was chosen
       (dict(_SHORT, out_lo=None, dbias=ADDR(63), dbias_partial=ADDR(64)), ELAUNCH, None),
       (dict(_SHORT, dbias=ADDR(63), dbias_partial=ADDR(64)), EINVAL, b"only on the short-sequence path"),
       (dict(_SHORT_RING, dbias=ADDR(63), dbias_partial=ADDR(64)), EINVAL, b"only on the short-sequence path"),
       (_SHORT_RING, ELAUNCH, None), (dict(_SHORT_RING, out_lo=None), ELAUNCH, None),
       (dict(_SHORT_RING, out_lo=None, dbias=ADDR(63), dbias_partial=ADDR(64)), ELAUNCH, None),
       (dict(_SHORT_RING, out_lo=None, workspace_bytes=0), EWORKSPACE, b"workspace"),
       (dict(lq=0), EINVAL, b"empty query or key"), (dict(lk=0), EINVAL, b"empty query or key"),
       (dict({k + "_stride": 96 for k in ("q", "k", "v", "dq", "dk", "dv")}, d=96), ELAUNCH, None), (dict(d=96), EINVAL, b"row stride")],
    ws=("gmlm_attention_bwd_workspace_bytes", "b h lq lk d", {}),
    empty=[(dict(b=0), (), OK), (dict(lq=0, lk=0), (), OK), (dict(b=0, d=128), (), EINVAL), (dict(b=0, scale=0.0), (), EINVAL)])

# ---- attention, d = 128
_D128_BASE = dict(b=1, h=1, lq=1, lk=1, d=128, q_stride=128, k_stride=128, v_stride=128, scale=0.088, dropout_p=0.0, seed=1, dtype=BF16)
_D128 = (each("d", (64, 96), EINVAL, b"head dim") + each("h", (0,), EINVAL, b"bad sizes") + each("b", (-1,), EINVAL, b"bad sizes") + DTYPE + DROPOUT
         + each("scale", (0.0,), EINVAL, b"scale must be positive") + each("b", (65536,), ELAUNCH) + [(dict(kv_len=None), ELAUNCH, None)]
         + [(dict(dtype=F32, out_lo=None), ELAUNCH, None), (dict(dtype=F32), EINVAL, b"out_lo"), (dict(out_lo=Off(4)), EINVAL, b"out_lo")])
row("gmlm_attention_d128_fwd", _D128_BASE, dict(q="req", k="cond", v="cond", kv_len="null", out="req", out_lo="cond", lse="null"),
    null_msg=b"null or", align="q k v out", align_msg=b"aligned",
    cases=_D128 + _strides("q_stride k_stride v_stride", 128) + nul("k v", EINVAL, b"null or not 16-byte") + [(dict(k=None, v=None, lk=0), ELAUNCH, None)],
    empty=[(dict(b=0), (), OK), (dict(lq=0), (), OK), (dict(b=0, d=64), (), EINVAL)])
row("gmlm_attention_d128_bwd", dict(_D128_BASE, dq_stride=128, dk_stride=128, dv_stride=128, workspace_bytes=1 << 30),
    dict(q="req", k="req", v="req", out="req", out_lo="cond", dout="req", lse="req", kv_len="null", dq="req", dk="req", dv="req", workspace="ws"),
    null_msg=b"null or", align="q k v dq dk dv out dout", align_msg=b"aligned",
    cases=_D128 + _strides("q_stride k_stride v_stride dq_stride dk_stride dv_stride", 128)
    + [(dict(lq=0), EINVAL, b"empty query or key"), (dict(lk=0), EINVAL, b"empty query or key")],
    ws=("gmlm_attention_d128_workspace_bytes", "b h lq", {}),
    empty=[(dict(b=0), (), OK), (dict(lq=0, lk=0), (), OK), (dict(b=0, dtype=2), (), EINVAL)])

# ---- causal attention, d = 128, grouped KV heads
_CAUSAL_BASE = dict(b=1, hq=2, hkv=1, lq=1, lk=1, d=128, q_stride=256, k_stride=128, v_stride=128, scale=0.088, dropout_p=0.0, dtype=BF16)
_CAUSAL = (each("d", (64,), EINVAL, b"head dim") + each("hkv", (0,), EINVAL, b"bad sizes") + [(dict(hq=3, hkv=2, q_stride=384, k_stride=256, v_stride=256), EINVAL, b"multiple")]
           + DTYPE + each("dropout_p", (-0.1, 1.0, 0.1), EINVAL, b"dropout_p must be 0") + each("scale", (0.0,), EINVAL, b"scale must be positive")
           + [(dict(dtype=F32, out_lo=None), ELAUNCH, None), (dict(dtype=F32), EINVAL, b"out_lo"), (dict(out_lo=Off(4)), EINVAL, b"out_lo")])
_CAUSAL_BWD_STRIDES = _strides("q_stride dq_stride", 256) + _strides("k_stride v_stride dk_stride dv_stride", 128)
row("gmlm_attention_causal_d128_fwd", _CAUSAL_BASE, dict(q="req", k="req", v="req", kv_len="null", out="req", out_lo="cond", lse="null"),
    null_msg=b"null or", align="q k v out", align_msg=b"aligned",
    cases=_CAUSAL + [(dict(lk=2), EINVAL, b"lq == lk")] + _strides("q_stride", 256) + _strides("k_stride v_stride", 128),
    empty=[(dict(b=0), (), OK), (dict(lq=0, lk=0), (), OK), (dict(b=0, d=64), (), EINVAL)])
row("gmlm_attention_causal_d128_bwd", dict(_CAUSAL_BASE, dq_stride=256, dk_stride=128, dv_stride=128, workspace_bytes=1 << 30),
    dict(q="req", k="req", v="req", out="req", out_lo="cond", dout="req", lse="req", kv_len="null", dq="req", dk="req", dv="req", workspace="ws"),
    null_msg=b"null or", align="q k v dq dk dv out dout", align_msg=b"aligned",
    cases=_CAUSAL + [(dict(lk=2), EINVAL, b"lq == lk")] + _CAUSAL_BWD_STRIDES,
    ws=("gmlm_attention_causal_d128_workspace_bytes", "b hq lq", {}),
    empty=[(dict(b=0), (), OK), (dict(lq=0, lk=0), (), OK), (dict(b=0, dtype=2), (), EINVAL)])
_VARLEN_BASE = dict(num_seqs=1, max_len=1, total_rows=1, hq=2, hkv=1, d=128, q_stride=256, k_stride=128, v_stride=128, scale=0.088,
                    dropout_p=0.0, dtype=BF16)
_VARLEN = _CAUSAL + each("max_len", (0,), EINVAL, b"max_len") + each("total_rows", (1 << 30, -1), EINVAL, b"2^30") + each("num_seqs", (-1,), EINVAL)
# cu_seqlens is required even by the empty call: the header calls it "required" and it is the first check
row("gmlm_attention_causal_d128_varlen_fwd", _VARLEN_BASE, dict(q="req", k="req", v="req", cu_seqlens="req", out="req", out_lo="cond", lse="null"),
    null_msg=b"null", align="q k v out", align_msg=b"aligned",
    cases=_VARLEN + _strides("q_stride", 256) + _strides("k_stride v_stride", 128),
    empty=[(dict(num_seqs=0), ("cu_seqlens",), OK), (dict(total_rows=0), ("cu_seqlens",), OK), (dict(total_rows=0, d=64), ("cu_seqlens",), EINVAL)])
row("gmlm_attention_causal_d128_varlen_bwd", dict(_VARLEN_BASE, dq_stride=256, dk_stride=128, dv_stride=128, workspace_bytes=1 << 30),
    dict(q="req", k="req", v="req", out="req", out_lo="cond", dout="req", lse="req", cu_seqlens="req", dq="req", dk="req", dv="req", workspace="ws"),
    null_msg=b"null", align="q k v dq dk dv out dout", align_msg=b"aligned", cases=_VARLEN + _CAUSAL_BWD_STRIDES,
    ws=("gmlm_attention_causal_d128_varlen_workspace_bytes", "total_rows hq", {}),
    empty=[(dict(num_seqs=0), ("cu_seqlens",), OK), (dict(total_rows=0), ("cu_seqlens",), OK), (dict(total_rows=0, dtype=2), ("cu_seqlens",), EINVAL)])

# ---- decoder row kernels
_RMS = (each("f", (12, 4104, 0), EINVAL, b"4096") + each("f", (4096,), ELAUNCH) + [(dict(dtype=F32, f=4), ELAUNCH, None), (dict(dtype=F32, f=6), EINVAL, b"multiple of")]
        + each("rows", (-1,), EINVAL) + DTYPE)
row("gmlm_add_rmsnorm_fwd", dict(rows=1, f=8, eps=1e-6, dtype=BF16), dict(a="req", b="cond", w="req", s="cond", y="req", rstd="req"),
    null_msg=b"null or not 16-byte", align="a b w s y", align_msg=b"null or not 16-byte",
    cases=_RMS + nul("b s", EINVAL, b"exactly when b is") + [(dict(b=None, s=None), ELAUNCH, None)],
    empty=[(dict(rows=0), (), OK), (dict(rows=0, f=12), (), EINVAL)])
row("gmlm_add_rmsnorm_bwd", dict(rows=1, f=8, dtype=BF16, workspace_bytes=1 << 30),
    dict(dy="cond", dres="null", s="cond", w="cond", rstd="cond", ds="cond", dw="req", workspace="ws"),
    null_msg=b"null dw", align="dy dres s w ds", align_msg=b"null or not 16-byte",
    cases=_RMS + nul("dy s w rstd ds", EINVAL, b"null or not 16-byte") + nul("dy s w rstd ds", ELAUNCH, rows=0),
    ws=("gmlm_add_rmsnorm_bwd_workspace_bytes", "rows f", {}),
    empty=[(dict(rows=0), ("dw",), ELAUNCH), (dict(rows=0), (), EINVAL), (dict(rows=0, f=12), ("dw",), EINVAL)])
_ROPE_BASE = dict(qkv_stride=384, max_len=1, tokens=1, hq=1, hkv=1, d=128, dtype=BF16)
_ROPE = (each("d", (64,), EINVAL, b"head dim") + each("hq", (0,), EINVAL, b"bad sizes") + each("max_len", (0,), EINVAL, b"empty cos / sin table") + DTYPE
         + each("qkv_stride", (376, 388), EINVAL, b"qkv row stride") + each("qkv_stride", (392,), ELAUNCH) + each("tokens", (-1,), EINVAL, b"bad sizes"))
_ROPE_SEQ = each("seq_len", (2,), EINVAL, b"exceeds") + each("seq_len", (0,), EINVAL, b"length 0")
_ROPE_FWD_PTR = dict(qkv="cond", q_weight="cond", k_weight="cond", cos_sin="cond", out="cond", rstd="cond")
_ROPE_OUT = each("out_stride", (248, 260), EINVAL, b"row stride") + each("out_stride", (264,), ELAUNCH)
_ROPE_FWD_NUL = nul("qkv q_weight k_weight cos_sin out rstd", EINVAL, b"null") + nul("qkv q_weight k_weight cos_sin out rstd", OK, tokens=0)
row("gmlm_qknorm_rope_fwd", dict(_ROPE_BASE, seq_len=1, eps=1e-6, out_stride=256), _ROPE_FWD_PTR,
    align="qkv out q_weight k_weight cos_sin", align_msg=b"aligned", cases=_ROPE + _ROPE_SEQ + _ROPE_OUT + _ROPE_FWD_NUL,
    empty=[(dict(tokens=0), (), OK), (dict(tokens=0, seq_len=0), (), OK), (dict(tokens=0, d=64), (), EINVAL)])
row("gmlm_qknorm_rope_pos_fwd", dict(_ROPE_BASE, eps=1e-6, out_stride=256), dict(_ROPE_FWD_PTR, pos_ids="cond"),
    align="qkv out q_weight k_weight cos_sin", align_msg=b"aligned",
    cases=_ROPE + _ROPE_OUT + _ROPE_FWD_NUL + nul("pos_ids", EINVAL, b"null pos_ids") + nul("pos_ids", OK, tokens=0),
    empty=[(dict(tokens=0), (), OK), (dict(tokens=0, d=64), (), EINVAL)])
_ROPE_BWD_PTR = dict(dqkv="cond", qkv="cond", q_weight="cond", k_weight="cond", cos_sin="cond", rstd="cond", dq_weight="req", dk_weight="req",
                     workspace="ws")
_ROPE_DW = dict(dq_weight=ADDR(70), dk_weight=ADDR(70) + 512)
_ROPE_BWD_NUL = (nul("dqkv qkv q_weight k_weight cos_sin rstd", EINVAL, b"null") + nul("dqkv qkv q_weight k_weight cos_sin rstd", ELAUNCH, tokens=0)
                 + [(dict(dk_weight=ADDR(71)), EINVAL, b"[2, 128]"), (dict(dk_weight=ADDR(70) + 256), EINVAL, b"[2, 128]")]
                 + each("dqkv_stride", (248, 260), EINVAL, b"row stride") + each("dqkv_stride", (264,), ELAUNCH))
row("gmlm_qknorm_rope_bwd", dict(_ROPE_BASE, seq_len=1, dqkv_stride=384, workspace_bytes=1 << 30), _ROPE_BWD_PTR, fixed=_ROPE_DW,
    null_msg=b"[2, 128]", align="dqkv qkv q_weight k_weight cos_sin", align_msg=b"aligned", cases=_ROPE + _ROPE_SEQ + _ROPE_BWD_NUL,
    ws=("gmlm_qknorm_rope_bwd_workspace_bytes", "tokens hq hkv dtype", {}),
    empty=[(dict(tokens=0), ("dq_weight", "dk_weight"), ELAUNCH), (dict(tokens=0), (), EINVAL), (dict(tokens=0, d=64), ("dq_weight", "dk_weight"), EINVAL)])
row("gmlm_qknorm_rope_pos_bwd", dict(_ROPE_BASE, dqkv_stride=384, workspace_bytes=1 << 30), dict(_ROPE_BWD_PTR, pos_ids="cond"), fixed=_ROPE_DW,
    null_msg=b"[2, 128]", align="dqkv qkv q_weight k_weight cos_sin", align_msg=b"aligned",
    cases=_ROPE + _ROPE_BWD_NUL + nul("pos_ids", EINVAL, b"null pos_ids") + nul("pos_ids", ELAUNCH, tokens=0),
    ws=("gmlm_qknorm_rope_bwd_workspace_bytes", "tokens hq hkv dtype", {}),
    empty=[(dict(tokens=0), ("dq_weight", "dk_weight"), ELAUNCH), (dict(tokens=0, dtype=2), ("dq_weight", "dk_weight"), EINVAL)])
_SWIGLU = each("inter", (12, 0), EINVAL, b"multiple of") + [(dict(dtype=F32, inter=4), ELAUNCH, None)] + each("rows", (-1,), EINVAL) + DTYPE
row("gmlm_swiglu_fwd", dict(rows=1, inter=8, dtype=BF16), dict(gate_up="cond", y="cond"), align="gate_up y", align_msg=b"null or not 16-byte",
    cases=_SWIGLU + nul("gate_up y", EINVAL, b"null or not 16-byte") + nul("gate_up y", OK, rows=0),
    empty=[(dict(rows=0), (), OK), (dict(rows=0, inter=12), (), EINVAL)])
row("gmlm_swiglu_bwd", dict(rows=1, inter=8, dtype=BF16), dict(dy="cond", gate_up="cond", dgate_up="cond"), align="dy gate_up dgate_up",
    align_msg=b"null or not 16-byte",
    cases=_SWIGLU + nul("dy gate_up dgate_up", EINVAL, b"null or not 16-byte") + nul("dy gate_up dgate_up", OK, rows=0),
    empty=[(dict(rows=0), (), OK), (dict(rows=0, dtype=2), (), EINVAL)])

# ---- embedding sum, mean pool, soft mask, bias + GELU
row("gmlm_embed_sum_fwd", dict(rows=1, p=4, vocab=1, npos=1, dtype=BF16),
    dict(word="req", pos="req", type0="req", tok="req", pos_ids="req", out="req", bad_flag="null"), null_msg=b"null pointer",
    align="word pos type0 out", align_msg=b"16-byte aligned",
    cases=each("p", (6, 0), EINVAL, b"multiple of 4") + each("vocab", (0,), EINVAL, b"bad sizes") + each("npos", (0,), EINVAL, b"bad sizes")
    + each("rows", (-1,), EINVAL, b"bad sizes") + DTYPE,
    empty=[(dict(rows=0), (), OK), (dict(rows=0, p=6), (), EINVAL)])
_POOL = (each("b", (65536,), EINVAL, b"65535") + each("b", (65535,), ELAUNCH) + each("p", (0,), EINVAL, b"bad sizes") + each("l", (-1,), EINVAL, b"bad sizes") + DTYPE
         + nul("len", EINVAL, b"null pointer") + [(dict(len=None, cu_seqlens=None), EINVAL, b"null pointer"), (dict(len=None, cu_seqlens=ADDR(80)), ELAUNCH, None), (dict(cu_seqlens=ADDR(80)), ELAUNCH, None)])
row("gmlm_meanpool_scatter_fwd", dict(b=1, l=1, p=1, dtype=BF16), dict(hs="cond", len="cond", node_idx="req", out="req", cu_seqlens="cond"),
    null_at_base=("cu_seqlens",), null_msg=b"null pointer", accepts_misaligned=("hs", "out"),
    cases=_POOL + nul("hs", EINVAL, b"null pointer") + nul("hs", ELAUNCH, l=0),
    empty=[(dict(b=0), (), OK), (dict(b=0, dtype=2), (), EINVAL)])
row("gmlm_meanpool_scatter_bwd", dict(b=1, l=1, p=1, dtype=BF16), dict(dout="req", len="cond", node_idx="req", dhs="req", cu_seqlens="cond"),
    null_at_base=("cu_seqlens",), null_msg=b"null pointer", accepts_misaligned=("dout", "dhs"), cases=_POOL,
    empty=[(dict(b=0), (), OK), (dict(l=0), (), OK), (dict(b=0, p=0), (), EINVAL)])
row("gmlm_softmask_blend_fwd", dict(beta=0.7, n=1, f=3, out_stride=3, dtype=BF16), dict(x="req", mask="req", token="req", out="req"),
    null_msg=b"null pointer", accepts_misaligned=("x", "token", "out"),
    cases=each("out_stride", (2,), EINVAL, b"bad sizes") + each("out_stride", (5,), ELAUNCH) + each("f", (0,), EINVAL, b"bad sizes")
    + each("n", (-1,), EINVAL, b"bad sizes") + DTYPE,
    empty=[(dict(n=0), (), OK), (dict(n=0, out_stride=2), (), EINVAL)])
row("gmlm_softmask_blend_bwd", dict(dout_stride=3, beta=0.7, n=1, f=3, workspace_bytes=1 << 30),
    dict(dout="cond", mask="cond", dtoken="req", workspace="ws"), null_msg=b"bad arguments", accepts_misaligned=("dout",),
    cases=nul("dout mask", EINVAL, b"null pointer") + nul("dout mask", ELAUNCH, n=0) + each("dout_stride", (2,), EINVAL, b"bad arguments")
    + each("f", (0,), EINVAL, b"bad arguments"),
    ws=("gmlm_softmask_blend_bwd_workspace_bytes", "n f", {}),
    empty=[(dict(n=0), ("dtoken",), ELAUNCH), (dict(n=0, dout_stride=2), ("dtoken",), EINVAL)])
_BG = (each("f", (12, 0), EINVAL) + [(dict(dtype=F32, f=4), ELAUNCH, None), (dict(dtype=F32, f=6), EINVAL, b"multiple of")] + each("rows", (-1,), EINVAL, b"bad sizes")
       + DROPOUT + DTYPE)
row("gmlm_bias_gelu_fwd", dict(rows=1, f=8, dropout_p=0.0, seed=1, dtype=BF16), dict(x="req", bias="null", y="req"),
    null_msg=b"null or misaligned", align="x y", align_msg=b"null or misaligned", accepts_misaligned=("bias",), cases=_BG,
    empty=[(dict(rows=0), (), OK), (dict(rows=0, f=12), (), EINVAL)])
row("gmlm_bias_gelu_bwd", dict(rows=1, f=8, dropout_p=0.0, seed=1, dtype=BF16, workspace_bytes=1 << 30),
    dict(dy="req", x="req", bias="null", dx="req", dbias="null", workspace="ws"),
    null_msg=b"null or misaligned", align="dy x dx", align_msg=b"null or misaligned", accepts_misaligned=("bias",),
    cases=_BG + [(dict(dbias=None, workspace=None, workspace_bytes=0), ELAUNCH, None)],
    ws=("gmlm_bias_gelu_bwd_workspace_bytes", "rows f dtype", {}),
    empty=[(dict(rows=0), (), OK), (dict(rows=0), ("dbias",), ELAUNCH), (dict(rows=0, dropout_p=1.0), (), EINVAL)])

# ---- split-K weight gradient (no empty call: t >= 32 always)
row("gmlm_wgrad_bf16", dict(ld_dy=256, ld_x=256, t=32, n=256, k=256, splits=0, ld_out=256, flags=0, workspace_bytes=1 << 30),
    dict(dy="req", x="req", out="req", workspace="ws"), null_msg=b"null pointer", align="dy x out workspace", align_msg=b"16-byte aligned",
    cases=each("t", (31, 0), EINVAL, b"need t >=") + each("t", (33,), ELAUNCH) + each("n", (128, 257, 264), EINVAL, b"multiples of 256")
    + each("k", (255, 384), EINVAL, b"multiples of 256") + each("n", (0,), EINVAL, b"need t >=") + each("ld_dy", (248,), EINVAL, b"smaller than the row")
    + each("ld_x", (255,), EINVAL, b"smaller than the row") + each("ld_out", (252,), EINVAL, b"smaller than the row")
    + each("ld_dy", (260,), EINVAL, b"16-byte aligned") + each("ld_x", (257,), EINVAL, b"16-byte aligned") + each("ld_out", (258,), EINVAL, b"16-byte aligned")
    + each("ld_dy", (264,), ELAUNCH) + each("ld_out", (260,), ELAUNCH) + each("splits", (-1,), EINVAL, b"bad splits") + each("flags", (4,), EINVAL, b"bad splits")
    + each("flags", (3,), ELAUNCH) + each("ld_dy", (1 << 26,), EINVAL, b"too large"),
    ws=("gmlm_wgrad_workspace_bytes", "t n k splits", {}))

# Empty calls that still launch, because they owe an output its zeros (ELAUNCH here), by name with the output they fill.
ZERO_FILLING_EMPTY_CALLS = {
    "gmlm_degree_i32": "deg", "gmlm_degree_f32": "deg", "gmlm_relation_histogram": "rel_count", "gmlm_segment_sort": "rowptr",
    "gmlm_colstats": "s1 / s2", "gmlm_graphnorm_bwd_stats": "gs", "gmlm_graphnorm_bwd_apply": "dweight / dbias / dmean_scale (from gs)",
    "gmlm_bias_res_layernorm_bwd": "dgamma / dbeta / dbias", "gmlm_softmask_blend_bwd": "dtoken", "gmlm_bias_gelu_bwd": "dbias",
    "gmlm_add_rmsnorm_bwd": "dw", "gmlm_qknorm_rope_bwd": "dq_weight", "gmlm_qknorm_rope_pos_bwd": "dq_weight",
}


# ------------------------------------------------------------------------------------------------------- table checks
def table_gaps(protos, rows):
    """What the table lacks against the header: rows, pointer classes, both sides of a condition."""
    gaps = []
    launching = [n for n, (ret, _) in protos.items() if ret == "int" and n not in HOST_ONLY]
    gaps += [f"{n}: no table row" for n in launching if n not in rows]
    gaps += [f"{n}: table row without a prototype" for n in rows if n not in launching]
    for name, r in rows.items():
        if name not in protos:
            continue
        params = protos[name][1]
        pointers = [pn for ct, pn in params if is_pointer(ct) and pn not in ALWAYS_NULLABLE]
        scalars = [pn for ct, pn in params if not is_pointer(ct)]
        gaps += [f"{name}: pointer `{p}` is not classified" for p in pointers if r["ptr"].get(p) not in ("req", "null", "cond", "ws")]
        gaps += [f"{name}: `{p}` classified but not a pointer of the prototype" for p in r["ptr"] if p not in pointers]
        gaps += [f"{name}: no baseline value for `{s}`" for s in scalars if s not in r["base"]]
        gaps += [f"{name}: baseline names `{s}`, which the prototype lacks" for s in r["base"] if s not in scalars]
        if ("workspace" in pointers) != (r["ws"] is not None) or ("workspace" in pointers) != (r["ptr"].get("workspace") == "ws"):
            gaps.append(f"{name}: workspace and its companion do not go together")
        for p, cls in r["ptr"].items():
            if cls != "cond":
                continue
            outcomes = {rc in (OK, ELAUNCH) for mut, rc, _ in r["cases"] if p in mut}
            if outcomes != {True, False}:
                gaps.append(f"{name}: conditional pointer `{p}` is not exercised on both sides of its condition")
        if any(rc == ELAUNCH for _, _, rc in r["empty"]) != (name in ZERO_FILLING_EMPTY_CALLS):
            gaps.append(f"{name}: launching empty call and ZERO_FILLING_EMPTY_CALLS disagree")
    return gaps


def test_every_entry_point_and_pointer_is_in_the_table():
    assert len(PROTOS) >= 60 and not table_gaps(PROTOS, ROWS), table_gaps(PROTOS, ROWS)


def test_table_check_notices_a_missing_row_and_an_unclassified_pointer():
    fewer = {k: v for k, v in ROWS.items() if k != "gmlm_colstats"}
    assert any("gmlm_colstats: no table row" in g for g in table_gaps(PROTOS, fewer))
    r = ROWS["gmlm_bias_res_layernorm_bwd"]
    holed = dict(ROWS, gmlm_bias_res_layernorm_bwd=dict(r, ptr={k: v for k, v in r["ptr"].items() if k != "dresidual"}))
    assert any("`dresidual` is not classified" in g for g in table_gaps(PROTOS, holed))
    grown = parse_header("int gmlm_new_entry(const float* a, int64_t n, gmlm_stream_t stream);\n")
    assert table_gaps(dict(PROTOS, **grown), ROWS) == ["gmlm_new_entry: no table row"]
    one_sided = dict(ROWS, gmlm_colstats=dict(ROWS["gmlm_colstats"], cases=[c for c in ROWS["gmlm_colstats"]["cases"] if c[1] != ELAUNCH]))
    assert any("`x` is not exercised on both sides" in g for g in table_gaps(PROTOS, one_sided))


# ---------------------------------------------------------------------------------------------------------- signatures
def test_ctypes_signatures_mirror_the_header():
    from gmlm_amd._lib import SIGNATURES
    assert not signature_mismatches(PROTOS, SIGNATURES), signature_mismatches(PROTOS, SIGNATURES)
    ret, params = PROTOS["gmlm_attention_bwd"]
    assert ret == "int" and len(params) == 36 and params[0] == ("const void *", "q") and params[-1] == ("gmlm_stream_t", "stream")
    assert PROTOS["gmlm_last_error"] == ("const char *", []) and PROTOS["gmlm_segment_sort_workspace_bytes"] == ("size_t", [("int64_t", "e")])


def test_signature_check_notices_a_wrong_type_a_swap_and_a_missing_parameter():
    from gmlm_amd._lib import SIGNATURES
    res, args = SIGNATURES["gmlm_relation_histogram"]                # (ptr, i64 e, int num_relations, ptr, ptr)
    widened = dict(SIGNATURES, gmlm_relation_histogram=(res, args[:2] + [C.c_int64] + args[3:]))
    assert signature_mismatches(PROTOS, widened) == ["gmlm_relation_histogram: parameter 2 `int num_relations` bound as %s" % C.c_int64]
    swapped = dict(SIGNATURES, gmlm_relation_histogram=(res, [args[1], args[0]] + args[2:]))
    assert len(signature_mismatches(PROTOS, swapped)) == 2
    short = dict(SIGNATURES, gmlm_relation_histogram=(res, args[:-1]))
    assert any("5 parameters in the header, 4 in SIGNATURES" in m for m in signature_mismatches(PROTOS, short))
    assert any("returns size_t" in m for m in signature_mismatches(PROTOS, dict(SIGNATURES, gmlm_colstats_workspace_bytes=(C.c_int, [C.c_int64] * 2))))
    assert any("only in SIGNATURES" in m for m in signature_mismatches(PROTOS, dict(SIGNATURES, gmlm_extra=(C.c_int, []))))
    f32 = dict(SIGNATURES, gmlm_softmask_blend_fwd=(res, [C.c_void_p] * 3 + [C.c_double] + SIGNATURES["gmlm_softmask_blend_fwd"][1][4:]))
    assert any("`float beta`" in m for m in signature_mismatches(PROTOS, f32))


# --------------------------------------------------------------------------------------------------------------- calls
@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    import gmlm_amd
    return gmlm_amd.lib()


def baseline(name):
    r, args = ROWS[name], {}
    for i, (ct, pn) in enumerate(PROTOS[name][1]):
        if is_pointer(ct):
            args[pn] = None if (pn in ALWAYS_NULLABLE or pn in r["null_at_base"]) else r["fixed"].get(pn, ADDR(i + 1))
        else:
            args[pn] = r["base"][pn]
    return args


def call(lib, name, mut=None, only=None):
    """The row's valid call with `mut` applied; only = the pointers that stay, every other one NULL (empty calls)."""
    args = baseline(name)
    for k, v in (mut or {}).items():
        assert k in args, (name, k)
        args[k] = args[k] + v.n if isinstance(v, Off) else v
    if only is not None:
        for ct, pn in PROTOS[name][1]:
            if is_pointer(ct) and pn not in only:
                args[pn] = None
    rc = getattr(lib, name)(*[args[pn] for _, pn in PROTOS[name][1]])
    return rc, lib.gmlm_last_error()


def expect(lib, name, mut, rc, msg=None, only=None):
    got, err = call(lib, name, mut, only)
    assert got == rc and (msg is None or msg in err), f"{name}{mut or ''} kept={only}: code {got} (want {rc}), message {err!r} (want {msg!r})"
    if rc == ELAUNCH:                                     # passed validation: the failure is the missing device, nothing else
        assert b"device" in err.lower() or b"hip" in err.lower(), (name, mut, err)


NAMES = sorted(ROWS)


@pytest.mark.parametrize("name", NAMES)
def test_baseline_passes_validation(lib, name):
    expect(lib, name, None, ELAUNCH)
    addrs = [v for v in baseline(name).values() if isinstance(v, int) and v >= ADDR(0)]
    assert len(set(addrs)) == len(addrs) and all(a % 16 == 0 for a in addrs)


@pytest.mark.parametrize("name", NAMES)
def test_pointer_classes(lib, name):
    r = ROWS[name]
    for p, cls in r["ptr"].items():
        if cls == "req":
            expect(lib, name, {p: None}, EINVAL, r["null_msg"] if r["null_msg"] else b"null")
        elif cls == "null":
            expect(lib, name, {p: None}, ELAUNCH)
    for p in ALWAYS_NULLABLE & {pn for _, pn in PROTOS[name][1]}:
        expect(lib, name, {p: ADDR(90)}, ELAUNCH)


@pytest.mark.parametrize("name", NAMES)
def test_alignment_rule(lib, name):
    r = ROWS[name]
    assert not set(r["align"]) & set(r["accepts_misaligned"])
    for p in r["align"]:
        for shift in (4, 2, 8):
            expect(lib, name, {p: Off(shift)}, EINVAL, r["align_msg"])
        expect(lib, name, {p: Off(16)}, ELAUNCH)
    for p in r["accepts_misaligned"]:                     # scalar accesses (header): element alignment is enough
        for shift in (4, 2) if r["base"].get("dtype") == BF16 and p not in ("comp", "dcomp", "token", "dout", "bias") else (4,):
            expect(lib, name, {p: Off(shift)}, ELAUNCH)


@pytest.mark.parametrize("name", NAMES)
def test_documented_refusals_and_edges(lib, name):
    for mut, rc, msg in ROWS[name]["cases"]:
        expect(lib, name, mut, rc, msg)


WS_NAMES = [n for n in NAMES if ROWS[n]["ws"]]


@pytest.mark.parametrize("name", WS_NAMES)
def test_workspace_boundary(lib, name):
    companion, argnames, mut = ROWS[name]["ws"]
    base = dict(baseline(name), **mut)
    need = getattr(lib, companion)(*[base[a] for a in argnames.split()])
    assert need > 0
    expect(lib, name, dict(mut, workspace_bytes=need), ELAUNCH)
    expect(lib, name, dict(mut, workspace_bytes=need - 1), EWORKSPACE, b"workspace")
    expect(lib, name, dict(mut, workspace_bytes=0), EWORKSPACE, b"workspace")
    expect(lib, name, dict(mut, workspace=None), EWORKSPACE, b"workspace")
    if name != "gmlm_wgrad_bf16":                         # the one entry without an empty call; its companion answers 0 below t = 32
        empties = [m for m, _, rc in ROWS[name]["empty"] if rc in (OK, ELAUNCH)]
        assert empties or name == "gmlm_basis_compose_bwd"
        for m in empties:
            assert getattr(lib, companion)(*[dict(base, **m)[a] for a in argnames.split()]) > 0, (name, m)


def test_workspace_rows_cover_every_companion():
    companions = {n for n, (ret, _) in PROTOS.items() if ret == "size_t"}
    assert companions == {ROWS[n]["ws"][0] for n in WS_NAMES}
    assert {n for n in ROWS if "workspace" in [pn for _, pn in PROTOS[n][1]]} == set(WS_NAMES)


@pytest.mark.parametrize("name", [n for n in NAMES if ROWS[n]["empty"]])
def test_nothing_to_do(lib, name):
    """rc = GMLM_OK without a device proves that nothing was launched; the empty calls that owe an output its zeros launch."""
    for mut, keep, rc in ROWS[name]["empty"]:
        expect(lib, name, mut, rc, None, only=set(keep))


def test_host_only_entry_points(lib):
    cl, cc = C.c_int64(-1), C.c_int64(-1)
    assert lib.gmlm_split_plan_capacity(10, 4, C.byref(cl), C.byref(cc)) == OK and (cl.value, cc.value) == (3, 5)
    assert lib.gmlm_split_plan_capacity(10, 0, C.byref(cl), C.byref(cc)) == EINVAL
    assert lib.gmlm_split_plan_capacity(-1, 4, C.byref(cl), C.byref(cc)) == EINVAL
    assert lib.gmlm_split_plan_capacity(10, 4, None, C.byref(cc)) == EINVAL and lib.gmlm_split_plan_capacity(10, 4, C.byref(cl), None) == EINVAL
    assert lib.gmlm_version() == 1
