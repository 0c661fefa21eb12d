"""The attention dispatch matrix: every reachable instantiation of the head-dim-64 / 96 / 128 attention kernels
(attn_kernels.hip, attn_fwd_pipe.hip, attn_bwd_pipe.hip, attn_short.hip, attn_d128.hip) run at least once through the ops
layer against dense float64 attention, with the instantiations that really ran read back by name from the profiler.

``CASES`` names, per case, the EXACT set of attention kernels the forward and the backward launch; ``UNREACHABLE`` lists the
compiled instantiations the host dispatch (gmlm_attention_fwd / gmlm_attention_bwd, attn_kernels.hip) cannot select.  Their
union must equal the attention kernels of the built library (tests/test_attention_matrix_cpu.py), so a new instantiation
without a parity case, or a stale entry here, fails the CPU suite.

Cases sit on both sides of every dispatch threshold: b*h = 511 / 512 (short sequences), rows 128 / 129 (short -> pipelined),
rows 2047 / 2048 and ceil(rows / 256) * b*h = 504 / 512 (8 waves: at 2,048 rows the product moves in steps of 8),
ceil(rows / 128) * b*h = 1023 / 1024 (4 waves) and max(lq, lk) rounding to R = 32 / 64 / 96 / 128 (short kernels).

Dropout masks come only from helpers.attn_dropout_scale, the independent restatement of the kernels' hash; the slab of a
(batch, head) is (b*h + head) * lq when padded and head * total_rows + cu[seq] when packed (seq_view, attn_common.hpp).  A
forward and a backward from different kernel families must therefore draw the same mask to pass."""
import zlib
from dataclasses import dataclass

import pytest
import torch

from helpers import _close, _dense_reference, attn_dropout_scale, kernels_run

pytestmark = pytest.mark.gpu

BF, F32 = "unsigned short", "float"          # bf16 is an unsigned short in the kernels' template ids


def _b(drop):
    return "true" if drop else "false"


def fwd(t, d, nw, dr):
    return f"attn_fwd_kernel<{t}, {d}, {nw}, {_b(dr)}>"


def dq(t, d, nw, dr):
    return f"attn_bwd_dq_kernel<{t}, {d}, {nw}, {_b(dr)}>"


def dkv(t, d, nw, dr, qt=32):
    return f"attn_bwd_dkv_kernel<{t}, {d}, {nw}, {_b(dr)}, {qt}>"


def delta(t):
    return f"attn_delta_kernel<{t}>"


def pfwd(d, nw, dr):
    return f"attn_fwd_pipe_kernel<{d}, {nw}, {_b(dr)}, 2>"


def pdq(d, nw, dr):
    return f"attn_bwd_dq_pipe_kernel<{d}, {nw}, {_b(dr)}>"


def pdkv(d, nw, dr):
    return f"attn_bwd_dkv_pipe_kernel<{d}, {nw}, {_b(dr)}>"


def sfwd(r, dr):
    return f"attn_fwd_short_kernel<64, {_b(dr)}, {r}>"


def sbwd(r, dr):
    return f"attn_bwd_short_kernel<64, {_b(dr)}, {r}>"


def d128(kind, t, dr=None):
    return f"d128::{kind}_kernel<{t}>" if dr is None else f"d128::{kind}_kernel<{t}, {_b(dr)}>"


def d128_bwd(t, dr):
    return {d128("delta", t), d128("dq", t, dr), d128("dkv", t, dr)}


@dataclass(frozen=True)
class Case:
    id: str
    dtype: torch.dtype
    d: int
    b: int                     # batch (padded) or number of sequences (packed)
    h: int
    lq: int                    # rows per sequence (padded) or total rows (packed)
    lk: int
    mode: str                  # "pad", "kvlen" (padded + kv_len), "packed" (cu_seqlens), "groups" (+ pack_sequence_groups)
    fwd: frozenset
    bwd: frozenset
    lens: tuple = ()           # kv_len per batch ("kvlen") or sequence lengths ("packed", "groups")
    p: float = 0.0
    layout: str = "contig"     # "contig" q / k / v, or "fused": column slices of one [b, l, 3hd] buffer (forward and backward)
    seed_dev: bool = False     # ops.SEED_DEVICE set: the kernels add a device counter to the host seed


def _kv(b, lk, tile):
    """Key lengths of a padded batch: all, 1, one past a tile boundary, none, one more than lk (clamped by the kernels),
    then a deterministic spread over [1, lk]."""
    head = (lk, 1, tile + 1, 0, lk + 7)
    return tuple(head[:b]) + tuple(1 + (37 * i + 11) % lk for i in range(b - len(head)))


def _packed(lens, h, **kw):
    return dict(b=len(lens), h=h, lq=sum(lens), lk=sum(lens), lens=tuple(lens), **kw)


# ragged packed lengths: 1, 31 / 32 / 33 and 127 / 128 around the 32-row blocks, the rest spread over [1, 128]
_SHORT_LENS = (1, 31, 32, 33, 127, 128) + tuple(1 + (53 * i + 7) % 128 for i in range(58))
# 14 consecutive one- to four-row sequences: the 13-sequence limit of a group, not its 128 rows, forces the split
_GROUP_LENS = (128, 1, 31, 32, 33, 127) + tuple(1 + i % 4 for i in range(14)) + tuple(1 + (29 * i + 3) % 128 for i in range(44))
_LONG_LENS = (1, 31, 32, 33, 127, 128, 129, 300)


def _case(id_, dtype, d, fwd_set, bwd_set, **kw):
    return Case(id=id_, dtype=dtype, d=d, fwd=frozenset(fwd_set), bwd=frozenset(bwd_set), **kw)


def _generic(t, d, nw, nwk, dr, qt=32):
    """forward / backward sets of the register-staged kernels (nwk: waves of the dK/dV kernel)"""
    return {fwd(t, d, nw, dr)}, {delta(t), dq(t, d, nw, dr), dkv(t, d, nwk, dr, qt)}


bf, f32 = torch.bfloat16, torch.float32
CASES = [
    # ---- fp32, register-staged kernels: 2 waves (grid under-fills the chip), 4 waves, 8 waves (>= 2048 rows) ----
    _case("f32_d64_w2_kvlen_fused", f32, 64, *_generic(F32, 64, 2, 2, False), b=5, h=2, lq=200, lk=200, mode="kvlen",
          lens=_kv(5, 200, 64), layout="fused"),
    _case("f32_d64_w2_drop_seeddev", f32, 64, *_generic(F32, 64, 2, 2, True), b=5, h=2, lq=200, lk=200, mode="kvlen",
          lens=_kv(5, 200, 32), p=0.3, seed_dev=True),
    _case("f32_d96_w2_cross", f32, 96, *_generic(F32, 96, 2, 2, False), b=2, h=3, lq=150, lk=230, mode="pad"),
    _case("f32_d96_w2_cross_drop", f32, 96, *_generic(F32, 96, 2, 2, True), b=5, h=3, lq=150, lk=230, mode="kvlen",
          lens=_kv(5, 230, 64), p=0.3),
    _case("f32_d64_bh1023_w2", f32, 64, *_generic(F32, 64, 2, 2, False), b=31, h=33, lq=128, lk=128, mode="pad"),
    _case("f32_d64_bh1024_w4", f32, 64, *_generic(F32, 64, 4, 4, False), b=64, h=16, lq=128, lk=128, mode="pad"),
    _case("f32_d64_bh1024_w4_drop", f32, 64, *_generic(F32, 64, 4, 4, True), b=64, h=16, lq=100, lk=128, mode="kvlen",
          lens=_kv(64, 128, 32), p=0.1),
    _case("f32_d96_w4", f32, 96, *_generic(F32, 96, 4, 4, False), b=128, h=4, lq=250, lk=250, mode="pad"),
    _case("f32_d96_w4_drop", f32, 96, *_generic(F32, 96, 4, 4, True), b=128, h=4, lq=250, lk=250, mode="kvlen",
          lens=_kv(128, 250, 64), p=0.3),
    _case("f32_d64_L2048_bh63_w2", f32, 64, *_generic(F32, 64, 2, 2, False), b=9, h=7, lq=2048, lk=2048, mode="pad"),
    _case("f32_d64_L2048_bh64_w8", f32, 64, *_generic(F32, 64, 8, 8, False), b=8, h=8, lq=2048, lk=2048, mode="pad"),
    _case("f32_d64_L2048_w8_drop", f32, 64, *_generic(F32, 64, 8, 8, True), b=8, h=8, lq=2048, lk=2048, mode="kvlen",
          lens=_kv(8, 2048, 64), p=0.3),
    # fp32 d = 96 at 8 waves: the dK/dV kernel stays at 4 waves (512 threads would spill)
    _case("f32_d96_w8", f32, 96, *_generic(F32, 96, 8, 4, False), b=8, h=8, lq=2100, lk=2100, mode="pad"),
    _case("f32_d96_w8_drop", f32, 96, *_generic(F32, 96, 8, 4, True), b=8, h=8, lq=2100, lk=2100, mode="kvlen",
          lens=_kv(8, 2100, 64), p=0.3),
    _case("f32_d64_packed_drop", f32, 64, *_generic(F32, 64, 2, 2, True), mode="packed", p=0.3, **_packed(_LONG_LENS, 2)),
    # ---- bf16 d = 64 beyond 128 rows: pipelined forward + register-staged backward (two families, one mask) ----
    _case("bf16_d64_L2048_w8", bf, 64, {pfwd(64, 4, False)}, {delta(BF), dq(BF, 64, 8, False), dkv(BF, 64, 8, False, 64)},
          b=8, h=8, lq=2048, lk=2048, mode="pad"),
    _case("bf16_d64_L2048_w8_drop", bf, 64, {pfwd(64, 4, True)}, {delta(BF), dq(BF, 64, 8, True), dkv(BF, 64, 8, True, 64)},
          b=8, h=8, lq=2048, lk=2048, mode="kvlen", lens=_kv(8, 2048, 64), p=0.3),
    _case("bf16_d64_L2047_w4", bf, 64, {pfwd(64, 4, False)}, {delta(BF), dq(BF, 64, 4, False), dkv(BF, 64, 4, False, 64)},
          b=8, h=8, lq=2047, lk=2047, mode="pad"),
    _case("bf16_d64_L129_bh512", bf, 64, {pfwd(64, 4, False)}, {delta(BF), dq(BF, 64, 4, False), dkv(BF, 64, 4, False, 64)},
          b=64, h=8, lq=129, lk=129, mode="kvlen", lens=_kv(64, 129, 64)),
    _case("bf16_d64_L129_bh512_drop", bf, 64, {pfwd(64, 4, True)}, {delta(BF), dq(BF, 64, 4, True), dkv(BF, 64, 4, True, 64)},
          b=64, h=8, lq=129, lk=129, mode="pad", p=0.3),
    _case("bf16_d64_L200_w2_fused", bf, 64, {pfwd(64, 4, False)}, {delta(BF), dq(BF, 64, 2, False), dkv(BF, 64, 2, False, 64)},
          b=2, h=4, lq=200, lk=200, mode="pad", layout="fused"),
    _case("bf16_d64_L200_w2_drop", bf, 64, {pfwd(64, 4, True)}, {delta(BF), dq(BF, 64, 2, True), dkv(BF, 64, 2, True, 64)},
          b=5, h=4, lq=200, lk=200, mode="kvlen", lens=_kv(5, 200, 64), p=0.3),
    _case("bf16_d64_packed_long_drop", bf, 64, {pfwd(64, 4, True)}, {delta(BF), dq(BF, 64, 2, True), dkv(BF, 64, 2, True, 64)},
          mode="packed", p=0.3, **_packed(_LONG_LENS, 4)),
    # ---- bf16 d = 64, <= 128 query rows, not the short path: register-staged forward ----
    _case("bf16_d64_lq100_lk1000", bf, 64, {fwd(BF, 64, 2, False)}, {delta(BF), dq(BF, 64, 2, False), dkv(BF, 64, 4, False, 128)},
          b=16, h=8, lq=100, lk=1000, mode="kvlen", lens=_kv(16, 1000, 64)),
    _case("bf16_d64_lq100_lk1000_drop", bf, 64, {fwd(BF, 64, 2, True)}, {delta(BF), dq(BF, 64, 2, True), dkv(BF, 64, 4, True, 128)},
          b=16, h=8, lq=100, lk=1000, mode="pad", p=0.3),
    _case("bf16_d64_lq120_lk200_bh1023", bf, 64, {fwd(BF, 64, 2, False)}, {delta(BF), dq(BF, 64, 2, False), dkv(BF, 64, 4, False, 128)},
          b=31, h=33, lq=120, lk=200, mode="pad"),
    _case("bf16_d64_lq120_lk200_bh1024", bf, 64, {fwd(BF, 64, 4, False)}, {delta(BF), dq(BF, 64, 4, False), dkv(BF, 64, 4, False, 128)},
          b=128, h=8, lq=120, lk=200, mode="pad"),
    _case("bf16_d64_lq120_lk200_bh1024_drop", bf, 64, {fwd(BF, 64, 4, True)}, {delta(BF), dq(BF, 64, 4, True), dkv(BF, 64, 4, True, 128)},
          b=128, h=8, lq=120, lk=200, mode="kvlen", lens=_kv(128, 200, 64), p=0.3),
    _case("bf16_d64_L128_bh511", bf, 64, {fwd(BF, 64, 2, False)}, {delta(BF), dq(BF, 64, 2, False), dkv(BF, 64, 2, False, 32)},
          b=73, h=7, lq=128, lk=128, mode="kvlen", lens=_kv(73, 128, 32)),
    _case("bf16_d64_L128_bh511_drop", bf, 64, {fwd(BF, 64, 2, True)}, {delta(BF), dq(BF, 64, 2, True), dkv(BF, 64, 2, True, 32)},
          b=73, h=7, lq=128, lk=128, mode="pad", p=0.3, seed_dev=True),
    # ---- bf16 d = 64 short sequences (b*h >= 512, every sequence <= 128 rows): one fused backward launch ----
    _case("short_R32", bf, 64, {sfwd(32, False)}, {sbwd(32, False)}, b=64, h=8, lq=32, lk=32, mode="pad"),
    _case("short_R32_cross_drop", bf, 64, {sfwd(32, True)}, {sbwd(32, True)}, b=64, h=8, lq=20, lk=32, mode="pad", p=0.3),
    _case("short_R64_L33_fused", bf, 64, {sfwd(64, False)}, {sbwd(64, False)}, b=64, h=8, lq=33, lk=33, mode="pad", layout="fused"),
    _case("short_R64_kvlen_drop_seeddev", bf, 64, {sfwd(64, True)}, {sbwd(64, True)}, b=64, h=8, lq=64, lk=64, mode="kvlen",
          lens=_kv(64, 64, 32), p=0.3, seed_dev=True),
    _case("short_R96_L65_kvlen", bf, 64, {sfwd(96, False)}, {sbwd(96, False)}, b=64, h=8, lq=65, lk=65, mode="kvlen",
          lens=_kv(64, 65, 32)),
    _case("short_R96_cross_drop", bf, 64, {sfwd(96, True)}, {sbwd(96, True)}, b=64, h=8, lq=96, lk=50, mode="pad", p=0.3),
    _case("short_R128_kvlen_bh512", bf, 64, {sfwd(128, False)}, {sbwd(128, False)}, b=64, h=8, lq=128, lk=128, mode="kvlen",
          lens=_kv(64, 128, 32)),
    _case("short_R128_L97_drop", bf, 64, {sfwd(128, True)}, {sbwd(128, True)}, b=64, h=8, lq=97, lk=97, mode="pad", p=0.3),
    _case("short_packed", bf, 64, {sfwd(128, False)}, {sbwd(128, False)}, mode="packed", **_packed(_SHORT_LENS, 8)),
    _case("short_groups_drop", bf, 64, {sfwd(128, True)}, {sbwd(128, True)}, mode="groups", p=0.3, **_packed(_GROUP_LENS, 8)),
    # ---- bf16 d = 96: pipelined forward and backward, 4 waves unless the grid fills the chip twice with 8 ----
    _case("bf16_d96_w4_fused", bf, 96, {pfwd(96, 4, False)}, {delta(BF), pdq(96, 4, False), pdkv(96, 4, False)},
          b=2, h=4, lq=300, lk=300, mode="pad", layout="fused"),
    # kv_len = 2, not 1: with a single valid key the true dK is exactly 0 and the pipelined forward's bf16 probabilities
    # (normalised by the unrounded sum, gmlm_hip.h) leave O = V (1 +- 2^-9), i.e. rounding noise in dK that 300 queries add
    # up past the max-rel budget; the kv_len = 1 edge runs in the other families' cases
    _case("bf16_d96_w4_kvlen", bf, 96, {pfwd(96, 4, False)}, {delta(BF), pdq(96, 4, False), pdkv(96, 4, False)},
          b=5, h=4, lq=300, lk=300, mode="kvlen", lens=(300, 2, 65, 0, 307)),
    _case("bf16_d96_w4_cross_drop_seeddev", bf, 96, {pfwd(96, 4, True)}, {delta(BF), pdq(96, 4, True), pdkv(96, 4, True)},
          b=2, h=4, lq=300, lk=450, mode="pad", p=0.3, seed_dev=True),
    _case("bf16_d96_L2048_w8", bf, 96, {pfwd(96, 8, False)}, {delta(BF), pdq(96, 8, False), pdkv(96, 8, False)},
          b=8, h=8, lq=2048, lk=2048, mode="pad"),
    _case("bf16_d96_L2048_w8_drop", bf, 96, {pfwd(96, 8, True)}, {delta(BF), pdq(96, 8, True), pdkv(96, 8, True)},
          b=8, h=8, lq=2048, lk=2048, mode="kvlen", lens=_kv(8, 2048, 64), p=0.3),
    # ---- head dim 128 (attn_d128.hip): one family per dtype; tests/test_gpu_attention_d128.py holds the larger shapes ----
    _case("d128_bf16", bf, 128, {d128("fwd", BF, False)}, d128_bwd(BF, False), b=5, h=2, lq=150, lk=150, mode="kvlen",
          lens=_kv(5, 150, 64)),
    _case("d128_bf16_drop_seeddev", bf, 128, {d128("fwd", BF, True)}, d128_bwd(BF, True), b=2, h=2, lq=150, lk=190, mode="pad",
          p=0.3, seed_dev=True),
    _case("d128_f32_fused", f32, 128, {d128("fwd", F32, False)}, d128_bwd(F32, False), b=2, h=2, lq=150, lk=150, mode="pad",
          layout="fused"),
    _case("d128_f32_drop", f32, 128, {d128("fwd", F32, True)}, d128_bwd(F32, True), b=5, h=2, lq=150, lk=150, mode="kvlen",
          lens=_kv(5, 150, 32), p=0.3),
]

_R = "the dispatch (gmlm_attention_fwd / _bwd, attn_kernels.hip) never selects it: "
UNREACHABLE = {
    **{fwd(BF, 64, 8, dr): _R + "bf16 d = 64 beyond 128 rows takes attn_fwd_pipe_kernel, and <= 128 rows never give 8 waves"
       for dr in (False, True)},
    **{fwd(BF, 96, nw, dr): _R + "the bf16 d = 96 forward always takes attn_fwd_pipe_kernel"
       for nw in (2, 4, 8) for dr in (False, True)},
    **{dq(BF, 96, nw, dr): _R + "the bf16 d = 96 backward always takes attn_bwd_dq_pipe_kernel"
       for nw in (2, 4, 8) for dr in (False, True)},
    **{dkv(BF, 96, nw, dr): _R + "the bf16 d = 96 backward always takes attn_bwd_dkv_pipe_kernel"
       for nw in (2, 4, 8) for dr in (False, True)},
    **{dkv(F32, 96, 8, dr): _R + "fp32 d = 96 never uses the 8-wave dK/dV kernel (it would spill): 4 waves instead"
       for dr in (False, True)},
    **{dkv(BF, 64, 8, dr): _R + "the bf16 8-wave dK/dV kernel always stages 64 query rows (QT = 64)" for dr in (False, True)},
    **{dkv(BF, 64, 4, dr): _R + "the bf16 4-wave dK/dV kernel stages 128 (<= 128 query rows) or 64 query rows (QT = 128 / 64)"
       for dr in (False, True)},
}


def _is_attention(name):
    return name.startswith("attn_") or name.startswith("d128::")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _budget(dtype, what):
    if dtype == torch.float32:
        return 1e-4, 1e-5
    return (2e-2, 6e-3) if what == "out" else (2e-2, 8e-3)


HOST_SEED, DEVICE_COUNTER = 2 ** 32 - 5, 7         # their 64-bit sum carries into the high word of the seed


@pytest.mark.parametrize("c", CASES, ids=[c.id for c in CASES])
def test_attention_instantiation_vs_dense_fp64(dev, monkeypatch, c):
    from gmlm_amd import ops
    h, d, b, lq, lk = c.h, c.d, c.b, c.lq, c.lk
    hd, scale = h * d, d ** -0.5
    packed = c.mode in ("packed", "groups")
    g = torch.Generator().manual_seed(zlib.crc32(c.id.encode()))
    seed = 0x1234_5678_9ABC
    if c.seed_dev:
        monkeypatch.setattr(ops, "SEED_DEVICE", torch.tensor([DEVICE_COUNTER], dtype=torch.int64, device=dev))
        seed = HOST_SEED
    mask_seed = seed + (DEVICE_COUNTER if c.seed_dev else 0)
    nb = 1 if packed else b
    # inputs rounded to the case's dtype once; the reference reads the same rounded values
    q = torch.randn(nb, lq, hd, generator=g).to(dev, c.dtype)
    k = (torch.randn(nb, lk, hd, generator=g) * 1.5).to(dev, c.dtype)     # scores ~ N(0, 1.5): neither flat nor one-hot
    v = torch.randn(nb, lk, hd, generator=g).to(dev, c.dtype)
    go = torch.randn(nb, lq, hd, generator=g).to(dev, c.dtype)
    kv_len = torch.tensor(c.lens, dtype=torch.int32, device=dev) if c.mode == "kvlen" else None

    if packed:
        qkv = torch.cat([q, k, v], -1)[0].requires_grad_(True)            # [total_rows, 3hd]
        cu = torch.tensor([0] + list(torch.tensor(c.lens).cumsum(0).tolist()), dtype=torch.int32, device=dev)
        groups = None
        if c.mode == "groups":
            bounds = ops.pack_sequence_groups(c.lens).tolist()
            # some group was closed by the 13-sequence limit although its next sequence would still fit in 128 rows
            assert any(e - s_ == 13 and sum(c.lens[s_:e + 1]) <= 128 for s_, e in zip(bounds[:-2], bounds[1:-1]))
            groups = torch.tensor(bounds, dtype=torch.int32, device=dev)
        box = {}
        fwd_k = kernels_run(lambda: box.setdefault("out", ops.AttentionQKV.apply(qkv, None, h, scale, c.p, seed, cu, max(c.lens),
                                                                                 None, groups)))
        out = box["out"]
        bwd_k = kernels_run(lambda: out.backward(go[0]))
        gq, gk, gv = qkv.grad[:, :hd], qkv.grad[:, hd:2 * hd], qkv.grad[:, 2 * hd:]
        outs = [out.detach(), gq, gk, gv]
        ref = [torch.zeros(lq, hd, dtype=torch.float64, device=dev) for _ in range(4)]
        # grouped mode draws the mask of a whole work item: slab head * total_rows + cu[first sequence of the group] and
        # indices relative to the group's first row (gmlm_hip.h, seq_groups); otherwise per sequence (seq_view)
        first = list(range(len(c.lens)))
        if groups is not None:
            gb = groups.tolist()
            first = [gb[j] for j in range(len(gb) - 1) for _ in range(gb[j], gb[j + 1])]
        cul = cu.tolist()
        for s, (r0, n) in enumerate(zip(cul[:-1], c.lens)):
            drop = None
            if c.p:
                g0 = cul[first[s]]
                drop = lambda bi, hi, r0=r0, n=n, g0=g0: attn_dropout_scale(mask_seed, hi * lq + g0, r0 - g0 + n, r0 - g0 + n, c.p,
                                                                            dev)[r0 - g0:, r0 - g0:]
            rs = _dense_reference(q[:, r0:r0 + n], k[:, r0:r0 + n], v[:, r0:r0 + n], go[:, r0:r0 + n], h, scale, None, drop)
            for i in range(4):
                ref[i][r0:r0 + n] = rs[i][0]
        valid = None
    else:
        if c.layout == "fused":
            assert lq == lk
            qkv = torch.cat([q, k, v], -1)
            qi, ki, vi = (qkv[..., i * hd:(i + 1) * hd].requires_grad_(True) for i in range(3))
            assert qi.stride(1) == 3 * hd
        else:
            qi, ki, vi = (t_.clone().requires_grad_(True) for t_ in (q, k, v))
        box = {}
        fwd_k = kernels_run(lambda: box.setdefault("out", ops.Attention.apply(qi, ki, vi, kv_len, h, scale, c.p, seed)))
        out = box["out"]
        bwd_k = kernels_run(lambda: out.backward(go))
        outs = [out.detach(), qi.grad, ki.grad, vi.grad]
        drop = None
        if c.p:
            drop = lambda bi, hi: attn_dropout_scale(mask_seed, (bi * h + hi) * lq, lq, lk, c.p, dev)
        ref = _dense_reference(q, k, v, go, h, scale, None if kv_len is None else kv_len.cpu(), drop)
        valid = None if kv_len is None else torch.arange(lk, device=dev)[None, :] < kv_len[:, None]

    fwd_a, bwd_a = {n for n in fwd_k if _is_attention(n)}, {n for n in bwd_k if _is_attention(n)}
    print(f"\n{c.id}: forward {sorted(fwd_a)}, backward {sorted(bwd_a)}")
    assert fwd_a == set(c.fwd), (sorted(fwd_a), sorted(c.fwd))
    assert bwd_a == set(c.bwd), (sorted(bwd_a), sorted(c.bwd))
    for name, got in zip(("out", "dq", "dk", "dv"), outs):
        assert bool(torch.isfinite(got).all()), name
    if not packed:                                         # where the error sits, batch by batch (read when a budget fails)
        for name, got, r_ in zip(("out", "dq", "dk", "dv"), outs, ref):
            e = [float((got[bi].double() - r_[bi]).abs().max()) / max(float(r_.abs().max()), 1e-300) for bi in range(b)]
            print(f"  {name} per batch max|err| / max|ref|: " + " ".join(f"{x:.1e}" for x in e))
    for name, got, r_ in zip(("out", "dq", "dk", "dv"), outs, ref):
        _close(name, got, r_, *_budget(c.dtype, name))
    if valid is not None:                                  # keys at or past kv_len: no gradient at all
        assert float(outs[2][~valid].abs().sum()) == 0.0 and float(outs[3][~valid].abs().sum()) == 0.0
        for bi in (kv_len == 0).nonzero().flatten().tolist():   # no valid key: zero output, zero dq (d = 128 contract)
            assert float(outs[0][bi].abs().max()) == 0.0 and float(outs[1][bi].abs().max()) == 0.0

