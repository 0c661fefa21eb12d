"""Host side of the wide-encoder kernels (no GPU needed): the fifth header (include/gmlm_hip_wide.h), its ctypes table and the
exported symbols agree type by type; the entry points decide every documented refusal, the workspace boundary and the
nothing-to-do cases before any launch; the older entry points keep their limits; ``nn.attention_wide_dim`` pads to the next
native head dim and ``CrossAttention`` takes that route above head dim 128 only."""
import os

import pytest
import torch

from conftest import ROOT
from gmlm_amd import _lib
from test_abi_contract_cpu import parse_header, signature_mismatches

OK, EINVAL, EWORKSPACE, ELAUNCH = 0, -1, -2, -3
F32, BF16 = 0, 1
A = 0x10000000        # fabricated, non-null, 16-byte aligned: every call below ends before or at the launch

no_device = pytest.mark.skipif(torch.cuda.device_count() > 0,
                               reason="fabricated addresses: only meaningful (and only safe) without a device")

NAMES = ["gmlm_attention_wide_bwd", "gmlm_attention_wide_bwd_workspace_bytes", "gmlm_attention_wide_fwd",
         "gmlm_bias_res_layernorm_wide_bwd", "gmlm_bias_res_layernorm_wide_bwd_workspace_bytes", "gmlm_bias_res_layernorm_wide_fwd"]


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libgmlm_hip.so not built")
    return _lib.lib()


def _protos():
    return parse_header(open(os.path.join(ROOT, "include", "gmlm_hip_wide.h")).read())


# ------------------------------------------------------------------------------------------------------------------ ABI
def test_header_ctypes_table_and_exports_agree(lib):
    protos = _protos()
    assert sorted(protos) == NAMES
    assert not signature_mismatches(protos, _lib.SIGNATURES_WIDE)
    for name in protos:
        assert hasattr(lib, name), f"{name} declared in include/gmlm_hip_wide.h but not exported"
    assert not set(_lib.SIGNATURES_WIDE) & (set(_lib.SIGNATURES) | set(_lib.SIGNATURES_SPLIT) | set(_lib.SIGNATURES_OPTIM) |
                                            set(_lib.SIGNATURES_D32))


# ------------------------------------------------------------------------------------------------------------ attention
_ATT = dict(q=A, k=A, v=A, kv_len=None, b=1, h=8, lq=64, lk=64, d=256, q_stride=2048, k_stride=2048, v_stride=2048, scale=0.0625,
            dropout_p=0.0, seed=1, seed_dev=None, out=A, out_lo=None, lse=A, dtype=BF16, stream=None, dout=A, dq=A, dk=A, dv=A,
            dq_stride=2048, dk_stride=2048, dv_stride=2048, workspace=A, workspace_bytes=1 << 40)
_FWD = "q k v kv_len b h lq lk d q_stride k_stride v_stride scale dropout_p seed seed_dev out out_lo lse dtype stream".split()
_BWD = ("q k v out out_lo dout lse kv_len b h lq lk d q_stride k_stride v_stride scale dropout_p seed seed_dev dq dk dv dq_stride "
        "dk_stride dv_stride dtype workspace workspace_bytes stream").split()


def _att(lib, which, **mut):
    a = dict(_ATT, **mut)
    fn, names = (lib.gmlm_attention_wide_fwd, _FWD) if which == "fwd" else (lib.gmlm_attention_wide_bwd, _BWD)
    return fn(*[a[n] for n in names]), lib.gmlm_last_error()


def test_argument_lists_follow_the_header():
    protos = _protos()
    assert [n for _, n in protos["gmlm_attention_wide_fwd"][1]] == _FWD
    assert [n for _, n in protos["gmlm_attention_wide_bwd"][1]] == _BWD
    assert [n for _, n in protos["gmlm_bias_res_layernorm_wide_fwd"][1]] == _LN_FWD
    assert [n for _, n in protos["gmlm_bias_res_layernorm_wide_bwd"][1]] == _LN_BWD


_ATT_REFUSALS = [
    (dict(d=128), b"head dim"), (dict(d=64), b"head dim"), (dict(d=320), b"head dim"), (dict(d=640), b"head dim"),
    (dict(dtype=2), b"dtype"), (dict(dtype=-1), b"dtype"),
    (dict(dropout_p=1.0), b"[0,1)"), (dict(dropout_p=-0.1), b"[0,1)"),
    (dict(scale=0.0), b"scale"), (dict(scale=-1.0), b"scale"),
    (dict(b=-1), b"bad sizes"), (dict(h=0), b"bad sizes"), (dict(lq=-1), b"bad sizes"), (dict(lk=-1), b"bad sizes"),
    (dict(q_stride=2040), b"stride"),                                   # below h * d
    (dict(q_stride=2052), b"stride"),                                   # bf16: not a multiple of 8 elements
    (dict(dtype=F32, k_stride=2050), b"stride"),                        # fp32: not a multiple of 4 elements
    (dict(v_stride=1 << 24), b"stride"),
    (dict(q=A + 8), b"aligned"), (dict(k=None), b"null"), (dict(v=A + 4, dtype=F32), b"aligned"),
    (dict(out_lo=A, dtype=F32), b"out_lo"), (dict(out_lo=A + 8), b"out_lo"),
    (dict(b=1 << 28, lq=1, lk=1), b"too many work items"),              # 2^31 work items of one 32-row tile
    (dict(b=1 << 31, h=1, lq=1, lk=1, q_stride=256, k_stride=256, v_stride=256), b"too many work items"),
]


@no_device
@pytest.mark.parametrize("which", ["fwd", "bwd"])
@pytest.mark.parametrize("mut,msg", _ATT_REFUSALS, ids=[",".join(f"{k}={v}" for k, v in m.items()) for m, _ in _ATT_REFUSALS])
def test_attention_refusals_are_decided_on_the_host(lib, which, mut, msg):
    rc, err = _att(lib, which, **mut)
    assert rc == EINVAL and msg in err, (mut, rc, err)


@no_device
def test_valid_attention_calls_reach_the_launch(lib):
    """Without a device a call that passes validation ends in GMLM_ELAUNCH: the three head dims, both dtypes, kv_len, out_lo,
    lq != lk, the largest admissible grid, and the row strides of a fused K|V buffer."""
    for which in ("fwd", "bwd"):
        for mut in (dict(), dict(dtype=F32), dict(d=384, q_stride=3072, k_stride=3072, v_stride=3072, dq_stride=3072, dk_stride=3072,
                                                  dv_stride=3072),
                    dict(d=512, q_stride=4096, k_stride=4096, v_stride=4096, dq_stride=4096, dk_stride=4096, dv_stride=4096),
                    dict(kv_len=A), dict(out_lo=A), dict(lq=70, lk=200), dict(b=(1 << 28) - 1, lq=1, lk=1),
                    dict(k_stride=4096, v_stride=4096, v=A + 4096)):
            rc, err = _att(lib, which, **mut)
            assert rc == ELAUNCH, (which, mut, rc, err)


@no_device
def test_attention_backward_only_refusals(lib):
    for mut, msg in ((dict(dq_stride=2040), b"dq"), (dict(dk=A + 8), b"dk"), (dict(dv=None), b"dv"), (dict(dout=None), b"out/dout/lse"),
                     (dict(lse=None), b"out/dout/lse"), (dict(out=A + 4), b"out/dout/lse"),
                     (dict(lq=0), b"empty query or key set"), (dict(lk=0), b"empty query or key set")):
        rc, err = _att(lib, "bwd", **mut)
        assert rc == EINVAL and msg in err, (mut, rc, err)


@no_device
def test_attention_workspace_boundary(lib):
    need = lib.gmlm_attention_wide_bwd_workspace_bytes(2, 8, 300)
    assert need == 2 * 8 * 300 * 4
    assert lib.gmlm_attention_wide_bwd_workspace_bytes(0, 8, 0) > 0                       # an empty problem still has a size
    shape = dict(b=2, lq=300, lk=300)
    assert _att(lib, "bwd", workspace_bytes=need, **shape)[0] == ELAUNCH
    rc, err = _att(lib, "bwd", workspace_bytes=need - 1, **shape)
    assert rc == EWORKSPACE and b"workspace" in err
    assert _att(lib, "bwd", workspace=None, **shape)[0] == EWORKSPACE


@no_device
def test_attention_nothing_to_do_needs_no_pointer_but_sizes_are_still_checked(lib):
    nothing = dict(q=None, k=None, v=None, out=None, lse=None, dout=None, dq=None, dk=None, dv=None, workspace=None, workspace_bytes=0)
    for empty in (dict(b=0), dict(lq=0, lk=0)):
        for which in ("fwd", "bwd"):
            assert _att(lib, which, **nothing, **empty)[0] == OK, (which, empty)
            rc, err = _att(lib, which, **nothing, **empty, d=128)
            assert rc == EINVAL and b"head dim" in err
    assert _att(lib, "fwd", **nothing, lq=0)[0] == OK                                     # the forward has no query row to write
    assert _att(lib, "fwd", k=None, v=None, lk=0)[0] == ELAUNCH                           # no key: k / v are not needed


# ------------------------------------------------------------------------------------------------------------ LayerNorm
_LN = dict(x=A, bias=A, residual=A, gamma=A, beta=A, rows=5, f=2560, eps=1e-5, act=0, dropout_p=0.0, seed=1, seed_dev=None, y=A,
           mean=A, rstd=A, dtype=BF16, stream=None, dy=A, dx=A, dresidual=A, dgamma=A, dbeta=A, dbias=A, workspace=A,
           workspace_bytes=1 << 40)
_LN_FWD = "x bias residual gamma beta rows f eps act dropout_p seed seed_dev y mean rstd dtype stream".split()
_LN_BWD = ("dy x bias residual gamma beta mean rstd rows f act dropout_p seed seed_dev dx dresidual dgamma dbeta dbias dtype workspace "
           "workspace_bytes stream").split()


def _ln(lib, which, **mut):
    a = dict(_LN, **mut)
    fn, names = (lib.gmlm_bias_res_layernorm_wide_fwd, _LN_FWD) if which == "fwd" else (lib.gmlm_bias_res_layernorm_wide_bwd, _LN_BWD)
    return fn(*[a[n] for n in names]), lib.gmlm_last_error()


_LN_REFUSALS = [
    (dict(f=1024), b"row width"), (dict(f=768), b"row width"), (dict(f=4104), b"row width"), (dict(f=8192), b"row width"),
    (dict(f=2052), b"row width"),                                       # bf16: not a multiple of 8
    (dict(f=2050, dtype=F32), b"row width"),                            # fp32: not a multiple of 4
    (dict(f=0), b"bad sizes"), (dict(rows=-1), b"bad sizes"),
    (dict(dtype=2), b"dtype"), (dict(dropout_p=1.0), b"[0,1)"), (dict(dropout_p=-0.5), b"[0,1)"),
    (dict(x=None), b"null"), (dict(gamma=None), b"null"), (dict(beta=None), b"null"),
    (dict(x=A + 8), b"alignment"), (dict(residual=A + 4), b"alignment"), (dict(bias=A + 4), b"alignment"),
    (dict(gamma=A + 8), b"alignment"), (dict(beta=A + 8), b"alignment"),
]


@no_device
@pytest.mark.parametrize("which", ["fwd", "bwd"])
@pytest.mark.parametrize("mut,msg", _LN_REFUSALS, ids=[",".join(f"{k}={v}" for k, v in m.items()) for m, _ in _LN_REFUSALS])
def test_layernorm_refusals_are_decided_on_the_host(lib, which, mut, msg):
    rc, err = _ln(lib, which, **mut)
    assert rc == EINVAL and msg in err, (mut, rc, err)


@no_device
def test_layernorm_direction_specific_refusals(lib):
    for which, mut, msg in (("fwd", dict(y=None), b"null"), ("fwd", dict(y=A + 8), b"alignment"), ("bwd", dict(dy=None), b"null"),
                            ("bwd", dict(dx=None), b"null"), ("bwd", dict(mean=None), b"null"), ("bwd", dict(rstd=None), b"null"),
                            ("bwd", dict(dy=A + 8), b"alignment"), ("bwd", dict(dx=A + 4), b"alignment"),
                            ("bwd", dict(dresidual=A + 8), b"alignment")):
        rc, err = _ln(lib, which, **mut)
        assert rc == EINVAL and msg in err, (which, mut, rc, err)


@no_device
def test_valid_layernorm_calls_reach_the_launch(lib):
    """Both ends of the width range in both dtypes, every optional operand absent, GELU and dropout."""
    for which in ("fwd", "bwd"):
        for mut in (dict(), dict(dtype=F32, f=1028), dict(f=1032), dict(f=4096), dict(dtype=F32, f=4096), dict(dtype=F32, f=4092),
                    dict(bias=None, residual=None, dresidual=None, dbias=None), dict(act=1, dropout_p=0.3),
                    dict(mean=None, rstd=None) if which == "fwd" else dict(dgamma=None, dbeta=None, dbias=None), dict(rows=100000)):
            rc, err = _ln(lib, which, **mut)
            assert rc == ELAUNCH, (which, mut, rc, err)


@no_device
def test_layernorm_workspace_boundary_and_empty_calls(lib):
    wsb = lib.gmlm_bias_res_layernorm_wide_bwd_workspace_bytes
    assert wsb(5, 2560) == 5 * 3 * 2560 * 4 and wsb(100000, 4096) == 256 * 3 * 4096 * 4 and wsb(0, 2048) > 0
    need = wsb(300, 2048)
    assert _ln(lib, "bwd", rows=300, f=2048, workspace_bytes=need)[0] == ELAUNCH
    rc, err = _ln(lib, "bwd", rows=300, f=2048, workspace_bytes=need - 1)
    assert rc == EWORKSPACE and b"workspace" in err
    assert _ln(lib, "bwd", workspace=None)[0] == EWORKSPACE
    nothing = dict(x=None, bias=None, residual=None, gamma=None, beta=None, y=None, mean=None, rstd=None, dy=None, dx=None,
                   dresidual=None, dgamma=None, dbeta=None, dbias=None, workspace=None, workspace_bytes=0, rows=0)
    for which in ("fwd", "bwd"):
        assert _ln(lib, which, **nothing)[0] == OK
        rc, err = _ln(lib, which, **nothing, f=1024)
        assert rc == EINVAL and b"row width" in err


# ------------------------------------------------------------------------------------------------ the old entries refuse
@no_device
def test_existing_entry_points_keep_their_limits(lib):
    rc = lib.gmlm_attention_d128_fwd(A, A, A, None, 1, 8, 16, 16, 256, 2048, 2048, 2048, 1.0, 0.0, 0, None, A, None, A, 1, None)
    assert rc == EINVAL and b"head dim" in lib.gmlm_last_error()
    rc = lib.gmlm_bias_res_layernorm_fwd(A, None, None, A, A, 4, 2048, 1e-5, 0, 0.0, 0, None, A, A, A, 1, None)
    assert rc == EINVAL and b"row width" in lib.gmlm_last_error()
    rc = lib.gmlm_bias_res_layernorm_bwd(A, A, None, None, A, A, A, A, 4, 2048, 0, 0.0, 0, None, A, None, A, A, None, 1, A, 1 << 30, None)
    assert rc == EINVAL and b"row width" in lib.gmlm_last_error()


# --------------------------------------------------------------------------------------------------------- host routing
@pytest.fixture
def recorded(monkeypatch):
    from gmlm_amd import ops
    calls = []

    def fake(q, k, v, kv_len, num_heads, scale, dropout_p=0.0, training=False):
        calls.append((tuple(q.shape), tuple(k.shape), tuple(v.shape), num_heads, scale))
        return torch.zeros_like(q)

    monkeypatch.setattr(ops, "attention", fake)
    return calls


@pytest.mark.parametrize("d,dp", [(160, 256), (320, 384), (500, 512), (129, 256), (257, 384), (385, 512)])
def test_attention_wide_dim_pads_to_the_next_native_head_dim(recorded, d, dp):
    from gmlm_amd import nn as gnn
    h, n = 2, 5
    q = torch.randn(1, n, h * d)
    k = torch.randn(1, n + 2, h * d)
    out = gnn.attention_wide_dim(q, k, k.clone(), None, h, d ** -0.5, 0.0, False)
    assert out.shape == q.shape
    (qs, ks, vs, heads, scale), = recorded
    assert qs == (1, n, h * dp) and ks == vs == (1, n + 2, h * dp) and heads == h
    assert scale == d ** -0.5                                     # the scale of the TRUE head dim


@pytest.mark.parametrize("d", [256, 384, 512])
def test_attention_wide_dim_passes_native_head_dims_through(recorded, d):
    from gmlm_amd import nn as gnn
    q = torch.randn(1, 3, 2 * d)
    gnn.attention_wide_dim(q, q, q, None, 2, d ** -0.5, 0.0, False)
    assert recorded == [((1, 3, 2 * d),) * 3 + (2, d ** -0.5)]


def test_attention_wide_dim_padding_is_zero_and_cut_back(monkeypatch):
    from gmlm_amd import nn as gnn, ops
    h, d, dp, n = 2, 320, 384, 4
    q = torch.randn(1, n, h * d)

    def fake(qp, kp, vp, *a, **kw):
        q4 = qp.reshape(1, n, h, dp)
        assert float(q4[..., d:].abs().max()) == 0.0 and torch.equal(q4[..., :d].reshape(1, n, h * d), q)
        return qp + 1.0                                            # the padding columns come back as 1: they must be cut

    monkeypatch.setattr(ops, "attention", fake)
    out = gnn.attention_wide_dim(q, q, q, None, h, 1.0, 0.0, False)
    assert torch.equal(out, q + 1.0)


def test_attention_wide_dim_raises_above_512_and_any_dim_above_128(recorded):
    from gmlm_amd import nn as gnn
    q = torch.zeros(1, 3, 2 * 520)
    with pytest.raises(NotImplementedError, match="512"):
        gnn.attention_wide_dim(q, q, q, None, 2, 1.0, 0.0, False)
    q = torch.zeros(1, 3, 2 * 256)
    with pytest.raises(NotImplementedError, match="128"):
        gnn.attention_any_dim(q, q, q, None, 2, 1.0, 0.0, False)
    assert not recorded


def test_cross_attention_takes_the_wide_route_above_head_dim_128_only(monkeypatch):
    from gmlm_amd import nn as gnn
    took = []
    monkeypatch.setattr(gnn, "attention_wide_dim", lambda q, *a, **kw: took.append("wide") or torch.zeros_like(q))
    monkeypatch.setattr(gnn, "attention_any_dim", lambda q, *a, **kw: took.append("any") or torch.zeros_like(q))
    x = torch.randn(1, 3, 2560)
    gnn.CrossAttention(2560)(x, x)
    x = torch.randn(1, 3, 1024)
    gnn.CrossAttention(1024)(x, x)
    assert took == ["wide", "any"]


def test_ring_block_refuses_wide_head_dims():
    from gmlm_amd import ops
    for d in (256, 384, 512):
        q = torch.zeros(1, 4, 8 * d)
        with pytest.raises(NotImplementedError, match="ring"):
            ops.AttentionBlock(8, 1.0).fwd(q, q, q, None, 0)


def test_layernorm_dispatch_names_the_wide_entries_above_1024(monkeypatch):
    """``ops.BiasResLayerNorm`` calls the wide entries for f > 1024 and the K6 entries up to 1,024 (recorded on a fake library)."""
    from gmlm_amd import ops
    assert ops.LN_WIDE_ABOVE == 1024 and ops.ATTN_WIDE_DIMS == (256, 384, 512)
    called = []

    class Fake:
        def __getattr__(self, name):
            def fn(*a):
                called.append(name)
                return 16 if name.endswith("workspace_bytes") else 0
            return fn

    monkeypatch.setattr(ops, "lib", lambda: Fake())
    monkeypatch.setattr(ops, "_cuda", lambda *a: None)
    monkeypatch.setattr(ops, "_stream", lambda: None)
    for f in (1024, 1032, 4096):
        x = torch.randn(2, f, requires_grad=True)
        y = ops.BiasResLayerNorm.apply(x, None, None, torch.ones(f), torch.zeros(f), 1e-5, False, 0.0, 0)
        y.backward(torch.ones_like(y))
    assert called == ["gmlm_bias_res_layernorm_fwd", "gmlm_layernorm_bwd_workspace_bytes", "gmlm_bias_res_layernorm_bwd"] + \
        ["gmlm_bias_res_layernorm_wide_fwd", "gmlm_bias_res_layernorm_wide_bwd_workspace_bytes", "gmlm_bias_res_layernorm_wide_bwd"] * 2


# --------------------------------------------------------------------------------------------------------- code objects
def test_wide_kernels_have_no_private_segment_and_no_packed_fp32():
    """No spill (a zero private segment in every kernel's metadata), no packed-fp32 VALU (DESIGN.md section 5 b), and the
    instantiations are the 58 that profiles/attn_wide_static.json lists: {fwd, dq, dkv} x {bf16, fp32} x {256, 384, 512} x
    {plain, dropout} + 2 delta; LayerNorm forward {bf16, fp32} x {plain, GELU} + backward x {dropout} x {residual}."""
    import re
    import shutil
    import subprocess
    import tempfile
    from test_wgrad_cpu import LLVM, _code_objects
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libgmlm_hip.so not built")
    if not all(os.path.exists(os.path.join(LLVM, t)) for t in ("llvm-readelf", "llvm-objdump", "llvm-objcopy")):
        pytest.skip("ROCm llvm tools not found")
    tmp = tempfile.mkdtemp()
    try:
        private, bodies = {}, {}
        for co in _code_objects(_lib.LIB_PATH, tmp):
            notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", co], check=True, capture_output=True, text=True).stdout
            for m in re.finditer(r"\.name:\s+(_ZN4gmlm(?:4wide|3lnw)\w+)\s+\.private_segment_fixed_size:\s+(\d+)", notes):
                private[m.group(1)] = int(m.group(2))
            dis = subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-d", "--mcpu=gfx950", co], check=True, capture_output=True,
                                 text=True).stdout
            for m in re.finditer(r"^[0-9a-f]+ <(_ZN4gmlm(?:4wide|3lnw)\w+)>:\n(.*?)(?=^[0-9a-f]+ <|\Z)", dis, re.S | re.M):
                bodies[m.group(1)] = m.group(2)
        assert len(private) == 58 and set(private) == set(bodies), (sorted(private), sorted(bodies))
        assert sum("4wide" in n for n in private) == 38
        assert not {n: v for n, v in private.items() if v}, private
        for name, body in bodies.items():
            assert "v_mfma" in body or "delta_kernel" in name or "3lnw" in name, name
            for op in ("v_pk_fma_f32", "v_pk_mul_f32", "v_pk_add_f32"):
                assert op not in body, (name, op)
            assert "scratch_" not in body, name
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
