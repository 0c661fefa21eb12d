"""bf16x3 without a device: the second header (include/gmlm_hip_split.h) against its ctypes table and the exported symbol, the
argument contract of gmlm_split_bf16x3 on fabricated addresses (the method of test_abi_contract_cpu.py: a call that passes
validation ends in GMLM_ELAUNCH, a refused one in GMLM_EINVAL, an empty one in GMLM_OK), the public option of GraphTextLM, and
the numerical design itself restated in torch: split, three-product GEMM and the operand plan of ops.LinearBf16x3."""
import os

import pytest
import torch
import torch.nn.functional as F

from conftest import ROOT
from test_abi_contract_cpu import ADDR, signature_mismatches, parse_header

OK, EINVAL, ELAUNCH = 0, -1, -3
NAME = "gmlm_split_bf16x3"
no_device = pytest.mark.skipif(torch.cuda.device_count() > 0, reason="fabricated addresses: only meaningful (and only safe) without a device")


def _protos():
    return parse_header(open(os.path.join(ROOT, "include", "gmlm_hip_split.h")).read())


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    import gmlm_amd
    return gmlm_amd.lib()


# --------------------------------------------------------------------------------------------------- header / table / symbol
def test_split_header_table_and_symbol_agree(lib):
    from gmlm_amd import _lib
    protos = _protos()
    assert sorted(protos) == [NAME] == sorted(_lib.SIGNATURES_SPLIT)
    assert not signature_mismatches(protos, _lib.SIGNATURES_SPLIT), signature_mismatches(protos, _lib.SIGNATURES_SPLIT)
    ret, params = protos[NAME]
    assert ret == "int" and [n for _, n in params] == ["x", "ld_x", "rows", "cols", "cols_out", "out", "ld_out", "part_stride", "order", "stream"]
    assert params[0] == ("const float *", "x") and params[5] == ("void *", "out") and params[-1] == ("gmlm_stream_t", "stream")
    assert hasattr(lib, NAME) and getattr(lib, NAME).argtypes == _lib.SIGNATURES_SPLIT[NAME][1]
    # the first header and its table are what they were: the new entry is in neither
    first = parse_header()
    assert NAME not in first and NAME not in _lib.SIGNATURES and sorted(first) == sorted(_lib.SIGNATURES)
    hdr = open(os.path.join(ROOT, "include", "gmlm_hip_split.h")).read()
    assert '#include "gmlm_hip.h"' in hdr and 'extern "C"' in hdr
    mk = open(os.path.join(ROOT, "gmlm_amd", "csrc", "Makefile")).read()
    assert "split_kernels.hip" in mk and "gmlm_hip_split.h" in mk


# ------------------------------------------------------------------------------------------------------ argument contract
# the valid call: 4 rows of 20 columns padded to 24, the parts side by side in one [4, 72] buffer
BASE = dict(x=ADDR(1), ld_x=20, rows=4, cols=20, cols_out=24, out=ADDR(2), ld_out=72, part_stride=24, order=0, stream=None)
STACKED = dict(ld_out=24, part_stride=4 * 24)
ORDER = ["x", "ld_x", "rows", "cols", "cols_out", "out", "ld_out", "part_stride", "order", "stream"]


def _call(lib, **mut):
    args = dict(BASE, **mut)
    rc = getattr(lib, NAME)(*[args[k] for k in ORDER])
    return rc, lib.gmlm_last_error()


def _expect(lib, rc, msg=None, **mut):
    got, err = _call(lib, **mut)
    assert got == rc and (msg is None or msg in err), f"{mut}: code {got} (want {rc}), message {err!r} (want {msg!r})"
    if rc == ELAUNCH:                                     # passed validation: the failure is the missing device, nothing else
        assert b"device" in err.lower() or b"hip" in err.lower(), (mut, err)


@no_device
def test_valid_calls_pass_validation(lib):
    _expect(lib, ELAUNCH)
    _expect(lib, ELAUNCH, order=1)
    _expect(lib, ELAUNCH, **STACKED)                                          # both accepted layouts
    _expect(lib, ELAUNCH, ld_out=80, part_stride=24)                          # side by side with slack behind the third part
    _expect(lib, ELAUNCH, ld_out=32, part_stride=3 * 32 + 24)                 # stacked, strided rows: (rows - 1) ld_out + cols_out
    _expect(lib, ELAUNCH, cols_out=40, ld_out=120, part_stride=40)            # more than one pad chunk
    _expect(lib, ELAUNCH, ld_x=24)                                            # a column slice of a wider matrix
    _expect(lib, ELAUNCH, stream=ADDR(9))
    _expect(lib, ELAUNCH, rows=(1 << 31) // 3 - 1, ld_out=24, part_stride=((1 << 31) // 3 - 1) * 24)   # rows * chunks just below 2^31


@no_device
def test_refusals_name_the_argument(lib):
    for p in ("x", "out"):
        _expect(lib, EINVAL, b"null pointer", **{p: None})
        for shift in (4, 2, 8):
            _expect(lib, EINVAL, b"16-byte aligned", **{p: BASE[p] + shift})
        _expect(lib, ELAUNCH, **{p: BASE[p] + 16})
    _expect(lib, EINVAL, b"ld_x", ld_x=16)                                    # < cols
    _expect(lib, EINVAL, b"ld_x", ld_x=22)                                    # not a multiple of 4
    _expect(lib, EINVAL, b"cols_out", cols_out=16, ld_out=48, part_stride=16)  # < cols
    _expect(lib, EINVAL, b"cols_out", cols_out=20, ld_out=72, part_stride=24)  # not a multiple of 8
    _expect(lib, EINVAL, b"ld_out", ld_out=76)
    _expect(lib, EINVAL, b"part_stride", part_stride=28)
    for order in (2, -1):
        _expect(lib, EINVAL, b"order", order=order)
    for k in ("rows", "cols", "cols_out", "ld_x", "ld_out", "part_stride"):
        _expect(lib, EINVAL, b"negative", **{k: -8})
    _expect(lib, EINVAL, b"2^31", rows=(1 << 31) // 3 + 1, ld_out=24, part_stride=((1 << 31) // 3 + 1) * 24)
    _expect(lib, EINVAL, b"2^31", rows=1 << 62, ld_out=24, part_stride=1 << 40)
    # overlapping parts
    _expect(lib, EINVAL, b"overlapping", part_stride=16)                      # side by side, parts closer than their width
    _expect(lib, EINVAL, b"overlapping", ld_out=64)                           # side by side, the row too short for three parts
    _expect(lib, EINVAL, b"overlapping", ld_out=24, part_stride=3 * 24)       # stacked, one row short
    _expect(lib, EINVAL, b"overlapping", ld_out=16, part_stride=4 * 24)       # stacked, rows narrower than a part
    _expect(lib, EINVAL, b"overlapping", part_stride=0)


@no_device
def test_empty_calls_return_ok_without_pointers(lib):
    _expect(lib, OK, rows=0, x=None, out=None)
    _expect(lib, OK, cols=0, cols_out=0, x=None, out=None)
    _expect(lib, OK, rows=0, part_stride=0, ld_out=0)
    _expect(lib, EINVAL, b"order", rows=0, order=3)                           # sizes and flags are checked before the empty return
    _expect(lib, EINVAL, b"ld_x", rows=0, ld_x=18)
    _expect(lib, ELAUNCH, cols=0)                                             # nothing to read, three parts of zeros to write


# ------------------------------------------------------------------------------------------------------ the public option
def _tiny_model(**kw):
    from transformers import BertConfig, BertModel
    import gmlm_amd
    enc = BertModel(BertConfig(vocab_size=200, hidden_size=64, num_hidden_layers=2, num_attention_heads=4, intermediate_size=128,
                               max_position_embeddings=64))
    return gmlm_amd.GraphTextLM(32, 16, 5, plm_encoder=enc, **kw)


def test_gemm_precision_option():
    import inspect
    import gmlm_amd
    sig = inspect.signature(gmlm_amd.GraphTextLM.__init__)
    assert sig.parameters["gemm_precision"].default == "native" and sig.parameters["gemm_precision"].kind == inspect.Parameter.KEYWORD_ONLY
    native, x3 = _tiny_model(), _tiny_model(gemm_precision="bf16x3")
    assert native.gemm_precision == "native" and x3.gemm_precision == "bf16x3"
    assert sorted(native.state_dict()) == sorted(x3.state_dict())
    for bad in ("bf16", "fp32", "BF16X3", ""):
        with pytest.raises(ValueError, match="gemm_precision"):
            _tiny_model(gemm_precision=bad)
    with pytest.raises(ValueError, match="bf16x3"):
        _tiny_model(gemm_precision="bf16x3", compute_dtype=torch.bfloat16)
    assert _tiny_model(gemm_precision="bf16x3", compute_dtype=torch.float32)._compute_dtype() == torch.float32
    assert native._compute_dtype() == torch.float32 and x3._compute_dtype() == torch.float32
    # torch.amp.autocast("cuda") switches itself off where there is no device, so the state it sets is set directly
    import warnings
    was = torch.is_autocast_enabled("cuda"), torch.get_autocast_dtype("cuda")
    try:
        torch.set_autocast_enabled("cuda", True)
        for dt in (torch.bfloat16, torch.float16):
            torch.set_autocast_dtype("cuda", dt)
            assert x3._compute_dtype() == torch.float32
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")                              # fp16 autocast runs as bf16: said once, elsewhere
                assert native._compute_dtype() == torch.bfloat16            # the native model follows autocast, as before
    finally:
        torch.set_autocast_enabled("cuda", was[0])
        torch.set_autocast_dtype("cuda", was[1])
    with pytest.raises(NotImplementedError, match="bf16x3"):
        x3.capture_hip_graphs(torch.zeros(4, 32), torch.zeros(2, 0, dtype=torch.long))
    assert callable(gmlm_amd.mm_bf16x3)


def test_prepare_weights_refuses_a_bad_mode():
    from transformers import BertConfig, BertModel
    from gmlm_amd import bert
    enc = BertModel(BertConfig(vocab_size=50, hidden_size=32, num_hidden_layers=1, num_attention_heads=2, intermediate_size=64,
                               max_position_embeddings=16))
    with pytest.raises(ValueError, match="gemm_precision"):
        bert.prepare_weights(enc, torch.float32, "tf32")
    with pytest.raises(ValueError, match="float32"):
        bert.prepare_weights(enc, torch.bfloat16, "bf16x3")
    lw = bert.prepare_weights(enc, torch.float32)[0]                         # the default is the fp32 copy of today
    assert isinstance(lw.wqkv, torch.Tensor) and lw.wqkv.dtype == torch.float32 and lw.wqkv.shape == (96, 32)


# --------------------------------------------------------------------------------------- the numerical design, in torch
def _bf(x):
    return x.to(torch.bfloat16).to(torch.float32)


def split_ref(x):
    """(hi, lo) as fp32 tensors holding bf16 values: the contract of gmlm_split_bf16x3."""
    hi = _bf(x)
    lo = torch.where(torch.isfinite(hi), _bf(x - hi), torch.zeros_like(x))
    return hi, lo


def parts(x, order):
    """[rows, 3 cols]: (hi, lo, hi) for order 0, (hi, hi, lo) for order 1."""
    hi, lo = split_ref(x)
    return torch.cat([hi, lo, hi] if order == 0 else [hi, hi, lo], 1)


def mm3(a, b):
    """a @ b^T as the ONE depth-3K GEMM of bf16 values with fp32 accumulation."""
    return parts(a, 1) @ parts(b, 0).t()


class Lin3(torch.autograd.Function):
    """The signature of bf16_emulation._Lin with the three-product form in all three GEMMs and nothing rounded."""

    @staticmethod
    def forward(ctx, x, w, b, round_wgrad, residual):
        ctx.save_for_backward(x, w)
        ctx.has_b = b is not None
        y = mm3(x.reshape(-1, x.shape[-1]), w).view(*x.shape[:-1], w.shape[0])
        if b is not None:
            y = y + b
        return (y, x.clone()) if residual else y

    @staticmethod
    def backward(ctx, dy, dres=None):
        x, w = ctx.saved_tensors
        dy2, x2 = dy.reshape(-1, dy.shape[-1]), x.reshape(-1, x.shape[-1])
        dx = mm3(dy2, w.t().contiguous())
        if dres is not None:
            dx = dx + dres.reshape(dx.shape)
        dw = mm3(dy2.t().contiguous(), x2.t().contiguous())
        return dx.view(x.shape), dw, (dy2.sum(0) if ctx.has_b else None), None, None


def test_three_product_dense_layers_hold_the_fp32_bar_on_the_emulation_model(monkeypatch):
    """Every dense layer of the oracle's emulation model on the three-product form, rounding otherwise off, against the fp32
    oracle in the form of test_bf16_emulation's first test: logits within 1e-4, every non-negligible gradient within 1e-4 of
    its own norm (measured: 1.6e-5 and 2.1e-5)."""
    import bf16_emulation as E
    import gmlm_oracle as O
    from test_bf16_emulation import _case, _grads
    om, x, ei, y, mask, ids, am = _case()
    ref = om(O.soft_masking_gnn_input(x, mask, om.gnn_mask_token_embed, 0.7), ei, ids, am, mask, plm_batch_size=16)
    F.cross_entropy(ref[mask], y[mask], label_smoothing=0.2).backward()
    g32 = _grads(om)
    om.zero_grad(set_to_none=True)
    monkeypatch.setattr(E, "r", lambda t: t)
    monkeypatch.setattr(E, "_Lin", Lin3)
    lg = E.forward(om, x, ei, ids, am, mask)
    F.cross_entropy(lg[mask], y[mask], label_smoothing=0.2).backward()
    ge = _grads(om)
    dl = float((lg - ref).abs().max())
    gmax = max(float(v.norm()) for v in g32.values())
    worst = max(float((ge[k] - b).norm()) / float(b.norm()) for k, b in g32.items() if float(b.norm()) > 1e-6 * gmax)
    print(f"\nthree-product emulation vs fp32 oracle: logits {dl:.2e}, worst gradient {worst:.2e} of its norm")
    assert dl > 0.0, "the patch did not take: the logits are the fp32 oracle's bit for bit"
    assert dl <= 1e-4
    assert set(ge) == set(g32)
    for k, b in g32.items():
        assert float((ge[k] - b).norm()) <= 1e-4 * float(b.norm()) + 1e-7 * gmax, k


def test_operand_plan_against_float64():
    """The plan of ops.LinearBf16x3 at T, K, N = 40, 24, 16: forward X1 @ W0^T, data gradient DY0 @ W1s (stacked), weight gradient
    from the SAME two activation buffers viewed as [3T, .]; each against float64 and against plain bf16 operands."""
    g = torch.Generator().manual_seed(11)
    t, k, n = 40, 24, 16
    x, w, dy = torch.randn(t, k, generator=g), torch.randn(n, k, generator=g) * 0.2, torch.randn(t, n, generator=g)
    x1, w0, dy0 = parts(x, 1), parts(w, 0), parts(dy, 0)
    whi, wlo = split_ref(w)
    w1s = torch.cat([whi, whi, wlo], 0)                                        # [3N, K]: (hi, hi, lo) stacked
    y, dx = x1 @ w0.t(), dy0 @ w1s
    dw = dy0.view(3 * t, n).t() @ x1.view(3 * t, k)                            # rows (hi, lo, hi) against (hi, hi, lo)
    # the views pair what they should: row 3 i + p of the view is part p of row i
    assert torch.equal(dy0.view(3 * t, n)[1::3], split_ref(dy)[1]) and torch.equal(x1.view(3 * t, k)[2::3], split_ref(x)[1])

    def rel(a, b):
        return float((a.double() - b).norm() / b.norm())

    refs = dict(y=(y, x.double() @ w.double().t(), _bf(x) @ _bf(w).t()), dx=(dx, dy.double() @ w.double(), _bf(dy) @ _bf(w)),
                dw=(dw, dy.double().t() @ x.double(), _bf(dy).t() @ _bf(x)))
    for name, (got, ref, plain) in refs.items():
        e3, e1 = rel(got, ref), rel(plain, ref)
        assert e3 <= 2e-5 and e3 <= e1 / 32, (name, e3, e1)                    # 3 * 2^-16 = 4.6e-5 worst case; measured 4.3-4.6e-6


def test_split_reference_edge_values():
    """The restated split at the values the kernel contract names: ties to even in both parities, NaN, infinities, the
    largest finite fp32 (hi rounds to infinity, lo is +0) and signed zeros."""
    big = torch.finfo(torch.float32).max
    x = torch.tensor([1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, float("inf"), -float("inf"), float("nan"), big, -big, 0.0, -0.0, 1.0 + 2.0 ** -9])
    hi, lo = split_ref(x)
    assert hi[0] == 1.0 and lo[0] == 2.0 ** -8                                 # tie, even neighbour below
    assert hi[1] == 1.0 + 2.0 ** -6 and lo[1] == -(2.0 ** -8)                  # tie, even neighbour above
    assert torch.isinf(hi[2]) and torch.isinf(hi[3]) and torch.isnan(hi[4]) and torch.isinf(hi[5]) and hi[6] == -float("inf")
    assert bool((lo[2:7] == 0).all()) and not bool(torch.signbit(lo[2:7]).any())
    assert hi[9] == 1.0 and lo[9] == 2.0 ** -9 and float((hi + lo)[9]) == float(x[9])
    assert bool(((hi + lo)[:2] == x[:2]).all())
