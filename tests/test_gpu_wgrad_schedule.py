"""The two main-loop schedules of the split-K weight-gradient kernel: the default (two wave groups a phase apart, two
barriers per stage) against ops.WGRAD_ONE_PHASE (one barrier per stage, all waves in lock-step).  Both give every
accumulator the stages of its slice in order, so the results must agree bit for bit; the plans are the smallest at which
the stagger could go wrong (slices shorter than the 4-deep ring, its first and second wrap, uneven slices in one launch)."""
import pytest
import torch

from gmlm_amd import ops
from gmlm_amd._lib import check, lib

pytestmark = pytest.mark.gpu

ONE = ops.WGRAD_ONE_PHASE
PLAIN = ops.WGRAD_NO_REMAP


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _operands(dev, t, n, k, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    dy = (torch.randn(t, n, device=dev, generator=g) * 0.05).bfloat16()
    x = torch.randn(t, k, device=dev, generator=g).bfloat16()
    return dy, x


def _int_operands(dev, t, n, k, seed):
    """Integer-valued bf16 operands, dy in [-3, 3] and x in [-4, 4]: every partial sum is an integer of magnitude at most
    12 t < 2^24, exact in fp32 whatever the order."""
    g = torch.Generator(device=dev).manual_seed(seed)
    dy = torch.randint(-3, 4, (t, n), device=dev, generator=g).bfloat16()
    x = torch.randint(-4, 5, (t, k), device=dev, generator=g).bfloat16()
    assert 12 * t < 2 ** 24
    return dy, x


_IDENTITY_PLANS = [(32 * s, 256, 256, 1) for s in (1, 2, 3, 4, 5, 9)] + [      # below the ring, first wrap, second wrap
    (32 * 7, 256, 256, 3),                                                       # slices of 2, 2, 3 stages
    (32 * 5, 256, 256, 4),                                                       # 1, 1, 1, 2: barrier counts differ per workgroup
    (32 * 9 + 17, 256, 256, 2),                                                  # 4, 5 and a 17-row token tail
    (32 * 7 + 5, 768, 512, 1), (32 * 7 + 5, 768, 512, 3), (32 * 7 + 5, 768, 512, 4),   # 6, 18 and 24 workgroups
    (16384, 2304, 768, 0), (16384, 768, 768, 0), (16384, 3072, 768, 0), (16384, 768, 3072, 0),   # BERT-base, default plan
]


@pytest.mark.parametrize("t,n,k,splits", _IDENTITY_PLANS, ids=[f"t{t}_n{n}_k{k}_s{s}" for t, n, k, s in _IDENTITY_PLANS])
def test_wgrad_schedules_bit_identical(dev, t, n, k, splits):
    dy, x = _operands(dev, t, n, k, 13 * t + n + k + splits)
    two = ops.wgrad_bf16(dy, x, splits)
    assert two.dtype == torch.float32 and bool(torch.isfinite(two).all())
    one = ops.wgrad_bf16(dy, x, splits, ONE)
    assert torch.equal(two, one), int((two != one).sum())
    two_plain, one_plain = ops.wgrad_bf16(dy, x, splits, PLAIN), ops.wgrad_bf16(dy, x, splits, PLAIN | ONE)
    assert torch.equal(two_plain, one_plain), int((two_plain != one_plain).sum())


# the small plans of test_gpu_wgrad.py (which runs them on the default schedule only)
_SMALL_PLANS = [(32 * s, 256, 256, 1) for s in (1, 2, 3, 4, 5, 9)] + [
    (33, 256, 256, 1), (63, 256, 256, 1), (32 * 5 + 31, 256, 256, 1),
    (32 * 7, 256, 256, 3), (32 * 5, 256, 256, 4), (32 * 9 + 17, 256, 256, 2), (32 * 3, 256, 256, 8), (32 * 40 + 5, 256, 256, 0),
    (32 * 7 + 5, 256, 512, 3), (32 * 7 + 5, 512, 256, 4),
    (32 * 7 + 5, 768, 512, 1), (32 * 7 + 5, 768, 512, 4), (32 * 7 + 5, 768, 512, 3),
]


@pytest.mark.parametrize("t,n,k,splits", _SMALL_PLANS, ids=[f"t{t}_n{n}_k{k}_s{s}" for t, n, k, s in _SMALL_PLANS])
def test_wgrad_one_phase_small_plans_exact(dev, t, n, k, splits):
    dy, x = _int_operands(dev, t, n, k, 1000 * t + n + k + splits)
    exact = (dy.double().t() @ x.double()).float()
    out = ops.wgrad_bf16(dy, x, splits, ONE)
    assert out.dtype == torch.float32 and torch.equal(out, exact), int((out != exact).sum())
    plain = ops.wgrad_bf16(dy, x, splits, ONE | PLAIN)
    assert torch.equal(plain, exact), int((plain != exact).sum())


def _launch(dy, x, t, n, k, splits, flags, ws, out):
    check(lib().gmlm_wgrad_bf16(dy.data_ptr(), dy.stride(0), x.data_ptr(), x.stride(0), t, n, k, splits, out.data_ptr(),
                                out.stride(0), flags, ws.data_ptr(), ws.numel() * 4, torch.cuda.current_stream().cuda_stream),
          "gmlm_wgrad_bf16")


@pytest.mark.parametrize("data", ["integer", "gaussian"])
def test_wgrad_two_phase_repeats_into_poisoned_workspace(dev, data):
    """A screen, not a proof (the kernel's header argues the schedule from its barrier rules): ten launches of the default
    schedule back to back, slices of 7, 8 and 8 stages and a 5-row token tail, each into its own workspace full of NaN."""
    t, n, k, splits = 32 * 23 + 5, 768, 512, 3
    dy, x = (_int_operands if data == "integer" else _operands)(dev, t, n, k, 77)
    words = lib().gmlm_wgrad_workspace_bytes(t, n, k, splits) // 4
    assert words == splits * n * k
    wss = [torch.full((words,), float("nan"), dtype=torch.float32, device=dev) for _ in range(10)]
    outs = [torch.full((n, k), float("nan"), dtype=torch.float32, device=dev) for _ in range(10)]
    for ws, out in zip(wss, outs):
        _launch(dy, x, t, n, k, splits, 0, ws, out)
    torch.cuda.synchronize()
    exact = dy.double().t() @ x.double()
    for i, out in enumerate(outs):
        assert torch.equal(out, outs[0]), (i, int((out != outs[0]).sum()))
    if data == "integer":
        assert torch.equal(outs[0], exact.float()), int((outs[0] != exact.float()).sum())
    else:
        # fp32 accumulation of exact products: 2^-24 per addition, t additions at the very worst; 1e-5 is the bound of the
        # fp64 checks in test_gpu_wgrad.py
        bound = dy.double().abs().t() @ x.double().abs()
        assert float(((outs[0].double() - exact).abs() - 1e-5 * bound).max()) <= 0.0
        assert torch.equal(outs[0], ops.wgrad_bf16(dy, x, splits, ONE))


def test_wgrad_schedules_strided_operands(dev):
    """Column slices of wider tensors at 16-byte-aligned nonzero offsets: slices of 2 and 3 stages, then the default plan
    (5 one-stage slices), each with a 7-row token tail; both schedules exact, hence equal."""
    t, n, k = 32 * 5 + 7, 512, 256
    wide, xw = _int_operands(dev, t, n + 72, k + 24, 11)
    dy, x = wide[:, 40:40 + n], xw[:, 8:8 + k]
    assert dy.stride(0) == n + 72 and x.stride(0) == k + 24 and dy.data_ptr() % 16 == 0 and x.data_ptr() % 16 == 0
    exact = (dy.double().t() @ x.double()).float()
    gw, gxw = _operands(dev, t, n + 72, k + 24, 12)
    gdy, gx = gw[:, 40:40 + n], gxw[:, 8:8 + k]
    for splits in (2, 0):
        for flags in (0, PLAIN):
            two, one = ops.wgrad_bf16(dy, x, splits, flags), ops.wgrad_bf16(dy, x, splits, flags | ONE)
            assert torch.equal(two, exact), (splits, flags, int((two != exact).sum()))
            assert torch.equal(one, exact), (splits, flags, int((one != exact).sum()))
            gtwo = ops.wgrad_bf16(gdy, gx, splits, flags)
            assert torch.equal(gtwo, ops.wgrad_bf16(gdy, gx, splits, flags | ONE))
            assert torch.equal(gtwo, ops.wgrad_bf16(gdy.contiguous(), gx.contiguous(), splits, flags))
