"""Split-K weight-gradient kernel (ops.wgrad_bf16, taken by nn._splitk_wgrad for bf16 -> fp32 at T >= 16384) against fp64 on
the bf16 operands, at the BERT-base and BERT-mini shapes; determinism, hipGraph replay, strided operands and the fallback."""
import pytest
import torch

from gmlm_amd import dense, nn, ops

pytestmark = pytest.mark.gpu

SHAPES = [(2304, 768), (768, 768), (3072, 768), (768, 3072),      # BERT-base: QKV, attention output, FFN in, FFN out
          (768, 256), (256, 256), (1024, 256), (256, 1024)]       # BERT-mini


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _operands(dev, t, n, k, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    dy = (torch.randn(t, n, device=dev, generator=g) * 0.05).bfloat16()
    x = torch.randn(t, k, device=dev, generator=g).bfloat16()
    return dy, x


def _check(out, dy, x):
    exact = dy.double().t() @ x.double()
    bound = dy.double().abs().t() @ x.double().abs()
    assert out.dtype == torch.float32 and out.shape == exact.shape
    err = (out.double() - exact).abs() - 1e-5 * bound
    assert float(err.max()) <= 0.0, float(((out.double() - exact).abs() / bound).max())


@pytest.mark.parametrize("t", [16384, 65536 + 37, 91698])
@pytest.mark.parametrize("n,k", SHAPES)
def test_wgrad_native_vs_fp64(dev, n, k, t):
    dy, x = _operands(dev, t, n, k, n * 7 + k + t)
    # nn sends the BERT-base weights (>= 9 tiles) to the kernel; the BERT-mini ones stay on the library path, the kernel still serves them
    native = n * k >= 9 * 256 * 256
    assert nn._native_wgrad_ok(dy, x, True) == native
    _check(ops.wgrad_bf16(dy, x), dy, x)
    if native:
        assert torch.equal(nn._splitk_wgrad(dy, x, keep_fp32=True), ops.wgrad_bf16(dy, x))


def test_wgrad_bitwise_repeatable(dev):
    dy, x = _operands(dev, 65536 + 37, 2304, 768, 1)
    a = ops.wgrad_bf16(dy, x)
    b = ops.wgrad_bf16(dy, x)
    assert torch.equal(a, b)


def test_wgrad_graph_replay_equals_eager(dev):
    dy, x = _operands(dev, 91698, 768, 768, 2)
    eager = ops.wgrad_bf16(dy, x)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        ops.wgrad_bf16(dy, x)                     # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = ops.wgrad_bf16(dy, x)
    for _ in range(2):
        out.fill_(float("nan"))
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager)


def test_wgrad_strided_column_slice(dev):
    """dy as a column slice of a wider tensor (e.g. the Q part of a fused QKV gradient), x likewise."""
    t = 65536 + 37
    wide, xw = _operands(dev, t, 2304, 1024, 3)
    dy, x = wide[:, 768:1536], xw[:, 256:1024]
    assert dy.stride(0) == 2304 and nn._native_wgrad_ok(dy, x, True)
    out = ops.wgrad_bf16(dy, x)
    _check(out, dy, x)
    assert torch.equal(out, ops.wgrad_bf16(dy.contiguous(), x.contiguous()))


# Small plans (stages = T // 32 token stages of the main kernel, the rest of T is the combine kernel's token tail): slices
# shorter than the 4-deep stage ring (1, 2, 3 stages: the prologue issues fewer than 3 stages and the vmcnt selection takes
# its short branches), the first ring wrap (4, 5) and a second one (9), uneven slices, splits clamped to the stage count,
# the default plan at a small T (one tile: 256 splits clamped to 40 one-stage slices), and non-square tile grids with
# tiles * splits below 8, a multiple of 8 and not a multiple of 8 (the XCD remap's q / r split).
_SMALL_PLANS = [(32 * s, 256, 256, 1) for s in (1, 2, 3, 4, 5, 9)] + [
    (33, 256, 256, 1), (63, 256, 256, 1), (32 * 5 + 31, 256, 256, 1),               # token tail of 1, 31 and 31 rows
    (32 * 7, 256, 256, 3),                                                           # slices of 2, 2, 3 stages
    (32 * 5, 256, 256, 4),                                                           # 1, 1, 1, 2
    (32 * 9 + 17, 256, 256, 2),                                                      # 4, 5 and a 17-row tail
    (32 * 3, 256, 256, 8),                                                           # splits clamped to 3
    (32 * 40 + 5, 256, 256, 0),                                                      # default plan
    (32 * 7 + 5, 256, 512, 3), (32 * 7 + 5, 512, 256, 4),                            # 2 tiles: 6 and 8 workgroups
    (32 * 7 + 5, 768, 512, 1), (32 * 7 + 5, 768, 512, 4), (32 * 7 + 5, 768, 512, 3),  # 6 tiles: 6, 24 and 18 workgroups
]


def _int_operands(dev, t, n, k, seed):
    """Integer-valued bf16 operands, dy in [-3, 3] and x in [-4, 4]: every partial sum is an integer of magnitude at most
    12 t < 2^24, exact in fp32 whatever the order."""
    g = torch.Generator(device=dev).manual_seed(seed)
    dy = torch.randint(-3, 4, (t, n), device=dev, generator=g).bfloat16()
    x = torch.randint(-4, 5, (t, k), device=dev, generator=g).bfloat16()
    assert 12 * t < 2 ** 24
    return dy, x


@pytest.mark.parametrize("t,n,k,splits", _SMALL_PLANS, ids=[f"t{t}_n{n}_k{k}_s{s}" for t, n, k, s in _SMALL_PLANS])
def test_wgrad_small_plans_exact(dev, t, n, k, splits):
    dy, x = _int_operands(dev, t, n, k, 1000 * t + n + k + splits)
    exact = (dy.double().t() @ x.double()).float()
    out = ops.wgrad_bf16(dy, x, splits)
    assert out.dtype == torch.float32 and torch.equal(out, exact), int((out != exact).sum())
    plain = ops.wgrad_bf16(dy, x, splits, ops.WGRAD_NO_REMAP)
    assert torch.equal(plain, exact)
    # Gaussian data: a mistake that integer data happens to mask; the plain order adds the same partials in the same order
    dy, x = _operands(dev, t, n, k, 7 * t + n + k + splits)
    out = ops.wgrad_bf16(dy, x, splits)
    _check(out, dy, x)
    assert torch.equal(ops.wgrad_bf16(dy, x, splits, ops.WGRAD_NO_REMAP), out)


def test_wgrad_small_plan_strided_and_poisoned(dev):
    """Column slices of wider tensors at 16-byte-aligned nonzero offsets, a workspace full of NaN (the header: 'no
    initialisation needed'), output rows padded by four columns that must stay as they were; two slices of 2 and 3 stages,
    then the default plan (2 tiles -> 128 splits, clamped to 5 one-stage slices), each with a 7-row token tail."""
    from gmlm_amd._lib import check, lib
    t, n, k = 32 * 5 + 7, 512, 256
    wide, xw = _int_operands(dev, t, n + 72, k + 24, 11)
    dy, x = wide[:, 40:40 + n], xw[:, 8:8 + k]
    assert dy.stride(0) == n + 72 and x.stride(0) == k + 24 and dy.data_ptr() % 16 == 0 and x.data_ptr() % 16 == 0
    exact = (dy.double().t() @ x.double()).float()
    sentinel = -12345.0
    for splits, flags in ((2, 0), (2, ops.WGRAD_NO_REMAP), (0, 0)):
        ld_out = k + 4
        out = torch.full((n, ld_out), sentinel, dtype=torch.float32, device=dev)
        nbytes = lib().gmlm_wgrad_workspace_bytes(t, n, k, splits)
        assert nbytes == (splits or 5) * n * k * 4
        ws = torch.full((nbytes // 4,), float("nan"), dtype=torch.float32, device=dev)
        check(lib().gmlm_wgrad_bf16(dy.data_ptr(), dy.stride(0), x.data_ptr(), x.stride(0), t, n, k, splits, out.data_ptr(), ld_out,
                                    flags, ws.data_ptr(), nbytes, torch.cuda.current_stream().cuda_stream), "gmlm_wgrad_bf16")
        assert torch.equal(out[:, :k], exact), (splits, flags, int((out[:, :k] != exact).sum()))
        assert bool((out[:, k:] == sentinel).all()), "the padding columns of the output rows were written"


@pytest.mark.parametrize("case", ["ragged_n", "short_t", "fp32", "bf16_result", "one_tile"])
def test_wgrad_unsupported_falls_back(dev, case):
    t, n, k = (4096 + 5, 768, 768) if case == "short_t" else (16384 + 3, 96 if case == "ragged_n" else 768, 768)
    if case == "one_tile":
        n, k = 256, 256
    dy, x = _operands(dev, t, n, k, 4)
    keep = case != "bf16_result"
    if case == "fp32":
        dy, x = dy.float(), x.float()
    assert not nn._native_wgrad_ok(dy, x, keep)
    out = nn._splitk_wgrad(dy, x, keep_fp32=keep)
    exact = dy.double().t() @ x.double()
    tol = 2 ** -7 if case == "bf16_result" else 1e-4
    assert float((out.double() - exact).abs().max()) <= tol * float(exact.abs().max())


def test_wgrad_switch_selects_library_path(dev):
    dy, x = _operands(dev, 16384, 768, 768, 5)
    try:
        dense.NATIVE_WGRAD = False
        assert not nn._native_wgrad_ok(dy, x, True)
        _check(nn._splitk_wgrad(dy, x, keep_fp32=True), dy, x)
    finally:
        dense.NATIVE_WGRAD = True
