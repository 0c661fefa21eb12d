"""Split-K weight-gradient kernel (ops.wgrad_bf16, taken by nn._splitk_wgrad for bf16 -> fp32 at T >= 16384) against fp64 on
the bf16 operands, at the BERT-base and BERT-mini shapes; determinism, hipGraph replay, strided operands and the fallback."""
import pytest
import torch

from gmlm_amd import nn, ops

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
        nn.NATIVE_WGRAD = False
        assert not nn._native_wgrad_ok(dy, x, True)
        _check(nn._splitk_wgrad(dy, x, keep_fp32=True), dy, x)
    finally:
        nn.NATIVE_WGRAD = True
