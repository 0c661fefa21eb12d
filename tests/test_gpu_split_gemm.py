"""The bf16x3 split kernel (gmlm::split3, include/gmlm_hip_split.h) bit for bit against torch on the CPU, and dense.mm_bf16x3
(forward, data gradient, weight gradient) against float64 with the elementwise bound that follows from the construction:

    |err_ij| <= (3 * 2^-16 + K' * 2^-23) * (|A| |B|)_ij

|x - hi - lo| <= 2^-16 |x| per operand and the dropped lo*lo term <= 2^-16 |a| |b| give the first part, fp32 accumulation over
the contraction length K' of the GEMM that actually runs (three parts of the zero-padded depth) the second."""
import pytest
import torch

from helpers import kernels_run

pytestmark = pytest.mark.gpu

GUARD = 64                                                   # sentinel elements before and after the output (a multiple of 8)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def up(n, q):
    return (n + q - 1) // q * q


# ----------------------------------------------------------------------------------------------------------- split kernel
BIG = torch.finfo(torch.float32).max
SPECIALS = [float("inf"), float("nan"), BIG, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, -0.0, 0.0, -float("inf"), -BIG,
            -(1.0 + 2.0 ** -8) * 2.0 ** 40, (1.0 + 3 * 2.0 ** -8) * 2.0 ** -60, 1.0 + 2.0 ** -9]


def make_input(rows, cols, seed):
    """Normal values with magnitudes spread over 2^-100 .. 2^100, then signed zeros, infinities, NaN, the largest finite fp32
    (hi rounds to infinity) and exact ties between two bf16 neighbours in both parities at scattered positions."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(rows, cols, generator=g) * torch.exp2(torch.randint(-100, 101, (rows, cols), generator=g).float())
    x = torch.where(x.abs() < 2.0 ** -100, torch.ones_like(x), x)            # lo >= 2^-123 stays a normal number (the contract)
    flat = x.view(-1)
    n = flat.numel()
    step = max(1, n // len(SPECIALS))
    for i, v in enumerate(SPECIALS):
        if i * step < n:
            flat[(i * step + (i * 3) % step) if step > 3 else i * step] = v
    return x


def split_expected(x):
    """(hi, lo) bf16 on the CPU: x.bfloat16() and (x - hi.float()).bfloat16(), lo = +0 where hi is not finite."""
    hi = x.bfloat16()
    lo = (x - hi.float()).bfloat16()
    lo = torch.where(torch.isfinite(hi), lo, torch.zeros_like(lo))
    return hi, lo


def sentinel(n):
    return ((torch.arange(n) % 251) + 0x4000).to(torch.int16)                # bf16 bit patterns of finite values around 2.0


def run_split(dev, xs, cols, cols_out, order, stacked, slack=8):
    """One raw call on a sentinel-filled buffer.  ``xs``: the fp32 source on the device (a view; row stride = its stride(0)).
    Returns (buffer after the call as int16 on the CPU, expected buffer, mask of positions where the expectation is NaN)."""
    from gmlm_amd import ops
    rows = xs.shape[0]
    if stacked:
        ld_out, part_stride = cols_out + slack, rows * (cols_out + slack)
        body = 3 * part_stride
    else:
        ld_out, part_stride = 3 * cols_out + slack, cols_out
        body = rows * ld_out
    buf = sentinel(2 * GUARD + body).to(dev)
    out_ptr = buf.data_ptr() + 2 * GUARD
    ld_x = xs.stride(0) if rows > 1 else up(cols, 4)
    ops.check(ops.lib().gmlm_split_bf16x3(xs.data_ptr(), ld_x, rows, cols, cols_out, out_ptr, ld_out, part_stride, order,
                                          ops._stream()), "gmlm_split_bf16x3")
    hi, lo = split_expected(xs[:, :cols].cpu())
    z = torch.zeros(rows, cols_out - cols, dtype=torch.bfloat16)
    want = sentinel(2 * GUARD + body).view(torch.bfloat16)
    for p, part in enumerate((hi, lo, hi) if order == 0 else (hi, hi, lo)):
        full = torch.cat([part, z], 1)
        for r in range(rows):
            o = GUARD + p * part_stride + r * ld_out
            want[o:o + cols_out] = full[r]
    return buf.cpu(), want.view(torch.int16), torch.isnan(want)


def assert_bits(got, want, nan):
    g = got.view(torch.bfloat16)
    assert bool(torch.isnan(g[nan]).all()), "a NaN of the input did not stay a NaN"
    bad = (got != want) & ~nan
    assert not bool(bad.any()), f"{int(bad.sum())} elements differ, first at {int(bad.nonzero()[0])} of {got.numel()}"


@pytest.mark.parametrize("cols", [8, 20, 768, 2089])
@pytest.mark.parametrize("rows", [1, 3, 257])
def test_split_kernel_bit_for_bit(dev, rows, cols):
    x = make_input(rows, cols, seed=rows * 10007 + cols)
    ld_x = up(cols, 4)
    store = torch.full((rows, ld_x), float("nan"))                            # what lies past `cols` must never be read
    store[:, :cols] = x
    xs = store.to(dev)[:, :cols]
    hi, lo = split_expected(x)
    assert bool((lo[~torch.isfinite(hi)].view(torch.int16) == 0).all())      # +0 wherever hi is not finite (the reference itself)
    for order in (0, 1):
        for stacked in (False, True):
            got, want, nan = run_split(dev, xs, cols, up(cols, 8), order, stacked)
            assert_bits(got, want, nan)
            again, _, _ = run_split(dev, xs, cols, up(cols, 8), order, stacked)
            assert torch.equal(again, got)                                    # a second identical call: identical bytes


def test_split_kernel_wide_padding_and_column_slice(dev):
    """cols_out = cols + 16 (whole chunks of zeros behind the straddling one), and a source that is a column slice of a wider
    matrix (ld_x > cols, the neighbours are NaN)."""
    rows, cols = 3, 20
    x = make_input(rows, cols, seed=5)
    wide = torch.full((rows, 64), float("nan"))
    wide[:, 8:8 + cols] = x
    wd = wide.to(dev)
    for xs in (x.to(dev), wd[:, 8:8 + cols]):
        for order in (0, 1):
            for stacked in (False, True):
                for cols_out in (24, cols + 16 + 4):
                    got, want, nan = run_split(dev, xs, cols, cols_out, order, stacked)
                    assert_bits(got, want, nan)


def test_split_wrapper_layouts_and_unaligned_sources(dev):
    """ops.split_bf16x3: shapes of the two layouts, zero rows behind every stacked part with ``part_rows``, and sources the kernel
    cannot read in place (odd width, odd row stride, transposed) go through one aligned copy."""
    from gmlm_amd import ops
    g = torch.Generator().manual_seed(2)
    for rows, cols in ((5, 13), (12, 16), (1, 7)):
        x = torch.randn(rows, cols, generator=g)
        hi, lo = split_expected(x)
        co = up(cols, 8)
        pad = torch.zeros(rows, co - cols, dtype=torch.bfloat16)
        hi, lo = torch.cat([hi, pad], 1), torch.cat([lo, pad], 1)
        xd = x.to(dev)
        assert torch.equal(ops.split_bf16x3(xd, 0).cpu(), torch.cat([hi, lo, hi], 1))
        assert torch.equal(ops.split_bf16x3(xd, 1).cpu(), torch.cat([hi, hi, lo], 1))
        assert torch.equal(ops.split_bf16x3(xd, 1, stacked=True).cpu(), torch.cat([hi, hi, lo], 0))
        pr = up(rows, 8)
        zr = torch.zeros(pr - rows, co, dtype=torch.bfloat16)
        assert torch.equal(ops.split_bf16x3(xd, 1, stacked=True, part_rows=pr).cpu(), torch.cat([hi, zr, hi, zr, lo, zr], 0))
        xt = x.t().contiguous().to(dev).t()                                   # column-major view of the same values
        assert torch.equal(ops.split_bf16x3(xt, 0).cpu(), torch.cat([hi, lo, hi], 1))
    with pytest.raises(TypeError):
        ops.split_bf16x3(torch.zeros(4, 8, device=dev, dtype=torch.bfloat16), 0)


# ------------------------------------------------------------------------------------------------------------- mm_bf16x3
def bound(a_abs, b_abs, depth):
    """(3 * 2^-16 + K' * 2^-23) * (|A| |B|): a_abs [M, K], b_abs [K, N] in float64, depth = K' of the GEMM that runs."""
    return (3 * 2.0 ** -16 + depth * 2.0 ** -23) * (a_abs @ b_abs)


def rel_l2(got, ref):
    return float((got.double() - ref).norm() / ref.norm())


def run_mm(dev, m, k, n, seed):
    from gmlm_amd import dense
    g = torch.Generator().manual_seed(seed)
    a = torch.randn(m, k, generator=g).to(dev).requires_grad_(True)
    b = (torch.randn(n, k, generator=g) * 0.5).to(dev).requires_grad_(True)
    dy = torch.randn(m, n, generator=g).to(dev)
    y = dense.mm_bf16x3(a, b)
    y.backward(dy)
    return a, b, dy, y.detach()


def check_three(a, b, dy, y, da, db, tag):
    """y, da, db against float64 with the elementwise bound, and each at most 1/32 of the plain bf16 GEMM's relative L2 error
    (bf16 operands, fp32 result: the most favourable form of the plain GEMM) on the same inputs."""
    m, k = a.shape
    n = b.shape[0]
    a64, b64, dy64 = a.detach().double(), b.detach().double(), dy.double()
    ab, bb, dyb = a.detach().bfloat16(), b.detach().bfloat16(), dy.bfloat16()
    f32 = dict(out_dtype=torch.float32)
    cases = [("y", y, a64 @ b64.t(), bound(a64.abs(), b64.abs().t(), 3 * up(k, 8)), torch.mm(ab, bb.t(), **f32)),
             ("da", da, dy64 @ b64, bound(dy64.abs(), b64.abs(), 3 * up(n, 8)), torch.mm(dyb, bb, **f32)),
             ("db", db, dy64.t() @ a64, bound(dy64.abs().t(), a64.abs(), 3 * m), torch.mm(dyb.t(), ab, **f32))]
    for name, got, ref, lim, plain in cases:
        assert got.dtype == torch.float32 and got.shape == ref.shape
        err = (got.double() - ref).abs()
        worst = float((err / lim.clamp(min=1e-300)).max())
        e3, e1 = rel_l2(got, ref), rel_l2(plain, ref)
        print(f"  {tag} {name}: worst err / bound = {worst:.3f}; rel L2 bf16x3 {e3:.2e}, plain bf16 {e1:.2e}, ratio {e1 / max(e3, 1e-30):.0f}x")
        assert worst <= 1.0, (tag, name, worst)
        assert e3 <= e1 / 32, (tag, name, e3, e1)


@pytest.mark.parametrize("n", [8, 264])
@pytest.mark.parametrize("k", [8, 20, 768])
@pytest.mark.parametrize("m", [1, 33])
def test_mm_bf16x3_forward_dx_dw_vs_float64(dev, m, k, n):
    a, b, dy, y = run_mm(dev, m, k, n, seed=m * 1000 + k * 10 + n)
    check_three(a, b, dy, y, a.grad, b.grad, f"M={m} K={k} N={n}")


@pytest.mark.parametrize("t,native", [(5504, True), (5440, False)])
def test_weight_gradient_through_the_split_k_kernel(dev, t, native):
    """3T = 16,512 >= 16,384 with N = K = 768: the viewed [3T, .] operands reach the split-K HIP kernel (K11) unchanged;
    3T = 16,320 stays on the library path.  Same bound, K' = 3T."""
    from gmlm_amd import dense, nn, ops
    n = k = 768
    g = torch.Generator().manual_seed(t)
    a = (torch.randn(t, k, generator=g) * 0.5).to(dev).requires_grad_(True)
    b = (torch.randn(n, k, generator=g) * 0.1).to(dev).requires_grad_(True)
    dy = torch.randn(t, n, generator=g).to(dev)
    x1, dy0 = ops.split_bf16x3(a.detach(), 1), ops.split_bf16x3(dy, 0)
    assert x1.shape == (t, 3 * k) and dy0.shape == (t, 3 * n)
    assert nn._native_wgrad_ok(dy0.view(3 * t, n), x1.view(3 * t, k), True) is native
    y = dense.mm_bf16x3(a, b)
    ran = kernels_run(lambda: y.backward(dy))
    assert any(r.startswith("wgrad_bf16_kernel") for r in ran) is native, sorted(ran)
    assert any(r.startswith("split3::split_rows_kernel<0>") for r in ran), sorted(ran)
    a64, dy64 = a.detach().double(), dy.double()
    ref = dy64.t() @ a64
    lim = bound(dy64.abs().t(), a64.abs(), 3 * t)
    worst = float(((b.grad.double() - ref).abs() / lim).max())
    e3 = rel_l2(b.grad, ref)
    e1 = rel_l2(torch.mm(dy.bfloat16().t(), a.detach().bfloat16(), out_dtype=torch.float32), ref)
    print(f"  T={t} dW ({'split-K kernel' if native else 'library'}): worst err / bound = {worst:.3f}; rel L2 {e3:.2e} (plain bf16 {e1:.2e})")
    assert worst <= 1.0 and e3 <= e1 / 32


def test_mm_with_a_split_weight_is_this_sequence_of_primitives(dev):
    """dense._mm with a SplitWeight at T, K, N = 40, 20, 16 (K' = 24: pad columns in both operands, the [:n, :k] cut of dW and
    the column cut of dx), the weight and the bias each stacked from two 8-row masters, residual output: the output and every
    gradient bit for bit equal to the split kernel, torch.mm with an fp32 result and the column-sum kernel called in that order."""
    from gmlm_amd import dense, ops
    t, k, n = 40, 20, 16
    g = torch.Generator().manual_seed(40)
    x = torch.randn(t, k, generator=g).to(dev).requires_grad_(True)
    masters = [p.to(dev).requires_grad_(True) for p in (torch.randn(8, k, generator=g), torch.randn(8, k, generator=g),
                                                        torch.randn(8, generator=g), torch.randn(8, generator=g))]
    dy, dres = torch.randn(t, n, generator=g).to(dev), torch.randn(t, k, generator=g).to(dev)
    w = torch.cat([m.detach() for m in masters[:2]], 0)
    bc = torch.cat([m.detach() for m in masters[2:]], 0)
    sw = dense.SplitWeight(w)
    w0, w1s = ops.split_bf16x3(w, 0), ops.split_bf16x3(w, 1, stacked=True, part_rows=n)
    assert sw.shape == (n, k) and torch.equal(sw.w0, w0) and torch.equal(sw.w1s, w1s) and w1s.shape == (3 * n, 24)

    y, xres = dense._mm(x, sw, bc, masters, residual=True)
    assert xres._base is x and xres.data_ptr() == x.data_ptr()
    torch.autograd.backward([y, xres], [dy, dres.clone()])

    f32 = dict(out_dtype=torch.float32)
    x1 = ops.split_bf16x3(x.detach(), 1)                                       # [T, 3 K'] (hi, hi, lo)
    assert torch.equal(y, torch.mm(x1, w0.t(), **f32).add_(bc))
    dy0 = ops.split_bf16x3(dy, 0)                                              # [T, 3 N'] (hi, lo, hi)
    assert torch.equal(x.grad, dres + torch.mm(dy0, w1s, **f32)[:, :k])
    dw = torch.mm(dy0.view(3 * t, n).t(), x1.view(3 * t, 24), **f32)[:n, :k]
    db = ops.column_sum(dy)
    for got, want in zip([m.grad for m in masters], [dw[:8], dw[8:], db[:8], db[8:]]):
        assert got.dtype == torch.float32 and torch.equal(got, want)


def test_inf_and_nan_stay_in_their_rows(dev):
    """One infinity and one NaN in x: exactly their rows of y stop being finite, nothing else.  (The row of the infinity holds
    infinities where w_hi and w_lo of that column agree in sign and NaN where they do not: inf * w_hi + inf * w_lo.)"""
    from gmlm_amd import dense
    g = torch.Generator().manual_seed(8)
    x = torch.randn(8, 24, generator=g)
    w = torch.randn(16, 24, generator=g)
    x[2, 5], x[5, 7] = float("inf"), float("nan")
    y = dense.mm_bf16x3(x.to(dev), w.to(dev)).cpu()
    finite = torch.isfinite(y)
    assert not bool(finite[2].any()) and bool(torch.isnan(y[5]).all())
    keep = [0, 1, 3, 4, 6, 7]
    assert bool(finite[keep].all())
    ref = x[keep].double() @ w.double().t()
    assert float((y[keep].double() - ref).abs().max()) <= 1e-4
    assert bool(torch.isinf(y[2]).any())                                       # the infinity itself survives where the signs agree
