"""The wide LayerNorm kernels (gmlm_bias_res_layernorm_wide_*, csrc/norm_wide.hip: rows of 1,028 ... 4,096, one 256-lane
workgroup per row) against float64, through ``ops.BiasResLayerNorm`` (the dispatch every caller takes).

Budgets: those test_gpu_norm_matrix.py uses for K6, restated here.  fp32 tensors, and the fp32 parameter gradients of bf16
cases: max |err| / max |ref| <= 1e-4, l2 rel <= 1e-5.  A bf16 output is fp32 arithmetic rounded once: each element within one
bf16 ulp of the float64 value plus (a) a term relative to the row's RMS for values computed from fp32 row statistics that
can cancel, (b) the floor of the bf16 kernels' erf_fast for values that pass through GELU.  The dropout mask is the host
restatement of the element hash K6's tests use (helpers.elem_dropout_scale): offset row * f + column, so the mask of a row
does not depend on which kernel, lane or chunk drew it."""
import pytest
import torch
import torch.nn.functional as F

from helpers import _close, elem_dropout_scale, kernels_run

pytestmark = pytest.mark.gpu

bf, f32 = torch.bfloat16, torch.float32
FP32_BUDGET = (1e-4, 1e-5)
SEED = 0x1234_5678_9ABC
MAX_BLOCKS = 256                     # norm_wide.hip, kMaxBlocks: the backward's grid; more rows take a second pass


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _tn(dtype):
    return "unsigned short" if dtype == bf else "float"


def _b(v):
    return "true" if v else "false"


def _bf16_ulp(ref):
    return torch.exp2(torch.floor(torch.log2(ref.abs().clamp_min(2.0 ** -126))) - 7)


def _ulp_check(name, got, ref, extra=None):
    assert got.dtype == torch.bfloat16, (name, got.dtype)
    err = (got.double() - ref).abs()
    bound = _bf16_ulp(ref)
    if extra is not None:
        bound = bound + extra
    ratio = err / bound
    worst, nbad = float(ratio.max()), int((ratio > 1).sum())
    print(f"  {name}: max err / bound = {worst:.2f}, {nbad} of {ratio.numel()} outside")
    assert nbad == 0, (name, worst, nbad)


def _erf_floor(x):
    return 0.5 * x.abs() * (1.5e-7 + 2.0 ** -23)


def _row_rms(t):
    return t.pow(2).mean(-1, keepdim=True).sqrt()


def _mask(rows, f, p, dev):
    if not p:
        return None
    return elem_dropout_scale(SEED, torch.arange(rows * f, dtype=torch.int64, device=dev), p).view(rows, f).double()


def _leaves(dev, dt, rows, f, bias, res, g):
    x = torch.randn(rows, f, generator=g).to(dev, dt)
    r = torch.randn(rows, f, generator=g).to(dev, dt) if res else None
    b = (0.1 * torch.randn(f, generator=g)).to(dev) if bias else None
    gamma, beta = (1 + 0.1 * torch.randn(f, generator=g)).to(dev), (0.1 * torch.randn(f, generator=g)).to(dev)
    gy = torch.randn(rows, f, generator=g).to(dev, dt)
    return [x, b, r, gamma, beta], gy


def _run(dev, dt, rows, f, bias, res, act, p, check_kernels=True):
    from gmlm_amd import ops
    eps = 1e-12
    g = torch.Generator().manual_seed(rows * 7919 + f)
    leaves, gy = _leaves(dev, dt, rows, f, bias, res, g)
    dv = [None if v is None else v.clone().requires_grad_(True) for v in leaves]
    box = {}
    fwd = lambda: box.setdefault("y", ops.BiasResLayerNorm.apply(dv[0], dv[1], dv[2], dv[3], dv[4], eps, act, p, SEED))
    print(f"\nwide LayerNorm rows={rows} f={f} {dt} bias={bias} res={res} act={act} p={p}:")
    if check_kernels:                                            # the profiler costs more than the kernels: not in every sub-case
        fwd_k = kernels_run(fwd)
        y = box["y"]
        bwd_k = kernels_run(lambda: y.backward(gy))
        t = _tn(dt)
        assert fwd_k == {f"lnw::fwd_kernel<{t}, {_b(act)}>"}, sorted(fwd_k)
        assert bwd_k == {f"lnw::bwd_kernel<{t}, {_b(act)}, {_b(p > 0)}, {_b(res)}>", "rows_sum_kernel"}, sorted(bwd_k)
    else:
        y = fwd()
        y.backward(gy)

    ref = [None if v is None else v.detach().double().requires_grad_(True) for v in leaves]
    m = _mask(rows, f, p, dev)
    z = ref[0] + ref[1] if bias else ref[0]
    if m is not None:
        z = z * m
    if res:
        z = z + ref[2]
    mu = z.mean(-1, keepdim=True)
    rs = ((z - mu).pow(2).mean(-1, keepdim=True) + eps).rsqrt()
    tpre = (z - mu) * rs * ref[3] + ref[4]
    yr = F.gelu(tpre) if act else tpre
    yr.backward(gy.double())
    names = ["dx", "dbias", "dres", "dgamma", "dbeta"]
    assert bool(torch.isfinite(y).all())
    if dt == f32:
        _close("y", y.detach(), yr.detach(), *FP32_BUDGET)
        for nm, a, r in zip(names, dv, ref):
            if a is not None:
                _close(nm, a.grad, r.grad, *FP32_BUDGET)
    else:
        tp = tpre.detach()
        ya = 2.0 ** -16 * _row_rms(tp) + (_erf_floor(tp) if act else 0.0)
        _ulp_check("y", y.detach(), yr.detach(), ya)
        dyn = gy.double() * (torch.autograd.functional.vjp(F.gelu, tp, torch.ones_like(tp))[1] if act else 1.0)
        gscale = 2.0 ** -15 * rs.detach() * _row_rms(dyn * ref[3].detach())
        _ulp_check("dx", dv[0].grad, ref[0].grad, gscale * (float(m.max()) if m is not None else 1.0))
        if res:
            _ulp_check("dres", dv[2].grad, ref[2].grad, gscale)
        for nm, a, r in zip(names, dv, ref):
            if nm in ("dbias", "dgamma", "dbeta") and a is not None:
                _close(nm, a.grad, r.grad, *FP32_BUDGET)
    if m is not None:
        assert bool((dv[0].grad[m == 0] == 0).all()), "dx of a dropped element is not zero"
    return leaves, gy, y.detach(), [None if v is None else v.grad for v in dv]


def _widths(dt):
    v = 4 if dt == f32 else 8
    return (1028 if dt == f32 else 1032, 2048, 2560, 4096 - v, 4096)


FEATURES = {"plain": dict(bias=False, res=False, act=False, p=0.0),
            "bias_res": dict(bias=True, res=True, act=False, p=0.0),
            "bias_gelu_drop": dict(bias=True, res=False, act=True, p=0.3),
            "res_drop": dict(bias=False, res=True, act=False, p=0.3)}


@pytest.mark.parametrize("feat", list(FEATURES))
@pytest.mark.parametrize("dt", [f32, bf], ids=("fp32", "bf16"))
def test_wide_layernorm_vs_fp64(dev, dt, feat):
    """Every width at both ends of the range and at the model widths, with 1, 3 and 257 rows (257: one more than the
    backward's grid, so one workgroup accumulates two rows and all 256 partial rows are summed)."""
    for f in _widths(dt):
        for rows in (1, 3, 257):
            _run(dev, dt, rows, f, check_kernels=rows == 3, **FEATURES[feat])


@pytest.mark.parametrize("dt", [f32, bf], ids=("fp32", "bf16"))
def test_second_stage_with_several_rows_per_workgroup(dev, dt):
    """2 * 256 + 77 rows: every workgroup of the backward strides through two or three rows before it writes its partial
    sums, and the forward's grid-stride loop is exercised by the same call only above 2,048 rows, so run that too (plain)."""
    _run(dev, dt, 2 * MAX_BLOCKS + 77, 1028 if dt == f32 else 1032, bias=True, res=True, act=True, p=0.3)
    _run(dev, dt, 2048 + 5, 2048, bias=False, res=False, act=False, p=0.0, check_kernels=False)


@pytest.mark.parametrize("dt", [f32, bf], ids=("fp32", "bf16"))
def test_dropout_mask_is_the_element_hash_of_k6(dev, dt):
    """x = 1, no bias / residual: an element of z is 0 (dropped) or the keep scale, so (z - mean) * rstd takes two values per
    row and y > 0 marks exactly the kept elements.  They must be the restated hash at offset row * f + column -- the function
    K6 draws (test_gpu_norm_matrix.py), so a 1,024-wide and a wide row of one tensor agree on the mask."""
    from gmlm_amd import ops
    rows, f, p = 5, 2560, 0.3
    x = torch.ones(rows, f, device=dev, dtype=dt)
    y = ops.BiasResLayerNorm.apply(x, None, None, torch.ones(f, device=dev), torch.zeros(f, device=dev), 1e-5, False, p, SEED)
    want = _mask(rows, f, p, dev) > 0
    assert bool(((y > 0) == want).all())
    assert abs(float(want.double().mean()) - (1 - p)) < 4 * (p * (1 - p) / (rows * f)) ** 0.5 + 1e-4


@pytest.mark.parametrize("dt", [f32, bf], ids=("fp32", "bf16"))
def test_repeat_and_workspace_size_give_identical_bytes(dev, dt):
    """Two calls, and the backward with an exact-size workspace (guard bytes behind it untouched) and a roomy one, give
    identical bytes."""
    import ctypes as C
    from gmlm_amd import ops
    from gmlm_amd._lib import BF16, F32, check, lib
    rows, f, p = 300, 2560, 0.3
    a = _run(dev, dt, rows, f, bias=True, res=True, act=True, p=p, check_kernels=False)
    b = _run(dev, dt, rows, f, bias=True, res=True, act=True, p=p, check_kernels=False)
    bits = lambda t: t.view(torch.int16 if t.element_size() == 2 else torch.int32)
    assert torch.equal(bits(a[2]), bits(b[2]))
    for ga, gb in zip(a[3], b[3]):
        assert torch.equal(bits(ga), bits(gb))
    (x, bias, res, gamma, beta), gy = a[0], a[1]
    mean, rstd = torch.empty(rows, device=dev), torch.empty(rows, device=dev)
    y = torch.empty_like(x)
    code = F32 if dt == f32 else BF16
    ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    check(lib().gmlm_bias_res_layernorm_wide_fwd(ptr(x), ptr(bias), ptr(res), ptr(gamma), ptr(beta), rows, f, 1e-12, 1, p, SEED, None,
                                                 ptr(y), ptr(mean), ptr(rstd), code, None), "fwd")
    need = lib().gmlm_bias_res_layernorm_wide_bwd_workspace_bytes(rows, f)
    assert need == min(rows, MAX_BLOCKS) * 3 * f * 4
    outs = []
    for extra in (0, 1 << 20):
        ws = torch.full((need + extra + 64,), 0x5A, dtype=torch.uint8, device=dev)
        dx, dres = torch.empty_like(x), torch.empty_like(x)
        dg, db, dbi = (torch.empty(f, device=dev) for _ in range(3))
        check(lib().gmlm_bias_res_layernorm_wide_bwd(ptr(gy), ptr(x), ptr(bias), ptr(res), ptr(gamma), ptr(beta), ptr(mean), ptr(rstd),
                                                     rows, f, 1, p, SEED, None, ptr(dx), ptr(dres), ptr(dg), ptr(db), ptr(dbi), code,
                                                     ptr(ws), need + extra, None), "bwd")
        torch.cuda.synchronize()
        assert bool((ws[need + extra:] == 0x5A).all()), "the backward wrote behind its workspace"
        if extra:
            assert bool((ws[need:need + extra] == 0x5A).all()), "the backward used more than the size it asks for"
        outs.append((dx, dres, dg, db, dbi))
    for u, w in zip(*outs):
        assert torch.equal(bits(u), bits(w))
    for u, w in zip(outs[0], (a[3][0], a[3][2], a[3][3], a[3][4], a[3][1])):     # and the bytes ops.BiasResLayerNorm returned
        assert torch.equal(bits(u), bits(w))
