"""The norm / row-op dispatch matrix: every reachable instantiation of the GraphNorm and LayerNorm kernels
(norm_kernels.hip) and of the bias+GELU, mean-pool, soft-mask and embedding-sum kernels (rowops_kernels.hip) run at least
once through the ops layer against a float64 reference built from the same rounded inputs the kernels read, with the
kernels that really ran read back by name from the profiler.

``CASES`` names, per case, the EXACT set of the project's kernels the forward and the backward launch; ``UNREACHABLE`` lists
the compiled LayerNorm instantiations the host dispatch (``ln_geom``, norm_kernels.hip) cannot select.  Their union must
equal the family's kernels in the built library (tests/test_norm_matrix_cpu.py).

LayerNorm geometries (lanes per row LPR, 16-byte chunks per lane CH) are met at both ends of their width range, each with
ACT, DROP and RES on and off and bias present and absent.  Dropout masks come only from helpers.elem_dropout_scale, the
independent restatement of the kernels' element hash: at bf16 f = 768 the forward (32 lanes x 3 chunks) and the backward
(64 x 2) must draw the same mask to pass.

Budgets.  fp32 tensors, and the fp32 statistics / parameter gradients of bf16 cases, use the fp32 budget of
_close (max |err| / max |ref| <= 1e-4, l2 rel <= 1e-5).  A bf16 output is fp32 arithmetic rounded once, so each element must
lie within one bf16 ulp of the float64 value, plus, only where named: (a) a term relative to the row's (LayerNorm) or
column's (GraphNorm) RMS for values computed from fp32 statistics or fp32 sums that can cancel (mean / rstd, the s1 / s2 or
m2 / mean_do terms of the gradients, the soft-mask blend), whose error is a few fp32 ulps of that scale and exceeds one bf16
ulp of a nearly cancelled result; (b) a floor for values that pass through the bf16 kernels' erf_fast (A&S 7.1.26, stated
|err| <= 1.5e-7, plus the fp32 rounding of 1 + erf), scaled by 0.5 |x| (forward) or |dy| (derivative): in the far negative
GELU tail one bf16 ulp of the result is smaller than that error."""
import zlib
from dataclasses import dataclass

import pytest
import torch
import torch.nn.functional as F

from helpers import _close, elem_dropout_scale, kernels_run

pytestmark = pytest.mark.gpu

BF, F32 = "unsigned short", "float"          # bf16 is an unsigned short in the kernels' template ids
bf, f32 = torch.bfloat16, torch.float32
FP32_BUDGET = (1e-4, 1e-5)
HOST_SEED, DEVICE_COUNTER = 2 ** 32 - 5, 7   # their 64-bit sum carries into the high word of the seed
SEED = 0x1234_5678_9ABC
ROWS_SUM, LN_FINAL, ZERO = "rows_sum_kernel", "ln_bwd_final_kernel", "zero_words_kernel"


def _b(v):
    return "true" if v else "false"


def _tn(dtype):
    return BF if dtype == bf else F32


def lnf(t, ch, lpr, act):
    return f"ln_fwd_kernel<{t}, {ch}, {lpr}, {_b(act)}>"


def lnb(t, ch, lpr, act, drop, res):
    return f"ln_bwd_kernel<{t}, {ch}, {lpr}, {_b(act)}, {_b(drop)}, {_b(res)}>"


def colstats(t):
    return f"col_reduce_partial_kernel<2, gmlm::ColStatsFn<{t}> >"


def gn_bwd_stats(t, act):
    return f"col_reduce_partial_kernel<2, gmlm::GraphNormBwdStatsFn<{t}, {_b(act)}> >"


SOFTMASK_BWD = "col_reduce_partial_kernel<1, gmlm::SoftmaskBwdFn>"


@dataclass(frozen=True)
class Case:
    id: str
    op: str                    # "ln", "gn", "bg" (bias+GELU), "pool", "softmask", "embed"
    dtype: torch.dtype
    fwd: frozenset
    bwd: frozenset
    rows: int = 0
    f: int = 0
    act: bool = False
    p: float = 0.0
    res: bool = False          # LayerNorm: residual operand
    bias: bool = False         # LayerNorm / bias+GELU: bias operand
    seed_dev: bool = False     # ops.SEED_DEVICE set: the kernels add a device counter to the host seed
    extra: str = ""            # GraphNorm: "out100" / "out1000" (row 0 that many sigma out in half the columns), "big";
    #                            mean-pool: "pad" / "packed"


def _case(id_, op, dtype, fwd, bwd, **kw):
    return Case(id=id_, op=op, dtype=dtype, fwd=frozenset(fwd), bwd=frozenset(bwd), **kw)


# ---- LayerNorm ----------------------------------------------------------------------------------------------------------
# (forward geometry, backward geometry, lowest width, highest width); geometry = (LPR, CH)
_LN_F32 = [((32, 1), (32, 1), 4, 128), ((64, 1), (64, 1), 132, 256), ((32, 3), (32, 3), 260, 384),
           ((64, 2), (64, 2), 388, 512), ((64, 3), (64, 3), 516, 768), ((64, 4), (64, 4), 772, 1024)]
# bf16: from 65 chunks the backward takes 64 lanes x 2 chunks (3 chunks of 8 bf16 with 3 accumulator sets need all VGPRs)
_LN_BF16 = [((32, 1), (32, 1), 8, 256), ((64, 1), (64, 1), 264, 512), ((32, 3), (64, 2), 520, 768),
            ((64, 2), (64, 2), 776, 1024)]


def _ln(id_, dtype, fg, bg, f, rows, act, p, res, bias, **kw):
    t = _tn(dtype)
    return _case(id_, "ln", dtype, {lnf(t, fg[1], fg[0], act)}, {lnb(t, bg[1], bg[0], act, p > 0, res), LN_FINAL},
                 rows=rows, f=f, act=act, p=p, res=res, bias=bias, **kw)


def _ln_cases():
    out = []
    for dtype, table in ((f32, _LN_F32), (bf, _LN_BF16)):
        for fg, bg, lo, hi in table:
            for i in range(8):
                act, drop, res = bool(i & 4), bool(i & 2), bool(i & 1)
                f = (lo, hi)[i & 1]
                bias = bin(i).count("1") % 2 == 1                      # present / absent crossed with every flag and width
                # 77 rows: the last wave of LPR 32 has one live row of two.  One row only where dropout is followed by a
                # residual or absent: a lone row that dropout leaves with one nonzero element is scale invariant under
                # LayerNorm (true dx = 0, fp32 gives rounding noise), which a budget relative to the tensor's max cannot take
                rows = 1 if i in (0, 3, 5) else 77
                tag = f"ln_{'bf16' if dtype == bf else 'f32'}_L{fg[0]}C{fg[1]}_f{f}_r{rows}" + \
                      "".join(s for s, on in (("_act", act), ("_drop", drop), ("_res", res), ("_bias", bias)) if on)
                out.append(_ln(tag, dtype, fg, bg, f, rows, act, 0.3 if drop else 0.0, res, bias))
    # row counts where the grid-stride loops repeat: forward above 8,192 * RPW rows (2,048 blocks x 4 waves x RPW rows),
    # backward above 8,192 rows (1,024 blocks of 8 rows)
    out.append(_ln("ln_f32_L64C1_rows20011_drop_res_bias", f32, (64, 1), (64, 1), 200, 20011, False, 0.1, True, True))
    out.append(_ln("ln_bf16_L32C1_rows16389_act_drop", bf, (32, 1), (32, 1), 256, 16389, True, 0.3, False, False,
                   seed_dev=True))
    # BertSelfOutput / BertOutput at the step's token count: bias, p = 0.1, residual; forward 32 x 3, backward 64 x 2
    out.append(_ln("ln_bf16_bert_91712x768", bf, (32, 3), (64, 2), 768, 91712, False, 0.1, True, True))
    # no rows: the forward launches nothing, the backward zero-fills dgamma / dbeta / dbias
    out.append(_case("ln_f32_rows0", "ln", f32, set(), {ZERO}, rows=0, f=768, act=True, p=0.1, res=True, bias=True))
    return out


def _ln_unreachable():
    r = "ln_geom (norm_kernels.hip) never selects it: "
    u = {}
    for t in (F32, BF):
        for act in (False, True):
            u[lnf(t, 2, 32, act)] = r + "33-64 chunks leave as many idle lanes at 32 lanes x 2 as at 64 x 1, and 64 x 1 wins ties"
            for drop in (False, True):
                for res in (False, True):
                    u[lnb(t, 2, 32, act, drop, res)] = u[lnf(t, 2, 32, act)]
    for act in (False, True):
        for ch in (3, 4):
            u[lnf(BF, ch, 64, act)] = r + "bf16 rows are at most 1,024 wide = 128 chunks = 64 lanes x 2"
        for drop in (False, True):
            for res in (False, True):
                for ch in (3, 4):
                    u[lnb(BF, ch, 64, act, drop, res)] = r + "bf16 rows are at most 1,024 wide = 128 chunks = 64 lanes x 2"
                u[lnb(BF, 3, 32, act, drop, res)] = r + "the bf16 backward moves 3 chunks per lane to 64 lanes x 2 (VGPRs)"
    return u


# ---- GraphNorm ----------------------------------------------------------------------------------------------------------
def _gn(id_, dtype, n, f, act, p, **kw):
    t = _tn(dtype)
    return _case(id_, "gn", dtype, {colstats(t), ROWS_SUM, "graphnorm_finalize_kernel", f"graphnorm_apply_kernel<{t}, {_b(act)}>"},
                 {gn_bwd_stats(t, act), ROWS_SUM, f"graphnorm_bwd_apply_kernel<{t}, {_b(act)}>"}, rows=n, f=f, act=act, p=p, **kw)


# col_reduce_plan: 16-row chunks while n < 16 * ceil(4096 / ceil(f / 64)): f = 6144 -> 688 rows, f = 1 -> 65,536 rows
_GN = [
    _gn("gn_f32_f100_n5", f32, 5, 100, False, 0.0),
    _gn("gn_f32_f1_n999_act_drop", f32, 999, 1, True, 0.3),
    _gn("gn_f32_f768_n5201_drop", f32, 5201, 768, False, 0.1),
    _gn("gn_f32_f768_n169343_act_drop_seeddev", f32, 169343, 768, True, 0.3, seed_dev=True),
    _gn("gn_f32_f6144_n600_act", f32, 600, 6144, True, 0.0),
    _gn("gn_f32_f6144_n700_drop", f32, 700, 6144, False, 0.3),
    _gn("gn_f32_outlier100_n169343", f32, 169343, 768, False, 0.0, extra="out100"),
    _gn("gn_f32_outlier1000_n5201_act_drop", f32, 5201, 768, True, 0.1, extra="out1000"),
    _gn("gn_bf16_f100_n17_act_drop", bf, 17, 100, True, 0.3),
    _gn("gn_bf16_f1_n70000", bf, 70000, 1, False, 0.0),
    _gn("gn_bf16_f768_n5201_act_drop", bf, 5201, 768, True, 0.1),
    _gn("gn_bf16_f768_n169343_drop_seeddev", bf, 169343, 768, False, 0.3, seed_dev=True),
    _gn("gn_bf16_f6144_n600_drop", bf, 600, 6144, False, 0.3),
    _gn("gn_bf16_f6144_n700_act", bf, 700, 6144, True, 0.0),
    _gn("gn_bf16_outlier100_n5201_act_drop", bf, 5201, 768, True, 0.3, extra="out100"),
    _gn("gn_bf16_outlier1000_n169343", bf, 169343, 768, False, 0.0, extra="out1000"),
    # 2^30 + 5 rows x 8 = 2^33 + 40 elements: the pair index (offset >> 1) of the last 5 rows has a high word, which 2^32 + 40
    # elements would not reach (S5 trains GraphNorm with dropout at 7.7e9 elements)
    _gn("gn_bf16_2pow33_elements_drop", bf, 2 ** 30 + 5, 8, False, 0.3, extra="big"),
]


# ---- bias + GELU --------------------------------------------------------------------------------------------------------
def _bg(id_, dtype, rows, f, p, bias):
    t = _tn(dtype)
    bwd = {f"bias_gelu_bwd_kernel<{t}, {_b(p > 0)}>"} | ({ROWS_SUM} if bias else set())
    return _case(id_, "bg", dtype, {f"bias_gelu_fwd_kernel<{t}, {_b(p > 0)}>"}, bwd, rows=rows, f=f, p=p, bias=bias)


# bg_geom: 256 / 192 / 128 / 64 chunk-columns per block, the largest dividing the chunk count (else 256 with idle lanes);
# grid.y = min(rows, ceil(4096 (forward) or 2048 (backward) / column blocks)), two rows per step
_BG = [
    _bg("bg_f32_bx256_f1024_r20001_drop_bias", f32, 20001, 1024, 0.3, True),
    _bg("bg_f32_bx192_f768_r1", f32, 1, 768, 0.0, False),
    _bg("bg_f32_bx128_f512_r333_drop", f32, 333, 512, 0.3, False),
    _bg("bg_f32_bx64_f1280_r5000_bias", f32, 5000, 1280, 0.0, True),
    _bg("bg_f32_idle_f1000_r4097_drop_bias", f32, 4097, 1000, 0.1, True),
    _bg("bg_bf16_bx256_f2048_r3_drop_bias", bf, 3, 2048, 0.3, True),
    _bg("bg_bf16_bx192_f3072_r20001_bias", bf, 20001, 3072, 0.0, True),
    _bg("bg_bf16_bx128_f1024_r1_drop", bf, 1, 1024, 0.3, False),
    _bg("bg_bf16_bx64_f512_r777", bf, 777, 512, 0.0, False),
    _bg("bg_bf16_idle_f8_r9999_drop_bias", bf, 9999, 8, 0.1, True),
]

# ---- mean-pool, soft-mask, embedding sum -------------------------------------------------------------------------------
_ROWOPS = [
    _case("pool_bf16_padded", "pool", bf, {f"meanpool_fwd_kernel<{BF}>"}, {f"meanpool_bwd_kernel<{BF}>"}, rows=7, f=768,
          extra="pad"),
    _case("pool_bf16_packed", "pool", bf, {f"meanpool_fwd_kernel<{BF}>"}, {f"meanpool_bwd_kernel<{BF}>"}, rows=9, f=776,
          extra="packed"),
    _case("pool_f32_packed", "pool", f32, {f"meanpool_fwd_kernel<{F32}>"}, {f"meanpool_bwd_kernel<{F32}>"}, rows=9, f=300,
          extra="packed"),
    _case("softmask_bf16_padded", "softmask", bf, {f"softmask_fwd_kernel<{BF}>"}, {SOFTMASK_BWD, ROWS_SUM}, rows=5201, f=1703),
    _case("softmask_f32", "softmask", f32, {f"softmask_fwd_kernel<{F32}>"}, {SOFTMASK_BWD, ROWS_SUM}, rows=333, f=100),
    # > 4 * 65,536 rows: the row loop wraps; 260 columns: the second 256-column step has one live lane
    _case("embed_f32_rows262147", "embed", f32, {f"embed_sum_fwd_kernel<{F32}>"}, set(), rows=262147, f=260),
    _case("embed_bf16_rows1", "embed", bf, {f"embed_sum_fwd_kernel<{BF}>"}, set(), rows=1, f=1028),
]

CASES = _ln_cases() + _GN + _BG + _ROWOPS
UNREACHABLE = _ln_unreachable()

_FAMILY = ("ln_", "graphnorm_", "bias_gelu_", "meanpool_", "softmask_", "embed_sum_")


def _is_norm_family(name):
    """The kernels the CPU guard holds to CASES / UNREACHABLE."""
    return name.startswith(_FAMILY) or name in {colstats(F32), colstats(BF), SOFTMASK_BWD} or \
        name.startswith("col_reduce_partial_kernel<2, gmlm::GraphNormBwdStatsFn<")


# ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _bf16_ulp(ref):
    """Spacing of bf16 numbers at |ref| (float64): 2^(floor(log2 |ref|) - 7), subnormals at the smallest normal's spacing."""
    return torch.exp2(torch.floor(torch.log2(ref.abs().clamp_min(2.0 ** -126))) - 7)


def _ulp_check(name, got, ref, extra=None):
    """|got - ref| <= one bf16 ulp of ref (+ ``extra``, an absolute term with a stated reason), per element."""
    assert got.dtype == torch.bfloat16, (name, got.dtype)
    err = (got.double() - ref).abs()
    bound = _bf16_ulp(ref)
    if extra is not None:
        bound = bound + extra
    ratio = err / bound
    worst = float(ratio.max()) if ratio.numel() else 0.0
    nbad = int((ratio > 1).sum())
    print(f"  {name}: max err / bound = {worst:.2f}, {nbad} of {ratio.numel()} outside")
    assert nbad == 0, (name, worst, nbad)


def _erf_floor(x):
    """|error| of the bf16 kernels' 0.5 x (1 + erf_fast(x / sqrt 2)) from erf_fast's 1.5e-7 and the fp32 1 + erf"""
    return 0.5 * x.abs() * (1.5e-7 + 2.0 ** -23)


def _erf_grad_floor(x, dy):
    """|error| of dy * gelu'(x) with erf_fast: the cdf term as above; x * pdf through exp2 of an fp32 argument -x^2 / 2 * log2 e,
    whose rounding is relative x^2 2^-22, plus a few fp32 ulps"""
    pdf = torch.exp(-0.5 * x * x) * 0.3989422804014327
    return dy.abs() * (0.5 * (1.5e-7 + 2.0 ** -23) + x.abs() * pdf * (x * x * 2.0 ** -22 + 2.0 ** -20))


def _row_rms(t):
    return t.pow(2).mean(-1, keepdim=True).sqrt()


def _col_rms(t):
    return t.pow(2).mean(0, keepdim=True).sqrt()


def _seed(c, monkeypatch, dev):
    from gmlm_amd import ops
    if c.seed_dev:
        monkeypatch.setattr(ops, "SEED_DEVICE", torch.tensor([DEVICE_COUNTER], dtype=torch.int64, device=dev))
        return HOST_SEED, HOST_SEED + DEVICE_COUNTER
    return SEED, SEED


def _mask(mask_seed, rows, f, p, dev):
    """[rows, f] float64 multiplier (0 or the fp32 keep scale) of element r * f + c, or None without dropout"""
    if not p:
        return None
    return elem_dropout_scale(mask_seed, torch.arange(rows * f, dtype=torch.int64, device=dev), p).view(rows, f).double()


def _check_kernels(c, fwd_k, bwd_k):
    print(f"\n{c.id}: forward {sorted(fwd_k)}, backward {sorted(bwd_k)}")
    assert fwd_k == set(c.fwd), (sorted(fwd_k), sorted(c.fwd))
    assert bwd_k == set(c.bwd), (sorted(bwd_k), sorted(c.bwd))


# ---------------------------------------------------------------------------------------------------------------------------
def _run_ln(c, dev, seed, mask_seed, g):
    from gmlm_amd import ops
    rows, f, dt = c.rows, c.f, c.dtype
    eps = 1e-12
    x = torch.randn(rows, f, generator=g).to(dev, dt)
    res = torch.randn(rows, f, generator=g).to(dev, dt) if c.res else None
    bias = (0.1 * torch.randn(f, generator=g)).to(dev) if c.bias else None
    gamma, beta = (1 + 0.1 * torch.randn(f, generator=g)).to(dev), (0.1 * torch.randn(f, generator=g)).to(dev)
    gy = torch.randn(rows, f, generator=g).to(dev, dt)
    leaves = [x, bias, res, gamma, beta]
    dv = [None if v is None else v.clone().requires_grad_(True) for v in leaves]
    box = {}
    run = lambda: box.setdefault("y", ops.BiasResLayerNorm.apply(dv[0], dv[1], dv[2], dv[3], dv[4], eps, c.act, c.p, seed))
    if rows == 0:
        run()
        fwd_k = set()
    else:
        fwd_k = kernels_run(run)
    y = box["y"]
    bwd_k = kernels_run(lambda: y.backward(gy))
    _check_kernels(c, fwd_k, bwd_k)
    if rows == 0:
        assert y.shape == (0, f) and dv[0].grad.shape == (0, f)
        for v in (dv[1], dv[3], dv[4]):
            assert float(v.grad.abs().max()) == 0.0
        return

    ref = [None if v is None else v.detach().double().requires_grad_(True) for v in leaves]
    m = _mask(mask_seed, rows, f, c.p, dev)
    z = ref[0] + ref[1] if c.bias else ref[0]
    if m is not None:
        z = z * m
    if c.res:
        z = z + ref[2]
    mu = z.mean(-1, keepdim=True)
    rs = ((z - mu).pow(2).mean(-1, keepdim=True) + eps).rsqrt()
    tpre = (z - mu) * rs * ref[3] + ref[4]
    yr = F.gelu(tpre) if c.act else tpre
    yr.backward(gy.double())
    names = ["dx", "dbias", "dres", "dgamma", "dbeta"]
    assert bool(torch.isfinite(y).all())
    if dt == f32:
        _close("y", y.detach(), yr.detach(), *FP32_BUDGET)
        for nm, a, r in zip(names, dv, ref):
            if a is not None:
                _close(nm, a.grad, r.grad, *FP32_BUDGET)
        return
    tp = tpre.detach()
    # (a): mean / rstd are fp32 sums over the row; (b) for ACT
    ya = 2.0 ** -16 * _row_rms(tp) + (_erf_floor(tp) if c.act else 0.0)
    _ulp_check("y", y.detach(), yr.detach(), ya)
    # (a): dz = rstd (g dy' - s1 - zhat s2) with s1, s2 fp32 row sums: a few fp32 ulps of the terms that cancel,
    # rstd * RMS(g dy') over the row (dy' = dy * gelu'(t) with ACT)
    dyn = gy.double() * (torch.autograd.functional.vjp(F.gelu, tp, torch.ones_like(tp))[1] if c.act else 1.0)
    gscale = 2.0 ** -15 * rs.detach() * _row_rms(dyn * ref[3].detach())
    _ulp_check("dx", dv[0].grad, ref[0].grad, gscale * (float(m.max()) if m is not None else 1.0))
    if m is not None:
        assert bool((dv[0].grad[m == 0] == 0).all()), "dx of a dropped element is not zero"
    if c.res:
        _ulp_check("dres", dv[2].grad, ref[2].grad, gscale)
    for nm, a, r in zip(names, dv, ref):
        if nm in ("dbias", "dgamma", "dbeta") and a is not None:
            _close(nm, a.grad, r.grad, *FP32_BUDGET)                # fp32 sums of fp32 products


def _gn_ref(z, w, b, ms, eps, act, m, go):
    zz, ww, bb, mm = (v.double().requires_grad_(True) for v in (z, w, b, ms))
    mean = zz.mean(0)
    o = zz - mean * mm
    rstd = (o.pow(2).mean(0) + eps).rsqrt()
    t = ww * o * rstd + bb
    y = F.gelu(t) if act else t
    if m is not None:
        y = y * m
    y.backward(go.double())
    return y.detach(), t.detach(), [zz.grad, ww.grad, bb.grad, mm.grad]


def _run_gn(c, dev, seed, mask_seed, g):
    from gmlm_amd import ops
    if c.extra == "big":
        return _run_gn_big(c, dev, seed, mask_seed, g)
    n, f, dt = c.rows, c.f, c.dtype
    eps = 1e-5
    z = torch.randn(n, f, generator=g) + 1.0                            # mean 1, sigma 1: the shift matters
    if f > 1:
        z[:, 1] = 0.75                                                  # a constant column (mean_scale 1 there: variance 0)
    if c.extra:
        # row 0 that many sigma out in the first half of the columns: those take the second statistics pass, the second
        # half keeps the one-pass statistics (ops.GN_ONE_PASS_MAX_RATIO), and both halves are checked
        z[0, :(f + 1) // 2] += float(c.extra[3:])
    z = z.to(dev, dt)
    ms = torch.tensor([0.5, 1.0, 1.7, 0.0])[torch.arange(f) % 4].to(dev)
    w, b = (1 + 0.1 * torch.randn(f, generator=g)).to(dev), (0.1 * torch.randn(f, generator=g)).to(dev)
    go = torch.randn(n, f, generator=g).to(dev, dt)
    dv = [v.clone().requires_grad_(True) for v in (z, w, b, ms)]
    box = {}
    fwd_k = kernels_run(lambda: box.setdefault("y", ops.GraphNormAct.apply(dv[0], dv[1], dv[2], dv[3], eps, c.act, c.p, seed,
                                                                             dt, None, None)))
    y = box["y"]
    bwd_k = kernels_run(lambda: y.backward(go))
    _check_kernels(c, fwd_k, bwd_k)
    m = _mask(mask_seed, n, f, c.p, dev)
    yr, t, grads = _gn_ref(z, w, b, ms, eps, c.act, m, go)
    names = ["dz", "dweight", "dbias", "dmean_scale"]
    assert bool(torch.isfinite(y).all()) and all(bool(torch.isfinite(a.grad).all()) for a in dv)
    if m is not None:
        assert bool((y[m == 0] == 0).all()), "a dropped element is not zero"
    if dt == f32:
        # the constant column (rstd = eps^-1/2) has ~300x larger dz: budgeted on its own so that it does not hide the rest
        for sl, tag in ((slice(1, 2), " (constant column)"), (torch.arange(f, device=dev) != 1, "")) if f > 1 else ((slice(None), ""),):
            _close("y" + tag, y.detach()[:, sl], yr[:, sl], *FP32_BUDGET)
            _close("dz" + tag, dv[0].grad[:, sl], grads[0][:, sl], *FP32_BUDGET)
        for nm, a, r in zip(names[1:], dv[1:], grads[1:]):
            _close(nm, a.grad, r, *FP32_BUDGET)
        return
    # (a): mean and rstd are fp32 column sums; (b) for ACT
    _ulp_check("y", y.detach(), yr, 2.0 ** -16 * _col_rms(t) + (_erf_floor(t) * (m if m is not None else 1.0) if c.act else 0.0))
    # (a): dz = w rstd (gz - ohat m2) - ms mean_do, with m2 and mean_do from fp32 column sums
    _ulp_check("dz", dv[0].grad, grads[0], 2.0 ** -15 * _col_rms(grads[0]))
    for nm, a, r in zip(names[1:], dv[1:], grads[1:]):
        _close(nm, a.grad, r, *FP32_BUDGET)


def _run_gn_big(c, dev, seed, mask_seed, g):
    """2^33 + 40 elements: statistics and gradients over all rows, the mask checked on the 5 rows whose element pairs pass
    2^32 (forward y and backward dz; the output gradient is zero elsewhere, so only those rows feed the column sums)."""
    from gmlm_amd import ops
    n, f, eps = c.rows, c.f, 1e-5
    tail = n - 2 ** 30
    assert (n - tail) * f == 2 ** 33
    z = torch.empty(n, f, dtype=bf, device=dev)
    gd = torch.Generator(device=dev).manual_seed(5)
    step = 1 << 26
    for r0 in range(0, n, step):
        r1 = min(n, r0 + step)
        z[r0:r1] = torch.randn(r1 - r0, f, generator=gd, device=dev).to(bf)
    ms = torch.tensor([0.5, 1.0, 1.7, 0.0] * 2, device=dev)
    w, b = (1 + 0.1 * torch.randn(f, generator=g)).to(dev), (0.1 * torch.randn(f, generator=g)).to(dev)
    zg = z.requires_grad_(True)
    box = {}
    fwd_k = kernels_run(lambda: box.setdefault("y", ops.GraphNormAct.apply(zg, w, b, ms, eps, False, c.p, seed, bf, None, None)))
    y = box["y"]
    go = torch.zeros(n, f, dtype=bf, device=dev)
    go[-tail:] = torch.randn(tail, f, generator=g).to(dev, bf)
    bwd_k = kernels_run(lambda: y.backward(go))
    _check_kernels(c, fwd_k, bwd_k)
    s1 = torch.zeros(f, dtype=torch.float64, device=dev)
    for r0 in range(0, n, step):
        s1 += z[r0:r0 + step].detach().double().sum(0)
    mean = s1 / n
    s2 = torch.zeros(f, dtype=torch.float64, device=dev)
    for r0 in range(0, n, step):
        s2 += (z[r0:r0 + step].detach().double() - mean * ms).pow(2).sum(0)
    rstd = (s2 / n + eps).rsqrt()
    zt = z[-tail:].detach().double()
    oh = (zt - mean * ms) * rstd
    idx = (torch.arange(n - tail, n, device=dev)[:, None] * f + torch.arange(f, device=dev)[None, :])
    assert int(idx.min()) >> 1 >= 2 ** 32
    m = elem_dropout_scale(mask_seed, idx, c.p).double()
    yr = (w * oh + b) * m
    assert bool((y[-tail:][m == 0] == 0).all())
    _ulp_check("y (rows past 2^33 elements)", y[-tail:].detach(), yr, 2.0 ** -16 * (w.abs() + b.abs()).double())
    gz = go[-tail:].double() * m
    sg, sgo = gz.sum(0), (gz * oh).sum(0)
    m2 = sgo / n
    mean_do = w * rstd * (sg / n - m2 * mean * (1 - ms) * rstd)
    dzr = w * rstd * (gz - oh * m2) - ms * mean_do
    _ulp_check("dz (rows past 2^33 elements)", zg.grad[-tail:], dzr, 2.0 ** -15 * (w * rstd).abs() * go[-tail:].double().abs().max())


def _run_bg(c, dev, seed, mask_seed, g):
    from gmlm_amd import ops
    rows, f, dt = c.rows, c.f, c.dtype
    x = torch.randn(rows, f, generator=g).mul(2.5).to(dev, dt)          # reaches the far GELU tail (x + bias ~ -10)
    bias = (0.5 * torch.randn(f, generator=g)).to(dev) if c.bias else None
    gy = torch.randn(rows, f, generator=g).to(dev, dt)
    xg = x.clone().requires_grad_(True)
    bg = bias.clone().requires_grad_(True) if c.bias else None
    box = {}
    fwd_k = kernels_run(lambda: box.setdefault("y", ops.BiasGelu.apply(xg, bg, c.p, seed)))
    y = box["y"]
    bwd_k = kernels_run(lambda: y.backward(gy))
    _check_kernels(c, fwd_k, bwd_k)
    xr = x.double().requires_grad_(True)
    br = bias.double().requires_grad_(True) if c.bias else None
    t = xr + br if c.bias else xr
    m = _mask(mask_seed, rows, f, c.p, dev)
    yr = F.gelu(t) if m is None else F.gelu(t) * m
    yr.backward(gy.double())
    if m is not None:
        assert bool((y[m == 0] == 0).all()) and bool((xg.grad[m == 0] == 0).all())
    if dt == f32:
        _close("y", y.detach(), yr.detach(), *FP32_BUDGET)
        _close("dx", xg.grad, xr.grad, *FP32_BUDGET)
    else:
        ks = m if m is not None else 1.0
        td = t.detach()
        _ulp_check("y", y.detach(), yr.detach(), _erf_floor(td) * ks)                               # (b)
        _ulp_check("dx", xg.grad, xr.grad, _erf_grad_floor(td, gy.double() * ks))                   # (b)
    if c.bias:
        _close("dbias", bg.grad, br.grad, *FP32_BUDGET)


def _run_pool(c, dev, g):
    from gmlm_amd import ops
    dt, p, b = c.dtype, c.f, c.rows
    nodes = 3 * b
    node_idx = torch.randperm(nodes, generator=g)[:b]
    if c.extra == "pad":
        l = 130
        lens = torch.tensor([130, 1, 0, 65, 129, 7, 2])[:b]
        hs = torch.randn(b, l, p, generator=g).to(dev, dt)
        rows_of = [(bi * l, int(lens[bi])) for bi in range(b)]
        flat = hs.view(b * l, p)
        cu, valid = None, None
        lens_arg = lens.to(dev, torch.int32)
    else:
        lens = torch.tensor([5, 0, 1, 128, 33, 0, 77, 2, 9])[:b]
        total = int(lens.sum())
        cu_l = [0] + torch.cumsum(lens, 0).tolist()
        pad = 11                                                          # rows behind cu_seqlens[-1]: zero gradient
        hs = torch.randn(total + pad, p, generator=g).to(dev, dt)
        rows_of = [(cu_l[bi], int(lens[bi])) for bi in range(b)]
        flat = hs
        cu, valid = torch.tensor(cu_l, dtype=torch.int32, device=dev), total
        lens_arg = None
    base = torch.zeros(nodes, p, device=dev)
    hg = hs.clone().requires_grad_(True)
    box = {}
    fwd_k = kernels_run(lambda: box.setdefault("out", ops.MeanPoolScatter.apply(base, hg, lens_arg, node_idx.to(dev), cu, valid)))
    out = box["out"]
    go = torch.randn(nodes, p, generator=g).to(dev)
    bwd_k = kernels_run(lambda: out.backward(go))
    _check_kernels(c, fwd_k, bwd_k)
    ref = torch.zeros(nodes, p, dtype=torch.float64, device=dev)
    dref = torch.zeros(flat.shape, dtype=torch.float64, device=dev)
    for bi, (r0, ln) in enumerate(rows_of):
        ni = int(node_idx[bi])
        ref[ni] = flat[r0:r0 + ln].double().sum(0) / max(ln, 1e-9)
        if ln:
            dref[r0:r0 + ln] = go[ni].double() / ln
    _close("out", out.detach(), ref, *FP32_BUDGET)
    dhs = hg.grad.view(dref.shape)
    if dt == f32:
        _close("dhs", dhs, dref, *FP32_BUDGET)
    else:
        _ulp_check("dhs", dhs, dref)
    assert float(dhs[dref == 0].abs().max()) == 0.0                       # padding rows and length-0 sequences


def _run_softmask(c, dev, g):
    from gmlm_amd import ops
    n, f, dt = c.rows, c.f, c.dtype
    beta = 0.7
    cols = (f + 15) // 16 * 16 if dt == bf else f                         # bf16: column padding to 16-byte rows
    x = torch.randn(n, f, generator=g).to(dev)
    mask = (torch.rand(n, generator=g) < 0.4).to(dev)
    tok = torch.randn(1, f, generator=g).to(dev).requires_grad_(True)
    box = {}
    fwd_k = kernels_run(lambda: box.setdefault("out", ops.SoftMask.apply(x, mask, tok, beta, dt, cols)))
    out = box["out"]
    go = torch.randn(n, cols, generator=g).to(dev, dt)
    bwd_k = kernels_run(lambda: out.backward(go))
    _check_kernels(c, fwd_k, bwd_k)
    xr, tr = x.double(), tok.detach().double()
    ref = torch.where(mask[:, None], (1 - beta) * xr + beta * tr, xr)
    dref = beta * go[:, :f].double()[mask].sum(0, keepdim=True)
    assert out.shape == (n, cols) and float(out.detach()[:, f:].abs().max() if cols > f else 0.0) == 0.0
    if dt == f32:
        _close("out", out.detach(), ref, *FP32_BUDGET)
    else:
        # (a): (1 - beta) x + beta t in fp32 (beta t and 1 - beta rounded to fp32 first) can cancel to below a bf16 ulp
        _ulp_check("out", out.detach()[:, :f], ref, 2.0 ** -22 * ((1 - beta) * xr.abs() + beta * tr.abs()))
    _close("dtoken", tok.grad, dref, *FP32_BUDGET)


def _run_embed(c, dev, g):
    from gmlm_amd import ops
    rows, p, dt = c.rows, c.f, c.dtype
    vocab, npos = 1000, 512
    word, pos, typ = (torch.randn(k, p, generator=g).to(dev) for k in (vocab, npos, 2))
    tok = torch.randint(0, vocab, (rows,), generator=g).to(dev)
    pid = torch.randint(0, npos, (rows,), generator=g).to(dev)
    box = {}
    fwd_k = kernels_run(lambda: box.setdefault("out", ops.embed_sum(tok, pid, word, pos, typ, dt)))
    _check_kernels(c, fwd_k, set())
    out = box["out"]
    # the contract is bit-exact: (word + type 0) + position in fp32, in that order, rounded once to the storage dtype
    assert torch.equal(out, ((word[tok] + typ[0]) + pos[pid]).to(dt))
    ref = word[tok].double() + typ[0].double() + pos[pid].double()
    if dt == f32:
        _close("out", out, ref, *FP32_BUDGET)
    else:
        _ulp_check("out", out, ref, 2.0 ** -23 * (word[tok].abs() + typ[0].abs() + pos[pid].abs()).double())


@pytest.mark.parametrize("c", CASES, ids=[c.id for c in CASES])
def test_norm_instantiation_vs_fp64(dev, monkeypatch, c):
    g = torch.Generator().manual_seed(zlib.crc32(c.id.encode()))
    seed, mask_seed = _seed(c, monkeypatch, dev)
    if c.op == "ln":
        _run_ln(c, dev, seed, mask_seed, g)
    elif c.op == "gn":
        _run_gn(c, dev, seed, mask_seed, g)
    elif c.op == "bg":
        _run_bg(c, dev, seed, mask_seed, g)
    elif c.op == "pool":
        _run_pool(c, dev, g)
    elif c.op == "softmask":
        _run_softmask(c, dev, g)
    else:
        _run_embed(c, dev, g)
