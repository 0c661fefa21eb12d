"""Every `*_workspace_bytes` companion reports enough for the kernels behind its entry point.

An under-report would let a kernel write past its workspace into whatever tensor the caching allocator placed next, silently.
Each case calls one workspace-taking entry point through the raw C ABI with real device tensors and valid arguments only:
  - the workspace is the first `need` bytes of a need + 4096 byte tensor filled with 0xA5, `need` being exactly what the
    companion returned; after the call the trailing 4096 bytes must be unchanged;
  - every output must equal, bit for bit, the output of the same call with a workspace of 4 * need bytes (the header promises
    fixed summation orders, and that no workspace needs initialising: both are filled with 0xA5 = NaN patterns).
Shapes: per family the smallest with more than one partial row / slice and a ragged last block, and LayerNorm backward once
past the 8,192 rows at which its companion clamps the block count.  No refusal runs here and no address is fabricated."""
import pytest
import torch

pytestmark = pytest.mark.gpu

F32, BF16 = 0, 1
bf, f32 = torch.bfloat16, torch.float32
TAIL = 4096


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    import gmlm_amd
    from gmlm_amd import _lib
    _lib.require_gfx950(0)
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def lib(dev):
    import gmlm_amd
    return gmlm_amd.lib()


def P(t):
    return None if t is None else t.data_ptr()


def ST():
    return torch.cuda.current_stream().cuda_stream


def rnd(dev, shape, dtype=f32, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).to(dtype).to(dev)


def ok(lib, rc):
    assert rc == 0, (rc, lib.gmlm_last_error())


def bits(t):
    return t.contiguous().view(torch.uint8).cpu()


def hold(lib, dev, need, run):
    """run(workspace pointer, workspace bytes) -> output tensors.  Exact-size run with a guarded tail against a roomy one."""
    assert need > 0
    exact = torch.full((need + TAIL,), 0xA5, dtype=torch.uint8, device=dev)
    assert exact.data_ptr() % 16 == 0
    got = run(P(exact), need)
    torch.cuda.synchronize()
    assert bool((exact[need:] == 0xA5).all()), "the kernels wrote past the bytes the companion reported"
    roomy = torch.full((4 * need,), 0xA5, dtype=torch.uint8, device=dev)
    want = run(P(roomy), 4 * need)
    torch.cuda.synchronize()
    assert len(got) == len(want) and len(got) > 0
    for i, (a, b) in enumerate(zip(got, want)):
        assert a.shape == b.shape and torch.equal(bits(a), bits(b)), f"output {i} depends on the workspace size"
        assert bool(torch.isfinite(a.float()).all()), f"output {i} is not finite"


def test_segment_sort(lib, dev):
    e, nseg = 3001, 40                                            # 12 blocks of 256 edges, the last with 185
    node = torch.randint(0, nseg, (e,), generator=torch.Generator().manual_seed(1)).to(dev)
    need = lib.gmlm_segment_sort_workspace_bytes(e)

    def run(ws, nbytes):
        perm, rowptr, bad = (torch.full((n,), -7, dtype=torch.int32, device=dev) for n in (e, nseg + 1, 1))
        ok(lib, lib.gmlm_segment_sort(P(node), None, None, 1, e, nseg, None, P(perm), P(rowptr), P(bad), ws, nbytes, ST()))
        return perm, rowptr, bad
    hold(lib, dev, need, run)
    ws = torch.empty(need, dtype=torch.uint8, device=dev)         # held in a name: a temporary would be freed, and reused, before the launch
    perm, rowptr, bad = run(P(ws), need)
    torch.cuda.synchronize()
    assert int(bad) == 0 and int(rowptr[-1]) == e and bool((node[perm.long()][1:] >= node[perm.long()][:-1]).all())


def test_basis_compose_bwd(lib, dev):
    ra, nb, cols = 3, 30, 2052                                    # 513 float4 columns: three blocks, the last with one
    comp, weight, dw = rnd(dev, (ra, nb), seed=2), rnd(dev, (nb, cols), seed=3), rnd(dev, (ra, cols), seed=4)
    need = lib.gmlm_basis_compose_bwd_workspace_bytes(ra, nb, cols)
    assert need == 3 * ra * nb * 4

    def run(ws, nbytes):
        dweight, dcomp = torch.empty_like(weight), torch.empty_like(comp)
        ok(lib, lib.gmlm_basis_compose_bwd(P(comp), P(weight), P(dw), ra, nb, cols, P(dweight), P(dcomp), ws, nbytes, ST()))
        return dweight, dcomp
    hold(lib, dev, need, run)


N, F = 100, 70                                                    # column reductions: 7 row chunks of 15 (last 10), 2 column tiles (64 + 6)


def test_colstats(lib, dev):
    x = rnd(dev, (N, F), bf, seed=5)
    need = lib.gmlm_colstats_workspace_bytes(N, F)
    assert need == 7 * 2 * F * 4

    def run(ws, nbytes):
        out = torch.empty(2, F, device=dev)
        ok(lib, lib.gmlm_colstats(P(x), BF16, None, N, F, P(out[0]), P(out[1]), ws, nbytes, ST()))
        return (out,)
    hold(lib, dev, need, run)


def test_graphnorm_bwd_stats(lib, dev):
    g, x = rnd(dev, (N, F), bf, seed=6), rnd(dev, (N, F), bf, seed=7)
    mean, rstd, w, b, ms = (rnd(dev, (F,), seed=s) for s in (8, 9, 10, 11, 12))
    rstd = rstd.abs() + 0.5
    need = lib.gmlm_colstats_workspace_bytes(N, F)

    def run(ws, nbytes):
        gs = torch.empty(2, F, device=dev)
        ok(lib, lib.gmlm_graphnorm_bwd_stats(P(g), BF16, P(x), P(mean), P(rstd), P(w), P(b), P(ms), N, F, 1, 0.25, 77, None, P(gs), ws, nbytes,
                                             ST()))
        return (gs,)
    hold(lib, dev, need, run)


@pytest.mark.parametrize("rows,blocks", [(37, 5), (8200, 1024)])   # 8 rows per block; above 8,192 rows the companion clamps to 1024 blocks
def test_layernorm_bwd(lib, dev, rows, blocks):
    f = 264
    x, res, dy = rnd(dev, (rows, f), bf, seed=13), rnd(dev, (rows, f), bf, seed=14), rnd(dev, (rows, f), bf, seed=15)
    bias, gamma, beta = rnd(dev, (f,), seed=16), rnd(dev, (f,), seed=17) + 1.0, rnd(dev, (f,), seed=18)
    y, mean, rstd = torch.empty_like(x), torch.empty(rows, device=dev), torch.empty(rows, device=dev)
    ok(lib, lib.gmlm_bias_res_layernorm_fwd(P(x), P(bias), P(res), P(gamma), P(beta), rows, f, 1e-5, 1, 0.1, 99, None, P(y), P(mean), P(rstd),
                                            BF16, ST()))
    need = lib.gmlm_layernorm_bwd_workspace_bytes(rows, f)
    assert need == blocks * 3 * f * 4

    def run(ws, nbytes):
        dx, dres = torch.empty_like(x), torch.empty_like(x)
        dg, db, dbias = (torch.empty(f, device=dev) for _ in range(3))
        ok(lib, lib.gmlm_bias_res_layernorm_bwd(P(dy), P(x), P(bias), P(res), P(gamma), P(beta), P(mean), P(rstd), rows, f, 1, 0.1, 99, None,
                                                P(dx), P(dres), P(dg), P(db), P(dbias), BF16, ws, nbytes, ST()))
        return dx, dres, dg, db, dbias
    hold(lib, dev, need, run)


B, L = 2, 70                                                      # attention: two 64-row tiles per (batch, head), the second with 6 rows


def _kv_len(dev):
    return torch.tensor([L, 41], dtype=torch.int32, device=dev)


def test_attention_bwd_streaming(lib, dev):
    h, d = 2, 64                                                  # b*h = 4 < 512: the streaming kernels (three launches, delta in the workspace)
    q, k, v, dout = (rnd(dev, (B, L, h, d), bf, seed=s) for s in (20, 21, 22, 23))
    kv = _kv_len(dev)
    out, lse = torch.empty_like(q), torch.empty(B, h, L, device=dev)
    ok(lib, lib.gmlm_attention_fwd(P(q), P(k), P(v), P(kv), B, h, L, L, d, h * d, h * d, h * d, 0.125, 0.0, 0, None, P(out), None, P(lse), BF16,
                                   None, 0, None, 0, ST()))
    need = lib.gmlm_attention_bwd_workspace_bytes(B, h, L, L, d)
    assert need == B * h * L * 4

    def run(ws, nbytes):
        dq, dk, dv = (torch.empty_like(q) for _ in range(3))
        ok(lib, lib.gmlm_attention_bwd(P(q), P(k), P(v), P(out), P(dout), P(lse), P(kv), B, h, L, L, d, h * d, h * d, h * d, 0.125, 0.0, 0, None,
                                       P(dq), P(dk), P(dv), h * d, h * d, h * d, BF16, None, 0, ws, nbytes, None, None, None, None, 0, ST()))
        return dq, dk, dv
    hold(lib, dev, need, run)


def test_attention_d128_bwd(lib, dev):
    h, d = 2, 128
    q, k, v, dout = (rnd(dev, (B, L, h, d), bf, seed=s) for s in (24, 25, 26, 27))
    kv = _kv_len(dev)
    out, lse = torch.empty_like(q), torch.empty(B, h, L, device=dev)
    ok(lib, lib.gmlm_attention_d128_fwd(P(q), P(k), P(v), P(kv), B, h, L, L, d, h * d, h * d, h * d, 0.088, 0.0, 0, None, P(out), None, P(lse),
                                        BF16, ST()))
    need = lib.gmlm_attention_d128_workspace_bytes(B, h, L)

    def run(ws, nbytes):
        dq, dk, dv = (torch.empty_like(q) for _ in range(3))
        ok(lib, lib.gmlm_attention_d128_bwd(P(q), P(k), P(v), P(out), None, P(dout), P(lse), P(kv), B, h, L, L, d, h * d, h * d, h * d, 0.088, 0.0,
                                            0, None, P(dq), P(dk), P(dv), h * d, h * d, h * d, BF16, ws, nbytes, ST()))
        return dq, dk, dv
    hold(lib, dev, need, run)


HQ, HKV = 4, 2


def test_attention_causal_bwd(lib, dev):
    q, dout = rnd(dev, (B, L, HQ, 128), bf, seed=28), rnd(dev, (B, L, HQ, 128), bf, seed=29)
    k, v = rnd(dev, (B, L, HKV, 128), bf, seed=30), rnd(dev, (B, L, HKV, 128), bf, seed=31)
    kv, qs, ks = _kv_len(dev), HQ * 128, HKV * 128
    out, lse = torch.empty_like(q), torch.empty(B, HQ, L, device=dev)
    ok(lib, lib.gmlm_attention_causal_d128_fwd(P(q), P(k), P(v), P(kv), B, HQ, HKV, L, L, 128, qs, ks, ks, 0.088, 0.0, P(out), None, P(lse), BF16,
                                               ST()))
    need = lib.gmlm_attention_causal_d128_workspace_bytes(B, HQ, L)

    def run(ws, nbytes):
        dq, dk, dv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
        ok(lib, lib.gmlm_attention_causal_d128_bwd(P(q), P(k), P(v), P(out), None, P(dout), P(lse), P(kv), B, HQ, HKV, L, L, 128, qs, ks, ks, 0.088,
                                                   0.0, P(dq), P(dk), P(dv), qs, ks, ks, BF16, ws, nbytes, ST()))
        return dq, dk, dv
    hold(lib, dev, need, run)


def test_attention_causal_varlen_bwd(lib, dev):
    cu = torch.tensor([0, 33, 33, 100], dtype=torch.int32, device=dev)       # 33 rows, an empty sequence, 67 rows (two tiles, ragged)
    seqs, max_len, rows = 3, 67, 100
    q, dout = rnd(dev, (rows, HQ, 128), bf, seed=32), rnd(dev, (rows, HQ, 128), bf, seed=33)
    k, v = rnd(dev, (rows, HKV, 128), bf, seed=34), rnd(dev, (rows, HKV, 128), bf, seed=35)
    qs, ks = HQ * 128, HKV * 128
    out, lse = torch.empty_like(q), torch.empty(HQ, rows, device=dev)
    ok(lib, lib.gmlm_attention_causal_d128_varlen_fwd(P(q), P(k), P(v), P(cu), seqs, max_len, rows, HQ, HKV, 128, qs, ks, ks, 0.088, 0.0, P(out),
                                                      None, P(lse), BF16, ST()))
    need = lib.gmlm_attention_causal_d128_varlen_workspace_bytes(rows, HQ)

    def run(ws, nbytes):
        dq, dk, dv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
        ok(lib, lib.gmlm_attention_causal_d128_varlen_bwd(P(q), P(k), P(v), P(out), None, P(dout), P(lse), P(cu), seqs, max_len, rows, HQ, HKV, 128,
                                                          qs, ks, ks, 0.088, 0.0, P(dq), P(dk), P(dv), qs, ks, ks, BF16, ws, nbytes, ST()))
        return dq, dk, dv
    hold(lib, dev, need, run)


def test_softmask_blend_bwd(lib, dev):
    dout = rnd(dev, (N, F), seed=36)
    mask = (torch.rand(N, generator=torch.Generator().manual_seed(37)) < 0.5).to(torch.uint8).to(dev)
    need = lib.gmlm_softmask_blend_bwd_workspace_bytes(N, F)
    assert need == 7 * F * 4

    def run(ws, nbytes):
        dtok = torch.empty(F, device=dev)
        ok(lib, lib.gmlm_softmask_blend_bwd(P(dout), F, P(mask), 0.7, N, F, P(dtok), ws, nbytes, ST()))
        return (dtok,)
    hold(lib, dev, need, run)


ROWS, WIDTH = 100, 264                                            # row kernels: 33 chunks of 8 bf16 (one ragged 256-lane block), 100 partial rows


def test_bias_gelu_bwd_with_dbias(lib, dev):
    dy, x, bias = rnd(dev, (ROWS, WIDTH), bf, seed=38), rnd(dev, (ROWS, WIDTH), bf, seed=39), rnd(dev, (WIDTH,), seed=40)
    need = lib.gmlm_bias_gelu_bwd_workspace_bytes(ROWS, WIDTH, BF16)
    assert need == ROWS * WIDTH * 4

    def run(ws, nbytes):
        dx, dbias = torch.empty_like(x), torch.empty(WIDTH, device=dev)
        ok(lib, lib.gmlm_bias_gelu_bwd(P(dy), P(x), P(bias), ROWS, WIDTH, 0.1, 55, None, P(dx), P(dbias), BF16, ws, nbytes, ST()))
        return dx, dbias
    hold(lib, dev, need, run)


def test_wgrad_bf16(lib, dev):
    t, n, k = 100, 256, 256                                       # three 32-token stages = three slices of the one tile, four tail rows
    dy, x = rnd(dev, (t, n), bf, seed=41), rnd(dev, (t, k), bf, seed=42)
    need = lib.gmlm_wgrad_workspace_bytes(t, n, k, 0)
    assert need == 3 * n * k * 4

    def run(ws, nbytes):
        out = torch.empty(n, k, device=dev)
        ok(lib, lib.gmlm_wgrad_bf16(P(dy), n, P(x), k, t, n, k, 0, P(out), k, 0, ws, nbytes, ST()))
        return (out,)
    hold(lib, dev, need, run)


def test_add_rmsnorm_bwd(lib, dev):
    a, b, dy, dres = (rnd(dev, (ROWS, WIDTH), bf, seed=s) for s in (43, 44, 45, 46))
    w = rnd(dev, (WIDTH,), seed=47) + 1.0
    s, y, rstd = torch.empty_like(a), torch.empty_like(a), torch.empty(ROWS, device=dev)
    ok(lib, lib.gmlm_add_rmsnorm_fwd(P(a), P(b), P(w), ROWS, WIDTH, 1e-6, P(s), P(y), P(rstd), BF16, ST()))
    need = lib.gmlm_add_rmsnorm_bwd_workspace_bytes(ROWS, WIDTH)
    assert need == 7 * WIDTH * 4

    def run(ws, nbytes):
        ds, dw = torch.empty_like(a), torch.empty(WIDTH, device=dev)
        ok(lib, lib.gmlm_add_rmsnorm_bwd(P(dy), P(dres), P(s), P(w), P(rstd), ROWS, WIDTH, P(ds), P(dw), BF16, ws, nbytes, ST()))
        return ds, dw
    hold(lib, dev, need, run)


@pytest.mark.parametrize("by_pos", [False, True])
def test_qknorm_rope_bwd(lib, dev, by_pos):
    tokens, hq, hkv, max_len = 37, 2, 1, 40                       # 111 head rows: seven blocks of 16, the last with 15
    stride, nqk = (hq + 2 * hkv) * 128, (hq + hkv) * 128
    qkv, grad = rnd(dev, (tokens, stride), bf, seed=48), rnd(dev, (tokens, stride), bf, seed=49)
    qw, kw = rnd(dev, (128,), seed=50) + 1.0, rnd(dev, (128,), seed=51) + 1.0
    ang = torch.rand(max_len, 64, generator=torch.Generator().manual_seed(52)) * 6.0
    cs = torch.stack([ang.cos(), ang.sin()], dim=1).contiguous().to(dev)                     # [max_len, 2, 64]
    pos = (torch.arange(tokens, dtype=torch.int32) * 7 % max_len).to(dev)
    out, rstd = torch.empty(tokens, nqk, dtype=bf, device=dev), torch.empty(tokens, hq + hkv, device=dev)
    if by_pos:
        ok(lib, lib.gmlm_qknorm_rope_pos_fwd(P(qkv), stride, P(qw), P(kw), P(cs), max_len, tokens, P(pos), hq, hkv, 128, 1e-6, P(out), nqk, P(rstd),
                                             BF16, ST()))
    else:
        ok(lib, lib.gmlm_qknorm_rope_fwd(P(qkv), stride, P(qw), P(kw), P(cs), max_len, tokens, tokens, hq, hkv, 128, 1e-6, P(out), nqk, P(rstd),
                                         BF16, ST()))
    need = lib.gmlm_qknorm_rope_bwd_workspace_bytes(tokens, hq, hkv, BF16)
    assert need == 7 * 256 * 4

    def run(ws, nbytes):
        dqkv, dwt = grad.clone(), torch.empty(2, 128, device=dev)                            # the backward works in place on dqkv
        if by_pos:
            ok(lib, lib.gmlm_qknorm_rope_pos_bwd(P(dqkv), stride, P(qkv), stride, P(qw), P(kw), P(cs), max_len, P(rstd), tokens, P(pos), hq, hkv,
                                                 128, P(dwt), P(dwt[1]), BF16, ws, nbytes, ST()))
        else:
            ok(lib, lib.gmlm_qknorm_rope_bwd(P(dqkv), stride, P(qkv), stride, P(qw), P(kw), P(cs), max_len, P(rstd), tokens, tokens, hq, hkv, 128,
                                             P(dwt), P(dwt[1]), BF16, ws, nbytes, ST()))
        return dqkv, dwt
    hold(lib, dev, need, run)


def test_every_workspace_entry_point_has_a_case():
    """The list of this file against the header: an entry point with a `workspace` parameter needs a test here."""
    import os
    import re
    from conftest import ROOT
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gmlm_hip.h")).read(), flags=re.S)
    takers = set(re.findall(r"\bint\s+(gmlm_[a-z0-9_]+)\s*\([^()]*\bvoid\s*\*\s*workspace\b", hdr))
    src = open(os.path.abspath(__file__)).read()
    assert len(takers) == 15 and all(f"lib.{n}(" in src for n in takers), sorted(n for n in takers if f"lib.{n}(" not in src)
