"""gmlm_amd.FusedAdamW (clip + AdamW as one multi-tensor step, include/gmlm_hip_optim.h) on the device.

Truth: the same recipe, ``clip_grad_norm_`` + ``torch.optim.AdamW``, in float64 on the CPU.  Yardstick: that recipe in fp32 on the
device (torch's for-each kernels).  The parity bound, per tensor and for p, m and v each:
    max|fused - truth| <= max(2 x max|stock fp32 - truth|, 4 fp32 ulps of the tensor's largest magnitude)
- both are fp32 evaluations of one formula in different operation orders, hence the factor 2; the ulp floor covers tensors on
which the stock run happens to be exact.  All sizes derive from C, the chunk size read from the library."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

MAX_NORM = 1.0
GROUPS = [dict(lr=1e-2, weight_decay=0.1), dict(lr=3e-3, weight_decay=0.0)]
SCALES = [0.1, 1e-4, 0.1, 1e-4, 0.1, 1e-4]     # global gradient norm ~ 40 and ~ 0.04: the clipped and the unclipped branch


def shapes():
    from gmlm_amd import optim
    c = optim.chunk_elems()
    return [(1,), (3,), (4,), (5,), (c - 1,), (c,), (c + 1,), (2 * c + 3,), (7, 9)]


def group_of(i):
    return i % 2


def make_case(seed=0, steps=6):
    g = torch.Generator().manual_seed(seed)
    init = [torch.randn(s, generator=g) for s in shapes()]
    grads = [[torch.randn(s, generator=g) * SCALES[k % len(SCALES)] for s in shapes()] for k in range(steps)]
    return init, grads


def _groups(params):
    return [dict(params=[p for i, p in enumerate(params) if group_of(i) == gi], **hp) for gi, hp in enumerate(GROUPS)]


def run_stock(init, grads, dtype, device, max_norm=MAX_NORM, has_grad=lambda step, i: True):
    """clip_grad_norm_ + torch.optim.AdamW.  Returns (p, m, v, step) per tensor as float64 CPU (None without state) and the norms."""
    params = [torch.nn.Parameter(t.to(device=device, dtype=dtype)) for t in init]
    opt = torch.optim.AdamW(_groups(params))
    norms = []
    for k, gs in enumerate(grads):
        for i, (p, g) in enumerate(zip(params, gs)):
            p.grad = g.to(device=device, dtype=dtype) if has_grad(k, i) else None
        with_grad = [p for p in params if p.grad is not None]
        if max_norm is not None:
            norms.append(float(torch.nn.utils.clip_grad_norm_(with_grad, max_norm)))
        else:
            norms.append(float(torch.linalg.vector_norm(torch.stack([p.grad.norm() for p in with_grad]))))
        opt.step()
    out = []
    for p in params:
        st = opt.state.get(p)
        out.append((p.detach().double().cpu(),) + ((st["exp_avg"].double().cpu(), st["exp_avg_sq"].double().cpu(), int(st["step"]))
                                                   if st else (None, None, None)))
    return out, norms


def fused_setup(init, offset=0):
    """Parameters on the device and a FusedAdamW over them; ``offset`` = 1: every parameter and moment is the view
    buf[1 : 1 + n] of a larger buffer (4-byte aligned only)."""
    import gmlm_amd
    dev = torch.device("cuda:0")

    def place(t):
        if not offset:
            return t.to(dev).clone()
        buf = torch.empty(t.numel() + 2 * offset, device=dev)
        view = buf[offset:offset + t.numel()].view(t.shape)
        view.copy_(t)
        assert view.data_ptr() % 16 == 4 * offset and view.is_contiguous()
        return view

    params = [torch.nn.Parameter(place(t)) for t in init]
    opt = gmlm_amd.FusedAdamW(_groups(params))
    if offset:
        for p in params:
            opt.state[p] = dict(step=torch.tensor(0.0), exp_avg=place(torch.zeros(p.shape)), exp_avg_sq=place(torch.zeros(p.shape)))
    return params, opt, place


def snapshot(params, opt):
    """(p, m, v, step) per tensor, fp32 on the CPU, the steps as state_dict() reports them."""
    sd = opt.state_dict()["state"]
    index = {id(p): j for j, p in enumerate(q for gp in opt.param_groups for q in gp["params"])}     # state_dict numbers them by group
    out = []
    for p in params:
        st = sd.get(index[id(p)])
        out.append((p.detach().cpu().clone(),) + ((st["exp_avg"].cpu().clone(), st["exp_avg_sq"].cpu().clone(), int(st["step"]))
                                                  if st else (None, None, None)))
    return out


def run_fused(init, grads, max_norm=MAX_NORM, offset=0, has_grad=lambda step, i: True):
    params, opt, place = fused_setup(init, offset)
    norms = []
    for k, gs in enumerate(grads):
        for i, (p, g) in enumerate(zip(params, gs)):
            p.grad = place(g) if has_grad(k, i) else None
        opt.step(max_grad_norm=max_norm)
        assert opt.last_grad_norm.dim() == 0 and opt.last_grad_norm.is_cuda
        norms.append(opt.last_grad_norm.item())
    assert all(p.grad is None or torch.equal(p.grad.cpu(), g) for p, g in zip(params, grads[-1]))   # .grad is read, never scaled
    assert opt.skipped_steps() == 0
    return snapshot(params, opt), norms


def ulp(x):
    return float(np.spacing(np.float32(x)))


def assert_parity(fused, stock, truth, what=""):
    worst = 0.0
    for i, (f, s, t) in enumerate(zip(fused, stock, truth)):
        assert (f[1] is None) == (t[1] is None) == (s[1] is None), (what, i)
        assert f[3] == t[3] == s[3], (what, i, f[3], s[3], t[3])                 # step counts
        for name, a, b, c in zip("pmv", f[:3], s[:3], t[:3]):
            if c is None:
                continue
            e_f, e_s = float((a.double() - c).abs().max()), float((b - c).abs().max())
            bound = max(2.0 * e_s, 4.0 * ulp(float(c.abs().max())))
            worst = max(worst, e_f / bound)
            print(f"{what} tensor {i} {tuple(c.shape)} {name}: fused {e_f:.3e} stock {e_s:.3e} bound {bound:.3e}")
            assert e_f <= bound, (what, i, name, e_f, e_s, bound)
    print(f"{what}: worst fused error / bound = {worst:.3f}")


def bitwise(a, b):
    for i, (x, y) in enumerate(zip(a, b)):
        assert x[3] == y[3], i
        for name, u, w in zip("pmv", x[:3], y[:3]):
            assert (u is None) == (w is None) and (u is None or torch.equal(u.view(torch.int32), w.view(torch.int32))), (i, name)


@pytest.fixture(scope="module")
def case():
    return make_case()


@pytest.fixture(scope="module")
def clipped(case):
    """The six-step run shared by the parity, alignment and determinism tests: float64 truth, fp32 stock on the device, fused."""
    init, grads = case
    dev = torch.device("cuda:0")
    truth, tn = run_stock(init, grads, torch.float64, "cpu")
    stock, _ = run_stock(init, grads, torch.float32, dev)
    fused, fn = run_fused(init, grads)
    return dict(truth=truth, truth_norms=tn, stock=stock, fused=fused, fused_norms=fn)


def test_parity_with_float64_clip_and_adamw(clipped):
    tn = clipped["truth_norms"]
    assert all(n > 10 * MAX_NORM for n in tn[0::2]) and all(n < 0.1 * MAX_NORM for n in tn[1::2])   # both branches did run
    assert_parity(clipped["fused"], clipped["stock"], clipped["truth"], "clipped")
    for k, (a, b) in enumerate(zip(clipped["fused_norms"], tn)):
        print(f"step {k}: grad norm fused {a:.9g} float64 {b:.9g} rel {abs(a - b) / b:.2e}")
        assert abs(a - b) <= 1e-6 * b, (k, a, b)


def test_views_at_a_4_byte_offset_give_the_same_bits(case, clipped):
    init, grads = case
    shifted, norms = run_fused(init, grads, offset=1)
    bitwise(shifted, clipped["fused"])
    assert norms == clipped["fused_norms"]


def test_two_runs_are_bit_identical(case, clipped):
    init, grads = case
    again, norms = run_fused(init, grads)
    bitwise(again, clipped["fused"])
    assert norms == clipped["fused_norms"]


def test_without_clipping(case):
    init, grads = case
    dev = torch.device("cuda:0")
    truth, tn = run_stock(init, grads[:3], torch.float64, "cpu", max_norm=None)
    stock, _ = run_stock(init, grads[:3], torch.float32, dev, max_norm=None)
    fused, fn = run_fused(init, grads[:3], max_norm=None)
    assert_parity(fused, stock, truth, "no clip")
    assert all(abs(a - b) <= 1e-6 * b for a, b in zip(fn, tn)), (fn, tn)        # the norm is still reported


def test_missing_gradients(case):
    """Tensor 5 (C elements) has no gradient in steps 2 and 4, tensor 2 never has one."""
    init, grads = case
    dev = torch.device("cuda:0")
    has = lambda step, i: not (i == 2 or (i == 5 and step in (1, 3)))
    truth, _ = run_stock(init, grads, torch.float64, "cpu", has_grad=has)
    stock, _ = run_stock(init, grads, torch.float32, dev, has_grad=has)
    fused, _ = run_fused(init, grads, has_grad=has)
    assert fused[5][3] == stock[5][3] == 4 and fused[0][3] == 6
    assert fused[2][1] is None and fused[2][3] is None and torch.equal(fused[2][0], init[2])      # never a gradient: no state
    assert_parity(fused, stock, truth, "missing gradients")


def test_non_finite_gradients_skip_the_step(case):
    init, grads = case
    dev = torch.device("cuda:0")
    params, opt, place = fused_setup(init)

    def step(gs):
        for p, g in zip(params, gs):
            p.grad = place(g)
        opt.step(max_grad_norm=MAX_NORM)

    step(grads[0])
    step(grads[1])
    before = snapshot(params, opt)
    assert opt.skipped_steps() == 0 and all(b[3] == 2 for b in before)
    c = shapes()[5][0]
    bad_inf = [g.clone() for g in grads[2]]
    bad_inf[7][c + 17] = float("inf")                        # inside the second chunk of the 2 C + 3 tensor
    bad_nan = [g.clone() for g in grads[2]]
    bad_nan[-1].view(-1)[-1] = float("nan")                  # the last element of the last chunk (a tail lane: 63 = 4 * 15 + 3)
    for n, bad in enumerate((bad_inf, bad_nan), 1):
        step(bad)
        bitwise(snapshot(params, opt), before)               # p, m, v and the reported steps: not a bit has moved
        assert opt.skipped_steps() == n
        assert not np.isfinite(opt.last_grad_norm.item())
    step(grads[2])                                           # the next clean step: the third step of a run that never saw the bad ones
    assert opt.skipped_steps() == 2
    truth, _ = run_stock(init, grads[:3], torch.float64, "cpu")
    stock, _ = run_stock(init, grads[:3], torch.float32, dev)
    assert_parity(snapshot(params, opt), stock, truth, "after two skipped steps")


def test_harness_train_step_with_the_fused_optimizer():
    """Three harness.train_step on the tiny model (the g4_bert_tiny encoder geometry: hidden 64, 2 layers, 4 heads, FFN 128; built
    like test_gpu_harness.py builds its model), fp32, dropout off, warm-up schedule, once with setup_optimizer(fused=True) and once
    with the stock optimiser from equal weights: the loss trajectories agree to the bar test_gpu_harness.py uses against its oracle
    (first step 1e-4, all steps 2e-3).

    The parameters are held to the parity bound, which needs a truth: the two device runs cannot serve as each other's, because
    some gradients are rounding noise around an exact zero (the key bias of softmax attention) and AdamW turns such noise into
    steps of +-lr.  So the fused run's own gradients and learning rates are recorded step by step and replayed through the recipe,
    clip_grad_norm_ + AdamW with the same three groups, in float64 on the CPU (truth) and in fp32 on the device (yardstick)."""
    import gmlm_amd
    import gmlm_oracle as O
    from gmlm_amd import harness
    from test_gpu_model import build_model
    dev = torch.device("cuda:0")
    plm = dict(hidden=64, layers=2, heads=4, inter=128, max_pos=64, vocab=200)
    n, e = 150, 700
    cfg = dict(n=n, e=e, f_in=48, hc=32, c=4, plm=plm, seed=31)
    g = torch.Generator().manual_seed(8)
    x, ei = torch.randn(n, 48, generator=g).to(dev), torch.randint(0, n, (2, e), generator=g).to(dev)
    y = torch.randint(0, 4, (n,), generator=g).to(dev)
    masks = [(torch.rand(n, generator=g) < 0.4).to(dev) for _ in range(3)]
    ids, am = O.synthetic_tokens(n, 12, 200, 3, 2)
    tokens = gmlm_amd.TokenizedTexts.from_mask(ids.to(dev), am.to(dev))
    lrs = dict(lr_graph=1e-3, lr_bert=1e-4, lr_other=5e-4, weight_decay=0.01)

    def run(fused):
        m = build_model(cfg, dev)
        opt = harness.setup_optimizer(m, fused=fused, **lrs)
        assert isinstance(opt, gmlm_amd.FusedAdamW) == fused
        sched = harness.linear_warmup_schedule(opt, 1, 10)
        params = [p for gp in opt.param_groups for p in gp["params"]]
        rec = dict(init=[p.detach().clone() for p in params], grads=[], lrs=[], losses=[])
        for mk in masks:
            rec["lrs"].append([gp["lr"] for gp in opt.param_groups])
            r = harness.train_step(m, opt, sched, x, ei, tokens, y, mk, beta=0.7, plm_batch_size=64, autocast=False)
            assert not r.skipped
            rec["losses"].append(r.loss)
            rec["grads"].append([None if p.grad is None else p.grad.detach().clone() for p in params])
        rec["params"], rec["opt"] = params, opt
        return rec

    stock, fused = run(False), run(True)
    assert all(torch.equal(a, b) for a, b in zip(stock["init"], fused["init"]))
    print(f"losses stock {stock['losses']} fused {fused['losses']}")
    assert abs(fused["losses"][0] - stock["losses"][0]) < 1e-4
    np.testing.assert_allclose(fused["losses"], stock["losses"], rtol=0, atol=2e-3)
    opt = fused["opt"]
    assert opt.skipped_steps() == 0 and float(opt.last_grad_norm) > 0
    sizes = [len(gp["params"]) for gp in opt.param_groups]

    def replay(dtype, device):
        ps = [torch.nn.Parameter(t.to(device=device, dtype=dtype)) for t in fused["init"]]
        groups, at = [], 0
        for gp, k in zip(opt.param_groups, sizes):
            groups.append(dict(params=ps[at:at + k], lr=gp["lr"], weight_decay=gp["weight_decay"]))
            at += k
        ro = torch.optim.AdamW(groups)
        for gs, lr in zip(fused["grads"], fused["lrs"]):
            for gp, v in zip(ro.param_groups, lr):
                gp["lr"] = v
            for p, gr in zip(ps, gs):
                p.grad = None if gr is None else gr.to(device=device, dtype=dtype)
            torch.nn.utils.clip_grad_norm_([p for p in ps if p.grad is not None], 1.0)
            ro.step()
        return [p.detach().double().cpu() for p in ps]

    truth, yard = replay(torch.float64, "cpu"), replay(torch.float32, dev)
    moved = 0
    for i, (p, t, s, p0) in enumerate(zip(fused["params"], truth, yard, fused["init"])):
        e_f, e_s = float((p.detach().double().cpu() - t).abs().max()), float((s - t).abs().max())
        bound = max(2.0 * e_s, 4.0 * ulp(float(t.abs().max())))
        assert e_f <= bound, (i, tuple(p.shape), e_f, e_s, bound)
        moved += int(not torch.equal(p.detach(), p0))
    assert moved > len(truth) // 2                             # the optimiser did move the model
    st = opt.state_dict()["state"]
    assert st and all(int(v["step"]) == 3 for v in st.values())
