"""FusedAdamW without a device: the third header (include/gmlm_hip_optim.h) against its ctypes table and the exported symbols,
the argument contract of the three launching entries on fabricated addresses (the method of test_abi_contract_cpu.py: a call
that passes validation ends in GMLM_ELAUNCH, a refused one in GMLM_EINVAL, an empty one in GMLM_OK), the chunk plan against
brute force, the construction refusals, the harness option and the state-dict exchange with torch.optim.AdamW."""
import itertools
import os

import numpy as np
import pytest
import torch

from conftest import ROOT
from test_abi_contract_cpu import ADDR, parse_header, signature_mismatches

OK, EINVAL, ELAUNCH = 0, -1, -3
HOST_ONLY = "gmlm_adamw_chunk_elems"
LAUNCHING = ["gmlm_adamw_sumsq", "gmlm_adamw_finalize", "gmlm_adamw_update"]
no_device = pytest.mark.skipif(torch.cuda.device_count() > 0, reason="fabricated addresses: only meaningful (and only safe) without a device")


def _protos():
    return parse_header(open(os.path.join(ROOT, "include", "gmlm_hip_optim.h")).read())


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    import gmlm_amd
    return gmlm_amd.lib()


# --------------------------------------------------------------------------------------------------- header / table / symbols
def test_optim_header_table_and_symbols_agree(lib):
    from gmlm_amd import _lib
    protos = _protos()
    assert sorted(protos) == sorted([HOST_ONLY] + LAUNCHING) == sorted(_lib.SIGNATURES_OPTIM)
    assert not signature_mismatches(protos, _lib.SIGNATURES_OPTIM), signature_mismatches(protos, _lib.SIGNATURES_OPTIM)
    assert protos[HOST_ONLY] == ("int64_t", [])
    for name in LAUNCHING:
        ret, params = protos[name]
        assert ret == "int" and params[-1] == ("gmlm_stream_t", "stream"), name
        assert hasattr(lib, name) and getattr(lib, name).argtypes == _lib.SIGNATURES_OPTIM[name][1]
    # the first two headers and their tables are what they were: the new entries are in neither
    first = parse_header()
    second = parse_header(open(os.path.join(ROOT, "include", "gmlm_hip_split.h")).read())
    assert sorted(first) == sorted(_lib.SIGNATURES) and sorted(second) == sorted(_lib.SIGNATURES_SPLIT)
    assert not set(protos) & (set(first) | set(second) | set(_lib.SIGNATURES) | set(_lib.SIGNATURES_SPLIT))
    hdr = open(os.path.join(ROOT, "include", "gmlm_hip_optim.h")).read()
    assert '#include "gmlm_hip.h"' in hdr and 'extern "C"' in hdr
    mk = open(os.path.join(ROOT, "gmlm_amd", "csrc", "Makefile")).read()
    assert "optim_kernels.hip" in mk and "gmlm_hip_optim.h" in mk
    assert "optim_kernels.o:" not in mk                                        # the common flags, no per-file override
    c = lib.gmlm_adamw_chunk_elems()
    assert c >= 1024 and c % 4 == 0


# ------------------------------------------------------------------------------------------------------ argument contract
# the valid call: 3 tensors in 5 chunks, 2 groups, 4 step slots
BASE = {
    "gmlm_adamw_sumsq": dict(addr=ADDR(1), numel=ADDR(2), chunks=ADDR(3), num_chunks=5, partial=ADDR(4), nonfinite=ADDR(5), stream=None),
    "gmlm_adamw_finalize": dict(partial=ADDR(4), nonfinite=ADDR(5), num_chunks=5, max_norm=1.0, group=ADDR(6), slot=ADDR(7),
                                num_tensors=3, hyper=ADDR(8), num_groups=2, steps=ADDR(9), num_slots=4, bias_corr=ADDR(10),
                                status=ADDR(11), stream=None),
    "gmlm_adamw_update": dict(addr=ADDR(1), numel=ADDR(2), group=ADDR(6), chunks=ADDR(3), num_chunks=5, hyper=ADDR(8), num_groups=2,
                              bias_corr=ADDR(10), status=ADDR(11), stream=None),
}
POINTERS = {n: [k for k, v in b.items() if isinstance(v, int) and v >= ADDR(1)] for n, b in BASE.items()}
COUNTS = {n: [k for k in b if k.startswith("num_")] for n, b in BASE.items()}


def _expect(lib, name, rc, msg=None, **mut):
    order = [n for _, n in _protos()[name][1]]
    assert order == list(BASE[name]), (name, order)                            # the table above follows the header
    args = dict(BASE[name], **mut)
    got = getattr(lib, name)(*[args[k] for k in order])
    err = lib.gmlm_last_error()
    assert got == rc and (msg is None or msg in err), f"{name} {mut}: code {got} (want {rc}), message {err!r} (want {msg!r})"
    if rc == ELAUNCH:                                      # passed validation: the failure is the missing device, nothing else
        assert b"device" in err.lower() or b"hip" in err.lower(), (name, mut, err)


@no_device
@pytest.mark.parametrize("name", LAUNCHING)
def test_valid_calls_pass_validation(lib, name):
    _expect(lib, name, ELAUNCH)
    _expect(lib, name, ELAUNCH, stream=ADDR(20))
    _expect(lib, name, ELAUNCH, num_chunks=(1 << 31) - 1)
    for p in POINTERS[name]:
        _expect(lib, name, ELAUNCH, **{p: BASE[name][p] + 16})
    if name == "gmlm_adamw_finalize":
        for mx in (0.0, -1.0, float("inf"), float("nan")):                     # "no clipping", not a refusal
            _expect(lib, name, ELAUNCH, max_norm=mx)
        _expect(lib, name, ELAUNCH, num_tensors=4)                             # == num_slots
        _expect(lib, name, ELAUNCH, num_tensors=5, num_slots=5)                # == num_chunks


@no_device
@pytest.mark.parametrize("name", LAUNCHING)
def test_refusals_name_the_argument(lib, name):
    for p in POINTERS[name]:
        _expect(lib, name, EINVAL, b"null pointer (" + p.encode() + b")", **{p: None})
        for shift in (4, 8, 2):
            _expect(lib, name, EINVAL, p.encode() + b" must be 16-byte aligned", **{p: BASE[name][p] + shift})
    for k in COUNTS[name]:
        _expect(lib, name, EINVAL, b"negative count (" + k.encode(), **{k: -1})
    for n in (1 << 31, 1 << 40):
        _expect(lib, name, EINVAL, b"num_chunks " + str(n).encode() + b" must be below 2^31", num_chunks=n)
    if name == "gmlm_adamw_finalize":
        _expect(lib, name, EINVAL, b"exceeds num_chunks", num_tensors=6, num_slots=6)
        _expect(lib, name, EINVAL, b"exceeds num_slots", num_tensors=5)
        _expect(lib, name, EINVAL, b"num_groups is 0", num_groups=0)
        _expect(lib, name, EINVAL, b"2^31", num_slots=1 << 31)
        _expect(lib, name, EINVAL, b"2^31", num_groups=1 << 31)
    if name == "gmlm_adamw_update":
        _expect(lib, name, EINVAL, b"num_groups is 0", num_groups=0)


@no_device
@pytest.mark.parametrize("name", LAUNCHING)
def test_empty_calls_return_ok_without_pointers(lib, name):
    nothing = {p: None for p in POINTERS[name]}
    if name == "gmlm_adamw_finalize":
        _expect(lib, name, OK, num_chunks=0, num_tensors=0, **nothing)
        _expect(lib, name, OK, num_tensors=0, **nothing)
        _expect(lib, name, OK, num_chunks=0, num_tensors=0, num_groups=0, num_slots=0, **nothing)
        _expect(lib, name, EINVAL, b"exceeds num_chunks", num_chunks=0, **nothing)       # counts are checked before the empty return
    else:
        _expect(lib, name, OK, num_chunks=0, **nothing)
    if "num_groups" in BASE[name]:
        _expect(lib, name, EINVAL, b"negative count", num_chunks=0, num_groups=-1, **nothing)
    _expect(lib, name, EINVAL, b"negative count", num_chunks=-1, **nothing)


# ------------------------------------------------------------------------------------------------------------ the chunk plan
def _sizes(c):
    return [1, 3, c - 1, c, c + 1, 2 * c + 3]


def test_chunk_plan_covers_every_element_exactly_once(lib):
    from gmlm_amd import optim
    c = optim.chunk_elems()
    assert c == lib.gmlm_adamw_chunk_elems()
    lists = [[n] for n in _sizes(c)] + [list(p) for p in itertools.permutations(_sizes(c), 2)] + [_sizes(c), _sizes(c)[::-1],
                                                                                                   [c, c, c], [1, 1, 2 * c + 3, 1]]
    for numels in lists:
        plan = optim.chunk_plan(numels)
        assert plan.dtype == np.int32 and plan.ndim == 2 and plan.shape[1] == 2
        assert plan.shape[0] == sum(-(-n // c) for n in numels), numels
        cover = [np.zeros(n, np.int32) for n in numels]                       # brute force: count every element's visits
        for t, k in plan.tolist():
            lo, hi = k * c, min((k + 1) * c, numels[t])
            assert 0 <= lo < hi, (numels, t, k)                               # no empty chunk, none past the end
            cover[t][lo:hi] += 1
        assert all(bool((v == 1).all()) for v in cover), numels
        keys = [tuple(r) for r in plan.tolist()]
        assert keys == sorted(keys), numels                                    # tensor-major, chunks ascending inside a tensor
    assert optim.chunk_plan([]).shape == (0, 2)
    with pytest.raises(ValueError):
        optim.chunk_plan([4, 0, 4])
    with pytest.raises(ValueError, match="31 bits"):
        optim.chunk_plan([c * (1 << 31)])
    assert optim.chunk_plan([10, 5], chunk=4).tolist() == [[0, 0], [0, 1], [0, 2], [1, 0], [1, 1]]


# ------------------------------------------------------------------------------------------------------------- construction
def test_construction_refusals():
    import gmlm_amd
    p = torch.nn.Parameter(torch.zeros(4, 6))
    opt = gmlm_amd.FusedAdamW([p], lr=1e-3, betas=(0.9, 0.99), eps=1e-6, weight_decay=0.1)
    assert isinstance(opt, torch.optim.Optimizer) and opt.last_grad_norm is None and opt.skipped_steps() == 0
    g = opt.param_groups[0]
    assert (g["lr"], g["betas"], g["eps"], g["weight_decay"]) == (1e-3, (0.9, 0.99), 1e-6, 0.1)
    with pytest.raises(ValueError, match="amsgrad"):
        gmlm_amd.FusedAdamW([p], amsgrad=True)
    with pytest.raises(ValueError, match="maximize"):
        gmlm_amd.FusedAdamW([p], maximize=True)
    with pytest.raises(ValueError, match="amsgrad"):
        gmlm_amd.FusedAdamW([{"params": [p], "amsgrad": True}])
    for dt in (torch.bfloat16, torch.float16, torch.float64):
        with pytest.raises(ValueError, match="float32"):
            gmlm_amd.FusedAdamW([torch.nn.Parameter(torch.zeros(4, dtype=dt))])
    with pytest.raises(ValueError, match="contiguous"):
        gmlm_amd.FusedAdamW([torch.nn.Parameter(torch.zeros(6, 4).t())])
    with pytest.raises(ValueError, match="one device"):
        gmlm_amd.FusedAdamW([p, torch.nn.Parameter(torch.zeros(3, device="meta"))])
    with pytest.raises(ValueError, match="one device"):
        gmlm_amd.FusedAdamW([{"params": [p]}, {"params": [torch.nn.Parameter(torch.zeros(3, device="meta"))]}])
    for bad in (dict(lr=-1.0), dict(eps=-1.0), dict(betas=(1.0, 0.9)), dict(betas=(0.9, -0.1)), dict(weight_decay=-0.1)):
        with pytest.raises(ValueError, match="Invalid"):
            gmlm_amd.FusedAdamW([p], **bad)
    # there is no CPU path: a step on CPU parameters is an error, not a fallback
    p.grad = torch.ones_like(p)
    with pytest.raises(gmlm_amd.GmlmHipError, match="GPU only"):
        opt.step(max_grad_norm=1.0)
    assert bool((p == 0).all()) and not opt.state[p]


# ----------------------------------------------------------------------------------------------------------------- harness
def _tiny_model():
    from transformers import BertConfig, BertModel
    import gmlm_amd
    enc = BertModel(BertConfig(vocab_size=200, hidden_size=64, num_hidden_layers=2, num_attention_heads=4, intermediate_size=128,
                               max_position_embeddings=64))
    return gmlm_amd.GraphTextLM(32, 16, 5, plm_encoder=enc)


def test_setup_optimizer_fused_has_the_same_three_groups():
    import inspect
    import gmlm_amd
    from gmlm_amd import harness
    sig = inspect.signature(harness.setup_optimizer)
    assert sig.parameters["fused"].default is False
    m = _tiny_model()
    stock = harness.setup_optimizer(m, 1e-3, 1e-5, 1e-4, 0.02)
    assert type(stock) is torch.optim.AdamW
    fused = harness.setup_optimizer(m, 1e-3, 1e-5, 1e-4, 0.02, fused=True)
    assert isinstance(fused, gmlm_amd.FusedAdamW) and gmlm_amd.FusedAdamW is gmlm_amd.optim.FusedAdamW
    assert len(fused.param_groups) == len(stock.param_groups) == 3
    for a, b in zip(fused.param_groups, stock.param_groups):
        assert len(a["params"]) == len(b["params"]) > 0
        assert all(x is y for x, y in zip(a["params"], b["params"]))
        assert (a["lr"], a["weight_decay"], a["betas"], a["eps"]) == (b["lr"], b["weight_decay"], b["betas"], b["eps"])
        assert list(a) == list(b)                                              # the same keys: a state dict loads either way
    assert [g["lr"] for g in fused.param_groups] == [1e-3, 1e-5, 1e-4] and [g["weight_decay"] for g in fused.param_groups] == [0.02, 0.01, 0.02]
    # LR schedulers drive it like any optimiser
    sched = harness.linear_warmup_schedule(fused, 2, 10)
    assert [g["lr"] for g in fused.param_groups] == [0.0, 0.0, 0.0]
    assert sched.get_last_lr() == [0.0, 0.0, 0.0]


# ---------------------------------------------------------------------------------------------------------------- state dict
def test_state_dict_moves_between_stock_adamw_and_fused():
    import gmlm_amd
    gen = torch.Generator().manual_seed(3)
    shapes = [(5, 3), (7,), (2, 2, 2)]

    def params():
        g = torch.Generator().manual_seed(1)
        return [torch.nn.Parameter(torch.randn(s, generator=g)) for s in shapes]

    def groups(ps):
        return [{"params": ps[:2], "lr": 1e-2, "weight_decay": 0.1}, {"params": ps[2:], "lr": 1e-3, "weight_decay": 0.0}]

    ps = params()
    stock = torch.optim.AdamW(groups(ps))
    for _ in range(2):
        for p in ps:
            p.grad = torch.randn(p.shape, generator=gen)
        stock.step()
    sd = stock.state_dict()

    fused = gmlm_amd.FusedAdamW(groups(params()))
    fused.load_state_dict(sd)
    fp = [p for g in fused.param_groups for p in g["params"]]
    for i, p in enumerate(fp):
        st = fused.state[p]
        assert float(st["step"]) == 2.0
        assert torch.equal(st["exp_avg"], sd["state"][i]["exp_avg"]) and torch.equal(st["exp_avg_sq"], sd["state"][i]["exp_avg_sq"])
        assert st["exp_avg"].dtype == torch.float32 and st["exp_avg"].is_contiguous() and st["exp_avg"].shape == p.shape
    assert [g["lr"] for g in fused.param_groups] == [1e-2, 1e-3]

    back = fused.state_dict()
    assert back["param_groups"] == sd["param_groups"]
    stock2 = torch.optim.AdamW(groups(params()))
    stock2.load_state_dict(back)
    sp = [p for g in stock2.param_groups for p in g["params"]]
    for i, p in enumerate(sp):
        st = stock2.state[p]
        assert float(st["step"]) == 2.0 and set(st) == {"step", "exp_avg", "exp_avg_sq"}
        assert torch.equal(st["exp_avg"], sd["state"][i]["exp_avg"]) and torch.equal(st["exp_avg_sq"], sd["state"][i]["exp_avg_sq"])
    # and the loaded stock optimiser still steps (the state has the types it expects)
    for p in sp:
        p.grad = torch.ones_like(p)
    stock2.step()
    assert all(float(stock2.state[p]["step"]) == 3.0 for p in sp)
