"""Host side of the band-limited grouped-KV attention at head dim 256 (no GPU needed): the fourteenth header
(include/gmlm_hip_gqa_band.h), its ctypes table ``_lib.SIGNATURES_GQA_BAND`` and the exported symbols agree type by type, the
table sitting strictly inside ``SIGNATURE_TABLES_LATER`` and sharing no name with any other; the four argument lists are those of
their ``gmlm_attention_gqa_d256_*`` namesakes plus ``window`` after ``causal``; the Makefile names the source and the header; the
entry points refuse a window outside [1, 2^30) after every refusal of the namesake that is documented before it, and return
GMLM_OK for an empty call without pointers; the Gemma3 encoder passes ``window = sliding_window`` to the band entry points on the
sliding layers of a call past the window when ``band=True`` and calls the un-banded entry points everywhere else; the two new
autograd nodes keep the frozen-input contract; and HF's own ``sliding_attention`` masks are the rule the header states."""
import os
import re

import pytest
import torch

from conftest import ROOT
from gmlm_amd import _lib, dense, gemma3, ops, ops_gemma
from test_abi_contract_cpu import parse_header, signature_mismatches
from test_attention_routes_cpu import Recorder, STREAM
from test_autograd_contract_cpu import Case, _cu, _gen, _pos, _r, assert_contract, patterns, rope_table, run_pattern

OK, EINVAL, EWORKSPACE, ELAUNCH = 0, -1, -2, -3
F32, BF16 = 0, 1
A = 0x10000000        # fabricated, non-null, 16-byte aligned: every call below ends before or at the launch
HEADER = os.path.join(ROOT, "include", "gmlm_hip_gqa_band.h")
STEM, OLD = "gmlm_attention_gqa_d256_band", "gmlm_attention_gqa_d256"
TAILS = ("_fwd", "_bwd", "_bwd_workspace_bytes", "_varlen_fwd", "_varlen_bwd", "_varlen_bwd_workspace_bytes")

no_device = pytest.mark.skipif(torch.cuda.device_count() > 0,
                               reason="fabricated addresses: only meaningful (and only safe) without a device")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libgmlm_hip.so not built")
    return _lib.lib()


# ------------------------------------------------------------------------------------------------------------------ ABI
def test_header_ctypes_table_and_exports_agree(lib):
    table = _lib.SIGNATURES_GQA_BAND
    protos = parse_header(open(HEADER).read())
    assert sorted(protos) == sorted(STEM + t for t in TAILS) and len(protos) == 6
    assert not signature_mismatches(protos, table)
    for name in protos:
        assert hasattr(lib, name), f"{name} declared in include/gmlm_hip_gqa_band.h but not exported"
        assert getattr(lib, name).argtypes == table[name][1]                                  # lib() bound the new table
    later = _lib.SIGNATURE_TABLES_LATER
    assert later[0] is _lib.SIGNATURES_RELBIAS and later[-1] is _lib.SIGNATURES_DISENT
    assert any(t is table for t in later[1:-1])                                                # strictly inside
    assert not any(t is table for t in _lib.SIGNATURE_TABLES)
    others = set().union(*(set(t) for t in _lib.SIGNATURE_TABLES + later if t is not table))
    assert not set(table) & others
    assert lib.gmlm_version() == 1
    text = open(HEADER).read()
    assert '#include "gmlm_hip.h"' in text and 'extern "C"' in text
    wide = parse_header(open(os.path.join(ROOT, "include", "gmlm_hip_gqa_wide.h")).read())
    assert not set(wide) & set(protos) and len(wide) == 16                                     # the thirteenth header is as it was


def _names(protos, name):
    return [n for _, n in protos[name][1]]


def test_argument_lists_are_the_namesakes_plus_window_after_causal():
    wide = parse_header(open(os.path.join(ROOT, "include", "gmlm_hip_gqa_wide.h")).read())
    protos = parse_header(open(HEADER).read())
    for tail in ("_fwd", "_bwd", "_varlen_fwd", "_varlen_bwd"):
        old, new = wide[OLD + tail], protos[STEM + tail]
        i = _names(wide, OLD + tail).index("causal") + 1
        assert new[0] == old[0] and new[1] == old[1][:i] + [("int64_t", "window")] + old[1][i:], tail
    for tail in ("_bwd_workspace_bytes", "_varlen_bwd_workspace_bytes"):
        assert protos[STEM + tail] == wide[OLD + tail]


def test_the_makefile_names_the_new_source_and_header():
    mk = open(os.path.join(ROOT, "gmlm_amd", "csrc", "Makefile")).read()
    srcs = re.search(r"^SRCS\s*=(.*)$", mk, re.M).group(1).split()
    assert "attn_gqa_band.hip" in srcs and os.path.exists(os.path.join(ROOT, "gmlm_amd", "csrc", "attn_gqa_band.hip"))
    assert "../../include/gmlm_hip_gqa_band.h" in re.search(r"^\$\(BUILD\)/%\.o:(.*)$", mk, re.M).group(1).split()


# ------------------------------------------------------------------------------------------------- entry-point refusals
W = 1280 + 8        # (3 + 2) heads of 256 and 8 more: the fused rows are wider than [q | k | v]
_BASE = dict(q=A, k=A, v=A, kv_len=None, b=2, hq=3, hkv=1, lq=64, lk=64, d=256, q_stride=W, k_stride=W, v_stride=W, scale=0.0625,
             dropout_p=0.0, causal=1, window=40, out=A, out_lo=None, lse=A, dtype=BF16, stream=None, dout=A, dq=A, dk=A, dv=A, dq_stride=W,
             dk_stride=W, dv_stride=W, workspace=A, workspace_bytes=1 << 40, cu_seqlens=A, num_seqs=2, max_len=64, total_rows=100)
_LISTS = {w: _names(parse_header(open(HEADER).read()), f"{STEM}_{w}") for w in ("fwd", "bwd", "varlen_fwd", "varlen_bwd")}
WHICH = tuple(_LISTS)
BAD_WINDOWS = (0, -1, 1 << 30)


def _call(lib, which, **mut):
    a = dict(_BASE, **mut)
    return getattr(lib, f"{STEM}_{which}")(*[a[n] for n in _LISTS[which]]), lib.gmlm_last_error()


# the namesake's refusals that its header documents BEFORE the scale check, in that order; each is still decided first when the
# window is bad as well, and each later one only when every earlier argument is good
_BEFORE = [(dict(hq=0), b"bad sizes"), (dict(d=128), b"head dim"), (dict(dtype=2), b"dtype"), (dict(out_lo=A, dtype=F32), b"out_lo"),
           (dict(lq=63), b"lq == lk"), (dict(hq=3, hkv=2), b"multiple of"), (dict(dropout_p=0.1), b"dropout"), (dict(scale=0.0), b"scale")]
# and those documented after it, which a bad window now precedes
_AFTER = [(dict(b=(1 << 31) // 3 + 1, lq=1, lk=1, num_seqs=(1 << 31) // 3 + 1, max_len=1), b"too many work items"),
          (dict(q_stride=760), b"stride"), (dict(q=A + 8), b"aligned"), (dict(k=None), b"null")]
_PACKED_FIRST = [(dict(cu_seqlens=None), b"cu_seqlens"), (dict(max_len=0), b"max_len"), (dict(total_rows=-1), b"packed rows")]


@no_device
@pytest.mark.parametrize("which", WHICH)
def test_window_refusals_and_their_place_in_the_order(lib, which):
    packed = which.startswith("varlen")
    for w in BAD_WINDOWS:
        rc, err = _call(lib, which, window=w)
        assert rc == EINVAL and b"window" in err and b"[1, 2^30)" in err, (w, rc, err)
    for w in (1, 2, 257, (1 << 30) - 1):
        assert _call(lib, which, window=w)[0] == ELAUNCH, w                                   # valid: ends at the launch (no device)
    before = [(m, msg) for m, msg in _BEFORE if not (packed and "lq" in m)] + (_PACKED_FIRST if packed else [])
    for i, (mut, msg) in enumerate(before):
        for w in (40, 0):
            rc, err = _call(lib, which, window=w, **mut)
            assert rc == EINVAL and msg in err, (mut, w, rc, err)
    order = [m for m, _ in _BEFORE if not (packed and "lq" in m)]
    for i, (mut, msg) in enumerate(_BEFORE):                            # the documented order among the namesake's own refusals
        if packed and "lq" in mut:
            continue
        later = {}
        for m, _ in _BEFORE[i + 1:]:
            if not (packed and "lq" in m) and not set(m) & set(mut):
                later.update(m)
        rc, err = _call(lib, which, window=0, **later, **mut)
        assert rc == EINVAL and msg in err, (mut, later, rc, err)
    assert order
    for mut, msg in _AFTER:
        rc, err = _call(lib, which, **mut)
        assert rc == EINVAL and msg in err, (mut, rc, err)
        rc, err = _call(lib, which, window=0, **mut)
        assert rc == EINVAL and b"window" in err, (mut, rc, err)
    if which.endswith("bwd"):
        assert _call(lib, which, workspace=None)[0] == EWORKSPACE and _call(lib, which, workspace=None, window=0)[0] == EINVAL


@no_device
def test_nothing_to_do_needs_no_pointer_but_sizes_and_window_are_still_checked(lib):
    nothing = dict(q=None, k=None, v=None, out=None, lse=None, dout=None, dq=None, dk=None, dv=None, workspace=None, workspace_bytes=0)
    for which, empties in (("fwd", (dict(b=0), dict(lq=0, lk=0))), ("bwd", (dict(b=0), dict(lq=0, lk=0))),
                           ("varlen_fwd", (dict(num_seqs=0), dict(total_rows=0))), ("varlen_bwd", (dict(num_seqs=0), dict(total_rows=0)))):
        for empty in empties:
            assert _call(lib, which, **nothing, **empty)[0] == OK, (which, empty)
            for mut, msg in ((dict(d=128), b"head dim"), (dict(dropout_p=0.5), b"dropout"), (dict(dtype=5), b"dtype"), (dict(window=0), b"window"),
                             (dict(window=1 << 30), b"window")):
                rc, err = _call(lib, which, **nothing, **empty, **mut)
                assert rc == EINVAL and msg in err, (which, empty, mut, rc, err)
    assert lib.gmlm_attention_gqa_d256_band_bwd_workspace_bytes(2, 3, 300) == lib.gmlm_attention_gqa_d256_bwd_workspace_bytes(2, 3, 300)
    assert lib.gmlm_attention_gqa_d256_band_varlen_bwd_workspace_bytes(100, 3) == 3 * 100 * 4


def test_new_ops_fail_loudly_without_a_gpu(lib):
    """CPU tensors raise the library's error: no eager fallback behind the new operators."""
    q, k = torch.zeros(1, 4, 768), torch.zeros(1, 4, 256)
    with pytest.raises(_lib.GmlmHipError):
        ops.gqa_d256_band_attention(q, k, k, None, 3, 1, 0.0625, True, 2)
    with pytest.raises(_lib.GmlmHipError):
        ops.gqa_d256_band_attention_varlen(q[0], k[0], k[0], torch.tensor([0, 4], dtype=torch.int32), 4, 3, 1, 0.0625, False, 2)
    with pytest.raises(_lib.GmlmHipError):
        ops.rope_gqa_d256(torch.zeros(1, 4, 1280), torch.zeros(256), torch.zeros(256), torch.zeros(8, 2, 128), None, 3, 1, 0.0625, True, window=2)
    for w in BAD_WINDOWS:
        with pytest.raises(ValueError, match="window"):
            ops.gqa_d256_band_attention(q, k, k, None, 3, 1, 0.0625, True, w)


# -------------------------------------------------------------------------------------------------------- host routing
@pytest.fixture
def rec(monkeypatch):
    """The recorder lib of test_attention_routes_cpu.py behind ops.py and ops_gemma.py; GEMMs run in fp32 on the host."""
    r = Recorder()
    for mod in (ops, ops_gemma):
        monkeypatch.setattr(mod, "lib", lambda: r)
        monkeypatch.setattr(mod, "check", lambda rc, what="": r.checked.append(what))
    monkeypatch.setattr(ops, "_cuda", lambda *ts: None)
    monkeypatch.setattr(ops, "_stream", lambda: STREAM)
    monkeypatch.setattr(ops, "SEED_DEVICE", None)

    def f32_out(op, *args, out=None, **kw):
        res = getattr(torch, op)(*[a.float() for a in args])
        return res if out is None else out.copy_(res)
    monkeypatch.setattr(dense, "_f32_out", f32_out)
    return r


def _tiny(bidir, window=8):
    from transformers import Gemma3TextConfig, Gemma3TextModel
    torch.manual_seed(0)
    cfg = Gemma3TextConfig(vocab_size=96, hidden_size=96, intermediate_size=64, num_hidden_layers=3, num_attention_heads=3,
                           num_key_value_heads=1, head_dim=256, max_position_embeddings=64, sliding_window=window, sliding_window_pattern=3,
                           pad_token_id=0, use_bidirectional_attention=bidir)
    return Gemma3TextModel(cfg)


def _attention_calls(rec):
    protos = parse_header(open(HEADER).read())
    protos.update(parse_header(open(os.path.join(ROOT, "include", "gmlm_hip_gqa_wide.h")).read()))
    out = []
    for name, args in rec.take():
        if name.startswith("gmlm_attention") and not name.endswith("workspace_bytes"):
            out.append((name, dict(zip(_names(protos, name), args))))
    return out


@pytest.mark.parametrize("packed", [False, True], ids=("padded", "packed"))
@pytest.mark.parametrize("bidir", [False, True], ids=("causal", "bidir"))
def test_the_encoder_routes_sliding_layers_past_the_window_to_the_band_entry_points(rec, bidir, packed):
    plm = _tiny(bidir)
    w = plm.config.sliding_window
    assert w == (5 if bidir else 8) and gemma3._layer_types(plm.config) == ["sliding_attention", "sliding_attention", "full_attention"]
    tail = "_varlen" if packed else ""

    def run(longest, band):
        lens = [longest, 2]
        if packed:
            tok = torch.ones(sum(lens), dtype=torch.long)
            pos = torch.cat([torch.arange(n) for n in lens])
            cu = torch.tensor([0, lens[0], sum(lens)], dtype=torch.int32)
            gemma3.gemma3_encode_packed(plm, tok, pos, cu, longest, torch.float32, band=band)
        else:
            gemma3.gemma3_encode(plm, torch.ones(2, longest, dtype=torch.long), torch.tensor(lens, dtype=torch.int32), torch.float32, band=band)
        return _attention_calls(rec)

    plain = [OLD + tail + "_fwd"] * 3
    for band in (False, True):                                         # short: the un-banded entry points, whatever ``band``
        for longest in (w - 1, w):
            calls = run(longest, band)
            assert [n for n, _ in calls] == plain, (band, longest)
            assert all(a["causal"] == (0 if bidir else 1) and "window" not in a for _, a in calls)
    with pytest.raises(ValueError, match=f"sequence length {w + 1} exceeds sliding_window {w}: there is no band kernel at head dim 256"):
        run(w + 1, False)
    rec.take()
    calls = run(w + 1, True)                                           # long, band=True: two sliding layers banded, the full layer not
    assert [n for n, _ in calls] == [STEM + tail + "_fwd"] * 2 + [OLD + tail + "_fwd"]
    for name, a in calls[:2]:
        assert type(a["window"]) is int and a["window"] == w and a["causal"] == (0 if bidir else 1) and a["d"] == 256
        assert a["hq"] == 3 and a["hkv"] == 1 and a["dropout_p"] == 0.0
    assert "window" not in calls[2][1]


def test_the_backward_of_a_banded_layer_calls_the_band_backward(rec):
    plm = _tiny(False)
    ids = torch.ones(1, 12, dtype=torch.long)
    out = gemma3.gemma3_encode(plm, ids, torch.tensor([12], dtype=torch.int32), torch.float32, training=True, band=True)
    rec.take()
    out.sum().backward()
    names = [n for n, _ in _attention_calls(rec)]
    assert names == [OLD + "_bwd"] + [STEM + "_bwd"] * 2               # the layers in reverse: the full layer first


@pytest.mark.parametrize("packed", [True, False], ids=("packed", "padded"))
def test_graphtextlm_forwards_the_attribute_to_the_gemma3_encoder_only(rec, monkeypatch, packed):
    """``encode_texts`` with the encoder functions replaced by stubs that record their keywords: the Gemma3 encoder gets
    ``band = plm_band_attention`` (False unless set), a Llama encoder, whose functions take no such keyword, gets none."""
    import inspect
    import gmlm_amd
    from gmlm_amd import llama
    from transformers import LlamaConfig, LlamaModel
    assert "plm_band_attention" not in inspect.signature(gmlm_amd.GraphTextLM.__init__).parameters
    for name in ("gemma3_encode", "gemma3_encode_packed"):
        assert inspect.signature(getattr(gemma3, name)).parameters["band"].default is False
    seen = []

    def stub(plm, ids, *args, **kw):                                 # [B, L] ids -> [B, L, P]; [T] token ids -> [T, P]
        seen.append(kw)
        return torch.zeros(*ids.shape, plm.config.hidden_size)

    n, width = 4, 6
    lens = torch.tensor([6, 3, 1, 4])
    am = (torch.arange(width)[None, :] < lens[:, None]).long()
    tokens = gmlm_amd.TokenizedTexts.from_mask(torch.ones(n, width, dtype=torch.long) * am, am)
    mask = torch.ones(n, dtype=torch.bool)
    torch.manual_seed(0)
    other = LlamaModel(LlamaConfig(hidden_size=128, num_attention_heads=2, num_key_value_heads=1, intermediate_size=192, num_hidden_layers=2,
                                   vocab_size=96))
    for mod, plm, names, mine in ((gemma3, _tiny(True), ("gemma3_encode", "gemma3_encode_packed"), True),
                                  (llama, other, ("llama_encode", "llama_encode_packed"), False)):
        for name in names:
            monkeypatch.setattr(mod, name, stub)
        model = gmlm_amd.GraphTextLM(12, 16, 3, plm_encoder=plm).eval()
        assert model._enc is mod and model.plm_band_attention is False
        model.plm_packed = packed
        for flag in (False, True):
            model.plm_band_attention = flag
            del seen[:]
            with torch.no_grad():
                model.encode_texts(tokens, mask, plm_batch_size=2)
            assert len(seen) == 2                                        # two micro-batches
            assert all(kw == ({"band": flag} if mine else {}) for kw in seen), (mod.__name__, flag, seen)


# ------------------------------------------------------------------------------------------------- the autograd contract
def b_band(dev="cpu", dt=torch.float32, hq=4, hkv=2, lens=(3, 2), packed=False, causal=True, window=2):
    g = _gen(31)
    shape = (sum(lens),) if packed else (len(lens), max(lens))
    inputs = dict(q=_r(g, *shape, hq * 256, dev=dev, dt=dt), k=_r(g, *shape, hkv * 256, dev=dev, dt=dt, s=1.5),
                  v=_r(g, *shape, hkv * 256, dev=dev, dt=dt))
    if packed:
        cu = _cu(lens, dev)
        return Case(inputs, lambda t: ops.gqa_d256_band_attention_varlen(t["q"], t["k"], t["v"], cu, max(lens), hq, hkv, 0.07, causal, window))
    kl = torch.tensor(lens, dtype=torch.int32, device=dev)
    return Case(inputs, lambda t: ops.gqa_d256_band_attention(t["q"], t["k"], t["v"], kl, hq, hkv, 0.07, causal, window))


def b_rope_band(dev="cpu", dt=torch.float32, hq=2, hkv=1, lens=(3, 2), packed=False, causal=True, window=2):
    g = _gen(32)
    shape = (sum(lens),) if packed else (len(lens), max(lens))
    inputs = dict(qkv=_r(g, *shape, (hq + 2 * hkv) * 256, dev=dev, dt=dt), qw=_r(g, 256, dev=dev, s=0.1), kw=_r(g, 256, dev=dev, s=0.1))
    cs = rope_table(max(lens) + 3, 128, dev)
    if packed:
        cu, pos = _cu(lens, dev), _pos(lens, dev)
        return Case(inputs, lambda t: ops.rope_gqa_d256_varlen(t["qkv"], t["qw"], t["kw"], cs, pos, cu, max(lens), hq, hkv, 0.07, causal,
                                                               window=window))
    kl = torch.tensor(lens, dtype=torch.int32, device=dev)
    return Case(inputs, lambda t: ops.rope_gqa_d256(t["qkv"], t["qw"], t["kw"], cs, kl, hq, hkv, 0.07, causal, window=window))


NODES = {"BandAttention256": b_band, "RopeGQABand256": b_rope_band}


def test_these_are_the_new_nodes_and_they_live_outside_the_scanned_modules():
    import inspect
    mine = {n for n, c in inspect.getmembers(ops_gemma, inspect.isclass)
            if issubclass(c, torch.autograd.Function) and c.__module__ == ops_gemma.__name__}
    assert mine == {"SandwichNorm", "RopeGQA256"} | set(NODES)
    for node, build in NODES.items():
        case = build()
        assert set(case.inputs) and callable(case.call)


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=("fp32", "bf16"))
@pytest.mark.parametrize("causal", [True, False], ids=("causal", "bidir"))
@pytest.mark.parametrize("packed", [False, True], ids=("padded", "packed"))
@pytest.mark.parametrize("node", sorted(NODES))
def test_freeze_patterns_of_the_new_nodes(rec, node, packed, causal, dt):
    case = NODES[node]("cpu", dt, packed=packed, causal=causal)
    failed = []
    for pattern in patterns(case.inputs):
        try:
            rec.take()
            leaves, outs = run_pattern(case, pattern)
            assert outs[0].grad_fn.name().startswith(node + "Backward")
            assert_contract(case, pattern, leaves)
            names = [n for n, _ in rec.take() if n.startswith("gmlm_attention") and not n.endswith("workspace_bytes")]
            tail = "_varlen" if packed else ""
            assert names == [STEM + tail + "_fwd", STEM + tail + "_bwd"], names
        except Exception as e:
            failed.append(f"trainable {pattern}: {type(e).__name__}: {e}")
    assert not failed, f"{node}: {len(failed)} patterns failed:\n  " + "\n  ".join(failed)


def test_window_zero_is_the_existing_node_and_call(rec):
    case = b_rope_band(window=0)
    leaves = {n: v.clone().requires_grad_(True) for n, v in case.inputs.items()}
    out = case.call(leaves)
    assert out.grad_fn.name().startswith("RopeGQA256Backward")
    assert [n for n, _ in rec.take() if n.startswith("gmlm_attention")] == [OLD + "_fwd"]


# ------------------------------------------------------------------------------------------------------ the mask is HF's
@pytest.mark.parametrize("bidir", [False, True], ids=("causal", "bidir"))
def test_hf_mask_is_the_stated_rule(bidir):
    """The ``sliding_attention`` mask as ``Gemma3TextModel.forward`` builds it (transformers' own mask functions), L = 12,
    ``sliding_window`` 4 (causal) and 8 (bidirectional: the config turns it into 5), against
    visible(i, j) = j < kv_len and (0 <= i - j < w if causal else |i - j| < w), element by element: an EXCLUSIVE window."""
    from transformers import Gemma3TextConfig
    from transformers.masking_utils import create_sliding_window_causal_mask
    from transformers.models.gemma3.modeling_gemma3 import _bidirectional_window_overlay
    L = 12
    cfg = Gemma3TextConfig(vocab_size=96, hidden_size=96, intermediate_size=64, num_hidden_layers=3, num_attention_heads=3,
                           num_key_value_heads=1, head_dim=256, max_position_embeddings=64, sliding_window=8 if bidir else 4,
                           sliding_window_pattern=3, pad_token_id=0, use_bidirectional_attention=bidir)
    cfg._attn_implementation = "eager"
    w = cfg.sliding_window
    assert w == (5 if bidir else 4)
    kv = [12, 7]
    attn = (torch.arange(L)[None, :] < torch.tensor(kv)[:, None]).long()
    kwargs = dict(config=cfg, attention_mask=attn, past_key_values=None, position_ids=torch.arange(L)[None].expand(2, -1))
    emb = torch.zeros(2, L, cfg.hidden_size)
    extra = dict(or_mask_function=_bidirectional_window_overlay(w)) if bidir else {}
    mask = create_sliding_window_causal_mask(inputs_embeds=emb, **kwargs, **extra)          # as Gemma3TextModel.forward calls it
    assert mask is not None and tuple(mask.shape) == (2, 1, L, L)
    seen = mask[:, 0] == 0 if mask.dtype != torch.bool else mask[:, 0]
    for b_, n in enumerate(kv):
        for i in range(L):
            for j in range(L):
                rule = j < n and (0 <= i - j < w if not bidir else abs(i - j) < w)
                assert bool(seen[b_, i, j]) == rule, (b_, i, j, w)
    # one step outside the window is invisible, the last step inside is visible: the window is exclusive
    i = 9
    assert bool(seen[0, i, i - (w - 1)]) and not bool(seen[0, i, i - w])
